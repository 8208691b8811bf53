"""k_disc_step4 with the mixup flags on a polling wave of their own (several polls in flight) and LDS status words in place of
the barriers around the two waits: the one-launch step must still give the bits of k_disc_chain4 + k_disc_wgrad -- weights,
both Adam moments and the three loss sums EQUAL -- at the benchmark's geometry (G = 8), with a single row group (G = 1: 4 mixup
and 8 BCE flags, poll waves mostly spare lanes), with a ragged last row group (B = 100) and with more than 64 mixup flags
(B = 272, G = 17: the second trip of the flag loop, more workgroups than the chip holds at once).  A few epochs of 4 steps
each; the flags are monotonic across epochs and across replays of an epoch's graph, which the last test holds to direct
launches."""
import numpy as np
import pytest

from test_gpu_world import Box, Loader

pytestmark = pytest.mark.gpu

F, HD, STEPS, EPOCHS = 86, 100, 4, 3
SLOT_DISC_STEP = 7   # the profiling slot of k_disc_step4 (tests/test_gpu_handoff_error.py: SLOTS)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def _problem(sg, B, seed):
    rng = np.random.default_rng(seed)
    ro = sg.RolloutStorage(STEPS, B, (3,), Box((2,)), 1, F)
    ro.obs_feat.copy_(ro.obs_feat.new_tensor(rng.standard_normal((STEPS + 1, B, F)).astype(np.float32)))
    expert = (rng.standard_normal((STEPS * B, F)) * 0.7 + 0.2).astype(np.float32)
    draws = [dict(expert_perm=rng.permutation(STEPS * B).astype(np.int64), policy_perm=rng.permutation(STEPS * B).astype(np.int64),
                  alpha=rng.random(STEPS * B).astype(np.float32)) for _ in range(EPOCHS)]
    p0 = sg.algo.gail.Discriminator(F, HD, None, seed=seed).get_flat_params()
    return ro, expert, draws, p0


def _epochs(sg, monkeypatch, B, ro, expert, draws, p0, fused, graph=True):
    """EPOCHS epochs of STEPS steps -> per epoch (losses, params, m, v), and whether the one-launch step ran"""
    from simgan_amd import _lib
    monkeypatch.setenv("SG_DISC_CHAIN", "thin")
    monkeypatch.setenv("SG_DISC_FUSED", "1" if fused else "0")
    if graph:
        monkeypatch.delenv("SG_DISC_GRAPH", raising=False)
    else:
        monkeypatch.setenv("SG_DISC_GRAPH", "0")
    D = sg.algo.gail.Discriminator(F, HD, None, seed=1)
    D.set_flat_params(p0)
    out = []
    for kw in draws:
        losses = D.update_gail_dyn(Loader(expert, B), ro, **kw)
        assert D.last_n_steps == STEPS
        m, v, _ = D.get_adam()
        out.append((np.asarray(losses, dtype=np.float64), D.get_flat_params(), m, v))
    # which form ran: one more epoch with the launch counters on (a profiled epoch is issued directly, so it comes last)
    ctx = _lib.Context.default()
    ctx.profile_reset()
    ctx.profile(True)
    D.update_gail_dyn(Loader(expert, B), ro, **draws[0])
    ctx.profile(False)
    return out, ctx.profile_read(SLOT_DISC_STEP)[1]


def _assert_equal(one, two, what):
    for e, (a, b) in enumerate(zip(one, two)):
        for x, y, name in zip(a, b, ("loss sums", "weights", "m", "v")):
            assert x.tobytes() == y.tobytes(), f"{what}, epoch {e}: {name}: {int((x != y).sum())} of {x.size} differ, worst {np.abs(x - y).max():.3g}"
            assert np.isfinite(x).all(), f"{what}, epoch {e}: {name} not finite"


@pytest.mark.parametrize("B", [128, 16, 100, 272], ids=["B128-G8", "B16-G1", "B100-ragged", "B272-G17"])
def test_one_launch_step_keeps_the_two_launch_bits(sg, monkeypatch, B):
    ro, expert, draws, p0 = _problem(sg, B, seed=1000 + B)
    two, n2 = _epochs(sg, monkeypatch, B, ro, expert, draws, p0, fused=False)
    one, n1 = _epochs(sg, monkeypatch, B, ro, expert, draws, p0, fused=True)
    assert n2 == 0 and n1 == STEPS, f"launches of k_disc_step4: {n1} forced on (want {STEPS}), {n2} forced off"
    _assert_equal(one, two, f"B {B}: one launch against two")
    assert np.abs(one[-1][1] - p0).max() > 1e-3


def test_graph_replay_keeps_the_bits_of_direct_launches(sg, monkeypatch):
    """the second and third epoch replay the graph captured in the first: the flags carry the Adam step number, which runs on"""
    B = 128
    ro, expert, draws, p0 = _problem(sg, B, seed=77)
    direct, nd = _epochs(sg, monkeypatch, B, ro, expert, draws, p0, fused=True, graph=False)
    replay, nr = _epochs(sg, monkeypatch, B, ro, expert, draws, p0, fused=True, graph=True)
    assert nd == STEPS and nr == STEPS
    _assert_equal(replay, direct, "graph replay against direct launches")
