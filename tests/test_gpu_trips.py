"""GPU: capped grids on their second trip.  Four launchers clamp the grid and let a block loop with base += gridDim.x * R; the
rest of the suite sends none of them round a second time with a ragged tile on the later trip:

  B1  sg_gru_forward_launch / k_gru_inproj     2 num_cu blocks of up to 32 rows
  B2  policy_forward_dev / k_policy_forward    4 num_cu blocks of up to 64 rows (it also serves a recurrent policy's heads)
  B3  disc_forward_dev / k_disc_forward        2 num_cu blocks of 32 rows (the buffer descriptor of a ragged tile on trip 2)
  B4  sg_rollout_dup_sym / k_dup_sym           at most 512 blocks over slots * ceil(n / tile_rows) tiles per field

Every case is sized from the cap with num_cu read from the device (sg_ctx_device_info), at the LARGEST tile the launcher can pick,
so the second trip is reached whatever it picks; the grid arithmetic is restated here and asserted.  Widths are small: the row count
is what matters.  References: tests/gru_ref.py, oracle/oracle64.py, the float64 discriminator forward of tests/disc_regimes.py and
tests/dup_sym_ref.py, at the project's tolerances (helpers.RTOL / ATOL)."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import disc_regimes as dr
import dup_sym_ref as ref
import gru_ref
import regimes as rg
from helpers import assert_close

pytestmark = pytest.mark.gpu


class Box:  # duck-typed gym.spaces.Box
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


@pytest.fixture(scope="module")
def num_cu(sg):
    from simgan_amd import _lib
    cu = _lib.Context.default().device_info()[1]
    assert cu >= 2
    return cu


def npv(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def trips(rows, cap_blocks, tile_rows):
    """trips of the busiest block of a grid of min(ceil(rows / tile_rows), cap_blocks) blocks that stride by gridDim.x * tile_rows"""
    tiles = -(-rows // tile_rows)
    return -(-tiles // min(tiles, cap_blocks))


def _launch(monkeypatch, variant, knob="SG_POLICY_GW"):
    for k in ("SG_POLICY_GW", "SG_DISC_GW", "SG_DISC_CHAIN", "SG_DISC_FUSED"):
        monkeypatch.delenv(k, raising=False)
    if variant == "gw":
        monkeypatch.setenv(knob, "1")


# ------------------------------------------------------------------------------------------- B1, and B2's recurrent case
@functools.lru_cache(maxsize=None)
def _gru_problem(T, n):
    """(5, 2, 16) on T * n rows; masks with zeros all along the sequence -> the inputs and gru_ref.evaluate's float64 results"""
    O, A, H = 5, 2, 16
    rng = np.random.default_rng([T, n, 41])
    params = rg._init_params(rng, "gru", O, A, H, 1, 1.0)
    obs = rng.standard_normal((T * n, O)).astype(np.float32)
    hxs = (0.5 * rng.standard_normal((n, H))).astype(np.float32)
    masks = (rng.random((T * n, 1)) > 0.05).astype(np.float32)
    masks[(T - 1) * n] = masks[(T - 1) * n + n - 1] = masks[(T // 2) * n + 1] = 0.0
    action = rng.standard_normal((T * n, A)).astype(np.float32)
    want = gru_ref.evaluate(gru_ref.unflatten(params, O, A, H), obs, hxs, masks, action)
    return params, obs, hxs, masks, action, want


def _check_gru_sequence(sg, T, n):
    O, A, H = 5, 2, 16
    params, obs, hxs, masks, action, (rv, rlp, rent, rh) = _gru_problem(T, n)
    p = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": H})
    p.set_flat_params(params)
    v, lp, ent, h = p.evaluate_actions(obs, hxs, masks, action)
    assert_close(v, rv, what="value")
    assert_close(lp, rlp, what="logp")
    assert_close(float(npv(ent)), rent, what="entropy")
    assert_close(h, rh, what="rnn_hxs")


@pytest.mark.parametrize("variant", ["default", "gw"])
def test_gru_input_projection_on_its_second_trip(sg, monkeypatch, num_cu, variant):
    """T = 129, n = num_cu / 2: just over 2 num_cu * 32 rows (16512 at 256 CUs).  The rows of the last steps -- the second trip of
    every block at the 32-row tile, the third and more at the 16-row one -- hold masks of zero, and every later step reads them
    through the state, so the final state sees a wrong GI row of any trip."""
    _launch(monkeypatch, variant)
    T, n = 129, max(1, num_cu // 2)
    rows = T * n
    assert trips(rows, 2 * num_cu, 32) >= 2 and trips(rows, 2 * num_cu, 16) >= 2
    masks = _gru_problem(T, n)[3]
    assert (masks[2 * num_cu * 32:] == 0).any(), "a zero mask in a row of the second trip"
    _check_gru_sequence(sg, T, n)


def test_recurrent_heads_on_their_second_trip(sg, monkeypatch, num_cu):
    """T = 513, n = num_cu / 2: the heads on h_t take two trips of 4 num_cu 64-row tiles where the input projection takes five."""
    _launch(monkeypatch, "default")
    T, n = 513, max(1, num_cu // 2)
    rows = T * n
    assert trips(rows, 4 * num_cu, 64) >= 2 and trips(rows, 2 * num_cu, 32) >= 5
    _check_gru_sequence(sg, T, n)


# ------------------------------------------------------------------------------------------- B2: the policy forward
HEAD_SHAPES = [("mlp", 5, 2, 8, 1), ("split", 14, 7, 100, 1)]


@functools.lru_cache(maxsize=None)
def _heads_reference(spec, rows):
    from oracle import oracle64 as o64
    kind, O, A, H, f = spec
    rng = np.random.default_rng([rows, O, A, H])
    params = rg._init_params(rng, kind, O, A, H, f, 1.0)
    obs = rng.standard_normal((rows, O)).astype(np.float32)
    action = rng.standard_normal((rows, A)).astype(np.float32)
    noise = rng.standard_normal((rows, A)).astype(np.float32)
    d = o64.dims(o64.KIND_MLP if kind == "mlp" else o64.KIND_SPLIT, O, A, H, f)
    with ThreadPoolExecutor(2) as pool:   # (the arbiter takes seconds on the wide shape: its two passes side by side)
        ev, act = pool.submit(o64.policy_evaluate, d, params, obs, action), pool.submit(o64.policy_act, d, params, obs, noise)
        return params, obs, action, noise, ev.result(), act.result()


@pytest.mark.parametrize("variant", ["default", "gw"])
@pytest.mark.parametrize("spec", HEAD_SHAPES, ids=[f"{s[0]}-{s[1]}x{s[2]}x{s[3]}" for s in HEAD_SHAPES])
def test_policy_forward_on_its_second_trip(sg, monkeypatch, num_cu, spec, variant):
    """4 num_cu * 64 + 37 rows: the last tile is ragged and lies in the second trip at the 64-row tile (and in a later one at the
    32- and 16-row tiles).  evaluate_actions, act with injected noise and get_value against the arbiter, every row."""
    _launch(monkeypatch, variant)
    kind, O, A, H, f = spec
    rows = 4 * num_cu * 64 + 37
    assert all(trips(rows, 4 * num_cu, r) >= 2 and rows % r for r in (16, 32, 64))
    params, obs, action, noise, (rv, rlp, rent), act = _heads_reference(spec, rows)
    av, aa, alp = act[0], act[1], act[2]
    if kind == "split":
        p = sg.SplitPolicy((O,), Box((A,)), base_kwargs={"hidden_size": H, "num_feet": f})
    else:
        p = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H})
    p.set_flat_params(params)
    v, lp, ent, _ = p.evaluate_actions(obs, None, None, action)
    assert_close(v, rv, what="evaluate value")
    assert_close(lp, rlp, what="evaluate logp")
    assert_close(float(npv(ent)), rent, what="entropy")
    v1, a1, lp1, _ = p.act(obs, None, None, noise=noise)
    assert_close(v1, av, what="act value")
    assert_close(a1, aa, what="act action")
    assert_close(lp1, alp, what="act logp")
    assert_close(p.get_value(obs, None, None), av, what="get_value")


# ------------------------------------------------------------------------------------------- B3: the discriminator forward
DISC_SHAPES = [(7, 16), (86, 100)]


def _two_reward_calls(sg, c):
    D = sg.algo.gail.Discriminator(c.F, c.Hd, None)
    assert [(n, tuple(s)) for n, s in D.param_shapes()] == dr.param_shapes(c.F, c.Hd)
    D.set_flat_params(c.params)
    assert D.returns is None
    out = []
    for k in range(2):
        rew, ret = D.predict_reward_combined(c.x[k], c.gamma, c.masks[k], offset=c.offset[k])
        out.append((npv(rew)[:, 0].astype(np.float64), npv(ret)[:, 0].astype(np.float64), npv(D.predict_prob(c.x[k]))[:, 0].astype(np.float64)))
    return out


@pytest.mark.parametrize("variant", ["default", "gw"])
@pytest.mark.parametrize("shape", DISC_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in DISC_SHAPES])
def test_disc_forward_ragged_tile_on_its_second_trip(sg, monkeypatch, num_cu, shape, variant):
    """2 num_cu * 32 + 7 rows: block 0 comes round again for the last tile, whose 7 rows get a shortened buffer descriptor.  The
    assertions of tests/test_gpu_disc_regimes.py::test_rewards_at_logits_of_six_hold_the_plain_contract on every row: reward,
    returns and predict_prob of two consecutive calls (masks of 0 and 1 and an offset in the second) at scale (4, 3), where the
    float32 oracle uses at most 0.29 of the tolerance on these 16391 rows (seeds 0 .. 3, both shapes).
    Not at scale (8, 4): that file's conditioning envelope (C = 2) was fitted on 128-row cases; on 16391 rows of 86 x 100 the float32
    oracle itself uses 0.58 .. 1.78 of it and misses it at 11 of the seeds 0 .. 39 (a logit near 0 that is a cancelling sum of
    a hundred saturated units carries 1e-5 of round-off in any float32 evaluation), so it judges nothing at this row count.  The
    global-weight instance was measured there once: 1 of 16391 rows at 1.10 x the bound (row 4218 of trip 1, logit -0.003,
    |error| 1.18e-5 against ATOL), every row of the ragged tile and of the second trip inside it."""
    _launch(monkeypatch, variant, "SG_DISC_GW")
    n = 2 * num_cu * 32 + 7
    assert trips(n, 2 * num_cu, 32) == 2 and n % 32 == 7
    c = dr.reward_case(*shape, 4.0, 3.0, 0, n)
    want, got = dr.rewards64(c), _two_reward_calls(sg, c)
    for k in range(2):
        assert_close(got[k][0], want[k][0], what=f"{c.tag}: reward, call {k}")
        assert_close(got[k][1], want[k][1], what=f"{c.tag}: returns, call {k}")
        assert_close(got[k][2], want[k][2], what=f"{c.tag}: predict_prob, call {k}")
    assert (c.masks[1] == 0).any() and (c.masks[1] == 1).any()
    assert max(float(np.abs(w[0]).max()) for w in want) > 4.0   # (the rewards do reach the tails that test is about)


# ------------------------------------------------------------------------------------------- B4: the mirrored half
def _dup_sym_tiles(T, n, w, mirrored, slots, budget=65536):
    """sg_rollout_dup_sym's tile arithmetic for one field -> (tile_rows, tiles)"""
    if not mirrored:
        tile_rows = max(1, 1024 // w)
    else:
        spans, mb, row = 8 * w, 4 * w * w, 4 * w
        left = budget - spans - (mb if spans + mb + row <= budget else 0)
        tile_rows = min(left // row, max(1, 2048 // w))
    tile_rows = min(tile_rows, n)
    return tile_rows, slots * -(-n // tile_rows)


def _chunked(fn, m, rows, step=256):
    return np.concatenate([fn(m, rows[i:i + step]) for i in range(0, len(rows), step)])


@pytest.mark.parametrize("kind", ["perm", "dense"])
def test_dup_sym_past_the_grid_cap(sg, kind):
    """T = 128, n = 65, O = feat_len = 111, A = 12 (a Laikago rollout's shape): the mirrored obs field has 129 x 4 = 516 tiles of
    18 rows, the copied feat field 129 x 8 = 1032 of 9 -- both more than the 512 blocks of the grid, so blocks come round again: on
    the mirrored path past its trailing barrier, with `xs` overwritten; on the copy path through its `continue`.  Sentinels in every
    field, as in tests/test_gpu_dup_sym.py::test_kernel_against_the_restatement, with its assertions."""
    from simgan_amd import _lib
    from test_gpu_dup_sym import ATTRS, fields_of
    T, n, O, A = 128, 65, 111, 12
    assert _dup_sym_tiles(T, n, O, True, T + 1) == (18, 516) and _dup_sym_tiles(T, n, O, False, T + 1) == (9, 1032)
    assert _dup_sym_tiles(T, n, A, True, T)[1] <= 512 and _dup_sym_tiles(T, n, 1, False, T + 1)[1] <= 512   # (the other fields: one trip)
    rng = np.random.default_rng(1000 * T + 10 * n + O)
    make = ref.signed_permutation if kind == "perm" else ref.dense
    m_obs, m_act = make(rng, O), make(rng, A)
    ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), 1, O)
    for k in ATTRS:
        t = getattr(ro, k)
        t.copy_(t.new_tensor((rng.standard_normal(tuple(t.shape)) * 3.0 + 40.0).astype(np.float32)))   # sentinels: no zero, no one
    ro.sync_to_device()
    before = fields_of(ro, ATTRS)
    adv0 = npv(ro.device_advantages()).copy()
    _lib.check(ro.lib.sg_rollout_set_mirrors(ro.h, _lib.fptr(m_obs), _lib.fptr(m_act)))
    _lib.check(ro.lib.sg_rollout_dup_sym(ro.h))
    ro.sync_from_device()
    got = fields_of(ro, ATTRS)
    assert np.array_equal(got["returns"], before["returns"])
    assert np.array_equal(npv(ro.device_advantages()), adv0)
    assert np.array_equal(got["value_preds"][T], before["value_preds"][T])
    for k in ATTRS:
        assert np.array_equal(got[k][:, :n], before[k][:, :n]), k
    for k, m in (("obs", m_obs), ("actions", m_act)):
        src = before[k][:, :n].reshape(-1, m.shape[0])
        out = got[k][:, n:].reshape(-1, m.shape[0])
        if kind == "perm":
            bad = np.nonzero((out != _chunked(ref.mirror, m, src)).any(axis=1))[0]
            assert bad.size == 0, (k, f"{bad.size} rows differ, the first (slot, row) = {divmod(int(bad[0]), n)}")
        else:
            err = np.abs(out.astype(np.float64) - _chunked(ref.mirror64, m, src))
            bound = _chunked(ref.mirror_bound, m, src)
            assert np.all(err <= bound), (k, float(err.max()), f"first (slot, row) = {divmod(int(np.nonzero((err > bound).any(axis=1))[0][0]), n)}")
    for k, slots in (("obs_feat", T + 1), ("masks", T + 1), ("bad_masks", T + 1), ("rewards", T), ("action_log_probs", T), ("value_preds", T)):
        assert np.array_equal(got[k][:slots, n:], before[k][:slots, :n]), k
