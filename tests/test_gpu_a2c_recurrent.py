"""GPU: A2C through time -- A2C_ACKTR(..., recurrent=True) / sg_a2c_create_rnn: k_a2c_gru_gather, the GRU scans, k_a2c_bwd_dx,
the accumulate paths of k_a2c_reduce / k_gru_reduce_acc and one k_a2c_rmsprop over heads + GRU -- against the reference-written
fixtures (tools/gen_golden_a2c_recurrent.py), the float64 restatement of tests/a2c_gru_ref.py per parameter block, and autograd.

The one-step gradient is recovered from the optimizer: a first RMSprop step from square_avg = 0 leaves square_avg =
(1 - alpha) g^2, so g = sign(p0 - p1) sqrt(square_avg / (1 - alpha)); the clip is put out of reach for those runs."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import a2c_gru_ref as ref
from helpers import assert_close, load
from test_a2c_recurrent_host import FIXTURES, fixture_updates

pytestmark = pytest.mark.gpu

HP = dict(value_loss_coef=0.5, entropy_coef=0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
NO_CLIP = 1e9
PARITY = {}     # measured per-block errors, printed by the last test (profiles/a2c_rnn_parity.json is written from it)


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def _policy(sg, O, A, H, params, **kw):
    p = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": H}, **kw)
    p.set_flat_params(np.asarray(params, np.float32))
    return p


def _agent(sg, p, **over):
    m = dict(HP, **over)
    return sg.algo.A2C_ACKTR(p, m["value_loss_coef"], m["entropy_coef"], lr=m["lr"], eps=m["eps"], alpha=m["alpha"],
                             max_grad_norm=m["max_grad_norm"], recurrent=True)


def _rollout(sg, c, T, N, O, A, H, hxs0, resident=False, **kw):
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), H, 1, **kw)
    for name in ("obs", "actions", "returns", "masks"):
        getattr(ro, name).copy_(getattr(ro, name).new_tensor(np.asarray(c[name], np.float32)))
    ro.recurrent_hidden_states[0].copy_(ro.obs.new_tensor(np.asarray(hxs0, np.float32)))
    if resident:
        ro.sync_to_device()
        ro.device_resident = True
        ro.enable_device_hidden()
    return ro


def _run(sg, c, updates=1, resident=False, fetch=True, **over):
    """-> (agent, policy, [losses per update]) after `updates` updates on the case's rollout"""
    p = _policy(sg, c["O"], c["A"], c["H"], c["params"])
    agent = _agent(sg, p, **over)
    ro = _rollout(sg, c, c["T"], c["N"], c["O"], c["A"], c["H"], c["hxs0"], resident)
    return agent, p, [agent.update(ro, fetch_losses=fetch) for _ in range(updates)]


def _recovered_gradient(p0, p1, sq, alpha=HP["alpha"]):
    oma = float(np.float32(1.0 - alpha))     # the float the kernel multiplies g^2 by
    return np.sign(np.asarray(p0, np.float64) - np.asarray(p1, np.float64)) * np.sqrt(np.asarray(sq, np.float64) / oma)


def _hold_gradient(sg, c, tag, reference=None):
    g64, l64, worst32 = ref.admitted(c)
    assert worst32 <= 0.5 * ref.RTOL_BLOCK, f"{tag}: the float32 restatement is {worst32:.2e} from float64: not a case"
    want = g64 if reference is None else reference
    agent, p, losses = _run(sg, c, max_grad_norm=NO_CLIP)
    sq, step = agent.get_rmsprop()
    assert step == 1
    got = _recovered_gradient(c["params"], p.get_flat_params(), sq)
    errs = ref.block_errors(got, want, c["O"], c["A"], c["H"])
    PARITY[tag] = dict(worst_block=max(errs, key=errs.get), worst=max(errs.values()), float32_restatement=worst32, blocks=errs)
    print(f"{tag}: worst block {PARITY[tag]['worst_block']} {PARITY[tag]['worst']:.3e} (float32 restatement {worst32:.3e})")
    assert max(errs.values()) <= ref.RTOL_BLOCK, (tag, {k: v for k, v in errs.items() if v > ref.RTOL_BLOCK})
    assert_close(losses[0], l64, what=f"{tag} losses")
    return got


# ------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_update_matches_the_reference_fixture(sg, name):
    from simgan_amd.utils import update_linear_schedule
    g = load(name)
    m = g["meta"]
    p = _policy(sg, m["O"], m["A"], m["H"], g["params0"])
    agent = _agent(sg, p, **{k: m[k] for k in HP})
    for j, (pre, ro_arrays, hxs0, lr) in enumerate(fixture_updates(g)):
        if m["iters"] > 1:
            update_linear_schedule(agent.optimizer, j, m["num_updates"], m["lr"])
            assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(lr)
        ro = _rollout(sg, ro_arrays, m["T"], m["N"], m["O"], m["A"], m["H"], hxs0)
        losses = agent.update(ro)
        assert_close(losses, g[pre + "losses"], what=f"losses {j}")
        sq, step = agent.get_rmsprop()
        assert step == j + 1
        assert_close(sq, g[pre + "square_avg"], rtol=1e-3, atol=1e-12, what=f"square_avg {j}")
        assert_close(p.get_flat_params(), g[pre + "params1"], what=f"params after update {j}")


# ------------------------------------------------------------------------------------------- gradient per block vs float64
@pytest.mark.parametrize("shape", ref.GPU_SHAPES[:5], ids=lambda s: "x".join(map(str, s)))
def test_gradient_per_block_against_float64(sg, shape):
    _hold_gradient(sg, ref.random_case(*shape), "x".join(map(str, shape)))


def test_gradient_in_three_groups_of_16_environments(sg, monkeypatch):
    """(13, 5, 20, 27, 48) again with the group size forced to 16: three groups through both accumulate paths (k_a2c_reduce's and
    k_gru_reduce_acc's), held to float64 like the one-group run -- and 1 / B stays 1 / (T N)."""
    monkeypatch.setenv("SG_A2C_GROUP_ENVS", "16")
    _hold_gradient(sg, ref.random_case(13, 5, 20, 27, 48), "13x5x20x27x48 groups of 16")


def test_gradient_ragged_last_group(sg, monkeypatch):
    """N = 33 in groups of 16: the last group is one environment, its padding rows hold the previous group's gate gradients."""
    monkeypatch.setenv("SG_A2C_GROUP_ENVS", "16")
    _hold_gradient(sg, ref.random_case(13, 5, 20, 9, 33), "13x5x20x9x33 groups of 16")


def test_gradient_with_global_weights(sg, monkeypatch):
    monkeypatch.setenv("SG_POLICY_GW", "1")
    _hold_gradient(sg, ref.random_case(*ref.GPU_SHAPES[5]), "13x5x20x9x33 SG_POLICY_GW=1")


def test_gradient_with_an_environment_that_never_leaves_its_reset(sg):
    shape, env = ref.DEAD_ENV_CASE
    c = ref.random_case(*shape, dead_env=env)
    assert (c["masks"][:, env] == 0).all()
    _hold_gradient(sg, c, "x".join(map(str, shape)) + f" masks of environment {env} all 0")


def test_autograd_anchor(sg):
    """The smallest case held to autograd through torch.nn.GRU directly, not to the restatement."""
    c = ref.random_case(*ref.ANCHOR_SHAPE)
    g_a, l_a = ref.autograd_grad(c["params"], c["O"], c["A"], c["H"], c, c["hxs0"], HP["value_loss_coef"], HP["entropy_coef"])
    _hold_gradient(sg, c, "anchor " + "x".join(map(str, ref.ANCHOR_SHAPE)), reference=g_a)


# ------------------------------------------------------------------------------------------- clip, optimizer state
def test_both_sides_of_the_clip(sg):
    c = ref.random_case(13, 5, 20, 9, 33)
    args = (c["params"], c["O"], c["A"], c["H"], c, c["hxs0"], HP["value_loss_coef"], HP["entropy_coef"], HP["lr"], HP["eps"], HP["alpha"])
    norm = ref.update(*args, NO_CLIP)["norm"]
    for mgn in (0.5 * norm, 2.0 * norm):
        want = ref.update(*args, mgn)
        agent, p, losses = _run(sg, c, max_grad_norm=mgn)
        sq, _ = agent.get_rmsprop()
        assert_close(sq, want["square_avg"], rtol=1e-3, atol=1e-12, what=f"square_avg at max_grad_norm {mgn:.3f} (norm {norm:.3f})")
        assert_close(p.get_flat_params(), want["params"], what="params")
    # the norm covers the GRU block: a norm over the heads alone would leave the clip at 0.9 x norm inactive
    heads = np.sqrt((ref.update(*args, NO_CLIP)["grad"][ref.gru_count(c["O"], c["A"], c["H"]):] ** 2).sum())
    assert heads < norm


def test_three_consecutive_updates(sg):
    c = ref.random_case(11, 3, 32, 8, 17)
    agent, p, losses = _run(sg, c, updates=3)
    params, sq = c["params"], None
    for j in range(3):
        r = ref.update(params, c["O"], c["A"], c["H"], c, c["hxs0"], HP["value_loss_coef"], HP["entropy_coef"], HP["lr"], HP["eps"],
                       HP["alpha"], HP["max_grad_norm"], square_avg=sq)
        assert_close(losses[j], r["losses"], what=f"losses {j}")
        params, sq = r["params"], r["square_avg"]
    got_sq, step = agent.get_rmsprop()
    assert step == 3
    assert_close(got_sq, sq, rtol=1e-3, atol=1e-12, what="square_avg after three updates")
    assert_close(p.get_flat_params(), params, what="params after three updates")


def test_rmsprop_state_round_trip(sg):
    c = ref.random_case(13, 5, 100, 8, 17)      # padded Hp: the GRU block's pad / unpad
    agent, p, _ = _run(sg, c)
    n = p.num_params
    state = (np.arange(1, n + 1, dtype=np.float32) * 1e-6)
    agent.set_rmsprop(state, 7)
    back, step = agent.get_rmsprop()
    assert step == 7 and np.array_equal(back, state)
    from simgan_amd import _lib
    with pytest.raises(_lib.SimganHipError, match="bad length"):
        agent.set_rmsprop(state[ref.gru_count(c["O"], c["A"], c["H"]):], 7)


# ------------------------------------------------------------------------------------------- same bits
def test_same_bits_twice_and_against_direct_launches(sg, monkeypatch):
    c = ref.random_case(11, 3, 16, 130, 32)
    out = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        agent, p, losses = _run(sg, c, updates=2)
        out.append((losses, p.get_flat_params(), agent.get_rmsprop()[0]))
    for other in out[1:]:
        assert out[0][0] == other[0]
        assert np.array_equal(out[0][1], other[1]) and np.array_equal(out[0][2], other[2])


def test_host_rollout_and_device_resident_rollout_give_the_same_bits(sg):
    c = ref.random_case(13, 5, 20, 9, 33)
    a1, p1, l1 = _run(sg, c)
    a2, p2, l2 = _run(sg, c, resident=True)
    assert l1 == l2 and np.array_equal(p1.get_flat_params(), p2.get_flat_params())
    assert np.array_equal(a1.get_rmsprop()[0], a2.get_rmsprop()[0])


def test_queued_update_through_the_learner_matches_the_synchronous_call(sg):
    """driver.PpoLearner with a recurrent A2C agent on a device-resident rollout that holds its hidden states: the update is
    queued (no host wait), its losses come through the results ring; against the same calls made synchronously.  The host-rollout
    mode runs too."""
    from simgan_amd import _lib
    from simgan_amd.driver import PpoLearner
    from simgan_amd.utils import update_linear_schedule
    c = ref.random_case(11, 3, 32, 8, 17)
    rewards = np.random.default_rng(5).standard_normal((c["T"], c["N"], 1)).astype(np.float32)

    def setup(resident):
        p = _policy(sg, c["O"], c["A"], c["H"], c["params"])
        agent = _agent(sg, p)
        ro = sg.RolloutStorage(c["T"], c["N"], (c["O"],), Box((c["A"],)), c["H"], 1)
        for name in ("obs", "actions", "masks"):
            getattr(ro, name).copy_(getattr(ro, name).new_tensor(c[name]))
        ro.rewards.copy_(ro.rewards.new_tensor(rewards))
        hx = np.random.default_rng(6).standard_normal((c["T"] + 1, c["N"], c["H"])).astype(np.float32) * 0.5
        ro.recurrent_hidden_states.copy_(ro.obs.new_tensor(hx))
        if resident:
            ro.sync_to_device()
            ro.device_resident = True
            ro.enable_device_hidden()
        return p, agent, ro

    p1, a1, r1 = setup(True)
    learner = PpoLearner(p1, a1, r1, use_linear_lr_decay=True, lr=HP["lr"], num_updates=10)
    pending = [learner.update() for _ in range(2)]
    ring = [(q["value_loss"], q["action_loss"], q["dist_entropy"]) for q in pending]

    p2, a2, r2 = setup(True)
    sync = []
    for j in range(2):
        update_linear_schedule(a2.optimizer, j, 10, HP["lr"])
        _lib.check(r2.lib.sg_rollout_compute_returns_policy(r2.h, p2.h, 1, 0.99, 0.95, 1))
        sync.append(a2.update(r2))
        r2.after_update()
    assert ring == sync
    assert np.array_equal(p1.get_flat_params(), p2.get_flat_params())
    assert np.array_equal(a1.get_rmsprop()[0], a2.get_rmsprop()[0])

    p3, a3, r3 = setup(False)
    host = PpoLearner(p3, a3, r3).update()
    assert all(np.isfinite(host[k]) for k in ("value_loss", "action_loss", "dist_entropy"))


def test_diagnostics_work_as_on_a_recurrent_ppo_agent(sg):
    c = ref.random_case(11, 3, 16, 5, 4)
    p = _policy(sg, c["O"], c["A"], c["H"], c["params"])
    ro = _rollout(sg, c, c["T"], c["N"], c["O"], c["A"], c["H"], c["hxs0"])
    d_a2c = _agent(sg, p).diagnostics(ro)
    d_ppo = sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5).diagnostics(ro)
    assert d_a2c["clip_fraction"] == 0.0 and d_a2c["rows"] == c["T"] * c["N"]   # clip_param = inf: nothing is clipped
    assert set(d_a2c) == set(d_ppo)
    for k in d_a2c:
        if k != "clip_fraction":
            np.testing.assert_equal(d_a2c[k], d_ppo[k], err_msg=k)


# ------------------------------------------------------------------------------------------- refusals
def test_refusals(sg):
    from simgan_amd import _lib
    from test_gpu_world import run_ranks
    cfg = _lib.A2CConfig(0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5)
    h = _lib.H()
    ff = sg.Policy((11,), Box((3,)), base_kwargs={"recurrent": False, "hidden_size": 16})
    with pytest.raises(_lib.SimganHipError, match="sg_a2c_create_rnn: A2C through time takes a recurrent Policy"):
        _lib.check(ff.lib.sg_a2c_create_rnn(ff.ctx.h, ff.h, C.byref(cfg), C.byref(h)))
    with pytest.raises(ValueError, match="takes a recurrent Policy"):
        sg.algo.A2C_ACKTR(ff, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, recurrent=True)
    p = sg.Policy((11,), Box((3,)), base_kwargs={"recurrent": True, "hidden_size": 16})
    with pytest.raises(NotImplementedError, match="refuses it with acktr"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=True, recurrent=True)
    agent = _agent(sg, p)
    ro = sg.RolloutStorage(2, 6, (11,), Box((3,)), 16, 1)
    with pytest.raises(_lib.SimganHipError, match="sg_ppo_set_hidden_states must hand over"):
        _lib.check(agent.lib.sg_ppo_update(agent.h, ro.h, None, 0, 0, (C.c_float * 3)()))
    agent.update(ro)                                  # the hand-over is consumed by the update ...
    with pytest.raises(_lib.SimganHipError, match="sg_ppo_set_hidden_states must hand over"):
        _lib.check(agent.lib.sg_ppo_update(agent.h, ro.h, None, 0, 0, (C.c_float * 3)()))   # ... and needed again
    with pytest.raises(ValueError, match="recurrent_hidden_states"):
        agent.update(sg.RolloutStorage(2, 6, (11,), Box((3,)), 1, 1))
    n = p.num_params
    mm, vv, step = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int64(0)
    with pytest.raises(_lib.SimganHipError, match="RMSprop"):
        _lib.check(agent.lib.sg_ppo_get_adam(agent.h, _lib.fptr(mm), _lib.fptr(vv), n, C.byref(step)))

    def body(rank, ctx):
        q = sg.Policy((6,), Box((2,)), base_kwargs={"recurrent": True, "hidden_size": 16}, ctx=ctx)
        try:
            sg.algo.A2C_ACKTR(q, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, recurrent=True)
        except _lib.SimganHipError as exc:
            return str(exc)
        return None

    errs = run_ranks(2, body)
    assert all(e is not None and "sg_a2c_create_rnn" in e and "world 2" in e for e in errs), errs


def test_zz_report_measured_errors():
    """Not a check: prints what the gradient tests of this run measured, in the form of profiles/a2c_rnn_parity.json."""
    print("A2C_RNN_PARITY " + json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "blocks"} for k, v in PARITY.items()}))
    if os.environ.get("SG_A2C_RNN_PARITY_OUT"):
        with open(os.environ["SG_A2C_RNN_PARITY_OUT"], "w") as f:
            json.dump(dict(bound=ref.RTOL_BLOCK, measure="max|g_lib - g_f64| / max|g_f64| per parameter block, GRU tensors gate by gate",
                           cases=PARITY), f, indent=1)
