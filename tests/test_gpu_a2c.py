"""GPU: A2C_ACKTR(acktr=False) -- k_a2c_gather, k_ppo_fwd, k_a2c_bwd, k_a2c_reduce, k_a2c_rmsprop -- against the reference's
fixtures (tools/gen_golden_a2c.py) and against the float64 restatement of tests/test_a2c_host.py at shapes too big for a
fixture; graph replay, the driver's results ring and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import assert_close, assert_close_adam, load  # noqa: E402
from test_a2c_host import a2c_update_restated  # noqa: E402

pytestmark = pytest.mark.gpu


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def _policy(sg, O, A, H, Hc, params, ctx=None):
    kw = {} if ctx is None else {"ctx": ctx}
    p = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H}, **kw)
    if Hc != H:
        p.reset_critic((O,))            # a2c/main.py:85: the 64-unit critic (before the agent holds the handle)
    p.set_flat_params(params)
    return p


def _rollout(sg, T, N, O, A, obs, actions, returns, ctx=None):
    kw = {} if ctx is None else {"ctx": ctx}
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 1, **kw)
    for name, arr in (("obs", obs), ("actions", actions), ("returns", returns)):
        getattr(ro, name).copy_(getattr(ro, name).new_tensor(np.asarray(arr, np.float32)))
    return ro


def _agent(sg, p, m, lr=None):
    return sg.algo.A2C_ACKTR(p, m["value_loss_coef"], m["entropy_coef"], lr=m["lr"] if lr is None else lr, eps=m["eps"],
                             alpha=m["alpha"], max_grad_norm=m["max_grad_norm"])


@pytest.mark.parametrize("name", ["a2c_tiny", "a2c_default", "a2c_critic64"])
def test_a2c_update_matches_the_reference_fixture(sg, name):
    g = load(name)
    m = g["meta"]
    p = _policy(sg, m["O"], m["A"], m["H"], m["Hc"], g["params0"])
    agent = _agent(sg, p, m)
    ro = _rollout(sg, m["T"], m["N"], m["O"], m["A"], g["obs"], g["actions"], g["returns"])
    losses = agent.update(ro)
    assert_close(losses, g["losses"], what="losses")
    sq, step = agent.get_rmsprop()
    assert step == 1
    assert_close(sq, g["square_avg"], rtol=1e-3, atol=1e-12, what="square_avg")
    assert_close(p.get_flat_params(), g["params1"], what="params after update")


def test_a2c_three_updates_with_linear_lr_decay_match_the_reference(sg):
    """a2c_multi: square_avg carried across updates, update_linear_schedule writing param_groups[0]['lr'] in between."""
    from simgan_amd.utils import update_linear_schedule
    g = load("a2c_multi")
    m = g["meta"]
    p = _policy(sg, m["O"], m["A"], m["H"], m["Hc"], g["it0_params0"])
    agent = _agent(sg, p, m)
    for j in range(m["iters"]):
        update_linear_schedule(agent.optimizer, j, m["num_updates"], m["lr"])
        assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(g["lrs"][j])
        p.set_flat_params(g[f"it{j}_params0"])   # the fixture perturbs the policy after every rollout
        ro = _rollout(sg, m["T"], m["N"], m["O"], m["A"], g[f"it{j}_obs"], g[f"it{j}_actions"], g[f"it{j}_returns"])
        losses = agent.update(ro)
        assert_close(losses, g[f"it{j}_losses"], what=f"losses {j}")
        sq, step = agent.get_rmsprop()
        assert step == j + 1
        assert_close(sq, g[f"it{j}_square_avg"], rtol=1e-3, atol=1e-12, what=f"square_avg {j}")
        assert_close(p.get_flat_params(), g[f"it{j}_params1"], what=f"params after update {j}")


def _random_case(O, A, H, T, N, seed):
    rng = np.random.default_rng(seed)
    from test_a2c_host import policy_slices
    _, n = policy_slices(O, A, H, H)
    params = (0.2 * rng.standard_normal(n) / np.sqrt(max(O, H))).astype(np.float32)
    params[-A:] = -0.5 + 0.1 * rng.standard_normal(A)                     # log-std
    obs = rng.standard_normal((T + 1, N, O)).astype(np.float32)
    actions = rng.standard_normal((T, N, A)).astype(np.float32)
    returns = (0.5 * rng.standard_normal((T + 1, N, 1))).astype(np.float32)
    return params, obs, actions, returns


# (O, A, H, T, N): the north-star rollout (16 chunks of 4096 rows, the specialised k_a2c_bwd<2, 3, 4>), the Hopper scripts'
# T=1000 x N=8 (two chunks, the second partial), a partial row tile (65 rows), hidden 256 (the global-weight instances)
SHAPES = [(47, 12, 64, 128, 512), (47, 12, 64, 1000, 8), (47, 12, 64, 5, 13), (20, 6, 256, 7, 11)]


@pytest.mark.parametrize("O,A,H,T,N", SHAPES)
def test_a2c_update_matches_the_restatement(sg, O, A, H, T, N):
    params, obs, actions, returns = _random_case(O, A, H, T, N, seed=O + H + T + N)
    lr = 7e-4
    m = dict(value_loss_coef=0.5, entropy_coef=0.01, lr=lr, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    p = _policy(sg, O, A, H, H, params)
    agent = _agent(sg, p, m)
    ro = _rollout(sg, T, N, O, A, obs, actions, returns)
    losses = agent.update(ro)
    want_p, want_sq, want_l = a2c_update_restated(params, np.zeros_like(params), obs, actions, returns, (O, A, H, H), 0.5, 0.01,
                                                  lr, 1e-5, 0.99, 0.5)
    assert_close(losses, want_l, what="losses")
    sq, _ = agent.get_rmsprop()
    assert_close(sq, want_sq, rtol=1e-3, atol=1e-12, what="square_avg")
    assert_close_adam(p.get_flat_params(), want_p, lr=lr, steps=1, what="params after update")


def test_graph_replay_is_bit_exact(sg, monkeypatch):
    """Two updates from identical state replayed from the captured graph against the same two launched kernel by kernel."""
    params, obs, actions, returns = _random_case(47, 12, 64, 40, 128, seed=3)   # 5120 rows: two chunks
    m = dict(value_loss_coef=0.5, entropy_coef=0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        p = _policy(sg, 47, 12, 64, 64, params)
        agent = _agent(sg, p, m)
        ro = _rollout(sg, 40, 128, 47, 12, obs, actions, returns)
        losses = [agent.update(ro) for _ in range(2)]
        out.append((losses, p.get_flat_params(), agent.get_rmsprop()[0]))
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_ppo_learner_results_ring_matches_the_synchronous_call(sg):
    """driver.PpoLearner with an A2C agent on a device-resident rollout (the update is queued, its losses come through the
    results ring) against the same calls made synchronously; and the host-rollout mode runs."""
    from simgan_amd import _lib
    from simgan_amd.driver import PpoLearner
    T, N, O, A, H = 5, 16, 47, 12, 64
    params, obs, actions, _ = _random_case(O, A, H, T, N, seed=11)
    rng = np.random.default_rng(12)
    rewards = rng.standard_normal((T, N, 1)).astype(np.float32)
    m = dict(value_loss_coef=0.5, entropy_coef=0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)

    def setup(resident):
        p = _policy(sg, O, A, H, H, params)
        agent = _agent(sg, p, m)
        ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 1)
        ro.obs.copy_(ro.obs.new_tensor(obs))
        ro.actions.copy_(ro.actions.new_tensor(actions))
        ro.rewards.copy_(ro.rewards.new_tensor(rewards))
        if resident:
            ro.sync_to_device()
            ro.device_resident = True
        return p, agent, ro

    p1, a1, r1 = setup(True)
    learner = PpoLearner(p1, a1, r1, use_linear_lr_decay=True, lr=m["lr"], num_updates=10)
    pending = [learner.update() for _ in range(2)]
    ring = [(q["value_loss"], q["action_loss"], q["dist_entropy"]) for q in pending]

    p2, a2, r2 = setup(True)
    sync = []
    from simgan_amd.utils import update_linear_schedule
    for j in range(2):
        update_linear_schedule(a2.optimizer, j, 10, m["lr"])
        _lib.check(r2.lib.sg_rollout_compute_returns_policy(r2.h, p2.h, 1, 0.99, 0.95, 1))
        sync.append(a2.update(r2))
        r2.after_update()
    assert ring == sync
    assert np.array_equal(p1.get_flat_params(), p2.get_flat_params())

    p3, a3, r3 = setup(False)
    host = PpoLearner(p3, a3, r3).update()
    assert all(np.isfinite(host[k]) for k in ("value_loss", "action_loss", "dist_entropy"))


def test_refusals(sg):
    """SplitPolicy, acktr=True, a world-2 context and Adam access on an A2C handle are refused with their own errors."""
    from simgan_amd import _lib
    from test_gpu_world import run_ranks
    m = dict(value_loss_coef=0.5, entropy_coef=0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    sp = sg.SplitPolicy((20,), Box((7,)), base_kwargs={"hidden_size": 32, "num_feet": 1})
    with pytest.raises(NotImplementedError, match="SplitPolicy"):
        sg.algo.A2C_ACKTR(sp, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    cfg = _lib.A2CConfig(0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5)
    h = _lib.H()
    with pytest.raises(_lib.SimganHipError, match="SplitPolicy"):   # the C ABI refuses it too
        _lib.check(sp.lib.sg_a2c_create(sp.ctx.h, sp.h, C.byref(cfg), C.byref(h)))
    p = sg.Policy((6,), Box((2,)), base_kwargs={"hidden_size": 16})
    with pytest.raises(NotImplementedError, match="K-FAC"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, acktr=True)
    agent = _agent(sg, p, m)
    n = p.num_params
    mm, vv, step = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int64(0)
    with pytest.raises(_lib.SimganHipError, match="RMSprop"):
        _lib.check(agent.lib.sg_ppo_get_adam(agent.h, _lib.fptr(mm), _lib.fptr(vv), n, C.byref(step)))
    with pytest.raises(_lib.SimganHipError, match="A2C"):
        _lib.check(agent.lib.sg_ppo_set_symmetry(agent.h, 1.0, None, _lib.fptr(np.eye(2, dtype=np.float32))))

    def body(rank, ctx):
        q = sg.Policy((6,), Box((2,)), base_kwargs={"hidden_size": 16}, ctx=ctx)
        try:
            sg.algo.A2C_ACKTR(q, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
        except _lib.SimganHipError as exc:
            return str(exc)
        return None

    errs = run_ranks(2, body)
    assert all(e is not None and "world 2" in e for e in errs), errs
