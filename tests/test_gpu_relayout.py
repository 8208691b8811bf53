"""GPU: ONE learner object fed rollouts of different geometry.  Between such updates the object grows its scratch buffers,
clears them for the new layout and captures its graph again (csrc/sg_ppo.hip); every other test builds a fresh agent per
rollout, so that path runs there only once per object.

Every case runs a sequence of updates on one agent and compares it, after every update, with the same sequence on fresh
handles: a new agent object before every update, the optimizer state carried over through get_adam / set_adam (get_rmsprop /
set_rmsprop).  Same kernels on the same numbers in the same order: losses, parameters and optimizer state must be EQUAL.  The
minibatches (20 and 54 rows) are no multiples of the 16-row tile, so the row tiles have padding rows and anything stale left in
the scratch by the other geometry would show.  ACKTR has no state setter: there the graph path is compared with direct launches."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

O, A, H, N, M, E = 11, 3, 64, 4, 2, 2
T_A, T_B = 10, 27          # 20-row and 54-row optimizer steps; B makes every scratch buffer grow
SEQ = "ABAA"               # grow at the second update, a new layout without reallocation at the third, a replay at the fourth


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def world():
    import simgan_amd as sg
    from simgan_amd import _lib
    lib = _lib.load()
    pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H}, seed=3)
    ros = {}
    for name, T, seed in (("A", T_A, 5), ("B", T_B, 6)):
        ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 4)
        ro.device_resident = True
        _lib.check(lib.sg_rollout_fill_synthetic(ro.h, pol.h, seed, 0.05))
        _lib.check(lib.sg_rollout_compute_returns_policy(ro.h, pol.h, 1, 0.99, 0.95, 1))
        ro.sync_from_device()
        ros[name] = ro
    rng = np.random.default_rng(41)
    # off the behaviour policy, so that ratios leave 1
    p0 = (pol.get_flat_params() + 0.01 * rng.standard_normal(pol.num_params)).astype(np.float32)
    return dict(sg=sg, lib=lib, _lib=_lib, ros=ros, p0=p0)


def _policy(sg, p0):
    pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H}, seed=3)
    pol.set_flat_params(p0)
    return pol


def _assert_same(one, fresh, what):
    assert len(one) == len(fresh)
    for i, (a, b) in enumerate(zip(one, fresh)):
        for x, y, name in zip(a, b, ("losses", "parameters", "optimizer state", "optimizer state (2)", "steps")):
            x, y = np.asarray(x), np.asarray(y)
            assert np.array_equal(x, y), f"{what}, update {i} ({name}): {(x != y).sum()} of {x.size} values differ"


def _ppo_perms(rng, T):
    return np.stack([rng.permutation(T * N) for _ in range(E)]).astype(np.int64)


def _ppo_agent(sg, pol):
    return sg.algo.PPO(pol, 0.2, E, M, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)


def _ppo_trajectory(world, steps, fresh, before=lambda agent, step: None):
    """steps: [(rollout, perms, tag)]; before(agent, tag) prepares the agent for the step (the symmetry toggle)."""
    sg = world["sg"]
    pol = _policy(sg, world["p0"])
    agent, state, out = None, None, []
    for ro, perms, tag in steps:
        if fresh or agent is None:
            agent = _ppo_agent(sg, pol)
            if state is not None:
                agent.set_adam(*state)
        before(agent, tag)
        losses = agent.update(ro, perms=perms)
        state = agent.get_adam()
        out.append((np.asarray(losses, np.float64), pol.get_flat_params(), state[0], state[1], state[2]))
    return out


def test_ppo_one_agent_across_rollout_geometries(world):
    rng = np.random.default_rng(1)
    steps = [(world["ros"][k], _ppo_perms(rng, T_A if k == "A" else T_B), k) for k in SEQ]
    one = _ppo_trajectory(world, steps, fresh=False)
    _assert_same(one, _ppo_trajectory(world, steps, fresh=True), "PPO")
    assert one[-1][4] == len(SEQ) * E * M and np.abs(one[-1][1] - world["p0"]).max() > 1e-3


def test_ppo_one_agent_with_the_symmetry_loss_toggled(world):
    """plain, symmetric, plain at one geometry: the symmetric step has a third grid column (more slabs, a third stack set, the
    mirrored epoch copy), so the toggle changes the scratch layout both ways."""
    _lib, lib = world["_lib"], world["lib"]
    rng = np.random.default_rng(2)
    m_obs = np.zeros((O, O), np.float32)
    m_obs[np.arange(O), rng.permutation(O)] = rng.choice([-1.0, 1.0], O)
    m_act = np.zeros((A, A), np.float32)
    m_act[np.arange(A), [1, 0, 2]] = [1.0, 1.0, -1.0]

    def toggle(agent, tag):
        if tag == "sym":
            _lib.check(lib.sg_ppo_set_symmetry(agent.h, 0.7, _lib.fptr(m_obs), _lib.fptr(m_act)))
        else:
            _lib.check(lib.sg_ppo_set_symmetry(agent.h, 0.0, None, None))

    steps = [(world["ros"]["A"], _ppo_perms(rng, T_A), tag) for tag in ("plain", "sym", "plain")]
    one = _ppo_trajectory(world, steps, fresh=False, before=toggle)
    _assert_same(one, _ppo_trajectory(world, steps, fresh=True, before=toggle), "PPO with the symmetry loss toggled")
    plain = _ppo_trajectory(world, steps, fresh=False)
    assert not np.array_equal(one[1][1], plain[1][1]), "the symmetry loss did not act"


def test_a2c_one_agent_across_rollout_geometries(world):
    sg = world["sg"]

    def run(fresh):
        pol = _policy(sg, world["p0"])
        agent, state, out = None, None, []
        for k in SEQ:
            if fresh or agent is None:
                agent = sg.algo.A2C_ACKTR(pol, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
                if state is not None:
                    agent.set_rmsprop(*state)
            losses = agent.update(world["ros"][k])
            state = agent.get_rmsprop()
            out.append((np.asarray(losses, np.float64), pol.get_flat_params(), state[0], state[1]))
        return out

    one = run(False)
    _assert_same(one, run(True), "A2C")
    assert one[-1][3] == len(SEQ) and np.abs(one[-1][1] - world["p0"]).max() > 1e-4


def test_recurrent_ppo_one_agent_across_rollout_geometries(world):
    sg = world["sg"]
    Hg = 32
    rng = np.random.default_rng(3)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    npv = lambda t: t.numpy() if hasattr(t, "numpy") else np.asarray(t)  # noqa: E731

    def gru_policy():
        return sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": Hg}, seed=7)

    behaviour = gru_policy()
    ros = {}
    for name, T in (("A", T_A), ("B", T_B)):
        ro = sg.RolloutStorage(T, N, (O,), Box((A,)), Hg, 1)
        ro.obs.copy_(ro.obs.new_tensor(f(T + 1, N, O)))
        masks = (rng.random((T + 1, N, 1)) > 0.08).astype(np.float32)
        masks[T // 2, 0] = 0.0
        ro.masks.copy_(ro.obs.new_tensor(masks))
        ro.recurrent_hidden_states[0].copy_(ro.obs.new_tensor(0.5 * f(N, Hg)))
        for step in range(T):
            v, a, lp, h = behaviour.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step], noise=f(N, A))
            ro.actions[step].copy_(a); ro.action_log_probs[step].copy_(lp); ro.value_preds[step].copy_(v)
            ro.recurrent_hidden_states[step + 1].copy_(h)
        ro.returns.copy_(ro.obs.new_tensor((npv(ro.value_preds) + 0.5 * f(T + 1, N, 1)).astype(np.float32)))
        ros[name] = ro
    p0 = (behaviour.get_flat_params() + 0.02 * rng.standard_normal(behaviour.num_params)).astype(np.float32)
    perms = [np.stack([rng.permutation(N) for _ in range(E)]).astype(np.int64) for _ in SEQ]

    def run(fresh):
        pol = gru_policy()
        pol.set_flat_params(p0)
        agent, state, out = None, None, []
        for k, pm in zip(SEQ, perms):
            if fresh or agent is None:
                agent = _ppo_agent(sg, pol)
                if state is not None:
                    agent.set_adam(*state)
            losses = agent.update(ros[k], perms=pm)   # (hands the hidden states of slot 0 over before the update)
            state = agent.get_adam()
            out.append((np.asarray(losses, np.float64), pol.get_flat_params(), state[0], state[1], state[2]))
        return out

    one = run(False)
    _assert_same(one, run(True), "recurrent PPO")
    assert one[-1][4] == len(SEQ) * E * M and np.abs(one[-1][1] - p0).max() > 1e-3


def test_acktr_one_agent_across_rollout_geometries_graph_vs_direct(world):
    sg, _lib = world["sg"], world["_lib"]
    rng = np.random.default_rng(4)
    noise = [rng.standard_normal((T_A if k == "A" else T_B, N, 1)).astype(np.float32) for k in SEQ]
    assert "SG_PPO_GRAPH" not in os.environ

    def run(graph):
        pol = _policy(sg, world["p0"])
        agent = sg.algo.A2C_ACKTR(pol, 0.5, 0.01, acktr=True)
        out = []
        if not graph:
            os.environ["SG_PPO_GRAPH"] = "0"
        try:
            for k, eps in zip(SEQ, noise):
                losses = agent.update(world["ros"][k], value_noise=eps)
                st = agent.get_kfac()
                out.append((np.asarray(losses, np.float64), pol.get_flat_params(), np.concatenate([x.ravel() for x in st["m_aa"] + st["m_gg"]]),
                            st["momentum_buffer"], st["steps"]))
        finally:
            os.environ.pop("SG_PPO_GRAPH", None)
        state = (C.c_int * 2)()
        _lib.check_test(_lib.load_test().sg_test_graph_state(agent.h, None, state))
        return out, state[0]

    with_graph, s_graph = run(True)
    direct, s_direct = run(False)
    assert (s_graph, s_direct) == (1, 0), (s_graph, s_direct)
    _assert_same(with_graph, direct, "ACKTR, graph vs direct launches")
    assert with_graph[-1][4] == len(SEQ) and np.abs(with_graph[-1][1] - world["p0"]).max() > 1e-4
