"""GPU: PPO's mirror-symmetry loss (a2c/algo/ppo.py:110-143) -- k_ppo_fwd_sym / k_ppo_bwd_sym / k_ppo_reduce_sym -- against the
reference's fixtures (tools/gen_golden_symmetry.py) and against the oracle + float64 restatement of tests/test_symmetry_host.py.
Tolerances: those of test_gpu_parity.py::test_ppo_update_golden."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import assert_close, assert_close_adam, load  # noqa: E402
from test_symmetry_host import mirrored_rows_of, nonlinear_obs, sym_update_restated  # noqa: E402

pytestmark = pytest.mark.gpu


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def _fill(ro, g):
    for name in ("obs", "actions", "value_preds", "returns", "action_log_probs", "masks", "bad_masks", "rewards", "obs_feat"):
        if name in g and getattr(ro, name).numel():
            getattr(ro, name).copy_(getattr(ro, name).new_tensor(np.asarray(g[name], np.float32)))


def _problem(sg, g, mirror_obs, mirror_act, coef=None, ctx=None):
    m = g["meta"]
    kw = {} if ctx is None else {"ctx": ctx}
    p = sg.Policy((m["O"],), Box((m["A"],)), base_kwargs={"recurrent": False, "hidden_size": m["H"]}, **kw)
    p.set_flat_params(g["params0"])
    F = g["obs_feat"].shape[-1] if "obs_feat" in g else 1
    ro = sg.RolloutStorage(m["T"], m["N"], (m["O"],), Box((m["A"],)), 1, F, **kw)
    _fill(ro, g)
    agent = sg.algo.PPO(p, m["clip_param"], m["ppo_epoch"], m["num_mini_batch"], m["value_loss_coef"], m["entropy_coef"],
                        symmetry_coef=m["symmetry_coef"] if coef is None else coef, lr=m["lr"], eps=m["eps"],
                        max_grad_norm=m["max_grad_norm"], mirror_obs=mirror_obs, mirror_act=mirror_act)
    return p, agent, ro


def _row_fn(mat):
    mat = np.asarray(mat, np.float64)
    return lambda x: list(mat @ np.asarray(x, np.float64))


FIXTURE_PATHS = [("ppo_sym_small", "matrix"), ("ppo_sym_small", "callable"), ("ppo_sym_laikago", "matrix"),
                 ("ppo_sym_laikago", "callable"), ("ppo_sym_nonlinear", "callable")]


@pytest.mark.parametrize("name,path", FIXTURE_PATHS)
def test_symmetric_update_matches_the_reference_fixture(sg, name, path):
    g = load(name)
    m = g["meta"]
    if path == "matrix":
        mo, ma = g["m_obs"], g["m_act"]                      # all on the device
    else:
        mo = nonlinear_obs if name == "ppo_sym_nonlinear" else _row_fn(g["m_obs"])
        ma = _row_fn(g["m_act"])                             # probed into its matrix
    p, agent, ro = _problem(sg, g, mo, ma)
    losses = agent.update(ro, perms=g["perms"])
    assert_close(ro.device_advantages(), g["advantages"], rtol=1e-5, what="advantages")
    assert_close(losses, g["losses"], what="ppo losses")
    mm, vv, step = agent.get_adam()
    assert step == m["ppo_epoch"] * m["num_mini_batch"]
    assert_close(mm, g["adam_m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert_close(vv, g["adam_v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close(p.get_flat_params(), g["params1"], what="params after update")
    _, _, _, sym = sym_update_restated(g, mirrored_rows_of(g))
    assert_close(agent.last_symmetry_loss, sym, rtol=1e-4, atol=1e-7, what="symmetry loss")


def _random_problem(O, A, H, T, N, E, M, coef, seed, m_obs, m_act):
    """A fixture-shaped problem on random data: an old policy near the current one, so ratios and clipping are exercised."""
    from oracle import oracle as orc
    rng = np.random.default_rng(seed)
    d = orc.dims(orc.KIND_MLP, O, A, H, 1)
    n = orc.policy_num_params(d)
    pi = (0.15 * rng.standard_normal(n)).astype(np.float32)
    old = (pi + 0.02 * rng.standard_normal(n)).astype(np.float32)
    obs = rng.standard_normal((T + 1, N, O)).astype(np.float32)
    v, a, lp = orc.policy_act(d, old, obs[:-1].reshape(-1, O), rng.standard_normal((T * N, A)).astype(np.float32))
    vp = np.concatenate([np.asarray(v).reshape(T, N, 1), np.zeros((1, N, 1))]).astype(np.float32)
    meta = dict(kind="mlp", O=O, A=A, H=H, T=T, N=N, ppo_epoch=E, num_mini_batch=M, clip_param=0.1, entropy_coef=0.0, lr=1.5e-4,
                eps=1e-5, value_loss_coef=0.5, max_grad_norm=0.5, symmetry_coef=coef)
    return dict(meta=meta, params0=pi, obs=obs, actions=np.asarray(a, np.float32).reshape(T, N, A),
                action_log_probs=np.asarray(lp, np.float32).reshape(T, N, 1), value_preds=vp,
                returns=(vp + 0.5 * rng.standard_normal(vp.shape)).astype(np.float32),
                perms=np.stack([rng.permutation(T * N) for _ in range(E)]).astype(np.int64),
                m_obs=np.asarray(m_obs, np.float32), m_act=np.asarray(m_act, np.float32))


def test_refine_minibatch_single_step_matches_the_restatement(sg):
    """One optimizer step at the refinement workload's minibatch (4096 rows of obs 111, act 12, hidden 64: the specialised
    k_ppo_bwd_sym<2, 7, 4>) with the Laikago mirrors, against the oracle + float64 restatement."""
    from simgan_amd.symmetry import laikago_mirror
    mo, ma = laikago_mirror(111)
    g = _random_problem(111, 12, 64, 16, 256, 1, 1, 1.0, 5, mo, ma)
    p, agent, ro = _problem(sg, g, mo, ma)
    losses = agent.update(ro, perms=g["perms"])
    par, _, want_losses, sym = sym_update_restated(g, mirrored_rows_of(g))
    assert_close(losses, want_losses, what="ppo losses")
    assert_close(agent.last_symmetry_loss, sym, rtol=1e-4, atol=1e-7, what="symmetry loss")
    assert_close_adam(p.get_flat_params(), par, lr=g["meta"]["lr"], steps=1, what="params after one step")


def test_hidden_256_global_weight_instances(sg):
    """A 256-unit policy (trunk larger than LDS: the GW instances of the symmetric step), two epochs, ragged minibatches."""
    rng = np.random.default_rng(2)
    mo = np.linalg.qr(rng.standard_normal((20, 20)))[0]
    ma = np.eye(6)[rng.permutation(6)] * np.where(rng.random(6) < 0.5, -1.0, 1.0)[:, None]
    g = _random_problem(20, 6, 256, 7, 11, 2, 3, 0.7, 9, mo, ma)
    p, agent, ro = _problem(sg, g, g["m_obs"], g["m_act"])
    losses = agent.update(ro, perms=g["perms"])
    par, adam, want_losses, sym = sym_update_restated(g, mirrored_rows_of(g))
    assert_close(losses, want_losses, what="ppo losses")
    assert_close(agent.last_symmetry_loss, sym, rtol=1e-4, atol=1e-7, what="symmetry loss")
    assert_close_adam(p.get_flat_params(), par, lr=g["meta"]["lr"], steps=6, what="params after update")


def test_zero_coefficient_is_plain_ppo_bit_for_bit(sg):
    """symmetry_coef = 0 with mirrors given: the reference skips the loss (a2c/algo/ppo.py:111) -- today's kernels, same bits."""
    g = load("ppo_sym_small")
    p0, a0, r0 = _problem(sg, g, None, None, coef=0.0)
    p1, a1, r1 = _problem(sg, g, g["m_obs"], g["m_act"], coef=0.0)
    l0 = a0.update(r0, perms=g["perms"])
    l1 = a1.update(r1, perms=g["perms"])
    assert l0 == l1
    assert np.array_equal(p0.get_flat_params(), p1.get_flat_params())
    assert a1.last_symmetry_loss == 0.0


@pytest.mark.parametrize("path", ["matrix", "callable"])
def test_graph_replay_is_bit_exact_with_symmetry(sg, monkeypatch, path):
    """Two updates replayed from the captured graph against the same two updates launched kernel by kernel."""
    g = load("ppo_sym_laikago")
    mo = g["m_obs"] if path == "matrix" else _row_fn(g["m_obs"])
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        p, agent, ro = _problem(sg, g, mo, g["m_act"])
        losses = [agent.update(ro, perms=g["perms"]) for _ in range(2)]
        out.append((losses, agent.last_symmetry_loss, p.get_flat_params(), agent.get_adam()[0]))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


def test_callable_mirror_reads_a_device_resident_rollout(sg):
    """A device-resident rollout (the driver's fast path): the callable path downloads obs before mirroring it."""
    g = load("ppo_sym_nonlinear")
    p, agent, ro = _problem(sg, g, nonlinear_obs, _row_fn(g["m_act"]))
    ro.sync_to_device()
    ro.device_resident = True
    ro.obs.zero_()                      # the host view is stale: only the device copy holds the rollout
    agent.update(ro, perms=g["perms"])
    assert_close(p.get_flat_params(), g["params1"], what="params after update")


def test_world_2_matches_world_1(sg):
    """Two ranks over the loopback communicator (each its own columns, injected global permutations) against one rank on the
    concatenated rollout: B is the global minibatch, the mirrored rows are each rank's own."""
    from simgan_amd import _lib
    from test_gpu_world import run_ranks
    from simgan_amd.symmetry import laikago_mirror
    mo, ma = laikago_mirror(37)
    T, N_loc, world = 6, 8, 2
    g = _random_problem(37, 12, 64, T, N_loc * world, 2, 3, 1.0, 21, mo, ma)

    def shard(rank):
        gs = dict(g)
        gs["meta"] = dict(g["meta"], N=N_loc)
        for k in ("obs", "actions", "action_log_probs", "value_preds", "returns"):
            gs[k] = np.ascontiguousarray(g[k][:, rank * N_loc:(rank + 1) * N_loc])
        return gs

    def body(rank, ctx):
        p, agent, ro = _problem(sg, shard(rank), mo, ma, ctx=ctx)
        losses = agent.update(ro, perms=g["perms"])
        return losses, agent.last_symmetry_loss, p.get_flat_params()

    got = run_ranks(world, body)
    ctx1 = _lib.Context(0)
    p1, a1, r1 = _problem(sg, g, mo, ma, ctx=ctx1)
    want = a1.update(r1, perms=g["perms"])
    for losses, sym, par in got:
        assert_close(losses, want, what="ppo losses")
        assert_close(sym, a1.last_symmetry_loss, rtol=1e-4, atol=1e-7, what="symmetry loss")
        assert_close(par, p1.get_flat_params(), what="params after update")
