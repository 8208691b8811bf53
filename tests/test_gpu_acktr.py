"""GPU: A2C_ACKTR(acktr=True) -- A2C's gradient kernels, k_acktr_fisher, k_kfac_stats, k_kfac_fold, k_kfac_eig, k_kfac_gemm,
k_kfac_step -- against the reference's fixtures (tools/gen_golden_acktr.py: its float32 run and its float64 run) and against
the float64 restatement of tests/test_acktr_host.py at shapes too big for a fixture; the eigensolver on its own; graph replay,
the driver's results ring, the library's own value noise and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import load  # noqa: E402
import acktr_regimes as ar  # noqa: E402
from test_acktr_host import ACKTR_CASES, acktr_update_restated, dims_of, new_state, rel_l2, restate_fixture  # noqa: E402
from test_a2c_host import policy_slices  # noqa: E402

pytestmark = pytest.mark.gpu
DP_TOL = 2e-4


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
        p.reset_critic((O,))
    p.set_flat_params(params)
    return p


def _rollout(sg, T, N, O, A, obs, actions, returns):
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 1)
    for name, arr in (("obs", obs), ("actions", actions), ("returns", returns)):
        getattr(ro, name).copy_(getattr(ro, name).new_tensor(np.asarray(arr, np.float32)))
    return ro


def _agent(sg, p, seed=0):
    return sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=True, seed=seed)   # a2c/main.py:159-161


def _flat_factors(k):
    return (np.concatenate([m.reshape(-1) for m in k["m_aa"]]), np.concatenate([m.reshape(-1) for m in k["m_gg"]]))


def _fixture_factors(m_aa, m_gg, dims):
    """a fixture's packed m_aa / m_gg (13 modules) -> the 12 distinct factors"""
    O, A, H, Hc = dims
    aa, gg, ia, ig = [], [], 0, 0
    for o, i in ((H, O), (H, 1), (H, H), (H, 1), (Hc, O), (Hc, 1), (Hc, Hc), (Hc, 1), (1, Hc), (1, 1), (A, H), (A, 1), (A, 1)):
        aa.append(m_aa[ia:ia + i * i].reshape(i, i))
        gg.append(m_gg[ig:ig + o * o].reshape(o, o))
        ia, ig = ia + i * i, ig + o * o
    return ar.distinct_factors(aa, gg)


@pytest.mark.parametrize("name", ACKTR_CASES)
def test_acktr_updates_match_the_reference_fixture(sg, name):
    """Every update of the fixture: losses, the running factors, and Delta p against the reference's float64 and float32 runs.
    Then the measures of tests/test_gpu_acktr_regimes.py against the fixture's float64 run (the restatement, which reproduces it
    to 1e-10): each distinct factor relative to its own Frobenius norm, every module's block of the momentum buffer and of Delta p,
    each within F x (the reference's own float32 run's distance) + FLOOR, and within DP_TOL wherever that float32 run is within
    acktr_regimes.COND itself (its Delta p is not on dist.logstd, up to 3.6e-4: the step there is 1e-4 of the parameter, at
    float32's resolution of it)."""
    from test_gpu_acktr_regimes import F, FLOOR, _record, judge
    rec, all_fails = {"case": f"fixture {name}: the float32 column is the reference's own float32 run", "updates": []}, []
    g = load(name)
    m = g["meta"]
    O, A, H, Hc = dims_of(m)
    ref64 = restate_fixture(g)
    p = _policy(sg, O, A, H, Hc, g["it0_params0"])
    agent = _agent(sg, p)
    for j in range(m["iters"]):
        pre = f"it{j}_"
        if m.get("lr_sched"):   # a2c/main.py:203-205 writes lr; K-FAC never reads it
            from simgan_amd.utils import update_linear_schedule
            update_linear_schedule(agent.optimizer, j, m["num_updates"], 0.25)
        p.set_flat_params(g[pre + "params0"])
        ro = _rollout(sg, m["T"], m["N"], O, A, g[pre + "obs"], g[pre + "actions"], g[pre + "returns"])
        losses = agent.update(ro, value_noise=g[pre + "eps"])
        assert np.allclose(losses, g[pre + "losses"], rtol=1e-5, atol=1e-6), (j, losses, g[pre + "losses"])
        k = agent.get_kfac()
        assert k["steps"] == j + 1
        aa, gm = _flat_factors(k)
        for mine, ref, what in ((aa, g[pre + "m_aa"], "m_aa"), (gm, g[pre + "m_gg"], "m_gg")):
            err = np.max(np.abs(mine - ref))
            assert err <= 1e-5 * np.max(np.abs(ref)), (j, what, err)
        p0 = g[pre + "params0"].astype(np.float64)
        dp = p.get_flat_params().astype(np.float64) - p0
        e64 = rel_l2(dp, g[pre + "params1_f64"] - p0)
        e32 = rel_l2(dp, g[pre + "params1"] - p0)
        assert e64 <= DP_TOL and e32 <= DP_TOL, (j, e64, e32)
        p1_64, _, st64 = ref64[j]
        dims = (O, A, H, Hc)
        f64 = [np.asarray(x) for x in st64["mA"] + st64["mG"]]
        hip = {"factors": ar.factor_distances(ar.distinct_factors(k["m_aa"], k["m_gg"]), f64),
               "nuv": ar.block_distances(k["momentum_buffer"], st64["buf"], dims), "dp": ar.block_distances(dp, p1_64 - p0, dims)}
        o32 = {"factors": ar.factor_distances(_fixture_factors(g[pre + "m_aa"], g[pre + "m_gg"], dims), f64),
               "nuv": ar.block_distances(g[pre + "momentum"], st64["buf"], dims),
               "dp": ar.block_distances(g[pre + "params1"].astype(np.float64) - p0, p1_64 - p0, dims)}
        fails = [f"{kind} {b}: HIP {x:.3e}, the reference's float32 run {o32[kind][b]:.3e}" for kind, d in hip.items() for b, x in d.items()
                 if not (x <= F * o32[kind][b] + FLOOR[kind] and (x <= DP_TOL or o32[kind][b] > ar.COND))]
        print(f"{name} update {j}: largest HIP distances", {kind: f"{max(d.values()):.2e}" for kind, d in hip.items()},
              "float32 run", {kind: f"{max(d.values()):.2e}" for kind, d in o32.items()})
        _, ratio, at = judge(name, hip, o32)
        rec["updates"].append({"hip_vs_f64": hip, "float32_vs_f64": o32, "worst_ratio": ratio, "worst_ratio_at": at, "worst_hip": ar.worst(hip)})
        all_fails += [(j, x) for x in fails]
    _record("fixture_" + name, rec)
    assert not all_fails, all_fails
    assert agent.optimizer.lr == 0.25


def _random_case(O, A, H, T, N, seed):
    rng = np.random.default_rng(seed)
    _, n = policy_slices(O, A, H, H)
    params = (0.2 * rng.standard_normal(n) / np.sqrt(max(O, H))).astype(np.float32)
    params[-A:] = -0.5 + 0.1 * rng.standard_normal(A)
    obs = rng.standard_normal((T + 1, N, O)).astype(np.float32)
    actions = rng.standard_normal((T, N, A)).astype(np.float32)
    returns = (0.5 * rng.standard_normal((T + 1, N, 1))).astype(np.float32)
    eps = rng.standard_normal((T, N, 1)).astype(np.float32)
    return params, obs, actions, returns, eps


# the north-star rollout (16 chunks), the Hopper scripts' T=1000 x N=8 (a partial second chunk), obs 150 / hidden 256 (the
# global-weight A2C instances and the eigensolver's global-memory path)
SHAPES = [(47, 12, 64, 128, 512), (47, 12, 64, 1000, 8), (150, 8, 256, 5, 13)]


@pytest.mark.parametrize("O,A,H,T,N", SHAPES)
def test_acktr_updates_match_the_restatement(sg, O, A, H, T, N):
    params, obs, actions, returns, eps = _random_case(O, A, H, T, N, seed=O + H + T + N)
    p = _policy(sg, O, A, H, H, params)
    agent = _agent(sg, p)
    ro = _rollout(sg, T, N, O, A, obs, actions, returns)
    st = new_state()
    cur = params
    for j in range(2):
        losses = agent.update(ro, value_noise=eps * (1 + j))
        want, want_l, st = acktr_update_restated(cur, st, obs, actions, returns, eps * (1 + j), (O, A, H, H), 0.5, 0.01)
        got = p.get_flat_params()
        assert np.allclose(losses, want_l, rtol=1e-5, atol=1e-6), (j, losses, want_l)
        err = rel_l2(got.astype(np.float64) - cur, want - cur)
        assert err <= DP_TOL, (j, err)
        cur = got.astype(np.float64)
        p.set_flat_params(got)


def _matrices(n, rng):
    X = rng.standard_normal((2 * n, n))
    Y = X[:max(1, n // 3)]
    Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.repeat([1.0, 2.0, 3.0], (n + 2) // 3)[:n]
    return {"spd": X.T @ X / (2 * n), "rank_deficient": Y.T @ Y, "repeated": Qm @ np.diag(ev) @ Qm.T,
            "zero": np.zeros((n, n))}


def _eig_errors(A, d, Q):
    A = A.astype(np.float64)
    s = max(np.abs(A).max(), 1.0 if not A.any() else 0.0)
    rec = np.abs(Q.astype(np.float64) @ np.diag(d.astype(np.float64)) @ Q.T.astype(np.float64) - A).max() / s
    orth = np.abs(Q.T.astype(np.float64) @ Q.astype(np.float64) - np.eye(A.shape[0])).max()
    return rec, orth


@pytest.mark.parametrize("n", [1, 3, 12, 47, 64, 128, 129, 256, 300])
def test_eigensolver_matches_numpy_float32(sg, n):
    """k_kfac_eig (LDS path for small n, global memory above): reconstruction and orthogonality within 4x of numpy's float32
    eigh on the same matrix (floor 1e-6); the eigenvalues above 1e-6 agree with it."""
    from simgan_amd import _lib
    lib = _lib.load_test()
    holder = sg.Policy((3,), Box((1,)), base_kwargs={"hidden_size": 8})   # keeps the context alive
    ctx = holder.ctx
    rng = np.random.default_rng(n)
    for kind, A64 in _matrices(n, rng).items():
        A = np.ascontiguousarray(A64.astype(np.float32))
        Q, d, sw = np.empty((n, n), np.float32), np.empty(n, np.float32), C.c_int(0)
        _lib.check_test(lib.sg_test_kfac_eig(ctx.h, n, _lib.fptr(A), _lib.fptr(Q), _lib.fptr(d), C.byref(sw)))
        assert sw.value >= 0, (n, kind, "sweep cap")
        dn, Qn = np.linalg.eigh(A)
        dn_t = np.where(dn > 1e-6, dn, 0.0)   # the threshold kfac.py:236-237 applies to both
        rec, orth = _eig_errors(A, d, Q)
        rec_n, orth_n = _eig_errors(A, dn_t, Qn.astype(np.float32))
        d_full, dn_t = np.sort(d), np.sort(dn_t)
        assert rec <= 4 * max(rec_n, 1e-6), (n, kind, rec, rec_n)
        assert orth <= 4 * max(orth_n, 1e-6), (n, kind, orth, orth_n)
        assert np.allclose(d_full, dn_t, rtol=1e-5, atol=1e-5 * max(1.0, np.abs(dn).max())), (n, kind)


def test_graph_replay_is_bit_exact_over_twelve_updates(sg, monkeypatch):
    """Twelve updates (eigen refreshes at steps 0 and 10) replayed from the captured graph against the same launched kernel
    by kernel."""
    params, obs, actions, returns, _ = _random_case(47, 12, 64, 40, 128, seed=3)   # 5120 rows: two chunks
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        p = _policy(sg, 47, 12, 64, 64, params)
        agent = _agent(sg, p, seed=5)
        ro = _rollout(sg, 40, 128, 47, 12, obs, actions, returns)
        losses = [agent.update(ro) for _ in range(12)]
        k = agent.get_kfac()
        out.append((losses, p.get_flat_params(), k["momentum_buffer"], _flat_factors(k)))
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert np.array_equal(out[0][3][0], out[1][3][0]) and np.array_equal(out[0][3][1], out[1][3][1])


def test_drawn_value_noise_is_seeded_and_standard_normal(sg):
    """Without injected noise: the same seed gives bit-identical updates, another seed differs; the draws have mean and
    variance within 0.02 of N(0, 1) over 65,536 rows."""
    from simgan_amd import _lib
    params, obs, actions, returns, _ = _random_case(11, 3, 16, 16, 32, seed=7)
    res = []
    for seed in (1, 1, 2):
        p = _policy(sg, 11, 3, 16, 16, params)
        agent = _agent(sg, p, seed=seed)
        ro = _rollout(sg, 16, 32, 11, 3, obs, actions, returns)
        res.append(([agent.update(ro) for _ in range(2)], p.get_flat_params()))
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])
    assert not np.array_equal(res[0][1], res[2][1])
    lib = _lib.load_test()
    eps = np.empty(65536, np.float32)
    _lib.check_test(lib.sg_test_acktr_noise(p.ctx.h, eps.size, 12345, 3, _lib.fptr(eps)))
    assert abs(float(eps.mean())) < 0.02 and abs(float(eps.var()) - 1.0) < 0.02


def test_ppo_learner_results_ring_matches_the_synchronous_call(sg):
    """driver.PpoLearner with an ACKTR agent on a device-resident rollout (queued updates, LR decay writes that change nothing)
    against the same calls made synchronously; and the host-rollout mode runs."""
    from simgan_amd import _lib
    from simgan_amd.driver import PpoLearner
    from simgan_amd.utils import update_linear_schedule
    T, N, O, A, H = 5, 16, 47, 12, 64
    params, obs, actions, _, _ = _random_case(O, A, H, T, N, seed=11)
    rewards = np.random.default_rng(12).standard_normal((T, N, 1)).astype(np.float32)

    def setup(resident):
        p = _policy(sg, O, A, H, H, params)
        agent = _agent(sg, p, seed=9)
        ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 1)
        ro.obs.copy_(ro.obs.new_tensor(obs))
        ro.actions.copy_(ro.actions.new_tensor(actions))
        ro.rewards.copy_(ro.rewards.new_tensor(rewards))
        if resident:
            ro.sync_to_device()
            ro.device_resident = True
        return p, agent, ro

    p1, a1, r1 = setup(True)
    learner = PpoLearner(p1, a1, r1, use_linear_lr_decay=True, lr=0.25, num_updates=10)
    pending = [learner.update() for _ in range(3)]
    ring = [(q["value_loss"], q["action_loss"], q["dist_entropy"]) for q in pending]
    assert len(a1.optimizer.lr_writes) == 3

    p2, a2, r2 = setup(True)
    sync = []
    for j in range(3):
        _lib.check(r2.lib.sg_rollout_compute_returns_policy(r2.h, p2.h, 1, 0.99, 0.95, 1))
        sync.append(a2.update(r2))
        r2.after_update()
    assert ring == sync
    assert np.array_equal(p1.get_flat_params(), p2.get_flat_params())
    update_linear_schedule(a2.optimizer, 5, 10, 0.25)
    assert a2.optimizer.lr == 0.25

    p3, a3, r3 = setup(False)
    host = PpoLearner(p3, a3, r3, use_linear_lr_decay=True, lr=0.25, num_updates=10).update()
    assert all(np.isfinite(host[k]) for k in ("value_loss", "action_loss", "dist_entropy"))


def test_refusals(sg):
    """SplitPolicy, a world-2 context, RMSprop arguments, and Adam / RMSprop access on an ACKTR handle are refused."""
    from simgan_amd import _lib
    from test_gpu_world import run_ranks
    sp = sg.SplitPolicy((20,), Box((7,)), base_kwargs={"hidden_size": 32, "num_feet": 1})
    with pytest.raises(NotImplementedError, match="SplitPolicy"):
        sg.algo.A2C_ACKTR(sp, 0.5, 0.01, acktr=True)
    cfg = _lib.ACKTRConfig(0.5, 0.01, 0.25, 0.9, 0.99, 0.001, 0.01, 10)
    h = _lib.H()
    with pytest.raises(_lib.SimganHipError, match="SplitPolicy"):
        _lib.check(sp.lib.sg_acktr_create(sp.ctx.h, sp.h, C.byref(cfg), C.byref(h)))
    p = sg.Policy((6,), Box((2,)), base_kwargs={"hidden_size": 16})
    for kw in (dict(lr=7e-4), dict(max_grad_norm=0.5), dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)):
        with pytest.raises(NotImplementedError, match="K-FAC"):
            sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=True, **kw)
    agent = _agent(sg, p)
    n = p.num_params
    mm, vv, step = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int64(0)
    with pytest.raises(_lib.SimganHipError, match="K-FAC"):
        _lib.check(agent.lib.sg_ppo_get_adam(agent.h, _lib.fptr(mm), _lib.fptr(vv), n, C.byref(step)))
    with pytest.raises(_lib.SimganHipError, match="K-FAC"):
        _lib.check(agent.lib.sg_ppo_set_adam(agent.h, _lib.fptr(mm), _lib.fptr(vv), n, 0))
    with pytest.raises(_lib.SimganHipError, match="K-FAC"):
        _lib.check(agent.lib.sg_a2c_get_rmsprop(agent.h, _lib.fptr(mm), n, C.byref(step)))
    with pytest.raises(_lib.SimganHipError, match="K-FAC"):
        _lib.check(agent.lib.sg_a2c_set_rmsprop(agent.h, _lib.fptr(mm), n, 0))

    def body(rank, ctx):
        q = sg.Policy((6,), Box((2,)), base_kwargs={"hidden_size": 16}, ctx=ctx)
        try:
            sg.algo.A2C_ACKTR(q, 0.5, 0.01, acktr=True)
        except _lib.SimganHipError as exc:
            return str(exc)
        return None

    errs = run_ranks(2, body)
    assert all(e is not None and "world 2" in e for e in errs), errs


def test_reference_acktr_checkpoint_loads_onto_the_device(sg, tmp_path):
    """ckpt_policy_acktr.pt (SplitBias modules, pickled K-FAC hooks) through load_policy and PpoLearner.warm_start: the
    reference's own outputs; written back, the file has the plain layout."""
    from helpers import GOLDEN, assert_close
    from simgan_amd import checkpoint as ck
    from simgan_amd.driver import PpoLearner
    g = load("ckpt_policy_acktr")
    path = os.path.join(GOLDEN, "ckpt_policy_acktr.pt")
    pol, ob_rms = ck.load_policy(path)
    assert np.array_equal(pol.get_flat_params(), g["flat"])
    v, a, lp, _ = pol.act(g["obs"], None, None, deterministic=True)
    assert_close(v, g["value"], what="value")
    assert_close(a, g["action"], what="action")
    assert_close(lp, g["logp"], what="log-prob")
    assert np.array_equal(np.asarray(ob_rms["mean"] if isinstance(ob_rms, dict) else ob_rms.mean), g["rms_mean"])
    out = str(tmp_path / "saved.pt")
    ck.save_policy(out, pol, ob_rms)
    back = ck.read_reference_checkpoint(out)
    assert list(back["state_dict"])[1] == "base.actor.0.bias"
    assert np.array_equal(np.concatenate([x.reshape(-1) for x in back["state_dict"].values()]), g["flat"])
    m = g["meta"]
    warm = PpoLearner.warm_start(path, (m["O"],), Box((m["A"],)))
    n_trunk = m["H"] * m["O"] + m["H"] + m["H"] * m["H"] + m["H"]   # the actor trunk (warm_start re-initialises the critic)
    assert np.array_equal(warm.get_flat_params()[:n_trunk], g["flat"][:n_trunk])


def test_bare_torch_load_of_an_acktr_checkpoint(sg):
    """a2c/main.py:81-83: a bare torch.load through the alias package (SplitBias / KFACOptimizer resolve to inert holders)
    gives a device-backed Policy with the reference's weights and outputs.  In a child process (no alias module here)."""
    import subprocess
    from helpers import GOLDEN
    code = (
        "import sys, numpy as np, torch\n"
        "import simgan_amd as sg\n"
        "sys.path.insert(0, %r)\n"
        "from helpers import load, assert_close\n"
        "g = load('ckpt_policy_acktr')\n"
        "ac, ob_rms = torch.load(%r, map_location='cpu', weights_only=False)\n"
        "assert isinstance(ac, sg.Policy), type(ac)\n"
        "assert np.array_equal(ac.get_flat_params(), g['flat'])\n"
        "v, a, lp, _ = ac.act(torch.from_numpy(g['obs']), None, None, deterministic=True)\n"
        "assert_close(a, g['action'], what='action'); assert_close(v, g['value'], what='value')\n"
        "assert type(ob_rms) is sg.RunningMeanStd and np.array_equal(ob_rms.mean, g['rms_mean'])\n"
        "print('ok')\n") % (os.path.join(ROOT, "tests"), os.path.join(GOLDEN, "ckpt_policy_acktr.pt"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env, cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]


def test_eigensolver_error_reaches_fetching_and_queued_updates(sg):
    """k_kfac_eig's sticky sweep-cap word (raised here through the test hook, as the kernel raises it) fails a fetching update,
    and a queued update through PpoLearner's results ring reports it when its losses are read."""
    from simgan_amd import _lib
    from simgan_amd.driver import PpoLearner
    T, N, O, A, H = 5, 16, 11, 3, 16
    params, obs, actions, returns, eps = _random_case(O, A, H, T, N, seed=21)
    lib = _lib.load_test()
    p = _policy(sg, O, A, H, H, params)
    agent = _agent(sg, p)
    ro = _rollout(sg, T, N, O, A, obs, actions, returns)
    agent.update(ro)
    _lib.check_test(lib.sg_test_raise_kfac_error(agent.h))
    with pytest.raises(_lib.SimganHipError, match="k_kfac_eig"):
        agent.update(ro)
    p2 = _policy(sg, O, A, H, H, params)
    a2 = _agent(sg, p2)
    r2 = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 1)
    r2.obs.copy_(r2.obs.new_tensor(obs))
    r2.actions.copy_(r2.actions.new_tensor(actions))
    r2.sync_to_device()
    r2.device_resident = True
    learner = PpoLearner(p2, a2, r2)
    ok = learner.update()
    assert np.isfinite(ok["value_loss"])
    _lib.check_test(lib.sg_test_raise_kfac_error(a2.h))
    bad = learner.update()
    with pytest.raises(_lib.SimganHipError, match="k_kfac_eig"):
        bad["value_loss"]
    assert a2.optimizer.steps == 2
