"""GPU: ACKTR's step against float64 per K-FAC block, unclipped, off the damping and with non-default configs.
tests/test_gpu_acktr.py holds k_acktr_fisher, k_kfac_stats, k_kfac_fold, k_kfac_eig, k_kfac_gemm and k_kfac_step to one number,
rel-L2 of the whole Delta p under the constructor defaults, where the KL clip is active in every update (nu v is then invariant
under a rescaling of the gradient), the small blocks are 5e-4 .. 4e-2 of the norm and, at the shapes that reach the chunked rows
and the eigensolver's global-memory path, v ~ g / damping (tests/test_acktr_regimes_host.py shows all three on the float64
restatement alone).  Here, on the cases of tests/acktr_regimes.py, each proven in float64 to reach what it claims, every update
of every case is held to float64 on
  * the three losses;
  * nu, recovered as <buffer, v> / <v, v> with v the buffer of the same updates run with a kl_clip no step reaches;
  * every module's block of nu v (the momentum buffer: momentum 0, or the first update);
  * every module's block of Delta p;
  * each of the 12 distinct factors, relative to its own Frobenius norm;
the handle built with a non-default sg_acktr_config in all cases but one.  Graph replay is bit-equal on a refresh case; the
refresh cases' factors, and the two straddling factors of the dropped threshold case, go through k_kfac_eig alone.

Tolerances.  distance = ||got - float64||_2 / (||float64||_2 + ATOL max|float64| sqrt(n)) per block (max over the whole vector),
||got - float64||_F / ||float64||_F per factor.  Every distance holds
  * the project's ACKTR contract, now per block: distance <= DP_TOL = 2e-4; and
  * the arbiter form: distance <= F x (the float32 restatement's distance on the same block) + FLOOR[kind], the float32 distance
    being the largest over the evaluation and three more with inputs moved by an ulp (acktr_regimes.describe).
  FLOOR = the float32 restatement's own largest distance over the damping_dominated cases, per kind of measure, re-derived by
  tests/test_acktr_regimes_host.py: nu v 2.1e-6, Delta p 1.8e-5, factors 5.0e-7.
  F = 2: the worst (HIP - FLOOR) / float32 ratio measured on the MI355X, doubled, and not below 2.  The worst ratio over the cases
  here is 0.77 (unclipped_default, Delta p of dist.logstd: HIP 7.885e-5, float32 7.885e-5), and 0.95 over the fixtures of
  tests/test_gpu_acktr.py, which are held to the same F and FLOOR with the reference's own float32 run as the float32 column
  (acktr_default, Delta p of dist.logstd: 3.621e-4 both).  Largest HIP distances: nu v 1.5e-5 (float32 6.9e-5), factors 3.2e-7
  (float32 4.6e-7), Delta p 7.9e-5 on the cases here.
  Before k_kfac_fold took its present form the fixture acktr_multi missed this bound: G.critic_linear, a 1x1 factor, 7.3e-7 from
  float64 after ten updates against the float32 run's 1.0e-7, growing by 4e-8 per update (the fold's weights summed to 1 + 3.8e-8).
nu: relative NU_TOL = 1e-5 against float64 (one double-precision sum in k_kfac_step); measured 1.2e-7 at the worst
(refresh_h129, update 3; the float32 restatement's own 3.5e-8).
SG_ACKTR_REGIMES_RECORD=<path> writes every case's per-update distances, HIP and float32, to that file
(profiles/acktr_regimes_parity.json; tests/test_gpu_acktr.py's fixtures add theirs as fixture_<name>)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import acktr_regimes as ar
from helpers import ATOL, RTOL

pytestmark = pytest.mark.gpu

DP_TOL = 2e-4
NU_TOL = 1e-5
F = 2.0
FLOOR = {"nuv": 2.1e-6, "dp": 1.8e-5, "factors": 5.0e-7}


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def _record(label, rec):
    path = os.environ.get("SG_ACKTR_REGIMES_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_acktr_regimes.py under SG_ACKTR_REGIMES_RECORD.  Per case and update: the distance of the HIP path "
                       "and of the float32 restatement from the float64 restatement, per block of nu v (nuv), per block of Delta p (dp) "
                       "and per distinct factor (factors); ratio = max(0, hip - FLOOR[kind]) / float32; nu against float64.  fixture_<name>: "
                       "tests/test_gpu_acktr.py's fixtures, the float32 column being the reference's own float32 run.",
               "F": F, "FLOOR": FLOOR, "cases": {}}
    doc["cases"][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def make_agent(sg, policy, cfg):
    """an A2C_ACKTR whose sg_acktr_config is `cfg`: the constructor reads the module's KFAC_DEFAULTS, replaced for the call only"""
    from simgan_amd.algo import a2c_acktr as mod
    saved = mod.KFAC_DEFAULTS
    mod.KFAC_DEFAULTS = dict(saved, **cfg)
    try:
        agent = sg.algo.A2C_ACKTR(policy, ar.VCOEF, ar.ECOEF, acktr=True)
    finally:
        mod.KFAC_DEFAULTS = saved
    assert mod.KFAC_DEFAULTS["kl_clip"] == 0.001 and agent.optimizer.kl_clip == cfg["kl_clip"]
    return agent


def run_case(sg, c, cfg):
    """every update of the case on one handle, each from its prescribed parameters -> [(losses, buffer, Delta p, factors)]"""
    O, A, H, Hc = c.dims
    p = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H})
    if Hc != H:
        p.reset_critic((O,))       # the reference's warm start: a critic trunk 64 wide whatever the actor's width
    assert (p.hidden_size, p.critic_hidden) == (H, Hc), (p.hidden_size, p.critic_hidden)
    p.set_flat_params(c.updates[0]["params"])
    agent = make_agent(sg, p, cfg)
    out = []
    for j, u in enumerate(c.updates):
        p.set_flat_params(u["params"])
        ro = sg.RolloutStorage(c.T, c.N, (O,), Box((A,)), 1, 1)
        for name in ("obs", "actions", "returns"):
            getattr(ro, name).copy_(getattr(ro, name).new_tensor(u[name]))
        losses = agent.update(ro, value_noise=u["eps"])
        k = agent.get_kfac()
        assert k["steps"] == j + 1
        dp = p.get_flat_params().astype(np.float64) - u["params"].astype(np.float64)
        out.append((np.asarray(losses, np.float64), k["momentum_buffer"].astype(np.float64), dp, ar.distinct_factors(k["m_aa"], k["m_gg"])))
    return out


def judge(label, hip, o32):
    """both bounds on every distance of one update -> (failures, worst ratio, its name)"""
    fails, worst, at = [], 0.0, None
    for kind in ("nuv", "dp", "factors"):
        for name, x in hip[kind].items():
            ref = o32[kind][name]
            ratio = max(0.0, x - FLOOR[kind]) / ref if ref > 0 else (0.0 if x <= FLOOR[kind] else float("inf"))
            if ratio > worst:
                worst, at = ratio, f"{kind} {name}"
            if not (x <= DP_TOL and x <= F * ref + FLOOR[kind]):
                fails.append(f"{kind} {name}: HIP {x:.3e} from float64 (contract {DP_TOL:g}; float32 {ref:.3e}, limit {F * ref + FLOOR[kind]:.3e})")
    return fails, worst, at


@pytest.mark.parametrize("name", ar.all_cases())
def test_every_update_against_float64_per_block(sg, name):
    c = ar.case(name)
    got = run_case(sg, c, c.cfg)
    unclipped = run_case(sg, c, ar.big_kl(c.cfg))
    fails, rec = [], {"case": c.tag, "config": c.cfg, "updates": []}
    for j, ((losses, buf, dp, factors), (_, v, _, _), d) in enumerate(zip(got, unclipped, c.desc)):
        label = f"{name} update {j}"
        assert np.isfinite(buf).all() and np.isfinite(dp).all() and np.isfinite(losses).all(), label
        bad = np.abs(losses - d["losses"]) > ATOL + RTOL * np.abs(d["losses"])
        if bad.any():
            fails.append(f"{label}: losses {losses} against {d['losses']}")
        nu = float(buf @ v / (v @ v))
        nu_err = abs(nu / d["nu"] - 1.0)
        hip = {"nuv": ar.block_distances(buf, d["step"], c.dims), "dp": ar.block_distances(dp, d["dp"], c.dims),
               "factors": ar.factor_distances(factors, d["factors"])}
        f, ratio, at = judge(label, hip, d["o32"])
        print(f"{label}: nu {nu:.6f} (float64 {d['nu']:.6f}, off by {nu_err:.1e}; float32 {d['nu32']:.1e}); largest HIP distance "
              f"{ar.worst(hip):.3e} (float32 {ar.worst(d['o32']):.3e}); worst ratio {ratio:.2f} at {at}")
        rec["updates"].append({"nu_hip": nu, "nu_f64": d["nu"], "nu_rel_err": nu_err, "nu_rel_err_float32": d["nu32"], "vg_lr2": d["vg"],
                               "hip_vs_f64": hip, "float32_vs_f64": d["o32"], "worst_ratio": ratio, "worst_ratio_at": at,
                               "worst_hip": ar.worst(hip)})
        fails += [f"{label}: {x}" for x in f]
        if nu_err > NU_TOL:
            fails.append(f"{label}: nu {nu!r} against {d['nu']!r}: off by {nu_err:.2e} relative")
        # the run with a kl_clip no step reaches gives v itself, block by block at the gradient's scale
        vd = ar.block_distances(v, d["v"], c.dims)
        fails += [f"{label}: v (kl_clip {ar.BIG_KL:g}) {k}: {x:.3e}" for k, x in vd.items() if not (x <= DP_TOL and x <= F * d["o32"]["nuv"][k] + FLOOR["nuv"])]
    _record(name, rec)
    assert not fails, fails


def test_graph_replay_is_bit_equal_on_a_refresh_case(sg, monkeypatch):
    """refresh_h129 (Tf 2, momentum 0, stat_decay 0.5, kl_clip 0.1: nothing at its default) replayed from the captured graph
    against the same kernels launched one by one: losses, buffers, parameters and factors bit-equal over the four updates."""
    c = ar.case("refresh_h129")
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        out.append(run_case(sg, c, c.cfg))
    for j, (a, b) in enumerate(zip(*out)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), j
        assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3])), j
    assert np.abs(out[0][3][1]).max() > 0


def _eig_alone(sg, ctx, lib, m64):
    from simgan_amd import _lib
    n = m64.shape[0]
    A = np.ascontiguousarray(m64.astype(np.float32))
    Q, d, sw = np.empty((n, n), np.float32), np.empty(n, np.float32), C.c_int(0)
    _lib.check_test(lib.sg_test_kfac_eig(ctx.h, n, _lib.fptr(A), _lib.fptr(Q), _lib.fptr(d), C.byref(sw)))
    assert sw.value >= 0, "sweep cap"
    return A.astype(np.float64), Q.astype(np.float64), d.astype(np.float64)


EIG_ALONE = [("refresh_small", 0), ("refresh_small", 2), ("refresh_h129", 0), ("refresh_h129", 2), ("threshold", 0)]


@pytest.mark.parametrize("name,j", EIG_ALONE, ids=[f"{n}-update{j}" for n, j in EIG_ALONE])
def test_factors_through_the_eigensolver_alone(sg, name, j):
    """The factors a refresh decomposes (update 0: first statistics; update 2: running averages; hidden 129: the global-memory
    path) through sg_test_kfac_eig, which tells a fault of the eigensolver from one of the rotations: against numpy's float64 eigh
    of the same float32 matrix, the eigenvalues within 2 x 2^-24 sqrt(n) max|d| (Weyl's bound on the float32 rounding of the matrix,
    and the float32 store), the same eigenvalues zeroed, Q orthogonal and Q d Q^T the matrix to 1e-6.  For the dropped threshold
    case: its two straddling factors, whose eigenvalues lie a factor of 3 from 1e-6 on both sides."""
    from simgan_amd import _lib
    lib = _lib.load_test()
    holder = sg.Policy((3,), Box((1,)), base_kwargs={"hidden_size": 8})   # keeps the context alive
    c = ar.case(name) if name in ar.SPECS else ar.build(name, check=False)
    d64 = c.desc[j]
    assert d64["refreshed"]
    names = c.straddle if name == "threshold" else ar.FACTORS
    for fname in names:
        m = d64["factors"][ar.FACTORS.index(fname)]
        n = m.shape[0]
        A, Q, d = _eig_alone(sg, holder.ctx, lib, m)
        ref = np.linalg.eigh(np.triu(A) + np.triu(A, 1).T)[0]
        ref_t = np.where(ref > ar.EIG_THRESHOLD, ref, 0.0)
        tol = 2.0 * 2.0 ** -24 * np.sqrt(n) * np.abs(ref).max()
        assert np.abs(np.sort(d) - np.sort(ref_t)).max() <= tol, (name, j, fname, np.abs(np.sort(d) - np.sort(ref_t)).max(), tol)
        assert int((d == 0).sum()) == int((ref_t == 0).sum()), (name, j, fname)
        scale = max(np.abs(A).max(), 1e-300)
        # the zeroed eigenvalues are part of A: reconstruct with the kept ones and compare on the kept subspace's share
        rec = np.abs(Q @ np.diag(d) @ Q.T - A).max() / scale
        lost = ref[ref <= ar.EIG_THRESHOLD]
        assert rec <= 1e-6 + (np.abs(lost).max() / scale if lost.size else 0.0), (name, j, fname, rec)
        assert np.abs(Q.T @ Q - np.eye(n)).max() <= 1e-6, (name, j, fname)
        if name == "threshold":
            assert (d >= 3.0 * ar.EIG_THRESHOLD).any() and (d == 0).any() and not ((d > 0) & (d < 3.0 * ar.EIG_THRESHOLD)).any(), (fname, d)
