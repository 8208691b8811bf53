"""CPU: the case builders of tests/acktr_regimes.py judged on the float64 restatement alone -- every case the GPU file
(tests/test_gpu_acktr_regimes.py) runs reaches what it claims and is well-conditioned (the float32 evaluation of the same
algorithm within 1e-4 of float64 on every block and factor), the floor constants of the GPU file are re-derived, and the reason
that file exists is restated as assertions: under the KL clip a doubled gradient leaves Delta p unchanged, a 30 % error in
critic_linear.bias stays under DP_TOL by the whole-vector measure, and the per-block measure flags both."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import acktr_regimes as ar  # noqa: E402
from helpers import load  # noqa: E402
from test_acktr_host import KFAC, acktr_update_restated, dims_of  # noqa: E402
from test_acktr_host import new_state as old_state  # noqa: E402


@pytest.mark.parametrize("name", ar.all_cases())
def test_case_reaches_what_it_claims(name):
    c = ar.case(name)          # the builder asserts the regime's conditions and the conditioning (acktr_regimes._check)
    print(ar.summary(c))
    O, A, H, Hc = c.dims
    for j, (u, d) in enumerate(zip(c.updates, c.desc)):
        assert all(u[k].dtype == np.float32 for k in ("params", "obs", "actions", "returns", "eps"))
        assert u["obs"].shape == (c.T + 1, c.N, O) and u["actions"].shape == (c.T, c.N, A) and u["eps"].shape == (c.T, c.N, 1)
        assert d["nu"] == min(1.0, np.sqrt(c.cfg["kl_clip"] / d["vg"]))
        assert len(d["eig"]) == len(d["factors"]) == len(ar.FACTORS) == 12
        lr_eff = c.cfg["lr"] * (1.0 - c.cfg["momentum"])
        if j == 0 or c.cfg["momentum"] == 0.0:      # the momentum buffer is nu v of this very update, Delta p = -lr (1 - momentum) nu v
            assert np.allclose(d["dp"], -lr_eff * d["step"], rtol=1e-6, atol=1e-7 * np.abs(u["params"]).max())
    if c.regime == "unclipped":
        assert all(d["nu"] == 1.0 for d in c.desc)
    if c.regime == "refresh":
        assert [d["refreshed"] for d in c.desc] == [True, False, True, False]
        assert not np.array_equal(c.updates[0]["obs"], c.updates[1]["obs"]) and not np.array_equal(c.updates[0]["params"], c.updates[1]["params"])
        # update 2 decomposes running averages: its factors are neither update 2's own statistics nor update 0's, by 100 x COND
        own = ar.update(c.updates[2]["params"], ar.new_state(), *(c.updates[2][k] for k in ("obs", "actions", "returns", "eps")), c.dims,
                        ar.VCOEF, ar.ECOEF, c.cfg)[3]
        for name_f, run, fresh, first in zip(ar.FACTORS, c.desc[2]["factors"], ar.state_factors(own), c.desc[0]["factors"]):
            if run.shape != (1, 1):
                far = 100 * ar.COND * np.linalg.norm(run)
                assert np.linalg.norm(run - fresh) > far and np.linalg.norm(run - first) > far, name_f


def test_the_cases_cover_the_kernel_edges_they_are_there_for():
    """SPECS' shapes against the code's constants: 16x16 and 32x32 tile edges, ragged row quads, a partial chunk of 1 .. 3 rows,
    the eigensolver's LDS limit (16 n^2 + 8192 bytes against 160 KB: n <= 98) and the issue's 128 / 129, the global-weight shape,
    a critic of another width, the default config and every config field moved off its default somewhere."""
    specs = ar.SPECS
    widths = {w for s in specs.values() for w in s["dims"]}
    assert {5, 16, 17, 47} <= widths and {31, 32, 33} <= widths and {98, 99, 128, 129, 256} <= widths
    lds_n = max(n for n in range(1, 513) if 16 * n * n + 8192 <= 160 * 1024)
    assert lds_n == 98
    rows = {s["T"] * s["N"] for s in specs.values()}
    assert {ar.CHUNK + 1, ar.CHUNK + 2, ar.CHUNK + 3} <= rows and any(r % 4 for r in rows) and 65536 in rows
    with open(os.path.join(ROOT, "simgan_amd", "csrc", "sg_ppo.hip")) as f:
        assert f"#define SG_A2C_CHUNK_ROWS {ar.CHUNK}\n" in f.read()
    assert any(s["dims"][3] != s["dims"][2] for s in specs.values())
    assert specs["eigen_global_weights"]["dims"][:3] == (150, 8, 256) and specs["eigen_global_weights"]["T"] * specs["eigen_global_weights"]["N"] >= 512
    assert specs["refresh_h129"]["dims"][2] == 129
    default = ar.config()
    assert specs["unclipped_default"]["cfg"] == default
    for field in default:
        assert any(s["cfg"][field] != default[field] for s in specs.values()), field
    from simgan_amd.algo.a2c_acktr import KFAC_DEFAULTS
    assert all(ar.f32(KFAC_DEFAULTS[k]) == default[k] for k in default)


def test_generalised_restatement_is_the_restatement():
    """acktr_regimes.update at float64 against tests/test_acktr_host.py's acktr_update_restated over the twelve updates of
    acktr_multi (two eigen refreshes, momentum carried): the same numbers."""
    g = load("acktr_multi")
    m = g["meta"]
    a, b = ar.new_state(), old_state()
    for j in range(m["iters"]):
        pre = f"it{j}_"
        args = (g[pre + "params0"], g[pre + "obs"], g[pre + "actions"], g[pre + "returns"], g[pre + "eps"])
        p1a, la, a, info = ar.update(args[0], a, *args[1:], dims_of(m), m["value_loss_coef"], m["entropy_coef"], KFAC)
        p1b, lb, b = acktr_update_restated(args[0], b, *args[1:], dims_of(m), m["value_loss_coef"], m["entropy_coef"])
        assert np.allclose(p1a, p1b, rtol=1e-13, atol=0.0) and np.allclose(la, lb, rtol=1e-14, atol=0.0), j
        assert np.allclose(a["buf"], b["buf"], rtol=1e-12, atol=1e-300), j
        assert info["refreshed"] == (j % 10 == 0)


@pytest.mark.parametrize("name", ar.all_cases())
def test_float32_restatement_is_within_the_condition_of_float64(name):
    """per block of nu v, per block of Delta p, per factor, every update: the float32 evaluation (the largest over the evaluation
    and three with inputs moved by an ulp) <= COND = 1e-4; its nu within 5e-6 relative, half of what the GPU file allows."""
    c = ar.case(name)
    for j, d in enumerate(c.desc):
        for what, dist in d["o32"].items():
            k = max(dist, key=dist.get)
            print(f"{c.tag} update {j}: {what}: worst {k} {dist[k]:.3e}")
            assert dist[k] <= ar.COND, (name, j, what, k, dist[k])
        assert d["nu32"] <= 5e-6, (name, j, d["nu32"])
    ar._check_conditioning(c)


def test_threshold_case_reaches_its_eigenvalues_but_not_the_condition():
    """The dropped case (acktr_regimes.DROPPED): A.obs and G.dist.fc_mean hold eigenvalues on both sides of 1e-6, every factor a
    factor of 3 away from it, and keeping the sub-threshold eigenvalues would move v by 100 x COND or more -- and the float32
    evaluation is outside COND, so no bound the project could defend would judge the HIP path on it."""
    c = ar.build("threshold", check=False)
    ar._check_regime(c)
    d = c.desc[0]
    print(ar.summary(c), "zeroing moves v by", c.zeroing_shows(d))
    assert ar.worst(d["o32"]) > ar.COND
    with pytest.raises(AssertionError, match="float32 evaluation"):
        ar._check_conditioning(c)


def test_the_floors_are_the_float32_distances_of_the_damping_dominated_cases():
    """tests/test_gpu_acktr_regimes.py's FLOOR, per kind of measure: the float32 evaluation's largest distance over the
    damping_dominated cases, where v is the gradient over a constant and no eigenvalue decides anything.  The constants may not
    be below the re-derived values, nor more than a quarter above (libm and BLAS builds move them in the second digit)."""
    import test_gpu_acktr_regimes as tg
    for what in ("nuv", "dp", "factors"):
        per = {n: max(max(d["o32"][what].values()) for d in ar.case(n).desc) for n in ar.all_cases() if ar.SPECS[n]["regime"] == "damping_dominated"}
        rest = {n: max(max(d["o32"][what].values()) for d in ar.case(n).desc) for n in ar.all_cases()}
        worst = max(per.values())
        print(f"FLOOR[{what}]: re-derived {worst:.3e} {per}; constant {tg.FLOOR[what]:.3e}; all cases up to {max(rest.values()):.3e}")
        assert worst <= tg.FLOOR[what] <= 1.25 * worst, (what, worst, tg.FLOOR[what])
    assert tg.F >= 2.0 and tg.DP_TOL == 2e-4 and tg.NU_TOL == 1e-5


# ------------------------------------------------------------------------------------------- what the whole-vector measure does not see
def _old_case(O, A, H, T, N):
    """tests/test_gpu_acktr.py's restated shapes under the constructor defaults, as a single-update case of this module"""
    from test_gpu_acktr import _random_case
    params, obs, actions, returns, eps = _random_case(O, A, H, T, N, seed=O + H + T + N)
    return (O, A, H, H), dict(params=params, obs=obs, actions=actions, returns=returns, eps=eps)


def _run(dims, u, cfg, **kw):
    p1, _, _, info = ar.update(u["params"], ar.new_state(), u["obs"], u["actions"], u["returns"], u["eps"], dims, ar.VCOEF, ar.ECOEF, cfg, **kw)
    return p1 - u["params"].astype(np.float64), info


@pytest.mark.parametrize("shape", [(47, 12, 64, 1000, 8), (150, 8, 256, 5, 13)])
def test_a_doubled_gradient_leaves_a_clipped_step_unchanged_and_an_unclipped_one_doubled(shape):
    """nu = sqrt(kl_clip / (lr^2 v g)) < 1 makes nu v invariant under g -> 2 g: on tests/test_gpu_acktr.py's own shapes a 1 / B
    off by 2 in the gradient ACKTR mode feeds to k_kfac_gemm changes Delta p by less than 1e-12 of itself, far inside DP_TOL.  On an
    unclipped case the same fault is a per-block distance of 1 (0.7 where the doubled step meets the clip)."""
    from test_gpu_acktr import DP_TOL
    dims, u = _old_case(*shape)
    dp, info = _run(dims, u, ar.config())
    dp2, info2 = _run(dims, u, ar.config(), grad_scale=2.0)
    print(f"{shape}: nu {info['nu']:.4f} -> {info2['nu']:.4f}, Delta p changes by {ar.whole_vector_distance(dp2, dp):.2e}")
    assert info["nu"] < 1.0 and abs(info2["nu"] / info["nu"] - 0.5) < 1e-12
    assert ar.whole_vector_distance(dp2, dp) < 1e-12 < DP_TOL            # the old measure is blind ...
    assert max(ar.block_distances(dp2, dp, dims).values()) < 1e-12       # ... and so is any measure under the clip
    for name in ("unclipped_default", "unclipped_tiles16", "damping_chunk"):
        c = ar.case(name)
        uu, d = c.updates[0], c.desc[0]
        dpf, inf = _run(c.dims, uu, c.cfg, grad_scale=2.0)
        dist = ar.block_distances(inf["step"], d["step"], c.dims)
        # (unclipped_default sits at v g lr^2 = 0.35 kl_clip: four times that clips the doubled step back to 1.7 x)
        want = 2.0 * inf["nu"] - 1.0
        assert want > 0.65 and (inf["nu"] == 1.0 or name == "unclipped_default")
        assert min(dist.values()) > 0.9 * want and ar.whole_vector_distance(dpf, d["dp"]) > 0.9 * want, (name, dist)


def test_a_wrong_small_block_passes_the_whole_vector_measure_and_fails_the_block_measure():
    """150x8x256 under the defaults (tests/test_gpu_acktr.py's shape): critic_linear.bias wrong by 30 %, dist.logstd by 3 %,
    critic.0.bias by 1 % all stay under DP_TOL = 2e-4 as rel-L2 of the whole Delta p; block by block they are 0.3, 0.03 and 0.01."""
    from test_gpu_acktr import DP_TOL
    dims, u = _old_case(150, 8, 256, 5, 13)
    dp, _ = _run(dims, u, ar.config())
    slices, _ = ar.block_slices(dims)
    shares = {k: float(np.linalg.norm(dp[s]) / np.linalg.norm(dp)) for k, s in slices.items()}
    print("shares of ||Delta p||:", {k: f"{x:.2e}" for k, x in shares.items()})
    for block, err in (("critic_linear.bias", 0.30), ("dist.logstd", 0.03), ("critic.0.bias", 0.01)):
        bad = dp.copy()
        bad[slices[block]] *= 1.0 + err
        whole, per = ar.whole_vector_distance(bad, dp), ar.block_distances(bad, dp, dims)
        print(f"{block} wrong by {err:.0%}: whole vector {whole:.2e}, block {per[block]:.2e}")
        assert whole < DP_TOL                                            # the old measure passes the fault
        assert per[block] > 0.5 * err > DP_TOL                           # the new one fails it
        assert all(x == 0.0 for k, x in per.items() if k != block)
