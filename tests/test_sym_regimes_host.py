"""CPU: the case builders of tests/sym_regimes.py judged on the references alone, and the reason tests/test_gpu_sym_regimes.py exists:
three wrong symmetry gradients that the older comparisons of tests/test_gpu_symmetry.py pass -- shown here on the float32 oracle +
float64 restatement, no kernel involved -- and that the per-block comparison against float64 fails by more than 100 times its bound."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import regimes as rg  # noqa: E402
import sym_regimes as sr  # noqa: E402
import test_symmetry_host as tsh  # noqa: E402
from helpers import RTOL, assert_close, assert_close_adam, load  # noqa: E402

IDS = ["-".join(str(x) for x in spec) for spec in sr.all_cases()]


@pytest.mark.parametrize("spec", sr.all_cases(), ids=IDS)
def test_case_reaches_what_it_claims(spec):
    regime, O, A, H, mirror, rows = spec
    c = sr.case(*spec)    # the builder asserts regimes._check, rms e, the float32 distance, the zeros / the shares (sym_regimes._check)
    worst = max(max(c.o32_clipped.values()), max(c.o32_plain.values()))
    print(c.tag, f"coef {c.symmetry_coef:g}, rms e {c.e_rms:.3g}, norm {c.norm:.3g}, float32 worst block {worst:.2e}, shares",
          {k: round(s, 2) for k, s in c.shares.items()})
    assert c.seed == sr.SEEDS.get(spec, 0) and c.T * c.N == rows
    assert c.e_rms >= sr.MIN_E_RMS and worst <= 0.5 * RTOL
    assert c.mrows.dtype == np.float32 and c.m_obs.dtype == np.float32 and c.m_act.dtype == np.float32
    x = c.obs[:-1].reshape(rows, O)
    assert np.array_equal(c.mrows, (x.astype(np.float64) @ c.m_obs.astype(np.float64).T).astype(np.float32))
    # the restatement with a dtype argument IS test_symmetry_host's at float64, and float32 through and through at float32
    l64, g64 = tsh.sym_loss_grad(c.params, x, c.mrows, c.m_act, c.symmetry_coef, O, A, H)
    l, g = sr.sym_loss_grad(c.params, x, c.mrows, c.m_act, c.symmetry_coef, O, A, H, np.float64)
    assert_close(g, g64, rtol=1e-12, atol=0.0, what="float64 restatement")
    assert abs(l - l64) <= 1e-12 * l64 and l64 == c.sym_loss
    assert_close(c.grad_clipped - c.desc["grad_clipped"], g64, rtol=1e-9, atol=1e-15, what="grad64 = PPO + symmetry")
    l32, g32 = sr.sym_loss_grad(c.params, x, c.mrows, c.m_act, c.symmetry_coef, O, A, H, np.float32)
    assert g32.dtype == np.float32 and l32.dtype == np.float32 and sr.grad32(c, True).dtype == np.float32
    norms = sr._block_norms(c, c.grad_clipped)
    if regime == "sym_only":
        assert c.symmetry_coef == 1.0 and c.entropy_coef == 0.0 and not c.desc["grad_clipped"].any()
        assert np.array_equal(c.grad_clipped, g64)       # the one-step gradient is the symmetry gradient alone
        for k, n in norms.items():
            assert (n == 0.0) == (k not in sr.ACTOR_BLOCKS), (k, n)
    else:
        assert all(sr.SHARE[0] <= s <= sr.SHARE[1] for s in c.shares.values()), c.shares
        assert c.symmetry_coef >= 1.0 and c.symmetry_coef == round(c.symmetry_coef)
        assert not np.array_equal(c.grad_clipped, c.grad_plain)
    if mirror == "dense":
        for m in (c.m_obs, c.m_act):
            assert np.linalg.norm(m - m.T) >= 0.1 * np.linalg.norm(m)
        assert np.abs(c.m_act @ c.m_act - np.eye(A)).max() > 0.1 and not c.m_act[A // 2].any()
    else:
        assert np.array_equal(c.m_act, c.m_act.T) and np.array_equal(c.m_obs, c.m_obs.T)   # why the fixture cannot see a transpose
    if regime == "saturated":
        assert c.desc["saturation"] > 0.2


def test_the_gradient_clip_case_lies_between_its_two_settings():
    c, hi = sr.clip_case()
    assert 1.1 * sr.CLIP_LO <= c.norm <= 0.9 * hi


# ------------------------------------------------------------------ the blind spots of the older comparisons
def _wrong_bias(factor):
    """test_symmetry_host.sym_loss_grad with the symmetry gradient of dist.fc_mean.bias multiplied by `factor`"""
    right = tsh.sym_loss_grad

    def wrong(params, x, xm, m_act, coef, O, A, H):
        loss, g = right(params, x, xm, m_act, coef, O, A, H)
        assert np.abs(g[tsh.actor_slices(O, A, H)["bh"]]).max() > 0.0
        g[tsh.actor_slices(O, A, H)["bh"]] *= factor
        return loss, g
    return wrong


def _refine_problem():
    import test_gpu_symmetry as tgs
    from simgan_amd.symmetry import laikago_mirror
    mo, ma = laikago_mirror(111)
    return tgs._random_problem(111, 12, 64, 16, 256, 1, 1, 1.0, 5, mo, ma)


def _hidden_256_problem():
    import test_gpu_symmetry as tgs
    rng = np.random.default_rng(2)
    mo = np.linalg.qr(rng.standard_normal((20, 20)))[0]
    ma = np.eye(6)[rng.permutation(6)] * np.where(rng.random(6) < 0.5, -1.0, 1.0)[:, None]
    return tgs._random_problem(20, 6, 256, 7, 11, 2, 3, 0.7, 9, mo, ma)


@pytest.mark.parametrize("problem,factor,steps", [(_hidden_256_problem, 0.0, 6), (_refine_problem, 0.5, 1)], ids=["hidden256-removed", "refine-halved"])
def test_old_comparison_passes_a_wrong_small_block(monkeypatch, problem, factor, steps):
    """assert_close_adam on post-Adam parameters (test_hidden_256_global_weight_instances, six steps;
    test_refine_minibatch_single_step_matches_the_restatement, one step) passes an update whose symmetry gradient of
    dist.fc_mean.bias was removed entirely / halved: after Adam a parameter moves by about lr sign(g)."""
    g = problem()
    rows = tsh.mirrored_rows_of(g)
    right = tsh.sym_update_restated(g, rows)[0]
    monkeypatch.setattr(tsh, "sym_loss_grad", _wrong_bias(factor))
    wrong = tsh.sym_update_restated(g, rows)[0]
    assert not np.array_equal(wrong, right), "the wrong gradient changed nothing: the demonstration is empty"
    assert_close_adam(wrong, right, lr=g["meta"]["lr"], steps=steps, what="a wrong dist.fc_mean.bias block")   # passes: the blind spot


def test_old_comparison_passes_a_transposed_action_mirror():
    """The Laikago M_a is a symmetric matrix: the restatement with M_a read transposed lands on ppo_sym_laikago's params1 and
    adam_m within test_symmetric_update_matches_the_reference_fixture's tolerances."""
    g = load("ppo_sym_laikago")
    assert np.array_equal(g["m_act"], g["m_act"].T) and np.array_equal(g["m_obs"], g["m_obs"].T)
    gt = dict(g, m_act=np.ascontiguousarray(g["m_act"].T))
    par, adam, losses, _ = tsh.sym_update_restated(gt, tsh.mirrored_rows_of(g))
    assert_close(par, g["params1"], what="params after update")
    assert_close(adam.m, g["adam_m"], rtol=1e-3, atol=1e-7, what="adam m")


# ------------------------------------------------------------------ the new comparison sees them
def _float32_with(c, bias_factor=1.0, m_act=None):
    """the float32 evaluation of a sym_only case with an error put into its symmetry part"""
    B = c.T * c.N
    g = rg.grad(c, True, 32)[0].astype(np.float32)
    _, gs = sr.sym_loss_grad(c.params, c.obs[:-1].reshape(B, c.O), c.mrows, c.m_act if m_act is None else m_act, c.symmetry_coef,
                             c.O, c.A, c.H, np.float32)
    gs[tsh.actor_slices(c.O, c.A, c.H)["bh"]] *= np.float32(bias_factor)
    return g + gs


@pytest.mark.parametrize("error", ["bias-removed", "bias-halved", "mirror-transposed"])
@pytest.mark.parametrize("spec", [("sym_only", 111, 12, 64, "dense", 128), ("sym_only", 5, 2, 8, "dense", 77)], ids=["111x12x64", "5x2x8"])
def test_new_comparison_fails_each_by_more_than_100_bounds(spec, error):
    import test_gpu_sym_regimes as tg
    c = sr.case(*spec)
    right = sr.distances(c, _float32_with(c))
    assert not tg.failing_blocks(right, c.o32_clipped), "the float32 evaluation itself must pass"
    got = _float32_with(c, **{"bias-removed": dict(bias_factor=0.0), "bias-halved": dict(bias_factor=0.5),
                              "mirror-transposed": dict(m_act=np.ascontiguousarray(c.m_act.T))}[error])
    dist = sr.distances(c, got)
    over = {k: dist[k] / tg.bound(c.o32_clipped[k]) for k in dist}
    print(c.tag, error, {k: f"{x:.3g}" for k, x in over.items()})
    assert tg.failing_blocks(dist, c.o32_clipped)
    if error == "mirror-transposed":
        assert min(over[k] for k in sr.ACTOR_BLOCKS) > 100.0     # every actor block
    else:
        assert over["dist.fc_mean.bias"] > 100.0
        assert all(over[k] <= 1.0 for k in over if k != "dist.fc_mean.bias")   # and only the block that is wrong


def test_the_arbiter_floor_is_the_float32_distance_of_the_unsaturated_cases():
    """tests/test_gpu_sym_regimes.py's FLOOR: the float32 evaluation's largest block distance over the sym_only and mixed cases"""
    import test_gpu_sym_regimes as tg
    worst = max(max(max(c.o32_clipped.values()), max(c.o32_plain.values())) for c in (sr.case(*spec) for spec in sr.floor_cases()))
    print("worst float32 block distance over the sym_only and mixed cases", worst)
    assert abs(worst / tg.FLOOR - 1.0) <= 0.1   # (libm and BLAS builds move it in the second digit)


def test_launch_table_follows_from_the_restated_launcher():
    """the instance every launch of tests/test_gpu_sym_regimes.py (3a, 3c) names is the one the restated launcher derives"""
    import test_gpu_sym_regimes as tg
    for env, shape, want in tg.LAUNCHES + tg.WIDE_LAUNCHES:
        for rows in (128, 77):
            assert tg.instance_of(*shape, rows, env) == want, (env, shape, rows)
    # (20, 130, 32): M_a alone is 67,600 bytes; 32-row groups need 182,416 bytes of LDS, 16-row groups 138,320
    assert tg.bwd_sym_lds_bytes(20, 130, 32, 2, False) == 182416 > tg.LDS_BYTES >= tg.bwd_sym_lds_bytes(20, 130, 32, 1, False) == 138320
