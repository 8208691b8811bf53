"""CPU: the case builders of tests/regimes.py, judged on the references alone (oracle/oracle64.py, tests/gru_ref.py) -- every
case the GPU file (tests/test_gpu_regimes.py) uses reaches every branch it claims, with no row within regimes.MARGIN of a branch
boundary and the gradient norm on the stated side of the gradient clip, and the float32 evaluation of the same algorithm sits
within the project's 1e-4 of the float64 one, so the GPU tests never run on a case that means nothing."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gru_ref  # noqa: E402
import regimes as rg  # noqa: E402
from helpers import ATOL, RTOL, assert_close, load  # noqa: E402

IDS = [f"{c[0]}-{c[1]}-{c[2]}x{c[3]}x{c[4]}" + (f"-w{c[6]:g}o{c[7]:g}" if c[0] == "saturated" else "") for c in rg.all_cases()]


@pytest.mark.parametrize("spec", rg.all_cases(), ids=IDS)
def test_case_reaches_what_it_claims(spec):
    regime, kind, O, A, H, f, sw, so = spec
    c = rg.case(regime, kind, O, A, H, f, sw, so)   # the builder asserts the class counts and the margins (regimes._check)
    d, cl = c.desc, c.desc["classes"]
    print(c.tag, cl, {k: d[k] for k in ("margin_ratio", "margin_value", "margin_uw", "norm", "norm_plain", "saturation")})
    assert sum(cl[k] for k in ("above_adv+", "above_adv-", "below_adv+", "below_adv-", "inside")) == c.T * c.N
    assert cl["u>w"] + cl["w>u_outside"] + cl["value_inside"] == c.T * c.N
    assert min(d["margin_ratio"], d["margin_value"], d["margin_uw"]) >= rg.MARGIN
    # the one-step gradient tests run with max_grad_norm = 1e9: the clip is inactive whatever the norm; it must be a number
    assert np.isfinite(d["norm"]) and np.isfinite(d["norm_plain"])
    if regime == "all_clipped":
        assert d["norm"] == 0.0 and d["norm_plain"] > 0.1     # with the value clip off the same rows have a gradient
        assert c.desc["losses_clipped"][0] > 0.1
    else:
        assert d["norm"] > 0.55, "the clip at max_grad_norm = 0.5 must be active by 10 %"
        # the two value losses differ on exactly the rows outside the value clip
        assert not np.array_equal(d["grad_clipped"], d["grad_plain"])
    if regime == "saturated":
        base = rg.case("off_policy", kind, O, A, H, f)
        # a fifth of the units (of the GRU's gates) sit within 1e-3 of their asymptote; next to none do at scale 1
        assert d["saturation"] > 0.2 and base.desc["saturation"] < 0.01, (d["saturation"], base.desc["saturation"])
        assert d["norm"] > 1.1 * 0.5


@pytest.mark.parametrize("spec", rg.all_cases(), ids=IDS)
def test_float32_gradient_is_within_the_contract_of_float64(spec):
    """rel-L2 over all parameters of the float32 evaluation's one-step gradient against float64 <= helpers.RTOL, and the
    losses at the project's tolerance: a case on which float32 itself could not hold 1e-4 would judge nothing."""
    regime, kind, O, A, H, f, sw, so = spec
    c = rg.case(regime, kind, O, A, H, f, sw, so)
    for uc in (True, False):
        g64, l64 = c.desc["grad_clipped" if uc else "grad_plain"], c.desc["losses_clipped" if uc else "losses_plain"]
        g32, l32 = rg.grad(c, uc, 32)
        if regime == "all_clipped" and uc:
            assert not g32.any(), "float32 must find the same exact zeros"
        else:
            rel = float(np.sqrt(((g32 - g64) ** 2).sum() / (g64 ** 2).sum()))
            print(c.tag, "clipped" if uc else "plain", "float32 vs float64 rel-L2", rel)
            assert rel <= RTOL
        assert_close(l32, l64, rtol=RTOL, atol=ATOL, what="losses")


def test_clip_sides_of_the_two_sided_cases():
    """tests/test_gpu_regimes.py, 2c: every step of the two updates sees a float64 norm above 0.5 and below 5.0 by 10 %."""
    for spec, perm_seed in rg.CLIP_CASES:
        c = rg.case("off_policy", *spec)
        perms = rg.clip_perms(c, perm_seed)
        for mg in (0.5, 5.0):
            norms = rg.ppo_update64(c, perms, 2, 2, rg.LR, rg.EPS, mg, updates=2)["norms"]
            assert len(norms) == 8 and min(norms) >= 1.1 * 0.5 and max(norms) <= 0.9 * 5.0, (spec, mg, norms)
    norm = rg.a2c_restated(rg.case("off_policy", *rg.A2C_CLIP_CASE), 0.5)[3]
    assert 1.1 * 0.5 <= norm <= 0.9 * 5.0, norm
    assert 1.1 * 0.5 <= rg.a2c_restated(rg.case("saturated", "mlp", 47, 12, 64, 1, 4.0, 3.0), 0.5)[3]   # 2e: the clip is active


def test_gru_ref_passes_use_clipped_through_and_float32_mode_agrees():
    """gru_ref.ppo_update(use_clipped=False) differs from the clipped update on a case with rows outside the value clip, and
    equals a hand-rolled step on minibatch_grad(use_clipped=False); the reference-written fixture still reproduces."""
    c = rg.case("off_policy", "gru", 13, 5, 20, 1)
    ro = {k: c[k] for k in ("obs", "actions", "value_preds", "returns", "action_log_probs", "masks")}
    perms = np.arange(c.N)[None]
    a = gru_ref.ppo_update(c.params, c.O, c.A, c.H, ro, c.hxs0, perms, 1, 1, rg.CLIP, rg.VCOEF, 0.01, 3e-4, 1e-5, 1e9)
    b = gru_ref.ppo_update(c.params, c.O, c.A, c.H, ro, c.hxs0, perms, 1, 1, rg.CLIP, rg.VCOEF, 0.01, 3e-4, 1e-5, 1e9, use_clipped=False)
    assert_close(a["adam_m"] / 0.1, c.desc["grad_clipped"], rtol=1e-12, atol=0.0, what="clipped")
    assert_close(b["adam_m"] / 0.1, c.desc["grad_plain"], rtol=1e-12, atol=0.0, what="plain")
    assert not np.allclose(a["adam_m"], b["adam_m"]) and a["losses"][0] != b["losses"][0]
    assert a["norms"] == [c.desc["norm"]]
    g = gru_ref.load_ppo("ppo_gru_onestep")
    m = g["meta"]
    r = gru_ref.ppo_update(g["params0"], m["O"], m["A"], m["H"], g, g["recurrent_hidden_states0"], g["perms"], m["ppo_epoch"], m["num_mini_batch"],
                           m["clip_param"], m["value_loss_coef"], m["entropy_coef"], m["lr"], m["eps"], m["max_grad_norm"], use_clipped=True)
    assert_close(r["params"], g["params1"], what="fixture params")


def test_the_arbiter_floor_is_the_float32_distance_of_the_least_saturated_cases():
    """tests/test_gpu_regimes.py's FLOOR: the float32 evaluation's largest block distance from float64 over the off_policy cases."""
    import test_gpu_regimes as tg
    worst = max(max(max(c.desc["o32_clipped"].values()), max(c.desc["o32_plain"].values()))
                for c in (rg.case(*spec) for spec in rg.all_cases() if spec[0] == "off_policy"))
    print("worst float32 block distance over the off_policy cases", worst)
    assert abs(worst / tg.FLOOR - 1.0) <= 0.1   # (libm and BLAS builds move it in the second digit)
