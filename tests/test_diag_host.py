"""CPU: the float64 reference of the update diagnostics (tests/diag_ref.py) held against the formulas written out literally, the
defects it must catch shown failing on the references alone, the conditions of every case tests/test_gpu_diag.py runs, and the
two entry points in the header and in the built library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diag_ref as dg  # noqa: E402


def hand_made():
    """three rows, every number chosen by hand: one ratio inside the clip, one above, one below"""
    lpn = np.array([-1.0, -2.0, -0.5])
    lpo = np.array([-1.1, -1.5, -0.9])
    ent = np.array([1.5, 1.25, 2.0])
    v = np.array([0.5, -1.0, 2.0])
    vp = np.array([0.25, -0.5, 1.0])
    ret = np.array([1.0, -2.0, 3.0])
    return lpn, ent, v, lpo, vp, ret


def test_helper_matches_the_formulas_written_out():
    lpn, ent, v, lpo, vp, ret = hand_made()
    got = dg.statistics(lpn, ent, v, lpo, vp, ret, 0.2)
    r = np.exp(lpn - lpo)
    want = {"rows": 3.0,
            "approx_kl": ((-1.1 + 1.0) + (-1.5 + 2.0) + (-0.9 + 0.5)) / 3.0,
            "approx_kl_k3": np.mean((r - 1.0) - np.log(r)),
            "clip_fraction": 2.0 / 3.0,          # exp(0.1) - 1 = 0.105 inside; exp(-0.5) - 1 = -0.39 and exp(0.4) - 1 = 0.49 beyond
            "entropy": (1.5 + 1.25 + 2.0) / 3.0,
            "ratio_min": np.exp(-0.5), "ratio_max": np.exp(0.4),
            "explained_variance_old": 1.0 - np.var(ret - vp) / np.var(ret),
            "explained_variance_new": 1.0 - np.var(ret - v) / np.var(ret),
            "value_mse": (0.5 ** 2 + 1.0 ** 2 + 1.0 ** 2) / 3.0}
    assert tuple(got) == dg.NAMES
    for k in dg.NAMES:
        assert abs(got[k] - want[k]) <= 1e-14 * max(1.0, abs(want[k])), (k, got[k], want[k])
    # numpy's variance is the population variance about the mean: the two explained variances written out once more
    e = ret - v
    assert abs(want["explained_variance_new"] - (1.0 - np.mean((e - e.mean()) ** 2) / np.mean((ret - ret.mean()) ** 2))) <= 1e-15


def test_one_row_has_nan_explained_variances_like_numpy():
    s = dg.statistics([-1.0], [1.0], [0.5], [-1.2], [0.4], [1.0])
    with np.errstate(all="ignore"):
        assert np.isnan(1.0 - np.var(np.array([0.5])) / np.var(np.array([1.0])))
    assert np.isnan(s["explained_variance_old"]) and np.isnan(s["explained_variance_new"]) and s["rows"] == 1.0


def _fails(name, fault, clip=dg.CLIP):
    c = dg.case(name)
    want, allow = dg.reference(c, clip)
    bad, _ = dg.reference(c, clip, fault=fault)
    return dg.compare(bad, want, allow)


def test_swapped_kl_sign_fails():
    d = _fails("mlp_77", "kl_sign")
    assert d["approx_kl"] > 100.0 and all(v == 0.0 for k, v in d.items() if k != "approx_kl"), d


def test_exchanged_value_arguments_fail():
    d = _fails("mlp_77", "swap_v")
    assert d["explained_variance_old"] > 10.0 and d["explained_variance_new"] > 10.0 and d["value_mse"] > 10.0, d


def test_greater_or_equal_in_the_clip_flag_fails_with_a_row_on_the_edge():
    lpn, ent, v, lpo, vp, ret = hand_made()
    clip = abs(float(np.exp(np.float64(lpn[0] - lpo[0]))) - 1.0)      # row 0 exactly at the edge, in float64
    good = dg.statistics(lpn, ent, v, lpo, vp, ret, clip)
    bad = dg.statistics(lpn, ent, v, lpo, vp, ret, clip, fault="clip_ge")
    assert good["clip_fraction"] == 2.0 / 3.0 and bad["clip_fraction"] == 1.0
    assert dg.compare(bad, good, dg.allowances(lpn, ent, v, lpo, vp, ret, clip))["clip_fraction"] == np.inf


def test_variance_about_zero_fails_on_returns_far_from_zero():
    c = dg.case("mlp_far_returns")
    _, _, R = dg.rollout_rows(c)
    assert abs(R.mean()) >= 900.0 * R.std(), (R.mean(), R.std())
    d = _fails("mlp_far_returns", "var_about_zero")
    assert d["explained_variance_old"] > 1000.0 and d["explained_variance_new"] > 1.0, d
    # ... and the one-pass float64 form E[x^2] - E[x]^2 carried out in float32 has nothing left of this variance at all
    r32 = R.astype(np.float32)
    one_pass = float(np.mean(r32 * r32, dtype=np.float32) - np.mean(r32, dtype=np.float32) ** 2)
    assert abs(one_pass - R.var()) > 0.01 * R.var()


@pytest.mark.parametrize("name", sorted(dg.CASES))
def test_conditions_hold_for_every_gpu_case(name):
    c = dg.case(name)
    out = dg.conditions(c)
    assert out["rows"] == c["T"] * c["N"]
    want, allow = dg.reference(c)
    assert want["rows"] == out["rows"] and want["clip_fraction"] == out["clip_fraction"]
    assert dg.compare(want, want, allow) == {k: 0.0 for k in dg.NAMES}
    if out["rows"] > 1:
        assert all(np.isfinite(want[k]) and np.isfinite(allow[k]) for k in dg.NAMES), (want, allow)
        assert want["ratio_min"] < 1.0 - dg.CLIP and want["ratio_max"] > 1.0 + dg.CLIP


def test_geometries_reach_the_tile_classes():
    """T*N = 1, 16 -> 16-row tiles; 17 -> one ragged 32-row tile; 33 -> 64-row tiles with one row in the second; 77, 130 -> 64-row
    tiles with a ragged last one (csrc/sg_policy_fwd.hpp: fwd_tile_mt; tests/test_gpu_act_step.py's header)"""
    assert [t * n for t, n in dg.GEOMETRIES] == [1, 16, 17, 77, 130]
    c = dg.case("split_33")
    assert c["T"] * c["N"] == 33


def test_header_declares_the_entries_and_the_library_exports_them():
    from simgan_amd import _lib
    text = open(os.path.join(ROOT, "include", "simgan_hip.h")).read()
    for name in ("sg_rollout_policy_diagnostics", "sg_rollout_policy_diagnostics_fetch"):
        assert re.search(r"SG_API\s+int\s+" + name + r"\s*\(", text), f"{name} is not declared in include/simgan_hip.h"
        assert name in _lib.PROTOTYPES, f"{name} has no prototype in simgan_amd/_lib.py"
        lib = ctypes.CDLL(_lib.LIB_PATH)
        assert hasattr(lib, name), f"{name} is not exported by {_lib.LIB_PATH}"
    assert re.search(r"#define\s+SG_DIAG_N\s+10\b", text)
