"""CPU: the numpy restatement of mirror-augmented rollouts (tests/dup_sym_ref.py) against what the reference's own rollout
fill wrote (tests/golden/dup_sym_*.npz, tools/gen_golden_dup_sym.py: a2c/main.py:181-245 with --dup-sym), and the host
arithmetic of simgan_amd.symmetry.matrix_rows against a sequential float64 sum.  No device call."""
import numpy as np
import pytest

import dup_sym_ref as ref
from helpers import load

FIXTURES = ("dup_sym_laikago", "dup_sym_dense")


def fixture(name):
    g = load(name)
    steps = {k: g["step_" + k] for k in ref.STEP_KEYS}
    return g, steps


def restated(name, variant=None):
    g, steps = fixture(name)
    return g, ref.restate(g["obs0"], g["feat0"], steps, g["m_obs"], g["m_act"], hidden=g["meta"]["hidden"], variant=variant)


def mismatches(g, out, name):
    """Fields of the restatement that differ from the fixture: bit for bit on the Laikago one (rows of at most two non-zero
    entries: no summation order to differ in), within float32 rounding of the float64 sum on the dense one (the reference sums
    through numpy's matrix product, whose order is its own)."""
    bad = []
    for k in ref.FIELDS:
        want, got = g["out_" + k], out[k]
        assert want.shape == got.shape, (k, want.shape, got.shape)
        if name == "dup_sym_laikago":
            ok = np.array_equal(want, got)
        else:
            ok = np.all(np.abs(want.astype(np.float64) - got) <= 2.0 ** -23 * np.abs(want) + 1e-12)
        if not ok:
            bad.append(k)
    return bad


def test_fixture_shapes_are_the_issue_s():
    a, b = load("dup_sym_laikago")["meta"], load("dup_sym_dense")["meta"]
    assert (a["O"], a["A"], a["T"], a["n"]) == (37, 12, 3, 2) and (b["O"], b["A"], b["T"], b["n"]) == (5, 2, 3, 3)
    for name in FIXTURES:
        g = load(name)
        n = g["meta"]["n"]
        assert g["out_obs"].shape[1] == 2 * n and g["feat0"].shape[1] == g["meta"]["O"]
    d = load("dup_sym_dense")
    for m in (d["m_obs"], d["m_act"]):     # neither symmetric nor an involution
        assert not np.allclose(m, m.T) and not np.allclose(m @ m, np.eye(len(m)), atol=1e-3)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference_rollout(name):
    g, out = restated(name)
    assert mismatches(g, out, name) == []
    n = g["meta"]["n"]
    assert np.array_equal(out["obs_feat"][:, n:], out["obs_feat"][:, :n])            # repeated, not mirrored
    assert not np.array_equal(out["obs"][:, n:], out["obs"][:, :n])


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("variant,field", [("mirror_feat", "obs_feat"), ("repeat_actions", "actions"), ("transpose_act", "actions")])
def test_wrong_restatements_fail_against_the_fixtures(name, variant, field):
    """Test of the test: mirroring obs_feat as well, repeating the actions unmirrored and M_act transposed are each caught."""
    if variant == "transpose_act" and name == "dup_sym_laikago":
        # the Laikago action mirror swaps pairs: it is its own transpose, so only the dense fixture can tell
        g = load(name)
        assert np.array_equal(g["m_act"], g["m_act"].T)
        return
    g, out = restated(name, variant)
    assert mismatches(g, out, name) == [field]


def test_host_arithmetic_is_a_sequential_float64_sum_cast_once():
    from simgan_amd import symmetry
    rng = np.random.default_rng(3)
    for w, rows in ((5, 7), (37, 4), (111, 3)):
        m = rng.standard_normal((w, w)).astype(np.float32)
        x = rng.standard_normal((rows, w)).astype(np.float32)
        want = np.cumsum(m.astype(np.float64)[None] * x.astype(np.float64)[:, None, :], axis=-1)[..., -1].astype(np.float32)
        got = symmetry.matrix_rows(m, x)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert np.array_equal(ref.mirror(m, x), want)                   # the tests' arbiter is the same sum
        assert np.all(np.abs(got.astype(np.float64) - ref.mirror64(m, x)) <= ref.mirror_bound(m, x))


def test_host_arithmetic_skips_zero_entries_and_is_exact_for_a_signed_permutation():
    from simgan_amd import symmetry
    rng = np.random.default_rng(4)
    m = ref.signed_permutation(rng, 9)
    x = rng.standard_normal((6, 9)).astype(np.float32)
    x[0, 3] = np.inf                                  # 0 * inf would poison every output of the row if zeros were not skipped
    got = symmetry.matrix_rows(m, x)
    want = np.stack([np.array([m[i, np.flatnonzero(m[i])[0]] * r[np.flatnonzero(m[i])[0]] for i in range(9)]) for r in x]).astype(np.float32)
    assert np.array_equal(got, want) and np.isinf(got[0]).sum() == 1
    lo, la = symmetry.laikago_mirror(37)
    y = rng.standard_normal((5, 12)).astype(np.float32)
    assert np.array_equal(symmetry.matrix_rows(la, y), y[:, [3, 4, 5, 0, 1, 2, 9, 10, 11, 6, 7, 8]])
