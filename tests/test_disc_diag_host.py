"""CPU: the float64 reference of the discriminator diagnostics (tests/disc_diag_ref.py) judged on its own -- the cases reach what
they claim, the closed-form input gradient equals autograd, every wrong restatement of a statistic fails the rule on at least one
case, and no allowance is wide enough to hide one.  The library half (names, ctypes, the learner's plumbing) is looked at as far
as a machine without a GPU can."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import disc_diag_ref as dd  # noqa: E402


@pytest.mark.parametrize("name", dd.CASES)
def test_conditions_hold(name):
    c = dd.case(name)
    m = dd.conditions(c)
    print(c.tag, m)
    assert c.policy.shape == (c.T * c.N, c.F) and c.expert.shape[1] == c.F
    assert c.policy.dtype == np.float32 and c.expert.dtype == np.float32 and c.params.dtype == np.float32
    if c.regime == "saturated":
        assert m["reward_abs_max"] >= 6.0, (c.tag, m)
    if name != "zero_head":
        F, Hd, T, N, n_e, regime, _ = dd.SPECS[name]
        assert (c.F, c.Hd, c.T, c.N, c.expert.shape[0], c.regime) == (F, Hd, T, N, n_e, regime)


def test_the_case_list_covers_what_it_claims():
    specs = dd.SPECS.values()
    assert {(s[0], s[1]) for s in specs} == {(7, 16), (86, 100), (150, 256)}
    assert {s[2] * s[3] for s in specs} >= {1, 16, 17, 77, 130}
    assert {s[4] for s in specs} >= {1, 16, 17, 100}
    assert {s[5] for s in specs} == set(dd.rg.SCALES)
    assert any(s[4] == 200 and s[2] * s[3] == 77 for s in specs), "n_e > T*N: no wrap"
    assert any(s[4] == 17 and s[2] * s[3] == 130 for s in specs), "n_e < T*N: the pairing wraps"
    assert dd.SPECS["both_7x16_large"][2:5] == (129, 520, 1000)
    a = dd.reference(dd.case("both_86x100_7x11_e100_shifted"))[0]
    assert a["policy_accuracy"] != a["expert_accuracy"] and abs(a["policy_accuracy"] - 0.5) > 0.05 and abs(a["expert_accuracy"] - 0.5) > 0.05, a


@pytest.mark.parametrize("name", dd.CASES)
def test_closed_form_gradient_equals_autograd(name):
    c = dd.case(name)
    for x in (c.policy, c.expert, dd.mid_rows(c.expert, c.policy)):
        a, b = dd.gnorm_autograd(c.params, c.F, c.Hd, x), dd.gnorm_closed(c.params, c.F, c.Hd, x)
        assert a.shape == b.shape == (x.shape[0],)
        assert np.abs(a - b).max() <= 1e-9, (c.tag, float(np.abs(a - b).max()))


def test_mid_rows_pair_expert_i_mod_n_e():
    c = dd.case("both_7x16_10x13_e17")
    mid = dd.mid_rows(c.expert, c.policy)
    assert np.array_equal(mid[17 + 3], np.float32(0.5) * c.expert[3] + np.float32(0.5) * c.policy[20])
    assert np.array_equal(mid[129], np.float32(0.5) * c.expert[129 % 17] + np.float32(0.5) * c.policy[129])


@pytest.mark.parametrize("fault", sorted(dd.FAULTS))
def test_every_fault_fails_the_rule_on_some_case(fault):
    """The reference with one statistic restated wrongly, judged as the kernels are: the statistic the fault breaks misses the
    rule on at least one case."""
    caught = []
    for name in dd.CASES:
        c = dd.case(name)
        want, allow = dd.reference(c)
        got, _ = dd.reference(c, fault=fault)
        dist = dd.compare(got, want, allow)
        if not dist[dd.FAULTS[fault]] <= 1.0:
            caught.append((name, dist[dd.FAULTS[fault]]))
    print(fault, "->", dd.FAULTS[fault], caught)
    assert caught, f"{fault}: {dd.FAULTS[fault]} stays within the rule on every case"


@pytest.mark.parametrize("name", dd.CASES)
def test_allowances_are_not_vacuous(name):
    """A cap on the test, not a measurement: for every statistic that is not exact, allowance <= 0.05 max(|statistic|, 1); the exact
    ones have none.  And the reference against itself is at distance 0."""
    want, allow = dd.reference(dd.case(name))
    assert tuple(want) == dd.NAMES and tuple(allow) == dd.NAMES
    for k in dd.NAMES:
        assert np.isfinite(want[k]) and np.isfinite(allow[k]) and allow[k] >= 0.0, (k, want[k], allow[k])
        if k in dd.EXACT:
            assert allow[k] == 0.0
        else:
            assert allow[k] <= dd.CAP * max(abs(want[k]), 1.0), (name, k, allow[k], want[k])
    assert max(dd.compare(want, want, allow).values()) == 0.0


def test_rule_is_exact_where_it_says_so():
    want, allow = dd.reference(dd.case("both_7x16_7x11_e200"))
    for k in dd.EXACT:
        got = dict(want)
        got[k] = want[k] + 1.0 / 77.0
        assert dd.compare(got, want, allow)[k] == np.inf
    got = dict(want)
    got["policy_bce"] = want["policy_bce"] * (1.0 + 3e-4) + 3.0 * allow["policy_bce"]
    assert dd.compare(got, want, allow)["policy_bce"] > 1.0


def test_names_and_prototypes_of_the_library():
    from simgan_amd import _lib
    from simgan_amd.algo import diagnostics
    assert diagnostics.DISC_NAMES == dd.NAMES and len(dd.NAMES) == 19
    text = open(os.path.join(ROOT, "include", "simgan_hip.h")).read()
    assert "#define SG_DDIAG_N 19" in text
    assert "sg_disc_diagnostics" in _lib.PROTOTYPES and "sg_disc_diagnostics_fetch" in _lib.PROTOTYPES
    from simgan_amd.algo.gail import Discriminator
    from simgan_amd.driver import GailDynLearner
    assert callable(Discriminator.diagnostics) and callable(Discriminator.last_diagnostics)
    assert isinstance(GailDynLearner.last_disc_diagnostics, property)
    import inspect
    sig = inspect.signature(GailDynLearner.update)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [("diagnostics", False), ("disc_diagnostics", False)]
    assert [(p.name, p.default) for p in inspect.signature(Discriminator.diagnostics).parameters.values()][1:] == \
        [("rollouts", inspect.Parameter.empty), ("fetch", True), ("slot", 0)]
