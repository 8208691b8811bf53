"""CPU: the world scope of the diagnostics on the references alone (tests/world_diag_ref.py), and the Python surface that needs no
device.  The arbiter of tests/test_gpu_world_diag.py is the existing float64 reference run once on the concatenated case; here
  - every union case the GPU file uses meets diag_ref.conditions / disc_diag_ref.conditions;
  - the per-rank-then-merge route, restated in float64, equals that one-pass reference to 1e-12 relative;
  - the three ways to get the merge wrong each miss the rule (compare) on the case built to catch it: the ranks' variances
    averaged ("means apart"), the expert part merged across ranks (expert_rows doubles), the local pairing i mod n_e (the wrapped
    case, 11 mod 17 != 0);
  - scope="galaxy" is a ValueError before any device call, and the learners take "world"."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diag_ref as dg  # noqa: E402
import disc_diag_ref as dd  # noqa: E402
import world_diag_ref as wd  # noqa: E402

REL = 1e-12


def rel_close(got, want, names):
    bad = {}
    for k in names:
        a, b = got[k], want[k]
        if np.isnan(a) and np.isnan(b):
            continue
        if not abs(a - b) <= REL * abs(b):
            bad[k] = (a, b)
    return bad


@pytest.mark.parametrize("name", wd.POLICY_CASES)
def test_policy_union_case_meets_the_conditions_and_the_route_is_the_reference(name):
    world, c = wd.policy_case(name)
    got = dg.conditions(c)
    assert got["rows"] == c["T"] * c["N"]
    want, allow = dg.reference(c)
    route = wd.merged_policy(c, world)
    assert not rel_close(route, want, dg.NAMES), rel_close(route, want, dg.NAMES)
    assert route["rows"] == want["rows"] == c["T"] * c["N"] and route["clip_fraction"] == want["clip_fraction"]
    dist = dg.compare(route, want, allow)
    assert all(dist[k] <= 1.0 for k in dg.NAMES), dist


def test_shards_concatenate_to_the_union():
    world, c = wd.policy_case("mlp_7x11_w4")
    shards = [wd.policy_shard(c, r, world) for r in range(world)]
    assert all(s["N"] == 11 and s["T"] == 7 for s in shards)
    for k in ("obs", "actions", "action_log_probs", "value_preds", "returns", "masks"):
        assert np.array_equal(np.concatenate([s[k] for s in shards], axis=1), c[k]), k
    world, d = wd.disc_case("sat_7x16_3x5_e7_w4")
    rows = np.stack([wd.disc_shard_rows(d, r, world).reshape(d.T, 5, d.F) for r in range(world)], axis=1)     # [T, world, N_loc, F]
    assert np.array_equal(rows.reshape(d.T * d.N, d.F), d.policy)


def test_means_apart_is_what_it_says():
    """the two ranks' return means are ~20 apart, their own spreads ~0.01: the between-rank term is all but all of Var(ret), and the
    log-probs are the base case's"""
    world, c = wd.policy_case("means_apart_w2")
    base = dg.gauss_case("mlp", 5, 2, 8, 1, 7, 22, 0, True)
    assert np.array_equal(c["action_log_probs"], base["action_log_probs"]) and np.array_equal(c["params"], base["params"])
    assert np.array_equal(base["returns"][:, :11], c["returns"][:, :11]) and not np.array_equal(base["returns"][:, 11:], c["returns"][:, 11:])
    R = c["returns"][:-1].astype(np.float64)
    within = np.mean([R[:, :11].var(), R[:, 11:].var()])
    assert abs(R[:, 11:].mean() - R[:, :11].mean() - 20.0) < 0.1 and within < 1e-3 and R.var() > 99.0
    assert dg.conditions(c)["clip_fraction"] == dg.conditions(base)["clip_fraction"]


def test_averaging_the_ranks_variances_misses_the_rule_on_means_apart():
    world, c = wd.policy_case("means_apart_w2")
    want, allow = dg.reference(c)
    dist = dg.compare(wd.merged_policy(c, world, fault="avg_var"), want, allow)
    assert dist["explained_variance_old"] > 1.0 and dist["explained_variance_new"] > 1.0, dist
    assert all(dist[k] <= 1.0 for k in dg.NAMES if not k.startswith("explained_variance")), dist


@pytest.mark.parametrize("name", wd.DISC_SPECS)
def test_disc_union_case_meets_the_conditions_and_the_route_is_the_reference(name):
    world, c = wd.disc_case(name)
    dd.conditions(c)
    assert c.seed <= 2, c.tag
    want, allow = wd.disc_reference(c)
    route = wd.merged_disc(c, world)
    assert not rel_close(route, want, dd.NAMES), rel_close(route, want, dd.NAMES)
    assert all(route[k] == want[k] for k in dd.EXACT)
    assert want["policy_rows"] == c.T * c.N and want["expert_rows"] == c.expert.shape[0]
    dist = dd.compare(route, want, allow)
    assert all(dist[k] <= 1.0 for k in dd.NAMES), dist


@pytest.mark.parametrize("name", wd.DISC_SPECS)
def test_an_expert_part_merged_across_ranks_misses_the_rule(name):
    world, c = wd.disc_case(name)
    want, allow = wd.disc_reference(c)
    got = wd.merged_disc(c, world, fault="expert_merged")
    assert got["expert_rows"] == world * c.expert.shape[0]
    assert dd.compare(got, want, allow)["expert_rows"] > 1.0


def test_the_local_pairing_misses_the_rule_on_the_wrapped_case():
    world, c = wd.disc_case("both_7x16_7x11_e17_w2")
    n_loc, n_e = c.N // world, c.expert.shape[0]
    assert n_e < c.T * n_loc and n_loc % n_e != 0 and c.N % n_e != 0
    want, allow = wd.disc_reference(c)
    dist = dd.compare(wd.merged_disc(c, world, fault="local_pairing"), want, allow)
    assert dist["mid_grad_norm_mean"] > 1.0 or dist["mid_grad_pen"] > 1.0, dist
    assert all(dist[k] <= 1.0 for k in dd.NAMES if not (k.startswith("mid_") or k == "grad_norm_max")), dist


# ------------------------------------------------------------------------------------------------- the Python surface
class _NoDevice(object):
    """stands where a library handle would: any use of it is a device call"""
    def __getattr__(self, name):
        raise AssertionError(f"a device call ({name}) before the scope was checked")


def test_an_unknown_scope_is_a_value_error_before_any_device_call():
    import simgan_amd as sg
    from simgan_amd.algo import diagnostics as diag
    assert diag.SCOPES == ("rank", "world")
    agent = types.SimpleNamespace(actor_critic=_NoDevice(), lib=_NoDevice(), clip_param=0.2)
    for bad in ("galaxy", "", None, True, 1, "World"):
        for call in (lambda: diag.run(agent, _NoDevice(), 0.2, scope=bad), lambda: diag.run_disc(_NoDevice(), _NoDevice(), scope=bad),
                     lambda: sg.algo.PPO.diagnostics(agent, _NoDevice(), scope=bad),
                     lambda: sg.algo.A2C_ACKTR.diagnostics(agent, _NoDevice(), scope=bad)):
            with pytest.raises(ValueError, match='scope = .*: "rank" or "world"'):
                call()


class _Recorder(object):
    def __init__(self):
        self.calls = []

    def diagnostics(self, rollouts, fetch=True, slot=None, scope="rank"):
        self.calls.append((fetch, slot, scope))

    def diagnostics_world(self, rollouts, fetch=True, slot=0):
        self.calls.append((fetch, slot, "world"))


def test_the_learners_take_world():
    from simgan_amd import driver
    assert [driver._diag_scope(x, "diagnostics") for x in (False, True, "world")] == [None, "rank", "world"]
    for bad in ("galaxy", "rank", 1, 0):
        with pytest.raises(ValueError, match='diagnostics = .*: False, True .* or "world"'):
            driver._diag_scope(bad, "diagnostics")
    for cls in (driver.GailDynLearner, driver.PpoLearner):
        me = object.__new__(cls)
        me.agent, me.rollouts = _Recorder(), None
        me._queue_diagnostics("world")
        me._queue_diagnostics()
        assert me.agent.calls == [(False, None, "world"), (False, None, "rank")] and me._diag_pending
    me = object.__new__(driver.GailDynLearner)
    me.discr, me.rollouts = _Recorder(), None
    me._queue_disc_diagnostics(0, "world")
    assert not me._ddiag_pending
    me._queue_disc_diagnostics(1, "world")
    assert me.discr.calls == [(False, 0, "world"), (False, 1, "world")] and me._ddiag_pending
    me._queue_disc_diagnostics(0)
    assert me.discr.calls[-1] == (False, 0, "rank") and not me._ddiag_pending
    # an argument that is neither is refused before the update touches anything
    for cls, kw in ((driver.GailDynLearner, {"disc_diagnostics": "galaxy"}), (driver.GailDynLearner, {"diagnostics": "galaxy"}),
                    (driver.PpoLearner, {"diagnostics": "galaxy"})):
        me = object.__new__(cls)
        me.rollouts = types.SimpleNamespace(lib=None)
        with pytest.raises(ValueError, match="galaxy"):
            me.update(**kw)
