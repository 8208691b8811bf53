"""GPU: update diagnostics on the device -- sg_rollout_policy_diagnostics / PPO.diagnostics, A2C_ACKTR.diagnostics and the
learners' update(diagnostics=True) -- against the float64 reference of tests/diag_ref.py under its rule: a statistic passes if
|hip - f64| <= 1e-4 |f64| + allowance; `rows` and `clip_fraction` are exact (diag_ref: THE RULE, CONDITIONS).

Which launch instance a row count reaches (csrc/sg_policy_fwd.hpp: fwd_tile_mt, followed by the launcher): T*N <= 16 -> 16-row
tiles <1>; 17..32 -> 32-row tiles <2>; >= 33 -> 64-row tiles <4>.  1 and 16 hit <1> (1: one live lane, NaN explained variances);
17 hits <2> with a ragged tile; 33 hits <4> with one row in the second workgroup; 77 and 130 hit <4> with a ragged last tile;
67,080 rows are 1,049 records, 17 per lane of the reduce.  Each with the weights in LDS, or -- SG_POLICY_GW=1, or a hidden width
of 256, whose trunk does not fit LDS -- read from global memory.  The kernel takes one tile per workgroup and its grid is not
capped, so there is no loop over tiles to reach.  The queued form is not captured into a graph, so SG_PPO_GRAPH has nothing to
change around it.

SG_DIAG_RECORD=<path> collects, per statistic, the worst ratio of distance to bound over all cases (profiles/diag_parity.json)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diag_ref as dg  # noqa: E402
import discrete_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu

LR, EPS = 3e-4, 1e-5
WORST = {}


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    yield simgan_amd
    path = os.environ.get("SG_DIAG_RECORD")
    if path and WORST:
        doc = {"what": "tests/test_gpu_diag.py under SG_DIAG_RECORD: per statistic, the worst |hip - float64| / (1e-4 |float64| + allowance) "
                       "over all cases, and the case it was seen on; rows and clip_fraction are exact (0)",
               "cases": len({c for v in WORST.values() for c in v["seen"]}),
               "worst": {k: {"ratio": v["ratio"], "case": v["case"]} for k, v in WORST.items()}}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)


def space_of(c):
    return dr.Box((c["A"],)) if c["kind"] in ("mlp", "split", "gru") else dr.space(c["dist"], c["K"])


def make_policy(sg, c, params=None):
    if c["kind"] == "split":
        p = sg.SplitPolicy((c["O"],), space_of(c), base_kwargs={"hidden_size": c["H"], "num_feet": c["f"]})
    else:
        p = sg.Policy((c["O"],), space_of(c), base_kwargs={"recurrent": c["kind"] == "gru", "hidden_size": c["H"]})
    assert [(n, tuple(s)) for n, s in p.param_shapes()] == [(n, tuple(s)) for n, s in c["shapes"]]
    p.set_flat_params(np.asarray(c["params"] if params is None else params, np.float32))
    return p


def make_rollout(sg, c, resident=True, hidden_on_device=False, F=1):
    H = c["H"] if c["kind"] == "gru" else 1
    ro = sg.RolloutStorage(c["T"], c["N"], (c["O"],), space_of(c), H, F)
    if F > 1:
        ro.obs_feat.copy_(ro.obs_feat.new_tensor(np.random.default_rng(3).standard_normal(tuple(ro.obs_feat.shape)).astype(np.float32)))
    for name in ("obs", "actions", "action_log_probs", "value_preds", "returns", "masks"):
        t = getattr(ro, name)
        t.copy_(t.new_tensor(np.asarray(c[name]).reshape(tuple(t.shape))))
    if c["kind"] == "gru":
        ro.recurrent_hidden_states[0].copy_(ro.recurrent_hidden_states.new_tensor(c["hxs0"]))
    if resident:
        ro.device_resident = True
        ro.sync_to_device()
        if hidden_on_device:
            ro.enable_device_hidden()
    return ro


def ppo(sg, pol, clip=dg.CLIP, epochs=1, mb=1, lr=LR):
    return sg.algo.PPO(pol, clip, epochs, mb, 0.5, 0.01, lr=lr, eps=EPS, max_grad_norm=0.5)


def judge(label, got, c, clip=dg.CLIP, params=None):
    want, allow = dg.reference(c, clip, params)
    dist = dg.compare(got, want, allow)
    for k, x in dist.items():
        w = WORST.setdefault(k, {"ratio": 0.0, "case": label, "seen": set()})
        w["seen"].add(label)
        if np.isfinite(x) and x > w["ratio"]:
            w["ratio"], w["case"] = float(x), label
    print(label, {k: (got[k], want[k], allow[k], round(dist[k], 4)) for k in dg.NAMES})
    bad = {k: (got[k], want[k], allow[k], dist[k]) for k in dg.NAMES if not dist[k] <= 1.0}
    assert not bad, f"{label}: (hip, float64, allowance, distance / bound) {bad}"
    return want, allow


def same(a, b):
    """two result dicts, bit for bit (NaN equal to NaN)"""
    return all(np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64) for k in dg.NAMES)


FEED_FORWARD = [n for n in dg.CASES if not n.startswith("gru")]


@pytest.mark.parametrize("name", FEED_FORWARD)
def test_feed_forward_against_float64(sg, name):
    c = dg.case(name)
    pol, ro = make_policy(sg, c), make_rollout(sg, c)
    got = ppo(sg, pol).diagnostics(ro)
    assert tuple(got) == dg.NAMES
    want, _ = judge(name, got, c)
    assert got["rows"] == c["T"] * c["N"] and got["clip_fraction"] == want["clip_fraction"]
    if c["T"] * c["N"] == 1:
        assert np.isnan(got["explained_variance_old"]) and np.isnan(got["explained_variance_new"])


@pytest.mark.parametrize("name", ["mlp_77", "mlp_16", "split_77"])
def test_forced_global_weight_path(sg, name, monkeypatch):
    c = dg.case(name)
    pol, ro = make_policy(sg, c), make_rollout(sg, c)
    agent = ppo(sg, pol)
    lds = agent.diagnostics(ro)
    monkeypatch.setenv("SG_POLICY_GW", "1")
    gw = agent.diagnostics(ro)
    monkeypatch.delenv("SG_POLICY_GW")
    judge(name + " SG_POLICY_GW=1", gw, c)
    assert gw["clip_fraction"] == lds["clip_fraction"] and gw["rows"] == lds["rows"]


@pytest.mark.parametrize("name", ["gru_9_17", "gru_5_1"])
def test_recurrent_against_float64_and_both_hidden_sources(sg, name):
    c = dg.case(name)
    assert (c["masks"][0] == 0).any() and (name != "gru_9_17" or (c["masks"][1:c["T"]] == 0).any())
    pol = make_policy(sg, c)
    host_h = ppo(sg, pol).diagnostics(make_rollout(sg, c))                               # hxs0 handed over from the host
    judge(name + " host hidden", host_h, c)
    dev_h = ppo(sg, pol).diagnostics(make_rollout(sg, c, hidden_on_device=True))         # hidden slot 0 of the device rollout
    assert same(host_h, dev_h), (host_h, dev_h)
    drop_in = ppo(sg, pol).diagnostics(make_rollout(sg, c, resident=False))
    assert same(host_h, drop_in), (host_h, drop_in)


@pytest.mark.parametrize("name", ["mlp_130", "split_33", "discrete_17"])
def test_same_bits_in_every_form(sg, name):
    c = dg.case(name)
    pol = make_policy(sg, c)
    agent, ro = ppo(sg, pol), make_rollout(sg, c)
    first = agent.diagnostics(ro)
    assert same(first, agent.diagnostics(ro)), "two calls"
    assert agent.diagnostics(ro, fetch=False) is None
    assert same(first, agent.last_diagnostics()), "fetch=False + last_diagnostics()"
    with pytest.raises(RuntimeError, match="no diagnostics are pending"):
        agent.last_diagnostics()
    host_ro = make_rollout(sg, c, resident=False)
    assert same(first, ppo(sg, pol).diagnostics(host_ro)), "host-resident rollout"
    assert same(first, ppo(sg, pol).diagnostics(host_ro)), "host-resident rollout, nothing stale to push"


def test_on_policy_right_after_a_collection(sg):
    """Collected by act_step with the parameters the diagnostics then see: N = 17 and T*N = 68 both sum on the side of the 32- and
    64-row tiles, so the new log-probs repeat the collection's; KL and k3 are within their allowance of 0 either way."""
    T, N, O, A, H = 4, 17, 5, 2, 8
    base = dg.gauss_case("mlp", O, A, H, 1, T, N)
    c = dict(base)
    pol = make_policy(sg, c, c["behaviour"])
    ro = sg.RolloutStorage(T, N, (O,), dr.Box((A,)), 1, 1)
    ro.device_resident = True
    ro.obs.copy_(ro.obs.new_tensor(c["obs"]))
    ro.returns.copy_(ro.returns.new_tensor(c["returns"]))
    ro.sync_to_device()
    for t in range(T):
        ro.act_step(pol)
        ro.insert_env(c["obs"][t + 1], np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32), np.ones((N, 1), np.float32),
                      np.zeros((N, 1), np.float32))
    ro.finish_collect()
    got = ppo(sg, pol).diagnostics(ro)
    ro.sync_from_device()
    for k in ("actions", "action_log_probs", "value_preds", "returns"):
        c[k] = np.array(getattr(ro, k).numpy())
    c["params"] = c["behaviour"]
    want, allow = judge("on-policy", got, c)
    assert abs(got["approx_kl"]) <= allow["approx_kl"] and abs(got["approx_kl_k3"]) <= allow["approx_kl_k3"], (got, allow)
    assert got["clip_fraction"] == 0.0 and want["clip_fraction"] == 0.0


def test_after_one_real_ppo_update(sg):
    c = dg.case("mlp_77")
    pol, ro = make_policy(sg, c), make_rollout(sg, c)
    agent = ppo(sg, pol, epochs=2, mb=2, lr=3e-3)
    before = agent.diagnostics(ro)
    agent.update(ro)
    got = agent.diagnostics(ro)
    params = pol.get_flat_params()
    assert not np.array_equal(params, c["params"]) and not same(before, got)
    v, lp, _ = dg.evaluate(c, params)
    edge = np.min(np.abs(np.abs(np.exp(lp - dg.rollout_rows(c)[0]) - 1.0) - dg.CLIP))
    assert edge >= dg.EDGE * dg.CLIP, f"the update left a row {edge:.2e} from the clip edge: the flag count is not decidable in float32"
    judge("after PPO.update", got, c, params=params)


@pytest.mark.parametrize("acktr", [False, True])
def test_a2c_acktr_diagnostics(sg, acktr):
    c = dict(dg.case("mlp_77"))
    pol, ro = make_policy(sg, c), make_rollout(sg, c)
    if acktr:
        agent = sg.algo.A2C_ACKTR(pol, 0.5, 0.01, acktr=True)
    else:
        agent = sg.algo.A2C_ACKTR(pol, 0.5, 0.01, lr=7e-4, eps=EPS, alpha=0.99, max_grad_norm=0.5)
    got = agent.diagnostics(ro)
    want, _ = judge(f"A2C_ACKTR(acktr={acktr})", got, c, clip=np.inf)
    assert got["clip_fraction"] == 0.0 and want["clip_fraction"] == 0.0
    assert same(got, ppo(sg, pol).diagnostics(ro) | {"clip_fraction": 0.0})      # the other nine do not depend on the clip
    if acktr:   # from the on-policy point, one K-FAC step: the measured KL to set beside kl_clip
        c["action_log_probs"] = dg.evaluate(c, c["behaviour"])[1].reshape(c["T"], c["N"], 1).astype(np.float32)
        pol.set_flat_params(c["behaviour"])
        ro = make_rollout(sg, c)
        start = agent.diagnostics(ro)
        agent.update(ro)
        moved = agent.diagnostics(ro)
        assert abs(start["approx_kl"]) < 1e-5 and start["ratio_max"] - start["ratio_min"] < 1e-4, start
        assert np.isfinite(moved["approx_kl"]) and moved["approx_kl"] > 1e-5 and moved["approx_kl_k3"] > 1e-5, moved
        judge("after ACKTR update", moved, c, clip=np.inf, params=pol.get_flat_params())


def _learner(sg, c):
    from simgan_amd.driver import PpoLearner
    pol, ro = make_policy(sg, c), make_rollout(sg, c)
    agent = ppo(sg, pol, epochs=2, mb=2)
    return PpoLearner(pol, agent, ro), pol, agent, ro


@pytest.mark.parametrize("resident", [True, False])
def test_ppo_learner_update_with_diagnostics(sg, resident):
    from simgan_amd import driver
    c = dg.case("mlp_130")
    runs = []
    for diagnostics in (False, True):
        learner, pol, agent, ro = _learner(sg, c)
        if not resident:
            ro.device_resident = False
        losses = learner.update(diagnostics=diagnostics)
        runs.append(([np.float32(losses[k]) for k in ("value_loss", "action_loss", "dist_entropy")], pol.get_flat_params(), learner))
    assert [x.view(np.uint32) for x in runs[0][0]] == [x.view(np.uint32) for x in runs[1][0]], "losses"
    assert np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32)), "parameters"
    assert runs[0][2].last_diagnostics is None
    got = runs[1][2].last_diagnostics
    assert got is runs[1][2].last_diagnostics and tuple(got) == dg.NAMES
    # the direct call at the same point: after the agent's update, before after_update
    learner, pol, agent, ro = _learner(sg, c)
    if resident:
        driver._returns_resident(learner)
        agent.update(ro, fetch_losses=False)
    else:
        ro.device_resident = False
        ro.compute_returns(pol.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]), True, 0.99, 0.95, True)
        agent.update(ro)
    assert same(got, agent.diagnostics(ro))


@pytest.mark.parametrize("resident", [True, False])
def test_gail_dyn_learner_update_with_diagnostics(sg, resident):
    from simgan_amd.driver import GailDynLearner
    c, F = dg.case("mlp_130"), 6
    expert = np.random.default_rng(4).standard_normal((64, F)).astype(np.float32)
    runs = []
    for diagnostics in (False, True):
        pol, ro = make_policy(sg, c), make_rollout(sg, c, resident=resident, F=F)
        disc, agent = sg.algo.gail.Discriminator(F, 16, None, seed=2), ppo(sg, pol, epochs=2, mb=2)
        disc.seed, agent.seed = 11, 12
        learner = GailDynLearner(pol, agent, disc, ro, expert, gail_batch_size=16, gail_epoch=2, gail_tar_length=5.0)
        losses = learner.update(diagnostics=diagnostics)
        runs.append(({k: np.float32(losses[k]).view(np.uint32) for k in losses}, pol.get_flat_params(), disc.get_flat_params(), learner))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) == 7, (runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32)), "policy parameters"
    assert np.array_equal(runs[0][2].view(np.uint32), runs[1][2].view(np.uint32)), "discriminator parameters"
    got = runs[1][3].last_diagnostics
    assert runs[0][3].last_diagnostics is None and tuple(got) == dg.NAMES and got["rows"] == 130.0
    assert all(np.isfinite(got[k]) for k in dg.NAMES) and 0.0 < got["clip_fraction"] < 1.0, got


def _everything(ro, pol):
    from simgan_amd import _lib
    out = {"params": pol.get_flat_params().copy()}
    T, N = ro.num_steps, ro.num_processes
    shapes = {_lib.F_OBS: (T + 1, N, ro.obs_dim), _lib.F_OBS_FEAT: (T + 1, N, ro.feat_len), _lib.F_ACTIONS: (T, N, ro.act_dim),
              _lib.F_REWARDS: (T, N, 1), _lib.F_VALUE_PREDS: (T + 1, N, 1), _lib.F_RETURNS: (T + 1, N, 1), _lib.F_LOGP: (T, N, 1),
              _lib.F_MASKS: (T + 1, N, 1), _lib.F_BAD_MASKS: (T + 1, N, 1), _lib.F_ADVANTAGES: (T, N, 1)}
    for f, shape in shapes.items():
        a = np.zeros(shape, np.float32)
        _lib.check(ro.lib.sg_rollout_download(ro.h, f, _lib.fptr(a), a.size))
        out[f] = a
    if getattr(ro, "device_hidden", False):
        h = np.zeros(tuple(ro.recurrent_hidden_states.shape), np.float32)
        _lib.check(ro.lib.sg_rollout_download_hidden(ro.h, _lib.fptr(h), h.size))
        out["hidden"] = h
    return out


@pytest.mark.parametrize("name", ["split_77", "gru_9_17"])
def test_nothing_but_the_result_is_written(sg, name):
    c = dg.case(name)
    pol, ro = make_policy(sg, c), make_rollout(sg, c, hidden_on_device=name.startswith("gru"))
    agent = ppo(sg, pol)
    agent.update(ro)                                        # (the advantages field holds something)
    before = _everything(ro, pol)
    agent.diagnostics(ro)
    agent.diagnostics(ro, fetch=False)
    agent.last_diagnostics()
    after = _everything(ro, pol)
    assert before.keys() == after.keys()
    for k in before:
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k


def test_refusals(sg):
    from simgan_amd import _lib
    c = dg.case("mlp_16")
    pol, ro = make_policy(sg, c), make_rollout(sg, c)
    lib, out = ro.lib, (C.c_double * 10)()
    err = _lib.SimganHipError
    with pytest.raises(err, match="no diagnostics are pending"):
        _lib.check(lib.sg_rollout_policy_diagnostics_fetch(ro.h, out))
    _lib.check(lib.sg_rollout_policy_diagnostics(ro.h, pol.h, 0.2, None, out))     # the synchronous form leaves nothing pending
    with pytest.raises(err, match="no diagnostics are pending"):
        _lib.check(lib.sg_rollout_policy_diagnostics_fetch(ro.h, out))
    for clip in (0.0, -0.2, float("nan"), float("-inf")):
        with pytest.raises(err, match="clip_param = .*must be positive"):
            _lib.check(lib.sg_rollout_policy_diagnostics(ro.h, pol.h, clip, None, out))
    wide = sg.RolloutStorage(2, 8, (c["O"] + 1,), dr.Box((c["A"],)), 1, 1)
    with pytest.raises(err, match=r"policy/rollout dims differ \(obs 5 vs 6, action 2 vs 2\)"):
        ppo(sg, pol).diagnostics(wide)
    g = dg.case("gru_5_1")
    gpol, gro = make_policy(sg, g), make_rollout(sg, g)
    with pytest.raises(err, match="recurrent and the rollout holds no hidden states.*hxs0_host"):
        _lib.check(lib.sg_rollout_policy_diagnostics(gro.h, gpol.h, 0.2, None, out))
    cnn = sg.Policy((1, 84, 84), dr.Discrete(4), base_kwargs={"hidden_size": 32})
    with pytest.raises(err, match="sg_rollout_policy_diagnostics: the policy has the CNN base"):
        _lib.check(lib.sg_rollout_policy_diagnostics(ro.h, cnn.h, 0.2, None, out))
    # none of the refused calls left anything behind
    with pytest.raises(err, match="no diagnostics are pending"):
        _lib.check(lib.sg_rollout_policy_diagnostics_fetch(ro.h, out))
