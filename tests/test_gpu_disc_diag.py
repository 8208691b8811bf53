"""GPU: discriminator diagnostics on the device -- sg_disc_diagnostics / Discriminator.diagnostics and
GailDynLearner.update(disc_diagnostics=True) -- against the float64 reference of tests/disc_diag_ref.py under its rule: a statistic
passes if |hip - f64| <= 1e-4 |f64| + allowance; the two row counts and the two accuracies are exact (disc_diag_ref: THE RULE,
CONDITIONS).

Which code a case reaches (csrc/sg_disc_diag.hip): 32-row tiles, policy | expert | mid, over a grid capped at 2 x CUs.  1, 16 and
17 rows: one live lane, half a tile, a ragged second tile; n_e = 200 > T*N = 77: no wrap of the mid pairing, n_e = 17 < T*N = 130:
it wraps inside a tile and across tiles; (150, 256) does not fit LDS and runs the global-weight instance, SG_DISC_GW=1 forces it on
the others; 129 x 520 with n_e = 1,000 are 4,226 tiles, several trips of every workgroup and more records than the reduce has
lanes.

SG_DDIAG_RECORD=<path> collects, per case, the largest ratio of distance to bound and its statistic (profiles/disc_diag_parity.json)."""
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
import disc_diag_ref as dd  # noqa: E402
import discrete_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    yield simgan_amd
    path = os.environ.get("SG_DDIAG_RECORD")
    if path and WORST:
        doc = {"what": "tests/test_gpu_disc_diag.py under SG_DDIAG_RECORD: per case, the largest |hip - float64| / (1e-4 |float64| + "
                       "allowance) over the nineteen statistics and the statistic it was seen on; row counts and accuracies are exact (0)",
               "cases": WORST, "worst": max(v["ratio"] for v in WORST.values())}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)


def make_disc(sg, c, params=None):
    d = sg.algo.gail.Discriminator(c.F, c.Hd, None, seed=1)
    d.set_flat_params(np.asarray(c.params if params is None else params, np.float32))
    d.set_expert(c.expert)
    return d


def make_rollout(sg, c, resident=True):
    """obs_feat[1:] are the case's policy rows; slot 0, which the launch must not read, holds 1e3"""
    ro = sg.RolloutStorage(c.T, c.N, (3,), dr.Box((1,)), 1, c.F)
    feat = np.concatenate([np.full((1, c.N, c.F), 1e3, np.float32), c.policy.reshape(c.T, c.N, c.F)])
    ro.obs_feat.copy_(ro.obs_feat.new_tensor(feat))
    if resident:
        ro.device_resident = True
        ro.sync_to_device()
    return ro


def judge(label, got, c, params=None):
    want, allow = dd.reference(c, params=params)
    dist = dd.compare(got, want, allow)
    k = max(dd.NAMES, key=lambda n: dist[n] if np.isfinite(dist[n]) else np.inf)
    WORST[label] = {"ratio": float(dist[k]), "statistic": k}
    print(label, f"largest distance / bound {dist[k]:.4f} ({k})", {n: (got[n], want[n], allow[n], round(dist[n], 4)) for n in dd.NAMES})
    bad = {n: (got[n], want[n], allow[n], dist[n]) for n in dd.NAMES if not dist[n] <= 1.0}
    assert not bad, f"{label}: (hip, float64, allowance, distance / bound) {bad}"
    for n in dd.EXACT:
        assert got[n] == want[n], (label, n, got[n], want[n])
    return want


def same(a, b):
    """two result dicts, bit for bit"""
    return tuple(a) == tuple(b) == dd.NAMES and all(np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64) for k in dd.NAMES)


@pytest.mark.parametrize("name", dd.CASES)
def test_against_float64(sg, name):
    c = dd.case(name)
    disc, ro = make_disc(sg, c), make_rollout(sg, c)
    got = disc.diagnostics(ro)
    assert tuple(got) == dd.NAMES
    want = judge(name, got, c)
    assert got["policy_rows"] == c.T * c.N and got["expert_rows"] == c.expert.shape[0]
    if name == "zero_head":     # d == 0 is wrong for both; the gradient is exactly 0
        assert got["policy_accuracy"] == 0.0 and got["expert_accuracy"] == 0.0 and got["grad_norm_max"] == 0.0 and got["mid_grad_pen"] == 10.0
    if c.T * c.N == 1:
        assert got["reward_std"] == 0.0 and got["policy_logit_std"] == 0.0 and got["reward_min"] == got["reward_max"] == got["reward_mean"]
    assert want["reward_min"] <= want["reward_mean"] <= want["reward_max"] and got["reward_min"] <= got["reward_mean"] <= got["reward_max"]


@pytest.mark.parametrize("name", ["both_7x16_10x13_e17", "both_86x100_7x11_e100", "sat_7x16_1x17_e17"])
def test_forced_global_weight_path(sg, name, monkeypatch):
    c = dd.case(name)
    disc, ro = make_disc(sg, c), make_rollout(sg, c)
    lds = disc.diagnostics(ro)
    monkeypatch.setenv("SG_DISC_GW", "1")
    gw = disc.diagnostics(ro)
    monkeypatch.delenv("SG_DISC_GW")
    judge(name + " SG_DISC_GW=1", gw, c)
    assert all(gw[k] == lds[k] for k in dd.EXACT)
    assert same(lds, disc.diagnostics(ro)), "back on the LDS instance"


@pytest.mark.parametrize("name", ["both_7x16_10x13_e17", "both_86x100_7x11_e100", "both_150x256_7x11_e16", "both_7x16_large"])
def test_same_bits_in_every_form(sg, name):
    c = dd.case(name)
    disc, ro = make_disc(sg, c), make_rollout(sg, c)
    first = disc.diagnostics(ro)
    assert same(first, disc.diagnostics(ro)), "twice in a row"
    assert same(first, disc.diagnostics(ro, slot=1)), "slot 1, direct"
    assert disc.diagnostics(ro, fetch=False) is None and disc.diagnostics(ro, fetch=False, slot=1) is None     # two pending at once
    assert same(first, disc.last_diagnostics(1)), "slot 1, queued"
    assert same(first, disc.last_diagnostics(0)), "slot 0, queued and read after slot 1"
    from simgan_amd import _lib
    for slot in (0, 1):
        with pytest.raises(_lib.SimganHipError, match=f"no diagnostics are pending in slot {slot}"):
            disc.last_diagnostics(slot)
    host_ro = make_rollout(sg, c, resident=False)
    assert same(first, make_disc(sg, c).diagnostics(host_ro)), "host rollout, another discriminator object"
    assert same(first, disc.diagnostics(host_ro)), "host rollout, nothing stale to push"


def test_two_slots_hold_two_results(sg):
    """slot 0 queued at one set of weights, slot 1 at another: each fetch returns its own"""
    c = dd.case("both_7x16_10x13_e17")
    disc, ro = make_disc(sg, c), make_rollout(sg, c)
    other = (c.params * np.float32(0.5)).astype(np.float32)
    a = disc.diagnostics(ro)
    disc.set_flat_params(other)
    b = disc.diagnostics(ro)
    assert not same(a, b)
    disc.set_flat_params(c.params)
    disc.diagnostics(ro, fetch=False, slot=0)
    disc.set_flat_params(other)
    disc.diagnostics(ro, fetch=False, slot=1)
    assert same(b, disc.last_diagnostics(1)) and same(a, disc.last_diagnostics(0))


def _state(sg, disc, ro):
    from simgan_amd import _lib
    m, v, step = disc.get_adam()
    out = {"params": disc.get_flat_params().copy(), "m": m, "v": v, "step": np.array([step], np.float64),
           "scalars": np.array(disc.scalars(), np.float64)}
    ret = disc.returns
    out["returns"] = np.zeros(0, np.float32) if ret is None else np.array(ret.numpy() if hasattr(ret, "numpy") else ret, np.float32)
    T, N = ro.num_steps, ro.num_processes
    shapes = {_lib.F_OBS: (T + 1, N, ro.obs_dim), _lib.F_OBS_FEAT: (T + 1, N, ro.feat_len), _lib.F_ACTIONS: (T, N, ro.act_dim),
              _lib.F_REWARDS: (T, N, 1), _lib.F_VALUE_PREDS: (T + 1, N, 1), _lib.F_RETURNS: (T + 1, N, 1), _lib.F_LOGP: (T, N, 1),
              _lib.F_MASKS: (T + 1, N, 1), _lib.F_BAD_MASKS: (T + 1, N, 1), _lib.F_ADVANTAGES: (T, N, 1)}
    for f, shape in shapes.items():
        a = np.zeros(shape, np.float32)
        _lib.check(ro.lib.sg_rollout_download(ro.h, f, _lib.fptr(a), a.size))
        out[f] = a
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("name", ["both_7x16_10x13_e17", "both_150x256_7x11_e16"])
def test_nothing_but_the_result_is_written(sg, name):
    """Parameters, Adam state, Discriminator.returns, the ret_rms scalars and every rollout field are bit-identical before and after;
    the expert matrix has no read-back, so it is held through what reads all of it: an update epoch whose expert permutation
    consumes every expert row gives the same bits with and without the diagnostics calls before it."""
    from simgan_amd.driver import ExpertLoader
    c = dd.case(name)
    n_e, n_p = c.expert.shape[0], c.T * c.N
    B = n_e                                           # one step per epoch consumes the whole matrix
    rng = np.random.default_rng(8)
    draws = dict(expert_perm=rng.permutation(n_e), policy_perm=rng.permutation(n_p), alpha=rng.random(n_e).astype(np.float32))
    runs = []
    for call in (False, True):
        disc, ro = make_disc(sg, c), make_rollout(sg, c)
        loader = ExpertLoader(c.expert, B)
        disc.update_gail_dyn(loader, ro, **draws)     # (Adam state and the step count hold something)
        disc.relabel_rewards_auto(ro, 0.99, 5.0)      # (so do returns and the ret_rms scalars)
        if call:
            before = _state(sg, disc, ro)
            disc.diagnostics(ro)
            disc.diagnostics(ro, fetch=False, slot=1)
            disc.last_diagnostics(1)
            after = _state(sg, disc, ro)
            assert before.keys() == after.keys()
            for k in before:
                assert np.array_equal(_bits(before[k]), _bits(after[k])), k
        losses = disc.update_gail_dyn(loader, ro, **draws)
        runs.append((np.asarray(losses, np.float32), _state(sg, disc, ro)))
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])), "losses of the update that follows"
    for k in runs[0][1]:
        assert np.array_equal(_bits(runs[0][1][k]), _bits(runs[1][1][k])), k


def _policy_and_rollout(sg, c, resident, F):
    p = sg.Policy((c["O"],), dr.Box((c["A"],)), base_kwargs={"recurrent": False, "hidden_size": c["H"]})
    p.set_flat_params(np.asarray(c["params"], np.float32))
    ro = sg.RolloutStorage(c["T"], c["N"], (c["O"],), dr.Box((c["A"],)), 1, F)
    ro.obs_feat.copy_(ro.obs_feat.new_tensor(np.random.default_rng(3).standard_normal(tuple(ro.obs_feat.shape)).astype(np.float32)))
    for name in ("obs", "actions", "action_log_probs", "value_preds", "returns", "masks"):
        t = getattr(ro, name)
        t.copy_(t.new_tensor(np.asarray(c[name]).reshape(tuple(t.shape))))
    if resident:
        ro.device_resident = True
        ro.sync_to_device()
    return p, ro


def _gail_learner(sg, c, resident, F=6, gail_epoch=2):
    from simgan_amd.driver import GailDynLearner
    expert = np.random.default_rng(4).standard_normal((64, F)).astype(np.float32)
    pol, ro = _policy_and_rollout(sg, c, resident, F)
    disc = sg.algo.gail.Discriminator(F, 16, None, seed=2)
    agent = sg.algo.PPO(pol, dg.CLIP, 2, 2, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    disc.seed, agent.seed = 11, 12
    return GailDynLearner(pol, agent, disc, ro, expert, gail_batch_size=16, gail_epoch=gail_epoch, gail_tar_length=5.0)


@pytest.mark.parametrize("resident", [True, False])
def test_gail_dyn_learner_update_with_disc_diagnostics(sg, resident):
    c = dg.case("mlp_130")
    runs = []
    for flag in (False, True):
        learner = _gail_learner(sg, c, resident)
        losses = learner.update(diagnostics=True, disc_diagnostics=flag)
        runs.append(({k: np.float32(losses[k]).view(np.uint32) for k in losses}, learner.actor_critic.get_flat_params(),
                     learner.discr.get_flat_params(), learner))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) == 7, (runs[0][0], runs[1][0])
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1])), "policy parameters"
    assert np.array_equal(_bits(runs[0][2]), _bits(runs[1][2])), "discriminator parameters"
    assert runs[0][3].last_disc_diagnostics is None
    got = runs[1][3].last_disc_diagnostics
    assert got is runs[1][3].last_disc_diagnostics and tuple(got) == ("before", "after")
    assert tuple(got["before"]) == dd.NAMES and tuple(got["after"]) == dd.NAMES
    # last_diagnostics stays what it was
    a, b = runs[0][3].last_diagnostics, runs[1][3].last_diagnostics
    assert tuple(a) == dg.NAMES and all(np.float64(a[k]).view(np.uint64) == np.float64(b[k]).view(np.uint64) for k in dg.NAMES)
    # the direct calls on a twin: before the first epoch, after the last
    twin = _gail_learner(sg, c, resident)
    disc, ro = twin.discr, twin.rollouts
    disc._bind_loader(twin.loader)
    assert same(got["before"], disc.diagnostics(ro)), (got["before"], disc.diagnostics(ro))
    for _ in range(twin.gail_epoch):
        disc.update_gail_dyn(twin.loader, ro, fetch_losses=False)
    assert same(got["after"], disc.diagnostics(ro))
    assert not same(got["before"], got["after"]) and got["before"]["policy_rows"] == 130.0 and got["before"]["expert_rows"] == 64.0
    assert np.array_equal(_bits(disc.get_flat_params()), _bits(runs[1][2]))
    # a second update publishes a new pair
    runs[1][3].update(disc_diagnostics=True)
    again = runs[1][3].last_disc_diagnostics
    assert again is not got and tuple(again["before"]) == dd.NAMES and tuple(again["after"]) == dd.NAMES


def test_refusals(sg):
    from simgan_amd import _lib
    c = dd.case("init_7x16_2x8_e16")
    disc, ro = make_disc(sg, c), make_rollout(sg, c)
    lib, out, err = ro.lib, (C.c_double * 19)(), _lib.SimganHipError
    with pytest.raises(err, match="no diagnostics are pending in slot 0"):
        _lib.check(lib.sg_disc_diagnostics_fetch(disc.h, 0, out))
    _lib.check(lib.sg_disc_diagnostics(disc.h, ro.h, 0, out))       # the synchronous form leaves nothing pending
    with pytest.raises(err, match="no diagnostics are pending in slot 0"):
        _lib.check(lib.sg_disc_diagnostics_fetch(disc.h, 0, out))
    _lib.check(lib.sg_disc_diagnostics(disc.h, ro.h, 1, None))
    with pytest.raises(err, match="no diagnostics are pending in slot 0"):      # slot 1 is pending, slot 0 is not
        _lib.check(lib.sg_disc_diagnostics_fetch(disc.h, 0, out))
    _lib.check(lib.sg_disc_diagnostics_fetch(disc.h, 1, out))
    with pytest.raises(err, match="sg_disc_diagnostics: NULL argument"):
        _lib.check(lib.sg_disc_diagnostics(None, ro.h, 0, out))
    with pytest.raises(err, match="sg_disc_diagnostics: NULL argument"):
        _lib.check(lib.sg_disc_diagnostics(disc.h, None, 0, out))
    with pytest.raises(err, match="sg_disc_diagnostics_fetch: NULL argument"):
        _lib.check(lib.sg_disc_diagnostics_fetch(disc.h, 0, None))
    for slot in (-1, 2):
        with pytest.raises(err, match=f"sg_disc_diagnostics: slot {slot} is out of range"):
            _lib.check(lib.sg_disc_diagnostics(disc.h, ro.h, slot, out))
        with pytest.raises(err, match=f"sg_disc_diagnostics_fetch: slot {slot} is out of range"):
            _lib.check(lib.sg_disc_diagnostics_fetch(disc.h, slot, out))
    wide = sg.RolloutStorage(2, 8, (3,), dr.Box((1,)), 1, c.F + 1)
    with pytest.raises(err, match=r"sg_disc_diagnostics: rollout feat_len 8 != discriminator input_dim 7"):
        disc.diagnostics(wide)
    bare = sg.algo.gail.Discriminator(c.F, c.Hd, None)
    with pytest.raises(err, match="sg_disc_diagnostics: no expert data"):
        bare.diagnostics(ro)
    ctx2 = _lib.Context(device=0)
    far = sg.algo.gail.Discriminator(c.F, c.Hd, None, ctx=ctx2)
    far.set_expert(c.expert)
    with pytest.raises(err, match="the discriminator and the rollout live on different contexts"):
        _lib.check(lib.sg_disc_diagnostics(far.h, ro.h, 0, out))
    # none of the refused calls left anything behind
    for slot in (0, 1):
        with pytest.raises(err, match="no diagnostics are pending"):
            _lib.check(lib.sg_disc_diagnostics_fetch(disc.h, slot, out))
