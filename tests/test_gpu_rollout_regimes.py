"""GPU: the kernels that turn a finished rollout into a learner's inputs, against float64, off the regime of the recorded
fixtures: k_compute_returns (RolloutStorage.compute_returns and sg_rollout_compute_returns_policy, GAE and plain returns, with
and without proper time limits), the relabel chain k_returns_scan / k_batch_stats / k_rms_scan / k_normalize_rewards
(Discriminator.relabel_rewards, and relabel_rewards_auto with the device alive bonus), and k_adv_stats (device_advantages()
after an update's advantage pass).  The cases are tests/rollout_regimes.py's, each proven on the references alone
(tests/test_rollout_regimes_host.py) to reach what it claims: a zero of masks and of bad_masks at every position of the 8-step
chunks, in slot T and at step 0; T below a chunk, one past a chunk, T = 1; N = 1, one past a 64-lane block, past the 256-thread
stride; gamma = 1 and lambda = 0; rewards clipped at -10 and at +10 with unclipped ones between; T = 2730 and 2731, the last
rollout length at which k_rms_scan stages its statistics in 64 KiB of LDS and the first at which it reads them from global memory;
advantages whose mean is 1000 standard deviations from 0, on 37, 1025 and 65,573 rows.

Distance = ||got - float64||_2 / (||float64||_2 + ATOL max|float64| sqrt(n)): per environment column of returns and of the
relabelled rewards (max over the field), over the whole array for Discriminator.returns, the statistics triple and the advantages.
Both must hold, per column or array:
  * the project's contract: distance <= helpers.RTOL = 1e-4;
  * the arbiter form: distance <= F x (the float32 oracle's distance on the same column or array) + FLOOR.
  FLOOR, per family, is the float32 oracle's own largest distance (tests/test_rollout_regimes_host.py re-derives it):
    returns     6.3e-7   (6.22e-7: T 128 N 4 without dones, plain returns with proper time limits at gamma 0.99 -- the longest chain);
    relabel     3.3e-6   (3.27e-6: 25 x 100, T 3, N 65 from the fresh statistics, second call, a column of three rewards);
    advantages  1.1e-7   (1.02e-7: n 37 at |mean| / std = 3).
  The relabel cases whose statistics clip nearly everything and the advantages at |mean| / std ~ 1000 are ill-conditioned by
  construction (a reward near 0 over a scale of 1e-3; the float32 rounding of a mean of 100 against a deviation of 0.1): the
  float32 oracle is up to 1.5e-5 and 2.3e-5 from float64 there, so they stay out of FLOOR and are held to F x their own float32
  distance + FLOOR.
  F = 2.0: twice the worst max(0, HIP - FLOOR) / float32 ratio measured on the MI355X is 1.99, so the lower limit 2 holds.  The
  worst ratio, 0.995, is advantages n 37 at |mean| / std ~ 1000: HIP 2.291e-5, float32 oracle 2.291e-5 -- k_adv_stats rounds the
  mean to float32 as the reference does, and that rounding is the whole distance; its results equal the float32 oracle's in all
  nine advantage cases, as k_compute_returns' do in all sixteen returns cases (ratio 0: largest HIP distance 6.22e-7, the case
  behind FLOOR).  Relabel: worst ratio 0.15 (7 x 16, T 17, N 257, nearly all clipped: HIP 3.56e-6, float32 oracle 3.58e-6); every
  other relabel case, T = 2730 and 2731 included, sits inside FLOOR (largest 2.77e-6, 25 x 100 with both clip sides reached).
  profiles/rollout_regimes_parity.json holds every case's figures.
Exact, with no tolerance: value_preds[T] == next_value (GAE) and returns[T] == next_value (plain returns) through both entry
points, next_value being get_value(obs[T]); value predictions otherwise untouched; clipped rewards are exactly +-10.0 at exactly
the elements the float64 reference clips (elements whose unclipped float64 value is within 1e-4 relative of +-10 decide nothing:
at most 1 % of a case); the statistics' count (their mean and variance are also held one by one, which the triple's distance
cannot do next to a count of 1e6: rollout_regimes.stats_failures); the done count of scalars(); r_sa == 0 without the alive bonus.
masks[0] and bad_masks[0] (compute_returns), masks[T] and obs_feat[0] (relabel) are NaN: no output may be.
SG_ROLLOUT_REGIMES_RECORD=<path> writes every case's HIP and float32 distances to that file."""
import json
import os

import numpy as np
import pytest

import rollout_regimes as rr
from helpers import RTOL
from test_gpu_world import Box

pytestmark = pytest.mark.gpu

F = 2.0
FLOOR = {"returns": 6.3e-7, "relabel": 3.3e-6, "advantages": 1.1e-7}


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def npv(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def put(t, a):
    t.copy_(t.new_tensor(np.asarray(a, np.float32).reshape(tuple(t.shape))))


def _record(family, label, rec):
    path = os.environ.get("SG_ROLLOUT_REGIMES_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_rollout_regimes.py under SG_ROLLOUT_REGIMES_RECORD.  Per case: the largest distance of the HIP result and "
                       "of the float32 oracle's from the float64 reference (per environment column for returns and relabelled rewards, whole "
                       "array otherwise), ratio = the largest max(0, hip - FLOOR) / float32 over the case's columns or arrays.",
               "F": F, "FLOOR": FLOOR, "returns": {}, "relabel": {}, "advantages": {}}
    doc[family][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


class Tally:
    """collects (hip, float32) distance pairs of one case, holds each to both bounds, and records the case"""

    def __init__(self, family, label):
        self.family, self.label, self.floor = family, label, FLOOR[family]
        self.hip, self.f32, self.ratio, self.fails = 0.0, 0.0, 0.0, []

    def add(self, what, hip, f32):
        hip, f32 = np.atleast_1d(np.asarray(hip, np.float64)), np.atleast_1d(np.asarray(f32, np.float64))
        assert hip.shape == f32.shape and np.isfinite(hip).all(), (self.label, what)
        over = np.maximum(0.0, hip - self.floor)
        ratio = np.where(f32 > 0, over / np.where(f32 > 0, f32, 1.0), np.where(over > 0, np.inf, 0.0))
        self.hip, self.f32, self.ratio = max(self.hip, float(hip.max())), max(self.f32, float(f32.max())), max(self.ratio, float(ratio.max()))
        bad = ~((hip <= RTOL) & (hip <= F * f32 + self.floor))
        if bad.any():
            i = int(np.argmax(np.where(bad, hip, -1.0)))
            self.fails.append(f"{what}: {int(bad.sum())} of {bad.size} outside; worst [{i}]: HIP {hip[i]:.3e} from float64 (contract {RTOL:g}; "
                              f"float32 oracle {f32[i]:.3e}, limit {F * f32[i] + self.floor:.3e})")

    def close(self):
        print(f"{self.label}: largest HIP distance {self.hip:.3e}, float32 oracle {self.f32:.3e}, worst ratio {self.ratio:.2f}")
        _record(self.family, self.label, {"hip_vs_f64": self.hip, "float32_vs_f64": self.f32, "worst_ratio": self.ratio})
        assert not self.fails, (self.label, self.fails)


# ------------------------------------------------------------------------------------------- compute_returns
RETURNS_IDS = [rr.spec_id(s) for s in rr.returns_specs()]
SENTINEL = 777.0        # fills returns before every call: a slot the kernel should have written and did not shows


def _fill_returns_rollout(ro, c):
    put(ro.rewards, c.rewards)
    put(ro.masks, c.masks)
    put(ro.bad_masks, c.bad_masks)


def _check_returns(c, tally, key, got_ret, got_vp, nv, use_gae, proper, gamma, lam):
    T = c.T
    r64 = rr.returns_ref(c, use_gae, proper, gamma, lam, 64, next_value=nv)[0]
    r32 = rr.returns_ref(c, use_gae, proper, gamma, lam, 32, next_value=nv)[0]
    upto = T if use_gae else T + 1
    assert np.isfinite(got_ret[:upto]).all(), (c.tag, key, "NaN or Inf in returns: masks[0] / bad_masks[0] were read")
    assert np.array_equal(got_vp[:T], c.value_preds[:T]), (c.tag, key, "value_preds[:T] changed")
    if use_gae:
        assert np.array_equal(got_vp[T], nv), (c.tag, key, "value_preds[T] != next_value")
    else:
        assert np.array_equal(got_ret[T], nv), (c.tag, key, "returns[T] != next_value")
        assert np.array_equal(got_vp[T], c.value_preds[T]), (c.tag, key, "value_preds[T] changed by the plain-returns branch")
    tally.add(key, rr.returns_distances(got_ret, c, use_gae, r64), rr.returns_distances(r32, c, use_gae, r64))


@pytest.mark.parametrize("spec", rr.returns_specs(), ids=RETURNS_IDS)
def test_compute_returns(sg, spec):
    """RolloutStorage.compute_returns: use_gae x proper x (gamma, lambda) on one rollout, returns refilled before every call"""
    c = rr.returns_case(*spec)
    ro = sg.RolloutStorage(c.T, c.N, (3,), Box((2,)), 1, 0)
    _fill_returns_rollout(ro, c)
    tally = Tally("returns", f"compute_returns {rr.spec_id(spec)}")
    for use_gae, proper in rr.MODES:
        for gamma, lam in rr.GAMMA_LAMBDA:
            put(ro.value_preds, c.value_preds)
            ro.returns.fill_(SENTINEL)
            ro.compute_returns(c.next_value, bool(use_gae), gamma, lam, bool(proper))
            _check_returns(c, tally, f"gae {use_gae} proper {proper} gamma {gamma} lambda {lam}", npv(ro.returns)[..., 0], npv(ro.value_preds)[..., 0],
                           c.next_value, use_gae, proper, gamma, lam)
    tally.close()


@pytest.mark.parametrize("spec", rr.returns_specs(), ids=RETURNS_IDS)
def test_compute_returns_policy(sg, spec):
    """sg_rollout_compute_returns_policy: next_value = get_value(obs[T]) computed on the device and parked in returns[T], which the
    plain-returns branch then reads and writes itself"""
    from simgan_amd import _lib
    c = rr.returns_case(*spec)
    rng = np.random.default_rng([c.T, c.N, 13])
    pol = sg.Policy((3,), Box((2,)), base_kwargs={"recurrent": False, "hidden_size": 64}, seed=5)
    ro = sg.RolloutStorage(c.T, c.N, (3,), Box((2,)), 1, 0)
    _fill_returns_rollout(ro, c)
    put(ro.obs, rng.standard_normal((c.T + 1, c.N, 3)))
    nv = npv(pol.get_value(npv(ro.obs)[c.T], None, None))[:, 0].copy()
    assert nv.shape == (c.N,) and np.isfinite(nv).all() and np.abs(nv).max() > 0
    ro.sync_to_device()
    tally = Tally("returns", f"compute_returns_policy {rr.spec_id(spec)}")
    for use_gae, proper in rr.MODES:
        for gamma, lam in rr.GAMMA_LAMBDA:
            put(ro.value_preds, c.value_preds)
            ro.returns.fill_(SENTINEL)
            ro.sync_to_device([_lib.F_VALUE_PREDS, _lib.F_RETURNS])
            _lib.check(ro.lib.sg_rollout_compute_returns_policy(ro.h, pol.h, use_gae, gamma, lam, proper))
            ro.sync_from_device([_lib.F_RETURNS, _lib.F_VALUE_PREDS])
            _check_returns(c, tally, f"gae {use_gae} proper {proper} gamma {gamma} lambda {lam}", npv(ro.returns)[..., 0], npv(ro.value_preds)[..., 0],
                           nv, use_gae, proper, gamma, lam)
    tally.close()


# ------------------------------------------------------------------------------------------- relabel
RELABEL_IDS = [rr.relabel_id(s) for s in rr.relabel_specs()]


def _make_disc(sg, c):
    D = sg.algo.gail.Discriminator(c.F, c.Hd, None)
    D.set_flat_params(c.params)
    return D


def _relabel_rollout(sg, c, k, resident=False):
    ro = sg.RolloutStorage(c.T, c.N, (3,), Box((2,)), 1, c.F)
    put(ro.obs_feat, c.obs_feat[k])
    put(ro.masks, c.masks[k])
    if resident:
        ro.device_resident = True
        ro.sync_to_device()
    return ro


def _check_clip(c, k, got, unclipped64):
    """exactly +-10.0 at exactly the elements the float64 reference clips, among the decided ones"""
    lo, hi, decided = rr.clip_classes(unclipped64)
    assert (~decided).mean() <= 0.01, (c.tag, k)
    assert np.array_equal(got[lo], np.full(int(lo.sum()), -rr.CLIP)), (c.tag, k, f"{int((got[lo] != -rr.CLIP).sum())} of {int(lo.sum())} low elements are not -10.0")
    assert np.array_equal(got[hi], np.full(int(hi.sum()), rr.CLIP)), (c.tag, k, f"{int((got[hi] != rr.CLIP).sum())} of {int(hi.sum())} high elements are not 10.0")
    inside = decided & ~lo & ~hi
    assert (np.abs(got[inside]) < rr.CLIP).all(), (c.tag, k, f"{int((np.abs(got[inside]) >= rr.CLIP).sum())} elements clipped that the reference does not clip")
    assert np.abs(got).max() <= rr.CLIP
    return int(lo.sum()), int(hi.sum()), int(inside.sum())


def _check_relabel_call(c, k, tally, got, r64, r32, unclipped64):
    rewards, returns, rms = got
    assert np.isfinite(rewards).all() and np.isfinite(returns).all() and np.isfinite(rms).all(), (c.tag, k, "NaN or Inf: masks[T] / obs_feat[0] were read")
    assert rms[2] == r64[2][2], (c.tag, k, "count", rms[2], r64[2][2])
    assert not rr.stats_failures(rms, r64[2]), (c.tag, k, rr.stats_failures(rms, r64[2]))
    classes = _check_clip(c, k, rewards, unclipped64)
    d_hip, d_f32 = rr.relabel_distances(got, r64), rr.relabel_distances(r32, r64)
    for field in ("rewards", "returns", "rms"):
        tally.add(f"call {k} {field}", d_hip[field], d_f32[field])
    return classes


@pytest.mark.parametrize("spec", rr.relabel_specs(), ids=RELABEL_IDS)
def test_relabel_rewards(sg, spec):
    """Discriminator.relabel_rewards, two consecutive calls: Discriminator.returns and the running statistics carried over"""
    c = rr.relabel_case(*spec)
    r64, r32, nps = rr.relabel_refs(*spec)
    D = _make_disc(sg, c)
    assert D.returns is None
    rms = sg.RunningMeanStd(shape=())
    rms.set_state(list(c.rms0))
    tally = Tally("relabel", f"relabel_rewards {rr.relabel_id(spec)}")
    for k in range(2):
        ro = _relabel_rollout(sg, c, k)
        D.relabel_rewards(ro, c.gamma, c.offset[k], rms)
        got = (npv(ro.rewards)[..., 0].astype(np.float64), npv(D.returns)[:, 0].astype(np.float64), np.asarray(rms.get_state(), np.float64))
        classes = _check_relabel_call(c, k, tally, got, r64[k], r32[k], nps[k]["unclipped"])
        print(f"{c.tag} call {k}: clipped low / high / unclipped {classes}")
    tally.close()


@pytest.mark.parametrize("dones", [True, False], ids=["dones", "no-dones"])
@pytest.mark.parametrize("no_alive_bonus", [False, True], ids=["alive-bonus", "no-alive-bonus"])
def test_relabel_rewards_auto(sg, dones, no_alive_bonus):
    """relabel_rewards_auto on a device-resident rollout: the offset is minus the alive bonus of the device's own done count;
    scalars() holds {mean, var, count}, the done count and r_sa"""
    from simgan_amd import _lib
    c = rr.auto_case(dones)
    (r64, scal), (r32, _) = rr.auto_ref(c, no_alive_bonus, 64), rr.auto_ref(c, no_alive_bonus, 32)
    D = _make_disc(sg, c)
    D.set_rms(list(c.rms0))
    tally = Tally("relabel", f"relabel_rewards_auto dones {dones} no_alive_bonus {no_alive_bonus}")
    ret, st = None, list(c.rms0)
    for k in range(2):
        ro = _relabel_rollout(sg, c, k, resident=True)
        D.relabel_rewards_auto(ro, c.gamma, rr.TAR_LENGTH, no_alive_bonus=no_alive_bonus)
        ro.sync_from_device([_lib.F_REWARDS])
        sc = D.scalars()
        assert sc[3] == scal[k][0] == float((c.masks[k] == 0).sum()), (c.tag, k, "done count", sc[3], scal[k][0])
        if no_alive_bonus:
            assert sc[4] == 0.0
        else:
            assert abs(sc[4] - scal[k][1]) <= 1e-12 * abs(scal[k][1]), (c.tag, k, "r_sa", sc[4], scal[k][1])
        o = rr.relabel_np(rr.Case(c, offset=[-scal[0][1], -scal[1][1]]), k, ret, st)
        ret, st = o["returns"], o["rms"]
        got = (npv(ro.rewards)[..., 0].astype(np.float64), npv(D.returns)[:, 0].astype(np.float64), np.asarray(sc[:3], np.float64))
        _check_relabel_call(c, k, tally, got, r64[k], r32[k], o["unclipped"])
    tally.close()


# ------------------------------------------------------------------------------------------- advantages
ADV_IDS = [f"n{n}-{r}" for n, r in rr.adv_specs()]


@pytest.mark.parametrize("spec", rr.adv_specs(), ids=ADV_IDS)
def test_advantages(sg, spec):
    """device_advantages() after one PPO update's advantage pass (k_adv_stats x 3) on T N = n rows"""
    n, regime = spec
    c = rr.adv_case(*spec)
    rng = np.random.default_rng([n, 53])
    pol = sg.Policy((4,), Box((2,)), base_kwargs={"recurrent": False, "hidden_size": 64}, seed=9)
    ro = sg.RolloutStorage(c.T, c.N, (4,), Box((2,)), 1, 0)
    obs = rng.standard_normal((c.T + 1, c.N, 4)).astype(np.float32)
    act = rng.standard_normal((c.T, c.N, 2)).astype(np.float32)
    _, logp, _, _ = pol.evaluate_actions(obs[:-1].reshape(n, 4), None, None, act.reshape(n, 2))
    put(ro.obs, obs)
    put(ro.actions, act)
    put(ro.action_log_probs, npv(logp))
    put(ro.value_preds, c.value_preds)
    put(ro.returns, c.returns)
    agent = sg.algo.PPO(pol, 0.2, 1, 16 if n > 4096 else 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    losses = agent.update(ro)
    adv = npv(ro.device_advantages()).reshape(-1).astype(np.float64)
    assert adv.shape == (n,) and np.isfinite(adv).all() and np.isfinite(losses).all()
    a64, a32 = rr.adv_ref(c, 64), rr.adv_ref(c, 32)
    tally = Tally("advantages", f"advantages n {n} {regime}")
    tally.add("advantages", rr.distance(adv, a64), rr.distance(a32, a64))
    tally.close()
