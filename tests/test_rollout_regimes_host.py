"""CPU: the cases of tests/rollout_regimes.py judged on the references alone (oracle/oracle64.py, oracle/oracle.py and numpy
float64 restatements checked against them), the FLOOR constants tests/test_gpu_rollout_regimes.py holds the HIP path to, and the
reason that file exists, restated as tests: a relabel without the +-10 clip or with one side of it, and a compute_returns that
ignores bad_masks[T], reproduce every recorded fixture the older tests compare with and fail the new cases; so does an advantage
normalisation whose mean is accumulated in float32, on the recorded advantages and on a stand-in for the full-size rollout."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rollout_regimes as rr  # noqa: E402
from helpers import RTOL, assert_close, load  # noqa: E402

RETURNS_IDS = [rr.spec_id(s) for s in rr.returns_specs()]
RELABEL_IDS = [rr.relabel_id(s) for s in rr.relabel_specs()]
ADV_IDS = [f"n{n}-{r}" for n, r in rr.adv_specs()]


# ------------------------------------------------------------------------------------------- float32 distances, shared
@functools.lru_cache(maxsize=None)
def returns_f32(spec):
    """{(use_gae, proper, gamma, lam): the float32 oracle's largest column distance from float64}"""
    c = rr.returns_case(*spec)
    out = {}
    for g, p in rr.MODES:
        for ga, la in rr.GAMMA_LAMBDA:
            r64, r32 = rr.returns_ref(c, g, p, ga, la, 64)[0], rr.returns_ref(c, g, p, ga, la, 32)[0]
            out[(g, p, ga, la)] = float(rr.returns_distances(r32, c, g, r64).max())
    return out


@functools.lru_cache(maxsize=None)
def relabel_f32(spec):
    """the float32 oracle's largest distance over both calls and over rewards (per column), returns and the statistics"""
    r64, r32, _ = rr.relabel_refs(*spec)
    ds = [rr.relabel_distances(r32[k], r64[k]) for k in range(2)]
    return max(max(float(d["rewards"].max()), d["returns"], d["rms"]) for d in ds)


@functools.lru_cache(maxsize=None)
def auto_f32(dones, no_alive_bonus):
    c = rr.auto_case(dones)
    a64, a32 = rr.auto_ref(c, no_alive_bonus, 64)[0], rr.auto_ref(c, no_alive_bonus, 32)[0]
    ds = [rr.relabel_distances(a32[k], a64[k]) for k in range(2)]
    return max(max(float(d["rewards"].max()), d["returns"], d["rms"]) for d in ds)


@functools.lru_cache(maxsize=None)
def adv_f32(spec):
    c = rr.adv_case(*spec)
    return rr.distance(rr.adv_ref(c, 32), rr.adv_ref(c, 64))


# ------------------------------------------------------------------------------------------- the cases' claims
def _count_after(count, merges, n):
    """RunningMeanStd's count after `merges` batches of n, added one batch at a time as the merge does"""
    for _ in range(merges):
        count = count + n
    return count


@pytest.mark.parametrize("spec", rr.returns_specs(), ids=RETURNS_IDS)
def test_returns_case_reaches_what_it_claims(spec):
    T, N, dones = spec
    c = rr.returns_case(*spec)
    d = rr.describe(c)
    print(c.tag, d)
    assert c.rewards.dtype == c.value_preds.dtype == c.masks.dtype == c.bad_masks.dtype == c.next_value.dtype == np.float32
    assert c.rewards.shape == (T, N) and c.value_preds.shape == c.masks.shape == c.bad_masks.shape == (T + 1, N)
    assert d["slot_0_is_nan"]
    assert set(np.unique(c.masks[1:])) <= {0.0, 1.0} and set(np.unique(c.bad_masks[1:])) <= {0.0, 1.0}
    if dones:
        every = list(range(min(rr.CHUNK, T)))
        assert d["masks_positions"] == every and d["bad_positions"] == every
        assert d["slot_T"] == (True, True) and d["step_0"] == (True, True)
        if T * N >= 500:      # the rates mean something only where the placed zeros are few among the slots
            assert 0.05 <= d["masks_zero_frac"] <= 0.15 and 0.15 <= d["bad_zero_frac"] <= 0.27
            assert abs(d["rewards_mean"] - 1.0) < 0.1 and 2.7 < d["value_scale"] < 3.3
    else:
        assert d["masks_zero_frac"] == 0.0 and d["bad_zero_frac"] == 0.0
    for g, p in rr.MODES:
        for ga, la in rr.GAMMA_LAMBDA:
            r64, vp64 = rr.returns_ref(c, g, p, ga, la, 64)
            upto = T if g else T + 1
            assert np.isfinite(r64[:upto]).all() and np.isfinite(vp64[:T]).all(), (c.tag, g, p)       # slot 0's NaN reaches nothing
            rn, vpn = rr.compute_returns_np(c.rewards, c.value_preds, c.masks, c.bad_masks, c.next_value, g, ga, la, p)
            assert np.allclose(rn[:upto], r64[:upto], rtol=1e-12, atol=1e-12), (c.tag, g, p, ga, la)
            assert np.array_equal((vp64 if g else r64)[T], c.next_value.astype(np.float64))
    if not dones and T == 128:
        r64 = rr.returns_ref(c, 0, 0, 1.0, 1.0, 64)[0]
        assert np.abs(r64).max() > 100.0           # the longest chain: 128 undiscounted rewards of mean 1
    f32 = returns_f32(spec)
    print(c.tag, "float32 oracle, largest column distance", max(f32.values()))
    assert max(f32.values()) <= RTOL


@pytest.mark.parametrize("spec", rr.relabel_specs(), ids=RELABEL_IDS)
def test_relabel_case_reaches_what_it_claims(spec):
    (F, Hd, T, N), regime = spec
    c = rr.relabel_case(*spec)
    r64, r32, nps = rr.relabel_refs(*spec)       # (asserts the numpy restatement against the arbiter)
    d = rr.describe(c)
    print(c.tag, d)
    assert d["max_abs_logit"] <= 6.0 and d["max_abs_logit"] >= 4.0     # the plain-contract regime, and not the initialisation's
    for k, x in enumerate(d["calls"]):
        assert x["slot_T_is_nan"] and x["feat_0_is_nan"]
        assert np.isfinite(r64[k][0]).all() and np.isfinite(r64[k][1]).all() and np.isfinite(r64[k][2]).all()
        assert x["positions"] == list(range(min(rr.CHUNK, T)))
        assert x["undecided_frac"] <= 0.01
        assert x["low"] + x["high"] + x["inside"] + round(x["undecided_frac"] * x["n"]) == x["n"] == T * N
        if regime == "fresh":
            assert x["low"] == x["high"] == 0
        elif regime == "both_sides" and spec[0] in rr.RELABEL_SHAPES:
            assert min(x["low"], x["high"], x["inside"]) >= 1, x
        elif regime == "all_clipped":
            assert x["low"] + x["high"] >= 0.9 * x["n"] and min(x["low"], x["high"]) >= 1, x
        # the reference's own clipped elements are exactly +-10
        lo, hi, _ = rr.clip_classes(nps[k]["unclipped"])
        assert (r64[k][0][lo] == -rr.CLIP).all() and (r64[k][0][hi] == rr.CLIP).all()
    if regime == "both_sides":
        assert d["calls"][0]["low"] >= 1 and d["calls"][0]["high"] >= 1 and d["calls"][0]["inside"] >= 1
    assert d["calls"][1]["masks0_zeros"] >= 1 and (N == 1 or d["calls"][1]["masks0_ones"] >= 1)
    assert c.offset[0] > 0 > c.offset[1]
    assert r64[1][2][2] == _count_after(c.rms0[2], 2 * T, N)
    for k in range(2):
        assert not rr.stats_failures(r32[k][2], r64[k][2]), (c.tag, k, "float32 oracle", rr.stats_failures(r32[k][2], r64[k][2]))
    x = relabel_f32(spec)
    print(c.tag, "float32 oracle, largest distance", x)
    assert x <= RTOL


def test_long_relabel_cases_are_the_two_sides_of_64_kib():
    T = rr.LONG_SHAPE[2]
    assert 3 * T * 8 > 64 * 1024 >= 3 * (T - 1) * 8 and rr.LAST_STAGED_SHAPE[2] == T - 1


@pytest.mark.parametrize("dones", [True, False], ids=["dones", "no-dones"])
@pytest.mark.parametrize("no_alive_bonus", [False, True], ids=["alive-bonus", "no-alive-bonus"])
def test_auto_case_reaches_what_it_claims(dones, no_alive_bonus):
    c = rr.auto_case(dones)
    calls, scal = rr.auto_ref(c, no_alive_bonus, 64)
    for k in range(2):
        m = c.masks[k]
        assert np.isfinite(m).all() and set(np.unique(m)) <= {0.0, 1.0}
        n_dones, r_sa = scal[k]
        assert n_dones == float((m == 0).sum()) and (n_dones > 0) == dones
        # a2c/main_gail_dyn_ppo.py:258-271 in closed form
        dd = n_dones + c.N / 2.0
        d_sa = 1.0 - dd / (dd + c.T * c.N / rr.TAR_LENGTH)
        assert r_sa == (0.0 if no_alive_bonus else pytest.approx(np.log(d_sa) - np.log(1.0 - d_sa), rel=1e-12))
        assert no_alive_bonus or abs(r_sa) > 0.1
        assert np.isfinite(calls[k][0]).all()
    assert calls[1][2][2] == _count_after(1e-4, 2 * c.T, c.N)
    assert auto_f32(dones, no_alive_bonus) <= RTOL


@pytest.mark.parametrize("spec", rr.adv_specs(), ids=ADV_IDS)
def test_adv_case_reaches_what_it_claims(spec):
    n, regime = spec
    c = rr.adv_case(*spec)
    d = rr.describe(c)
    print(c.tag, d, "float32 oracle distance", adv_f32(spec))
    assert d["n"] == n == c.T * c.N
    assert d["ratio"] <= rr.ADV_MAX_RATIO
    if regime == "zero_mean":
        assert d["ratio"] < 1e-6
    elif regime == "ratio_3":
        assert 2.9 < d["ratio"] < 3.1
    else:
        assert 990.0 < d["ratio"] <= 1000.0
    assert sorted(rr.ADV_N) == [37, 1025, 65573] and 37 < 1024 < 1025 < 64 * 1024 < 65573     # one block's stride, the whole grid
    assert adv_f32(spec) <= RTOL


# ------------------------------------------------------------------------------------------- FLOOR
def _floor_sources():
    """per family, {label: float32 distance} over the cases FLOOR is taken from: every returns case; the relabel cases from the
    fresh and both_sides statistics (the auto cases included); the advantage cases of ratio 0 and 3.  The all_clipped and
    ratio_1000 cases are ill-conditioned by construction (a reward near 0 divided by a scale of 1e-3; a mean 1000 standard
    deviations from 0) and are held to F x their own float32 distance + FLOOR."""
    out = {"returns": {}, "relabel": {}, "advantages": {}}
    for spec in rr.returns_specs():
        for key, x in returns_f32(spec).items():
            out["returns"][f"{rr.spec_id(spec)} gae {key[0]} proper {key[1]} gamma {key[2]} lambda {key[3]}"] = x
    for spec in rr.relabel_specs():
        if spec[1] != "all_clipped":
            out["relabel"][rr.relabel_id(spec)] = relabel_f32(spec)
    for dn in (True, False):
        for nab in (False, True):
            out["relabel"][f"auto dones {dn} no_alive_bonus {nab}"] = auto_f32(dn, nab)
    for spec in rr.adv_specs():
        if spec[1] != "ratio_1000":
            out["advantages"][f"n {spec[0]} {spec[1]}"] = adv_f32(spec)
    return out


def test_floor_is_the_float32_oracles_largest_distance():
    """tests/test_gpu_rollout_regimes.py's FLOOR, per family: not below the float32 oracle's largest distance from float64 over
    the family's cases, nor more than a quarter above it."""
    import test_gpu_rollout_regimes as tg
    for family, per in _floor_sources().items():
        worst = max(per, key=per.get)
        print(f"FLOOR[{family}]: re-derived {per[worst]:.3e} ({worst}); constant {tg.FLOOR[family]:.3e}")
        assert per[worst] <= tg.FLOOR[family] <= 1.25 * per[worst], (family, worst, per[worst])
    hard = {rr.relabel_id(s): relabel_f32(s) for s in rr.relabel_specs() if s[1] == "all_clipped"}
    hard.update({f"advantages n {s[0]} {s[1]}": adv_f32(s) for s in rr.adv_specs() if s[1] == "ratio_1000"})
    print("held to F x float32 + FLOOR:", hard)
    assert tg.F >= 2.0 and max(hard.values()) <= 0.5 * RTOL     # room for F >= 2 inside the contract


# ------------------------------------------------------------------------------------------- what the older tests cannot see
def _golden_relabel(name, clip):
    """the recorded relabel calls of tests/golden/<name>.npz through the numpy restatement with `clip` -> [(got, want)]"""
    g = load(name)
    m = g["meta"]
    c = rr.Case(F=m["F"], Hd=m["Hd"], T=m["T"], N=m["N"], gamma=m["gamma"], params=g["params"],
                obs_feat=[g["obs_feat0"], g["obs_feat1"]], masks=[g["masks0"][..., 0], g["masks1"][..., 0]],
                offset=[float(g["offset0"]), float(g["offset1"])])
    out, ret, st = [], None, [0.0, 1.0, 1e-4]
    for k in range(2):
        o = rr.relabel_np(c, k, ret, st, clip=clip)
        ret, st = o["returns"], o["rms"]
        out.append((o, g[f"rewards{k}"][..., 0], g[f"d_returns{k}"][:, 0], g[f"rms{k}"]))
    return out


WRONG_CLIPS = {"no clip": (None, None), "clip above only": (None, rr.CLIP)}


@pytest.mark.parametrize("name", list(WRONG_CLIPS))
def test_a_relabel_with_a_wrong_clip_reproduces_the_recorded_calls_and_fails_the_new_cases(name):
    clip = WRONG_CLIPS[name]
    top = 0.0
    for fixture in ("relabel_tiny", "relabel_northstar"):
        for k, (o, rewards, d_ret, rms) in enumerate(_golden_relabel(fixture, clip)):
            assert_close(o["rewards"], rewards, what=f"{name}: {fixture} rewards, call {k}")          # tests/test_oracle_golden.py's comparison
            assert_close(o["returns"], d_ret, what=f"{name}: {fixture} D.returns, call {k}")
            assert_close(o["rms"], rms, rtol=1e-5, what=f"{name}: {fixture} ret_rms, call {k}")
            top = max(top, float(np.abs(rewards).max()))
    print(f"{name}: all four recorded calls reproduced; largest recorded |reward| {top:.2f}")
    assert top < 3.0
    for spec in rr.relabel_specs():
        if spec[1] == "fresh":
            continue
        c = rr.relabel_case(*spec)
        r64, _, _ = rr.relabel_refs(*spec)
        o = rr.relabel_np(c, 0, None, list(c.rms0), clip=clip)
        worst = float(rr.column_distances(o["rewards"], r64[0][0]).max())
        print(f"{name}: {c.tag}: largest column distance {worst:.3g}")
        assert worst > 100 * RTOL, c.tag
    # ... while the right clip holds the new cases (the restatement is checked against the arbiter in rollout_regimes.relabel_refs)


def test_a_compute_returns_blind_to_bad_masks_T_reproduces_the_recorded_rollout_and_fails_the_new_cases():
    g = load("gae")
    T = g["rewards"].shape[0]
    assert (g["bad_masks"][:T] == 0).sum() == 7 and (g["bad_masks"][T] == 1).all()
    for use_gae, proper in rr.MODES:
        ret, vp = rr.compute_returns_np(g["rewards"][..., 0], g["value_preds"][..., 0], g["masks"][..., 0], g["bad_masks"][..., 0],
                                        g["next_value"][:, 0], use_gae, 0.99, 0.95, proper, ignore_bad_T=True)
        upto = T if use_gae else T + 1
        assert_close(ret[:upto], g[f"returns_gae{use_gae}_proper{proper}"][:upto, :, 0], rtol=1e-5, what=f"gae.npz, gae {use_gae} proper {proper}")
        assert_close(vp, g[f"value_preds_gae{use_gae}_proper{proper}"][..., 0], what="value_preds")
    for spec in rr.returns_specs():
        if not spec[2]:
            continue
        c = rr.returns_case(*spec)
        for use_gae in (1, 0):
            for ga, la in rr.GAMMA_LAMBDA:
                r64 = rr.returns_ref(c, use_gae, 1, ga, la, 64)[0]
                ret, _ = rr.compute_returns_np(c.rewards, c.value_preds, c.masks, c.bad_masks, c.next_value, use_gae, ga, la, 1, ignore_bad_T=True)
                worst = float(rr.returns_distances(ret, c, use_gae, r64).max())
                assert worst > 10 * RTOL, (c.tag, use_gae, ga, la, worst)


def advantages_f32_mean(returns, value_preds):
    """the deliberately wrong form: the sum behind the mean accumulated sequentially in float32 (the reference and the kernel
    accumulate in float64 and round the MEAN to float32), the rest as oracle/sg_oracle.c has it"""
    a = (np.asarray(returns, np.float32) - np.asarray(value_preds, np.float32)).reshape(-1)
    mean = np.float32(np.cumsum(a, dtype=np.float32)[-1] / np.float32(a.size))
    dd = a.astype(np.float64) - np.float64(mean)
    std = np.float32(np.sqrt((dd * dd).sum() / (a.size - 1)))
    return (a - mean) / (std + np.float32(1e-5))


def test_an_advantage_mean_accumulated_in_float32_passes_the_existing_data_and_fails_the_new_cases():
    """The recorded advantages (tests/golden/ppo_*.npz) sit at |mean| / std < 1 on at most 128 rows.  The full-size rollout of
    tests/test_gpu_fullsize.py exists on the GPU only; its advantages are 65,536 values of |mean| / std ~ 0, and a numpy draw
    of that description stands in for it here (compared as that test compares: elementwise, rtol 1e-5)."""
    from oracle import oracle as o32
    for name in ("ppo_mlp_tiny", "ppo_mlp_northstar", "ppo_mlp_onestep", "ppo_split_hopper", "ppo_split_laikago"):
        g = load(name)
        assert_close(advantages_f32_mean(g["returns"][:-1], g["value_preds"][:-1]), g["advantages"].reshape(-1), rtol=1e-5, what=name)
    rng = np.random.default_rng(3)
    vp = rng.standard_normal(65536).astype(np.float32)
    ret = (vp + 0.02 + 0.5 * rng.standard_normal(65536)).astype(np.float32)
    assert_close(advantages_f32_mean(ret, vp), o32.advantages(ret, vp), rtol=1e-5, what="full-size stand-in")
    for n in rr.ADV_N:
        c = rr.adv_case(n, "ratio_1000")
        x = rr.distance(advantages_f32_mean(c.returns[:-1], c.value_preds[:-1]), rr.adv_ref(c, 64))
        print(f"{c.tag}: float32-accumulated mean, distance {x:.3g}; float32 oracle {adv_f32((n, 'ratio_1000')):.3g}")
        if n > 1024:
            assert x > RTOL, c.tag
