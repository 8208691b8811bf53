"""Case builders for the kernels that turn a finished rollout into a learner's inputs (tests/test_rollout_regimes_host.py on
the CPU, tests/test_gpu_rollout_regimes.py on the GPU): k_compute_returns, the relabel chain (k_returns_scan, k_batch_stats,
k_rms_scan, k_normalize_rewards, the device alive bonus) and k_adv_stats.  The rest of the suite runs them on two small recorded
rollouts and on the full-size synthetic one, where the reward clip at +-10 is never reached (largest recorded |reward| 2.40),
bad_masks[T] is never 0, gamma and lambda never leave (0.99, 0.95), and T, N never sit on the edges of the 8-step chunks, the
64-lane blocks or the 256-thread stride.  Here:

  returns     (T, N) in RETURNS_SHAPES x use_gae x proper x (gamma, lambda) in GAMMA_LAMBDA, masks and bad_masks with a zero at every
              position of an 8-step chunk, in slot T and at step 0; (1, 1) and (128, 4) once more without any done;
  relabel     (F, Hd, T, N) in RELABEL_SHAPES x three starting running statistics -- fresh, both clip sides reached, nearly all
              clipped -- two consecutive calls each; (7, 16, 2730, 2) and (7, 16, 2731, 2), the two sides of the rollout length at which
              k_rms_scan's 3 T doubles pass 64 KiB of LDS; one case
              through relabel_rewards_auto (alive bonus on and off, with and without dones);
  advantages  n = T N in ADV_N x |mean| / std of the advantages in {0, 3, ~1000}.

Nothing here touches the library.  Inputs are numpy draws at fixed seeds; references are oracle/oracle64.py (compute_returns,
relabel, advantages, alive_bonus), the float32 yardstick is oracle/oracle.py on the same inputs, and the numpy float64
restatements below (which tests/test_rollout_regimes_host.py mutates to show what the older tests cannot see) are checked
against oracle64.  describe_*() returns the facts a case claims, computed on the references alone."""
import functools

import numpy as np

import disc_regimes as dr
from helpers import ATOL, RTOL

Case = dr.Case


# ------------------------------------------------------------------------------------------- distance
def distance(got, ref, scale=None):
    """||got - ref||_2 / (||ref||_2 + ATOL scale sqrt(n)), scale = max|ref| unless given"""
    g, r = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    scale = float(np.max(np.abs(r))) if scale is None else scale
    return float(np.sqrt(((g - r) ** 2).sum()) / (np.sqrt((r ** 2).sum()) + ATOL * scale * np.sqrt(r.size) + 1e-300))


def column_distances(got, ref):
    """per environment column of a [rows, N] field, the floor on the scale of the field's largest element -> [N]"""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert g.shape == r.shape and r.ndim == 2, (g.shape, r.shape)
    scale = float(np.max(np.abs(r)))
    return np.array([distance(g[:, n], r[:, n], scale) for n in range(r.shape[1])])


# ------------------------------------------------------------------------------------------- returns
RETURNS_SHAPES = [(1, 1), (7, 3), (8, 64), (9, 65), (17, 130), (128, 4)]
NO_DONES_SHAPES = [(1, 1), (128, 4)]     # (128, 4): the longest dependent chain; (1, 1): the only way next_value reaches a one-step rollout
GAMMA_LAMBDA = [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)]
MODES = [(g, p) for g in (1, 0) for p in (1, 0)]     # (use_gae, proper)
CHUNK = 8


def returns_specs():
    return [(T, N, True) for T, N in RETURNS_SHAPES] + [(T, N, False) for T, N in NO_DONES_SHAPES]


def spec_id(spec):
    return f"T{spec[0]}-N{spec[1]}" + ("" if spec[2] else "-no-dones")


@functools.lru_cache(maxsize=None)
def returns_case(T, N, dones=True):
    """rewards 1 + N(0,1), value predictions and next_value 3 N(0,1); masks ~10 % and bad_masks ~20 % zeros in slots 1 .. T, and
    placed zeros: for every chunk position u < min(8, T) step T - 1 - u (slot T - u) has a masks zero in column u % N and a
    bad_masks zero in column (u + 1) % N -- u = 0 is slot T -- and step 0 (slot 1) has one of each.  Slot 0 of both is NaN: no
    branch of compute_returns reads it."""
    rng = np.random.default_rng([T, N, 11])
    c = Case(T=T, N=N, dones=dones, tag=f"returns T {T} N {N}" + ("" if dones else " no dones"))
    c["rewards"] = (1.0 + rng.standard_normal((T, N))).astype(np.float32)
    c["value_preds"] = (3.0 * rng.standard_normal((T + 1, N))).astype(np.float32)
    c["next_value"] = (3.0 * rng.standard_normal(N)).astype(np.float32)
    masks, bad = np.ones((T + 1, N), np.float32), np.ones((T + 1, N), np.float32)
    if dones:
        masks[1:][rng.random((T, N)) < 0.1] = 0.0
        bad[1:][rng.random((T, N)) < 0.2] = 0.0
        for u in range(min(CHUNK, T)):
            masks[T - u, u % N] = 0.0
            bad[T - u, (u + 1) % N] = 0.0
        masks[1, 0] = 0.0
        bad[1, 1 % N] = 0.0
    masks[0], bad[0] = np.nan, np.nan
    c["masks"], c["bad_masks"] = masks, bad
    return c


def returns_ref(c, use_gae, proper, gamma, lam, bits=64, next_value=None):
    """-> (returns [T + 1, N], value_preds [T + 1, N]) as float64 arrays, from the arbiter (bits = 64) or the float32 oracle"""
    if bits == 64:
        from oracle import oracle64 as orc
    else:
        from oracle import oracle as orc
    nv = c.next_value if next_value is None else next_value
    ret, vp = orc.compute_returns(c.rewards, c.value_preds, c.masks, c.bad_masks, nv, use_gae, gamma, lam, proper)
    return np.asarray(ret, np.float64), np.asarray(vp, np.float64)


def compute_returns_np(rewards, value_preds, masks, bad_masks, next_value, use_gae, gamma, lam, proper, ignore_bad_T=False):
    """numpy float64 restatement of RolloutStorage.compute_returns (all four branches) -> (returns, value_preds).
    ignore_bad_T: the deliberately wrong form that takes bad_masks[T] for 1."""
    rw, vp = np.asarray(rewards, np.float64), np.array(value_preds, np.float64)
    mk, bm = np.asarray(masks, np.float64), np.array(bad_masks, np.float64)
    T = rw.shape[0]
    if ignore_bad_T:
        bm[T] = 1.0
    ret = np.zeros_like(vp)
    if use_gae:
        vp[T] = next_value
        gae = np.zeros(rw.shape[1])
        for t in range(T - 1, -1, -1):
            delta = rw[t] + gamma * vp[t + 1] * mk[t + 1] - vp[t]
            gae = delta + gamma * lam * mk[t + 1] * gae
            if proper:
                gae = gae * bm[t + 1]
            ret[t] = gae + vp[t]
    else:
        ret[T] = next_value
        for t in range(T - 1, -1, -1):
            if proper:
                ret[t] = (ret[t + 1] * gamma * mk[t + 1] + rw[t]) * bm[t + 1] + (1.0 - bm[t + 1]) * vp[t]
            else:
                ret[t] = ret[t + 1] * gamma * mk[t + 1] + rw[t]
    return ret, vp


def chunk_positions(zero_slots, T):
    """positions within k_compute_returns' 8-step chunks (counted back from step T - 1) that hold a zero: slot j gates step j - 1"""
    steps = np.nonzero((zero_slots[1:] == 0).any(axis=1))[0]
    return sorted({int((T - 1 - t) % CHUNK) for t in steps})


def describe_returns(c):
    T = c.T
    m, b = c.masks, c.bad_masks
    return dict(masks_zero_frac=float((m[1:] == 0).mean()), bad_zero_frac=float((b[1:] == 0).mean()),
                masks_positions=chunk_positions(m, T), bad_positions=chunk_positions(b, T),
                slot_T=(bool((m[T] == 0).any()), bool((b[T] == 0).any())), step_0=(bool((m[1] == 0).any()), bool((b[1] == 0).any())),
                slot_0_is_nan=bool(np.isnan(m[0]).all() and np.isnan(b[0]).all()),
                rewards_mean=float(c.rewards.mean()), value_scale=float(c.value_preds.std()) if c.value_preds.size > 2 else float("nan"))


def returns_distances(got_returns, c, use_gae, ref_returns):
    """column distances over the slots the branch defines: [:T] with GAE (it never writes returns[T]), [:T + 1] without"""
    upto = c.T if use_gae else c.T + 1
    return column_distances(np.asarray(got_returns, np.float64)[:upto], ref_returns[:upto])


# ------------------------------------------------------------------------------------------- relabel
RELABEL_SHAPES = [(7, 16, 9, 5), (7, 16, 17, 257), (25, 100, 3, 65)]
LONG_SHAPE = (7, 16, 2731, 2)          # 3 T doubles = 65,544 bytes: the first T past 64 KiB of LDS in k_rms_scan
LAST_STAGED_SHAPE = (7, 16, 2730, 2)   # 65,520 bytes: the largest T whose statistics k_rms_scan still stages in LDS
RMS_REGIMES = {"fresh": (0.0, 1.0, 1e-4), "both_sides": (0.3, 0.01, 1e6), "all_clipped": (5.0, 1e-6, 1e9)}
RELABEL_GAMMA = 0.99
CLIP = 10.0
NEAR_CLIP = 1e-4                       # elements whose unclipped float64 value is this close (relative) to +-10 decide nothing
RELABEL_SCALES = {(7, 16): (5.0, 2.0), (25, 100): (4.0, 1.5)}     # (scale_w, scale_x): every logit within +-6
AUTO_SHAPE = (7, 16, 9, 65)
TAR_LENGTH = 25.0


def relabel_specs():
    return [(s, r) for s in RELABEL_SHAPES + [LAST_STAGED_SHAPE, LONG_SHAPE] for r in RMS_REGIMES]


def relabel_id(spec):
    (F, Hd, T, N), regime = spec
    return f"{F}x{Hd}-T{T}-N{N}-{regime}"


@functools.lru_cache(maxsize=None)
def relabel_case(shape, regime, dones=True):
    """two consecutive relabel calls: obs_feat scale_x N(0,1) with slot 0 NaN (the relabel reads obs_feat[1:]), masks with ~10 %
    zeros in slots 0 .. T - 1, a zero at every position of k_returns_scan's 8-step chunks (slot u, column u % N), masks[0] zeros in
    some columns of the second call, and slot T NaN (the relabel reads masks[:T]); offsets of both signs."""
    F, Hd, T, N = shape
    rng = np.random.default_rng([F, Hd, T, N, 41])
    sw, sx = RELABEL_SCALES[(F, Hd)]
    c = Case(F=F, Hd=Hd, T=T, N=N, regime=regime, rms0=list(RMS_REGIMES[regime]), gamma=RELABEL_GAMMA, offset=[0.5, -0.5],
             tag=f"relabel {F}x{Hd} T {T} N {N} {regime}" + ("" if dones else " no dones"))
    c["params"] = dr.init_params(rng, F, Hd, sw)
    feats, masks = [], []
    for k in range(2):
        f = (sx * rng.standard_normal((T + 1, N, F))).astype(np.float32)
        f[0] = np.nan
        m = np.ones((T + 1, N), np.float32)
        if dones:
            m[:T][rng.random((T, N)) < 0.1] = 0.0
            for u in range(min(CHUNK, T)):
                m[u, u % N] = 0.0
            if k == 1:
                m[0, ::2] = 0.0
                m[0, 1::2] = 1.0
                m[0, 0] = 0.0
        m[T] = np.nan
        feats.append(f)
        masks.append(m)
    c["obs_feat"], c["masks"] = feats, masks
    return c


def rms_update_np(state, x):
    """RunningMeanStd.update in float64: population mean / variance of the batch, Chan's merge"""
    mean, var, count = state
    n = x.size
    bmean, bvar = x.mean(), x.var()
    delta, tot = bmean - mean, count + n
    M2 = var * count + bvar * n + delta * delta * count * n / tot
    return [mean + delta * n / tot, M2 / tot, tot]


def relabel_np(c, k, d_returns, rms_state, clip=(-CLIP, CLIP), params=None):
    """numpy float64 restatement of one relabel call -> dict(rewards, unclipped, logits, returns, rms).  clip = (lo, hi), either
    None: the deliberately wrong forms without a clip or with one side only."""
    F, Hd, T, N = c.F, c.Hd, c.T, c.N
    logits = dr.logits64(c.params if params is None else params, F, Hd, c.obs_feat[k][1:].reshape(T * N, F)).reshape(T, N)
    raw = dr.reward64(logits)[0] + c.offset[k]
    mk = np.asarray(c.masks[k], np.float64)
    st = list(rms_state)
    unclipped = np.empty((T, N))
    ret = None if d_returns is None else np.asarray(d_returns, np.float64).copy()
    for t in range(T):
        ret = raw[t].copy() if ret is None else ret * c.gamma * mk[t] + raw[t]
        st = rms_update_np(st, ret)
        unclipped[t] = raw[t] / np.sqrt(st[1] + 1e-7)
    rewards = unclipped.copy()
    if clip[0] is not None:
        rewards = np.maximum(rewards, clip[0])
    if clip[1] is not None:
        rewards = np.minimum(rewards, clip[1])
    return dict(rewards=rewards, unclipped=unclipped, logits=logits, returns=ret, rms=st)


def relabel_ref(c, bits=64, offsets=None):
    """both calls through the arbiter (bits = 64) or the float32 oracle, Discriminator.returns and the statistics carried
    -> [(rewards [T, N], returns [N], rms [3])] as float64"""
    if bits == 64:
        from oracle import oracle64 as orc
    else:
        from oracle import oracle as orc
    out, ret, st = [], None, list(c.rms0)
    for k in range(2):
        off = c.offset[k] if offsets is None else offsets[k]
        rew, ret, st = orc.relabel(c.F, c.Hd, c.params, c.obs_feat[k], c.masks[k], c.gamma, off, ret, st)
        out.append((np.asarray(rew, np.float64), np.asarray(ret, np.float64).copy(), [float(x) for x in st]))
    return out


@functools.lru_cache(maxsize=None)
def relabel_refs(shape, regime, dones=True):
    """(float64 reference, float32 oracle, numpy float64 restatement with the unclipped values) of both calls, computed once"""
    c = relabel_case(shape, regime, dones)
    r64, r32 = relabel_ref(c, 64), relabel_ref(c, 32)
    nps, ret, st = [], None, list(c.rms0)
    for k in range(2):
        o = relabel_np(c, k, ret, st)
        ret, st = o["returns"], o["rms"]
        nps.append(o)
        # the restatement against the arbiter: the unclipped values below are those of the reference itself
        assert np.allclose(o["rewards"], r64[k][0], rtol=1e-9, atol=1e-11), (c.tag, k, float(np.abs(o["rewards"] - r64[k][0]).max()))
        assert np.allclose(o["returns"], r64[k][1], rtol=1e-9, atol=1e-11) and np.allclose(o["rms"], r64[k][2], rtol=1e-12, atol=0), (c.tag, k)
    return r64, r32, nps


def clip_classes(unclipped):
    """-> (low, high, decided): elements the float64 reference clips at -10 / at +10, and the mask of the elements that are not
    within NEAR_CLIP (relative) of either limit"""
    u = np.asarray(unclipped, np.float64)
    decided = np.abs(np.abs(u) - CLIP) > NEAR_CLIP * CLIP
    return (u < -CLIP) & decided, (u > CLIP) & decided, decided


def describe_relabel(c, nps):
    T = c.T
    out = dict(max_abs_logit=float(max(np.abs(o["logits"]).max() for o in nps)), calls=[])
    for k, o in enumerate(nps):
        lo, hi, decided = clip_classes(o["unclipped"])
        m = c.masks[k]
        out["calls"].append(dict(low=int(lo.sum()), high=int(hi.sum()), inside=int(((np.abs(o["unclipped"]) < CLIP) & decided).sum()),
                                 undecided_frac=float((~decided).mean()), n=int(decided.size),
                                 masks_zero_frac=float((m[:T] == 0).mean()), masks0_zeros=int((m[0] == 0).sum()), masks0_ones=int((m[0] == 1).sum()),
                                 positions=sorted({int(t % CHUNK) for t in np.nonzero((m[:T] == 0).any(axis=1))[0]}),
                                 slot_T_is_nan=bool(np.isnan(m[T]).all()), feat_0_is_nan=bool(np.isnan(c.obs_feat[k][0]).all())))
    return out


def stats_failures(got, ref):
    """the running mean and variance one by one (in the triple's distance the count, 1e6 or 1e9, hides both):
    |mean - mean64| <= RTOL |mean64| + ATOL sqrt(var64), the mean's error against the spread it describes, and
    |var - var64| <= RTOL var64 -> the list of what fails"""
    out = []
    if not abs(got[0] - ref[0]) <= RTOL * abs(ref[0]) + ATOL * np.sqrt(ref[1]):
        out.append(f"mean {got[0]!r} against {ref[0]!r}")
    if not abs(got[1] - ref[1]) <= RTOL * ref[1]:
        out.append(f"var {got[1]!r} against {ref[1]!r}")
    return out


def relabel_distances(got, ref):
    """one call: (rewards [T, N], returns [N], rms [3]) against the reference's -> dict(rewards: per column [N], returns, rms)"""
    return dict(rewards=column_distances(got[0], ref[0]), returns=distance(got[1], ref[1]), rms=distance(got[2], ref[2]))


# --- relabel_rewards_auto: the offset is -(alive bonus) from the device's own done count over masks[0 .. T]
@functools.lru_cache(maxsize=None)
def auto_case(dones=True):
    """AUTO_SHAPE from the fresh statistics; every mask slot is a number (the done count runs over masks[0 .. T])"""
    base = relabel_case(AUTO_SHAPE, "fresh", dones)
    c = Case(base)
    rng = np.random.default_rng([5, 43])
    c["masks"] = [np.where(np.isnan(m), (rng.random(m.shape) > (0.1 if dones else -1.0)).astype(np.float32), m) for m in base.masks]
    c["tag"] = "auto " + base.tag
    return c


def auto_ref(c, no_alive_bonus, bits=64):
    """-> (calls as relabel_ref, [(dones, r_sa)] per call): float64 alive bonus (as the reference's host code computes it) in both"""
    from oracle import oracle64 as o64
    r_sa, dones = [], []
    for k in range(2):
        dones.append(float((1.0 - c.masks[k].astype(np.float64)).sum()))
        r_sa.append(0.0 if no_alive_bonus else o64.alive_bonus(c.masks[k], c.T, c.N, TAR_LENGTH))
    return relabel_ref(c, bits, offsets=[-x for x in r_sa]), list(zip(dones, r_sa))


# ------------------------------------------------------------------------------------------- advantages
ADV_N = {37: (37, 1), 1025: (25, 41), 65573: (23, 2851)}     # n = T N -> (T, N): below one block's stride, past it, past the 64 x 1024 grid
ADV_REGIMES = {"zero_mean": (0.0, 1.0), "ratio_3": (3.0, 1.0), "ratio_1000": (100.0, 0.1)}     # advantages = shift + sd noise
ADV_MAX_RATIO = 1e3       # beyond it the float32 reference leaves the contract by itself (2.2e-4 at 1e4)


def adv_specs():
    return [(n, r) for n in ADV_N for r in ADV_REGIMES]


@functools.lru_cache(maxsize=None)
def adv_case(n, regime):
    """returns = values + shift + sd noise, the noise standardised (mean 0, std 1.002 over the n draws, so that |mean| / std stays
    below 1000 after the float32 rounding of the returns) -> returns / value_preds [T + 1, N] float32"""
    T, N = ADV_N[n]
    shift, sd = ADV_REGIMES[regime]
    rng = np.random.default_rng([n, 47])
    z = rng.standard_normal(n)
    z = (z - z.mean()) / z.std(ddof=1) * 1.002
    vp = rng.standard_normal((T + 1, N)).astype(np.float32)
    ret = np.zeros((T + 1, N), np.float32)
    ret[:T] = (vp[:T].astype(np.float64) + shift + sd * z.reshape(T, N)).astype(np.float32)
    return Case(n=n, T=T, N=N, regime=regime, returns=ret, value_preds=vp, tag=f"advantages n {n} {regime}")


def adv_ref(c, bits=64):
    if bits == 64:
        from oracle import oracle64 as orc
    else:
        from oracle import oracle as orc
    return np.asarray(orc.advantages(c.returns[:-1], c.value_preds[:-1]), np.float64)


def describe_adv(c):
    a = c.returns[:-1].astype(np.float64) - c.value_preds[:-1].astype(np.float64)
    return dict(n=int(a.size), mean=float(a.mean()), std=float(a.std(ddof=1)), ratio=float(abs(a.mean()) / a.std(ddof=1)))


def describe(c):
    """the facts a case of any of the three families claims, computed on the references alone"""
    if "bad_masks" in c:
        return describe_returns(c)
    if "obs_feat" in c:
        return describe_relabel(c, relabel_refs((c.F, c.Hd, c.T, c.N), c.regime)[2])
    return describe_adv(c)
