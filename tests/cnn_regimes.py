"""Cases for the CNN base off the regime of tests/cnn_ref.py's six: heads away from their initialisation, the default width, more
rows than one slab / one block of the loss kernels holds, and ReLU pre-activations at exactly 0.  Everything is built on the
references alone (tests/cnn_ref.py, tests/a2c_cnn_ref.py: their forward, losses and autograd are imported, not restated); nothing
touches the library.  tests/test_cnn_regimes_host.py re-proves every condition below for every case, tests/test_gpu_cnn_regimes.py
holds the kernels to the cases.

FRAMES.  cnn_ref searches whole-case seeds for one clear of the ReLU kinks, which succeeds about once in ten at 17 rows and never
at 513.  The kink condition is a property of (params, one frame), so `build_rows` draws candidate frames in batches and keeps a
frame only where every ReLU pre-activation of its float64 forward lies at least SELECT_FACTOR = 2 KINK_FACTOR times its layer's
float32-forward error (the largest over the batch) from zero; the finished case is then held to cr.kink_margin's own condition at
KINK_FACTOR over all of its rows at once, and to cr.acceptable's branch margins.

HEADS.  Each regime is a condition on the float64 forward that the builder asserts:
  "peaked"  dist.linear scaled by PEAK_SCALE and its biases spread over +-PEAK_BIAS: over the case's rows some class probability
            >= 0.9 and some <= 1e-3; rows 0, 1 take their mode, rows 2, 3 their least likely class (log-prob <= -4)
  "sigma"   the log-std a permutation of linspace(-2, 1, A): one <= -1.5, one >= 0.5; actions drawn from those sigmas
  "relu_zero"  eight conv1 channels with bias exactly 0 and two all-zero frames (pre-activation exactly 0 at all 400 pixels of
            both frames), four FC units with zero weight rows and zero bias (exactly 0 in every row); every other bias at least
            0.05 from 0.  The kink condition exempts a unit only where the float64 AND the float32 forward give exactly 0.
            torch's derivative of ReLU at 0 is 0: the FC units' bias and weight gradients are exactly 0.

ADMISSION.  A case counts only where torch's float32 CPU gradient of the same expressions lies within 0.5 RTOL of the float64
one in every block (`admitted`).  Where the edge was, measured on the "default" case's PPO gradient (worst block dist.linear.bias;
the ratio's exp amplifies the rounding of logits of size |log-prob|): PEAK_SCALE 60 leaves the rarest taken action at log-prob
-13.9 and float32 at 0.08 RTOL, 150 at -33 and 0.30 RTOL, 400 at -88 and 0.91 RTOL -- no longer a case.  "peaked-18" stays below
0.17 RTOL up to 400.  PEAK_SCALE = 60 keeps a factor 6 to the edge.  The log-std range [-2, 1] is admitted as it stands
(0.13 RTOL).

FAULTS, for the test of the test (`fault_grad`), each injected into the float64 reference gradient:
  rows_first_256   the loss kernels' rows past the first block of 256 contribute nothing (gradient and the three loss sums)
  slab_cap_drop    conv1's reduction rows (image, oy, ox) past 32 * 512 dropped from its weight and bias gradient
  fc_one_slab      rows past 512 dropped from the FC layer's weight and bias gradient
  k_tail           the last Hs % 4 features dropped from the FC layer's data gradient (their own weight rows keep theirs)
  relu_ge          ReLU's derivative taken as 1 at exactly 0
  ent_at_uniform   the entropy's gradient evaluated at the uniform distribution, where it vanishes
  sigma_unit       var taken as 1 in d loss / d log-std
tests/test_cnn_regimes_host.py lists which of them the old cases cannot see."""
import functools

import numpy as np
import torch

import a2c_cnn_ref as a2
import cnn_ref as cr
from cnn_ref import ar
from helpers import RTOL

HW = cr.HW
SELECT_FACTOR = 2.0 * cr.KINK_FACTOR
BATCH = 64
PEAK_SCALE, PEAK_BIAS = 60.0, 2.0
BIAS_CLEAR = 0.05
ZERO_CHANNELS, ZERO_UNITS, ZERO_FRAMES = 8, 4, (1, 3)
SAMPLE_MARGIN = 1e-4

# tag -> the case; every seed was found by `python tests/cnn_regimes.py` and is re-checked by tests/test_cnn_regimes_host.py
SPECS = {
    "peaked-18": dict(C=1, Hs=16, dist="categorical", P=18, T=3, N=5, head="peaked", seed=0),
    "peaked-ent": dict(C=1, Hs=16, dist="categorical", P=18, T=3, N=5, head="peaked", seed=0, ecoef=1.0),
    "one-class": dict(C=1, Hs=16, dist="categorical", P=1, T=1, N=3, head="init", seed=0),
    "sigma-17": dict(C=2, Hs=18, dist="gaussian", P=17, T=3, N=3, head="sigma", seed=0),
    "hs-40": dict(C=1, Hs=40, dist="categorical", P=5, T=2, N=3, head="init", seed=0),
    "default": dict(C=4, Hs=512, dist="categorical", P=6, T=3, N=2, head="peaked", seed=0),
    "rows-41": dict(C=1, Hs=16, dist="categorical", P=5, T=1, N=41, head="init", seed=0),
    "rows-513": dict(C=1, Hs=16, dist="categorical", P=5, T=27, N=19, head="init", seed=0),
    "branches-513": dict(C=1, Hs=16, dist="categorical", P=5, T=27, N=19, head="init", seed=0, regime="branches"),
    "relu-zero": dict(C=1, Hs=16, dist="gaussian", P=3, T=1, N=4, head="relu_zero", seed=0),
}
TAGS = list(SPECS)
A2C_TAGS = [t for t in TAGS if t != "branches-513"]
PLAIN_TAGS = ["peaked-18", "sigma-17", "rows-513"]            # the plain value loss as well
FORWARD_TAGS = ["peaked-18", "sigma-17", "hs-40", "default"]
A2C_CHUNKS = [("rows-513", 256), ("rows-513", 512), ("rows-41", 40)]     # 256 + 256 + 1, 512 + 1, 40 + 1 rows
GATHER_TAG, GATHER_M, GATHER_PERM_SEED = "rows-513", 3, 0
# fault -> the new case that must see it; DROPPED: faults an old case of cr.GRAD_CASES already sees (their figures are in
# tests/test_cnn_regimes_host.py's docstring), so they close no gap and are only held to be seen by both
FAULTS = {"rows_first_256": "rows-513", "slab_cap_drop": "rows-41", "fc_one_slab": "rows-513", "k_tail": "sigma-17",
          "relu_ge": "relu-zero"}
DROPPED = {"ent_at_uniform": "peaked-ent", "sigma_unit": "sigma-17"}


def slab_arithmetic(n):
    """csrc/sg_cnn.hip's cnn_wgrad_slabs / rows_per_slab restated: layer -> (reduction rows, slabs, rows per slab)"""
    out = {}
    for name, per in (("conv1", 400), ("conv2", 81), ("conv3", 49), ("fc", 1)):
        rows = n * per
        s = min(32, max(1, (rows + 511) // 512))
        out[name] = (rows, s, ((rows + s - 1) // s + 3) & ~3)
    return out


# ------------------------------------------------------------------------------------------------------------ kinks
def frame_margins(shapes, params, obs, exempt_zeros=False):
    """cr.kink_margin's quantity per frame: min over the four ReLU layers of min|z64| / max|z32 - z64|, the error taken over the
    whole batch's layer -> (margins [n], number of exempted units).  exempt_zeros: a unit at which both forwards give exactly 0
    is left out (and only such a unit)."""
    n = obs.shape[0]
    with torch.no_grad():
        _, z64 = cr.trunk(cr.leaves(params, shapes), ar.t64(obs))
        p32 = {k: v.detach().to(torch.float32) for k, v in cr.leaves(params, shapes).items()}
        _, z32 = cr.trunk(p32, torch.as_tensor(np.asarray(obs, np.float32)))
    out, exempted = np.full(n, np.inf), 0
    for a, b in zip(z64, z32):
        a, b = a.numpy().reshape(n, -1), b.to(cr.F64).numpy().reshape(n, -1)
        err = max(float(np.abs(b - a).max()), 1e-300)
        mag = np.abs(a)
        if exempt_zeros:
            both = (a == 0.0) & (b == 0.0)
            exempted += int(both.sum())
            mag = np.where(both, np.inf, mag)
        out = np.minimum(out, mag.min(1) / err)
    return out, exempted


# ------------------------------------------------------------------------------------------------------------ heads
def _block(shapes, name):
    off = 0
    for k, shape in shapes:
        n = int(np.prod(shape))
        if k == name:
            return slice(off, off + n), shape
        off += n
    raise KeyError(name)


def apply_head(params, shapes, head, rng):
    params = params.copy()
    if head == "peaked":
        w, _ = _block(shapes, "dist.linear.weight")
        b, (P,) = _block(shapes, "dist.linear.bias")
        params[w] *= PEAK_SCALE
        params[b] = rng.permutation(np.linspace(-PEAK_BIAS, PEAK_BIAS, P))
    elif head == "sigma":
        s, (A, _) = _block(shapes, "dist.logstd._bias")
        params[s] = rng.permutation(np.linspace(-2.0, 1.0, A))
    elif head == "relu_zero":
        for name, shape in shapes:      # every bias at least BIAS_CLEAR from 0
            if name.endswith(".bias"):
                sl, _ = _block(shapes, name)
                params[sl] = rng.choice([-1.0, 1.0], shape) * rng.uniform(BIAS_CLEAR, 3 * BIAS_CLEAR, shape)
        b1, _ = _block(shapes, "base.main.0.bias")
        params[b1.start:b1.start + ZERO_CHANNELS] = 0.0
        wf, (Hs, flat) = _block(shapes, "base.main.7.weight")
        bf, _ = _block(shapes, "base.main.7.bias")
        params[wf.start:wf.start + ZERO_UNITS * flat] = 0.0
        params[bf.start:bf.start + ZERO_UNITS] = 0.0
    else:
        assert head == "init", head
    return params.astype(np.float32)


def head_facts(c):
    """the float64 forward's figures the head regimes are stated in"""
    r = cr.rows_of(c)
    out = cr.forward64(c.shapes, c.params, r["obs"], c.dist)
    if c.dist == "categorical":
        ls = cr.log_softmax64(out[1])
        taken = ls[np.arange(ls.shape[0]), r["actions"].reshape(-1)]
        return dict(p_max=float(np.exp(ls).max()), p_min=float(np.exp(ls).min()), rare=int((taken <= -4.0).sum()),
                    modes=int((r["actions"].reshape(-1) == out[1].argmax(1)).sum()), logp_min=float(taken.min()))
    ls = out[2][0]
    return dict(logstd_min=float(ls.min()), logstd_max=float(ls.max()))


def head_holds(c):
    f = head_facts(c)
    if c.head == "peaked":
        return f["p_max"] >= 0.9 and f["p_min"] <= 1e-3 and f["rare"] >= 2 and f["modes"] >= 2
    if c.head == "sigma":
        return f["logstd_min"] <= -1.5 and f["logstd_max"] >= 0.5
    return True


# ------------------------------------------------------------------------------------------------------------ the builder
def build_rows(C, Hs, dist, P, T, N, head="init", seed=0, regime="off_policy", ecoef=cr.ECOEF, tag=None):
    """-> a cr.Case (params, obs, actions, value_preds, returns, action_log_probs, adv as cr.build leaves them) with `head`,
    `ecoef`, and for the forward tests `uniform` [T N] (Categorical: draws SAMPLE_MARGIN clear of every cumulative boundary) or
    `noise` [T N, A] (Gaussian).  params and obs depend on (seed, shape, head) alone, so "branches" has "off_policy"'s rows."""
    rng = np.random.default_rng([seed, C, Hs, P, T, N, ["init", "peaked", "sigma", "relu_zero"].index(head)])
    shapes = cr.param_shapes(C, Hs, dist, P)
    B = T * N
    c = cr.Case(C=C, Hs=Hs, dist=dist, P=P, T=T, N=N, regime=regime, seed=seed, shapes=shapes, head=head, ecoef=ecoef,
                tag=tag or f"{regime} {head} C={C} Hs={Hs} {dist}({P}) {T}x{N} seed {seed}")
    c["params"] = apply_head(cr.init_params(rng, shapes), shapes, head, rng)
    kept, need, tries = [], (T + 1) * N, 0
    while len(kept) < need:
        tries += 1
        assert tries <= 40, f"{c.tag}: {len(kept)} of {need} frames after {tries - 1} batches"
        cand = rng.integers(0, 256, (BATCH, C, HW, HW)).astype(np.float32)
        m, _ = frame_margins(shapes, c.params, cand, exempt_zeros=head == "relu_zero")
        kept.extend(cand[i] for i in np.nonzero(m >= SELECT_FACTOR)[0])
    obs = np.stack(kept[:need]).reshape(T + 1, N, C, HW, HW)
    if head == "relu_zero":
        for i in ZERO_FRAMES:
            obs[i // N, i % N] = 0.0
    c["obs"] = obs
    actions = None
    if dist == "categorical":
        logits = cr.forward64(shapes, c.params, obs[:-1].reshape(B, C, HW, HW), dist)[1]
        actions = rng.integers(0, P, B)
        if head == "peaked":
            actions[:2] = logits[:2].argmax(1)
            actions[2:4] = logits[2:4].argmin(1)
    cr.complete(c, np.random.default_rng([seed, C, Hs, P, T, N, 100 + ["off_policy", "branches"].index(regime)]), actions)
    if dist == "categorical":
        u = rng.uniform(0.0, 1.0, B)
        for i in range(B):
            for _ in range(100):
                if cr.categorical_sample(logits[i:i + 1], u[i:i + 1])[1] >= 2 * SAMPLE_MARGIN:
                    break
                u[i] = rng.uniform()
        c["uniform"] = u.astype(np.float32)
    else:
        c["noise"] = rng.standard_normal((B, P)).astype(np.float32)
    assert head_holds(c), (c.tag, head_facts(c))
    return c


def acceptable(c):
    """cr.acceptable with the exemption for exact zeros (only the relu_zero head may use it) -> (ok, kink margin, exempted
    units, classes, margins)"""
    r = cr.rows_of(c)
    m, exempted = frame_margins(c.shapes, c.params, r["obs"], exempt_zeros=c.head == "relu_zero")
    km = float(m.min())
    classes, margins = cr.describe(c)
    ok = km >= cr.KINK_FACTOR and min(margins["ratio"], margins["value"], margins["uw"]) >= cr.MARGIN
    if c.regime == "branches":
        ok = ok and min(classes.values()) >= 1 and margins["adv"] >= 1e-3
    if c.head != "relu_zero":
        ok = ok and exempted == 0 and cr.acceptable(c)[0]
    return ok, km, exempted, classes, margins


@functools.lru_cache(maxsize=None)
def case(tag):
    """the case of a tag, built once per process (callers must not write into it)"""
    return build_rows(tag=tag, **SPECS[tag])


# ------------------------------------------------------------------------------------------------------------ gradients
def _ppo_args(c, rows=None):
    r = cr.rows_of(c)
    keys = ("obs", "actions", "old_logp", "value_preds", "returns", "adv")
    return (c.shapes, c.params) + tuple(r[k] if rows is None else r[k][rows] for k in keys) + (c.dist,)


def ppo_grad(c, use_clipped=True, rows=None, dtype=cr.F64, tap=None):
    """cr.ppo_grad on the case's rows (or the given subset, advantages normalised over the whole rollout) at the case's ecoef"""
    return cr.ppo_grad(*_ppo_args(c, rows), use_clipped, c.ecoef, dtype=dtype, tap=tap)


def a2c_grad(c, dtype=cr.F64):
    return a2.case_grad(c, ecoef=c.ecoef, dtype=dtype)


@functools.lru_cache(maxsize=None)
def admitted(tag, algo="ppo", use_clipped=True):
    """-> (float64 gradient, float64 losses, the float32 torch gradient's per-block distances from it, the indices at which both
    gradients are exactly 0); computed once"""
    c = case(tag)
    if algo == "ppo":
        g64, l64 = ppo_grad(c, use_clipped)
        g32, _ = ppo_grad(c, use_clipped, dtype=torch.float32)
    else:
        g64, l64 = a2c_grad(c)
        g32, _ = a2c_grad(c, dtype=torch.float32)
    return g64, l64, cr.block_distances(g32, g64, c.shapes), np.nonzero((np.asarray(g64) == 0) & (np.asarray(g32) == 0))[0]


def exact_zero_elements(tag, algo="ppo", use_clipped=True):
    """indices into the flat gradient at which torch gives exactly 0 in float64 AND in float32: the units ReLU switches off in
    every row, those at exactly 0 included (derivative 0 there).  The library's gradient must be exactly 0 at them too."""
    return admitted(tag, algo, use_clipped)[3]


GATHER_WEIGHTS = (0.9 * 0.9 * 0.1, 0.9 * 0.1, 0.1)      # Adam's first moment after three steps at lr = 0


@functools.lru_cache(maxsize=None)
def _gather_reference(tag):
    c = case(tag)
    B = c.T * c.N
    perm = np.random.default_rng(GATHER_PERM_SEED).permutation(B).astype(np.int64)
    mb = B // GATHER_M
    parts = [ppo_grad(c, rows=perm[k * mb:(k + 1) * mb])[0] for k in range(GATHER_M)]      # advantages normalised over all rows
    return sum(w * g for w, g in zip(GATHER_WEIGHTS, parts)), parts, perm


def gather_reference(c):
    """E = 1, M = 3 at lr = 0 with an injected permutation: m = 0.9^2 0.1 g1 + 0.9 0.1 g2 + 0.1 g3, each g autograd's on exactly
    its 171 permuted rows -> (m, [g1, g2, g3], permutation)"""
    return _gather_reference(c.tag)


def zero_unit_elements(c):
    """indices into the flat gradient of the relu_zero head's FC units: their bias and weight-row gradients are exactly 0"""
    wf, (Hs, flat) = _block(c.shapes, "base.main.7.weight")
    bf, _ = _block(c.shapes, "base.main.7.bias")
    return np.concatenate([np.arange(wf.start, wf.start + ZERO_UNITS * flat), np.arange(bf.start, bf.start + ZERO_UNITS)])


# ------------------------------------------------------------------------------------------------------------ faults
def _relu_ge_tap():
    """derivative 1 where a pre-activation is exactly 0: a = relu(z) + (z - z.detach()) [z == 0], the same forward"""
    seen = {}

    def tap(name, t):
        if name in ("z1", "z2", "z3", "zf"):
            seen[name] = t
            return t
        z = seen[{"a1": "z1", "a2": "z2", "a3": "z3", "feat": "zf"}[name]]
        return t + (z - z.detach()) * (z == 0).to(z.dtype)
    return tap


def _detach_tap(name, keep):
    """the gradient stops at `name` wherever keep (broadcast to the tensor) is 0; the forward is unchanged"""
    def tap(which, t):
        if which != name:
            return t
        k = torch.as_tensor(keep, dtype=t.dtype).expand_as(t)
        return t * k + (t * (1.0 - k)).detach()
    return tap


def fault_grad(c, fault, use_clipped=True):
    """the float64 PPO gradient and losses of the case with one defect injected"""
    B = c.T * c.N
    g, losses = ppo_grad(c, use_clipped)
    g, losses = g.copy(), losses.copy()
    blk = lambda name: _block(c.shapes, name)[0]  # noqa: E731
    if fault == "rows_first_256":          # the loss is a mean of per-row terms: g = sum_r g_r / B
        if B > 256:
            g256, l256 = ppo_grad(c, use_clipped, rows=np.arange(256))
            g, losses = g256 * (256.0 / B), l256 * (256.0 / B)
    elif fault == "fc_one_slab":
        if B > 512:
            g512, _ = ppo_grad(c, use_clipped, rows=np.arange(512))
            for name in ("base.main.7.weight", "base.main.7.bias"):
                g[blk(name)] = g512[blk(name)] * (512.0 / B)
    elif fault == "slab_cap_drop":         # conv1 has no data gradient, so stopping dZ1 there changes its own gradients only
        if B * 400 > 32 * 512:
            keep = (np.arange(B * 400) < 32 * 512).astype(np.float64).reshape(B, 1, 20, 20)
            gd, _ = ppo_grad(c, use_clipped, tap=_detach_tap("z1", keep))
            for name in ("base.main.0.weight", "base.main.0.bias"):
                g[blk(name)] = gd[blk(name)]
    elif fault == "k_tail":                # without the last Hs % 4 units' path into the convolutions; the FC blocks keep theirs
        tail = c.Hs % 4
        if tail:
            keep = (np.arange(c.Hs) < c.Hs - tail).astype(np.float64).reshape(1, c.Hs)
            gd, _ = ppo_grad(c, use_clipped, tap=_detach_tap("zf", keep))
            for name, _ in c.shapes[:6]:
                g[blk(name)] = gd[blk(name)]
    elif fault == "relu_ge":
        g, losses = ppo_grad(c, use_clipped, tap=_relu_ge_tap())
    elif fault == "ent_at_uniform":        # p (log p + H) vanishes at the uniform distribution: no entropy gradient at all
        if c.dist == "categorical":
            saved = c.ecoef
            try:
                c["ecoef"] = 0.0
                g0, _ = ppo_grad(c, use_clipped)
            finally:
                c["ecoef"] = saved
            for name in [n for n, _ in c.shapes]:
                g[blk(name)] = g0[blk(name)]
    elif fault == "sigma_unit":            # d loss / d logstd_k = sum_r dlogp_r (diff^2 / var - 1) - ecoef, with var = 1
        if c.dist == "gaussian":
            r = cr.rows_of(c)
            p = cr.leaves(c.params, c.shapes)
            values, logp, entropy = cr.evaluate(p, ar.t64(r["obs"]), r["actions"], c.dist)
            total, _ = ar.ppo_loss(values, logp, entropy, ar.t64(r["old_logp"]), ar.t64(r["adv"]), ar.t64(r["value_preds"]), ar.t64(r["returns"]),
                                   cr.CLIP, cr.VCOEF, c.ecoef, use_clipped)
            dlogp = torch.autograd.grad(total, logp)[0].numpy()
            mean = cr.forward64(c.shapes, c.params, r["obs"], c.dist)[1]
            diff = r["actions"].astype(np.float64) - mean
            g[blk("dist.logstd._bias")] = (dlogp[:, None] * (diff * diff - 1.0)).sum(0) - c.ecoef
    else:
        raise KeyError(fault)
    return g, losses


def old_case(key, ecoef=cr.ECOEF):
    """a tests/cnn_ref.py case dressed as one of this file's (for fault_grad on the old cases)"""
    c = cr.Case(cr.case(*key))
    c["head"], c["ecoef"] = "init", ecoef
    return c


if __name__ == "__main__":   # the search behind the seeds, and the figures the docstrings quote
    import sys
    for tag in sys.argv[1:] or TAGS:
        spec = dict(SPECS[tag])
        for seed in range(spec.pop("seed"), 200):
            try:
                c = build_rows(tag=tag, seed=seed, **spec)
            except AssertionError as exc:
                print(tag, seed, "builder:", str(exc)[:200], flush=True)
                continue
            ok, km, exempted, classes, margins = acceptable(c)
            print(tag, seed, ok, round(km, 2), exempted, head_facts(c), margins, flush=True)
            if ok:
                break
