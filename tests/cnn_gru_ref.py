"""The arbiter of the recurrent CNN base, CNNBase(recurrent=True) (a2c/model.py:117-230): nothing in it is derived by hand.  The
convolutions and the FC layer are tests/cnn_ref.py's `trunk`, the GRU is the real torch.nn.GRU stepped with h * mask_t
(tests/autograd_ref.py's `gru_states`; the float32 admission runs the same module at float32), the heads are cnn_ref's `heads` on
the GRU state, PPO's loss is autograd_ref's `ppo_loss`, and every gradient is torch.autograd's in float64.  Nothing touches the
library.

Flat order (state_dict of the reference's Policy): base.gru.{weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0} first --
NNBase.__init__ creates the GRU before CNNBase.__init__ creates `main` -- then cnn_ref.param_shapes.

CASES come from seeds written below.  A gradient case counts only when, on the references alone,
  * every ReLU pre-activation of the trunk is clear of its kink by cnn_ref.KINK_FACTOR (frames selected as tests/cnn_regimes.py
    selects them, then the finished case held to the condition over all its rows at once) and every row is clear of the loss
    branches by cnn_ref.MARGIN, and
  * torch's float32 CPU gradient of the same expressions lies within 0.5 RTOL of the float64 one in every parameter block
    (cnn_regimes' admission rule).
`python tests/cnn_gru_ref.py` is the search behind SEEDS (capped at 400 per shape); tests/test_cnn_gru_host.py re-checks every
one, so the GPU tests do not search.

MASKS of every case: 0 at t = 0 for one environment, at an interior step, at two consecutive steps, and for one whole
environment (as far as T and N allow); h0 is nonzero.

FAULTS, for the test of the test (`fault_grad`), each on the references alone:
  head_relu_mask  the FC layer's ReLU mask [F > 0] applied to d loss / d h_t at the heads
  no_f_mask       no ReLU mask on d loss / d F (derivative 1 everywhere)
  no_h_mask       h not multiplied by masks[t]
  gate_order      the gates r, z, n of weight_ih permuted to z, n, r
  gru_last        the GRU block placed after base.main.* in the flat order
TILE_FAULTS, what a launch past one tile can lose (each does nothing at all -- distance exactly 0 -- where a step fits one tile of
its kind, which is every GRAD_CASES key; tests/test_cnn_gru_tiles_host.py):
  dx_rows_first_64     no gradient from the GRU's input into the trunk for step rows >= 64 (weight_ih's own gradient is whole)
  scan_envs_first_16   environments j >= 16 of a step hand the heads a detached h_t (the heads' weights keep their gradient)
  wgrad_first_range    the GRU block's weight and bias gradients lack the step rows of every KS range of k_gru_wgrad but the first
  loss_rows_first_256  step rows >= 256 add nothing to the three loss sums or to any gradient; the divisor stays the row count"""
import functools

import numpy as np
import torch

import cnn_ref as cr
import cnn_regimes as cg
from cnn_ref import ar
from helpers import RTOL

F64 = cr.F64
HW = cr.HW
GRU_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def gru_shapes(Hs):
    return [("base.gru.weight_ih_l0", (3 * Hs, Hs)), ("base.gru.weight_hh_l0", (3 * Hs, Hs)),
            ("base.gru.bias_ih_l0", (3 * Hs,)), ("base.gru.bias_hh_l0", (3 * Hs,))]


def param_shapes(C, Hs, dist, P):
    return gru_shapes(Hs) + cr.param_shapes(C, Hs, dist, P)


def n_gru(Hs):
    return cr.num_params(gru_shapes(Hs))


# ------------------------------------------------------------------------------------------------------------ forward
def gru_states(p, x, hxs0, masks, T, mask_h=True, leaf_rows=None):
    """float64: autograd_ref.gru_states itself.  Any other dtype (the float32 admission), mask_h False or leaf_rows (the injected
    defects): the same stepping of the same torch.nn.GRU module at that dtype.  leaf_rows: time-major rows >= leaf_rows go through
    the module with detached copies of its four tensors (the state and the input keep their gradient), the others with the leaves:
    two calls per step on the two column subsets."""
    if x.dtype == F64 and mask_h and leaf_rows is None:
        return ar.gru_states(p, x, hxs0, masks, T)
    H = p["base.gru.weight_hh_l0"].shape[1]
    gru = torch.nn.GRU(H, H).to(x.dtype)
    weights = {k: p["base.gru." + k] for k in GRU_NAMES}
    detached = {k: w.detach() for k, w in weights.items()}
    n = x.shape[0] // T
    h, out = ar.t64(hxs0).to(x.dtype).unsqueeze(0), []
    masks = ar.t64(masks).to(x.dtype).reshape(T, n)
    for t in range(T):
        hin = h * masks[t].view(1, n, 1) if mask_h else h
        xt = x[t * n:(t + 1) * n].unsqueeze(0)
        if leaf_rows is None:
            y, h = torch.func.functional_call(gru, weights, (xt, hin))
            out.append(y[0])
            continue
        cut = min(n, max(0, leaf_rows - t * n))
        ys, hs = [], []
        for w, cols in ((weights, slice(0, cut)), (detached, slice(cut, n))):
            if cols.stop > cols.start:
                y, hn = torch.func.functional_call(gru, w, (xt[:, cols], hin[:, cols]))
                ys.append(y[0])
                hs.append(hn)
        h = torch.cat(hs, 1)
        out.append(torch.cat(ys, 0))
    return torch.cat(out, 0)


class _MaskedIdentity(torch.autograd.Function):
    """identity forward; backward multiplied by [other > 0] (the head_relu_mask defect)"""

    @staticmethod
    def forward(ctx, h, other):
        ctx.save_for_backward(other)
        return h.clone()

    @staticmethod
    def backward(ctx, g):
        (other,) = ctx.saved_tensors
        return g * (other > 0).to(g.dtype), None


def states(p, x, hxs0, masks, T, fault=None, tap=None):
    """-> (h_t [T n, Hs] the heads' input, features [T n, Hs], the trunk's four pre-activations); x [T n, C, 84, 84] time-major"""
    if fault == "no_f_mask":      # relu(z) + (z - z.detach()) [z <= 0]: the same forward, derivative 1 everywhere
        seen = {}

        def tap(name, t):  # noqa: F811
            if name == "zf":
                seen["zf"] = t
            if name == "feat":
                z = seen["zf"]
                return t + (z - z.detach()) * (z <= 0).to(z.dtype)
            return t
    if fault == "dx_rows_first_64" and x.shape[0] > 64:
        def tap(name, t):  # noqa: F811
            return torch.cat([t[:64], t[64:].detach()], 0) if name == "feat" else t
    feat, zs = cr.trunk(p, x, tap=tap)
    pg = p
    if fault == "gate_order":
        Hs = feat.shape[1]
        w = p["base.gru.weight_ih_l0"]
        pg = dict(p)
        pg["base.gru.weight_ih_l0"] = torch.cat([w[Hs:2 * Hs], w[2 * Hs:], w[:Hs]], 0)
    leaf_rows = None
    if fault == "wgrad_first_range":
        n = x.shape[0] // T
        geo = geometry(T, n, 1, feat.shape[1])
        if geo["KS"] > 1:
            leaf_rows = 16 * geo["ranges"][0][1]
    h = gru_states(pg, feat, hxs0, masks, T, mask_h=fault != "no_h_mask", leaf_rows=leaf_rows)
    if fault == "head_relu_mask":
        h = _MaskedIdentity.apply(h, feat.detach())
    if fault == "scan_envs_first_16" and x.shape[0] // T > 16:
        late = (torch.arange(x.shape[0]) % (x.shape[0] // T) >= 16).view(-1, 1)
        h = torch.where(late, h.detach(), h)
    return h, feat, zs


def dist_terms(p, h, actions, dist):
    """the heads on h [rows, Hs] and the distribution's terms at `actions` -> (values [rows], logp [rows], entropy.mean())"""
    out = cr.heads(p, h, dist)
    if dist == "categorical":
        ls = torch.nn.functional.log_softmax(out[1], dim=-1)
        a = torch.as_tensor(np.asarray(actions).reshape(-1).astype(np.int64))
        return out[0], ls.gather(1, a.view(-1, 1))[:, 0], -(ls.exp() * ls).sum(-1).mean()
    acts = torch.as_tensor(np.asarray(actions, np.float64).reshape(h.shape[0], -1), dtype=h.dtype)
    return out[0], ar.normal_log_probs(out[1], out[2], acts), ar.normal_entropy(out[2])


def evaluate(p, x, hxs0, masks, T, actions, dist, fault=None):
    """Policy.evaluate_actions (a2c/model.py:107-114) -> (values [rows], logp [rows], entropy.mean(), h_T [n, Hs])"""
    h, _, _ = states(p, x, hxs0, masks, T, fault)
    return dist_terms(p, h, actions, dist) + (h[-(x.shape[0] // T):],)


def forward64(shapes, params, obs, hxs0, masks, T, dist):
    """float64: [value, head outputs ...] as cnn_ref.forward64, then h_t [T n, Hs]"""
    with torch.no_grad():
        p = cr.leaves(params, shapes)
        h, _, _ = states(p, ar.t64(obs), hxs0, masks, T)
        return [t.numpy() for t in cr.heads(p, h, dist)] + [h.numpy()]


def act64(shapes, params, obs, hxs0, masks, T, dist, noise=None):
    """cnn_ref.act64 on the GRU state -> dict(value, action, logp, margin, hxs [n, Hs] the state after the last step)"""
    out = forward64(shapes, params, obs, hxs0, masks, T, dist)
    n = np.asarray(obs).shape[0] // T
    h = out[-1]
    if dist == "categorical":
        lsm = cr.log_softmax64(out[1])
        if noise is None:
            top = np.sort(out[1], 1)
            act, margin = out[1].argmax(1), float((top[:, -1] - top[:, -2]).min())
        else:
            act, margin = cr.categorical_sample(out[1], noise)
        return dict(value=out[0], action=act, logp=lsm[np.arange(len(act)), act], margin=margin, hxs=h[-n:])
    mean, ls = out[1], out[2]
    act = mean if noise is None else mean + np.exp(ls) * np.asarray(noise, np.float64)
    act = act.astype(np.float32).astype(np.float64)
    lp = (-((act - mean) ** 2) / (2.0 * np.exp(ls) ** 2) - ls - ar.HALF_LOG_2PI).sum(1)
    return dict(value=out[0], action=act, logp=lp, margin=1.0, hxs=h[-n:])


# ------------------------------------------------------------------------------------------------------------ PPO
def ppo_grad(shapes, params, obs, hxs0, masks, T, actions, old_logp, value_preds, returns, adv, dist, use_clipped=True, ecoef=cr.ECOEF,
             fault=None, dtype=F64):
    """One optimizer step on the given time-major rows (obs [T per, C, 84, 84], hxs0 [per, Hs], masks [T per], the rest [T per];
    adv normalised over the WHOLE rollout) -> (flat gradient, losses[3])"""
    t = lambda a: ar.t64(a).to(dtype)  # noqa: E731
    p = cr.leaves(params, shapes, dtype, grad=True)
    B = np.asarray(obs).shape[0]
    if fault == "loss_rows_first_256" and B > 256:
        # ppo_loss on the first 256 rows alone, its means turned back into sums over them divided by B: the entropy term too
        h, _, _ = states(p, t(obs), hxs0, masks, T)
        values, logp, entropy = dist_terms(p, h[:256], np.asarray(actions)[:256], dist)
        cut = lambda a: t(a).reshape(-1)[:256]  # noqa: E731
        total, parts = ar.ppo_loss(values, logp, entropy, cut(old_logp), cut(adv), cut(value_preds), cut(returns), cr.CLIP, cr.VCOEF,
                                   ecoef, use_clipped)
        total, parts = total * (256.0 / B), tuple(x * (256.0 / B) for x in parts)
    else:
        values, logp, entropy, _ = evaluate(p, t(obs), hxs0, masks, T, actions, dist, fault)
        total, parts = ar.ppo_loss(values, logp, entropy, t(old_logp).reshape(-1), t(adv).reshape(-1), t(value_preds).reshape(-1),
                                   t(returns).reshape(-1), cr.CLIP, cr.VCOEF, ecoef, use_clipped)
    g = ar.flat_grad(total, p)
    if fault == "gru_last":
        k = n_gru(p["base.gru.weight_hh_l0"].shape[1])
        g = np.concatenate([g[k:], g[:k]])
    return g, ar.terms(*parts)


# ------------------------------------------------------------------------------------------------------------ cases
def default_masks(T, N):
    m = np.ones((T + 1, N), np.float32)
    m[0, 0] = 0.0                         # t = 0
    if T >= 3:
        m[T // 2, min(1, N - 1)] = 0.0    # an interior step
    if T >= 4:
        m[1, N - 1] = m[2, N - 1] = 0.0   # two consecutive steps
    if N >= 3:
        m[:, 2] = 0.0                     # one whole environment
    return m.reshape(T + 1, N, 1)


def init_params(rng, C, Hs, dist, P, noise=0.02):
    """GRU: orthogonal (gain 1) on each whole [3 Hs, Hs] weight, zero biases (a2c/model.py:126-130); the rest as cnn_ref.init_params;
    plus noise * randn on everything, so that the biases' gradients are looked at"""
    gru = []
    for name, shape in gru_shapes(Hs):
        w = np.zeros(shape) if "bias" in name else cr._orthogonal(rng, shape[0], shape[1], 1.0)
        gru.append((w + noise * rng.standard_normal(shape)).reshape(-1))
    return np.concatenate(gru + [cr.init_params(rng, cr.param_shapes(C, Hs, dist, P), noise)]).astype(np.float32)


# key (C, Hs, dist, P, T, N) -> seed
SEEDS = {(1, 16, "categorical", 5, 4, 4): 0, (2, 20, "gaussian", 3, 3, 3): 0, (1, 18, "categorical", 4, 5, 7): 0,
         (4, 512, "categorical", 6, 3, 2): 0, (1, 16, "gaussian", 3, 3, 3): 0,
         # TILE_CASES (seeds 0 and 1 refuse the 4 x 17 Gaussian shape)
         (1, 16, "categorical", 5, 8, 33): 0, (1, 16, "categorical", 5, 4, 34): 0, (2, 20, "gaussian", 3, 4, 17): 2,
         (4, 512, "categorical", 6, 3, 6): 0}
HEADS = {(4, 512, "categorical", 6, 3, 2): "peaked", (1, 16, "gaussian", 3, 3, 3): "fc_zero", (4, 512, "categorical", 6, 3, 6): "peaked"}
ZERO_UNITS = 2     # "fc_zero": FC units 0, 1 have zero weight rows and zero bias -> F is exactly 0 there in every row


def build(C, Hs, dist, P, T, N, seed=None, head=None):
    key = (C, Hs, dist, P, T, N)
    seed = SEEDS[key] if seed is None else seed
    head = HEADS.get(key, "init") if head is None else head
    rng = np.random.default_rng([seed, C, Hs, P, T, N, 77])
    shapes = param_shapes(C, Hs, dist, P)
    cshapes = cr.param_shapes(C, Hs, dist, P)
    k = n_gru(Hs)
    c = cr.Case(C=C, Hs=Hs, dist=dist, P=P, T=T, N=N, seed=seed, shapes=shapes, head=head, ecoef=cr.ECOEF, regime="off_policy",
                tag=f"cnn-gru {head} C={C} Hs={Hs} {dist}({P}) {T}x{N} seed {seed}")
    params = init_params(rng, C, Hs, dist, P)
    if head == "peaked":
        params[k:] = cg.apply_head(params[k:], cshapes, "peaked", rng)
    elif head == "fc_zero":
        wf, (_, flat) = cg._block(cshapes, "base.main.7.weight")
        bf, _ = cg._block(cshapes, "base.main.7.bias")
        params[k + wf.start:k + wf.start + ZERO_UNITS * flat] = 0.0
        params[k + bf.start:k + bf.start + ZERO_UNITS] = 0.0
    c["params"] = params
    kept, need, tries = [], (T + 1) * N, 0
    while len(kept) < need:       # frame selection as tests/cnn_regimes.py:build_rows
        tries += 1
        assert tries <= 40, f"{c.tag}: {len(kept)} of {need} frames after {tries - 1} batches"
        cand = rng.integers(0, 256, (cg.BATCH, C, HW, HW)).astype(np.float32)
        m, _ = cg.frame_margins(cshapes, params[k:], cand, exempt_zeros=head == "fc_zero")
        kept.extend(cand[i] for i in np.nonzero(m >= cg.SELECT_FACTOR)[0])
    c["obs"] = np.stack(kept[:need]).reshape(T + 1, N, C, HW, HW)
    c["masks"] = default_masks(T, N)
    c["hxs"] = np.zeros((T + 1, N, Hs), np.float32)
    c["hxs"][0] = 0.5 * rng.standard_normal((N, Hs))
    B = T * N
    rows = c.obs[:-1].reshape(B, C, HW, HW)
    out = forward64(shapes, params, rows, c.hxs[0], c.masks[:-1].reshape(-1), T, dist)
    v = out[0]
    if dist == "categorical":
        act = rng.integers(0, P, B)
        if head == "peaked":
            act[:2] = out[1][:2].argmax(1)
        c["actions"] = act.reshape(T, N, 1).astype(np.int64)
        lp = cr.log_softmax64(out[1])[np.arange(B), act]
        u = rng.uniform(0.0, 1.0, B)
        for i in range(B):
            for _ in range(100):
                if cr.categorical_sample(out[1][i:i + 1], u[i:i + 1])[1] >= 2 * cg.SAMPLE_MARGIN:
                    break
                u[i] = rng.uniform()
        c["uniform"] = u.astype(np.float32)
    else:
        a32 = (out[1] + np.exp(out[2]) * rng.standard_normal((B, P))).astype(np.float32)
        c["actions"] = a32.reshape(T, N, P)
        lp = (-((a32 - out[1]) ** 2) / (2.0 * np.exp(out[2]) ** 2) - out[2] - ar.HALF_LOG_2PI).sum(1)
        c["noise"] = rng.standard_normal((B, P)).astype(np.float32)
    vp, ret = np.zeros((T + 1, N, 1)), np.zeros((T + 1, N, 1))
    vp[:T] = (v + rng.uniform(-0.5, 0.5, B)).reshape(T, N, 1)
    ret[:T] = (v + 0.5 * rng.standard_normal(B)).reshape(T, N, 1)
    c["value_preds"], c["returns"] = vp.astype(np.float32), ret.astype(np.float32)
    c["adv"] = ar.normalised_advantages(c.returns[:-1].reshape(-1), c.value_preds[:-1].reshape(-1)).numpy()
    c["action_log_probs"] = (lp + rng.uniform(-0.6, 0.6, B)).reshape(T, N, 1).astype(np.float32)
    return c


def rows_of(c, envs=None):
    """the time-major rows of the minibatch holding environments `envs` (default: all, in order): row t * per + j <- (t, envs[j])"""
    envs = np.arange(c.N) if envs is None else np.asarray(envs)
    T = c.T
    g = lambda a: np.ascontiguousarray(np.asarray(a)[:T][:, envs].reshape((T * len(envs),) + np.asarray(a).shape[2:]))  # noqa: E731
    return dict(obs=g(c.obs), hxs0=c.hxs[0][envs], masks=g(c.masks).reshape(-1), actions=g(c.actions), old_logp=g(c.action_log_probs).reshape(-1),
                value_preds=g(c.value_preds).reshape(-1), returns=g(c.returns).reshape(-1), adv=g(c.adv.reshape(T, c.N, 1)).reshape(-1))


def case_grad(c, envs=None, use_clipped=True, dtype=F64, fault=None):
    r = rows_of(c, envs)
    return ppo_grad(c.shapes, c.params, r["obs"], r["hxs0"], r["masks"], c.T, r["actions"], r["old_logp"], r["value_preds"], r["returns"],
                    r["adv"], c.dist, use_clipped, c.ecoef, fault, dtype)


def margins(c):
    """kink margin of the trunk over all rows at once (exact zeros exempt for the fc_zero head only) and the least distance of a
    row to a branch boundary of the clipped surrogate / value loss, in float64"""
    k = n_gru(c.Hs)
    r = rows_of(c)
    m, exempted = cg.frame_margins(cr.param_shapes(c.C, c.Hs, c.dist, c.P), c.params[k:], r["obs"], exempt_zeros=c.head == "fc_zero")
    with torch.no_grad():
        values, logp, _, _ = evaluate(cr.leaves(c.params, c.shapes), ar.t64(r["obs"]), r["hxs0"], r["masks"], c.T, r["actions"], c.dist)
    v, lp = values.numpy(), logp.numpy()
    ratio = np.exp(lp - r["old_logp"].astype(np.float64))
    vo, R = r["value_preds"].astype(np.float64), r["returns"].astype(np.float64)
    dvv = v - vo
    vc = vo + np.clip(dvv, -cr.CLIP, cr.CLIP)
    u, w = (v - R) ** 2, (vc - R) ** 2
    outside = np.abs(dvv) > cr.CLIP
    branch = min(float(np.min(np.minimum(np.abs(ratio - (1 + cr.CLIP)), np.abs(ratio - (1 - cr.CLIP))))),
                 float(np.min(np.abs(np.abs(dvv) - cr.CLIP))), float(np.min(np.abs(u - w)[outside])) if outside.any() else np.inf)
    return float(m.min()), exempted, branch


@functools.lru_cache(maxsize=None)
def admitted(key, use_clipped=True):
    """-> (float64 gradient, losses, float32 torch gradient's block distances from it, indices where both are exactly 0)"""
    c = case(*key)
    g64, l64 = case_grad(c, use_clipped=use_clipped)
    g32, _ = case_grad(c, use_clipped=use_clipped, dtype=torch.float32)
    return g64, l64, cr.block_distances(g32, g64, c.shapes), np.nonzero((np.asarray(g64) == 0) & (np.asarray(g32) == 0))[0]


def acceptable(c, key=None):
    km, exempted, branch = margins(c)
    ok = km >= cr.KINK_FACTOR and branch >= cr.MARGIN and (exempted == 0 or c.head == "fc_zero")
    if not ok:
        return False, km, branch, None
    g64, _ = case_grad(c)
    g32, _ = case_grad(c, dtype=torch.float32)
    d = cr.block_distances(g32, g64, c.shapes)
    return max(d.values()) <= 0.5 * RTOL, km, branch, max(d.values())


def find_seed(C, Hs, dist, P, T, N, limit=400):
    for seed in range(limit):
        try:
            c = build(C, Hs, dist, P, T, N, seed=seed)
        except AssertionError:
            continue
        ok, km, branch, d32 = acceptable(c)
        if ok:
            return seed, km, branch, d32
    raise RuntimeError(f"no seed below {limit} admits ({C}, {Hs}, {dist}, {P}, {T}x{N}): shorten T before loosening anything")


@functools.lru_cache(maxsize=None)
def case(C, Hs, dist, P, T, N):
    """build() at the committed seed, once per process (callers must not write into it)"""
    return build(C, Hs, dist, P, T, N)


FAULTS = ("head_relu_mask", "no_f_mask", "no_h_mask", "gate_order", "gru_last")
# the one-step gradient cases of tests/test_gpu_cnn_gru.py: key -> num_mini_batch
GRAD_CASES = {(1, 16, "categorical", 5, 4, 4): 2, (2, 20, "gaussian", 3, 3, 3): 2, (1, 18, "categorical", 4, 5, 7): 1,
              (4, 512, "categorical", 6, 3, 2): 1, (1, 16, "gaussian", 3, 3, 3): 1}
PERM_SEED = 3
# at max_grad_norm = 0.5 the clip acts in every optimizer step of every case but this one, whose gradient norm stays below 0.5
# (tests/test_cnn_gru_host.py holds both statements on the references)
CLIP_INACTIVE = {(1, 18, "categorical", 4, 5, 7)}
# the one-step gradient cases of tests/test_gpu_cnn_gru_tiles.py, past one row tile, one scan tile and one loss block: key ->
# num_mini_batch (geometry() below and tests/test_cnn_gru_tiles_host.py's FACTS say which edge each one sits on)
TILE_CASES = {(1, 16, "categorical", 5, 8, 33): 1, (1, 16, "categorical", 5, 4, 34): 2, (2, 20, "gaussian", 3, 4, 17): 1,
              (4, 512, "categorical", 6, 3, 6): 1}
# max_grad_norm at which the clip acts in every optimizer step of a TILE_CASES key under both value losses: half the smallest
# float64 step-gradient norm of the case, two significant digits (tests/test_cnn_gru_tiles_host.py recomputes each)
TILE_CLIP = {(1, 16, "categorical", 5, 8, 33): 0.037, (1, 16, "categorical", 5, 4, 34): 0.15, (2, 20, "gaussian", 3, 4, 17): 0.92,
             (4, 512, "categorical", 6, 3, 6): 38.0}
TILE_FAULTS = ("dx_rows_first_64", "scan_envs_first_16", "wgrad_first_range", "loss_rows_first_256")
LDS_ROOM = 160 * 1024 - 1024     # a gfx950 workgroup's LDS less the 1 KiB the launchers leave


def geometry(T, N, M, Hs, cus=256):
    """The launch arithmetic of one optimizer step of cnn_gru_ppo_update (simgan_amd/csrc/sg_ppo.hip), restated: per, S, mb; rows_p,
    the 16-row chunks, KS and the chunk range [c0, c1) of every blockIdx.y of k_gru_wgrad; the scans' workgroups and the live rows
    of the last one; k_cnn_head_loss's blocks; k_gru_dx's grid by both formulas and the tiles each workgroup walks; which instances
    run, by the LDS sizes of sg_gru_dx_lds / sg_gru_scan_lds / sg_gru_bwd_lds (the GRU reads the Hs features: O = H = Hs)."""
    per = N // M
    assert N % per == 0
    mb = T * per
    rows_p = (mb + 15) & ~15
    chunks = rows_p // 16
    KS = max(1, min(16, chunks // 8))
    each = (chunks + KS - 1) // KS
    ranges = [(ks * each, min(chunks, ks * each + each)) for ks in range(KS)]
    Hp = (Hs + 15) & ~15
    ld = Hp + 4
    dx_lds = 4 * (3 * Hp * ld + 16 * (3 * Hp + 4))
    scan_lds = 4 * (3 * Hp * ld + 2 * 16 * ld)
    bwd_lds = 4 * (3 * Hp * ld + 16 * ld + 16 * (3 * Hp + 4))
    gw_dx, gw_scan = dx_lds > LDS_ROOM, scan_lds > LDS_ROOM or bwd_lds > LDS_ROOM
    dx_grid_lds, dx_grid_gw = min((chunks + 3) // 4, cus), min(chunks, cus)
    tiles = (mb + 15) // 16     # k_gru_dx walks base = blockIdx.x * 16, + gridDim.x * 16, ... while base < mb
    walk = lambda grid: [list(range(b, tiles, grid)) for b in range(grid)]  # noqa: E731
    return dict(per=per, S=N // per, mb=mb, rows_p=rows_p, pad_rows=rows_p - mb, chunks=chunks, KS=KS, each=each, ranges=ranges,
                sizes=[max(0, c1 - c0) for c0, c1 in ranges], scan_workgroups=(per + 15) // 16, last_live=per - 16 * ((per - 1) // 16),
                loss_blocks=(mb + 255) // 256, Hp=Hp, gw_dx=gw_dx, gw_scan=gw_scan, dx_grid_lds=dx_grid_lds, dx_grid_gw=dx_grid_gw,
                dx_grid=dx_grid_gw if gw_dx else dx_grid_lds, dx_walk_lds=walk(dx_grid_lds), dx_walk_gw=walk(dx_grid_gw),
                last_tile_live=mb - 16 * ((mb - 1) // 16))


def step_envs(key, M, perm):
    """the environments of every optimizer step of one epoch: per = N // M, N // per steps (a2c/storage.py:196-202)"""
    N = key[5]
    per = N // M
    return [np.asarray(perm[s:s + per]) for s in range(0, N, per)]


TIER2 = [(1, 16, "categorical", 5, 4, 4), (2, 20, "gaussian", 3, 3, 3)]


def tier2():
    """Only where the reference checkout is present, in a process of its own (tools/ref_import.py): the reference's own
    Policy((C, 84, 84), space, base_kwargs={'recurrent': True}) after .double() -- its state_dict keys against param_shapes, its
    evaluate_actions against `evaluate`, and the .grad its own PPO.update (one epoch, one minibatch, both value losses) leaves against
    `case_grad`.  Nothing of the reference is copied: it is imported.  -> {label: dict(keys_equal, forward, worst_block, worst, loss_error)}"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (root, os.path.join(root, "tools"), os.path.join(root, "tests")):
        if path not in sys.path:
            sys.path.insert(0, path)
    cases = [case(*key) for key in TIER2]
    from ref_import import Box, import_reference
    ns = import_reference()

    class Discrete(object):
        def __init__(self, n):
            self.n = n
    out = {}
    for c in cases:
        sp = Discrete(c.P) if c.dist == "categorical" else Box(shape=(c.P,))
        for uc in (True, False):
            policy = ns.Policy((c.C, HW, HW), sp, base_kwargs={"recurrent": True, "hidden_size": c.Hs}).double()
            sd = {k: v.detach().clone() for k, v in cr.leaves(c.params, c.shapes).items()}
            keys_equal = list(policy.state_dict()) == list(sd)
            policy.load_state_dict(sd)
            ro = ns.RolloutStorage(c.T, c.N, (c.C, HW, HW), sp, c.Hs, 1)
            for name in ("obs", "value_preds", "returns", "action_log_probs", "masks"):
                setattr(ro, name, ar.t64(c[name]))
            ro.actions = torch.as_tensor(c.actions) if c.dist == "categorical" else ar.t64(c.actions)
            ro.obs_feat, ro.recurrent_hidden_states = ro.obs_feat.double(), ar.t64(c.hxs)
            r = rows_of(c)
            with torch.no_grad():
                a = torch.as_tensor(r["actions"]) if c.dist == "categorical" else ar.t64(r["actions"])
                rv, rlp, rent, rh = policy.evaluate_actions(ar.t64(r["obs"]), ar.t64(r["hxs0"]), ar.t64(r["masks"]).view(-1, 1), a)
                v, lp, ent, h = evaluate(cr.leaves(c.params, c.shapes), ar.t64(r["obs"]), r["hxs0"], r["masks"], c.T, r["actions"], c.dist)
            fwd = max(float((rv.view(-1) - v).abs().max()), float((rlp.view(-1) - lp).abs().max()), float((rent - ent).abs()), float((rh - h).abs().max()))
            # one minibatch of all environments: the reference draws its own permutation, which only reorders the columns
            losses = ns.PPO(policy, cr.CLIP, 1, 1, cr.VCOEF, c.ecoef, lr=cr.LR, eps=cr.EPS, max_grad_norm=1e9, use_clipped_value_loss=uc).update(ro)
            got = np.concatenate([q.grad.reshape(-1).numpy() for q in policy.parameters()])
            g, la = case_grad(c, use_clipped=uc)
            d = cr.block_distances(got, g, c.shapes, atol=0.0)
            worst = max(d, key=d.get)
            out[f"{c.tag} {'clipped' if uc else 'plain'}"] = dict(keys_equal=keys_equal, forward=fwd, worst_block=worst, worst=d[worst],
                                                                  loss_error=float(np.max(np.abs(la - np.asarray(losses, np.float64)))))
    return out


if __name__ == "__main__":   # the search behind SEEDS; `--tier2` prints tier 2 (the child process of tests/test_cnn_gru_host.py)
    import sys
    if "--tier2" in sys.argv:
        import json
        print("TIER2 " + json.dumps(tier2()))
        sys.exit(0)
    keys = [k for k in SEEDS if not sys.argv[1:] or str(k[1]) in sys.argv[1:]]
    for key in keys:
        print(key, find_seed(*key), flush=True)
