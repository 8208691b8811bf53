"""The arbiter of the CNN base (a2c/model.py:204-230): its forward written with torch.nn.functional.conv2d / linear / relu on
float64 leaves in state_dict order, PPO's loss from tests/autograd_ref.py (imported, not copied: ppo_loss, normalised_advantages,
the Gaussian log-prob / entropy, the float32 constants at float32 value) and torch.autograd for every gradient.  Nothing here is
derived and nothing touches the library; the C oracle has no CNN.

Cases for the gradient tests are built here from seeds written down below.  A ReLU unit whose pre-activation lies within float32
rounding of zero can take a different side in a different summation order, which moves the gradient by far more than the
tolerance; the forward is continuous, the gradient is not.  So a gradient case must keep clear of the kinks ON THE REFERENCES
ALONE: every ReLU pre-activation of the float64 forward satisfies |z| >= KINK_FACTOR * max|z32 - z64| of its layer, z32 being
torch's float32 CPU forward.  Roughly one seed in ten meets that at 17 rows; `find_seed` is the search that produced SEEDS, and
tests/test_cnn_host.py re-checks the condition for every case the GPU tests use, so those do not search."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import autograd_ref as ar
from helpers import ATOL, RTOL

F64 = torch.float64
HW = 84
KINK_FACTOR = 4.0
CLIP, VCOEF, ECOEF, LR, EPS = 0.2, 0.5, 0.01, 3e-4, 1e-5
MARGIN = 1e-4   # no row closer than this to a branch boundary of the clipped surrogate / value loss (tests/regimes.py)


class Case(dict):
    __getattr__ = dict.__getitem__


def param_shapes(C, Hs, dist, P):
    """state_dict order of Policy((C, 84, 84), ...): dist "categorical" (P classes) or "gaussian" (P action dimensions)"""
    head = ([("dist.linear.weight", (P, Hs)), ("dist.linear.bias", (P,))] if dist == "categorical" else
            [("dist.fc_mean.weight", (P, Hs)), ("dist.fc_mean.bias", (P,)), ("dist.logstd._bias", (P, 1))])
    return [("base.main.0.weight", (32, C, 8, 8)), ("base.main.0.bias", (32,)),
            ("base.main.2.weight", (64, 32, 4, 4)), ("base.main.2.bias", (64,)),
            ("base.main.4.weight", (32, 64, 3, 3)), ("base.main.4.bias", (32,)),
            ("base.main.7.weight", (Hs, 32 * 7 * 7)), ("base.main.7.bias", (Hs,)),
            ("base.critic_linear.weight", (1, Hs)), ("base.critic_linear.bias", (1,))] + head


def num_params(shapes):
    return int(sum(np.prod(s) for _, s in shapes))


def blocks(shapes, flat):
    out, off = [], 0
    for name, shape in shapes:
        n = int(np.prod(shape))
        out.append((name, np.asarray(flat)[off:off + n]))
        off += n
    return out


def block_distances(got, ref, shapes, atol=ATOL):
    """tests/regimes.py:block_distances over this policy's blocks: rel-L2 per parameter block with the floor atol * max|ref| * sqrt(n)"""
    ref = np.asarray(ref, np.float64)
    scale = atol * np.max(np.abs(ref))
    out = {}
    for (name, g), (_, r) in zip(blocks(shapes, np.asarray(got, np.float64)), blocks(shapes, ref)):
        out[name] = float(np.sqrt(((g - r) ** 2).sum()) / (np.sqrt((r ** 2).sum()) + scale * np.sqrt(r.size) + 1e-300))
    return out


def leaves(flat, shapes, dtype=F64, grad=None):
    """grad None: float64 leaves take a gradient, others do not (tests/cnn_regimes.py's float32 admission asks for one)"""
    flat = np.asarray(flat, np.float64).reshape(-1)
    out, off = {}, 0
    for name, shape in shapes:
        n = int(np.prod(shape))
        out[name] = torch.as_tensor(np.ascontiguousarray(flat[off:off + n].reshape(shape)), dtype=dtype).requires_grad_(dtype == F64 if grad is None else grad)
        off += n
    assert off == flat.size, (off, flat.size)
    return out


# ------------------------------------------------------------------------------------------------------------ forward
def trunk(p, x, fault=None, tap=None):
    """CNNBase.main on x [n, C, 84, 84] (a2c/model.py:211-215, 225) -> (features [n, Hs], the four pre-activations).  `fault`
    injects one defect, for the test of the test: "no_div255", "flatten_yxc" (ppo_grad has three more).  `tap(name, tensor) ->
    tensor` sees every pre-activation ("z1", "z2", "z3", "zf") and every activation ("a1", "a2", "a3", "feat") and may replace it:
    tests/cnn_regimes.py builds its injected defects from it (a tap that returns what it is given changes nothing)."""
    tap = tap or (lambda name, t: t)
    x = x if fault == "no_div255" else x / 255.0
    z1 = tap("z1", F.conv2d(x, p["base.main.0.weight"], p["base.main.0.bias"], stride=4))
    z2 = tap("z2", F.conv2d(tap("a1", F.relu(z1)), p["base.main.2.weight"], p["base.main.2.bias"], stride=2))
    z3 = tap("z3", F.conv2d(tap("a2", F.relu(z2)), p["base.main.4.weight"], p["base.main.4.bias"], stride=1))
    a3 = tap("a3", F.relu(z3))
    flat = a3.permute(0, 2, 3, 1).reshape(a3.shape[0], -1) if fault == "flatten_yxc" else a3.reshape(a3.shape[0], -1)
    zf = tap("zf", F.linear(flat, p["base.main.7.weight"], p["base.main.7.bias"]))
    return tap("feat", F.relu(zf)), (z1, z2, z3, zf)


def heads(p, feat, dist):
    """-> (value [n], logits [n, K]) or (value [n], mean [n, A], logstd [n, A])"""
    value = F.linear(feat, p["base.critic_linear.weight"], p["base.critic_linear.bias"])[:, 0]
    if dist == "categorical":
        return value, F.linear(feat, p["dist.linear.weight"], p["dist.linear.bias"])
    mean = F.linear(feat, p["dist.fc_mean.weight"], p["dist.fc_mean.bias"])
    return value, mean, torch.zeros_like(mean) + p["dist.logstd._bias"].t().view(1, -1)


def evaluate(p, x, actions, dist, fault=None, tap=None):
    """Policy.evaluate_actions (a2c/model.py:107-114) -> (values [n], logp [n], entropy.mean())"""
    feat, _ = trunk(p, x, fault, tap)
    h = heads(p, feat, dist)
    if dist == "categorical":
        ls = F.log_softmax(h[1], dim=-1)                       # FixedCategorical.log_probs / entropy, a2c/distributions.py:33-48
        a = torch.as_tensor(np.asarray(actions).reshape(-1).astype(np.int64))
        return h[0], ls.gather(1, a.view(-1, 1))[:, 0], -(ls.exp() * ls).sum(-1).mean()
    acts = torch.as_tensor(np.asarray(actions, np.float64).reshape(x.shape[0], -1), dtype=x.dtype)
    return h[0], ar.normal_log_probs(h[1], h[2], acts), ar.normal_entropy(h[2])


def forward64(shapes, params, obs, dist):
    """float64 results of the three policy calls on obs [n, C, 84, 84]: value, head outputs (logits, or mean and logstd)"""
    with torch.no_grad():
        p = leaves(params, shapes)
        feat, _ = trunk(p, ar.t64(obs))
        return [t.numpy() for t in heads(p, feat, dist)]


def categorical_sample(logits, u):
    """the library's convention for injected uniform draws (tests/discrete_ref.py, sg_policy.hip): the first class whose running
    sum of probabilities (ascending index) exceeds u, clamped to K - 1 -> (actions [n], margin: the least distance of u to a
    cumulative boundary, so that a float32 evaluation picks the same class)"""
    z = np.asarray(logits, np.float64)
    pr = np.exp(z - z.max(1, keepdims=True))
    cum = np.cumsum(pr / pr.sum(1, keepdims=True), 1)
    u = np.asarray(u, np.float64).reshape(-1, 1)
    act = np.minimum((cum <= u).sum(1), z.shape[1] - 1)
    return act, float(np.min(np.abs(cum[:, :-1] - u))) if z.shape[1] > 1 else 1.0


def log_softmax64(logits):
    z = np.asarray(logits, np.float64)
    z = z - z.max(1, keepdims=True)
    return z - np.log(np.exp(z).sum(1, keepdims=True))


def act64(shapes, params, obs, dist, noise=None):
    """Policy.act (a2c/model.py:89-101) in float64 -> dict(value, action, logp, margin).  noise None: the mode.  Categorical:
    noise [n] uniform draws; Gaussian: noise [n, A] standard normal, action = mean + exp(logstd) * noise."""
    out = forward64(shapes, params, obs, dist)
    if dist == "categorical":
        lsm = log_softmax64(out[1])
        if noise is None:
            top = np.sort(out[1], 1)
            act, margin = out[1].argmax(1), float((top[:, -1] - top[:, -2]).min())
        else:
            act, margin = categorical_sample(out[1], noise)
        return dict(value=out[0], action=act, logp=lsm[np.arange(len(act)), act], margin=margin)
    mean, ls = out[1], out[2]
    act = mean if noise is None else mean + np.exp(ls) * np.asarray(noise, np.float64)
    act = act.astype(np.float32).astype(np.float64)   # the action crosses the ABI as float32; its log-prob is of THAT number
    lp = (-((act - mean) ** 2) / (2.0 * np.exp(ls) ** 2) - ls - ar.HALF_LOG_2PI).sum(1)
    return dict(value=out[0], action=act, logp=lp, margin=1.0)


# ------------------------------------------------------------------------------------------------------------ PPO
def ppo_grad(shapes, params, obs, actions, old_logp, value_preds, returns, adv, dist, use_clipped=True, ecoef=ECOEF, fault=None,
             dtype=F64, tap=None):
    """One optimizer step's loss and gradient on the given rows: obs [n, C, 84, 84], the rest [n]; adv = the rows' normalised
    advantages (normalised over the WHOLE rollout, a2c/algo/ppo.py:66-68) -> (flat gradient, losses[3]).  dtype torch.float32:
    the same expressions evaluated by torch's float32 CPU kernels (the admission rule of tests/cnn_regimes.py)."""
    t = lambda a: ar.t64(a).to(dtype)  # noqa: E731
    p = leaves(params, shapes, dtype, grad=True)
    values, logp, entropy = evaluate(p, t(obs), actions, dist, fault, tap)
    total, parts = ar.ppo_loss(values, logp, entropy, t(old_logp).reshape(-1), t(adv).reshape(-1), t(value_preds).reshape(-1),
                               t(returns).reshape(-1), CLIP, VCOEF, ecoef, use_clipped)
    g = ar.flat_grad(total, p)
    if fault == "wgrad_khkw":      # conv1's weight gradient with kh and kw swapped
        n = int(np.prod(shapes[0][1]))
        g[:n] = g[:n].reshape(shapes[0][1]).transpose(0, 1, 3, 2).reshape(-1)
    elif fault == "no_conv_bias":  # conv2's bias gradient dropped
        off = num_params(shapes[:3])
        g[off:off + 64] = 0.0
    elif fault == "mask_wrong_layer":   # the FC layer's ReLU derivative taken from conv3's sign pattern instead of its own
        g = _grad_wrong_mask(shapes, params, obs, actions, old_logp, value_preds, returns, adv, dist, use_clipped, ecoef)
    return g, ar.terms(*parts)


class _ReluMaskFrom(torch.autograd.Function):
    """relu(z) forward; backward masked by ANOTHER tensor's sign pattern (the injected defect)"""

    @staticmethod
    def forward(ctx, z, other):
        ctx.save_for_backward(other)
        return z.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        (other,) = ctx.saved_tensors
        return g * (other > 0).to(g.dtype), None


def _grad_wrong_mask(shapes, params, obs, actions, old_logp, value_preds, returns, adv, dist, use_clipped, ecoef):
    p = leaves(params, shapes)
    x = ar.t64(obs) / 255.0
    z1 = F.conv2d(x, p["base.main.0.weight"], p["base.main.0.bias"], stride=4)
    z2 = F.conv2d(F.relu(z1), p["base.main.2.weight"], p["base.main.2.bias"], stride=2)
    z3 = F.conv2d(F.relu(z2), p["base.main.4.weight"], p["base.main.4.bias"], stride=1)
    # the FC layer's ReLU masked by the pattern of conv3's first Hs units instead of its own
    zf = F.linear(F.relu(z3).reshape(z3.shape[0], -1), p["base.main.7.weight"], p["base.main.7.bias"])
    feat = _ReluMaskFrom.apply(zf, z3.reshape(z3.shape[0], -1)[:, :zf.shape[1]].detach())
    h = heads(p, feat, dist)
    if dist == "categorical":
        ls = F.log_softmax(h[1], dim=-1)
        a = torch.as_tensor(np.asarray(actions).reshape(-1).astype(np.int64))
        logp, ent = ls.gather(1, a.view(-1, 1))[:, 0], -(ls.exp() * ls).sum(-1).mean()
    else:
        logp, ent = ar.normal_log_probs(h[1], h[2], ar.t64(actions).reshape(x.shape[0], -1)), ar.normal_entropy(h[2])
    total, _ = ar.ppo_loss(h[0], logp, ent, ar.t64(old_logp).reshape(-1), ar.t64(adv).reshape(-1), ar.t64(value_preds).reshape(-1),
                           ar.t64(returns).reshape(-1), CLIP, VCOEF, ecoef, use_clipped)
    return ar.flat_grad(total, p)


def clip_factor(g, max_grad_norm):
    """clip_grad_norm_'s factor (a2c/algo/ppo.py:143): clamp(max_norm / (||g|| + 1e-6), max=1); NaN where the norm is NaN, as
    torch.clamp leaves it (a one-row rollout: the advantages' unbiased std is NaN in the reference)"""
    coef = max_grad_norm / (float(np.sqrt((np.asarray(g, np.float64) ** 2).sum())) + 1e-6)
    return 1.0 if coef > 1.0 else coef


def adam_update64(shapes, c, perms, E, M, max_grad_norm, use_clipped=True):
    """PPO.update (a2c/algo/ppo.py:63-160) in float64 with torch.optim.Adam's arithmetic: -> (losses[3] averaged over the E * M
    steps, parameters after the update, the first step's gradient)"""
    params = c.params.astype(np.float64).copy()
    B = c.T * c.N
    mb = B // M
    adv = ar.normalised_advantages(c.returns[:-1].reshape(-1), c.value_preds[:-1].reshape(-1)).numpy()
    obs = c.obs[:-1].reshape(B, c.C, HW, HW)
    m, v, t = np.zeros_like(params), np.zeros_like(params), 0
    acc, first = np.zeros(3), None
    for e in range(E):
        for k in range(M):
            idx = np.asarray(perms[e][k * mb:(k + 1) * mb])
            g, losses = ppo_grad(shapes, params, obs[idx], c.actions.reshape(B, -1)[idx], c.action_log_probs.reshape(B)[idx],
                                 c.value_preds[:-1].reshape(B)[idx], c.returns[:-1].reshape(B)[idx], adv[idx], c.dist, use_clipped)
            first = g if first is None else first
            g = g * clip_factor(g, max_grad_norm)
            t += 1
            m = 0.9 * m + 0.1 * g
            v = 0.999 * v + 0.001 * g * g
            params = params - (LR / (1 - 0.9 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + EPS)
            acc += losses
    return acc / (E * M), params, first


# ------------------------------------------------------------------------------------------------------------ cases
def _orthogonal(rng, rows, cols, gain):
    a = rng.standard_normal((rows, cols))
    q, r = np.linalg.qr(a.T if rows < cols else a)
    q = q * np.sign(np.diag(r))
    return gain * (q.T if rows < cols else q)


def init_params(rng, shapes, noise=0.02):
    """the reference's initialisation (orthogonal, ReLU gain for main, 1 for critic_linear, 0.01 / 1 for the heads, zero biases,
    log-std 0) plus noise * randn on everything: biases and the log-std are off zero, so their gradients are looked at"""
    out = []
    for name, shape in shapes:
        if name.endswith("bias"):
            w = np.zeros(shape)
        else:
            gain = np.sqrt(2.0) if name.startswith("base.main") else (0.01 if name.startswith("dist.linear") else 1.0)
            w = _orthogonal(rng, shape[0], int(np.prod(shape[1:])), gain).reshape(shape)
        out.append((w + noise * rng.standard_normal(shape)).reshape(-1))
    return np.concatenate(out).astype(np.float32)


def kink_margin(shapes, params, obs):
    """min over the four ReLU layers of min|z64| / max|z32 - z64|: the references alone"""
    with torch.no_grad():
        _, z64 = trunk(leaves(params, shapes), ar.t64(obs))
        p32 = {k: v.detach().to(torch.float32) for k, v in leaves(params, shapes).items()}
        _, z32 = trunk(p32, torch.as_tensor(np.asarray(obs, np.float32)))
    worst = np.inf
    for a, b in zip(z64, z32):
        err = float((b.to(F64) - a).abs().max())
        worst = min(worst, float(a.abs().min()) / max(err, 1e-300))
    return worst


# (C, Hs, dist, P, T, N, regime) -> seed, found by find_seed; tests/test_cnn_host.py re-checks every one
SEEDS = {(1, 16, "categorical", 5, 1, 1, "off_policy"): 0, (1, 16, "categorical", 5, 1, 3, "off_policy"): 0,
         (1, 16, "categorical", 5, 17, 1, "off_policy"): 1, (3, 20, "gaussian", 3, 3, 5, "off_policy"): 7,
         (1, 16, "categorical", 5, 3, 9, "branches"): 0, (1, 16, "categorical", 5, 4, 4, "off_policy"): 2}


def build(C, Hs, dist, P, T, N, regime="off_policy", seed=None):
    """-> Case with params (float32 flat), obs [T+1, N, C, 84, 84] (float32 holding uint8 values), actions, value_preds, returns,
    action_log_probs ([T(+1), N, 1]) and `adv` [T*N].  regime "off_policy": ratios and value errors spread about the clip;
    "branches": rows dealt round-robin into every branch of the clipped surrogate (above / below / inside the clip x both signs of
    the advantage) and of the clipped value loss (inside; outside with u > w; outside with w > u)."""
    key = (C, Hs, dist, P, T, N, regime)
    seed = SEEDS[key] if seed is None else seed
    rng = np.random.default_rng([seed, C, Hs, P, T, N])
    shapes = param_shapes(C, Hs, dist, P)
    c = Case(C=C, Hs=Hs, dist=dist, P=P, T=T, N=N, regime=regime, seed=seed, shapes=shapes, tag=f"{regime} C={C} Hs={Hs} {dist}({P}) {T}x{N} seed {seed}")
    c["params"] = init_params(rng, shapes)
    c["obs"] = rng.integers(0, 256, (T + 1, N, C, HW, HW)).astype(np.float32)
    return complete(c, rng)


def complete(c, rng, actions=None):
    """the rest of a case from its params and obs: actions (drawn here unless given: Categorical class indices [T * N]), value
    predictions, returns and old log-probs of the case's regime, the normalised advantages"""
    C, dist, P, T, N, regime, shapes = c.C, c.dist, c.P, c.T, c.N, c.regime, c.shapes
    B = T * N
    rows = c.obs[:-1].reshape(B, C, HW, HW)
    out = forward64(shapes, c.params, rows, dist)
    v = out[0]
    if dist == "categorical":
        act = rng.integers(0, P, B) if actions is None else np.asarray(actions).reshape(B)
        c["actions"] = act.reshape(T, N, 1).astype(np.int64)
        lp = log_softmax64(out[1] )[np.arange(B), act]
    else:
        a32 = (out[1] + np.exp(out[2]) * rng.standard_normal((B, P))).astype(np.float32)
        c["actions"] = a32.reshape(T, N, P)
        lp = (-((a32 - out[1]) ** 2) / (2.0 * np.exp(out[2]) ** 2) - out[2] - ar.HALF_LOG_2PI).sum(1)
    vp, ret = np.zeros((T + 1, N, 1)), np.zeros((T + 1, N, 1))
    if regime == "branches":
        vcls = np.arange(B) % 3
        dv = np.where(vcls == 0, rng.uniform(-0.15, 0.15, B), np.where(vcls == 1, rng.uniform(0.3, 0.5, B), rng.uniform(0.3, 0.5, B)))
        vp[:T] = (v - dv).reshape(T, N, 1)                                  # v - v_old = dv: class 0 inside the clip, 1 and 2 outside (above)
        # outside, v_clipped = v_old + clip < v: u = (v - R)^2 > w = (v_c - R)^2 iff R < (v + v_c) / 2
        vc = v - dv + CLIP
        ret[:T] = np.where(vcls == 1, vc - rng.uniform(0.2, 0.6, B), np.where(vcls == 2, v + rng.uniform(0.2, 0.6, B), v + 0.5 * rng.standard_normal(B))).reshape(T, N, 1)
    else:
        vp[:T] = (v + rng.uniform(-0.5, 0.5, B)).reshape(T, N, 1)
        ret[:T] = (v + 0.5 * rng.standard_normal(B)).reshape(T, N, 1)
    c["value_preds"], c["returns"] = vp.astype(np.float32), ret.astype(np.float32)
    adv = ar.normalised_advantages(c.returns[:-1].reshape(-1), c.value_preds[:-1].reshape(-1)).numpy()
    c["adv"] = adv
    if regime == "branches":
        rcls = (np.arange(B) // 3) % 3     # 0 above the clip, 1 below, 2 inside; the advantages' signs are whatever they are
        lr_ = np.where(rcls == 0, rng.uniform(0.3, 0.5, B), np.where(rcls == 1, -rng.uniform(0.3, 0.5, B), rng.uniform(-0.15, 0.15, B)))
        olp = lp - lr_
    else:
        olp = lp + rng.uniform(-0.6, 0.6, B)
    c["action_log_probs"] = olp.reshape(T, N, 1).astype(np.float32)
    return c


def rows_of(c):
    B = c.T * c.N
    return dict(obs=c.obs[:-1].reshape(B, c.C, HW, HW), actions=c.actions.reshape(B, -1), old_logp=c.action_log_probs.reshape(B),
                value_preds=c.value_preds[:-1].reshape(B), returns=c.returns[:-1].reshape(B), adv=c.adv)


def describe(c):
    """classes of the rows and the margins to every branch boundary, in float64"""
    r = rows_of(c)
    with torch.no_grad():
        values, logp, _ = evaluate(leaves(c.params, c.shapes), ar.t64(r["obs"]), r["actions"], c.dist)
    v, lp = values.numpy(), logp.numpy()
    ratio = np.exp(lp - r["old_logp"].astype(np.float64))
    adv, vo, R = r["adv"], r["value_preds"].astype(np.float64), r["returns"].astype(np.float64)
    dvv = v - vo
    vc = vo + np.clip(dvv, -CLIP, CLIP)
    u, w = (v - R) ** 2, (vc - R) ** 2
    above, below, outside = ratio > 1 + CLIP, ratio < 1 - CLIP, np.abs(dvv) > CLIP
    classes = {"above_adv+": int((above & (adv > 0)).sum()), "above_adv-": int((above & (adv < 0)).sum()),
               "below_adv+": int((below & (adv > 0)).sum()), "below_adv-": int((below & (adv < 0)).sum()),
               "inside": int((~above & ~below).sum()), "u>w": int((outside & (u > w)).sum()), "w>u_outside": int((outside & (w > u)).sum()),
               "value_inside": int((~outside).sum())}
    margins = {"ratio": float(np.min(np.minimum(np.abs(ratio - (1 + CLIP)), np.abs(ratio - (1 - CLIP))))),
               "value": float(np.min(np.abs(np.abs(dvv) - CLIP))),
               "uw": float(np.min(np.abs(u - w)[outside])) if outside.any() else np.inf, "adv": float(np.min(np.abs(adv)))}
    return classes, margins


def acceptable(c):
    """what every gradient case must satisfy, on the references alone -> (ok, kink margin, classes, margins)"""
    r = rows_of(c)
    km = kink_margin(c.shapes, c.params, r["obs"])
    classes, margins = describe(c)
    ok = km >= KINK_FACTOR and min(margins["ratio"], margins["value"], margins["uw"]) >= MARGIN
    if c.regime == "branches":
        ok = ok and min(classes.values()) >= 1 and margins["adv"] >= 1e-3
    return ok, km, classes, margins


def find_seed(C, Hs, dist, P, T, N, regime="off_policy", limit=400):
    for seed in range(limit):
        c = build(C, Hs, dist, P, T, N, regime, seed=seed)
        ok, km, classes, margins = acceptable(c)
        if ok:
            return seed, km
    raise RuntimeError(f"no seed below {limit} keeps ({C}, {Hs}, {dist}, {P}, {T}x{N}, {regime}) clear of the ReLU kinks")


@functools.lru_cache(maxsize=None)
def case(C, Hs, dist, P, T, N, regime="off_policy"):
    """build() at the committed seed, once per process (callers must not write into it)"""
    return build(C, Hs, dist, P, T, N, regime)


# the gradient cases of tests/test_gpu_cnn.py (2: one step per block; 3: the minibatch gather; 5, 6: determinism, the learner)
GRAD_CASES = [(1, 16, "categorical", 5, 1, 1, "off_policy"), (1, 16, "categorical", 5, 1, 3, "off_policy"),
              (1, 16, "categorical", 5, 17, 1, "off_policy"), (3, 20, "gaussian", 3, 3, 5, "off_policy"),
              (1, 16, "categorical", 5, 3, 9, "branches")]
GATHER_CASE = (1, 16, "categorical", 5, 4, 4, "off_policy")
GATHER_PERM_SEED = 0


if __name__ == "__main__":   # the search behind SEEDS
    for key in GRAD_CASES + [GATHER_CASE]:
        print(key, find_seed(*key), flush=True)
