"""Float64 arbiter of Policy on Discrete / MultiBinary action spaces: the reference's PPO and A2C losses (a2c/algo/ppo.py:92-108,
a2c/algo/a2c_acktr.py:56-91) over a Categorical / Bernoulli head (a2c/distributions.py:33-88,157-168) written FORWARD-ONLY in
torch.float64 and differentiated by torch.autograd, with the conventions of tests/autograd_ref.py (float32 constants at their
float32 value; nothing derived by hand).  `dtype=torch.float32` evaluates the very same code in float32: the "any float32
evaluation" yardstick of the saturated cases.  `fault=` injects a wrong restatement for the tests of the test.

Also here, for tests/test_discrete_host.py and tests/test_gpu_discrete.py: the duck-typed action spaces, the fixtures' loader, a
numpy restatement of the samplers and the case builders of the per-block gradient checks."""
import json
import os

import numpy as np
import torch

import autograd_ref as ar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CATEGORICAL, BERNOULLI = 1, 2
CLIP, VCOEF, ECOEF = 0.2, 0.5, 0.01
FIXTURES = ("discrete_k2", "discrete_k17", "discrete_k130", "discrete_b1", "discrete_b5", "discrete_b33")


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


class Discrete:
    def __init__(self, n):
        self.n = int(n)


class MultiBinary:
    def __init__(self, n):
        self.n, self.shape = int(n), (int(n),)


def space(dist, K):
    return Discrete(K) if dist == CATEGORICAL else MultiBinary(K)


def param_shapes(O, K, H, Hc=None):
    """The reference's state_dict order of Policy on Discrete(K) / MultiBinary(K): a2c/model.py:233-253, then dist.linear"""
    Hc = Hc or H
    return [("base.actor.0.weight", (H, O)), ("base.actor.0.bias", (H,)), ("base.actor.2.weight", (H, H)), ("base.actor.2.bias", (H,)),
            ("base.critic.0.weight", (Hc, O)), ("base.critic.0.bias", (Hc,)), ("base.critic.2.weight", (Hc, Hc)), ("base.critic.2.bias", (Hc,)),
            ("base.critic_linear.weight", (1, Hc)), ("base.critic_linear.bias", (1,)),
            ("dist.linear.weight", (K, H)), ("dist.linear.bias", (K,))]


def blocks(shapes):
    """[(name, slice of the flat vector)]"""
    out, off = [], 0
    for name, shape in shapes:
        n = int(np.prod(shape))
        out.append((name, slice(off, off + n)))
        off += n
    return out


def block_distances(got, want, shapes):
    """{block: max |got - want| / max(1e-30, max |want| over the block)}: the per-parameter-block relative distance"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return {name: float(np.max(np.abs(got[sl] - want[sl])) / max(1e-30, float(np.max(np.abs(want[sl]))))) for name, sl in blocks(shapes)}


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(bytes(g["meta"]).decode())
    return g


# ------------------------------------------------------------------------------------------- the forward, in any dtype
def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float64)), dtype=dtype)


def _leaves(flat, shapes, dtype):
    if dtype == ar.F64:
        return ar.leaves(flat, shapes)
    flat = np.asarray(flat, np.float64).reshape(-1)
    out, off = {}, 0
    for name, shape in shapes:
        n = int(np.prod(shape))
        out[name] = _t(flat[off:off + n].reshape(shape), dtype).requires_grad_(True)
        off += n
    return out


def forward(dist, p, x):
    """-> (values [rows], logits [rows, K])"""
    value = ar.linear(p, "base.critic_linear", ar.trunk(p, "base.critic", x))
    return value[:, 0], ar.linear(p, "dist.linear", ar.trunk(p, "base.actor", x))


def softplus(z):
    """log(1 + e^z) without torch.nn.functional.softplus's threshold (which returns z itself above 20)"""
    return torch.logaddexp(z, torch.zeros_like(z))


def log_probs(dist, z, actions, fault=None):
    """FixedCategorical.log_probs / FixedBernoulli.log_probs (a2c/distributions.py:37-44,64-65) -> [rows].  actions: [rows, 1]
    class indices, or [rows, K] bits."""
    if dist == CATEGORICAL:
        idx = torch.as_tensor(np.asarray(actions).reshape(-1).astype(np.int64))
        if fault == "index_off_by_one":
            idx = (idx + 1) % z.shape[1]
        lp = z - torch.logsumexp(z, dim=-1, keepdim=True)
        return lp.gather(1, idx.view(-1, 1))[:, 0]
    a = _t(actions, z.dtype).reshape(z.shape)
    return (a * z - softplus(z)).sum(-1)


def entropy_rows(dist, z):
    """dist.entropy() per row (a2c/distributions.py:67-68; torch's Categorical.entropy)"""
    if dist == CATEGORICAL:
        lp = z - torch.logsumexp(z, dim=-1, keepdim=True)
        return -(lp.exp() * lp).sum(-1)
    return (softplus(z) - torch.sigmoid(z) * z).sum(-1)


def _faulty_logp(dist, z, actions, fault):
    """`p_for_a_minus_p`: a log-prob whose gradient in the logits is +p instead of a - p (its value is irrelevant to the test)"""
    if fault == "p_for_a_minus_p":
        if dist == CATEGORICAL:
            return torch.logsumexp(z, dim=-1)
        return softplus(z).sum(-1)
    return log_probs(dist, z, actions, fault)


def evaluate(dist, shapes, params, obs, actions, dtype=ar.F64):
    """Policy.evaluate_actions (a2c/model.py:107-114) -> (values [rows], logp [rows], entropy rows [rows]) as numpy float64"""
    p = _leaves(params, shapes, dtype)
    with torch.no_grad():
        v, z = forward(dist, p, _t(obs, dtype))
        return (v.double().numpy(), log_probs(dist, z, actions).double().numpy(), entropy_rows(dist, z).double().numpy(),
                z.double().numpy())


def ppo_grad(dist, shapes, params, obs, actions, old_logp, value_preds, returns, clip=CLIP, vcoef=VCOEF, ecoef=ECOEF, use_clipped=True,
             adv=None, dtype=ar.F64, fault=None):
    """One minibatch of all rows -> (flat gradient, losses[3]).  adv None: the normalised advantages of a2c/algo/ppo.py:66-68."""
    p = _leaves(params, shapes, dtype)
    values, z = forward(dist, p, _t(obs, dtype))
    logp = _faulty_logp(dist, z, actions, fault)
    ent = entropy_rows(dist, z).mean()
    if fault == "no_entropy_gradient":
        ent = ent.detach()
    a = ar.normalised_advantages(returns, value_preds).to(dtype) if adv is None else _t(adv, dtype)
    total, parts = ar.ppo_loss(values, logp, ent, _t(old_logp, dtype), a, _t(value_preds, dtype), _t(returns, dtype), clip, vcoef, ecoef,
                               use_clipped)
    gs = torch.autograd.grad(total, list(p.values()), allow_unused=True)
    flat = np.concatenate([(torch.zeros_like(x) if g is None else g).reshape(-1).double().numpy() for g, x in zip(gs, p.values())])
    return flat, ar.terms(*parts)


def a2c_grad(dist, shapes, params, obs, actions, returns, vcoef=VCOEF, ecoef=ECOEF, dtype=ar.F64, fault=None):
    """a2c/algo/a2c_acktr.py:56-91 (acktr=False) over all rows -> (flat gradient, (value_loss, action_loss, entropy))"""
    p = _leaves(params, shapes, dtype)
    values, z = forward(dist, p, _t(obs, dtype))
    logp = _faulty_logp(dist, z, actions, fault)
    ent = entropy_rows(dist, z).mean()
    if fault == "no_entropy_gradient":
        ent = ent.detach()
    adv = _t(returns, dtype) - values
    value_loss = adv.pow(2).mean()
    action_loss = -(adv.detach() * logp).mean()
    total = value_loss * vcoef + action_loss - ent * ecoef
    gs = torch.autograd.grad(total, list(p.values()), allow_unused=True)
    flat = np.concatenate([(torch.zeros_like(x) if g is None else g).reshape(-1).double().numpy() for g, x in zip(gs, p.values())])
    return flat, ar.terms(value_loss, action_loss, ent)


# ------------------------------------------------------------------------------------------- the samplers, in numpy
def probs32(dist, logits):
    """The float32 probabilities the head kernels sample from: softmax with the row maximum subtracted and the normaliser taken as
    log1p of the other classes' mass / the sigmoid from exp(-|z|) -- float32 throughout, as csrc/sg_policy.hip forms them."""
    z = np.asarray(logits, np.float32)
    if dist == CATEGORICAL:
        am = np.argmax(z, axis=1)
        m = z[np.arange(z.shape[0]), am][:, None]
        e = np.exp((z - m).astype(np.float32)).astype(np.float32)
        S = np.zeros(z.shape[0], np.float32)
        for k in range(z.shape[1]):   # ascending k, float32 running sum, the argmax left out
            S = np.where(am == k, S, (S + e[:, k]).astype(np.float32)).astype(np.float32)
        l1p = np.log1p(S).astype(np.float32)[:, None]
        return np.exp(((z - m).astype(np.float32) - l1p).astype(np.float32)).astype(np.float32)
    e = np.exp(-np.abs(z)).astype(np.float32)
    one = np.float32(1.0)
    return np.where(z >= 0, one / (one + e), e / (one + e)).astype(np.float32)


def sample(dist, logits, u):
    """Categorical: the first k whose float32 running sum of p over ascending k exceeds u, clamped to K - 1 -> int64 [rows, 1].
    Bernoulli: u_k < p_k -> float32 0/1 [rows, K]."""
    p = probs32(dist, logits)
    u = np.asarray(u, np.float32).reshape(p.shape[0], -1)
    if dist == CATEGORICAL:
        cdf = np.zeros_like(p)
        run = np.zeros(p.shape[0], np.float32)
        for k in range(p.shape[1]):
            run = (run + p[:, k]).astype(np.float32)
            cdf[:, k] = run
        over = cdf > u
        return np.where(over.any(1), over.argmax(1), p.shape[1] - 1).astype(np.int64).reshape(-1, 1)
    return (u < p).astype(np.float32)


def sample_margin(dist, logits, u):
    """min |u - boundary| over rows: the boundaries are the CDF values (categorical) or p_k (Bernoulli), in float64"""
    p = probs32(dist, logits).astype(np.float64)
    u = np.asarray(u, np.float64).reshape(p.shape[0], -1)
    return float(np.min(np.abs(u - (np.cumsum(p, axis=1) if dist == CATEGORICAL else p))))


# ------------------------------------------------------------------------------------------- cases of the gradient checks
# (O, K, H) of the issue's shapes; minibatch rows 16 / 77 / 128: one 16-row group exactly, an odd count over several groups
# with a ragged tail, a whole number of 32-row groups
SHAPES = {CATEGORICAL: ((4, 2, 16), (11, 17, 64), (20, 130, 32)), BERNOULLI: ((4, 1, 16), (11, 5, 64), (20, 33, 32))}
ROWS = (16, 77, 128)


def init_params(shapes, seed, scale=0.4, head_scale=1.0):
    rng = np.random.default_rng(seed)
    parts = []
    for name, shape in shapes:
        s = head_scale if name.startswith("dist.") else scale
        parts.append((rng.standard_normal(shape) * s / np.sqrt(shape[-1] if len(shape) > 1 else 1.0)).astype(np.float32).reshape(-1)
                     if name.endswith("weight") else (0.1 * rng.standard_normal(shape)).astype(np.float32).reshape(-1))
    return np.concatenate(parts)


def make_case(dist, O, K, H, rows, seed, saturated=False):
    """A one-minibatch PPO / A2C case off the on-policy regime: actions drawn from the behaviour policy, the policy then
    perturbed so that ratio != 1, advantages of both signs -- rows in all three branches of the clipped surrogate (clipped low,
    inside, clipped high; asserted by `surrogate_branches`), none within 1e-4 of a boundary: rows that land nearer have their
    behaviour log-prob moved until they do not.  saturated: logit gaps of about 15 (head weights scaled up)."""
    shapes = param_shapes(O, K, H)
    rng = np.random.default_rng(seed)
    behaviour = init_params(shapes, seed + 1, head_scale=1.5)
    obs = rng.standard_normal((rows, O)).astype(np.float32)
    _, _, _, z = evaluate(dist, shapes, behaviour, obs, np.zeros((rows, 1 if dist == CATEGORICAL else K)))
    if saturated:   # scale dist.linear until the median gap (top two logits / a logit and 0) is 15
        gap = np.median(np.sort(z, 1)[:, -1] - np.sort(z, 1)[:, -2]) if dist == CATEGORICAL else np.median(np.abs(z))
        head = blocks(shapes)[-2][1].start
        behaviour[head:] *= np.float32(15.0 / gap)
        _, _, _, z = evaluate(dist, shapes, behaviour, obs, np.zeros((rows, 1 if dist == CATEGORICAL else K)))
    u = rng.random((rows, 1 if dist == CATEGORICAL else K)).astype(np.float32)
    actions = sample(dist, z, u)
    if saturated:   # near-certain actions are the regime; a few rows take another class so that adv * (a - p) is not all ~0
        if dist == CATEGORICAL:
            actions[::5, 0] = rng.integers(0, K, size=actions[::5].shape[0])
        else:
            actions[::5] = 1.0 - actions[::5]
    # (saturated: an absolute perturbation -- one relative to the scaled-up head would move the trunks, and the gaps, too far)
    params = (behaviour + rng.standard_normal(behaviour.shape).astype(np.float32) *
              (0.003 if saturated else 0.08 * np.abs(behaviour).mean())).astype(np.float32)
    _, logp_b, _, _ = evaluate(dist, shapes, behaviour, obs, actions)
    v, logp, _, _ = evaluate(dist, shapes, params, obs, actions)
    old_logp = logp_b.astype(np.float32)
    # spread the ratios over all three branches: every third row is pushed below 1 - clip, every third above 1 + clip
    shift = np.zeros(rows)
    shift[0::3] = np.log(1.0 - CLIP) - 0.12
    shift[1::3] = np.log(1.0 + CLIP) + 0.12
    old_logp = (logp - (np.where(shift != 0, shift, logp - old_logp))).astype(np.float32)
    ratio = np.exp(logp - old_logp.astype(np.float64))
    for edge in (1.0 - CLIP, 1.0 + CLIP):   # nobody within 1e-4 of a clip boundary
        near = np.abs(ratio - edge) < 2e-4
        old_logp[near] -= np.float32(0.01)
    value_preds = (v + 0.3 * rng.standard_normal(rows)).astype(np.float32)
    returns = (v + rng.standard_normal(rows)).astype(np.float32)
    return dict(dist=dist, O=O, K=K, H=H, rows=rows, shapes=shapes, params=params, obs=obs, actions=actions, old_logp=old_logp,
                value_preds=value_preds, returns=returns)


def surrogate_branches(case):
    """-> (rows clipped low, rows inside, rows clipped high, smallest distance of a ratio from a clip boundary), float64"""
    _, logp, _, _ = evaluate(case["dist"], case["shapes"], case["params"], case["obs"], case["actions"])
    ratio = np.exp(logp - case["old_logp"].astype(np.float64))
    lo, hi = 1.0 - CLIP, 1.0 + CLIP
    return (int((ratio < lo).sum()), int(((ratio >= lo) & (ratio <= hi)).sum()), int((ratio > hi).sum()),
            float(min(np.abs(ratio - lo).min(), np.abs(ratio - hi).min())))
