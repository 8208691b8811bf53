"""Float64 numpy restatement of ONE A2C update on a recurrent Policy: a2c/algo/a2c_acktr.py:55-102 (acktr=False) over
a2c/model.py:117-201 -- evaluate_actions on the rollout's T*N rows in their own order with the GRU stepped h <- h * masks[t] from
the state of slot 0, adv = returns[:-1] - values, value_loss = mean(adv^2), action_loss = -mean(adv.detach() logp), loss =
vcoef value_loss + action_loss - ecoef entropy, back-propagation through the heads and through time, clip_grad_norm_ over ALL
parameters, one RMSprop step in torch's form (square_avg from 0).  Built on tests/gru_ref.py's cell, trunks and layout.

`autograd_grad` is the independent arbiter: the same loss written forward-only in torch.float64 through the real torch.nn.GRU
(tests/autograd_ref.py's policy_forward) and differentiated by autograd; the float32 constants stay at their float32 value.

`wrong=` injects the four faults the tests must be able to see (the test of the test): "no_mask", "group_mean" (with group_envs),
"clip_without_gru", "half_value"."""
import numpy as np

import gru_ref

RTOL_BLOCK = 1e-4    # a block of the library's gradient against float64, relative to the block's largest magnitude
N_GRU = 4            # the GRU's tensors lead param_shapes()


def gru_count(O, A, H):
    return sum(int(np.prod(s)) for _, s in gru_ref.param_shapes(O, A, H)[:N_GRU])


def _grad_rows(sd, obs, hxs, masks, action, ret, vcoef, ecoef, B, f, mask_h=True, half_value=False):
    """The gradient of the rows given (n environments, time-major, all T steps) with every mean taken over B rows ->
    (gradient dict, (sum adv^2, sum -adv logp, entropy)).  f = np.float32 carries every array in float32."""
    half_log_2pi = f(gru_ref.HALF_LOG_2PI)
    vcoef, ecoef, B = f(vcoef), f(ecoef), f(B)
    obs, h = np.asarray(obs, f), np.asarray(hxs, f)
    masks = np.asarray(masks, f).reshape(-1)
    n, H = h.shape
    T = obs.shape[0] // n
    Wih, Whh = sd["base.gru.weight_ih_l0"], sd["base.gru.weight_hh_l0"]
    bih, bhh = sd["base.gru.bias_ih_l0"], sd["base.gru.bias_hh_l0"]
    one = f(1.0)
    saved, xs = [], []
    for t in range(T):
        sl = slice(t * n, (t + 1) * n)
        mk = masks[sl, None] if mask_h else np.ones((n, 1), f)
        hm = h * mk
        gi = obs[sl] @ Wih.T + bih
        gh = hm @ Whh.T + bhh
        r = gru_ref._sigmoid(gi[:, :H] + gh[:, :H]).astype(f)
        z = gru_ref._sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H]).astype(f)
        hn = gh[:, 2 * H:]
        nn = np.tanh(gi[:, 2 * H:] + r * hn)
        h = (one - z) * nn + z * hm
        saved.append((r, z, nn, hn, hm, mk))
        xs.append(h)
    x = np.concatenate(xs)
    a1, a2 = gru_ref._trunk_fwd(sd, "base.actor", x)
    c1, c2 = gru_ref._trunk_fwd(sd, "base.critic", x)
    value = (c2 @ sd["base.critic_linear.weight"].T + sd["base.critic_linear.bias"])[:, 0]
    mean = a2 @ sd["dist.fc_mean.weight"].T + sd["dist.fc_mean.bias"]
    logstd = sd["dist.logstd._bias"].reshape(-1)
    var = np.exp(f(2.0) * logstd)
    diff = np.asarray(action, f) - mean
    logp = (-(diff * diff) / (f(2.0) * var) - logstd - half_log_2pi).sum(-1)
    ent = float(np.sum(f(0.5) + half_log_2pi + logstd))
    adv = np.asarray(ret, f).reshape(-1) - value
    vscale = f(0.5) if half_value else one     # (the fault: PPO's 0.5 (R - v)^2)
    sums = (float(vscale * (adv * adv).sum()), float(-(adv * logp).sum()), ent)
    dlogp = -adv / B
    dv = vcoef * vscale * f(2.0) * (value - np.asarray(ret, f).reshape(-1)) / B
    rows = f(obs.shape[0])
    g = {}
    dmean = dlogp[:, None] * diff / var
    # the entropy term is a mean over rows of a row-independent number: these rows' share of it is rows / B
    g["dist.logstd._bias"] = ((dlogp[:, None] * (diff * diff / var - one)).sum(0) - ecoef * rows / B).reshape(-1, 1)
    g["dist.fc_mean.weight"] = dmean.T @ a2
    g["dist.fc_mean.bias"] = dmean.sum(0)
    g["base.critic_linear.weight"] = dv[None, :] @ c2
    g["base.critic_linear.bias"] = np.array([dv.sum()], f)
    dx = gru_ref._trunk_bwd(sd, "base.actor", x, a1, a2, dmean @ sd["dist.fc_mean.weight"], g)
    dx = dx + gru_ref._trunk_bwd(sd, "base.critic", x, c1, c2, dv[:, None] * sd["base.critic_linear.weight"], g)
    gWih, gWhh, gbih, gbhh = np.zeros_like(Wih), np.zeros_like(Whh), np.zeros_like(bih), np.zeros_like(bhh)
    carry = np.zeros((n, H), f)
    for t in range(T - 1, -1, -1):     # no gradient is formed for h_0 or the observations
        sl = slice(t * n, (t + 1) * n)
        r, z, nn, hn, hm, mk = saved[t]
        dh = dx[sl] + carry
        dn = dh * (one - z) * (one - nn * nn)
        dz = dh * (hm - nn) * z * (one - z)
        dr = dn * hn * r * (one - r)
        dgi = np.concatenate([dr, dz, dn], 1)
        dgh = np.concatenate([dr, dz, dn * r], 1)
        gWih += dgi.T @ obs[sl]
        gWhh += dgh.T @ hm
        gbih += dgi.sum(0)
        gbhh += dgh.sum(0)
        carry = (dh * z + dgh @ Whh) * mk
    g["base.gru.weight_ih_l0"], g["base.gru.weight_hh_l0"], g["base.gru.bias_ih_l0"], g["base.gru.bias_hh_l0"] = gWih, gWhh, gbih, gbhh
    return g, sums


def _rows(ro, hxs0, envs):
    """the time-major rows of the environments `envs`: obs[:-1], masks[:-1], actions, returns[:-1]"""
    T = np.asarray(ro["actions"]).shape[0]
    tm = lambda a: np.asarray(a)[:T][:, envs].reshape(T * len(envs), *np.asarray(a).shape[2:])  # noqa: E731
    return tm(ro["obs"]), np.asarray(hxs0)[envs], tm(ro["masks"])[:, 0], tm(ro["actions"]), tm(ro["returns"])[:, 0]


def grad(flat, O, A, H, ro, hxs0, vcoef, ecoef, dtype=np.float64, group_envs=None, wrong=None):
    """-> (flat gradient in param_shapes order, losses (value_loss, action_loss, entropy)).  group_envs: the environments go
    through in groups of that many, each group's gradient added to the sum -- the same number, whatever the group size, as long
    as every mean is over the WHOLE rollout's T*N rows (wrong="group_mean": over the group's)."""
    f = dtype
    T, N = np.asarray(ro["actions"]).shape[:2]
    sd = gru_ref.unflatten(flat, O, A, H, dtype=f)
    ng = N if group_envs is None else int(group_envs)
    total, sums = None, np.zeros(3)
    for e0 in range(0, N, ng):
        envs = np.arange(e0, min(N, e0 + ng))
        B = T * len(envs) if wrong == "group_mean" else T * N
        g, s = _grad_rows(sd, *_rows(ro, hxs0, envs), vcoef, ecoef, B, f, mask_h=wrong != "no_mask", half_value=wrong == "half_value")
        gf = np.concatenate([np.asarray(g[name], f).reshape(-1) for name, _ in gru_ref.param_shapes(O, A, H)])
        total = gf if total is None else total + gf
        sums[:2] += np.array(s[:2]) / B
        sums[2] = s[2]
    return total, sums


def update(flat0, O, A, H, ro, hxs0, vcoef, ecoef, lr, eps, alpha, max_grad_norm, square_avg=None, group_envs=None, wrong=None):
    """One update in float64 -> dict(params, losses, square_avg, grad (before the clip), norm)."""
    p = np.asarray(flat0, np.float64).copy()
    g, losses = grad(p, O, A, H, ro, hxs0, vcoef, ecoef, np.float64, group_envs, wrong)
    clipped = g[gru_count(O, A, H):] if wrong == "clip_without_gru" else g
    norm = float(np.sqrt((clipped * clipped).sum()))
    gc = g * min(1.0, max_grad_norm / (norm + 1e-6))
    sq = np.zeros_like(p) if square_avg is None else np.asarray(square_avg, np.float64).copy()
    sq = alpha * sq + (1.0 - alpha) * gc * gc      # torch.optim.RMSprop: centered False, momentum 0, weight decay 0
    p = p - lr * gc / (np.sqrt(sq) + eps)
    return dict(params=p, losses=losses, square_avg=sq, grad=g, norm=norm)


def autograd_grad(flat, O, A, H, ro, hxs0, vcoef, ecoef):
    """The arbiter: a2c/algo/a2c_acktr.py:56-73, 92-94 forward-only in torch.float64 through torch.nn.GRU, differentiated by
    autograd -> (flat gradient, losses)."""
    import autograd_ref as ar
    T, N = np.asarray(ro["actions"]).shape[:2]
    obs, h0, masks, actions, ret = _rows(ro, hxs0, np.arange(N))
    p = ar.leaves(flat, gru_ref.param_shapes(O, A, H))
    values, mean, logstd = ar.policy_forward("gru", p, ar.t64(obs), h0, masks, T)
    logp = ar.normal_log_probs(mean, logstd, ar.t64(actions), ar.HALF_LOG_2PI)
    entropy = ar.normal_entropy(logstd, ar.HALF_LOG_2PI)
    advantages = ar.t64(ret) - values
    value_loss = advantages.pow(2).mean()
    action_loss = -(advantages.detach() * logp).mean()
    return ar.flat_grad(value_loss * vcoef + action_loss - entropy * ecoef, p), ar.terms(value_loss, action_loss, entropy)


def block_errors(got, ref, O, A, H):
    """{block: max|got - ref| / max|ref| over the block}: every parameter tensor, the GRU's gate by gate (regimes.blocks)"""
    import regimes
    ref = np.asarray(ref, np.float64)
    out = {}
    for (name, g), (_, r) in zip(regimes.blocks("gru", O, A, H, 1, np.asarray(got, np.float64)), regimes.blocks("gru", O, A, H, 1, ref)):
        out[name] = float(np.max(np.abs(g - r)) / (np.max(np.abs(r)) + 1e-300))
    return out


def random_case(O, A, H, T, N, seed=0, dead_env=None):
    """A rollout in the middle of training at a shape that has no fixture -> dict(params float32 flat, obs, actions, returns, masks,
    hxs0): zeros in masks (p = 0.08, slot 0 included), a non-zero state in slot 0, actions drawn around the policy's own means,
    returns around its values.  dead_env: that environment's masks are 0 at every step."""
    import regimes
    rng = np.random.default_rng([seed, O, A, H, T, N])
    c = dict(O=O, A=A, H=H, T=T, N=N)
    c["params"] = regimes._init_params(rng, "gru", O, A, H, 1, 1.0)
    c["obs"] = rng.standard_normal((T + 1, N, O)).astype(np.float32)
    masks = (rng.random((T + 1, N, 1)) > 0.08).astype(np.float32)
    masks[0, N // 2] = 0.0
    if dead_env is not None:
        masks[:, dead_env] = 0.0
    c["masks"] = masks
    c["hxs0"] = (0.5 * rng.standard_normal((N, H))).astype(np.float32)
    sd = gru_ref.unflatten(c["params"], O, A, H)
    v, _, _, _ = gru_ref.evaluate(sd, c["obs"][:-1].reshape(T * N, O), c["hxs0"], masks[:-1].reshape(-1), np.zeros((T * N, A)))
    x, _ = gru_ref.gru_sequence(sd, c["obs"][:-1].reshape(T * N, O), c["hxs0"], masks[:-1].reshape(-1))
    _, mean, ls = gru_ref.heads(sd, x)
    c["actions"] = (mean + np.exp(ls) * rng.standard_normal((T * N, A))).reshape(T, N, A).astype(np.float32)
    ret = np.zeros((T + 1, N, 1))
    ret[:T] = (v[:, 0] + 0.5 * rng.standard_normal(T * N)).reshape(T, N, 1)
    c["returns"] = ret.astype(np.float32)
    return c


def admitted(c, vcoef=0.5, ecoef=0.01):
    """-> (float64 gradient, losses, worst block error of the float32 mode).  A case may be used against the library only where
    the float32 evaluation of the same algorithm stays within HALF the bound of float64 in every block."""
    g64, l64 = grad(c["params"], c["O"], c["A"], c["H"], c, c["hxs0"], vcoef, ecoef)
    g32, _ = grad(c["params"], c["O"], c["A"], c["H"], c, c["hxs0"], vcoef, ecoef, dtype=np.float32)
    worst = max(block_errors(g32, g64, c["O"], c["A"], c["H"]).values())
    return g64, l64, worst


# (O, A, H, T, N) of the GPU gradient checks (tests/test_gpu_a2c_recurrent.py); the host file admits each of them
GPU_SHAPES = [(47, 12, 64, 8, 17), (13, 5, 100, 8, 17), (11, 3, 16, 1, 16), (13, 5, 20, 27, 48), (11, 3, 16, 130, 32), (13, 5, 20, 9, 33)]
DEAD_ENV_CASE = ((11, 3, 32, 8, 17), 5)    # environment 5 never leaves its reset
ANCHOR_SHAPE = (11, 3, 16, 5, 4)
