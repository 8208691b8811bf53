"""Float64 numpy restatement of the recurrent Policy's forward (a2c/model.py:117-201, 233-264 with recurrent=True;
a2c/distributions.py:51-59, 91-118): nn.GRU (gates r, z, n) stepped with h <- h * masks[t], then the actor / critic
trunks on the GRU state, critic_linear and the diagonal Gaussian.  Independent of the HIP code; pinned against the
reference-written fixtures by tests/test_recurrent_host.py and used by the GPU tests for shapes that have no fixture."""
import os

import numpy as np

# The reference's float32 constants at their float32 VALUE, as in every float64 arbiter (the convention is stated once, in
# tests/autograd_ref.py): torch subtracts the double log(sqrt(2 pi)) from a float32 tensor, PPO.update adds 1e-5 to a float32 std.
HALF_LOG_2PI = float(np.float32(0.5 * np.log(2.0 * np.pi)))
ADV_EPS = float(np.float32(1e-5))


def param_shapes(O, A, H, Hc=None):
    Hc = Hc or H
    return [("base.gru.weight_ih_l0", (3 * H, O)), ("base.gru.weight_hh_l0", (3 * H, H)),
            ("base.gru.bias_ih_l0", (3 * H,)), ("base.gru.bias_hh_l0", (3 * H,)),
            ("base.actor.0.weight", (H, H)), ("base.actor.0.bias", (H,)),
            ("base.actor.2.weight", (H, H)), ("base.actor.2.bias", (H,)),
            ("base.critic.0.weight", (Hc, H)), ("base.critic.0.bias", (Hc,)),
            ("base.critic.2.weight", (Hc, Hc)), ("base.critic.2.bias", (Hc,)),
            ("base.critic_linear.weight", (1, Hc)), ("base.critic_linear.bias", (1,)),
            ("dist.fc_mean.weight", (A, H)), ("dist.fc_mean.bias", (A,)),
            ("dist.logstd._bias", (A, 1))]


def unflatten(flat, O, A, H, Hc=None, dtype=np.float64):
    out, off = {}, 0
    flat = np.asarray(flat, dtype).reshape(-1)
    for name, shape in param_shapes(O, A, H, Hc):
        n = int(np.prod(shape))
        out[name] = flat[off:off + n].reshape(shape)
        off += n
    assert off == flat.size, (off, flat.size)
    return out


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def gru_cell(sd, x, h):
    H = h.shape[1]
    gi = x @ sd["base.gru.weight_ih_l0"].T + sd["base.gru.bias_ih_l0"]
    gh = h @ sd["base.gru.weight_hh_l0"].T + sd["base.gru.bias_hh_l0"]
    r = _sigmoid(gi[:, :H] + gh[:, :H])
    z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1.0 - z) * n + z * h


def gru_sequence(sd, obs, hxs, masks):
    """obs [T*n, O] time-major, hxs [n, H], masks [T*n] -> (h_t stacked [T*n, H], last state [n, H])."""
    obs, h = np.asarray(obs, np.float64), np.asarray(hxs, np.float64)
    masks = np.asarray(masks, np.float64).reshape(-1)
    n = h.shape[0]
    T = obs.shape[0] // n
    assert T * n == obs.shape[0] == masks.size
    out = []
    for t in range(T):
        h = gru_cell(sd, obs[t * n:(t + 1) * n], h * masks[t * n:(t + 1) * n, None])
        out.append(h)
    return np.concatenate(out), h


def heads(sd, x):
    """-> (value [rows, 1], mean [rows, A], logstd [A])"""
    a = np.tanh(np.tanh(x @ sd["base.actor.0.weight"].T + sd["base.actor.0.bias"]) @ sd["base.actor.2.weight"].T + sd["base.actor.2.bias"])
    c = np.tanh(np.tanh(x @ sd["base.critic.0.weight"].T + sd["base.critic.0.bias"]) @ sd["base.critic.2.weight"].T + sd["base.critic.2.bias"])
    value = c @ sd["base.critic_linear.weight"].T + sd["base.critic_linear.bias"]
    mean = a @ sd["dist.fc_mean.weight"].T + sd["dist.fc_mean.bias"]
    return value, mean, sd["dist.logstd._bias"].reshape(-1)


def log_prob(mean, logstd, action):
    std = np.exp(logstd)
    lp = -((action - mean) ** 2) / (2.0 * std * std) - logstd - HALF_LOG_2PI
    return lp.sum(-1, keepdims=True)


def evaluate(sd, obs, hxs, masks, action):
    """Policy.evaluate_actions -> (value [rows, 1], logp [rows, 1], entropy scalar, hxs_out [n, H])"""
    x, h_last = gru_sequence(sd, obs, hxs, masks)
    value, mean, logstd = heads(sd, x)
    ent = float(np.sum(0.5 + HALF_LOG_2PI + logstd))
    return value, log_prob(mean, logstd, np.asarray(action, np.float64)), ent, h_last


def act(sd, obs, hxs, masks, noise=None):
    """Policy.act (noise None: deterministic) -> (value, action, logp, hxs_out)"""
    x, h_last = gru_sequence(sd, obs, hxs, masks)
    value, mean, logstd = heads(sd, x)
    action = mean if noise is None else mean + np.exp(logstd) * np.asarray(noise, np.float64)
    return value, action, log_prob(mean, logstd, action), h_last


# ------------------------------------------------------------------------------------------- one whole PPO update
# a2c/algo/ppo.py:65-157 with actor_critic.is_recurrent over a2c/storage.py:194-251, float64: loss, back-propagation through the
# heads and through time, clip_grad_norm_ over all parameters, torch.optim.Adam (single-tensor form).

def flatten(d, O, A, H, Hc=None):
    return np.concatenate([np.asarray(d[name], np.float64).reshape(-1) for name, _ in param_shapes(O, A, H, Hc)])


def _trunk_fwd(sd, pre, x):
    h1 = np.tanh(x @ sd[pre + ".0.weight"].T + sd[pre + ".0.bias"])
    h2 = np.tanh(h1 @ sd[pre + ".2.weight"].T + sd[pre + ".2.bias"])
    return h1, h2


def _trunk_bwd(sd, pre, x, h1, h2, dh2, g):
    d2 = dh2 * (1.0 - h2 * h2)
    g[pre + ".2.weight"] = d2.T @ h1
    g[pre + ".2.bias"] = d2.sum(0)
    d1 = (d2 @ sd[pre + ".2.weight"]) * (1.0 - h1 * h1)
    g[pre + ".0.weight"] = d1.T @ x
    g[pre + ".0.bias"] = d1.sum(0)
    return d1 @ sd[pre + ".0.weight"]


def minibatch_grad(sd, obs, hxs, masks, action, old_logp, adv, vpred, ret, clip, vcoef, ecoef, use_clipped=True, dtype=np.float64):
    """obs [T*n, O] time-major ... -> (gradient dict, (value_loss, action_loss, entropy)).  dtype=np.float32 (with sd
    unflattened at float32) carries every array in float32: the same algorithm at the library's precision, for tests that
    measure the library's distance from float64 against a float32 evaluation's own."""
    f = dtype
    half_log_2pi = f(HALF_LOG_2PI)  # (a float32 scalar must not promote the arrays)
    clip, vcoef, ecoef = f(clip), f(vcoef), f(ecoef)
    obs, h = np.asarray(obs, f), np.asarray(hxs, f)
    masks = np.asarray(masks, f).reshape(-1)
    n, H = h.shape
    T = obs.shape[0] // n
    B = T * n
    Wih, Whh = sd["base.gru.weight_ih_l0"], sd["base.gru.weight_hh_l0"]
    bih, bhh = sd["base.gru.bias_ih_l0"], sd["base.gru.bias_hh_l0"]
    saved, xs = [], []
    for t in range(T):
        sl = slice(t * n, (t + 1) * n)
        hm = h * masks[sl, None]
        gi = obs[sl] @ Wih.T + bih
        gh = hm @ Whh.T + bhh
        r = _sigmoid(gi[:, :H] + gh[:, :H])
        z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        hn = gh[:, 2 * H:]
        nn = np.tanh(gi[:, 2 * H:] + r * hn)
        h = (1.0 - z) * nn + z * hm
        saved.append((r, z, nn, hn, hm))
        xs.append(h)
    x = np.concatenate(xs)
    a1, a2 = _trunk_fwd(sd, "base.actor", x)
    c1, c2 = _trunk_fwd(sd, "base.critic", x)
    value = (c2 @ sd["base.critic_linear.weight"].T + sd["base.critic_linear.bias"])[:, 0]
    mean = a2 @ sd["dist.fc_mean.weight"].T + sd["dist.fc_mean.bias"]
    logstd = sd["dist.logstd._bias"].reshape(-1)
    var = np.exp(2.0 * logstd)
    action = np.asarray(action, f)
    diff = action - mean
    logp = (-(diff * diff) / (2.0 * var) - logstd - half_log_2pi).sum(-1)
    ent = float(np.sum(0.5 + half_log_2pi + logstd))
    old_logp, adv, vpred, ret = (np.asarray(q, f).reshape(-1) for q in (old_logp, adv, vpred, ret))
    ratio = np.exp(logp - old_logp)
    s1, s2 = ratio * adv, np.clip(ratio, f(1.0) - clip, f(1.0) + clip) * adv
    action_loss = -np.minimum(s1, s2).mean()
    inside = ((ratio >= f(1.0) - clip) & (ratio <= f(1.0) + clip)).astype(f)
    dlogp = -(np.where(s1 <= s2, adv, adv * inside) * ratio) / B
    if use_clipped:
        vc = vpred + np.clip(value - vpred, -clip, clip)
        u, w = (value - ret) ** 2, (vc - ret) ** 2
        value_loss = 0.5 * np.maximum(u, w).mean()
        vin = (np.abs(value - vpred) <= clip).astype(f)
        dv = vcoef * 0.5 * np.where(u >= w, 2.0 * (value - ret), 2.0 * (vc - ret) * vin) / B
    else:
        value_loss = 0.5 * ((ret - value) ** 2).mean()
        dv = vcoef * (value - ret) / B
    g = {}
    dmean = dlogp[:, None] * diff / var
    g["dist.logstd._bias"] = ((dlogp[:, None] * (diff * diff / var - 1.0)).sum(0) - ecoef).reshape(-1, 1)
    g["dist.fc_mean.weight"] = dmean.T @ a2
    g["dist.fc_mean.bias"] = dmean.sum(0)
    g["base.critic_linear.weight"] = dv[None, :] @ c2
    g["base.critic_linear.bias"] = np.array([dv.sum()], f)
    dx = _trunk_bwd(sd, "base.actor", x, a1, a2, dmean @ sd["dist.fc_mean.weight"], g)
    dx = dx + _trunk_bwd(sd, "base.critic", x, c1, c2, dv[:, None] * sd["base.critic_linear.weight"], g)
    gWih, gWhh, gbih, gbhh = np.zeros_like(Wih), np.zeros_like(Whh), np.zeros_like(bih), np.zeros_like(bhh)
    carry = np.zeros((n, H), f)
    for t in range(T - 1, -1, -1):
        sl = slice(t * n, (t + 1) * n)
        r, z, nn, hn, hm = saved[t]
        dh = dx[sl] + carry
        dn = dh * (1.0 - z) * (1.0 - nn * nn)
        dz = dh * (hm - nn) * z * (1.0 - z)
        dr = dn * hn * r * (1.0 - r)
        dgi = np.concatenate([dr, dz, dn], 1)
        dgh = np.concatenate([dr, dz, dn * r], 1)
        gWih += dgi.T @ obs[sl]
        gWhh += dgh.T @ hm
        gbih += dgi.sum(0)
        gbhh += dgh.sum(0)
        carry = (dh * z + dgh @ Whh) * masks[sl, None]
    g["base.gru.weight_ih_l0"], g["base.gru.weight_hh_l0"], g["base.gru.bias_ih_l0"], g["base.gru.bias_hh_l0"] = gWih, gWhh, gbih, gbhh
    return g, (float(value_loss), float(action_loss), ent)


def ppo_update(flat0, O, A, H, ro, hxs0, perms, ppo_epoch, num_mini_batch, clip, vcoef, ecoef, lr, eps, max_grad_norm, Hc=None,
               adam=None, use_clipped=True):
    """ro: dict of the rollout's arrays (obs [T+1,N,O], actions, value_preds, returns, action_log_probs, masks); hxs0 [N, H];
    perms [ppo_epoch, N] -> dict(params, losses, adam_m, adam_v, steps, advantages, norms: every step's gradient norm before the clip)"""
    p = np.asarray(flat0, np.float64).copy()
    obs, act = np.asarray(ro["obs"], np.float64), np.asarray(ro["actions"], np.float64)
    vp, ret = np.asarray(ro["value_preds"], np.float64)[..., 0], np.asarray(ro["returns"], np.float64)[..., 0]
    olp, mk = np.asarray(ro["action_log_probs"], np.float64)[..., 0], np.asarray(ro["masks"], np.float64)[..., 0]
    T, N = act.shape[:2]
    adv = ret[:-1] - vp[:-1]
    adv = (adv - adv.mean()) / (adv.std(ddof=1) + ADV_EPS)
    per = N // num_mini_batch
    assert N % per == 0
    m, v, step = (np.zeros_like(p), np.zeros_like(p), 0) if adam is None else (np.asarray(adam[0], np.float64).copy(),
                                                                                 np.asarray(adam[1], np.float64).copy(), int(adam[2]))
    sums, norms = np.zeros(3), []
    for e in range(ppo_epoch):
        for start in range(0, N, per):
            envs = np.asarray(perms[e][start:start + per])
            tm = lambda a: a[:, envs].reshape(T * per, *a.shape[2:])  # noqa: E731
            sd = unflatten(p, O, A, H, Hc)
            g, losses = minibatch_grad(sd, tm(obs[:-1]), np.asarray(hxs0, np.float64)[envs], tm(mk[:-1]), tm(act), tm(olp), tm(adv),
                                       tm(vp[:-1]), tm(ret[:-1]), clip, vcoef, ecoef, use_clipped)
            gf = flatten(g, O, A, H, Hc)
            norms.append(float(np.sqrt((gf * gf).sum())))
            gf = gf * min(1.0, max_grad_norm / (norms[-1] + 1e-6))
            step += 1
            m = 0.9 * m + 0.1 * gf
            v = 0.999 * v + 0.001 * gf * gf
            p = p - (lr / (1.0 - 0.9 ** step)) * m / (np.sqrt(v) / np.sqrt(1.0 - 0.999 ** step) + eps)
            sums += losses
    return dict(params=p, losses=sums / (ppo_epoch * num_mini_batch), adam_m=m, adam_v=v, steps=step, advantages=adv[..., None], norms=norms)


def load_ppo(name):
    """An update fixture: <name>.npz, plus <name>_params1 / _adam_m / _adam_v .npz where the generator wrote those arrays to files
    of their own (the hidden-64 cases, to keep every file under 300 KB)."""
    from helpers import GOLDEN, load
    g = load(name)
    for key in ("params1", "adam_m", "adam_v"):
        if key not in g:
            g[key] = np.load(os.path.join(GOLDEN, f"{name}_{key}.npz"))[key]
    return g
