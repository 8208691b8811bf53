"""The independent arbiter of the float64 arbiters: the reference's losses written FORWARD-ONLY in torch.float64 and differentiated
by torch.autograd.  Every gradient check of the suite ends at a hand-derived float64 restatement (oracle/oracle64.py,
tests/gru_ref.py, test_a2c_host.a2c_loss_grad, acktr_regimes.update, test_symmetry_host.sym_loss_grad); the kernels were written
against those, so a derivation error shared by a kernel and its arbiter passes every test.  Nothing here is derived: no backward
pass is written down, the GRU is torch.nn.GRU itself, the K-FAC step is a dense linear solve without any eigenbasis.
tests/test_autograd_arbiter_host.py holds every restatement to this file on every case the GPU regimes files look at;
tests/test_gpu_autograd_anchor.py holds the HIP kernels to it directly, one smallest case per family.

Nothing here touches the library or the oracle.  Every dtype is passed explicitly (torch.set_default_dtype would leak into other
tests).  Gradients come back flat, in param_shapes() order, with the loss terms.

CONSTANTS -- the one convention of every float64 arbiter, stated here once: the reference's float32 constants at their float32
VALUE.  The reference computes in float32: torch's Normal.log_prob subtracts the Python double math.log(math.sqrt(2 pi)) from a
float32 tensor, PPO.update adds the double 1e-5 to a float32 std (a2c/algo/ppo.py:67-68), predict_reward adds 1e-7 to a float32
sigmoid -- in its arithmetic each of them is that double rounded to float32.  A float64 arbiter is "the same algorithm carried out
exactly", so it keeps those rounded values (oracle/sg_oracle_f64.c documents the same for its float literals); tests/gru_ref.py,
tests/regimes.py, test_a2c_host.py and tests/disc_regimes.py take the three numbers below in the same way.  The difference is not
academic: exp(-(c32 - c) A) moves every PPO ratio by 1.56e-8 per action dimension.  `EXACT` is for one use only: the reference's
own modules after .double() compute with the exact doubles (tier 2 of tests/test_autograd_arbiter_host.py)."""
import math

import numpy as np
import torch

F64 = torch.float64


def f32_value(x):
    """the double nearest to x that is a float32 number"""
    return float(np.float32(x))


HALF_LOG_2PI = f32_value(0.5 * math.log(2.0 * math.pi))    # torch/distributions/normal.py log_prob, entropy
ADV_EPS = f32_value(1e-5)                                  # a2c/algo/ppo.py:68
REWARD_EPS = f32_value(1e-7)                               # a2c/algo/gail.py predict_reward_combined
CONVENTION = dict(half_log_2pi=HALF_LOG_2PI, adv_eps=ADV_EPS)
EXACT = dict(half_log_2pi=0.5 * math.log(2.0 * math.pi), adv_eps=1e-5)


def t64(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float64)), dtype=F64)


def leaves(flat, shapes):
    """flat parameters -> {name: float64 leaf tensor} in `shapes` order"""
    flat = np.asarray(flat, np.float64).reshape(-1)
    out, off = {}, 0
    for name, shape in shapes:
        n = int(np.prod(shape))
        out[name] = t64(flat[off:off + n].reshape(shape)).requires_grad_(True)
        off += n
    assert off == flat.size, (off, flat.size)
    return out


def flat_grad(loss, p):
    """d loss / d p, flat in p's order; a parameter the loss does not reach has gradient exactly 0"""
    gs = torch.autograd.grad(loss, list(p.values()), allow_unused=True)
    return np.concatenate([(torch.zeros_like(x) if g is None else g).reshape(-1).numpy() for g, x in zip(gs, p.values())])


def terms(*xs):
    return np.array([float(x.detach()) for x in xs], np.float64)


def linear(p, name, x):
    return torch.nn.functional.linear(x, p[name + ".weight"], p[name + ".bias"])


def trunk(p, pre, x):
    """nn.Sequential(Linear, Tanh, Linear, Tanh): a2c/model.py:243-251"""
    return torch.tanh(linear(p, pre + ".2", torch.tanh(linear(p, pre + ".0", x))))


# ------------------------------------------------------------------------------------------- the diagonal Gaussian
def normal_log_probs(mean, logstd, action, half_log_2pi=HALF_LOG_2PI):
    """FixedNormal.log_probs, a2c/distributions.py:51-53, over torch's Normal(mean, logstd.exp()).log_prob -> [rows]"""
    scale = logstd.exp()
    return (-((action - mean) ** 2) / (2.0 * scale ** 2) - scale.log() - half_log_2pi).sum(-1)


def normal_entropy(logstd, half_log_2pi=HALF_LOG_2PI):
    """dist.entropy().mean(): a2c/distributions.py:55-56, a2c/model.py:262"""
    return (0.5 + half_log_2pi + logstd.exp().log()).sum(-1).mean()


# ------------------------------------------------------------------------------------------- the policies' forward
def policy_forward(kind, p, x, hxs0=None, masks=None, T=None, swap_logstd=False):
    """-> (values [rows], mean [rows, A], logstd [rows, A]) of Policy (mlp, gru: a2c/model.py:117-201, 233-264;
    a2c/distributions.py:91-118) or SplitPolicy (a2c/model_split.py:157-238).  gru: x [T * n, O] time-major, hxs0 [n, H],
    masks [T * n].  swap_logstd: a fault to inject (the log-std heads concatenated actuator first), for the test of the test."""
    if kind == "split":
        value = linear(p, "base.critic_full.4", trunk(p, "base.critic_full", x))
        contact, actuator = trunk(p, "base.actor_contact", x), trunk(p, "base.actor_actuator", x)
        # torch.cat in the reference's order, contact then actuator (model_split.py:235-236)
        mean = torch.cat((linear(p, "dist.contact_mean", contact), linear(p, "dist.actuator_mean", actuator)), 1)
        logstd = (linear(p, "dist.contact_logstd", contact), linear(p, "dist.actuator_logstd", actuator))
        logstd = torch.cat(logstd[::-1] if swap_logstd else logstd, 1)
        return value[:, 0], mean, logstd
    if kind == "gru":
        x = gru_states(p, x, hxs0, masks, T)
    value = linear(p, "base.critic_linear", trunk(p, "base.critic", x))
    mean = linear(p, "dist.fc_mean", trunk(p, "base.actor", x))
    logstd = torch.zeros_like(mean) + p["dist.logstd._bias"].t().view(1, -1)      # AddBias on zeros: distributions.py:112-117
    return value[:, 0], mean, logstd


def gru_states(p, x, hxs0, masks, T):
    """NNBase._forward_gru (a2c/model.py:146-201) through the real torch.nn.GRU, one step at a time with h * mask_t (the reference
    batches runs of steps without a reset; stepping is the same recurrence).  The module is the independent party: no cell is
    written here."""
    H, O = p["base.gru.weight_hh_l0"].shape[1], p["base.gru.weight_ih_l0"].shape[1]
    gru = torch.nn.GRU(O, H).to(F64)
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    assert [k for k, _ in gru.named_parameters()] == list(names)
    weights = {k: p["base.gru." + k] for k in names}
    n = x.shape[0] // T
    h, out = t64(hxs0).unsqueeze(0), []
    masks = t64(masks).reshape(T, n)
    for t in range(T):
        y, h = torch.func.functional_call(gru, weights, (x[t * n:(t + 1) * n].unsqueeze(0), h * masks[t].view(1, n, 1)))
        out.append(y[0])
    return torch.cat(out, 0)


# ------------------------------------------------------------------------------------------- PPO
def normalised_advantages(returns, value_preds, adv_eps=ADV_EPS):
    """a2c/algo/ppo.py:66-68 on the rollout's first T steps (torch's std is the unbiased one)"""
    adv = t64(returns) - t64(value_preds)
    return (adv - adv.mean()) / (adv.std() + adv_eps)


def ppo_loss(values, logp, entropy, old_logp, adv, vpred, ret, clip, vcoef, ecoef, use_clipped, sym=0.0):
    """a2c/algo/ppo.py:92-108, 139-142 -> (the scalar that is back-propagated, (value_loss, action_loss, entropy))"""
    ratio = torch.exp(logp - old_logp)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv
    action_loss = -torch.min(surr1, surr2).mean()
    if use_clipped:
        clipped = vpred + (values - vpred).clamp(-clip, clip)
        value_loss = 0.5 * torch.max((values - ret).pow(2), (clipped - ret).pow(2)).mean()
    else:
        value_loss = 0.5 * (ret - values).pow(2).mean()
    return value_loss * vcoef + action_loss - entropy * ecoef + sym, (value_loss, action_loss, entropy)


def ppo_grad(kind, shapes, params, obs, actions, old_logp, value_preds, returns, clip, vcoef, ecoef, use_clipped=True, hxs0=None,
             masks=None, T=None, consts=CONVENTION, symmetry=None, swap_logstd=False):
    """One minibatch of all rows (ppo_epoch = 1, num_mini_batch = 1): obs [rows, O] time-major, actions [rows, A], the rest [rows]
    -> (flat gradient, losses[3]).  symmetry = (mirrored rows [rows, O], M_a [A, A], coef): ppo.py:111-134 added; the fourth loss
    term is then mean(e^2)."""
    p = leaves(params, shapes)
    x = t64(obs)
    values, mean, logstd = policy_forward(kind, p, x, hxs0, masks, T, swap_logstd)
    logp = normal_log_probs(mean, logstd, t64(actions), consts["half_log_2pi"])
    entropy = normal_entropy(logstd, consts["half_log_2pi"])
    adv = normalised_advantages(returns, value_preds, consts["adv_eps"])
    extra, sym = (), 0.0
    if symmetry is not None:
        mrows, m_act, coef = symmetry
        extra = (symmetry_loss(kind, p, x, t64(mrows), t64(m_act)),)
        sym = extra[0] * coef
    total, parts = ppo_loss(values, logp, entropy, t64(old_logp), adv, t64(value_preds), t64(returns), clip, vcoef, ecoef, use_clipped, sym)
    return flat_grad(total, p), terms(*parts, *extra)


def symmetry_loss(kind, p, x, xm, m_act):
    """a2c/algo/ppo.py:111-134: (M_a mu(s) - mu(s_m))^2 .mean().  The .detach() is the reference's numpy round trip:
    mirror_obsact_batch (my_pybullet_envs/utils.py:334-357) takes act_mean to numpy, applies the mirror there and builds a new
    tensor, so no gradient reaches the actor through M_a mu(s); it flows through mu(s_m) alone."""
    assert kind == "mlp"
    mu = policy_forward(kind, p, x)[1]
    mum = policy_forward(kind, p, xm)[1]
    e = (mu @ m_act.t()).detach() - mum
    return e.pow(2).mean()


# ------------------------------------------------------------------------------------------- the discriminator step
def disc_shapes(F, Hd):
    return [("0.weight", (Hd, F)), ("0.bias", (Hd,)), ("2.weight", (Hd, Hd)), ("2.bias", (Hd,)), ("4.weight", (1, Hd)), ("4.bias", (1,))]


def disc_trunk(p, x):
    """nn.Sequential(Linear, Tanh, Linear, Tanh, Linear): a2c/algo/gail.py:40-43"""
    return linear(p, "4", torch.tanh(linear(p, "2", torch.tanh(linear(p, "0", x)))))


def disc_grad(F, Hd, params, expert, policy, alpha, lambda_=10.0):
    """Discriminator.update_gail_dyn's loss on one minibatch (a2c/algo/gail.py:168-187) with compute_grad_pen_combined (:67-89) at
    the given alpha: the penalty's gradient is a double backward -> (flat gradient, losses (total, expert, policy))."""
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    p = leaves(params, disc_shapes(F, Hd))
    e, q = t64(expert), t64(policy)
    expert_d, policy_d = disc_trunk(p, e), disc_trunk(p, q)
    expert_loss = bce(expert_d, torch.ones(expert_d.size(), dtype=F64))
    policy_loss = bce(policy_d, torch.zeros(policy_d.size(), dtype=F64))
    al = t64(alpha).reshape(-1, 1).expand_as(e)
    mixup = (al * e + (1 - al) * q).detach().requires_grad_(True)
    disc = disc_trunk(p, mixup)
    grad = torch.autograd.grad(outputs=disc, inputs=mixup, grad_outputs=torch.ones(disc.size(), dtype=F64), create_graph=True,
                               retain_graph=True, only_inputs=True)[0]
    grad_pen = lambda_ * (grad.norm(2, dim=1) - 1).pow(2).mean()
    total = expert_loss + policy_loss + grad_pen
    return flat_grad(total, p), terms(total, expert_loss, policy_loss)


# ------------------------------------------------------------------------------------------- A2C and ACKTR's statistics
def a2c_shapes(O, A, H, Hc):
    """Policy's state_dict order (test_a2c_host.policy_slices), the critic trunk Hc wide"""
    return [("base.actor.0.weight", (H, O)), ("base.actor.0.bias", (H,)), ("base.actor.2.weight", (H, H)), ("base.actor.2.bias", (H,)),
            ("base.critic.0.weight", (Hc, O)), ("base.critic.0.bias", (Hc,)), ("base.critic.2.weight", (Hc, Hc)), ("base.critic.2.bias", (Hc,)),
            ("base.critic_linear.weight", (1, Hc)), ("base.critic_linear.bias", (1,)),
            ("dist.fc_mean.weight", (A, H)), ("dist.fc_mean.bias", (A,)), ("dist.logstd._bias", (A, 1))]


def a2c_grad(dims, params, obs, actions, returns, vcoef, ecoef, consts=CONVENTION):
    """a2c/algo/a2c_acktr.py:60-73, 92-94 on all rows at once -> (flat gradient, (value_loss, action_loss, entropy))"""
    p = leaves(params, a2c_shapes(*dims))
    values, mean, logstd = policy_forward("mlp", p, t64(obs))
    logp = normal_log_probs(mean, logstd, t64(actions), consts["half_log_2pi"])
    entropy = normal_entropy(logstd, consts["half_log_2pi"])
    advantages = t64(returns).reshape(-1) - values
    value_loss = advantages.pow(2).mean()
    action_loss = -(advantages.detach() * logp).mean()
    return flat_grad(value_loss * vcoef + action_loss - entropy * ecoef, p), terms(value_loss, action_loss, entropy)


def acktr_factors(dims, params, obs, actions, eps):
    """The sampled Fisher statistics of one update (a2c/algo/a2c_acktr.py:75-90 with the case's value noise `eps`; kfac.py's
    _save_input / _save_grad_output with split_bias): for each of KFACOptimizer's modules the gradient of
    pg_fisher_loss + vf_fisher_loss with respect to the module's OUTPUT, by autograd.grad, and from it the 12 distinct factors in
    acktr_regimes.FACTORS order: fA = a^T a / B of a Linear's input (the bias is a module of its own, an AddBias whose A factor
    is 1), fG = B u^T u of the output's gradient u."""
    p = leaves(params, a2c_shapes(*dims))
    x = t64(obs)
    B = x.shape[0]
    pre, act = {}, {"obs": x}
    for tr in ("actor", "critic"):
        pre[tr + ".0"] = linear(p, f"base.{tr}.0", x)
        act[tr + "_h1"] = torch.tanh(pre[tr + ".0"])
        pre[tr + ".2"] = linear(p, f"base.{tr}.2", act[tr + "_h1"])
        act[tr + "_h2"] = torch.tanh(pre[tr + ".2"])
    pre["critic_linear"] = linear(p, "base.critic_linear", act["critic_h2"])
    pre["dist.fc_mean"] = linear(p, "dist.fc_mean", act["actor_h2"])
    pre["dist.logstd"] = torch.zeros_like(pre["dist.fc_mean"]) + p["dist.logstd._bias"].t().view(1, -1)   # AddBias's output, [rows, A]
    values = pre["critic_linear"]
    logp = normal_log_probs(pre["dist.fc_mean"], pre["dist.logstd"], t64(actions))
    pg_fisher_loss = -logp.mean()
    sample_values = values + t64(eps).reshape(-1, 1)
    vf_fisher_loss = -(values - sample_values.detach()).pow(2).mean()
    order = ["actor.0", "actor.2", "critic.0", "critic.2", "critic_linear", "dist.fc_mean", "dist.logstd"]
    us = torch.autograd.grad(pg_fisher_loss + vf_fisher_loss, [pre[k] for k in order])
    fA = [(a.t() @ a / B).detach().numpy() for a in (act[k] for k in ("obs", "actor_h1", "actor_h2", "critic_h1", "critic_h2"))]
    fG = [(B * (u.t() @ u)).numpy() for u in us]
    return fA + fG


def kfac_solve(grad, d_g, q_g, d_a, q_a, damping):
    """K-FAC's preconditioned gradient of one module WITHOUT the eigen path (kfac.py:225-249 solves in the eigenbases): rebuild the
    thresholded factors G' = Q_g diag(d_g) Q_g^T, A' = Q_a diag(d_a) Q_a^T and solve (G' (x) A' + damping I) vec(v) = vec(grad)
    densely (row-major vec of the [out, in] matrix; A' is symmetric).  One step of iterative refinement: at damping 1e-5 the system's
    condition number is ~1e6, and the residual is cheap."""
    d_g, q_g, d_a, q_a = (np.asarray(a, np.float64) for a in (d_g, q_g, d_a, q_a))
    G, A = (q_g * d_g) @ q_g.T, (q_a * d_a) @ q_a.T
    M = np.kron(G, A) + damping * np.eye(G.shape[0] * A.shape[0])
    b = np.asarray(grad, np.float64).reshape(-1)
    v = np.linalg.solve(M, b)
    v = v + np.linalg.solve(M, b - M @ v)
    return v


# ------------------------------------------------------------------------------------------- the regimes modules' cases
def ppo_case_grad(c, use_clipped=True, consts=CONVENTION, params=None, swap_logstd=False):
    """regimes.grad(c, use_clipped, 64)'s counterpart on a tests/regimes.py case"""
    import regimes as rg
    B = c.T * c.N
    gru = dict(hxs0=c.hxs0, masks=c.masks[:-1].reshape(B), T=c.T) if c.kind == "gru" else {}
    return ppo_grad(c.kind, rg.param_shapes(c.kind, c.O, c.A, c.H, c.f), c.params if params is None else params, c.obs[:-1].reshape(B, c.O),
                    c.actions.reshape(B, c.A), c.action_log_probs.reshape(B), c.value_preds[:-1].reshape(B), c.returns[:-1].reshape(B),
                    rg.CLIP, rg.VCOEF, c.entropy_coef, use_clipped, consts=consts, swap_logstd=swap_logstd, **gru)


def sym_case_grad(c, use_clipped=True, m_act=None):
    """the symmetric one-step gradient of a tests/sym_regimes.py case -> (flat gradient, (value_loss, action_loss, entropy, mean(e^2)))"""
    import regimes as rg
    B = c.T * c.N
    return ppo_grad("mlp", rg.param_shapes("mlp", c.O, c.A, c.H, 1), c.params, c.obs[:-1].reshape(B, c.O), c.actions.reshape(B, c.A),
                    c.action_log_probs.reshape(B), c.value_preds[:-1].reshape(B), c.returns[:-1].reshape(B), rg.CLIP, rg.VCOEF,
                    c.entropy_coef, use_clipped, symmetry=(c.mrows, c.m_act if m_act is None else m_act, c.symmetry_coef))


def disc_case_grad(c, expert=None, policy=None, alpha=None):
    import disc_regimes as dr
    return disc_grad(c.F, c.Hd, c.params, c.expert if expert is None else expert, c.policy if policy is None else policy,
                     c.alpha if alpha is None else alpha, dr.LAMBDA)


def a2c_case_grad(c):
    """A2C on a tests/regimes.py mlp case (regimes.a2c_restated's rollout)"""
    import regimes as rg
    B = c.T * c.N
    return a2c_grad((c.O, c.A, c.H, c.H), c.params, c.obs[:-1].reshape(B, c.O), c.actions.reshape(B, c.A), c.returns[:-1].reshape(B),
                    rg.VCOEF, c.entropy_coef)


# ------------------------------------------------------------------------------------------- restatement against autograd
BOUND = 1e-9          # per block; see tests/test_autograd_arbiter_host.py
LOSS_ATOL = 1e-12


def judge(restated, autograd, named_blocks, distances, losses_restated=(), losses_autograd=()):
    """One comparison -> dict(worst_block, worst, distances, loss_error, zeros_broken).  distances(got, ref) is the family's own
    block_distances at atol = 0, the restatement measured FROM autograd; zeros_broken: the blocks in which autograd's gradient is
    exactly 0.0 and the restatement's is not."""
    restated, autograd = np.asarray(restated, np.float64), np.asarray(autograd, np.float64)
    d = distances(restated, autograd)
    broken = [k for (k, a), (_, r) in zip(named_blocks(autograd), named_blocks(restated)) if not a.any() and r.any()]
    zero = [k for k, a in named_blocks(autograd) if not a.any()]
    worst = max(d, key=d.get)
    err = float(np.max(np.abs(np.asarray(losses_restated, np.float64) - np.asarray(losses_autograd, np.float64)))) if len(losses_restated) else 0.0
    return dict(worst_block=worst, worst=d[worst], distances=d, loss_error=err, zeros_broken=broken, zero_blocks=zero)


def passes(j):
    return j["worst"] <= BOUND and j["loss_error"] <= LOSS_ATOL and not j["zeros_broken"]


def judge_ppo(c, use_clipped, restated=None, **kw):
    import regimes as rg
    key = "clipped" if use_clipped else "plain"
    g, losses = ppo_case_grad(c, use_clipped, **kw)
    return judge(c.desc["grad_" + key] if restated is None else restated, g, lambda v: rg.blocks(c.kind, c.O, c.A, c.H, c.f, v),
                 lambda a, b: rg.block_distances(a, b, c.kind, c.O, c.A, c.H, c.f, 0.0), c.desc["losses_" + key], losses)


def first_minibatch(c, perm_seed, M=2):
    """The first step of tests/test_gpu_regimes.py's 2c (E = 2, M = 2 over regimes.clip_perms): half the rows (GRU: half the
    environments) with advantages normalised over the whole rollout -> (restated gradient, losses, autograd gradient, losses)."""
    import gru_ref
    import regimes as rg
    perm = rg.clip_perms(c, perm_seed)[0]
    B, adv = c.T * c.N, rg.advantages64(c)
    shapes = rg.param_shapes(c.kind, c.O, c.A, c.H, c.f)
    if c.kind == "gru":
        envs = perm[:c.N // M]
        tm = lambda a: np.asarray(a)[:, envs].reshape(c.T * envs.size, -1)  # noqa: E731
        args = (tm(c.obs[:-1]), c.hxs0[envs], tm(c.masks[:-1])[:, 0], tm(c.actions), tm(c.action_log_probs)[:, 0], tm(adv[..., None])[:, 0],
                tm(c.value_preds[:-1])[:, 0], tm(c.returns[:-1])[:, 0])
        g, losses = gru_ref.minibatch_grad(gru_ref.unflatten(c.params, c.O, c.A, c.H), *args, rg.CLIP, rg.VCOEF, c.entropy_coef, True)
        g, losses = gru_ref.flatten(g, c.O, c.A, c.H), np.array(losses)
        obs, hxs0, masks, act, olp, advr, vp, ret = args
        gru = dict(hxs0=hxs0, masks=masks, T=c.T)
    else:
        from oracle import oracle64 as orc
        rows = perm[:B // M]
        flat = lambda a: np.asarray(a).reshape(B, -1)  # noqa: E731
        cfg = orc.ppo_cfg(rg.CLIP, 1, M, rg.VCOEF, c.entropy_coef, 3e-4, 1e-5, 1e9, True)
        g, sums = orc.ppo_grad_rows(rg._dims(c, orc), c.params, cfg, flat(c.obs[:-1]), flat(c.actions), flat(c.value_preds[:-1])[:, 0],
                                    flat(c.returns[:-1])[:, 0], flat(c.action_log_probs)[:, 0], adv.reshape(B), rows, 1.0 / rows.size)
        losses = sums / rows.size
        obs, act, olp, advr, vp, ret = (flat(a)[rows] for a in (c.obs[:-1], c.actions, c.action_log_probs, adv, c.value_preds[:-1], c.returns[:-1]))
        olp, advr, vp, ret = olp[:, 0], advr[:, 0], vp[:, 0], ret[:, 0]
        gru = {}
    p = leaves(c.params, shapes)
    values, mean, logstd = policy_forward(c.kind, p, t64(obs), **gru)
    total, parts = ppo_loss(values, normal_log_probs(mean, logstd, t64(act)), normal_entropy(logstd), t64(olp), t64(advr), t64(vp), t64(ret),
                            rg.CLIP, rg.VCOEF, c.entropy_coef, True)
    return np.asarray(g, np.float64), losses, flat_grad(total, p), terms(*parts)


def judge_first_minibatch(c, perm_seed):
    import regimes as rg
    g, losses, ga, la = first_minibatch(c, perm_seed)
    return judge(g, ga, lambda v: rg.blocks(c.kind, c.O, c.A, c.H, c.f, v), lambda a, b: rg.block_distances(a, b, c.kind, c.O, c.A, c.H, c.f, 0.0),
                 losses, la)


def judge_a2c(c, restated=None):
    """test_a2c_host.a2c_loss_grad on a tests/regimes.py mlp case (regimes.a2c_restated's rows)"""
    import regimes as rg
    from test_a2c_host import a2c_loss_grad
    B = c.T * c.N
    losses, g = a2c_loss_grad(c.params, c.obs[:-1].reshape(B, c.O), c.actions.reshape(B, c.A), c.returns[:-1].reshape(B), (c.O, c.A, c.H, c.H),
                              rg.VCOEF, c.entropy_coef)
    ga, la = a2c_case_grad(c)
    return judge(g if restated is None else restated, ga, lambda v: rg.blocks("mlp", c.O, c.A, c.H, 1, v),
                 lambda a, b: rg.block_distances(a, b, "mlp", c.O, c.A, c.H, 1, 0.0), losses, la)


def judge_disc(c, restated=None, rows=None):
    """rows = (expert, policy, alpha): another minibatch of the case's discriminator (an epoch case's first step)"""
    import disc_regimes as dr
    if rows is None:
        g, losses = c.desc["grad"], c.desc["losses"]
        ga, la = disc_case_grad(c)
    else:
        sub = dr.Case(c)
        sub["expert"], sub["policy"], sub["alpha"] = rows
        g, losses, _ = dr.grad(sub, 64)
        ga, la = disc_case_grad(sub)
    return judge(g if restated is None else restated, ga, lambda v: dr.blocks(c.F, c.Hd, v), lambda a, b: dr.block_distances(a, b, c.F, c.Hd, 0.0),
                 losses, la)


def epoch_first_step(c, batch):
    """the rows of the first step of an epoch case's first epoch (orc_disc_update: perm[:batch], alpha[:batch])"""
    ep, pp, al = c.draws[0]
    return c.expert[ep[:batch]], c.policy[pp[:batch]], al[:batch]


def judge_sym(c, use_clipped, **kw):
    import regimes as rg
    key = "clipped" if use_clipped else "plain"
    ga, la = sym_case_grad(c, use_clipped, **kw)
    return judge(c["grad_" + key], ga, lambda v: rg.blocks("mlp", c.O, c.A, c.H, 1, v),
                 lambda a, b: rg.block_distances(a, b, "mlp", c.O, c.A, c.H, 1, 0.0), list(c["losses_" + key]) + [c.sym_loss], la)


KFAC_SOLVE_MAX = 2048     # elements of a case's largest module up to which the dense solve (n^3) stays well under a second


def judge_acktr(c, solve):
    """Every update of a tests/acktr_regimes.py case -> [dict(gradient=judge(...), factors={factor: distance}, kfac={block:
    distance} or None)]: a2c_loss_grad's gradient and losses, the 12 running factors (autograd's statistics folded exactly as
    kfac.py:172-173 folds them: the first update's factor itself, then stat_decay m + (1 - stat_decay) f), and, where `solve`,
    info.v of every module against the dense solve."""
    import acktr_regimes as ak
    from test_a2c_host import policy_slices
    sl, _ = policy_slices(*c.dims)
    O, A = c.dims[0], c.dims[1]
    named = lambda v: [(name, v[sl[key][0]]) for name, (key, _, _) in zip(ak.BLOCKS, ak.MODULES)]  # noqa: E731
    out, running, sd = [], None, c.cfg["stat_decay"]
    for u, d in zip(c.updates, c.desc):
        T = u["obs"].shape[0] - 1
        x, act, ret = u["obs"][:T].reshape(-1, O), u["actions"].reshape(-1, A), u["returns"][:T].reshape(-1)
        ga, la = a2c_grad(c.dims, u["params"], x, act, ret, ak.VCOEF, ak.ECOEF)
        rec = dict(gradient=judge(d["g"], ga, named, lambda a, b: ak.block_distances(a, b, c.dims, 0.0), d["losses"], la))
        f = acktr_factors(c.dims, u["params"], x, act, u["eps"])
        running = f if running is None else [sd * m + (1.0 - sd) * fj for m, fj in zip(running, f)]
        rec["factors"] = ak.factor_distances(ak.state_factors(d), running)
        rec["kfac"] = None
        if solve:
            rec["kfac"] = {}
            for name, (key, fa, fg) in zip(ak.BLOCKS, ak.MODULES):
                s, shape = sl[key]
                da, qa = (np.ones(1), np.ones((1, 1))) if fa is None else d["eA"][fa]
                dg, qg = d["eG"][fg]
                v = kfac_solve(d["g"][s], dg, qg, da, qa, c.cfg["damping"])
                rec["kfac"][name] = float(np.linalg.norm(d["v"][s] - v) / (np.linalg.norm(v) + 1e-300))
        out.append(rec)
    return out


def largest_module(dims):
    from test_a2c_host import policy_slices
    return max(int(np.prod(shape)) for _, shape in policy_slices(*dims)[0].values())


# ------------------------------------------------------------------------------------------- tier 2: the reference's own modules
TIER2_PPO = [("mlp", 5, 2, 8, 1), ("split", 14, 7, 100, 1), ("gru", 13, 5, 20, 1)]      # off_policy, both value losses
TIER2_DISC = ("both_sides", 7, 16, 13)


def tier2():
    """Only where the reference checkout is present, and only in a process of its own (tools/ref_import.py puts stand-in modules
    and the reference's `third_party` package into the interpreter): the reference's own Policy / SplitPolicy with PPO.update, and
    its Discriminator with update_gail_dyn, after .double() and with the case's parameters loaded, run their own loss and
    .backward(); the .grad they leave is compared with this file at BOUND.  Nothing of the reference is copied: it is imported.
    After .double() the reference's constants are the exact doubles, so this file is evaluated with EXACT here (and only here).
    -> {label: judge(...)}"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (root, os.path.join(root, "tools"), os.path.join(root, "tests")):
        if path not in sys.path:
            sys.path.insert(0, path)
    import disc_regimes as dr
    import regimes as rg
    cases = [rg.case("off_policy", *spec) for spec in TIER2_PPO]       # (the oracle is loaded before the reference's packages)
    dc = dr.case(*TIER2_DISC)
    from ref_import import import_reference
    ns = import_reference()
    out = {}

    def load(module, flat, shapes):
        module.double()
        sd = {k: v.detach().clone() for k, v in leaves(flat, shapes).items()}
        assert list(module.state_dict()) == list(sd), (list(module.state_dict()), list(sd))
        module.load_state_dict(sd)
        return module

    def grads(module):
        return np.concatenate([q.grad.reshape(-1).numpy() for q in module.parameters()])

    for c in cases:
        kw = {"hidden_size": c.H, "num_feet": c.f} if c.kind == "split" else {"recurrent": c.kind == "gru", "hidden_size": c.H}
        shapes = rg.param_shapes(c.kind, c.O, c.A, c.H, c.f)
        for uc in (True, False):
            policy = load((ns.SplitPolicy if c.kind == "split" else ns.Policy)((c.O,), ns.Box(shape=(c.A,)), base_kwargs=kw), c.params, shapes)
            ro = ns.RolloutStorage(c.T, c.N, (c.O,), ns.Box(shape=(c.A,)), c.H if c.kind == "gru" else 1, 1)
            for name in ("obs", "actions", "value_preds", "returns", "action_log_probs", "masks"):
                setattr(ro, name, t64(c[name]))
            ro.obs_feat, ro.recurrent_hidden_states = ro.obs_feat.double(), ro.recurrent_hidden_states.double()
            if c.kind == "gru":
                ro.recurrent_hidden_states[0] = t64(c.hxs0)
            agent = ns.PPO(policy, rg.CLIP, 1, 1, rg.VCOEF, c.entropy_coef, lr=rg.LR, eps=rg.EPS, max_grad_norm=1e9, use_clipped_value_loss=uc)
            losses = agent.update(ro)          # one minibatch of every row (GRU: every environment), in an order of its own
            ga, la = ppo_case_grad(c, uc, consts=EXACT)
            out[f"ppo {c.tag} {'clipped' if uc else 'plain'}"] = judge(
                ga, grads(policy), lambda v: rg.blocks(c.kind, c.O, c.A, c.H, c.f, v),
                lambda a, b: rg.block_distances(a, b, c.kind, c.O, c.A, c.H, c.f, 0.0), la, losses)

    class Loader(list):
        batch_size = dc.expert.shape[0]

    class Rollouts:     # feed_forward_generator's last element is the policy rows (storage.py:191-193)
        def feed_forward_generator(self, advantages, mini_batch_size=None):
            yield (t64(dc.policy),)

    disc = ns.Discriminator(dc.F, dc.Hd, "cpu")
    load(disc.trunk, dc.params, disc_shapes(dc.F, dc.Hd))
    # compute_grad_pen_combined draws alpha itself (gail.py:72): the same draw from the same seed, handed to this file
    torch.manual_seed(11)
    alpha = torch.rand(dc.expert.shape[0], 1).double().numpy()[:, 0]
    torch.manual_seed(11)
    losses = disc.update_gail_dyn(Loader([(t64(dc.expert),)]), Rollouts())
    ga, la = disc_case_grad(dc, alpha=alpha)
    out[f"disc {dc.tag}, alpha of seed 11"] = judge(ga, grads(disc.trunk), lambda v: dr.blocks(dc.F, dc.Hd, v),
                                                    lambda a, b: dr.block_distances(a, b, dc.F, dc.Hd, 0.0), la, losses)
    return out


def _brief(j):
    return {k: j[k] for k in ("worst_block", "worst", "loss_error", "zeros_broken")}


def reference_present():
    """whether tools/ref_import.py's reference checkout exists (read without putting tools/ on this process's path)"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("_ref_import_probe", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                     "tools", "ref_import.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return os.path.isdir(mod.REFERENCE_ROOT)


def survey():
    """every comparison of tests/test_autograd_arbiter_host.py's first tier -> {family: {label: figures}}"""
    import acktr_regimes as ak
    import disc_regimes as dr
    import gru_ref
    import regimes as rg
    import sym_regimes as sr
    doc = {"ppo": {}, "ppo_first_minibatch": {}, "a2c": {}, "disc": {}, "acktr": {}, "sym": {}}
    for spec in rg.all_cases():
        c = rg.case(*spec)
        for uc in (True, False):
            doc["ppo"][f"{c.tag} {'clipped' if uc else 'plain'}"] = _brief(judge_ppo(c, uc))
    for spec, seed in rg.CLIP_CASES:
        c = rg.case("off_policy", *spec)
        doc["ppo_first_minibatch"][c.tag] = _brief(judge_first_minibatch(c, seed))
    c = rg.case("off_policy", *rg.A2C_CLIP_CASE)
    doc["a2c"][c.tag] = _brief(judge_a2c(c))
    for c in [dr.case(*spec) for spec in dr.all_cases()] + [dr.zero_head_case()]:
        doc["disc"][c.tag] = _brief(judge_disc(c))
    for shape in dr.EPOCH_SHAPES:
        c = dr.epoch_case(*shape)
        doc["disc"][c.tag + ", first step"] = _brief(judge_disc(c, rows=epoch_first_step(c, dr.EPOCH_B)))
    for name in ak.all_cases():
        c = ak.case(name)
        for k, r in enumerate(judge_acktr(c, largest_module(c.dims) <= KFAC_SOLVE_MAX)):
            doc["acktr"][f"{c.tag} update {k}"] = dict(gradient=_brief(r["gradient"]), worst_factor=max(r["factors"], key=r["factors"].get),
                                                      factor=max(r["factors"].values()),
                                                      kfac_dense_solve=None if r["kfac"] is None else max(r["kfac"].values()))
    for spec in sr.all_cases():
        c = sr.case(*spec)
        for uc in ((True,) if c.regime == "sym_only" else (True, False)):
            doc["sym"][f"{c.tag} {'clipped' if uc else 'plain'}"] = _brief(judge_sym(c, uc))
    # the two constant conventions on the recurrent policy: gru_ref with the EXACT doubles against this file with the exact doubles
    # (the figure the convention's change leaves behind), and against this file on the convention (the split that was there before)
    doc["gru_constants"] = {}
    saved = gru_ref.HALF_LOG_2PI, gru_ref.ADV_EPS
    try:
        gru_ref.HALF_LOG_2PI, gru_ref.ADV_EPS = EXACT["half_log_2pi"], EXACT["adv_eps"]
        for spec in rg.SHAPES:
            if spec[0] == "gru":
                c = rg.case("off_policy", *spec)
                g, _ = rg.grad(c, True, 64)
                doc["gru_constants"][c.tag] = {
                    "gru_ref exact vs autograd exact": _brief(judge_ppo(c, True, restated=g, consts=EXACT))["worst"],
                    "gru_ref exact vs autograd float32-valued": _brief(judge_ppo(c, True, restated=g))["worst"]}
    finally:
        gru_ref.HALF_LOG_2PI, gru_ref.ADV_EPS = saved
    return doc


if __name__ == "__main__":   # profiles/autograd_arbiter.json; `--tier2` prints tier 2 alone (the test's child process)
    import json
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if "--tier2" in sys.argv:
        print("TIER2 " + json.dumps({k: _brief(j) for k, j in tier2().items()}))
        sys.exit(0)
    sys.path.insert(0, ROOT)
    doc = {"what": "python tests/autograd_ref.py: every float64 restatement's distance from torch.float64 autograd of the reference's loss "
                   "written forward-only (tier 1: worst block and its distance by the family's block_distances at atol = 0, largest "
                   "loss-term error), the reference's own modules' .grad against the same autograd expressions (tier 2; null where "
                   "the reference checkout is absent), and the recurrent policy under both constant conventions.",
           "bound": BOUND, "loss_atol": LOSS_ATOL, "constants": CONVENTION}
    doc["tier1"] = survey()
    doc["tier2"] = None
    if reference_present():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tier2"], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        doc["tier2"] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TIER2 ")][-1][6:])
    flat = [x for fam in ("ppo", "ppo_first_minibatch", "a2c", "disc", "sym") for x in doc["tier1"][fam].values()]
    flat += [x["gradient"] for x in doc["tier1"]["acktr"].values()] + list((doc["tier2"] or {}).values())
    doc["worst_gradient_distance"] = max(x["worst"] for x in flat)
    doc["worst_factor_distance"] = max(x["factor"] for x in doc["tier1"]["acktr"].values())
    doc["worst_kfac_dense_solve_distance"] = max(x["kfac_dense_solve"] or 0.0 for x in doc["tier1"]["acktr"].values())
    def lines(x, depth=0):     # one line per case: the record is read by people
        if not isinstance(x, dict) or (x and not any(isinstance(v, dict) for v in x.values())):
            return json.dumps(x)
        pad = " " * (depth + 1)
        return "{\n" + ",\n".join(f"{pad}{json.dumps(k)}: {lines(v, depth + 1)}" for k, v in x.items()) + "\n" + " " * depth + "}"
    with open(os.path.join(ROOT, "profiles", "autograd_arbiter.json"), "w") as f:
        f.write(lines(doc) + "\n")
    print({k: doc[k] for k in ("worst_gradient_distance", "worst_factor_distance", "worst_kfac_dense_solve_distance")}, doc["tier1"]["gru_constants"])
