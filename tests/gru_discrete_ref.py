"""The arbiter of the recurrent Policy on Discrete / MultiBinary action spaces (a2c/model.py:40-62,117-201 with
base_kwargs={'recurrent': True}): the reference's PPO and A2C losses (a2c/algo/ppo.py:74-108, a2c/algo/a2c_acktr.py:56-91) written
FORWARD-ONLY in torch and differentiated by torch.autograd.  The GRU is torch.nn.GRU itself, stepped with h <- h * masks[t]
(tests/autograd_ref.py:gru_states, here in any dtype); the heads, log-probs and entropies are tests/discrete_ref.py's
(torch's Categorical / Bernoulli arithmetic on the logits; Bernoulli: log-probs summed over the bits, the entropy summed over the
bits and then averaged over the rows, a2c/distributions.py:63-71).  dtype=torch.float32 evaluates the very same expressions in
float32: a case counts only where that evaluation stays within half the bound of float64 (`admit`).

`wrong=` injects the faults the tests must be able to see (the test of the test):
  "no_critic_dh"   the critic trunk's d loss / d h_t left out of the reverse scan (every heads block right, every GRU block wrong)
  "no_actor_dh"    the actor trunk's left out
  "no_mask"        masks ignored
  "entropy_mean"   the Bernoulli entropy averaged over the bits, not summed
  "padding"        nonzero d loss / d logits in the head tile's padding columns folded into d loss / d h_t"""
import numpy as np
import torch

import autograd_ref as ar
import discrete_ref as dr

RTOL_BLOCK = 1e-4      # the project's bound per parameter block (tests/a2c_gru_ref.py)
CATEGORICAL, BERNOULLI = dr.CATEGORICAL, dr.BERNOULLI
CLIP, VCOEF, ECOEF = dr.CLIP, dr.VCOEF, dr.ECOEF
GRU_NAMES = ("base.gru.weight_ih_l0", "base.gru.weight_hh_l0", "base.gru.bias_ih_l0", "base.gru.bias_hh_l0")
WRONG = ("no_critic_dh", "no_actor_dh", "no_mask", "entropy_mean", "padding")


def param_shapes(O, K, H):
    """state_dict order: nn.GRU's four tensors first (a2c/model.py:124-131), the trunks on its H-wide state, dist.linear last"""
    return [(GRU_NAMES[0], (3 * H, O)), (GRU_NAMES[1], (3 * H, H)), (GRU_NAMES[2], (3 * H,)), (GRU_NAMES[3], (3 * H,))] + dr.param_shapes(H, K, H)


def gru_count(O, K, H):
    return sum(int(np.prod(s)) for _, s in param_shapes(O, K, H)[:4])


def blocks(O, K, H):
    """[(block name, slice of the flat vector)]: every parameter tensor, the GRU's gate by gate (r, z, n)"""
    out, off = [], 0
    for name, shape in param_shapes(O, K, H):
        n = int(np.prod(shape))
        if name in GRU_NAMES:
            for k, gate in enumerate("rzn"):
                out.append((f"{name}[{gate}]", slice(off + k * n // 3, off + (k + 1) * n // 3)))
        else:
            out.append((name, slice(off, off + n)))
        off += n
    return out


def block_errors(got, ref, O, K, H):
    """{block: max|got - ref| / max|ref| over the block}"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return {name: float(np.max(np.abs(got[sl] - ref[sl])) / (np.max(np.abs(ref[sl])) + 1e-300)) for name, sl in blocks(O, K, H)}


def gru_states(p, x, hxs0, masks, T, dtype=ar.F64):
    """NNBase._forward_gru (a2c/model.py:146-201) through the real torch.nn.GRU, one step at a time with h * mask_t"""
    H, O = p[GRU_NAMES[1]].shape[1], p[GRU_NAMES[0]].shape[1]
    gru = torch.nn.GRU(O, H).to(dtype)
    weights = {k.split(".")[-1]: p[k] for k in GRU_NAMES}
    assert [k for k, _ in gru.named_parameters()] == list(weights)
    n = x.shape[0] // T
    h, out = dr._t(hxs0, dtype).unsqueeze(0), []
    masks = dr._t(masks, dtype).reshape(T, n)
    for t in range(T):
        y, h = torch.func.functional_call(gru, weights, (x[t * n:(t + 1) * n].unsqueeze(0), h * masks[t].view(1, n, 1)))
        out.append(y[0])
    return torch.cat(out, 0)


def forward(dist, p, obs, hxs0, masks, T, actions, dtype=ar.F64, wrong=None):
    """Policy.evaluate_actions over a sequence -> (values [rows], logp [rows], entropy (a scalar: the mean over rows), logits,
    the extra loss term of wrong="padding")"""
    if wrong == "no_mask":
        masks = np.ones_like(np.asarray(masks, np.float64))
    x = gru_states(p, dr._t(obs, dtype), hxs0, masks, T, dtype)
    xa = x.detach() if wrong == "no_actor_dh" else x
    xc = x.detach() if wrong == "no_critic_dh" else x
    a2 = ar.trunk(p, "base.actor", xa)
    values = ar.linear(p, "base.critic_linear", ar.trunk(p, "base.critic", xc))[:, 0]
    z = ar.linear(p, "dist.linear", a2)
    logp = dr.log_probs(dist, z, actions)
    ent_rows = dr.entropy_rows(dist, z)
    if wrong == "entropy_mean" and dist == BERNOULLI:
        ent_rows = ent_rows / z.shape[1]
    extra = 0.0
    if wrong == "padding":     # a padding column whose gradient is not zero reaches h_t through the head's rows behind K
        K = z.shape[1]
        wpad = dr._t(np.random.default_rng(K).standard_normal(((-K) % 16 or 16, a2.shape[1])), dtype)
        extra = 1e-3 * (a2 @ wpad.t()).sum() / z.shape[0]
    return values, logp, ent_rows.mean(), z, extra


def _flat(total, p):
    gs = torch.autograd.grad(total, list(p.values()), allow_unused=True)
    return np.concatenate([(torch.zeros_like(x) if g is None else g).reshape(-1).double().numpy() for g, x in zip(gs, p.values())])


def _rows(c):
    """the time-major rows of the whole rollout: obs[:-1], masks[:-1], actions, ..."""
    T, N = c["T"], c["N"]
    tm = lambda a: np.asarray(a)[:T].reshape(T * N, -1)  # noqa: E731
    return tm(c["obs"]), c["hxs0"], tm(c["masks"])[:, 0], tm(c["actions"])


def a2c_grad(c, vcoef=VCOEF, ecoef=ECOEF, dtype=ar.F64, wrong=None):
    """a2c/algo/a2c_acktr.py:56-73, 92-94 over the whole rollout -> (flat gradient, (value_loss, action_loss, entropy))"""
    p = dr._leaves(c["params"], param_shapes(c["O"], c["K"], c["H"]), dtype)
    obs, hxs0, masks, actions = _rows(c)
    values, logp, ent, _, extra = forward(c["dist"], p, obs, hxs0, masks, c["T"], actions, dtype, wrong)
    adv = dr._t(c["returns"][:c["T"]].reshape(-1), dtype) - values
    value_loss = adv.pow(2).mean()
    action_loss = -(adv.detach() * logp).mean()
    return _flat(value_loss * vcoef + action_loss - ent * ecoef + extra, p), ar.terms(value_loss, action_loss, ent)


def ppo_grad(c, use_clipped=True, clip=CLIP, vcoef=VCOEF, ecoef=ECOEF, dtype=ar.F64, wrong=None, adv_eps=ar.ADV_EPS):
    """a2c/algo/ppo.py:66-108 with ppo_epoch = 1 and one minibatch of every environment -> (flat gradient, losses[3]).  adv_eps:
    the float32 value of 1e-5 (tests/autograd_ref.py's convention); the exact double only against the reference after .double()"""
    p = dr._leaves(c["params"], param_shapes(c["O"], c["K"], c["H"]), dtype)
    obs, hxs0, masks, actions = _rows(c)
    B = c["T"] * c["N"]
    values, logp, ent, _, extra = forward(c["dist"], p, obs, hxs0, masks, c["T"], actions, dtype, wrong)
    vp, ret = c["value_preds"][:c["T"]].reshape(B), c["returns"][:c["T"]].reshape(B)
    adv = ar.normalised_advantages(ret, vp, adv_eps).to(dtype)
    total, parts = ar.ppo_loss(values, logp, ent, dr._t(c["action_log_probs"].reshape(B), dtype), adv, dr._t(vp, dtype), dr._t(ret, dtype),
                               clip, vcoef, ecoef, use_clipped)
    return _flat(total + extra, p), ar.terms(*parts)


def evaluate(c, dtype=ar.F64):
    """-> (values, logp, entropy rows, logits, states) of the rollout's rows as float64 numpy"""
    p = dr._leaves(c["params"], param_shapes(c["O"], c["K"], c["H"]), dtype)
    obs, hxs0, masks, actions = _rows(c)
    with torch.no_grad():
        x = gru_states(p, dr._t(obs, dtype), hxs0, masks, c["T"], dtype)
        v, z = dr.forward(c["dist"], p, x)
        return (v.double().numpy(), dr.log_probs(c["dist"], z, actions).double().numpy(), dr.entropy_rows(c["dist"], z).double().numpy(),
                z.double().numpy(), x.double().numpy())


def surrogate_branches(c, clip=CLIP):
    """-> (rows clipped low, inside, clipped high, the smallest distance of a ratio from a clip boundary), on the float64 side"""
    logp = evaluate(c)[1]
    ratio = np.exp(logp - c["action_log_probs"].reshape(-1).astype(np.float64))
    lo, hi = 1.0 - clip, 1.0 + clip
    return (int((ratio < lo).sum()), int(((ratio >= lo) & (ratio <= hi)).sum()), int((ratio > hi).sum()),
            float(min(np.abs(ratio - lo).min(), np.abs(ratio - hi).min())))


def admit(c, algo, use_clipped=True):
    """-> (float64 gradient, losses, the worst block of the float32 evaluation of the same expression against it)"""
    f = (lambda **kw: ppo_grad(c, use_clipped, **kw)) if algo == "ppo" else (lambda **kw: a2c_grad(c, **kw))
    g64, l64 = f()
    g32, _ = f(dtype=torch.float32)
    return g64, l64, max(block_errors(g32, g64, c["O"], c["K"], c["H"]).values())


# ------------------------------------------------------------------------------------------- cases
def init_params(O, K, H, seed):
    """a policy in the middle of training: trunks and head as tests/discrete_ref.py draws them, GRU weights of the same scale"""
    rng = np.random.default_rng([seed, O, K, H])
    parts = []
    for name, shape in param_shapes(O, K, H):
        if name.endswith("weight") or "weight_" in name:
            s = 1.0 if name.startswith("dist.") else (0.8 if name in GRU_NAMES else 0.6)
            parts.append((rng.standard_normal(shape) * s / np.sqrt(shape[-1])).astype(np.float32).reshape(-1))
        else:
            parts.append((0.1 * rng.standard_normal(shape)).astype(np.float32).reshape(-1))
    return np.concatenate(parts)


def random_case(dist, O, K, H, T, N, seed=0, dead_env=None):
    """A rollout off the on-policy point -> dict(dist, O, K, H, T, N, A, params, obs [T+1,N,O], masks [T+1,N,1] (zeros at p = 0.08,
    slot 0 included), hxs0 [N,H] non-zero, actions [T,N,A] drawn from a behaviour policy, action_log_probs [T,N,1] placed so that a
    third of the rows is clipped low, a third high and none is within 1e-3 of a clip boundary, value_preds / returns [T+1,N,1] around
    the policy's values).  dead_env: that environment's masks are 0 at every step."""
    rng = np.random.default_rng([seed, dist, O, K, H, T, N])
    A = 1 if dist == CATEGORICAL else K
    c = dict(dist=dist, O=O, K=K, H=H, T=T, N=N, A=A)
    c["params"] = init_params(O, K, H, seed)
    c["obs"] = rng.standard_normal((T + 1, N, O)).astype(np.float32)
    masks = (rng.random((T + 1, N, 1)) > 0.08).astype(np.float32)
    masks[0, N // 2] = 0.0
    if dead_env is not None:
        masks[:, dead_env] = 0.0
    c["masks"] = masks
    c["hxs0"] = (0.5 * rng.standard_normal((N, H))).astype(np.float32)
    c["actions"] = np.zeros((T, N, A), np.float32)
    c["action_log_probs"] = np.zeros((T, N, 1), np.float32)
    v, _, _, z, _ = evaluate(c)
    u = rng.random((T * N, A)).astype(np.float32)
    acts = dr.sample(dist, z + 0.3 * rng.standard_normal(z.shape), u)      # a behaviour policy near this one
    c["actions"] = acts.reshape(T, N, A).astype(np.int64 if dist == CATEGORICAL else np.float32)
    logp = evaluate(c)[1]
    shift = 0.05 * rng.standard_normal(T * N)
    shift[0::3] = np.log(1.0 - CLIP) - 0.12          # ratio = exp(shift)
    shift[1::3] = np.log(1.0 + CLIP) + 0.12
    old = (logp - shift).astype(np.float32)
    for _ in range(4):
        ratio = np.exp(logp - old.astype(np.float64))
        near = (np.abs(ratio - (1.0 - CLIP)) < 1e-3) | (np.abs(ratio - (1.0 + CLIP)) < 1e-3)
        old[near] -= np.float32(0.01)
    c["action_log_probs"] = old.reshape(T, N, 1)
    vp, ret = np.zeros((T + 1, N, 1)), np.zeros((T + 1, N, 1))
    vp[:T] = (v + 0.25 * rng.standard_normal(T * N)).reshape(T, N, 1)     # (both sides of the value clip at 0.2)
    ret[:T] = (v + 0.7 * rng.standard_normal(T * N)).reshape(T, N, 1)
    c["value_preds"], c["returns"] = vp.astype(np.float32), ret.astype(np.float32)
    return c


# (O, K or n, H, T, N) of the GPU checks, per head, and what each reaches (tests/test_gpu_gru_discrete.py)
ANCHOR = (11, 3, 16, 5, 4)
COMMON = [ANCHOR, (11, 3, 16, 1, 16), (47, 18, 64, 8, 17), (13, 2, 100, 8, 17), (11, 17, 16, 27, 48)]
SHAPES = {CATEGORICAL: COMMON + [(13, 130, 20, 9, 33)], BERNOULLI: COMMON + [(13, 33, 20, 9, 33), (11, 1, 16, 5, 4)]}
UNCLIPPED = (ANCHOR, (47, 18, 64, 8, 17))                  # PPO with the unclipped value loss too
GW_SHAPES = {CATEGORICAL: ((13, 130, 20, 9, 33), ANCHOR), BERNOULLI: (ANCHOR,)}
DEAD_ENV_CASE = ((11, 3, 32, 8, 17), 5)                     # environment 5 never leaves its reset
DIST_NAME = {CATEGORICAL: "cat", BERNOULLI: "ber"}


def tag(dist, shape, extra=""):
    return DIST_NAME[dist] + " " + "x".join(map(str, shape)) + (" " + extra if extra else "")


# ------------------------------------------------------------------------------------------- the reference's own modules
TIER2 = [(CATEGORICAL, (11, 3, 16, 5, 4)), (BERNOULLI, (11, 3, 16, 5, 4)), (CATEGORICAL, (13, 17, 20, 9, 6))]


def tier2():
    """Only where the reference checkout is present, in a process of its own (tools/ref_import.py): the reference's Policy with
    base_kwargs={'recurrent': True} on Discrete / MultiBinary after .double(), updated by its own PPO (both value losses) and
    A2C_ACKTR; the .grad they leave against this file at tests/autograd_ref.py's BOUND.  Nothing of the reference is copied: it is
    imported.  -> {label: dict(worst_block, worst, loss_error)}"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (root, os.path.join(root, "tools"), os.path.join(root, "tests")):
        if path not in sys.path:
            sys.path.insert(0, path)
    cases = [random_case(dist, *shape) for dist, shape in TIER2]
    from ref_import import import_reference
    ns = import_reference()
    from third_party.a2c_ppo_acktr.algo.a2c_acktr import A2C_ACKTR
    out = {}

    def setup(c):
        sp = dr.space(c["dist"], c["K"])
        policy = ns.Policy((c["O"],), sp, base_kwargs={"recurrent": True, "hidden_size": c["H"]}).double()
        sd = {k: v.detach().clone() for k, v in ar.leaves(c["params"], param_shapes(c["O"], c["K"], c["H"])).items()}
        assert list(policy.state_dict()) == list(sd), (list(policy.state_dict()), list(sd))
        policy.load_state_dict(sd)
        ro = ns.RolloutStorage(c["T"], c["N"], (c["O"],), sp, c["H"], 1)
        for name in ("obs", "value_preds", "returns", "action_log_probs", "masks"):
            setattr(ro, name, ar.t64(c[name]))
        ro.actions = torch.as_tensor(c["actions"]) if c["dist"] == CATEGORICAL else ar.t64(c["actions"])
        ro.obs_feat, ro.recurrent_hidden_states = ro.obs_feat.double(), ro.recurrent_hidden_states.double()
        ro.recurrent_hidden_states[0] = ar.t64(c["hxs0"])
        return policy, ro

    def record(label, c, policy, g, la, losses):
        got = np.concatenate([q.grad.reshape(-1).numpy() for q in policy.parameters()])
        e = block_errors(g, got, c["O"], c["K"], c["H"])
        worst = max(e, key=e.get)
        out[label] = dict(worst_block=worst, worst=e[worst], loss_error=float(np.max(np.abs(np.asarray(la) - np.asarray(losses, np.float64)))))

    for c, (dist, shape) in zip(cases, TIER2):
        for uc in (True, False):
            policy, ro = setup(c)
            losses = ns.PPO(policy, CLIP, 1, 1, VCOEF, ECOEF, lr=3e-4, eps=1e-5, max_grad_norm=1e9, use_clipped_value_loss=uc).update(ro)
            g, la = ppo_grad(c, uc, adv_eps=1e-5)
            record(tag(dist, shape, "ppo " + ("clipped" if uc else "plain")), c, policy, g, la, losses)
        policy, ro = setup(c)
        losses = A2C_ACKTR(policy, VCOEF, ECOEF, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=1e9).update(ro)
        g, la = a2c_grad(c)
        record(tag(dist, shape, "a2c"), c, policy, g, la, losses)
    return out


if __name__ == "__main__":     # `--tier2` prints tier 2 (the child process of tests/test_gru_discrete_host.py)
    import json
    import sys
    if "--tier2" in sys.argv:
        print("TIER2 " + json.dumps(tier2()))
