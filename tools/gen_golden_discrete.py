"""Generate tests/golden/discrete_*.npz and ckpt_policy_{categorical,bernoulli}.pt by running the reference's Policy on
Discrete / MultiBinary action spaces (dev-only).

Drives the reference's own Policy (a2c/model.py:52-62: Categorical on Discrete, Bernoulli on MultiBinary), RolloutStorage
(a2c/storage.py:42-48: int64 actions [T, N, 1] for Discrete), PPO and A2C_ACKTR(acktr=False) through tools/ref_import.py on the
CPU, with duck-typed action spaces (the reference reads only the class name, .n and .shape).  Per case:
  * the rollout the reference's act() collected, then the policy perturbed (ratio != 1, values != value_preds): params0;
  * evaluate_actions on all T*N rows and the deterministic actions (the generator asserts that no two top logits, and no logit
    and 0, lie within 1e-4 of each other: the modes are then unambiguous in any float32 evaluation);
  * the reference's .grad of ONE PPO step over all rows and of one A2C step, both with the gradient clip out of reach
    (max_grad_norm = 1e9), PPO's with both use_clipped_value_loss settings;
  * a whole PPO update (E = 2, M = 2) with its recorded randperms, Adam's m / v, params1 and the loss triple; a whole A2C
    update with RMSprop's square_avg.
Re-run:
    python tools/gen_golden_discrete.py
"""
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the reference and hooks torch.randperm)
from third_party.a2c_ppo_acktr.algo.a2c_acktr import A2C_ACKTR  # noqa: E402  (the reference's, via ref_import)

ns = gg.ns
CLIP, VCOEF, ECOEF, LR, EPS, ALPHA, MAXN = 0.2, 0.5, 0.01, 3e-4, 1e-5, 0.99, 0.5
E, M = 2, 2


class Discrete:
    def __init__(self, n):
        self.n = int(n)


class MultiBinary:
    def __init__(self, n):
        self.n, self.shape = int(n), (int(n),)


def make_policy(space, O, H, seed):
    torch.manual_seed(seed)
    p = ns.Policy((O,), space, base_kwargs={"recurrent": False, "hidden_size": H})
    with torch.no_grad():   # Categorical's head starts at gain 0.01: move everything so that the logits differ between classes
        for name, q in p.named_parameters():
            q.add_((0.6 if name.startswith("dist.") else 0.05) * torch.randn_like(q))
    return p


def collect(p, space, T, N, O, seed):
    ro = ns.RolloutStorage(T, N, (O,), space, 1, 1)
    g = torch.Generator().manual_seed(seed)
    ro.obs[0].copy_(torch.randn(N, O, generator=g))
    for step in range(T):
        with torch.no_grad():
            value, action, logp, hxs = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
        ro.insert(torch.randn(N, O, generator=g), hxs, action, logp, value, torch.randn(N, 1, generator=g),
                  (torch.rand(N, 1, generator=g) > 0.08).float(), (torch.rand(N, 1, generator=g) > 0.03).float(),
                  torch.randn(N, 1, generator=g))
    with torch.no_grad():
        nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    return ro


def grads(p):
    return np.concatenate([q.grad.numpy().reshape(-1) for q in p.parameters()]).astype(np.float32)


def opt_state(agent, key):
    st = agent.optimizer.state_dict()["state"]
    return np.concatenate([st[i][key].numpy().reshape(-1) for i in range(len(st))]).astype(np.float32)


def gen(name, space, O, H, T, N, seed):
    K = space.n
    categorical = type(space).__name__ == "Discrete"
    p = make_policy(space, O, H, seed)
    assert [k for k, _ in p.named_parameters()][-2:] == ["dist.linear.weight", "dist.linear.bias"]
    torch.manual_seed(seed + 5)
    ro = collect(p, space, T, N, O, seed + 6)
    assert ro.actions.dtype == (torch.int64 if categorical else torch.float32) and tuple(ro.actions.shape) == (T, N, 1 if categorical else K)
    gg.perturb(p, 0.03, seed + 7)
    out = dict(params0=gg.flat_params(p))
    for k, v in gg.rollout_arrays(ro).items():
        if k in ("obs", "actions", "returns", "value_preds", "action_log_probs", "masks"):
            out[k] = v
    rows = ro.obs[:-1].reshape(T * N, O)
    with torch.no_grad():
        ev, elp, eent, _ = p.evaluate_actions(rows, None, None, ro.actions.reshape(T * N, -1))
        _, det, det_lp, _ = p.act(rows, None, None, deterministic=True)
        logits = p.dist.linear(p.base(rows, None, None)[1])
    top = torch.sort(logits, dim=1).values
    margin = float((top[:, -1] - top[:, -2]).min()) if categorical else float(logits.abs().min())
    assert margin > 1e-4, f"{name}: a deterministic action hangs on {margin:.2e} between logits"
    assert det.dtype == (torch.int64 if categorical else torch.float32)
    out.update(eval_value=ev.numpy(), eval_logp=elp.numpy(), eval_entropy=np.float32(eent.item()), det_action=det.numpy(),
               det_logp=det_lp.numpy(), logits=logits.numpy(), mode_margin=np.float64(margin))
    # the reference's .grad of one step over all rows, the clip out of reach
    for key, uc in (("grad_ppo_clipped", True), ("grad_ppo_plain", False)):
        q = copy.deepcopy(p)
        agent = ns.PPO(q, CLIP, 1, 1, VCOEF, ECOEF, lr=LR, eps=EPS, max_grad_norm=1e9, use_clipped_value_loss=uc)
        torch.manual_seed(seed + 8)
        losses = agent.update(ro)
        out[key] = grads(q)
        out[key.replace("grad", "losses")] = np.array(losses, np.float64)
    q = copy.deepcopy(p)
    agent = A2C_ACKTR(q, VCOEF, ECOEF, lr=LR, eps=EPS, alpha=ALPHA, max_grad_norm=1e9)
    out["losses_a2c_grad"] = np.array(agent.update(ro), np.float64)
    out["grad_a2c"] = grads(q)
    # whole updates
    q = copy.deepcopy(p)
    agent = ns.PPO(q, CLIP, E, M, VCOEF, ECOEF, lr=LR, eps=EPS, max_grad_norm=MAXN)
    gg._REC.clear()
    torch.manual_seed(seed + 9)
    out["ppo_losses"] = np.array(agent.update(ro), np.float64)
    out["perms"] = np.stack([r for k, r in gg._REC if k == "randperm"]).astype(np.int64)
    assert out["perms"].shape == (E, T * N)
    out.update(ppo_params1=gg.flat_params(q), adam_m=opt_state(agent, "exp_avg"), adam_v=opt_state(agent, "exp_avg_sq"))
    q = copy.deepcopy(p)
    agent = A2C_ACKTR(q, VCOEF, ECOEF, lr=LR, eps=EPS, alpha=ALPHA, max_grad_norm=MAXN)
    out["a2c_losses"] = np.array(agent.update(ro), np.float64)
    out.update(a2c_params1=gg.flat_params(q), square_avg=opt_state(agent, "square_avg"))
    gg.save(name, meta=gg.meta(dist="categorical" if categorical else "bernoulli", O=O, K=K, H=H, T=T, N=N, ppo_epoch=E, num_mini_batch=M,
                               clip_param=CLIP, value_loss_coef=VCOEF, entropy_coef=ECOEF, lr=LR, eps=EPS, alpha=ALPHA,
                               max_grad_norm=MAXN), **out)
    size = os.path.getsize(os.path.join(gg.OUT, name + ".npz"))
    assert size < 300 * 1024, f"{name}.npz is {size} bytes: fixtures stay under 300 KiB"


def gen_checkpoints():
    """One whole-module checkpoint per distribution, as the reference's torch.save([actor_critic, ob_rms]) writes it (legacy
    container, without the classes' source text)."""
    g = torch.Generator().manual_seed(91)
    for tag, space, seed in (("categorical", Discrete(6), 900), ("bernoulli", MultiBinary(4), 910)):
        p = make_policy(space, 9, 16, seed)
        path = os.path.join(gg.OUT, f"ckpt_policy_{tag}.pt")
        gg.save_legacy_without_source([p, None], path)
        blob = open(path, "rb").read()
        for needle in (b"class Categorical", b"class Bernoulli", b"class FixedCategorical", b"import torch"):
            assert needle not in blob, f"{path} embeds reference source ({needle!r})"
        obs = torch.randn(7, 9, generator=g)
        with torch.no_grad():
            v, a, lp, _ = p.act(obs, None, None, deterministic=True)
        gg.save(f"ckpt_policy_{tag}", meta=gg.meta(dist=tag, O=9, K=space.n, H=16, names=[k for k, _ in p.named_parameters()]),
                flat=gg.flat_params(p), obs=obs.numpy(), value=v.numpy(), action=a.numpy(), logp=lp.numpy())


if __name__ == "__main__":
    gen("discrete_k2", Discrete(2), O=4, H=16, T=8, N=4, seed=1000)
    gen("discrete_k17", Discrete(17), O=11, H=32, T=11, N=7, seed=1010)
    gen("discrete_k130", Discrete(130), O=20, H=24, T=8, N=8, seed=1020)
    gen("discrete_b1", MultiBinary(1), O=4, H=16, T=8, N=4, seed=1030)
    gen("discrete_b5", MultiBinary(5), O=11, H=32, T=11, N=7, seed=1040)
    gen("discrete_b33", MultiBinary(33), O=20, H=32, T=8, N=8, seed=1050)
    gen_checkpoints()
