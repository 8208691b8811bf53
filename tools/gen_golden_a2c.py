"""Generate tests/golden/a2c_*.npz by running the reference's A2C_ACKTR(acktr=False) (dev-only).

Drives the reference's own A2C_ACKTR (a2c/algo/a2c_acktr.py:30-102: RMSprop, clip_grad_norm_) through tools/ref_import.py on
CPU, as a2c/main.py:123-131 builds it, and saves the inputs, the parameters before and after the update, RMSprop's square_avg
and the loss triple.  The policy is perturbed after its rollout is collected (as tools/gen_golden.py's gen_ppo does), so the
values the update evaluates differ from the stored value_preds.  Re-run:
    python tools/gen_golden_a2c.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the reference and hooks torch.randperm)
from third_party.a2c_ppo_acktr.algo.a2c_acktr import A2C_ACKTR  # noqa: E402  (the reference's, via ref_import)

LR, EPS, ALPHA, VCOEF, ECOEF, MAXN = 3e-4, 1e-5, 0.99, 0.5, 0.01, 0.5   # a2c/arguments.py defaults


def square_avg(agent):
    st = agent.optimizer.state_dict()["state"]
    return np.concatenate([st[i]["square_avg"].numpy().reshape(-1) for i in range(len(st))]).astype(np.float32)


def fresh_rollout(p, T, N, O, A, seed, pert):
    ro = gg.rollout_from_policy(p, T, N, O, A, 1, seed, "mlp")
    with torch.no_grad():
        nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    gg.perturb(p, pert, seed + 1)   # values != value_preds: the update must evaluate the current parameters
    return ro


def gen_a2c(name, O, A, H, T, N, seed, critic64=False, iters=1, num_updates=10, lr=LR, pert=0.02):
    p = gg.make_policy("mlp", O, A, H, 1, seed)
    if critic64:
        torch.manual_seed(seed + 1)
        p.reset_critic((O,))                        # a2c/main.py:85: a 64-unit critic beside the H-wide actor
        with torch.no_grad():
            for q in p.parameters():
                q.add_(0.05 * torch.randn_like(q))
    agent = A2C_ACKTR(p, VCOEF, ECOEF, lr=lr, eps=EPS, alpha=ALPHA, max_grad_norm=MAXN)
    out, lrs = {}, []
    for j in range(iters):
        if iters > 1:
            gg.ns.a2c_utils.update_linear_schedule(agent.optimizer, j, num_updates, lr)   # a2c/main.py:201-205
        lrs.append(agent.optimizer.param_groups[0]["lr"])
        torch.manual_seed(seed + 10 + j)
        ro = fresh_rollout(p, T, N, O, A, seed + 20 + 2 * j, pert)
        pre = "" if iters == 1 else f"it{j}_"
        out[pre + "params0"] = gg.flat_params(p)
        for k, v in gg.rollout_arrays(ro).items():
            if k in ("obs", "actions", "returns", "value_preds", "action_log_probs", "masks"):
                out[pre + k] = v
        vl, al, de = agent.update(ro)
        out[pre + "params1"] = gg.flat_params(p)
        out[pre + "square_avg"] = square_avg(agent)
        out[pre + "losses"] = np.array([vl, al, de], np.float64)
    Hc = 64 if critic64 else H
    gg.save(name, meta=gg.meta(kind="mlp", O=O, A=A, H=H, Hc=Hc, T=T, N=N, lr=lr, eps=EPS, alpha=ALPHA, value_loss_coef=VCOEF,
                               entropy_coef=ECOEF, max_grad_norm=MAXN, iters=iters, num_updates=num_updates),
            lrs=np.array(lrs, np.float64), **out)


if __name__ == "__main__":
    gen_a2c("a2c_tiny", O=5, A=3, H=8, T=4, N=3, seed=800)
    gen_a2c("a2c_default", O=47, A=12, H=64, T=5, N=16, seed=810)
    gen_a2c("a2c_critic64", O=20, A=6, H=100, T=5, N=8, seed=820, critic64=True)
    gen_a2c("a2c_multi", O=11, A=3, H=16, T=5, N=6, seed=830, iters=3, num_updates=10, lr=7e-4)
