"""Generate tests/golden/a2c_gru_*.npz by running the reference's A2C_ACKTR(acktr=False) on a recurrent Policy (dev-only).

Drives the reference's own A2C_ACKTR (a2c/algo/a2c_acktr.py:55-102) over Policy(..., base_kwargs={'recurrent': True})
(a2c/model.py:117-201) through tools/ref_import.py on the CPU, as a2c/main.py:123-131 builds it with --recurrent-policy, and
saves the inputs, the parameters before and after every update, RMSprop's square_avg and the loss triple.  Helpers and
conventions are tools/gen_golden_recurrent.py's: the rollout is filled act -> insert with episode ends inside it (8 % zero
masks), the policy is perturbed after its rollout is collected.  Every case has a zero mask in slot 0 and a non-zero
recurrent_hidden_states[0] (a rollout in the middle of training: after_update() carries both over).  Only data is committed.
Re-run:
    python tools/gen_golden_a2c_recurrent.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the reference and hooks torch.randperm)
import gen_golden_recurrent as ggr  # noqa: E402
from gen_golden_a2c import square_avg  # noqa: E402
from third_party.a2c_ppo_acktr.algo.a2c_acktr import A2C_ACKTR  # noqa: E402  (the reference's, via ref_import)

ns = gg.ns
EPS, ALPHA, VCOEF, ECOEF = 1e-5, 0.99, 0.5, 0.01   # a2c/arguments.py defaults


def rollout_mid_training(p, T, N, O, A, H, seed):
    """ggr.rollout_gru from a slot 0 that a previous rollout left behind: a non-zero hidden state, and masks[0] with zeros."""
    ro = ns.RolloutStorage(T, N, (O,), ns.Box(shape=(A,)), H, 1)
    g = torch.Generator().manual_seed(seed)
    ro.obs[0].copy_(torch.randn(N, O, generator=g))
    ro.recurrent_hidden_states[0].copy_(0.5 * torch.randn(N, H, generator=g))
    m0 = (torch.rand(N, 1, generator=g) > 0.08).float()
    if m0.min() > 0:
        m0[N // 2] = 0.0
    ro.masks[0].copy_(m0)
    for step in range(T):
        with torch.no_grad():
            value, action, logp, hxs = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
        obs = torch.randn(N, O, generator=g)
        reward = torch.randn(N, 1, generator=g)
        masks = (torch.rand(N, 1, generator=g) > 0.08).float()
        bad = (torch.rand(N, 1, generator=g) > 0.03).float()
        ro.insert(obs, hxs, action, logp, value, reward, masks, bad, torch.zeros(N, 1))
    if T > 2 and ro.masks[1:-1].min() > 0:
        ro.masks[T // 2, 0] = 0.0
    with torch.no_grad():
        nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    return ro


def gen_a2c_gru(name, O, A, H, T, N, seed, iters=1, num_updates=10, lr=7e-4, max_grad_norm=0.5, pert=0.02):
    p = ggr.make_gru_policy(O, A, H, seed)
    agent = A2C_ACKTR(p, VCOEF, ECOEF, lr=lr, eps=EPS, alpha=ALPHA, max_grad_norm=max_grad_norm)
    out, lrs, norms = {}, [], []
    for j in range(iters):
        if iters > 1:
            ns.a2c_utils.update_linear_schedule(agent.optimizer, j, num_updates, lr)   # a2c/main.py:201-205
        lrs.append(agent.optimizer.param_groups[0]["lr"])
        torch.manual_seed(seed + 10 + j)
        ro = rollout_mid_training(p, T, N, O, A, H, seed + 20 + 2 * j)
        pre = "" if iters == 1 else f"it{j}_"
        assert float(ro.masks[0].min()) == 0.0 and float(ro.recurrent_hidden_states[0].abs().max()) > 0.0
        if j == 0:   # the initial parameters, once: every later update starts from the one before it
            gg.perturb(p, pert, seed + 21)   # values != value_preds: the update must evaluate the current parameters
            out["params0"] = gg.flat_params(p)
        for k, v in gg.rollout_arrays(ro).items():
            if k in ("obs", "actions", "returns", "value_preds", "action_log_probs", "masks"):
                out[pre + k] = v
        out[pre + "hxs0"] = ro.recurrent_hidden_states[0].numpy().copy()
        clip = torch.nn.utils.clip_grad_norm_   # record the norm the clip measured (it scales the gradients in place)
        torch.nn.utils.clip_grad_norm_ = lambda *a, **k: norms.append(float(clip(*a, **k))) or norms[-1]
        try:
            vl, al, de = agent.update(ro)
        finally:
            torch.nn.utils.clip_grad_norm_ = clip
        assert len(norms) == j + 1
        out[pre + "params1"] = gg.flat_params(p)
        out[pre + "square_avg"] = square_avg(agent)
        out[pre + "losses"] = np.array([vl, al, de], np.float64)
    sd = p.state_dict()
    gg.save(name, meta=gg.meta(O=O, A=A, H=H, T=T, N=N, lr=lr, eps=EPS, alpha=ALPHA, value_loss_coef=VCOEF, entropy_coef=ECOEF,
                               max_grad_norm=max_grad_norm, iters=iters, num_updates=num_updates, grad_norms=norms,
                               names=list(sd.keys()), shapes=[list(t.shape) for t in sd.values()]),
            lrs=np.array(lrs, np.float64), **out)
    size = os.path.getsize(os.path.join(gg.OUT, name + ".npz"))
    assert size < 300 * 1024, (name, size)
    print(f"{name}: {iters} update(s), gradient norms {['%.3f' % q for q in norms]} (clip at {max_grad_norm}), {size / 1024:.0f} KiB")
    return norms


if __name__ == "__main__":
    # the gradient check: the clip inactive
    n = gen_a2c_gru("a2c_gru_onestep", O=11, A=3, H=16, T=5, N=4, seed=1200, max_grad_norm=1e3)
    assert max(n) < 1e3
    # three updates under linear LR decay, the clip active at 0.5
    n = gen_a2c_gru("a2c_gru_tiny", O=11, A=3, H=32, T=5, N=16, seed=1210, iters=3)
    assert min(n) > 0.5, n
    # three scan tiles, the last with one environment
    gen_a2c_gru("a2c_gru_ragged", O=13, A=5, H=20, T=9, N=33, seed=1220)
