"""Generate tests/golden/gru_cat_*.npz, gru_ber_*.npz and ckpt_policy_gru_cat.* by running the reference on a recurrent Policy
with a Categorical / Bernoulli head (dev-only).

Drives the reference's own Policy((O,), Discrete(K) | MultiBinary(n), base_kwargs={'recurrent': True}) (a2c/model.py:40-62,
117-201) with PPO (a2c/algo/ppo.py, 2 epochs x 2 minibatches over recurrent_generator) and A2C_ACKTR(acktr=False)
(a2c/algo/a2c_acktr.py:55-102, one update) through tools/ref_import.py on the CPU, in the manner of tools/gen_golden_recurrent.py
and tools/gen_golden_a2c_recurrent.py: the rollout is filled act -> insert with episode ends inside it, slot 0 carries a zero mask
and a non-zero hidden state, the policy is perturbed after its rollout is collected.  Only data is committed.  Re-run:
    python tools/gen_golden_gru_discrete.py
"""
import copy
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


class Discrete:
    """Duck-typed gym.spaces.Discrete: the hot path reads __class__.__name__ and .n (a2c/model.py:52-54, a2c/storage.py:42-43)"""

    def __init__(self, n):
        self.n = int(n)


class MultiBinary:
    """Duck-typed gym.spaces.MultiBinary: __class__.__name__ and .shape (a2c/model.py:58-60, a2c/storage.py:44-45)"""

    def __init__(self, n):
        self.n, self.shape = int(n), (int(n),)


def space(dist, K):
    return Discrete(K) if dist == "cat" else MultiBinary(K)


def make_policy(dist, O, K, H, seed):
    torch.manual_seed(seed)
    p = ns.Policy((O,), space(dist, K), base_kwargs={"recurrent": True, "hidden_size": H})
    with torch.no_grad():   # non-zero biases everywhere; logits that tell the classes apart (the Categorical init has gain 0.01)
        for name, q in p.named_parameters():
            q.add_((0.5 if name.startswith("dist.") else 0.05) * torch.randn_like(q))
    return p


def rollout_mid_training(p, dist, T, N, O, K, H, seed):
    """act -> insert from a slot 0 that a previous rollout left behind: a non-zero hidden state, masks[0] with zeros"""
    ro = ns.RolloutStorage(T, N, (O,), space(dist, K), H, 1)
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


def arrays(ro):
    out = {k: v for k, v in gg.rollout_arrays(ro).items() if k in ("obs", "actions", "returns", "value_preds", "action_log_probs", "masks")}
    out["hxs0"] = ro.recurrent_hidden_states[0].numpy().copy()
    return out


def shapes_meta(p):
    sd = p.state_dict()
    return dict(names=list(sd.keys()), shapes=[list(t.shape) for t in sd.values()])


def finish(name):
    size = os.path.getsize(os.path.join(gg.OUT, name + ".npz"))
    assert size < 300 * 1024, (name, size)


def gen_ppo(name, dist, O, K, H, T, N, E, M, clip, lr, seed, pert=0.05):
    p = make_policy(dist, O, K, H, seed)
    torch.manual_seed(seed + 5)
    ro = rollout_mid_training(p, dist, T, N, O, K, H, seed + 6)
    gg.perturb(p, pert, seed + 7)
    params0 = gg.flat_params(p)
    p64, ro64 = copy.deepcopy(p).double(), copy.deepcopy(ro)
    for k, v in vars(ro64).items():
        if torch.is_tensor(v) and v.dtype == torch.float32:
            setattr(ro64, k, v.double())
    agent = ns.PPO(p, clip, E, M, VCOEF, ECOEF, lr=lr, eps=EPS, max_grad_norm=0.5)
    arrs = arrays(ro)
    gg._REC.clear()
    torch.manual_seed(seed + 8)
    vl, al, de = agent.update(ro)
    perms = np.stack([r for k, r in gg._REC if k == "randperm"]).astype(np.int64)
    assert perms.shape == (E, N)
    steps = E * (N // (N // M))
    assert int(agent.optimizer.state_dict()["state"][0]["step"]) == steps
    adv = ro.returns[:-1] - ro.value_preds[:-1]
    adv = (adv - adv.mean()) / (adv.std() + 1e-5)
    m, v = ggr.adam_state(agent)
    # the same update by the reference in float64 with the permutations replayed: its float32 rounding uses under a tenth of the
    # tolerances the tests apply
    replay = [torch.from_numpy(q.copy()) for q in perms]
    rp = torch.randperm
    torch.randperm = lambda n, *a_, **k_: replay.pop(0)
    try:
        l64 = ns.PPO(p64, clip, E, M, VCOEF, ECOEF, lr=lr, eps=EPS, max_grad_norm=0.5).update(ro64)
    finally:
        torch.randperm = rp
    p1_64 = np.concatenate([q.detach().numpy().reshape(-1) for q in p64.state_dict().values()])
    r = (ggr.within_tenth(gg.flat_params(p).astype(np.float64), p1_64, name + " params"), ggr.within_tenth([vl, al, de], l64, name + " losses"))
    print(f"{name}: {steps} optimizer steps; float32 vs float64 / tolerance: params {r[0]:.4f}, losses {r[1]:.4f}")
    gg.save(name, meta=gg.meta(dist=dist, O=O, K=K, H=H, T=T, N=N, ppo_epoch=E, num_mini_batch=M, steps=steps, clip_param=clip,
                               entropy_coef=ECOEF, lr=lr, eps=EPS, value_loss_coef=VCOEF, max_grad_norm=0.5, **shapes_meta(p)),
            params0=params0, perms=perms, advantages=adv.numpy(), losses=np.array([vl, al, de], np.float64), params1=gg.flat_params(p),
            adam_m=m, adam_v=v, **arrs)
    finish(name)


def gen_a2c(name, dist, O, K, H, T, N, seed, lr=7e-4, max_grad_norm=0.5, pert=0.05):
    p = make_policy(dist, O, K, H, seed)
    agent = A2C_ACKTR(p, VCOEF, ECOEF, lr=lr, eps=EPS, alpha=ALPHA, max_grad_norm=max_grad_norm)
    torch.manual_seed(seed + 10)
    ro = rollout_mid_training(p, dist, T, N, O, K, H, seed + 20)
    gg.perturb(p, pert, seed + 21)
    params0 = gg.flat_params(p)
    arrs = arrays(ro)
    norms = []
    clip = torch.nn.utils.clip_grad_norm_   # record the norm the clip measured
    torch.nn.utils.clip_grad_norm_ = lambda *a, **k: norms.append(float(clip(*a, **k))) or norms[-1]
    try:
        vl, al, de = agent.update(ro)
    finally:
        torch.nn.utils.clip_grad_norm_ = clip
    gg.save(name, meta=gg.meta(dist=dist, O=O, K=K, H=H, T=T, N=N, lr=lr, eps=EPS, alpha=ALPHA, value_loss_coef=VCOEF, entropy_coef=ECOEF,
                               max_grad_norm=max_grad_norm, grad_norms=norms, **shapes_meta(p)),
            params0=params0, params1=gg.flat_params(p), square_avg=square_avg(agent), losses=np.array([vl, al, de], np.float64), **arrs)
    finish(name)
    print(f"{name}: gradient norm {norms[0]:.3f} (clip at {max_grad_norm})")


def gen_ckpt():
    """[actor_critic, ob_rms] of a recurrent Categorical policy in the legacy container (class names and data, no source text)"""
    O, K, H, n = 7, 5, 16, 6
    p = make_policy("cat", O, K, H, 2300)
    rms = ns.RunningMeanStd(shape=(O,))
    rms.update(np.random.RandomState(4).randn(40, O) * 1.5 - 0.25)
    path = os.path.join(gg.OUT, "ckpt_policy_gru_cat.pt")
    gg.save_legacy_without_source([p, rms], path)
    blob = open(path, "rb").read()
    for needle in (b"class NNBase", b"class GRU", b"def _forward_gru", b"class Categorical"):
        assert needle not in blob, f"{path} embeds source ({needle!r})"
    g = torch.Generator().manual_seed(2301)
    obs, hxs = torch.randn(n, O, generator=g), 0.5 * torch.randn(n, H, generator=g)
    masks = ggr.masks_with_zeros((n, 1), g, 0.3)
    with torch.no_grad():
        v, a, lp, h = p.act(obs, hxs, masks, deterministic=True)
        logits = p.dist(p.base(obs, hxs, masks)[1]).logits
    top = torch.sort(logits, dim=1).values
    assert float((top[:, -1] - top[:, -2]).min()) > 1e-3, "the mode must not hang on rounding"
    gg.save("ckpt_policy_gru_cat", meta=gg.meta(O=O, K=K, H=H, **shapes_meta(p)), flat=gg.flat_params(p), obs=obs.numpy(), hxs=hxs.numpy(),
            masks=masks.numpy(), value=v.numpy(), action=a.numpy(), logp=lp.numpy(), hxs_out=h.numpy(), rms_mean=rms.mean,
            rms_var=rms.var, rms_count=np.float64(rms.count))
    print(f"ckpt_policy_gru_cat.pt: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    # two scan tiles (N = 24), K / n beyond one 16-column tile, T beyond one 8-step chunk; 2 epochs x 2 minibatches of 12 environments
    gen_ppo("gru_cat_ppo", "cat", O=11, K=17, H=32, T=10, N=24, E=2, M=2, clip=0.2, lr=3e-4, seed=2100)
    gen_ppo("gru_ber_ppo", "ber", O=11, K=5, H=32, T=10, N=24, E=2, M=2, clip=0.2, lr=3e-4, seed=2110)
    gen_a2c("gru_cat_a2c", "cat", O=13, K=6, H=20, T=9, N=33, seed=2200)       # three scan tiles, the last with one environment
    gen_a2c("gru_ber_a2c", "ber", O=13, K=17, H=20, T=9, N=33, seed=2210)
    gen_ckpt()
