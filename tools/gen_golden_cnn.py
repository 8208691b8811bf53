"""Generate tests/golden/policy_cnn_*.npz, ppo_cnn_*.npz and ckpt_policy_cnn.{pt,npz} by running the reference's Policy on image
observations (dev-only).

Drives the reference's own Policy with its CNNBase (a2c/model.py:204-230, picked for a 3-D obs_shape at :42-46), RolloutStorage and
PPO through tools/ref_import.py on the CPU, with duck-typed action spaces.  Everything written is data: weights, observations as
uint8, injected noise, and the results of act / get_value / evaluate_actions / PPO.update.
  * policy_cnn_<tag>: params, obs (uint8), the three calls' results on the first n rows for every n of NS (the entropy is a mean
    over the call's rows), the deterministic actions (no two top logits within 1e-4), and for the sampled action
      - Box: the normal draws the reference's act() consumed (action = mean + std * noise, checked), with its action and log-prob;
      - Discrete: as tools/gen_golden_discrete.py: torch's multinomial draw has no uniform to inject, so the fixture carries the
        reference's logits and `uniform` draws that keep 1e-4 clear of every cumulative boundary; the library's convention (first
        class whose running probability sum exceeds u) decides the class, evaluate_actions of the reference gives its log-prob.
  * ppo_cnn_<tag>: a 4 x 4 rollout collected by the reference's act(), the policy perturbed (ratio != 1), the recorded randperms,
    the loss triple and -- in ppo_cnn_<tag>_params1 -- the parameters after PPO.update with E = 2, M = 2.
  * ckpt_policy_cnn.pt: torch.save([actor_critic, None]) in the legacy container without the classes' source text, with the
    policy's deterministic act() on 7 rows beside it.
Every float32 result is asserted to lie within a tenth of the tests' tolerance of tests/cnn_ref.py's float64 evaluation of the same
thing (for the whole update: seeds are tried in order until that holds -- a ReLU unit within rounding of zero in one of the four
steps takes the float32 run off the float64 one, which says nothing about either).
Re-run:
    python tools/gen_golden_cnn.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import gen_golden as gg  # noqa: E402  (imports the reference and hooks torch.randperm)
import cnn_ref as cr     # noqa: E402

ns = gg.ns
HW = 84
CLIP, VCOEF, ECOEF, LR, EPS, MAXN = cr.CLIP, cr.VCOEF, cr.ECOEF, cr.LR, cr.EPS, 0.5
E, M = 2, 2
LIMIT = 860 * 1024   # the largest fixture before this generator


class Discrete:
    def __init__(self, n):
        self.n = int(n)


def space_of(dist, P):
    return Discrete(P) if dist == "categorical" else ns.Box(shape=(P,))


def make_policy(C, Hs, dist, P, seed):
    torch.manual_seed(seed)
    p = ns.Policy((C, HW, HW), space_of(dist, P), base_kwargs={"hidden_size": Hs})
    assert type(p.base).__name__ == "CNNBase"
    with torch.no_grad():   # biases off zero, the Categorical head (gain 0.01) far enough for distinct logits
        for name, q in p.named_parameters():
            q.add_((0.6 if name.startswith("dist.linear") else 0.02) * torch.randn_like(q))
    assert [(k, tuple(v.shape)) for k, v in p.state_dict().items()] == cr.param_shapes(C, Hs, dist, P)
    return p


def tenth(got, ref, what):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    r = float(np.max(np.abs(got - ref) / (cr.ATOL + cr.RTOL * np.abs(ref))))
    assert r <= 0.1, f"{what}: the reference's float32 result is {r:.3f} of the tolerance from float64"
    return r


def images(g, shape, levels=256):
    step = 255 // (levels - 1)
    return (torch.randint(0, levels, shape, generator=g) * step).to(torch.uint8)


def gen_policy(tag, C, Hs, dist, P, NS, seed, levels=256):
    p = make_policy(C, Hs, dist, P, seed)
    shapes = cr.param_shapes(C, Hs, dist, P)
    params = gg.flat_params(p)
    g = torch.Generator().manual_seed(seed + 1)
    n = max(NS)
    obs8 = images(g, (n, C, HW, HW), levels)
    obs = obs8.float()
    out = dict(params=params, obs=obs8.numpy())
    with torch.no_grad():
        gv = p.get_value(obs, None, None)
        v_det, a_det, lp_det, _ = p.act(obs, None, None, deterministic=True)
        feat = p.base(obs, None, None)[1]
    f64 = cr.forward64(shapes, params, obs.numpy(), dist)
    tenth(gv.numpy(), f64[0], f"{tag} value")
    d64 = cr.act64(shapes, params, obs.numpy(), dist)
    out.update(get_value=gv.numpy(), det_action=a_det.numpy(), det_logp=lp_det.numpy())
    tenth(lp_det.numpy(), d64["logp"], f"{tag} det logp")
    if dist == "categorical":
        with torch.no_grad():
            logits = p.dist.linear(feat)
        assert d64["margin"] > 1e-4 and np.array_equal(a_det.numpy().reshape(-1), d64["action"])
        u = torch.rand(n, generator=g).numpy().astype(np.float32)
        act, margin = cr.categorical_sample(f64[1], u)
        assert margin > 1e-4, f"{tag}: a uniform draw lies {margin:.2e} from a cumulative boundary"
        ref_act = torch.as_tensor(act.reshape(n, 1))
        out.update(logits=logits.numpy(), uniform=u, act_action=act.reshape(n, 1).astype(np.int64))
    else:
        with torch.no_grad():
            torch.manual_seed(seed + 2)
            value, action, logp, _ = p.act(obs, None, None)
            torch.manual_seed(seed + 2)
            noise = torch.randn(n, P)    # the stream torch.normal(mean, std) consumed
            d = p.dist(feat)
            if not torch.allclose(d.mean + d.stddev * noise, action, rtol=0, atol=1e-6):
                noise = (action - d.mean) / d.stddev
        a64 = cr.act64(shapes, params, obs.numpy(), dist, noise.numpy())
        tenth(action.numpy(), a64["action"], f"{tag} sampled action")
        out.update(noise=noise.numpy(), act_action=action.numpy(), act_logp=logp.numpy(), act_value=value.numpy())
        ref_act = action + 0.3 * torch.randn(n, P, generator=g)
    out["eval_action"] = ref_act.numpy()
    for k in NS:
        with torch.no_grad():
            ev, elp, eent, _ = p.evaluate_actions(obs[:k], None, None, ref_act[:k])
            v64, lp64, ent64 = cr.evaluate(cr.leaves(params, shapes), cr.ar.t64(obs[:k].numpy()), ref_act[:k].numpy(), dist)
        tenth(ev.numpy(), v64.numpy(), f"{tag} eval value n={k}")
        tenth(elp.numpy(), lp64.numpy(), f"{tag} eval logp n={k}")
        tenth(eent.numpy(), ent64.numpy(), f"{tag} entropy n={k}")
        out[f"eval_entropy_{k}"] = np.float32(eent.item())
        if k == n:
            out.update(eval_value=ev.numpy(), eval_logp=elp.numpy())
    name = f"policy_cnn_{tag}"
    gg.save(name, meta=gg.meta(C=C, Hs=Hs, dist=dist, P=P, NS=list(NS)), **out)
    assert os.path.getsize(os.path.join(gg.OUT, name + ".npz")) <= LIMIT, name


def collect(p, dist, P, C, T, N, seed):
    ro = ns.RolloutStorage(T, N, (C, HW, HW), space_of(dist, P), 1, 1)
    g = torch.Generator().manual_seed(seed)
    ro.obs[0].copy_(images(g, (N, C, HW, HW)).float())
    for step in range(T):
        with torch.no_grad():
            value, action, logp, hxs = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
        ro.insert(images(g, (N, C, HW, HW)).float(), hxs, action, logp, value, torch.randn(N, 1, generator=g),
                  (torch.rand(N, 1, generator=g) > 0.08).float(), (torch.rand(N, 1, generator=g) > 0.03).float(),
                  torch.randn(N, 1, generator=g))
    with torch.no_grad():
        nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    return ro


def gen_ppo(tag, C, Hs, dist, P, T, N, seed0):
    shapes = cr.param_shapes(C, Hs, dist, P)
    for seed in range(seed0, seed0 + 40):
        p = make_policy(C, Hs, dist, P, seed)
        torch.manual_seed(seed + 5)
        ro = collect(p, dist, P, C, T, N, seed + 6)
        gg.perturb(p, 0.01, seed + 7)
        params0 = gg.flat_params(p)
        q = copy.deepcopy(p)
        agent = ns.PPO(q, CLIP, E, M, VCOEF, ECOEF, lr=LR, eps=EPS, max_grad_norm=MAXN)
        gg._REC.clear()
        torch.manual_seed(seed + 9)
        losses = np.array(agent.update(ro), np.float64)
        perms = np.stack([r for k, r in gg._REC if k == "randperm"]).astype(np.int64)
        assert perms.shape == (E, T * N)
        params1 = gg.flat_params(q)
        arrs = gg.rollout_arrays(ro)
        c = cr.Case(C=C, T=T, N=N, dist=dist, params=params0, obs=arrs["obs"], actions=arrs["actions"], action_log_probs=arrs["action_log_probs"],
                    value_preds=arrs["value_preds"], returns=arrs["returns"])
        l64, p64, _ = cr.adam_update64(shapes, c, perms, E, M, MAXN)
        # Adam's step is lr * m / (sqrt(v) + eps): after 4 steps every element has moved by about 4 lr whatever its gradient, so the
        # distance that counts is the one assert_close_adam measures; a tenth of it
        err = np.abs(params1.astype(np.float64) - p64)
        bad = err > 0.1 * (cr.ATOL + cr.RTOL * np.abs(p64))
        lr_ = float(np.max(np.abs(losses - l64) / (cr.ATOL + cr.RTOL * np.abs(l64))))
        print(f"ppo_cnn_{tag} seed {seed}: losses {lr_:.3f} of tol, {int(bad.sum())}/{bad.size} parameters past a tenth, max err {err.max():.2e}")
        if lr_ <= 0.1 and bad.sum() <= max(1, int(5e-4 * bad.size)) and err.max() <= LR * E * M:   # assert_close_adam's outlier rule, at a tenth of its tolerance
            break
    else:
        raise RuntimeError(f"ppo_cnn_{tag}: no seed whose float32 update stays with the float64 one")
    keep = {k: arrs[k] for k in ("actions", "returns", "value_preds", "action_log_probs", "masks")}
    assert np.array_equal(arrs["obs"], arrs["obs"].astype(np.uint8))
    gg.save(f"ppo_cnn_{tag}", meta=gg.meta(C=C, Hs=Hs, dist=dist, P=P, T=T, N=N, ppo_epoch=E, num_mini_batch=M, clip_param=CLIP,
                                          value_loss_coef=VCOEF, entropy_coef=ECOEF, lr=LR, eps=EPS, max_grad_norm=MAXN, seed=seed),
            params0=params0, obs=arrs["obs"].astype(np.uint8), perms=perms, ppo_losses=losses, **keep)
    gg.save(f"ppo_cnn_{tag}_params1", ppo_params1=params1)
    for name in (f"ppo_cnn_{tag}", f"ppo_cnn_{tag}_params1"):
        assert os.path.getsize(os.path.join(gg.OUT, name + ".npz")) <= LIMIT, name


def gen_checkpoint():
    C, Hs, K = 1, 16, 5
    p = make_policy(C, Hs, "categorical", K, 930)
    path = os.path.join(gg.OUT, "ckpt_policy_cnn.pt")
    gg.save_legacy_without_source([p, None], path)
    blob = open(path, "rb").read()
    for needle in (b"class CNNBase", b"class Flatten", b"class Categorical", b"import torch", b"def forward"):
        assert needle not in blob, f"{path} embeds reference source ({needle!r})"
    assert len(blob) <= LIMIT
    g = torch.Generator().manual_seed(931)
    obs8 = images(g, (7, C, HW, HW))
    with torch.no_grad():
        v, a, lp, _ = p.act(obs8.float(), None, None, deterministic=True)
        logits = p.dist.linear(p.base(obs8.float(), None, None)[1])
    top = torch.sort(logits, dim=1).values
    assert float((top[:, -1] - top[:, -2]).min()) > 1e-4
    gg.save("ckpt_policy_cnn", meta=gg.meta(C=C, Hs=Hs, dist="categorical", P=K, names=[k for k, _ in p.named_parameters()],
                                            shapes=[list(q.shape) for _, q in p.named_parameters()]),
            obs=obs8.numpy(), value=v.numpy(), action=a.numpy(), logp=lp.numpy(),
            checksum=np.float64(sum(float(q.double().sum()) for q in p.parameters())))


if __name__ == "__main__":
    gen_policy("cat", 1, 16, "categorical", 5, (1, 5, 17), seed=1100)
    gen_policy("box", 3, 20, "gaussian", 3, (33,), seed=1110, levels=16)
    gen_ppo("cat", 1, 16, "categorical", 5, 4, 4, seed0=1120)
    gen_ppo("box", 1, 16, "gaussian", 3, 4, 4, seed0=1160)
    gen_checkpoint()
