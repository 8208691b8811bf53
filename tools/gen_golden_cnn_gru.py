"""Generate tests/golden/policy_cnn_gru_{cat,box}.npz, ppo_cnn_gru_{cat,box}.npz (+ _params1) and ckpt_policy_cnn_gru.{pt,npz} by
running the reference's Policy on image observations with base_kwargs={'recurrent': True} (dev-only).

Drives the reference's own Policy with CNNBase(recurrent=True) (a2c/model.py:117-230), RolloutStorage and PPO through
tools/ref_import.py on the CPU.  Everything written is data: weights, the state_dict's key list, observations as uint8, hidden
states, masks, injected draws, and the results of act / get_value / evaluate_actions / PPO.update.
  * policy_cnn_gru_<tag>: params and `keys` (the reference's state_dict order), obs [T n] (uint8, time-major), hxs [n, Hs] (nonzero),
    masks [T n] (tests/cnn_gru_ref.py:default_masks), and the reference's float32 results: evaluate_actions over all T n rows (values,
    log-probs, the entropy, the final hidden state), and on the first step's n rows get_value, the deterministic act, and
      - Box: the normal draws act() consumed with its action and log-prob;
      - Discrete: `uniform` draws 1e-4 clear of every cumulative boundary of the float64 forward; the library's convention decides
        the class, evaluate_actions of the reference gives its log-prob (as tools/gen_golden_cnn.py).
  * ppo_cnn_gru_<tag>: a rollout collected by the reference's act() with its hidden states, the policy perturbed, the recorded
    randperms of the recurrent generator ([E, N]), the loss triple and -- in _params1 -- the parameters after PPO.update, E = 2, M = 2.
  * ckpt_policy_cnn_gru.pt: torch.save([actor_critic, None]) in the legacy container without the classes' source text, with the
    policy's flat parameters' checksum and its evaluate_actions on a 3 x 2 sequence beside it.
Every float32 result is asserted to lie within a tenth of the tests' tolerance of tests/cnn_gru_ref.py's float64 evaluation (for the
whole update: seeds are tried in order until that holds, as tools/gen_golden_cnn.py does).
Re-run:
    python tools/gen_golden_cnn_gru.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import gen_golden as gg      # noqa: E402  (imports the reference and hooks torch.randperm)
import cnn_gru_ref as gr     # noqa: E402
import cnn_ref as cr         # noqa: E402
from gen_golden_cnn import images, space_of, tenth   # noqa: E402

ns = gg.ns
HW = 84
CLIP, VCOEF, ECOEF, LR, EPS, MAXN = cr.CLIP, cr.VCOEF, cr.ECOEF, cr.LR, cr.EPS, 0.5
E, M = 2, 2
LIMIT = 860 * 1024


def make_policy(C, Hs, dist, P, seed):
    torch.manual_seed(seed)
    p = ns.Policy((C, HW, HW), space_of(dist, P), base_kwargs={"recurrent": True, "hidden_size": Hs})
    assert type(p.base).__name__ == "CNNBase" and p.is_recurrent
    with torch.no_grad():
        for name, q in p.named_parameters():
            q.add_((0.6 if name.startswith("dist.linear") else 0.02) * torch.randn_like(q))
    assert [(k, tuple(v.shape)) for k, v in p.state_dict().items()] == gr.param_shapes(C, Hs, dist, P)
    return p


def gen_policy(tag, C, Hs, dist, P, T, n, seed):
    p = make_policy(C, Hs, dist, P, seed)
    shapes = gr.param_shapes(C, Hs, dist, P)
    params = gg.flat_params(p)
    g = torch.Generator().manual_seed(seed + 1)
    obs8 = images(g, (T * n, C, HW, HW))
    obs = obs8.float()
    hxs = 0.5 * torch.randn(n, Hs, generator=g)
    masks = torch.from_numpy(gr.default_masks(T, n)[:T].reshape(-1, 1).copy())
    out = dict(params=params, keys=np.array(list(p.state_dict())), obs=obs8.numpy(), hxs=hxs.numpy(), masks=masks.numpy())
    m0, o0 = masks[:n], obs[:n]
    with torch.no_grad():
        gv = p.get_value(o0, hxs, m0)
        v_det, a_det, lp_det, h_det = p.act(o0, hxs, m0, deterministic=True)
    d64 = gr.act64(shapes, params, o0.numpy(), hxs.numpy(), m0.numpy().reshape(-1), 1, dist)
    tenth(gv.numpy(), d64["value"], f"{tag} value")
    tenth(lp_det.numpy(), d64["logp"], f"{tag} det logp")
    tenth(h_det.numpy(), d64["hxs"], f"{tag} hidden state")
    out.update(get_value=gv.numpy(), det_action=a_det.numpy(), det_logp=lp_det.numpy(), det_hxs=h_det.numpy())
    f64 = gr.forward64(shapes, params, obs.numpy(), hxs.numpy(), masks.numpy().reshape(-1), T, dist)
    if dist == "categorical":
        assert d64["margin"] > 1e-4 and np.array_equal(a_det.numpy().reshape(-1), d64["action"])
        u = torch.rand(T * n, generator=g).numpy().astype(np.float32)
        act, margin = cr.categorical_sample(f64[1], u)
        assert margin > 1e-4, f"{tag}: a uniform draw lies {margin:.2e} from a cumulative boundary"
        ref_act = torch.as_tensor(act.reshape(-1, 1))
        out.update(uniform=u, act_action=act.reshape(-1, 1).astype(np.int64))
    else:
        with torch.no_grad():
            torch.manual_seed(seed + 2)
            value, action, logp, _ = p.act(o0, hxs, m0)
            torch.manual_seed(seed + 2)
            noise = torch.randn(n, P)
        a64 = gr.act64(shapes, params, o0.numpy(), hxs.numpy(), m0.numpy().reshape(-1), 1, dist, noise.numpy())
        if float(np.abs(action.numpy() - a64["action"]).max()) > 1e-5:      # the stream torch.normal consumed is another one: solve for it
            with torch.no_grad():
                _, feat, _ = p.base(o0, hxs, m0)
                d = p.dist(feat)
                noise = (action - d.mean) / d.stddev
            a64 = gr.act64(shapes, params, o0.numpy(), hxs.numpy(), m0.numpy().reshape(-1), 1, dist, noise.numpy())
        tenth(action.numpy(), a64["action"], f"{tag} sampled action")
        out.update(noise=noise.numpy(), act_action=action.numpy(), act_logp=logp.numpy(), act_value=value.numpy())
        ref_act = torch.randn(T * n, P, generator=g) * 0.5
    with torch.no_grad():
        ev, elp, eent, eh = p.evaluate_actions(obs, hxs, masks, ref_act)
        v64, lp64, ent64, h64 = gr.evaluate(cr.leaves(params, shapes), cr.ar.t64(obs.numpy()), hxs.numpy(), masks.numpy().reshape(-1), T,
                                            ref_act.numpy(), dist)
    tenth(ev.numpy(), v64.numpy(), f"{tag} eval value")
    tenth(elp.numpy(), lp64.numpy(), f"{tag} eval logp")
    tenth(eent.numpy(), ent64.numpy(), f"{tag} entropy")
    tenth(eh.numpy(), h64.numpy(), f"{tag} final hidden state")
    out.update(eval_action=ref_act.numpy(), eval_value=ev.numpy(), eval_logp=elp.numpy(), eval_entropy=np.float32(eent.item()), eval_hxs=eh.numpy())
    name = f"policy_cnn_gru_{tag}"
    gg.save(name, meta=gg.meta(C=C, Hs=Hs, dist=dist, P=P, T=T, n=n), **out)
    assert os.path.getsize(os.path.join(gg.OUT, name + ".npz")) <= LIMIT, name


def collect(p, dist, P, C, Hs, T, N, seed):
    ro = ns.RolloutStorage(T, N, (C, HW, HW), space_of(dist, P), Hs, 1)
    g = torch.Generator().manual_seed(seed)
    ro.obs[0].copy_(images(g, (N, C, HW, HW)).float())
    ro.recurrent_hidden_states[0].copy_(0.5 * torch.randn(N, Hs, generator=g))
    ro.masks[0, 0] = 0.0
    for step in range(T):
        with torch.no_grad():
            value, action, logp, hxs = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
        mask = torch.ones(N, 1)
        if step == 0:
            mask[N - 1] = 0.0      # an interior reset (masks[1]) ...
        if step == 1 and T > 2:
            mask[N - 1] = 0.0      # ... and the step after it
        ro.insert(images(g, (N, C, HW, HW)).float(), hxs, action, logp, value, torch.randn(N, 1, generator=g), mask,
                  (torch.rand(N, 1, generator=g) > 0.03).float(), torch.randn(N, 1, generator=g))
    with torch.no_grad():
        nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    return ro


def case_of(C, Hs, dist, P, T, N, params, arrs, hxs):
    return cr.Case(C=C, Hs=Hs, dist=dist, P=P, T=T, N=N, shapes=gr.param_shapes(C, Hs, dist, P), params=params, ecoef=ECOEF, head="init",
                   obs=arrs["obs"], actions=arrs["actions"], action_log_probs=arrs["action_log_probs"], value_preds=arrs["value_preds"],
                   returns=arrs["returns"], masks=arrs["masks"], hxs=hxs,
                   adv=cr.ar.normalised_advantages(arrs["returns"][:-1].reshape(-1), arrs["value_preds"][:-1].reshape(-1)).numpy())


def adam_update64(c, perms):
    params = c.params.astype(np.float64).copy()
    m, v, t, acc = np.zeros_like(params), np.zeros_like(params), 0, np.zeros(3)
    cc = cr.Case(c)
    key = (c.C, c.Hs, c.dist, c.P, c.T, c.N)
    for e in range(E):
        for envs in gr.step_envs(key, M, perms[e]):
            cc["params"] = params
            g, l3 = gr.case_grad(cc, envs)
            g = g * cr.clip_factor(g, MAXN)
            t += 1
            m = 0.9 * m + 0.1 * g
            v = 0.999 * v + 0.001 * g * g
            params = params - (LR / (1 - 0.9 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + EPS)
            acc += l3
    return acc / (E * M), params, t


def gen_ppo(tag, C, Hs, dist, P, T, N, seed0):
    for seed in range(seed0, seed0 + 40):
        p = make_policy(C, Hs, dist, P, seed)
        torch.manual_seed(seed + 5)
        ro = collect(p, dist, P, C, Hs, T, N, seed + 6)
        gg.perturb(p, 0.01, seed + 7)
        params0 = gg.flat_params(p)
        q = copy.deepcopy(p)
        agent = ns.PPO(q, CLIP, E, M, VCOEF, ECOEF, lr=LR, eps=EPS, max_grad_norm=MAXN)
        gg._REC.clear()
        torch.manual_seed(seed + 9)
        losses = np.array(agent.update(ro), np.float64)
        perms = np.stack([r for k, r in gg._REC if k == "randperm"]).astype(np.int64)
        assert perms.shape == (E, N), perms.shape
        params1 = gg.flat_params(q)
        arrs = gg.rollout_arrays(ro)
        hxs = ro.recurrent_hidden_states.numpy().copy()
        l64, p64, steps = adam_update64(case_of(C, Hs, dist, P, T, N, params0, arrs, hxs), perms)
        err = np.abs(params1.astype(np.float64) - p64)
        bad = err > 0.1 * (cr.ATOL + cr.RTOL * np.abs(p64))
        lr_ = float(np.max(np.abs(losses - l64) / (cr.ATOL + cr.RTOL * np.abs(l64))))
        print(f"ppo_cnn_gru_{tag} seed {seed}: losses {lr_:.3f} of tol, {int(bad.sum())}/{bad.size} parameters past a tenth, max err {err.max():.2e}")
        if lr_ <= 0.1 and bad.sum() <= max(1, int(5e-4 * bad.size)) and err.max() <= LR * steps:
            break
    else:
        raise RuntimeError(f"ppo_cnn_gru_{tag}: no seed whose float32 update stays with the float64 one")
    keep = {k: arrs[k] for k in ("actions", "returns", "value_preds", "action_log_probs", "masks")}
    assert np.array_equal(arrs["obs"], arrs["obs"].astype(np.uint8))
    gg.save(f"ppo_cnn_gru_{tag}", meta=gg.meta(C=C, Hs=Hs, dist=dist, P=P, T=T, N=N, ppo_epoch=E, num_mini_batch=M, clip_param=CLIP,
                                              value_loss_coef=VCOEF, entropy_coef=ECOEF, lr=LR, eps=EPS, max_grad_norm=MAXN, seed=seed, steps=steps),
            params0=params0, obs=arrs["obs"].astype(np.uint8), hxs=hxs, perms=perms, ppo_losses=losses, **keep)
    gg.save(f"ppo_cnn_gru_{tag}_params1", ppo_params1=params1)
    for name in (f"ppo_cnn_gru_{tag}", f"ppo_cnn_gru_{tag}_params1"):
        assert os.path.getsize(os.path.join(gg.OUT, name + ".npz")) <= LIMIT, name


def gen_checkpoint():
    C, Hs, K, T, n = 1, 16, 5, 3, 2
    p = make_policy(C, Hs, "categorical", K, 1930)
    path = os.path.join(gg.OUT, "ckpt_policy_cnn_gru.pt")
    gg.save_legacy_without_source([p, None], path)
    blob = open(path, "rb").read()
    for needle in (b"class CNNBase", b"class NNBase", b"class Flatten", b"class Categorical", b"import torch", b"def forward"):
        assert needle not in blob, f"{path} embeds reference source ({needle!r})"
    assert len(blob) <= LIMIT
    g = torch.Generator().manual_seed(1931)
    obs8 = images(g, (T * n, C, HW, HW))
    hxs = 0.5 * torch.randn(n, Hs, generator=g)
    masks = torch.ones(T * n, 1)
    masks[2] = 0.0
    acts = torch.randint(0, K, (T * n, 1), generator=g)
    with torch.no_grad():
        v, lp, ent, h = p.evaluate_actions(obs8.float(), hxs, masks, acts)
    gg.save("ckpt_policy_cnn_gru", meta=gg.meta(C=C, Hs=Hs, dist="categorical", P=K, T=T, n=n, names=[k for k, _ in p.named_parameters()],
                                                shapes=[list(q.shape) for _, q in p.named_parameters()]),
            params=gg.flat_params(p), obs=obs8.numpy(), hxs=hxs.numpy(), masks=masks.numpy(), actions=acts.numpy(), value=v.numpy(), logp=lp.numpy(),
            entropy=np.float32(ent.item()), hxs_out=h.numpy(),
            checksum=np.float64(sum(float(q.double().sum()) for q in p.parameters())))


if __name__ == "__main__":
    gen_policy("cat", 1, 16, "categorical", 5, 5, 3, seed=2100)
    gen_policy("box", 2, 20, "gaussian", 3, 3, 2, seed=2110)
    gen_ppo("cat", 1, 16, "categorical", 5, 4, 4, seed0=2120)
    gen_ppo("box", 2, 20, "gaussian", 3, 3, 4, seed0=2160)
    gen_checkpoint()
