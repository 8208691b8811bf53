"""Generate tests/golden/policy_gru_*.npz, ppo_gru_*.npz, recgen_gru.npz and ckpt_policy_gru.{pt,npz} by running the reference
(dev-only).

Drives the reference's own Policy(..., base_kwargs={'recurrent': True}) (a2c/model.py:117-201, 233-264) and
RolloutStorage.recurrent_generator (a2c/storage.py:194-251) through tools/ref_import.py on the CPU and saves inputs and
outputs.  Only the data is committed.  The generator also checks what the tests rely on:
  * sequence evaluation (masks with zeros, the reference's cut-at-zero-mask loop) reproduces the values the step-by-step
    rollout recorded -- i.e. "h <- h * masks[t] at every step" is what the reference computes for 0/1 masks;
  * the reference's own float32 results stay within a tenth of the tests' tolerance of its float64 results.
Re-run:
    python tools/gen_golden_recurrent.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the reference and hooks torch.randperm)

ns = gg.ns
RTOL, ATOL = 1e-4, 1e-5   # tests/helpers.py


def make_gru_policy(O, A, H, seed):
    torch.manual_seed(seed)
    p = ns.Policy((O,), ns.Box(shape=(A,)), base_kwargs={"recurrent": True, "hidden_size": H})
    with torch.no_grad():   # as gen_golden.make_policy: non-trivial means, non-zero biases
        for q in p.parameters():
            q.add_(0.05 * torch.randn_like(q))
    return p


def masks_with_zeros(shape, g, p_zero=0.08):
    m = (torch.rand(*shape, generator=g) > p_zero).float()
    flat = m.view(-1)
    if flat.min() > 0:   # every fixture exercises the reset
        flat[flat.numel() // 2] = 0.0
    return m


def within_tenth(f32, f64, what, rtol=RTOL, atol=ATOL):
    f32, f64 = np.asarray(f32, np.float64), np.asarray(f64, np.float64)
    ratio = float(np.max(np.abs(f32 - f64) / (atol + rtol * np.abs(f64))))
    assert ratio <= 0.1, f"{what}: the reference's float32 is {ratio:.3f} of the tolerance away from its float64"
    return ratio


def gen_policy_gru(name, O, A, H, n, T, seed):
    p = make_gru_policy(O, A, H, seed)
    sd = p.state_dict()
    names = list(sd.keys())
    shapes = [list(v.shape) for v in sd.values()]
    g = torch.Generator().manual_seed(seed + 1)
    out = {}
    with torch.no_grad():
        # ---- one step
        obs = torch.randn(n, O, generator=g)
        hxs = 0.5 * torch.randn(n, H, generator=g)
        masks = masks_with_zeros((n, 1), g, 0.3)
        torch.manual_seed(seed + 2)
        value, action, logp, hxs1 = p.act(obs, hxs, masks)
        _, feat, _ = p.base(obs, hxs, masks)
        dist = p.dist(feat)
        noise = (action - dist.mean) / dist.stddev
        _, a_det, lp_det, hxs_det = p.act(obs, hxs, masks, deterministic=True)
        assert torch.equal(hxs_det, hxs1)
        gv = p.get_value(obs, hxs, masks)
        out.update(obs=obs.numpy(), hxs=hxs.numpy(), masks=masks.numpy(), noise=noise.numpy(), act_value=value.numpy(),
                   act_action=action.numpy(), act_logp=logp.numpy(), act_hxs=hxs1.numpy(), det_action=a_det.numpy(),
                   det_logp=lp_det.numpy(), get_value=gv.numpy())
        # ---- a rollout collected step by step, then evaluated as one sequence
        ro = ns.RolloutStorage(T, n, (O,), ns.Box(shape=(A,)), H, 1)
        ro.obs[0].copy_(torch.randn(n, O, generator=g))
        ro.recurrent_hidden_states[0].copy_(0.5 * torch.randn(n, H, generator=g))
        ro.masks[0].copy_(masks_with_zeros((n, 1), g, 0.3))
        all_masks = masks_with_zeros((T, n, 1), g)
        torch.manual_seed(seed + 3)
        for step in range(T):
            v, a, lp, h = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
            ro.insert(torch.randn(n, O, generator=g), h, a, lp, v, torch.zeros(n, 1), all_masks[step], torch.ones(n, 1),
                      torch.zeros(n, 1))
        seq_obs = ro.obs[:-1].reshape(-1, O)
        seq_masks = ro.masks[:-1].reshape(-1, 1)
        hxs0 = ro.recurrent_hidden_states[0].clone()
        ev_v, ev_lp, _, ev_h = p.evaluate_actions(seq_obs, hxs0, seq_masks, ro.actions.reshape(-1, A))
        # the equivalence the GPU scan is built on
        bitwise = torch.equal(ev_v, ro.value_preds[:-1].reshape(-1, 1)) and torch.equal(ev_h, ro.recurrent_hidden_states[-1])
        # bit for bit at the shipped width; at hidden 8 the reference's own one-step and sequence GEMMs round differently (its
        # BLAS picks another kernel for 3-row operands), so that case is held to 2e-6 below
        assert bitwise or H < 64, "sequence evaluation is not bit-identical to the step-by-step rollout"
        assert torch.allclose(ev_v, ro.value_preds[:-1].reshape(-1, 1), rtol=0, atol=2e-6), "sequence evaluation != step-by-step values"
        assert torch.allclose(ev_lp, ro.action_log_probs.reshape(-1, 1), rtol=0, atol=2e-5)
        assert torch.allclose(ev_h, ro.recurrent_hidden_states[-1], rtol=0, atol=2e-6)
        act_eval = ro.actions.reshape(-1, A) + 0.3 * torch.randn(T * n, A, generator=g)
        ev_v, ev_lp, ev_ent, ev_h = p.evaluate_actions(seq_obs, hxs0, seq_masks, act_eval)
        pd = copy.deepcopy(p).double()
        dv, dlp, dent, dh = pd.evaluate_actions(seq_obs.double(), hxs0.double(), seq_masks.double(), act_eval.double())
        r = [within_tenth(ev_v.numpy(), dv.numpy(), name + " value"), within_tenth(ev_lp.numpy(), dlp.numpy(), name + " logp"),
             within_tenth(ev_h.numpy(), dh.numpy(), name + " hxs"), within_tenth(ev_ent.item(), dent.item(), name + " entropy")]
        out.update(seq_obs=seq_obs.numpy(), seq_hxs=hxs0.numpy(), seq_masks=seq_masks.numpy(), seq_action=act_eval.numpy(),
                   seq_value=ev_v.numpy(), seq_logp=ev_lp.numpy(), seq_entropy=np.float32(ev_ent.item()), seq_hxs_out=ev_h.numpy(),
                   step_values=ro.value_preds[:-1].numpy().copy(), step_hxs=ro.recurrent_hidden_states.numpy().copy())
    zeros = int((seq_masks == 0).sum())
    print(f"{name}: sequence == steps bitwise: {bitwise}; {zeros} zero masks; float32 vs float64 / tolerance: {max(r):.4f}")
    gg.save(name, meta=gg.meta(O=O, A=A, H=H, n=n, T=T, names=names, shapes=shapes, zero_masks=zeros), params=gg.flat_params(p), **out)


def rollout_gru(p, T, N, O, A, H, seed):
    """Fill a RolloutStorage the way the main loop does (act -> insert) with the policy's real hidden size, synthetic env,
    episode ends inside the rollout (8 % zero masks)."""
    ro = ns.RolloutStorage(T, N, (O,), ns.Box(shape=(A,)), H, 1)
    g = torch.Generator().manual_seed(seed)
    ro.obs[0].copy_(torch.randn(N, O, generator=g))
    for step in range(T):
        with torch.no_grad():
            value, action, logp, hxs = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
        obs = torch.randn(N, O, generator=g)
        reward = torch.randn(N, 1, generator=g)
        masks = (torch.rand(N, 1, generator=g) > 0.08).float()
        bad = (torch.rand(N, 1, generator=g) > 0.03).float()
        ro.insert(obs, hxs, action, logp, value, reward, masks, bad, torch.zeros(N, 1))
    if ro.masks[1:-1].min() > 0:
        ro.masks[T // 2, 0] = 0.0
    return ro


def adam_state(agent):
    st = agent.optimizer.state_dict()["state"]
    return (np.concatenate([st[i]["exp_avg"].numpy().reshape(-1) for i in range(len(st))]),
            np.concatenate([st[i]["exp_avg_sq"].numpy().reshape(-1) for i in range(len(st))]))


def gen_ppo_gru(name, O, A, H, T, N, E, M, clip, ecoef, lr, seed, pert=0.02, split=False):
    p = make_gru_policy(O, A, H, seed)
    torch.manual_seed(seed + 5)
    ro = rollout_gru(p, T, N, O, A, H, seed + 6)
    with torch.no_grad():
        nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    gg.perturb(p, pert, seed + 7)
    params0 = gg.flat_params(p)
    p64 = copy.deepcopy(p).double()
    ro64 = copy.deepcopy(ro)
    for k, v in vars(ro64).items():
        if torch.is_tensor(v):
            setattr(ro64, k, v.double())
    agent = ns.PPO(p, clip, E, M, 0.5, ecoef, lr=lr, eps=1e-5, max_grad_norm=0.5)
    arrs = gg.rollout_arrays(ro)
    arrs["recurrent_hidden_states0"] = ro.recurrent_hidden_states[0].numpy().copy()   # the update reads slot 0 only (a2c/storage.py:216-217)
    gg._REC.clear()
    torch.manual_seed(seed + 8)
    vl, al, de = agent.update(ro)
    perms = np.stack([r for k, r in gg._REC if k == "randperm"]).astype(np.int64)
    assert perms.shape == (E, N)
    per = N // M
    steps = E * (N // per)
    st = agent.optimizer.state_dict()["state"]
    assert int(st[0]["step"]) == steps
    adv = ro.returns[:-1] - ro.value_preds[:-1]
    adv = (adv - adv.mean()) / (adv.std() + 1e-5)
    m, v = adam_state(agent)
    # the same update by the reference in float64, replaying the permutations: its own float32 rounding must use under a tenth of
    # what the tests allow (helpers.assert_close for losses, assert_close_adam without outliers for parameters)
    replay = [torch.from_numpy(q.copy()) for q in perms]
    rp = torch.randperm
    torch.randperm = lambda n, *a_, **k_: replay.pop(0)
    try:
        agent64 = ns.PPO(p64, clip, E, M, 0.5, ecoef, lr=lr, eps=1e-5, max_grad_norm=0.5)
        l64 = agent64.update(ro64)
    finally:
        torch.randperm = rp
    p1, p1_64 = gg.flat_params(p).astype(np.float64), np.concatenate([q.detach().numpy().reshape(-1) for q in p64.state_dict().values()])
    ratio_p = within_tenth(p1, p1_64, name + " params after the update")
    ratio_l = within_tenth([vl, al, de], l64, name + " losses")
    m64, v64 = adam_state(agent64)
    adv64 = ro64.returns[:-1] - ro64.value_preds[:-1]
    adv64 = (adv64 - adv64.mean()) / (adv64.std() + 1e-5)
    ratio_a = max(within_tenth(m, m64, name + " adam m", 1e-3, 1e-7), within_tenth(v, v64, name + " adam v", 1e-3, 1e-10),
                  within_tenth(adv.numpy(), adv64.numpy(), name + " advantages", 1e-5, ATOL))
    print(f"{name}: {steps} optimizer steps; float32 vs float64 / tolerance: params {ratio_p:.4f}, losses {ratio_l:.4f}, adam / advantages {ratio_a:.4f}")
    gg.save(name, meta=gg.meta(O=O, A=A, H=H, T=T, N=N, ppo_epoch=E, num_mini_batch=M, steps=steps, clip_param=clip, entropy_coef=ecoef,
                               lr=lr, eps=1e-5, value_loss_coef=0.5, max_grad_norm=0.5, names=list(p.state_dict().keys()),
                               shapes=[list(t.shape) for t in p.state_dict().values()]),
            params0=params0, perms=perms, advantages=adv.numpy(), losses=np.array([vl, al, de], np.float64),
            **({} if split else dict(params1=gg.flat_params(p), adam_m=m, adam_v=v)), **arrs)
    files = [name]
    if split:   # hidden 64: every parameter-sized array is 130-160 KB, so each result goes into a file of its own (<name>_<key>.npz)
        for key, arr in (("params1", gg.flat_params(p)), ("adam_m", m), ("adam_v", v)):
            gg.save(f"{name}_{key}", **{key: arr})
            files.append(f"{name}_{key}")
    for f in files:
        assert os.path.getsize(os.path.join(gg.OUT, f + ".npz")) < 300 * 1024, f


def gen_recgen():
    """recurrent_generator's minibatches, permutation recorded: N = 8 with M = 3 (4 minibatches) and M = 5 (8), N = 6 with M = 2."""
    out, cases = {}, []
    for ci, (T, N, M) in enumerate([(5, 8, 3), (3, 8, 5), (4, 6, 2)]):
        O, A, H = 3, 2, 4
        ro = ns.RolloutStorage(T, N, (O,), ns.Box(shape=(A,)), H, 1)
        gg.fill_rollout(ro, T, N, O, A, 1, 900 + ci)
        g = torch.Generator().manual_seed(950 + ci)
        ro.recurrent_hidden_states.copy_(torch.randn(T + 1, N, H, generator=g))
        ro.returns.copy_(torch.randn(T + 1, N, 1, generator=g))
        adv = torch.randn(T, N, 1, generator=g)
        gg._REC.clear()
        torch.manual_seed(970 + ci)
        batches = list(ro.recurrent_generator(adv, M))
        perm = [r for k, r in gg._REC if k == "randperm"]
        assert len(perm) == 1 and perm[0].shape == (N,)
        pre = f"c{ci}_"
        out[pre + "perm"] = perm[0].astype(np.int64)
        out[pre + "advantages"] = adv.numpy()
        out[pre + "recurrent_hidden_states"] = ro.recurrent_hidden_states.numpy().copy()
        for k, v in gg.rollout_arrays(ro).items():
            out[pre + k] = v
        for bi, b in enumerate(batches):
            assert len(b) == 8
            for fi, t in enumerate(b):
                out[f"{pre}b{bi}_{fi}"] = t.numpy().copy()
        cases.append(dict(T=T, N=N, M=M, n_batches=len(batches)))
    assert [c["n_batches"] for c in cases] == [4, 8, 2]
    # N % (N // M) != 0: the reference runs past its permutation
    ro = ns.RolloutStorage(2, 7, (3,), ns.Box(shape=(2,)), 4, 1)
    try:
        list(ro.recurrent_generator(torch.zeros(2, 7, 1), 2))
        raise SystemExit("expected the reference to fail for N = 7, M = 2")
    except IndexError:
        pass
    gg.save("recgen_gru", meta=gg.meta(cases=cases), **out)


def gen_ckpt():
    """[actor_critic, ob_rms] of a recurrent policy in the legacy container, written as gen_golden.gen_checkpoints writes the
    others (class names and data, no source text)."""
    O, A, H, n = 7, 3, 16, 5
    p = make_gru_policy(O, A, H, 730)
    rms = ns.RunningMeanStd(shape=(O,))
    rms.update(np.random.RandomState(4).randn(40, O) * 1.5 - 0.25)
    path = os.path.join(gg.OUT, "ckpt_policy_gru.pt")
    gg.save_legacy_without_source([p, rms], path)
    blob = open(path, "rb").read()
    for needle in (b"class NNBase", b"class GRU", b"def _forward_gru"):
        assert needle not in blob, f"{path} embeds source ({needle!r})"
    g = torch.Generator().manual_seed(731)
    obs, hxs = torch.randn(n, O, generator=g), 0.5 * torch.randn(n, H, generator=g)
    masks = masks_with_zeros((n, 1), g, 0.3)
    with torch.no_grad():
        v, a, lp, h = p.act(obs, hxs, masks, deterministic=True)
    sd = p.state_dict()
    gg.save("ckpt_policy_gru", meta=gg.meta(O=O, A=A, H=H, names=list(sd.keys()), shapes=[list(t.shape) for t in sd.values()]),
            flat=gg.flat_params(p), obs=obs.numpy(), hxs=hxs.numpy(), masks=masks.numpy(), value=v.numpy(), action=a.numpy(),
            logp=lp.numpy(), hxs_out=h.numpy(), rms_mean=rms.mean, rms_var=rms.var, rms_count=np.float64(rms.count))
    print(f"ckpt_policy_gru.pt: {os.path.getsize(path) / 1024:.1f} KiB")


def gen_ppo_all():
    # Four parameter-sized arrays (before, after, Adam m, v) are most of a fixture.  Hidden 32 keeps a whole case in one file under
    # 300 KB; the hidden-64 cases (W_hh LDS-resident at the shipped width) write params1 / adam_m / adam_v to files of their own.
    gen_ppo_gru("ppo_gru_onestep", O=11, A=3, H=32, T=10, N=6, E=1, M=1, clip=0.1, ecoef=0.01, lr=1.5e-4, seed=1100, pert=0.05)
    gen_ppo_gru("ppo_gru_onestep64", O=11, A=3, H=64, T=10, N=6, E=1, M=1, clip=0.1, ecoef=0.01, lr=1.5e-4, seed=1105, pert=0.05, split=True)
    gen_ppo_gru("ppo_gru_tiny", O=5, A=2, H=8, T=6, N=8, E=2, M=3, clip=0.2, ecoef=0.01, lr=3e-4, seed=1110, pert=0.05)   # 4 steps per epoch
    gen_ppo_gru("ppo_gru_hopper", O=11, A=3, H=64, T=16, N=8, E=4, M=4, clip=0.2, ecoef=0.0, lr=3e-4, seed=1120, split=True)
    gen_ppo_gru("ppo_gru_laikago", O=47, A=12, H=64, T=12, N=8, E=3, M=2, clip=0.2, ecoef=0.01, lr=3e-4, seed=1130, split=True)
    gen_ppo_gru("ppo_gru_long", O=11, A=3, H=32, T=128, N=8, E=2, M=2, clip=0.2, ecoef=0.01, lr=3e-4, seed=1140)   # the north-star rollout length


if __name__ == "__main__":
    if sys.argv[1:] == ["ppo"]:   # the update fixtures only
        gen_ppo_all()
        sys.exit(0)
    gen_policy_gru("policy_gru_tiny", O=5, A=2, H=8, n=3, T=6, seed=1000)
    gen_policy_gru("policy_gru_hopper", O=11, A=3, H=64, n=8, T=16, seed=1010)
    gen_policy_gru("policy_gru_laikago", O=47, A=12, H=64, n=20, T=12, seed=1020)
    gen_recgen()
    gen_ckpt()
    gen_ppo_all()
