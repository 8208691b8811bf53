"""Generate tests/golden/acktr_*.npz by running the reference's A2C_ACKTR(acktr=True) with KFACOptimizer (dev-only).

Drives the reference's own A2C_ACKTR (a2c/algo/a2c_acktr.py:30-102) and KFACOptimizer (a2c/algo/kfac.py) through
tools/ref_import.py on CPU, as a2c/main.py:159-161 builds them, and saves per update: the inputs, the parameters before and
after, the loss triple, the value noise the update drew (torch.manual_seed right before update(); nothing in the update draws
before torch.randn(values.size())), the 13 modules' m_aa / m_gg and the momentum buffer.  Beside the float32 run, a float64
run of the reference itself (default dtype float64, policy .double()) takes the same rollouts, parameters and value noise and
carries its own K-FAC state: its parameters after every update are saved as *params1_f64.
gen_ckpt writes tests/golden/ckpt_policy_acktr.pt: `torch.save([actor_critic, ob_rms])` after an ACKTR update
(a2c/main.py:261-269), so the file holds the SplitBias modules and the K-FAC hooks split_bias / _prepare_model installed.
torch 2.x has removed torch.symeig; the generator installs the equivalent torch.linalg.eigh(UPLO="U") call.  Re-run:
    python tools/gen_golden_acktr.py
"""
import copy
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the reference and hooks torch.randperm)
from third_party.a2c_ppo_acktr.algo.a2c_acktr import A2C_ACKTR  # noqa: E402  (the reference's, via ref_import)

VCOEF, ECOEF = 0.5, 0.01   # a2c/arguments.py defaults
torch.symeig = lambda A, eigenvectors=True, upper=True: torch.linalg.eigh(A, UPLO="U" if upper else "L")
_randn = torch.randn


def kfac_state(agent):
    opt = agent.optimizer
    aa = np.concatenate([opt.m_aa[m].detach().numpy().reshape(-1) for m in opt.modules]).astype(np.float32)
    gm = np.concatenate([opt.m_gg[m].detach().numpy().reshape(-1) for m in opt.modules]).astype(np.float32)
    buf = np.concatenate([opt.optim.state[q]["momentum_buffer"].numpy().reshape(-1)
                          for q in agent.actor_critic.parameters()]).astype(np.float32)
    return aa, gm, buf


def as_f64_rollout(ro):
    return types.SimpleNamespace(obs=ro.obs.double(), recurrent_hidden_states=ro.recurrent_hidden_states.double(),
                                 masks=ro.masks.double(), actions=ro.actions.double(), returns=ro.returns.double(),
                                 rewards=ro.rewards.double())


def update_f64(agent64, ro, eps):
    """The reference's update at float64 with the float32 run's value noise injected."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    torch.randn = lambda *a, **k: eps.double().clone()
    try:
        return agent64.update(as_f64_rollout(ro))
    finally:
        torch.randn = _randn
        torch.set_default_dtype(prev)


def run(O, A, H, T, N, seed, critic64=False, iters=1, num_updates=20, lr_sched=False, pert=0.02):
    p = gg.make_policy("mlp", O, A, H, 1, seed)
    if critic64:
        torch.manual_seed(seed + 1)
        p.reset_critic((O,))                        # a2c/main.py:85: a 64-unit critic beside the H-wide actor
        with torch.no_grad():
            for q in p.parameters():
                q.add_(0.05 * torch.randn_like(q))
    p64 = copy.deepcopy(p).double()
    agent = A2C_ACKTR(p, VCOEF, ECOEF, acktr=True)      # a2c/main.py:159-161
    agent64 = A2C_ACKTR(p64, VCOEF, ECOEF, acktr=True)
    out = {}
    for j in range(iters):
        if lr_sched:   # a2c/main.py:201-205: writes KFACOptimizer.param_groups[0]['lr'], which step() never reads
            gg.ns.a2c_utils.update_linear_schedule(agent.optimizer, j, num_updates, 0.25)
            gg.ns.a2c_utils.update_linear_schedule(agent64.optimizer, j, num_updates, 0.25)
        torch.manual_seed(seed + 10 + j)
        ro = gg.rollout_from_policy(p, T, N, O, A, 1, seed + 20 + 2 * j, "mlp")
        with torch.no_grad():
            nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
        ro.compute_returns(nv, True, 0.99, 0.95, True)
        gg.perturb(p, pert, seed + 21 + 2 * j)   # values != value_preds: the update must evaluate the current parameters
        pre = f"it{j}_"
        out[pre + "params0"] = gg.flat_params(p)
        with torch.no_grad():
            for q64, q in zip(p64.parameters(), p.parameters()):
                q64.copy_(q.double())
        for k, v in gg.rollout_arrays(ro).items():
            if k in ("obs", "actions", "returns", "value_preds"):
                out[pre + k] = v
        torch.manual_seed(seed + 100 + j)
        eps = _randn(T, N, 1)
        torch.manual_seed(seed + 100 + j)
        vl, al, de = agent.update(ro)
        out[pre + "eps"] = eps.numpy().astype(np.float32)
        out[pre + "params1"] = gg.flat_params(p)
        out[pre + "losses"] = np.array([vl, al, de], np.float64)
        out[pre + "m_aa"], out[pre + "m_gg"], out[pre + "momentum"] = kfac_state(agent)
        vl64, al64, de64 = update_f64(agent64, ro, eps)
        out[pre + "params1_f64"] = np.concatenate([q.detach().numpy().reshape(-1) for q in p64.parameters()])
        out[pre + "losses_f64"] = np.array([vl64, al64, de64], np.float64)
    Hc = 64 if critic64 else H
    return out, dict(kind="mlp", O=O, A=A, H=H, Hc=Hc, T=T, N=N, value_loss_coef=VCOEF, entropy_coef=ECOEF, iters=iters,
                     num_updates=num_updates, lr_sched=lr_sched, lr=0.25, momentum=0.9, stat_decay=0.99, kl_clip=0.001,
                     damping=0.01, Tf=10)


def gen_acktr(name, **kw):
    out, m = run(**kw)
    if kw.get("lr_sched"):   # LR decay has no effect under ACKTR: the same trajectory without the writes
        plain, _ = run(**dict(kw, lr_sched=False))
        for k, v in out.items():
            assert np.array_equal(v, plain[k]), k
    gg.save(name, meta=gg.meta(**m), **out)


def gen_ckpt():
    """The policy file a reference `--algo acktr` run saves, and what reading it must give (flat parameters in the plain
    Policy's state_dict order, deterministic actions and values)."""
    O, A, H, T, N, seed = 11, 3, 16, 4, 6, 940
    p = gg.make_policy("mlp", O, A, H, 1, seed)
    agent = A2C_ACKTR(p, VCOEF, ECOEF, acktr=True)
    torch.manual_seed(seed + 1)
    ro = gg.rollout_from_policy(p, T, N, O, A, 1, seed + 2, "mlp")
    with torch.no_grad():
        nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    agent.update(ro)
    rms = gg.ns.RunningMeanStd(shape=(O,))
    rms.update(np.random.RandomState(4).randn(40, O) * 1.5 - 0.2)
    path = os.path.join(gg.OUT, "ckpt_policy_acktr.pt")
    gg.save_legacy_without_source([p, rms], path)
    obs = torch.randn(6, O, generator=torch.Generator().manual_seed(seed + 3))
    with torch.no_grad():
        v, a, lp, _ = p.act(obs, None, None, deterministic=True)
    keys = [k for k in p.state_dict()]
    assert any(k.endswith(".module.weight") for k in keys) and any(k.endswith(".add_bias._bias") for k in keys), keys
    gg.save("ckpt_policy_acktr", meta=gg.meta(kind="mlp", O=O, A=A, H=H, f=1), flat=gg.flat_params(p), obs=obs.numpy(),
            value=v.numpy(), action=a.numpy(), logp=lp.numpy(), rms_mean=rms.mean, rms_var=rms.var,
            rms_count=np.float64(rms.count))


if __name__ == "__main__":
    gen_acktr("acktr_tiny", O=5, A=3, H=8, T=4, N=3, seed=900)
    gen_acktr("acktr_default", O=47, A=12, H=64, T=5, N=16, seed=910, iters=2)
    gen_acktr("acktr_critic64", O=20, A=6, H=100, T=5, N=8, seed=920, critic64=True)
    gen_acktr("acktr_multi", O=11, A=3, H=16, T=5, N=6, seed=930, iters=12, num_updates=20, lr_sched=True)
    gen_ckpt()
