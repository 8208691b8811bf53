"""Generate tests/golden/ppo_sym_*.npz by running the reference's PPO with the mirror-symmetry loss (dev-only).

Drives the reference's own PPO(..., symmetry_coef=..., mirror_obs=..., mirror_act=...) (a2c/algo/ppo.py:110-143) through
tools/ref_import.py, records the samplers' permutations as tools/gen_golden.py does and saves the inputs, the parameters
after the update, Adam's moments, the losses and the advantages.  The mirror functions are defined here, per row, the way
the reference's env package defines its own (my_pybullet_envs/laikago.py:437-497); each fixture stores the matrices of
the linear ones (m_obs / m_act) and the test suite restates the nonlinear one.  Re-run:
    python tools/gen_golden_symmetry.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402  (imports the reference and hooks torch.randperm)


# ------------------------------------------------------------------ mirrors (per row, as the reference applies them)
def small_obs_matrix():
    """O = 6: a signed permutation with a 2 x 2 mixing block on entries 4, 5."""
    m = np.zeros((6, 6))
    m[0, 1], m[1, 0], m[2, 2], m[3, 3] = 1.0, 1.0, -1.0, 1.0
    m[4:6, 4:6] = [[0.6, 0.8], [0.8, -0.6]]
    return m


def small_act_matrix():
    """A = 4: swap the two halves, flip the sign of the last entry."""
    m = np.zeros((4, 4))
    m[0, 2], m[1, 3], m[2, 0], m[3, 1] = 1.0, 1.0, 1.0, -1.0
    return m


def nonlinear_obs(x):
    """A nonlinear mirror (only the per-row callable path can serve it): the small map plus a bounded elementwise term."""
    x = np.asarray(x, np.float64)
    return small_obs_matrix() @ x + 0.25 * np.sin(x[::-1])


def laikago_obs_matrix(obs_dim=111):
    """The Laikago obs mirror as a matrix: per 37-float step block, root rotation R -> Rz(3.14159) F R F (F = diag(-1, 1, 1)),
    root velocity y flipped, the leg joint groups and the feet swapped left / right (foot y flipped)."""
    blk = np.zeros((37, 37))
    blk[0, 0] = 1.0
    yaw = 3.14159
    rz = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
    f = np.diag([-1.0, 1.0, 1.0])
    for k in range(3):               # column of the 9x9 block: the image of the unit matrix E_kj
        for j in range(3):
            e = np.zeros((3, 3))
            e[k, j] = 1.0
            blk[1:10, 1 + 3 * k + j] = (rz @ f @ e @ f).reshape(-1)
    blk[10, 10], blk[11, 11], blk[12, 12] = 1.0, -1.0, 1.0
    for base in (13, 19):
        for i in range(6):
            blk[base + i, base + (i + 3) % 6] = 1.0
    for base in (25, 31):
        for i in range(6):
            blk[base + i, base + (i + 3) % 6] = -1.0 if i % 3 == 1 else 1.0
    m = np.zeros((obs_dim, obs_dim))
    for b in range(obs_dim // 37):
        m[37 * b:37 * (b + 1), 37 * b:37 * (b + 1)] = blk
    return m


def laikago_act_matrix():
    m = np.zeros((12, 12))
    for base in (0, 6):
        for i in range(6):
            m[base + i, base + (i + 3) % 6] = 1.0
    return m


def row_fn(m):
    return lambda x: list(m @ np.asarray(x, np.float64))


# ------------------------------------------------------------------ fixtures
def gen_ppo_sym(name, O, A, H, T, N, E, M, clip, ecoef, lr, coef, m_obs, m_act, obs_fn, seed, pert=0.02):
    p = gg.make_policy("mlp", O, A, H, 1, seed)
    torch.manual_seed(seed + 5)
    ro = gg.rollout_from_policy(p, T, N, O, A, 1, seed + 6, "mlp")
    with torch.no_grad():
        nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    gg.perturb(p, pert, seed + 7)
    params0 = gg.flat_params(p)
    agent = gg.ns.PPO(p, clip, E, M, 0.5, ecoef, symmetry_coef=coef, lr=lr, eps=1e-5, max_grad_norm=0.5,
                      mirror_obs=obs_fn, mirror_act=row_fn(m_act))
    arrs = gg.rollout_arrays(ro)
    gg._REC.clear()
    torch.manual_seed(seed + 8)
    vl, al, de = agent.update(ro)
    perms = np.stack([r for k, r in gg._REC if k == "randperm"]).astype(np.int64)
    assert perms.shape == (E, T * N)
    adv = ro.returns[:-1] - ro.value_preds[:-1]
    adv = (adv - adv.mean()) / (adv.std() + 1e-5)
    st = agent.optimizer.state_dict()["state"]
    exp_avg = np.concatenate([st[i]["exp_avg"].numpy().reshape(-1) for i in range(len(st))])
    exp_avg_sq = np.concatenate([st[i]["exp_avg_sq"].numpy().reshape(-1) for i in range(len(st))])
    extra = {} if m_obs is None else {"m_obs": m_obs.astype(np.float32)}
    gg.save(name, meta=gg.meta(kind="mlp", O=O, A=A, H=H, num_feet=1, T=T, N=N, ppo_epoch=E, num_mini_batch=M, clip_param=clip,
                               entropy_coef=ecoef, lr=lr, eps=1e-5, value_loss_coef=0.5, max_grad_norm=0.5, symmetry_coef=coef,
                               linear_obs_mirror=m_obs is not None),
            params0=params0, params1=gg.flat_params(p), perms=perms, advantages=adv.numpy(),
            losses=np.array([vl, al, de], np.float64), adam_m=exp_avg, adam_v=exp_avg_sq, m_act=m_act.astype(np.float32),
            **extra, **arrs)


if __name__ == "__main__":
    ms, ma = small_obs_matrix(), small_act_matrix()
    gen_ppo_sym("ppo_sym_small", O=6, A=4, H=8, T=6, N=5, E=2, M=3, clip=0.2, ecoef=0.01, lr=3e-4, coef=0.5,
                m_obs=ms, m_act=ma, obs_fn=row_fn(ms), seed=700)
    ml, mal = laikago_obs_matrix(111), laikago_act_matrix()
    gen_ppo_sym("ppo_sym_laikago", O=111, A=12, H=64, T=8, N=16, E=3, M=4, clip=0.1, ecoef=0.0, lr=1.5e-4, coef=1.0,
                m_obs=ml, m_act=mal, obs_fn=row_fn(ml), seed=710)
    gen_ppo_sym("ppo_sym_nonlinear", O=6, A=4, H=8, T=6, N=5, E=2, M=3, clip=0.2, ecoef=0.01, lr=3e-4, coef=0.5,
                m_obs=None, m_act=ma, obs_fn=nonlinear_obs, seed=720)
