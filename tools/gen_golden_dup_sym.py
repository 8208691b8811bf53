"""Generate tests/golden/dup_sym_*.npz by driving the reference's rollout fill with --dup-sym (dev-only).

The reference's own RolloutStorage(T, 2n, ...) and my_pybullet_envs.utils.mirror_obsact_batch / replace_obs_with_feat
(through tools/ref_import.py) run the literal sequence of a2c/main.py:181-245: slot 0 from cat(obs, mirror_obs(obs)) and the
features repeated, then T inserts of the augmented / repeated rows.  What the loop takes from the policy and the
environments (value, action, log-prob, hidden state, obs, reward, done flags) are seeded draws: the fill does not depend on
where they come from.  Stored, as data only: the n-wide inputs, the mirror matrices and the resulting 2n-wide fields.  The
mirror callables are per-row maps over matrices whose entries are float32 values (stored), as tools/gen_golden_symmetry.py
defines its own; the Laikago pair is my_pybullet_envs/laikago.py:437-497 (the module itself needs pybullet).  Re-run:
    python tools/gen_golden_dup_sym.py
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref_import  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")


def row_fn(m32):
    m = m32.astype(np.float64)
    return lambda x: list(m @ np.asarray(x, np.float64))


def gen(name, ns, O, A, T, n, hidden, m_obs, m_act, seed):
    m_obs, m_act = m_obs.astype(np.float32), m_act.astype(np.float32)
    mirror_obs, mirror_action = row_fn(m_obs), row_fn(m_act)
    utils = ns.gan_utils
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    obs = randn(n, O)
    obs_feat = utils.replace_obs_with_feat(obs, False, None, return_tensor=True)   # a2c/main.py:168
    feat_len = obs_feat.size(1)
    rollouts = ns.RolloutStorage(T, 2 * n, (O,), ns.Box(shape=(A,)), hidden, feat_len)   # :175-178
    inputs = {"obs0": obs.numpy().copy(), "feat0": obs_feat.numpy().copy()}
    steps = {k: [] for k in ("obs", "obs_feat", "hxs", "actions", "logp", "value", "reward", "masks", "bad_masks")}
    # :181-185
    obs_s = utils.mirror_obsact_batch(obs, False, mirror_obs, augment=True)
    obs_feat_s = obs_feat.repeat(2, 1)
    rollouts.obs[0].copy_(obs_s)
    rollouts.obs_feat[0].copy_(obs_feat_s)
    for step in range(T):   # :207-245
        value, action, action_log_prob, recurrent_hidden_states = randn(n, 1), randn(n, A), randn(n, 1), randn(n, hidden)
        obs, reward = randn(n, O), randn(n, 1)
        done = torch.rand(n, generator=g) < 0.25
        bad = torch.rand(n, generator=g) < 0.15
        obs_feat = utils.replace_obs_with_feat(obs, False, None, return_tensor=True)
        masks = torch.Tensor([[0.0] if done_ else [1.0] for done_ in done])
        bad_masks = torch.Tensor([[0.0] if b else [1.0] for b in bad])
        for k, v in zip(steps, (obs, obs_feat, recurrent_hidden_states, action, action_log_prob, value, reward, masks, bad_masks)):
            steps[k].append(v.numpy().copy())
        obs_s = utils.mirror_obsact_batch(obs, False, mirror_obs, augment=True)
        action_s = utils.mirror_obsact_batch(action, False, mirror_action, augment=True)
        recurrent_hidden_states_s = recurrent_hidden_states.repeat(2, 1)
        action_log_prob_s = action_log_prob.repeat(2, 1)
        value_s = value.repeat(2, 1)
        reward_s = reward.repeat(2, 1)
        masks_s = masks.repeat(2, 1)
        bad_masks_s = bad_masks.repeat(2, 1)
        obs_feat_s = obs_feat.repeat(2, 1)
        rollouts.insert(obs_s, recurrent_hidden_states_s, action_s,
                        action_log_prob_s, value_s, reward_s, masks_s, bad_masks_s, obs_feat_s)
    fields = {"out_" + k: getattr(rollouts, k).numpy().copy() for k in
              ("obs", "obs_feat", "recurrent_hidden_states", "actions", "action_log_probs", "value_preds", "rewards", "masks", "bad_masks")}
    meta = np.frombuffer(json.dumps({"O": O, "A": A, "T": T, "n": n, "hidden": hidden, "feat_len": int(feat_len)}).encode(), dtype=np.uint8)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, meta=meta, m_obs=m_obs, m_act=m_act, **inputs, **{"step_" + k: np.stack(v) for k, v in steps.items()}, **fields)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def dense_matrix(w, seed):
    """Neither symmetric nor an involution."""
    m = np.random.default_rng(seed).standard_normal((w, w))
    assert not np.allclose(m, m.T) and not np.allclose(m @ m, np.eye(w))
    return m


if __name__ == "__main__":
    ns = ref_import.import_reference()
    from simgan_amd.symmetry import laikago_mirror
    lo, la = laikago_mirror(37)
    gen("dup_sym_laikago", ns, O=37, A=12, T=3, n=2, hidden=1, m_obs=lo, m_act=la, seed=810)
    gen("dup_sym_dense", ns, O=5, A=2, T=3, n=3, hidden=4, m_obs=dense_matrix(5, 821), m_act=dense_matrix(2, 822), seed=820)
