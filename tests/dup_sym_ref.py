"""Mirror-augmented rollouts (a2c/main.py:171-245, --dup-sym) restated in numpy: the arbiter of tests/test_dup_sym_host.py
(pinned on the reference-written fixtures tests/golden/dup_sym_*.npz) and of tests/test_gpu_dup_sym.py.

The contract: the rollout has N = 2n columns, [0, n) the environments and column n + j the mirror image of column j.  Slot 0
of obs is cat(obs, mirror_obs(obs)) and of obs_feat the features repeated (:181-185); every step inserts cat(obs,
mirror_obs(obs)) and cat(action, mirror_action(action)) and REPEATS recurrent_hidden_states, action_log_probs, value_preds,
rewards, masks, bad_masks and obs_feat (:231-242) -- obs_feat too, although it is a copy of the observation.

A linear mirror is M x with the device kernels' arithmetic: float32 entries widened to float64, the products summed over
ascending j, zero entries of M skipped, one cast to float32."""
import numpy as np

STEP_KEYS = ("obs", "obs_feat", "hxs", "actions", "logp", "value", "reward", "masks", "bad_masks")
FIELDS = ("obs", "obs_feat", "recurrent_hidden_states", "actions", "action_log_probs", "value_preds", "rewards", "masks", "bad_masks")


def products(m, rows):
    """[R, n_out, n_in] float64: M[i][j] * x[r][j], exact (two float32 factors)."""
    m = np.asarray(m, np.float32).astype(np.float64)
    x = np.asarray(rows, np.float32).astype(np.float64)
    return m[None, :, :] * x[:, None, :]


def mirror64(m, rows):
    """The float64 sum before any cast: ascending j, zero entries of M skipped."""
    p = products(m, rows)
    keep = np.asarray(m, np.float32) != 0
    s = np.zeros(p.shape[:2], np.float64)
    for j in range(p.shape[2]):
        s = np.where(keep[None, :, j], s + p[:, :, j], s)
    return s


def mirror(m, rows):
    return mirror64(m, rows).astype(np.float32)


def mirror_bound(m, rows):
    """|got - want| <= 2^-24 |want| + n 2^-53 sum_j |M_ij x_j|: the one cast plus the accumulation's own bound."""
    p = np.abs(products(m, rows))
    return 2.0 ** -24 * np.abs(mirror64(m, rows)) + p.shape[2] * 2.0 ** -53 * p.sum(axis=2)


def restate(obs0, feat0, steps, m_obs, m_act, hidden=1, variant=None, mirror_obs_fn=None):
    """-> the 2n-wide fields of the reference's RolloutStorage(T, 2n, ...) after slot 0 and T inserts.  obs0 [n, O], feat0
    [n, F]; steps: {key: [T, n, width]} for STEP_KEYS.  mirror_obs_fn: rows -> mirrored rows instead of m_obs (a callable mirror).
    variant: a deliberately WRONG restatement (the tests show each fails against the fixtures): "mirror_feat" mirrors obs_feat
    as well, "repeat_actions" repeats the actions unmirrored, "transpose_act" applies M_act transposed."""
    f32 = lambda a: np.asarray(a, np.float32)  # noqa: E731
    mo = mirror_obs_fn if mirror_obs_fn is not None else (lambda rows: mirror(m_obs, rows))
    ma = np.asarray(m_act, np.float32)
    if variant == "transpose_act":
        ma = ma.T
    aug_obs = lambda r: np.concatenate([f32(r), mo(f32(r))])  # noqa: E731
    rep = lambda r: np.concatenate([f32(r), f32(r)])  # noqa: E731
    aug_feat = aug_obs if variant == "mirror_feat" else rep
    aug_act = rep if variant == "repeat_actions" else (lambda r: np.concatenate([f32(r), mirror(ma, f32(r))]))
    T, n = steps["obs"].shape[:2]
    O, F, A = obs0.shape[1], feat0.shape[1], steps["actions"].shape[2]
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    out = {"obs": z(T + 1, 2 * n, O), "obs_feat": z(T + 1, 2 * n, F), "recurrent_hidden_states": z(T + 1, 2 * n, hidden),
           "actions": z(T, 2 * n, A), "action_log_probs": z(T, 2 * n, 1), "value_preds": z(T + 1, 2 * n, 1),
           "rewards": z(T, 2 * n, 1), "masks": np.ones((T + 1, 2 * n, 1), np.float32),
           "bad_masks": np.ones((T + 1, 2 * n, 1), np.float32)}
    out["obs"][0] = aug_obs(obs0)
    out["obs_feat"][0] = aug_feat(feat0)
    for t in range(T):
        out["obs"][t + 1] = aug_obs(steps["obs"][t])
        out["obs_feat"][t + 1] = aug_feat(steps["obs_feat"][t])
        out["recurrent_hidden_states"][t + 1] = rep(steps["hxs"][t])
        out["actions"][t] = aug_act(steps["actions"][t])
        out["action_log_probs"][t] = rep(steps["logp"][t])
        out["value_preds"][t] = rep(steps["value"][t])
        out["rewards"][t] = rep(steps["reward"][t])
        out["masks"][t + 1] = rep(steps["masks"][t])
        out["bad_masks"][t + 1] = rep(steps["bad_masks"][t])
    return out


def random_steps(rng, T, n, O, A, F, hidden=1):
    """Per-step inputs of a rollout fill: n rows each."""
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return {"obs": f(T, n, O), "obs_feat": f(T, n, F), "hxs": f(T, n, hidden), "actions": f(T, n, A), "logp": f(T, n, 1),
            "value": f(T, n, 1), "reward": f(T, n, 1), "masks": (rng.random((T, n, 1)) > 0.2).astype(np.float32),
            "bad_masks": (rng.random((T, n, 1)) > 0.1).astype(np.float32)}


def signed_permutation(rng, w):
    m = np.zeros((w, w), np.float32)
    m[np.arange(w), rng.permutation(w)] = rng.choice([-1.0, 1.0], w)
    return m


def dense(rng, w):
    """Neither symmetric nor an involution, a few exact zeros."""
    m = rng.standard_normal((w, w)).astype(np.float32)
    m[rng.random((w, w)) < 0.15] = 0.0
    return m
