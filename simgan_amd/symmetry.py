"""Mirror maps for PPO's mirror-symmetry loss (a2c/algo/ppo.py:110-143, a2c/main.py:133-146).

The reference hands PPO two per-row callables, `mirror_obs` and `mirror_act`, and applies them row by row through
mirror_obsact_batch (my_pybullet_envs/utils.py:334-357).  On the GPU the action mirror is a matrix M_a ([A, A], row-major:
mirrored = M_a @ a); the observation mirror is either a matrix too (every step on the device) or the callable itself, applied
on the host once per update.

laikago_mirror() gives the Laikago mirrors (my_pybullet_envs/laikago.py:437-497) as matrices.  They are exactly linear: per
37-float step block the root rotation R (row-major, obs[1:10]) goes to Rz(3.14159) F R F with F = diag(-1, 1, 1) -- the
reference's Euler round trip (roll, -pitch, 3.14159 - yaw) -- and every other entry is a sign flip or a left / right swap.
"""
import numpy as np

_LAIKAGO_BLOCK = 37
_LAIKAGO_YAW = 3.14159   # my_pybullet_envs/laikago.py: root_rpy_m = [r, -p, 3.14159 - y]


def _swap_halves(m, base):
    """mirror_leg_q on entries [base, base + 6): the two 3-vectors trade places."""
    for k in range(6):
        m[base + k, base + (k + 3) % 6] = 1.0


def _laikago_step_block():
    m = np.zeros((_LAIKAGO_BLOCK, _LAIKAGO_BLOCK), np.float64)
    m[0, 0] = 1.0                                    # root z
    c, s = np.cos(_LAIKAGO_YAW), np.sin(_LAIKAGO_YAW)
    rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    f = np.array([-1.0, 1.0, 1.0])
    for i in range(3):                               # R_m[i, j] = sum_k Rz[i, k] f_k R[k, j] f_j
        for j in range(3):
            for k in range(3):
                m[1 + 3 * i + j, 1 + 3 * k + j] = rz[i, k] * f[k] * f[j]
    m[10, 10], m[11, 11], m[12, 12] = 1.0, -1.0, 1.0   # root linear velocity
    _swap_halves(m, 13)                              # joint q, two groups of 6
    _swap_halves(m, 19)
    for base in (25, 31):                            # mirror_foot_pos: [l0, -l1, l2, r0, -r1, r2]
        for k in range(6):
            m[base + k, base + (k + 3) % 6] = -1.0 if k % 3 == 1 else 1.0
    return m


def laikago_mirror(obs_dim=111):
    """-> (M_obs [obs_dim, obs_dim], M_act [12, 12]) float32: my_pybullet_envs/laikago.py mirror_obs / mirror_action as
    matrices (obs_dim a multiple of the 37-float step block, as mirror_obs asserts)."""
    if obs_dim <= 0 or obs_dim % _LAIKAGO_BLOCK:
        raise ValueError(f"laikago_mirror: obs_dim {obs_dim} is not a multiple of {_LAIKAGO_BLOCK}")
    blk = _laikago_step_block()
    m_obs = np.zeros((obs_dim, obs_dim), np.float64)
    for b in range(obs_dim // _LAIKAGO_BLOCK):
        sl = slice(b * _LAIKAGO_BLOCK, (b + 1) * _LAIKAGO_BLOCK)
        m_obs[sl, sl] = blk
    m_act = np.zeros((12, 12), np.float64)
    _swap_halves(m_act, 0)
    _swap_halves(m_act, 6)
    return m_obs.astype(np.float32), m_act.astype(np.float32)


def as_matrix(m, n, what):
    """A mirror given as a matrix -> float32 [n, n] C-contiguous."""
    a = np.ascontiguousarray(np.asarray(m, np.float32))
    if a.shape != (n, n):
        raise ValueError(f"{what}: a mirror matrix must be [{n}, {n}], got {list(a.shape)}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what}: the mirror matrix holds non-finite entries")
    return a


def probe_linear(fn, n, what, trials=8, seed=0):
    """A per-row mirror callable -> its matrix [n, n] float32, probed on the identity basis and then checked on random
    vectors: a callable that is not linear raises ValueError."""
    cols = [np.asarray(fn(e), np.float64).reshape(-1) for e in np.eye(n)]
    if any(c.shape != (n,) for c in cols):
        raise ValueError(f"{what}: the mirror must map a {n}-vector to a {n}-vector")
    m = np.stack(cols, axis=1)
    rng = np.random.default_rng(seed)
    for _ in range(trials):
        x = rng.standard_normal(n)
        y = np.asarray(fn(x), np.float64).reshape(-1)
        want = m @ x
        if not np.allclose(y, want, rtol=1e-5, atol=1e-6 * (1.0 + np.abs(x).max())):
            raise ValueError(f"{what}: the mirror callable is not linear (max deviation {np.abs(y - want).max():.3g} from its "
                             "probed matrix); pass a linear map")
    return as_matrix(m, n, what)


def matrix_rows(m, rows):
    """M x for every row of `rows` ([R, n] float32) with the device kernels' arithmetic (k_mirror_rows, k_dup_sym): the float32
    entries widened to float64, the products summed over ascending j, zero entries of M skipped, one cast to float32.  A
    signed permutation is exact; a dense M gives the bits the device gives."""
    m = np.asarray(m, np.float32)
    x = np.asarray(rows, np.float32)
    x = x.reshape(-1, m.shape[1]).astype(np.float64)
    out = np.zeros((x.shape[0], m.shape[0]), np.float64)
    for j in range(m.shape[1]):
        col = m[:, j].astype(np.float64)
        nz = col != 0.0
        if nz.any():
            out[:, nz] = out[:, nz] + x[:, j:j + 1] * col[nz]
    return np.ascontiguousarray(out.astype(np.float32))


def mirror_rows(fn, rows):
    """mirror_obsact_batch(rows, ..., fn, augment=False) (my_pybullet_envs/utils.py:334-357): fn on every row, float32."""
    out = np.asarray([np.asarray(fn(r), np.float64).reshape(-1) for r in rows], np.float32)
    return np.ascontiguousarray(out.reshape(len(rows), -1))
