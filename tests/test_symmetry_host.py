"""CPU: the mirror-symmetry loss's host side (simgan_amd/symmetry.py, the PPO constructor) and a restatement of the reference's
symmetric PPO update (a2c/algo/ppo.py:110-143) that the GPU tests measure the kernels against.

The restatement: the CPU oracle's PPO gradient of every minibatch plus the symmetry term in float64 numpy, then the oracle's
clip + Adam.  The symmetry term is coef * mean((M_a mu(s) - mu(s_m))^2) with M_a mu(s) a constant (the reference mirrors it
through numpy: my_pybullet_envs/utils.py:334-357), so its gradient flows through the actor on the mirrored rows only."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from helpers import assert_close, load  # noqa: E402

SYM_CASES = ["ppo_sym_small", "ppo_sym_laikago", "ppo_sym_nonlinear"]


# ------------------------------------------------------------------ restatement
def actor_slices(O, A, H):
    """Offsets of the actor's tensors in the flat state_dict order of Policy (a2c/model.py:233-264)."""
    n = {}
    off = 0
    for key, size in (("w1", H * O), ("b1", H), ("w2", H * H), ("b2", H)):
        n[key] = slice(off, off + size)
        off += size
    off += H * O + H + H * H + H + H + 1          # critic trunk + critic_linear
    n["wh"] = slice(off, off + A * H)
    off += A * H
    n["bh"] = slice(off, off + A)
    return n


def actor_mean(params, x, O, A, H):
    """fc_mean(actor(x)) in float64 -> (mu, h1, h2)."""
    s = actor_slices(O, A, H)
    p = np.asarray(params, np.float64)
    h1 = np.tanh(x @ p[s["w1"]].reshape(H, O).T + p[s["b1"]])
    h2 = np.tanh(h1 @ p[s["w2"]].reshape(H, H).T + p[s["b2"]])
    return h2 @ p[s["wh"]].reshape(A, H).T + p[s["bh"]], h1, h2


def sym_loss_grad(params, x, xm, m_act, coef, O, A, H):
    """(coef-free symmetry loss mean(e^2), d(coef * loss)/d params) for one minibatch, float64."""
    x, xm = np.asarray(x, np.float64), np.asarray(xm, np.float64)
    mu, _, _ = actor_mean(params, x, O, A, H)
    mum, h1, h2 = actor_mean(params, xm, O, A, H)
    e = mu @ np.asarray(m_act, np.float64).T - mum
    B = x.shape[0]
    d = -coef * 2.0 / (B * A) * e                 # d / d mu(s_m)
    s = actor_slices(O, A, H)
    p = np.asarray(params, np.float64)
    g = np.zeros(p.size)
    g[s["wh"]] = (d.T @ h2).reshape(-1)
    g[s["bh"]] = d.sum(0)
    dz2 = (d @ p[s["wh"]].reshape(A, H)) * (1.0 - h2 * h2)
    g[s["w2"]] = (dz2.T @ h1).reshape(-1)
    g[s["b2"]] = dz2.sum(0)
    dz1 = (dz2 @ p[s["w2"]].reshape(H, H)) * (1.0 - h1 * h1)
    g[s["w1"]] = (dz1.T @ xm).reshape(-1)
    g[s["b1"]] = dz1.sum(0)
    return float(np.mean(e * e)), g


def sym_update_restated(g, mirrored_rows, params0=None, adam=None, perms=None):
    """One reference update of fixture-shaped problem `g` with the symmetry loss: (params1, adam, losses[3], mean sym loss).
    mirrored_rows: [T*N, O] the mirrored observations of the rollout's first T steps."""
    from oracle import oracle as orc
    m = g["meta"]
    O, A, H, T, N, E, M = (m[k] for k in ("O", "A", "H", "T", "N", "ppo_epoch", "num_mini_batch"))
    d = orc.dims(orc.KIND_MLP, O, A, H, 1)
    cfg = orc.ppo_cfg(m["clip_param"], E, M, m["value_loss_coef"], m["entropy_coef"], m["lr"], m["eps"], m["max_grad_norm"], True)
    par = np.array(g["params0"] if params0 is None else params0, np.float32)
    adam = adam or orc.AdamState(par.size)
    perms = g["perms"] if perms is None else perms
    obs = np.ascontiguousarray(g["obs"], np.float32)
    obs_rows = obs.reshape(-1, O)[:T * N]
    adv = orc.advantages(g["returns"][:-1], g["value_preds"][:-1])
    mb = T * N // M
    losses, sym = np.zeros(3), 0.0
    for e in range(E):
        for k in range(M):
            rows = np.ascontiguousarray(perms[e][k * mb:(k + 1) * mb], np.int64)
            G, sums = orc.ppo_grad_rows(d, par, cfg, obs, g["actions"], g["value_preds"], g["returns"], g["action_log_probs"], adv,
                                        rows, 1.0 / mb)
            ls, gs = sym_loss_grad(par, obs_rows[rows], mirrored_rows[rows], g["m_act"], m["symmetry_coef"], O, A, H)
            G = (np.asarray(G, np.float64) + gs).astype(np.float32)
            orc.ppo_apply(par, G, adam, cfg)
            losses += np.asarray(sums) / mb
            sym += ls
    return par, adam, losses / (E * M), sym / (E * M)


def nonlinear_obs(x):
    """tools/gen_golden_symmetry.py nonlinear_obs, restated: the small fixture's matrix plus 0.25 sin of the reversed row."""
    x = np.asarray(x, np.float64)
    return load_small_obs_matrix() @ x + 0.25 * np.sin(x[::-1])


def load_small_obs_matrix():
    return np.asarray(load("ppo_sym_small")["m_obs"], np.float64)


def mirrored_rows_of(g):
    m = g["meta"]
    rows = np.asarray(g["obs"], np.float32).reshape(-1, m["O"])[:m["T"] * m["N"]]
    if "m_obs" in g:
        return (rows.astype(np.float64) @ np.asarray(g["m_obs"], np.float64).T).astype(np.float32)
    return np.asarray([nonlinear_obs(r) for r in rows], np.float32)


@pytest.mark.parametrize("name", SYM_CASES)
def test_restatement_reproduces_the_reference_fixture(name):
    """The oracle + float64 symmetry restatement lands on the reference's own update (guards the restatement the GPU tests use,
    and the semantics: no gradient through the mirrored M_a mu(s))."""
    g = load(name)
    m = g["meta"]
    par, adam, losses, sym = sym_update_restated(g, mirrored_rows_of(g))
    assert_close(losses, g["losses"], what="losses")
    assert_close(par, g["params1"], what="params after update")
    assert_close(adam.m, g["adam_m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert sym > 0.0 and m["symmetry_coef"] > 0


# ------------------------------------------------------------------ mirrors
def test_laikago_mirror_matches_the_euler_round_trip():
    """laikago_mirror's rotation block against a scipy restatement of mirror_obs_per_step's Euler round trip
    (my_pybullet_envs/laikago.py:451-483: rpy -> (r, -p, 3.14159 - y)) on random rotations; the other entries exactly."""
    Rot = pytest.importorskip("scipy.spatial.transform").Rotation
    from simgan_amd.symmetry import laikago_mirror
    m_obs, m_act = laikago_mirror(111)
    assert m_obs.shape == (111, 111) and m_act.shape == (12, 12)
    rng = np.random.default_rng(3)

    def euler_mirror_block(x):
        out = np.array(x, np.float64)
        rpy = Rot.from_matrix(np.asarray(x[1:10]).reshape(3, 3)).as_euler("xyz")
        out[1:10] = Rot.from_euler("xyz", [rpy[0], -rpy[1], 3.14159 - rpy[2]]).as_matrix().reshape(-1)
        out[10:13] = [x[10], -x[11], x[12]]
        for base in (13, 19):
            out[base:base + 6] = list(x[base + 3:base + 6]) + list(x[base:base + 3])
        for base in (25, 31):
            r, l_ = x[base:base + 3], x[base + 3:base + 6]
            out[base:base + 6] = [l_[0], -l_[1], l_[2], r[0], -r[1], r[2]]
        return out

    worst = 0.0
    for _ in range(200):
        x = rng.standard_normal(111)
        for b in range(3):
            x[37 * b + 1:37 * b + 10] = Rot.random(random_state=rng.integers(1 << 30)).as_matrix().reshape(-1)
        want = np.concatenate([euler_mirror_block(x[37 * b:37 * (b + 1)]) for b in range(3)])
        worst = max(worst, float(np.abs(m_obs.astype(np.float64) @ x - want).max()))
    assert worst < 2e-6, worst   # float32 matrix entries (sin 3.14159 = 2.65e-6 rounds at 1e-13 relative)
    a = rng.standard_normal(12).astype(np.float32)
    assert np.array_equal(m_act @ a, np.concatenate([a[3:6], a[0:3], a[9:12], a[6:9]]))


def test_laikago_mirror_is_an_involution_up_to_the_yaw_constant():
    from simgan_amd.symmetry import laikago_mirror
    m_obs, m_act = laikago_mirror(37)
    assert np.array_equal(m_act @ m_act, np.eye(12, dtype=np.float32))
    assert np.abs(m_obs.astype(np.float64) @ m_obs - np.eye(37)).max() < 1e-5
    with pytest.raises(ValueError):
        laikago_mirror(40)


def test_mirror_act_probe_recovers_the_matrix():
    from simgan_amd.symmetry import probe_linear
    rng = np.random.default_rng(0)
    m = rng.standard_normal((5, 5))
    got = probe_linear(lambda x: list(m @ np.asarray(x)), 5, "mirror_act")
    assert got.dtype == np.float32 and got.shape == (5, 5)
    assert np.array_equal(got, m.astype(np.float32))
    perm = lambda x: list(x[3:6]) + list(x[:3])   # noqa: E731  (mirror_leg_q)
    assert np.array_equal(probe_linear(perm, 6, "mirror_act") @ np.arange(6, dtype=np.float32), [3, 4, 5, 0, 1, 2])


def test_mirror_act_probe_rejects_nonlinear_and_misshapen_maps():
    from simgan_amd.symmetry import as_matrix, probe_linear
    with pytest.raises(ValueError, match="not linear"):
        probe_linear(lambda x: np.tanh(np.asarray(x) * 3.0), 4, "mirror_act")
    with pytest.raises(ValueError, match="not linear"):
        probe_linear(lambda x: np.asarray(x) + 0.5, 4, "mirror_act")   # affine
    with pytest.raises(ValueError):
        probe_linear(lambda x: list(x)[:3], 4, "mirror_act")
    with pytest.raises(ValueError):
        as_matrix(np.eye(3), 4, "mirror_obs")


def test_mirror_rows_matches_the_reference_batch_helper():
    from simgan_amd.symmetry import mirror_rows
    rows = np.random.default_rng(1).standard_normal((7, 6)).astype(np.float32)
    out = mirror_rows(nonlinear_obs, rows)
    assert out.dtype == np.float32 and out.shape == (7, 6)
    assert np.array_equal(out, np.asarray([list(nonlinear_obs(r)) for r in rows], np.float32))


# ------------------------------------------------------------------ constructor (no device call is reached)
class _FakePolicy:
    obs_dim, act_dim = 6, 4


class _FakeSplit(_FakePolicy):
    pass


_FakeSplit.__name__ = "SplitPolicy"


def _bare_ppo():
    from simgan_amd.algo.ppo import PPO
    return PPO.__new__(PPO)


def test_symmetry_without_mirror_act_raises():
    agent = _bare_ppo()
    agent.actor_critic = _FakePolicy()
    with pytest.raises(ValueError, match="without mirror_act"):
        agent._set_symmetry(0.5, np.eye(6), None)


def test_symmetry_with_nonlinear_mirror_act_raises():
    agent = _bare_ppo()
    agent.actor_critic = _FakePolicy()
    with pytest.raises(ValueError, match="not linear"):
        agent._set_symmetry(0.5, np.eye(6), lambda a: np.abs(np.asarray(a)))


def test_symmetry_on_split_policy_is_not_implemented():
    agent = _bare_ppo()
    agent.actor_critic = _FakeSplit()
    with pytest.raises(NotImplementedError, match="SplitPolicy"):
        agent._set_symmetry(0.5, np.eye(6), np.eye(4))


# ------------------------------------------------------------------ C ABI
def test_symmetry_abi_is_declared_exported_and_prototyped():
    import ctypes
    from simgan_amd import _lib
    header = open(os.path.join(ROOT, "include", "simgan_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym in ("sg_ppo_set_symmetry", "sg_ppo_set_mirrored_obs", "sg_ppo_last_symmetry_loss"):
        assert f"{sym}(" in header
        assert hasattr(lib, sym)
        assert sym in _lib.PROTOTYPES
