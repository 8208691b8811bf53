"""GPU: mirror-augmented rollouts (a2c/main.py:171-245, --dup-sym) -- k_dup_sym, sg_rollout_upload_columns,
RolloutStorage.insert_dup_sym and PpoLearner(dup_sym=...) -- against the numpy restatement tests/dup_sym_ref.py, which
tests/test_dup_sym_host.py pins on the reference-written fixtures."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dup_sym_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

ATTRS = ("obs", "obs_feat", "actions", "rewards", "value_preds", "returns", "action_log_probs", "masks", "bad_masks")


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def npv(t):
    return t.numpy() if hasattr(t, "numpy") else t


def fields_of(ro, attrs=ATTRS + ("recurrent_hidden_states",)):
    return {k: npv(getattr(ro, k)).copy() for k in attrs}


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 17, 65])
@pytest.mark.parametrize("O,A", [(5, 2), (37, 12), (111, 12)])
def test_kernel_against_the_restatement(sg, T, n, O, A):
    """sg_rollout_dup_sym on a rollout whose every float is a sentinel: the mirrored half of the slots it owns equals the
    restatement -- bit for bit with signed-permutation mirrors, within the cast plus the accumulation's own bound with dense
    ones -- and columns [0, n), VALUE_PREDS[T], RETURNS and ADVANTAGES are untouched.  n = 1 with O = 5 puts the mirrored half
    at float 5 of a row: no 16-byte alignment to lean on; n = 65 takes several tiles per slot; O = 111 stages a 48 KiB mirror."""
    from simgan_amd import _lib
    rng = np.random.default_rng(1000 * T + 10 * n + O)
    for F in (0, O):
        for kind in ("perm", "dense"):
            make = ref.signed_permutation if kind == "perm" else ref.dense
            m_obs, m_act = make(rng, O), make(rng, A)
            ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), 1, F)
            for k in ATTRS:
                t = getattr(ro, k)
                if t.numel():
                    t.copy_(t.new_tensor((rng.standard_normal(tuple(t.shape)) * 3.0 + 40.0).astype(np.float32)))   # sentinels: no zero, no one
            ro.sync_to_device()
            before = fields_of(ro, ATTRS)
            adv0 = npv(ro.device_advantages()).copy()
            _lib.check(ro.lib.sg_rollout_set_mirrors(ro.h, _lib.fptr(m_obs), _lib.fptr(m_act)))
            _lib.check(ro.lib.sg_rollout_dup_sym(ro.h))
            ro.sync_from_device()
            got = fields_of(ro, ATTRS)
            what = f"T={T} n={n} O={O} A={A} F={F} {kind}"
            assert np.array_equal(got["returns"], before["returns"]), what
            assert np.array_equal(npv(ro.device_advantages()), adv0), what
            assert np.array_equal(got["value_preds"][T], before["value_preds"][T]), what
            for k in ATTRS:
                assert np.array_equal(got[k][:, :n], before[k][:, :n]), (what, k)
            for k, m in (("obs", m_obs), ("actions", m_act)):
                src = before[k][:, :n].reshape(-1, m.shape[0])
                out = got[k][:, n:].reshape(-1, m.shape[0])
                if kind == "perm":
                    assert np.array_equal(out, ref.mirror(m, src)), (what, k)
                else:
                    err = np.abs(out.astype(np.float64) - ref.mirror64(m, src))
                    assert np.all(err <= ref.mirror_bound(m, src)), (what, k, float(err.max()))
            for k, slots in (("obs_feat", T + 1), ("masks", T + 1), ("bad_masks", T + 1), ("rewards", T), ("action_log_probs", T),
                             ("value_preds", T)):
                assert np.array_equal(got[k][:slots, n:], before[k][:slots, :n]), (what, k)


def test_kernel_without_an_obs_mirror_leaves_obs_alone(sg):
    """m_obs NULL (the caller mirrors observations itself): OBS is not touched, everything else as before."""
    from simgan_amd import _lib
    rng = np.random.default_rng(5)
    T, n, O, A = 2, 3, 7, 4
    ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), 1, O)
    for k in ATTRS:
        t = getattr(ro, k)
        t.copy_(t.new_tensor(rng.standard_normal(tuple(t.shape)).astype(np.float32)))
    ro.sync_to_device()
    before = fields_of(ro, ATTRS)
    m_act = ref.dense(rng, A)
    _lib.check(ro.lib.sg_rollout_set_mirrors(ro.h, None, _lib.fptr(m_act)))
    _lib.check(ro.lib.sg_rollout_dup_sym(ro.h))
    ro.sync_from_device()
    got = fields_of(ro, ATTRS)
    assert np.array_equal(got["obs"], before["obs"])
    assert np.array_equal(got["actions"][:, n:].reshape(-1, A), ref.mirror(m_act, before["actions"][:, :n].reshape(-1, A)))
    assert np.array_equal(got["obs_feat"][:, n:], before["obs_feat"][:, :n])


# ------------------------------------------------------------------------------------------ the rollout
def fill_dup(ro, obs0, feat0, steps):
    ro.set_initial_obs_dup_sym(obs0, feat0)
    T = steps["obs"].shape[0]
    for t in range(T):
        ro.insert_dup_sym(steps["obs"][t], steps["hxs"][t], steps["actions"][t], steps["logp"][t], steps["value"][t],
                          steps["reward"][t], steps["masks"][t], steps["bad_masks"][t], steps["obs_feat"][t])


def fill_plain(ro, want):
    for k, a in want.items():
        t = getattr(ro, k)
        t.copy_(t.new_tensor(a))


def case(rng, T, n, O, A, hidden=1, dense=True):
    make = ref.dense if dense else ref.signed_permutation
    obs0 = rng.standard_normal((n, O)).astype(np.float32)
    steps = ref.random_steps(rng, T, n, O, A, O, hidden)
    return obs0, obs0.copy(), steps, make(rng, O), make(rng, A)


def test_the_mirrored_half_never_crosses_the_link(sg):
    """Device-resident: the host tensors' mirrored halves are NaN when sync_to_device() runs; the device fields hold the
    restatement and no NaN, and bytes_uploaded grew by the first halves only."""
    rng = np.random.default_rng(11)
    T, n, O, A = 3, 5, 9, 4
    obs0, feat0, steps, m_obs, m_act = case(rng, T, n, O, A)
    ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), 1, O)
    ro.device_resident = True
    ro.enable_dup_sym(m_obs, m_act)
    fill_dup(ro, obs0, feat0, steps)
    for k in ATTRS:
        npv(getattr(ro, k))[:, n:] = np.nan
    first_halves = sum(npv(getattr(ro, k)).nbytes // 2 for k in ATTRS)
    b0 = ro.bytes_uploaded
    ro.sync_to_device()
    assert ro.bytes_uploaded - b0 == first_halves
    ro.sync_from_device()
    got = fields_of(ro, ATTRS)
    want = ref.restate(obs0, feat0, steps, m_obs, m_act)
    for k in ATTRS:
        assert not np.isnan(got[k]).any(), k
        if k != "returns":
            assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("dense", [False, True])
def test_host_mode_and_device_resident_mode_leave_identical_bits(sg, dense):
    rng = np.random.default_rng(12)
    T, n, O, A, Hs = 3, 17, 37, 12, 6
    obs0, feat0, steps, m_obs, m_act = case(rng, T, n, O, A, Hs, dense)
    out = []
    for resident in (False, True):
        ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), Hs, O)
        ro.device_resident = resident
        ro.enable_dup_sym(m_obs, m_act)
        fill_dup(ro, obs0, feat0, steps)
        if resident:
            ro.sync_to_device()
            ro.sync_from_device()
        out.append(fields_of(ro))
    want = ref.restate(obs0, feat0, steps, m_obs, m_act, hidden=Hs)
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
        if k != "returns":
            assert np.array_equal(out[0][k], want[k]), k


def nonlinear_obs(x):
    x = np.asarray(x, np.float64)
    return list(x[::-1] + 0.25 * np.sin(x))


@pytest.mark.parametrize("resident", [False, True])
def test_a_callable_mirror_obs_runs_on_the_host_in_both_modes(sg, resident):
    """A nonlinear per-row callable: OBS is mirrored through symmetry.mirror_rows and, device-resident, uploaded full-width."""
    from simgan_amd import symmetry
    rng = np.random.default_rng(13)
    T, n, O, A = 2, 3, 5, 2
    obs0, feat0, steps, _, m_act = case(rng, T, n, O, A)
    ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), 1, O)
    ro.device_resident = resident
    ro.enable_dup_sym(nonlinear_obs, lambda a: list(m_act.astype(np.float64) @ np.asarray(a, np.float64)))
    fill_dup(ro, obs0, feat0, steps)
    if resident:
        b0 = ro.bytes_uploaded
        ro.sync_to_device()
        others = sum(npv(getattr(ro, k)).nbytes // 2 for k in ATTRS if k != "obs")
        assert ro.bytes_uploaded - b0 == others + npv(ro.obs).nbytes
        npv(ro.obs)[...] = np.nan
        ro.sync_from_device()
    want = ref.restate(obs0, feat0, steps, None, m_act, mirror_obs_fn=lambda rows: symmetry.mirror_rows(nonlinear_obs, rows))
    got = fields_of(ro, ATTRS)
    for k in ATTRS:
        if k != "returns":
            assert np.array_equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------ updates
def make_policy(sg, O, A, H, recurrent, seed=3):
    return sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": recurrent, "hidden_size": H}, seed=seed)


def policy_steps(p, rng, T, n, O, A, obs0):
    """A rollout fill's per-step inputs with the policy's own actions, values, log-probs and states."""
    Hs = p.recurrent_hidden_state_size
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    steps = ref.random_steps(rng, T, n, O, A, O, Hs)
    obs, hxs, masks = obs0, np.zeros((n, Hs), np.float32), np.ones((n, 1), np.float32)
    for t in range(T):
        v, a, lp, h = p.act(obs, hxs, masks, noise=f(n, A))
        steps["value"][t], steps["actions"][t], steps["logp"][t] = npv(v), npv(a), npv(lp)
        steps["hxs"][t] = npv(h).reshape(n, Hs) if p.is_recurrent else 0.0
        steps["obs_feat"][t] = steps["obs"][t]
        obs, hxs, masks = steps["obs"][t], steps["hxs"][t], steps["masks"][t]
    return steps


UPDATE_CASES = [("ppo", False), ("ppo", True), ("ppo_sym", False), ("a2c", False)]


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("algo,recurrent", UPDATE_CASES)
def test_update_on_a_dup_sym_rollout_equals_the_update_on_the_plain_2n_rollout(sg, algo, recurrent, resident):
    """The same update on a rollout filled through insert_dup_sym and on a plain 2n-column rollout filled from the
    restatement: losses, parameters and optimizer state are bitwise equal (hidden states repeated for the recurrent policy)."""
    O, A, H, T, n = (13, 5, 20, 3, 2) if recurrent else (5, 2, 8, 3, 3)
    rng = np.random.default_rng(21)
    m_obs, m_act = ref.dense(rng, O), ref.dense(rng, A)
    p0 = make_policy(sg, O, A, H, recurrent)
    Hs = p0.recurrent_hidden_state_size
    obs0 = rng.standard_normal((n, O)).astype(np.float32)
    steps = policy_steps(p0, rng, T, n, O, A, obs0)
    want = ref.restate(obs0, obs0, steps, m_obs, m_act, hidden=Hs)
    params0 = (p0.get_flat_params() + 0.02 * rng.standard_normal(p0.num_params)).astype(np.float32)
    next_value = rng.standard_normal((2 * n, 1)).astype(np.float32)
    E, M = 2, 2
    perms = np.stack([rng.permutation(2 * n if recurrent else T * 2 * n) for _ in range(E)]).astype(np.int64)
    results = []
    for which in ("dup", "plain"):
        p = make_policy(sg, O, A, H, recurrent)
        p.set_flat_params(params0)
        ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), Hs, O)
        if which == "dup":
            ro.device_resident = resident
            ro.enable_dup_sym(m_obs, m_act)
            fill_dup(ro, obs0, obs0, steps)
            if resident:
                ro.sync_to_device()
        else:
            fill_plain(ro, want)
        ro.compute_returns(next_value, True, 0.99, 0.95, True)
        if algo == "a2c":
            agent = sg.algo.A2C_ACKTR(p, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, acktr=False)
            losses = agent.update(ro)
            sq, step = agent.get_rmsprop()
            state = [sq, np.array(step)]
        else:
            kw = dict(symmetry_coef=0.5, mirror_obs=m_obs, mirror_act=m_act) if algo == "ppo_sym" else {}
            agent = sg.algo.PPO(p, 0.2, E, M, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5, **kw)
            losses = agent.update(ro, perms=perms)
            mm, vv, step = agent.get_adam()
            state = [mm, vv, np.array(step)]
        results.append((np.asarray(losses, np.float64), p.get_flat_params(), state))
    (l0, q0, s0), (l1, q1, s1) = results
    assert np.isfinite(l0).all() and not np.array_equal(q0, params0)
    assert np.array_equal(l0, l1), (l0, l1)
    assert np.array_equal(q0, q1)
    for a, b in zip(s0, s1):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ the learner
class StubEnvs:
    """Deterministic: the next observation, reward and flags are functions of the action and a seeded stream."""

    def __init__(self, n, O, seed):
        self.num_envs, self.O, self.rng = n, O, np.random.default_rng(seed)

    def step(self, action):
        a = npv(action).astype(np.float32)
        n = self.num_envs
        obs = (0.5 * self.rng.standard_normal((n, self.O)) + np.tanh(a.sum(axis=1, keepdims=True))).astype(np.float32)
        reward = (a[:, :1] * 0.1 + self.rng.standard_normal((n, 1))).astype(np.float32)
        done = self.rng.random(n) < 0.2
        infos = [{"bad_transition": True} if self.rng.random() < 0.1 else {} for _ in range(n)]
        return obs, reward, done, infos


def reference_loop(sg, p, agent, ro, envs, m_obs, m_act, iterations, obs0):
    """a2c/main.py:181-257 written out on a plain 2n-column rollout, the mirrored rows from the restatement's arithmetic."""
    from simgan_amd.utils import to_host_tensor
    n = envs.num_envs
    rep = lambda x: np.concatenate([npv(x), npv(x)]).astype(np.float32)  # noqa: E731
    aug = lambda x, m: np.concatenate([npv(x), ref.mirror(m, npv(x))]).astype(np.float32)  # noqa: E731
    ro.obs[0].copy_(to_host_tensor(aug(obs0, m_obs)))
    ro.obs_feat[0].copy_(to_host_tensor(rep(obs0)))
    for _ in range(iterations):
        for step in range(ro.num_steps):
            value, action, logp, hxs = p.act(ro.obs[step, :n], ro.recurrent_hidden_states[step, :n], ro.masks[step, :n])
            obs, reward, done, infos = envs.step(action)
            masks = np.array([[0.0] if d else [1.0] for d in done], np.float32)
            bad = np.array([[0.0] if 'bad_transition' in info.keys() else [1.0] for info in infos], np.float32)
            ro.insert(to_host_tensor(aug(obs, m_obs)), to_host_tensor(rep(hxs)), to_host_tensor(aug(action, m_act)),
                      to_host_tensor(rep(logp)), to_host_tensor(rep(value)), to_host_tensor(rep(reward)), to_host_tensor(rep(masks)),
                      to_host_tensor(rep(bad)), to_host_tensor(rep(obs)))
        next_value = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1])
        ro.compute_returns(next_value, True, 0.99, 0.95, True)
        agent.update(ro)
        ro.after_update()


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("recurrent", [False, True])
def test_ppo_learner_with_dup_sym_equals_the_reference_loop(sg, recurrent, resident):
    """Two iterations of PpoLearner(dup_sym=...) against the reference's sequence written out by hand on a plain rollout:
    parameters and Adam state bitwise equal.  Recurrent and device-resident: the bootstrap value of the mirrored columns is
    V(mirror(s_T)) -- get_value sees slot T of the device's obs, not a repeat of the first half."""
    from simgan_amd.driver import PpoLearner
    O, A, H, T, n = (13, 5, 20, 3, 2) if recurrent else (5, 2, 8, 3, 3)
    rng = np.random.default_rng(31)
    m_obs, m_act = ref.dense(rng, O), ref.dense(rng, A)
    obs0 = rng.standard_normal((n, O)).astype(np.float32)
    out = []
    for which in ("learner", "loop"):
        p = make_policy(sg, O, A, H, recurrent)
        if out:
            p.seed = out[0][3]                      # the same action-noise stream as the learner's policy
        ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), p.recurrent_hidden_state_size, O)
        agent = sg.algo.PPO(p, 0.2, 2, 2, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5, seed=7)
        envs = StubEnvs(n, O, seed=41)
        if which == "learner":
            ro.device_resident = resident
            learner = PpoLearner(p, agent, ro, dup_sym=(m_obs, m_act))
            ro.set_initial_obs_dup_sym(obs0, obs0)
            for _ in range(2):
                learner.collect(envs)
                res = learner.update()
                res = res.resolve() if hasattr(res, "resolve") else res
                assert np.isfinite(float(res["value_loss"]))
        else:
            reference_loop(sg, p, agent, ro, envs, m_obs, m_act, 2, obs0)
        mm, vv, step = agent.get_adam()
        out.append((p.get_flat_params(), mm, vv, p.seed, step))
    assert out[0][4] == out[1][4] == 2 * 2 * 2
    for a, b in zip(out[0][:3], out[1][:3]):
        assert np.array_equal(a, b)


def test_recurrent_resident_bootstrap_reads_the_mirrored_obs_of_slot_T(sg):
    """_returns_resident on a mirror-augmented rollout fetches slot T of obs and masks: the host mirrors' second half is the
    device's mirror image afterwards, not what the host held."""
    from simgan_amd.driver import PpoLearner
    O, A, H, T, n = 13, 5, 20, 3, 2
    rng = np.random.default_rng(32)
    m_obs, m_act = ref.dense(rng, O), ref.dense(rng, A)
    p = make_policy(sg, O, A, H, True)
    ro = sg.RolloutStorage(T, 2 * n, (O,), Box((A,)), H, O)
    ro.device_resident = True
    agent = sg.algo.PPO(p, 0.2, 1, 2, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    learner = PpoLearner(p, agent, ro, dup_sym=(m_obs, m_act))
    ro.set_initial_obs_dup_sym(rng.standard_normal((n, O)).astype(np.float32), None)
    learner.collect(StubEnvs(n, O, seed=42))
    last = npv(ro.obs)[-1].copy()
    assert np.all(last[n:] == 0)                      # the host never held the mirrored half
    learner.update().resolve()
    assert np.array_equal(npv(ro.obs)[0, n:], ref.mirror(m_obs, last[:n]))   # fetched for get_value, carried over by after_update


# ------------------------------------------------------------------------------------------ refusals
def test_refusals_name_the_mismatch(sg):
    from simgan_amd import _lib
    from simgan_amd.driver import PpoLearner
    O, A, T = 5, 2, 2
    rng = np.random.default_rng(51)
    m_obs, m_act = ref.dense(rng, O), ref.dense(rng, A)
    odd = sg.RolloutStorage(T, 3, (O,), Box((A,)), 1, O)
    with pytest.raises(ValueError, match="num_processes = 3, an odd number"):
        odd.enable_dup_sym(m_obs, m_act)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_set_mirrors: the rollout has N = 3 columns, an odd number"):
        _lib.check(odd.lib.sg_rollout_set_mirrors(odd.h, _lib.fptr(m_obs), _lib.fptr(m_act)))
    ro = sg.RolloutStorage(T, 4, (O,), Box((A,)), 1, O)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_dup_sym: the rollout has no mirrors: call sg_rollout_set_mirrors first"):
        _lib.check(ro.lib.sg_rollout_dup_sym(ro.h))
    with pytest.raises(RuntimeError, match="insert_dup_sym: the rollout is not mirror-augmented: call enable_dup_sym"):
        ro.insert_dup_sym(*[np.zeros((2, 1), np.float32)] * 8)
    with pytest.raises(ValueError, match=r"mirror_obs: a mirror matrix must be \[5, 5\], got \[2, 2\]"):
        ro.enable_dup_sym(m_act, m_act)
    with pytest.raises(ValueError, match=r"mirror_act: a mirror matrix must be \[2, 2\], got \[5, 5\]"):
        ro.enable_dup_sym(m_obs, m_obs)
    with pytest.raises(ValueError, match="mirror_act: the mirror callable is not linear"):
        ro.enable_dup_sym(m_obs, lambda a: list(np.asarray(a, np.float64) ** 2))
    bad = m_act.copy()
    bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="mirror_act: the mirror matrix holds non-finite entries"):
        ro.enable_dup_sym(m_obs, bad)
    with pytest.raises(_lib.SimganHipError, match=r"sg_rollout_set_mirrors: m_act\[1\]\[0\] is not finite"):
        _lib.check(ro.lib.sg_rollout_set_mirrors(ro.h, _lib.fptr(m_obs), _lib.fptr(bad)))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_set_mirrors: the action mirror m_act is required"):
        _lib.check(ro.lib.sg_rollout_set_mirrors(ro.h, _lib.fptr(m_obs), None))
    a = npv(ro.obs)
    with pytest.raises(_lib.SimganHipError, match=r"sg_rollout_upload_columns: 5 columns out of range \(0, 4\]"):
        _lib.check(ro.lib.sg_rollout_upload_columns(ro.h, _lib.F_OBS, 5, _lib.fptr(a), a.size))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_upload_columns: host is the full-width field 0 of 60 floats, got 30"):
        _lib.check(ro.lib.sg_rollout_upload_columns(ro.h, _lib.F_OBS, 2, _lib.fptr(a), a.size // 2))
    ro.enable_dup_sym(m_obs, m_act)
    with pytest.raises(ValueError, match="insert_dup_sym: obs must hold n = 2 rows"):
        ro.insert_dup_sym(np.zeros((4, O), np.float32), *[np.zeros((2, 1), np.float32)] * 7)
    p = make_policy(sg, O, A, 8, False)
    agent = sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    learner = PpoLearner(p, agent, sg.RolloutStorage(T, 4, (O,), Box((A,)), 1, O), dup_sym=(m_obs, m_act))
    with pytest.raises(ValueError, match="the rollout has 4 columns; 3 environments and their mirror images need 2 \\* num_envs = 6"):
        learner.collect(StubEnvs(3, O, seed=1))
