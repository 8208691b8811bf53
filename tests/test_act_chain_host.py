"""CPU: the host side of the chained act -- sg_rollout_act_step_chain is declared, exported and prototyped, and the Python
bookkeeping around it (RolloutStorage.act_step_chain / insert_env_rest / finish_collect_chain, the two drivers' collect(inner=))
does what the two separate calls would: counters, seeds, host mirrors, bytes_uploaded, the "slot already complete" rule, argument
checks and the envs.step contract.  The library is a stub that records its calls and writes recognisable floats; nothing here
needs a device."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MASK = 2 ** 64 - 1


def test_the_entry_point_is_declared_exported_and_prototyped():
    from simgan_amd import _lib
    header = open(os.path.join(ROOT, "include", "simgan_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "SG_API int sg_rollout_act_step_chain(" in header
    assert "SG_CHAIN_INNER_FIRST = 0, SG_CHAIN_LEARNER_FIRST = 1" in header
    assert hasattr(lib, "sg_rollout_act_step_chain")
    restype, argtypes = _lib.PROTOTYPES["sg_rollout_act_step_chain"]
    assert restype is ctypes.c_int and len(argtypes) == 20
    assert (_lib.CHAIN_INNER_FIRST, _lib.CHAIN_LEARNER_FIRST) == (0, 1)
    assert len(_lib.PROTOTYPES["sg_rollout_act_step"][1]) == 8 and len(_lib.PROTOTYPES["sg_policy_act_ensemble"][1]) == 11
    assert "sg_test_squash" in _lib.TEST_PROTOTYPES and hasattr(ctypes.CDLL(_lib.TEST_LIB_PATH), "sg_test_squash")
    assert "sg_test_squash" in open(os.path.join(ROOT, "simgan_amd", "csrc", "sg_test_api.h")).read()


# ------------------------------------------------------------------------------------------------ stubs
def arr(ptr, shape, dtype=np.float32):
    if ptr is None:
        return None
    return np.ctypeslib.as_array(ptr, shape=shape)


class StubLib:
    """Records every call; the chained step writes action = 100 t + row + k / 10, inner action = -(the same) - 0.5."""

    def __init__(self, N, O, A, Oi, Ai):
        self.N, self.O, self.A, self.Oi, self.Ai = N, O, A, Oi, Ai
        self.calls = []

    def _fill(self, t, width, sign):
        return (sign * (100 * t + np.arange(self.N)[:, None] + np.arange(width)[None, :] / 10.0 + (0.5 if sign < 0 else 0))).astype(np.float32)

    def sg_rollout_act_step_chain(self, r, p, t, order, members, K, idx, iobs, state, obs, inz, iseed, idet, nz, seed, det, squash,
                                  action, inner_action, inner_raw):
        N = self.N
        rec = {"fn": "chain", "t": t, "order": order, "K": K, "idx": arr(idx, (N,)).copy(), "iseed": iseed, "seed": seed,
               "idet": idet, "det": det, "squash": squash, "has": {k: v is not None for k, v in
                                                                   (("iobs", iobs), ("state", state), ("obs", obs), ("inz", inz), ("nz", nz),
                                                                    ("action", action), ("inner_raw", inner_raw))}}
        if iobs is not None:
            rec["iobs"] = arr(iobs, (N, self.Oi)).copy()
        if obs is not None:
            rec["obs"] = arr(obs, (N, self.O)).copy()
        self.calls.append(rec)
        if action is not None:
            arr(action, (N, self.A))[...] = self._fill(t, self.A, 1)
        arr(inner_action, (N, self.Ai))[...] = self._fill(t, self.Ai, -1)
        return 0

    def sg_rollout_act_step(self, r, p, t, obs, nz, seed, det, action):
        self.calls.append({"fn": "step", "t": t, "seed": seed, "obs": arr(obs, (self.N, self.O)).copy()})
        arr(action, (self.N, self.A))[...] = self._fill(t, self.A, 1) + 0.25
        return 0

    def sg_rollout_upload(self, r, f, ptr, count):
        self.calls.append({"fn": "upload", "field": f})
        return 0

    def sg_rollout_upload_step(self, r, f, t, ptr, count):
        self.calls.append({"fn": "upload_step", "field": f, "t": t})
        return 0

    def sg_rollout_after_update(self, r):
        self.calls.append({"fn": "after_update"})
        return 0

    def sg_rollout_destroy(self, r):
        return 0


class StubPolicy:
    is_recurrent, dist_kind, cnn = False, 0, 0

    def __init__(self, O, A, seed=1000):
        self.obs_dim, self.act_dim, self.seed, self._act_calls, self.h = O, A, seed, 0, object()


class StubEnsemble:
    def __init__(self, O, A, K=3, seed=7000):
        self.obs_dim, self.act_dim, self.seed, self._calls, self.K, self._handles = O, A, seed, 0, K, object()

    def __len__(self):
        return self.K


def make_rollout(T, N, O, A, lib, F=2):
    import torch
    from simgan_amd.storage import RolloutStorage
    ro = object.__new__(RolloutStorage)
    z = lambda *s: torch.zeros(*s)  # noqa: E731
    ro.obs, ro.obs_feat, ro.recurrent_hidden_states = z(T + 1, N, O), z(T + 1, N, F), z(T + 1, N, 1)
    ro.rewards, ro.value_preds, ro.returns = z(T, N, 1), z(T + 1, N, 1), z(T + 1, N, 1)
    ro.action_log_probs, ro.actions = z(T, N, 1), z(T, N, A)
    ro.masks, ro.bad_masks = torch.ones(T + 1, N, 1), torch.ones(T + 1, N, 1)
    ro.image_shape, ro.discrete, ro.box_actions = None, False, True
    ro.num_steps, ro.num_processes, ro.step = T, N, 0
    ro.obs_dim, ro.act_dim, ro.feat_len = O, A, F
    ro._device_resident, ro._host_written, ro._synced, ro._crcs = True, False, {}, {}
    ro.bytes_uploaded, ro._dup, ro.device_hidden = 0, None, False
    ro.lib, ro.h, ro.ctx = lib, object(), None
    return ro


# GAIL-dyn shapes: state 4, members 4 -> 2, learner 6 -> 3;  refinement: learner 4 -> 2, members 6 -> 3
T, N = 3, 5


def gail_setup():
    lib = StubLib(N, 6, 3, 4, 2)
    return lib, make_rollout(T, N, 6, 3, lib), StubPolicy(6, 3), StubEnsemble(4, 2)


def refine_setup():
    lib = StubLib(N, 4, 2, 6, 3)
    return lib, make_rollout(T, N, 4, 2, lib, F=4), StubPolicy(4, 2), StubEnsemble(6, 3)


# ------------------------------------------------------------------------------------------------ act_step_chain
def test_inner_first_counters_seeds_mirrors_and_bytes():
    from simgan_amd import _lib
    lib, ro, pol, ens = gail_setup()
    state = np.arange(N * 4, dtype=np.float32).reshape(N, 4)
    ind = np.array([0, 2, 1, 1, 0])
    ro.step = 1
    action, inner_action, got_ind = ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=state, ind=ind)
    assert pol._act_calls == 1 and ens._calls == 1          # as Policy.act / act_step and PolicyEnsemble.act count
    c = lib.calls[-1]
    assert c["fn"] == "chain" and c["t"] == 1 and c["order"] == 0 and c["K"] == 3
    assert c["seed"] == (pol.seed + 1) & MASK and c["iseed"] == (ens.seed + 1) & MASK
    assert np.array_equal(c["idx"], ind) and np.array_equal(got_ind, ind) and got_ind.dtype == np.int32
    # the state is what the members act on: it travels as inner_obs and no second copy goes up
    assert c["has"] == {"iobs": True, "state": False, "obs": False, "inz": False, "nz": False, "action": True, "inner_raw": False}
    assert np.array_equal(c["iobs"], state) and c["squash"] == 1 and c["det"] == 0 and c["idet"] == 0
    assert np.array_equal(action.numpy(), lib._fill(1, 3, 1)) and np.array_equal(inner_action.numpy(), lib._fill(1, 2, -1))
    assert np.array_equal(ro.actions[1].numpy(), action.numpy())
    assert np.array_equal(ro.obs[1].numpy(), np.concatenate([state, inner_action.numpy()], axis=1))   # the host mirror of the seam row
    assert ro.bytes_uploaded == state.nbytes + 4 * N
    assert ro.step == 1                                     # only insert_env_rest advances
    # separate state and inner_obs (Laikago): both go up and are counted
    ens5 = StubEnsemble(5, 2)
    lib.Oi = 5
    io = np.ones((N, 5), np.float32)
    before = ro.bytes_uploaded
    ro.act_step_chain(pol, ens5, _lib.CHAIN_INNER_FIRST, inner_obs=io, state=state, ind=ind, noise=np.zeros((N, 3)),
                      inner_noise=np.zeros((N, 2)), deterministic=True, inner_deterministic=True, squash=False)
    c = lib.calls[-1]
    assert c["has"]["state"] and c["has"]["iobs"] and c["has"]["nz"] and c["has"]["inz"]
    assert (c["det"], c["idet"], c["squash"]) == (1, 1, 0)
    assert ro.bytes_uploaded - before == io.nbytes + state.nbytes + 4 * N
    assert pol._act_calls == 2 and ens5._calls == 1 and c["seed"] == (pol.seed + 2) & MASK


def test_ind_is_drawn_like_policy_ensemble_act_draws_it():
    from simgan_amd import _lib
    lib, ro, pol, ens = gail_setup()
    _, _, ind = ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=np.zeros((N, 4)), rng=np.random.default_rng(3))
    assert np.array_equal(ind, np.random.default_rng(3).integers(0, 3, size=N))


def test_learner_first_uploads_the_host_slot_and_leaves_obs_alone():
    from simgan_amd import _lib
    lib, ro, pol, ens = refine_setup()
    ro.obs[0].copy_(ro.obs.new_tensor(np.arange(N * 4, dtype=np.float32).reshape(N, 4)))
    before = ro.obs.clone()
    action, env_action, ind = ro.act_step_chain(pol, ens, _lib.CHAIN_LEARNER_FIRST, ind=np.zeros(N, np.int64))
    c = lib.calls[-1]
    assert c["order"] == 1 and c["t"] == 0 and c["has"]["obs"] and not c["has"]["iobs"] and not c["has"]["state"]
    assert np.array_equal(c["obs"], before[0].numpy())
    assert np.array_equal(ro.obs.numpy(), before.numpy())
    assert np.array_equal(ro.actions[0].numpy(), action.numpy()) and tuple(env_action.shape) == (N, 3)
    assert pol._act_calls == 1 and ens._calls == 1
    assert ro.bytes_uploaded == N * 4 * 4 + 4 * N


def test_argument_checks():
    from simgan_amd import _lib
    lib, ro, pol, ens = gail_setup()
    st = np.zeros((N, 4), np.float32)
    with pytest.raises(ValueError, match="unknown order"):
        ro.act_step_chain(pol, ens, 2, state=st)
    with pytest.raises(ValueError, match="needs inner_obs"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST)
    with pytest.raises(ValueError, match="ind must hold N = 5 member numbers in \\[0, 3\\)"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=st, ind=np.array([0, 1, 2, 3, 0]))
    with pytest.raises(ValueError, match="inner_obs holds 4 rows"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, inner_obs=np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="state holds 15 floats"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, inner_obs=st, state=np.zeros((N, 3), np.float32))
    with pytest.raises(ValueError, match="dims do not add up"):       # members 5 -> 2 without a state of its own: 5 + 2 != 6
        ro.act_step_chain(pol, StubEnsemble(5, 2), _lib.CHAIN_INNER_FIRST, inner_obs=np.zeros((N, 5), np.float32))
    with pytest.raises(ValueError, match="dims do not add up"):       # a member action as wide as the learner's observation
        ro.act_step_chain(pol, StubEnsemble(4, 6), _lib.CHAIN_INNER_FIRST, inner_obs=st)
    with pytest.raises(ValueError, match="learner/rollout dims differ"):
        ro.act_step_chain(StubPolicy(7, 3), ens, _lib.CHAIN_INNER_FIRST, state=st)
    with pytest.raises(ValueError, match="inner_obs is not taken"):
        ro.act_step_chain(pol, StubEnsemble(9, 2), _lib.CHAIN_LEARNER_FIRST, inner_obs=st)
    with pytest.raises(ValueError, match="dims do not add up"):       # refinement: members 8 -> 2, learner 6 -> 3: 6 + 3 != 8
        ro.act_step_chain(pol, StubEnsemble(8, 2), _lib.CHAIN_LEARNER_FIRST)
    for attr, val in (("is_recurrent", True), ("dist_kind", 1), ("cnn", 3)):
        bad = StubPolicy(6, 3)
        setattr(bad, attr, val)
        with pytest.raises(ValueError, match="feed-forward learner with the MLP base and a Gaussian head"):
            ro.act_step_chain(bad, ens, _lib.CHAIN_INNER_FIRST, state=st)
    assert pol._act_calls == 0 and ens._calls == 0 and not lib.calls and ro.bytes_uploaded == 0   # a refused call consumes nothing
    # the same checks in front as act_step
    ro._device_resident = False
    with pytest.raises(ValueError, match="act_step_chain: the rollout is not device-resident"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=st)
    ro._device_resident, ro._dup = True, {"n": 1}
    with pytest.raises(ValueError, match="act_step_chain: the rollout is mirror-augmented"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=st)
    ro._dup, ro.image_shape = None, (1, 84, 84)
    with pytest.raises(NotImplementedError, match="act_step_chain: on-device collection is not built for image observations"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=st)
    with pytest.raises(NotImplementedError, match="insert_env_rest"):
        ro.insert_env_rest(np.zeros((N, 1)), np.ones((N, 1)), np.ones((N, 1)))
    ro.image_shape = None
    lib2, ro2, _, ens2 = gail_setup()
    with pytest.raises(ValueError, match="no act_step_chain call has served this rollout yet"):
        ro2.finish_collect_chain(ens2, state=st)


def test_insert_env_rest_and_the_slot_already_complete_rule():
    from simgan_amd import _lib
    lib, ro, pol, ens = gail_setup()
    st = lambda k: np.full((N, 4), float(k), np.float32)  # noqa: E731
    ones = np.ones((N, 1), np.float32)
    assert not ro.chain_slot_complete
    for s in range(T):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=st(s), ind=np.zeros(N, np.int64))
        obs_before = ro.obs.clone()
        ro.insert_env_rest(np.full((N, 1), 10.0 + s, np.float32), 0 * ones if s == 1 else ones, ones, np.full((N, 2), 20.0 + s, np.float32))
        assert np.array_equal(ro.obs.numpy(), obs_before.numpy())        # the next observation is not known yet
        assert float(ro.rewards[s, 0, 0]) == 10.0 + s and float(ro.obs_feat[s + 1, 0, 0]) == 20.0 + s
        assert float(ro.masks[s + 1, 0, 0]) == (0.0 if s == 1 else 1.0)
        assert ro.step == (s + 1) % T and ro._host_written
    inner_action, ind = ro.finish_collect_chain(ens, state=st(T), ind=np.ones(N, np.int64))
    c = [x for x in lib.calls if x["fn"] == "chain"][-1]
    assert c["t"] == T and not c["has"]["action"] and ens._calls == T + 1 and pol._act_calls == T   # the learner does not act at T
    assert np.array_equal(ro.obs[T].numpy(), np.concatenate([st(T), inner_action.numpy()], axis=1))
    # ... then what finish_collect does
    from simgan_amd import _lib as L
    ups = [x for x in lib.calls if x["fn"] in ("upload", "upload_step")]
    assert [x["field"] for x in ups if x["fn"] == "upload"] == [L.F_OBS_FEAT, L.F_REWARDS, L.F_RETURNS, L.F_MASKS, L.F_BAD_MASKS]
    assert [(x["field"], x["t"]) for x in ups if x["fn"] == "upload_step"] == [(L.F_OBS, T), (L.F_VALUE_PREDS, T)]
    assert not ro.chain_slot_complete                       # slot T is complete, the cursor is at 0
    ro.after_update()
    assert ro.chain_slot_complete and ro.step == 0
    assert np.array_equal(ro.obs[0].numpy(), ro.obs[T].numpy())          # the host mirror rolled over with the device
    with pytest.raises(ValueError, match="slot 0 is already complete"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=st(9))
    assert ens._calls == T + 1 and pol._act_calls == T      # the refused call took no draw
    ro.act_step(pol)
    assert lib.calls[-1]["fn"] == "step" and np.array_equal(lib.calls[-1]["obs"], ro.obs[0].numpy())
    ro.insert_env_rest(ones, ones, ones)
    assert not ro.chain_slot_complete
    ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=st(5), ind=np.zeros(N, np.int64))       # slot 1: chained again
    # an update without a chained finish leaves nothing marked complete
    ro.after_update()
    ro.step = 0
    assert not ro.chain_slot_complete


# ------------------------------------------------------------------------------------------------ drivers
class GailEnv:
    """The pool's side of the INNER_FIRST contract: step(action, inner_action) -> state (or (state, inner_obs))."""

    def __init__(self, pair):
        self.pair, self.steps, self.k = pair, [], 0

    def step(self, action, inner_action):
        self.steps.append((action.numpy().copy(), inner_action.numpy().copy()))
        self.k += 1
        state = np.full((N, 4), float(self.k), np.float32)
        out = (state, np.full((N, 5), -float(self.k), np.float32)) if self.pair else state
        return out, np.full((N, 1), 0.5, np.float32), [False] * N, [{"sas_feat": np.full(2, float(self.k), np.float32)} for _ in range(N)]


def learner_of(cls, ro, pol):
    ln = object.__new__(cls)
    ln.rollouts, ln.actor_critic, ln.dup_sym = ro, pol, False
    return ln


def sas(infos):
    return np.stack([i["sas_feat"] for i in infos])


@pytest.mark.parametrize("pair", [False, True])
def test_gail_dyn_collect_chains_and_keeps_the_pending_inner_action(pair):
    from simgan_amd.driver import GailDynLearner
    lib, ro, pol, ens = gail_setup()
    if pair:
        ens, lib.Oi = StubEnsemble(5, 2), 5
    ln, env = learner_of(GailDynLearner, ro, pol), GailEnv(pair)
    with pytest.raises(ValueError, match="the first collection needs state="):
        ln.collect(env, sas, on_device=True, inner=ens)
    with pytest.raises(ValueError, match="on_device=True"):
        ln.collect(env, sas, inner=ens)
    s0 = np.zeros((N, 4), np.float32)
    kw = {"inner_obs": np.zeros((N, 5), np.float32)} if pair else {}
    ln.collect(env, sas, on_device=True, inner=ens, state=s0, rng=np.random.default_rng(0), **kw)
    chain = [c for c in lib.calls if c["fn"] == "chain"]
    assert [c["t"] for c in chain] == [0, 1, 2, 3] and all(c["order"] == 0 for c in chain)
    assert all(c["has"]["state"] == pair for c in chain)
    assert ens._calls == T + 1 and pol._act_calls == T and len(env.steps) == T
    for s, (a, ia) in enumerate(env.steps):                 # envs.step gets the learner's action and the action inside obs[s]
        assert np.array_equal(a, lib._fill(s, 3, 1)) and np.array_equal(ia, lib._fill(s, 2, -1))
        assert np.array_equal(ro.obs[s].numpy()[:, 4:], ia)
        assert np.all(ro.obs[s].numpy()[:, :4] == float(s))                   # the state the previous step returned
    if pair:
        assert all(np.all(c["iobs"] == -float(c["t"])) for c in chain[1:])
    assert np.all(ro.obs_feat[1:].numpy() == np.arange(1, T + 1, dtype=np.float32)[:, None, None])
    assert np.array_equal(ln._chain_inner_action.numpy(), lib._fill(T, 2, -1))
    # second collection: slot 0 is the rolled-over obs[T] and takes the plain step, with the pending inner action
    ro.after_update()
    n0 = len(lib.calls)
    ln.collect(env, sas, on_device=True, inner=ens)
    kinds = [(c["fn"], c["t"]) for c in lib.calls[n0:] if c["fn"] in ("step", "chain")]
    assert kinds == [("step", 0), ("chain", 1), ("chain", 2), ("chain", 3)]
    assert ens._calls == 2 * T + 1 and pol._act_calls == 2 * T               # not one draw more than the two-call path takes
    a, ia = env.steps[T]
    assert np.array_equal(a, lib._fill(0, 3, 1) + 0.25) and np.array_equal(ia, lib._fill(T, 2, -1))


class RefineEnv:
    def __init__(self, pair):
        self.pair, self.steps, self.k = pair, [], 0

    def step(self, action, env_action):
        self.steps.append((action.numpy().copy(), env_action.numpy().copy()))
        self.k += 1
        obs = np.full((N, 4), float(self.k), np.float32)
        out = (obs, np.full((N, 4), -float(self.k), np.float32)) if self.pair else obs
        return out, np.zeros((N, 1), np.float32), [False] * N, [{} for _ in range(N)]


@pytest.mark.parametrize("pair", [False, True])
def test_ppo_collect_chains_learner_first(pair):
    from simgan_amd.driver import PpoLearner
    lib, ro, pol, ens = refine_setup()
    ln, env = learner_of(PpoLearner, ro, pol), RefineEnv(pair)
    with pytest.raises(ValueError, match="on_device=True"):
        ln.collect(env, inner=ens)
    ln.collect(env, on_device=True, inner=ens, rng=np.random.default_rng(1), **({"state": np.zeros((N, 4), np.float32)} if pair else {}))
    chain = [c for c in lib.calls if c["fn"] == "chain"]
    assert [c["t"] for c in chain] == [0, 1, 2] and all(c["order"] == 1 and c["has"]["obs"] for c in chain)
    assert all(c["has"]["state"] == pair for c in chain)
    assert pol._act_calls == T and ens._calls == T
    for s, (a, ea) in enumerate(env.steps):
        assert np.array_equal(a, lib._fill(s, 2, 1)) and np.array_equal(ea, lib._fill(s, 3, -1))
    assert np.all(ro.obs[1:].numpy() == np.arange(1, T + 1, dtype=np.float32)[:, None, None])
    assert np.array_equal(ro.obs_feat.numpy(), ro.obs.numpy())               # the feature slot carries the observation
    assert any(c["fn"] == "upload_step" and c["t"] == T for c in lib.calls)   # finish_collect, as without inner=


def test_collect_without_inner_is_unchanged():
    """The existing on-device collection makes the calls it made: one plain step per slot, envs.step(action) alone."""
    from simgan_amd.driver import PpoLearner
    lib, ro, pol, ens = refine_setup()

    class Env:
        def step(self, action):
            return np.zeros((N, 4), np.float32), np.zeros((N, 1), np.float32), [False] * N, [{} for _ in range(N)]

    learner_of(PpoLearner, ro, pol).collect(Env(), on_device=True)
    assert [(c["fn"], c["t"]) for c in lib.calls if c["fn"] in ("step", "chain")] == [("step", 0), ("step", 1), ("step", 2)]
