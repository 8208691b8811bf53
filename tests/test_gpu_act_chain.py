"""GPU: the chained act -- sg_rollout_act_step_chain / RolloutStorage.act_step_chain, insert_env_rest, finish_collect_chain and
collect(on_device=True, inner=...) -- against the two-call path it replaces: PolicyEnsemble.act, a host squash and concat, and
RolloutStorage.act_step.  The claim is bit identity of each half with its stand-alone launch: every comparison on policy outputs
is on the floats' bit patterns, no tolerance.  The one toleranced check is the squash itself against float64 tanh.

Shapes: GAIL-dyn order (INNER_FIRST): members Policy 11 -> 3 (h 64), learner SplitPolicy 14 -> 7 (h 32, one foot: 11 + 3 = 14).
Refinement order (LEARNER_FIRST): learner Policy 11 -> 3 (h 64), members SplitPolicy 14 -> 7.  T = 3.

Row tile classes (csrc/sg_policy_fwd.hpp fwd_tile_mt; csrc/sg_policy.hip sg_policy_act_ensemble): the learner's own launch runs
16-row tiles (two interleaved accumulators per dot product) for N <= 16 and wider ones above; the ensemble's runs 16-row tiles
while N < 16 K.  So with K = 1 the halves differ at N = 16 (members wide, learner 16-row), with K = 3 at N = 17 and 33 (members
16-row, learner wide); the chain runs each half in its own class and every case here MATCHES bit for bit -- none is refused.
The weight paths: LDS, and global memory forced by SG_POLICY_GW=1 or natural at hidden 256; a learner on one path with members on
the other is REFUSED with the documented message (test_weight_paths_that_differ_are_refused).
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

T = 3
NS = (1, 5, 16, 17, 33)
KS = (1, 3)


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


class Discrete:
    def __init__(self, n):
        self.n = n


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def bits(a):
    a = a.numpy() if hasattr(a, "numpy") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.size == b.size and np.array_equal(a.reshape(-1), b.reshape(-1))


def make_policy(sg, kind, O, A, H, seed, ctx=None):
    if kind == "mlp":
        pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H}, ctx=ctx)
    else:
        pol = sg.SplitPolicy((O,), Box((A,)), base_kwargs={"hidden_size": H, "num_feet": A // 7}, ctx=ctx)
    rng = np.random.default_rng(seed)   # off the initialiser's zero biases and near-zero mean heads
    pol.set_flat_params((0.3 * rng.standard_normal(pol.get_flat_params().size)).astype(np.float32))
    pol.seed = 0x1234 + seed            # (the constructor derives a per-instance seed: fixed here so that runs can be repeated)
    return pol


def make_ensemble(sg, kind, O, A, H, K, seed=40):
    from simgan_amd.ensemble import PolicyEnsemble
    ens = PolicyEnsemble([make_policy(sg, kind, O, A, H, seed + k) for k in range(K)])
    ens.seed = 0x77 + seed
    return ens


def gail_pair(sg, K, H_inner=64, H_learner=32):
    """(learner SplitPolicy 14 -> 7, members Policy 11 -> 3)"""
    return make_policy(sg, "split", 14, 7, H_learner, 5), make_ensemble(sg, "mlp", 11, 3, H_inner, K)


def refine_pair(sg, K):
    """(learner Policy 11 -> 3, members SplitPolicy 14 -> 7)"""
    return make_policy(sg, "mlp", 11, 3, 64, 6), make_ensemble(sg, "split", 14, 7, 32, K)


def make_rollout(sg, N, O, A, F=0):
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, F)
    ro.device_resident = True
    return ro


def field_shapes(ro):
    from simgan_amd import _lib
    N = ro.num_processes
    return {_lib.F_OBS: (T + 1, N, ro.obs_dim), _lib.F_OBS_FEAT: (T + 1, N, ro.feat_len), _lib.F_ACTIONS: (T, N, ro.act_dim),
            _lib.F_REWARDS: (T, N, 1), _lib.F_VALUE_PREDS: (T + 1, N, 1), _lib.F_RETURNS: (T + 1, N, 1), _lib.F_LOGP: (T, N, 1),
            _lib.F_MASKS: (T + 1, N, 1), _lib.F_BAD_MASKS: (T + 1, N, 1), _lib.F_ADVANTAGES: (T, N, 1)}


def download_all(ro):
    from simgan_amd import _lib
    out = {}
    for f, shape in field_shapes(ro).items():
        a = np.zeros(shape, np.float32)
        if a.size:
            _lib.check(ro.lib.sg_rollout_download(ro.h, f, _lib.fptr(a), a.size))
        out[f] = a
    return out


def squash(x):
    """The device's own squash (sg_test_squash): the twin's host-side tanh."""
    from simgan_amd import _lib
    x = np.ascontiguousarray(x.numpy() if hasattr(x, "numpy") else x, np.float32)
    out = np.empty_like(x)
    _lib.check_test(_lib.load_test().sg_test_squash(_lib.fptr(x.reshape(-1)), _lib.fptr(out.reshape(-1)), x.size))
    return out


def mixed_ind(N, K):
    """Members mixed inside one tile, every member present when N allows."""
    return ((np.arange(N) * 7 + 1) % K).astype(np.int32)


MODES = ("library", "deterministic", "injected")


def mode_kw(mode, rng, N, A, Ai):
    if mode == "injected":
        return {"noise": rng.standard_normal((N, A)).astype(np.float32)}, {"noise": rng.standard_normal((N, Ai)).astype(np.float32)}
    if mode == "deterministic":
        return {"deterministic": True}, {"deterministic": True}
    return {}, {}


# --------------------------------------------------------------------------------- values from before any chained call (check 8)
def existing_surface(sg):
    """act_step, PolicyEnsemble.act and collect(on_device=True) without inner=, at fixed seeds."""
    from simgan_amd import _lib
    from simgan_amd.driver import PpoLearner
    N = 17
    pol, ens = gail_pair(sg, 3)
    rng = np.random.default_rng(99)
    obs = rng.standard_normal((N, 14)).astype(np.float32)
    ro = make_rollout(sg, N, 14, 7, F=14)
    ro.obs[0].copy_(ro.obs.new_tensor(obs))
    out = [ro.act_step(pol).numpy().copy()]
    out += [download_all(ro)[f] for f in (_lib.F_VALUE_PREDS, _lib.F_ACTIONS, _lib.F_LOGP)]
    v, a, lp, _ = ens.act(obs[:, :11], ind=mixed_ind(N, 3), full=True)
    out += [v.numpy().copy(), a.numpy().copy(), lp.numpy().copy()]

    class Env:
        def step(self, action):
            o = np.tanh(action.numpy() @ np.ones((7, 14), np.float32) * 0.1).astype(np.float32)
            return o, o[:, :1].copy(), [False] * N, [{} for _ in range(N)]

    ln = object.__new__(PpoLearner)
    ln.rollouts, ln.actor_critic, ln.dup_sym = ro, pol, False
    ro.step = 0
    ln.collect(Env(), on_device=True)
    d = download_all(ro)
    return out + [d[f] for f in sorted(d)]


@pytest.fixture(scope="module", autouse=True)
def before_chain(sg):
    return existing_surface(sg)


# --------------------------------------------------------------------------------- checks 1-3, INNER_FIRST
def check_inner_first(sg, N, K, H_inner=64, H_learner=32):
    from simgan_amd import _lib
    pol, ens = gail_pair(sg, K, H_inner, H_learner)
    ro, twin = make_rollout(sg, N, 14, 7), make_rollout(sg, N, 14, 7)
    rng = np.random.default_rng(100 * N + K)
    ind = mixed_ind(N, K)
    t = 1
    for mode in MODES:
        what = f"N={N} K={K} {mode}"
        state = (1.5 * rng.standard_normal((N, 11))).astype(np.float32)
        # injected mode doubles as the case where the members act on something else than the state (Laikago)
        inner_obs = (1.5 * rng.standard_normal((N, 11))).astype(np.float32) if mode == "injected" else state
        lkw, ikw = mode_kw(mode, rng, N, 7, 3)
        e_calls, p_calls = ens._calls, pol._act_calls
        v_ref, raw_ref, lp_ref, _ = ens.act(inner_obs, ind=ind, full=True, **ikw)
        assert ens._calls == e_calls + 1
        ens._calls = e_calls
        raw = np.empty((N, 3), np.float32)
        ro.step = t
        ckw = {"deterministic": mode == "deterministic", "inner_deterministic": mode == "deterministic",
               "noise": lkw.get("noise"), "inner_noise": ikw.get("noise")}
        action, inner_action, got_ind = ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=state,
                                                          inner_obs=None if inner_obs is state else inner_obs, ind=ind,
                                                          inner_raw_out=raw, **ckw)
        # 1. the inner half
        assert same_bits(raw, raw_ref), f"{what}: inner raw action vs PolicyEnsemble.act"
        assert ens._calls == e_calls + 1 and pol._act_calls == p_calls + 1 and np.array_equal(got_ind, ind)
        # 2. the seam
        d = download_all(ro)
        sq = squash(raw)
        assert same_bits(d[_lib.F_OBS][t][:, :11], state), f"{what}: state part of OBS[t]"
        assert same_bits(d[_lib.F_OBS][t][:, 11:], sq), f"{what}: squashed action part of OBS[t]"
        assert same_bits(inner_action, sq), f"{what}: returned inner_action"
        assert same_bits(ro.obs[t], d[_lib.F_OBS][t]), f"{what}: host mirror of obs[t]"
        # 3. the learner half: plain act_step on a twin whose host slot holds the chain's OBS[t]
        twin.obs[t].copy_(twin.obs.new_tensor(d[_lib.F_OBS][t]))
        twin.step = t
        pol._act_calls = p_calls
        a_ref = twin.act_step(pol, **lkw)
        assert pol._act_calls == p_calls + 1
        dt = download_all(twin)
        for f, name in ((_lib.F_VALUE_PREDS, "value_preds"), (_lib.F_ACTIONS, "actions"), (_lib.F_LOGP, "action_log_probs")):
            assert same_bits(d[f][t], dt[f][t]), f"{what}: {name}[t]"
        assert same_bits(action, a_ref) and same_bits(ro.actions[t], a_ref), f"{what}: returned action"
        if mode == "library":
            assert np.abs(raw - np.tanh(raw)).max() > 1e-3, "nothing to squash"
        for f in d:   # nothing else moved: every other slot is as created
            other = [s for s in range(d[f].shape[0]) if s != t]
            assert same_bits(d[f][other], dt[f][other]), f"{what}: field {f} outside slot t"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_inner_first_halves_have_the_bits_of_their_own_launches(sg, monkeypatch, N, K):
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    check_inner_first(sg, N, K)


# --------------------------------------------------------------------------------- checks 1-3, LEARNER_FIRST
def check_learner_first(sg, N, K):
    from simgan_amd import _lib
    pol, ens = refine_pair(sg, K)
    ro, twin = make_rollout(sg, N, 11, 3), make_rollout(sg, N, 11, 3)
    rng = np.random.default_rng(200 * N + K)
    ind = mixed_ind(N, K)
    t = 2
    for mode in MODES:
        what = f"N={N} K={K} {mode}"
        obs = (1.5 * rng.standard_normal((N, 11))).astype(np.float32)
        state = (1.5 * rng.standard_normal((N, 11))).astype(np.float32) if mode == "injected" else None
        lkw, ikw = mode_kw(mode, rng, N, 3, 7)
        e_calls, p_calls = ens._calls, pol._act_calls
        for r in (ro, twin):
            r.obs[t].copy_(r.obs.new_tensor(obs))
            r.step = t
        a_ref = twin.act_step(pol, **lkw)
        pol._act_calls = p_calls
        env_in = np.concatenate([obs if state is None else state, squash(a_ref)], axis=1)
        _, raw_ref, _, _ = ens.act(env_in, ind=ind, full=True, **ikw)
        ens._calls = e_calls
        raw = np.empty((N, 7), np.float32)
        action, env_action, _ = ro.act_step_chain(pol, ens, _lib.CHAIN_LEARNER_FIRST, state=state, ind=ind, inner_raw_out=raw,
                                                  deterministic=mode == "deterministic", inner_deterministic=mode == "deterministic",
                                                  noise=lkw.get("noise"), inner_noise=ikw.get("noise"))
        assert ens._calls == e_calls + 1 and pol._act_calls == p_calls + 1
        d, dt = download_all(ro), download_all(twin)
        for f in d:
            assert same_bits(d[f], dt[f]), f"{what}: rollout field {f} vs plain act_step"
        assert same_bits(action, a_ref) and same_bits(ro.actions[t], a_ref), f"{what}: returned action"
        assert same_bits(env_action, raw_ref) and same_bits(raw, raw_ref), f"{what}: members' raw action vs PolicyEnsemble.act"


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("N", NS)
def test_learner_first_halves_have_the_bits_of_their_own_launches(sg, monkeypatch, N, K):
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    check_learner_first(sg, N, K)


# --------------------------------------------------------------------------------- check 2: the squash itself
def ulp_distance(a, b):
    """Units in the last place between float32 arrays (monotone integer images of the floats)."""
    def key(x):
        u = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(u < 0, -(u & 0x7FFFFFFF), u)
    return np.abs(key(a) - key(b))


def test_squash_is_within_the_relative_contract_of_float64_tanh():
    """1e-4 relative (the project's contract) on [-20, 20], with 0 and both saturated ends; the worst ulp distance is recorded."""
    rng = np.random.default_rng(7)
    x = np.concatenate([np.linspace(-20, 20, 40001), rng.uniform(-1e-3, 1e-3, 2000), rng.uniform(-9.5, 9.5, 8000),
                        [0.0, -0.0, 20.0, -20.0, 1e-30, -1e-30]]).astype(np.float32)
    got = squash(x)
    ref = np.tanh(x.astype(np.float64))
    rel = np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), 1e-300)
    rel[ref == 0] = np.abs(got[ref == 0])
    ulps = ulp_distance(got, ref.astype(np.float32))
    record = {"function": "sg_squash (tanhf), via sg_test_squash", "points": int(x.size), "range": [-20.0, 20.0],
              "worst_relative_error_vs_float64_tanh": float(rel.max()), "contract_relative": 1e-4,
              "worst_ulp_distance_vs_rounded_float64_tanh": int(ulps.max()), "at_x": float(x[int(np.argmax(ulps))])}
    print(json.dumps(record))
    if os.environ.get("SG_ACT_CHAIN_RECORD"):       # (profiles/act_chain_parity.json is this record)
        with open(os.environ["SG_ACT_CHAIN_RECORD"], "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    assert np.all(got[x == 0] == 0.0)
    assert got[-4] == 1.0 and got[-3] == -1.0 and np.all(np.abs(got) <= 1.0)
    assert rel.max() <= 1e-4, record


# --------------------------------------------------------------------------------- check 4: whole collections through the drivers
def learner_of(cls, ro, pol):
    ln = object.__new__(cls)
    ln.rollouts, ln.actor_critic, ln.dup_sym = ro, pol, False
    return ln


def sas(infos):
    return np.stack([i["sas_feat"] for i in infos])


class GailPool:
    """A small deterministic pool for the GAIL-dyn stage.  ens=None: the policy is taken out of it (the chained contract:
    step(action, inner_action) -> state).  With ens: the behaviour policy lives inside, as in the reference's environments:
    step(action) -> cat(state, squash(a_b)), the two-call path with the device's squash on the host."""

    def __init__(self, N, ens=None, rng=None):
        g = np.random.default_rng(11)
        self.state = g.standard_normal((N, 11)).astype(np.float32)
        self.P, self.Q = (0.3 * g.standard_normal((7, 11))).astype(np.float32), (0.3 * g.standard_normal((3, 11))).astype(np.float32)
        self.N, self.ens, self.rng, self.k, self.pending = N, ens, rng, 0, None

    def behaviour(self):
        a = self.ens.act(self.state, ind=self.rng.integers(0, len(self.ens), size=self.N))[0]
        self.pending = squash(a)
        return np.concatenate([self.state, self.pending], axis=1)

    def step(self, action, inner_action=None):
        action = np.asarray(action.numpy() if hasattr(action, "numpy") else action, np.float32)
        ia = self.pending if self.ens is not None else np.asarray(inner_action.numpy(), np.float32)
        self.state = (0.8 * self.state + np.tanh(action @ self.P + ia @ self.Q)).astype(np.float32)
        self.k += 1
        reward = self.state[:, :1] * np.float32(0.5)
        done = [(self.k + i) % 4 == 0 for i in range(self.N)]
        infos = [dict({"sas_feat": self.state[i, :5].copy()}, **({"bad_transition": True} if (self.k + i) % 7 == 0 else {}))
                 for i in range(self.N)]
        return (self.behaviour() if self.ens is not None else self.state.copy()), reward, done, infos


def compare_rollouts(ro, twin, what):
    from simgan_amd import _lib
    d, dt = download_all(ro), download_all(twin)
    for f in d:
        assert same_bits(d[f], dt[f]), f"{what}: device field {f}"
    ro.sync_from_device()
    twin.sync_from_device()
    for name in ("obs", "obs_feat", "actions", "rewards", "value_preds", "returns", "action_log_probs", "masks", "bad_masks"):
        assert same_bits(getattr(ro, name), getattr(twin, name)), f"{what}: rollouts.{name}"


@pytest.mark.parametrize("N,K", [(5, 1), (17, 3), (33, 3)])
def test_whole_gail_dyn_collections_equal_the_two_call_path(sg, monkeypatch, N, K):
    from simgan_amd.driver import GailDynLearner
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    pol, ens = gail_pair(sg, K)
    ro, twin = make_rollout(sg, N, 14, 7, F=5), make_rollout(sg, N, 14, 7, F=5)
    # chained: two collections with an update's roll-over between them; slot 0 of the second takes the plain step
    pool = GailPool(N)
    ln = learner_of(GailDynLearner, ro, pol)
    rng = np.random.default_rng(3)
    ln.collect(pool, sas, on_device=True, inner=ens, state=pool.state.copy(), rng=rng)
    first = download_all(ro)
    ro.after_update()
    assert ro.chain_slot_complete
    ln.collect(pool, sas, on_device=True, inner=ens, rng=rng)
    calls = (pol._act_calls, ens._calls)
    assert calls == (2 * T, 2 * T + 1)
    # the two-call path: the same pool with the behaviour policy inside, plain on-device collection
    pol._act_calls, ens._calls = 0, 0
    tpool = GailPool(N, ens, np.random.default_rng(3))
    tl = learner_of(GailDynLearner, twin, pol)
    twin.obs[0].copy_(twin.obs.new_tensor(tpool.behaviour()))
    tl.collect(tpool, sas, on_device=True)
    tfirst = download_all(twin)
    for f in first:
        assert same_bits(first[f], tfirst[f]), f"first collection: device field {f}"
    twin.after_update()
    tl.collect(tpool, sas, on_device=True)
    assert (pol._act_calls, ens._calls) == calls
    compare_rollouts(ro, twin, f"N={N} K={K} second collection")
    assert same_bits(pool.state, tpool.state)


class RefinePool:
    """The refinement stage: ens=None: step(action, env_action) -> obs; with ens the dynamics policies live inside."""

    def __init__(self, N, ens=None, rng=None, pair=False):
        g = np.random.default_rng(12)
        self.obs = g.standard_normal((N, 11)).astype(np.float32)
        self.P = (0.3 * g.standard_normal((7, 11))).astype(np.float32)
        self.N, self.ens, self.rng, self.k, self.pair = N, ens, rng, 0, pair

    def state(self):
        return (self.obs[:, ::-1] * np.float32(0.5)).copy() if self.pair else None

    def step(self, action, env_action=None):
        if self.ens is not None:
            st = self.state()
            env_in = np.concatenate([self.obs if st is None else st, squash(action)], axis=1)
            env_action = self.ens.act(env_in, ind=self.rng.integers(0, len(self.ens), size=self.N))[0]
        ea = np.asarray(env_action.numpy() if hasattr(env_action, "numpy") else env_action, np.float32)
        self.obs = (0.8 * self.obs + np.tanh(ea @ self.P)).astype(np.float32)
        self.k += 1
        done = [(self.k + 2 * i) % 5 == 0 for i in range(self.N)]
        out = self.obs.copy()
        if self.ens is None and self.pair:
            out = (out, self.state())
        return out, self.obs[:, 1:2] * np.float32(2.0), done, [{} for _ in range(self.N)]


@pytest.mark.parametrize("N,K,pair", [(5, 1, False), (17, 3, True), (33, 3, False)])
def test_whole_refinement_collections_equal_the_two_call_path(sg, monkeypatch, N, K, pair):
    from simgan_amd.driver import PpoLearner
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    pol, ens = refine_pair(sg, K)
    ro, twin = make_rollout(sg, N, 11, 3, F=11), make_rollout(sg, N, 11, 3, F=11)
    pool, tpool = RefinePool(N, pair=pair), RefinePool(N, ens, np.random.default_rng(4), pair=pair)
    ln, tl = learner_of(PpoLearner, ro, pol), learner_of(PpoLearner, twin, pol)
    rng = np.random.default_rng(4)
    for r, p in ((ro, pool), (twin, tpool)):
        r.obs[0].copy_(r.obs.new_tensor(p.obs))
        r.obs_feat[0].copy_(r.obs_feat.new_tensor(p.obs))
    ln.collect(pool, on_device=True, inner=ens, rng=rng, state=pool.state())
    ro.after_update()
    ln.collect(pool, on_device=True, inner=ens, rng=rng)
    calls = (pol._act_calls, ens._calls)
    assert calls == (2 * T, 2 * T)
    pol._act_calls, ens._calls = 0, 0
    tl.collect(tpool, on_device=True)
    twin.after_update()
    tl.collect(tpool, on_device=True)
    assert (pol._act_calls, ens._calls) == calls
    compare_rollouts(ro, twin, f"N={N} K={K} pair={pair}")
    assert same_bits(pool.obs, tpool.obs)


# --------------------------------------------------------------------------------- check 5: t == T
def test_step_T_completes_obs_T_and_nothing_else(sg, monkeypatch):
    from simgan_amd import _lib
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    N, K = 17, 3
    pol, ens = gail_pair(sg, K)
    ro = make_rollout(sg, N, 14, 7, F=2)
    rng = np.random.default_rng(5)
    for f, shape in field_shapes(ro).items():          # every field holds something recognisable
        if f != _lib.F_ADVANTAGES:
            a = rng.standard_normal(shape).astype(np.float32)
            _lib.check(ro.lib.sg_rollout_upload(ro.h, f, _lib.fptr(a), a.size))
    before = download_all(ro)
    state = rng.standard_normal((N, 11)).astype(np.float32)
    ind = mixed_ind(N, K)
    calls = pol._act_calls
    _, raw_ref, _, _ = ens.act(state, ind=ind, full=True)
    ens._calls -= 1
    inner_action = np.empty((N, 3), np.float32)
    _lib.check(ro.lib.sg_rollout_act_step_chain(ro.h, pol.h, T, _lib.CHAIN_INNER_FIRST, ens._handles, K, ind.ctypes.data_as(C.POINTER(C.c_int32)),
                                                _lib.fptr(state), None, None, None, (ens.seed + ens._calls + 1) & (2 ** 64 - 1), 0, None, 0, 0,
                                                1, None, _lib.fptr(inner_action), None))
    after = download_all(ro)
    assert same_bits(inner_action, squash(raw_ref))
    assert same_bits(after[_lib.F_OBS][T], np.concatenate([state, inner_action], axis=1))
    assert not same_bits(after[_lib.F_OBS][T], before[_lib.F_OBS][T])
    for f in before:
        keep = slice(0, T) if f == _lib.F_OBS else slice(None)
        assert same_bits(before[f][keep], after[f][keep]), f"field {f} changed"
    assert pol._act_calls == calls


# --------------------------------------------------------------------------------- check 6: weight paths
@pytest.mark.parametrize("N,K", [(5, 3), (16, 1), (33, 3)])
def test_both_orders_on_the_forced_global_weight_instances(sg, monkeypatch, N, K):
    monkeypatch.setenv("SG_POLICY_GW", "1")
    check_inner_first(sg, N, K)
    check_learner_first(sg, N, K)


@pytest.mark.parametrize("N", [5, 33])
def test_hidden_256_takes_the_global_weight_path_on_its_own(sg, monkeypatch, N):
    """Both halves 256 wide: neither trunk fits LDS, both launches read global memory, the chain does too and matches."""
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    check_inner_first(sg, N, 3, H_inner=256, H_learner=256)


def test_weight_paths_that_differ_are_refused(sg, monkeypatch):
    """Learner 256 wide (global memory), members 64 wide (LDS): the documented refusal, nothing consumed, nothing written."""
    from simgan_amd import _lib
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    N = 5
    pol, ens = gail_pair(sg, 3, H_inner=64, H_learner=256)
    ro = make_rollout(sg, N, 14, 7)
    before = download_all(ro)
    with pytest.raises(_lib.SimganHipError, match="reads its weights from global memory and the members' from LDS; the chained step "
                                                  "runs both halves on one weight path"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=np.zeros((N, 11), np.float32), ind=mixed_ind(N, 3))
    after = download_all(ro)
    assert all(same_bits(before[f], after[f]) for f in before)


# --------------------------------------------------------------------------------- check 7: refusals
def test_refusals_through_c_and_python(sg, monkeypatch):
    from simgan_amd import _lib
    from simgan_amd.ensemble import PolicyEnsemble
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    N, K = 5, 3
    pol, ens = gail_pair(sg, K)
    ro = make_rollout(sg, N, 14, 7)
    lib = ro.lib
    state = np.zeros((N, 11), np.float32)
    ind = mixed_ind(N, K)
    act, iact = np.empty((N, 7), np.float32), np.empty((N, 3), np.float32)

    def call(r=ro, learner=pol, t=0, order=_lib.CHAIN_INNER_FIRST, handles=None, k=K, idx=ind, iobs=state, st=None, action=act,
             inner_action=iact):
        handles = ens._handles if handles is None else handles
        p = lambda a: None if a is None else _lib.fptr(a)  # noqa: E731
        return lib.sg_rollout_act_step_chain(r.h if r is not None else None, learner.h if learner is not None else None, t, order, handles, k,
                                             None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_int32)), p(iobs), p(st), None, None,
                                             1, 0, None, 1, 0, 1, p(action), p(inner_action), None)

    def refused(match, **kw):
        assert call(**kw) != 0, match
        msg = lib.sg_last_error().decode()
        assert match in msg, (match, msg)

    alive = []                                                   # (a handle array does not keep its policies alive)

    def handles_of(*pols):
        alive.extend(pols)
        return (_lib.H * len(pols))(*[p.h for p in pols])

    assert call() == 0                                           # the call the refusals are variations of
    before = download_all(ro)
    refused("NULL argument", r=None)
    refused("NULL argument", learner=None)
    refused("NULL argument", idx=None)
    refused("NULL inner_action_host", inner_action=None)
    refused("NULL action_host", action=None)
    refused("NULL inner_obs_host", iobs=None)
    refused("unknown order 2", order=2)
    refused("1..8 members, got 0", k=0)
    refused("step -1 out of range [0,3]", t=-1)
    refused("step 4 out of range [0,3]", t=T + 1)
    refused("step 3 out of range [0,3) (SG_CHAIN_LEARNER_FIRST)", t=T, order=_lib.CHAIN_LEARNER_FIRST,
            handles=handles_of(make_policy(sg, "mlp", 21, 3, 64, 1)), k=1, idx=np.zeros(N, np.int32))
    bad_idx = ind.copy()
    bad_idx[3] = K
    refused("idx[3] = 3 outside [0, 3)", idx=bad_idx)
    bad_idx[3] = -1
    refused("idx[3] = -1 outside [0, 3)", idx=bad_idx)
    # learner
    cnn = sg.Policy((1, 84, 84), Box((7,)), base_kwargs={"hidden_size": 32})
    gru = sg.Policy((14,), Box((7,)), base_kwargs={"recurrent": True, "hidden_size": 32})
    cat = sg.Policy((14,), Discrete(7))
    refused("the learner has the CNN base", learner=cnn)
    refused("the learner is recurrent", learner=gru)
    refused("the learner has a Categorical / Bernoulli head", learner=cat)
    wide = make_policy(sg, "split", 15, 7, 32, 2)
    refused("learner/rollout dims differ (obs 15 vs 14, action 7 vs 7)", learner=wide)
    other = _lib.Context(0)
    elsewhere = make_policy(sg, "split", 14, 7, 32, 2, ctx=other)
    refused("the learner and the rollout live on different contexts", learner=elsewhere)
    # members
    m = ens.policies
    refused("member 1 has the CNN base", handles=handles_of(m[0], sg.Policy((1, 84, 84), Box((3,)), base_kwargs={"hidden_size": 32}), m[2]))
    refused("member 2 is a recurrent policy", handles=handles_of(m[0], m[1], sg.Policy((11,), Box((3,)), base_kwargs={"recurrent": True})))
    refused("member 0 has a Categorical / Bernoulli head", handles=handles_of(sg.Policy((11,), Discrete(3)), m[1], m[2]))
    refused("member 1 has a different shape", handles=handles_of(m[0], make_policy(sg, "mlp", 11, 3, 32, 3), m[2]))
    refused("member 2 is NULL or lives on another context", handles=handles_of(m[0], m[1], make_policy(sg, "mlp", 11, 3, 64, 3, ctx=other)))
    # dims that do not add up
    refused("dims do not add up: the learner's observation (14) must be state + member action (3), and without state_host",
            handles=handles_of(make_policy(sg, "mlp", 12, 3, 64, 1)), k=1, idx=np.zeros(N, np.int32), iobs=np.zeros((N, 12), np.float32))
    refused("dims do not add up: the members' observation (11) must be state + learner action (7)", order=_lib.CHAIN_LEARNER_FIRST)
    after = download_all(ro)
    assert all(same_bits(before[f], after[f]) for f in after), "a refused call wrote to the rollout"
    # ... and through Python
    with pytest.raises(ValueError, match="feed-forward learner with the MLP base and a Gaussian head"):
        ro.act_step_chain(gru, ens, _lib.CHAIN_INNER_FIRST, state=state, ind=ind)
    with pytest.raises(ValueError, match="feed-forward learner with the MLP base and a Gaussian head"):
        ro.act_step_chain(cat, ens, _lib.CHAIN_INNER_FIRST, state=state, ind=ind)
    with pytest.raises(ValueError, match="feed-forward learner with the MLP base and a Gaussian head"):
        ro.act_step_chain(cnn, ens, _lib.CHAIN_INNER_FIRST, state=state, ind=ind)
    with pytest.raises(NotImplementedError, match="MLP base only"):
        PolicyEnsemble([sg.Policy((1, 84, 84), Box((3,)), base_kwargs={"hidden_size": 32})])
    with pytest.raises(NotImplementedError, match="feed-forward members only"):
        PolicyEnsemble([sg.Policy((11,), Box((3,)), base_kwargs={"recurrent": True})])
    with pytest.raises(NotImplementedError, match="Box action spaces only"):
        PolicyEnsemble([sg.Policy((11,), Discrete(3))])
    with pytest.raises(AssertionError, match="must share kind"):
        PolicyEnsemble([m[0], make_policy(sg, "mlp", 11, 3, 32, 3)])
    with pytest.raises(_lib.SimganHipError, match="lives on another context"):
        ro.act_step_chain(pol, PolicyEnsemble([make_policy(sg, "mlp", 11, 3, 64, 3, ctx=other)]), _lib.CHAIN_INNER_FIRST, state=state,
                          ind=np.zeros(N, np.int32))
    with pytest.raises(ValueError, match="ind must hold"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=state, ind=bad_idx)
    with pytest.raises(ValueError, match="dims do not add up"):
        ro.act_step_chain(pol, ens, _lib.CHAIN_LEARNER_FIRST, ind=ind)
    with pytest.raises(ValueError, match="unknown order"):
        ro.act_step_chain(pol, ens, 5, state=state, ind=ind)


# --------------------------------------------------------------------------------- check 8 (last: after every chained call above)
def test_existing_surface_has_the_bits_it_had_before_any_chained_call(sg, monkeypatch, before_chain):
    from simgan_amd import _lib
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    pol, ens = gail_pair(sg, 1)
    ro = make_rollout(sg, 5, 14, 7)
    ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=np.ones((5, 11), np.float32))   # (at least one, if this test runs alone)
    now = existing_surface(sg)
    assert len(now) == len(before_chain) == 17
    for i, (a, b) in enumerate(zip(before_chain, now)):
        assert same_bits(a, b), f"existing surface, item {i}"
