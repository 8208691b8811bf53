"""GPU: collection on the device -- sg_rollout_act_step / RolloutStorage.act_step, insert_env, finish_collect and
collect(on_device=True) -- against today's path, Policy.act + insert + sync_to_device.  The claim is bit identity: every
comparison here is on the floats' bit patterns, no tolerance.

Which launch instance a row count N reaches (csrc/sg_policy_fwd.hpp: fwd_tile_mt, which the step's launcher follows so that it
sums in the order of sg_policy_act's forward launch): N <= 16 -> 16-row tiles <1> (two interleaved accumulators per dot
product); 17 <= N <= 32 -> 32-row tiles <2>; N >= 33 -> 64-row tiles <4>.  N = 1, 16 hit <1>; 17, 32 hit <2> (17: a ragged
tile); 33, 130 hit <4> (33: one row in the second workgroup; 130: three workgroups, the last with 2 rows).  Each with the
weights in LDS, or -- SG_POLICY_GW=1, or a hidden width of 256, whose trunk does not fit LDS -- read from global memory.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


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


# (class, O, A, hidden, num_feet, critic_hidden)
SPECS = {"mlp_11_3_64": ("mlp", 11, 3, 64, 1, None), "mlp_47_12_64": ("mlp", 47, 12, 64, 1, None),
         "mlp_30_6_32_critic64": ("mlp", 30, 6, 32, 1, 64), "split_20_7_32_f1": ("split", 20, 7, 32, 1, None),
         "split_47_14_64_f2": ("split", 47, 14, 64, 2, None), "mlp_47_12_256": ("mlp", 47, 12, 256, 1, None)}
ROWS = (1, 16, 17, 32, 33, 130)


def make_policy(sg, spec, seed=5, ctx=None, flat=None):
    kind, O, A, H, feet, Hc = SPECS[spec] if isinstance(spec, str) else spec
    if kind == "mlp":
        pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H}, ctx=ctx, critic_hidden=Hc)
    else:
        pol = sg.SplitPolicy((O,), Box((A,)), base_kwargs={"hidden_size": H, "num_feet": feet}, ctx=ctx)
    if flat is None:   # off the initialiser's zero biases and near-zero mean heads
        rng = np.random.default_rng(seed)
        flat = (0.3 * rng.standard_normal(pol.get_flat_params().size)).astype(np.float32)
    pol.set_flat_params(flat)
    return pol


def make_rollout(sg, T, N, O, A, F=0, ctx=None, resident=True):
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, F, ctx=ctx)
    ro.device_resident = resident
    return ro


def field_shapes(ro):
    from simgan_amd import _lib
    T, N = ro.num_steps, ro.num_processes
    return {_lib.F_OBS: (T + 1, N, ro.obs_dim), _lib.F_OBS_FEAT: (T + 1, N, ro.feat_len), _lib.F_ACTIONS: (T, N, ro.act_dim),
            _lib.F_REWARDS: (T, N, 1), _lib.F_VALUE_PREDS: (T + 1, N, 1), _lib.F_RETURNS: (T + 1, N, 1), _lib.F_LOGP: (T, N, 1),
            _lib.F_MASKS: (T + 1, N, 1), _lib.F_BAD_MASKS: (T + 1, N, 1), _lib.F_ADVANTAGES: (T, N, 1)}


def download_all(ro):
    """All ten device fields."""
    from simgan_amd import _lib
    out = {}
    for f, shape in field_shapes(ro).items():
        a = np.zeros(shape, np.float32)
        if a.size:
            _lib.check(ro.lib.sg_rollout_download(ro.h, f, _lib.fptr(a), a.size))
        out[f] = a
    return out


def download_step(ro, f, t):
    from simgan_amd import _lib
    a = np.zeros(field_shapes(ro)[f][1:], np.float32)
    _lib.check(ro.lib.sg_rollout_download_step(ro.h, f, t, _lib.fptr(a), a.size))
    return a


def slot_results(ro, t):
    from simgan_amd import _lib
    return [download_step(ro, f, t) for f in (_lib.F_VALUE_PREDS, _lib.F_ACTIONS, _lib.F_LOGP)]


def check_step_equals_act(sg, spec, N, seed=0):
    """The three noise modes at slot t = 1 of a T = 3 rollout."""
    _, O, A = SPECS[spec][:3]
    rng = np.random.default_rng(1000 * seed + N)
    pol = make_policy(sg, spec)
    ro = make_rollout(sg, 3, N, O, A)
    t = 1
    for mode in ("injected", "library", "deterministic"):
        obs = rng.standard_normal((N, O)).astype(np.float32) * 1.5
        ro.obs[t].copy_(ro.obs.new_tensor(obs))
        ro.step = t
        calls = pol._act_calls
        kw = {"injected": {"noise": rng.standard_normal((N, A)).astype(np.float32)}, "library": {},
              "deterministic": {"deterministic": True}}[mode]
        v, a, lp, _ = pol.act(obs, None, None, **kw)
        pol._act_calls = calls              # the same (seed, call count) for the step: the same library draws
        got = ro.act_step(pol, **kw)
        assert pol._act_calls == calls + 1
        dv, da, dlp = slot_results(ro, t)
        what = f"{spec} N={N} {mode}"
        assert same_bits(dv, v), f"{what}: value_preds[t]"
        assert same_bits(da, a), f"{what}: actions[t]"
        assert same_bits(dlp, lp), f"{what}: action_log_probs[t]"
        assert same_bits(got, a) and tuple(got.shape) == (N, A), f"{what}: returned action"
        assert same_bits(ro.actions[t], a), f"{what}: host mirror of actions[t]"
        assert same_bits(download_step(ro, 0, t), obs), f"{what}: obs[t] on the device"
        if mode == "library":
            assert not same_bits(a, pol.act(obs, None, None, deterministic=True)[1]), "the library draw moved nothing"


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("spec", [s for s in SPECS if s != "mlp_47_12_256"])
def test_step_has_the_bits_of_act(sg, monkeypatch, spec, N):
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    check_step_equals_act(sg, spec, N)


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("spec", ["mlp_47_12_64", "split_47_14_64_f2"])
def test_step_has_the_bits_of_act_on_the_forced_global_weight_instances(sg, monkeypatch, spec, N):
    monkeypatch.setenv("SG_POLICY_GW", "1")
    check_step_equals_act(sg, spec, N, seed=1)


@pytest.mark.parametrize("N", ROWS)
def test_step_has_the_bits_of_act_at_hidden_256(sg, monkeypatch, N):
    """A 256-wide trunk (266 KB) does not fit a CU's LDS: the global-weight instances without the switch."""
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    check_step_equals_act(sg, "mlp_47_12_256", N, seed=2)


@pytest.mark.parametrize("spec", ["mlp_47_12_64", "split_20_7_32_f1"])
def test_only_slot_t_is_written(sg, spec):
    """Sentinels in all ten device fields; steps at t = 0, a middle t and T - 1, one of them on observations that are already on
    the device (obs_host NULL behind the C ABI): nothing but obs[t] and the three slot rows changes, bit for bit."""
    from simgan_amd import _lib
    _, O, A = SPECS[spec][:3]
    T, N, F = 5, 17, 9
    rng = np.random.default_rng(7)
    pol = make_policy(sg, spec)
    ro = make_rollout(sg, T, N, O, A, F)
    want = {}
    for f, shape in field_shapes(ro).items():
        if f == _lib.F_ADVANTAGES:      # read-only: whatever the device holds is the sentinel
            continue
        a = (rng.standard_normal(shape) * 3.0 + 100.0 * (f + 1)).astype(np.float32)
        _lib.check(ro.lib.sg_rollout_upload(ro.h, f, _lib.fptr(a), a.size))
        want[f] = a
    want[_lib.F_ADVANTAGES] = download_all(ro)[_lib.F_ADVANTAGES]
    for t, resident_obs in ((0, False), (2, True), (T - 1, False)):
        noise = rng.standard_normal((N, A)).astype(np.float32)
        action = np.full((N, A), np.nan, np.float32)
        if resident_obs:
            obs = want[_lib.F_OBS][t].copy()
            _lib.check(ro.lib.sg_rollout_act_step(ro.h, pol.h, t, None, _lib.fptr(noise), 0, 0, _lib.fptr(action)))
        else:
            obs = rng.standard_normal((N, O)).astype(np.float32)
            _lib.check(ro.lib.sg_rollout_act_step(ro.h, pol.h, t, _lib.fptr(obs), _lib.fptr(noise), 0, 0, _lib.fptr(action)))
        v, a, lp, _ = pol.act(obs, None, None, noise=noise)
        assert same_bits(action, a)
        want[_lib.F_OBS][t] = obs
        want[_lib.F_VALUE_PREDS][t], want[_lib.F_ACTIONS][t], want[_lib.F_LOGP][t] = v.numpy(), a.numpy(), lp.numpy()
        got = download_all(ro)
        for f in want:
            assert same_bits(got[f], want[f]), f"field {f} after the step at t = {t}"


# ------------------------------------------------------------------------------------------------- whole collections
class ScriptedEnvs:
    """N environments whose next observation, reward, done and bad_transition are deterministic functions of the action (and of
    the step count): columns finish at different steps, every other finished column carries 'bad_transition'."""

    def __init__(self, N, O, A, F, seed):
        rng = np.random.default_rng(seed)
        self.N, self.t = N, 0
        self.Wo = rng.standard_normal((A, O)).astype(np.float32)
        self.Wf = rng.standard_normal((A, F)).astype(np.float32)

    def step(self, action):
        a = np.asarray(action.numpy() if hasattr(action, "numpy") else action, np.float32)
        assert a.shape == (self.N, self.Wo.shape[0])
        self.t += 1
        col = np.arange(self.N)
        obs = np.tanh(a @ self.Wo + 0.1 * self.t).astype(np.float32)
        reward = (a.sum(1, keepdims=True) * 0.25 + 0.01 * col[:, None]).astype(np.float32)
        done = ((self.t + col) % (3 + col % 4) == 0) | (a[:, 0] > 1.0)
        feat = np.sin(a @ self.Wf + 0.05 * self.t).astype(np.float32)
        infos = [{"sas_feat": feat[i], **({"bad_transition": True} if (done[i] and i % 2) else {})} for i in range(self.N)]
        return obs, reward, done, infos


def run_learner(sg, which, T, N, on_device):
    from simgan_amd.driver import GailDynLearner, PpoLearner
    rng = np.random.default_rng(21)
    if which == "ppo":
        spec, F = ("mlp", 13, 5, 64, 1, None), 13
    else:
        spec, F = ("split", 14, 7, 32, 1, None), 25
    _, O, A = spec[:3]
    pol = make_policy(sg, spec, seed=3)
    pol.seed, pol._act_calls = 4242, 0                  # (the constructor mixes an instance counter into the noise stream)
    agent = sg.algo.PPO(pol, 0.2, 2, 2, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    agent.seed = 12
    ro = make_rollout(sg, T, N, O, A, F)
    ro.obs[0].copy_(ro.obs.new_tensor(rng.standard_normal((N, O)).astype(np.float32)))
    if which == "ppo":
        ro.obs_feat[0].copy_(ro.obs[0])
    ro.sync_to_device()
    disc = None
    if which == "ppo":
        learner = PpoLearner(pol, agent, ro)
        collect = lambda envs: learner.collect(envs, on_device=on_device)   # noqa: E731
    else:
        disc = sg.algo.gail.Discriminator(F, 100, None, seed=2)
        disc.seed = 11
        expert = rng.standard_normal((64, F)).astype(np.float32)
        learner = GailDynLearner(pol, agent, disc, ro, expert, gail_batch_size=16, gail_epoch=2, gail_tar_length=5.0)
        collect = lambda envs: learner.collect(envs, lambda infos: np.stack([i["sas_feat"] for i in infos]), on_device=on_device)  # noqa: E731
    envs = ScriptedEnvs(N, O, A, F, seed=9)
    log = []
    for _ in range(2):                                    # twice: after_update's rollover of device and host slot 0
        before = ro.bytes_uploaded
        collect(envs)
        fields = download_all(ro)
        losses = dict(learner.update())
        log.append({"bytes": ro.bytes_uploaded - before, "fields": fields, "losses": losses, "pi": pol.get_flat_params(),
                    "d": None if disc is None else disc.get_flat_params(), "after": download_all(ro)})
    return log, (T, N, A)


@pytest.mark.parametrize("T,N", [(5, 17), (9, 33)])
@pytest.mark.parametrize("which", ["ppo", "gail_split"])
def test_whole_collections_agree(sg, which, T, N):
    """PpoLearner on a Policy and GailDynLearner on a SplitPolicy, two iterations, collect(on_device=False) against
    collect(on_device=True) from the same parameters and seeds: the ten device fields after each collection and after each
    update, the losses, the policy's and the discriminator's parameters -- all the same bits.  The on-device collection
    uploads less by exactly slots 0..T-1 of value_preds, actions and action_log_probs, the rows the device now writes itself
    (slot T of value_preds, which no step writes, still goes up so that the device rollout is what sync_to_device() leaves)."""
    host, (T, N, A) = run_learner(sg, which, T, N, False)
    dev, _ = run_learner(sg, which, T, N, True)
    for j, (h, d) in enumerate(zip(host, dev)):
        for f in h["fields"]:
            assert same_bits(h["fields"][f], d["fields"][f]), f"iteration {j}: device field {f} after the collection"
            assert same_bits(h["after"][f], d["after"][f]), f"iteration {j}: device field {f} after the update"
        assert h["losses"].keys() == d["losses"].keys()
        for k in h["losses"]:
            assert np.float64(h["losses"][k]).tobytes() == np.float64(d["losses"][k]).tobytes(), (j, k, h["losses"][k], d["losses"][k])
        assert same_bits(h["pi"], d["pi"]), f"iteration {j}: policy parameters"
        if h["d"] is not None:
            assert same_bits(h["d"], d["d"]), f"iteration {j}: discriminator parameters"
        assert h["bytes"] - d["bytes"] == 4 * T * N * (1 + A + 1), (h["bytes"], d["bytes"])
    moved = [f for f in host[0]["fields"] if not same_bits(host[0]["fields"][f], host[1]["fields"][f])]
    assert len(moved) >= 8, moved    # the second collection is another rollout: the comparison above is not of two empty ones


def test_world_2_each_rank_draws_its_own_stream(sg):
    """Loopback communicator, two ranks, the same policy, seed, call count and observations on both: act_step equals act on
    each rank (the rank enters the generator's stream as it does in k_gauss_head), and the two ranks' actions differ."""
    from test_gpu_world import run_ranks
    spec, N = "mlp_47_12_64", 33
    _, O, A = SPECS[spec][:3]
    rng = np.random.default_rng(4)
    obs = rng.standard_normal((N, O)).astype(np.float32)

    def body(rank, ctx):
        pol = make_policy(sg, spec, ctx=ctx)
        pol.seed, pol._act_calls = 777, 5
        ro = make_rollout(sg, 2, N, O, A, ctx=ctx)
        ro.obs[0].copy_(ro.obs.new_tensor(obs))
        v, a, lp, _ = pol.act(obs, None, None)
        pol._act_calls = 5
        got = ro.act_step(pol)
        dv, da, dlp = slot_results(ro, 0)
        return [np.array(x.numpy() if hasattr(x, "numpy") else x) for x in (v, a, lp, got, dv, da, dlp)]

    out = run_ranks(2, body)
    for rank, (v, a, lp, got, dv, da, dlp) in enumerate(out):
        assert same_bits(got, a) and same_bits(da, a) and same_bits(dv, v) and same_bits(dlp, lp), f"rank {rank}"
    assert same_bits(out[0][0], out[1][0]) and not same_bits(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_behind_the_c_abi(sg):
    from simgan_amd import _lib
    T, N, O, A = 3, 4, 11, 3
    pol = make_policy(sg, "mlp_11_3_64")
    ro = make_rollout(sg, T, N, O, A)
    obs, act = np.zeros((N, O), np.float32), np.zeros((N, A), np.float32)

    def call(r, p, t, out=act):
        _lib.check(r.lib.sg_rollout_act_step(r.h, p.h, t, _lib.fptr(obs), None, 1, 0, _lib.fptr(out)))

    call(ro, pol, 0)
    for t in (-1, T, T + 5):
        with pytest.raises(_lib.SimganHipError, match=r"sg_rollout_act_step: step -?\d+ out of range \[0,3\)"):
            call(ro, pol, t)
    rec = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": 32})
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step: the policy is recurrent .* holds no hidden state"):
        call(ro, rec, 0)
    cat = sg.Policy((O,), Discrete(5))
    ro_cat = sg.RolloutStorage(T, N, (O,), Discrete(5), 1, 0)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step: the policy has a Categorical / Bernoulli head"):
        call(ro_cat, cat, 0, np.zeros((N, 1), np.float32))
    for other in (make_rollout(sg, T, N, O + 1, A), make_rollout(sg, T, N, O, A + 1)):
        with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step: policy/rollout dims differ"):
            call(other, pol, 0, np.zeros((N, A + 1), np.float32))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step: NULL argument"):
        _lib.check(ro.lib.sg_rollout_act_step(ro.h, pol.h, 0, _lib.fptr(obs), None, 1, 0, None))


def test_refusals_in_python(sg):
    from simgan_amd import _lib
    from simgan_amd.driver import GailDynLearner, PpoLearner
    T, N, O, A = 3, 4, 11, 3
    pol = make_policy(sg, "mlp_11_3_64")
    host_ro = make_rollout(sg, T, N, O, A, O, resident=False)
    for call in (lambda: host_ro.act_step(pol), host_ro.finish_collect):
        with pytest.raises(ValueError, match="the rollout is not device-resident"):
            call()
    ro = make_rollout(sg, T, N, O, A, O)
    rec = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": 32})
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step: the policy is recurrent"):
        ro.act_step(rec)
    wide = make_policy(sg, ("mlp", O, A + 2, 64, 1, None))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step: policy/rollout dims differ"):
        ro.act_step(wide)
    ro.step = 0

    def ppo(p, r, **kw):
        return PpoLearner(p, sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5), r, **kw)

    with pytest.raises(ValueError, match=r"PpoLearner.collect\(on_device=True\): the rollout is not device-resident"):
        ppo(pol, host_ro).collect(None, on_device=True)
    with pytest.raises(ValueError, match=r"PpoLearner.collect\(on_device=True\): the policy is recurrent"):
        ppo(rec, make_rollout(sg, T, N, O, A, O)).collect(None, on_device=True)
    cat = sg.Policy((O,), Discrete(5))
    ro_cat = sg.RolloutStorage(T, N, (O,), Discrete(5), 1, O)
    ro_cat.device_resident = True
    with pytest.raises(ValueError, match=r"PpoLearner.collect\(on_device=True\): the policy has a Discrete / MultiBinary action space"):
        ppo(cat, ro_cat).collect(None, on_device=True)
    m_obs, m_act = np.eye(O, dtype=np.float32), np.eye(A, dtype=np.float32)
    with pytest.raises(ValueError, match=r"PpoLearner.collect\(on_device=True\): the rollout is mirror-augmented"):
        ppo(pol, make_rollout(sg, T, N, O, A, O), dup_sym=(m_obs, m_act)).collect(None, on_device=True)
    split = make_policy(sg, "split_20_7_32_f1")
    disc = sg.algo.gail.Discriminator(9, 100, None, seed=2)
    gail = GailDynLearner(split, sg.algo.PPO(split, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5), disc,
                          make_rollout(sg, T, N, 20, 7, 9, resident=False), np.zeros((16, 9), np.float32))
    with pytest.raises(ValueError, match=r"GailDynLearner.collect\(on_device=True\): the rollout is not device-resident"):
        gail.collect(None, None, on_device=True)
