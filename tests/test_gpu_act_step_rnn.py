"""GPU: recurrent collection on the device -- the hidden-state buffer of the device rollout, sg_rollout_act_step_rnn /
RolloutStorage.act_step with a recurrent Policy, the device-side hand-over of hidden slot 0 to PPO and get_value(obs[T], h[T],
masks[T]) inside sg_rollout_compute_returns_policy -- against today's path: Policy.act + insert + sync_to_device, the host
hand-over and the host get_value.  The claim is bit identity: every comparison is on the floats' bit patterns, no tolerance.

Which instance a case reaches (csrc/sg_act_step.hip: the launcher follows the weight path of each of sg_policy_act_rnn's three
launches and the row tile class of its trunks): N <= 16 -> 16-row tiles; 17 <= N <= 32 -> 32-row tiles; N >= 33 -> 64-row tiles
where they fit (H = 100 and H = 256 stay at 32 rows and walk their GRU phases through the tile in 16-row chunks).  H = 16: one
column tile, one wave does the cell; H = 100: not a multiple of 16, W_hh (156 KB) read from global memory while W_ih and the
trunks are staged in LDS; H = 256: every weight from global memory; SG_POLICY_GW=1: the same, forced.
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


# (O, A, H, critic_hidden)
SPECS = {"gru_11_3_16": (11, 3, 16, None), "gru_47_12_64": (47, 12, 64, None), "gru_30_6_32_critic64": (30, 6, 32, 64),
         "gru_11_3_100": (11, 3, 100, None), "gru_47_12_256": (47, 12, 256, None)}
ROWS = (1, 16, 17, 33, 130)


def make_policy(sg, spec, seed=5):
    O, A, H, Hc = SPECS[spec] if isinstance(spec, str) else spec
    pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": H}, critic_hidden=Hc)
    rng = np.random.default_rng(seed)       # off the initialiser's zero biases and near-zero mean heads
    pol.set_flat_params((0.3 * rng.standard_normal(pol.get_flat_params().size)).astype(np.float32))
    return pol


def make_rollout(sg, T, N, O, A, H, F=0, hidden=True):
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), H, F)
    ro.device_resident = True
    if hidden:
        ro.enable_device_hidden()
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


def download_hidden(ro):
    from simgan_amd import _lib
    a = np.zeros(tuple(ro.recurrent_hidden_states.shape), np.float32)
    _lib.check(ro.lib.sg_rollout_download_hidden(ro.h, _lib.fptr(a), a.size))
    return a


def upload_hidden(ro, a):
    from simgan_amd import _lib
    a = np.ascontiguousarray(a, np.float32)
    _lib.check(ro.lib.sg_rollout_upload_hidden(ro.h, _lib.fptr(a), a.size))


def some_masks(rng, N):
    """Zeros and ones; zeros in row 0, the last row and a row of the second 16-row tile when there is one."""
    m = (rng.random((N, 1)) > 0.3).astype(np.float32)
    m[0] = m[N - 1] = 0.0
    if N > 16:
        m[min(19, N - 1)] = 0.0
    if N > 2:
        m[1] = 1.0
    return m


def check_step_equals_act(sg, spec, N, seed=0):
    """The three noise modes at slot t = 1 of a T = 3 rollout."""
    from simgan_amd import _lib
    O, A, H = SPECS[spec][:3]
    rng = np.random.default_rng(1000 * seed + N)
    pol = make_policy(sg, spec)
    ro = make_rollout(sg, 3, N, O, A, H)
    t = 1
    for mode in ("injected", "library", "deterministic"):
        obs = rng.standard_normal((N, O)).astype(np.float32) * 1.5
        hxs = (rng.standard_normal((N, H)) * 0.8 + 0.1).astype(np.float32)
        masks = some_masks(rng, N)
        hid = (rng.standard_normal((4, N, H)) * 0.5).astype(np.float32)
        hid[t] = hxs
        upload_hidden(ro, hid)
        ro.obs[t].copy_(ro.obs.new_tensor(obs))
        ro.masks[t].copy_(ro.masks.new_tensor(masks))
        ro.step = t
        calls = pol._act_calls
        kw = {"injected": {"noise": rng.standard_normal((N, A)).astype(np.float32)}, "library": {},
              "deterministic": {"deterministic": True}}[mode]
        v, a, lp, hx = pol.act(obs, hxs, masks, **kw)
        pol._act_calls = calls              # the same (seed, call count) for the step: the same library draws
        got = ro.act_step(pol, **kw)
        assert pol._act_calls == calls + 1
        dev = download_all(ro)
        what = f"{spec} N={N} {mode}"
        assert same_bits(dev[_lib.F_VALUE_PREDS][t], v), f"{what}: value_preds[t]"
        assert same_bits(dev[_lib.F_ACTIONS][t], a), f"{what}: actions[t]"
        assert same_bits(dev[_lib.F_LOGP][t], lp), f"{what}: action_log_probs[t]"
        assert same_bits(got, a) and tuple(got.shape) == (N, A), f"{what}: returned action"
        assert same_bits(ro.actions[t], a), f"{what}: host mirror of actions[t]"
        dh = download_hidden(ro)
        assert same_bits(dh[t + 1], hx), f"{what}: hidden slot t + 1"
        hid[t + 1] = dh[t + 1]
        assert same_bits(dh, hid), f"{what}: the other hidden slots"
        assert same_bits(dev[_lib.F_OBS][t], obs), f"{what}: obs[t] on the device"
        assert same_bits(dev[_lib.F_MASKS][t], masks), f"{what}: masks[t] on the device"
        if mode == "library":
            assert not same_bits(a, pol.act(obs, hxs, masks, deterministic=True)[1]), "the library draw moved nothing"


def _lds_budget(O, A, H):
    """csrc/sg_gru_kernels.hpp: sg_gru_scan_lds(g, gw=false) and csrc/sg_policy_fwd.hpp: fwd_lds_bytes(d, MT=1) of the heads on h,
    in bytes, and the room the launchers compare them with (a gfx950 workgroup's 160 KiB of LDS less 1 KiB)."""
    pad = lambda x: (x + 15) & ~15   # noqa: E731
    ld = lambda x: pad(x) + 4        # noqa: E731
    Hp, ldH = pad(H), ld(H)
    trunk = lambda P, ex: Hp * ldH + Hp + Hp * ldH + Hp + pad(P) * ldH + pad(P) + (pad(ex) if ex else 0)   # noqa: E731
    scan = 4 * (3 * Hp * ldH + 2 * 16 * ldH)
    fwd = 4 * (max(trunk(A, A), trunk(1, 0)) + 16 * ldH + 2 * 16 * ldH + 16 * max(ld(A), ld(1)))
    return scan, fwd, 160 * 1024 - 1024


def test_hidden_100_mixes_the_weight_paths():
    """(11, 3, 100): the cell step reads W_hh from global memory while the trunks stay in LDS -- the case in which the phases of
    the one launch disagree about their weight path.  H = 64 takes LDS for both, H = 256 global memory for both."""
    scan, fwd, room = _lds_budget(11, 3, 100)
    assert scan > room >= fwd, (scan, fwd, room)
    scan, fwd, room = _lds_budget(47, 12, 64)
    assert scan <= room and fwd <= room
    scan, fwd, room = _lds_budget(47, 12, 256)
    assert scan > room and fwd > room


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("spec", list(SPECS))
def test_step_has_the_bits_of_act(sg, monkeypatch, spec, N):
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    check_step_equals_act(sg, spec, N)


@pytest.mark.parametrize("N", ROWS)
def test_step_has_the_bits_of_act_on_the_forced_global_weight_instances(sg, monkeypatch, N):
    monkeypatch.setenv("SG_POLICY_GW", "1")
    check_step_equals_act(sg, "gru_47_12_64", N, seed=1)


def test_only_the_named_slots_are_written(sg):
    """Sentinels in all ten device fields and in the hidden buffer; one step at t = 1 with host observations and masks, then one
    at t = 3 on slots that are already on the device (obs_host and masks_host NULL behind the C ABI): nothing changes but slot t
    of OBS, MASKS, VALUE_PREDS, ACTIONS and LOGP and slot t + 1 of the hidden states, bit for bit."""
    from simgan_amd import _lib
    O, A, H = SPECS["gru_47_12_64"][:3]
    T, N, F = 5, 17, 9
    rng = np.random.default_rng(7)
    pol = make_policy(sg, "gru_47_12_64")
    ro = make_rollout(sg, T, N, O, A, H, F)
    want = {}
    for f, shape in field_shapes(ro).items():
        if f == _lib.F_ADVANTAGES:      # read-only: whatever the device holds is the sentinel
            continue
        a = (rng.standard_normal(shape) * 3.0 + 100.0 * (f + 1)).astype(np.float32)
        if f == _lib.F_MASKS:
            a[3] = some_masks(rng, N)   # the step at t = 3 reads this slot from the device
        if f == _lib.F_OBS:
            a[3] = rng.standard_normal((N, O)).astype(np.float32)
        _lib.check(ro.lib.sg_rollout_upload(ro.h, f, _lib.fptr(a), a.size))
        want[f] = a
    want[_lib.F_ADVANTAGES] = download_all(ro)[_lib.F_ADVANTAGES]
    hid = (rng.standard_normal((T + 1, N, H)) * 0.7).astype(np.float32)
    upload_hidden(ro, hid)
    for t, resident in ((1, False), (3, True)):
        noise = rng.standard_normal((N, A)).astype(np.float32)
        action = np.full((N, A), np.nan, np.float32)
        if resident:
            obs, masks = want[_lib.F_OBS][t].copy(), want[_lib.F_MASKS][t].copy()
            _lib.check(ro.lib.sg_rollout_act_step_rnn(ro.h, pol.h, t, None, None, _lib.fptr(noise), 0, 0, _lib.fptr(action)))
        else:
            obs, masks = rng.standard_normal((N, O)).astype(np.float32), some_masks(rng, N)
            _lib.check(ro.lib.sg_rollout_act_step_rnn(ro.h, pol.h, t, _lib.fptr(obs), _lib.fptr(masks), _lib.fptr(noise), 0, 0,
                                                      _lib.fptr(action)))
        v, a, lp, hx = pol.act(obs, hid[t], masks, noise=noise)
        assert same_bits(action, a)
        want[_lib.F_OBS][t], want[_lib.F_MASKS][t] = obs, masks
        want[_lib.F_VALUE_PREDS][t], want[_lib.F_ACTIONS][t], want[_lib.F_LOGP][t] = v.numpy(), a.numpy(), lp.numpy()
        hid[t + 1] = hx.numpy()
        got = download_all(ro)
        for f in want:
            assert same_bits(got[f], want[f]), f"field {f} after the step at t = {t}"
        assert same_bits(download_hidden(ro), hid), f"hidden states after the step at t = {t}"


# ------------------------------------------------------------------------------------------------- whole collections
def run_learner(sg, T, N, on_device, which="ppo"):
    from simgan_amd.driver import GailDynLearner, PpoLearner
    from test_gpu_act_step import ScriptedEnvs
    rng = np.random.default_rng(21)
    O, A, H, F = (13, 5, 32, 13) if which == "ppo" else (14, 7, 32, 25)
    pol = make_policy(sg, (O, A, H, None), seed=3)
    pol.seed, pol._act_calls = 4242, 0                  # (the constructor mixes an instance counter into the noise stream)
    agent = sg.algo.PPO(pol, 0.2, 2, 3, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    agent.seed = 12
    ro = make_rollout(sg, T, N, O, A, H, F, hidden=False)
    ro.obs[0].copy_(ro.obs.new_tensor(rng.standard_normal((N, O)).astype(np.float32)))
    if which == "ppo":
        ro.obs_feat[0].copy_(ro.obs[0])
    ro.recurrent_hidden_states[0].copy_(ro.obs.new_tensor((rng.standard_normal((N, H)) * 0.5).astype(np.float32)))
    ro.sync_to_device()
    if on_device:
        ro.enable_device_hidden()
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
    for _ in range(2):                                    # twice: after_update's rollover of hidden slot T -> 0 on the device
        before = ro.bytes_uploaded
        collect(envs)
        fields = download_all(ro)
        hidden = download_hidden(ro) if on_device else ro.recurrent_hidden_states.numpy().copy()
        dict(learner.update())
        m, v = agent.get_adam()[:2]
        log.append({"bytes": ro.bytes_uploaded - before, "fields": fields, "hidden": hidden, "pi": pol.get_flat_params(),
                    "m": np.array(m), "v": np.array(v), "after": download_all(ro)})
    return log


@pytest.mark.parametrize("which", ["ppo", "gail"])
def test_whole_collections_agree(sg, which):
    """Two PpoLearners (and two GailDynLearners) on a recurrent policy from the same parameters and seeds, T = 5, N = 33, episode ends in several columns
    and steps: collect() through insert + sync_to_device and the host hand-overs, against enable_device_hidden() +
    collect(on_device=True).  After each collection the ten device fields and the [T+1, N, H] hidden states (the host learner's:
    its host tensor) agree; after each update the fields, the flat parameters and the Adam moments agree -- all bit for bit."""
    T, N = 5, 33
    host = run_learner(sg, T, N, False, which)
    dev = run_learner(sg, T, N, True, which)
    for j, (h, d) in enumerate(zip(host, dev)):
        for f in h["fields"]:
            assert same_bits(h["fields"][f], d["fields"][f]), f"iteration {j}: device field {f} after the collection"
            assert same_bits(h["after"][f], d["after"][f]), f"iteration {j}: device field {f} after the update"
        assert same_bits(h["hidden"], d["hidden"]), f"iteration {j}: hidden states after the collection"
        assert same_bits(h["pi"], d["pi"]), f"iteration {j}: policy parameters"
        assert same_bits(h["m"], d["m"]) and same_bits(h["v"], d["v"]), f"iteration {j}: Adam moments"
        assert d["bytes"] < h["bytes"], (h["bytes"], d["bytes"])
    from simgan_amd import _lib
    assert (host[0]["fields"][_lib.F_MASKS] == 0).sum() >= 4 and not same_bits(host[0]["hidden"], host[1]["hidden"])
    assert not same_bits(host[0]["pi"], host[1]["pi"])


def test_after_update_rolls_the_hidden_states(sg):
    """Hidden slot 0 becomes the former slot T, the other slots stay; the fields roll as they always did."""
    from simgan_amd import _lib
    ro = make_rollout(sg, 4, 17, 11, 3, 16)
    rng = np.random.default_rng(2)
    hid = rng.standard_normal((5, 17, 16)).astype(np.float32)
    upload_hidden(ro, hid)
    for f in (_lib.F_OBS, _lib.F_MASKS, _lib.F_VALUE_PREDS):
        a = rng.standard_normal(field_shapes(ro)[f]).astype(np.float32)
        _lib.check(ro.lib.sg_rollout_upload(ro.h, f, _lib.fptr(a), a.size))
    before = download_all(ro)
    ro.after_update()
    hid[0] = hid[4]
    assert same_bits(download_hidden(ro), hid)
    after = download_all(ro)
    for f in (_lib.F_OBS, _lib.F_OBS_FEAT, _lib.F_MASKS, _lib.F_BAD_MASKS):
        before[f][0] = before[f][-1]
    for f in before:
        assert same_bits(after[f], before[f]), f
    plain = make_rollout(sg, 4, 17, 11, 3, 16, hidden=False)    # without hidden states: today's launch
    plain.after_update()


@pytest.mark.parametrize("use_gae", [True, False])
def test_compute_returns_policy_with_device_hidden(sg, use_gae):
    """returns and value_preds[T] from sg_rollout_compute_returns_policy on a rollout with hidden states equal those from the
    host's get_value(obs[T], h[T], masks[T]) handed to sg_rollout_compute_returns."""
    from simgan_amd import _lib
    spec = "gru_30_6_32_critic64"
    O, A, H = SPECS[spec][:3]
    T, N = 4, 33
    rng = np.random.default_rng(11)
    pol = make_policy(sg, spec)
    ro = make_rollout(sg, T, N, O, A, H)
    state = {}
    for f, shape in field_shapes(ro).items():
        if f == _lib.F_ADVANTAGES or not np.prod(shape):
            continue
        a = rng.standard_normal(shape).astype(np.float32)
        if f in (_lib.F_MASKS, _lib.F_BAD_MASKS):
            a = (rng.random(shape) > 0.25).astype(np.float32)
        state[f] = a
    hid = (rng.standard_normal((T + 1, N, H)) * 0.6).astype(np.float32)

    def load():
        for f, a in state.items():
            _lib.check(ro.lib.sg_rollout_upload(ro.h, f, _lib.fptr(a), a.size))
        upload_hidden(ro, hid)

    load()
    nv = _lib.as_f32(pol.get_value(state[_lib.F_OBS][T], hid[T], state[_lib.F_MASKS][T])).reshape(-1)
    _lib.check(ro.lib.sg_rollout_compute_returns(ro.h, _lib.fptr(nv), 1 if use_gae else 0, 0.99, 0.95, 1))
    want = download_all(ro)
    load()
    _lib.check(ro.lib.sg_rollout_compute_returns_policy(ro.h, pol.h, 1 if use_gae else 0, 0.99, 0.95, 1))
    got = download_all(ro)
    assert same_bits(got[_lib.F_RETURNS], want[_lib.F_RETURNS])
    assert same_bits(got[_lib.F_VALUE_PREDS], want[_lib.F_VALUE_PREDS])
    if use_gae:
        assert same_bits(got[_lib.F_VALUE_PREDS][T], nv)
    assert not same_bits(got[_lib.F_RETURNS][:T], state[_lib.F_RETURNS][:T])
    for f in state:
        if f not in (_lib.F_RETURNS, _lib.F_VALUE_PREDS):
            assert same_bits(got[f], state[f]), f
    assert same_bits(download_hidden(ro), hid)


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_behind_the_c_abi(sg):
    from simgan_amd import _lib
    T, N, O, A, H = 3, 4, 11, 3, 16
    pol = make_policy(sg, "gru_11_3_16")
    ro = make_rollout(sg, T, N, O, A, H)
    lib = ro.lib
    obs, masks, act = np.zeros((N, O), np.float32), np.ones(N, np.float32), np.zeros((N, A), np.float32)

    def call(r, p, t, out=act):
        _lib.check(lib.sg_rollout_act_step_rnn(r.h, p.h, t, _lib.fptr(obs), _lib.fptr(masks), None, 1, 0, _lib.fptr(out)))

    call(ro, pol, 0)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: NULL argument"):
        _lib.check(lib.sg_rollout_act_step_rnn(ro.h, pol.h, 0, _lib.fptr(obs), _lib.fptr(masks), None, 1, 0, None))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: NULL argument"):
        _lib.check(lib.sg_rollout_act_step_rnn(None, pol.h, 0, _lib.fptr(obs), _lib.fptr(masks), None, 1, 0, _lib.fptr(act)))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: NULL argument"):
        _lib.check(lib.sg_rollout_act_step_rnn(ro.h, None, 0, _lib.fptr(obs), _lib.fptr(masks), None, 1, 0, _lib.fptr(act)))
    ff = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": 16})
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: the policy is feed-forward"):
        call(ro, ff, 0)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: the rollout holds no hidden states"):
        call(make_rollout(sg, T, N, O, A, H, hidden=False), pol, 0)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: the rollout's hidden states are 32 wide, the policy's 16"):
        call(make_rollout(sg, T, N, O, A, 32), pol, 0)
    for other in (make_rollout(sg, T, N, O + 1, A, H), make_rollout(sg, T, N, O, A + 1, H)):
        with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: policy/rollout dims differ"):
            call(other, pol, 0, np.zeros((N, A + 1), np.float32))
    for t in (-1, T, T + 5):
        with pytest.raises(_lib.SimganHipError, match=r"sg_rollout_act_step_rnn: step -?\d+ out of range \[0,3\)"):
            call(ro, pol, t)
    mirrored = make_rollout(sg, T, N, O, A, H)
    _lib.check(lib.sg_rollout_set_mirrors(mirrored.h, None, _lib.fptr(np.eye(A, dtype=np.float32))))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: the rollout is mirror-augmented"):
        call(mirrored, pol, 0)
    other_ctx = _lib.Context(0)
    far = sg.RolloutStorage(T, N, (O,), Box((A,)), H, 0, ctx=other_ctx)
    _lib.check(lib.sg_rollout_enable_hidden(far.h, H))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: the policy and the rollout live on different contexts"):
        call(far, pol, 0)
    # the buffer itself
    hid = np.zeros((T + 1, N, H), np.float32)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_upload_hidden: the hidden states hold 256 floats, got 255"):
        _lib.check(lib.sg_rollout_upload_hidden(ro.h, _lib.fptr(hid), hid.size - 1))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_download_hidden: the hidden states hold 256 floats, got 64"):
        _lib.check(lib.sg_rollout_download_hidden(ro.h, _lib.fptr(hid), 64))
    _lib.check(lib.sg_rollout_enable_hidden(ro.h, H))           # the same width again: nothing happens
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_enable_hidden: the rollout already holds hidden states of width 16, not 32"):
        _lib.check(lib.sg_rollout_enable_hidden(ro.h, 32))
    bare = make_rollout(sg, T, N, O, A, H, hidden=False)
    for fn in (lib.sg_rollout_upload_hidden, lib.sg_rollout_download_hidden):
        with pytest.raises(_lib.SimganHipError, match="the rollout holds no hidden states"):
            _lib.check(fn(bare.h, _lib.fptr(hid), hid.size))
    agent = sg.algo.PPO(pol, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    with pytest.raises(_lib.SimganHipError, match="sg_ppo_set_hidden_states_rollout: the rollout holds no hidden states"):
        _lib.check(lib.sg_ppo_set_hidden_states_rollout(agent.h, bare.h))
    with pytest.raises(_lib.SimganHipError, match="sg_ppo_set_hidden_states must hand over"):
        _lib.check(lib.sg_ppo_update(agent.h, ro.h, None, 0, 0, (C.c_float * 3)()))
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_compute_returns_policy: the policy is recurrent"):
        _lib.check(lib.sg_rollout_compute_returns_policy(bare.h, pol.h, 1, 0.99, 0.95, 1))


def test_refusals_in_python(sg):
    from simgan_amd import _lib
    from simgan_amd.driver import PpoLearner
    T, N, O, A, H = 3, 4, 11, 3, 16
    pol = make_policy(sg, "gru_11_3_16")
    host_ro = sg.RolloutStorage(T, N, (O,), Box((A,)), H, O)
    with pytest.raises(ValueError, match="enable_device_hidden: the rollout is not device-resident"):
        host_ro.enable_device_hidden()
    ff_ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, O)
    ff_ro.device_resident = True
    with pytest.raises(ValueError, match="enable_device_hidden: recurrent_hidden_state_size is 1"):
        ff_ro.enable_device_hidden()
    dup = make_rollout(sg, T, N, O, A, H, O, hidden=False)
    dup.enable_dup_sym(np.eye(O, dtype=np.float32), np.eye(A, dtype=np.float32))
    with pytest.raises(ValueError, match="enable_device_hidden: the rollout is mirror-augmented"):
        dup.enable_device_hidden()
    assert not host_ro.device_hidden and not ff_ro.device_hidden and not dup.device_hidden
    with pytest.raises(ValueError, match="enable_dup_sym: the rollout holds its hidden states on the device"):    # ... nor the other way round
        make_rollout(sg, T, N, O, A, H, O).enable_dup_sym(np.eye(O, dtype=np.float32), np.eye(A, dtype=np.float32))
    # without the opt-in a recurrent policy meets today's messages
    bare = make_rollout(sg, T, N, O, A, H, O, hidden=False)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step: the policy is recurrent"):
        bare.act_step(pol)
    agent = sg.algo.PPO(pol, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    with pytest.raises(ValueError, match=r"PpoLearner.collect\(on_device=True\): the policy is recurrent and the device rollout holds no hidden state"):
        PpoLearner(pol, agent, bare).collect(None, on_device=True)
