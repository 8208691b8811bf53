"""GPU: the library's OWN random draws -- what every production run and every bench.py number samples -- against the host
restatement of csrc/sg_rng.hpp and of each consumer's documented (seed, stream, counter) layout (tests/rng_ref.py).

  primitives   sg_uniform / sg_perm_at on the device at the product's streams against numpy uint64, exactly; sg_normal against
               the float64 Box-Muller on 2^16 counters that include both ends of u1, within 4 x what numpy float32 costs the
               same formula (measured; SG_RNG_RECORD=<path> writes the figures: profiles/rng_parity.json)
  uniform      Categorical / Bernoulli act with no `noise` equals the same policy with noise=rng_ref.uniform(...) at the stated
               layout: actions, log-probs and values with np.array_equal, two consecutive calls
  Gaussian     the same with noise= the device's own sg_normal at the stated layout (sg_test_rng_at), bit for bit: Policy,
               SplitPolicy, the GRU and CNN bases, PolicyEnsemble, act_step, act_step_rnn, act_step_chain
  ranks        two ranks over the loopback communicator draw on SG_ACT_STREAM + rank
  permutations agent.last_perms() / D.last_draws() after updates without injected draws equal the restatement, exactly
  ACKTR        an update on the library's value noise equals the update fed sg_normal at SG_KFAC_STREAM + update, bit for bit

Every comparison but sg_normal's is exact.  A policy's seed is set explicitly (the constructor derives a per-instance one), some
of them two below 2^64 so that the per-call seed wraps."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rng_ref as rr  # noqa: E402
from test_gpu_world import run_ranks  # noqa: E402

pytestmark = pytest.mark.gpu

M64 = rr.M64
WRAP_SEED = M64 - 1      # call 1 draws on seed 2^64 - 1, call 2 on seed 0
HW = 84


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


class Discrete:
    def __init__(self, n):
        self.n = int(n)


class MultiBinary:
    def __init__(self, n):
        self.n, self.shape = int(n), (int(n),)


class Loader:
    def __init__(self, expert, batch_size):
        self.expert, self.batch_size = expert, batch_size


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    from simgan_amd import _lib
    _lib.load_test()
    return simgan_amd


def npv(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def same_bits(a, b):
    a, b = np.ascontiguousarray(npv(a)), np.ascontiguousarray(npv(b))
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def dev_draw(kind, n, seed, stream, ctr0=0, ctx=None):
    """sg_test_rng_at: n values of the device's generator at (seed, stream, ctr0 + i); kind 0: sg_fill_perm's permutation."""
    from simgan_amd import _lib
    ctx = ctx or _lib.Context.default()
    out = np.empty(n, np.int64 if kind == 0 else np.float32)
    _lib.check_test(_lib.load_test().sg_test_rng_at(ctx.h, kind, n, seed & M64, stream & M64, ctr0 & M64, out.ctypes.data_as(C.c_void_p)))
    return out


def expected_noise(kind, obj_seed, call, rank, n, width, ctx=None):
    """What the consumer must have drawn in its call-th act call: [n, width] at rng_ref.act_layout.  'uniform': the restatement's
    values (exact on any machine); 'normal': the device's own sg_normal at those counters."""
    seed, stream, ctr = rr.act_layout(obj_seed, call, rank, n, width)
    if kind == "uniform":
        return rr.uniform(seed, stream, ctr.reshape(-1)).reshape(n, width)
    assert int(ctr[0, 0]) == 0 and np.array_equal(ctr.reshape(-1), np.arange(n * width, dtype=np.uint64))
    return dev_draw(2, n * width, seed, stream, 0, ctx).reshape(n, width)


# ------------------------------------------------------------------------------------------------ primitives
PRODUCT_STREAMS = (rr.SG_ACT_STREAM, rr.SG_ACT_STREAM + 1, 0xE0000001, 0xF0000400, 3 * rr.PPO_EPOCH_MUL + 1)
SEEDS = (0, 1234, M64, (1 << 63) + 12345, rr.derive_seed(0, rr.SALT_PPO) + 1)


@pytest.mark.parametrize("stream", PRODUCT_STREAMS)
def test_device_uniform_and_permutation_equal_the_restatement(sg, stream):
    for seed in SEEDS:
        for ctr0 in (0, (1 << 32) - 7, M64 - 100):    # a counter past 2^32, and one that wraps
            got = dev_draw(1, 4099, seed, stream, ctr0)
            want = rr.uniform(seed, stream, np.arange(4099, dtype=np.uint64) + np.uint64(ctr0))
            assert np.array_equal(got, want), (seed, stream, ctr0)
        for n in (1, 2, 35, 77, 4096, 4097):
            assert np.array_equal(dev_draw(0, n, seed, stream), rr.fill_perm(n, seed, stream)), (seed, stream, n)


def test_device_normal_against_float64_box_muller(sg):
    """2^16 counters of the action stream: 2^15 from 0, and 2^14 around each of the two counters (found by scanning on the host)
    where u1 = 2^-24 (|z| = sqrt(48 ln 2) = 5.768, the generator's largest) and u1 = 1 (z = 0).  The bound is not fixed in
    advance: 4 x the largest absolute distance of the same formula in numpy float32 from the float64 one, the factor covering
    another libm's logf / cosf."""
    seed, stream = 0x5EED5EED, rr.SG_ACT_STREAM
    lo, hi = rr.find_u1_ends(seed, stream)
    u1, _ = rr.normal_uniforms(seed, stream, [lo, hi])
    assert u1[0] == 2.0 ** -24 and u1[1] == 1.0
    blocks = [(0, 1 << 15), (lo - (1 << 13), 1 << 14), (hi - (1 << 13), 1 << 14)]
    ctr = np.concatenate([np.arange(c0, c0 + n, dtype=np.uint64) for c0, n in blocks])
    got = np.concatenate([dev_draw(2, n, seed, stream, c0) for c0, n in blocks]).astype(np.float64)
    assert ctr.size == 1 << 16 and lo in ctr and hi in ctr and np.isfinite(got).all()
    z64, z32 = rr.normal64(seed, stream, ctr), rr.normal32(seed, stream, ctr).astype(np.float64)
    dev_err, f32_err = np.abs(got - z64), np.abs(z32 - z64)
    bound = 4.0 * f32_err.max()
    at = {"u1_min": int(np.nonzero(ctr == lo)[0][0]), "u1_one": int(np.nonzero(ctr == hi)[0][0])}
    rec = {"what": "tests/test_gpu_rng.py::test_device_normal_against_float64_box_muller under SG_RNG_RECORD: device sg_normal and "
                   "the numpy float32 evaluation of the same formula, absolute distance from the float64 Box-Muller (rng_ref.normal64)",
           "seed": seed, "stream": stream, "counters": int(ctr.size), "counter_u1_min": lo, "counter_u1_one": hi,
           "device_max_abs": float(dev_err.max()), "device_mean_abs": float(dev_err.mean()),
           "float32_max_abs": float(f32_err.max()), "float32_mean_abs": float(f32_err.mean()),
           "bound_applied": float(bound), "bound_rule": "4 x float32_max_abs",
           "at_u1_min": {"device": float(got[at["u1_min"]]), "float64": float(z64[at["u1_min"]]), "float32": float(z32[at["u1_min"]])},
           "at_u1_one": {"device": float(got[at["u1_one"]]), "float64": float(z64[at["u1_one"]]), "float32": float(z32[at["u1_one"]])},
           "largest_abs_z": {"device": float(np.abs(got).max()), "float64": float(np.abs(z64).max())},
           "bits_equal_to_numpy_float32": float((got.astype(np.float32) == z32.astype(np.float32)).mean())}
    print(json.dumps(rec, indent=1))
    path = os.environ.get("SG_RNG_RECORD")
    if path:
        with open(path, "w") as f:
            json.dump(rec, f, indent=1)
    assert dev_err.max() <= bound, (dev_err.max(), bound)
    assert abs(abs(z64[at["u1_min"]]) - np.sqrt(48 * np.log(2.0)) * abs(np.cos(rr.TWO_PI_F32 * rr.normal_uniforms(seed, stream, [lo])[1][0]))) < 1e-12
    assert got[at["u1_one"]] == 0.0


# ------------------------------------------------------------------------------------------------ acting policies
def set_form(monkeypatch, form):
    for name, val in zip(("SG_PPO_ROWS", "SG_POLICY_GW"), {"default": (None, None), "rows16": ("16", None), "gw": (None, "1")}[form]):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def twin_policies(make, seed, perturb=0.1):
    """Two policies with the same parameters and the same action-noise seed: `a` will draw, `b` will be fed."""
    a, b = make(), make()
    flat = a.get_flat_params()
    if perturb:   # off the initialiser's zero biases and near-zero mean heads
        flat = (flat + perturb * np.random.default_rng(7).standard_normal(flat.size)).astype(np.float32)
    a.set_flat_params(flat)
    b.set_flat_params(flat)
    a.seed = b.seed = seed
    return a, b


def check_act_draws(a, b, kind, width, obs_of_call, rank=0, ctx=None, extra=lambda call: ((None, None), {}), calls=2):
    """Calls 1..calls of `a` (library draws) against `b` fed the layout's draws; then that the comparison can see a wrong call
    number at all (the draws of call + 7 give other actions).  extra(call) -> ((rnn_hxs, masks), keyword arguments)."""
    for call in range(1, calls + 1):
        obs = obs_of_call(call)
        n = obs.shape[0]
        args, kw = extra(call)
        got = a.act(obs, *args, **kw)
        assert a._act_calls == call
        want = b.act(obs, *args, noise=expected_noise(kind, a.seed, call, rank, n, width, ctx), **kw)
        for g, w, what in zip(got[:3], want[:3], ("value", "action", "log-prob")):
            assert same_bits(g, w), f"call {call}: {what} differs from the stated layout's draws ({int((npv(g) != npv(w)).sum())} of {npv(g).size})"
        if got[3] is not None and want[3] is not None:
            assert same_bits(got[3], want[3]), f"call {call}: hidden state"
        if n * width >= 16:
            b._act_calls -= 1
            other = b.act(obs, *args, noise=expected_noise(kind, a.seed, call + 7, rank, n, width, ctx), **kw)
            assert not np.array_equal(npv(other[1]), npv(got[1])), "the comparison is blind: another call's draws give the same actions"


def fixed_obs(n, O, seed=3):
    obs = np.random.default_rng(seed).standard_normal((n, O)).astype(np.float32)
    return lambda call: obs


UNIFORM_CASES = ([("categorical", K, n, "default") for K in (2, 17, 130) for n in (1, 16, 77, 130)] +
                 [("bernoulli", K, n, "default") for K in (5, 33) for n in (1, 16, 77, 130)] +
                 [(d, K, 77, form) for d, K in (("categorical", 17), ("bernoulli", 33)) for form in ("rows16", "gw")])


@pytest.mark.parametrize("dist,K,n,form", UNIFORM_CASES)
def test_discrete_action_draws_are_the_uniforms_of_the_layout(sg, monkeypatch, dist, K, n, form):
    """Categorical: one uniform per row at counter row; Bernoulli: one per bit at counter row * K + k."""
    set_form(monkeypatch, form)
    O, H = 11, 32
    space = Discrete(K) if dist == "categorical" else MultiBinary(K)
    a, b = twin_policies(lambda: sg.Policy((O,), space, base_kwargs={"recurrent": False, "hidden_size": H}),
                         WRAP_SEED if K in (17, 33) else 20240607 + K, perturb=0.3)
    check_act_draws(a, b, "uniform", 1 if dist == "categorical" else K, fixed_obs(n, O))


@pytest.mark.parametrize("dist,K", [("categorical", 6), ("bernoulli", 5)])
def test_recurrent_discrete_action_draws(sg, dist, K):
    O, H, n = 9, 16, 77
    space = Discrete(K) if dist == "categorical" else MultiBinary(K)
    a, b = twin_policies(lambda: sg.Policy((O,), space, base_kwargs={"recurrent": True, "hidden_size": H}, recurrent_heads=True), WRAP_SEED,
                         perturb=0.3)
    rng = np.random.default_rng(2)
    hxs, masks = (0.5 * rng.standard_normal((n, H))).astype(np.float32), (rng.random((n, 1)) > 0.3).astype(np.float32)
    check_act_draws(a, b, "uniform", 1 if dist == "categorical" else K, fixed_obs(n, O), extra=lambda call: ((hxs, masks), {}))


def test_cnn_discrete_action_draws_span_two_inference_passes(sg):
    """130 rows of the CNN base are two inference passes (128 + 2): the counter is the row of the batch in both."""
    C_, Hs, K, n = 1, 16, 6, 130
    a, b = twin_policies(lambda: sg.Policy((C_, HW, HW), Discrete(K), base_kwargs={"hidden_size": Hs}), 99, perturb=0)
    obs = np.random.default_rng(4).random((n, C_ * HW * HW)).astype(np.float32)
    check_act_draws(a, b, "uniform", 1, lambda call: obs, extra=lambda call: ((None, None), {}))
    u = expected_noise("uniform", 99, 1, 0, n, 1)
    assert not np.array_equal(u[128:], u[:2]), "rows 128, 129 must not redraw rows 0, 1"


def _gauss_makers(sg):
    return {"mlp_47_12_64": (47, 12, lambda: sg.Policy((47,), Box((12,)), base_kwargs={"recurrent": False, "hidden_size": 64})),
            "split_20_7_f1": (20, 7, lambda: sg.SplitPolicy((20,), Box((7,)), base_kwargs={"hidden_size": 32, "num_feet": 1})),
            "split_30_28_f4": (30, 28, lambda: sg.SplitPolicy((30,), Box((28,)), base_kwargs={"hidden_size": 64, "num_feet": 4}))}


GAUSS_CASES = ([(spec, n, "default") for spec in ("mlp_47_12_64", "split_20_7_f1", "split_30_28_f4") for n in (1, 16, 77, 130)] +
               [(spec, 77, "gw") for spec in ("mlp_47_12_64", "split_30_28_f4")] + [("mlp_47_12_64", 16, "gw")])


@pytest.mark.parametrize("spec,n,form", GAUSS_CASES)
def test_gaussian_action_draws_are_sg_normal_at_the_layout(sg, monkeypatch, spec, n, form):
    """n = 1, 16: 16-row tiles; 77, 130: 64-row tiles over two and three workgroups; gw: the global-weight instances."""
    set_form(monkeypatch, form)
    O, A, make = _gauss_makers(sg)[spec]
    a, b = twin_policies(make, WRAP_SEED if n == 77 else 31337 + n)
    check_act_draws(a, b, "normal", A, fixed_obs(n, O), extra=lambda call: ((None, None), {}))


def test_recurrent_gaussian_action_draws(sg):
    O, A, H, n = 11, 3, 16, 77
    a, b = twin_policies(lambda: sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": H}), 4242)
    rng = np.random.default_rng(2)
    hxs, masks = (0.5 * rng.standard_normal((n, H))).astype(np.float32), (rng.random((n, 1)) > 0.3).astype(np.float32)
    check_act_draws(a, b, "normal", A, fixed_obs(n, O), extra=lambda call: ((hxs, masks), {}))


def test_cnn_gaussian_action_draws_span_two_inference_passes(sg):
    C_, Hs, A, n = 1, 16, 3, 130
    a, b = twin_policies(lambda: sg.Policy((C_, HW, HW), Box((A,)), base_kwargs={"hidden_size": Hs}), 77, perturb=0)
    obs = np.random.default_rng(4).random((n, C_ * HW * HW)).astype(np.float32)
    check_act_draws(a, b, "normal", A, lambda call: obs, extra=lambda call: ((None, None), {}))


def _members(sg, kind, O, A, H, K, seed0):
    out = []
    for k in range(K):
        p = (sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H}) if kind == "mlp" else
             sg.SplitPolicy((O,), Box((A,)), base_kwargs={"hidden_size": H, "num_feet": A // 7}))
        rng = np.random.default_rng(seed0 + k)
        p.set_flat_params((0.3 * rng.standard_normal(p.get_flat_params().size)).astype(np.float32))
        out.append(p)
    return out


def interleaved(n, K):
    return ((np.arange(n) * 7 + 1) % K).astype(np.int32)


@pytest.mark.parametrize("n", [16, 77, 130])
def test_ensemble_draws_are_counted_by_the_batch_row(sg, n):
    """K = 3 members interleaved inside every tile: a row's counter is its row in the batch, not its row within its member."""
    from simgan_amd.ensemble import PolicyEnsemble
    O, A, K = 11, 3, 3
    ens, fed = PolicyEnsemble(_members(sg, "mlp", O, A, 64, K, 40)), PolicyEnsemble(_members(sg, "mlp", O, A, 64, K, 40))
    ens.seed = fed.seed = WRAP_SEED
    ind = interleaved(n, K)
    obs = np.random.default_rng(n).standard_normal((n, O)).astype(np.float32)
    for call in (1, 2):
        got = ens.act(obs, ind=ind, full=True)
        want = fed.act(obs, ind=ind, full=True, noise=expected_noise("normal", ens.seed, call, 0, n, A))
        for g, w, what in zip(got[:3], want[:3], ("value", "action", "log-prob")):
            assert same_bits(g, w), f"call {call}: {what}"
    # the defect the layout excludes: counters that run within each member
    within = np.zeros(n, np.int64)
    for k in range(K):
        within[ind == k] = np.arange((ind == k).sum())
    z = expected_noise("normal", ens.seed, 2, 0, n, A)
    fed._calls -= 1
    wrong = fed.act(obs, ind=ind, full=True, noise=z[within])
    assert not np.array_equal(npv(wrong[1]), npv(got[1]))


# ------------------------------------------------------------------------------------------------ collection on the device
def download_step(ro, f, t, shape):
    from simgan_amd import _lib
    a = np.zeros(shape, np.float32)
    _lib.check(ro.lib.sg_rollout_download_step(ro.h, f, t, _lib.fptr(a), a.size))
    return a


def slot_results(ro, t):
    from simgan_amd import _lib
    N, A = ro.num_processes, ro.act_dim
    return [download_step(ro, f, t, s) for f, s in ((_lib.F_VALUE_PREDS, (N, 1)), (_lib.F_ACTIONS, (N, A)), (_lib.F_LOGP, (N, 1)))]


@pytest.mark.parametrize("N", [16, 77])
def test_act_step_draws_follow_the_act_call_sequence(sg, N):
    """Three steps through RolloutStorage.act_step: step t draws what the policy's (t + 1)-th act call draws."""
    O, A, T = 11, 3, 3
    make = lambda: sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": 64})  # noqa: E731
    a, b = twin_policies(make, WRAP_SEED)
    c, _ = twin_policies(make, WRAP_SEED)
    ros = []
    for _ in range(2):
        ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 0)
        ro.device_resident = True
        ros.append(ro)
    rng = np.random.default_rng(N)
    for t in range(T):
        obs = (1.5 * rng.standard_normal((N, O))).astype(np.float32)
        for ro in ros:
            ro.obs[t].copy_(ro.obs.new_tensor(obs))
            ro.step = t
        got = ros[0].act_step(a)
        want = ros[1].act_step(b, noise=expected_noise("normal", a.seed, t + 1, 0, N, A))
        assert a._act_calls == t + 1 and same_bits(got, want), f"step {t}: returned action"
        for g, w, what in zip(slot_results(ros[0], t), slot_results(ros[1], t), ("value_preds", "actions", "action_log_probs")):
            assert same_bits(g, w), f"step {t}: {what}[t]"
        assert same_bits(c.act(obs, None, None)[1], got), f"step {t}: Policy.act's call {t + 1} draws the same"


@pytest.mark.parametrize("N", [16, 33])
def test_act_step_rnn_draws_follow_the_act_call_sequence(sg, N):
    from simgan_amd import _lib
    O, A, H, T = 11, 3, 16, 3
    a, b = twin_policies(lambda: sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": H}), 987654321)
    rng = np.random.default_rng(N)
    h0 = np.zeros((T + 1, N, H), np.float32)
    h0[0] = 0.5 * rng.standard_normal((N, H))
    ros = []
    for _ in range(2):
        ro = sg.RolloutStorage(T, N, (O,), Box((A,)), H, 0)
        ro.device_resident = True
        ro.enable_device_hidden()
        _lib.check(ro.lib.sg_rollout_upload_hidden(ro.h, _lib.fptr(h0), h0.size))
        ros.append(ro)
    for t in range(T):
        obs = (1.5 * rng.standard_normal((N, O))).astype(np.float32)
        masks = (rng.random((N, 1)) > 0.3).astype(np.float32)
        for ro in ros:
            ro.obs[t].copy_(ro.obs.new_tensor(obs))
            ro.masks[t].copy_(ro.masks.new_tensor(masks))
            ro.step = t
        got = ros[0].act_step(a)
        want = ros[1].act_step(b, noise=expected_noise("normal", a.seed, t + 1, 0, N, A))
        assert same_bits(got, want), f"step {t}: returned action"
        for g, w, what in zip(slot_results(ros[0], t), slot_results(ros[1], t), ("value_preds", "actions", "action_log_probs")):
            assert same_bits(g, w), f"step {t}: {what}[t]"
    hid = []
    for ro in ros:
        h = np.zeros((T + 1, N, H), np.float32)
        _lib.check(ro.lib.sg_rollout_download_hidden(ro.h, _lib.fptr(h), h.size))
        hid.append(h)
    assert same_bits(hid[0], hid[1])


@pytest.mark.parametrize("order", ["inner_first", "learner_first"])
def test_chained_act_draws_learner_on_the_policy_seed_and_inner_on_the_ensemble_seed(sg, order):
    from simgan_amd import _lib
    from simgan_amd.ensemble import PolicyEnsemble
    N, K, T = 33, 3, 3
    inner_first = order == "inner_first"
    if inner_first:   # learner SplitPolicy 14 -> 7, members Policy 11 -> 3
        (O, A, lk, lH), (Oi, Ai, ik, iH) = (14, 7, "split", 32), (11, 3, "mlp", 64)
    else:             # learner Policy 11 -> 3, members SplitPolicy 14 -> 7
        (O, A, lk, lH), (Oi, Ai, ik, iH) = (11, 3, "mlp", 64), (14, 7, "split", 32)
    pols = [_members(sg, lk, O, A, lH, 1, 5)[0] for _ in range(2)]
    enss = [PolicyEnsemble(_members(sg, ik, Oi, Ai, iH, K, 40)) for _ in range(2)]
    for p, e in zip(pols, enss):
        p.seed, e.seed = WRAP_SEED, 0x77 + 40
    ros = []
    for _ in range(2):
        ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 0)
        ro.device_resident = True
        ros.append(ro)
    rng = np.random.default_rng(12)
    ind = interleaved(N, K)
    enss[0]._calls = enss[1]._calls = 4     # the two call counters need not agree
    for t in range(T):
        state = (1.5 * rng.standard_normal((N, 11))).astype(np.float32)
        lz = expected_noise("normal", pols[0].seed, t + 1, 0, N, A)
        iz = expected_noise("normal", enss[0].seed, 4 + t + 1, 0, N, Ai)
        assert not np.array_equal(lz.reshape(-1)[:N * min(A, Ai)], iz.reshape(-1)[:N * min(A, Ai)]), "the two halves share a noise block"
        raws = [np.empty((N, Ai), np.float32) for _ in range(2)]
        outs = []
        for i, (ro, p, e) in enumerate(zip(ros, pols, enss)):
            ro.step = t
            kw = {"noise": lz, "inner_noise": iz} if i else {}
            if inner_first:
                outs.append(ro.act_step_chain(p, e, _lib.CHAIN_INNER_FIRST, state=state, ind=ind, inner_raw_out=raws[i], **kw))
            else:
                ro.obs[t].copy_(ro.obs.new_tensor(state))
                outs.append(ro.act_step_chain(p, e, _lib.CHAIN_LEARNER_FIRST, ind=ind, inner_raw_out=raws[i], **kw))
        assert pols[0]._act_calls == t + 1 and enss[0]._calls == 4 + t + 1
        assert same_bits(outs[0][0], outs[1][0]), f"step {t}: learner action"
        assert same_bits(outs[0][1], outs[1][1]) and same_bits(raws[0], raws[1]), f"step {t}: inner action"
        for g, w, what in zip(slot_results(ros[0], t), slot_results(ros[1], t), ("value_preds", "actions", "action_log_probs")):
            assert same_bits(g, w), f"step {t}: {what}[t]"
        # ... and the halves are not swapped: feeding each half the other's seed gives other actions
        if t == 0:
            ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 0)
            ro.device_resident = True
            ro.step = 0
            pols[1]._act_calls -= 1
            enss[1]._calls -= 1
            sw_l = expected_noise("normal", enss[0].seed, 5, 0, N, A)
            sw_i = expected_noise("normal", pols[0].seed, 1, 0, N, Ai)
            if inner_first:
                sw = ro.act_step_chain(pols[1], enss[1], _lib.CHAIN_INNER_FIRST, state=state, ind=ind, noise=sw_l, inner_noise=sw_i)
            else:
                ro.obs[0].copy_(ro.obs.new_tensor(state))
                sw = ro.act_step_chain(pols[1], enss[1], _lib.CHAIN_LEARNER_FIRST, ind=ind, noise=sw_l, inner_noise=sw_i)
            assert not np.array_equal(npv(sw[0]), npv(outs[0][0])) and not np.array_equal(npv(sw[1]), npv(outs[0][1]))


# ------------------------------------------------------------------------------------------------ ranks
def test_each_rank_draws_its_action_noise_on_its_own_stream(sg):
    O, A, n, seed = 11, 3, 77, 555

    def rank_fn(rank, ctx):
        make = lambda: sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": 32}, ctx=ctx)  # noqa: E731
        a, b = twin_policies(make, seed)
        check_act_draws(a, b, "normal", A, fixed_obs(n, O), rank=rank, ctx=ctx, extra=lambda call: ((None, None), {}))
        dist = Discrete(17)
        a, b = twin_policies(lambda: sg.Policy((O,), dist, base_kwargs={"recurrent": False, "hidden_size": 32}, ctx=ctx), seed, perturb=0.3)
        check_act_draws(a, b, "uniform", 1, fixed_obs(n, O), rank=rank, ctx=ctx)
        c, _ = twin_policies(make, seed)
        return npv(c.act(fixed_obs(n, O)(1), None, None)[1]).copy()

    res = run_ranks(2, rank_fn)
    assert res[0].shape == res[1].shape == (n, A) and not np.array_equal(res[0], res[1]), "ranks 0 and 1 drew the same noise"
    assert not np.any(res[0] == res[1])


# ------------------------------------------------------------------------------------------------ permutations
def filled_rollout(sg, pol, T, N, O, space, hidden=1, F=1, ctx=None, seed=0):
    """A rollout that is consistent with `pol`: its actions, log-probs and values come from one act call on all T * N rows."""
    kw = {} if ctx is None else {"ctx": ctx}
    ro = sg.RolloutStorage(T, N, tuple(O) if isinstance(O, tuple) else (O,), space, hidden, F, **kw)
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal(tuple(ro.obs.shape)).astype(np.float32)
    ro.obs.copy_(ro.obs.new_tensor(obs))
    rows = obs[:-1].reshape(T * N, -1)
    if pol.is_recurrent:
        hx = np.zeros((N, pol.hidden_size), np.float32)
        for t in range(T):
            ro.recurrent_hidden_states[t].copy_(ro.obs.new_tensor(hx))
            v, a, lp, hx = pol.act(obs[t].reshape(N, -1), hx, npv(ro.masks[t]), deterministic=False, noise=_some_noise(pol, N, rng))
            hx = npv(hx)
            ro.actions[t].copy_(ro.actions.new_tensor(npv(a)))
            ro.action_log_probs[t].copy_(ro.action_log_probs.new_tensor(npv(lp)))
            ro.value_preds[t].copy_(ro.value_preds.new_tensor(npv(v)))
    else:
        v, a, lp, _ = pol.act(rows, None, None, noise=_some_noise(pol, T * N, rng))
        a = npv(a)
        ro.actions.copy_(ro.actions.new_tensor(a.reshape(tuple(ro.actions.shape))))
        ro.action_log_probs.copy_(ro.action_log_probs.new_tensor(npv(lp).reshape(T, N, 1)))
        ro.value_preds[:-1].copy_(ro.value_preds.new_tensor(npv(v).reshape(T, N, 1)))
    ro.returns.copy_(ro.returns.new_tensor(rng.standard_normal(tuple(ro.returns.shape)).astype(np.float32)))
    ro.obs_feat.copy_(ro.obs_feat.new_tensor(rng.standard_normal(tuple(ro.obs_feat.shape)).astype(np.float32)))
    return ro


def _some_noise(pol, n, rng):
    return (rng.random((n, pol.act_dim)) if pol.dist_kind else rng.standard_normal((n, pol.act_dim))).astype(np.float32)


@pytest.mark.parametrize("T,N", [(7, 5), (7, 11), (64, 64), (241, 17)])
def test_ppo_minibatch_permutations_are_the_restatement(sg, T, N):
    """T * N = 35, 77, 4096 (the whole Feistel domain: no cycle walking) and 4097 (3/4 of the first hits walk on); three epochs
    (stream id e * 2654435761), two consecutive updates (seed + call)."""
    O, A, E = 11, 3, 3
    assert T * N in (35, 77, 4096, 4097)
    pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": 32})
    agent = sg.algo.PPO(pol, 0.2, E, 4, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    seed = agent.seed
    assert seed == rr.derive_seed(0, rr.SALT_PPO)
    ro = filled_rollout(sg, pol, T, N, O, Box((A,)))
    for call in (1, 2):
        out = agent.update(ro)
        assert all(np.isfinite(x) for x in out)
        got = agent.last_perms()
        assert got.shape == (E, T * N) and np.array_equal(got, rr.ppo_perms(seed, call, E, T * N)), f"update {call}"
        assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(T * N), (E, 1)))
        assert not np.array_equal(got[0], got[1]) and not np.array_equal(got[1], got[2])
    assert not np.array_equal(got, rr.ppo_perms(seed, 1, E, T * N))


def test_recurrent_ppo_permutes_the_environments(sg):
    O, A, H, T, N, E = 9, 3, 16, 4, 8, 3
    pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": H})
    agent = sg.algo.PPO(pol, 0.2, E, 4, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5, seed=5)
    assert agent.seed == rr.derive_seed(5, rr.SALT_PPO)
    ro = filled_rollout(sg, pol, T, N, O, Box((A,)), hidden=H)
    for call in (1, 2):
        agent.update(ro)
        got = agent.last_perms()
        assert got.shape == (E, N) and np.array_equal(got, rr.ppo_perms(agent.seed, call, E, N)), f"update {call}"


def test_cnn_ppo_permutations(sg):
    C_, Hs, K, T, N, E = 1, 16, 6, 2, 8, 3
    pol = sg.Policy((C_, HW, HW), Discrete(K), base_kwargs={"hidden_size": Hs})
    agent = sg.algo.PPO(pol, 0.2, E, 2, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5, seed=9)
    ro = filled_rollout(sg, pol, T, N, (C_, HW, HW), Discrete(K))
    for call in (1, 2):
        agent.update(ro)
        got = agent.last_perms()
        assert got.shape == (E, T * N) and np.array_equal(got, rr.ppo_perms(agent.seed, call, E, T * N)), f"update {call}"


def test_data_parallel_ppo_adds_the_rank_to_the_stream(sg):
    O, A, T, N, E = 11, 3, 7, 5, 3

    def rank_fn(rank, ctx):
        pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": 32}, ctx=ctx)
        agent = sg.algo.PPO(pol, 0.2, E, 5, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
        agent.seed = 1234
        ro = filled_rollout(sg, pol, T, N, O, Box((A,)), ctx=ctx, seed=rank)
        out = []
        for _ in (1, 2):
            agent.update(ro)
            out.append(agent.last_perms())
        return out

    res = run_ranks(2, rank_fn)
    for rank in (0, 1):
        for call in (1, 2):
            assert np.array_equal(res[rank][call - 1], rr.ppo_perms(1234, call, E, T * N, rank=rank)), (rank, call)
    assert not np.array_equal(res[0][0], res[1][0])


# ------------------------------------------------------------------------------------------------ discriminator
NE, DT, DN, DF, DHD, DB = 300, 7, 11, 9, 16, 32


def _disc_setup(sg, ctx=None, seed=0):
    kw = {} if ctx is None else {"ctx": ctx}
    rng = np.random.default_rng(seed)
    D = sg.algo.gail.Discriminator(DF, DHD, None, seed=11, **kw)
    ro = sg.RolloutStorage(DT, DN, (5,), Box((2,)), 1, DF, **kw)
    ro.obs_feat.copy_(ro.obs_feat.new_tensor(rng.standard_normal((DT + 1, DN, DF)).astype(np.float32)))
    expert = np.random.default_rng(100).standard_normal((NE, DF)).astype(np.float32)
    return D, ro, Loader(expert, DB)


def test_discriminator_epoch_draws_are_the_restatement(sg):
    """Expert rows 300, T * N = 77, batch 32: two steps per epoch, 64 alphas.  A grad-pen call between the two epochs advances
    the object's call count (the seed) but not the handle's epoch count (the streams)."""
    D, ro, loader = _disc_setup(sg)
    assert D.seed == rr.derive_seed(11, rr.SALT_DISC)
    D.seed = M64 - 1
    n_alpha = min(NE // DB, DT * DN // DB) * DB
    D.update_gail_dyn(loader, ro)
    assert D.last_n_steps == n_alpha // DB == 2
    for got, want, what in zip(D.last_draws(), rr.disc_draws(D.seed, 1, 1, NE, DT * DN, n_alpha), ("expert perm", "policy perm", "alpha")):
        assert got.shape == want.shape and np.array_equal(got, want), f"epoch 1: {what}"
    rng = np.random.default_rng(1)
    e, p = rng.standard_normal((37, DF)).astype(np.float32), rng.standard_normal((37, DF)).astype(np.float32)
    pen = lambda **kw: npv(D.compute_grad_pen(e[:, :6], e[:, 6:], p[:, :6], p[:, 6:], **kw))  # noqa: E731
    pen_lib = pen()                                                                            # call 2
    al = rr.uniform(*rr.grad_pen_layout(D.seed, 2, 37))
    D._calls -= 1
    assert same_bits(pen_lib, pen(alpha=al)), "grad pen: alpha is not the layout's"
    D._calls -= 1
    assert not same_bits(pen_lib, pen(alpha=rr.uniform(*rr.grad_pen_layout(D.seed, 3, 37))))
    assert D._calls == 2
    D.update_gail_dyn(loader, ro)                                                              # call 3, epoch 2
    for got, want, what in zip(D.last_draws(), rr.disc_draws(D.seed, 3, 2, NE, DT * DN, n_alpha), ("expert perm", "policy perm", "alpha")):
        assert np.array_equal(got, want), f"epoch 2: {what}"
    assert got.min() >= 0.0 and got.max() < 1.0


def test_sharded_discriminator_adds_the_rank_to_the_policy_permutation(sg):
    def rank_fn(rank, ctx):
        ctx.set_disc_dp(True)
        D, ro, loader = _disc_setup(sg, ctx, seed=rank)
        D.seed = 77
        out = []
        for _ in (1, 2):
            D.update_gail_dyn(loader, ro)
            out.append((D.last_draws(), D.last_n_steps))
        return out

    res = run_ranks(2, rank_fn)
    n_d = min(NE // DB, DT * DN // (DB // 2))
    for rank in (0, 1):
        for call in (1, 2):
            draws, steps = res[rank][call - 1]
            assert steps == n_d
            want = rr.disc_draws(77, call, call, NE, DT * DN, n_d * DB, rank=rank, sharded=True)
            for got, w, what in zip(draws, want, ("expert perm", "policy perm", "alpha")):
                assert got.shape == w.shape and np.array_equal(got, w), (rank, call, what)
    assert np.array_equal(res[0][0][0][0], res[1][0][0][0]) and np.array_equal(res[0][0][0][2], res[1][0][0][2])
    assert not np.array_equal(res[0][0][0][1], res[1][0][0][1])


# ------------------------------------------------------------------------------------------------ ACKTR
def test_acktr_value_noise_is_sg_normal_on_the_kfac_stream(sg):
    """Updates 0 and 1 on the library's value noise against updates fed sg_normal at (agent.seed, SG_KFAC_STREAM + update, row):
    parameters and K-FAC factors bit for bit."""
    T, N, O, A, H = 5, 16, 11, 3, 16
    make = lambda: sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H})  # noqa: E731
    pa, pb = twin_policies(make, 1)
    agents = [sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=True, seed=3) for p in (pa, pb)]
    assert agents[0].seed == agents[1].seed == rr.derive_seed(3, rr.SALT_ACKTR)
    ros = [filled_rollout(sg, p, T, N, O, Box((A,)), seed=4) for p in (pa, pb)]
    for update in (0, 1):
        seed, stream, ctr = rr.acktr_layout(agents[0].seed, update, T * N)
        assert np.array_equal(ctr, np.arange(T * N, dtype=np.uint64))
        eps = dev_draw(2, T * N, seed, stream, 0)
        la = agents[0].update(ros[0])
        lb = agents[1].update(ros[1], value_noise=eps.reshape(T, N, 1))
        assert la == lb, (update, la, lb)
        assert same_bits(pa.get_flat_params(), pb.get_flat_params()), f"update {update}: parameters"
        ka, kb = agents[0].get_kfac(), agents[1].get_kfac()
        assert ka["steps"] == kb["steps"] == update + 1
        for name in ("m_aa", "m_gg"):
            for i, (x, y) in enumerate(zip(ka[name], kb[name])):
                assert same_bits(x, y), f"update {update}: {name}[{i}]"
        assert same_bits(ka["momentum_buffer"], kb["momentum_buffer"])
        # the stream moves with the update index: update 0's noise in update 1 gives other factors
        if update == 1:
            pc, _ = twin_policies(make, 1)
            ac = sg.algo.A2C_ACKTR(pc, 0.5, 0.01, acktr=True, seed=3)
            rc = filled_rollout(sg, pc, T, N, O, Box((A,)), seed=4)
            e0 = dev_draw(2, T * N, *rr.acktr_layout(ac.seed, 0, T * N)[:2], 0)
            ac.update(rc, value_noise=e0.reshape(T, N, 1))
            ac.update(rc, value_noise=e0.reshape(T, N, 1))
            assert not same_bits(ac.get_kfac()["m_gg"][4], ka["m_gg"][4])
