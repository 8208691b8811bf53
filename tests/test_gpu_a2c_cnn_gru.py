"""GPU: A2C through time on the recurrent CNN base -- A2C_ACKTR(..., recurrent_cnn=True) / sg_a2c_create_cnn_rnn: per environment
group k_cnn_gru_index_group, the trunk, k_gru_pad_rows, k_gru_inproj, the scans, k_cnn_head_loss_a2c_idx, k_cnn_head_dh, the
accumulate forms of k_cnn_head_wgrad, k_gru_reduce_acc and k_cnn_reduce, k_gru_wgrad, k_gru_dx; then k_sumsq and one k_a2c_rmsprop
over both blocks (csrc/sg_ppo.hip: a2c_cnn_gru_update) -- against float64 autograd per parameter block (tests/a2c_cnn_gru_ref.py,
whose cases tests/test_a2c_cnn_gru_host.py admits), the float64 RMSprop recurrence and the reference-written fixtures
(tools/gen_golden_a2c_cnn_gru.py).

The one-step gradient is recovered from the optimizer as in tests/test_gpu_a2c_cnn.py: a first RMSprop step from square_avg = 0
leaves square_avg = (1 - alpha) g^2, so g = sign(p0 - p1) sqrt(square_avg / (1 - alpha)); the clip is put out of reach for those
runs and eps = 1e-12.
SG_A2C_CNN_GRU_RECORD=<path> collects the measured worst block per case (profiles/a2c_cnn_gru_parity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import a2c_cnn_gru_ref as ref
import cnn_gru_ref as gr
import cnn_ref as cr
from helpers import RTOL, assert_close, load

pytestmark = pytest.mark.gpu

HW = 84
HP = dict(value_loss_coef=ref.VCOEF, entropy_coef=ref.ECOEF, lr=ref.LR, eps=ref.EPS, alpha=ref.ALPHA, max_grad_norm=ref.MAX_GRAD_NORM)
KNOB = "SG_A2C_CNN_GRU_GROUP_ENVS"


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


class Discrete(object):
    def __init__(self, n):
        self.n = int(n)


class Box(object):
    def __init__(self, shape):
        self.shape = tuple(shape)


def space(dist, P):
    return Discrete(P) if dist == "categorical" else Box((P,))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _policy(sg, C_, Hs, dist, P, params=None):
    p = sg.Policy((C_, HW, HW), space(dist, P), base_kwargs={"recurrent": True, "hidden_size": Hs}, recurrent_cnn=True)
    assert [(n, tuple(s)) for n, s in p.param_shapes()] == gr.param_shapes(C_, Hs, dist, P)
    if params is not None:
        p.set_flat_params(np.asarray(params, np.float32))
    return p


def _agent(sg, p, **over):
    m = dict(HP, **over)
    return sg.algo.A2C_ACKTR(p, m["value_loss_coef"], m["entropy_coef"], lr=m["lr"], eps=m["eps"], alpha=m["alpha"],
                             max_grad_norm=m["max_grad_norm"], recurrent_cnn=True)


def _rollout(sg, C_, Hs, dist, P, T, N, resident=False, **fields):
    ro = sg.RolloutStorage(T, N, (C_, HW, HW), space(dist, P), Hs, 1)
    for name, arr in fields.items():
        t = getattr(ro, name)
        t.copy_(t.new_tensor(np.asarray(arr).reshape(tuple(t.shape))))
    if resident:
        ro.sync_to_device()
        ro.device_resident = True
    return ro


def _case_rollout(sg, c, resident=False):
    return _rollout(sg, c.C, c.Hs, c.dist, c.P, c.T, c.N, resident, obs=c.obs, actions=c.actions, returns=c.returns, masks=c.masks,
                    recurrent_hidden_states=c.hxs)


def _run(sg, c, updates=1, resident=False, fetch=True, **over):
    """-> (agent, policy, [losses per update]) after `updates` updates on the case's rollout"""
    p = _policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = _agent(sg, p, **over)
    ro = _case_rollout(sg, c, resident)
    return agent, p, [agent.update(ro, fetch_losses=fetch) for _ in range(updates)]


def _record(label, rec):
    path = os.environ.get("SG_A2C_CNN_GRU_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_a2c_cnn_gru.py under SG_A2C_CNN_GRU_RECORD: one-step gradients per parameter block as the rel-L2 "
                       "distance of tests/cnn_ref.py:block_distances to float64 autograd, over RTOL = 1e-4 (the bound is 1); the losses' "
                       "largest error over ATOL + RTOL |ref|", "cases": {}}
    doc["cases"][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def _hold_gradient(sg, key, label):
    """the recovered one-step gradient against float64 autograd per block; exactly 0 where torch's is 0 in both precisions; the
    losses with assert_close -> the recovered gradient"""
    c = ref.case(key)
    want, want_losses, _, zeros = ref.admitted(key)
    agent, p, losses = _run(sg, c, max_grad_norm=ref.NO_CLIP, eps=ref.EPS_RECOVER)
    sq, step = agent.get_rmsprop()
    assert step == 1
    got = ref.recovered_gradient(c.params, p.get_flat_params(), sq)
    d = cr.block_distances(got, want, c.shapes)
    lr_ = float(np.max(np.abs(np.asarray(losses[0]) - want_losses) / (cr.ATOL + RTOL * np.abs(want_losses))))
    print(f"{label}: worst block {max(d, key=d.get)} {max(d.values()) / RTOL:.3f} x RTOL, losses {lr_:.3f} of tol")
    _record(label, {"worst_block": max(d, key=d.get), "worst": max(d.values()) / RTOL, "losses": lr_})
    assert_close(losses[0], want_losses, what=f"{label} losses")
    bad = {k: x for k, x in d.items() if not x <= RTOL}
    assert not bad, f"{label}: blocks past {RTOL:g}: {bad}"
    assert not np.any(got[zeros]), f"{label}: {np.count_nonzero(got[zeros])} of {zeros.size} exact zeros are not zero"
    return got


# ------------------------------------------------------------------------------------------- gradient per block vs float64
@pytest.mark.parametrize("key,group", ref.GPU_CASES, ids=[ref.tag(k, g).replace(" ", "_") for k, g in ref.GPU_CASES])
def test_one_step_gradient_per_block(sg, monkeypatch, key, group):
    if group:
        assert ref.geometry(key[4], key[5], group)["n_groups"] > 1
        monkeypatch.setenv(KNOB, str(group))
    else:
        monkeypatch.delenv(KNOB, raising=False)
        assert ref.geometry(key[4], key[5])["n_groups"] == 1
    got = _hold_gradient(sg, key, "gradient " + ref.tag(key, group))
    if key == ref.FC_ZERO:
        assert ref.admitted(key)[3].size >= gr.ZERO_UNITS * (32 * 7 * 7 + 1)
        assert np.count_nonzero(got) > got.size // 2


NARROW = [(k, g) for k, g in ref.GPU_CASES if k != ref.WIDE]


@pytest.mark.parametrize("key,group", NARROW, ids=[ref.tag(k, g).replace(" ", "_") for k, g in NARROW])
def test_one_step_gradient_on_the_global_weight_instances(sg, monkeypatch, key, group):
    """the narrow cases again with the GRU's weights read from global memory (the instances Hs = 512 runs by LDS size)"""
    monkeypatch.setenv("SG_POLICY_GW", "1")
    if group:
        monkeypatch.setenv(KNOB, str(group))
    else:
        monkeypatch.delenv(KNOB, raising=False)
    _hold_gradient(sg, key, "gradient (global weights) " + ref.tag(key, group))


# ------------------------------------------------------------------------------------------- the step, the state
@pytest.mark.parametrize("key", list(ref.CLIP_CASES), ids=[ref.tag(k).replace(" ", "_") for k in ref.CLIP_CASES])
def test_the_clip_acts_over_both_blocks(sg, monkeypatch, key):
    """max_grad_norm = half the float64 gradient norm: the step is lr g factor / (sqrt(sq) + eps) with float64's g and ONE factor
    over the CNN and GRU blocks together"""
    group, norm = ref.CLIP_CASES[key]
    monkeypatch.setenv(KNOB, str(group))
    c = ref.case(key)
    mgn = float(np.float32(0.5 * norm))
    r = ref.update64(c, max_grad_norm=mgn)
    assert 0.45 < r["factor"] < 0.55
    agent, p, losses = _run(sg, c, max_grad_norm=mgn)
    sq, _ = agent.get_rmsprop()
    step64 = c.params.astype(np.float64) - r["params"]
    d = cr.block_distances(c.params.astype(np.float64) - p.get_flat_params(), step64, c.shapes)
    _record("step with the clip acting " + ref.tag(key, group), {"clip_factor": r["factor"], "worst": max(d.values()) / RTOL})
    assert max(d.values()) <= RTOL, d
    assert_close(sq, r["square_avg"], rtol=1e-3, atol=1e-12, what="square_avg = (1 - alpha) (g factor)^2")
    assert_close(losses[0], r["losses"], what="losses")


def test_square_avg_per_block_in_state_dict_order(sg, monkeypatch):
    """get_rmsprop after one unclipped step is (1 - alpha) g^2 block by block: the GRU's four tensors first, then the CNN order"""
    monkeypatch.setenv(KNOB, "2")
    key = (2, 20, ref.BOX, 3, 3, 3)
    c = ref.case(key)
    g64 = ref.admitted(key)[0]
    agent, p, _ = _run(sg, c, max_grad_norm=ref.NO_CLIP)
    sq, step = agent.get_rmsprop()
    assert step == 1 and sq.size == p.num_params == g64.size
    want = (1.0 - ref.ALPHA) * g64 ** 2
    d = cr.block_distances(sq, want, c.shapes)
    assert max(d.values()) <= 4 * RTOL, d      # (g^2: twice the gradient's relative error, both sides of the bound)
    k = gr.n_gru(c.Hs)
    assert np.linalg.norm(sq[:k] - want[:k]) < 0.01 * np.linalg.norm(want[:k]) < np.linalg.norm(sq[:k] - want[k:2 * k])


def test_rmsprop_state_round_trip_and_the_lr(sg):
    c = ref.case((1, 16, ref.CAT, 5, 1, 3))
    agent, p, _ = _run(sg, c)
    n = p.num_params
    state = np.arange(1, n + 1, dtype=np.float32) * 1e-6
    agent.set_rmsprop(state, 7)
    back, step = agent.get_rmsprop()
    assert step == 7 and np.array_equal(back, state)
    from simgan_amd import _lib
    with pytest.raises(_lib.SimganHipError, match="sg_a2c_set_rmsprop: bad length"):
        agent.set_rmsprop(state[1:], 7)
    agent.optimizer.param_groups[0]["lr"] = 0.0      # reaches the device: the next update moves nothing
    before = p.get_flat_params()
    agent.update(_case_rollout(sg, c))
    assert np.array_equal(before, p.get_flat_params()) and agent.get_rmsprop()[1] == 8


# ------------------------------------------------------------------------------------------- determinism
def test_same_bits_twice_on_replay_and_against_direct_launches(sg, monkeypatch):
    """4 x 34 in groups of 17: two scan workgroups per group, every gradient accumulating inside the graph"""
    monkeypatch.setenv(KNOB, "17")
    c = ref.case((1, 16, ref.CAT, 5, 4, 34))
    out = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        agent, p, losses = _run(sg, c, updates=2)      # (the second update of a graph run is a replay)
        out.append((losses, p.get_flat_params(), agent.get_rmsprop()[0]))
    for other in out[1:]:
        assert out[0][0] == other[0]
        assert np.array_equal(bits(out[0][1]), bits(other[1]))
        assert np.array_equal(bits(out[0][2]), bits(other[2]))
    assert np.isfinite(out[0][1]).all() and np.abs(out[0][1] - c.params).max() > 1e-4


def test_host_resident_and_queued_updates_give_the_same_bits(sg):
    c = ref.case((1, 16, ref.CAT, 5, 4, 4))
    a1, p1, l1 = _run(sg, c)
    a2, p2, l2 = _run(sg, c, resident=True)
    a3, p3, l3 = _run(sg, c, resident=True, fetch=False)
    assert l1 == l2 and l3 == [None]
    for a, p in ((a2, p2), (a3, p3)):
        assert np.array_equal(bits(p1.get_flat_params()), bits(p.get_flat_params()))
        assert np.array_equal(bits(a1.get_rmsprop()[0]), bits(a.get_rmsprop()[0]))
    assert a3.get_rmsprop()[1] == 1


# ------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_updates_match_the_reference_fixture(sg, name):
    from simgan_amd.utils import update_linear_schedule
    g = load(name)
    m = g["meta"]
    p = _policy(sg, m["C"], m["Hs"], m["dist"], m["P"], g["params0"])
    agent = _agent(sg, p, **{k: m[k] for k in HP})
    n = p.num_params
    for j, (pre, rows, lr) in enumerate(ref.fixture_updates(g)):
        update_linear_schedule(agent.optimizer, j, m["num_updates"], m["lr"])
        assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(lr)
        hxs = np.zeros((m["T"] + 1, m["N"], m["Hs"]), np.float32)
        hxs[0] = g[pre + "hxs0"]
        ro = _rollout(sg, m["C"], m["Hs"], m["dist"], m["P"], m["T"], m["N"], obs=g[pre + "obs"].astype(np.float32), actions=g[pre + "actions"],
                      returns=g[pre + "returns"], masks=g[pre + "masks"], recurrent_hidden_states=hxs)
        losses = agent.update(ro)
        idx = ref.sample_index(n, j)
        sq, step = agent.get_rmsprop()
        assert step == j + 1
        assert_close(losses, g[pre + "losses"], what=f"losses {j}")
        assert_close(sq[idx], g[pre + "square_avg"], rtol=1e-3, atol=1e-12, what=f"square_avg {j}")
        assert_close(p.get_flat_params()[idx], g[pre + "params1"], what=f"params after update {j}")


# ------------------------------------------------------------------------------------------- refusals
def test_refusals(sg):
    from simgan_amd import _lib
    from test_gpu_world import run_ranks
    E = _lib.SimganHipError
    cfg = _lib.A2CConfig(0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5)
    kw = dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    h = _lib.H()
    mlp = sg.Policy((11,), Box((3,)), base_kwargs={"recurrent": False, "hidden_size": 16})
    gru = sg.Policy((11,), Box((3,)), base_kwargs={"recurrent": True, "hidden_size": 16})
    cnn = sg.Policy((1, HW, HW), Box((3,)), base_kwargs={"hidden_size": 16})
    for other, hint in ((mlp, "has neither a CNN nor a GRU \\(sg_a2c_create\\)"), (gru, "has the GRU base on vector observations \\(sg_a2c_create_rnn\\)"),
                        (cnn, "has the feed-forward CNN base \\(sg_a2c_create_cnn\\)")):
        with pytest.raises(E, match="sg_a2c_create_cnn_rnn: A2C through time on image observations takes a policy with the recurrent CNN base.*" + hint):
            _lib.check(other.lib.sg_a2c_create_cnn_rnn(other.ctx.h, other.h, C.byref(cfg), C.byref(h)))
        with pytest.raises(ValueError, match="A2C_ACKTR\\(recurrent_cnn=True\\) takes a Policy with the recurrent CNN base"):
            sg.algo.A2C_ACKTR(other, 0.5, 0.01, recurrent_cnn=True, **kw)
    p = _policy(sg, 1, 16, "gaussian", 3)
    # the old calls keep their old texts
    for name in ("sg_a2c_create", "sg_a2c_create_rnn", "sg_a2c_create_cnn"):
        with pytest.raises(E, match=f"{name}: .*not implemented for the recurrent CNN base"):
            _lib.check(getattr(p.lib, name)(p.ctx.h, p.h, C.byref(cfg), C.byref(h)))
    with pytest.raises(E, match="sg_a2c_create_cnn: .*its row chunks carry no hidden state"):
        _lib.check(p.lib.sg_a2c_create_cnn(p.ctx.h, p.h, C.byref(cfg), C.byref(h)))
    with pytest.raises(E, match="sg_acktr_create: ACKTR is not implemented for the recurrent CNN base"):
        _lib.check(p.lib.sg_acktr_create(p.ctx.h, p.h, C.byref(_lib.ACKTRConfig(0.5, 0.01, 0.25, 0.9, 0.99, 0.001, 1e-2, 10)), C.byref(h)))
    for more in (dict(acktr=True), kw, dict(kw, cnn=True), dict(kw, recurrent=True)):
        with pytest.raises(NotImplementedError, match="A2C_ACKTR: not implemented for the recurrent CNN base"):
            sg.algo.A2C_ACKTR(p, 0.5, 0.01, **more)
    with pytest.raises(NotImplementedError, match="A2C_ACKTR\\(acktr=True, recurrent_cnn=True\\): ACKTR is not implemented"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=True, recurrent_cnn=True)
    with pytest.raises(E, match="sg_a2c_create_cnn_rnn: alpha must lie in \\[0, 1\\]"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, recurrent_cnn=True, lr=7e-4, eps=1e-5, alpha=1.5, max_grad_norm=0.5)
    agent = _agent(sg, p)
    with pytest.raises(NotImplementedError, match="A2C_ACKTR.diagnostics"):
        agent.diagnostics(None)
    n = p.num_params
    mm, vv, step = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int64(0)
    with pytest.raises(E, match="RMSprop"):
        _lib.check(agent.lib.sg_ppo_get_adam(agent.h, _lib.fptr(mm), _lib.fptr(vv), n, C.byref(step)))
    vec = sg.RolloutStorage(2, 2, (5,), Box((3,)), 1, 1)
    with pytest.raises(E, match="rollout dims \\(obs 5, act 3\\) do not match the policy \\(7056, 3\\)"):
        _lib.check(agent.lib.sg_ppo_update(agent.h, vec.h, None, 0, 0, (C.c_float * 3)()))
    ro = sg.RolloutStorage(2, 2, (1, HW, HW), Box((3,)), 16, 1)
    perms = np.arange(2, dtype=np.int64)
    with pytest.raises(E, match="perms must be NULL"):
        _lib.check(agent.lib.sg_ppo_update(agent.h, ro.h, perms.ctypes.data_as(C.POINTER(C.c_int64)), 2, 0, (C.c_float * 3)()))
    # a missing hand-over of slot 0's hidden states: refused with the existing text; a second update needs a second hand-over
    with pytest.raises(E, match="sg_ppo_set_hidden_states must hand over 32 floats before every update \\(pending: 0\\)"):
        _lib.check(agent.lib.sg_ppo_update(agent.h, ro.h, None, 0, 0, (C.c_float * 3)()))
    agent.update(ro)
    with pytest.raises(E, match="sg_ppo_set_hidden_states must hand over"):
        _lib.check(agent.lib.sg_ppo_update(agent.h, ro.h, None, 0, 0, (C.c_float * 3)()))
    with pytest.raises(NotImplementedError, match="enable_device_hidden: the rollout holds image observations"):
        ro.enable_device_hidden()
    ro.sync_to_device()
    with pytest.raises(E, match="sg_rollout_enable_hidden: this is an image rollout"):
        _lib.check(agent.lib.sg_rollout_enable_hidden(ro.h, 16))
    # T > 4096: one environment's steps do not fit a group (a vector-sized stand-in would not reach the check: the dims come first)
    long_ro = sg.RolloutStorage(4097, 1, (1, HW, HW), Box((3,)), 16, 1)
    hx = np.zeros((1, 16), np.float32)
    _lib.check(agent.lib.sg_ppo_set_hidden_states(agent.h, _lib.fptr(hx), hx.size))
    with pytest.raises(E, match="the 4097 steps of one exceed the 4096 rows a group may hold"):
        _lib.check(agent.lib.sg_ppo_update(agent.h, long_ro.h, None, 0, 0, (C.c_float * 3)()))

    def body(rank, ctx):
        q = sg.Policy((1, HW, HW), Box((2,)), base_kwargs={"recurrent": True, "hidden_size": 16}, recurrent_cnn=True, ctx=ctx)
        out = []
        try:
            sg.algo.A2C_ACKTR(q, 0.5, 0.01, recurrent_cnn=True, **kw)
        except NotImplementedError as exc:
            out.append(str(exc))
        try:
            _lib.check(q.lib.sg_a2c_create_cnn_rnn(ctx.h, q.h, C.byref(cfg), C.byref(_lib.H())))
        except E as exc:
            out.append(str(exc))
        return out

    for errs in run_ranks(2, body):
        assert len(errs) == 2 and "runs on one rank (this context's world is 2)" in errs[0], errs
        assert "sg_a2c_create_cnn_rnn" in errs[1] and "world 2" in errs[1], errs
