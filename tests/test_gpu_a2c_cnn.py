"""GPU: A2C on the CNN base -- A2C_ACKTR(..., cnn=True) / sg_a2c_create_cnn: the forward of csrc/sg_cnn.hip per row chunk,
k_cnn_head_loss_a2c, the accumulate forms of k_cnn_head_wgrad and k_cnn_reduce, k_sumsq and one k_a2c_rmsprop -- against float64
autograd per parameter block (tests/a2c_cnn_ref.py on tests/cnn_ref.py's cases, which keep clear of the ReLU kinks:
tests/test_a2c_cnn_host.py), the float64 RMSprop recurrence and the reference-written fixtures (tools/gen_golden_a2c_cnn.py).

The one-step gradient is recovered from the optimizer: a first RMSprop step from square_avg = 0 leaves square_avg =
(1 - alpha) g^2, so g = sign(p0 - p1) sqrt(square_avg / (1 - alpha)); the clip is put out of reach for those runs and eps =
1e-12, so every non-zero g moves its parameter by about 10 lr and the sign is never lost.
SG_A2C_CNN_RECORD=<path> collects the measured per-block distances (profiles/a2c_cnn_parity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import a2c_cnn_ref as ref
import cnn_ref as cr
from helpers import RTOL, assert_close, load

pytestmark = pytest.mark.gpu

HW = 84
HP = dict(value_loss_coef=ref.VCOEF, entropy_coef=ref.ECOEF, lr=ref.LR, eps=ref.EPS, alpha=ref.ALPHA, max_grad_norm=ref.MAX_GRAD_NORM)


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


def _policy(sg, C_, Hs, dist, P, params=None):
    p = sg.Policy((C_, HW, HW), space(dist, P), base_kwargs={"hidden_size": Hs})
    assert [(n, tuple(s)) for n, s in p.param_shapes()] == cr.param_shapes(C_, Hs, dist, P) and p.cnn == C_
    if params is not None:
        p.set_flat_params(np.asarray(params, np.float32))
    return p


def _agent(sg, p, **over):
    m = dict(HP, **over)
    return sg.algo.A2C_ACKTR(p, m["value_loss_coef"], m["entropy_coef"], lr=m["lr"], eps=m["eps"], alpha=m["alpha"],
                             max_grad_norm=m["max_grad_norm"], cnn=True)


def _rollout(sg, C_, dist, P, T, N, obs, actions, returns, resident=False):
    ro = sg.RolloutStorage(T, N, (C_, HW, HW), space(dist, P), 1, 1)
    for name, arr in (("obs", obs), ("actions", actions), ("returns", returns)):
        t = getattr(ro, name)
        t.copy_(t.new_tensor(np.asarray(arr).reshape(tuple(t.shape))))
    if resident:
        ro.sync_to_device()
        ro.device_resident = True
    return ro


def _run(sg, c, updates=1, resident=False, fetch=True, **over):
    """-> (agent, policy, [losses per update]) after `updates` updates on the case's rollout"""
    p = _policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = _agent(sg, p, **over)
    ro = _rollout(sg, c.C, c.dist, c.P, c.T, c.N, c.obs, c.actions, c.returns, resident)
    return agent, p, [agent.update(ro, fetch_losses=fetch) for _ in range(updates)]


def _record(label, rec):
    path = os.environ.get("SG_A2C_CNN_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_a2c_cnn.py under SG_A2C_CNN_RECORD: one-step gradients per parameter block as the rel-L2 distance "
                       "of tests/cnn_ref.py:block_distances to float64 autograd, over RTOL = 1e-4; the losses' largest error over "
                       "ATOL + RTOL |ref|", "cases": {}}
    doc["cases"][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def _hold_gradient(sg, key, label):
    return hold_case(sg, ref.case(key), label)


def hold_case(sg, c, label, want=None, record=None, **over):
    """the recovered one-step gradient of a case against float64 autograd (`want`: its gradient and losses, where the caller has
    them already) per block, the losses with assert_close -> the recovered gradient.  tests/test_gpu_cnn_regimes.py's cases come
    through here too, with their own record."""
    want, want_losses = ref.case_grad(c, **({"ecoef": over["entropy_coef"]} if "entropy_coef" in over else {})) if want is None else want
    agent, p, losses = _run(sg, c, max_grad_norm=ref.NO_CLIP, eps=ref.EPS_RECOVER, **over)
    sq, step = agent.get_rmsprop()
    assert step == 1
    got = ref.recovered_gradient(c.params, p.get_flat_params(), sq)
    d = cr.block_distances(got, want, c.shapes)
    lr_ = float(np.max(np.abs(np.asarray(losses[0]) - want_losses) / (cr.ATOL + RTOL * np.abs(want_losses))))
    print(f"{label}: worst block {max(d, key=d.get)} {max(d.values()) / RTOL:.3f} x RTOL, losses {lr_:.3f} of tol")
    (record or _record)(label, {"worst": max(d.values()) / RTOL, "blocks": {k: x / RTOL for k, x in d.items()}, "losses": lr_})
    assert_close(losses[0], want_losses, what=f"{label} losses")
    bad = {k: x for k, x in d.items() if not x <= RTOL}
    assert not bad, f"{label}: blocks past {RTOL:g}: {bad}"
    return got


# ------------------------------------------------------------------------------------------- gradient per block vs float64
@pytest.mark.parametrize("key", ref.CASES, ids=ref.tag)
def test_one_step_gradient_per_block(sg, key):
    _hold_gradient(sg, key, "gradient " + ref.tag(key))


def test_the_clip_acts(sg):
    """max_grad_norm = 0.5 on the Gaussian case: the step is lr g factor / (sqrt(sq) + eps) with float64's g and factor < 1"""
    c = ref.case(ref.GAUSSIAN_CASE)
    obs, actions, returns = ref.rows_of(c)
    r = ref.update64(c.shapes, c.dist, c.params, None, obs, actions, returns)
    assert r["factor"] < 1.0
    agent, p, losses = _run(sg, c)
    sq, _ = agent.get_rmsprop()
    step64 = c.params.astype(np.float64) - r["params"]
    # (the step read back from p0 - p1 in float64: elements with |g| << eps / 0.1 barely move, so an absolute floor at their rounding)
    assert np.allclose(step64, ref.LR * r["grad"] * r["factor"] / (np.sqrt(r["square_avg"]) + ref.EPS), rtol=1e-9, atol=1e-15)
    d = cr.block_distances(c.params.astype(np.float64) - p.get_flat_params(), step64, c.shapes)
    _record("step with the clip acting " + ref.tag(ref.GAUSSIAN_CASE), {"clip_factor": r["factor"], "worst": max(d.values()) / RTOL})
    assert max(d.values()) <= RTOL, d
    assert_close(sq, r["square_avg"], rtol=1e-3, atol=1e-12, what="square_avg = (1 - alpha) (g factor)^2")
    assert_close(losses[0], r["losses"], what="losses")
    # the unclipped square_avg is 1 / factor^2 of it: a norm over part of the parameters, or no clip, would show
    assert r["factor"] ** 2 < 0.9


# ------------------------------------------------------------------------------------------- chunks
@pytest.mark.parametrize("key,chunk", ref.CHUNKED, ids=lambda v: ref.tag(v) if isinstance(v, tuple) else str(v))
def test_gradient_in_row_chunks(sg, monkeypatch, key, chunk):
    """the same float64 gradient of the UNCHUNKED loss, the rows taken `chunk` at a time: every pass after the first adds to the
    flat gradient, and 1 / B stays 1 / (T N)"""
    assert key[4] * key[5] > chunk
    monkeypatch.setenv("SG_A2C_CNN_CHUNK_ROWS", str(chunk))
    chunked = _hold_gradient(sg, key, "gradient " + ref.tag(key, chunk))
    monkeypatch.delenv("SG_A2C_CNN_CHUNK_ROWS")
    c = ref.case(key)
    agent, p, _ = _run(sg, c, max_grad_norm=ref.NO_CLIP, eps=ref.EPS_RECOVER)
    whole = ref.recovered_gradient(c.params, p.get_flat_params(), agent.get_rmsprop()[0])
    assert max(cr.block_distances(chunked, whole, c.shapes).values()) <= RTOL


# ------------------------------------------------------------------------------------------- determinism
def test_same_bits_twice_and_against_direct_launches(sg, monkeypatch):
    monkeypatch.setenv("SG_A2C_CNN_CHUNK_ROWS", "4")      # three accumulating passes inside the graph
    c = ref.case(ref.GAUSSIAN_CASE)
    out = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        agent, p, losses = _run(sg, c, updates=2)      # (the second update of a graph run is a replay)
        out.append((losses, p.get_flat_params(), agent.get_rmsprop()[0]))
    for other in out[1:]:
        assert out[0][0] == other[0]
        assert np.array_equal(out[0][1].view(np.uint32), other[1].view(np.uint32))
        assert np.array_equal(out[0][2].view(np.uint32), other[2].view(np.uint32))
    assert np.isfinite(out[0][1]).all() and np.abs(out[0][1] - c.params).max() > 1e-4


def test_second_update_follows_the_float64_recurrence(sg):
    """two updates on one agent: the second replays the graph with square_avg != 0"""
    c = ref.case((1, 16, "categorical", 5, 4, 4))
    obs, actions, returns = ref.rows_of(c)
    agent, p, losses = _run(sg, c, updates=2)
    params, sq = c.params, None
    for j in range(2):
        r = ref.update64(c.shapes, c.dist, params, sq, obs, actions, returns)
        assert_close(losses[j], r["losses"], what=f"losses {j}")
        params, sq = r["params"], r["square_avg"]
    got_sq, step = agent.get_rmsprop()
    assert step == 2
    assert_close(got_sq, sq, rtol=1e-3, atol=1e-12, what="square_avg after two updates")
    assert_close(p.get_flat_params(), params, what="params after two updates")


# ------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_updates_match_the_reference_fixture(sg, name):
    from simgan_amd.utils import update_linear_schedule
    g = load(name)
    m = g["meta"]
    p = _policy(sg, m["C"], m["Hs"], m["dist"], m["P"], g["params0"])
    agent = _agent(sg, p, **{k: m[k] for k in HP})
    n = p.num_params
    for j, (pre, _, _, _, lr) in enumerate(ref.fixture_updates(g)):
        update_linear_schedule(agent.optimizer, j, m["num_updates"], m["lr"])
        assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(lr)
        ro = _rollout(sg, m["C"], m["dist"], m["P"], m["T"], m["N"], g[pre + "obs"].astype(np.float32), g[pre + "actions"], g[pre + "returns"])
        losses = agent.update(ro)
        idx = ref.sample_index(n, j)
        sq, step = agent.get_rmsprop()
        assert step == j + 1
        assert_close(losses, g[pre + "losses"], what=f"losses {j}")
        assert_close(sq[idx], g[pre + "square_avg"], rtol=1e-3, atol=1e-12, what=f"square_avg {j}")
        assert_close(p.get_flat_params()[idx], g[pre + "params1"], what=f"params after update {j}")
    assert agent.optimizer.param_groups[0]["lr"] == pytest.approx(m["lr"] * (1 - (m["iters"] - 1) / m["num_updates"]))


# ------------------------------------------------------------------------------------------- rollouts, the interface
def test_host_resident_and_queued_updates_give_the_same_bits(sg):
    c = ref.case((1, 16, "categorical", 5, 4, 4))
    a1, p1, l1 = _run(sg, c)
    a2, p2, l2 = _run(sg, c, resident=True)
    a3, p3, l3 = _run(sg, c, resident=True, fetch=False)
    assert l1 == l2 and l3 == [None]
    for a, p in ((a2, p2), (a3, p3)):
        assert np.array_equal(p1.get_flat_params().view(np.uint32), p.get_flat_params().view(np.uint32))
        assert np.array_equal(a1.get_rmsprop()[0].view(np.uint32), a.get_rmsprop()[0].view(np.uint32))
    assert a3.get_rmsprop()[1] == 1


def test_int64_actions_of_a_discrete_rollout_are_taken(sg):
    c = ref.case((1, 16, "categorical", 5, 1, 3))
    ro = sg.RolloutStorage(c.T, c.N, (c.C, HW, HW), Discrete(c.P), 1, 1)
    assert str(ro.actions.dtype).endswith("int64") and c.actions.dtype == np.int64
    ro.obs.copy_(ro.obs.new_tensor(c.obs))
    ro.actions.copy_(ro.actions.new_tensor(c.actions))
    ro.returns.copy_(ro.returns.new_tensor(c.returns))
    p = _policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    losses = _agent(sg, p).update(ro)
    assert_close(losses, ref.case_grad(c)[1], what="losses")
    # another class in one row is another action loss
    other = c.actions.copy()
    other[0, 0, 0] = (other[0, 0, 0] + 1) % c.P
    ro.actions.copy_(ro.actions.new_tensor(other))
    q = _policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    assert abs(_agent(sg, q).update(ro)[1] - losses[1]) > 1e-3


def test_rmsprop_state_round_trip_and_the_lr(sg):
    c = ref.case((1, 16, "categorical", 5, 1, 1))
    agent, p, _ = _run(sg, c)
    n = p.num_params
    state = np.arange(1, n + 1, dtype=np.float32) * 1e-6
    agent.set_rmsprop(state, 7)
    back, step = agent.get_rmsprop()
    assert step == 7 and np.array_equal(back, state)
    from simgan_amd import _lib
    with pytest.raises(_lib.SimganHipError, match="sg_a2c_set_rmsprop: bad length"):
        agent.set_rmsprop(state[1:], 7)
    # lr = 0 through the param group reaches the device: the next update moves nothing
    agent.optimizer.param_groups[0]["lr"] = 0.0
    before = p.get_flat_params()
    agent.update(_rollout(sg, c.C, c.dist, c.P, c.T, c.N, c.obs, c.actions, c.returns))
    assert np.array_equal(before, p.get_flat_params()) and agent.get_rmsprop()[1] == 8


# ------------------------------------------------------------------------------------------- refusals
def test_refusals(sg):
    from simgan_amd import _lib
    from test_gpu_world import run_ranks
    E = _lib.SimganHipError
    cfg = _lib.A2CConfig(0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5)
    kw = dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    h = _lib.H()
    mlp = sg.Policy((11,), Box((3,)), base_kwargs={"recurrent": False, "hidden_size": 16})
    with pytest.raises(E, match="sg_a2c_create_cnn: A2C on image observations takes a policy with the CNN base"):
        _lib.check(mlp.lib.sg_a2c_create_cnn(mlp.ctx.h, mlp.h, C.byref(cfg), C.byref(h)))
    with pytest.raises(ValueError, match="A2C_ACKTR\\(cnn=True\\) takes a Policy with the CNN base"):
        sg.algo.A2C_ACKTR(mlp, 0.5, 0.01, cnn=True, **kw)
    p = _policy(sg, 1, 16, "gaussian", 3)
    # the old calls keep their old texts
    with pytest.raises(E, match="sg_a2c_create: A2C is not implemented for the CNN base \\(image observations\\): PPO is"):
        _lib.check(p.lib.sg_a2c_create(p.ctx.h, p.h, C.byref(cfg), C.byref(h)))
    with pytest.raises(E, match="sg_acktr_create: ACKTR is not implemented for the CNN base"):
        _lib.check(p.lib.sg_acktr_create(p.ctx.h, p.h, C.byref(_lib.ACKTRConfig(0.5, 0.01, 0.25, 0.9, 0.99, 0.001, 1e-2, 10)), C.byref(h)))
    for acktr in (False, True):
        with pytest.raises(NotImplementedError, match="A2C_ACKTR: not implemented for the CNN base \\(image observations\\), in either mode; PPO is"):
            sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=acktr, **({} if acktr else kw))
    with pytest.raises(NotImplementedError, match="K-FAC has no convolution statistics here"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=True, cnn=True)
    with pytest.raises(E, match="alpha must lie in \\[0, 1\\]"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, cnn=True, lr=7e-4, eps=1e-5, alpha=1.5, max_grad_norm=0.5)
    agent = _agent(sg, p)
    with pytest.raises(NotImplementedError, match="A2C_ACKTR.diagnostics: the diagnostics kernels do not cover the CNN base"):
        agent.diagnostics(None)
    n = p.num_params
    mm, vv, step = np.empty(n, np.float32), np.empty(n, np.float32), C.c_int64(0)
    with pytest.raises(E, match="RMSprop"):
        _lib.check(agent.lib.sg_ppo_get_adam(agent.h, _lib.fptr(mm), _lib.fptr(vv), n, C.byref(step)))
    with pytest.raises(E, match="rollout dims \\(obs 5, act 3\\) do not match the policy \\(7056, 3\\)"):
        agent.update(sg.RolloutStorage(2, 2, (5,), Box((3,)), 1, 1))
    perms = np.arange(4, dtype=np.int64)
    ro = sg.RolloutStorage(2, 2, (1, HW, HW), Box((3,)), 1, 1)
    with pytest.raises(E, match="perms must be NULL"):
        _lib.check(agent.lib.sg_ppo_update(agent.h, ro.h, perms.ctypes.data_as(C.POINTER(C.c_int64)), 4, 0, (C.c_float * 3)()))

    def body(rank, ctx):
        q = sg.Policy((1, HW, HW), Box((2,)), base_kwargs={"hidden_size": 16}, ctx=ctx)
        out = []
        try:
            sg.algo.A2C_ACKTR(q, 0.5, 0.01, cnn=True, **kw)
        except NotImplementedError as exc:
            out.append(str(exc))
        try:
            _lib.check(q.lib.sg_a2c_create_cnn(ctx.h, q.h, C.byref(cfg), C.byref(_lib.H())))
        except E as exc:
            out.append(str(exc))
        return out

    for errs in run_ranks(2, body):
        assert len(errs) == 2 and "runs on one rank (this context's world is 2)" in errs[0], errs
        assert "sg_a2c_create_cnn" in errs[1] and "world 2" in errs[1], errs
