"""GPU: the recurrent CNN base -- Policy((C, 84, 84), space, base_kwargs={'recurrent': True}, recurrent_cnn=True): CNN trunk, GRU,
heads on the GRU state (csrc/sg_cnn.hip, sg_gru_kernels.hpp: k_gru_dx, sg_ppo.hip: cnn_gru_ppo_update) through act, get_value,
evaluate_actions, RolloutStorage, PPO.update and PpoLearner, against tests/cnn_gru_ref.py in float64.

  1 forward     the three policy calls against the float64 forward; evaluate_actions over T n rows against T chained one-step
                calls, bit for bit
  2 gradient    Adam's first moment after one update at lr = 0, per parameter block against float64 autograd within RTOL: clipped
                and plain value loss, the clip out of reach and at max_grad_norm = 0.5; LDS-weight and global-weight instances
  3 update      whole updates (E = 2, M = 2) against torch.optim.Adam's arithmetic in float64; the library's own permutations
                against tests/rng_ref.py
  4 same bits   two runs, graph replay against SG_PPO_GRAPH=0, device-resident against host rollout; a feed-forward CNN policy
                before and after a recurrent one ran
  5 refusals    the C ABI's, each by its own message
  6 learner     PpoLearner on a host rollout against the hand-written sequence, bit for bit
SG_CNN_GRU_RECORD=<path> collects the measured worst block per gradient case (profiles/cnn_gru_parity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import cnn_gru_ref as gr
import cnn_ref as cr
import rng_ref
from helpers import ATOL, GOLDEN, RTOL, assert_close, assert_close_adam, load

pytestmark = pytest.mark.gpu

LR, EPS = cr.LR, cr.EPS
HW = 84


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


class MultiBinary(object):
    def __init__(self, n):
        self.n, self.shape = int(n), (int(n),)


def space(dist, P):
    return Discrete(P) if dist == "categorical" else Box((P,))


def npv(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def bits(a):
    return np.ascontiguousarray(npv(a), np.float32).view(np.uint32)


def make_policy(sg, C_, Hs, dist, P, params=None):
    p = sg.Policy((C_, HW, HW), space(dist, P), base_kwargs={"recurrent": True, "hidden_size": Hs}, recurrent_cnn=True)
    assert [(n, tuple(s)) for n, s in p.param_shapes()] == gr.param_shapes(C_, Hs, dist, P)
    assert p.is_recurrent and p.recurrent_hidden_state_size == Hs and p.cnn == C_
    if params is not None:
        p.set_flat_params(params)
        assert np.array_equal(p.get_flat_params(), params)
    return p


def fill(ro, **fields):
    for name, arr in fields.items():
        t = getattr(ro, name)
        t.copy_(t.new_tensor(np.asarray(arr).reshape(tuple(t.shape))))


def rollout_of(sg, c):
    ro = sg.RolloutStorage(c.T, c.N, (c.C, HW, HW), space(c.dist, c.P), c.Hs, 1)
    assert tuple(ro.obs.shape) == (c.T + 1, c.N, c.C, HW, HW) and tuple(ro.recurrent_hidden_states.shape) == (c.T + 1, c.N, c.Hs)
    fill(ro, obs=c.obs, actions=c.actions, action_log_probs=c.action_log_probs, value_preds=c.value_preds, returns=c.returns, masks=c.masks,
         recurrent_hidden_states=c.hxs)
    return ro


def _record(label, rec):
    path = os.environ.get("SG_CNN_GRU_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_cnn_gru.py under SG_CNN_GRU_RECORD: one-step gradients per parameter block as the rel-L2 distance of "
                       "tests/cnn_ref.py:block_distances over RTOL (the bound is 1)", "cases": {}}
    doc["cases"][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


# ------------------------------------------------------------------------------------------------- 1 forward
# (C, Hs, dist, P, T, n): one step; a short sequence; Hp = 32 with 12 padded units per gate; a second, ragged 16-environment scan
# workgroup; the default width (global-weight instances); 130 rows = a second 128-row trunk pass
FORWARD = [(1, 16, "categorical", 5, 1, 1), (1, 16, "categorical", 5, 5, 3), (2, 20, "gaussian", 3, 3, 2), (1, 16, "categorical", 5, 2, 17),
           (4, 512, "categorical", 6, 3, 2), (1, 16, "categorical", 5, 65, 2)]


def forward_inputs(C_, Hs, dist, P, T, n):
    rng = np.random.default_rng([C_, Hs, P, T, n, 5])
    params = gr.init_params(rng, C_, Hs, dist, P, noise=0.05)
    if dist == "categorical":
        params[-P * (Hs + 1):] *= 30.0      # logits that differ
    obs = rng.integers(0, 256, (T * n, C_, HW, HW)).astype(np.float32)
    hxs = (0.5 * rng.standard_normal((n, Hs))).astype(np.float32)
    masks = gr.default_masks(T, n)[:T].reshape(-1)
    acts = rng.integers(0, P, (T * n, 1)) if dist == "categorical" else rng.standard_normal((T * n, P)).astype(np.float32)
    return params, obs, hxs, masks, acts


@pytest.mark.parametrize("key", FORWARD, ids=["-".join(map(str, k)) for k in FORWARD])
def test_forward_matches_float64_and_chained_steps_give_the_same_bits(sg, key):
    C_, Hs, dist, P, T, n = key
    params, obs, hxs, masks, acts = forward_inputs(*key)
    shapes = gr.param_shapes(C_, Hs, dist, P)
    p = make_policy(sg, C_, Hs, dist, P, params)
    with torch.no_grad():
        rv, rlp, rent, rh = gr.evaluate(cr.leaves(params, shapes), cr.ar.t64(obs), hxs, masks, T, acts, dist)
    assert T * n == 1 or np.ptp(rv.numpy()) > 1e-4
    v, lp, ent, hT = p.evaluate_actions(obs, hxs, masks.reshape(-1, 1), acts)
    assert tuple(v.shape) == (T * n, 1) and tuple(lp.shape) == (T * n, 1) and tuple(hT.shape) == (n, Hs)
    assert_close(npv(v), rv.numpy(), what="value")
    assert_close(npv(lp), rlp.numpy(), what="logp")
    assert_close(npv(ent), rent.numpy(), what="entropy")
    assert_close(npv(hT), rh.numpy(), what="final hidden state")
    # T chained one-step calls: the same bits in values, log-probs and the final hidden state
    h, vs, lps = hxs, [], []
    for t in range(T):
        sl = slice(t * n, (t + 1) * n)
        v1, lp1, _, h = p.evaluate_actions(obs[sl], h, masks[sl].reshape(-1, 1), acts[sl])
        if t == 0:
            va, _, _, ha = p.act(obs[sl], hxs, masks[sl].reshape(-1, 1), deterministic=True)
            assert np.array_equal(bits(va), bits(v1)) and np.array_equal(bits(ha), bits(h))
            assert np.array_equal(bits(p.get_value(obs[sl], hxs, masks[sl].reshape(-1, 1))), bits(v1))
        vs.append(npv(v1))
        lps.append(npv(lp1))
    assert np.array_equal(bits(np.concatenate(vs)), bits(v)), "values: a sequence and its chained steps differ"
    assert np.array_equal(bits(np.concatenate(lps)), bits(lp)), "log-probs: a sequence and its chained steps differ"
    assert np.array_equal(bits(h), bits(hT)), "final hidden state: a sequence and its chained steps differ"
    # act on the first step: the mode, and an injected draw
    det = gr.act64(shapes, params, obs[:n], hxs, masks[:n], 1, dist)
    v, a, lp, h1 = p.act(obs[:n], hxs, masks[:n].reshape(-1, 1), deterministic=True)
    assert_close(npv(v), det["value"], what="value from act")
    assert_close(npv(h1), det["hxs"], what="hidden state from act")
    if dist == "categorical":
        if det["margin"] > 1e-3:
            assert np.array_equal(npv(a).reshape(-1), det["action"])
            assert_close(npv(lp), det["logp"], what="logp of the mode")
        u = np.random.default_rng(9).uniform(0, 1, n).astype(np.float32)
        smp = gr.act64(shapes, params, obs[:n], hxs, masks[:n], 1, dist, noise=u)
        v, a, lp, _ = p.act(obs[:n], hxs, masks[:n].reshape(-1, 1), noise=u.reshape(n, 1))
        if smp["margin"] > 1e-3:
            assert npv(a).dtype == np.int64 and np.array_equal(npv(a).reshape(-1), smp["action"])
            assert_close(npv(lp), smp["logp"], what="logp of the drawn class")
    else:
        assert_close(npv(a), det["action"], what="mode")
        assert_close(npv(lp), det["logp"], what="logp of the mode")
        z = np.random.default_rng(9).standard_normal((n, P)).astype(np.float32)
        smp = gr.act64(shapes, params, obs[:n], hxs, masks[:n], 1, dist, noise=z)
        v, a, lp, _ = p.act(obs[:n], hxs, masks[:n].reshape(-1, 1), noise=z)
        assert_close(npv(a), smp["action"], what="sampled action")
        assert_close(npv(lp), smp["logp"], what="its log-prob")


# ------------------------------------------------------------------------------------------------- 2 one-step gradient
def agent_for(sg, c, p, E, M, max_grad_norm=1e9, use_clipped=True, lr=LR, **kw):
    return sg.algo.PPO(p, cr.CLIP, E, M, cr.VCOEF, c.ecoef, lr=lr, eps=EPS, max_grad_norm=max_grad_norm, use_clipped_value_loss=use_clipped, **kw)


def reference_moment(c, key, M, perm, max_grad_norm, use_clipped):
    """one epoch at lr = 0: m = sum_k 0.9^(S-1-k) 0.1 clip_k g_k, each g_k autograd's on exactly step k's environments"""
    steps = gr.step_envs(key, M, perm)
    m, losses, factors = 0.0, np.zeros(3), []
    for k, envs in enumerate(steps):
        g, l3 = gr.case_grad(c, envs, use_clipped)
        f = cr.clip_factor(g, max_grad_norm)
        factors.append(f)
        m = m + 0.9 ** (len(steps) - 1 - k) * 0.1 * f * g
        losses += l3
    return m, losses / M, factors      # (a2c/algo/ppo.py:151-155 divides by ppo_epoch * num_mini_batch)


GRAD_RUNS = [(key, mgn, clipped, gw) for key in gr.GRAD_CASES for mgn, clipped in ((1e9, True), (0.5, True), (1e9, False), (0.5, False))
             for gw in ((False, True) if key[1] == 16 and key[2] == "categorical" else (False,))
             if not (gw and (mgn < 1 or not clipped))]


@pytest.mark.parametrize("key,max_grad_norm,use_clipped,gw", GRAD_RUNS,
                         ids=[f"{'-'.join(map(str, k))}-clip{m:g}-{'clipped' if u else 'plain'}{'-gw' if g else ''}" for k, m, u, g in GRAD_RUNS])
def test_one_step_gradient_per_block(sg, monkeypatch, key, max_grad_norm, use_clipped, gw):
    if gw:
        monkeypatch.setenv("SG_POLICY_GW", "1")      # the global-weight instances of the GRU kernels, k_gru_dx's included
    c, M = gr.case(*key), gr.GRAD_CASES[key]
    perm = np.random.default_rng(gr.PERM_SEED).permutation(c.N).astype(np.int64)
    ref, ref_losses, factors = reference_moment(c, key, M, perm, max_grad_norm, use_clipped)
    if max_grad_norm >= 1.0 or key in gr.CLIP_INACTIVE:
        assert all(f == 1.0 for f in factors)
    else:
        assert all(f < 1.0 for f in factors)      # the clip acts in every step of this run
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = agent_for(sg, c, p, 1, M, max_grad_norm, use_clipped, lr=0.0)
    losses = agent.update(rollout_of(sg, c), perms=perm[None])
    m, v, step = agent.get_adam()
    assert step == len(factors) and np.array_equal(agent.last_perms(), perm[None])
    assert np.array_equal(p.get_flat_params(), c.params)
    d = cr.block_distances(m, ref, c.shapes)
    _record(f"gradient {c.tag} M={M} max_grad_norm={max_grad_norm:g} {'clipped' if use_clipped else 'plain'}{' gw' if gw else ''}",
            {"worst": max(d.values()) / RTOL, "blocks": {k: x / RTOL for k, x in d.items()}})
    assert_close(losses, ref_losses, what="losses")
    bad = {k: x for k, x in d.items() if not x <= RTOL}
    assert not bad, f"{c.tag}: blocks past {RTOL:g}: {bad}"
    if c.head == "fc_zero" and len(factors) == 1:
        zeros = gr.admitted(key, use_clipped)[3]
        assert zeros.size >= gr.ZERO_UNITS * (1568 + 1 + 3 * c.Hs)      # the FC rows, their biases, the matching weight_ih columns
        assert not m[zeros].any(), "the gradient is not exactly 0 where torch's is in both precisions"


# ------------------------------------------------------------------------------------------------- 3 whole updates
def adam_update64(c, key, perms, E, M, max_grad_norm):
    """PPO.update over the recurrent generator's minibatches in float64 with torch.optim.Adam's arithmetic"""
    params = c.params.astype(np.float64).copy()
    m, v, t, acc = np.zeros_like(params), np.zeros_like(params), 0, np.zeros(3)
    cc = cr.Case(c)
    for e in range(E):
        for envs in gr.step_envs(key, M, perms[e]):
            cc["params"] = params
            g, l3 = gr.case_grad(cc, envs)
            g = g * cr.clip_factor(g, max_grad_norm)
            t += 1
            m = 0.9 * m + 0.1 * g
            v = 0.999 * v + 0.001 * g * g
            params = params - (LR / (1 - 0.9 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + EPS)
            acc += l3
    return acc / (E * M), params, t


UPDATE_KEYS = [(1, 16, "categorical", 5, 4, 4), (2, 20, "gaussian", 3, 3, 3)]


@pytest.mark.parametrize("key", UPDATE_KEYS, ids=["-".join(map(str, k)) for k in UPDATE_KEYS])
def test_whole_update_matches_float64_adam(sg, key):
    c, E, M = gr.case(*key), 2, 2
    perms = np.stack([np.random.default_rng([gr.PERM_SEED, e]).permutation(c.N) for e in range(E)]).astype(np.int64)
    ref_losses, ref_params, steps = adam_update64(c, key, perms, E, M, 0.5)
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = agent_for(sg, c, p, E, M, 0.5)
    losses = agent.update(rollout_of(sg, c), perms=perms)
    assert agent.get_adam()[2] == steps and np.array_equal(agent.last_perms(), perms)
    assert_close(losses, ref_losses, what="losses")
    assert_close_adam(p.get_flat_params(), ref_params, LR, steps, what="params after the update")


def test_the_library_draws_the_recurrent_streams_permutations(sg):
    key = UPDATE_KEYS[0]
    c, E, M = gr.case(*key), 2, 2
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = agent_for(sg, c, p, E, M, 0.5, seed=9)
    agent.update(rollout_of(sg, c))
    got = agent.last_perms()
    assert got.shape == (E, c.N)
    want = rng_ref.ppo_perms(agent.seed, 1, E, c.N)
    assert np.array_equal(got, np.asarray(want).reshape(E, c.N))


# ------------------------------------------------------------------------------------------------- 4 the same bits
def test_two_runs_graph_replay_and_resident_rollouts_give_the_same_bits(sg, monkeypatch):
    key = UPDATE_KEYS[0]
    c, E, M = gr.case(*key), 2, 2
    perms = np.stack([np.random.default_rng([gr.PERM_SEED, e]).permutation(c.N) for e in range(E)]).astype(np.int64)
    out = []
    for graph, resident in (("1", False), ("1", False), ("0", False), ("1", True)):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
        agent = agent_for(sg, c, p, E, M, 0.5)
        ro = rollout_of(sg, c)
        if resident:
            ro.device_resident = True
            ro.sync_to_device()
        losses = [agent.update(ro, perms=perms) for _ in range(2)]      # (the second update of a graph run is a replay)
        out.append((losses, p.get_flat_params(), *agent.get_adam()[:2]))
    for other in out[1:]:
        assert other[0] == out[0][0]
        for a, b in zip(out[0][1:], other[1:]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(out[0][1]).all() and np.abs(out[0][1] - c.params).max() > 1e-4
    # padding stays zero: the flat vectors round-trip, and a second policy loaded with the updated parameters acts the same
    q = make_policy(sg, c.C, c.Hs, c.dist, c.P, out[0][1])
    r = gr.rows_of(c)
    a = p.evaluate_actions(r["obs"], r["hxs0"], r["masks"].reshape(-1, 1), r["actions"])
    b = q.evaluate_actions(r["obs"], r["hxs0"], r["masks"].reshape(-1, 1), r["actions"])
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def test_a_feed_forward_cnn_policy_is_untouched_by_a_recurrent_one(sg):
    c = cr.case(*cr.GATHER_CASE)

    def run():
        p = sg.Policy((c.C, HW, HW), space(c.dist, c.P), base_kwargs={"hidden_size": c.Hs})
        p.set_flat_params(c.params)
        ro = sg.RolloutStorage(c.T, c.N, (c.C, HW, HW), space(c.dist, c.P), 1, 1)
        fill(ro, **{k: c[k] for k in ("obs", "actions", "action_log_probs", "value_preds", "returns")})
        act = p.act(c.obs[0], None, None, deterministic=True)[:3]
        agent = sg.algo.PPO(p, cr.CLIP, 1, 2, cr.VCOEF, cr.ECOEF, lr=LR, eps=EPS, max_grad_norm=0.5)
        perm = np.random.default_rng(1).permutation(c.T * c.N).astype(np.int64)[None]
        losses = agent.update(ro, perms=perm)
        return [npv(x).astype(np.float32) for x in act] + [np.asarray(losses, np.float32), p.get_flat_params(), *agent.get_adam()[:2]]
    before = run()
    key = UPDATE_KEYS[0]
    g = gr.case(*key)
    rp = make_policy(sg, g.C, g.Hs, g.dist, g.P, g.params)
    agent_for(sg, g, rp, 1, 2, 0.5).update(rollout_of(sg, g))
    after = run()
    for a, b in zip(before, after):
        assert np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------- 5 refusals
def test_c_abi_refusals(sg):
    from simgan_amd import _lib
    c = gr.case(*UPDATE_KEYS[0])
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    lib, ctx, h = p.lib, p.ctx, _lib.H()
    E = _lib.SimganHipError
    with pytest.raises(E, match="sg_policy_create_cnn_rnn: the CNN base is built with the Gaussian \\(Box\\) and Categorical \\(Discrete\\) heads; dist 2"):
        _lib.check(lib.sg_policy_create_cnn_rnn(ctx.h, 1, 84, 84, 16, 2, 5, 5, C.byref(h)))
    with pytest.raises(E, match="sg_policy_create_cnn_rnn: hidden 4096: the GRU's 16-row tiles .* do not fit"):
        _lib.check(lib.sg_policy_create_cnn_rnn(ctx.h, 1, 84, 84, 4096, 1, 1, 5, C.byref(h)))
    a2c = _lib.A2CConfig(0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5)
    for name in ("sg_a2c_create", "sg_a2c_create_rnn", "sg_a2c_create_cnn"):
        with pytest.raises(E, match=f"{name}: .*not implemented for the recurrent CNN base"):
            _lib.check(getattr(lib, name)(ctx.h, p.h, C.byref(a2c), C.byref(h)))
    with pytest.raises(E, match="sg_acktr_create: ACKTR is not implemented for the recurrent CNN base"):
        _lib.check(lib.sg_acktr_create(ctx.h, p.h, C.byref(_lib.ACKTRConfig(0.5, 0.01, 0.25, 0.9, 0.99, 0.001, 0.01, 1)), C.byref(h)))
    with pytest.raises(E, match="this policy is recurrent"):
        v = np.zeros(1, np.float32)
        _lib.check(lib.sg_policy_get_value(p.h, _lib.fptr(c.obs[0, :1].reshape(-1).copy()), 1, _lib.fptr(v)))
    ro = rollout_of(sg, c)
    ro.device_resident = True
    ro.sync_to_device()
    with pytest.raises(E, match="sg_rollout_enable_hidden: this is an image rollout"):
        _lib.check(lib.sg_rollout_enable_hidden(ro.h, c.Hs))
    with pytest.raises(E, match="sg_rollout_compute_returns_policy: the policy has the recurrent CNN base"):
        _lib.check(lib.sg_rollout_compute_returns_policy(ro.h, p.h, 1, 0.99, 0.95, 0))
    act = np.zeros((c.N, 1), np.float32)
    with pytest.raises(E, match="sg_rollout_act_step: the policy has the recurrent CNN base"):
        _lib.check(lib.sg_rollout_act_step(ro.h, p.h, 0, None, None, 0, 1, _lib.fptr(act)))
    with pytest.raises(E, match="sg_rollout_act_step_rnn: the policy has the recurrent CNN base"):
        _lib.check(lib.sg_rollout_act_step_rnn(ro.h, p.h, 0, None, None, None, 0, 1, _lib.fptr(act)))
    agent = agent_for(sg, c, p, 1, 1)
    with pytest.raises(E, match="sg_ppo_set_symmetry: the mirror-symmetry loss is not implemented for the recurrent CNN"):
        _lib.check(lib.sg_ppo_set_symmetry(agent.h, 1.0, None, _lib.fptr(np.eye(1, dtype=np.float32))))
    with pytest.raises(E, match="sg_ppo_set_hidden_states must hand over"):
        _lib.check(lib.sg_ppo_update(agent.h, ro.h, None, 0, 1, (C.c_float * 3)()))
    big = sg.RolloutStorage(1025, 4, (1, HW, HW), Discrete(5), 16, 1)
    with pytest.raises(E, match="a minibatch of 4100 rows .* on the recurrent CNN base exceeds 4096"):
        agent.update(big)


# ------------------------------------------------------------------------------------------------- 6 the learner
class _Env(object):
    """A deterministic vectorised environment of [C, 84, 84] frames: the next frame and the reward are functions of the step and
    the actions."""

    def __init__(self, n, C_, K):
        self.num_envs, self.C, self.K, self.t = n, C_, K, 0
        yy, xx = np.meshgrid(np.arange(HW), np.arange(HW), indexing="ij")
        self.base = (yy * 3 + xx * 5)[None, None]

    def step(self, action):
        a = npv(action)
        assert a.dtype == np.int64 and a.shape == (self.num_envs, 1) and a.min() >= 0 and a.max() < self.K
        self.t += 1
        shift = (a[:, :, None, None] * 37 + self.t * 11 + np.arange(self.num_envs)[:, None, None, None] * 7 + np.arange(self.C)[None, :, None, None] * 13)
        obs = ((self.base + shift) % 256).astype(np.float32)
        reward = (np.cos(a.astype(np.float64) + self.t) * 0.5).astype(np.float32)
        done = [(self.t + i) % 3 == 0 for i in range(self.num_envs)]
        return obs, reward, done, [{} for _ in range(self.num_envs)]


def run_learner(sg, params, by_hand):
    from simgan_amd.driver import PpoLearner, step_masks
    from simgan_amd.utils import to_host_tensor
    C_, Hs, K, T, N = 1, 16, 5, 4, 4
    p = make_policy(sg, C_, Hs, "categorical", K, params)
    p.seed = 4242
    agent = sg.algo.PPO(p, 0.2, 2, 2, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=0.5, seed=9)
    ro = sg.RolloutStorage(T, N, (C_, HW, HW), Discrete(K), Hs, 1)
    env = _Env(N, C_, K)
    ro.obs[0].copy_(ro.obs.new_tensor(env.step(np.zeros((N, 1), np.int64))[0]))
    learner = PpoLearner(p, agent, ro)
    losses, snaps, hidden = [], [], []
    for j in range(2):
        if by_hand:      # the reference's sequence: act, insert, get_value, compute_returns, update, after_update
            for step in range(T):
                value, action, logp, hxs = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
                obs, reward, done, infos = env.step(action)
                masks, bad = step_masks(done, infos)
                ro.insert(obs, hxs, action, logp, value, reward, to_host_tensor(masks), to_host_tensor(bad), None)
            nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1])
            ro.compute_returns(nv, learner.use_gae, learner.gamma, learner.gae_lambda, learner.use_proper_time_limits)
            res = dict(zip(("value_loss", "action_loss", "dist_entropy"), agent.update(ro)))
            hidden.append(npv(ro.recurrent_hidden_states).copy())
            ro.after_update()
        else:
            learner.collect(env)
            hidden.append(npv(ro.recurrent_hidden_states).copy())
            res = learner.update()
        losses.append(tuple(float(np.float32(res[k])) for k in ("value_loss", "action_loss", "dist_entropy")))
        snaps.append(p.get_flat_params())
    return losses, snaps, hidden, npv(ro.masks).copy()


def test_ppo_learner_equals_the_hand_written_sequence(sg):
    params = gr.init_params(np.random.default_rng(11), 1, 16, "categorical", 5)
    params[-5 * 17:] *= 30.0
    a = run_learner(sg, params, by_hand=False)
    b = run_learner(sg, params, by_hand=True)
    assert a[0] == b[0] and np.isfinite(a[0]).all()
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        assert np.array_equal(bits(x), bits(y))
    assert np.abs(a[2][1][0]).max() > 0 and (a[3] == 0).any()      # the second rollout starts from a carried state; episodes end
    assert np.abs(a[1][1] - params).max() > 1e-4


# ------------------------------------------------------------------------------------------------- 7 the reference's fixtures
@pytest.mark.parametrize("name", ["policy_cnn_gru_cat", "policy_cnn_gru_box"])
def test_forward_matches_the_reference_fixture(sg, name):
    """tests/golden/policy_cnn_gru_*.npz: the reference's own float32 act / get_value / evaluate_actions (tools/gen_golden_cnn_gru.py)"""
    g = load(name)
    m = g["meta"]
    cat = m["dist"] == "categorical"
    T, n = m["T"], m["n"]
    p = make_policy(sg, m["C"], m["Hs"], m["dist"], m["P"], g["params"])
    assert [k for k, _ in p.param_shapes()] == [str(k) for k in g["keys"]]
    obs, hxs, masks = g["obs"].astype(np.float32), g["hxs"], g["masks"].reshape(-1, 1)
    v, lp, ent, h = p.evaluate_actions(obs, hxs, masks, g["eval_action"])
    assert_close(npv(v), g["eval_value"], what="value")
    assert_close(npv(lp), g["eval_logp"], what="logp")
    assert_close(npv(ent), g["eval_entropy"], what="entropy")
    assert_close(npv(h), g["eval_hxs"], what="final hidden state")
    assert_close(npv(p.get_value(obs[:n], hxs, masks[:n])), g["get_value"], what="get_value")
    v, a, lp, h1 = p.act(obs[:n], hxs, masks[:n], deterministic=True)
    a = npv(a)
    assert a.dtype == g["det_action"].dtype and a.shape == g["det_action"].shape
    if cat:
        assert np.array_equal(a, g["det_action"])
    else:
        assert_close(a, g["det_action"], what="mode")
    assert_close(npv(lp), g["det_logp"], what="logp of the mode")
    assert_close(npv(v), g["get_value"], what="value from act")
    assert_close(npv(h1), g["det_hxs"], what="hidden state from act")
    if cat:      # the injected uniforms through the inverse CDF, over the whole sequence (evaluate's log-probs are the drawn classes')
        h, acts, lps = hxs, [], []
        for t in range(T):
            sl = slice(t * n, (t + 1) * n)
            _, a, lp, h = p.act(obs[sl], h, masks[sl], noise=g["uniform"][sl].reshape(n, 1))
            acts.append(npv(a)); lps.append(npv(lp))
        assert np.array_equal(np.concatenate(acts), g["act_action"])
        assert_close(np.concatenate(lps), g["eval_logp"], what="logp of the drawn classes")
    else:
        v, a, lp, _ = p.act(obs[:n], hxs, masks[:n], noise=g["noise"])
        assert_close(npv(a), g["act_action"], what="sampled action")
        assert_close(npv(lp), g["act_logp"], what="its log-prob")
        assert_close(npv(v), g["act_value"], what="value")


def fixture_case(g):
    m = g["meta"]
    return cr.Case(C=m["C"], Hs=m["Hs"], dist=m["dist"], P=m["P"], T=m["T"], N=m["N"], params=g["params0"], obs=g["obs"].astype(np.float32),
                   actions=g["actions"], action_log_probs=g["action_log_probs"], value_preds=g["value_preds"], returns=g["returns"],
                   masks=g["masks"], hxs=g["hxs"])


@pytest.mark.parametrize("name", ["ppo_cnn_gru_cat", "ppo_cnn_gru_box"])
def test_whole_update_matches_the_reference_fixture(sg, name):
    """E = 2, M = 2 at (1, 16, Discrete(5), 4 x 4) and (2, 20, Box(3), 3 x 4) against the reference's own float32 PPO.update with its
    recorded permutations: losses within the tolerance, parameters within assert_close_adam's rule (tests/test_gpu_cnn.py's)"""
    g = load(name)
    m, c = g["meta"], fixture_case(g)
    assert (m["T"], m["N"], m["ppo_epoch"], m["num_mini_batch"]) in ((4, 4, 2, 2), (3, 4, 2, 2)) and (g["masks"][:-1] == 0).sum() >= 3
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = sg.algo.PPO(p, m["clip_param"], m["ppo_epoch"], m["num_mini_batch"], m["value_loss_coef"], m["entropy_coef"], lr=m["lr"], eps=m["eps"],
                        max_grad_norm=m["max_grad_norm"])
    losses = agent.update(rollout_of(sg, c), perms=g["perms"])
    assert agent.get_adam()[2] == m["steps"] == 4 and np.array_equal(agent.last_perms(), g["perms"])
    ref = load(name + "_params1")["ppo_params1"]
    assert_close(losses, g["ppo_losses"], what="losses")
    assert_close_adam(p.get_flat_params(), ref, m["lr"], m["steps"], what="params after the update")


def test_the_reference_checkpoint_loads_and_evaluates(sg):
    from simgan_amd.checkpoint import load_policy
    g = load("ckpt_policy_cnn_gru")
    m = g["meta"]
    p, ob_rms = load_policy(os.path.join(GOLDEN, "ckpt_policy_cnn_gru.pt"))
    assert ob_rms is None and p.is_recurrent and p.cnn == m["C"] and p.hidden_size == m["Hs"] and p.recurrent_hidden_state_size == m["Hs"]
    assert [k for k, _ in p.param_shapes()] == m["names"] and [list(s) for _, s in p.param_shapes()] == m["shapes"]
    assert np.array_equal(p.get_flat_params(), g["params"])
    assert abs(float(p.get_flat_params().astype(np.float64).sum()) - float(g["checksum"])) < 1e-6 * max(1.0, abs(float(g["checksum"])))
    v, lp, ent, h = p.evaluate_actions(g["obs"].astype(np.float32), g["hxs"], g["masks"], g["actions"])
    assert_close(npv(v), g["value"], what="value")
    assert_close(npv(lp), g["logp"], what="logp")
    assert_close(npv(ent), g["entropy"], what="entropy")
    assert_close(npv(h), g["hxs_out"], what="final hidden state")


# ------------------------------------------------------------------------------------------------- 8 the remaining C-ABI refusals
def test_c_abi_refusals_of_diagnostics_chain_ensemble_and_world(sg):
    import threading
    from simgan_amd import _lib
    c = gr.case(*UPDATE_KEYS[0])
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    lib, E = p.lib, _lib.SimganHipError
    ro = rollout_of(sg, c)
    ro.device_resident = True
    ro.sync_to_device()
    out = (C.c_double * 16)()
    hx = np.ascontiguousarray(c.hxs[0])
    for name in ("sg_rollout_policy_diagnostics", "sg_rollout_policy_diagnostics_world"):
        with pytest.raises(E, match=f"{name}: the policy has the recurrent CNN base"):
            _lib.check(getattr(lib, name)(ro.h, p.h, 0.2, _lib.fptr(hx), out))
    n = c.N
    members = (_lib.H * 1)(p.h)
    idx = np.zeros(n, np.int32)
    f = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    a, ia, ir = f(n, 1), f(n, 1), f(n, 1)
    with pytest.raises(E, match="sg_rollout_act_step_chain: the learner has the recurrent CNN base"):
        _lib.check(lib.sg_rollout_act_step_chain(ro.h, p.h, 0, _lib.CHAIN_LEARNER_FIRST, members, 1, idx.ctypes.data_as(C.POINTER(C.c_int32)), None, None,
                                                 None, None, 0, 1, None, 0, 1, 0, _lib.fptr(a), _lib.fptr(ia), _lib.fptr(ir)))
    obs = np.ascontiguousarray(c.obs[0].reshape(n, -1))
    v, lp = f(n), f(n)
    with pytest.raises(E, match="sg_policy_act_ensemble: member 0 has the recurrent CNN base"):
        _lib.check(lib.sg_policy_act_ensemble(members, 1, idx.ctypes.data_as(C.POINTER(C.c_int32)), _lib.fptr(obs), n, None, 0, 1, _lib.fptr(v),
                                              _lib.fptr(a), _lib.fptr(lp)))
    # a communicator of world 2 (the loopback transport, two contexts on this device, one host thread each)
    uid = _lib.comm_loopback_id()
    msgs, errs = [None, None], [None, None]

    def body(rank):
        try:
            ctx = _lib.Context(0)
            ctx.comm_init(uid, rank, 2)
            q = sg.Policy((c.C, HW, HW), space(c.dist, c.P), base_kwargs={"recurrent": True, "hidden_size": c.Hs}, recurrent_cnn=True, ctx=ctx)
            cfg = _lib.PPOConfig(0.2, 1, 1, 0.5, 0.01, 3e-4, 1e-5, 0.5, 1)
            h = _lib.H()
            try:
                _lib.check(ctx.lib.sg_ppo_create(ctx.h, q.h, C.byref(cfg), C.byref(h)))
                msgs[rank] = "created"
            except E as exc:
                msgs[rank] = str(exc)
            ctx.synchronize()
        except BaseException as exc:   # noqa: BLE001 -- reported below
            errs[rank] = exc
    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads) and errs == [None, None], errs
    for msg in msgs:
        assert "sg_ppo_create: PPO on the recurrent CNN base runs on one rank" in msg and "world 2" in msg, msg
