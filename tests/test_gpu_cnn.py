"""GPU: Policy on image observations -- the CNN base (csrc/sg_cnn.hip, sg_cnn_kernels.hpp) through act, get_value,
evaluate_actions, RolloutStorage, PPO.update and PpoLearner.

  1 forward     the three policy calls against the reference's fixtures (tests/golden/policy_cnn_*.npz) and, at the default width
                (C = 4, Hs = 512, Discrete(6)) and past one 128-row pass (n = 130), against tests/cnn_ref.py in float64
  2 gradient    one optimizer step read back as m / (1 - beta1) from Adam's first moment, per parameter block against float64
                autograd within RTOL: with the clip out of reach and at max_grad_norm = 0.5 (the restated clip factor applied to
                the reference); cases from tests/cnn_ref.py, which keep clear of the ReLU kinks (tests/test_cnn_host.py)
  3 gather      E = 1, M = 2 with injected permutations at lr = 0: m = 0.9 * 0.1 * g1 + 0.1 * g2 with g1, g2 autograd's on exactly
                the first and the second 8 permuted rows (the weights differ, so swapped or unpermuted halves show)
  4 update      whole updates (E = 2, M = 2, 16 rows) against the reference's fixtures (ppo_cnn_*.npz)
  5 determinism two updates from the same state, replayed from the captured graph and launched kernel by kernel: the same bits
  6 learner     driver.PpoLearner on host and device-resident rollouts, the results ring, the linear schedule
  7 round trips state_dict / flat parameters / native pickle; the reference's checkpoint fixture
  8 refusals    in C and in Python, each by its own message
SG_CNN_RECORD=<path> collects the measured distances of 1, 2 and 4 (profiles/cnn_parity.json)."""
import ctypes as C
import json
import os
import pickle
import warnings

import numpy as np
import pytest
import torch

import cnn_ref as cr
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


def make_policy(sg, C_, Hs, dist, P, params=None, **kw):
    p = sg.Policy((C_, HW, HW), space(dist, P), base_kwargs={"hidden_size": Hs}, **kw)
    assert [(n, tuple(s)) for n, s in p.param_shapes()] == cr.param_shapes(C_, Hs, dist, P)
    assert not p.is_recurrent and p.recurrent_hidden_state_size == 1 and p.cnn == C_
    if params is not None:
        p.set_flat_params(params)
    return p


def fill(ro, **fields):
    for name, arr in fields.items():
        t = getattr(ro, name)
        t.copy_(t.new_tensor(np.asarray(arr).reshape(tuple(t.shape))))


def rollout_of(sg, c):
    ro = sg.RolloutStorage(c.T, c.N, (c.C, HW, HW), space(c.dist, c.P), 1, 1)
    assert tuple(ro.obs.shape) == (c.T + 1, c.N, c.C, HW, HW)
    fill(ro, **{k: c[k] for k in ("obs", "actions", "action_log_probs", "value_preds", "returns")})
    return ro


def ratio(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    return float(np.max(np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))))


def _record(label, rec):
    path = os.environ.get("SG_CNN_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_cnn.py under SG_CNN_RECORD: the largest ratio to the tolerance per case -- forward values "
                       "element by element against ATOL + RTOL |ref|, one-step gradients per parameter block as the rel-L2 distance of "
                       "tests/cnn_ref.py:block_distances over RTOL, whole updates as the losses' ratio and the parameters' largest "
                       "error over lr * steps", "cases": {}}
    doc["cases"][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


# ------------------------------------------------------------------------------------------------- 1 forward
@pytest.mark.parametrize("name,n", [("policy_cnn_cat", 1), ("policy_cnn_cat", 5), ("policy_cnn_cat", 17), ("policy_cnn_box", 33)])
def test_forward_matches_the_reference_fixture(sg, name, n):
    g = load(name)
    m = g["meta"]
    cat = m["dist"] == "categorical"
    p = make_policy(sg, m["C"], m["Hs"], m["dist"], m["P"], g["params"])
    obs = torch.from_numpy(g["obs"][:n].astype(np.float32))
    assert tuple(obs.shape) == (n, m["C"], HW, HW)
    rec = {}
    v, lp, ent, hx = p.evaluate_actions(obs, None, None, torch.from_numpy(g["eval_action"][:n]))
    assert tuple(v.shape) == (n, 1) and tuple(lp.shape) == (n, 1) and hx is None
    rec["evaluate"] = max(ratio(npv(v), g["eval_value"][:n]), ratio(npv(lp), g["eval_logp"][:n]), ratio(npv(ent), g[f"eval_entropy_{n}"]))
    assert_close(npv(v), g["eval_value"][:n], what="value")
    assert_close(npv(lp), g["eval_logp"][:n], what="logp")
    assert_close(npv(ent), g[f"eval_entropy_{n}"], what="entropy")
    gv = p.get_value(obs.reshape(n, -1), None, None)      # flat [n, C * 7056] rows are taken too
    assert_close(npv(gv), g["get_value"][:n], what="get_value")
    assert np.array_equal(npv(gv), npv(p.get_value(obs, None, None)))
    v, a, lp, _ = p.act(obs, None, None, deterministic=True)
    a = npv(a)
    assert a.dtype == g["det_action"].dtype and a.shape == (n, 1 if cat else m["P"])
    if cat:
        assert np.array_equal(a, g["det_action"][:n])     # (the generator keeps every mode 1e-4 clear of a tie)
    else:
        assert_close(a, g["det_action"][:n], what="mode")
    assert_close(npv(lp), g["det_logp"][:n], what="logp of the mode")
    assert_close(npv(v), g["get_value"][:n], what="value from act")
    rec["act_deterministic"] = max(ratio(npv(lp), g["det_logp"][:n]), ratio(npv(v), g["get_value"][:n]))
    # the injected draw: uniforms through the inverse CDF (Discrete), normals through mean + std * z (Box)
    noise = g["uniform"][:n].reshape(n, 1) if cat else g["noise"][:n]
    v, a, lp, _ = p.act(obs, None, None, noise=noise)
    if cat:
        assert np.array_equal(npv(a), g["act_action"][:n])     # (every draw 1e-4 clear of a cumulative boundary)
        assert_close(npv(lp), g["eval_logp"][:n], what="logp of the drawn class")    # eval_action IS the drawn class
        rec["act_sampled"] = ratio(npv(lp), g["eval_logp"][:n])
    else:
        assert_close(npv(a), g["act_action"][:n], what="sampled action")
        assert_close(npv(lp), g["act_logp"][:n], what="its log-prob")
        assert_close(npv(v), g["act_value"][:n], what="value")
        rec["act_sampled"] = max(ratio(npv(a), g["act_action"][:n]), ratio(npv(v), g["act_value"][:n]))
    _record(f"forward {name} n={n}", rec)


def default_width_inputs(C_=4, P=6, n=2):
    """parameters off the initialisation (biases off zero, a head 30 x its gain-0.01 start so that the logits differ) and frames"""
    shapes = cr.param_shapes(C_, 512, "categorical", P)
    rng = np.random.default_rng(5)
    params = cr.init_params(rng, shapes)
    params[-P * 513:] *= 30.0
    return params, rng.integers(0, 256, (n, C_, HW, HW)).astype(np.float32)


def test_forward_at_the_default_width_matches_float64(sg):
    """C = 4, Hs = 512 (the default, a2c/model.py:205), Discrete(6), n = 2: the FC layer's 3.2 MB weight, streamed"""
    C_, P, n = 4, 6, 2
    p = sg.Policy((C_, HW, HW), Discrete(P), seed=3)
    assert p.hidden_size == 512 and p.num_params == 32 * C_ * 64 + 32 + 32768 + 64 + 18432 + 32 + 512 * 1568 + 512 + 512 + 1 + P * 512 + P
    shapes = cr.param_shapes(C_, 512, "categorical", P)
    blocks = dict(cr.blocks(shapes, p.get_flat_params()))     # the constructor's initialisation: orthogonal rows at ReLU gain, zero biases
    assert not blocks["base.main.0.bias"].any() and abs(np.linalg.norm(blocks["base.main.2.weight"].reshape(64, -1)[0]) - np.sqrt(2)) < 1e-3
    assert abs(np.linalg.norm(blocks["base.critic_linear.weight"]) - 1.0) < 1e-3
    params, obs = default_width_inputs()
    p.set_flat_params(params)
    det = cr.act64(shapes, params, obs, "categorical")
    assert det["margin"] > 1e-3
    v, a, lp, _ = p.act(obs, None, None, deterministic=True)
    assert np.array_equal(npv(a).reshape(-1), det["action"])
    assert_close(npv(v), det["value"], what="value")
    assert_close(npv(lp), det["logp"], what="logp")
    acts = np.array([[1], [4]], np.int64)
    with torch.no_grad():
        rv, rlp, rent = cr.evaluate(cr.leaves(params, shapes), cr.ar.t64(obs), acts, "categorical")
    v, lp, ent, _ = p.evaluate_actions(obs, None, None, acts)
    assert_close(npv(v), rv.numpy(), what="value")
    assert_close(npv(lp), rlp.numpy(), what="logp")
    assert_close(npv(ent), rent.numpy(), what="entropy")
    _record("forward C=4 Hs=512 Discrete(6) n=2", {"evaluate": max(ratio(npv(v), rv.numpy()), ratio(npv(lp), rlp.numpy()), ratio(npv(ent), rent.numpy()))})


def test_forward_past_one_pass_of_rows_matches_float64(sg):
    """n = 130: the inference forward takes 128 rows per pass (SG_CNN_FWD_ROWS), so rows 128 and 129 come from a second pass that
    writes into the head stacks at its row offset; C = 1, Hs = 16, Box((3,))"""
    C_, Hs, P, n = 1, 16, 3, 130
    shapes = cr.param_shapes(C_, Hs, "gaussian", P)
    rng = np.random.default_rng(21)
    params = cr.init_params(rng, shapes)
    obs = rng.integers(0, 256, (n, C_, HW, HW)).astype(np.float32)
    acts = rng.standard_normal((n, P)).astype(np.float32)
    p = make_policy(sg, C_, Hs, "gaussian", P, params)
    with torch.no_grad():
        rv, rlp, rent = cr.evaluate(cr.leaves(params, shapes), cr.ar.t64(obs), acts, "gaussian")
    assert np.ptp(rv.numpy()) > 1e-3      # the rows differ, so a row written to another row's place shows
    v, lp, ent, _ = p.evaluate_actions(obs, None, None, acts)
    assert tuple(v.shape) == (n, 1) and tuple(lp.shape) == (n, 1)
    assert_close(npv(v), rv.numpy(), what="value")
    assert_close(npv(lp), rlp.numpy(), what="logp")
    assert_close(npv(ent), rent.numpy(), what="entropy")
    rec = {"evaluate": max(ratio(npv(v), rv.numpy()), ratio(npv(lp), rlp.numpy()), ratio(npv(ent), rent.numpy()))}
    det = cr.act64(shapes, params, obs, "gaussian")
    v, a, lp, _ = p.act(obs, None, None, deterministic=True)
    assert_close(npv(a), det["action"], what="mode")
    assert_close(npv(v), det["value"], what="value from act")
    assert_close(npv(lp), det["logp"], what="logp of the mode")
    assert_close(npv(p.get_value(obs, None, None)), det["value"], what="get_value")
    rec["act_deterministic"] = max(ratio(npv(v), det["value"]), ratio(npv(lp), det["logp"]), ratio(npv(a), det["action"]))
    _record(f"forward C=1 Hs=16 Box(3) n={n}", rec)


# ------------------------------------------------------------------------------------------------- 2 one-step gradient
def one_step(sg, c, max_grad_norm, use_clipped, perms=None, E=1, M=1, lr=LR, ecoef=cr.ECOEF):
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = sg.algo.PPO(p, cr.CLIP, E, M, cr.VCOEF, ecoef, lr=lr, eps=EPS, max_grad_norm=max_grad_norm, use_clipped_value_loss=use_clipped)
    B = c.T * c.N
    perms = np.arange(B, dtype=np.int64)[None] if perms is None else perms
    losses = agent.update(rollout_of(sg, c), perms=perms)
    m, v, step = agent.get_adam()
    assert step == E * M and np.array_equal(agent.last_perms(), perms)
    return m, losses, p


GRAD_RUNS = [(key, mgn, True) for key in cr.GRAD_CASES for mgn in (1e9, 0.5)] + [(cr.GRAD_CASES[4], 1e9, False), (cr.GRAD_CASES[4], 0.5, False)]


@pytest.mark.parametrize("key,max_grad_norm,use_clipped", GRAD_RUNS,
                         ids=[f"{'-'.join(map(str, k))}-clip{m}-{'clipped' if u else 'plain'}" for k, m, u in GRAD_RUNS])
def test_one_step_gradient_per_block(sg, key, max_grad_norm, use_clipped):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")    # (1 x 1: the unbiased std of one advantage)
        c = cr.case(*key)
        r = cr.rows_of(c)
        ref, ref_losses = cr.ppo_grad(c.shapes, c.params, r["obs"], r["actions"], r["old_logp"], r["value_preds"], r["returns"], r["adv"], c.dist,
                                      use_clipped)
    m, losses, _ = one_step(sg, c, max_grad_norm, use_clipped)
    got = m.astype(np.float64) / (1.0 - 0.9)
    factor = cr.clip_factor(ref, max_grad_norm)
    label = f"gradient {c.tag} max_grad_norm={max_grad_norm:g} {'clipped' if use_clipped else 'plain'} value loss"
    if c.T * c.N == 1:
        # the reference has no finite number here (tests/test_cnn_host.py): NaN advantage, NaN norm, every element NaN
        assert np.isnan(factor) and np.isnan(got).all() and np.isnan(losses[1])
        assert_close(losses[0], ref_losses[0], what="value loss")
        assert_close(losses[2], ref_losses[2], what="entropy")
        _record(label, {"all_nan_as_in_the_reference": True})
        return
    if max_grad_norm < 1.0:
        assert factor < 1.0      # the clip acts in every such run
    else:
        assert factor == 1.0
    d = cr.block_distances(got, ref * factor, c.shapes)
    _record(label, {"clip_factor": factor, "worst": max(d.values()) / RTOL, "blocks": {k: x / RTOL for k, x in d.items()},
                    "losses": ratio(losses, ref_losses)})
    assert_close(losses, ref_losses, what="losses")
    bad = {k: x for k, x in d.items() if not x <= RTOL}
    assert not bad, f"{c.tag}: blocks past {RTOL:g}: {bad}"


# ------------------------------------------------------------------------------------------------- 3 the minibatch gather
def test_minibatches_are_exactly_the_permuted_rows(sg):
    c = cr.case(*cr.GATHER_CASE)
    B = c.T * c.N
    perm = np.random.default_rng(cr.GATHER_PERM_SEED).permutation(B).astype(np.int64)
    assert not np.array_equal(perm, np.arange(B)) and sorted(perm[:8]) != list(range(8))
    r = cr.rows_of(c)
    gs = []
    for half in (perm[:B // 2], perm[B // 2:]):
        g, _ = cr.ppo_grad(c.shapes, c.params, r["obs"][half], r["actions"][half], r["old_logp"][half], r["value_preds"][half], r["returns"][half],
                           r["adv"][half], c.dist)     # advantages normalised over all 16 rows
        gs.append(g)
    # lr = 0: the parameters stay put, so the second step's gradient is autograd's at the same parameters
    m, _, p = one_step(sg, c, 1e9, True, perms=perm[None], E=1, M=2, lr=0.0)
    assert np.array_equal(p.get_flat_params(), c.params)
    want = 0.9 * 0.1 * gs[0] + 0.1 * gs[1]
    d = cr.block_distances(m, want, c.shapes)
    assert max(d.values()) <= RTOL, d
    # the test of the test: the halves swapped, or the rows taken in rollout order, are seen
    assert max(cr.block_distances(0.9 * 0.1 * gs[1] + 0.1 * gs[0], want, c.shapes).values()) > 10 * RTOL
    plain = [cr.ppo_grad(c.shapes, c.params, *(r[k][s] for k in ("obs", "actions", "old_logp", "value_preds", "returns", "adv")), c.dist)[0]
             for s in (slice(0, 8), slice(8, 16))]
    assert max(cr.block_distances(0.09 * plain[0] + 0.1 * plain[1], want, c.shapes).values()) > 10 * RTOL


# ------------------------------------------------------------------------------------------------- 4 whole updates
def fixture_case(g):
    m = g["meta"]
    return cr.Case(C=m["C"], Hs=m["Hs"], dist=m["dist"], P=m["P"], T=m["T"], N=m["N"], params=g["params0"], obs=g["obs"].astype(np.float32),
                   actions=g["actions"], action_log_probs=g["action_log_probs"], value_preds=g["value_preds"], returns=g["returns"])


def fixture_agent(sg, g, **kw):
    m, c = g["meta"], fixture_case(g)
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = sg.algo.PPO(p, m["clip_param"], m["ppo_epoch"], m["num_mini_batch"], m["value_loss_coef"], m["entropy_coef"], lr=m["lr"], eps=m["eps"],
                        max_grad_norm=m["max_grad_norm"], **kw)
    return p, agent, rollout_of(sg, c)


@pytest.mark.parametrize("name", ["ppo_cnn_cat", "ppo_cnn_box"])
def test_whole_update_matches_the_reference_fixture(sg, name):
    g = load(name)
    m = g["meta"]
    p, agent, ro = fixture_agent(sg, g)
    losses = agent.update(ro, perms=g["perms"])
    assert agent.get_adam()[2] == 4 and np.array_equal(agent.last_perms(), g["perms"])
    ref = load(name + "_params1")["ppo_params1"]
    got = p.get_flat_params()
    _record(f"update {name}", {"losses": ratio(losses, g["ppo_losses"]), "params_max_err_over_lr_steps": float(np.abs(got - ref).max() / (m["lr"] * 4)),
                               "params_out_of_tol": int((np.abs(got.astype(np.float64) - ref) > ATOL + RTOL * np.abs(ref)).sum())})
    assert_close(losses, g["ppo_losses"], what="losses")
    assert_close_adam(got, ref, m["lr"], 4, what="params after the update")


# ------------------------------------------------------------------------------------------------- 5 determinism
def test_two_runs_and_the_graph_replay_give_the_same_bits(sg, monkeypatch):
    g = load("ppo_cnn_cat")
    out = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        p, agent, ro = fixture_agent(sg, g)
        losses = [agent.update(ro, perms=g["perms"]) for _ in range(2)]      # (the second update of a graph run is a replay)
        out.append((losses, p.get_flat_params(), *agent.get_adam()[:2]))
    for other in out[1:]:
        assert other[0] == out[0][0]
        for a, b in zip(out[0][1:], other[1:]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(out[0][1]).all() and np.abs(out[0][1] - g["params0"]).max() > 1e-4


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
        done = [(self.t + i) % 5 == 0 for i in range(self.num_envs)]
        return obs, reward, done, [{} for _ in range(self.num_envs)]


def run_learner(sg, params, resident, by_hand=False, decay=True):
    from simgan_amd.driver import PpoLearner, _returns_resident
    C_, Hs, K, T, N = 1, 16, 5, 3, 4
    p = make_policy(sg, C_, Hs, "categorical", K, params)
    p.seed = 4242
    agent = sg.algo.PPO(p, 0.2, 2, 2, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=0.5, seed=9)
    ro = sg.RolloutStorage(T, N, (C_, HW, HW), Discrete(K), 1, 1)
    env = _Env(N, C_, K)
    ro.obs[0].copy_(ro.obs.new_tensor(env.step(np.zeros((N, 1), np.int64))[0]))
    ro.device_resident = resident
    learner = PpoLearner(p, agent, ro, use_linear_lr_decay=decay, lr=LR if decay else None, num_updates=2 if decay else None)
    losses, snaps = [], []
    for j in range(2):
        learner.collect(env)
        if by_hand:      # PpoLearner.update()'s resident body with the losses fetched synchronously
            if decay:
                sg.update_linear_schedule(agent.optimizer, j, 2, LR)
            _returns_resident(learner)
            res = dict(zip(("value_loss", "action_loss", "dist_entropy"), agent.update(ro)))
            ro.after_update()
            learner.j += 1
        else:
            res = learner.update()
        losses.append(tuple(float(np.float32(res[k])) for k in ("value_loss", "action_loss", "dist_entropy")))
        snaps.append(p.get_flat_params())
    return losses, snaps, agent.optimizer.param_groups[0]["lr"], npv(ro.actions).copy()


def test_ppo_learner_on_host_and_device_resident_rollouts(sg):
    params = cr.init_params(np.random.default_rng(11), cr.param_shapes(1, 16, "categorical", 5))
    params[-5 * 17:] *= 30.0      # a head that prefers some classes: the environment sees different actions
    ring = run_learner(sg, params, resident=True)
    hand = run_learner(sg, params, resident=True, by_hand=True)
    host = run_learner(sg, params, resident=False)
    flat = run_learner(sg, params, resident=True, decay=False)
    assert ring[0] == hand[0], "the results ring and the synchronous calls disagree"
    for a, b in zip(ring[1], hand[1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(ring[3], hand[3]) and len(set(ring[3].reshape(-1).tolist())) > 1
    assert np.isfinite(host[0]).all() and np.isfinite(host[1][1]).all() and np.abs(host[1][1] - params).max() > 1e-4
    assert np.array_equal(host[3], ring[3]), "host and device-resident modes collected different actions"
    assert_close(host[0], ring[0], what="losses, host against device-resident")
    # a2c/utils.py:68-72: lr, then lr / 2 -- the first update is the undecayed one, the second is not
    assert ring[2] == LR * 0.5 and flat[2] == LR
    assert np.array_equal(ring[1][0], flat[1][0]) and not np.array_equal(ring[1][1], flat[1][1])
    step2 = np.abs(ring[1][1].astype(np.float64) - ring[1][0]).mean() / np.abs(flat[1][1].astype(np.float64) - flat[1][0]).mean()
    assert 0.4 < step2 < 0.6, step2
    from simgan_amd.driver import PpoLearner
    # (a Box policy: with a Discrete one the older check of the action space answers first, as its tests pin)
    p = make_policy(sg, 1, 16, "gaussian", 3)
    ro = sg.RolloutStorage(3, 4, (1, HW, HW), Box((3,)), 1, 1)
    ro.device_resident = True
    learner = PpoLearner(p, sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=0.5), ro)
    with pytest.raises(ValueError, match=r"PpoLearner.collect\(on_device=True\): the policy has the CNN base"):
        learner.collect(_Env(4, 1, 5), on_device=True)


# ------------------------------------------------------------------------------------------------- 7 round trips
def test_state_dict_flat_parameters_and_pickle_round_trip(sg):
    c = cr.case(*cr.GRAD_CASES[3])
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    sd = p.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == c.shapes
    assert np.array_equal(np.concatenate([npv(v).reshape(-1) for v in sd.values()]), c.params)
    q = make_policy(sg, c.C, c.Hs, c.dist, c.P, seed=1)
    assert not np.array_equal(q.get_flat_params(), c.params)
    q.load_state_dict(sd)
    assert np.array_equal(q.get_flat_params(), c.params)
    obs = cr.rows_of(c)["obs"][:4]
    want = [npv(x) for x in p.act(obs, None, None, deterministic=True)[:3]]
    back = pickle.loads(pickle.dumps(p))
    assert type(back) is sg.Policy and back.cnn == c.C and back.hidden_size == c.Hs and np.array_equal(back.get_flat_params(), c.params)
    for a, b in zip(want, back.act(obs, None, None, deterministic=True)[:3]):
        assert np.array_equal(a, npv(b))
    q.reset_variance(Box((c.P,)), -1.25)
    assert np.array_equal(npv(q.state_dict()["dist.logstd._bias"]), np.full((c.P, 1), -1.25, np.float32))
    with pytest.raises(NotImplementedError, match="reset_critic on a policy with the CNN base"):
        q.reset_critic((c.C, HW, HW))


def test_the_reference_checkpoint_acts_as_the_reference_did(sg):
    from simgan_amd.checkpoint import load_policy
    g = load("ckpt_policy_cnn")
    m = g["meta"]
    p, rms = load_policy(os.path.join(GOLDEN, "ckpt_policy_cnn.pt"))
    assert rms is None and type(p) is sg.Policy and p.cnn == m["C"] and p.hidden_size == m["Hs"] and p.n_out == m["P"] and p.dist_kind == 1
    assert list(p.state_dict()) == m["names"]
    v, a, lp, _ = p.act(g["obs"].astype(np.float32), None, None, deterministic=True)
    assert np.array_equal(npv(a), g["action"])
    assert_close(npv(v), g["value"], what="value")
    assert_close(npv(lp), g["logp"], what="logp")


# ------------------------------------------------------------------------------------------------- 8 refusals
def test_refusals_behind_the_c_abi(sg):
    from simgan_amd import _lib
    p = make_policy(sg, 1, 16, "categorical", 5)
    box = make_policy(sg, 1, 16, "gaussian", 3)
    lib, ctx, h = p.lib, p.ctx, _lib.H()
    E = _lib.SimganHipError
    with pytest.raises(E, match="the CNN base takes 84 x 84 images only \\(got 64 x 84\\)"):
        _lib.check(lib.sg_policy_create_cnn(ctx.h, 1, 64, 84, 16, 1, 1, 5, C.byref(h)))
    with pytest.raises(E, match="the CNN base is built with the Gaussian \\(Box\\) and Categorical \\(Discrete\\) heads; dist 2"):
        _lib.check(lib.sg_policy_create_cnn(ctx.h, 1, 84, 84, 16, 2, 5, 5, C.byref(h)))
    with pytest.raises(E, match="sg_policy_create_cnn: bad dims"):
        _lib.check(lib.sg_policy_create_cnn(ctx.h, 0, 84, 84, 16, 1, 1, 5, C.byref(h)))
    # the three older constructors do not reach the CNN base
    for call in (lambda: lib.sg_policy_create(ctx.h, 3, 4, 2, 8, 1, C.byref(h)), lambda: lib.sg_policy_create2(ctx.h, 3, 4, 2, 8, 1, 0, C.byref(h)),
                 lambda: lib.sg_policy_create3(ctx.h, 3, 4, 2, 8, 1, 0, 0, 0, C.byref(h))):
        with pytest.raises(E, match="unknown kind 3"):
            _lib.check(call())
    with pytest.raises(E, match="sg_a2c_create: A2C is not implemented for the CNN base"):
        _lib.check(lib.sg_a2c_create(ctx.h, p.h, C.byref(_lib.A2CConfig(0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5)), C.byref(h)))
    with pytest.raises(E, match="sg_acktr_create: ACKTR is not implemented for the CNN base"):
        _lib.check(lib.sg_acktr_create(ctx.h, box.h, C.byref(_lib.ACKTRConfig(0.5, 0.01, 0.25, 0.9, 0.99, 0.001, 1e-2, 10)), C.byref(h)))
    agent = sg.algo.PPO(box, 0.2, 1, 1, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=0.5)
    eye = np.eye(3, dtype=np.float32)
    with pytest.raises(E, match="sg_ppo_set_symmetry: the mirror-symmetry loss is not implemented for the CNN base"):
        _lib.check(lib.sg_ppo_set_symmetry(agent.h, 1.0, None, _lib.fptr(eye)))
    _lib.check(lib.sg_ppo_set_symmetry(agent.h, 0.0, None, None))     # coef 0 is plain PPO and stays accepted
    n = 2
    obs = np.zeros((n, 7056), np.float32)
    val, act, lp = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    handles = (_lib.H * 1)(box.h)
    idx = np.zeros(n, np.int32)
    with pytest.raises(E, match="sg_policy_act_ensemble: member 0 has the CNN base"):
        _lib.check(lib.sg_policy_act_ensemble(handles, 1, idx.ctypes.data_as(C.POINTER(C.c_int32)), _lib.fptr(obs), n, None, 1, 1, _lib.fptr(val),
                                              _lib.fptr(act), _lib.fptr(lp)))
    ro = sg.RolloutStorage(2, n, (1, HW, HW), Box((3,)), 1, 1)
    with pytest.raises(E, match="sg_rollout_act_step: the policy has the CNN base"):
        _lib.check(lib.sg_rollout_act_step(ro.h, box.h, 0, _lib.fptr(obs), None, 1, 1, _lib.fptr(act)))
    masks = np.ones(n, np.float32)
    with pytest.raises(E, match="sg_rollout_act_step_rnn: the policy has the CNN base"):
        _lib.check(lib.sg_rollout_act_step_rnn(ro.h, box.h, 0, _lib.fptr(obs), _lib.fptr(masks), None, 1, 1, _lib.fptr(act)))
    # a rollout of other dimensions is refused by the update as for every policy
    small = sg.RolloutStorage(2, n, (5,), Box((3,)), 1, 1)
    with pytest.raises(E, match="rollout dims \\(obs 5, act 3\\) do not match the policy \\(7056, 3\\)"):
        agent.update(small)


def test_refusals_in_python_on_a_live_policy(sg):
    from simgan_amd.driver import GailDynLearner
    from simgan_amd.ensemble import PolicyEnsemble
    p = make_policy(sg, 1, 16, "gaussian", 3)
    for acktr in (False, True):
        with pytest.raises(NotImplementedError, match="A2C_ACKTR: not implemented for the CNN base"):
            sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=acktr, **({} if acktr else dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)))
    with pytest.raises(NotImplementedError, match="PolicyEnsemble: members with the MLP base only"):
        PolicyEnsemble([p])
    with pytest.raises(NotImplementedError, match="mirror-symmetry loss: not implemented for the CNN base"):
        sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.0, symmetry_coef=1.0, lr=LR, eps=EPS, max_grad_norm=0.5, mirror_obs=np.eye(3), mirror_act=np.eye(3))
    with pytest.raises(NotImplementedError, match="GailDynLearner: the GAIL-dyn loop is built for 1-D observations"):
        GailDynLearner(p, None, None, None, None)
    with pytest.raises(NotImplementedError, match="Policy on image observations with a MultiBinary action space"):
        sg.Policy((1, HW, HW), MultiBinary(4))
    with pytest.raises(ValueError, match=r"the CNN base takes \[C, 84, 84\] only"):
        sg.Policy((1, 80, 80), Discrete(4))
    ro = sg.RolloutStorage(2, 2, (1, HW, HW), Box((3,)), 1, 1)
    ro.device_resident = True
    with pytest.raises(NotImplementedError, match="act_step: on-device collection is not built for image observations"):
        ro.act_step(p)
    with pytest.raises(NotImplementedError, match="enable_dup_sym: a mirror-augmented rollout mirrors observations"):
        ro.enable_dup_sym(np.eye(3), np.eye(3))
    with pytest.raises(NotImplementedError, match="enable_device_hidden: the rollout holds image observations"):
        ro.enable_device_hidden()


def test_ppo_on_the_cnn_base_is_refused_on_two_ranks(sg):
    from simgan_amd import _lib
    from test_gpu_world import run_ranks

    def rank_fn(rank, ctx):
        p = make_policy(sg, 1, 16, "categorical", 5, ctx=ctx)
        try:
            sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=0.5)
            py = "accepted"
        except NotImplementedError as exc:
            py = str(exc)
        h = _lib.H()
        cfg = _lib.PPOConfig(0.2, 1, 1, 0.5, 0.01, LR, EPS, 0.5, 1)
        rc = p.lib.sg_ppo_create(ctx.h, p.h, C.byref(cfg), C.byref(h))
        return py, rc, p.lib.sg_last_error().decode()

    for py, rc, msg in run_ranks(2, rank_fn):
        assert "PPO on the CNN base (image observations) runs on one rank" in py and "world 2" in py
        assert rc != 0 and "sg_ppo_create: PPO on the CNN base (image observations) runs on one rank" in msg
