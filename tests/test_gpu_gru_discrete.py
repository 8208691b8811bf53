"""GPU: the recurrent Policy on Discrete / MultiBinary action spaces (Policy(..., recurrent_heads=True) / sg_policy_create_rnn_dist):
act, get_value and evaluate_actions through the GRU into k_discrete_head, PPO through time with k_ppo_bwd_dist_dx and A2C through
time with k_a2c_bwd_dist_dx -- against the arbiter of tests/gru_discrete_ref.py per parameter block, against its feed-forward and
Gaussian twins bit for bit, and against the reference-written fixtures of tools/gen_golden_gru_discrete.py.

The one-step gradient is recovered from the optimizer: Adam's first step leaves m = (1 - beta1) g; RMSprop's first step from
square_avg = 0 leaves square_avg = (1 - alpha) g^2, so g = sign(p0 - p1) sqrt(square_avg / (1 - alpha)).  The clip is put out of
reach for those runs."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import diag_ref as dg
import gru_discrete_ref as ref
from helpers import assert_close, assert_close_adam, load, relerr

pytestmark = pytest.mark.gpu

A2C_HP = dict(value_loss_coef=ref.VCOEF, entropy_coef=ref.ECOEF, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
PPO_HP = dict(clip_param=ref.CLIP, ppo_epoch=1, num_mini_batch=1, value_loss_coef=ref.VCOEF, entropy_coef=ref.ECOEF, lr=3e-4, eps=1e-5,
              max_grad_norm=0.5, use_clipped_value_loss=True)
NO_CLIP = 1e9
PARITY = {}     # measured per-block errors, written by the last test (profiles/gru_discrete_parity.json)
DISTS = (ref.CATEGORICAL, ref.BERNOULLI)
ALL = [(d, s) for d in DISTS for s in ref.SHAPES[d]]
_id = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else (ref.DIST_NAME.get(v, str(v)) if isinstance(v, int) else str(v))  # noqa: E731


def npv(t):
    return t.numpy() if hasattr(t, "numpy") else np.asarray(t)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


@functools.lru_cache(maxsize=None)
def _case(dist, shape, dead_env=None):
    return ref.random_case(dist, *shape, dead_env=dead_env)


@functools.lru_cache(maxsize=None)
def _admitted(dist, shape, algo, use_clipped=True, dead_env=None):
    """the float64 gradient and losses of a case, computed once; a case counts only where float32 torch stays within half the bound"""
    g64, l64, worst32 = ref.admit(_case(dist, shape, dead_env), algo, use_clipped)
    assert worst32 <= 0.5 * ref.RTOL_BLOCK, f"{ref.tag(dist, shape)} {algo}: the float32 evaluation is {worst32:.2e} from float64: not a case"
    if algo == "ppo":       # rows in all three branches of the clipped surrogate, on the float64 side
        lo, mid, hi, margin = ref.surrogate_branches(_case(dist, shape, dead_env))
        assert lo >= 2 and mid >= 2 and hi >= 2 and margin > 1e-4, (lo, mid, hi, margin)
    return g64, l64, worst32


def _policy(sg, c, params=None, **kw):
    p = sg.Policy((c["O"],), ref.dr.space(c["dist"], c["K"]), base_kwargs={"recurrent": True, "hidden_size": c["H"]}, recurrent_heads=True, **kw)
    p.set_flat_params(np.asarray(c["params"] if params is None else params, np.float32))
    return p


def _rollout(sg, c, resident=False):
    ro = sg.RolloutStorage(c["T"], c["N"], (c["O"],), ref.dr.space(c["dist"], c["K"]), c["H"], 1)
    for name in ("obs", "actions", "returns", "masks", "value_preds", "action_log_probs"):
        t = getattr(ro, name)
        t.copy_(t.new_tensor(np.asarray(c[name], np.int64 if str(t.dtype).endswith("int64") else np.float32)))
    ro.recurrent_hidden_states[0].copy_(ro.obs.new_tensor(np.asarray(c["hxs0"], np.float32)))
    if resident:
        ro.sync_to_device()
        ro.device_resident = True
        ro.enable_device_hidden()
    return ro


def _a2c(sg, p, **over):
    m = dict(A2C_HP, **over)
    return sg.algo.A2C_ACKTR(p, m["value_loss_coef"], m["entropy_coef"], lr=m["lr"], eps=m["eps"], alpha=m["alpha"],
                             max_grad_norm=m["max_grad_norm"], recurrent=True)


def _ppo(sg, p, **over):
    m = dict(PPO_HP, **over)
    return sg.algo.PPO(p, m["clip_param"], m["ppo_epoch"], m["num_mini_batch"], m["value_loss_coef"], m["entropy_coef"], lr=m["lr"],
                       eps=m["eps"], max_grad_norm=m["max_grad_norm"], use_clipped_value_loss=m["use_clipped_value_loss"])


def _run(sg, c, algo, updates=1, resident=False, perms=None, **over):
    """-> (agent, policy, [losses per update]) after `updates` updates on the case's rollout"""
    p = _policy(sg, c)
    ro = _rollout(sg, c, resident)
    if algo == "a2c":
        agent = _a2c(sg, p, **over)
        return agent, p, [agent.update(ro) for _ in range(updates)]
    agent = _ppo(sg, p, **over)
    E = dict(PPO_HP, **over)["ppo_epoch"]
    perms = np.tile(np.arange(c["N"], dtype=np.int64), (E, 1)) if perms is None else perms
    return agent, p, [agent.update(ro, perms=perms) for _ in range(updates)]


def _gradient(sg, c, algo, **over):
    agent, p, losses = _run(sg, c, algo, max_grad_norm=NO_CLIP, **over)
    if algo == "a2c":
        sq, step = agent.get_rmsprop()
        assert step == 1
        oma = float(np.float32(1.0 - A2C_HP["alpha"]))     # the float the kernel multiplies g^2 by
        got = np.sign(np.asarray(c["params"], np.float64) - p.get_flat_params().astype(np.float64)) * np.sqrt(sq.astype(np.float64) / oma)
    else:
        mm, _, step = agent.get_adam()
        assert step == 1
        got = mm.astype(np.float64) / float(np.float32(1.0) - np.float32(0.9))
    return got, losses[0]


def _hold(sg, dist, shape, algo, label="", use_clipped=True, dead_env=None, **over):
    g64, l64, worst32 = _admitted(dist, shape, algo, use_clipped, dead_env)
    c = _case(dist, shape, dead_env)
    if algo == "ppo":
        over = dict(over, use_clipped_value_loss=use_clipped)
    got, losses = _gradient(sg, c, algo, **over)
    errs = ref.block_errors(got, g64, c["O"], c["K"], c["H"])
    tag = ref.tag(dist, shape, f"{algo}{'' if use_clipped else ' plain'}{' ' + label if label else ''}")
    PARITY[tag] = dict(worst_block=max(errs, key=errs.get), worst=max(errs.values()), float32_torch=worst32, blocks=errs)
    print(f"{tag}: worst block {PARITY[tag]['worst_block']} {PARITY[tag]['worst']:.3e} (float32 torch {worst32:.3e})")
    assert max(errs.values()) <= ref.RTOL_BLOCK, (tag, {k: v for k, v in errs.items() if v > ref.RTOL_BLOCK})
    assert_close(losses, l64, what=f"{tag} losses")


# ------------------------------------------------------------------------------------------- 1. gradient per block vs the arbiter
@pytest.mark.parametrize("rows", [16, 32])
@pytest.mark.parametrize("dist,shape", ALL, ids=_id)
def test_ppo_gradient_per_block(sg, monkeypatch, dist, shape, rows):
    monkeypatch.setenv("SG_PPO_ROWS", str(rows))
    _hold(sg, dist, shape, "ppo", f"{rows}-row groups")


@pytest.mark.parametrize("dist,shape", [(d, s) for d in DISTS for s in ref.UNCLIPPED], ids=_id)
def test_ppo_gradient_with_the_unclipped_value_loss(sg, dist, shape):
    _hold(sg, dist, shape, "ppo", use_clipped=False)


@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_ppo_gradient_32_row_groups_on_four_waves(sg, monkeypatch, dist):
    monkeypatch.setenv("SG_PPO_ROWS", "32")
    monkeypatch.setenv("SG_PPO_WAVES", "4")
    _hold(sg, dist, (47, 18, 64, 8, 17), "ppo", "32-row groups, SG_PPO_WAVES=4")


@pytest.mark.parametrize("dist,shape", ALL, ids=_id)
def test_a2c_gradient_per_block(sg, dist, shape):
    _hold(sg, dist, shape, "a2c")


@pytest.mark.parametrize("algo,rows", [("ppo", 16), ("ppo", 32), ("a2c", 0)])
@pytest.mark.parametrize("dist,shape", [(d, s) for d in DISTS for s in ref.GW_SHAPES[d]] + [(ref.BERNOULLI, (13, 33, 20, 9, 33))], ids=_id)
def test_gradient_on_the_global_weight_instances(sg, monkeypatch, dist, shape, algo, rows):
    monkeypatch.setenv("SG_POLICY_GW", "1")
    if rows:
        monkeypatch.setenv("SG_PPO_ROWS", str(rows))
    _hold(sg, dist, shape, algo, "SG_POLICY_GW=1" + (f" {rows}-row groups" if rows else ""))


@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_a2c_gradient_in_three_groups_of_16_environments(sg, monkeypatch, dist):
    """(11, 17, 16, 27, 48) with the group size forced to 16: three groups through both accumulate paths, 1 / B stays 1 / (T N)"""
    monkeypatch.setenv("SG_A2C_GROUP_ENVS", "16")
    _hold(sg, dist, (11, 17, 16, 27, 48), "a2c", "groups of 16")


@pytest.mark.parametrize("dist,shape", [(ref.CATEGORICAL, (13, 130, 20, 9, 33)), (ref.BERNOULLI, (13, 33, 20, 9, 33))], ids=_id)
def test_a2c_gradient_ragged_last_group(sg, monkeypatch, dist, shape):
    """N = 33 in groups of 16: the last group is one environment"""
    monkeypatch.setenv("SG_A2C_GROUP_ENVS", "16")
    _hold(sg, dist, shape, "a2c", "groups of 16")


# ------------------------------------------------------------------------------------------- 2. an environment that never leaves its reset
@pytest.mark.parametrize("algo", ["ppo", "a2c"])
@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_gradient_with_an_environment_that_never_leaves_its_reset(sg, dist, algo):
    shape, env = ref.DEAD_ENV_CASE
    assert (_case(dist, shape, env)["masks"][:, env] == 0).all()
    _hold(sg, dist, shape, algo, f"masks of environment {env} all 0", dead_env=env)


# ------------------------------------------------------------------------------------------- 3. composition, bit for bit
def _composition_case(dist, O, K, H, n):
    """One step of n environments with parameters whose mode does not hang on rounding: the first of a fixed list of seeds whose
    float64 logits keep the top two classes (Bernoulli: every logit and 0) more than 1e-3 apart -> (case, that gap)"""
    c = dict(ref.random_case(dist, O, K, H, 1, n, seed=3))
    for seed in range(7, 40):
        c["params"] = ref.init_params(O, K, H, seed)
        z = ref.evaluate(c)[3]
        gap = float((np.sort(z, 1)[:, -1] - np.sort(z, 1)[:, -2]).min() if dist == ref.CATEGORICAL else np.abs(z).min())
        if gap > 1e-3:
            break
    return c, gap


@pytest.mark.parametrize("n", [1, 16, 17, 77])
@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_composition_with_the_gaussian_and_the_feed_forward_twin(sg, dist, n):
    """act (injected uniform draws, and deterministic) and evaluate_actions of the new policy: hxs_out is the Gaussian recurrent
    twin's (same GRU tensors), value / action / log-prob / entropy are the feed-forward discrete twin's (obs_dim = H, same heads)
    fed that hxs_out -- the same bits: the GRU launches and the heads' forward launch are shared."""
    O, K, H = 13, 6, 20
    c, gap = _composition_case(dist, O, K, H, n)
    assert gap > 1e-3, gap      # the deterministic rows must not hang on rounding: checked on the float64 side
    ng = ref.gru_count(O, K, H)
    p = _policy(sg, c)
    A_g = 3
    gauss = sg.Policy((O,), ref.dr.Box((A_g,)), base_kwargs={"recurrent": True, "hidden_size": H})
    fg = gauss.get_flat_params()
    fg[:ng] = c["params"][:ng]
    gauss.set_flat_params(fg)
    ff = sg.Policy((H,), ref.dr.space(dist, K), base_kwargs={"hidden_size": H})
    ff.set_flat_params(c["params"][ng:])
    obs, masks, hxs = c["obs"][0], c["masks"][0], c["hxs0"]
    rng = np.random.default_rng(n)
    u = rng.random((n, c["A"])).astype(np.float32)
    h_twin = npv(gauss.act(obs, hxs, masks, deterministic=True)[3])
    for kw in (dict(noise=u), dict(deterministic=True)):
        v, a, lp, h = p.act(obs, hxs, masks, **kw)
        assert np.array_equal(npv(h), h_twin)
        v2, a2, lp2, _ = ff.act(h_twin, None, None, **kw)
        assert npv(a).dtype == npv(a2).dtype and npv(a).dtype == (np.int64 if dist == ref.CATEGORICAL else np.float32)
        assert np.array_equal(npv(v), npv(v2)) and np.array_equal(npv(a), npv(a2)) and np.array_equal(npv(lp), npv(lp2))
    assert np.array_equal(npv(p.get_value(obs, hxs, masks)), npv(ff.get_value(h_twin, None, None)))
    acts = c["actions"][0]
    v, lp, ent, h = p.evaluate_actions(obs, hxs, masks, acts)
    v2, lp2, ent2, _ = ff.evaluate_actions(h_twin, None, None, acts)
    assert np.array_equal(npv(h), h_twin)
    assert np.array_equal(npv(v), npv(v2)) and np.array_equal(npv(lp), npv(lp2)) and float(ent) == float(ent2)


# ------------------------------------------------------------------------------------------- 4. evaluate_actions over a sequence
@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_evaluate_actions_over_a_sequence(sg, dist):
    """T = 9, N = 33 with sequences cut at t = 0, mid-sequence and t = T - 1: value, log-prob, entropy against the arbiter's forward"""
    T, N = 9, 33
    c = dict(ref.random_case(dist, 13, 17, 20, T, N, seed=4))
    masks = np.ones((T + 1, N, 1), np.float32)
    masks[0, 3], masks[T // 2, 7], masks[T - 1, 32], masks[T // 2, 16], masks[0, 16] = 0.0, 0.0, 0.0, 0.0, 0.0
    c["masks"] = masks
    v64, lp64, ent64, _, x64 = ref.evaluate(c)
    p = _policy(sg, c)
    B = T * N
    v, lp, ent, h = p.evaluate_actions(c["obs"][:T].reshape(B, -1), c["hxs0"], masks[:T].reshape(B, 1), c["actions"].reshape(B, -1))
    for what, got, want in (("value", npv(v), v64), ("logp", npv(lp), lp64), ("entropy", float(ent), ent64.mean()),
                            ("rnn_hxs", npv(h), x64[(T - 1) * N:])):
        assert_close(got, want, what=what)
        assert relerr(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)) <= 1e-4, what
    # stepping the same rows through act() carries the same states (the sequence and the steps share the scan)
    hs = c["hxs0"]
    for t in range(T):
        hs = npv(p.act(c["obs"][t], hs, masks[t], deterministic=True)[3])
    assert np.array_equal(hs, npv(h))


# ------------------------------------------------------------------------------------------- 5. whole updates against reference fixtures
def _fixture_problem(sg, g, resident=False):
    m = g["meta"]
    dist = ref.CATEGORICAL if m["dist"] == "cat" else ref.BERNOULLI
    c = dict(dist=dist, O=m["O"], K=m["K"], H=m["H"], T=m["T"], N=m["N"], A=1 if dist == ref.CATEGORICAL else m["K"], params=g["params0"],
             hxs0=g["hxs0"], **{k: g[k] for k in ("obs", "actions", "returns", "masks", "value_preds", "action_log_probs")})
    assert m["names"] == [n for n, _ in ref.param_shapes(m["O"], m["K"], m["H"])]
    return c, _policy(sg, c), _rollout(sg, c, resident)


@pytest.mark.parametrize("name", ["gru_cat_ppo", "gru_ber_ppo"])
def test_ppo_update_matches_the_reference_fixture(sg, name):
    g = load(name)
    m = g["meta"]
    c, p, ro = _fixture_problem(sg, g)
    agent = _ppo(sg, p, **{k: m[k] for k in PPO_HP if k in m})
    losses = agent.update(ro, perms=g["perms"])
    assert np.array_equal(agent.last_perms(), g["perms"]) and g["perms"].shape == (m["ppo_epoch"], m["N"])
    assert_close(ro.device_advantages(), g["advantages"], rtol=1e-5, what="advantages")
    assert_close(losses, g["losses"], what="ppo losses")
    mm, vv, step = agent.get_adam()
    assert step == m["steps"] == 4
    assert_close(mm, g["adam_m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert_close(vv, g["adam_v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close_adam(p.get_flat_params(), g["params1"], m["lr"], m["steps"], what="params after the update")


@pytest.mark.parametrize("name", ["gru_cat_a2c", "gru_ber_a2c"])
def test_a2c_update_matches_the_reference_fixture(sg, name):
    g = load(name)
    m = g["meta"]
    c, p, ro = _fixture_problem(sg, g)
    assert m["grad_norms"][0] > m["max_grad_norm"]      # the clip is active
    agent = _a2c(sg, p, **{k: m[k] for k in A2C_HP})
    losses = agent.update(ro)
    assert_close(losses, g["losses"], what="a2c losses")
    sq, step = agent.get_rmsprop()
    assert step == 1
    assert_close(sq, g["square_avg"], rtol=1e-3, atol=1e-12, what="square_avg")
    assert_close(p.get_flat_params(), g["params1"], what="params after the update")


def test_reference_checkpoint_loads_and_acts(sg):
    from simgan_amd.checkpoint import RECURRENT_SAVE_MSG, load_policy, save_policy
    g = load("ckpt_policy_gru_cat")
    pol, rms = load_policy(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ckpt_policy_gru_cat.pt"))
    assert pol.is_recurrent and pol.dist_kind == ref.CATEGORICAL and np.array_equal(pol.get_flat_params(), g["flat"])
    v, a, lp, h = pol.act(g["obs"], g["hxs"], g["masks"], deterministic=True)
    assert np.array_equal(npv(a), g["action"]) and npv(a).dtype == np.int64
    for what, got, want in (("value", v, g["value"]), ("logp", lp, g["logp"]), ("hxs", h, g["hxs_out"])):
        assert_close(npv(got), want, what=what)
    with pytest.raises(NotImplementedError) as e:
        save_policy("/nonexistent/never_written.pt", pol)
    assert str(e.value) == RECURRENT_SAVE_MSG


# ------------------------------------------------------------------------------------------- 6. determinism and forms
@pytest.mark.parametrize("algo", ["ppo", "a2c"])
@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_same_bits_twice_directly_launched_and_device_resident(sg, monkeypatch, dist, algo):
    c = _case(dist, (11, 17, 16, 27, 48))
    over = dict(ppo_epoch=2, num_mini_batch=3) if algo == "ppo" else {}
    perms = np.stack([np.random.default_rng(e).permutation(c["N"]) for e in range(2)]).astype(np.int64) if algo == "ppo" else None

    def run(resident=False):
        agent, p, losses = _run(sg, c, algo, updates=2, resident=resident, perms=perms, **over)
        state = agent.get_adam() if algo == "ppo" else agent.get_rmsprop()
        return losses, p.get_flat_params(), [np.asarray(s) for s in state]

    a, b, r = run(), run(), run(resident=True)
    monkeypatch.setenv("SG_PPO_GRAPH", "0")
    d = run()
    for other in (b, r, d):
        assert [tuple(np.asarray(x).tolist()) for x in a[0]] == [tuple(np.asarray(x).tolist()) for x in other[0]]
        assert np.array_equal(a[1], other[1]) and all(np.array_equal(x, y) for x, y in zip(a[2], other[2]))
    assert np.isfinite(a[1]).all()


def test_a_gaussian_and_a_categorical_agent_of_equal_shapes_keep_their_own_graphs(sg):
    """Same O, H, T, N and action width 1, one context, updates interleaved: the graph key carries the distribution"""
    c = _case(ref.CATEGORICAL, (11, 3, 16, 5, 4))
    alone = _run(sg, c, "ppo", updates=2)[1].get_flat_params()
    p = _policy(sg, c)
    agent, ro = _ppo(sg, p), _rollout(sg, c)
    pg = sg.Policy((c["O"],), ref.dr.Box((1,)), base_kwargs={"recurrent": True, "hidden_size": c["H"]})
    rg = sg.RolloutStorage(c["T"], c["N"], (c["O"],), ref.dr.Box((1,)), c["H"], 1)
    for name in ("obs", "returns", "masks", "value_preds", "action_log_probs"):
        getattr(rg, name).copy_(getattr(rg, name).new_tensor(np.asarray(c[name], np.float32)))
    ag = _ppo(sg, pg)
    perms = np.arange(c["N"], dtype=np.int64)[None]
    for _ in range(2):
        agent.update(ro, perms=perms)
        assert np.isfinite(ag.update(rg, perms=perms)).all()
    assert np.array_equal(p.get_flat_params(), alone)


@pytest.mark.parametrize("algo", ["ppo", "a2c"])
def test_queued_update_through_the_learner_matches_the_synchronous_call(sg, algo):
    """driver.PpoLearner on a device-resident rollout that holds its hidden states: the update is queued, its losses come through the
    results ring; against the same calls made synchronously (after_update, the recurrent compute_returns_policy and the hand-over
    of hidden slot 0 included).  The host-rollout mode runs too."""
    from simgan_amd import _lib
    from simgan_amd.driver import PpoLearner
    c = _case(ref.CATEGORICAL, (11, 3, 32, 8, 17), 5)
    rewards = np.random.default_rng(5).standard_normal((c["T"], c["N"], 1)).astype(np.float32)
    hx = np.random.default_rng(6).standard_normal((c["T"] + 1, c["N"], c["H"])).astype(np.float32) * 0.5

    def setup(resident):
        p = _policy(sg, c)
        agent = _a2c(sg, p) if algo == "a2c" else _ppo(sg, p, ppo_epoch=2, num_mini_batch=1)
        ro = _rollout(sg, c)
        ro.rewards.copy_(ro.rewards.new_tensor(rewards))
        ro.recurrent_hidden_states.copy_(ro.obs.new_tensor(hx))
        if resident:
            ro.sync_to_device()
            ro.device_resident = True
            ro.enable_device_hidden()
        return p, agent, ro

    p1, a1, r1 = setup(True)
    learner = PpoLearner(p1, a1, r1)
    pending = [learner.update() for _ in range(2)]
    ring = [(float(q["value_loss"]), float(q["action_loss"]), float(q["dist_entropy"])) for q in pending]
    p2, a2, r2 = setup(True)      # (PPO: both agents draw the same environment permutations from the same seed)
    sync = []
    for j in range(2):
        _lib.check(r2.lib.sg_rollout_compute_returns_policy(r2.h, p2.h, 1, 0.99, 0.95, 1))
        sync.append(tuple(float(x) for x in (a2.update(r2))))
        r2.after_update()
    assert ring == sync
    assert np.array_equal(p1.get_flat_params(), p2.get_flat_params())
    p3, a3, r3 = setup(False)
    host = PpoLearner(p3, a3, r3).update()
    assert all(np.isfinite(float(host[k])) for k in ("value_loss", "action_loss", "dist_entropy"))


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_learner_iterations_collect_through_policy_act(sg, dist, resident):
    """collect() acts through Policy.act (int64 class indices / 0-1 bits into the rollout, the hidden state carried), update() runs
    PPO through time; after_update carries the last state into slot 0."""
    from simgan_amd.driver import PpoLearner
    rng = np.random.default_rng(9)
    O, K, H, T, N = 11, 5, 32, 6, 8
    seen = []

    class Envs:
        def step(self, action):
            seen.append(npv(action).copy())
            done = rng.random(N) < 0.1
            return (rng.standard_normal((N, O)).astype(np.float32), rng.standard_normal((N, 1)).astype(np.float32), done, [{} for _ in range(N)])

    p = sg.Policy((O,), ref.dr.space(dist, K), base_kwargs={"recurrent": True, "hidden_size": H}, recurrent_heads=True, seed=2)
    ro = sg.RolloutStorage(T, N, (O,), ref.dr.space(dist, K), p.recurrent_hidden_state_size, O)
    ro.obs[0].copy_(ro.obs.new_tensor(rng.standard_normal((N, O)).astype(np.float32)))
    ro.device_resident = resident
    agent = sg.algo.PPO(p, 0.2, 2, 4, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5, seed=5)
    learner = PpoLearner(p, agent, ro)
    for _ in range(2):
        learner.collect(Envs())
        last = npv(ro.recurrent_hidden_states)[-1].copy()
        assert np.abs(last).max() > 0
        out = learner.update()
        out = out.resolve() if hasattr(out, "resolve") else out
        assert all(np.isfinite(float(out[k])) for k in ("value_loss", "action_loss", "dist_entropy"))
        assert np.array_equal(npv(ro.recurrent_hidden_states)[0], last)
    assert agent.get_adam()[2] == 2 * 2 * 4
    a = np.concatenate(seen)
    if dist == ref.CATEGORICAL:
        assert a.dtype == np.int64 and a.min() >= 0 and a.max() < K and len(np.unique(a)) > 1
    else:
        assert set(np.unique(a)) == {0.0, 1.0}


def _adam_step(p, m, v, g, t, lr, eps):
    m, v = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
    return p - lr * (m / (1 - 0.9 ** t)) / (np.sqrt(v / (1 - 0.999 ** t)) + eps), m, v


@pytest.mark.parametrize("algo", ["ppo", "a2c"])
@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_three_consecutive_updates(sg, dist, algo):
    """Three updates (the clip at 0.5 active) against the trajectory of the arbiter's float32 torch gradients stepped by the
    optimizer's own rule (torch.optim.Adam / RMSprop: no weight decay, no momentum), carried in float64"""
    import torch
    c = dict(_case(dist, (11, 3, 32, 8, 17), 5))
    agent, p, losses = _run(sg, c, algo, updates=3)
    params = np.asarray(c["params"], np.float64)
    m = v = sq = np.zeros_like(params)
    for j in range(3):
        cj = dict(c, params=params.astype(np.float32))
        g, l = (ref.ppo_grad(cj, dtype=torch.float32) if algo == "ppo" else ref.a2c_grad(cj, dtype=torch.float32))
        assert_close(losses[j], l, what=f"losses {j}")
        gc = g * min(1.0, 0.5 / (np.sqrt((g * g).sum()) + 1e-6))
        if algo == "ppo":
            params, m, v = _adam_step(params, m, v, gc, j + 1, PPO_HP["lr"], PPO_HP["eps"])
        else:
            sq = A2C_HP["alpha"] * sq + (1.0 - A2C_HP["alpha"]) * gc * gc
            params = params - A2C_HP["lr"] * gc / (np.sqrt(sq) + A2C_HP["eps"])
    if algo == "ppo":
        mm, vv, step = agent.get_adam()
        assert step == 3
        assert_close(mm, m, rtol=1e-3, atol=1e-7, what="adam m")
        assert_close(vv, v, rtol=1e-3, atol=1e-10, what="adam v")
        assert_close_adam(p.get_flat_params(), params, PPO_HP["lr"], 3, what="params after three updates")
    else:
        got_sq, step = agent.get_rmsprop()
        assert step == 3
        assert_close(got_sq, sq, rtol=1e-3, atol=1e-12, what="square_avg after three updates")
        assert_close(p.get_flat_params(), params, what="params after three updates")


def test_optimizer_state_round_trips_with_the_gru_tensors_first(sg):
    from simgan_amd import _lib
    c = _case(ref.CATEGORICAL, (13, 2, 100, 8, 17))      # padded Hp: the GRU block's pad / unpad
    n = c["params"].size
    ng = ref.gru_count(c["O"], c["K"], c["H"])
    state = np.arange(1, n + 1, dtype=np.float32) * 1e-6
    agent, p, _ = _run(sg, c, "a2c")
    assert p.num_params == n
    agent.set_rmsprop(state, 7)
    back, step = agent.get_rmsprop()
    assert step == 7 and np.array_equal(back, state)
    with pytest.raises(_lib.SimganHipError, match="bad length"):
        agent.set_rmsprop(state[ng:], 7)
    agent, p, _ = _run(sg, c, "ppo")
    agent.set_adam(state, 2 * state, 5)
    m2, v2, s2 = agent.get_adam()
    assert s2 == 5 and np.array_equal(m2, state) and np.array_equal(v2, 2 * state)
    # the flat order: a gradient that lives in the GRU block alone shows up in the first gru_count entries of Adam's m
    sd = p.state_dict()
    assert list(sd)[:4] == list(ref.GRU_NAMES) and list(sd)[-2:] == ["dist.linear.weight", "dist.linear.bias"]


# ------------------------------------------------------------------------------------------- 7. both sides of the gradient clip
@pytest.mark.parametrize("algo", ["ppo", "a2c"])
@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_both_sides_of_the_clip(sg, dist, algo):
    shape = (13, 130, 20, 9, 33) if dist == ref.CATEGORICAL else (13, 33, 20, 9, 33)
    g64, _, _ = _admitted(dist, shape, algo)
    c = _case(dist, shape)
    norm = float(np.sqrt((g64 * g64).sum()))
    heads = float(np.sqrt((g64[ref.gru_count(c["O"], c["K"], c["H"]):] ** 2).sum()))
    assert heads < 0.98 * norm      # a norm over the heads alone would give another coefficient below, beyond the tolerance
    for mgn in (0.5 * norm, 2.0 * norm):
        gc = g64 * min(1.0, mgn / (norm + 1e-6))
        agent, p, _ = _run(sg, c, algo, max_grad_norm=mgn)
        if algo == "ppo":
            mm, vv, _ = agent.get_adam()
            assert_close(mm, 0.1 * gc, rtol=1e-3, atol=1e-7, what=f"adam m at max_grad_norm {mgn:.3f} (norm {norm:.3f})")
            assert_close(vv, 0.001 * gc * gc, rtol=1e-3, atol=1e-10, what="adam v")
        else:
            sq, _ = agent.get_rmsprop()
            want = (1.0 - A2C_HP["alpha"]) * gc * gc
            assert_close(sq, want, rtol=1e-3, atol=1e-12, what=f"square_avg at max_grad_norm {mgn:.3f} (norm {norm:.3f})")
            assert_close(p.get_flat_params(), np.asarray(c["params"], np.float64) - A2C_HP["lr"] * gc / (np.sqrt(want) + A2C_HP["eps"]),
                         what="params")


# ------------------------------------------------------------------------------------------- 8. diagnostics
@pytest.mark.parametrize("dist", DISTS, ids=_id)
def test_diagnostics_against_the_float64_reference(sg, dist):
    c = _case(dist, (11, 17, 16, 27, 48))
    v, lp, ent, _, _ = ref.evaluate(c)
    B = c["T"] * c["N"]
    rows = (c["action_log_probs"].reshape(B).astype(np.float64), c["value_preds"][:c["T"]].reshape(B).astype(np.float64),
            c["returns"][:c["T"]].reshape(B).astype(np.float64))
    r = np.exp(lp - rows[0])
    assert np.min(np.abs(np.abs(r - 1.0) - ref.CLIP)) >= dg.EDGE * ref.CLIP and 0.1 <= (np.abs(r - 1.0) > ref.CLIP).mean() <= 0.9
    want, allow = dg.statistics(lp, ent, v, *rows, ref.CLIP), dg.allowances(lp, ent, v, *rows, ref.CLIP)
    p = _policy(sg, c)
    for resident in (False, True):
        got = _ppo(sg, p).diagnostics(_rollout(sg, c, resident))
        d = dg.compare(got, want, allow)
        assert max(d.values()) <= 1.0, {k: x for k, x in d.items() if x > 1.0}
    d_a2c = _a2c(sg, p).diagnostics(_rollout(sg, c))
    d_ppo = sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5).diagnostics(_rollout(sg, c))
    assert d_a2c["clip_fraction"] == 0.0 and d_a2c["rows"] == B and set(d_a2c) == set(d_ppo)
    for k in d_a2c:
        if k != "clip_fraction":
            np.testing.assert_equal(d_a2c[k], d_ppo[k], err_msg=k)


# ------------------------------------------------------------------------------------------- 9. refusals
def test_refusals_at_the_c_level_and_through_python(sg):
    from simgan_amd import _lib
    from simgan_amd.ensemble import PolicyEnsemble
    from test_gpu_world import run_ranks
    c = _case(ref.CATEGORICAL, (11, 3, 16, 5, 4))
    p = _policy(sg, c)
    lib, h = p.lib, _lib.H()
    # the constructor's entry points
    with pytest.raises(_lib.SimganHipError, match="feed-forward Policy"):
        _lib.check(lib.sg_policy_create3(p.ctx.h, _lib.POLICY_GRU, 4, 1, 8, 1, 0, 1, 5, C.byref(h)))
    with pytest.raises(_lib.SimganHipError, match="sg_policy_create_rnn_dist: dist 0"):
        _lib.check(lib.sg_policy_create_rnn_dist(p.ctx.h, 4, 8, 0, 0, 5, C.byref(h)))
    with pytest.raises(_lib.SimganHipError, match="2\\^24"):
        _lib.check(lib.sg_policy_create_rnn_dist(p.ctx.h, 4, 8, 0, 1, 1 << 24, C.byref(h)))
    with pytest.raises(NotImplementedError, match="the GRU base is built with the Gaussian head"):
        sg.Policy((4,), ref.dr.Discrete(3), base_kwargs={"recurrent": True, "hidden_size": 8})
    # the feed-forward entry points, ACKTR, the symmetry loss, the ensemble
    obs = np.zeros((2, c["O"]), np.float32)
    out = np.zeros((2, 1), np.float32)
    with pytest.raises(_lib.SimganHipError, match="this policy is recurrent"):
        _lib.check(lib.sg_policy_act(p.h, _lib.fptr(obs), 2, None, 0, 1, _lib.fptr(out), _lib.fptr(out.copy()), _lib.fptr(out.copy())))
    cfg = _lib.ACKTRConfig(0.5, 0.01, 0.25, 0.9, 0.99, 0.001, 1e-2, 10)
    with pytest.raises(_lib.SimganHipError, match="ACKTR is not defined for a recurrent Policy"):
        _lib.check(lib.sg_acktr_create(p.ctx.h, p.h, C.byref(cfg), C.byref(h)))
    with pytest.raises(NotImplementedError, match="ACKTR is not built for a recurrent Policy on a Discrete / MultiBinary"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=True, recurrent=True)
    with pytest.raises(NotImplementedError, match="A2C through time is opt-in"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    acfg = _lib.A2CConfig(0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5)
    with pytest.raises(_lib.SimganHipError, match="sg_a2c_create: A2C is implemented for feed-forward policies only"):
        _lib.check(lib.sg_a2c_create(p.ctx.h, p.h, C.byref(acfg), C.byref(h)))
    agent = _ppo(sg, p)
    m1 = np.eye(1, dtype=np.float32)
    with pytest.raises(_lib.SimganHipError, match="sg_ppo_set_symmetry"):
        _lib.check(lib.sg_ppo_set_symmetry(agent.h, 1.0, _lib.fptr(np.eye(c["O"], dtype=np.float32)), _lib.fptr(m1)))
    with pytest.raises(NotImplementedError, match="mirror-symmetry loss: not for a recurrent Policy on a Discrete / MultiBinary"):
        sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.0, symmetry_coef=1.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5, mirror_obs=np.eye(c["O"]), mirror_act=m1)
    with pytest.raises(NotImplementedError, match="PolicyEnsemble: a recurrent member on a Discrete / MultiBinary action space"):
        PolicyEnsemble([p])
    # on-device collection: the act kernels carry the Gaussian head
    ro = _rollout(sg, c, resident=True)
    act = np.zeros((c["N"], 1), np.float32)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_act_step_rnn: the recurrent policy has a Categorical head"):
        _lib.check(lib.sg_rollout_act_step_rnn(ro.h, p.h, 0, _lib.fptr(np.ascontiguousarray(c["obs"][0])), _lib.fptr(np.ascontiguousarray(c["masks"][0])),
                                               None, 0, 1, _lib.fptr(act)))
    with pytest.raises(NotImplementedError, match="act_step: a recurrent policy on a Discrete / MultiBinary action space"):
        ro.act_step(p)
    with pytest.raises(ValueError, match="the chained step takes a feed-forward learner"):
        ro._chain_inner("act_step_chain", p, [], True, None, None, None, None, None)
    from simgan_amd.driver import PpoLearner
    with pytest.raises(ValueError, match="collect\\(on_device=True\\): the policy is recurrent with a Discrete / MultiBinary"):
        PpoLearner(p, agent, ro).collect(None, on_device=True)
    with pytest.raises(NotImplementedError, match="mirrors actions through a linear map"):
        _rollout(sg, _case(ref.CATEGORICAL, (11, 3, 16, 1, 16))).enable_dup_sym(np.eye(c["O"]), np.eye(1))
    with pytest.raises(NotImplementedError, match="the CNN base is built feed-forward only"):
        sg.Policy((4, 84, 84), ref.dr.Discrete(6), base_kwargs={"recurrent": True}, recurrent_heads=True)
    with pytest.raises(ValueError, match="no log-std to reset"):
        p.reset_variance(ref.dr.Discrete(3), -1.0)
    # a hidden-state hand-over is needed before every update
    with pytest.raises(_lib.SimganHipError, match="sg_ppo_set_hidden_states must hand over"):
        _lib.check(agent.lib.sg_ppo_update(agent.h, ro.h, None, 0, 0, (C.c_float * 3)()))

    def body(rank, ctx):
        q = sg.Policy((6,), ref.dr.Discrete(3), base_kwargs={"recurrent": True, "hidden_size": 16}, ctx=ctx, recurrent_heads=True)
        msgs = []
        for make in (lambda: sg.algo.PPO(q, 0.2, 1, 1, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5),
                     lambda: sg.algo.A2C_ACKTR(q, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, recurrent=True)):
            try:
                make()
                msgs.append(None)
            except (_lib.SimganHipError, NotImplementedError) as exc:
                msgs.append(str(exc))
        return msgs

    for msgs in run_ranks(2, body):
        assert msgs[0] is not None and "runs on one rank" in msgs[0] and "world 2" in msgs[0], msgs
        assert msgs[1] is not None and "sg_a2c_create_rnn" in msgs[1] and "world 2" in msgs[1], msgs


@pytest.mark.parametrize("algo", ["ppo", "a2c"])
def test_a_head_too_wide_for_lds_beside_w1_takes_the_global_weight_instance(sg, algo):
    """K = 400 at H = 64: the actor trunk (36 K floats) and the forward's row tiles still fit a CU's 160 KB LDS, the fused
    backward's tile set beside them does not -- the launcher takes the global-weight instance by itself (no SG_POLICY_GW)"""
    assert "SG_POLICY_GW" not in os.environ
    _hold(sg, ref.CATEGORICAL, (11, 400, 64, 3, 5), algo, "K = 400")


# ------------------------------------------------------------------------------------------- 10. the record
def test_zz_report_measured_errors():
    """Not a check: writes what the gradient tests of this run measured, in the form of profiles/gru_discrete_parity.json."""
    print("GRU_DISCRETE_PARITY " + json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "blocks"} for k, v in PARITY.items()}))
    if os.environ.get("SG_GRU_DISCRETE_PARITY_OUT"):
        with open(os.environ["SG_GRU_DISCRETE_PARITY_OUT"], "w") as f:
            json.dump(dict(bound=ref.RTOL_BLOCK, measure="max|g_lib - g_f64| / max|g_f64| per parameter block, GRU tensors gate by gate; "
                           "g_f64: torch.float64 autograd of the reference's loss (tests/gru_discrete_ref.py)", cases=PARITY), f, indent=1)
