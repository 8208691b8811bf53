"""GPU: the recurrent Policy (GRU base, a2c/model.py:117-201) -- act / get_value / evaluate_actions through time
(k_gru_inproj, k_gru_scan_fwd, then the feed-forward heads on h_t) and PPO through time (the reverse scan, the GRU's weight
gradients, one clip and one Adam over all parameters) against the reference-written fixtures (tests/golden/policy_gru_*.npz,
ppo_gru_*.npz) and, for forward shapes without a fixture, the float64 restatement of tests/gru_ref.py.
Tolerances are the project's (helpers.RTOL / ATOL)."""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

import gru_ref
from helpers import GOLDEN, assert_close, assert_close_adam, load

pytestmark = pytest.mark.gpu

CASES = ["policy_gru_tiny", "policy_gru_hopper", "policy_gru_laikago"]


class Box:  # duck-typed gym.spaces.Box (a2c/model.py:55-57 reads __class__.__name__ and .shape)
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def npv(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def make(sg, O, A, H, seed=0, **kw):
    return sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": H}, seed=seed, **kw)


def from_fixture(sg, g):
    m = g["meta"]
    p = make(sg, m["O"], m["A"], m["H"])
    p.set_flat_params(g["params"])
    return p


def check_fixture(p, g):
    v, a, lp, h = p.act(g["obs"], g["hxs"], g["masks"], noise=g["noise"])
    assert_close(v, g["act_value"], what="act value")
    assert_close(a, g["act_action"], what="act action")
    assert_close(lp, g["act_logp"], what="act logp")
    assert_close(h, g["act_hxs"], what="act rnn_hxs")
    v, a, lp, h = p.act(g["obs"], g["hxs"], g["masks"], deterministic=True)
    assert_close(a, g["det_action"], what="det action")
    assert_close(lp, g["det_logp"], what="det logp")
    assert_close(h, g["act_hxs"], what="det rnn_hxs")
    assert_close(p.get_value(g["obs"], g["hxs"], g["masks"]), g["get_value"], what="get_value")
    assert (g["seq_masks"] == 0).sum() > 0
    v, lp, ent, h = p.evaluate_actions(g["seq_obs"], g["seq_hxs"], g["seq_masks"], g["seq_action"])
    assert_close(v, g["seq_value"], what="sequence value")
    assert_close(lp, g["seq_logp"], what="sequence logp")
    assert_close(ent, g["seq_entropy"], what="sequence entropy")
    assert_close(h, g["seq_hxs_out"], what="sequence rnn_hxs")


@pytest.mark.parametrize("name", CASES)
def test_policy_gru_golden(sg, name):
    g = load(name)
    p = from_fixture(sg, g)
    assert p.is_recurrent and p.recurrent_hidden_state_size == g["meta"]["H"]
    assert p.num_params == g["params"].size
    assert np.array_equal(p.get_flat_params(), g["params"])   # pad / unpad round trip, GRU block included
    assert [n for n, _ in p.param_shapes()] == g["meta"]["names"]
    check_fixture(p, g)


def test_policy_gru_golden_on_the_global_weight_instances(sg, monkeypatch):
    """SG_POLICY_GW=1: W_ih / W_hh are read through L2 instead of an LDS image (the path of widths that do not fit)."""
    monkeypatch.setenv("SG_POLICY_GW", "1")
    g = load("policy_gru_hopper")
    check_fixture(from_fixture(sg, g), g)


def _random_problem(rng, O, A, H, T, n, p_zero=0.08):
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    masks = (rng.random((T * n, 1)) > p_zero).astype(np.float32)
    masks[(T // 2) * n] = 0.0
    return f(T * n, O), (0.5 * f(n, H)), masks, f(T * n, A)


def _perturbed(sg, rng, O, A, H, **kw):
    p = make(sg, O, A, H, seed=int(rng.integers(1 << 30)), **kw)
    flat = p.get_flat_params()
    p.set_flat_params((flat + 0.05 * rng.standard_normal(flat.size)).astype(np.float32))
    return p


@pytest.mark.parametrize("O,A,H,T,n", [(47, 12, 64, 128, 8),      # the north-star rollout length
                                       (47, 12, 64, 128, 40),     # three 16-environment tiles, the last one ragged
                                       (30, 6, 256, 9, 5),        # hidden 256: W_hh does not fit LDS (global-weight instances)
                                       (13, 5, 20, 7, 19),        # widths that are no multiple of 16
                                       (111, 12, 100, 5, 33)])
def test_sequence_against_the_float64_restatement(sg, O, A, H, T, n):
    rng = np.random.default_rng(O * 1000 + H + T)
    p = _perturbed(sg, rng, O, A, H)
    sd = gru_ref.unflatten(p.get_flat_params(), O, A, H)
    obs, hxs, masks, action = _random_problem(rng, O, A, H, T, n)
    v, lp, ent, h = p.evaluate_actions(obs, hxs, masks, action)
    rv, rlp, rent, rh = gru_ref.evaluate(sd, obs, hxs, masks, action)
    assert_close(v, rv, what="value")
    assert_close(lp, rlp, what="logp")
    assert_close(ent, rent, what="entropy")
    assert_close(h, rh, what="rnn_hxs")
    noise = rng.standard_normal((n, A)).astype(np.float32)
    v, a, lp, h = p.act(obs[:n], hxs, masks[:n], noise=noise)
    rv, ra, rlp, rh = gru_ref.act(sd, obs[:n], hxs, masks[:n], noise)
    assert_close(v, rv, what="act value")
    assert_close(a, ra, what="act action")
    assert_close(lp, rlp, what="act logp")
    assert_close(h, rh, what="act rnn_hxs")


def test_critic_of_its_own_width(sg):
    rng = np.random.default_rng(5)
    O, A, H, T, n = 9, 4, 32, 6, 7
    p = _perturbed(sg, rng, O, A, H, critic_hidden=64)
    assert [s for nm, s in p.param_shapes() if nm == "base.critic.0.weight"] == [(64, H)]
    sd = gru_ref.unflatten(p.get_flat_params(), O, A, H, 64)
    obs, hxs, masks, action = _random_problem(rng, O, A, H, T, n)
    v, lp, _, h = p.evaluate_actions(obs, hxs, masks, action)
    rv, rlp, _, rh = gru_ref.evaluate(sd, obs, hxs, masks, action)
    assert_close(v, rv, what="value")
    assert_close(lp, rlp, what="logp")
    assert_close(h, rh, what="rnn_hxs")


def test_steps_and_sequence_agree_bit_for_bit_and_runs_repeat(sg):
    """The main's act / insert loop through RolloutStorage, then the whole rollout as one sequence: the GRU's arithmetic per
    row is the same in both (fixed summation order, no atomics), so the states are identical bits; two runs are identical in
    everything."""
    g = load("policy_gru_hopper")
    m = g["meta"]
    O, A, H, T, n = m["O"], m["A"], m["H"], m["T"], m["n"]
    p = from_fixture(sg, g)
    ro = sg.RolloutStorage(T, n, (O,), Box((A,)), p.recurrent_hidden_state_size, 1)
    assert tuple(ro.recurrent_hidden_states.shape) == (T + 1, n, H)
    obs = g["seq_obs"].reshape(T, n, O)
    masks = g["seq_masks"].reshape(T, n, 1)
    ro.obs[0].copy_(ro.obs.new_tensor(obs[0]))
    ro.recurrent_hidden_states[0].copy_(ro.obs.new_tensor(g["seq_hxs"]))
    ro.masks[0].copy_(ro.obs.new_tensor(masks[0]))
    rng = np.random.default_rng(1)
    for step in range(T):
        v, a, lp, h = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step], noise=rng.standard_normal((n, A)).astype(np.float32))
        nxt_obs = obs[step + 1] if step + 1 < T else rng.standard_normal((n, O)).astype(np.float32)
        nxt_mask = masks[step + 1] if step + 1 < T else np.ones((n, 1), np.float32)
        ro.insert(ro.obs.new_tensor(nxt_obs), h, a, lp, v, ro.obs.new_tensor(np.zeros((n, 1), np.float32)), ro.obs.new_tensor(nxt_mask),
                  ro.obs.new_tensor(np.ones((n, 1), np.float32)))
    assert_close(npv(ro.recurrent_hidden_states)[1:], g["step_hxs"][1:], what="states along the rollout")
    run = lambda: p.evaluate_actions(npv(ro.obs)[:-1].reshape(-1, O), npv(ro.recurrent_hidden_states)[0], npv(ro.masks)[:-1].reshape(-1, 1),  # noqa: E731
                                     npv(ro.actions).reshape(-1, A))
    v, lp, ent, h = run()
    # the state trajectory has the same bits either way (the GRU kernels sum in one order whatever the row count); the heads
    # pick their row tile by the row count, so values and log-probs agree to rounding
    assert np.array_equal(npv(h), npv(ro.recurrent_hidden_states)[-1]), "sequence state != step-by-step state"
    assert_close(npv(v).reshape(T, n, 1), npv(ro.value_preds)[:-1], what="sequence values vs step-by-step values")
    assert_close(npv(lp).reshape(T, n, 1), npv(ro.action_log_probs), what="sequence logp vs step-by-step logp")
    v2, lp2, ent2, h2 = run()
    assert np.array_equal(npv(v), npv(v2)) and np.array_equal(npv(lp), npv(lp2)) and np.array_equal(npv(h), npv(h2))
    assert float(npv(ent)) == float(npv(ent2))
    # a2c/storage.py:96-101: after_update carries the last state (and mask) into slot 0
    last = npv(ro.recurrent_hidden_states)[-1].copy()
    ro.after_update()
    assert np.array_equal(npv(ro.recurrent_hidden_states)[0], last)
    nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1])
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    assert np.isfinite(npv(ro.returns)).all()
    batches = list(ro.recurrent_generator(npv(ro.returns)[:-1] - npv(ro.value_preds)[:-1], 3))
    assert len(batches) == n // (n // 3) and tuple(batches[0][0].shape) == (T * (n // 3), O) and tuple(batches[0][1].shape) == (n // 3, H)


def test_library_noise_and_masks_reset_the_state(sg):
    rng = np.random.default_rng(3)
    O, A, H, n = 11, 3, 64, 6
    p = _perturbed(sg, rng, O, A, H)
    obs, hxs = rng.standard_normal((n, O)).astype(np.float32), rng.standard_normal((n, H)).astype(np.float32)
    zero, one = np.zeros((n, 1), np.float32), np.ones((n, 1), np.float32)
    v0, a0, lp0, h0 = p.act(obs, hxs, zero, deterministic=True)
    v1, a1, lp1, h1 = p.act(obs, np.zeros_like(hxs), one, deterministic=True)
    assert np.array_equal(npv(h0), npv(h1)) and np.array_equal(npv(v0), npv(v1))   # mask 0 == a zero state
    v2, _, _, h2 = p.act(obs, hxs, one, deterministic=True)
    assert not np.array_equal(npv(h2), npv(h0))
    _, s1, _, _ = p.act(obs, hxs, one)   # library RNG: two calls draw different noise, the state does not depend on it
    _, s2, _, hs = p.act(obs, hxs, one)
    assert not np.array_equal(npv(s1), npv(s2)) and np.array_equal(npv(hs), npv(h2))


def test_init_and_native_pickle(sg):
    p = make(sg, 11, 3, 64, seed=4)
    sd = {k: npv(v) for k, v in p.state_dict().items()}
    for k in ("base.gru.weight_ih_l0", "base.gru.weight_hh_l0"):   # a2c/model.py:126-130: orthogonal, gain 1, on the whole matrix
        w = sd[k].astype(np.float64)
        gram = w.T @ w if w.shape[0] >= w.shape[1] else w @ w.T
        assert_close(gram, np.eye(gram.shape[0]), atol=1e-5, what=k + " orthogonality")
    assert not sd["base.gru.bias_ih_l0"].any() and not sd["base.gru.bias_hh_l0"].any()
    q = pickle.loads(pickle.dumps(p))
    assert q.is_recurrent and q.recurrent_hidden_state_size == 64
    assert np.array_equal(q.get_flat_params(), p.get_flat_params())


def test_reference_checkpoint_of_a_recurrent_policy_loads_and_acts(sg):
    from simgan_amd.checkpoint import load_policy
    from simgan_amd.driver import PpoLearner
    g = load("ckpt_policy_gru")
    path = os.path.join(GOLDEN, "ckpt_policy_gru.pt")
    p, rms = load_policy(path)
    assert p.is_recurrent and np.array_equal(p.get_flat_params(), g["flat"])
    assert_close(rms["var"], g["rms_var"], what="ob_rms var")
    v, a, lp, h = p.act(g["obs"], g["hxs"], g["masks"], deterministic=True)
    assert_close(v, g["value"], what="value")
    assert_close(a, g["action"], what="action")
    assert_close(lp, g["logp"], what="logp")
    assert_close(h, g["hxs_out"], what="rnn_hxs")
    # a2c/main.py:85 resets the critic on every warm start; on a recurrent policy that only works when O == H (a2c/model.py:80-87)
    m = g["meta"]
    with pytest.raises(ValueError, match="obs size == hidden size"):
        PpoLearner.warm_start(path, (m["O"],), Box((m["A"],)))


def test_refusals(sg):
    from simgan_amd import _lib, checkpoint
    from simgan_amd.ensemble import PolicyEnsemble
    p = make(sg, 11, 3, 16)
    ff = sg.Policy((11,), Box((3,)), base_kwargs={"recurrent": False, "hidden_size": 16})
    with pytest.raises(NotImplementedError, match="mirror-symmetry loss: implemented for feed-forward policies only"):
        sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.0, symmetry_coef=1.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5, mirror_obs=np.eye(11, dtype=np.float32),
                    mirror_act=np.eye(3, dtype=np.float32))
    with pytest.raises(NotImplementedError, match="not for a recurrent Policy"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    with pytest.raises(NotImplementedError, match="not for a recurrent Policy"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, acktr=True)
    with pytest.raises(NotImplementedError, match="feed-forward members only"):
        PolicyEnsemble([p, p])
    with pytest.raises(NotImplementedError, match="reference's object layout"):
        checkpoint.save_policy(os.path.join(GOLDEN, "never_written.pt"), p)
    with pytest.raises(ValueError, match="obs size == hidden size"):
        p.reset_critic((11,))
    with pytest.raises(ValueError, match="needs rnn_hxs"):
        p.act(np.zeros((2, 11), np.float32), None, None)
    # the same refusals behind the C ABI, each naming the mismatch
    lib, h = p.lib, _lib.H()
    agent = sg.algo.PPO(p, 0.2, 1, 3, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    eye = np.eye(3, dtype=np.float32)
    with pytest.raises(_lib.SimganHipError, match="sg_ppo_set_symmetry: the mirror-symmetry loss is implemented for feed-forward"):
        _lib.check(lib.sg_ppo_set_symmetry(agent.h, 1.0, None, _lib.fptr(eye)))
    ff_agent = sg.algo.PPO(ff, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    with pytest.raises(_lib.SimganHipError, match="sg_ppo_set_hidden_states: the policy is feed-forward"):
        _lib.check(lib.sg_ppo_set_hidden_states(ff_agent.h, _lib.fptr(np.zeros(16, np.float32)), 16))
    ro2 = sg.RolloutStorage(2, 2, (11,), Box((3,)), 16, 1)
    with pytest.raises(_lib.SimganHipError, match="PPO requires the number of processes"):
        agent.update(ro2)                        # N = 2 < M = 3: the reference's assertion
    ro7 = sg.RolloutStorage(2, 7, (11,), Box((3,)), 16, 1)
    with pytest.raises(_lib.SimganHipError, match="do not split into minibatches"):
        agent.update(ro7)                        # per = 2, 7 % 2 != 0: the reference's IndexError
    ro6 = sg.RolloutStorage(2, 6, (11,), Box((3,)), 16, 1)
    with pytest.raises(_lib.SimganHipError, match="not a permutation of the 6 environments"):
        agent.update(ro6, perms=np.zeros((1, 6), np.int64))
    with pytest.raises(ValueError, match="recurrent_hidden_states"):
        agent.update(sg.RolloutStorage(2, 6, (11,), Box((3,)), 1, 1))
    with pytest.raises(_lib.SimganHipError, match="sg_ppo_set_hidden_states must hand over"):
        _lib.check(lib.sg_ppo_update(agent.h, ro6.h, None, 0, 0, (C.c_float * 3)()))
    acfg = _lib.A2CConfig(0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5)
    with pytest.raises(_lib.SimganHipError, match="sg_a2c_create: A2C is implemented for feed-forward"):
        _lib.check(lib.sg_a2c_create(p.ctx.h, p.h, C.byref(acfg), C.byref(h)))
    kcfg = _lib.ACKTRConfig(0.5, 0.01, 0.25, 0.9, 0.99, 0.001, 1e-2, 10)
    with pytest.raises(_lib.SimganHipError, match="sg_acktr_create: ACKTR is not defined for a recurrent"):
        _lib.check(lib.sg_acktr_create(p.ctx.h, p.h, C.byref(kcfg), C.byref(h)))
    obs, out = np.zeros((2, 11), np.float32), np.zeros((2, 1), np.float32)
    hx, mk = np.zeros((2, 16), np.float32), np.ones(2, np.float32)
    with pytest.raises(_lib.SimganHipError, match="sg_policy_get_value: this policy is recurrent"):
        _lib.check(lib.sg_policy_get_value(p.h, _lib.fptr(obs), 2, _lib.fptr(out)))
    with pytest.raises(_lib.SimganHipError, match="sg_policy_get_value_rnn: this policy is feed-forward"):
        _lib.check(lib.sg_policy_get_value_rnn(ff.h, _lib.fptr(obs), _lib.fptr(hx), _lib.fptr(mk), 2, _lib.fptr(out)))
    handles = (_lib.H * 1)(p.h)
    idx = np.zeros(2, np.int32)
    act, lp = np.zeros((2, 3), np.float32), np.zeros((2, 1), np.float32)
    with pytest.raises(_lib.SimganHipError, match="sg_policy_act_ensemble: member 0 is a recurrent policy"):
        _lib.check(lib.sg_policy_act_ensemble(handles, 1, idx.ctypes.data_as(C.POINTER(C.c_int32)), _lib.fptr(obs), 2, None, 0, 1,
                                              _lib.fptr(out), _lib.fptr(act), _lib.fptr(lp)))
    ro = sg.RolloutStorage(2, 2, (11,), Box((3,)), 16, 1)
    with pytest.raises(_lib.SimganHipError, match="sg_rollout_compute_returns_policy: the policy is recurrent"):
        _lib.check(lib.sg_rollout_compute_returns_policy(ro.h, p.h, 1, 0.99, 0.95, 1))
    with pytest.raises(_lib.SimganHipError, match="unknown kind 3"):
        _lib.check(lib.sg_policy_create2(p.ctx.h, 3, 4, 2, 8, 1, 0, C.byref(h)))


def test_feed_forward_is_unchanged(sg):
    g = load("ppo_mlp_tiny")
    m = g["meta"]
    p = sg.Policy((m["O"],), Box((m["A"],)), base_kwargs={"recurrent": False, "hidden_size": m["H"]})
    assert p.is_recurrent is False and p.recurrent_hidden_state_size == 1
    assert [n for n, _ in p.param_shapes()][0] == "base.actor.0.weight" and len(p.param_shapes()) == 13
    assert p.param_shapes()[0][1] == (m["H"], m["O"])
    p.set_flat_params(g["params0"])
    v, a, lp, hx = p.act(g["obs"][0], None, None, deterministic=True)   # None for rnn_hxs / masks, as the smoke test calls it
    assert hx is None
    ro = sg.RolloutStorage(m["T"], m["N"], (m["O"],), Box((m["A"],)), 1, g["obs_feat"].shape[-1])
    for name in ("obs", "obs_feat", "actions", "rewards", "value_preds", "returns", "action_log_probs", "masks", "bad_masks"):
        if getattr(ro, name).numel():
            getattr(ro, name).copy_(getattr(ro, name).new_tensor(g[name]))
    agent = sg.algo.PPO(p, m["clip_param"], m["ppo_epoch"], m["num_mini_batch"], m["value_loss_coef"], m["entropy_coef"], lr=m["lr"],
                        eps=m["eps"], max_grad_norm=m["max_grad_norm"])
    losses = agent.update(ro, perms=g["perms"])
    assert_close(losses, g["losses"], what="ppo losses")
    assert_close(p.get_flat_params(), g["params1"], what="params after update")


# ------------------------------------------------------------------------------------------- PPO through time
PPO_CASES = ["ppo_gru_tiny", "ppo_gru_hopper", "ppo_gru_laikago", "ppo_gru_long"]   # hopper, laikago: hidden 64; long: T = 128
load_ppo = gru_ref.load_ppo


def _ppo_problem(sg, g, device_resident=False):
    m = g["meta"]
    p = make(sg, m["O"], m["A"], m["H"])
    p.set_flat_params(g["params0"])
    ro = sg.RolloutStorage(m["T"], m["N"], (m["O"],), Box((m["A"],)), p.recurrent_hidden_state_size, g["obs_feat"].shape[-1])
    for name in ("obs", "obs_feat", "actions", "rewards", "value_preds", "returns", "action_log_probs", "masks", "bad_masks"):
        if getattr(ro, name).numel():
            getattr(ro, name).copy_(getattr(ro, name).new_tensor(g[name]))
    ro.recurrent_hidden_states[0].copy_(ro.obs.new_tensor(g["recurrent_hidden_states0"]))
    if device_resident:
        ro.sync_to_device()
        ro.device_resident = True
    agent = sg.algo.PPO(p, m["clip_param"], m["ppo_epoch"], m["num_mini_batch"], m["value_loss_coef"], m["entropy_coef"], lr=m["lr"],
                        eps=m["eps"], max_grad_norm=m["max_grad_norm"])
    return p, agent, ro


def _blocks(p, flat):
    """name -> slice of a flat state_dict-ordered vector: the GRU's tensors are reported by name, so a wrong gate shows up as one"""
    out, off = {}, 0
    for name, shape in p.param_shapes():
        n = int(np.prod(shape))
        out[name] = flat[off:off + n]
        off += n
    return out


@pytest.mark.parametrize("name", ["ppo_gru_onestep", "ppo_gru_onestep64"])   # hidden 32, and the shipped hidden 64
def test_ppo_gru_onestep_is_the_gradient_check(sg, name):
    """ppo_epoch = 1, one minibatch: Adam's m = 0.1 g and v = 0.001 g^2 after one step ARE the clipped gradient, block by block."""
    g = load_ppo(name)
    p, agent, ro = _ppo_problem(sg, g)
    losses = agent.update(ro, perms=g["perms"])
    assert_close(ro.device_advantages(), g["advantages"], rtol=1e-5, what="advantages")
    assert_close(losses, g["losses"], what="ppo losses")
    mm, vv, step = agent.get_adam()
    assert step == 1
    bm, bv, rm, rv = _blocks(p, mm), _blocks(p, vv), _blocks(p, g["adam_m"]), _blocks(p, g["adam_v"])
    for name in bm:
        print(name, "max |m - ref|", float(np.max(np.abs(bm[name] - rm[name]))), "max |ref|", float(np.max(np.abs(rm[name]))))
    for name in bm:
        gate = 3 if name.startswith("base.gru") else 1
        for k in range(gate):   # the GRU's tensors gate by gate: r, z, n
            a, b = np.array_split(bm[name], gate)[k], np.array_split(rm[name], gate)[k]
            assert_close(a, b, rtol=1e-3, atol=1e-7, what=f"adam m of {name}" + (f" gate {'rzn'[k]}" if gate == 3 else ""))
            assert_close(np.array_split(bv[name], gate)[k], np.array_split(rv[name], gate)[k], rtol=1e-3, atol=1e-10,
                         what=f"adam v of {name}" + (f" gate {'rzn'[k]}" if gate == 3 else ""))
    assert_close(p.get_flat_params(), g["params1"], what="params after the step")


@pytest.mark.parametrize("name", PPO_CASES)
def test_ppo_gru_golden(sg, name):
    g = load_ppo(name)
    m = g["meta"]
    p, agent, ro = _ppo_problem(sg, g)
    losses = agent.update(ro, perms=g["perms"])
    assert np.array_equal(agent.last_perms(), g["perms"]) and g["perms"].shape == (m["ppo_epoch"], m["N"])
    assert_close(ro.device_advantages(), g["advantages"], rtol=1e-5, what="advantages")
    assert_close(losses, g["losses"], what="ppo losses")
    mm, vv, step = agent.get_adam()
    per = m["N"] // m["num_mini_batch"]
    assert step == m["steps"] == m["ppo_epoch"] * (m["N"] // per)
    assert_close(mm, g["adam_m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert_close(vv, g["adam_v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close_adam(p.get_flat_params(), g["params1"], m["lr"], m["steps"], what="params after the update")


def test_ppo_gru_global_weight_instances(sg, monkeypatch):
    monkeypatch.setenv("SG_POLICY_GW", "1")
    g = load_ppo("ppo_gru_laikago")
    m = g["meta"]
    p, agent, ro = _ppo_problem(sg, g)
    losses = agent.update(ro, perms=g["perms"])
    assert_close(losses, g["losses"], what="ppo losses")
    mm, vv, _ = agent.get_adam()
    assert_close(mm, g["adam_m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert_close(vv, g["adam_v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close_adam(p.get_flat_params(), g["params1"], m["lr"], m["steps"], what="params after the update")


def test_ppo_gru_is_bit_reproducible(sg, monkeypatch):
    """The same update twice from the same state, the captured graph against direct launches, and a device-resident rollout
    against a host rollout: identical parameters and Adam state (no atomics, one summation order)."""
    g = load_ppo("ppo_gru_hopper")

    def run(resident=False, updates=2):
        p, agent, ro = _ppo_problem(sg, g, device_resident=resident)
        out = [agent.update(ro, perms=g["perms"]) for _ in range(updates)]
        return out, p.get_flat_params(), agent.get_adam()

    a, b, c = run(), run(), run(resident=True)
    monkeypatch.setenv("SG_PPO_GRAPH", "0")
    d = run()
    for other in (b, c, d):
        assert a[0] == other[0]
        assert np.array_equal(a[1], other[1])
        assert np.array_equal(a[2][0], other[2][0]) and np.array_equal(a[2][1], other[2][1]) and a[2][2] == other[2][2]
    assert np.isfinite(a[1]).all()


def test_ppo_gru_library_permutations_and_adam_round_trip(sg):
    g = load_ppo("ppo_gru_tiny")
    m = g["meta"]
    p, agent, ro = _ppo_problem(sg, g)
    losses = agent.update(ro)                       # the library draws the environment permutations
    perms = agent.last_perms()
    assert perms.shape == (m["ppo_epoch"], m["N"])
    assert all(np.array_equal(np.sort(r), np.arange(m["N"])) for r in perms)
    assert np.isfinite(losses).all()
    mm, vv, step = agent.get_adam()
    p2, agent2, ro2 = _ppo_problem(sg, g)           # replay: same permutations -> same bits
    agent2.update(ro2, perms=perms)
    assert np.array_equal(p.get_flat_params(), p2.get_flat_params())
    agent2.set_adam(mm, vv, step)
    m2, v2, s2 = agent2.get_adam()
    assert np.array_equal(mm, m2) and np.array_equal(vv, v2) and s2 == step


def test_ppo_learner_iteration_with_a_recurrent_policy(sg):
    from simgan_amd.driver import PpoLearner
    rng = np.random.default_rng(9)
    O, A, H, T, N = 11, 3, 64, 8, 8

    class Envs:
        def step(self, action):
            done = rng.random(N) < 0.1
            return (rng.standard_normal((N, O)).astype(np.float32), rng.standard_normal((N, 1)).astype(np.float32), done,
                    [{} for _ in range(N)])

    p = make(sg, O, A, H, seed=2)
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), p.recurrent_hidden_state_size, O)
    ro.obs[0].copy_(ro.obs.new_tensor(rng.standard_normal((N, O)).astype(np.float32)))
    agent = sg.algo.PPO(p, 0.2, 2, 4, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    learner = PpoLearner(p, agent, ro)
    for _ in range(2):
        learner.collect(Envs())
        last = npv(ro.recurrent_hidden_states)[-1].copy()
        assert np.abs(last).max() > 0
        out = learner.update()
        assert all(np.isfinite(float(v)) for v in out.values())
        assert np.array_equal(npv(ro.recurrent_hidden_states)[0], last)   # after_update carried the state over
    assert agent.get_adam()[2] == 2 * 2 * 4


@pytest.mark.parametrize("O,A,H,T,N,E,M", [(30, 6, 256, 9, 8, 2, 2),      # hidden 256: global-weight scans, 16 column tiles over 4 waves
                                           (13, 5, 100, 7, 20, 2, 1),     # hidden 100: no multiple of 16, 7 column tiles, two environment tiles
                                           (47, 12, 64, 128, 8, 1, 2)])   # the north-star sequence length at the shipped width
def test_ppo_gru_update_against_the_float64_restatement(sg, O, A, H, T, N, E, M):
    """Widths with no fixture: the whole update against tests/gru_ref.py's float64 numpy update (pinned on the reference-written
    fixtures by tests/test_recurrent_host.py)."""
    rng = np.random.default_rng(O * 1000 + H + T)
    p = _perturbed(sg, rng, O, A, H)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), H, 1)
    ro.obs.copy_(ro.obs.new_tensor(f(T + 1, N, O)))
    masks = (rng.random((T + 1, N, 1)) > 0.08).astype(np.float32)
    masks[T // 2, 0] = 0.0
    ro.masks.copy_(ro.obs.new_tensor(masks))
    ro.recurrent_hidden_states[0].copy_(ro.obs.new_tensor(0.5 * f(N, H)))
    for step in range(T):   # behaviour policy's own actions / values, states carried as the main's loop carries them
        v, a, lp, h = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step], noise=f(N, A))
        ro.actions[step].copy_(a); ro.action_log_probs[step].copy_(lp); ro.value_preds[step].copy_(v)
        ro.recurrent_hidden_states[step + 1].copy_(h)
    ro.returns.copy_(ro.obs.new_tensor((npv(ro.value_preds) + 0.5 * f(T + 1, N, 1)).astype(np.float32)))
    p0 = (p.get_flat_params() + 0.02 * rng.standard_normal(p.num_params)).astype(np.float32)   # off the behaviour policy: clipping acts
    p.set_flat_params(p0)
    lr = 3e-4
    agent = sg.algo.PPO(p, 0.2, E, M, 0.5, 0.01, lr=lr, eps=1e-5, max_grad_norm=0.5)
    perms = np.stack([rng.permutation(N) for _ in range(E)]).astype(np.int64)
    arrs = {k: npv(getattr(ro, k)).copy() for k in ("obs", "actions", "value_preds", "returns", "action_log_probs", "masks")}
    hxs0 = npv(ro.recurrent_hidden_states)[0].copy()
    ref = gru_ref.ppo_update(p0, O, A, H, arrs, hxs0, perms, E, M, 0.2, 0.5, 0.01, lr, 1e-5, 0.5)
    losses = agent.update(ro, perms=perms)
    assert_close(losses, ref["losses"], what="ppo losses")
    mm, vv, step = agent.get_adam()
    assert step == ref["steps"]
    bm, rm = _blocks(p, mm), _blocks(p, ref["adam_m"])
    for name in bm:
        assert_close(bm[name], rm[name], rtol=1e-3, atol=1e-7, what=f"adam m of {name}")
    assert_close(vv, ref["adam_v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close_adam(p.get_flat_params(), ref["params"], lr, ref["steps"], what="params after the update")


@pytest.mark.parametrize("learner_kind", ["ppo", "gail"])
def test_learners_on_a_device_resident_rollout_with_a_recurrent_policy(sg, learner_kind):
    """device_resident = True: the value of slot T comes from get_value on the host mirrors (the device rollout has no
    hidden-state field), GAE and the update run on the device copy.  Pinned: both learners run (no refusal), every update
    makes its E * (N // per) steps, and after_update carries the last state into slot 0 on the host mirrors."""
    from simgan_amd.driver import GailDynLearner, PpoLearner
    O, A, H, T, N, F = 11, 3, 64, 8, 8, 6

    def run(resident):
        rng = np.random.default_rng(9)

        class Envs:
            def step(self, action):
                done = rng.random(N) < 0.1
                return (rng.standard_normal((N, O)).astype(np.float32), rng.standard_normal((N, 1)).astype(np.float32), done,
                        [{"sas_feat": rng.standard_normal(F).astype(np.float32)} for _ in range(N)])

        p = make(sg, O, A, H, seed=2)
        ro = sg.RolloutStorage(T, N, (O,), Box((A,)), p.recurrent_hidden_state_size, F if learner_kind == "gail" else O)
        ro.obs[0].copy_(ro.obs.new_tensor(rng.standard_normal((N, O)).astype(np.float32)))
        ro.device_resident = resident
        agent = sg.algo.PPO(p, 0.2, 2, 4, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5, seed=5)
        if learner_kind == "gail":
            disc = sg.algo.gail.Discriminator(F, 32, None, seed=3)
            learner = GailDynLearner(p, agent, disc, ro, rng.standard_normal((64, F)).astype(np.float32), gail_batch_size=16, gail_epoch=1)
        else:
            learner = PpoLearner(p, agent, ro)
        feats = lambda infos: np.stack([i["sas_feat"] for i in infos])  # noqa: E731
        for _ in range(2):
            learner.collect(Envs(), feats) if learner_kind == "gail" else learner.collect(Envs())
            last = npv(ro.recurrent_hidden_states)[-1].copy()
            out = learner.update()
            out = out.resolve() if hasattr(out, "resolve") else out
            assert np.isfinite(float(out["value_loss"]))
            assert np.array_equal(npv(ro.recurrent_hidden_states)[0], last)
        assert agent.get_adam()[2] == 2 * 2 * 4
        return p.get_flat_params()

    a, b = run(True), run(False)   # (every Policy object draws its own action noise, so the two runs are different trajectories)
    assert np.isfinite(a).all() and np.isfinite(b).all()


def test_world_2_is_refused_by_the_library_too(sg):
    """A communicator of world 2 (loopback ranks on one GPU): PPO on a recurrent policy is refused by the Python class and by
    sg_ppo_create, each naming the world."""
    from simgan_amd import _lib
    from test_gpu_world import run_ranks

    def body(rank, ctx):
        q = sg.Policy((6,), Box((2,)), base_kwargs={"recurrent": True, "hidden_size": 16}, ctx=ctx)
        out = []
        try:
            sg.algo.PPO(q, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
        except NotImplementedError as exc:
            out.append(str(exc))
        cfg, h = _lib.PPOConfig(0.2, 1, 1, 0.5, 0.0, 3e-4, 1e-5, 0.5, 1), _lib.H()
        try:
            _lib.check(q.lib.sg_ppo_create(ctx.h, q.h, C.byref(cfg), C.byref(h)))
        except _lib.SimganHipError as exc:
            out.append(str(exc))
        return out

    for errs in run_ranks(2, body):
        assert len(errs) == 2 and "runs on one rank" in errs[0] and "world 2" in errs[0], errs
        assert "sg_ppo_create: PPO with a recurrent policy runs on one rank" in errs[1] and "world 2" in errs[1], errs
