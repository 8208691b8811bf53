"""CPU: the recurrent Policy on Discrete / MultiBinary action spaces -- the arbiter of tests/gru_discrete_ref.py held to the
reference's own modules (where a reference checkout is present), the faults it must be able to see, the admission of every case
tests/test_gpu_gru_discrete.py looks at, the flat parameter order, the constructor's opt-in and the Python-level refusals."""
import json
import os
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest

import autograd_ref as ar
import gru_discrete_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTS = (ref.CATEGORICAL, ref.BERNOULLI)
CASES = [(d, s) for d in DISTS for s in ref.SHAPES[d]] + [(d, ref.DEAD_ENV_CASE[0]) for d in DISTS]
HEADS = ("base.actor", "base.critic", "dist.linear")


# ------------------------------------------------------------------------------------------- the arbiter itself
@pytest.mark.skipif(not ar.reference_present(), reason="needs the reference checkout (development container only)")
def test_the_arbiter_against_the_references_own_modules():
    """gru_discrete_ref.tier2 in a child process: PPO.update (both value losses) and A2C_ACKTR.update of the reference's recurrent
    Policy on Discrete / MultiBinary after .double(); the .grad they leave against the arbiter, per block, at autograd_ref.BOUND."""
    r = subprocess.run([sys.executable, "-s", os.path.join(ROOT, "tests", "gru_discrete_ref.py"), "--tier2"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT, env={k: v for k, v in os.environ.items() if k != "PYTHONPATH"})
    assert r.returncode == 0, r.stderr[-3000:]
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TIER2 ")][-1][6:])
    assert len(doc) == 3 * len(ref.TIER2), list(doc)
    for label, j in doc.items():
        assert j["worst"] <= ar.BOUND and j["loss_error"] <= ar.LOSS_ATOL, (label, j)


@pytest.mark.parametrize("dist", DISTS, ids=["cat", "ber"])
@pytest.mark.parametrize("algo", ["ppo", "a2c"])
def test_wrong_restatements_fail_on_the_references_alone(dist, algo):
    """Each fault moves the gradient by more than the bound the GPU tests hold the library to, in the blocks it should."""
    c = ref.random_case(dist, 11, 3, 16, 5, 4)
    f = (lambda **kw: ref.ppo_grad(c, **kw)[0]) if algo == "ppo" else (lambda **kw: ref.a2c_grad(c, **kw)[0])
    good = f()
    errs = {w: ref.block_errors(f(wrong=w), good, c["O"], c["K"], c["H"]) for w in ref.WRONG}
    gru = [k for k in errs["no_mask"] if k.startswith("base.gru")]
    assert len(gru) == 12
    for w in ("no_critic_dh", "no_actor_dh"):      # every heads block right, every GRU block wrong
        assert all(errs[w][k] > 100 * ref.RTOL_BLOCK for k in gru), (w, errs[w])
        assert all(v == 0.0 for k, v in errs[w].items() if k.startswith(HEADS)), (w, errs[w])
    assert all(v > 10 * ref.RTOL_BLOCK for v in errs["no_mask"].values()), errs["no_mask"]
    wrong_entropy = [k for k, v in errs["entropy_mean"].items() if v > ref.RTOL_BLOCK]
    if dist == ref.BERNOULLI:
        assert set(wrong_entropy) >= set(gru) | {"dist.linear.weight", "dist.linear.bias", "base.actor.0.weight"}, errs["entropy_mean"]
    else:
        assert not wrong_entropy        # (the Categorical entropy has no bits to average over)
    assert all(errs["padding"][k] > 10 * ref.RTOL_BLOCK for k in gru + ["base.actor.0.weight", "base.actor.2.bias"]), errs["padding"]
    assert errs["padding"]["dist.linear.weight"] == 0.0 and errs["padding"]["base.critic.0.weight"] == 0.0


@pytest.mark.parametrize("dist,shape", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ref.DIST_NAME[v])
def test_every_gpu_case_is_a_case(dist, shape):
    """What tests/test_gpu_gru_discrete.py relies on, asserted where it is cheap: rows in all three branches of the clipped
    surrogate, none within 1e-4 of a clip boundary, value-loss rows on both sides of the value clip, zero masks (slot 0 included),
    and the float32 evaluation of the arbiter's own expressions within half the bound of float64 -- for PPO and A2C."""
    dead = ref.DEAD_ENV_CASE[1] if shape == ref.DEAD_ENV_CASE[0] else None
    c = ref.random_case(dist, *shape, dead_env=dead)
    lo, mid, hi, margin = ref.surrogate_branches(c)
    assert lo >= 2 and mid >= 2 and hi >= 2 and margin > 1e-4, (lo, mid, hi, margin)
    T = c["T"]
    assert (c["masks"][0] == 0).any() and (T < 3 or (c["masks"][:T] == 0).sum() >= 2)
    dv = np.abs(ref.evaluate(c)[0] - c["value_preds"][:T].reshape(-1))
    assert (dv > ref.CLIP).any() and (dv < ref.CLIP).any()
    for algo, uc in (("ppo", True), ("ppo", False), ("a2c", True)):
        worst = ref.admit(c, algo, uc)[2]
        assert worst <= 0.5 * ref.RTOL_BLOCK, f"{ref.tag(dist, shape)} {algo}: float32 is {worst:.2e} from float64: not a case"


# ------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("dist,K", [(ref.CATEGORICAL, 17), (ref.BERNOULLI, 5)])
def test_param_shapes_gru_first_linear_head_last(dist, K):
    import simgan_amd as sg
    p = sg.Policy.__new__(sg.Policy)
    p.__dict__.update(_dist_kind=dist, n_out=K, obs_dim=11, act_dim=1 if dist == ref.CATEGORICAL else K, hidden_size=32, critic_hidden=32,
                      recurrent=True)
    got = [(n, tuple(s)) for n, s in p.param_shapes()]
    assert got == ref.param_shapes(11, K, 32)
    assert [n for n, _ in got[:4]] == list(ref.GRU_NAMES) and [n for n, _ in got[-2:]] == ["dist.linear.weight", "dist.linear.bias"]
    assert got[4] == ("base.actor.0.weight", (32, 32)) and got[8] == ("base.critic.0.weight", (32, 32))      # the trunks read the H-wide state
    assert p.recurrent_hidden_state_size == 32 and p.is_recurrent
    with pytest.raises(ValueError, match="no log-std to reset"):
        p.reset_variance(None, -1.0)


# ------------------------------------------------------------------------------------------- construction
def _spy_create(monkeypatch):
    import simgan_amd as sg
    calls = []
    monkeypatch.setattr(sg.Policy, "_create", lambda self, *a, **kw: calls.append((a, kw)))
    monkeypatch.setattr(sg.Policy, "_init_params", lambda self, rng: None)
    return sg, calls


@pytest.mark.parametrize("space", [ref.dr.Discrete(3), ref.dr.MultiBinary(3)], ids=["Discrete", "MultiBinary"])
def test_construction_is_opt_in(monkeypatch, space):
    sg, calls = _spy_create(monkeypatch)
    monkeypatch.delenv("SG_RECURRENT_HEADS", raising=False)
    kw = dict(base_kwargs={"recurrent": True, "hidden_size": 8})
    with pytest.raises(NotImplementedError, match="the GRU base is built with the Gaussian head \\(Box actions\\) only"):
        sg.Policy((4,), space, **kw)
    with pytest.raises(NotImplementedError, match="the GRU base is built with the Gaussian head"):
        sg.Policy((4,), space, recurrent_heads=False, **kw)
    monkeypatch.setenv("SG_RECURRENT_HEADS", "0")
    with pytest.raises(NotImplementedError, match="the GRU base is built with the Gaussian head"):
        sg.Policy((4,), space, **kw)
    assert not calls
    sg.Policy((4,), space, recurrent_heads=True, **kw)                   # the keyword
    monkeypatch.setenv("SG_RECURRENT_HEADS", "1")
    sg.Policy((4,), space, **kw)                                         # the environment switch, read at construction
    with pytest.raises(NotImplementedError, match="the GRU base is built with the Gaussian head"):
        sg.Policy((4,), space, recurrent_heads=False, **kw)              # the keyword wins
    assert len(calls) == 2
    is_cat = type(space).__name__ == "Discrete"
    for a, k in calls:
        assert a[:4] == (4, 1 if is_cat else 3, 8, 1) and k["recurrent"] is True and k["n_out"] == 3
        assert k["dist"] == (ref.CATEGORICAL if is_cat else ref.BERNOULLI)


def test_the_cnn_base_stays_feed_forward(monkeypatch):
    sg, calls = _spy_create(monkeypatch)
    with pytest.raises(NotImplementedError, match="the CNN base is built feed-forward only"):
        sg.Policy((4, 84, 84), ref.dr.Discrete(6), base_kwargs={"recurrent": True}, recurrent_heads=True)
    assert not calls


# ------------------------------------------------------------------------------------------- refusals, on stand-ins
def test_python_level_refusals():
    """Each with a message of its own, before any device object is touched."""
    import simgan_amd as sg
    from simgan_amd import driver
    from simgan_amd.ensemble import PolicyEnsemble
    from simgan_amd.storage import RolloutStorage
    pol = types.SimpleNamespace(is_recurrent=True, KIND=0, dist_kind=ref.CATEGORICAL, cnn=0, ctx=types.SimpleNamespace(world=1))
    with pytest.raises(NotImplementedError, match="ACKTR is not built for a recurrent Policy on a Discrete / MultiBinary"):
        sg.algo.A2C_ACKTR(pol, 0.5, 0.01, acktr=True, recurrent=True)
    with pytest.raises(NotImplementedError, match="A2C through time is opt-in"):
        sg.algo.A2C_ACKTR(pol, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    with pytest.raises(NotImplementedError, match="mirror-symmetry loss: not for a recurrent Policy on a Discrete / MultiBinary"):
        sg.algo.PPO(pol, 0.2, 1, 1, 0.5, 0.0, symmetry_coef=1.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5, mirror_obs=np.eye(3),
                    mirror_act=np.eye(1))
    with pytest.raises(NotImplementedError, match="PolicyEnsemble: a recurrent member on a Discrete / MultiBinary action space"):
        PolicyEnsemble([pol])
    two = types.SimpleNamespace(is_recurrent=True, KIND=0, dist_kind=ref.BERNOULLI, cnn=0, ctx=types.SimpleNamespace(world=2))
    with pytest.raises(NotImplementedError, match="PPO with a recurrent Policy runs on one rank"):
        sg.algo.PPO(two, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    ro = RolloutStorage.__new__(RolloutStorage)
    ro.__dict__.update(box_actions=False, num_processes=4, _device_resident=True, _dup=None, device_hidden=True, step=0)
    with pytest.raises(NotImplementedError, match="enable_dup_sym: a mirror-augmented rollout mirrors actions through a linear map"):
        ro.enable_dup_sym(np.eye(3), np.eye(1))
    with pytest.raises(NotImplementedError, match="act_step: a recurrent policy on a Discrete / MultiBinary action space acts through"):
        ro.act_step(pol)
    with pytest.raises(ValueError, match="act_step_chain: the chained step takes a feed-forward learner"):
        ro._chain_inner("act_step_chain", pol, [], True, None, None, None, None, None)
    with pytest.raises(ValueError, match="collect\\(on_device=True\\): the policy is recurrent with a Discrete / MultiBinary action space"):
        driver._check_on_device(ro, pol, False, "collect")


def test_rollout_storage_keeps_int64_actions_beside_hidden_states():
    """a2c/storage.py:40-48: int64 [T, N, 1] actions (float [T, N, n] for MultiBinary) together with a hidden-state width above 1;
    recurrent_generator hands them out per environment; the device sees float32 class indices in both directions of the sync."""
    from simgan_amd import _lib
    from simgan_amd.storage import RolloutStorage
    from test_discrete_host import _FakeCtx, _FakeRolloutLib
    lib = _FakeRolloutLib()
    T, N, O, K, H = 3, 4, 5, 130, 6
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ro = RolloutStorage(T, N, (O,), ref.dr.Discrete(K), H, 1, ctx=types.SimpleNamespace(lib=lib, h=None))
        mb = RolloutStorage(T, N, (O,), ref.dr.MultiBinary(7), H, 1, ctx=_FakeCtx())
    assert tuple(ro.actions.shape) == (T, N, 1) and str(ro.actions.dtype).endswith("int64")
    assert tuple(mb.actions.shape) == (T, N, 7) and str(mb.actions.dtype).endswith("float32")
    assert tuple(ro.recurrent_hidden_states.shape) == (T + 1, N, H) == tuple(mb.recurrent_hidden_states.shape)
    rng = np.random.default_rng(0)
    acts = rng.integers(0, K, size=(T, N, 1))
    hx = rng.standard_normal((T + 1, N, H)).astype(np.float32)
    ro.actions.copy_(ro.actions.new_tensor(acts))
    ro.recurrent_hidden_states.copy_(ro.recurrent_hidden_states.new_tensor(hx))
    perm = np.array([2, 0, 3, 1])
    batches = list(ro.recurrent_generator(None, 2, perm=perm))
    assert len(batches) == 2
    for k, b in enumerate(batches):
        envs = perm[2 * k:2 * k + 2]
        a = np.asarray(b[2])
        assert a.dtype == np.int64 and np.array_equal(a, acts[:, envs].reshape(-1, 1))
        assert np.array_equal(np.asarray(b[1]), hx[0, envs])
    ro.sync_to_device([_lib.F_ACTIONS])
    dev = lib.fields[_lib.F_ACTIONS]
    assert dev.dtype == np.float32 and np.array_equal(dev, acts.reshape(-1).astype(np.float32))
    lib.fields[_lib.F_ACTIONS] = ((dev + 1) % K).astype(np.float32)
    ro.sync_from_device([_lib.F_ACTIONS])
    assert str(ro.actions.dtype).endswith("int64") and np.array_equal(np.asarray(ro.actions), (acts + 1) % K)


def test_reference_checkpoint_of_a_recurrent_categorical_policy_is_read():
    """tests/golden/ckpt_policy_gru_cat.pt (tools/gen_golden_gru_discrete.py): kind, dims and the state_dict in the flat order"""
    from helpers import load
    from simgan_amd.checkpoint import read_reference_checkpoint
    g = load("ckpt_policy_gru_cat")
    m = g["meta"]
    ck = read_reference_checkpoint(os.path.join(ROOT, "tests", "golden", "ckpt_policy_gru_cat.pt"))
    assert ck["kind"] == "mlp_categorical" and ck["recurrent"] and (ck["obs_dim"], ck["n_out"], ck["hidden"], ck["act_dim"]) == (m["O"], m["K"], m["H"], 1)
    shapes = ref.param_shapes(m["O"], m["K"], m["H"])
    assert [n for n, _ in shapes] == m["names"]
    flat = np.concatenate([np.asarray(ck["state_dict"][n], np.float32).reshape(-1) for n, _ in shapes])
    assert np.array_equal(flat, g["flat"])
    assert np.allclose(ck["ob_rms"]["mean"], g["rms_mean"])
