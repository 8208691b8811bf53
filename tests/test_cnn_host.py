"""CPU: the arbiter of the CNN base (tests/cnn_ref.py) against the reference's fixtures, the conditions its gradient cases must
meet, the test of the test, and the host half of the Python layer.

  fixtures    cnn_ref's float64 evaluation reproduces every policy_cnn_* / ppo_cnn_* value within a tenth of the tolerance (what
              the float32 reference's own rounding leaves)
  kinks       every gradient case tests/test_gpu_cnn.py uses keeps every ReLU pre-activation KINK_FACTOR x the float32 forward's
              error away from zero, and every row MARGIN away from a branch boundary of the loss -- on the references alone
  defects     a conv weight gradient with kh and kw swapped, a dropped /255, a ReLU mask taken from the wrong layer, a flatten in
              (y, x, channel) order, a dropped conv bias gradient: each fails the per-block comparison the GPU test makes
  host layer  state_dict names / order / shapes, the checkpoint fixture through the allowlisted unpickler and through a bare
              torch.load under the alias package, the rollout's 5-D observations, every refusal that needs no device"""
import os
import pickle
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest
import torch

import cnn_ref as cr
from helpers import ATOL, GOLDEN, RTOL, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLICY_FIXTURES = ["policy_cnn_cat", "policy_cnn_box"]
PPO_FIXTURES = ["ppo_cnn_cat", "ppo_cnn_box"]


def tenth(got, ref, what):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    r = float(np.max(np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))))
    assert r <= 0.1, f"{what}: {r:.3f} of the tolerance"


# ------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", POLICY_FIXTURES)
def test_the_arbiter_reproduces_the_policy_fixture(name):
    g = load(name)
    m = g["meta"]
    shapes = cr.param_shapes(m["C"], m["Hs"], m["dist"], m["P"])
    assert g["params"].size == cr.num_params(shapes) and g["obs"].dtype == np.uint8
    obs = g["obs"].astype(np.float32)
    out = cr.forward64(shapes, g["params"], obs, m["dist"])
    tenth(g["get_value"], out[0], "get_value")
    det = cr.act64(shapes, g["params"], obs, m["dist"])
    tenth(g["det_logp"], det["logp"], "log-prob of the mode")
    if m["dist"] == "categorical":
        assert det["margin"] > 1e-4 and np.array_equal(g["det_action"].reshape(-1), det["action"])
        tenth(g["logits"], out[1], "logits")
        smp = cr.act64(shapes, g["params"], obs, m["dist"], g["uniform"])
        assert smp["margin"] > 1e-4 and np.array_equal(g["act_action"].reshape(-1), smp["action"])
        assert len(set(g["act_action"].reshape(-1).tolist())) > 1
    else:
        tenth(g["det_action"], det["action"], "mode")
        smp = cr.act64(shapes, g["params"], obs, m["dist"], g["noise"])
        tenth(g["act_action"], smp["action"], "sampled action")
        tenth(g["act_logp"], smp["logp"], "its log-prob")
        tenth(g["act_value"], smp["value"], "value from act")
    for n in m["NS"]:
        with torch.no_grad():
            v, lp, ent = cr.evaluate(cr.leaves(g["params"], shapes), cr.ar.t64(obs[:n]), g["eval_action"][:n], m["dist"])
        tenth(g[f"eval_entropy_{n}"], ent.numpy(), f"entropy over {n} rows")
        tenth(g["eval_value"][:n], v.numpy(), "evaluate value")
        tenth(g["eval_logp"][:n], lp.numpy(), "evaluate logp")


def ppo_case(g):
    m = g["meta"]
    return cr.Case(C=m["C"], T=m["T"], N=m["N"], dist=m["dist"], params=g["params0"], obs=g["obs"].astype(np.float32), actions=g["actions"],
                   action_log_probs=g["action_log_probs"], value_preds=g["value_preds"], returns=g["returns"])


@pytest.mark.parametrize("name", PPO_FIXTURES)
def test_the_arbiter_reproduces_the_whole_update(name):
    g = load(name)
    m = g["meta"]
    assert (m["ppo_epoch"], m["num_mini_batch"], m["T"] * m["N"]) == (2, 2, 16) and g["obs"].dtype == np.uint8
    shapes = cr.param_shapes(m["C"], m["Hs"], m["dist"], m["P"])
    losses, params1, _ = cr.adam_update64(shapes, ppo_case(g), g["perms"], 2, 2, m["max_grad_norm"])
    tenth(g["ppo_losses"], losses, "losses")
    ref = load(name + "_params1")["ppo_params1"]
    err = np.abs(ref.astype(np.float64) - params1)
    bad = err > 0.1 * (ATOL + RTOL * np.abs(params1))      # helpers.assert_close_adam's rule at a tenth of its tolerance
    assert bad.sum() <= max(1, int(5e-4 * bad.size)) and err.max() <= m["lr"] * 4, (int(bad.sum()), float(err.max()))
    assert np.abs(ref - g["params0"]).max() > 0.5 * m["lr"], "the update moved nothing"


# ------------------------------------------------------------------------------------------------- the gradient cases
@pytest.mark.parametrize("key", cr.GRAD_CASES + [cr.GATHER_CASE], ids=lambda k: "-".join(map(str, k)))
def test_gradient_cases_keep_clear_of_the_relu_kinks_and_the_branch_boundaries(key):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (1 x 1: the unbiased std of one advantage)
        c = cr.case(*key)
        ok, km, classes, margins = cr.acceptable(c)
    assert km >= cr.KINK_FACTOR, f"{c.tag}: a ReLU pre-activation lies {km:.2f} x the float32 forward's error from zero"
    assert ok, (c.tag, km, classes, margins)
    if c.regime == "branches":
        assert min(classes.values()) >= 1, classes


def test_the_one_row_rollout_has_no_finite_gradient_in_the_reference():
    """T x N = 1 x 1: torch's unbiased std of one advantage is NaN (a2c/algo/ppo.py:67-68), so is the loss and, through
    clip_grad_norm_, every gradient element.  The GPU test holds the library to that: the case checks that a one-row minibatch
    runs, not a number."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = cr.case(*cr.GRAD_CASES[0])
        r = cr.rows_of(c)
        assert np.isnan(r["adv"]).all()
        g, _ = cr.ppo_grad(c.shapes, c.params, r["obs"], r["actions"], r["old_logp"], r["value_preds"], r["returns"], r["adv"], c.dist)
    assert np.isnan(g).any() and np.isnan(cr.clip_factor(g, 0.5)) and np.isnan(cr.clip_factor(g, 1e9))


@pytest.mark.parametrize("fault", ["wgrad_khkw", "no_div255", "mask_wrong_layer", "flatten_yxc", "no_conv_bias"])
def test_every_injected_defect_fails_the_per_block_comparison(fault):
    c = cr.case(*cr.GRAD_CASES[1])
    r = cr.rows_of(c)
    args = (c.shapes, c.params, r["obs"], r["actions"], r["old_logp"], r["value_preds"], r["returns"], r["adv"], c.dist)
    good, _ = cr.ppo_grad(*args)
    broken, _ = cr.ppo_grad(*args, fault=fault)
    d = cr.block_distances(broken, good, c.shapes)
    assert max(d.values()) > 10 * RTOL, (fault, d)
    assert max(cr.block_distances(good, cr.ppo_grad(*args)[0], c.shapes).values()) == 0.0


def test_the_gaussian_case_pads_and_the_branches_case_has_both_value_losses():
    c = cr.case(*cr.GRAD_CASES[3])
    assert (c.C, c.Hs, c.P) == (3, 20, 3) and c.Hs % 16 and c.T * c.N == 15
    c = cr.case(*cr.GRAD_CASES[4])
    r = cr.rows_of(c)
    args = (c.shapes, c.params, r["obs"], r["actions"], r["old_logp"], r["value_preds"], r["returns"], r["adv"], c.dist)
    assert max(cr.block_distances(cr.ppo_grad(*args, use_clipped=False)[0], cr.ppo_grad(*args, use_clipped=True)[0], c.shapes).values()) > 1e-2


# ------------------------------------------------------------------------------------------------- host layer
def bare_policy(C, Hs, dist, P):
    import simgan_amd as sg
    p = sg.Policy.__new__(sg.Policy)
    p.__dict__.update(_dist_kind=1 if dist == "categorical" else 0, n_out=P, obs_dim=C * 84 * 84, act_dim=1 if dist == "categorical" else P,
                      hidden_size=Hs, critic_hidden=Hs, recurrent=False, cnn=C)
    return p


def test_param_shapes_are_the_references():
    g = load("ckpt_policy_cnn")
    m = g["meta"]
    p = bare_policy(m["C"], m["Hs"], m["dist"], m["P"])
    assert [n for n, _ in p.param_shapes()] == m["names"]
    assert [list(s) for _, s in p.param_shapes()] == m["shapes"]
    assert [(n, tuple(s)) for n, s in p.param_shapes()] == cr.param_shapes(m["C"], m["Hs"], m["dist"], m["P"])
    box = bare_policy(3, 20, "gaussian", 3)
    assert [(n, tuple(s)) for n, s in box.param_shapes()] == cr.param_shapes(3, 20, "gaussian", 3)
    assert box.param_shapes()[-1] == ("dist.logstd._bias", (3, 1))
    assert not p.is_recurrent and p.recurrent_hidden_state_size == 1


def test_the_checkpoint_fixture_is_read_by_the_allowlisted_unpickler():
    from simgan_amd import checkpoint as ck
    g = load("ckpt_policy_cnn")
    m = g["meta"]
    path = os.path.join(GOLDEN, "ckpt_policy_cnn.pt")
    blob = open(path, "rb").read()
    assert b"def forward(" not in blob and b"import torch" not in blob, "the fixture carries source text"
    out = ck.read_reference_checkpoint(path)
    assert out["kind"] == "cnn_categorical" and out["class_name"] == "Policy" and out["ob_rms"] is None
    assert (out["cnn"], out["hidden"], out["n_out"], out["act_dim"], out["dist"], out["obs_dim"]) == (m["C"], m["Hs"], m["P"], 1, 1, m["C"] * 7056)
    assert list(out["state_dict"]) == m["names"] and [list(v.shape) for v in out["state_dict"].values()] == m["shapes"]
    flat = np.concatenate([v.reshape(-1) for v in out["state_dict"].values()])
    assert abs(float(flat.astype(np.float64).sum()) - float(g["checksum"])) < 1e-6
    det = cr.act64(cr.param_shapes(m["C"], m["Hs"], m["dist"], m["P"]), flat, g["obs"].astype(np.float32), m["dist"])
    assert np.array_equal(det["action"], g["action"].reshape(-1))
    tenth(g["logp"], det["logp"], "logp")
    tenth(g["value"], det["value"], "value")
    # the allowlist grew by Conv2d and ReLU only: anything else a file may name is still refused
    assert ("torch.nn.modules.conv", "Conv2d") in ck._ALLOWED and ("torch.nn.modules.activation", "ReLU") in ck._ALLOWED
    assert not [k for k in ck._ALLOWED if k[0].startswith("torch.nn.modules") and k[1] not in ("Linear", "Tanh", "Sequential", "Conv2d", "ReLU")]
    for mod, name in (("torch.nn.modules.conv", "Conv1d"), ("torch.nn.modules.conv", "ConvTranspose2d"), ("torch.hub", "load"), ("builtins", "eval")):
        with pytest.raises(pickle.UnpicklingError):
            ck._StubUnpickler(open(os.devnull, "rb")).find_class(mod, name)


def test_a_bare_torch_load_under_the_alias_package_gives_a_pending_policy():
    """a2c/main.py:81-83: torch.load of the reference's file resolves Policy / CNNBase / Flatten through third_party.a2c_ppo_acktr;
    the weights are read when the policy is first used (no device here: the pending state is inspected instead).  Writing the
    reference's layout back is refused.  In a child process: this one never imports the alias package."""
    m = load("ckpt_policy_cnn")["meta"]
    code = (
        "import pickle, warnings, torch\n"
        "import third_party.a2c_ppo_acktr.model as alias\n"
        "from simgan_amd.checkpoint import policy_from_module_state\n"
        "assert issubclass(alias.CNNBase, alias.NNBase) and hasattr(alias, 'Flatten')\n"
        "warnings.simplefilter('ignore')\n"
        f"obj = torch.load({os.path.join(GOLDEN, 'ckpt_policy_cnn.pt')!r}, map_location='cpu', weights_only=False)\n"
        "pol = obj[0]\n"
        "assert type(pol) is alias.Policy and obj[1] is None\n"
        "st = pol.__dict__['_pending']\n"
        "assert type(st['_modules']['base']) is alias.CNNBase\n"
        "dims, sd = policy_from_module_state('Policy', st)\n"
        f"assert dims['kind'] == 'cnn_categorical' and dims['cnn'] == {m['C']} and dims['hidden'] == {m['Hs']} and list(sd) == {m['names']!r}\n"
        "q = alias.Policy.__new__(alias.Policy)\n"
        "q.__dict__.update(_dist_kind=1, n_out=5, obs_dim=7056, act_dim=1, hidden_size=16, critic_hidden=16, recurrent=False, cnn=1)\n"
        "try:\n"
        "    pickle.dumps(q)\n"
        "    raise SystemExit('pickled')\n"
        "except NotImplementedError as e:\n"
        "    assert 'object layout (nn.Conv2d' in str(e), e\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT), cwd="/tmp")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


class _FakeRolloutLib(object):
    def __init__(self):
        self.fields, self.created = {}, None

    def sg_rollout_create(self, ctx, T, N, O, A, F, out):
        self.created = (T, N, O, A, F)
        return 0

    def sg_rollout_destroy(self, h):
        return 0

    def sg_rollout_upload(self, h, field, ptr, count):
        self.fields[field] = np.ctypeslib.as_array(ptr, shape=(count,)).copy()
        return 0


class Discrete(object):
    def __init__(self, n):
        self.n = n


class Box(object):
    def __init__(self, shape):
        self.shape = tuple(shape)


class MultiBinary(object):
    def __init__(self, n):
        self.n, self.shape = n, (n,)


def test_the_rollout_keeps_five_dimensional_observations_on_the_host():
    from simgan_amd import _lib
    from simgan_amd.storage import RolloutStorage
    lib = _FakeRolloutLib()
    T, N, C = 2, 3, 2
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (no device: pageable host tensors)
        ro = RolloutStorage(T, N, (C, 84, 84), Discrete(4), 1, 1, ctx=types.SimpleNamespace(lib=lib, h=None))
    assert lib.created == (T, N, C * 7056, 1, 1)
    assert tuple(ro.obs.shape) == (T + 1, N, C, 84, 84) and str(ro.obs.dtype).endswith("float32")
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (T + 1, N, C, 84, 84)).astype(np.float32)
    ro.obs[0].copy_(torch.from_numpy(frames[0]))
    for t in range(T):
        ro.insert(torch.from_numpy(frames[t + 1]), np.zeros((N, 1), np.float32), np.full((N, 1), t, np.int64), np.zeros((N, 1), np.float32),
                  np.zeros((N, 1), np.float32), np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32), np.ones((N, 1), np.float32))
    assert np.array_equal(ro.obs.numpy(), frames)
    perm = np.arange(T * N)[::-1].copy()
    batches = list(ro.feed_forward_generator(None, num_mini_batch=2, perm=perm))
    assert [tuple(b[0].shape) for b in batches] == [(3, C, 84, 84)] * 2
    assert np.array_equal(np.concatenate([b[0].numpy() for b in batches]), frames[:-1].reshape(T * N, C, 84, 84)[perm])
    ro.sync_to_device([_lib.F_OBS])
    assert np.array_equal(lib.fields[_lib.F_OBS], frames.reshape(-1))      # one row of C * 84 * 84 floats per image, NCHW
    ro.after_update()
    assert np.array_equal(ro.obs[0].numpy(), frames[-1])
    for call, match in ((lambda: ro.act_step(None), "act_step: on-device collection is not built for image observations"),
                        (lambda: ro.insert_env(None, None, None, None), "insert_env: on-device collection is not built for image"),
                        (lambda: ro.finish_collect(), "finish_collect: on-device collection is not built for image observations"),
                        (lambda: ro.enable_dup_sym(np.eye(2), np.eye(1)), "enable_dup_sym: a mirror-augmented rollout mirrors observations"),
                        (lambda: ro.enable_device_hidden(), "enable_device_hidden: the rollout holds image observations"),
                        (lambda: next(iter(ro.recurrent_generator(None, 1))), "recurrent_generator: image observations are read by the feed-forward")):
        with pytest.raises(NotImplementedError, match=match):
            call()
    with pytest.raises(NotImplementedError, match="1-D observations only"):
        RolloutStorage(T, N, (84, 84), Discrete(4), 1, 1, ctx=types.SimpleNamespace(lib=lib, h=None))


def test_python_refusals_that_need_no_device():
    import simgan_amd as sg
    from simgan_amd.checkpoint import save_policy
    from simgan_amd.driver import GailDynLearner, _check_on_device
    from simgan_amd.ensemble import PolicyEnsemble
    with pytest.raises(ValueError, match=r"the CNN base takes \[C, 84, 84\] only \(the reference hard-codes Linear\(32 \* 7 \* 7"):
        sg.Policy((4, 64, 64), Discrete(6))
    with pytest.raises(NotImplementedError, match="Policy on image observations with base_kwargs={'recurrent': True}"):
        sg.Policy((4, 84, 84), Discrete(6), base_kwargs={"recurrent": True})
    with pytest.raises(NotImplementedError, match="Policy on image observations with a MultiBinary action space"):
        sg.Policy((4, 84, 84), MultiBinary(6))
    with pytest.raises(NotImplementedError, match="only the MLP base on 1-D observations is built"):
        sg.Policy((84, 84), Discrete(6))
    with pytest.raises(NotImplementedError, match="only the MLP base on 1-D observations is built"):
        sg.Policy((4, 84, 84), Discrete(6), base=object)
    pol = types.SimpleNamespace(is_recurrent=False, KIND=0, dist_kind=1, cnn=4, ctx=types.SimpleNamespace(world=1))
    for acktr in (False, True):
        with pytest.raises(NotImplementedError, match="A2C_ACKTR: not implemented for the CNN base"):
            sg.algo.A2C_ACKTR(pol, 0.5, 0.01, acktr=acktr, **({} if acktr else dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)))
    with pytest.raises(NotImplementedError, match="PolicyEnsemble: members with the MLP base only"):
        PolicyEnsemble([pol])
    box = types.SimpleNamespace(is_recurrent=False, KIND=0, dist_kind=0, cnn=4, ctx=types.SimpleNamespace(world=1))
    with pytest.raises(NotImplementedError, match="mirror-symmetry loss: not implemented for the CNN base"):
        sg.algo.PPO(box, 0.2, 1, 1, 0.5, 0.0, symmetry_coef=1.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5, mirror_obs=np.eye(3), mirror_act=np.eye(1))
    box.ctx.world = 2
    with pytest.raises(NotImplementedError, match="PPO on the CNN base \\(image observations\\) runs on one rank"):
        sg.algo.PPO(box, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    with pytest.raises(NotImplementedError, match="GailDynLearner: the GAIL-dyn loop is built for 1-D observations"):
        GailDynLearner(pol, None, None, None, None)
    ro = types.SimpleNamespace(device_resident=True, dup_sym=False)
    with pytest.raises(ValueError, match=r"PpoLearner.collect\(on_device=True\): the policy has the CNN base"):
        _check_on_device(ro, types.SimpleNamespace(is_recurrent=False, dist_kind=0, cnn=1), False, "PpoLearner.collect")
    # the earlier checks keep their order and texts
    with pytest.raises(ValueError, match="the rollout is not device-resident"):
        _check_on_device(types.SimpleNamespace(device_resident=False), types.SimpleNamespace(is_recurrent=False, dist_kind=0, cnn=1), False, "x")
    with pytest.raises(ValueError, match="the policy has a Discrete / MultiBinary action space"):
        _check_on_device(ro, types.SimpleNamespace(is_recurrent=False, dist_kind=1, cnn=1), False, "x")
    p = bare_policy(1, 16, "categorical", 5)
    with pytest.raises(NotImplementedError, match="reset_critic on a policy with the CNN base"):
        p.reset_critic((1, 84, 84))
    with pytest.raises(NotImplementedError, match="cannot be written in the reference's object layout \\(nn.Conv2d"):
        save_policy("/nonexistent/x.pt", p)
