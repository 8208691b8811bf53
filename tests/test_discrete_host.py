"""CPU: Policy on Discrete / MultiBinary action spaces, everything that needs no device.

  * the reference's own gradients (tests/golden/discrete_*.npz, tools/gen_golden_discrete.py: .grad of one PPO step with both
    value losses and of one A2C step) against tests/discrete_ref.py -- float64, forward-only, differentiated by autograd --
    per parameter block within 1e-4, and the fixtures' evaluate_actions / losses with them;
  * the test of that test: three deliberately wrong restatements (the entropy's gradient dropped, +p in place of a - p, the
    class index off by one) miss the same bound by far;
  * the numpy samplers the GPU tests compare against: the reference's deterministic actions, and frequencies;
  * the host-side refusals, each with its own message;
  * RolloutStorage's int64 actions through insert, the generator and both directions of the device sync (the library's rollout
    calls stood in for by a float32 store);
  * checkpoints in the reference's object layout: the reference-written files are read, what this package writes reads back
    the same, and -- where a checkout of the reference is present -- the reference itself loads it and computes the same."""
import ctypes as C
import os
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest

import discrete_ref as dr
from helpers import GOLDEN, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-4
DIST = {"categorical": dr.CATEGORICAL, "bernoulli": dr.BERNOULLI}


def fixture_case(name):
    g = dr.load(name)
    m = g["meta"]
    T, N, O = m["T"], m["N"], m["O"]
    dist = DIST[m["dist"]]
    return g, m, dist, dr.param_shapes(O, m["K"], m["H"]), dict(
        obs=g["obs"][:-1].reshape(T * N, O), actions=g["actions"].reshape(T * N, -1), old_logp=g["action_log_probs"].reshape(-1),
        value_preds=g["value_preds"][:-1].reshape(-1), returns=g["returns"][:-1].reshape(-1))


def ref_grads(name, fault=None):
    """-> {key: (float64 restatement's flat gradient, losses)} for the three gradients a fixture holds"""
    g, m, dist, shapes, c = fixture_case(name)
    kw = dict(clip=m["clip_param"], vcoef=m["value_loss_coef"], ecoef=m["entropy_coef"], fault=fault)
    out = {}
    for key, uc in (("ppo_clipped", True), ("ppo_plain", False)):
        out[key] = dr.ppo_grad(dist, shapes, g["params0"], c["obs"], c["actions"], c["old_logp"], c["value_preds"], c["returns"],
                               use_clipped=uc, **kw)
    out["a2c"] = dr.a2c_grad(dist, shapes, g["params0"], c["obs"], c["actions"], c["returns"], vcoef=m["value_loss_coef"],
                             ecoef=m["entropy_coef"], fault=fault)
    return g, shapes, out


@pytest.mark.parametrize("name", dr.FIXTURES)
def test_reference_gradients_match_the_float64_restatement(name):
    g, shapes, out = ref_grads(name)
    for key, (grad, losses) in out.items():
        d = dr.block_distances(g["grad_" + key], grad, shapes)
        assert max(d.values()) <= BOUND, (name, key, {k: v for k, v in d.items() if v > BOUND})
        assert_close(g["losses_" + key if key != "a2c" else "losses_a2c_grad"], losses, what=f"{name} {key}: losses")


@pytest.mark.parametrize("name", dr.FIXTURES)
def test_fixture_forward_matches_the_float64_restatement(name):
    g, m, dist, shapes, c = fixture_case(name)
    v, lp, ent, z = dr.evaluate(dist, shapes, g["params0"], c["obs"], c["actions"])
    assert_close(g["eval_value"].reshape(-1), v, what="value")
    assert_close(g["eval_logp"].reshape(-1), lp, what="logp")
    assert_close(g["eval_entropy"], ent.mean(), what="entropy")
    assert_close(g["logits"], z, what="logits")
    assert float(g["mode_margin"]) > 1e-4
    mode = z.argmax(1).reshape(-1, 1) if dist == dr.CATEGORICAL else (z > 0).astype(np.float32)
    assert np.array_equal(g["det_action"], mode) and g["det_action"].dtype == (np.int64 if dist == dr.CATEGORICAL else np.float32)
    assert g["actions"].dtype == (np.int64 if dist == dr.CATEGORICAL else np.float32)


# (a Bernoulli action has no class index to be off by one)
FAULTS = [(n, f) for n in ("discrete_k17", "discrete_b5") for f in ("no_entropy_gradient", "p_for_a_minus_p", "index_off_by_one")
          if not (n == "discrete_b5" and f == "index_off_by_one")]


@pytest.mark.parametrize("name,fault", FAULTS)
def test_wrong_restatements_fail_the_bound(name, fault):
    """The bound can tell: each fault moves at least one parameter block of every gradient it touches by far more than 1e-4."""
    g, shapes, out = ref_grads(name, fault=fault)
    for key, (grad, _) in out.items():
        d = dr.block_distances(g["grad_" + key], grad, shapes)
        assert max(d.values()) > 30 * BOUND, (name, key, fault, max(d.values()))
        # ... and the critic's blocks, which none of the faults touches, still agree
        assert max(v for k, v in d.items() if k.startswith("base.critic")) <= BOUND


@pytest.mark.parametrize("dist,K", [(dr.CATEGORICAL, 2), (dr.CATEGORICAL, 17), (dr.BERNOULLI, 5)])
def test_numpy_samplers(dist, K):
    """The inverse CDF / u < p restatement: clamped at u -> 1, the first class at u = 0, frequencies within 5 sigma of p."""
    rng = np.random.default_rng(3)
    z = rng.standard_normal((1, K)).astype(np.float32) * 1.5
    p = dr.probs32(dist, z).astype(np.float64)[0]
    if dist == dr.CATEGORICAL:
        assert abs(p.sum() - 1.0) < 1e-6
        assert dr.sample(dist, z, [[0.0]])[0, 0] == 0 and dr.sample(dist, z, [[0.99999994]])[0, 0] == K - 1
    n = 65536
    u = rng.random((n, 1 if dist == dr.CATEGORICAL else K)).astype(np.float32)
    a = dr.sample(dist, np.repeat(z, n, 0), u)
    freq = np.bincount(a[:, 0], minlength=K) / n if dist == dr.CATEGORICAL else a.mean(0)
    assert np.all(np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / n) + 1e-9)


@pytest.mark.parametrize("dist,spec", [(d, s) for d in (dr.CATEGORICAL, dr.BERNOULLI) for s in dr.SHAPES[d]])
def test_gradient_cases_cover_the_three_surrogate_branches(dist, spec):
    """What tests/test_gpu_discrete.py relies on, asserted where it is cheap: every case has rows clipped low, inside and clipped
    high, none within 1e-4 of a clip boundary; the saturated ones have logit gaps of about 15."""
    for rows in dr.ROWS:
        for saturated in (False, True):
            c = dr.make_case(dist, *spec, rows, seed=11, saturated=saturated)
            lo, mid, hi, margin = dr.surrogate_branches(c)
            assert lo >= 2 and mid >= 2 and hi >= 2 and margin > 1e-4, (rows, saturated, lo, mid, hi, margin)
            if saturated:
                z = dr.evaluate(dist, c["shapes"], c["params"], c["obs"], c["actions"])[3]
                gap = np.median(np.sort(z, 1)[:, -1] - np.sort(z, 1)[:, -2]) if dist == dr.CATEGORICAL else np.median(np.abs(z))
                assert 7.5 < gap < 25.0, gap   # (a median over as few as 16 rows, after the perturbation)


# ------------------------------------------------------------------------------------------------- refusals
def test_host_side_refusals_for_a_discrete_policy():
    """Each with its own message, before any device object is touched; reset_critic is not among them."""
    import simgan_amd as sg
    from simgan_amd.ensemble import PolicyEnsemble
    from simgan_amd.storage import RolloutStorage
    pol = types.SimpleNamespace(is_recurrent=False, KIND=0, dist_kind=dr.CATEGORICAL)
    with pytest.raises(NotImplementedError, match="K-FAC's Fisher sampling is built for the Gaussian head"):
        sg.algo.A2C_ACKTR(pol, 0.5, 0.01, acktr=True)
    with pytest.raises(NotImplementedError, match="mirror-symmetry loss: it compares action means"):
        sg.algo.PPO(pol, 0.2, 1, 1, 0.5, 0.0, symmetry_coef=1.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5, mirror_obs=np.eye(3),
                    mirror_act=np.eye(1))
    with pytest.raises(NotImplementedError, match="PolicyEnsemble: members with Box action spaces only"):
        PolicyEnsemble([pol])
    for space in (dr.Discrete(3), dr.MultiBinary(3)):
        with pytest.raises(NotImplementedError, match="the GRU base is built with the Gaussian head"):
            sg.Policy((4,), space, base_kwargs={"recurrent": True, "hidden_size": 8})
    ro = RolloutStorage.__new__(RolloutStorage)
    ro.box_actions, ro.num_processes = False, 4
    with pytest.raises(NotImplementedError, match="enable_dup_sym: a mirror-augmented rollout mirrors actions through a linear map"):
        ro.enable_dup_sym(np.eye(3), np.eye(1))
    p = sg.Policy.__new__(sg.Policy)
    p.__dict__.update(_dist_kind=dr.BERNOULLI, n_out=3)
    with pytest.raises(ValueError, match="no log-std to reset"):
        p.reset_variance(dr.MultiBinary(3), -1.0)
    with pytest.raises(NotImplementedError, match="Box, Discrete and MultiBinary are built"):
        sg.Policy((4,), types.SimpleNamespace(), base_kwargs={"hidden_size": 8})
    with pytest.raises(ValueError, match="exact below 2\\^24"):
        sg.Policy((4,), dr.Discrete(2 ** 24), base_kwargs={"hidden_size": 8})


def test_param_shapes_end_with_the_linear_head():
    import simgan_amd as sg
    for dist, K in ((dr.CATEGORICAL, 17), (dr.BERNOULLI, 5)):
        p = sg.Policy.__new__(sg.Policy)
        p.__dict__.update(_dist_kind=dist, n_out=K, obs_dim=11, act_dim=1 if dist == dr.CATEGORICAL else K, hidden_size=32, critic_hidden=32,
                          recurrent=False)
        assert [(n, tuple(s)) for n, s in p.param_shapes()] == dr.param_shapes(11, K, 32)


# ------------------------------------------------------------------------------------------------- int64 rollout actions
class _FakeRolloutLib(object):
    """The four rollout calls RolloutStorage makes, over a float32 store per field: what the device twin is to the host code."""

    def __init__(self):
        self.fields, self.created = {}, None

    def sg_rollout_create(self, ctx, T, N, O, A, F, out):
        self.created = (T, N, O, A, F)
        return 0

    def sg_rollout_destroy(self, h):
        return 0

    def sg_rollout_upload(self, h, field, ptr, count):
        self.fields[field] = np.ctypeslib.as_array(ptr, shape=(count,)).copy()
        assert self.fields[field].dtype == np.float32
        return 0

    def sg_rollout_download(self, h, field, ptr, count):
        np.ctypeslib.as_array(ptr, shape=(count,))[:] = self.fields[field]
        return 0


def test_discrete_rollout_keeps_int64_actions_on_the_host():
    """a2c/storage.py:42-48: actions [T, N, 1] int64 for Discrete.  insert() takes the policy's int64 actions, the generator hands
    int64 minibatches out, the device sees float32 class indices, and a download writes them back into the int64 tensor."""
    from simgan_amd import _lib
    from simgan_amd.storage import RolloutStorage
    lib = _FakeRolloutLib()
    ctx = types.SimpleNamespace(lib=lib, h=None)
    T, N, O, K = 3, 4, 5, 130
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (no device: the host tensors fall back to pageable memory)
        ro = RolloutStorage(T, N, (O,), dr.Discrete(K), 1, 1, ctx=ctx)
        mb = RolloutStorage(T, N, (O,), dr.MultiBinary(6), 1, 1, ctx=_FakeCtx())
    assert lib.created == (T, N, O, 1, 1)
    assert tuple(ro.actions.shape) == (T, N, 1) and str(ro.actions.dtype).endswith("int64")
    assert tuple(mb.actions.shape) == (T, N, 6) and str(mb.actions.dtype).endswith("float32")
    rng = np.random.default_rng(0)
    acts = rng.integers(0, K, size=(T, N, 1))
    for t in range(T):
        ro.insert(np.zeros((N, O), np.float32), np.zeros((N, 1), np.float32), _lib.as_i64(acts[t]) if t else ro.actions.new_tensor(acts[t]),
                  np.zeros((N, 1), np.float32), np.zeros((N, 1), np.float32), np.zeros((N, 1), np.float32), np.ones((N, 1), np.float32),
                  np.ones((N, 1), np.float32))
    assert np.array_equal(np.asarray(ro.actions), acts)
    batches = list(ro.feed_forward_generator(None, num_mini_batch=2, perm=np.arange(T * N)[::-1].copy()))
    got = np.concatenate([np.asarray(b[2]) for b in batches])
    assert got.dtype == np.int64 and np.array_equal(got, acts.reshape(-1, 1)[::-1])
    ro.sync_to_device([_lib.F_ACTIONS])
    dev = lib.fields[_lib.F_ACTIONS]
    assert dev.dtype == np.float32 and np.array_equal(dev, acts.reshape(-1).astype(np.float32))
    lib.fields[_lib.F_ACTIONS] = ((dev + 1) % K).astype(np.float32)
    ro.sync_from_device([_lib.F_ACTIONS])
    assert str(ro.actions.dtype).endswith("int64") and np.array_equal(np.asarray(ro.actions), (acts + 1) % K)
    ro.actions = ro.actions.float()
    with pytest.raises(TypeError, match="must stay a contiguous int64 host tensor"):
        ro.sync_to_device([_lib.F_ACTIONS])


class _FakeCtx(object):
    def __init__(self):
        self.lib, self.h = _FakeRolloutLib(), None


# ------------------------------------------------------------------------------------------------- checkpoints
@pytest.mark.parametrize("tag", ["categorical", "bernoulli"])
def test_reference_checkpoints_are_read_and_written(tag, tmp_path):
    from simgan_amd.checkpoint import read_reference_checkpoint, save_reference_checkpoint
    g = dr.load(f"ckpt_policy_{tag}")
    m = g["meta"]
    path = os.path.join(GOLDEN, f"ckpt_policy_{tag}.pt")
    blob = open(path, "rb").read()
    assert b"def forward(" not in blob and b"import torch" not in blob, "the fixture carries source text"
    ck = read_reference_checkpoint(path)
    assert ck["kind"] == "mlp_" + tag and ck["dist"] == DIST[tag] and ck["class_name"] == "Policy"
    assert (ck["obs_dim"], ck["n_out"], ck["hidden"], ck["act_dim"]) == (m["O"], m["K"], m["H"], 1 if tag == "categorical" else m["K"])
    assert list(ck["state_dict"]) == m["names"] and m["names"][-2:] == ["dist.linear.weight", "dist.linear.bias"]
    assert np.array_equal(np.concatenate([v.reshape(-1) for v in ck["state_dict"].values()]), g["flat"])
    # the restatement on the checkpoint's weights gives the reference's deterministic act
    shapes = dr.param_shapes(m["O"], m["K"], m["H"])
    v, lp, _, z = dr.evaluate(DIST[tag], shapes, g["flat"], g["obs"], g["action"])
    assert_close(g["value"].reshape(-1), v, what="value")
    assert_close(g["logp"].reshape(-1), lp, what="logp")
    # written in the reference's layout, it reads back the same
    out = str(tmp_path / "w.pt")
    save_reference_checkpoint(out, ck["kind"], ck["state_dict"])
    back = read_reference_checkpoint(out)
    assert back["kind"] == ck["kind"] and list(back["state_dict"]) == m["names"]
    for k in m["names"]:
        assert np.array_equal(back["state_dict"][k], ck["state_dict"][k]), k
    # the two heads have the same parameters: the dist module's class is what tells them apart
    other = "bernoulli" if tag == "categorical" else "categorical"
    save_reference_checkpoint(out, "mlp_" + other, ck["state_dict"])
    assert read_reference_checkpoint(out)["kind"] == "mlp_" + other


REFERENCE = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "third_party", "a2c_ppo_acktr")), reason="no checkout of the reference")
@pytest.mark.parametrize("tag", ["categorical", "bernoulli"])
def test_the_real_reference_loads_what_this_package_writes(tag, tmp_path):
    """save_reference_checkpoint's file through the reference's own torch.load (in a child process, tools/ref_import.py): its
    Policy.act(deterministic=True) on the fixture's observations gives the fixture's numbers."""
    from simgan_amd.checkpoint import read_reference_checkpoint, save_reference_checkpoint
    ck = read_reference_checkpoint(os.path.join(GOLDEN, f"ckpt_policy_{tag}.pt"))
    out = str(tmp_path / "w.pt")
    save_reference_checkpoint(out, ck["kind"], ck["state_dict"])
    code = ("import sys, numpy as np, torch\n"
            f"sys.path.insert(0, {os.path.join(ROOT, 'tools')!r})\n"
            "from ref_import import import_reference\n"
            "ns = import_reference()\n"
            f"p, rms = torch.load({out!r}, weights_only=False)\n"
            f"g = np.load({os.path.join(GOLDEN, f'ckpt_policy_{tag}.npz')!r})\n"
            f"assert type(p.dist).__name__ == {tag.capitalize()!r} and type(p).__module__.startswith('third_party.'), type(p.dist)\n"
            "with torch.no_grad():\n"
            "    v, a, lp, _ = p.act(torch.from_numpy(g['obs']), None, None, deterministic=True)\n"
            "assert np.array_equal(a.numpy(), g['action']) and a.numpy().dtype == g['action'].dtype\n"
            "assert np.allclose(v.numpy(), g['value'], rtol=1e-6, atol=1e-7) and np.allclose(lp.numpy(), g['logp'], rtol=1e-6, atol=1e-7)\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-1000:], r.stderr[-3000:])
