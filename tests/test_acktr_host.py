"""CPU: A2C_ACKTR(acktr=True)'s host side (the alias package, the RMSprop-argument refusal) and a float64 numpy restatement of
the reference's ACKTR update (a2c/algo/a2c_acktr.py:52-102 with KFACOptimizer, a2c/algo/kfac.py) that reproduces every acktr_*
fixture (tools/gen_golden_acktr.py).  The GPU tests (tests/test_gpu_acktr.py) measure the kernels against the fixtures and
against this restatement at shapes too big for a fixture."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import load  # noqa: E402
from test_a2c_host import a2c_loss_grad, policy_slices  # noqa: E402

ACKTR_CASES = ["acktr_tiny", "acktr_default", "acktr_critic64", "acktr_multi"]
KFAC = dict(lr=0.25, momentum=0.9, stat_decay=0.99, kl_clip=0.001, damping=0.01, Tf=10)
# KFACOptimizer.modules in order (split_bias): (flat key, distinct A factor or None for an AddBias, distinct G factor).
# Distinct factors: A 0 obs, 1 actor h1, 2 actor h2, 3 critic h1, 4 critic h2; G 0 actor.0, 1 actor.2, 2 critic.0, 3 critic.2,
# 4 critic_linear, 5 dist.fc_mean, 6 dist.logstd
MODULES = [("aw1", 0, 0), ("ab1", None, 0), ("aw2", 1, 1), ("ab2", None, 1), ("cw1", 0, 2), ("cb1", None, 2),
           ("cw2", 3, 3), ("cb2", None, 3), ("vw", 4, 4), ("vb", None, 4), ("mw", 2, 5), ("mb", None, 5), ("ls", None, 6)]


def new_state():
    return {"mA": None, "mG": None, "eA": None, "eG": None, "buf": None, "steps": 0}


def acktr_update_restated(params, state, obs, actions, returns, eps, dims, vcoef, ecoef, kfac=KFAC, **loss_kw):
    """One A2C_ACKTR.update (acktr=True) on rollout arrays obs [T+1, N, O], actions [T, N, A], returns [T+1, N, 1] and value
    noise eps [T, N, 1], float64 -> (params1, losses[3], state); `state` (new_state()) carries the running factors, the
    eigenbases, the momentum buffer and steps.  a2c_acktr.py:72-100 and kfac.py:152-255 with Ts 1 and weight_decay 0."""
    O, A, H, Hc = dims
    obs = np.asarray(obs, np.float64)
    T, N = obs.shape[0] - 1, obs.shape[1]
    B = T * N
    sl, n = policy_slices(O, A, H, Hc)
    flat = np.asarray(params, np.float64)
    p = {k: flat[s].reshape(shape) for k, (s, shape) in sl.items()}
    x = obs[:T].reshape(-1, O)
    act = np.asarray(actions, np.float64).reshape(-1, A)
    losses, g = a2c_loss_grad(flat, x, act, np.asarray(returns)[:T].reshape(-1), dims, vcoef, ecoef, **loss_kw)
    # the sampled Fisher loss -mean(logp) - mean((v - (v + eps).detach())^2), back-propagated to every Linear output
    a1 = np.tanh(x @ p["aw1"].T + p["ab1"])
    a2 = np.tanh(a1 @ p["aw2"].T + p["ab2"])
    mu = a2 @ p["mw"].T + p["mb"]
    c1 = np.tanh(x @ p["cw1"].T + p["cb1"])
    c2 = np.tanh(c1 @ p["cw2"].T + p["cb2"])
    var = np.exp(2.0 * p["ls"])
    diff = act - mu
    gmu = -diff / var / B
    gls = -(diff * diff / var - 1.0) / B
    gv = 2.0 * np.asarray(eps, np.float64).reshape(-1, 1) / B
    za2 = (gmu @ p["mw"]) * (1.0 - a2 * a2)
    za1 = (za2 @ p["aw2"]) * (1.0 - a1 * a1)
    zc2 = (gv @ p["vw"]) * (1.0 - c2 * c2)
    zc1 = (zc2 @ p["cw2"]) * (1.0 - c1 * c1)
    fA = [u.T @ u / B for u in (x, a1, a2, c1, c2)]
    fG = [B * (u.T @ u) for u in (za1, za2, zc1, zc2, gv, gmu, gls)]
    sd = kfac["stat_decay"]
    first = state["steps"] == 0
    mA = [((f if first else m) * (sd / (1.0 - sd)) + f) * (1.0 - sd) for f, m in zip(fA, state["mA"] or fA)]
    mG = [((f if first else m) * (sd / (1.0 - sd)) + f) * (1.0 - sd) for f, m in zip(fG, state["mG"] or fG)]
    eA, eG = state["eA"], state["eG"]
    if state["steps"] % kfac["Tf"] == 0:
        def eig(m):
            d, q = np.linalg.eigh(m, UPLO="U")
            return d * (d > 1e-6), q
        eA, eG = [eig(m) for m in mA], [eig(m) for m in mG]
    one = (np.ones(1), np.ones((1, 1)))
    v = np.zeros(n)
    for key, fa, fg in MODULES:
        s, shape = sl[key]
        grad = g[s].reshape(shape[0], -1) if len(shape) == 2 else g[s].reshape(-1, 1)
        da, qa = one if fa is None else eA[fa]
        dg, qg = eG[fg]
        v1 = qg.T @ grad @ qa
        v2 = v1 / (dg[:, None] * da[None, :] + kfac["damping"])
        v[s] = (qg @ v2 @ qa.T).reshape(-1)
    vg = float(np.sum(v * g)) * kfac["lr"] ** 2
    nu = min(1.0, np.sqrt(kfac["kl_clip"] / vg))
    buf = nu * v if first else kfac["momentum"] * state["buf"] + nu * v
    p1 = flat - kfac["lr"] * (1.0 - kfac["momentum"]) * buf
    new = {"mA": mA, "mG": mG, "eA": eA, "eG": eG, "buf": buf, "steps": state["steps"] + 1}
    return p1, np.array(losses), new


def packed_factors(state, dims):
    """m_aa / m_gg of the 13 modules, packed in module order (the fixtures' and sg_acktr_get_state's layout)."""
    aa = [np.ones((1, 1)) if fa is None else state["mA"][fa] for _, fa, _ in MODULES]
    gm = [state["mG"][fg] for _, _, fg in MODULES]
    return np.concatenate([m.reshape(-1) for m in aa]), np.concatenate([m.reshape(-1) for m in gm])


def dims_of(m):
    return (m["O"], m["A"], m["H"], m["Hc"])


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def restate_fixture(g):
    """Every update of a fixture from its own starting parameters, the K-FAC state carried -> [(params1, losses, state)].
    The fixtures' float64 run is the reference after .double(), where log(sqrt(2 pi)) is the exact double (it enters the losses
    alone, by 1.56e-8 per action dimension; the float32 run is compared at 1e-5), so the fixtures are restated with that one;
    everywhere else the restatement keeps the float32 value, like every float64 arbiter (tests/autograd_ref.py)."""
    m = g["meta"]
    st, out = new_state(), []
    for j in range(m["iters"]):
        pre = f"it{j}_"
        p1, losses, st = acktr_update_restated(g[pre + "params0"], st, g[pre + "obs"], g[pre + "actions"], g[pre + "returns"],
                                               g[pre + "eps"], dims_of(m), m["value_loss_coef"], m["entropy_coef"],
                                               half_log_2pi=0.5 * np.log(2.0 * np.pi))
        out.append((p1, losses, st))
    return out


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", ACKTR_CASES)
def test_restatement_reproduces_the_float64_reference(name):
    """The restatement against the reference run at float64 with the same value noise: 1e-10 relative on every update."""
    g = load(name)
    for j, (p1, losses, _) in enumerate(restate_fixture(g)):
        pre = f"it{j}_"
        dp_ref = g[pre + "params1_f64"] - g[pre + "params0"].astype(np.float64)
        assert rel_l2(p1 - g[pre + "params0"], dp_ref) < 1e-10, j
        assert np.allclose(losses, g[pre + "losses_f64"], rtol=1e-10, atol=1e-14), j


@pytest.mark.parametrize("name", ACKTR_CASES)
def test_restatement_matches_the_float32_reference(name):
    """... and against the reference's own float32 run: Delta p within 1e-4 relative L2, the factors within 1e-5 max|m|."""
    g = load(name)
    for j, (p1, losses, st) in enumerate(restate_fixture(g)):
        pre = f"it{j}_"
        p0 = g[pre + "params0"].astype(np.float64)
        assert rel_l2(p1 - p0, g[pre + "params1"] - p0) < 1e-4, j
        assert np.allclose(losses, g[pre + "losses"], rtol=1e-5, atol=1e-6), j
        aa, gm = packed_factors(st, dims_of(g["meta"]))
        for mine, ref in ((aa, g[pre + "m_aa"]), (gm, g[pre + "m_gg"])):
            assert np.max(np.abs(mine - ref)) <= 1e-5 * np.max(np.abs(ref)), j
        assert rel_l2(st["buf"], g[pre + "momentum"]) < 1e-4, j


def test_multi_fixture_refreshes_the_eigenbases_twice():
    """acktr_multi spans steps 0..11: eigendecompositions at steps 0 and 10, and the LR schedule's writes did nothing."""
    g = load("acktr_multi")
    m = g["meta"]
    assert m["iters"] == 12 and m["Tf"] == 10 and m["lr_sched"]
    assert [j for j in range(m["iters"]) if j % m["Tf"] == 0] == [0, 10]


def test_alias_package_binds_both_import_forms_and_refuses_rmsprop_arguments():
    """Both import forms of a2c/main.py bind to the library's class, and acktr=True with RMSprop arguments is refused there."""
    import subprocess
    code = ("import pytest\n"
            "from third_party.a2c_ppo_acktr import algo\n"
            "from third_party.a2c_ppo_acktr.algo.a2c_acktr import A2C_ACKTR\n"
            "from simgan_amd.algo import A2C_ACKTR as ours\n"
            "assert algo.A2C_ACKTR is ours and A2C_ACKTR is ours\n"
            "class Policy: pass\n"
            "for kw in (dict(lr=7e-4), dict(eps=1e-5), dict(alpha=0.99), dict(max_grad_norm=0.5)):\n"
            "    with pytest.raises(NotImplementedError, match='K-FAC'):\n"
            "        algo.A2C_ACKTR(Policy(), 0.5, 0.01, acktr=True, **kw)\n")
    subprocess.run([sys.executable, "-s", "-c", code], cwd=ROOT, check=True, timeout=300)


def test_rmsprop_arguments_are_refused_with_acktr_before_any_device_work():
    from simgan_amd.algo.a2c_acktr import A2C_ACKTR

    class Policy:
        pass

    for k, v in (("lr", 7e-4), ("eps", 1e-5), ("alpha", 0.99), ("max_grad_norm", 0.5)):
        with pytest.raises(NotImplementedError, match=f"K-FAC.*|{k}") as exc:
            A2C_ACKTR(Policy(), 0.5, 0.01, acktr=True, **{k: v})
        assert k in str(exc.value) and "K-FAC" in str(exc.value)


def test_kfac_view_constants():
    """agent.optimizer of an ACKTR agent: KFACOptimizer's constructor defaults (a2c/main.py:205 reads lr)."""
    from simgan_amd.algo.a2c_acktr import KFAC_DEFAULTS
    assert KFAC_DEFAULTS == dict(lr=0.25, momentum=0.9, stat_decay=0.99, kl_clip=0.001, damping=1e-2, weight_decay=0, Ts=1, Tf=10)


def test_abi_declares_the_acktr_entry_points():
    from simgan_amd import _lib
    for name in ("sg_acktr_create", "sg_acktr_set_value_noise", "sg_acktr_get_state"):
        assert name in _lib.PROTOTYPES
        assert name in open(os.path.join(ROOT, "include", "simgan_hip.h")).read()
    assert [f for f, _ in _lib.ACKTRConfig._fields_] == ["value_loss_coef", "entropy_coef", "lr", "momentum", "stat_decay",
                                                          "kl_clip", "damping", "Tf"]


def test_fixtures_stay_small():
    for name in ACKTR_CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < (1 << 20)


# ------------------------------------------------------------------ checkpoints saved after ACKTR
def test_reference_acktr_checkpoint_reads_to_the_plain_flat_parameters():
    """ckpt_policy_acktr.pt (tools/gen_golden_acktr.py:gen_ckpt) is `torch.save([actor_critic, ob_rms])` after an ACKTR update:
    SplitBias modules and pickled K-FAC hooks.  The allowlisted reader folds the keys back to the plain layout."""
    from simgan_amd import checkpoint as ck
    g = load("ckpt_policy_acktr")
    r = ck.read_reference_checkpoint(os.path.join(ROOT, "tests", "golden", "ckpt_policy_acktr.pt"))
    m = g["meta"]
    assert (r["class_name"], r["obs_dim"], r["act_dim"], r["hidden"]) == ("Policy", m["O"], m["A"], m["H"])
    assert list(r["state_dict"])[:2] == ["base.actor.0.weight", "base.actor.0.bias"]
    assert r["state_dict"]["base.actor.0.bias"].shape == (m["H"],)
    flat = np.concatenate([v.reshape(-1) for v in r["state_dict"].values()])
    assert np.array_equal(flat, g["flat"])
    assert np.array_equal(r["ob_rms"]["mean"], g["rms_mean"]) and r["ob_rms"]["count"] == g["rms_count"]


def test_bare_torch_load_of_an_acktr_checkpoint_through_the_alias_package():
    """a2c/main.py:81-83's bare torch.load resolves SplitBias / KFACOptimizer to the inert holders of
    third_party/a2c_ppo_acktr/algo/kfac.py; the policy's pickled state gives the expected parameters (the device twin is
    built on first use: tests/test_gpu_acktr.py).  In a child process, as the other alias-package tests."""
    import subprocess
    code = ("import numpy as np, torch\n"
            "from simgan_amd.checkpoint import policy_from_module_state\n"
            "import third_party.a2c_ppo_acktr.algo.kfac as kfac\n"
            f"g = np.load({os.path.join(ROOT, 'tests', 'golden', 'ckpt_policy_acktr.npz')!r})\n"
            f"ac, rms = torch.load({os.path.join(ROOT, 'tests', 'golden', 'ckpt_policy_acktr.pt')!r}, map_location='cpu', "
            "weights_only=False)\n"
            "assert type(ac).__module__ == 'third_party.a2c_ppo_acktr.model', type(ac)\n"
            "dims, sd = policy_from_module_state('Policy', ac.__dict__['_pending'])\n"
            "assert np.array_equal(np.concatenate([v.reshape(-1) for v in sd.values()]), g['flat'])\n"
            "hooks = [h for m in ac.__dict__['_pending']['_modules']['base'].__dict__['_modules']['actor'].__dict__['_modules']"
            "['0'].__dict__['_modules'].values() for h in m.__dict__['_forward_pre_hooks'].values()]\n"
            "assert hooks and all(isinstance(h.__self__, kfac.KFACOptimizer) and h(None, None) is None for h in hooks)\n")
    subprocess.run([sys.executable, "-s", "-c", code], cwd=ROOT, check=True, timeout=300)


class _Getattr:
    def __init__(self, target, name):
        self.target, self.name = target, name

    def __reduce__(self):
        return (getattr, (self.target, self.name))


def _reference_kfac_instance(monkeypatch):
    """An object that pickles by reference to a reference class (a2c_ppo_acktr.algo.kfac.KFACOptimizer, a stub root of the
    reader) without importing the alias package into this process."""
    import types
    for name in ("a2c_ppo_acktr", "a2c_ppo_acktr.algo", "a2c_ppo_acktr.algo.kfac"):
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    cls = type("KFACOptimizer", (object,), {"__module__": "a2c_ppo_acktr.algo.kfac"})
    sys.modules["a2c_ppo_acktr.algo.kfac"].KFACOptimizer = cls
    return cls()


def test_checkpoint_getattr_on_anything_but_a_reference_kfac_hook_is_refused(tmp_path, monkeypatch):
    """The reader resolves `getattr` to a guard: a crafted file that applies it to a real object (an allowlisted class or
    container, even with a hook's name) or asks a reference stand-in for another name is refused before anything runs."""
    import collections
    import pickle
    import torch
    from simgan_amd import checkpoint as ck
    ref = _reference_kfac_instance(monkeypatch)
    for i, payload in enumerate((_Getattr(collections.OrderedDict, "fromkeys"), _Getattr({}, "update"),
                                 _Getattr(collections.OrderedDict, "_save_input"), [None, _Getattr(ref, "__class__")],
                                 _Getattr(ref, "step"), _Getattr(ref, "_save_input_"))):
        for legacy in (True, False):
            path = str(tmp_path / f"ga{i}_{int(legacy)}.pt")
            torch.save([payload, None], path, _use_new_zipfile_serialization=not legacy)
            with pytest.raises(pickle.UnpicklingError, match="refusing to resolve"):
                ck.read_reference_checkpoint(path)
    stub = ck._stub_class("a2c_ppo_acktr.algo.kfac", "KFACOptimizer")()
    assert ck._guarded_getattr(stub, "_save_input")(None, None) is None
    assert ck._guarded_getattr(stub, "_save_grad_output")(None, None, None) is None


def test_checkpoint_fixture_stays_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ckpt_policy_acktr.pt")) < (1 << 20)
