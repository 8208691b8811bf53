"""CPU: the recurrent CNN base without a device -- tests/cnn_gru_ref.py (the arbiter of tests/test_gpu_cnn_gru.py) held to its own
conditions, and the Python layer's layout, generator and refusals.

  1 arbiter     every committed seed's admission re-checked (kink margin, branch margins, torch's float32 gradient within 0.5 RTOL
                of the float64 one per block); in which gradient runs the clip at max_grad_norm = 0.5 acts; where a reference
                checkout is present, the arbiter against the reference's own Policy(... recurrent=True): state_dict keys,
                evaluate_actions, and the .grad its PPO.update leaves (a child process; skipped elsewhere)
  2 defects     five injected defects, each on the references alone, each moving some block by at least 10 RTOL
  3 layout      Policy.param_shapes' names and order; construction is opt-in and the default refusal keeps its text
  4 generator   recurrent_generator on an image rollout with H > 1 against a restatement; it still raises with H = 1
  5 refusals    A2C_ACKTR in every mode, diagnostics, PolicyEnsemble, symmetry_coef > 0, world > 1, saving"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cnn_gru_ref as gr
import cnn_ref as cr
from cnn_ref import ar
from helpers import GOLDEN, RTOL, assert_close, load

HW = 84


class Discrete(object):
    def __init__(self, n):
        self.n = int(n)


class Box(object):
    def __init__(self, shape):
        self.shape = tuple(shape)


# ------------------------------------------------------------------------------------------------- 1 the arbiter
@pytest.mark.parametrize("key", list(gr.SEEDS), ids=["-".join(map(str, k)) for k in gr.SEEDS])
def test_every_seed_is_admitted_on_the_references_alone(key):
    c = gr.case(*key)
    km, exempted, branch = gr.margins(c)
    assert km >= cr.KINK_FACTOR and branch >= cr.MARGIN, (c.tag, km, branch)
    assert (exempted > 0) == (c.head == "fc_zero")
    d32 = gr.admitted(key)[2]
    assert max(d32.values()) <= 0.5 * RTOL, (c.tag, d32)
    # the masks reach what they are meant to reach, the state of slot 0 is not zero
    m = c.masks[:-1, :, 0]
    assert m[0, 0] == 0 and np.abs(c.hxs[0]).min() > 0
    if c.T >= 4:
        assert m[1, -1] == 0 and m[2, -1] == 0
    if c.N >= 3:
        assert not m[:, 2].any()
    if c.head == "fc_zero":      # FC units 0, 1 are exactly 0 in every row; torch's gradient is exactly 0 at their rows, biases and
        zeros = set(gr.admitted(key)[3].tolist())      # the matching weight_ih columns, in both precisions
        k, Hs = gr.n_gru(c.Hs), c.Hs
        wf, _ = gr.cg._block(cr.param_shapes(c.C, Hs, c.dist, c.P), "base.main.7.weight")
        assert all(k + wf.start + i in zeros for i in range(gr.ZERO_UNITS * 1568))
        assert all(row * Hs + u in zeros for row in range(3 * Hs) for u in range(gr.ZERO_UNITS))


def test_where_the_clip_at_one_half_acts():
    for key, M in gr.GRAD_CASES.items():
        c = gr.case(*key)
        perm = np.random.default_rng(gr.PERM_SEED).permutation(c.N)
        for use_clipped in (True, False):
            acts = [cr.clip_factor(gr.case_grad(c, envs, use_clipped)[0], 0.5) < 1.0 for envs in gr.step_envs(key, M, perm)]
            assert all(acts) if key not in gr.CLIP_INACTIVE else not any(acts), (key, use_clipped, acts)
    assert len(gr.CLIP_INACTIVE) == 1


@pytest.mark.skipif(not ar.reference_present(), reason="the reference checkout is not on this machine")
def test_the_arbiter_against_the_references_own_policy():
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "cnn_gru_ref.py"), "--tier2"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("TIER2 ")][-1]
    res = json.loads(line[len("TIER2 "):])
    assert len(res) == 2 * len(gr.TIER2)
    # Categorical: autograd_ref's bounds as they stand.  Gaussian: the arbiter takes 0.5 log(2 pi) at its float32 value (the library's
    # and torch-float32's constant, tests/autograd_ref.py CONVENTION), the reference's .double() policy at the double's: every log-prob is
    # shifted by exactly A * |f32(c) - c|, the entropy likewise, so the ratio -- and with it the action loss and every gradient --
    # moves by a relative exp(shift) - 1 ~ shift.  Twice the shift bounds all three.
    shift = 3 * abs(float(np.float32(0.5 * np.log(2 * np.pi))) - 0.5 * np.log(2 * np.pi))
    for label, r in res.items():
        assert r["keys_equal"], label
        extra = 2 * shift if "gaussian" in label else 0.0
        assert r["forward"] <= ar.BOUND + extra and r["worst"] <= ar.BOUND + extra and r["loss_error"] <= ar.LOSS_ATOL + extra, (label, r)


# ------------------------------------------------------------------------------------------------- 2 injected defects
@pytest.mark.parametrize("fault", gr.FAULTS)
def test_injected_defects_are_seen(fault):
    key = (1, 16, "categorical", 5, 4, 4)
    c = gr.case(*key)
    g = gr.admitted(key)[0]
    gf, _ = gr.case_grad(c, fault=fault)
    d = cr.block_distances(gf, g, c.shapes)
    assert max(d.values()) >= 10 * RTOL, (fault, d)


# ------------------------------------------------------------------------------------------------- 3 layout and construction
def _spy_create(monkeypatch):
    import simgan_amd as sg
    calls = []

    def create(self, *a, **kw):
        calls.append((a, kw))
        self.__dict__.update(cnn=kw.get("cnn") or 0, recurrent=bool(kw.get("recurrent")), _dist_kind=kw.get("dist") or 0, n_out=kw.get("n_out") or a[1],
                             obs_dim=a[0], act_dim=a[1], hidden_size=a[2], critic_hidden=a[2])
    monkeypatch.setattr(sg.Policy, "_create", create)
    monkeypatch.setattr(sg.Policy, "_init_params", lambda self, rng: None)
    return sg, calls


def test_construction_is_opt_in_and_the_default_refusal_keeps_its_text(monkeypatch):
    sg, calls = _spy_create(monkeypatch)
    monkeypatch.delenv("SG_RECURRENT_CNN", raising=False)
    kw = dict(base_kwargs={"recurrent": True, "hidden_size": 16})
    old = "Policy on image observations with base_kwargs=\\{'recurrent': True\\}: the CNN base is built feed-forward only \\(a recurrent CNN base is not\\)"
    with pytest.raises(NotImplementedError, match=old):
        sg.Policy((4, HW, HW), Discrete(6), **kw)
    with pytest.raises(NotImplementedError, match=old):
        sg.Policy((4, HW, HW), Discrete(6), recurrent_cnn=False, **kw)
    assert not calls
    p = sg.Policy((4, HW, HW), Discrete(6), recurrent_cnn=True, **kw)
    monkeypatch.setenv("SG_RECURRENT_CNN", "1")
    sg.Policy((2, HW, HW), Box((3,)), **kw)      # the environment switch, read at construction
    with pytest.raises(NotImplementedError, match=old):
        sg.Policy((4, HW, HW), Discrete(6), recurrent_cnn=False, **kw)      # the keyword wins
    assert len(calls) == 2 and all(k["recurrent"] is True for _, k in calls) and [k["cnn"] for _, k in calls] == [4, 2]
    assert p.is_recurrent and p.recurrent_hidden_state_size == 16
    with pytest.raises(NotImplementedError, match="MultiBinary action space: the CNN base is built with the"):
        class MultiBinary(object):
            shape = (3,)
        sg.Policy((1, HW, HW), MultiBinary(), recurrent_cnn=True, **kw)
    # the feed-forward CNN base is what it was
    q = sg.Policy((4, HW, HW), Discrete(6), base_kwargs={"hidden_size": 16})
    assert not q.is_recurrent and q.recurrent_hidden_state_size == 1
    assert [(n, tuple(s)) for n, s in q.param_shapes()] == cr.param_shapes(4, 16, "categorical", 6)


@pytest.mark.parametrize("dist,P", [("categorical", 6), ("gaussian", 3)])
def test_param_shapes_speak_the_references_order(monkeypatch, dist, P):
    sg, _ = _spy_create(monkeypatch)
    p = sg.Policy((4, HW, HW), Discrete(P) if dist == "categorical" else Box((P,)), base_kwargs={"recurrent": True, "hidden_size": 24},
                  recurrent_cnn=True)
    got = [(n, tuple(s)) for n, s in p.param_shapes()]
    assert got == gr.param_shapes(4, 24, dist, P)
    names = [n for n, _ in got]
    assert names[:4] == ["base.gru." + k for k in gr.GRU_NAMES] and names[4] == "base.main.0.weight"
    assert got[0][1] == (72, 24) and got[1][1] == (72, 24)      # nn.GRU(Hs, Hs): the GRU reads the Hs features
    assert names[12:14] == ["base.critic_linear.weight", "base.critic_linear.bias"] and names[14].startswith("dist.")


# ------------------------------------------------------------------------------------------------- 4 the generator
def test_recurrent_generator_on_an_image_rollout(monkeypatch):
    from simgan_amd.storage import recurrent_batches

    class Ro(object):
        pass
    T, N, C_, H = 3, 4, 2, 5
    rng = np.random.default_rng(0)
    ro = Ro()
    ro.obs = rng.integers(0, 256, (T + 1, N, C_, HW, HW)).astype(np.float32)
    ro.recurrent_hidden_states = rng.standard_normal((T + 1, N, H)).astype(np.float32)
    ro.actions = rng.integers(0, 5, (T, N, 1)).astype(np.int64)
    ro.rewards = np.zeros((T, N, 1), np.float32)
    for name, slots in (("value_preds", T + 1), ("returns", T + 1), ("masks", T + 1), ("action_log_probs", T)):
        setattr(ro, name, rng.standard_normal((slots, N, 1)).astype(np.float32))
    adv = rng.standard_normal((T, N, 1)).astype(np.float32)
    perm = np.array([2, 0, 3, 1])
    batches = list(recurrent_batches(ro, adv, 2, perm))
    assert len(batches) == 2 and all(len(b) == 8 for b in batches)
    for k, b in enumerate(batches):
        envs = perm[2 * k:2 * k + 2]
        obs, hxs, act, vp, ret, mk, olp, a = [x.numpy() if hasattr(x, "numpy") else np.asarray(x) for x in b]
        assert obs.shape == (T * 2, C_, HW, HW)      # 4-D frames, as the reference's _flatten_helper leaves them
        for t in range(T):
            for j, e in enumerate(envs):
                r = t * 2 + j
                assert np.array_equal(obs[r], ro.obs[t, e]) and act[r, 0] == ro.actions[t, e, 0] and mk[r, 0] == ro.masks[t, e, 0]
                assert vp[r, 0] == ro.value_preds[t, e, 0] and ret[r, 0] == ro.returns[t, e, 0] and olp[r, 0] == ro.action_log_probs[t, e, 0]
                assert a[r, 0] == adv[t, e, 0]
        assert np.array_equal(hxs, ro.recurrent_hidden_states[0, envs])


class _FakeLib(object):
    """every entry point succeeds and writes nothing: enough to build a RolloutStorage without a device"""

    def __getattr__(self, name):
        return lambda *a, **k: 0


def test_recurrent_generator_refusal_depends_on_the_hidden_size(monkeypatch):
    import simgan_amd as sg
    from simgan_amd import _lib

    class Ctx(object):
        h, lib, world, rank = None, _FakeLib(), 1, 0
    monkeypatch.setattr(_lib.Context, "default", staticmethod(lambda: Ctx()))
    one = sg.RolloutStorage(2, 2, (1, HW, HW), Discrete(3), 1, 1)
    wide = sg.RolloutStorage(2, 2, (1, HW, HW), Discrete(3), 8, 1)
    with pytest.raises(NotImplementedError, match="recurrent_generator: image observations are read by the feed-forward"):
        next(iter(one.recurrent_generator(None, 1)))
    b = next(iter(wide.recurrent_generator(None, 1, perm=np.array([1, 0]))))
    assert tuple(b[0].shape) == (4, 1, HW, HW) and tuple(b[1].shape) == (2, 8)
    with pytest.raises(NotImplementedError, match="enable_device_hidden: the rollout holds image observations"):
        wide.enable_device_hidden()


# ------------------------------------------------------------------------------------------------- 5 refusals
class _Pol(object):
    """what the refusals read of a recurrent CNN policy"""
    cnn, is_recurrent, dist_kind, recurrent_hidden_state_size = 1, True, 1, 16

    class ctx(object):
        world = 1


def test_python_refusals_name_the_recurrent_cnn_base():
    import simgan_amd as sg
    from simgan_amd.algo import diagnostics
    from simgan_amd.checkpoint import CNN_SAVE_MSG, save_policy
    from simgan_amd.ensemble import PolicyEnsemble
    p = _Pol()
    for kw in (dict(acktr=True), dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5), dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, cnn=True),
               dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, recurrent=True)):
        with pytest.raises(NotImplementedError, match="A2C_ACKTR: not implemented for the recurrent CNN base"):
            sg.algo.A2C_ACKTR(p, 0.5, 0.01, **kw)
    with pytest.raises(NotImplementedError, match="PolicyEnsemble: a member with the recurrent CNN base is not served"):
        PolicyEnsemble([p])
    with pytest.raises(NotImplementedError, match="mirror-symmetry loss: not implemented for the recurrent CNN base"):
        sg.algo.PPO(p, 0.2, 1, 1, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5, symmetry_coef=1.0, mirror_obs=np.eye(2), mirror_act=np.eye(1))

    class Wide(_Pol):
        class ctx(object):
            world = 2
    with pytest.raises(NotImplementedError, match="PPO on the recurrent CNN base runs on one rank"):
        sg.algo.PPO(Wide(), 0.2, 1, 1, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)

    class Agent(object):
        actor_critic = p
    with pytest.raises(NotImplementedError, match="diagnostics: not built for the recurrent CNN base"):
        diagnostics.run(Agent(), None, 0.2)
    with pytest.raises(NotImplementedError) as exc:
        save_policy("/nonexistent/never-written.pt", p)
    assert str(exc.value) == CNN_SAVE_MSG


# ------------------------------------------------------------------------------------------------- 6 the reference's fixtures
@pytest.mark.parametrize("name", ["policy_cnn_gru_cat", "policy_cnn_gru_box"])
def test_the_arbiter_matches_the_references_forward_fixture(name):
    """tests/golden/policy_cnn_gru_*.npz (tools/gen_golden_cnn_gru.py: the reference's own float32 results) against the arbiter"""
    import torch
    g = load(name)
    m = g["meta"]
    shapes = gr.param_shapes(m["C"], m["Hs"], m["dist"], m["P"])
    assert [str(k) for k in g["keys"]] == [n for n, _ in shapes]      # the reference's state_dict order
    T, n = m["T"], m["n"]
    obs, masks = g["obs"].astype(np.float32), g["masks"].reshape(-1)
    with torch.no_grad():
        v, lp, ent, h = gr.evaluate(cr.leaves(g["params"], shapes), ar.t64(obs), g["hxs"], masks, T, g["eval_action"], m["dist"])
    assert_close(g["eval_value"], v.numpy(), what="value")
    assert_close(g["eval_logp"], lp.numpy(), what="logp")
    assert_close(g["eval_entropy"], ent.numpy(), what="entropy")
    assert_close(g["eval_hxs"], h.numpy(), what="final hidden state")
    det = gr.act64(shapes, g["params"], obs[:n], g["hxs"], masks[:n], 1, m["dist"])
    assert_close(g["get_value"], det["value"], what="get_value")
    assert_close(g["det_logp"], det["logp"], what="logp of the mode")
    assert_close(g["det_hxs"], det["hxs"], what="hidden state after one step")
    assert masks[0] == 0 and (masks == 0).sum() >= 2 and np.abs(g["hxs"]).min() > 0


@pytest.mark.parametrize("dist,P,name", [("categorical", 5, "policy_cnn_gru_cat"), ("gaussian", 3, "policy_cnn_gru_box")])
def test_param_shapes_against_the_fixtures_state_dict_keys(monkeypatch, dist, P, name):
    g = load(name)
    m = g["meta"]
    sg, _ = _spy_create(monkeypatch)
    p = sg.Policy((m["C"], HW, HW), Discrete(P) if dist == "categorical" else Box((P,)), base_kwargs={"recurrent": True, "hidden_size": m["Hs"]},
                  recurrent_cnn=True)
    assert [n for n, _ in p.param_shapes()] == [str(k) for k in g["keys"]]
    assert sum(int(np.prod(s)) for _, s in p.param_shapes()) == g["params"].size


def test_the_checkpoint_fixture_reads_as_a_recurrent_cnn_policy():
    """checkpoint.read_reference_checkpoint on the reference's own torch.save of such a policy (no device: the dims and the weights)"""
    from simgan_amd.checkpoint import read_reference_checkpoint
    g = load("ckpt_policy_cnn_gru")
    m = g["meta"]
    ck = read_reference_checkpoint(os.path.join(GOLDEN, "ckpt_policy_cnn_gru.pt"))
    assert ck["kind"] == "cnn_categorical" and ck["recurrent"] is True and ck["cnn"] == m["C"] and ck["hidden"] == m["Hs"] and ck["n_out"] == m["P"]
    assert list(ck["state_dict"]) == m["names"] == [n for n, _ in gr.param_shapes(m["C"], m["Hs"], "categorical", m["P"])]
    flat = np.concatenate([np.asarray(v, np.float32).reshape(-1) for v in ck["state_dict"].values()])
    assert np.array_equal(flat, g["params"])
    for needle in (b"class CNNBase", b"class NNBase", b"def forward", b"import torch"):
        assert needle not in open(os.path.join(GOLDEN, "ckpt_policy_cnn_gru.pt"), "rb").read()
