"""CPU: A2C through time (A2C_ACKTR(..., recurrent=True)) -- the float64 restatement of one update (tests/a2c_gru_ref.py) against
the reference-written fixtures (tools/gen_golden_a2c_recurrent.py) and against autograd through torch.nn.GRU, the faults the
references must be able to see, the cases the GPU file may use, and the interface that needs no device."""
import ctypes
import os
import types

import numpy as np
import pytest

import a2c_gru_ref as ref
from helpers import assert_close, load

FIXTURES = ["a2c_gru_onestep", "a2c_gru_tiny", "a2c_gru_ragged"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture_updates(g):
    """-> [(prefix, rollout dict, hxs0, lr)] of the fixture's updates in order"""
    m = g["meta"]
    out = []
    for j in range(m["iters"]):
        pre = "" if m["iters"] == 1 else f"it{j}_"
        out.append((pre, {k: g[pre + k] for k in ("obs", "actions", "returns", "masks")}, g[pre + "hxs0"], float(g["lrs"][j])))
    return out


def test_fixtures_are_what_the_issue_describes():
    shapes = {"a2c_gru_onestep": (11, 3, 16, 5, 4, 1), "a2c_gru_tiny": (11, 3, 32, 5, 16, 3), "a2c_gru_ragged": (13, 5, 20, 9, 33, 1)}
    for name in FIXTURES:
        g = load(name)
        m = g["meta"]
        assert (m["O"], m["A"], m["H"], m["T"], m["N"], m["iters"]) == shapes[name]
        for pre, ro, hxs0, _ in fixture_updates(g):
            assert (ro["masks"][0] == 0).any() and (ro["masks"][1:-1] == 0).any() or m["T"] <= 2, name
            assert np.abs(hxs0).max() > 0
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 300 * 1024
    assert max(load("a2c_gru_onestep")["meta"]["grad_norms"]) < load("a2c_gru_onestep")["meta"]["max_grad_norm"]   # clip inactive
    assert min(load("a2c_gru_tiny")["meta"]["grad_norms"]) > 0.5 == load("a2c_gru_tiny")["meta"]["max_grad_norm"]   # clip active


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(name):
    g = load(name)
    m = g["meta"]
    p, sq = g["params0"], None
    for j, (pre, ro, hxs0, lr) in enumerate(fixture_updates(g)):
        r = ref.update(p, m["O"], m["A"], m["H"], ro, hxs0, m["value_loss_coef"], m["entropy_coef"], lr, m["eps"], m["alpha"],
                       m["max_grad_norm"], square_avg=sq)
        assert_close(r["losses"], g[pre + "losses"], what=f"{name} losses {j}")
        assert_close(r["params"], g[pre + "params1"], what=f"{name} params {j}")
        assert_close(r["square_avg"], g[pre + "square_avg"], rtol=1e-4, atol=1e-12, what=f"{name} square_avg {j}")
        assert r["norm"] == pytest.approx(m["grad_norms"][j], rel=1e-4)
        p, sq = r["params"], r["square_avg"]


def _fixture_case(name):
    g = load(name)
    m = g["meta"]
    pre, ro, hxs0, _ = fixture_updates(g)[0]
    return g, m, ro, hxs0


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_matches_autograd_per_block(name):
    g, m, ro, hxs0 = _fixture_case(name)
    args = (g["params0"], m["O"], m["A"], m["H"], ro, hxs0, m["value_loss_coef"], m["entropy_coef"])
    g_r, l_r = ref.grad(*args)
    g_a, l_a = ref.autograd_grad(*args)
    errs = ref.block_errors(g_r, g_a, m["O"], m["A"], m["H"])
    assert len(errs) == 4 * 3 + 13
    assert max(errs.values()) <= 1e-9, errs
    assert np.max(np.abs(l_r - l_a) / np.abs(l_a)) <= 1e-12
    # in groups of 16 environments the sum is the same number (the library's accumulate paths restated)
    g_g, l_g = ref.grad(*args, group_envs=16)
    assert max(ref.block_errors(g_g, g_a, m["O"], m["A"], m["H"]).values()) <= 1e-9
    assert np.max(np.abs(l_g - l_a) / np.abs(l_a)) <= 1e-12


@pytest.mark.parametrize("wrong", ["no_mask", "group_mean", "half_value"])
def test_wrong_restatements_fail_against_autograd(wrong):
    g, m, ro, hxs0 = _fixture_case("a2c_gru_ragged")
    args = (g["params0"], m["O"], m["A"], m["H"], ro, hxs0, m["value_loss_coef"], m["entropy_coef"])
    g_a, l_a = ref.autograd_grad(*args)
    g_w, l_w = ref.grad(*args, group_envs=16 if wrong == "group_mean" else None, wrong=wrong)
    errs = ref.block_errors(g_w, g_a, m["O"], m["A"], m["H"])
    assert max(errs.values()) > 1e-3, (wrong, errs)
    # ... and against the fixture, within the contract's 1e-4
    r = ref.update(*args, float(g["lrs"][0]), m["eps"], m["alpha"], m["max_grad_norm"], group_envs=16 if wrong == "group_mean" else None,
                   wrong=wrong)
    with pytest.raises(AssertionError):
        assert_close(r["params"], g["params1"], what=wrong)
        assert_close(r["losses"], g["losses"], what=wrong)


def test_clip_norm_without_the_gru_block_fails_against_the_fixture():
    """a2c_gru_tiny clips at 0.5: a norm over the heads' gradient alone scales the step differently."""
    g = load("a2c_gru_tiny")
    m = g["meta"]
    pre, ro, hxs0, lr = fixture_updates(g)[0]
    args = (g["params0"], m["O"], m["A"], m["H"], ro, hxs0, m["value_loss_coef"], m["entropy_coef"], lr, m["eps"], m["alpha"], m["max_grad_norm"])
    good, bad = ref.update(*args), ref.update(*args, wrong="clip_without_gru")
    assert bad["norm"] < good["norm"] * (1 - 1e-3) and good["norm"] == pytest.approx(m["grad_norms"][0], rel=1e-4)
    assert_close(good["square_avg"], g[pre + "square_avg"], rtol=1e-4, atol=1e-12, what="square_avg")
    with pytest.raises(AssertionError):
        assert_close(bad["square_avg"], g[pre + "square_avg"], rtol=1e-4, atol=1e-12, what="square_avg without the GRU block in the norm")


def _gpu_cases():
    return [ref.random_case(*s) for s in ref.GPU_SHAPES + [ref.ANCHOR_SHAPE]] + [ref.random_case(*ref.DEAD_ENV_CASE[0], dead_env=ref.DEAD_ENV_CASE[1])]


def test_gpu_cases_are_admitted():
    """Every shape the GPU file holds to float64: the float32 mode of the restatement stays within half the bound in every block,
    and the restatement agrees with autograd there too (T = 1, T*N past one heads' chunk and a padded hidden width included)."""
    for c in _gpu_cases():
        g64, l64, worst = ref.admitted(c)
        assert worst <= 0.5 * ref.RTOL_BLOCK, (c["O"], c["A"], c["H"], c["T"], c["N"], worst)
        assert (c["masks"][0] == 0).any() and np.abs(c["hxs0"]).max() > 0
        if c["T"] * c["N"] <= 1500:
            g_a, _ = ref.autograd_grad(c["params"], c["O"], c["A"], c["H"], c, c["hxs0"], 0.5, 0.01)
            assert max(ref.block_errors(g64, g_a, c["O"], c["A"], c["H"]).values()) <= 1e-9
    dead = _gpu_cases()[-1]
    assert (dead["masks"][:, ref.DEAD_ENV_CASE[1]] == 0).all()


# ------------------------------------------------------------------------------------------- interface
def test_default_refusal_is_intact_and_the_keyword_is_checked():
    import simgan_amd as sg
    rec = types.SimpleNamespace(is_recurrent=True, KIND=0)
    kw = dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    with pytest.raises(NotImplementedError, match="not for a recurrent Policy"):
        sg.algo.A2C_ACKTR(rec, 0.5, 0.01, **kw)
    with pytest.raises(NotImplementedError, match="recurrent=True"):   # the refusal points at the keyword
        sg.algo.A2C_ACKTR(rec, 0.5, 0.01, **kw)
    with pytest.raises(NotImplementedError, match="refuses it with acktr"):
        sg.algo.A2C_ACKTR(rec, 0.5, 0.01, acktr=True, recurrent=True)
    ff = types.SimpleNamespace(is_recurrent=False, KIND=0)
    with pytest.raises(ValueError, match="takes a recurrent Policy"):
        sg.algo.A2C_ACKTR(ff, 0.5, 0.01, recurrent=True, **kw)


def test_the_library_exports_the_entry_point():
    from simgan_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "sg_a2c_create_rnn")
    header = open(os.path.join(ROOT, "include", "simgan_hip.h")).read()
    assert "SG_API int sg_a2c_create_rnn(sg_ctx *ctx, sg_policy *p, const sg_a2c_config *cfg, sg_ppo **out);" in header
