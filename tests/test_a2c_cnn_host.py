"""CPU: A2C on the CNN base (A2C_ACKTR(..., cnn=True) / sg_a2c_create_cnn) -- the interface that needs no device, the cases the GPU
file may use (clear of the ReLU kinks on the references alone), the defects the per-block comparison must be able to see, and the
reference-written fixtures (tools/gen_golden_a2c_cnn.py) against the float64 restatement of tests/a2c_cnn_ref.py."""
import ctypes
import os
import types

import numpy as np
import pytest

import a2c_cnn_ref as ref
import cnn_ref as cr
from helpers import GOLDEN, RTOL, assert_close, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)


def test_the_library_exports_the_entry_point():
    from simgan_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "sg_a2c_create_cnn")
    assert _lib.PROTOTYPES["sg_a2c_create_cnn"] == _lib.PROTOTYPES["sg_a2c_create_rnn"]
    header = open(os.path.join(ROOT, "include", "simgan_hip.h")).read()
    assert "SG_API int sg_a2c_create_cnn(sg_ctx *ctx, sg_policy *p, const sg_a2c_config *cfg, sg_ppo **out);" in header
    assert "a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:204-230" in header


def test_python_refusals_that_need_no_device():
    import simgan_amd as sg
    cnn = types.SimpleNamespace(is_recurrent=False, KIND=0, dist_kind=1, cnn=4, ctx=types.SimpleNamespace(world=1))
    # without the keyword the refusal is the old one, in either mode
    for acktr in (False, True):
        with pytest.raises(NotImplementedError, match="A2C_ACKTR: not implemented for the CNN base \\(image observations\\), in either mode; PPO is"):
            sg.algo.A2C_ACKTR(cnn, 0.5, 0.01, acktr=acktr, **({} if acktr else KW))
    with pytest.raises(NotImplementedError, match="opt-in: A2C_ACKTR\\(..., acktr=False, cnn=True\\)"):
        sg.algo.A2C_ACKTR(cnn, 0.5, 0.01, **KW)
    with pytest.raises(NotImplementedError, match="K-FAC has no convolution statistics here"):
        sg.algo.A2C_ACKTR(cnn, 0.5, 0.01, acktr=True, cnn=True)
    mlp = types.SimpleNamespace(is_recurrent=False, KIND=0, dist_kind=0, cnn=0, ctx=types.SimpleNamespace(world=1))
    with pytest.raises(ValueError, match="A2C_ACKTR\\(cnn=True\\) takes a Policy with the CNN base"):
        sg.algo.A2C_ACKTR(mlp, 0.5, 0.01, cnn=True, **KW)
    cnn.ctx.world = 2
    with pytest.raises(NotImplementedError, match="A2C on the CNN base \\(image observations\\) runs on one rank \\(this context's world is 2\\)"):
        sg.algo.A2C_ACKTR(cnn, 0.5, 0.01, cnn=True, **KW)
    cnn.ctx.world = 1
    with pytest.raises(ValueError, match="needs lr, eps, alpha, max_grad_norm"):
        sg.algo.A2C_ACKTR(cnn, 0.5, 0.01, cnn=True)
    agent = sg.algo.A2C_ACKTR.__new__(sg.algo.A2C_ACKTR)
    agent.cnn = True
    with pytest.raises(NotImplementedError, match="A2C_ACKTR.diagnostics: the diagnostics kernels do not cover the CNN base"):
        agent.diagnostics(None)


def test_the_alias_package_hands_the_keyword_through():
    """third_party.a2c_ppo_acktr re-exports the class itself, so cnn=True needs no passing on (read as text: this process must not
    import the alias package, tests/test_interop.py)"""
    import inspect
    import simgan_amd as sg
    for rel in ("algo/__init__.py", "algo/a2c_acktr.py"):
        text = open(os.path.join(ROOT, "third_party", "a2c_ppo_acktr", rel)).read()
        assert "from simgan_amd.algo.a2c_acktr import A2C_ACKTR" in text and "def " not in text
    assert "cnn" in inspect.signature(sg.algo.A2C_ACKTR.__init__).parameters


@pytest.mark.parametrize("key", ref.CASES, ids=ref.tag)
def test_every_gpu_case_keeps_clear_of_the_relu_kinks(key):
    assert key + ("off_policy",) in cr.SEEDS       # a committed seed, not a search
    c = ref.case(key)
    obs, actions, returns = ref.rows_of(c)
    assert obs.shape[0] == c.T * c.N <= 17
    assert cr.kink_margin(c.shapes, c.params, obs) >= cr.KINK_FACTOR
    g, losses = ref.case_grad(c)
    assert np.isfinite(g).all() and np.isfinite(losses).all()      # one row too: A2C has no advantage std
    assert all(np.abs(b).max() > 0 for _, b in cr.blocks(c.shapes, g))
    assert set(k for k, _ in ref.CHUNKED) <= set(ref.CASES)


@pytest.mark.parametrize("key,chunk", ref.CHUNKED, ids=lambda v: ref.tag(v) if isinstance(v, tuple) else str(v))
def test_chunked_sums_are_the_unchunked_gradient(key, chunk):
    """what the library's accumulate path computes, restated: sum over chunks of (rows / (T N)) x the chunk's own mean-loss gradient"""
    c = ref.case(key)
    obs, actions, returns = ref.rows_of(c)
    n = obs.shape[0]
    assert n > chunk
    whole, _ = ref.case_grad(c)
    acc = np.zeros_like(whole)
    for b in range(0, n, chunk):
        e = min(b + chunk, n)
        acc += ref.a2c_grad(c.shapes, c.params, obs[b:e], actions[b:e], returns[b:e], c.dist)[0] * ((e - b) / n)
    assert max(cr.block_distances(acc, whole, c.shapes).values()) <= 1e-9


@pytest.mark.parametrize("fault", ["inv_chunk", "drop_last_chunk", "value_no_2", "adv_attached"])
@pytest.mark.parametrize("key,chunk", ref.CHUNKED, ids=lambda v: ref.tag(v) if isinstance(v, tuple) else str(v))
def test_the_per_block_comparison_sees_each_defect(key, chunk, fault):
    c = ref.case(key)
    whole, _ = ref.case_grad(c)
    wrong, _ = ref.case_grad(c, fault=fault, chunk=chunk)
    worst = max(cr.block_distances(wrong, whole, c.shapes).values())
    assert worst > 10 * RTOL, (fault, worst)


def test_the_recovered_gradient_is_the_gradient():
    """the GPU file's read-back restated in float64 / float32: a first step from square_avg = 0 at eps = 1e-12"""
    c = ref.case(ref.GAUSSIAN_CASE)
    g, _ = ref.case_grad(c)
    p1, sq, f = ref.rmsprop64(c.params, g, np.zeros_like(g), eps=ref.EPS_RECOVER, max_grad_norm=ref.NO_CLIP)
    assert f == 1.0
    p1_32 = p1.astype(np.float32)
    assert (np.abs(c.params.astype(np.float64) - p1_32)[g != 0] > 5 * ref.LR).all()      # ~10 lr: no sign is lost in float32
    back = ref.recovered_gradient(c.params, p1_32, sq.astype(np.float32))
    assert max(cr.block_distances(back, g, c.shapes).values()) <= 1e-6


@pytest.mark.parametrize("name", ref.FIXTURES)
def test_fixture_is_what_the_issue_describes_and_consistent_with_float64(name):
    g = load(name)
    m = g["meta"]
    assert (m["C"], m["Hs"], m["T"], m["N"], m["iters"]) == (1, 16, 3, 4, 2)
    assert (m["dist"], m["P"]) == (("categorical", 5) if name.endswith("cat") else ("gaussian", 3))
    assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) <= 716 * 1024
    shapes = cr.param_shapes(m["C"], m["Hs"], m["dist"], m["P"])
    assert [(k, tuple(s)) for k, s in zip(m["names"], m["shapes"])] == shapes
    n = cr.num_params(shapes)
    assert g["params0"].size == n and g["params0"].dtype == np.float32
    # update_linear_schedule (a2c/utils.py:68-72)
    assert_close(g["lrs"], [m["lr"] * (1 - j / m["num_updates"]) for j in range(m["iters"])], rtol=1e-12, atol=0, what="lrs")
    p, sq = g["params0"].astype(np.float64), None
    for j, (pre, obs, actions, returns, lr) in enumerate(ref.fixture_updates(g)):
        assert g[pre + "obs"].dtype == np.uint8 and g[pre + "obs"].shape == (m["T"] + 1, m["N"], m["C"], 84, 84)
        assert cr.kink_margin(shapes, p, obs) >= cr.KINK_FACTOR, (name, j)
        r = ref.update64(shapes, m["dist"], p, sq, obs, actions, returns, vcoef=m["value_loss_coef"], ecoef=m["entropy_coef"], lr=lr,
                         eps=m["eps"], alpha=m["alpha"], max_grad_norm=m["max_grad_norm"])
        idx = ref.sample_index(n, j)
        assert idx.size >= n // m["sample_stride"] and g[pre + "params1"].size == idx.size == g[pre + "square_avg"].size
        assert_close(g[pre + "losses"], r["losses"], what=f"{name} losses {j}")
        assert_close(g[pre + "params1"], r["params"][idx], what=f"{name} params {j}")
        assert_close(g[pre + "square_avg"], r["square_avg"][idx], rtol=1e-3, atol=1e-12, what=f"{name} square_avg {j}")
        assert r["factor"] == pytest.approx(float(g[pre + "factor"]), rel=1e-9)
        p, sq = r["params"], r["square_avg"]
