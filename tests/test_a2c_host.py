"""CPU: A2C_ACKTR's host side (the alias package, the constructor's refusals) and a float64 numpy restatement of the reference's
update (a2c/algo/a2c_acktr.py:52-102, acktr=False) that reproduces every a2c_* fixture (tools/gen_golden_a2c.py).  The GPU
tests (tests/test_gpu_a2c.py) measure the kernels against this restatement at shapes too big for a fixture."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from helpers import ATOL, RTOL, assert_close, load  # noqa: E402

A2C_CASES = ["a2c_tiny", "a2c_default", "a2c_critic64"]
HALF_LOG_2PI = float(np.float32(0.5 * np.log(2.0 * np.pi)))   # the float32 value, as in every float64 arbiter (tests/autograd_ref.py)


# ------------------------------------------------------------------ restatement
def policy_slices(O, A, H, Hc):
    """Flat state_dict order of Policy (a2c/model.py:233-264, simgan_amd/model.py param_shapes)."""
    out, off = {}, 0
    for key, shape in (("aw1", (H, O)), ("ab1", (H,)), ("aw2", (H, H)), ("ab2", (H,)),
                       ("cw1", (Hc, O)), ("cb1", (Hc,)), ("cw2", (Hc, Hc)), ("cb2", (Hc,)),
                       ("vw", (1, Hc)), ("vb", (1,)), ("mw", (A, H)), ("mb", (A,)), ("ls", (A,))):
        n = int(np.prod(shape))
        out[key] = (slice(off, off + n), shape)
        off += n
    return out, off


def _trunk_bwd(g, sl, p, x, h1, h2, dout, wkey, w1, b1, w2, b2, bh):
    """Back-propagate d loss / d head (dout [B, P]) through head `wkey` and the tanh trunk (w1, b1, w2, b2) into g."""
    W = p[wkey]
    g[sl[wkey][0]] += (dout.T @ h2).reshape(-1)
    g[sl[bh][0]] += dout.sum(0)
    one = h2.dtype.type(1.0)
    dz2 = (dout @ W) * (one - h2 * h2)
    g[sl[w2][0]] += (dz2.T @ h1).reshape(-1)
    g[sl[b2][0]] += dz2.sum(0)
    dz1 = (dz2 @ p[w2]) * (one - h1 * h1)
    g[sl[w1][0]] += (dz1.T @ x).reshape(-1)
    g[sl[b1][0]] += dz1.sum(0)


def a2c_loss_grad(params, obs_rows, act_rows, ret_rows, dims, vcoef, ecoef, dtype=np.float64, half_log_2pi=HALF_LOG_2PI):
    """(value_loss, action_loss, dist_entropy), d loss / d params -- all rows of the rollout at once, evaluated in `dtype`
    (float64: the restatement; float32: the same arithmetic at the kernels' precision, for the conditioning of a case).
    half_log_2pi: log(sqrt(2 pi)) as the run compared with had it (the reference after .double(): the exact double)."""
    O, A, H, Hc = dims
    sl, n = policy_slices(O, A, H, Hc)
    f = np.dtype(dtype).type
    flat = np.asarray(params, dtype)
    p = {k: flat[s].reshape(shape) for k, (s, shape) in sl.items()}
    x = np.asarray(obs_rows, dtype)
    act = np.asarray(act_rows, dtype)
    R = np.asarray(ret_rows, dtype).reshape(-1)
    B = x.shape[0]
    a1 = np.tanh(x @ p["aw1"].T + p["ab1"])
    a2 = np.tanh(a1 @ p["aw2"].T + p["ab2"])
    mu = a2 @ p["mw"].T + p["mb"]
    c1 = np.tanh(x @ p["cw1"].T + p["cb1"])
    c2 = np.tanh(c1 @ p["cw2"].T + p["cb2"])
    v = (c2 @ p["vw"].T + p["vb"]).reshape(-1)
    ls = p["ls"]
    var = np.exp(f(2.0) * ls)
    diff = act - mu
    logp = (-(diff * diff) / (f(2.0) * var) - ls - f(half_log_2pi)).sum(1)
    ent = float(np.sum(f(0.5) + f(half_log_2pi) + ls))
    adv = R - v
    value_loss = float(np.mean(adv * adv))
    action_loss = float(-np.mean(adv * logp))
    g = np.zeros(n, dtype)
    dv = f(vcoef) * f(2.0) * (v - R) / f(B)             # d(vcoef mean(adv^2)) / dv
    dlogp = -adv / f(B)                                 # adv detached
    dmu = dlogp[:, None] * diff / var
    g[sl["ls"][0]] = (dlogp[:, None] * (diff * diff / var - f(1.0))).sum(0) - f(ecoef)
    _trunk_bwd(g, sl, p, x, a1, a2, dmu, "mw", "aw1", "ab1", "aw2", "ab2", "mb")
    _trunk_bwd(g, sl, p, x, c1, c2, dv[:, None], "vw", "cw1", "cb1", "cw2", "cb2", "vb")
    return (value_loss, action_loss, ent), g


def a2c_update_restated(params, square_avg, obs, actions, returns, dims, vcoef, ecoef, lr, eps, alpha, max_grad_norm):
    """One A2C_ACKTR.update (acktr=False) on rollout arrays obs [T+1, N, O], actions [T, N, A], returns [T+1, N, 1]:
    -> (params1 float32, square_avg float32, losses[3]).  clip_grad_norm_ then torch's RMSprop step, float64."""
    O, A = dims[0], dims[1]
    obs = np.asarray(obs)
    T, N = obs.shape[0] - 1, obs.shape[1]
    losses, g = a2c_loss_grad(params, obs[:T].reshape(-1, O), np.asarray(actions).reshape(-1, A),
                              np.asarray(returns)[:T].reshape(-1), dims, vcoef, ecoef)
    norm = np.sqrt(np.sum(g * g))
    g = g * min(1.0, max_grad_norm / (norm + 1e-6))
    sq = alpha * np.asarray(square_avg, np.float64) + (1.0 - alpha) * g * g
    p1 = np.asarray(params, np.float64) - lr * g / (np.sqrt(sq) + eps)
    return p1.astype(np.float32), sq.astype(np.float32), np.array(losses)


def fixture_dims(m):
    return (m["O"], m["A"], m["H"], m["Hc"])


def restate_fixture(g, pre="", square_avg=None, lr=None):
    m = g["meta"]
    sq0 = np.zeros_like(g[pre + "params0"]) if square_avg is None else square_avg
    return a2c_update_restated(g[pre + "params0"], sq0, g[pre + "obs"], g[pre + "actions"], g[pre + "returns"], fixture_dims(m),
                               m["value_loss_coef"], m["entropy_coef"], m["lr"] if lr is None else lr, m["eps"], m["alpha"],
                               m["max_grad_norm"])


# ------------------------------------------------------------------ tests
def test_alias_package_binds_both_import_forms():
    """a2c/main.py's `from a2c_ppo_acktr import algo; algo.A2C_ACKTR` and the module form both bind to the library's class.
    (In a child process: other tests require that no `third_party` module is loaded in theirs.)"""
    import subprocess
    code = ("from third_party.a2c_ppo_acktr import algo\n"
            "from third_party.a2c_ppo_acktr.algo.a2c_acktr import A2C_ACKTR\n"
            "from simgan_amd.algo import A2C_ACKTR as ours\n"
            "assert algo.A2C_ACKTR is ours and A2C_ACKTR is ours\n")
    subprocess.run([sys.executable, "-s", "-c", code], cwd=ROOT, check=True, timeout=300)


@pytest.mark.parametrize("name", A2C_CASES)
def test_restatement_reproduces_the_reference_fixture(name):
    g = load(name)
    par, sq, losses = restate_fixture(g)
    assert not np.allclose(g["value_preds"], 0.0)
    assert_close(losses, g["losses"], rtol=RTOL, atol=ATOL, what="losses")
    assert_close(sq, g["square_avg"], rtol=RTOL, atol=1e-12, what="square_avg")
    assert_close(par, g["params1"], rtol=RTOL, atol=ATOL, what="params after update")


def test_restatement_reproduces_the_multi_update_fixture():
    """Three updates on fresh rollouts with update_linear_schedule between them: square_avg carried, lr decayed."""
    g = load("a2c_multi")
    m = g["meta"]
    assert m["iters"] == 3
    lrs = [m["lr"] - m["lr"] * j / m["num_updates"] for j in range(3)]
    assert np.allclose(g["lrs"], lrs)
    sq = None
    for j in range(3):
        par, sq, losses = restate_fixture(g, f"it{j}_", square_avg=sq, lr=lrs[j])
        assert_close(losses, g[f"it{j}_losses"], what=f"losses {j}")
        assert_close(sq, g[f"it{j}_square_avg"], rtol=RTOL, atol=1e-12, what=f"square_avg {j}")
        assert_close(par, g[f"it{j}_params1"], what=f"params after update {j}")


def test_stored_value_preds_are_not_the_values_the_update_uses():
    """The fixtures perturb the policy after collecting the rollout: a value loss built on value_preds is outside the
    tolerance the fixture tests apply."""
    g = load("a2c_default")
    T = g["meta"]["T"]
    _, _, losses = restate_fixture(g)
    vp_loss = float(np.mean((g["returns"][:T].astype(np.float64) - g["value_preds"][:T]) ** 2))
    assert abs(vp_loss - losses[0]) > ATOL + RTOL * abs(losses[0])


def test_constructor_refusals_before_any_device_work():
    """acktr=True, SplitPolicy and missing optimizer arguments are refused in Python, before the library is touched."""
    from simgan_amd.algo.a2c_acktr import A2C_ACKTR

    class Policy:   # a stand-in: the checks run before the policy's device handle is read
        pass

    class SplitPolicy:
        pass

    with pytest.raises(NotImplementedError, match="K-FAC"):
        A2C_ACKTR(Policy(), 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, acktr=True)
    with pytest.raises(NotImplementedError, match="SplitPolicy"):
        A2C_ACKTR(SplitPolicy(), 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    for missing in ("lr", "eps", "alpha", "max_grad_norm"):
        kw = dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
        kw[missing] = None
        with pytest.raises(ValueError, match=missing):
            A2C_ACKTR(Policy(), 0.5, 0.01, **kw)


def test_fixtures_stay_small():
    for name in A2C_CASES + ["a2c_multi"]:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < (1 << 20)
