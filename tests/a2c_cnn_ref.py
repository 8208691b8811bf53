"""The arbiter of A2C on the CNN base (a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:204-230): the loss written forward-only in
torch.float64 on tests/cnn_ref.py's evaluate / leaves, torch.autograd for the gradient, torch.optim.RMSprop's recurrence in numpy
float64.  Nothing is derived by hand and nothing touches the library.

Cases are tests/cnn_ref.py's at its committed seeds.  The A2C gradient reads only params, obs, actions and returns of a case, and
the kink condition (every ReLU pre-activation of the float64 forward at least KINK_FACTOR times the float32 forward's error away
from zero) is a property of params and obs alone, so the proof tests/test_cnn_host.py gives for those seeds holds here;
tests/test_a2c_cnn_host.py checks it again for every case the GPU file uses.

`fault` injects one defect into the gradient, for the test of the test: "inv_chunk" (every chunk's rows weighted 1 / chunk
instead of 1 / (T N)), "drop_last_chunk", "value_no_2" (the value loss's gradient without its factor 2) and "adv_attached" (the
advantage of the action loss not detached)."""
import warnings

import numpy as np

import cnn_ref as cr
from cnn_ref import ar

HW = cr.HW
VCOEF, ECOEF, LR, EPS, ALPHA, MAX_GRAD_NORM = 0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5   # a2c/arguments.py defaults
NO_CLIP = 1e9
EPS_RECOVER = 1e-12     # the gradient-recovery runs: every non-zero g then moves its parameter by about 10 lr

# (C, Hs, dist, P, T, N): tests/cnn_ref.py's "off_policy" cases, one row up to 17
CASES = [(1, 16, "categorical", 5, 1, 1), (1, 16, "categorical", 5, 1, 3), (1, 16, "categorical", 5, 17, 1),
         (3, 20, "gaussian", 3, 3, 5), (1, 16, "categorical", 5, 4, 4)]
GAUSSIAN_CASE = CASES[3]
# (case, SG_A2C_CNN_CHUNK_ROWS): a ragged last chunk of one row; 4 + 4 + 4 + 3 rows, three accumulating passes; two full chunks;
# one row per chunk
CHUNKED = [((1, 16, "categorical", 5, 17, 1), 16), ((3, 20, "gaussian", 3, 3, 5), 4), ((1, 16, "categorical", 5, 4, 4), 8),
           ((1, 16, "categorical", 5, 1, 3), 1)]
FIXTURES = ["a2c_cnn_cat", "a2c_cnn_box"]
SAMPLE_STRIDE = 5       # the fixtures keep every SAMPLE_STRIDE-th element of a result vector (sample_index)


def case(key):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")    # (1 x 1: the unbiased std of one advantage, which PPO's case carries and A2C never reads)
        return cr.case(*key)


def tag(key, chunk=None):
    C, Hs, dist, P, T, N = key
    return f"C={C} Hs={Hs} {dist}({P}) {T}x{N}" + (f" chunk {chunk}" if chunk else "")


def rows_of(c):
    B = c.T * c.N
    return (c.obs[:-1].reshape(B, c.C, HW, HW), np.asarray(c.actions).reshape(B, -1), np.asarray(c.returns)[:-1].reshape(B))


def a2c_loss(p, obs, actions, returns, dist, vcoef=VCOEF, ecoef=ECOEF, fault=None, dtype=cr.F64):
    """a2c/algo/a2c_acktr.py:55-72 on the given rows -> (total, (value_loss, action_loss, dist_entropy))"""
    values, logp, entropy = cr.evaluate(p, ar.t64(obs).to(dtype), actions, dist)
    adv = ar.t64(returns).to(dtype).reshape(-1) - values
    value_loss = adv.pow(2).mean()
    action_loss = -((adv if fault == "adv_attached" else adv.detach()) * logp).mean()
    v_term = 0.5 * value_loss + 0.5 * value_loss.detach() if fault == "value_no_2" else value_loss
    return v_term * vcoef + action_loss - entropy * ecoef, (value_loss, action_loss, entropy)


def a2c_grad(shapes, params, obs, actions, returns, dist, vcoef=VCOEF, ecoef=ECOEF, fault=None, chunk=None, dtype=cr.F64):
    """-> (flat gradient of the loss over ALL the given rows, losses[3]).  The chunked faults take `chunk` rows at a time.  dtype
    torch.float32: the same expressions in torch's float32 CPU arithmetic (the admission rule of tests/cnn_regimes.py)."""
    if fault in ("inv_chunk", "drop_last_chunk"):
        n = obs.shape[0]
        g = np.zeros(cr.num_params(shapes))
        bounds = [(b, min(b + chunk, n)) for b in range(0, n, chunk)]
        for b, e in bounds[:-1] if fault == "drop_last_chunk" else bounds:
            gk, _ = a2c_grad(shapes, params, obs[b:e], actions[b:e], returns[b:e], dist, vcoef, ecoef)
            g += gk * ((e - b) / n if fault == "drop_last_chunk" else (e - b) / chunk)
        return g, a2c_grad(shapes, params, obs, actions, returns, dist, vcoef, ecoef)[1]
    p = cr.leaves(params, shapes, dtype, grad=True)
    total, parts = a2c_loss(p, obs, actions, returns, dist, vcoef, ecoef, fault, dtype)
    return ar.flat_grad(total, p), np.array([float(t.detach()) for t in parts])


def case_grad(c, **kw):
    obs, actions, returns = rows_of(c)
    return a2c_grad(c.shapes, c.params, obs, actions, returns, c.dist, **kw)


def rmsprop64(params, g, sq, lr=LR, eps=EPS, alpha=ALPHA, max_grad_norm=MAX_GRAD_NORM):
    """clip_grad_norm_ + torch.optim.RMSprop (centered False, momentum 0) in float64 -> (params, square_avg, clip factor)"""
    f = cr.clip_factor(g, max_grad_norm)
    g = np.asarray(g, np.float64) * f
    sq = alpha * np.asarray(sq, np.float64) + (1.0 - alpha) * g * g
    return np.asarray(params, np.float64) - lr * g / (np.sqrt(sq) + eps), sq, f


def update64(shapes, dist, params, sq, obs, actions, returns, **hp):
    """one A2C update in float64 -> dict(params, square_avg, losses, grad, factor)"""
    g, losses = a2c_grad(shapes, params, obs, actions, returns, dist, hp.pop("vcoef", VCOEF), hp.pop("ecoef", ECOEF))
    p1, sq1, f = rmsprop64(params, g, np.zeros_like(g) if sq is None else sq, **hp)
    return dict(params=p1, square_avg=sq1, losses=losses, grad=g, factor=f)


def recovered_gradient(p0, p1, sq, alpha=ALPHA):
    """the gradient of a first RMSprop step from square_avg = 0: square_avg = (1 - alpha) g^2, the sign from the step"""
    oma = float(np.float32(1.0 - alpha))     # the float the kernel multiplies g^2 by
    return np.sign(np.asarray(p0, np.float64) - np.asarray(p1, np.float64)) * np.sqrt(np.asarray(sq, np.float64) / oma)


# ------------------------------------------------------------------------------------------------------------ fixtures
def sample_index(n, j):
    """the elements of an n-vector the fixtures keep for update j: every SAMPLE_STRIDE-th from offset j, and the last 256 (the
    heads and the log-std)"""
    return np.unique(np.concatenate([np.arange(j % SAMPLE_STRIDE, n, SAMPLE_STRIDE), np.arange(max(0, n - 256), n)]))


def fixture_updates(g):
    """-> [(prefix, obs [T*N, C, 84, 84] float32, actions [T*N, -1], returns [T*N], lr)] of a fixture's updates"""
    m = g["meta"]
    B = m["T"] * m["N"]
    out = []
    for j in range(m["iters"]):
        pre = f"it{j}_"
        obs = g[pre + "obs"].astype(np.float32)[:-1].reshape(B, m["C"], HW, HW)
        out.append((pre, obs, g[pre + "actions"].reshape(B, -1), g[pre + "returns"][:-1].reshape(B), float(g["lrs"][j])))
    return out
