"""Float64 reference of the discriminator diagnostics (include/simgan_hip.h: sg_disc_diagnostics), its allowances, and the cases
of tests/test_disc_diag_host.py (CPU) and tests/test_gpu_disc_diag.py (GPU).  Nothing here touches the library.

THE STATISTICS.  Logits from disc_regimes.logits64, rewards from disc_regimes.reward64 (the float32 constant 1e-7 at its float32
value).  The input gradient dD/dx per row comes from torch.autograd.grad in float64 on the forward written out (gnorm_autograd):
the independent party; the closed-form numpy gradient (gnorm_closed) serves the faults and is held to it within 1e-9
(tests/test_disc_diag_host.py).  The three populations: policy = obs_feat[1:] of the rollout, expert = the expert matrix,
mid[i] = 0.5f * expert[i mod n_e] + 0.5f * policy[i] formed in float32 (both products are exact, the sum rounds once, in any
order and with or without a fused multiply-add), as the kernel forms it.

THE RULE (tests/diag_ref.py's).  A statistic passes if |hip - f64| <= 1e-4 |f64| + allowance.  The allowance is the largest
change of the float64 statistic when every row's logit and |g| moves by 1e-4 |value| + 1e-5 (helpers.RTOL / ATOL), the worst
sign pattern, row by row:
  *_logit_mean, *_grad_norm_mean, *_bce, mid_grad_pen   means of a per-row term: the mean of each row's own larger change
  *_std                                                 Var(x + u) - Var(x) <= 2 mean(|x - mean x| |u|) + mean(u^2), through the root
  reward_min, reward_max, grad_norm_max                 every row up / every row down
  reward_*                                              a row's reward moves by its change under the logit's move PLUS
                                                        C_ENV * disc_regimes.reward_envelope(s): the conditioning of the reward in
                                                        the float32 sigmoid (C_ENV = 2, tests/test_gpu_disc_regimes.py's constant,
                                                        derived from the float32 oracle in tests/test_disc_regimes_host.py)
  the two row counts, the two accuracies                exact: allowance 0 (CONDITIONS keep every logit 1e-3 from 0, two orders
                                                        beyond what the contract moves it by)

CONDITIONS, asserted on the float64 reference alone (conditions()): no row has |d| < 1e-3; both accuracies lie in [0.1, 0.9]
unless the population is one row; on both_sides cases the mid rows hold at least 8 rows with |g| > 1.1 and 8 with |g| < 0.9;
reward_std > 0 wherever there is more than one row.  The builder moves the head's bias between the two populations' medians,
moves rows too near d = 0, and takes the next seed (and, both_sides, the next weight scale within [2, 3]) until they hold.
ONE case is exempt by construction: zero_head (4.weight = 0, 4.bias = 0, one row each), whose logits are exactly 0 in every
arithmetic -- the case `d == 0 is wrong for both` needs."""
import functools

import numpy as np
import torch

import disc_regimes as rg
from helpers import ATOL, RTOL

NAMES = ("policy_rows", "expert_rows", "policy_accuracy", "expert_accuracy", "policy_logit_mean", "policy_logit_std",
         "expert_logit_mean", "expert_logit_std", "policy_bce", "expert_bce", "reward_mean", "reward_std", "reward_min", "reward_max",
         "policy_grad_norm_mean", "expert_grad_norm_mean", "mid_grad_norm_mean", "mid_grad_pen", "grad_norm_max")
EXACT = ("policy_rows", "expert_rows", "policy_accuracy", "expert_accuracy")
LAMBDA = 10.0
EDGE = 1e-3        # no logit within EDGE of 0
C_ENV = 2.0
CAP = 0.05         # an allowance is at most CAP * max(|statistic|, 1): tests/test_disc_diag_host.py
# fault -> the statistic it breaks (tests/test_disc_diag_host.py: each fails the rule there on at least one case)
FAULTS = {"expert_acc_lt": "expert_accuracy", "acc_ge": "policy_accuracy", "bce_swapped": "policy_bce", "sample_std": "policy_logit_std",
          "mid_clamped": "mid_grad_norm_mean", "no_s1": "mid_grad_norm_mean", "pen_sq": "mid_grad_pen", "gmax_policy_only": "grad_norm_max"}


# ------------------------------------------------------------------------------------------------- the input gradient
def gnorm_autograd(params, F, Hd, x):
    """|dD/dx| per row of x [n, F]: torch.autograd.grad in float64 on the forward written out"""
    W1, b1, W2, b2, w3, b3 = (torch.tensor(np.asarray(a, np.float64)) for a in rg._unpack(params, F, Hd))
    X = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    d = torch.tanh(torch.tanh(X @ W1.T + b1) @ W2.T + b2) @ w3 + b3
    g, = torch.autograd.grad(d.sum(), X)     # rows are independent: the gradient of the sum holds every row's own
    return g.norm(dim=1).numpy()


def gnorm_closed(params, F, Hd, x, drop_s1=False):
    """numpy float64: g = ((w3 (1 - h2^2)) W2 (1 - h1^2)) W1.  drop_s1: the fault without layer 1's 1 - h1^2"""
    W1, b1, W2, b2, w3, _ = rg._unpack(params, F, Hd)
    h1 = np.tanh(np.asarray(x, np.float64) @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    d1 = (w3 * (1.0 - h2 * h2)) @ W2
    if not drop_s1:
        d1 = d1 * (1.0 - h1 * h1)
    return np.sqrt(((d1 @ W1) ** 2).sum(-1))


def mid_rows(expert, policy, clamped=False):
    n_p, n_e = policy.shape[0], expert.shape[0]
    idx = np.minimum(np.arange(n_p), n_e - 1) if clamped else np.arange(n_p) % n_e
    return (np.float32(0.5) * expert[idx] + np.float32(0.5) * policy).astype(np.float32)


def rows(c, fault=None, params=None):
    """per-row float64 arrays of the case at `params` (default: its own): logits of policy / expert, |g| of policy / expert / mid"""
    p = c.params if params is None else np.asarray(params, np.float32)
    F, Hd = c.F, c.Hd
    mid = mid_rows(c.expert, c.policy, clamped=fault == "mid_clamped")
    gn = (lambda x: gnorm_closed(p, F, Hd, x, drop_s1=True)) if fault == "no_s1" else (lambda x: gnorm_autograd(p, F, Hd, x))
    return dict(d_p=rg.logits64(p, F, Hd, c.policy), d_e=rg.logits64(p, F, Hd, c.expert), g_p=gn(c.policy), g_e=gn(c.expert), g_m=gn(mid))


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def statistics(r, fault=None):
    """the nineteen statistics of NAMES from rows() -> {name: float}.  fault: one of FAULTS, a wrong restatement"""
    d_p, d_e, g_p, g_e, g_m = r["d_p"], r["d_e"], r["g_p"], r["g_e"], r["g_m"]
    rew, _ = rg.reward64(d_p)
    std = lambda x: float(x.std(ddof=1 if fault == "sample_std" and x.size > 1 else 0))  # noqa: E731
    if fault == "acc_ge":
        acc_p, acc_e = (d_p <= 0).mean(), (d_e >= 0).mean()
    else:
        acc_p, acc_e = (d_p < 0).mean(), ((d_e < 0) if fault == "expert_acc_lt" else (d_e > 0)).mean()
    bce_p, bce_e = (softplus(-d_p), softplus(d_e)) if fault == "bce_swapped" else (softplus(d_p), softplus(-d_e))
    pen = (g_m ** 2 - 1.0) ** 2 if fault == "pen_sq" else (g_m - 1.0) ** 2
    gmax = g_p.max() if fault == "gmax_policy_only" else max(g_p.max(), g_e.max(), g_m.max())
    with np.errstate(all="ignore"):
        vals = (d_p.size, d_e.size, acc_p, acc_e, d_p.mean(), std(d_p), d_e.mean(), std(d_e), bce_p.mean(), bce_e.mean(),
                rew.mean(), std(rew), rew.min(), rew.max(), g_p.mean(), g_e.mean(), g_m.mean(), LAMBDA * pen.mean(), gmax)
    return {k: float(v) for k, v in zip(NAMES, vals)}


def _std_allow(x, u):
    var = ((x - x.mean()) ** 2).mean()
    dv = 2.0 * (np.abs(x - x.mean()) * u).mean() + (u ** 2).mean()
    return float(max(np.sqrt(var + dv) - np.sqrt(var), np.sqrt(var) - np.sqrt(max(var - dv, 0.0))))


def _ext_allow(x, u, ext):
    return float(max(abs(ext(x + u) - ext(x)), abs(ext(x - u) - ext(x))))


def allowances(r):
    """{name: allowance}: see THE RULE."""
    d_p, d_e, g_p, g_e, g_m = r["d_p"], r["d_e"], r["g_p"], r["g_e"], r["g_m"]
    u = lambda x: RTOL * np.abs(x) + ATOL  # noqa: E731
    rew, s = rg.reward64(d_p)
    u_r = np.maximum(np.abs(rg.reward64(d_p + u(d_p))[0] - rew), np.abs(rg.reward64(d_p - u(d_p))[0] - rew)) + C_ENV * rg.reward_envelope(s)
    sp_move = lambda z: np.maximum(np.abs(softplus(z + u(z)) - softplus(z)), np.abs(softplus(z - u(z)) - softplus(z))).mean()  # noqa: E731
    pen = lambda g: (g - 1.0) ** 2  # noqa: E731
    g_all, u_all = np.concatenate([g_p, g_e, g_m]), np.concatenate([u(g_p), u(g_e), u(g_m)])
    out = dict.fromkeys(EXACT, 0.0)
    out.update(policy_logit_mean=u(d_p).mean(), policy_logit_std=_std_allow(d_p, u(d_p)), expert_logit_mean=u(d_e).mean(),
               expert_logit_std=_std_allow(d_e, u(d_e)), policy_bce=sp_move(d_p), expert_bce=sp_move(-d_e),
               reward_mean=u_r.mean(), reward_std=_std_allow(rew, u_r), reward_min=_ext_allow(rew, u_r, np.min),
               reward_max=_ext_allow(rew, u_r, np.max), policy_grad_norm_mean=u(g_p).mean(), expert_grad_norm_mean=u(g_e).mean(),
               mid_grad_norm_mean=u(g_m).mean(),
               mid_grad_pen=LAMBDA * np.maximum(np.abs(pen(g_m + u(g_m)) - pen(g_m)), np.abs(pen(g_m - u(g_m)) - pen(g_m))).mean(),
               grad_norm_max=_ext_allow(g_all, u_all, np.max))
    return {k: float(out[k]) for k in NAMES}


def distance(name, got, want, allow):
    """|got - want| / bound of the rule (0 / 0 -> 0); inf where one side is not finite and the other differs"""
    if not (np.isfinite(want) and np.isfinite(got)):
        return 0.0 if (got == want or (np.isnan(want) and np.isnan(got))) else np.inf
    err = abs(got - want)
    bound = 0.0 if name in EXACT else RTOL * abs(want) + allow
    return 0.0 if err == 0.0 else (np.inf if bound == 0.0 else err / bound)


def compare(got, want, allow):
    """-> {name: distance in units of the rule's bound}; a statistic passes at <= 1"""
    return {k: distance(k, float(got[k]), float(want[k]), float(allow[k])) for k in NAMES}


def reference(c, fault=None, params=None):
    """-> (statistics, allowances); the allowances are always the unfaulted reference's"""
    if fault is None and params is None:
        return _reference0(c.name)
    return statistics(rows(c, fault, params), fault), allowances(rows(c, None, params))


@functools.lru_cache(maxsize=None)
def _reference0(name):
    r = rows(case(name))
    return statistics(r), allowances(r)


# ------------------------------------------------------------------------------------------------- cases
def conditions(c):
    """Asserts the CONDITIONS on the float64 reference alone; -> dict of what it measured"""
    r = rows(c)
    st = statistics(r)
    out = dict(edge=float(min(np.abs(r["d_p"]).min(), np.abs(r["d_e"]).min())), policy_accuracy=st["policy_accuracy"],
               expert_accuracy=st["expert_accuracy"], mid_above=int((r["g_m"] > 1.1).sum()), mid_below=int((r["g_m"] < 0.9).sum()),
               reward_std=st["reward_std"], reward_abs_max=max(abs(st["reward_min"]), abs(st["reward_max"])))
    if c.get("zero_head"):
        assert out["edge"] == 0.0 and c.policy.shape[0] == 1 and c.expert.shape[0] == 1, c.tag
        return out
    assert out["edge"] >= EDGE, f"{c.tag}: a row with |d| = {out['edge']:.2e}"
    if c.policy.shape[0] > 1:
        assert 0.1 <= out["policy_accuracy"] <= 0.9, f"{c.tag}: {out}"
        assert out["reward_std"] > 0.0, c.tag
    if c.expert.shape[0] > 1:
        assert 0.1 <= out["expert_accuracy"] <= 0.9, f"{c.tag}: {out}"
    if c.regime == "saturated":     # logits of both signs (the accuracies above) and rewards well into the tails
        assert out["reward_abs_max"] >= 6.0, f"{c.tag}: {out}"
    if c.regime == "both_sides":
        assert out["mid_above"] >= 8 and out["mid_below"] >= 8, f"{c.tag}: {out}"
    return out


def build(F, Hd, T, N, n_e, regime, seed, scale_w=None, shift=0.0):
    """disc_regimes' initialiser and row recipe at the regime's scales; expert rows around `shift` (in units of scale_x) more"""
    sw, sx = rg.SCALES[regime]
    sw = (rg.BOTH_SIDES_SCALE_W.get((F, Hd), sw) if regime == "both_sides" else sw) if scale_w is None else scale_w
    n_p = T * N
    rng = np.random.default_rng([seed, F, Hd, n_p, n_e, 91])
    c = rg.Case(F=F, Hd=Hd, T=T, N=N, regime=regime, seed=seed, scale_w=sw, scale_x=sx,
                tag=f"ddiag {regime}({sw:g}, {sx:g}) {F}x{Hd} T, N = {T}, {N} n_e {n_e} seed {seed}{f' shift {shift:g}' if shift else ''}")
    params = rg.init_params(rng, F, Hd, sw)
    c["expert"] = (sx * (0.7 * rng.standard_normal((n_e, F)) + 0.2 + shift)).astype(np.float32)
    c["policy"] = (sx * rng.standard_normal((n_p, F))).astype(np.float32)
    # the head's bias between the two populations' medians: logits of both signs among both
    b3 = rg.block_slice(F, Hd, "4.bias")
    params[b3] = 0.0
    params[b3] = np.float32(-0.5 * (np.median(rg.logits64(params, F, Hd, c.policy)) + np.median(rg.logits64(params, F, Hd, c.expert))))
    c["params"] = params
    for x in (c["policy"], c["expert"]):     # rows too near d = 0 are moved, a little at a time, until none is
        for _ in range(50):
            near = np.abs(rg.logits64(params, F, Hd, x)) < 2.0 * EDGE
            if not near.any():
                break
            x[near] += (0.05 * sx * rng.standard_normal((int(near.sum()), F))).astype(np.float32)
    return c


# name -> (F, Hd, T, N, n_e, regime, shift).  T x N = 1x1, 2x8, 1x17, 7x11, 10x13 (1, 16, 17, 77, 130 rows: one row, half a 32-row
# tile, a ragged second tile ...), n_e = 1, 16, 17, 100, 200 (> T*N = 77: no wrap) and 17 < T*N = 130 (the pairing wraps)
SPECS = {
    "init_7x16_1x1_e1": (7, 16, 1, 1, 1, "init", 0.0),
    "init_7x16_2x8_e16": (7, 16, 2, 8, 16, "init", 0.0),
    "sat_7x16_1x17_e17": (7, 16, 1, 17, 17, "saturated", 0.0),
    "both_7x16_7x11_e200": (7, 16, 7, 11, 200, "both_sides", 0.0),
    "both_7x16_10x13_e17": (7, 16, 10, 13, 17, "both_sides", 0.0),
    "init_86x100_1x17_e100": (86, 100, 1, 17, 100, "init", 0.0),
    "both_86x100_7x11_e100": (86, 100, 7, 11, 100, "both_sides", 0.0),
    "sat_86x100_10x13_e17": (86, 100, 10, 13, 17, "saturated", 0.0),
    "both_86x100_7x11_e100_shifted": (86, 100, 7, 11, 100, "both_sides", 0.25),   # the two accuracies differ, and from 0.5
    "init_150x256_2x8_e1": (150, 256, 2, 8, 1, "init", 0.0),                      # the global-weight instance on its own
    "both_150x256_7x11_e16": (150, 256, 7, 11, 16, "both_sides", 0.0),
    "sat_150x256_10x13_e100": (150, 256, 10, 13, 100, "saturated", 0.0),
    "both_7x16_large": (7, 16, 129, 520, 1000, "both_sides", 0.0),   # 67,080 rows: more tiles than the capped grid, several trips
}
BOTH_SIDES_SCALES = (None, 2.0, 2.25, 2.75, 3.0)    # None: disc_regimes' own for the shape
MAX_SEED = 40


@functools.lru_cache(maxsize=None)
def case(name):
    """the first (seed, scale) at which the conditions hold; computed once per process and shared (callers must not write into it)"""
    if name == "zero_head":
        c = build(7, 16, 1, 1, 1, "init", 0)
        p = c.params.copy()
        p[rg.block_slice(7, 16, "4.weight")] = 0.0
        p[rg.block_slice(7, 16, "4.bias")] = 0.0
        c["params"], c["zero_head"], c["tag"], c["name"] = p, True, c.tag + ", 4.weight = 4.bias = 0", name
        conditions(c)
        return c
    F, Hd, T, N, n_e, regime, shift = SPECS[name]
    last = None
    for seed in range(MAX_SEED):
        for sw in (BOTH_SIDES_SCALES if regime == "both_sides" else (None,)):
            c = build(F, Hd, T, N, n_e, regime, seed, sw, shift)
            c["name"] = name
            try:
                conditions(c)
            except AssertionError as exc:
                last = exc
                continue
            return c
    raise AssertionError(f"{name}: no seed below {MAX_SEED} meets the conditions; the last miss: {last}")


CASES = tuple(SPECS) + ("zero_head",)
