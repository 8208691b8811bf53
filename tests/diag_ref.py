"""Float64 reference of the update diagnostics (include/simgan_hip.h: sg_rollout_policy_diagnostics), its allowances, and the
cases of tests/test_diag_host.py (CPU) and tests/test_gpu_diag.py (GPU).  Nothing here touches the library.

THE STATISTICS are formed in torch.float64 from forward pieces that already exist and are held to the reference elsewhere:
tests/autograd_ref.py's policy_forward, normal_log_probs and normal_entropy (the GRU states through the real torch.nn.GRU:
gru_states) and the float64 forward of tests/discrete_ref.py.  The float32 constants stay at their float32 value, as everywhere
(autograd_ref: CONSTANTS).

THE RULE.  A statistic passes if |hip - f64| <= 1e-4 |f64| + allowance; `rows` must be exact, and so must `clip_fraction`, whose
allowance is 0 under the conditions below.  1e-4 relative is the project's contract for a forward value, and a statistic's
ALLOWANCE is the largest change of the float64 statistic when every row's new log-prob, entropy and value is moved by 1e-4
relative, in either direction, row by row (the worst sign pattern, not all rows the same way):
  approx_kl, approx_kl_k3, entropy, value_mse   means of a per-row term: the mean of each row's own larger change
  ratio_min, ratio_max                          monotone in every row: the larger change of all rows up / all rows down
  explained_variance_new                        Var(e + u) - Var(e) = 2 cov(e, u) + Var(u) <= 2 mean(|e - mean e| |u|) + mean(u^2)
                                                for e = ret - v_new and |u_i| = 1e-4 |v_new_i|; divided by Var(ret)
  explained_variance_old, rows                  no forward value enters: 0
  clip_fraction                                 0: CONDITIONS keeps every row 1e-3 clip from the edge, two orders beyond what a float32
                                                evaluation moves a ratio by (~1e-6), so a flag that differs is a wrong flag
Statistics that are differences of nearly equal numbers (approx_kl near the on-policy point) inherit their conditioning from this;
they get no number of their own.

CONDITIONS, asserted on the float64 reference alone (conditions()): the clip fraction lies in [0.1, 0.9] with rows beyond the clip
on both sides; no row has ||r - 1| - clip| < 1e-3 clip, so no float32 evaluation within the contract flips a flag; Var(ret) > 0.
The one-row case is exempt from the first (one row cannot lie on both sides) and the last (its variance is 0: both explained
variances are NaN, which is what the case is for).

CASES follow tests/regimes.py's off_policy family (its initialiser, observations, actions drawn from the behaviour policy in
float64) with one change the diagnostics call for: the old log-probs and value predictions are the BEHAVIOUR policy's, and the
policy under test is that policy with perturbed parameters, so ratios lie on both sides of 1 the way they do after an update.  The
same construction serves the Discrete / MultiBinary shapes on tests/discrete_ref.py's initialiser and sampler."""
import functools

import numpy as np
import torch

import autograd_ref as ar
import discrete_ref as dr
import regimes

NAMES = ("rows", "approx_kl", "approx_kl_k3", "clip_fraction", "entropy", "ratio_min", "ratio_max", "explained_variance_old",
         "explained_variance_new", "value_mse")
CLIP = 0.2
REL = 1e-4     # the contract for a forward value
EDGE = 1e-3    # no row within EDGE * clip of the clip edge
EXACT = ("rows", "clip_fraction")
FAULTS = ("kl_sign", "clip_ge", "swap_v", "var_about_zero")


def _t(a):
    return ar.t64(np.asarray(a, np.float64).reshape(-1))


def statistics(logp_new, entropy, v_new, logp_old, vpred, ret, clip=CLIP, fault=None):
    """The ten statistics of NAMES from per-row float64 arrays -> {name: float}.  fault: one of FAULTS, a wrong restatement for the
    test of the test."""
    lpn, ent, v, lpo, vp, R = (_t(x) for x in (logp_new, entropy, v_new, logp_old, vpred, ret))
    if fault == "swap_v":
        v, vp = vp, v
    d = lpn - lpo
    r = d.exp()
    kl = (lpn - lpo).mean() if fault == "kl_sign" else (lpo - lpn).mean()
    beyond = ((r - 1.0).abs() >= clip) if fault == "clip_ge" else ((r - 1.0).abs() > clip)

    def var(x):   # population variance, about the mean
        return (x * x).mean() if fault == "var_about_zero" else ((x - x.mean()) ** 2).mean()

    with np.errstate(all="ignore"):
        out = {"rows": float(d.numel()), "approx_kl": float(kl), "approx_kl_k3": float(((r - 1.0) - d).mean()),
               "clip_fraction": float(beyond.to(ar.F64).mean()), "entropy": float(ent.mean()), "ratio_min": float(r.min()),
               "ratio_max": float(r.max()), "explained_variance_old": float(1.0 - var(R - vp) / var(R)),
               "explained_variance_new": float(1.0 - var(R - v) / var(R)), "value_mse": float(((R - v) ** 2).mean())}
    return out


def allowances(logp_new, entropy, v_new, logp_old, vpred, ret, clip=CLIP):
    """{name: allowance}: see THE RULE."""
    lpn, ent, v, lpo, R = (np.asarray(x, np.float64).reshape(-1) for x in (logp_new, entropy, v_new, logp_old, ret))
    d = lpn - lpo
    u_lp, u_v = REL * np.abs(lpn), REL * np.abs(v)
    k3 = lambda x: np.expm1(x) - x  # noqa: E731
    e = R - v
    var_ret = ((R - R.mean()) ** 2).mean()
    with np.errstate(all="ignore"):
        ev_new = (2.0 * (np.abs(e - e.mean()) * u_v).mean() + (u_v ** 2).mean()) / var_ret
    r_up, r_dn, r = np.exp(d + u_lp), np.exp(d - u_lp), np.exp(d)
    return {"rows": 0.0, "approx_kl": float(u_lp.mean()),
            "approx_kl_k3": float(np.maximum(np.abs(k3(d + u_lp) - k3(d)), np.abs(k3(d - u_lp) - k3(d))).mean()),
            "clip_fraction": 0.0, "entropy": float((REL * np.abs(np.asarray(entropy, np.float64))).mean()),
            "ratio_min": float(max(abs(r_up.min() - r.min()), abs(r_dn.min() - r.min()))),
            "ratio_max": float(max(abs(r_up.max() - r.max()), abs(r_dn.max() - r.max()))),
            "explained_variance_old": 0.0, "explained_variance_new": float(ev_new),
            "value_mse": float((2.0 * np.abs(e) * u_v + u_v ** 2).mean())}


def distance(name, got, want, allow):
    """|got - want| / bound of the rule (0 / 0 -> 0); inf where one side is NaN and the other is not, 0 where both are"""
    if np.isnan(want) or np.isnan(got):
        return 0.0 if (np.isnan(want) and np.isnan(got)) else np.inf
    if np.isinf(want) or np.isinf(got):
        return 0.0 if got == want else np.inf
    err = abs(got - want)
    bound = 0.0 if name in EXACT else REL * abs(want) + allow
    return 0.0 if err == 0.0 else (np.inf if bound == 0.0 else err / bound)


def compare(got, want, allow):
    """-> {name: distance in units of the rule's bound}; a statistic passes at <= 1"""
    return {k: distance(k, float(got[k]), float(want[k]), float(allow[k])) for k in NAMES}


# ------------------------------------------------------------------------------------------------- the forward, per row
def evaluate(c, params=None):
    """Policy.evaluate_actions on the case's T*N rows, time-major -> float64 numpy (v_new [B], logp_new [B], entropy rows [B])"""
    params = c["params"] if params is None else params
    T, N = c["T"], c["N"]
    B = T * N
    obs = c["obs"][:-1].reshape(B, -1)
    with torch.no_grad():
        if c["kind"] in ("cat", "ber"):
            v, lp, ent, _ = dr.evaluate(c["dist"], c["shapes"], params, obs, c["actions"].reshape(B, -1))
            return v, lp, ent
        p = ar.leaves(params, c["shapes"])
        kw = dict(hxs0=c["hxs0"], masks=c["masks"][:-1].reshape(B), T=T) if c["kind"] == "gru" else {}
        v, mean, ls = ar.policy_forward(c["kind"], p, ar.t64(obs), **kw)
        lp = ar.normal_log_probs(mean, ls, ar.t64(c["actions"].reshape(B, -1)))
        ent = (0.5 + ar.HALF_LOG_2PI + ls.exp().log()).sum(-1)     # normal_entropy's rows: its mean is held to it right here
        assert abs(float(ent.mean()) - float(ar.normal_entropy(ls))) <= 1e-12 * max(1.0, abs(float(ent.mean())))
        return v.numpy(), lp.numpy(), ent.numpy()


def rollout_rows(c):
    """float64 (logp_old [B], vpred [B], ret [B]) from the case's float32 rollout arrays"""
    B = c["T"] * c["N"]
    return (c["action_log_probs"].reshape(B).astype(np.float64), c["value_preds"][:-1].reshape(B).astype(np.float64),
            c["returns"][:-1].reshape(B).astype(np.float64))


def reference(c, clip=CLIP, params=None, fault=None):
    """-> (statistics, allowances) of the case at `params` (default: the case's own)"""
    v, lp, ent = evaluate(c, params)
    lpo, vp, R = rollout_rows(c)
    return statistics(lp, ent, v, lpo, vp, R, clip, fault), allowances(lp, ent, v, lpo, vp, R, clip)


def conditions(c, clip=CLIP):
    """Asserts the CONDITIONS on the float64 reference alone; -> dict of what it measured"""
    v, lp, ent = evaluate(c)
    lpo, vp, R = rollout_rows(c)
    r = np.exp(lp - lpo)
    edge = float(np.min(np.abs(np.abs(r - 1.0) - clip)))
    frac = float((np.abs(r - 1.0) > clip).mean())
    out = dict(rows=r.size, clip_fraction=frac, above=int((r > 1.0 + clip).sum()), below=int((r < 1.0 - clip).sum()), edge=edge,
               var_ret=float(R.var()))
    assert edge >= EDGE * clip, f"{c['tag']}: a row {edge:.2e} from the clip edge"
    if r.size > 1:
        assert 0.1 <= frac <= 0.9 and out["above"] >= 1 and out["below"] >= 1, f"{c['tag']}: {out}"
        assert out["var_ret"] > 0.0, c["tag"]
    return out


# ------------------------------------------------------------------------------------------------- cases
def _finish(c, rng, v_b, lp_b, far_returns):
    """the behaviour policy's value and log-prob become the rollout's; returns around the value; the policy under test is moved off
    the behaviour until the clip catches between 0.3 and 0.7 of the rows; rows too near the clip edge get their old log-prob moved"""
    T, N = c["T"], c["N"]
    B = T * N
    z = lambda a: np.concatenate([np.asarray(a, np.float64).reshape(T, N, 1), np.zeros((1, N, 1))]).astype(np.float32)  # noqa: E731
    if far_returns:   # the mean of the returns 1000 standard deviations from 0; a critic that explains half their variance
        ret = 10.0 + 0.01 * rng.standard_normal(B)
        c["returns"], c["value_preds"] = z(ret), z(ret + 0.007 * rng.standard_normal(B))
    else:
        c["returns"], c["value_preds"] = z(v_b + 0.5 * rng.standard_normal(B)), z(v_b)
    c["action_log_probs"] = lp_b.reshape(T, N, 1).astype(np.float32)
    lpo = c["action_log_probs"].reshape(B).astype(np.float64)
    direction = rng.standard_normal(c["behaviour"].shape) * np.abs(c["behaviour"]).mean()
    scale, frac = (1e-3, 0.0) if B > 1 else (0.05, 0.0)   # (one row: a fixed move; there is no fraction to aim at)
    while True:
        c["params"] = (c["behaviour"] + scale * direction).astype(np.float32)
        _, lp, _ = evaluate(c)
        frac = float((np.abs(np.exp(lp - lpo) - 1.0) > CLIP).mean())
        if B == 1 or frac >= 0.3 or scale > 100.0:
            break
        scale *= 1.25
    for _ in range(20):
        near = np.abs(np.abs(np.exp(lp - lpo) - 1.0) - CLIP) < 2.0 * EDGE * CLIP
        if not near.any():
            break
        c["action_log_probs"].reshape(B)[near] -= np.float32(0.01)
        lpo = c["action_log_probs"].reshape(B).astype(np.float64)
    c["scale"] = scale
    return c


@functools.lru_cache(maxsize=None)
def gauss_case(kind, O, A, H, f, T, N, seed=0, far_returns=False):
    """mlp / split / gru with the Gaussian head: regimes' initialiser and off_policy recipe (callers must not write into it)"""
    rng = np.random.default_rng([seed, O, A, H, T, N, {"mlp": 0, "split": 1, "gru": 2}[kind]])
    c = dict(kind=kind, O=O, A=A, H=H, f=f, T=T, N=N, shapes=regimes.param_shapes(kind, O, A, H, f),
             tag=f"diag {kind} ({O}, {A}, {H}, f={f}) T, N = {T}, {N} seed {seed}{' far returns' if far_returns else ''}")
    c["behaviour"] = regimes._init_params(rng, kind, O, A, H, f, 1.0)
    c["obs"] = rng.standard_normal((T + 1, N, O)).astype(np.float32)
    masks = np.ones((T + 1, N, 1), np.float32)
    if kind == "gru":   # episode ends in the middle and at t = 0: the state of slot 0 is dropped for those environments
        if T > 2:
            masks[1:T] = (rng.random((T - 1, N, 1)) > 0.15).astype(np.float32)
            masks[T // 2, 0] = 0.0
        masks[0, ::3] = 0.0
        c["hxs0"] = (0.5 * rng.standard_normal((N, H))).astype(np.float32)
    c["masks"] = masks
    c["actions"] = np.zeros((T, N, A), np.float32)
    with torch.no_grad():
        p = ar.leaves(c["behaviour"], c["shapes"])
        kw = dict(hxs0=c["hxs0"], masks=masks[:-1].reshape(T * N), T=T) if kind == "gru" else {}
        v, mean, ls = (x.numpy() for x in ar.policy_forward(kind, p, ar.t64(c["obs"][:-1].reshape(T * N, O)), **kw))
    c["actions"] = (mean + np.exp(ls) * rng.standard_normal((T * N, A))).reshape(T, N, A).astype(np.float32)
    _, lp_b, _ = evaluate(c, c["behaviour"])
    return _finish(c, rng, v, lp_b, far_returns)


@functools.lru_cache(maxsize=None)
def discrete_case(dist, O, K, H, T, N, seed=0):
    """Discrete(K) / MultiBinary(K): discrete_ref's initialiser and float32 sampler, the same recipe"""
    rng = np.random.default_rng([seed, O, K, H, T, N, 10 + dist])
    c = dict(kind="cat" if dist == dr.CATEGORICAL else "ber", dist=dist, O=O, K=K, A=1 if dist == dr.CATEGORICAL else K, H=H, T=T, N=N,
             shapes=dr.param_shapes(O, K, H), tag=f"diag {'Discrete' if dist == dr.CATEGORICAL else 'MultiBinary'} ({O}, {K}, {H}) "
             f"T, N = {T}, {N} seed {seed}")
    c["behaviour"] = dr.init_params(c["shapes"], seed + 1, head_scale=1.5)
    c["obs"] = rng.standard_normal((T + 1, N, O)).astype(np.float32)
    c["masks"] = np.ones((T + 1, N, 1), np.float32)
    B = T * N
    rows = c["obs"][:-1].reshape(B, O)
    v, _, _, z = dr.evaluate(dist, c["shapes"], c["behaviour"], rows, np.zeros((B, c["A"])))
    c["actions"] = dr.sample(dist, z, rng.random((B, c["A"])).astype(np.float32)).reshape(T, N, c["A"])
    _, lp_b, _ = evaluate(c, c["behaviour"])
    return _finish(c, rng, v, lp_b, False)


# What tests/test_gpu_diag.py runs, by name -> (builder, arguments); tests/test_diag_host.py asserts the conditions on every one.
GEOMETRIES = ((1, 1), (2, 8), (1, 17), (7, 11), (10, 13))     # T*N = 1, 16, 17, 77, 130
CASES = {}
for _T, _N in GEOMETRIES:
    CASES[f"mlp_{_T * _N}"] = (gauss_case, ("mlp", 5, 2, 8, 1, _T, _N))
CASES["split_77"] = (gauss_case, ("split", 14, 7, 100, 1, 7, 11))
CASES["split_33"] = (gauss_case, ("split", 14, 7, 100, 1, 3, 11))
for _O, _K, _H in dr.SHAPES[dr.CATEGORICAL]:
    CASES[f"discrete_{_K}"] = (discrete_case, (dr.CATEGORICAL, _O, _K, _H, 7, 11))
CASES["multibinary_5"] = (discrete_case, (dr.BERNOULLI, 11, 5, 64, 7, 11))
CASES["mlp_h256"] = (gauss_case, ("mlp", 47, 12, 256, 1, 3, 11))          # the global-weight path by itself
CASES["mlp_large"] = (gauss_case, ("mlp", 5, 2, 8, 1, 129, 520))          # 67,080 rows: 1,049 records through the reduce
CASES["gru_9_17"] = (gauss_case, ("gru", 13, 5, 20, 1, 9, 17))            # two scan workgroups
CASES["gru_5_1"] = (gauss_case, ("gru", 13, 5, 20, 1, 5, 1, 2))         # seed 2: the first at which five rows meet the conditions
CASES["mlp_far_returns"] = (gauss_case, ("mlp", 5, 2, 8, 1, 7, 11, 0, True))


def case(name):
    fn, args = CASES[name]
    return fn(*args)
