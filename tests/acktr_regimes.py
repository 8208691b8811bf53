"""Case builders for ACKTR's numerical regimes (tests/test_acktr_regimes_host.py on the CPU, tests/test_gpu_acktr_regimes.py on
the GPU).  tests/test_gpu_acktr.py holds the K-FAC kernels to one number, rel-L2 of the whole Delta p under the constructor
defaults, and on its cases (the float64 restatement alone shows it, tests/test_acktr_regimes_host.py):
  * the KL clip is active in every update, nu = 0.009 .. 0.8, so the step nu v is invariant under a rescaling of the gradient;
  * the small blocks (critic_linear.bias, dist.fc_mean.bias, dist.logstd) are 5e-4 .. 4e-2 of ||Delta p||;
  * at the shapes that reach the chunked rows and the eigensolver's global-memory path d_g d_a is below the damping on nearly
    every pair, so v ~ g / damping and the eigenbases hardly reach Delta p;
  * nothing but KFAC_DEFAULTS is ever passed to sg_acktr_create.
Here every case is a (shape, per-update inputs, sg_acktr_config) triple, described in float64 by update() below, the restatement
of tests/test_acktr_host.py generalised (float32 as well as float64; nu, v g lr^2, v before nu, every factor and its
eigenvalues per update); the builder ASSERTS on that description that the case reaches what it claims:

  unclipped          v g lr^2 <= 0.8 kl_clip: nu = 1, the branch of k_kfac_step no other test runs, and the step's scale is the
                     gradient's.  One case under the constructor defaults (actions drawn from the policy's own Gaussian, returns
                     near its values, 65,536 rows); the others through a large kl_clip in the config;
  clipped            nu in (0.5, 0.95), and nu < 0.1;
  eigen_dominated    unit-gain weights, damping 1e-5: the median of d_g d_a over every weight module's pairs is >= 10 x damping, and
                     no eigenvalue of any factor lies in [1e-7, 1e-5], where float32 could decide the 1e-6 threshold otherwise;
  damping_dominated  damping 1e6: v damping is ACKTR mode's gradient itself, block by block and with its scale visible;
  threshold          DROPPED (see DROPPED below): with eigenvalues on both sides of 1e-6 and a damping small enough for the
                     zeroing to show in v, the float32 evaluation itself is 1.6e-4 .. 1.1e-3 from float64;
  refresh            Tf = 2, momentum 0, four updates on changing rollouts: updates 1 and 3 use stale eigenbases with fresh
                     gradients, update 2 decomposes running-average factors.

Every update of a case starts from prescribed float32 parameters (the float64 trajectory's, rounded), so an update is judged on
its own; the K-FAC state (running factors, eigenbases) is carried.  With momentum 0, and on the first update with any momentum, the
momentum buffer is nu v of that very update.  The config values are float32 numbers (sg_acktr_config's fields), held as doubles.

A case is kept only if the float32 evaluation of the same algorithm stays within COND = 1e-4 of float64 on every block of nu v,
every block of Delta p and every factor (the largest over the evaluation and JITTERS more with inputs moved by an ulp).

Blocks are KFACOptimizer's 13 modules in state_dict order; factors are the 12 distinct ones."""
import functools

import numpy as np

from helpers import ATOL
from test_a2c_host import a2c_loss_grad, policy_slices
from test_acktr_host import MODULES

COND = 1e-4           # a case judges something only where float32 itself is within this of float64
JITTERS = 3
VCOEF, ECOEF = 0.5, 0.01
EIG_THRESHOLD = 1e-6  # kfac.py:236-237
CHUNK = 4096          # SG_A2C_CHUNK_ROWS (simgan_amd/csrc/sg_ppo.hip): rows per k_ppo_fwd .. k_kfac_stats pass
ZEROING_SHOWS = 100 * COND   # threshold: v with the sub-threshold eigenvalues kept is this far (rel-L2) from v, 50 x the HIP bound
BIG_KL = 1e30         # a kl_clip no step reaches: nu = 1

BLOCKS = ["actor.0.weight", "actor.0.bias", "actor.2.weight", "actor.2.bias", "critic.0.weight", "critic.0.bias", "critic.2.weight",
          "critic.2.bias", "critic_linear.weight", "critic_linear.bias", "dist.fc_mean.weight", "dist.fc_mean.bias", "dist.logstd"]
WEIGHT_BLOCKS = [b for b in BLOCKS if b.endswith("weight")]
FACTORS = ["A.obs", "A.actor_h1", "A.actor_h2", "A.critic_h1", "A.critic_h2", "G.actor.0", "G.actor.2", "G.critic.0", "G.critic.2",
           "G.critic_linear", "G.dist.fc_mean", "G.dist.logstd"]
# the module (index into BLOCKS) whose m_aa / m_gg of get_kfac() is each distinct factor
A_FROM_MODULE = [0, 2, 10, 6, 8]
G_FROM_MODULE = [0, 2, 4, 6, 8, 10, 12]


def f32(x):
    return float(np.float32(x))


def config(lr=0.25, momentum=0.9, stat_decay=0.99, kl_clip=0.001, damping=0.01, Tf=10):
    """sg_acktr_config's K-FAC fields as the float32 numbers the library receives (defaults: KFACOptimizer's)"""
    return dict(lr=f32(lr), momentum=f32(momentum), stat_decay=f32(stat_decay), kl_clip=f32(kl_clip), damping=f32(damping), Tf=int(Tf))


class Case(dict):
    __getattr__ = dict.__getitem__


def new_state():
    return {"mA": None, "mG": None, "eA": None, "eG": None, "raw": None, "buf": None, "steps": 0}


def update(params, state, obs, actions, returns, eps, dims, vcoef, ecoef, kfac, dtype=np.float64, grad_scale=1.0):
    """tests/test_acktr_host.py's acktr_update_restated, evaluated in `dtype` -> (params1, losses[3], state, info).  grad_scale: a
    fault to inject, the gradient handed to the preconditioning times this (a 1 / B off by a factor).  info: nu,
    vg (v g lr^2), v (flat, before nu), g (the gradient), step (nu v), refreshed (this update decomposed the factors), eig
    (every distinct factor's eigenvalues before the threshold, as of the last refresh), mA / mG (the running factors)."""
    f = np.dtype(dtype).type
    O, A, H, Hc = dims
    obs = np.asarray(obs, dtype)
    T, N = obs.shape[0] - 1, obs.shape[1]
    B = T * N
    sl, n = policy_slices(O, A, H, Hc)
    flat = np.asarray(params, dtype)
    p = {k: flat[s].reshape(shape) for k, (s, shape) in sl.items()}
    x = obs[:T].reshape(-1, O)
    act = np.asarray(actions, dtype).reshape(-1, A)
    losses, g = a2c_loss_grad(flat, x, act, np.asarray(returns, dtype)[:T].reshape(-1), dims, vcoef, ecoef, dtype)
    g = g * f(grad_scale)
    one = f(1.0)
    a1 = np.tanh(x @ p["aw1"].T + p["ab1"])
    a2 = np.tanh(a1 @ p["aw2"].T + p["ab2"])
    mu = a2 @ p["mw"].T + p["mb"]
    c1 = np.tanh(x @ p["cw1"].T + p["cb1"])
    c2 = np.tanh(c1 @ p["cw2"].T + p["cb2"])
    var = np.exp(f(2.0) * p["ls"])
    diff = act - mu
    gmu = -diff / var / f(B)
    gls = -(diff * diff / var - one) / f(B)
    gv = f(2.0) * np.asarray(eps, dtype).reshape(-1, 1) / f(B)
    za2 = (gmu @ p["mw"]) * (one - a2 * a2)
    za1 = (za2 @ p["aw2"]) * (one - a1 * a1)
    zc2 = (gv @ p["vw"]) * (one - c2 * c2)
    zc1 = (zc2 @ p["cw2"]) * (one - c1 * c1)
    fA = [u.T @ u / f(B) for u in (x, a1, a2, c1, c2)]
    fG = [f(B) * (u.T @ u) for u in (za1, za2, zc1, zc2, gv, gmu, gls)]
    sd = kfac["stat_decay"]
    m_scale, f_scale = f(sd / (1.0 - sd)), f(1.0 - sd)
    first = state["steps"] == 0
    mA = [((fa if first else m) * m_scale + fa) * f_scale for fa, m in zip(fA, state["mA"] or fA)]
    mG = [((fg if first else m) * m_scale + fg) * f_scale for fg, m in zip(fG, state["mG"] or fG)]
    eA, eG, raw = state["eA"], state["eG"], state["raw"]
    refreshed = state["steps"] % kfac["Tf"] == 0
    if refreshed:
        raw = []

        def eig(m):
            d, q = np.linalg.eigh(m, UPLO="U")
            raw.append(np.asarray(d, np.float64))
            return d * (d > f(EIG_THRESHOLD)), q
        eA, eG = [eig(m) for m in mA], [eig(m) for m in mG]
    unit = (np.ones(1, dtype), np.ones((1, 1), dtype))
    v = np.zeros(n, dtype)
    damping = f(kfac["damping"])
    for key, fa, fg in MODULES:
        s, shape = sl[key]
        grad = g[s].reshape(shape[0], -1) if len(shape) == 2 else g[s].reshape(-1, 1)
        da, qa = unit if fa is None else eA[fa]
        dg, qg = eG[fg]
        v1 = qg.T @ grad @ qa
        v2 = v1 / (dg[:, None] * da[None, :] + damping)
        v[s] = (qg @ v2 @ qa.T).reshape(-1)
    lr = kfac["lr"]
    vg = float(np.sum(v.astype(np.float64) * g.astype(np.float64))) * lr * lr     # (k_kfac_step sums in double)
    nu = min(1.0, float(np.sqrt(kfac["kl_clip"] / vg))) if vg > 0 else 1.0
    step = f(nu) * v
    mom = f(kfac["momentum"])
    buf = step if first else mom * state["buf"] + step
    p1 = flat - f(lr * (1.0 - kfac["momentum"])) * buf
    new = {"mA": mA, "mG": mG, "eA": eA, "eG": eG, "raw": raw, "buf": buf, "steps": state["steps"] + 1}
    info = Case(nu=nu, vg=vg, v=v, g=g, step=step, refreshed=refreshed, eig=raw, mA=mA, mG=mG, eA=eA, eG=eG)
    return p1, np.array(losses), new, info


# ------------------------------------------------------------------------------------------- distances
def block_slices(dims):
    sl, n = policy_slices(*dims)
    return {name: sl[key][0] for name, (key, _, _) in zip(BLOCKS, MODULES)}, n


def block_distances(got, ref, dims, atol=ATOL):
    """{block: ||got - ref||_2 / (||ref||_2 + atol max|ref| sqrt(n))}: tests/disc_regimes.py's formula, the floor on the scale of
    the whole vector's largest element"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    slices, n = block_slices(dims)
    assert got.shape == ref.shape == (n,), (got.shape, ref.shape, n)
    scale = atol * np.max(np.abs(ref))
    return {name: float(np.linalg.norm(got[s] - ref[s]) / (np.linalg.norm(ref[s]) + scale * np.sqrt(ref[s].size) + 1e-300))
            for name, s in slices.items()}


def whole_vector_distance(got, ref):
    """tests/test_gpu_acktr.py's measure: rel-L2 over all parameters"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))


def distinct_factors(m_aa, m_gg):
    """get_kfac()'s 13 + 13 per-module factors -> the 12 distinct ones in FACTORS order"""
    return [np.asarray(m_aa[i], np.float64) for i in A_FROM_MODULE] + [np.asarray(m_gg[i], np.float64) for i in G_FROM_MODULE]


def state_factors(info):
    return [np.asarray(m, np.float64) for m in list(info["mA"]) + list(info["mG"])]


def factor_distances(got, ref):
    """{factor: ||got - ref||_F / ||ref||_F}: each factor relative to its own Frobenius norm"""
    assert len(got) == len(ref) == len(FACTORS)
    out = {}
    for name, a, b in zip(FACTORS, got, ref):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        out[name] = float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))
    return out


def measures(p0, p1, step, factors, ref, dims):
    """every distance of one update from the float64 description `ref` (a describe() entry): {"nuv": blocks, "dp": blocks,
    "factors": factors}"""
    dp = np.asarray(p1, np.float64) - np.asarray(p0, np.float64)
    return {"nuv": block_distances(step, ref["step"], dims), "dp": block_distances(dp, ref["dp"], dims),
            "factors": factor_distances(factors, ref["factors"])}


def worst(m):
    return max(max(d.values()) for d in m.values())


# ------------------------------------------------------------------------------------------- inputs
def draw_params(rng, dims, gain, zero_bias=False, value_head_gain=1.0, logstd=None):
    """tests/test_gpu_acktr.py's _random_case weights at `gain` (0.2 there); zero_bias: every Linear bias 0, the reference's own
    initialisation, so that a bias block's Delta p is exact in float32 however small the step"""
    O, A, H, Hc = dims
    sl, n = policy_slices(*dims)
    params = (gain * rng.standard_normal(n) / np.sqrt(max(O, H))).astype(np.float32)
    params[-A:] = -0.5 + 0.1 * rng.standard_normal(A)
    if logstd is not None:
        params[-A:] = logstd
    params[sl["vw"][0]] *= np.float32(value_head_gain)    # scales both critic G factors by its square
    if zero_bias:
        for key in ("ab1", "ab2", "cb1", "cb2", "vb", "mb"):
            params[sl[key][0]] = 0.0
    return params


def forward64(params, x, dims):
    """float64: (mu, std, v) of rows x"""
    sl, _ = policy_slices(*dims)
    flat = np.asarray(params, np.float64)
    p = {k: flat[s].reshape(shape) for k, (s, shape) in sl.items()}
    x = np.asarray(x, np.float64)
    a2 = np.tanh(np.tanh(x @ p["aw1"].T + p["ab1"]) @ p["aw2"].T + p["ab2"])
    c2 = np.tanh(np.tanh(x @ p["cw1"].T + p["cb1"]) @ p["cw2"].T + p["cb2"])
    return a2 @ p["mw"].T + p["mb"], np.exp(p["ls"]), (c2 @ p["vw"].T + p["vb"])


def draw_rollout(rng, params, dims, T, N, on_policy=None, obs_scale=None):
    """tests/test_gpu_acktr.py's _random_case rows: N(0, 1) observations and actions, 0.5 N(0, 1) returns, N(0, 1) value noise.
    on_policy = s: actions from the policy's own Gaussian and returns = its values + s (a unit-variance linear function of the
    observation + 0.1 N(0, 1)).  obs_scale: per-column factors (the threshold case)."""
    O, A, _, _ = dims
    obs = rng.standard_normal((T + 1, N, O))
    if obs_scale is not None:
        obs = obs * np.asarray(obs_scale)
    obs = obs.astype(np.float32)
    noise = rng.standard_normal((T, N, A))
    ret_noise = rng.standard_normal((T + 1, N, 1))
    eps = rng.standard_normal((T, N, 1)).astype(np.float32)
    if on_policy is None:
        actions, returns = noise, 0.5 * ret_noise
    else:
        mu, std, v = forward64(params, obs.reshape(-1, O), dims)
        actions = mu.reshape(T + 1, N, A)[:T] + std * noise
        w = rng.standard_normal((O, 1)) / np.sqrt(O)        # a value error the critic can fit: linear in the observation
        returns = v.reshape(T + 1, N, 1) + on_policy * (obs.astype(np.float64) @ w + 0.1 * ret_noise)
    return dict(obs=obs, actions=actions.astype(np.float32), returns=returns.astype(np.float32), eps=eps)


# ------------------------------------------------------------------------------------------- the cases
# name -> regime, dims (O, A, H, Hc), T, N, gain, config, seed, updates, extras.  What each shape is there for:
#   k_kfac_stats' 16x16 tiles       factor widths 5, 17, 47 (47x5x17) and 16 (11x3x16), row counts that are no multiple of 4 (63,
#                                   4097, 4098, 4099, 65)
#   the row loop's chunks           CHUNK + 1, + 2, + 3 rows: a partial second chunk of 1 .. 3 rows
#   k_kfac_gemm's 32x32 tiles       widths 31, 32, 33 (31 observations, 32 actions, hidden 33)
#   k_kfac_eig, LDS against global  hidden 98 / 99 (16 n^2 bytes + 8 KB against a 160 KB CU) and 128 / 129
#   global path on a running average  refresh at hidden 129
#   global-weight A2C instances     150x8x256 in eigen_dominated, B = 512
#   Hc != H                         47x5x17 with the 64-wide critic of Policy.reset_critic (the only other width the library builds)
_EIG = dict(regime="eigen_dominated", gain=1.4, value_head_gain=10.0, T=8, N=64)
SPECS = {
    "unclipped_default":   dict(regime="unclipped", dims=(11, 3, 16, 16), T=512, N=128, gain=0.1, cfg=config(), on_policy=0.35, zero_bias=True),
    "unclipped_tiles16":   dict(regime="unclipped", dims=(47, 5, 17, 64), T=7, N=9, gain=0.2, cfg=config(kl_clip=1e3)),
    "unclipped_tiles32":   dict(regime="unclipped", dims=(31, 32, 33, 33), T=17, N=241, gain=0.2, cfg=config(kl_clip=1e3, momentum=0.0)),
    "clipped_mild":        dict(regime="clipped", dims=(11, 3, 16, 16), T=6, N=683, gain=0.2, cfg=config(kl_clip=2.6e-4, momentum=0.0),
                                nu=(0.5, 0.95)),
    "clipped_hard":        dict(regime="clipped", dims=(47, 12, 64, 64), T=1, N=4099, gain=0.2, cfg=config(lr=2.5, momentum=0.0), nu=(0.0, 0.1)),
    "eigen_small":         dict(regime="eigen_dominated", dims=(11, 3, 16, 16), T=8, N=64, gain=1.0, value_head_gain=4.0,
                                cfg=config(damping=1e-5, kl_clip=1e3)),
    "eigen_northstar":     dict(regime="eigen_dominated", dims=(47, 12, 64, 64), T=40, N=128, gain=1.0, value_head_gain=10.0,
                                cfg=config(damping=1e-5, kl_clip=0.1, momentum=0.0)),
    "eigen_h98":           dict(_EIG, dims=(64, 3, 98, 98), cfg=config(damping=1e-5, kl_clip=1e3)),
    "eigen_h99":           dict(_EIG, dims=(64, 3, 99, 99), cfg=config(damping=1e-5, kl_clip=1.0, momentum=0.0)),
    "eigen_h128":          dict(_EIG, dims=(64, 3, 128, 128), cfg=config(damping=1e-5, kl_clip=1e3)),
    "eigen_h129":          dict(_EIG, dims=(64, 3, 129, 129), cfg=config(damping=1e-5, kl_clip=1.0, momentum=0.0)),
    "eigen_global_weights": dict(regime="eigen_dominated", dims=(150, 8, 256, 256), T=8, N=128, gain=1.3, value_head_gain=20.0,
                                 cfg=config(damping=1e-5, kl_clip=1.0, momentum=0.0)),
    "damping_chunk":       dict(regime="damping_dominated", dims=(47, 12, 64, 64), T=1, N=4099, gain=0.2,
                                cfg=config(damping=1e6, lr=2.5e6, kl_clip=BIG_KL, momentum=0.0)),
    "damping_global_weights": dict(regime="damping_dominated", dims=(150, 8, 256, 256), T=5, N=13, gain=0.2,
                                   cfg=config(damping=1e6, lr=2.5e6, kl_clip=BIG_KL)),
    "refresh_small":       dict(regime="refresh", dims=(11, 3, 16, 16), T=8, N=64, gain=1.0, value_head_gain=4.0,
                                cfg=config(damping=1e-4, momentum=0.0, Tf=2, stat_decay=0.5, kl_clip=0.01), updates=4),
    "refresh_h129":        dict(regime="refresh", dims=(64, 3, 129, 129), T=8, N=64, gain=1.4, value_head_gain=10.0,
                                cfg=config(damping=1e-4, momentum=0.0, Tf=2, stat_decay=0.5, kl_clip=0.1), updates=4),
}
# name -> seed; every other case: 0 (`python tests/acktr_regimes.py` searches again)
SEEDS = {"eigen_h99": 1, "eigen_h128": 1, "eigen_h129": 1,    # seed 0: an eigenvalue of G.critic.2 within [1e-7, 1e-5]
         "eigen_global_weights": 6,                            # seeds 0 .. 5: the same
         "refresh_h129": 1,
         "threshold": 2}                                       # seeds 0, 1: an eigenvalue of G.actor.2 within 3x of 1e-6
# NOT among the cases the GPU file runs.  threshold: three observation columns x 3e-3 and three x 3e-4 put A.obs's eigenvalues at
# 1, 9e-6 and 9e-8; log-stds of 5.5 and 8 put G.dist.fc_mean's at 8.7, 1.7e-5 and 1.1e-7; every other factor stays a factor of 3
# away from 1e-6, and at damping 1e-6 keeping the sub-threshold eigenvalues would move v by 3 .. 5 %.  But the float32
# evaluation is then 1.6e-4 .. 1.1e-3 from float64 (seeds 2, 4, 6, 7, 12, 13, 14 of 16; the other seeds miss the factor of 3), and
# 6e-4 .. 1.2e-3 at damping 1e-8: dividing by d_g d_a + damping at the scale of float32's own eigenvalue error is ill-conditioned,
# so the whole-update case is dropped, not given a wider bound (tests/test_acktr_regimes_host.py asserts both halves).  Its two
# straddling factors still go through the eigensolver alone on the GPU, where the claim -- which eigenvalues are zeroed -- is
# well-conditioned.
DROPPED = {
    "threshold": dict(regime="threshold", dims=(11, 3, 16, 16), T=8, N=64, gain=1.0, value_head_gain=4.0, on_policy=0.5,
                      obs_scale=[1.0] * 5 + [3e-3] * 3 + [3e-4] * 3, logstd=[-0.5, 5.5, 8.0], straddle=["A.obs", "G.dist.fc_mean"],
                      cfg=config(damping=1e-6, kl_clip=1e3, momentum=0.0)),
}


def describe(c):
    """the float64 description of every update -> list of Case(nu, vg, v, g, step, dp, losses, factors, eig, refreshed, ...) and,
    under "o32", the float32 evaluation's distances (the largest over the evaluation and JITTERS more with inputs moved by an
    ulp) with "nu32", its nu's largest relative error"""
    out, st = [], new_state()
    for u in c.updates:
        p1, losses, st, info = update(u["params"], st, u["obs"], u["actions"], u["returns"], u["eps"], c.dims, VCOEF, ECOEF, c.cfg)
        info["dp"], info["losses"], info["factors"], info["p1"] = p1 - u["params"].astype(np.float64), losses, state_factors(info), p1
        out.append(info)
    for k in range(JITTERS + 1):
        jr = np.random.default_rng([c.seed, k, 83])
        jit = (lambda a: a) if k == 0 else (lambda a: (a * (1.0 + jr.uniform(-1.0, 1.0, a.shape) * 2.0 ** -24)).astype(np.float32))
        st = new_state()
        for u, ref in zip(c.updates, out):
            par = jit(u["params"])
            p1, _, st, info = update(par, st, jit(u["obs"]), jit(u["actions"]), jit(u["returns"]), jit(u["eps"]), c.dims, VCOEF, ECOEF, c.cfg,
                                     np.float32)
            m = measures(par, p1, info["step"], state_factors(info), ref, c.dims)
            if k == 0:
                ref["o32"], ref["nu32"] = m, 0.0
            else:
                for what, d in m.items():
                    for name, x in d.items():
                        ref["o32"][what][name] = max(ref["o32"][what][name], x)
            ref["nu32"] = max(ref["nu32"], abs(info["nu"] / ref["nu"] - 1.0))
    return out


def pair_products(info, c):
    """{weight block: d_g d_a over its pairs} with the eigenvalues the update used (after the threshold)"""
    out = {}
    for name, (key, fa, fg) in zip(BLOCKS, MODULES):
        if fa is not None:
            out[name] = np.outer(np.asarray(info["eG"][fg][0], np.float64), np.asarray(info["eA"][fa][0], np.float64))
    return out


def band(info, lo=1e-7, hi=1e-5):
    """{factor: eigenvalues in [lo, hi]} as of the last refresh"""
    return {name: d[(d >= lo) & (d <= hi)] for name, d in zip(FACTORS, info["eig"]) if ((d >= lo) & (d <= hi)).any()}


def _check(c):
    _check_regime(c)
    _check_conditioning(c)


def _check_conditioning(c):
    """a case judges something only where the float32 evaluation itself is within COND of float64"""
    for j, d in enumerate(c.desc):
        w = worst(d["o32"])
        assert w <= COND, f"{c.tag}, update {j}: the float32 evaluation is {w:.2e} from float64: " \
                          f"{({k: max(x, key=x.get) + f' {max(x.values()):.1e}' for k, x in d['o32'].items()})}"


def _check_regime(c):
    cfg, regime = c.cfg, c.regime
    for j, d in enumerate(c.desc):
        tag = f"{c.tag}, update {j}"
        assert np.isfinite(d["step"]).all() and np.isfinite(d["losses"]).all() and d["vg"] > 0, tag
        if regime in ("unclipped", "damping_dominated"):
            assert d["vg"] <= 0.8 * cfg["kl_clip"] and d["nu"] == 1.0, f"{tag}: v g lr^2 = {d['vg']:.3e} against kl_clip {cfg['kl_clip']:.3e}"
        if regime == "clipped":
            lo, hi = c.nu
            assert lo < d["nu"] < hi, f"{tag}: nu = {d['nu']:.4f} outside ({lo}, {hi})"
        if regime == "eigen_dominated":
            med = {k: float(np.median(x)) for k, x in pair_products(d, c).items()}
            assert min(med.values()) >= 10.0 * cfg["damping"], f"{tag}: median d_g d_a / damping {({k: x / cfg['damping'] for k, x in med.items()})}"
        if regime in ("eigen_dominated", "refresh"):
            b = band(d)
            assert not b, f"{tag}: eigenvalues within a decade of the threshold: {b}"
        if regime == "damping_dominated":
            x = block_distances(d["v"] * cfg["damping"], d["g"], c.dims, atol=0.0)
            assert max(x.values()) <= 1e-3, f"{tag}: v damping is {max(x.values()):.2e} from the gradient"
        if regime == "threshold":
            for name in c.straddle:
                e = d["eig"][FACTORS.index(name)]
                assert (e >= 3.0 * EIG_THRESHOLD).any() and (e <= EIG_THRESHOLD / 3.0).any(), (tag, name, e)
            for name, e in zip(FACTORS, d["eig"]):
                near = e[(e > EIG_THRESHOLD / 3.0) & (e < 3.0 * EIG_THRESHOLD)]
                assert not near.size, f"{tag}: {name} has eigenvalues within 3x of the threshold: {near}"
            # the zeroing shows: with the sub-threshold eigenvalues kept, v would be another vector
            assert c.zeroing_shows(d) >= ZEROING_SHOWS, f"{tag}: keeping the eigenvalues below the threshold moves v by {c.zeroing_shows(d):.2e} only"
        if regime == "refresh":
            assert cfg["Tf"] == 2 and cfg["momentum"] == 0.0 and len(c.updates) == 4
            assert d["refreshed"] == (j % 2 == 0)


def build(name, seed=None, check=True, **over):
    spec = dict(SPECS.get(name) or DROPPED[name], **over)
    seed = SEEDS.get(name, 0) if seed is None else seed
    dims, T, N = spec["dims"], spec["T"], spec["N"]
    rng = np.random.default_rng([seed] + list(dims) + [T, N])
    c = Case(name=name, regime=spec["regime"], dims=dims, T=T, N=N, cfg=spec["cfg"], seed=seed, nu=spec.get("nu"),
             tag=f"{name} {dims[0]}x{dims[1]}x{dims[2]}" + (f" (critic {dims[3]})" if dims[3] != dims[2] else "") + f" B {T}x{N} seed {seed}")
    params = draw_params(rng, dims, spec["gain"], spec.get("zero_bias", False), spec.get("value_head_gain", 1.0), spec.get("logstd"))
    c["updates"], st = [], new_state()
    for j in range(spec.get("updates", 1)):     # changing rollouts; the next update starts from this one's float64 result, rounded
        u = draw_rollout(rng, params, dims, T, N, spec.get("on_policy"), spec.get("obs_scale"))
        u["params"] = params
        c["updates"].append(u)
        if j + 1 < spec.get("updates", 1):
            p1, _, st, _ = update(params, st, u["obs"], u["actions"], u["returns"], u["eps"], dims, VCOEF, ECOEF, c.cfg)
            params = p1.astype(np.float32)
    if spec["regime"] == "threshold":
        c["straddle"] = spec["straddle"]
        c["zeroing_shows"] = lambda d: _zeroing_shows(c, d)
    c["desc"] = describe(c)
    if check:
        _check(c)
    return c


def _zeroing_shows(c, d):
    """rel-L2 between v and the v the same eigenbases give with every eigenvalue kept (no 1e-6 threshold)"""
    u = c.updates[0]
    sl, n = policy_slices(*c.dims)
    v = np.zeros(n)
    k = 0
    raw_a, raw_g = d["eig"][:5], d["eig"][5:]
    for key, fa, fg in MODULES:
        s, shape = sl[key]
        grad = d["g"][s].reshape(shape[0], -1) if len(shape) == 2 else d["g"][s].reshape(-1, 1)
        da, qa = (np.ones(1), np.ones((1, 1))) if fa is None else (raw_a[fa], d["eA"][fa][1])
        dg, qg = raw_g[fg], d["eG"][fg][1]
        v[s] = (qg @ ((qg.T @ grad @ qa) / (dg[:, None] * da[None, :] + c.cfg["damping"])) @ qa.T).reshape(-1)
        k += 1
    return whole_vector_distance(v, d["v"])


@functools.lru_cache(maxsize=None)
def case(name):
    """build() at the committed seed, computed once per process and shared (callers must not write into it)"""
    return build(name)


def all_cases():
    return list(SPECS)


def big_kl(cfg):
    """the same config with a kl_clip no step reaches: the run that gives v itself, for nu = <buffer, v> / <v, v>"""
    return dict(cfg, kl_clip=f32(BIG_KL))


def summary(c):
    out = []
    for j, d in enumerate(c.desc):
        med = {k: float(np.median(x)) / c.cfg["damping"] for k, x in pair_products(d, c).items()}
        out.append(f"{c.tag} update {j}: nu {d['nu']:.4f}, v g lr^2 {d['vg']:.3e} (kl_clip {c.cfg['kl_clip']:.3g}), median d_g d_a / damping "
                   f"{min(med.values()):.3g} .. {max(med.values()):.3g}, threshold band {({k: x.size for k, x in band(d).items()})}, "
                   f"float32 worst {worst(d['o32']):.2e}, nu32 {d['nu32']:.1e}")
    return "\n".join(out)


if __name__ == "__main__":   # the seed search: prints what SEEDS needs
    import sys
    for name in (sys.argv[1:] or all_cases()):
        last = None
        for seed in range(40):
            try:
                c = build(name, seed=seed)
            except AssertionError as exc:
                last = str(exc)[:600]
                continue
            print(f"    {name!r}: {seed},", flush=True)
            print(summary(c), flush=True)
            break
        else:
            print("# NO SEED for", name, last, flush=True)
