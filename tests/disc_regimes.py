"""Case builders for the discriminator's numerical regimes (tests/test_disc_regimes_host.py on the CPU,
tests/test_gpu_disc_regimes.py on the GPU).  The rest of the suite runs the discriminator step at nn.Linear's default
initialisation, where every row's input-gradient norm |g| is 0.1 .. 0.2, so the penalty coefficient
c_r = 2 lambda / B (|g| - 1) / |g| is negative on every row and every logit lies within +-0.5, and it looks at the step
through post-Adam weights only, which hardly see a gradient that is wrong by a factor.  Here:

  init        the default initialisation: every row |g| < 0.5 (the baseline);
  both_sides  weights x ~2.5, rows x 1.5: rows on both sides of |g| = 1, logits of both signs among expert and policy rows;
  saturated   weights x 6, rows x 3: tanh units saturate, logits reach +-6 and beyond, |g| far above 1.

Nothing here touches the library.  A case is described in float64 by the arbiter (oracle/oracle64.py: the gradient and the
three loss sums) and by a short numpy float64 forward (per-row logits, sigmoid, |g|) that is checked against the arbiter;
the builder ASSERTS on that description that the case reaches what it claims.  A case that misses a condition gets the
next seed from SEEDS, never an exclusion.

Parameter blocks in Discriminator.param_shapes() order: 0.weight, 0.bias, 2.weight, 2.bias, 4.weight, 4.bias."""
import functools

import numpy as np

from helpers import ATOL, RTOL

LAMBDA = 10.0
B = 128               # rows of a regime case: eight 16-row groups, thirty-two 4-row groups
MIN_ROWS = 8          # rows every class of a 128-row case must hold (ragged cases: 1)
JITTERS = 3           # jittered float32 evaluations behind every case's float32 distance
REGIMES = ("init", "both_sides", "saturated")

# (F, Hd): every kernel instance the launcher can choose -- <1,1>, <2,7>, <6,7>, the run-time-shape 16-row kernel <0,0>,
# and a discriminator beyond a CU's LDS (the global-weight instances)
SHAPES = [(7, 16), (25, 100), (86, 100), (40, 64), (150, 256)]
THIN_SHAPES = [(7, 16), (25, 100), (86, 100)]          # the shapes the 4-row kernels exist for
RAGGED_SHAPES = [(7, 16), (86, 100)]
RAGGED_B = [1, 13, 130]
EPOCH_SHAPES = [(7, 16), (25, 100), (86, 100)]
EPOCH_B, EPOCH_STEPS = 32, 6
REWARD_SHAPES = [(7, 16), (25, 100), (86, 100)]
REWARD_SEEDS = [0, 1, 2, 3]
REWARD_SCALES = [(4.0, 3.0), (8.0, 4.0)]               # |reward| up to about 6, and up to about 13

SCALES = {"init": (1.0, 1.0), "both_sides": (2.5, 1.5), "saturated": (6.0, 3.0)}   # (scale_w, scale_x)
# both_sides: scale_w tuned per shape within [2, 3] so that rows fall on both sides of |g| = 1 (default 2.5)
BOTH_SIDES_SCALE_W = {(150, 256): 2.2, (40, 64): 2.5}
# (regime, F, Hd, B) -> seed; every other case: 0 (`python tests/disc_regimes.py` searches again)
SEEDS = {("both_sides", 150, 256, 128): 5,     # seeds 0 .. 4: fewer than 8 rows with |g| > 1.1 at scale_w 2.2
         ("saturated", 25, 100, 128): 1}      # seed 0: a row with |g| < 1


class Case(dict):
    __getattr__ = dict.__getitem__


def param_shapes(F, Hd):
    return [("0.weight", (Hd, F)), ("0.bias", (Hd,)), ("2.weight", (Hd, Hd)), ("2.bias", (Hd,)), ("4.weight", (1, Hd)), ("4.bias", (1,))]


def num_params(F, Hd):
    return sum(int(np.prod(s)) for _, s in param_shapes(F, Hd))


def blocks(F, Hd, flat):
    out, off = [], 0
    for name, shape in param_shapes(F, Hd):
        n = int(np.prod(shape))
        out.append((name, flat[off:off + n]))
        off += n
    assert off == flat.size, (off, flat.size)
    return out


def block_slice(F, Hd, name):
    off = 0
    for k, shape in param_shapes(F, Hd):
        n = int(np.prod(shape))
        if k == name:
            return slice(off, off + n)
        off += n
    raise KeyError(name)


def block_distances(got, ref, F, Hd, atol=ATOL):
    """regimes.block_distances' formula: {block: ||got - ref||_2 / (||ref||_2 + atol * max|ref| * sqrt(n))}, the floor on the
    scale of the whole gradient's largest element."""
    out = {}
    ref = np.asarray(ref, np.float64)
    scale = atol * np.max(np.abs(ref))
    for (name, g), (_, r) in zip(blocks(F, Hd, np.asarray(got, np.float64)), blocks(F, Hd, ref)):
        out[name] = float(np.sqrt(((g - r) ** 2).sum()) / (np.sqrt((r ** 2).sum()) + scale * np.sqrt(r.size) + 1e-300))
    return out


def init_params(rng, F, Hd, scale_w):
    """nn.Linear's default: U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for weight and bias; every weight MATRIX x scale_w"""
    parts = []
    for name, shape in param_shapes(F, Hd):
        fan_in = shape[1] if len(shape) == 2 else (F if name == "0.bias" else Hd)
        b = 1.0 / np.sqrt(fan_in)
        w = rng.uniform(-b, b, size=int(np.prod(shape)))
        parts.append(w * scale_w if name.endswith("weight") else w)
    return np.concatenate(parts).astype(np.float32)


def _unpack(params, F, Hd):
    p = np.asarray(params, np.float64)
    b = dict(blocks(F, Hd, p))
    return b["0.weight"].reshape(Hd, F), b["0.bias"], b["2.weight"].reshape(Hd, Hd), b["2.bias"], b["4.weight"], b["4.bias"][0]


def logits64(params, F, Hd, x):
    """numpy float64: D(x) for rows x [n, F]"""
    W1, b1, W2, b2, w3, b3 = _unpack(params, F, Hd)
    h1 = np.tanh(np.asarray(x, np.float64) @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    return h2 @ w3 + b3


def gnorm64(params, F, Hd, expert, policy, alpha):
    """numpy float64: |dD/dx| at the mixed rows alpha e + (1 - alpha) p"""
    W1, b1, W2, b2, w3, _ = _unpack(params, F, Hd)
    al = np.asarray(alpha, np.float64)[:, None]
    xm = al * np.asarray(expert, np.float64) + (1.0 - al) * np.asarray(policy, np.float64)
    h1 = np.tanh(xm @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    d1 = ((w3 * (1.0 - h2 * h2)) @ W2) * (1.0 - h1 * h1)
    return np.sqrt(((d1 @ W1) ** 2).sum(-1))


def sigmoid64(d):
    return 1.0 / (1.0 + np.exp(-np.asarray(d, np.float64)))


EPS_R = float(np.float32(1e-7))     # the reward's 1e-7f keeps its float32 value in the arbiter


def reward64(d):
    """log(s + 1e-7) - log(1 - s + 1e-7) of logits d, float64 -> (reward, s)"""
    s = sigmoid64(d)
    return np.log(s + EPS_R) - np.log(1.0 - s + EPS_R), s


def log_sigmoid64(x):
    return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


def grad(c, bits=64, params=None, expert=None, policy=None):
    """the one-step gradient of the case's minibatch -> (flat gradient, losses (total, expert, policy)): the arbiter
    (bits = 64) or the float32 oracle"""
    if bits == 64:
        from oracle import oracle64 as orc
    else:
        from oracle import oracle as orc
    nb = c.expert.shape[0]
    G, sums = orc.disc_grad_rows(c.F, c.Hd, c.params if params is None else params, c.expert if expert is None else expert,
                                 c.policy if policy is None else policy, c.alpha, 1.0 / nb, LAMBDA)
    el, pl, gp = sums[0] / nb, sums[1] / nb, LAMBDA * sums[2] / nb
    return np.asarray(G, np.float64), np.array([el + pl + gp, el, pl]), sums


def describe(c):
    F, Hd, nb = c.F, c.Hd, c.expert.shape[0]
    d = Case()
    d["logit_e"], d["logit_p"] = logits64(c.params, F, Hd, c.expert), logits64(c.params, F, Hd, c.policy)
    d["gnorm"] = gnorm64(c.params, F, Hd, c.expert, c.policy, c.alpha)
    g64, l64, sums = grad(c, 64)
    d["grad"], d["losses"] = g64, l64
    # the numpy forward against the arbiter itself: the three sums are functions of exactly the per-row quantities above
    want = np.array([(-log_sigmoid64(d["logit_e"])).sum(), (d["logit_p"] - log_sigmoid64(d["logit_p"])).sum(), ((d["gnorm"] - 1.0) ** 2).sum()])
    assert np.allclose(sums, want, rtol=1e-11, atol=1e-13), (c.tag, sums, want)
    g = d["gnorm"]
    d["classes"] = {"|g|<0.9": int((g < 0.9).sum()), "|g|>1.1": int((g > 1.1).sum()), "|g|<1": int((g < 1.0).sum()), "|g|>1": int((g > 1.0).sum()),
                    "expert+": int((d["logit_e"] > 0).sum()), "expert-": int((d["logit_e"] < 0).sum()),
                    "policy+": int((d["logit_p"] > 0).sum()), "policy-": int((d["logit_p"] < 0).sum())}
    # the float32 evaluation's distance: the largest over the evaluation itself and JITTERS more with inputs moved by an ulp
    o32 = block_distances(grad(c, 32)[0], g64, F, Hd)
    for k in range(JITTERS):
        jr = np.random.default_rng([c.seed, k, 79])
        jit = lambda a: (a * (1.0 + jr.uniform(-1.0, 1.0, a.shape) * 2.0 ** -24)).astype(np.float32)  # noqa: E731
        for name, x in block_distances(grad(c, 32, jit(c.params), jit(c.expert), jit(c.policy))[0], g64, F, Hd).items():
            o32[name] = max(o32[name], x)
    d["o32"] = o32
    return d


def _check(c):
    d, cl = c.desc, c.desc["classes"]
    g, nb = d["gnorm"], c.expert.shape[0]
    assert np.isfinite(d["grad"]).all() and np.isfinite(d["losses"]).all(), c.tag
    need = MIN_ROWS if nb >= B else 1
    if c.regime == "init":
        assert g.max() < 0.5, f"{c.tag}: a row with |g| = {g.max():.3f}"
    elif c.regime == "both_sides":
        assert 2.0 <= c.scale_w <= 3.0, c.tag
        assert g.min() >= 1e-3, f"{c.tag}: a row with |g| = {g.min():.2e}"
        if nb > 1:      # one row has none of the class conditions
            short = {k: cl[k] for k in ("|g|<0.9", "|g|>1.1", "expert+", "expert-", "policy+", "policy-") if cl[k] < need}
            assert not short, f"{c.tag}: classes with fewer than {need} rows: {short} (all: {cl})"
    else:
        if c.Hd == 100:
            assert g.min() > 1.0, f"{c.tag}: a row with |g| = {g.min():.3f}"
        assert np.abs(d["logit_e"]).max() >= 6.0 and np.abs(d["logit_p"]).max() >= 6.0, \
            f"{c.tag}: max |logit| {np.abs(d['logit_e']).max():.2f} (expert) / {np.abs(d['logit_p']).max():.2f} (policy)"
    # a case judges something only where float32 evaluations themselves hold the contract with room for F >= 2
    assert max(d["o32"].values()) <= 0.5 * RTOL, f"{c.tag}: float32 evaluations are up to {max(d['o32'].values()):.2e} from float64"


def draw_rows(rng, n, F, scale_x):
    """expert rows scale_x (0.7 N(0,1) + 0.2), policy rows scale_x N(0,1), alpha ~ U(0,1): float32"""
    expert = (scale_x * (0.7 * rng.standard_normal((n, F)) + 0.2)).astype(np.float32)
    policy = (scale_x * rng.standard_normal((n, F))).astype(np.float32)
    return expert, policy, rng.random(n).astype(np.float32)


def build(regime, F, Hd, nb=B, seed=None, scale_w=None, scale_x=None, check=True):
    assert regime in REGIMES
    sw, sx = SCALES[regime]
    if regime == "both_sides":
        sw = BOTH_SIDES_SCALE_W.get((F, Hd), sw)
    sw, sx = (sw if scale_w is None else scale_w), (sx if scale_x is None else scale_x)
    seed = SEEDS.get((regime, F, Hd, nb), 0) if seed is None else seed
    rng = np.random.default_rng([seed, F, Hd, nb])
    c = Case(regime=regime, F=F, Hd=Hd, seed=seed, scale_w=sw, scale_x=sx, tag=f"{regime}({sw:g}, {sx:g}) {F}x{Hd} B {nb} seed {seed}")
    c["params"] = init_params(rng, F, Hd, sw)
    c["expert"], c["policy"], c["alpha"] = draw_rows(rng, nb, F, sx)
    c["desc"] = describe(c)
    if check:
        _check(c)
    return c


@functools.lru_cache(maxsize=None)
def case(regime, F, Hd, nb=B):
    """build() at the committed seed, computed once per process and shared (callers must not write into it)"""
    return build(regime, F, Hd, nb)


def all_cases():
    """every (regime, F, Hd, B) whose one-step gradient the GPU file looks at"""
    out = [(r, F, Hd, B) for r in REGIMES for F, Hd in SHAPES]
    out += [("both_sides", F, Hd, nb) for F, Hd in RAGGED_SHAPES for nb in RAGGED_B]
    return out


@functools.lru_cache(maxsize=None)
def zero_head_case(F=86, Hd=100):
    """a both_sides case with 4.weight = 0: every row's input gradient is exactly 0 (the `nn > 0` guard), every logit is 4.bias"""
    base = case("both_sides", F, Hd)
    c = Case(base)
    p = base.params.copy()
    p[block_slice(F, Hd, "4.weight")] = 0.0
    c["params"], c["tag"] = p, base.tag + ", 4.weight = 0"
    c["desc"] = describe(c)
    return c


# ------------------------------------------------------------------------------------------- moments over real epochs
@functools.lru_cache(maxsize=None)
def epoch_case(F, Hd):
    """EPOCH_STEPS * EPOCH_B rows of the both_sides recipe in one draw, and the (expert_perm, policy_perm, alpha) of two epochs"""
    n = EPOCH_STEPS * EPOCH_B
    c = build("both_sides", F, Hd, nb=n)
    rng = np.random.default_rng([5, F, Hd])
    c["draws"] = [(rng.permutation(n).astype(np.int64), rng.permutation(n).astype(np.int64), rng.random(n).astype(np.float32)) for _ in range(2)]
    return c


def disc_update64(c, draws, batch, adam=None, expert=None, policy=None, lr=1e-3, eps=1e-8):
    """oracle64.disc_update over the epochs `draws` from the case's weights -> dict(params, m, v, steps, losses per epoch).
    The policy rows sit in obs_feat[1:] of a one-step rollout."""
    from oracle import oracle64 as o64
    expert = c.expert if expert is None else expert
    policy = c.policy if policy is None else policy
    n, F = policy.shape
    feat = np.concatenate([np.zeros((1, n, F)), policy[None].astype(np.float64)])
    p = c.params.astype(np.float64)
    st = o64.AdamState(p.size)
    if adam is not None:
        st.m[:], st.v[:], st.t.value = np.asarray(adam[0], np.float64), np.asarray(adam[1], np.float64), int(adam[2])
    losses = []
    for ep, pp, al in draws:
        l, n_d = o64.disc_update(F, c.Hd, p, st, expert, feat, batch, ep, pp, al, lr, eps)
        losses.append(l)
    return dict(params=p, m=st.m, v=st.v, steps=st.t.value, losses=losses, n_d=n_d)


# ------------------------------------------------------------------------------------------- rewards
@functools.lru_cache(maxsize=None)
def reward_case(F, Hd, scale_w, scale_x, seed, n=B):
    """weights x scale_w, rows scale_x N(0,1): two calls' rows, masks (the second call's mix 0 and 1) and float64 logits"""
    rng = np.random.default_rng([seed, F, Hd, 31])
    c = Case(F=F, Hd=Hd, seed=seed, scale_w=scale_w, scale_x=scale_x, gamma=0.99, tag=f"reward({scale_w:g}, {scale_x:g}) {F}x{Hd} seed {seed}")
    c["params"] = init_params(rng, F, Hd, scale_w)
    c["x"] = [(scale_x * rng.standard_normal((n, F))).astype(np.float32) for _ in range(2)]
    c["masks"] = [np.ones(n, np.float32), (rng.random(n) > 0.4).astype(np.float32)]
    c["offset"] = [0.0, -0.3]
    c["logits"] = [logits64(c.params, F, Hd, x) for x in c.x]
    return c


def reward_envelope(s64):
    """the conditioning of log(s + 1e-7) - log(1 - s + 1e-7) in s: one float32 ulp of s (2^-24 below 1) moves the reward by this"""
    return 2.0 ** -24 * (1.0 / (1.0 - s64 + EPS_R) + 1.0 / (s64 + EPS_R))


def reward_excess(got, r64, s64):
    """per element, (|got - r64| - (RTOL |r64| + ATOL)) in units of reward_envelope(s64): the multiple C has to cover"""
    return (np.abs(np.asarray(got, np.float64) - r64) - (RTOL * np.abs(r64) + ATOL)) / reward_envelope(s64)


def rewards64(c):
    """the two calls through the arbiter -> [(reward, returns, s)], and the numpy forward checked against it"""
    from oracle import oracle64 as o64
    out, ret = [], None
    for k in range(2):
        rew, ret = o64.disc_predict_reward(c.F, c.Hd, c.params, c.x[k], c.gamma, c.masks[k], c.offset[k], ret)
        r, s = reward64(c.logits[k])
        # (1 - s is a difference of nearly equal float64 numbers in both: an ulp of exp() is 1e-9 of the reward at 1 - s ~ 1e-7)
        assert np.allclose(rew[:, 0], r + c.offset[k], rtol=1e-7, atol=1e-9), (c.tag, float(np.abs(rew[:, 0] - r - c.offset[k]).max()))
        out.append((rew[:, 0].copy(), ret[:, 0].copy(), s))
    return out


@functools.lru_cache(maxsize=None)
def relabel_case(F, Hd, T=6, N=16, scale_w=4.0, scale_x=3.0, seed=0):
    """two relabel calls' rollouts: masks with a done at t = 0, a done at T - 1 and one column done throughout"""
    rng = np.random.default_rng([seed, F, Hd, 37])
    c = Case(F=F, Hd=Hd, T=T, N=N, gamma=0.99, tag=f"relabel({scale_w:g}, {scale_x:g}) {F}x{Hd}")
    c["params"] = init_params(rng, F, Hd, scale_w)
    c["obs_feat"] = [(scale_x * rng.standard_normal((T + 1, N, F))).astype(np.float32) for _ in range(2)]
    masks = []
    for _ in range(2):
        m = (rng.random((T + 1, N)) > 0.1).astype(np.float32)
        m[0, 1], m[T - 1, 2], m[:, 3] = 0.0, 0.0, 0.0
        m[1:T - 1, 1], m[:T - 1, 2] = 1.0, 1.0
        masks.append(m)
    c["masks"], c["offset"] = masks, [0.0, -0.2]
    return c


if __name__ == "__main__":   # the seed search: prints what SEEDS needs
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    specs = all_cases() + [("both_sides", F, Hd, EPOCH_STEPS * EPOCH_B) for F, Hd in EPOCH_SHAPES]
    for regime, F, Hd, nb in specs:
        for seed in range(200):
            try:
                c = build(regime, F, Hd, nb, seed=seed)
            except AssertionError as exc:
                last = str(exc)[:200]
                continue
            d = c.desc
            print(f"    {(regime, F, Hd, nb)}: {seed},   # |g| {d['gnorm'].min():.3g} .. {d['gnorm'].max():.3g}, logits {min(d['logit_e'].min(), d['logit_p'].min()):.2f} .. "
                  f"{max(d['logit_e'].max(), d['logit_p'].max()):.2f}, o32 {max(d['o32'].values()):.1e}, {d['classes']}", flush=True)
            break
        else:
            print("# NO SEED for", (regime, F, Hd, nb), last, flush=True)
