"""CPU: the case builders of tests/disc_regimes.py judged on the references alone (oracle/oracle64.py and a numpy float64
forward checked against it), the constants tests/test_gpu_disc_regimes.py holds the HIP path to (FLOOR, C), and the reason
that file exists, restated as a test: a discriminator gradient that is wrong by a factor -- the whole of it, or one block --
leaves the post-Adam weights inside the comparison every other discriminator test makes, and is flagged by the per-block
distance of the one-step gradient."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import disc_regimes as dr  # noqa: E402
from helpers import ATOL, RTOL, assert_close, assert_close_adam  # noqa: E402

IDS = [f"{r}-{F}x{Hd}-B{nb}" for r, F, Hd, nb in dr.all_cases()]


@pytest.mark.parametrize("spec", dr.all_cases(), ids=IDS)
def test_case_reaches_what_it_claims(spec):
    regime, F, Hd, nb = spec
    c = dr.case(*spec)          # the builder asserts the regime's conditions (disc_regimes._check)
    d, cl = c.desc, c.desc["classes"]
    g = d["gnorm"]
    print(c.tag, cl, f"|g| {g.min():.3g} .. {g.max():.3g}", f"logits {min(d['logit_e'].min(), d['logit_p'].min()):.2f} .. "
          f"{max(d['logit_e'].max(), d['logit_p'].max()):.2f}", f"losses {d['losses']}", f"float32 distance {max(d['o32'].values()):.2e}")
    assert c.params.dtype == c.expert.dtype == c.policy.dtype == c.alpha.dtype == np.float32
    assert c.expert.shape == c.policy.shape == (nb, F) and c.alpha.shape == (nb,) and c.params.size == dr.num_params(F, Hd)
    assert cl["|g|<1"] + cl["|g|>1"] == nb and cl["expert+"] + cl["expert-"] == nb and cl["policy+"] + cl["policy-"] == nb
    if regime == "init":        # the regime of the rest of the suite: c_r < 0 on every row, logits within +-1
        assert cl["|g|>1"] == 0 and g.max() < 0.5 and max(np.abs(d["logit_e"]).max(), np.abs(d["logit_p"]).max()) < 1.0
    elif regime == "both_sides" and nb >= dr.B:
        assert min(cl["|g|<0.9"], cl["|g|>1.1"], cl["expert+"], cl["expert-"], cl["policy+"], cl["policy-"]) >= dr.MIN_ROWS
    elif regime == "both_sides" and nb > 1:
        assert min(cl["|g|<1"], cl["|g|>1"]) >= 1
    elif regime == "saturated":
        assert min(np.abs(d["logit_e"]).max(), np.abs(d["logit_p"]).max()) >= 6.0 and (Hd != 100 or g.min() > 1.0)
        assert d["losses"][0] > 5.0       # the penalty dominates: far from the init regime
    # the penalty's own share of the loss, from the per-row norms
    assert_close(d["losses"][0] - d["losses"][1] - d["losses"][2], dr.LAMBDA * ((g - 1.0) ** 2).mean(), rtol=1e-9, atol=1e-12, what="penalty")
    assert max(d["o32"].values()) <= 0.5 * RTOL


@pytest.mark.parametrize("F,Hd", dr.EPOCH_SHAPES)
def test_epoch_cases_hold_both_sides_in_every_minibatch(F, Hd):
    """tests/test_gpu_disc_regimes.py, moments over real epochs: the 192 rows are one both_sides draw, and each of the twelve
    32-row minibatches of the two epochs has mixed rows on both sides of |g| = 1 at the starting weights."""
    c = dr.epoch_case(F, Hd)
    assert c.desc["gnorm"].min() >= 1e-3
    for ep, pp, al in c.draws:
        for k in range(dr.EPOCH_STEPS):
            sl = slice(k * dr.EPOCH_B, (k + 1) * dr.EPOCH_B)
            g = dr.gnorm64(c.params, F, Hd, c.expert[ep[sl]], c.policy[pp[sl]], al[sl])
            assert (g < 1.0).any() and (g > 1.0).any(), (c.tag, k, g.min(), g.max())
    ref = dr.disc_update64(c, c.draws, dr.EPOCH_B)
    assert ref["steps"] == 2 * dr.EPOCH_STEPS and ref["n_d"] == dr.EPOCH_STEPS and np.isfinite(ref["params"]).all()


def test_zero_head_case_has_exactly_zero_gradient_below_the_head():
    """4.weight = 0: every row's input gradient is 0 (the `nn > 0` guard: c_r = 0, the zero subgradient the reference's autograd
    gives), every logit is 4.bias, the penalty is lambda (0 - 1)^2 and only the head's two blocks have a gradient."""
    c = dr.zero_head_case()
    d = c.desc
    b = float(c.params[-1])
    assert not d["gnorm"].any() and np.allclose(d["logit_e"], b, rtol=0, atol=1e-15) and np.allclose(d["logit_p"], b, rtol=0, atol=1e-15)
    for name, g in dr.blocks(c.F, c.Hd, d["grad"]):
        assert g.any() == (name in ("4.weight", "4.bias")), name
    g32 = dr.grad(c, 32)[0]
    for name, g in dr.blocks(c.F, c.Hd, g32):
        assert g.any() == (name in ("4.weight", "4.bias")), f"float32 oracle, {name}"
    sp = lambda x: -dr.log_sigmoid64(np.float64(x))  # noqa: E731  softplus(-x)
    assert_close(d["losses"], [sp(b) + sp(-b) + dr.LAMBDA, sp(b), sp(-b)], rtol=1e-12, atol=0, what="closed-form losses")


def _floor_cases():
    return [dr.case(*spec) for spec in dr.all_cases() if spec[0] in ("init", "both_sides")]


def test_the_arbiter_floor_is_the_float32_distance_of_the_init_and_both_sides_cases():
    """tests/test_gpu_disc_regimes.py's FLOOR: the float32 oracle's largest block distance from float64 over the init and
    both_sides cases (ragged ones included).  The constant may not be below it, nor more than a quarter above it."""
    import test_gpu_disc_regimes as tg
    per = {c.tag: max(c.desc["o32"].values()) for c in _floor_cases()}
    worst = max(per, key=per.get)
    for tag, x in per.items():
        print(f"{tag}: float32 block distance {x:.3e}")
    sat = {c.tag: max(c.desc["o32"].values()) for c in (dr.case(*s) for s in dr.all_cases() if s[0] == "saturated")}
    print(f"FLOOR: re-derived {per[worst]:.3e} ({worst}); constant {tg.FLOOR:.3e}; saturated cases: up to {max(sat.values()):.3e}")
    assert per[worst] <= tg.FLOOR <= 1.25 * per[worst]
    assert tg.F >= 2.0


# ------------------------------------------------------------------------------------------- what post-Adam weights do not see
def _four_adam_steps(c, mutate, lr=1e-3, nb=128):
    """the float32 oracle's own four steps on four 128-row minibatches -> (weights, m after the first step)"""
    from oracle import oracle as orc
    p, st, m1 = c.params.copy(), orc.AdamState(c.params.size), None
    for k in range(4):
        sl = slice(k * nb, (k + 1) * nb)
        G, _ = orc.disc_grad_rows(c.F, c.Hd, p, c.expert[sl], c.policy[sl], c.alpha[sl], 1.0 / nb)
        orc.adam_step(p, np.ascontiguousarray(mutate(G), np.float32), st, lr, 1e-8)
        m1 = st.m.copy() if k == 0 else m1
    return p, m1


MUTATIONS = {"whole gradient x 2 (1/B off by 2)": (lambda sl: (lambda G: G * np.float32(2.0)), None),
             "0.bias block x 3": (lambda sl: (lambda G: np.concatenate([G[:sl.start], G[sl] * np.float32(3.0), G[sl.stop:]])), "0.bias")}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_post_adam_weights_are_blind_to_a_scaled_gradient_and_the_block_distance_is_not(name):
    """Adam's step is lr m / (sqrt(v) + eps), invariant per element under a rescaling of the gradient: with the gradient
    doubled, or one block tripled, the float32 oracle's weights after four steps (F 86, Hd 100, B 128, lr 1e-3) stay inside the
    comparison the discriminator tests make (helpers.assert_close_adam), while m after the first step -- 0.1 g -- is a block
    distance of 1 (x 2) or 2 (x 3) from the float64 gradient."""
    F, Hd, nb = 86, 100, 128
    c = dr.build("init", F, Hd, nb=4 * nb)
    make, block = MUTATIONS[name]
    sl = dr.block_slice(F, Hd, block) if block else slice(0, 0)
    p_true, m_true = _four_adam_steps(c, lambda G: G)
    p_mut, m_mut = _four_adam_steps(c, make(sl))
    assert np.abs(p_true - c.params).max() > 3e-3           # four real steps
    err = np.abs(p_mut.astype(np.float64) - p_true)
    outside = int((err > ATOL + RTOL * np.abs(p_true)).sum())
    print(f"{name}: {outside} of {p_true.size} weights outside (RTOL, ATOL), max abs difference {err.max():.3e}")
    assert_close_adam(p_mut, p_true, lr=1e-3, steps=4, what="the existing comparison")      # blind: does not raise
    first = _first_minibatch(c, nb)
    g64 = dr.grad(first, 64)[0]
    d_true = dr.block_distances(m_true.astype(np.float64) / 0.1, g64, F, Hd)
    d_mut = dr.block_distances(m_mut.astype(np.float64) / 0.1, g64, F, Hd)
    print("block distances of m / 0.1, true gradient:", d_true, "mutated:", d_mut)
    assert max(d_true.values()) <= RTOL
    mutated = [block] if block else list(d_mut)
    for k, x in d_mut.items():
        assert (x >= 0.5) if k in mutated else (x <= RTOL), (k, x)


def _first_minibatch(c, nb):
    """the first minibatch of a 4 nb-row case as a case of its own"""
    first = dr.Case(c)
    first["expert"], first["policy"], first["alpha"] = c.expert[:nb], c.policy[:nb], c.alpha[:nb]
    return first


# ------------------------------------------------------------------------------------------- rewards
REWARD_CASES = [(F, Hd, seed) for F, Hd in dr.REWARD_SHAPES for seed in dr.REWARD_SEEDS]


def _rewards32(c):
    from oracle import oracle as orc
    out, ret = [], None
    for k in range(2):
        rew, ret = orc.disc_predict_reward(c.F, c.Hd, c.params, c.x[k], c.gamma, c.masks[k], c.offset[k], ret)
        out.append((rew[:, 0].astype(np.float64), ret[:, 0].astype(np.float64)))
    return out


def test_reward_envelope_constant_is_derived_from_the_float32_oracle():
    """tests/test_gpu_disc_regimes.py's C.  log(s + 1e-7) - log(1 - s + 1e-7) moves by (1 / (s + 1e-7) + 1 / (1 - s + 1e-7)) ds:
    where a trained discriminator lives (|reward| ~ 13, 1 - s ~ 2e-6) one float32 ulp of s is a relative 1e-3 of the reward, in
    the reference as in any float32 evaluation.  The float32 oracle's own worst excess over (RTOL, ATOL) in units of that
    envelope, over the (8, 4) cases, doubled and not below 2, is C; at (4, 3) the oracle holds the plain contract."""
    import test_gpu_disc_regimes as tg
    worst, top, plain = 0.0, 0.0, 0.0
    for F, Hd, seed in REWARD_CASES:
        c = dr.reward_case(F, Hd, 8.0, 4.0, seed)
        r64, r32 = dr.rewards64(c), _rewards32(c)
        for k in range(2):
            rew64, _, s64 = r64[k]
            ex = float(dr.reward_excess(r32[k][0], rew64, s64).max())
            over = float((np.abs(r32[k][0] - rew64) / (ATOL + RTOL * np.abs(rew64))).max())
            print(f"{c.tag} call {k}: |reward| up to {np.abs(rew64 - c.offset[k]).max():.2f}, float32 oracle {over:.1f} x the plain tolerance, "
                  f"{ex:.3f} envelopes over it")
            worst, top, plain = max(worst, ex), max(top, float(np.abs(rew64 - c.offset[k]).max())), max(plain, over)
    print(f"C: worst multiple {worst:.3f} -> C = {max(2.0, 2.0 * worst):.3f}; constant {tg.C}")
    assert top >= 12.0 and plain > 1.0          # the cases reach the tail, where the plain contract cannot hold in float32
    assert worst > 0.0 and max(2.0, 2.0 * worst) <= tg.C <= 1.1 * max(2.0, 2.0 * worst)
    for F, Hd, seed in REWARD_CASES:            # (4, 3): |reward| up to about 6, the plain contract
        c = dr.reward_case(F, Hd, 4.0, 3.0, seed)
        r64, r32 = dr.rewards64(c), _rewards32(c)
        for k in range(2):
            assert np.abs(r64[k][0]).max() < 11.0
            assert_close(r32[k][0], r64[k][0], what=f"{c.tag}: float32 oracle reward, call {k}")
            assert_close(r32[k][1], r64[k][1], what=f"{c.tag}: float32 oracle returns, call {k}")
    assert max(np.abs(dr.rewards64(dr.reward_case(F, Hd, 4.0, 3.0, s))[0][0]).max() for F, Hd, s in REWARD_CASES) >= 5.0


def test_relabel_case_masks_and_float32_oracle():
    """the relabel case's masks hold a done at t = 0, a done at T - 1 and a column that is done throughout, in both calls, and
    the float32 oracle's relabel holds the plain contract against the arbiter's at scale (4, 3)"""
    from oracle import oracle as o32
    from oracle import oracle64 as o64
    c = dr.relabel_case(86, 100)
    for m in c.masks:
        assert m[0, 1] == 0 and m[1:c.T - 1, 1].all() and m[c.T - 1, 2] == 0 and m[:c.T - 1, 2].all() and not m[:, 3].any()
        assert 0.0 < m[:c.T].mean() < 1.0
    ret = {32: None, 64: None}
    rms = {32: [0.0, 1.0, 1e-4], 64: [0.0, 1.0, 1e-4]}
    for k in range(2):
        out = {}
        for bits, orc in ((32, o32), (64, o64)):
            out[bits], ret[bits], rms[bits] = orc.relabel(c.F, c.Hd, c.params, c.obs_feat[k], c.masks[k], c.gamma, c.offset[k], ret[bits], rms[bits])
        assert_close(out[32], out[64], what=f"rewards, call {k}")
        assert_close(ret[32], ret[64], what=f"returns, call {k}")
        assert np.abs(out[64]).max() < 10.0 and np.abs(out[64]).max() > 0.5      # the clip at +-10 is not what is compared
