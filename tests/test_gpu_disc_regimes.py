"""GPU: the discriminator step's GRADIENT against float64, block by block, off the initialisation regime, and the rewards at a
trained discriminator's logits.  Every other discriminator test compares losses and post-Adam weights, at nn.Linear's default
initialisation (|g| ~ 0.15 on every row, so the penalty coefficient c_r is negative everywhere, logits within +-0.5); Adam's
step is invariant under a rescaling of the gradient, so a gradient wrong by a factor passes them
(tests/test_disc_regimes_host.py shows it on the float32 oracle alone).  Here, on the cases of tests/disc_regimes.py, each
proven on the float64 references alone to reach what it claims:

  C   the one-step gradient (Adam's m / 0.1 and sqrt(v / 0.001) after one step of one epoch) and the three losses, on every kernel
      instance the launcher can choose (k_disc_chain4 / k_disc_step4 <1,1> <2,7> <6,7>, k_disc_chain <..>, <0,0>, the global-weight
      instances), in the regimes init / both_sides / saturated, at ragged batch sizes, with the one-launch step bit-equal to the
      two-launch step, and at the exact edge g = 0;
  D   m, v and weights over two epochs of six steps against the float64 restatement, one step from Adam state far from step 0,
      and the gradient of the global minibatch on every rank of a world of 2 in both data-parallel modes;
  E   predict_reward_combined / predict_prob / relabel_rewards at logits of +-6 (plain contract) and +-13 (conditioning envelope).

Tolerances of the gradient comparisons, per parameter block, distance = ||got - float64||_2 / (||float64||_2 + ATOL max|float64| sqrt(n)):
  * the project's contract: distance <= helpers.RTOL = 1e-4;
  * the arbiter form of tests/test_gpu_regimes.py: distance <= F x (the float32 oracle's distance on the same block) + FLOOR.
  FLOOR = 2.2e-6: the float32 oracle's own largest block distance over the init and both_sides cases (measured 2.15e-6,
  both_sides 86 x 100 B 128, block 4.bias; tests/test_disc_regimes_host.py re-derives it).
  F = 2.0: twice the worst max(0, HIP - FLOOR) / float32 ratio measured on the MI355X is 0.59, so the lower limit 2 holds.  The
  worst ratio, 0.30, is saturated 150 x 256 B 128 on the global-weight instances, block 0.weight: HIP 3.56e-6 (the largest HIP
  distance of all cases and variants), float32 oracle 4.59e-6.  In every init and both_sides case, ragged ones included, the
  ratio is 0: HIP sits inside FLOOR (largest 1.82e-6, both_sides 86 x 100 on the 4-row kernels, block 4.bias).
  The float32 distance is the largest over the evaluation and three more with inputs moved by an ulp (disc_regimes.describe).
Rewards at scale (8, 4), per element: |got - r64| <= RTOL |r64| + ATOL + C 2^-24 (1 / (1 - s64 + 1e-7) + 1 / (s64 + 1e-7)), C = 2.0:
  the float32 oracle's own worst multiple of the last term is 0.915 (7 x 16 seed 0; tests/test_disc_regimes_host.py), doubled, and
  not below 2.  HIP's measured multiple is the same 0.915 on the same element, and equal to the float32 oracle's in all twelve
  cases: where the envelope matters s is saturated, a logit error of 1e-6 moves it by 1e-12, so both round s64 to the same float32.
SG_DISC_REGIMES_RECORD=<path> writes every case's and variant's per-block distances (HIP and float32), and HIP's multiple of the
reward envelope, to that file (profiles/disc_regimes_parity.json)."""
import json
import os

import numpy as np
import pytest

import disc_regimes as dr
from helpers import ATOL, RTOL, assert_close, assert_close_adam
from test_gpu_world import Box, Loader, run_ranks, shard

pytestmark = pytest.mark.gpu

F, FLOOR = 2.0, 2.2e-6
C = 2.0
LR = 1e-3


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


@pytest.fixture(autouse=True)
def _no_inherited_knobs(monkeypatch):
    for k in ("SG_DISC_CHAIN", "SG_DISC_FUSED", "SG_DISC_GW"):
        monkeypatch.delenv(k, raising=False)


def npv(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def _record(section, label, rec):
    path = os.environ.get("SG_DISC_REGIMES_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_disc_regimes.py under SG_DISC_REGIMES_RECORD.  gradient: per parameter block, the distance of the HIP "
                       "one-step gradient and of the float32 oracle's from the float64 reference, ratio = max(0, hip - FLOOR) / float32.  "
                       "rewards: the worst excess over (RTOL, ATOL) in units of the conditioning envelope, HIP and the float32 oracle.",
               "gradient": {}, "rewards": {}}
    doc[section][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


VARIANT_ENV = {"thin_unfused": {"SG_DISC_CHAIN": "thin", "SG_DISC_FUSED": "0"}, "thin": {"SG_DISC_CHAIN": "thin"},
               "wide": {"SG_DISC_CHAIN": "wide"}, "gw": {"SG_DISC_GW": "1"}, "default": {}}


def set_variant(monkeypatch, variant):
    for k, x in VARIANT_ENV[variant].items():
        monkeypatch.setenv(k, x)


def variants_of(shape):
    if shape in dr.THIN_SHAPES:
        return ["thin_unfused", "thin", "wide", "gw"]
    return ["wide", "gw"] if shape == (40, 64) else ["default"]


def make_disc(sg, c, ctx=None):
    D = sg.algo.gail.Discriminator(c.F, c.Hd, None) if ctx is None else sg.algo.gail.Discriminator(c.F, c.Hd, None, ctx=ctx)
    assert [(n, tuple(s)) for n, s in D.param_shapes()] == dr.param_shapes(c.F, c.Hd)
    D.set_flat_params(c.params)
    return D


def make_rollout(sg, policy_rows, other_rows, ctx=None):
    """a one-step rollout whose obs_feat[1:] holds the policy rows (obs_feat[0], which the step must not read: other rows)"""
    n, Fin = policy_rows.shape
    ro = sg.RolloutStorage(1, n, (3,), Box((2,)), 1, Fin) if ctx is None else sg.RolloutStorage(1, n, (3,), Box((2,)), 1, Fin, ctx=ctx)
    ro.obs_feat.copy_(ro.obs_feat.new_tensor(np.stack([other_rows, policy_rows])))
    return ro


def one_step(sg, c, D=None):
    """one epoch of exactly one step on the case's rows in their own order -> (D, losses, m, v)"""
    D = make_disc(sg, c) if D is None else D
    nb = c.expert.shape[0]
    idx = np.arange(nb, dtype=np.int64)
    losses = D.update_gail_dyn(Loader(c.expert, nb), make_rollout(sg, c.policy, c.expert), expert_perm=idx, policy_perm=idx, alpha=c.alpha)
    m, v, step = D.get_adam()
    assert step == 1 and D.last_n_steps == 1
    return D, losses, m, v


def check_one_step_gradient(sg, c, label):
    """Adam's m = 0.1 g and v = 0.001 g^2 after the first step ARE the gradient: block by block against float64."""
    d = c.desc
    g64, o32 = d["grad"], d["o32"]
    _, losses, m, v = one_step(sg, c)
    assert np.isfinite(m).all() and np.isfinite(v).all() and np.isfinite(losses).all(), label
    hip = dr.block_distances(m.astype(np.float64) / 0.1, g64, c.F, c.Hd)
    ratio = {k: (max(0.0, hip[k] - FLOOR) / o32[k] if o32[k] > 0 else (0.0 if hip[k] <= FLOOR else float("inf"))) for k in hip}
    worst = max(ratio, key=ratio.get)
    print(f"{label}: worst block {worst}: HIP {hip[worst]:.3e}, float32 {o32[worst]:.3e}, ratio {ratio[worst]:.2f}; "
          f"largest HIP distance {max(hip.values()):.3e}")
    _record("gradient", label, {"case": c.tag, "hip_vs_f64": hip, "float32_vs_f64": o32, "worst_ratio": ratio[worst], "worst_hip": max(hip.values())})
    fails = [f"{k}: HIP {hip[k]:.3e} from float64 (contract {RTOL:g}; float32 oracle {o32[k]:.3e}, limit {F * o32[k] + FLOOR:.3e})"
             for k in hip if not (hip[k] <= RTOL and hip[k] <= F * o32[k] + FLOOR)]
    assert not fails, (label, fails)
    vd = dr.block_distances(np.sqrt(v.astype(np.float64) / 0.001), np.abs(g64), c.F, c.Hd)
    assert max(vd.values()) <= RTOL, (label, "sqrt(v / 0.001) against |float64 gradient|", {k: x for k, x in vd.items() if x > RTOL})
    assert_close(losses, d["losses"], what=f"{label}: losses")


# ------------------------------------------------------------------------------------------- C: the one-step gradient
GRAD_CASES = [(r, s, v) for r in dr.REGIMES for s in dr.SHAPES for v in variants_of(s)]


@pytest.mark.parametrize("regime,shape,variant", GRAD_CASES, ids=[f"{r}-{s[0]}x{s[1]}-{v}" for r, s, v in GRAD_CASES])
def test_one_step_gradient(sg, monkeypatch, regime, shape, variant):
    """128 rows: eight 16-row groups, thirty-two 4-row groups.  both_sides holds at least 8 rows on each side of |g| = 1 (the sign
    of c_r, v_sqrt / v_rcp on both sides) and logits of both signs in expert and in policy rows; saturated reaches |logit| >= 6."""
    set_variant(monkeypatch, variant)
    check_one_step_gradient(sg, dr.case(regime, *shape), f"C {regime} {shape[0]}x{shape[1]} B {dr.B} {variant}")


RAGGED = [(s, nb, v) for s in dr.RAGGED_SHAPES for nb in dr.RAGGED_B for v in ("thin", "wide")]


@pytest.mark.parametrize("shape,nb,variant", RAGGED, ids=[f"{s[0]}x{s[1]}-B{nb}-{v}" for s, nb, v in RAGGED])
def test_one_step_gradient_ragged(sg, monkeypatch, shape, nb, variant):
    """batch sizes that are no multiple of the 4-row / 16-row groups, and a single row"""
    set_variant(monkeypatch, variant)
    check_one_step_gradient(sg, dr.case("both_sides", *shape, nb), f"C both_sides {shape[0]}x{shape[1]} B {nb} {variant}")


@pytest.mark.parametrize("regime", ["both_sides", "saturated"])
def test_one_launch_step_gives_the_two_launch_steps_bits(sg, monkeypatch, regime):
    """k_disc_step4 forced (SG_DISC_FUSED=1) against k_disc_chain4 + k_disc_wgrad (SG_DISC_FUSED=0) at 86 x 100: m, v, weights
    and losses bit-equal off the initialisation regime too."""
    c = dr.case(regime, 86, 100)
    out = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("SG_DISC_CHAIN", "thin")
        monkeypatch.setenv("SG_DISC_FUSED", fused)
        D, losses, m, v = one_step(sg, c)
        out[fused] = (np.asarray(losses), m, v, D.get_flat_params())
    for a, b, what in zip(out["0"], out["1"], ("losses", "m", "v", "weights")):
        assert np.array_equal(a, b), f"{what}: {int((np.asarray(a) != np.asarray(b)).sum())} elements differ"
    assert np.abs(out["1"][1]).max() > 0


@pytest.mark.parametrize("variant", ["thin_unfused", "thin", "wide", "gw"])
def test_zero_input_gradient_is_an_exact_edge(sg, monkeypatch, variant):
    """4.weight = 0: g = 0 on every row, where c_r = 2 lambda / B (|g| - 1) / |g| is 0 / 0 and the `nn > 0` guard (the reference's
    zero subgradient of the norm) applies.  Nothing may be NaN or Inf; every block below the head has m == v == 0 exactly; the head's
    two blocks hold the contract against float64.  Every logit is 4.bias, so the epoch's total loss is the penalty's value,
    compute_grad_pen_combined's lambda (0 - 1)^2, plus the two BCE terms of that one logit.  (The total cannot EQUAL the penalty:
    the BCE terms softplus(-b) + softplus(b) >= 2 ln 2 are part of it; the test holds total - expert - policy to the penalty and
    all three to the closed forms.)"""
    set_variant(monkeypatch, variant)
    c = dr.zero_head_case()
    d = c.desc
    D = make_disc(sg, c)
    pen = float(D.compute_grad_pen_combined(c.expert, c.policy, 10.0, alpha=c.alpha))      # at the case's weights: before the step
    D, losses, m, v = one_step(sg, c, D)
    assert np.isfinite(losses).all() and np.isfinite(m).all() and np.isfinite(v).all() and np.isfinite(D.get_flat_params()).all()
    assert_close(pen, dr.LAMBDA, what="penalty at g = 0")
    assert_close(losses[0], pen + d["losses"][1] + d["losses"][2], what="total loss = penalty + BCE terms of the one logit")
    assert_close(losses[0] - losses[1] - losses[2], pen, what="total - expert - policy = penalty")
    assert_close(losses, d["losses"], what="losses")
    for name in ("0.weight", "0.bias", "2.weight", "2.bias"):
        sl = dr.block_slice(c.F, c.Hd, name)
        assert not m[sl].any() and not v[sl].any(), f"{name}: {int(np.count_nonzero(m[sl]))} non-zero elements of m, max {np.abs(m[sl]).max():.3e}"
    hip = dr.block_distances(m.astype(np.float64) / 0.1, d["grad"], c.F, c.Hd)
    vd = dr.block_distances(np.sqrt(v.astype(np.float64) / 0.001), np.abs(d["grad"]), c.F, c.Hd)
    for name in ("4.weight", "4.bias"):
        assert hip[name] <= RTOL and vd[name] <= RTOL, (name, hip[name], vd[name])
    _record("gradient", f"C zero_head 86x100 {variant}", {"case": c.tag, "hip_vs_f64": hip, "float32_vs_f64": d["o32"]})


# ------------------------------------------------------------------------------------------- D: moments over real epochs
EPOCHS = [(s, v) for s in dr.EPOCH_SHAPES for v in ("thin", "wide", "gw")]


@pytest.mark.parametrize("shape,variant", EPOCHS, ids=[f"{s[0]}x{s[1]}-{v}" for s, v in EPOCHS])
def test_moments_over_two_epochs_and_far_from_step_zero(sg, monkeypatch, shape, variant):
    """Two epochs of six 32-row steps from both_sides weights: losses, m, v and weights against oracle64.disc_update from the same
    state (m and v at the tolerances tests/test_gpu_regimes.py uses for PPO).  Then set_adam(m0, v0, 200000) and one step: the
    bias corrections far from step 0, moments that are not the gradient's own -- the three Adam implementations of
    sg_disc_kernels.hpp (k_disc_wgrad's tiles and vectors, k_disc_step4's)."""
    set_variant(monkeypatch, variant)
    c = dr.epoch_case(*shape)
    nb, n = dr.EPOCH_B, dr.EPOCH_B * dr.EPOCH_STEPS
    ref = dr.disc_update64(c, c.draws, nb)
    D = make_disc(sg, c)
    ro, loader = make_rollout(sg, c.policy, c.expert), Loader(c.expert, nb)
    for e, (ep, pp, al) in enumerate(c.draws):
        losses = D.update_gail_dyn(loader, ro, expert_perm=ep, policy_perm=pp, alpha=al)
        assert D.last_n_steps == dr.EPOCH_STEPS
        assert_close(losses, ref["losses"][e], what=f"losses, epoch {e}")
    m, v, step = D.get_adam()
    assert step == ref["steps"] == 2 * dr.EPOCH_STEPS
    assert_close(m, ref["m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert_close(v, ref["v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close_adam(D.get_flat_params(), ref["params"], lr=LR, steps=12, what="weights after 12 steps")
    # far from step 0
    rng = np.random.default_rng(11)
    m0 = (1e-3 * rng.standard_normal(c.params.size)).astype(np.float32)
    v0 = (m0.astype(np.float64) ** 2 + 1e-8).astype(np.float32)
    idx = np.arange(nb, dtype=np.int64)
    e1, p1, a1 = c.expert[:nb], c.policy[:nb], c.alpha[:nb]
    ref = dr.disc_update64(c, [(idx, idx, a1)], nb, adam=(m0, v0, 200000), expert=e1, policy=p1)
    D = make_disc(sg, c)
    D.set_adam(m0, v0, 200000)
    losses = D.update_gail_dyn(Loader(e1, nb), make_rollout(sg, p1, e1), expert_perm=idx, policy_perm=idx, alpha=a1)
    m, v, step = D.get_adam()
    assert step == 200001 == ref["steps"]
    assert_close(losses, ref["losses"][0], what="losses, step 200001")
    assert_close(m, ref["m"], rtol=1e-3, atol=1e-7, what="adam m, step 200001")
    assert_close(v, ref["v"], rtol=1e-3, atol=1e-10, what="adam v, step 200001")
    assert_close_adam(D.get_flat_params(), ref["params"], lr=LR, steps=1, what="weights after step 200001")
    assert np.abs(D.get_flat_params() - c.params).max() > 0.5 * LR * 0.1      # the step was taken with these moments


@pytest.mark.parametrize("mode", ["replicated", "sharded"])
@pytest.mark.parametrize("shape", [(7, 16), (86, 100)], ids=["7x16", "86x100"])
def test_world2_gradient_of_the_global_minibatch(sg, shape, mode):
    """Two ranks on one device (the loopback harness of tests/test_gpu_world.py), 64 columns each, one step: in replicated mode
    every rank computes the 128-row gradient itself, in sharded mode each takes 64 rows at inv_B = 1 / 128 and the all-reduce sums
    them.  m / 0.1 on every rank is the float64 gradient of the GLOBAL minibatch block by block -- a 1 / B_local, or a sum
    taken twice, is a distance of 1 -- and m is bit-equal across ranks."""
    c = dr.case("both_sides", *shape)
    world, n_loc = 2, dr.B // 2
    feat = np.stack([c.expert, c.policy])      # [T + 1 = 2, N_global, F]
    idx = np.arange(dr.B, dtype=np.int64)

    def rank_fn(rank, ctx):
        ctx.set_disc_dp(mode == "sharded")
        D = make_disc(sg, c, ctx)
        ro = sg.RolloutStorage(1, n_loc, (3,), Box((2,)), 1, c.F, ctx=ctx)
        ro.obs_feat.copy_(ro.obs_feat.new_tensor(shard(feat, rank, n_loc)))
        losses = D.update_gail_dyn(Loader(c.expert, dr.B), ro, expert_perm=idx, policy_perm=idx, alpha=c.alpha)
        m, v, step = D.get_adam()
        return dict(losses=losses, m=m, v=v, step=step, n=D.last_n_steps)

    res = run_ranks(world, rank_fn)
    for rank, r in enumerate(res):
        assert r["step"] == 1 and r["n"] == 1
        assert np.array_equal(r["m"], res[0]["m"]) and np.array_equal(r["v"], res[0]["v"]), f"rank {rank}: moments differ from rank 0's"
        hip = dr.block_distances(r["m"].astype(np.float64) / 0.1, c.desc["grad"], c.F, c.Hd)
        assert max(hip.values()) <= RTOL, (f"rank {rank}, {mode}", hip)
        assert_close(r["losses"], c.desc["losses"], what=f"rank {rank}, {mode}: losses")
    _record("gradient", f"D world 2 {mode} {shape[0]}x{shape[1]}", {"case": c.tag, "hip_vs_f64": hip, "float32_vs_f64": c.desc["o32"]})


# ------------------------------------------------------------------------------------------- E: rewards
REWARD_CASES = [(s, seed) for s in dr.REWARD_SHAPES for seed in dr.REWARD_SEEDS]
REWARD_IDS = [f"{s[0]}x{s[1]}-seed{seed}" for s, seed in REWARD_CASES]


def _two_reward_calls(sg, c):
    D = make_disc(sg, c)
    assert D.returns is None
    out = []
    for k in range(2):
        rew, ret = D.predict_reward_combined(c.x[k], c.gamma, c.masks[k], offset=c.offset[k])
        out.append((npv(rew)[:, 0].astype(np.float64), npv(ret)[:, 0].astype(np.float64), npv(D.predict_prob(c.x[k]))[:, 0].astype(np.float64)))
    return out


@pytest.mark.parametrize("shape,seed", REWARD_CASES, ids=REWARD_IDS)
def test_rewards_at_logits_of_six_hold_the_plain_contract(sg, shape, seed):
    """scale (4, 3): |reward| up to about 6.  Two consecutive calls, the second with masks mixing 0 and 1 and an offset, so
    Discriminator.returns is carried and reset."""
    c = dr.reward_case(*shape, 4.0, 3.0, seed)
    want, got = dr.rewards64(c), _two_reward_calls(sg, c)
    for k in range(2):
        assert_close(got[k][0], want[k][0], what=f"{c.tag}: reward, call {k}")
        assert_close(got[k][1], want[k][1], what=f"{c.tag}: returns, call {k}")
        assert_close(got[k][2], want[k][2], what=f"{c.tag}: predict_prob, call {k}")
    assert (c.masks[1] == 0).any() and (c.masks[1] == 1).any()


@pytest.mark.parametrize("shape,seed", REWARD_CASES, ids=REWARD_IDS)
def test_rewards_at_logits_of_thirteen_hold_the_conditioning_envelope(sg, shape, seed):
    """scale (8, 4): |reward| up to about 13, where one ulp of s is 1e-3 of the reward in any float32 evaluation.  Per element
    |got - r64| <= RTOL |r64| + ATOL + C envelope(s64); returns carry the first call's bound through gamma * mask; predict_prob
    holds the plain contract against s64."""
    c = dr.reward_case(*shape, 8.0, 4.0, seed)
    want, got = dr.rewards64(c), _two_reward_calls(sg, c)
    from oracle import oracle as o32
    worst, worst32, carried, ret32 = 0.0, 0.0, 0.0, None
    for k in range(2):
        r64, ret64, s64 = want[k]
        bound = RTOL * np.abs(r64) + ATOL + C * dr.reward_envelope(s64)
        r32, ret32 = o32.disc_predict_reward(c.F, c.Hd, c.params, c.x[k], c.gamma, c.masks[k], c.offset[k], ret32)
        worst, worst32 = max(worst, float(dr.reward_excess(got[k][0], r64, s64).max())), max(worst32, float(dr.reward_excess(r32[:, 0], r64, s64).max()))
        print(f"{c.tag} call {k}: |reward| up to {np.abs(r64).max():.2f}; HIP {worst:.3f} envelopes over (RTOL, ATOL), float32 oracle {worst32:.3f}")
        err = np.abs(got[k][0] - r64)
        assert (err <= bound).all(), f"{c.tag}: reward, call {k}: {int((err > bound).sum())} outside, worst {float((err / bound).max()):.2f} x the bound"
        rbound = RTOL * np.abs(ret64) + ATOL + C * dr.reward_envelope(s64) + c.gamma * c.masks[k] * carried
        rerr = np.abs(got[k][1] - ret64)
        assert (rerr <= rbound).all(), f"{c.tag}: returns, call {k}: worst {float((rerr / rbound).max()):.2f} x the bound"
        carried = rbound
        assert_close(got[k][2], s64, what=f"{c.tag}: predict_prob, call {k}")
    _record("rewards", c.tag, {"hip_multiple": worst, "float32_multiple": worst32, "C": C, "max_abs_reward": float(max(np.abs(w[0]).max() for w in want))})


@pytest.mark.parametrize("shape", dr.REWARD_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in dr.REWARD_SHAPES])
def test_relabel_at_logits_of_six(sg, shape):
    """relabel_rewards (T 6, N 16) at scale (4, 3) against oracle64.relabel, two calls with Discriminator.returns and the running
    statistics carried; the masks hold a done at t = 0, a done at T - 1 and one column that is done throughout."""
    from oracle import oracle64 as o64
    c = dr.relabel_case(*shape)
    D = make_disc(sg, c)
    rms = sg.RunningMeanStd(shape=())
    ret, st = None, list(rms.get_state())
    for k in range(2):
        ro = sg.RolloutStorage(c.T, c.N, (3,), Box((2,)), 1, c.F)
        ro.obs_feat.copy_(ro.obs_feat.new_tensor(c.obs_feat[k]))
        ro.masks.copy_(ro.masks.new_tensor(c.masks[k][..., None]))
        D.relabel_rewards(ro, c.gamma, c.offset[k], rms)
        want, ret, st = o64.relabel(c.F, c.Hd, c.params, c.obs_feat[k], c.masks[k], c.gamma, c.offset[k], ret, st)
        assert_close(npv(ro.rewards)[..., 0], want, what=f"{c.tag}: rewards, call {k}")
        assert_close(npv(D.returns)[:, 0], ret, what=f"{c.tag}: Discriminator.returns, call {k}")
        assert_close(rms.get_state(), st, what=f"{c.tag}: ret_rms, call {k}")
