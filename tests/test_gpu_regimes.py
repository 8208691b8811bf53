"""GPU: PPO / A2C / GRU parity off the on-policy path.  The rest of the GPU suite builds its problems on the behaviour policy itself
(ratio == 1, values inside the clip) with max_grad_norm = 0.5 < the gradient norm and use_clipped_value_loss = True; here the
kernels run on the cases of tests/regimes.py, each proven on the float64 references alone (tests/test_regimes_host.py) to hold
rows in every branch of the clipped surrogate and of the clipped value loss, none within 1e-4 of a branch boundary:

  2a  the one-step gradient (Adam's m / 0.1 after one step at max_grad_norm = 1e9), block by block, on every shape, with and
      without the clipped value loss, on the fused, unfused and global-weight launch paths;
  2b  `all_clipped`: every row in a zero-gradient branch -> m == v == 0 exactly and bit-identical parameters;
  2c  both sides of the gradient clip (max_grad_norm = 0.5 and 5.0), PPO, recurrent PPO and A2C, and the ratio of the moments;
  2d  every log-prob pass of k_ppo_bwd the launcher can reach;
  2e  saturated tanh units and GRU gates: forward, gradient, A2C, and an update from Adam state far from step 0.

Tolerances of the gradient comparisons (2a, 2d, 2e), per parameter block (GRU tensors gate by gate), distance =
||got - float64||_2 / (||float64||_2 + ATOL max|float64| sqrt(n)):
  * the project's contract: distance <= helpers.RTOL = 1e-4;
  * the arbiter form of tests/test_gpu_f64_arbiter.py: distance <= F x (the float32 evaluation's distance on the same block) + FLOOR,
    where the float32 evaluation is oracle/sg_oracle.c (gru_ref at float32 for the recurrent policy).
  F = 2.1: twice the worst HIP / float32 ratio measured on the MI355X, max(0, HIP - FLOOR) / float32 = 1.03 (recurrent policy
  47 x 12 x 64 at saturated(8, 5), block base.gru.bias_hh_l0[n]; every off_policy case: 0, HIP sits inside FLOOR), and not below 2.
  The largest HIP distance measured is 7.8e-5 (the same case), the largest at scale 1 is 5.3e-6 (profiles/regimes_parity.json).
  FLOOR = 8.7e-6: the float32 evaluation's own largest block distance over the off_policy cases, the least saturated ones
  (measured 8.66e-6, mlp 20 x 130 x 32; tests/test_regimes_host.py re-derives it).
The float32 distance is the largest over the evaluation and three more with inputs moved by an ulp (regimes.describe).
SG_REGIMES_RECORD=<path> writes every case's per-block distances (HIP and float32) to that file."""
import json
import os

import numpy as np
import pytest

import regimes as rg
from helpers import ATOL, RTOL, assert_close, assert_close_adam, load

pytestmark = pytest.mark.gpu

F, FLOOR = 2.1, 8.7e-6
LR, EPS = rg.LR, rg.EPS


class Box:  # duck-typed gym.spaces.Box
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def npv(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def _record(label, rec):
    path = os.environ.get("SG_REGIMES_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_regimes.py under SG_REGIMES_RECORD: per parameter block, the distance of the HIP one-step gradient and "
                       "of the float32 evaluation's from the float64 reference; ratio = max(0, hip - FLOOR) / float32", "cases": {}}
    doc["cases"][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def make_policy(sg, c):
    if c.kind == "split":
        p = sg.SplitPolicy((c.O,), Box((c.A,)), base_kwargs={"hidden_size": c.H, "num_feet": c.f})
    else:
        p = sg.Policy((c.O,), Box((c.A,)), base_kwargs={"recurrent": c.kind == "gru", "hidden_size": c.H})
    assert [(n, tuple(s)) for n, s in p.param_shapes()] == [(n, tuple(s)) for n, s in rg.param_shapes(c.kind, c.O, c.A, c.H, c.f)]
    p.set_flat_params(c.params)
    return p


def make_rollout(sg, c):
    ro = sg.RolloutStorage(c.T, c.N, (c.O,), Box((c.A,)), c.H if c.kind == "gru" else 1, 1)
    for name in ("obs", "actions", "value_preds", "returns", "action_log_probs", "masks"):
        getattr(ro, name).copy_(getattr(ro, name).new_tensor(c[name]))
    if c.kind == "gru":
        ro.recurrent_hidden_states[0].copy_(ro.obs.new_tensor(c.hxs0))
    return ro


def make_ppo(sg, p, c, E, M, max_grad_norm, use_clipped=True):
    return sg.algo.PPO(p, rg.CLIP, E, M, rg.VCOEF, c.entropy_coef, lr=LR, eps=EPS, max_grad_norm=max_grad_norm, use_clipped_value_loss=use_clipped)


def identity_perms(c, E=1):
    """one minibatch of all rows in rollout order (GRU: of all environments): the minibatch is the case's own row order"""
    return np.tile(np.arange(c.N if c.kind == "gru" else c.T * c.N, dtype=np.int64), (E, 1))


def one_step(sg, c, use_clipped, max_grad_norm=1e9):
    """ppo_epoch = 1, one minibatch: -> (policy, agent, losses, m, v) after the step"""
    p = make_policy(sg, c)
    agent = make_ppo(sg, p, c, 1, 1, max_grad_norm, use_clipped)
    losses = agent.update(make_rollout(sg, c), perms=identity_perms(c))
    m, v, step = agent.get_adam()
    assert step == 1
    return p, agent, losses, m, v


def check_one_step_gradient(sg, c, use_clipped, label):
    """Adam's m = 0.1 g and v = 0.001 g^2 after one step at max_grad_norm = 1e9 ARE the gradient: block by block against float64."""
    d = c.desc
    key = "clipped" if use_clipped else "plain"
    g64, l64, o32 = d["grad_" + key], d["losses_" + key], d["o32_" + key]
    assert d["norm" if use_clipped else "norm_plain"] < 0.9 * 1e9      # the clip is inactive
    _, _, losses, m, v = one_step(sg, c, use_clipped)
    hip = rg.block_distances(m.astype(np.float64) / 0.1, g64, c.kind, c.O, c.A, c.H, c.f, ATOL)
    ratio = {k: (max(0.0, hip[k] - FLOOR) / o32[k] if o32[k] > 0 else (0.0 if hip[k] <= FLOOR else float("inf"))) for k in hip}
    worst = max(ratio, key=ratio.get)
    print(f"{label}: worst block {worst}: HIP {hip[worst]:.3e}, float32 {o32[worst]:.3e}, ratio {ratio[worst]:.2f}; "
          f"largest HIP distance {max(hip.values()):.3e}")
    _record(label, {"case": c.tag, "use_clipped_value_loss": use_clipped, "hip_vs_f64": hip, "float32_vs_f64": o32,
                    "worst_ratio": ratio[worst], "worst_hip": max(hip.values())})
    fails = [f"{k}: HIP {hip[k]:.3e} from float64 (contract {RTOL:g}; float32 evaluation {o32[k]:.3e}, limit {F * o32[k] + FLOOR:.3e})"
             for k in hip if not (hip[k] <= RTOL and hip[k] <= F * o32[k] + FLOOR)]
    assert not fails, (label, fails)
    # v = 0.001 g^2: |g| read back from it holds the same contract (|.| cannot move two vectors apart)
    vd = rg.block_distances(np.sqrt(v.astype(np.float64) / 0.001), np.abs(g64), c.kind, c.O, c.A, c.H, c.f, ATOL)
    assert max(vd.values()) <= RTOL, (label, "sqrt(v / 0.001) against |float64 gradient|", {k: x for k, x in vd.items() if x > RTOL})
    assert_close(losses, l64, what=f"{label}: losses")


def case_id(spec):
    kind, O, A, H, f = spec
    return f"{kind}-{O}x{A}x{H}" + (f"f{f}" if kind == "split" else "")


# ------------------------------------------------------------------------------------------- 2a: the gradient, branch by branch
VARIANTS = [(s, v) for s in rg.SHAPES for v in (("fused", "unfused", "gw") if s[0] == "mlp" else ("default", "gw"))]


@pytest.mark.parametrize("use_clipped", [True, False], ids=["clipped_value", "plain_value"])
@pytest.mark.parametrize("spec,variant", VARIANTS, ids=[f"{case_id(s)}-{v}" for s, v in VARIANTS])
def test_one_step_gradient_off_policy(sg, monkeypatch, spec, variant, use_clipped):
    """Every branch of the surrogate (w1 / inr) and of the value loss (m1 / pass, and the unclipped loss) holds at least 8 of
    the 128 rows; a wrong branch moves whole blocks of the gradient by far more than 1e-4."""
    if variant == "unfused":
        monkeypatch.setenv("SG_PPO_FUSED", "0")
    elif variant == "gw":
        monkeypatch.setenv("SG_POLICY_GW", "1")
    c = rg.case("off_policy", *spec)
    check_one_step_gradient(sg, c, use_clipped, f"2a {case_id(spec)} {variant} {'clipped' if use_clipped else 'plain'}")


# ------------------------------------------------------------------------------------------- 2b: exact zeros
@pytest.mark.parametrize("spec", rg.SHAPES, ids=[case_id(s) for s in rg.SHAPES])
def test_all_clipped_rows_give_exact_zeros(sg, spec):
    """Every row sits in a branch whose gradient is zero (the surrogate's min picked the clipped term, the value loss's max the
    clipped value outside the clip) and entropy_coef = 0: the gradient of every block -- actor, log-std, critic, the GRU's
    tensors -- is exactly 0, its norm 0, the clip coefficient clamps to 1 and Adam's step is 0 / (0 + eps)."""
    c = rg.case("all_clipped", *spec)
    assert not c.desc["grad_clipped"].any() and c.desc["actor_zero"].all() and c.desc["value_zero"].all()
    p, agent, losses, m, v = one_step(sg, c, True, max_grad_norm=0.5)
    assert np.array_equal(m, np.zeros_like(m)), f"{int(np.count_nonzero(m))} non-zero elements of m, max {np.abs(m).max():.3e}"
    assert np.array_equal(v, np.zeros_like(v)), f"{int(np.count_nonzero(v))} non-zero elements of v"
    assert np.array_equal(p.get_flat_params().view(np.uint32), c.params.view(np.uint32)), "the parameters moved"
    assert_close(losses, c.desc["losses_clipped"], what="losses")


# ------------------------------------------------------------------------------------------- 2c: both sides of the gradient clip
def _blockwise_ratio(c, num, den):
    return {k: float((a * b).sum() / (b * b).sum()) for (k, a), (_, b) in zip(rg.blocks(c.kind, c.O, c.A, c.H, c.f, np.asarray(num, np.float64)),
                                                                              rg.blocks(c.kind, c.O, c.A, c.H, c.f, np.asarray(den, np.float64)))}


@pytest.mark.parametrize("spec,perm_seed", rg.CLIP_CASES, ids=[case_id(s) for s, _ in rg.CLIP_CASES])
def test_ppo_on_both_sides_of_the_gradient_clip(sg, spec, perm_seed):
    """max_grad_norm = 0.5 (coef = 0.5 / norm < 1) and 5.0 (coef clamps to 1) on the same case; the float64 norm of every one
    of the 8 steps lies between them with 10 % to spare (tests/test_regimes_host.py).  Two updates of E = 2, M = 2."""
    c = rg.case("off_policy", *spec)
    perms = rg.clip_perms(c, perm_seed)
    for mg in (0.5, 5.0):
        ref = rg.ppo_update64(c, perms, 2, 2, LR, EPS, mg, updates=2)
        assert min(ref["norms"]) >= 1.1 * 0.5 and max(ref["norms"]) <= 0.9 * 5.0, ref["norms"]
        p = make_policy(sg, c)
        agent, ro = make_ppo(sg, p, c, 2, 2, mg), make_rollout(sg, c)
        for _ in range(2):
            losses = agent.update(ro, perms=perms)
        m, v, step = agent.get_adam()
        assert step == ref["steps"] == 8
        assert_close(losses, ref["losses"], what=f"max_grad_norm {mg}: losses")
        assert_close(m, ref["m"], rtol=1e-3, atol=1e-7, what=f"max_grad_norm {mg}: adam m")
        assert_close(v, ref["v"], rtol=1e-3, atol=1e-10, what=f"max_grad_norm {mg}: adam v")
        assert_close_adam(p.get_flat_params(), ref["params"], LR, 8, what=f"max_grad_norm {mg}: params")
    # after the FIRST step m = 0.1 coef g: the same gradient under the two settings, so m(5.0) / m(0.5), block by block, is the
    # ratio of the two clip coefficients, 1 / (0.5 / (norm + 1e-6)).  Adam's parameters hardly see a coefficient that is
    # wrong in one branch only; this ratio does.  Its tolerance is the contract's: the norm is a function of the gradient.
    m5, m05 = one_step(sg, c, True, 5.0)[3], one_step(sg, c, True, 0.5)[3]
    want = (c.desc["norm"] + 1e-6) / 0.5
    assert 1.1 * 0.5 <= c.desc["norm"] <= 0.9 * 5.0
    for k, r in _blockwise_ratio(c, m5, m05).items():
        assert abs(r - want) <= RTOL * want, f"{k}: m(5.0) / m(0.5) = {r:.7g}, the clip coefficients' ratio is {want:.7g}"
    assert_close(m5, 0.1 * c.desc["grad_clipped"], rtol=1e-3, atol=1e-7, what="m at max_grad_norm 5.0 is 0.1 g")


def test_a2c_on_both_sides_of_the_gradient_clip(sg):
    """k_a2c_rmsprop's clip coefficient: one RMSprop update at max_grad_norm = 0.5 and at 5.0 against the float64 restatement;
    square_avg = 0.01 (coef g)^2, so sqrt(square_avg(5.0) / square_avg(0.5)) is the ratio of the coefficients."""
    c = rg.case("off_policy", *rg.A2C_CLIP_CASE)
    lr, sq = 7e-4, {}
    for mg in (0.5, 5.0):
        want_p, want_sq, want_l, norm = rg.a2c_restated(c, mg, lr)
        assert 1.1 * 0.5 <= norm <= 0.9 * 5.0
        p = make_policy(sg, c)
        agent = sg.algo.A2C_ACKTR(p, rg.VCOEF, c.entropy_coef, lr=lr, eps=EPS, alpha=0.99, max_grad_norm=mg)
        losses = agent.update(make_rollout(sg, c))
        sq[mg], _ = agent.get_rmsprop()
        assert_close(losses, want_l, what=f"max_grad_norm {mg}: losses")
        assert_close(sq[mg], want_sq, rtol=1e-3, atol=1e-12, what=f"max_grad_norm {mg}: square_avg")
        assert_close_adam(p.get_flat_params(), want_p, lr=lr, steps=1, what=f"max_grad_norm {mg}: params")
    want = ((norm + 1e-6) / 0.5) ** 2
    for k, r in _blockwise_ratio(c, sq[5.0], sq[0.5]).items():
        assert abs(r - want) <= 2 * RTOL * want, f"{k}: square_avg(5.0) / square_avg(0.5) = {r:.7g}, want {want:.7g}"


# ------------------------------------------------------------------------------------------- 2d: every log-prob pass
# (SG_PPO_ROWS, SG_PPO_WAVES or None, shape, the pass the derivation below says it takes)
LOGP_CASES = [("16", None, ("mlp", 20, 12, 32, 1), "fast L=16"), ("32", None, ("mlp", 20, 12, 32, 1), "fast L=16, 512 threads"),
              ("64", None, ("mlp", 20, 12, 32, 1), "fast L=8"), ("32", "4", ("mlp", 20, 12, 32, 1), "fast L=8, 256 threads"),
              ("64", "4", ("mlp", 20, 12, 32, 1), "fast L=4"),
              ("64", None, ("mlp", 20, 40, 32, 1), "fast L=8, 5 dims per lane"), ("64", "4", ("mlp", 20, 40, 32, 1), "general (40 > 32)"),
              ("32", None, ("mlp", 20, 70, 32, 1), "fast L=16, 5 dims per lane"), ("32", "4", ("mlp", 20, 70, 32, 1), "general (70 > 64)"),
              ("16", None, ("mlp", 20, 130, 32, 1), "general (130 > 128)"),
              ("64", None, ("split", 14, 35, 32, 5), "fast L=8, split heads"), ("64", "4", ("split", 14, 35, 32, 5), "general, split heads")]


@pytest.mark.parametrize("rows,waves,spec,which", LOGP_CASES,
                         ids=[f"rows{r}" + (f"-waves{w}" if w else "") + f"-{case_id(s)}" for r, w, s, _ in LOGP_CASES])
def test_every_log_prob_pass(sg, monkeypatch, rows, waves, spec, which):
    """Which pass of k_ppo_bwd's Gaussian log-prob phase a launch takes (simgan_amd/csrc/sg_ppo.hip, sg_ppo_kernels.hpp):
    a row group is R = 16 MT rows, MT = SG_PPO_ROWS / 16 (default: 1 at these 128-row minibatches); the workgroup has 512
    threads when MT >= 2 and SG_PPO_WAVES != 4, else 256; a row gets L = threads / R lanes:
        SG_PPO_ROWS   16    32    64      with SG_PPO_WAVES=4:   16    32    64
        L             16    16     8                             16     8     4
    The fast pass (hardware exp / rcp, log(exp(ls)) taken as ls, at most 8 action dimensions per lane) runs when A <= 8 L and
    reduces a row's lanes with DPP butterflies: two steps for L = 4, a third for L >= 8, a fourth for L = 16.  The general pass
    (libm, 32 lanes per row, shuffles) runs when A > 8 L: A > 128 at 16-row groups, A > 64 at 32 rows with 4 waves, A > 32 at
    64 rows with 4 waves.  No geometry the launcher can choose gives L >= 32, so the fast pass has no other reduction.
    The one-step gradient, branch by branch as in 2a, on an off_policy case at each."""
    monkeypatch.setenv("SG_PPO_ROWS", rows)
    if waves:
        monkeypatch.setenv("SG_PPO_WAVES", waves)
    R = int(rows)
    L = (512 if R >= 32 and not waves else 256) // R
    assert ("general" in which) == (spec[2] > 8 * L) and (f"L={L}" in which or "general" in which)
    c = rg.case("off_policy", *spec)
    for uc in (True, False):
        check_one_step_gradient(sg, c, uc, f"2d rows{rows} waves{waves or 'default'} {case_id(spec)} {'clipped' if uc else 'plain'}")


def test_64_row_groups_keep_the_reference_trajectory(sg, monkeypatch):
    """SG_PPO_ROWS=64 (k_ppo_fwd / k_ppo_bwd <4, 0, 0>) on the reference-written update of ppo_mlp_tiny."""
    monkeypatch.setenv("SG_PPO_ROWS", "64")
    g = load("ppo_mlp_tiny")
    m = g["meta"]
    p = sg.Policy((m["O"],), Box((m["A"],)), base_kwargs={"recurrent": False, "hidden_size": m["H"]})
    p.set_flat_params(g["params0"])
    ro = sg.RolloutStorage(m["T"], m["N"], (m["O"],), Box((m["A"],)), 1, g["obs_feat"].shape[-1])
    for name in ("obs", "obs_feat", "actions", "rewards", "value_preds", "returns", "action_log_probs", "masks", "bad_masks"):
        if name in g and getattr(ro, name).numel():
            getattr(ro, name).copy_(getattr(ro, name).new_tensor(g[name]))
    agent = sg.algo.PPO(p, m["clip_param"], m["ppo_epoch"], m["num_mini_batch"], m["value_loss_coef"], m["entropy_coef"], lr=m["lr"],
                        eps=m["eps"], max_grad_norm=m["max_grad_norm"])
    losses = agent.update(ro, perms=g["perms"])
    assert_close(losses, g["losses"], what="ppo losses")
    mm, vv, _ = agent.get_adam()
    assert_close(mm, g["adam_m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert_close(vv, g["adam_v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close(p.get_flat_params(), g["params1"], what="params after update")


# ------------------------------------------------------------------------------------------- 2e: saturation
SAT = [(s, sc) for s in rg.SHAPES for sc in rg.SATURATIONS]
SAT_IDS = [f"{case_id(s)}-w{sc[0]:g}o{sc[1]:g}" for s, sc in SAT]


@pytest.mark.parametrize("spec,scales", SAT, ids=SAT_IDS)
def test_saturated_forward(sg, spec, scales):
    """act (injected noise), get_value and evaluate_actions with weights x scale_w, observations x scale_obs: sg_tanh's and
    sg_sigmoid's tails.  float64 references: the arbiter, gru_ref."""
    import gru_ref
    c = rg.case("saturated", *spec, *scales)
    p = make_policy(sg, c)
    B = c.T * c.N
    obs, act = c.obs[:-1].reshape(B, c.O), c.actions.reshape(B, c.A)
    noise = np.random.default_rng(5).standard_normal((B, c.A)).astype(np.float32)
    if c.kind == "gru":
        sd = gru_ref.unflatten(c.params, c.O, c.A, c.H)
        masks = c.masks[:-1].reshape(B, 1)
        v, lp, ent, h = p.evaluate_actions(obs, c.hxs0, masks, act)
        rv, rlp, rent, rh = gru_ref.evaluate(sd, obs, c.hxs0, masks, act)
        assert_close(h, rh, what="sequence rnn_hxs")
        n = c.N
        v1, a1, lp1, h1 = p.act(obs[:n], c.hxs0, masks[:n], noise=noise[:n])
        r1 = gru_ref.act(sd, obs[:n], c.hxs0, masks[:n], noise[:n])
        gv, rgv = p.get_value(obs[:n], c.hxs0, masks[:n]), r1[0]
        assert_close(h1, r1[3], what="act rnn_hxs")
    else:
        from oracle import oracle64 as o64
        d = rg._dims(c, o64)
        v, lp, ent, _ = p.evaluate_actions(obs, None, None, act)
        rv, rlp, rent = o64.policy_evaluate(d, c.params, obs, act)
        v1, a1, lp1, _ = p.act(obs, None, None, noise=noise)
        r1 = o64.policy_act(d, c.params, obs, noise)
        gv, rgv = p.get_value(obs, None, None), r1[0]
    assert_close(v, rv, what="evaluate value")
    assert_close(lp, rlp, what="evaluate logp")
    assert_close(float(npv(ent)), rent, what="entropy")
    assert_close(v1, r1[0], what="act value")
    assert_close(a1, r1[1], what="act action")
    assert_close(lp1, r1[2], what="act logp")
    assert_close(gv, rgv, what="get_value")


@pytest.mark.parametrize("use_clipped", [True, False], ids=["clipped_value", "plain_value"])
@pytest.mark.parametrize("spec,scales", SAT, ids=SAT_IDS)
def test_saturated_one_step_gradient(sg, spec, scales, use_clipped):
    """1 - h^2 and z (1 - z) where the units saturate, under every branch of the losses (the cases are off_policy ones)."""
    c = rg.case("saturated", *spec, *scales)
    check_one_step_gradient(sg, c, use_clipped, f"2e {case_id(spec)} w{scales[0]:g}o{scales[1]:g} {'clipped' if use_clipped else 'plain'}")


def test_saturated_a2c(sg):
    c = rg.case("saturated", "mlp", 47, 12, 64, 1, 4.0, 3.0)
    lr = 7e-4
    want_p, want_sq, want_l, norm = rg.a2c_restated(c, 0.5, lr)
    assert norm >= 1.1 * 0.5
    p = make_policy(sg, c)
    agent = sg.algo.A2C_ACKTR(p, rg.VCOEF, c.entropy_coef, lr=lr, eps=EPS, alpha=0.99, max_grad_norm=0.5)
    losses = agent.update(make_rollout(sg, c))
    assert_close(losses, want_l, what="losses")
    assert_close(agent.get_rmsprop()[0], want_sq, rtol=1e-3, atol=1e-12, what="square_avg")
    assert_close_adam(p.get_flat_params(), want_p, lr=lr, steps=1, what="params after update")


@pytest.mark.parametrize("spec", rg.SHAPES, ids=[case_id(s) for s in rg.SHAPES])
def test_saturated_update_from_adam_state_far_from_step_zero(sg, spec):
    """set_adam(m, v, step = 200000), then one step: the bias-correction slots far from step 0 (1 - 0.9^t and 1 - 0.999^t both
    round to 1), moments that are not the gradient's own.  Against the float64 restatement started from the same state."""
    c = rg.case("saturated", *spec, 4.0, 3.0)
    rng = np.random.default_rng(11)
    m0 = (1e-3 * rng.standard_normal(c.params.size)).astype(np.float32)
    v0 = (m0.astype(np.float64) ** 2 + 1e-8).astype(np.float32)
    ref = rg.ppo_update64(c, identity_perms(c), 1, 1, LR, EPS, 0.5, adam=(m0, v0, 200000))
    assert ref["norms"][0] >= 1.1 * 0.5
    p = make_policy(sg, c)
    agent = make_ppo(sg, p, c, 1, 1, 0.5)
    agent.set_adam(m0, v0, 200000)
    losses = agent.update(make_rollout(sg, c), perms=identity_perms(c))
    m, v, step = agent.get_adam()
    assert step == 200001 == ref["steps"]
    assert_close(losses, ref["losses"], what="losses")
    assert_close(m, ref["m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert_close(v, ref["v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close_adam(p.get_flat_params(), ref["params"], LR, 1, what="params after the step")
