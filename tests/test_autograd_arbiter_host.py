"""CPU: the float64 arbiters held to autograd, not to their own derivations.  Every gradient check of the suite ends at a hand-derived
float64 restatement -- oracle/oracle64.py (PPO for Policy / SplitPolicy, the discriminator step with the double backward of the
gradient penalty), tests/gru_ref.py (back-propagation through time), test_a2c_host.a2c_loss_grad, acktr_regimes.update (Fisher
statistics, the K-FAC step), test_symmetry_host.sym_loss_grad -- and the kernels were written against those.  The reference's
fixtures pin them on the fixtures' own regime only.  Here each restatement is compared with tests/autograd_ref.py -- the reference's
loss written forward-only in torch.float64 and differentiated by torch.autograd, the GRU torch.nn.GRU itself, the K-FAC step a
dense solve -- on EVERY case the GPU regimes files look at, with the family's own block_distances at atol = 0.

Tier 1, per parameter block: distance(restatement, autograd) <= 1e-9.  With the constants of all arbiters on one convention
(autograd_ref's docstring) the worst distance measured is 9.1e-14 for the gradients (recurrent PPO at saturated(8, 5)), 1.4e-14 for a K-FAC
factor and 2.4e-13 for K-FAC's v against the dense solve (damping 1e-5); the smallest discrepancy this check exists to catch is
1.56e-8, one float32-valued constant on one action dimension (what separated gru_ref from oracle64 before).  1e-9 sits four orders
above the first and one below the second.  Where autograd's gradient of a block is exactly 0.0 the restatement's must be exactly 0.0;
the loss terms agree within 1e-12 absolute.  No case is excluded, and none needed a tie-break: every builder keeps every row MARGIN
from a branch boundary, which is asserted here on entry.

Tier 2, where the reference checkout is present (skipped otherwise, like tests/test_interop.py): the reference's own Policy /
SplitPolicy / PPO and Discriminator, imported through tools/ref_import.py in a child process (this process must never import the
reference), .double(), with the case's parameters loaded, run their own loss and .backward(); their .grad against autograd_ref at
the same bound.  This ties tier 1's few lines of torch to the reference itself.

`python tests/autograd_ref.py` writes every figure to profiles/autograd_arbiter.json."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import acktr_regimes as ak
import autograd_ref as ar
import disc_regimes as dr
import gru_ref
import regimes as rg
import sym_regimes as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND, LOSS_ATOL = ar.BOUND, ar.LOSS_ATOL
assert (BOUND, LOSS_ATOL) == (1e-9, 1e-12)


def hold(j, label):
    print(f"{label}: worst block {j['worst_block']} {j['worst']:.3e}, loss terms within {j['loss_error']:.1e}, "
          f"{len(j['zero_blocks'])} blocks exactly zero")
    assert not j["zeros_broken"], f"{label}: autograd's gradient is exactly 0.0 in {j['zeros_broken']} and the restatement's is not"
    bad = {k: x for k, x in j["distances"].items() if not x <= BOUND}
    assert not bad, f"{label}: blocks farther than {BOUND:g} from autograd: {bad}"
    assert j["loss_error"] <= LOSS_ATOL, f"{label}: a loss term is {j['loss_error']:.3e} from autograd's"


def away_from_ties(c):
    """on entry: no row within MARGIN of a branch boundary of the surrogate's min / clamp or the value loss's max / clamp, where
    autograd's subgradient and a restatement's may differ legitimately"""
    d = c.desc
    for k in ("margin_ratio", "margin_value", "margin_uw"):
        assert d[k] >= rg.MARGIN, (c.tag, k, d[k])


def ppo_id(spec):
    regime, kind, O, A, H, f, sw, so = spec
    return f"{regime}-{kind}-{O}x{A}x{H}" + (f"f{f}" if kind == "split" else "") + (f"-w{sw:g}o{so:g}" if regime == "saturated" else "")


# ------------------------------------------------------------------------------------------- PPO: Policy, SplitPolicy, the GRU
@pytest.mark.parametrize("use_clipped", [True, False], ids=["clipped_value", "plain_value"])
@pytest.mark.parametrize("spec", rg.all_cases(), ids=[ppo_id(s) for s in rg.all_cases()])
def test_ppo_restatements_against_autograd(spec, use_clipped):
    """oracle64 (mlp, split) and gru_ref (gru) on regimes.all_cases(), LOGP_SHAPES included: every branch of the clipped surrogate
    and of the clipped value loss, the unclipped value loss, saturated units and gates, the state-dependent log-std heads.  On
    `all_clipped` autograd's gradient is exactly 0.0 in every block (clipped value loss), and so must the restatement's be."""
    c = rg.case(*spec)
    away_from_ties(c)
    j = ar.judge_ppo(c, use_clipped)
    if c.regime == "all_clipped" and use_clipped:
        assert len(j["zero_blocks"]) == len(j["distances"]), (c.tag, "autograd's gradient is not zero everywhere", j["distances"])
    hold(j, f"{c.tag} {'clipped' if use_clipped else 'plain'}")


@pytest.mark.parametrize("spec,perm_seed", rg.CLIP_CASES, ids=[f"{s[0]}-{s[1]}x{s[2]}x{s[3]}" for s, _ in rg.CLIP_CASES])
def test_ppo_minibatch_of_the_clip_cases_against_autograd(spec, perm_seed):
    """CLIP_CASES run E = 2, M = 2: a minibatch is half the rows (GRU: half the environments, whole sequences) with advantages
    normalised over the whole rollout.  The first step's gradient, orc_ppo_grad_rows' row list and gru_ref's gather."""
    c = rg.case("off_policy", *spec)
    away_from_ties(c)
    hold(ar.judge_first_minibatch(c, perm_seed), f"{c.tag}, first minibatch")


def test_a2c_restatement_against_autograd():
    """test_a2c_host.a2c_loss_grad on A2C_CLIP_CASE: advantages.detach() in the action loss, the value loss without a 0.5"""
    c = rg.case("off_policy", *rg.A2C_CLIP_CASE)
    hold(ar.judge_a2c(c), f"A2C {c.tag}")


# ------------------------------------------------------------------------------------------- the discriminator step
DISC = dr.all_cases()


@pytest.mark.parametrize("spec", DISC, ids=[f"{r}-{F}x{Hd}-B{nb}" for r, F, Hd, nb in DISC])
def test_discriminator_restatement_against_autograd(spec):
    """oracle64's hand-written double backward of lambda mean((|dD/dx| - 1)^2) against autograd.grad(create_graph=True) and a second
    autograd.grad, on both sides of |g| = 1, saturated, ragged batches and a single row"""
    c = dr.case(*spec)
    hold(ar.judge_disc(c), c.tag)


def test_discriminator_zero_input_gradient_against_autograd():
    """4.weight = 0: |g| = 0 on every row, where grad.norm(2, dim=1) has no derivative; torch's subgradient there is 0, the
    restatement's `nn > 0` guard gives the same, so the case needs no exclusion.  0.weight .. 2.bias get exactly 0.0 in both."""
    c = dr.zero_head_case()
    assert not c.desc["gnorm"].any()
    j = ar.judge_disc(c)
    assert set(j["zero_blocks"]) == {"0.weight", "0.bias", "2.weight", "2.bias"}, j["zero_blocks"]
    hold(j, c.tag)


@pytest.mark.parametrize("shape", dr.EPOCH_SHAPES, ids=[f"{F}x{Hd}" for F, Hd in dr.EPOCH_SHAPES])
def test_discriminator_first_step_of_an_epoch_against_autograd(shape):
    c = dr.epoch_case(*shape)
    hold(ar.judge_disc(c, rows=ar.epoch_first_step(c, dr.EPOCH_B)), f"{c.tag}, first step")


# ------------------------------------------------------------------------------------------- ACKTR
# the cases whose largest module is small enough for a dense solve of (A' (x) G' + damping I): at most 2048 elements (33 x 33 = 1089
# here; the next size, 64 x 64 = 4096, is a 134 MB matrix and several seconds)
KFAC_SOLVE_CASES = ["unclipped_default", "unclipped_tiles32", "clipped_mild", "eigen_small", "refresh_small"]


def test_the_dense_solve_runs_on_every_case_that_is_small_enough():
    assert KFAC_SOLVE_CASES == [n for n in ak.all_cases() if ar.largest_module(ak.SPECS[n]["dims"]) <= ar.KFAC_SOLVE_MAX]
    regimes = {ak.SPECS[n]["regime"] for n in KFAC_SOLVE_CASES}
    assert regimes == {"unclipped", "clipped", "eigen_dominated", "refresh"}, regimes      # off damping, stale eigenbases included


@pytest.mark.parametrize("name", ak.all_cases())
def test_acktr_restatement_against_autograd(name):
    """Every update of every case: (1) a2c_loss_grad's gradient and losses; (2) all 12 distinct running factors, from autograd.grad of
    pg_fisher_loss + vf_fisher_loss with respect to each layer's pre-activation (fG = B u^T u, fA = a^T a / B, a bias a module of
    its own); (3) on KFAC_SOLVE_CASES, v of every module against numpy.linalg.solve on the rebuilt thresholded factors: the
    eigen path (kfac.py:225-249: rotate, divide by d_g d_a + damping, rotate back) without any eigenbasis in the check."""
    c = ak.case(name)
    for k, r in enumerate(ar.judge_acktr(c, name in KFAC_SOLVE_CASES)):
        label = f"{c.tag} update {k}"
        hold(r["gradient"], label)
        assert set(r["factors"]) == set(ak.FACTORS)
        bad = {f: x for f, x in r["factors"].items() if not x <= BOUND}
        assert not bad, f"{label}: factors farther than {BOUND:g} from autograd's: {bad}"
        assert (r["kfac"] is not None) == (name in KFAC_SOLVE_CASES)
        if r["kfac"] is not None:
            assert set(r["kfac"]) == set(ak.BLOCKS)
            bad = {b: x for b, x in r["kfac"].items() if not x <= BOUND}
            print(f"{label}: v against the dense solve, worst {max(r['kfac'].values()):.3e}")
            assert not bad, f"{label}: v farther than {BOUND:g} from the dense solve: {bad}"


# ------------------------------------------------------------------------------------------- the symmetry loss
SYM = sr.all_cases()


def test_the_floor_cases_are_among_the_cases():
    assert set(sr.floor_cases()) <= set(SYM)


@pytest.mark.parametrize("spec", SYM, ids=["-".join(str(x) for x in s) for s in SYM])
def test_symmetry_restatement_against_autograd(spec):
    """oracle64's PPO gradient + test_symmetry_host.sym_loss_grad against autograd of the whole loss, (M_a mu(s)).detach() included.
    sym_only: autograd's gradient is exactly 0.0 in every critic block and in dist.logstd._bias, and so is the restatement's."""
    c = sr.case(*spec)
    away_from_ties(c)
    for uc in ((True,) if c.regime == "sym_only" else (True, False)):
        j = ar.judge_sym(c, uc)
        if c.regime == "sym_only":
            assert set(j["zero_blocks"]) == {k for k, _ in rg.param_shapes("mlp", c.O, c.A, c.H)} - set(sr.ACTOR_BLOCKS), j["zero_blocks"]
        hold(j, f"{c.tag} {'clipped' if uc else 'plain'}")


# ------------------------------------------------------------------------------------------- the test bites
def fails(j):
    with pytest.raises(AssertionError):
        hold(j, "an injected fault")
    return j["worst"]


def test_a_block_scaled_by_one_part_in_a_million_fails():
    """each family's restatement with ONE block x (1 + 1e-6): the bound is three orders below"""
    c = rg.case("off_policy", "split", 14, 7, 100, 1)
    g = c.desc["grad_clipped"].copy()
    rg.blocks(c.kind, c.O, c.A, c.H, c.f, g)[-1][1][:] *= 1.0 + 1e-6          # (views into g)
    assert 0.5e-6 < fails(ar.judge_ppo(c, True, restated=g)) < 2e-6
    hold(ar.judge_ppo(c, True), "the same case, unscaled")
    d = dr.case("both_sides", 7, 16, 13)
    g = d.desc["grad"].copy()
    g[dr.block_slice(d.F, d.Hd, "2.bias")] *= 1.0 + 1e-6
    assert 0.5e-6 < fails(ar.judge_disc(d, restated=g)) < 2e-6
    a = rg.case("off_policy", *rg.A2C_CLIP_CASE)
    from test_a2c_host import a2c_loss_grad
    B = a.T * a.N
    _, g = a2c_loss_grad(a.params, a.obs[:-1].reshape(B, a.O), a.actions.reshape(B, a.A), a.returns[:-1].reshape(B), (a.O, a.A, a.H, a.H),
                         rg.VCOEF, a.entropy_coef)
    g[:a.H * a.O] *= 1.0 + 1e-6
    assert 0.5e-6 < fails(ar.judge_a2c(a, restated=g)) < 2e-6


def test_swapped_log_std_heads_fail():
    """contact_logstd and actuator_logstd concatenated in the other order (actuator first) in the forward: the arbiter's order is
    the reference's, and the check tells the two apart by eight orders"""
    c = rg.case("off_policy", "split", 14, 7, 100, 1)
    assert fails(ar.judge_ppo(c, True, swap_logstd=True)) > 1e-2


def test_a_transposed_action_mirror_fails_unless_the_mirror_is_symmetric():
    c = sr.case("mixed", 5, 2, 8, "dense", 77)
    assert fails(ar.judge_sym(c, True, m_act=c.m_act.T)) > 1e-2
    lk = sr.case("mixed", 111, 12, 64, "laikago", 128)
    assert np.array_equal(lk.m_act, lk.m_act.T)
    hold(ar.judge_sym(lk, True, m_act=lk.m_act.T), "Laikago's symmetric mirror, transposed: blind, as tests/sym_regimes.py says")


def test_a_differentiated_mirror_fails():
    """without the .detach() of ppo.py's numpy round trip the gradient also flows through M_a mu(s)"""
    c = sr.case("mixed", 5, 2, 8, "dense", 77)
    B = c.T * c.N
    p = ar.leaves(c.params, rg.param_shapes("mlp", c.O, c.A, c.H, 1))
    x, xm = ar.t64(c.obs[:-1].reshape(B, c.O)), ar.t64(c.mrows)
    e = ar.policy_forward("mlp", p, x)[1] @ ar.t64(c.m_act).t() - ar.policy_forward("mlp", p, xm)[1]
    wrong = ar.flat_grad(e.pow(2).mean() * c.symmetry_coef, p)
    d = rg.block_distances(c.symmetry_coef * c.grad_sym1, wrong, "mlp", c.O, c.A, c.H, 1, 0.0)
    assert min(d[k] for k in sr.ACTOR_BLOCKS) > 1e-2, d


# ------------------------------------------------------------------------------------------- one convention
def test_the_float64_arbiters_share_their_constants():
    """oracle64 and gru_ref give the same log-prob for one shared (mean, logstd, action) triple to 1e-14: log(sqrt(2 pi)) is the
    reference's float32 value in both (before, gru_ref's exact double put them 1.56e-8 x A apart), and so are autograd_ref's and
    test_a2c_host's; likewise the 1e-5 of the advantages."""
    from oracle import oracle64 as o64
    import test_a2c_host
    c = rg.case("off_policy", "mlp", 5, 2, 8, 1)
    B = c.T * c.N
    d = rg._dims(c, o64)
    obs, act = c.obs[:-1].reshape(B, c.O), c.actions.reshape(B, c.A)
    _, mean, logstd = o64.policy_forward(d, c.params, obs)
    _, lp64, ent64 = o64.policy_evaluate(d, c.params, obs, act)
    lp_gru = gru_ref.log_prob(mean, logstd, act.astype(np.float64))
    assert np.abs(lp64 - lp_gru).max() <= 1e-14, np.abs(lp64 - lp_gru).max()
    lp_ar = ar.normal_log_probs(ar.t64(mean), ar.t64(logstd), ar.t64(act)).numpy()
    assert np.abs(lp64[:, 0] - lp_ar).max() <= 1e-14
    assert abs(ent64 - float(np.sum(0.5 + gru_ref.HALF_LOG_2PI + logstd[0]))) <= 1e-14
    assert gru_ref.HALF_LOG_2PI == test_a2c_host.HALF_LOG_2PI == ar.HALF_LOG_2PI == float(np.float32(0.5 * np.log(2.0 * np.pi)))
    assert gru_ref.ADV_EPS == ar.ADV_EPS == float(np.float32(1e-5)) and dr.EPS_R == ar.REWARD_EPS == float(np.float32(1e-7))
    vp, ret = c.value_preds[:-1].reshape(B), c.returns[:-1].reshape(B)
    adv = [o64.advantages(ret, vp), rg.advantages64(c).reshape(B), ar.normalised_advantages(ret, vp).numpy()]
    assert np.abs(adv[0] - adv[1]).max() <= 1e-14 and np.abs(adv[0] - adv[2]).max() <= 1e-14


# ------------------------------------------------------------------------------------------- tier 2: the reference's own modules
@pytest.mark.skipif(not ar.reference_present(), reason="needs the reference checkout (development container only)")
def test_the_references_own_modules_against_autograd():
    """autograd_ref.tier2 in a child process: PPO.update of the reference's Policy (mlp, GRU) and SplitPolicy on one off_policy case
    each, both value losses, and Discriminator.update_gail_dyn at both_sides; the .grad they leave against autograd_ref."""
    r = subprocess.run([sys.executable, "-s", os.path.join(ROOT, "tests", "autograd_ref.py"), "--tier2"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT, env={k: v for k, v in os.environ.items() if k != "PYTHONPATH"})
    assert r.returncode == 0, r.stderr[-3000:]
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("TIER2 ")][-1][6:])
    assert len(doc) == 2 * len(ar.TIER2_PPO) + 1 and sum(k.startswith("disc") for k in doc) == 1, list(doc)
    for label, j in doc.items():
        print(f"{label}: worst block {j['worst_block']} {j['worst']:.3e}, loss terms within {j['loss_error']:.1e}")
        assert j["worst"] <= BOUND and not j["zeros_broken"], (label, j)
        # the discriminator builds its BCE targets in float32 whatever the module's dtype, and torch then returns the two BCE terms
        # in float32: its loss terms (not its gradient) carry the float32 round-off of O(1) numbers after .double()
        assert j["loss_error"] <= (1e-6 if label.startswith("disc") else LOSS_ATOL), (label, j)
