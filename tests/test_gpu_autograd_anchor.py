"""GPU: one anchor per family, the HIP one-step gradient held DIRECTLY to autograd (tests/autograd_ref.py: the reference's loss
written forward-only in torch.float64 and differentiated by torch.autograd).  The regimes files hold the kernels to hand-derived
float64 restatements, and tests/test_autograd_arbiter_host.py holds those restatements to autograd; this file closes the triangle on
the device, so that a later edit of a kernel and of its arbiter together still meets an independent party.  One smallest case each.

Nothing here sets a tolerance.  Each test takes the gradient through its family's own helper (one_step, Adam's m / 0.1; A2C:
sqrt(square_avg / 0.01) = |g| at a max_grad_norm the norm stays under) and applies its family's own limit, read from the family's
GPU file: distance <= RTOL and distance <= F x (the float32 evaluation's distance on the same block) + FLOOR, every distance now
measured from autograd's gradient: regimes.block_distances / disc_regimes.block_distances with their ATOL floor; the float32
evaluation's is the largest over the evaluation itself and JITTERS more with inputs moved by at most an ulp, drawn as the family's
builder draws them."""
import numpy as np
import pytest

import autograd_ref as ar
import disc_regimes as dr
import regimes as rg
import sym_regimes as sr
import test_gpu_disc_regimes as family_disc
import test_gpu_regimes as family_ppo
import test_gpu_sym_regimes as family_sym
from helpers import ATOL, RTOL, assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def jitters(seed, stream, arrays, n):
    """the arrays themselves, then n more sets with every element moved by at most an ulp (regimes.describe's recipe)"""
    yield arrays
    for k in range(n):
        jr = np.random.default_rng([seed, k, stream])
        yield [(a * (1.0 + jr.uniform(-1.0, 1.0, a.shape) * 2.0 ** -24)).astype(np.float32) for a in arrays]


def largest(dicts):
    out = {}
    for d in dicts:
        for k, x in d.items():
            out[k] = max(out.get(k, 0.0), x)
    return out


def hold(hip, o32, family, label):
    ratio = {k: max(0.0, hip[k] - family.FLOOR) / o32[k] if o32[k] > 0 else (0.0 if hip[k] <= family.FLOOR else float("inf")) for k in hip}
    worst = max(ratio, key=ratio.get)
    print(f"{label}: worst block {worst}: HIP {hip[worst]:.3e} from autograd, float32 {o32[worst]:.3e}, ratio {ratio[worst]:.2f}; "
          f"largest HIP distance {max(hip.values()):.3e}")
    fails = [f"{k}: HIP {hip[k]:.3e} from autograd (contract {RTOL:g}; float32 evaluation {o32[k]:.3e}, limit {family.F * o32[k] + family.FLOOR:.3e})"
             for k in hip if not (hip[k] <= RTOL and hip[k] <= family.F * o32[k] + family.FLOOR)]
    assert not fails, (label, fails)


def test_discriminator_step_against_autograd(sg, monkeypatch):
    """both_sides 7 x 16 at B = 13: rows on both sides of |g| = 1, three 4-row groups and a single row"""
    for k in ("SG_DISC_CHAIN", "SG_DISC_FUSED", "SG_DISC_GW"):
        monkeypatch.delenv(k, raising=False)
    c = dr.case("both_sides", 7, 16, 13)
    g, losses = ar.disc_case_grad(c)
    o32 = largest(dr.block_distances(dr.grad(c, 32, *j)[0], g, c.F, c.Hd) for j in jitters(c.seed, 79, [c.params, c.expert, c.policy], dr.JITTERS))
    _, got_losses, m, v = family_disc.one_step(sg, c)
    hold(dr.block_distances(m.astype(np.float64) / 0.1, g, c.F, c.Hd), o32, family_disc, f"discriminator {c.tag}")
    vd = dr.block_distances(np.sqrt(v.astype(np.float64) / 0.001), np.abs(g), c.F, c.Hd)
    assert max(vd.values()) <= RTOL, vd
    assert_close(got_losses, losses, what="losses")


@pytest.mark.parametrize("spec", [("mlp", 5, 2, 8, 1), ("split", 14, 7, 100, 1), ("gru", 13, 5, 20, 1)], ids=["mlp-5x2x8", "split-14x7x100", "gru-13x5x20"])
def test_ppo_step_against_autograd(sg, monkeypatch, spec):
    """off_policy, the clipped value loss: Policy, SplitPolicy (the state-dependent log-std heads) and the recurrent Policy (torch.nn.GRU
    against the kernels' back-propagation through time)"""
    for k in ("SG_PPO_FUSED", "SG_POLICY_GW", "SG_PPO_ROWS", "SG_PPO_WAVES"):
        monkeypatch.delenv(k, raising=False)
    c = rg.case("off_policy", *spec)
    g, losses = ar.ppo_case_grad(c, True)
    assert np.sqrt((g * g).sum()) < 0.9 * 1e9
    dist = lambda got: rg.block_distances(got, g, c.kind, c.O, c.A, c.H, c.f, ATOL)  # noqa: E731

    def grad32(params, obs):
        cj = rg.Case(c)
        cj["params"], cj["obs"] = params, obs
        return rg.grad(cj, True, 32)[0]
    o32 = largest(dist(grad32(*j)) for j in jitters(c.seed, 77, [c.params, c.obs], rg.JITTERS))
    _, _, got_losses, m, v = family_ppo.one_step(sg, c, True)
    hold(dist(m.astype(np.float64) / 0.1), o32, family_ppo, f"PPO {c.tag}")
    vd = rg.block_distances(np.sqrt(v.astype(np.float64) / 0.001), np.abs(g), c.kind, c.O, c.A, c.H, c.f, ATOL)
    assert max(vd.values()) <= RTOL, vd
    assert_close(got_losses, losses, what="losses")


def test_a2c_step_against_autograd(sg):
    """A2C_CLIP_CASE at max_grad_norm = 5.0, above the norm: square_avg = (1 - alpha) g^2 after the first RMSprop step, so
    sqrt(square_avg / 0.01) is |g|, block by block against |autograd's gradient|"""
    from test_a2c_host import a2c_loss_grad
    c = rg.case("off_policy", *rg.A2C_CLIP_CASE)
    B, dims = c.T * c.N, (c.O, c.A, c.H, c.H)
    g, losses = ar.a2c_case_grad(c)
    assert np.sqrt((g * g).sum()) <= 0.9 * 5.0
    dist = lambda got: rg.block_distances(np.abs(got), np.abs(g), "mlp", c.O, c.A, c.H, 1, ATOL)  # noqa: E731
    o32 = largest(dist(a2c_loss_grad(p, o[:-1].reshape(B, c.O), c.actions.reshape(B, c.A), c.returns[:-1].reshape(B), dims, rg.VCOEF,
                                     c.entropy_coef, np.float32)[1]) for p, o in jitters(c.seed, 77, [c.params, c.obs], rg.JITTERS))
    p = family_ppo.make_policy(sg, c)
    agent = sg.algo.A2C_ACKTR(p, rg.VCOEF, c.entropy_coef, lr=7e-4, eps=rg.EPS, alpha=0.99, max_grad_norm=5.0)
    got_losses = agent.update(family_ppo.make_rollout(sg, c))
    sq, _ = agent.get_rmsprop()
    hold(dist(np.sqrt(np.asarray(sq, np.float64) / 0.01)), o32, family_ppo, f"A2C {c.tag}")
    assert_close(got_losses, losses, what="losses")


def test_symmetry_step_against_autograd(sg, monkeypatch):
    """mixed (5, 2, 8), dense mirrors, 77 rows: the symmetry term and the PPO term of equal weight, M_a neither symmetric nor an
    involution, (M_a mu(s)).detach()"""
    family_sym.set_env(monkeypatch, {})
    c = sr.case("mixed", 5, 2, 8, "dense", 77)
    g, losses = ar.sym_case_grad(c, True)
    dist = lambda got: rg.block_distances(got, g, "mlp", c.O, c.A, c.H, 1, ATOL)  # noqa: E731
    o32 = largest(dist(sr.grad32(c, True, *j)) for j in jitters(c.seed, 79, [c.params, c.obs, c.mrows], rg.JITTERS))
    agent, got_losses, m, v = family_sym.one_step(sg, c, True)
    hold(dist(m.astype(np.float64) / 0.1), o32, family_sym, f"symmetry {c.tag}")
    vd = rg.block_distances(np.sqrt(v.astype(np.float64) / 0.001), np.abs(g), "mlp", c.O, c.A, c.H, 1, ATOL)
    assert max(vd.values()) <= RTOL, vd
    ca = rg.Case(c)
    ca["sym_loss"] = float(losses[3])          # the family's own check, against autograd's mean(e^2)
    family_sym.hold_symmetry_loss(agent, ca, f"symmetry {c.tag}")
    assert_close(got_losses, losses[:3], what="losses")
