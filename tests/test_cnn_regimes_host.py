"""CPU: every case of tests/cnn_regimes.py re-proved on the references alone, and the test of the test.

  conditions  per case: every ReLU pre-activation of the float64 forward at least KINK_FACTOR x the float32 forward's error from
              zero (exempt only where both forwards give exactly 0, and only in "relu-zero"), every row MARGIN from a branch
              boundary, "branches" with every class populated, the head regime's condition, the paths the case is there to reach
              (csrc/sg_cnn.hip's slab arithmetic restated)
  admission   torch's float32 CPU gradient within 0.5 RTOL of the float64 one in every block, PPO (both value losses where the
              GPU file runs both) and A2C
  faults      each kept fault stays within RTOL (here: leaves the gradient unchanged) on every old case of cr.GRAD_CASES with more
              than one row -- the gap written down -- and passes 10 RTOL in some block of its new case

Faults dropped because an old case already sees them (distance of the faulty gradient over RTOL, worst block, measured here):
  ent_at_uniform   10.5 / 6.2 / 45.1 on the 1x3, 17x1 and "branches" Categorical cases: at gain 0.01 the probabilities lie within
                   [0.173, 0.249], and an entropy gradient of that size is already 6 to 45 RTOL of dist.linear's blocks
  sigma_unit       299 on the Gaussian case (3x5): its sigmas lie within 3 % of 1, so 1 / var differs from 1 by up to 6 %
Both stay in cnn_regimes.fault_grad, and a test below holds that the old cases do see them, so this paragraph cannot go stale.
"peaked-ent" and "sigma-17" remain as cases: they put those terms where they lead (the faults' distances there are 8100 and
16000 RTOL)."""
import numpy as np
import pytest
import torch

import cnn_ref as cr
import cnn_regimes as rg
from helpers import ATOL, RTOL

OLD = [k for k in cr.GRAD_CASES if k[4] * k[5] > 1]


@pytest.mark.parametrize("tag", rg.TAGS)
def test_case_meets_its_conditions(tag):
    c = rg.case(tag)
    ok, km, exempted, classes, margins = rg.acceptable(c)
    assert km >= cr.KINK_FACTOR, f"{tag}: a ReLU pre-activation lies {km:.2f} x the float32 forward's error from zero"
    assert ok, (tag, km, exempted, classes, margins)
    if c.regime == "branches":
        assert min(classes.values()) >= 1, classes
        assert min(classes[k] for k in ("above_adv+", "above_adv-", "below_adv+", "below_adv-", "u>w", "w>u_outside")) >= 2
    assert rg.head_holds(c), rg.head_facts(c)
    if c.head == "relu_zero":
        # exactly 0 in both forwards: 8 channels x 400 pixels of the two zero frames, 4 FC units in all four rows -- and nothing else
        assert exempted == len(rg.ZERO_FRAMES) * rg.ZERO_CHANNELS * 400 + rg.ZERO_UNITS * c.T * c.N
        assert not cr.rows_of(c)["obs"][list(rg.ZERO_FRAMES)].any()
        biases = np.concatenate([b for name, b in cr.blocks(c.shapes, c.params) if name.endswith(".bias")])
        assert int((biases == 0).sum()) == rg.ZERO_CHANNELS + rg.ZERO_UNITS and np.abs(biases[biases != 0]).min() >= rg.BIAS_CLEAR
    else:
        assert exempted == 0 and cr.kink_margin(c.shapes, c.params, cr.rows_of(c)["obs"]) >= cr.KINK_FACTOR


def test_the_cases_reach_the_paths_they_are_there_for():
    n = {t: rg.case(t).T * rg.case(t).N for t in rg.TAGS}
    # conv1 reaches the 32-slab cap from 41 images, with 516 rows per slab: slab edges fall inside an image
    assert rg.slab_arithmetic(40)["conv1"][1] == 32 and 40 * 400 <= 32 * 512 < 41 * 400
    assert rg.slab_arithmetic(n["rows-41"])["conv1"] == (16400, 32, 516) and 516 % 400
    assert rg.slab_arithmetic(27)["conv1"][1] < 32      # the largest old case never reached the cap
    # 513 rows: every layer capped, the FC layer in 2 slabs (1 until n > 512), the loss kernels in 3 blocks of 256 rows
    s = rg.slab_arithmetic(n["rows-513"])
    assert [s[k][1] for k in ("conv1", "conv2", "conv3", "fc")] == [32, 32, 32, 2] and s["fc"][2] == 260
    assert rg.slab_arithmetic(512)["fc"][1] == 1 and (n["rows-513"] + 255) // 256 == 3 and n["branches-513"] == 513
    for tag, chunk in rg.A2C_CHUNKS:
        assert n[tag] % chunk == 1      # a ragged last chunk of one row
    assert n[rg.GATHER_TAG] % rg.GATHER_M == 0
    c = rg.case("peaked-18")
    assert c.P > 16 and np.array_equal(c.actions.reshape(-1)[:2], cr.forward64(c.shapes, c.params, cr.rows_of(c)["obs"][:2], c.dist)[1].argmax(1))
    c = rg.case("sigma-17")
    assert c.Hs % 4 == 2 and c.P > 16      # the K tail of the FC layer's data gradient; head stacks 32 wide
    c = rg.case("hs-40")
    assert (c.Hs + 15) // 16 == 3 and c.Hs % 16 == 8 and (c.Hs + 31) // 32 == 2      # a ragged third row tile of co, a second column tile
    c = rg.case("default")
    assert (c.C, c.Hs, c.P) == (4, 512, 6) and ((c.P + 1) * (c.Hs + 1) + 255) // 256 == 15      # k_cnn_head_wgrad's 15 blocks
    c = rg.case("one-class")
    g, _ = rg.admitted("one-class")[:2]
    head = dict(cr.blocks(c.shapes, g))
    assert c.P == 1 and not head["dist.linear.weight"].any() and not head["dist.linear.bias"].any()      # exactly 0 in the reference
    assert rg.case("peaked-ent").ecoef == 1.0 and np.array_equal(rg.case("peaked-ent").params, rg.case("peaked-18").params)
    assert np.array_equal(rg.case("branches-513").obs, rg.case("rows-513").obs)


@pytest.mark.parametrize("tag", rg.FORWARD_TAGS)
def test_forward_cases_keep_their_draws_clear_of_the_boundaries(tag):
    c = rg.case(tag)
    obs = cr.rows_of(c)["obs"]
    det = cr.act64(c.shapes, c.params, obs, c.dist)
    if c.dist == "categorical":
        smp = cr.act64(c.shapes, c.params, obs, c.dist, c.uniform)
        assert det["margin"] > 1e-3 and smp["margin"] >= rg.SAMPLE_MARGIN
        if c.head == "peaked":
            assert (smp["logp"] <= -4.0).any() or (cr.rows_of(c)["actions"].reshape(-1) != det["action"]).any()
    else:
        assert c.noise.shape == (c.T * c.N, c.P)


ADMISSIONS = ([(t, "ppo", True) for t in rg.TAGS] + [(t, "ppo", False) for t in rg.PLAIN_TAGS] + [(t, "a2c", True) for t in rg.A2C_TAGS])


@pytest.mark.parametrize("tag,algo,use_clipped", ADMISSIONS, ids=[f"{t}-{a}-{'clipped' if u else 'plain'}" for t, a, u in ADMISSIONS])
def test_float32_torch_holds_the_case(tag, algo, use_clipped):
    g64, _, d32, _ = rg.admitted(tag, algo, use_clipped)
    assert np.isfinite(g64).all()
    print(f"{tag} {algo}: float32 torch worst block {max(d32, key=d32.get)} {max(d32.values()) / RTOL:.3f} x RTOL")
    assert max(d32.values()) <= 0.5 * RTOL, (tag, algo, {k: v for k, v in d32.items() if v > 0.5 * RTOL})


def test_the_zero_units_have_gradient_exactly_zero_in_torch():
    c = rg.case("relu-zero")
    idx = rg.zero_unit_elements(c)
    for algo in ("ppo", "a2c"):
        g64 = rg.admitted("relu-zero", algo)[0]
        g32 = (rg.ppo_grad if algo == "ppo" else rg.a2c_grad)(c, dtype=torch.float32)[0]
        assert not g64[idx].any() and not g32[idx].any() and idx.size == rg.ZERO_UNITS * (cr.num_params(c.shapes[6:7]) // c.Hs + 1)
        assert np.isin(idx, rg.exact_zero_elements("relu-zero", algo)).all()
    # conv1's channels with bias 0: most have a gradient from the two frames that are not zero; those that are dead on these two
    # frames as well have bias gradient exactly 0 in torch, which only derivative 0 AT 0 (the zero frames) keeps.  relu_ge moves
    # all eight, and nothing else of that block
    b1 = dict(cr.blocks(c.shapes, rg.admitted("relu-zero")[0]))["base.main.0.bias"]
    lo = cr.num_params(c.shapes[:1])
    dead = [k for k in range(rg.ZERO_CHANNELS) if lo + k in rg.exact_zero_elements("relu-zero", "ppo")]
    assert dead and all(b1[k] == 0 for k in dead) and len(dead) < rg.ZERO_CHANNELS
    bad = dict(cr.blocks(c.shapes, rg.fault_grad(c, "relu_ge")[0]))["base.main.0.bias"]
    assert np.abs(bad[:rg.ZERO_CHANNELS] - b1[:rg.ZERO_CHANNELS]).min() > 10 * RTOL * np.abs(b1).max()
    assert np.array_equal(bad[rg.ZERO_CHANNELS:], b1[rg.ZERO_CHANNELS:])


def _distances(c, fault, good=None):
    good, good_losses = rg.ppo_grad(c) if good is None else good
    bad, bad_losses = rg.fault_grad(c, fault)
    loss_ratio = float(np.max(np.abs(bad_losses - good_losses) / (ATOL + RTOL * np.abs(good_losses))))
    return cr.block_distances(bad, good, c.shapes), loss_ratio


@pytest.mark.parametrize("fault", list(rg.FAULTS))
def test_fault_is_invisible_to_the_old_cases_and_seen_by_its_new_case(fault):
    for key in OLD:
        d, losses = _distances(rg.old_case(key), fault)
        assert max(d.values()) <= RTOL and losses <= 1.0, (fault, key, d)
    tag = rg.FAULTS[fault]
    d, losses = _distances(rg.case(tag), fault, rg.admitted(tag)[:2])
    print(f"{fault} on {tag}: worst block {max(d, key=d.get)} {max(d.values()) / RTOL:.1f} x RTOL, losses {losses:.1f} of tol")
    assert max(d.values()) > 10 * RTOL, (fault, tag, d)
    if fault == "rows_first_256":
        assert losses > 10.0      # the three loss sums are compared with assert_close
    if fault == "k_tail":         # the FC layer's own blocks and the heads keep their gradient: only the data gradient is hit
        assert max(v for k, v in d.items() if not k.startswith("base.main.") or k.startswith("base.main.7")) == 0.0


@pytest.mark.parametrize("fault", list(rg.DROPPED))
def test_dropped_fault_is_already_seen_by_an_old_case(fault):
    worst = max(max(_distances(rg.old_case(key), fault)[0].values()) for key in OLD)
    assert worst > RTOL, (fault, worst)
    tag = rg.DROPPED[fault]
    assert max(_distances(rg.case(tag), fault, rg.admitted(tag)[:2])[0].values()) > 10 * RTOL


def test_the_gather_parts_differ_and_their_order_shows():
    """the arithmetic tests/test_gpu_cnn_regimes.py's gather test rests on: three parts of 171 permuted rows, weights 0.081,
    0.09, 0.1 -- parts swapped, or rows in rollout order, are more than 10 RTOL away"""
    c = rg.case(rg.GATHER_TAG)
    want, parts, perm = rg.gather_reference(c)
    assert perm.size == 513 and sorted(perm[:171]) != list(range(171))
    w = rg.GATHER_WEIGHTS
    assert max(cr.block_distances(w[0] * parts[1] + w[1] * parts[0] + w[2] * parts[2], want, c.shapes).values()) > 10 * RTOL
    plain = [rg.ppo_grad(c, rows=np.arange(k * 171, (k + 1) * 171))[0] for k in range(3)]
    assert max(cr.block_distances(sum(wk * g for wk, g in zip(w, plain)), want, c.shapes).values()) > 10 * RTOL
