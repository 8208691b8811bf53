"""GPU: the CNN base (csrc/sg_cnn_kernels.hpp, sg_cnn.hip, the CNN paths of sg_ppo.hip) off the regime of tests/cnn_ref.py's six
cases -- tests/cnn_regimes.py's: peaked and one-class Categorical heads, sigmas from e^-2 to e, Hs = 18 / 40 / 512, 41 and 513
rows, every clip branch past one block of rows, ReLU pre-activations at exactly 0.  tests/test_cnn_regimes_host.py proves on the
CPU that every case keeps clear of the ReLU kinks and the branch boundaries, that float32 torch holds it within half the bound,
and which injected defects only these cases see.  Nothing here searches.

  1 PPO       one optimizer step read back from Adam's m, per parameter block against float64 autograd within RTOL, the clip out
              of reach and at max_grad_norm = 0.5; the clipped value loss for every case, the plain one for three
  2 A2C       the same through RMSprop's square_avg, at the default chunk and with a ragged last chunk of one row
  3 forward   evaluate_actions, get_value, act (mode, and with injected noise) against float64; sampled classes exact
  4 gather    E = 1, M = 3 over 513 permuted rows at lr = 0
  5 bits      the graph replay against direct launches on 41 rows (conv1 at its slab cap)
Wherever torch's gradient is exactly 0 in float64 and in float32 (units ReLU switches off in every row, units AT 0 included) the
library's must be exactly 0 too.  The bound is helpers.RTOL / ATOL through cr.block_distances and assert_close, for every case.
SG_CNN_RECORD=<path> collects the measured distances (profiles/cnn_regimes_parity.json)."""
import json
import os

import numpy as np
import pytest
import torch

import cnn_ref as cr
import cnn_regimes as rg
import test_gpu_a2c_cnn as ta
import test_gpu_cnn as tc
from helpers import RTOL, assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def _record(label, rec):
    path = os.environ.get("SG_CNN_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_cnn_regimes.py under SG_CNN_RECORD: per case of tests/cnn_regimes.py the one-step gradient's "
                       "rel-L2 distance (tests/cnn_ref.py:block_distances) to float64 autograd per parameter block over RTOL = 1e-4, "
                       "for PPO (from Adam's m) and A2C (from RMSprop's square_avg), with the float32 torch gradient's worst block "
                       "beside it; forward values element by element over ATOL + RTOL |ref|", "cases": {}}
    doc["cases"][label] = rec
    doc["worst"] = max(r["worst"] for r in doc["cases"].values())
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def _zeros_hold(got, tag, algo, use_clipped=True):
    idx = rg.exact_zero_elements(tag, algo, use_clipped)
    bad = idx[np.asarray(got)[idx] != 0]
    assert bad.size == 0, f"{tag} {algo}: {bad.size} of {idx.size} elements that are exactly 0 in torch are not (first {bad[:5]})"
    return int(idx.size)


# ------------------------------------------------------------------------------------------------- 1 PPO, one step per block
PPO_RUNS = ([(t, m, True) for t in rg.TAGS for m in (1e9, 0.5)] + [(t, m, False) for t in rg.PLAIN_TAGS for m in (1e9, 0.5)])


@pytest.mark.parametrize("tag,max_grad_norm,use_clipped", PPO_RUNS, ids=[f"{t}-clip{m:g}-{'clipped' if u else 'plain'}" for t, m, u in PPO_RUNS])
def test_ppo_one_step_gradient_per_block(sg, tag, max_grad_norm, use_clipped):
    ref, ref_losses, d32, _ = rg.admitted(tag, "ppo", use_clipped)
    assert max(d32.values()) <= 0.5 * RTOL, f"{tag}: float32 torch is {max(d32.values()):.2e} from float64: not a case"
    c = rg.case(tag)
    m, losses, _ = tc.one_step(sg, c, max_grad_norm, use_clipped, ecoef=c.ecoef)
    got = m.astype(np.float64) / (1.0 - 0.9)
    factor = cr.clip_factor(ref, max_grad_norm)
    assert factor == 1.0 if max_grad_norm > 1.0 else factor <= 1.0
    d = cr.block_distances(got, ref * factor, c.shapes)
    label = f"ppo {tag} max_grad_norm={max_grad_norm:g} {'clipped' if use_clipped else 'plain'} value loss"
    print(f"{label}: clip factor {factor:.4f}, worst block {max(d, key=d.get)} {max(d.values()) / RTOL:.3f} x RTOL "
          f"(float32 torch {max(d32.values()) / RTOL:.3f}), losses {tc.ratio(losses, ref_losses):.3f} of tol")
    _record(label, {"clip_factor": factor, "worst": max(d.values()) / RTOL, "float32_torch_worst": max(d32.values()) / RTOL,
                    "blocks": {k: x / RTOL for k, x in d.items()}, "losses": tc.ratio(losses, ref_losses)})
    assert_close(losses, ref_losses, what=f"{label} losses")
    bad = {k: x for k, x in d.items() if not x <= RTOL}
    assert not bad, f"{label}: blocks past {RTOL:g}: {bad}"
    n_zero = _zeros_hold(got, tag, "ppo", use_clipped)
    if tag == "relu-zero":
        assert not got[rg.zero_unit_elements(c)].any() and n_zero >= rg.zero_unit_elements(c).size
    if tag == "one-class":      # K = 1: the one class has probability 1 whatever the logit is
        head = dict(cr.blocks(c.shapes, got))
        assert not head["dist.linear.weight"].any() and not head["dist.linear.bias"].any() and losses[2] == 0.0


# ------------------------------------------------------------------------------------------------- 2 A2C, one step per block
def _a2c(sg, tag, label):
    want, want_losses, d32, _ = rg.admitted(tag, "a2c")
    assert max(d32.values()) <= 0.5 * RTOL, f"{tag}: float32 torch is {max(d32.values()):.2e} from float64: not a case"
    c = rg.case(tag)
    got = ta.hold_case(sg, c, label, want=(want, want_losses), record=_record, entropy_coef=c.ecoef)
    _zeros_hold(got, tag, "a2c")
    return c, got


@pytest.mark.parametrize("tag", rg.A2C_TAGS)
def test_a2c_one_step_gradient_per_block(sg, tag):
    c, got = _a2c(sg, tag, f"a2c {tag}")
    if tag == "relu-zero":
        assert not got[rg.zero_unit_elements(c)].any()
    if tag == "one-class":
        head = dict(cr.blocks(c.shapes, got))
        assert not head["dist.linear.weight"].any() and not head["dist.linear.bias"].any()


@pytest.mark.parametrize("tag,chunk", rg.A2C_CHUNKS, ids=[f"{t}-chunk{k}" for t, k in rg.A2C_CHUNKS])
def test_a2c_gradient_in_row_chunks(sg, monkeypatch, tag, chunk):
    monkeypatch.setenv("SG_A2C_CNN_CHUNK_ROWS", str(chunk))
    c, _ = _a2c(sg, tag, f"a2c {tag} chunk {chunk}")
    assert c.T * c.N % chunk == 1


# ------------------------------------------------------------------------------------------------- 3 forward
@pytest.mark.parametrize("tag", rg.FORWARD_TAGS)
def test_forward_matches_float64(sg, tag):
    c = rg.case(tag)
    r = cr.rows_of(c)
    obs, n, cat = r["obs"], c.T * c.N, c.dist == "categorical"
    p = tc.make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    acts = r["actions"].astype(np.int64) if cat else r["actions"].astype(np.float32)
    with torch.no_grad():
        rv, rlp, rent = cr.evaluate(cr.leaves(c.params, c.shapes), cr.ar.t64(obs), acts, c.dist)
    v, lp, ent, _ = p.evaluate_actions(obs, None, None, acts)
    assert tuple(v.shape) == (n, 1) and tuple(lp.shape) == (n, 1)
    rec = {"evaluate": max(tc.ratio(tc.npv(v), rv.numpy()), tc.ratio(tc.npv(lp), rlp.numpy()), tc.ratio(tc.npv(ent), rent.numpy()))}
    assert_close(tc.npv(v), rv.numpy(), what="value")
    assert_close(tc.npv(lp), rlp.numpy(), what="logp")      # (peaked: rows whose taken class has log-prob <= -4 among them)
    assert_close(tc.npv(ent), rent.numpy(), what="entropy")
    if c.head == "peaked":
        assert (rlp.numpy() <= -4.0).sum() >= 2
    assert_close(tc.npv(p.get_value(obs, None, None)), rv.numpy(), what="get_value")
    det = cr.act64(c.shapes, c.params, obs, c.dist)
    v, a, lp, _ = p.act(obs, None, None, deterministic=True)
    if cat:
        assert np.array_equal(tc.npv(a).reshape(-1), det["action"])
    else:
        assert_close(tc.npv(a), det["action"], what="mode")
    assert_close(tc.npv(v), det["value"], what="value from act")
    assert_close(tc.npv(lp), det["logp"], what="logp of the mode")
    rec["act_deterministic"] = max(tc.ratio(tc.npv(v), det["value"]), tc.ratio(tc.npv(lp), det["logp"]))
    noise = c.uniform.reshape(n, 1) if cat else c.noise
    smp = cr.act64(c.shapes, c.params, obs, c.dist, c.uniform if cat else c.noise)
    v, a, lp, _ = p.act(obs, None, None, noise=noise)
    if cat:
        assert smp["margin"] >= rg.SAMPLE_MARGIN and np.array_equal(tc.npv(a).reshape(-1), smp["action"])
    else:
        assert_close(tc.npv(a), smp["action"], what="sampled action")
    assert_close(tc.npv(lp), smp["logp"], what="logp of the draw")
    assert_close(tc.npv(v), smp["value"], what="value")
    rec["act_sampled"] = max(tc.ratio(tc.npv(lp), smp["logp"]), tc.ratio(tc.npv(v), smp["value"]))
    rec["worst"] = max(rec.values())
    _record(f"forward {tag}", rec)


# ------------------------------------------------------------------------------------------------- 4 the minibatch gather
def test_three_minibatches_are_exactly_the_permuted_rows(sg):
    c = rg.case(rg.GATHER_TAG)
    want, parts, perm = rg.gather_reference(c)
    # lr = 0: the parameters stay put, so every step's gradient is autograd's at the same parameters
    m, _, p = tc.one_step(sg, c, 1e9, True, perms=perm[None], E=1, M=rg.GATHER_M, lr=0.0, ecoef=c.ecoef)
    assert np.array_equal(p.get_flat_params(), c.params)
    d = cr.block_distances(m, want, c.shapes)
    _record(f"gather {rg.GATHER_TAG} M={rg.GATHER_M}", {"worst": max(d.values()) / RTOL, "blocks": {k: x / RTOL for k, x in d.items()}})
    assert max(d.values()) <= RTOL, d


# ------------------------------------------------------------------------------------------------- 5 determinism
def test_graph_replay_and_direct_launches_give_the_same_bits_at_the_slab_cap(sg, monkeypatch):
    c = rg.case("rows-41")
    B = c.T * c.N
    perms = np.arange(B, dtype=np.int64)[None]
    out = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        p = tc.make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
        agent = sg.algo.PPO(p, cr.CLIP, 1, 1, cr.VCOEF, c.ecoef, lr=cr.LR, eps=cr.EPS, max_grad_norm=0.5)
        ro = tc.rollout_of(sg, c)
        losses = [agent.update(ro, perms=perms) for _ in range(2)]      # (the second update of a graph run is a replay)
        out.append((losses, p.get_flat_params(), *agent.get_adam()[:2]))
    for other in out[1:]:
        assert other[0] == out[0][0]
        for a, b in zip(out[0][1:], other[1:]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(out[0][1]).all() and np.abs(out[0][1] - c.params).max() > 1e-4


def test_a2c_graph_replay_and_direct_launches_give_the_same_bits_in_chunks_of_40(sg, monkeypatch):
    monkeypatch.setenv("SG_A2C_CNN_CHUNK_ROWS", "40")      # 40 + 1 rows: an accumulating pass of one row inside the graph
    c = rg.case("rows-41")
    out = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        agent, p, losses = ta._run(sg, c, updates=2)
        out.append((losses, p.get_flat_params(), agent.get_rmsprop()[0]))
    for other in out[1:]:
        assert out[0][0] == other[0]
        assert np.array_equal(out[0][1].view(np.uint32), other[1].view(np.uint32))
        assert np.array_equal(out[0][2].view(np.uint32), other[2].view(np.uint32))
    assert np.isfinite(out[0][1]).all() and np.abs(out[0][1] - c.params).max() > 1e-4
