"""GPU: the recurrent CNN base's PPO step past one row tile, one scan tile and one loss block.  Every gradient case of
tests/test_gpu_cnn_gru.py is one workgroup of everything (35 step rows at the most, 7 environments).  The cases of
cnn_gru_ref.TILE_CASES reach, in cnn_gru_ppo_update (simgan_amd/csrc/sg_ppo.hip):
  8 x 33, M = 1            264 rows: three scan workgroups (the last with one live environment), KS = 2 with ragged ranges over
                           padding rows and the three loss sums picked up behind the flat block, two blocks of k_cnn_head_loss,
                           the LDS-weight k_gru_dx on a grid of 5
  4 x 34, M = 2            per = 17: step 1 reads perm + 17, h0 rows 17 .. and rollout rows through k_cnn_gru_index, none at a
                           multiple of 16; two scan workgroups; k_gru_dx with a real grid stride (SG_POLICY_GW=1: a grid of 5)
  4 x 17 Box(3), Hs = 20   Hp = Op = 32 against the unpadded [mb][20] matrices F and dZf, over two k_gru_dx and two scan workgroups;
                           the Gaussian head's dls past one row tile
  3 x 6, Hs = 512          the global-weight instances by size at two row tiles, the second with 2 live rows
tests/test_cnn_gru_tiles_host.py restates the launcher's arithmetic, holds every case to its edge, admits every seed on the
references alone and shows that four defects of exactly these launches are invisible to the older cases.

  1 gradient    Adam's first moment after one epoch at lr = 0 per parameter block against float64 autograd within RTOL: clipped
                and plain value loss, the clip out of reach and at cnn_gru_ref.TILE_CLIP; the narrow cases again under
                SG_POLICY_GW=1
  2 update      E = 2, M = 2 on 4 x 34 against torch.optim.Adam's arithmetic in float64
  3 same bits   two runs, a graph replay and SG_PPO_GRAPH=0 on 4 x 34 and 8 x 33: no sum here depends on the grid's schedule
  4 forward     evaluate_actions at 33 environments and at Hs = 20 with 17 against float64; T chained one-step calls, bit for bit
SG_CNN_GRU_RECORD=<path> collects the measured worst block per gradient run (profiles/cnn_gru_parity.json)."""
import functools

import numpy as np
import pytest
import torch

import cnn_gru_ref as gr
import cnn_ref as cr
from helpers import RTOL, assert_close, assert_close_adam
from test_gpu_cnn_gru import LR, _record, adam_update64, agent_for, bits, make_policy, npv, reference_moment, rollout_of

pytestmark = pytest.mark.gpu

CAT33, CAT34, BOX17, WIDE6 = list(gr.TILE_CASES)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def _launch(monkeypatch, gw):
    if gw:
        monkeypatch.setenv("SG_POLICY_GW", "1")      # the global-weight instances of the GRU kernels, k_gru_dx's included
    else:
        monkeypatch.delenv("SG_POLICY_GW", raising=False)


def step_perm(key):
    return np.random.default_rng(gr.PERM_SEED).permutation(key[5]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def reference(key, max_grad_norm, use_clipped):
    """reference_moment, once per (case, clip, value loss): the SG_POLICY_GW=1 run shares the default launch's"""
    return reference_moment(gr.case(*key), key, gr.TILE_CASES[key], step_perm(key), max_grad_norm, use_clipped)


# ------------------------------------------------------------------------------------------------- 1 one-step gradient
TILE_RUNS = [(key, at_clip, clipped, False) for key in gr.TILE_CASES for clipped in (True, False) for at_clip in (False, True)] + \
            [(key, False, True, True) for key in gr.TILE_CASES if key[1] <= 20]


@pytest.mark.parametrize("key,at_clip,use_clipped,gw", TILE_RUNS,
                         ids=[f"{'-'.join(map(str, k))}-{'tileclip' if a else 'noclip'}-{'clipped' if u else 'plain'}{'-gw' if g else ''}"
                              for k, a, u, g in TILE_RUNS])
def test_one_step_gradient_per_block_past_one_tile(sg, monkeypatch, key, at_clip, use_clipped, gw):
    _launch(monkeypatch, gw)
    c, M = gr.case(*key), gr.TILE_CASES[key]
    max_grad_norm = gr.TILE_CLIP[key] if at_clip else 1e9
    perm = step_perm(key)
    if M > 1:      # the two minibatches are not the rollout's own halves, and every environment of step 1 comes through perm + per
        assert set(perm[:c.N // M]) != set(range(c.N // M))
    ref, ref_losses, factors = reference(key, max_grad_norm, use_clipped)
    assert len(factors) == M and (all(f < 1.0 for f in factors) if at_clip else all(f == 1.0 for f in factors))
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = agent_for(sg, c, p, 1, M, max_grad_norm, use_clipped, lr=0.0)
    losses = agent.update(rollout_of(sg, c), perms=perm[None])
    m, v, step = agent.get_adam()
    assert step == M and np.array_equal(agent.last_perms(), perm[None])
    assert np.array_equal(p.get_flat_params(), c.params)
    d = cr.block_distances(m, ref, c.shapes)
    print(c.tag, "worst block / RTOL", max(d.values()) / RTOL, "losses", list(losses), "float64", list(ref_losses))
    _record(f"gradient {c.tag} M={M} max_grad_norm={max_grad_norm:g} {'clipped' if use_clipped else 'plain'}{' gw' if gw else ''}",
            {"worst": max(d.values()) / RTOL, "blocks": {k: x / RTOL for k, x in d.items()}})
    assert_close(losses, ref_losses, what="losses")
    bad = {k: x for k, x in d.items() if not x <= RTOL}
    assert not bad, f"{c.tag}: blocks past {RTOL:g}: {bad}"


# ------------------------------------------------------------------------------------------------- 2 the whole update
def epoch_perms(key, E):
    return np.stack([np.random.default_rng([gr.PERM_SEED, e]).permutation(key[5]) for e in range(E)]).astype(np.int64)


def test_whole_update_of_two_steps_of_seventeen_environments(sg, monkeypatch):
    _launch(monkeypatch, False)
    key = CAT34
    c, E, M = gr.case(*key), 2, 2
    perms = epoch_perms(key, E)
    ref_losses, ref_params, steps = adam_update64(c, key, perms, E, M, gr.TILE_CLIP[key])
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    agent = agent_for(sg, c, p, E, M, gr.TILE_CLIP[key])
    losses = agent.update(rollout_of(sg, c), perms=perms)
    assert agent.get_adam()[2] == steps == 4 and np.array_equal(agent.last_perms(), perms)
    assert_close(losses, ref_losses, what="losses")
    assert_close_adam(p.get_flat_params(), ref_params, LR, steps, what="params after the update")


# ------------------------------------------------------------------------------------------------- 3 the same bits
@pytest.mark.parametrize("key", [CAT34, CAT33], ids=["4x34-M2", "8x33-M1"])
def test_two_runs_and_graph_replay_give_the_same_bits_past_one_tile(sg, monkeypatch, key):
    """More than one workgroup of k_gru_dx and of the scans, and (8 x 33) two KS partials feeding k_gru_reduce's sum: the order of
    every sum is the grid's own, so a fresh run, a replay of the captured graph and the uncaptured launch sequence agree bit for bit"""
    _launch(monkeypatch, False)
    c, M = gr.case(*key), gr.TILE_CASES[key]
    perms = epoch_perms(key, 1)
    out = []
    for graph in ("1", "1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
        agent = agent_for(sg, c, p, 1, M, gr.TILE_CLIP[key])
        ro = rollout_of(sg, c)
        losses = [agent.update(ro, perms=perms) for _ in range(2)]      # (the second update of a graph run is a replay)
        out.append((losses, p.get_flat_params(), *agent.get_adam()[:2]))
    for other in out[1:]:
        assert other[0] == out[0][0]
        for a, b in zip(out[0][1:], other[1:]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isfinite(out[0][1]).all() and np.abs(out[0][1] - c.params).max() > 1e-4


# ------------------------------------------------------------------------------------------------- 4 forward at the new widths
@pytest.mark.parametrize("key", [CAT33, BOX17], ids=["8x33", "4x17-Hs20"])
def test_forward_matches_float64_and_chained_steps_give_the_same_bits(sg, monkeypatch, key):
    _launch(monkeypatch, False)
    c = gr.case(*key)
    T, n = c.T, c.N
    r = gr.rows_of(c)
    obs, hxs, masks, acts = r["obs"], r["hxs0"], r["masks"], r["actions"]
    p = make_policy(sg, c.C, c.Hs, c.dist, c.P, c.params)
    with torch.no_grad():
        rv, rlp, rent, rh = gr.evaluate(cr.leaves(c.params, c.shapes), cr.ar.t64(obs), hxs, masks, T, acts, c.dist)
    v, lp, ent, hT = p.evaluate_actions(obs, hxs, masks.reshape(-1, 1), acts)
    assert tuple(v.shape) == (T * n, 1) and tuple(lp.shape) == (T * n, 1) and tuple(hT.shape) == (n, c.Hs)
    assert_close(npv(v), rv.numpy(), what="value")
    assert_close(npv(lp), rlp.numpy(), what="logp")
    assert_close(npv(ent), rent.numpy(), what="entropy")
    assert_close(npv(hT), rh.numpy(), what="final hidden state")
    h, vs, lps = hxs, [], []
    for t in range(T):
        sl = slice(t * n, (t + 1) * n)
        v1, lp1, _, h = p.evaluate_actions(obs[sl], h, masks[sl].reshape(-1, 1), acts[sl])
        vs.append(npv(v1))
        lps.append(npv(lp1))
    assert np.array_equal(bits(np.concatenate(vs)), bits(v)), "values: a sequence and its chained steps differ"
    assert np.array_equal(bits(np.concatenate(lps)), bits(lp)), "log-probs: a sequence and its chained steps differ"
    assert np.array_equal(bits(h), bits(hT)), "final hidden state: a sequence and its chained steps differ"
