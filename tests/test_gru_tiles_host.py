"""CPU: the cases of regimes.GRU_TILE_CASES / GRU_STEPS_CASE (tests/test_gpu_gru_tiles.py runs them on the GPU), judged without the
library: the launch arithmetic of the recurrent update (simgan_amd/csrc/sg_ppo.hip, gru_ppo_update, and k_gru_wgrad in
sg_gru_kernels.hpp) is restated here and every case is held to the fact it was chosen for, so a change to the launcher that moves
a case off its edge fails here instead of silently emptying the GPU test; and on the float64 restatement (tests/gru_ref.py) a
reverse scan that loses every environment past the first 16-environment workgroup is shown to be invisible to every older
recurrent case and far outside the contract on the new ones."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import gru_ref  # noqa: E402
import regimes as rg  # noqa: E402
from helpers import ATOL, RTOL, load  # noqa: E402

TILE = 16   # environments per workgroup of k_gru_scan_fwd / k_gru_scan_bwd; rows per chunk of k_gru_wgrad


def geometry(T, N, num_mini_batch=1):
    """gru_ppo_update's launch arithmetic: per, the scans' workgroups and the live rows of the last one, rows_p, the weight
    gradient's chunks, KS and the chunk range [c0, c1) of every blockIdx.y (k_gru_wgrad: c1 <= c0 is an empty range)."""
    per = N // num_mini_batch
    assert N % per == 0
    mb = T * per
    rows_p = (mb + 15) & ~15
    chunks = rows_p // TILE
    KS = max(1, min(16, chunks // 8))
    each = (chunks + KS - 1) // KS
    ranges = [(ks * each, min(chunks, ks * each + each)) for ks in range(KS)]
    return dict(per=per, steps=N // per, mb=mb, workgroups=(per + TILE - 1) // TILE, last_live=per - TILE * ((per - 1) // TILE),
                rows_p=rows_p, chunks=chunks, KS=KS, each=each, ranges=ranges, sizes=[max(0, c1 - c0) for c0, c1 in ranges])


def _lds(H):
    """bytes of k_gru_scan_fwd's and k_gru_scan_bwd's LDS-resident instances (sg_gru_scan_lds, sg_gru_bwd_lds) and the room the
    launcher compares them with (a gfx950 workgroup's 160 KiB less 1 KiB)"""
    Hp = (H + 15) & ~15
    ldH = Hp + 4
    return 4 * (3 * Hp * ldH + 2 * 16 * ldH), 4 * (3 * Hp * ldH + 16 * ldH + 16 * (3 * Hp + 4)), 160 * 1024 - 1024


# (shape, T, N) -> the facts the case exists for
FACTS = {(("gru", 11, 3, 32, 1), 8, 17): dict(workgroups=2, last_live=1, KS=1, sizes=[9], pad_rows=8),
         (("gru", 47, 12, 64, 1), 8, 17): dict(workgroups=2, last_live=1, KS=1, sizes=[9], pad_rows=8),
         (("gru", 13, 5, 100, 1), 8, 17): dict(workgroups=2, last_live=1, KS=1, sizes=[9], pad_rows=8),
         (("gru", 13, 5, 20, 1), 9, 33): dict(workgroups=3, last_live=1, KS=2, sizes=[10, 9], pad_rows=7),
         (("gru", 13, 5, 20, 1), 27, 48): dict(workgroups=3, last_live=16, KS=10, sizes=[9] * 9 + [0], pad_rows=0),
         (("gru", 47, 12, 64, 1), 27, 48): dict(workgroups=3, last_live=16, KS=10, sizes=[9] * 9 + [0], pad_rows=0),
         (("gru", 13, 5, 20, 1), 43, 48): dict(workgroups=3, last_live=16, KS=16, sizes=[9] * 14 + [3, 0], pad_rows=0)}
CASES = list(rg.GRU_TILE_CASES)
IDS = [f"{s[1]}x{s[2]}x{s[3]}-T{t}N{n}" for s, t, n in CASES]
OLD_GRU = [spec for spec in rg.all_cases() if spec[1] == "gru"]


def test_every_case_has_its_facts_and_every_edge_has_a_case():
    assert sorted(FACTS) == sorted(CASES)
    geo = [geometry(t, n) for _, t, n in CASES]
    assert all(g["workgroups"] > 1 for g in geo), "every case runs a workgroup other than block 0"
    assert any(g["last_live"] < TILE for g in geo) and any(g["last_live"] == TILE for g in geo)
    assert any(g["KS"] > 1 and len(set(s for s in g["sizes"] if s)) > 1 for g in geo), "a ragged last range"
    assert any(0 in g["sizes"] for g in geo), "an empty range"
    assert any(g["KS"] == 16 for g in geo), "the cap"
    assert any(g["KS"] > 1 and g["mb"] % TILE for g in geo), "KS > 1 on padding rows of dgi / dgh"
    assert any(s[3] == 64 and g["KS"] == 1 for (s, _, _), g in zip(CASES, geo)) and \
        any(s[3] == 64 and 0 in g["sizes"] for (s, _, _), g in zip(CASES, geo)), "the shipped width on both"


@pytest.mark.parametrize("spec,T,N", CASES, ids=IDS)
def test_case_sits_on_its_edge_of_the_launcher(spec, T, N):
    g, want = geometry(T, N), FACTS[(spec, T, N)]
    print(spec, T, N, g)
    assert g["per"] == N > TILE and g["steps"] == 1
    assert g["workgroups"] == want["workgroups"] > 1 and g["last_live"] == want["last_live"]
    assert g["KS"] == want["KS"] and g["sizes"] == want["sizes"] and sum(g["sizes"]) == g["chunks"]
    assert g["rows_p"] - g["mb"] == want["pad_rows"]
    # the ranges tile [0, chunks) in order; an empty one starts at or past the end (k_gru_wgrad must then read nothing)
    end = 0
    for c0, c1 in g["ranges"]:
        assert c0 == end or c1 <= c0, g["ranges"]
        end = max(end, c1)
    assert end == g["chunks"]
    scan, bwd, room = _lds(spec[3])
    if spec[3] == 100:   # the scans read W_hh through L2 by size (both of them), while the trunks on h stay in LDS
        assert scan > room and bwd > room
        Hp, ldH, Pp = 112, 116, 16   # (csrc/sg_policy_fwd.hpp: fwd_lds_bytes at MT = 1 -- the widest trunk's block beside one row tile)
        trunk = lambda ex: 2 * (Hp * ldH + Hp) + Pp * ldH + Pp + ex   # noqa: E731
        assert 4 * (max(trunk(16), trunk(0)) + 3 * 16 * ldH + 16 * (Pp + 4)) <= room
    else:
        assert scan <= room and bwd <= room


def test_the_two_step_case_reaches_the_offsets_of_step_1():
    spec, T, N = rg.GRU_STEPS_CASE
    g = geometry(T, N, 2)
    assert g["per"] == 17 and g["steps"] == 2 and g["workgroups"] == 2 and g["last_live"] == 1
    assert g["mb"] == 136 and g["mb"] % TILE == 8      # step 1 starts at row block 136 and at h0 + 17 H: neither is tile-aligned
    c = rg.case("off_policy", *spec, T=T, N=N)
    assert c.T == T and c.N == N and c.hxs0.shape == (N, spec[3])


def test_the_older_recurrent_updates_never_left_block_0():
    """every recurrent update the suite ran before: per <= 16, one workgroup, KS <= 4 with chunks dividing evenly"""
    for spec in OLD_GRU:
        assert geometry(rg.T, rg.N)["workgroups"] == 1
    for name in ("ppo_gru_tiny", "ppo_gru_hopper", "ppo_gru_laikago", "ppo_gru_long", "ppo_gru_onestep", "ppo_gru_onestep64"):
        m = load(name)["meta"]
        g = geometry(m["T"], m["N"], m["num_mini_batch"])
        assert g["workgroups"] == 1 and g["KS"] in (1, 4) and len(set(g["sizes"])) == 1 and g["sizes"][0] > 0, (name, g)
        assert g["KS"] == 1 or g["mb"] % TILE == 0, (name, g)


def grad_with_only_the_first_workgroup(c, use_clipped):
    """The float64 one-step gradient with the reverse scan run on environments [0, 16) only: the GRU's four tensors lose the terms of
    every later environment; the heads' blocks are untouched.  An environment's back-propagation through time does not see the
    others (the advantages are normalised beforehand and the losses are means over the T N rows), so the GRU blocks of the first
    16 environments are those of a 16-environment minibatch, its 1 / (16 T) turned back into 1 / (N T)."""
    B, keep = c.T * c.N, min(c.N, TILE)
    sd = gru_ref.unflatten(c.params, c.O, c.A, c.H)
    tm = lambda a: np.asarray(a).reshape(c.T, c.N, -1)[:, :keep].reshape(c.T * keep, -1)   # noqa: E731
    g, _ = gru_ref.minibatch_grad(sd, tm(c.obs[:-1]), c.hxs0[:keep], tm(c.masks[:-1])[:, 0], tm(c.actions), tm(c.action_log_probs)[:, 0],
                                  tm(rg.advantages64(c))[:, 0], tm(c.value_preds[:-1])[:, 0], tm(c.returns[:-1])[:, 0], rg.CLIP,
                                  rg.VCOEF, c.entropy_coef, use_clipped)
    part = gru_ref.flatten(g, c.O, c.A, c.H) * (keep / c.N)
    out = c.desc["grad_clipped" if use_clipped else "grad_plain"].copy()
    n_gru = sum(int(np.prod(s)) for name, s in gru_ref.param_shapes(c.O, c.A, c.H) if name.startswith("base.gru"))
    out[:n_gru] = part[:n_gru]
    assert B == c.T * c.N and n_gru == 3 * c.H * (c.O + c.H + 2)
    return out


@pytest.mark.parametrize("spec,T,N", CASES, ids=IDS)
def test_losing_the_later_workgroups_is_far_outside_the_contract(spec, T, N):
    """What a reverse scan with a wrong `base` would do at its mildest: on every new case at least one GRU block moves by more
    than 100 x the contract's 1e-4 (17 environments: one of them missing is ~1 / 17 of a block), under both value losses."""
    c = rg.case("off_policy", *spec, T=T, N=N)
    for uc in (True, False):
        ref = c.desc["grad_clipped" if uc else "grad_plain"]
        d = rg.block_distances(grad_with_only_the_first_workgroup(c, uc), ref, c.kind, c.O, c.A, c.H, c.f, ATOL)
        gru = {k: x for k, x in d.items() if k.startswith("base.gru")}
        print(c.tag, "clipped" if uc else "plain", "GRU blocks moved by", min(gru.values()), "..", max(gru.values()))
        assert max(gru.values()) >= 100 * RTOL, gru
        assert all(x == 0.0 for k, x in d.items() if k not in gru)
        # and the check that judges the GPU (distance <= RTOL on every block) does see it
        assert any(x > RTOL for x in gru.values())


@pytest.mark.parametrize("spec", OLD_GRU, ids=[f"{s[0]}-{s[2]}x{s[3]}x{s[4]}" + (f"-w{s[6]:g}o{s[7]:g}" if s[0] == "saturated" else "") for s in OLD_GRU])
def test_losing_the_later_workgroups_is_invisible_to_the_older_cases(spec):
    regime, kind, O, A, H, f, sw, so = spec
    c = rg.case(regime, kind, O, A, H, f, sw, so)
    assert c.N <= TILE
    for uc in (True, False):
        ref = c.desc["grad_clipped" if uc else "grad_plain"]
        got = grad_with_only_the_first_workgroup(c, uc)
        assert np.array_equal(got, ref), "the mutation changed a case that has no environment past 16"


def test_the_new_seeds_are_the_first_that_build():
    """SEEDS carries (T, N) for rollouts of another geometry; every seed below the committed one misses a builder condition."""
    for spec, T, N in CASES + [rg.GRU_STEPS_CASE]:
        kind, O, A, H, f = spec
        seed = rg.SEEDS.get(rg.seed_key("off_policy", kind, O, A, H, f, T=T, N=N), 0)
        assert rg.case("off_policy", *spec, T=T, N=N).seed == seed
        for s in range(max(0, seed - 2), seed):   # (the two seeds before it: the whole search is `python tests/regimes.py`)
            with pytest.raises(AssertionError):
                rg.build("off_policy", kind, O, A, H, f, T=T, N=N, seed=s)
    assert rg.seed_key("off_policy", "gru", 47, 12, 64, 1) == ("off_policy", "gru", 47, 12, 64, 1)   # the older keys are unchanged
