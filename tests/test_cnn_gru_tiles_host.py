"""CPU: the cases of cnn_gru_ref.TILE_CASES (tests/test_gpu_cnn_gru_tiles.py runs them on the GPU), judged without the library.

  1 geometry    cnn_gru_ref.geometry restates the launch arithmetic of one optimizer step of cnn_gru_ppo_update
                (simgan_amd/csrc/sg_ppo.hip; k_gru_dx, k_gru_wgrad and the scans in sg_gru_kernels.hpp, k_cnn_head_loss in
                sg_cnn_kernels.hpp) and FACTS holds every case to the edge it was chosen for, so a change to the launcher that moves a
                case off its edge fails here instead of silently emptying the GPU test; every older gradient case is one workgroup
                of everything
  2 admission   every new seed under the three conditions of tests/test_cnn_gru_host.py, none loosened
  3 clip        at cnn_gru_ref.TILE_CLIP the clip acts in every optimizer step under both value losses, and each value is half the
                case's smallest float64 step-gradient norm at two significant digits
  4 defects     four injected defects, each what a launch past one tile would lose, each on the references alone: exactly
                invisible to every older case, at least 10 RTOL in the new case named for it"""
import numpy as np
import pytest

import cnn_gru_ref as gr
import cnn_ref as cr
from helpers import RTOL

CAT33, CAT34, BOX17, WIDE6 = list(gr.TILE_CASES)
KEYS = list(gr.TILE_CASES)
IDS = ["-".join(map(str, k)) for k in KEYS]
# key -> the facts the case exists for (dx_walk: the 16-row tiles each k_gru_dx workgroup walks, LDS-weight grid / global-weight grid)
FACTS = {
    CAT33: dict(M=1, per=33, S=1, mb=264, rows_p=272, pad_rows=8, chunks=17, KS=2, sizes=[9, 8], scan_workgroups=3, last_live=1,
                loss_blocks=2, gw_dx=False, gw_scan=False, dx_grid_lds=5, dx_grid_gw=17, last_tile_live=8,
                dx_walk_lds=[[0, 5, 10, 15], [1, 6, 11, 16], [2, 7, 12], [3, 8, 13], [4, 9, 14]]),
    CAT34: dict(M=2, per=17, S=2, mb=68, rows_p=80, pad_rows=12, chunks=5, KS=1, sizes=[5], scan_workgroups=2, last_live=1,
                loss_blocks=1, gw_dx=False, gw_scan=False, dx_grid_lds=2, dx_grid_gw=5, last_tile_live=4, dx_walk_lds=[[0, 2, 4], [1, 3]]),
    BOX17: dict(M=1, per=17, S=1, mb=68, rows_p=80, pad_rows=12, chunks=5, KS=1, sizes=[5], scan_workgroups=2, last_live=1,
                loss_blocks=1, gw_dx=False, gw_scan=False, dx_grid_lds=2, dx_grid_gw=5, last_tile_live=4, dx_walk_lds=[[0, 2, 4], [1, 3]]),
    WIDE6: dict(M=1, per=6, S=1, mb=18, rows_p=32, pad_rows=14, chunks=2, KS=1, sizes=[2], scan_workgroups=1, last_live=6,
                loss_blocks=1, gw_dx=True, gw_scan=True, dx_grid_lds=1, dx_grid_gw=2, last_tile_live=2, dx_walk_lds=[[0, 1]])}


def geo_of(key, M):
    return gr.geometry(key[4], key[5], M, key[1])


# ------------------------------------------------------------------------------------------------- 1 geometry
def test_the_cases_are_the_four_of_the_table_and_stay_out_of_the_older_runs():
    assert KEYS == [(1, 16, "categorical", 5, 8, 33), (1, 16, "categorical", 5, 4, 34), (2, 20, "gaussian", 3, 4, 17),
                    (4, 512, "categorical", 6, 3, 6)]
    assert [gr.TILE_CASES[k] for k in KEYS] == [1, 2, 1, 1] and [gr.SEEDS[k] for k in KEYS] == [0, 0, 2, 0]
    assert gr.HEADS.get(WIDE6) == "peaked" and all(k not in gr.HEADS for k in KEYS[:3])
    assert not set(KEYS) & set(gr.GRAD_CASES) and len(gr.GRAD_CASES) == 5 and sorted(FACTS) == sorted(KEYS)
    assert sorted(gr.TILE_CLIP) == sorted(KEYS) and len(gr.CLIP_INACTIVE) == 1


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_case_sits_on_its_edge_of_the_launcher(key):
    want = dict(FACTS[key])
    g = geo_of(key, want.pop("M"))
    print(key, g)
    for name, value in want.items():
        assert g[name] == value, (name, g[name], value)
    assert g["mb"] == key[4] * g["per"] and g["S"] * g["per"] == key[5] and sum(g["sizes"]) == g["chunks"] == g["rows_p"] // 16
    # the ranges of k_gru_wgrad tile [0, chunks) in order
    end = 0
    for c0, c1 in g["ranges"]:
        assert c0 == end < c1
        end = c1
    assert end == g["chunks"]
    # every workgroup of k_gru_dx has a tile, every tile one workgroup, and the global-weight grid is one tile per workgroup
    for walk in (g["dx_walk_lds"], g["dx_walk_gw"]):
        assert all(walk) and sorted(t for w in walk for t in w) == list(range((g["mb"] + 15) // 16))
    assert all(len(w) == 1 for w in g["dx_walk_gw"]) and g["dx_grid"] == (g["dx_grid_gw"] if g["gw_dx"] else g["dx_grid_lds"])
    assert g["Hp"] == ((key[1] + 15) // 16) * 16


def test_every_edge_has_a_case():
    g33, g34, g17, g6 = (geo_of(k, gr.TILE_CASES[k]) for k in KEYS)
    # 8 x 33: a third scan workgroup with one live environment, KS = 2 with ragged ranges whose last runs over padding rows, a
    # second loss block, an LDS-weight k_gru_dx grid of 5 with a grid stride of 5 tiles
    assert g33["scan_workgroups"] == 3 and g33["last_live"] == 1 and g33["KS"] == 2 and len(set(g33["sizes"])) == 2
    assert g33["pad_rows"] > 0 and g33["loss_blocks"] == 2 and g33["mb"] > 256 and g33["dx_grid_lds"] == 5
    assert 16 * g33["ranges"][0][1] == 144 and 144 % g33["per"] != 0      # the range boundary falls inside a time step's rows
    # 4 x 34, M = 2: per = 17; step 1's permutation, h0 rows and row block start off every 16-multiple; a real grid stride
    assert g34["S"] == 2 and g34["per"] == 17 and g34["mb"] == 68 and g34["mb"] % 16 == 4 and g34["dx_walk_lds"][0] == [0, 2, 4] and g34["dx_grid_gw"] == 5
    # 4 x 17 Gaussian at Hs = 20: Hp = Op = 32 against the unpadded [mb][20] matrices, over two workgroups of both kinds
    assert g17["Hp"] == 32 and BOX17[1] % 16 and g17["dx_grid_lds"] == 2 and g17["scan_workgroups"] == 2 and not g17["gw_dx"]
    # 3 x 6 at Hs = 512: global-weight instances by size, two row tiles, the second with 2 live rows
    assert g6["gw_dx"] and g6["gw_scan"] and g6["dx_grid"] == 2 and g6["last_tile_live"] == 2
    for k in KEYS[:3]:     # the three narrow cases run the LDS-weight instances unless the switch forces the others
        assert not geo_of(k, gr.TILE_CASES[k])["gw_dx"] and not geo_of(k, gr.TILE_CASES[k])["gw_scan"]


def test_the_older_gradient_cases_are_one_workgroup_of_everything():
    """the gap in one line: k_gru_dx's grid in every run of either instance, the scans' grid, KS and the loss blocks are all 1.
    The global-weight instance ran where the LDS sizes choose it (Hs = 512) and where tests/test_gpu_cnn_gru.py's GRAD_RUNS set
    SG_POLICY_GW=1 (the Hs = 16 Discrete key); the 5 x 7 key's 3 chunks met the LDS-weight formula only, which gives 1."""
    switched = [k for k in gr.GRAD_CASES if k[1] == 16 and k[2] == "categorical"]
    assert switched == [(1, 16, "categorical", 5, 4, 4)]
    for key, M in gr.GRAD_CASES.items():
        g = geo_of(key, M)
        assert (g["dx_grid"], g["scan_workgroups"], g["KS"], g["loss_blocks"]) == (1, 1, 1, 1), (key, g)
        assert g["dx_grid_lds"] == 1 and (g["dx_grid_gw"] == 1 or not (g["gw_dx"] or key in switched)), (key, g)
        assert g["mb"] <= 35 and g["per"] <= 7 and g["chunks"] <= 3
    assert geo_of((4, 512, "categorical", 6, 3, 2), 1)["gw_dx"] and not geo_of(switched[0], 2)["gw_dx"]


# ------------------------------------------------------------------------------------------------- 2 admission
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_every_new_seed_is_admitted_on_the_references_alone(key):
    c = gr.case(*key)
    assert c.seed == gr.SEEDS[key] and c.head == gr.HEADS.get(key, "init")
    km, exempted, branch = gr.margins(c)
    print(c.tag, "kink margin", km, "branch margin", branch)
    assert km >= cr.KINK_FACTOR and branch >= cr.MARGIN and exempted == 0, (c.tag, km, branch, exempted)
    d32 = gr.admitted(key)[2]
    print(c.tag, "worst float32 block", max(d32.values()))
    assert max(d32.values()) <= 0.5 * RTOL, (c.tag, d32)
    # the masks and h0 are default_masks' / build's: every kind of reset is there, the state of slot 0 is not zero
    m = c.masks[:-1, :, 0]
    assert np.array_equal(c.masks, gr.default_masks(c.T, c.N)) and np.abs(c.hxs[0]).min() > 0
    assert m[0, 0] == 0 and m[c.T // 2, 1] == 0 and not m[:, 2].any()
    if c.T >= 4:
        assert m[1, -1] == 0 and m[2, -1] == 0      # (in the last scan workgroup's one live environment where N = 33, 34, 17)


def test_the_gaussian_seed_is_the_first_that_find_seed_admits():
    assert gr.find_seed(*BOX17)[0] == gr.SEEDS[BOX17] == 2


# ------------------------------------------------------------------------------------------------- 3 clip
def two_digits(x):
    return float(f"{x:.1e}")


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_the_clip_acts_in_every_step_at_tile_clip(key):
    c, M = gr.case(*key), gr.TILE_CASES[key]
    perm = np.random.default_rng(gr.PERM_SEED).permutation(c.N)
    norms = []
    for use_clipped in (True, False):
        for envs in gr.step_envs(key, M, perm):
            g = gr.case_grad(c, envs, use_clipped)[0]
            norms.append(float(np.sqrt((g ** 2).sum())))
            assert cr.clip_factor(g, gr.TILE_CLIP[key]) < 1.0, (key, use_clipped, norms[-1])
    print(key, "step-gradient norms", norms)
    assert len(norms) == 2 * geo_of(key, M)["S"] and gr.TILE_CLIP[key] == two_digits(0.5 * min(norms))
    if key in (CAT33, CAT34):      # at the suite's usual 0.5 the clip would not act in any step of the two Discrete(5) cases
        assert max(norms) < 0.5


# ------------------------------------------------------------------------------------------------- 4 injected defects
SEEN_IN = {"dx_rows_first_64": (BOX17, CAT33), "scan_envs_first_16": (CAT33, CAT34, BOX17), "wgrad_first_range": (CAT33,),
           "loss_rows_first_256": (CAT33,)}
GRU_BLOCKS = tuple("base.gru." + k for k in gr.GRU_NAMES)
UNTOUCHED = 1e-12      # a block the defect does not reach: the same sum of the same terms (torch may group a batched product differently)


def test_every_new_defect_has_its_cases():
    assert set(SEEN_IN) == set(gr.TILE_FAULTS) and not set(gr.TILE_FAULTS) & set(gr.FAULTS)


@pytest.mark.parametrize("fault", gr.TILE_FAULTS)
def test_the_new_defects_are_exactly_invisible_to_every_older_case(fault):
    for key in gr.GRAD_CASES:
        c = gr.case(*key)
        g, losses = gr.admitted(key)[:2]
        gf, lf = gr.case_grad(c, fault=fault)
        d = cr.block_distances(gf, g, c.shapes)
        assert all(x == 0.0 for x in d.values()) and np.array_equal(gf, g) and np.array_equal(lf, losses), (fault, key, d)


@pytest.mark.parametrize("fault,key", [(f, k) for f in gr.TILE_FAULTS for k in SEEN_IN[f]],
                         ids=[f"{f}-{'-'.join(map(str, k))}" for f in gr.TILE_FAULTS for k in SEEN_IN[f]])
def test_the_new_defects_are_seen_in_their_cases(fault, key):
    c, M = gr.case(*key), gr.TILE_CASES[key]
    perm = np.random.default_rng(gr.PERM_SEED).permutation(c.N)
    envs = gr.step_envs(key, M, perm)[0]      # the first optimizer step of the GPU test's own epoch
    g, losses = gr.case_grad(c, envs)
    gf, lf = gr.case_grad(c, envs, fault=fault)
    d = cr.block_distances(gf, g, c.shapes)
    moved = {k for k, x in d.items() if x >= 10 * RTOL}
    print(fault, c.tag, {k: f"{x:.3g}" for k, x in d.items()})
    assert moved, (fault, d)
    trunk = {k for k in d if k.startswith("base.main.")}
    heads = set(d) - trunk - set(GRU_BLOCKS)
    if fault == "dx_rows_first_64":          # the trunk alone: weight_ih's own gradient, the GRU's other tensors and the heads are whole
        assert moved <= trunk and "base.main.7.weight" in moved and all(d[k] <= UNTOUCHED for k in set(d) - trunk)
    elif fault == "scan_envs_first_16":      # the GRU block and the trunk lose the environments; the heads' weights keep them
        assert moved <= trunk | set(GRU_BLOCKS) and set(GRU_BLOCKS) & moved and trunk & moved and all(d[k] <= UNTOUCHED for k in heads)
    elif fault == "wgrad_first_range":       # the GRU block alone
        assert moved <= set(GRU_BLOCKS) and all(d[k] <= UNTOUCHED for k in set(d) - set(GRU_BLOCKS))
    else:                                    # the loss sums too: 256 of 264 rows over the divisor 264
        assert np.abs(lf - losses).max() > 1e-3 * np.abs(losses).max()
    if fault != "loss_rows_first_256":
        assert np.abs(lf - losses).max() <= UNTOUCHED
