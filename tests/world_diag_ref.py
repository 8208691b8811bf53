"""The world scope of the two diagnostics families (include/simgan_hip.h: sg_rollout_policy_diagnostics_world,
sg_disc_diagnostics_world): the union cases of tests/test_world_diag_host.py (CPU) and tests/test_gpu_world_diag.py (GPU), their
column shards, and the per-rank-then-merge route restated in float64.  Nothing here touches the library.

THE ARBITER is the existing float64 reference run ONCE on the concatenated case: diag_ref.reference(c) with c built at
N = world * N_loc, disc_diag_ref.reference(c) likewise -- its mid_rows pairs union row i = t * (world * N_loc) + n_global with
expert[i mod n_e], the global pairing.  Global column = rank * N_loc + n (tests/test_gpu_world.py).  No
tolerance of its own: diag_ref.compare / disc_diag_ref.compare under their rule, their EXACT names exact.

THE ROUTE (merged_policy, merged_disc) is what the library does, in float64: the union's per-row terms split by columns, per rank a
record of plain sums, minimum / maximum and (count, mean, M2) triples, the records merged in ascending rank order by Chan, Golub
and LeVeque's update, then the finalise.  It serves tests/test_world_diag_host.py alone: there it equals the one-pass reference
to 1e-12 relative, and its wrong variants (FAULTS) miss the rule on the case built to catch each."""
import functools

import numpy as np

import diag_ref as dg
import disc_diag_ref as dd
import discrete_ref as dr
import disc_regimes as rg

FAULTS = ("avg_var", "expert_merged", "local_pairing")


# ------------------------------------------------------------------------------------------------- policy cases
def _means_apart():
    """the far-returns recipe at T, N = 7, 22 with 20.0 added to the returns and value predictions of columns [11, 22): the two
    ranks' return means lie far apart, so almost all of Var(ret) is the between-rank term of Chan's formula.  The log-probs are
    untouched: diag_ref.conditions holds as for the base case."""
    c = dict(dg.gauss_case("mlp", 5, 2, 8, 1, 7, 22, 0, True))
    for k in ("returns", "value_preds"):
        a = np.array(c[k])
        a[:, 11:22] += np.float32(20.0)
        c[k] = a
    c["tag"] += ", columns [11, 22) 20 higher"
    return c


# name -> (world, builder of the union case): tests/test_gpu_world_diag.py runs every one, T, N_loc in the comment
POLICY_CASES = {
    "mlp_2x8_w2": (2, lambda: dg.gauss_case("mlp", 5, 2, 8, 1, 2, 16)),                # 2, 8: half a tile per rank
    "mlp_7x11_w2": (2, lambda: dg.gauss_case("mlp", 5, 2, 8, 1, 7, 22)),               # 7, 11: 77 rows per rank, ragged last tile
    "mlp_7x11_w4": (4, lambda: dg.gauss_case("mlp", 5, 2, 8, 1, 7, 44)),               # 7, 11
    "mlp_1x1_w4": (4, lambda: dg.gauss_case("mlp", 5, 2, 8, 1, 1, 4)),                 # 1, 1: one row per rank, four in the union
    "split_3x11_w2": (2, lambda: dg.gauss_case("split", 14, 7, 100, 1, 3, 22)),        # 3, 11
    "discrete_7x11_w2": (2, lambda: dg.discrete_case(dr.CATEGORICAL, *dr.SHAPES[dr.CATEGORICAL][0], 7, 22)),   # 7, 11
    "means_apart_w2": (2, _means_apart),                                               # 7, 11
}


@functools.lru_cache(maxsize=None)
def policy_case(name):
    """-> (world, union case); computed once per process and shared (callers must not write into it)"""
    world, build = POLICY_CASES[name]
    c = build()
    assert c["N"] % world == 0
    return world, c


def policy_shard(c, rank, world):
    """rank's columns [rank * N_loc, (rank + 1) * N_loc) of the union case, as a case of its own"""
    n = c["N"] // world
    s = dict(c, N=n, tag=f"{c['tag']} rank {rank}/{world}")
    for k in ("obs", "actions", "action_log_probs", "value_preds", "returns", "masks"):
        s[k] = np.ascontiguousarray(np.asarray(c[k])[:, rank * n:(rank + 1) * n])
    return s


# ------------------------------------------------------------------------------------------------- discriminator cases
# name -> (F, Hd, T, N_loc, n_e, world, regime)
DISC_SPECS = {
    "both_7x16_7x11_e17_w2": (7, 16, 7, 11, 17, 2, "both_sides"),     # the pairing wraps; 11 mod 17 != 0: the local pairing differs
    "init_7x16_2x8_e5_w2": (7, 16, 2, 8, 5, 2, "init"),
    "sat_7x16_3x5_e7_w4": (7, 16, 3, 5, 7, 4, "saturated"),
    "both_86x100_7x11_e100_w2": (86, 100, 7, 11, 100, 2, "both_sides"),
    "init_7x16_1x1_e1_w2": (7, 16, 1, 1, 1, 2, "init"),
}


@functools.lru_cache(maxsize=None)
def disc_case(name):
    """-> (world, union case): disc_diag_ref.build at N = world * N_loc, the first (seed, scale) of its search at which its
    conditions hold; computed once per process and shared"""
    F, Hd, T, n_loc, n_e, world, regime = DISC_SPECS[name]
    last = None
    for seed in range(dd.MAX_SEED):
        for sw in (dd.BOTH_SIDES_SCALES if regime == "both_sides" else (None,)):
            c = dd.build(F, Hd, T, world * n_loc, n_e, regime, seed, sw)
            c["name"] = name
            try:
                dd.conditions(c)
            except AssertionError as exc:
                last = exc
                continue
            return world, c
    raise AssertionError(f"{name}: no seed below {dd.MAX_SEED} meets the conditions; the last miss: {last}")


def disc_reference(c):
    """disc_diag_ref.reference on a case that is not one of its own (its cache goes by name)"""
    r = dd.rows(c)
    return dd.statistics(r), dd.allowances(r)


def disc_shard_rows(c, rank, world):
    """rank's policy rows [T * N_loc, F], time-major, out of the union's [T * N, F]"""
    n = c.N // world
    return np.ascontiguousarray(c.policy.reshape(c.T, c.N, c.F)[:, rank * n:(rank + 1) * n].reshape(c.T * n, c.F))


# ------------------------------------------------------------------------------------------------- the route, in float64
def _triple(x):
    x = np.asarray(x, np.float64)
    m = x.mean()
    return [float(x.size), float(m), float(((x - m) ** 2).sum())]


def _chan(a, b):
    """(count, mean, M2) a <- merged with b"""
    na, nb = a[0], b[0]
    if nb == 0.0:
        return a
    n, delta = na + nb, b[1] - a[1]
    return [n, a[1] + delta * (nb / n), a[2] + b[2] + delta * delta * (na * (nb / n))]


def _columns(x, T, N, rank, world):
    n = N // world
    return np.asarray(x).reshape(T, N, *np.shape(x)[1:])[:, rank * n:(rank + 1) * n].reshape(T * n, *np.shape(x)[1:])


def merged_policy(c, world, clip=dg.CLIP, fault=None):
    """the ten statistics by the route; fault "avg_var": the ranks' variances averaged instead of merged"""
    v, lp, ent = dg.evaluate(c)
    lpo, vp, R = dg.rollout_rows(c)
    T, N = c["T"], c["N"]
    sums, rmin, rmax = np.zeros(6), np.inf, -np.inf
    tri = {k: [0.0, 0.0, 0.0] for k in ("ret", "eo", "en")}
    var = {k: [] for k in tri}
    for rank in range(world):
        col = lambda x: _columns(np.asarray(x, np.float64).reshape(-1), T, N, rank, world)  # noqa: E731
        d = col(lp) - col(lpo)
        r = np.exp(d)
        en, eo, ret = col(R) - col(v), col(R) - col(vp), col(R)
        sums += [d.size, (-d).sum(), (np.expm1(d) - d).sum(), (np.abs(r - 1.0) > clip).sum(), col(ent).sum(), (en ** 2).sum()]
        rmin, rmax = min(rmin, r.min()), max(rmax, r.max())
        for k, x in (("ret", ret), ("eo", eo), ("en", en)):
            tri[k] = _chan(tri[k], _triple(x))
            var[k].append(x.var())
    n = sums[0]
    if fault == "avg_var":
        v_ret, v_eo, v_en = (float(np.mean(var[k])) for k in ("ret", "eo", "en"))
    else:
        v_ret, v_eo, v_en = (tri[k][2] / n for k in ("ret", "eo", "en"))
    with np.errstate(all="ignore"):
        vals = (n, sums[1] / n, sums[2] / n, sums[3] / n, sums[4] / n, rmin, rmax, np.float64(1.0) - np.float64(v_eo) / np.float64(v_ret),
                np.float64(1.0) - np.float64(v_en) / np.float64(v_ret), sums[5] / n)
    return {k: float(x) for k, x in zip(dg.NAMES, vals)}


def _part(d, g, expert):
    """one population's part of a record from its logits and gradient norms"""
    rew, _ = rg.reward64(d)
    z = -d if expert else d
    return dict(n=float(d.size), flag=float((z < 0).sum()), bce=float(dd.softplus(z).sum()), g_sum=float(g.sum()),
                pen=float(((g - 1.0) ** 2).sum()), r_min=float(rew.min()), r_max=float(rew.max()), g_max=float(g.max()),
                lg=_triple(d), rw=_triple(rew))


def _merge_part(a, b):
    if a is None:
        return b
    out = {k: a[k] + b[k] for k in ("n", "flag", "bce", "g_sum", "pen")}
    out.update(r_min=min(a["r_min"], b["r_min"]), r_max=max(a["r_max"], b["r_max"]), g_max=max(a["g_max"], b["g_max"]),
               lg=_chan(a["lg"], b["lg"]), rw=_chan(a["rw"], b["rw"]))
    return out


def merged_disc(c, world, fault=None):
    """the nineteen statistics by the route: policy and mid parts merged in rank order, the expert part rank 0's.  fault
    "expert_merged": every rank's expert part merged too; "local_pairing": a rank's mid row i = t * N_loc + n takes
    expert[i mod n_e], not the row of its number in the union"""
    r = dd.rows(c)
    p, F, Hd, T, N = c.params, c.F, c.Hd, c.T, c.N
    pol = mid = exp = None
    for rank in range(world):
        col = lambda x: _columns(x, T, N, rank, world)  # noqa: E731
        g_m = col(r["g_m"])
        if fault == "local_pairing":
            g_m = dd.gnorm_autograd(p, F, Hd, dd.mid_rows(c.expert, disc_shard_rows(c, rank, world)))
        pol = _merge_part(pol, _part(col(r["d_p"]), col(r["g_p"]), False))
        mid = _merge_part(mid, _part(col(r["d_p"]), g_m, False))       # (of a mid part only the gradient terms are used)
        if rank == 0 or fault == "expert_merged":
            exp = _merge_part(exp, _part(r["d_e"], r["g_e"], True))
    std = lambda t: float(np.sqrt(t[2] / t[0]))  # noqa: E731
    vals = (pol["n"], exp["n"], pol["flag"] / pol["n"], exp["flag"] / exp["n"], pol["lg"][1], std(pol["lg"]), exp["lg"][1], std(exp["lg"]),
            pol["bce"] / pol["n"], exp["bce"] / exp["n"], pol["rw"][1], std(pol["rw"]), pol["r_min"], pol["r_max"], pol["g_sum"] / pol["n"],
            exp["g_sum"] / exp["n"], mid["g_sum"] / mid["n"], dd.LAMBDA * (mid["pen"] / mid["n"]), max(pol["g_max"], exp["g_max"], mid["g_max"]))
    return {k: float(x) for k, x in zip(dd.NAMES, vals)}
