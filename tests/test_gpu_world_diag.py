"""GPU: the world scope of the update and discriminator diagnostics -- sg_rollout_policy_diagnostics_world /
sg_disc_diagnostics_world, the scope="world" keyword of PPO.diagnostics, Discriminator.diagnostics_world, and the learners'
update(diagnostics="world", disc_diagnostics="world") -- on ONE device: `world` contexts, one host thread each, joined by a loopback
communicator (tests/test_gpu_world.py's run_ranks pattern).

The arbiter is the float64 reference run once on the concatenated case (tests/world_diag_ref.py: THE ARBITER): rank r holds the
union's columns [r * N_loc, (r + 1) * N_loc).  For every case
  1. the ten / nineteen doubles are bit-identical on all ranks;
  2. they pass diag_ref.compare / disc_diag_ref.compare against the union reference, EXACT names exact;
  3. against a single-context rank-scope launch on the concatenated rollout the order-free entries are bit-equal and the others
     pass the same compare (the tiles differ, so their bits may);
  4. rows == world * T * N_loc, expert_rows == n_e;
  5. the queued form gives the synchronous form's bits;
  6. the discriminator's two slots give the same bits.

SG_WDIAG_RECORD=<path> collects, per statistic, the worst distance / bound over all cases (profiles/world_diag_parity.json)."""
import ctypes as C
import json
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diag_ref as dg  # noqa: E402
import disc_diag_ref as dd  # noqa: E402
import discrete_ref as dr  # noqa: E402
import world_diag_ref as wd  # noqa: E402

pytestmark = pytest.mark.gpu

POLICY_ORDER_FREE = ("rows", "clip_fraction", "ratio_min", "ratio_max")
DISC_ORDER_FREE = ("policy_rows", "expert_rows", "policy_accuracy", "expert_accuracy", "reward_min", "reward_max", "grad_norm_max")
WORST = {"policy": {}, "disc": {}}


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    yield simgan_amd
    path = os.environ.get("SG_WDIAG_RECORD")
    if path and (WORST["policy"] or WORST["disc"]):
        doc = {"what": "tests/test_gpu_world_diag.py under SG_WDIAG_RECORD: per statistic, the worst |world scope - float64 on the "
                       "concatenated case| / (1e-4 |float64| + allowance) over all cases (ranks as threads of one process on one "
                       "device, loopback communicator), and the case it was seen on; the EXACT names are exact (0)",
               "policy": WORST["policy"], "disc": WORST["disc"]}
        with open(path, "w") as f:
            json.dump(doc, f, indent=1)


def run_ranks(world, fn, timeout_s=600):
    """fn(rank, ctx) on `world` threads, each with its own context on device 0 joined by one loopback communicator.
    Returns the list of results; the first exception of any rank is re-raised."""
    from simgan_amd import _lib
    os.environ.setdefault("SG_LOOPBACK_TIMEOUT_S", "120")
    uid = _lib.comm_loopback_id()
    out, err = [None] * world, [None] * world

    def body(rank):
        try:
            ctx = _lib.Context(0)
            ctx.comm_init(uid, rank, world)
            assert ctx.comm_kind() == "loopback" and ctx.comm_info() == (rank, world)
            out[rank] = fn(rank, ctx)
            ctx.synchronize()
        except BaseException as exc:   # noqa: BLE001 -- reported to the test below
            err[rank] = exc

    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout_s)
    assert not any(t.is_alive() for t in threads), "a rank is still running (loopback collective stuck?)"
    bad = [(r, e) for r, e in enumerate(err) if e is not None]
    if bad:   # a rank that fails leaves its peers to time out in their next collective: report the root cause first
        bad.sort(key=lambda re_: ("peer rank failed" in str(re_[1])) + 2 * ("timed out" in str(re_[1])))
        raise AssertionError("; ".join(f"rank {r}: {type(e).__name__}: {str(e)[:300]}" for r, e in bad[:3])) from bad[0][1]
    return out


def bits(d, names):
    return tuple(int(np.float64(d[k]).view(np.uint64)) for k in names)


def note(family, label, dist):
    for k, x in dist.items():
        w = WORST[family].setdefault(k, {"ratio": 0.0, "case": label})
        if np.isfinite(x) and x > w["ratio"]:
            w["ratio"], w["case"] = float(x), label


# ------------------------------------------------------------------------------------------------- policy
def space_of(c):
    return dr.Box((c["A"],)) if c["kind"] in ("mlp", "split") else dr.space(c["dist"], c["K"])


def make_policy(sg, c, ctx=None):
    if c["kind"] == "split":
        p = sg.SplitPolicy((c["O"],), space_of(c), base_kwargs={"hidden_size": c["H"], "num_feet": c["f"]}, ctx=ctx)
    else:
        p = sg.Policy((c["O"],), space_of(c), base_kwargs={"recurrent": False, "hidden_size": c["H"]}, ctx=ctx)
    p.set_flat_params(np.asarray(c["params"], np.float32))
    return p


def make_rollout(sg, c, ctx=None, F=1, obs_feat=None):
    ro = sg.RolloutStorage(c["T"], c["N"], (c["O"],), space_of(c), 1, F, ctx=ctx)
    if obs_feat is not None:
        ro.obs_feat.copy_(ro.obs_feat.new_tensor(obs_feat))
    for name in ("obs", "actions", "action_log_probs", "value_preds", "returns", "masks"):
        t = getattr(ro, name)
        t.copy_(t.new_tensor(np.asarray(c[name]).reshape(tuple(t.shape))))
    ro.device_resident = True
    ro.sync_to_device()
    return ro


def ppo(sg, pol, epochs=1, mb=1):
    return sg.algo.PPO(pol, dg.CLIP, epochs, mb, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)


@pytest.mark.parametrize("name", wd.POLICY_CASES)
def test_policy_world_scope(sg, name):
    world, c = wd.policy_case(name)

    def rank_fn(rank, ctx):
        s = wd.policy_shard(c, rank, world)
        agent, ro = ppo(sg, make_policy(sg, s, ctx)), make_rollout(sg, s, ctx)
        sync = agent.diagnostics(ro, scope="world")
        assert agent.diagnostics(ro, fetch=False, scope="world") is None
        return sync, agent.last_diagnostics()

    res = run_ranks(world, rank_fn)
    got = res[0][0]
    assert tuple(got) == dg.NAMES
    for rank, (sync, queued) in enumerate(res):
        assert bits(sync, dg.NAMES) == bits(got, dg.NAMES), f"rank {rank} differs from rank 0: {sync} vs {got}"
        assert bits(queued, dg.NAMES) == bits(sync, dg.NAMES), f"rank {rank}: the queued form differs: {queued} vs {sync}"
    want, allow = dg.reference(c)
    dist = dg.compare(got, want, allow)
    note("policy", name, dist)
    print(name, {k: (got[k], want[k], allow[k], round(dist[k], 4)) for k in dg.NAMES})
    assert not {k: (got[k], want[k], allow[k], dist[k]) for k in dg.NAMES if not dist[k] <= 1.0}, (got, want, dist)
    assert got["rows"] == world * c["T"] * (c["N"] // world) == want["rows"] and got["clip_fraction"] == want["clip_fraction"]
    single = ppo(sg, make_policy(sg, c)).diagnostics(make_rollout(sg, c))
    assert bits(got, POLICY_ORDER_FREE) == bits(single, POLICY_ORDER_FREE), (got, single)
    dist = dg.compare(got, single, allow)
    assert all(dist[k] <= 1.0 for k in dg.NAMES), (got, single, dist)


# ------------------------------------------------------------------------------------------------- discriminator
def make_disc(sg, c, ctx=None, expert=None):
    d = sg.algo.gail.Discriminator(c.F, c.Hd, None, ctx=ctx, seed=1)
    d.set_flat_params(np.asarray(c.params, np.float32))
    d.set_expert(c.expert if expert is None else expert)
    return d


def disc_rollout(sg, T, N, F, rows, ctx=None):
    """obs_feat[1:] are the policy rows; slot 0, which the launch must not read, holds 1e3"""
    ro = sg.RolloutStorage(T, N, (3,), dr.Box((1,)), 1, F, ctx=ctx)
    ro.obs_feat.copy_(ro.obs_feat.new_tensor(np.concatenate([np.full((1, N, F), 1e3, np.float32), rows.reshape(T, N, F)])))
    ro.device_resident = True
    ro.sync_to_device()
    return ro


@pytest.mark.parametrize("sharded", [False, True], ids=["replicated", "sharded"])
@pytest.mark.parametrize("name", wd.DISC_SPECS)
def test_disc_world_scope(sg, name, sharded):
    world, c = wd.disc_case(name)
    n_loc, n_e = c.N // world, c.expert.shape[0]

    def rank_fn(rank, ctx):
        ctx.set_disc_dp(sharded)
        disc, ro = make_disc(sg, c, ctx), disc_rollout(sg, c.T, n_loc, c.F, wd.disc_shard_rows(c, rank, world), ctx)
        slot0, slot1 = disc.diagnostics_world(ro), disc.diagnostics_world(ro, slot=1)
        assert disc.diagnostics_world(ro, fetch=False) is None and disc.diagnostics_world(ro, fetch=False, slot=1) is None
        return slot0, slot1, disc.last_diagnostics(1), disc.last_diagnostics(0)

    res = run_ranks(world, rank_fn)
    got = res[0][0]
    assert tuple(got) == dd.NAMES
    for rank, forms in enumerate(res):
        for what, other in zip(("slot 0", "slot 1", "slot 1 queued", "slot 0 queued"), forms):
            assert bits(other, dd.NAMES) == bits(got, dd.NAMES), f"rank {rank}, {what} differs from rank 0, slot 0: {other} vs {got}"
    want, allow = wd.disc_reference(c)
    dist = dd.compare(got, want, allow)
    note("disc", f"{name} {'sharded' if sharded else 'replicated'}", dist)
    print(name, {k: (got[k], want[k], allow[k], round(dist[k], 4)) for k in dd.NAMES})
    assert not {k: (got[k], want[k], allow[k], dist[k]) for k in dd.NAMES if not dist[k] <= 1.0}, (got, want, dist)
    assert all(got[k] == want[k] for k in dd.EXACT), (got, want)
    assert got["policy_rows"] == world * c.T * n_loc and got["expert_rows"] == n_e
    single = make_disc(sg, c).diagnostics(disc_rollout(sg, c.T, c.N, c.F, c.policy))
    assert bits(got, DISC_ORDER_FREE) == bits(single, DISC_ORDER_FREE), (got, single)
    dist = dd.compare(got, single, allow)
    assert all(dist[k] <= 1.0 for k in dd.NAMES), (got, single, dist)


# ------------------------------------------------------------------------------------------------- once, not per case
def _both_scopes(sg, ctx):
    """rank and world scope of both families on one context -> four dicts"""
    _, c = wd.policy_case("mlp_7x11_w2")
    agent, ro = ppo(sg, make_policy(sg, c, ctx)), make_rollout(sg, c, ctx)
    _, d = wd.disc_case("both_7x16_7x11_e17_w2")
    disc, dro = make_disc(sg, d, ctx), disc_rollout(sg, d.T, d.N, d.F, d.policy, ctx)
    assert agent.diagnostics(ro, fetch=False, scope="world") is None
    queued = agent.last_diagnostics()
    return agent.diagnostics(ro), agent.diagnostics(ro, scope="world"), queued, disc.diagnostics(dro), \
        disc.diagnostics_world(dro), disc.diagnostics_world(dro, slot=1)


def _check_both_scopes(res):
    p_rank, p_world, p_queued, d_rank, d_world, d_world1 = res
    assert bits(p_rank, dg.NAMES) == bits(p_world, dg.NAMES) == bits(p_queued, dg.NAMES), (p_rank, p_world, p_queued)
    assert bits(d_rank, dd.NAMES) == bits(d_world, dd.NAMES) == bits(d_world1, dd.NAMES), (d_rank, d_world, d_world1)
    assert p_rank["rows"] == 154.0 and d_rank["policy_rows"] == 154.0 and d_rank["expert_rows"] == 17.0


def test_world_scope_without_a_communicator_is_the_rank_scope(sg):
    _check_both_scopes(_both_scopes(sg, None))


def test_world_scope_on_a_one_rank_communicator_is_the_rank_scope(sg):
    _check_both_scopes(run_ranks(1, lambda rank, ctx: _both_scopes(sg, ctx))[0])


def test_rank_scope_at_world_2_stays_local(sg):
    """today's behaviour: each rank's own numbers -- the bits a context of its own gives on the shard -- and no collective (rank 1
    issues nothing while rank 0 asks twice)"""
    world, c = wd.policy_case("mlp_7x11_w2")
    _, d = wd.disc_case("both_7x16_7x11_e17_w2")

    def local(rank, ctx):
        s = wd.policy_shard(c, rank, world)
        p = ppo(sg, make_policy(sg, s, ctx)).diagnostics(make_rollout(sg, s, ctx))
        return p, make_disc(sg, d, ctx).diagnostics(disc_rollout(sg, d.T, d.N // world, d.F, wd.disc_shard_rows(d, rank, world), ctx))

    def rank_fn(rank, ctx):
        out = local(rank, ctx)
        return local(rank, ctx) if rank == 0 else out

    res = run_ranks(world, rank_fn)
    for rank in range(world):
        alone = local(rank, None)
        assert bits(res[rank][0], dg.NAMES) == bits(alone[0], dg.NAMES) and res[rank][0]["rows"] == 77.0
        assert bits(res[rank][1], dd.NAMES) == bits(alone[1], dd.NAMES) and res[rank][1]["policy_rows"] == 77.0
    assert bits(res[0][0], dg.NAMES) != bits(res[1][0], dg.NAMES) and bits(res[0][1], dd.NAMES) != bits(res[1][1], dd.NAMES)


def test_unequal_shards_are_refused_by_the_fetch_on_every_rank(sg):
    """N_loc = 8 and 9: the collective completes on both ranks, the fetch returns the row-count error -- both forms, both families
    -- and nothing stays pending; likewise expert matrices of 5 and 6 rows.  An error return: no kernel is aborted, and the next
    collective runs."""
    from simgan_amd import _lib
    err = _lib.SimganHipError
    cases = [dg.gauss_case("mlp", 5, 2, 8, 1, 2, 8), dg.gauss_case("mlp", 5, 2, 8, 1, 2, 9)]
    _, d = wd.disc_case("init_7x16_2x8_e5_w2")

    def rank_fn(rank, ctx):
        c, n = cases[rank], 8 + rank
        agent, ro = ppo(sg, make_policy(sg, c, ctx)), make_rollout(sg, c, ctx)
        with pytest.raises(err, match="sg_rollout_policy_diagnostics_fetch: the ranks of the world scope hold different numbers of rows"):
            agent.diagnostics(ro, scope="world")
        assert agent.diagnostics(ro, fetch=False, scope="world") is None
        with pytest.raises(err, match="sg_rollout_policy_diagnostics_fetch: the ranks of the world scope hold different numbers of rows"):
            agent.last_diagnostics()
        with pytest.raises(err, match="no diagnostics are pending"):
            _lib.check(ro.lib.sg_rollout_policy_diagnostics_fetch(ro.h, (C.c_double * 10)()))
        dro = disc_rollout(sg, 2, n, d.F, d.policy[:2 * n], ctx)
        disc = make_disc(sg, d, ctx)
        with pytest.raises(err, match="sg_disc_diagnostics_fetch: the ranks of the world scope hold different numbers of rows"):
            disc.diagnostics_world(dro)
        assert disc.diagnostics_world(dro, fetch=False, slot=1) is None
        with pytest.raises(err, match="sg_disc_diagnostics_fetch: the ranks of the world scope hold different numbers of rows"):
            disc.last_diagnostics(1)
        with pytest.raises(err, match="no diagnostics are pending in slot 1"):
            disc.last_diagnostics(1)
        # equal rows, expert matrices of 5 and 6 rows
        dro = disc_rollout(sg, 2, 8, d.F, d.policy[:16], ctx)
        odd = make_disc(sg, d, ctx, expert=np.concatenate([d.expert, d.expert[:rank]]))
        with pytest.raises(err, match="sg_disc_diagnostics_fetch: the ranks of the world scope hold expert matrices of different"):
            odd.diagnostics_world(dro)
        # the rank scope is untouched by all this, and an equal-shard collective right after gives numbers
        assert agent.diagnostics(ro)["rows"] == 2.0 * n and disc.diagnostics(dro)["policy_rows"] == 16.0
        return disc.diagnostics_world(dro)

    res = run_ranks(2, rank_fn)
    assert bits(res[0], dd.NAMES) == bits(res[1], dd.NAMES) and res[0]["policy_rows"] == 32.0 and res[0]["expert_rows"] == 5.0


# ------------------------------------------------------------------------------------------------- learners
def test_gail_dyn_learner_world_diagnostics_at_world_2(sg):
    """two updates of GailDynLearner.update(diagnostics="world", disc_diagnostics="world") per rank, on the 7 x 16 discriminator
    and the (5, 2, 8) policy: the published results are the same on both ranks and carry the global row counts; losses and
    parameters are those of the same run with the diagnostics off, bit for bit"""
    from simgan_amd.driver import ExpertLoader, GailDynLearner
    world, c = wd.policy_case("mlp_7x11_w2")
    T, Ng, F, Hd, n_e, B = c["T"], c["N"], 7, 16, 64, 16
    rng = np.random.default_rng(5)
    feat = rng.standard_normal((T + 1, Ng, F)).astype(np.float32)
    expert = rng.standard_normal((n_e, F)).astype(np.float32)

    def run(flag):
        def rank_fn(rank, ctx):
            ctx.set_disc_dp(False)
            s = wd.policy_shard(c, rank, world)
            n = s["N"]
            pol = make_policy(sg, s, ctx)
            ro = make_rollout(sg, s, ctx, F=F, obs_feat=np.ascontiguousarray(feat[:, rank * n:(rank + 1) * n]))
            disc, agent = sg.algo.gail.Discriminator(F, Hd, None, ctx=ctx, seed=2), ppo(sg, pol, epochs=2, mb=2)
            agent.seed, disc.seed = 1234, 77          # the streams that must agree across ranks are seeded explicitly
            learner = GailDynLearner(pol, agent, disc, ro, ExpertLoader(expert, B), gail_batch_size=B, gail_epoch=2, gail_tar_length=5.0)
            out = []
            for _ in range(2):
                losses = dict(learner.update(diagnostics=flag, disc_diagnostics=flag))     # (the ring is read in the rank's own thread)
                out.append(dict(losses={k: int(np.float32(v).view(np.uint32)) for k, v in losses.items()}, diag=learner.last_diagnostics,
                                ddiag=learner.last_disc_diagnostics))
            return out, pol.get_flat_params(), disc.get_flat_params()
        return run_ranks(world, rank_fn)

    off, on = run(False), run("world")
    for rank in range(world):
        for u in range(2):
            assert off[rank][0][u]["losses"] == on[rank][0][u]["losses"] and len(on[rank][0][u]["losses"]) == 7, (rank, u)
            assert off[rank][0][u]["diag"] is None and off[rank][0][u]["ddiag"] is None
        assert np.array_equal(off[rank][1].view(np.uint32), on[rank][1].view(np.uint32)), "policy parameters"
        assert np.array_equal(off[rank][2].view(np.uint32), on[rank][2].view(np.uint32)), "discriminator parameters"
    for u in range(2):
        a, b = on[0][0][u], on[1][0][u]
        assert tuple(a["diag"]) == dg.NAMES and tuple(a["ddiag"]) == ("before", "after")
        assert bits(a["diag"], dg.NAMES) == bits(b["diag"], dg.NAMES), (u, a["diag"], b["diag"])
        assert a["diag"]["rows"] == float(T * Ng) and all(np.isfinite(a["diag"][k]) for k in dg.NAMES)
        for half in ("before", "after"):
            assert tuple(a["ddiag"][half]) == dd.NAMES
            assert bits(a["ddiag"][half], dd.NAMES) == bits(b["ddiag"][half], dd.NAMES), (u, half, a["ddiag"][half], b["ddiag"][half])
            assert a["ddiag"][half]["policy_rows"] == float(T * Ng) and a["ddiag"][half]["expert_rows"] == float(n_e)
        assert bits(a["ddiag"]["before"], dd.NAMES) != bits(a["ddiag"]["after"], dd.NAMES)
    assert bits(on[0][0][0]["diag"], dg.NAMES) != bits(on[0][0][1]["diag"], dg.NAMES), "the second update publishes a new result"
