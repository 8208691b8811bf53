"""What the world scope of the two diagnostics families costs over the rank scope, on one device, in one process: the queued rank
scope (k_*_diag, fold + finalise) against the queued world scope (k_*_diag, fold alone, the float64 all-gather of the ranks'
folded records -- 128 bytes per rank for the policy, 288 for the discriminator --, fold + finalise over them) on a ONE-RANK
communicator, the arrangement profiles/r06_comm_floor_n1.json used for the all-reduce floor.  Each call lies between two
timestamps the device takes on the library's stream (sg_ctx_mark: device time; the host does not wait inside the bracket); the
host's wall time until the call returns is beside it.  Medians of REPS = 20 after a warm-up, with min and max.
Shapes: the north-star ones of tools/diag_times.py and tools/disc_diag_times.py -- Policy (47, 12, h64) and the (86, 100)
discriminator with the benchmark's 100,000 expert rows, on a 128 x 512 rollout.
--comm rccl (default): ncclCommInitRank(world = 1); if that communicator cannot be created the record says so and the loopback
form is timed instead.  --comm loopback: the one-host transport, which synchronises the stream inside every collective -- a
test transport, NOT a performance path; its numbers say what the tests pay, nothing about a real run.
One rank says nothing about the wait for peers either: with world > 1 the all-gather completes when the slowest rank arrives.
Run on the GPU box:  python tools/world_diag_times.py [--comm rccl|loopback] [--json PATH]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402

REPS, WARMUP = 20, 3
T, N, O, A, H = 128, 512, 47, 12, 64
F, HD, NE = 86, 100, 100000


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def spread(ts):
    ts = np.asarray(ts, np.float64)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4), "n": int(ts.size)}


def stream_ms(ctx, fn):
    ts, wall = [], []
    for i in range(WARMUP + REPS):
        ctx.synchronize()
        t0 = time.perf_counter()
        a = ctx.mark()
        fn()
        b = ctx.mark()
        t1 = time.perf_counter()
        ctx.synchronize()
        if i >= WARMUP:
            ts.append(ctx.mark_elapsed(a, b))
            wall.append((t1 - t0) * 1e3)
        ctx.marks_reset()
    return spread(ts), spread(wall)


def both_scopes(ctx, queue, fetch, names):
    """queue(scope) queues one call, fetch() reads it -> the two scopes' times and whether their bits agree (one rank: they must)"""
    out, bits = {}, {}
    for scope in ("rank", "world", "rank", "world"):      # each scope twice, alternating: the second pass is the one kept
        queue(scope)
        got = fetch()
        bits[scope] = [int(np.float64(got[k]).view(np.uint64)) for k in names]
        s, w = stream_ms(ctx, lambda: queue(scope))
        fetch()
        out[scope] = {"queued_stream": s, "queued_host_wall_until_return": w}
    out["world_minus_rank_stream_median_ms"] = round(out["world"]["queued_stream"]["median_ms"] - out["rank"]["queued_stream"]["median_ms"], 4)
    out["world_scope_bits_equal_rank_scope"] = bits["rank"] == bits["world"]
    return out


def measure(ctx):
    rng = np.random.default_rng(0)
    pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H}, seed=0, ctx=ctx)
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, F, ctx=ctx)
    ro.obs.copy_(ro.obs.new_tensor(rng.standard_normal(tuple(ro.obs.shape)).astype(np.float32)))
    ro.obs_feat.copy_(ro.obs_feat.new_tensor(rng.standard_normal(tuple(ro.obs_feat.shape)).astype(np.float32)))
    ro.actions.copy_(ro.actions.new_tensor(rng.standard_normal((T, N, A)).astype(np.float32)))
    v, lp, _, _ = pol.evaluate_actions(ro.obs[:-1].reshape(T * N, O), ro.recurrent_hidden_states[0], ro.masks[:-1].reshape(T * N, 1),
                                       ro.actions.reshape(T * N, A))
    ro.action_log_probs.copy_(lp.reshape(T, N, 1))
    ro.value_preds[:-1].copy_(v.reshape(T, N, 1))
    ro.returns[:-1].copy_(v.reshape(T, N, 1) + ro.returns.new_tensor(0.5 * rng.standard_normal((T, N, 1)).astype(np.float32)))
    flat = pol.get_flat_params()
    pol.set_flat_params((flat + 0.01 * np.abs(flat).mean() * rng.standard_normal(flat.size)).astype(np.float32))
    ro.device_resident = True
    ro.sync_to_device()
    agent = sg.algo.PPO(pol, 0.2, 10, 32, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    disc = sg.algo.gail.Discriminator(F, HD, None, seed=0, ctx=ctx)
    disc.set_expert(rng.standard_normal((NE, F)).astype(np.float32))
    from simgan_amd.algo import diagnostics as diag
    return {"policy": dict(both_scopes(ctx, lambda scope: agent.diagnostics(ro, fetch=False, scope=scope), agent.last_diagnostics, diag.NAMES),
                           shape={"T": T, "N": N, "rows": T * N, "obs": O, "act": A, "hidden": H, "gathered_bytes_per_rank": 128}),
            "discriminator": dict(both_scopes(ctx, lambda scope: (disc.diagnostics_world if scope == "world" else disc.diagnostics)(ro, fetch=False), disc.last_diagnostics,
                                              diag.DISC_NAMES),
                                  shape={"T": T, "N": N, "policy_rows": T * N, "input_dim": F, "hidden_dim": HD, "expert_rows": NE,
                                         "gathered_bytes_per_rank": 288})}


def main():
    want = sys.argv[sys.argv.index("--comm") + 1] if "--comm" in sys.argv else "rccl"
    if want not in ("rccl", "loopback"):
        raise SystemExit(f"--comm {want}: rccl or loopback")
    ctx = _lib.Context(0)
    out = {"timing": f"sg_ctx_mark timestamps on the library's stream around each queued call (device time), medians of {REPS} after "
                     f"{WARMUP} warm-up calls, both scopes alternating in one process; host wall time by time.perf_counter until the call returns",
           "device": ctx.device_info()[0], "world": 1}
    if want == "rccl":
        try:
            ctx.comm_init(_lib.comm_unique_id(), 0, 1)          # ncclCommInitRank(world = 1)
        except _lib.SimganHipError as exc:
            out["rccl_one_rank_communicator"] = f"could not be created: {str(exc)[:300]}"
            ctx, want = _lib.Context(0), "loopback"
    if want == "loopback":
        ctx.comm_init(_lib.comm_loopback_id(), 0, 1)
        out["not_a_performance_path"] = ("the loopback transport copies through host memory and synchronises the stream inside every "
                                         "collective: these numbers are what the tests pay, not what a run over RCCL pays")
    out["communicator"] = ctx.comm_kind()
    out.update(measure(ctx))
    for k in ("policy", "discriminator"):
        print(k, out[k], flush=True)
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
