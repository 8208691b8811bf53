"""What the discriminator diagnostics cost on the device, against the host route they replace, in one process, at the north-star
shape (rollout 128 x 512, discriminator (86, 100), the benchmark's expert matrix of 100,000 rows):
  * queued:      Discriminator.diagnostics(rollouts, fetch=False) on a device-resident rollout -- k_disc_diag, k_disc_diag_reduce --
                 between two timestamps the device takes on the library's stream (sg_ctx_mark: device time; the host does not wait
                 inside the bracket), and the host's wall time until the call returns;
  * host route:  rollouts.sync_from_device(), predict_prob on the T*N policy rows and on the expert rows, the statistics in numpy, and
                 compute_grad_pen_combined (sg_disc_grad_pen: one scalar workgroup per row) on the T*N mixup rows at alpha = 0.5 --
                 the host's wall time around all of it, and of each part;
  * beside them: one discriminator epoch of the same update (update_gail_dyn(fetch_losses=False), stream timestamps), the yardstick
                 of what the feature costs.
Medians of REPS after a warm-up, with min and max beside them.
Run on the GPU box:  python tools/disc_diag_times.py [--json PATH]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd.driver import ExpertLoader  # noqa: E402

REPS, WARMUP, HOST_REPS = 20, 3, 5
T, N, F, HD, NE, B = 128, 512, 86, 100, 100000, 128


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def spread(ts):
    ts = np.asarray(ts, np.float64)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4), "n": int(ts.size)}


def host_route(disc, ro, expert, parts):
    """today's route to the same numbers -> a few of them; parts: {name: [ms]} of its stages"""
    t = [time.perf_counter()]
    ro.sync_from_device()
    t.append(time.perf_counter())
    policy = ro.obs_feat[1:].numpy().reshape(T * N, F)
    s_p = disc.predict_prob(policy).numpy().reshape(-1).astype(np.float64)
    s_e = disc.predict_prob(expert).numpy().reshape(-1).astype(np.float64)
    t.append(time.perf_counter())
    eps = float(np.float32(1e-7))
    rew = np.log(s_p + eps) - np.log(1.0 - s_p + eps)
    out = {"policy_accuracy": float((s_p < 0.5).mean()), "expert_accuracy": float((s_e > 0.5).mean()),
           "policy_bce": float(-np.log1p(-s_p).mean()), "expert_bce": float(-np.log(s_e).mean()),
           "reward_mean": float(rew.mean()), "reward_std": float(rew.std()), "reward_min": float(rew.min()), "reward_max": float(rew.max())}
    t.append(time.perf_counter())
    idx = np.arange(T * N) % expert.shape[0]
    pen = disc.compute_grad_pen_combined(expert[idx], policy, 10.0, alpha=np.full(T * N, 0.5, np.float32))
    out["mid_grad_pen"] = float(pen)
    t.append(time.perf_counter())
    for k, name in enumerate(("sync_from_device", "predict_prob_policy_and_expert", "numpy", "grad_pen_mid_rows")):
        parts.setdefault(name, []).append((t[k + 1] - t[k]) * 1e3)
    parts.setdefault("total", []).append((t[-1] - t[0]) * 1e3)
    return out


def main():
    rng = np.random.default_rng(0)
    disc = sg.algo.gail.Discriminator(F, HD, None, seed=0)
    expert = rng.standard_normal((NE, F)).astype(np.float32)
    loader = ExpertLoader(expert, B)
    disc._bind_loader(loader)
    ro = sg.RolloutStorage(T, N, (47,), Box((12,)), 1, F)
    ro.obs_feat.copy_(ro.obs_feat.new_tensor(rng.standard_normal(tuple(ro.obs_feat.shape)).astype(np.float32)))
    ro.device_resident = True
    ro.sync_to_device()
    ctx = ro.ctx
    dev = disc.diagnostics(ro)
    parts = {}
    host = host_route(disc, ro, expert, parts)
    parts.clear()

    def stream_ms(fn):
        ts, wall = [], []
        for i in range(WARMUP + REPS):
            ctx.synchronize()
            t0 = time.perf_counter()
            a = ctx.mark()
            fn()
            b = ctx.mark()
            t1 = time.perf_counter()
            if i >= WARMUP:
                ts.append(ctx.mark_elapsed(a, b))
                wall.append((t1 - t0) * 1e3)
            ctx.marks_reset()
        return ts, wall

    q_ts, q_wall = stream_ms(lambda: disc.diagnostics(ro, fetch=False))
    disc.last_diagnostics()
    for _ in range(HOST_REPS):
        ctx.synchronize()
        host_route(disc, ro, expert, parts)
    # the epoch last: it moves the weights (the diagnostics above saw one fixed discriminator)
    e_ts, _ = stream_ms(lambda: disc.update_gail_dyn(loader, ro, fetch_losses=False))
    out = {"timing": f"sg_ctx_mark timestamps on the library's stream around each call (device time), medians of {REPS} after {WARMUP} "
                     f"warm-up calls, one process; the host route by time.perf_counter, {HOST_REPS} runs after one warm-up",
           "device": sg._lib.Context.default().device_info()[0],
           "shape": {"T": T, "N": N, "policy_rows": T * N, "input_dim": F, "hidden_dim": HD, "expert_rows": NE, "gail_batch": B},
           "queued_diagnostics_stream": spread(q_ts), "queued_diagnostics_host_wall_until_return": spread(q_wall),
           "host_route_host_wall": {k: spread(v) for k, v in parts.items()},
           "one_disc_epoch_stream": spread(e_ts), "one_disc_epoch_steps": int(disc.last_n_steps)}
    q = out["queued_diagnostics_stream"]["median_ms"]
    out["host_route_wall_over_queued_stream"] = round(out["host_route_host_wall"]["total"]["median_ms"] / q, 1)
    out["queued_stream_share_of_one_disc_epoch"] = round(q / out["one_disc_epoch_stream"]["median_ms"], 4)
    out["two_calls_share_of_the_five_epochs"] = round(2.0 * q / (5.0 * out["one_disc_epoch_stream"]["median_ms"]), 4)
    out["device_vs_host_numbers"] = {k: [dev[k], host[k]] for k in host}
    print({k: v for k, v in out.items() if k != "device_vs_host_numbers"}, flush=True)
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
