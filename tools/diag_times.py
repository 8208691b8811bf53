"""What the update diagnostics cost on the device, against the host route they replace, in one process:
  * queued:      PPO.diagnostics(rollouts, fetch=False) on a device-resident rollout -- the GRU forward for a recurrent policy,
                 k_policy_diag, k_policy_diag_reduce -- between two timestamps the device takes on the library's stream
                 (sg_ctx_mark: device time; the host does not wait inside the bracket);
  * host route:  Policy.evaluate_actions on all T*N rows through the host (rows up, value and log-prob rows down), then the ten
                 statistics in numpy from the host tensors -- the same two stream timestamps around the evaluate call (what the
                 update loop's stream is occupied or idle for) and the host's wall time around evaluate + numpy (what the loop's
                 host thread loses, on top of the wait that the queued form does not have);
  * beside them: that update's own time (agent.update(fetch_losses=False), stream timestamps), from the same run.
Shapes: north-star (Policy, 128 x 512, obs 47, act 12, h64), Hopper's SplitPolicy (128 x 256, obs 14, act 7, h100, one foot), and
the recurrent Policy (47, 12, 64) at 128 x 512.  Medians of REPS = 20 after a warm-up, with min and max beside them.
Run on the GPU box:  python tools/diag_times.py [--json PATH]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402

REPS, WARMUP = 20, 3
# name -> (kind, T, N, O, A, H, feet, ppo_epoch, num_mini_batch)
SHAPES = {"northstar_mlp_47_12_h64": ("mlp", 128, 512, 47, 12, 64, 1, 10, 32),
          "hopper_split_14_7_h100": ("split", 128, 256, 14, 7, 100, 1, 10, 16),
          "recurrent_gru_47_12_h64": ("gru", 128, 512, 47, 12, 64, 1, 1, 16)}


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def spread(ts):
    ts = np.asarray(ts, np.float64)
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(ts.min()), 4), "max_ms": round(float(ts.max()), 4), "n": int(ts.size)}


def host_route(pol, ro, clip):
    """evaluate_actions through the host, then the statistics in numpy -> the ten numbers"""
    T, N = ro.num_steps, ro.num_processes
    v, lp, ent, _ = pol.evaluate_actions(ro.obs[:-1].reshape(T * N, -1), ro.recurrent_hidden_states[0], ro.masks[:-1].reshape(T * N, 1),
                                         ro.actions.reshape(T * N, -1))
    v, lp = v.numpy().reshape(-1).astype(np.float64), lp.numpy().reshape(-1).astype(np.float64)
    lpo = ro.action_log_probs.numpy().reshape(-1).astype(np.float64)
    vp, ret = (x.numpy()[:-1].reshape(-1).astype(np.float64) for x in (ro.value_preds, ro.returns))
    r = np.exp(lp - lpo)
    return {"rows": float(r.size), "approx_kl": float(np.mean(lpo - lp)), "approx_kl_k3": float(np.mean((r - 1.0) - np.log(r))),
            "clip_fraction": float(np.mean(np.abs(r - 1.0) > clip)), "entropy": float(ent), "ratio_min": float(r.min()),
            "ratio_max": float(r.max()), "explained_variance_old": float(1.0 - np.var(ret - vp) / np.var(ret)),
            "explained_variance_new": float(1.0 - np.var(ret - v) / np.var(ret)), "value_mse": float(np.mean((ret - v) ** 2))}


def measure(kind, T, N, O, A, H, feet, E, M):
    if kind == "split":
        pol = sg.SplitPolicy((O,), Box((A,)), base_kwargs={"hidden_size": H, "num_feet": feet}, seed=0)
    else:
        pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": kind == "gru", "hidden_size": H}, seed=0)
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), H if kind == "gru" else 1, 1)
    rng = np.random.default_rng(0)
    ro.obs.copy_(ro.obs.new_tensor(rng.standard_normal(tuple(ro.obs.shape)).astype(np.float32)))
    if kind == "gru":
        ro.masks[1:T].copy_(ro.masks.new_tensor((rng.random((T - 1, N, 1)) > 0.02).astype(np.float32)))
    # the collection's own numbers: evaluate the behaviour policy, then move the policy a little so the ratios are not all 1
    actions = rng.standard_normal((T, N, A)).astype(np.float32)
    ro.actions.copy_(ro.actions.new_tensor(actions))
    v, lp, _, _ = pol.evaluate_actions(ro.obs[:-1].reshape(T * N, O), ro.recurrent_hidden_states[0], ro.masks[:-1].reshape(T * N, 1),
                                       ro.actions.reshape(T * N, A))
    ro.action_log_probs.copy_(lp.reshape(T, N, 1))
    ro.value_preds[:-1].copy_(v.reshape(T, N, 1))
    ro.returns[:-1].copy_(v.reshape(T, N, 1) + ro.returns.new_tensor(0.5 * rng.standard_normal((T, N, 1)).astype(np.float32)))
    flat = pol.get_flat_params()
    pol.set_flat_params((flat + 0.01 * np.abs(flat).mean() * rng.standard_normal(flat.size)).astype(np.float32))
    ro.device_resident = True
    ro.sync_to_device()
    if kind == "gru":
        ro.enable_device_hidden()
    agent = sg.algo.PPO(pol, 0.2, E, M, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    ctx = ro.ctx
    dev = agent.diagnostics(ro)
    host = host_route(pol, ro, 0.2)
    agree = {k: [dev[k], host[k]] for k in dev}

    def stream_ms(fn, sync_after=False):
        ts, wall = [], []
        for i in range(WARMUP + REPS):
            ctx.synchronize()
            t0 = time.perf_counter()
            a = ctx.mark()
            fn()
            b = ctx.mark()
            if sync_after:
                ctx.synchronize()
            t1 = time.perf_counter()
            if i >= WARMUP:
                ts.append(ctx.mark_elapsed(a, b))
                wall.append((t1 - t0) * 1e3)
            ctx.marks_reset()
        return ts, wall

    q_ts, q_wall = stream_ms(lambda: agent.diagnostics(ro, fetch=False))
    agent.last_diagnostics()
    h_ts, h_wall = stream_ms(lambda: host_route(pol, ro, 0.2))
    out = {"T": T, "N": N, "rows": T * N, "obs": O, "act": A, "hidden": H,
           "queued_diagnostics_stream": spread(q_ts), "queued_diagnostics_host_wall_until_return": spread(q_wall),
           "host_route_stream": spread(h_ts), "host_route_host_wall": spread(h_wall)}
    # the update itself, last: it moves the parameters (the diagnostics above saw one fixed policy)
    u_ts, _ = stream_ms(lambda: agent.update(ro, fetch_losses=False))
    out["update_stream"] = spread(u_ts)
    out["update"] = f"PPO.update, ppo_epoch {E}, {M} minibatches"
    q = out["queued_diagnostics_stream"]["median_ms"]
    out["host_route_wall_over_queued_stream"] = round(out["host_route_host_wall"]["median_ms"] / q, 1)
    out["queued_stream_share_of_update"] = round(q / out["update_stream"]["median_ms"], 4)
    out["device_vs_host_numbers"] = agree
    return out


def main():
    out = {"timing": f"sg_ctx_mark timestamps on the library's stream around each call (device time), medians of {REPS} after {WARMUP} "
                     "warm-up calls, one process; host wall time by time.perf_counter where a route makes the host wait",
           "device": sg._lib.Context.default().device_info()[0]}
    for name, spec in SHAPES.items():
        out[name] = measure(*spec)
        print(name, {k: v for k, v in out[name].items() if k != "device_vs_host_numbers"}, flush=True)
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
