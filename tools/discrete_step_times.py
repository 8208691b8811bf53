"""Record what Policy on a Discrete action space costs on the GPU, and that the Box path's north-star figure did not move.

  python tools/discrete_step_times.py [--parent DIR] [--repeats 3] [--out profiles/discrete_step_times.json]

Part 1: Policy.act (sampling, the library's own draws) and one PPO update (ppo_epoch = 4, 16 minibatches) on a device-resident
rollout of T = 128 steps x N = 512 environments, obs 47, hidden 64 -- the north-star rollout with Discrete(2) and Discrete(18)
in place of its Box(12) -- timed with a host clock around work that ends in a stream synchronisation, after warm-up.  Recorded
only: there is no threshold on these numbers.

Part 2 (--parent DIR: a built tree of the parent commit): bench.py's north-star line from DIR and from this tree, alternating,
`--repeats` times each in this one call.  "unchanged" means: the difference of the two means lies inside the spread (max - min)
of the parent's own repeats."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_ARGS = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline", "--no-line-keeper"]


class Discrete:
    def __init__(self, n):
        self.n = int(n)


def step_times(K, T=128, N=512, O=47, H=64, E=4, M=16, iters=10):
    import numpy as np
    sys.path.insert(0, ROOT)
    import simgan_amd as sg
    space = Discrete(K)
    p = sg.Policy((O,), space, base_kwargs={"recurrent": False, "hidden_size": H}, seed=K)
    agent = sg.algo.PPO(p, 0.2, E, M, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    ro = sg.RolloutStorage(T, N, (O,), space, 1, 1)
    rng = np.random.default_rng(K)
    ro.obs.copy_(ro.obs.new_tensor(rng.standard_normal((T + 1, N, O)).astype(np.float32)))
    ro.rewards.copy_(ro.rewards.new_tensor(rng.standard_normal((T, N, 1)).astype(np.float32)))
    for t in range(T):
        v, a, lp, _ = p.act(ro.obs[t], None, None)
        ro.actions[t].copy_(a); ro.action_log_probs[t].copy_(lp); ro.value_preds[t].copy_(v)
    ro.compute_returns(p.get_value(ro.obs[-1], None, None), True, 0.99, 0.95, True)
    ro.sync_to_device()
    ro.device_resident = True
    ctx = p.ctx
    obs = ro.obs[0]

    def timed(fn, n):
        for _ in range(3):
            fn()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    act_ms = timed(lambda: p.act(obs, None, None), 50)
    upd_ms = timed(lambda: agent.update(ro, fetch_losses=False), iters)
    return {"K": K, "T": T, "N": N, "obs": O, "hidden": H, "ppo_epoch": E, "num_mini_batch": M,
            "act_ms_per_call_host_rows": round(act_ms, 4), "act_rows": N,
            "ppo_update_ms": round(upd_ms, 3), "ppo_step_us": round(upd_ms * 1e3 / (E * M), 2)}


def bench_line(tree):
    r = subprocess.run([sys.executable, "bench.py"] + BENCH_ARGS, cwd=tree, capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"bench.py in {tree} failed (rc {r.returncode}): {r.stderr[-2000:]}")
    d = json.loads(lines[-1])
    return {"value": d["value"], "ms_per_step": d["ms_per_step"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built tree of the parent commit: bench.py is run there and here, alternating")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "discrete_step_times.json"))
    a = ap.parse_args()
    doc = {"what": "tools/discrete_step_times.py: Policy.act and PPO step times on Discrete(2) / Discrete(18) at the north-star rollout "
                   "shape (recorded only, no threshold), and bench.py's north-star line at the parent commit and at this one",
           "step_times": [step_times(K) for K in (2, 18)]}
    if a.parent:
        runs = {"parent": [], "head": []}
        for _ in range(a.repeats):
            runs["parent"].append(bench_line(os.path.abspath(a.parent)))
            runs["head"].append(bench_line(ROOT))
        mean = lambda rs: sum(r["ms_per_step"] for r in rs) / len(rs)  # noqa: E731
        spread = max(r["ms_per_step"] for r in runs["parent"]) - min(r["ms_per_step"] for r in runs["parent"])
        diff = mean(runs["head"]) - mean(runs["parent"])
        doc["north_star"] = {"bench_args": " ".join(BENCH_ARGS), "order": "parent, head, alternating", "runs": runs,
                             "parent_mean_ms_per_step": round(mean(runs["parent"]), 4), "head_mean_ms_per_step": round(mean(runs["head"]), 4),
                             "head_minus_parent_ms": round(diff, 4), "parent_spread_ms": round(spread, 4),
                             "inside_parent_spread": bool(abs(diff) <= spread)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
