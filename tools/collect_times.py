"""Host wall time of the collection loop's policy step through both paths, in one process:
  * per call: Policy.act (two launches, three copies back) and RolloutStorage.act_step (one launch, the actions written into
    page-locked host memory by the kernel), and the same with their insert / insert_env, at N = 8 / 256 / 512;
  * per collection: PpoLearner.collect at T=128 x N=512 against an environment that costs nothing, on_device False / True, each
    with its final upload, and the host->device bytes of one collection;
for the north-star Policy (obs 47, act 12, h64) and the Laikago SplitPolicy (obs 64, act 28, h100, 4 feet).  Medians over CALLS
calls / COLLECTS collections after a warm-up, with min, p10, p90 and max beside them (time.perf_counter around each call: every
call ends in a stream wait, so host wall time is the cost the collection loop sees).
Run on the GPU box:  python tools/collect_times.py [calls] [--json PATH] [--trace-only]
(--trace-only: two collections per path of the north-star case and nothing else, for
 `rocprofv3 --kernel-trace --stats -- python tools/collect_times.py --trace-only`)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd.driver import PpoLearner  # noqa: E402

POLICIES = [("northstar_policy_47_12_h64", "mlp", 47, 12, 64, 1), ("laikago_split_64_28_h100_f4", "split", 64, 28, 100, 4)]
ROWS = (8, 256, 512)
T_COLLECT, N_COLLECT = 128, 512


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


class FreeEnvs:
    """step() hands back the same arrays every time: the loop's cost is the policy step and the rollout writes alone."""

    def __init__(self, N, O):
        rng = np.random.default_rng(1)
        self.obs = rng.standard_normal((N, O)).astype(np.float32)
        self.reward = np.zeros((N, 1), np.float32)
        self.done = np.zeros(N, bool)
        self.infos = [{} for _ in range(N)]

    def step(self, action):
        return self.obs, self.reward, self.done, self.infos


def spread(ts, scale, unit):
    ts = np.asarray(ts) * scale
    q = lambda p: round(float(np.percentile(ts, p)), 2)  # noqa: E731
    return {f"median_{unit}": q(50), f"min_{unit}": q(0), f"p10_{unit}": q(10), f"p90_{unit}": q(90), f"max_{unit}": q(100), "n": int(ts.size)}


def timed(fn, n, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def make(kind, O, A, H, feet, T, N):
    if kind == "mlp":
        pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H}, seed=0)
    else:
        pol = sg.SplitPolicy((O,), Box((A,)), base_kwargs={"hidden_size": H, "num_feet": feet}, seed=0)
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, O)
    ro.obs[0].copy_(ro.obs.new_tensor(np.random.default_rng(0).standard_normal((N, O)).astype(np.float32)))
    ro.device_resident = True
    ro.sync_to_device()
    return pol, ro


def per_call(kind, O, A, H, feet, N, calls):
    pol, ro = make(kind, O, A, H, feet, 8, N)
    envs = FreeEnvs(N, O)
    one = ro.obs.new_tensor(np.ones((N, 1), np.float32))
    hxs = ro.recurrent_hidden_states[0]

    def act():
        return pol.act(ro.obs[ro.step], hxs, ro.masks[ro.step])

    def act_insert():
        v, a, lp, h = act()
        ro.insert(envs.obs, h, a, lp, v, envs.reward, one, one, envs.obs)

    def step():
        return ro.act_step(pol)

    def step_insert():
        ro.act_step(pol)
        ro.insert_env(envs.obs, envs.reward, one, one, envs.obs)

    out = {}
    for name, fn in (("act", act), ("act_step", step), ("act_plus_insert", act_insert), ("act_step_plus_insert_env", step_insert)):
        out[name] = spread(timed(fn, calls, 30), 1e6, "us")
    return out


def collections(kind, O, A, H, feet, n, warmup=2):
    out = {}
    for key, on_device in (("collect_host_path", False), ("collect_on_device", True)):
        pol, ro = make(kind, O, A, H, feet, T_COLLECT, N_COLLECT)
        agent = sg.algo.PPO(pol, 0.2, 1, 16, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
        learner, envs = PpoLearner(pol, agent, ro), FreeEnvs(N_COLLECT, O)
        before = ro.bytes_uploaded
        learner.collect(envs, on_device=on_device)
        nbytes = ro.bytes_uploaded - before
        res = spread(timed(lambda: learner.collect(envs, on_device=on_device), n, warmup), 1e3, "ms")   # noqa: B023
        res["host_to_device_bytes_per_collection"] = int(nbytes)
        out[key] = res
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--json" in sys.argv:
        args.remove(sys.argv[sys.argv.index("--json") + 1])
    calls = max(200, int(args[0])) if args else 300
    if "--trace-only" in sys.argv:
        _, kind, O, A, H, feet = POLICIES[0]
        for on_device in (False, True):
            pol, ro = make(kind, O, A, H, feet, T_COLLECT, N_COLLECT)
            agent = sg.algo.PPO(pol, 0.2, 1, 16, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
            learner, envs = PpoLearner(pol, agent, ro), FreeEnvs(N_COLLECT, O)
            for _ in range(2):
                learner.collect(envs, on_device=on_device)
        ro.ctx.synchronize()
        return
    out = {"timing": "time.perf_counter around each call (each ends in a stream wait); one process; medians with min / p10 / p90 / max",
           "collect": f"PpoLearner.collect, T={T_COLLECT} x N={N_COLLECT}, an environment that costs nothing, final upload included"}
    for name, kind, O, A, H, feet in POLICIES:
        res = {"obs": O, "act": A, "hidden": H}
        for N in ROWS:
            res[f"N{N}"] = per_call(kind, O, A, H, feet, N, calls)
            print(name, N, res[f"N{N}"], flush=True)
        res.update(collections(kind, O, A, H, feet, 20))
        print(name, {k: res[k] for k in ("collect_host_path", "collect_on_device")}, flush=True)
        out[name] = res
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
