"""Host wall time of the collection loop's policy step for a RECURRENT Policy through both paths, in one process:
  * per call: Policy.act (sg_policy_act_rnn: four launches, three to four copies up, four back) and RolloutStorage.act_step on a
    rollout that holds its hidden states (enable_device_hidden: one launch, two copies up, the actions written into page-locked
    host memory by the kernel), and the same with their insert / insert_env, at N = 8 / 256 / 512;
  * per collection: PpoLearner.collect at T=128 x N=512 against an environment that costs nothing, on_device False / True, each
    with its final upload, and the host->device bytes of one collection;
  * per update: PpoLearner.update on the device-resident rollout of each path -- until the call returns (the host path waits in
    get_value(obs[T], h[T], masks[T]) and reads hidden slot 0; the device path only queues) and until the device is done;
for the recurrent policies (obs 47, act 12, h64) and (obs 11, act 3, h64).  Medians over CALLS calls / COLLECTS collections /
UPDATES updates after a warm-up, with min, p10, p90 and max beside them (time.perf_counter; every act call ends in a stream wait,
so host wall time is the cost the collection loop sees).  The yardstick is the host path of the same run.
Run on the GPU box:  python tools/collect_rnn_times.py [calls] [--json PATH]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd.driver import PpoLearner  # noqa: E402

POLICIES = [("gru_policy_47_12_h64", 47, 12, 64), ("gru_policy_11_3_h64", 11, 3, 64)]
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


def make_policy(O, A, H):
    return sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": H}, seed=0)


def make_rollout(O, A, H, T, N, device_hidden):
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), H, O)
    ro.obs[0].copy_(ro.obs.new_tensor(np.random.default_rng(0).standard_normal((N, O)).astype(np.float32)))
    ro.device_resident = True
    ro.sync_to_device()
    if device_hidden:
        ro.enable_device_hidden()
    return ro


def per_call(O, A, H, N, calls):
    pol = make_policy(O, A, H)
    host, dev = make_rollout(O, A, H, 8, N, False), make_rollout(O, A, H, 8, N, True)
    envs = FreeEnvs(N, O)
    one = host.obs.new_tensor(np.ones((N, 1), np.float32))

    def act():
        return pol.act(host.obs[host.step], host.recurrent_hidden_states[host.step], host.masks[host.step])

    def act_insert():
        v, a, lp, h = act()
        host.insert(envs.obs, h, a, lp, v, envs.reward, one, one, envs.obs)

    def step():
        return dev.act_step(pol)

    def step_insert():
        dev.act_step(pol)
        dev.insert_env(envs.obs, envs.reward, one, one, envs.obs)

    out = {}
    for name, fn in (("act", act), ("act_step", step), ("act_plus_insert", act_insert), ("act_step_plus_insert_env", step_insert)):
        out[name] = spread(timed(fn, calls, 30), 1e6, "us")
    return out


def collections_and_updates(O, A, H, n, n_updates, warmup=2):
    out = {}
    for key, on_device in (("host_path", False), ("on_device", True)):
        pol = make_policy(O, A, H)
        ro = make_rollout(O, A, H, T_COLLECT, N_COLLECT, on_device)
        agent = sg.algo.PPO(pol, 0.2, 1, 16, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
        learner, envs = PpoLearner(pol, agent, ro), FreeEnvs(N_COLLECT, O)
        before = ro.bytes_uploaded
        learner.collect(envs, on_device=on_device)
        nbytes = ro.bytes_uploaded - before
        res = spread(timed(lambda: learner.collect(envs, on_device=on_device), n, warmup), 1e3, "ms")   # noqa: B023
        res["host_to_device_bytes_per_collection"] = int(nbytes)
        out[f"collect_{key}"] = res
        # the update: until update() returns, and until the device has finished it (each update starts on an idle device)
        returned, done = [], []
        for i in range(warmup + n_updates):
            ro.ctx.synchronize()
            t0 = time.perf_counter()
            learner.update()
            t1 = time.perf_counter()
            ro.ctx.synchronize()
            t2 = time.perf_counter()
            if i >= warmup:
                returned.append(t1 - t0)
                done.append(t2 - t0)
        out[f"update_{key}"] = {"until_update_returns": spread(returned, 1e3, "ms"), "until_device_done": spread(done, 1e3, "ms")}
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--json" in sys.argv:
        args.remove(sys.argv[sys.argv.index("--json") + 1])
    calls = max(200, int(args[0])) if args else 300
    out = {"timing": "time.perf_counter around each call (each act ends in a stream wait); one process; medians with min / p10 / p90 / max",
           "collect": f"PpoLearner.collect, recurrent Policy, T={T_COLLECT} x N={N_COLLECT}, an environment that costs nothing, final upload included",
           "update": "PpoLearner.update on the device-resident rollout (ppo_epoch 1, 16 minibatches of 32 environments): host_path = host "
                     "get_value + host hand-over of hidden slot 0, on_device = enable_device_hidden()"}
    for name, O, A, H in POLICIES:
        res = {"obs": O, "act": A, "hidden": H}
        for N in ROWS:
            res[f"N{N}"] = per_call(O, A, H, N, calls)
            print(name, N, res[f"N{N}"], flush=True)
        res.update(collections_and_updates(O, A, H, 20, 20))
        print(name, {k: v for k, v in res.items() if k.startswith(("collect_", "update_"))}, flush=True)
        out[name] = res
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
