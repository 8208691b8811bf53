"""Time of one environment step's policy work: the chained call (RolloutStorage.act_step_chain) against the two-call sequence
it replaces -- PolicyEnsemble.act, a host tanh and concat, RolloutStorage.act_step -- at N = 512 environments.

    python tools/act_chain_times.py [--out profiles/act_chain_times.json] [--runs 12] [--steps 300]

Shapes: the Hopper GAIL-dyn stage (behaviour policy 11 -> 3, learner SplitPolicy 14 -> 7), the Laikago GAIL-dyn stage (behaviour
policy 52 -> 12, learner SplitPolicy 64 -> 28) and the Hopper refinement stage (learner Policy 11 -> 3, K = 5 dynamics policies
14 -> 7 drawn per row).  Per shape and path: `runs` windows of `steps` calls each, the two paths alternating window by window in
one process; a window is timed with the host clock and every call in it ends in a stream synchronisation inside the library, so
the figure is the host-visible time per environment step (launch, copies and wait included, the environment itself excluded).
Median, minimum and maximum over the windows, in microseconds per step.  Launches, copies and host waits per step are counted
from the launchers' code (csrc/sg_policy.hip, sg_act_step.hip, sg_act_chain.hip), not measured.  Both paths produce the same
bits (tests/test_gpu_act_chain.py); the squash of the two-call path here is numpy's tanh, as the reference's is torch's."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 512
COUNTS = {   # per environment step
    "inner_first": {"two_call": {"launches": 2, "h2d_copies": 3, "d2h_copies": 3, "host_waits": 2},
                    "chained": {"launches": 1, "h2d_copies": 1, "d2h_copies": 0, "host_waits": 1}},
    "learner_first": {"two_call": {"launches": 2, "h2d_copies": 3, "d2h_copies": 3, "host_waits": 2},
                      "chained": {"launches": 1, "h2d_copies": 2, "d2h_copies": 0, "host_waits": 1}},
}


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def policy(sg, kind, O, A, seed):
    if kind == "mlp":
        p = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": 64}, seed=seed)
    else:
        p = sg.SplitPolicy((O,), Box((A,)), base_kwargs={"hidden_size": 64, "num_feet": A // 7}, seed=seed)
    rng = np.random.default_rng(seed)
    p.set_flat_params((0.3 * rng.standard_normal(p.get_flat_params().size)).astype(np.float32))
    return p


def shape_case(sg, name, order, learner, member, K):
    from simgan_amd import _lib
    from simgan_amd.ensemble import PolicyEnsemble
    pol = policy(sg, *learner, seed=1)
    ens = PolicyEnsemble([policy(sg, *member, seed=10 + k) for k in range(K)])
    O, A = learner[1], learner[2]
    ro = sg.RolloutStorage(4, N, (O,), Box((A,)), 1, 0)
    ro.device_resident = True
    rng = np.random.default_rng(0)
    ind = rng.integers(0, K, size=N).astype(np.int32)
    inner_first = order == "inner_first"
    state = rng.standard_normal((N, member[1] if inner_first else O)).astype(np.float32)
    if not inner_first:
        ro.obs[0].copy_(ro.obs.new_tensor(state))

    def two_call():
        if inner_first:
            a, _ = ens.act(state, ind=ind)
            ro.obs[0].copy_(ro.obs.new_tensor(np.concatenate([state, np.tanh(a)], axis=1)))
            return ro.act_step(pol)
        act = ro.act_step(pol)
        return ens.act(np.concatenate([state, np.tanh(act.numpy())], axis=1), ind=ind)[0]

    def chained():
        if inner_first:
            return ro.act_step_chain(pol, ens, _lib.CHAIN_INNER_FIRST, state=state, ind=ind)
        return ro.act_step_chain(pol, ens, _lib.CHAIN_LEARNER_FIRST, ind=ind)

    return {"name": name, "order": order, "K": K, "learner": list(learner), "member": list(member), "two_call": two_call,
            "chained": chained}


def window(fn, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act_chain_times.json"))
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--steps", type=int, default=300)
    args = ap.parse_args()
    assert args.runs >= 10, "at least 10 windows per path"
    import simgan_amd as sg
    cases = [shape_case(sg, "hopper_gail_dyn", "inner_first", ("split", 14, 7), ("mlp", 11, 3), 1),
             shape_case(sg, "laikago_gail_dyn", "inner_first", ("split", 64, 28), ("mlp", 52, 12), 1),
             shape_case(sg, "hopper_refinement_K5", "learner_first", ("mlp", 11, 3), ("split", 14, 7), 5)]
    doc = {"what": "tools/act_chain_times.py: host-visible microseconds per environment step of the policies' work at N = 512, chained "
                   "call vs the two-call sequence, windows alternating in one process; counts per step are read off the launchers",
           "N": N, "runs": args.runs, "steps_per_window": args.steps, "cases": {}}
    for c in cases:
        for fn in (c["two_call"], c["chained"]):           # warm up both paths: code objects, staging buffers
            window(fn, 50)
        t = {"two_call": [], "chained": []}
        for _ in range(args.runs):
            for path in ("two_call", "chained"):
                t[path].append(window(c[path], args.steps))
        rec = {"order": c["order"], "K": c["K"], "learner": c["learner"], "member": c["member"]}
        for path in ("two_call", "chained"):
            rec[path] = {"median_us": round(statistics.median(t[path]), 2), "min_us": round(min(t[path]), 2),
                         "max_us": round(max(t[path]), 2), **COUNTS[c["order"]][path]}
        rec["chained_over_two_call_median"] = round(rec["chained"]["median_us"] / rec["two_call"]["median_us"], 4)
        doc["cases"][c["name"]] = rec
        print(c["name"], json.dumps(rec))
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
