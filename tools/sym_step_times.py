"""Milliseconds per PPO update at the refinement shape (bench.py --workload refine: T=128, N=256, obs 111, act 12, h64,
ppo_epoch 10, num_mini_batch 8) with the mirror-symmetry loss off, on through the Laikago matrices (all on the device) and on
through per-row callables (the host mirrors the rollout once per update and uploads it).
Run on the GPU box:  python tools/sym_step_times.py [updates] [--json PATH]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402
from simgan_amd.symmetry import laikago_mirror  # noqa: E402

W = dict(T=128, N=256, O=111, A=12, H=64, E=10, M=8, clip=0.1, lr=1.5e-4, coef=1.0)


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def time_mode(mode, updates, warmup=2):
    m_obs, m_act = laikago_mirror(W["O"])
    pol = sg.Policy((W["O"],), Box((W["A"],)), base_kwargs={"recurrent": False, "hidden_size": W["H"]}, seed=0)
    kw = {}
    if mode == "matrix":
        kw = dict(symmetry_coef=W["coef"], mirror_obs=m_obs, mirror_act=m_act)
    elif mode == "callable":
        mo, ma = m_obs.astype(np.float64), m_act.astype(np.float64)
        kw = dict(symmetry_coef=W["coef"], mirror_obs=lambda x: list(mo @ np.asarray(x, np.float64)),
                  mirror_act=lambda x: list(ma @ np.asarray(x, np.float64)))
    agent = sg.algo.PPO(pol, W["clip"], W["E"], W["M"], 0.5, 0.0, lr=W["lr"], eps=1e-5, max_grad_norm=0.5, **kw)
    ro = sg.RolloutStorage(W["T"], W["N"], (W["O"],), Box((W["A"],)), 1, 1)
    ro.device_resident = True
    lib = _lib.load()
    _lib.check(lib.sg_rollout_fill_synthetic(ro.h, pol.h, 1234, 0.01))
    _lib.check(lib.sg_rollout_compute_returns_policy(ro.h, pol.h, 1, 0.99, 0.95, 1))
    for _ in range(warmup):
        agent.update(ro)
    times = []
    for _ in range(updates):
        t0 = time.perf_counter()
        agent.update(ro)        # returns after the losses are on the host: the whole update, host work included
        times.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_median=round(float(np.median(times)), 3), ms_min=round(float(np.min(times)), 3),
                ms_max=round(float(np.max(times)), 3), updates=updates, last_symmetry_loss=agent.last_symmetry_loss)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    updates = int(args[0]) if args else 10
    out = {"shape": W, "optimizer_steps_per_update": W["E"] * W["M"]}
    for mode in ("off", "matrix", "callable"):
        out[mode] = time_mode(mode, updates)
        print(mode, out[mode], flush=True)
    for mode in ("matrix", "callable"):
        out[f"{mode}_over_off"] = round(out[mode]["ms_median"] / out["off"]["ms_median"], 3)
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
