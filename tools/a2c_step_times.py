"""Milliseconds per A2C update (A2C_ACKTR, acktr=False) at three shapes: T=5 x N=16 (a2c/arguments.py's defaults), T=1000 x N=8
(the Hopper scripts' rollout) and T=128 x N=512 (the north-star rollout), obs 47, act 12, h64.  At the north-star shape the same
process also times one PPO epoch over the same rows (PPO with ppo_epoch 1, num_mini_batch 16: 16 optimizer steps of 4096 rows),
the work A2C's single step over all rows should not exceed.
Each update is bracketed by two device timestamps on the library's stream (sg_ctx_mark) after a synchronise; the update is
queued without a host wait (fetch_losses=False) and the spread is read after the loop.
Run on the GPU box:  python tools/a2c_step_times.py [updates] [--json PATH]"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402

O, A, H = 47, 12, 64
SHAPES = [("T5_N16", 5, 16), ("T1000_N8", 1000, 8), ("T128_N512", 128, 512)]


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _mark(lib, ctx):
    i = C.c_int(0)
    _lib.check(lib.sg_ctx_mark(ctx.h, C.byref(i)))
    return i.value


def time_updates(agent, ro, ctx, updates, warmup=3):
    lib = ctx.lib
    for _ in range(warmup):
        agent.update(ro)
    ctx.synchronize()
    marks = []
    for _ in range(updates):
        m0 = _mark(lib, ctx)
        agent.update(ro, fetch_losses=False)
        marks.append((m0, _mark(lib, ctx)))
    times = []
    for m0, m1 in marks:
        ms = C.c_double(0.0)
        _lib.check(lib.sg_ctx_mark_elapsed(ctx.h, m0, m1, C.byref(ms)))
        times.append(ms.value)
    _lib.check(lib.sg_ctx_mark(ctx.h, None))
    return dict(us_median=round(1e3 * float(np.median(times)), 2), us_min=round(1e3 * float(np.min(times)), 2),
                us_max=round(1e3 * float(np.max(times)), 2), updates=updates)


def problem(T, N):
    pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": False, "hidden_size": H}, seed=0)
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), 1, 1)
    ro.device_resident = True
    lib = pol.lib
    _lib.check(lib.sg_rollout_fill_synthetic(ro.h, pol.h, 1234, 0.01))
    _lib.check(lib.sg_rollout_compute_returns_policy(ro.h, pol.h, 1, 0.99, 0.95, 1))
    return pol, ro


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    updates = int(args[0]) if args else 20
    ctx = _lib.Context.default()
    out = {"obs": O, "act": A, "hidden": H, "timing": "device timestamps around each queued update (sg_ctx_mark)"}
    for name, T, N in SHAPES:
        pol, ro = problem(T, N)
        agent = sg.algo.A2C_ACKTR(pol, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
        out[name] = dict(rows=T * N, a2c=time_updates(agent, ro, ctx, updates))
        if name == "T128_N512":
            pol2, ro2 = problem(T, N)
            ppo = sg.algo.PPO(pol2, 0.2, 1, 16, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
            out[name]["ppo_epoch_16_steps"] = time_updates(ppo, ro2, ctx, updates)
            out[name]["a2c_over_ppo_epoch"] = round(out[name]["a2c"]["us_median"] / out[name]["ppo_epoch_16_steps"]["us_median"], 3)
            del ppo, pol2, ro2
        print(name, out[name], flush=True)
        del agent, pol, ro
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
