"""Microseconds per ACKTR update (A2C_ACKTR, acktr=True) at three shapes: T=5 x N=16 (a2c/arguments.py's defaults), T=1000 x N=8
(the Hopper scripts' rollout) and T=128 x N=512 (the north-star rollout), obs 47, act 12, h64; beside A2C (acktr=False) on
the same rows in the same process.  An ACKTR update whose step count is a multiple of Tf = 10 also refreshes the eigenbases
(k_kfac_eig); those updates are reported apart from the others.
Each update is bracketed by two device timestamps on the library's stream (sg_ctx_mark) after a synchronise; the update is
queued without a host wait (fetch_losses=False) and the spread is read after the loop.
Run on the GPU box:  python tools/acktr_step_times.py [updates] [--json PATH]"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import a2c_step_times as a2t  # noqa: E402
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402


def time_acktr(agent, ro, ctx, updates, warmup=3):
    """-> (no-refresh stats, refresh stats): update k of the agent refreshes when k % Tf == 0."""
    lib = ctx.lib
    for _ in range(warmup):
        agent.update(ro)
    ctx.synchronize()
    first = agent.get_kfac()["steps"]
    marks = []
    for _ in range(updates):
        m0 = a2t._mark(lib, ctx)
        agent.update(ro, fetch_losses=False)
        marks.append((m0, a2t._mark(lib, ctx)))
    plain, refresh = [], []
    for i, (m0, m1) in enumerate(marks):
        ms = C.c_double(0.0)
        _lib.check(lib.sg_ctx_mark_elapsed(ctx.h, m0, m1, C.byref(ms)))
        (refresh if (first + i) % agent.optimizer.Tf == 0 else plain).append(ms.value)
    _lib.check(lib.sg_ctx_mark(ctx.h, None))

    def stats(t):
        return dict(us_median=round(1e3 * float(np.median(t)), 2), us_min=round(1e3 * float(np.min(t)), 2),
                    us_max=round(1e3 * float(np.max(t)), 2), updates=len(t))
    return stats(plain), stats(refresh)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    updates = int(args[0]) if args else 40
    ctx = _lib.Context.default()
    out = {"obs": a2t.O, "act": a2t.A, "hidden": a2t.H, "Tf": 10,
           "timing": "device timestamps around each queued update (sg_ctx_mark)"}
    for name, T, N in a2t.SHAPES:
        pol, ro = a2t.problem(T, N)
        agent = sg.algo.A2C_ACKTR(pol, 0.5, 0.01, acktr=True)
        plain, refresh = time_acktr(agent, ro, ctx, updates)
        pol2, ro2 = a2t.problem(T, N)
        a2c = sg.algo.A2C_ACKTR(pol2, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
        base = a2t.time_updates(a2c, ro2, ctx, updates)
        out[name] = dict(rows=T * N, acktr=plain, acktr_eigen_refresh=refresh, a2c=base,
                         acktr_over_a2c=round(plain["us_median"] / base["us_median"], 3),
                         refresh_extra_us=round(refresh["us_median"] - plain["us_median"], 2))
        print(name, out[name], flush=True)
        del agent, pol, ro, a2c, pol2, ro2
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
