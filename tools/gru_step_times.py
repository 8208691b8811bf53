"""Microseconds per optimizer step and per update of PPO through time (recurrent Policy, GRU base) at T=128 x N=512 with 16
minibatches (32 environments x 128 steps = 4096 rows per step), obs 47 / act 12 / h64, and at the Hopper shape (obs 11, act 3,
T=128 x N=64, 4 minibatches), beside the feed-forward PPO step over the same rows measured in the same process.
Each update is bracketed by two device timestamps on the library's stream (sg_ctx_mark) after a synchronise; the rollouts
are device-resident, the update is queued without fetching its losses and the spread is read after the loop.
Run on the GPU box:  python tools/gru_step_times.py [updates] [--json PATH] [--trace-only]
(--trace-only: a few updates of the recurrent north-star case and nothing else, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402

SHAPES = [("northstar_T128_N512_M16", 47, 12, 64, 128, 512, 16), ("hopper_T128_N64_M4", 11, 3, 64, 128, 64, 4)]


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


def _mark(lib, ctx):
    i = C.c_int(0)
    _lib.check(lib.sg_ctx_mark(ctx.h, C.byref(i)))
    return i.value


def time_updates(agent, ro, ctx, updates, steps, warmup=3):
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
    med = 1e3 * float(np.median(times))
    return dict(update_us_median=round(med, 2), update_us_min=round(1e3 * float(np.min(times)), 2),
                update_us_max=round(1e3 * float(np.max(times)), 2), step_us_median=round(med / steps, 2), steps=steps, updates=updates)


def problem(O, A, H, T, N, recurrent):
    """A rollout collected with the policy itself (one act call per step over all N environments), 1 % episode ends."""
    rng = np.random.default_rng(0)
    pol = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": recurrent, "hidden_size": H}, seed=0)
    ro = sg.RolloutStorage(T, N, (O,), Box((A,)), pol.recurrent_hidden_state_size, 1)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    ro.obs[0].copy_(ro.obs.new_tensor(f32(N, O)))
    one = ro.obs.new_tensor(np.ones((N, 1), np.float32))
    for step in range(T):
        v, a, lp, h = pol.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
        masks = ro.obs.new_tensor((rng.random((N, 1)) > 0.01).astype(np.float32))
        ro.insert(ro.obs.new_tensor(f32(N, O)), h if recurrent else ro.recurrent_hidden_states[step], a, lp, v, ro.obs.new_tensor(f32(N, 1)),
                  masks, one)
    nv = pol.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1])
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    ro.sync_to_device()
    ro.device_resident = True   # as tools/a2c_step_times.py: no field crosses PCIe inside a bracketed update
    return pol, ro


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    updates = int(args[0]) if args else 20
    ctx = _lib.Context.default()
    if "--trace-only" in sys.argv:
        name, O, A, H, T, N, M = SHAPES[0]
        pol, ro = problem(O, A, H, T, N, True)
        agent = sg.algo.PPO(pol, 0.2, 1, M, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
        for _ in range(5):
            agent.update(ro)
        ctx.synchronize()
        return
    out = {"timing": "device timestamps around each queued update (sg_ctx_mark); ppo_epoch 1; device-resident rollouts in both columns",
           "bracket": "the update's launches (advantages, the captured graph of gathers and steps); the recurrent column also holds the "
                      "hand-over of the N x H states of slot 0 (a host memcpy into a page-locked slot and one asynchronous copy)"}
    for name, O, A, H, T, N, M in SHAPES:
        res = dict(obs=O, act=A, hidden=H, T=T, N=N, num_mini_batch=M, rows_per_step=T * (N // M))
        for key, rec in (("recurrent", True), ("feed_forward", False)):
            pol, ro = problem(O, A, H, T, N, rec)
            agent = sg.algo.PPO(pol, 0.2, 1, M, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
            res[key] = time_updates(agent, ro, ctx, updates, M)
            del agent, pol, ro
        res["recurrent_over_feed_forward"] = round(res["recurrent"]["step_us_median"] / res["feed_forward"]["step_us_median"], 2)
        out[name] = res
        print(name, res, flush=True)
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
