"""Microseconds per update of A2C through time (A2C_ACKTR(..., recurrent=True): one forward and one reverse scan over all N
environments) at T=128 x N=512, obs 47 / act 12 / h64, and at the Hopper shape (obs 11, act 3, T=128 x N=64), beside -- measured
in the same process -- one epoch of PPO through time over the same rows (16 / 4 minibatches: a scan pair per minibatch) and the
feed-forward A2C update of the same shape.
Each update is bracketed by two device timestamps on the library's stream (sg_ctx_mark) after a synchronise; the rollouts are
device-resident (the recurrent ones hold their hidden states on the device: the hand-over of slot 0 is a device copy), the
update is queued without fetching its losses and the spread is read after the loop.
Run on the GPU box:  python tools/a2c_rnn_step_times.py [updates] [--json PATH] [--trace-only]
(--trace-only: a few updates of the recurrent north-star case and nothing else, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402
from gru_step_times import problem, time_updates  # noqa: E402

SHAPES = [("northstar_T128_N512", 47, 12, 64, 128, 512, 16), ("hopper_T128_N64", 11, 3, 64, 128, 64, 4)]
A2C = dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)


def recurrent_problem(O, A, H, T, N):
    pol, ro = problem(O, A, H, T, N, True)
    ro.enable_device_hidden()
    return pol, ro


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    updates = int(args[0]) if args else 20
    ctx = _lib.Context.default()
    if "--trace-only" in sys.argv:
        name, O, A, H, T, N, M = SHAPES[0]
        pol, ro = recurrent_problem(O, A, H, T, N)
        agent = sg.algo.A2C_ACKTR(pol, 0.5, 0.01, recurrent=True, **A2C)
        for _ in range(5):
            agent.update(ro)
        ctx.synchronize()
        return
    out = {"timing": "device timestamps around each queued update (sg_ctx_mark); device-resident rollouts in every column, hidden states "
                     "on the device in the recurrent ones",
           "bracket": "the update's launches: the hand-over of slot 0 (one device copy) and the captured graph"}
    for name, O, A, H, T, N, M in SHAPES:
        res = dict(obs=O, act=A, hidden=H, T=T, N=N, rows=T * N)
        pol, ro = recurrent_problem(O, A, H, T, N)
        res["a2c_recurrent"] = time_updates(sg.algo.A2C_ACKTR(pol, 0.5, 0.01, recurrent=True, **A2C), ro, ctx, updates, 1)
        del pol, ro
        pol, ro = recurrent_problem(O, A, H, T, N)
        res["ppo_recurrent_one_epoch"] = dict(time_updates(sg.algo.PPO(pol, 0.2, 1, M, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5),
                                                           ro, ctx, updates, M), num_mini_batch=M)
        del pol, ro
        pol, ro = problem(O, A, H, T, N, False)
        res["a2c_feed_forward"] = time_updates(sg.algo.A2C_ACKTR(pol, 0.5, 0.01, **A2C), ro, ctx, updates, 1)
        del pol, ro
        res["ppo_epoch_over_a2c_recurrent"] = round(res["ppo_recurrent_one_epoch"]["update_us_median"] / res["a2c_recurrent"]["update_us_median"], 2)
        res["a2c_recurrent_over_feed_forward"] = round(res["a2c_recurrent"]["update_us_median"] / res["a2c_feed_forward"]["update_us_median"], 2)
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
