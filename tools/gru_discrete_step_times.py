"""Microseconds per optimizer step of PPO through time and per update of A2C through time on a recurrent Policy (GRU base) with
a Categorical (K = 18) and a Bernoulli (n = 12) head, beside the Gaussian (A = 12) recurrent policy, all in one process:
obs 47, h64, T=128 x N=512; PPO with 16 minibatches (32 environments x 128 steps = 4096 rows per step), A2C on the whole rollout.
Each update is bracketed by two device timestamps on the library's stream (sg_ctx_mark), as tools/gru_step_times.py takes them;
the rollouts are device-resident, the update is queued without fetching its losses and the spread is read after the loop.
Run on the GPU box:  python tools/gru_discrete_step_times.py [updates] [--json PATH] [--trace-only]
(--trace-only: a few PPO and A2C updates of the Categorical policy and nothing else, for `rocprofv3 --kernel-trace --stats -- python ...`)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from gru_step_times import Box, time_updates  # noqa: E402
from simgan_amd import _lib  # noqa: E402

O, H, T, N, M = 47, 64, 128, 512, 16


class Discrete:
    def __init__(self, n):
        self.n = int(n)


class MultiBinary:
    def __init__(self, n):
        self.n, self.shape = int(n), (int(n),)


HEADS = [("gaussian_A12", Box((12,))), ("categorical_K18", Discrete(18)), ("bernoulli_n12", MultiBinary(12))]


def problem(space):
    """A rollout collected with the policy itself (one act call per step over all N environments), 1 % episode ends; the hidden
    states live on the device beside the fields (enable_device_hidden), so no state crosses PCIe inside a bracketed update"""
    rng = np.random.default_rng(0)
    pol = sg.Policy((O,), space, base_kwargs={"recurrent": True, "hidden_size": H}, seed=0, recurrent_heads=True)
    ro = sg.RolloutStorage(T, N, (O,), space, pol.recurrent_hidden_state_size, 1)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    ro.obs[0].copy_(ro.obs.new_tensor(f32(N, O)))
    one = ro.obs.new_tensor(np.ones((N, 1), np.float32))
    for step in range(T):
        v, a, lp, h = pol.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
        masks = ro.obs.new_tensor((rng.random((N, 1)) > 0.01).astype(np.float32))
        ro.insert(ro.obs.new_tensor(f32(N, O)), h, a, lp, v, ro.obs.new_tensor(f32(N, 1)), masks, one)
    nv = pol.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1])
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    ro.sync_to_device()
    ro.device_resident = True
    ro.enable_device_hidden()
    return pol, ro


def agents(pol):
    return (("ppo", M, lambda: sg.algo.PPO(pol, 0.2, 1, M, 0.5, 0.01, lr=3e-4, eps=1e-5, max_grad_norm=0.5)),
            ("a2c", 1, lambda: sg.algo.A2C_ACKTR(pol, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, recurrent=True)))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    updates = int(args[0]) if args else 20
    ctx = _lib.Context.default()
    if "--trace-only" in sys.argv:
        pol, ro = problem(HEADS[1][1])
        for _, _, make in agents(pol):
            agent = make()
            for _ in range(5):
                agent.update(ro)
            ctx.synchronize()
            del agent
        return
    out = {"timing": "device timestamps around each queued update (sg_ctx_mark), medians; device-resident rollouts that hold their hidden "
                     "states; ppo: ppo_epoch 1, step = update / 16; a2c: one update is one optimizer step over all 65,536 rows",
           "shape": dict(obs=O, hidden=H, T=T, N=N, ppo_num_mini_batch=M, ppo_rows_per_step=T * (N // M))}
    for name, space in HEADS:
        pol, ro = problem(space)
        res = {}
        for algo, steps, make in agents(pol):
            agent = make()
            res[algo] = time_updates(agent, ro, ctx, updates, steps)
            del agent
        out[name] = res
        print(name, res, flush=True)
        del pol, ro
    for algo in ("ppo", "a2c"):
        g = out[HEADS[0][0]][algo]["step_us_median"]
        out[algo + "_step_over_gaussian"] = {name: round(out[name][algo]["step_us_median"] / g, 3) for name, _ in HEADS[1:]}
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
