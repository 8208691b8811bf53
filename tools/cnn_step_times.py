"""Times of the CNN base (Policy on [4, 84, 84] frames, Hs = 512, Discrete(6): the Atari shape of the a2c_ppo_acktr package) beside
the same network and loss in eager PyTorch on the same GPU: T = 128 x N = 8, 4 epochs x 4 minibatches of 256 rows.

  act          policy.act on the 8 frames of one step, host frames in, host results out (a host clock around a call that ends in
               a synchronise); torch: the frames copied to the device, forward, Categorical sample, results copied back
  update       one PPO.update of 16 optimizer steps on a device-resident rollout, between two device timestamps (sg_ctx_mark) /
               two torch.cuda events, queued without reading the losses inside the bracket
  step         update / 16: forward, loss, backward, norm, clip, Adam on 256 rows, with its share of the advantages' pass
Every figure: WARMUP unrecorded repeats, then the median, minimum and maximum of the recorded ones.  The FLOP count is the
algorithm's, from the shapes: 15,281,152 per row forward (2 * rows * columns * K of the four GEMMs and the heads), the backward
adds the weight gradients (as much again) and the data gradients of every layer but conv1; the fraction of peak is that count
over the step's time over the fp32 MFMA peak (MI355X_MICROARCH: 157.3 TFLOP/s) -- a whole-step rate, not a kernel's.
The torch network is written here with torch.nn (Conv2d / Linear / ReLU as a2c/model.py:211-220 describes it).
Run on the GPU box:  python tools/cnn_step_times.py [repeats] [--json PATH]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402

CH, HS, K, T, N, E, M = 4, 512, 6, 128, 8, 4, 4
CLIP, VCOEF, ECOEF, LR, EPS, MAXN = 0.1, 0.5, 0.01, 2.5e-4, 1e-5, 0.5
WARMUP = 3
PEAK_FP32_MFMA = 157.3e12


class Discrete:
    def __init__(self, n):
        self.n = n


def flops_forward_per_row():
    gemms = [(400, 32, CH * 64), (81, 64, 32 * 16), (49, 32, 64 * 9), (1, HS, 1568), (1, 1 + K, HS)]
    return sum(2 * r * c * k for r, c, k in gemms)


def flops_step_per_row():
    f = flops_forward_per_row()
    conv1 = 2 * 400 * 32 * CH * 64
    return f + f + (f - conv1)      # forward, weight gradients, data gradients (none into the frames)


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(median_us=round(1e3 * float(np.median(ms)), 1), min_us=round(1e3 * float(ms.min()), 1), max_us=round(1e3 * float(ms.max()), 1),
                repeats=int(ms.size))


def _mark(lib, ctx):
    i = C.c_int(0)
    _lib.check(lib.sg_ctx_mark(ctx.h, C.byref(i)))
    return i.value


def library(frames, repeats):
    ctx = _lib.Context.default()
    lib = ctx.lib
    pol = sg.Policy((CH, 84, 84), Discrete(K), seed=0)
    ro = sg.RolloutStorage(T, N, (CH, 84, 84), Discrete(K), 1, 1)
    rng = np.random.default_rng(1)
    ro.obs.copy_(torch.from_numpy(frames))
    for step in range(T):
        v, a, lp, _ = pol.act(ro.obs[step], None, None)
        ro.actions[step].copy_(a); ro.action_log_probs[step].copy_(lp); ro.value_preds[step].copy_(v)
    ro.rewards.copy_(torch.from_numpy(rng.standard_normal((T, N, 1)).astype(np.float32)))
    ro.masks.copy_(torch.from_numpy((rng.random((T + 1, N, 1)) > 0.01).astype(np.float32)))
    ro.compute_returns(pol.get_value(ro.obs[-1], None, None), True, 0.99, 0.95, True)
    ro.sync_to_device()
    ro.device_resident = True
    act = []
    for i in range(WARMUP + repeats):
        t0 = time.perf_counter()
        pol.act(ro.obs[i % T], None, None)
        act.append(1e3 * (time.perf_counter() - t0))
    agent = sg.algo.PPO(pol, CLIP, E, M, VCOEF, ECOEF, lr=LR, eps=EPS, max_grad_norm=MAXN)
    for _ in range(WARMUP):
        agent.update(ro)
    ctx.synchronize()
    marks = []
    for _ in range(repeats):
        m0 = _mark(lib, ctx)
        agent.update(ro, fetch_losses=False)
        marks.append((m0, _mark(lib, ctx)))
    upd = []
    for m0, m1 in marks:
        ms = C.c_double(0.0)
        _lib.check(lib.sg_ctx_mark_elapsed(ctx.h, m0, m1, C.byref(ms)))
        upd.append(ms.value)
    _lib.check(lib.sg_ctx_mark(ctx.h, None))
    fields = {k: getattr(ro, k).numpy().copy() for k in ("actions", "action_log_probs", "value_preds", "returns")}
    return stats(act[WARMUP:]), stats(upd), fields


class TorchPolicy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.main = nn.Sequential(nn.Conv2d(CH, 32, 8, stride=4), nn.ReLU(), nn.Conv2d(32, 64, 4, stride=2), nn.ReLU(),
                                  nn.Conv2d(64, 32, 3, stride=1), nn.ReLU(), nn.Flatten(), nn.Linear(32 * 7 * 7, HS), nn.ReLU())
        self.critic_linear = nn.Linear(HS, 1)
        self.dist_linear = nn.Linear(HS, K)

    def forward(self, x):
        f = self.main(x / 255.0)
        return self.critic_linear(f), torch.distributions.Categorical(logits=self.dist_linear(f))


def eager_torch(frames, fields, repeats):
    dev = torch.device("cuda")
    net = TorchPolicy().to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=LR, eps=EPS)
    obs = torch.from_numpy(frames).to(dev)
    act = []
    for i in range(WARMUP + repeats):
        x = torch.from_numpy(frames[i % T])
        t0 = time.perf_counter()
        with torch.no_grad():
            v, d = net(x.to(dev))
            a = d.sample()
            out = (v.cpu(), a.cpu(), d.log_prob(a).cpu())
        act.append(1e3 * (time.perf_counter() - t0))
    del out
    f = {k: torch.from_numpy(v).to(dev) for k, v in fields.items()}
    rows = obs[:-1].reshape(T * N, CH, 84, 84)
    actions, old_lp = f["actions"].reshape(-1).long(), f["action_log_probs"].reshape(-1)
    vpred, ret = f["value_preds"][:-1].reshape(-1), f["returns"][:-1].reshape(-1)

    def update():
        adv = ret - vpred
        adv = (adv - adv.mean()) / (adv.std() + 1e-5)
        mb = T * N // M
        for _ in range(E):
            perm = torch.randperm(T * N, device=dev)
            for k in range(M):
                idx = perm[k * mb:(k + 1) * mb]
                v, d = net(rows[idx])
                v = v[:, 0]
                lp, ent = d.log_prob(actions[idx]), d.entropy().mean()
                ratio = torch.exp(lp - old_lp[idx])
                s1, s2 = ratio * adv[idx], torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv[idx]
                action_loss = -torch.min(s1, s2).mean()
                vc = vpred[idx] + (v - vpred[idx]).clamp(-CLIP, CLIP)
                value_loss = 0.5 * torch.max((v - ret[idx]).pow(2), (vc - ret[idx]).pow(2)).mean()
                opt.zero_grad()
                (value_loss * VCOEF + action_loss - ent * ECOEF).backward()
                torch.nn.utils.clip_grad_norm_(net.parameters(), MAXN)
                opt.step()

    for _ in range(WARMUP):
        update()
    torch.cuda.synchronize()
    upd = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        update()
        e1.record()
        e1.synchronize()
        upd.append(e0.elapsed_time(e1))
    return stats(act[WARMUP:]), stats(upd)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 10
    if not torch.cuda.is_available():
        raise SystemExit("tools/cnn_step_times.py measures on the GPU; no device here")
    frames = np.random.default_rng(0).integers(0, 256, (T + 1, N, CH, 84, 84)).astype(np.float32)
    lib_act, lib_upd, fields = library(frames, repeats)
    th_act, th_upd = eager_torch(frames, fields, repeats)
    steps, mb = E * M, T * N // M
    step_flop = flops_step_per_row() * mb

    def with_step(u):
        s = u["median_us"] / steps
        return dict(update=u, step_us_median=round(s, 1), step_tflops=round(step_flop / (s * 1e-6) / 1e12, 2),
                    fraction_of_fp32_mfma_peak=round(step_flop / (s * 1e-6) / PEAK_FP32_MFMA, 4))

    out = {"shape": dict(channels=CH, hidden=HS, actions=K, T=T, N=N, ppo_epoch=E, num_mini_batch=M, rows_per_step=mb),
           "timing": "act: host clock around the call (host frames in, host results out); update: device timestamps around one queued "
                     f"update of {steps} steps; {WARMUP} warm-up repeats, then median / min / max",
           "flop_forward_per_row": flops_forward_per_row(), "flop_step_per_row": flops_step_per_row(), "peak_fp32_mfma_tflops": PEAK_FP32_MFMA / 1e12,
           "library": dict(act_n8=lib_act, **with_step(lib_upd)), "eager_torch": dict(act_n8=th_act, **with_step(th_upd)),
           "torch_over_library": dict(act=round(th_act["median_us"] / lib_act["median_us"], 3),
                                      update=round(th_upd["median_us"] / lib_upd["median_us"], 3))}
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
