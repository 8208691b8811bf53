"""Times of A2C on the CNN base (Policy on [4, 84, 84] frames, Hs = 512, Discrete(6): the Atari shape of the a2c_ppo_acktr package)
beside the same network and loss in eager PyTorch on the same GPU, and beside this tree's PPO optimizer step.

  a2c update   one A2C_ACKTR(cnn=True).update on a device-resident rollout -- forward, loss, backward over all T * N rows, norm,
               clip, RMSprop -- between two device timestamps (sg_ctx_mark) / two torch.cuda events, queued without reading the
               losses inside the bracket; at T = 5 x N = 16 (80 rows, the reference's default) and T = 128 x N = 8 (1024 rows)
  ppo step     PPO.update at T = 128 x N = 8 with 4 epochs x 4 minibatches, over its 16 steps: 256 rows per step
  chunk table  the A2C update at T = 128 x N = 64 (8192 rows) with SG_A2C_CNN_CHUNK_ROWS = 256 ... 4096, and the scratch each
               chunk size needs (sg_cnn_fwd_floats + sg_cnn_bwd_floats + the head stacks of csrc/sg_cnn.hip, restated here)
Every figure: WARMUP unrecorded repeats, then the median, minimum and maximum of the recorded ones.
The torch network is written here with torch.nn (Conv2d / Linear / ReLU as a2c/model.py:211-220 describes it).
SG_A2C_CNN_RECORD-style parity is not this tool's: tests/test_gpu_a2c_cnn.py writes profiles/a2c_cnn_parity.json.
Run on the GPU box:  python tools/a2c_cnn_step_times.py [repeats] [--json PATH] [--no-chunks]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402

CH, HS, K = 4, 512, 6
VCOEF, ECOEF, LR, EPS, ALPHA, MAXN = 0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5
WARMUP = 3
CHUNKS = (256, 512, 1024, 2048, 4096)


class Discrete:
    def __init__(self, n):
        self.n = n


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return dict(median_us=round(1e3 * float(np.median(ms)), 1), min_us=round(1e3 * float(ms.min()), 1), max_us=round(1e3 * float(ms.max()), 1),
                repeats=int(ms.size))


def _mark(lib, ctx):
    i = C.c_int(0)
    _lib.check(lib.sg_ctx_mark(ctx.h, C.byref(i)))
    return i.value


def scratch_bytes(chunk):
    """csrc/sg_cnn.hip's sizes for one chunk: head stacks 2 * 16 floats a row, activations, their gradients, loss rows, slabs"""
    def slabs(rows):
        return max(1, min(32, (rows + 511) // 512))
    act = 32 * 20 * 20 + 64 * 9 * 9 + 1568 + HS
    slab = max(slabs(chunk * 400) * 32 * (CH * 64 + 1), slabs(chunk * 81) * 64 * 513, slabs(chunk * 49) * 32 * 577, slabs(chunk) * HS * 1569)
    return 4 * (chunk * (2 * 16 + 2 * act + (K + 1) + 1 + 3) + slab + 16)


def timed_updates(ctx, agent, ro, repeats):
    lib = ctx.lib
    for _ in range(WARMUP):
        agent.update(ro)
    ctx.synchronize()
    marks = []
    for _ in range(repeats):
        m0 = _mark(lib, ctx)
        agent.update(ro, fetch_losses=False)
        marks.append((m0, _mark(lib, ctx)))
    out = []
    for m0, m1 in marks:
        ms = C.c_double(0.0)
        _lib.check(lib.sg_ctx_mark_elapsed(ctx.h, m0, m1, C.byref(ms)))
        out.append(ms.value)
    _lib.check(lib.sg_ctx_mark(ctx.h, None))
    return stats(out)


def rollout(T, N, seed):
    rng = np.random.default_rng(seed)
    ro = sg.RolloutStorage(T, N, (CH, 84, 84), Discrete(K), 1, 1)
    frames = rng.integers(0, 256, (T + 1, N, CH, 84, 84), dtype=np.uint8)
    ro.obs.copy_(torch.from_numpy(frames))
    fields = dict(actions=rng.integers(0, K, (T, N, 1)), returns=rng.standard_normal((T + 1, N, 1)).astype(np.float32),
                  value_preds=rng.standard_normal((T + 1, N, 1)).astype(np.float32),
                  action_log_probs=np.full((T, N, 1), -np.log(K), np.float32) + 0.1 * rng.standard_normal((T, N, 1)).astype(np.float32))
    for k, v in fields.items():
        getattr(ro, k).copy_(torch.from_numpy(v))
    ro.sync_to_device()
    ro.device_resident = True
    return ro, frames, fields


def library_a2c(ctx, ro, repeats):
    pol = sg.Policy((CH, 84, 84), Discrete(K), seed=0)
    agent = sg.algo.A2C_ACKTR(pol, VCOEF, ECOEF, lr=LR, eps=EPS, alpha=ALPHA, max_grad_norm=MAXN, cnn=True)
    return timed_updates(ctx, agent, ro, repeats)


def library_ppo(ctx, ro, repeats):
    pol = sg.Policy((CH, 84, 84), Discrete(K), seed=0)
    agent = sg.algo.PPO(pol, 0.1, 4, 4, VCOEF, ECOEF, lr=2.5e-4, eps=EPS, max_grad_norm=MAXN)
    return timed_updates(ctx, agent, ro, repeats)


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


def eager_torch_a2c(frames, fields, T, N, repeats):
    dev = torch.device("cuda")
    net = TorchPolicy().to(dev)
    opt = torch.optim.RMSprop(net.parameters(), LR, eps=EPS, alpha=ALPHA)
    rows = torch.from_numpy(frames[:-1].reshape(T * N, CH, 84, 84)).to(dev).float()
    actions = torch.from_numpy(fields["actions"]).to(dev).reshape(-1).long()
    ret = torch.from_numpy(fields["returns"][:-1]).to(dev).reshape(-1)

    def update():      # a2c/algo/a2c_acktr.py:52-102
        v, d = net(rows)
        adv = ret - v[:, 0]
        value_loss = adv.pow(2).mean()
        action_loss = -(adv.detach() * d.log_prob(actions)).mean()
        opt.zero_grad()
        (value_loss * VCOEF + action_loss - d.entropy().mean() * ECOEF).backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), MAXN)
        opt.step()

    for _ in range(WARMUP):
        update()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        update()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return stats(out)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 10
    if not torch.cuda.is_available():
        raise SystemExit("tools/a2c_cnn_step_times.py measures on the GPU; no device here")
    os.environ.pop("SG_A2C_CNN_CHUNK_ROWS", None)
    ctx = _lib.Context.default()
    out = {"shape": dict(channels=CH, hidden=HS, actions=K),
           "timing": f"device timestamps around one queued update on a device-resident rollout; {WARMUP} warm-up repeats, then median / "
                     "min / max; eager torch: torch.cuda events around the same update in torch.nn on the same GPU"}
    for T, N in ((5, 16), (128, 8)):
        ro, frames, fields = rollout(T, N, seed=T)
        lib_t = library_a2c(ctx, ro, repeats)
        th_t = eager_torch_a2c(frames, fields, T, N, repeats)
        rec = dict(rows=T * N, library=lib_t, eager_torch=th_t, torch_over_library=round(th_t["median_us"] / lib_t["median_us"], 3),
                   library_us_per_row=round(lib_t["median_us"] / (T * N), 2))
        if (T, N) == (128, 8):
            ppo = library_ppo(ctx, ro, repeats)
            out["ppo_step_256_rows"] = dict(update=ppo, step_us_median=round(ppo["median_us"] / 16, 1),
                                            us_per_row=round(ppo["median_us"] / 16 / 256, 2), parent_measured_step_us=2104)
        out[f"a2c_update_{T}x{N}"] = rec
        del ro
        torch.cuda.empty_cache()
    if "--no-chunks" not in sys.argv:
        T, N = 128, 64
        ro, _, _ = rollout(T, N, seed=3)
        table = []
        for chunk in CHUNKS:
            os.environ["SG_A2C_CNN_CHUNK_ROWS"] = str(chunk)
            t = library_a2c(ctx, ro, max(3, repeats // 2))
            table.append(dict(chunk_rows=chunk, chunks=(T * N + chunk - 1) // chunk, scratch_mb=round(scratch_bytes(chunk) / 1e6, 1), **t,
                              us_per_row=round(t["median_us"] / (T * N), 2)))
        os.environ.pop("SG_A2C_CNN_CHUNK_ROWS")
        out["chunk_table_128x64"] = dict(rows=T * N, table=table)
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
