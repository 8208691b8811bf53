"""Times of A2C through time on the recurrent CNN base (Policy on [4, 84, 84] frames, Hs = 512, Discrete(6), base_kwargs={'recurrent':
True}; A2C_ACKTR(..., recurrent_cnn=True)) at three rollouts: T = 5 x N = 16 (the reference's A2C default), 128 x 8
(one environment group) and 128 x 64 (two groups of 32 environments).  Each shape is measured beside three things in the same
process, the four alternating per repeat:

  a2c_through_time  one update of this library's A2C on the recurrent CNN policy, device-resident rollout
  ppo_one_epoch     one epoch of this library's PPO through time over the same rows of the same policy kind, in minibatches of
                    min(N, max(1, 256 // T)) whole environments (about 256 rows per optimizer step, section 4.20's shape)
  a2c_feedforward   this library's A2C on the feed-forward CNN base (cnn=True, section 4.18) on the same frames
  eager_torch       the recurrent network written with torch.nn incl. nn.GRU (the sequence cut where any mask is 0, as
                    NNBase._forward_gru cuts it), the same loss over all rows, clip_grad_norm_ and torch.optim.RMSprop

Every update is queued without reading its losses and timed between two device timestamps (sg_ctx_mark / torch.cuda events); WARMUP
unrecorded repeats, then the median, minimum and maximum of the recorded ones.
The per-kernel split is a separate run:  rocprofv3 --kernel-trace --stats -- python tools/a2c_cnn_gru_step_times.py 3 --library-only
Run on the GPU box:  python tools/a2c_cnn_gru_step_times.py [repeats] [--json PATH] [--library-only] [--shapes 5x16,128x8]"""
import ctypes as C
import gc
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402

CH, HS, K = 4, 512, 6
SHAPES = [(5, 16), (128, 8), (128, 64)]
VCOEF, ECOEF, LR, EPS, ALPHA, MAXN, CLIP = 0.5, 0.01, 7e-4, 1e-5, 0.99, 0.5, 0.1
WARMUP = 2


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


def fill_rollout(pol, ro, frames, rng, recurrent, T, N):
    ro.obs.copy_(torch.from_numpy(frames))
    ro.masks.copy_(torch.from_numpy((rng.random((T + 1, N, 1)) > 0.01).astype(np.float32)))
    for step in range(T):
        v, a, lp, h = pol.act(ro.obs[step], ro.recurrent_hidden_states[step] if recurrent else None, ro.masks[step] if recurrent else None)
        ro.actions[step].copy_(a); ro.action_log_probs[step].copy_(lp); ro.value_preds[step].copy_(v)
        if recurrent:
            ro.recurrent_hidden_states[step + 1].copy_(h)
    ro.rewards.copy_(torch.from_numpy(rng.standard_normal((T, N, 1)).astype(np.float32)))
    nv = pol.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1] if recurrent else None, ro.masks[-1] if recurrent else None)
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    ro.sync_to_device()
    ro.device_resident = True


class LibRun(object):
    """kind: "a2c_rnn" | "ppo_rnn" | "a2c_ff"; the two recurrent kinds share one rollout"""

    def __init__(self, kind, frames, T, N, ro=None):
        self.ctx = _lib.Context.default()
        recurrent = kind != "a2c_ff"
        kw = dict(base_kwargs={"recurrent": True}, recurrent_cnn=True) if recurrent else {}
        self.pol = sg.Policy((CH, 84, 84), Discrete(K), seed=0, **kw)
        self.ro = ro
        if ro is None:
            self.ro = sg.RolloutStorage(T, N, (CH, 84, 84), Discrete(K), HS if recurrent else 1, 1)
            fill_rollout(self.pol, self.ro, frames, np.random.default_rng(1), recurrent, T, N)
        if kind == "ppo_rnn":
            per = min(N, max(1, 256 // T))
            self.steps = N // per
            self.agent = sg.algo.PPO(self.pol, CLIP, 1, self.steps, VCOEF, ECOEF, lr=LR, eps=EPS, max_grad_norm=MAXN)
        else:
            self.steps = 1
            self.agent = sg.algo.A2C_ACKTR(self.pol, VCOEF, ECOEF, lr=LR, eps=EPS, alpha=ALPHA, max_grad_norm=MAXN,
                                           **(dict(recurrent_cnn=True) if recurrent else dict(cnn=True)))
        self.marks = []

    def update(self, record):
        lib = self.ctx.lib
        m0 = _mark(lib, self.ctx)
        self.agent.update(self.ro, fetch_losses=False)
        m1 = _mark(lib, self.ctx)
        if record:
            self.marks.append((m0, m1))

    def times(self):
        out = []
        for m0, m1 in self.marks:
            ms = C.c_double(0.0)
            _lib.check(self.ctx.lib.sg_ctx_mark_elapsed(self.ctx.h, m0, m1, C.byref(ms)))
            out.append(ms.value)
        return out


class TorchPolicy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.gru = nn.GRU(HS, HS)
        self.main = nn.Sequential(nn.Conv2d(CH, 32, 8, stride=4), nn.ReLU(), nn.Conv2d(32, 64, 4, stride=2), nn.ReLU(),
                                  nn.Conv2d(64, 32, 3, stride=1), nn.ReLU(), nn.Flatten(), nn.Linear(32 * 7 * 7, HS), nn.ReLU())
        self.critic_linear = nn.Linear(HS, 1)
        self.dist_linear = nn.Linear(HS, K)

    def forward(self, x, hxs, masks, cuts):
        """x [T n, C, 84, 84] time-major, hxs [n, Hs], masks [T, n]; cuts: the steps at which some mask is 0 (host list)"""
        n = hxs.shape[0]
        f = self.main(x / 255.0).view(-1, n, HS)
        h, outs = hxs.unsqueeze(0), []
        bounds = [0] + [c for c in cuts if c > 0] + [f.shape[0]]
        for a, b in zip(bounds[:-1], bounds[1:]):
            y, h = self.gru(f[a:b], h * masks[a].view(1, n, 1))
            outs.append(y)
        y = torch.cat(outs, 0).view(-1, HS)
        return self.critic_linear(y), torch.distributions.Categorical(logits=self.dist_linear(y))


class TorchRun(object):
    def __init__(self, frames, ro, T, N):
        dev = torch.device("cuda")
        self.T, self.N = T, N
        self.net = TorchPolicy().to(dev)
        self.opt = torch.optim.RMSprop(self.net.parameters(), LR, eps=EPS, alpha=ALPHA)
        self.obs = torch.from_numpy(frames).to(dev)[:-1].reshape(T * N, CH, 84, 84)
        g = lambda t: torch.from_numpy(np.ascontiguousarray(t.numpy())).to(dev)  # noqa: E731
        self.actions = g(ro.actions)[..., 0].long().reshape(-1)
        self.ret, self.masks = g(ro.returns)[:-1, :, 0].reshape(-1), g(ro.masks)[:-1, :, 0]
        self.h0 = g(ro.recurrent_hidden_states)[0]
        self.cuts = [int(t) for t in np.nonzero((ro.masks.numpy()[:-1, :, 0] == 0).any(1))[0]]
        self.times = []

    def update(self, record):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        v, d = self.net(self.obs, self.h0, self.masks, self.cuts)
        adv = self.ret - v[:, 0]
        value_loss = adv.pow(2).mean()
        action_loss = -(adv.detach() * d.log_prob(self.actions)).mean()
        self.opt.zero_grad()
        (value_loss * VCOEF + action_loss - d.entropy().mean() * ECOEF).backward()
        torch.nn.utils.clip_grad_norm_(self.net.parameters(), MAXN)
        self.opt.step()
        e1.record()
        e1.synchronize()
        if record:
            self.times.append(e0.elapsed_time(e1))


def measure(T, N, repeats, library_only):
    frames = np.random.default_rng(0).integers(0, 256, (T + 1, N, CH, 84, 84)).astype(np.float32)
    a2c = LibRun("a2c_rnn", frames, T, N)
    runs = [a2c]
    if not library_only:
        runs += [LibRun("ppo_rnn", frames, T, N, ro=a2c.ro), LibRun("a2c_ff", frames, T, N), TorchRun(frames, a2c.ro, T, N)]
    for i in range(WARMUP + repeats):
        for r in runs:      # alternating
            r.update(i >= WARMUP)
    a2c.ctx.synchronize()
    ne = max(1, min(N, 4096 // T))
    out = {"T": T, "N": N, "rows": T * N, "group_envs": ne, "groups": (N + ne - 1) // ne, "a2c_through_time": stats(a2c.times())}
    if not library_only:
        out["ppo_one_epoch"] = dict(stats(runs[1].times()), optimizer_steps=runs[1].steps)
        out["a2c_feedforward"] = stats(runs[2].times())
        out["eager_torch"] = stats(runs[3].times)
        m = out["a2c_through_time"]["median_us"]
        out["ppo_epoch_over_a2c"] = round(out["ppo_one_epoch"]["median_us"] / m, 3)
        out["a2c_over_feedforward"] = round(m / out["a2c_feedforward"]["median_us"], 3)
        out["torch_over_a2c"] = round(out["eager_torch"]["median_us"] / m, 3)
    del runs, a2c, frames
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    args = [a for a in sys.argv[1:] if a.isdigit()]
    repeats = int(args[0]) if args else 7
    if not torch.cuda.is_available():
        raise SystemExit("tools/a2c_cnn_gru_step_times.py measures on the GPU; no device here")
    shapes = SHAPES
    if "--shapes" in sys.argv:
        shapes = [tuple(int(v) for v in s.split("x")) for s in sys.argv[sys.argv.index("--shapes") + 1].split(",")]
    out = {"network": dict(channels=CH, hidden=HS, actions=K),
           "timing": f"device timestamps around one queued update; {WARMUP} warm-up repeats, then median / min / max in microseconds; "
                     "the configurations alternate within every repeat", "shapes": []}
    for T, N in shapes:
        out["shapes"].append(measure(T, N, repeats, "--library-only" in sys.argv))
        print(json.dumps(out["shapes"][-1]), flush=True)
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
