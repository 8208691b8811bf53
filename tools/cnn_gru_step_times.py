"""Times of the recurrent CNN base (Policy on [4, 84, 84] frames, Hs = 512, Discrete(6), base_kwargs={'recurrent': True}: the Atari
shape of the a2c_ppo_acktr package with --recurrent-policy): T = 128 x N = 8, 4 epochs x 4 minibatches of 2 whole environments
(256 rows, time-major) per optimizer step.  Measured against two things in the same process, the three alternating per repeat:

  recurrent    one PPO.update (16 steps) of this library's recurrent CNN policy on a device-resident rollout
  feedforward  the same library's feed-forward CNN policy on the same rollout: 16 steps of 256 permuted rows each
  eager_torch  the recurrent network written with torch.nn (Conv2d / Linear / ReLU / nn.GRU as a2c/model.py:117-230 describes it,
               the sequence cut where any mask is 0 as NNBase._forward_gru cuts it) with the same loss, clip and Adam

Every update is queued without reading its losses and timed between two device timestamps (sg_ctx_mark / torch.cuda events);
WARMUP unrecorded repeats, then the median, minimum and maximum of the recorded ones, per update and per optimizer step.
The per-kernel split is a separate run:  rocprofv3 --kernel-trace --stats -- python tools/cnn_gru_step_times.py 3 --library-only
Run on the GPU box:  python tools/cnn_gru_step_times.py [repeats] [--json PATH] [--library-only]"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simgan_amd as sg  # noqa: E402
from simgan_amd import _lib  # noqa: E402

CH, HS, K, T, N, E, M = 4, 512, 6, 128, 8, 4, 4
CLIP, VCOEF, ECOEF, LR, EPS, MAXN = 0.1, 0.5, 0.01, 2.5e-4, 1e-5, 0.5
WARMUP = 3


class Discrete:
    def __init__(self, n):
        self.n = n


def stats(ms):
    ms = np.asarray(ms, np.float64)
    steps = E * M
    return dict(update_median_us=round(1e3 * float(np.median(ms)), 1), update_min_us=round(1e3 * float(ms.min()), 1),
                update_max_us=round(1e3 * float(ms.max()), 1), step_median_us=round(1e3 * float(np.median(ms)) / steps, 1),
                step_min_us=round(1e3 * float(ms.min()) / steps, 1), step_max_us=round(1e3 * float(ms.max()) / steps, 1), repeats=int(ms.size))


def _mark(lib, ctx):
    i = C.c_int(0)
    _lib.check(lib.sg_ctx_mark(ctx.h, C.byref(i)))
    return i.value


def fill_rollout(pol, ro, frames, rng, recurrent):
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
    def __init__(self, frames, recurrent):
        self.ctx = _lib.Context.default()
        kw = dict(base_kwargs={"recurrent": True}, recurrent_cnn=True) if recurrent else {}
        self.pol = sg.Policy((CH, 84, 84), Discrete(K), seed=0, **kw)
        self.ro = sg.RolloutStorage(T, N, (CH, 84, 84), Discrete(K), HS if recurrent else 1, 1)
        fill_rollout(self.pol, self.ro, frames, np.random.default_rng(1), recurrent)
        self.agent = sg.algo.PPO(self.pol, CLIP, E, M, VCOEF, ECOEF, lr=LR, eps=EPS, max_grad_norm=MAXN)
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
    def __init__(self, frames, ro):
        dev = torch.device("cuda")
        self.dev = dev
        self.net = TorchPolicy().to(dev)
        self.opt = torch.optim.Adam(self.net.parameters(), lr=LR, eps=EPS)
        self.obs = torch.from_numpy(frames).to(dev)[:-1]
        g = lambda t: torch.from_numpy(np.ascontiguousarray(t.numpy())).to(dev)  # noqa: E731
        self.actions, self.old_lp = g(ro.actions)[..., 0].long(), g(ro.action_log_probs)[..., 0]
        self.vpred, self.ret, self.masks = g(ro.value_preds)[:-1, :, 0], g(ro.returns)[:-1, :, 0], g(ro.masks)[:-1, :, 0]
        self.h0 = g(ro.recurrent_hidden_states)[0]
        self.masks_host = ro.masks.numpy()[:-1, :, 0]
        self.times = []

    def update(self, record):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        adv = self.ret - self.vpred
        adv = (adv - adv.mean()) / (adv.std() + 1e-5)
        per = N // M
        for _ in range(E):
            perm = torch.randperm(N)
            for k in range(M):
                envs = perm[k * per:(k + 1) * per]
                ed = envs.to(self.dev)
                cuts = [int(t) for t in np.nonzero((self.masks_host[:, envs.numpy()] == 0).any(1))[0]]
                v, d = self.net(self.obs[:, ed].reshape(T * per, CH, 84, 84), self.h0[ed], self.masks[:, ed], cuts)
                v = v[:, 0]
                sel = lambda t: t[:, ed].reshape(-1)  # noqa: E731
                lp, ent = d.log_prob(sel(self.actions)), d.entropy().mean()
                ratio = torch.exp(lp - sel(self.old_lp))
                a = sel(adv)
                action_loss = -torch.min(ratio * a, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * a).mean()
                vp, rt = sel(self.vpred), sel(self.ret)
                vc = vp + (v - vp).clamp(-CLIP, CLIP)
                value_loss = 0.5 * torch.max((v - rt).pow(2), (vc - rt).pow(2)).mean()
                self.opt.zero_grad()
                (value_loss * VCOEF + action_loss - ent * ECOEF).backward()
                torch.nn.utils.clip_grad_norm_(self.net.parameters(), MAXN)
                self.opt.step()
        e1.record()
        e1.synchronize()
        if record:
            self.times.append(e0.elapsed_time(e1))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--") and a.isdigit()]
    repeats = int(args[0]) if args else 10
    if not torch.cuda.is_available():
        raise SystemExit("tools/cnn_gru_step_times.py measures on the GPU; no device here")
    frames = np.random.default_rng(0).integers(0, 256, (T + 1, N, CH, 84, 84)).astype(np.float32)
    rec = LibRun(frames, True)
    runs = [rec]
    if "--library-only" not in sys.argv:
        runs += [LibRun(frames, False), TorchRun(frames, rec.ro)]
    for i in range(WARMUP + repeats):
        for r in runs:      # alternating
            r.update(i >= WARMUP)
    rec.ctx.synchronize()
    out = {"shape": dict(channels=CH, hidden=HS, actions=K, T=T, N=N, ppo_epoch=E, num_mini_batch=M, rows_per_step=T * N // M),
           "timing": f"device timestamps around one queued update of {E * M} optimizer steps; {WARMUP} warm-up repeats, then median / min / max; "
                     "the configurations alternate within every repeat",
           "recurrent": stats(rec.times())}
    if len(runs) > 1:
        out["feedforward"] = stats(runs[1].times())
        out["eager_torch"] = stats(runs[2].times)
        out["recurrent_over_feedforward"] = round(out["recurrent"]["step_median_us"] / out["feedforward"]["step_median_us"], 3)
        out["torch_over_recurrent"] = round(out["eager_torch"]["step_median_us"] / out["recurrent"]["step_median_us"], 3)
    print(json.dumps(out))
    if "--json" in sys.argv:
        path = sys.argv[sys.argv.index("--json") + 1]
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
