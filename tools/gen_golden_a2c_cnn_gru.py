"""Generate tests/golden/a2c_cnn_gru_{cat,box}.npz by running the reference's A2C_ACKTR(acktr=False) on its recurrent CNN base
(dev-only).

Drives the reference's own Policy with CNNBase(recurrent=True) (a2c/model.py:117-230) and A2C_ACKTR (a2c/algo/a2c_acktr.py:52-102)
through tools/ref_import.py on the CPU, as a2c/main.py:123-131 builds them with --recurrent-policy: C = 1, Hs = 16, Discrete(5) /
Box(3), T = 3, N = 4, two updates under update_linear_schedule (a2c/main.py:201-205), each on a fresh rollout collected act -> insert
by the policy the update before it left.  The masks have zeros (t = 0 of one environment, two consecutive steps of another) and the
hidden state of slot 0 is not zero.  Everything written is data: the parameters before the first update, the frames as uint8 (16 grey
levels, which the archive packs), actions, returns, masks, slot 0's hidden states, the learning rates, the loss triples, and of the
parameters and RMSprop's square_avg after each update every 5th element (tests/a2c_cnn_ref.py:sample_index) plus the last 256 (the
heads); the GRU's four tensors come first in the vector and are sampled like the rest.

Seeds are tried in order until, before each of the two updates, the rows keep clear of the ReLU kinks on the references alone
(tests/cnn_ref.py:kink_margin >= KINK_FACTOR at the parameters that update starts from), and the float32 results lie within a tenth
of the tests' tolerance of the float64 restatement (tests/a2c_cnn_gru_ref.py).
Re-run:
    python tools/gen_golden_a2c_cnn_gru.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import gen_golden as gg  # noqa: E402  (imports the reference)
import gen_golden_cnn_gru as ggr  # noqa: E402
from gen_golden_a2c import square_avg  # noqa: E402
from gen_golden_a2c_cnn import tenth  # noqa: E402
from gen_golden_cnn import images, space_of  # noqa: E402
import a2c_cnn_gru_ref as ref  # noqa: E402
import cnn_gru_ref as gr  # noqa: E402
import cnn_ref as cr  # noqa: E402
from third_party.a2c_ppo_acktr.algo.a2c_acktr import A2C_ACKTR  # noqa: E402  (the reference's, via ref_import)

ns = gg.ns
HW = 84
C, HS, T, N, ITERS, NUM_UPDATES = 1, 16, 3, 4, 2, 10
GOLDEN = gg.OUT


def collect(p, dist, P, seed):
    ro = ns.RolloutStorage(T, N, (C, HW, HW), space_of(dist, P), HS, 1)
    g = torch.Generator().manual_seed(seed)
    ro.obs[0].copy_(images(g, (N, C, HW, HW), 16).float())
    ro.recurrent_hidden_states[0].copy_(0.5 * torch.randn(N, HS, generator=g))
    ro.masks[0, 0] = 0.0
    for step in range(T):
        with torch.no_grad():
            value, action, logp, hxs = p.act(ro.obs[step], ro.recurrent_hidden_states[step], ro.masks[step])
        mask = torch.ones(N, 1)
        if step < 2:
            mask[N - 1] = 0.0      # masks[1] and masks[2] of the last environment
        ro.insert(images(g, (N, C, HW, HW), 16).float(), hxs, action, logp, value, torch.randn(N, 1, generator=g), mask,
                  (torch.rand(N, 1, generator=g) > 0.03).float(), torch.randn(N, 1, generator=g))
    with torch.no_grad():
        nv = p.get_value(ro.obs[-1], ro.recurrent_hidden_states[-1], ro.masks[-1]).detach()
    ro.compute_returns(nv, True, 0.99, 0.95, True)
    return ro


def attempt(dist, P, seed):
    """-> the fixture's arrays, or a string saying why this seed is not one"""
    shapes = gr.param_shapes(C, HS, dist, P)
    cshapes = cr.param_shapes(C, HS, dist, P)
    k = gr.n_gru(HS)
    p = ggr.make_policy(C, HS, dist, P, seed)
    agent = A2C_ACKTR(p, ref.VCOEF, ref.ECOEF, lr=ref.LR, eps=ref.EPS, alpha=ref.ALPHA, max_grad_norm=ref.MAX_GRAD_NORM)
    out, lrs, notes = dict(params0=gg.flat_params(p)), [], []
    p64, sq64 = out["params0"].astype(np.float64), None
    n = out["params0"].size
    c = cr.Case(C=C, Hs=HS, dist=dist, P=P, T=T, N=N, shapes=shapes, params=out["params0"])
    for j in range(ITERS):
        ns.a2c_utils.update_linear_schedule(agent.optimizer, j, NUM_UPDATES, ref.LR)   # a2c/main.py:201-205
        lrs.append(agent.optimizer.param_groups[0]["lr"])
        torch.manual_seed(seed + 10 + j)
        ro = collect(p, dist, P, seed + 20 + 2 * j)
        arrs = gg.rollout_arrays(ro)
        obs8 = arrs["obs"].astype(np.uint8)
        assert np.array_equal(arrs["obs"], obs8)
        hxs0 = ro.recurrent_hidden_states[0].numpy().copy()
        masks = ro.masks.numpy().copy()
        rows = dict(obs=arrs["obs"][:-1].reshape(T * N, C, HW, HW), hxs0=hxs0, masks=masks[:-1].reshape(-1),
                    actions=arrs["actions"].reshape(T * N, -1), returns=arrs["returns"][:-1].reshape(-1))
        km = min(cr.kink_margin(cshapes, gg.flat_params(p)[k:], rows["obs"]), cr.kink_margin(cshapes, p64[k:], rows["obs"]))
        if km < cr.KINK_FACTOR:
            return f"update {j}: kink margin {km:.2f}"
        pre = f"it{j}_"
        out[pre + "obs"], out[pre + "actions"], out[pre + "returns"] = obs8, arrs["actions"], arrs["returns"]
        out[pre + "masks"], out[pre + "hxs0"] = masks, hxs0
        vl, al, de = agent.update(ro)
        r = ref.update64(c, params=p64, sq=sq64, rows=rows, lr=lrs[-1])
        p64, sq64 = r["params"], r["square_avg"]
        idx = ref.sample_index(n, j)
        out[pre + "losses"] = np.array([vl, al, de], np.float64)
        out[pre + "params1"], out[pre + "square_avg"] = gg.flat_params(p)[idx], square_avg(agent)[idx]
        out[pre + "factor"] = np.float64(r["factor"])
        for ratio, note in (tenth(out[pre + "losses"], r["losses"], f"losses {j}"), tenth(out[pre + "params1"], p64[idx], f"params {j}"),
                            tenth(out[pre + "square_avg"], sq64[idx], f"square_avg {j}", rtol=1e-3, atol=1e-12)):
            notes.append(note)
            if ratio > 0.1:
                return "past a tenth of the tolerance: " + note
    out["lrs"] = np.array(lrs, np.float64)
    print("   ", ", ".join(notes))
    return out


def gen(tag, dist, P, seed0):
    limit = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if "cnn" in f and not f.startswith("a2c_cnn_gru"))
    for seed in range(seed0, seed0 + 60):
        out = attempt(dist, P, seed)
        print(f"a2c_cnn_gru_{tag} seed {seed}: {out if isinstance(out, str) else 'taken'}", flush=True)
        if not isinstance(out, str):
            break
    else:
        raise RuntimeError(f"a2c_cnn_gru_{tag}: no seed keeps both updates clear of the ReLU kinks")
    shapes = gr.param_shapes(C, HS, dist, P)
    name = f"a2c_cnn_gru_{tag}"
    gg.save(name, meta=gg.meta(C=C, Hs=HS, dist=dist, P=P, T=T, N=N, iters=ITERS, num_updates=NUM_UPDATES, lr=ref.LR, eps=ref.EPS,
                               alpha=ref.ALPHA, value_loss_coef=ref.VCOEF, entropy_coef=ref.ECOEF, max_grad_norm=ref.MAX_GRAD_NORM,
                               seed=seed, sample_stride=ref.SAMPLE_STRIDE, names=[k for k, _ in shapes], shapes=[list(s) for _, s in shapes]),
            **out)
    size = os.path.getsize(os.path.join(GOLDEN, name + ".npz"))
    assert size < limit, (name, size, limit)
    print(f"{name}: {size} bytes (largest earlier CNN fixture {limit})")


if __name__ == "__main__":
    gen("cat", "categorical", 5, seed0=1500)
    gen("box", "gaussian", 3, seed0=1560)
