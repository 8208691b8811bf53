"""The arbiter of A2C through time on the recurrent CNN base (a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:117-230): the loss
written forward-only in torch.float64 on tests/cnn_gru_ref.py's `evaluate` (cnn_ref.trunk, the real torch.nn.GRU, the heads),
torch.autograd for the gradient, tests/a2c_cnn_ref.py's `rmsprop64` over the concatenated vector (the GRU's four tensors first, then
the CNN order: the reference's state_dict).  Nothing is derived by hand and nothing touches the library.

Cases are cnn_gru_ref.build(C, Hs, dist, P, T, N, seed=SEEDS[key], head=HEADS.get(key)): frames clear of the ReLU kinks whatever the
loss is (a property of params and obs alone).  A case counts only when torch's float32 gradient of the SAME loss lies within 0.5
RTOL of the float64 one in every parameter block (`admitted`; tests/test_a2c_cnn_gru_host.py re-checks every one).

`geometry(T, N, group)` restates the group arithmetic of a2c_cnn_gru_update (simgan_amd/csrc/sg_ppo.hip).

`fault` injects one defect, for the test of the test, each on the references alone:
  inv_group        every group's gradient scaled by 1 / (group rows) instead of 1 / (T N)
  drop_last_group  the last group adds nothing
  h0_rows_0        the h0 of group k taken from rows 0 .. n-1 instead of e0 .. e0+n-1
  adv_attached     the advantage of the action loss not detached
  gru_out_of_norm  (update64) the GRU block left out of the clip's norm
  gru_last         (update64) the GRU's square_avg returned behind the CNN's"""
import functools

import numpy as np
import torch

import a2c_cnn_ref as ac
import cnn_gru_ref as gr
import cnn_ref as cr
from cnn_ref import ar
from helpers import RTOL

HW = cr.HW
VCOEF, ECOEF, LR, EPS, ALPHA, MAX_GRAD_NORM = ac.VCOEF, ac.ECOEF, ac.LR, ac.EPS, ac.ALPHA, ac.MAX_GRAD_NORM
NO_CLIP, EPS_RECOVER = ac.NO_CLIP, ac.EPS_RECOVER
GROUP_ROWS = 4096       # SG_A2C_CNN_GRU_GROUP_ROWS

CAT, BOX = "categorical", "gaussian"
# key (C, Hs, dist, P, T, N) -> seed of cnn_gru_ref.build
SEEDS = {(1, 16, CAT, 5, 4, 4): 0, (2, 20, BOX, 3, 3, 3): 0, (1, 16, BOX, 3, 3, 3): 0, (1, 18, CAT, 4, 5, 7): 0,
         (2, 20, BOX, 3, 4, 17): 2, (1, 16, CAT, 5, 4, 34): 0, (1, 16, CAT, 5, 8, 33): 0, (4, 512, CAT, 6, 3, 6): 0,
         (1, 16, CAT, 5, 1, 3): 0, (1, 16, CAT, 5, 5, 16): 2}
HEADS = {(1, 16, BOX, 3, 3, 3): "fc_zero", (4, 512, CAT, 6, 3, 6): "peaked"}
FC_ZERO = (1, 16, BOX, 3, 3, 3)
WIDE = (4, 512, CAT, 6, 3, 6)
# the GPU file's gradient cases: (key, SG_A2C_CNN_GRU_GROUP_ENVS or None)
GPU_CASES = [((1, 16, CAT, 5, 4, 4), None), ((1, 16, CAT, 5, 4, 4), 1), ((1, 16, CAT, 5, 1, 3), None), ((1, 16, CAT, 5, 5, 16), None),
             ((2, 20, BOX, 3, 3, 3), None), ((2, 20, BOX, 3, 3, 3), 2), (FC_ZERO, None),
             ((2, 20, BOX, 3, 4, 17), None), ((2, 20, BOX, 3, 4, 17), 16), ((2, 20, BOX, 3, 4, 17), 5),
             ((1, 16, CAT, 5, 4, 34), None), ((1, 16, CAT, 5, 4, 34), 17), ((1, 16, CAT, 5, 8, 33), None), ((1, 16, CAT, 5, 8, 33), 32),
             (WIDE, None), (WIDE, 4), ((1, 18, CAT, 4, 5, 7), 3)]
# the cases whose parameter step is held with the clip acting, at max_grad_norm = half the case's float64 gradient norm:
# key -> (SG_A2C_CNN_GRU_GROUP_ENVS, that norm to three significant digits; tests/test_a2c_cnn_gru_host.py recomputes each)
CLIP_CASES = {(1, 16, CAT, 5, 4, 4): (1, 0.735), (2, 20, BOX, 3, 3, 3): (2, 3.39), (2, 20, BOX, 3, 4, 17): (16, 0.813),
              (1, 16, CAT, 5, 4, 34): (17, 0.442), (1, 16, CAT, 5, 8, 33): (32, 0.140), WIDE: (4, 54.2)}
FIXTURES = ["a2c_cnn_gru_cat", "a2c_cnn_gru_box"]
SAMPLE_STRIDE = ac.SAMPLE_STRIDE


def tag(key, group=None):
    C, Hs, dist, P, T, N = key
    return f"C={C} Hs={Hs} {dist}({P}) {T}x{N}" + (f" group {group}" if group else "")


@functools.lru_cache(maxsize=None)
def case(key):
    """cnn_gru_ref.build at the seed written above, once per process (callers must not write into it)"""
    return gr.build(*key, seed=SEEDS[key], head=HEADS.get(key, "init"))


# ------------------------------------------------------------------------------------------------------------ geometry
def group_envs(T, N, group=None):
    ne = max(1, min(N, GROUP_ROWS // T))
    return min(group, ne) if group else ne


def geometry(T, N, group=None):
    """The group arithmetic of a2c_cnn_gru_update, restated: ne, the groups [(e0, n)], and per group its rows, the padded rows,
    KS of k_gru_wgrad, the scans' workgroups with the live environments of the last one, k_cnn_head_loss_a2c_idx's blocks, and the
    padding rows that still hold a larger earlier group's values (`stale`)."""
    assert T <= GROUP_ROWS
    ne = group_envs(T, N, group)
    ks_of = lambda rp: max(1, min(16, (rp // 16) // 8))  # noqa: E731
    groups, high = [], 0
    for e0 in range(0, N, ne):
        n = min(ne, N - e0)
        rows = T * n
        rows_p = (rows + 15) & ~15
        groups.append(dict(e0=e0, n=n, rows=rows, rows_p=rows_p, KS=ks_of(rows_p), scan_workgroups=(n + 15) // 16,
                           last_live=n - 16 * ((n - 1) // 16), loss_blocks=(rows + 255) // 256, stale=max(0, min(high, rows_p) - rows)))
        high = max(high, rows)
    return dict(ne=ne, n_groups=len(groups), groups=groups, rows_p=(T * ne + 15) & ~15, KS=ks_of((T * ne + 15) & ~15))


# ------------------------------------------------------------------------------------------------------------ the loss
def a2c_loss(p, r, T, dist, vcoef=VCOEF, ecoef=ECOEF, fault=None, dtype=cr.F64):
    """a2c/algo/a2c_acktr.py:55-72 on the time-major rows r (cnn_gru_ref.rows_of) -> (total, (value_loss, action_loss, dist_entropy))"""
    values, logp, entropy, _ = gr.evaluate(p, ar.t64(r["obs"]).to(dtype), r["hxs0"], r["masks"], T, r["actions"], dist)
    adv = ar.t64(r["returns"]).to(dtype).reshape(-1) - values
    value_loss = adv.pow(2).mean()
    action_loss = -((adv if fault == "adv_attached" else adv.detach()) * logp).mean()
    return value_loss * vcoef + action_loss - entropy * ecoef, (value_loss, action_loss, entropy)


def rows_grad(c, r, vcoef=VCOEF, ecoef=ECOEF, fault=None, dtype=cr.F64):
    p = cr.leaves(c.params, c.shapes, dtype, grad=True)
    total, parts = a2c_loss(p, r, c.T, c.dist, vcoef, ecoef, fault, dtype)
    return ar.flat_grad(total, p), np.array([float(t.detach()) for t in parts])


def case_grad(c, vcoef=VCOEF, ecoef=ECOEF, fault=None, group=None, dtype=cr.F64):
    """-> (flat gradient of the ONE loss over all T N rows, losses[3]).  The grouped faults take the environments `group` at a time
    (environments do not interact, so the whole gradient is the groups' weighted by rows / (T N))."""
    if fault in ("inv_group", "drop_last_group", "h0_rows_0"):
        geo = geometry(c.T, c.N, group)
        g = np.zeros(cr.num_params(c.shapes))
        full = c.T * geo["ne"]
        for k, q in enumerate(geo["groups"]):
            if fault == "drop_last_group" and k + 1 == geo["n_groups"]:
                continue
            r = gr.rows_of(c, np.arange(q["e0"], q["e0"] + q["n"]))
            if fault == "h0_rows_0":
                r["hxs0"] = c.hxs[0][:q["n"]]
            gk, _ = rows_grad(c, r, vcoef, ecoef)
            g += gk * (q["rows"] / full if fault == "inv_group" else q["rows"] / (c.T * c.N))
        return g, rows_grad(c, gr.rows_of(c), vcoef, ecoef)[1]
    return rows_grad(c, gr.rows_of(c), vcoef, ecoef, fault, dtype)


@functools.lru_cache(maxsize=None)
def admitted(key):
    """-> (float64 gradient, losses, the float32 torch gradient's block distances from it, indices where both are exactly 0)"""
    c = case(key)
    g64, l64 = case_grad(c)
    g32, _ = case_grad(c, dtype=torch.float32)
    return g64, l64, cr.block_distances(g32, g64, c.shapes), np.nonzero((np.asarray(g64) == 0) & (np.asarray(g32) == 0))[0]


def update64(c, params=None, sq=None, rows=None, fault=None, lr=LR, eps=EPS, alpha=ALPHA, max_grad_norm=MAX_GRAD_NORM, vcoef=VCOEF,
             ecoef=ECOEF):
    """one A2C update in float64 -> dict(params, square_avg, losses, grad, factor); params / rows default to the case's"""
    cc = c if params is None else cr.Case(dict(c, params=np.asarray(params)))
    g, losses = rows_grad(cc, gr.rows_of(c) if rows is None else rows, vcoef, ecoef)
    k = gr.n_gru(c.Hs)
    sq = np.zeros_like(g) if sq is None else sq
    if fault == "gru_out_of_norm":     # the factor from the CNN block's norm alone, applied to everything
        f = cr.clip_factor(g[k:], max_grad_norm)
        p1, sq1, _ = ac.rmsprop64(cc.params, g * f, sq, lr=lr, eps=eps, alpha=alpha, max_grad_norm=NO_CLIP)
    else:
        p1, sq1, f = ac.rmsprop64(cc.params, g, sq, lr=lr, eps=eps, alpha=alpha, max_grad_norm=max_grad_norm)
    if fault == "gru_last":
        sq1 = np.concatenate([sq1[k:], sq1[:k]])
    return dict(params=p1, square_avg=sq1, losses=losses, grad=g, factor=f)


recovered_gradient = ac.recovered_gradient
sample_index = ac.sample_index


def fixture_updates(g):
    """-> [(prefix, rows dict as cnn_gru_ref.rows_of gives it, lr)] of a fixture's updates"""
    m = g["meta"]
    T, N = m["T"], m["N"]
    B = T * N
    out = []
    for j in range(m["iters"]):
        pre = f"it{j}_"
        rows = dict(obs=g[pre + "obs"].astype(np.float32)[:-1].reshape(B, m["C"], HW, HW), hxs0=g[pre + "hxs0"],
                    masks=g[pre + "masks"][:-1].reshape(-1), actions=g[pre + "actions"].reshape(B, -1), returns=g[pre + "returns"][:-1].reshape(B))
        out.append((pre, rows, float(g["lrs"][j])))
    return out


def fixture_case(g):
    """what update64 reads of a case, from a fixture's meta"""
    m = g["meta"]
    return cr.Case(C=m["C"], Hs=m["Hs"], dist=m["dist"], P=m["P"], T=m["T"], N=m["N"], shapes=gr.param_shapes(m["C"], m["Hs"], m["dist"], m["P"]),
                   params=g["params0"])


TIER2 = [(1, 16, CAT, 5, 4, 4), (2, 20, BOX, 3, 3, 3)]


def tier2():
    """Only where the reference checkout is present, in a process of its own (tools/ref_import.py): the reference's own
    Policy((C, 84, 84), space, base_kwargs={'recurrent': True}) after .double() and its A2C_ACKTR(acktr=False).update -- the .grad it
    leaves (max_grad_norm out of reach, lr 0) against `case_grad`, and its loss triple.  Nothing of the reference is copied: it is
    imported.  -> {label: dict(worst_block, worst, loss_error)}"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in (root, os.path.join(root, "tools"), os.path.join(root, "tests")):
        if path not in sys.path:
            sys.path.insert(0, path)
    cases = [case(key) for key in TIER2]
    from ref_import import Box, import_reference
    ns = import_reference()
    from third_party.a2c_ppo_acktr.algo.a2c_acktr import A2C_ACKTR

    class Discrete(object):
        def __init__(self, n):
            self.n = n
    out = {}
    for c in cases:
        sp = Discrete(c.P) if c.dist == CAT else Box(shape=(c.P,))
        policy = ns.Policy((c.C, HW, HW), sp, base_kwargs={"recurrent": True, "hidden_size": c.Hs}).double()
        policy.load_state_dict({k: v.detach().clone() for k, v in cr.leaves(c.params, c.shapes).items()})
        ro = ns.RolloutStorage(c.T, c.N, (c.C, HW, HW), sp, c.Hs, 1)
        for name in ("obs", "value_preds", "returns", "action_log_probs", "masks"):
            setattr(ro, name, ar.t64(c[name]))
        ro.actions = torch.as_tensor(c.actions) if c.dist == CAT else ar.t64(c.actions)
        ro.obs_feat, ro.recurrent_hidden_states = ro.obs_feat.double(), ar.t64(c.hxs)
        losses = A2C_ACKTR(policy, VCOEF, ECOEF, lr=0.0, eps=EPS, alpha=ALPHA, max_grad_norm=NO_CLIP, acktr=False).update(ro)
        got = np.concatenate([q.grad.reshape(-1).numpy() for q in policy.parameters()])
        g, la = case_grad(c)
        d = cr.block_distances(got, g, c.shapes, atol=0.0)
        worst = max(d, key=d.get)
        out[c.tag] = dict(worst_block=worst, worst=d[worst], loss_error=float(np.max(np.abs(la - np.asarray(losses, np.float64)))))
    return out


if __name__ == "__main__":   # the admission of every seed; `--tier2` prints tier 2 (the child process of the host test)
    import sys
    if "--tier2" in sys.argv:
        import json
        print("TIER2 " + json.dumps(tier2()))
        sys.exit(0)
    for key in SEEDS:
        g64, _, d, _ = admitted(key)
        print(tag(key), f"float32 within {max(d.values()) / RTOL:.4f} x RTOL, |g| = {np.linalg.norm(g64):.4g}", flush=True)
