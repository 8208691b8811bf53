"""GPU: Policy on Discrete / MultiBinary action spaces -- act, evaluate_actions, PPO and A2C (csrc/sg_policy.hip k_discrete_head,
csrc/sg_ppo_kernels.hpp k_ppo_bwd_dist / k_a2c_bwd_dist).

  forward    evaluate_actions and deterministic act against the reference's fixtures (tests/golden/discrete_*.npz)
  sampling   injected uniforms against the numpy inverse CDF, exactly; the library's own draws against p within 5 sigma
  gradient   one optimizer step at max_grad_norm = 1e9 read back from Adam's m (PPO) / RMSprop's square_avg and the sign of the
             step (A2C), per parameter block against tests/discrete_ref.py (float64 autograd) within 1e-4: every shape, 16 / 77 /
             128 rows, both value losses, every launch form such a policy reaches (LDS-resident and global-weight, 16- and
             32-row groups, 4 and 8 waves); saturated logits against max(1e-4, 2 x the float32 evaluation's distance)
  updates    whole PPO / A2C updates against the fixtures, exact zeros on an all-clipped rollout, graph replay, two ranks over
             the loopback communicator, PpoLearner on a host and on a device-resident rollout
SG_DISCRETE_RECORD=<path> collects every gradient case's HIP and float32 distances (profiles/discrete_parity.json)."""
import json
import os

import numpy as np
import pytest
import torch

import discrete_ref as dr
from helpers import RTOL, assert_close, assert_close_adam

pytestmark = pytest.mark.gpu

LR, EPS, ALPHA = 3e-4, 1e-5, 0.99
DIST = {"categorical": dr.CATEGORICAL, "bernoulli": dr.BERNOULLI}
TAG = {dr.CATEGORICAL: "cat", dr.BERNOULLI: "ber"}


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def npv(x):
    return x.numpy() if hasattr(x, "numpy") else np.asarray(x)


def make_policy(sg, dist, O, K, H, params, ctx=None):
    kw = {} if ctx is None else {"ctx": ctx}
    p = sg.Policy((O,), dr.space(dist, K), base_kwargs={"recurrent": False, "hidden_size": H}, **kw)
    assert p.dist_kind == dist
    assert [(n, tuple(s)) for n, s in p.param_shapes()] == dr.param_shapes(O, K, H)
    assert list(p.state_dict())[-2:] == ["dist.linear.weight", "dist.linear.bias"]
    p.set_flat_params(params)
    return p


def fill(ro, **fields):
    for name, arr in fields.items():
        t = getattr(ro, name)
        t.copy_(t.new_tensor(np.asarray(arr).reshape(tuple(t.shape))))


def rollout_of_rows(sg, c):
    """the case's rows as a rollout of T = rows steps of one environment: one minibatch in rollout order is the case's order"""
    rows, O = c["rows"], c["O"]
    ro = sg.RolloutStorage(rows, 1, (O,), dr.space(c["dist"], c["K"]), 1, 1)
    pad = lambda a: np.concatenate([np.asarray(a, np.float32).reshape(rows, -1), np.zeros((1, np.asarray(a).reshape(rows, -1).shape[1]), np.float32)])  # noqa: E731
    fill(ro, obs=pad(c["obs"]), actions=c["actions"], action_log_probs=c["old_logp"], value_preds=pad(c["value_preds"]),
         returns=pad(c["returns"]))
    return ro


def fixture_rollout(sg, g, ctx=None, cols=None):
    m = g["meta"]
    sl = slice(None) if cols is None else cols
    N = m["N"] if cols is None else cols.stop - cols.start
    kw = {} if ctx is None else {"ctx": ctx}
    ro = sg.RolloutStorage(m["T"], N, (m["O"],), dr.space(DIST[m["dist"]], m["K"]), 1, 1, **kw)
    fill(ro, **{k: np.ascontiguousarray(g[k][:, sl]) for k in ("obs", "actions", "action_log_probs", "value_preds", "returns", "masks")})
    return ro


def _record(label, rec):
    path = os.environ.get("SG_DISCRETE_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_discrete.py under SG_DISCRETE_RECORD: per parameter block, the distance of the HIP one-step "
                       "gradient and of the float32 torch evaluation's from the float64 autograd reference (tests/discrete_ref.py)",
               "cases": {}}
    doc["cases"][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


# ------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", dr.FIXTURES)
def test_forward_matches_the_reference_fixture(sg, name):
    g = dr.load(name)
    m = g["meta"]
    dist, T, N, O, K = DIST[m["dist"]], m["T"], m["N"], m["O"], m["K"]
    p = make_policy(sg, dist, O, K, m["H"], g["params0"])
    rows = g["obs"][:-1].reshape(T * N, O)
    acts = g["actions"].reshape(T * N, -1)
    v, lp, ent, _ = p.evaluate_actions(torch.from_numpy(rows), None, None, torch.from_numpy(acts))
    assert tuple(v.shape) == (T * N, 1) and tuple(lp.shape) == (T * N, 1)
    assert_close(npv(v), g["eval_value"], what="value")
    assert_close(npv(lp), g["eval_logp"], what="logp")
    assert_close(npv(ent), g["eval_entropy"], what="entropy")
    v, a, lp, _ = p.act(torch.from_numpy(rows), None, None, deterministic=True)
    a = npv(a)
    assert a.dtype == g["det_action"].dtype == (np.int64 if dist == dr.CATEGORICAL else np.float32)
    assert a.shape == g["det_action"].shape == (T * N, 1 if dist == dr.CATEGORICAL else K)
    assert np.array_equal(a, g["det_action"])          # (the generator keeps every mode 1e-4 clear of a tie)
    assert_close(npv(lp), g["det_logp"], what="logp of the mode")
    assert_close(npv(v), g["eval_value"], what="value from act")
    assert_close(npv(p.get_value(torch.from_numpy(rows), None, None)), g["eval_value"], what="get_value")


def test_near_certain_log_prob_comes_from_the_other_classes_mass(sg):
    """logits with one class 40 above the rest: log p of that class is -(K - 1) e^-40 ~ -1.7e-17, which 1 - p cannot hold in float32;
    the others' log-probs are ~ -40.  Same for a Bernoulli bit at z = +-30."""
    O, K, H = 4, 5, 16
    shapes = dr.param_shapes(O, K, H)
    for dist in (dr.CATEGORICAL, dr.BERNOULLI):
        params = np.zeros(sum(int(np.prod(s)) for _, s in shapes), np.float32)
        bias = np.zeros(K, np.float32)
        bias[2] = 40.0 if dist == dr.CATEGORICAL else 30.0
        if dist == dr.BERNOULLI:
            bias[1] = -30.0
        params[-K:] = bias
        p = make_policy(sg, dist, O, K, H, params)
        obs = np.ones((3, O), np.float32)
        acts = np.full((3, 1), 2, np.int64) if dist == dr.CATEGORICAL else np.tile(np.array([0, 0, 1, 0, 1], np.float32), (3, 1))
        _, lp, ent, _ = p.evaluate_actions(obs, None, None, acts)
        _, want, want_ent, _ = dr.evaluate(dist, shapes, params, obs, acts)
        if dist == dr.CATEGORICAL:   # float64's logsumexp rounds 1 + 1.7e-17 to 1 as well: the closed form, through log1p
            S = (K - 1) * np.exp(-40.0)
            top, rest = -np.log1p(S), -40.0 - np.log1p(S)
            want = np.full(3, top)
            want_ent = np.full(3, -(np.exp(top) * top + (K - 1) * np.exp(rest) * rest))
        lp = npv(lp).reshape(-1).astype(np.float64)
        assert np.all(lp < 0) and np.all(np.abs(lp - want) <= 1e-4 * np.abs(want)), (lp, want)
        assert abs(float(npv(ent)) - want_ent.mean()) <= 1e-4 * want_ent.mean() + 1e-12


# ------------------------------------------------------------------------------------------------- sampling
@pytest.mark.parametrize("dist,spec", [(d, s) for d in (dr.CATEGORICAL, dr.BERNOULLI) for s in dr.SHAPES[d]])
def test_injected_uniforms_give_the_inverse_cdf_exactly(sg, dist, spec):
    O, K, H = spec
    shapes = dr.param_shapes(O, K, H)
    rng = np.random.default_rng(K)
    params = dr.init_params(shapes, 5, head_scale=2.0)
    n = 300
    obs = rng.standard_normal((n, O)).astype(np.float32)
    z = dr.evaluate(dist, shapes, params, obs, np.zeros((n, 1 if dist == dr.CATEGORICAL else K)))[3]
    u = rng.random((n, 1 if dist == dr.CATEGORICAL else K)).astype(np.float32)
    if dist == dr.CATEGORICAL:
        u[0], u[1] = 0.0, np.float32(1.0 - 2.0 ** -24)     # the ends of [0, 1): the first class; the last classes or the clamp to K - 1
    p = dr.probs32(dist, z).astype(np.float64)
    edges = np.cumsum(p, axis=1) if dist == dr.CATEGORICAL else p
    for _ in range(8):      # move every u that sits within 1e-5 of a boundary (the logits differ by float32 rounding on the device)
        near = np.abs(u.astype(np.float64)[:, :, None] - edges[:, None, :]).min(-1) < 1e-5 if dist == dr.CATEGORICAL else np.abs(u - edges) < 1e-5
        near[:2] = False
        u[near] = ((u[near] + 0.0137) % 1.0).astype(np.float32)
    assert dr.sample_margin(dist, z[2:], u[2:]) > 1e-5      # (rows 0 and 1 are the end points: not compared exactly below)
    want = dr.sample(dist, z, u)
    pol = make_policy(sg, dist, O, K, H, params)
    v, a, lp, _ = pol.act(obs, None, None, noise=u)
    a = npv(a)
    assert a.dtype == want.dtype and a.shape == want.shape
    assert np.array_equal(a[2:], want[2:]), f"{int((a[2:] != want[2:]).sum())} of {a[2:].size} actions differ from the inverse CDF"
    if dist == dr.CATEGORICAL:
        assert a[0, 0] == 0 and 0 <= a[1, 0] <= K - 1 and a.min() >= 0 and a.max() <= K - 1
    # the log-prob returned with a sampled action is evaluate_actions' of that action
    _, lp2, _, _ = pol.evaluate_actions(obs, None, None, a)
    assert np.array_equal(npv(lp), npv(lp2))


@pytest.mark.parametrize("dist,K", [(dr.CATEGORICAL, 2), (dr.CATEGORICAL, 17), (dr.CATEGORICAL, 130), (dr.BERNOULLI, 5)])
def test_library_draws_follow_the_probabilities(sg, dist, K):
    """65,536 rows of ONE observation, the library's own uniforms at a fixed seed: class / bit frequencies within 5 sigma of p."""
    O, H, n = 6, 16, 65536
    shapes = dr.param_shapes(O, K, H)
    params = dr.init_params(shapes, 9, head_scale=2.0)
    one = np.random.default_rng(1).standard_normal((1, O)).astype(np.float32)
    z = dr.evaluate(dist, shapes, params, one, np.zeros((1, 1 if dist == dr.CATEGORICAL else K)))[3]
    p = (np.exp(z - z.max()) / np.exp(z - z.max()).sum() if dist == dr.CATEGORICAL else 1.0 / (1.0 + np.exp(-z)))[0]
    pol = make_policy(sg, dist, O, K, H, params)
    pol.seed = 20240607
    a = npv(pol.act(np.repeat(one, n, 0), None, None)[1])
    freq = np.bincount(a[:, 0], minlength=K) / n if dist == dr.CATEGORICAL else a.mean(0)
    assert set(np.unique(a).tolist()) <= (set(range(K)) if dist == dr.CATEGORICAL else {0.0, 1.0})
    bad = np.abs(freq - p) > 5 * np.sqrt(p * (1 - p) / n)
    assert not bad.any(), (freq[bad], p[bad])
    a2 = npv(pol.act(np.repeat(one, n, 0), None, None)[1])      # the next call draws anew
    assert not np.array_equal(a, a2)


# ------------------------------------------------------------------------------------------------- one-step gradient
# launch forms a Discrete / MultiBinary policy reaches: (SG_PPO_ROWS, SG_PPO_WAVES, SG_POLICY_GW)
FORMS = {"default": (None, None, None), "rows16": ("16", None, None), "rows32": ("32", None, None), "rows32_waves4": ("32", "4", None),
         "gw16": ("16", None, "1"), "gw32": ("32", None, "1")}
A2C_FORMS = ("default", "rows32", "gw16", "gw32")
SPECS = [(d, s) for d in (dr.CATEGORICAL, dr.BERNOULLI) for s in dr.SHAPES[d]]
PPO_CASES = ([(d, s, rows, "default", uc) for d, s in SPECS for rows in dr.ROWS for uc in (True, False)] +
             [(d, s, 77, form, True) for d, s in SPECS for form in ("rows16", "rows32", "rows32_waves4", "gw16", "gw32")])
A2C_CASES = ([(d, s, rows, "default") for d, s in SPECS for rows in dr.ROWS] +
             [(d, s, 77, form) for d, s in SPECS for form in A2C_FORMS[1:]])


def set_form(monkeypatch, form):
    for name, val in zip(("SG_PPO_ROWS", "SG_PPO_WAVES", "SG_POLICY_GW"), FORMS[form]):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


def ppo_gradient(sg, c, use_clipped):
    p = make_policy(sg, c["dist"], c["O"], c["K"], c["H"], c["params"])
    agent = sg.algo.PPO(p, dr.CLIP, 1, 1, dr.VCOEF, dr.ECOEF, lr=LR, eps=EPS, max_grad_norm=1e9, use_clipped_value_loss=use_clipped)
    losses = agent.update(rollout_of_rows(sg, c), perms=np.arange(c["rows"], dtype=np.int64)[None])
    m, v, step = agent.get_adam()
    assert step == 1
    return m.astype(np.float64) / 0.1, losses          # m = 0.1 g after the first step


def a2c_gradient(sg, c):
    p = make_policy(sg, c["dist"], c["O"], c["K"], c["H"], c["params"])
    agent = sg.algo.A2C_ACKTR(p, dr.VCOEF, dr.ECOEF, lr=7e-4, eps=EPS, alpha=ALPHA, max_grad_norm=1e9)
    losses = agent.update(rollout_of_rows(sg, c))
    sq, step = agent.get_rmsprop()
    assert step == 1
    # square_avg = (1 - alpha) g^2 and the step is -lr g / (sqrt(square_avg) + eps): |g| from the first, its sign from the second
    step_dir = p.get_flat_params().astype(np.float64) - c["params"].astype(np.float64)
    return -np.sign(step_dir) * np.sqrt(sq.astype(np.float64) / float(np.float32(1.0 - float(np.float32(ALPHA))))), losses


def check(label, c, got, losses, want, want_losses, f32, saturated):
    hip, o32 = dr.block_distances(got, want, c["shapes"]), dr.block_distances(f32, want, c["shapes"])
    bound = {k: max(RTOL, 2.0 * o32[k]) if saturated else RTOL for k in hip}
    worst = max(hip, key=lambda k: hip[k] / bound[k])
    print(f"{label}: worst block {worst}: HIP {hip[worst]:.3e}, float32 {o32[worst]:.3e}, bound {bound[worst]:.3e}")
    _record(label, {"hip_vs_f64": hip, "float32_vs_f64": o32, "saturated": saturated})
    fails = [f"{k}: HIP {hip[k]:.3e} from float64, bound {bound[k]:.3e} (float32 evaluation {o32[k]:.3e})" for k in hip if hip[k] > bound[k]]
    assert not fails, (label, fails)
    assert_close(losses, want_losses, what=f"{label}: losses")


def case_label(kind, dist, spec, rows, form, extra=""):
    return f"{kind} {TAG[dist]} {spec[0]}x{spec[1]}x{spec[2]} rows{rows} {form}{extra}"


@pytest.mark.parametrize("dist,spec,rows,form,use_clipped", PPO_CASES,
                         ids=[f"{TAG[d]}-{s[0]}x{s[1]}x{s[2]}-{r}-{f}-{'clipped' if uc else 'plain'}" for d, s, r, f, uc in PPO_CASES])
def test_ppo_one_step_gradient(sg, monkeypatch, dist, spec, rows, form, use_clipped):
    set_form(monkeypatch, form)
    c = dr.make_case(dist, *spec, rows, seed=11)
    lo, mid, hi, margin = dr.surrogate_branches(c)
    assert min(lo, mid, hi) >= 2 and margin > 1e-4
    args = (dist, c["shapes"], c["params"], c["obs"], c["actions"], c["old_logp"], c["value_preds"], c["returns"])
    want, want_l = dr.ppo_grad(*args, use_clipped=use_clipped)
    f32, _ = dr.ppo_grad(*args, use_clipped=use_clipped, dtype=torch.float32)
    got, losses = ppo_gradient(sg, c, use_clipped)
    check(case_label("ppo", dist, spec, rows, form, " clipped" if use_clipped else " plain"), c, got, losses, want, want_l, f32, False)


@pytest.mark.parametrize("dist,spec,rows,form", A2C_CASES, ids=[f"{TAG[d]}-{s[0]}x{s[1]}x{s[2]}-{r}-{f}" for d, s, r, f in A2C_CASES])
def test_a2c_one_step_gradient(sg, monkeypatch, dist, spec, rows, form):
    set_form(monkeypatch, form)
    c = dr.make_case(dist, *spec, rows, seed=11)
    args = (dist, c["shapes"], c["params"], c["obs"], c["actions"], c["returns"])
    want, want_l = dr.a2c_grad(*args)
    f32, _ = dr.a2c_grad(*args, dtype=torch.float32)
    got, losses = a2c_gradient(sg, c)
    check(case_label("a2c", dist, spec, rows, form), c, got, losses, want, want_l, f32, False)


@pytest.mark.parametrize("algo", ["ppo", "a2c"])
@pytest.mark.parametrize("dist,spec", SPECS, ids=[f"{TAG[d]}-{s[0]}x{s[1]}x{s[2]}" for d, s in SPECS])
def test_saturated_one_step_gradient(sg, monkeypatch, dist, spec, algo):
    """Logit gaps of about 15: the gradient is ill-conditioned in ANY float32 evaluation, so the bound per block is
    max(1e-4, 2 x the distance of the same torch loss evaluated in float32 from the float64 one)."""
    set_form(monkeypatch, "default")
    c = dr.make_case(dist, *spec, 77, seed=11, saturated=True)
    if algo == "ppo":
        args = (dist, c["shapes"], c["params"], c["obs"], c["actions"], c["old_logp"], c["value_preds"], c["returns"])
        want, want_l = dr.ppo_grad(*args)
        f32, _ = dr.ppo_grad(*args, dtype=torch.float32)
        got, losses = ppo_gradient(sg, c, True)
    else:
        args = (dist, c["shapes"], c["params"], c["obs"], c["actions"], c["returns"])
        want, want_l = dr.a2c_grad(*args)
        f32, _ = dr.a2c_grad(*args, dtype=torch.float32)
        got, losses = a2c_gradient(sg, c)
    check(case_label(algo, dist, spec, 77, "default", " saturated"), c, got, losses, want, want_l, f32, True)


# ------------------------------------------------------------------------------------------------- whole updates
def ppo_agent(sg, p, m, **kw):
    return sg.algo.PPO(p, m["clip_param"], m["ppo_epoch"], m["num_mini_batch"], m["value_loss_coef"], m["entropy_coef"], lr=m["lr"],
                       eps=m["eps"], max_grad_norm=m["max_grad_norm"], **kw)


@pytest.mark.parametrize("name", dr.FIXTURES)
def test_ppo_update_matches_the_reference_fixture(sg, name):
    g = dr.load(name)
    m = g["meta"]
    p = make_policy(sg, DIST[m["dist"]], m["O"], m["K"], m["H"], g["params0"])
    agent = ppo_agent(sg, p, m)
    losses = agent.update(fixture_rollout(sg, g), perms=g["perms"])
    adam_m, adam_v, step = agent.get_adam()
    assert step == m["ppo_epoch"] * m["num_mini_batch"]
    assert_close(losses, g["ppo_losses"], what="losses")
    assert_close(adam_m, g["adam_m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert_close(adam_v, g["adam_v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close_adam(p.get_flat_params(), g["ppo_params1"], m["lr"], step, what="params after the update")


@pytest.mark.parametrize("name", dr.FIXTURES)
def test_a2c_update_matches_the_reference_fixture(sg, name):
    g = dr.load(name)
    m = g["meta"]
    p = make_policy(sg, DIST[m["dist"]], m["O"], m["K"], m["H"], g["params0"])
    agent = sg.algo.A2C_ACKTR(p, m["value_loss_coef"], m["entropy_coef"], lr=m["lr"], eps=m["eps"], alpha=m["alpha"],
                              max_grad_norm=m["max_grad_norm"])
    losses = agent.update(fixture_rollout(sg, g))
    sq, step = agent.get_rmsprop()
    assert step == 1
    assert_close(losses, g["a2c_losses"], what="losses")
    assert_close(sq, g["square_avg"], rtol=1e-3, atol=1e-12, what="square_avg")
    assert_close(p.get_flat_params(), g["a2c_params1"], what="params after the update")


def all_clipped_case(dist, O, K, H, rows, seed):
    """Every row in a branch whose gradient is exactly zero: the surrogate's min picks the clipped term (ratio 1.5 where adv > 0,
    0.5 where adv < 0), the value loss's max the clipped value outside the clip; entropy_coef = 0."""
    c = dr.make_case(dist, O, K, H, rows, seed)
    rng = np.random.default_rng(seed)
    v, logp, _, _ = dr.evaluate(dist, c["shapes"], c["params"], c["obs"], c["actions"])
    s = np.where(rng.random(rows) < 0.5, 1.0, -1.0)
    d, e = 0.5 + rng.random(rows), 0.2 + 0.8 * rng.random(rows)
    c["value_preds"] = (v - s * d).astype(np.float32)          # |v - v_old| > clip; the clipped value lies between v_old and v
    c["returns"] = (v + s * e).astype(np.float32)              # ... and further from the return than v is
    adv = dr.ar.normalised_advantages(c["returns"], c["value_preds"]).numpy()
    assert np.abs(adv).min() > 1e-3
    c["old_logp"] = (logp - np.where(adv > 0, np.log(1.5), np.log(0.5))).astype(np.float32)
    return c


@pytest.mark.parametrize("dist,spec", [(dr.CATEGORICAL, (11, 17, 64)), (dr.BERNOULLI, (20, 33, 32))], ids=["cat", "ber"])
def test_all_clipped_rows_give_exact_zeros(sg, dist, spec):
    c = all_clipped_case(dist, *spec, 77, seed=3)
    want, _ = dr.ppo_grad(dist, c["shapes"], c["params"], c["obs"], c["actions"], c["old_logp"], c["value_preds"], c["returns"], ecoef=0.0)
    assert not want.any()
    p = make_policy(sg, dist, *spec, c["params"])
    agent = sg.algo.PPO(p, dr.CLIP, 1, 1, dr.VCOEF, 0.0, lr=LR, eps=EPS, max_grad_norm=0.5)
    agent.update(rollout_of_rows(sg, c), perms=np.arange(77, dtype=np.int64)[None])
    m, v, _ = agent.get_adam()
    assert np.array_equal(m, np.zeros_like(m)), f"{int(np.count_nonzero(m))} non-zero elements of m, max {np.abs(m).max():.3e}"
    assert np.array_equal(v, np.zeros_like(v))
    assert np.array_equal(p.get_flat_params().view(np.uint32), c["params"].view(np.uint32)), "the parameters moved"


@pytest.mark.parametrize("name", ["discrete_k17", "discrete_b33"])
def test_graph_replay_is_bit_exact(sg, monkeypatch, name):
    """Two updates replayed from the captured graph against the same two launched kernel by kernel, PPO and A2C."""
    g = dr.load(name)
    m = g["meta"]
    out = []
    for graph in ("1", "0"):
        monkeypatch.setenv("SG_PPO_GRAPH", graph)
        p = make_policy(sg, DIST[m["dist"]], m["O"], m["K"], m["H"], g["params0"])
        agent, ro = ppo_agent(sg, p, m), fixture_rollout(sg, g)
        losses = [agent.update(ro, perms=g["perms"]) for _ in range(2)]
        q = make_policy(sg, DIST[m["dist"]], m["O"], m["K"], m["H"], g["params0"])
        a2c = sg.algo.A2C_ACKTR(q, 0.5, 0.01, lr=7e-4, eps=EPS, alpha=ALPHA, max_grad_norm=0.5)
        losses += [a2c.update(ro) for _ in range(2)]
        out.append((losses, p.get_flat_params(), agent.get_adam()[0], q.get_flat_params(), a2c.get_rmsprop()[0]))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["discrete_k130", "discrete_b33"])
def test_world2_equals_the_one_rank_update_on_the_joined_rollout(sg, name):
    """Two ranks over the loopback communicator, each on half the columns, with the reference's permutations over the joined
    rollout: the one-rank update on that rollout (and, through it, the reference's own)."""
    from test_gpu_world import run_ranks
    g = dr.load(name)
    m = g["meta"]
    n_loc = m["N"] // 2
    assert 2 * n_loc == m["N"]
    p = make_policy(sg, DIST[m["dist"]], m["O"], m["K"], m["H"], g["params0"])
    agent = ppo_agent(sg, p, m)
    one = agent.update(fixture_rollout(sg, g), perms=g["perms"])

    def rank_fn(rank, ctx):
        q = make_policy(sg, DIST[m["dist"]], m["O"], m["K"], m["H"], g["params0"], ctx=ctx)
        a = ppo_agent(sg, q, m)
        ro = fixture_rollout(sg, g, ctx=ctx, cols=slice(rank * n_loc, (rank + 1) * n_loc))
        return a.update(ro, perms=g["perms"]), q.get_flat_params()

    res = run_ranks(2, rank_fn)
    assert np.array_equal(res[0][1], res[1][1]) and res[0][0] == res[1][0], "replicas diverged"
    assert_close(res[0][0], one, what="losses, world 2 against one rank")
    assert_close_adam(res[0][1], p.get_flat_params(), m["lr"], 4, what="params, world 2 against one rank")
    assert_close_adam(res[0][1], g["ppo_params1"], m["lr"], 4, what="params, world 2 against the reference")


class _Env(object):
    """A deterministic vectorised environment: the next observation and the reward are functions of the step and the actions."""

    def __init__(self, n, O, dist, K):
        self.num_envs, self.O, self.dist, self.K, self.t = n, O, dist, K, 0

    def step(self, action):
        a = npv(action)
        assert a.dtype == (np.int64 if self.dist == dr.CATEGORICAL else np.float32), a.dtype
        assert a.shape == (self.num_envs, 1 if self.dist == dr.CATEGORICAL else self.K)
        assert a.min() >= 0 and a.max() <= (self.K - 1 if self.dist == dr.CATEGORICAL else 1)
        self.t += 1
        s = a.astype(np.float64).sum(1, keepdims=True)
        obs = (np.sin(0.7 * self.t + np.arange(self.O)[None] + 0.3 * s) + 0.01 * np.arange(self.num_envs)[:, None]).astype(np.float32)
        reward = (np.cos(s + self.t) * 0.5).astype(np.float32)
        done = [(self.t + i) % 5 == 0 for i in range(self.num_envs)]
        return obs, reward, done, [{} for _ in range(self.num_envs)]


@pytest.mark.parametrize("dist,K", [(dr.CATEGORICAL, 17), (dr.BERNOULLI, 5)], ids=["cat", "ber"])
def test_ppo_learner_host_and_device_resident_rollouts_agree(sg, dist, K):
    """driver.PpoLearner: two iterations of collect() + update() with a host rollout and with a device-resident one.  Both run
    the same kernels on the same numbers (the same action draws: the policies share the noise stream's seed), so the parameters
    are the same bit for bit; the environment is handed int64 class indices / float32 bits."""
    from simgan_amd.driver import PpoLearner
    T, N, O, H = 6, 8, 7, 16
    params = dr.init_params(dr.param_shapes(O, K, H), 21, head_scale=1.5)
    obs0 = np.random.default_rng(2).standard_normal((N, O)).astype(np.float32)
    out = []
    for resident in (False, True):
        p = make_policy(sg, dist, O, K, H, params)
        p.seed = 777
        agent = sg.algo.PPO(p, 0.2, 2, 2, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=0.5, seed=5)
        ro = sg.RolloutStorage(T, N, (O,), dr.space(dist, K), 1, O)
        ro.obs[0].copy_(ro.obs.new_tensor(obs0))
        ro.device_resident = resident
        learner, env = PpoLearner(p, agent, ro), _Env(N, O, dist, K)
        losses = []
        for _ in range(2):
            learner.collect(env)
            res = learner.update()
            losses.append(tuple(res[k] for k in ("value_loss", "action_loss", "dist_entropy")))
        assert str(ro.actions.dtype).endswith("int64" if dist == dr.CATEGORICAL else "float32")
        out.append((losses, p.get_flat_params(), npv(ro.actions).copy()))
    assert np.array_equal(out[0][2], out[1][2]), "the two modes collected different actions"
    assert np.array_equal(out[0][1], out[1][1]), np.abs(out[0][1] - out[1][1]).max()
    assert np.abs(out[0][1] - params).max() > 1e-4
    assert_close(out[0][0], out[1][0], what="losses")


def test_device_refusals(sg):
    """What only the library can refuse: a Gaussian-only entry point handed a Categorical policy through the C ABI."""
    import ctypes as C
    from simgan_amd import _lib
    p = make_policy(sg, dr.CATEGORICAL, 4, 3, 8, dr.init_params(dr.param_shapes(4, 3, 8), 1))
    lib, h = p.lib, _lib.H()
    cfg = _lib.ACKTRConfig(0.5, 0.01, 0.25, 0.9, 0.99, 0.001, 1e-2, 10)
    with pytest.raises(_lib.SimganHipError, match="ACKTR is implemented for Box action spaces only"):
        _lib.check(lib.sg_acktr_create(p.ctx.h, p.h, C.byref(cfg), C.byref(h)))
    with pytest.raises(_lib.SimganHipError, match="unknown kind 3"):
        _lib.check(lib.sg_policy_create2(p.ctx.h, 3, 4, 2, 8, 1, 0, C.byref(h)))
    with pytest.raises(_lib.SimganHipError, match="unknown dist 3"):
        _lib.check(lib.sg_policy_create3(p.ctx.h, 0, 4, 1, 8, 1, 0, 3, 2, C.byref(h)))
    with pytest.raises(_lib.SimganHipError, match="2\\^24"):
        _lib.check(lib.sg_policy_create3(p.ctx.h, 0, 4, 1, 8, 1, 0, 1, 1 << 24, C.byref(h)))
    with pytest.raises(_lib.SimganHipError, match="act_dim \\(2\\) must be 1"):
        _lib.check(lib.sg_policy_create3(p.ctx.h, 0, 4, 2, 8, 1, 0, 1, 5, C.byref(h)))
    with pytest.raises(_lib.SimganHipError, match="feed-forward Policy"):
        _lib.check(lib.sg_policy_create3(p.ctx.h, 2, 4, 1, 8, 1, 0, 1, 5, C.byref(h)))
    # reset_critic is not refused: a 64-unit critic beside the 8-wide actor, the head kept
    sd = p.state_dict()
    p.reset_critic((4,))
    assert p.critic_hidden == 64 and p.dist_kind == dr.CATEGORICAL
    assert np.array_equal(npv(p.state_dict()["dist.linear.weight"]), npv(sd["dist.linear.weight"]))
    v, a, lp, _ = p.act(np.zeros((3, 4), np.float32), None, None, deterministic=True)
    assert npv(a).dtype == np.int64 and np.isfinite(npv(v)).all()
