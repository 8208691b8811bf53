"""GPU: the mirror-symmetry PPO step -- k_ppo_epoch_gather_sym, k_mirror_rows, k_ppo_fwd_sym, k_ppo_bwd_sym, k_ppo_reduce_sym,
k_ppo_adam_sym -- block by block against float64, on every instance the launcher can choose.  tests/test_gpu_symmetry.py holds
Adam's m on the 16-row run-time-shape instance only (its fixtures have 10 and 32 rows) and post-Adam parameters elsewhere, which
pass a wrong small block and, the Laikago mirrors being symmetric matrices, a transposed M_a (tests/test_sym_regimes_host.py shows
both on the references alone).  Here the kernels run on the cases of tests/sym_regimes.py:

  3a  the one-step gradient (Adam's m / 0.1 after one step at max_grad_norm = 1e9; sqrt(v / 0.001) = |g|) on every instance of
      k_ppo_fwd_sym / k_ppo_bwd_sym, at 128 rows and at 77 (a ragged last row group), `sym_only` (the gradient IS the symmetry
      gradient) and `mixed` (symmetry and PPO parts of equal weight), with the clipped and the unclipped value loss;
  3b  `sym_only`: m and v of every critic block and of dist.logstd._bias are exactly 0; last_symmetry_loss against float64 mean(e^2);
  3c  action widths 40 and 130 (Pp > 16, the log-prob passes of the actor column, 67 KB of M_a in LDS);
  3d  mirror_obs as a matrix (k_mirror_rows) and as a row callable (host upload), each against float64 and against each other;
  3e  saturated tanh units, on the mirrored rows too;
  3f  both sides of the gradient clip: the norm k_ppo_adam_sym clips by includes the mirrored column's slabs;
  3g  two ranks: sym_c uses the global minibatch.

Tolerances, per parameter block, distance = regimes.block_distances (rel-L2 with a floor of ATOL on the gradient's scale):
  * the project's contract: distance <= helpers.RTOL = 1e-4;
  * the arbiter form: distance <= F x (the float32 evaluation's distance on the same block) + FLOOR; the float32 evaluation is the
    oracle's float32 gradient + the symmetry restatement on float32 arrays, its distance the largest over the evaluation and three
    more with inputs moved by an ulp (sym_regimes.float32_distances).
  FLOOR = 8.6e-6: the float32 evaluation's own largest block distance over the sym_only and mixed cases (measured 8.61e-6, mixed
  20 x 130 x 32; tests/test_sym_regimes_host.py re-derives it).
  F = 2: twice the worst HIP / float32 ratio measured on the MI355X and not below 2.  The worst max(0, HIP - FLOOR) / float32 is 0.18
  (saturated 111 x 12 x 64, base.critic.0.weight: HIP 1.10e-5 against float32's 1.32e-5); on every sym_only and mixed case it is 0,
  HIP sits inside FLOOR (largest HIP distance 5.3e-6, mixed 20 x 130 x 32; sym_only 2.8e-7 .. 3.5e-7) -- profiles/sym_regimes_parity.json.
SG_SYM_REGIMES_RECORD=<path> writes every case's per-block distances (HIP and float32) to that file."""
import json
import os

import numpy as np
import pytest

import regimes as rg
import sym_regimes as sr
from helpers import ATOL, RTOL, assert_close

pytestmark = pytest.mark.gpu

F, FLOOR = 2.0, 8.6e-6
LR, EPS = rg.LR, rg.EPS
KNOBS = ("SG_PPO_ROWS", "SG_PPO_WAVES", "SG_POLICY_GW")


class Box:  # duck-typed gym.spaces.Box
    def __init__(self, shape):
        self.shape = tuple(shape)


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


# ------------------------------------------------------------------------------------------- which instance a launch takes
# sg_ppo_update (simgan_amd/csrc/sg_ppo.hip) restated for Policy with the symmetry loss on; see test_every_instance.
LDS_BYTES, NUM_CU = 160 * 1024, 256      # an MI355X compute unit's LDS (hipDeviceProp_t::sharedMemPerBlock), its CUs


def _pad16(x):
    return (x + 15) & ~15


def _layout(O, A, H):
    """sg_layout.cpp make_trunk: (ldO, ldH, ldP, largest trunk in floats, largest trunk from w2 on, both trunks)"""
    Hp, ldO, ldH, Pp = _pad16(H), _pad16(O) + 4, _pad16(H) + 4, _pad16(A)
    w2 = Hp * ldO + Hp
    actor = w2 + Hp * ldH + Hp + Pp * ldH + Pp + _pad16(A)       # ... | wh | bh | logstd
    critic = w2 + Hp * ldH + Hp + 16 * ldH + 16
    return ldO, ldH, Pp + 4, max(actor, critic), max(actor, critic) - w2, actor + critic


def fwd_lds_bytes(O, A, H, mt, gw):
    ldO, ldH, _, trunk = _layout(O, A, H)[:4]
    R = 16 * mt
    return 4 * ((0 if gw else trunk) + R * ldO + 2 * R * ldH)


def _bwd_tiles(O, A, H, mt, w_floats, n_out, ma):
    ldO, ldH, ldP = _layout(O, A, H)[:3]
    R = 16 * mt
    return 4 * (w_floats + R * ldO + 2 * R * ldH + n_out * R * ldP + ((R * A + 3) & ~3) + 7 * R + (((A * A + 3) & ~3) if ma else 0))


def bwd_lds_bytes(O, A, H, mt, gw):       # the plain step's fused backward (Policy, <= 32-row groups): the whole trunk
    return _bwd_tiles(O, A, H, mt, 0 if gw else _layout(O, A, H)[3], 2, False)


def bwd_sym_lds_bytes(O, A, H, mt, gw):   # k_ppo_bwd_sym: the trunk from w2 on, three head tiles, M_a
    return _bwd_tiles(O, A, H, mt, 0 if gw else _layout(O, A, H)[4], 3, True)


def instance_of(O, A, H, mb, env):
    """-> (instance of k_ppo_fwd_sym / k_ppo_bwd_sym, threads per workgroup) of a symmetric step on one minibatch of `mb` rows"""
    ldO, ldH, ldP, trunk, _, total = _layout(O, A, H)

    def fits(mt, gw):
        return max(fwd_lds_bytes(O, A, H, mt, gw), bwd_lds_bytes(O, A, H, mt, gw), bwd_sym_lds_bytes(O, A, H, mt, gw)) <= LDS_BYTES

    needs_gw = env.get("SG_POLICY_GW") == "1" or 4 * (trunk + 16 * ldO + 32 * ldH + 16 * ldP) > LDS_BYTES - 1024
    gw = needs_gw or not fits(1, False)
    mt = 2 if (((mb + 15) // 16) * (total + 8) * 4 > (24 << 20) or ((mb + 31) // 32) * 3 >= NUM_CU) else 1
    if env.get("SG_PPO_ROWS") in ("16", "32", "64"):
        mt = int(env["SG_PPO_ROWS"]) // 16
    mt = min(mt, 2)                       # the symmetric and the global-weight families stop at 32-row groups
    while mt > 1 and not fits(mt, gw):
        mt //= 2
    threads = 512 if mt >= 2 and env.get("SG_PPO_WAVES") != "4" else 256
    if gw:
        return f"gw<{mt}>", threads
    shape = (_pad16(O) // 16, _pad16(H) // 16)
    return (f"<{mt}, {shape[0]}, {shape[1]}>" if (mt,) + shape == (2, 7, 4) else f"<{mt}, 0, 0>"), threads


LAUNCHES = [({}, (111, 12, 64), ("<1, 0, 0>", 256)),
            ({"SG_PPO_ROWS": "32"}, (111, 12, 64), ("<2, 7, 4>", 512)),
            ({"SG_PPO_ROWS": "32", "SG_PPO_WAVES": "4"}, (111, 12, 64), ("<2, 7, 4>", 256)),
            ({"SG_POLICY_GW": "1"}, (111, 12, 64), ("gw<1>", 256)),
            ({"SG_POLICY_GW": "1", "SG_PPO_ROWS": "32"}, (111, 12, 64), ("gw<2>", 512)),
            ({}, (47, 12, 64), ("<1, 0, 0>", 256)),
            ({"SG_PPO_ROWS": "32"}, (47, 12, 64), ("<2, 0, 0>", 512))]
# the settings of test_gpu_regimes.LOGP_CASES for these widths (the symmetric family caps SG_PPO_ROWS=64 at 32 rows itself)
WIDE_LAUNCHES = [({"SG_PPO_ROWS": "64"}, (20, 40, 32), ("<2, 0, 0>", 512)),
                 ({"SG_PPO_ROWS": "64", "SG_PPO_WAVES": "4"}, (20, 40, 32), ("<2, 0, 0>", 256)),
                 ({"SG_PPO_ROWS": "16"}, (20, 130, 32), ("<1, 0, 0>", 256)),
                 ({"SG_PPO_ROWS": "32"}, (20, 130, 32), ("<1, 0, 0>", 256))]     # 32-row groups do not fit LDS: falls back to 16


def env_id(env):
    return "-".join(f"{k[3:].lower()}{v}" for k, v in env.items()) or "default"


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------- the step
def _record(label, rec):
    path = os.environ.get("SG_SYM_REGIMES_RECORD")
    if not path:
        return
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        doc = {"what": "tests/test_gpu_sym_regimes.py under SG_SYM_REGIMES_RECORD: per parameter block, the distance of the HIP one-step "
                       "gradient of the mirror-symmetry PPO step and of the float32 evaluation's from the float64 reference; "
                       "ratio = max(0, hip - FLOOR) / float32", "FLOOR": FLOOR, "cases": {}}
    doc["cases"][label] = rec
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def row_fn(mat):
    mat = np.asarray(mat, np.float64)
    return lambda x: list(mat @ np.asarray(x, np.float64))


def one_step(sg, c, use_clipped=True, max_grad_norm=1e9, mirror_obs="matrix", ctx=None, perms=None):
    """ppo_epoch = 1, one minibatch of all rows in rollout order -> (agent, losses, m, v) after the step"""
    kw = {} if ctx is None else {"ctx": ctx}
    p = sg.Policy((c.O,), Box((c.A,)), base_kwargs={"recurrent": False, "hidden_size": c.H}, **kw)
    assert [(n, tuple(s)) for n, s in p.param_shapes()] == [(n, tuple(s)) for n, s in rg.param_shapes("mlp", c.O, c.A, c.H)]
    p.set_flat_params(c.params)
    ro = sg.RolloutStorage(c.T, c.N, (c.O,), Box((c.A,)), 1, 1, **kw)
    for name in ("obs", "actions", "value_preds", "returns", "action_log_probs", "masks"):
        getattr(ro, name).copy_(getattr(ro, name).new_tensor(c[name]))
    agent = sg.algo.PPO(p, rg.CLIP, 1, 1, rg.VCOEF, c.entropy_coef, symmetry_coef=c.symmetry_coef, lr=LR, eps=EPS, max_grad_norm=max_grad_norm,
                        use_clipped_value_loss=use_clipped, mirror_obs=c.m_obs if mirror_obs == "matrix" else row_fn(c.m_obs),
                        mirror_act=c.m_act)
    losses = agent.update(ro, perms=np.arange(c.T * c.N, dtype=np.int64)[None] if perms is None else perms)
    m, v, step = agent.get_adam()
    assert step == 1
    return agent, losses, m, v


def bound(o32):
    """the largest distance from float64 a block may have whose float32 evaluation sits o32 away"""
    return min(RTOL, F * o32 + FLOOR)


def failing_blocks(hip, o32):
    return [f"{k}: {hip[k]:.3e} from float64 (contract {RTOL:g}; float32 evaluation {o32[k]:.3e}, limit {F * o32[k] + FLOOR:.3e})"
            for k in hip if not (hip[k] <= RTOL and hip[k] <= F * o32[k] + FLOOR)]


def hold_gradient(c, m, v, use_clipped, label, scale=1.0):
    """m / 0.1 (and sqrt(v / 0.001)) against `scale` x the float64 gradient, block by block"""
    o32 = c["o32_clipped" if use_clipped else "o32_plain"]
    hip = sr.distances(c, m.astype(np.float64) / 0.1, use_clipped, scale)
    ratio = {k: (max(0.0, hip[k] - FLOOR) / o32[k] if o32[k] > 0 else (0.0 if hip[k] <= FLOOR else float("inf"))) for k in hip}
    worst = max(ratio, key=ratio.get)
    print(f"{label}: worst block {worst}: HIP {hip[worst]:.3e}, float32 {o32[worst]:.3e}, ratio {ratio[worst]:.2f}; "
          f"largest HIP distance {max(hip.values()):.3e}")
    _record(label, {"case": c.tag, "use_clipped_value_loss": use_clipped, "hip_vs_f64": hip, "float32_vs_f64": o32,
                    "worst_ratio": ratio[worst], "worst_hip": max(hip.values())})
    fails = failing_blocks(hip, o32)
    assert not fails, (label, fails)
    g64 = scale * c["grad_clipped" if use_clipped else "grad_plain"]
    vd = rg.block_distances(np.sqrt(v.astype(np.float64) / 0.001), np.abs(g64), "mlp", c.O, c.A, c.H, 1, ATOL)
    assert max(vd.values()) <= RTOL, (label, "sqrt(v / 0.001) against |float64 gradient|", {k: x for k, x in vd.items() if x > RTOL})


def hold_symmetry_loss(agent, c, label):
    got = agent.last_symmetry_loss
    assert abs(got - c.sym_loss) <= 1e-4 * c.sym_loss, f"{label}: last_symmetry_loss {got:.8g}, float64 mean(e^2) {c.sym_loss:.8g}"


def hold_exact_zeros(c, m, v, label):
    """3b: the PPO gradient is exactly zero and the symmetry term reaches the actor's trunk and mean head alone"""
    for (k, bm), (_, bv) in zip(rg.blocks("mlp", c.O, c.A, c.H, 1, m), rg.blocks("mlp", c.O, c.A, c.H, 1, v)):
        if k not in sr.ACTOR_BLOCKS:
            assert not bm.any() and not bv.any(), f"{label}: {k}: {int(np.count_nonzero(bm))} non-zero elements of m, max {np.abs(bm).max():.3e}"
        else:
            assert bm.any(), f"{label}: {k}: m is all zero"


def check_one_step_gradient(sg, c, use_clipped, label, mirror_obs="matrix"):
    assert c.norm < 0.9 * 1e9 and c.norm_plain < 0.9 * 1e9      # the clip is inactive
    agent, losses, m, v = one_step(sg, c, use_clipped, mirror_obs=mirror_obs)
    hold_gradient(c, m, v, use_clipped, label)
    if c.regime == "sym_only":
        hold_exact_zeros(c, m, v, label)
    hold_symmetry_loss(agent, c, label)
    assert_close(losses, c["losses_clipped" if use_clipped else "losses_plain"], what=f"{label}: losses")
    return m


# (regime, clipped value loss): sym_only has no value loss (every row's is clipped away)
VARIANTS = [("sym_only", True), ("mixed", True), ("mixed", False)]
VARIANT_IDS = ["sym_only", "mixed-clipped_value", "mixed-plain_value"]


def shape_id(s):
    return "x".join(str(x) for x in s)


# ------------------------------------------------------------------------------------------- 3a, 3b: every instance
EVERY = [(env, shape, mirror, rows, want) for env, shape, want in LAUNCHES for mirror, rows in
         ((("laikago", 128), ("laikago", 77), ("dense", 128), ("dense", 77)) if shape[0] == 111 else (("dense", 128), ("dense", 77)))]


@pytest.mark.parametrize("regime,use_clipped", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("env,shape,mirror,rows,want", EVERY, ids=[f"{shape_id(s)}-{env_id(e)}-{mi}-{r}" for e, s, mi, r, _ in EVERY])
def test_every_instance(sg, monkeypatch, env, shape, mirror, rows, want, regime, use_clipped):
    """Which instance of k_ppo_fwd_sym / k_ppo_bwd_sym a launch takes (simgan_amd/csrc/sg_ppo.hip; restated in instance_of above):
    the step runs on a grid of (row groups, 3) -- actor, critic, actor on the mirrored rows.  ppo_row_tiles starts from 16-row
    groups (MT = 1): 32-row ones only when ((mb + 31) / 32) x 3 columns >= 256 CUs or the 16-row slabs pass 24 MB, neither at 128
    or 77 rows.  SG_PPO_ROWS = 32 asks for MT = 2; 64 is capped to 2, the symmetric and the global-weight families having no 64-row
    instance; MT is then halved until `fits`: the forward tiles, the plain step's backward tiles and bwd_sym_lds -- the trunk from
    w2 on, X, H1, H2, THREE head tiles [R][ldP], the actions, 7 R scalars and the [A][A] M_a -- each within the CU's 160 KB.  At
    (111, 12, 64) bwd_sym_lds(2) is 65,088 bytes, at (47, 12, 64) 56,896: both fit.  Global-weight instances run when
    SG_POLICY_GW=1 or the trunk does not fit (not at these shapes).  ppo_launch then takes, in order, the instance specialised
    for (MT, Op / 16, Hp / 16) -- the symmetric family has one, <2, 7, 4>: obs 111 -> Op = 112, hidden 64 -- else the
    run-time-shape <MT, 0, 0>; ppo_block_threads gives 512 threads when MT >= 2 unless SG_PPO_WAVES=4, else 256:
        (111, 12, 64)  default <1, 0, 0>   ROWS=32 <2, 7, 4> 512 threads   ROWS=32 WAVES=4 <2, 7, 4> 256 threads
                       GW=1 the 16-row global-weight instance   GW=1 ROWS=32 the 32-row one
        (47, 12, 64)   default <1, 0, 0>   ROWS=32 <2, 0, 0>
    77 rows = four 16-row groups + 13 rows, or two 32-row groups + 13: the last group is ragged in either.  The one-step
    gradient block by block, the exact zeros of sym_only (3b) and last_symmetry_loss on each."""
    assert instance_of(*shape, rows, env) == want
    set_env(monkeypatch, env)
    c = sr.case(regime, *shape, mirror, rows)
    check_one_step_gradient(sg, c, use_clipped, f"3a {shape_id(shape)} {env_id(env)} {mirror} {rows} {regime} {'clipped' if use_clipped else 'plain'}")


@pytest.mark.parametrize("regime,use_clipped", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("rows_env", [None, "32"], ids=["default", "rows32"])
def test_one_tile_of_everything(sg, monkeypatch, rows_env, regime, use_clipped):
    """(5, 2, 8): Op = Hp = Pp = 16, A A = 4 floats of M_a, 77 rows"""
    env = {"SG_PPO_ROWS": rows_env} if rows_env else {}
    assert instance_of(5, 2, 8, 77, env) == (f"<{2 if rows_env else 1}, 0, 0>", 512 if rows_env else 256)
    set_env(monkeypatch, env)
    c = sr.case(regime, 5, 2, 8, "dense", 77)
    check_one_step_gradient(sg, c, use_clipped, f"3a 5x2x8 {env_id(env)} {regime} {'clipped' if use_clipped else 'plain'}")


# ------------------------------------------------------------------------------------------- 3c: wide action heads
@pytest.mark.parametrize("regime,use_clipped", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("env,shape,want", WIDE_LAUNCHES, ids=[f"{shape_id(s)}-{env_id(e)}" for e, s, _ in WIDE_LAUNCHES])
def test_wide_action_heads(sg, monkeypatch, env, shape, want, regime, use_clipped):
    """A = 40 (Pp = 48, ldP = 52) and A = 130 (Pp = 144, ldP = 148): head tiles of several MFMA column tiles, the e = M_a mu(s) -
    mu(s_m) loop over A > 16 columns, and the log-prob phase of the actor column, which k_ppo_bwd_sym shares with k_ppo_bwd
    (test_gpu_regimes.test_every_log_prob_pass): a row gets L = threads / R lanes, the fast pass runs when A <= 8 L.
      (20, 40, 32)   SG_PPO_ROWS=64 is capped at 32 rows: bwd_sym_lds(2) = 58,240 bytes fits -> <2, 0, 0>; 512 threads: L = 16,
                     fast pass, 3 dimensions per lane; with SG_PPO_WAVES=4, 256 threads: L = 8, fast pass, 5 per lane.
      (20, 130, 32)  M_a alone is 67,600 bytes.  bwd_sym_lds(2) = 4 x (6,656 trunk floats from w2 on + 1,152 X + 2,304 H1, H2 +
                     14,208 for three head tiles + 4,160 actions + 224 + 16,900 M_a) = 182,416 bytes > 163,840: fits(2) fails
                     and the launcher FALLS BACK to 16-row groups whatever SG_PPO_ROWS asks (bwd_sym_lds(1) = 138,320 bytes
                     fits): <1, 0, 0>, 256 threads, L = 16, and 130 > 128 takes the general log-prob pass.  Both settings are
                     run; both are that one instance."""
    c = sr.case(regime, *shape, "dense", {40: 77, 130: 128}[shape[1]])
    assert instance_of(*shape, c.rows, env) == want
    set_env(monkeypatch, env)
    check_one_step_gradient(sg, c, use_clipped, f"3c {shape_id(shape)} {env_id(env)} {regime} {'clipped' if use_clipped else 'plain'}")


# ------------------------------------------------------------------------------------------- 3d: both mirror paths
@pytest.mark.parametrize("regime", ["sym_only", "mixed"])
def test_both_mirror_paths(sg, monkeypatch, regime):
    """mirror_obs as a matrix (k_mirror_rows: the row product in double on the device) and as a row callable (mirrored on the host
    in float64, uploaded through sg_ppo_set_mirrored_obs): each against float64, and against each other at 1e-6 -- the two
    double-precision row products add in different orders and may round a mirrored float32 one ulp apart."""
    set_env(monkeypatch, {})
    c = sr.case(regime, 111, 12, 64, "dense", 77)
    m_mat = check_one_step_gradient(sg, c, True, f"3d {regime} matrix", mirror_obs="matrix")
    m_fn = check_one_step_gradient(sg, c, True, f"3d {regime} callable", mirror_obs="callable")
    apart = rg.block_distances(m_fn, m_mat, "mlp", c.O, c.A, c.H, 1, ATOL)
    assert max(apart.values()) <= 1e-6, {k: x for k, x in apart.items() if x > 1e-6}


# ------------------------------------------------------------------------------------------- 3e: saturated
@pytest.mark.parametrize("use_clipped", [True, False], ids=["clipped_value", "plain_value"])
@pytest.mark.parametrize("rows_env", [None, "32"], ids=["default", "rows32"])
@pytest.mark.parametrize("shape", [s[:3] for s in sr.SATURATED_SHAPES], ids=[shape_id(s[:3]) for s in sr.SATURATED_SHAPES])
def test_saturated(sg, monkeypatch, shape, rows_env, use_clipped):
    """weights x 4, observations x 3: 1 - h^2 where the units saturate, on the rows and on the mirrored rows (a dense M_obs keeps
    their scale), in the 16-row instance and in the 32-row one (<2, 7, 4> at obs 111, <2, 0, 0> at obs 47)"""
    set_env(monkeypatch, {"SG_PPO_ROWS": rows_env} if rows_env else {})
    c = sr.case("saturated", *shape, "dense", 128)
    assert c.desc["saturation"] > 0.2
    check_one_step_gradient(sg, c, use_clipped, f"3e {shape_id(shape)} rows{rows_env or 'default'} {'clipped' if use_clipped else 'plain'}")


# ------------------------------------------------------------------------------------------- 3f: both sides of the gradient clip
def test_both_sides_of_the_gradient_clip(sg, monkeypatch):
    """max_grad_norm = 0.5 (coef = 0.5 / (norm + 1e-6) < 1) and a value above the float64 norm (coef clamps to 1) on one mixed case
    whose norm lies between them with 10 % to spare.  Half of the actor blocks' gradient comes from the mirrored column's slabs: a
    norm taken without them would be off by tens of per cent, and m -- held per block against 0.1 g min(1, c / (||g|| + 1e-6)) --
    with it.  m(hi) / m(0.5), block by block, is the ratio of the two clip coefficients."""
    set_env(monkeypatch, {})
    c, hi = sr.clip_case()
    assert 1.1 * sr.CLIP_LO <= c.norm <= 0.9 * hi
    ms = {}
    for mg in (sr.CLIP_LO, hi):
        agent, losses, m, v = one_step(sg, c, True, max_grad_norm=mg)
        hold_gradient(c, m, v, True, f"3f max_grad_norm {mg:g}", scale=min(1.0, mg / (c.norm + 1e-6)))
        hold_symmetry_loss(agent, c, f"3f max_grad_norm {mg:g}")
        assert_close(losses, c.losses_clipped, what=f"max_grad_norm {mg:g}: losses")
        ms[mg] = m.astype(np.float64)
    want = (c.norm + 1e-6) / sr.CLIP_LO
    for (k, a), (_, b) in zip(rg.blocks("mlp", c.O, c.A, c.H, 1, ms[hi]), rg.blocks("mlp", c.O, c.A, c.H, 1, ms[sr.CLIP_LO])):
        r = float((a * b).sum() / (b * b).sum())
        assert abs(r - want) <= RTOL * want, f"{k}: m({hi:g}) / m(0.5) = {r:.7g}, the clip coefficients' ratio is {want:.7g}"


# ------------------------------------------------------------------------------------------- 3g: two ranks
def test_world_of_2(sg, monkeypatch):
    """Two ranks over the loopback communicator, 8 of the 16 columns each, the injected permutation the global rollout order: after
    the all-reduce m / 0.1 on EVERY rank is the float64 gradient of the concatenated rollout -- sym_c = 2 coef / (B A) must use the
    global minibatch B = 128, not the rank's 64 rows (that would double every block) -- and the symmetry loss is the global mean."""
    from test_gpu_world import run_ranks
    set_env(monkeypatch, {})
    c = sr.case("sym_only", 111, 12, 64, "dense", 128)
    world, n_loc = 2, c.N // 2
    perms = np.arange(c.T * c.N, dtype=np.int64)[None]

    def body(rank, ctx):
        cs = rg.Case(c)
        cs["N"] = n_loc
        for k in ("obs", "actions", "action_log_probs", "value_preds", "returns", "masks"):
            cs[k] = np.ascontiguousarray(c[k][:, rank * n_loc:(rank + 1) * n_loc])
        agent, losses, m, v = one_step(sg, cs, True, ctx=ctx, perms=perms)
        return agent.last_symmetry_loss, losses, m, v

    for rank, (sym, losses, m, v) in enumerate(run_ranks(world, body)):
        hold_gradient(c, m, v, True, f"3g rank {rank}")
        hold_exact_zeros(c, m, v, f"3g rank {rank}")
        assert abs(sym - c.sym_loss) <= 1e-4 * c.sym_loss, (rank, sym, c.sym_loss)
        assert_close(losses, c.losses_clipped, what=f"rank {rank}: losses")
