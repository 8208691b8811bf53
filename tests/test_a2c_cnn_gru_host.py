"""CPU: A2C through time on the recurrent CNN base without a device -- tests/a2c_cnn_gru_ref.py (the arbiter of
tests/test_gpu_a2c_cnn_gru.py) held to its own conditions, and the Python layer's keyword.

  1 admission   every case: kink margin of the frames, torch's float32 gradient of the same loss within 0.5 RTOL of float64 per block,
                masks and h0 as the cases promise; the clip norms of CLIP_CASES recomputed
  2 geometry    `geometry` holds every GPU case to the edge it is named for (FACTS)
  3 defects     six injected defects, each on the references alone, each moving some block by at least 10 RTOL in a named case
  4 keyword     A2C_ACKTR(recurrent_cnn=True): what it refuses, on stand-in policies; without it the old refusal keeps its text
  5 anchors     the arbiter against the reference-written fixtures, and, where a reference checkout is present, against the .grad
                the reference's own Policy(recurrent=True) + A2C_ACKTR(acktr=False) leaves, to 1e-9"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import a2c_cnn_gru_ref as ref
import cnn_gru_ref as gr
import cnn_ref as cr
from cnn_ref import ar
from helpers import RTOL, assert_close, load

CAT, BOX = ref.CAT, ref.BOX


# ------------------------------------------------------------------------------------------------- 1 admission
@pytest.mark.parametrize("key", list(ref.SEEDS), ids=[ref.tag(k).replace(" ", "_") for k in ref.SEEDS])
def test_every_case_is_admitted_on_the_references_alone(key):
    c = ref.case(key)
    k = gr.n_gru(c.Hs)
    km, exempted = gr.cg.frame_margins(cr.param_shapes(c.C, c.Hs, c.dist, c.P), c.params[k:], gr.rows_of(c)["obs"], exempt_zeros=c.head == "fc_zero")
    assert float(km.min()) >= cr.KINK_FACTOR, (c.tag, float(km.min()))
    assert (exempted > 0) == (c.head == "fc_zero")
    g64, _, d32, zeros = ref.admitted(key)
    assert max(d32.values()) <= 0.5 * RTOL, (c.tag, d32)
    m = c.masks[:-1, :, 0]
    assert m[0, 0] == 0 and np.abs(c.hxs[0]).min() > 0
    if c.T >= 4:
        assert m[1, -1] == 0 and m[2, -1] == 0
    if c.N >= 3:
        assert not m[:, 2].any()
    if c.head == "fc_zero":
        wf, _ = gr.cg._block(cr.param_shapes(c.C, c.Hs, c.dist, c.P), "base.main.7.weight")
        have = set(zeros.tolist())
        assert all(k + wf.start + i in have for i in range(gr.ZERO_UNITS * 1568))


def test_the_cases_of_the_gpu_file_are_the_admitted_ones_and_the_clip_norms_hold():
    assert {k for k, _ in ref.GPU_CASES} == set(ref.SEEDS)
    assert ref.SEEDS[(1, 16, CAT, 5, 5, 16)] == 2 and ref.SEEDS[(1, 16, CAT, 5, 1, 3)] == 0     # (the reference's A2C default rollout)
    for key, (group, norm) in ref.CLIP_CASES.items():
        g64 = ref.admitted(key)[0]
        assert float(np.linalg.norm(g64)) == pytest.approx(norm, rel=5e-3), key
        assert ref.geometry(key[4], key[5], group)["n_groups"] > 1
        f = ref.update64(ref.case(key), max_grad_norm=float(np.float32(0.5 * norm)))["factor"]
        assert 0.49 < f < 0.51


# ------------------------------------------------------------------------------------------------- 2 geometry
# (key, group) -> what the case sits on: the groups' environments, and the facts named in the GPU file's table
FACTS = {
    ((1, 16, CAT, 5, 4, 4), None): dict(sizes=[4]),
    ((1, 16, CAT, 5, 4, 4), 1): dict(sizes=[1, 1, 1, 1], rows=[4, 4, 4, 4]),
    ((1, 16, CAT, 5, 1, 3), None): dict(sizes=[3], rows=[3]),
    ((1, 16, CAT, 5, 5, 16), None): dict(sizes=[16], rows=[80], scan=[1], live=[16]),
    ((2, 20, BOX, 3, 3, 3), None): dict(sizes=[3]),
    ((2, 20, BOX, 3, 3, 3), 2): dict(sizes=[2, 1], rows=[6, 3], stale=[0, 3]),
    (ref.FC_ZERO, None): dict(sizes=[3]),
    ((2, 20, BOX, 3, 4, 17), None): dict(sizes=[17], scan=[2], live=[1]),
    ((2, 20, BOX, 3, 4, 17), 16): dict(sizes=[16, 1], rows=[64, 4], stale=[0, 12], e0=[0, 16]),
    ((2, 20, BOX, 3, 4, 17), 5): dict(sizes=[5, 5, 5, 2], rows=[20, 20, 20, 8], stale=[0, 0, 0, 8]),
    ((1, 16, CAT, 5, 4, 34), None): dict(sizes=[34], scan=[3], live=[2]),
    ((1, 16, CAT, 5, 4, 34), 17): dict(sizes=[17, 17], e0=[0, 17], scan=[2, 2], live=[1, 1]),
    ((1, 16, CAT, 5, 8, 33), None): dict(sizes=[33], rows=[264], KS=[2], loss_blocks=[2], scan=[3]),
    ((1, 16, CAT, 5, 8, 33), 32): dict(sizes=[32, 1], rows=[256, 8], KS=[2, 1], loss_blocks=[1, 1], stale=[0, 8]),
    (ref.WIDE, None): dict(sizes=[6], rows=[18]),
    (ref.WIDE, 4): dict(sizes=[4, 2], rows=[12, 6], stale=[0, 6]),
    ((1, 18, CAT, 4, 5, 7), 3): dict(sizes=[3, 3, 1], rows=[15, 15, 5], stale=[0, 0, 10]),
}
NAMES = dict(sizes="n", rows="rows", stale="stale", e0="e0", scan="scan_workgroups", live="last_live", KS="KS", loss_blocks="loss_blocks")


def test_geometry_holds_every_gpu_case_to_its_edge():
    assert set(FACTS) == set(ref.GPU_CASES)
    for (key, group), facts in FACTS.items():
        geo = ref.geometry(key[4], key[5], group)
        for name, want in facts.items():
            assert [q[NAMES[name]] for q in geo["groups"]] == want, (key, group, name)
        assert sum(q["n"] for q in geo["groups"]) == key[5] and all(q["rows"] <= ref.GROUP_ROWS for q in geo["groups"])
    # the global-weight instances by LDS size at Hs = 512, the LDS-weight ones at the narrow widths
    assert gr.geometry(3, 6, 1, 512)["gw_scan"] and gr.geometry(3, 6, 1, 512)["gw_dx"]
    assert not gr.geometry(4, 17, 1, 20)["gw_scan"] and not gr.geometry(4, 17, 1, 20)["gw_dx"]
    # the default group: max(1, min(N, 4096 // T)) whole environments
    assert ref.group_envs(128, 64) == 32 and ref.group_envs(128, 8) == 8 and ref.group_envs(5, 16) == 16 and ref.group_envs(4096, 3) == 1
    assert ref.group_envs(3000, 5) == 1 and ref.group_envs(4, 17, 99) == 17
    with pytest.raises(AssertionError):
        ref.geometry(4097, 1)


# ------------------------------------------------------------------------------------------------- 3 injected defects
GRAD_FAULTS = [("inv_group", (2, 20, BOX, 3, 4, 17), 16), ("drop_last_group", (2, 20, BOX, 3, 4, 17), 16), ("h0_rows_0", (1, 16, CAT, 5, 4, 34), 17),
               ("adv_attached", (1, 16, CAT, 5, 4, 4), None)]


@pytest.mark.parametrize("fault,key,group", GRAD_FAULTS, ids=[f[0] for f in GRAD_FAULTS])
def test_injected_gradient_defects_are_seen(fault, key, group):
    c = ref.case(key)
    g = ref.admitted(key)[0]
    gf, _ = ref.case_grad(c, fault=fault, group=group)
    d = cr.block_distances(gf, g, c.shapes)
    assert max(d.values()) >= 10 * RTOL, (fault, d)
    if group:      # the same split without the defect is the whole gradient
        sound = np.zeros_like(g)
        for q in ref.geometry(c.T, c.N, group)["groups"]:
            sound += ref.rows_grad(c, gr.rows_of(c, np.arange(q["e0"], q["e0"] + q["n"])))[0] * (q["rows"] / (c.T * c.N))
        assert max(cr.block_distances(sound, g, c.shapes, atol=0.0).values()) <= 1e-9


@pytest.mark.parametrize("fault", ["gru_out_of_norm", "gru_last"])
def test_injected_update_defects_are_seen(fault):
    key = (2, 20, BOX, 3, 3, 3)
    c = ref.case(key)
    mgn = 0.5 * ref.CLIP_CASES[key][1]
    good, bad = ref.update64(c, max_grad_norm=mgn), ref.update64(c, max_grad_norm=mgn, fault=fault)
    what = "square_avg" if fault == "gru_last" else "params"
    base = np.zeros_like(c.params, dtype=np.float64) if fault == "gru_last" else c.params.astype(np.float64)
    d = cr.block_distances(bad[what] - base, good[what] - base, c.shapes)
    assert max(d.values()) >= 10 * RTOL, (fault, d)


# ------------------------------------------------------------------------------------------------- 4 the keyword
class _Pol(object):
    """what the checks read of a recurrent CNN policy"""
    cnn, is_recurrent, dist_kind, recurrent_hidden_state_size = 1, True, 1, 16

    class ctx(object):
        world = 1


def test_keyword_refusals():
    import simgan_amd as sg
    kw = dict(lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)

    class Mlp(_Pol):
        cnn, is_recurrent = 0, False

    class Gru(_Pol):
        cnn = 0

    class Cnn(_Pol):
        is_recurrent = False

    class SplitPolicy(_Pol):
        cnn, is_recurrent = 0, False

    for other in (Mlp(), Gru(), Cnn(), SplitPolicy()):
        for more in (kw, dict(acktr=True), dict(kw, cnn=True), dict(kw, recurrent=True)):
            with pytest.raises(ValueError, match="A2C_ACKTR\\(recurrent_cnn=True\\) takes a Policy with the recurrent CNN base"):
                sg.algo.A2C_ACKTR(other, 0.5, 0.01, recurrent_cnn=True, **more)
    p = _Pol()
    for more in (dict(acktr=True), dict(kw, acktr=True)):
        with pytest.raises(NotImplementedError, match="ACKTR"):
            sg.algo.A2C_ACKTR(p, 0.5, 0.01, recurrent_cnn=True, **more)
    with pytest.raises(NotImplementedError, match="A2C_ACKTR\\(acktr=True, recurrent_cnn=True\\): ACKTR is not implemented for the recurrent CNN base"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, recurrent_cnn=True, acktr=True)

    class Wide(_Pol):
        class ctx(object):
            world = 2
    with pytest.raises(NotImplementedError, match="A2C on the recurrent CNN base runs on one rank \\(this context's world is 2\\)"):
        sg.algo.A2C_ACKTR(Wide(), 0.5, 0.01, recurrent_cnn=True, **kw)
    with pytest.raises(ValueError, match="A2C_ACKTR\\(acktr=False\\) needs lr, eps"):
        sg.algo.A2C_ACKTR(p, 0.5, 0.01, recurrent_cnn=True, alpha=0.99, max_grad_norm=0.5)
    # without the keyword: the present refusal, in the four modes tests/test_cnn_gru_host.py tries, and with the keyword off
    for more in (dict(acktr=True), kw, dict(kw, cnn=True), dict(kw, recurrent=True), dict(kw, recurrent_cnn=False)):
        with pytest.raises(NotImplementedError, match="A2C_ACKTR: not implemented for the recurrent CNN base \\(image observations with "
                                                      "base_kwargs=\\{'recurrent': True\\}\\), in any mode -- acktr, cnn=True or recurrent=True; PPO is"):
            sg.algo.A2C_ACKTR(p, 0.5, 0.01, **more)


def test_the_keyword_reaches_the_new_entry_point_and_hands_over_slot_0():
    import simgan_amd as sg
    calls = []

    class Lib(object):
        def __getattr__(self, name):
            def f(*a):
                calls.append((name, a))
                return 0
            return f

    class Pol(_Pol):
        num_params = 10

        class ctx(object):
            world, h, lib = 1, None, Lib()
        h = None

    class Ro(object):
        h, num_processes, device_hidden, device_resident = None, 3, False, True
        recurrent_hidden_states = np.arange(4 * 3 * 16, dtype=np.float32).reshape(4, 3, 16)

        def _push(self, fields):
            calls.append(("push", tuple(fields)))
    agent = sg.algo.A2C_ACKTR(Pol(), 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5, recurrent_cnn=True)
    assert [n for n, _ in calls] == ["sg_a2c_create_cnn_rnn"] and agent.recurrent and agent.cnn and not agent.acktr
    from simgan_amd import _lib
    del calls[:]
    agent.update(Ro())
    names = [n for n, _ in calls]
    assert names == ["push", "push", "sg_ppo_set_hidden_states", "sg_ppo_update"]
    assert calls[1][1] == (_lib.F_MASKS,) and calls[2][1][2] == 3 * 16
    assert calls[3][1][2] is None and calls[3][1][3] == 0      # perms NULL
    with pytest.raises(NotImplementedError, match="A2C_ACKTR.diagnostics"):
        agent.diagnostics(Ro())
    agent.h = None


# ------------------------------------------------------------------------------------------------- 5 anchors
@pytest.mark.parametrize("name", ref.FIXTURES)
def test_the_arbiter_follows_the_reference_fixtures(name):
    g = load(name)
    m = g["meta"]
    c = ref.fixture_case(g)
    assert m["T"] == 3 and m["N"] == 4 and m["C"] == 1 and m["Hs"] == 16 and m["iters"] == 2
    params, sq = g["params0"].astype(np.float64), None
    n = params.size
    hp = {k: m[k] for k in ("eps", "alpha", "max_grad_norm")}
    for j, (pre, rows, lr) in enumerate(ref.fixture_updates(g)):
        assert (rows["masks"] == 0).any() and np.abs(rows["hxs0"]).max() > 0
        r = ref.update64(c, params=params, sq=sq, rows=rows, lr=lr, vcoef=m["value_loss_coef"], ecoef=m["entropy_coef"], **hp)
        idx = ref.sample_index(n, j)
        assert_close(g[pre + "losses"], r["losses"], rtol=0.1 * RTOL, atol=0.1 * cr.ATOL, what=f"{name} losses {j}")
        assert_close(g[pre + "square_avg"], r["square_avg"][idx], rtol=1e-4, atol=1e-13, what=f"{name} square_avg {j}")
        assert_close(g[pre + "params1"], r["params"][idx], rtol=0.1 * RTOL, atol=0.1 * cr.ATOL, what=f"{name} params {j}")
        params, sq = r["params"], r["square_avg"]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    largest = max(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path) if "cnn" in f and not f.startswith("a2c_cnn_gru"))
    assert os.path.getsize(os.path.join(path, name + ".npz")) < largest


@pytest.mark.skipif(not ar.reference_present(), reason="the reference checkout is not on this machine")
def test_the_arbiter_against_the_references_own_a2c():
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "a2c_cnn_gru_ref.py"), "--tier2"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("TIER2 ")][-1]
    res = json.loads(line[len("TIER2 "):])
    assert len(res) == len(ref.TIER2)
    # Gaussian: the arbiter takes 0.5 log(2 pi) at its float32 value, the reference's .double() policy at the double's
    # (tests/test_cnn_gru_host.py): every log-prob and the entropy shift by a constant, which moves the action loss and the
    # entropy but no gradient (the advantage is detached)
    shift = 3 * abs(float(np.float32(0.5 * np.log(2 * np.pi))) - 0.5 * np.log(2 * np.pi))
    for label, r in res.items():
        assert r["worst"] <= 1e-9, (label, r)
        assert r["loss_error"] <= 1e-9 + (2 * shift if "gaussian" in label else 0.0), (label, r)
