"""GPU: recurrent PPO past one 16-environment tile.  k_gru_scan_fwd<.., TRAIN> and k_gru_scan_bwd run (per + 15) / 16 workgroups, each
starting at base = blockIdx.x * 16, and k_gru_wgrad splits the minibatch's 16-row chunks into KS row ranges; every other recurrent
update in the suite has per <= 16 (block 0 alone; KS = 1, or 4 even ranges).  The cases of regimes.GRU_TILE_CASES reach a second
and third workgroup, a last workgroup with one live row, ragged and empty ranges, the cap KS = 16, and KS > 1 on padding rows of
dgi / dgh; tests/test_gru_tiles_host.py restates the launcher's arithmetic and holds every case to the edge it exists for, and
shows on float64 that losing the environments past the first workgroup moves GRU blocks by 3e-2 .. 1.2 (the contract: 1e-4).

  A1-A5  the one-step gradient block by block (GRU tensors gate by gate) against float64: tests/test_gpu_regimes.py's
         check_one_step_gradient with its tolerances (RTOL, F x float32 + FLOOR) unchanged, both value losses, the default launch
         and SG_POLICY_GW=1;
  A6     two optimizer steps per epoch at per = 17: step 1 reads h0 + 17 H and row block 136 (neither a multiple of 16);
  A7     no tolerance: the state trajectory is the same bits whichever workgroup, and whichever row of it, carries an environment.
SG_REGIMES_RECORD=<path> records the per-block distances of A1-A5 (profiles/gru_tiles_parity.json)."""
import numpy as np
import pytest

import gru_ref
import regimes as rg
from helpers import assert_close, assert_close_adam
from test_gpu_regimes import EPS, LR, Box, check_one_step_gradient, make_policy, make_ppo, make_rollout, npv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sg():
    import simgan_amd
    return simgan_amd


def _launch(monkeypatch, variant):
    if variant == "gw":
        monkeypatch.setenv("SG_POLICY_GW", "1")
    else:
        monkeypatch.delenv("SG_POLICY_GW", raising=False)


def tile_id(spec, T, N):
    return f"{spec[1]}x{spec[2]}x{spec[3]}-T{T}N{N}"


# ------------------------------------------------------------------------------------------- A1-A5: the gradient, tile by tile
@pytest.mark.parametrize("use_clipped", [True, False], ids=["clipped_value", "plain_value"])
@pytest.mark.parametrize("variant", ["default", "gw"])
@pytest.mark.parametrize("spec,T,N", rg.GRU_TILE_CASES, ids=[tile_id(*c) for c in rg.GRU_TILE_CASES])
def test_one_step_gradient_past_one_tile(sg, monkeypatch, spec, T, N, variant, use_clipped):
    """One minibatch of all N > 16 environments in rollout order: environment j runs in workgroup j / 16, row j % 16."""
    _launch(monkeypatch, variant)
    c = rg.case("off_policy", *spec, T=T, N=N)
    assert c.N == N > 16 and c.T == T
    check_one_step_gradient(sg, c, use_clipped, f"tiles {tile_id(spec, T, N)} {variant} {'clipped' if use_clipped else 'plain'}")


# ------------------------------------------------------------------------------------------- A6: two steps per epoch, per = 17
@pytest.mark.parametrize("variant", ["default", "gw"])
def test_two_steps_per_epoch_of_seventeen_environments(sg, monkeypatch, variant):
    """num_mini_batch = 2 on N = 34: step k takes the hidden states at h0 + k * 17 * H and the rows from k * 8 * 17 on, each in two
    workgroups (16 + 1 environments), under a permutation that moves every environment.  The whole update against gru_ref.ppo_update
    with the assertions of test_gpu_recurrent.py::test_ppo_gru_update_against_the_float64_restatement."""
    _launch(monkeypatch, variant)
    spec, T, N = rg.GRU_STEPS_CASE
    c = rg.case("off_policy", *spec, T=T, N=N)
    perms = np.random.default_rng(1).permutation(N)[None].astype(np.int64)
    assert not np.array_equal(perms[0], np.arange(N))
    assert set(perms[0, :17]) != set(range(17))   # the two minibatches are not the rollout's own halves
    ro = {k: c[k] for k in ("obs", "actions", "value_preds", "returns", "action_log_probs", "masks")}
    ref = gru_ref.ppo_update(c.params, c.O, c.A, c.H, ro, c.hxs0, perms, 1, 2, rg.CLIP, rg.VCOEF, c.entropy_coef, LR, EPS, 0.5)
    p = make_policy(sg, c)
    agent = make_ppo(sg, p, c, 1, 2, 0.5)
    losses = agent.update(make_rollout(sg, c), perms=perms)
    assert_close(losses, ref["losses"], what="ppo losses")
    mm, vv, step = agent.get_adam()
    assert step == ref["steps"] == 2
    for (name, got), (_, want) in zip(rg.blocks(c.kind, c.O, c.A, c.H, c.f, mm), rg.blocks(c.kind, c.O, c.A, c.H, c.f, ref["adam_m"])):
        assert_close(got, want, rtol=1e-3, atol=1e-7, what=f"adam m of {name}")
    assert_close(vv, ref["adam_v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close_adam(p.get_flat_params(), ref["params"], LR, ref["steps"], what="params after the update")


# ------------------------------------------------------------------------------------------- A7: the same bits in every tile
def test_states_do_not_depend_on_the_workgroup_or_the_row(sg, monkeypatch):
    """(11, 3, 32), T = 5, n = 33 (three workgroups, the last with one live row).  Rotating the environment order by 1 moves every
    environment to another row of its workgroup (and 16 -> 15, 32 -> 31, 0 -> 32 across workgroups); by 16, to another workgroup.
    The GRU's arithmetic per environment has one order wherever it runs (test_steps_and_sequence_agree_bit_for_bit_and_runs_repeat),
    so the final states of the sequence call and the states of a T-step act loop are bit-identical after undoing the rotation.
    The heads choose their row tile by the row count: values and log-probs agree to rounding."""
    monkeypatch.delenv("SG_POLICY_GW", raising=False)
    O, A, H, T, n = 11, 3, 32, 5, 33
    rng = np.random.default_rng(7)
    p = sg.Policy((O,), Box((A,)), base_kwargs={"recurrent": True, "hidden_size": H}, seed=3)
    flat = p.get_flat_params()
    p.set_flat_params((flat + 0.05 * rng.standard_normal(flat.size)).astype(np.float32))
    obs = rng.standard_normal((T, n, O)).astype(np.float32)
    hxs = (0.5 * rng.standard_normal((n, H))).astype(np.float32)
    masks = (rng.random((T, n, 1)) > 0.15).astype(np.float32)
    masks[2, 0] = masks[3, 16] = masks[1, 32] = 0.0
    action = rng.standard_normal((T, n, A)).astype(np.float32)

    def run(shift):
        env = (np.arange(n) + shift) % n          # position j holds environment env[j]
        o, m, a, h = obs[:, env], masks[:, env], action[:, env], hxs[env]
        v, lp, ent, hl = p.evaluate_actions(o.reshape(T * n, O), h, m.reshape(T * n, 1), a.reshape(T * n, A))
        steps = []
        for t in range(T):
            h = npv(p.act(o[t], h, m[t], deterministic=True)[3]).copy()
            steps.append(h)
        back = np.empty(n, np.int64)
        back[env] = np.arange(n)                  # environment e sits at position back[e]
        return (npv(v).reshape(T, n)[:, back], npv(lp).reshape(T, n)[:, back], float(npv(ent)), npv(hl)[back].copy(),
                np.stack(steps)[:, back])

    v0, lp0, ent0, hl0, st0 = run(0)
    assert np.array_equal(hl0.view(np.uint32), st0[-1].view(np.uint32)), "sequence state != step-by-step state"
    sd = gru_ref.unflatten(p.get_flat_params(), O, A, H)
    rv, rlp, rent, rh = gru_ref.evaluate(sd, obs.reshape(T * n, O), hxs, masks.reshape(T * n, 1), action.reshape(T * n, A))
    assert_close(v0, rv, what="value")
    assert_close(lp0, rlp, what="logp")
    assert_close(ent0, rent, what="entropy")
    assert_close(hl0, rh, what="rnn_hxs")
    for shift in (1, 16):
        v, lp, ent, hl, st = run(shift)
        assert np.array_equal(hl.view(np.uint32), hl0.view(np.uint32)), f"rotation by {shift}: final states differ in " \
            f"environments {sorted(set(np.nonzero(hl != hl0)[0]))}"
        assert np.array_equal(st.view(np.uint32), st0.view(np.uint32)), f"rotation by {shift}: per-step states differ in " \
            f"environments {sorted(set(np.nonzero(st != st0)[1]))}"
        assert_close(v, v0, what=f"rotation by {shift}: values")
        assert_close(lp, lp0, what=f"rotation by {shift}: log-probs")
        assert ent == ent0
