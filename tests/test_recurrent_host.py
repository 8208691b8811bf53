"""CPU: the host side of the recurrent Policy -- the numpy restatement (tests/gru_ref.py) against the reference-written
fixtures, the parameter order, RolloutStorage.recurrent_generator, the reference checkpoint of a recurrent policy and the
refusals that need no device.  No compute entry point of the library is called here."""
import os
import types

import numpy as np
import pytest

import gru_ref
from helpers import GOLDEN, assert_close, load

CASES = ["policy_gru_tiny", "policy_gru_hopper", "policy_gru_laikago"]


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    g = load(name)
    m = g["meta"]
    sd = gru_ref.unflatten(g["params"], m["O"], m["A"], m["H"])
    v, a, lp, h = gru_ref.act(sd, g["obs"], g["hxs"], g["masks"], g["noise"])
    assert_close(v, g["act_value"], what="act value")
    assert_close(a, g["act_action"], what="act action")
    assert_close(lp, g["act_logp"], what="act logp")
    assert_close(h, g["act_hxs"], what="act hxs")
    v, a, lp, _ = gru_ref.act(sd, g["obs"], g["hxs"], g["masks"])
    assert_close(a, g["det_action"], what="det action")
    assert_close(lp, g["det_logp"], what="det logp")
    assert_close(v, g["get_value"], what="get_value")
    assert m["zero_masks"] > 0 and (g["seq_masks"] == 0).sum() == m["zero_masks"]
    v, lp, ent, h = gru_ref.evaluate(sd, g["seq_obs"], g["seq_hxs"], g["seq_masks"], g["seq_action"])
    assert_close(v, g["seq_value"], what="sequence value")
    assert_close(lp, g["seq_logp"], what="sequence logp")
    assert_close(ent, g["seq_entropy"], what="sequence entropy")
    assert_close(h, g["seq_hxs_out"], what="sequence hxs")
    # step by step == one sequence (what the generator asserted of the reference): the states the rollout stored
    x, _ = gru_ref.gru_sequence(sd, g["seq_obs"], g["seq_hxs"], g["seq_masks"])
    assert_close(x.reshape(m["T"], m["n"], m["H"]), g["step_hxs"][1:], what="states along the rollout")


@pytest.mark.parametrize("name", CASES + ["ckpt_policy_gru"])
def test_param_shapes_follow_the_reference_state_dict(name):
    from simgan_amd.model import Policy
    m = load(name)["meta"]
    stub = types.SimpleNamespace(obs_dim=m["O"], act_dim=m["A"], hidden_size=m["H"], critic_hidden=m["H"], _rec=lambda: True)
    shapes = Policy.param_shapes(stub)
    assert [n for n, _ in shapes] == m["names"]
    assert [list(s) for _, s in shapes] == m["shapes"]
    assert shapes == gru_ref.param_shapes(m["O"], m["A"], m["H"])
    stub._rec = lambda: False   # the feed-forward order is today's
    ff = Policy.param_shapes(stub)
    assert [n for n, _ in ff] == m["names"][4:] and ff[0][1] == (m["H"], m["O"])


def _rollout_stub(g, pre):
    return types.SimpleNamespace(**{k: g[pre + k] for k in ("obs", "obs_feat", "actions", "rewards", "value_preds", "returns",
                                                             "action_log_probs", "masks", "recurrent_hidden_states")})


def test_recurrent_generator_matches_the_reference():
    from simgan_amd.storage import recurrent_batches
    g = load("recgen_gru")
    for ci, case in enumerate(g["meta"]["cases"]):
        pre = f"c{ci}_"
        ro = _rollout_stub(g, pre)
        batches = list(recurrent_batches(ro, g[pre + "advantages"], case["M"], perm=g[pre + "perm"]))
        assert len(batches) == case["n_batches"] == case["N"] // (case["N"] // case["M"])
        for bi, b in enumerate(batches):
            assert len(b) == 8
            for fi, t in enumerate(b):
                ref = g[f"{pre}b{bi}_{fi}"]
                got = t.numpy() if hasattr(t, "numpy") else np.asarray(t)
                assert got.shape == ref.shape, (ci, bi, fi, got.shape, ref.shape)
                assert np.array_equal(got, ref), (ci, bi, fi)
    assert [c["n_batches"] for c in g["meta"]["cases"]] == [4, 8, 2]   # N = 8: M = 3 -> 4 minibatches, M = 5 -> 8


def test_recurrent_generator_refusals():
    from simgan_amd.storage import recurrent_batches
    g = load("recgen_gru")
    ro = _rollout_stub(g, "c0_")   # N = 8
    with pytest.raises(AssertionError, match="PPO requires the number of processes"):
        list(recurrent_batches(ro, None, 9))
    ro7 = types.SimpleNamespace(**{k: v[:, :7] for k, v in vars(ro).items()})
    with pytest.raises(ValueError, match="do not split"):
        list(recurrent_batches(ro7, None, 2))   # per = 3, 7 % 3 != 0: the reference's IndexError
    with pytest.raises(AssertionError, match="permutation"):
        list(recurrent_batches(ro, None, 2, perm=np.zeros(8, np.int64)))
    assert len(list(recurrent_batches(ro, None, 4))) == 4   # library-drawn permutation, no advantages


def test_reference_checkpoint_of_a_recurrent_policy_is_read():
    from simgan_amd.checkpoint import read_reference_checkpoint
    g = load("ckpt_policy_gru")
    m = g["meta"]
    ck = read_reference_checkpoint(os.path.join(GOLDEN, "ckpt_policy_gru.pt"))
    assert ck["recurrent"] is True and ck["class_name"] == "Policy"
    assert (ck["obs_dim"], ck["act_dim"], ck["hidden"], ck["critic_hidden"]) == (m["O"], m["A"], m["H"], m["H"])
    assert list(ck["state_dict"]) == m["names"]
    flat = np.concatenate([v.reshape(-1) for v in ck["state_dict"].values()])
    assert np.array_equal(flat, g["flat"])
    assert_close(ck["ob_rms"]["mean"], g["rms_mean"], what="ob_rms mean")
    # the feed-forward checkpoint still reads as feed-forward
    assert not read_reference_checkpoint(os.path.join(GOLDEN, "ckpt_policy_mlp.pt")).get("recurrent")


def test_host_side_refusals_for_a_recurrent_policy():
    """Each with its own message, before any device object is touched."""
    import simgan_amd as sg
    from simgan_amd import checkpoint
    from simgan_amd.ensemble import PolicyEnsemble
    pol = types.SimpleNamespace(is_recurrent=True, KIND=0)
    with pytest.raises(NotImplementedError, match="mirror-symmetry loss: implemented for feed-forward policies only"):
        sg.algo.PPO(pol, 0.2, 1, 1, 0.5, 0.0, symmetry_coef=1.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5, mirror_obs=np.eye(3),
                    mirror_act=np.eye(2))
    pol.ctx = types.SimpleNamespace(world=2)
    with pytest.raises(NotImplementedError, match="runs on one rank"):
        sg.algo.PPO(pol, 0.2, 1, 1, 0.5, 0.0, lr=3e-4, eps=1e-5, max_grad_norm=0.5)
    with pytest.raises(NotImplementedError, match="not for a recurrent Policy"):
        sg.algo.A2C_ACKTR(pol, 0.5, 0.01, lr=7e-4, eps=1e-5, alpha=0.99, max_grad_norm=0.5)
    with pytest.raises(NotImplementedError, match="not for a recurrent Policy"):
        sg.algo.A2C_ACKTR(pol, 0.5, 0.01, acktr=True)
    with pytest.raises(NotImplementedError, match="feed-forward members only"):
        PolicyEnsemble([pol])
    with pytest.raises(NotImplementedError, match="reference's object layout"):
        checkpoint.save_policy("/nonexistent/never_written.pt", pol)


@pytest.mark.parametrize("name", ["ppo_gru_onestep", "ppo_gru_onestep64", "ppo_gru_tiny", "ppo_gru_hopper", "ppo_gru_laikago", "ppo_gru_long"])
def test_update_restatement_reproduces_the_reference(name):
    """One whole update (advantages, losses, back-propagation through the heads and through time, clip, Adam) in float64 numpy
    against what the reference produced: the restatement the GPU tests use for widths that have no fixture."""
    g = gru_ref.load_ppo(name)
    m = g["meta"]
    r = gru_ref.ppo_update(g["params0"], m["O"], m["A"], m["H"], g, g["recurrent_hidden_states0"], g["perms"], m["ppo_epoch"],
                           m["num_mini_batch"], m["clip_param"], m["value_loss_coef"], m["entropy_coef"], m["lr"], m["eps"], m["max_grad_norm"])
    assert r["steps"] == m["steps"] == m["ppo_epoch"] * (m["N"] // (m["N"] // m["num_mini_batch"]))
    assert_close(r["advantages"], g["advantages"], rtol=1e-5, what="advantages")
    assert_close(r["losses"], g["losses"], what="losses")
    assert_close(r["adam_m"], g["adam_m"], rtol=1e-3, atol=1e-7, what="adam m")
    assert_close(r["adam_v"], g["adam_v"], rtol=1e-3, atol=1e-10, what="adam v")
    assert_close(r["params"], g["params1"], what="params after the update")


def test_alias_package_policy_refuses_the_reference_layout_when_recurrent():
    """torch.save of a policy built through the alias modules writes the reference's object layout (__reduce_ex__); for a
    recurrent policy that is refused instead of writing a file the reference may not load."""
    import pickle
    from third_party.a2c_ppo_acktr.model import Policy as AliasPolicy
    p = AliasPolicy.__new__(AliasPolicy)
    p.__dict__["recurrent"] = True
    with pytest.raises(NotImplementedError, match="reference's object layout"):
        pickle.dumps(p)
