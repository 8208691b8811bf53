"""CPU: the host side of recurrent collection on the device -- the C ABI of the rollout's hidden-state buffer, of the one-launch
recurrent step and of PPO's device-side hand-over is declared, exported and prototyped, and collect(on_device=True) lets a
recurrent policy through exactly when the rollout holds its hidden states (driver._check_on_device)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW = ("sg_rollout_enable_hidden", "sg_rollout_upload_hidden", "sg_rollout_download_hidden", "sg_rollout_act_step_rnn",
       "sg_ppo_set_hidden_states_rollout")


def test_the_five_functions_are_declared_exported_and_prototyped():
    import ctypes
    from simgan_amd import _lib
    header = open(os.path.join(ROOT, "include", "simgan_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym in NEW:
        assert f"SG_API int {sym}(" in header, sym
        assert hasattr(lib, sym), sym
        assert sym in _lib.PROTOTYPES, sym
    restype, argtypes = _lib.PROTOTYPES["sg_rollout_act_step_rnn"]
    assert restype is ctypes.c_int and len(argtypes) == 9      # r, p, t, obs, masks, noise, seed, deterministic, action
    assert len(_lib.PROTOTYPES["sg_rollout_act_step"][1]) == 8   # the feed-forward step keeps its signature
    assert len(_lib.PROTOTYPES["sg_ppo_set_hidden_states_rollout"][1]) == 2


class _Rollout:
    def __init__(self, device_resident=True, dup_sym=False, device_hidden=None):
        self.device_resident, self.dup_sym = device_resident, dup_sym
        if device_hidden is not None:
            self.device_hidden = device_hidden


class _Policy:
    def __init__(self, recurrent, dist_kind=None):
        self.is_recurrent = recurrent
        if dist_kind is not None:
            self.dist_kind = dist_kind


def test_check_on_device_lets_a_recurrent_policy_through_with_device_hidden():
    from simgan_amd import _lib
    from simgan_amd.driver import _check_on_device
    who = "PpoLearner.collect"
    _check_on_device(_Rollout(device_hidden=True), _Policy(True), False, who)
    _check_on_device(_Rollout(device_hidden=True), _Policy(False), False, who)
    _check_on_device(_Rollout(), _Policy(False), False, who)
    today = r"PpoLearner.collect\(on_device=True\): the policy is recurrent and the device rollout holds no hidden state$"
    for ro in (_Rollout(), _Rollout(device_hidden=False)):      # a rollout object from before the attribute, and one without the opt-in
        with pytest.raises(ValueError, match=today):
            _check_on_device(ro, _Policy(True), False, who)
    # the checks in front of it keep their order and their texts
    with pytest.raises(ValueError, match="the rollout is not device-resident"):
        _check_on_device(_Rollout(device_resident=False, device_hidden=True), _Policy(True), False, who)
    with pytest.raises(ValueError, match="the rollout is mirror-augmented"):
        _check_on_device(_Rollout(dup_sym=True, device_hidden=True), _Policy(True), False, who)
    with pytest.raises(ValueError, match="the policy has a Discrete / MultiBinary action space"):
        _check_on_device(_Rollout(device_hidden=True), _Policy(False, _lib.DIST_CATEGORICAL), False, who)
