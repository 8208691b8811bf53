"""Update diagnostics on the device (include/simgan_hip.h: sg_rollout_policy_diagnostics): approximate KL, clip fraction,
entropy, ratio range, explained variance and value error of the agent's policy over the T*N rows of a rollout, which the
reference's learners do not return (a2c/algo/ppo.py:65-157, a2c/algo/a2c_acktr.py:52-102).  Shared by PPO and A2C_ACKTR."""
import ctypes as C

import numpy as np

from .. import _lib

NAMES = ("rows", "approx_kl", "approx_kl_k3", "clip_fraction", "entropy", "ratio_min", "ratio_max", "explained_variance_old",
         "explained_variance_new", "value_mse")


def _as_dict(out):
    return {k: float(out[i]) for i, k in enumerate(NAMES)}


def run(agent, rollouts, clip_param, fetch=True):
    """Pushes the fields the launch reads (as update() does: a host-resident rollout works and gives the device-resident one's
    numbers), hands a recurrent policy the hidden states of slot 0 the way PPO.update does, and queues the two launches.
    fetch=True: wait and return the dict of NAMES; False: return None (fetch_last reads the result later)."""
    pol = agent.actor_critic
    rollouts._push([_lib.F_OBS, _lib.F_ACTIONS, _lib.F_VALUE_PREDS, _lib.F_RETURNS, _lib.F_LOGP])
    hxs0 = None
    if getattr(pol, "is_recurrent", False):
        rollouts._push([_lib.F_MASKS])
        if not (getattr(rollouts, "device_hidden", False) and rollouts.device_resident):
            hxs0 = rollouts.recurrent_hidden_states[0]
            hxs0 = np.ascontiguousarray(hxs0.numpy() if hasattr(hxs0, "numpy") else hxs0, np.float32)
            if hxs0.shape != (rollouts.num_processes, pol.recurrent_hidden_state_size):
                raise ValueError(f"rollouts.recurrent_hidden_states[0] is {hxs0.shape}; the policy's state is "
                                 f"[{rollouts.num_processes}, {pol.recurrent_hidden_state_size}] (build RolloutStorage with "
                                 "actor_critic.recurrent_hidden_state_size)")
    out = (C.c_double * len(NAMES))()
    _lib.check(agent.lib.sg_rollout_policy_diagnostics(rollouts.h, pol.h, float(clip_param), None if hxs0 is None else _lib.fptr(hxs0),
                                                       out if fetch else None))
    agent._diag_rollouts = None if fetch else rollouts
    return _as_dict(out) if fetch else None


def fetch_last(agent):
    """The result of the last diagnostics(fetch=False): waits for it.  An error when none is pending."""
    ro = getattr(agent, "_diag_rollouts", None)
    if ro is None:
        raise RuntimeError("last_diagnostics: no diagnostics are pending (call diagnostics(rollouts, fetch=False) first)")
    out = (C.c_double * len(NAMES))()
    _lib.check(agent.lib.sg_rollout_policy_diagnostics_fetch(ro.h, out))
    agent._diag_rollouts = None
    return _as_dict(out)
