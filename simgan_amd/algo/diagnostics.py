"""Update diagnostics on the device (include/simgan_hip.h: sg_rollout_policy_diagnostics): approximate KL, clip fraction,
entropy, ratio range, explained variance and value error of the agent's policy over the T*N rows of a rollout, which the
reference's learners do not return (a2c/algo/ppo.py:65-157, a2c/algo/a2c_acktr.py:52-102).  Shared by PPO and A2C_ACKTR."""
import ctypes as C

import numpy as np

from .. import _lib

NAMES = ("rows", "approx_kl", "approx_kl_k3", "clip_fraction", "entropy", "ratio_min", "ratio_max", "explained_variance_old",
         "explained_variance_new", "value_mse")


# include/simgan_hip.h: sg_disc_diagnostics -- Discriminator.diagnostics / GailDynLearner.update(disc_diagnostics=True)
DISC_NAMES = ("policy_rows", "expert_rows", "policy_accuracy", "expert_accuracy", "policy_logit_mean", "policy_logit_std",
              "expert_logit_mean", "expert_logit_std", "policy_bce", "expert_bce", "reward_mean", "reward_std", "reward_min", "reward_max",
              "policy_grad_norm_mean", "expert_grad_norm_mean", "mid_grad_norm_mean", "mid_grad_pen", "grad_norm_max")


SCOPES = ("rank", "world")


def check_scope(scope):
    """"rank": this rank's rows, no collective.  "world": all ranks' rows, the same bits on every rank -- a collective, which every
    rank issues at the same point of its stream's collectives.  Anything else is a ValueError, before any device call."""
    if not (isinstance(scope, str) and scope in SCOPES):
        raise ValueError(f'scope = {scope!r}: "rank" or "world"')
    return scope


def _as_dict(out):
    return {k: float(out[i]) for i, k in enumerate(NAMES)}


def run(agent, rollouts, clip_param, fetch=True, scope="rank"):
    """Pushes the fields the launch reads (as update() does: a host-resident rollout works and gives the device-resident one's
    numbers), hands a recurrent policy the hidden states of slot 0 the way PPO.update does, and queues the two launches.
    fetch=True: wait and return the dict of NAMES; False: return None (fetch_last reads the result later).  scope: check_scope."""
    call = {"rank": "sg_rollout_policy_diagnostics", "world": "sg_rollout_policy_diagnostics_world"}[check_scope(scope)]
    pol = agent.actor_critic
    if getattr(pol, "cnn", 0) and getattr(pol, "is_recurrent", False):
        raise NotImplementedError("diagnostics: not built for the recurrent CNN base (the launch runs the MLP trunks only); evaluate the "
                                  "rollout through Policy.evaluate_actions and reduce on the host")
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
    _lib.check(getattr(agent.lib, call)(rollouts.h, pol.h, float(clip_param), None if hxs0 is None else _lib.fptr(hxs0),
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


def run_disc(disc, rollouts, fetch=True, slot=0, scope="rank"):
    """Discriminator.diagnostics: pushes OBS_FEAT as the other discriminator calls do (a host-resident rollout gives the
    device-resident one's numbers) and queues the two launches into `slot`.  fetch=True: wait and return the dict of DISC_NAMES;
    False: return None (fetch_disc reads the slot later).  scope: check_scope."""
    call = {"rank": "sg_disc_diagnostics", "world": "sg_disc_diagnostics_world"}[check_scope(scope)]
    rollouts._push([_lib.F_OBS_FEAT])
    out = (C.c_double * len(DISC_NAMES))()
    _lib.check(getattr(disc.lib, call)(disc.h, rollouts.h, int(slot), out if fetch else None))
    return {k: float(out[i]) for i, k in enumerate(DISC_NAMES)} if fetch else None


def fetch_disc(disc, slot=0):
    """The pending result of `slot`: waits for it.  An error when none is pending there."""
    out = (C.c_double * len(DISC_NAMES))()
    _lib.check(disc.lib.sg_disc_diagnostics_fetch(disc.h, int(slot), out))
    return {k: float(out[i]) for i, k in enumerate(DISC_NAMES)}
