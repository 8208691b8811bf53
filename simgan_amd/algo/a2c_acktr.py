"""A2C_ACKTR -- host mirror of a2c/algo/a2c_acktr.py:30-102 with acktr=False (the --algo a2c branch of a2c/main.py:123-131).
update() runs entirely on the GPU: evaluate_actions over the whole rollout, the A2C loss, its gradient, global-norm clipping
and one RMSprop step.  The device object is an sg_ppo in A2C mode (include/simgan_hip.h: sg_a2c_create)."""
import ctypes as C

import numpy as np

from .. import _lib
from .ppo import _Group, _ParamGroups


class _RMSprop(object):
    """optimizer.param_groups[0]: lr (writes reach the device: a2c/utils.py:68-72 update_linear_schedule), eps, alpha."""

    def __init__(self, agent, lr, eps, alpha):
        self._agent = agent
        self.param_groups = _ParamGroups([_Group(self, lr=lr, eps=eps, alpha=alpha, centered=False, momentum=0, weight_decay=0)])

    def _set_lr(self, lr):
        _lib.check(self._agent.lib.sg_ppo_set_lr(self._agent.h, lr))

    def state(self):
        return self._agent.get_rmsprop()


class A2C_ACKTR():
    def __init__(self,
                 actor_critic,
                 value_loss_coef,
                 entropy_coef,
                 lr=None,
                 eps=None,
                 alpha=None,
                 max_grad_norm=None,
                 acktr=False):
        if acktr:
            raise NotImplementedError("A2C_ACKTR(acktr=True): ACKTR (the K-FAC optimizer of a2c/algo/kfac.py) is not implemented; "
                                      "acktr=False (A2C with RMSprop) is")
        if type(actor_critic).__name__ == "SplitPolicy":
            raise NotImplementedError("A2C_ACKTR: implemented for Policy (MLP) only, not for SplitPolicy")
        missing = [k for k, v in (("lr", lr), ("eps", eps), ("alpha", alpha), ("max_grad_norm", max_grad_norm)) if v is None]
        if missing:
            raise ValueError(f"A2C_ACKTR(acktr=False) needs {', '.join(missing)} (RMSprop and clip_grad_norm_ take them; "
                             "a2c/main.py:123-131 passes --lr, --eps, --alpha, --max-grad-norm)")
        self.actor_critic = actor_critic
        self.acktr = acktr
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.is_cuda = True   # the rollout the update reads lives in HBM whatever the host tensors are

        self.ctx = actor_critic.ctx
        self.lib = self.ctx.lib
        cfg = _lib.A2CConfig(float(value_loss_coef), float(entropy_coef), float(lr), float(eps), float(alpha), float(max_grad_norm))
        h = _lib.H()
        _lib.check(self.lib.sg_a2c_create(self.ctx.h, actor_critic.h, C.byref(cfg), C.byref(h)))
        self.h = h
        if hasattr(actor_critic, "_register_handle_user"):
            actor_critic._register_handle_user(self)
        self.optimizer = _RMSprop(self, lr, eps, alpha)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.sg_ppo_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def update(self, rollouts, fetch_losses=True):
        """a2c/algo/a2c_acktr.py:52-102 -> (value_loss, action_loss, dist_entropy).  fetch_losses=False: queue the update and
        return None without waiting for it (the losses are read later through the results ring, simgan_amd/driver.py)."""
        rollouts._push([_lib.F_OBS, _lib.F_ACTIONS, _lib.F_RETURNS])
        out = (C.c_float * 3)()
        _lib.check(self.lib.sg_ppo_update(self.h, rollouts.h, None, 0, 0, out if fetch_losses else None))
        return (float(out[0]), float(out[1]), float(out[2])) if fetch_losses else None

    def get_rmsprop(self):
        """-> (square_avg flat in state_dict order, optimizer steps taken)."""
        n = self.actor_critic.num_params
        sq = np.empty(n, np.float32)
        step = C.c_int64(0)
        _lib.check(self.lib.sg_a2c_get_rmsprop(self.h, _lib.fptr(sq), n, C.byref(step)))
        return sq, step.value

    def set_rmsprop(self, square_avg, step):
        sq = _lib.as_f32(square_avg).reshape(-1)
        _lib.check(self.lib.sg_a2c_set_rmsprop(self.h, _lib.fptr(sq), sq.size, int(step)))
