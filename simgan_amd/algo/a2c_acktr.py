"""A2C_ACKTR -- host mirror of a2c/algo/a2c_acktr.py:30-102: acktr=False (the --algo a2c branch of a2c/main.py:123-131) and
acktr=True (--algo acktr, a2c/main.py:159-161, with KFACOptimizer of a2c/algo/kfac.py).
update() runs entirely on the GPU: evaluate_actions over the whole rollout, the A2C loss and its gradient, then either
global-norm clipping and one RMSprop step, or the K-FAC statistics, preconditioning and KL-bounded momentum-SGD step.  The
device object is an sg_ppo in A2C or ACKTR mode (include/simgan_hip.h: sg_a2c_create, sg_a2c_create_rnn, sg_a2c_create_cnn,
sg_a2c_create_cnn_rnn, sg_acktr_create).  A2C through time (recurrent=True), A2C on the CNN base (cnn=True) and A2C through time on
the recurrent CNN base (recurrent_cnn=True) are opt-in by keyword."""
import ctypes as C

import numpy as np

from .. import _lib
from ..utils import derive_seed
from . import diagnostics as _diag
from .ppo import _Group, _ParamGroups

# KFACOptimizer's constructor defaults (a2c/algo/kfac.py:97-107), which a2c/main.py:159-161 keeps
KFAC_DEFAULTS = dict(lr=0.25, momentum=0.9, stat_decay=0.99, kl_clip=0.001, damping=1e-2, weight_decay=0, Ts=1, Tf=10)


class _RMSprop(object):
    """optimizer.param_groups[0]: lr (writes reach the device: a2c/utils.py:68-72 update_linear_schedule), eps, alpha."""

    def __init__(self, agent, lr, eps, alpha):
        self._agent = agent
        self.param_groups = _ParamGroups([_Group(self, lr=lr, eps=eps, alpha=alpha, centered=False, momentum=0, weight_decay=0)])

    def _set_lr(self, lr):
        _lib.check(self._agent.lib.sg_ppo_set_lr(self._agent.h, lr))

    def state(self):
        return self._agent.get_rmsprop()


class _KFAC(object):
    """agent.optimizer of an ACKTR agent: KFACOptimizer's constants, steps, and param_groups.  KFACOptimizer.step never reads its
    param_groups, so lr writes (update_linear_schedule under --use-linear-lr-decay, a2c/main.py:203-205) are recorded in
    lr_writes and change nothing on the device."""

    def __init__(self, agent):
        self._agent = agent
        for k, v in KFAC_DEFAULTS.items():
            setattr(self, k, v)
        self.lr_writes = []
        self.param_groups = _ParamGroups([_Group(self)])

    def _set_lr(self, lr):
        self.lr_writes.append(lr)

    @property
    def steps(self):
        """KFACOptimizer.steps: the updates this agent has issued (counted on the host; no device round trip)."""
        return self._agent._steps

    def state(self):
        return self._agent.get_kfac()


class A2C_ACKTR():
    def __init__(self,
                 actor_critic,
                 value_loss_coef,
                 entropy_coef,
                 lr=None,
                 eps=None,
                 alpha=None,
                 max_grad_norm=None,
                 acktr=False,
                 seed=0,
                 recurrent=False,
                 cnn=False,
                 recurrent_cnn=False):
        is_rcnn = bool(getattr(actor_critic, "cnn", 0)) and bool(getattr(actor_critic, "is_recurrent", False))
        if recurrent_cnn:
            if not is_rcnn:
                raise ValueError("A2C_ACKTR(recurrent_cnn=True) takes a Policy with the recurrent CNN base (a [C, 84, 84] obs_shape, "
                                 "base_kwargs={'recurrent': True}, recurrent_cnn=True); this policy has another base: leave the keyword out")
            if acktr:
                raise NotImplementedError("A2C_ACKTR(acktr=True, recurrent_cnn=True): ACKTR is not implemented for the recurrent CNN "
                                          "base: K-FAC has neither convolution nor GRU statistics here (the reference refuses "
                                          "--recurrent-policy with acktr too); acktr=False (A2C through time) runs")
            if getattr(getattr(actor_critic, "ctx", None), "world", 1) > 1:
                raise NotImplementedError("A2C_ACKTR(recurrent_cnn=True): A2C on the recurrent CNN base runs on one rank "
                                          f"(this context's world is {actor_critic.ctx.world}): data-parallel A2C through time on "
                                          "images is not implemented")
            cnn = recurrent = True   # the checks below then see both of its bases opted in
        if acktr:
            given = [k for k, v in (("lr", lr), ("eps", eps), ("alpha", alpha), ("max_grad_norm", max_grad_norm)) if v is not None]
            if given:
                raise NotImplementedError(f"A2C_ACKTR(acktr=True) with {', '.join(given)}: ACKTR's K-FAC optimizer "
                                          "(a2c/algo/kfac.py) ignores the RMSprop arguments -- it steps with its own lr 0.25 and "
                                          "bounds the step by KL, not by a gradient-norm clip; call it as a2c/main.py:159-161 "
                                          "does, without lr, eps, alpha and max_grad_norm")
        if type(actor_critic).__name__ == "SplitPolicy":
            raise NotImplementedError("A2C_ACKTR: implemented for Policy (MLP) only, not for SplitPolicy")
        is_cnn = bool(getattr(actor_critic, "cnn", 0))
        if is_rcnn and not recurrent_cnn:
            raise NotImplementedError("A2C_ACKTR: not implemented for the recurrent CNN base (image observations with "
                                      "base_kwargs={'recurrent': True}), in any mode -- acktr, cnn=True or recurrent=True; PPO is")
        if cnn and acktr:
            raise NotImplementedError("A2C_ACKTR(acktr=True, cnn=True): ACKTR is not implemented for the CNN base (image "
                                      "observations): K-FAC has no convolution statistics here; acktr=False (A2C) runs")
        if is_cnn and not cnn:
            raise NotImplementedError("A2C_ACKTR: not implemented for the CNN base (image observations), in either mode; PPO is "
                                      "(A2C on the CNN base is opt-in: A2C_ACKTR(..., acktr=False, cnn=True); ACKTR on it is not built)")
        if cnn and not is_cnn:
            raise ValueError("A2C_ACKTR(cnn=True) takes a Policy with the CNN base (a [C, 84, 84] obs_shape); this policy has "
                             "none: leave the keyword out")
        if cnn and getattr(getattr(actor_critic, "ctx", None), "world", 1) > 1:
            raise NotImplementedError("A2C_ACKTR(cnn=True): A2C on the CNN base (image observations) runs on one rank "
                                      f"(this context's world is {actor_critic.ctx.world}): data-parallel A2C is not implemented")
        is_rec = bool(getattr(actor_critic, "is_recurrent", False))
        if is_rec and acktr and getattr(actor_critic, "dist_kind", 0):
            raise NotImplementedError("A2C_ACKTR(acktr=True): ACKTR is not built for a recurrent Policy on a Discrete / MultiBinary action "
                                      "space (the reference refuses --recurrent-policy with acktr, and K-FAC's Fisher sampling is "
                                      "built for the Gaussian head); acktr=False, recurrent=True (A2C through time) runs")
        if is_rec and (acktr or not recurrent):
            raise NotImplementedError("A2C_ACKTR: implemented for feed-forward policies only, not for a recurrent Policy "
                                      "(the reference allows --recurrent-policy with a2c and refuses it with acktr); "
                                      "A2C through time is opt-in: A2C_ACKTR(..., acktr=False, recurrent=True)")
        if recurrent and not is_rec:
            raise ValueError("A2C_ACKTR(recurrent=True) takes a recurrent Policy (base_kwargs={'recurrent': True}); this policy is "
                             "feed-forward: leave the keyword out")
        if acktr and getattr(actor_critic, "dist_kind", 0):
            raise NotImplementedError("A2C_ACKTR(acktr=True): K-FAC's Fisher sampling is built for the Gaussian head (Box action spaces) "
                                      "only, not for a Discrete / MultiBinary policy; acktr=False (A2C) runs")
        if acktr:
            self._init_acktr(actor_critic, value_loss_coef, entropy_coef, seed)
            return
        missing = [k for k, v in (("lr", lr), ("eps", eps), ("alpha", alpha), ("max_grad_norm", max_grad_norm)) if v is None]
        if missing:
            raise ValueError(f"A2C_ACKTR(acktr=False) needs {', '.join(missing)} (RMSprop and clip_grad_norm_ take them; "
                             "a2c/main.py:123-131 passes --lr, --eps, --alpha, --max-grad-norm)")
        self.actor_critic = actor_critic
        self.acktr = acktr
        self.recurrent = is_rec
        self.cnn = is_cnn
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.is_cuda = True   # the rollout the update reads lives in HBM whatever the host tensors are

        self.ctx = actor_critic.ctx
        self.lib = self.ctx.lib
        cfg = _lib.A2CConfig(float(value_loss_coef), float(entropy_coef), float(lr), float(eps), float(alpha), float(max_grad_norm))
        h = _lib.H()
        create = (self.lib.sg_a2c_create_cnn_rnn if is_rcnn else self.lib.sg_a2c_create_cnn if is_cnn else
                  self.lib.sg_a2c_create_rnn if is_rec else self.lib.sg_a2c_create)
        _lib.check(create(self.ctx.h, actor_critic.h, C.byref(cfg), C.byref(h)))
        self.h = h
        if hasattr(actor_critic, "_register_handle_user"):
            actor_critic._register_handle_user(self)
        self.optimizer = _RMSprop(self, lr, eps, alpha)

    def _init_acktr(self, actor_critic, value_loss_coef, entropy_coef, seed):
        self.actor_critic = actor_critic
        self.acktr = True
        self.recurrent = False
        self.cnn = False
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = None
        self.is_cuda = True
        self.seed = derive_seed(seed, 0xACC7)   # the library's own value noise (a2c/algo/a2c_acktr.py:82)
        self._steps = 0
        self.ctx = actor_critic.ctx
        self.lib = self.ctx.lib
        d = KFAC_DEFAULTS
        cfg = _lib.ACKTRConfig(float(value_loss_coef), float(entropy_coef), d["lr"], d["momentum"], d["stat_decay"], d["kl_clip"],
                               d["damping"], d["Tf"])
        h = _lib.H()
        _lib.check(self.lib.sg_acktr_create(self.ctx.h, actor_critic.h, C.byref(cfg), C.byref(h)))
        self.h = h
        if hasattr(actor_critic, "_register_handle_user"):
            actor_critic._register_handle_user(self)
        self.optimizer = _KFAC(self)

    def kfac_modules(self):
        """[(name, (out, in))] of KFACOptimizer.modules in order (split_bias: a bias is an [out, 1] AddBias module)."""
        p = self.actor_critic
        O, A, H, Hc = p.obs_dim, p.act_dim, p.hidden_size, p.critic_hidden
        mods = []
        for name, (o, i) in (("actor.0", (H, O)), ("actor.2", (H, H)), ("critic.0", (Hc, O)), ("critic.2", (Hc, Hc)),
                             ("critic_linear", (1, Hc)), ("dist.fc_mean", (A, H))):
            mods += [(name + ".weight", (o, i)), (name + ".bias", (o, 1))]
        mods.append(("dist.logstd", (A, 1)))
        return mods

    def get_kfac(self):
        """-> {"m_aa": [13 arrays [in, in]], "m_gg": [13 arrays [out, out]], "momentum_buffer": flat, "steps": int}, the K-FAC
        state of a2c/algo/kfac.py in module (state_dict) order."""
        mods = self.kfac_modules()
        n_aa = sum(i * i for _, (o, i) in mods)
        n_gg = sum(o * o for _, (o, i) in mods)
        aa, gg = np.empty(n_aa, np.float32), np.empty(n_gg, np.float32)
        buf = np.empty(self.actor_critic.num_params, np.float32)
        steps = C.c_int64(0)
        _lib.check(self.lib.sg_acktr_get_state(self.h, _lib.fptr(aa), n_aa, _lib.fptr(gg), n_gg, _lib.fptr(buf), buf.size,
                                               C.byref(steps)))
        out_aa, out_gg, ia, ig = [], [], 0, 0
        for _, (o, i) in mods:
            out_aa.append(aa[ia:ia + i * i].reshape(i, i))
            out_gg.append(gg[ig:ig + o * o].reshape(o, o))
            ia += i * i
            ig += o * o
        return {"m_aa": out_aa, "m_gg": out_gg, "momentum_buffer": buf, "steps": steps.value}

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.sg_ppo_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def update(self, rollouts, fetch_losses=True, value_noise=None):
        """a2c/algo/a2c_acktr.py:52-102 -> (value_loss, action_loss, dist_entropy).  fetch_losses=False: queue the update and
        return None without waiting for it (the losses are read later through the results ring, simgan_amd/driver.py).
        value_noise (ACKTR only): the update's torch.randn(values.size()) [T, N, 1] instead of the library's own draws."""
        rollouts._push([_lib.F_OBS, _lib.F_ACTIONS, _lib.F_RETURNS])
        if self.recurrent:
            self._hand_over_hidden(rollouts)
        seed = 0
        if self.acktr:
            if value_noise is not None:
                eps = np.ascontiguousarray(np.asarray(value_noise, np.float32).reshape(-1))
                _lib.check(self.lib.sg_acktr_set_value_noise(self.h, _lib.fptr(eps), eps.size))
            seed = self.seed
        elif value_noise is not None:
            raise ValueError("value_noise is ACKTR's (acktr=True); A2C draws no noise")
        out = (C.c_float * 3)()
        _lib.check(self.lib.sg_ppo_update(self.h, rollouts.h, None, 0, seed, out if fetch_losses else None))
        if self.acktr:
            self._steps += 1
        return (float(out[0]), float(out[1]), float(out[2])) if fetch_losses else None

    def _hand_over_hidden(self, rollouts):
        """recurrent_hidden_states[0] for the next update, as PPO.update hands it over: device to device from a rollout that
        holds its hidden states there (enable_device_hidden), from the host tensor otherwise."""
        rollouts._push([_lib.F_MASKS])
        if getattr(rollouts, "device_hidden", False) and rollouts.device_resident:
            _lib.check(self.lib.sg_ppo_set_hidden_states_rollout(self.h, rollouts.h))
            return
        hxs0 = rollouts.recurrent_hidden_states[0]
        hxs0 = np.ascontiguousarray(hxs0.numpy() if hasattr(hxs0, "numpy") else hxs0, np.float32)
        if hxs0.shape != (rollouts.num_processes, self.actor_critic.recurrent_hidden_state_size):
            raise ValueError(f"rollouts.recurrent_hidden_states[0] is {hxs0.shape}; the policy's state is "
                             f"[{rollouts.num_processes}, {self.actor_critic.recurrent_hidden_state_size}] (build RolloutStorage with "
                             "actor_critic.recurrent_hidden_state_size)")
        _lib.check(self.lib.sg_ppo_set_hidden_states(self.h, _lib.fptr(hxs0), hxs0.size))

    def diagnostics(self, rollouts, fetch=True, scope="rank"):
        """PPO.diagnostics for A2C / ACKTR (both modes): the same ten numbers with clip_param = inf, so clip_fraction is exactly
        0 -- neither learner clips a ratio; approx_kl is the measured KL to set beside ACKTR's kl_clip.  The rollout's
        action_log_probs and value_preds (the collection's) are read, which update() itself does not need.  scope: PPO's; A2C and
        ACKTR run at world 1, where "world" gives the rank scope's bits."""
        if getattr(self, "cnn", False):
            raise NotImplementedError("A2C_ACKTR.diagnostics: the diagnostics kernels do not cover the CNN base (image "
                                      "observations); update() returns the three losses")
        return _diag.run(self, rollouts, float("inf"), fetch, scope)

    def last_diagnostics(self):
        return _diag.fetch_last(self)

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
