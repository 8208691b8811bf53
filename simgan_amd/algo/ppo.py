"""PPO -- host mirror of a2c/algo/ppo.py:29-157.  update() runs entirely on the GPU
(advantage normalisation, E_p x M clipped-surrogate steps with global-norm clipping and Adam)."""
import ctypes as C

import numpy as np

from .. import _lib
from .. import symmetry as _sym
from . import diagnostics as _diag
from ..utils import derive_seed


class _ParamGroups(list):
    """`optimizer.param_groups[i]['lr'] = x` (a2c/utils.py:68-72) must reach the device."""


class _Group(dict):
    def __init__(self, owner, **kw):
        super().__init__(**kw)
        self._owner = owner

    def __setitem__(self, k, v):
        super().__setitem__(k, v)
        if k == 'lr':
            self._owner._set_lr(float(v))


class _Optimizer(object):
    def __init__(self, agent, lr, eps):
        self._agent = agent
        self.param_groups = _ParamGroups([_Group(self, lr=lr, eps=eps, betas=(0.9, 0.999))])

    def _set_lr(self, lr):
        _lib.check(self._agent.lib.sg_ppo_set_lr(self._agent.h, lr))

    def state(self):
        return self._agent.get_adam()


class PPO():
    def __init__(self,
                 actor_critic,
                 clip_param,
                 ppo_epoch,
                 num_mini_batch,
                 value_loss_coef,
                 entropy_coef,
                 symmetry_coef=0,
                 lr=None,
                 eps=None,
                 max_grad_norm=None,
                 use_clipped_value_loss=True,
                 mirror_obs=None,
                 mirror_act=None,
                 seed=0):
        self.actor_critic = actor_critic
        self.clip_param = clip_param
        self.ppo_epoch = ppo_epoch
        self.num_mini_batch = num_mini_batch
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        self.symmetry_coef = symmetry_coef
        self.mirror_obs = mirror_obs
        self.mirror_act = mirror_act
        self.is_cuda = True   # the rollout the update reads lives in HBM whatever the host tensors are

        self.recurrent = bool(getattr(actor_critic, "is_recurrent", False))   # a2c/algo/ppo.py:74-76: recurrent_generator
        if self.recurrent and getattr(actor_critic, "cnn", 0):   # the recurrent CNN base (CNN + GRU): plain PPO through time on one rank
            if mirror_obs is not None and symmetry_coef > 0:
                raise NotImplementedError("mirror-symmetry loss: not implemented for the recurrent CNN base (image observations have no "
                                          "mirror map here and the mirrored rows no hidden state); symmetry_coef > 0 needs the MLP base")
            if getattr(actor_critic.ctx, "world", 1) > 1:
                raise NotImplementedError("PPO on the recurrent CNN base runs on one rank: data-parallel PPO through time on image "
                                          f"observations is not implemented (this context's communicator has world {actor_critic.ctx.world})")
        if self.recurrent and getattr(actor_critic, "dist_kind", 0) and mirror_obs is not None and symmetry_coef > 0:
            raise NotImplementedError("mirror-symmetry loss: not for a recurrent Policy on a Discrete / MultiBinary action space (it "
                                      "compares action means of a feed-forward policy); symmetry_coef > 0 needs the MLP base and Box")
        if self.recurrent and mirror_obs is not None and symmetry_coef > 0:
            raise NotImplementedError("mirror-symmetry loss: implemented for feed-forward policies only, not for a recurrent Policy")
        if self.recurrent and getattr(actor_critic.ctx, "world", 1) > 1:
            raise NotImplementedError("PPO with a recurrent Policy runs on one rank: data-parallel PPO through time is not implemented "
                                      f"(this context's communicator has world {actor_critic.ctx.world})")
        if getattr(actor_critic, "dist_kind", 0) and mirror_obs is not None and symmetry_coef > 0:
            raise NotImplementedError("mirror-symmetry loss: it compares action means, which a Categorical / Bernoulli head (Discrete / "
                                      "MultiBinary action space) does not have; symmetry_coef > 0 needs a Box action space")
        if getattr(actor_critic, "cnn", False) and mirror_obs is not None and symmetry_coef > 0:
            raise NotImplementedError("mirror-symmetry loss: not implemented for the CNN base (image observations have no mirror map "
                                      "here); symmetry_coef > 0 needs the MLP base")
        if getattr(actor_critic, "cnn", False) and getattr(actor_critic.ctx, "world", 1) > 1:
            raise NotImplementedError("PPO on the CNN base (image observations) runs on one rank: data-parallel PPO on it is not "
                                      f"implemented (this context's communicator has world {actor_critic.ctx.world})")
        self.ctx = actor_critic.ctx
        self.lib = self.ctx.lib
        cfg = _lib.PPOConfig(float(clip_param), int(ppo_epoch), int(num_mini_batch), float(value_loss_coef),
                             float(entropy_coef), float(lr), float(eps), float(max_grad_norm),
                             1 if use_clipped_value_loss else 0)
        h = _lib.H()
        _lib.check(self.lib.sg_ppo_create(self.ctx.h, actor_critic.h, C.byref(cfg), C.byref(h)))
        self.h = h
        if hasattr(actor_critic, "_register_handle_user"):
            actor_critic._register_handle_user(self)
        self.optimizer = _Optimizer(self, lr, eps)
        self._calls = 0
        self.seed = derive_seed(seed, 0xBADC0FFEE)   # minibatch-permutation stream (a2c/storage.py:159-162)
        self._mirror_obs_fn = None
        # a2c/algo/ppo.py:110: the symmetry loss runs when mirror_obs is given and symmetry_coef > 0, plain PPO otherwise
        if mirror_obs is not None and symmetry_coef > 0:
            self._set_symmetry(float(symmetry_coef), mirror_obs, mirror_act)

    def _set_symmetry(self, coef, mirror_obs, mirror_act):
        """mirror_obs: per-row callable (applied on the host each update, any map) or [O, O] matrix (all on the device);
        mirror_act: per-row callable (must be linear: probed into its matrix) or [A, A] matrix.  Matrices act on rows:
        mirrored = M @ x."""
        ac = self.actor_critic
        if type(ac).__name__ == "SplitPolicy":
            raise NotImplementedError("mirror-symmetry loss: implemented for Policy (MLP) only, not for SplitPolicy")
        if mirror_act is None:
            raise ValueError("mirror-symmetry loss: mirror_obs was given without mirror_act")
        O, A = ac.obs_dim, ac.act_dim
        m_act = _sym.probe_linear(mirror_act, A, "mirror_act") if callable(mirror_act) else _sym.as_matrix(mirror_act, A, "mirror_act")
        if callable(mirror_obs):
            self._mirror_obs_fn, m_obs = mirror_obs, None
        else:
            m_obs = _sym.as_matrix(mirror_obs, O, "mirror_obs")
        self._m_act, self._m_obs = m_act, m_obs
        _lib.check(self.lib.sg_ppo_set_symmetry(self.h, coef, None if m_obs is None else _lib.fptr(m_obs), _lib.fptr(m_act)))

    @property
    def last_symmetry_loss(self):
        """The last update's symmetry_loss.item(), averaged over its ppo_epoch * num_mini_batch steps like the returned losses
        (0.0 with the loss off).  Not part of update()'s return value, which stays the reference's triple."""
        out = C.c_float(0.0)
        _lib.check(self.lib.sg_ppo_last_symmetry_loss(self.h, C.byref(out)))
        return float(out.value)

    def _upload_mirrored_obs(self, rollouts):
        """Callable mirror_obs: the rollout's first T steps mirrored row by row on the host and handed to the next update."""
        T, N = rollouts.num_steps, rollouts.num_processes
        if rollouts.device_resident:
            obs = np.empty(((T + 1) * N, self.actor_critic.obs_dim), np.float32)
            _lib.check(rollouts.lib.sg_rollout_download(rollouts.h, _lib.F_OBS, _lib.fptr(obs), obs.size))
        else:
            obs = rollouts._host_np(_lib.F_OBS)
        rows = _sym.mirror_rows(self._mirror_obs_fn, obs.reshape(-1, self.actor_critic.obs_dim)[:T * N])
        _lib.check(self.lib.sg_ppo_set_mirrored_obs(self.h, _lib.fptr(rows), rows.size))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.sg_ppo_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def update(self, rollouts, perms=None, fetch_losses=True):
        """a2c/algo/ppo.py:65-157 -> (value_loss_epoch, action_loss_epoch, dist_entropy_epoch).
        `perms` ([ppo_epoch, T*N] int64) injects the samplers' permutations (parity tests);
        default = the library's counter-based generator.  With a communicator of world > 1 the injected
        permutations are the reference's at num_processes = world * N: [ppo_epoch, T*N*world], the same on every rank
        (include/simgan_hip.h: sg_ppo_update).  fetch_losses=False: queue the update and return None without waiting for
        it (the losses are read later through the results ring, simgan_amd/driver.py)."""
        rollouts._push([_lib.F_OBS, _lib.F_ACTIONS, _lib.F_VALUE_PREDS, _lib.F_RETURNS, _lib.F_LOGP])
        if self.recurrent and getattr(rollouts, "device_hidden", False) and rollouts.device_resident:
            # the rollout holds its hidden states on the device (enable_device_hidden): slot 0 is handed over there, no host read
            rollouts._push([_lib.F_MASKS])
            _lib.check(self.lib.sg_ppo_set_hidden_states_rollout(self.h, rollouts.h))
        elif self.recurrent:
            # whole environments per minibatch, from the state of slot 0 (a2c/storage.py:194-251): `perms` is [ppo_epoch, N]
            rollouts._push([_lib.F_MASKS])
            hxs0 = rollouts.recurrent_hidden_states[0]
            hxs0 = np.ascontiguousarray(hxs0.numpy() if hasattr(hxs0, "numpy") else hxs0, np.float32)
            if hxs0.shape != (rollouts.num_processes, self.actor_critic.recurrent_hidden_state_size):
                raise ValueError(f"rollouts.recurrent_hidden_states[0] is {hxs0.shape}; the policy's state is "
                                 f"[{rollouts.num_processes}, {self.actor_critic.recurrent_hidden_state_size}] (build RolloutStorage with "
                                 "actor_critic.recurrent_hidden_state_size)")
            _lib.check(self.lib.sg_ppo_set_hidden_states(self.h, _lib.fptr(hxs0), hxs0.size))
        if self._mirror_obs_fn is not None:
            self._upload_mirrored_obs(rollouts)
        out = (C.c_float * 3)()
        self._calls += 1
        if perms is not None:
            perms = _lib.as_i64(perms).reshape(self.ppo_epoch, -1)   # lengths and index ranges are checked behind the C ABI
        _lib.check(self.lib.sg_ppo_update(self.h, rollouts.h, None if perms is None else _lib.i64ptr(perms),
                                          0 if perms is None else perms.size, (self.seed + self._calls) & (2 ** 64 - 1),
                                          out if fetch_losses else None))
        self._last_perm_shape = (self.ppo_epoch, rollouts.num_processes if self.recurrent else rollouts.num_steps * rollouts.num_processes)
        return (float(out[0]), float(out[1]), float(out[2])) if fetch_losses else None

    def diagnostics(self, rollouts, fetch=True, scope="rank"):
        """What one looks at after an update, over the rollout's T*N rows and the policy's current parameters, computed on the
        device (include/simgan_hip.h: sg_rollout_policy_diagnostics) -> {rows, approx_kl, approx_kl_k3, clip_fraction (at this
        agent's clip_param), entropy, ratio_min, ratio_max, explained_variance_old, explained_variance_new, value_mse}.
        fetch=False: queue it, return None without waiting; last_diagnostics() reads it later.  Call it before
        rollouts.after_update(), which overwrites obs[0].  scope="rank": this rank's rows, no collective.  scope="world"
        (sg_rollout_policy_diagnostics_world): all ranks' rows, the same bits on every rank, rows = world * T*N -- a collective
        that every rank issues at the same point; the rank scope's bits without a communicator."""
        return _diag.run(self, rollouts, self.clip_param, fetch, scope)

    def last_diagnostics(self):
        return _diag.fetch_last(self)

    def last_perms(self):
        """[ppo_epoch, T*N] permutations the last update() consumed (injected or library-drawn); [ppo_epoch, N] for a recurrent
        policy (the environments of every epoch's minibatches)."""
        perms = np.empty(self._last_perm_shape, np.int64)
        _lib.check(self.lib.sg_ppo_last_perms(self.h, _lib.i64ptr(perms), perms.size))
        return perms

    def get_adam(self):
        n = self.actor_critic.num_params
        m, v = np.empty(n, np.float32), np.empty(n, np.float32)
        step = C.c_int64(0)
        _lib.check(self.lib.sg_ppo_get_adam(self.h, _lib.fptr(m), _lib.fptr(v), n, C.byref(step)))
        return m, v, step.value

    def set_adam(self, m, v, step):
        m, v = _lib.as_f32(m).reshape(-1), _lib.as_f32(v).reshape(-1)
        _lib.check(self.lib.sg_ppo_set_adam(self.h, _lib.fptr(m), _lib.fptr(v), m.size, int(step)))
