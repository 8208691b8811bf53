"""RolloutStorage -- host mirror of a2c/storage.py:31-192 with a device-resident twin.

The reference mains read and write the buffers by slicing (`rollouts.obs[0].copy_(obs)`,
`rollouts.rewards[step] = ...`), so the attributes stay ordinary host tensors with the
reference's shapes.  The HBM copy inside libsimgan_hip.so is refreshed per operation:
  * default (drop-in) mode: every device operation first uploads the fields it reads -- those whose host tensor
    changed since the device copy last matched it -- and downloads the fields it writes: PCIe-inclusive, coherent with
    host-side edits.  "Changed" is read off the tensor itself: every in-place torch operation on the attribute or on
    a slice of it (`rollouts.rewards[step] = ...`, `rollouts.obs[0].copy_(obs)`, `insert`) bumps its `_version`; an
    attribute that is re-bound is a different tensor.  So `obs_feat` crosses PCIe once per rollout, not once per
    discriminator epoch.  Writes torch cannot see (through a `.numpy()` view of the attribute) need
    `mark_host_written()`; without torch (plain numpy mirrors) and with SG_ROLLOUT_ALWAYS_UPLOAD=1 every call uploads;
    SG_ROLLOUT_VERIFY=1 (debugging a port) checksums every field the tracker takes for unchanged and raises when it was
    written behind torch's back;
  * `device_resident = True` (driver / bench fast path): uploads are skipped, the device copy is
    the source of truth and `sync_from_device()` refreshes the host view on demand.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib
from .utils import to_host_tensor, torch

_VERIFY = os.environ.get("SG_ROLLOUT_VERIFY") == "1"

# data pointer of a rollout's obs_feat host tensor -> the rollout: lets Discriminator.predict_reward_combined recognise the unchanged
# main's `rollouts.obs_feat[step + 1]` / `rollouts.masks[step]` slices (a2c/main_gail_dyn_ppo.py:276-280) and serve the loop's T
# calls from one fused launch (simgan_amd/algo/gail.py)
_BY_FEAT_PTR = weakref.WeakValueDictionary()


def rollout_of_feat_slice(t):
    """The RolloutStorage whose obs_feat tensor `t` is a slice of (torch view), or None."""
    base = getattr(t, "_base", None)
    if base is None or not hasattr(base, "data_ptr"):
        return None
    ro = _BY_FEAT_PTR.get(base.data_ptr())
    return ro if ro is not None and ro.obs_feat is base else None

_FIELD_ATTR = {
    _lib.F_OBS: "obs", _lib.F_OBS_FEAT: "obs_feat", _lib.F_ACTIONS: "actions",
    _lib.F_REWARDS: "rewards", _lib.F_VALUE_PREDS: "value_preds", _lib.F_RETURNS: "returns",
    _lib.F_LOGP: "action_log_probs", _lib.F_MASKS: "masks", _lib.F_BAD_MASKS: "bad_masks",
}


def _put(dst, src):
    """src (tensor / array-like) into the host slot dst, through torch where dst is a tensor (its version counter moves)."""
    if torch is not None and hasattr(dst, "copy_"):
        dst.copy_(src if hasattr(src, "dim") else torch.as_tensor(np.asarray(src, np.int64 if dst.dtype == torch.int64 else np.float32)))
    else:
        dst[...] = np.asarray(src, dst.dtype)


class RolloutStorage(object):
    def __init__(self, num_steps, num_processes, obs_shape, action_space,
                 recurrent_hidden_state_size, feat_len=0, ctx=None):
        T, N = int(num_steps), int(num_processes)
        if len(obs_shape) not in (1, 3):
            raise NotImplementedError("1-D observations only")
        # image observations (a2c/storage.py:34: obs [T+1, N, *obs_shape]) for the CNN base: the host tensor keeps the reference's
        # 5-D shape, the device twin holds each image as one row of C*H*W floats
        self.image_shape = tuple(int(x) for x in obs_shape) if len(obs_shape) == 3 else None
        # a2c/storage.py:42-48: Discrete -> actions [T, N, 1] int64 (the class index; float32 on the device), else [T, N, shape[0]]
        self.discrete = action_space.__class__.__name__ == 'Discrete'
        self.box_actions = action_space.__class__.__name__ == 'Box'
        O, A, F = int(np.prod(obs_shape)), 1 if self.discrete else int(action_space.shape[0]), int(feat_len)
        self.ctx = ctx or _lib.Context.default()   # (first: creating the context is what initialises the HIP runtime, with its settings)
        self.lib = self.ctx.lib
        # the host tensors live in page-locked memory (sg_host_alloc): ordinary CPU tensors to whoever slices them, one DMA
        # per field at the link's speed to sg_rollout_upload / _download
        z = lambda *s: to_host_tensor(_lib.pinned_array(s, 0.0))  # noqa: E731
        o = lambda *s: to_host_tensor(_lib.pinned_array(s, 1.0))  # noqa: E731
        self.obs = z(T + 1, N, *(self.image_shape or (O,)))
        self.obs_feat = z(T + 1, N, F)
        self.recurrent_hidden_states = z(T + 1, N, recurrent_hidden_state_size)
        self.rewards = z(T, N, 1)
        self.value_preds = z(T + 1, N, 1)
        self.returns = z(T + 1, N, 1)
        self.action_log_probs = z(T, N, 1)
        self.actions = z(T, N, A)
        if self.discrete:
            self.actions = self.actions.long() if hasattr(self.actions, "long") else self.actions.astype(np.int64)
        self.masks = o(T + 1, N, 1)
        # Masks that indicate whether it's a true terminal state or time limit end state
        self.bad_masks = o(T + 1, N, 1)
        if hasattr(self.obs_feat, "data_ptr") and self.obs_feat.numel():
            _BY_FEAT_PTR[self.obs_feat.data_ptr()] = self
        self.num_steps = T
        self.num_processes = N
        self.step = 0
        self.obs_dim, self.act_dim, self.feat_len = O, A, F
        self._device_resident = False
        self._host_written = False   # insert() wrote host slots since the last after_update()
        self._synced = {}            # field -> (weakref of the host tensor, its _version) when the device copy last matched it
        self._crcs = {}              # SG_ROLLOUT_VERIFY=1: field -> crc32 of the host content at that moment
        self.bytes_uploaded = 0      # host -> device traffic of this rollout so far (bench.py's `dropin` leg reads it)
        self._dup = None             # enable_dup_sym: {"n", "m_obs" | None, "m_act", "obs_fn" | None}
        self.device_hidden = False   # enable_device_hidden: the device twin holds recurrent_hidden_states too

        h = _lib.H()
        _lib.check(self.lib.sg_rollout_create(self.ctx.h, T, N, O, A, F, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.sg_rollout_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def to(self, device):
        return None  # host tensors stay on the host; the HBM twin lives in the library

    # ----------------------------------------------------------------- host <-> device
    def _host_np(self, field):
        t = getattr(self, _FIELD_ATTR[field])
        a = t.numpy() if hasattr(t, "numpy") else t
        if field == _lib.F_ACTIONS and self.__dict__.get("discrete"):
            if a.dtype != np.int64 or not a.flags["C_CONTIGUOUS"]:
                raise TypeError("rollouts.actions of a Discrete action space must stay a contiguous int64 host tensor")
            return a
        if a.dtype != np.float32 or not a.flags["C_CONTIGUOUS"]:
            raise TypeError(f"rollouts.{_FIELD_ATTR[field]} must stay a contiguous float32 host tensor")
        return a

    @property
    def device_resident(self):
        return self._device_resident

    @device_resident.setter
    def device_resident(self, value):
        # resident operations change the device copy without telling the host mirrors: nothing is known to match afterwards
        self._device_resident = bool(value)
        self._synced = {}

    def _stamp(self, field):
        """What identifies the present content of a host field: (the tensor, its version counter), or None when writes to
        it cannot be seen (numpy mirrors)."""
        t = getattr(self, _FIELD_ATTR[field])
        v = getattr(t, "_version", None)
        return None if v is None else (weakref.ref(t), v)

    def _matches(self, field):
        was, now = self._synced.get(field), self._stamp(field)
        return was is not None and now is not None and was[0]() is now[0]() and was[1] == now[1]

    def mark_host_written(self, fields=None):
        """Tell the rollout that host fields were written behind torch's back (through a numpy view)."""
        for f in (fields if fields is not None else list(self._synced)):
            self._synced.pop(f, None)

    def _crc(self, field):
        import zlib
        return zlib.crc32(self._host_np(field))

    def sync_to_device(self, fields=None):
        if self._dup is not None and self.device_resident:
            return self._sync_to_device_dup_sym(fields)
        for f in (fields if fields is not None else _FIELD_ATTR):
            a = self._host_np(f)
            if a.size:
                up = a.astype(np.float32) if a.dtype == np.int64 else a   # Discrete actions: int64 on the host, float32 on the device
                _lib.check(self.lib.sg_rollout_upload(self.h, f, _lib.fptr(up), up.size))
                self.bytes_uploaded += up.nbytes
            self._synced[f] = self._stamp(f)
            if _VERIFY:
                self._crcs[f] = self._crc(f)
        if fields is None and self.__dict__.get("device_hidden"):
            hx = self._hidden_np()
            _lib.check(self.lib.sg_rollout_upload_hidden(self.h, _lib.fptr(hx), hx.size))
            self.bytes_uploaded += hx.nbytes

    def _hidden_np(self):
        t = self.recurrent_hidden_states
        a = t.numpy() if hasattr(t, "numpy") else t
        if a.dtype != np.float32 or not a.flags["C_CONTIGUOUS"]:
            raise TypeError("rollouts.recurrent_hidden_states must stay a contiguous float32 host tensor")
        return a

    def enable_device_hidden(self):
        """Opt in: the device twin also holds recurrent_hidden_states ([T+1, N, H], uploaded from the host tensor now), so that a
        recurrent policy can act through act_step() -- one launch per step that reads hidden slot `step` and writes slot
        `step + 1` on the device -- and PPO.update / the learners' GAE take the states from there.  sync_to_device() /
        sync_from_device() without a field list move the buffer with the fields; after an on-device collection the host tensor
        is stale until sync_from_device(), like value_preds.  Device-resident rollouts only, not mirror-augmented ones."""
        H = int(self.recurrent_hidden_states.shape[-1])
        if self.__dict__.get("image_shape"):
            raise NotImplementedError("enable_device_hidden: the rollout holds image observations, which only the feed-forward CNN base "
                                      "reads: there is no hidden state to keep on the device")
        if not self.device_resident:
            raise ValueError("enable_device_hidden: the rollout is not device-resident (rollouts.device_resident = True): in drop-in "
                             "mode the host tensors are the rollout")
        if H <= 1:
            raise ValueError(f"enable_device_hidden: recurrent_hidden_state_size is {H}: the rollout was built for a feed-forward "
                             "policy, which has no hidden state")
        if self._dup is not None:
            raise ValueError("enable_device_hidden: the rollout is mirror-augmented (enable_dup_sym): its mirrored columns have no "
                             "hidden states of their own on the device")
        _lib.check(self.lib.sg_rollout_enable_hidden(self.h, H))
        hx = self._hidden_np()
        _lib.check(self.lib.sg_rollout_upload_hidden(self.h, _lib.fptr(hx), hx.size))
        self.bytes_uploaded += hx.nbytes
        self.device_hidden = True

    def sync_from_device(self, fields=None):
        if fields is None and self.__dict__.get("device_hidden"):
            hx = self._hidden_np()
            _lib.check(self.lib.sg_rollout_download_hidden(self.h, _lib.fptr(hx), hx.size))
        for f in (fields if fields is not None else _FIELD_ATTR):
            a = self._host_np(f)
            if a.size and a.dtype == np.int64:   # Discrete actions: the device's float32 class indices back into the int64 host tensor
                down = np.empty(a.shape, np.float32)
                _lib.check(self.lib.sg_rollout_download(self.h, f, _lib.fptr(down), down.size))
                a[...] = down
            elif a.size:
                _lib.check(self.lib.sg_rollout_download(self.h, f, _lib.fptr(a), a.size))
            self._synced[f] = self._stamp(f)   # (written through the numpy view: the version counter did not move)
            if _VERIFY:
                self._crcs[f] = self._crc(f)

    def _push(self, fields):
        if self.device_resident:
            return
        if os.environ.get("SG_ROLLOUT_ALWAYS_UPLOAD") == "1":
            return self.sync_to_device(fields)
        stale = [f for f in fields if not self._matches(f)]
        if _VERIFY:
            # SG_ROLLOUT_VERIFY=1: a field the tracker takes for unchanged is checksummed against what was uploaded -- a write that
            # did not go through torch (rollouts.x.numpy()[...] = ..., a .data view, an array shared through torch.from_numpy, C or
            # environment code filling the buffer) is then an error here instead of a silently stale device copy
            for f in fields:
                if f not in stale and f in self._crcs and self._crc(f) != self._crcs[f]:
                    raise RuntimeError(f"rollouts.{_FIELD_ATTR[f]} was written behind torch's version counter since its last upload "
                                       "(a numpy view / .data / shared buffer): call rollouts.mark_host_written() after such writes, "
                                       "or set SG_ROLLOUT_ALWAYS_UPLOAD=1")
        if stale:
            self.sync_to_device(stale)

    def _pull(self, fields):
        if not self.device_resident:
            self.sync_from_device(fields)

    def device_advantages(self):
        out = np.empty((self.num_steps, self.num_processes, 1), np.float32)
        _lib.check(self.lib.sg_rollout_download(self.h, _lib.F_ADVANTAGES, _lib.fptr(out), out.size))
        return to_host_tensor(out)

    # ------------------------------------------------------------- reference methods
    def insert(self, obs, recurrent_hidden_states, actions, action_log_probs,
               value_preds, rewards, masks, bad_masks, obs_feat=None):
        """a2c/storage.py:70-84"""
        s = self.step

        def put(dst, src):
            if torch is not None and hasattr(dst, "copy_"):
                dst.copy_(src if hasattr(src, "dim") else torch.as_tensor(np.asarray(src, np.int64 if dst.dtype == torch.int64 else np.float32)))
            else:
                dst[...] = np.asarray(src, dst.dtype)

        put(self.obs[s + 1], obs)
        if obs_feat is not None:
            put(self.obs_feat[s + 1], obs_feat)
        put(self.recurrent_hidden_states[s + 1], recurrent_hidden_states)
        put(self.actions[s], actions)
        put(self.action_log_probs[s], action_log_probs)
        put(self.value_preds[s], value_preds)
        put(self.rewards[s], rewards)
        put(self.masks[s + 1], masks)
        put(self.bad_masks[s + 1], bad_masks)
        self.step = (self.step + 1) % self.num_steps
        self._host_written = True

    # ------------------------------------------------- collection on the device (a2c/main_gail_dyn_ppo.py:209-236)
    def _on_device_only(self, who):
        if self.__dict__.get("image_shape"):
            raise NotImplementedError(f"{who}: on-device collection is not built for image observations (the CNN base): act through "
                                      "policy.act and insert()")
        if not self.device_resident:
            raise ValueError(f"{who}: the rollout is not device-resident (rollouts.device_resident = True): in drop-in mode the host "
                             "tensors are the rollout and the next device call would overwrite what the step wrote on the device")
        if self._dup is not None:
            raise ValueError(f"{who}: the rollout is mirror-augmented (enable_dup_sym): its column upload would overwrite the fields "
                             "the step writes on the device; collect through insert_dup_sym")

    def act_step(self, policy, deterministic=False, noise=None):
        """policy.act (a2c/model.py:89-101) on host slot `self.step` of obs, in one launch that also fills the policy's half of
        insert() (a2c/storage.py:70-84) on the DEVICE: value_preds[step], actions[step], action_log_probs[step].  Returns the
        [N, A] action as act() returns it and writes it into the host mirror actions[step]; the values and log-probs do not come
        back (the host mirrors of value_preds and action_log_probs are stale until sync_from_device()).  The draw is the policy's
        own stream, (policy.seed + policy._act_calls) after incrementing _act_calls, as in policy.act: a run through either path
        consumes the same draws and gets the same bits.  `noise` ([N, A] standard normal) injects the draw.  bytes_uploaded
        counts the observation slot.  Device-resident rollouts only; feed-forward policies with a Gaussian head -- and, once
        enable_device_hidden() was called, recurrent ones: Policy.act with recurrent=True (a2c/model.py:89-101, 117-201, 255-264) on
        host slots obs[step] and masks[step] (both uploaded and counted) and DEVICE hidden slot `step`, the new state written to
        hidden slot step + 1 on the device; it does not come back either."""
        self._on_device_only("act_step")
        if getattr(policy, "is_recurrent", False) and getattr(policy, "dist_kind", 0):
            raise NotImplementedError("act_step: a recurrent policy on a Discrete / MultiBinary action space acts through Policy.act and "
                                      "insert(): the one-launch recurrent step carries the Gaussian head only")
        s, N = self.step, self.num_processes
        obs = self._host_np(_lib.F_OBS)[s]
        nz = None if noise is None else _lib.as_f32(noise).reshape(N, self.act_dim)
        action = np.empty((N, self.act_dim), np.float32)
        policy._act_calls += 1
        if getattr(policy, "is_recurrent", False) and self.__dict__.get("device_hidden"):
            # recurrent policy on a rollout that holds its hidden states (enable_device_hidden): the GRU step runs in the same
            # launch on hidden slot s and masks[s], and the new state lands in hidden slot s + 1 on the device
            masks = self._host_np(_lib.F_MASKS)[s]
            _lib.check(self.lib.sg_rollout_act_step_rnn(self.h, policy.h, s, _lib.fptr(obs), _lib.fptr(masks),
                                                        None if nz is None else _lib.fptr(nz),
                                                        (policy.seed + policy._act_calls) & (2 ** 64 - 1), 1 if deterministic else 0,
                                                        _lib.fptr(action)))
            self.bytes_uploaded += obs.nbytes + masks.nbytes
            _put(self.actions[s], action)
            return to_host_tensor(action)
        _lib.check(self.lib.sg_rollout_act_step(self.h, policy.h, s, _lib.fptr(obs), None if nz is None else _lib.fptr(nz),
                                                (policy.seed + policy._act_calls) & (2 ** 64 - 1), 1 if deterministic else 0,
                                                _lib.fptr(action)))
        self.bytes_uploaded += obs.nbytes
        _put(self.actions[s], action)
        return to_host_tensor(action)

    def insert_env(self, obs, rewards, masks, bad_masks, obs_feat=None):
        """The environment's half of insert() (a2c/storage.py:70-84) after act_step(): host slots obs[s+1], obs_feat[s+1],
        rewards[s], masks[s+1], bad_masks[s+1]; advances `step`."""
        if self.__dict__.get("image_shape"):
            raise NotImplementedError("insert_env: on-device collection is not built for image observations (the CNN base): act "
                                      "through policy.act and insert()")
        s = self.step
        _put(self.obs[s + 1], obs)
        if obs_feat is not None:
            _put(self.obs_feat[s + 1], obs_feat)
        _put(self.rewards[s], rewards)
        _put(self.masks[s + 1], masks)
        _put(self.bad_masks[s + 1], bad_masks)
        self.step = (self.step + 1) % self.num_steps
        self._host_written = True   # after_update() rolls the host mirrors over as it does after insert()

    def finish_collect(self):
        """End of a collection through act_step() / insert_env(): uploads what the device does not have -- obs_feat, rewards,
        masks, bad_masks, slot T of obs (slots 0..T-1 went up step by step) -- and, so that the device rollout is float for float
        what sync_to_device() would have left, the host's returns and slot T of value_preds, which no step writes.  Slots
        0..T-1 of value_preds, actions and action_log_probs never cross the link: the device wrote them itself.  The host mirrors
        of value_preds and action_log_probs are STALE afterwards (they hold what they held before the collection) until
        sync_from_device(); actions is current."""
        self._on_device_only("finish_collect")
        T = self.num_steps
        self.sync_to_device([_lib.F_OBS_FEAT, _lib.F_REWARDS, _lib.F_RETURNS, _lib.F_MASKS, _lib.F_BAD_MASKS])
        for f in (_lib.F_OBS, _lib.F_VALUE_PREDS):
            a = self._host_np(f)[T]
            _lib.check(self.lib.sg_rollout_upload_step(self.h, f, T, _lib.fptr(a), a.size))
            self.bytes_uploaded += a.nbytes

    # ------------------------------------------------- chained act: in-environment policy and learner in one launch
    # (my_pybullet_envs/hopper_env_combined_policy.py:195-216,298-325, laikago_env_combined_policy.py:240-268,420-438)
    @property
    def chain_slot_complete(self):
        """True when the observation of slot `step` is already complete on the device and in the host mirror -- slot 0 after
        finish_collect_chain() and after_update(), which rolled the completed OBS[T] over.  Such a slot takes plain act_step():
        the in-environment policy has acted on that state already and its draw must not be taken twice."""
        return self.__dict__.get("_chain_complete") == self.step

    def _chain_inner(self, who, policy, ensemble, inner_first, inner_obs, state, ind, rng, inner_noise):
        """The checked inputs of one chained call: (inner_obs | None, state | None, ind, inner noise | None, state width)."""
        N, K = self.num_processes, len(ensemble)
        if getattr(policy, "cnn", 0) or getattr(policy, "is_recurrent", False) or getattr(policy, "dist_kind", 0):
            raise ValueError(f"{who}: the chained step takes a feed-forward learner with the MLP base and a Gaussian head (Policy / "
                             "SplitPolicy on a Box action space); a CNN base, a GRU or a Discrete / MultiBinary head acts through "
                             "PolicyEnsemble.act and act_step")
        if policy.obs_dim != self.obs_dim or policy.act_dim != self.act_dim:
            raise ValueError(f"{who}: learner/rollout dims differ (obs {policy.obs_dim} vs {self.obs_dim}, action {policy.act_dim} vs "
                             f"{self.act_dim})")
        Oi, Ai = ensemble.obs_dim, ensemble.act_dim
        Os = self.obs_dim - Ai if inner_first else Oi - self.act_dim
        if Os <= 0:
            raise ValueError(f"{who}: dims do not add up: " + (f"the learner's observation ({self.obs_dim}) must be state + member action ({Ai})"
                             if inner_first else f"the members' observation ({Oi}) must be state + learner action ({self.act_dim})"))
        if inner_first:
            if inner_obs is None and state is not None:
                inner_obs, state = state, None          # the state is what the members act on
            if inner_obs is None:
                raise ValueError(f"{who}: INNER_FIRST needs inner_obs [N, {Oi}] (or state, where the members act on the state itself)")
            inner_obs = _lib.as_f32(inner_obs).reshape(-1, Oi)
            if inner_obs.shape[0] != N:
                raise ValueError(f"{who}: inner_obs holds {inner_obs.shape[0]} rows, the rollout {N} environments")
            if state is None and Oi != Os:
                raise ValueError(f"{who}: dims do not add up: without state the members' observation ({Oi}) is the state, and state + "
                                 f"member action ({Ai}) must be the learner's observation ({self.obs_dim})")
        else:
            if inner_obs is not None:
                raise ValueError(f"{who}: LEARNER_FIRST builds the members' observation itself (cat(state, squash(action))); inner_obs is "
                                 "not taken")
            if state is None and Os != self.obs_dim:
                raise ValueError(f"{who}: dims do not add up: without state the rollout's observation ({self.obs_dim}) is the state, and "
                                 f"state + learner action ({self.act_dim}) must be the members' observation ({Oi})")
        if state is not None:
            state = _lib.as_f32(state).reshape(-1)
            if state.size != N * Os:
                raise ValueError(f"{who}: state holds {state.size} floats, not [N, Os] = [{N}, {Os}]")
            state = state.reshape(N, Os)
        if ind is None:
            ind = (rng or np.random.default_rng()).integers(0, K, size=N)
        ind = np.ascontiguousarray(ind, np.int32).reshape(-1)
        if ind.shape != (N,) or ind.min() < 0 or ind.max() >= K:
            raise ValueError(f"{who}: ind must hold N = {N} member numbers in [0, {K})")
        inz = None if inner_noise is None else _lib.as_f32(inner_noise).reshape(N, Ai)
        return inner_obs, state, ind, inz, Os

    def _chain_call(self, policy, ensemble, t, order, ind, inner_obs, state, obs, inz, inner_deterministic, nz, deterministic, squash,
                    action, inner_action, inner_raw=None):
        p = lambda a: None if a is None else _lib.fptr(a)  # noqa: E731
        _lib.check(self.lib.sg_rollout_act_step_chain(
            self.h, policy.h, t, order, ensemble._handles, len(ensemble), ind.ctypes.data_as(C.POINTER(C.c_int32)),
            p(inner_obs), p(state), p(obs), p(inz), (ensemble.seed + ensemble._calls) & (2 ** 64 - 1), 1 if inner_deterministic else 0,
            p(nz), (policy.seed + policy._act_calls) & (2 ** 64 - 1), 1 if deterministic else 0, 1 if squash else 0,
            p(action), p(inner_action), p(inner_raw)))
        self.bytes_uploaded += ind.nbytes + sum(a.nbytes for a in (inner_obs, state, obs) if a is not None)

    def act_step_chain(self, policy, ensemble, order, inner_obs=None, state=None, ind=None, rng=None, noise=None, inner_noise=None,
                       deterministic=False, inner_deterministic=False, squash=True, inner_raw_out=None):
        """ensemble.act and act_step(policy) on slot `step` as ONE launch, with the environment's seam between them -- tanh on the
        first action (squash=False: none), concatenated behind the state -- kept on the device.  Returns (action [N, A], the
        learner's raw action as act_step returns it; inner_action; ind [N], the member each row used, drawn like
        PolicyEnsemble.act draws it when not given).
          order = _lib.CHAIN_INNER_FIRST (GAIL-dyn stage): the members act on inner_obs [N, O_member]; obs[step] becomes
            cat(state, squash(a_inner)) on the device AND in the host mirror; the learner acts on it.  state [N, O - A_member];
            None: inner_obs is the state.  inner_action is the squashed member action, the one inside obs[step].
          order = _lib.CHAIN_LEARNER_FIRST (refinement stage): the learner acts on host slot obs[step] (uploaded, as in act_step);
            the members act on cat(state, squash(action)); state None: obs[step] is the state.  inner_action is the members' raw
            action, what the environment steps with.
        policy._act_calls and ensemble._calls advance, and the draws are taken, exactly as by the two separate calls: either
        path gives the same bits.  The learner's half fills value_preds[step], actions[step], action_log_probs[step] on the
        device and the host mirror of actions, like act_step.  bytes_uploaded counts ind and the arrays that went up.
        inner_raw_out (optional, a contiguous float32 [N, A_member] array): receives the members' raw action in either order."""
        self._on_device_only("act_step_chain")
        if order not in (_lib.CHAIN_INNER_FIRST, _lib.CHAIN_LEARNER_FIRST):
            raise ValueError(f"act_step_chain: unknown order {order!r} (_lib.CHAIN_INNER_FIRST / _lib.CHAIN_LEARNER_FIRST)")
        inner_first = order == _lib.CHAIN_INNER_FIRST
        s, N = self.step, self.num_processes
        if inner_first and self.chain_slot_complete:
            raise ValueError(f"act_step_chain: the observation of slot {s} is already complete (finish_collect_chain made it and "
                             "after_update rolled it over): the in-environment policy has acted on that state; take act_step()")
        inner_obs, state, ind, inz, Os = self._chain_inner("act_step_chain", policy, ensemble, inner_first, inner_obs, state, ind, rng,
                                                           inner_noise)
        nz = None if noise is None else _lib.as_f32(noise).reshape(N, self.act_dim)
        if inner_raw_out is not None and (not isinstance(inner_raw_out, np.ndarray) or inner_raw_out.shape != (N, ensemble.act_dim)):
            raise ValueError(f"act_step_chain: inner_raw_out must be a float32 numpy array of shape [{N}, {ensemble.act_dim}]")
        obs = None if inner_first else self._host_np(_lib.F_OBS)[s]
        action = np.empty((N, self.act_dim), np.float32)
        inner_action = np.empty((N, ensemble.act_dim), np.float32)
        policy._act_calls += 1
        ensemble._calls += 1
        self._chain_call(policy, ensemble, s, order, ind, inner_obs, state, obs, inz, inner_deterministic, nz, deterministic, squash,
                         action, inner_action, inner_raw_out)
        self.__dict__["_chain_policy"] = weakref.ref(policy)
        if inner_first:
            _put(self.obs[s], np.concatenate([inner_obs if state is None else state, inner_action], axis=1))
        _put(self.actions[s], action)
        return to_host_tensor(action), to_host_tensor(inner_action), ind

    def insert_env_rest(self, rewards, masks, bad_masks, obs_feat=None):
        """The environment's half of insert() (a2c/storage.py:70-84) in an INNER_FIRST collection, where the next observation is
        not known until the next chained call makes it: host slots obs_feat[s+1], rewards[s], masks[s+1], bad_masks[s+1];
        advances `step`."""
        if self.__dict__.get("image_shape"):
            raise NotImplementedError("insert_env_rest: on-device collection is not built for image observations (the CNN base)")
        s = self.step
        if obs_feat is not None:
            _put(self.obs_feat[s + 1], obs_feat)
        _put(self.rewards[s], rewards)
        _put(self.masks[s + 1], masks)
        _put(self.bad_masks[s + 1], bad_masks)
        self.step = (self.step + 1) % self.num_steps
        self._host_written = True
        self.__dict__["_chain_complete"] = None

    def finish_collect_chain(self, ensemble, inner_obs=None, state=None, policy=None, ind=None, rng=None, inner_noise=None,
                             inner_deterministic=False, squash=True):
        """End of an INNER_FIRST collection: the members act on the state the last environment step left (one chained call at
        t == T, the learner does not act) and obs[T] = cat(state, squash(a_inner)) is completed on the device and in the host
        mirror; then what finish_collect() does.  Returns (inner_action, ind): the learner keeps the inner action for the next
        envs.step, since slot 0 of the next collection -- obs[T] rolled over by after_update() -- takes plain act_step().
        policy: the learner (default: the one the last act_step_chain served)."""
        self._on_device_only("finish_collect_chain")
        if policy is None:
            ref = self.__dict__.get("_chain_policy")
            policy = ref() if ref is not None else None
            if policy is None:
                raise ValueError("finish_collect_chain: no act_step_chain call has served this rollout yet; pass policy=")
        T, N = self.num_steps, self.num_processes
        inner_obs, state, ind, inz, Os = self._chain_inner("finish_collect_chain", policy, ensemble, True, inner_obs, state, ind, rng,
                                                           inner_noise)
        inner_action = np.empty((N, ensemble.act_dim), np.float32)
        ensemble._calls += 1
        self._chain_call(policy, ensemble, T, _lib.CHAIN_INNER_FIRST, ind, inner_obs, state, None, inz, inner_deterministic, None, False,
                         squash, None, inner_action)
        _put(self.obs[T], np.concatenate([inner_obs if state is None else state, inner_action], axis=1))
        self._host_written = True
        self.finish_collect()
        self.__dict__["_chain_complete"] = T
        return to_host_tensor(inner_action), ind

    # ------------------------------------------------- mirror-augmented rollouts (a2c/main.py:171-245, --dup-sym)
    def enable_dup_sym(self, mirror_obs, mirror_act):
        """The rollout's N = 2n columns are n environments and their n mirror images: column n + j mirrors column j.
        mirror_act: [A, A] matrix or a per-row callable, which must be linear (probed into its matrix; ValueError otherwise).
        mirror_obs: [O, O] matrix (the mirrored observations are made where the rollout lives) or any per-row callable,
        applied on the host row by row in both modes, as PPO applies it for the symmetry loss.  Matrices act on rows:
        mirrored = M @ x.  Fill the rollout through set_initial_obs_dup_sym / insert_dup_sym afterwards."""
        from . import symmetry as _sym
        if self.__dict__.get("image_shape"):
            raise NotImplementedError("enable_dup_sym: a mirror-augmented rollout mirrors observations through a linear map or a "
                                      "per-row callable on 1-D rows; image observations (the CNN base) have neither here")
        if not self.__dict__.get("box_actions", True):
            raise NotImplementedError("enable_dup_sym: a mirror-augmented rollout mirrors actions through a linear map, which a class "
                                      "index or a bit vector (Discrete / MultiBinary action space) does not have; Box action spaces only")
        if self.__dict__.get("device_hidden"):
            raise ValueError("enable_dup_sym: the rollout holds its hidden states on the device (enable_device_hidden): the mirrored "
                             "columns would have none of their own there")
        N = self.num_processes
        if N % 2:
            raise ValueError(f"enable_dup_sym: the rollout has num_processes = {N}, an odd number: a mirror-augmented rollout "
                             "holds n environments and their n mirror images (num_processes = 2n)")
        if mirror_act is None:
            raise ValueError("enable_dup_sym: mirror_act is required")
        A, O = self.act_dim, self.obs_dim
        m_act = _sym.probe_linear(mirror_act, A, "mirror_act") if callable(mirror_act) else _sym.as_matrix(mirror_act, A, "mirror_act")
        if callable(mirror_obs):
            obs_fn, m_obs = mirror_obs, None
        else:
            obs_fn, m_obs = None, _sym.as_matrix(mirror_obs, O, "mirror_obs")
        _lib.check(self.lib.sg_rollout_set_mirrors(self.h, None if m_obs is None else _lib.fptr(m_obs), _lib.fptr(m_act)))
        self._dup = {"n": N // 2, "m_obs": m_obs, "m_act": m_act, "obs_fn": obs_fn}

    @property
    def dup_sym(self):
        """True once enable_dup_sym made the rollout mirror-augmented."""
        return self._dup is not None

    def _dup_state(self, who):
        if self._dup is None:
            raise RuntimeError(f"{who}: the rollout is not mirror-augmented: call enable_dup_sym(mirror_obs, mirror_act) first")
        return self._dup

    def _dup_rows(self, x, width, who, what):
        a = _lib.as_f32(x).reshape(-1, width) if width else np.zeros((self._dup["n"], 0), np.float32)
        if a.shape[0] != self._dup["n"]:
            raise ValueError(f"{who}: {what} must hold n = {self._dup['n']} rows (one per environment), got {a.shape[0]}")
        return a

    def _dup_mirror_obs(self, rows):
        from . import symmetry as _sym
        d = self._dup
        return _sym.mirror_rows(d["obs_fn"], rows) if d["obs_fn"] is not None else _sym.matrix_rows(d["m_obs"], rows)

    def _dup_put(self, dst, rows, mirrored=None, both=False):
        """rows -> columns [0, n) of the slot `dst`; columns [n, 2n) get `mirrored` (default: the rows again) in host mode,
        or when `both` is set; on a device-resident rollout they are left to sg_rollout_dup_sym."""
        n = self._dup["n"]
        full = both or not self.device_resident
        src = np.concatenate([rows, rows if mirrored is None else mirrored]) if full else rows
        tgt = dst if full else dst[:n]
        if torch is not None and hasattr(tgt, "copy_"):
            tgt.copy_(torch.as_tensor(np.ascontiguousarray(src)).reshape(tgt.shape))
        else:
            tgt[...] = src.reshape(tgt.shape)

    def set_initial_obs_dup_sym(self, obs, obs_feat=None):
        """a2c/main.py:181-185: obs[0] = cat(obs, mirror_obs(obs)), obs_feat[0] = obs_feat repeated; obs / obs_feat hold n rows."""
        d = self._dup_state("set_initial_obs_dup_sym")
        rows = self._dup_rows(obs, self.obs_dim, "set_initial_obs_dup_sym", "obs")
        host_obs = d["obs_fn"] is not None     # a callable mirror: OBS is mirrored here and crosses the link full-width
        self._dup_put(self.obs[0], rows, self._dup_mirror_obs(rows) if (host_obs or not self.device_resident) else None, both=host_obs)
        if obs_feat is not None:
            self._dup_put(self.obs_feat[0], self._dup_rows(obs_feat, self.feat_len, "set_initial_obs_dup_sym", "obs_feat"))
        self._host_written = True

    def insert_dup_sym(self, obs, recurrent_hidden_states, actions, action_log_probs,
                       value_preds, rewards, masks, bad_masks, obs_feat=None):
        """a2c/main.py:231-242: insert()'s arguments with n rows each; observations and actions are mirrored into columns
        [n, 2n), everything else (obs_feat included) is repeated.  Host (drop-in) mode writes both halves of the host tensors, the
        mirrored half in the device kernel's arithmetic (symmetry.matrix_rows).  On a device-resident rollout only columns
        [0, n) are written -- recurrent_hidden_states, which has no device twin, in both halves -- and sync_to_device() sends
        those columns and has the device make the rest."""
        from . import symmetry as _sym
        d = self._dup_state("insert_dup_sym")
        who, s = "insert_dup_sym", self.step
        resident, host_obs = self.device_resident, d["obs_fn"] is not None
        rows = self._dup_rows(obs, self.obs_dim, who, "obs")
        self._dup_put(self.obs[s + 1], rows, self._dup_mirror_obs(rows) if (host_obs or not resident) else None, both=host_obs)
        if obs_feat is not None:
            self._dup_put(self.obs_feat[s + 1], self._dup_rows(obs_feat, self.feat_len, who, "obs_feat"))
        hx = self.recurrent_hidden_states
        self._dup_put(hx[s + 1], self._dup_rows(recurrent_hidden_states, hx.shape[-1], who, "recurrent_hidden_states"), both=True)
        act = self._dup_rows(actions, self.act_dim, who, "actions")
        self._dup_put(self.actions[s], act, None if resident else _sym.matrix_rows(d["m_act"], act))
        self._dup_put(self.action_log_probs[s], self._dup_rows(action_log_probs, 1, who, "action_log_probs"))
        self._dup_put(self.value_preds[s], self._dup_rows(value_preds, 1, who, "value_preds"))
        self._dup_put(self.rewards[s], self._dup_rows(rewards, 1, who, "rewards"))
        self._dup_put(self.masks[s + 1], self._dup_rows(masks, 1, who, "masks"))
        self._dup_put(self.bad_masks[s + 1], self._dup_rows(bad_masks, 1, who, "bad_masks"))
        self.step = (self.step + 1) % self.num_steps
        self._host_written = True

    def _sync_to_device_dup_sym(self, fields=None):
        """sync_to_device() of a device-resident mirror-augmented rollout: columns [0, n) of every field cross the link (OBS
        full-width when mirror_obs is a callable), then one launch makes columns [n, 2n) on the device."""
        d = self._dup
        for f in (fields if fields is not None else _FIELD_ATTR):
            a = self._host_np(f)
            if a.size:
                if f == _lib.F_OBS and d["obs_fn"] is not None:
                    _lib.check(self.lib.sg_rollout_upload(self.h, f, _lib.fptr(a), a.size))
                    self.bytes_uploaded += a.nbytes
                else:
                    _lib.check(self.lib.sg_rollout_upload_columns(self.h, f, d["n"], _lib.fptr(a), a.size))
                    self.bytes_uploaded += a.nbytes // 2
            self._synced[f] = self._stamp(f)
        _lib.check(self.lib.sg_rollout_dup_sym(self.h))

    def mod_reward(self, offset, reverse_l):
        """a2c/storage.py:86-94 (called by no shipped script): add the per-environment `offset` [N] to the rewards of the
        `reverse_l` most recently inserted steps, walking back from the insert cursor with wrap-around.  Host tensors; the
        write is seen by the next device call like any other in-place edit."""
        off = offset.reshape(-1, 1) if hasattr(offset, "reshape") else np.asarray(offset, np.float32).reshape(-1, 1)
        assert off.shape[0] == self.rewards.shape[1], (off.shape, self.rewards.shape)
        for back in range(1, int(reverse_l) + 1):
            self.rewards[(self.step - back) % self.num_steps] += off

    def after_update(self):
        """a2c/storage.py:96-101"""
        # a slot T completed by finish_collect_chain() becomes the complete slot 0 of the next collection
        self.__dict__["_chain_complete"] = 0 if self.__dict__.get("_chain_complete") == self.num_steps else None
        if self.device_resident:   # the device copy is the rollout; the host mirrors are refreshed by sync_from_device()
            _lib.check(self.lib.sg_rollout_after_update(self.h))
            if not self._host_written:
                return
            # a host-side collector (driver.collect) filled this rollout through insert(): its next act() reads host
            # slot 0 and its next sync_to_device() uploads it, so the host mirrors must roll over as well
        for name in ("obs", "obs_feat", "recurrent_hidden_states", "masks", "bad_masks"):
            t = getattr(self, name)
            t[0] = t[-1]
        self._host_written = False

    def compute_returns(self, next_value, use_gae, gamma, gae_lambda, use_proper_time_limits=True):
        """a2c/storage.py:103-142, on device (one thread per env column, reverse scan over T)."""
        self._push([_lib.F_REWARDS, _lib.F_VALUE_PREDS, _lib.F_RETURNS, _lib.F_MASKS, _lib.F_BAD_MASKS])
        nv = _lib.as_f32(next_value).reshape(-1)
        assert nv.size == self.num_processes
        _lib.check(self.lib.sg_rollout_compute_returns(self.h, _lib.fptr(nv), 1 if use_gae else 0,
                                                       float(gamma), float(gae_lambda),
                                                       1 if use_proper_time_limits else 0))
        self._pull([_lib.F_RETURNS, _lib.F_VALUE_PREDS])

    def feed_forward_generator(self, advantages, num_mini_batch=None, mini_batch_size=None, perm=None):
        """a2c/storage.py:144-192 -- host-side generator kept for API completeness (the device PPO / discriminator
        updates gather rows themselves and do not use it).  `perm` injects the sampler's permutation of the T*N row ids
        (the reference draws torch.randperm through SubsetRandomSampler, a2c/storage.py:159-162); default: numpy's
        global generator."""
        return feed_forward_batches(self, advantages, num_mini_batch, mini_batch_size, perm)

    def recurrent_generator(self, advantages, num_mini_batch, perm=None):
        """a2c/storage.py:194-251 -- host-side generator: whole environments per minibatch, rows time-major, the hidden
        state of slot 0.  `perm` injects the reference's torch.randperm(num_processes) draw; default: numpy's generator."""
        # (an image rollout built with recurrent_hidden_state_size > 1 serves the recurrent CNN base: frames come out 4-D, [T * per, C, H, W])
        if self.__dict__.get("image_shape") and int(self.recurrent_hidden_states.shape[-1]) <= 1:
            raise NotImplementedError("recurrent_generator: image observations are read by the feed-forward CNN base only (a recurrent "
                                      "CNN base is not built): use feed_forward_generator")
        return recurrent_batches(self, advantages, num_mini_batch, perm)


def recurrent_batches(ro, advantages, num_mini_batch, perm=None):
    """a2c/storage.py:194-251 on any object carrying the rollout's host buffers (needs no device): minibatch k holds the
    environments perm[k*per : (k+1)*per], per = N // num_mini_batch, all T steps each, stacked time-major (row t*per + j);
    the hidden state is the one of slot 0 only ([per, H]).  The reference's loop is range(0, N, per): N // per minibatches
    (more than num_mini_batch when per does not divide N into exactly that many), and it dies with an IndexError when
    N % per != 0 -- a ValueError here."""
    num_steps, num_processes = ro.rewards.shape[0:2]
    assert num_processes >= num_mini_batch, (
        "PPO requires the number of processes ({}) "
        "to be greater than or equal to the number of "
        "PPO mini batches ({}).".format(num_processes, num_mini_batch))
    per = num_processes // num_mini_batch
    if num_processes % per:
        raise ValueError(f"recurrent_generator: {num_processes} processes do not split into minibatches of "
                         f"{per} = {num_processes} // {num_mini_batch} environments (the reference indexes past its permutation here)")
    if perm is None:
        perm = np.random.permutation(num_processes)
    else:
        perm = _lib.as_i64(perm).reshape(-1)
        assert perm.size == num_processes and np.array_equal(np.sort(perm), np.arange(num_processes)), \
            "perm must be a permutation of the N environment ids"

    def arr(t):
        return t.numpy() if hasattr(t, "numpy") else t

    for start in range(0, num_processes, per):
        envs = perm[start:start + per]

        def g(t, sl):   # [T(+1), N, w] -> the minibatch's [T * per, w], time-major
            a = arr(t)[sl][:, envs]
            if a.ndim == 5:   # image observations [T, per, C, H, W] -> [T * per, C, H, W] (a2c/storage.py:236-238: _flatten_helper)
                return to_host_tensor(np.ascontiguousarray(a.reshape(-1, *a.shape[2:])))
            return to_host_tensor(np.ascontiguousarray(a.reshape(-1, a.shape[-1])))

        cur, al = slice(None, -1), slice(None)
        adv = None if advantages is None else to_host_tensor(np.ascontiguousarray(
            _lib.as_f32(advantages).reshape(num_steps, num_processes, 1)[:, envs].reshape(-1, 1)))
        hxs = to_host_tensor(np.ascontiguousarray(arr(ro.recurrent_hidden_states)[0, envs]))
        # (the reference's recurrent generator yields 8 fields: no obs_feat pair, a2c/storage.py:249-251)
        yield (g(ro.obs, cur), hxs, g(ro.actions, al), g(ro.value_preds, cur), g(ro.returns, cur), g(ro.masks, cur),
               g(ro.action_log_probs, al), adv)


def feed_forward_batches(ro, advantages, num_mini_batch=None, mini_batch_size=None, perm=None):
    """The generator body on any object carrying the rollout's host buffers (needs no device): yields the reference's
    10-tuple (obs, hxs, actions, value_preds, returns, masks, old_logp, adv | None, obs_feat, next_obs_feat) per minibatch,
    rows in flattened (t, n) order t*N+n, "cur" fields from slots [:-1], next_obs_feat from obs_feat[1:], the ragged tail
    dropped (BatchSampler(drop_last=True))."""
    num_steps, num_processes = ro.rewards.shape[0:2]
    batch_size = num_processes * num_steps
    if mini_batch_size is None:
        assert batch_size >= num_mini_batch, (
            "PPO requires the number of processes ({}) "
            "* number of steps ({}) = {} "
            "to be greater than or equal to the number of PPO mini batches ({})."
            "".format(num_processes, num_steps, num_processes * num_steps, num_mini_batch))
        mini_batch_size = batch_size // num_mini_batch
    if perm is None:
        perm = np.random.permutation(batch_size)
    else:
        perm = _lib.as_i64(perm).reshape(-1)
        assert perm.size == batch_size and np.array_equal(np.sort(perm), np.arange(batch_size)), "perm must be a permutation of the T*N row ids"

    def flat(t, sl):
        a = t.numpy() if hasattr(t, "numpy") else t
        a = a[sl]
        if a.ndim == 5:   # image observations [T, N, C, H, W] -> obs_batch [-1, C, H, W] (a2c/storage.py:165)
            return a.reshape(-1, *a.shape[2:])
        return a.reshape(-1, a.shape[-1])

    cur, nxt, al = slice(None, -1), slice(1, None), slice(None)
    for k in range(batch_size // mini_batch_size):  # drop_last
        idx = perm[k * mini_batch_size:(k + 1) * mini_batch_size]
        g = lambda t, sl: to_host_tensor(np.ascontiguousarray(flat(t, sl)[idx]))  # noqa: E731
        adv = None if advantages is None else to_host_tensor(
            np.ascontiguousarray(_lib.as_f32(advantages).reshape(-1, 1)[idx]))
        yield (g(ro.obs, cur), g(ro.recurrent_hidden_states, cur), g(ro.actions, al),
               g(ro.value_preds, cur), g(ro.returns, cur), g(ro.masks, cur),
               g(ro.action_log_probs, al), adv, g(ro.obs_feat, cur), g(ro.obs_feat, nxt))
