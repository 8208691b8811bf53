"""Policy -- host mirror of a2c/model.py:37-114 (image observations [C, 84, 84]: CNNBase, a2c/model.py:204-230, with the Categorical or Gaussian head; else MLPBase + DiagGaussian on Box actions, Categorical on Discrete, Bernoulli on
MultiBinary, a2c/model.py:52-62; feed-forward, or recurrent with the GRU base of a2c/model.py:117-201 -- on Discrete / MultiBinary
with recurrent_heads=True or SG_RECURRENT_HEADS=1).  Parameters live in HBM inside libsimgan_hip.so; this class keeps the
reference's constructor and method signatures and hands host tensors across the C ABI."""
import ctypes as C

import numpy as np

from . import _lib
from .utils import derive_seed, orthogonal, to_host_tensor


# Context for policies that build their device twin lazily (a bare torch.load of a reference checkpoint): None = the
# process default (`Context.default()`, which `ctx.make_default()` re-points).  A process that holds several contexts
# (loopback ranks on threads) assigns `simgan_amd.model.MATERIALISE_CTX = ctx` around its torch.load, or uses
# `checkpoint.load_policy(path, ctx=ctx)`, which builds the policy on `ctx` directly and never comes through here.
MATERIALISE_CTX = None

CNN_HW = 84   # the CNN base's image size: the reference hard-codes Linear(32 * 7 * 7, hidden) behind its convolutions (a2c/model.py:216)


class _PolicyBase(object):
    KIND = None

    def _create(self, obs_dim, act_dim, hidden, num_feet, ctx, critic_hidden=None, recurrent=False, dist=0, n_out=None, cnn=None):
        # cnn: None, or the channel count C of [C, 84, 84] image observations -- the CNN base (a2c/model.py:204-230); obs_dim is
        # then the flat row width C * 84 * 84
        self.__dict__["cnn"] = int(cnn) if cnn else 0
        # dist_kind: _lib.DIST_GAUSSIAN (Box), DIST_CATEGORICAL (Discrete(n_out): act_dim 1, the class index) or DIST_BERNOULLI
        # (MultiBinary(n_out): act_dim n_out); n_out: the head's outputs
        self.__dict__["_dist_kind"] = int(dist or 0)
        self.__dict__["n_out"] = int(n_out) if self.__dict__["_dist_kind"] else int(act_dim)
        self.__dict__["recurrent"] = bool(recurrent)   # GRU base (a2c/model.py:117-131): the device kind is POLICY_GRU, the class stays Policy
        self.ctx = ctx or _lib.Context.default()
        self.lib = self.ctx.lib
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.hidden_size, self.num_feet = int(hidden), int(num_feet)
        # width of the critic trunk: the actors' unless reset_critic rebuilt it (a2c/model.py:80-87: always 64 units)
        self.critic_hidden = int(critic_hidden) if critic_hidden else self.hidden_size
        h = _lib.H()
        ch = 0 if self.critic_hidden == self.hidden_size else self.critic_hidden
        if self.cnn and self._rec():   # the recurrent CNN base (a2c/model.py:204-230 with recurrent=True): an entry point of its own
            _lib.check(self.lib.sg_policy_create_cnn_rnn(self.ctx.h, self.cnn, CNN_HW, CNN_HW, self.hidden_size, self.dist_kind, self.act_dim,
                                                         self.n_out, C.byref(h)))
        elif self.cnn:
            _lib.check(self.lib.sg_policy_create_cnn(self.ctx.h, self.cnn, CNN_HW, CNN_HW, self.hidden_size, self.dist_kind, self.act_dim,
                                                     self.n_out, C.byref(h)))
        elif self.dist_kind and self._rec():   # the GRU base with a Categorical / Bernoulli head: an entry point of its own
            _lib.check(self.lib.sg_policy_create_rnn_dist(self.ctx.h, self.obs_dim, self.hidden_size, ch, self.dist_kind, self.n_out, C.byref(h)))
        elif self.dist_kind:
            _lib.check(self.lib.sg_policy_create3(self.ctx.h, self.KIND, self.obs_dim, self.act_dim, self.hidden_size, self.num_feet, ch,
                                                  self.dist_kind, self.n_out, C.byref(h)))
        else:
            _lib.check(self.lib.sg_policy_create2(self.ctx.h, _lib.POLICY_GRU if self._rec() else self.KIND, self.obs_dim, self.act_dim, self.hidden_size, self.num_feet,
                                                  ch, C.byref(h)))
        self.h = h
        n = C.c_int64(0)
        _lib.check(self.lib.sg_policy_num_params(self.h, C.byref(n)))
        self.num_params = n.value
        self.seed = derive_seed(0, 0x5EED, per_instance=True)   # action-noise stream; re-derived from the constructor seed below
        self._act_calls = 0

    def _rec(self):
        """True for the GRU base.  Objects assembled without the constructor (a torch.load still pending, a bare instance that
        only lends its class's layout) count as feed-forward until their device twin says otherwise."""
        if "recurrent" not in self.__dict__ and self.__dict__.get("_pending") is not None:
            self._materialise()
        return self.__dict__.get("recurrent", False)

    @property
    def dist_kind(self):
        """_lib.DIST_GAUSSIAN / DIST_CATEGORICAL / DIST_BERNOULLI.  Like _rec(): an object still pending materialises first, one
        assembled without the constructor counts as Gaussian."""
        if "_dist_kind" not in self.__dict__ and self.__dict__.get("_pending") is not None:
            self._materialise()
        return self.__dict__.get("_dist_kind", 0)

    def _register_handle_user(self, obj):
        """Objects that keep this policy's device handle (PPO, PolicyEnsemble) announce themselves: reset_critic refuses to
        replace the handle while one of them is alive."""
        import weakref
        self.__dict__.setdefault("_handle_users", []).append(weakref.ref(obj))

    def __del__(self):
        try:
            h = self.__dict__.get("h")
            if h:
                self.__dict__["lib"].sg_policy_destroy(h)
                self.__dict__["h"] = None
        except Exception:
            pass

    def __getattr__(self, name):
        # Only reached for attributes that are not set: an object torch.load is still assembling (see __setstate__)
        # builds its device twin on first use.
        if not name.startswith("__") and self.__dict__.get("_pending") is not None:
            self._materialise()
            return getattr(self, name)
        raise AttributeError(name)

    def _materialise(self):
        from .checkpoint import policy_from_module_state
        st = self.__dict__.pop("_pending")
        try:
            dims, sd = policy_from_module_state(type(self).__name__, st)
            # the context an unpickled policy lands on: `simgan_amd.model.MATERIALISE_CTX` when the caller set one,
            # the process default otherwise (see the module-level comment)
            self._create(dims["obs_dim"], dims["act_dim"], dims["hidden"], dims["num_feet"], MATERIALISE_CTX,
                         critic_hidden=dims.get("critic_hidden"), recurrent=dims.get("recurrent", False),
                         dist=dims.get("dist", 0), n_out=dims.get("n_out"), cnn=dims.get("cnn"))
            self.seed = derive_seed(0, 0x5EED, per_instance=True)
            self.load_state_dict(sd)
        except BaseException:
            # keep the pickled state: the next attribute access retries (and raises the real cause again) instead of a
            # bare AttributeError with the state lost
            for k in ("h", "ctx", "lib"):
                self.__dict__.pop(k, None)
            self.__dict__["_pending"] = st
            raise

    # ---- nn.Module-ish surface the reference mains touch
    @property
    def is_recurrent(self):
        return self._rec()

    @property
    def recurrent_hidden_state_size(self):
        """Size of rnn_hx."""
        return self.hidden_size if self._rec() else 1

    def to(self, device):
        return self

    def train(self, mode=True):
        return self

    def eval(self):
        return self

    def parameters(self):
        """One flat host tensor (a copy): enough for `next(p.parameters())`-style probes."""
        yield to_host_tensor(self.get_flat_params())

    def forward(self, inputs, rnn_hxs, masks):
        raise NotImplementedError

    # ---- flat parameter access (torch state_dict order, see oracle/sg_oracle.c header)
    def get_flat_params(self):
        out = np.empty(self.num_params, np.float32)
        _lib.check(self.lib.sg_policy_get_params(self.h, _lib.fptr(out), out.size))
        return out

    def set_flat_params(self, flat):
        flat = _lib.as_f32(flat).reshape(-1)
        _lib.check(self.lib.sg_policy_set_params(self.h, _lib.fptr(flat), flat.size))

    def state_dict(self):
        flat, out, off = self.get_flat_params(), {}, 0
        for name, shape in self.param_shapes():
            n = int(np.prod(shape))
            out[name] = to_host_tensor(flat[off:off + n].reshape(shape).copy())
            off += n
        return out

    def load_state_dict(self, sd):
        parts = []
        for name, shape in self.param_shapes():
            a = _lib.as_f32(sd[name])
            assert tuple(a.shape) == tuple(shape), (name, a.shape, shape)
            parts.append(a.reshape(-1))
        self.set_flat_params(np.concatenate(parts))

    def __getstate__(self):
        return {"obs_dim": self.obs_dim, "act_dim": self.act_dim, "hidden": self.hidden_size,
                "num_feet": self.num_feet, "critic_hidden": self.critic_hidden, "recurrent": self._rec(),
                "dist": self.dist_kind, "n_out": self.n_out, "cnn": self.__dict__.get("cnn", 0), "flat": self.get_flat_params()}

    def __reduce_ex__(self, protocol):
        """A policy built through the reference's import path (`third_party.a2c_ppo_acktr.model[_split]`, i.e. by the
        unchanged mains) pickles in the REFERENCE's object layout: what their `torch.save([actor_critic, ob_rms], path)`
        writes is then a file the reference itself loads -- on the CPU, without this package (the stage-2 environment
        workers do, my_pybullet_envs/utils.py:24-57).  Loading it here goes through `__setstate__`'s "_modules" branch like
        any reference checkpoint.  The package's own classes keep their compact native pickle."""
        if type(self).__module__.startswith("third_party."):
            if self.__dict__.get("cnn"):   # (the recurrent CNN base too)
                from .checkpoint import CNN_SAVE_MSG
                raise NotImplementedError(CNN_SAVE_MSG)
            if self._rec():
                from .checkpoint import RECURRENT_SAVE_MSG
                raise NotImplementedError(RECURRENT_SAVE_MSG)
            import copyreg
            from .checkpoint import reference_module_state
            kind = {_lib.DIST_CATEGORICAL: "mlp_categorical", _lib.DIST_BERNOULLI: "mlp_bernoulli"}.get(self.dist_kind, "mlp")
            return (copyreg.__newobj__, (type(self),), reference_module_state(kind if self.KIND == _lib.POLICY_MLP else "split", self.state_dict()))
        return object.__reduce_ex__(self, protocol)

    def __setstate__(self, st):
        if "_modules" in st:   # a reference whole-module pickle (a2c/main.py:81-83) resolved to this class by the alias modules.
            # torch's legacy container fills the tensors' storages only AFTER the whole object graph is unpickled, so the
            # weights are read when the policy is first used, not here.
            self.__dict__["_pending"] = st
            return
        self._create(st["obs_dim"], st["act_dim"], st["hidden"], st["num_feet"], None, critic_hidden=st.get("critic_hidden"),
                     recurrent=st.get("recurrent", False), dist=st.get("dist", 0), n_out=st.get("n_out"), cnn=st.get("cnn"))
        self.seed = derive_seed(0, 0x5EED, per_instance=True)
        self.set_flat_params(st["flat"])

    def _rnn_inputs(self, rnn_hxs, masks, n_env, n_rows):
        if rnn_hxs is None or masks is None:
            raise ValueError("a recurrent policy needs rnn_hxs [n, hidden_size] and masks [rows, 1]")
        hxs = _lib.as_f32(rnn_hxs).reshape(-1, self.hidden_size)
        m = _lib.as_f32(masks).reshape(-1)
        if hxs.shape[0] != n_env or m.size != n_rows:
            raise ValueError(f"recurrent policy: rnn_hxs {tuple(hxs.shape)} / masks [{m.size}] do not match {n_env} states and {n_rows} rows")
        return hxs, m

    # ---- the three calls on the hot path
    def act(self, inputs, rnn_hxs, masks, deterministic=False, noise=None):
        """a2c/model.py:89-101 -> (value [n,1], action [n,A], action_log_probs [n,1], rnn_hxs).
        `noise` ([n,A] standard normal) injects the sampling draw; default = library RNG.
        Discrete: action is int64 [n,1] and `noise` [n,1] UNIFORM draws in [0,1) (inverse CDF over ascending class index);
        MultiBinary: action is float32 0/1 [n,n_bits] and `noise` [n,n_bits] uniform draws (bit = u < p)."""
        obs = _lib.as_f32(inputs).reshape(-1, self.obs_dim)
        n = obs.shape[0]
        value = np.empty((n, 1), np.float32)
        action = np.empty((n, self.act_dim), np.float32)
        logp = np.empty((n, 1), np.float32)
        nz = None if noise is None else _lib.as_f32(noise).reshape(n, self.act_dim)
        self._act_calls += 1
        if self._rec():
            hxs, m = self._rnn_inputs(rnn_hxs, masks, n, n)
            hxs_out = np.empty_like(hxs)
            _lib.check(self.lib.sg_policy_act_rnn(self.h, _lib.fptr(obs), _lib.fptr(hxs), _lib.fptr(m), n,
                                                  None if nz is None else _lib.fptr(nz), (self.seed + self._act_calls) & (2 ** 64 - 1),
                                                  1 if deterministic else 0, _lib.fptr(value), _lib.fptr(action), _lib.fptr(logp),
                                                  _lib.fptr(hxs_out)))
            if self.dist_kind == _lib.DIST_CATEGORICAL:   # the class index crossed the ABI as a float
                action = action.astype(np.int64)
            return to_host_tensor(value), to_host_tensor(action), to_host_tensor(logp), to_host_tensor(hxs_out)
        _lib.check(self.lib.sg_policy_act(self.h, _lib.fptr(obs), n,
                                          None if nz is None else _lib.fptr(nz), (self.seed + self._act_calls) & (2 ** 64 - 1),
                                          1 if deterministic else 0, _lib.fptr(value),
                                          _lib.fptr(action), _lib.fptr(logp)))
        if self.dist_kind == _lib.DIST_CATEGORICAL:   # the class index crossed the ABI as a float
            action = action.astype(np.int64)
        return to_host_tensor(value), to_host_tensor(action), to_host_tensor(logp), rnn_hxs

    def get_value(self, inputs, rnn_hxs, masks):
        """a2c/model.py:103-105"""
        obs = _lib.as_f32(inputs).reshape(-1, self.obs_dim)
        value = np.empty((obs.shape[0], 1), np.float32)
        if self._rec():
            hxs, m = self._rnn_inputs(rnn_hxs, masks, obs.shape[0], obs.shape[0])
            _lib.check(self.lib.sg_policy_get_value_rnn(self.h, _lib.fptr(obs), _lib.fptr(hxs), _lib.fptr(m), obs.shape[0], _lib.fptr(value)))
            return to_host_tensor(value)
        _lib.check(self.lib.sg_policy_get_value(self.h, _lib.fptr(obs), obs.shape[0], _lib.fptr(value)))
        return to_host_tensor(value)

    def evaluate_actions(self, inputs, rnn_hxs, masks, action):
        """a2c/model.py:107-114 -> (value, action_log_probs, dist_entropy, rnn_hxs)"""
        obs = _lib.as_f32(inputs).reshape(-1, self.obs_dim)
        n = obs.shape[0]
        act = _lib.as_f32(action).reshape(n, self.act_dim)
        value = np.empty((n, 1), np.float32)
        logp = np.empty((n, 1), np.float32)
        ent = C.c_float(0)
        if self._rec():
            # a2c/model.py:137-199: rnn_hxs [n_env, H] with inputs [T * n_env, O] flattened time-major (T == 1: one step)
            n_env = _lib.as_f32(rnn_hxs).reshape(-1, self.hidden_size).shape[0]
            if n_env == 0 or n % n_env:
                raise ValueError(f"evaluate_actions: {n} input rows are not a whole number of steps of the {n_env} hidden states")
            hxs, m = self._rnn_inputs(rnn_hxs, masks, n_env, n)
            hxs_out = np.empty_like(hxs)
            _lib.check(self.lib.sg_policy_evaluate_rnn(self.h, _lib.fptr(obs), _lib.fptr(hxs), _lib.fptr(m), _lib.fptr(act), n // n_env, n_env,
                                                       _lib.fptr(value), _lib.fptr(logp), C.byref(ent), _lib.fptr(hxs_out)))
            return to_host_tensor(value), to_host_tensor(logp), to_host_tensor(np.array(ent.value, np.float32)), to_host_tensor(hxs_out)
        _lib.check(self.lib.sg_policy_evaluate(self.h, _lib.fptr(obs), _lib.fptr(act), n,
                                               _lib.fptr(value), _lib.fptr(logp), C.byref(ent)))
        ent_t = to_host_tensor(np.array(ent.value, np.float32))
        return to_host_tensor(value), to_host_tensor(logp), ent_t, rnn_hxs


class Policy(_PolicyBase):
    KIND = _lib.POLICY_MLP

    def __init__(self, obs_shape, action_space, base=None, base_kwargs=None, ctx=None, seed=0, critic_hidden=None, recurrent_heads=None,
                 recurrent_cnn=None):
        # recurrent_cnn: the CNN base with base_kwargs['recurrent'] (CNN + GRU, a2c/model.py:204-230 with recurrent=True) is opt-in the
        # same way: True here, or SG_RECURRENT_CNN=1 in the environment when the policy is constructed; with neither it is refused as before
        if recurrent_cnn is None:
            import os
            recurrent_cnn = os.environ.get("SG_RECURRENT_CNN", "") == "1"
        # recurrent_heads: the GRU base with a Categorical / Bernoulli head (Discrete / MultiBinary with base_kwargs['recurrent']) is
        # opt-in: True here, or SG_RECURRENT_HEADS=1 in the environment when the policy is constructed (for an unchanged reference
        # main); with neither the pair is refused as before
        if recurrent_heads is None:
            import os
            recurrent_heads = os.environ.get("SG_RECURRENT_HEADS", "") == "1"
        if base_kwargs is None:
            base_kwargs = {}
        if base is not None or len(obs_shape) not in (1, 3):
            raise NotImplementedError("only the MLP base on 1-D observations is built (SURVEY.md section 2, row 3)")
        cnn = len(obs_shape) == 3   # a2c/model.py:42-46: CNNBase for image observations
        if cnn and (int(obs_shape[1]) != CNN_HW or int(obs_shape[2]) != CNN_HW):
            raise ValueError(f"Policy on image observations {tuple(obs_shape)}: the CNN base takes [C, {CNN_HW}, {CNN_HW}] only (the "
                             "reference hard-codes Linear(32 * 7 * 7, hidden) behind its three convolutions, a2c/model.py:216)")
        if cnn and int(obs_shape[0]) < 1:
            raise ValueError(f"Policy on image observations {tuple(obs_shape)}: need at least one channel")
        if cnn and base_kwargs.get("recurrent", False) and not recurrent_cnn:
            raise NotImplementedError("Policy on image observations with base_kwargs={'recurrent': True}: the CNN base is built "
                                      "feed-forward only (a recurrent CNN base is not)")
        # a2c/model.py:52-62
        space = action_space.__class__.__name__
        if space == "Box":
            dist, act_dim, n_out = _lib.DIST_GAUSSIAN, action_space.shape[0], None
        elif space == "Discrete":
            dist, act_dim, n_out = _lib.DIST_CATEGORICAL, 1, int(action_space.n)
            if not 0 < n_out < 2 ** 24:
                raise ValueError(f"Discrete({n_out}): the class index crosses the C ABI as a float32, exact below 2^24 only")
        elif space == "MultiBinary":
            n_out = int(action_space.shape[0])
            dist, act_dim = _lib.DIST_BERNOULLI, n_out
        else:
            raise NotImplementedError(f"action space {space}: Box, Discrete and MultiBinary are built (a2c/model.py:52-62)")
        if cnn and dist == _lib.DIST_BERNOULLI:
            raise NotImplementedError("Policy on image observations with a MultiBinary action space: the CNN base is built with the "
                                      "Categorical (Discrete) and Gaussian (Box) heads only")
        if not cnn and dist != _lib.DIST_GAUSSIAN and base_kwargs.get("recurrent", False) and not recurrent_heads:
            raise NotImplementedError(f"Policy on a {space} action space with base_kwargs={{'recurrent': True}}: the GRU base is built "
                                      "with the Gaussian head (Box actions) only")
        hidden = base_kwargs.get("hidden_size", 512 if cnn else 64)   # a2c/model.py:205,234
        if cnn:
            if critic_hidden not in (None, hidden):
                raise NotImplementedError("Policy on image observations: critic_linear reads the shared features (a2c/model.py:220-230); "
                                          "there is no critic trunk to give a width of its own")
            self._create(int(obs_shape[0]) * CNN_HW * CNN_HW, act_dim, hidden, 1, ctx, recurrent=bool(base_kwargs.get("recurrent", False)),
                         dist=dist, n_out=n_out, cnn=int(obs_shape[0]))
        else:
            self._create(obs_shape[0], act_dim, hidden, 1, ctx, critic_hidden=critic_hidden,
                         recurrent=base_kwargs.get("recurrent", False), dist=dist, n_out=n_out)
        self.seed = derive_seed(seed, 0x5EED, per_instance=True)
        self._init_params(np.random.default_rng(seed))

    def param_shapes(self):
        O, A, Hh, Hc = self.obs_dim, self.act_dim, self.hidden_size, self.critic_hidden
        if getattr(self, "cnn", 0):   # a2c/model.py:211-220: main = Conv, ReLU, Conv, ReLU, Conv, ReLU, Flatten, Linear, ReLU
            head = ([("dist.linear.weight", (self.n_out, Hh)), ("dist.linear.bias", (self.n_out,))] if self.dist_kind else
                    [("dist.fc_mean.weight", (A, Hh)), ("dist.fc_mean.bias", (A,)), ("dist.logstd._bias", (A, 1))])
            # recurrent=True: NNBase.__init__ creates nn.GRU(Hs, Hs) before `main` (a2c/model.py:124-131,208-216), so its tensors come first
            gru = ([("base.gru.weight_ih_l0", (3 * Hh, Hh)), ("base.gru.weight_hh_l0", (3 * Hh, Hh)),
                    ("base.gru.bias_ih_l0", (3 * Hh,)), ("base.gru.bias_hh_l0", (3 * Hh,))] if self._rec() else [])
            return gru + [("base.main.0.weight", (32, self.cnn, 8, 8)), ("base.main.0.bias", (32,)),
                          ("base.main.2.weight", (64, 32, 4, 4)), ("base.main.2.bias", (64,)),
                          ("base.main.4.weight", (32, 64, 3, 3)), ("base.main.4.bias", (32,)),
                          ("base.main.7.weight", (Hh, 32 * 7 * 7)), ("base.main.7.bias", (Hh,)),
                          ("base.critic_linear.weight", (1, Hh)), ("base.critic_linear.bias", (1,))] + head
        gru = []
        if self._rec():   # a2c/model.py:124-131: nn.GRU's four tensors come first and the trunks read its H-wide state
            gru = [("base.gru.weight_ih_l0", (3 * Hh, O)), ("base.gru.weight_hh_l0", (3 * Hh, Hh)),
                   ("base.gru.bias_ih_l0", (3 * Hh,)), ("base.gru.bias_hh_l0", (3 * Hh,))]
            O = Hh
        if getattr(self, "dist_kind", 0):   # a2c/distributions.py:74-88,157-168: Categorical / Bernoulli hold one Linear, no log-std
            K = self.n_out
            return gru + [("base.actor.0.weight", (Hh, O)), ("base.actor.0.bias", (Hh,)),
                          ("base.actor.2.weight", (Hh, Hh)), ("base.actor.2.bias", (Hh,)),
                          ("base.critic.0.weight", (Hc, O)), ("base.critic.0.bias", (Hc,)),
                          ("base.critic.2.weight", (Hc, Hc)), ("base.critic.2.bias", (Hc,)),
                          ("base.critic_linear.weight", (1, Hc)), ("base.critic_linear.bias", (1,)),
                          ("dist.linear.weight", (K, Hh)), ("dist.linear.bias", (K,))]
        return gru + [("base.actor.0.weight", (Hh, O)), ("base.actor.0.bias", (Hh,)),
                      ("base.actor.2.weight", (Hh, Hh)), ("base.actor.2.bias", (Hh,)),
                      ("base.critic.0.weight", (Hc, O)), ("base.critic.0.bias", (Hc,)),
                      ("base.critic.2.weight", (Hc, Hc)), ("base.critic.2.bias", (Hc,)),
                      ("base.critic_linear.weight", (1, Hc)), ("base.critic_linear.bias", (1,)),
                      ("dist.fc_mean.weight", (A, Hh)), ("dist.fc_mean.bias", (A,)),
                      ("dist.logstd._bias", (A, 1))]

    def _init_params(self, rng):
        """a2c/model.py:240-251 (orthogonal, gain sqrt2, zero bias), a2c/distributions.py:95-104
        (fc_mean gain 1 then /50, logstd -0.5), :78-84 (Categorical: dist.linear gain 0.01), :161-164 (Bernoulli: gain 1); the GRU, a2c/model.py:126-130: orthogonal (gain 1) on each whole [3H, .]
        weight, zero biases."""
        sd = {}
        for name, shape in self.param_shapes():
            if name.endswith("logstd._bias"):
                sd[name] = np.full(shape, -0.5, np.float32)
            elif name.endswith("bias") or name.startswith("base.gru.bias"):
                sd[name] = np.zeros(shape, np.float32)
            elif name.startswith("base.gru.weight"):
                sd[name] = orthogonal(rng, *shape, gain=1.0)
            elif name.startswith("dist.fc_mean"):
                sd[name] = orthogonal(rng, *shape, gain=1.0) / 50.0
            elif name.startswith("dist.linear"):
                sd[name] = orthogonal(rng, *shape, gain=0.01 if self.dist_kind == _lib.DIST_CATEGORICAL else 1.0)
            elif name.startswith("base.main"):   # a2c/model.py:208-215: orthogonal over [out, in * kh * kw], ReLU gain
                sd[name] = orthogonal(rng, shape[0], int(np.prod(shape[1:])), gain=np.sqrt(2)).reshape(shape)
            elif name.startswith("base.critic_linear") and getattr(self, "cnn", 0):   # a2c/model.py:217-220: gain 1
                sd[name] = orthogonal(rng, *shape, gain=1.0)
            else:
                sd[name] = orthogonal(rng, *shape, gain=np.sqrt(2))
        self.load_state_dict(sd)

    def reset_variance(self, action_space, log_std):
        """a2c/model.py:76-78"""
        if self.dist_kind:   # (the reference dies with an AttributeError: Categorical / Bernoulli have no reset_variance)
            raise ValueError("reset_variance: a Categorical / Bernoulli head has no log-std to reset (Box action spaces only)")
        sd = self.state_dict()
        sd["dist.logstd._bias"] = np.full((action_space.shape[0], 1), log_std, np.float32)
        self.load_state_dict(sd)

    def reset_critic(self, obs_shape, seed=1):
        """a2c/model.py:80-87: a fresh critic -- Linear(obs, 64)-Tanh-Linear(64, 64)-Tanh + Linear(64, 1), orthogonal with gain
        sqrt 2, zero biases -- whatever the actor's width ("64" is hard-coded in the reference; a2c/main.py:85 calls this on
        every warm start).  When the actor is not 64 wide the policy is rebuilt on the device with a critic trunk of its own
        width (sg_policy_create2); actor, mean head and log-std keep their values.  Call it BEFORE constructing PPO on this
        policy, as the reference's main does (:85 then :149): an agent built earlier holds the old device handle."""
        if getattr(self, "cnn", 0):
            # the reference's call would hang a fresh MLP critic on the CNNBase that its forward never uses (a2c/model.py:80-87,224-230)
            raise NotImplementedError("reset_critic on a policy with the CNN base: the reference's call leaves a `critic` module that "
                                      "CNNBase.forward never reads; there is nothing to reset")
        if int(obs_shape[0]) != self.obs_dim:
            raise ValueError(f"reset_critic: obs_shape {tuple(obs_shape)} != the policy's observation size {self.obs_dim}")
        if self._rec() and self.obs_dim != self.hidden_size:
            # the reference builds Linear(obs_shape[0], 64) against the H-wide GRU state: its next forward fails unless O == H
            raise ValueError(f"reset_critic on a recurrent policy needs obs size == hidden size (the reference's new critic reads "
                             f"{self.obs_dim} inputs from a {self.hidden_size}-wide GRU state)")
        rng = np.random.default_rng(seed)
        sd = self.state_dict()
        if self.critic_hidden != 64:
            users = [u for u in self.__dict__.get("_handle_users", ()) if u() is not None]
            if users:   # they hold the device handle that is about to be replaced: refuse instead of freeing it under them
                raise RuntimeError(f"reset_critic: {len(users)} object(s) built on this policy ({', '.join(type(u()).__name__ for u in users)}) "
                                   "hold its device handle, which a critic of another width replaces; call reset_critic first "
                                   "(a2c/main.py:85 precedes :149) or rebuild them afterwards")
            old, seed_, calls_ = self.h, self.seed, self._act_calls
            self._create(self.obs_dim, self.act_dim, self.hidden_size, self.num_feet, self.ctx, critic_hidden=64,
                         recurrent=self._rec(), dist=self.dist_kind, n_out=self.__dict__.get("n_out"))
            self.seed, self._act_calls = seed_, calls_     # the action-noise stream goes on where it was
            self.lib.sg_policy_destroy(old)
        for name, shape in self.param_shapes():
            if name.startswith("base.critic"):
                sd[name] = (np.zeros(shape, np.float32) if name.endswith("bias")
                            else orthogonal(rng, *shape, gain=np.sqrt(2)))
        self.load_state_dict(sd)
