/*
 * simgan_hip.h -- C ABI of libsimgan_hip.so: SimGAN's GAIL+PPO update path as
 * hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference (jyf588/SimGAN) has no FFI: its hot path sits behind Python
 * classes.  Each entry point below replaces the body of
 * one reference method; the Python shim in simgan_amd/ keeps the reference's
 * class/method surface and binds these symbols with ctypes.
 * a2c/ = third_party/a2c_ppo_acktr/ in the reference tree.
 *
 * Conventions
 *   - plain C types only; all tensors are float32, row-major, caller-owned HOST
 *     pointers unless a name says "dev"; indices are int64.
 *   - every function returns 0 on success, <0 on error; sg_last_error() returns
 *     a thread-local message.
 *   - handles are opaque; one sg_ctx per GPU/process; not thread-safe (the
 *     reference learner is single-threaded: a2c/main_gail_dyn_ppo.py:64).
 *   - every stochastic input is optional by pointer: pass the reference's
 *     RNG artefacts (permutations / alpha / noise) for parity, or NULL to use
 *     the library's own counter-based generator seeded by `seed`.
 *   - flat parameter vectors use torch state_dict order of the reference
 *     modules (see oracle/sg_oracle.c header for the exact order).
 */
#ifndef SIMGAN_HIP_H
#define SIMGAN_HIP_H

#include <stdint.h>

/* The library is built with -fvisibility=hidden: exactly the entry points declared here are exported
 * (tests/test_abi.py checks both directions against `nm -D`).  Test hooks and probe kernels live in a
 * separate libsimgan_hip_test.so (simgan_amd/csrc/sg_test_api.h), never in the product library. */
#define SG_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sg_ctx sg_ctx;
typedef struct sg_policy sg_policy;
typedef struct sg_rollout sg_rollout;
typedef struct sg_ppo sg_ppo;
typedef struct sg_disc sg_disc;

/* ------------------------------------------------------------------ context */
SG_API const char *sg_last_error(void);
SG_API const char *sg_version(void);
/* Creates the context on HIP device `device` (one stream, scratch arenas). */
SG_API int sg_ctx_create(int device, sg_ctx **out);
SG_API int sg_ctx_destroy(sg_ctx *ctx);
SG_API int sg_ctx_synchronize(sg_ctx *ctx);
/* Device properties the bench reports: name, CU count, HBM bytes. */
SG_API int sg_ctx_device_info(sg_ctx *ctx, char *name, int name_len, int *num_cu, int64_t *hbm_bytes);

/* Data-parallel communicator over RCCL (one process per GPU, xGMI). Replaces nothing in the
 * reference (single process, a2c/main_gail_dyn_ppo.py:64); added per BASELINE.json north_star.
 * id is the 128-byte ncclUniqueId produced on rank 0 and broadcast by the host launcher. */
SG_API int sg_comm_unique_id(uint8_t id[128]);
/* An id for the LOOPBACK transport instead: `world` contexts of ONE host (threads or processes, any devices -- also all
 * on the same device) exchange through a shared-memory segment named by the id; sg_ctx_comm_init recognises the id's
 * tag.  Every world > 1 code path of the library then runs on a one-GPU box (tests, bench.py --loopback); it
 * synchronises the stream per collective and is not a performance path. */
SG_API int sg_comm_loopback_id(uint8_t id[128]);
SG_API int sg_ctx_comm_init(sg_ctx *ctx, const uint8_t id[128], int rank, int world);
/* *kind = 0 no communicator, 1 RCCL, 2 loopback; + 4 when the per-step float32 gradient all-reduces run as one kernel over
 * peer-mapped device memory instead of a library collective (SG_COMM_PEER=1 in the environment at sg_ctx_comm_init: opt-in,
 * built over either transport). */
SG_API int sg_ctx_comm_kind(sg_ctx *ctx, int *kind);
/* Collective over an initialised communicator (every rank, same argument): 1 builds the peer mesh for the per-step float32
 * gradient all-reduce (what SG_COMM_PEER=1 does at sg_ctx_comm_init), 0 returns to the base communicator.  The outcome is
 * collective: every rank leaves with the mesh or every rank gets the error.  No counterpart in the reference (single process,
 * a2c/main_gail_dyn_ppo.py:64); bench.py times both all-reduce forms with it on the first multi-GPU run. */
SG_API int sg_ctx_comm_set_peer(sg_ctx *ctx, int enable);
/* rank / world as the communicator itself reports them (ncclCommUserRank / ncclCommCount) once it exists. */
SG_API int sg_ctx_comm_info(sg_ctx *ctx, int *rank, int *world);
/* Discriminator data-parallel mode for world > 1: 0 = replicated (default: one all-gather of
 * the ranks' rows per epoch, identical full-batch steps everywhere), 1 = sharded (batch/world rows per rank and one
 * gradient all-reduce per step).  Initial value: SG_DISC_DP=sharded in the environment. */
SG_API int sg_ctx_set_disc_dp(sg_ctx *ctx, int sharded);

/* ------------------------------------------------------------------- policy */
enum { SG_POLICY_MLP = 0, SG_POLICY_SPLIT = 1, SG_POLICY_GRU = 2 };
/* kind SG_POLICY_GRU (sg_policy_create / sg_policy_create2; num_feet ignored): Policy(..., base_kwargs={'recurrent': True,
 * 'hidden_size': H}), a2c/model.py:117-131,233-253 -- nn.GRU(obs_dim, H) (one layer, gates r, z, n), then the actor and critic
 * trunks on the H-wide GRU state, critic_linear and DiagGaussian.  Flat parameter order: base.gru.weight_ih_l0 [3H, O],
 * weight_hh_l0 [3H, H], bias_ih_l0 [3H], bias_hh_l0 [3H], then the MLP kind's order with obs_dim replaced by H.  Such a policy
 * is served by the sg_policy_*_rnn entry points below; sg_policy_act / _get_value / _evaluate / _act_ensemble refuse it (and
 * the _rnn calls refuse a feed-forward policy), as do sg_a2c_create, sg_a2c_create_cnn, sg_acktr_create,
 * sg_rollout_compute_returns_policy (on a rollout without hidden states) and sg_rollout_fill_synthetic.  sg_ppo_create takes it: sg_ppo_update then runs PPO through time (sg_ppo_set_hidden_states). */
/* Policy(obs_shape, action_space, base_kwargs)            a2c/model.py:38-67   (kind MLP)
 * SplitPolicy(obs_shape, action_space, base_kwargs)       a2c/model_split.py:40-52 (kind SPLIT;
 * requires act_dim == 7*num_feet, a2c/model_split.py:205). Parameters start at zero. */
SG_API int sg_policy_create(sg_ctx *ctx, int kind, int obs_dim, int act_dim, int hidden, int num_feet,
                     sg_policy **out);
/* The same with a critic trunk of its own width (critic_hidden; 0 = hidden): Policy.reset_critic(obs_shape) rebuilds a
 * 64-unit critic beside an actor of ANY hidden size (a2c/model.py:80-87; a2c/main.py:85 calls it on every warm start).
 * state_dict order and entry points are unchanged; base.critic.* and base.critic_linear take the critic's width. */
SG_API int sg_policy_create2(sg_ctx *ctx, int kind, int obs_dim, int act_dim, int hidden, int num_feet, int critic_hidden,
                             sg_policy **out);
/* Policy on a Discrete / MultiBinary action space (a2c/model.py:52-62, a2c/distributions.py:33-88,157-168): sg_policy_create2's
 * arguments plus the distribution and its head width.  dist SG_DIST_GAUSSIAN: n_out is ignored and the call is
 * sg_policy_create2.  SG_DIST_CATEGORICAL (Discrete(n_out)): act_dim must be 1 -- an action row holds the class index as a
 * float, which is why n_out < 2^24 -- and the head is Linear(hidden, n_out).  SG_DIST_BERNOULLI (MultiBinary(n_out)): act_dim
 * == n_out, an action row holds n_out 0/1 floats.  Neither has a log-std: the flat order ends with dist.linear.weight
 * [n_out, hidden], dist.linear.bias [n_out].  kind must be SG_POLICY_MLP.  `noise` of sg_policy_act is then UNIFORM draws in
 * [0, 1): one per row (categorical: inverse CDF over ascending class index) or one per bit (Bernoulli: bit = u < p).
 * sg_ppo_create (any world) and sg_a2c_create take such a policy (sg_a2c_create_cnn: the Categorical head on the CNN base);
 * sg_acktr_create, sg_ppo_set_symmetry (coef > 0) and sg_policy_act_ensemble refuse it. */
enum { SG_DIST_GAUSSIAN = 0, SG_DIST_CATEGORICAL = 1, SG_DIST_BERNOULLI = 2 };
SG_API int sg_policy_create3(sg_ctx *ctx, int kind, int obs_dim, int act_dim, int hidden, int num_feet, int critic_hidden,
                             int dist, int n_out, sg_policy **out);
/* The recurrent Policy on a Discrete / MultiBinary action space (a2c/model.py:40-62 with base_kwargs={'recurrent': True}): kind
 * SG_POLICY_GRU with dist SG_DIST_CATEGORICAL (an action row is 1 class index) or SG_DIST_BERNOULLI (n_out bits); sg_policy_create3
 * keeps refusing the pair.  The heads are sg_policy_create3's on the hidden-wide GRU state; flat order: base.gru.weight_ih_l0,
 * .weight_hh_l0, .bias_ih_l0, .bias_hh_l0, the trunks, base.critic_linear, dist.linear.weight [n_out, hidden], dist.linear.bias.
 * sg_policy_act_rnn / _get_value_rnn / _evaluate_rnn take it (`noise`: uniform draws, one per row or per bit), as do sg_ppo_create
 * and sg_a2c_create_rnn (one rank each) and sg_rollout_policy_diagnostics; sg_acktr_create, sg_ppo_set_symmetry (coef > 0),
 * sg_policy_act_ensemble, sg_rollout_act_step_rnn and sg_rollout_act_step_chain refuse it (those act kernels carry the Gaussian
 * head: act through sg_policy_act_rnn). */
SG_API int sg_policy_create_rnn_dist(sg_ctx *ctx, int obs_dim, int hidden, int critic_hidden, int dist, int n_out, sg_policy **out);
/* Policy on image observations: the CNN base, a2c/model.py:204-230 (CNNBase, feed-forward), which Policy.__init__ picks for a
 * 3-D obs_shape (a2c/model.py:40-50).  x / 255.0 -> Conv2d(channels, 32, 8, stride 4) -> Conv2d(32, 64, 4, stride 2) ->
 * Conv2d(64, 32, 3, stride 1) -> Flatten (channel-major, 1568 values) -> Linear(1568, hidden), ReLU after each; critic_linear =
 * Linear(hidden, 1) and the distribution's Linear read the same features.  height and width must be 84 (the reference
 * hard-codes 32 * 7 * 7, a2c/model.py:216).  dist SG_DIST_GAUSSIAN (Box((act_dim,)); n_out ignored) or SG_DIST_CATEGORICAL
 * (Discrete(n_out); act_dim 1); SG_DIST_BERNOULLI is refused.  An observation row is channels * 84 * 84 floats (NCHW).  Flat
 * parameter order: base.main.0.weight [32, channels, 8, 8], .bias, base.main.2.weight [64, 32, 4, 4], .bias, base.main.4.weight
 * [32, 64, 3, 3], .bias, base.main.7.weight [hidden, 1568], .bias, base.critic_linear.weight [1, hidden], .bias, then
 * dist.linear.weight [n_out, hidden], .bias or dist.fc_mean.weight [act_dim, hidden], .bias, dist.logstd._bias [act_dim].
 * The handle is taken by sg_policy_act / _get_value / _evaluate / _get_params / _set_params / _num_params, sg_ppo_create
 * (one rank), sg_ppo_update (feed-forward sampler, injected perms, sg_ppo_last_perms, the results ring), sg_ppo_get_adam /
 * _set_adam, sg_a2c_create_cnn (one rank; sg_a2c_get_rmsprop / _set_rmsprop), sg_rollout_compute_returns_policy and
 * sg_rollout_fill_synthetic; it is refused, each with a message naming the CNN base, by sg_a2c_create (A2C on it is opt-in by
 * entry point), sg_acktr_create, sg_ppo_set_symmetry (coef > 0), sg_policy_act_ensemble, sg_rollout_act_step,
 * sg_rollout_act_step_rnn and by sg_ppo_create on a context whose communicator has world > 1.  sg_policy_create / create2 /
 * create3 do not reach it: they keep refusing every kind but their three. */
SG_API int sg_policy_create_cnn(sg_ctx *ctx, int channels, int height, int width, int hidden, int dist, int act_dim, int n_out,
                                sg_policy **out);
/* The same base with recurrent=True (a2c/model.py:117-230, --recurrent-policy on image observations): the three convolutions and
 * the FC layer, then nn.GRU(hidden, hidden) on the features, then critic_linear and the Categorical / Gaussian head on the GRU
 * state.  sg_policy_create_cnn's checks and heads; it also refuses, with its own message, a `hidden` whose 16-row GRU tiles
 * (input projection, the two scans, the input gradient) do not fit a CU's LDS even with the weights read from global memory
 * (hidden = 512, the reference's default, fits).  Flat (state_dict) order: base.gru.weight_ih_l0 [3 hidden, hidden], weight_hh_l0,
 * bias_ih_l0, bias_hh_l0 (NNBase.__init__ creates the GRU before `main`), then sg_policy_create_cnn's order; on the device the
 * CNN's flat block comes first and the GRU's tile-padded block behind it (padding stays zero in weights, gradient and moments).
 * Served by sg_policy_act_rnn / _get_value_rnn / _evaluate_rnn (obs rows are the C * 7056-float images; hxs [n][hidden], masks
 * [T * n]; a one-step call and the same step inside a sequence give the same bits), sg_policy_get_params / _set_params,
 * sg_ppo_create (one rank) with sg_ppo_set_hidden_states (slot 0) before every sg_ppo_update -- PPO through time over minibatches
 * of N // num_mini_batch whole environments read time-major in place from the image rollout, injected perms [ppo_epoch][N],
 * minibatches above 4096 rows refused -- and sg_ppo_get_adam / _set_adam; and by sg_a2c_create_cnn_rnn (one rank; A2C through
 * time, sg_a2c_get_rmsprop / _set_rmsprop).  Everything else that can reach the handle refuses it
 * with a message naming the recurrent CNN base: sg_a2c_create / _create_rnn / _create_cnn, sg_acktr_create, the diagnostics entry
 * points, sg_rollout_act_step / _act_step_rnn / _act_step_chain, sg_rollout_compute_returns_policy, sg_policy_act_ensemble,
 * sg_ppo_set_symmetry (coef > 0), sg_ppo_create on a communicator of world > 1; sg_rollout_enable_hidden refuses an image rollout. */
SG_API int sg_policy_create_cnn_rnn(sg_ctx *ctx, int channels, int height, int width, int hidden, int dist, int act_dim, int n_out,
                                    sg_policy **out);
SG_API int sg_policy_destroy(sg_policy *p);
SG_API int sg_policy_num_params(const sg_policy *p, int64_t *n);
/* nn.Module.load_state_dict / state_dict, flattened. */
SG_API int sg_policy_set_params(sg_policy *p, const float *flat, int64_t n);
SG_API int sg_policy_get_params(sg_policy *p, float *flat, int64_t n);
/* Policy.act a2c/model.py:89-101, SplitPolicy.act a2c/model_split.py:70-82.
 * obs[n,O]; noise[n,A] standard normal draws or NULL (-> library RNG with `seed`);
 * deterministic != 0 -> dist.mode().  Outputs value[n], action[n,A], logp[n]. */
SG_API int sg_policy_act(sg_policy *p, const float *obs, int n, const float *noise, uint64_t seed,
                  int deterministic, float *value, float *action, float *logp);
/* Policy.get_value a2c/model.py:103-105 */
SG_API int sg_policy_get_value(sg_policy *p, const float *obs, int n, float *value);
/* Policy.evaluate_actions a2c/model.py:107-114: value[n], logp[n], *entropy = dist.entropy().mean() */
SG_API int sg_policy_evaluate(sg_policy *p, const float *obs, const float *action, int n, float *value,
                       float *logp, float *entropy);
/* Recurrent forms (kind SG_POLICY_GRU).  One step, MLPBase.forward -> NNBase._forward_gru with x.size(0) == hxs.size(0),
 * a2c/model.py:137-141,255-264: h' = GRU(obs, hxs * masks); the heads run on h'.  obs[n,O], hxs[n,H], masks[n] ->
 * hxs_out[n,H] = h'; the other arguments as in sg_policy_act (Policy.act, a2c/model.py:89-101). */
SG_API int sg_policy_act_rnn(sg_policy *p, const float *obs, const float *hxs, const float *masks, int n, const float *noise,
                      uint64_t seed, int deterministic, float *value, float *action, float *logp, float *hxs_out);
/* Policy.get_value a2c/model.py:103-105 on a recurrent policy (the new state is dropped, as the reference drops it). */
SG_API int sg_policy_get_value_rnn(sg_policy *p, const float *obs, const float *hxs, const float *masks, int n, float *value);
/* Policy.evaluate_actions a2c/model.py:107-114 over a sequence, NNBase._forward_gru's second branch a2c/model.py:142-199:
 * obs[T*n,O], masks[T*n] and action[T*n,A] are time-major (row t*n + j), hxs[n,H] is the state before step 0.  The reference
 * cuts the sequence where a mask is 0 and multiplies h by masks[t] at the head of each piece; for 0/1 masks that is
 * h_{t-1} * masks[t] at every step, which is what runs here.  value[T*n], logp[T*n], *entropy = dist.entropy().mean(),
 * hxs_out[n,H] = the state after step T-1.  T == 1 is the one-step form. */
SG_API int sg_policy_evaluate_rnn(sg_policy *p, const float *obs, const float *hxs, const float *masks, const float *action,
                           int T, int n, float *value, float *logp, float *entropy, float *hxs_out);
/* The policies that live INSIDE the reference's hybrid-sim environments, batched over the N environments of a
 * pool: every worker calls a batch-1 actor_critic.act per step, in refinement mode on one of five saved dynamics
 * policies drawn per step (my_pybullet_envs/hopper_env_combined_policy.py:113-140,211-216,
 * laikago_env_combined_policy.py:126-153,263-268).  ONE launch: row i of obs[n,O] goes through
 * policies[idx[i]] (0 <= idx[i] < n_policies <= SG_ENSEMBLE_MAX, all members the same kind and shape, weights
 * resident).  noise / seed / deterministic and the outputs are as in sg_policy_act. */
#define SG_ENSEMBLE_MAX 8
SG_API int sg_policy_act_ensemble(sg_policy *const *policies, int n_policies, const int32_t *idx, const float *obs,
                           int n, const float *noise, uint64_t seed, int deterministic, float *value,
                           float *action, float *logp);

/* ------------------------------------------------------------------ rollout */
/* RolloutStorage(num_steps, num_processes, obs_shape, action_space, rhs, feat_len) a2c/storage.py:32-56.
 * Device-resident buffers, same shapes and row-major (t, n, ·) order as the reference. */
enum {
    SG_F_OBS = 0,          /* [T+1, N, O] */
    SG_F_OBS_FEAT = 1,     /* [T+1, N, F] */
    SG_F_ACTIONS = 2,      /* [T,   N, A] */
    SG_F_REWARDS = 3,      /* [T,   N]    */
    SG_F_VALUE_PREDS = 4,  /* [T+1, N]    */
    SG_F_RETURNS = 5,      /* [T+1, N]    */
    SG_F_LOGP = 6,         /* [T,   N]  action_log_probs */
    SG_F_MASKS = 7,        /* [T+1, N]    */
    SG_F_BAD_MASKS = 8,    /* [T+1, N]    */
    SG_F_ADVANTAGES = 9,   /* [T,   N]  normalised advantages of the last sg_ppo_update (read-only) */
    SG_F_COUNT = 10
};
SG_API int sg_rollout_create(sg_ctx *ctx, int T, int N, int obs_dim, int act_dim, int feat_dim,
                      sg_rollout **out);
SG_API int sg_rollout_destroy(sg_rollout *r);
/* Whole-field host<->device copies; count = number of floats (must equal the field size). */
SG_API int sg_rollout_upload(sg_rollout *r, int field, const float *host, int64_t count);
SG_API int sg_rollout_download(sg_rollout *r, int field, float *host, int64_t count);
/* One time-slot [t] of a field (N * width floats): the reference's rollouts.obs[step].copy_(..). */
SG_API int sg_rollout_upload_step(sg_rollout *r, int field, int t, const float *host, int64_t count);
SG_API int sg_rollout_download_step(sg_rollout *r, int field, int t, float *host, int64_t count);
/* RolloutStorage.after_update a2c/storage.py:96-101: slot T -> slot 0 for obs, obs_feat, masks, bad_masks */
SG_API int sg_rollout_after_update(sg_rollout *r);
/* RolloutStorage.compute_returns a2c/storage.py:103-142 (all four branches); next_value[N] host. */
SG_API int sg_rollout_compute_returns(sg_rollout *r, const float *next_value, int use_gae, float gamma,
                               float gae_lambda, int use_proper_time_limits);
/* Same, with next_value = policy.get_value(obs[T]) computed on device (a2c/main_gail_dyn_ppo.py:239-242,299).  A recurrent
 * policy is taken when the rollout holds hidden states of its width (sg_rollout_enable_hidden): next_value =
 * get_value(obs[T], h[T], masks[T]) from the rollout's own slots, the bits of sg_policy_get_value_rnn; refused otherwise. */
SG_API int sg_rollout_compute_returns_policy(sg_rollout *r, sg_policy *p, int use_gae, float gamma,
                                      float gae_lambda, int use_proper_time_limits);
/* Synthetic rollout fill on device for benchmarks: obs, obs_feat ~ N(0,1);
 * actions/logp/value_preds from policy.act; masks ~ Bernoulli(1-p_done); bad_masks = 1. */
SG_API int sg_rollout_fill_synthetic(sg_rollout *r, sg_policy *p, uint64_t seed, float p_done);
/* Mirror-augmented rollouts, a2c/main.py:171-245 (--dup-sym): the rollout has N = 2n columns, [0, n) the environments and
 * column n + j the mirror image of column j.  The reference mirrors every step's rows on the host and inserts 2n rows
 * (:181-185, :231-242); here the mirrored half is made on the device.  m_obs [O*O] and m_act [A*A] are row-major linear
 * maps, mirrored = M x (what mirror_obsact_batch's per-row callable computes, my_pybullet_envs/utils.py:334-357), uploaded
 * once.  m_act is required; m_obs NULL (the convention of sg_ppo_set_symmetry): the caller mirrors observations itself and
 * uploads OBS full-width, and sg_rollout_dup_sym leaves OBS alone.  Odd N and non-finite entries are errors. */
SG_API int sg_rollout_set_mirrors(sg_rollout *r, const float *m_obs, const float *m_act);
/* The mirrored half of every slot in ONE launch, queued on the context's stream (the host does not wait): a2c/main.py:232-242
 * for all T steps at once and :181-185 for slot 0.  OBS and ACTIONS go through M_obs / M_act (double accumulation over
 * ascending j, zero entries skipped, one cast: sg_ppo_set_symmetry's arithmetic, exact for a signed permutation); OBS_FEAT,
 * REWARDS, VALUE_PREDS, LOGP, MASKS and BAD_MASKS are repeated (.repeat(2, 1), obs_feat included although it is a copy of the
 * observation).  Slots 0..T of OBS, OBS_FEAT, MASKS, BAD_MASKS and slots 0..T-1 of ACTIONS, REWARDS, LOGP, VALUE_PREDS are
 * written; VALUE_PREDS[T], RETURNS, ADVANTAGES and columns [0, n) of every field are left alone (the bootstrap value of a
 * mirrored column is get_value(obs[-1]) = V(mirror(s_T)), :247-250, not a repeat).  An error before sg_rollout_set_mirrors. */
SG_API int sg_rollout_dup_sym(sg_rollout *r);
/* Columns [0, n_cols) of every slot of a field, host -> device, as one strided copy: what crosses the link of a rollout whose
 * other columns the device makes itself (the first half of a2c/main.py:241-242's insert).  host is the FULL-width field
 * (count = its size, as for sg_rollout_upload), e.g. the page-locked host tensor; its other columns are not read. */
SG_API int sg_rollout_upload_columns(sg_rollout *r, int field, int n_cols, const float *host, int64_t count);
/* One step of the collection loop on the device (a2c/main_gail_dyn_ppo.py:209-236): Policy.act / SplitPolicy.act
 * (a2c/model.py:89-101, a2c/model_split.py:70-82) on the N rows of rollout slot t, written where rollouts.insert
 * (a2c/storage.py:70-84) puts them: value_preds[t], actions[t] and action_log_probs[t] of the DEVICE rollout; the actions also
 * to action_host[N,A].  obs_host[N,O] is copied into slot t of OBS first; NULL: slot t is already on the device.  noise[N,A]
 * (host, standard normal draws) or NULL -> the library generator with `seed`, as in sg_policy_act; deterministic != 0 ->
 * dist.mode().  Per call: one host->device copy (one more with injected noise), ONE kernel launch -- which writes the actions
 * into a page-locked block of the context as well, so nothing is copied back -- and one host wait.  Value, action and log-prob
 * have the bits sg_policy_act gives for the same observations and draws.  No other float of the rollout is written.
 * Feed-forward policies (SG_POLICY_MLP, SG_POLICY_SPLIT) with the Gaussian head; a recurrent policy, a Categorical / Bernoulli
 * head, policy and rollout dimensions that differ and t outside [0, T) are errors. */
SG_API int sg_rollout_act_step(sg_rollout *r, sg_policy *p, int t, const float *obs_host, const float *noise, uint64_t seed,
                        int deterministic, float *action_host);
/* rollouts.recurrent_hidden_states (a2c/storage.py:40) on the device, opt-in: a zeroed [T+1, N, hidden_dim] float buffer beside
 * the SG_F_COUNT fields.  Calling it again with the same hidden_dim does nothing; another width is an error.  Once enabled,
 * sg_rollout_after_update rolls slot T of the buffer to slot 0 with the fields (a2c/storage.py:96-101), in the same launch. */
SG_API int sg_rollout_enable_hidden(sg_rollout *r, int hidden_dim);
/* The whole buffer host <-> device; count must be (T+1)*N*hidden_dim.  Errors before sg_rollout_enable_hidden. */
SG_API int sg_rollout_upload_hidden(sg_rollout *r, const float *host, int64_t count);
SG_API int sg_rollout_download_hidden(sg_rollout *r, float *host, int64_t count);
/* sg_rollout_act_step for a recurrent policy (kind SG_POLICY_GRU): Policy.act with recurrent=True (a2c/model.py:89-101,
 * 117-201, 255-264) on slot t -- x = GRU(obs[t], h[t] * masks[t]), the trunks and the Gaussian head on x -- and the policy's
 * half of rollouts.insert (a2c/storage.py:70-84), hidden state included: value_preds[t], actions[t], action_log_probs[t] and
 * hidden slot t + 1 of the DEVICE rollout; the actions also to action_host[N,A].  obs_host[N,O] and masks_host[N] are copied
 * into slot t of OBS / MASKS first; NULL: that slot is already on the device.  noise, seed, deterministic as in
 * sg_rollout_act_step.  ONE kernel launch and one host wait per call; value, action, log-prob and new state have the bits
 * sg_policy_act_rnn gives for the same inputs and draws.  No other float of the rollout is written.  Errors: a feed-forward
 * policy, a rollout without hidden states or with another width, policy and rollout dimensions that differ, t outside [0, T),
 * a mirror-augmented rollout (sg_rollout_set_mirrors), and a shape whose row tile does not fit a CU's LDS (act through
 * sg_policy_act_rnn then). */
SG_API int sg_rollout_act_step_rnn(sg_rollout *r, sg_policy *p, int t, const float *obs_host, const float *masks_host,
                            const float *noise, uint64_t seed, int deterministic, float *action_host);
/* The two policies of a hybrid-sim environment step in ONE launch: the policy that lives inside the environment (row i acts
 * with members[idx[i]], as in sg_policy_act_ensemble) and the learner (as in sg_rollout_act_step), with what the environment
 * does between them -- squash the first action, concatenate it behind the state -- kept on the device.
 *   SG_CHAIN_INNER_FIRST (GAIL-dyn stage, my_pybullet_envs/hopper_env_combined_policy.py:298-325,
 *     laikago_env_combined_policy.py:420-438): the members act on inner_obs_host[N,O_member]; OBS[t] of the device rollout
 *     becomes cat(state, squash(a_inner)); the learner acts on that row and fills value_preds[t], actions[t] and
 *     action_log_probs[t].  state_host[N,Os] with Os = O - A_member; NULL: inner_obs_host is the state (O_member == Os).
 *     obs_host is not read.  t == T is allowed: the members run, OBS[T] is completed, the learner does not act and action_host
 *     is not written (it may be NULL then).  inner_action_host[N,A_member] gets the SQUASHED member action (what sits in OBS).
 *   SG_CHAIN_LEARNER_FIRST (refinement stage, hopper...:195-216, laikago...:240-268): the learner acts on OBS[t] (obs_host[N,O]
 *     is copied into the slot first; NULL: the slot as it is) and fills the slot's three fields; the members act on
 *     cat(state, squash(action)), state_host[N,Os] with Os = O_member - A; NULL: OBS[t] is the state (Os == O).
 *     inner_obs_host is not read.  inner_action_host gets the members' RAW action.
 * squash != 0: tanhf; 0: the action passes as it is.  action_host[N,A]: the learner's raw action.  inner_raw_host[N,A_member]
 * (optional): the members' raw action in both orders.  noise / seed / deterministic drive the learner's head and inner_noise /
 * inner_seed / inner_deterministic the members', each exactly as in its stand-alone call, and each half has that call's bits:
 * the same weight path, the same row tile class (a half whose own launch would run 16-row tiles runs them inside the chain
 * too), the same head arithmetic and draw indexing.  Per call: one host->device copy (one more for obs_host), ONE launch, one
 * host wait.  Errors, each with its own message: NULL arguments; an unknown order; a learner or member with the CNN base, a GRU
 * or a Categorical / Bernoulli head; members of differing shape or on another context; idx outside [0, n_members); dims that do
 * not add up; t out of range; halves whose stand-alone launches read their weights differently (one from LDS, one from global
 * memory); a tile of both policies that does not fit a CU's LDS. */
enum { SG_CHAIN_INNER_FIRST = 0, SG_CHAIN_LEARNER_FIRST = 1 };
SG_API int sg_rollout_act_step_chain(sg_rollout *r, sg_policy *learner, int t, int order, sg_policy *const *members, int n_members,
                              const int32_t *idx, const float *inner_obs_host, const float *state_host, const float *obs_host,
                              const float *inner_noise, uint64_t inner_seed, int inner_deterministic, const float *noise,
                              uint64_t seed, int deterministic, int squash, float *action_host, float *inner_action_host,
                              float *inner_raw_host);
/* What one looks at after an update, over the T*N rows of the first T slots of the DEVICE rollout and the policy's CURRENT
 * parameters.  Replaces the host route to numbers the reference's learners do not return (a2c/algo/ppo.py:65-157 and
 * a2c/algo/a2c_acktr.py:52-102 give value loss, action loss and entropy): Policy.evaluate_actions / SplitPolicy.evaluate_actions
 * (a2c/model.py:107-114, a2c/model_split.py:84-95) on every row through the host, ratio = exp(action_log_probs -
 * old_action_log_probs) (a2c/algo/ppo.py:93-94) and the caller's numpy reductions over the downloaded arrays.  With logp_old =
 * LOGP, vpred = VALUE_PREDS[:-1], ret = RETURNS[:-1], (v_new, logp_new, entropy) = evaluate_actions(OBS[:-1], ACTIONS) and
 * r = exp(logp_new - logp_old), out10 = SG_DIAG_N doubles:
 *   [0] rows                    T*N
 *   [1] approx_kl               mean(logp_old - logp_new)
 *   [2] approx_kl_k3            mean((r - 1) - log r)
 *   [3] clip_fraction           share of rows with |r - 1| > clip_param
 *   [4] entropy                 mean entropy
 *   [5] ratio_min, [6] ratio_max
 *   [7] explained_variance_old  1 - Var(ret - vpred) / Var(ret)
 *   [8] explained_variance_new  1 - Var(ret - v_new) / Var(ret)
 *   [9] value_mse               mean((ret - v_new)^2)
 * Both variances are population variances, formed about the mean (a mean far from zero costs no digits); Var(ret) == 0 gives NaN
 * (or -inf), as numpy's expression does.  Two launches on the context's stream (a recurrent policy: the GRU forward over all N
 * environments and T steps with MASKS[:-1] first, from hidden slot 0 of a rollout that holds its hidden states
 * (sg_rollout_enable_hidden), else from hxs0_host[N*H], which is then required); sums in double, no atomics: the same call gives
 * the same bits.  Nothing of the rollout or the policy is written.  out10 == NULL: the launches are queued and the call returns
 * without a host wait; sg_rollout_policy_diagnostics_fetch waits for the LAST queued result and reads it, once -- with nothing
 * pending it is an error.  out10 != NULL is the two calls in one.
 *   - clip_param = INFINITY is accepted and gives a clip fraction of exactly 0 (A2C / ACKTR have no clip); zero, negative and NaN
 *     are errors.
 *   - with a communicator of world > 1 the statistics cover the rank's own columns; no collective is issued (scope "rank").
 * Policy, SplitPolicy, a Discrete / MultiBinary policy and a recurrent one are taken.  Errors, each with its own message: policy
 * and rollout on different contexts, dims that differ, a bad clip_param, a recurrent policy with neither hidden source, and a
 * policy with the CNN base. */
#define SG_DIAG_N 10
SG_API int sg_rollout_policy_diagnostics(sg_rollout *r, sg_policy *p, float clip_param, const float *hxs0_host, double *out10);
SG_API int sg_rollout_policy_diagnostics_fetch(sg_rollout *r, double out10[10]);
/* Scope "world": the same ten numbers over the union of all ranks' rows -- what one process computes on the concatenated
 * rollout, global column = rank * N + n -- and the same bits on every rank.  The rank's workgroup records are folded into one
 * 16-double record (plain sums, minimum / maximum, three (count, mean, M2) triples), the ranks' records are all-gathered in
 * float64, and every rank merges them in ascending rank order (Chan's formula for the triples, so the between-rank part of a
 * variance is kept) and finalises.  Arguments, queued form (out10 == NULL), fetch and errors are sg_rollout_policy_diagnostics's.
 *   - THIS CALL IS A COLLECTIVE: every rank issues it, at the same point of its stream's sequence of collectives (a rank that
 *     does not leaves its peers waiting in the all-gather).
 *   - no communicator, or one of world 1: the rank scope's bits.
 *   - the ranks' T*N must be equal (the global numbering assumes equal column shards).  If they differ the collective still
 *     completes, and sg_rollout_policy_diagnostics_fetch -- or this call with out10 != NULL -- returns an error with its own
 *     message on every rank instead of numbers. */
SG_API int sg_rollout_policy_diagnostics_world(sg_rollout *r, sg_policy *p, float clip_param, const float *hxs0_host, double *out10);

/* ---------------------------------------------------------------------- PPO */
typedef struct {
    float clip_param;
    int ppo_epoch;
    int num_mini_batch;
    float value_loss_coef;
    float entropy_coef;
    float lr;
    float eps;
    float max_grad_norm;
    int use_clipped_value_loss;
} sg_ppo_config;
/* PPO(actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr, eps,
 *     max_grad_norm, use_clipped_value_loss)  a2c/algo/ppo.py:30-63 (Adam state starts at zero). */
SG_API int sg_ppo_create(sg_ctx *ctx, sg_policy *p, const sg_ppo_config *cfg, sg_ppo **out);
SG_API int sg_ppo_destroy(sg_ppo *a);
/* optimizer.param_groups[i]['lr'] = lr  (a2c/utils.py:68-72 update_linear_schedule) */
SG_API int sg_ppo_set_lr(sg_ppo *a, float lr);
/* PPO.update(rollouts) a2c/algo/ppo.py:65-157 -> out3 = {value_loss, action_loss, dist_entropy}.
 * perms: [ppo_epoch][T*N] int64 = the permutation each epoch's sampler draws (a2c/storage.py:159-162) with n_perms =
 * its element count (checked, as is every index), or NULL (n_perms ignored) -> device-generated from `seed`.
 * With a communicator of world > 1 an injected permutation is the reference's draw at num_processes = world * N:
 * [ppo_epoch][T*N*world] ids in its numbering t*(N*world) + rank*N + n, the same array on every rank; each rank takes
 * the rows of every minibatch it owns (NULL: every rank permutes its own rows and gives T*N/num_mini_batch per step). */
SG_API int sg_ppo_update(sg_ppo *a, sg_rollout *r, const int64_t *perms, int64_t n_perms, uint64_t seed, float out3[3]);
/* out3 may be NULL (as for sg_disc_update_gail_dyn): the update is queued and the call returns without waiting for it.
 * An outer iteration made of such calls -- sg_disc_update_gail_dyn x gail_epoch, sg_disc_relabel_rewards_auto,
 * sg_rollout_compute_returns_policy, sg_ppo_update, sg_rollout_after_update -- never makes the host wait; its scalars (the
 * reference main's log line, a2c/main_gail_dyn_ppo.py:322-338) are published into one of SG_RESULT_SLOTS = 8 pinned
 * host slots by sg_results_publish (d and/or a may be NULL) and read with sg_results_fetch when the caller wants them:
 * out13 = {D loss sums x3 of the last epoch, ret_rms mean / var / count, sum(1 - masks), r_sa, PPO loss sums x3,
 * n_d, ppo_epoch * num_mini_batch}; losses = sums / their step count (float32, as the synchronous calls return them). */
SG_API int sg_results_publish(sg_ctx *ctx, sg_disc *d, sg_ppo *a, int slot);
SG_API int sg_results_fetch(sg_ctx *ctx, int slot, double out13[13]);
/* The permutations the last sg_ppo_update consumed ([ppo_epoch][T*N]; [ppo_epoch][N] for a recurrent policy: the environments of
 * every epoch; injected or library-drawn), so a run made
 * with the library's generator can be replayed elsewhere (the role torch.manual_seed plays for the reference). */
SG_API int sg_ppo_last_perms(sg_ppo *a, int64_t *perms, int64_t count);
/* Adam state access for checkpoint/parity: m, v flat [n] in state_dict order (a recurrent policy: the GRU's tensors first); *step = t. */
SG_API int sg_ppo_get_adam(sg_ppo *a, float *m, float *v, int64_t n, int64_t *step);
SG_API int sg_ppo_set_adam(sg_ppo *a, const float *m, const float *v, int64_t n, int64_t step);
/* PPO.update with a recurrent policy (kind SG_POLICY_GRU), a2c/algo/ppo.py:74-90 over RolloutStorage.recurrent_generator
 * a2c/storage.py:194-251: sg_ppo_update then takes whole environments per minibatch -- per = N // num_mini_batch of them, all T
 * steps each, N // per optimizer steps per epoch (more than num_mini_batch when per does not divide N into that many; the
 * returned losses are still divided by ppo_epoch * num_mini_batch, as the reference divides them; N % per != 0, where the
 * reference runs past its permutation, is an error) -- and back-propagates through the GRU scan.  perms is [ppo_epoch][N], the
 * torch.randperm(num_processes) of every epoch (sg_ppo_last_perms returns the same shape), or NULL.  The sequences start from
 * rollouts.recurrent_hidden_states[0] (a2c/storage.py:216-217) and use masks[:-1]: the rollout's MASKS field must be current,
 * and the states of slot 0, hxs0[N*H], are handed over with this call before EVERY update (the device rollout has no
 * hidden-state field unless sg_rollout_enable_hidden gave it one: sg_ppo_set_hidden_states_rollout then).  One rank only; sg_ppo_set_symmetry refuses a recurrent policy. */
SG_API int sg_ppo_set_hidden_states(sg_ppo *a, const float *hxs0, int64_t count);
/* The same hand-over from a rollout that holds its hidden states (sg_rollout_enable_hidden, of the policy's width): slot 0 is
 * copied device to device on the stream; the host reads no state and does not wait.  Before every update, like the call above. */
SG_API int sg_ppo_set_hidden_states_rollout(sg_ppo *a, sg_rollout *r);
/* Mirror-symmetry loss of PPO.update, a2c/algo/ppo.py:110-143 (a2c/main.py:133-146, --loss-sym): every optimizer step adds
 * coef * mean((M_a mu(s) - mu(mirror_obs(s)))^2) over the minibatch's B x A elements, mu = the DiagGaussian mean (fc_mean);
 * M_a mu(s) is a constant of the loss (the reference mirrors it through numpy), so its gradient reaches the actor trunk and
 * fc_mean through the mirrored pass mu(mirror_obs(s)) only, never the critic or the log-std.  Policy (MLP)
 * only.  coef == 0 turns it off (plain PPO, today's kernels).  m_act [A*A] (required when coef > 0) and m_obs [O*O] are
 * row-major linear maps: mirrored = M x.  m_obs NULL: the caller mirrors the rollout's observations itself and hands them
 * over with sg_ppo_set_mirrored_obs before every update (the reference's per-row callable, my_pybullet_envs/utils.py:334-357). */
SG_API int sg_ppo_set_symmetry(sg_ppo *a, float coef, const float *m_obs, const float *m_act);
/* host[T*N*O] = mirror_obs(obs[t, n]) for the first T rollout steps, row t*N + n; consumed by the next sg_ppo_update */
SG_API int sg_ppo_set_mirrored_obs(sg_ppo *a, const float *host, int64_t count);
/* the last update's symmetry_loss.item() averaged over its ppo_epoch * num_mini_batch steps (0 when the loss is off) */
SG_API int sg_ppo_last_symmetry_loss(sg_ppo *a, float *out);

/* ---------------------------------------------------------------------- A2C */
typedef struct {
    float value_loss_coef;
    float entropy_coef;
    float lr;
    float eps;
    float alpha;
    float max_grad_norm;
} sg_a2c_config;
/* A2C_ACKTR(actor_critic, value_loss_coef, entropy_coef, lr, eps, alpha, max_grad_norm, acktr=False)  a2c/algo/a2c_acktr.py:30-51,
 * built by a2c/main.py:123-131 (--algo a2c): RMSprop(lr, eps, alpha; centered False, momentum 0), square_avg starting at zero.
 * The handle is an sg_ppo in A2C mode: sg_ppo_update (perms == NULL only; out3 == NULL queues it), sg_ppo_set_lr, sg_ppo_destroy
 * and sg_results_publish (step count 1) take it; sg_ppo_get_adam / sg_ppo_set_adam / sg_ppo_set_symmetry /
 * sg_ppo_set_mirrored_obs refuse it.  Refused here: SplitPolicy, and a context with a communicator of world > 1.
 * One update (a2c/algo/a2c_acktr.py:52-102): evaluate_actions on all T*N rollout rows with the current parameters,
 * adv = returns[:-1] - values, out3 = {mean(adv^2), -mean(adv.detach() * logp), mean(entropy)}, loss = out3[0] * vcoef +
 * out3[1] - out3[2] * ecoef, clip_grad_norm_(max_grad_norm), one RMSprop step. */
SG_API int sg_a2c_create(sg_ctx *ctx, sg_policy *p, const sg_a2c_config *cfg, sg_ppo **out);
/* The same learner on a recurrent policy (kind SG_POLICY_GRU; --algo a2c --recurrent-policy): A2C through time.  Opt-in by entry
 * point: sg_a2c_create keeps refusing a recurrent policy.  Refused here, each with its own message: a feed-forward policy, a head
 * other than the Gaussian one, and a context with a communicator of world > 1.
 * One update (a2c/algo/a2c_acktr.py:55-102 with a2c/model.py:117-201): evaluate_actions on the rollout's T*N rows in their own
 * order t*N + n, the GRU stepped with h <- h * masks[t] from the hidden states of slot 0, which the caller hands over before
 * EVERY update with sg_ppo_set_hidden_states or sg_ppo_set_hidden_states_rollout (as for PPO through time); the losses and out3
 * as above, all means over T*N rows; back-propagation through the heads and through time (no gradient for h_0 or the
 * observations); clip_grad_norm_ over ALL parameters, the GRU's included; one RMSprop step over all of them.  The environments
 * go through the scans in groups of at most 65,536 rows (whole multiples of 16 environments; SG_A2C_GROUP_ENVS=<multiple of 16>
 * forces a smaller group: test knob), so the scratch does not grow with N.  sg_a2c_get_rmsprop / sg_a2c_set_rmsprop cover the
 * GRU's tensors, which come first in state_dict order. */
SG_API int sg_a2c_create_rnn(sg_ctx *ctx, sg_policy *p, const sg_a2c_config *cfg, sg_ppo **out);
/* The same learner on the CNN base (sg_policy_create_cnn; --algo a2c on image observations, the reference's default pairing):
 * a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:204-230.  Opt-in by entry point: sg_a2c_create keeps refusing a CNN policy.
 * Refused here, each with its own message: a policy without the CNN base, and a context with a communicator of world > 1.
 * One update: evaluate_actions on the rollout's T*N rows in their own order, the losses and out3 as above, all means over T*N
 * rows; clip_grad_norm_ over all parameters, one RMSprop step (the learning rate of sg_ppo_set_lr).  The rows go through the
 * network in chunks of at most 4096 (SG_A2C_CNN_CHUNK_ROWS=<n >= 1> forces a smaller chunk: test and tuning knob), each
 * chunk's gradient added to that of the chunks before it in a fixed order, so the scratch (167 KB per chunk row) does not grow
 * with T*N, no rollout size is refused below 2^30 rows, and two runs are bit-identical.  sg_a2c_get_rmsprop / sg_a2c_set_rmsprop
 * take square_avg in the CNN's flat order (sg_policy_create_cnn). */
SG_API int sg_a2c_create_cnn(sg_ctx *ctx, sg_policy *p, const sg_a2c_config *cfg, sg_ppo **out);
/* The same learner on the recurrent CNN base (sg_policy_create_cnn_rnn; --algo a2c --recurrent-policy on image observations):
 * a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:117-230, A2C through time on images.  Opt-in by entry point: sg_a2c_create,
 * sg_a2c_create_rnn and sg_a2c_create_cnn keep refusing that base.  Refused here, each with its own message: a policy that is not
 * sg_policy_create_cnn_rnn's, and a context with a communicator of world > 1.
 * One update: evaluate_actions on the rollout's T*N rows -- the trunk on every frame, the GRU stepped with h <- h * masks[t] from
 * the hidden states of slot 0, which the caller hands over before EVERY update with sg_ppo_set_hidden_states ([N][hidden]; a
 * missing hand-over is refused; sg_rollout_enable_hidden keeps refusing image rollouts) --, the losses and out3 as above, all
 * means over T*N rows; back-propagation through the heads, through time and through the trunk; ONE clip_grad_norm_ over the CNN
 * and GRU parameters together, one RMSprop step over both (the learning rate of sg_ppo_set_lr).  The rows go through the network
 * in groups of max(1, min(N, 4096 / T)) whole environments with all T steps, time-major, read in place from the rollout
 * (SG_A2C_CNN_GRU_GROUP_ENVS=<n >= 1> forces a smaller group: test and tuning knob); each group's gradient is added to that of
 * the groups before it in a fixed order, so the scratch (167 KB per group row) does not grow with N and two runs are
 * bit-identical.  T > 4096 is refused by sg_ppo_update.  perms must be NULL; out3 == NULL queues the update.  sg_ppo_set_lr,
 * sg_ppo_destroy and sg_results_publish take the handle; sg_a2c_get_rmsprop / sg_a2c_set_rmsprop take square_avg in flat
 * state_dict order: the GRU's four tensors first, then the CNN's flat order (sg_policy_create_cnn_rnn). */
SG_API int sg_a2c_create_cnn_rnn(sg_ctx *ctx, sg_policy *p, const sg_a2c_config *cfg, sg_ppo **out);
/* RMSprop state for checkpoint/parity: square_avg flat [n] in state_dict order; *step = optimizer steps taken. */
SG_API int sg_a2c_get_rmsprop(sg_ppo *a, float *square_avg, int64_t n, int64_t *step);
SG_API int sg_a2c_set_rmsprop(sg_ppo *a, const float *square_avg, int64_t n, int64_t step);

/* -------------------------------------------------------------------- ACKTR */
typedef struct {
    float value_loss_coef;
    float entropy_coef;
    float lr;            /* KFACOptimizer(lr=0.25): the SGD step is lr * (1 - momentum), kl_clip bounds it through lr^2 */
    float momentum;      /* 0.9 */
    float stat_decay;    /* 0.99 */
    float kl_clip;       /* 0.001 */
    float damping;       /* 1e-2 */
    int Tf;              /* 10: eigendecompositions every Tf updates */
} sg_acktr_config;
/* A2C_ACKTR(actor_critic, value_loss_coef, entropy_coef, acktr=True)  a2c/algo/a2c_acktr.py:30-51, built by a2c/main.py:159-161
 * (--algo acktr) with KFACOptimizer(actor_critic) a2c/algo/kfac.py:97-150 (weight_decay 0, Ts 1; the constructor values
 * above).  The handle is an sg_ppo in ACKTR mode: sg_ppo_update (perms == NULL only; out3 == NULL queues it; seed keys the
 * library's own value noise), sg_ppo_destroy and sg_results_publish (step count 1) take it; sg_ppo_get_adam / sg_ppo_set_adam /
 * sg_a2c_get_rmsprop / sg_a2c_set_rmsprop / sg_ppo_set_symmetry / sg_ppo_set_mirrored_obs refuse it; sg_ppo_set_lr is accepted
 * and read by nothing (KFACOptimizer.step never reads its param_groups).  Refused here: SplitPolicy, and a context with a
 * communicator of world > 1.
 * One update (a2c/algo/a2c_acktr.py:52-102, kfac.py:152-255): A2C's loss and gradient over all T*N rows (no clip); the sampled
 * Fisher loss -mean(logp) - mean((v - (v + eps).detach())^2) back-propagated for the Kronecker factors A = a^T a / B and
 * G = B g^T g of the 13 K-FAC modules (split_bias: every Linear weight and bias, dist.logstd), folded into running averages;
 * symeig of the factors when steps % Tf == 0; v = Q_g ((Q_g^T grad Q_a) / (d_g d_a^T + damping)) Q_a^T;
 * nu = min(1, sqrt(kl_clip / sum(v grad lr^2))); SGD(lr (1 - momentum), momentum) on nu v; steps += 1.
 * If the eigensolver hits its sweep cap, a fetching call fails (the losses come back with the error); a queued update
 * (out3 == NULL) reports it through sg_results_fetch of the slot sg_results_publish filled for it, and so does every later
 * one, since the word stays raised. */
SG_API int sg_acktr_create(sg_ctx *ctx, sg_policy *p, const sg_acktr_config *cfg, sg_ppo **out);
/* eps [n] float32, n = T*N in rollout order: torch.randn(values.size()) of a2c/algo/a2c_acktr.py:82 for the NEXT update only;
 * NULL: the library draws its own (keyed on sg_ppo_update's seed, the update index and the row). */
SG_API int sg_acktr_set_value_noise(sg_ppo *a, const float *eps, int64_t n);
/* K-FAC state (kfac.py:131-133, 148): m_aa / m_gg of the 13 modules in module (= state_dict) order, each [in][in] / [out][out]
 * row-major and packed back to back (a bias module's m_aa is [[1]]; n_aa / n_gg must be the packed sizes); SGD's momentum
 * buffer flat [n] in state_dict order (zero before the first update); *steps = KFACOptimizer.steps. */
SG_API int sg_acktr_get_state(sg_ppo *a, float *m_aa, int64_t n_aa, float *m_gg, int64_t n_gg, float *momentum_buf, int64_t n,
                              int64_t *steps);

/* ------------------------------------------------------------ discriminator */
/* Discriminator(input_dim, hidden_dim, device) a2c/algo/gail.py:35-51; Adam(lr 1e-3, eps 1e-8). */
SG_API int sg_disc_create(sg_ctx *ctx, int input_dim, int hidden_dim, sg_disc **out);
SG_API int sg_disc_destroy(sg_disc *d);
SG_API int sg_disc_num_params(const sg_disc *d, int64_t *n);
SG_API int sg_disc_set_params(sg_disc *d, const float *flat, int64_t n);
SG_API int sg_disc_get_params(sg_disc *d, float *flat, int64_t n);
SG_API int sg_disc_get_adam(sg_disc *d, float *m, float *v, int64_t n, int64_t *step);
SG_API int sg_disc_set_adam(sg_disc *d, const float *m, const float *v, int64_t n, int64_t step);
/* The expert matrix [n_rows, input_dim] (a2c/main_gail_dyn_ppo.py:163-165) stays resident in HBM. */
SG_API int sg_disc_set_expert(sg_disc *d, const float *expert, int64_t n_rows);
/* Discriminator.update_gail_dyn(expert_loader, rollouts) a2c/algo/gail.py:154-193, one epoch.
 * batch_size = expert_loader.batch_size; n_d = min(n_expert/batch, T*N/batch) steps.
 * expert_perm[n_expert] (DataLoader shuffle), policy_perm[T*N] (feed_forward_generator),
 * alpha[n_d*batch] (torch.rand per step, a2c/algo/gail.py:72) -- each may be NULL -> `seed`; each comes with its
 * element count (n_expert_perm == n_expert, n_policy_perm == rows the permutation ranges over, n_alpha >= n_d*batch;
 * ignored for a NULL pointer), and lengths and index ranges are checked before anything is copied to the device.
 * With a communicator of world > 1 the injected policy_perm is the reference's draw at num_processes = world*N
 * ([T*N*world] ids in its numbering t*(N*world) + rank*N + n), the same arrays on every rank, in both data-parallel
 * modes; n_d = min(n_expert/batch, T*N*world/batch).  Sharded mode takes the three arrays together or none.
 * out3 = {mean(gail_loss+grad_pen), mean expert_loss, mean policy_loss}; *n_steps = n_d.  out3 may be NULL when the caller
 * has no use for this epoch's losses (the reference's main keeps only the last epoch's, a2c/main_gail_dyn_ppo.py:255-256):
 * the call then returns as soon as the epoch is queued instead of waiting for it.
 * n_expert < batch_size is an error (the reference raises on the size mismatch). */
SG_API int sg_disc_update_gail_dyn(sg_disc *d, sg_rollout *r, int batch_size, const int64_t *expert_perm, int64_t n_expert_perm,
                            const int64_t *policy_perm, int64_t n_policy_perm, const float *alpha, int64_t n_alpha,
                            uint64_t seed, float out3[3], int *n_steps);
/* Discriminator.update(expert_loader, rollouts, obsfilt, is_gail_dyn, a_dim) a2c/algo/gail.py:91-152, one
 * epoch: the same step on caller-assembled policy rows [n_rows, input_dim] (host): (state | action)
 * rows for classic GAIL, (obs_feat | action | next_obs_feat) for is_gail_dyn (a2c/algo/gail.py:102-109).
 * The expert matrix (sg_disc_set_expert) is assembled the same way.  Other arguments as above;
 * policy_perm ranges over n_rows (x world with a communicator).  n_cols = environment columns per time slot when the
 * rows are a rollout's (t, n) grid (needed to number the union of the ranks' rows as the reference would at
 * num_processes = world*N), 0 = unstructured rows (the union is numbered rank after rank). */
SG_API int sg_disc_update_rows(sg_disc *d, const float *policy_rows, int64_t n_rows, int n_cols, int batch_size,
                        const int64_t *expert_perm, int64_t n_expert_perm, const int64_t *policy_perm, int64_t n_policy_perm,
                        const float *alpha, int64_t n_alpha, uint64_t seed, float out3[3], int *n_steps);
/* Discriminator.predict_reward_combined(d_in, gamma, masks, offset) a2c/algo/gail.py:201-210.
 * x[n,F], masks[n] -> reward[n], returns[n]; Discriminator.returns persists inside the handle
 * (first call: returns = reward).  n must stay the same across calls. */
SG_API int sg_disc_predict_reward(sg_disc *d, const float *x, int n, float gamma, const float *masks,
                           float offset, float *reward, float *returns);
/* Discriminator.predict_prob_single_step(s, a, s_n) a2c/algo/gail.py:212-217: prob[n] = sigmoid(D(x)) on the
 * caller-concatenated rows x[n,F]. */
/* The T consecutive predict_reward_combined calls of the reference main's relabel loop (a2c/main_gail_dyn_ppo.py:275-280:
 * call t passes obs_feat[t + 1], masks[t]) in ONE pass over the rollout's device copy of obs_feat and masks: reward[t*N + n] and
 * returns[t*N + n] are bit for bit what the t-th sg_disc_predict_reward call returns, Discriminator.returns (a2c/algo/gail.py:206-209)
 * is left where the T-th call leaves it.  The host mirror (simgan_amd/algo/gail.py) uses it to serve the unchanged main's 128 calls
 * from one launch; the rollout's fields must be current on the device (sg_rollout_upload). */
SG_API int sg_disc_predict_reward_steps(sg_disc *d, sg_rollout *r, float gamma, float offset, float *reward, float *returns);
SG_API int sg_disc_predict_prob(sg_disc *d, const float *x, int n, float *prob);
/* Discriminator.compute_grad_pen_combined(expert_combined, policy_combined, lambda_) a2c/algo/gail.py:67-89 (and
 * compute_grad_pen :53-65 on caller-concatenated rows), the VALUE only: pen[i] = (||dD/dx(alpha_i e_i + (1 - alpha_i) p_i)||_2 - 1)^2
 * for the n row pairs expert_rows[n,F] / policy_rows[n,F]; the reference's scalar is lambda_ * mean(pen).  alpha[n] is the
 * reference's torch.rand(n, 1) draw (:72), NULL -> the library's generator with `seed`.  The differentiable term the reference adds
 * to its loss is formed inside the update kernels (sg_disc_update_gail_dyn / _rows); this call changes no state. */
SG_API int sg_disc_grad_pen(sg_disc *d, const float *expert_rows, const float *policy_rows, const float *alpha, int n,
                     uint64_t seed, float *pen);
/* The draws the last update epoch consumed: expert_perm[n_expert], policy_perm[n_policy_rows], alpha[n_alpha]
 * (injected or library-drawn); each pointer may be NULL, each count must match the epoch's size (returned in
 * counts3 = {n_expert, n_policy_rows, n_alpha} when counts3 != NULL). */
SG_API int sg_disc_last_draws(sg_disc *d, int64_t *expert_perm, int64_t *policy_perm, float *alpha, int64_t counts3[3]);
SG_API int sg_disc_reset_returns(sg_disc *d);
SG_API int sg_disc_get_returns(sg_disc *d, float *returns, int n, int *is_none);
SG_API int sg_disc_set_returns(sg_disc *d, const float *returns, int n);
/* Fused reward relabel, all T steps on device: a2c/main_gail_dyn_ppo.py:275-292
 *   for t: rewards[t], ret = predict_reward_combined(obs_feat[t+1], gamma, masks[t], offset)
 *          ret_rms.update(ret); rewards[t] = clip(rewards[t]/sqrt(ret_rms.var+1e-7), -10, 10)
 * rms_state = {mean, var, count} float64 (RunningMeanStd, a2c/baselines/common/running_mean_std.py:27-58),
 * updated in place.  Writes rollout field REWARDS. */
SG_API int sg_disc_relabel_rewards(sg_disc *d, sg_rollout *r, float gamma, float offset,
                            double rms_state[3]);
/* The same with the alive-bonus offset computed on the device as well (a2c/main_gail_dyn_ppo.py:258-271: r_sa from
 * sum(1 - masks), num_processes (all ranks), num_steps and gail_tar_length; no_alive_bonus != 0 -> 0) and ret_rms kept inside
 * the handle (initially RunningMeanStd(): {0, 1, 1e-4}): nothing is read back, the call only queues work.
 * sg_disc_set_rms overwrites the resident state; sg_disc_get_scalars reads {mean, var, count, sum(1 - masks), r_sa}. */
SG_API int sg_disc_relabel_rewards_auto(sg_disc *d, sg_rollout *r, float gamma, double gail_tar_length, int no_alive_bonus);
SG_API int sg_disc_set_rms(sg_disc *d, const double rms_state[3]);
SG_API int sg_disc_get_scalars(sg_disc *d, double out5[5]);
/* Discriminator diagnostics on the device: what one looks at in the discriminator half of the GAIL-dyn loop, over three row
 * populations in two queued launches -- policy: the T*N rows of OBS_FEAT[1:] (the rows sg_disc_update_gail_dyn trains on and
 * the relabel scores); expert: the n_e rows of sg_disc_set_expert; mid: the T*N rows 0.5f * expert[i mod n_e] + 0.5f * policy[i],
 * the reference's mixup (a2c/algo/gail.py:72-75) at alpha = 0.5, formed on the fly.  Replaces a download of obs_feat,
 * predict_prob on every row, sg_disc_grad_pen on the mixed rows and numpy.  With d the logit D(x), s = sigmoid(d), g = dD/dx
 * and |g| its 2-norm per row, out19 = SG_DDIAG_N doubles:
 *   [0]  policy_rows            T*N                        [1]  expert_rows            n_e
 *   [2]  policy_accuracy        mean(d_p < 0)              [3]  expert_accuracy        mean(d_e > 0)      (d == 0 is wrong for both)
 *   [4]  policy_logit_mean                                 [5]  policy_logit_std       population standard deviation
 *   [6]  expert_logit_mean                                 [7]  expert_logit_std
 *   [8]  policy_bce             mean softplus(d_p)         [9]  expert_bce             mean softplus(-d_e)
 *   [10] reward_mean  [11] reward_std  [12] reward_min  [13] reward_max    over the policy rows, of log(s + 1e-7) - log(1 - s + 1e-7)
 *                               (1e-7 at its float32 value): the raw reward of sg_disc_predict_reward, no offset, before ret_rms
 *   [14] policy_grad_norm_mean  [15] expert_grad_norm_mean  [16] mid_grad_norm_mean     mean |g| over each population
 *   [17] mid_grad_pen           10 mean((|g| - 1)^2) over the mid rows
 *   [18] grad_norm_max          over all three populations
 * Forward and input gradient in float32 on the matrix cores (the forward is sg_disc_predict_reward's), sums in double, no
 * atomics, records merged in a fixed order: the same call gives the same bits.  Nothing of the discriminator, the rollout or the
 * expert matrix is written.  slot is 0 or 1: two results may be pending at once (before and after the discriminator epochs).
 * out19 == NULL: the launches are queued and the call returns without a host wait; sg_disc_diagnostics_fetch waits for the LAST
 * result queued into the slot and reads it, once -- with nothing pending in the slot it is an error.  out19 != NULL is the two
 * calls in one.  The rollout's OBS_FEAT must be current on the device (sg_rollout_upload).
 * With world > 1 or a sharded discriminator the numbers cover THIS rank's own rollout rows and the expert rows it holds: no
 * collective is issued (scope "rank").
 * Errors, each with its own message: NULL argument, slot out of range, discriminator and rollout on different contexts, rollout
 * feat_len != input_dim, no expert set. */
#define SG_DDIAG_N 19
SG_API int sg_disc_diagnostics(sg_disc *d, sg_rollout *r, int slot, double *out19);
SG_API int sg_disc_diagnostics_fetch(sg_disc *d, int slot, double out19[SG_DDIAG_N]);
/* Scope "world": the same nineteen numbers over the union of all ranks' rollout rows -- what one process computes on the
 * concatenated rollout -- and the same bits on every rank, in both discriminator data-parallel modes (sg_ctx_set_disc_dp 0 and
 * 1).  Per population: the policy and mid parts of the ranks' folded 36-double records are merged in ascending rank order after
 * a float64 all-gather; every rank holds the whole expert matrix, so the expert part is rank 0's, not a merge, and expert_rows
 * is n_e.  Mid row (t, n) of rank k is paired with expert[(t * world * N + k * N + n) mod n_e], the pairing of its row number in
 * the concatenated rollout.  Slots, queued form, fetch and errors are sg_disc_diagnostics's, and world * T*N < 2^31.
 *   - THIS CALL IS A COLLECTIVE: every rank issues it, at the same point of its stream's sequence of collectives.
 *   - no communicator, or one of world 1: the rank scope's bits.
 *   - the ranks' T*N must be equal, and so must their n_e.  If either differs the collective still completes, and
 *     sg_disc_diagnostics_fetch -- or this call with out19 != NULL -- returns an error with its own message on every rank
 *     instead of numbers. */
SG_API int sg_disc_diagnostics_world(sg_disc *d, sg_rollout *r, int slot, double *out19);
/* sum(1 - masks) over all T+1 slots (a2c/main_gail_dyn_ppo.py:258), for the alive-bonus offset. */
SG_API int sg_rollout_count_dones(sg_rollout *r, double *dones);

/* Page-locked host memory for buffers that cross the boundary every update (the rollout's host tensors: a2c/storage.py:37-53
 * allocates them with torch.zeros and `.to(device)` moves them, :57-68; here they stay on the host and sg_rollout_upload /
 * _download move their content).  From such memory a field crosses PCIe as one DMA at the link's speed; from pageable
 * memory the same calls work, through the runtime's staging path.  No context needed. */
SG_API int sg_host_alloc(int64_t bytes, void **out);
SG_API int sg_host_free(void *p);

/* ------------------------------------------------------------- measurement */
/* HIP-event timing of the dominant kernels on the library's stream since the last reset:
 * which = 0 k_disc_chain (discriminator step, serial part), 1 k_disc_wgrad (weight gradients + Adam),
 * 2 k_ppo_fwd, 3 k_ppo_bwd, 4 k_ppo_reduce, 5 relabel forward, 6 k_ppo_adam (clip + Adam), 7 k_disc_step4 (the one-launch
 * discriminator step), 8 the per-step float32 gradient all-reduce (N > 1: RCCL, loopback or the peer mesh, whichever runs).
 * Enabled by sg_ctx_profile(ctx, 1); adds start/stop events to every launch (do not enable inside
 * the timed bench region). */
SG_API int sg_ctx_profile(sg_ctx *ctx, int enable);
SG_API int sg_ctx_profile_read(sg_ctx *ctx, int which, double *total_ms, int64_t *launches);
SG_API int sg_ctx_profile_reset(sg_ctx *ctx);
/* A timestamp on the library's stream, taken by the device when it gets there (one HIP event; the host does not wait):
 * *id = the mark's number.  bench.py brackets every timed update with one and reads the per-update spread after the loop --
 * the reference times its updates with time.time() around the same calls (a2c/main_gail_dyn_ppo.py:318-321).
 * id = NULL: synchronise and forget every mark. */
SG_API int sg_ctx_mark(sg_ctx *ctx, int *id);
/* Milliseconds between two marks (waits for mark `to`). */
SG_API int sg_ctx_mark_elapsed(sg_ctx *ctx, int from, int to, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* SIMGAN_HIP_H */
