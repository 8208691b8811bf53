// sg_ppo.hip -- PPO.update on gfx950: advantage normalisation, then per optimizer step the
// clipped-surrogate / clipped-value / entropy loss, its gradient, global-norm clipping and Adam.
//
// Replaces (reference, a2c/ = third_party/a2c_ppo_acktr/): PPO.__init__/update a2c/algo/ppo.py:29-157,
// the minibatch gather of RolloutStorage.feed_forward_generator a2c/storage.py:144-192 and
// nn.utils.clip_grad_norm_ + optim.Adam (a2c/algo/ppo.py:143-145).  Kernels: sg_ppo_kernels.hpp.
//
// Launch sequence of one update (all on the library's stream, one host synchronisation at the end):
//   k_adv_stats x3                                   advantages, global mean / unbiased std
//   per epoch:   k_ppo_epoch_gather                  permuted copy of the rollout
//   per step:    k_ppo_fwd -> k_ppo_bwd -> k_ppo_reduce [-> all-reduce -> k_sumsq] -> k_ppo_adam
//   then         k_opt_commit                        Adam's step base += E*M
// With the mirror-symmetry loss (sg_ppo_set_symmetry) the rollout's mirrored observations are formed first (k_mirror_rows, or
// uploaded by the host), the epoch gather permutes them too and every step runs k_ppo_fwd_sym -> k_ppo_bwd_sym ->
// k_ppo_reduce_sym -> k_ppo_adam_sym: the two-launch form with a third grid column, the actor trunk on the mirrored rows.
// Everything from the first epoch gather on is captured into a hipGraph once and replayed per update (single GPU;
// with a communicator the RCCL calls are issued directly between the kernels).
//
// A2C (sg_a2c_create: a mode of the same object, a2c/algo/a2c_acktr.py:30-102 with acktr=False), one update:
//   k_a2c_gather                                    the rollout's T*N rows in their own order (no permutation, no advantages)
//   per chunk of <= SG_A2C_CHUNK_ROWS rows:  k_ppo_fwd -> k_a2c_bwd -> k_a2c_reduce (adds to the gradient)
//   then         k_a2c_rmsprop                      clip + RMSprop, the update's one optimizer step
//
// A2C through time (sg_a2c_create_rnn: the same learner on a recurrent Policy; a2c_gru_update), per group of environments:
//   k_a2c_gru_gather -> k_gru_inproj -> k_gru_scan_fwd<TRAIN>;  per chunk:  k_ppo_fwd -> k_a2c_bwd_dx -> k_a2c_reduce;
//   k_gru_scan_bwd -> k_gru_wgrad -> k_gru_reduce_acc;  then one k_a2c_rmsprop over heads + GRU
//
// A recurrent Policy with a Categorical / Bernoulli head (sg_policy_create_rnn_dist) runs both sequences through time
// with the head kernels k_ppo_bwd_dist_dx / k_a2c_bwd_dist_dx: the Categorical / Bernoulli loss block followed by the d loss / d h_t
// epilogue of both trunks.
//
// A2C on the CNN base (sg_a2c_create_cnn; a2c_cnn_update), per chunk of <= SG_A2C_CNN_CHUNK_ROWS rows:
//   the forward of sg_cnn.hip -> k_cnn_head_loss_a2c -> head, FC, conv3, conv2, conv1 gradients (adding from the second chunk on);
//   then k_sumsq -> k_a2c_rmsprop
//
// A2C through time on the recurrent CNN base (sg_a2c_create_cnn_rnn; a2c_cnn_gru_update), per group of whole
// environments:  k_cnn_gru_index_group -> the trunk's forward -> k_gru_pad_rows -> k_gru_inproj -> k_gru_scan_fwd<TRAIN> -> the heads
//   on h_t -> k_cnn_head_loss_a2c_idx -> k_cnn_head_dh -> k_cnn_head_wgrad -> k_gru_scan_bwd -> k_gru_wgrad -> k_gru_reduce_acc ->
//   k_gru_dx -> the trunk's backward (every gradient adding from the second group on);  then k_sumsq -> k_a2c_rmsprop over both blocks
//
// ACKTR (sg_acktr_create: A2C's gradient with the K-FAC step of a2c/algo/kfac.py, sg_kfac.hpp), one update:
//   k_a2c_gather
//   per chunk:  k_ppo_fwd -> k_a2c_bwd -> k_a2c_reduce -> k_acktr_fisher -> k_kfac_stats (adds to the factor sums)
//   then        k_kfac_fold -> k_kfac_eig (exits unless steps % Tf == 0) -> k_kfac_gemm x4 -> k_kfac_step -> k_kfac_tick
// (its host-side state: sg_kfac_host.hpp)
//
// The file reads: launch helpers and kernel-instance tables, API, A2C / ACKTR, PPO through time, PPO, results ring.  The three
// updates stay three functions; what they share lies underneath them: ensure_cap (growing a scratch buffer), sg_graph_run (the
// capture / replay cache; each update builds its own key and its own "may I use a graph"), both in sg_common.h, and here
// ppo_bwd_tiles_lds, ppo_row_tiles, ppo_launch, enqueue_adv_stats and clear_for_layout.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "sg_common.h"
#include "sg_rng.hpp"
#include "sg_ppo_kernels.hpp"
#include "sg_kfac_host.hpp"
#include "sg_gru_kernels.hpp"

__global__ void k_fill_perm(int64_t* perm, int64_t n, int half_bits, uint64_t key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) perm[i] = sg_perm_at(i, n, half_bits, key);
}

int sg_fill_perm(sg_ctx* ctx, int64_t* d_perm, int64_t n, uint64_t seed, uint64_t stream_id) {
    const uint64_t key = sg_key(seed, 0x5045524Dull, stream_id);
    hipLaunchKernelGGL(k_fill_perm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_perm, n,
                       sg_perm_half_bits((uint64_t)n), key);
    SG_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------- launch
static int max_trunk_floats(const SgPolicyDesc& d) {
    int m = 0;
    for (int t = 0; t < d.n_trunks; ++t) m = d.trunk[t].size > m ? d.trunk[t].size : m;
    return m;
}
static int max_bwd_floats(const SgPolicyDesc& d) {
    int m = 0;
    for (int t = 0; t < d.n_trunks; ++t) { const int s = d.trunk[t].size - d.trunk[t].w2; m = s > m ? s : m; }
    return m;
}
static int stack_ldP(const SgPolicyDesc& d) {
    int m = 0;
    for (int t = 0; t < d.n_trunks; ++t) m = d.trunk[t].ldP > m ? d.trunk[t].ldP : m;
    return m;
}
// gw: the global-weight instances (trunks larger than a CU's LDS, sg_policy_needs_gw): LDS holds the row tiles only
static size_t ppo_fwd_lds(const SgPolicyDesc& d, int MT, bool gw) {
    const int R = 16 * MT;
    return sizeof(float) * ((gw ? 0 : (size_t)max_trunk_floats(d)) + R * d.ldO + 2 * R * d.ldH);
}
// LDS bytes of every kernel built on sg_ppo_bwd_body (k_ppo_bwd, k_ppo_bwd_sym, k_a2c_bwd, k_ppo_pair, k_ppo_fwd_critic).  It
// MIRRORS the carve-up at the head of sg_ppo_bwd_body (sg_ppo_kernels.hpp): Wimg | X H1 H2 | O0 O1 [OM] | ACT | SC[4][R]
// ROWL[2][R] VALID[R] | [MA] -- change the two together.
//   w_floats  the weight image in front of the tiles: 0 (global-weight instances), the whole trunk (max_trunk_floats: the
//             fused forms recompute the forward) or the trunk from w2 on (max_bwd_floats: the two-launch backward)
//   n_out     [R][ldP] head-output tiles: 2, or 3 with the other actor column's (k_ppo_bwd_sym)
//   ma        the [A][A] action mirror M_a behind everything (k_ppo_bwd_sym)
static size_t ppo_bwd_tiles_lds(const SgPolicyDesc& d, int MT, size_t w_floats, int n_out, bool ma) {
    const int R = 16 * MT;
    return sizeof(float) * (w_floats + R * d.ldO + 2 * R * d.ldH + (size_t)n_out * R * stack_ldP(d) + ((R * d.A + 3) & ~3) + 7 * R +
                            (ma ? (d.A * d.A + 3) & ~3 : 0));
}
// (a Categorical / Bernoulli policy has the fused form only -- LDS-resident or global-weight: SG_PPO_FUSED does not apply)
static bool ppo_fused(const SgPolicyDesc& d, int MT) {
    return d.kind == SG_POLICY_MLP && MT <= 2 && (d.dist != SG_DIST_GAUSSIAN || !sg_env_is_off("SG_PPO_FUSED"));
}
// rows of the rollout one A2C forward / backward / reduce pass covers: the slabs and row stacks are sized for this many rows
// whatever T*N is (the north-star PPO minibatch: 65,536 rows / 16)
#define SG_A2C_CHUNK_ROWS 4096

// Row-group size of a step on `mb` rows and `ncols` grid columns, in 16-row tiles.  32-row groups as long as they still give
// every CU a workgroup (half the gradient slabs for k_ppo_reduce to stream: -1.8 us per step at the north-star shape against
// +0.6 us in k_ppo_bwd), or (slab_rule) when the 16-row slabs would exceed 24 MB; otherwise 16-row groups (more workgroups in
// flight hide the phases' latencies).  SG_PPO_ROWS (tuning knob) overrides with 16, 32 or 64 rows as far as the mode has
// instances for them: env_max_mt tiles, 0 = the mode does not read the knob.  Then at most cap_mt, then halved until fits(MT).
template <typename Fits>
static int ppo_row_tiles(const sg_ctx* ctx, const SgPolicyDesc& d, int mb, int ncols, bool slab_rule, int env_max_mt, int cap_mt, Fits&& fits) {
    int MT = ((slab_rule && (size_t)((mb + 15) / 16) * (size_t)(d.total + 8) * sizeof(float) > ((size_t)24 << 20)) ||
              ((mb + 31) / 32) * ncols >= ctx->num_cu) ? 2 : 1;
    if (const char* e = env_max_mt ? getenv("SG_PPO_ROWS") : nullptr) {
        const int v = atoi(e);
        if ((v == 16 || v == 32 || v == 64) && v / 16 <= env_max_mt) MT = v / 16;
    }
    if (MT > cap_mt) MT = cap_mt;
    while (MT > 1 && !fits(MT)) MT /= 2;
    return MT;
}

// 8 waves once a workgroup has two row tiles to deal out (SG_PPO_WAVES=4: tuning knob, 4 waves always)
static int ppo_block_threads(int MT) {
    const char* we = getenv("SG_PPO_WAVES");
    return (MT >= 2 && !(we && atoi(we) == 4)) ? 512 : 256;
}

// ------------------------------------------------------------------------- kernel instances
// Every family of row-group kernels exists in a few instances: shape-specialised ones X(MT, Op/16, Hp/16) for the shipped
// configurations at the row-group size the launch heuristic picks for them, run-time-shape ones
// X(MT, 0, 0), and global-weight ones (run-time shapes, weights through L2).  A family is its list of each; the lists are
// what gets compiled.
#define SG_PPO_SHAPES(X, K) X(K, 1, 3, 4) X(K, 2, 3, 4) /* north-star: obs 47, h64 */ X(K, 2, 1, 7) /* HopperCombined: obs 14, h100 */ \
                            X(K, 2, 4, 7) /* LaikagoCombined: obs 64, h100 */ X(K, 2, 7, 4) /* Laikago refinement: obs 111, h64 */
#define SG_SPLIT_SHAPES(X, K) X(K, 2, 4, 7) /* LaikagoCombined (k_ppo_pair: at <= 2720-row minibatches) */ X(K, 2, 1, 7) /* HopperCombined */
#define SG_FUSED_SHAPES(X, K) X(K, 1, 3, 4) X(K, 2, 3, 4) X(K, 2, 7, 4)   // Policy: north-star, Laikago refinement
#define SG_SYM_SHAPES(X, K) X(K, 2, 7, 4)                                 // the Laikago refinement
#define SG_A2C_SHAPES(X, K) X(K, 2, 3, 4) X(K, 1, 3, 4)                   // north-star
#define SG_NONE(X, K)
#define SG_MT_421(X, K) X(K, 4, 0, 0) X(K, 2, 0, 0) X(K, 1, 0, 0)
#define SG_MT_21(X, K) X(K, 2, 0, 0) X(K, 1, 0, 0)

struct PpoInstance {
    int mt, ko, kh;
    bool gw;
    void (*kernel)(PpoArgs);
};
#define SG_INST(K, mt, o, h) {mt, o, h, false, K(mt, o, h, false)},
#define SG_INST_GW(K, mt, o, h) {mt, o, h, true, K(mt, o, h, true)},
// SHAPES first: ppo_launch takes the first instance that matches
#define SG_PPO_FAMILY(name, K, SHAPES, RUNTIME_MT, GW_MT) \
    static const PpoInstance name[] = {SHAPES(SG_INST, K) RUNTIME_MT(SG_INST, K) GW_MT(SG_INST_GW, K)}

#define SG_K_FWD(mt, o, h, gw) k_ppo_fwd<mt, o, h, gw>
#define SG_K_FWD_CRITIC(mt, o, h, gw) k_ppo_fwd_critic<mt, o, h>
#define SG_K_PAIR(mt, o, h, gw) k_ppo_pair<mt, o, h>
#define SG_K_BWD(mt, o, h, gw) k_ppo_bwd<mt, o, h, false, gw>
#define SG_K_BWD_FUSED(mt, o, h, gw) k_ppo_bwd<mt, o, h, true, gw>
#define SG_K_BWD_FUSED_DX(mt, o, h, gw) k_ppo_bwd<mt, o, h, true, gw, true>
#define SG_K_FWD_SYM(mt, o, h, gw) k_ppo_fwd_sym<mt, o, h, gw>
#define SG_K_BWD_SYM(mt, o, h, gw) k_ppo_bwd_sym<mt, o, h, gw>
#define SG_K_A2C_BWD(mt, o, h, gw) k_a2c_bwd<mt, o, h, gw>
#define SG_K_A2C_BWD_DX(mt, o, h, gw) k_a2c_bwd_dx<mt, gw>
#define SG_K_BWD_FUSED_CAT(mt, o, h, gw) k_ppo_bwd_dist<mt, gw, SG_DIST_CATEGORICAL>
#define SG_K_BWD_FUSED_BER(mt, o, h, gw) k_ppo_bwd_dist<mt, gw, SG_DIST_BERNOULLI>
#define SG_K_A2C_BWD_CAT(mt, o, h, gw) k_a2c_bwd_dist<mt, gw, SG_DIST_CATEGORICAL>
#define SG_K_A2C_BWD_BER(mt, o, h, gw) k_a2c_bwd_dist<mt, gw, SG_DIST_BERNOULLI>
#define SG_K_BWD_FUSED_CAT_DX(mt, o, h, gw) k_ppo_bwd_dist_dx<mt, gw, SG_DIST_CATEGORICAL>
#define SG_K_BWD_FUSED_BER_DX(mt, o, h, gw) k_ppo_bwd_dist_dx<mt, gw, SG_DIST_BERNOULLI>
#define SG_K_A2C_BWD_CAT_DX(mt, o, h, gw) k_a2c_bwd_dist_dx<mt, gw, SG_DIST_CATEGORICAL>
#define SG_K_A2C_BWD_BER_DX(mt, o, h, gw) k_a2c_bwd_dist_dx<mt, gw, SG_DIST_BERNOULLI>
SG_PPO_FAMILY(ppo_fwd_family, SG_K_FWD, SG_PPO_SHAPES, SG_MT_421, SG_MT_21);
SG_PPO_FAMILY(ppo_fwd_critic_family, SG_K_FWD_CRITIC, SG_SPLIT_SHAPES, SG_MT_21, SG_NONE);   // SplitPolicy, critic in the forward launch
SG_PPO_FAMILY(ppo_pair_family, SG_K_PAIR, SG_SPLIT_SHAPES, SG_MT_21, SG_NONE);               // SplitPolicy, one launch per step
SG_PPO_FAMILY(ppo_bwd_family, SG_K_BWD, SG_PPO_SHAPES, SG_MT_421, SG_MT_21);
// Policy (independent actor / critic trunks): forward recomputed inside, no k_ppo_fwd launch
SG_PPO_FAMILY(ppo_bwd_fused_family, SG_K_BWD_FUSED, SG_FUSED_SHAPES, SG_MT_21, SG_MT_21);
SG_PPO_FAMILY(ppo_bwd_fused_dx_family, SG_K_BWD_FUSED_DX, SG_NONE, SG_MT_21, SG_MT_21);      // the recurrent policy's heads: + d loss / d h_t
SG_PPO_FAMILY(ppo_fwd_sym_family, SG_K_FWD_SYM, SG_SYM_SHAPES, SG_MT_21, SG_MT_21);               // mirror-symmetry loss: grid (row groups, 3)
SG_PPO_FAMILY(ppo_bwd_sym_family, SG_K_BWD_SYM, SG_SYM_SHAPES, SG_MT_21, SG_MT_21);
SG_PPO_FAMILY(a2c_bwd_family, SG_K_A2C_BWD, SG_A2C_SHAPES, SG_MT_21, SG_MT_21);
SG_PPO_FAMILY(a2c_bwd_dx_family, SG_K_A2C_BWD_DX, SG_NONE, SG_MT_21, SG_MT_21);               // A2C through time: + d loss / d h_t
// Policy on a Discrete / MultiBinary action space: PPO in the fused form, A2C in the two-launch form; run-time shapes
SG_PPO_FAMILY(ppo_bwd_fused_cat_family, SG_K_BWD_FUSED_CAT, SG_NONE, SG_MT_21, SG_MT_21);
SG_PPO_FAMILY(ppo_bwd_fused_ber_family, SG_K_BWD_FUSED_BER, SG_NONE, SG_MT_21, SG_MT_21);
SG_PPO_FAMILY(a2c_bwd_cat_family, SG_K_A2C_BWD_CAT, SG_NONE, SG_MT_21, SG_MT_21);
SG_PPO_FAMILY(a2c_bwd_ber_family, SG_K_A2C_BWD_BER, SG_NONE, SG_MT_21, SG_MT_21);
// ... as the heads of a recurrent Policy (sg_policy_create_rnn_dist): + d loss / d h_t
SG_PPO_FAMILY(ppo_bwd_fused_cat_dx_family, SG_K_BWD_FUSED_CAT_DX, SG_NONE, SG_MT_21, SG_MT_21);
SG_PPO_FAMILY(ppo_bwd_fused_ber_dx_family, SG_K_BWD_FUSED_BER_DX, SG_NONE, SG_MT_21, SG_MT_21);
SG_PPO_FAMILY(a2c_bwd_cat_dx_family, SG_K_A2C_BWD_CAT_DX, SG_NONE, SG_MT_21, SG_MT_21);
SG_PPO_FAMILY(a2c_bwd_ber_dx_family, SG_K_A2C_BWD_BER_DX, SG_NONE, SG_MT_21, SG_MT_21);

// Launches the family's instance for (MT, the policy's shape, gw): with gw a global-weight instance, else the one specialised
// for the shape, else the run-time-shape one.  (The specialised instances fold ONE hidden width into the code: a policy whose
// critic was rebuilt at another width -- Policy.reset_critic, d.Hc != d.H -- has kh = 0 here, which matches none of them.)
// A row-group size the family has no instance for is an error: grid and LDS size were computed for MT, no other fits them.
template <size_t NI>
static int ppo_launch(sg_ctx* ctx, const PpoInstance (&family)[NI], const char* what, int prof, int MT, const SgPolicyDesc& d, dim3 grid,
                      size_t lds, const PpoArgs& pa, bool gw) {
    const int ko = d.Op / 16, kh = d.Hc == d.H ? d.Hp / 16 : 0;
    const PpoInstance* inst = nullptr;
    for (const PpoInstance& i : family)
        if (!inst && i.mt == MT && i.gw == gw && ((i.ko == 0 && i.kh == 0) || (!gw && i.ko == ko && i.kh == kh))) inst = &i;
    SG_REQUIRE(inst, "sg_ppo_update: %s has no instance for %d-row groups%s", what, 16 * MT, gw ? " with global weights" : "");
    SG_LAUNCH(ctx, prof, inst->kernel, grid, dim3(ppo_block_threads(MT)), lds, pa);
    return 0;
}

// ---------------------------------------------------------------------------------- PPO API
extern "C" int sg_ppo_create(sg_ctx* ctx, sg_policy* p, const sg_ppo_config* cfg, sg_ppo** out) {
    SG_DEVICE_WIDE();
    SG_REQUIRE(ctx && p && cfg && out, "sg_ppo_create: NULL argument");
    SG_REQUIRE(!(sg_policy_cnn_rnn(p) && ctx->use_comm && ctx->world > 1), "sg_ppo_create: PPO on the recurrent CNN base runs on one rank: "
               "this context has a communicator of world %d (data-parallel PPO through time on images is not implemented)", ctx->world);
    SG_REQUIRE(!(p->recurrent && ctx->use_comm && ctx->world > 1), "sg_ppo_create: PPO with a recurrent policy runs on one rank: this "
               "context has a communicator of world %d (data-parallel PPO through time is not implemented)", ctx->world);
    SG_REQUIRE(cfg->ppo_epoch > 0 && cfg->num_mini_batch > 0, "sg_ppo_create: ppo_epoch and num_mini_batch must be positive");
    SG_REQUIRE(!(p->cnn && ctx->use_comm && ctx->world > 1), "sg_ppo_create: PPO on the CNN base (image observations) runs on one rank: "
               "this context has a communicator of world %d (data-parallel PPO on it is not implemented)", ctx->world);
    // a policy whose trunk does not fit a CU's LDS runs on the global-weight instances; only the 16-row tiles must fit
    const size_t tiles_f = ppo_fwd_lds(p->desc, 1, true), tiles_b = ppo_bwd_tiles_lds(p->desc, 1, 0, 2, false);
    SG_REQUIRE(p->cnn || (tiles_f <= (size_t)ctx->lds_bytes && tiles_b <= (size_t)ctx->lds_bytes),
               "sg_ppo_create: the 16-row activation tiles of this policy do not fit LDS (%zu / %zu > %d bytes)", tiles_f, tiles_b,
               ctx->lds_bytes);
    SG_CHECK(hipSetDevice(ctx->device));
    sg_ppo* a = new sg_ppo();
    a->ctx = ctx; a->policy = p; a->cfg = *cfg;
    const size_t tot = sg_policy_padded_count(p) + 8;   // (recurrent: heads block | GRU block, one Adam over both)
    SG_CHECK(sg_dev_malloc((void**)&a->d_m, sizeof(float) * tot));
    SG_CHECK(sg_dev_malloc((void**)&a->d_v, sizeof(float) * tot));
    SG_CHECK(sg_dev_malloc((void**)&a->d_grad, sizeof(float) * tot));
    SG_CHECK(sg_dev_malloc((void**)&a->d_state, sizeof(SgOptState)));
    SG_CHECK(sg_dev_malloc((void**)&a->d_loss_acc, sizeof(double) * 8));
    SG_CHECK(sg_dev_malloc((void**)&a->d_part, sizeof(float) * ((tot + 8 + SG_PPO_REDUCE_PARAMS - 1) / SG_PPO_REDUCE_PARAMS + 8 +
                                                                 (p->recurrent ? (p->gru.total + 255) / 256 : 0))));
    SG_CHECK(hipMemsetAsync(a->d_m, 0, sizeof(float) * tot, ctx->stream));
    SG_CHECK(hipMemsetAsync(a->d_v, 0, sizeof(float) * tot, ctx->stream));
    SG_CHECK(hipMemsetAsync(a->d_loss_acc, 0, sizeof(double) * 8, ctx->stream));
    // the recurrent CNN base: the floats between the flat block and the GRU block are written by no kernel and read by the norm and Adam
    if (sg_policy_cnn_rnn(p)) SG_CHECK(hipMemsetAsync(a->d_grad, 0, sizeof(float) * tot, ctx->stream));
    SG_CHECK(sg_dev_malloc((void**)&a->d_pair, SG_PAIR_BYTES));            // k_ppo_pair: error word
    SG_CHECK(hipMemsetAsync(a->d_pair, 0, SG_PAIR_BYTES, ctx->stream));
    SgOptState st;
    memset(&st, 0, sizeof st);
    st.lr = cfg->lr;
    SG_CHECK(hipMemcpyAsync(a->d_state, &st, sizeof st, hipMemcpyHostToDevice, ctx->stream));
    SG_CHECK(hipStreamSynchronize(ctx->stream));
    sg_ctx_learner_born(ctx);
    *out = a;
    return 0;
}

// a2c/main.py:123-131 -> A2C_ACKTR(actor_critic, value_loss_coef, entropy_coef, lr, eps, alpha, max_grad_norm), acktr=False
// (a2c/algo/a2c_acktr.py:30-51: RMSprop, square_avg starting at zero).  Policy (MLP) on one rank only.
extern "C" int sg_a2c_create(sg_ctx* ctx, sg_policy* p, const sg_a2c_config* cfg, sg_ppo** out) {
    SG_REQUIRE(ctx && p && cfg && out, "sg_a2c_create: NULL argument");
    SG_REQUIRE(!sg_policy_cnn_rnn(p), "sg_a2c_create: A2C is not implemented for the recurrent CNN base (sg_policy_create_cnn_rnn): PPO is");
    SG_REQUIRE(!p->cnn, "sg_a2c_create: A2C is not implemented for the CNN base (image observations): PPO is (A2C on it has an "
               "entry point of its own, sg_a2c_create_cnn)");
    SG_REQUIRE(!p->recurrent, "sg_a2c_create: A2C is implemented for feed-forward policies only, not for a recurrent Policy");
    SG_REQUIRE(p->desc.kind == SG_POLICY_MLP, "sg_a2c_create: A2C is implemented for Policy (MLP) only, not for SplitPolicy");
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_a2c_create: A2C runs on one rank: this context has a communicator of "
               "world %d (data-parallel A2C is not implemented)", ctx->world);
    SG_REQUIRE(cfg->alpha >= 0.f && cfg->alpha <= 1.f && cfg->eps >= 0.f && cfg->max_grad_norm > 0.f,
               "sg_a2c_create: alpha must lie in [0, 1], eps >= 0 and max_grad_norm > 0 (got %g, %g, %g)", (double)cfg->alpha,
               (double)cfg->eps, (double)cfg->max_grad_norm);
    sg_ppo_config pc;
    memset(&pc, 0, sizeof pc);
    pc.ppo_epoch = 1; pc.num_mini_batch = 1;   // one optimizer step per update: the results ring's step count
    pc.value_loss_coef = cfg->value_loss_coef; pc.entropy_coef = cfg->entropy_coef;
    pc.lr = cfg->lr; pc.eps = cfg->eps; pc.max_grad_norm = cfg->max_grad_norm;
    sg_ppo* a = nullptr;
    SG_TRY(sg_ppo_create(ctx, p, &pc, &a));
    a->a2c = true;
    a->alpha = cfg->alpha;
    *out = a;
    return 0;
}

// The same learner on a recurrent Policy (a2c/main.py:123-131 with --recurrent-policy): evaluate_actions steps the GRU through
// the rollout from the state of slot 0 (a2c/algo/a2c_acktr.py:56-63, a2c/model.py:117-201); clip and RMSprop cover the GRU's
// tensors too.  An entry point of its own: sg_a2c_create keeps refusing a recurrent policy.
extern "C" int sg_a2c_create_rnn(sg_ctx* ctx, sg_policy* p, const sg_a2c_config* cfg, sg_ppo** out) {
    SG_REQUIRE(ctx && p && cfg && out, "sg_a2c_create_rnn: NULL argument");
    SG_REQUIRE(!sg_policy_cnn_rnn(p), "sg_a2c_create_rnn: A2C through time is not implemented for the recurrent CNN base "
               "(sg_policy_create_cnn_rnn): PPO is");
    SG_REQUIRE(p->recurrent, "sg_a2c_create_rnn: A2C through time takes a recurrent Policy (kind SG_POLICY_GRU); this policy is "
               "feed-forward (sg_a2c_create)");
    SG_REQUIRE(!p->cnn && p->desc.kind == SG_POLICY_MLP,
               "sg_a2c_create_rnn: A2C through time is implemented for the GRU base of Policy only, not for the CNN base");
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_a2c_create_rnn: A2C with a recurrent policy runs on one rank: this context has a "
               "communicator of world %d (data-parallel A2C through time is not implemented)", ctx->world);
    SG_REQUIRE(cfg->alpha >= 0.f && cfg->alpha <= 1.f && cfg->eps >= 0.f && cfg->max_grad_norm > 0.f,
               "sg_a2c_create_rnn: alpha must lie in [0, 1], eps >= 0 and max_grad_norm > 0 (got %g, %g, %g)", (double)cfg->alpha,
               (double)cfg->eps, (double)cfg->max_grad_norm);
    sg_ppo_config pc;
    memset(&pc, 0, sizeof pc);
    pc.ppo_epoch = 1; pc.num_mini_batch = 1;
    pc.value_loss_coef = cfg->value_loss_coef; pc.entropy_coef = cfg->entropy_coef;
    pc.lr = cfg->lr; pc.eps = cfg->eps; pc.max_grad_norm = cfg->max_grad_norm;
    sg_ppo* a = nullptr;
    SG_TRY(sg_ppo_create(ctx, p, &pc, &a));
    a->a2c = true;
    a->a2c_rnn = true;
    a->alpha = cfg->alpha;
    *out = a;
    return 0;
}

// The same learner on the CNN base (a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:204-230, the reference's default pairing):
// the update takes the whole rollout in row chunks whose gradients accumulate (a2c_cnn_update).  An entry point of its own:
// sg_a2c_create keeps refusing a CNN policy.
extern "C" int sg_a2c_create_cnn(sg_ctx* ctx, sg_policy* p, const sg_a2c_config* cfg, sg_ppo** out) {
    SG_REQUIRE(ctx && p && cfg && out, "sg_a2c_create_cnn: NULL argument");
    SG_REQUIRE(!sg_policy_cnn_rnn(p), "sg_a2c_create_cnn: A2C on image observations is not implemented for the recurrent CNN base "
               "(sg_policy_create_cnn_rnn): its row chunks carry no hidden state; PPO is");
    SG_REQUIRE(p->cnn, "sg_a2c_create_cnn: A2C on image observations takes a policy with the CNN base (sg_policy_create_cnn); this "
               "policy has none (sg_a2c_create%s)", p->recurrent ? "_rnn" : "");
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_a2c_create_cnn: A2C on the CNN base (image observations) runs on one rank: this "
               "context has a communicator of world %d (data-parallel A2C is not implemented)", ctx->world);
    SG_REQUIRE(cfg->alpha >= 0.f && cfg->alpha <= 1.f && cfg->eps >= 0.f && cfg->max_grad_norm > 0.f,
               "sg_a2c_create_cnn: alpha must lie in [0, 1], eps >= 0 and max_grad_norm > 0 (got %g, %g, %g)", (double)cfg->alpha,
               (double)cfg->eps, (double)cfg->max_grad_norm);
    sg_ppo_config pc;
    memset(&pc, 0, sizeof pc);
    pc.ppo_epoch = 1; pc.num_mini_batch = 1;
    pc.value_loss_coef = cfg->value_loss_coef; pc.entropy_coef = cfg->entropy_coef;
    pc.lr = cfg->lr; pc.eps = cfg->eps; pc.max_grad_norm = cfg->max_grad_norm;
    sg_ppo* a = nullptr;
    SG_TRY(sg_ppo_create(ctx, p, &pc, &a));
    a->a2c = true;
    a->a2c_cnn = true;
    a->alpha = cfg->alpha;
    *out = a;
    return 0;
}

// The same learner on the recurrent CNN base (a2c/main.py --algo a2c --recurrent-policy on image observations:
// a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:117-230): the update takes the whole rollout through time in groups of whole
// environments whose gradients accumulate (a2c_cnn_gru_update).  An entry point of its own: the three above keep refusing this base.
extern "C" int sg_a2c_create_cnn_rnn(sg_ctx* ctx, sg_policy* p, const sg_a2c_config* cfg, sg_ppo** out) {
    SG_REQUIRE(ctx && p && cfg && out, "sg_a2c_create_cnn_rnn: NULL argument");
    SG_REQUIRE(sg_policy_cnn_rnn(p), "sg_a2c_create_cnn_rnn: A2C through time on image observations takes a policy with the recurrent "
               "CNN base (sg_policy_create_cnn_rnn); this policy %s (sg_a2c_create%s)",
               p->cnn ? "has the feed-forward CNN base" : p->recurrent ? "has the GRU base on vector observations" : "has neither a CNN nor a GRU",
               p->cnn ? "_cnn" : p->recurrent ? "_rnn" : "");
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_a2c_create_cnn_rnn: A2C on the recurrent CNN base runs on one rank: this context "
               "has a communicator of world %d (data-parallel A2C through time on images is not implemented)", ctx->world);
    SG_REQUIRE(cfg->alpha >= 0.f && cfg->alpha <= 1.f && cfg->eps >= 0.f && cfg->max_grad_norm > 0.f,
               "sg_a2c_create_cnn_rnn: alpha must lie in [0, 1], eps >= 0 and max_grad_norm > 0 (got %g, %g, %g)", (double)cfg->alpha,
               (double)cfg->eps, (double)cfg->max_grad_norm);
    sg_ppo_config pc;
    memset(&pc, 0, sizeof pc);
    pc.ppo_epoch = 1; pc.num_mini_batch = 1;
    pc.value_loss_coef = cfg->value_loss_coef; pc.entropy_coef = cfg->entropy_coef;
    pc.lr = cfg->lr; pc.eps = cfg->eps; pc.max_grad_norm = cfg->max_grad_norm;
    sg_ppo* a = nullptr;
    SG_TRY(sg_ppo_create(ctx, p, &pc, &a));
    a->a2c = true;
    a->a2c_cnn_rnn = true;
    a->alpha = cfg->alpha;
    *out = a;
    return 0;
}

// a2c/main.py:159-161 -> A2C_ACKTR(actor_critic, value_loss_coef, entropy_coef, acktr=True): KFACOptimizer(actor_critic) with
// the constructor values in cfg (a2c/algo/kfac.py:97-150).  Policy (MLP) on one rank only.
extern "C" int sg_acktr_create(sg_ctx* ctx, sg_policy* p, const sg_acktr_config* cfg, sg_ppo** out) {
    SG_DEVICE_WIDE();   // kfac_setup's clears and copies on ctx->stream, never beside a capture in flight (recursive with sg_ppo_create's)
    SG_REQUIRE(ctx && p && cfg && out, "sg_acktr_create: NULL argument");
    SG_REQUIRE(!sg_policy_cnn_rnn(p), "sg_acktr_create: ACKTR is not implemented for the recurrent CNN base (sg_policy_create_cnn_rnn): "
               "neither its convolutions nor its GRU have K-FAC blocks here; PPO is");
    SG_REQUIRE(!p->cnn, "sg_acktr_create: ACKTR is not implemented for the CNN base (image observations): its convolutions have no "
               "K-FAC blocks here; PPO is");
    SG_REQUIRE(!p->recurrent, "sg_acktr_create: ACKTR is not defined for a recurrent Policy (the reference refuses it too: "
               "a2c/arguments.py:253-255)");
    SG_REQUIRE(p->desc.kind == SG_POLICY_MLP, "sg_acktr_create: ACKTR is implemented for Policy (MLP) only, not for SplitPolicy");
    SG_REQUIRE(p->desc.dist == SG_DIST_GAUSSIAN, "sg_acktr_create: ACKTR is implemented for Box action spaces only: this policy has a "
               "%s head (its Fisher sampling is not built)", p->desc.dist == SG_DIST_CATEGORICAL ? "Categorical" : "Bernoulli");
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_acktr_create: ACKTR runs on one rank: this context has a communicator of "
               "world %d (data-parallel ACKTR is not implemented)", ctx->world);
    SG_REQUIRE(cfg->lr > 0.f && cfg->momentum >= 0.f && cfg->momentum < 1.f && cfg->stat_decay > 0.f && cfg->stat_decay < 1.f &&
               cfg->kl_clip > 0.f && cfg->damping >= 0.f && cfg->Tf >= 1,
               "sg_acktr_create: need lr > 0, momentum in [0, 1), stat_decay in (0, 1), kl_clip > 0, damping >= 0 and Tf >= 1");
    sg_a2c_config ac;
    memset(&ac, 0, sizeof ac);
    ac.value_loss_coef = cfg->value_loss_coef; ac.entropy_coef = cfg->entropy_coef;
    ac.lr = cfg->lr; ac.eps = 1.f; ac.alpha = 0.f; ac.max_grad_norm = 1.f;   // unused: no RMSprop, no clip
    sg_ppo* a = nullptr;
    SG_TRY(sg_a2c_create(ctx, p, &ac, &a));
    a->kfac = new SgKfac();
    a->kfac->cfg = *cfg;
    const int rc = kfac_setup(ctx, a->kfac, p->desc, a->d_grad);
    if (rc != 0) {
        const std::string err = sg_last_error();
        sg_ppo_destroy(a);
        sg_set_error("%s", err.c_str());
        return rc;
    }
    *out = a;
    return 0;
}

extern "C" int sg_ppo_destroy(sg_ppo* a) {
    SG_DEVICE_WIDE();
    if (!a) return 0;
    (void)hipStreamSynchronize(a->ctx->stream);
    sg_ctx_learner_gone(a->ctx);
    for (auto& q : a->ctx->res_a) if (q == a) q = nullptr;
    float* ptrs[] = {a->d_m, a->d_v, a->d_grad, a->d_slabs, a->d_state, a->d_part, a->d_stacks, a->d_mobs_mat, a->d_mact, a->d_mrows,
                     a->d_h0, a->d_gru};
    for (float* q : ptrs) if (q) (void)sg_dev_free(q);
    if (a->d_perms) (void)sg_dev_free(a->d_perms);
    if (a->d_loss_acc) (void)sg_dev_free(a->d_loss_acc);
    if (a->d_pair) (void)sg_dev_free(a->d_pair);
    if (a->h_h0) (void)sg_host_release(a->h_h0);
    for (hipEvent_t ev : a->h0_ev) if (ev) (void)hipEventDestroy(ev);
    sg_graph_release(&a->steps_graph);
    kfac_free(a);
    delete a;
    return 0;
}

__global__ void k_set_lr(SgOptState* st, float lr) { st->lr = lr; }

extern "C" int sg_ppo_set_lr(sg_ppo* a, float lr) {
    SG_REQUIRE(a, "sg_ppo_set_lr: NULL argument");
    SG_CHECK(hipSetDevice(a->ctx->device));
    a->cfg.lr = lr;
    // by kernel argument, in stream order: no host synchronisation (the schedule writes it before every update)
    hipLaunchKernelGGL(k_set_lr, dim3(1), dim3(1), 0, a->ctx->stream, reinterpret_cast<SgOptState*>(a->d_state), lr);
    SG_CHECK(hipGetLastError());
    return 0;
}

// a2c/algo/ppo.py:110-136 (enabled by a2c/main.py:133-146, --loss-sym): symmetry_coef > 0 adds coef * mean((M_a mu(s) -
// mu(mirror_obs(s)))^2) to every optimizer step's loss.  m_obs NULL: the caller mirrors the rows itself and hands them over
// before every update (sg_ppo_set_mirrored_obs).
extern "C" int sg_ppo_set_symmetry(sg_ppo* a, float coef, const float* m_obs, const float* m_act) {
    SG_REQUIRE(a, "sg_ppo_set_symmetry: NULL argument");
    SG_REQUIRE(!a->a2c, "sg_ppo_set_symmetry: the mirror-symmetry loss is a PPO option; this is an A2C / ACKTR handle");
    SG_REQUIRE(coef >= 0.f && coef < INFINITY, "sg_ppo_set_symmetry: symmetry_coef must be finite and >= 0 (got %g)", (double)coef);
    sg_ctx* ctx = a->ctx;
    const SgPolicyDesc& d = a->policy->desc;
    SG_CHECK(hipSetDevice(ctx->device));
    SG_CHECK(hipStreamSynchronize(ctx->stream));   // a queued update may still read the mirrors
    if (coef == 0.f) { a->sym_coef = 0.f; return 0; }   // a2c/algo/ppo.py:111: plain PPO
    SG_REQUIRE(m_act, "sg_ppo_set_symmetry: symmetry_coef > 0 needs the action mirror m_act");
    SG_REQUIRE(!sg_policy_cnn_rnn(a->policy), "sg_ppo_set_symmetry: the mirror-symmetry loss is not implemented for the recurrent CNN "
               "base (image observations have no linear mirror map here, and the mirrored rows have no hidden state)");
    SG_REQUIRE(!a->policy->cnn, "sg_ppo_set_symmetry: the mirror-symmetry loss is not implemented for the CNN base (image "
               "observations have no linear mirror map here)");
    SG_REQUIRE(d.kind == SG_POLICY_MLP, "sg_ppo_set_symmetry: the mirror-symmetry loss is implemented for Policy (MLP) only, "
               "not for SplitPolicy");
    SG_REQUIRE(d.dist == SG_DIST_GAUSSIAN, "sg_ppo_set_symmetry: the mirror-symmetry loss compares action means: it is defined for "
               "Box action spaces only, not for a %s head", d.dist == SG_DIST_CATEGORICAL ? "Categorical" : "Bernoulli");
    SG_REQUIRE(!a->policy->recurrent, "sg_ppo_set_symmetry: the mirror-symmetry loss is implemented for feed-forward policies only, "
               "not for a recurrent Policy");
    SG_REQUIRE(ppo_bwd_tiles_lds(d, 1, 0, 3, true) <= (size_t)ctx->lds_bytes,
               "sg_ppo_set_symmetry: the 16-row tiles of the symmetric step do not fit LDS (%zu > %d bytes)",
               ppo_bwd_tiles_lds(d, 1, 0, 3, true), ctx->lds_bytes);
    if (!a->d_mact) SG_CHECK(sg_dev_malloc((void**)&a->d_mact, sizeof(float) * d.A * d.A));
    SG_COPY_SYNC(ctx, a->d_mact, m_act, sizeof(float) * d.A * d.A, hipMemcpyHostToDevice);
    if (m_obs) {
        if (!a->d_mobs_mat) SG_CHECK(sg_dev_malloc((void**)&a->d_mobs_mat, sizeof(float) * d.O * d.O));
        SG_COPY_SYNC(ctx, a->d_mobs_mat, m_obs, sizeof(float) * d.O * d.O, hipMemcpyHostToDevice);
    } else if (a->d_mobs_mat) {
        SG_CHECK(sg_dev_free(a->d_mobs_mat));
        a->d_mobs_mat = nullptr;
    }
    a->sym_coef = coef;
    return 0;
}

// mirror_obsact_batch(obs, ..., mirror_obs, augment=False) of every rollout row (my_pybullet_envs/utils.py:334-357), done by
// the caller: host[T*N][O] float32, consumed by the next sg_ppo_update (which requires count == T*N*O)
extern "C" int sg_ppo_set_mirrored_obs(sg_ppo* a, const float* host, int64_t count) {
    SG_REQUIRE(a && host, "sg_ppo_set_mirrored_obs: NULL argument");
    SG_REQUIRE(!a->a2c, "sg_ppo_set_mirrored_obs: the mirror-symmetry loss is a PPO option; this is an A2C / ACKTR handle");
    SG_REQUIRE(count > 0 && count % a->policy->desc.O == 0, "sg_ppo_set_mirrored_obs: %lld floats is not a whole number of %d-float rows",
               (long long)count, a->policy->desc.O);
    sg_ctx* ctx = a->ctx;
    SG_CHECK(hipSetDevice(ctx->device));
    SG_CHECK(hipStreamSynchronize(ctx->stream));   // a queued update may still read the previous rows
    SG_TRY(ensure_cap(ctx->stream, &a->d_mrows, &a->mrows_cap, count));
    SG_COPY_SYNC(ctx, a->d_mrows, host, sizeof(float) * count, hipMemcpyHostToDevice);
    a->mrows_host = count;
    return 0;
}

// the last update's symmetry_loss.item(), averaged over its ppo_epoch * num_mini_batch steps like out3 (0 with the loss off)
extern "C" int sg_ppo_last_symmetry_loss(sg_ppo* a, float* out) {
    SG_REQUIRE(a && out, "sg_ppo_last_symmetry_loss: NULL argument");
    SG_CHECK(hipSetDevice(a->ctx->device));
    double acc = 0.0;
    SG_TRY(sg_ctx_fetch_f64(a->ctx, a->d_loss_acc + 3, &acc, 1));
    *out = (float)(acc / ((double)a->cfg.ppo_epoch * a->cfg.num_mini_batch));
    return 0;
}

extern "C" int sg_ppo_last_perms(sg_ppo* a, int64_t* perms, int64_t count) {
    SG_REQUIRE(a && perms, "sg_ppo_last_perms: NULL argument");
    SG_REQUIRE(a->last_perm_count > 0, "sg_ppo_last_perms: no update has run on this agent");
    SG_REQUIRE(count == a->last_perm_count, "sg_ppo_last_perms: the last update used %lld indices, asked for %lld",
               (long long)a->last_perm_count, (long long)count);
    SG_CHECK(hipSetDevice(a->ctx->device));
    SG_CHECK(hipStreamSynchronize(a->ctx->stream));
    SG_COPY_SYNC(a->ctx, perms, a->d_perms, sizeof(int64_t) * count, hipMemcpyDeviceToHost);
    return 0;
}

extern "C" int sg_ppo_get_adam(sg_ppo* a, float* m, float* v, int64_t n, int64_t* step) {
    SG_REQUIRE(a && m && v && step, "sg_ppo_get_adam: NULL argument");
    SG_REQUIRE(!a->kfac, "sg_ppo_get_adam: an ACKTR handle has K-FAC state, not Adam's (sg_acktr_get_state)");
    SG_REQUIRE(!a->a2c, "sg_ppo_get_adam: an A2C handle has RMSprop state, not Adam's (sg_a2c_get_rmsprop)");
    const SgPolicyDesc& d = a->policy->desc;
    const sg_policy* pol = a->policy;
    const int64_t n_gru = pol->recurrent ? sg_gru_flat_count(pol->gru) : 0;   // the GRU's tensors come first in the flat order
    if (sg_policy_cnn_rnn(pol)) {   // flat: the GRU's tensors, then the CNN base's; device: the flat CNN block, then the GRU's tiles
        SG_REQUIRE(n == pol->cnnd.total + n_gru, "sg_ppo_get_adam: bad length");
        const size_t ptot = sg_policy_padded_count(pol);
        std::vector<float> pm(ptot), pv(ptot);
        SG_CHECK(hipStreamSynchronize(a->ctx->stream));
        SG_COPY_SYNC(a->ctx, pm.data(), a->d_m, sizeof(float) * ptot, hipMemcpyDeviceToHost);
        SG_COPY_SYNC(a->ctx, pv.data(), a->d_v, sizeof(float) * ptot, hipMemcpyDeviceToHost);
        sg_gru_unpad(pol->gru, pm.data() + pol->gru.off, m);
        sg_gru_unpad(pol->gru, pv.data() + pol->gru.off, v);
        memcpy(m + n_gru, pm.data(), sizeof(float) * (size_t)pol->cnnd.total);
        memcpy(v + n_gru, pv.data(), sizeof(float) * (size_t)pol->cnnd.total);
        *step = a->opt_t;
        return 0;
    }
    if (pol->cnn) {   // the CNN base keeps the flat order on the device
        SG_REQUIRE(n == pol->cnnd.total, "sg_ppo_get_adam: bad length");
        SG_CHECK(hipStreamSynchronize(a->ctx->stream));
        SG_COPY_SYNC(a->ctx, m, a->d_m, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost);
        SG_COPY_SYNC(a->ctx, v, a->d_v, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost);
        *step = a->opt_t;
        return 0;
    }
    SG_REQUIRE(n == sg_policy_flat_count(d) + n_gru, "sg_ppo_get_adam: bad length");
    const size_t ptot = sg_policy_padded_count(pol);
    std::vector<float> pm(ptot), pv(ptot);
    SG_CHECK(hipStreamSynchronize(a->ctx->stream));
    SG_COPY_SYNC(a->ctx, pm.data(), a->d_m, sizeof(float) * ptot, hipMemcpyDeviceToHost);
    SG_COPY_SYNC(a->ctx, pv.data(), a->d_v, sizeof(float) * ptot, hipMemcpyDeviceToHost);
    if (pol->recurrent) {
        sg_gru_unpad(pol->gru, pm.data() + pol->gru.off, m);
        sg_gru_unpad(pol->gru, pv.data() + pol->gru.off, v);
    }
    sg_policy_unpad(d, pm.data(), m + n_gru);
    sg_policy_unpad(d, pv.data(), v + n_gru);
    *step = a->opt_t;
    return 0;
}

extern "C" int sg_ppo_set_adam(sg_ppo* a, const float* m, const float* v, int64_t n, int64_t step) {
    SG_REQUIRE(a && m && v, "sg_ppo_set_adam: NULL argument");
    SG_REQUIRE(!a->kfac, "sg_ppo_set_adam: an ACKTR handle has K-FAC state, not Adam's (sg_acktr_get_state)");
    SG_REQUIRE(!a->a2c, "sg_ppo_set_adam: an A2C handle has RMSprop state, not Adam's (sg_a2c_set_rmsprop)");
    const SgPolicyDesc& d = a->policy->desc;
    const sg_policy* pol = a->policy;
    const int64_t n_gru = pol->recurrent ? sg_gru_flat_count(pol->gru) : 0;
    if (sg_policy_cnn_rnn(pol)) {
        SG_REQUIRE(n == pol->cnnd.total + n_gru, "sg_ppo_set_adam: bad length");
        SG_REQUIRE(step >= 0 && step < (1ll << 30), "sg_ppo_set_adam: step out of range");
        const size_t ptot = sg_policy_padded_count(pol);
        std::vector<float> pm(ptot, 0.f), pv(ptot, 0.f);
        sg_gru_pad(pol->gru, m, pm.data() + pol->gru.off);
        sg_gru_pad(pol->gru, v, pv.data() + pol->gru.off);
        memcpy(pm.data(), m + n_gru, sizeof(float) * (size_t)pol->cnnd.total);
        memcpy(pv.data(), v + n_gru, sizeof(float) * (size_t)pol->cnnd.total);
        const int t0r = (int)step;
        SG_CHECK(hipStreamSynchronize(a->ctx->stream));
        SG_COPY_SYNC(a->ctx, a->d_m, pm.data(), sizeof(float) * ptot, hipMemcpyHostToDevice);
        SG_COPY_SYNC(a->ctx, a->d_v, pv.data(), sizeof(float) * ptot, hipMemcpyHostToDevice);
        SG_COPY_SYNC(a->ctx, &reinterpret_cast<SgOptState*>(a->d_state)->t0, &t0r, sizeof t0r, hipMemcpyHostToDevice);
        a->opt_t = step;
        return 0;
    }
    if (pol->cnn) {
        SG_REQUIRE(n == pol->cnnd.total, "sg_ppo_set_adam: bad length");
        SG_REQUIRE(step >= 0 && step < (1ll << 30), "sg_ppo_set_adam: step out of range");
        const int t0c = (int)step;
        SG_CHECK(hipStreamSynchronize(a->ctx->stream));
        SG_COPY_SYNC(a->ctx, a->d_m, m, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
        SG_COPY_SYNC(a->ctx, a->d_v, v, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
        SG_COPY_SYNC(a->ctx, &reinterpret_cast<SgOptState*>(a->d_state)->t0, &t0c, sizeof t0c, hipMemcpyHostToDevice);
        a->opt_t = step;
        return 0;
    }
    SG_REQUIRE(n == sg_policy_flat_count(d) + n_gru, "sg_ppo_set_adam: bad length");
    const size_t ptot = sg_policy_padded_count(pol);
    std::vector<float> pm(ptot, 0.f), pv(ptot, 0.f);
    if (pol->recurrent) {
        sg_gru_pad(pol->gru, m, pm.data() + pol->gru.off);
        sg_gru_pad(pol->gru, v, pv.data() + pol->gru.off);
    }
    sg_policy_pad(d, m + n_gru, pm.data());
    sg_policy_pad(d, v + n_gru, pv.data());
    SG_REQUIRE(step >= 0 && step < (1ll << 30), "sg_ppo_set_adam: step out of range");
    const int t0 = (int)step;
    SG_CHECK(hipStreamSynchronize(a->ctx->stream));
    SG_COPY_SYNC(a->ctx, a->d_m, pm.data(), sizeof(float) * ptot, hipMemcpyHostToDevice);
    SG_COPY_SYNC(a->ctx, a->d_v, pv.data(), sizeof(float) * ptot, hipMemcpyHostToDevice);
    SG_COPY_SYNC(a->ctx, &reinterpret_cast<SgOptState*>(a->d_state)->t0, &t0, sizeof t0, hipMemcpyHostToDevice);
    // the words k_ppo_pair's actor workgroups swap carry Adam step numbers: a step count set from outside may repeat old ones,
    // so the row stacks they live in are cleared before the next update
    a->cleared.mode = SG_LAYOUT_INVALID;
    a->pair_primed = false;
    a->opt_t = step;
    return 0;
}

// square_avg [n] flat in state_dict order, *step = completed RMSprop steps
extern "C" int sg_a2c_get_rmsprop(sg_ppo* a, float* square_avg, int64_t n, int64_t* step) {
    SG_REQUIRE(a && square_avg && step, "sg_a2c_get_rmsprop: NULL argument");
    SG_REQUIRE(!a->kfac, "sg_a2c_get_rmsprop: an ACKTR handle has K-FAC state, not RMSprop's (sg_acktr_get_state)");
    SG_REQUIRE(a->a2c, "sg_a2c_get_rmsprop: not an A2C handle (sg_ppo_get_adam)");
    const SgPolicyDesc& d = a->policy->desc;
    const sg_policy* pol = a->policy;
    const int64_t n_gru = pol->recurrent ? sg_gru_flat_count(pol->gru) : 0;   // the GRU's tensors come first in the flat order
    if (sg_policy_cnn_rnn(pol)) {   // flat: the GRU's tensors, then the CNN base's; device: the flat CNN block, then the GRU's tiles
        SG_REQUIRE(n == pol->cnnd.total + n_gru, "sg_a2c_get_rmsprop: bad length");
        const size_t ptot = sg_policy_padded_count(pol);
        std::vector<float> pv(ptot);
        SG_CHECK(hipSetDevice(a->ctx->device));
        SG_CHECK(hipStreamSynchronize(a->ctx->stream));
        SG_COPY_SYNC(a->ctx, pv.data(), a->d_v, sizeof(float) * ptot, hipMemcpyDeviceToHost);
        sg_gru_unpad(pol->gru, pv.data() + pol->gru.off, square_avg);
        memcpy(square_avg + n_gru, pv.data(), sizeof(float) * (size_t)pol->cnnd.total);
        *step = a->opt_t;
        return 0;
    }
    if (pol->cnn) {   // the CNN base keeps the flat order on the device
        SG_REQUIRE(n == pol->cnnd.total, "sg_a2c_get_rmsprop: bad length");
        SG_CHECK(hipSetDevice(a->ctx->device));
        SG_CHECK(hipStreamSynchronize(a->ctx->stream));
        SG_COPY_SYNC(a->ctx, square_avg, a->d_v, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost);
        *step = a->opt_t;
        return 0;
    }
    SG_REQUIRE(n == sg_policy_flat_count(d) + n_gru, "sg_a2c_get_rmsprop: bad length");
    const size_t ptot = sg_policy_padded_count(pol);
    std::vector<float> pv(ptot);
    SG_CHECK(hipSetDevice(a->ctx->device));
    SG_CHECK(hipStreamSynchronize(a->ctx->stream));
    SG_COPY_SYNC(a->ctx, pv.data(), a->d_v, sizeof(float) * ptot, hipMemcpyDeviceToHost);
    if (pol->recurrent) sg_gru_unpad(pol->gru, pv.data() + pol->gru.off, square_avg);
    sg_policy_unpad(d, pv.data(), square_avg + n_gru);
    *step = a->opt_t;
    return 0;
}

extern "C" int sg_a2c_set_rmsprop(sg_ppo* a, const float* square_avg, int64_t n, int64_t step) {
    SG_REQUIRE(a && square_avg, "sg_a2c_set_rmsprop: NULL argument");
    SG_REQUIRE(!a->kfac, "sg_a2c_set_rmsprop: an ACKTR handle has K-FAC state, not RMSprop's (sg_acktr_get_state)");
    SG_REQUIRE(a->a2c, "sg_a2c_set_rmsprop: not an A2C handle (sg_ppo_set_adam)");
    const SgPolicyDesc& d = a->policy->desc;
    const sg_policy* pol = a->policy;
    const int64_t n_gru = pol->recurrent ? sg_gru_flat_count(pol->gru) : 0;
    if (sg_policy_cnn_rnn(pol)) {
        SG_REQUIRE(n == pol->cnnd.total + n_gru, "sg_a2c_set_rmsprop: bad length");
        SG_REQUIRE(step >= 0, "sg_a2c_set_rmsprop: step out of range");
        const size_t ptot = sg_policy_padded_count(pol);
        std::vector<float> pv(ptot, 0.f);
        sg_gru_pad(pol->gru, square_avg, pv.data() + pol->gru.off);
        memcpy(pv.data(), square_avg + n_gru, sizeof(float) * (size_t)pol->cnnd.total);
        SG_CHECK(hipSetDevice(a->ctx->device));
        SG_CHECK(hipStreamSynchronize(a->ctx->stream));
        SG_COPY_SYNC(a->ctx, a->d_v, pv.data(), sizeof(float) * ptot, hipMemcpyHostToDevice);
        a->opt_t = step;
        return 0;
    }
    if (pol->cnn) {
        SG_REQUIRE(n == pol->cnnd.total, "sg_a2c_set_rmsprop: bad length");
        SG_REQUIRE(step >= 0, "sg_a2c_set_rmsprop: step out of range");
        SG_CHECK(hipSetDevice(a->ctx->device));
        SG_CHECK(hipStreamSynchronize(a->ctx->stream));
        SG_COPY_SYNC(a->ctx, a->d_v, square_avg, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
        a->opt_t = step;
        return 0;
    }
    SG_REQUIRE(n == sg_policy_flat_count(d) + n_gru, "sg_a2c_set_rmsprop: bad length");
    SG_REQUIRE(step >= 0, "sg_a2c_set_rmsprop: step out of range");
    const size_t ptot = sg_policy_padded_count(pol);
    std::vector<float> pv(ptot, 0.f);
    if (pol->recurrent) sg_gru_pad(pol->gru, square_avg, pv.data() + pol->gru.off);
    sg_policy_pad(d, square_avg + n_gru, pv.data());
    SG_CHECK(hipSetDevice(a->ctx->device));
    SG_CHECK(hipStreamSynchronize(a->ctx->stream));
    SG_COPY_SYNC(a->ctx, a->d_v, pv.data(), sizeof(float) * ptot, hipMemcpyHostToDevice);
    a->opt_t = step;
    return 0;
}

// ------------------------------------------------------------------- shared by the three updates
// advantages of the rollout's T*N rows (global mean / unbiased std) into its advantage field
static int enqueue_adv_stats(sg_ctx* ctx, sg_rollout* r, sg_ppo* a, bool with_comm) {
    const int64_t TN = (int64_t)r->T * r->N;
    double* stats = a->d_loss_acc + 4;
    for (int pass = 0; pass < 3; ++pass) {
        hipLaunchKernelGGL(k_adv_stats, dim3(pass == 2 ? 64 : 1), dim3(1024), 0, ctx->stream, r->d_field[SG_F_RETURNS],
                           r->d_field[SG_F_VALUE_PREDS], TN, r->d_field[SG_F_ADVANTAGES], stats, pass);
        if (with_comm && pass == 0) SG_TRY(sg_comm_allreduce_f64(ctx, stats, 3));       // sum and n are linear
        if (with_comm && pass == 1) SG_TRY(sg_comm_allreduce_f64(ctx, stats + 1, 1));   // squares about the global mean
    }
    SG_CHECK(hipGetLastError());
    return 0;
}

// ld-padding columns of the slabs and rows past the minibatch are never written by the kernels and must read as zero; the
// epoch copy's slack rows must be finite.  Both hold for as long as the scratch layout is unchanged, so the buffers (35 MB at
// the north-star shape) are cleared when the layout differs from the one they were last cleared for, not on every update.
// gru_f: floats of d_gru the mode uses (0: none).
static int clear_for_layout(sg_ppo* a, const SgScratchLayout& layout, size_t slab_f, size_t stack_f, size_t gru_f) {
    if (memcmp(&a->cleared, &layout, sizeof layout) == 0) return 0;
    SG_CHECK(hipMemsetAsync(a->d_slabs, 0, sizeof(float) * slab_f, a->ctx->stream));
    SG_CHECK(hipMemsetAsync(a->d_stacks, 0, sizeof(float) * stack_f, a->ctx->stream));
    if (gru_f) SG_CHECK(hipMemsetAsync(a->d_gru, 0, sizeof(float) * gru_f, a->ctx->stream));
    a->cleared = layout;
    return 0;
}

// A2C_ACKTR.update(rollouts), acktr=False (a2c/algo/a2c_acktr.py:52-102): evaluate_actions on all T*N rows with the current
// parameters, adv = returns[:-1] - values, loss = vcoef mean(adv^2) + (-mean(adv.detach() logp)) - ecoef mean(ent), one
// clip_grad_norm_ + RMSprop step.  The rows are taken in chunks of SG_A2C_CHUNK_ROWS; each chunk's slabs are added to the
// gradient, so the scratch does not grow with T*N.
static int a2c_update(sg_ppo* a, sg_rollout* r, uint64_t seed, float out3[3]) {
    sg_ctx* ctx = a->ctx;
    const SgPolicyDesc& d = a->policy->desc;
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_ppo_update: A2C runs on one rank (this context's world is %d)", ctx->world);
    const int64_t TN = (int64_t)r->T * r->N;
    SG_REQUIRE(TN > 0 && TN < (1ll << 30), "sg_ppo_update: %lld rollout rows", (long long)TN);
    SG_CHECK(hipSetDevice(ctx->device));
    const int chunk = (int)std::min<int64_t>(TN, SG_A2C_CHUNK_ROWS);
    const int n_chunks = (int)((TN + chunk - 1) / chunk);
    // k_a2c_bwd: the unfused backward's tiles (w2 on in LDS), whatever ppo_fused says
    auto bwd_lds = [&](int mt, bool g) { return ppo_bwd_tiles_lds(d, mt, g ? 0 : max_bwd_floats(d), 2, false); };
    auto fits = [&](int mt, bool g) { return ppo_fwd_lds(d, mt, g) <= (size_t)ctx->lds_bytes && bwd_lds(mt, g) <= (size_t)ctx->lds_bytes; };
    const bool gw = sg_policy_needs_gw(ctx, d) || !fits(1, false);
    SG_REQUIRE(fits(1, gw), "sg_ppo_update: the 16-row tiles of the A2C step do not fit LDS");
    // row-group size: PPO's heuristic at a minibatch of `chunk` rows (two grid columns: actor, critic); SG_PPO_ROWS: 16 or 32
    const int MT = ppo_row_tiles(ctx, d, chunk, d.n_trunks, true, 2, 2, [&](int mt) { return fits(mt, gw); });
    const int R = 16 * MT;
    const int G = (chunk + R - 1) / R;   // row groups of a full chunk: the slab count
    const int mbp = G * R;
    const int ldP = stack_ldP(d);
    const int slab_stride = (d.total + 8 + 63) & ~63;
    const int TNp = (int)TN + 64;        // slack rows: the last row tile reads up to R - 1 <= 63 rows past the rollout
    const size_t slab_f = (size_t)G * slab_stride;
    const size_t epoch_f = (size_t)TNp * (d.ldO + d.A + 4);
    const size_t stack_f = (size_t)d.n_trunks * mbp * (2 * (size_t)d.ldH + ldP);
    bool grew = false;
    SG_TRY(ensure_cap(ctx->stream, &a->d_slabs, &a->slabs_cap, slab_f, &grew));
    SG_TRY(ensure_cap(ctx->stream, &a->d_stacks, &a->stacks_cap, epoch_f + stack_f, &grew));
    if (grew) a->cleared.mode = SG_LAYOUT_INVALID;
    SG_TRY(clear_for_layout(a, {SG_LAYOUT_A2C, {G, slab_stride, mbp, TNp, MT}}, slab_f, epoch_f + stack_f, 0));
    hipLaunchKernelGGL(k_zero_f64, dim3(1), dim3(64), 0, ctx->stream, a->d_loss_acc, 4);

    float* epX = a->d_stacks;
    float* epACT = epX + (size_t)TNp * d.ldO;
    float* epSC = epACT + (size_t)TNp * d.A;
    float* stk = a->d_stacks + epoch_f;

    EpochGatherArgs ga;
    memset(&ga, 0, sizeof ga);
    ga.obs = r->d_field[SG_F_OBS]; ga.actions = r->d_field[SG_F_ACTIONS]; ga.ret = r->d_field[SG_F_RETURNS];
    ga.TN = TN; ga.O = d.O; ga.Op = d.Op; ga.ldO = d.ldO; ga.A = d.A; ga.sc_stride = TNp;
    ga.X = epX; ga.ACT = epACT; ga.SC = epSC;

    PpoArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.d = d; pa.params = a->policy->d_params;
    pa.sc_stride = TNp; pa.mbp = mbp; pa.inv_B = 1.0f / (float)TN;
    pa.vcoef = a->cfg.value_loss_coef; pa.ecoef = a->cfg.entropy_coef;
    pa.slabs = a->d_slabs; pa.slab_stride = slab_stride; pa.ldP = ldP;
    pa.st = reinterpret_cast<SgOptState*>(a->d_state); pa.G = G; pa.k1 = 1;
    for (int t = 0; t < d.n_trunks; ++t) {
        pa.H1[t] = stk; stk += (size_t)mbp * d.ldH;
        pa.H2[t] = stk; stk += (size_t)mbp * d.ldH;
        pa.OUT[t] = stk; stk += (size_t)mbp * ldP;
    }
    const int wb_f = gw ? 0 : max_trunk_floats(d), wb_b = gw ? 0 : max_bwd_floats(d);
    const size_t lds_f = ppo_fwd_lds(d, MT, gw), lds_b = bwd_lds(MT, gw);
    const int nblk = (d.total + 8 + 255) / 256;
    const int nblk_r = (d.total + 8 + SG_PPO_REDUCE_PARAMS - 1) / SG_PPO_REDUCE_PARAMS;
    const double oma = 1.0 - (double)a->alpha;   // torch: value = 1 - alpha in Python doubles

    // ACKTR: the value noise of this update (injected, or drawn outside the graph), the chunk's Fisher stacks
    SgKfac* kf = a->kfac;
    AcktrFisherArgs fa;
    KfacStatsArgs sa;
    KfacEigArgs ea;
    memset(&fa, 0, sizeof fa);
    memset(&sa, 0, sizeof sa);
    memset(&ea, 0, sizeof ea);
    size_t lds_fish = 0, lds_eig = 0;
    if (kf) {
        SG_REQUIRE(!kf->eps_pending || (int64_t)kf->eps_host.size() == TN,
                   "sg_ppo_update: the injected value noise has %lld values, the rollout %lld rows", (long long)kf->eps_host.size(),
                   (long long)TN);
        const int frows = (chunk + 63) & ~63;
        const int ldZ = d.ldH;
        const size_t fish_f = (size_t)frows * (4 * (size_t)ldZ + 2 * (size_t)d.A + 1);
        SG_TRY(ensure_cap(ctx->stream, &kf->d_eps, &kf->eps_cap, TN));
        SG_TRY(ensure_cap(ctx->stream, &kf->d_fish, &kf->fish_cap, fish_f));
        if (kf->eps_pending) {
            SG_COPY_SYNC(ctx, kf->d_eps, kf->eps_host.data(), sizeof(float) * TN, hipMemcpyHostToDevice);
            kf->eps_pending = false;
            kf->eps_host.clear();
        } else {
            hipLaunchKernelGGL(k_acktr_noise, dim3((unsigned)((TN + 255) / 256)), dim3(256), 0, ctx->stream, kf->d_eps, TN, seed,
                               (int64_t)a->opt_t);
        }
        fa.d = d; fa.params = a->policy->d_params; fa.ldP = ldP; fa.ldZ = ldZ; fa.inv_B = pa.inv_B;
        float* fz = kf->d_fish;
        for (int t = 0; t < 2; ++t) {
            fa.H1[t] = pa.H1[t]; fa.H2[t] = pa.H2[t]; fa.OUT[t] = pa.OUT[t];
            fa.Z1[t] = fz; fz += (size_t)frows * ldZ;
            fa.Z2[t] = fz; fz += (size_t)frows * ldZ;
        }
        fa.GMU = fz; fz += (size_t)frows * d.A;
        fa.GLS = fz; fz += (size_t)frows * d.A;
        fa.GV = fz;
        lds_fish = sizeof(float) * SG_ACKTR_FROWS * (size_t)(d.A + d.Hp);
        const SgTrunk& ac = d.trunk[0];
        const SgTrunk& cr = d.trunk[1];
        const float* src[SG_KFAC_NF] = {nullptr, pa.H1[0], pa.H2[0], pa.H1[1], pa.H2[1], fa.Z1[0], fa.Z2[0], fa.Z1[1], fa.Z2[1],
                                        fa.GV, fa.GMU, fa.GLS};
        const int lds_[SG_KFAC_NF] = {d.ldO, ac.ldH, ac.ldH, cr.ldH, cr.ldH, ldZ, ldZ, ldZ, ldZ, 1, d.A, d.A};
        for (int f = 0; f < SG_KFAC_NF; ++f) {
            sa.U[f] = src[f]; sa.ld[f] = lds_[f]; sa.n[f] = kf->n[f]; sa.off[f] = kf->off[f];
        }
        sa.tiles = kf->d_tiles; sa.acc = kf->d_acc;
        ea = kfac_eig_args(kf);
        lds_eig = kfac_eig_lds(kf);
    }

    auto enqueue_step = [&]() -> int {
        hipLaunchKernelGGL(k_a2c_gather, dim3((unsigned)((TN + 63) / 64)), dim3(256), 0, ctx->stream, ga);
        for (int c = 0; c < n_chunks; ++c) {
            const int64_t rb = (int64_t)c * chunk;
            const int cnt = (int)std::min<int64_t>(chunk, TN - rb);
            const int Gc = (cnt + R - 1) / R;
            pa.mb = cnt;
            pa.X = epX + rb * d.ldO; pa.ACT = epACT + rb * d.A; pa.SC = epSC + rb;
            pa.wbuf_floats = wb_f;
            SG_TRY(ppo_launch(ctx, ppo_fwd_family, "k_ppo_fwd", SG_PROF_PPO_FWD, MT, d, dim3(Gc, d.n_trunks), lds_f, pa, gw));
            pa.wbuf_floats = wb_b;
            if (d.dist == SG_DIST_CATEGORICAL)
                SG_TRY(ppo_launch(ctx, a2c_bwd_cat_family, "k_a2c_bwd (categorical)", SG_PROF_PPO_BWD, MT, d, dim3(Gc, d.n_trunks), lds_b, pa, gw));
            else if (d.dist == SG_DIST_BERNOULLI)
                SG_TRY(ppo_launch(ctx, a2c_bwd_ber_family, "k_a2c_bwd (Bernoulli)", SG_PROF_PPO_BWD, MT, d, dim3(Gc, d.n_trunks), lds_b, pa, gw));
            else
                SG_TRY(ppo_launch(ctx, a2c_bwd_family, "k_a2c_bwd", SG_PROF_PPO_BWD, MT, d, dim3(Gc, d.n_trunks), lds_b, pa, gw));
            SG_LAUNCH(ctx, SG_PROF_PPO_REDUCE, k_a2c_reduce, dim3(nblk_r), dim3(256), 0, a->d_slabs, Gc, slab_stride, d.total, a->d_grad,
                      a->d_part, c > 0 ? 1 : 0);
            if (kf) {
                fa.ACT = epACT + rb * d.A; fa.eps = kf->d_eps + rb; fa.cnt = cnt;
                hipLaunchKernelGGL(k_acktr_fisher, dim3((unsigned)((cnt + SG_ACKTR_FROWS - 1) / SG_ACKTR_FROWS), 2), dim3(256),
                                   lds_fish, ctx->stream, fa);
                sa.U[0] = epX + rb * d.ldO; sa.cnt = cnt; sa.accumulate = c > 0 ? 1 : 0;
                hipLaunchKernelGGL(k_kfac_stats, dim3((unsigned)kf->n_tiles), dim3(64 * SG_KFAC_STATS_WAVES), 0, ctx->stream, sa);
            }
        }
        if (kf) {
            const sg_acktr_config& kc = kf->cfg;
            const double sd = (double)kc.stat_decay;
            hipLaunchKernelGGL(k_kfac_fold, dim3((unsigned)((kf->fac_total + 255) / 256)), dim3(256), 0, ctx->stream, kf->d_m,
                               kf->d_acc, kf->fac_total, kf->g_start, pa.inv_B, (float)TN, kf->d_ks, kc.stat_decay, (float)(1.0 - sd));
            hipLaunchKernelGGL(k_kfac_eig, dim3(SG_KFAC_NF), dim3(512), lds_eig, ctx->stream, ea);
            for (int st = 0; st < 4; ++st)
                hipLaunchKernelGGL(k_kfac_gemm, dim3((unsigned)kf->max_tiles, SG_KFAC_MODULES), dim3(256), 0, ctx->stream,
                                   kf->d_jobs + st * SG_KFAC_MODULES, kf->max_tiles, kc.damping, kf->d_vpart);
            const double mom = (double)kc.momentum;
            hipLaunchKernelGGL(k_kfac_step, dim3((unsigned)nblk), dim3(256), 0, ctx->stream, a->policy->d_params, a->d_m,
                               kf->d_vec, kf->d_vpart, SG_KFAC_MODULES * kf->max_tiles, d.total, kf->d_ks, kc.lr, kc.kl_clip,
                               kc.momentum, (float)((double)kc.lr * (1.0 - mom)));
            hipLaunchKernelGGL(k_kfac_tick, dim3(1), dim3(64), 0, ctx->stream, kf->d_ks, a->d_grad, d.total, pa.inv_B,
                               a->d_loss_acc);
            return 0;
        }
        SG_LAUNCH(ctx, SG_PROF_PPO_ADAM, k_a2c_rmsprop, dim3(nblk), dim3(256), 0, a->policy->d_params, a->d_v, a->d_grad, a->d_part,
                  nblk_r, d.total, pa.st, a->alpha, (float)oma, a->cfg.eps, a->cfg.max_grad_norm, pa.inv_B, a->d_loss_acc);
        return 0;
    };
    const bool use_graph = !ctx->use_comm && !ctx->profile && !sg_env_is_off("SG_PPO_GRAPH");
    uint32_t fbits[6];
    const float fv[6] = {a->alpha, a->cfg.value_loss_coef, a->cfg.entropy_coef, a->cfg.eps, a->cfg.max_grad_norm, pa.inv_B};
    memcpy(fbits, fv, sizeof fbits);
    const uint64_t key[SG_GRAPH_KEY_WORDS] = {
            (uint64_t)(uintptr_t)a->d_slabs, (uint64_t)(uintptr_t)a->d_stacks, 0,
            (uint64_t)(uintptr_t)r->d_field[SG_F_OBS], (uint64_t)(uintptr_t)r->d_field[SG_F_ACTIONS],
            (uint64_t)(uintptr_t)r->d_field[SG_F_RETURNS], (uint64_t)(uintptr_t)a->policy->d_params,
            (uint64_t)TN, ((uint64_t)n_chunks << 32) | (uint64_t)chunk, ((uint64_t)MT << 32) | (uint64_t)G,
            ((uint64_t)fbits[0] << 32) | fbits[1], ((uint64_t)fbits[2] << 32) | fbits[3],
            ((uint64_t)fbits[4] << 32) | fbits[5], kf ? (uint64_t)(uintptr_t)kf->d_eps : 0,
            kf ? (uint64_t)(uintptr_t)kf->d_fish : 0, 0x413243ull + (gw ? 8 : 0) + (1ull << 7) + (kf ? (1ull << 9) : 0),
            0, 0};
    SG_TRY(sg_graph_run(ctx, &a->steps_graph, use_graph, key, enqueue_step));
    SG_CHECK(hipGetLastError());
    a->opt_t += 1;
    if (!out3) return 0;   // queued: the losses come through the results ring (step count 1)
    double acc[4];
    SG_TRY(sg_ctx_fetch_f64(ctx, a->d_loss_acc, acc, kf ? 4 : 3));
    for (int i = 0; i < 3; ++i) out3[i] = (float)acc[i];
    SG_REQUIRE(!kf || acc[3] == 0.0, "sg_ppo_update: k_kfac_eig hit its sweep cap (%d): the K-FAC eigenbases are not valid",
               SG_KFAC_SWEEPS);
    return 0;
}

// ------------------------------------------------------------------- PPO through time (recurrent policy)
// rollouts.recurrent_hidden_states[0] ([N][H], a2c/storage.py:216-217: the minibatches start from the state of slot 0) for the
// NEXT sg_ppo_update of a recurrent policy; the rollout's device twin has no hidden-state field, so the caller hands it over
extern "C" int sg_ppo_set_hidden_states(sg_ppo* a, const float* hxs0, int64_t count) {
    SG_REQUIRE(a && hxs0, "sg_ppo_set_hidden_states: NULL argument");
    SG_REQUIRE(a->policy->recurrent, "sg_ppo_set_hidden_states: the policy is feed-forward: it has no hidden state");
    const int H = a->policy->gru.H;
    SG_REQUIRE(count > 0 && count % H == 0, "sg_ppo_set_hidden_states: %lld floats is not a whole number of %d-float states",
               (long long)count, H);
    sg_ctx* ctx = a->ctx;
    SG_CHECK(hipSetDevice(ctx->device));
    if (a->h0_cap < count) {
        SG_DEVICE_WIDE();
        SG_CHECK(hipStreamSynchronize(ctx->stream));
        if (a->d_h0) SG_CHECK(sg_dev_free(a->d_h0));
        if (a->h_h0) SG_CHECK(sg_host_release(a->h_h0));
        a->d_h0 = nullptr; a->h_h0 = nullptr; a->h0_cap = 0;
        SG_CHECK(sg_dev_malloc((void**)&a->d_h0, sizeof(float) * count));
        SG_CHECK(sg_host_malloc((void**)&a->h_h0, sizeof(float) * count * SG_H0_SLOTS));
        a->h0_cap = count;
    }
    // No host wait for the queued updates: the states go through one of SG_H0_SLOTS page-locked staging slots and an asynchronous
    // copy in stream order (behind the previous update's reads); a slot is reused only once its own copy has run.
    const int slot = (int)(a->h0_calls++ % SG_H0_SLOTS);
    if (!a->h0_ev[slot]) SG_CHECK(hipEventCreateWithFlags(&a->h0_ev[slot], hipEventDisableTiming));
    else SG_CHECK(hipEventSynchronize(a->h0_ev[slot]));
    float* stage = a->h_h0 + (size_t)slot * a->h0_cap;
    memcpy(stage, hxs0, sizeof(float) * count);
    SG_CHECK(hipMemcpyAsync(a->d_h0, stage, sizeof(float) * count, hipMemcpyHostToDevice, ctx->stream));
    SG_CHECK(hipEventRecord(a->h0_ev[slot], ctx->stream));
    a->h0_count = count;
    return 0;
}

// The same hand-over from a rollout that holds its hidden states on the device (sg_rollout_enable_hidden): slot 0 goes into
// d_h0 device to device, in stream order; the host neither reads a state nor waits.
extern "C" int sg_ppo_set_hidden_states_rollout(sg_ppo* a, sg_rollout* r) {
    SG_REQUIRE(a && r, "sg_ppo_set_hidden_states_rollout: NULL argument");
    SG_REQUIRE(a->policy->recurrent, "sg_ppo_set_hidden_states_rollout: the policy is feed-forward: it has no hidden state");
    SG_REQUIRE(a->ctx == r->ctx, "sg_ppo_set_hidden_states_rollout: the agent and the rollout live on different contexts");
    const int H = a->policy->gru.H;
    SG_REQUIRE(r->d_hidden, "sg_ppo_set_hidden_states_rollout: the rollout holds no hidden states (sg_rollout_enable_hidden)");
    SG_REQUIRE(r->hidden_dim == H, "sg_ppo_set_hidden_states_rollout: the rollout's hidden states are %d wide, the policy's %d",
               r->hidden_dim, H);
    sg_ctx* ctx = a->ctx;
    const int64_t count = (int64_t)r->N * H;
    SG_CHECK(hipSetDevice(ctx->device));
    if (a->h0_cap < count) {
        SG_DEVICE_WIDE();
        SG_CHECK(hipStreamSynchronize(ctx->stream));
        if (a->d_h0) SG_CHECK(sg_dev_free(a->d_h0));
        if (a->h_h0) SG_CHECK(sg_host_release(a->h_h0));
        a->d_h0 = nullptr; a->h_h0 = nullptr; a->h0_cap = 0;
        SG_CHECK(sg_dev_malloc((void**)&a->d_h0, sizeof(float) * count));
        SG_CHECK(sg_host_malloc((void**)&a->h_h0, sizeof(float) * count * SG_H0_SLOTS));
        a->h0_cap = count;
    }
    SG_CHECK(hipMemcpyAsync(a->d_h0, r->d_hidden, sizeof(float) * count, hipMemcpyDeviceToDevice, ctx->stream));
    a->h0_count = count;
    return 0;
}

// PPO.update with actor_critic.is_recurrent (a2c/algo/ppo.py:74-90) over RolloutStorage.recurrent_generator's minibatches
// (a2c/storage.py:194-251): per = N // num_mini_batch whole environments per optimizer step, N // per steps per epoch.
//   k_adv_stats x3
//   per epoch:  k_gru_epoch_gather            environment-permuted, time-major copy of the rollout
//   per step:   k_gru_inproj -> k_gru_scan_fwd<TRAIN> (h_t = the heads' input rows) -> k_ppo_bwd<fused, DX> (a Categorical /
//               Bernoulli head: k_ppo_bwd_dist_dx) -> k_ppo_reduce
//               -> k_gru_scan_bwd -> k_gru_wgrad -> k_gru_reduce -> k_ppo_adam over heads + GRU (one norm, one clip)
//   then        k_opt_commit
// All of it from the first gather on is one captured graph, replayed per update; no host wait inside.
static int gru_ppo_update(sg_ppo* a, sg_rollout* r, const int64_t* perms, int64_t n_perms, uint64_t seed, float out3[3]) {
    sg_ctx* ctx = a->ctx;
    sg_policy* pol = a->policy;
    const SgPolicyDesc& d = pol->desc;
    const SgGruDesc& g = pol->gru;
    SG_REQUIRE(r->O == g.O && r->A == d.A, "sg_ppo_update: rollout dims (obs %d, act %d) do not match the policy (%d, %d)", r->O, r->A,
               g.O, d.A);
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_ppo_update: PPO with a recurrent policy runs on one rank (world %d)", ctx->world);
    const int T = r->T, N = r->N, M = a->cfg.num_mini_batch, E = a->cfg.ppo_epoch;
    // a2c/storage.py:196-199
    SG_REQUIRE(N >= M, "PPO requires the number of processes (%d) to be greater than or equal to the number of PPO mini batches (%d).", N, M);
    const int per = N / M;
    SG_REQUIRE(N % per == 0, "sg_ppo_update: %d processes do not split into minibatches of %d = %d // %d environments (the reference "
               "indexes past its permutation here)", N, per, N, M);
    const int S = N / per;                        // optimizer steps per epoch (a2c/storage.py:202: range(0, N, per))
    SG_REQUIRE((int64_t)a->h0_count == (int64_t)N * g.H, "sg_ppo_update: a recurrent policy takes the hidden states of rollout slot 0 "
               "from the host: sg_ppo_set_hidden_states must hand over %lld floats before every update (pending: %lld)",
               (long long)N * g.H, (long long)a->h0_count);
    a->h0_count = 0;
    const int64_t TN = (int64_t)T * N;
    SG_REQUIRE(TN < (1ll << 30), "sg_ppo_update: rollout too large");
    if (perms) {
        SG_REQUIRE(n_perms == (int64_t)E * N, "sg_ppo_update: perms holds %lld indices, %d epochs x %d environments need %lld",
                   (long long)n_perms, E, N, (long long)E * N);
        std::vector<uint8_t> seen((size_t)N);
        for (int e = 0; e < E; ++e) {
            std::fill(seen.begin(), seen.end(), (uint8_t)0);
            for (int i = 0; i < N; ++i) {
                const int64_t v = perms[(size_t)e * N + i];
                SG_REQUIRE(v >= 0 && v < N && !seen[(size_t)v], "sg_ppo_update: perms of epoch %d are not a permutation of the %d environments", e, N);
                seen[(size_t)v] = 1;
            }
        }
    }
    SG_CHECK(hipSetDevice(ctx->device));

    // advantages (global mean / unbiased std over all T*N, as for the feed-forward update)
    SG_TRY(enqueue_adv_stats(ctx, r, a, false));

    // permutations of the environments: [E][N]
    SG_TRY(ensure_cap(ctx->stream, &a->d_perms, &a->perms_cap, (int64_t)E * N));
    a->last_perm_count = (int64_t)E * N;
    if (perms) {
        SG_CHECK(hipMemcpyAsync(a->d_perms, perms, sizeof(int64_t) * (size_t)E * N, hipMemcpyHostToDevice, ctx->stream));
        if (!out3) SG_CHECK(hipStreamSynchronize(ctx->stream));
    } else {
        for (int e = 0; e < E; ++e) SG_TRY(sg_fill_perm(ctx, a->d_perms + (size_t)e * N, N, seed, (uint64_t)e * 2654435761ull));
    }

    // geometry.  Heads: the fused forward + backward on 16- or 32-row groups of the step's T*per rows.  Scans: one workgroup per
    // 16 environments of the minibatch.
    const int mb = T * per;
    // (a Categorical / Bernoulli head: the actor trunk carries an n_out-wide head beside w1, so the whole fused tile set decides,
    // not the forward's alone -- what does not fit a CU's LDS takes the global-weight instances)
    const bool dist_heads = d.dist != SG_DIST_GAUSSIAN;
    const bool gw = sg_policy_needs_gw(ctx, d) || ppo_fwd_lds(d, 1, false) > (size_t)ctx->lds_bytes ||
                    (dist_heads && ppo_bwd_tiles_lds(d, 1, max_trunk_floats(d), 2, false) > (size_t)ctx->lds_bytes);
    const int ldP = stack_ldP(d);
    auto bwd_lds = [&](int mt) { return ppo_bwd_tiles_lds(d, mt, gw ? 0 : max_trunk_floats(d), 2, false); };   // the fused form
    // (neither SG_PPO_ROWS nor the 24 MB slab rule here; 32-row groups fall back to 16-row ones only.  The Categorical / Bernoulli
    // heads read SG_PPO_ROWS = 16 / 32, as their feed-forward step does.)
    const int MT = ppo_row_tiles(ctx, d, mb, d.n_trunks, false, dist_heads ? 2 : 0, 2, [&](int mt) { return bwd_lds(mt) <= (size_t)ctx->lds_bytes; });
    SG_REQUIRE(bwd_lds(MT) <= (size_t)ctx->lds_bytes, "sg_ppo_update: the heads' 16-row tiles do not fit LDS (%zu bytes)", bwd_lds(MT));
    const int R = 16 * MT, G = (mb + R - 1) / R, mbp = G * R;
    const int slab_stride = (d.total + 8 + 63) & ~63;
    const int TNp = (int)TN + 64;
    const int rows_p = (mb + 15) & ~15;
    const int Hp = g.Hp, G3 = 3 * Hp;
    const int chunks = rows_p / 16;
    const int KS = std::max(1, std::min(16, chunks / 8));
    const int gblocks = (g.total + 255) / 256;
    const int nblk_r = (d.total + 8 + SG_PPO_REDUCE_PARAMS - 1) / SG_PPO_REDUCE_PARAMS;
    const int tot_all = d.total + g.total;
    const int nblk = (tot_all + 8 + 255) / 256;

    // scratch: slabs; d_stacks = heads' input rows | ACT | SC; d_gru = everything of the GRU
    const size_t slab_f = (size_t)G * slab_stride;
    const size_t hx_f = (size_t)(mbp + 64) * d.ldO;
    const size_t stack_f = hx_f + (size_t)TNp * d.A + 4 * (size_t)TNp;
    auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t o_x = 0, o_mk = o_x + r4((size_t)TNp * g.ldO), o_h0 = o_mk + r4((size_t)TNp), o_gi = o_h0 + r4((size_t)N * g.H);
    const size_t o_sr = o_gi + (size_t)rows_p * G3, o_sz = o_sr + (size_t)rows_p * Hp, o_sn = o_sz + (size_t)rows_p * Hp;
    const size_t o_shn = o_sn + (size_t)rows_p * Hp, o_hm = o_shn + (size_t)rows_p * Hp, o_dgi = o_hm + (size_t)rows_p * g.ldH;
    const size_t o_dgh = o_dgi + (size_t)rows_p * G3, o_dxa = o_dgh + (size_t)rows_p * G3, o_dxc = o_dxa + (size_t)mbp * d.ldO;
    const size_t o_part = o_dxc + (size_t)mbp * d.ldO, gru_f = o_part + (size_t)KS * g.total;
    bool grew = false;
    SG_TRY(ensure_cap(ctx->stream, &a->d_slabs, &a->slabs_cap, slab_f, &grew));
    SG_TRY(ensure_cap(ctx->stream, &a->d_stacks, &a->stacks_cap, stack_f, &grew));
    SG_TRY(ensure_cap(ctx->stream, &a->d_gru, &a->gru_cap, gru_f, &grew));
    if (grew) a->cleared.mode = SG_LAYOUT_INVALID;
    SG_TRY(clear_for_layout(a, {SG_LAYOUT_GRU, {G, slab_stride, mbp, TNp, MT, KS, per, ((int64_t)g.total << 32) | (int64_t)rows_p}},
                            slab_f, stack_f, gru_f));
    hipLaunchKernelGGL(k_zero_f64, dim3(1), dim3(64), 0, ctx->stream, a->d_loss_acc, 4);

    float* hX = a->d_stacks;
    float* epACT = hX + hx_f;
    float* epSC = epACT + (size_t)TNp * d.A;
    float* gb = a->d_gru;

    GruGatherArgs ga;
    ga.obs = r->d_field[SG_F_OBS]; ga.actions = r->d_field[SG_F_ACTIONS]; ga.old_logp = r->d_field[SG_F_LOGP];
    ga.adv = r->d_field[SG_F_ADVANTAGES];
    ga.vpred = r->d_field[SG_F_VALUE_PREDS]; ga.ret = r->d_field[SG_F_RETURNS]; ga.masks = r->d_field[SG_F_MASKS]; ga.h0 = a->d_h0;
    ga.T = T; ga.N = N; ga.per = per; ga.O = g.O; ga.ldO = g.ldO; ga.A = d.A; ga.H = g.H; ga.sc_stride = TNp;
    ga.X = gb + o_x; ga.ACT = epACT; ga.SC = epSC; ga.MK = gb + o_mk; ga.H0 = gb + o_h0;

    PpoArgs pa;
    pa.d = d; pa.params = pol->d_params;
    pa.sc_stride = TNp; pa.mb = mb; pa.mbp = mbp; pa.inv_B = 1.0f / (float)mb;
    pa.clip = a->cfg.clip_param; pa.vcoef = a->cfg.value_loss_coef; pa.ecoef = a->cfg.entropy_coef;
    pa.use_clipped = a->cfg.use_clipped_value_loss;
    pa.slabs = a->d_slabs; pa.slab_stride = slab_stride; pa.ldP = ldP;
    pa.st = reinterpret_cast<SgOptState*>(a->d_state); pa.G = G; pa.k1 = 0;
    pa.pair = a->d_pair; pa.Xm = nullptr; pa.MA = nullptr; pa.sym_c = 0.f;
    for (int t = 0; t < 3; ++t) { pa.H1[t] = hX; pa.H2[t] = hX; pa.OUT[t] = hX; }   // the fused form keeps its activations in LDS
    pa.X = hX;
    pa.DX[0] = gb + o_dxa; pa.DX[1] = gb + o_dxc;
    pa.wbuf_floats = gw ? 0 : max_trunk_floats(d);

    GruScanArgs tr;
    tr.sr = gb + o_sr; tr.sz = gb + o_sz; tr.sn = gb + o_sn; tr.shn = gb + o_shn; tr.hm = gb + o_hm;
    GruBwdArgs ba;
    ba.g = g; ba.W = pol->d_params + g.off; ba.dxa = gb + o_dxa; ba.dxc = gb + o_dxc; ba.dx_ld = d.ldO;
    ba.sr = tr.sr; ba.sz = tr.sz; ba.sn = tr.sn; ba.shn = tr.shn; ba.hm = tr.hm; ba.T = T; ba.n = per;
    ba.dgi = gb + o_dgi; ba.dgh = gb + o_dgh;
    GruWgradArgs wa;
    wa.g = g; wa.dgi = ba.dgi; wa.dgh = ba.dgh; wa.hm = tr.hm; wa.rows_p = rows_p; wa.KS = KS; wa.partial = gb + o_part;
    const bool gw_scan = sg_gru_force_gw() || sg_gru_scan_lds(g, false) > (size_t)ctx->lds_bytes - 1024 ||
                         sg_gru_bwd_lds(g, false) > (size_t)ctx->lds_bytes - 1024;
    const int n_tiles = (G3 / 16) * (g.Op / 16 + Hp / 16) + 2 * (G3 / 16);
    const size_t lds_b = bwd_lds(MT);
    SgOptState* st = reinterpret_cast<SgOptState*>(a->d_state);

    auto enqueue_steps = [&]() -> int {
        hipLaunchKernelGGL(k_opt_prepare_first, dim3(1), dim3(1), 0, ctx->stream, st);
        for (int e = 0; e < E; ++e) {
            ga.perm = a->d_perms + (size_t)e * N;
            hipLaunchKernelGGL(k_gru_epoch_gather<0>, dim3((unsigned)TN), dim3(64), 0, ctx->stream, ga);
            for (int k = 0; k < S; ++k) {
                const size_t rb = (size_t)k * mb;
                const float* xk = gb + o_x + rb * g.ldO;
                const float* mk = gb + o_mk + rb;
                SG_TRY(sg_gru_forward_launch(ctx, g, pol->d_params + g.off, xk, g.ldO, gb + o_h0 + (size_t)k * per * g.H, mk, T, per,
                                             gb + o_gi, hX, d.ldO, nullptr, &tr));
                pa.ACT = epACT + rb * d.A; pa.SC = epSC + rb;
                pa.k1 = e * S + k + 1;
                if (d.dist == SG_DIST_CATEGORICAL)
                    SG_TRY(ppo_launch(ctx, ppo_bwd_fused_cat_dx_family, "k_ppo_bwd_dist_dx (Categorical)", SG_PROF_PPO_BWD, MT, d, dim3(G, 2),
                                      lds_b, pa, gw));
                else if (d.dist == SG_DIST_BERNOULLI)
                    SG_TRY(ppo_launch(ctx, ppo_bwd_fused_ber_dx_family, "k_ppo_bwd_dist_dx (Bernoulli)", SG_PROF_PPO_BWD, MT, d, dim3(G, 2),
                                      lds_b, pa, gw));
                else
                    SG_TRY(ppo_launch(ctx, ppo_bwd_fused_dx_family, "k_ppo_bwd (fused, with d loss / d h)", SG_PROF_PPO_BWD, MT, d, dim3(G, 2),
                                      lds_b, pa, gw));
                SG_LAUNCH(ctx, SG_PROF_PPO_REDUCE, k_ppo_reduce, dim3(nblk_r), dim3(256), 0, a->d_slabs, G, slab_stride, d.total, a->d_grad,
                          a->d_part);
                ba.masks = mk;
                if (gw_scan) hipLaunchKernelGGL(k_gru_scan_bwd<true>, dim3((per + 15) / 16), dim3(256), sg_gru_bwd_lds(g, true), ctx->stream, ba);
                else hipLaunchKernelGGL(k_gru_scan_bwd<false>, dim3((per + 15) / 16), dim3(256), sg_gru_bwd_lds(g, false), ctx->stream, ba);
                wa.x = xk;
                hipLaunchKernelGGL(k_gru_wgrad<0>, dim3(n_tiles, KS), dim3(64), 0, ctx->stream, wa);
                hipLaunchKernelGGL(k_gru_reduce<0>, dim3(gblocks), dim3(256), 0, ctx->stream, wa.partial, KS, g.total, a->d_grad, d.total,
                                   a->d_part, nblk_r);
                SG_LAUNCH(ctx, SG_PROF_PPO_ADAM, k_ppo_adam, dim3(nblk), dim3(256), 0, pol->d_params, a->d_m, a->d_v, a->d_grad, a->d_part,
                          nblk_r + gblocks, tot_all, st, e * S + k + 1, a->cfg.eps, a->cfg.max_grad_norm, pa.inv_B, a->d_loss_acc);
            }
        }
        hipLaunchKernelGGL(k_opt_commit, dim3(1), dim3(1), 0, ctx->stream, st, E * S);
        SG_CHECK(hipGetLastError());
        return 0;
    };
    const bool use_graph = !ctx->profile && !sg_env_is_off("SG_PPO_GRAPH");
    uint32_t fbits[6];
    const float fv[6] = {a->cfg.clip_param, a->cfg.value_loss_coef, a->cfg.entropy_coef, a->cfg.eps, a->cfg.max_grad_norm, pa.inv_B};
    memcpy(fbits, fv, sizeof fbits);
    const uint64_t key[SG_GRAPH_KEY_WORDS] = {
            (uint64_t)(uintptr_t)a->d_slabs, (uint64_t)(uintptr_t)a->d_stacks, (uint64_t)(uintptr_t)a->d_perms,
            (uint64_t)(uintptr_t)r->d_field[SG_F_OBS], (uint64_t)(uintptr_t)r->d_field[SG_F_ACTIONS],
            (uint64_t)(uintptr_t)r->d_field[SG_F_RETURNS], (uint64_t)(uintptr_t)pol->d_params,
            (uint64_t)TN, ((uint64_t)E << 32) | (uint64_t)M, ((uint64_t)MT << 32) | (uint64_t)G,
            ((uint64_t)fbits[0] << 32) | fbits[1], ((uint64_t)fbits[2] << 32) | fbits[3],
            ((uint64_t)fbits[4] << 32) | fbits[5], (uint64_t)a->cfg.use_clipped_value_loss,
            (uint64_t)(uintptr_t)r->d_field[SG_F_LOGP],
            // 'GRU': the recurrent step sequence; the head's distribution (0 for the Gaussian: its key is what it was)
            0x475255ull + (gw ? 8 : 0) + (gw_scan ? 16 : 0) + ((uint64_t)d.dist << 24) + ((uint64_t)N << 32),
            (uint64_t)(uintptr_t)a->d_gru, (uint64_t)(uintptr_t)a->d_h0 ^ ((uint64_t)(uintptr_t)r->d_field[SG_F_MASKS] << 1)};
    SG_TRY(sg_graph_run(ctx, &a->steps_graph, use_graph, key, enqueue_steps));
    SG_CHECK(hipGetLastError());
    a->opt_t += (int64_t)E * S;
    if (!out3) return 0;
    double acc[3];
    SG_TRY(sg_ctx_fetch_f64(ctx, a->d_loss_acc, acc, 3));
    const double nu = (double)E * M;   // a2c/algo/ppo.py:151-155 divides by ppo_epoch * num_mini_batch whatever N // per is
    for (int i = 0; i < 3; ++i) out3[i] = (float)(acc[i] / nu);
    return 0;
}

// PPO.update(rollouts) on the CNN base (a2c/algo/ppo.py:63-160 with a2c/storage.py:144-192's feed-forward sampler; the network:
// a2c/model.py:204-230): ppo_epoch x num_mini_batch optimizer steps on minibatches of T*N // num_mini_batch rows.
//   k_adv_stats x3
//   per step:  the forward of sg_cnn.hip on the step's rows (read in place from the rollout through the permutation: no epoch
//              copy of the 28 K-float observations) -> k_cnn_head_loss -> head, FC, conv3, conv2, conv1 gradients, each weight
//              gradient as slabs + k_cnn_reduce -> k_sumsq -> k_ppo_adam over the one flat gradient (one norm, one clip)
//   then       k_opt_commit
// All of it behind the permutations is one captured graph, replayed per update; no host wait inside.  The activation and
// gradient stacks are 41 K floats per minibatch row: minibatches of more than SG_CNN_MAX_MB rows are refused.
#define SG_CNN_MAX_MB 4096
static int cnn_ppo_update(sg_ppo* a, sg_rollout* r, const int64_t* perms, int64_t n_perms, uint64_t seed, float out3[3]) {
    sg_ctx* ctx = a->ctx;
    sg_policy* pol = a->policy;
    const SgPolicyDesc& d = pol->desc;
    const SgCnnDesc& c = pol->cnnd;
    SG_REQUIRE(r->O == d.O && r->A == d.A, "sg_ppo_update: rollout dims (obs %d, act %d) do not match the policy (%d, %d)", r->O, r->A,
               d.O, d.A);
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_ppo_update: PPO on the CNN base runs on one rank (world %d)", ctx->world);
    const int64_t TN = (int64_t)r->T * r->N;
    const int M = a->cfg.num_mini_batch, E = a->cfg.ppo_epoch;
    SG_REQUIRE(TN >= M, "PPO requires the number of processes (%d) * number of steps (%d) = %lld to be greater than "
               "or equal to the number of PPO mini batches (%d).", r->N, r->T, (long long)TN, M);
    SG_REQUIRE(TN < (1ll << 30), "sg_ppo_update: rollout too large");
    const int mb = (int)(TN / M);
    SG_REQUIRE(mb <= SG_CNN_MAX_MB, "sg_ppo_update: a minibatch of %d rows on the CNN base exceeds %d (its activation stacks are "
               "158 KB per row): raise num_mini_batch", mb, SG_CNN_MAX_MB);
    if (perms) {
        SG_REQUIRE(n_perms == (int64_t)E * TN, "sg_ppo_update: perms holds %lld indices, %d epochs x %lld rows need %lld",
                   (long long)n_perms, E, (long long)TN, (long long)E * TN);
        for (int64_t i = 0; i < n_perms; ++i)
            SG_REQUIRE(perms[i] >= 0 && perms[i] < TN, "sg_ppo_update: perms[%lld] = %lld is outside [0, %lld)", (long long)i,
                       (long long)perms[i], (long long)TN);
    }
    SG_CHECK(hipSetDevice(ctx->device));
    SG_TRY(enqueue_adv_stats(ctx, r, a, false));
    SG_TRY(ensure_cap(ctx->stream, &a->d_perms, &a->perms_cap, (int64_t)E * TN));
    a->last_perm_count = (int64_t)E * TN;
    if (perms) {
        SG_CHECK(hipMemcpyAsync(a->d_perms, perms, sizeof(int64_t) * (size_t)E * TN, hipMemcpyHostToDevice, ctx->stream));
        if (!out3) SG_CHECK(hipStreamSynchronize(ctx->stream));
    } else {
        for (int e = 0; e < E; ++e) SG_TRY(sg_fill_perm(ctx, a->d_perms + (size_t)e * TN, TN, seed, (uint64_t)e * 2654435761ull));
    }
    // scratch: head stacks | activation stacks | gradient stacks and slabs
    const int hld = d.trunk[0].Pp > 16 ? d.trunk[0].Pp : 16;
    const size_t heads_f = 2 * (size_t)mb * hld, fwd_f = sg_cnn_fwd_floats(c, mb), bwd_f = sg_cnn_bwd_floats(c, mb);
    bool grew = false;
    SG_TRY(ensure_cap(ctx->stream, &a->d_stacks, &a->stacks_cap, heads_f + fwd_f + bwd_f, &grew));
    if (grew) a->cleared.mode = SG_LAYOUT_INVALID;
    float* heads = a->d_stacks;
    float* act = heads + heads_f;
    float* bwd = act + fwd_f;
    hipLaunchKernelGGL(k_zero_f64, dim3(1), dim3(64), 0, ctx->stream, a->d_loss_acc, 4);
    const float inv_B = 1.0f / (float)mb;
    const int nblk = (c.total + 255) / 256;
    SgOptState* st = reinterpret_cast<SgOptState*>(a->d_state);
    const float* obs = r->d_field[SG_F_OBS];

    auto enqueue_steps = [&]() -> int {
        hipLaunchKernelGGL(k_opt_prepare_first, dim3(1), dim3(1), 0, ctx->stream, st);
        for (int e = 0; e < E; ++e)
            for (int k = 0; k < M; ++k) {
                const int64_t* idx = a->d_perms + (size_t)e * TN + (size_t)k * mb;
                SG_TRY(sg_cnn_forward_launch(ctx, pol, obs, idx, mb, act, heads, hld, 0, mb));
                SG_TRY(sg_cnn_backward_launch(ctx, pol, r, obs, idx, mb, act, heads, hld, bwd, a->d_grad, inv_B, a->cfg.clip_param,
                                              a->cfg.value_loss_coef, a->cfg.entropy_coef, a->cfg.use_clipped_value_loss, 0, 0, 0));
                hipLaunchKernelGGL(k_sumsq, dim3(nblk), dim3(256), 0, ctx->stream, a->d_grad, c.total, a->d_part);
                SG_LAUNCH(ctx, SG_PROF_PPO_ADAM, k_ppo_adam, dim3(nblk), dim3(256), 0, pol->d_params, a->d_m, a->d_v, a->d_grad, a->d_part,
                          nblk, c.total, st, e * M + k + 1, a->cfg.eps, a->cfg.max_grad_norm, inv_B, a->d_loss_acc);
            }
        hipLaunchKernelGGL(k_opt_commit, dim3(1), dim3(1), 0, ctx->stream, st, E * M);
        SG_CHECK(hipGetLastError());
        return 0;
    };
    const bool use_graph = !ctx->profile && !sg_env_is_off("SG_PPO_GRAPH");
    uint32_t fbits[6];
    const float fv[6] = {a->cfg.clip_param, a->cfg.value_loss_coef, a->cfg.entropy_coef, a->cfg.eps, a->cfg.max_grad_norm, inv_B};
    memcpy(fbits, fv, sizeof fbits);
    const uint64_t key[SG_GRAPH_KEY_WORDS] = {
            (uint64_t)(uintptr_t)a->d_stacks, (uint64_t)(uintptr_t)a->d_grad, (uint64_t)(uintptr_t)a->d_perms,
            (uint64_t)(uintptr_t)r->d_field[SG_F_OBS], (uint64_t)(uintptr_t)r->d_field[SG_F_ACTIONS],
            (uint64_t)(uintptr_t)r->d_field[SG_F_RETURNS], (uint64_t)(uintptr_t)pol->d_params,
            (uint64_t)TN, ((uint64_t)E << 32) | (uint64_t)M, (uint64_t)mb,
            ((uint64_t)fbits[0] << 32) | fbits[1], ((uint64_t)fbits[2] << 32) | fbits[3],
            ((uint64_t)fbits[4] << 32) | fbits[5], (uint64_t)a->cfg.use_clipped_value_loss,
            (uint64_t)(uintptr_t)r->d_field[SG_F_LOGP],
            0x434E4Eull + ((uint64_t)r->N << 32),   // 'CNN': the convolutional step sequence
            (uint64_t)(uintptr_t)r->d_field[SG_F_VALUE_PREDS], (uint64_t)(uintptr_t)r->d_field[SG_F_ADVANTAGES]};
    SG_TRY(sg_graph_run(ctx, &a->steps_graph, use_graph, key, enqueue_steps));
    SG_CHECK(hipGetLastError());
    a->opt_t += (int64_t)E * M;
    if (!out3) return 0;
    double acc[3];
    SG_TRY(sg_ctx_fetch_f64(ctx, a->d_loss_acc, acc, 3));
    const double nu = (double)E * M;
    for (int i = 0; i < 3; ++i) out3[i] = (float)(acc[i] / nu);
    return 0;
}

// PPO.update on the recurrent CNN base (a2c/algo/ppo.py:74-90 over RolloutStorage.recurrent_generator, a2c/storage.py:194-251; the
// network: a2c/model.py:117-230 with recurrent=True): per = N // num_mini_batch whole environments per optimizer step, time-major.
//   k_adv_stats x3, the environment permutations [E][N]            (checks, per, S and the loss division as in gru_ppo_update)
//   per step:  k_cnn_gru_index          row t * per + j -> rollout row t * N + perm[k * per + j]; masks and h0 gathered.  The frames
//                                       and the per-row scalars are read in place through the index: no epoch copy of observations
//              the CNN trunk's forward (sg_cnn.hip) -> k_gru_pad_rows (F as padded rows) -> k_gru_inproj -> k_gru_scan_fwd<TRAIN>
//              -> k_cnn_head_fwd on h_t -> k_cnn_head_loss -> k_cnn_head_dh (d loss / d h_t, no ReLU mask) -> k_cnn_head_wgrad
//              -> k_gru_scan_bwd -> k_gru_wgrad (x = F) -> k_gru_dx (dZf = (dGI W_ih) [F > 0]) -> the trunk's backward from dZf
//              -> k_sumsq over the flat block, k_gru_reduce behind it -> k_ppo_adam over both blocks (one norm, one clip)
//   then       k_opt_commit
// All of it behind the permutations is one captured graph, replayed per update; no host wait inside.
static int cnn_gru_ppo_update(sg_ppo* a, sg_rollout* r, const int64_t* perms, int64_t n_perms, uint64_t seed, float out3[3]) {
    sg_ctx* ctx = a->ctx;
    sg_policy* pol = a->policy;
    const SgPolicyDesc& d = pol->desc;
    const SgCnnDesc& c = pol->cnnd;
    const SgGruDesc& g = pol->gru;
    SG_REQUIRE(r->O == d.O && r->A == d.A, "sg_ppo_update: rollout dims (obs %d, act %d) do not match the policy (%d, %d)", r->O, r->A,
               d.O, d.A);
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_ppo_update: PPO on the recurrent CNN base runs on one rank (world %d)", ctx->world);
    const int T = r->T, N = r->N, M = a->cfg.num_mini_batch, E = a->cfg.ppo_epoch;
    // a2c/storage.py:196-199
    SG_REQUIRE(N >= M, "PPO requires the number of processes (%d) to be greater than or equal to the number of PPO mini batches (%d).", N, M);
    const int per = N / M;
    SG_REQUIRE(N % per == 0, "sg_ppo_update: %d processes do not split into minibatches of %d = %d // %d environments (the reference "
               "indexes past its permutation here)", N, per, N, M);
    const int S = N / per;
    const int64_t TN = (int64_t)T * N;
    SG_REQUIRE(TN < (1ll << 30), "sg_ppo_update: rollout too large");
    const int mb = T * per;
    SG_REQUIRE(mb <= SG_CNN_MAX_MB, "sg_ppo_update: a minibatch of %d rows (%d steps x %d environments) on the recurrent CNN base exceeds "
               "%d (its activation stacks are 158 KB per row): raise num_mini_batch", mb, T, per, SG_CNN_MAX_MB);
    SG_REQUIRE((int64_t)a->h0_count == (int64_t)N * g.H, "sg_ppo_update: a recurrent policy takes the hidden states of rollout slot 0 "
               "from the host: sg_ppo_set_hidden_states must hand over %lld floats before every update (pending: %lld)",
               (long long)N * g.H, (long long)a->h0_count);
    a->h0_count = 0;
    if (perms) {
        SG_REQUIRE(n_perms == (int64_t)E * N, "sg_ppo_update: perms holds %lld indices, %d epochs x %d environments need %lld",
                   (long long)n_perms, E, N, (long long)E * N);
        std::vector<uint8_t> seen((size_t)N);
        for (int e = 0; e < E; ++e) {
            std::fill(seen.begin(), seen.end(), (uint8_t)0);
            for (int i = 0; i < N; ++i) {
                const int64_t v = perms[(size_t)e * N + i];
                SG_REQUIRE(v >= 0 && v < N && !seen[(size_t)v], "sg_ppo_update: perms of epoch %d are not a permutation of the %d environments", e, N);
                seen[(size_t)v] = 1;
            }
        }
    }
    SG_CHECK(hipSetDevice(ctx->device));
    SG_TRY(enqueue_adv_stats(ctx, r, a, false));
    SG_TRY(ensure_cap(ctx->stream, &a->d_perms, &a->perms_cap, (int64_t)E * N));
    a->last_perm_count = (int64_t)E * N;
    if (perms) {
        SG_CHECK(hipMemcpyAsync(a->d_perms, perms, sizeof(int64_t) * (size_t)E * N, hipMemcpyHostToDevice, ctx->stream));
        if (!out3) SG_CHECK(hipStreamSynchronize(ctx->stream));
    } else {
        for (int e = 0; e < E; ++e) SG_TRY(sg_fill_perm(ctx, a->d_perms + (size_t)e * N, N, seed, (uint64_t)e * 2654435761ull));
    }

    // scratch.  d_stacks: head stacks | activation stacks | gradient stacks and slabs, as the feed-forward CNN step.  d_gru: the
    // step's index vector, masks and h0, F as padded rows, GI, h_t, the scan's saves, the gate gradients, the two d loss / d h_t
    // tiles and the weight-gradient partials; rows mb .. rows_p-1 of every [rows_p] block are never written and stay zero.
    const int hld = d.trunk[0].Pp > 16 ? d.trunk[0].Pp : 16;
    const size_t heads_f = 2 * (size_t)mb * hld, fwd_f = sg_cnn_fwd_floats(c, mb), bwd_f = sg_cnn_bwd_floats(c, mb);
    const int rows_p = (mb + 15) & ~15;
    const int Hp = g.Hp, G3 = 3 * Hp;
    const int chunks = rows_p / 16;
    const int KS = std::max(1, std::min(16, chunks / 8));
    auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t o_idx = 0, o_mk = o_idx + r4(2 * (size_t)rows_p), o_h0 = o_mk + r4((size_t)rows_p), o_fp = o_h0 + r4((size_t)per * g.H);
    const size_t o_gi = o_fp + (size_t)rows_p * g.ldO, o_h = o_gi + (size_t)rows_p * G3, o_sr = o_h + r4((size_t)rows_p * g.H);
    const size_t o_sz = o_sr + (size_t)rows_p * Hp, o_sn = o_sz + (size_t)rows_p * Hp, o_shn = o_sn + (size_t)rows_p * Hp;
    const size_t o_hm = o_shn + (size_t)rows_p * Hp, o_dgi = o_hm + (size_t)rows_p * g.ldH, o_dgh = o_dgi + (size_t)rows_p * G3;
    const size_t o_dxa = o_dgh + (size_t)rows_p * G3, o_dxc = o_dxa + (size_t)rows_p * g.ldH, o_part = o_dxc + (size_t)rows_p * g.ldH;
    const size_t gru_f = o_part + (size_t)KS * g.total;
    bool grew = false;
    SG_TRY(ensure_cap(ctx->stream, &a->d_stacks, &a->stacks_cap, heads_f + fwd_f + bwd_f, &grew));
    SG_TRY(ensure_cap(ctx->stream, &a->d_gru, &a->gru_cap, gru_f, &grew));
    if (grew) a->cleared.mode = SG_LAYOUT_INVALID;
    {
        const SgScratchLayout layout = {SG_LAYOUT_CNN_GRU, {T, per, rows_p, KS, g.total, c.total, hld, N}};
        if (memcmp(&a->cleared, &layout, sizeof layout) != 0) {
            SG_CHECK(hipMemsetAsync(a->d_gru, 0, sizeof(float) * gru_f, ctx->stream));
            a->cleared = layout;
        }
    }
    float* heads = a->d_stacks;
    float* act = heads + heads_f;
    float* bwd = act + fwd_f;
    float* F = act + (size_t)mb * (sg_cnn_fwd_floats(c, 1) - c.Hs);                       // [mb][Hs] in the activation stacks
    float* dZf = bwd + (size_t)mb * (sg_cnn_fwd_floats(c, 1) - c.Hs);                     // [mb][Hs] in the gradient stacks
    float* gb = a->d_gru;
    int64_t* idx = reinterpret_cast<int64_t*>(gb + o_idx);
    hipLaunchKernelGGL(k_zero_f64, dim3(1), dim3(64), 0, ctx->stream, a->d_loss_acc, 4);
    const float inv_B = 1.0f / (float)mb;
    const float* obs = r->d_field[SG_F_OBS];
    SgOptState* st = reinterpret_cast<SgOptState*>(a->d_state);

    CnnGruIndexArgs ia;
    ia.masks = r->d_field[SG_F_MASKS]; ia.h0 = a->d_h0; ia.T = T; ia.N = N; ia.per = per; ia.H = g.H;
    ia.idx = idx; ia.MK = gb + o_mk; ia.H0 = gb + o_h0;
    GruScanArgs tr;
    tr.sr = gb + o_sr; tr.sz = gb + o_sz; tr.sn = gb + o_sn; tr.shn = gb + o_shn; tr.hm = gb + o_hm;
    GruBwdArgs ba;
    ba.g = g; ba.W = pol->d_params + g.off; ba.dxa = gb + o_dxa; ba.dxc = gb + o_dxc; ba.dx_ld = g.ldH;
    ba.sr = tr.sr; ba.sz = tr.sz; ba.sn = tr.sn; ba.shn = tr.shn; ba.hm = tr.hm; ba.masks = gb + o_mk; ba.T = T; ba.n = per;
    ba.dgi = gb + o_dgi; ba.dgh = gb + o_dgh;
    GruWgradArgs wa;
    wa.g = g; wa.dgi = ba.dgi; wa.dgh = ba.dgh; wa.x = gb + o_fp; wa.hm = tr.hm; wa.rows_p = rows_p; wa.KS = KS; wa.partial = gb + o_part;
    const bool gw_scan = sg_gru_force_gw() || sg_gru_scan_lds(g, false) > (size_t)ctx->lds_bytes - 1024 ||
                         sg_gru_bwd_lds(g, false) > (size_t)ctx->lds_bytes - 1024;
    const bool gw_dx = sg_gru_force_gw() || sg_gru_dx_lds(g, false) > (size_t)ctx->lds_bytes - 1024;
    GruDxArgs xa;
    xa.g = g; xa.W = pol->d_params + g.off; xa.dgi = ba.dgi; xa.f = F; xa.f_ld = c.Hs; xa.rows = mb; xa.dzf = dZf; xa.dz_ld = c.Hs;
    xa.wbuf_floats = gw_dx ? 0 : 3 * Hp * g.ldO;
    // LDS-weight instance: persistent, a workgroup stages its W_ih image once and walks at least four 16-row tiles where the step
    // has that many.  Global-weight instance: nothing is staged (W_ih comes through L2 for every tile whoever computes it), so one
    // tile per workgroup -- measured at Hs = 512, 256 rows: 490 us against 1,069 us with four tiles per workgroup.
    // The order of every output's sum is its tile's own, whatever the grid is.
    const int dx_grid = gw_dx ? std::min(chunks, ctx->num_cu) : std::min((chunks + 3) / 4, ctx->num_cu);
    const int n_tiles = (G3 / 16) * (g.Op / 16 + Hp / 16) + 2 * (G3 / 16);
    const int gblocks = (g.total + 255) / 256;
    const int nb_flat = (g.off + 255) / 256;
    const int tot_all = g.off + g.total;
    const int nblk = (tot_all + 8 + 255) / 256;

    auto enqueue_steps = [&]() -> int {
        hipLaunchKernelGGL(k_opt_prepare_first, dim3(1), dim3(1), 0, ctx->stream, st);
        for (int e = 0; e < E; ++e)
            for (int k = 0; k < S; ++k) {
                ia.perm = a->d_perms + (size_t)e * N + (size_t)k * per;
                hipLaunchKernelGGL(k_cnn_gru_index<0>, dim3((unsigned)((mb + 255) / 256)), dim3(256), 0, ctx->stream, ia);
                SG_TRY(sg_cnn_trunk_forward_launch(ctx, pol, obs, idx, mb, act, nullptr));
                hipLaunchKernelGGL(k_gru_pad_rows<0>, dim3((unsigned)(((int64_t)mb * g.ldO + 255) / 256)), dim3(256), 0, ctx->stream, F, mb,
                                   c.Hs, gb + o_fp, g.ldO);
                SG_TRY(sg_gru_forward_launch(ctx, g, pol->d_params + g.off, gb + o_fp, g.ldO, gb + o_h0, gb + o_mk, T, per, gb + o_gi,
                                             gb + o_h, g.H, nullptr, &tr));
                SG_TRY(sg_cnn_gru_heads_launch(ctx, pol, r, idx, mb, gb + o_h, heads, hld, bwd, a->d_grad, gb + o_dxa, gb + o_dxc, g.ldH,
                                               inv_B, a->cfg.clip_param, a->cfg.value_loss_coef, a->cfg.entropy_coef,
                                               a->cfg.use_clipped_value_loss, 0, 0));
                if (gw_scan) hipLaunchKernelGGL(k_gru_scan_bwd<true>, dim3((per + 15) / 16), dim3(256), sg_gru_bwd_lds(g, true), ctx->stream, ba);
                else hipLaunchKernelGGL(k_gru_scan_bwd<false>, dim3((per + 15) / 16), dim3(256), sg_gru_bwd_lds(g, false), ctx->stream, ba);
                hipLaunchKernelGGL(k_gru_wgrad<0>, dim3(n_tiles, KS), dim3(64), 0, ctx->stream, wa);
                if (gw_dx) hipLaunchKernelGGL(k_gru_dx<true>, dim3(dx_grid), dim3(256), sg_gru_dx_lds(g, true), ctx->stream, xa);
                else hipLaunchKernelGGL(k_gru_dx<false>, dim3(dx_grid), dim3(256), sg_gru_dx_lds(g, false), ctx->stream, xa);
                SG_TRY(sg_cnn_trunk_backward_launch(ctx, pol, obs, idx, mb, act, bwd, a->d_grad, 0));
                hipLaunchKernelGGL(k_sumsq, dim3(nb_flat), dim3(256), 0, ctx->stream, a->d_grad, g.off, a->d_part);
                hipLaunchKernelGGL(k_gru_reduce<0>, dim3(gblocks), dim3(256), 0, ctx->stream, wa.partial, KS, g.total, a->d_grad, g.off,
                                   a->d_part, nb_flat);
                SG_LAUNCH(ctx, SG_PROF_PPO_ADAM, k_ppo_adam, dim3(nblk), dim3(256), 0, pol->d_params, a->d_m, a->d_v, a->d_grad, a->d_part,
                          nb_flat + gblocks, tot_all, st, e * S + k + 1, a->cfg.eps, a->cfg.max_grad_norm, inv_B, a->d_loss_acc);
            }
        hipLaunchKernelGGL(k_opt_commit, dim3(1), dim3(1), 0, ctx->stream, st, E * S);
        SG_CHECK(hipGetLastError());
        return 0;
    };
    const bool use_graph = !ctx->profile && !sg_env_is_off("SG_PPO_GRAPH");
    uint32_t fbits[6];
    const float fv[6] = {a->cfg.clip_param, a->cfg.value_loss_coef, a->cfg.entropy_coef, a->cfg.eps, a->cfg.max_grad_norm, inv_B};
    memcpy(fbits, fv, sizeof fbits);
    const uint64_t key[SG_GRAPH_KEY_WORDS] = {
            (uint64_t)(uintptr_t)a->d_stacks, (uint64_t)(uintptr_t)a->d_grad, (uint64_t)(uintptr_t)a->d_perms,
            (uint64_t)(uintptr_t)r->d_field[SG_F_OBS], (uint64_t)(uintptr_t)r->d_field[SG_F_ACTIONS],
            (uint64_t)(uintptr_t)r->d_field[SG_F_RETURNS], (uint64_t)(uintptr_t)pol->d_params,
            (uint64_t)TN, ((uint64_t)E << 32) | (uint64_t)M, (uint64_t)mb,
            ((uint64_t)fbits[0] << 32) | fbits[1], ((uint64_t)fbits[2] << 32) | fbits[3],
            ((uint64_t)fbits[4] << 32) | fbits[5], (uint64_t)a->cfg.use_clipped_value_loss,
            (uint64_t)(uintptr_t)r->d_field[SG_F_LOGP] ^ ((uint64_t)(uintptr_t)r->d_field[SG_F_VALUE_PREDS] << 1) ^
                    ((uint64_t)(uintptr_t)r->d_field[SG_F_ADVANTAGES] << 2),
            // 'CNG': the recurrent CNN step sequence
            0x434E47ull + (gw_scan ? 16 : 0) + (gw_dx ? 8 : 0) + ((uint64_t)N << 32),
            (uint64_t)(uintptr_t)a->d_gru, (uint64_t)(uintptr_t)a->d_h0 ^ ((uint64_t)(uintptr_t)r->d_field[SG_F_MASKS] << 1)};
    SG_TRY(sg_graph_run(ctx, &a->steps_graph, use_graph, key, enqueue_steps));
    SG_CHECK(hipGetLastError());
    a->opt_t += (int64_t)E * S;
    if (!out3) return 0;
    double acc[3];
    SG_TRY(sg_ctx_fetch_f64(ctx, a->d_loss_acc, acc, 3));
    const double nu = (double)E * M;   // a2c/algo/ppo.py:151-155 divides by ppo_epoch * num_mini_batch whatever N // per is
    for (int i = 0; i < 3; ++i) out3[i] = (float)(acc[i] / nu);
    return 0;
}

// ------------------------------------------------------------------- A2C on the CNN base
// Rows of one chunk: its activation and gradient stacks are 167 KB per row, 684 MB at 4096 -- the fastest of 256 ... 4096 measured
// at 8192 rows (66.6, 58.7, 58.2, 56.3, 56.0 ms) that stays under 1 GB, and PPO's minibatch cap.  A rollout of
// fewer rows is one chunk of its own size.  SG_A2C_CNN_CHUNK_ROWS (any n >= 1: test and tuning knob, after SG_A2C_GROUP_ENVS)
// forces a smaller chunk.
#define SG_A2C_CNN_CHUNK_ROWS 4096
static int a2c_cnn_chunk_rows(int64_t TN) {
    int chunk = SG_A2C_CNN_CHUNK_ROWS;
    if (const char* e = getenv("SG_A2C_CNN_CHUNK_ROWS")) {
        const long v = atol(e);
        if (v >= 1) chunk = (int)std::min<long>(v, SG_CNN_MAX_MB);
    }
    return (int)std::min<int64_t>(chunk, TN);
}

// A2C_ACKTR.update(rollouts), acktr=False, on the CNN base (a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:204-230): ONE loss
// over all T*N rows, one clip, one RMSprop step.  The rows go through the network in chunks, in rollout order:
//   per chunk:  the forward of sg_cnn.hip on the chunk's frames (read in place from the rollout: no epoch copy)
//               -> k_cnn_head_loss_a2c (inv_B = 1 / (T N) whatever the chunk) -> head, FC, conv3, conv2, conv1 gradients, each
//               weight gradient as slabs + k_cnn_reduce; from the second chunk on every reduce ADDS to the flat gradient
//               (acc = 1: the running value starts from what the gradient holds), so nothing is cleared and the summation
//               order of every element is fixed by T*N and the chunk size
//   then        k_sumsq -> k_a2c_rmsprop (the learning rate from the device scalars: sg_ppo_set_lr)
// One captured graph, replayed per update; no host wait inside.  The scratch is sized by the chunk, not by T*N.
static int a2c_cnn_update(sg_ppo* a, sg_rollout* r, float out3[3]) {
    sg_ctx* ctx = a->ctx;
    sg_policy* pol = a->policy;
    const SgPolicyDesc& d = pol->desc;
    const SgCnnDesc& c = pol->cnnd;
    SG_REQUIRE(r->O == d.O && r->A == d.A, "sg_ppo_update: rollout dims (obs %d, act %d) do not match the policy (%d, %d)", r->O, r->A,
               d.O, d.A);
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_ppo_update: A2C on the CNN base runs on one rank (world %d)", ctx->world);
    const int64_t TN = (int64_t)r->T * r->N;
    SG_REQUIRE(TN > 0 && TN < (1ll << 30), "sg_ppo_update: %lld rollout rows", (long long)TN);
    SG_CHECK(hipSetDevice(ctx->device));
    const int chunk = a2c_cnn_chunk_rows(TN);
    const int n_chunks = (int)((TN + chunk - 1) / chunk);
    // scratch of one full chunk: head stacks | activation stacks | gradient stacks and slabs
    const int hld = d.trunk[0].Pp > 16 ? d.trunk[0].Pp : 16;
    const size_t heads_f = 2 * (size_t)chunk * hld, fwd_f = sg_cnn_fwd_floats(c, chunk), bwd_f = sg_cnn_bwd_floats(c, chunk);
    bool grew = false;
    SG_TRY(ensure_cap(ctx->stream, &a->d_stacks, &a->stacks_cap, heads_f + fwd_f + bwd_f, &grew));
    if (grew) a->cleared.mode = SG_LAYOUT_INVALID;
    float* heads = a->d_stacks;
    float* act = heads + heads_f;
    float* bwd = act + fwd_f;
    hipLaunchKernelGGL(k_zero_f64, dim3(1), dim3(64), 0, ctx->stream, a->d_loss_acc, 4);
    const float inv_B = 1.0f / (float)TN;
    const int nblk = (c.total + 255) / 256;
    const double oma = 1.0 - (double)a->alpha;   // torch: value = 1 - alpha in Python doubles
    SgOptState* st = reinterpret_cast<SgOptState*>(a->d_state);
    const float* obs = r->d_field[SG_F_OBS];

    auto enqueue_step = [&]() -> int {
        for (int k = 0; k < n_chunks; ++k) {
            const int64_t rb = (int64_t)k * chunk;
            const int cnt = (int)std::min<int64_t>(chunk, TN - rb);
            const float* frames = obs + (size_t)rb * d.O;
            SG_TRY(sg_cnn_forward_launch(ctx, pol, frames, nullptr, cnt, act, heads, hld, 0, cnt));
            SG_TRY(sg_cnn_backward_launch(ctx, pol, r, frames, nullptr, cnt, act, heads, hld, bwd, a->d_grad, inv_B, 0.f,
                                          a->cfg.value_loss_coef, a->cfg.entropy_coef, 0, 1, k > 0 ? 1 : 0, rb));
        }
        hipLaunchKernelGGL(k_sumsq, dim3(nblk), dim3(256), 0, ctx->stream, a->d_grad, c.total, a->d_part);
        SG_LAUNCH(ctx, SG_PROF_PPO_ADAM, k_a2c_rmsprop, dim3(nblk), dim3(256), 0, pol->d_params, a->d_v, a->d_grad, a->d_part, nblk,
                  c.total, st, a->alpha, (float)oma, a->cfg.eps, a->cfg.max_grad_norm, inv_B, a->d_loss_acc);
        SG_CHECK(hipGetLastError());
        return 0;
    };
    const bool use_graph = !ctx->profile && !sg_env_is_off("SG_PPO_GRAPH");
    uint32_t fbits[6];
    const float fv[6] = {a->alpha, a->cfg.value_loss_coef, a->cfg.entropy_coef, a->cfg.eps, a->cfg.max_grad_norm, inv_B};
    memcpy(fbits, fv, sizeof fbits);
    const uint64_t key[SG_GRAPH_KEY_WORDS] = {
            (uint64_t)(uintptr_t)a->d_stacks, (uint64_t)(uintptr_t)a->d_grad, 0,
            (uint64_t)(uintptr_t)r->d_field[SG_F_OBS], (uint64_t)(uintptr_t)r->d_field[SG_F_ACTIONS],
            (uint64_t)(uintptr_t)r->d_field[SG_F_RETURNS], (uint64_t)(uintptr_t)pol->d_params,
            (uint64_t)TN, ((uint64_t)n_chunks << 32) | (uint64_t)chunk, 0,
            ((uint64_t)fbits[0] << 32) | fbits[1], ((uint64_t)fbits[2] << 32) | fbits[3],
            ((uint64_t)fbits[4] << 32) | fbits[5], 0, 0,
            0x413243434Eull,   // 'A2CCN': A2C on the CNN base, the chunked step sequence
            0, 0};
    SG_TRY(sg_graph_run(ctx, &a->steps_graph, use_graph, key, enqueue_step));
    SG_CHECK(hipGetLastError());
    a->opt_t += 1;
    if (!out3) return 0;   // queued: the losses come through the results ring (step count 1)
    double acc[3];
    SG_TRY(sg_ctx_fetch_f64(ctx, a->d_loss_acc, acc, 3));
    for (int i = 0; i < 3; ++i) out3[i] = (float)acc[i];
    return 0;
}

// ------------------------------------------------------------------- A2C through time on the recurrent CNN base
// Rows of one environment group: the trunk's activation and gradient stacks are 167 KB per row, so a group holds the most whole
// environments (all T steps each) that stay within a2c_cnn_update's chunk and PPO's minibatch cap.  SG_A2C_CNN_GRU_GROUP_ENVS (any
// n >= 1: test and tuning knob, after SG_A2C_GROUP_ENVS and SG_A2C_CNN_CHUNK_ROWS) forces a smaller group.
#define SG_A2C_CNN_GRU_GROUP_ROWS 4096
static int a2c_cnn_gru_group_envs(int T, int N) {
    int ne = std::max(1, std::min(N, SG_A2C_CNN_GRU_GROUP_ROWS / T));
    if (const char* e = getenv("SG_A2C_CNN_GRU_GROUP_ENVS")) {
        const long v = atol(e);
        if (v >= 1) ne = (int)std::min<long>(v, ne);
    }
    return ne;
}

// A2C_ACKTR.update(rollouts), acktr=False, on CNNBase(recurrent=True) (a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:117-230):
// evaluate_actions runs the trunk on all T*N frames and steps the GRU through the T steps of the N environments from the state of
// slot 0; ONE loss over the T*N rows (inv_B = 1 / (T N) in every group), one clip over the CNN and GRU parameters together, one
// RMSprop step.  Per group k of n <= ne whole environments [e0, e0 + n), time-major (the last group may be smaller):
//   k_cnn_gru_index_group     group row t * n + j -> rollout row t * N + e0 + j; masks and h0 rows e0 .. gathered.  Frames, actions
//                             and returns are read in place through the index: no copy of observations
//   the CNN trunk's forward -> k_gru_pad_rows -> k_gru_inproj -> k_gru_scan_fwd<TRAIN> -> k_cnn_head_fwd on h_t
//   -> k_cnn_head_loss_a2c_idx -> k_cnn_head_dh -> k_cnn_head_wgrad (acc = k > 0: head gradients and the three loss sums add up)
//   -> k_gru_scan_bwd -> k_gru_wgrad -> k_gru_reduce_acc (adds to the GRU's gradient; the last group finishes it) -> k_gru_dx
//   -> the trunk's backward from dZf (acc = k > 0: every k_cnn_reduce adds to the flat gradient)
// then k_sumsq over the flat block (the GRU block's sums are k_gru_reduce_acc's) -> k_a2c_rmsprop over both blocks.
// Every sum has one order, fixed by T, N and the group size.  One captured graph, replayed per update; no host wait inside.  The
// scratch is sized by the group, not by T*N.
static int a2c_cnn_gru_update(sg_ppo* a, sg_rollout* r, float out3[3]) {
    sg_ctx* ctx = a->ctx;
    sg_policy* pol = a->policy;
    const SgPolicyDesc& d = pol->desc;
    const SgCnnDesc& c = pol->cnnd;
    const SgGruDesc& g = pol->gru;
    SG_REQUIRE(r->O == d.O && r->A == d.A, "sg_ppo_update: rollout dims (obs %d, act %d) do not match the policy (%d, %d)", r->O, r->A,
               d.O, d.A);
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_ppo_update: A2C on the recurrent CNN base runs on one rank (world %d)", ctx->world);
    const int T = r->T, N = r->N;
    SG_REQUIRE(T <= SG_A2C_CNN_GRU_GROUP_ROWS, "sg_ppo_update: A2C on the recurrent CNN base takes whole environments per group: the %d "
               "steps of one exceed the %d rows a group may hold (its activation stacks are 167 KB per row)", T, SG_A2C_CNN_GRU_GROUP_ROWS);
    SG_REQUIRE((int64_t)a->h0_count == (int64_t)N * g.H, "sg_ppo_update: a recurrent policy takes the hidden states of rollout slot 0 "
               "from the host: sg_ppo_set_hidden_states must hand over %lld floats before every update (pending: %lld)",
               (long long)N * g.H, (long long)a->h0_count);
    a->h0_count = 0;
    const int64_t TN = (int64_t)T * N;
    SG_REQUIRE(TN > 0 && TN < (1ll << 30), "sg_ppo_update: %lld rollout rows", (long long)TN);
    SG_CHECK(hipSetDevice(ctx->device));

    // geometry of a full group; a smaller last group uses the head of every block
    const int ne = a2c_cnn_gru_group_envs(T, N);
    const int n_groups = (N + ne - 1) / ne;
    const int mb = T * ne;
    const int hld = d.trunk[0].Pp > 16 ? d.trunk[0].Pp : 16;
    const size_t heads_f = 2 * (size_t)mb * hld, fwd_f = sg_cnn_fwd_floats(c, mb), bwd_f = sg_cnn_bwd_floats(c, mb);
    const int rows_p = (mb + 15) & ~15;
    const int Hp = g.Hp, G3 = 3 * Hp;
    auto ks_of = [](int rp) { return std::max(1, std::min(16, (rp / 16) / 8)); };   // row ranges of k_gru_wgrad, as in the PPO step
    const int KS = ks_of(rows_p);
    // scratch.  d_stacks: head stacks | activation stacks | gradient stacks and slabs, as the feed-forward CNN step.  d_gru: the
    // group's index vector, masks and h0, F as padded rows, GI, h_t, the scan's saves, the gate gradients, the two d loss / d h_t
    // tiles, the weight-gradient partials and the running GRU gradient; rows mb .. rows_p-1 of every [rows_p] block are never
    // written and stay zero.
    auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t o_idx = 0, o_mk = o_idx + r4(2 * (size_t)rows_p), o_h0 = o_mk + r4((size_t)rows_p), o_fp = o_h0 + r4((size_t)ne * g.H);
    const size_t o_gi = o_fp + (size_t)rows_p * g.ldO, o_h = o_gi + (size_t)rows_p * G3, o_sr = o_h + r4((size_t)rows_p * g.H);
    const size_t o_sz = o_sr + (size_t)rows_p * Hp, o_sn = o_sz + (size_t)rows_p * Hp, o_shn = o_sn + (size_t)rows_p * Hp;
    const size_t o_hm = o_shn + (size_t)rows_p * Hp, o_dgi = o_hm + (size_t)rows_p * g.ldH, o_dgh = o_dgi + (size_t)rows_p * G3;
    const size_t o_dxa = o_dgh + (size_t)rows_p * G3, o_dxc = o_dxa + (size_t)rows_p * g.ldH, o_part = o_dxc + (size_t)rows_p * g.ldH;
    const size_t o_acc = o_part + (size_t)KS * g.total, gru_f = o_acc + r4((size_t)g.total);
    bool grew = false;
    SG_TRY(ensure_cap(ctx->stream, &a->d_stacks, &a->stacks_cap, heads_f + fwd_f + bwd_f, &grew));
    SG_TRY(ensure_cap(ctx->stream, &a->d_gru, &a->gru_cap, gru_f, &grew));
    if (grew) a->cleared.mode = SG_LAYOUT_INVALID;
    {
        const SgScratchLayout layout = {SG_LAYOUT_A2C_CNN_GRU, {T, ne, rows_p, KS, g.total, c.total, hld, N}};
        if (memcmp(&a->cleared, &layout, sizeof layout) != 0) {
            SG_CHECK(hipMemsetAsync(a->d_gru, 0, sizeof(float) * gru_f, ctx->stream));
            a->cleared = layout;
        }
    }
    float* heads = a->d_stacks;
    float* act = heads + heads_f;
    float* bwd = act + fwd_f;
    float* gb = a->d_gru;
    int64_t* idx = reinterpret_cast<int64_t*>(gb + o_idx);
    hipLaunchKernelGGL(k_zero_f64, dim3(1), dim3(64), 0, ctx->stream, a->d_loss_acc, 4);
    const float inv_B = 1.0f / (float)TN;   // 1 / (T N) of the whole rollout, whatever the group
    const float* obs = r->d_field[SG_F_OBS];
    SgOptState* st = reinterpret_cast<SgOptState*>(a->d_state);
    const double oma = 1.0 - (double)a->alpha;   // torch: value = 1 - alpha in Python doubles

    CnnGruGroupIndexArgs ia;
    ia.masks = r->d_field[SG_F_MASKS]; ia.h0 = a->d_h0; ia.T = T; ia.N = N; ia.e0 = 0; ia.n = ne; ia.H = g.H;
    ia.idx = idx; ia.MK = gb + o_mk; ia.H0 = gb + o_h0;
    GruScanArgs tr;
    tr.sr = gb + o_sr; tr.sz = gb + o_sz; tr.sn = gb + o_sn; tr.shn = gb + o_shn; tr.hm = gb + o_hm;
    GruBwdArgs ba;
    ba.g = g; ba.W = pol->d_params + g.off; ba.dxa = gb + o_dxa; ba.dxc = gb + o_dxc; ba.dx_ld = g.ldH;
    ba.sr = tr.sr; ba.sz = tr.sz; ba.sn = tr.sn; ba.shn = tr.shn; ba.hm = tr.hm; ba.masks = gb + o_mk; ba.T = T; ba.n = ne;
    ba.dgi = gb + o_dgi; ba.dgh = gb + o_dgh;
    GruWgradArgs wa;
    wa.g = g; wa.dgi = ba.dgi; wa.dgh = ba.dgh; wa.x = gb + o_fp; wa.hm = tr.hm; wa.rows_p = rows_p; wa.KS = KS; wa.partial = gb + o_part;
    const bool gw_scan = sg_gru_force_gw() || sg_gru_scan_lds(g, false) > (size_t)ctx->lds_bytes - 1024 ||
                         sg_gru_bwd_lds(g, false) > (size_t)ctx->lds_bytes - 1024;
    const bool gw_dx = sg_gru_force_gw() || sg_gru_dx_lds(g, false) > (size_t)ctx->lds_bytes - 1024;
    GruDxArgs xa;
    xa.g = g; xa.W = pol->d_params + g.off; xa.dgi = ba.dgi; xa.f_ld = c.Hs; xa.dz_ld = c.Hs;
    xa.wbuf_floats = gw_dx ? 0 : 3 * Hp * g.ldO;
    const int n_tiles = (G3 / 16) * (g.Op / 16 + Hp / 16) + 2 * (G3 / 16);
    const int gblocks = (g.total + 255) / 256;
    const int nb_flat = (g.off + 255) / 256;
    const int tot_all = g.off + g.total;
    const int nblk = (tot_all + 8 + 255) / 256;
    const size_t trunk_row_f = sg_cnn_fwd_floats(c, 1) - c.Hs;   // A1 | A2 | A3 of one row: F and dZf lie behind the group's

    auto enqueue_step = [&]() -> int {
        for (int k = 0; k < n_groups; ++k) {
            const int e0 = k * ne, n = std::min(ne, N - e0), rows = T * n, rows_pk = (rows + 15) & ~15, chunks = rows_pk / 16;
            const int acc = k > 0 ? 1 : 0;
            float* F = act + (size_t)rows * trunk_row_f;      // [rows][Hs] in the activation stacks
            float* dZf = bwd + (size_t)rows * trunk_row_f;    // [rows][Hs] in the gradient stacks
            ia.e0 = e0; ia.n = n;
            hipLaunchKernelGGL(k_cnn_gru_index_group<0>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, ia);
            SG_TRY(sg_cnn_trunk_forward_launch(ctx, pol, obs, idx, rows, act, nullptr));
            hipLaunchKernelGGL(k_gru_pad_rows<0>, dim3((unsigned)(((int64_t)rows * g.ldO + 255) / 256)), dim3(256), 0, ctx->stream, F, rows,
                               c.Hs, gb + o_fp, g.ldO);
            SG_TRY(sg_gru_forward_launch(ctx, g, pol->d_params + g.off, gb + o_fp, g.ldO, gb + o_h0, gb + o_mk, T, n, gb + o_gi, gb + o_h,
                                         g.H, nullptr, &tr));
            SG_TRY(sg_cnn_gru_heads_launch(ctx, pol, r, idx, rows, gb + o_h, heads, hld, bwd, a->d_grad, gb + o_dxa, gb + o_dxc, g.ldH,
                                           inv_B, 0.f, a->cfg.value_loss_coef, a->cfg.entropy_coef, 0, 1, acc));
            if (rows_pk > rows && n < ne) {   // a smaller last group: its padding rows hold a full group's gate gradients
                SG_CHECK(hipMemsetAsync(gb + o_dgi + (size_t)rows * G3, 0, sizeof(float) * (size_t)(rows_pk - rows) * G3, ctx->stream));
                SG_CHECK(hipMemsetAsync(gb + o_dgh + (size_t)rows * G3, 0, sizeof(float) * (size_t)(rows_pk - rows) * G3, ctx->stream));
            }
            ba.n = n;
            if (gw_scan) hipLaunchKernelGGL(k_gru_scan_bwd<true>, dim3((n + 15) / 16), dim3(256), sg_gru_bwd_lds(g, true), ctx->stream, ba);
            else hipLaunchKernelGGL(k_gru_scan_bwd<false>, dim3((n + 15) / 16), dim3(256), sg_gru_bwd_lds(g, false), ctx->stream, ba);
            wa.rows_p = rows_pk; wa.KS = ks_of(rows_pk);
            hipLaunchKernelGGL(k_gru_wgrad<0>, dim3(n_tiles, wa.KS), dim3(64), 0, ctx->stream, wa);
            hipLaunchKernelGGL(k_gru_reduce_acc<0>, dim3(gblocks), dim3(256), 0, ctx->stream, wa.partial, wa.KS, g.total, gb + o_acc, acc,
                               k + 1 == n_groups ? 1 : 0, a->d_grad, g.off, a->d_part, nb_flat);
            xa.f = F; xa.rows = rows; xa.dzf = dZf;
            // grid: as cnn_gru_ppo_update (LDS-weight instance: at least four 16-row tiles per workgroup; global-weight: one)
            const int dx_grid = gw_dx ? std::min(chunks, ctx->num_cu) : std::min((chunks + 3) / 4, ctx->num_cu);
            if (gw_dx) hipLaunchKernelGGL(k_gru_dx<true>, dim3(dx_grid), dim3(256), sg_gru_dx_lds(g, true), ctx->stream, xa);
            else hipLaunchKernelGGL(k_gru_dx<false>, dim3(dx_grid), dim3(256), sg_gru_dx_lds(g, false), ctx->stream, xa);
            SG_TRY(sg_cnn_trunk_backward_launch(ctx, pol, obs, idx, rows, act, bwd, a->d_grad, acc));
        }
        hipLaunchKernelGGL(k_sumsq, dim3(nb_flat), dim3(256), 0, ctx->stream, a->d_grad, g.off, a->d_part);
        SG_LAUNCH(ctx, SG_PROF_PPO_ADAM, k_a2c_rmsprop, dim3(nblk), dim3(256), 0, pol->d_params, a->d_v, a->d_grad, a->d_part,
                  nb_flat + gblocks, tot_all, st, a->alpha, (float)oma, a->cfg.eps, a->cfg.max_grad_norm, inv_B, a->d_loss_acc);
        SG_CHECK(hipGetLastError());
        return 0;
    };
    const bool use_graph = !ctx->profile && !sg_env_is_off("SG_PPO_GRAPH");
    uint32_t fbits[6];
    const float fv[6] = {a->alpha, a->cfg.value_loss_coef, a->cfg.entropy_coef, a->cfg.eps, a->cfg.max_grad_norm, inv_B};
    memcpy(fbits, fv, sizeof fbits);
    const uint64_t key[SG_GRAPH_KEY_WORDS] = {
            (uint64_t)(uintptr_t)a->d_stacks, (uint64_t)(uintptr_t)a->d_grad, (uint64_t)(uintptr_t)a->d_gru,
            (uint64_t)(uintptr_t)r->d_field[SG_F_OBS], (uint64_t)(uintptr_t)r->d_field[SG_F_ACTIONS],
            (uint64_t)(uintptr_t)r->d_field[SG_F_RETURNS], (uint64_t)(uintptr_t)pol->d_params,
            (uint64_t)TN, ((uint64_t)T << 32) | (uint64_t)N, ((uint64_t)n_groups << 32) | (uint64_t)ne,
            ((uint64_t)fbits[0] << 32) | fbits[1], ((uint64_t)fbits[2] << 32) | fbits[3],
            ((uint64_t)fbits[4] << 32) | fbits[5], (uint64_t)(uintptr_t)r->d_field[SG_F_MASKS],
            (uint64_t)(uintptr_t)a->d_h0,
            // 'A2CNG': A2C through time on the recurrent CNN base, the grouped step sequence
            0x4132434E47ull + (gw_scan ? 16 : 0) + (gw_dx ? 8 : 0),
            ((uint64_t)rows_p << 32) | (uint64_t)KS, (uint64_t)(uintptr_t)a->d_part};
    SG_TRY(sg_graph_run(ctx, &a->steps_graph, use_graph, key, enqueue_step));
    SG_CHECK(hipGetLastError());
    a->opt_t += 1;
    if (!out3) return 0;   // queued: the losses come through the results ring (step count 1)
    double acc[3];
    SG_TRY(sg_ctx_fetch_f64(ctx, a->d_loss_acc, acc, 3));
    for (int i = 0; i < 3; ++i) out3[i] = (float)acc[i];
    return 0;
}

// ------------------------------------------------------------------- A2C through time (recurrent policy)
// Rows one environment group may hold: the scan scratch is rows x (13 Hp + 5 ldH + ldO) floats (GI, dGI, dGH: 9 Hp; the saved
// gates: 4 Hp; the masked state, the heads' input and the two d loss / d h: 4 ldH beside ACT and SC; the observation copy: ldO),
// 4.6 KB per row at H = 64, obs 47.  65,536 rows (303 MB there) make the north-star rollout (128 x 512) ONE group: fewer
// environments per scan do not shorten its T-long chain, they only run it again.
#define SG_A2C_RNN_GROUP_ROWS 65536
// environments per group: the most that fit the row cap, in whole scan tiles of 16; SG_A2C_GROUP_ENVS (a multiple of 16: test
// knob) forces a smaller group
static int a2c_gru_group_envs(int T, int N) {
    int ng = std::max(16, (SG_A2C_RNN_GROUP_ROWS / T) & ~15);
    if (const char* e = getenv("SG_A2C_GROUP_ENVS")) {
        const int v = atoi(e);
        if (v >= 16 && v % 16 == 0) ng = v;
    }
    return std::min(ng, N);
}

// A2C_ACKTR.update(rollouts), acktr=False, with actor_critic.is_recurrent (a2c/algo/a2c_acktr.py:52-102 over a2c/model.py:117-201):
// evaluate_actions steps the GRU through all T steps of all N environments from the state of slot 0 (h <- h * masks[t]), the
// heads see the states; one loss over the T*N rows, one clip over ALL parameters, one RMSprop step.  Per environment group:
//   k_a2c_gru_gather -> k_gru_inproj -> k_gru_scan_fwd<TRAIN>
//   per chunk of <= SG_A2C_CHUNK_ROWS rows:  k_ppo_fwd -> k_a2c_bwd_dx (a Categorical / Bernoulli head: k_a2c_bwd_dist_dx)
//                                            -> k_a2c_reduce (adds to the heads' gradient)
//   k_gru_scan_bwd -> k_gru_wgrad -> k_gru_reduce_acc (adds to the GRU's gradient; the last group finishes it)
// then k_a2c_rmsprop over heads + GRU.  One captured graph from the first gather on; no host wait inside.
static int a2c_gru_update(sg_ppo* a, sg_rollout* r, float out3[3]) {
    sg_ctx* ctx = a->ctx;
    sg_policy* pol = a->policy;
    const SgPolicyDesc& d = pol->desc;
    const SgGruDesc& g = pol->gru;
    SG_REQUIRE(r->O == g.O && r->A == d.A, "sg_ppo_update: rollout dims (obs %d, act %d) do not match the policy (%d, %d)", r->O, r->A,
               g.O, d.A);
    SG_REQUIRE(!(ctx->use_comm && ctx->world > 1), "sg_ppo_update: A2C with a recurrent policy runs on one rank (world %d)", ctx->world);
    const int T = r->T, N = r->N;
    SG_REQUIRE((int64_t)a->h0_count == (int64_t)N * g.H, "sg_ppo_update: a recurrent policy takes the hidden states of rollout slot 0 "
               "from the host: sg_ppo_set_hidden_states must hand over %lld floats before every update (pending: %lld)",
               (long long)N * g.H, (long long)a->h0_count);
    a->h0_count = 0;
    const int64_t TN = (int64_t)T * N;
    SG_REQUIRE(TN > 0 && TN < (1ll << 30), "sg_ppo_update: %lld rollout rows", (long long)TN);
    SG_CHECK(hipSetDevice(ctx->device));

    // geometry.  Groups of ng environments (the last one may be smaller); a full group has Bg rows, time-major.  Heads: the
    // two-launch A2C form on chunks of the group's rows.  Scans: one workgroup per 16 environments of the group.
    const int ng = a2c_gru_group_envs(T, N);
    const int n_groups = (N + ng - 1) / ng;
    SG_REQUIRE((int64_t)T * ng < (1ll << 26), "sg_ppo_update: %d steps x %d environments do not fit one scan group", T, ng);
    const int Bg = T * ng;
    const int chunk = std::min(Bg, SG_A2C_CHUNK_ROWS);
    auto bwd_lds = [&](int mt, bool gwv) { return ppo_bwd_tiles_lds(d, mt, gwv ? 0 : max_bwd_floats(d), 2, false); };
    auto fits = [&](int mt, bool gwv) { return ppo_fwd_lds(d, mt, gwv) <= (size_t)ctx->lds_bytes && bwd_lds(mt, gwv) <= (size_t)ctx->lds_bytes; };
    const bool gw = sg_policy_needs_gw(ctx, d) || !fits(1, false);
    SG_REQUIRE(fits(1, gw), "sg_ppo_update: the 16-row tiles of the A2C step do not fit LDS");
    const int MT = ppo_row_tiles(ctx, d, chunk, d.n_trunks, true, 2, 2, [&](int mt) { return fits(mt, gw); });
    const int R = 16 * MT, G = (chunk + R - 1) / R, mbp = G * R;
    const int ldP = stack_ldP(d);
    const int slab_stride = (d.total + 8 + 63) & ~63;
    const int Bgp = Bg + 64;             // slack rows: the last row tile reads (and writes d loss / d h) up to R - 1 rows past the group
    const int rows_p = (Bg + 15) & ~15;
    const int Hp = g.Hp, G3 = 3 * Hp;
    auto ks_of = [](int rp) { return std::max(1, std::min(16, (rp / 16) / 8)); };   // row ranges of k_gru_wgrad, as in the PPO step
    const int KS = ks_of(rows_p);
    const int gblocks = (g.total + 255) / 256;
    const int nblk_r = (d.total + 8 + SG_PPO_REDUCE_PARAMS - 1) / SG_PPO_REDUCE_PARAMS;
    const int tot_all = d.total + g.total;
    const int nblk = (tot_all + 8 + 255) / 256;

    // scratch: slabs; d_stacks = heads' input rows | ACT | SC | the chunk's activation stacks; d_gru = everything of the GRU
    const size_t slab_f = (size_t)G * slab_stride;
    const size_t hx_f = (size_t)Bgp * d.ldO;
    auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t act_f = r4((size_t)Bgp * d.A);   // (the activation stacks behind ACT and SC stay 16-byte aligned)
    const size_t ep_f = hx_f + act_f + 4 * (size_t)Bgp;
    const size_t stack_f = ep_f + (size_t)d.n_trunks * mbp * (2 * (size_t)d.ldH + ldP);
    const size_t o_x = 0, o_mk = o_x + r4((size_t)Bgp * g.ldO), o_h0 = o_mk + r4((size_t)Bgp), o_gi = o_h0 + r4((size_t)ng * g.H);
    const size_t o_sr = o_gi + (size_t)rows_p * G3, o_sz = o_sr + (size_t)rows_p * Hp, o_sn = o_sz + (size_t)rows_p * Hp;
    const size_t o_shn = o_sn + (size_t)rows_p * Hp, o_hm = o_shn + (size_t)rows_p * Hp, o_dgi = o_hm + (size_t)rows_p * g.ldH;
    const size_t o_dgh = o_dgi + (size_t)rows_p * G3, o_dxa = o_dgh + (size_t)rows_p * G3, o_dxc = o_dxa + (size_t)Bgp * d.ldO;
    const size_t o_part = o_dxc + (size_t)Bgp * d.ldO, o_acc = o_part + (size_t)KS * g.total, gru_f = o_acc + r4((size_t)g.total);
    bool grew = false;
    SG_TRY(ensure_cap(ctx->stream, &a->d_slabs, &a->slabs_cap, slab_f, &grew));
    SG_TRY(ensure_cap(ctx->stream, &a->d_stacks, &a->stacks_cap, stack_f, &grew));
    SG_TRY(ensure_cap(ctx->stream, &a->d_gru, &a->gru_cap, gru_f, &grew));
    if (grew) a->cleared.mode = SG_LAYOUT_INVALID;
    SG_TRY(clear_for_layout(a, {SG_LAYOUT_A2C_GRU, {G, slab_stride, mbp, Bgp, MT, KS, ng, ((int64_t)g.total << 32) | (int64_t)rows_p}},
                            slab_f, stack_f, gru_f));
    hipLaunchKernelGGL(k_zero_f64, dim3(1), dim3(64), 0, ctx->stream, a->d_loss_acc, 4);

    float* hX = a->d_stacks;
    float* epACT = hX + hx_f;
    float* epSC = epACT + act_f;
    float* stk = a->d_stacks + ep_f;
    float* gb = a->d_gru;

    A2cGruGatherArgs ga;
    ga.obs = r->d_field[SG_F_OBS]; ga.actions = r->d_field[SG_F_ACTIONS]; ga.ret = r->d_field[SG_F_RETURNS];
    ga.masks = r->d_field[SG_F_MASKS]; ga.h0 = a->d_h0;
    ga.T = T; ga.N = N; ga.e0 = 0; ga.n = ng; ga.O = g.O; ga.ldO = g.ldO; ga.A = d.A; ga.H = g.H; ga.sc_stride = Bgp;
    ga.X = gb + o_x; ga.ACT = epACT; ga.SC = epSC; ga.MK = gb + o_mk; ga.H0 = gb + o_h0;

    PpoArgs pa;
    memset(&pa, 0, sizeof pa);
    pa.d = d; pa.params = pol->d_params;
    pa.sc_stride = Bgp; pa.mbp = mbp; pa.inv_B = 1.0f / (float)TN;   // 1 / (T N) of the whole rollout, whatever the group or chunk
    pa.vcoef = a->cfg.value_loss_coef; pa.ecoef = a->cfg.entropy_coef;
    pa.slabs = a->d_slabs; pa.slab_stride = slab_stride; pa.ldP = ldP;
    pa.st = reinterpret_cast<SgOptState*>(a->d_state); pa.G = G; pa.k1 = 1;
    for (int t = 0; t < d.n_trunks; ++t) {
        pa.H1[t] = stk; stk += (size_t)mbp * d.ldH;
        pa.H2[t] = stk; stk += (size_t)mbp * d.ldH;
        pa.OUT[t] = stk; stk += (size_t)mbp * ldP;
    }
    const int wb_f = gw ? 0 : max_trunk_floats(d), wb_b = gw ? 0 : max_bwd_floats(d);
    const size_t lds_f = ppo_fwd_lds(d, MT, gw), lds_b = bwd_lds(MT, gw);
    const double oma = 1.0 - (double)a->alpha;

    GruScanArgs tr;
    tr.sr = gb + o_sr; tr.sz = gb + o_sz; tr.sn = gb + o_sn; tr.shn = gb + o_shn; tr.hm = gb + o_hm;
    GruBwdArgs ba;
    ba.g = g; ba.W = pol->d_params + g.off; ba.dxa = gb + o_dxa; ba.dxc = gb + o_dxc; ba.dx_ld = d.ldO;
    ba.sr = tr.sr; ba.sz = tr.sz; ba.sn = tr.sn; ba.shn = tr.shn; ba.hm = tr.hm; ba.T = T; ba.n = ng;
    ba.masks = gb + o_mk; ba.dgi = gb + o_dgi; ba.dgh = gb + o_dgh;
    GruWgradArgs wa;
    wa.g = g; wa.dgi = ba.dgi; wa.dgh = ba.dgh; wa.hm = tr.hm; wa.x = gb + o_x; wa.rows_p = rows_p; wa.KS = KS; wa.partial = gb + o_part;
    const bool gw_scan = sg_gru_force_gw() || sg_gru_scan_lds(g, false) > (size_t)ctx->lds_bytes - 1024 ||
                         sg_gru_bwd_lds(g, false) > (size_t)ctx->lds_bytes - 1024;
    const int n_tiles = (G3 / 16) * (g.Op / 16 + Hp / 16) + 2 * (G3 / 16);

    auto enqueue_step = [&]() -> int {
        for (int k = 0; k < n_groups; ++k) {
            const int e0 = k * ng, n = std::min(ng, N - e0), rows = T * n, rows_pk = (rows + 15) & ~15;
            ga.e0 = e0; ga.n = n;
            hipLaunchKernelGGL(k_a2c_gru_gather<0>, dim3((unsigned)rows), dim3(64), 0, ctx->stream, ga);
            SG_TRY(sg_gru_forward_launch(ctx, g, pol->d_params + g.off, gb + o_x, g.ldO, gb + o_h0, gb + o_mk, T, n, gb + o_gi, hX, d.ldO,
                                         nullptr, &tr));
            for (int rb = 0, c = 0; rb < rows; rb += chunk, ++c) {
                const int cnt = std::min(chunk, rows - rb), Gc = (cnt + R - 1) / R;
                pa.mb = cnt;
                pa.X = hX + (size_t)rb * d.ldO; pa.ACT = epACT + (size_t)rb * d.A; pa.SC = epSC + rb;
                pa.DX[0] = gb + o_dxa + (size_t)rb * d.ldO; pa.DX[1] = gb + o_dxc + (size_t)rb * d.ldO;
                pa.wbuf_floats = wb_f;
                SG_TRY(ppo_launch(ctx, ppo_fwd_family, "k_ppo_fwd", SG_PROF_PPO_FWD, MT, d, dim3(Gc, d.n_trunks), lds_f, pa, gw));
                pa.wbuf_floats = wb_b;
                if (d.dist == SG_DIST_CATEGORICAL)
                    SG_TRY(ppo_launch(ctx, a2c_bwd_cat_dx_family, "k_a2c_bwd_dist_dx (Categorical)", SG_PROF_PPO_BWD, MT, d, dim3(Gc, d.n_trunks),
                                      lds_b, pa, gw));
                else if (d.dist == SG_DIST_BERNOULLI)
                    SG_TRY(ppo_launch(ctx, a2c_bwd_ber_dx_family, "k_a2c_bwd_dist_dx (Bernoulli)", SG_PROF_PPO_BWD, MT, d, dim3(Gc, d.n_trunks),
                                      lds_b, pa, gw));
                else
                    SG_TRY(ppo_launch(ctx, a2c_bwd_dx_family, "k_a2c_bwd (with d loss / d h)", SG_PROF_PPO_BWD, MT, d, dim3(Gc, d.n_trunks),
                                      lds_b, pa, gw));
                SG_LAUNCH(ctx, SG_PROF_PPO_REDUCE, k_a2c_reduce, dim3(nblk_r), dim3(256), 0, a->d_slabs, Gc, slab_stride, d.total, a->d_grad,
                          a->d_part, (k > 0 || c > 0) ? 1 : 0);
            }
            if (rows_pk > rows && n < ng) {   // a smaller last group: its padding rows hold a full group's gate gradients
                SG_CHECK(hipMemsetAsync(gb + o_dgi + (size_t)rows * G3, 0, sizeof(float) * (size_t)(rows_pk - rows) * G3, ctx->stream));
                SG_CHECK(hipMemsetAsync(gb + o_dgh + (size_t)rows * G3, 0, sizeof(float) * (size_t)(rows_pk - rows) * G3, ctx->stream));
            }
            ba.n = n;
            if (gw_scan) hipLaunchKernelGGL(k_gru_scan_bwd<true>, dim3((n + 15) / 16), dim3(256), sg_gru_bwd_lds(g, true), ctx->stream, ba);
            else hipLaunchKernelGGL(k_gru_scan_bwd<false>, dim3((n + 15) / 16), dim3(256), sg_gru_bwd_lds(g, false), ctx->stream, ba);
            wa.rows_p = rows_pk; wa.KS = ks_of(rows_pk);
            hipLaunchKernelGGL(k_gru_wgrad<0>, dim3(n_tiles, wa.KS), dim3(64), 0, ctx->stream, wa);
            hipLaunchKernelGGL(k_gru_reduce_acc<0>, dim3(gblocks), dim3(256), 0, ctx->stream, wa.partial, wa.KS, g.total, gb + o_acc,
                               k > 0 ? 1 : 0, k + 1 == n_groups ? 1 : 0, a->d_grad, d.total, a->d_part, nblk_r);
        }
        SG_LAUNCH(ctx, SG_PROF_PPO_ADAM, k_a2c_rmsprop, dim3(nblk), dim3(256), 0, pol->d_params, a->d_v, a->d_grad, a->d_part,
                  nblk_r + gblocks, tot_all, pa.st, a->alpha, (float)oma, a->cfg.eps, a->cfg.max_grad_norm, pa.inv_B, a->d_loss_acc);
        SG_CHECK(hipGetLastError());
        return 0;
    };
    const bool use_graph = !ctx->profile && !sg_env_is_off("SG_PPO_GRAPH");
    uint32_t fbits[6];
    const float fv[6] = {a->alpha, a->cfg.value_loss_coef, a->cfg.entropy_coef, a->cfg.eps, a->cfg.max_grad_norm, pa.inv_B};
    memcpy(fbits, fv, sizeof fbits);
    const uint64_t key[SG_GRAPH_KEY_WORDS] = {
            (uint64_t)(uintptr_t)a->d_slabs, (uint64_t)(uintptr_t)a->d_stacks, (uint64_t)(uintptr_t)a->d_gru,
            (uint64_t)(uintptr_t)r->d_field[SG_F_OBS], (uint64_t)(uintptr_t)r->d_field[SG_F_ACTIONS],
            (uint64_t)(uintptr_t)r->d_field[SG_F_RETURNS], (uint64_t)(uintptr_t)pol->d_params,
            (uint64_t)TN, ((uint64_t)T << 32) | (uint64_t)N, ((uint64_t)MT << 32) | (uint64_t)G,
            ((uint64_t)fbits[0] << 32) | fbits[1], ((uint64_t)fbits[2] << 32) | fbits[3],
            ((uint64_t)fbits[4] << 32) | fbits[5], (uint64_t)(uintptr_t)r->d_field[SG_F_MASKS],
            (uint64_t)(uintptr_t)a->d_h0,
            // 'A2G': A2C through time, the head's distribution (0 for the Gaussian), the group size
            0x413247ull + (gw ? 8 : 0) + (gw_scan ? 16 : 0) + ((uint64_t)d.dist << 24) + ((uint64_t)ng << 32),
            ((uint64_t)chunk << 32) | (uint64_t)rows_p, (uint64_t)KS};
    SG_TRY(sg_graph_run(ctx, &a->steps_graph, use_graph, key, enqueue_step));
    SG_CHECK(hipGetLastError());
    a->opt_t += 1;
    if (!out3) return 0;   // queued: the losses come through the results ring (step count 1)
    double acc[3];
    SG_TRY(sg_ctx_fetch_f64(ctx, a->d_loss_acc, acc, 3));
    for (int i = 0; i < 3; ++i) out3[i] = (float)acc[i];
    return 0;
}

extern "C" int sg_ppo_update(sg_ppo* a, sg_rollout* r, const int64_t* perms, int64_t n_perms, uint64_t seed, float out3[3]) {
    SG_REQUIRE(a && r, "sg_ppo_update: NULL argument");
    if (a->a2c) {
        SG_REQUIRE(!perms, "sg_ppo_update: an A2C update takes the rollout in its own order: perms must be NULL");
        if (a->a2c_rnn) return a2c_gru_update(a, r, out3);
        if (a->a2c_cnn) return a2c_cnn_update(a, r, out3);
        if (a->a2c_cnn_rnn) return a2c_cnn_gru_update(a, r, out3);
        SG_REQUIRE(r->O == a->policy->desc.O && r->A == a->policy->desc.A,
                   "sg_ppo_update: rollout dims (obs %d, act %d) do not match the policy (%d, %d)", r->O, r->A,
                   a->policy->desc.O, a->policy->desc.A);
        return a2c_update(a, r, seed, out3);
    }
    if (sg_policy_cnn_rnn(a->policy)) return cnn_gru_ppo_update(a, r, perms, n_perms, seed, out3);
    if (a->policy->recurrent) return gru_ppo_update(a, r, perms, n_perms, seed, out3);
    if (a->policy->cnn) return cnn_ppo_update(a, r, perms, n_perms, seed, out3);
    sg_ctx* ctx = a->ctx;
    const SgPolicyDesc& d = a->policy->desc;
    SG_REQUIRE(r->O == d.O && r->A == d.A, "sg_ppo_update: rollout dims (obs %d, act %d) do not match the policy (%d, %d)",
               r->O, r->A, d.O, d.A);
    const int64_t TN = (int64_t)r->T * r->N;
    const int M = a->cfg.num_mini_batch, E = a->cfg.ppo_epoch;
    // a2c/storage.py:152-157
    SG_REQUIRE(TN >= M, "PPO requires the number of processes (%d) * number of steps (%d) = %lld to be greater than "
               "or equal to the number of PPO mini batches (%d).", r->N, r->T, (long long)TN, M);
    SG_CHECK(hipSetDevice(ctx->device));
    const int world = ctx->world;
    // Minibatch geometry.  Single rank, or the library's own generator: every rank permutes its own TN rows and gives
    // TN / M of them to each step.  World > 1 with INJECTED permutations ("owned" mode, the parity form of SURVEY.md 8(e)):
    // the permutations are the reference's own draws at num_processes = world * N -- [E][TN * world] ids in its numbering
    // t * (N * world) + rank * N + n (a2c/storage.py:159-185) -- and rank r takes, of every minibatch, the rows it owns,
    // so the counts per step are uneven; row groups past a step's count are masked inside the kernels.
    const bool owned = perms != nullptr && ctx->use_comm && world > 1;
    const int64_t TN_perm = owned ? TN * world : TN;
    if (perms) {
        SG_REQUIRE(n_perms == (int64_t)E * TN_perm, "sg_ppo_update: perms holds %lld indices, %d epochs x %lld rows need %lld",
                   (long long)n_perms, E, (long long)TN_perm, (long long)E * TN_perm);
        for (int64_t i = 0; i < n_perms; ++i)
            SG_REQUIRE(perms[i] >= 0 && perms[i] < TN_perm, "sg_ppo_update: perms[%lld] = %lld is outside [0, %lld)", (long long)i,
                       (long long)perms[i], (long long)TN_perm);
    }
    std::vector<int> step_cnt((size_t)E * M), step_off((size_t)E * M);   // rows [off, off + cnt) of the epoch's permuted copy
    std::vector<int64_t> own_perm;                                       // owned mode: [E][TN] local row ids, compacted per epoch
    std::vector<int64_t> epoch_rows(E, TN);                              // rows the epoch's gather copies
    int mb = (int)(TN / M);
    int64_t mb_global = (int64_t)mb * (ctx->use_comm ? world : 1);
    if (owned) {
        const int64_t Ng = (int64_t)r->N * world;
        mb_global = TN_perm / M;
        own_perm.assign((size_t)E * TN, 0);
        mb = 1;
        std::vector<uint8_t> seen((size_t)TN_perm);
        for (int e = 0; e < E; ++e) {
            // every epoch's row must be a true permutation (a2c/storage.py:159-162 draws one): with repeated ids a rank could
            // be handed more than its T*N rows, past the end of own_perm and of the device's epoch copy
            std::fill(seen.begin(), seen.end(), (uint8_t)0);
            for (int64_t i = 0; i < TN_perm; ++i) {
                const int64_t g = perms[(size_t)e * TN_perm + i];
                SG_REQUIRE(!seen[(size_t)g], "sg_ppo_update: perms of epoch %d repeat row id %lld: not a permutation", e, (long long)g);
                seen[(size_t)g] = 1;
            }
            int64_t n_own = 0;
            for (int k = 0; k < M; ++k) {
                step_off[(size_t)e * M + k] = (int)n_own;
                for (int64_t i = 0; i < mb_global; ++i) {
                    const int64_t g = perms[(size_t)e * TN_perm + (size_t)k * mb_global + i];
                    const int64_t t = g / Ng, c = g - t * Ng, owner = c / r->N;
                    if (owner == ctx->rank) {
                        SG_REQUIRE(n_own < TN, "sg_ppo_update: epoch %d hands this rank more than its %lld rows", e, (long long)TN);
                        own_perm[(size_t)e * TN + n_own++] = t * r->N + (c - owner * r->N);
                    }
                }
                const int cnt = (int)n_own - step_off[(size_t)e * M + k];
                step_cnt[(size_t)e * M + k] = cnt;
                if (cnt > mb) mb = cnt;
            }
            epoch_rows[e] = n_own;
        }
    } else {
        for (int e = 0; e < E; ++e)
            for (int k = 0; k < M; ++k) { step_cnt[(size_t)e * M + k] = mb; step_off[(size_t)e * M + k] = k * mb; }
    }

    // mirrored observations of the rollout's T*N rows (the same for every epoch: the reference mirrors each minibatch anew)
    const bool sym = a->sym_coef > 0.f;
    if (sym) {
        if (a->d_mobs_mat) {
            SG_TRY(ensure_cap(ctx->stream, &a->d_mrows, &a->mrows_cap, TN * d.O));
            hipLaunchKernelGGL(k_mirror_rows, dim3((unsigned)((TN * d.O + 255) / 256)), dim3(256), 0, ctx->stream,
                               r->d_field[SG_F_OBS], a->d_mobs_mat, a->d_mrows, TN, d.O);
            SG_CHECK(hipGetLastError());
        } else {
            SG_REQUIRE(a->mrows_host == TN * d.O, "sg_ppo_update: the symmetry loss takes its mirrored observations from the host: "
                       "sg_ppo_set_mirrored_obs must hand over %lld floats (T*N rows of %d) before every update (pending: %lld)",
                       (long long)(TN * d.O), d.O, (long long)a->mrows_host);
            a->mrows_host = 0;
        }
    }

    SG_TRY(enqueue_adv_stats(ctx, r, a, ctx->use_comm));

    // permutations
    SG_TRY(ensure_cap(ctx->stream, &a->d_perms, &a->perms_cap, (int64_t)E * TN));
    a->last_perm_count = owned ? 0 : (int64_t)E * TN;   // owned mode: the device holds this rank's share only
    if (owned) {
        SG_CHECK(hipMemcpyAsync(a->d_perms, own_perm.data(), sizeof(int64_t) * (size_t)E * TN, hipMemcpyHostToDevice, ctx->stream));
        SG_CHECK(hipStreamSynchronize(ctx->stream));   // own_perm goes out of scope with this call
    } else if (perms) {
        SG_CHECK(hipMemcpyAsync(a->d_perms, perms, sizeof(int64_t) * (size_t)E * TN, hipMemcpyHostToDevice, ctx->stream));
        // a queued update (out3 == NULL) returns without a host wait: the caller's array must have been read by then
        if (!out3) SG_CHECK(hipStreamSynchronize(ctx->stream));
    } else {
        for (int e = 0; e < E; ++e)
            SG_TRY(sg_fill_perm(ctx, a->d_perms + (size_t)e * TN, TN, seed, (uint64_t)e * 2654435761ull + (uint64_t)ctx->rank));
    }

    // launch geometry (ppo_row_tiles).  The backward launch: the fused form keeps the whole trunk in LDS, the two-launch form
    // the trunk from w2 on; k_ppo_bwd_sym is the two-launch backward + the other actor column's head tile + M_a
    const int ncols = d.n_trunks + (sym ? 1 : 0);   // grid columns: the trunks, + the mirrored actor
    auto bwd_lds = [&](int mt, bool g) { return ppo_bwd_tiles_lds(d, mt, g ? 0 : ppo_fused(d, mt) ? max_trunk_floats(d) : max_bwd_floats(d), 2, false); };
    auto bwd_sym_lds = [&](int mt, bool g) { return ppo_bwd_tiles_lds(d, mt, g ? 0 : max_bwd_floats(d), 3, true); };
    auto fits = [&](int mt, bool g) {
        return ppo_fwd_lds(d, mt, g) <= (size_t)ctx->lds_bytes && bwd_lds(mt, g) <= (size_t)ctx->lds_bytes &&
               (!sym || bwd_sym_lds(mt, g) <= (size_t)ctx->lds_bytes);
    };
    // global-weight instances when a trunk (+ one 16-row tile) does not fit LDS: in the forward, or in the backward launch
    const bool gw = sg_policy_needs_gw(ctx, d) || !fits(1, false);
    // (SG_PPO_ROWS may ask for 64-row groups; the global-weight and the symmetric instances stop at 32)
    // (... and so do the Categorical / Bernoulli instances, which have the fused form only)
    const int MT = ppo_row_tiles(ctx, d, mb, ncols, true, 4, (gw || sym || d.dist != SG_DIST_GAUSSIAN) ? 2 : 4, [&](int mt) { return fits(mt, gw); });
    const int R = 16 * MT;
    const int G = (mb + R - 1) / R;
    const int mbp = G * R;
    const int ldP = stack_ldP(d);
    // 64-float (256-byte) multiple: k_ppo_reduce's waves read 64 consecutive floats of every slab, and with a stride that is
    // not a multiple of the 128-byte line each such read straddles three lines instead of two (round 3: FETCH_SIZE of the
    // reduce 1.4-1.95x the slab bytes before)
    const int slab_stride = (d.total + 8 + 63) & ~63;
    // slack rows: the last row tile may read past the last minibatch (owned mode: a short step still reads mbp rows)
    const int TNp = (int)TN + 64 + (owned ? mbp : 0);

    // scratch: slabs | epoch copy (X, ACT, SC[, Xm]) | per-column row stacks (H1, H2, OUT)
    // (symmetry: G more slabs for the mirrored column, the mirrored epoch copy at a 16-byte boundary, a third stack set)
    const size_t slab_f = (size_t)(sym ? 2 : 1) * G * slab_stride;
    const size_t xm_off = ((size_t)TNp * (d.ldO + d.A + 4) + 3) & ~(size_t)3;
    const size_t epoch_f = sym ? xm_off + (size_t)TNp * d.ldO : (size_t)TNp * (d.ldO + d.A + 4);
    const size_t stack_f = (size_t)ncols * mbp * (2 * (size_t)d.ldH + ldP);
    bool grew = false;
    SG_TRY(ensure_cap(ctx->stream, &a->d_slabs, &a->slabs_cap, slab_f, &grew));
    SG_TRY(ensure_cap(ctx->stream, &a->d_stacks, &a->stacks_cap, epoch_f + stack_f, &grew));
    if (grew) a->cleared.mode = SG_LAYOUT_INVALID;
    SG_TRY(clear_for_layout(a, {SG_LAYOUT_PPO, {G, slab_stride, mbp, TNp, MT, sym}}, slab_f, epoch_f + stack_f, 0));
    hipLaunchKernelGGL(k_zero_f64, dim3(1), dim3(64), 0, ctx->stream, a->d_loss_acc, 4);

    float* epX = a->d_stacks;
    float* epACT = epX + (size_t)TNp * d.ldO;
    float* epSC = epACT + (size_t)TNp * d.A;
    float* epXm = sym ? a->d_stacks + xm_off : nullptr;
    float* stk = a->d_stacks + epoch_f;

    EpochGatherArgs ga;
    ga.obs = r->d_field[SG_F_OBS]; ga.actions = r->d_field[SG_F_ACTIONS]; ga.old_logp = r->d_field[SG_F_LOGP];
    ga.adv = r->d_field[SG_F_ADVANTAGES]; ga.vpred = r->d_field[SG_F_VALUE_PREDS]; ga.ret = r->d_field[SG_F_RETURNS];
    ga.TN = TN; ga.O = d.O; ga.Op = d.Op; ga.ldO = d.ldO; ga.A = d.A; ga.sc_stride = TNp;
    ga.X = epX; ga.ACT = epACT; ga.SC = epSC;
    ga.mobs = sym ? a->d_mrows : nullptr; ga.Xm = epXm;

    PpoArgs pa;
    pa.d = d; pa.params = a->policy->d_params;
    pa.sc_stride = TNp; pa.mb = mb; pa.mbp = mbp; pa.inv_B = 1.0f / (float)mb_global;
    pa.clip = a->cfg.clip_param; pa.vcoef = a->cfg.value_loss_coef; pa.ecoef = a->cfg.entropy_coef;
    pa.use_clipped = a->cfg.use_clipped_value_loss;
    pa.slabs = a->d_slabs; pa.slab_stride = slab_stride; pa.ldP = ldP;
    pa.st = reinterpret_cast<SgOptState*>(a->d_state); pa.G = G; pa.k1 = 0;
    pa.pair = a->d_pair;
    pa.Xm = nullptr; pa.MA = a->d_mact;
    pa.sym_c = sym ? (float)(2.0 * a->sym_coef / ((double)mb_global * d.A)) : 0.f;
    for (int t = 0; t < 3; ++t) {
        const bool on = t < ncols;
        pa.H1[t] = on ? stk : nullptr; if (on) stk += (size_t)mbp * d.ldH;
        pa.H2[t] = on ? stk : nullptr; if (on) stk += (size_t)mbp * d.ldH;
        pa.OUT[t] = on ? stk : nullptr; if (on) stk += (size_t)mbp * ldP;
    }
    const int wb_f = gw ? 0 : max_trunk_floats(d), wb_b = gw ? 0 : max_bwd_floats(d);
    const bool fused = !sym && ppo_fused(d, MT);
    // SplitPolicy with more (row group, trunk) workgroups than CUs: the critic's whole fused forward + backward rides in the
    // forward launch (k_ppo_fwd_critic), the backward launch covers the two actor trunks.  SG_PPO_CRITIC_FIRST=0/1 forces it.
    const size_t lds_fc = ppo_bwd_tiles_lds(d, MT, wb_f, 2, false);   // a fused body: the whole trunk
    const char* cfenv = getenv("SG_PPO_CRITIC_FIRST");
    const bool crit_first = !gw && !fused && d.kind == SG_POLICY_SPLIT && MT <= 2 && lds_fc <= (size_t)ctx->lds_bytes &&
                            (cfenv ? cfenv[0] == '1' : G * d.n_trunks > ctx->num_cu);
    // SplitPolicy whose 3 G (row group, trunk) workgroups are all resident at once: ONE launch per step, every trunk fused,
    // the two actor workgroups of a row group exchanging their head outputs inside it (k_ppo_pair).  SG_PPO_PAIR=0: two launches.
    const char* penv = getenv("SG_PPO_PAIR");
    const bool pair = !gw && !fused && !crit_first && d.kind == SG_POLICY_SPLIT && d.n_trunks == 3 && MT <= 2 &&
                      lds_fc <= (size_t)ctx->lds_bytes && 3 * G <= ctx->num_cu && 2 * ldP + 2 <= std::min(d.trunk[0].ldH, d.trunk[1].ldH) &&
                      !a->self_wait_failed && (penv ? strcmp(penv, "0") != 0 : sg_ctx_exclusive(ctx));   // (=1 forces it on a shared device: tests)
    // (the tagged words live in the ACTOR trunks' H1 rows, indexed with the trunk's own ldH: d.ldH is the widest trunk's, which a
    // critic rebuilt wider than the actors -- sg_policy_create2 -- would make too generous a bound)
    // the words the actor pairs swap live in the H1 row stacks: an update that ran the two-launch step left activations there,
    // and a bit pattern must never be mistaken for a tagged word -- clear them whenever the mode is (re-)entered
    if (pair && !a->pair_primed) SG_CHECK(hipMemsetAsync(a->d_stacks, 0, sizeof(float) * (epoch_f + stack_f), ctx->stream));
    a->pair_primed = pair;
    const size_t lds_f = ppo_fwd_lds(d, MT, gw), lds_b = sym ? bwd_sym_lds(MT, gw) : bwd_lds(MT, gw);
    const int nblk = (d.total + 8 + 255) / 256;
    const int nblk_r = (d.total + 8 + SG_PPO_REDUCE_PARAMS - 1) / SG_PPO_REDUCE_PARAMS;
    SgOptState* st = reinterpret_cast<SgOptState*>(a->d_state);

    // The E*M optimizer steps (+ one row gather per epoch) depend only on buffer addresses, the minibatch geometry
    // and the PPO coefficients: the learning rate and Adam's step count live on the device.  The sequence is
    // captured into a hipGraph once and replayed per update, so the host issues one call instead of ~650.
    auto enqueue_steps = [&]() -> int {
        hipLaunchKernelGGL(k_opt_prepare_first, dim3(1), dim3(1), 0, ctx->stream, st);
        for (int e = 0; e < E; ++e) {
            ga.perm = a->d_perms + (size_t)e * TN;
            ga.TN = epoch_rows[e];
            if (ga.TN) hipLaunchKernelGGL(sym ? k_ppo_epoch_gather_sym : k_ppo_epoch_gather, dim3((unsigned)((ga.TN + 63) / 64)), dim3(256), 0,
                                          ctx->stream, ga);
            for (int k = 0; k < M; ++k) {
                const size_t rb = (size_t)step_off[(size_t)e * M + k];
                pa.mb = step_cnt[(size_t)e * M + k];
                pa.X = epX + rb * d.ldO; pa.ACT = epACT + rb * d.A; pa.SC = epSC + rb;
                if (sym) pa.Xm = epXm + rb * d.ldO;
                pa.k1 = e * M + k + 1;
                if (sym) {
                    pa.wbuf_floats = wb_f;
                    SG_TRY(ppo_launch(ctx, ppo_fwd_sym_family, "k_ppo_fwd_sym", SG_PROF_PPO_FWD, MT, d, dim3(G, 3), lds_f, pa, gw));
                    pa.wbuf_floats = wb_b;
                    SG_TRY(ppo_launch(ctx, ppo_bwd_sym_family, "k_ppo_bwd_sym", SG_PROF_PPO_BWD, MT, d, dim3(G, 3), lds_b, pa, gw));
                } else if (pair) {   // grid = 3 G workgroups, trunk index fastest
                    pa.wbuf_floats = wb_f;
                    SG_TRY(ppo_launch(ctx, ppo_pair_family, "k_ppo_pair", SG_PROF_PPO_BWD, MT, d, dim3(3 * G), lds_fc, pa, false));
                } else if (crit_first) {
                    pa.wbuf_floats = wb_f;
                    SG_TRY(ppo_launch(ctx, ppo_fwd_critic_family, "k_ppo_fwd_critic", SG_PROF_PPO_FWD, MT, d, dim3(G, d.n_trunks),
                                      lds_fc > lds_f ? lds_fc : lds_f, pa, false));
                    pa.wbuf_floats = wb_b;
                    SG_TRY(ppo_launch(ctx, ppo_bwd_family, "k_ppo_bwd", SG_PROF_PPO_BWD, MT, d, dim3(G, d.n_trunks - 1), lds_b, pa,
                                      false));   // trunks 0, 1: the actors
                } else if (fused) {
                    pa.wbuf_floats = wb_f;
                    if (d.dist == SG_DIST_CATEGORICAL)
                        SG_TRY(ppo_launch(ctx, ppo_bwd_fused_cat_family, "k_ppo_bwd (fused, categorical)", SG_PROF_PPO_BWD, MT, d, dim3(G, d.n_trunks), lds_b, pa, gw));
                    else if (d.dist == SG_DIST_BERNOULLI)
                        SG_TRY(ppo_launch(ctx, ppo_bwd_fused_ber_family, "k_ppo_bwd (fused, Bernoulli)", SG_PROF_PPO_BWD, MT, d, dim3(G, d.n_trunks), lds_b, pa, gw));
                    else
                        SG_TRY(ppo_launch(ctx, ppo_bwd_fused_family, "k_ppo_bwd (fused)", SG_PROF_PPO_BWD, MT, d, dim3(G, d.n_trunks), lds_b, pa, gw));
                } else {
                    pa.wbuf_floats = wb_f;
                    SG_TRY(ppo_launch(ctx, ppo_fwd_family, "k_ppo_fwd", SG_PROF_PPO_FWD, MT, d, dim3(G, d.n_trunks), lds_f, pa, gw));
                    pa.wbuf_floats = wb_b;
                    SG_TRY(ppo_launch(ctx, ppo_bwd_family, "k_ppo_bwd", SG_PROF_PPO_BWD, MT, d, dim3(G, d.n_trunks), lds_b, pa, gw));
                }
                if (sym) SG_LAUNCH(ctx, SG_PROF_PPO_REDUCE, k_ppo_reduce_sym, dim3(nblk_r), dim3(256), 0, a->d_slabs, G, slab_stride,
                                   d.total, a->d_grad, a->d_part, d.trunk[0].off, d.trunk[0].off + d.trunk[0].ex);
                else SG_LAUNCH(ctx, SG_PROF_PPO_REDUCE, k_ppo_reduce, dim3(nblk_r), dim3(256), 0, a->d_slabs, G, slab_stride,
                               d.total, a->d_grad, a->d_part);
                if (ctx->use_comm) {
                    SG_TRY(sg_comm_allreduce_f32(ctx, a->d_grad, d.total + 8));
                    hipLaunchKernelGGL(k_sumsq, dim3(nblk), dim3(256), 0, ctx->stream, a->d_grad, d.total, a->d_part);
                }
                SG_LAUNCH(ctx, SG_PROF_PPO_ADAM, sym ? k_ppo_adam_sym : k_ppo_adam, dim3(nblk), dim3(256), 0, a->policy->d_params, a->d_m,
                          a->d_v, a->d_grad, a->d_part, ctx->use_comm ? nblk : nblk_r, d.total, st, e * M + k + 1, a->cfg.eps,
                          a->cfg.max_grad_norm, pa.inv_B, a->d_loss_acc);
            }
        }
        hipLaunchKernelGGL(k_opt_commit, dim3(1), dim3(1), 0, ctx->stream, st, E * M);
        return 0;
    };
    // With a communicator the RCCL all-reduces are part of the captured sequence (RCCL enqueues them on the capturing
    // stream like any kernel), so N > 1 keeps the one-call-per-update property; SG_PPO_GRAPH_COMM=0 or a capture the
    // RCCL build refuses falls back to direct launches.
    const bool comm_ok = !ctx->use_comm || (sg_comm_graph_ok(ctx) && !sg_env_is_off("SG_PPO_GRAPH_COMM"));
    const bool use_graph = comm_ok && !owned && !ctx->profile && !sg_env_is_off("SG_PPO_GRAPH");
    uint32_t fbits[6];
    const float fv[6] = {a->cfg.clip_param, a->cfg.value_loss_coef, a->cfg.entropy_coef, a->cfg.eps, a->cfg.max_grad_norm, pa.inv_B};
    memcpy(fbits, fv, sizeof fbits);
    uint32_t cbits;
    memcpy(&cbits, &a->sym_coef, sizeof cbits);
    const uint64_t key[SG_GRAPH_KEY_WORDS] = {
            (uint64_t)(uintptr_t)a->d_slabs, (uint64_t)(uintptr_t)a->d_stacks, (uint64_t)(uintptr_t)a->d_perms,
            (uint64_t)(uintptr_t)r->d_field[SG_F_OBS], (uint64_t)(uintptr_t)r->d_field[SG_F_ACTIONS],
            (uint64_t)(uintptr_t)r->d_field[SG_F_RETURNS], (uint64_t)(uintptr_t)a->policy->d_params,
            (uint64_t)TN, ((uint64_t)E << 32) | (uint64_t)M, ((uint64_t)MT << 32) | (uint64_t)G,
            ((uint64_t)fbits[0] << 32) | fbits[1], ((uint64_t)fbits[2] << 32) | fbits[3],
            ((uint64_t)fbits[4] << 32) | fbits[5], (uint64_t)a->cfg.use_clipped_value_loss,
            (uint64_t)(uintptr_t)r->d_field[SG_F_LOGP], 0x50504full + (fused ? 1 : 0) + (ctx->use_comm ? 2 : 0) + (crit_first ? 4 : 0) + (gw ? 8 : 0) + (pair ? 16 : 0) + (sg_comm_peer_on(ctx) ? 32 : 0) + (sym ? 64 : 0) + ((uint64_t)sg_comm_peer_generation(ctx) << 32),
            sym ? (uint64_t)(uintptr_t)a->d_mrows : 0, sym ? (uint64_t)cbits : 0};   // (M_a lives at one address for the object's life: read at run time)
    SG_TRY(sg_graph_run(ctx, &a->steps_graph, use_graph, key, enqueue_steps));
    SG_CHECK(hipGetLastError());
    a->opt_t += (int64_t)E * M;
    if (!out3) return 0;   // the caller reads the losses later (sg_results_publish): the update stays queued, no host wait
    double acc[3];
    SG_TRY(sg_ctx_fetch_f64(ctx, a->d_loss_acc, acc, 3));
    if (pair && (acc[0] != acc[0] || acc[1] != acc[1] || acc[2] != acc[2])) {   // NaN: either the data, or a workgroup of k_ppo_pair gave up waiting
        unsigned err = 0;
        SG_COPY_SYNC(ctx, &err, a->d_pair + SG_PAIR_ERR_WORD, sizeof err, hipMemcpyDeviceToHost);
        if (err) {
            SG_CHECK(hipMemsetAsync(a->d_pair + SG_PAIR_ERR_WORD, 0, sizeof err, ctx->stream));
            a->self_wait_failed = true;
            SG_REQUIRE(false, "sg_ppo_update: a workgroup of k_ppo_pair waited %d s for its partner's words and gave "
                       "up (the policy's state is undefined; SG_PPO_PAIR=0 runs the multi-launch step)", (int)(SG_PAIR_TIMEOUT_TICKS / 100000000ll));
        }
    }
    const double nu = (double)E * M;
    for (int i = 0; i < 3; ++i) out3[i] = (float)(acc[i] / nu);
    return 0;
}

// ------------------------------------------------------------------------------- results ring
// One update's scalars, published without a host synchronisation: slot layout (doubles)
//   [0..2] discriminator loss sums of the last epoch (divide by [11])   [3..5] ret_rms mean / var / count   [6] sum(1 - masks)
//   [7] r_sa   [8..10] PPO loss sums (divide by [12])   [11] n_d   [12] ppo_epoch * num_mini_batch
__global__ void k_publish(double* dst, const double* d_acc, const double* d_scal, const double* p_acc, double n_d, double n_p,
                          const unsigned* d_err, const unsigned* a_err, const unsigned* peer_err) {
    const int t = threadIdx.x;
    if (t < 3) dst[t] = d_acc ? d_acc[t] : 0.0;
    else if (t < 8) dst[t] = d_scal ? d_scal[t - 3] : 0.0;
    else if (t < 11) dst[t] = p_acc ? p_acc[t - 8] : 0.0;
    else if (t == 11) dst[t] = n_d;
    else if (t == 12) dst[t] = n_p;
    // the sticky error words of the launches that wait inside themselves (k_disc_step4, k_ppo_pair): an update queued without
    // a host wait has nobody else to read them
    else if (t == 13) dst[t] = d_err ? (double)*d_err : 0.0;
    else if (t == 14) dst[t] = a_err ? (double)*a_err : 0.0;
    else if (t == 15) dst[t] = peer_err ? (double)__hip_atomic_load(peer_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;   // the peer mesh's (sg_comm.cpp)
}

extern "C" int sg_results_publish(sg_ctx* ctx, sg_disc* d, sg_ppo* a, int slot) {
    SG_REQUIRE(ctx && slot >= 0 && slot < SG_RESULT_SLOTS, "sg_results_publish: bad argument");
    SG_REQUIRE((!d || d->ctx == ctx) && (!a || a->ctx == ctx), "sg_results_publish: objects of another context");
    SG_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, ctx->stream, ctx->results + 16 * slot, d ? d->d_loss_acc : nullptr,
                       d ? d->d_scal : nullptr, a ? a->d_loss_acc : nullptr, d ? (double)d->last_n_d : 1.0,
                       a ? (double)a->cfg.ppo_epoch * a->cfg.num_mini_batch : 1.0,
                       d ? sg_disc_err_word(d) : nullptr,
                       (a && a->kfac) ? reinterpret_cast<const unsigned*>(&a->kfac->d_ks->err)   // ACKTR: the eigensolver's word
                                      : (a && a->d_pair) ? a->d_pair + SG_PAIR_ERR_WORD : nullptr,
                       sg_comm_peer_err_word(ctx));
    SG_CHECK(hipGetLastError());
    SG_CHECK(hipEventRecord(ctx->res_ev[slot], ctx->stream));
    ctx->res_d[slot] = d;
    ctx->res_a[slot] = a;
    return 0;
}

// A hand-off time-out inside a queued update surfaces HERE (the synchronous calls report it themselves): the error is
// returned, the sticky device word is cleared and the object runs its multi-launch form from now on.
extern "C" int sg_results_fetch(sg_ctx* ctx, int slot, double out13[13]) {
    SG_REQUIRE(ctx && out13 && slot >= 0 && slot < SG_RESULT_SLOTS, "sg_results_fetch: bad argument");
    SG_CHECK(hipEventSynchronize(ctx->res_ev[slot]));
    const double* src = ctx->results + 16 * slot;
    memcpy(out13, src, sizeof(double) * 13);
    const bool d_err = src[13] != 0.0;
    // slot 14 is the policy object's word: k_ppo_pair's hand-off time-out, or for an ACKTR object k_kfac_eig's sweep cap
    const bool k_err = src[14] != 0.0 && ctx->res_a[slot] && ctx->res_a[slot]->kfac;
    const bool a_err = src[14] != 0.0 && !k_err;
    if (src[15] != 0.0) {
        SG_CHECK(hipSetDevice(ctx->device));
        if (unsigned* w = sg_comm_peer_err_word(ctx)) SG_CHECK(hipMemsetAsync(w, 0, sizeof(unsigned), ctx->stream));
        SG_REQUIRE(false, "sg_results_fetch: rank %d: a peer-mesh all-reduce (SG_COMM_PEER) waited 20 s for a peer's flags and gave up "
                   "during or before the update this slot reports; that step's gradient was NaN on this rank", ctx->rank);
    }
    if (d_err || a_err) {
        SG_CHECK(hipSetDevice(ctx->device));
        sg_disc* d = ctx->res_d[slot];
        sg_ppo* a = ctx->res_a[slot];
        if (d_err && d) {
            d->self_wait_failed = true;
            SG_CHECK(hipMemsetAsync(sg_disc_err_word(d), 0, sizeof(unsigned), ctx->stream));
        }
        if (a_err && a && a->d_pair) {
            a->self_wait_failed = true;
            SG_CHECK(hipMemsetAsync(a->d_pair + SG_PAIR_ERR_WORD, 0, sizeof(unsigned), ctx->stream));
        }
        SG_REQUIRE(false, "sg_results_fetch: %s%s%s waited for workgroups of its own launch and gave up during the update this slot reports "
                   "(another process on this GPU?): the %s undefined and the slot's losses are NaN; later updates of the object run the "
                   "multi-launch form", d_err ? "k_disc_step4" : "", d_err && a_err ? " and " : "", a_err ? "k_ppo_pair" : "",
                   d_err && a_err ? "discriminator's and the policy's state are" : d_err ? "discriminator's state is" : "policy's state is");
    }
    SG_REQUIRE(!k_err, "sg_results_fetch: k_kfac_eig hit its sweep cap (%d) during or before the ACKTR update this slot reports: "
               "the K-FAC eigenbases are not valid and the update stepped with them", SG_KFAC_SWEEPS);
    return 0;
}
