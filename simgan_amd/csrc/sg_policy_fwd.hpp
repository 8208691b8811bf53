// sg_policy_fwd.hpp -- what the translation units that run a policy's trunks forward and act on the result share (sg_policy.hip,
// sg_act_step.hip, sg_act_chain.hip): row-tile staging, the trunk forward on an LDS row tile and the loop over a policy's trunks,
// the Gaussian head of one row, the LDS budgets and row tiles of the forward and the ensemble launch, and the host-side launch
// dispatch over (row tile, weight path).  Every launch that must reproduce sg_policy_act's bits calls these, so it does.
#pragma once
#include <type_traits>

#include "sg_common.h"
#include "sg_rng.hpp"

#define SG_ACT_STREAM 0x41435400ull

// Fills the [R][ld] LDS tile X, columns [0, cols), from global rows: local row r takes value(row, c) of row = rowmap(r) for
// c < width, zero where rowmap(r) < 0 (no such row) and in the padding columns.  No barrier inside.
template <typename M, typename V>
__device__ __forceinline__ void stage_rows(float* X, int R, int cols, int ld, int width, M&& rowmap, V&& value) {
    for (int i = threadIdx.x; i < R * cols; i += blockDim.x) {
        const int r = i / cols, c = i - r * cols;
        const auto row = rowmap(r);   // (int, or int64_t where the map is a gather through 64-bit indices)
        X[r * ld + c] = (row >= 0 && c < width) ? value(row, c) : 0.f;
    }
}
// ... from the [*, width] rows of src themselves
template <typename M>
__device__ __forceinline__ void stage_rows(float* X, int R, int cols, int ld, const float* src, int width, M&& rowmap) {
    stage_rows(X, R, cols, ld, width, rowmap, [&](auto row, int c) { return src[(size_t)row * width + c]; });
}

// One trunk forward on R = 16*MT rows held in LDS.  W = the trunk's parameter block: its LDS image, or (GW) the block in
// global memory itself -- the general-shape path for trunks that do not fit a CU's LDS (any hidden size the reference's
// --hidden-size accepts, a2c/arguments.py:107-109; weights come through L2 one MFMA fragment at a time, sg_gemm.hpp).
template <int MT, bool GW = false>
__device__ __forceinline__ void trunk_forward(const SgPolicyDesc& d, const SgTrunk& tr, const float* W,
                                              const float* X, float* H1, float* H2, float* OUT,
                                              int ldP) {
    const int ldO = d.ldO, ldH = tr.ldH, Hp = tr.Hp;   // this trunk's own width (the critic's may differ from the actors')
    const float* b1 = W + tr.b1;
    const float* b2 = W + tr.b2;
    const float* bh = W + tr.bh;
    sg_layer_nt<MT, GW>(X, ldO, W + tr.w1, ldO, d.Op, Hp,
                        [&](int r, int c, float v) { H1[r * ldH + c] = sg_tanh(v + b1[c]); });
    __syncthreads();
    sg_layer_nt<MT, GW>(H1, ldH, W + tr.w2, ldH, Hp, Hp,
                        [&](int r, int c, float v) { H2[r * ldH + c] = sg_tanh(v + b2[c]); });
    __syncthreads();
    sg_layer_nt<MT, GW>(H2, ldH, W + tr.wh, ldH, Hp, tr.Pp,
                        [&](int r, int c, float v) { OUT[r * ldP + c] = v + bh[c]; });
}

// Every trunk of a policy on the R = 16*MT rows X, trunk t's head outputs to OUT + t * R * ldPmax (stride tr.ldP).  The trunks'
// parameter blocks take the SAME LDS region (smem) in turn, or are read from global memory (GW).  dual: a launch whose
// stand-alone form would run 16-row tiles (fwd_tile_mt: two interleaved accumulators per dot product) runs 16 rows at a time
// here too, whatever MT is.  Barriers before the first staging and after the last trunk.
template <int MT, bool GW>
__device__ __forceinline__ void run_trunks(const SgPolicyDesc& d, const float* params, bool dual, float* smem, const float* X,
                                           float* H1, float* H2, float* OUT, int ldPmax) {
    constexpr int R = 16 * MT;
    for (int t = 0; t < d.n_trunks; ++t) {
        const SgTrunk tr = d.trunk[t];
        __syncthreads();
        if (!GW) sg_stage(smem, params + tr.off, tr.size / 4);
        __syncthreads();
        const float* W = GW ? params + tr.off : smem;
        float* out = OUT + t * R * ldPmax;
        if (MT == 1 || !dual) trunk_forward<MT, GW>(d, tr, W, X, H1, H2, out, tr.ldP);
        else
            for (int s = 0; s < MT; ++s)
                trunk_forward<1, GW>(d, tr, W, X + s * 16 * d.ldO, H1 + s * 16 * tr.ldH, H2 + s * 16 * tr.ldH, out + s * 16 * tr.ldP, tr.ldP);
    }
    __syncthreads();
}

// The Gaussian head of ONE row (DiagGaussian / StateDiagGaussianNew / FixedNormal, a2c/distributions.py:51-59,91-118,
// a2c/model_split.py:201-238): the one copy of this arithmetic, for every launch that acts.  h0 / h1: the row's head outputs
// of trunks 0 and 1 (h1 is read by the split policy only); row: the ORIGINAL row number -- it indexes noise, action_in and the
// library's draws, so a row's action does not depend on how a launch groups the rows.  mode 0: sample with noise (or the
// library's draw if noise is NULL); 1: deterministic; 2: evaluate action_in.  emit(k, act) takes the actions in ascending k.
// Returns the log-prob; ENT: *ent takes the entropy too.
template <bool ENT = false, typename F>
__device__ __forceinline__ float gauss_head_row(const SgPolicyDesc& d, const float* params, const float* h0, const float* h1, int row,
                                                int mode, const float* noise, const float* action_in, uint64_t seed, uint64_t stream,
                                                F&& emit, float* ent = nullptr) {
    float logp = 0.f, e = 0.f;
    for (int k = 0; k < d.A; ++k) {
        float mean, ls;
        if (d.kind == SG_POLICY_MLP) {
            mean = h0[k];
            ls = params[d.trunk[0].off + d.trunk[0].ex + k];
        } else if (k < d.nc) {
            mean = h0[k];
            ls = h0[d.nc + k];
        } else {
            mean = h1[k - d.nc];
            ls = h1[d.na + k - d.nc];
        }
        const float sigma = expf(ls);
        float act;
        if (action_in && mode == 2) act = action_in[(size_t)row * d.A + k];   // (a literal NULL folds the branch away)
        else if (mode == 1) act = mean;
        else {
            const float z = noise ? noise[(size_t)row * d.A + k] : sg_normal(seed, stream, (uint64_t)row * d.A + k);
            act = z * sigma + mean;
        }
        emit(k, act);
        const float diff = act - mean, var = sigma * sigma;
        logp += -(diff * diff) / (2.0f * var) - logf(sigma) - HALF_LOG_2PI;
        if (ENT) e += 0.5f + HALF_LOG_2PI + logf(sigma);
    }
    if (ENT) *ent = e;
    return logp;
}

// LDS floats needed by the forward kernel / the PPO gradient kernel for a given MT.
static inline int max_trunk_size(const SgPolicyDesc& d, int t0, int nt) {
    int m = 0;
    for (int t = t0; t < t0 + nt; ++t) m = d.trunk[t].size > m ? d.trunk[t].size : m;
    return m;
}
static inline int max_ldP(const SgPolicyDesc& d) {
    int m = 0;
    for (int t = 0; t < d.n_trunks; ++t) m = d.trunk[t].ldP > m ? d.trunk[t].ldP : m;
    return m;
}
static inline size_t fwd_lds_bytes(const SgPolicyDesc& d, int MT, bool gw = false) {
    const int R = 16 * MT;
    return sizeof(float) * (size_t)((gw ? 0 : max_trunk_size(d, 0, d.n_trunks)) + R * d.ldO + 2 * R * d.ldH + R * max_ldP(d));
}
// Row tile (16*MT rows) of the forward launch over n rows: the largest that fits LDS and is not mostly padding.  MT == 1 sums a
// dot product in two interleaved accumulators (sg_mma_nt, DUAL), MT > 1 in one: a launch that must reproduce the forward
// launch's bits (k_policy_act_step) has to fall on the same side.
static inline int fwd_tile_mt(const sg_ctx* ctx, const SgPolicyDesc& d, int n, bool gw) {
    int MT = 4;
    while (MT > 1 && (fwd_lds_bytes(d, MT, gw) > (size_t)ctx->lds_bytes - 1024 || 16 * (MT / 2) >= n)) MT /= 2;
    return MT;
}

// The ensemble launch (k_policy_act_ensemble, sg_policy.hip): its LDS budget, its weight path and its row tile -- 32-row tiles
// unless the pool is small or LDS is short.  Shared with the chained act (sg_act_chain.hip), whose member half has to fall on
// the same weight path and the same side of MT == 1.
static inline size_t ens_lds_bytes(const SgPolicyDesc& d, int MT, bool gw = false) {
    const int R = 16 * MT;
    return sizeof(float) * (size_t)((gw ? 0 : max_trunk_size(d, 0, d.n_trunks)) + R * d.ldO + 2 * R * d.ldH + d.n_trunks * R * max_ldP(d)) +
           sizeof(int) * (size_t)(R + 256 + 4);
}
static inline bool ens_needs_gw(const sg_ctx* ctx, const SgPolicyDesc& d) {
    return sg_policy_needs_gw(ctx, d) || ens_lds_bytes(d, 1) > (size_t)ctx->lds_bytes - 1024;
}
static inline int ens_tile_mt(const sg_ctx* ctx, const SgPolicyDesc& d, int n, int n_policies, bool gw) {
    int MT = 2;
    while (MT > 1 && (ens_lds_bytes(d, MT, gw) > (size_t)ctx->lds_bytes - 1024 || 16 * MT * n_policies > 2 * n)) MT /= 2;
    return MT;
}
// What a launch over an ensemble asks of its n members and of idx[n_rows]: live feed-forward MLP-trunk policies of ctx with the
// Gaussian head and member 0's shape; every idx inside [0, n).  who: the entry point, what: its launch ("the ensemble launch").
static inline int ens_check_members(const char* who, const char* what, const sg_ctx* ctx, sg_policy* const* members, int n,
                                    const int32_t* idx, int n_rows) {
    for (int k = 0; k < n; ++k) {
        SG_REQUIRE(members[k] && members[k]->ctx == ctx, "%s: member %d is NULL or lives on another context", who, k);
        SG_REQUIRE(!sg_policy_cnn_rnn(members[k]), "%s: member %d has the recurrent CNN base (sg_policy_create_cnn_rnn); %s runs the MLP "
                   "trunks only and carries no hidden state", who, k, what);
        SG_REQUIRE(!members[k]->cnn, "%s: member %d has the CNN base (image observations); %s runs the MLP trunks only", who, k, what);
        SG_REQUIRE(!members[k]->recurrent, "%s: member %d is a recurrent policy; %s carries no hidden state (feed-forward policies only)",
                   who, k, what);
        const SgPolicyDesc &e = members[k]->desc, &d = members[0]->desc;
        SG_REQUIRE(e.dist == SG_DIST_GAUSSIAN, "%s: member %d has a Categorical / Bernoulli head; %s carries the Gaussian head only (Box "
                   "action spaces)", who, k, what);
        SG_REQUIRE(e.kind == d.kind && e.O == d.O && e.A == d.A && e.H == d.H && e.Hc == d.Hc && e.num_feet == d.num_feet,
                   "%s: member %d has a different shape", who, k);
    }
    for (int i = 0; i < n_rows; ++i) SG_REQUIRE(idx[i] >= 0 && idx[i] < n, "%s: idx[%d] = %d outside [0, %d)", who, i, idx[i], n);
    return 0;
}

// Host side: calls launch(mt, g) with mt = std::integral_constant<int, MT> and g = std::bool_constant<gw> for the run-time pair
// (MT, gw), MT in {MTMAX, .., 2, 1}: a generic lambda that launches kernel<decltype(mt)::value, decltype(g)::value> instantiates
// the kernel for exactly those pairs.
template <int MTMAX, typename F>
static inline void sg_dispatch_mt_gw(int MT, bool gw, F&& launch) {
    auto both = [&](auto mt) {
        if (gw) launch(mt, std::true_type{});
        else launch(mt, std::false_type{});
    };
    if constexpr (MTMAX >= 4) {
        if (MT == 4) return both(std::integral_constant<int, 4>{});
    }
    if (MT == 2) both(std::integral_constant<int, 2>{});
    else both(std::integral_constant<int, 1>{});
}
