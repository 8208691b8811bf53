// sg_policy_fwd.hpp -- what the translation units that run a policy's trunks forward share (sg_policy.hip, sg_act_step.hip):
// the trunk forward on an LDS row tile, the LDS budget of the forward launch and its choice of row tile.
#pragma once
#include "sg_common.h"

#define HALF_LOG_2PI 0.91893853320467274178f
#define SG_ACT_STREAM 0x41435400ull

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
