// sg_disc_diag.hip -- what one looks at in the discriminator half of the GAIL-dyn loop, computed where the rows lie: accuracy,
// logit distribution and BCE on the rollout's rows and on the expert rows, the raw reward distribution, and the size of the
// input gradient dD/dx on both row sets and where the penalty acts (the mixup rows).
//
// Replaces (reference, a2c/ = third_party/a2c_ppo_acktr/) the host route to the same numbers, which update_gail_dyn does not
// return (a2c/algo/gail.py:154-193 gives three BCE means):
//   Discriminator.trunk on the T*N rows of obs_feat[1:] and on the expert matrix     a2c/algo/gail.py:166-178
//   log(s + 1e-7) - log(1 - s + 1e-7), before offset and ret_rms                     a2c/algo/gail.py:204-205
//   the mixup rows and autograd.grad(disc, mixup_data) of compute_grad_pen_combined  a2c/algo/gail.py:72-88, at alpha = 0.5
//   and the numpy reductions a caller would run on the downloaded arrays.
// Two launches, queued on the context's stream: k_disc_diag (one partial record per workgroup) and k_disc_diag_reduce.  Nothing
// but the record block and the SG_DDIAG_N results of the slot is written.
// Scope "rank" (sg_disc_diagnostics): this rank's rows, no collective.  Scope "world" (sg_disc_diagnostics_world): the statistic
// over the union of all ranks' rows, the same bits on every rank -- the rank's records folded into one, sg_comm_allgather_f64 of
// the ranks' folded records, the same fold + finalise over those in ascending rank order; the expert part is rank 0's and mid
// row (t, n) of rank k pairs with expert row (t * world * N + k * N + n) mod n_e, as one launch on the concatenated rollout
// would.  That call is a collective: every rank issues it at the same point of its stream's collectives.
#include <math.h>
#include <string.h>

#include "sg_common.h"

// A population's part of a workgroup's record, in doubles: the same twelve words for each of the three populations (what a
// population has no use for -- the mixup rows' reward, say -- costs a few flops per row and keeps one code path).
enum {
    DD_CNT = 0,              // rows
    DD_FLAG,                 // rows judged right: d < 0 (policy, mid), d > 0 (expert)
    DD_L_MEAN, DD_L_M2,      // logit
    DD_BCE,                  // sum of softplus(d) (policy, mid) / softplus(-d) (expert)
    DD_R_MEAN, DD_R_M2,      // raw reward
    DD_R_MIN, DD_R_MAX,
    DD_G_SUM,                // sum of |g|
    DD_PEN,                  // sum of (|g| - 1)^2
    DD_G_MAX,
    DD_POP = 12
};
enum { DD_POLICY = 0, DD_EXPERT, DD_MID, DD_REC = 3 * DD_POP };

struct DiscDiagArgs {
    SgDiscDesc d;
    const float* params;
    const float* policy;     // [n_p, F]: OBS_FEAT[1:]
    const float* expert;     // [n_e, F]
    int n_p, n_e;
    int tiles_p, tiles_e;    // 32-row tiles of the policy (and mid) rows, of the expert rows
    int cols, cols_g, col0;  // the mid pairing: this rank's columns N, the world's, this rank's first (rank scope: N, N, 0)
    double* rec;             // [gridDim.x][DD_REC]
};

// butterfly reductions over the 64 lanes of a wave beside sg_wave_sum (sg_gemm.hpp): every lane ends with the same bits
__device__ __forceinline__ double dd_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double dd_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// (na, *mean, *m2) <- merged with (nb, mb, m2b): Chan, Golub and LeVeque's pairwise update.  nb == 0 changes nothing.
__device__ __forceinline__ void dd_chan(double na, double* mean, double* m2, double nb, double mb, double m2b) {
    if (nb == 0.0) return;
    const double n = na + nb, delta = mb - *mean;
    *mean += delta * (nb / n);
    *m2 += m2b + delta * delta * (na * (nb / n));
}
// population part b folded into a: plain sums added, minimum / maximum taken, the two (mean, M2) pairs merged by Chan's formula
__device__ __forceinline__ void dd_merge(double* a, const double* b) {
    const double na = a[DD_CNT], nb = b[DD_CNT];
    if (nb == 0.0) return;
    a[DD_FLAG] += b[DD_FLAG]; a[DD_BCE] += b[DD_BCE]; a[DD_G_SUM] += b[DD_G_SUM]; a[DD_PEN] += b[DD_PEN];
    a[DD_R_MIN] = fmin(a[DD_R_MIN], b[DD_R_MIN]);
    a[DD_R_MAX] = fmax(a[DD_R_MAX], b[DD_R_MAX]);
    a[DD_G_MAX] = fmax(a[DD_G_MAX], b[DD_G_MAX]);
    dd_chan(na, &a[DD_L_MEAN], &a[DD_L_M2], nb, b[DD_L_MEAN], b[DD_L_M2]);
    dd_chan(na, &a[DD_R_MEAN], &a[DD_R_M2], nb, b[DD_R_MEAN], b[DD_R_M2]);
    a[DD_CNT] = na + nb;
}
__device__ __forceinline__ void dd_clear(double* a) {
#pragma unroll
    for (int k = 0; k < DD_POP; ++k) a[k] = 0.0;
    a[DD_R_MIN] = INFINITY;
    a[DD_R_MAX] = -INFINITY;
    a[DD_G_MAX] = -INFINITY;
}

// LDS of one workgroup: k_disc_forward's layout (parameter image unless GW | X | H1 | H2), then the tile's logits and gradient
// norms and the workgroup's record
static size_t disc_diag_lds_bytes(const SgDiscDesc& d, bool gw) {
    return sizeof(float) * ((gw ? 0 : (size_t)d.total) + 32 * d.ldF + 2 * 32 * d.ldH + 64) + sizeof(double) * DD_REC;
}

// Row tiles as in k_disc_forward: 32 rows, 256 threads, a capped grid with trips over the remaining tiles.  The tiles are
// numbered policy | expert | mid; a tile lies in one population.  mid row i is 0.5f * expert[g mod n_e] + 0.5f * policy[i]
// (a2c/algo/gail.py:72-75 at alpha = 0.5), formed while the tile is staged; g is row i = t * cols + n in the world's numbering,
// t * cols_g + col0 + n (< 2^31: the launcher), which is i itself at cols_g = cols, col0 = 0.  Per tile:
//   H1 = tanh(X W1^T + b1), H2 = tanh(H1 W2^T + b2), d = H2 . w3 + b3                            (k_disc_forward's forward)
//   D2 = w3 (1 - H2^2) (over H2), D1 = (D2 W2) (1 - H1^2) (over H1), G = D1 W1 (over X), |g| = ||G||_2 per row
// every contraction an LDS-tile fp32 MFMA GEMM.  Then one lane of wave 0 per row forms the row's terms -- the reward by
// k_disc_forward's expression, so these are the relabel's scores -- and the tile's rows are reduced in double by wave butterflies,
// the two (count, mean, M2) triples in two passes; lane 0 folds the tile into the workgroup's record in LDS, tile after tile in
// trip order.  No atomics: the records and their order are a function of (n_p, n_e, grid) alone.
template <bool GW>
__global__ __launch_bounds__(256) void k_disc_diag(DiscDiagArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 32;
    const SgDiscDesc& d = a.d;
    const int tid = threadIdx.x, F = d.F, ldF = d.ldF, ldH = d.ldH, Fp = d.Fp, Hp = d.Hp;
    const float* W = GW ? a.params : smem;
    float* X = smem + (GW ? 0 : d.total);
    float* H1 = X + R * ldF;
    float* H2 = H1 + R * ldH;
    float* DL = H2 + R * ldH;     // [R] logits
    float* GN = DL + R;           // [R] |g|
    double* ACC = reinterpret_cast<double*>(GN + R);   // [DD_REC] (an even number of floats from a 16-byte aligned base)
    const float* b1 = W + d.b1;
    const float* b2 = W + d.b2;
    const float* w3 = W + d.w3;
    if (!GW) sg_stage(smem, a.params, d.total / 4);
    if (tid < 3) dd_clear(ACC + tid * DD_POP);
    const int total = 2 * a.tiles_p + a.tiles_e;
    for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {
        int pop = DD_POLICY, t = tile;
        if (t >= a.tiles_p) { pop = DD_EXPERT; t -= a.tiles_p; }
        if (pop == DD_EXPERT && t >= a.tiles_e) { pop = DD_MID; t -= a.tiles_e; }
        const int base = t * R, n = pop == DD_EXPERT ? a.n_e : a.n_p;
        __syncthreads();
        {   // the row tile through range-checked buffer loads (k_disc_forward's staging): rows past n and the padding columns
            // [F, Fp) read as zero; a mid tile reads its policy rows the same way and the expert rows i mod n_e beside them
            const float* src = (pop == DD_EXPERT ? a.expert : a.policy) + (size_t)base * F;
            const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, (n - base < R ? n - base : R) * F * 4, 0x00020000);
            const __amdgpu_buffer_rsrc_t re = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.expert), 0, a.n_e * F * 4, 0x00020000);
            for (int i0 = tid; i0 < R * Fp; i0 += 4 * blockDim.x) {
                float v[4], e[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u * blockDim.x, r = i / Fp, c = i - r * Fp;
                    const bool in = i < R * Fp && c < F;
                    v[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, in ? (r * F + c) * 4 : 0x7ffffff0, 0, 0));
                    e[u] = 0.f;
                    if (pop == DD_MID) {
                        const unsigned t = (unsigned)(base + r) / (unsigned)a.cols;
                        const unsigned g = t * (unsigned)a.cols_g + (unsigned)a.col0 + ((unsigned)(base + r) - t * (unsigned)a.cols);
                        e[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(re, in ? (int)((g % (unsigned)a.n_e) * F + c) * 4 : 0x7ffffff0, 0, 0));
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + u * blockDim.x, r = i / Fp, c = i - r * Fp;
                    if (i < R * Fp) X[r * ldF + c] = pop == DD_MID ? 0.5f * e[u] + 0.5f * v[u] : v[u];
                }
            }
        }
        __syncthreads();
        sg_layer_nt<2, GW>(X, ldF, W + d.w1, ldF, Fp, Hp, [&](int r, int c, float v) { H1[r * ldH + c] = sg_tanh(v + b1[c]); });
        __syncthreads();
        sg_layer_nt<2, GW>(H1, ldH, W + d.w2, ldH, Hp, Hp, [&](int r, int c, float v) { H2[r * ldH + c] = sg_tanh(v + b2[c]); });
        __syncthreads();
        {   // the logit, and D2 over H2: an element is read and rewritten by the one lane that owns it
            const int r = tid >> 3, sub = tid & 7;
            float s = 0.f;
            for (int c = sub; c < Hp; c += 8) {
                const float h = H2[r * ldH + c], w = w3[c];
                s += h * w;
                H2[r * ldH + c] = w * (1.0f - h * h);
            }
            s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
            if (sub == 0) DL[r] = s + W[d.b3];
        }
        __syncthreads();
        // D1 over H1: the GEMM reads H2 and W2 only, the epilogue's element is its lane's alone
        sg_layer_nn<2>(H2, ldH, W + d.w2, ldH, Hp, Hp, [&](int r, int c, float v) {
            const float h = H1[r * ldH + c];
            H1[r * ldH + c] = v * (1.0f - h * h);
        });
        __syncthreads();
        sg_layer_nn<2>(H1, ldH, W + d.w1, ldF, Hp, Fp, [&](int r, int c, float v) { X[r * ldF + c] = v; });
        __syncthreads();
        {
            const int r = tid >> 3, sub = tid & 7;
            float q = 0.f;
            for (int c = sub; c < Fp; c += 8) { const float g = X[r * ldF + c]; q += g * g; }   // (the padding columns hold zeros)
            q += __shfl_xor(q, 1); q += __shfl_xor(q, 2); q += __shfl_xor(q, 4);
            if (sub == 0) GN[r] = sqrtf(q);
        }
        __syncthreads();
        if (tid < 64) {   // wave 0: a tile's 32 rows in its lower half
            const bool live = tid < R && base + tid < n;
            double flag = 0.0, lg = 0.0, bce = 0.0, rw = 0.0, gn = 0.0, pen = 0.0;
            if (live) {
                const float dl = DL[tid];
                const float sg = 1.f / (1.f + expf(-dl));
                const float z = pop == DD_EXPERT ? -dl : dl;     // binary_cross_entropy_with_logits against 1 / against 0
                flag = z < 0.f ? 1.0 : 0.0;                      // d == 0 is wrong for both
                lg = (double)dl;
                bce = (double)(fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))));
                rw = (double)(logf(sg + 1e-7f) - logf(1.f - sg + 1e-7f));   // a2c/algo/gail.py:204-205
                gn = (double)GN[tid];
                pen = (gn - 1.0) * (gn - 1.0);
            }
            const double c = sg_wave_sum(live ? 1.0 : 0.0);   // >= 1: every tile holds a row
            const double s_flag = sg_wave_sum(flag), s_bce = sg_wave_sum(bce), s_gn = sg_wave_sum(gn), s_pen = sg_wave_sum(pen);
            const double r_min = dd_wave_min(live ? rw : (double)INFINITY), r_max = dd_wave_max(live ? rw : -(double)INFINITY);
            const double g_max = dd_wave_max(live ? gn : -(double)INFINITY);
            const double m_lg = sg_wave_sum(lg) / c, m_rw = sg_wave_sum(rw) / c;
            const double d_lg = live ? lg - m_lg : 0.0, d_rw = live ? rw - m_rw : 0.0;
            const double q_lg = sg_wave_sum(d_lg * d_lg), q_rw = sg_wave_sum(d_rw * d_rw);
            if (tid == 0) {
                double b[DD_POP];
                b[DD_CNT] = c; b[DD_FLAG] = s_flag; b[DD_L_MEAN] = m_lg; b[DD_L_M2] = q_lg; b[DD_BCE] = s_bce;
                b[DD_R_MEAN] = m_rw; b[DD_R_M2] = q_rw; b[DD_R_MIN] = r_min; b[DD_R_MAX] = r_max;
                b[DD_G_SUM] = s_gn; b[DD_PEN] = s_pen; b[DD_G_MAX] = g_max;
                dd_merge(ACC + pop * DD_POP, b);
            }
        }
    }
    __syncthreads();
    if (tid < DD_REC) a.rec[(size_t)blockIdx.x * DD_REC + tid] = ACC[tid];
}

// One workgroup of one wave.  Population by population, the nrec records' parts are merged in ascending workgroup order, all in
// double, in two levels: lane i folds the contiguous run [i * per, (i + 1) * per) of them, in order, into its own part, then
// lane 0 folds the 64 lane parts, in order.  The shape of that tree depends on nrec alone.  A part folded into the empty
// accumulator keeps its bits, so one record through this fold is that record.
//   DD_FINAL  the fold, then the results: out[SG_DDIAG_N] (include/simgan_hip.h), and out[SG_DDIAG_N] itself = 0
//   DD_FOLD   the fold alone: out[DD_REC] is the folded record
//   DD_WORLD  DD_FINAL over the ranks' folded records in ascending rank order -- the policy and mid parts; every rank holds the
//             whole expert matrix (sg_disc_set_expert; the update slices the batch by rank, not the matrix), so the world's expert
//             population is one rank's: rank 0's part is taken, none merged.  out[SG_DDIAG_N] = 1 if the ranks' policy row
//             counts differ, + 2 if their expert row counts do -- the fetch then refuses the numbers
enum { DD_FINAL = 0, DD_FOLD, DD_WORLD };
template <int MODE>
__global__ __launch_bounds__(64) void k_disc_diag_reduce(const double* rec, int nrec, double* out) {
    __shared__ double part[64][DD_POP + 1];
    const int lane = threadIdx.x;
    const int per = (nrec + 63) / 64;
    double g_max = -INFINITY;
    for (int pop = 0; pop < 3; ++pop) {
        const int npop = MODE == DD_WORLD && pop == DD_EXPERT ? 1 : nrec;
        double acc[DD_POP];
        dd_clear(acc);
        for (int i = lane * per; i < npop && i < (lane + 1) * per; ++i) {
            double b[DD_POP];
#pragma unroll
            for (int k = 0; k < DD_POP; ++k) b[k] = rec[(size_t)i * DD_REC + pop * DD_POP + k];
            dd_merge(acc, b);
        }
        __syncthreads();   // (the previous population's parts have been read)
#pragma unroll
        for (int k = 0; k < DD_POP; ++k) part[lane][k] = acc[k];
        __syncthreads();
        if (lane != 0) continue;
        for (int j = 1; j < 64; ++j) {
            double b[DD_POP];
#pragma unroll
            for (int k = 0; k < DD_POP; ++k) b[k] = part[j][k];
            dd_merge(acc, b);
        }
        if (MODE == DD_FOLD) {
#pragma unroll
            for (int k = 0; k < DD_POP; ++k) out[pop * DD_POP + k] = acc[k];
            continue;
        }
        const double n = acc[DD_CNT];
        g_max = fmax(g_max, acc[DD_G_MAX]);
        if (pop == DD_POLICY) {
            out[0] = n;
            out[2] = acc[DD_FLAG] / n;
            out[4] = acc[DD_L_MEAN];
            out[5] = sqrt(acc[DD_L_M2] / n);     // population standard deviations
            out[8] = acc[DD_BCE] / n;
            out[10] = acc[DD_R_MEAN];
            out[11] = sqrt(acc[DD_R_M2] / n);
            out[12] = acc[DD_R_MIN];
            out[13] = acc[DD_R_MAX];
            out[14] = acc[DD_G_SUM] / n;
        } else if (pop == DD_EXPERT) {
            out[1] = n;
            out[3] = acc[DD_FLAG] / n;
            out[6] = acc[DD_L_MEAN];
            out[7] = sqrt(acc[DD_L_M2] / n);
            out[9] = acc[DD_BCE] / n;
            out[15] = acc[DD_G_SUM] / n;
        } else {
            out[16] = acc[DD_G_SUM] / n;
            out[17] = 10.0 * (acc[DD_PEN] / n);  // lambda = 10, a2c/algo/gail.py:67
            out[18] = g_max;
            double differ = 0.0;
            if (MODE == DD_WORLD) {
                bool rows = false, experts = false;
                for (int i = 1; i < nrec; ++i) {
                    rows |= rec[(size_t)i * DD_REC + DD_POLICY * DD_POP + DD_CNT] != rec[DD_POLICY * DD_POP + DD_CNT];
                    experts |= rec[(size_t)i * DD_REC + DD_EXPERT * DD_POP + DD_CNT] != rec[DD_EXPERT * DD_POP + DD_CNT];
                }
                differ = (rows ? 1.0 : 0.0) + (experts ? 2.0 : 0.0);
            }
            out[SG_DDIAG_N] = differ;
        }
    }
}

// Both scopes.  `who` names the entry point in the messages (the rank scope's are pinned by its tests).
static int disc_diagnostics(const char* who, bool world_scope, sg_disc* d, sg_rollout* r, int slot, double* out19) {
    SG_REQUIRE(d && r, "%s: NULL argument", who);
    SG_REQUIRE(slot == 0 || slot == 1, "%s: slot %d is out of range (two results may be pending: slot 0 or 1)", who, slot);
    SG_REQUIRE(d->ctx == r->ctx, "%s: the discriminator and the rollout live on different contexts", who);
    SG_REQUIRE(r->F == d->desc.F, "%s: rollout feat_len %d != discriminator input_dim %d", who, r->F, d->desc.F);
    SG_REQUIRE(d->d_expert && d->n_expert > 0, "%s: no expert data (call sg_disc_set_expert first)", who);
    SG_REQUIRE((int64_t)r->T * r->N < (1ll << 30), "%s: T*N = %lld rows: fewer than 2^30 are taken", who, (long long)r->T * r->N);
    SG_REQUIRE(d->n_expert * d->desc.F < (1ll << 29), "%s: an expert matrix of %lld x %d floats: fewer than 2^29 are taken", who,
               (long long)d->n_expert, d->desc.F);
    sg_ctx* ctx = d->ctx;
    const SgDiscDesc& dd = d->desc;
    // world scope: the ranks' records are gathered when there is a communicator, and a mid row pairs with the expert row of its
    // number in the world's rollout
    const bool gather = world_scope && ctx->comm;
    const int world = gather ? ctx->world : 1, rank = gather ? ctx->rank : 0;
    SG_REQUIRE((int64_t)world * r->T * r->N < (1ll << 31), "%s: %d ranks of T*N = %lld rows: fewer than 2^31 rows in the world are taken",
               who, world, (long long)r->T * r->N);
    // the weight path of the forward launch (SG_DISC_GW=1 forces global weights), or the image does not fit beside this tile
    const bool gw = sg_disc_needs_gw(ctx, dd) || disc_diag_lds_bytes(dd, false) > (size_t)ctx->lds_bytes;
    const size_t lds = disc_diag_lds_bytes(dd, gw);
    SG_REQUIRE(lds <= (size_t)ctx->lds_bytes, "%s: the activation tiles of a (%d x %d) discriminator need %zu bytes of LDS, "
               "the CU has %d", who, dd.F, dd.Hd, lds, ctx->lds_bytes);
    SG_CHECK(hipSetDevice(ctx->device));
    if (!d->h_ddiag) {
        SG_CHECK(sg_host_malloc((void**)&d->h_ddiag, sizeof(double) * 2 * SG_DDIAG_STRIDE));
        for (int s = 0; s < 2; ++s) SG_CHECK(hipEventCreateWithFlags(&d->ddiag_ev[s], hipEventDisableTiming));
    }
    DiscDiagArgs a;
    a.d = dd; a.params = d->d_params;
    a.policy = r->d_field[SG_F_OBS_FEAT] + (size_t)r->N * r->F;
    a.expert = d->d_expert;
    a.n_p = r->T * r->N; a.n_e = (int)d->n_expert;
    a.tiles_p = (a.n_p + 31) / 32; a.tiles_e = (a.n_e + 31) / 32;
    a.cols = r->N; a.cols_g = world * r->N; a.col0 = rank * r->N;
    int grid = 2 * a.tiles_p + a.tiles_e;
    if (grid > 2 * ctx->num_cu) grid = 2 * ctx->num_cu;
    // (sized for the capped grid once, with the world scope's folded record and the ranks' gathered ones behind it: a result
    // pending in the other slot never sees the block move)
    const size_t grid_doubles = (size_t)2 * ctx->num_cu * DD_REC;
    SG_TRY(ensure_cap(ctx->stream, &d->d_ddiag, &d->ddiag_cap, grid_doubles + (size_t)(1 + ctx->world) * DD_REC));
    a.rec = d->d_ddiag;
    if (gw) hipLaunchKernelGGL(k_disc_diag<true>, dim3(grid), dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL(k_disc_diag<false>, dim3(grid), dim3(256), lds, ctx->stream, a);
    SG_CHECK(hipGetLastError());
    double* out = d->h_ddiag + slot * SG_DDIAG_STRIDE;
    if (!world_scope) {
        hipLaunchKernelGGL(k_disc_diag_reduce<DD_FINAL>, dim3(1), dim3(64), 0, ctx->stream, d->d_ddiag, grid, out);
    } else {
        double* mine = d->d_ddiag + grid_doubles;
        double* all = mine + DD_REC;
        hipLaunchKernelGGL(k_disc_diag_reduce<DD_FOLD>, dim3(1), dim3(64), 0, ctx->stream, d->d_ddiag, grid, mine);
        SG_CHECK(hipGetLastError());
        if (gather) SG_TRY(sg_comm_allgather_f64(ctx, mine, all, DD_REC));
        hipLaunchKernelGGL(k_disc_diag_reduce<DD_WORLD>, dim3(1), dim3(64), 0, ctx->stream, gather ? all : mine, world, out);
    }
    SG_CHECK(hipGetLastError());
    SG_CHECK(hipEventRecord(d->ddiag_ev[slot], ctx->stream));
    d->ddiag_pending[slot] = true;
    if (out19) return sg_disc_diagnostics_fetch(d, slot, out19);
    return 0;
}

extern "C" int sg_disc_diagnostics(sg_disc* d, sg_rollout* r, int slot, double* out19) {
    return disc_diagnostics("sg_disc_diagnostics", false, d, r, slot, out19);
}

// The world scope: k_disc_diag with the world's mid pairing, the fold alone, the all-gather of the ranks' 36-double records,
// fold + finalise over them.  A COLLECTIVE: every rank issues it at the same point of its stream's sequence of collectives, in
// either discriminator data-parallel mode.  No communicator: the rank scope's bits.
extern "C" int sg_disc_diagnostics_world(sg_disc* d, sg_rollout* r, int slot, double* out19) {
    return disc_diagnostics("sg_disc_diagnostics_world", true, d, r, slot, out19);
}

extern "C" int sg_disc_diagnostics_fetch(sg_disc* d, int slot, double out19[SG_DDIAG_N]) {
    SG_REQUIRE(d && out19, "sg_disc_diagnostics_fetch: NULL argument");
    SG_REQUIRE(slot == 0 || slot == 1, "sg_disc_diagnostics_fetch: slot %d is out of range (two results may be pending: slot 0 or 1)", slot);
    SG_REQUIRE(d->ddiag_pending[slot], "sg_disc_diagnostics_fetch: no diagnostics are pending in slot %d of this discriminator (queue them "
               "with sg_disc_diagnostics(..., out19 = NULL) first; a result is fetched once)", slot);
    SG_CHECK(hipEventSynchronize(d->ddiag_ev[slot]));
    d->ddiag_pending[slot] = false;
    const double differ = d->h_ddiag[slot * SG_DDIAG_STRIDE + SG_DDIAG_N];
    SG_REQUIRE(differ != 1.0 && differ != 3.0, "sg_disc_diagnostics_fetch: the ranks of the world scope hold different numbers of rows "
               "(%lld in all): the global numbering takes equal column shards, no numbers are returned",
               (long long)d->h_ddiag[slot * SG_DDIAG_STRIDE]);
    SG_REQUIRE(differ == 0.0, "sg_disc_diagnostics_fetch: the ranks of the world scope hold expert matrices of different numbers of rows "
               "(rank 0: %lld): every rank holds the whole expert matrix, no numbers are returned",
               (long long)d->h_ddiag[slot * SG_DDIAG_STRIDE + 1]);
    memcpy(out19, d->h_ddiag + slot * SG_DDIAG_STRIDE, sizeof(double) * SG_DDIAG_N);
    return 0;
}
