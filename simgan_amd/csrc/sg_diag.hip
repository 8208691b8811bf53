// sg_diag.hip -- what one looks at after an update, computed where the rollout lies: approximate KL, clip fraction, entropy,
// ratio range, explained variance and value error of a policy over the T*N rows of a device rollout.
//
// Replaces (reference, a2c/ = third_party/a2c_ppo_acktr/) the host route to the same numbers, which the reference's learners do
// not return (a2c/algo/ppo.py:65-157 and a2c/algo/a2c_acktr.py:52-102 give value loss, action loss and entropy only):
//   Policy.evaluate_actions / SplitPolicy.evaluate_actions on all T*N rows   a2c/model.py:107-114, a2c/model_split.py:84-95
//   ratio = exp(action_log_probs - old_action_log_probs)                    a2c/algo/ppo.py:93-94
//   and the numpy reductions a caller would run on the three downloaded arrays.
// Two launches, queued on the context's stream: k_policy_diag (one partial record per workgroup) and k_policy_diag_reduce; a
// recurrent policy runs the GRU forward of sg_gru.hip over the rollout first.  Nothing but the record block and the ten results
// is written.
// Scope "rank" (sg_rollout_policy_diagnostics): this rank's rows, no collective.  Scope "world"
// (sg_rollout_policy_diagnostics_world): the statistic over the union of all ranks' rows, the same bits on every rank -- the
// rank's records folded into one, sg_comm_allgather_f64 of the ranks' folded records, the same fold + finalise over those in
// ascending rank order.  That call is a collective: every rank issues it at the same point of its stream's collectives.
#include <math.h>
#include <string.h>

#include "sg_common.h"
#include "sg_gru_kernels.hpp"
#include "sg_policy_fwd.hpp"

// A workgroup's partial record, in doubles.  The three (count, mean, M2) triples cover the same rows and share word 0.
enum {
    DG_CNT = 0,    // rows
    DG_NEGD,       // sum of -(logp_new - logp_old)
    DG_K3,         // sum of (r - 1) - log r
    DG_FLAG,       // rows with |r - 1| > clip
    DG_ENT,        // sum of the entropy
    DG_RMIN, DG_RMAX,
    DG_SQ,         // sum of (ret - v_new)^2
    DG_RET_MEAN, DG_RET_M2,      // ret
    DG_EO_MEAN, DG_EO_M2,        // ret - vpred
    DG_EN_MEAN, DG_EN_M2,        // ret - v_new
    DG_REC = 16
};

struct DiagArgs {
    SgPolicyDesc d;
    const float* params;
    const float* x;          // [n, d.O]: OBS[:-1], or the GRU states of a recurrent policy
    const float* action;     // [n, A]: ACTIONS
    const float* logp_old;   // [n]: LOGP
    const float* vpred;      // [n]: VALUE_PREDS[:-1]
    const float* ret;        // [n]: RETURNS[:-1]
    int n;
    float clip;
    double* rec;             // [tiles][DG_REC]
    int wbuf_floats, ldPmax;
};

// Butterfly reductions over the 64 lanes of a wave: every lane ends with the same bits, in an order that is the wave's alone.
__device__ __forceinline__ double dg_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double dg_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double dg_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// (na, *mean, *m2) <- merged with (nb, mb, m2b): Chan, Golub and LeVeque's pairwise update.  nb == 0 changes nothing.
__device__ __forceinline__ void dg_chan(double na, double* mean, double* m2, double nb, double mb, double m2b) {
    if (nb == 0.0) return;
    const double n = na + nb, delta = mb - *mean;
    *mean += delta * (nb / n);
    *m2 += m2b + delta * delta * (na * (nb / n));
}

// Categorical / Bernoulli evaluation of ONE row on its given action: k_discrete_head's arithmetic (sg_policy.hip) in mode 2 --
// row maximum subtracted, the log-prob of a class from the OTHER classes' mass, softplus and the Bernoulli entropy without their
// cancellations.  z: the row's n_out logits.  Returns the log-prob, *ent the entropy.
__device__ __forceinline__ float dg_discrete_row(const SgPolicyDesc& d, const float* z, const float* action_in, int row, float* ent) {
    const int K = d.n_out;
    float logp = 0.f, e = 0.f;
    if (d.dist == SG_DIST_CATEGORICAL) {
        float m = z[0];
        int am = 0;
        for (int k = 1; k < K; ++k)
            if (z[k] > m) { m = z[k]; am = k; }
        float S = 0.f;
        for (int k = 0; k < K; ++k)
            if (k != am) S += expf(z[k] - m);
        const float l1p = log1pf(S);
        int act = (int)action_in[row];
        act = act < 0 ? 0 : (act > K - 1 ? K - 1 : act);
        for (int k = 0; k < K; ++k) {
            const float lp = (z[k] - m) - l1p;
            e -= expf(lp) * lp;
        }
        logp = (z[act] - m) - l1p;
    } else {
        for (int k = 0; k < K; ++k) {
            const float zk = z[k], az = fabsf(zk);
            const float ex = expf(-az), l1p = log1pf(ex);
            const float act = action_in[(size_t)row * K + k];
            logp += act * zk - (fmaxf(zk, 0.f) + l1p);
            e += l1p + az * (ex / (1.f + ex));
        }
    }
    *ent = e;
    return logp;
}

// Workgroup w takes the 16*MT-row tile w of the rollout's first T slots (time-major rows t*N + n, read in place), in
// k_policy_act_step's pattern: rows staged in LDS, every trunk run on them (weights staged per trunk, or read from global memory:
// GW), then one lane of wave 0 per row evaluates the head on the rollout's action -- gauss_head_row in mode 2, or
// dg_discrete_row -- and forms, with d = logp_new - logp_old:
//   -d | (r - 1) - d | |r - 1| > clip | entropy | r = expf(d) | ret - v_new | ret - vpred | ret
// r - 1 is expm1f(d), not expf(d) - 1.f: the same number without the rounding of r to the grid around 1, which near the on-policy
// point would be all that is left of (r - 1) - d.  The tile's rows are reduced in double by wave butterflies (a tile is at most
// 64 rows: one wave), the three (count, mean, M2) triples in two passes -- mean first, then the squared deviations from it, so a
// mean far from zero costs nothing.  No atomics: the order is a function of (n, MT) alone.  The grid is not capped (one tile per
// workgroup, as k_policy_act_step; a loop over tiles with the weights restaged per tile costs the LDS instances 20 bytes of
// scratch), so the records and their merge order do not depend on the device's CU count either.
template <int MT, bool GW = false>
__global__ __launch_bounds__(256) void k_policy_diag(DiagArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 16 * MT;
    const SgPolicyDesc& d = a.d;
    const int tid = threadIdx.x, base = blockIdx.x * R;
    float* X = smem + a.wbuf_floats;
    float* H1 = X + R * d.ldO;
    float* H2 = H1 + R * d.ldH;
    float* OUT = H2 + R * d.ldH;                       // [n_trunks][R][ldPmax]
    stage_rows(X, R, d.Op, d.ldO, a.x, d.O, [&](int r) { return base + r < a.n ? base + r : -1; });
    run_trunks<MT, GW>(d, a.params, false, smem, X, H1, H2, OUT, a.ldPmax);
    if (tid >= 64) return;   // wave 0
    const int row = base + tid;
    const bool live = tid < R && row < a.n;
    double nd = 0.0, k3 = 0.0, flag = 0.0, ent = 0.0, ratio = 1.0, ret = 0.0, eo = 0.0, en = 0.0;
    if (live) {
        const float* h0 = OUT + tid * d.trunk[0].ldP;
        const float* h1 = OUT + R * a.ldPmax + tid * d.trunk[1].ldP;
        const float* hc = OUT + (d.n_trunks - 1) * R * a.ldPmax + tid * d.trunk[d.n_trunks - 1].ldP;
        float e, logp;
        if (d.dist == SG_DIST_GAUSSIAN)
            logp = gauss_head_row<true>(d, a.params, h0, h1, row, 2, nullptr, a.action, 0, 0, [](int, float) {}, &e);
        else logp = dg_discrete_row(d, h0, a.action, row, &e);
        const float dl = logp - a.logp_old[row];
        const float rm1 = expm1f(dl);
        nd = -(double)dl;
        k3 = (double)rm1 - (double)dl;
        flag = fabsf(rm1) > a.clip ? 1.0 : 0.0;
        ent = (double)e;
        ratio = (double)expf(dl);
        ret = (double)a.ret[row];
        eo = ret - (double)a.vpred[row];
        en = ret - (double)hc[0];
    }
    const double c = dg_wave_sum(live ? 1.0 : 0.0);   // >= 1: every tile of the grid holds a row
    const double s_nd = dg_wave_sum(nd), s_k3 = dg_wave_sum(k3), s_flag = dg_wave_sum(flag), s_ent = dg_wave_sum(ent);
    const double s_sq = dg_wave_sum(en * en);
    const double rmin = dg_wave_min(live ? ratio : (double)INFINITY), rmax = dg_wave_max(live ? ratio : -(double)INFINITY);
    const double m_ret = dg_wave_sum(ret) / c, m_eo = dg_wave_sum(eo) / c, m_en = dg_wave_sum(en) / c;
    const double d_ret = live ? ret - m_ret : 0.0, d_eo = live ? eo - m_eo : 0.0, d_en = live ? en - m_en : 0.0;
    const double q_ret = dg_wave_sum(d_ret * d_ret), q_eo = dg_wave_sum(d_eo * d_eo), q_en = dg_wave_sum(d_en * d_en);
    if (tid == 0) {
        double* o = a.rec + (size_t)blockIdx.x * DG_REC;
        o[DG_CNT] = c; o[DG_NEGD] = s_nd; o[DG_K3] = s_k3; o[DG_FLAG] = s_flag; o[DG_ENT] = s_ent;
        o[DG_RMIN] = rmin; o[DG_RMAX] = rmax; o[DG_SQ] = s_sq;
        o[DG_RET_MEAN] = m_ret; o[DG_RET_M2] = q_ret; o[DG_EO_MEAN] = m_eo; o[DG_EO_M2] = q_eo;
        o[DG_EN_MEAN] = m_en; o[DG_EN_M2] = q_en; o[14] = 0.0; o[15] = 0.0;
    }
}

// rec (b) folded into acc (a): plain sums added, minimum / maximum taken, triples merged by Chan's formula.
__device__ __forceinline__ void dg_merge(double* a, const double* b) {
    const double na = a[DG_CNT], nb = b[DG_CNT];
    if (nb == 0.0) return;
    a[DG_NEGD] += b[DG_NEGD]; a[DG_K3] += b[DG_K3]; a[DG_FLAG] += b[DG_FLAG]; a[DG_ENT] += b[DG_ENT]; a[DG_SQ] += b[DG_SQ];
    a[DG_RMIN] = fmin(a[DG_RMIN], b[DG_RMIN]);
    a[DG_RMAX] = fmax(a[DG_RMAX], b[DG_RMAX]);
    dg_chan(na, &a[DG_RET_MEAN], &a[DG_RET_M2], nb, b[DG_RET_MEAN], b[DG_RET_M2]);
    dg_chan(na, &a[DG_EO_MEAN], &a[DG_EO_M2], nb, b[DG_EO_MEAN], b[DG_EO_M2]);
    dg_chan(na, &a[DG_EN_MEAN], &a[DG_EN_M2], nb, b[DG_EN_MEAN], b[DG_EN_M2]);
    a[DG_CNT] = na + nb;
}

// One workgroup of one wave.  The nrec records are merged in ascending workgroup order, all in double, in two levels: lane i
// folds the contiguous run [i * per, (i + 1) * per) of them, in order, into its own record, then lane 0 folds the 64 lane
// records, in order.  The shape of that tree depends on nrec alone.  Folding a record into the empty accumulator leaves the
// record's bits (0 + x, min(inf, x), Chan's update at na = 0), so one record through this fold is that record.
//   DG_FINAL  the fold, then the ten results: out[SG_DIAG_N] (include/simgan_hip.h), and out[SG_DIAG_N] itself = 0
//   DG_FOLD   the fold alone: out[DG_REC] is the folded record (plain sums, minimum / maximum, the three triples)
//   DG_WORLD  DG_FINAL over the ranks' folded records in ascending rank order (nrec = world <= 64: one record per lane);
//             out[SG_DIAG_N] = 1 if the ranks' row counts differ -- the fetch then refuses the numbers
enum { DG_FINAL = 0, DG_FOLD, DG_WORLD };
template <int MODE>
__global__ __launch_bounds__(64) void k_policy_diag_reduce(const double* rec, int nrec, double* out) {
    __shared__ double part[64][DG_REC + 1];
    const int lane = threadIdx.x;
    const int per = (nrec + 63) / 64;
    double acc[DG_REC];
#pragma unroll
    for (int k = 0; k < DG_REC; ++k) acc[k] = 0.0;
    acc[DG_RMIN] = INFINITY;
    acc[DG_RMAX] = -INFINITY;
    for (int i = lane * per; i < nrec && i < (lane + 1) * per; ++i) {
        double b[DG_REC];
#pragma unroll
        for (int k = 0; k < DG_REC; ++k) b[k] = rec[(size_t)i * DG_REC + k];
        dg_merge(acc, b);
    }
#pragma unroll
    for (int k = 0; k < DG_REC; ++k) part[lane][k] = acc[k];
    __syncthreads();
    if (lane != 0) return;
    for (int j = 1; j < 64; ++j) {
        double b[DG_REC];
#pragma unroll
        for (int k = 0; k < DG_REC; ++k) b[k] = part[j][k];
        dg_merge(acc, b);
    }
    if (MODE == DG_FOLD) {
#pragma unroll
        for (int k = 0; k < DG_REC; ++k) out[k] = acc[k];
        return;
    }
    const double n = acc[DG_CNT];
    const double var_ret = acc[DG_RET_M2] / n;   // population variances; 0 / 0 is NaN, as numpy's 1 - var(e) / var(ret) is
    out[0] = n;
    out[1] = acc[DG_NEGD] / n;
    out[2] = acc[DG_K3] / n;
    out[3] = acc[DG_FLAG] / n;
    out[4] = acc[DG_ENT] / n;
    out[5] = acc[DG_RMIN];
    out[6] = acc[DG_RMAX];
    out[7] = 1.0 - (acc[DG_EO_M2] / n) / var_ret;
    out[8] = 1.0 - (acc[DG_EN_M2] / n) / var_ret;
    out[9] = acc[DG_SQ] / n;
    double differ = 0.0;
    if (MODE == DG_WORLD)
        for (int i = 1; i < nrec; ++i)
            if (rec[(size_t)i * DG_REC + DG_CNT] != rec[DG_CNT]) differ = 1.0;
    out[SG_DIAG_N] = differ;
}

// LDS of one workgroup: k_policy_act_step's layout (weights of one trunk | X | H1 | H2 | every trunk's head outputs)
static size_t diag_lds_bytes(const SgPolicyDesc& d, int MT, bool gw) {
    const int R = 16 * MT;
    return sizeof(float) * (size_t)((gw ? 0 : max_trunk_size(d, 0, d.n_trunks)) + R * d.ldO + 2 * R * d.ldH + d.n_trunks * R * max_ldP(d));
}

// Both scopes.  `who` names the entry point in the messages (the rank scope's are pinned by its tests).
static int policy_diagnostics(const char* who, bool world_scope, sg_rollout* r, sg_policy* p, float clip_param, const float* hxs0_host,
                              double* out10) {
    SG_REQUIRE(r && p, "%s: NULL argument", who);
    SG_REQUIRE(p->ctx == r->ctx, "%s: the policy and the rollout live on different contexts", who);
    SG_REQUIRE(!sg_policy_cnn_rnn(p), "%s: the policy has the recurrent CNN base (sg_policy_create_cnn_rnn); the diagnostics launch "
               "runs the MLP trunks only: evaluate the rollout through sg_policy_evaluate_rnn and reduce on the host", who);
    SG_REQUIRE(!p->cnn, "%s: the policy has the CNN base (image observations); the diagnostics launch runs "
               "the MLP trunks only: evaluate the rollout through sg_policy_evaluate and reduce on the host", who);
    const int O = p->recurrent ? p->gru.O : p->desc.O;
    SG_REQUIRE(O == r->O && p->desc.A == r->A, "%s: policy/rollout dims differ (obs %d vs %d, action %d vs %d)", who,
               O, r->O, p->desc.A, r->A);
    SG_REQUIRE(clip_param > 0.f, "%s: clip_param = %g: it must be positive (INFINITY is accepted and gives "
               "a clip fraction of 0)", who, (double)clip_param);
    if (p->recurrent && r->d_hidden)
        SG_REQUIRE(r->hidden_dim == p->gru.H, "%s: the rollout's hidden states are %d wide, the policy's %d", who,
                   r->hidden_dim, p->gru.H);
    SG_REQUIRE(!p->recurrent || r->d_hidden || hxs0_host, "%s: the policy is recurrent and the rollout holds "
               "no hidden states (sg_rollout_enable_hidden): hxs0_host, the N*H states of slot 0, is required", who);
    SG_REQUIRE((int64_t)r->T * r->N < (1ll << 30), "%s: T*N = %lld rows: fewer than 2^30 are taken", who,
               (long long)r->T * r->N);
    sg_ctx* ctx = r->ctx;
    const SgPolicyDesc& d = p->desc;
    const int n = r->T * r->N;
    const size_t room = (size_t)ctx->lds_bytes - 1024;
    // the weight path of the forward launch (sg_policy_needs_gw; SG_POLICY_GW=1 forces global weights) unless every trunk's
    // head outputs beside a 16-row tile leave no room for the weights
    const bool gw = sg_policy_needs_gw(ctx, d) || diag_lds_bytes(d, 1, false) > room;
    int MT = fwd_tile_mt(ctx, d, n, gw);
    while (MT > 1 && diag_lds_bytes(d, MT, gw) > room) MT /= 2;
    SG_REQUIRE(diag_lds_bytes(d, MT, gw) <= room, "%s: a 16-row tile of this policy with every trunk's head "
               "outputs (%zu B) does not fit the %d-byte LDS", who, diag_lds_bytes(d, MT, gw), ctx->lds_bytes);
    SG_CHECK(hipSetDevice(ctx->device));
    const int R = 16 * MT, gx = (n + R - 1) / R;
    if (!r->h_diag) {
        SG_CHECK(sg_host_malloc((void**)&r->h_diag, sizeof(double) * 16));
        SG_CHECK(hipEventCreateWithFlags(&r->diag_ev, hipEventDisableTiming));
    }
    // world scope: behind the workgroups' records, this rank's folded record and the world's gathered ones
    const bool gather = world_scope && ctx->comm;
    const int world = gather ? ctx->world : 1;
    SG_TRY(ensure_cap(ctx->stream, &r->d_diag, &r->diag_cap, (size_t)gx * DG_REC + (world_scope ? (size_t)(1 + world) * DG_REC : 0)));
    DiagArgs a;
    a.x = r->d_field[SG_F_OBS];
    if (p->recurrent) {
        // the states the heads read: the GRU forward over all N environments and T steps from the state of slot 0, as the PPO step
        // feeds its heads (h_{t-1} * masks[t] at every step, MASKS[:-1])
        const SgGruDesc& g = p->gru;
        auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
        const size_t f_h0 = r4((size_t)r->N * g.H), f_gi = r4((size_t)n * 3 * g.Hp), f_h = r4((size_t)n * g.H);
        SG_TRY(sg_policy_io_reserve(p, sizeof(float) * (f_h0 + f_gi + f_h)));
        float* d_h0 = p->d_io;
        float* d_gi = d_h0 + f_h0;
        float* d_hout = d_gi + f_gi;
        if (!r->d_hidden)
            SG_CHECK(hipMemcpyAsync(d_h0, hxs0_host, sizeof(float) * (size_t)r->N * g.H, hipMemcpyHostToDevice, ctx->stream));
        SG_TRY(sg_gru_forward_launch(ctx, g, p->d_params + g.off, r->d_field[SG_F_OBS], g.O, r->d_hidden ? r->d_hidden : d_h0,
                                     r->d_field[SG_F_MASKS], r->T, r->N, d_gi, d_hout, g.H, nullptr, nullptr));
        a.x = d_hout;
    }
    a.d = d; a.params = p->d_params;
    a.action = r->d_field[SG_F_ACTIONS]; a.logp_old = r->d_field[SG_F_LOGP];
    a.vpred = r->d_field[SG_F_VALUE_PREDS]; a.ret = r->d_field[SG_F_RETURNS];
    a.n = n; a.clip = clip_param; a.rec = r->d_diag;
    a.wbuf_floats = gw ? 0 : max_trunk_size(d, 0, d.n_trunks); a.ldPmax = max_ldP(d);
    const size_t lds = diag_lds_bytes(d, MT, gw);
    sg_dispatch_mt_gw<4>(MT, gw, [&](auto mt, auto g) {
        hipLaunchKernelGGL((k_policy_diag<decltype(mt)::value, decltype(g)::value>), dim3(gx), dim3(256), lds, ctx->stream, a);
    });
    SG_CHECK(hipGetLastError());
    if (!world_scope) {
        hipLaunchKernelGGL(k_policy_diag_reduce<DG_FINAL>, dim3(1), dim3(64), 0, ctx->stream, r->d_diag, gx, r->h_diag);
    } else {
        double* mine = r->d_diag + (size_t)gx * DG_REC;
        double* all = mine + DG_REC;
        hipLaunchKernelGGL(k_policy_diag_reduce<DG_FOLD>, dim3(1), dim3(64), 0, ctx->stream, r->d_diag, gx, mine);
        SG_CHECK(hipGetLastError());
        if (gather) SG_TRY(sg_comm_allgather_f64(ctx, mine, all, DG_REC));
        hipLaunchKernelGGL(k_policy_diag_reduce<DG_WORLD>, dim3(1), dim3(64), 0, ctx->stream, gather ? all : mine, world, r->h_diag);
    }
    SG_CHECK(hipGetLastError());
    SG_CHECK(hipEventRecord(r->diag_ev, ctx->stream));
    r->diag_pending = true;
    if (out10) return sg_rollout_policy_diagnostics_fetch(r, out10);
    return 0;
}

extern "C" int sg_rollout_policy_diagnostics(sg_rollout* r, sg_policy* p, float clip_param, const float* hxs0_host, double* out10) {
    return policy_diagnostics("sg_rollout_policy_diagnostics", false, r, p, clip_param, hxs0_host, out10);
}

// The world scope: k_policy_diag, the fold alone, the all-gather of the ranks' 16-double records, fold + finalise over them.
// A COLLECTIVE: every rank issues it at the same point of its stream's sequence of collectives.  No communicator: the rank
// scope's bits (the folded record through the second fold is itself).
extern "C" int sg_rollout_policy_diagnostics_world(sg_rollout* r, sg_policy* p, float clip_param, const float* hxs0_host, double* out10) {
    return policy_diagnostics("sg_rollout_policy_diagnostics_world", true, r, p, clip_param, hxs0_host, out10);
}

extern "C" int sg_rollout_policy_diagnostics_fetch(sg_rollout* r, double out10[10]) {
    SG_REQUIRE(r && out10, "sg_rollout_policy_diagnostics_fetch: NULL argument");
    SG_REQUIRE(r->diag_pending, "sg_rollout_policy_diagnostics_fetch: no diagnostics are pending on this rollout (queue them with "
               "sg_rollout_policy_diagnostics(..., out10 = NULL) first; a result is fetched once)");
    SG_CHECK(hipEventSynchronize(r->diag_ev));
    r->diag_pending = false;
    SG_REQUIRE(r->h_diag[SG_DIAG_N] == 0.0, "sg_rollout_policy_diagnostics_fetch: the ranks of the world scope hold different numbers of "
               "rows (this rank: T*N = %lld): the global numbering takes equal column shards, no numbers are returned",
               (long long)r->T * r->N);
    memcpy(out10, r->h_diag, sizeof(double) * SG_DIAG_N);
    return 0;
}
