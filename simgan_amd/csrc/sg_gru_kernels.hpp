// sg_gru_kernels.hpp -- the GRU base of a recurrent Policy (a2c/model.py:117-201) as gfx950 kernels: input projection, the
// scan over time (forward and reverse), the weight gradients after the scan.  Used by sg_gru.hip (act / get_value /
// evaluate_actions; it also holds the forward launcher that sg_ppo.hip calls) and sg_ppo.hip (PPO through time: the reverse
// scan, the weight gradients, the gather).  Every kernel is a template: a translation unit carries only what it launches.
//
//   k_gru_inproj       GI = X W_ih^T + b_ih for ALL T*n rows: row-parallel, off the sequential chain
//   k_gru_scan_fwd     t = 0..T-1: h_t = cell(GI[t], h_{t-1} * masks[t]); one workgroup carries 16 environments through
//                      all T steps with W_hh resident in LDS (GW: through L2).  TRAIN: saves r, z, n, W_hn h + b_hn and
//                      the masked previous state for the reverse scan and writes h_t as the heads' padded input rows
//   k_gru_scan_bwd     t = T-1..0: dh_t = dL/dx_t (both trunks) + carried; gate gradients; writes the pre-activation gate
//                      gradients [dr, dz, dn] (input side) and [dr, dz, dn r] (hidden side); carried = (dh z + dGH W_hh) masks[t]
//   k_gru_wgrad        dW_ih = dGI^T X, dW_hh = dGH^T Hm, db = column sums: GEMMs over all T*per rows AFTER the scan, split
//                      over row ranges into partial blocks;  k_gru_reduce adds the partials in a fixed order
//   k_a2c_gru_gather   A2C through time: a group of environments in the rollout's own order, time-major;  k_gru_reduce_acc adds the
//                      groups' GRU gradients in group order and finishes them after the last
//   k_gru_dx           the recurrent CNN base (sg_cnn.hip, sg_ppo.hip: cnn_gru_ppo_update): dZf = (dGI W_ih) [F > 0], the gradient the
//                      CNN trunk's backward continues from;  k_cnn_gru_index, k_gru_pad_rows: its step's index vector and padded x
//                      (k_cnn_gru_index_group: the index of one environment group of a2c_cnn_gru_update, no permutation)
// No floating-point atomics anywhere: every sum has one order, two runs give the same bits.
#pragma once
#include "sg_common.h"

// logistic function on the fast exp / rcp units (v_exp_f32, v_rcp_f32: 1 ulp each); exp(-x) = inf gives 0, as it should
__device__ __forceinline__ float sg_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.f + __expf(-x));
}

// ----------------------------------------------------------------------------- input projection
struct GruProjArgs {
    SgGruDesc g;
    const float* W;      // the GRU block (padded image) in global memory
    const float* x;      // [rows][x_ld] (x_ld == O: compact rows; x_ld == ldO: padded rows)
    int x_ld;
    int rows;
    float* gi;           // [rows][3*Hp]: gate k of hidden unit c at column k*Hp + c, b_ih added
    int wbuf_floats;     // LDS floats of the W_ih image (0: GW)
};

template <int MT, bool GW>
__global__ __launch_bounds__(256) void k_gru_inproj(GruProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 16 * MT;
    const SgGruDesc& g = a.g;
    const float* W = GW ? a.W + g.wih : smem;
    float* X = smem + a.wbuf_floats;
    const float* bih = a.W + g.bih;
    const int G3 = 3 * g.Hp;
    if (!GW) sg_stage(smem, a.W + g.wih, (3 * g.Hp * g.ldO) / 4);
    for (int base = blockIdx.x * R; base < a.rows; base += gridDim.x * R) {
        __syncthreads();
        for (int i = threadIdx.x; i < R * g.Op; i += blockDim.x) {
            const int r = i / g.Op, c = i - r * g.Op;
            const int row = base + r;
            X[r * g.ldO + c] = (row < a.rows && c < g.O) ? a.x[(size_t)row * a.x_ld + c] : 0.f;
        }
        __syncthreads();
        // unit-distributed: every 16x16 output tile is one <1, 1> MFMA chain whatever MT is, so a row's GI -- and with it the
        // whole state trajectory -- has the same bits in a one-step call and inside a sequence
        sg_layer_nt_u<MT, GW>(X, g.ldO, W, g.ldO, g.Op, G3, [&](int r, int c, float v) {
            if (base + r < a.rows) a.gi[(size_t)(base + r) * G3 + c] = v + bih[c];
        });
    }
}

// ------------------------------------------------------------------------------------- the scan
struct GruScanArgs {
    SgGruDesc g;
    const float* W;       // the GRU block (padded image) in global memory
    const float* gi;      // [T*n][3*Hp]
    const float* h0;      // [n, H]
    const float* masks;   // [T*n]
    int T, n;
    float* hout;          // [T*n][hout_ld]  h_t, row t*n + env (the heads' input)
    int hout_ld;
    float* hlast;         // [n, H]    h_{T-1}, or NULL
    // TRAIN: what the reverse scan needs, [T*n][Hp] each (hm: [T*n][ldH])
    float *sr, *sz, *sn, *shn, *hm;
};

// One workgroup = 16 environments (one MFMA row tile) x all T steps.  Per step every wave owns whole column tiles of the
// hidden state: for its 16 hidden units it forms the r, z and n pre-activations W_h{r,z,n} h as three 16x16 MFMA tiles whose
// accumulators line up lane for lane, so the gate arithmetic runs in registers and h_t goes straight into the other of two
// LDS state tiles (already multiplied by masks[t + 1] for the next step): ONE barrier per step, no gate tile in LDS.
// GI[t] is fetched before the MFMAs of the step, so its latency hides behind them.
template <bool GW, bool TRAIN = false>
__global__ __launch_bounds__(256) void k_gru_scan_fwd(GruScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SgGruDesc& g = a.g;
    const int Hp = g.Hp, ldH = g.ldH, H = g.H, G3 = 3 * g.Hp;
    const int wfl = GW ? 0 : 3 * Hp * ldH;
    const float* W = GW ? a.W + g.whh : smem;
    float* Hb0 = smem + wfl;
    float* Hb1 = Hb0 + 16 * ldH;
    const float* bhh = a.W + g.bhh;
    const int base = blockIdx.x * 16;
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
    if (!GW) sg_stage(smem, a.W + g.whh, (3 * Hp * ldH) / 4);
    for (int i = threadIdx.x; i < 16 * ldH; i += blockDim.x) {
        const int r = i / ldH, c = i - r * ldH;
        const int row = base + r;
        Hb0[i] = (row < a.n && c < H) ? a.h0[(size_t)row * H + c] * a.masks[row] : 0.f;
        Hb1[i] = 0.f;
    }
    __syncthreads();
    for (int t = 0; t < a.T; ++t) {
        const float* cur = (t & 1) ? Hb1 : Hb0;
        float* nxt = (t & 1) ? Hb0 : Hb1;
        for (int tn = wave; tn * 16 < Hp; tn += nw) {
            const int c = tn * 16 + li;
            float gir[4], giz[4], gin[4], mnext[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = base + 4 * lq + r;
                const bool live = row < a.n;
                const float* gp = a.gi + ((size_t)t * a.n + (live ? row : 0)) * G3 + c;
                gir[r] = live ? gp[0] : 0.f;
                giz[r] = live ? gp[Hp] : 0.f;
                gin[r] = live ? gp[2 * Hp] : 0.f;
                mnext[r] = (live && t + 1 < a.T) ? a.masks[(size_t)(t + 1) * a.n + row] : 1.f;
            }
            const float br = bhh[c], bz = bhh[Hp + c], bn = bhh[2 * Hp + c];
            f32x4 ar[1][1], az[1][1], an[1][1];
            sg_acc_zero(ar); sg_acc_zero(az); sg_acc_zero(an);
            if (GW) {
                sg_mma_nt_g<1, 1>(cur, ldH, W + (size_t)(tn * 16) * ldH, ldH, Hp, ar);
                sg_mma_nt_g<1, 1>(cur, ldH, W + (size_t)(Hp + tn * 16) * ldH, ldH, Hp, az);
                sg_mma_nt_g<1, 1>(cur, ldH, W + (size_t)(2 * Hp + tn * 16) * ldH, ldH, Hp, an);
            } else {
                sg_mma_nt<1, 1>(cur, ldH, W + (tn * 16) * ldH, ldH, Hp, ar);
                sg_mma_nt<1, 1>(cur, ldH, W + (Hp + tn * 16) * ldH, ldH, Hp, az);
                sg_mma_nt<1, 1>(cur, ldH, W + (2 * Hp + tn * 16) * ldH, ldH, Hp, an);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = 4 * lq + r, row = base + lr;
                const float hm = cur[lr * ldH + c];
                const float hn = an[0][0][r] + bn;
                const float rg = sg_sigmoid(gir[r] + (ar[0][0][r] + br));
                const float zg = sg_sigmoid(giz[r] + (az[0][0][r] + bz));
                const float ng = sg_tanh(gin[r] + rg * hn);
                const float h = (1.f - zg) * ng + zg * hm;
                const bool real = row < a.n && c < H;
                nxt[lr * ldH + c] = real ? h * mnext[r] : 0.f;
                if (real) {
                    a.hout[((size_t)t * a.n + row) * a.hout_ld + c] = h;
                    if (a.hlast && t + 1 == a.T) a.hlast[(size_t)row * H + c] = h;
                }
                if (TRAIN && row < a.n) {
                    const size_t q = ((size_t)t * a.n + row) * Hp + c;
                    a.sr[q] = rg; a.sz[q] = zg; a.sn[q] = ng; a.shn[q] = hn;
                    a.hm[((size_t)t * a.n + row) * ldH + c] = hm;
                }
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------- the reverse scan
struct GruBwdArgs {
    SgGruDesc g;
    const float* W;                 // the GRU block
    const float *dxa, *dxc;         // [T*n..][dx_ld]: dL/dx_t from the actor and the critic trunk (added in this order)
    int dx_ld;
    const float *sr, *sz, *sn, *shn, *hm;
    const float* masks;             // [T*n]
    int T, n;
    float *dgi, *dgh;               // [T*n][3*Hp]
};

// One workgroup = the same 16 environments, t = T-1 .. 0, two phases per step:
//   A (element-wise, a thread per (row, unit)): dh = dL/dx_t + carried; gate gradients; the hidden-side tile [dr, dz, dn r] goes
//     to LDS and to global memory, the input-side one [dr, dz, dn] to global memory; dh z stays in the carried tile
//   B (MFMA): carried = (dh z + [dr, dz, dn r] W_hh) * masks[t]   -- the only matrix product on the chain (16 x 3Hp x Hp)
// No gradient is formed for h_0 or the observations.
template <bool GW>
__global__ __launch_bounds__(256) void k_gru_scan_bwd(GruBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SgGruDesc& g = a.g;
    const int Hp = g.Hp, ldH = g.ldH, G3 = 3 * g.Hp, ld3 = G3 + 4;
    const int wfl = GW ? 0 : 3 * Hp * ldH;
    const float* W = GW ? a.W + g.whh : smem;
    float* DH = smem + wfl;          // [16][ldH]
    float* DG = DH + 16 * ldH;       // [16][ld3]
    const int base = blockIdx.x * 16;
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (!GW) sg_stage(smem, a.W + g.whh, (3 * Hp * ldH) / 4);
    for (int i = threadIdx.x; i < 16 * ldH; i += blockDim.x) DH[i] = 0.f;
    for (int i = threadIdx.x; i < 16 * ld3; i += blockDim.x) DG[i] = 0.f;
    __syncthreads();
    for (int t = a.T - 1; t >= 0; --t) {
        for (int i = threadIdx.x; i < 16 * Hp; i += blockDim.x) {
            const int r = i / Hp, c = i - r * Hp;
            const int row = base + r;
            float d_r = 0.f, d_z = 0.f, d_n = 0.f, d_nr = 0.f, keep = 0.f;
            if (row < a.n) {
                const size_t idx = (size_t)t * a.n + row;
                const float dh = (a.dxa[idx * a.dx_ld + c] + a.dxc[idx * a.dx_ld + c]) + DH[r * ldH + c];
                const size_t q = idx * Hp + c;
                const float rg = a.sr[q], zg = a.sz[q], ng = a.sn[q], hn = a.shn[q], hm = a.hm[idx * ldH + c];
                d_n = dh * (1.f - zg) * (1.f - ng * ng);
                d_z = dh * (hm - ng) * zg * (1.f - zg);
                d_r = d_n * hn * rg * (1.f - rg);
                d_nr = d_n * rg;
                keep = dh * zg;
                float* gi = a.dgi + idx * G3 + c;
                float* gh = a.dgh + idx * G3 + c;
                gi[0] = d_r; gi[Hp] = d_z; gi[2 * Hp] = d_n;
                gh[0] = d_r; gh[Hp] = d_z; gh[2 * Hp] = d_nr;
            }
            DG[r * ld3 + c] = d_r; DG[r * ld3 + Hp + c] = d_z; DG[r * ld3 + 2 * Hp + c] = d_nr;
            DH[r * ldH + c] = keep;
        }
        __syncthreads();
        for (int tn = wave; tn * 16 < Hp; tn += nw) {
            f32x4 acc[1][1];
            sg_acc_zero(acc);
            sg_mma_nn<1, 1>(DG, ld3, W + tn * 16, ldH, G3, acc);
            sg_tile_foreach(acc[0][0], 0, tn * 16, [&](int r, int c, float v) {
                const int row = base + r;
                const float m = row < a.n ? a.masks[(size_t)t * a.n + row] : 0.f;
                DH[r * ldH + c] = (DH[r * ldH + c] + v) * m;
            });
        }
        __syncthreads();
    }
}

// --------------------------------------------------------------------------- weight gradients
struct GruWgradArgs {
    SgGruDesc g;
    const float *dgi, *dgh;   // [rows_p][3*Hp], rows past the minibatch are zero
    const float* x;           // [rows_p..][ldO] padded observations of the minibatch (finite past its end)
    const float* hm;          // [rows_p][ldH]
    int rows_p;               // multiple of 16
    int KS;                   // row ranges
    float* partial;           // [KS][g.total]
};

// One wave per (output tile, row range).  Tiles: dW_ih (3Hp/16 x Op/16), dW_hh (3Hp/16 x Hp/16), then the two bias vectors
// (3Hp/16 column tiles each).  Operands are read from global memory in the TN fragment order (16 consecutive floats per row).
template <int DUMMY = 0>
__global__ __launch_bounds__(64) void k_gru_wgrad(GruWgradArgs a) {
    const SgGruDesc& g = a.g;
    const int tm_n = 3 * g.Hp / 16, to_n = g.Op / 16, th_n = g.Hp / 16;
    const int n_ih = tm_n * to_n, n_hh = tm_n * th_n;
    const int tile = blockIdx.x, ks = blockIdx.y;
    const int chunks = a.rows_p / 16, per = (chunks + a.KS - 1) / a.KS;
    const int c0 = ks * per, c1 = min(chunks, c0 + per);
    const int G3 = 3 * g.Hp;
    float* out = a.partial + (size_t)ks * g.total;
    const int lane = threadIdx.x & 63, li = lane & 15, lq = lane >> 4;
    if (tile < n_ih + n_hh) {
        const bool ih = tile < n_ih;
        const int tt = ih ? tile : tile - n_ih, cols = ih ? to_n : th_n;
        const int tm = tt / cols, tn = tt - tm * cols;
        const float* A = (ih ? a.dgi : a.dgh) + (size_t)c0 * 16 * G3 + tm * 16;
        const int ldb = ih ? g.ldO : g.ldH;
        const float* B = (ih ? a.x : a.hm) + (size_t)c0 * 16 * ldb + tn * 16;
        f32x4 acc[1][1];
        sg_acc_zero(acc);
        if (c1 > c0) sg_mma_tn<1, 1>(A, G3, B, ldb, (c1 - c0) * 16, acc);
        float* o = out + (ih ? g.wih : g.whh);
        sg_tile_foreach(acc[0][0], tm * 16, tn * 16, [&](int r, int c, float v) { o[(size_t)r * ldb + c] = v; });
    } else {
        const int tb = tile - n_ih - n_hh;
        const bool ih = tb < tm_n;
        const int tc = ih ? tb : tb - tm_n;
        const float* A = (ih ? a.dgi : a.dgh) + tc * 16 + li;
        float s = 0.f;
        for (int row = c0 * 16 + lq; row < c1 * 16; row += 4) s += A[(size_t)row * G3];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (lq == 0) out[(ih ? g.bih : g.bhh) + tc * 16 + li] = s;
    }
}

// grad[total + i] = sum over the KS partials (fixed order) for the gtotal GRU entries; the three loss sums k_ppo_reduce left at
// grad[total ..] move behind them (k_ppo_adam reads them past the last parameter); part[part_off + block] = the block's sum of
// squares, so that the clip's norm covers all parameters
template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_gru_reduce(const float* partial, int KS, int gtotal, float* grad, int total, float* part,
                                                    int part_off) {
    __shared__ float ws[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float tail = 0.f;
    if (blockIdx.x == 0 && threadIdx.x < 8) tail = grad[total + threadIdx.x];
    float s = 0.f;
    if (i < gtotal)
        for (int k = 0; k < KS; ++k) s += partial[(size_t)k * gtotal + i];
    __syncthreads();
    if (i < gtotal) grad[total + i] = s;
    float sq = sg_wave_sum(s * s);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) part[part_off + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    if (blockIdx.x == 0 && threadIdx.x < 8) grad[total + gtotal + threadIdx.x] = tail;
}

// The accumulate variant (A2C through time: the environments go through the scans in groups).  Group k's partial sums are added
// to gacc, the sums of the groups before it (acc == 0: the first group starts them), in group order -- one order, the same bits
// every run.  Only the last group (last != 0) touches grad and part: the finished GRU gradient goes behind the heads', the loss
// sums move behind it and the blocks' sums of squares are taken over the finished gradient, as k_gru_reduce does for its one group.
template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_gru_reduce_acc(const float* partial, int KS, int gtotal, float* gacc, int acc, int last,
                                                        float* grad, int total, float* part, int part_off) {
    __shared__ float ws[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    float s = 0.f;
    if (i < gtotal) {
        if (acc) s = gacc[i];
        for (int k = 0; k < KS; ++k) s += partial[(size_t)k * gtotal + i];
    }
    if (!last) {
        if (i < gtotal) gacc[i] = s;
        return;
    }
    float tail = 0.f;
    if (blockIdx.x == 0 && threadIdx.x < 8) tail = grad[total + threadIdx.x];
    __syncthreads();
    if (i < gtotal) grad[total + i] = s;
    float sq = sg_wave_sum(s * s);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = sq;
    __syncthreads();
    if (threadIdx.x == 0) part[part_off + blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
    if (blockIdx.x == 0 && threadIdx.x < 8) grad[total + gtotal + threadIdx.x] = tail;
}

// ------------------------------------------------------------- group gather of A2C through time (a2c/algo/a2c_acktr.py:56-63)
// Group row rr = t * n + j  <-  rollout row t * N + e0 + j: the group's n environments in the rollout's own order, time-major.
// Padded observations, actions, the return (the one per-row scalar A2C reads), masks[:-1], and the hidden state of slot 0.
struct A2cGruGatherArgs {
    const float *obs, *actions, *ret, *masks, *h0;
    int T, N, e0, n, O, ldO, A, H, sc_stride;
    float *X, *ACT, *SC, *MK, *H0;
};

template <int DUMMY = 0>
__global__ __launch_bounds__(64) void k_a2c_gru_gather(A2cGruGatherArgs a) {
    const int rr = blockIdx.x;   // one workgroup per group row
    const int t = rr / a.n, j = rr - t * a.n;
    const size_t src = (size_t)t * a.N + a.e0 + j;
    for (int c = threadIdx.x; c < a.ldO; c += blockDim.x) a.X[(size_t)rr * a.ldO + c] = c < a.O ? a.obs[src * a.O + c] : 0.f;
    for (int c = threadIdx.x; c < a.A; c += blockDim.x) a.ACT[(size_t)rr * a.A + c] = a.actions[src * a.A + c];
    if (threadIdx.x == 0) {
        a.SC[3 * (size_t)a.sc_stride + rr] = a.ret[src];
        a.MK[rr] = a.masks[src];
    }
    if (t == 0)
        for (int c = threadIdx.x; c < a.H; c += blockDim.x) a.H0[(size_t)j * a.H + c] = a.h0[(size_t)(a.e0 + j) * a.H + c];
}

// ------------------------------------------------------------------------- epoch gather (a2c/storage.py:194-251)
// Epoch row rr = (k * T + t) * per + j  <-  rollout row t * N + perm[k * per + j]: minibatch k holds per whole environments,
// time-major.  Padded observations, actions, the four per-row scalars, masks, and the hidden state of slot 0 per environment.
struct GruGatherArgs {
    const float *obs, *actions, *old_logp, *adv, *vpred, *ret, *masks, *h0;
    const int64_t* perm;   // [N]
    int T, N, per, O, ldO, A, H, sc_stride;
    float *X, *ACT, *SC, *MK, *H0;
};

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_gru_epoch_gather(GruGatherArgs a) {
    const int rr = blockIdx.x;   // one workgroup per epoch row
    const int mb = a.T * a.per;
    const int k = rr / mb, rem = rr - k * mb, t = rem / a.per, j = rem - t * a.per;
    const int env = (int)a.perm[k * a.per + j];
    const size_t src = (size_t)t * a.N + env;
    for (int c = threadIdx.x; c < a.ldO; c += blockDim.x) a.X[(size_t)rr * a.ldO + c] = c < a.O ? a.obs[src * a.O + c] : 0.f;
    for (int c = threadIdx.x; c < a.A; c += blockDim.x) a.ACT[(size_t)rr * a.A + c] = a.actions[src * a.A + c];
    if (threadIdx.x == 0) {
        a.SC[0 * (size_t)a.sc_stride + rr] = a.old_logp[src];
        a.SC[1 * (size_t)a.sc_stride + rr] = a.adv[src];
        a.SC[2 * (size_t)a.sc_stride + rr] = a.vpred[src];
        a.SC[3 * (size_t)a.sc_stride + rr] = a.ret[src];
        a.MK[rr] = a.masks[src];
    }
    if (t == 0)
        for (int c = threadIdx.x; c < a.H; c += blockDim.x) a.H0[(size_t)(k * a.per + j) * a.H + c] = a.h0[(size_t)env * a.H + c];
}

// --------------------------------------------------------- the recurrent CNN base (a2c/model.py:204-230 with recurrent=True)
// The GRU reads the FC layer's features F = relu(Zf), so the gradient that the CNN trunk's backward continues from is
//   dZf[row][k] = (sum_{j < 3 Hp} dGI[row][j] W_ih[j][k]) * [F[row][k] > 0]      (ReLU's derivative at exactly 0 is 0, as in torch)
// Row-parallel over the step's rows, a persistent grid: a workgroup stages W_ih once (GW: reads it through L2) and walks 16-row
// tiles; per tile the dGI rows go to LDS and every wave forms whole 16x16 output tiles as one MFMA chain over K = 3 Hp in
// ascending k -- one order whatever the grid is, no atomics.
struct GruDxArgs {
    SgGruDesc g;
    const float* W;      // the GRU block
    const float* dgi;    // [rows..][3*Hp]
    const float* f;      // [rows][f_ld]: the features the GRU read (post-ReLU)
    int f_ld;
    int rows;
    float* dzf;          // [rows][dz_ld], columns < g.O written
    int dz_ld;
    int wbuf_floats;     // LDS floats of the W_ih image (0: GW)
};

template <bool GW>
__global__ __launch_bounds__(256) void k_gru_dx(GruDxArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SgGruDesc& g = a.g;
    const int G3 = 3 * g.Hp, ld3 = G3 + 4;
    const float* W = GW ? a.W + g.wih : smem;
    float* DG = smem + a.wbuf_floats;    // [16][ld3]
    if (!GW) sg_stage(smem, a.W + g.wih, (3 * g.Hp * g.ldO) / 4);
    for (int base = blockIdx.x * 16; base < a.rows; base += gridDim.x * 16) {
        __syncthreads();
        for (int i = threadIdx.x; i < 16 * (G3 / 4); i += blockDim.x) {
            const int r = i / (G3 / 4), c4 = i - r * (G3 / 4);
            const int row = base + r;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < a.rows) v = *reinterpret_cast<const float4*>(a.dgi + (size_t)row * G3 + 4 * c4);
            *reinterpret_cast<float4*>(DG + r * ld3 + 4 * c4) = v;
        }
        __syncthreads();
        sg_layer_nn_u<1>(DG, ld3, W, g.ldO, G3, g.Op, [&](int r, int c, float v) {
            const int row = base + r;
            if (row < a.rows && c < g.O) a.dzf[(size_t)row * a.dz_ld + c] = a.f[(size_t)row * a.f_ld + c] > 0.f ? v : 0.f;
        });
    }
}

// One optimizer step's rows of PPO through time on the image rollout (a2c/storage.py:194-251): step row rr = t * per + j is
// rollout row t * N + perm[j].  The index vector (the 28 K-float frames and the per-row scalars are read in place through
// it), the masks time-major, and the hidden state of slot 0 per environment.
struct CnnGruIndexArgs {
    const int64_t* perm;   // [per] environments of this step
    const float *masks, *h0;
    int T, N, per, H;
    int64_t* idx;          // [T*per]
    float *MK, *H0;        // [T*per], [per][H]
};

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_cnn_gru_index(CnnGruIndexArgs a) {
    const int rr = blockIdx.x * blockDim.x + threadIdx.x;
    if (rr < a.T * a.per) {
        const int t = rr / a.per, j = rr - t * a.per;
        const int64_t src = (int64_t)t * a.N + a.perm[j];
        a.idx[rr] = src;
        a.MK[rr] = a.masks[src];
    }
    for (int i = rr; i < a.per * a.H; i += gridDim.x * blockDim.x) {
        const int j = i / a.H, c = i - j * a.H;
        a.H0[i] = a.h0[(size_t)a.perm[j] * a.H + c];
    }
}

// The identity-offset form (A2C through time on the image rollout, a2c/algo/a2c_acktr.py:56-63): a group of n environments
// e0 .. e0 + n - 1 in the rollout's own order, group row rr = t * n + j is rollout row t * N + e0 + j; H0 rows are h0's e0 ..
struct CnnGruGroupIndexArgs {
    const float *masks, *h0;
    int T, N, e0, n, H;
    int64_t* idx;          // [T*n]
    float *MK, *H0;        // [T*n], [n][H]
};

template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_cnn_gru_index_group(CnnGruGroupIndexArgs a) {
    const int rr = blockIdx.x * blockDim.x + threadIdx.x;
    if (rr < a.T * a.n) {
        const int t = rr / a.n, j = rr - t * a.n;
        const int64_t src = (int64_t)t * a.N + a.e0 + j;
        a.idx[rr] = src;
        a.MK[rr] = a.masks[src];
    }
    for (int i = rr; i < a.n * a.H; i += gridDim.x * blockDim.x) a.H0[i] = a.h0[(size_t)a.e0 * a.H + i];
}

// compact rows [rows][w] -> padded rows [rows][ld] (zero in columns w .. ld-1): the features as k_gru_wgrad's x operand
template <int DUMMY = 0>
__global__ __launch_bounds__(256) void k_gru_pad_rows(const float* src, int rows, int w, float* dst, int ld) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)rows * ld) return;
    const int r = (int)(i / ld), c = (int)(i - (int64_t)r * ld);
    dst[i] = c < w ? src[(size_t)r * w + c] : 0.f;
}

static inline size_t sg_gru_dx_lds(const SgGruDesc& g, bool gw) {
    return sizeof(float) * (size_t)((gw ? 0 : 3 * g.Hp * g.ldO) + 16 * (3 * g.Hp + 4));
}
static inline size_t sg_gru_proj_lds(const SgGruDesc& g, int MT, bool gw) {
    return sizeof(float) * (size_t)((gw ? 0 : 3 * g.Hp * g.ldO) + 16 * MT * g.ldO);
}
static inline size_t sg_gru_scan_lds(const SgGruDesc& g, bool gw) {
    return sizeof(float) * (size_t)((gw ? 0 : 3 * g.Hp * g.ldH) + 2 * 16 * g.ldH);
}
static inline size_t sg_gru_bwd_lds(const SgGruDesc& g, bool gw) {
    return sizeof(float) * (size_t)((gw ? 0 : 3 * g.Hp * g.ldH) + 16 * g.ldH + 16 * (3 * g.Hp + 4));
}
static inline bool sg_gru_force_gw() {
    const char* e = getenv("SG_POLICY_GW");
    return e && e[0] == '1';
}

// sg_gru.hip: GI for `rows` = T*n rows of d_x, then the scan over [T][n]; train != NULL: the TRAIN instance with its save buffers
// set in *train.  The forward kernels are instantiated in that translation unit only.
int sg_gru_forward_launch(sg_ctx* ctx, const SgGruDesc& g, const float* W, const float* d_x, int x_ld, const float* d_h0,
                          const float* d_masks, int T, int n, float* d_gi, float* d_hout, int hout_ld, float* d_hlast,
                          const GruScanArgs* train);
