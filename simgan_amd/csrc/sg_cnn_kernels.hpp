// sg_cnn_kernels.hpp -- the CNN base of Policy on image observations (a2c/model.py:204-230) as implicit GEMMs on the gfx950
// fp32 matrix cores (v_mfma_f32_16x16x4_f32 through sg_mfma).
//
// Every convolution, the FC layer (a 7x7 convolution of the [32, 7, 7] map onto one pixel: its K index (ci, ky, kx) IS torch's
// channel-major flatten order) and their backward products are one of three GEMM forms.  None builds an im2col buffer: the
// A-operand load computes the patch address (conv1's patches overlap 4x, so an explicit im2col would quadruple the largest read
// of the step).  A wave owns a 16-row x 32-column output tile and walks K four at a time, lane (i = lane & 15, q = lane >> 4)
// supplying A[row i][k + q] and B[k + q][column i] straight from global memory (L1 / L2 serve the reuse between the lanes of a
// tile and between neighbouring tiles).  The summation order of every output element is fixed by the shape alone, so two runs,
// and a graph replay against direct launches, are bit-identical.
//
//   forward          rows (image, oy, ox)   columns co   K = (ci, ky, kx)   A = x[n, ci, oy s + ky, ox s + kx]   B = W[co][K]
//   data gradient    rows (image, iy, ix)   columns ci   K = (co, ky, kx)   A = dZ[n, co, (iy - ky) / s, (ix - kx) / s] where
//                    that is a pixel of the output map, else 0 (the gather form of col2im: no atomics)     B = W[co][ci][ky][kx]
//   weight gradient  rows co   columns (ci, ky, kx) and one more, the bias   reduction over (image, oy, ox), cut into slabs that
//                    k_cnn_reduce adds in ascending order                   A = dZ^T   B = the patches (1 for the bias column)
//
// Tensors are NCHW as in torch.  dZ is always the gradient at a layer's PRE-activation: the data-gradient epilogue masks with
// (activation > 0) of the layer below, ReLU's derivative at exactly 0 being 0 as in torch.
#pragma once
#include "sg_common.h"

#define SG_CNN_HW 84
#define SG_CNN_FLAT 1568   // 32 * 7 * 7

struct CnnConvArgs {
    const float* in;      // forward: [*, Ci, IH, IW]; data gradient: dZ of the layer's OUTPUT [n, Co, OH, OW]
    const float* w;       // [Co][Ci * KH * KW]
    const float* bias;    // forward: [Co]
    const float* mask;    // data gradient: the activations the layer READ, [n, Ci, IH, IW] (post-ReLU)
    float* out;           // forward: [n, Co, OH, OW]; data gradient: [n, Ci, IH, IW]
    const int64_t* idx;   // forward, optional: image n is in[idx[n]] (a minibatch read in place from the rollout)
    int n_img, Ci, Co, IH, IW, OH, OW;
    int div255;           // forward: the input is x / 255.0 (a2c/model.py:226), a true float32 division
    int wt;               // forward: B[k][co] = w[k * Co + co] (the FC layer's data gradient, dZ x W, as a 1x1 "convolution")
};

template <int KH, int KW, int S>
__global__ __launch_bounds__(256) void k_cnn_conv_fwd(CnnConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
    constexpr int KK = KH * KW;
    const int OHW = a.OH * a.OW, IHW = a.IH * a.IW;
    const int M = a.n_img * OHW, K = a.Ci * KK;
    const int row0 = (blockIdx.x * 4 + wave) * 16;
    if (row0 >= M) return;
    const int col0 = blockIdx.y * 32;
    const int row = row0 + li;
    const bool rv = row < M;
    const int rr = rv ? row : row0;
    const int n = rr / OHW, p = rr - n * OHW, oy = p / a.OW, ox = p - oy * a.OW;
    const int64_t img = a.idx ? a.idx[n] : (int64_t)n;
    const float* ap = a.in + (size_t)img * a.Ci * IHW + (oy * S) * a.IW + ox * S;
    const int c0 = col0 + li, c1 = c0 + 16;
    const bool cv0 = c0 < a.Co, cv1 = c1 < a.Co;
    const float* bp0 = a.wt ? a.w + c0 : a.w + (size_t)c0 * K;
    const float* bp1 = a.wt ? a.w + c1 : a.w + (size_t)c1 * K;
    const int bs = a.wt ? a.Co : 1;
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + lq;
        const bool kv = k < K;
        const int kk = kv ? k : 0;
        const int ci = kk / KK, r2 = kk - ci * KK, ky = r2 / KW, kx = r2 - ky * KW;
        float av = (rv && kv) ? ap[ci * IHW + ky * a.IW + kx] : 0.f;
        if (a.div255) av = av / 255.0f;
        const float b0 = (cv0 && kv) ? bp0[(size_t)kk * bs] : 0.f;
        const float b1 = (cv1 && kv) ? bp1[(size_t)kk * bs] : 0.f;
        acc0 = sg_mfma(av, b0, acc0);
        acc1 = sg_mfma(av, b1, acc1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int orow = row0 + 4 * lq + r;
        if (orow >= M) continue;
        const int n2 = orow / OHW, p2 = orow - n2 * OHW;
        if (cv0) {
            const float v = a.bias ? fmaxf(acc0[r] + a.bias[c0], 0.f) : acc0[r];
            a.out[((size_t)n2 * a.Co + c0) * OHW + p2] = v;
        }
        if (cv1) {
            const float v = a.bias ? fmaxf(acc1[r] + a.bias[c1], 0.f) : acc1[r];
            a.out[((size_t)n2 * a.Co + c1) * OHW + p2] = v;
        }
    }
}

// d loss / d (the layer's input), masked by that input's own ReLU.  wt forms (FC) go through k_cnn_conv_fwd; this is the
// convolutions' gather form.
template <int KH, int KW, int S>
__global__ __launch_bounds__(256) void k_cnn_conv_bwd_data(CnnConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
    constexpr int KK = KH * KW;
    const int OHW = a.OH * a.OW, IHW = a.IH * a.IW;
    const int M = a.n_img * IHW, K = a.Co * KK;
    const int row0 = (blockIdx.x * 4 + wave) * 16;
    if (row0 >= M) return;
    const int col0 = blockIdx.y * 32;
    const int row = row0 + li;
    const bool rv = row < M;
    const int rr = rv ? row : row0;
    const int n = rr / IHW, p = rr - n * IHW, iy = p / a.IW, ix = p - iy * a.IW;
    const float* ap = a.in + (size_t)n * a.Co * OHW;
    const int c0 = col0 + li, c1 = c0 + 16;
    const bool cv0 = c0 < a.Ci, cv1 = c1 < a.Ci;
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int k = k0 + lq;   // K = Co * KH * KW is a multiple of 4 for every layer
        const int co = k / KK, r2 = k - co * KK, ky = r2 / KW, kx = r2 - ky * KW;
        const int dy = iy - ky, dx = ix - kx;
        const int oy = dy / S, ox = dx / S;
        const bool ok = rv && dy >= 0 && dx >= 0 && oy * S == dy && ox * S == dx && oy < a.OH && ox < a.OW;
        const float av = ok ? ap[co * OHW + oy * a.OW + ox] : 0.f;
        const float b0 = cv0 ? a.w[((size_t)co * a.Ci + c0) * KK + r2] : 0.f;
        const float b1 = cv1 ? a.w[((size_t)co * a.Ci + c1) * KK + r2] : 0.f;
        acc0 = sg_mfma(av, b0, acc0);
        acc1 = sg_mfma(av, b1, acc1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int orow = row0 + 4 * lq + r;
        if (orow >= M) continue;
        const int n2 = orow / IHW, p2 = orow - n2 * IHW;
        if (cv0) {
            const size_t o = ((size_t)n2 * a.Ci + c0) * IHW + p2;
            a.out[o] = a.mask[o] > 0.f ? acc0[r] : 0.f;
        }
        if (cv1) {
            const size_t o = ((size_t)n2 * a.Ci + c1) * IHW + p2;
            a.out[o] = a.mask[o] > 0.f ? acc1[r] : 0.f;
        }
    }
}

// The FC layer's data gradient comes out of k_cnn_conv_fwd unmasked (wt form); this applies conv3's ReLU mask in place.
__global__ __launch_bounds__(256) void k_cnn_relu_mask(float* g, const float* act, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = act[i] > 0.f ? g[i] : 0.f;
}

struct CnnWgradArgs {
    const float* dz;      // [n, Co, OW, OW] gradient at the layer's pre-activation
    const float* in;      // [*, Ci, IW, IW] what the layer read
    const int64_t* idx;   // optional, as in CnnConvArgs
    float* slabs;         // [gridDim.z][Co][Ci * KH * KW + 1]: weight rows with the bias gradient as their last column
    int n_img, Ci, Co;
    int rows_per_slab;    // reduction rows (image, oy, ox) per slab, a multiple of 4
    int div255;
};

template <int KH, int KW, int S, int OW>
__global__ __launch_bounds__(256) void k_cnn_wgrad(CnnWgradArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lq = lane >> 4;
    constexpr int KK = KH * KW, OHW = OW * OW, IW = (OW - 1) * S + KW, IHW = IW * IW;
    const int K = a.Ci * KK, N = K + 1;
    const int n0 = (blockIdx.x * 4 + wave) * 32;
    if (n0 >= N) return;
    const int m0 = blockIdx.y * 16;
    const int co = m0 + li;
    const bool cov = co < a.Co;
    const int ka = n0 + li, kb = ka + 16;
    int offa = 0, offb = 0;
    if (ka < K) { const int ci = ka / KK, r2 = ka - ci * KK, ky = r2 / KW; offa = ci * IHW + ky * IW + (r2 - ky * KW); }
    if (kb < K) { const int ci = kb / KK, r2 = kb - ci * KK, ky = r2 / KW; offb = ci * IHW + ky * IW + (r2 - ky * KW); }
    const int M = a.n_img * OHW;
    const int r_begin = blockIdx.z * a.rows_per_slab;
    const int r_end = min(M, r_begin + a.rows_per_slab);
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r0 = r_begin; r0 < r_end; r0 += 4) {
        const int r = r0 + lq;
        const bool rv = r < r_end;
        const int rr = rv ? r : r_begin;
        const int n = rr / OHW, p = rr - n * OHW, oy = p / OW, ox = p - oy * OW;
        const float av = (rv && cov) ? a.dz[((size_t)n * a.Co + co) * OHW + p] : 0.f;
        const int64_t img = a.idx ? a.idx[n] : (int64_t)n;
        const float* ip = a.in + (size_t)img * a.Ci * IHW + (oy * S) * IW + ox * S;
        float b0 = 0.f, b1 = 0.f;
        if (rv) {
            if (ka < K) { b0 = ip[offa]; if (a.div255) b0 = b0 / 255.0f; } else if (ka == K) b0 = 1.f;
            if (kb < K) { b1 = ip[offb]; if (a.div255) b1 = b1 / 255.0f; } else if (kb == K) b1 = 1.f;
        }
        acc0 = sg_mfma(av, b0, acc0);
        acc1 = sg_mfma(av, b1, acc1);
    }
    float* slab = a.slabs + (size_t)blockIdx.z * a.Co * N;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = m0 + 4 * lq + r;
        if (m >= a.Co) continue;
        if (ka < N) slab[(size_t)m * N + ka] = acc0[r];
        if (kb < N) slab[(size_t)m * N + kb] = acc1[r];
    }
}

// slabs [S][Co][K + 1] -> the flat gradient's weight [Co][K] and bias [Co], slab 0 first.  acc: the running value starts from
// what the flat gradient already holds (a later row chunk of one A2C update) instead of from 0
__global__ __launch_bounds__(256) void k_cnn_reduce(const float* slabs, int n_slabs, int Co, int K, float* gw, float* gb, int acc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = K + 1;
    if (i >= Co * N) return;
    const int co = i / N, k = i - co * N;
    float* dst = k < K ? gw + (size_t)co * K + k : gb + co;
    float g = acc ? *dst : 0.f;
    for (int s = 0; s < n_slabs; ++s) g += slabs[(size_t)s * Co * N + i];
    *dst = g;
}

// ------------------------------------------------------------------------------------------------ heads
// critic_linear and the distribution's Linear on the Hs shared features (a2c/model.py:229-230, a2c/distributions.py:74-104):
// 1 + P outputs per row, written in the layout k_gauss_head / k_discrete_head read (trunk 0: the P logits or means, trunk 1:
// the value in column 0).
struct CnnHeadArgs {
    SgCnnDesc d;
    const float* params;
    const float* feat;    // [n][Hs]
    int n;                // rows of this launch
    int row0, n_total;    // they are rows [row0, row0 + n) of the n_total-row head stacks
    float* heads;         // [2][n_total][hld]
    int hld;
};

__global__ __launch_bounds__(256) void k_cnn_head_fwd(CnnHeadArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int P1 = a.d.P + 1;
    if (i >= a.n * P1) return;
    const int row = i / P1, j = i - row * P1;
    const float* f = a.feat + (size_t)row * a.d.Hs;
    const float* w = j == 0 ? a.params + a.d.wc : a.params + a.d.wd + (size_t)(j - 1) * a.d.Hs;
    float s = 0.f;
    for (int h = 0; h < a.d.Hs; ++h) s += f[h] * w[h];
    s += j == 0 ? a.params[a.d.bc] : a.params[a.d.bd + j - 1];
    const size_t r = (size_t)(a.row0 + row);
    if (j == 0) a.heads[((size_t)a.n_total + r) * a.hld] = s;
    else a.heads[r * a.hld + (j - 1)] = s;
}

// The per-row losses and their gradients at the head outputs, one thread per row.  PPO (k_cnn_head_loss, a2c/algo/ppo.py:92-106):
// the arithmetic of k_ppo_bwd / k_ppo_bwd_dist's loss blocks (the clipped surrogate through sg_ppo_row_weight's lines, the clipped
// or plain value loss, the entropy bonus), reading the row's action and scalars in place from the rollout through idx.  A2C
// (k_cnn_head_loss_a2c, a2c/algo/a2c_acktr.py:65-72): adv = R - v, value loss adv^2, action loss -adv.detach() logp, on the
// chunk's rows [row0, row0 + n) of the rollout in its own order.  Both share the distribution arithmetic below.
struct CnnLossArgs {
    SgCnnDesc d;
    const float* params;
    const float* heads;   // [2][n][hld]
    int hld, n;
    const int64_t* idx;   // PPO: [n] rollout rows of this minibatch
    int64_t row0;         // A2C: the chunk's first rollout row
    const float *actions, *old_logp, *adv, *vpred, *ret;   // rollout fields (A2C reads actions and ret only)
    float inv_B, clip, vcoef, ecoef;   // A2C: inv_B = 1 / (T N) of the whole rollout in every chunk
    int use_clipped;
    float* dout;          // [n][1 + P]: d loss / d value, then d loss / d logits (or means)
    float* dls;           // [n][A] per-row d loss / d log-std (Gaussian)
    float* rowl;          // [3][n]: value loss, action loss, entropy of each row
};

// log-prob of the row's action and the entropy of its distribution at the head outputs z: Categorical with the row maximum
// subtracted and the log-normaliser from the OTHER classes' mass (log1p), Gaussian with the float32 constants of
// a2c/distributions.py's FixedNormal.  m, l1p and act are what sg_cnn_dist_grad needs again.
struct CnnDistRow {
    float logp, ent, m, l1p;
    int act;
};
__device__ __forceinline__ CnnDistRow sg_cnn_dist_row(const SgCnnDesc& d, const float* params, const float* z, const float* actions,
                                                      int64_t src) {
    CnnDistRow s;
    s.logp = 0.f; s.ent = 0.f; s.m = 0.f; s.l1p = 0.f; s.act = 0;
    if (d.dist == SG_DIST_CATEGORICAL) {
        const int K = d.P;
        s.m = z[0];
        int am = 0;
        for (int k = 1; k < K; ++k)
            if (z[k] > s.m) { s.m = z[k]; am = k; }
        float S = 0.f;
        for (int k = 0; k < K; ++k)
            if (k != am) S += expf(z[k] - s.m);
        s.l1p = log1pf(S);
        for (int k = 0; k < K; ++k) { const float lp = (z[k] - s.m) - s.l1p; s.ent -= expf(lp) * lp; }
        s.act = (int)actions[src];
        s.act = s.act < 0 ? 0 : (s.act > K - 1 ? K - 1 : s.act);
        s.logp = (z[s.act] - s.m) - s.l1p;
    } else {
        for (int k = 0; k < d.A; ++k) {
            const float ls = params[d.ls + k];
            const float sigma = expf(ls), diff = actions[src * d.A + k] - z[k], lsig = logf(sigma);
            s.logp += -(diff * diff) / (2.f * sigma * sigma) - lsig - 0.91893853320467274178f;
            s.ent += 0.5f + 0.91893853320467274178f + lsig;
        }
    }
    return s;
}

// d loss / d logits (or means, and the row's d loss / d log-std) from dlogp = d loss / d logp and dent = ecoef inv_B, the
// entropy bonus's weight
__device__ __forceinline__ void sg_cnn_dist_grad(const SgCnnDesc& d, const float* params, const float* z, const float* actions,
                                                 int64_t src, const CnnDistRow& s, float dlogp, float dent, float* dout, float* dls) {
    if (d.dist == SG_DIST_CATEGORICAL) {
        for (int k = 0; k < d.P; ++k) {
            const float lp = (z[k] - s.m) - s.l1p, p = expf(lp);
            dout[1 + k] = dlogp * ((k == s.act ? 1.f : 0.f) - p) + dent * p * (lp + s.ent);
        }
    } else {
        for (int k = 0; k < d.A; ++k) {
            const float ls = params[d.ls + k];
            const float sigma = expf(ls), var = sigma * sigma, diff = actions[src * d.A + k] - z[k];
            dout[1 + k] = dlogp * diff / var;
            dls[k] = dlogp * (diff * diff / var - 1.f) - dent;
        }
    }
}

__global__ __launch_bounds__(256) void k_cnn_head_loss(CnnLossArgs a) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.n) return;
    const SgCnnDesc& d = a.d;
    const int64_t src = a.idx[row];
    const float* z = a.heads + (size_t)row * a.hld;
    const float v = a.heads[((size_t)a.n + row) * a.hld];
    float* dout = a.dout + (size_t)row * (d.P + 1);
    {   // value loss
        const float Rt = a.ret[src], vo = a.vpred[src];
        float dv, lv;
        if (a.use_clipped) {
            const float dvv = v - vo;
            const float vc = vo + fminf(fmaxf(dvv, -a.clip), a.clip);
            const float u = (v - Rt) * (v - Rt), w = (vc - Rt) * (vc - Rt);
            const float m1 = u > w ? 1.f : (u < w ? 0.f : 0.5f);          // torch.max tie -> 1/2, 1/2
            const float pass = (dvv >= -a.clip && dvv <= a.clip) ? 1.f : 0.f;
            dv = 0.5f * a.inv_B * (m1 * 2.f * (v - Rt) + (1.f - m1) * 2.f * (vc - Rt) * pass);
            lv = 0.5f * fmaxf(u, w);
        } else {
            dv = 0.5f * a.inv_B * (-2.f) * (Rt - v);
            lv = 0.5f * (Rt - v) * (Rt - v);
        }
        dout[0] = dv * a.vcoef;
        a.rowl[row] = lv;
    }
    const CnnDistRow s = sg_cnn_dist_row(d, a.params, z, a.actions, src);
    // the clipped surrogate (a2c/algo/ppo.py:92-97)
    const float adv = a.adv[src];
    const float ratio = expf(s.logp - a.old_logp[src]);
    const float surr1 = ratio * adv;
    const float surr2 = fminf(fmaxf(ratio, 1.f - a.clip), 1.f + a.clip) * adv;
    const float w1 = surr1 < surr2 ? 1.f : (surr1 > surr2 ? 0.f : 0.5f);  // torch.min tie -> 1/2, 1/2
    const float inr = (ratio >= 1.f - a.clip && ratio <= 1.f + a.clip) ? 1.f : 0.f;
    const float dlogp = -a.inv_B * (w1 * adv + (1.f - w1) * adv * inr) * ratio;
    const float dent = a.ecoef * a.inv_B;
    a.rowl[a.n + row] = -fminf(surr1, surr2);
    a.rowl[2 * a.n + row] = s.ent;
    sg_cnn_dist_grad(d, a.params, z, a.actions, src, s, dlogp, dent, dout, a.dls + (size_t)row * d.A);
}

// A2C: loss = vcoef mean(adv^2) - mean(adv.detach() logp) - ecoef mean(ent) over ALL T N rows, of which this launch holds n;
// src: the rollout row of the launch's row `row`
__device__ __forceinline__ void sg_cnn_head_loss_a2c_row(const CnnLossArgs& a, int row, int64_t src) {
    const SgCnnDesc& d = a.d;
    const float* z = a.heads + (size_t)row * a.hld;
    const float v = a.heads[((size_t)a.n + row) * a.hld];
    float* dout = a.dout + (size_t)row * (d.P + 1);
    const float Rt = a.ret[src];
    const float adv = Rt - v;
    dout[0] = a.vcoef * 2.f * (v - Rt) * a.inv_B;
    a.rowl[row] = adv * adv;
    const CnnDistRow s = sg_cnn_dist_row(d, a.params, z, a.actions, src);
    a.rowl[a.n + row] = -(adv * s.logp);
    a.rowl[2 * a.n + row] = s.ent;
    // d/dlogp of -adv logp inv_B with adv detached; the value head's gradient is dout[0] alone
    sg_cnn_dist_grad(d, a.params, z, a.actions, src, s, -adv * a.inv_B, a.ecoef * a.inv_B, dout, a.dls + (size_t)row * d.A);
}

// a row chunk of the rollout in its own order: row -> row0 + row
__global__ __launch_bounds__(256) void k_cnn_head_loss_a2c(CnnLossArgs a) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.n) return;
    sg_cnn_head_loss_a2c_row(a, row, a.row0 + row);
}

// the indexed form (A2C through time on the recurrent CNN base: a group of environments, time-major): row -> idx[row]
__global__ __launch_bounds__(256) void k_cnn_head_loss_a2c_idx(CnnLossArgs a) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.n) return;
    sg_cnn_head_loss_a2c_row(a, row, a.idx[row]);
}

struct CnnHeadBwdArgs {
    SgCnnDesc d;
    const float* params;
    const float* feat;    // [n][Hs]
    const float* dout;    // [n][1 + P]
    const float* dls;     // [n][A]
    const float* rowl;    // [3][n]
    int n;
    int acc;              // k_cnn_head_wgrad: add to what grad holds (a later row chunk of one A2C update) instead of starting from 0
    float* dzf;           // [n][Hs]: gradient at the FC layer's pre-activation
    float* grad;          // the flat gradient (+ 3 loss sums behind it)
};

// d loss / d features through both heads, masked by the FC layer's ReLU
__global__ __launch_bounds__(256) void k_cnn_head_dfeat(CnnHeadBwdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const SgCnnDesc& d = a.d;
    if (i >= a.n * d.Hs) return;
    const int row = i / d.Hs, h = i - row * d.Hs;
    const float* dout = a.dout + (size_t)row * (d.P + 1);
    float g = dout[0] * a.params[d.wc + h];
    for (int j = 0; j < d.P; ++j) g += dout[1 + j] * a.params[d.wd + (size_t)j * d.Hs + h];
    a.dzf[i] = a.feat[i] > 0.f ? g : 0.f;
}

// The recurrent CNN base: the heads read the GRU state h_t, which is no ReLU output, so d loss / d h_t carries no mask.  Written as
// the two [n][ld] tiles k_gru_scan_bwd adds (dxa: through the distribution's Linear, dxc: through critic_linear), the padding
// columns Hs .. ld-1 as zero so that the padded hidden units' gate gradients stay zero.
struct CnnHeadDhArgs {
    SgCnnDesc d;
    const float* params;
    const float* dout;    // [n][1 + P]
    int n, ld;
    float *dxa, *dxc;     // [n][ld]
};

__global__ __launch_bounds__(256) void k_cnn_head_dh(CnnHeadDhArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const SgCnnDesc& d = a.d;
    if (i >= a.n * a.ld) return;
    const int row = i / a.ld, h = i - row * a.ld;
    float ga = 0.f, gc = 0.f;
    if (h < d.Hs) {
        const float* dout = a.dout + (size_t)row * (d.P + 1);
        gc = dout[0] * a.params[d.wc + h];
        for (int j = 0; j < d.P; ++j) ga += dout[1 + j] * a.params[d.wd + (size_t)j * d.Hs + h];
    }
    a.dxa[i] = ga;
    a.dxc[i] = gc;
}

// gradients of critic_linear, the distribution's Linear and the log-std: one thread per parameter, rows in ascending order;
// block 0 also leaves the three loss sums behind the gradient (k_ppo_adam's convention).  acc: every element, the loss sums
// too, starts from what grad already holds
__global__ __launch_bounds__(256) void k_cnn_head_wgrad(CnnHeadBwdArgs a) {
    const SgCnnDesc& d = a.d;
    const int P1 = d.P + 1, Hs = d.Hs;
    const int n_w = P1 * Hs, n_b = P1, n_ls = d.dist == SG_DIST_GAUSSIAN ? d.A : 0;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_w) {
        const int j = i / Hs, h = i - j * Hs;
        float* dst = a.grad + (j == 0 ? d.wc : d.wd + (j - 1) * Hs) + h;
        float g = a.acc ? *dst : 0.f;
        for (int r = 0; r < a.n; ++r) g += a.dout[(size_t)r * P1 + j] * a.feat[(size_t)r * Hs + h];
        *dst = g;
    } else if (i < n_w + n_b) {
        const int j = i - n_w;
        float* dst = a.grad + (j == 0 ? d.bc : d.bd + (j - 1));
        float g = a.acc ? *dst : 0.f;
        for (int r = 0; r < a.n; ++r) g += a.dout[(size_t)r * P1 + j];
        *dst = g;
    } else if (i < n_w + n_b + n_ls) {
        const int k = i - n_w - n_b;
        float g = a.acc ? a.grad[d.ls + k] : 0.f;
        for (int r = 0; r < a.n; ++r) g += a.dls[(size_t)r * d.A + k];
        a.grad[d.ls + k] = g;
    }
    if (blockIdx.x == 0) {
        __shared__ float red[256];
        for (int l = 0; l < 3; ++l) {
            float s = 0.f;
            for (int r = threadIdx.x; r < a.n; r += 256) s += a.rowl[(size_t)l * a.n + r];
            red[threadIdx.x] = s;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
                __syncthreads();
            }
            if (threadIdx.x == 0) a.grad[d.total + l] = a.acc ? a.grad[d.total + l] + red[0] : red[0];
            __syncthreads();
        }
    }
}
