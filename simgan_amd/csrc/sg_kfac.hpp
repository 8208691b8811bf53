// sg_kfac.hpp -- device kernels of ACKTR's K-FAC step (a2c/algo/kfac.py:148-255 with a2c/algo/a2c_acktr.py:72-100), the
// third mode of sg_ppo (sg_acktr_create).  The gradient is A2C's (k_ppo_fwd -> k_a2c_bwd -> k_a2c_reduce per chunk); per
// chunk the K-FAC statistics come from the same forward's row stacks:
//   k_acktr_fisher   the sampled-Fisher head gradients (a2c_acktr.py:75-90) back-propagated through both tanh trunks: the
//                    per-row gradient at every Linear output (the backward hook's grad_output, kfac.py:167-183)
//   k_kfac_stats     a^T a / g^T g of every distinct factor over the chunk's rows on the matrix cores (upper tiles only,
//                    mirrored), added to the update's sums: scratch is one set of factors, whatever T*N is
// then once per update:
//   k_kfac_fold      running averages m <- m 0.99 + f 0.01 (update_running_stat, kfac.py:90-94; m = f on the first update)
//   k_kfac_eig       cyclic Jacobi per distinct factor on the upper triangle (torch.symeig(upper=True), kfac.py:229-237),
//                    only when the device step counter says steps % Tf == 0; eigenvalues <= 1e-6 set to 0
//   k_kfac_gemm x4   v = Q_g ((Q_g^T grad Q_a) / (d_g d_a^T + damping)) Q_a^T per module, and the tiles' sums of v * grad
//   k_kfac_step      nu = min(1, sqrt(kl_clip / (sum(v grad) lr^2))), SGD with momentum (lr (1 - momentum)) on nu v
//   k_kfac_tick      steps += 1, the loss sums, the eigensolver's error word
#pragma once
#include "sg_common.h"
#include "sg_gemm.hpp"
#include "sg_rng.hpp"
#include "sg_thin.hpp"

#include <vector>

// distinct factors of Policy: A (layer inputs) 0 obs (actor.0 and critic.0 share it), 1 actor h1, 2 actor h2, 3 critic h1,
// 4 critic h2;  G (grad_output) 5 actor.0, 6 actor.2, 7 critic.0, 8 critic.2, 9 critic_linear, 10 dist.fc_mean, 11 dist.logstd
#define SG_KFAC_NA 5
#define SG_KFAC_NF 12
#define SG_KFAC_MODULES 13
#define SG_KFAC_SWEEPS 40          // Jacobi sweep cap: the solver raises the error word instead of returning a partial basis
#define SG_KFAC_JACOBI_TOL 1e-10   // rotate (p, q) while |a_pq| > tol sqrt(|a_pp a_qq|) and |a_pq| > tol ||A||_F / n (double)
#define SG_ACKTR_FROWS 32          // rows per k_acktr_fisher workgroup
#define SG_KFAC_STREAM 0xACC7000000ull   // sg_rng stream of the library's own value noise (+ the update index)

struct KfacDevState {   // device scalars of the K-FAC object
    int steps;          // KFACOptimizer.steps: completed updates
    int err;            // sticky: a Jacobi run hit SG_KFAC_SWEEPS
    int pad[2];
};

// value noise of one update: eps[r] = N(0, 1) keyed on (seed, update, row) -- torch.randn(values.size()) of a2c_acktr.py:82
__global__ __launch_bounds__(256) void k_acktr_noise(float* eps, int64_t n, uint64_t seed, int64_t update) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) eps[i] = sg_normal(seed, SG_KFAC_STREAM + (uint64_t)update, (uint64_t)i);
}

struct AcktrFisherArgs {
    SgPolicyDesc d;
    const float* params;
    const float* ACT;      // [cnt][A] the chunk's actions
    const float* eps;      // [cnt] the chunk's value noise
    const float* H1[2];    // [rows][trunk ldH] post-tanh activations of k_ppo_fwd (actor, critic)
    const float* H2[2];
    const float* OUT[2];   // [rows][ldP] head outputs
    int ldP, ldZ, cnt;
    float inv_B;
    float* Z1[2];          // [rows][ldZ] d fisher / d (layer-1 output), per trunk
    float* Z2[2];          // ... layer 2
    float* GMU;            // [rows][A] d fisher / d mu
    float* GLS;            // [rows][A] d fisher / d logstd (per row)
    float* GV;             // [rows] d fisher / d v
};

// grid (ceil(cnt / SG_ACKTR_FROWS), 2 trunks); dynamic LDS: FROWS * (P + H) floats
__global__ __launch_bounds__(256) void k_acktr_fisher(AcktrFisherArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int RB = SG_ACKTR_FROWS;
    const int t = blockIdx.y;
    const SgPolicyDesc& d = a.d;
    const SgTrunk& tr = d.trunk[t];
    const int H = tr.H, ldH = tr.ldH, A = d.A, P = t == 0 ? A : 1;
    const int r0 = blockIdx.x * RB;
    float* s_go = smem;
    float* s_z2 = smem + RB * P;
    const float* W = a.params + tr.off;
    // fisher_loss = -mean(logp) - mean((v - (v + eps).detach())^2): d/dmu = -(a - mu) / var / B, d/dlogstd = -((a - mu)^2 / var
    // - 1) / B, d/dv = 2 eps / B
    for (int i = threadIdx.x; i < RB * P; i += blockDim.x) {
        const int r = i / P, j = i - r * P, row = r0 + r;
        float g = 0.f;
        if (row < a.cnt) {
            if (t == 0) {
                const float mu = a.OUT[0][(size_t)row * a.ldP + j];
                const float sc = expf(W[tr.ex + j]);
                const float var = sc * sc;
                const float df = a.ACT[(size_t)row * A + j] - mu;
                g = -(df / var) * a.inv_B;
                a.GMU[(size_t)row * A + j] = g;
                a.GLS[(size_t)row * A + j] = -((df * df) / var - 1.f) * a.inv_B;
            } else {
                g = 2.f * a.eps[row] * a.inv_B;
                a.GV[row] = g;
            }
        }
        s_go[i] = g;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RB * H; i += blockDim.x) {   // z2 = (g_head W_h) * (1 - h2^2)
        const int r = i / H, c = i - r * H, row = r0 + r;
        float s = 0.f;
        for (int j = 0; j < P; ++j) s += s_go[r * P + j] * W[tr.wh + j * ldH + c];
        float z = 0.f;
        if (row < a.cnt) {
            const float h = a.H2[t][(size_t)row * ldH + c];
            z = s * (1.f - h * h);
            a.Z2[t][(size_t)row * a.ldZ + c] = z;
        }
        s_z2[i] = z;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RB * H; i += blockDim.x) {   // z1 = (z2 W_2) * (1 - h1^2)
        const int r = i / H, c = i - r * H, row = r0 + r;
        if (row >= a.cnt) continue;
        float s = 0.f;
        for (int k = 0; k < H; ++k) s += s_z2[r * H + k] * W[tr.w2 + k * ldH + c];
        const float h = a.H1[t][(size_t)row * ldH + c];
        a.Z1[t][(size_t)row * a.ldZ + c] = s * (1.f - h * h);
    }
}

struct KfacStatsArgs {
    const float* U[SG_KFAC_NF];   // [cnt][ld] the chunk's rows of each factor's source
    int ld[SG_KFAC_NF];
    int n[SG_KFAC_NF];
    int off[SG_KFAC_NF];          // factor f's [n][n] block in acc
    const int4* tiles;            // {factor, tile row, tile column (>= tile row), 0}
    float* acc;
    int cnt, accumulate;
};

// one workgroup per upper 16x16 tile of a factor: its 16 waves split the chunk's rows (v_mfma_f32_16x16x4_f32: lane (i, q)
// feeds row 4 s + q, column i of both operands; each wave issues the loads of four row quads before their MFMAs), combined in
// LDS in a fixed order and written to both triangles
#define SG_KFAC_STATS_WAVES 16
__global__ __launch_bounds__(64 * SG_KFAC_STATS_WAVES) void k_kfac_stats(KfacStatsArgs a) {
    constexpr int NW = SG_KFAC_STATS_WAVES;
    __shared__ float red[NW][256];
    const int4 tl = a.tiles[blockIdx.x];
    const int f = tl.x;
    const float* U = a.U[f];
    const int ld = a.ld[f], n = a.n[f];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = lane >> 4, ci = tl.y * 16 + (lane & 15), cj = tl.z * 16 + (lane & 15);
    const bool vi = ci < n, vj = cj < n;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int nq = (a.cnt + 3) >> 2;
    for (int s0 = w; s0 < nq; s0 += 4 * NW) {
        float x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = 4 * (s0 + u * NW) + q;
            x[u] = (row < a.cnt && vi) ? U[(size_t)row * ld + ci] : 0.f;
            y[u] = (row < a.cnt && vj) ? U[(size_t)row * ld + cj] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = sg_mfma(x[u], y[u], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[w][r * 64 + lane] = acc[r];
    __syncthreads();
    if (w == 0) {
        float* C = a.acc + a.off[f];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = tl.y * 16 + 4 * q + r;
            float v = 0.f;
            for (int k = 0; k < NW; k += 4)
                v += (red[k][r * 64 + lane] + red[k + 1][r * 64 + lane]) + (red[k + 2][r * 64 + lane] + red[k + 3][r * 64 + lane]);
            if (i < n && vj) {
                if (a.accumulate) v += C[(size_t)i * n + cj];
                C[(size_t)i * n + cj] = v;
                if (tl.y != tl.z) C[(size_t)cj * n + i] = v;
            }
        }
    }
}

// f = sums / B (A factors: a^T (a / B), kfac.py:72) or sums * B (G factors: (g B)^T (g B / B), kfac.py:87-88); m <- f on the
// first update, then m <- m * stat_decay + f * (1 - stat_decay) (update_running_stat).  Not in the reference's form
// ((m * 99) + f) * 0.01: in float32 neither 99.00009 (0.99f / (1 - 0.99f), rounded up by half an ulp) times 0.00999999 nor the
// reference's own 99 times 0.01f makes the two weights sum to 1, so every factor drifts by 3.8e-8 (2.2e-8 there) of itself per
// update, 3.8e-6 in the long run.  stat_decay and 1 - stat_decay are both float32 numbers (exactly, from 0.5 up): they sum to 1
__global__ __launch_bounds__(256) void k_kfac_fold(float* m, const float* acc, int total, int g_start, float inv_b, float b,
                                                   const KfacDevState* ks, float decay, float one_minus_decay) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float f = acc[i] * (i < g_start ? inv_b : b);
    const float v = ks->steps == 0 ? f : m[i];
    m[i] = __fmaf_rn(v, decay, __fmul_rn(f, one_minus_decay));
}

// Cyclic Jacobi, round-robin pair order, in double.  a: [n][n] working matrix (the upper triangle of m is mirrored into it),
// v: [n][n] eigenvector columns; both in LDS (small n) or in a global working copy.  Returns the sweeps taken, or -1.
__device__ int sg_kfac_jacobi(double* a, double* v, int n, const float* m, double* s_cs, int* s_pq, int* s_flag,
                              double* s_red) {
    const int tid = threadIdx.x, nt = blockDim.x;
    double part = 0.0;
    for (int i = tid; i < n * n; i += nt) {
        const int r = i / n, c = i - r * n;
        const double x = (double)(r <= c ? m[i] : m[(size_t)c * n + r]);
        a[i] = x;
        v[i] = r == c ? 1.0 : 0.0;
        part += x * x;
    }
    // ||A||_F for the absolute threshold
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    if ((tid & 63) == 0) s_red[tid >> 6] = part;
    __syncthreads();
    double nrm = 0.0;
    for (int w = 0; w < (nt + 63) / 64; ++w) nrm += s_red[w];
    nrm = sqrt(nrm);
    const double tabs = SG_KFAC_JACOBI_TOL * nrm / (double)(n > 0 ? n : 1);
    const int mm = n + (n & 1), np = mm / 2;
    for (int sweep = 0; sweep < SG_KFAC_SWEEPS; ++sweep) {
        if (tid == 0) *s_flag = 0;
        __syncthreads();
        for (int k = 0; k < mm - 1; ++k) {
            for (int i = tid; i < np; i += nt) {   // the round's disjoint pairs and their rotations
                int p, q;
                if (i == 0) { p = k; q = mm - 1; }
                else { p = (k + i) % (mm - 1); q = (k - i + (mm - 1)) % (mm - 1); }
                if (p > q) { const int x = p; p = q; q = x; }
                double c = 1.0, s = 0.0;
                int on = 0;
                if (q < n) {
                    const double app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q], apq = a[(size_t)p * n + q];
                    if (fabs(apq) > SG_KFAC_JACOBI_TOL * sqrt(fabs(app)) * sqrt(fabs(aqq)) && fabs(apq) > tabs) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                        on = 1;
                        *s_flag = 1;
                    }
                }
                s_cs[2 * i] = c; s_cs[2 * i + 1] = s;
                s_pq[2 * i] = on ? p : -1; s_pq[2 * i + 1] = q;
            }
            __syncthreads();
            for (int idx = tid; idx < np * n; idx += nt) {   // rows p, q <- J^T A
                const int i = idx / n, col = idx - i * n;
                const int p = s_pq[2 * i];
                if (p < 0) continue;
                const int q = s_pq[2 * i + 1];
                const double c = s_cs[2 * i], s = s_cs[2 * i + 1];
                const double ap = a[(size_t)p * n + col], aq = a[(size_t)q * n + col];
                a[(size_t)p * n + col] = c * ap - s * aq;
                a[(size_t)q * n + col] = s * ap + c * aq;
            }
            __syncthreads();
            for (int idx = tid; idx < np * n; idx += nt) {   // columns p, q <- A J, V J
                const int i = idx / n, row = idx - i * n;
                const int p = s_pq[2 * i];
                if (p < 0) continue;
                const int q = s_pq[2 * i + 1];
                const double c = s_cs[2 * i], s = s_cs[2 * i + 1];
                double* ar = a + (size_t)row * n;
                double* vr = v + (size_t)row * n;
                const double ap = ar[p], aq = ar[q];
                ar[p] = c * ap - s * aq;
                ar[q] = s * ap + c * aq;
                const double vp = vr[p], vq = vr[q];
                vr[p] = c * vp - s * vq;
                vr[q] = s * vp + c * vq;
            }
            __syncthreads();
            for (int i = tid; i < np; i += nt) {   // the rotated pair's off-diagonal entries are zero by construction
                const int p = s_pq[2 * i];
                if (p < 0) continue;
                const int q = s_pq[2 * i + 1];
                a[(size_t)p * n + q] = 0.0;
                a[(size_t)q * n + p] = 0.0;
            }
            __syncthreads();
        }
        if (*s_flag == 0) return sweep;
        __syncthreads();
    }
    return -1;
}

struct KfacEigArgs {
    const float* m;        // running factors
    float* Q;              // [n][n] eigenvectors (columns)
    float* dv;             // [n] eigenvalues, <= 1e-6 set to 0
    double* work;          // 2 n^2 doubles per factor for the global-memory path
    int n[SG_KFAC_NF];
    int off[SG_KFAC_NF];   // [n][n] blocks
    int voff[SG_KFAC_NF];  // [n] blocks
    int64_t woff[SG_KFAC_NF];
    int lds_n;             // largest n solved in LDS
    int tf;                // refresh every tf updates
    KfacDevState* ks;
    int* sweeps;           // [SG_KFAC_NF] optional (test hook)
};

// one workgroup per distinct factor; exits at once unless steps % Tf == 0 (one captured graph covers every update)
__global__ __launch_bounds__(512) void k_kfac_eig(KfacEigArgs a) {
    extern __shared__ __attribute__((aligned(16))) double dsm[];
    __shared__ double s_cs[2 * 256];
    __shared__ int s_pq[2 * 256];
    __shared__ int s_flag;
    __shared__ double s_red[8];
    if (a.ks && a.ks->steps % a.tf != 0) return;
    const int f = blockIdx.x, n = a.n[f];
    if (n <= 0) return;
    const bool lds = n <= a.lds_n;
    double* wa = lds ? dsm : a.work + a.woff[f];
    double* wv = wa + (size_t)n * n;
    int sw;
    if (n > 512) sw = -1;   // the pair arrays hold 256 pairs (sg_acktr_create refuses wider factors)
    else sw = sg_kfac_jacobi(wa, wv, n, a.m + a.off[f], s_cs, s_pq, &s_flag, s_red);
    if (sw < 0) {
        if (threadIdx.x == 0 && a.ks) atomicExch(&a.ks->err, 1);
    }
    if (threadIdx.x == 0 && a.sweeps) a.sweeps[f] = sw;
    float* Q = a.Q + a.off[f];
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) Q[i] = (float)wv[i];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float e = (float)wa[(size_t)i * n + i];
        a.dv[a.voff[f] + i] = e > 1e-6f ? e : 0.f;
    }
}

// One stage of the preconditioning, per module (blockIdx.y) and 32x32 output tile (blockIdx.x):
// C[M][N] = op(A)[M][K] op(B)[K][N]; epi 1: C /= (dg[m] da[n] + damping); epi 2: also sum(C * G) per tile into part.
struct KfacJob {
    int M, N, K, lda, ldb, ldc, ldg, ta, tb, epi;
    const float* A;
    const float* B;
    float* C;
    const float* dg;
    const float* da;
    const float* G;
};

__global__ __launch_bounds__(256) void k_kfac_gemm(const KfacJob* jobs, int max_tiles, float damping, float* part) {
    __shared__ float sA[16][33], sB[16][33];
    __shared__ float s_ws[4];
    const KfacJob& jb = jobs[blockIdx.y];
    const int tn = (jb.N + 31) >> 5, tm = (jb.M + 31) >> 5;
    const int tile = blockIdx.x, tid = threadIdx.x;
    if (tile >= tm * tn) {
        if (jb.epi == 2 && tid == 0) part[blockIdx.y * max_tiles + tile] = 0.f;
        return;
    }
    const int m0 = (tile / tn) * 32, n0 = (tile % tn) * 32;
    const int tx = tid & 15, ty = tid >> 4;
    float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
    for (int k0 = 0; k0 < jb.K; k0 += 16) {
        for (int e = tid; e < 512; e += 256) {
            const int kk = e >> 5, x = e & 31;
            const int k = k0 + kk, mr = m0 + x, nc = n0 + x;
            float va = 0.f, vb = 0.f;
            if (k < jb.K && mr < jb.M) va = jb.ta ? jb.A[(size_t)k * jb.lda + mr] : jb.A[(size_t)mr * jb.lda + k];
            if (k < jb.K && nc < jb.N) vb = jb.tb ? jb.B[(size_t)nc * jb.ldb + k] : jb.B[(size_t)k * jb.ldb + nc];
            sA[kk][x] = va;
            sB[kk][x] = vb;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int w = 0; w < 2; ++w) acc[u][w] += sA[kk][ty + 16 * u] * sB[kk][tx + 16 * w];
        }
        __syncthreads();
    }
    float vg = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int mr = m0 + ty + 16 * u, nc = n0 + tx + 16 * w;
            if (mr < jb.M && nc < jb.N) {
                float c = acc[u][w];
                if (jb.epi == 1) c = c / (jb.dg[mr] * jb.da[nc] + damping);
                jb.C[(size_t)mr * jb.ldc + nc] = c;
                if (jb.epi == 2) vg += c * jb.G[(size_t)mr * jb.ldg + nc];
            }
        }
    if (jb.epi == 2) {
        vg = sg_wave_sum(vg);
        if ((tid & 63) == 0) s_ws[tid >> 6] = vg;
        __syncthreads();
        if (tid == 0) part[blockIdx.y * max_tiles + tile] = (s_ws[0] + s_ws[1]) + (s_ws[2] + s_ws[3]);
    }
}

// nu = min(1, sqrt(kl_clip / (sum(v grad) lr^2))) (kfac.py:243-247, summed in double in a fixed order by every block);
// grad <- nu v; torch SGD(momentum, dampening 0): buf = grad on the first step, else buf * momentum + grad; p -= sgd_lr buf
__global__ __launch_bounds__(256) void k_kfac_step(float* params, float* buf, const float* v, const float* part, int n_part,
                                                   int total, const KfacDevState* ks, float lr, float kl_clip, float momentum,
                                                   float sgd_lr) {
    __shared__ double s_ws[4];
    __shared__ float s_nu;
    double s = 0.0;
    for (int j = threadIdx.x; j < n_part; j += 256) s += (double)part[j];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) s_ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double vg = ((s_ws[0] + s_ws[1]) + (s_ws[2] + s_ws[3])) * (double)lr * (double)lr;
        const double r = sqrt((double)kl_clip / vg);
        s_nu = (float)(r < 1.0 ? r : 1.0);
    }
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const float g = v[i] * s_nu;
        const float b = ks->steps == 0 ? g : __fadd_rn(__fmul_rn(buf[i], momentum), g);
        buf[i] = b;
        params[i] = __fadd_rn(params[i], __fmul_rn(-sgd_lr, b));
    }
}

// end of the update: steps += 1; the loss sums (the gradient's tail) over inv_b; loss_acc[3] <- the eigensolver's error word
__global__ void k_kfac_tick(KfacDevState* ks, const float* grad, int total, float inv_b, double* loss_acc) {
    if (threadIdx.x < 3) loss_acc[threadIdx.x] += (double)(grad[total + threadIdx.x] * inv_b);
    if (threadIdx.x == 0) {
        loss_acc[3] = (double)ks->err;
        ks->steps += 1;
    }
}

// ------------------------------------------------------------------------- host-side state (set up and read by sg_kfac_host.hpp)
// module m of KFACOptimizer.modules (a2c/algo/kfac.py:144-150 after split_bias: state_dict order): its gradient block in the
// padded vector and the distinct factors it reads (a_f < 0: an AddBias, A = [[1]])
struct KfacModule {
    int a_f, g_f;
    int goff, gld, out, in;
    int toff;   // its [out][in] block in the preconditioning temporaries
};

struct SgKfac {
    sg_acktr_config cfg;
    KfacModule mod[SG_KFAC_MODULES];
    int n[SG_KFAC_NF], off[SG_KFAC_NF], voff[SG_KFAC_NF];
    int64_t woff[SG_KFAC_NF];
    int fac_total = 0, vec_total = 0, g_start = 0, tmp_total = 0, max_tiles = 0, n_tiles = 0, lds_n = 0;
    int64_t work_doubles = 0;
    float *d_acc = nullptr, *d_m = nullptr, *d_Q = nullptr, *d_d = nullptr;   // factor sums, running averages, eigenbases
    double* d_work = nullptr;                                                 // the Jacobi working copies of large factors
    KfacDevState* d_ks = nullptr;
    float *d_vec = nullptr, *d_t0 = nullptr, *d_t1 = nullptr, *d_one = nullptr, *d_vpart = nullptr;
    KfacJob* d_jobs = nullptr;   // [4][13] preconditioning stages
    int4* d_tiles = nullptr;     // k_kfac_stats' tile list
    float* d_eps = nullptr;      // [T*N] value noise of the update
    int64_t eps_cap = 0;
    std::vector<float> eps_host; // injected noise for the next update (sg_acktr_set_value_noise)
    bool eps_pending = false;
    float* d_fish = nullptr;     // per-chunk Fisher gradients (k_acktr_fisher)
    size_t fish_cap = 0;
};
