// sg_cnn.hip -- the CNN base of Policy on [C, 84, 84] image observations: creation, layout and the launch sequences of its
// forward and backward passes (kernels: sg_cnn_kernels.hpp).  The entry points a policy handle goes through (sg_policy_act /
// _get_value / _evaluate, sg_rollout_compute_returns_policy: sg_policy.hip; sg_ppo_update: sg_ppo.hip) call in here.
// The backward has two forms: PPO's (one minibatch through a permutation, the gradient written) and A2C's (one row chunk of the
// rollout in place, k_cnn_head_loss_a2c, the gradient written by the first chunk and added to by every later one).
//
// Replaces (reference, a2c/ = third_party/a2c_ppo_acktr/):
//   CNNBase.__init__ / forward        a2c/model.py:204-230   (feed-forward: Conv 8/4 - Conv 4/2 - Conv 3/1 - Flatten - Linear, ReLU
//                                                             after each, critic_linear on the shared features)
//   Policy.__init__'s base choice     a2c/model.py:40-50     (len(obs_shape) == 3 -> CNNBase)
#include <string.h>

#include "sg_common.h"
#include "sg_cnn_kernels.hpp"

// per-row floats of the three feature maps
#define SG_CNN_A1 (32 * 20 * 20)
#define SG_CNN_A2 (64 * 9 * 9)
#define SG_CNN_A3 SG_CNN_FLAT

static SgCnnDesc make_cnn_desc(int C, int Hs, int dist, int act_dim, int n_out) {
    SgCnnDesc c;
    memset(&c, 0, sizeof c);
    c.C = C; c.Hs = Hs; c.dist = dist; c.A = act_dim; c.P = dist == SG_DIST_GAUSSIAN ? act_dim : n_out;
    int o = 0;
    c.w1 = o; o += 32 * C * 64;  c.b1 = o; o += 32;
    c.w2 = o; o += 64 * 32 * 16; c.b2 = o; o += 64;
    c.w3 = o; o += 32 * 64 * 9;  c.b3 = o; o += 32;
    c.wf = o; o += Hs * SG_CNN_FLAT; c.bf = o; o += Hs;
    c.wc = o; o += Hs; c.bc = o; o += 1;
    c.wd = o; o += c.P * Hs; c.bd = o; o += c.P;
    c.ls = o; if (dist == SG_DIST_GAUSSIAN) o += act_dim;
    c.total = o;
    return c;
}

size_t sg_cnn_fwd_floats(const SgCnnDesc& c, int n) { return (size_t)n * (SG_CNN_A1 + SG_CNN_A2 + SG_CNN_A3 + c.Hs); }

// weight-gradient slabs of one layer: its (image, oy, ox) reduction in at most 32 pieces of at least 512 rows
static int cnn_wgrad_slabs(int64_t rows) {
    const int64_t s = (rows + 511) / 512;
    return (int)(s < 1 ? 1 : (s > 32 ? 32 : s));
}
static size_t cnn_slab_floats(const SgCnnDesc& c, int n) {
    const size_t l1 = (size_t)cnn_wgrad_slabs((int64_t)n * 400) * 32 * (c.C * 64 + 1);
    const size_t l2 = (size_t)cnn_wgrad_slabs((int64_t)n * 81) * 64 * (32 * 16 + 1);
    const size_t l3 = (size_t)cnn_wgrad_slabs((int64_t)n * 49) * 32 * (64 * 9 + 1);
    const size_t lf = (size_t)cnn_wgrad_slabs(n) * c.Hs * (SG_CNN_FLAT + 1);
    size_t m = l1 > l2 ? l1 : l2;
    m = m > l3 ? m : l3;
    return m > lf ? m : lf;
}
// dZ1 | dZ2 | dZ3 | dZf | dout | dls | rowl | slabs
size_t sg_cnn_bwd_floats(const SgCnnDesc& c, int n) {
    return (size_t)n * (SG_CNN_A1 + SG_CNN_A2 + SG_CNN_A3 + c.Hs + (c.P + 1) + c.A + 3) + cnn_slab_floats(c, n) + 16;
}

/* CNNBase on image observations, a2c/model.py:204-230 (chosen by Policy.__init__, a2c/model.py:40-50, for a 3-D obs_shape). */
extern "C" int sg_policy_create_cnn(sg_ctx* ctx, int channels, int height, int width, int hidden, int dist, int act_dim, int n_out,
                                    sg_policy** out) {
    SG_DEVICE_WIDE();
    SG_REQUIRE(ctx && out, "sg_policy_create_cnn: NULL argument");
    SG_REQUIRE(height == SG_CNN_HW && width == SG_CNN_HW, "sg_policy_create_cnn: the CNN base takes %d x %d images only (got %d x %d): "
               "the reference hard-codes Linear(32 * 7 * 7, hidden) behind its three convolutions (a2c/model.py:216)", SG_CNN_HW,
               SG_CNN_HW, height, width);
    SG_REQUIRE(channels > 0 && channels <= 4096 && hidden > 0 && hidden <= 65536, "sg_policy_create_cnn: bad dims (channels %d, hidden %d)",
               channels, hidden);
    SG_REQUIRE(dist == SG_DIST_GAUSSIAN || dist == SG_DIST_CATEGORICAL, "sg_policy_create_cnn: the CNN base is built with the Gaussian "
               "(Box) and Categorical (Discrete) heads; dist %d (%s) is not", dist, dist == SG_DIST_BERNOULLI ? "Bernoulli / MultiBinary" : "unknown");
    SG_REQUIRE(act_dim > 0 && act_dim <= 4096, "sg_policy_create_cnn: bad act_dim %d", act_dim);
    if (dist == SG_DIST_CATEGORICAL) {
        SG_REQUIRE(n_out > 0 && n_out <= 4096, "sg_policy_create_cnn: n_out = %d: need 0 < n_out <= 4096", n_out);
        SG_REQUIRE(act_dim == 1, "sg_policy_create_cnn: act_dim (%d) must be 1 for a Categorical head (an action row is one class index)", act_dim);
    }
    SG_CHECK(hipSetDevice(ctx->device));
    sg_policy* p = new sg_policy();
    p->ctx = ctx;
    p->cnn = true;
    p->cnnd = make_cnn_desc(channels, hidden, dist, act_dim, n_out);
    // the stand-in the shared code reads: row widths, the head kernels' layout (trunk 0: P outputs, trunk 1: the value) and the
    // log-std's place in the parameter vector
    SgPolicyDesc& d = p->desc;
    memset(&d, 0, sizeof d);
    d.kind = SG_POLICY_MLP; d.O = channels * SG_CNN_HW * SG_CNN_HW; d.A = act_dim; d.H = hidden; d.Hc = hidden; d.num_feet = 1;
    d.n_trunks = 2; d.dist = dist; d.n_out = p->cnnd.P; d.total = p->cnnd.total;
    d.trunk[0].P = p->cnnd.P; d.trunk[0].Pp = SG_PAD16(p->cnnd.P); d.trunk[0].ex = p->cnnd.ls; d.trunk[0].EX = dist == SG_DIST_GAUSSIAN ? act_dim : 0;
    d.trunk[1].P = 1; d.trunk[1].Pp = 16;
    SG_CHECK(sg_dev_malloc((void**)&p->d_params, sizeof(float) * (size_t)d.total));
    SG_CHECK(hipMemsetAsync(p->d_params, 0, sizeof(float) * (size_t)d.total, ctx->stream));
    *out = p;
    return 0;
}

static dim3 cnn_grid(int64_t rows, int cols) { return dim3((unsigned)((rows + 63) / 64), (unsigned)((cols + 31) / 32)); }

int sg_cnn_forward_launch(sg_ctx* ctx, const sg_policy* p, const float* d_obs, const int64_t* d_idx, int n, float* act,
                          float* heads, int hld, int row0, int n_total) {
    const SgCnnDesc& c = p->cnnd;
    const float* W = p->d_params;
    float* A1 = act;
    float* A2 = A1 + (size_t)n * SG_CNN_A1;
    float* A3 = A2 + (size_t)n * SG_CNN_A2;
    float* F = A3 + (size_t)n * SG_CNN_A3;
    CnnConvArgs a;
    memset(&a, 0, sizeof a);
    a.n_img = n;
    a.in = d_obs; a.idx = d_idx; a.w = W + c.w1; a.bias = W + c.b1; a.out = A1; a.div255 = 1;
    a.Ci = c.C; a.Co = 32; a.IH = a.IW = 84; a.OH = a.OW = 20;
    hipLaunchKernelGGL((k_cnn_conv_fwd<8, 8, 4>), cnn_grid((int64_t)n * 400, 32), dim3(256), 0, ctx->stream, a);
    a.in = A1; a.idx = nullptr; a.w = W + c.w2; a.bias = W + c.b2; a.out = A2; a.div255 = 0;
    a.Ci = 32; a.Co = 64; a.IH = a.IW = 20; a.OH = a.OW = 9;
    hipLaunchKernelGGL((k_cnn_conv_fwd<4, 4, 2>), cnn_grid((int64_t)n * 81, 64), dim3(256), 0, ctx->stream, a);
    a.in = A2; a.w = W + c.w3; a.bias = W + c.b3; a.out = A3;
    a.Ci = 64; a.Co = 32; a.IH = a.IW = 9; a.OH = a.OW = 7;
    hipLaunchKernelGGL((k_cnn_conv_fwd<3, 3, 1>), cnn_grid((int64_t)n * 49, 32), dim3(256), 0, ctx->stream, a);
    a.in = A3; a.w = W + c.wf; a.bias = W + c.bf; a.out = F;
    a.Ci = 32; a.Co = c.Hs; a.IH = a.IW = 7; a.OH = a.OW = 1;
    hipLaunchKernelGGL((k_cnn_conv_fwd<7, 7, 1>), cnn_grid(n, c.Hs), dim3(256), 0, ctx->stream, a);
    CnnHeadArgs h;
    h.d = c; h.params = W; h.feat = F; h.n = n; h.row0 = row0; h.n_total = n_total; h.heads = heads; h.hld = hld;
    hipLaunchKernelGGL(k_cnn_head_fwd, dim3((unsigned)(((int64_t)n * (c.P + 1) + 255) / 256)), dim3(256), 0, ctx->stream, h);
    SG_CHECK(hipGetLastError());
    return 0;
}

template <typename KernelT>
static void cnn_wgrad_layer(sg_ctx* ctx, KernelT kernel, const float* dz, const float* in, const int64_t* idx, int n, int ohw, int Ci, int Co,
                            int kk, int div255, float* slabs, float* gw, float* gb, int acc) {
    const int64_t rows = (int64_t)n * ohw;
    const int S = cnn_wgrad_slabs(rows);
    CnnWgradArgs w;
    w.dz = dz; w.in = in; w.idx = idx; w.slabs = slabs; w.n_img = n; w.Ci = Ci; w.Co = Co; w.div255 = div255;
    w.rows_per_slab = (int)((((rows + S - 1) / S) + 3) & ~(int64_t)3);
    const int K = Ci * kk, N = K + 1;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((N + 127) / 128), (unsigned)((Co + 15) / 16), (unsigned)S), dim3(256), 0, ctx->stream, w);
    hipLaunchKernelGGL(k_cnn_reduce, dim3((unsigned)(((int64_t)Co * N + 255) / 256)), dim3(256), 0, ctx->stream, slabs, S, Co, K, gw, gb, acc);
}

int sg_cnn_backward_launch(sg_ctx* ctx, const sg_policy* p, const sg_rollout* r, const float* d_obs, const int64_t* d_idx, int n,
                           const float* act, const float* heads, int hld, float* bwd, float* grad, float inv_B, float clip,
                           float vcoef, float ecoef, int use_clipped, int a2c, int acc, int64_t row0) {
    const SgCnnDesc& c = p->cnnd;
    const float* W = p->d_params;
    const float* A1 = act;
    const float* A2 = A1 + (size_t)n * SG_CNN_A1;
    const float* A3 = A2 + (size_t)n * SG_CNN_A2;
    const float* F = A3 + (size_t)n * SG_CNN_A3;
    float* dZ1 = bwd;
    float* dZ2 = dZ1 + (size_t)n * SG_CNN_A1;
    float* dZ3 = dZ2 + (size_t)n * SG_CNN_A2;
    float* dZf = dZ3 + (size_t)n * SG_CNN_A3;
    float* dout = dZf + (size_t)n * c.Hs;
    float* dls = dout + (size_t)n * (c.P + 1);
    float* rowl = dls + (size_t)n * c.A;
    float* slabs = rowl + 3 * (size_t)n;
    slabs += (4 - ((slabs - bwd) & 3)) & 3;

    CnnLossArgs l;
    l.d = c; l.params = W; l.heads = heads; l.hld = hld; l.n = n; l.idx = d_idx; l.row0 = row0;
    l.actions = r->d_field[SG_F_ACTIONS]; l.old_logp = r->d_field[SG_F_LOGP]; l.adv = r->d_field[SG_F_ADVANTAGES];
    l.vpred = r->d_field[SG_F_VALUE_PREDS]; l.ret = r->d_field[SG_F_RETURNS];
    l.inv_B = inv_B; l.clip = clip; l.vcoef = vcoef; l.ecoef = ecoef; l.use_clipped = use_clipped;
    l.dout = dout; l.dls = dls; l.rowl = rowl;
    if (a2c) hipLaunchKernelGGL(k_cnn_head_loss_a2c, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, l);
    else hipLaunchKernelGGL(k_cnn_head_loss, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, l);

    CnnHeadBwdArgs hb;
    hb.d = c; hb.params = W; hb.feat = F; hb.dout = dout; hb.dls = dls; hb.rowl = rowl; hb.n = n; hb.acc = acc; hb.dzf = dZf; hb.grad = grad;
    hipLaunchKernelGGL(k_cnn_head_dfeat, dim3((unsigned)(((int64_t)n * c.Hs + 255) / 256)), dim3(256), 0, ctx->stream, hb);
    const int n_head = (c.P + 1) * (c.Hs + 1) + c.A;
    hipLaunchKernelGGL(k_cnn_head_wgrad, dim3((unsigned)((n_head + 255) / 256)), dim3(256), 0, ctx->stream, hb);

    // FC: weight gradient on A3, data gradient dZf x Wf (a 1x1 "convolution" with the weight read transposed), conv3's mask
    cnn_wgrad_layer(ctx, k_cnn_wgrad<7, 7, 1, 1>, dZf, A3, nullptr, n, 1, 32, c.Hs, 49, 0, slabs, grad + c.wf, grad + c.bf, acc);
    CnnConvArgs a;
    memset(&a, 0, sizeof a);
    a.n_img = n;
    a.in = dZf; a.w = W + c.wf; a.out = dZ3; a.wt = 1;
    a.Ci = c.Hs; a.Co = SG_CNN_FLAT; a.IH = a.IW = 1; a.OH = a.OW = 1;
    hipLaunchKernelGGL((k_cnn_conv_fwd<1, 1, 1>), cnn_grid(n, SG_CNN_FLAT), dim3(256), 0, ctx->stream, a);
    const int64_t n3 = (int64_t)n * SG_CNN_A3;
    hipLaunchKernelGGL(k_cnn_relu_mask, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, ctx->stream, dZ3, A3, n3);
    // conv3
    cnn_wgrad_layer(ctx, k_cnn_wgrad<3, 3, 1, 7>, dZ3, A2, nullptr, n, 49, 64, 32, 9, 0, slabs, grad + c.w3, grad + c.b3, acc);
    a.wt = 0;
    a.in = dZ3; a.w = W + c.w3; a.mask = A2; a.out = dZ2;
    a.Ci = 64; a.Co = 32; a.IH = a.IW = 9; a.OH = a.OW = 7;
    hipLaunchKernelGGL((k_cnn_conv_bwd_data<3, 3, 1>), cnn_grid((int64_t)n * 81, 64), dim3(256), 0, ctx->stream, a);
    // conv2
    cnn_wgrad_layer(ctx, k_cnn_wgrad<4, 4, 2, 9>, dZ2, A1, nullptr, n, 81, 32, 64, 16, 0, slabs, grad + c.w2, grad + c.b2, acc);
    a.in = dZ2; a.w = W + c.w2; a.mask = A1; a.out = dZ1;
    a.Ci = 32; a.Co = 64; a.IH = a.IW = 20; a.OH = a.OW = 9;
    hipLaunchKernelGGL((k_cnn_conv_bwd_data<4, 4, 2>), cnn_grid((int64_t)n * 400, 32), dim3(256), 0, ctx->stream, a);
    // conv1 (no data gradient: the observation is a leaf)
    cnn_wgrad_layer(ctx, k_cnn_wgrad<8, 8, 4, 20>, dZ1, d_obs, d_idx, n, 400, c.C, 32, 64, 1, slabs, grad + c.w1, grad + c.b1, acc);
    SG_CHECK(hipGetLastError());
    return 0;
}
