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
#include "sg_gru_kernels.hpp"

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

// rnn: sg_policy_create_cnn_rnn, the same base with nn.GRU(hidden, hidden) between the FC layer and the heads
static int cnn_create(const char* who, sg_ctx* ctx, int channels, int height, int width, int hidden, int dist, int act_dim, int n_out,
                      bool rnn, sg_policy** out) {
    SG_DEVICE_WIDE();
    SG_REQUIRE(ctx && out, "%s: NULL argument", who);
    SG_REQUIRE(height == SG_CNN_HW && width == SG_CNN_HW, "%s: the CNN base takes %d x %d images only (got %d x %d): "
               "the reference hard-codes Linear(32 * 7 * 7, hidden) behind its three convolutions (a2c/model.py:216)", who, SG_CNN_HW,
               SG_CNN_HW, height, width);
    SG_REQUIRE(channels > 0 && channels <= 4096 && hidden > 0 && hidden <= 65536, "%s: bad dims (channels %d, hidden %d)", who,
               channels, hidden);
    SG_REQUIRE(dist == SG_DIST_GAUSSIAN || dist == SG_DIST_CATEGORICAL, "%s: the CNN base is built with the Gaussian "
               "(Box) and Categorical (Discrete) heads; dist %d (%s) is not", who, dist, dist == SG_DIST_BERNOULLI ? "Bernoulli / MultiBinary" : "unknown");
    SG_REQUIRE(act_dim > 0 && act_dim <= 4096, "%s: bad act_dim %d", who, act_dim);
    if (dist == SG_DIST_CATEGORICAL) {
        SG_REQUIRE(n_out > 0 && n_out <= 4096, "%s: n_out = %d: need 0 < n_out <= 4096", who, n_out);
        SG_REQUIRE(act_dim == 1, "%s: act_dim (%d) must be 1 for a Categorical head (an action row is one class index)", who, act_dim);
    }
    const SgCnnDesc cd = make_cnn_desc(channels, hidden, dist, act_dim, n_out);
    // the GRU block starts on a 16-byte boundary behind the flat block (its images are staged with 128-bit loads)
    SgGruDesc gd;
    memset(&gd, 0, sizeof gd);
    if (rnn) {
        // before the descriptor is built (its offsets are ints): the reverse scan's two tiles hold at least 16 x 4 Hp floats
        // (sg_gru_bwd_lds), so a width whose 256 bytes per hidden unit exceed the LDS can never fit
        SG_REQUIRE((int64_t)256 * hidden <= (int64_t)ctx->lds_bytes, "%s: hidden %d: the GRU's 16-row tiles (at least %lld bytes for the "
                   "reverse scan's) do not fit the %d-byte LDS of a CU even with the weights read from global memory", who, hidden,
                   (long long)256 * hidden, ctx->lds_bytes);
        gd = sg_make_gru_desc(hidden, hidden, (cd.total + 3) & ~3);
        // the 16-row tiles of the global-weight instances are what has to fit: input projection, both scans, k_gru_dx
        const size_t need[4] = {sg_gru_proj_lds(gd, 1, true), sg_gru_scan_lds(gd, true), sg_gru_bwd_lds(gd, true), sg_gru_dx_lds(gd, true)};
        size_t worst = 0;
        for (size_t v : need) worst = v > worst ? v : worst;
        SG_REQUIRE(sg_cnn_gru_fits(ctx, gd), "%s: hidden %d: the GRU's 16-row tiles (%zu bytes for the largest: projection %zu, scan %zu, "
                   "reverse scan %zu, input gradient %zu) do not fit the %d-byte LDS of a CU even with the weights read from global "
                   "memory", who, hidden, worst, need[0], need[1], need[2], need[3], ctx->lds_bytes);
    }
    SG_CHECK(hipSetDevice(ctx->device));
    sg_policy* p = new sg_policy();
    p->ctx = ctx;
    p->cnn = true;
    p->cnnd = cd;
    // the stand-in the shared code reads: row widths, the head kernels' layout (trunk 0: P outputs, trunk 1: the value) and the
    // log-std's place in the parameter vector
    SgPolicyDesc& d = p->desc;
    memset(&d, 0, sizeof d);
    d.kind = SG_POLICY_MLP; d.O = channels * SG_CNN_HW * SG_CNN_HW; d.A = act_dim; d.H = hidden; d.Hc = hidden; d.num_feet = 1;
    d.n_trunks = 2; d.dist = dist; d.n_out = p->cnnd.P; d.total = p->cnnd.total;
    d.trunk[0].P = p->cnnd.P; d.trunk[0].Pp = SG_PAD16(p->cnnd.P); d.trunk[0].ex = p->cnnd.ls; d.trunk[0].EX = dist == SG_DIST_GAUSSIAN ? act_dim : 0;
    d.trunk[1].P = 1; d.trunk[1].Pp = 16;
    if (rnn) {
        p->recurrent = true;
        p->gru = gd;
    }
    const size_t total = sg_policy_padded_count(p);
    SG_CHECK(sg_dev_malloc((void**)&p->d_params, sizeof(float) * total));
    SG_CHECK(hipMemsetAsync(p->d_params, 0, sizeof(float) * total, ctx->stream));
    *out = p;
    return 0;
}

/* CNNBase on image observations, a2c/model.py:204-230 (chosen by Policy.__init__, a2c/model.py:40-50, for a 3-D obs_shape). */
extern "C" int sg_policy_create_cnn(sg_ctx* ctx, int channels, int height, int width, int hidden, int dist, int act_dim, int n_out,
                                    sg_policy** out) {
    return cnn_create("sg_policy_create_cnn", ctx, channels, height, width, hidden, dist, act_dim, n_out, false, out);
}

/* CNNBase(recurrent=True), a2c/model.py:117-230: the same trunk, nn.GRU(hidden, hidden) on its features (NNBase.__init__ creates it
   before `main`, so its four tensors come first in the flat order), critic_linear and the distribution's Linear on the GRU state.
   An entry point of its own: sg_policy_create_cnn is unchanged. */
extern "C" int sg_policy_create_cnn_rnn(sg_ctx* ctx, int channels, int height, int width, int hidden, int dist, int act_dim, int n_out,
                                        sg_policy** out) {
    return cnn_create("sg_policy_create_cnn_rnn", ctx, channels, height, width, hidden, dist, act_dim, n_out, true, out);
}

static dim3 cnn_grid(int64_t rows, int cols) { return dim3((unsigned)((rows + 63) / 64), (unsigned)((cols + 31) / 32)); }

int sg_cnn_trunk_forward_launch(sg_ctx* ctx, const sg_policy* p, const float* d_obs, const int64_t* d_idx, int n, float* act, float* F_out) {
    const SgCnnDesc& c = p->cnnd;
    const float* W = p->d_params;
    float* A1 = act;
    float* A2 = A1 + (size_t)n * SG_CNN_A1;
    float* A3 = A2 + (size_t)n * SG_CNN_A2;
    float* F = F_out ? F_out : A3 + (size_t)n * SG_CNN_A3;
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
    SG_CHECK(hipGetLastError());
    return 0;
}

int sg_cnn_head_forward_launch(sg_ctx* ctx, const sg_policy* p, const float* feat, int n, float* heads, int hld, int row0, int n_total) {
    const SgCnnDesc& c = p->cnnd;
    CnnHeadArgs h;
    h.d = c; h.params = p->d_params; h.feat = feat; h.n = n; h.row0 = row0; h.n_total = n_total; h.heads = heads; h.hld = hld;
    hipLaunchKernelGGL(k_cnn_head_fwd, dim3((unsigned)(((int64_t)n * (c.P + 1) + 255) / 256)), dim3(256), 0, ctx->stream, h);
    SG_CHECK(hipGetLastError());
    return 0;
}

int sg_cnn_forward_launch(sg_ctx* ctx, const sg_policy* p, const float* d_obs, const int64_t* d_idx, int n, float* act,
                          float* heads, int hld, int row0, int n_total) {
    SG_TRY(sg_cnn_trunk_forward_launch(ctx, p, d_obs, d_idx, n, act, nullptr));
    return sg_cnn_head_forward_launch(ctx, p, act + (size_t)n * (SG_CNN_A1 + SG_CNN_A2 + SG_CNN_A3), n, heads, hld, row0, n_total);
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
    const float* F = act + (size_t)n * (SG_CNN_A1 + SG_CNN_A2 + SG_CNN_A3);
    float* dZf = bwd + (size_t)n * (SG_CNN_A1 + SG_CNN_A2 + SG_CNN_A3);
    float* dout = dZf + (size_t)n * c.Hs;
    float* dls = dout + (size_t)n * (c.P + 1);
    float* rowl = dls + (size_t)n * c.A;

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
    return sg_cnn_trunk_backward_launch(ctx, p, d_obs, d_idx, n, act, bwd, grad, acc);
}

int sg_cnn_trunk_backward_launch(sg_ctx* ctx, const sg_policy* p, const float* d_obs, const int64_t* d_idx, int n, const float* act,
                                 float* bwd, float* grad, int acc) {
    const SgCnnDesc& c = p->cnnd;
    const float* W = p->d_params;
    const float* A1 = act;
    const float* A2 = A1 + (size_t)n * SG_CNN_A1;
    const float* A3 = A2 + (size_t)n * SG_CNN_A2;
    float* dZ1 = bwd;
    float* dZ2 = dZ1 + (size_t)n * SG_CNN_A1;
    float* dZ3 = dZ2 + (size_t)n * SG_CNN_A2;
    float* dZf = dZ3 + (size_t)n * SG_CNN_A3;
    float* slabs = dZf + (size_t)n * (c.Hs + (c.P + 1) + c.A + 3);
    slabs += (4 - ((slabs - bwd) & 3)) & 3;

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

// ------------------------------------------------------------------------------------- the recurrent CNN base
// sg_policy.hip: value / action / log-prob / entropy of n rows from head stacks [2][n][hld] (k_gauss_head / k_discrete_head)
int sg_policy_heads_device(sg_policy* p, const float* d_heads, int hld, int n, int mode, const float* d_noise, uint64_t seed,
                           const float* d_action_in, float* d_value, float* d_action, float* d_logp, float* d_ent);
int sg_policy_heads_ld(const SgPolicyDesc& d);

// CNNBase.forward with recurrent=True (a2c/model.py:224-230): x = main(inputs / 255); x, rnn_hxs = _forward_gru(x, rnn_hxs, masks);
// critic_linear(x), then the distribution on x.  The trunk runs in SG_CNN_FWD_ROWS-row passes into one feature matrix, the input
// projection and the scan over all T*n rows, the heads on h_t.  A row's trunk, GI and state have the same bits in a one-step
// call and inside a sequence (every output element is one fixed MFMA chain).
int sg_cnn_gru_forward_device(sg_policy* p, const float* d_obs, const float* d_h0, const float* d_masks, int T, int n, int mode,
                              const float* d_noise, uint64_t seed, const float* d_action_in, float* d_value, float* d_action,
                              float* d_logp, float* d_ent, float* d_hlast) {
    sg_ctx* ctx = p->ctx;
    const SgCnnDesc& c = p->cnnd;
    const SgGruDesc& g = p->gru;
    const int rows = T * n;
    const int hld = sg_policy_heads_ld(p->desc);
    const int chunk = rows < SG_CNN_FWD_ROWS ? rows : SG_CNN_FWD_ROWS;
    auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t f_heads = r4(2 * (size_t)rows * hld), f_feat = r4((size_t)rows * c.Hs), f_gi = r4((size_t)rows * 3 * g.Hp);
    float* scratch = nullptr;
    SG_TRY(sg_ctx_scratch(ctx, sizeof(float) * (f_heads + 2 * f_feat + f_gi + sg_cnn_fwd_floats(c, chunk)), &scratch));
    float* heads = scratch;
    float* F = heads + f_heads;
    float* hout = F + f_feat;
    float* gi = hout + f_feat;
    float* act = gi + f_gi;
    for (int r0 = 0; r0 < rows; r0 += chunk)
        SG_TRY(sg_cnn_trunk_forward_launch(ctx, p, d_obs + (size_t)r0 * p->desc.O, nullptr, rows - r0 < chunk ? rows - r0 : chunk, act,
                                           F + (size_t)r0 * c.Hs));
    SG_TRY(sg_gru_forward_launch(ctx, g, p->d_params + g.off, F, c.Hs, d_h0, d_masks, T, n, gi, hout, c.Hs, d_hlast, nullptr));
    SG_TRY(sg_cnn_head_forward_launch(ctx, p, hout, rows, heads, hld, 0, rows));
    return sg_policy_heads_device(p, heads, hld, rows, mode, d_noise, seed, d_action_in, d_value, d_action, d_logp, d_ent);
}

// The heads of the recurrent CNN base on the GRU states of n rows: forward, loss block, d loss / d h_t, head gradients.  a2c: the
// A2C loss block on the indexed rows (k_cnn_head_loss_a2c_idx) instead of PPO's; acc: the head gradients and the three loss sums
// add to what grad holds (a later environment group of one A2C update).  PPO passes 0, 0.
int sg_cnn_gru_heads_launch(sg_ctx* ctx, const sg_policy* p, const sg_rollout* r, const int64_t* d_idx, int n, const float* hstate,
                            float* heads, int hld, float* bwd, float* grad, float* dxa, float* dxc, int dx_ld, float inv_B, float clip,
                            float vcoef, float ecoef, int use_clipped, int a2c, int acc) {
    const SgCnnDesc& c = p->cnnd;
    const float* W = p->d_params;
    float* dZf = bwd + (size_t)n * (SG_CNN_A1 + SG_CNN_A2 + SG_CNN_A3);
    float* dout = dZf + (size_t)n * c.Hs;
    float* dls = dout + (size_t)n * (c.P + 1);
    float* rowl = dls + (size_t)n * c.A;
    SG_TRY(sg_cnn_head_forward_launch(ctx, p, hstate, n, heads, hld, 0, n));
    CnnLossArgs l;
    l.d = c; l.params = W; l.heads = heads; l.hld = hld; l.n = n; l.idx = d_idx; l.row0 = 0;
    l.actions = r->d_field[SG_F_ACTIONS]; l.old_logp = r->d_field[SG_F_LOGP]; l.adv = r->d_field[SG_F_ADVANTAGES];
    l.vpred = r->d_field[SG_F_VALUE_PREDS]; l.ret = r->d_field[SG_F_RETURNS];
    l.inv_B = inv_B; l.clip = clip; l.vcoef = vcoef; l.ecoef = ecoef; l.use_clipped = use_clipped;
    l.dout = dout; l.dls = dls; l.rowl = rowl;
    if (a2c) hipLaunchKernelGGL(k_cnn_head_loss_a2c_idx, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, l);
    else hipLaunchKernelGGL(k_cnn_head_loss, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, l);
    CnnHeadDhArgs dh;
    dh.d = c; dh.params = W; dh.dout = dout; dh.n = n; dh.ld = dx_ld; dh.dxa = dxa; dh.dxc = dxc;
    hipLaunchKernelGGL(k_cnn_head_dh, dim3((unsigned)(((int64_t)n * dx_ld + 255) / 256)), dim3(256), 0, ctx->stream, dh);
    CnnHeadBwdArgs hb;
    hb.d = c; hb.params = W; hb.feat = hstate; hb.dout = dout; hb.dls = dls; hb.rowl = rowl; hb.n = n; hb.acc = acc; hb.dzf = nullptr; hb.grad = grad;
    hb.d.total = p->gru.off;   // the three loss sums go where k_gru_reduce picks them up: behind the flat block's padding
    const int n_head = (c.P + 1) * (c.Hs + 1) + c.A;
    hipLaunchKernelGGL(k_cnn_head_wgrad, dim3((unsigned)((n_head + 255) / 256)), dim3(256), 0, ctx->stream, hb);
    SG_CHECK(hipGetLastError());
    return 0;
}
