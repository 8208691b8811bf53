// sg_gru.hip -- the GRU base of a recurrent Policy (act / get_value / evaluate_actions through time) as gfx950 kernels.
//
// Replaces (reference, a2c/ = third_party/a2c_ppo_acktr/):
//   NNBase.__init__ / _forward_gru            a2c/model.py:117-201  (nn.GRU(obs_dim, H), one layer, gates r, z, n)
//   MLPBase.forward with recurrent=True       a2c/model.py:255-264  (x = GRU(inputs, rnn_hxs * masks); trunks on x)
//   Policy.act / get_value / evaluate_actions a2c/model.py:89-114   (returning the new rnn_hxs)
//
// Two kernels (sg_gru_kernels.hpp: k_gru_inproj, k_gru_scan_fwd), then the feed-forward heads of sg_policy.hip on x = h_t
// (an MLP policy whose observation is the GRU state; with a Categorical / Bernoulli head -- sg_policy_create_rnn_dist -- the heads'
// launch is k_discrete_head, `noise` uniform draws and an action row a class index or n bits).  PPO through time is in sg_ppo.hip.
// The reference cuts the sequence where any mask is 0 and multiplies h by masks[t] at the head of each piece (a2c/model.py:
// 150-193); for 0/1 masks that is h_{t-1} <- h_{t-1} * masks[t] at every step, which is what the scan does.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sg_common.h"

int sg_policy_forward_device(sg_policy* p, const float* d_obs, int n, int mode, const float* d_noise,
                             uint64_t seed, const float* d_action_in, float* d_value, float* d_action,
                             float* d_logp, float* d_ent);

#include "sg_gru_kernels.hpp"

// GI for `rows` rows of d_x, then the scan over [T][n]; train != NULL: the TRAIN instance with its save buffers set in *train
// (PPO through time, sg_ppo.hip)
int sg_gru_forward_launch(sg_ctx* ctx, const SgGruDesc& g, const float* W, const float* d_x, int x_ld, const float* d_h0,
                                        const float* d_masks, int T, int n, float* d_gi, float* d_hout, int hout_ld, float* d_hlast,
                                        const GruScanArgs* train) {
    const int rows = T * n;
    {
        GruProjArgs a;
        a.g = g; a.W = W; a.x = d_x; a.x_ld = x_ld; a.rows = rows; a.gi = d_gi;
        const bool gw = sg_gru_force_gw() || sg_gru_proj_lds(g, 1, false) > (size_t)ctx->lds_bytes - 1024;
        a.wbuf_floats = gw ? 0 : 3 * g.Hp * g.ldO;
        int MT = 2;
        if (sg_gru_proj_lds(g, MT, gw) > (size_t)ctx->lds_bytes - 1024 || rows <= 16) MT = 1;
        const int R = 16 * MT;
        int gx = (rows + R - 1) / R;
        if (gx > 2 * ctx->num_cu) gx = 2 * ctx->num_cu;
        const size_t lds = sg_gru_proj_lds(g, MT, gw);
        if (gw) {
            if (MT == 2) hipLaunchKernelGGL((k_gru_inproj<2, true>), dim3(gx), dim3(256), lds, ctx->stream, a);
            else hipLaunchKernelGGL((k_gru_inproj<1, true>), dim3(gx), dim3(256), lds, ctx->stream, a);
        } else if (MT == 2) hipLaunchKernelGGL((k_gru_inproj<2, false>), dim3(gx), dim3(256), lds, ctx->stream, a);
        else hipLaunchKernelGGL((k_gru_inproj<1, false>), dim3(gx), dim3(256), lds, ctx->stream, a);
        SG_CHECK(hipGetLastError());
    }
    {
        GruScanArgs a;
        if (train) a = *train;
        else { a.sr = a.sz = a.sn = a.shn = a.hm = nullptr; }
        a.g = g; a.W = W; a.gi = d_gi; a.h0 = d_h0; a.masks = d_masks; a.T = T; a.n = n; a.hout = d_hout; a.hout_ld = hout_ld;
        a.hlast = d_hlast;
        const bool gw = sg_gru_force_gw() || sg_gru_scan_lds(g, false) > (size_t)ctx->lds_bytes - 1024;
        const size_t lds = sg_gru_scan_lds(g, gw);
        const dim3 grid((n + 15) / 16);
        if (train) {
            if (gw) hipLaunchKernelGGL((k_gru_scan_fwd<true, true>), grid, dim3(256), lds, ctx->stream, a);
            else hipLaunchKernelGGL((k_gru_scan_fwd<false, true>), grid, dim3(256), lds, ctx->stream, a);
        } else if (gw) hipLaunchKernelGGL((k_gru_scan_fwd<true, false>), grid, dim3(256), lds, ctx->stream, a);
        else hipLaunchKernelGGL((k_gru_scan_fwd<false, false>), grid, dim3(256), lds, ctx->stream, a);
        SG_CHECK(hipGetLastError());
    }
    return 0;
}

// the activation tiles of the global-weight instances are what has to fit (sg_policy_create2 checks it)
bool sg_gru_fits(const sg_ctx* ctx, const SgGruDesc& g) {
    return sg_gru_proj_lds(g, 1, true) <= (size_t)ctx->lds_bytes - 1024 && sg_gru_scan_lds(g, true) <= (size_t)ctx->lds_bytes - 1024 &&
           sg_gru_bwd_lds(g, true) <= (size_t)ctx->lds_bytes - 1024;
}

// the recurrent CNN base: the same three, and k_gru_dx's gate-gradient tile
bool sg_cnn_gru_fits(const sg_ctx* ctx, const SgGruDesc& g) {
    return sg_gru_fits(ctx, g) && sg_gru_dx_lds(g, true) <= (size_t)ctx->lds_bytes - 1024;
}

// GRU over a [T*n, O] time-major sequence (T == 1: one step) -> d_hout [T*n, H], d_hlast [n, H]; d_gi is [T*n][3*Hp] scratch.
static int gru_forward_dev(sg_policy* p, const float* d_x, const float* d_h0, const float* d_masks, int T, int n, float* d_gi,
                           float* d_hout, float* d_hlast) {
    return sg_gru_forward_launch(p->ctx, p->gru, p->d_params + p->gru.off, d_x, p->gru.O, d_h0, d_masks, T, n, d_gi, d_hout, p->gru.H,
                                 d_hlast, nullptr);
}

// host-pointer front end shared by the three recurrent calls: obs [T*n, O], hxs [n, H], masks [T*n]
static int gru_host_call(sg_policy* p, const char* who, const float* obs, const float* hxs, const float* masks, int T, int n,
                         int mode, const float* noise, uint64_t seed, const float* action_in, float* value, float* action,
                         float* logp, float* ent_rows, float* hxs_out) {
    sg_ctx* ctx = p->ctx;
    SG_REQUIRE(p->recurrent, "%s: this policy is feed-forward (kind %d); the recurrent entry points take a policy of kind SG_POLICY_GRU",
               who, p->desc.kind);
    SG_REQUIRE(T > 0 && n > 0 && (int64_t)T * n < (1ll << 30), "%s: T and n must be positive (got %d, %d)", who, T, n);
    const SgGruDesc& g = p->gru;
    // the recurrent CNN base (sg_cnn.hip): an observation row is the C*84*84-float image; its features, GI and h_t live in the
    // context's scratch, not in this staging block
    const bool cnn = sg_policy_cnn_rnn(p);
    const int O = cnn ? p->desc.O : g.O, H = g.H, A = p->desc.A;
    const size_t rows = (size_t)T * n;
    auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    SG_CHECK(hipSetDevice(ctx->device));
    // device staging: obs | noise/action_in | action | value | logp | ent | hxs | masks | GI | h_t | h_last
    const size_t f_obs = r4(rows * O), f_na = r4(rows * A), f_row = r4(rows), f_h = r4((size_t)n * H);
    const size_t f_gi = cnn ? 0 : r4(rows * 3 * g.Hp), f_hout = cnn ? 0 : r4(rows * H);
    const size_t need = sizeof(float) * (f_obs + 2 * f_na + 4 * f_row + 2 * f_h + f_gi + f_hout);
    SG_TRY(sg_policy_io_reserve(p, need));
    float* d_obs = p->d_io;
    float* d_in = d_obs + f_obs;
    float* d_action = d_in + f_na;
    float* d_value = d_action + f_na;
    float* d_logp = d_value + f_row;
    float* d_ent = d_logp + f_row;
    float* d_masks = d_ent + f_row;
    float* d_h0 = d_masks + f_row;
    float* d_hlast = d_h0 + f_h;
    float* d_gi = d_hlast + f_h;
    float* d_hout = d_gi + f_gi;
    SG_CHECK(hipMemcpyAsync(d_obs, obs, sizeof(float) * rows * O, hipMemcpyHostToDevice, ctx->stream));
    SG_CHECK(hipMemcpyAsync(d_h0, hxs, sizeof(float) * (size_t)n * H, hipMemcpyHostToDevice, ctx->stream));
    SG_CHECK(hipMemcpyAsync(d_masks, masks, sizeof(float) * rows, hipMemcpyHostToDevice, ctx->stream));
    const float* src_in = mode == 2 ? action_in : noise;
    if (src_in) SG_CHECK(hipMemcpyAsync(d_in, src_in, sizeof(float) * rows * A, hipMemcpyHostToDevice, ctx->stream));
    if (cnn) {
        SG_TRY(sg_cnn_gru_forward_device(p, d_obs, d_h0, d_masks, T, n, mode, (mode == 0 && noise) ? d_in : nullptr, seed,
                                         mode == 2 ? d_in : nullptr, d_value, d_action, d_logp, d_ent, d_hlast));
    } else {
        SG_TRY(gru_forward_dev(p, d_obs, d_h0, d_masks, T, n, d_gi, d_hout, d_hlast));
        SG_TRY(sg_policy_forward_device(p, d_hout, (int)rows, mode, (mode == 0 && noise) ? d_in : nullptr, seed,
                                        mode == 2 ? d_in : nullptr, d_value, d_action, d_logp, d_ent));
    }
    if (value) SG_CHECK(hipMemcpyAsync(value, d_value, sizeof(float) * rows, hipMemcpyDeviceToHost, ctx->stream));
    if (action) SG_CHECK(hipMemcpyAsync(action, d_action, sizeof(float) * rows * A, hipMemcpyDeviceToHost, ctx->stream));
    if (logp) SG_CHECK(hipMemcpyAsync(logp, d_logp, sizeof(float) * rows, hipMemcpyDeviceToHost, ctx->stream));
    if (ent_rows) SG_CHECK(hipMemcpyAsync(ent_rows, d_ent, sizeof(float) * rows, hipMemcpyDeviceToHost, ctx->stream));
    if (hxs_out) SG_CHECK(hipMemcpyAsync(hxs_out, d_hlast, sizeof(float) * (size_t)n * H, hipMemcpyDeviceToHost, ctx->stream));
    SG_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

// Policy.get_value (a2c/model.py:103-105) of a recurrent policy on DEVICE inputs (sg_rollout_compute_returns_policy: slot T of a
// rollout that holds its hidden states): the three launches of sg_policy_get_value_rnn -- the same bits -- with GI, h and the value
// in the policy's staging block; nothing is copied and nothing waits (unless the block has to grow).
int sg_gru_value_device(sg_policy* p, const float* d_obs, const float* d_hxs, const float* d_masks, int n, float** d_value) {
    sg_ctx* ctx = p->ctx;
    const SgGruDesc& g = p->gru;
    auto r4 = [](size_t x) { return (x + 3) & ~(size_t)3; };
    const size_t f_row = r4((size_t)n), f_gi = r4((size_t)n * 3 * g.Hp), f_h = r4((size_t)n * g.H);
    const size_t need = sizeof(float) * (f_row + f_gi + f_h);
    SG_CHECK(hipSetDevice(ctx->device));
    SG_TRY(sg_policy_io_reserve(p, need));
    float* d_v = p->d_io;
    float* d_gi = d_v + f_row;
    float* d_hout = d_gi + f_gi;
    SG_TRY(gru_forward_dev(p, d_obs, d_hxs, d_masks, 1, n, d_gi, d_hout, nullptr));
    SG_TRY(sg_policy_forward_device(p, d_hout, n, 1, nullptr, 0, nullptr, d_v, nullptr, nullptr, nullptr));
    *d_value = d_v;
    return 0;
}

extern "C" int sg_policy_act_rnn(sg_policy* p, const float* obs, const float* hxs, const float* masks, int n, const float* noise,
                                 uint64_t seed, int deterministic, float* value, float* action, float* logp, float* hxs_out) {
    SG_REQUIRE(p && obs && hxs && masks && value && action && logp && hxs_out, "sg_policy_act_rnn: NULL argument");
    return gru_host_call(p, "sg_policy_act_rnn", obs, hxs, masks, 1, n, deterministic ? 1 : 0, noise, seed, nullptr, value, action,
                         logp, nullptr, hxs_out);
}

extern "C" int sg_policy_get_value_rnn(sg_policy* p, const float* obs, const float* hxs, const float* masks, int n, float* value) {
    SG_REQUIRE(p && obs && hxs && masks && value, "sg_policy_get_value_rnn: NULL argument");
    return gru_host_call(p, "sg_policy_get_value_rnn", obs, hxs, masks, 1, n, 1, nullptr, 0, nullptr, value, nullptr, nullptr,
                         nullptr, nullptr);
}

extern "C" int sg_policy_evaluate_rnn(sg_policy* p, const float* obs, const float* hxs, const float* masks, const float* action,
                                      int T, int n, float* value, float* logp, float* entropy, float* hxs_out) {
    SG_REQUIRE(p && obs && hxs && masks && action && value && logp && entropy && hxs_out, "sg_policy_evaluate_rnn: NULL argument");
    SG_REQUIRE(T > 0 && n > 0, "sg_policy_evaluate_rnn: T and n must be positive (got %d, %d)", T, n);
    std::vector<float> ent((size_t)T * n);
    SG_TRY(gru_host_call(p, "sg_policy_evaluate_rnn", obs, hxs, masks, T, n, 2, nullptr, 0, action, value, nullptr, logp, ent.data(),
                         hxs_out));
    double s = 0.0;
    for (size_t i = 0; i < ent.size(); ++i) s += ent[i];
    *entropy = (float)(s / (double)ent.size());
    return 0;
}
