// sg_policy.hip -- MLP / split policy forward (act / get_value / evaluate_actions) as gfx950 kernels.
// The PPO update lives in sg_ppo.hip.
//
// Replaces (reference, a2c/ = third_party/a2c_ppo_acktr/):
//   Policy.act / get_value / evaluate_actions          a2c/model.py:89-114, a2c/model_split.py:70-95
//   MLPBase.forward, SplitPolicyBaseNew.forward        a2c/model.py:255-264, a2c/model_split.py:187-198
//   DiagGaussian / StateDiagGaussianNew / FixedNormal  a2c/distributions.py:51-59,91-118, a2c/model_split.py:201-238
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sg_common.h"
#include "sg_policy_fwd.hpp"
#include "sg_rng.hpp"

// --------------------------------------------------------------------------------- forward

struct FwdArgs {
    SgPolicyDesc d;
    const float* params;
    const float* obs;     // [*, O]
    const int64_t* idx;   // optional row gather
    int n;
    float* heads;         // [n_trunks][n][hld]
    int hld;
    int wbuf_floats;
};

template <int MT, bool GW = false>
__global__ __launch_bounds__(256) void k_policy_forward(FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 16 * MT;
    const SgPolicyDesc& d = a.d;
    const SgTrunk tr = d.trunk[blockIdx.y];
    const float* W = GW ? a.params + tr.off : smem;
    float* X = smem + (GW ? 0 : a.wbuf_floats);
    float* H1 = X + R * d.ldO;
    float* H2 = H1 + R * d.ldH;
    float* OUT = H2 + R * d.ldH;
    const int ldP = tr.ldP;
    if (!GW) sg_stage(smem, a.params + tr.off, tr.size / 4);
    float* heads = a.heads + (size_t)blockIdx.y * a.n * a.hld;
    for (int base = blockIdx.x * R; base < a.n; base += gridDim.x * R) {
        __syncthreads();
        stage_rows(X, R, d.Op, d.ldO, a.obs, d.O, [&](int r) -> int64_t {
            const int row = base + r;
            return row < a.n ? (a.idx ? a.idx[row] : (int64_t)row) : -1;
        });
        __syncthreads();
        trunk_forward<MT, GW>(d, tr, W, X, H1, H2, OUT, ldP);
        __syncthreads();
        for (int i = threadIdx.x; i < R * tr.Pp; i += blockDim.x) {
            const int r = i / tr.Pp, c = i - r * tr.Pp;
            if (base + r < a.n && c < a.hld) heads[(size_t)(base + r) * a.hld + c] = OUT[r * ldP + c];
        }
    }
}

// Gaussian head: value, action (sampled / mode / given), log-prob, per-row entropy.
struct HeadArgs {
    SgPolicyDesc d;
    const float* params;
    const float* heads;
    int hld, n;
    int mode;             // 0: sample with noise (or RNG if noise NULL); 1: deterministic; 2: evaluate given action
    const float* noise;   // [n, A] or NULL
    uint64_t seed;
    uint64_t stream;      // RNG stream of this call: 'ACT\0' + data-parallel rank (every rank draws its own noise)
    const float* action_in;  // mode 2
    float *value, *action, *logp, *ent;  // any may be NULL
};

__global__ void k_gauss_head(HeadArgs a) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.n) return;
    const SgPolicyDesc& d = a.d;
    const size_t hs = (size_t)a.n * a.hld;
    const float* h0 = a.heads + (size_t)row * a.hld;
    const float* h1 = h0 + hs;
    const float* hc = a.heads + (size_t)(d.n_trunks - 1) * hs + (size_t)row * a.hld;
    if (a.value) a.value[row] = hc[0];
    if (!a.logp && !a.action && !a.ent) return;
    float ent;
    const float logp = gauss_head_row<true>(d, a.params, h0, h1, row, a.mode, a.noise, a.action_in, a.seed, a.stream, [&](int k, float act) {
        if (a.action) a.action[(size_t)row * d.A + k] = act;
    }, &ent);
    if (a.logp) a.logp[row] = logp;
    if (a.ent) a.ent[row] = ent;
}

// Categorical / Bernoulli head (a2c/distributions.py:33-88,157-168; Discrete / MultiBinary action spaces): value, action
// (sampled / mode / given), log-prob, per-row entropy from the n_out logits of the actor trunk.  One thread per row, the
// logits read in ascending k.  `noise` / the library's draws are UNIFORM in [0, 1): one per row (categorical) or per bit.
//   categorical: m = max_k z_k (first k on ties), S = sum_{k != argmax} exp(z_k - m), log p_k = (z_k - m) - log1p(S): the
//     log-prob of a near-certain class comes from the OTHER classes' mass S, not from log(1 - ...) of a rounded 1.  A sample
//     is the first k whose float32 running sum of p_k (ascending k) exceeds u, clamped to K - 1; the mode is the argmax.
//   Bernoulli: e = exp(-|z|), p = sigmoid(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e); log p(a) = a z - softplus(z) with
//     softplus(z) = max(z, 0) + log1p(e); entropy = log1p(e) + |z| e / (1 + e) (softplus(z) - p z without its
//     cancellation).  A sample is u < p, the mode z > 0 (p > 0.5).
// An action row holds the class index as a float (d.A == 1) or the n_out bits (d.A == n_out).
__global__ void k_discrete_head(HeadArgs a) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.n) return;
    const SgPolicyDesc& d = a.d;
    const size_t hs = (size_t)a.n * a.hld;
    const float* z = a.heads + (size_t)row * a.hld;
    const float* hc = a.heads + (size_t)(d.n_trunks - 1) * hs + (size_t)row * a.hld;
    if (a.value) a.value[row] = hc[0];
    if (!a.logp && !a.action && !a.ent) return;
    const int K = d.n_out;
    float logp = 0.f, ent = 0.f;
    if (d.dist == SG_DIST_CATEGORICAL) {
        float m = z[0];
        int am = 0;
        for (int k = 1; k < K; ++k)
            if (z[k] > m) { m = z[k]; am = k; }
        float S = 0.f;
        for (int k = 0; k < K; ++k)
            if (k != am) S += expf(z[k] - m);
        const float l1p = log1pf(S);
        int act = am;
        if (a.mode == 2) {
            act = (int)a.action_in[row];
            act = act < 0 ? 0 : (act > K - 1 ? K - 1 : act);   // (a class index outside [0, K) has no logit to read)
        } else if (a.mode == 0) {
            const float u = a.noise ? a.noise[row] : sg_uniform(a.seed, a.stream, (uint64_t)row);
            float cum = 0.f;
            act = K - 1;
            for (int k = 0; k < K; ++k) {
                cum += expf((z[k] - m) - l1p);
                if (cum > u) { act = k; break; }
            }
        }
        for (int k = 0; k < K; ++k) {
            const float lp = (z[k] - m) - l1p;
            ent -= expf(lp) * lp;
        }
        logp = (z[act] - m) - l1p;
        if (a.action) a.action[row] = (float)act;
    } else {
        for (int k = 0; k < K; ++k) {
            const float zk = z[k], az = fabsf(zk);
            const float e = expf(-az), l1p = log1pf(e);
            const float p = zk >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            float act;
            if (a.mode == 2) act = a.action_in[(size_t)row * K + k];
            else if (a.mode == 1) act = zk > 0.f ? 1.f : 0.f;
            else {
                const float u = a.noise ? a.noise[(size_t)row * K + k] : sg_uniform(a.seed, a.stream, (uint64_t)row * K + k);
                act = u < p ? 1.f : 0.f;
            }
            if (a.action) a.action[(size_t)row * K + k] = act;
            // a z - softplus(z), a in [0, 1] (the reference evaluates float actions as they are)
            logp += act * zk - (fmaxf(zk, 0.f) + l1p);
            ent += l1p + az * (e / (1.f + e));
        }
    }
    if (a.logp) a.logp[row] = logp;
    if (a.ent) a.ent[row] = ent;
}

// The LDS-resident kernels need a trunk's whole parameter block beside one 16-row tile; a policy that does not fit takes
// the global-weight instances (SG_POLICY_GW=1 forces them for any shape: tests).
bool sg_policy_needs_gw(const sg_ctx* ctx, const SgPolicyDesc& d) {
    const char* e = getenv("SG_POLICY_GW");
    if (e && e[0] == '1') return true;
    return fwd_lds_bytes(d, 1) > (size_t)ctx->lds_bytes - 1024;
}

// Runs all trunks forward over n rows (device obs) into ctx scratch `heads`; returns hld.
static int policy_forward_dev(sg_policy* p, const float* d_obs, const int64_t* d_idx, int n, float* d_heads, int hld) {
    sg_ctx* ctx = p->ctx;
    FwdArgs a;
    a.d = p->desc; a.params = p->d_params; a.obs = d_obs; a.idx = d_idx; a.n = n; a.heads = d_heads; a.hld = hld;
    const bool gw = sg_policy_needs_gw(ctx, p->desc);
    a.wbuf_floats = gw ? 0 : max_trunk_size(p->desc, 0, p->desc.n_trunks);
    const int MT = fwd_tile_mt(ctx, p->desc, n, gw);
    SG_REQUIRE(fwd_lds_bytes(p->desc, MT, gw) <= (size_t)ctx->lds_bytes,
               "policy forward: one 16-row activation tile (%zu B) does not fit LDS", fwd_lds_bytes(p->desc, MT, gw));
    const int R = 16 * MT;
    int gx = (n + R - 1) / R;
    if (gx > 4 * ctx->num_cu) gx = 4 * ctx->num_cu;
    dim3 grid(gx, p->desc.n_trunks);
    const size_t lds = fwd_lds_bytes(p->desc, MT, gw);
    sg_dispatch_mt_gw<4>(MT, gw, [&](auto mt, auto g) {
        hipLaunchKernelGGL((k_policy_forward<decltype(mt)::value, decltype(g)::value>), grid, dim3(256), lds, ctx->stream, a);
    });
    SG_CHECK(hipGetLastError());
    return 0;
}

int sg_policy_heads_ld(const SgPolicyDesc& d) {
    int m = 0;
    for (int t = 0; t < d.n_trunks; ++t) m = d.trunk[t].Pp > m ? d.trunk[t].Pp : m;
    return m;
}

// value / action / log-prob / entropy of n rows from the head stacks [n_trunks][n][hld] (also the last launch of the recurrent
// CNN base's forward, sg_cnn.hip)
int sg_policy_heads_device(sg_policy* p, const float* d_heads, int hld, int n, int mode, const float* d_noise, uint64_t seed,
                           const float* d_action_in, float* d_value, float* d_action, float* d_logp, float* d_ent) {
    sg_ctx* ctx = p->ctx;
    HeadArgs h;
    h.d = p->desc; h.params = p->d_params; h.heads = d_heads; h.hld = hld; h.n = n; h.mode = mode;
    h.noise = d_noise; h.seed = seed; h.stream = SG_ACT_STREAM + (uint64_t)ctx->rank; h.action_in = d_action_in;
    h.value = d_value; h.action = d_action; h.logp = d_logp; h.ent = d_ent;
    if (p->desc.dist == SG_DIST_GAUSSIAN) hipLaunchKernelGGL(k_gauss_head, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, h);
    else hipLaunchKernelGGL(k_discrete_head, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, h);
    SG_CHECK(hipGetLastError());
    return 0;
}

// Device-side entry used by the rollout code (compute_returns_policy, synthetic fill).
int sg_policy_forward_device(sg_policy* p, const float* d_obs, int n, int mode, const float* d_noise,
                             uint64_t seed, const float* d_action_in, float* d_value, float* d_action,
                             float* d_logp, float* d_ent) {
    sg_ctx* ctx = p->ctx;
    const int hld = sg_policy_heads_ld(p->desc);
    float* scratch = nullptr;
    const size_t heads_bytes = sizeof(float) * (size_t)p->desc.n_trunks * n * hld;
    if (p->cnn) {
        // the CNN base (sg_cnn.hip) fills the same head stacks, SG_CNN_FWD_ROWS rows at a time so that the activation stacks
        // behind them stay bounded whatever n is
        const int chunk = n < SG_CNN_FWD_ROWS ? n : SG_CNN_FWD_ROWS;
        SG_TRY(sg_ctx_scratch(ctx, heads_bytes + sizeof(float) * sg_cnn_fwd_floats(p->cnnd, chunk), &scratch));
        float* act = scratch + (size_t)p->desc.n_trunks * n * hld;
        for (int r0 = 0; r0 < n; r0 += chunk)
            SG_TRY(sg_cnn_forward_launch(ctx, p, d_obs + (size_t)r0 * p->desc.O, nullptr, n - r0 < chunk ? n - r0 : chunk, act, scratch, hld,
                                         r0, n));
    } else {
        SG_TRY(sg_ctx_scratch(ctx, heads_bytes, &scratch));
        SG_TRY(policy_forward_dev(p, d_obs, nullptr, n, scratch, hld));
    }
    return sg_policy_heads_device(p, scratch, hld, n, mode, d_noise, seed, d_action_in, d_value, d_action, d_logp, d_ent);
}

// ------------------------------------------------------------------------------ policy API

extern "C" int sg_policy_create(sg_ctx* ctx, int kind, int obs_dim, int act_dim, int hidden, int num_feet,
                                sg_policy** out) {
    return sg_policy_create2(ctx, kind, obs_dim, act_dim, hidden, num_feet, 0, out);
}

extern "C" int sg_policy_create2(sg_ctx* ctx, int kind, int obs_dim, int act_dim, int hidden, int num_feet, int critic_hidden,
                                 sg_policy** out) {
    return sg_policy_create3(ctx, kind, obs_dim, act_dim, hidden, num_feet, critic_hidden, SG_DIST_GAUSSIAN, 0, out);
}

// rnn_heads: a Categorical / Bernoulli head on kind SG_POLICY_GRU is admitted (sg_policy_create_rnn_dist)
static int policy_create(sg_ctx* ctx, int kind, int obs_dim, int act_dim, int hidden, int num_feet, int critic_hidden, int dist, int n_out,
                         bool rnn_heads, sg_policy** out) {
    SG_DEVICE_WIDE();
    SG_REQUIRE(ctx && out, "sg_policy_create: NULL argument");
    SG_REQUIRE(critic_hidden >= 0, "sg_policy_create2: bad critic_hidden");
    SG_REQUIRE(kind == SG_POLICY_MLP || kind == SG_POLICY_SPLIT || kind == SG_POLICY_GRU, "sg_policy_create: unknown kind %d", kind);
    SG_REQUIRE(obs_dim > 0 && act_dim > 0 && hidden > 0, "sg_policy_create: bad dims");
    SG_REQUIRE(dist == SG_DIST_GAUSSIAN || dist == SG_DIST_CATEGORICAL || dist == SG_DIST_BERNOULLI,
               "sg_policy_create3: unknown dist %d", dist);
    if (dist != SG_DIST_GAUSSIAN) {
        SG_REQUIRE(kind == SG_POLICY_MLP || (rnn_heads && kind == SG_POLICY_GRU), "sg_policy_create3: a Categorical / Bernoulli head is "
                   "built on the feed-forward Policy (kind SG_POLICY_MLP) only, not on kind %d", kind);
        SG_REQUIRE(n_out > 0 && n_out < (1 << 24), "sg_policy_create3: n_out = %d: need 0 < n_out < 2^24 (a class index travels as a "
                   "float)", n_out);
        SG_REQUIRE(act_dim == (dist == SG_DIST_CATEGORICAL ? 1 : n_out), "sg_policy_create3: act_dim (%d) must be %s", act_dim,
                   dist == SG_DIST_CATEGORICAL ? "1 for a Categorical head (an action row is one class index)"
                                               : "n_out for a Bernoulli head (an action row is n_out bits)");
    }
    if (kind == SG_POLICY_SPLIT)
        SG_REQUIRE(num_feet > 0 && act_dim == 7 * num_feet,
                   "SplitPolicy: num_outputs (%d) must equal (4+3)*num_feet (%d)", act_dim, 7 * num_feet);
    SG_CHECK(hipSetDevice(ctx->device));
    sg_policy* p = new sg_policy();
    p->ctx = ctx;
    if (kind == SG_POLICY_GRU) {
        // a2c/model.py:233-253 with recurrent=True: the trunks' first layers take the GRU state (H inputs), not the observation
        p->recurrent = true;
        // (the heads block is the feed-forward layout with obs_dim = H, whatever the head: a Categorical / Bernoulli one has no log-std)
        p->desc = sg_make_policy_desc(SG_POLICY_MLP, hidden, act_dim, hidden, 1, critic_hidden, dist, n_out);
        p->gru = sg_make_gru_desc(obs_dim, hidden, p->desc.total);
        if (!sg_gru_fits(ctx, p->gru)) {
            delete p;
            sg_set_error("sg_policy_create: one 16-row tile of this GRU (obs %d, hidden %d) does not fit the %d-byte LDS", obs_dim, hidden,
                         ctx->lds_bytes);
            return -2;
        }
    } else
        p->desc = sg_make_policy_desc(kind, obs_dim, act_dim, hidden, num_feet, critic_hidden, dist, n_out);
    // any width the reference's constructor accepts (a2c/arguments.py:107-109, a2c/model.py:233-253): a trunk that fits a
    // CU's LDS runs on the LDS-resident kernels, a larger one on the global-weight instances; only one 16-row activation
    // tile has to fit
    SG_REQUIRE(fwd_lds_bytes(p->desc, 1, true) <= (size_t)ctx->lds_bytes - 1024,
               "sg_policy_create: one 16-row activation tile of this policy (obs %d, hidden %d: %zu bytes) does not fit the %d-byte LDS",
               obs_dim, hidden, fwd_lds_bytes(p->desc, 1, true), ctx->lds_bytes);
    SG_CHECK(sg_dev_malloc((void**)&p->d_params, sizeof(float) * sg_policy_padded_count(p)));
    SG_CHECK(hipMemsetAsync(p->d_params, 0, sizeof(float) * sg_policy_padded_count(p), ctx->stream));
    *out = p;
    return 0;
}

extern "C" int sg_policy_create3(sg_ctx* ctx, int kind, int obs_dim, int act_dim, int hidden, int num_feet, int critic_hidden,
                                 int dist, int n_out, sg_policy** out) {
    return policy_create(ctx, kind, obs_dim, act_dim, hidden, num_feet, critic_hidden, dist, n_out, false, out);
}

// Policy(obs_shape, Discrete(K) | MultiBinary(n), base_kwargs={'recurrent': True}) (a2c/model.py:40-62): kind SG_POLICY_GRU with a
// Categorical / Bernoulli head.  The heads block is sg_policy_create3's MLP layout on the H-wide GRU state (no log-std, the
// n_out-wide head, an action row of 1 class index or n_out bits), the GRU block sits behind it; in the flat order the four GRU
// tensors come first and dist.linear.{weight, bias} last.  An entry point of its own: sg_policy_create3 keeps refusing the pair.
extern "C" int sg_policy_create_rnn_dist(sg_ctx* ctx, int obs_dim, int hidden, int critic_hidden, int dist, int n_out, sg_policy** out) {
    SG_REQUIRE(dist == SG_DIST_CATEGORICAL || dist == SG_DIST_BERNOULLI, "sg_policy_create_rnn_dist: dist %d: SG_DIST_CATEGORICAL or "
               "SG_DIST_BERNOULLI (the Gaussian head on the GRU base is sg_policy_create2 with kind SG_POLICY_GRU)", dist);
    return policy_create(ctx, SG_POLICY_GRU, obs_dim, dist == SG_DIST_CATEGORICAL ? 1 : n_out, hidden, 1, critic_hidden, dist, n_out, true, out);
}

extern "C" int sg_policy_destroy(sg_policy* p) {
    SG_DEVICE_WIDE();
    if (!p) return 0;
    (void)hipStreamSynchronize(p->ctx->stream);
    if (p->d_params) (void)sg_dev_free(p->d_params);
    if (p->d_io) (void)sg_dev_free(p->d_io);
    delete p;
    return 0;
}

// flat (state_dict) and padded (device) sizes of the whole policy: a recurrent one carries its GRU's four tensors FIRST in the
// flat order (base.gru.* precede base.actor.*, a2c/model.py:124-131,240-251) and BEHIND the heads' block on the device
static int64_t policy_flat_total(const sg_policy* p) {
    if (p->cnn) return p->cnnd.total + (p->recurrent ? sg_gru_flat_count(p->gru) : 0);   // the CNN base keeps the flat order on the device
    return sg_policy_flat_count(p->desc) + (p->recurrent ? sg_gru_flat_count(p->gru) : 0);
}
size_t sg_policy_padded_count(const sg_policy* p) {
    if (sg_policy_cnn_rnn(p)) return (size_t)p->gru.off + (size_t)p->gru.total;   // flat CNN block | padding to 16 bytes | GRU block
    return (size_t)p->desc.total + (p->recurrent ? (size_t)p->gru.total : 0);
}

extern "C" int sg_policy_num_params(const sg_policy* p, int64_t* n) {
    SG_REQUIRE(p && n, "sg_policy_num_params: NULL argument");
    *n = policy_flat_total(p);
    return 0;
}

extern "C" int sg_policy_set_params(sg_policy* p, const float* flat, int64_t n) {
    SG_REQUIRE(p && flat, "sg_policy_set_params: NULL argument");
    SG_REQUIRE(n == policy_flat_total(p), "sg_policy_set_params: expected %lld floats, got %lld",
               (long long)policy_flat_total(p), (long long)n);
    if (sg_policy_cnn_rnn(p)) {   // flat: the GRU's four tensors, then the CNN base's state_dict order; device: the other way round
        std::vector<float> dev(sg_policy_padded_count(p), 0.f);
        const int64_t n_gru = sg_gru_flat_count(p->gru);
        sg_gru_pad(p->gru, flat, dev.data() + p->gru.off);
        memcpy(dev.data(), flat + n_gru, sizeof(float) * (size_t)p->cnnd.total);
        SG_CHECK(hipStreamSynchronize(p->ctx->stream));
        SG_COPY_SYNC(p->ctx, p->d_params, dev.data(), sizeof(float) * dev.size(), hipMemcpyHostToDevice);
        return 0;
    }
    if (p->cnn) {
        SG_CHECK(hipStreamSynchronize(p->ctx->stream));
        SG_COPY_SYNC(p->ctx, p->d_params, flat, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
        return 0;
    }
    std::vector<float> padded(sg_policy_padded_count(p), 0.f);
    const int64_t n_gru = p->recurrent ? sg_gru_flat_count(p->gru) : 0;
    if (p->recurrent) sg_gru_pad(p->gru, flat, padded.data() + p->gru.off);
    sg_policy_pad(p->desc, flat + n_gru, padded.data());
    SG_CHECK(hipStreamSynchronize(p->ctx->stream));
    SG_COPY_SYNC(p->ctx, p->d_params, padded.data(), sizeof(float) * padded.size(), hipMemcpyHostToDevice);
    return 0;
}

extern "C" int sg_policy_get_params(sg_policy* p, float* flat, int64_t n) {
    SG_REQUIRE(p && flat, "sg_policy_get_params: NULL argument");
    SG_REQUIRE(n == policy_flat_total(p), "sg_policy_get_params: expected %lld floats, got %lld",
               (long long)policy_flat_total(p), (long long)n);
    if (sg_policy_cnn_rnn(p)) {
        std::vector<float> dev(sg_policy_padded_count(p));
        SG_CHECK(hipStreamSynchronize(p->ctx->stream));
        SG_COPY_SYNC(p->ctx, dev.data(), p->d_params, sizeof(float) * dev.size(), hipMemcpyDeviceToHost);
        const int64_t n_gru = sg_gru_flat_count(p->gru);
        sg_gru_unpad(p->gru, dev.data() + p->gru.off, flat);
        memcpy(flat + n_gru, dev.data(), sizeof(float) * (size_t)p->cnnd.total);
        return 0;
    }
    if (p->cnn) {
        SG_CHECK(hipStreamSynchronize(p->ctx->stream));
        SG_COPY_SYNC(p->ctx, flat, p->d_params, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost);
        return 0;
    }
    std::vector<float> padded(sg_policy_padded_count(p));
    SG_CHECK(hipStreamSynchronize(p->ctx->stream));
    SG_COPY_SYNC(p->ctx, padded.data(), p->d_params, sizeof(float) * padded.size(), hipMemcpyDeviceToHost);
    const int64_t n_gru = p->recurrent ? sg_gru_flat_count(p->gru) : 0;
    if (p->recurrent) sg_gru_unpad(p->gru, padded.data() + p->gru.off, flat);
    sg_policy_unpad(p->desc, padded.data(), flat + n_gru);
    return 0;
}

int sg_policy_io_reserve(sg_policy* p, size_t need) {
    if (need <= p->io_bytes) return 0;
    SG_CHECK(hipStreamSynchronize(p->ctx->stream));
    if (p->d_io) SG_CHECK(sg_dev_free(p->d_io));
    p->d_io = nullptr;
    p->io_bytes = 0;
    const size_t cap = need + need / 2;
    SG_CHECK(sg_dev_malloc((void**)&p->d_io, cap));
    p->io_bytes = cap;
    return 0;
}

// host-pointer front end shared by act / get_value / evaluate
static int policy_host_call(sg_policy* p, const float* obs, int n, int mode, const float* noise, uint64_t seed,
                            const float* action_in, float* value, float* action, float* logp, float* ent_rows) {
    sg_ctx* ctx = p->ctx;
    SG_REQUIRE(n > 0, "policy: n must be positive");
    const int O = p->desc.O, A = p->desc.A;
    SG_CHECK(hipSetDevice(ctx->device));
    // device staging: obs | noise/action_in | action | value | logp | ent
    const size_t f_obs = (size_t)n * O, f_na = (size_t)n * A;
    const size_t need = sizeof(float) * (f_obs + 2 * f_na + 3 * (size_t)n);
    SG_TRY(sg_policy_io_reserve(p, need));
    float* d_io = p->d_io;
    float* d_obs = d_io;
    float* d_in = d_obs + f_obs;
    float* d_action = d_in + f_na;
    float* d_value = d_action + f_na;
    float* d_logp = d_value + n;
    float* d_ent = d_logp + n;
    int rc = 0;
    do {
        if (hipMemcpyAsync(d_obs, obs, sizeof(float) * f_obs, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { rc = -1; break; }
        const float* src_in = mode == 2 ? action_in : noise;
        if (src_in && hipMemcpyAsync(d_in, src_in, sizeof(float) * f_na, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) { rc = -1; break; }
        rc = sg_policy_forward_device(p, d_obs, n, mode, (mode == 0 && noise) ? d_in : nullptr, seed,
                                      mode == 2 ? d_in : nullptr, d_value, d_action, d_logp, d_ent);
        if (rc) break;
        if (value && hipMemcpyAsync(value, d_value, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) { rc = -1; break; }
        if (action && hipMemcpyAsync(action, d_action, sizeof(float) * f_na, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) { rc = -1; break; }
        if (logp && hipMemcpyAsync(logp, d_logp, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) { rc = -1; break; }
        if (ent_rows && hipMemcpyAsync(ent_rows, d_ent, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) { rc = -1; break; }
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = -1; break; }
    } while (0);
    if (rc == -1) sg_set_error("policy call: HIP error: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

extern "C" int sg_policy_act(sg_policy* p, const float* obs, int n, const float* noise, uint64_t seed,
                             int deterministic, float* value, float* action, float* logp) {
    SG_REQUIRE(p && obs && value && action && logp, "sg_policy_act: NULL argument");
    SG_REQUIRE(!p->recurrent, "%s: this policy is recurrent (kind SG_POLICY_GRU); call %s_rnn with its hidden state and masks", "sg_policy_act", "sg_policy_act");
    return policy_host_call(p, obs, n, deterministic ? 1 : 0, noise, seed, nullptr, value, action, logp, nullptr);
}

extern "C" int sg_policy_get_value(sg_policy* p, const float* obs, int n, float* value) {
    SG_REQUIRE(p && obs && value, "sg_policy_get_value: NULL argument");
    SG_REQUIRE(!p->recurrent, "%s: this policy is recurrent (kind SG_POLICY_GRU); call %s_rnn with its hidden state and masks", "sg_policy_get_value", "sg_policy_get_value");
    return policy_host_call(p, obs, n, 1, nullptr, 0, nullptr, value, nullptr, nullptr, nullptr);
}


// ------------------------------------------------------------------- ensemble act
// One launch for "row i acts with policy idx[i]" over K resident weight sets of one shape.  Block (tile, k):
//   1. ranks the rows that drew policy k (a block-wide count + exclusive scan over idx, stable in row order) and
//      keeps the R = 16*MT of them that belong to its tile -- blocks past the end of policy k's rows exit;
//   2. per trunk: stages policy k's parameter block in LDS, runs the LDS-tile MFMA forward on the gathered rows;
//   3. Gaussian head per row (sample / mode), written back at the ORIGINAL row positions.
// Deterministic (no atomics); the noise of row i is indexed by i, so the result does not depend on the grouping.
struct EnsArgs {
    SgPolicyDesc d;
    const float* params[SG_ENSEMBLE_MAX];
    int K;
    const int32_t* idx;   // [n]
    const float* obs;     // [n, O]
    int n;
    int mode;             // 0 sample, 1 deterministic
    const float* noise;   // [n, A] or NULL
    uint64_t seed, stream;
    float *value, *action, *logp;
    int wbuf_floats, ldPmax;
};

template <int MT, bool GW = false>
__global__ __launch_bounds__(256) void k_policy_act_ensemble(EnsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 16 * MT;
    const SgPolicyDesc& d = a.d;
    const int tid = threadIdx.x, k = blockIdx.y, tile = blockIdx.x;
    float* X = smem + a.wbuf_floats;
    float* H1 = X + R * d.ldO;
    float* H2 = H1 + R * d.ldH;
    float* OUT = H2 + R * d.ldH;                       // [n_trunks][R][ldPmax]
    int* rows = reinterpret_cast<int*>(OUT + d.n_trunks * R * a.ldPmax);   // [R]
    int* cnt = rows + R;                               // [256] + total
    // 1. rows of policy k, ranked in row order
    const int chunk = (a.n + 255) / 256, lo = tid * chunk, hi = min(a.n, lo + chunk);
    int c = 0;
    for (int i = lo; i < hi; ++i) c += (a.idx[i] == k);
    cnt[tid] = c;
    if (tid < R) rows[tid] = -1;
    __syncthreads();
    if (tid < 64) {   // exclusive scan of the 256 counts by one wave: 4 per lane + a wave scan
        int v[4], s = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) { v[u] = cnt[4 * tid + u]; s += v[u]; }
        int inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (tid >= o) inc += t; }
        int base = inc - s;
#pragma unroll
        for (int u = 0; u < 4; ++u) { cnt[4 * tid + u] = base; base += v[u]; }
        if (tid == 63) cnt[256] = inc;
    }
    __syncthreads();
    const int total = cnt[256], first = tile * R;
    if (first >= total) return;
    const int nrows = min(R, total - first);
    {
        int rank = cnt[tid];
        for (int i = lo; i < hi; ++i)
            if (a.idx[i] == k) { if (rank >= first && rank < first + R) rows[rank - first] = i; ++rank; }
    }
    __syncthreads();
    stage_rows(X, R, d.Op, d.ldO, a.obs, d.O, [&](int r) { return rows[r]; });
    // 2. trunks
    run_trunks<MT, GW>(d, a.params[k], false, smem, X, H1, H2, OUT, a.ldPmax);
    // 3. heads
    if (tid < nrows) {
        const int row = rows[tid];
        const float* h0 = OUT + tid * d.trunk[0].ldP;
        const float* h1 = OUT + R * a.ldPmax + tid * d.trunk[1].ldP;
        const float* hc = OUT + (d.n_trunks - 1) * R * a.ldPmax + tid * d.trunk[d.n_trunks - 1].ldP;
        a.value[row] = hc[0];
        a.logp[row] = gauss_head_row(d, a.params[k], h0, h1, row, a.mode, a.noise, nullptr, a.seed, a.stream,
                                     [&](int j, float act) { a.action[(size_t)row * d.A + j] = act; });
    }
}

extern "C" int sg_policy_act_ensemble(sg_policy* const* policies, int n_policies, const int32_t* idx, const float* obs,
                                      int n, const float* noise, uint64_t seed, int deterministic, float* value,
                                      float* action, float* logp) {
    SG_REQUIRE(policies && idx && obs && value && action && logp, "sg_policy_act_ensemble: NULL argument");
    SG_REQUIRE(n_policies > 0 && n_policies <= SG_ENSEMBLE_MAX, "sg_policy_act_ensemble: 1..%d policies, got %d", SG_ENSEMBLE_MAX, n_policies);
    SG_REQUIRE(n > 0, "sg_policy_act_ensemble: n must be positive");
    sg_policy* p0 = policies[0];
    SG_REQUIRE(p0, "sg_policy_act_ensemble: NULL policy");
    sg_ctx* ctx = p0->ctx;
    const SgPolicyDesc& d = p0->desc;
    SG_TRY(ens_check_members("sg_policy_act_ensemble", "the ensemble launch", ctx, policies, n_policies, idx, n));
    EnsArgs a;
    for (int k = 0; k < n_policies; ++k) a.params[k] = policies[k]->d_params;
    SG_CHECK(hipSetDevice(ctx->device));
    const int O = d.O, A = d.A;
    // device staging in the first member's io buffer: obs | noise | action | value | logp | idx
    const size_t f_obs = (size_t)n * O, f_na = (size_t)n * A;
    SG_TRY(sg_policy_io_reserve(p0, sizeof(float) * (f_obs + 2 * f_na + 3 * (size_t)n)));
    float* d_obs = p0->d_io;
    float* d_noise = d_obs + f_obs;
    float* d_action = d_noise + f_na;
    float* d_value = d_action + f_na;
    float* d_logp = d_value + n;
    int32_t* d_idx = reinterpret_cast<int32_t*>(d_logp + n);
    SG_CHECK(hipMemcpyAsync(d_obs, obs, sizeof(float) * f_obs, hipMemcpyHostToDevice, ctx->stream));
    SG_CHECK(hipMemcpyAsync(d_idx, idx, sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    if (noise && !deterministic) SG_CHECK(hipMemcpyAsync(d_noise, noise, sizeof(float) * f_na, hipMemcpyHostToDevice, ctx->stream));
    a.d = d; a.K = n_policies; a.idx = d_idx; a.obs = d_obs; a.n = n; a.mode = deterministic ? 1 : 0;
    a.noise = (noise && !deterministic) ? d_noise : nullptr; a.seed = seed; a.stream = SG_ACT_STREAM + (uint64_t)ctx->rank;
    a.value = d_value; a.action = d_action; a.logp = d_logp;
    const bool gw = ens_needs_gw(ctx, d);
    a.wbuf_floats = gw ? 0 : max_trunk_size(d, 0, d.n_trunks); a.ldPmax = max_ldP(d);
    const int MT = ens_tile_mt(ctx, d, n, n_policies, gw);
    SG_REQUIRE(ens_lds_bytes(d, MT, gw) <= (size_t)ctx->lds_bytes, "sg_policy_act_ensemble: an activation tile does not fit LDS (%zu B)", ens_lds_bytes(d, MT, gw));
    const int R = 16 * MT;
    const dim3 grid((n + R - 1) / R, n_policies);
    const size_t lds_e = ens_lds_bytes(d, MT, gw);
    sg_dispatch_mt_gw<2>(MT, gw, [&](auto mt, auto g) {
        hipLaunchKernelGGL((k_policy_act_ensemble<decltype(mt)::value, decltype(g)::value>), grid, dim3(256), lds_e, ctx->stream, a);
    });
    SG_CHECK(hipGetLastError());
    SG_CHECK(hipMemcpyAsync(value, d_value, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    SG_CHECK(hipMemcpyAsync(action, d_action, sizeof(float) * f_na, hipMemcpyDeviceToHost, ctx->stream));
    SG_CHECK(hipMemcpyAsync(logp, d_logp, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    SG_CHECK(hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" int sg_policy_evaluate(sg_policy* p, const float* obs, const float* action, int n, float* value,
                                  float* logp, float* entropy) {
    SG_REQUIRE(p && obs && action && value && logp && entropy, "sg_policy_evaluate: NULL argument");
    SG_REQUIRE(!p->recurrent, "%s: this policy is recurrent (kind SG_POLICY_GRU); call %s_rnn with its hidden state and masks", "sg_policy_evaluate", "sg_policy_evaluate");
    std::vector<float> ent(n);
    SG_TRY(policy_host_call(p, obs, n, 2, nullptr, 0, action, value, nullptr, logp, ent.data()));
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += ent[i];
    *entropy = (float)(s / n);
    return 0;
}
