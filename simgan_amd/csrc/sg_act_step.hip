// sg_act_step.hip -- the collection loop's environment step on the device: act on a rollout slot and fill it, in one launch.
//
// Replaces (reference, a2c/ = third_party/a2c_ppo_acktr/), per step of a2c/main_gail_dyn_ppo.py:209-236:
//   Policy.act / SplitPolicy.act                        a2c/model.py:89-101, a2c/model_split.py:70-82
//   the policy's half of RolloutStorage.insert          a2c/storage.py:70-84
#include <string.h>

#include "sg_common.h"
#include "sg_policy_fwd.hpp"
#include "sg_rng.hpp"

// One environment step of the collection loop (a2c/main_gail_dyn_ppo.py:209-236): Policy.act (a2c/model.py:89-101,
// a2c/model_split.py:70-82) on the N rows of rollout slot t, its results written where rollouts.insert (a2c/storage.py:70-84)
// puts them -- value_preds[t], actions[t], action_log_probs[t] of the DEVICE rollout -- and the actions once more into
// page-locked host memory for the environments.  ONE launch: workgroup `tile` runs every trunk on its 16*MT rows (weights staged
// per trunk, or read from global memory: GW) and then the Gaussian head, one thread per row, in k_gauss_head's arithmetic.
// The bits are those of sg_policy_act: same row tile class (fwd_tile_mt), same weight path, same head expression, the library's
// draws indexed by row * A + j on stream SG_ACT_STREAM + rank.
struct ActStepArgs {
    SgPolicyDesc d;
    const float* params;
    const float* obs;     // [n, O]: slot t of the rollout's OBS
    int n;
    int mode;             // 0 sample, 1 deterministic
    const float* noise;   // [n, A] or NULL
    uint64_t seed, stream;
    float *value, *action, *logp;   // slot t of VALUE_PREDS / ACTIONS / LOGP
    float* action_host;   // [n, A] device-visible page-locked host memory
    int wbuf_floats, ldPmax;
};

template <int MT, bool GW = false>
__global__ __launch_bounds__(256) void k_policy_act_step(ActStepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 16 * MT;
    const SgPolicyDesc& d = a.d;
    const int tid = threadIdx.x, base = blockIdx.x * R;
    float* X = smem + a.wbuf_floats;
    float* H1 = X + R * d.ldO;
    float* H2 = H1 + R * d.ldH;
    float* OUT = H2 + R * d.ldH;                       // [n_trunks][R][ldPmax]
    for (int i = tid; i < R * d.Op; i += blockDim.x) {
        const int r = i / d.Op, c = i - r * d.Op;
        const int row = base + r;
        X[r * d.ldO + c] = (row < a.n && c < d.O) ? a.obs[(size_t)row * d.O + c] : 0.f;
    }
    for (int t = 0; t < d.n_trunks; ++t) {
        const SgTrunk tr = d.trunk[t];
        __syncthreads();
        if (!GW) sg_stage(smem, a.params + tr.off, tr.size / 4);
        __syncthreads();
        trunk_forward<MT, GW>(d, tr, GW ? a.params + tr.off : smem, X, H1, H2, OUT + t * R * a.ldPmax, tr.ldP);
    }
    __syncthreads();
    const int row = base + tid;
    if (tid < R && row < a.n) {
        const float* h0 = OUT + tid * d.trunk[0].ldP;
        const float* h1 = OUT + R * a.ldPmax + tid * d.trunk[1].ldP;
        const float* hc = OUT + (d.n_trunks - 1) * R * a.ldPmax + tid * d.trunk[d.n_trunks - 1].ldP;
        a.value[row] = hc[0];
        float logp = 0.f;
        for (int k = 0; k < d.A; ++k) {
            float mean, ls;
            if (d.kind == SG_POLICY_MLP) {
                mean = h0[k];
                ls = a.params[d.trunk[0].off + d.trunk[0].ex + k];
            } else if (k < d.nc) {
                mean = h0[k];
                ls = h0[d.nc + k];
            } else {
                mean = h1[k - d.nc];
                ls = h1[d.na + k - d.nc];
            }
            const float sigma = expf(ls);
            float act;
            if (a.mode == 1) act = mean;
            else {
                const float z = a.noise ? a.noise[(size_t)row * d.A + k]
                                        : sg_normal(a.seed, a.stream, (uint64_t)row * d.A + k);
                act = z * sigma + mean;
            }
            a.action[(size_t)row * d.A + k] = act;
            a.action_host[(size_t)row * d.A + k] = act;
            const float diff = act - mean, var = sigma * sigma;
            logp += -(diff * diff) / (2.0f * var) - logf(sigma) - HALF_LOG_2PI;
        }
        a.logp[row] = logp;
    }
}

static size_t act_step_lds_bytes(const SgPolicyDesc& d, int MT, bool gw) {
    const int R = 16 * MT;
    return sizeof(float) * (size_t)((gw ? 0 : max_trunk_size(d, 0, d.n_trunks)) + R * d.ldO + 2 * R * d.ldH + d.n_trunks * R * max_ldP(d));
}

extern "C" int sg_rollout_act_step(sg_rollout* r, sg_policy* p, int t, const float* obs_host, const float* noise, uint64_t seed,
                                   int deterministic, float* action_host) {
    SG_REQUIRE(r && p && action_host, "sg_rollout_act_step: NULL argument");
    SG_REQUIRE(p->ctx == r->ctx, "sg_rollout_act_step: the policy and the rollout live on different contexts");
    SG_REQUIRE(!p->recurrent, "sg_rollout_act_step: the policy is recurrent (kind SG_POLICY_GRU) and the device rollout holds no hidden "
               "state; act through sg_policy_act_rnn and insert on the host");
    SG_REQUIRE(p->desc.dist == SG_DIST_GAUSSIAN, "sg_rollout_act_step: the policy has a Categorical / Bernoulli head; the one-launch step "
               "carries the Gaussian head only (Box action spaces)");
    SG_REQUIRE(p->desc.O == r->O && p->desc.A == r->A, "sg_rollout_act_step: policy/rollout dims differ (obs %d vs %d, action %d vs %d)",
               p->desc.O, r->O, p->desc.A, r->A);
    SG_REQUIRE(t >= 0 && t < r->T, "sg_rollout_act_step: step %d out of range [0,%d)", t, r->T);
    sg_ctx* ctx = r->ctx;
    const SgPolicyDesc& d = p->desc;
    const int n = r->N, O = d.O, A = d.A;
    const size_t f_na = (size_t)n * A;
    // the tile class and the weight path of sg_policy_act's forward launch: they decide the summation order (fwd_tile_mt)
    const bool gw = sg_policy_needs_gw(ctx, d);
    const int MTf = fwd_tile_mt(ctx, d, n, gw);
    int MT = MTf;
    while (MT > 1 && act_step_lds_bytes(d, MT, gw) > (size_t)ctx->lds_bytes - 1024) MT /= 2;
    SG_REQUIRE(act_step_lds_bytes(d, MT, gw) <= (size_t)ctx->lds_bytes && (MT == 1) == (MTf == 1),
               "sg_rollout_act_step: a %d-row tile of this policy with every trunk's head outputs (%zu B) does not fit the %d-byte "
               "LDS; act through sg_policy_act and insert on the host", 16 * MTf, act_step_lds_bytes(d, MTf, gw), ctx->lds_bytes);
    SG_CHECK(hipSetDevice(ctx->device));
    void* h_act = nullptr;
    SG_TRY(sg_ctx_pinned(ctx, sizeof(float) * f_na, &h_act));
    const bool inject = noise && !deterministic;
    if (inject && sizeof(float) * f_na > p->io_bytes) {
        const size_t need = sizeof(float) * f_na;
        SG_CHECK(hipStreamSynchronize(ctx->stream));
        if (p->d_io) SG_CHECK(sg_dev_free(p->d_io));
        p->d_io = nullptr;
        p->io_bytes = 0;
        SG_CHECK(sg_dev_malloc((void**)&p->d_io, need + need / 2));
        p->io_bytes = need + need / 2;
    }
    float* d_obs = r->d_field[SG_F_OBS] + (size_t)t * n * O;
    if (obs_host) SG_CHECK(hipMemcpyAsync(d_obs, obs_host, sizeof(float) * (size_t)n * O, hipMemcpyHostToDevice, ctx->stream));
    if (inject) SG_CHECK(hipMemcpyAsync(p->d_io, noise, sizeof(float) * f_na, hipMemcpyHostToDevice, ctx->stream));
    ActStepArgs a;
    a.d = d; a.params = p->d_params; a.obs = d_obs; a.n = n; a.mode = deterministic ? 1 : 0;
    a.noise = inject ? p->d_io : nullptr; a.seed = seed; a.stream = SG_ACT_STREAM + (uint64_t)ctx->rank;
    a.value = r->d_field[SG_F_VALUE_PREDS] + (size_t)t * n;
    a.action = r->d_field[SG_F_ACTIONS] + (size_t)t * f_na;
    a.logp = r->d_field[SG_F_LOGP] + (size_t)t * n;
    a.action_host = static_cast<float*>(h_act);
    a.wbuf_floats = gw ? 0 : max_trunk_size(d, 0, d.n_trunks); a.ldPmax = max_ldP(d);
    const int R = 16 * MT;
    const dim3 grid((n + R - 1) / R);
    const size_t lds = act_step_lds_bytes(d, MT, gw);
    if (gw) {
        if (MT == 4) hipLaunchKernelGGL((k_policy_act_step<4, true>), grid, dim3(256), lds, ctx->stream, a);
        else if (MT == 2) hipLaunchKernelGGL((k_policy_act_step<2, true>), grid, dim3(256), lds, ctx->stream, a);
        else hipLaunchKernelGGL((k_policy_act_step<1, true>), grid, dim3(256), lds, ctx->stream, a);
    } else if (MT == 4) hipLaunchKernelGGL(k_policy_act_step<4>, grid, dim3(256), lds, ctx->stream, a);
    else if (MT == 2) hipLaunchKernelGGL(k_policy_act_step<2>, grid, dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL(k_policy_act_step<1>, grid, dim3(256), lds, ctx->stream, a);
    SG_CHECK(hipGetLastError());
    SG_CHECK(hipStreamSynchronize(ctx->stream));
    memcpy(action_host, h_act, sizeof(float) * f_na);
    return 0;
}
