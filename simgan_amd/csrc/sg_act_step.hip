// sg_act_step.hip -- the collection loop's environment step on the device: act on a rollout slot and fill it, in one launch.
//
// Replaces (reference, a2c/ = third_party/a2c_ppo_acktr/), per step of a2c/main_gail_dyn_ppo.py:209-236:
//   Policy.act / SplitPolicy.act                        a2c/model.py:89-101, a2c/model_split.py:70-82
//   the policy's half of RolloutStorage.insert          a2c/storage.py:70-84
#include <string.h>

#include "sg_common.h"
#include "sg_gru_kernels.hpp"
#include "sg_policy_fwd.hpp"
#include "sg_rng.hpp"

// One environment step of the collection loop (a2c/main_gail_dyn_ppo.py:209-236): Policy.act (a2c/model.py:89-101,
// a2c/model_split.py:70-82) on the N rows of rollout slot t, its results written where rollouts.insert (a2c/storage.py:70-84)
// puts them -- value_preds[t], actions[t], action_log_probs[t] of the DEVICE rollout -- and the actions once more into
// page-locked host memory for the environments.  ONE launch: workgroup `tile` runs every trunk on its 16*MT rows (weights staged
// per trunk, or read from global memory: GW -- run_trunks) and then the Gaussian head, one thread per row (gauss_head_row).
// The bits are those of sg_policy_act: same row tile class (fwd_tile_mt), same weight path, the same head function, the library's
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
    stage_rows(X, R, d.Op, d.ldO, a.obs, d.O, [&](int r) { return base + r < a.n ? base + r : -1; });
    run_trunks<MT, GW>(d, a.params, false, smem, X, H1, H2, OUT, a.ldPmax);
    const int row = base + tid;
    if (tid < R && row < a.n) {
        const float* h0 = OUT + tid * d.trunk[0].ldP;
        const float* h1 = OUT + R * a.ldPmax + tid * d.trunk[1].ldP;
        const float* hc = OUT + (d.n_trunks - 1) * R * a.ldPmax + tid * d.trunk[d.n_trunks - 1].ldP;
        a.value[row] = hc[0];
        a.logp[row] = gauss_head_row(d, a.params, h0, h1, row, a.mode, a.noise, nullptr, a.seed, a.stream, [&](int k, float act) {
            a.action[(size_t)row * d.A + k] = act;
            a.action_host[(size_t)row * d.A + k] = act;
        });
    }
}

// What both steps do before their launch, into the fields that ActStepArgs and ActStepRnnArgs share: the page-locked block
// the kernel writes the actions to, injected noise uploaded through the policy's staging block, the head's mode and draws,
// slot t of the rollout's VALUE_PREDS / ACTIONS / LOGP.
template <typename Args>
static int act_step_open(sg_rollout* r, sg_policy* p, int t, const float* noise, uint64_t seed, int deterministic, Args* a) {
    sg_ctx* ctx = r->ctx;
    const int n = r->N;
    const size_t f_na = (size_t)n * p->desc.A;
    SG_CHECK(hipSetDevice(ctx->device));
    void* h_act = nullptr;
    SG_TRY(sg_ctx_pinned(ctx, sizeof(float) * f_na, &h_act));
    const bool inject = noise && !deterministic;
    if (inject) {
        SG_TRY(sg_policy_io_reserve(p, sizeof(float) * f_na));
        SG_CHECK(hipMemcpyAsync(p->d_io, noise, sizeof(float) * f_na, hipMemcpyHostToDevice, ctx->stream));
    }
    a->n = n; a->mode = deterministic ? 1 : 0;
    a->noise = inject ? p->d_io : nullptr; a->seed = seed; a->stream = SG_ACT_STREAM + (uint64_t)ctx->rank;
    a->value = r->d_field[SG_F_VALUE_PREDS] + (size_t)t * n;
    a->action = r->d_field[SG_F_ACTIONS] + (size_t)t * f_na;
    a->logp = r->d_field[SG_F_LOGP] + (size_t)t * n;
    a->action_host = static_cast<float*>(h_act);
    return 0;
}
// ... and after it: wait for the step and hand the actions to the caller
static int act_step_close(sg_ctx* ctx, const float* h_act, size_t f_na, float* action_host) {
    SG_CHECK(hipGetLastError());
    SG_CHECK(hipStreamSynchronize(ctx->stream));
    memcpy(action_host, h_act, sizeof(float) * f_na);
    return 0;
}

static size_t act_step_lds_bytes(const SgPolicyDesc& d, int MT, bool gw) {
    const int R = 16 * MT;
    return sizeof(float) * (size_t)((gw ? 0 : max_trunk_size(d, 0, d.n_trunks)) + R * d.ldO + 2 * R * d.ldH + d.n_trunks * R * max_ldP(d));
}

extern "C" int sg_rollout_act_step(sg_rollout* r, sg_policy* p, int t, const float* obs_host, const float* noise, uint64_t seed,
                                   int deterministic, float* action_host) {
    SG_REQUIRE(r && p && action_host, "sg_rollout_act_step: NULL argument");
    SG_REQUIRE(p->ctx == r->ctx, "sg_rollout_act_step: the policy and the rollout live on different contexts");
    SG_REQUIRE(!sg_policy_cnn_rnn(p), "sg_rollout_act_step: the policy has the recurrent CNN base (sg_policy_create_cnn_rnn); the "
               "one-launch step runs the MLP trunks only: act through sg_policy_act_rnn and upload the step");
    SG_REQUIRE(!p->cnn, "sg_rollout_act_step: the policy has the CNN base (image observations); the one-launch step runs the MLP "
               "trunks only: act through sg_policy_act and upload the step");
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
    ActStepArgs a;
    SG_TRY(act_step_open(r, p, t, noise, seed, deterministic, &a));
    float* d_obs = r->d_field[SG_F_OBS] + (size_t)t * n * O;
    if (obs_host) SG_CHECK(hipMemcpyAsync(d_obs, obs_host, sizeof(float) * (size_t)n * O, hipMemcpyHostToDevice, ctx->stream));
    a.d = d; a.params = p->d_params; a.obs = d_obs;
    a.wbuf_floats = gw ? 0 : max_trunk_size(d, 0, d.n_trunks); a.ldPmax = max_ldP(d);
    const int R = 16 * MT;
    const dim3 grid((n + R - 1) / R);
    const size_t lds = act_step_lds_bytes(d, MT, gw);
    sg_dispatch_mt_gw<4>(MT, gw, [&](auto mt, auto g) {
        hipLaunchKernelGGL((k_policy_act_step<decltype(mt)::value, decltype(g)::value>), grid, dim3(256), lds, ctx->stream, a);
    });
    return act_step_close(ctx, a.action_host, f_na, action_host);
}

// ------------------------------------------------------------------------------------------------ recurrent policy
// The same step for a recurrent policy (kind SG_POLICY_GRU), hidden state included.  Replaces, per step:
//   Policy.act with recurrent=True                      a2c/model.py:89-101, 117-201, 255-264
//   the policy's half of RolloutStorage.insert          a2c/storage.py:70-84 (recurrent_hidden_states[step + 1] too)
// i.e. sg_policy_act_rnn's four launches (k_gru_inproj, k_gru_scan_fwd with T = 1, k_policy_forward, k_gauss_head) and its
// eight copies, as ONE launch on the rollout's own slots.  Workgroup `tile` owns R = 16*MT environments and runs four phases;
// the GRU phases work through the tile in chunks of 16*mc rows (mc == MT unless the GI tile would not fit):
//   1  stage the chunk's observations and h[t] * masks[t] (h[t]: hidden slot t), zero in the padding
//   2  GI = X W_ih^T + b_ih into LDS: every 16x16 tile one <1, 1> MFMA chain, as k_gru_inproj forms it
//   3  one GRU cell step per 16-row sub-tile in k_gru_scan_fwd's arithmetic; h goes (unmasked) to hidden slot t + 1 and into the
//      LDS tile that is the trunks' input
//   4  the trunks and the Gaussian head, as k_policy_act_step
// Every phase takes the weight path -- LDS image staged for the phase, or global memory -- that its launch of sg_policy_act_rnn
// takes (gwp: sg_gru_proj_lds, gws: sg_gru_scan_lds, GW: sg_policy_needs_gw; they can disagree), and the trunks the same row
// tile class, so value, action, log-prob and new state have sg_policy_act_rnn's bits.
// LDS: [weights of the phase][XT: R x ldH, the trunks' input][phases 1-3: X | HM | GI of one chunk  /  phase 4: H1 | H2 | OUT].
struct ActStepRnnArgs {
    SgPolicyDesc d;       // the heads on h (O == H)
    SgGruDesc g;
    const float* params;  // the policy's parameter vector (heads block first)
    const float* gruW;    // its GRU block
    const float* obs;     // [n, O]: slot t of OBS
    const float* masks;   // [n]: slot t of MASKS
    const float* hin;     // [n, H]: hidden slot t
    float* hout;          // [n, H]: hidden slot t + 1
    int n;
    int mode;             // 0 sample, 1 deterministic
    const float* noise;   // [n, A] or NULL
    uint64_t seed, stream;
    float *value, *action, *logp;   // slot t of VALUE_PREDS / ACTIONS / LOGP
    float* action_host;   // [n, A] device-visible page-locked host memory
    int wbuf_floats, ldPmax;
    int mc;               // 16-row sub-tiles per chunk of the GRU phases
    int gwp, gws;         // input projection / cell step read their weights from global memory
};

template <int MT, bool GW = false>
__global__ __launch_bounds__(256) void k_policy_act_step_rnn(ActStepRnnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 16 * MT;
    const SgPolicyDesc& d = a.d;
    const SgGruDesc& g = a.g;
    const int tid = threadIdx.x, base = blockIdx.x * R;
    const int wave = tid >> 6, nw = blockDim.x >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
    const int Hp = g.Hp, ldH = g.ldH, H = g.H, G3 = 3 * g.Hp, ldG = G3 + 4;
    float* XT = smem + a.wbuf_floats;                  // [R][d.ldO]: h_{t+1}, the trunks' input
    float* U = XT + R * d.ldO;
    const int RC = 16 * a.mc;
    float* XO = U;                                     // [RC][g.ldO]
    float* HM = XO + RC * g.ldO;                       // [RC][ldH]: h[t] * masks[t]
    float* GI = HM + RC * ldH;                         // [RC][ldG]
    const float* bih = a.gruW + g.bih;
    const float* bhh = a.gruW + g.bhh;
    for (int c0 = 0; c0 < MT; c0 += a.mc) {
        const int cbase = base + 16 * c0;              // first environment of the chunk
        __syncthreads();
        auto chunk_row = [&](int r) { return cbase + r < a.n ? cbase + r : -1; };
        stage_rows(XO, RC, g.Op, g.ldO, a.obs, g.O, chunk_row);
        stage_rows(HM, RC, ldH, ldH, H, chunk_row, [&](int64_t row, int c) { return a.hin[(size_t)row * H + c] * a.masks[row]; });
        if (!a.gwp) sg_stage(smem, a.gruW + g.wih, (3 * Hp * g.ldO) / 4);
        __syncthreads();
        {
            const float* W = a.gwp ? a.gruW + g.wih : smem;
            const int ntl = G3 >> 4;
            for (int u = wave; u < a.mc * ntl; u += nw) {
                const int i = u / ntl, tn = u - i * ntl;
                f32x4 acc[1][1];
                sg_acc_zero(acc);
                if (a.gwp) sg_mma_nt_g<1, 1>(XO + i * 16 * g.ldO, g.ldO, W + (size_t)tn * 16 * g.ldO, g.ldO, g.Op, acc);
                else sg_mma_nt<1, 1>(XO + i * 16 * g.ldO, g.ldO, W + tn * 16 * g.ldO, g.ldO, g.Op, acc);
                sg_tile_foreach(acc[0][0], i * 16, tn * 16, [&](int r, int c, float v) { GI[r * ldG + c] = v + bih[c]; });
            }
        }
        __syncthreads();
        if (!a.gws) sg_stage(smem, a.gruW + g.whh, (3 * Hp * ldH) / 4);
        __syncthreads();
        {
            const float* W = a.gws ? a.gruW + g.whh : smem;
            const int ntl = Hp >> 4;
            for (int u = wave; u < a.mc * ntl; u += nw) {
                const int i = u / ntl, tn = u - i * ntl;
                const int c = tn * 16 + li;
                const float* cur = HM + i * 16 * ldH;
                float gir[4], giz[4], gin[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int lr = i * 16 + 4 * lq + r;
                    const bool live = cbase + lr < a.n;
                    const float* gp = GI + lr * ldG + c;
                    gir[r] = live ? gp[0] : 0.f;
                    giz[r] = live ? gp[Hp] : 0.f;
                    gin[r] = live ? gp[2 * Hp] : 0.f;
                }
                const float br = bhh[c], bz = bhh[Hp + c], bn = bhh[2 * Hp + c];
                f32x4 ar[1][1], az[1][1], an[1][1];
                sg_acc_zero(ar); sg_acc_zero(az); sg_acc_zero(an);
                if (a.gws) {
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
                    const int lr = i * 16 + 4 * lq + r, row = cbase + lr;
                    const float hm = HM[lr * ldH + c];
                    const float hn = an[0][0][r] + bn;
                    const float rg = sg_sigmoid(gir[r] + (ar[0][0][r] + br));
                    const float zg = sg_sigmoid(giz[r] + (az[0][0][r] + bz));
                    const float ng = sg_tanh(gin[r] + rg * hn);
                    const float h = (1.f - zg) * ng + zg * hm;
                    const bool real = row < a.n && c < H;
                    XT[(16 * c0 + lr) * d.ldO + c] = real ? h : 0.f;
                    if (real) a.hout[(size_t)row * H + c] = h;
                }
            }
        }
    }
    float* H1 = U;
    float* H2 = H1 + R * d.ldH;
    float* OUT = H2 + R * d.ldH;                       // [n_trunks][R][ldPmax]
    run_trunks<MT, GW>(d, a.params, false, smem, XT, H1, H2, OUT, a.ldPmax);
    const int row = base + tid;
    if (tid < R && row < a.n) {
        const float* h0 = OUT + tid * d.trunk[0].ldP;
        const float* hc = OUT + (d.n_trunks - 1) * R * a.ldPmax + tid * d.trunk[d.n_trunks - 1].ldP;
        a.value[row] = hc[0];
        // (the heads of a recurrent policy are an MLP policy's: no second actor trunk for h1 to point at)
        a.logp[row] = gauss_head_row(d, a.params, h0, nullptr, row, a.mode, a.noise, nullptr, a.seed, a.stream, [&](int k, float act) {
            a.action[(size_t)row * d.A + k] = act;
            a.action_host[(size_t)row * d.A + k] = act;
        });
    }
}

static size_t act_step_rnn_wbuf(const SgPolicyDesc& d, const SgGruDesc& g, bool gwp, bool gws, bool gw) {
    size_t w = gw ? 0 : (size_t)max_trunk_size(d, 0, d.n_trunks);
    if (!gwp && (size_t)3 * g.Hp * g.ldO > w) w = (size_t)3 * g.Hp * g.ldO;
    if (!gws && (size_t)3 * g.Hp * g.ldH > w) w = (size_t)3 * g.Hp * g.ldH;
    return w;
}
static size_t act_step_rnn_lds_bytes(const SgPolicyDesc& d, const SgGruDesc& g, int MT, int mc, bool gwp, bool gws, bool gw) {
    const size_t R = 16 * MT, RC = 16 * mc;
    const size_t gru = RC * (size_t)(g.ldO + g.ldH + 3 * g.Hp + 4);
    const size_t trunks = 2 * R * d.ldH + d.n_trunks * R * max_ldP(d);
    return sizeof(float) * (act_step_rnn_wbuf(d, g, gwp, gws, gw) + R * d.ldO + (gru > trunks ? gru : trunks));
}

extern "C" int sg_rollout_act_step_rnn(sg_rollout* r, sg_policy* p, int t, const float* obs_host, const float* masks_host,
                                       const float* noise, uint64_t seed, int deterministic, float* action_host) {
    SG_REQUIRE(r && p && action_host, "sg_rollout_act_step_rnn: NULL argument");
    SG_REQUIRE(p->ctx == r->ctx, "sg_rollout_act_step_rnn: the policy and the rollout live on different contexts");
    SG_REQUIRE(!sg_policy_cnn_rnn(p), "sg_rollout_act_step_rnn: the policy has the recurrent CNN base (sg_policy_create_cnn_rnn), "
               "which the one-launch steps do not serve (an image rollout holds no hidden states on the device): act through "
               "sg_policy_act_rnn and upload the step");
    SG_REQUIRE(!p->cnn, "sg_rollout_act_step_rnn: the policy has the CNN base (image observations), which is feed-forward and not "
               "served by the one-launch steps: act through sg_policy_act and upload the step");
    SG_REQUIRE(p->recurrent, "sg_rollout_act_step_rnn: the policy is feed-forward (kind %d); act through sg_rollout_act_step",
               p->desc.kind);
    SG_REQUIRE(p->desc.dist == SG_DIST_GAUSSIAN, "sg_rollout_act_step_rnn: the recurrent policy has a %s head; the one-launch recurrent "
               "step carries the Gaussian head only (Box action spaces): act through sg_policy_act_rnn and insert on the host",
               p->desc.dist == SG_DIST_CATEGORICAL ? "Categorical" : "Bernoulli");
    SG_REQUIRE(r->d_hidden, "sg_rollout_act_step_rnn: the rollout holds no hidden states; call sg_rollout_enable_hidden first");
    SG_REQUIRE(r->hidden_dim == p->gru.H, "sg_rollout_act_step_rnn: the rollout's hidden states are %d wide, the policy's %d",
               r->hidden_dim, p->gru.H);
    SG_REQUIRE(p->gru.O == r->O && p->desc.A == r->A, "sg_rollout_act_step_rnn: policy/rollout dims differ (obs %d vs %d, action %d vs %d)",
               p->gru.O, r->O, p->desc.A, r->A);
    SG_REQUIRE(t >= 0 && t < r->T, "sg_rollout_act_step_rnn: step %d out of range [0,%d)", t, r->T);
    SG_REQUIRE(!r->mirrors_set, "sg_rollout_act_step_rnn: the rollout is mirror-augmented (sg_rollout_set_mirrors): its mirrored "
               "columns have no hidden states of their own; act through sg_policy_act_rnn and insert on the host");
    sg_ctx* ctx = r->ctx;
    const SgPolicyDesc& d = p->desc;
    const SgGruDesc& g = p->gru;
    const int n = r->N, O = g.O, A = d.A, H = g.H;
    const size_t f_na = (size_t)n * A;
    // the weight path of each of sg_policy_act_rnn's launches (sg_gru_forward_launch, policy_forward_dev) and the row tile class
    // of its trunks: they decide the summation order
    const size_t room = (size_t)ctx->lds_bytes - 1024;
    const bool gwp = sg_gru_force_gw() || sg_gru_proj_lds(g, 1, false) > room;
    const bool gws = sg_gru_force_gw() || sg_gru_scan_lds(g, false) > room;
    const bool gw = sg_policy_needs_gw(ctx, d);
    const int MTf = fwd_tile_mt(ctx, d, n, gw);
    int MT = MTf;
    while (MT > 1 && act_step_rnn_lds_bytes(d, g, MT, 1, gwp, gws, gw) > room) MT /= 2;
    int mc = MT;
    while (mc > 1 && act_step_rnn_lds_bytes(d, g, MT, mc, gwp, gws, gw) > room) mc /= 2;
    SG_REQUIRE(act_step_rnn_lds_bytes(d, g, MT, mc, gwp, gws, gw) <= (size_t)ctx->lds_bytes && (MT == 1) == (MTf == 1),
               "sg_rollout_act_step_rnn: a %d-row tile of this policy with its GRU step and every trunk's head outputs (%zu B) does not fit "
               "the %d-byte LDS; act through sg_policy_act_rnn and insert on the host", 16 * MTf,
               act_step_rnn_lds_bytes(d, g, MTf, 1, gwp, gws, gw), ctx->lds_bytes);
    ActStepRnnArgs a;
    SG_TRY(act_step_open(r, p, t, noise, seed, deterministic, &a));
    float* d_obs = r->d_field[SG_F_OBS] + (size_t)t * n * O;
    float* d_masks = r->d_field[SG_F_MASKS] + (size_t)t * n;
    if (obs_host) SG_CHECK(hipMemcpyAsync(d_obs, obs_host, sizeof(float) * (size_t)n * O, hipMemcpyHostToDevice, ctx->stream));
    if (masks_host) SG_CHECK(hipMemcpyAsync(d_masks, masks_host, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    a.d = d; a.g = g; a.params = p->d_params; a.gruW = p->d_params + g.off; a.obs = d_obs; a.masks = d_masks;
    a.hin = r->d_hidden + (size_t)t * n * H; a.hout = r->d_hidden + (size_t)(t + 1) * n * H;
    a.wbuf_floats = (int)act_step_rnn_wbuf(d, g, gwp, gws, gw); a.ldPmax = max_ldP(d);
    a.mc = mc; a.gwp = gwp ? 1 : 0; a.gws = gws ? 1 : 0;
    const int R = 16 * MT;
    const dim3 grid((n + R - 1) / R);
    const size_t lds = act_step_rnn_lds_bytes(d, g, MT, mc, gwp, gws, gw);
    sg_dispatch_mt_gw<4>(MT, gw, [&](auto mt, auto w) {
        hipLaunchKernelGGL((k_policy_act_step_rnn<decltype(mt)::value, decltype(w)::value>), grid, dim3(256), lds, ctx->stream, a);
    });
    return act_step_close(ctx, a.action_host, f_na, action_host);
}
