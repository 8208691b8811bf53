// sg_act_chain.hip -- the two policies of a hybrid-sim environment step in ONE launch: the policy that lives inside the
// environment and the learner, back to back, with the squash-and-concatenate seam between them kept on the device.
//
// Replaces (reference; a2c/ = third_party/a2c_ppo_acktr/, envs = my_pybullet_envs/), per environment step:
//   GAIL-dyn stage   envs/hopper_env_combined_policy.py:298-325, envs/laikago_env_combined_policy.py:420-438: after the physics
//                    step the fixed behaviour policy acts on the new state, the learner's observation is
//                    cat(state, tanh(a_b)), and SplitPolicy.act (a2c/model_split.py:70-82) follows in the main's loop
//                    (a2c/main_gail_dyn_ppo.py:209-236)                                               -> SG_CHAIN_INNER_FIRST
//   refinement stage envs/hopper_env_combined_policy.py:195-216, envs/laikago_env_combined_policy.py:240-268: Policy.act
//                    (a2c/model.py:89-101), then one of five saved dynamics policies, drawn per step, on
//                    cat(state, tanh(a)) before any physics                                           -> SG_CHAIN_LEARNER_FIRST
// i.e. sg_policy_act_ensemble, a host tanh and concat, and sg_rollout_act_step: two launches and two host waits, as one of each.
#include <string.h>

#include <vector>

#include "sg_act_chain.hpp"
#include "sg_common.h"
#include "sg_policy_fwd.hpp"
#include "sg_rng.hpp"

// Workgroup `tile` carries R = 16*MT rows through both networks.  The host groups the rows by ensemble member (idx is a host
// array), so a tile holds rows of ONE member, in row order, like a block of k_policy_act_ensemble: tiles[tile] = {member,
// R row numbers, -1 in the padding}.  The learner does not care which rows share its tile -- a row's MFMA products and its
// draws (indexed by the ORIGINAL row number) do not depend on its neighbours.
//   SG_CHAIN_INNER_FIRST    member on inner_obs -> OBS[t] = cat(state, squash(a_inner)), also left in LDS -> learner on it
//   SG_CHAIN_LEARNER_FIRST  learner on OBS[t] -> cat(state or OBS[t], squash(action)) in LDS -> member on it
// Each half keeps the bits of its stand-alone launch: the trunk weights staged per trunk in the same LDS region in turn (or
// read from global memory: GW -- run_trunks), the one head function (gauss_head_row), and the row tile CLASS of that launch -- a half whose
// launch would run 16-row tiles (fwd_tile_mt: two interleaved accumulators per dot product) runs its trunks 16 rows at a
// time here too (dual_*), whatever the tile of the chain.
struct ActChainArgs {
    SgPolicyDesc dl, di;  // learner, ensemble member
    const float* lparams;
    const float* iparams[SG_ENSEMBLE_MAX];
    const int* tiles;     // [n_tiles][1 + R]
    int n, order, run_learner, squash;
    int dual_l, dual_i;   // that half runs as 16-row sub-tiles
    int Os;               // width of the state part of the seam row
    const float* inner_obs;  // [n, di.O] (INNER_FIRST)
    const float* state;   // [n, Os] or NULL: inner_obs (INNER_FIRST) / OBS[t] (LEARNER_FIRST) serves
    float* obs;           // slot t of OBS, [n, dl.O]
    int lmode, imode;     // 0 sample, 1 deterministic
    const float *lnoise, *inoise;   // [n, A] or NULL
    uint64_t lseed, iseed, stream;
    float *value, *action, *logp;   // slot t of VALUE_PREDS / ACTIONS / LOGP
    float *action_host, *inner_action_host, *inner_raw_host;   // device-visible page-locked host memory; the last may be NULL
    int wbuf_floats, ldH, out_floats, ldPmax_l, ldPmax_i;
};

template <int MT, bool GW = false>
__global__ __launch_bounds__(256) void k_policy_act_chain(ActChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int R = 16 * MT;
    const SgPolicyDesc& dl = a.dl;
    const SgPolicyDesc& di = a.di;
    const int tid = threadIdx.x;
    float* XI = smem + a.wbuf_floats;                  // [R][di.ldO]
    float* XL = XI + R * di.ldO;                       // [R][dl.ldO]
    float* H1 = XL + R * dl.ldO;
    float* H2 = H1 + R * a.ldH;
    float* OUT = H2 + R * a.ldH;                       // [n_trunks][R][ldPmax] of the half that is running
    int* rows = reinterpret_cast<int*>(OUT + a.out_floats);   // [R]
    const int* tl = a.tiles + (size_t)blockIdx.x * (R + 1);
    const int k = tl[0];
    if (tid < R) rows[tid] = tl[1 + tid];
    __syncthreads();
    const float* ip = a.iparams[k];
    const int Os = a.Os;
    auto tile_row = [&](int r) { return rows[r]; };
    // The heads of a half that has just run its trunks, thread tid on local row tid (original row `row`); emit(j, act) takes the
    // actions.  The learner's also fills the rollout's value and log-prob.
    const int row = tid < R ? rows[tid] : -1;
    auto member_heads = [&](auto&& emit) {
        if (row < 0) return;
        gauss_head_row(di, ip, OUT + tid * di.trunk[0].ldP, OUT + R * a.ldPmax_i + tid * di.trunk[1].ldP, row, a.imode, a.inoise, nullptr,
                       a.iseed, a.stream, emit);
    };
    auto learner_heads = [&](auto&& emit) {
        if (row < 0) return;
        const float* hc = OUT + (dl.n_trunks - 1) * R * a.ldPmax_l + tid * dl.trunk[dl.n_trunks - 1].ldP;
        a.value[row] = hc[0];
        a.logp[row] = gauss_head_row(dl, a.lparams, OUT + tid * dl.trunk[0].ldP, OUT + R * a.ldPmax_l + tid * dl.trunk[1].ldP, row, a.lmode,
                                     a.lnoise, nullptr, a.lseed, a.stream, emit);
    };
    if (a.order == SG_CHAIN_INNER_FIRST) {
        stage_rows(XI, R, di.Op, di.ldO, a.inner_obs, di.O, tile_row);
        // the state part of the seam row: into the learner's LDS tile and into OBS[t]; the action part comes from the head
        const float* st = a.state ? a.state : a.inner_obs;
        stage_rows(XL, R, dl.Op, dl.ldO, Os, tile_row, [&](int64_t src, int c) {
            const float v = st[(size_t)src * Os + c];
            a.obs[(size_t)src * dl.O + c] = v;
            return v;
        });
        run_trunks<MT, GW>(di, ip, a.dual_i != 0, smem, XI, H1, H2, OUT, a.ldPmax_i);
        member_heads([&](int j, float act) {
            const float sq = sg_squash(act, a.squash);
            XL[tid * dl.ldO + Os + j] = sq;
            a.obs[(size_t)row * dl.O + Os + j] = sq;
            a.inner_action_host[(size_t)row * di.A + j] = sq;
            if (a.inner_raw_host) a.inner_raw_host[(size_t)row * di.A + j] = act;
        });
        if (!a.run_learner) return;
        run_trunks<MT, GW>(dl, a.lparams, a.dual_l != 0, smem, XL, H1, H2, OUT, a.ldPmax_l);
        learner_heads([&](int j, float act) {
            a.action[(size_t)row * dl.A + j] = act;
            a.action_host[(size_t)row * dl.A + j] = act;
        });
    } else {
        stage_rows(XL, R, dl.Op, dl.ldO, a.obs, dl.O, tile_row);
        const float* st = a.state ? a.state : a.obs;   // (state NULL: Os == dl.O)
        stage_rows(XI, R, di.Op, di.ldO, st, Os, tile_row);
        run_trunks<MT, GW>(dl, a.lparams, a.dual_l != 0, smem, XL, H1, H2, OUT, a.ldPmax_l);
        learner_heads([&](int j, float act) {
            a.action[(size_t)row * dl.A + j] = act;
            a.action_host[(size_t)row * dl.A + j] = act;
            XI[tid * di.ldO + Os + j] = sg_squash(act, a.squash);
        });
        run_trunks<MT, GW>(di, ip, a.dual_i != 0, smem, XI, H1, H2, OUT, a.ldPmax_i);
        member_heads([&](int j, float act) {
            a.inner_action_host[(size_t)row * di.A + j] = act;
            if (a.inner_raw_host) a.inner_raw_host[(size_t)row * di.A + j] = act;
        });
    }
}

static int chain_max(int a, int b) { return a > b ? a : b; }
static size_t chain_wbuf(const SgPolicyDesc& dl, const SgPolicyDesc& di, bool gw) {
    return gw ? 0 : (size_t)chain_max(max_trunk_size(dl, 0, dl.n_trunks), max_trunk_size(di, 0, di.n_trunks));
}
static size_t chain_out_floats(const SgPolicyDesc& dl, const SgPolicyDesc& di, int R) {
    return (size_t)R * chain_max(dl.n_trunks * max_ldP(dl), di.n_trunks * max_ldP(di));
}
static size_t chain_lds_bytes(const SgPolicyDesc& dl, const SgPolicyDesc& di, int MT, bool gw) {
    const size_t R = 16 * MT;
    return sizeof(float) * (chain_wbuf(dl, di, gw) + R * di.ldO + R * dl.ldO + 2 * R * chain_max(dl.ldH, di.ldH) + chain_out_floats(dl, di, (int)R)) +
           sizeof(int) * R;
}

extern "C" int sg_rollout_act_step_chain(sg_rollout* r, sg_policy* learner, int t, int order, sg_policy* const* members, int n_members,
                                         const int32_t* idx, const float* inner_obs_host, const float* state_host, const float* obs_host,
                                         const float* inner_noise, uint64_t inner_seed, int inner_deterministic, const float* noise,
                                         uint64_t seed, int deterministic, int squash, float* action_host, float* inner_action_host,
                                         float* inner_raw_host) {
    SG_REQUIRE(r && learner && members && idx, "sg_rollout_act_step_chain: NULL argument");
    SG_REQUIRE(order == SG_CHAIN_INNER_FIRST || order == SG_CHAIN_LEARNER_FIRST, "sg_rollout_act_step_chain: unknown order %d", order);
    const bool inner_first = order == SG_CHAIN_INNER_FIRST;
    SG_REQUIRE(inner_action_host, "sg_rollout_act_step_chain: NULL inner_action_host (the in-environment policy's action has nowhere to go)");
    SG_REQUIRE(n_members > 0 && n_members <= SG_ENSEMBLE_MAX, "sg_rollout_act_step_chain: 1..%d members, got %d", SG_ENSEMBLE_MAX, n_members);
    SG_REQUIRE(learner->ctx == r->ctx, "sg_rollout_act_step_chain: the learner and the rollout live on different contexts");
    SG_REQUIRE(!sg_policy_cnn_rnn(learner), "sg_rollout_act_step_chain: the learner has the recurrent CNN base (sg_policy_create_cnn_rnn); "
               "the chained step runs the MLP trunks only and carries no hidden state");
    SG_REQUIRE(!learner->cnn, "sg_rollout_act_step_chain: the learner has the CNN base (image observations); the chained step runs the MLP "
               "trunks only");
    SG_REQUIRE(!learner->recurrent, "sg_rollout_act_step_chain: the learner is recurrent (kind SG_POLICY_GRU); the chained step carries no "
               "hidden state: act through sg_policy_act_ensemble and sg_rollout_act_step_rnn");
    SG_REQUIRE(learner->desc.dist == SG_DIST_GAUSSIAN, "sg_rollout_act_step_chain: the learner has a Categorical / Bernoulli head; the chained "
               "step carries the Gaussian head only (Box action spaces)");
    sg_ctx* ctx = r->ctx;
    SG_REQUIRE(members[0], "sg_rollout_act_step_chain: member 0 is NULL");
    const SgPolicyDesc& dl = learner->desc;
    const SgPolicyDesc& di = members[0]->desc;
    const int n = r->N, O = r->O, A = r->A, Oi = di.O, Ai = di.A;
    SG_TRY(ens_check_members("sg_rollout_act_step_chain", "the chained step", ctx, members, n_members, idx, n));
    ActChainArgs a;
    for (int k = 0; k < SG_ENSEMBLE_MAX; ++k) a.iparams[k] = k < n_members ? members[k]->d_params : nullptr;
    SG_REQUIRE(dl.O == O && dl.A == A, "sg_rollout_act_step_chain: learner/rollout dims differ (obs %d vs %d, action %d vs %d)", dl.O, O,
               dl.A, A);
    int Os;
    if (inner_first) {
        SG_REQUIRE(inner_obs_host, "sg_rollout_act_step_chain: NULL inner_obs_host (SG_CHAIN_INNER_FIRST: what the members act on)");
        Os = O - Ai;
        SG_REQUIRE(Os > 0 && (state_host || Oi == Os), "sg_rollout_act_step_chain: dims do not add up: the learner's observation (%d) must be "
                   "state + member action (%d)%s", O, Ai, state_host ? "" : ", and without state_host the members' observation is the state");
        SG_REQUIRE(t >= 0 && t <= r->T, "sg_rollout_act_step_chain: step %d out of range [0,%d] (SG_CHAIN_INNER_FIRST; step T completes "
                   "OBS[T] only)", t, r->T);
    } else {
        Os = Oi - A;
        SG_REQUIRE(Os > 0 && (state_host || Os == O), "sg_rollout_act_step_chain: dims do not add up: the members' observation (%d) must be "
                   "state + learner action (%d)%s", Oi, A, state_host ? "" : ", and without state_host the rollout's observation is the state");
        SG_REQUIRE(t >= 0 && t < r->T, "sg_rollout_act_step_chain: step %d out of range [0,%d) (SG_CHAIN_LEARNER_FIRST)", t, r->T);
    }
    const bool run_learner = t < r->T;
    SG_REQUIRE(action_host || !run_learner, "sg_rollout_act_step_chain: NULL action_host (the learner's action has nowhere to go)");
    // Weight path and row tile class of each half's own launch (sg_rollout_act_step; sg_policy_act_ensemble): they decide the
    // summation order.  The tile classes may differ -- each half then runs in its own; the weight paths may not.
    const size_t room = (size_t)ctx->lds_bytes - 1024;
    const bool gw_l = sg_policy_needs_gw(ctx, dl);
    const bool gw_i = ens_needs_gw(ctx, di);
    SG_REQUIRE(gw_l == gw_i, "sg_rollout_act_step_chain: the learner's launch reads its weights from %s and the members' from %s; the "
               "chained step runs both halves on one weight path and would not reproduce their bits: act through sg_policy_act_ensemble "
               "and sg_rollout_act_step", gw_l ? "global memory" : "LDS", gw_i ? "global memory" : "LDS");
    const bool gw = gw_l;
    const bool dual_l = fwd_tile_mt(ctx, dl, n, gw) == 1;
    const bool dual_i = ens_tile_mt(ctx, di, n, n_members, gw) == 1;
    const int MT = (dual_l && dual_i) ? 1 : 2;
    SG_REQUIRE(chain_lds_bytes(dl, di, MT, gw) <= room, "sg_rollout_act_step_chain: a %d-row tile of both policies (%zu B) does not fit the "
               "%d-byte LDS; act through sg_policy_act_ensemble and sg_rollout_act_step", 16 * MT, chain_lds_bytes(dl, di, MT, gw),
               ctx->lds_bytes);
    // rows grouped by member, in row order, cut into tiles
    const int R = 16 * MT;
    std::vector<int> cnt(n_members, 0);
    for (int i = 0; i < n; ++i) ++cnt[idx[i]];
    int n_tiles = 0;
    std::vector<int> first(n_members, 0);
    for (int k = 0; k < n_members; ++k) { first[k] = n_tiles; n_tiles += (cnt[k] + R - 1) / R; }
    const size_t tile_ints = (size_t)n_tiles * (R + 1);
    // one page-locked block: what goes up (tiles | inner_obs | state | inner noise | noise) and what the kernel writes back
    const size_t f_na = (size_t)n * A, f_ni = (size_t)n * Ai;
    const bool inject_l = noise && !deterministic && run_learner, inject_i = inner_noise && !inner_deterministic;
    const size_t up_iobs = inner_first ? (size_t)n * Oi : 0, up_state = state_host ? (size_t)n * Os : 0;
    const size_t up_words = tile_ints + up_iobs + up_state + (inject_i ? f_ni : 0) + (inject_l ? f_na : 0);
    const size_t out_words = f_na + 2 * f_ni;
    SG_CHECK(hipSetDevice(ctx->device));
    void* h_blk = nullptr;
    SG_TRY(sg_ctx_pinned(ctx, 4 * (up_words + out_words), &h_blk));
    SG_TRY(sg_policy_io_reserve(learner, 4 * up_words));
    int* h_tiles = static_cast<int*>(h_blk);
    for (size_t i = 0; i < tile_ints; ++i) h_tiles[i] = -1;
    {
        std::vector<int> fill(n_members, 0);
        for (int k = 0; k < n_members; ++k)
            for (int u = 0; u < (cnt[k] + R - 1) / R; ++u) h_tiles[(size_t)(first[k] + u) * (R + 1)] = k;
        for (int i = 0; i < n; ++i) {
            const int k = idx[i], j = fill[k]++;
            h_tiles[(size_t)(first[k] + j / R) * (R + 1) + 1 + j % R] = i;
        }
    }
    float* h_up = static_cast<float*>(h_blk) + tile_ints;
    float* d_up = learner->d_io + tile_ints;
    const float *d_iobs = nullptr, *d_state = nullptr, *d_inoise = nullptr, *d_lnoise = nullptr;
    size_t off = 0;
    if (up_iobs) { memcpy(h_up + off, inner_obs_host, 4 * up_iobs); d_iobs = d_up + off; off += up_iobs; }
    if (up_state) { memcpy(h_up + off, state_host, 4 * up_state); d_state = d_up + off; off += up_state; }
    if (inject_i) { memcpy(h_up + off, inner_noise, 4 * f_ni); d_inoise = d_up + off; off += f_ni; }
    if (inject_l) { memcpy(h_up + off, noise, 4 * f_na); d_lnoise = d_up + off; off += f_na; }
    float* h_out = static_cast<float*>(h_blk) + up_words;
    float* d_obs = r->d_field[SG_F_OBS] + (size_t)t * n * O;
    if (!inner_first && obs_host) SG_CHECK(hipMemcpyAsync(d_obs, obs_host, sizeof(float) * (size_t)n * O, hipMemcpyHostToDevice, ctx->stream));
    SG_CHECK(hipMemcpyAsync(learner->d_io, h_blk, 4 * up_words, hipMemcpyHostToDevice, ctx->stream));
    a.dl = dl; a.di = di; a.lparams = learner->d_params; a.tiles = reinterpret_cast<const int*>(learner->d_io);
    a.n = n; a.order = order; a.run_learner = run_learner ? 1 : 0; a.squash = squash ? 1 : 0;
    a.dual_l = dual_l ? 1 : 0; a.dual_i = dual_i ? 1 : 0; a.Os = Os;
    a.inner_obs = d_iobs; a.state = d_state; a.obs = d_obs;
    a.lmode = deterministic ? 1 : 0; a.imode = inner_deterministic ? 1 : 0;
    a.lnoise = d_lnoise; a.inoise = d_inoise; a.lseed = seed; a.iseed = inner_seed; a.stream = SG_ACT_STREAM + (uint64_t)ctx->rank;
    const int ts = run_learner ? t : 0;   // (step T has no such slots: the learner half does not run and nothing is written)
    a.value = r->d_field[SG_F_VALUE_PREDS] + (size_t)ts * n;
    a.action = r->d_field[SG_F_ACTIONS] + (size_t)ts * f_na;
    a.logp = r->d_field[SG_F_LOGP] + (size_t)ts * n;
    a.action_host = h_out; a.inner_action_host = h_out + f_na; a.inner_raw_host = inner_raw_host ? h_out + f_na + f_ni : nullptr;
    a.wbuf_floats = (int)chain_wbuf(dl, di, gw); a.ldH = chain_max(dl.ldH, di.ldH); a.out_floats = (int)chain_out_floats(dl, di, R);
    a.ldPmax_l = max_ldP(dl); a.ldPmax_i = max_ldP(di);
    const dim3 grid(n_tiles);
    const size_t lds = chain_lds_bytes(dl, di, MT, gw);
    sg_dispatch_mt_gw<2>(MT, gw, [&](auto mt, auto g) {
        hipLaunchKernelGGL((k_policy_act_chain<decltype(mt)::value, decltype(g)::value>), grid, dim3(256), lds, ctx->stream, a);
    });
    SG_CHECK(hipGetLastError());
    SG_CHECK(hipStreamSynchronize(ctx->stream));
    if (run_learner) memcpy(action_host, h_out, sizeof(float) * f_na);
    memcpy(inner_action_host, h_out + f_na, sizeof(float) * f_ni);
    if (inner_raw_host) memcpy(inner_raw_host, h_out + f_na + f_ni, sizeof(float) * f_ni);
    return 0;
}
