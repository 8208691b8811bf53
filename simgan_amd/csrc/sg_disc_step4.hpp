// sg_disc_step4.hpp -- one discriminator optimizer step as ONE launch: k_disc_chain4's row blocks and k_disc_wgrad's tile /
// vector blocks side by side, joined by a one-way hand-off inside the launch.
//
// Why (round 4, measured with bodies removed, ms per update -> us per step): two EMPTY dependent launches cost a step 3.8 us,
// the chain blocks add 3.3 and the weight-gradient blocks 2.9 -- of which ~1 us is the first-touch latency of a freshly
// launched block and ~1 us the transfer of 64 KB of operands the other XCDs have just written back.  A step is
//     weights(k) -> chain -> operand stacks -> weight gradient + Adam -> weights(k+1),
// two all-to-all edges.  Putting BOTH inside a persistent launch loses (tools/pstep_probe.py: 11 us per step with no
// compute at all: two polled hand-offs cost more than two launch boundaries).  Putting only the FIRST edge inside wins:
//   * the weight-gradient blocks are resident from the start of the launch: their code is fetched, their tile's parameter
//     and moments and the Adam scalars are in registers, and they sit in a poll loop when the chain ends;
//   * the chain blocks publish their rows of the operand stacks with write-through (`sc1`) stores, drain them, and raise one
//     flag word each (the Adam step number: monotonic, never reset inside an epoch or across replays of the epoch's graph);
//     the other side polls the words with coalesced L1-bypassing loads -- in a tile workgroup wave 7 the 8G BCE flags and
//     wave 6 the 4G mixup flags, each telling the other waves through an LDS word of its own -- and then reads its two
//     operand slabs with `sc1` loads (MI355X: write-through stores + sc1 loads are the cross-XCD-coherent pair);
//   * the dependence is ONE-WAY -- no chain block ever waits for anything -- so whatever the dispatcher does (blocks are
//     dispatched in index order, the chain blocks first) the launch cannot deadlock on residency; the spin is bounded by the
//     wall clock all the same and a time-out is reported through an error word the host reads at its next synchronisation;
//   * the second edge (new weights -> the next step's chain blocks) stays a launch boundary, which is also what keeps every
//     L2 coherent for the plain loads of the next launch.
// Arithmetic, summation order and stores are those of the two-launch step: results are bit-identical at every batch size
// (tests/test_gpu_parity.py, tests/test_gpu_step4_detect.py).
//
// Anatomy of the hand-off in a tile workgroup (north-star shape, ns after the first chain block starts, medians of the stamp
// build; before -> now): the last mixup flag is stored at 4410 -> 4360; the mixup operands are requested at ~5840 (behind a
// barrier, the BCE half's loads and one poll queued behind them) -> 5540 (wave 6 sees the flags at 5330, the other waves its
// LDS word); all operands contracted at 6500 -> 5970.  Polls in flight on the mixup flags (SG_STEP4_POLLS = k), device
// clock per step incl. the epoch's row copy, three alternations on one box: before 8.67-8.80 us; k = 1: 8.51-8.54;
// k = 2: 8.55-8.58; k = 3: 8.60-8.62.  The polling wave of its own and the LDS words are the gain; every further poll in
// flight costs ~0.04 us (91 workgroups x 32 lines x k reads per round trip queue in front of the chain's write-through stores,
// as round 4's four polls on all 96 lines did), so k = 1 ships.
//
// Round 5 tried the hand-off WITHOUT flags (every operand word poisoned one launch ahead and validated by its reader, no drain, no
// flag: `SG_STEP4_POISON`): measured negative (profiles/r05_step4_poison_handoff_negative.txt) and removed from the library in
// round 6 (git show 9df2324:simgan_amd/csrc/sg_disc_step4.hpp has it).
//
// The kernel carries no build switches.  The experiment switches of rounds 3-6 (ablations of the waits and of the chain's
// publication, a re-read verifier of the operands, the hand-off without its drain, the poll without its sleep, the store and
// load flavours below) were measured and removed; `git show b28af2c:simgan_amd/csrc/sg_disc_step4.hpp` has them.  The one
// diagnostic that is still of use, the wall-clock stamps behind tools/step4_times.py, is tools/diag/step4_stamps.patch.
#pragma once

struct Step4Args {          // not preloaded: read by the workgroups that copy the next step's rows and by one vector lane at its end
    PregatherArgs next;
    double* loss_acc;
};

// (SG_STEP4_FLAG_WORD0 / _MAX_FLAGS / _FLAG_STRIDE / _ERR_WORD / _STATE_BYTES: sg_common.h, next to sg_disc::d_state)
#define SG_STEP4_TIMEOUT_TICKS 300000000ll   // 3 s of the 100 MHz wall clock

__device__ __forceinline__ float sg_ld_sc1(__amdgpu_buffer_rsrc_t r, int byte_off) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 16 /* sc1: served past this CU's L1 */));
}
// The tile workgroups read the operand stacks with it too once the flags are up: past this XCD's L2, so every tile workgroup
// pulls its 64 KB through the fabric.  A/B, round 5, against plain loads (the 13 tiles of an XCD share a 32 KB slab through
// its L2) and sc0 loads: measured and removed; `git show b28af2c:simgan_amd/csrc/sg_disc_step4.hpp` has the switch.

// One wave waits until the flags of workgroups [lo, hi) all hold `want`; false on time-out.
// Measured and removed, round 4 (north-star, ms per update; 26.19-26.24 with this plain loop):
//  * FOUR polls kept in flight per waiting wave, issued 0.15 us apart and examined oldest first (asm loads + `s_waitcnt
//    vmcnt(6)`: the compiler's wait-count pass drains such a pipe every fourth poll): 27.59 -- 91 waiting workgroups x 96 flag
//    lines x 4 is traffic the chain blocks' write-through stores and the flags themselves queue behind (stores drained 0.3 us
//    later, flags seen 1.28 us after the last one was raised instead of 0.96);
//  * ONE sentinel flag per waiting workgroup polled first, the whole set only once it is up: 26.57 (a serial round trip more
//    at the moment that counts); a further 0.3 us of sleep between the BCE and the mixup flags: 27.6;
//  * no poll before 3.4 us after the workgroup's start (the chain cannot be done sooner): 26.08-26.20, i.e. the early polls
//    do not disturb the chain blocks measurably.
// The hand-off is two fabric round trips -- data acknowledged (0.36-0.40 us), flag visible and sampled (0.96 us) -- and a third
// for the operands (0.68 us with their transfer); tools/step4_times.py prints them.
__device__ __forceinline__ bool sg_step4_wait(const unsigned* flags, int lo, int hi, unsigned want, int lane) {
    const long long deadline = wall_clock64() + SG_STEP4_TIMEOUT_TICKS;
    for (int it = 0;; ++it) {
        bool ok = true;
        for (int j = lo + lane; j < hi; j += 64) ok = ok & (__hip_atomic_load(flags + j * SG_STEP4_FLAG_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == want);
        if (__all(ok)) return true;
        if ((it & 31) == 31 && wall_clock64() > deadline) return false;
        __builtin_amdgcn_s_sleep(1);
    }
}

// The same wait on n <= 64 flags from [0, n) with SG_STEP4_POLLS polls in flight, one flag per lane.  The polls are asm loads
// and the waits are spelt out: the compiler's wait-count pass knows nothing of them (and would drain a pipe it knew of).  The
// prologue spaces the polls a k-th of a round trip apart; from then on a poll is re-issued when the oldest has been examined,
// which keeps the spacing.  On return up to k - 1 polls are still in flight: their registers stay in `pp`, which the caller
// hands to sg_step4_polls_retire() behind its next full `vmcnt` wait, so that nothing else is allocated to them before.
// `quit` is an LDS word whose value 2 ends the wait (the other polling wave gave up).
#define SG_STEP4_POLLS 1                     // 1, 2 or 3: measured 8.52 / 8.57 / 8.61 us per step
#define SG_STEP4_POLL_START_TICKS 340        // no mixup poll before 3.4 us after the tile workgroup's start
struct SgStep4Polls { unsigned r[SG_STEP4_POLLS] = {}; };
__device__ __forceinline__ unsigned sg_step4_poll(const unsigned* p) {
    unsigned r;
    asm volatile("global_load_dword %0, %1, off sc1" : "=v"(r) : "v"(p) : "memory");
    return r;
}
__device__ __forceinline__ bool sg_step4_wait_piped(SgStep4Polls& pp, const unsigned* flags, int n, unsigned want, int lane, const int* quit) {
    constexpr int K = SG_STEP4_POLLS;
    static_assert(K >= 1 && K <= 3, "SG_STEP4_POLLS: 1, 2 or 3");
    const unsigned* p = flags + (lane < n ? lane : n - 1) * SG_STEP4_FLAG_STRIDE;   // spare lanes repeat the last flag
    const long long deadline = wall_clock64() + SG_STEP4_TIMEOUT_TICKS;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        pp.r[i] = sg_step4_poll(p);
        if (i + 1 < K) __builtin_amdgcn_s_sleep(28 / K);   // 64 clocks each: ~0.75 us / k
    }
    for (int it = 0;; ++it) {
#pragma unroll
        for (int i = 0; i < K; ++i) {   // oldest first
            asm volatile("s_waitcnt vmcnt(%1)" : "+v"(pp.r[i]) : "n"(K - 1) : "memory");
            if (__all(pp.r[i] == want)) return true;
            __builtin_amdgcn_s_sleep(1);
            pp.r[i] = sg_step4_poll(p);
        }
        if ((it & 31) == 31 && (wall_clock64() > deadline || __hip_atomic_load(quit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 2)) return false;
    }
}
__device__ __forceinline__ void sg_step4_polls_retire(SgStep4Polls& pp) {
#pragma unroll
    for (int i = 0; i < SG_STEP4_POLLS; ++i) asm volatile("" : "+v"(pp.r[i]) : : "memory");
}

template <int KF, int KH>
__global__ __launch_bounds__(512) void k_disc_step4(float* c_params, float* c_m, float* c_v, float* c_wT, float* c_ops,
                                                   SgOptState* c_st, int c_pack /* G | k1 << 14 (sg_wgrad_pack) */,
                                                   int c_B, Step4Args a) {
    constexpr int Fp = 16 * KF, Hp = 16 * KH, ldF = Fp + 4, ldH = Hp + 4;
    constexpr int NWC = KF > KH ? KF : KH;
    constexpr int W_LDS = 8 * 256, C_LDS = SG_CHAIN4_LDS_FLOATS(KF, KH);
    __shared__ __attribute__((aligned(16))) float sm[(C_LDS > W_LDS ? C_LDS : W_LDS) + 4];
    const int c_G = c_pack & 1023, c_k1 = (int)((unsigned)c_pack >> 14);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int Kt = 64 * c_G, n_chain = 12 * c_G, w_base = (n_chain + 7) & ~7;
    unsigned* flags = reinterpret_cast<unsigned*>(c_st) + SG_STEP4_FLAG_WORD0;
    // scratch = stacks[0] | stacks[1] | partials (disc_update_core); this step's stacks are stacks[(k1 - 1) & 1]
    float* c_part = c_ops + (size_t)(2 - ((c_k1 - 1) & 1)) * ((size_t)Kt * (3 * Hp + ldF + Fp));

    if ((int)blockIdx.x < n_chain) {
        // ------------------------------------------------------------------ the chain: k_disc_chain4's body, published
        if (wave >= NWC) return;   // the launch has 8 waves per workgroup for the tile blocks; the chain uses one per column tile
        int t0 = 0;
        if (tid == 0) t0 = c_st->t0;
        Chain4Args ca{c_params, c_wT, c_ops, c_part, c_B, c_G, 1.0f / (float)c_B, 10.0f};
        sg_chain4_body<KF, KH, true>(ca, sm);
        // every wave drains its write-through stores BEFORE the barrier the flag store sits behind.  The wait has to be spelt
        // out: __syncthreads() is a workgroup-scope fence, for which gfx950 needs no vmcnt wait (the waves of a workgroup share
        // their CU's L1), and the compiler emits none -- the flag then overtakes the data under load (replicas of 8 contexts
        // sharing one GPU diverged in the 6th digit: tests/test_gpu_world.py).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) __hip_atomic_store(flags + blockIdx.x * SG_STEP4_FLAG_STRIDE, (unsigned)(t0 + c_k1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int wb = (int)blockIdx.x - w_base;
    constexpr int th = KH, tf = KF, T2 = th * th, ntv = 8 * (th + tf), NV = (3 * Hp + 4 + 63) / 64;
    static_assert((8 - th) * (th + tf) > NV, "k_disc_step4: a spare slot must exist for the Adam-scalar lane");
    if (wb < 0) return;            // padding up to a multiple of 8: the tile map below counts XCDs from w_base
    if (wb >= ntv) {               // the next step's rows (see k_disc_chain4)
        if (a.next.ops) sg_disc_pregather(a.next, wb - ntv);
        return;
    }
    SgDiscDesc d;
    d.F = 0; d.Hd = 0; d.Hp = Hp; d.Fp = Fp; d.ldF = ldF; d.ldH = ldH;
    d.w1 = 0; d.b1 = Hp * ldF; d.w2 = d.b1 + Hp; d.b2 = d.w2 + Hp * ldH; d.w3 = d.b2 + Hp; d.b3 = d.w3 + Hp; d.total = d.b3 + 16;
    float (*red)[256] = reinterpret_cast<float (*)[256]>(sm);
    int* sh_ok = reinterpret_cast<int*>(sm + W_LDS);
    unsigned* err = reinterpret_cast<unsigned*>(c_st) + SG_STEP4_ERR_WORD;
    // tile -> XCD map of k_disc_wgrad: all tiles of one 16-row weight panel on one XCD (workgroups go to XCDs round-robin)
    const int xcd = wb & 7, slot = wb >> 3;
    const int li = lane & 15, lq = lane >> 4;
    constexpr int nw = 8;
    if (xcd < th) {
        // -------------------------------------------------------------- a 16 x 16 weight tile: k_disc_wgrad's tile body
        const int b = slot < th ? xcd * th + slot : T2 + xcd * tf + (slot - th);
        const bool w2 = b < T2;
        const int t = w2 ? b : b - T2;
        const int tm = w2 ? t / th : t / tf, tn = w2 ? t % th : t % tf;
        const int ldp = w2 ? ldH : ldF;
        const int idx = (w2 ? d.w2 : d.w1) + (tm * 16 + ((tid & 255) >> 4)) * ldp + tn * 16 + (tid & 15);
        // everything that does not depend on the chain is requested before the wait: the tile's parameters and moments, the
        // Adam scalars of both parities, the step base
        float p0 = 0.f, m0 = 0.f, v0 = 0.f;
        float4 sc = float4{0.f, 0.f, 1.f, 1.f};
        int t0 = 0;
        if (tid < 256) {
            p0 = c_params[idx]; m0 = c_m[idx]; v0 = c_v[idx];
            sc = *reinterpret_cast<const float4*>(c_st->step_size2);
        }
        if (tid < 256 || wave >= 6) t0 = c_st->t0;
        const SgStacks stk = sg_disc_stacks(c_ops, Kt, Hp, Fp, ldF);
        const float* L = (w2 ? stk.L2 : stk.L1) + (size_t)tm * Kt * 16;
        const float* Rr = (w2 ? stk.R2 : stk.R1t) + (size_t)tn * Kt * 16;
        const int n_chunks = Kt >> 4;
        const __amdgpu_buffer_rsrc_t rL = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(L), 0, Kt * 64, 0x00020000);
        const __amdgpu_buffer_rsrc_t rR = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Rr), 0, Kt * 64, 0x00020000);
        int img0 = 0, img1 = 0;
        sg_disc_img_pos(d, w2, tm * 16 + ((tid & 255) >> 4), tn * 16 + (tid & 15), img0, img1);
        // The stacked rows [0, 32G) come from the BCE workgroups (chain blocks [4G, 12G)), which finish ~0.7 us before the mixup
        // workgroups ([0, 4G): seven dependent GEMMs against three).  Wave 7 waits for the BCE flags, wave 6 for the mixup flags
        // (with SG_STEP4_POLLS polls in flight, see sg_step4_wait_piped); each tells the others through an LDS word of its own
        // -- 0 pending, 1 up, 2 gave up -- written once and spun on with LDS reads, so no wave stands at a barrier while the
        // flag it needs is already up.  A wave requests its first BCE batch when the BCE word is up and its first mixup batch
        // when the mixup word is up, into fragment registers of their own and before the BCE batch is consumed.  Waves take
        // 16-row chunks round-robin, two chunks (16 loads per lane) per batch, BCE chunks before mixup chunks: a wave's chunks
        // and their order are those of k_disc_wgrad, so the sums are bit-identical to it.
        const int half_chunks = n_chunks >> 1;
        // byte offsets of one batch of a wave's share of chunks [.., c_hi): chunks c0 and c0 + 8
        auto batch_offs = [&](int c0, int c_hi, int (&o)[2][4]) {
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int c = c0 + cc * nw;
                    const int r = c < c_hi ? 16 * c + 4 * s + lq : Kt;   // past this half: the buffer's range check returns zero
                    o[cc][s] = (r * 16 + li) * 4;
                }
        };
        // the first batch of either half: its offsets are worked out here, ahead of the waits (the empty asm keeps the compiler
        // from sinking the sixteen address computations to their use, between a word coming up and the requests)
        // chunk c goes to wave c mod 8 in both halves, as in k_disc_wgrad: the mixup half starts at this wave's first chunk at or
        // past half_chunks (half_chunks + wave whenever G is a multiple of 4; before, the mixup half was dealt from half_chunks
        // on, which at other G gave a wave other chunks than k_disc_wgrad gives it and the sums another rounding)
        const int mix0 = half_chunks + ((wave - half_chunks) & (nw - 1));
        int oa[2][4], ob[2][4];
        batch_offs(wave, half_chunks, oa);
        batch_offs(mix0, n_chunks, ob);
#pragma unroll
        for (int cc = 0; cc < 2; ++cc)
#pragma unroll
            for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(oa[cc][s]), "+v"(ob[cc][s]));
        int* sh_bce = sh_ok + 1;
        int* sh_mix = sh_ok + 2;
        if (tid == 0) { *sh_bce = 0; *sh_mix = 0; }
        const long long poll_from = wall_clock64() + SG_STEP4_POLL_START_TICKS;
        __syncthreads();
        const unsigned want = (unsigned)(t0 + c_k1);
        auto word_set = [&](int* w, bool up) {
            if (lane == 0) __hip_atomic_store(w, up ? 1 : 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
        auto word_up = [&](int* w) -> bool {   // bounded by the polling wave, which always writes its word
            int s;
            while ((s = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0) __builtin_amdgcn_s_sleep(1);
            asm volatile("" ::: "memory");     // the operand loads stay behind the word
            return s == 1;
        };
        // (a time-out is sticky: once the error word is up, the waiting workgroups of every later launch give up at once instead
        // of spinning out their own three seconds -- the update ends in its normal time, with NaN losses and the error reported)
        SgStep4Polls pp;
        if (wave == 7) {
            word_set(sh_bce, __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 && sg_step4_wait(flags, 4 * c_G, n_chain, want, lane));
        } else if (wave == 6) {
            bool up = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
            if (up) {
                while (wall_clock64() < poll_from) __builtin_amdgcn_s_sleep(2);   // the mixup chain cannot be done sooner
                // the pipe holds one flag per lane; a larger batch (4G > 64) keeps the plain loop over all its flags
                up = 4 * c_G <= 64 ? sg_step4_wait_piped(pp, flags, 4 * c_G, want, lane, sh_bce) : sg_step4_wait(flags, 0, 4 * c_G, want, lane);
            }
            word_set(sh_mix, up);
        }
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f}, alt = acc;
        auto load_offs = [&](const int (&o)[2][4], float (&x)[2][4], float (&y)[2][4]) {
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    x[cc][s] = sg_ld_sc1(rL, o[cc][s]);
                    y[cc][s] = sg_ld_sc1(rR, o[cc][s]);
                }
        };
        auto load_batch = [&](int c0, int c_hi, float (&x)[2][4], float (&y)[2][4]) {
            int o[2][4];
            batch_offs(c0, c_hi, o);
            load_offs(o, x, y);
        };
        auto mma_batch = [&](const float (&x)[2][4], const float (&y)[2][4]) {
#pragma unroll
            for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    if (s & 1) alt = sg_mfma(x[cc][s], y[cc][s], alt);
                    else acc = sg_mfma(x[cc][s], y[cc][s], acc);
                }
        };
        float xa[2][4], ya[2][4], xb[2][4], yb[2][4];
        bool up = word_up(sh_bce);
        if (up) {
            load_offs(oa, xa, ya);
            up = word_up(sh_mix);
        }
        if (!up) { if (tid == 0) { atomicOr(err, 1u); a.loss_acc[0] = __builtin_nanf(""); } return; }   // the host sees NaN losses, then the error word
        load_offs(ob, xb, yb);
        __builtin_amdgcn_sched_barrier(0);   // the mixup requests go out before the first wait for a BCE operand
        mma_batch(xa, ya);
        for (int c0 = wave + 2 * nw; c0 < half_chunks; c0 += 2 * nw) { load_batch(c0, half_chunks, xa, ya); mma_batch(xa, ya); }
        mma_batch(xb, yb);
        for (int c0 = mix0 + 2 * nw; c0 < n_chunks; c0 += 2 * nw) { load_batch(c0, n_chunks, xb, yb); mma_batch(xb, yb); }
        acc += alt;
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(4 * lq + r) * 16 + li] = acc[r];
        sg_step4_polls_retire(pp);   // the sums above needed operands requested after the last poll: every poll has landed
        __syncthreads();
        if (tid < 256) {
            float g = 0.f;
            {
                float r8[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) r8[w] = red[w][tid];
#pragma unroll
                for (int w = 0; w < 8; ++w) g += r8[w];
            }
            const bool odd = (t0 + c_k1) & 1;
            const float step_size = odd ? sc.y : sc.x, bc2_sqrt = odd ? sc.w : sc.z;
            m0 = m0 + (g - m0) * (float)(1.0 - 0.9);
            v0 = v0 * (float)0.999 + (float)(1.0 - 0.999) * g * g;
            const float denom = sqrtf(v0) / bc2_sqrt + SG_DISC_ADAM_EPS;
            p0 = p0 - step_size * (m0 / denom);
            __builtin_amdgcn_sched_barrier(0);
            // streaming stores for what the next launch's chain blocks read.  A/B, round 4: write-through (agent-scope atomic)
            // stores of the parameters and images, and plain stores written back by the end-of-kernel release -- neither beat
            // these.  Measured and removed; `git show b28af2c:simgan_amd/csrc/sg_disc_step4.hpp` has the switch.
            __builtin_nontemporal_store(p0, c_params + idx);
            __builtin_nontemporal_store(m0, c_m + idx);
            __builtin_nontemporal_store(v0, c_v + idx);
            __builtin_nontemporal_store(p0, c_wT + img0);
            __builtin_nontemporal_store(p0, c_wT + img1);
        }
        return;
    }
    const int vid = (xcd - th) * (th + tf) + slot;
    if (vid > NV) return;
    if (vid == NV) {               // the next step's Adam scalars (double-precision pow), off everybody's path
        if (tid == 0) sg_opt_prepare(c_st, c_st->t0 + c_k1 + 1);
        return;
    }
    {
        // ------------------------------------------------------------------ biases, w3, loss sums: k_disc_wgrad's vector body
        const int nparts = n_chain, stride = 4 * Hp, NE = 3 * Hp + 4;
        const int i = 64 * vid + lane;
        const float4 sc = *reinterpret_cast<const float4*>(c_st->step_size2);
        const int t0 = c_st->t0;
        const bool odd = (t0 + c_k1) & 1;
        const float step_size = odd ? sc.y : sc.x, bc2_sqrt = odd ? sc.w : sc.z;
        const bool is_param = wave == 0 && i < 3 * Hp + 1;
        const int pidx = i < Hp ? d.b1 + i : i < 2 * Hp ? d.b2 + (i - Hp) : i < 3 * Hp ? d.w3 + (i - 2 * Hp) : d.b3;
        float pv = 0.f, pm = 0.f, pvv = 0.f;
        if (is_param) { pv = c_params[pidx]; pm = c_m[pidx]; pvv = c_v[pidx]; }
        const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc(c_part, 0, nparts * stride * 4, 0x00020000);
        if (tid == 0) *sh_ok = 1;
        __syncthreads();
        if (wave == 7 && (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 || !sg_step4_wait(flags, 0, n_chain, (unsigned)(t0 + c_k1), lane)) && lane == 0) *sh_ok = 0;
        __syncthreads();
        if (!*sh_ok) { if (tid == 0) { atomicOr(err, 1u); a.loss_acc[0] = __builtin_nanf(""); } return; }   // the host sees NaN losses, then the error word
        float g = 0.f;
        if (i < NE) {
            for (int s0 = wave; s0 < nparts; s0 += 16 * nw) {
                float tt[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int sidx = s0 + u * nw;
                    tt[u] = sidx < nparts ? sg_ld_sc1(rP, (sidx * stride + i) * 4) : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 16; ++u) g += tt[u];
            }
        }
        red[wave][lane] = g;
        __syncthreads();
        if (wave == 0 && i < NE) {
            g = 0.f;
            {
                float r8[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) r8[w] = red[w][lane];
#pragma unroll
                for (int w = 0; w < 8; ++w) g += r8[w];
            }
            if (i < 3 * Hp + 1) {
                pm = pm + (g - pm) * (float)(1.0 - 0.9);
                pvv = pvv * (float)0.999 + (float)(1.0 - 0.999) * g * g;
                const float denom = sqrtf(pvv) / bc2_sqrt + SG_DISC_ADAM_EPS;
                c_params[pidx] = pv - step_size * (pm / denom);
                c_m[pidx] = pm;
                c_v[pidx] = pvv;
            }
            const int l0 = (3 * Hp) & 63;
            const float el_s = __shfl(g, l0 + 1), pl_s = __shfl(g, l0 + 2), gp_s = __shfl(g, l0 + 3);
            if (i == 3 * Hp) {
                // a2c/algo/gail.py:181-184: loss.item() etc. are float32, accumulated in Python doubles
                const float inv_B = 1.0f / (float)c_B;
                const float el = el_s * inv_B, pl = pl_s * inv_B, gp = 10.0f * (gp_s * inv_B);
                a.loss_acc[0] += (double)(el + pl + gp);
                a.loss_acc[1] += (double)el;
                a.loss_acc[2] += (double)pl;
            }
        }
    }
}
