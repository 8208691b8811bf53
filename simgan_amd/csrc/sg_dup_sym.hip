// sg_dup_sym.hip -- mirror-augmented rollouts (--dup-sym): the mirrored half of a 2n-column rollout made on the device.
//
// Replaces (reference): the rollout fill of a2c/main.py:171-245 with --dup-sym -- every step's rows are mirrored on the host
// (mirror_obsact_batch(..., augment=True), my_pybullet_envs/utils.py:334-357) or repeated (.repeat(2, 1)) and a rollout of
// twice the width is inserted.  Here columns [0, n) are uploaded and one launch writes column n + j of every slot from
// column j.
#include <math.h>

#include "sg_common.h"

// One field of the launch: columns [0, n) of `slots` time slots -> columns [n, 2n).  m == NULL: a copy (.repeat(2, 1));
// otherwise out = M x per row, in k_mirror_rows' arithmetic (sg_ppo_kernels.hpp): double accumulation over ascending j, the zero
// entries of M skipped, one cast -- a signed permutation is exact, and both symmetry features give the same bits.
struct DupSymField {
    float* base;       // the field, [slots..][2n][w]
    const float* m;    // [w][w] row-major mirror, or NULL
    int w;             // floats per row
    int slots;         // time slots written (0 .. slots-1)
    int tile_rows;     // rows of one tile (a tile never crosses a slot)
    int m_lds;         // the mirror is staged in LDS (it fits beside a tile); else read from global memory
};
#define SG_DUP_FIELDS 8
struct DupSymArgs {
    DupSymField f[SG_DUP_FIELDS];
    int n;             // columns per half
};

// grid (tiles, fields): blockIdx.y picks the field, the blocks of a row stride over its (slot, row tile) pairs.  Every access
// is a single float: the mirrored half of a slot starts n * w floats into the row, which is 16-byte aligned only by accident
// (n = 1, O = 5: float 5), so nothing here is wider than its alignment.  A tile's source rows are contiguous and each source
// float is fetched from global memory once (mirrored fields: into LDS, from where the w outputs of its row read it).
__global__ __launch_bounds__(256) void k_dup_sym(DupSymArgs a) {
    extern __shared__ float sg_dup_lds[];
    const DupSymField f = a.f[blockIdx.y];
    const int n = a.n, w = f.w;
    const int tiles_per_slot = (n + f.tile_rows - 1) / f.tile_rows;
    const int64_t tiles = (int64_t)f.slots * tiles_per_slot;
    if ((int64_t)blockIdx.x >= tiles) return;
    const int64_t half = (int64_t)n * w;           // floats of one half of a slot
    // LDS: lo[w] | hi[w] (the span of non-zero entries of every mirror row) | [w][w] mirror when staged | [tile_rows][w] tile
    int* lo = reinterpret_cast<int*>(sg_dup_lds);
    int* hi = lo + w;
    float* ms = sg_dup_lds + 2 * w;
    float* xs = ms + (f.m && f.m_lds ? w * w : 0);
    const float* mm = f.m_lds ? ms : f.m;
    if (f.m) {
        if (f.m_lds) {
            for (int i = threadIdx.x; i < w * w; i += blockDim.x) ms[i] = f.m[i];
            __syncthreads();
        }
        // entries outside [lo, hi) are zero and would be skipped one by one: a block-diagonal mirror (Laikago: 37-float
        // blocks, at most three non-zeros per row) walks a handful of entries per output instead of all w
        for (int i = threadIdx.x; i < w; i += blockDim.x) {
            const float* mi = mm + (size_t)i * w;
            int first = w, end = 0;
            for (int j = 0; j < w; ++j)
                if (mi[j] != 0.f) {
                    if (first == w) first = j;
                    end = j + 1;
                }
            lo[i] = first;
            hi[i] = end;
        }
        __syncthreads();
    }
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t slot = tile / tiles_per_slot;
        const int r0 = (int)(tile - slot * tiles_per_slot) * f.tile_rows;
        const int rows = n - r0 < f.tile_rows ? n - r0 : f.tile_rows;
        const int cnt = rows * w;                  // floats of this tile
        const float* src = f.base + slot * 2 * half + (int64_t)r0 * w;
        float* dst = f.base + slot * 2 * half + half + (int64_t)r0 * w;
        if (!f.m) {
            for (int e = threadIdx.x; e < cnt; e += blockDim.x) dst[e] = src[e];
            continue;
        }
        for (int e = threadIdx.x; e < cnt; e += blockDim.x) xs[e] = src[e];
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
            const int r = e / w, i = e - r * w;
            const float* x = xs + r * w;
            const float* mi = mm + (size_t)i * w;
            double s = 0.0;
            const int j1 = hi[i];
            for (int j = lo[i]; j < j1; ++j) {
                const float c = mi[j];
                if (c != 0.f) s += (double)c * (double)x[j];
            }
            dst[e] = (float)s;
        }
        __syncthreads();                           // the next tile overwrites xs
    }
}

static int check_mirror(const float* m, int w, const char* name) {
    for (int64_t i = 0; i < (int64_t)w * w; ++i)
        SG_REQUIRE(isfinite(m[i]), "sg_rollout_set_mirrors: %s[%lld][%lld] is not finite (%g)", name, (long long)(i / w),
                   (long long)(i % w), (double)m[i]);
    return 0;
}

extern "C" int sg_rollout_set_mirrors(sg_rollout* r, const float* m_obs, const float* m_act) {
    SG_DEVICE_WIDE();
    SG_REQUIRE(r, "sg_rollout_set_mirrors: rollout is NULL");
    SG_REQUIRE(m_act, "sg_rollout_set_mirrors: the action mirror m_act is required");
    SG_REQUIRE(r->N % 2 == 0, "sg_rollout_set_mirrors: the rollout has N = %d columns, an odd number: a mirror-augmented rollout "
               "holds n environments and their n mirror images (N = 2n)", r->N);
    SG_TRY(check_mirror(m_act, r->A, "m_act"));
    if (m_obs) SG_TRY(check_mirror(m_obs, r->O, "m_obs"));
    sg_ctx* ctx = r->ctx;
    SG_CHECK(hipSetDevice(ctx->device));
    SG_CHECK(hipStreamSynchronize(ctx->stream));   // a queued sg_rollout_dup_sym may still read the mirrors
    const size_t ba = sizeof(float) * (size_t)r->A * r->A, bo = sizeof(float) * (size_t)r->O * r->O;
    if (!r->d_mact) SG_CHECK(sg_dev_malloc((void**)&r->d_mact, ba));
    SG_COPY_SYNC(ctx, r->d_mact, m_act, ba, hipMemcpyHostToDevice);
    if (m_obs) {
        if (!r->d_mobs) SG_CHECK(sg_dev_malloc((void**)&r->d_mobs, bo));
        SG_COPY_SYNC(ctx, r->d_mobs, m_obs, bo, hipMemcpyHostToDevice);
    } else if (r->d_mobs) {
        SG_CHECK(sg_dev_free(r->d_mobs));
        r->d_mobs = nullptr;
    }
    r->mirrors_set = true;
    return 0;
}

extern "C" int sg_rollout_dup_sym(sg_rollout* r) {
    SG_REQUIRE(r, "sg_rollout_dup_sym: rollout is NULL");
    SG_REQUIRE(r->mirrors_set, "sg_rollout_dup_sym: the rollout has no mirrors: call sg_rollout_set_mirrors first");
    const int n = r->N / 2, T = r->T;
    // LDS budget of a block: what every gfx950 launch may ask for without opting in
    const size_t budget = (size_t)(r->ctx->lds_bytes < 65536 ? r->ctx->lds_bytes : 65536);
    DupSymArgs a;
    a.n = n;
    int nf = 0;
    int64_t max_tiles = 0;
    size_t lds = 0;
    auto add = [&](int field, const float* m, int slots) -> int {
        const int w = r->field_width[field];
        if (w == 0) return 0;                      // feat_len = 0: an empty field
        DupSymField& f = a.f[nf];
        f.base = r->d_field[field]; f.m = m; f.w = w; f.slots = slots; f.m_lds = 0;
        size_t need = 0;
        if (!m) {
            f.tile_rows = 1024 / w > 0 ? 1024 / w : 1;
        } else {
            const size_t mb = sizeof(float) * (size_t)w * w, row = sizeof(float) * (size_t)w;
            const size_t spans = 2 * sizeof(int) * (size_t)w;   // lo[w], hi[w]
            SG_REQUIRE(spans + row <= budget, "sg_rollout_dup_sym: one %d-float row does not fit LDS (%zu bytes)", w, budget);
            f.m_lds = spans + mb + row <= budget ? 1 : 0;
            const size_t left = budget - spans - (f.m_lds ? mb : 0);
            size_t rows = left / row;
            const size_t want = 2048 / (size_t)w > 0 ? 2048 / (size_t)w : 1;   // ~8 KiB of rows per tile
            if (rows > want) rows = want;
            f.tile_rows = (int)rows;
            need = spans + (f.m_lds ? mb : 0) + rows * row;
        }
        if (f.tile_rows > n) f.tile_rows = n;
        const int64_t tiles = (int64_t)slots * ((n + f.tile_rows - 1) / f.tile_rows);
        if (tiles > max_tiles) max_tiles = tiles;
        if (need > lds) lds = need;
        ++nf;
        return 0;
    };
    if (r->d_mobs) SG_TRY(add(SG_F_OBS, r->d_mobs, T + 1));
    SG_TRY(add(SG_F_ACTIONS, r->d_mact, T));
    SG_TRY(add(SG_F_OBS_FEAT, nullptr, T + 1));
    SG_TRY(add(SG_F_MASKS, nullptr, T + 1));
    SG_TRY(add(SG_F_BAD_MASKS, nullptr, T + 1));
    SG_TRY(add(SG_F_REWARDS, nullptr, T));
    SG_TRY(add(SG_F_LOGP, nullptr, T));
    SG_TRY(add(SG_F_VALUE_PREDS, nullptr, T));    // (slot T is compute_returns' next_value: V(mirror(s_T)), not a repeat)
    const unsigned gx = (unsigned)(max_tiles < 512 ? max_tiles : 512);
    hipLaunchKernelGGL(k_dup_sym, dim3(gx, nf), dim3(256), lds, r->ctx->stream, a);
    SG_CHECK(hipGetLastError());
    r->feat_version = sg_next_feat_version();
    return 0;
}

extern "C" int sg_rollout_upload_columns(sg_rollout* r, int field, int n_cols, const float* host, int64_t count) {
    SG_REQUIRE(r, "sg_rollout_upload_columns: rollout is NULL");
    SG_REQUIRE(field >= 0 && field < SG_F_COUNT, "sg_rollout_upload_columns: unknown field %d", field);
    SG_REQUIRE(host, "sg_rollout_upload_columns: host is NULL");
    SG_REQUIRE(field != SG_F_ADVANTAGES, "sg_rollout_upload_columns: advantages are read-only");
    SG_REQUIRE(count == r->field_count[field], "sg_rollout_upload_columns: host is the full-width field %d of %lld floats, got %lld",
               field, (long long)r->field_count[field], (long long)count);
    SG_REQUIRE(n_cols > 0 && n_cols <= r->N, "sg_rollout_upload_columns: %d columns out of range (0, %d]", n_cols, r->N);
    if (count == 0) return 0;
    const size_t pitch = sizeof(float) * (size_t)r->N * r->field_width[field];
    const size_t width = sizeof(float) * (size_t)n_cols * r->field_width[field];
    SG_CHECK(hipMemcpy2DAsync(r->d_field[field], pitch, host, pitch, width, (size_t)r->field_slots[field], hipMemcpyHostToDevice,
                              r->ctx->stream));
    SG_CHECK(hipStreamSynchronize(r->ctx->stream));
    if (field == SG_F_OBS_FEAT) r->feat_version = sg_next_feat_version();
    return 0;
}
