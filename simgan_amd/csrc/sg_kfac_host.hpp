// sg_kfac_host.hpp -- host side of the ACKTR mode of sg_ppo (included by sg_ppo.hip alone): the K-FAC object's device state
// (SgKfac, sg_kfac.hpp), its set-up and release, the arguments of k_kfac_eig, and the two entry points that touch nothing else.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "sg_kfac.hpp"

static void kfac_free(sg_ppo* a) {
    SgKfac* k = a->kfac;
    if (!k) return;
    void* ptrs[] = {k->d_acc, k->d_m, k->d_Q, k->d_d, k->d_work, k->d_ks, k->d_vec, k->d_t0, k->d_t1, k->d_one, k->d_vpart,
                    k->d_jobs, k->d_tiles, k->d_eps, k->d_fish};
    for (void* q : ptrs) if (q) (void)sg_dev_free(q);
    delete k;
    a->kfac = nullptr;
}

static int kfac_setup(sg_ctx* ctx, SgKfac* k, const SgPolicyDesc& d, float* d_grad) {
    const SgTrunk& ac = d.trunk[0];
    const SgTrunk& cr = d.trunk[1];
    const int O = d.O, A = d.A, H = ac.H, Hc = cr.H;
    const int nf[SG_KFAC_NF] = {O, H, H, Hc, Hc, H, H, Hc, Hc, 1, A, A};
    int fo = 0, vo = 0;
    int64_t wo = 0;
    k->lds_n = 0;
    while (16 * (k->lds_n + 1) * (k->lds_n + 1) + 8192 <= ctx->lds_bytes) ++k->lds_n;
    for (int f = 0; f < SG_KFAC_NF; ++f) {
        if (f == SG_KFAC_NA) k->g_start = fo;
        k->n[f] = nf[f]; k->off[f] = fo; k->voff[f] = vo; k->woff[f] = wo;
        fo += nf[f] * nf[f]; vo += nf[f];
        if (nf[f] > k->lds_n) wo += 2 * (int64_t)nf[f] * nf[f];
        SG_REQUIRE(nf[f] <= 512, "sg_acktr_create: a %d-wide Kronecker factor is larger than the eigensolver's 512", nf[f]);
    }
    k->fac_total = fo; k->vec_total = vo; k->work_doubles = wo;
    const KfacModule mods[SG_KFAC_MODULES] = {
        {0, 5, ac.off + ac.w1, d.ldO, H, O, 0},     {-1, 5, ac.off + ac.b1, 1, H, 1, 0},
        {1, 6, ac.off + ac.w2, ac.ldH, H, H, 0},    {-1, 6, ac.off + ac.b2, 1, H, 1, 0},
        {0, 7, cr.off + cr.w1, d.ldO, Hc, O, 0},    {-1, 7, cr.off + cr.b1, 1, Hc, 1, 0},
        {3, 8, cr.off + cr.w2, cr.ldH, Hc, Hc, 0},  {-1, 8, cr.off + cr.b2, 1, Hc, 1, 0},
        {4, 9, cr.off + cr.wh, cr.ldH, 1, Hc, 0},   {-1, 9, cr.off + cr.bh, 1, 1, 1, 0},
        {2, 10, ac.off + ac.wh, ac.ldH, A, H, 0},   {-1, 10, ac.off + ac.bh, 1, A, 1, 0},
        {-1, 11, ac.off + ac.ex, 1, A, 1, 0}};
    int to = 0;
    k->max_tiles = 0;
    for (int m = 0; m < SG_KFAC_MODULES; ++m) {
        k->mod[m] = mods[m];
        k->mod[m].toff = to;
        to += mods[m].out * mods[m].in;
        k->max_tiles = std::max(k->max_tiles, ((mods[m].out + 31) / 32) * ((mods[m].in + 31) / 32));
    }
    k->tmp_total = to;
    SG_CHECK(sg_dev_malloc((void**)&k->d_acc, sizeof(float) * fo));
    SG_CHECK(sg_dev_malloc((void**)&k->d_m, sizeof(float) * fo));
    SG_CHECK(sg_dev_malloc((void**)&k->d_Q, sizeof(float) * fo));
    SG_CHECK(sg_dev_malloc((void**)&k->d_d, sizeof(float) * vo));
    if (wo) SG_CHECK(sg_dev_malloc((void**)&k->d_work, sizeof(double) * wo));
    SG_CHECK(sg_dev_malloc((void**)&k->d_ks, sizeof(KfacDevState)));
    SG_CHECK(sg_dev_malloc((void**)&k->d_vec, sizeof(float) * (d.total + 8)));
    SG_CHECK(sg_dev_malloc((void**)&k->d_t0, sizeof(float) * to));
    SG_CHECK(sg_dev_malloc((void**)&k->d_t1, sizeof(float) * to));
    SG_CHECK(sg_dev_malloc((void**)&k->d_one, sizeof(float) * 4));
    SG_CHECK(sg_dev_malloc((void**)&k->d_vpart, sizeof(float) * SG_KFAC_MODULES * k->max_tiles));
    SG_CHECK(hipMemsetAsync(k->d_m, 0, sizeof(float) * fo, ctx->stream));
    SG_CHECK(hipMemsetAsync(k->d_Q, 0, sizeof(float) * fo, ctx->stream));
    SG_CHECK(hipMemsetAsync(k->d_d, 0, sizeof(float) * vo, ctx->stream));
    SG_CHECK(hipMemsetAsync(k->d_ks, 0, sizeof(KfacDevState), ctx->stream));
    SG_CHECK(hipMemsetAsync(k->d_vec, 0, sizeof(float) * (d.total + 8), ctx->stream));
    const float one[4] = {1.f, 1.f, 1.f, 1.f};
    SG_COPY_SYNC(ctx, k->d_one, one, sizeof one, hipMemcpyHostToDevice);
    // the four preconditioning stages of every module (see k_kfac_gemm): t0 = Q_g^T grad; t1 = (t0 Q_a) / (d_g d_a^T + la);
    // t0 = Q_g t1; v = t0 Q_a^T (with the tile sums of v * grad)
    std::vector<KfacJob> jobs(4 * SG_KFAC_MODULES);
    for (int m = 0; m < SG_KFAC_MODULES; ++m) {
        const KfacModule& md = k->mod[m];
        const float* Qa = md.a_f >= 0 ? k->d_Q + k->off[md.a_f] : k->d_one;
        const float* da = md.a_f >= 0 ? k->d_d + k->voff[md.a_f] : k->d_one;
        const float* Qg = k->d_Q + k->off[md.g_f];
        const float* dg = k->d_d + k->voff[md.g_f];
        float* t0 = k->d_t0 + md.toff;
        float* t1 = k->d_t1 + md.toff;
        const int M = md.out, N = md.in;
        KfacJob j;
        memset(&j, 0, sizeof j);
        j.M = M; j.N = N;
        KfacJob s1 = j, s2 = j, s3 = j, s4 = j;
        s1.K = M; s1.A = Qg; s1.lda = M; s1.ta = 1; s1.B = d_grad + md.goff; s1.ldb = md.gld; s1.C = t0; s1.ldc = N;
        s2.K = N; s2.A = t0; s2.lda = N; s2.B = Qa; s2.ldb = N; s2.C = t1; s2.ldc = N; s2.epi = 1; s2.dg = dg; s2.da = da;
        s3.K = M; s3.A = Qg; s3.lda = M; s3.B = t1; s3.ldb = N; s3.C = t0; s3.ldc = N;
        s4.K = N; s4.A = t0; s4.lda = N; s4.B = Qa; s4.ldb = N; s4.tb = 1; s4.C = k->d_vec + md.goff; s4.ldc = md.gld; s4.epi = 2;
        s4.G = d_grad + md.goff; s4.ldg = md.gld;
        jobs[0 * SG_KFAC_MODULES + m] = s1;
        jobs[1 * SG_KFAC_MODULES + m] = s2;
        jobs[2 * SG_KFAC_MODULES + m] = s3;
        jobs[3 * SG_KFAC_MODULES + m] = s4;
    }
    SG_CHECK(sg_dev_malloc((void**)&k->d_jobs, sizeof(KfacJob) * jobs.size()));
    SG_COPY_SYNC(ctx, k->d_jobs, jobs.data(), sizeof(KfacJob) * jobs.size(), hipMemcpyHostToDevice);
    std::vector<int4> tiles;
    for (int f = 0; f < SG_KFAC_NF; ++f) {
        const int T = (k->n[f] + 15) / 16;
        for (int ti = 0; ti < T; ++ti)
            for (int tj = ti; tj < T; ++tj) tiles.push_back(make_int4(f, ti, tj, 0));
    }
    k->n_tiles = (int)tiles.size();
    SG_CHECK(sg_dev_malloc((void**)&k->d_tiles, sizeof(int4) * tiles.size()));
    SG_COPY_SYNC(ctx, k->d_tiles, tiles.data(), sizeof(int4) * tiles.size(), hipMemcpyHostToDevice);
    return 0;
}

static KfacEigArgs kfac_eig_args(const SgKfac* k) {
    KfacEigArgs e;
    memset(&e, 0, sizeof e);
    e.m = k->d_m; e.Q = k->d_Q; e.dv = k->d_d; e.work = k->d_work;
    for (int f = 0; f < SG_KFAC_NF; ++f) { e.n[f] = k->n[f]; e.off[f] = k->off[f]; e.voff[f] = k->voff[f]; e.woff[f] = k->woff[f]; }
    e.lds_n = k->lds_n; e.tf = k->cfg.Tf; e.ks = k->d_ks;
    return e;
}

static size_t kfac_eig_lds(const SgKfac* k) {
    int nl = 0;
    for (int f = 0; f < SG_KFAC_NF; ++f) if (k->n[f] <= k->lds_n) nl = std::max(nl, k->n[f]);
    return sizeof(double) * 2 * (size_t)nl * nl;
}

extern "C" int sg_acktr_set_value_noise(sg_ppo* a, const float* eps, int64_t n) {
    SG_REQUIRE(a, "sg_acktr_set_value_noise: NULL argument");
    SG_REQUIRE(a->kfac, "sg_acktr_set_value_noise: not an ACKTR handle");
    SgKfac* k = a->kfac;
    if (!eps) {
        k->eps_pending = false;
        k->eps_host.clear();
        return 0;
    }
    SG_REQUIRE(n > 0 && n < (1ll << 30), "sg_acktr_set_value_noise: %lld values", (long long)n);
    k->eps_host.assign(eps, eps + n);
    k->eps_pending = true;
    return 0;
}

extern "C" int sg_acktr_get_state(sg_ppo* a, float* m_aa, int64_t n_aa, float* m_gg, int64_t n_gg, float* momentum_buf,
                                  int64_t n, int64_t* steps) {
    SG_REQUIRE(a && m_aa && m_gg && momentum_buf && steps, "sg_acktr_get_state: NULL argument");
    SG_REQUIRE(a->kfac, "sg_acktr_get_state: not an ACKTR handle");
    const SgKfac* k = a->kfac;
    const SgPolicyDesc& d = a->policy->desc;
    SG_REQUIRE(n == sg_policy_flat_count(d), "sg_acktr_get_state: bad momentum length");
    int64_t want_aa = 0, want_gg = 0;
    for (int m = 0; m < SG_KFAC_MODULES; ++m) {
        want_aa += (int64_t)k->mod[m].in * k->mod[m].in;
        want_gg += (int64_t)k->mod[m].out * k->mod[m].out;
    }
    SG_REQUIRE(n_aa == want_aa && n_gg == want_gg, "sg_acktr_get_state: m_aa / m_gg take %lld / %lld floats", (long long)want_aa,
               (long long)want_gg);
    std::vector<float> fac(k->fac_total), buf(d.total);
    KfacDevState ks;
    SG_CHECK(hipSetDevice(a->ctx->device));
    SG_CHECK(hipStreamSynchronize(a->ctx->stream));
    SG_COPY_SYNC(a->ctx, fac.data(), k->d_m, sizeof(float) * k->fac_total, hipMemcpyDeviceToHost);
    SG_COPY_SYNC(a->ctx, buf.data(), a->d_m, sizeof(float) * d.total, hipMemcpyDeviceToHost);
    SG_COPY_SYNC(a->ctx, &ks, k->d_ks, sizeof ks, hipMemcpyDeviceToHost);
    SG_REQUIRE(!ks.err, "sg_acktr_get_state: k_kfac_eig hit its sweep cap (%d) on an earlier update", SG_KFAC_SWEEPS);
    float *pa = m_aa, *pg = m_gg;
    for (int m = 0; m < SG_KFAC_MODULES; ++m) {
        const KfacModule& md = k->mod[m];
        if (md.a_f >= 0) {
            memcpy(pa, fac.data() + k->off[md.a_f], sizeof(float) * md.in * md.in);
        } else {
            pa[0] = ks.steps > 0 ? 1.f : 0.f;   // ones^T ones / B
        }
        pa += (int64_t)md.in * md.in;
        memcpy(pg, fac.data() + k->off[md.g_f], sizeof(float) * md.out * md.out);
        pg += (int64_t)md.out * md.out;
    }
    sg_policy_unpad(d, buf.data(), momentum_buf);
    *steps = ks.steps;
    return 0;
}
