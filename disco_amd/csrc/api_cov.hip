// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): masked covariances (staged form)
#include "host.h"
#include "k_cov.h"
#include "k_cov_wide.h"

using namespace disco;
using namespace disco_host;

namespace disco_host {
int cov_chunks(const disco_ctx* ctx) {
    const long long g = (long long)ctx->geom_rooms * ctx->cfg.nodes;
    long long c = (2048 + g - 1) / g;
    if (c > 8) c = 8;
    if (ctx->tune_cov_chunks > 0) c = ctx->tune_cov_chunks;
    if (c > ctx->T) c = ctx->T;
    if (c < 1) c = 1;
    return (int)c;
}

// frame chunks of the float64 step-1 statistics of the wide shapes (k_cov_loc_f64 starts (tiles + 1) workgroups of 4 waves per node and
// chunk: one chunk as soon as that fills the chip; every chunk leaves a (hi, lo) PAIR of blocks).  ONE definition for the launch and for
// reserve_scratch (round-4 ADVICE: a node shard or a chip of more than 256 CUs made the launch ask for more than was reserved).
int cov1_f64_chunks(const disco_ctx* ctx) {
    if (ctx->tune_cov_chunks > 0) return cov_chunks(ctx);
    const long long wgs = (long long)ctx->geom_rooms * ctx->Kl * ((ctx->F - 1 + 63) / 64 + 1);
    return (int)std::max<long long>(1, std::min<long long>(std::min(8, ctx->T), (8LL * ctx->n_cu + wgs - 1) / wgs));
}

int cov_finalize(disco_ctx* ctx, disco_c32* Rss, disco_c32* Rnn, disco_stream s) {
    PendingSums ps;
    if (!partials_pending(ctx, &ps) || ps.part_loc) return fail(ctx, DISCO_E_ARG, "cov_finalize: no whole-triangle partial sums are pending");
    const long long n_gf = (long long)ctx->cfg.rooms * ctx->Kl * ctx->F;
    hipLaunchKernelGGL(k_cov_finalize, dim3((unsigned)std::min<long long>((n_gf + 127) / 128, 65535)), dim3(128), 0,
                       (hipStream_t)s, ps.part, (c32*)Rss, (c32*)Rnn, n_gf, ctx->F, ps.blocks, ps.P,
                       1.0f / (float)ctx->T, ctx->d_lens, ctx->Kl);
    return check_launch(ctx, "k_cov_finalize");
}

int pending_matrices(disco_ctx* ctx, disco_c32* Rss, disco_c32* Rnn, disco_stream s) {
    PendingSums ps;
    if (!partials_pending(ctx, &ps)) return fail(ctx, DISCO_E_ARG, "disco_selftest_pending_matrices: no partial sums are pending");
    if (!ps.part_loc) return cov_finalize(ctx, Rss, Rnn, s);
    if (ps.M_loc < 1 || ps.M_loc > ps.P || ps.blocks_loc < 1)
        return fail(ctx, DISCO_E_ARG, "disco_selftest_pending_matrices: the pending pencil names no kept step-1 blocks");
    const long long n_gf = (long long)ctx->cfg.rooms * ctx->Kl * ctx->F;
    hipLaunchKernelGGL(k_cov_finalize_tail, dim3((unsigned)std::min<long long>((n_gf + 127) / 128, 65535)), dim3(128), 0, (hipStream_t)s,
                       ps.part, ps.part_loc, (c32*)Rss, (c32*)Rnn, n_gf, ctx->F, ps.blocks, ps.blocks_loc, ps.P, ps.M_loc,
                       1.0f / (float)ctx->T, ctx->d_lens, ctx->Kl);
    return check_launch(ctx, "k_cov_finalize_tail");
}
static CovArgs cov_args(const disco_ctx* ctx, const disco_c32* X, const float* mask, const disco_c32* Zs, const disco_c32* Zn, float4* part,
                        int chunks, int mask_remote) {
    CovArgs a;
    a.X = (const c32*)X;
    a.mask = mask;
    a.Zs = (const c32*)Zs;
    a.Zn = (const c32*)Zn;
    a.part = part;
    a.K = ctx->cfg.nodes;
    a.T = ctx->T;
    a.F = ctx->F;
    a.chunks = chunks;
    a.mask_remote = mask_remote;
    a.Kl = ctx->Kl;
    a.k0 = ctx->k0;
    a.zblk = ctx->zblk;
    a.R = ctx->cfg.rooms;
    a.lens = ctx->d_lens;
    return a;
}

// 17 <= P <= 32 (k_cov_wide.h): always the whole triangle into the full block (the step-1 sums are not re-used: no skiploc)
static int cov_partials_wide(disco_ctx* ctx, const disco_c32* X, const float* mask, const disco_c32* Zs, const disco_c32* Zn,
                             int mask_remote, int P, disco_stream s) {
    const disco_cfg& c = ctx->cfg;
    const int M = c.mics, KR = P - M;
    const int chunks = cov_chunks(ctx);
    const SumsPlan plan{(long long)c.rooms * ctx->Kl, chunks, chunks, P, false};
    const int tiles = (ctx->F - 1 + 63) / 64;
    const int nbg = (cov_wide_blocks(P) + CW_WAVES - 1) / CW_WAVES;
    const long long grid = xcd_grid(plan.G * (tiles + 1) * chunks * nbg);
    if (grid > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_cov_masked: batch too large (P > 16: more than 2^31 workgroups)");
    // the block this batch needs is checked before anything runs
    int rc = 0;
    float4* part = partials_begin(ctx, plan, &rc);
    if (rc) {
        (void)hipGetLastError();
        char m[400];
        snprintf(m, sizeof(m), "disco_cov_masked: P = %d needs %.2f GiB of partial-sum scratch (%lld units x %d chunks x %d bins x %d pairs "
                 "x 16 B), which the device cannot provide: split the batch into fewer rooms", P, plan.bytes(ctx->F) / 1073741824.0, plan.G, chunks,
                 ctx->F, plan.pairs());
        return fail(ctx, DISCO_E_UNSUPPORTED, m);
    }
    const CovArgs a = cov_args(ctx, X, mask, Zs, Zn, part, chunks, mask_remote);
    with_bool(Zs == Zn, [&](auto samez) {
        constexpr bool SAMEZ = decltype(samez)::value;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_wide<SAMEZ>), dim3((unsigned)grid), dim3(64 * CW_WAVES), 0, (hipStream_t)s, a, M, KR);
    });
    partials_commit(ctx, plan);
    return check_launch(ctx, "k_cov_wide");
}

// the block-partitioned kernels k_cov_split_lds / k_cov_loc_f64 (api_cov_split.hip); false: (M, KR) is not one of their shapes
bool cov_split_shape(int M, int KR);
bool launch_cov_split_shape(int M, int KR, bool skiploc, unsigned nblk, hipStream_t st, const disco::CovArgs& a);

// skiploc (step 2 only, internal): where the step-1 partial sums of THIS X with THIS mask are still kept (step1_held), the leading
// M x M block is neither accumulated nor written, the partial sums go to the tail block and the solver assembles the pencil from
// both.  Honoured only by k_cov_split.
int cov_partials(disco_ctx* ctx, const disco_c32* X, const float* mask, const disco_c32* Zs, const disco_c32* Zn,
                 int mask_remote, int P, disco_stream s, bool skiploc) {
    const disco_cfg& c = ctx->cfg;
    const int M = c.mics, KR = P - M;
    if (!X || !mask) return fail(ctx, DISCO_E_ARG, "disco_cov_masked: null argument");
    if (KR != 0 && KR != c.nodes - 1) return fail(ctx, DISCO_E_ARG, "disco_cov_masked: P must be M or M + K - 1");
    if (KR > 0 && (!Zs || !Zn)) return fail(ctx, DISCO_E_ARG, "disco_cov_masked: Zs/Zn required when P > M");
    if (M > 8) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_cov_masked: M > 8 mics per node not supported");
    if (P > CW_PMAX) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_cov_masked: P = M + K - 1 > 32 not supported");
    if (P > CB_PMAX) return cov_partials_wide(ctx, X, mask, Zs, Zn, mask_remote, P, s);
    const bool same = (Zs == Zn);
    const bool split = (KR == 0 || (P > 8 && same && mask_remote && (ctx->F - 1) % 64 == 0)) && cov_split_shape(M, KR);
    // step-1 shapes of the split kernels (KR = 0, M >= 7): float64 accumulators, every frame chunk leaves a (hi, lo) PAIR of partial blocks
    const bool f64 = split && KR == 0;
    const int chunks = f64 ? cov1_f64_chunks(ctx) : cov_chunks(ctx);
    skiploc = skiploc && split && KR > 0 && step1_held(ctx, X, mask);
    const SumsPlan plan{(long long)c.rooms * ctx->Kl, chunks, f64 ? 2 * chunks : chunks, P, skiploc};
    const long long G = plan.G;
    int rc = 0;
    float4* part = partials_begin(ctx, plan, &rc);
    if (rc) return rc;
    const CovArgs a = cov_args(ctx, X, mask, Zs, Zn, part, chunks, mask_remote);
    const hipStream_t st = (hipStream_t)s;
    // one workgroup per (node, bin tile | Nyquist, chunk): the split kernels and k_cov_big
    const long long nblk = G * ((ctx->F - 1 + 63) / 64 + 1) * chunks;
    const bool mkr = !split && for_mkr(M, KR, [&](auto m, auto kr) {          // P <= 8: one thread per bin holds the whole triangle
        with_bool(c.n_fft == 512, [&](auto n512) { with_bool(KR == 0 || same, [&](auto samez) {
            constexpr int M_ = decltype(m)::value, KR_ = decltype(kr)::value, NT = decltype(n512)::value ? 320 : 576;
            constexpr bool SAMEZ = decltype(samez)::value;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov<M_, KR_, SAMEZ, NT>), dim3((unsigned)(G * chunks)),
                               dim3((unsigned)(ctx->F - 1 + 64)), 0, st, a);
        }); });
    });
    if (!mkr) {                 // 9 <= P <= 16 (and the step-1 shapes M >= 7)
        if (nblk > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_cov_masked: batch too large");
        if (split)              // one vector for both statistics: one block of pairs per wave
            launch_cov_split_shape(M, KR, skiploc, (unsigned)nblk, st, a);
        else                    // pairs split over the waves of a workgroup
            with_bool(KR == 0 || same, [&](auto samez) {
                constexpr bool SAMEZ = decltype(samez)::value;
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_big<SAMEZ>), dim3((unsigned)nblk), dim3(64 * CB_S), 0, st, a, M, KR);
            });
    }
    partials_commit(ctx, plan);
    // step-1 sums (P == M, all nodes here) can be re-used by a step 2 on the same mask
    if (KR == 0 && !sharded(ctx)) step1_keep(ctx, X, mask);
    return check_launch(ctx, "k_cov");
}

// Both partial-sum blocks at the largest size any covariance call of this context can ask for with the present geometry: the plan of the
// widest pencil (P = M + K - 1) with the largest of the chunk counts above and of the other units (stft_cov_chunks, step2_chunks,
// room_chunks).  Pairing the largest count with the widest pencil over-sizes; the sizes are kept (tests/test_partials_state_emulated.py).
int reserve_scratch(disco_ctx* ctx) {
    const disco_cfg& c = ctx->cfg;
    const long long G = (long long)c.rooms * ctx->Kl;
    const int P2 = c.mics + c.nodes - 1;
    auto bytes = [&](int chunks, int P) { return SumsPlan{G, chunks, chunks, P, false}.bytes(ctx->F); };
    if (P2 > CB_PMAX && P2 <= CW_PMAX && c.mics <= 8) {
        // 17 <= P <= 32: step 1 (P = M, the chunk counts below) and step 2 (k_cov_wide, cov_chunks) size the full block; the tail block
        // only ever pairs with re-used step-1 sums, which the wide route does not take
        int ch1 = cov_chunks(ctx);
        if (c.mics >= 7) ch1 = std::max(ch1, 2 * cov1_f64_chunks(ctx));
        ch1 = std::max(ch1, stft_cov_chunks(ctx, nullptr));
        const size_t need1 = bytes(ch1, c.mics);
        return partials_reserve(ctx, std::max(need1, bytes(cov_chunks(ctx), P2)), need1);
    }
    int chunks = std::max(cov_chunks(ctx), step2_chunks(ctx, (ctx->F - 1) / 64 + 1));
    if (c.mics >= 7) chunks = std::max(chunks, 2 * cov1_f64_chunks(ctx));                       // the (hi, lo) pairs of k_cov_loc_f64
    if (c.mics <= 8) chunks = std::max(chunks, stft_cov_chunks(ctx, nullptr));
    if (P2 > 8) chunks = std::max(chunks, room_chunks(ctx));
    const size_t need = bytes(chunks, std::min(P2, 16));
    return partials_reserve(ctx, need, need);
}
}  // namespace disco_host

extern "C" int disco_cov_masked(disco_ctx* ctx, const disco_c32* X, const float* mask, const disco_c32* Zs,
                                const disco_c32* Zn, int mask_remote, int P, disco_c32* Rss, disco_c32* Rnn,
                                disco_stream s) {
    DISCO_ENTER(ctx);
    return cov_pass_entry(ctx, "disco_cov_masked", Rss, Rnn, s, [&] { return cov_partials(ctx, X, mask, Zs, Zn, mask_remote, P, s); });
}

// test-only (include/disco_hip.h): cov_finalize for whatever is pending, two-block pencils included
extern "C" int disco_selftest_pending_matrices(disco_ctx* ctx, disco_c32* Rss, disco_c32* Rnn, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!Rss || !Rnn) return fail(ctx, DISCO_E_ARG, "disco_selftest_pending_matrices: null argument");
    return pending_matrices(ctx, Rss, Rnn, s);
}
