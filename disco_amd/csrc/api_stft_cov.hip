// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): STFT + step-1 covariance in one pass
#include "host.h"
#include "k_stft.h"

using namespace disco;
using namespace disco_host;

// frame chunks (= workgroups per node) of the fused STFT + covariance pass and the frames each of its waves streams: runs as long
// as possible while leaving >= ~2048 workgroups for the chip, but NOT LONGER THAN DISCO_STFT_COV_RUN frames: a workgroup's fold sums the
// frames of its four waves' runs in float32, and the length of that sum is what the distance of the C3 output from the float64 oracle follows
// (the whole-batch sweep's worst room of 1000, output against the oracle: 4.1e-5 at 80 frames per wave, 2.3e-5 at 40, 1.3e-5 at 20 -- every room halves
// with the run, profiles/r05_t_runw_parity.txt), while the pass itself is as fast at 40 or 20 as at 80 (profiles/r05_t_runw_speed.txt); what
// more blocks cost is the solvers' fetch (k_solve_small.h: four blocks of an entry in flight together).
#ifndef DISCO_STFT_COV_RUN
#define DISCO_STFT_COV_RUN 40
#endif
namespace disco_host {
int stft_cov_chunks(const disco_ctx* ctx, int* runw_out) {
    const long long G = (long long)ctx->geom_rooms * ctx->cfg.nodes;
    const long long chunks_wanted = std::max<long long>(1, (2048 + G - 1) / G);
    int runw = (int)((ctx->T + STFT_WAVES * chunks_wanted - 1) / (STFT_WAVES * chunks_wanted));
    runw = std::min(DISCO_STFT_COV_RUN, std::max(8, runw));
    if (ctx->tune_runw > 0) runw = ctx->tune_runw;
    if (runw_out) *runw_out = runw;
    return (ctx->T + STFT_WAVES * runw - 1) / (STFT_WAVES * runw);
}

// o: host.h (StftCovOpts)
int stft_cov_partials(disco_ctx* ctx, const float* y, const float* mask_z, disco_c32* X, disco_stream s, const StftCovOpts& o) {
    const bool store = o.store, packed = o.layout == XLayout::Packed;
    if (!y || !mask_z || (store && !X)) return fail(ctx, DISCO_E_ARG, "disco_stft_cov_fused: null argument");
    if (packed && (!store || ctx->cfg.n_fft != 512)) return fail(ctx, DISCO_E_UNSUPPORTED, "stft_cov: the packed layout needs n_fft = 512 and stored spectra");
    // (works on a node shard too: nothing in this pass looks beyond one node -- X, masks and partial sums then hold the shard's Kl nodes per room)
    const disco_cfg& c = ctx->cfg;
    const int M = c.mics;
    if (M > 8) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_stft_cov_fused: more than 8 mics per node");
    if (c.n_fft == 1024 && M > 6) {        // staged form of the same two operations
        // (Round 3 built the one-pass form for this shape -- four transform waves with a channel pair each plus eight fold waves, one
        // bin per thread, two LDS tiles, one barrier per frame: parity-green and SLOWER, 12.8 ms against 5.1 + 3.9 ms per C5 launch.
        // The 144 accumulator registers per bin force 12 waves and 100 KiB of LDS into one workgroup, i.e. ONE workgroup and four
        // transform waves per CU where k_stft_pairs keeps eight; the transforms set the pace.  Dropped, see DESIGN.md.)
        if (!store) return fail(ctx, DISCO_E_UNSUPPORTED, "stft_cov without store: shape needs the staged kernels");
        int rc0 = STAGE(ctx, s, "stft", disco_stft(ctx, y, (int64_t)c.rooms * ctx->Kl, M, X, s));
        if (rc0) return rc0;
        return STAGE(ctx, s, "cov1", cov_partials(ctx, X, mask_z, nullptr, nullptr, 0, M, s));
    }
    int runw = 0;
    const int chunks = stft_cov_chunks(ctx, &runw);
    const SumsPlan plan{(long long)c.rooms * ctx->Kl, chunks, chunks, M, false};
    const long long G = plan.G;
    int rc = 0;
    float4* part = partials_begin(ctx, plan, &rc);
    if (rc) return rc;
    if (G * chunks > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_stft_cov_fused: batch too large");
    const auto launch = [&](auto n512, auto st, auto pack) {
        constexpr int N = decltype(n512)::value ? 512 : 1024;
        constexpr bool STORE = decltype(st)::value, PACK = decltype(pack)::value;
        if constexpr (PACK && !(N == 512 && STORE)) {          // packed rows: 512 points, stored spectra (refused above otherwise)
            return false;
        } else {                                                // the 1024-point spectrum tile of 7-8 mics does not fit the 160 KiB LDS
            return for_int<1, (N == 512 ? 8 : 6)>(M, [&](auto m) {
                constexpr int M_ = decltype(m)::value;
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stft_cov<N, M_, STORE, PACK>), dim3((unsigned)(G * chunks)), dim3(64 * STFT_WAVES), 0,
                                   (hipStream_t)s, y, mask_z, STORE ? (c32*)X : nullptr, part, ctx->d_win, ctx->d_tw, c.length, ctx->T, c.pad_mode, chunks,
                                   runw, ctx->d_lens, ctx->Kl, o.zero_beyond ? 1 : 0);
            });
        }
    };
    const bool ok = STAGE(ctx, s, store ? "stft_cov1" : "stft_cov1_nostore", with_bool(c.n_fft == 512, [&](auto n512) {
        return with_bool(store, [&](auto st) { return with_bool(packed, [&](auto pack) { return launch(n512, st, pack); }); });
    }));
    if (!ok) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_stft_cov_fused: unsupported mic count");
    partials_commit(ctx, plan);
    // kept for a possible re-use by step 2, unless there is nothing to pair these sums with later (no spectra; a shard runs the staged step 2)
    if (store && !sharded(ctx)) step1_keep(ctx, X, mask_z);
    return check_launch(ctx, "k_stft_cov");
}

}  // namespace disco_host

extern "C" int disco_stft_cov_fused(disco_ctx* ctx, const float* y, const float* mask_z, disco_c32* X, disco_c32* Rss,
                                    disco_c32* Rnn, disco_stream s) {
    DISCO_ENTER(ctx);
    return cov_pass_entry(ctx, "disco_stft_cov_fused", Rss, Rnn, s, [&] { return stft_cov_partials(ctx, y, mask_z, X, s); });
}

// test-only: the same pass writing X in the packed workspace layout (include/disco_hip.h)
extern "C" int disco_selftest_stft_cov_packed(disco_ctx* ctx, const float* y, const float* mask_z, disco_c32* X, disco_c32* Rss,
                                              disco_c32* Rnn, disco_stream s) {
    DISCO_ENTER(ctx);
    StftCovOpts o;
    o.layout = XLayout::Packed;
    return cov_pass_entry(ctx, "disco_selftest_stft_cov_packed", Rss, Rnn, s, [&] { return stft_cov_partials(ctx, y, mask_z, X, s, o); });
}
