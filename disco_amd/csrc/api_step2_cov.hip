// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): step 2 with the z exchange on chip: covariances
#include "step2_launch.h"

using namespace disco;
using namespace disco_host;

// step 2 with the in-register z exchange
namespace disco_host {
int step2_chunks(const disco_ctx* ctx, int tiles_plus_1) {
    const long long base = (long long)ctx->geom_rooms * tiles_plus_1;
    long long c = (4096 + base - 1) / base;
    if (c > 8) c = 8;
    if (ctx->tune_step2_chunks > 0) c = ctx->tune_step2_chunks;
    if (c > ctx->T) c = ctx->T;
    if (c < 1) c = 1;
    return (int)c;
}

// lead, layout: host.h.  The packed layout is that of the shapes the fused route of the whole path takes (K >= 2, 512 points) -- the same z and
// partial sums.
int step2_cov_partials(disco_ctx* ctx, const disco_c32* X, const float* mask_w, const disco_c32* w_loc, disco_c32* z_out, disco_stream s,
                       LeadBlock lead, XLayout layout) {
    if (!X || !mask_w || !w_loc) return fail(ctx, DISCO_E_ARG, "disco_step2_cov_fused: null argument");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "fused kernels need every node of a room on this GPU (node shard active)");
    const disco_cfg& c = ctx->cfg;
    const int M = c.mics, K = c.nodes, P = M + K - 1;
    if (P > 8) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_cov_fused: M + K - 1 > 8 not supported yet");
    const bool skiploc = lead == LeadBlock::Step1, packed = layout == XLayout::Packed;
    const int tiles = (ctx->F - 1) / 64;
    const int chunks = step2_chunks(ctx, tiles + 1);
    const SumsPlan plan{(long long)c.rooms * K, chunks, chunks, P, skiploc};
    int rc = 0;
    float4* part = partials_begin(ctx, plan, &rc);
    if (rc) return rc;
    const Step2Args a = step2_args(ctx, X, mask_w, w_loc, nullptr, z_out, nullptr, part, chunks);
    const long long nblk = (long long)c.rooms * (tiles + 1) * chunks;
    if (nblk > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_cov_fused: batch too large");
    if (packed && (K < 2 || c.n_fft != 512)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_cov_fused: the packed layout needs K >= 2 and n_fft = 512");
    const bool found = for_mkr(M, K - 1, [&](auto m, auto kr) { with_bool(skiploc, [&](auto skip) { with_bool(packed, [&](auto pack) {
        constexpr int M_ = decltype(m)::value, K_ = decltype(kr)::value + 1;
        constexpr bool SKIPLOC = decltype(skip)::value, PACK = decltype(pack)::value;
        if constexpr (!PACK || K_ >= 2)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_step2_cov_fused<M_, K_, SKIPLOC, PACK>), dim3((unsigned)nblk), dim3(64 * K_), 0, (hipStream_t)s, a);
    }); }); });
    if (!found) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_cov_fused: unsupported (M, K) combination");
    partials_commit(ctx, plan);
    return check_launch(ctx, "k_step2_cov_fused");
}

}  // namespace disco_host

extern "C" int disco_step2_cov_fused_reuse(disco_ctx* ctx, const disco_c32* X, const float* mask_w, const disco_c32* w_loc,
                                           disco_c32* z_out, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!step1_any(ctx) || ctx->cfg.nodes < 2 || ctx->Kl != ctx->cfg.nodes)
        return fail(ctx, DISCO_E_ARG, "disco_step2_cov_fused_reuse: no step-1 partial sums of disco_stft_cov_fused are held by this context");
    if (!step1_held(ctx, X, mask_w))
        return fail(ctx, DISCO_E_ARG, "disco_step2_cov_fused_reuse: X / mask_w are not the arrays the held step-1 partial sums were computed from");
    return step2_cov_partials(ctx, X, mask_w, w_loc, z_out, s, LeadBlock::Step1, XLayout::Public);
}
extern "C" int disco_step2_cov_fused(disco_ctx* ctx, const disco_c32* X, const float* mask_w, const disco_c32* w_loc,
                                     disco_c32* z_out, disco_c32* Rss, disco_c32* Rnn, disco_stream s) {
    DISCO_ENTER(ctx);
    return cov_pass_entry(ctx, "disco_step2_cov_fused", Rss, Rnn, s,
                          [&] { return step2_cov_partials(ctx, X, mask_w, w_loc, z_out, s, LeadBlock::Accumulate, XLayout::Public); });
}

// test-only: the same passes reading X in the packed workspace layout (include/disco_hip.h)
extern "C" int disco_selftest_step2_cov_packed(disco_ctx* ctx, const disco_c32* X, const float* mask_w, const disco_c32* w_loc,
                                               disco_c32* z_out, disco_c32* Rss, disco_c32* Rnn, int reuse, disco_stream s) {
    DISCO_ENTER(ctx);
    const char* refusal = "disco_selftest_step2_cov_packed: Rss and Rnn must both be given or both be NULL, and NULL with reuse";
    if (reuse && (Rss || Rnn)) return fail(ctx, DISCO_E_ARG, refusal);
    return cov_pass_entry(ctx, "disco_selftest_step2_cov_packed", Rss, Rnn, s, [&] {
        if (reuse && (!step1_any(ctx) || ctx->cfg.nodes < 2 || ctx->Kl != ctx->cfg.nodes || !step1_held(ctx, X, mask_w)))
            return fail(ctx, DISCO_E_ARG, "disco_selftest_step2_cov_packed: no step-1 partial sums of X / mask_w are held by this context");
        return step2_cov_partials(ctx, X, mask_w, w_loc, z_out, s, reuse ? LeadBlock::Step1 : LeadBlock::Accumulate, XLayout::Packed);
    }, refusal);
}
