// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): step 2 with the z exchange on chip: filter + iSTFT
#include "step2_launch.h"

using namespace disco;
using namespace disco_host;

// the kernel's tile within the 160 KiB LDS?
template <int M, int K>
constexpr bool apply_istft_fits = sizeof(ApplyIstftShared<512, M, K>) <= 160 * 1024;

// frame pairs per run of a workgroup (k_step2_apply_istft) or of a wave (k_stft_apply_istft): as many as possible (<= 64) while leaving
// >= ~8192 waves (one per node and run); *runs: the runs of 2 pairs - 1 hop segments that cover the clip
static int frame_pairs(const disco_ctx* ctx, int* runs) {
    const disco_cfg& c = ctx->cfg;
    const int n_seg = (c.length + c.hop - 1) / c.hop;
    const long long units = (long long)ctx->geom_rooms * c.nodes;
    const long long runs_wanted = std::max<long long>(1, (8192 + units - 1) / units);
    int pairs = (int)(((n_seg + runs_wanted - 1) / runs_wanted + 2) / 2);
    pairs = std::min(64, std::max(4, pairs));
    if (ctx->tune_pairs > 0) pairs = ctx->tune_pairs;
    *runs = (n_seg + 2 * pairs - 2) / (2 * pairs - 1);
    return pairs;
}

namespace disco_host {
// does disco_step2_apply_istft_fused take this context's shape?  (512-point STFT, P <= 8, the kernel's tile within the 160 KiB LDS)
bool step2_apply_istft_ok(const disco_ctx* ctx) {
    const disco_cfg& c = ctx->cfg;
    const int M = c.mics, K = c.nodes;
    if (c.n_fft != 512 || M + K - 1 > 8 || sharded(ctx)) return false;
    bool fits = false;
    for_mkr(M, K - 1, [&](auto m, auto kr) { fits = apply_istft_fits<decltype(m)::value, decltype(kr)::value + 1>; });
    return fits;
}
}  // namespace disco_host

extern "C" int disco_step2_apply_istft_fused(disco_ctx* ctx, const disco_c32* X, const disco_c32* w_loc,
                                             const disco_c32* w_glo, float* out, disco_stream s) {
    DISCO_ENTER(ctx);
    return step2_apply_istft(ctx, X, w_loc, w_glo, out, s, XLayout::Public);
}

int disco_host::step2_apply_istft(disco_ctx* ctx, const disco_c32* X, const disco_c32* w_loc, const disco_c32* w_glo, float* out, disco_stream s,
                                  XLayout layout) {
    if (!X || !w_loc || !w_glo || !out) return fail(ctx, DISCO_E_ARG, "disco_step2_apply_istft_fused: null argument");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "fused kernels need every node of a room on this GPU (node shard active)");
    const disco_cfg& c = ctx->cfg;
    const int M = c.mics, K = c.nodes, P = M + K - 1;
    if (c.n_fft != 512 || P > 8) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_apply_istft_fused: needs n_fft = 512 and M + K - 1 <= 8");
    const Step2Args a = step2_args(ctx, X, nullptr, w_loc, w_glo, nullptr, nullptr, nullptr, 1);
    int bpr = 0;
    const int pairs = frame_pairs(ctx, &bpr);
    const long long nblk = (long long)c.rooms * bpr;
    if (nblk > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_apply_istft_fused: batch too large");
    bool ran = false;
    for_mkr(M, K - 1, [&](auto m, auto kr) { with_bool(layout == XLayout::Packed, [&](auto pack) {
        constexpr int M_ = decltype(m)::value, K_ = decltype(kr)::value + 1;
        constexpr bool PACK = decltype(pack)::value;           // the packed workspace layout: the fused route of the whole path only (K >= 2)
        if constexpr (apply_istft_fits<M_, K_> && (!PACK || K_ >= 2)) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_step2_apply_istft<512, M_, K_, PACK>), dim3((unsigned)nblk), dim3(64 * K_), 0, (hipStream_t)s, a, out,
                               ctx->d_win, ctx->d_tw, c.length, bpr, pairs, ctx->d_lens);
            ran = true;
        }
    }); });
    if (!ran) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_apply_istft_fused: shape does not fit the LDS budget");
    return check_launch(ctx, "k_step2_apply_istft");
}

namespace disco_host {
// Single node, enhanced output only: iSTFT(w^H STFT(y)) straight from the samples (k_stft_apply_istft), 512-point STFT, M <= 4
int stft_apply_istft(disco_ctx* ctx, const float* y, const disco_c32* w, float* out, disco_stream s) {
    const disco_cfg& c = ctx->cfg;
    const long long G = (long long)c.rooms * c.nodes;
    int runs = 0;
    const int pairs = frame_pairs(ctx, &runs);
    const long long items = G * runs;
    if (stft_blocks(items) > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_tango_enhance: batch too large for one launch");
    const bool found = for_int<1, 4>(c.mics, [&](auto m) {
        constexpr int M_ = decltype(m)::value;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_stft_apply_istft<512, M_>), dim3((unsigned)stft_blocks(items)), dim3(64 * STFT_WAVES), 0,
                           (hipStream_t)s, y, (const c32*)w, out, ctx->d_win, ctx->d_tw, c.length, ctx->T, c.pad_mode, runs, pairs, items, ctx->d_lens,
                           c.nodes);
    });
    if (!found) return DISCO_E_UNSUPPORTED;
    return check_launch(ctx, "k_stft_apply_istft");
}
}  // namespace disco_host
