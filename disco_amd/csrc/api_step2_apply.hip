// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): step 2 with the z exchange on chip: filter
#include "step2_launch.h"

using namespace disco;
using namespace disco_host;

extern "C" int disco_step2_apply_fused(disco_ctx* ctx, const disco_c32* X, const disco_c32* w_loc, const disco_c32* w_glo,
                                       disco_c32* z_out, disco_c32* yf, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!X || !w_loc || !w_glo || !yf) return fail(ctx, DISCO_E_ARG, "disco_step2_apply_fused: null argument");
    if (sharded(ctx)) return fail(ctx, DISCO_E_UNSUPPORTED, "fused kernels need every node of a room on this GPU (node shard active)");
    const disco_cfg& c = ctx->cfg;
    const int M = c.mics, K = c.nodes, P = M + K - 1;
    if (P > 8) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_apply_fused: M + K - 1 > 8 not supported yet");
    const int tiles = (ctx->F - 1) / 64;
    const Step2Args a = step2_args(ctx, X, nullptr, w_loc, w_glo, z_out, yf, nullptr, step2_chunks(ctx, tiles + 1));
    const long long nblk = (long long)c.rooms * (tiles + 1) * a.chunks;
    if (nblk > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_apply_fused: batch too large");
    const bool found = for_mkr(M, K - 1, [&](auto m, auto kr) {
        constexpr int M_ = decltype(m)::value, K_ = decltype(kr)::value + 1;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_step2_apply_fused<M_, K_>), dim3((unsigned)nblk), dim3(64 * K_), 0, (hipStream_t)s, a);
    });
    if (!found) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_step2_apply_fused: unsupported (M, K) combination");
    return check_launch(ctx, "k_step2_apply_fused");
}
