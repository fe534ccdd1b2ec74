// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): intern_filter's other two branches
#include "host.h"
#include "k_solve.h"

using namespace disco;
using namespace disco_host;

// The two branches of intern_filter the hot path never takes (see k_mwf_variants)
extern "C" int disco_mwf_filter(disco_ctx* ctx, const disco_c32* Rxx, const disco_c32* Rnn, int64_t n_prob, int P, float mu,
                                int type, disco_c32* w, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!Rxx || !Rnn || !w || n_prob < 1) return fail(ctx, DISCO_E_ARG, "disco_mwf_filter: bad argument");
    if (type != DISCO_FILTER_R1_MWF && type != DISCO_FILTER_MWF) return fail(ctx, DISCO_E_ARG, "disco_mwf_filter: unknown filter type");
    if (P < 1 || P > 16) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_mwf_filter: P must be in 1..16");
    if (n_prob / 4 > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_mwf_filter: batch too large");
    hipStream_t st = (hipStream_t)s;
    for_int<1, 16>(P, [&](auto p) { with_bool(type == DISCO_FILTER_MWF, [&](auto mwf) {
        constexpr int P_ = decltype(p)::value, TYPE = decltype(mwf)::value ? FILTER_MWF : FILTER_R1_MWF;
        using Geom = SolveGeom<P_>;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mwf_variants<P_, TYPE>),
                           dim3((unsigned)((n_prob + Geom::PROBS - 1) / Geom::PROBS)), dim3(Geom::THREADS), 0, st, (const c32*)Rxx, (const c32*)Rnn,
                           (long long)n_prob, (double)mu, (c32*)w);
    }); });
    return check_launch(ctx, "k_mwf_variants");
}
