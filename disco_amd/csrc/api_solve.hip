// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): rank-1 GEVD-MWF solves
#include "host.h"
#include "k_solve.h"
#include "k_solve_small.h"
#include "k_solve_wide.h"

using namespace disco;
using namespace disco_host;

namespace disco_host {
// api_solve_dpp.hip: 9 <= P <= 16 in registers (k_solve_dpp.h)
void launch_solve_dpp(int P, const SolveSrc& src, long long n_prob, double mu, c32* w, c32* t1, hipStream_t s);
}

template <int P>
static void launch_solve(const SolveSrc& src, long long n_prob, double mu, c32* w, c32* t1, hipStream_t s, bool thread) {
    if (P <= 4 || (P <= 8 && thread)) {             // one thread per pencil (k_solve_small.h)
        if constexpr (P <= 8) {
        constexpr int SOLVE_SMALL_THREADS = solve_small_threads<P>();
        const long long grid = (n_prob + SOLVE_SMALL_THREADS - 1) / SOLVE_SMALL_THREADS;
        with_bool(src.part != nullptr, [&](auto part) {
            constexpr bool FROM_PART = decltype(part)::value;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gevd_mwf_r1_thread<P, FROM_PART>), dim3((unsigned)grid), dim3(SOLVE_SMALL_THREADS), 0, s, src,
                               n_prob, mu, w, t1);
        });
        }
        return;
    }
    if constexpr (P >= 5) {
    const int probs = SolveGeom<P>::PROBS;
    const long long grid = (n_prob + probs - 1) / probs;
    with_bool(src.part != nullptr, [&](auto part) {
        constexpr bool FROM_PART = decltype(part)::value;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gevd_mwf_r1<P, FROM_PART>), dim3((unsigned)grid), dim3(SolveGeom<P>::THREADS), 0, s, src, n_prob,
                           mu, w, t1);
    });
    }
}

static int solve_dispatch(disco_ctx* ctx, const SolveSrc& src, int64_t n_prob, int P, float mu, disco_c32* w, disco_c32* t1,
                          disco_stream s) {
    if (P < 1 || P > SW_PMAX) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_gevd_mwf_r1: P must be in 1..32");
    if (n_prob / 4 > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_gevd_mwf_r1: batch too large");
    hipStream_t st = (hipStream_t)s;
    if (P >= SW_PMIN) {                          // 17 <= P <= 32: one wave per pencil (k_solve_wide.h)
        if (n_prob > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_gevd_mwf_r1: batch too large (P > 16: at most 2^31 - 1 pencils)");
        if (src.part_loc) return fail(ctx, DISCO_E_ARG, "disco_gevd_mwf_r1: P > 16 takes no re-used step-1 block");
        with_bool(src.part != nullptr, [&](auto part) {
            constexpr bool FROM_PART = decltype(part)::value;
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gevd_mwf_r1_wide<FROM_PART>), dim3((unsigned)n_prob), dim3(64), 0, st, src, (long long)n_prob, P,
                               (double)mu, (c32*)w, (c32*)t1);
        });
        return check_launch(ctx, "k_gevd_mwf_r1_wide");
    }
    if (P >= 9 && ctx->opt[DISCO_OPT_SOLVE_DPP] != 0) {
        launch_solve_dpp(P, src, n_prob, (double)mu, (c32*)w, (c32*)t1, st);
        return check_launch(ctx, "k_gevd_mwf_r1_dpp");
    }
    for_int<1, 16>(P, [&](auto p) {
        launch_solve<decltype(p)::value>(src, n_prob, (double)mu, (c32*)w, (c32*)t1, st, ctx->opt[DISCO_OPT_SOLVE_THREAD] != 0);
    });
    return check_launch(ctx, "k_gevd_mwf_r1");
}

extern "C" int disco_gevd_mwf_r1(disco_ctx* ctx, const disco_c32* Rss, const disco_c32* Rnn, int64_t n_prob, int P,
                                 float mu, disco_c32* w, disco_c32* t1, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!Rss || !Rnn || !w || n_prob < 1) return fail(ctx, DISCO_E_ARG, "disco_gevd_mwf_r1: bad argument");
    return solve_dispatch(ctx, SolveSrc::matrices((const c32*)Rss, (const c32*)Rnn), n_prob, P, mu, w, t1, s);
}
extern "C" int disco_gevd_mwf_r1_pending(disco_ctx* ctx, float mu, disco_c32* w, disco_c32* t1, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!w) return fail(ctx, DISCO_E_ARG, "disco_gevd_mwf_r1_pending: null argument");
    PendingSums ps;
    if (!partials_pending(ctx, &ps))
        return fail(ctx, DISCO_E_ARG, "disco_gevd_mwf_r1_pending: no covariance call has left partial sums in this context");
    return solve_dispatch(ctx, SolveSrc::pending(ps, ctx->F), (int64_t)ctx->cfg.rooms * ctx->Kl * ctx->F, ps.P, mu, w, t1, s);
}
