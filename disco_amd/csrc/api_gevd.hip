// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): rank-R GEVD-MWF solves (k_gevd_full.h)
#include "host.h"
#include "k_gevd_full.h"

using namespace disco;
using namespace disco_host;

template <int P>
static void launch_gevd_full(const c32* Rxx, const c32* Rnn, long long n_prob, int r, double mu, c32* w, c32* t1, hipStream_t s) {
    if constexpr (P <= 4) {
        constexpr int THREADS = 128;
        const long long grid = (n_prob + THREADS - 1) / THREADS;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gevd_full_thread<P>), dim3((unsigned)grid), dim3(THREADS), 0, s, Rxx, Rnn, n_prob, r, mu, w, t1);
    } else {
        const int probs = SolveGeom<P>::PROBS;
        const long long grid = (n_prob + probs - 1) / probs;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gevd_full_group<P>), dim3((unsigned)grid), dim3(SolveGeom<P>::THREADS), 0, s, Rxx, Rnn, n_prob, r,
                           mu, w, t1);
    }
}

extern "C" int disco_gevd_mwf(disco_ctx* ctx, const disco_c32* Rxx, const disco_c32* Rnn, int64_t n_prob, int P, int rank, float mu,
                              disco_c32* w, disco_c32* t1, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!Rxx || !Rnn || !w || n_prob < 1) return fail(ctx, DISCO_E_ARG, "disco_gevd_mwf: bad argument");
    if (rank < 0) return fail(ctx, DISCO_E_ARG, "disco_gevd_mwf: rank must be >= 0 (map the reference's negative ranks first)");
    if (P < 1 || P > 16) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_gevd_mwf: P must be in 1..16");
    if (n_prob / 4 > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_gevd_mwf: batch too large");
    const int r = rank < P ? rank : P;
    const c32* a = (const c32*)Rxx;
    const c32* b = (const c32*)Rnn;
    hipStream_t st = (hipStream_t)s;
    for_int<1, 16>(P, [&](auto p) { launch_gevd_full<decltype(p)::value>(a, b, n_prob, r, (double)mu, (c32*)w, (c32*)t1, st); });
    return check_launch(ctx, "k_gevd_full");
}
