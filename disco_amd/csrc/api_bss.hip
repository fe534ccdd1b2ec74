// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): lag correlations and BSS-eval energies
#include "host.h"
#include "k_bss.h"

using namespace disco;
using namespace disco_host;

namespace {

int lag_chunks(int start, int stop) { return std::max(1, (stop - start + LC_SPAN - 1) / LC_SPAN); }

// lag correlations of n_pair pairs into out[n_pair][nlag] through part[n_pair][n_chunk][nlag].  stop_sig (device, one per pair or per
// set, or null): the chunks then cover [start, stop) with stop = len, the longest span a pair can have.
int launch_lag(disco_ctx* ctx, const float* a, const float* b, long long n_pair, long long len, int start, int stop, const int* stop_sig,
               int lag_lo, int nlag, int mode, int nsrc, int n_est, int kest, double* part, double* out, hipStream_t st) {
    const int n_chunk = lag_chunks(start, stop);
    hipLaunchKernelGGL(k_lag_corr, dim3((unsigned)(n_pair * n_chunk)), dim3(BSS_THREADS), 0, st, a, b, len, start, stop, stop_sig, lag_lo, nlag,
                       n_chunk, mode, nsrc, n_est, kest, part);
    if (int rc = check_launch(ctx, "k_lag_corr")) return rc;
    const long long total = n_pair * nlag;
    hipLaunchKernelGGL(k_lag_reduce, dim3(ew_grid(total)), dim3(BSS_THREADS), 0, st, (const double*)part, n_chunk, nlag, total, out);
    return check_launch(ctx, "k_lag_reduce");
}

struct BssLayout {
    size_t crr, cd, part, stat, g, total;
};
BssLayout bss_layout(long long n_set, int nsrc, int flen, long long len) {
    BssLayout l;
    const size_t corr = (size_t)n_set * nsrc * nsrc * flen * sizeof(double);
    const size_t n_chunk = (size_t)std::max<long long>(1, (len + LC_SPAN - 1) / LC_SPAN);
    size_t off = 0;
    l.crr = off, off += align_up(corr);
    l.cd = off, off += align_up(corr);
    l.part = off, off += align_up(corr * n_chunk);
    l.stat = off, off += align_up((size_t)n_set * nsrc * sizeof(int));
    l.g = off, off += align_up((size_t)n_set * (size_t)bss_set_words(nsrc, flen) * sizeof(double));
    l.total = off;
    return l;
}

}  // namespace

extern "C" size_t disco_lag_corr_workspace_bytes(const disco_ctx* ctx, int64_t n_pair, int64_t len, int n_lag) {
    (void)ctx;
    if (n_pair < 1 || len < 1 || n_lag < 1) return 0;
    return (size_t)n_pair * (size_t)((len + LC_SPAN - 1) / LC_SPAN) * (size_t)n_lag * sizeof(double);
}

// disco_lag_corr (stop_sig null) and disco_lag_corr_spans (stop = len, the chunk geometry of the longest span)
static int lag_corr_impl(disco_ctx* ctx, const float* a, const float* b, int64_t n_pair, int64_t len, int start, int stop, const int32_t* stop_sig,
                         int lag_lo, int lag_hi, double* out, void* workspace, size_t workspace_bytes, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!a || !b || !out || !workspace || n_pair < 1 || len < 1) return fail(ctx, DISCO_E_ARG, "disco_lag_corr: bad argument");
    if (start < 0 || stop > len || stop < start)
        return fail(ctx, DISCO_E_ARG, stop_sig ? "disco_lag_corr: need 0 <= start <= len" : "disco_lag_corr: need 0 <= start <= stop <= len");
    if (lag_lo > lag_hi) return fail(ctx, DISCO_E_ARG, "disco_lag_corr: need lag_lo <= lag_hi");
    if (lag_lo < -(BSS_MAX_FLEN - 1) || lag_hi > BSS_MAX_FLEN - 1) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_lag_corr: lags within +-511");
    if (len > 0x7fffffffLL - LC_SPAN - 2048) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_lag_corr: signals longer than 2^31 - 18432 samples");
    const int nlag = lag_hi - lag_lo + 1;
    if (n_pair * lag_chunks(start, stop) > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_lag_corr: batch too large");
    if (workspace_bytes < (size_t)n_pair * lag_chunks(start, stop) * nlag * sizeof(double))
        return fail(ctx, DISCO_E_ARG, "disco_lag_corr: workspace smaller than disco_lag_corr_workspace_bytes");
    return launch_lag(ctx, a, b, n_pair, len, start, stop, (const int*)stop_sig, lag_lo, nlag, 0, 1, 1, 0, (double*)workspace, out, (hipStream_t)s);
}

extern "C" int disco_lag_corr(disco_ctx* ctx, const float* a, const float* b, int64_t n_pair, int64_t len, int start, int stop, int lag_lo,
                              int lag_hi, double* out, void* workspace, size_t workspace_bytes, disco_stream s) {
    return lag_corr_impl(ctx, a, b, n_pair, len, start, stop, nullptr, lag_lo, lag_hi, out, workspace, workspace_bytes, s);
}

extern "C" int disco_lag_corr_spans(disco_ctx* ctx, const float* a, const float* b, int64_t n_pair, int64_t len, int start, const int32_t* stop,
                                    int lag_lo, int lag_hi, double* out, void* workspace, size_t workspace_bytes, disco_stream s) {
    if (ctx && len > 0x7fffffffLL - LC_SPAN - 2048) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_lag_corr: signals longer than 2^31 - 18432 samples");
    return lag_corr_impl(ctx, a, b, n_pair, len, start, (int)len, stop, lag_lo, lag_hi, out, workspace, workspace_bytes, s);
}

extern "C" size_t disco_bss_workspace_bytes(const disco_ctx* ctx, int64_t n_set, int nsrc, int flen, int64_t len) {
    (void)ctx;
    if (n_set < 1 || nsrc < 1 || nsrc > BSS_MAX_SRC || flen < 1 || flen > BSS_MAX_FLEN || len < 1) return 0;
    return bss_layout(n_set, nsrc, flen, len).total;
}

// disco_bss_eval (stop_sig null) and disco_bss_eval_spans (stop = len: chunks and the batch-size check from len - start)
static int bss_eval_impl(disco_ctx* ctx, const float* refs, const float* ests, int64_t n_set, int nsrc, int n_est, int64_t len, int start, int stop,
                         const int32_t* stop_set, int flen, int all_pairs, double* out, int32_t* status, void* workspace, size_t workspace_bytes,
                         disco_stream s) {
    DISCO_ENTER(ctx);
    const int* stop_sig = (const int*)stop_set;
    if (n_set < 1 || n_est < 1 || len < 1 || nsrc < 1 || flen < 1) return fail(ctx, DISCO_E_ARG, "disco_bss_eval: bad argument");
    if (nsrc > BSS_MAX_SRC) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_bss_eval: at most 4 sources (nsrc <= 4)");
    if (flen > BSS_MAX_FLEN) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_bss_eval: filters of at most 512 taps (flen <= 512)");
    if (!refs || !ests || !out || !status || !workspace) return fail(ctx, DISCO_E_ARG, "disco_bss_eval: bad argument");
    if (start < 0 || stop > len || stop < start)
        return fail(ctx, DISCO_E_ARG, stop_sig ? "disco_bss_eval: need 0 <= start <= len" : "disco_bss_eval: need 0 <= start <= stop <= len");
    if (len > 0x7fffffffLL - LC_SPAN - 2048) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_bss_eval: signals longer than 2^31 - 18432 samples");
    const long long n_pair = (long long)n_set * nsrc * nsrc;
    if (n_pair * lag_chunks(start, stop) > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_bss_eval: batch too large");
    const BssLayout l = bss_layout(n_set, nsrc, flen, len);
    if (workspace_bytes < l.total) return fail(ctx, DISCO_E_ARG, "disco_bss_eval: workspace smaller than disco_bss_workspace_bytes");
    char* ws = (char*)workspace;
    double *crr = (double*)(ws + l.crr), *cd = (double*)(ws + l.cd), *part = (double*)(ws + l.part), *g = (double*)(ws + l.g);
    int* stat = (int*)(ws + l.stat);
    hipStream_t st = (hipStream_t)s;
    const long long set_words = bss_set_words(nsrc, flen);
    if (int rc = STAGE(ctx, s, "bss_corr", launch_lag(ctx, refs, refs, n_pair, len, start, stop, stop_sig, 0, flen, 1, nsrc, n_est, 0, part, crr, st))) return rc;
    {
        StageScope stage_scope_(ctx, s, "bss_factor");
        hipLaunchKernelGGL(k_bss_factor, dim3((unsigned)(n_set * nsrc)), dim3(BSS_THREADS), 0, st, (const double*)crr, g, set_words, nsrc, flen, stat);
        if (int rc = check_launch(ctx, "k_bss_factor")) return rc;
    }
    const int ngrp = (nsrc + PJ_RHS - 1) / PJ_RHS;
    for (int k = 0; k < n_est; ++k) {
        if (int rc = STAGE(ctx, s, "bss_corr", launch_lag(ctx, refs, ests, n_pair, len, start, stop, stop_sig, 0, flen, 2, nsrc, n_est, k, part, cd, st))) return rc;
        StageScope stage_scope_(ctx, s, "bss_project");
        hipLaunchKernelGGL(k_bss_project, dim3((unsigned)(n_set * nsrc * ngrp)), dim3(BSS_THREADS), 0, st, (const double*)cd, (const double*)g, set_words,
                           (const int*)stat, ests, (long long)len, start, stop, stop_sig, nsrc, flen, n_est, k, all_pairs ? 1 : 0, out, (int*)status);
        if (int rc = check_launch(ctx, "k_bss_project")) return rc;
    }
    return 0;
}

extern "C" int disco_bss_eval(disco_ctx* ctx, const float* refs, const float* ests, int64_t n_set, int nsrc, int n_est, int64_t len, int start,
                              int stop, int flen, int all_pairs, double* out, int32_t* status, void* workspace, size_t workspace_bytes,
                              disco_stream s) {
    return bss_eval_impl(ctx, refs, ests, n_set, nsrc, n_est, len, start, stop, nullptr, flen, all_pairs, out, status, workspace, workspace_bytes, s);
}

extern "C" int disco_bss_eval_spans(disco_ctx* ctx, const float* refs, const float* ests, int64_t n_set, int nsrc, int n_est, int64_t len, int start,
                                    const int32_t* stop, int flen, int all_pairs, double* out, int32_t* status, void* workspace,
                                    size_t workspace_bytes, disco_stream s) {
    if (ctx && len > 0x7fffffffLL - LC_SPAN - 2048) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_bss_eval: signals longer than 2^31 - 18432 samples");
    return bss_eval_impl(ctx, refs, ests, n_set, nsrc, n_est, len, start, (int)len, stop, flen, all_pairs, out, status, workspace, workspace_bytes, s);
}

extern "C" int disco_bss_estimates(disco_ctx* ctx, const float* y, const float* sh, const float* szh, int64_t n_sig, int64_t len, int start,
                                   const int32_t* stop, float* ests, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!y || !sh || !szh || !ests || n_sig < 1 || len < 1) return fail(ctx, DISCO_E_ARG, "disco_bss_estimates: bad argument");
    if (start < 0 || start > len) return fail(ctx, DISCO_E_ARG, "disco_bss_estimates: need 0 <= start <= len");
    if (len > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_bss_estimates: signals longer than 2^31 - 1 samples");
    const long long tiles = (long long)n_sig * ((len + BE_TILE - 1) / BE_TILE);
    hipLaunchKernelGGL(k_bss_estimates, dim3((unsigned)std::min<long long>(tiles, 1 << 16)), dim3(BSS_THREADS), 0, (hipStream_t)s, y, sh, szh,
                       (long long)n_sig, (long long)len, start, (int)len, (const int*)stop, ests);
    return check_launch(ctx, "k_bss_estimates");
}
