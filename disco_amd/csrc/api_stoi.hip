// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): STOI of (clean, processed) signal pairs
#include "host.h"
#include "k_stoi.h"

using namespace disco;
using namespace disco_host;

namespace {

struct StoiLayout {
    size_t tw, wf, wd, xr, yr, E, idx, nk, tob_x, tob_y, part, total;
    int n10max, nfmax, tmax, n_chunk;
};
// sized by the longest span a pair of the batch can have (stop = len)
StoiLayout stoi_layout(long long n_pair, long long len, int start, int p, int q) {
    StoiLayout l{};
    const int n = len > start ? (int)(len - start) : 0;
    l.n10max = stoi_len10(n, p, q);
    l.nfmax = stoi_frames(l.n10max);
    l.tmax = std::max(l.nfmax - 1, 0);
    const long long items = (long long)std::max(l.tmax - (STOI_SEG - 1), 0) * STOI_BANDS;
    l.n_chunk = (int)((items + STOI_THREADS - 1) / STOI_THREADS);
    const size_t np = (size_t)n_pair;
    const size_t sig = p == q ? 0 : np * (size_t)l.n10max * sizeof(float);
    size_t off = 0;
    l.tw = off, off += align_up(STOI_TW_BYTES);
    l.wf = off, off += align_up(STOI_WF_BYTES);
    l.wd = off, off += align_up(STOI_WD_BYTES);
    l.xr = off, off += align_up(sig);
    l.yr = off, off += align_up(sig);
    l.E = off, off += align_up(np * (size_t)l.nfmax * sizeof(double));
    l.idx = off, off += align_up(np * (size_t)l.nfmax * sizeof(int));
    l.nk = off, off += align_up(np * sizeof(int));
    l.tob_x = off, off += align_up(np * STOI_BANDS * (size_t)l.tmax * sizeof(float));
    l.tob_y = off, off += align_up(np * STOI_BANDS * (size_t)l.tmax * sizeof(float));
    l.part = off, off += align_up(np * (size_t)l.n_chunk * sizeof(double));
    l.total = off;
    return l;
}

bool stoi_shape_ok(long long n_pair, long long len, int p, int q, int n_taps) {
    if (n_pair < 1 || len < 1 || p < 1 || q < 1) return false;
    if (p != q && (n_taps < 1 || n_taps > STOI_MAX_TAPS || !(n_taps & 1))) return false;
    return len <= 0x3fffffffLL && len * p / q <= 0x3fffffffLL;
}

}  // namespace

extern "C" size_t disco_stoi_workspace_bytes(const disco_ctx* ctx, int64_t n_pair, int64_t len, int p, int q, int n_taps) {
    (void)ctx;
    if (!stoi_shape_ok(n_pair, len, p, q, n_taps)) return 0;
    return stoi_layout(n_pair, len, 0, p, q).total;
}

extern "C" int disco_stoi(disco_ctx* ctx, const float* x, const float* y, int64_t n_pair, int64_t len, int start, const int32_t* stop, int p, int q,
                          const double* taps, int n_taps, double* out, int32_t* status, void* workspace, size_t workspace_bytes, disco_stream s) {
    DISCO_ENTER(ctx);
    if (n_pair < 1 || len < 1 || p < 1 || q < 1) return fail(ctx, DISCO_E_ARG, "disco_stoi: bad argument");
    if (p != q && n_taps > STOI_MAX_TAPS) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_stoi: resampling filters of at most 65536 taps");
    if (p != q && (n_taps < 1 || !(n_taps & 1) || !taps)) return fail(ctx, DISCO_E_ARG, "disco_stoi: resampling needs an odd number of taps (2 L + 1)");
    if (!stoi_shape_ok(n_pair, len, p, q, n_taps)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_stoi: signals of at most 2^30 samples, before and after resampling");
    if (!x || !y || !out || !status || !workspace) return fail(ctx, DISCO_E_ARG, "disco_stoi: bad argument");
    if (start < 0 || start > len) return fail(ctx, DISCO_E_ARG, "disco_stoi: need 0 <= start <= len");
    const StoiLayout l = stoi_layout(n_pair, len, start, p, q);
    if (workspace_bytes < stoi_layout(n_pair, len, 0, p, q).total) return fail(ctx, DISCO_E_ARG, "disco_stoi: workspace smaller than disco_stoi_workspace_bytes");
    const bool rs = p != q;
    const int nblk = (l.n10max + STOI_THREADS - 1) / STOI_THREADS;
    const long long n_items = (long long)n_pair * l.tmax;
    if (n_pair * 2 * std::max(nblk, 1) > 0x7fffffffLL || n_items > 0x7fffffffLL || n_pair * std::max(l.n_chunk, 1) > 0x7fffffffLL)
        return fail(ctx, DISCO_E_UNSUPPORTED, "disco_stoi: batch too large");
    char* ws = (char*)workspace;
    c32* tw = (c32*)(ws + l.tw);
    float *wf = (float*)(ws + l.wf), *xr = (float*)(ws + l.xr), *yr = (float*)(ws + l.yr), *tob_x = (float*)(ws + l.tob_x), *tob_y = (float*)(ws + l.tob_y);
    double *wd = (double*)(ws + l.wd), *E = (double*)(ws + l.E), *part = (double*)(ws + l.part);
    int *idx = (int*)(ws + l.idx), *nk = (int*)(ws + l.nk);
    hipStream_t st = (hipStream_t)s;
    // the 10-kHz signals the later stages read: the resampled rows, or the caller's own from `start`
    const float *sx = rs ? xr : x, *sy = rs ? yr : y;
    const long long stride = rs ? l.n10max : len;
    const int off = rs ? 0 : start;
    if (rs && l.n10max > 0) {
        StageScope stage_scope_(ctx, s, "stoi_resample");
        hipLaunchKernelGGL(k_stoi_resample, dim3((unsigned)(n_pair * 2 * nblk)), dim3(STOI_THREADS), 0, st, x, y, (long long)len, start, (const int*)stop, p, q,
                           taps, n_taps, l.n10max, nblk, xr, yr);
        if (int rc = check_launch(ctx, "k_stoi_resample")) return rc;
    }
    {
        StageScope stage_scope_(ctx, s, "stoi_frames");
        hipLaunchKernelGGL(k_stoi_tables, dim3(1), dim3(STOI_THREADS), 0, st, tw, wf, wd);
        if (int rc = check_launch(ctx, "k_stoi_tables")) return rc;
        hipLaunchKernelGGL(k_stoi_frames, dim3((unsigned)n_pair), dim3(STOI_FR_THREADS), 0, st, sx, stride, off, (long long)len, start, (const int*)stop, p, q,
                           (const double*)wd, l.nfmax, E, idx, nk);
        if (int rc = check_launch(ctx, "k_stoi_frames")) return rc;
    }
    if (n_items > 0) {
        StageScope stage_scope_(ctx, s, "stoi_tob");
        const unsigned grid = (unsigned)((n_items + STOI_THREADS / 64 - 1) / (STOI_THREADS / 64));
        hipLaunchKernelGGL(k_stoi_tob, dim3(grid), dim3(STOI_THREADS), 0, st, sx, sy, stride, off, (const c32*)tw, (const float*)wf, (const int*)idx,
                           (const int*)nk, l.nfmax, l.tmax, n_items, tob_x, tob_y);
        if (int rc = check_launch(ctx, "k_stoi_tob")) return rc;
    }
    {
        StageScope stage_scope_(ctx, s, "stoi_corr");
        if (l.n_chunk > 0) {
            hipLaunchKernelGGL(k_stoi_corr, dim3((unsigned)(n_pair * l.n_chunk)), dim3(STOI_THREADS), 0, st, (const float*)tob_x, (const float*)tob_y,
                               (const int*)nk, l.tmax, l.n_chunk, part);
            if (int rc = check_launch(ctx, "k_stoi_corr")) return rc;
        }
        hipLaunchKernelGGL(k_stoi_finish, dim3((unsigned)((n_pair + STOI_THREADS - 1) / STOI_THREADS)), dim3(STOI_THREADS), 0, st, (const double*)part,
                           (const int*)nk, l.n_chunk, (long long)len, start, (const int*)stop, p, q, (long long)n_pair, out, (int*)status);
        if (int rc = check_launch(ctx, "k_stoi_finish")) return rc;
    }
    return 0;
}
