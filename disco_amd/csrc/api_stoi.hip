// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): STOI and ESTOI of (clean, processed) signal pairs
#include "host.h"
#include "k_estoi.h"

using namespace disco;
using namespace disco_host;

namespace {

static_assert(ESTOI_SEGS == DISCO_ESTOI_SEGS, "include/disco_hip.h states the segments per workgroup of k_estoi_corr");

struct StoiLayout {
    size_t tw, wf, wd, xr, yr, E, idx, nk, tob_x, tob_y, part, total;
    int n10max, nfmax, tmax, n_chunk;
};

// workgroups of k_estoi_corr per pair of at most tmax frames
int estoi_chunks(int tmax) { return (std::max(tmax - (STOI_SEG - 1), 0) + ESTOI_SEGS - 1) / ESTOI_SEGS; }

// sized by the longest span a pair of the batch can have (stop = len); extended: the partial sums of k_estoi_corr in place of k_stoi_corr's
StoiLayout stoi_layout(long long n_pair, long long len, int start, int p, int q, bool extended) {
    StoiLayout l{};
    const int n = len > start ? (int)(len - start) : 0;
    l.n10max = stoi_len10(n, p, q);
    l.nfmax = stoi_frames(l.n10max);
    l.tmax = std::max(l.nfmax - 1, 0);
    const long long items = (long long)std::max(l.tmax - (STOI_SEG - 1), 0) * STOI_BANDS;
    l.n_chunk = extended ? estoi_chunks(l.tmax) : (int)((items + STOI_THREADS - 1) / STOI_THREADS);
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

int fail_as(disco_ctx* ctx, int code, const char* who, const char* msg) {
    char text[192];
    snprintf(text, sizeof(text), "%s: %s", who, msg);
    return fail(ctx, code, text);
}

// the pointers of a workspace laid out by stoi_layout
struct StoiBuffers {
    c32* tw;
    float *wf, *xr, *yr, *tob_x, *tob_y;
    double *wd, *E, *part;
    int *idx, *nk;
    StoiBuffers(void* workspace, const StoiLayout& l) {
        char* ws = (char*)workspace;
        tw = (c32*)(ws + l.tw);
        wf = (float*)(ws + l.wf), xr = (float*)(ws + l.xr), yr = (float*)(ws + l.yr), tob_x = (float*)(ws + l.tob_x), tob_y = (float*)(ws + l.tob_y);
        wd = (double*)(ws + l.wd), E = (double*)(ws + l.E), part = (double*)(ws + l.part);
        idx = (int*)(ws + l.idx), nk = (int*)(ws + l.nk);
    }
};

// The refusals disco_stoi and disco_estoi share, each under its own name `who` (`ws_name`: its workspace query, for the message);
// on success *l is the layout of the call.
int stoi_check(disco_ctx* ctx, const char* who, const char* ws_name, bool extended, const float* x, const float* y, int64_t n_pair, int64_t len,
               int start, int p, int q, const double* taps, int n_taps, double* out, int32_t* status, void* workspace, size_t workspace_bytes,
               StoiLayout* l) {
    if (n_pair < 1 || len < 1 || p < 1 || q < 1) return fail_as(ctx, DISCO_E_ARG, who, "bad argument");
    if (p != q && n_taps > STOI_MAX_TAPS) return fail_as(ctx, DISCO_E_UNSUPPORTED, who, "resampling filters of at most 65536 taps");
    if (p != q && (n_taps < 1 || !(n_taps & 1) || !taps)) return fail_as(ctx, DISCO_E_ARG, who, "resampling needs an odd number of taps (2 L + 1)");
    if (!stoi_shape_ok(n_pair, len, p, q, n_taps)) return fail_as(ctx, DISCO_E_UNSUPPORTED, who, "signals of at most 2^30 samples, before and after resampling");
    if (!x || !y || !out || !status || !workspace) return fail_as(ctx, DISCO_E_ARG, who, "bad argument");
    if (start < 0 || start > len) return fail_as(ctx, DISCO_E_ARG, who, "need 0 <= start <= len");
    *l = stoi_layout(n_pair, len, start, p, q, extended);
    if (workspace_bytes < stoi_layout(n_pair, len, 0, p, q, extended).total) {
        char msg[96];
        snprintf(msg, sizeof(msg), "workspace smaller than %s", ws_name);
        return fail_as(ctx, DISCO_E_ARG, who, msg);
    }
    const int nblk = (l->n10max + STOI_THREADS - 1) / STOI_THREADS;
    if (n_pair * 2 * std::max(nblk, 1) > 0x7fffffffLL || (long long)n_pair * l->tmax > 0x7fffffffLL || n_pair * std::max(l->n_chunk, 1) > 0x7fffffffLL)
        return fail_as(ctx, DISCO_E_UNSUPPORTED, who, "batch too large");
    return 0;
}

// Stages 1 - 3 of k_stoi.h, what STOI and ESTOI share: both signals to 10 kHz, the kept frames of x, the third-octave envelopes of the kept
// frame pairs -> b.nk [pair], b.tob_x, b.tob_y [pair][15][l.tmax]
int stoi_stages(disco_ctx* ctx, const float* x, const float* y, int64_t n_pair, int64_t len, int start, const int32_t* stop, int p, int q,
                const double* taps, int n_taps, const StoiLayout& l, const StoiBuffers& b, disco_stream s) {
    const bool rs = p != q;
    const int nblk = (l.n10max + STOI_THREADS - 1) / STOI_THREADS;
    const long long n_items = (long long)n_pair * l.tmax;
    hipStream_t st = (hipStream_t)s;
    // the 10-kHz signals the later stages read: the resampled rows, or the caller's own from `start`
    const float *sx = rs ? b.xr : x, *sy = rs ? b.yr : y;
    const long long stride = rs ? l.n10max : len;
    const int off = rs ? 0 : start;
    if (rs && l.n10max > 0) {
        StageScope stage_scope_(ctx, s, "stoi_resample");
        hipLaunchKernelGGL(k_stoi_resample, dim3((unsigned)(n_pair * 2 * nblk)), dim3(STOI_THREADS), 0, st, x, y, (long long)len, start, (const int*)stop, p, q,
                           taps, n_taps, l.n10max, nblk, b.xr, b.yr);
        if (int rc = check_launch(ctx, "k_stoi_resample")) return rc;
    }
    {
        StageScope stage_scope_(ctx, s, "stoi_frames");
        hipLaunchKernelGGL(k_stoi_tables, dim3(1), dim3(STOI_THREADS), 0, st, b.tw, b.wf, b.wd);
        if (int rc = check_launch(ctx, "k_stoi_tables")) return rc;
        hipLaunchKernelGGL(k_stoi_frames, dim3((unsigned)n_pair), dim3(STOI_FR_THREADS), 0, st, sx, stride, off, (long long)len, start, (const int*)stop, p, q,
                           (const double*)b.wd, l.nfmax, b.E, b.idx, b.nk);
        if (int rc = check_launch(ctx, "k_stoi_frames")) return rc;
    }
    if (n_items > 0) {
        StageScope stage_scope_(ctx, s, "stoi_tob");
        const unsigned grid = (unsigned)((n_items + STOI_THREADS / 64 - 1) / (STOI_THREADS / 64));
        hipLaunchKernelGGL(k_stoi_tob, dim3(grid), dim3(STOI_THREADS), 0, st, sx, sy, stride, off, (const c32*)b.tw, (const float*)b.wf, (const int*)b.idx,
                           (const int*)b.nk, l.nfmax, l.tmax, n_items, b.tob_x, b.tob_y);
        if (int rc = check_launch(ctx, "k_stoi_tob")) return rc;
    }
    return 0;
}

// The last stage of ESTOI: envelopes [pair][15][tmax] with T = frames[pair] - sub frames each (tmax without `frames`) -> out, status
int estoi_last_stage(disco_ctx* ctx, const float* tob_x, const float* tob_y, int64_t n_pair, int tmax, const int* frames, int sub, int n_chunk,
                     double* part, int spans, int64_t len, int start, const int32_t* stop, int p, int q, double* out, int32_t* status, disco_stream s) {
    hipStream_t st = (hipStream_t)s;
    StageScope stage_scope_(ctx, s, "estoi_corr");
    if (n_chunk > 0) {
        hipLaunchKernelGGL(k_estoi_corr, dim3((unsigned)(n_pair * n_chunk)), dim3(STOI_THREADS), 0, st, tob_x, tob_y, frames, sub, tmax, n_chunk, part);
        if (int rc = check_launch(ctx, "k_estoi_corr")) return rc;
    }
    hipLaunchKernelGGL(k_estoi_finish, dim3((unsigned)((n_pair + STOI_THREADS - 1) / STOI_THREADS)), dim3(STOI_THREADS), 0, st, (const double*)part, frames, sub,
                       tmax, n_chunk, spans, (long long)len, start, (const int*)stop, p, q, (long long)n_pair, out, (int*)status);
    return check_launch(ctx, "k_estoi_finish");
}

}  // namespace

extern "C" size_t disco_stoi_workspace_bytes(const disco_ctx* ctx, int64_t n_pair, int64_t len, int p, int q, int n_taps) {
    (void)ctx;
    if (!stoi_shape_ok(n_pair, len, p, q, n_taps)) return 0;
    return stoi_layout(n_pair, len, 0, p, q, false).total;
}

extern "C" int disco_stoi(disco_ctx* ctx, const float* x, const float* y, int64_t n_pair, int64_t len, int start, const int32_t* stop, int p, int q,
                          const double* taps, int n_taps, double* out, int32_t* status, void* workspace, size_t workspace_bytes, disco_stream s) {
    DISCO_ENTER(ctx);
    StoiLayout l;
    if (int rc = stoi_check(ctx, "disco_stoi", "disco_stoi_workspace_bytes", false, x, y, n_pair, len, start, p, q, taps, n_taps, out, status, workspace,
                            workspace_bytes, &l))
        return rc;
    const StoiBuffers b(workspace, l);
    if (int rc = stoi_stages(ctx, x, y, n_pair, len, start, stop, p, q, taps, n_taps, l, b, s)) return rc;
    hipStream_t st = (hipStream_t)s;
    {
        StageScope stage_scope_(ctx, s, "stoi_corr");
        if (l.n_chunk > 0) {
            hipLaunchKernelGGL(k_stoi_corr, dim3((unsigned)(n_pair * l.n_chunk)), dim3(STOI_THREADS), 0, st, (const float*)b.tob_x, (const float*)b.tob_y,
                               (const int*)b.nk, l.tmax, l.n_chunk, b.part);
            if (int rc = check_launch(ctx, "k_stoi_corr")) return rc;
        }
        hipLaunchKernelGGL(k_stoi_finish, dim3((unsigned)((n_pair + STOI_THREADS - 1) / STOI_THREADS)), dim3(STOI_THREADS), 0, st, (const double*)b.part,
                           (const int*)b.nk, l.n_chunk, (long long)len, start, (const int*)stop, p, q, (long long)n_pair, out, (int*)status);
        if (int rc = check_launch(ctx, "k_stoi_finish")) return rc;
    }
    return 0;
}

extern "C" size_t disco_estoi_workspace_bytes(const disco_ctx* ctx, int64_t n_pair, int64_t len, int p, int q, int n_taps) {
    (void)ctx;
    if (!stoi_shape_ok(n_pair, len, p, q, n_taps)) return 0;
    return stoi_layout(n_pair, len, 0, p, q, true).total;
}

extern "C" int disco_estoi(disco_ctx* ctx, const float* x, const float* y, int64_t n_pair, int64_t len, int start, const int32_t* stop, int p, int q,
                           const double* taps, int n_taps, double* out, int32_t* status, void* workspace, size_t workspace_bytes, disco_stream s) {
    DISCO_ENTER(ctx);
    StoiLayout l;
    if (int rc = stoi_check(ctx, "disco_estoi", "disco_estoi_workspace_bytes", true, x, y, n_pair, len, start, p, q, taps, n_taps, out, status, workspace,
                            workspace_bytes, &l))
        return rc;
    const StoiBuffers b(workspace, l);
    if (int rc = stoi_stages(ctx, x, y, n_pair, len, start, stop, p, q, taps, n_taps, l, b, s)) return rc;
    return estoi_last_stage(ctx, b.tob_x, b.tob_y, n_pair, l.tmax, b.nk, 1, l.n_chunk, b.part, 1, len, start, stop, p, q, out, status, s);
}

extern "C" int disco_estoi_bands(disco_ctx* ctx, const float* tob_x, const float* tob_y, int64_t n_pair, int tmax, const int32_t* frames, double* out,
                                 int32_t* status, void* workspace, size_t workspace_bytes, disco_stream s) {
    DISCO_ENTER(ctx);
    if (n_pair < 1 || tmax < 1 || !tob_x || !tob_y || !out || !status) return fail(ctx, DISCO_E_ARG, "disco_estoi_bands: bad argument");
    const int n_chunk = estoi_chunks(tmax);
    if (n_pair * std::max(n_chunk, 1) > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_estoi_bands: batch too large");
    if (n_chunk > 0 && (!workspace || workspace_bytes < (size_t)n_pair * (size_t)n_chunk * sizeof(double)))
        return fail(ctx, DISCO_E_ARG, "disco_estoi_bands: workspace smaller than 8 n_pair ceil((tmax - 29) / DISCO_ESTOI_SEGS) bytes");
    return estoi_last_stage(ctx, tob_x, tob_y, n_pair, tmax, (const int*)frames, 0, n_chunk, (double*)workspace, 0, 1, 0, nullptr, 1, 1, out, status, s);
}
