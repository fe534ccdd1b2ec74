// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): segmental SNR
#include "host.h"
#include "k_segsnr.h"

using namespace disco;
using namespace disco_host;

extern "C" int disco_seg_snr(disco_ctx* ctx, const float* s, const float* n, const float* vad, int64_t n_sig, int64_t len, int start,
                             const int32_t* stop, int win_len, int win_hop, float lo_db, float hi_db, double* out, disco_stream st) {
    static_assert(SEG_MAX_WIN % 64 == 0 && SEG_MAX_WIN == 2048, "a lane holds SEG_MAX_WIN / 64 samples of a window; the message below");
    DISCO_ENTER(ctx);
    if (!s || !n || !out || n_sig < 0 || len < 0 || win_len < 1 || win_hop < 1 || win_hop > win_len || !(lo_db < hi_db))
        return fail(ctx, DISCO_E_ARG, "disco_seg_snr: bad argument");
    if (start < 0 || start > len) return fail(ctx, DISCO_E_ARG, "disco_seg_snr: need 0 <= start <= len");
    if (win_len > SEG_MAX_WIN) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_seg_snr: windows longer than 2048 samples");
    if (len > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_seg_snr: signals longer than 2^31 - 1 samples");
    if (n_sig > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_seg_snr: batch too large");
    if (n_sig == 0) return 0;
    hipLaunchKernelGGL(k_seg_snr, dim3((unsigned)n_sig), dim3(SEG_THREADS), 0, (hipStream_t)st, s, n, vad, (long long)len, start,
                       (const int*)stop, win_len, win_hop, (double)lo_db, (double)hi_db, out);
    return check_launch(ctx, "k_seg_snr");
}
