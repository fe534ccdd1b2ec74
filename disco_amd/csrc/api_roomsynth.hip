// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): from reverberated sources to rooms -- the
// per-sample VAD of the images and the scaled mix
#include "host.h"
#include "k_roomsynth.h"

using namespace disco;
using namespace disco_host;

// ---- vad_oracle_batch per sample (sigproc_utils.py:12-55; get_convolved_vads, convolve_signals.py:102-115) -------------------------------

extern "C" int disco_vad_samples(disco_ctx* ctx, const float* x, int64_t n_sig, int64_t len, const int32_t* stop, int win_len, int win_hop,
                                 float thr, int rat, float* vad, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!x || !vad || n_sig < 0 || len < 0) return fail(ctx, DISCO_E_ARG, "disco_vad_samples: bad argument");
    if (win_len < 1 || win_hop < 1 || win_len % win_hop != 0)
        return fail(ctx, DISCO_E_ARG, "disco_vad_samples: need 1 <= win_hop <= win_len, win_len a multiple of win_hop");
    if (rat < 1) return fail(ctx, DISCO_E_ARG, "disco_vad_samples: need rat >= 1");
    if (!(thr >= 0.f) || !std::isfinite(thr)) return fail(ctx, DISCO_E_ARG, "disco_vad_samples: thr must be finite and not negative");
    if (len > (int64_t)VAD_MAX_SEG * win_hop) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_vad_samples: signal longer than 4096 hops (len <= 4096 * win_hop)");
    if (len > (1LL << 30)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_vad_samples: signals longer than 2^30 samples");
    if (n_sig > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_vad_samples: batch too large");
    if (n_sig == 0 || len == 0) return 0;
    hipLaunchKernelGGL(k_vad_samples, dim3((unsigned)n_sig), dim3(VAD_THREADS), 0, (hipStream_t)s, x, (const int*)stop, vad, (int)len, win_len,
                       win_hop, thr, 0.99f, rat);
    return check_launch(ctx, "k_vad_samples");
}

// ---- noise scaled to a gain and mixed in (increase_to_snr's last line, sigproc_utils.py:212, 223; mix_sigs, post_generator.py:103-113) ---

extern "C" int disco_mix_scaled(disco_ctx* ctx, const float* s, const float* n, int64_t n_sig, int64_t len, int64_t n_len, const float* gain,
                                int group, const int32_t* stop, float* n_out, float* y_out, disco_stream st) {
    DISCO_ENTER(ctx);
    if (!n || !gain || (!n_out && !y_out) || n_sig < 0 || len < 0) return fail(ctx, DISCO_E_ARG, "disco_mix_scaled: bad argument");
    if ((s == nullptr) != (y_out == nullptr)) return fail(ctx, DISCO_E_ARG, "disco_mix_scaled: s and y_out must both be given or both be NULL");
    if (n_len < 0 || n_len > len) return fail(ctx, DISCO_E_ARG, "disco_mix_scaled: need 0 <= n_len <= len");
    if (group < 1 || n_sig % group != 0) return fail(ctx, DISCO_E_ARG, "disco_mix_scaled: n_sig must be a multiple of group >= 1");
    if (n_out == n && n_len != len) return fail(ctx, DISCO_E_ARG, "disco_mix_scaled: n_out == n (in place) needs n_len == len");
    if (len > 0x7fffffffLL - MIX_CHUNK) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_mix_scaled: signals longer than 2^31 - 1025 samples");
    if (n_sig == 0 || len == 0) return 0;
    const long long items = (long long)n_sig * ((len + MIX_CHUNK - 1) / MIX_CHUNK);
    const dim3 grid((unsigned)std::min<long long>(items, 1 << 16));
    const uintptr_t bits = (uintptr_t)s | (uintptr_t)n | (uintptr_t)n_out | (uintptr_t)y_out;      // NULL adds nothing
    if (len % 4 == 0 && n_len % 4 == 0 && (bits & 15) == 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mix_scaled<true>), grid, dim3(MIX_THREADS), 0, (hipStream_t)st, s, n, gain, group, (const int*)stop, n_out,
                           y_out, (long long)n_sig, (int)len, (int)n_len);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mix_scaled<false>), grid, dim3(MIX_THREADS), 0, (hipStream_t)st, s, n, gain, group, (const int*)stop, n_out,
                           y_out, (long long)n_sig, (int)len, (int)n_len);
    return check_launch(ctx, "k_mix_scaled");
}

// ---- a meeting room of S talkers: mix, own talker and the sum of the others per channel (simulate_room, gen_meetit/convolve_signals.py:140-148)

extern "C" int disco_source_mix(disco_ctx* ctx, const float* images, int n_src, int64_t n_row, int64_t len, const int32_t* target, int n_mic,
                                const int32_t* stop, float* y_out, float* s_out, float* n_out, disco_stream st) {
    DISCO_ENTER(ctx);
    if (!images || !target || (!y_out && !s_out && !n_out) || n_row < 0 || len < 0) return fail(ctx, DISCO_E_ARG, "disco_source_mix: bad argument");
    if (n_src < 2 || n_src > MIX_MAX_SOURCES) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_source_mix: the number of sources must be 2 <= n_src <= 8");
    if (n_mic < 1 || n_row % n_mic != 0) return fail(ctx, DISCO_E_ARG, "disco_source_mix: n_row must be a multiple of n_mic >= 1");
    if (n_mic > MIX_MAX_CHANNELS) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_source_mix: more than 64 channels per room");
    MixTargets tg = {};
    for (int c = 0; c < n_mic; ++c) {
        if (target[c] < 0 || target[c] >= n_src) return fail(ctx, DISCO_E_ARG, "disco_source_mix: target must name a source, 0 <= target[c] < n_src");
        tg.t[c] = (unsigned char)target[c];
    }
    if (len > 0x7fffffffLL - MIX_CHUNK) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_source_mix: signals longer than 2^31 - 1025 samples");
    if (n_row == 0 || len == 0) return 0;
    const long long items = (long long)n_row * ((len + MIX_CHUNK - 1) / MIX_CHUNK);
    const dim3 grid((unsigned)std::min<long long>(items, 1 << 16));
    const uintptr_t bits = (uintptr_t)images | (uintptr_t)y_out | (uintptr_t)s_out | (uintptr_t)n_out;      // NULL adds nothing
    with_bool(len % 4 == 0 && (bits & 15) == 0, [&](auto vec) {
        constexpr bool VEC = decltype(vec)::value;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_source_mix<VEC>), grid, dim3(MIX_THREADS), 0, (hipStream_t)st, images, n_src, tg, n_mic, (const int*)stop,
                           y_out, s_out, n_out, (long long)n_row, (int)len);
    });
    return check_launch(ctx, "k_source_mix");
}
