// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): dry sources prepared on the device -- the
// speech-shaped noise of noise_from_signal (one long real transform, random phases, the inverse) and the levelling pass
#include "host.h"
#include "k_sources.h"

using namespace disco;
using namespace disco_host;

// ---- noise_from_signal (sigproc_utils.py:257-279) ---------------------------------------------------------------------------------------

namespace {
// W_N^j = exp(-2 pi i j / N) for j < N / 2, then the 1024- and the 512-point tables of the wave transform: float64 on the host, rounded once
int source_tables(disco_ctx* ctx, int p) {
    if (ctx->src_tw[p]) return 0;
    const size_t M = (size_t)1 << (p - 1), n = M + 1024 + 512;
    std::vector<c32> tw(n);
    const double two_pi = 6.283185307179586476925286766559;
    auto fill = [&](c32* t, size_t count, double N) {
        for (size_t j = 0; j < count; ++j) {
            const double a = two_pi * (double)j / N;
            t[j].x = (float)std::cos(a);
            t[j].y = (float)(-std::sin(a));
        }
    };
    fill(tw.data(), M, 2.0 * (double)M);
    fill(tw.data() + M, 1024, 1024.0);
    fill(tw.data() + M + 1024, 512, 512.0);
    c32* d = nullptr;
    HIPCHK(ctx, hipMalloc((void**)&d, n * sizeof(c32)));
    const hipError_t e = hipMemcpy(d, tw.data(), n * sizeof(c32), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        HIPCHK(ctx, e);
    }
    ctx->src_tw[p] = d;
    return 0;
}

void launch_pass(const SrcIo& io, int radix, int P, long long n_sig, hipStream_t st) {
    const int S = io.M / radix;
    if (radix >= 512) {
        const int T = S >= SRC_T ? SRC_T : 1;
        const long long items = n_sig * (S / T);
        const dim3 grid((unsigned)((items + SRC_WAVES - 1) / SRC_WAVES)), block(64 * SRC_WAVES);
        if (radix == 512 && T == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_src_wave_pass<512, 1>), grid, block, 0, st, io, P, items);
        else if (radix == 512) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_src_wave_pass<512, SRC_T>), grid, block, 0, st, io, P, items);
        else if (T == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_src_wave_pass<1024, 1>), grid, block, 0, st, io, P, items);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_src_wave_pass<1024, SRC_T>), grid, block, 0, st, io, P, items);
        return;
    }
    const int bps = (S + SRC_THREADS - 1) / SRC_THREADS;
    const dim3 grid((unsigned)(n_sig * bps)), block(SRC_THREADS);
    if (radix == 4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_src_small_pass<4>), grid, block, 0, st, io, P, bps);
    else if (radix == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_src_small_pass<8>), grid, block, 0, st, io, P, bps);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_src_small_pass<16>), grid, block, 0, st, io, P, bps);
}
}  // namespace

extern "C" int disco_noise_from_signal(disco_ctx* ctx, const float* x, int64_t n_sig, int64_t len, const int32_t* stop, int64_t n_fft,
                                       const float* phase, float* out, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!x || !phase || !out || n_sig < 0 || len < 0) return fail(ctx, DISCO_E_ARG, "disco_noise_from_signal: bad argument");
    if (n_fft < 1 || (n_fft & (n_fft - 1)) != 0) return fail(ctx, DISCO_E_ARG, "disco_noise_from_signal: n_fft must be a power of two");
    if (!stop && n_fft < len) return fail(ctx, DISCO_E_ARG, "disco_noise_from_signal: n_fft < len needs a stop per signal");
    int p = 0;
    while (((int64_t)1 << p) < n_fft) ++p;
    if (p < SRC_MIN_LOG2 || p > SRC_MAX_LOG2)
        return fail(ctx, DISCO_E_UNSUPPORTED, "disco_noise_from_signal: n_fft must be a power of two from 2^10 = 1024 to 2^22 = 4194304");
    if (len > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_noise_from_signal: signals longer than 2^31 - 1 samples");
    // one wave of the first pass per 512 (or 4 x 512) points: the largest grid of the sequence, and the workspace, bound the batch
    if (n_sig > (((int64_t)1 << 40) >> p)) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_noise_from_signal: batch too large (n_sig * n_fft > 2^40)");
    if (n_sig == 0 || len == 0) return 0;
    const int rct = source_tables(ctx, p);
    if (rct) return rct;
    const int M = (int)(n_fft / 2);
    const size_t plane = (size_t)n_sig * M * sizeof(c32);
    const int rcw = grow(ctx, ctx->src_ws, 2 * align_up(plane));
    if (rcw) return rcw;
    c32* planes[2] = {(c32*)ctx->src_ws.p, (c32*)((char*)ctx->src_ws.p + align_up(plane))};
    hipStream_t st = (hipStream_t)s;
    const SrcPlan plan = src_plan(p - 1);
    int n_pass = 0;
    while (n_pass < 3 && plan.radix[n_pass]) ++n_pass;
    SrcIo io{};
    io.x = x, io.out = out, io.stop = (const int*)stop, io.tw = ctx->src_tw[p], io.M = M, io.len = (int)len;
    int cur = 1;                                               // the plane that holds the latest result
    for (int j = 0, P = 1; j < n_pass; P *= plan.radix[j], ++j) {          // Z = FFT(x[2 n] + i x[2 n + 1])
        io.real_in = j == 0, io.real_out = 0;
        io.src = planes[cur], io.dst = planes[cur ^ 1];
        launch_pass(io, plan.radix[j], P, n_sig, st);
        cur ^= 1;
    }
    const int bps = (M / 2 + 1 + SRC_THREADS - 1) / SRC_THREADS;
    hipLaunchKernelGGL(k_src_mid, dim3((unsigned)(n_sig * bps)), dim3(SRC_THREADS), 0, st, planes[cur], phase, (const c32*)io.tw, M, bps);
    for (int j = 0, P = 1; j < n_pass; P *= plan.radix[j], ++j) {          // FFT(conj V / M), its last pass writing the samples
        io.real_in = 0, io.real_out = j == n_pass - 1;
        io.src = planes[cur], io.dst = planes[cur ^ 1];
        launch_pass(io, plan.radix[j], P, n_sig, st);
        cur ^= 1;
    }
    if (len > n_fft)
        ew_launch(k_src_zero_tail, n_sig * (len - n_fft), st, out, (long long)n_sig, (int)len, (int)n_fft);
    return check_launch(ctx, "disco_noise_from_signal");
}

// ---- subtract, scale, shift, wrap (get_target_segment, _read_random_signal: signal_setups.py:54-69, 133-136) ----------------------------

extern "C" int disco_affine_segment(disco_ctx* ctx, const float* x, int64_t n_sig, int64_t len, const int32_t* stop, const int32_t* start,
                                    const int32_t* count, const double* mean, const double* gain, int lead, float* out, int64_t out_len,
                                    disco_stream s) {
    DISCO_ENTER(ctx);
    if (!x || !out || n_sig < 0 || len < 0 || out_len < 0) return fail(ctx, DISCO_E_ARG, "disco_affine_segment: bad argument");
    if (lead < 0 || lead > out_len) return fail(ctx, DISCO_E_ARG, "disco_affine_segment: need 0 <= lead <= out_len");
    if (len > 0x7fffffffLL - AFF_CHUNK || out_len > 0x7fffffffLL - AFF_CHUNK)
        return fail(ctx, DISCO_E_UNSUPPORTED, "disco_affine_segment: signals longer than 2^31 - 1025 samples");
    if (n_sig == 0 || out_len == 0) return 0;
    const long long items = (long long)n_sig * ((out_len + AFF_CHUNK - 1) / AFF_CHUNK);
    const dim3 grid((unsigned)std::min<long long>(items, 1 << 16));
    const bool vec = len % 4 == 0 && out_len % 4 == 0 && (((uintptr_t)x | (uintptr_t)out) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_affine_segment<true>), grid, dim3(AFF_THREADS), 0, (hipStream_t)s, x, (const int*)stop, (const int*)start,
                           (const int*)count, mean, gain, lead, out, (long long)n_sig, (int)len, (int)out_len);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_affine_segment<false>), grid, dim3(AFF_THREADS), 0, (hipStream_t)s, x, (const int*)stop, (const int*)start,
                           (const int*)count, mean, gain, lead, out, (long long)n_sig, (int)len, (int)out_len);
    return check_launch(ctx, "k_affine_segment");
}
