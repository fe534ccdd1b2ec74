// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): direct-to-reverberant and signal-to-reverberation energies
#include "host.h"
#include "k_reverb.h"

using namespace disco;
using namespace disco_host;

static constexpr int RV_MAX_PARTS = DISCO_REVERB_MAX_RIR / CV_B;

extern "C" int disco_rir_split(disco_ctx* ctx, const float* rir, int64_t n_rir, int rir_len, int n_direct, int32_t* split, double* energy,
                               disco_stream s) {
    DISCO_ENTER(ctx);
    if (!rir || !split || !energy || n_rir < 0 || rir_len < 1 || n_direct < 0) return fail(ctx, DISCO_E_ARG, "disco_rir_split: bad argument");
    if (rir_len > DISCO_REVERB_MAX_RIR) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_rir_split: impulse responses longer than 8192 taps");
    if (n_rir > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_rir_split: batch too large");
    if (n_rir == 0) return 0;
    hipLaunchKernelGGL(k_rir_split, dim3((unsigned)n_rir), dim3(RV_THREADS), 0, (hipStream_t)s, rir, rir_len, n_direct, (int*)split, energy);
    return check_launch(ctx, "k_rir_split");
}

// the 1024-point twiddles disco_rir_convolve uses, made by whichever of the two entry points runs first
static int conv_twiddles(disco_ctx* ctx) {
    if (ctx->d_tw_conv) return 0;
    if (ctx->cfg.n_fft == CV_N) {
        ctx->d_tw_conv = ctx->d_tw;
        return 0;
    }
    std::vector<c32> tw(CV_N);
    const double two_pi = 6.283185307179586476925286766559;
    for (int i = 0; i < CV_N; ++i) {
        tw[i].x = (float)std::cos(two_pi * i / CV_N);
        tw[i].y = (float)(-std::sin(two_pi * i / CV_N));
    }
    c32* d = nullptr;
    HIPCHK(ctx, hipMalloc((void**)&d, CV_N * sizeof(c32)));
    hipError_t e = hipMemcpy(d, tw.data(), CV_N * sizeof(c32), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        HIPCHK(ctx, e);
    }
    ctx->d_tw_conv = d;
    return 0;
}

extern "C" int disco_reverb_energies(disco_ctx* ctx, const float* dry, const float* rir, const int32_t* split, int64_t n_sig, int n_ch,
                                     int dry_len, int rir_len, double* energy, disco_stream s) {
    DISCO_ENTER(ctx);
    if (!dry || !rir || !split || !energy || n_sig < 0 || n_ch < 1 || dry_len < 1 || rir_len < 1)
        return fail(ctx, DISCO_E_ARG, "disco_reverb_energies: bad argument");
    const int P = (rir_len + CV_B - 1) / CV_B;
    if (P > RV_MAX_PARTS) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_reverb_energies: impulse responses longer than 8192 taps");
    if (n_sig * n_ch > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_reverb_energies: batch too large");
    if (n_sig == 0) return 0;
    const long long Lfull = (long long)dry_len + rir_len - 1;             // the full convolution: the tail rings past the dry signal
    if (Lfull > 0x7fffffffLL - CV_N) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_reverb_energies: signals too long");
    const int nb = (int)((Lfull + CV_B - 1) / CV_B);
    hipStream_t st = (hipStream_t)s;
    const int rct = conv_twiddles(ctx);
    if (rct) return rct;
    const size_t x_bytes = (size_t)n_sig * nb * CV_F * sizeof(c32);
    const size_t h_bytes = (size_t)n_sig * n_ch * (P + 1) * CV_F * sizeof(c32);
    const int rcw = grow(ctx, ctx->conv_ws, align_up(x_bytes) + h_bytes);
    if (rcw) return rcw;
    c32* X = (c32*)ctx->conv_ws.p;
    c32* H = (c32*)((char*)ctx->conv_ws.p + align_up(x_bytes));
    const long long nx = (long long)n_sig * nb, nh = (long long)n_sig * n_ch * (P + 1);
    auto grid_of = [](long long items) { return dim3((unsigned)std::min<long long>((items + CV_WAVES - 1) / CV_WAVES, 1 << 20)); };
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_conv_spectra<true>), grid_of(nx), dim3(64 * CV_WAVES), 0, st, dry, (long long)dry_len, nb, nx, X,
                       ctx->d_tw_conv);
    hipLaunchKernelGGL(k_reverb_spectra, grid_of(nh), dim3(64 * CV_WAVES), 0, st, rir, (const int*)split, rir_len, P, nh, H, ctx->d_tw_conv);
    const dim3 grid((unsigned)(n_sig * n_ch));
    if (P <= 8)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reverb_mac_energy<8>), grid, dim3(64 * CV_WAVES), 0, st, X, H, (const int*)split, energy,
                           ctx->d_tw_conv, n_ch, nb, P, rir_len, Lfull);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reverb_mac_energy<16>), grid, dim3(64 * CV_WAVES), 0, st, X, H, (const int*)split, energy,
                           ctx->d_tw_conv, n_ch, nb, P, rir_len, Lfull);
    return check_launch(ctx, "k_reverb_mac_energy");
}
