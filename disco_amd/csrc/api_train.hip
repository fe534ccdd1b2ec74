// libdisco_hip.so -- host side of the C ABI declared in include/disco_hip.h (gfx950 only): the CRNN training path's kernels (k_train.h)
#include "host.h"
#include "k_train.h"

using namespace disco;
using namespace disco_host;

static_assert(TRAIN_LOSS_THREADS == 256 && DISCO_RECON_LOSS_MAX_BLOCKS * 16 == DISCO_RECON_LOSS_WS_BYTES, "header and kernel disagree");

// ctx may be NULL in every entry point of this unit (the DNN owns no context): current_device / launched of host.h
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline unsigned gate_grid(long long items) { return (unsigned)std::min<long long>((items + 255) / 256, 65536); }

extern "C" int disco_gru_gates_train(disco_ctx* ctx, const float* gi, int64_t gi_stride, const float* gh, const float* gh_bias, const float* h_prev,
                                     float* h_out, float* saved, int64_t n, int H, disco_stream s) {
    if (!gi || !h_out || !saved || (!gh && !gh_bias) || n < 1 || H < 1 || gi_stride < 3 * (int64_t)H)
        return fail(ctx, DISCO_E_ARG, "disco_gru_gates_train: bad argument");
    DevGuard dev_guard_(current_device(ctx));
    const bool wide = H % 4 == 0 && gi_stride % 4 == 0 && al16(gi) && al16(gh ? gh : gh_bias) && al16(h_prev) && al16(h_out) && al16(saved);
    if (wide)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gru_gates_train<4>), dim3(gate_grid((long long)n * (H / 4))), dim3(256), 0, (hipStream_t)s, gi,
                           (long long)gi_stride, gh, gh_bias, h_prev, h_out, saved, (long long)n, H);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gru_gates_train<1>), dim3(gate_grid((long long)n * H)), dim3(256), 0, (hipStream_t)s, gi,
                           (long long)gi_stride, gh, gh_bias, h_prev, h_out, saved, (long long)n, H);
    return launched();
}

extern "C" int disco_gru_gates_backward(disco_ctx* ctx, const float* d_out, int64_t d_out_stride, const float* d_carry, const float* saved,
                                        const float* h_prev, float* d_gi, int64_t d_gi_stride, float* d_gh, float* d_h_direct, int64_t n, int H,
                                        disco_stream s) {
    if ((!d_out && !d_carry) || !saved || !d_gi || !d_gh || !d_h_direct || n < 1 || H < 1 || (d_out && d_out_stride < H) || d_gi_stride < 3 * (int64_t)H)
        return fail(ctx, DISCO_E_ARG, "disco_gru_gates_backward: bad argument");
    DevGuard dev_guard_(current_device(ctx));
    const bool wide = H % 4 == 0 && d_gi_stride % 4 == 0 && (!d_out || d_out_stride % 4 == 0) && al16(d_out) && al16(d_carry) && al16(saved) &&
                      al16(h_prev) && al16(d_gi) && al16(d_gh) && al16(d_h_direct);
    if (wide)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gru_gates_backward<4>), dim3(gate_grid((long long)n * (H / 4))), dim3(256), 0, (hipStream_t)s, d_out,
                           (long long)d_out_stride, d_carry, saved, h_prev, d_gi, (long long)d_gi_stride, d_gh, d_h_direct, (long long)n, H);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gru_gates_backward<1>), dim3(gate_grid((long long)n * H)), dim3(256), 0, (hipStream_t)s, d_out,
                           (long long)d_out_stride, d_carry, saved, h_prev, d_gi, (long long)d_gi_stride, d_gh, d_h_direct, (long long)n, H);
    return launched();
}

// workgroups of the loss's first pass: a function of the number of terms alone, so that the order of summation is too
static inline int loss_blocks(long long total) {
    return (int)std::min<long long>((total + TRAIN_LOSS_THREADS - 1) / TRAIN_LOSS_THREADS, DISCO_RECON_LOSS_MAX_BLOCKS);
}
static inline bool loss_shape_ok(int64_t B, int C, int W, int F, int ff_in, int n_out) {
    return B >= 1 && C >= 1 && W >= 1 && F >= 1 && n_out >= 1 && ff_in >= 0 && (long long)ff_in + n_out <= W;
}

extern "C" int disco_recon_loss(disco_ctx* ctx, const float* est, const float* y, const float* x, int64_t B, int C, int W, int F, int ff_in, int n_out,
                                double* sums, void* workspace, size_t workspace_bytes, disco_stream s) {
    if (!est || !y || !x || !sums || !workspace || !loss_shape_ok(B, C, W, F, ff_in, n_out) || ((uintptr_t)workspace & 7))
        return fail(ctx, DISCO_E_ARG, "disco_recon_loss: bad argument");
    const long long total = (long long)B * n_out * F;
    const int blocks = loss_blocks(total);
    if (workspace_bytes < (size_t)blocks * 2 * sizeof(double)) return fail(ctx, DISCO_E_ARG, "disco_recon_loss: workspace too small");
    DevGuard dev_guard_(current_device(ctx));
    hipLaunchKernelGGL(k_recon_loss_partial, dim3((unsigned)blocks), dim3(TRAIN_LOSS_THREADS), 0, (hipStream_t)s, est, y, x, total, C, W, F, ff_in,
                       n_out, (double*)workspace);
    hipLaunchKernelGGL(k_recon_loss_fold, dim3(1), dim3(TRAIN_LOSS_THREADS), 0, (hipStream_t)s, (const double*)workspace, blocks, sums);
    return launched();
}

extern "C" int disco_recon_loss_grad(disco_ctx* ctx, const float* est, const float* y, const float* x, int64_t B, int C, int W, int F, int ff_in,
                                     int n_out, const double* sums, const float* g, float* d_est, disco_stream s) {
    if (!est || !y || !x || !sums || !g || !d_est || !loss_shape_ok(B, C, W, F, ff_in, n_out))
        return fail(ctx, DISCO_E_ARG, "disco_recon_loss_grad: bad argument");
    DevGuard dev_guard_(current_device(ctx));
    const long long total = (long long)B * n_out * F;
    hipLaunchKernelGGL(k_recon_loss_grad, dim3(gate_grid(total)), dim3(256), 0, (hipStream_t)s, est, y, x, total, C, W, F, ff_in, n_out, sums, g, d_est);
    return launched();
}

extern "C" int disco_train_batch(disco_ctx* ctx, const float* bank, int S, int64_t N, int T, int F, const int32_t* tab, const int32_t* tab_host,
                                 int64_t B, int C, int W, float* x, float* y, disco_stream s) {
    if (!bank || !tab || !x || !y || S < 1 || N < 1 || T < 1 || F < 1 || B < 1 || C < 1 || W < 1 || W > T)
        return fail(ctx, DISCO_E_ARG, "disco_train_batch: bad argument");
    if ((long long)W * F > 0x7fffffffLL) return fail(ctx, DISCO_E_UNSUPPORTED, "disco_train_batch: window too large");
    if (tab_host)                       // the caller's host copy of the tables: refused here, before anything is launched
        for (int64_t b = 0; b < B; ++b) {
            const int32_t* t = tab_host + b * (C + 3);
            bool ok = t[0] >= 0 && t[0] < N && t[1] >= 0 && t[1] <= T - W;
            for (int j = 0; j <= C; ++j) ok = ok && t[2 + j] >= 0 && t[2 + j] < S;
            if (!ok) return fail(ctx, DISCO_E_ARG, "disco_train_batch: table entry out of range (segment, m + W > T, or signal row)");
        }
    DevGuard dev_guard_(current_device(ctx));
    const long long runs = (long long)B * (C + 1);
    hipLaunchKernelGGL(k_train_batch, dim3((unsigned)std::min<long long>(runs, 16384)), dim3(256), 0, (hipStream_t)s, bank, S, (long long)N, T, F,
                       (const int*)tab, (long long)B, C, W, x, y);
    return launched();
}
