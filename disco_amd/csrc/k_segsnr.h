// Segmental SNR (disco_theque/metrics.py:131-173): the clipped level ratio of every whole window of a signal pair, weighted and summed.
//   window m covers [start + m hop, start + m hop + W);  N_w = (L - W) / hop + 1 for L = stop - start >= W, else 0
//   var = np.var of the window in float64 on the float32 samples (two passes: the mean, then the squared deviations), floored at eps
//   v_m = clip(10 log10(var_s / var_n), lo, hi);  g_m = 1, or vad[start + m hop] (the reference's own decimation of a per-sample VAD,
//   tango.py:219-220)
//   out[sig] = { sum g_m v_m, sum g_m, N_w, #windows with v_m at a clip bound }
// One workgroup per signal pair, one wave per window: a lane keeps its W / 64 samples of both signals in registers between the two
// passes (that staging is what bounds W at SEG_MAX_WIN), the wave sums are butterflies, a wave adds its windows in window order and the
// four waves are added in wave order -- a row's bits depend on nothing but the row.  Nothing at or beyond a signal's stop is read.
#pragma once
#include "k_metrics.h"

namespace disco {

constexpr int SEG_THREADS = 256;
constexpr int SEG_MAX_WIN = DISCO_SEG_SNR_MAX_WIN;      // samples of one window a wave holds in registers
constexpr int SEG_SLOTS = SEG_MAX_WIN / 64;
constexpr int SEG_STATS = 4;

static __global__ __launch_bounds__(SEG_THREADS) void k_seg_snr(const float* __restrict__ s, const float* __restrict__ n,
                                                                 const float* __restrict__ vad, long long len, int start,
                                                                 const int* __restrict__ stop_sig, int W, int hop, double lo, double hi,
                                                                 double* __restrict__ out) {
    __shared__ double red[SEG_THREADS / 64][SEG_STATS - 1];
    const long long sig = blockIdx.x;
    const int stop = span_stop(stop_sig, sig, len, start, (int)len);
    const int L = stop - start;
    const int n_win = L >= W ? (L - W) / hop + 1 : 0;
    const int lane = threadIdx.x & 63, w = wave_id();
    const double eps = 2.220446049250313e-16;             // sys.float_info.epsilon
    double sum_gv = 0.0, sum_g = 0.0, n_clip = 0.0;
    for (int m = w; m < n_win; m += SEG_THREADS / 64) {
        const long long base = sig * len + start + (long long)m * hop;
        float xs[SEG_SLOTS], xn[SEG_SLOTS];
        double s1 = 0.0, n1 = 0.0;
#pragma unroll
        for (int e = 0; e < SEG_SLOTS; ++e) {
            xs[e] = xn[e] = 0.f;
            if (64 * e < W) {                              // wave-uniform
                const int idx = lane + 64 * e;
                if (idx < W) {
                    xs[e] = s[base + idx];
                    xn[e] = n[base + idx];
                }
                s1 += (double)xs[e];
                n1 += (double)xn[e];
            }
        }
        const double mean_s = wave_sum(s1) / W, mean_n = wave_sum(n1) / W;
        double s2 = 0.0, n2 = 0.0;
#pragma unroll
        for (int e = 0; e < SEG_SLOTS; ++e) {
            if (64 * e < W) {
                const bool in = lane + 64 * e < W;
                const double ds = (double)xs[e] - mean_s, dn = (double)xn[e] - mean_n;
                s2 += in ? ds * ds : 0.0;
                n2 += in ? dn * dn : 0.0;
            }
        }
        double var_s = wave_sum(s2) / W, var_n = wave_sum(n2) / W;
        var_s = var_s < eps ? eps : var_s;                 // np.maximum(var, eps): a NaN stays
        var_n = var_n < eps ? eps : var_n;
        double v = 10.0 * log10(var_s / var_n);
        v = v < lo ? lo : (v > hi ? hi : v);               // np.clip: a NaN stays
        const double g = vad ? (double)vad[base] : 1.0;
        sum_gv += g * v;
        sum_g += g;
        n_clip += (v <= lo || v >= hi) ? 1.0 : 0.0;
    }
    if (lane == 0) {
        red[w][0] = sum_gv;
        red[w][1] = sum_g;
        red[w][2] = n_clip;
    }
    __syncthreads();
    if (threadIdx.x < SEG_STATS - 1) {
        double t = 0.0;
#pragma unroll
        for (int ww = 0; ww < SEG_THREADS / 64; ++ww) t += red[ww][threadIdx.x];
        out[sig * SEG_STATS + (threadIdx.x == 2 ? 3 : threadIdx.x)] = t;
    }
    if (threadIdx.x == SEG_STATS - 1) out[sig * SEG_STATS + 2] = (double)n_win;
}

}  // namespace disco
