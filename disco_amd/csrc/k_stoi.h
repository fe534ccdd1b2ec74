// STOI, the short-time objective intelligibility measure (Taal, Hendriks, Heusdens, Jensen 2011; what the reference calls as pystoi.stoi,
// tango.py:569-578), batched over (clean, processed) pairs.  Restated from the definition with the constants and conventions of pystoi;
// the package is third-party and absent, so this is pinned by the float64 yardstick of tests/stoi_checks.py, not against the package.
//   1. k_stoi_resample   both signals to 10 kHz: polyphase FIR with the caller's float64 taps (not launched at 10 kHz)
//   2. k_stoi_frames     energies of the Hann-windowed 256-sample frames of x (hop 128), the frames within 40 dB of the loudest, in order
//   3. k_stoi_tob        per kept frame pair: the overlap-added, windowed 256 samples of x and y as ONE 512-point wave FFT (x real part, y
//                        imaginary part), untangled, |.|^2 summed over the 15 third-octave bin ranges, sqrt -> tob_x, tob_y [pair][15][T]
//   4. k_stoi_corr       per (segment of 30 frames, band): normalise, clip, centre, correlate (float64) -> per-block partial sums;
//      k_stoi_finish     the partial sums in block order, / (J 15), the status and the count of kept frames
// The overlap-added signals are never written: frame j of the overlap-added signal is formed from the kept source frames j - 1, j, j + 1.
// Every sum runs in a fixed order and the launch geometry of a pair depends on that pair's span alone: a pair gives the same bits
// alone, in any batch and from run to run.  No atomics.
#pragma once
#include "fft.h"

namespace disco {

constexpr int STOI_FRAME = 256, STOI_HOP = 128, STOI_NFFT = 512, STOI_BANDS = 15, STOI_SEG = 30;
constexpr double STOI_EPS = 2.220446049250313e-16;
constexpr double STOI_DYN_RANGE = 40.0;
constexpr double STOI_CLIP = 6.623413251903491;          // 1 + 10^(15 / 20)
constexpr int STOI_THREADS = 256;
constexpr int STOI_FR_THREADS = 1024;
constexpr int STOI_MAX_TAPS = 1 << 16;                   // 48 kHz needs 1741, 44.1 kHz 31947
constexpr int STOI_TW_BYTES = STOI_NFFT * 8, STOI_WF_BYTES = STOI_FRAME * 4, STOI_WD_BYTES = STOI_FRAME * 8;

// first bin of band i on the grid k 10000 / 512 (band i = bins [lo(i), lo(i + 1)): the upper edge of a band rounds to the lower edge of the next)
__host__ __device__ __forceinline__ int stoi_band_lo(int i) {
    constexpr int lo[STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
    return lo[i];
}

// samples of pair `pair` at the input rate (stop clamped into [start, len]), at 10 kHz, and its frames range(0, n10 - 256, 128)
__host__ __device__ __forceinline__ int stoi_span(long long len, int start, const int* __restrict__ stop, long long pair) {
    long long e = stop ? (long long)stop[pair] : len;
    e = e > len ? len : e;
    return e > start ? (int)(e - start) : 0;
}
__host__ __device__ __forceinline__ int stoi_len10(int n, int p, int q) { return p == q ? n : (int)(((long long)n * p + q - 1) / q); }
__host__ __device__ __forceinline__ int stoi_frames(int n10) { return n10 > STOI_FRAME ? (n10 - STOI_FRAME + STOI_HOP - 1) / STOI_HOP : 0; }

__device__ __forceinline__ double stoi_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// twiddles exp(-2 pi i k / 512), the window hanning(258)[1:-1] in float32 (transform) and float64 (energies); one block of 256 threads
static __global__ __launch_bounds__(STOI_THREADS) void k_stoi_tables(c32* __restrict__ tw, float* __restrict__ wf, double* __restrict__ wd) {
    const int t = threadIdx.x;
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = t; k < STOI_NFFT; k += STOI_THREADS) tw[k] = make_float2((float)cos(two_pi * k / STOI_NFFT), (float)(-sin(two_pi * k / STOI_NFFT)));
    const double w = 0.5 - 0.5 * cos(two_pi * (t + 1) / (STOI_FRAME + 1));
    wf[t] = (float)w;
    wd[t] = w;
}

// out[m] = p sum_i h[m q + half - p i] x[start + i] over the i in [0, n) whose tap index lies in [0, n_taps): scipy.signal.resample_poly(x, p, q,
// window = h).  One output sample per lane; float32 sample x float64 tap accumulated in float64 in tap order (i descending).
// grid = n_pair * 2 * nblk: block = ((pair, x or y), 256 outputs)
static __global__ __launch_bounds__(STOI_THREADS) void k_stoi_resample(const float* __restrict__ x, const float* __restrict__ y, long long len,
                                                                        int start, const int* __restrict__ stop, int p, int q,
                                                                        const double* __restrict__ taps, int n_taps, int n10max, int nblk,
                                                                        float* __restrict__ xr, float* __restrict__ yr) {
    const long long row = blockIdx.x / nblk;
    const int b = (int)(blockIdx.x - row * nblk);
    const long long pair = row >> 1;
    const int n = stoi_span(len, start, stop, pair);
    const int n10 = stoi_len10(n, p, q);
    const int m = b * STOI_THREADS + (int)threadIdx.x;
    if (m >= n10) return;
    const float* src = ((row & 1) ? y : x) + pair * len + start;
    const long long c = (long long)m * q + (n_taps - 1) / 2;       // tap index against sample 0
    const long long t = c - (n_taps - 1);
    long long i_hi = c / p, i_lo = t <= 0 ? 0 : (t + p - 1) / p;
    if (i_hi > n - 1) i_hi = n - 1;
    double acc = 0.0;
    for (long long i = i_hi; i >= i_lo; --i) acc += taps[c - (long long)p * i] * (double)src[i];
    ((row & 1) ? yr : xr)[pair * n10max + m] = (float)((double)p * acc);
}

// One workgroup per pair.  E[f] = 20 log10(|w x[128 f : 128 f + 256]| + EPS) in float64 (a wave per frame), their maximum, then the frames
// with E[f] > max - 40 in ascending order -> idx[pair][0 .. n_kept), nk[pair] = n_kept.  sx: the 10-kHz signals, rows of `stride`
// samples starting at `off` (the resampled rows, or the caller's at `start`).
static __global__ __launch_bounds__(STOI_FR_THREADS) void k_stoi_frames(const float* __restrict__ sx, long long stride, int off, long long len,
                                                                         int start, const int* __restrict__ stop, int p, int q,
                                                                         const double* __restrict__ wd, int nfmax, double* __restrict__ E,
                                                                         int* __restrict__ idx, int* __restrict__ nk) {
    constexpr int NW = STOI_FR_THREADS / 64;
    __shared__ double wmax[NW];
    __shared__ int wcnt[NW];
    const long long pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = wave_id();
    const int NF = stoi_frames(stoi_len10(stoi_span(len, start, stop, pair), p, q));
    const float* src = sx + pair * stride + off;
    double* Ep = E + pair * nfmax;
    int* ip = idx + pair * nfmax;
    double wv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) wv[e] = wd[lane + 64 * e];
    for (int f = w; f < NF; f += NW) {
        double s = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double v = (double)src[(long long)f * STOI_HOP + lane + 64 * e] * wv[e];
            s += v * v;
        }
        s = stoi_wave_sum(s);
        if (lane == 0) Ep[f] = 20.0 * log10(sqrt(s) + STOI_EPS);
    }
    __syncthreads();
    double mx = -1.0e300;
    for (int f = tid; f < NF; f += STOI_FR_THREADS) mx = fmax(mx, Ep[f]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) wmax[w] = mx;
    __syncthreads();
    mx = wmax[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) mx = fmax(mx, wmax[i]);
    const double thr = mx - STOI_DYN_RANGE;
    int base = 0;
    for (int f0 = 0; f0 < NF; f0 += STOI_FR_THREADS) {
        const int f = f0 + tid;
        const bool keep = f < NF && Ep[f] > thr;
        const unsigned long long bal = __ballot(keep ? 1 : 0);
        const int before = __builtin_popcountll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[w] = __builtin_popcountll(bal);
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            woff += i < w ? wcnt[i] : 0;
            total += wcnt[i];
        }
        if (keep) ip[base + woff + before] = f;
        base += total;
        __syncthreads();
    }
    if (tid == 0) nk[pair] = base;
}

// One wave per (pair, frame j of the overlap-added signals), j < T = n_kept - 1.  Sample n of that frame is
//   n < 128:  w[n] x[128 idx[j] + n] + w[n + 128] x[128 idx[j - 1] + n + 128]      (no second term for j = 0)
//   n >= 128: w[n] x[128 idx[j] + n] + w[n - 128] x[128 idx[j + 1] + n - 128]
// windowed again by w, zero-padded to 512; x and y ride one transform as its real and imaginary part (halved, which the untangle undoes).
static __global__ __launch_bounds__(STOI_THREADS) void k_stoi_tob(const float* __restrict__ sx, const float* __restrict__ sy, long long stride, int off,
                                                                   const c32* __restrict__ tw, const float* __restrict__ wf,
                                                                   const int* __restrict__ idx, const int* __restrict__ nk, int nfmax, int tmax,
                                                                   long long n_items, float* __restrict__ tob_x, float* __restrict__ tob_y) {
    constexpr int E = FftPlan<STOI_NFFT>::E;
    __shared__ c32 bufs[STOI_THREADS / 64][fft_buf_len<STOI_NFFT>()];
    const int lane = threadIdx.x & 63, w = wave_id();
    const long long item = (long long)blockIdx.x * (STOI_THREADS / 64) + w;
    if (item >= n_items) return;
    const long long pair = item / tmax;
    const int j = (int)(item - pair * tmax);
    if (j >= nk[pair] - 1) return;                               // wave-uniform; no workgroup barrier below
    c32* buf = bufs[w];
    WaveTw<STOI_NFFT> wtw;
    wtw.init(tw, lane);
    const int* ip = idx + pair * nfmax;
    const int i1 = ip[j], i0 = j > 0 ? ip[j - 1] : i1, i2 = ip[j + 1];
    const float* px = sx + pair * stride + off;
    const float* py = sy + pair * stride + off;
    c32 v[E];
    bool nzx = false, nzy = false;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int n = lane + 64 * e;
        const int n2 = e < 2 ? n + STOI_HOP : n - STOI_HOP;
        const long long a = (long long)i1 * STOI_HOP + n, b = (long long)(e < 2 ? i0 : i2) * STOI_HOP + n2;
        const float w1 = wf[n], w2 = wf[n2];
        const bool two = e >= 2 || j > 0;
        const float ox = w1 * px[a] + (two ? w2 * px[b] : 0.f);
        const float oy = w1 * py[a] + (two ? w2 * py[b] : 0.f);
        const float wh = 0.5f * w1;
        v[e] = make_float2(wh * ox, wh * oy);
        nzx = nzx || ox != 0.f;
        nzy = nzy || oy != 0.f;
    }
    // The two spectra share one transform, whose rounding leaves some 1e-7 of each in the other.  Next to a signal that is nothing: a frame
    // of exact zeros has the spectrum zero (an all-zero x must come out as d = 0 through the EPS terms).
    const bool some_x = __any(nzx ? 1 : 0), some_y = __any(nzy ? 1 : 0);
#pragma unroll
    for (int e = 4; e < E; ++e) v[e] = make_float2(0.f, 0.f);
    fft_wave<STOI_NFFT>(v, wtw, buf, lane);
    DISCO_LDS_WAR();                                             // the last pass' reads of buf are done in every lane
    rfft_pair_untangle<STOI_NFFT>(v, buf, lane, [&](int jj, int f, c32 A, c32 B) {
        if (jj < E / 2) buf[f] = make_float2(A.x * A.x + A.y * A.y, B.x * B.x + B.y * B.y);      // bins 0 .. 255; the bands end at 218
    });
    DISCO_LDS_RAW();
    if (lane < 2 * STOI_BANDS) {
        const int which = lane >= STOI_BANDS ? 1 : 0, band = lane - which * STOI_BANDS;
        float s = 0.f;
        for (int f = stoi_band_lo(band); f < stoi_band_lo(band + 1); ++f) s += which ? buf[f].y : buf[f].x;
        (which ? tob_y : tob_x)[(pair * STOI_BANDS + band) * tmax + j] = (which ? some_y : some_x) ? sqrtf(s) : 0.f;
    }
}

// Thread = (band, segment) of a pair, item = band J + s with J = T - 29 segments; a workgroup owns 256 consecutive items of one pair and
// leaves their sum, added in a fixed tree, in part[pair][chunk].  Float64 throughout:
//   c = |x| / (|y| + EPS);  y' = min(c y, x (1 + 10^(15/20)));  both centred, both divided by (norm + EPS);  d = sum y' x
static __global__ __launch_bounds__(STOI_THREADS) void k_stoi_corr(const float* __restrict__ tob_x, const float* __restrict__ tob_y,
                                                                    const int* __restrict__ nk, int tmax, int n_chunk, double* __restrict__ part) {
    __shared__ double red[STOI_THREADS];
    const long long pair = blockIdx.x / n_chunk;
    const int chunk = (int)(blockIdx.x - pair * n_chunk);
    const int tid = threadIdx.x;
    const int J = nk[pair] - 1 - (STOI_SEG - 1);
    if (J <= 0 || (long long)chunk * STOI_THREADS >= (long long)J * STOI_BANDS) return;          // uniform over the workgroup
    const int it = chunk * STOI_THREADS + tid;
    double d = 0.0;
    if (it < J * STOI_BANDS) {
        const int band = it / J, s = it - band * J;
        const float* fx = tob_x + (pair * STOI_BANDS + band) * tmax + s;
        const float* fy = tob_y + (pair * STOI_BANDS + band) * tmax + s;
        double xs[STOI_SEG], ys[STOI_SEG];
        double sxx = 0.0, syy = 0.0;
#pragma unroll
        for (int n = 0; n < STOI_SEG; ++n) {
            xs[n] = (double)fx[n];
            ys[n] = (double)fy[n];
            sxx += xs[n] * xs[n];
            syy += ys[n] * ys[n];
        }
        const double c = sqrt(sxx) / (sqrt(syy) + STOI_EPS);
        double mx = 0.0, my = 0.0;
#pragma unroll
        for (int n = 0; n < STOI_SEG; ++n) {
            ys[n] = fmin(c * ys[n], xs[n] * STOI_CLIP);
            mx += xs[n];
            my += ys[n];
        }
        mx /= STOI_SEG;
        my /= STOI_SEG;
        sxx = syy = 0.0;
#pragma unroll
        for (int n = 0; n < STOI_SEG; ++n) {
            xs[n] -= mx;
            ys[n] -= my;
            sxx += xs[n] * xs[n];
            syy += ys[n] * ys[n];
        }
        const double ix = sqrt(sxx) + STOI_EPS, iy = sqrt(syy) + STOI_EPS;
#pragma unroll
        for (int n = 0; n < STOI_SEG; ++n) d += (ys[n] / iy) * (xs[n] / ix);
    }
    red[tid] = d;
    __syncthreads();
    for (int o = STOI_THREADS / 2; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) part[pair * n_chunk + chunk] = red[0];
}

// out[pair] = {d, n_kept}, status[pair]: 0 scored; 1 fewer than 30 frames, d = 1e-5; 2 the span gives no frame at all, d = NaN
static __global__ __launch_bounds__(STOI_THREADS) void k_stoi_finish(const double* __restrict__ part, const int* __restrict__ nk, int n_chunk,
                                                                      long long len, int start, const int* __restrict__ stop, int p, int q,
                                                                      long long n_pair, double* __restrict__ out, int* __restrict__ status) {
    const long long pair = (long long)blockIdx.x * STOI_THREADS + threadIdx.x;
    if (pair >= n_pair) return;
    const int NF = stoi_frames(stoi_len10(stoi_span(len, start, stop, pair), p, q));
    const int kept = NF > 0 ? nk[pair] : 0, T = kept - 1;
    double d;
    int st;
    if (NF == 0) {
        d = __builtin_nan("");
        st = 2;
    } else if (T < STOI_SEG) {
        d = 1e-5;
        st = 1;
    } else {
        const long long items = (long long)(T - (STOI_SEG - 1)) * STOI_BANDS;
        const int nch = (int)((items + STOI_THREADS - 1) / STOI_THREADS);
        double s = 0.0;
        for (int c = 0; c < nch; ++c) s += part[pair * n_chunk + c];
        d = s / (double)items;
        st = 0;
    }
    out[2 * pair] = d;
    out[2 * pair + 1] = (double)kept;
    status[pair] = st;
}

}  // namespace disco
