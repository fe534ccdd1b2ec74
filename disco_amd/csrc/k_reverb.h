// How reverberant a simulated room came out (disco_theque/metrics.py:176-208): the direct-to-reverberant ratio of every impulse
// response and the signal-to-reverberation ratio of a dry signal through it.
//   split = min(argmax(rir) + n_direct, rir_len);  h_d = rir[:split], h_r = rir[split:]
//   DRR = 10 log10(sum h_d^2 / sum h_r^2)                       k_rir_split: the split and the two tap energies
//   SRR = 10 log10(sum (x * h_d)^2 / sum (x * h_r)^2)           k_reverb_spectra + k_reverb_mac_energy: the two signal energies
// The signal energies come from the partitioned overlap-save of k_conv.h (1024-point wave FFT, 512 new samples per block; the input
// spectra are k_conv_spectra<true>'s) WITHOUT an output store: neither convolution is ever written.  h, h_d and h_r differ in the one
// partition that contains the split, so a (signal, channel) has P + 1 spectra: slot p < P is partition p -- cut to its direct taps where
// the split falls inside it -- and slot P is the tail taps of that partition.  Both halves are transformed from their own taps; neither
// is a difference of spectra or of time signals, so a tail 40 dB below the direct path keeps its digits.  A workgroup owns one (signal,
// channel), holds its P + 1 spectra in LDS, and every output block has two accumulator sets: the direct one takes the partitions up to
// the split's, the tail one those from it.  Each set that received a product is inverse-transformed on its own, the 512 valid samples
// are squared and summed in float64 per lane; a wave adds its blocks in block order, the wave sums are butterflies and the four waves
// are added in wave order: the bits of a row depend on nothing but the row.  Products: the convolution's plus one partition per block.
#pragma once
#include "k_conv.h"
#include "k_metrics.h"

namespace disco {

constexpr int RV_THREADS = 256;

// one workgroup per impulse response: np.argmax (first maximum; a NaN wins, at its first index), the split, the energies on both sides
static __global__ __launch_bounds__(RV_THREADS) void k_rir_split(const float* __restrict__ rir, int rir_len, int n_direct,
                                                                  int* __restrict__ split, double* __restrict__ energy) {
    __shared__ float best_v[RV_THREADS];
    __shared__ int best_i[RV_THREADS];
    __shared__ double red[RV_THREADS / 64][2];
    __shared__ int s_split;
    const long long row = blockIdx.x;
    const float* h = rir + row * rir_len;
    // a beats b: a is NaN and b is not, or a > b; equal values and two NaNs go to the lower index
    float bv = 0.f;
    int bi = -1;
    for (int i = threadIdx.x; i < rir_len; i += RV_THREADS) {
        const float v = h[i];
        if (bi < 0 || (!(bv != bv) && (v != v || v > bv))) {
            bv = v;
            bi = i;
        }
    }
    best_v[threadIdx.x] = bv;
    best_i[threadIdx.x] = bi;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < RV_THREADS; ++t) {
            const float v = best_v[t];
            const int i = best_i[t];
            if (i < 0) continue;
            const bool nan_b = bv != bv, nan_v = v != v;
            const bool better = nan_b ? (nan_v && i < bi) : (nan_v || v > bv || (v == bv && i < bi));
            if (better) {
                bv = v;
                bi = i;
            }
        }
        const long long sp = (long long)bi + n_direct;
        s_split = (int)(sp > rir_len ? rir_len : sp);
        if (split) split[row] = s_split;
    }
    __syncthreads();
    const int sp = s_split;
    double e_d = 0.0, e_r = 0.0;
    for (int i = threadIdx.x; i < rir_len; i += RV_THREADS) {
        const double v = (double)h[i];
        if (i < sp) e_d += v * v;
        else e_r += v * v;
    }
    e_d = wave_sum(e_d);
    e_r = wave_sum(e_r);
    const int w = wave_id();
    if ((threadIdx.x & 63) == 0) {
        red[w][0] = e_d;
        red[w][1] = e_r;
    }
    __syncthreads();
    if (energy && threadIdx.x < 2) {
        double t = 0.0;
#pragma unroll
        for (int ww = 0; ww < RV_THREADS / 64; ++ww) t += red[ww][threadIdx.x];
        energy[row * 2 + threadIdx.x] = t;
    }
}

// the split of one response as read from device memory, clamped into [0, rir_len], and what follows from it
struct RvSplit {
    int s;          // taps [0, s) are direct, [s, rir_len) the tail
    int p_mix;      // the partition with taps of both kinds, or -1: its direct taps are slot p_mix, its tail taps slot P
    int p_dir_hi;   // last partition with direct taps (-1: none)
    int p_tail_lo;  // first partition with tail taps (P: none)
};
__device__ __forceinline__ RvSplit rv_split(const int* __restrict__ split, long long ic, int rir_len, int P) {
    int s = __builtin_amdgcn_readfirstlane(split[ic]);
    s = s < 0 ? 0 : (s > rir_len ? rir_len : s);
    RvSplit r;
    r.s = s;
    r.p_mix = (s % CV_B != 0 && s < rir_len) ? s / CV_B : -1;
    r.p_dir_hi = (s + CV_B - 1) / CV_B - 1;
    r.p_tail_lo = s >= rir_len ? P : s / CV_B;
    return r;
}

// H[ic][slot][CV_F], slot = 0 .. P: one wave per spectrum
static __global__ __launch_bounds__(64 * CV_WAVES) void k_reverb_spectra(const float* __restrict__ rir, const int* __restrict__ split,
                                                                          int rir_len, int P, long long n_items, c32* __restrict__ H,
                                                                          const c32* __restrict__ tw) {
    __shared__ c32 buf[CV_WAVES][fft_buf_len<CV_N>()];
    const int lane = threadIdx.x & 63, w = wave_id();
    WaveTw<CV_N> wtw;
    wtw.init(tw, lane);
    for (long long it = (long long)blockIdx.x * CV_WAVES + w; it < n_items; it += (long long)gridDim.x * CV_WAVES) {
        const long long ic = it / (P + 1);
        const int slot = (int)(it % (P + 1));
        const RvSplit sp = rv_split(split, ic, rir_len, P);
        // taps [lo, hi) of the response enter this spectrum, at offsets from `base`
        int base, lo, hi;
        if (slot < P) {
            base = slot * CV_B;
            lo = base;
            hi = min(base + CV_B, rir_len);
            if (slot == sp.p_mix) hi = sp.s;
        } else {
            base = (sp.p_mix < 0 ? 0 : sp.p_mix) * CV_B;
            lo = sp.p_mix < 0 ? 0 : sp.s;
            hi = sp.p_mix < 0 ? 0 : min(base + CV_B, rir_len);
        }
        const float* hr = rir + ic * rir_len;
        c32 v[CV_E];
#pragma unroll
        for (int e = 0; e < CV_E; ++e) {
            const int idx = base + lane + 64 * e;
            const bool in = idx >= lo && idx < hi;
            const float val = hr[idx < rir_len ? idx : rir_len - 1];
            v[e] = make_float2(in ? val : 0.f, 0.f);
        }
        fft_wave<CV_N>(v, wtw, buf[w], lane);
        c32* Ho = H + it * CV_F;
#pragma unroll
        for (int e = 0; e < CV_EH; ++e) Ho[lane + 64 * e] = v[e];
        if (lane == 0) Ho[CV_N / 2] = v[CV_EH];
    }
}

template <int PMAX>
struct alignas(16) ReverbShared {
    c32 H[PMAX + 1][CV_F + 3];                // the P + 1 spectra of this (signal, channel)
    c32 buf[CV_WAVES][fft_buf_len<CV_N>()];
    double red[CV_WAVES][2];
};

// acc += x h over the 513 stored bins of a lane
__device__ __forceinline__ void rv_mac(c32 (&acc)[CV_EH + 1], const c32 (&x)[CV_EH + 1], const c32* __restrict__ h, int lane) {
#pragma unroll
    for (int e = 0; e < CV_EH; ++e) {
        const c32 hv = h[lane + 64 * e];
        acc[e].x = fmaf(x[e].x, hv.x, fmaf(-x[e].y, hv.y, acc[e].x));
        acc[e].y = fmaf(x[e].x, hv.y, fmaf(x[e].y, hv.x, acc[e].y));
    }
    const c32 hv = h[CV_N / 2];
    acc[CV_EH].x = fmaf(x[CV_EH].x, hv.x, fmaf(-x[CV_EH].y, hv.y, acc[CV_EH].x));
    acc[CV_EH].y = fmaf(x[CV_EH].x, hv.y, fmaf(x[CV_EH].y, hv.x, acc[CV_EH].y));
}

// sum of the squared samples [b 512, (b + 1) 512) below Lfull of the block whose spectrum is acc (k_conv_mac_ifft's inverse transform)
__device__ __forceinline__ double rv_block_energy(const c32 (&acc)[CV_EH + 1], const WaveTw<CV_N>& wtw, c32* buf, int lane, int b,
                                                  long long Lfull) {
    DISCO_LDS_WAR();
#pragma unroll
    for (int e = 0; e < CV_EH; ++e) {
        const int f = lane + 64 * e;
        const c32 a = acc[e];
        buf[fft_pad<CV_N>(f)] = make_float2(a.x, -a.y);                       // conj(Z[f])
        if (f != 0) buf[fft_pad<CV_N>(CV_N - f)] = a;                          // conj(Z[N-f]) = Z[f]
    }
    if (lane == 0) buf[fft_pad<CV_N>(CV_N / 2)] = make_float2(acc[CV_EH].x, -acc[CV_EH].y);
    DISCO_LDS_RAW();
    c32 v[CV_E];
#pragma unroll
    for (int e = 0; e < CV_E; ++e) v[e] = buf[fft_pad<CV_N>(lane + 64 * e)];
    fft_wave<CV_N>(v, wtw, buf, lane);
    double en = 0.0;
#pragma unroll
    for (int e = CV_EH; e < CV_E; ++e) {                                       // samples 512 .. 1023 of the window
        const long long pos = (long long)b * CV_B + lane + 64 * (e - CV_EH);
        const double y = (double)(v[e].x * (1.0f / CV_N));
        en += pos < Lfull ? y * y : 0.0;
    }
    return en;
}

template <int PMAX>
__global__ __launch_bounds__(64 * CV_WAVES) void k_reverb_mac_energy(const c32* __restrict__ X, const c32* __restrict__ Hs,
                                                                      const int* __restrict__ split, double* __restrict__ energy,
                                                                      const c32* __restrict__ tw, int n_ch, int n_blocks, int P,
                                                                      int rir_len, long long Lfull) {
    __shared__ ReverbShared<PMAX> sh;
    const int lane = threadIdx.x & 63, w = wave_id();
    const long long ic = blockIdx.x;                       // (signal, channel)
    const long long i = ic / n_ch;
    {
        const c32* src = Hs + ic * (long long)(P + 1) * CV_F;
        for (int q = threadIdx.x; q < (P + 1) * CV_F; q += 64 * CV_WAVES) sh.H[q / CV_F][q % CV_F] = src[q];
    }
    const RvSplit sp = rv_split(split, ic, rir_len, P);
    WaveTw<CV_N> wtw;
    wtw.init(tw, lane);
    __syncthreads();
    const c32* Xi = X + i * (long long)n_blocks * CV_F;
    c32* buf = sh.buf[w];
    double e_d = 0.0, e_r = 0.0;
    const int n_groups = (n_blocks + CV_NB - 1) / CV_NB;
    for (int g = w; g < n_groups; g += CV_WAVES) {
        const int b0 = g * CV_NB;
        c32 acc_d[CV_NB][CV_EH + 1], acc_r[CV_NB][CV_EH + 1];
        bool any_d[CV_NB], any_r[CV_NB];
#pragma unroll
        for (int bb = 0; bb < CV_NB; ++bb) {
            any_d[bb] = any_r[bb] = false;
#pragma unroll
            for (int e = 0; e <= CV_EH; ++e) acc_d[bb][e] = acc_r[bb][e] = make_float2(0.f, 0.f);
        }
        const int j_lo = max(0, b0 - P + 1), j_hi = min(n_blocks - 1, b0 + CV_NB - 1);
        for (int j = j_lo; j <= j_hi; ++j) {
            const c32* Xp = Xi + (long long)j * CV_F;
            c32 x[CV_EH + 1];
#pragma unroll
            for (int e = 0; e < CV_EH; ++e) x[e] = Xp[lane + 64 * e];
            x[CV_EH] = Xp[CV_N / 2];
#pragma unroll
            for (int bb = 0; bb < CV_NB; ++bb) {
                const int p = b0 + bb - j;                 // wave-uniform
                if (p >= 0 && p < P) {
                    if (p <= sp.p_dir_hi) {
                        rv_mac(acc_d[bb], x, sh.H[p], lane);
                        any_d[bb] = true;
                    }
                    if (p >= sp.p_tail_lo) {
                        rv_mac(acc_r[bb], x, sh.H[p == sp.p_mix ? P : p], lane);
                        any_r[bb] = true;
                    }
                }
            }
        }
        // a set without a product is exact zeros and adds nothing
#pragma unroll
        for (int bb = 0; bb < CV_NB; ++bb) {
            const int b = b0 + bb;
            if (b < n_blocks) {                            // wave-uniform
                if (any_d[bb]) e_d += rv_block_energy(acc_d[bb], wtw, buf, lane, b, Lfull);
                if (any_r[bb]) e_r += rv_block_energy(acc_r[bb], wtw, buf, lane, b, Lfull);
            }
        }
    }
    e_d = wave_sum(e_d);
    e_r = wave_sum(e_r);
    if (lane == 0) {
        sh.red[w][0] = e_d;
        sh.red[w][1] = e_r;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double t = 0.0;
#pragma unroll
        for (int ww = 0; ww < CV_WAVES; ++ww) t += sh.red[ww][threadIdx.x];
        energy[ic * 2 + threadIdx.x] = t;
    }
}

}  // namespace disco
