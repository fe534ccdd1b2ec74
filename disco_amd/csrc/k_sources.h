// Dry sources prepared on the device (disco_theque/dataset_utils/signal_setups.py:42-138, sigproc_utils.py:257-279):
//   noise_from_signal   one long real transform per signal, the magnitudes given random phases, and the inverse
//   k_affine_segment    (x - mean) * gain written at an offset, read from a start with wrap-around
//
// ---- the long transform -------------------------------------------------------------------------------------------------------------------
// A real signal of n_fft = 2 M points is transformed as the complex signal z[n] = x[2 n] + i x[2 n + 1] of M = 2^q points, 9 <= q <= 21.
// The complex transform is a Stockham auto-sort schedule over GLOBAL memory: pass j of radix R, with P the product of the radices before it
// and S = M / R, computes for every butterfly i in [0, S), k = i mod P,
//     u[r] = src[i + r S] W_{P R}^{k r},   U = DFT_R(u),   dst[(i - k) R + k + r P] = U[r],       r < R
// out of place, between the two halves of the context's workspace; after the last pass dst holds the spectrum in natural order.  It is the
// formula of fft_pass (fft.h) one level up: the radices 512 and 1024 ARE the in-register wave transform of fft.h (k_src_wave_pass: a wave
// per group of butterflies, the long-transform twiddle applied on the way in), the radices 4, 8, 16 the register DFTs (k_src_small_pass:
// a lane per butterfly).  src_plan() lists the radices per q; wave radices come first, where P is small and their stores are whole runs of
// lanes, register radices last, where a lane's neighbours are its neighbours in memory on both sides.
//   k_src_wave_pass    SRC_T = 4 consecutive butterflies per wave: every access of a strided pass is then 32 contiguous bytes per lane
//                      instead of 8, and the 4 waves of a workgroup take 16 consecutive butterflies -- whole 128-byte lines
//   k_src_mid          Z -> X (untangle) -> |X| (cos 2 pi u + i sin 2 pi u) -> conj(V) / M (the half-length packing of the inverse), in place
// The inverse runs the same forward passes on conj(V) / M: w = FFT(conj V / M), x[2 n] = Re w[n], x[2 n + 1] = -Im w[n].
// Twiddles W_N^j, j < M, come from a table the host computed in float64 (api_sources.hip); W_M^j is its entry 2 j, negated beyond the half
// circle.  No atomics, no cross-signal state: a signal's bits do not depend on the batch.
#pragma once
#include <cstdint>

#include "fft.h"

namespace disco {

constexpr int SRC_T = 4;          // consecutive butterflies a wave of k_src_wave_pass takes
constexpr int SRC_WAVES = 4;      // waves per workgroup there
constexpr int SRC_MIN_LOG2 = 10, SRC_MAX_LOG2 = 22;       // n_fft = 2^p

// radices of the M = 2^q point complex transform, q = p - 1 in [9, 21]; 0 ends the list
struct SrcPlan {
    int radix[3];
};
__host__ __device__ inline SrcPlan src_plan(int q) {
    switch (q) {
        case 9: return {{512, 0, 0}};
        case 10: return {{1024, 0, 0}};
        case 11: return {{512, 4, 0}};
        case 12: return {{512, 8, 0}};
        case 13: return {{512, 16, 0}};
        case 14: return {{1024, 16, 0}};
        case 15: return {{512, 8, 8}};
        case 16: return {{512, 16, 8}};
        case 17: return {{512, 16, 16}};
        case 18: return {{512, 512, 0}};
        case 19: return {{512, 1024, 0}};
        case 20: return {{1024, 1024, 0}};
        case 21: return {{512, 512, 8}};
        default: return {{0, 0, 0}};
    }
}

// what a pass reads and writes: the complex workspace, or the real signal on the outer side of the first / last pass
struct SrcIo {
    const c32* src;          // complex input rows [n_sig][M]                         (real_in == 0)
    c32* dst;                // complex output rows [n_sig][M]                        (real_out == 0)
    const float* x;          // real input rows [n_sig][len], read below L only       (real_in == 1)
    float* out;              // real output rows [n_sig][len]                         (real_out == 1)
    const int* stop;         // one L per signal or NULL (= len), clamped into [0, min(len, n_fft)]
    const c32* tw;           // W_N^j, j < M
    int M, len, real_in, real_out;
};

__device__ __forceinline__ int src_length(const SrcIo& io, long long sig) {
    const int cap = min(io.len, 2 * io.M);
    return io.stop ? min(max(io.stop[sig], 0), cap) : cap;
}

// W_M^j, j < M, from the table of W_N^j (N = 2 M, half a circle)
__device__ __forceinline__ c32 src_twiddle(const c32* __restrict__ tw, int j, int M) {
    const int j2 = 2 * j;
    if (j2 < M) return tw[j2];
    const c32 t = tw[j2 - M];
    return make_float2(-t.x, -t.y);
}

// z[n] of the packed real signal: samples at or beyond L are zero and are not read
__device__ __forceinline__ c32 src_load_real(const float* __restrict__ xr, int n, int L) {
    const int a = 2 * n;
    return make_float2(a < L ? xr[a] : 0.f, a + 1 < L ? xr[a + 1] : 0.f);
}
// samples 2 n, 2 n + 1 of the output from w[n]: the value below L, zero from L to the end of the row
__device__ __forceinline__ void src_store_real(float* __restrict__ orow, int n, c32 w, int L, int len) {
    const int a = 2 * n;
    if (a < len) orow[a] = a < L ? w.x : 0.f;
    if (a + 1 < len) orow[a + 1] = a + 1 < L ? -w.y : 0.f;
}

// One pass of radix N = 512 / 1024.  A wave takes the T butterflies i0 .. i0 + T - 1 of one signal (T = 1: the single-pass plans, where
// S = 1); `items` = n_sig * S / T.  P >= T or P == 1 (the host's plans: P is 1 or >= 512), S % T == 0.
template <int N, int T>
__global__ __launch_bounds__(64 * SRC_WAVES) void k_src_wave_pass(SrcIo io, int P, long long items) {
    constexpr int E = FftPlan<N>::E;
    __shared__ c32 buf[SRC_WAVES][fft_buf_len<N>()];
    const int lane = threadIdx.x & 63, w = wave_id();
    const long long it = (long long)blockIdx.x * SRC_WAVES + w;
    if (it >= items) return;                                   // wave-uniform; the exchange buffers are wave-private
    const int M = io.M, S = M / N, per_sig = S / T;
    const long long sig = it / per_sig;
    const int i0 = (int)(it - sig * per_sig) * T;
    const int L = src_length(io, sig);
    const int k0 = i0 & (P - 1), step = S / P;                 // W_{P N}^{k r} = W_M^{k r step}
    WaveTw<N> wtw;
    wtw.init(io.tw + M + (N == 512 ? 1024 : 0), lane);         // the 1024- and 512-point tables follow the long one (api_sources.hip)
    c32 d[T][E];
    if (io.real_in) {
        const float* xr = io.x + sig * io.len;
#pragma unroll
        for (int e = 0; e < E; ++e)
#pragma unroll
            for (int t = 0; t < T; ++t) d[t][e] = src_load_real(xr, i0 + t + (lane + 64 * e) * S, L);
    } else {
        const c32* sr = io.src + sig * M;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const c32* p = sr + i0 + (long long)(lane + 64 * e) * S;
            if constexpr (T == 4) {
                const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 2);
                d[0][e] = make_float2(a.x, a.y), d[1][e] = make_float2(a.z, a.w);
                d[2][e] = make_float2(b.x, b.y), d[3][e] = make_float2(b.z, b.w);
            } else {
#pragma unroll
                for (int t = 0; t < T; ++t) d[t][e] = p[t];
            }
        }
    }
    float* orow = io.real_out ? io.out + sig * io.len : nullptr;
    c32* dr = io.real_out ? nullptr : io.dst + sig * M;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        c32 v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = d[t][e];
        if (P > 1) {
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = cmul(v[e], src_twiddle(io.tw, (k0 + t) * (lane + 64 * e) * step, M));
        }
        fft_wave<N>(v, wtw, buf[w], lane);
        if (P == 1) {                                          // dst[i N + r]: a run of lanes is a run of memory
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int pos = (i0 + t) * N + lane + 64 * e;
                if (io.real_out) src_store_real(orow, pos, v[e], L, io.len);
                else dr[pos] = v[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < E; ++e) d[t][e] = v[e];
        }
    }
    if (P > 1) {                                               // dst[(i0 - k0) N + k0 + t + r P]: T consecutive values per lane
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const long long pos = (long long)(i0 - k0) * N + k0 + (long long)(lane + 64 * e) * P;
            if (io.real_out) {
#pragma unroll
                for (int t = 0; t < T; ++t) src_store_real(orow, (int)pos + t, d[t][e], L, io.len);
            } else if constexpr (T == 4) {
                *reinterpret_cast<float4*>(dr + pos) = make_float4(d[0][e].x, d[0][e].y, d[1][e].x, d[1][e].y);
                *reinterpret_cast<float4*>(dr + pos + 2) = make_float4(d[2][e].x, d[2][e].y, d[3][e].x, d[3][e].y);
            } else {
#pragma unroll
                for (int t = 0; t < T; ++t) dr[pos + t] = d[t][e];
            }
        }
    }
}

constexpr int SRC_THREADS = 256;

// One pass of radix R = 4 / 8 / 16, a lane per butterfly: lanes i, i + 1 read and write neighbouring elements (P >= 64).
// `blocks_per_sig` workgroups cover the S = M / R butterflies of a signal.  Never the first pass: P > 1, complex input.
template <int R>
__global__ __launch_bounds__(SRC_THREADS) void k_src_small_pass(SrcIo io, int P, int blocks_per_sig) {
    const long long sig = blockIdx.x / blocks_per_sig;
    const int i = (int)(blockIdx.x - sig * blocks_per_sig) * SRC_THREADS + (int)threadIdx.x;
    const int M = io.M, S = M / R;
    if (i >= S) return;
    const int k = i & (P - 1), step = S / P;
    const c32* sr = io.src + sig * M;
    c32 u[R];
#pragma unroll
    for (int r = 0; r < R; ++r) u[r] = sr[i + (long long)r * S];
#pragma unroll
    for (int r = 1; r < R; ++r) u[r] = cmul(u[r], src_twiddle(io.tw, k * r * step, M));
    dftR<R>(u);
    const long long o = (long long)(i - k) * R + k;
    if (io.real_out) {
        const int L = src_length(io, sig);
        float* orow = io.out + sig * io.len;
#pragma unroll
        for (int r = 0; r < R; ++r) src_store_real(orow, (int)(o + (long long)r * P), u[r], L, io.len);
    } else {
        c32* dr = io.dst + sig * M;
#pragma unroll
        for (int r = 0; r < R; ++r) dr[o + (long long)r * P] = u[r];
    }
}

// cos 2 pi u + i sin 2 pi u for u in turns: the argument is reduced before the sine and cosine are evaluated, so the error of the factor
// does not grow with the angle
__device__ __forceinline__ c32 src_unit(float u) {
#if defined(__clang__)
    float sn, cs;
    sincospif(2.f * u, &sn, &cs);
    return make_float2(cs, sn);
#else
    const double a = 6.283185307179586476925286766559 * (double)u;
    return make_float2((float)cos(a), (float)sin(a));
#endif
}
__device__ __forceinline__ float src_abs(c32 a) { return sqrtf(a.x * a.x + a.y * a.y); }

// Between the transforms, in place on Z [n_sig][M], a thread per pair (k, M - k), k <= M / 2; phase [n_sig][M + 1] in turns.
//   untangle   E = (Z[k] + conj Z[M-k]) / 2, O = -i (Z[k] - conj Z[M-k]) / 2:   X[k] = E + W_N^k O,   X[M-k] = conj(E - W_N^k O)
//   phases     Y[k] = |X[k]| (cos 2 pi u_k + i sin 2 pi u_k);  bins 0 and M (Nyquist) keep the real part only, as irfft does
//   packing    E' = (Y[k] + conj Y[M-k]) / 2, O' = conj(W_N^k) (Y[k] - conj Y[M-k]) / 2:   V[k] = E' + i O',   V[M-k] = conj(E') + i conj(O')
//   stored     conj(V) / M: the inverse is a forward transform of it, its scale 1 / M (the 1 / n_fft of irfft and the halves above)
__global__ __launch_bounds__(SRC_THREADS) void k_src_mid(c32* __restrict__ Z, const float* __restrict__ phase, const c32* __restrict__ tw, int M,
                                                          int blocks_per_sig) {
    const long long sig = blockIdx.x / blocks_per_sig;
    const int k = (int)(blockIdx.x - sig * blocks_per_sig) * SRC_THREADS + (int)threadIdx.x;
    if (k > M / 2) return;
    c32* z = Z + sig * M;
    const float* u = phase + sig * ((long long)M + 1);
    const float inv = 1.0f / (float)M;
    if (k == 0) {
        const c32 a = z[0];
        const float y0 = fabsf(a.x + a.y) * src_unit(u[0]).x, ym = fabsf(a.x - a.y) * src_unit(u[M]).x;
        z[0] = make_float2(0.5f * (y0 + ym) * inv, -0.5f * (y0 - ym) * inv);
        return;
    }
    const c32 a = z[k], b = z[M - k], wk = tw[k];
    const c32 e = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
    const c32 o = cmul_mi(make_float2(0.5f * (a.x - b.x), 0.5f * (a.y + b.y)));
    const c32 wo = cmul(wk, o);
    const c32 xk = cadd(e, wo), xm = cconj(csub(e, wo));
    const float mk = src_abs(xk), mm = src_abs(xm);
    const c32 pk = src_unit(u[k]), pm = src_unit(u[M - k]);
    const c32 yk = make_float2(mk * pk.x, mk * pk.y), ym = make_float2(mm * pm.x, mm * pm.y);
    const c32 e2 = make_float2(0.5f * (yk.x + ym.x), 0.5f * (yk.y - ym.y));
    const c32 o2 = cmul(cconj(wk), make_float2(0.5f * (yk.x - ym.x), 0.5f * (yk.y + ym.y)));
    const c32 io2 = cmul_pi(o2);
    const c32 vk = cadd(e2, io2);                              // V[k];  conj V[M-k] = E' - i O'
    const c32 vmc = csub(e2, io2);
    z[k] = make_float2(vk.x * inv, -vk.y * inv);
    if (k != M - k) z[M - k] = make_float2(vmc.x * inv, vmc.y * inv);
}

// zeros in [from, len) of every row: the part of a row beyond n_fft, which no pass writes
__global__ __launch_bounds__(SRC_THREADS) void k_src_zero_tail(float* __restrict__ out, long long n_sig, int len, int from) {
    const long long per = len - from, n = n_sig * per;
    for (long long q = (long long)blockIdx.x * SRC_THREADS + threadIdx.x; q < n; q += (long long)gridDim.x * SRC_THREADS) {
        const long long sig = q / per;
        out[sig * len + from + (q - sig * per)] = 0.f;
    }
}

// ---- subtract, scale, shift, wrap ---------------------------------------------------------------------------------------------------------
constexpr int AFF_THREADS = 256;
constexpr int AFF_CHUNK = AFF_THREADS * 4;            // output samples of one row a workgroup takes per step

// the subtraction and the product each rounded in float64, one rounding to float32
__device__ __forceinline__ float affine_one(float x, double mean, double gain) {
    const double d = (double)x - mean;
    return (float)(d * gain);
}

// out[i][lead + t] = (x[i][(start_i + t) mod L_i] - mean_i) gain_i for 0 <= t < min(count_i, out_len - lead), exact zeros elsewhere in
// [0, out_len).  A workgroup takes AFF_CHUNK output samples of one row per step of a grid-stride loop over (row, chunk).  VEC: len and
// out_len are multiples of 4 and both arrays are 16-byte aligned (the host checks): every store is a float4, and a quad whose four
// sources are one aligned run inside [0, L) is read as a float4; any other quad -- at the segment's ends, across the wrap, or with
// (start - lead) no multiple of 4 -- is read by element.  Nothing of x at or beyond L is read.
template <bool VEC>
__global__ __launch_bounds__(AFF_THREADS) void k_affine_segment(const float* __restrict__ x, const int* __restrict__ stop, const int* __restrict__ start,
                                                                const int* __restrict__ count, const double* __restrict__ mean,
                                                                const double* __restrict__ gain, int lead, float* __restrict__ out,
                                                                long long n_sig, int len, int out_len) {
    const int chunks = (out_len + AFF_CHUNK - 1) / AFF_CHUNK;
    const long long items = n_sig * chunks;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long row = it / chunks;
        const int o0 = (int)(it - row * chunks) * AFF_CHUNK + (int)threadIdx.x * 4;
        if (o0 >= out_len) continue;
        const int L = stop ? min(max(stop[row], 0), len) : len;
        const long long cnt_in = L == 0 ? 0 : (count ? max(count[row], 0) : L);
        const int cnt = (int)(cnt_in < (long long)(out_len - lead) ? cnt_in : (long long)(out_len - lead));      // samples of the segment
        const double m = mean ? mean[row] : 0.0, g = gain ? gain[row] : 1.0;
        const float* xr = x + row * len;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const int n = VEC ? 4 : min(4, out_len - o0);
        const int t0 = o0 - lead;                                              // may be negative: before the segment
        if (cnt > 0 && t0 + 4 > 0 && t0 < cnt) {                                // the quad meets the segment, which is not empty: L > 0
            int st = start ? start[row] % L : 0;
            st = st < 0 ? st + L : st;
            const int tf = max(t0, 0);
            int sidx = (int)(((long long)st + tf) % L);                        // source of the first sample of the quad inside the segment
            if (VEC && t0 >= 0 && t0 + 4 <= cnt && (sidx & 3) == 0 && sidx + 4 <= L) {
                const float4 q = *reinterpret_cast<const float4*>(xr + sidx);
                v[0] = affine_one(q.x, m, g), v[1] = affine_one(q.y, m, g), v[2] = affine_one(q.z, m, g), v[3] = affine_one(q.w, m, g);
            } else {
                for (int j = tf - t0; j < 4 && t0 + j < cnt; ++j) {
                    v[j] = affine_one(xr[sidx], m, g);
                    sidx = sidx + 1 == L ? 0 : sidx + 1;
                }
            }
        }
        float* orow = out + row * out_len;
        if (VEC) {
            *reinterpret_cast<float4*>(orow + o0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (int j = 0; j < n; ++j) orow[o0 + j] = v[j];
        }
    }
}

}  // namespace disco
