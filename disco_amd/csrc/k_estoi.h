// ESTOI, the extended short-time objective intelligibility measure (Jensen, Taal 2016; what pystoi computes with extended=True), batched
// over (clean, processed) pairs.  Stages 1 - 3 are those of STOI (k_stoi.h: resampling, silent-frame removal, the third-octave envelopes
// tob_x, tob_y [pair][15][T]); only the last stage differs.  With J = T - 29 segments and, for segment m, Xm = X[:, m : m + 30] and Ym alike,
// in float64:
//   rows:     every row of Xm, Ym minus its mean over the 30 frames, divided by (its norm + EPS)
//   columns:  every column of the row-normalised matrices minus its mean over the 15 bands, divided by (its norm + EPS)
//   d_m = sum(Xn o Yn) / 30,  d = sum_m d_m / J
// Restated from the definition; pystoi is third-party and absent, so this is pinned by the float64 yardstick of tests/estoi_checks.py, not
// against the package.  pystoi adds EPS randn to the matrices before each normalisation so that it never divides by zero; that jitter is
// not reproduced (it moves d by some 1e-15 on the compared cases): the result is deterministic, and a row or column whose centred norm
// is exactly 0 contributes 0 through the "+ EPS" of its denominator.
//   k_estoi_corr     a workgroup owns ESTOI_SEGS consecutive segments of one pair -> its partial sum in part[pair][chunk]
//   k_estoi_finish   the partial sums in chunk order, / (30 J), the status and the count of frames
// Every sum runs in a fixed order and the launch geometry of a pair depends on that pair's frame count alone: a pair gives the same bits
// alone, in any batch and from run to run.  No atomics.
#pragma once
#include "k_stoi.h"

namespace disco {

constexpr int ESTOI_SEGS = 64;                                   // segments per workgroup: one wave-width, so that a wave walks one frame offset
constexpr int ESTOI_SLAB = ESTOI_SEGS + STOI_SEG - 1;            // envelope frames a workgroup reads per band

// frames T of pair `pair`: frames[pair] - sub clamped into [.., tmax] (disco_estoi: the kept frames minus one; disco_estoi_bands: the
// caller's count), or tmax without `frames`
__device__ __forceinline__ int estoi_T(const int* __restrict__ frames, int sub, int tmax, long long pair) {
    const int T = frames ? frames[pair] - sub : tmax;
    return T > tmax ? tmax : T;
}

// grid = n_pair * n_chunk, block = (pair, segments [chunk S, chunk S + S)).
//   1. the 15 x (S + 29) slab of both envelopes -> LDS (float32 as stored; every later use converts to float64)
//   2. item (band, segment): mean and 1 / (norm of the centred row + EPS) of x and y, each a plain 30-term sum in frame order
//   3. item (frame offset n, segment): the column of 15 row-normalised values of x and y, centred, divided by (norm + EPS), multiplied and
//      summed in band order; a lane adds its items in ascending order
//   4. the 256 lane sums in a fixed tree -> part[pair][chunk]
static __global__ __launch_bounds__(STOI_THREADS) void k_estoi_corr(const float* __restrict__ tob_x, const float* __restrict__ tob_y,
                                                                     const int* __restrict__ frames, int sub, int tmax, int n_chunk,
                                                                     double* __restrict__ part) {
    __shared__ float sx[STOI_BANDS][ESTOI_SLAB], sy[STOI_BANDS][ESTOI_SLAB];
    __shared__ double mx[STOI_BANDS][ESTOI_SEGS], my[STOI_BANDS][ESTOI_SEGS], ix[STOI_BANDS][ESTOI_SEGS], iy[STOI_BANDS][ESTOI_SEGS];
    __shared__ double red[STOI_THREADS];
    const long long pair = blockIdx.x / n_chunk;
    const int chunk = (int)(blockIdx.x - pair * n_chunk);
    const int tid = threadIdx.x;
    const int T = estoi_T(frames, sub, tmax, pair);
    const int J = T - (STOI_SEG - 1);
    const int s0 = chunk * ESTOI_SEGS;
    if (J <= 0 || s0 >= J) return;                               // uniform over the workgroup, before any barrier
    const int nseg = J - s0 < ESTOI_SEGS ? J - s0 : ESTOI_SEGS;
    const int ncol = nseg + STOI_SEG - 1;                        // s0 + ncol <= T <= tmax
    for (int i = tid; i < STOI_BANDS * ESTOI_SLAB; i += STOI_THREADS) {
        const int band = i / ESTOI_SLAB, c = i - band * ESTOI_SLAB;
        const long long at = (pair * STOI_BANDS + band) * tmax + s0 + c;
        sx[band][c] = c < ncol ? tob_x[at] : 0.f;
        sy[band][c] = c < ncol ? tob_y[at] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < STOI_BANDS * ESTOI_SEGS; i += STOI_THREADS) {
        const int band = i / ESTOI_SEGS, s = i - band * ESTOI_SEGS;
        if (s < nseg) {
            double ax = 0.0, ay = 0.0;
#pragma unroll
            for (int n = 0; n < STOI_SEG; ++n) {
                ax += (double)sx[band][s + n];
                ay += (double)sy[band][s + n];
            }
            ax /= STOI_SEG;
            ay /= STOI_SEG;
            double qx = 0.0, qy = 0.0;
#pragma unroll
            for (int n = 0; n < STOI_SEG; ++n) {
                const double vx = (double)sx[band][s + n] - ax, vy = (double)sy[band][s + n] - ay;
                qx += vx * vx;
                qy += vy * vy;
            }
            mx[band][s] = ax;
            my[band][s] = ay;
            ix[band][s] = 1.0 / (sqrt(qx) + STOI_EPS);
            iy[band][s] = 1.0 / (sqrt(qy) + STOI_EPS);
        }
    }
    __syncthreads();
    double d = 0.0;
    for (int i = tid; i < STOI_SEG * ESTOI_SEGS; i += STOI_THREADS) {
        const int n = i / ESTOI_SEGS, s = i - n * ESTOI_SEGS;
        if (s < nseg) {
            double xs[STOI_BANDS], ys[STOI_BANDS];
            double ax = 0.0, ay = 0.0;
#pragma unroll
            for (int b = 0; b < STOI_BANDS; ++b) {
                xs[b] = ((double)sx[b][s + n] - mx[b][s]) * ix[b][s];
                ys[b] = ((double)sy[b][s + n] - my[b][s]) * iy[b][s];
                ax += xs[b];
                ay += ys[b];
            }
            ax /= STOI_BANDS;
            ay /= STOI_BANDS;
            double qx = 0.0, qy = 0.0;
#pragma unroll
            for (int b = 0; b < STOI_BANDS; ++b) {
                xs[b] -= ax;
                ys[b] -= ay;
                qx += xs[b] * xs[b];
                qy += ys[b] * ys[b];
            }
            const double cx = 1.0 / (sqrt(qx) + STOI_EPS), cy = 1.0 / (sqrt(qy) + STOI_EPS);
            double e = 0.0;
#pragma unroll
            for (int b = 0; b < STOI_BANDS; ++b) e += (xs[b] * cx) * (ys[b] * cy);
            d += e;
        }
    }
    red[tid] = d;
    __syncthreads();
    for (int o = STOI_THREADS / 2; o >= 1; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) part[pair * n_chunk + chunk] = red[0];
}

// out[pair] = {d, count}, status[pair].  spans != 0 (disco_estoi): count = the kept frames of the pair's span, T = count - 1; status 0
// scored, 1 fewer than 30 frames (d = 1e-5), 2 the span gives no frame at all (d = NaN).  spans == 0 (disco_estoi_bands): count = T = the
// caller's frames clamped into [0, tmax]; status 0 or 1.
static __global__ __launch_bounds__(STOI_THREADS) void k_estoi_finish(const double* __restrict__ part, const int* __restrict__ frames, int sub, int tmax,
                                                                       int n_chunk, int spans, long long len, int start, const int* __restrict__ stop,
                                                                       int p, int q, long long n_pair, double* __restrict__ out,
                                                                       int* __restrict__ status) {
    const long long pair = (long long)blockIdx.x * STOI_THREADS + threadIdx.x;
    if (pair >= n_pair) return;
    const int NF = spans ? stoi_frames(stoi_len10(stoi_span(len, start, stop, pair), p, q)) : 1;
    int T = NF > 0 ? estoi_T(frames, sub, tmax, pair) : -1;
    if (!spans && T < 0) T = 0;
    double d;
    int st;
    if (NF == 0) {
        d = __builtin_nan("");
        st = 2;
    } else if (T < STOI_SEG) {
        d = 1e-5;
        st = 1;
    } else {
        const int J = T - (STOI_SEG - 1);
        const int nch = (J + ESTOI_SEGS - 1) / ESTOI_SEGS;
        double s = 0.0;
        for (int c = 0; c < nch; ++c) s += part[pair * n_chunk + c];
        d = s / ((double)STOI_SEG * (double)J);
        st = 0;
    }
    out[2 * pair] = d;
    out[2 * pair + 1] = (double)(NF > 0 ? T + sub : 0);
    status[pair] = st;
}

}  // namespace disco
