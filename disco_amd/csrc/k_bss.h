// BSS-eval (Vincent, Gribonval, Fevotte 2006; what the reference calls as mir_eval.separation.bss_eval_sources, tango.py:541-567):
// SDR / SIR / SAR of an estimate against nsrc references through a flen-tap filtered projection.  Every figure is a function of lag
// correlations only, so no delayed-reference matrix and no residual signal is ever formed:
//   c_pq[t] = sum_n r_p[n] r_q[n + t],  d_p[t] = sum_n r_p[n] e[n + t],  ee = sum_n e[n]^2          (float32 in, exact float64 products)
//   G = block-Toeplitz (block (p, q) entry (a, b) = c_pq[a - b]),  G = L L^T,  y = L^-1 d
//   p_all = |y|^2 (projection on all delayed references),  p_j = |y[0 : flen]|^2 with source j ordered first.
// Three kernels: k_lag_corr (+ k_lag_reduce) -- where the flops are --, k_bss_factor (blocked left-looking Cholesky, one workgroup per
// factorisation) and k_bss_project (forward substitution + the energies).  All sums run in a fixed order: results are bit-identical
// from run to run and do not depend on what else is in the batch.  No atomics.
#pragma once
#include "common.h"

namespace disco {

// scored end of row / set i: the launch's scalar `stop`, or stop_sig[i] clamped into [start, len] (disco_stoi's rule)
__device__ __forceinline__ int bss_stop(const int* __restrict__ stop_sig, long long i, long long len, int start, int stop) {
    if (!stop_sig) return stop;
    const long long e = stop_sig[i];
    return (int)(e < start ? start : e > len ? len : e);
}

constexpr int BSS_THREADS = 256;
constexpr int BSS_MAX_SRC = 4;
constexpr int BSS_MAX_FLEN = 512;
constexpr int BSS_ENERGIES = 4;                              // {p_j, p_all, ee, status} per (estimate, source)

// ---- lag correlation ---------------------------------------------------------------------------------------------------------
// A workgroup owns (pair, time chunk of LC_SPAN samples) and walks the chunk in LC_PASSES passes of LC_TC samples.  Per pass the
// samples of a and the samples of b widened by the lag range are staged in LDS as float64, zero outside [start, stop) -- the
// inner loop then needs no bounds.  A thread owns LC_LPT = 8 consecutive lags and one of TS time slices of the pass; it keeps a
// sliding window of 12 values of b in registers, so a block of 8 lags x 4 times (32 FMAs) costs 4 new values of b and 4 broadcast
// values of a: 0.25 LDS reads per FMA, all 16-byte reads.  LDS layout: 2 words of padding after every 8 (lc_pos), which puts the
// 64-byte lane stride of the b reads on 80 bytes -- 16 lanes x 16 bytes then cover 16 distinct bank quads.
// The chunk geometry depends on the span and the lag range only, never on the batch: a pair gives the same bits alone or in a batch.
constexpr int LC_TC = 2048;
constexpr int LC_PASSES = 8;
constexpr int LC_SPAN = LC_TC * LC_PASSES;
constexpr int LC_LPT = 8;
constexpr int LC_MAX_NLAG = 2 * BSS_MAX_FLEN - 1;
constexpr int LC_MAX_LG = (LC_MAX_NLAG + LC_LPT - 1) / LC_LPT;                 // 128 lag groups at most: TS >= 2

__device__ __forceinline__ int lc_pos(int e) { return e + ((e >> 3) << 1); }
constexpr int LC_A_WORDS = LC_TC + LC_TC / 4;                                  // lc_pos(LC_TC)
constexpr int LC_B_LOGICAL = LC_TC + LC_MAX_LG * LC_LPT + 8;
constexpr int LC_B_WORDS = LC_B_LOGICAL + LC_B_LOGICAL / 4 + 8;

// rows of the signal pair: mode 0: a[pair], b[pair]; mode 1: references (p, q) of a set; mode 2: reference p and estimate q of
// estimate set `kest` -- pair = set * nsrc^2 + p * nsrc + q in both.
__device__ __forceinline__ void lag_rows(int mode, int nsrc, int n_est, int kest, long long pair, long long& ra, long long& rb) {
    if (mode == 0) {
        ra = rb = pair;
        return;
    }
    const long long set = pair / (nsrc * nsrc);
    const int pq = (int)(pair - set * (nsrc * nsrc));
    const int p = pq / nsrc, q = pq - p * nsrc;
    ra = set * nsrc + p;
    rb = mode == 1 ? set * nsrc + q : (set * n_est + kest) * nsrc + q;
}

// part[pair][chunk][l] = sum over the chunk's n (n and n + t inside [start, stop)) of a[n] b[n + t],  t = lag_lo + l,  l < nlag
// stop_sig: one stop per pair (mode 0) or per reference set (modes 1, 2).  Chunk c starts at start + c LC_SPAN whatever the stop and a
// chunk wholly past the pair's stop writes zero partials, so the sum in chunk order has the bits of a launch with that scalar stop.
static __global__ __launch_bounds__(BSS_THREADS) void k_lag_corr(const float* __restrict__ a, const float* __restrict__ b, long long len,
                                                                 int start, int stop_all, const int* __restrict__ stop_sig, int lag_lo, int nlag,
                                                                 int n_chunk, int mode, int nsrc, int n_est, int kest, double* __restrict__ part) {
    __shared__ double As[LC_A_WORDS] __attribute__((aligned(16)));
    __shared__ double Bs[LC_B_WORDS] __attribute__((aligned(16)));
    const int tid = threadIdx.x;
    const long long pair = blockIdx.x / n_chunk;
    const int chunk = (int)(blockIdx.x - pair * n_chunk);
    long long ra, rb;
    lag_rows(mode, nsrc, n_est, kest, pair, ra, rb);
    const int stop = bss_stop(stop_sig, mode == 0 ? pair : pair / (nsrc * nsrc), len, start, stop_all);
    const float* pa = a + ra * len;
    const float* pb = b + rb * len;
    const int LG = (nlag + LC_LPT - 1) / LC_LPT;
    int TS = 1;
    while (TS * 2 * LG <= BSS_THREADS) TS *= 2;
    const int SL = LC_TC / TS;                                   // samples per time slice: a multiple of 8
    const int nlag_pad = LG * LC_LPT;
    const int nb = LC_TC + nlag_pad + 8;
    const int lg = tid % LG, ts = tid / LG;
    const bool active = ts < TS;
    const int l0 = lg * LC_LPT;
    double acc[LC_LPT];
#pragma unroll
    for (int i = 0; i < LC_LPT; ++i) acc[i] = 0.0;
    for (int pass = 0; pass < LC_PASSES; ++pass) {
        const long long n0 = (long long)start + (long long)chunk * LC_SPAN + (long long)pass * LC_TC;
        if (n0 >= stop) break;                                   // uniform over the workgroup
        __syncthreads();                                         // the previous pass is consumed
        for (int m = tid; m < LC_TC; m += BSS_THREADS) {
            const long long n = n0 + m;
            As[lc_pos(m)] = n < stop ? (double)pa[n] : 0.0;
        }
        for (int e = tid; e < nb; e += BSS_THREADS) {
            const long long n = n0 + lag_lo + e;
            Bs[lc_pos(e)] = (n >= start && n < stop) ? (double)pb[n] : 0.0;
        }
        __syncthreads();
        if (active) {
            const int m0 = ts * SL;
            double w[12];
            {
                const int e0 = m0 + l0;                          // a multiple of 8: the 8 words are contiguous
                const double* src = &Bs[lc_pos(e0)];
#pragma unroll
                for (int k = 0; k < 8; k += 2) {
                    const double2 v = *reinterpret_cast<const double2*>(src + k);
                    w[k] = v.x;
                    w[k + 1] = v.y;
                }
            }
#pragma unroll 2
            for (int m = m0; m < m0 + SL; m += 4) {
                const double* sa = &As[lc_pos(m)];
                const double2 a01 = *reinterpret_cast<const double2*>(sa);
                const double2 a23 = *reinterpret_cast<const double2*>(sa + 2);
                const double* sb = &Bs[lc_pos(m + l0 + 8)];
                const double2 b01 = *reinterpret_cast<const double2*>(sb);
                const double2 b23 = *reinterpret_cast<const double2*>(sb + 2);
                w[8] = b01.x;
                w[9] = b01.y;
                w[10] = b23.x;
                w[11] = b23.y;
                const double av[4] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
                for (int i = 0; i < LC_LPT; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i] += av[j] * w[i + j];       // exact products: float32 x float32 in float64
#pragma unroll
                for (int k = 0; k < 8; ++k) w[k] = w[k + 4];
            }
        }
    }
    __syncthreads();
    double* red = Bs;                                            // [TS][nlag_pad] <= 2048 words
    if (active) {
#pragma unroll
        for (int i = 0; i < LC_LPT; ++i) red[ts * nlag_pad + l0 + i] = acc[i];
    }
    __syncthreads();
    for (int l = tid; l < nlag; l += BSS_THREADS) {
        double s = 0.0;
        for (int t = 0; t < TS; ++t) s += red[t * nlag_pad + l];
        part[((long long)pair * n_chunk + chunk) * nlag + l] = s;
    }
}

// out[pair][l] = sum of the chunk partials in chunk order
static __global__ __launch_bounds__(BSS_THREADS) void k_lag_reduce(const double* __restrict__ part, int n_chunk, int nlag, long long total,
                                                                   double* __restrict__ out) {
    for (long long idx = (long long)blockIdx.x * BSS_THREADS + threadIdx.x; idx < total; idx += (long long)gridDim.x * BSS_THREADS) {
        const long long pair = idx / nlag;
        const int l = (int)(idx - pair * nlag);
        double s = 0.0;
        for (int c = 0; c < n_chunk; ++c) s += part[(pair * n_chunk + c) * nlag + l];
        out[idx] = s;
    }
}

// ---- factorisation ---------------------------------------------------------------------------------------------------------
// Jobs of a reference set: job 0 factors the whole G (sources in their own order, N = nsrc flen): p_all of every estimate, and p_0
// from the leading flen entries of y, because the leading block of L is the factor of G_00.  Job j >= 1 factors the diagonal block
// G_jj alone (N = flen): p_j.  (Ordering source j first and factoring all of G again would give the same p_j at nsrc^3 times the work.)
// The matrices are padded to a multiple of 32 with an identity block, so no tile needs a guard.
constexpr int CH_NB = 32;       // tile
constexpr int CH_RB = 128;      // rows updated together: 256 threads x (4 x 4) entries
constexpr int CH_P = 33;        // LDS pitch in words: rows 4 apart sit 8 banks apart, 8 rows x 8-byte reads cover all 64 banks once

__host__ __device__ __forceinline__ int bss_np(int n) { return (n + CH_NB - 1) & ~(CH_NB - 1); }
// words of factor workspace per set
__host__ __device__ __forceinline__ long long bss_set_words(int nsrc, int flen) {
    const long long n0 = ((long long)nsrc * flen + CH_NB - 1) & ~(long long)(CH_NB - 1), n1 = ((long long)flen + CH_NB - 1) & ~(long long)(CH_NB - 1);
    return n0 * n0 + (nsrc - 1) * n1 * n1;
}

// entry (r, c) of the job's padded G from the set's correlations C[p][q][t] = c_pq[t], t >= 0  (c_pq[-t] = c_qp[t])
__device__ __forceinline__ double bss_g(const double* __restrict__ C, int nsrc, int flen, int job, int N, int r, int c) {
    if (r < c) {
        const int t = r;
        r = c;
        c = t;
    }
    if (r >= N) return r == c ? 1.0 : 0.0;
    int p, q, ia, ib;
    if (job == 0) {
        p = r / flen;
        ia = r - p * flen;
        q = c / flen;
        ib = c - q * flen;
    } else {
        p = q = job;
        ia = r;
        ib = c;
    }
    const int d = ia - ib;
    return d >= 0 ? C[((long long)p * nsrc + q) * flen + d] : C[((long long)q * nsrc + p) * flen - d];
}

// One workgroup per (set, job).  Left-looking by block columns of 32: the block column's rows, 128 at a time, start from G (read
// straight from the correlations), subtract L[rows, 0 : c0] L[c0 : c0 + 32, 0 : c0]^T tile by tile through LDS (a thread holds 4 x 4
// entries: 8 LDS reads per 16 FMAs), then the 32 x 32 diagonal tile is factored in LDS and every row below is solved against it by
// one thread.  L is written once and read ~N / 96 times from HBM / L2: 45 MB per N = 1024, against 180 MB for a right-looking sweep.
// A pivot at or below N eps times its own diagonal entry of G sets stat (the energies of the set become NaN); the sweep goes on with
// that diagonal entry in its place so that nothing non-finite is produced on the way.
static __global__ __launch_bounds__(BSS_THREADS) void k_bss_factor(const double* __restrict__ Crr, double* __restrict__ G, long long set_words,
                                                                   int nsrc, int flen, int* __restrict__ stat) {
    __shared__ double As[CH_RB * CH_P];
    __shared__ double Bs[CH_NB * CH_P];
    __shared__ double Ds[CH_NB * CH_P];
    __shared__ double Dinv[CH_NB];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const long long set = blockIdx.x / nsrc;
    const int job = (int)(blockIdx.x - set * nsrc);
    const int N = job == 0 ? nsrc * flen : flen;
    const int Np = bss_np(N), Np0 = bss_np(nsrc * flen), Np1 = bss_np(flen);
    double* Lw = G + set * set_words + (job == 0 ? 0 : (long long)Np0 * Np0 + (long long)(job - 1) * Np1 * Np1);
    const double* C = Crr + set * nsrc * nsrc * flen;
    const double thr = (double)N * 2.220446049250313e-16;
    const int tr = tid >> 3, tc = tid & 7;
    if (tid == 0) bad = 0;
    for (int c0 = 0; c0 < Np; c0 += CH_NB) {
        for (int g0 = c0; g0 < Np; g0 += CH_RB) {
            const int nrows = (Np - g0) < CH_RB ? (Np - g0) : CH_RB;
            double acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = g0 + tr * 4 + i, c = c0 + tc * 4 + j;
                    acc[i][j] = r < Np ? bss_g(C, nsrc, flen, job, N, r, c) : 0.0;
                }
            for (int kk0 = 0; kk0 < c0; kk0 += CH_NB) {
                __syncthreads();
#pragma unroll
                for (int u = 0; u < CH_RB * CH_NB / BSS_THREADS; ++u) {
                    const int idx = tid + BSS_THREADS * u, row = idx >> 5, col = idx & 31;
                    As[row * CH_P + col] = row < nrows ? Lw[(long long)(g0 + row) * Np + kk0 + col] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < CH_NB * CH_NB / BSS_THREADS; ++u) {
                    const int idx = tid + BSS_THREADS * u, row = idx >> 5, col = idx & 31;
                    Bs[row * CH_P + col] = Lw[(long long)(c0 + row) * Np + kk0 + col];
                }
                __syncthreads();
#pragma unroll 8
                for (int kq = 0; kq < CH_NB; ++kq) {
                    double av[4], bv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) av[i] = As[(tr * 4 + i) * CH_P + kq];
#pragma unroll
                    for (int j = 0; j < 4; ++j) bv[j] = Bs[(tc * 4 + j) * CH_P + kq];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[i][j] -= av[i] * bv[j];
                }
            }
            __syncthreads();                                     // As / Bs are free
            if (g0 == c0) {
                if (tr < CH_NB / 4) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) Ds[(tr * 4 + i) * CH_P + tc * 4 + j] = acc[i][j];
                }
                __syncthreads();
                for (int c = 0; c < CH_NB; ++c) {
                    if (tid == 0) {
                        double piv = Ds[c * CH_P + c];
                        const double gd = bss_g(C, nsrc, flen, job, N, c0 + c, c0 + c);
                        if (!(piv > thr * gd)) {
                            bad = 1;
                            piv = gd > 0.0 ? gd : 1.0;
                        }
                        const double d = sqrt(piv);
                        Ds[c * CH_P + c] = d;
                        Dinv[c] = 1.0 / d;
                    }
                    __syncthreads();
                    if (tid > c && tid < CH_NB) Ds[tid * CH_P + c] *= Dinv[c];
                    __syncthreads();
#pragma unroll
                    for (int u = 0; u < CH_NB * CH_NB / BSS_THREADS; ++u) {
                        const int idx = tid + BSS_THREADS * u, r = idx >> 5, c2 = idx & 31;
                        if (c2 > c && c2 <= r) Ds[r * CH_P + c2] -= Ds[r * CH_P + c] * Ds[c2 * CH_P + c];
                    }
                    __syncthreads();
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) As[(tr * 4 + i) * CH_P + tc * 4 + j] = acc[i][j];
            __syncthreads();
            if (tid < nrows) {
                double* xr = &As[tid * CH_P];
                if (g0 == c0 && tid < CH_NB) {                   // the diagonal tile itself: its factor, zeros above
                    for (int c = 0; c < CH_NB; ++c) xr[c] = c <= tid ? Ds[tid * CH_P + c] : 0.0;
                } else {                                         // x D^T = row  ->  forward substitution along the row
                    double x[CH_NB];
#pragma unroll
                    for (int c = 0; c < CH_NB; ++c) x[c] = xr[c];
#pragma unroll
                    for (int c = 0; c < CH_NB; ++c) {
                        double s = x[c];
#pragma unroll
                        for (int c2 = 0; c2 < c; ++c2) s -= x[c2] * Ds[c * CH_P + c2];
                        x[c] = s * Dinv[c];
                    }
#pragma unroll
                    for (int c = 0; c < CH_NB; ++c) xr[c] = x[c];
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < CH_RB * CH_NB / BSS_THREADS; ++u) {
                const int idx = tid + BSS_THREADS * u, row = idx >> 5, col = idx & 31;
                if (row < nrows) Lw[(long long)(g0 + row) * Np + c0 + col] = As[row * CH_P + col];
            }
        }
    }
    __syncthreads();
    if (tid == 0) stat[set * nsrc + job] = bad;
}

// ---- forward substitution and energies ----------------------------------------------------------------------------------------
// One workgroup per (set, job, pair of estimates of estimate set `kest`): y = L^-1 d for both right-hand sides at once (L is read
// once for the two), block row by block row: 256 threads form the 32 partial products against the y already known (8 threads per
// row, summed in lane order), then wave h solves the 32 x 32 diagonal tile for right-hand side h, one row per lane, the solved
// entry handed on by a shuffle.  Job 0 also sums ee over the estimate itself.
//   all_pairs = 0: out[set][kest][i][4]      estimate i against source i
//   all_pairs = 1: out[set][kest][i][j][4]   estimate i against source j
//   each {p_j, p_all, ee, status}; a set with any stat != 0 gets NaN energies and status 1.
constexpr int PJ_RHS = 2;
constexpr int PJ_MAX_N = BSS_MAX_SRC * BSS_MAX_FLEN;

static __global__ __launch_bounds__(BSS_THREADS) void k_bss_project(const double* __restrict__ Cd, const double* __restrict__ G, long long set_words,
                                                                    const int* __restrict__ stat, const float* __restrict__ ests, long long len,
                                                                    int start, int stop_all, const int* __restrict__ stop_sig, int nsrc, int flen,
                                                                    int n_est, int kest, int all_pairs, double* __restrict__ out,
                                                                    int* __restrict__ status) {
    __shared__ double ys[PJ_RHS][PJ_MAX_N];
    __shared__ double red[PJ_RHS][CH_NB][9];
    __shared__ double rs[3 * PJ_RHS][BSS_THREADS];
    __shared__ double fin[3 * PJ_RHS];
    const int tid = threadIdx.x;
    const int ngrp = (nsrc + PJ_RHS - 1) / PJ_RHS;
    const int grp = blockIdx.x % ngrp;
    const long long sj = blockIdx.x / ngrp;
    const long long set = sj / nsrc;
    const int job = (int)(sj - set * nsrc);
    const int stop = bss_stop(stop_sig, set, len, start, stop_all);
    const int i0 = grp * PJ_RHS;
    const int nr = (nsrc - i0) < PJ_RHS ? (nsrc - i0) : PJ_RHS;
    const int N = job == 0 ? nsrc * flen : flen;
    const int Np = bss_np(N), Np0 = bss_np(nsrc * flen), Np1 = bss_np(flen);
    const double* Lw = G + set * set_words + (job == 0 ? 0 : (long long)Np0 * Np0 + (long long)(job - 1) * Np1 * Np1);
    for (int r = tid; r < Np; r += BSS_THREADS) {
        int p = job, ia = r;
        if (job == 0) {
            p = r / flen;
            ia = r - p * flen;
        }
#pragma unroll
        for (int h = 0; h < PJ_RHS; ++h)
            ys[h][r] = (h < nr && r < N) ? Cd[(((long long)set * nsrc + p) * nsrc + i0 + h) * flen + ia] : 0.0;
    }
    __syncthreads();
    const int row = tid >> 3, cl = tid & 7;
    const int wv = tid >> 6, lane = tid & 63, rr = lane & 31;
    for (int c0 = 0; c0 < Np; c0 += CH_NB) {
        {
            const double* Lr = Lw + (long long)(c0 + row) * Np;
            double s0 = 0.0, s1 = 0.0;
            for (int c = cl; c < c0; c += 8) {
                const double l = Lr[c];
                s0 += l * ys[0][c];
                s1 += l * ys[1][c];
            }
            red[0][row][cl] = s0;
            red[1][row][cl] = s1;
        }
        __syncthreads();
        if (wv < PJ_RHS) {                                       // whole waves: the shuffles below see all 64 lanes
            const int h = wv;
            double t = ys[h][c0 + rr];
#pragma unroll
            for (int q = 0; q < 8; ++q) t -= red[h][rr][q];
            double Lrow[CH_NB];
            const double* Lr = Lw + (long long)(c0 + rr) * Np + c0;
#pragma unroll
            for (int c = 0; c < CH_NB; ++c) Lrow[c] = Lr[c];
            double dg = 1.0;
#pragma unroll
            for (int c = 0; c < CH_NB; ++c) dg = rr == c ? Lrow[c] : dg;
            const double inv = 1.0 / dg;
            double ymine = 0.0;
#pragma unroll
            for (int c = 0; c < CH_NB; ++c) {
                const double yc = __shfl(t * inv, c, 64);        // lane c holds its final t at step c
                if (rr > c) t -= Lrow[c] * yc;
                if (rr == c) ymine = yc;
            }
            if (lane < CH_NB) ys[h][c0 + rr] = ymine;
        }
        __syncthreads();
    }
    double pf[PJ_RHS], pa[PJ_RHS], ee[PJ_RHS];
#pragma unroll
    for (int h = 0; h < PJ_RHS; ++h) {
        pf[h] = pa[h] = ee[h] = 0.0;
        for (int r = tid; r < N; r += BSS_THREADS) {
            const double v = ys[h][r];
            pa[h] += v * v;
            if (r < flen) pf[h] += v * v;
        }
        if (job == 0 && h < nr) {
            const float* pe = ests + (((long long)set * n_est + kest) * nsrc + i0 + h) * len;
            for (int n = start + tid; n < stop; n += BSS_THREADS) {
                const double v = (double)pe[n];
                ee[h] += v * v;
            }
        }
        rs[3 * h + 0][tid] = pf[h];
        rs[3 * h + 1][tid] = pa[h];
        rs[3 * h + 2][tid] = ee[h];
    }
    __syncthreads();
    if (tid < 3 * PJ_RHS) {
        double s = 0.0;
        for (int t = 0; t < BSS_THREADS; ++t) s += rs[tid][t];
        fin[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        int b = 0;
        for (int j = 0; j < nsrc; ++j) b |= stat[set * nsrc + j] != 0;
        const double nanv = __builtin_nan("");
        for (int h = 0; h < nr; ++h) {
            const int i = i0 + h;
            const double vpf = b ? nanv : fin[3 * h], vpa = b ? nanv : fin[3 * h + 1], vee = b ? nanv : fin[3 * h + 2];
            const long long est = ((long long)set * n_est + kest) * nsrc + i;
            if (job == 0) {
                for (int j = 0; j < nsrc; ++j) {
                    if (!all_pairs && j != i) continue;
                    double* o = out + (all_pairs ? (est * nsrc + j) : est) * BSS_ENERGIES;
                    if (j == 0) o[0] = vpf;
                    o[1] = vpa;
                    o[2] = vee;
                    o[3] = b ? 1.0 : 0.0;
                }
            } else if (all_pairs || i == job) {
                out[(all_pairs ? (est * nsrc + job) : est) * BSS_ENERGIES] = vpf;
            }
        }
        if (job == 0 && grp == 0) status[set] = b;
    }
}

// ---- the estimate sets of a room's nodes ------------------------------------------------------------------------------------------
// The three estimate sets the reference scores per node (tango.py:547-549) from the mixture y, the step-2 output sh and the step-1
// output szh, rows [n_sig][len]:  ests[sig][3][2][len] = {sh, y - sh}, {szh, y - szh}, {y, y - sh}, each difference formed in float64
// and rounded to float32 once.  Samples outside [start, stop of the signal) are written as exact zeros and not read.  A workgroup
// walks tiles of (signal, BE_TILE consecutive samples): every load and store of a wave covers 64 consecutive floats.
constexpr int BE_TILE = 4 * BSS_THREADS;

static __global__ __launch_bounds__(BSS_THREADS) void k_bss_estimates(const float* __restrict__ y, const float* __restrict__ sh,
                                                                      const float* __restrict__ szh, long long n_sig, long long len, int start,
                                                                      int stop_all, const int* __restrict__ stop_sig, float* __restrict__ ests) {
    const long long tiles_per_sig = (len + BE_TILE - 1) / BE_TILE, n_tile = n_sig * tiles_per_sig;
    for (long long tile = blockIdx.x; tile < n_tile; tile += gridDim.x) {
        const long long sig = tile / tiles_per_sig;
        const long long n0 = (tile - sig * tiles_per_sig) * BE_TILE;
        const int stop = bss_stop(stop_sig, sig, len, start, stop_all);
        const float *py = y + sig * len, *ps = sh + sig * len, *pz = szh + sig * len;
        float* o = ests + sig * 6 * len;
#pragma unroll
        for (int u = 0; u < BE_TILE / BSS_THREADS; ++u) {
            const long long n = n0 + u * BSS_THREADS + threadIdx.x;
            if (n >= len) break;
            float vy = 0.f, vs = 0.f, vz = 0.f, dys = 0.f, dyz = 0.f;
            if (n >= start && n < stop) {
                vy = py[n], vs = ps[n], vz = pz[n];
                dys = (float)((double)vy - (double)vs);
                dyz = (float)((double)vy - (double)vz);
            }
            o[n] = vs;
            o[len + n] = dys;
            o[2 * len + n] = vz;
            o[3 * len + n] = dyz;
            o[4 * len + n] = vy;
            o[5 * len + n] = dys;
        }
    }
}

}  // namespace disco
