// The online / adaptive MWF with COMPANIONS (disco_online_mwf_ref): the recursion, the solve and the `out` of k_online.h, and at every
// frame the filter in force applied to one or two further inputs laid out as X / Z -- the target and the noise image of the mixture:
//     out^c_t = w_t^H v^c_t,       v^c_t = [X^c_k(t, f, 0..M-1) ; Z^c_j(t, f), j < k ; Z^c_j(t, f), j > k]
// which is what every score of the reference needs (tango.py:541-593: sf, nf, z_s, z_n through the SAME filters as the mixture).  A
// filter history for a second pass would be P times the size of the output (one update per frame), so the companions ride through the
// walk itself.  They never enter Rss, Rnn or the solve: out and w_last are those of the plain kernels, bit for bit.
//
// Sibling kernels, not a template parameter of k_online_mwf / k_online_mwf_thread and not a frame body shared with them: moving the plain
// kernels' body into a function both forms inline changed hipcc's register allocation of six plain instantiations (thread<2, true>,
// <6, true>, <7, *>, group <7>, <15>), and the plain kernels are to stay what they are.  The walk below is theirs, statement for
// statement in everything that feeds `out` (the order of additions included), without the resumable state of the stream: scoring is a
// whole-clip job.
#pragma once
#include "k_online.h"

namespace disco {

struct OnlineComp {
    const c32* X[2];     // [R][Kl][T][F][M] each
    const c32* Z[2];     // [R][K][T][F] each, in the layout of OnlineArgs::Z (zblk), or NULL (P == M)
    c32* out[2];         // [R][Kl][T][F] each
    int n;               // 1 or 2
};

// entry c of a companion's v_t; xb: the problem's rows of its X, zb: its Z + f or NULL
__device__ __forceinline__ c32 online_comp_row(const OnlineArgs& a, const c32* xb, const c32* zb, int c, int t, int k, long long r, long long TF) {
    const int M = a.M;
    if (c < M) return xb[(long long)t * a.F * M + c];
    const int jn = (c - M) < k ? (c - M) : (c - M) + 1;        // skip the node's own z
    return zb ? zb[z_plane(r, jn, a.K, a.R, a.zblk) * TF + (long long)t * a.F] : make_float2(0.f, 0.f);
}

template <int P>
__global__ __launch_bounds__(SolveGeom<P>::THREADS, (P > 4 && P <= 8) ? DISCO_ONLINE_WPE : 1) void k_online_mwf_ref(OnlineArgs a, OnlineComp cm) {
    constexpr int G = SolveGeom<P>::G, PROBS = SolveGeom<P>::PROBS;
    __shared__ c64 s_L[PROBS][SolveGeom<P>::LSZ];
    __shared__ c64 s_Y[PROBS][P][SolveGeom<P>::YW];
    const int j = threadIdx.x % G;
    const int slot = threadIdx.x / G;
    const long long pid = (long long)blockIdx.x * PROBS + slot;
    const bool live = pid < a.n_prob;
    const bool col = live && j < P;
    const long long pc = live ? pid : 0;                  // dead groups walk problem 0 and write nothing
    const long long g = pc / a.F;                         // (room, local node)
    const int f = (int)(pc % a.F);
    const long long r = g / a.Kl;
    const int k = a.k0 + (int)(g % a.Kl);                 // global node index (remote-row order depends on it)
    const int M = a.M;

    const c32* xb = a.X + ((g * a.Tx + a.tx0) * a.F + f) * (long long)M;
    const c32* zb = a.Z ? a.Z + f : nullptr;
    const long long TF = (long long)a.Tm * a.F;
    const float* mp = a.mask + (g * a.Tm) * a.F + f;

    c32 rowA[P], rowB[P];
#pragma unroll
    for (int c = 0; c < P; ++c) {
        rowA[c] = make_float2(0.f, 0.f);
        rowB[c] = make_float2(c == j ? (col ? a.init_diag : 1.f) : 0.f, 0.f);
    }
    const float lam = a.lambda_cor, oml = 1.f - a.lambda_cor;
    c32 wj = make_float2(0.f, 0.f);
    int until_update = 0;
    for (int t = 0; t < a.T; ++t) {
        c32 v[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            if (c < M) {
                v[c] = xb[(long long)t * a.F * M + c];
            } else {
                const int jn = (c - M) < k ? (c - M) : (c - M) + 1;        // skip the node's own z
                v[c] = zb ? zb[z_plane(r, jn, a.K, a.R, a.zblk) * TF + (long long)t * a.F] : make_float2(0.f, 0.f);
            }
        }
        const float m = mp[(long long)t * a.F];
        c32 vj = make_float2(0.f, 0.f);
#pragma unroll
        for (int c = 0; c < P; ++c) {
            if (c == j) vj = v[c];
        }
        if (col) {
            const float cs = oml * m, cn = oml * (1.f - m);
#pragma unroll
            for (int c = 0; c < P; ++c) {
                float pr, pi;                                            // v_j conj(v_c), every product rounded on its own as in k_online_mwf
                {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
                    pr = vj.x * v[c].x + vj.y * v[c].y;
                    pi = vj.y * v[c].x - vj.x * v[c].y;
                }
                rowA[c] = make_float2(lam * rowA[c].x + cs * pr, lam * rowA[c].y + cs * pi);
                rowB[c] = make_float2(lam * rowB[c].x + cn * pr, lam * rowB[c].y + cn * pi);
            }
        }
        if (until_update == 0) {                           // block-uniform: every group updates at the same frames
            c64 t1;
            double gain;
            gevd_solve_group<P, true>(rowA, rowB, s_L[slot], s_Y[slot], j, a.mu, t1, gain);
            wj = make_float2((float)(t1.x * gain), (float)(t1.y * gain));
            until_update = a.update_every;
        }
        --until_update;
        // out_t = sum_j conj(w_j) v_j over the group's lanes
        float orx = j < P ? wj.x * vj.x + wj.y * vj.y : 0.f;
        float oix = j < P ? wj.x * vj.y - wj.y * vj.x : 0.f;
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
            orx += __shfl_xor(orx, off, G);
            oix += __shfl_xor(oix, off, G);
        }
        if (live && j == 0) a.out[(g * a.Tm + t) * a.F + f] = make_float2(orx, oix);
        // the companions of the frame, fetched once its out is formed: lane j needs entry j of each alone; the same xor tree
#pragma unroll
        for (int q = 0; q < 2; ++q) {                      // (unrolled: cm's arrays are read with compile-time indices)
            if (q >= cm.n) break;                          // block-uniform
            c32 u = make_float2(0.f, 0.f);
            if (j < P) u = online_comp_row(a, cm.X[q] + (xb - a.X), cm.Z[q] ? cm.Z[q] + f : nullptr, j, t, k, r, TF);
            float crx = j < P ? wj.x * u.x + wj.y * u.y : 0.f;
            float cix = j < P ? wj.x * u.y - wj.y * u.x : 0.f;
#pragma unroll
            for (int off = G / 2; off >= 1; off >>= 1) {
                crx += __shfl_xor(crx, off, G);
                cix += __shfl_xor(cix, off, G);
            }
            if (live && j == 0) cm.out[q][(g * a.Tm + t) * a.F + f] = make_float2(crx, cix);
        }
    }
    if (col && a.w_last) a.w_last[pid * P + j] = wj;
}

// P <= 7: one thread per (room, node, bin), as k_online_mwf_thread; the companions re-use v[] once the frame's out is formed
template <int P, bool SQ32>
__global__ __launch_bounds__(solve_small_threads<P>()) void k_online_mwf_thread_ref(OnlineArgs a, OnlineComp cm) {
    constexpr int SOLVE_SMALL_THREADS = solve_small_threads<P>();
    constexpr int NO = P > 1 ? P * (P - 1) / 2 : 1;
    const long long pid = (long long)blockIdx.x * SOLVE_SMALL_THREADS + threadIdx.x;
    const bool live = pid < a.n_prob;
    const long long pc = live ? pid : 0;                  // dead threads walk problem 0 and write nothing
    const long long g = pc / a.F;
    const int f = (int)(pc % a.F);
    const long long r = g / a.Kl;
    const int k = a.k0 + (int)(g % a.Kl);
    const int M = a.M;
    const c32* xb = a.X + ((g * a.Tx + a.tx0) * a.F + f) * (long long)M;
    const c32* zb = a.Z ? a.Z + f : nullptr;
    const long long TF = (long long)a.Tm * a.F;
    const float* mp = a.mask + (g * a.Tm) * a.F + f;
    float a_d[P], b_d[P];
    c32 a_o[NO], b_o[NO];
#pragma unroll
    for (int i = 0; i < P; ++i) {
        a_d[i] = 0.f;
        b_d[i] = a.init_diag;
    }
#pragma unroll
    for (int q = 0; q < NO; ++q) a_o[q] = b_o[q] = make_float2(0.f, 0.f);
    const float lam = a.lambda_cor, oml = 1.f - a.lambda_cor;
    c32 wv[P];
#pragma unroll
    for (int i = 0; i < P; ++i) wv[i] = make_float2(0.f, 0.f);
    int until_update = 0;
    for (int t = 0; t < a.T; ++t) {
        c32 v[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            if (c < M) {
                v[c] = xb[(long long)t * a.F * M + c];
            } else {
                const int jn = (c - M) < k ? (c - M) : (c - M) + 1;        // skip the node's own z
                v[c] = zb ? zb[z_plane(r, jn, a.K, a.R, a.zblk) * TF + (long long)t * a.F] : make_float2(0.f, 0.f);
            }
        }
        const float m = mp[(long long)t * a.F];
        const float cs = oml * m, cn = oml * (1.f - m);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const float p2 = v[i].x * v[i].x + v[i].y * v[i].y;
            a_d[i] = lam * a_d[i] + cs * p2;
            b_d[i] = lam * b_d[i] + cn * p2;
#pragma unroll
            for (int c = 0; c < i; ++c) {
                const float pr = v[i].x * v[c].x + v[i].y * v[c].y;          // v_i conj(v_c)
                const float pi = v[i].y * v[c].x - v[i].x * v[c].y;
                const int q = i * (i - 1) / 2 + c;
                a_o[q] = make_float2(lam * a_o[q].x + cs * pr, lam * a_o[q].y + cs * pi);
                b_o[q] = make_float2(lam * b_o[q].x + cn * pr, lam * b_o[q].y + cn * pi);
            }
        }
        if (until_update == 0) {                           // uniform: every problem updates at the same frames
            c64 w[P], t1[P];
            gevd_solve_thread<P, SQ32>(a_d, a_o, b_d, b_o, a.mu, w, t1);
#pragma unroll
            for (int i = 0; i < P; ++i) wv[i] = make_float2((float)w[i].x, (float)w[i].y);
            until_update = a.update_every;
        }
        --until_update;
        float orx = 0.f, oix = 0.f;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            orx += wv[i].x * v[i].x + wv[i].y * v[i].y;
            oix += wv[i].x * v[i].y - wv[i].y * v[i].x;
        }
        if (live) a.out[(g * a.Tm + t) * a.F + f] = make_float2(orx, oix);
        // the companions of the frame through the filter in force, fetched once its out is formed: v[] is free again
#pragma unroll
        for (int q = 0; q < 2; ++q) {                      // (unrolled: cm's arrays are read with compile-time indices)
            if (q >= cm.n) break;
            const c32* cxb = cm.X[q] + (xb - a.X);
            const c32* czb = cm.Z[q] ? cm.Z[q] + f : nullptr;
#pragma unroll
            for (int c = 0; c < P; ++c) v[c] = online_comp_row(a, cxb, czb, c, t, k, r, TF);
            float crx = 0.f, cix = 0.f;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                crx += wv[i].x * v[i].x + wv[i].y * v[i].y;
                cix += wv[i].x * v[i].y - wv[i].y * v[i].x;
            }
            if (live) cm.out[q][(g * a.Tm + t) * a.F + f] = make_float2(crx, cix);
        }
    }
    if (live && a.w_last) {
#pragma unroll
        for (int i = 0; i < P; ++i) a.w_last[pid * P + i] = wv[i];
    }
}

}  // namespace disco
