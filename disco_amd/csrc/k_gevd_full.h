// Batched rank-R GEVD-MWF solve -- intern_filter(Rxx, Rnn, mu, type='gevd', rank=R), disco_theque/se_utils/internal_formulas.py:56-73,
// for Hermitian pencils of size P <= 16 and any kept rank r (0 <= r <= P; the caller maps the reference's slicing rule to r).
//
// The reference forms  Wint = (Q D (D + mu I)^-1 Q^-1)[:, 0]  with the eigenvalues clamped to [eps, 1e6], sorted descending and all but
// the first r set to 0, and t1 = Q[:, 0] (Q^-1)[0, 0].  With Rnn = L L^H and C = L^-1 Rxx L^-H = V diag(d) V^H one has Q = L^-H V and
// Q^-1 = V^H L^H, so both are invariant to how the eigenvectors are scaled:
//     w  = L00 L^-H sum_{i kept} f_i v_i conj(v_i[0]),   f_i = dc_i / (dc_i + mu),  dc_i = d_i clamped to [eps, 1e6]
//     t1 = L00 L^-H v_top conj(v_top[0])                 (the same as rank 1; does not depend on r)
// Kept set: d_i's position in the descending order is #{k : d_k > d_i, or d_k == d_i and k < i}; the pair is kept where that position is
// below r, and position 0 gives t1.  The order is that of the UNCLAMPED eigenvalues, ties broken by index (where several eigenvalues clamp
// to the same bound, or tie at the truncation boundary, the reference's order is LAPACK's accident and nothing is there to match).
//
// Unlike rank 1 (k_solve.h, k_solve_small.h: the top pair only, by repeated squaring) this needs every eigenpair of C: cyclic complex
// Jacobi in float64.  Whitening reuses the rank-1 Cholesky with its pivot floor, so a singular Rnn behaves exactly as at rank 1.
//   P <= 4  : one thread per pencil, C and V in registers, cyclic (p, q) order -- every index compile-time (k_gevd_full_thread).
//   P >= 5  : a group of G = 8 / 16 lanes per pencil (SolveGeom<P>), lane j owns COLUMN j of C and ROW j of V; parallel round-robin
//             ordering (N - 1 rounds of N / 2 disjoint pairs, N = P rounded up to even).  Per round: the columns go to LDS, the two lanes
//             of a pair compute the same rotation from the same LDS words, apply it to their columns (C J) and the lower one publishes
//             it; then every lane applies all rotations of the round to the rows of its column (J^H C J) and the columns of its row of V.
// Stop: off(C)^2 <= DISCO_JACOBI_TOL2 ||C||_F^2, tested before every sweep, at most DISCO_JACOBI_SWEEPS sweeps.  A pencil that is done
// (or not finite: the test is false for NaN / inf, so it counts as done) stops rotating -- its results do not depend on how long the rest
// of its wave runs -- and the wave leaves when all of its pencils are done.
#pragma once
#include "k_solve.h"
#include "k_solve_small.h"
#include "dpp64.h"                                   // static_for

namespace disco {

#ifndef DISCO_JACOBI_SWEEPS
#define DISCO_JACOBI_SWEEPS 12
#endif
#ifndef DISCO_JACOBI_TOL2
#define DISCO_JACOBI_TOL2 1e-26
#endif

// The Jacobi rotation J = diag(1, conj(e)) [[c, s], [-s, c]] that zeroes b = C[p][q] of the Hermitian 2 x 2 block [[app, b], [conj b, aqq]]:
// J^H [[app, b], [conj b, aqq]] J is diagonal.  e = b / |b|; t = tan(theta) in [-1, 1] from the stable form of tan(2 theta).
__device__ __forceinline__ void jacobi_rotation(double app, double aqq, c64 b, double& c, double& s, c64& e) {
    const double ab2 = b.x * b.x + b.y * b.y;
    if (ab2 > 1e-300) {
        const double rab = rsqrt64(ab2), ab = ab2 * rab;
        const double dd = aqq - app, r2 = fma(dd, dd, 4.0 * ab2);
        const double t = 2.0 * ab * rcp64(fabs(dd) + r2 * rsqrt64(r2));
        const double ts = dd < 0.0 ? -t : t;
        c = rsqrt64(fma(ts, ts, 1.0));
        s = ts * c;
        e = zscale(b, rab);
    } else {
        c = 1.0;
        s = 0.0;
        e = make_double2(1.0, 0.0);
    }
}

// (x, y) <- (c x - s e y, s x + c e y): rows p, q of J^H X;  with conj(e): columns p, q of X J
__device__ __forceinline__ void jacobi_apply(c64& x, c64& y, double c, double s, c64 e) {
    const c64 ey = zmul(e, y);
    const c64 nx = make_double2(fma(c, x.x, -s * ey.x), fma(c, x.y, -s * ey.y));
    const c64 ny = make_double2(fma(s, x.x, c * ey.x), fma(s, x.y, c * ey.y));
    x = nx;
    y = ny;
}

// f_i of a kept pair, 0 for a dropped one (pos: the pair's position in the descending order)
__device__ __forceinline__ double gevd_kept_gain(double d, int pos, int r, double mu) {
    return pos < r ? mwf_gain(d, mu) : 0.0;
}

// ---- P <= 4: one thread per pencil ---------------------------------------------------------------------------------------------------
template <int P>
__global__ DISCO_KERNEL_ALIGN __launch_bounds__(128) void k_gevd_full_thread(const c32* __restrict__ Rxx, const c32* __restrict__ Rnn,
                                                                         long long n_prob, int r, double mu, c32* __restrict__ w_out,
                                                                         c32* __restrict__ t1_out) {
    constexpr int NO = P > 1 ? P * (P - 1) / 2 : 1;
    auto lo = [](int i, int k) { return i * (i - 1) / 2 + k; };
    const long long pid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = pid < n_prob;
    const long long pc = live ? pid : n_prob - 1;                 // dead lanes stand in for the last pencil (and store nothing)
    const c32* A = Rxx + pc * P * P;
    const c32* B = Rnn + pc * P * P;
    double Ld[P], rL[P];
    c64 Lo[NO];
    thread_cholesky<P>([&](int i) { return (double)B[i * P + i].x; },
                       [&](int i, int k) { return make_double2((double)B[i * P + k].x, (double)B[i * P + k].y); }, Ld, rL, Lo);
    // C = L^-1 (L^-1 Rxx)^H from the lower triangle of Rxx (entry (i, k), i < k, is the conjugate of (k, i)), all of it kept
    c64 C[P][P], Y[P][P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const c32 a = i >= k ? A[i * P + k] : A[k * P + i];
            c64 x = make_double2((double)a.x, i >= k ? (double)a.y : -(double)a.y);
            if (i == k) x.y = 0.0;
#pragma unroll
            for (int m = 0; m < i; ++m) x = zfnma(x, Lo[lo(i, m)], Y[m][k]);
            Y[i][k] = zscale(x, rL[i]);
        }
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            c64 x = make_double2(Y[k][i].x, -Y[k][i].y);
#pragma unroll
            for (int m = 0; m < i; ++m) x = zfnma(x, Lo[lo(i, m)], C[m][k]);
            C[i][k] = zscale(x, rL[i]);
        }
    }
    c64 V[P][P];
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int k = 0; k < P; ++k) V[i][k] = make_double2(i == k ? 1.0 : 0.0, 0.0);

    bool done = P == 1;
#pragma unroll 1
    for (int sweep = 0; sweep < DISCO_JACOBI_SWEEPS; ++sweep) {
        double off = 0.0, fro = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i)
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const double a2 = fma(C[i][k].x, C[i][k].x, C[i][k].y * C[i][k].y);
                fro += a2;
                if (i != k) off += a2;
            }
        done = done || !(off > DISCO_JACOBI_TOL2 * fro);          // NaN / inf / zero: done
        if (!__any(!done)) break;
        if (!done) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
#pragma unroll
                for (int q = p + 1; q < P; ++q) {
                    double c, s;
                    c64 e;
                    jacobi_rotation(C[p][p].x, C[q][q].x, C[p][q], c, s, e);
                    const c64 ce = make_double2(e.x, -e.y);
#pragma unroll
                    for (int i = 0; i < P; ++i) jacobi_apply(C[i][p], C[i][q], c, s, ce);     // C J
#pragma unroll
                    for (int k = 0; k < P; ++k) jacobi_apply(C[p][k], C[q][k], c, s, e);      // J^H (C J)
#pragma unroll
                    for (int i = 0; i < P; ++i) jacobi_apply(V[i][p], V[i][q], c, s, ce);     // V J
                    C[p][q] = C[q][p] = make_double2(0.0, 0.0);
                    C[p][p].y = C[q][q].y = 0.0;
                }
            }
        }
    }
    // ---- kept set by counting, u = sum_kept f_i conj(V[0][i]) v_i, u1 = conj(V[0][top]) v_top, then q = L^-H u
    c64 u[P], u1[P];
#pragma unroll
    for (int i = 0; i < P; ++i) u[i] = u1[i] = make_double2(0.0, 0.0);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        int pos = 0;
#pragma unroll
        for (int k = 0; k < P; ++k) pos += (C[k][k].x > C[i][i].x || (C[k][k].x == C[i][i].x && k < i)) ? 1 : 0;
        const double f = gevd_kept_gain(C[i][i].x, pos, r, mu);
        const c64 v0c = make_double2(V[0][i].x, -V[0][i].y);
        const c64 gf = zscale(v0c, f), g1 = pos == 0 ? v0c : make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < P; ++k) {
            u[k] = zfma(u[k], gf, V[k][i]);
            u1[k] = zfma(u1[k], g1, V[k][i]);
        }
    }
    c64 q[P], q1[P];
#pragma unroll
    for (int i = P - 1; i >= 0; --i) {
        c64 a = u[i], a1 = u1[i];
#pragma unroll
        for (int k = i + 1; k < P; ++k) {
            a = zfnmca(a, Lo[lo(k, i)], q[k]);
            a1 = zfnmca(a1, Lo[lo(k, i)], q1[k]);
        }
        q[i] = zscale(a, rL[i]);
        q1[i] = zscale(a1, rL[i]);
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            w_out[pid * P + i] = make_float2((float)(Ld[0] * q[i].x), (float)(Ld[0] * q[i].y));
            if (t1_out) t1_out[pid * P + i] = make_float2((float)(Ld[0] * q1[i].x), (float)(Ld[0] * q1[i].y));
        }
    }
}

// ---- 5 <= P <= 16: a group of G lanes per pencil -------------------------------------------------------------------------------------
// round-robin (circle method) partner of player i in round rd of N players (N even): N - 1 rounds, every pair exactly once
__host__ __device__ constexpr int rr_partner(int i, int rd, int N) {
    if (i == N - 1) return rd;
    const int k = ((2 * rd - i) % (N - 1) + (N - 1)) % (N - 1);
    return k == i ? N - 1 : k;
}

template <int P>
__global__ DISCO_KERNEL_ALIGN __launch_bounds__(SolveGeom<P>::THREADS, SolveGeom<P>::WPE) void k_gevd_full_group(
    const c32* __restrict__ Rxx, const c32* __restrict__ Rnn, long long n_prob, int r, double mu, c32* __restrict__ w_out,
    c32* __restrict__ t1_out) {
    static_assert(P >= 5, "P <= 4 runs one thread per pencil");
    using SG = SolveGeom<P>;
    constexpr int G = SG::G, PROBS = SG::PROBS, YW = SG::YW;
    constexpr int N = (P + 1) & ~1;
    __shared__ c64 s_L[PROBS][SG::LSZ];
    __shared__ c64 s_Y[PROBS][P * YW];
    __shared__ c64 s_rot[PROBS][N][2];                // the rotation of the pair whose lower index is the slot: (c, s), e
    const int j = threadIdx.x % G, slot = threadIdx.x / G;
    const long long pid = (long long)blockIdx.x * PROBS + slot;
    const bool col = pid < n_prob && j < P;
    c64* Lm = s_L[slot];
    c64(*Ym)[YW] = reinterpret_cast<c64(*)[YW]>(s_Y[slot]);
    c64(*Rot)[2] = s_rot[slot];

    c32 rowA[P], rowB[P];
    const SolveSrc src = SolveSrc::matrices(Rxx, Rnn);
    if (col) {
        solve_load_row<P, false>(src, pid, j, rowA, rowB);
    } else {
#pragma unroll
        for (int c = 0; c < P; ++c) {
            rowA[c] = make_float2(0.f, 0.f);
            rowB[c] = make_float2(c == j ? 1.f : 0.f, 0.f);
        }
    }
    group_cholesky<P>(rowB, Lm, j);
    // column j of Y = L^-1 Rxx (Rxx[i][j] = conj(Rxx[j][i])), then column j of C = L^-1 Y^H
    c64 g[P];
#pragma unroll
    for (int i = 0; i < P; ++i) g[i] = make_double2((double)rowA[i].x, -(double)rowA[i].y);
    group_forward_substitute<P>(g, Lm);
#pragma unroll
    for (int i = 0; i < P; ++i) {
        // g is only stored under `j < P` below: without a use here hipcc sinks the substitution into that branch while its LDS loads
        // stay outside, i.e. all of L is loaded (and spilled) first
        DISCO_CONSUME(g[i].x);
        DISCO_CONSUME(g[i].y);
    }
    if (j < P) {
#pragma unroll
        for (int i = 0; i < P; ++i) Ym[i][j] = g[i];
    }
    DISCO_GROUP_SYNC();
#pragma unroll
    for (int i = 0; i < P; ++i) g[i] = j < P ? make_double2(Ym[j][i].x, -Ym[j][i].y) : make_double2(0.0, 0.0);
    group_forward_substitute<P>(g, Lm);
    c64 vr[P];                                        // row j of V
#pragma unroll
    for (int i = 0; i < P; ++i) vr[i] = make_double2(i == j ? 1.0 : 0.0, 0.0);

    bool done = false;
    DISCO_GROUP_SYNC();                               // the reads of Y are done before the rounds write their columns
#pragma unroll 1
    for (int sweep = 0; sweep < DISCO_JACOBI_SWEEPS; ++sweep) {
        double off = 0.0, fro = 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const double a2 = fma(g[i].x, g[i].x, g[i].y * g[i].y);
            fro += a2;
            off += i == j ? 0.0 : a2;
        }
#pragma unroll
        for (int o = G / 2; o >= 1; o >>= 1) {        // (a butterfly: every lane of the group ends with the same sums)
            off += __shfl_xor(off, o, G);
            fro += __shfl_xor(fro, o, G);
        }
        done = done || !(off > DISCO_JACOBI_TOL2 * fro);          // NaN / inf / zero: done
        if (!__any(!done)) break;
        static_for<0, N - 1>([&](auto RD) {          // the rounds, so that every row index below is a compile-time constant
            constexpr int rd = decltype(RD)::value;
            // the partner and its addresses are the same in every sweep: formed here, from an opaque copy of j, so that hipcc does not
            // hoist those of all N - 1 rounds out of the sweep loop and keep them live through it (scratch from P = 11 on)
            int jr = j;
            DISCO_CONSUME(jr);
            const int pj = jr < N ? rr_partner(jr, rd, N) : jr;
            const bool pair = j < P && pj < P;
            const int lo_ = j < pj ? j : pj, hi_ = j < pj ? pj : j;
            if (j < P) {
#pragma unroll
                for (int i = 0; i < P; ++i) Ym[i][j] = g[i];
            }
            DISCO_GROUP_SYNC();
            if (pair && !done) {
                // both lanes of the pair compute the same rotation from the same words
                double c, s;
                c64 e;
                jacobi_rotation(Ym[lo_][lo_].x, Ym[hi_][hi_].x, Ym[lo_][hi_], c, s, e);
                if (j == lo_) {
                    Rot[lo_][0] = make_double2(c, s);
                    Rot[lo_][1] = e;
                }
                const c64 ce = make_double2(e.x, -e.y);
#pragma unroll
                for (int i = 0; i < P; ++i) {         // C J: this lane's column and its partner's
                    // a row at a time: without the fences hipcc hoists every LDS load of the round above the first multiply (scratch)
                    DISCO_SCHED_FENCE();
                    c64 x = g[i], y = Ym[i][pj];
                    if (j == lo_) jacobi_apply(x, y, c, s, ce);
                    else jacobi_apply(y, x, c, s, ce);
                    g[i] = x;
                }
            }
            DISCO_GROUP_SYNC();                       // Rot is written; every read of Ym of this round is done
            if (!done) {
                // J^H (C J) on the rows of this lane's column and V J on its row of V, for every pair of the round
                static_for<0, P>([&](auto PP) {
                    constexpr int p = decltype(PP)::value, qq = rr_partner(p, rd, N);
                    if constexpr (qq > p && qq < P) {
                        DISCO_SCHED_FENCE();
                        const c64 cs = Rot[p][0], e = Rot[p][1];
                        jacobi_apply(g[p], g[qq], cs.x, cs.y, e);
                        jacobi_apply(vr[p], vr[qq], cs.x, cs.y, make_double2(e.x, -e.y));
                    }
                });
                if (pair) {                            // the annihilated entry, and a real diagonal
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        if (i == pj) g[i] = make_double2(0.0, 0.0);
                        if (i == j) g[i].y = 0.0;
                    }
                }
            }
        });
    }
    // ---- eigenvalue d_j of lane j; kept set by counting; u_j = sum_kept f_i conj(V[0][i]) V[j][i]; u1_j the same for the top pair only
    double dj = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i)
        if (i == j) dj = g[i].x;
    int pos = 0;                                      // this lane's pair's position in the descending order
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const double dk = __shfl(dj, k, G);
        pos += (dk > dj || (dk == dj && k < j)) ? 1 : 0;
    }
    const double fj = gevd_kept_gain(dj, pos, r, mu), topj = pos == 0 ? 1.0 : 0.0;
    c64 uj = make_double2(0.0, 0.0), u1j = make_double2(0.0, 0.0);
#pragma unroll
    for (int i = 0; i < P; ++i) {                     // pair i's f_i and flag from lane i, V[0][i] from lane 0
        const double f = __shfl(fj, i, G), top = __shfl(topj, i, G);
        const c64 v0c = make_double2(__shfl(vr[i].x, 0, G), -__shfl(vr[i].y, 0, G));
        uj = zfma(uj, zscale(v0c, f), vr[i]);
        u1j = zfma(u1j, zscale(v0c, top), vr[i]);
    }
    DISCO_GROUP_SYNC();
    if (j < P) {
        Ym[0][j] = uj;
        Ym[1][j] = u1j;
    }
    DISCO_GROUP_SYNC();
    const double l00 = Lm[SG::lt(0, 0)].y;
    // q = L^-H u for both vectors, one after the other (every lane forms all of q and keeps its own entry)
    auto back = [&](int row) {
        c64 u[P], q[P];
#pragma unroll
        for (int i = 0; i < P; ++i) u[i] = Ym[row][i];
        group_back_substitute<P>(u, Lm, q);
        c64 out = make_double2(0.0, 0.0);
#pragma unroll
        for (int i = 0; i < P; ++i)
            if (i == j) out = zscale(q[i], l00);
        DISCO_CONSUME(out.x);
        DISCO_CONSUME(out.y);
        return out;
    };
    const c64 wj = back(0);
    const c64 tj = back(1);
    if (col) {
        w_out[pid * P + j] = make_float2((float)wj.x, (float)wj.y);
        if (t1_out) t1_out[pid * P + j] = make_float2((float)tj.x, (float)tj.y);
    }
}

}  // namespace disco
