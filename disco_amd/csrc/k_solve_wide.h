// Rank-1 GEVD-MWF solve for 17 <= P <= 32 (networks whose step-2 pencil P = M + K - 1 exceeds 16 channels).
//
// The algorithm is the one described at the top of k_solve.h, step for step, with the rules stated there (DISCO_TRACE_OK ... mwf_gain).
//
// Mapping: ONE WAVE PER PENCIL, the matrices in LDS.  A 32 x 32 complex float64 matrix is 16 KiB: a 32-lane group owning one column
// per lane (the P <= 16 form) would need 2 x 32 complex doubles of column per lane in the squaring alone (256 VGPRs) and spill.  Here
// lane (c, h) = (lane % 32, lane / 32) owns the upper (h = 0) or lower (h = 1) 16 rows of column c of the matrix being squared:
// 16 + 16 complex doubles (the column and its square) = 128 VGPRs.  One product B^2[i][c] = sum_k B[i][k] B[k][c] reads B[k][c] once
// (32 consecutive entries per half-wave) and B[i][k] for the lane's 16 rows (the same address in all 32 lanes of a half: a broadcast).
// The run-time P (17..32) only guards loops: one code object serves every size.
// LDS per pencil: Rxx as float32 [32][33] 8.25 KiB, the packed factor 8.25 KiB, the float64 work matrix [32][33] 16.5 KiB, one vector:
// 33.5 KiB -> 4 pencils (4 waves) per CU.  No pencil shares a wave, so a non-finite or flagged pencil affects nothing but itself.
#pragma once
#include "common.h"
#include "k_solve.h"

namespace disco {

constexpr int SW_PMIN = 17, SW_PMAX = 32;
constexpr int SW_YW = SW_PMAX + 1;               // row pitch: 33 x 16 B, so that a column read walks the banks
__host__ __device__ constexpr int sw_lt(int i, int k) { return i * (i + 1) / 2 + k; }

struct SolveWideLds {
    c32 A[SW_PMAX][SW_YW];                       // Rxx as the solvers receive it (float32)
    c64 L[SW_PMAX * (SW_PMAX + 1) / 2 + 1];      // Rnn's lower triangle -> the factor; diagonal slots -> (1 / L[c][c], L[c][c])
    c64 Y[SW_PMAX][SW_YW];                       // Y = L^-1 Rxx, then C (transposed), then the squares
    c64 V[SW_PMAX];                              // the eigenvector / q
};

// both matrices of pencil pid into LDS.  Partial sums: the chunks are combined in float64 and rounded ONCE to float32, exactly as
// solve_load_row does (the lower triangle is the conjugate of the upper one, the diagonal is real).
template <bool FROM_PART>
__device__ __forceinline__ void wide_load(const SolveSrc& src, long long pid, int P, int lane, SolveWideLds& s) {
    if constexpr (!FROM_PART) {
        const c32* rs = src.Rss + pid * P * P;
        const c32* rn = src.Rnn + pid * P * P;
        for (int e = lane; e < P * P; e += 64) {
            const int j = e / P, c = e - j * P;
            s.A[j][c] = rs[e];
            if (c <= j) {
                const c32 b = rn[e];
                s.L[sw_lt(j, c)] = make_double2((double)b.x, (double)b.y);
            }
        }
    } else {
        const int NP = P * (P + 1) / 2;
        const long long g = pid / src.F;
        const int f = (int)(pid % src.F);
        const float4* pb = src.part + ((g * src.chunks) * src.F + f) * (long long)NP;
        const long long cs = (long long)src.F * NP;
        const double it = (double)src.inv_T;
        for (int q = lane; q < NP; q += 64) {
            int i = 0, r = q;
            while (r >= P - i) {
                r -= P - i;
                ++i;
            }
            const int c = i + r;                 // upper-triangle entry (i, c), c >= i
            double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
            for (int ch = 0; ch < src.chunks; ++ch) {
                const float4 v = pb[ch * cs + q];
                sx += (double)v.x;
                sy += (double)v.y;
                sz += (double)v.z;
                sw += (double)v.w;
            }
            const float ax = (float)(sx * it), ay = c == i ? 0.f : (float)(sy * it), ayl = c == i ? 0.f : (float)(sy * -it);
            const float bx = (float)(sz * it), byl = c == i ? 0.f : (float)(sw * -it);
            s.A[i][c] = make_float2(ax, ay);
            s.A[c][i] = make_float2(ax, ayl);
            s.L[sw_lt(c, i)] = make_double2((double)bx, (double)byl);
        }
    }
}

// Cholesky factor of the lower triangle in s.L (group_cholesky_factor with the rows over the lanes of half 0)
__device__ __forceinline__ void wide_cholesky(SolveWideLds& s, int P, int lane) {
    const int j = lane & 31, h = lane >> 5;
    double rd_prev = 0.0, d_prev = 0.0;
    for (int c = 0; c < P; ++c) {
        if (c > 0 && lane == 0) s.L[sw_lt(c - 1, c - 1)] = make_double2(rd_prev, d_prev);
        const double a_cc = s.L[sw_lt(c, c)].x;
        double d2 = a_cc;
        for (int k = 0; k < c; ++k) {
            const c64 l = s.L[sw_lt(c, k)];
            d2 -= l.x * l.x + l.y * l.y;
        }
        const double fl = fmax(1e-7 * a_cc, 1e-30);
        const bool brk = !(d2 >= fl);            // also true for NaN
        const double d2c = brk ? fl : d2;
        const double rd = rsqrt64(d2c);
        rd_prev = rd;
        d_prev = d2c * rd;
        if (h == 0 && j > c && j < P) {
            c64 a = s.L[sw_lt(j, c)];
            for (int k = 0; k < c; ++k) a = zsub(a, zmulc(s.L[sw_lt(j, k)], s.L[sw_lt(c, k)]));
            s.L[sw_lt(j, c)] = brk ? make_double2(0.0, 0.0) : zscale(a, rd);
        }
        DISCO_GROUP_SYNC();
    }
    if (lane == 0) s.L[sw_lt(P - 1, P - 1)] = make_double2(rd_prev, d_prev);
    DISCO_GROUP_SYNC();
}

// C = L^-1 Rxx L^-H, left TRANSPOSED in s.Y (s.Y[j][i] = C[i][j]): lane j (half 0) forms column j of Y = L^-1 Rxx into s.Y[.][j], then
// column j of C from row j of Y, in place in row j (a lane only ever touches its own row in the second pass)
__device__ __forceinline__ void wide_whiten(SolveWideLds& s, int P, int lane) {
    const int j = lane & 31, h = lane >> 5;
    DISCO_GROUP_SYNC();                          // a previous pass's readers of Y are done
    if (h == 0 && j < P) {
        for (int i = 0; i < P; ++i) {
            const c32 ra = s.A[j][i];
            c64 a = make_double2((double)ra.x, -(double)ra.y);
            for (int k = 0; k < i; ++k) a = zsub(a, zmul(s.L[sw_lt(i, k)], s.Y[k][j]));
            s.Y[i][j] = zscale(a, s.L[sw_lt(i, i)].x);
        }
    }
    DISCO_GROUP_SYNC();
    if (h == 0 && j < P) {
        for (int i = 0; i < P; ++i) {
            const c64 yv = s.Y[j][i];
            c64 a = make_double2(yv.x, -yv.y);
            for (int k = 0; k < i; ++k) a = zsub(a, zmul(s.L[sw_lt(i, k)], s.Y[j][k]));
            s.Y[j][i] = zscale(a, s.L[sw_lt(i, i)].x);
        }
    }
    DISCO_GROUP_SYNC();
}

// Everything after the factor (gevd_pass_group): top eigenpair of C (in s.Y, transposed) by squaring, back substitution, t1 / gain.
// Returns `suspect`: trace <= 0, a first-check stop with tr(B^2) < DISCO_KEPT_TAU_MIN, or a negative Rayleigh quotient.
__device__ __forceinline__ bool wide_pass(SolveWideLds& s, int P, int lane, double mu, bool shift, c64& t1_j, double& gain_out) {
    const int j = lane & 31, h = lane >> 5, r0 = 16 * h;
    c64 g[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) g[r] = (j < P && r0 + r < P) ? s.Y[j][r0 + r] : make_double2(0.0, 0.0);
    double fro = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) fro = fma(g[r].x, g[r].x, fma(g[r].y, g[r].y, fro));
    fro = group_sum<64>(fro);
    const bool own_diag = j < P && j >= r0 && j < r0 + 16;
    if (shift) {
        const double sh = sqrt(fro);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (own_diag && r0 + r == j) g[r].x += sh;
    }
    bool done, tr_bad, exit0 = false;
    {
        double trl = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (own_diag && r0 + r == j) trl = g[r].x;
        trl = group_sum<64>(trl);
        const bool ok = DISCO_TRACE_OK(trl);
        const double rt = ok ? rcp64(trl) : 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = ok ? zscale(g[r], rt) : make_double2(0.0, 0.0);
        done = !ok;
        tr_bad = DISCO_TRACE_BAD(trl, fro);
    }
    for (int it = 0; it < DISCO_SQUARINGS_MAX; ++it) {
        DISCO_GROUP_SYNC();                      // every lane has read the previous content of Y
#pragma unroll
        for (int r = 0; r < 16; ++r) s.Y[r0 + r][j] = g[r];
        DISCO_GROUP_SYNC();
        c64 nn[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) nn[r] = make_double2(0.0, 0.0);
        for (int k = 0; k < P; ++k) {
            DISCO_SCHED_FENCE();
            const c64 b = s.Y[k][j];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const c64 a = s.Y[r0 + r][k];
                nn[r].x = fma(a.x, b.x, fma(-a.y, b.y, nn[r].x));
                nn[r].y = fma(a.x, b.y, fma(a.y, b.x, nn[r].y));
            }
        }
        c64 tc = make_double2(0.0, 0.0);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (own_diag && r0 + r == j) tc = nn[r];
        tc.x = group_sum<64>(tc.x);
        tc.y = group_sum<64>(tc.y);
        const double den = tc.x * tc.x + tc.y * tc.y;
        const double rden = den > 0.0 ? rcp64(den) : 0.0;
        const c64 itau = make_double2(tc.x * rden, -tc.y * rden);
        if (!done) {
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = zmul(nn[r], itau);
        }
        DISCO_SQUARING_AFTER(it, tc.x, den > 0.0, done, exit0);
        if (done) break;                         // wave-uniform: one pencil per wave
    }
    // ---- B = v0 v0^H: the longest column (ties: lowest index)
    double nrm = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) nrm += g[r].x * g[r].x + g[r].y * g[r].y;
    nrm += __shfl_xor(nrm, 32);
    double best = nrm;
    int bj = j;
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int oj = __shfl_xor(bj, off);
        if (ob > best || (ob == best && oj < bj)) {
            best = ob;
            bj = oj;
        }
    }
    double kept = nrm;
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) kept += __shfl_xor(kept, off);
    const bool suspect = DISCO_SUSPECT(P, tr_bad, exit0, kept);
    const bool have = best > 0.0;
    const double rb = have ? rsqrt64(best) : 0.0;
    DISCO_GROUP_SYNC();
    if (have) {
        if (j == bj) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s.V[r0 + r] = zscale(g[r], rb);
        }
    } else if (lane < SW_PMAX) {
        s.V[lane] = make_double2(lane == 0 ? 1.0 : 0.0, 0.0);
    }
    DISCO_GROUP_SYNC();
    // ---- power steps on the kept square: (B v)[c] = sum_i conj(B[i][c]) v[i]
    for (int st = 0; st < DISCO_POWER_STEPS; ++st) {
        c64 u = make_double2(0.0, 0.0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const c64 v = s.V[r0 + r];
            u.x = fma(g[r].x, v.x, fma(g[r].y, v.y, u.x));
            u.y = fma(g[r].x, v.y, fma(-g[r].y, v.x, u.y));
        }
        u.x += __shfl_xor(u.x, 32);
        u.y += __shfl_xor(u.y, 32);
        DISCO_GROUP_SYNC();
        if (have && h == 0) s.V[j] = u;
        DISCO_GROUP_SYNC();
    }
    c64 vj = j < P ? s.V[j] : make_double2(0.0, 0.0);           // this lane's component of v0
    if (DISCO_POWER_STEPS > 0 && have) {
        double n2 = vj.x * vj.x + vj.y * vj.y;
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) n2 += __shfl_xor(n2, off);
        vj = zscale(vj, rsqrt64(n2));
    }
    const c64 v00 = make_double2(__shfl(vj.x, 0), __shfl(vj.y, 0));
    // ---- q = L^-H v0, one component per step: q_i = r_i / L[i][i], then r_j -= conj(L[i][j]) q_i for j < i
    c64 rj = vj, qj = make_double2(0.0, 0.0);
    for (int i = P - 1; i >= 0; --i) {
        const c64 qi = zscale(make_double2(__shfl(rj.x, i), __shfl(rj.y, i)), s.L[sw_lt(i, i)].x);
        if (j == i) qj = qi;
        if (j < i) {
            const c64 l = s.L[sw_lt(i, j)];
            rj = zsub(rj, zmul(make_double2(l.x, -l.y), qi));
        }
    }
    DISCO_GROUP_SYNC();
    if (h == 0 && j < P) s.V[j] = qj;
    DISCO_GROUP_SYNC();
    // ---- d0 = q^H Rxx q: lane j forms (Rxx q)_j from row j of Rxx
    double e = 0.0;
    if (h == 0 && j < P) {
        c64 sj = make_double2(0.0, 0.0);
        for (int c = 0; c < P; ++c) {
            const c32 a = s.A[j][c];
            const c64 q = s.V[c];
            sj.x = fma((double)a.x, q.x, fma(-(double)a.y, q.y, sj.x));
            sj.y = fma((double)a.x, q.y, fma((double)a.y, q.x, sj.y));
        }
        e = qj.x * sj.x + qj.y * sj.y;
    }
    e = group_sum<64>(e);
    const double d0 = have ? e : 0.0;
    const double dcl = clamp_eigenvalue(d0);
    const double l00 = s.L[sw_lt(0, 0)].y;
    const c64 gsc = make_double2(l00 * v00.x, -l00 * v00.y);     // L[0,0] conj(v0[0]) = (Q^-1)[0,0]
    gain_out = dcl / (dcl + mu);                                 // mwf_gain, around the read of L: the listing follows the statement order
    t1_j = zmul(qj, gsc);
    return suspect || d0 < 0.0;
}

// grid = n_prob workgroups of one wave
template <bool FROM_PART>
__global__ __launch_bounds__(64) void k_gevd_mwf_r1_wide(SolveSrc src, long long n_prob, int P, double mu, c32* __restrict__ w_out,
                                                         c32* __restrict__ t1_out) {
    __shared__ SolveWideLds s;
    const long long pid = blockIdx.x;
    if (pid >= n_prob) return;                   // (whole workgroup)
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    wide_load<FROM_PART>(src, pid, P, lane, s);
    DISCO_GROUP_SYNC();
    wide_cholesky(s, P, lane);
    wide_whiten(s, P, lane);
    c64 t1;
    double gain;
    if (wide_pass(s, P, lane, mu, false, t1, gain)) {
        wide_whiten(s, P, lane);                 // the squarings overwrote C: formed again from the factor and Rxx
        (void)wide_pass(s, P, lane, mu, true, t1, gain);
    }
    if (h == 0 && j < P) {
        if (t1_out) t1_out[pid * P + j] = make_float2((float)t1.x, (float)t1.y);
        w_out[pid * P + j] = make_float2((float)(t1.x * gain), (float)(t1.y * gain));
    }
}

}  // namespace disco
