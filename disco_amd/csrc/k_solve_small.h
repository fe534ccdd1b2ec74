// Rank-1 GEVD-MWF for SMALL pencils (P <= 4: every step-1 solve of a node with up to 4 microphones), one THREAD per
// problem.  The algorithm, its float64 arithmetic and its rules are those of k_solve.h (described at its top) -- but at this size a
// group of 4 lanes spends more
// instructions on hand-offs (LDS round trips, fences, shuffle reductions) than on arithmetic, so everything lives in the
// registers of one thread: no LDS or shuffles in the arithmetic (only the wave-cooperative fetch of the partial sums goes
// through LDS), 64 problems per wave instead of 16.  The Hermitian matrices are held as (real diagonal, strict lower
// triangle); B^2 is formed on that half only, which also keeps B exactly Hermitian.
#pragma once
#include "k_solve.h"

namespace disco {

template <int P>
struct HermReg {                       // Hermitian P x P: d[i] = A[i][i] (real), o[i(i-1)/2 + k] = A[i][k], i > k
    double d[P];
    c64 o[P > 1 ? P * (P - 1) / 2 : 1];
    __device__ __forceinline__ c64 at(int i, int k) const {       // i, k compile-time after unrolling
        if (i == k) return make_double2(d[i], 0.0);
        if (i > k) return o[i * (i - 1) / 2 + k];
        const c64 v = o[k * (k - 1) / 2 + i];
        return make_double2(v.x, -v.y);
    }
};

// ---- the squarings in packed float32 (round 4) ------------------------------------------------------------------------------------
// The eigenvector that the squarings find is only as good as the pencil: Rxx / Rnn arrive ROUNDED TO FLOAT32 (6e-8 relative), which moves
// the whitened matrix by 6e-8 cond(Rnn) and its dominant eigenvector by that over the relative gap.  A float32 rounding inside squaring j
// moves the vector by 6e-8 / (2^j gap) -- the gap doubles with every squaring --: summed over the squarings, twice the rounding of a
// matrix that is better conditioned than the input by cond(Rnn).  So the squarings (two thirds of the solve's instructions: P^3 / 2
// complex multiply-adds each, as many as the wave's slowest pencil needs) run on v_pk_fma_f32 -- one complex multiply-add = 2 instructions
// instead of 4 float64 ones -- and everything that touches the ill-conditioned factor (Cholesky, whitening, back substitution, the
// Rayleigh quotient) stays float64.
// WHERE: the online mode (template parameter SQ32 of the solve; option "online_sq32"), which re-solves every (bin, frame) and spends
// 3/4 of its time squaring: 185 -> 143 ms per C3-shaped step, parity 2.0e-6 either way.  On random pencils the added error measured half
// of what the complex64 rounding of the inputs costs, at every gap (tests: check_solver_small_gap's `inherent`).  The offline solves keep
// float64 squarings: they are 4 % of a C3 step, and on C5's ill-conditioned 8-microphone statistics (cond(Rnn) 1e4..1e5) the float32
// squarings moved room 199 between 3.0e-5 and 7.5e-5 with the order of the additions -- too close to the 1e-4 bar for 0.06 ms.
template <int P>
struct HermPk {                        // Hermitian P x P in float32: o as HermReg, the real diagonal two to a register pair (d[2m], d[2m+1])
    static constexpr int NO = P > 1 ? P * (P - 1) / 2 : 1, ND = (P + 1) / 2;
    c32 o[NO];
    c32 dp[ND];
};
// S = B B on the stored half; returns tr S.  Term k of S[i][j] (i > j) is B[i][k] B[k][j] with the upper triangle read as the conjugate of
// the stored entry: a conjugating multiply-add (k < j, k > i), a plain one (j < k < i), a real scaling (k = j, k = i).
// Order of the instructions: a complex multiply-add is two DEPENDENT v_pk_fma_f32 and the kernel runs one or two waves per SIMD, so the
// sums advance together -- for every k the first halves of all P (P - 1) / 2 sums, then their second halves -- instead of one sum after
// the other (the compiler schedules inline asm in source order: back-to-back dependent instructions made the first version of this
// slower than float64 wherever few squarings were needed: C5's step-1 solves 0.71 -> 0.98 ms).
template <int P>
__device__ __forceinline__ float herm_square_pk(const HermPk<P>& B, HermPk<P>& S) {
    constexpr int NO = HermPk<P>::NO;
    auto lo = [](int i, int k) { return i * (i - 1) / 2 + k; };
    // |off-diagonal|^2 into the row's and the column's sum (two squares per sum kept apart until the end), walked along the diagonals
    // i - j = d so that neighbouring instructions touch different sums
    c32 accr[P], accc[P];
#pragma unroll
    for (int j = 0; j < P; ++j) accr[j] = accc[j] = make_float2(0.f, 0.f);
#pragma unroll
    for (int d = 1; d < P; ++d) {
#pragma unroll
        for (int j = 0; j + d < P; ++j) accr[j + d] = PkD::fma_comp(B.o[lo(j + d, j)], B.o[lo(j + d, j)], accr[j + d]);
#pragma unroll
        for (int j = 0; j + d < P; ++j) accc[j] = PkD::fma_comp(B.o[lo(j + d, j)], B.o[lo(j + d, j)], accc[j]);
    }
    // k = j and k = i: the real diagonal
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int i = j + 1; i < P; ++i)
            S.o[lo(i, j)] = (j & 1) ? scale_by_half<1>(B.o[lo(i, j)], B.dp[j / 2]) : scale_by_half<0>(B.o[lo(i, j)], B.dp[j / 2]);
#pragma unroll
    for (int j = 0; j < P; ++j)
#pragma unroll
        for (int i = j + 1; i < P; ++i)
            S.o[lo(i, j)] = (i & 1) ? fma_by_half<1>(B.o[lo(i, j)], B.dp[i / 2], S.o[lo(i, j)]) : fma_by_half<0>(B.o[lo(i, j)], B.dp[i / 2], S.o[lo(i, j)]);
#pragma unroll
    for (int k = 0; k < P; ++k) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int j = 0; j < P; ++j) {
#pragma unroll
                for (int i = j + 1; i < P; ++i) {
                    if (k == i || k == j) continue;
                    // (u, v): the two stored entries; conj: u enters conjugated
                    const bool cj = k < j || k > i;
                    const c32 u = k < j ? B.o[lo(j, k)] : (k < i ? B.o[lo(i, k)] : B.o[lo(k, i)]);
                    const c32 v = k < j ? B.o[lo(i, k)] : B.o[lo(k, j)];
                    c32& a = S.o[lo(i, j)];
                    if (half == 0) a = PkD::cfma_lo(u, v, a);
                    else if (cj) a = PkD::cfma_hi_conj(u, v, a);
                    else a = PkD::cfma_hi(u, v, a);
                }
            }
        }
    }
    float tau = 0.f;
#pragma unroll
    for (int m = 0; m < HermPk<P>::ND; ++m) {
        c32 d2 = PkD::mul_comp(B.dp[m], B.dp[m]);
        d2.x += (accr[2 * m].x + accr[2 * m].y) + (accc[2 * m].x + accc[2 * m].y);
        if (2 * m + 1 < P) d2.y += (accr[2 * m + 1].x + accr[2 * m + 1].y) + (accc[2 * m + 1].x + accc[2 * m + 1].y);
        S.dp[m] = d2;
        tau += d2.x + (2 * m + 1 < P ? d2.y : 0.f);
    }
    (void)NO;
    return tau;
}

// Cholesky Rnn = L L^H with the pivot floor of k_solve.h (numerically singular noise statistics): Ld = diag L, rL = 1 / diag L,
// Lo = strict lower triangle.  bd(i) / bo(i, k) (i > k) hand out Rnn's entries -- from registers, an LDS tile or memory.
template <int P, class BD, class BO>
__device__ __forceinline__ void thread_cholesky(BD bd, BO bo, double* Ld, double* rL, c64* Lo) {
    auto lo = [](int i, int k) { return i * (i - 1) / 2 + k; };
#pragma unroll
    for (int c = 0; c < P; ++c) {
        const double a_cc = bd(c);
        double d2 = a_cc;
#pragma unroll
        for (int k = 0; k < c; ++k) d2 = fma(-Lo[lo(c, k)].y, Lo[lo(c, k)].y, fma(-Lo[lo(c, k)].x, Lo[lo(c, k)].x, d2));
        const double fl = fmax(1e-7 * a_cc, 1e-30);
        const bool brk = !(d2 >= fl);
        const double d2c = brk ? fl : d2;
        const double rd = rsqrt64(d2c);
        rL[c] = rd;
        Ld[c] = d2c * rd;
#pragma unroll
        for (int i = c + 1; i < P; ++i) {
            c64 s = bo(i, c);
#pragma unroll
            for (int k = 0; k < c; ++k) s = zfnmac(s, Lo[lo(i, k)], Lo[lo(c, k)]);
            Lo[lo(i, c)] = brk ? make_double2(0.0, 0.0) : zscale(s, rd);
        }
    }
}

// Rank-1 GEVD-MWF of ONE pencil in the registers of one thread.  load_a / load_b(float* d, c32* o) fill (diagonal, strict lower triangle)
// of Rxx / Rnn in float32 -- from the registers of the caller, an LDS tile or memory -- as ONE batch of independent loads, and may be
// called again: with RECOMPUTE the Cholesky factor and Rxx are NOT kept across the squarings -- both matrices are fetched and the factor
// is formed a second time for the back substitution -- so that only B and B^2 live through the loop (P = 7: 2 x 98 registers instead of
// 2 x 98 + 112 + 49: two waves per SIMD instead of one; P = 8 runs without scratch).
// Whitening C = L^-1 Rxx L^-H as LAPACK's zhegs2 does it (itype 1, lower): in place on the Hermitian half, P^3 / 2 complex multiply-adds
// where the column-by-column form of round 2 took 1.2 P^3.
// t1: this problem's P entries, gain: d0 / (d0 + mu).  Returns `suspect` (group_dominant, k_solve.h: C may be indefinite and the
// dominant eigenpair not the top one); SHIFT: the second pass of a wave with such a pencil, which solves it again on C + ||C||_F I
// where `shift` and repeats the first pass elsewhere.  Float64 squarings only.
template <int P, bool RECOMPUTE, bool SQ32, bool SHIFT, class LA, class LB>
__device__ __forceinline__ bool gevd_solve_thread_pass(LA load_a, LB load_b, const double mu, c64* t1, double& gain_out, const bool shift = false) {
    static_assert(!(SQ32 && SHIFT), "the shifted pass squares in float64");
    constexpr int NO = P > 1 ? P * (P - 1) / 2 : 1;
    auto lo = [](int i, int k) { return i * (i - 1) / 2 + k; };
    auto f2z = [](c32 v) { return make_double2((double)v.x, (double)v.y); };
    HermReg<P> B;
    double tr = 0.0;
    double Ld[P], rL[P];
    c64 Lo[NO];
    float a_d[P], b_d[P];
    c32 a_o[NO], b_o[NO];
    if constexpr (SHIFT) asm volatile("" ::: "memory");   // the second pass loads again (not merged with the first: see gevd_solve_group)
    load_b(b_d, b_o);
    load_a(a_d, a_o);
    auto ad = [&](int i) { return (double)a_d[i]; };
    auto ao = [&](int i, int k) { return f2z(a_o[i * (i - 1) / 2 + k]); };
    auto bd = [&](int i) { return (double)b_d[i]; };
    auto bo = [&](int i, int k) { return f2z(b_o[i * (i - 1) / 2 + k]); };
    thread_cholesky<P>(bd, bo, Ld, rL, Lo);
    {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            B.d[i] = ad(i);
#pragma unroll
            for (int k = 0; k < i; ++k) B.o[lo(i, k)] = ao(i, k);
        }
#pragma unroll
        for (int k = 0; k < P; ++k) {
            const double akk = B.d[k] * rL[k] * rL[k];
            B.d[k] = akk;
            tr += akk;
            const double ct = -0.5 * akk;
#pragma unroll
            for (int i = k + 1; i < P; ++i) {                    // x = A(k+1:, k) / L(k, k) + ct L(k+1:, k)
                const c64 l_ik = Lo[lo(i, k)];
                c64 x = zscale(B.o[lo(i, k)], rL[k]);
                x.x = fma(ct, l_ik.x, x.x);
                x.y = fma(ct, l_ik.y, x.y);
                B.o[lo(i, k)] = x;
            }
#pragma unroll
            for (int i = k + 1; i < P; ++i) {                    // A(k+1:, k+1:) -= x y^H + y x^H,  y = L(k+1:, k)   (lower triangle)
                const c64 xi = B.o[lo(i, k)], yi = Lo[lo(i, k)];
                B.d[i] = fma(-2.0 * xi.y, yi.y, fma(-2.0 * xi.x, yi.x, B.d[i]));
#pragma unroll
                for (int j = k + 1; j < i; ++j) {
                    const c64 xj = B.o[lo(j, k)], yj = Lo[lo(j, k)];
                    B.o[lo(i, j)] = zfnmac(zfnmac(B.o[lo(i, j)], xi, yj), yi, xj);
                }
            }
#pragma unroll
            for (int i = k + 1; i < P; ++i) {                    // x += ct y, then x <- L(k+1:, k+1:)^-1 x
                const c64 l_ik = Lo[lo(i, k)];
                c64 x = B.o[lo(i, k)];
                x.x = fma(ct, l_ik.x, x.x);
                x.y = fma(ct, l_ik.y, x.y);
#pragma unroll
                for (int m = k + 1; m < i; ++m) x = zfnma(x, Lo[lo(i, m)], B.o[lo(m, k)]);
                B.o[lo(i, k)] = zscale(x, rL[i]);
            }
        }
    }
    // ---- dominant eigenpair by repeated squaring of B = C / tr C (see k_solve.h); tau = tr(B^2) = ||B||_F^2 is real here
    double fro = 0.0;                                            // ||C||_F^2
#pragma unroll
    for (int i = 0; i < P; ++i) fro = fma(B.d[i], B.d[i], fro);
#pragma unroll
    for (int q = 0; q < NO; ++q) fro = fma(2.0 * B.o[q].x, B.o[q].x, fma(2.0 * B.o[q].y, B.o[q].y, fro));
    DISCO_CONSUME(fro);          // formed HERE: sunk to its use at the end, it kept the unscaled B live through the squarings
    if constexpr (SHIFT) {
        const double sh = sqrt(fro);
#pragma unroll
        for (int i = 0; i < P; ++i) B.d[i] = shift ? B.d[i] + sh : B.d[i];
        tr = shift ? tr + P * sh : tr;
    }
    const bool tr_bad = DISCO_TRACE_BAD(tr, fro);
    bool exit0 = false;
    const bool ok = DISCO_TRACE_OK(tr);
    {
        const double rt = ok ? rcp64(tr) : 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) B.d[i] = ok ? B.d[i] * rt : 0.0;
#pragma unroll
        for (int q = 0; q < NO; ++q) B.o[q] = ok ? zscale(B.o[q], rt) : make_double2(0.0, 0.0);
    }
    bool done = !ok || P == 1;
    // SQ32 (round 5): the choice of the start vector and all but the LAST power step on packed float32 as well -- 2 P^2 v_pk_fma_f32 per
    // step where the float64 form issues 4 P^2 half-rate v_fma_f64.  A power step is self-correcting (its result is the dominant vector
    // of the matrix it multiplies by, to that multiplication's rounding over the gap of the SQUARED matrix, < 0.01 here), and the closing
    // float64 step removes the float32 rounding of the steps before it: the vector that enters the back substitution is as accurate as before.
    constexpr int STEPS32 = (SQ32 && P > 1 && DISCO_POWER_STEPS > 1) ? DISCO_POWER_STEPS - 1 : 0;
    c32 vf[SQ32 ? P : 1];
    bool have32 = false;
    if constexpr (SQ32 && P > 1) {
        HermPk<P> Bf;
#pragma unroll
        for (int m = 0; m < HermPk<P>::ND; ++m) Bf.dp[m] = make_float2((float)B.d[2 * m], 2 * m + 1 < P ? (float)B.d[2 * m + 1] : 0.f);
#pragma unroll
        for (int q = 0; q < NO; ++q) Bf.o[q] = make_float2((float)B.o[q].x, (float)B.o[q].y);
        for (int it = 0; it < DISCO_SQUARINGS_MAX; ++it) {
            if (!__any(!done)) break;
            HermPk<P> S;
            const float tau = herm_square_pk<P>(Bf, S);
            const float rtau = tau > 0.f ? 1.0f / tau : 0.f;
            const c32 rr = make_float2(rtau, rtau);
            if (!done) {
#pragma unroll
                for (int m = 0; m < HermPk<P>::ND; ++m) Bf.dp[m] = PkD::mul_comp(S.dp[m], rr);
#pragma unroll
                for (int q = 0; q < NO; ++q) Bf.o[q] = scale_by_half<0>(S.o[q], rr);
            }
            DISCO_SQUARING_AFTER_F32(tau, done);
        }
        // the longest column of the kept square and STEPS32 power steps, still in float32 (B comes back to float64 only afterwards: the
        // two copies never live together)
        {
            auto atf = [&](int i, int k) {               // B[i][k] of the float32 half-storage (i, k compile-time after unrolling)
                if (i == k) return make_float2((i & 1) ? Bf.dp[i / 2].y : Bf.dp[i / 2].x, 0.f);
                if (i > k) return Bf.o[lo(i, k)];
                const c32 v = Bf.o[lo(k, i)];
                return make_float2(v.x, -v.y);
            };
            float best = -1.f;
#pragma unroll
            for (int j = 0; j < P; ++j) {
                float nj = 0.f;
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    const c32 b = atf(i, j);
                    nj += b.x * b.x + b.y * b.y;
                }
                if (nj > best) {
                    best = nj;
#pragma unroll
                    for (int i = 0; i < P; ++i) vf[i] = atf(i, j);
                }
            }
            have32 = best > 0.f;
            const float rb = have32 ? rsqrtf(best) : 0.f;
#pragma unroll
            for (int i = 0; i < P; ++i) vf[i] = have32 ? make_float2(vf[i].x * rb, vf[i].y * rb) : make_float2(i == 0 ? 1.f : 0.f, 0.f);
#pragma unroll 1
            for (int s = 0; s < STEPS32; ++s) {
                c32 u[P];
#pragma unroll
                for (int i = 0; i < P; ++i) u[i] = (i & 1) ? scale_by_half<1>(vf[i], Bf.dp[i / 2]) : scale_by_half<0>(vf[i], Bf.dp[i / 2]);
                // the two halves of every complex multiply-add apart, the sums advancing together (see herm_square_pk)
#pragma unroll
                for (int half = 0; half < 2; ++half)
#pragma unroll
                    for (int k = 0; k < P; ++k)
#pragma unroll
                        for (int i = 0; i < P; ++i) {
                            if (i == k) continue;
                            const c32 b = i > k ? Bf.o[lo(i, k)] : Bf.o[lo(k, i)];   // B[i][k] = conj of the stored entry above the diagonal
                            if (half == 0) u[i] = PkD::cfma_lo(b, vf[k], u[i]);
                            else if (i > k) u[i] = PkD::cfma_hi(b, vf[k], u[i]);
                            else u[i] = PkD::cfma_hi_conj(b, vf[k], u[i]);
                        }
                if (have32) {
#pragma unroll
                    for (int i = 0; i < P; ++i) vf[i] = u[i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < P; ++i) B.d[i] = (double)((i & 1) ? Bf.dp[i / 2].y : Bf.dp[i / 2].x);
#pragma unroll
        for (int q = 0; q < NO; ++q) B.o[q] = make_double2((double)Bf.o[q].x, (double)Bf.o[q].y);
    } else {
    for (int it = 0; it < DISCO_SQUARINGS_MAX; ++it) {
        if (!__any(!done)) break;
        HermReg<P> S;
        double tau = 0.0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            double dj = 0.0;
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const c64 b = B.at(j, k);
                dj = fma(b.x, b.x, fma(b.y, b.y, dj));
            }
            S.d[j] = dj;
            tau += dj;
#pragma unroll
            for (int i = j + 1; i < P; ++i) {
                c64 a = make_double2(0.0, 0.0);
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    const c64 x = B.at(i, k), y = B.at(k, j);
                    a.x = fma(x.x, y.x, fma(-x.y, y.y, a.x));
                    a.y = fma(x.x, y.y, fma(x.y, y.x, a.y));
                }
                S.o[lo(i, j)] = a;
            }
        }
        const double rtau = tau > 0.0 ? rcp64(tau) : 0.0;
        if (!done) {
#pragma unroll
            for (int i = 0; i < P; ++i) B.d[i] = S.d[i] * rtau;
#pragma unroll
            for (int q = 0; q < NO; ++q) B.o[q] = zscale(S.o[q], rtau);
        }
        DISCO_SQUARING_AFTER(it, tau, tau > 0.0, done, exit0);
    }
    }
    // ---- B = v0 v0^H: the longest column (ties: lowest index), normalised
    c64 v0[P];
    bool have;
    double kept = 0.0;                                           // tr(B^2) of the kept square (float64 form)
    if constexpr (SQ32 && P > 1) {
        have = have32;
#pragma unroll
        for (int i = 0; i < P; ++i) v0[i] = make_double2((double)vf[i].x, (double)vf[i].y);
    } else {
        double best = -1.0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            double nj = 0.0;
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const c64 b = B.at(i, j);
                nj += b.x * b.x + b.y * b.y;
            }
            kept += nj;
            if (nj > best) {
                best = nj;
#pragma unroll
                for (int i = 0; i < P; ++i) v0[i] = B.at(i, j);
            }
        }
        have = best > 0.0;
        DISCO_CONSUME(kept);     // (as fro above: formed here, not from a B kept live to the end)
        const double rb = have ? rsqrt64(best) : 0.0;
#pragma unroll
        for (int i = 0; i < P; ++i) v0[i] = have ? zscale(v0[i], rb) : make_double2(i == 0 ? 1.0 : 0.0, 0.0);
    }
    // ---- power steps v <- B v on the kept square (k_solve.h: DISCO_POWER_STEPS), then unit length
    // SQ32 (round 5): all but the LAST step on packed float32 as well -- 2 P^2 v_pk_fma_f32 per step where the float64 form issues 4 P^2
    // half-rate v_fma_f64.  A power step is self-correcting (its result is the dominant vector of the matrix it multiplies by, to that
    // multiplication's rounding over the gap of the SQUARED matrix, < 0.01 here), and the closing float64 step removes the float32
    // rounding of the steps before it: the vector that goes into the back substitution is as accurate as before.
    if (P > 1) {
#pragma unroll 1
        for (int s = STEPS32; s < DISCO_POWER_STEPS; ++s) {
            c64 u[P];
#pragma unroll
            for (int i = 0; i < P; ++i) {
                c64 a = make_double2(0.0, 0.0);
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    const c64 b = B.at(i, k);
                    a.x = fma(b.x, v0[k].x, fma(-b.y, v0[k].y, a.x));
                    a.y = fma(b.x, v0[k].y, fma(b.y, v0[k].x, a.y));
                }
                u[i] = a;
            }
            if (have) {
#pragma unroll
                for (int i = 0; i < P; ++i) v0[i] = u[i];
            }
        }
        if (DISCO_POWER_STEPS > 0 && have) {
            double n2 = 0.0;
#pragma unroll
            for (int i = 0; i < P; ++i) n2 = fma(v0[i].x, v0[i].x, fma(v0[i].y, v0[i].y, n2));
            const double rn = rsqrt64(n2);
#pragma unroll
            for (int i = 0; i < P; ++i) v0[i] = zscale(v0[i], rn);
        }
    }
    // ---- q = L^-H v0, d0 = q^H Rxx q (q^H Rnn q = 1), t1 = q L[0][0] conj(v0[0]), w = t1 d0 / (d0 + mu)
    if constexpr (RECOMPUTE) {
        // the squarings must not see the factor as live: an opaque touch of v0 keeps hipcc from hoisting this second factorisation
        // (bit-identical to the first) above the loop and carrying it through
        DISCO_CONSUME(v0[0].x);
        load_b(b_d, b_o);
        load_a(a_d, a_o);
            thread_cholesky<P>(bd, bo, Ld, rL, Lo);
    }
    c64 q[P];
#pragma unroll
    for (int i = P - 1; i >= 0; --i) {
        c64 a = v0[i];
#pragma unroll
        for (int k = i + 1; k < P; ++k) a = zfnmca(a, Lo[lo(k, i)], q[k]);
        q[i] = zscale(a, rL[i]);
    }
    double d0 = 0.0;
#pragma unroll
    for (int i = 0; i < P; ++i) {
        c64 sj = make_double2(ad(i) * q[i].x, ad(i) * q[i].y);
#pragma unroll
        for (int k = 0; k < P; ++k) {
            if (k == i) continue;
            const c64 e = k < i ? ao(i, k) : ao(k, i);
            sj = k < i ? zfma(sj, e, q[k]) : zfmca(sj, e, q[k]);
        }
        d0 += q[i].x * sj.x + q[i].y * sj.y;
    }
    d0 = have ? d0 : 0.0;
    gain_out = mwf_gain(d0, mu);
    const c64 gsc = make_double2(Ld[0] * v0[0].x, -Ld[0] * v0[0].y);
#pragma unroll
    for (int i = 0; i < P; ++i) t1[i] = zmul(q[i], gsc);
    // (the SQ32 form is reached only from the online mode, whose pencils are PSD by construction: it flags nothing)
    return !SQ32 && P > 1 && (DISCO_SUSPECT(P, tr_bad, exit0, kept) || d0 < 0.0);
}

// w, t1: this problem's P filter entries.  Contains a wave-wide vote: every lane of the wave must call it (dead lanes pass Rxx = 0, Rnn = I).
template <int P, bool RECOMPUTE, bool SQ32, class LA, class LB>
__device__ __forceinline__ void gevd_solve_thread_acc(LA load_a, LB load_b, const double mu, c64* w, c64* t1) {
    double gain;
    const bool suspect = gevd_solve_thread_pass<P, RECOMPUTE, SQ32, false>(load_a, load_b, mu, t1, gain);
    if constexpr (!SQ32 && P > 1) {
        // a flagged pencil re-solves its whole wave (wave-uniform vote; never taken by a PSD pencil): the others repeat the first pass,
        // so that nothing of it has to stay live through the second
        if (__any(suspect)) (void)gevd_solve_thread_pass<P, RECOMPUTE, false, true>(load_a, load_b, mu, t1, gain, suspect);
    }
#pragma unroll
    for (int i = 0; i < P; ++i) w[i] = zscale(t1[i], gain);
}

// the same with both matrices handed over in registers as (diag, strict lower triangle) in float32 (the online kernel's state)
template <int P, bool SQ32 = false>
__device__ __forceinline__ void gevd_solve_thread(const float* a_d, const c32* a_o, const float* b_d, const c32* b_o, const double mu,
                                                  c64* w, c64* t1) {
    constexpr int NO = P > 1 ? P * (P - 1) / 2 : 1;
    auto copy = [](const float* sd, const c32* so, float* d, c32* o) {
#pragma unroll
        for (int i = 0; i < P; ++i) d[i] = sd[i];
#pragma unroll
        for (int q = 0; q < NO; ++q) o[q] = so[q];
    };
    gevd_solve_thread_acc<P, (P >= 6), SQ32>([&](float* d, c32* o) { copy(a_d, a_o, d, o); }, [&](float* d, c32* o) { copy(b_d, b_o, d, o); }, mu, w, t1);
}

#ifndef DISCO_SOLVE_LOAD_GROUP
#define DISCO_SOLVE_LOAD_GROUP 4        // partial blocks of an entry fetched together by k_gevd_mwf_r1_thread's loader
#endif
// threads per workgroup: two waves, one for the larger pencils (the wave-cooperative fetch stages 64 * NP float4 per wave in LDS)
template <int P>
constexpr int solve_small_threads() { return P <= 6 ? 128 : 64; }

template <int P, bool FROM_PART>
__global__ DISCO_KERNEL_ALIGN __launch_bounds__(solve_small_threads<P>()) void k_gevd_mwf_r1_thread(SolveSrc src, long long n_prob, double mu,
                                                                              c32* __restrict__ w_out, c32* __restrict__ t1_out) {
    constexpr int SOLVE_SMALL_THREADS = solve_small_threads<P>();
    constexpr int NP = P * (P + 1) / 2;
    constexpr bool RECOMPUTE = P >= 6;
    const long long pid = (long long)blockIdx.x * SOLVE_SMALL_THREADS + threadIdx.x;
    const bool live = pid < n_prob;
    const long long pc = live ? pid : n_prob - 1;                 // dead lanes stand in for the last pencil (and store nothing)
    c64 w[P], t1[P];
    if constexpr (FROM_PART) {
        // The partial sums of a wave's 64 pencils are 64 * NP consecutive float4 per block (pencils are (g, f)-major like the partial
        // array): fetched lane-linearly, the blocks of an entry combined in float64 and rounded once (as in every other loader), and
        // handed over through LDS -- a thread loading its own NP entries reads 16 bytes of every 16 NP, NP times over, and the lines do
        // not survive in L1 / L2 in between (PMC, C3: 2.07 GB fetched for 0.33 GB of partial sums).  Entries of the leading
        // M_loc x M_loc block come from the step-1 partial sums (SolveSrc::part_loc) -- since round 4 through the same fetch.
        __shared__ float4 s_tile[SOLVE_SMALL_THREADS / 64][64 * NP];
        const int lane = threadIdx.x & 63, wv = wave_id();
        const int ML = src.M_loc, NPL = ML * (ML + 1) / 2;
        const long long g = pc / src.F;
        const int f = (int)(pc % src.F);
        const long long off = ((g * src.chunks) * src.F + f) * (long long)NP;                    // block 0 of this lane's pencil
        const long long offl = ML > 0 ? ((g * src.chunks_loc) * src.F + f) * (long long)NPL : 0;
        const int off_lo = (int)(unsigned)(off & 0xffffffffLL), off_hi = (int)(off >> 32);
        const int offl_lo = (int)(unsigned)(offl & 0xffffffffLL), offl_hi = (int)(offl >> 32);
        const double it = (double)src.inv_T;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int e = lane + 64 * k, pe = e / NP, q = e % NP;     // element e of the wave's block belongs to lane pe's pencil
            int r = 0, rem = q;                                       // q = (r, c), r <= c, in the row-major upper triangle of P
#pragma unroll
            for (int rr = 0; rr < P - 1; ++rr) {
                if (rem >= P - r) {
                    rem -= P - r;
                    ++r;
                }
            }
            const int c = r + rem;
            const bool loc = c < ML;
            const long long o_main = ((long long)__shfl(off_hi, pe) << 32) | (unsigned)__shfl(off_lo, pe);
            const long long o_loc = ((long long)__shfl(offl_hi, pe) << 32) | (unsigned)__shfl(offl_lo, pe);
            const float4* ptr = loc ? src.part_loc + o_loc + (r * ML - (r * (r - 1)) / 2 + (c - r)) : src.part + o_main + q;
            const long long stride = loc ? (long long)src.F * NPL : (long long)src.F * NP;
            const int nch = loc ? src.chunks_loc : src.chunks;
            // Blocks in groups of FOUR, every load of a group unconditional (a block that does not exist re-reads block 0 and is weighed 0), so
            // that the loads of ALL entries of the unrolled loop are independent and in flight together: the fused STFT + covariance pass
            // leaves 4 blocks per node at BASELINE's batch sizes (runs of 40 frames per wave: the length of its float32 sums is what C3's
            // distance from the float64 oracle follows, profiles/r05_t_*); a block count beyond 4 takes another round of the loop.
            double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
            for (int c0 = 0; c0 < nch; c0 += DISCO_SOLVE_LOAD_GROUP) {
                float4 v[DISCO_SOLVE_LOAD_GROUP];
#pragma unroll
                for (int u = 0; u < DISCO_SOLVE_LOAD_GROUP; ++u) v[u] = ptr[(c0 + u < nch ? c0 + u : 0) * stride];
#pragma unroll
                for (int u = 0; u < DISCO_SOLVE_LOAD_GROUP; ++u) {
                    const double m = c0 + u < nch ? 1.0 : 0.0;
                    sx += m * (double)v[u].x;
                    sy += m * (double)v[u].y;
                    sz += m * (double)v[u].z;
                    sw += m * (double)v[u].w;
                }
            }
            s_tile[wv][e] = make_float4((float)(sx * it), (float)(sy * it), (float)(sz * it), (float)(sw * it));
        }
        DISCO_GROUP_SYNC();                                           // wave-local hand-over
        const float4* tp = &s_tile[wv][lane * NP];
        // entry (i, k), i >= k, of the Hermitian matrices = conj of the stored upper-triangle entry (k, i)
        auto tri = [](int k, int i) { return k * P - (k * (k - 1)) / 2 + (i - k); };
        gevd_solve_thread_acc<P, RECOMPUTE, false>(
            [&](float* d, c32* o) {
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    d[i] = tp[tri(i, i)].x;
#pragma unroll
                    for (int k = 0; k < i; ++k) o[i * (i - 1) / 2 + k] = make_float2(tp[tri(k, i)].x, -tp[tri(k, i)].y);
                }
            },
            [&](float* d, c32* o) {
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    d[i] = tp[tri(i, i)].z;
#pragma unroll
                    for (int k = 0; k < i; ++k) o[i * (i - 1) / 2 + k] = make_float2(tp[tri(k, i)].z, -tp[tri(k, i)].w);
                }
            },
            mu, w, t1);
    } else {
        const c32* A = src.Rss + pc * P * P;
        const c32* Bm = src.Rnn + pc * P * P;
        auto ld = [](const c32* m, float* d, c32* o) {
#pragma unroll
            for (int i = 0; i < P; ++i) {
                d[i] = m[i * P + i].x;
#pragma unroll
                for (int k = 0; k < i; ++k) o[i * (i - 1) / 2 + k] = m[i * P + k];
            }
        };
        gevd_solve_thread_acc<P, RECOMPUTE, false>([&](float* d, c32* o) { ld(A, d, o); }, [&](float* d, c32* o) { ld(Bm, d, o); }, mu, w, t1);
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < P; ++i) {
            w_out[pid * P + i] = make_float2((float)w[i].x, (float)w[i].y);
            if (t1_out) t1_out[pid * P + i] = make_float2((float)t1[i].x, (float)t1[i].y);
        }
    }
}

}  // namespace disco
