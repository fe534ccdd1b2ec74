// Masked covariance partial sums for 17 <= P <= 32 (step 2 of networks whose pencil P = M + K - 1 exceeds 16 channels).
//
// Same output as every other covariance kernel: part[g][chunk][f][q], q over the upper triangle, float4 (Rss.re, Rss.im, Rnn.re,
// Rnn.im), float32 sums over the chunk's frames.  NP = P(P+1)/2 reaches 528 pairs = 2112 accumulators per bin, so the triangle is cut
// into BLOCKS: the components are taken in groups of CW_GRP = 4 ([4a, 4a + 4)), and the block (a, b), a <= b, of 4 x 4 pairs is owned by
// one wave.  A lane keeps 16 pairs x 2 statistics in registers (64 VGPRs) and loads the 8 components its block touches (4 + 4 complex
// values per statistic): ~110 VGPRs, 4 waves per SIMD.  (k_cov_big's "every wave loads all P components and owns pairs q % 4" would
// need 132 pairs per wave and 64 live inputs per lane at P = 32: spills.)  ceil(P / 4) groups give 15 (P = 17..20) to 36 (P = 29..32)
// blocks; a workgroup of CW_WAVES waves serves CW_WAVES consecutive blocks of one (node, 64-bin tile, frame chunk).
// Every component is loaded by the ceil(P / 4) waves whose block touches its group: these re-loads are served by L1 / L2, HBM sees
// each sample once per node.  The workgroups of one (room, tile, chunk) -- all its blocks and all K nodes, which read the same K - 1 z
// rows -- are consecutive logical items dealt to ONE XCD (as k_apply_m): a z row of a room is fetched from HBM once and shared through
// that L2 by the K nodes.  The Nyquist bin gets one more tile whose lanes stride over frames (as in k_cov_big).
#pragma once
#include "common.h"
#include "k_cov.h"

namespace disco {

constexpr int CW_GRP = 4, CW_WAVES = 4, CW_PMAX = 32;

__host__ __device__ constexpr int cov_wide_groups(int P) { return (P + CW_GRP - 1) / CW_GRP; }
__host__ __device__ constexpr int cov_wide_blocks(int P) { return cov_wide_groups(P) * (cov_wide_groups(P) + 1) / 2; }

template <bool SAMEZ>
__device__ __forceinline__ void cov_wide_wave(const CovArgs& a, int M, int KR, long long g, int c, int tile, int ga, int gb, int lane) {
    const int P = M + KR, NP = P * (P + 1) / 2;
    const int K = a.K, T = a.T, F = a.F, nbin = F - 1, tiles = (nbin + 63) / 64;
    const long long r = g / a.Kl;
    const int k = a.k0 + (int)(g % a.Kl);
    const long long TF = (long long)T * F;
    const int t0 = (int)(((long long)T * c) / a.chunks), t1 = (int)(((long long)T * (c + 1)) / a.chunks);
    const bool nyq = tile == tiles;
    int f = nyq ? nbin : tile * 64 + lane;
    const bool live = nyq || f < nbin;
    if (f > nbin) f = nbin;
    const int t_step = nyq ? 64 : 1, t_off = nyq ? lane : 0;
    // the 8 components of the block: e < 4 -> 4 ga + e, else 4 gb + e - 4.  Per component the plane (wave-uniform), its stride per
    // (t, f) element (M for the node's own channels, 1 for a z row, 0 past P) and whether the local mask weighs it
    const c32* ps[8];
    const c32* pn[8];
    int stride[8];
    bool loc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int p = e < 4 ? CW_GRP * ga + e : CW_GRP * gb + e - 4;
        if (p < M) {
            ps[e] = pn[e] = a.X + g * TF * M + p;
            stride[e] = M;
            loc[e] = true;
        } else if (p < P) {
            const int jj = p - M, j = jj < k ? jj : jj + 1;      // concatenate_signals order: z_j (j < k), z_j (j > k)
            const long long zo = z_plane(r, j, K, a.R, a.zblk) * TF;
            ps[e] = a.Zs + zo;
            pn[e] = SAMEZ ? ps[e] : a.Zn + zo;
            stride[e] = 1;
            loc[e] = false;
        } else {
            ps[e] = pn[e] = a.X;
            stride[e] = 0;
            loc[e] = true;
        }
    }
    const float* mg = a.mask + g * TF;
    const bool diag = ga == gb;
    c32 acc_s[16], acc_n[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc_s[q] = acc_n[q] = make_float2(0.f, 0.f);
    for (int tu = t0; tu < t1; tu += t_step) {
        const int t = tu + t_off;
        const bool ok = live && t < t1;
        const long long tf = (long long)(ok ? t : t0) * F + f;
        const float mraw = mg[tf];
        const float m = ok ? mraw : 0.f, mc = ok ? 1.f - mraw : 0.f;
        const float gs = a.mask_remote ? m : (ok ? 1.f : 0.f), gn = a.mask_remote ? mc : (ok ? 1.f : 0.f);
        c32 vs[8], vn[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool on = stride[e] != 0;
            const c32 xs = on ? ps[e][tf * stride[e]] : make_float2(0.f, 0.f);
            const c32 xn = SAMEZ ? xs : (on ? pn[e][tf * stride[e]] : make_float2(0.f, 0.f));
            const float ws = loc[e] ? m : gs, wn = loc[e] ? mc : gn;
            vs[e] = make_float2(ws * xs.x, ws * xs.y);
            vn[e] = make_float2(wn * xn.x, wn * xn.y);
        }
#pragma unroll
        for (int er = 0; er < 4; ++er) {
#pragma unroll
            for (int ec = 0; ec < 4; ++ec) {
                const int q = er * 4 + ec;
                const c32 si = vs[er], sj = vs[4 + ec], ni = vn[er], nj = vn[4 + ec];
                // v_i conj(v_j)
                acc_s[q].x = fmaf(si.x, sj.x, fmaf(si.y, sj.y, acc_s[q].x));
                acc_n[q].x = fmaf(ni.x, nj.x, fmaf(ni.y, nj.y, acc_n[q].x));
                if (!(diag && er == ec)) {
                    acc_s[q].y = fmaf(si.y, sj.x, fmaf(-si.x, sj.y, acc_s[q].y));
                    acc_n[q].y = fmaf(ni.y, nj.x, fmaf(-ni.x, nj.y, acc_n[q].y));
                }
            }
        }
    }
    if (nyq) {      // whole wave: reduce the 64 per-lane partial sums of the Nyquist bin
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                acc_s[q].x += __shfl_xor(acc_s[q].x, off);
                acc_s[q].y += __shfl_xor(acc_s[q].y, off);
                acc_n[q].x += __shfl_xor(acc_n[q].x, off);
                acc_n[q].y += __shfl_xor(acc_n[q].y, off);
            }
    }
    if (live && (!nyq || lane == 0)) {
        float4* o = a.part + (((g * a.chunks + c) * F) + f) * (long long)NP;
#pragma unroll
        for (int er = 0; er < 4; ++er) {
#pragma unroll
            for (int ec = 0; ec < 4; ++ec) {
                const int i = CW_GRP * ga + er, j = CW_GRP * gb + ec, q = er * 4 + ec;
                if (j < P && (!diag || ec >= er))
                    o[i * P - (i * (i - 1)) / 2 + (j - i)] = make_float4(acc_s[q].x, acc_s[q].y, acc_n[q].x, acc_n[q].y);
            }
        }
    }
}

// grid: n_items = R * Kl * (tiles + 1) * chunks * nbg logical items (nbg = ceil(blocks / CW_WAVES)), padded to a multiple of
// N_XCD (xcd_item, common.h); block = 64 * CW_WAVES threads, wave w of item bg takes block bg * CW_WAVES + w
template <bool SAMEZ>
__global__ __launch_bounds__(64 * CW_WAVES) void k_cov_wide(CovArgs a, int M, int KR) {
    const int P = M + KR, ng = cov_wide_groups(P), nblk = cov_wide_blocks(P), nbg = (nblk + CW_WAVES - 1) / CW_WAVES;
    const int tiles = (a.F - 1 + 63) / 64;
    const long long n_items = a.R * a.Kl * (long long)(tiles + 1) * a.chunks * nbg;
    long long item = xcd_item();
    if (item >= n_items) return;
    const int bg = (int)(item % nbg);
    item /= nbg;
    const int kl = (int)(item % a.Kl);
    item /= a.Kl;
    const int c = (int)(item % a.chunks);
    item /= a.chunks;
    const int tile = (int)(item % (tiles + 1));
    const long long g = (item / (tiles + 1)) * a.Kl + kl;
    int blk = bg * CW_WAVES + (int)(threadIdx.x / 64);
    if (blk >= nblk) return;                     // (whole wave; the kernel has no workgroup barrier)
    int ga = 0;
    while (blk >= ng - ga) {                     // blocks enumerated row by row: (0, 0..ng-1), (1, 1..ng-1), ...
        blk -= ng - ga;
        ++ga;
    }
    const int gb = ga + blk;
    cov_wide_wave<SAMEZ>(a, M, KR, g, c, tile, ga, gb, (int)(threadIdx.x & 63));
}

}  // namespace disco
