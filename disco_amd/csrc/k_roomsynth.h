// Between a reverberated source and a room the path can enhance (gen_disco/convolve_signals.py:102-115, 255-273; post_generator.py:99-115):
//   k_vad_samples   vad_oracle_batch (sigproc_utils.py:12-55) with one decision per SAMPLE and a length per signal -- the phases of
//                   k_vad_mask (k_vad.h: mean, radix-select quantile, counts per hop segment), then window -> segment -> sample
//   k_mix_scaled    n_out = gain * n (a shorter noise lands in a zero buffer), y_out = s + n_out, zeros beyond a signal's length
// and a meeting room of S talkers (gen_meetit/convolve_signals.py:140-148, 176-185):
//   k_source_mix    per channel: the mix of all S images, the image of the channel's own talker, the sum of the others -- one pass
#pragma once
#include <cstdint>

#include "k_vad.h"

namespace disco {

// number of windows of vad_oracle_batch, int(ceil((L - win) / hop + 1)) in integers: 0 while L <= win - hop
__host__ __device__ __forceinline__ int vad_n_windows(int L, int win, int hop) {
    const long long a = (long long)L - win + hop;
    return a <= 0 ? 0 : (int)((a + hop - 1) / hop);
}

// One workgroup per signal.  x [n_sig][len]; stop: n_sig ints (clamped into [0, len]) or NULL; vad [n_sig][len] of 0.f / 1.f, zeros at and
// beyond L = stop[sig].  Nothing of x at or beyond L is read.  len <= VAD_MAX_SEG * hop, win % hop == 0 (the host checks both).
static __global__ __launch_bounds__(VAD_THREADS) void k_vad_samples(const float* __restrict__ xs, const int* __restrict__ stop, float* __restrict__ vad,
                                                             int len, int win, int hop, float thr_rel, float quant, int rat) {
    __shared__ VadShared sh;
    __shared__ unsigned char win_on[VAD_MAX_SEG], seg_on[VAD_MAX_SEG];       // n_win <= n_seg <= VAD_MAX_SEG
    const int tid = threadIdx.x;
    const long long sig = blockIdx.x;
    const float* x = xs + sig * len;
    float* v = vad + sig * len;
    const int L = stop ? min(max(stop[sig], 0), len) : len;
    int n_seg = 0;
    if (L > 0) {                                                             // block-uniform
        const float mean = vad_mean(sh, x, L);
        const float thr = vad_threshold(sh, x, L, mean, thr_rel, quant);
        n_seg = vad_segment_counts(sh, x, L, hop, mean, thr);
        // window n covers segments n .. n + win/hop - 1 (clipped at L): active iff its count >= int(its length / rat)
        const int spw = win / hop, n_win = vad_n_windows(L, win, hop);
        for (int n = tid; n < n_win; n += VAD_THREADS) {
            int c = 0;
            for (int sg = n, e = min(n + spw, n_seg); sg < e; ++sg) c += sh.cnt[sg];
            const long long lo = (long long)n * hop, hi = lo + win < L ? lo + win : L;
            const int n_len = (int)(hi - lo);
            win_on[n] = c >= n_len / rat ? 1 : 0;
        }
        __syncthreads();
        // a segment is on iff an active window covers it: windows sg - spw + 1 .. sg
        for (int sg = tid; sg < n_seg; sg += VAD_THREADS) {
            unsigned char on = 0;
            for (int n = max(0, sg - spw + 1), e = min(sg, n_win - 1); n <= e; ++n) on |= win_on[n];
            seg_on[sg] = on;
        }
        __syncthreads();
    }
    // ---- one value per sample; 16-byte stores where the row allows it (L <= n_seg * hop: a sample below L has a segment)
    int t0 = 0;
    if ((((uintptr_t)v) & 15) == 0) {
        const int n4 = len / 4;
        for (int q = tid; q < n4; q += VAD_THREADS) {
            const int t = 4 * q;
            float4 o;
            o.x = (t + 0 < L && seg_on[(t + 0) / hop]) ? 1.f : 0.f;
            o.y = (t + 1 < L && seg_on[(t + 1) / hop]) ? 1.f : 0.f;
            o.z = (t + 2 < L && seg_on[(t + 2) / hop]) ? 1.f : 0.f;
            o.w = (t + 3 < L && seg_on[(t + 3) / hop]) ? 1.f : 0.f;
            *reinterpret_cast<float4*>(v + t) = o;
        }
        t0 = 4 * n4;
    }
    for (int t = t0 + tid; t < len; t += VAD_THREADS) v[t] = (t < L && seg_on[t / hop]) ? 1.f : 0.f;
}

constexpr int MIX_THREADS = 256;
constexpr int MIX_CHUNK = MIX_THREADS * 4;             // samples of one row a workgroup takes per step

// gain * n, rounded on its own, and s + that: the stored noise is exactly what was added (y - s == n_out), so no fused multiply-add here
// has_n / has_s: the sample lies below the end of the noise / of the signal; exact zeros elsewhere, whatever the gain is (inf, NaN)
__device__ __forceinline__ void mix_one(float g, float nv, float sv, bool has_n, bool has_s, float& n_o, float& y_o) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = g * nv;
    n_o = has_n ? p : 0.f;
    const float y = sv + n_o;
    y_o = has_s ? y : 0.f;
}

// Rows of s [n_sig][len] and n [n_sig][n_len], n_len <= len, one gain per `group` consecutive rows.  A workgroup takes MIX_CHUNK samples
// of one row per step of a grid-stride loop over (row, chunk).  n_out may be n itself (n_len == len): every sample is read before its own
// store and by no other thread.  VEC: len and n_len are multiples of 4 and every array is 16-byte aligned (the host checks), so each
// thread moves one float4 per array; neither s nor n is read at or beyond L = stop[row], so a float4 that straddles L is read by element.
template <bool VEC>
static __global__ __launch_bounds__(MIX_THREADS) void k_mix_scaled(const float* s, const float* n, const float* __restrict__ gain, int group,
                                                            const int* __restrict__ stop, float* n_out, float* y_out, long long n_sig,
                                                            int len, int n_len) {
    const int chunks = (len + MIX_CHUNK - 1) / MIX_CHUNK;
    const long long items = n_sig * chunks;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long row = it / chunks;
        const int t0 = (int)(it - row * chunks) * MIX_CHUNK + (int)threadIdx.x * 4;
        if (t0 >= len) continue;
        const int L = stop ? min(max(stop[row], 0), len) : len;
        const int Ln = min(L, n_len);                                        // the noise exists below Ln, the target below L
        const float g = gain[row / group];
        const float* sr = s ? s + row * len : nullptr;
        const float* nr = n + row * n_len;
        float nv[4] = {0.f, 0.f, 0.f, 0.f}, sv[4] = {0.f, 0.f, 0.f, 0.f}, no[4], yo[4];
        const int cnt = VEC ? 4 : min(4, len - t0);
        if (VEC && t0 + 4 <= Ln) {
            const float4 q = *reinterpret_cast<const float4*>(nr + t0);
            nv[0] = q.x, nv[1] = q.y, nv[2] = q.z, nv[3] = q.w;
        } else {
            for (int j = 0; j < cnt; ++j)
                if (t0 + j < Ln) nv[j] = nr[t0 + j];
        }
        if (sr) {
            if (VEC && t0 + 4 <= L) {
                const float4 q = *reinterpret_cast<const float4*>(sr + t0);
                sv[0] = q.x, sv[1] = q.y, sv[2] = q.z, sv[3] = q.w;
            } else {
                for (int j = 0; j < cnt; ++j)
                    if (t0 + j < L) sv[j] = sr[t0 + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) mix_one(g, nv[j], sv[j], t0 + j < Ln, t0 + j < L, no[j], yo[j]);
        if (VEC) {
            if (n_out) *reinterpret_cast<float4*>(n_out + row * len + t0) = make_float4(no[0], no[1], no[2], no[3]);
            if (y_out) *reinterpret_cast<float4*>(y_out + row * len + t0) = make_float4(yo[0], yo[1], yo[2], yo[3]);
        } else {
            for (int j = 0; j < cnt; ++j) {
                if (n_out) n_out[row * len + t0 + j] = no[j];
                if (y_out) y_out[row * len + t0 + j] = yo[j];
            }
        }
    }
}

constexpr int MIX_MAX_SOURCES = 8;
constexpr int MIX_MAX_CHANNELS = 64;
// the talker each channel of a room listens to, by value in the kernel's arguments (the host has checked every entry against S)
struct MixTargets {
    unsigned char t[MIX_MAX_CHANNELS];
};

// img [S][n_row][len], row = (room, channel), channel = row % n_mic -> y = ((img_0 + img_1) + img_2) + ..., s = img_tgt, n = the sum over
// j != tgt in ascending j, tgt = targets.t[channel]; each output [n_row][len] or NULL.  Plain float32 additions in exactly that order (there is
// no product to fuse, and no sum starts from a zero: -0 stays -0), so every output equals the NumPy float32 sums.  Exact zeros at and beyond
// L = stop[row], where no input is read.  The work split and VEC are k_mix_scaled's: one float4 per source and thread where len is a
// multiple of 4 and every array is 16-byte aligned, a float4 that straddles L read by element.
template <bool VEC>
static __global__ __launch_bounds__(MIX_THREADS) void k_source_mix(const float* __restrict__ img, int S, MixTargets targets, int n_mic,
                                                            const int* __restrict__ stop, float* __restrict__ y_out,
                                                            float* __restrict__ s_out, float* __restrict__ n_out, long long n_row, int len) {
    const int chunks = (len + MIX_CHUNK - 1) / MIX_CHUNK;
    const long long items = n_row * chunks;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const long long row = it / chunks;
        const int t0 = (int)(it - row * chunks) * MIX_CHUNK + (int)threadIdx.x * 4;
        if (t0 >= len) continue;
        const int L = stop ? min(max(stop[row], 0), len) : len;
        const int tgt = targets.t[row % n_mic];
        const int cnt = VEC ? 4 : min(4, len - t0);
        float yo[4] = {0.f, 0.f, 0.f, 0.f}, so[4] = {0.f, 0.f, 0.f, 0.f}, no[4] = {0.f, 0.f, 0.f, 0.f};
        if (t0 < L) {
            bool first_n = true;
            for (int j = 0; j < S; ++j) {
                const float* xr = img + ((long long)j * n_row + row) * len;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                if (VEC && t0 + 4 <= L) {
                    const float4 q = *reinterpret_cast<const float4*>(xr + t0);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                } else {
                    for (int e = 0; e < cnt; ++e)
                        if (t0 + e < L) v[e] = xr[t0 + e];
                }
                const bool own = j == tgt, start_n = !own && first_n;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    yo[e] = j == 0 ? v[e] : yo[e] + v[e];
                    so[e] = own ? v[e] : so[e];
                    no[e] = own ? no[e] : (start_n ? v[e] : no[e] + v[e]);
                }
                first_n = first_n && own;
            }                                                                // (a quad that straddles L: the unread samples are +0, and so are their sums)
        }
        float* const outs[3] = {y_out, s_out, n_out};
        const float* const vals[3] = {yo, so, no};
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            if (!outs[o]) continue;
            float* dst = outs[o] + row * len + t0;
            if (VEC) {
                *reinterpret_cast<float4*>(dst) = make_float4(vals[o][0], vals[o][1], vals[o][2], vals[o][3]);
            } else {
                for (int e = 0; e < cnt; ++e) dst[e] = vals[o][e];
            }
        }
    }
}

}  // namespace disco
