// STFT / oracle-mask / iSTFT kernels (librosa semantics, see oracle/stft_oracle.py for the restated
// algorithm and the reference call sites: tango.py:335-342, 528-539; math_utils.py:134-152).
//
// A wave owns one frame of one signal group at a time and transforms its channels two per complex FFT
// (fft.h).  Window and twiddle factors depend on the lane only and are held in registers; the only LDS is the
// wave-private exchange buffer, so the four waves of a block never synchronise with each other in the
// forward kernels.  All samples of a frame are requested before the first butterfly, and the spectra of all
// channel pairs are written together: one contiguous 8*chans-byte vector per (frame, bin), i.e. 512*chans
// contiguous bytes per wave store.
#pragma once
#include "fft.h"
#include "k_cov.h"

namespace disco {

#ifndef DISCO_STFT_WAVES
#define DISCO_STFT_WAVES 4
#endif
#ifndef DISCO_STFT_RUN
#define DISCO_STFT_RUN 16
#endif
constexpr int STFT_WAVES = DISCO_STFT_WAVES;     // waves per block; each streams its own run of frames
constexpr int STFT_RUN = DISCO_STFT_RUN;         // consecutive frames per wave
// host side: launch geometry of the per-wave-run kernels
inline int stft_runs(int T) { return (T + STFT_RUN - 1) / STFT_RUN; }
inline long long stft_blocks(long long n_witems) { return (n_witems + STFT_WAVES - 1) / STFT_WAVES; }

template <int N>
struct StftShared {
    c32 buf[STFT_WAVES][fft_buf_len<N>()];
};

template <int N>
__device__ __forceinline__ void load_window(float* w, const float* __restrict__ win, int lane) {
#pragma unroll
    for (int e = 0; e < FftPlan<N>::E; ++e) w[e] = win[lane + 64 * e];
}
// The analysis window at HALF weight: the transforms below run on (a + i b) / 2, which is what lets rfft_pair_untangle
// separate the two spectra with one packed add each (fft.h).  0.5 w is exact, so every spectrum is bit-for-bit what the
// full-weight window followed by the division gives.
template <int N>
__device__ __forceinline__ void load_window_half(float* w, const float* __restrict__ win, int lane) {
#pragma unroll
    for (int e = 0; e < FftPlan<N>::E; ++e) w[e] = 0.5f * win[lane + 64 * e];
}
// (a, b) * (w, w) for a full channel pair, (a, 0) * w when the pair's second channel does not exist.  One packed multiply per
// slot: the window registers are read as pairs (w[2m], w[2m+1]) and the slot's weight is broadcast by the operand selectors.
template <int N>
__device__ __forceinline__ void apply_window(c32* v, const c32* raw, const float* w, bool has_b) {
#pragma unroll
    for (int m = 0; m < FftPlan<N>::E / 2; ++m) {
        const c32 wp = make_float2(w[2 * m], w[2 * m + 1]);
        v[2 * m] = scale_by_half<0>(raw[2 * m], wp);
        v[2 * m + 1] = scale_by_half<1>(raw[2 * m + 1], wp);
        if (!has_b) {
            v[2 * m].y = 0.f;
            v[2 * m + 1].y = 0.f;
        }
    }
}

// Slots [E0, E1) of centre-padded frame t of the channel pair (xa, xb), un-windowed: v[e] = (a, b)[lane + 64 e].
// With hop = N/2 the first half of frame t+1 is the second half of frame t, so a wave streaming consecutive
// frames only ever fetches slots [E/2, E) after its first frame.
template <int N, int E0, int E1>
__device__ __forceinline__ void load_frame_slots(c32* v, const float* __restrict__ xa, const float* __restrict__ xb,
                                                 int t, int L, int pad_mode, int lane) {
    constexpr int H = N / 2;
    const int p0 = t * H - N / 2;
    const bool interior = (p0 + 64 * E0 >= 0) && (p0 + 64 * E1 <= L);      // wave-uniform (t is)
    // xb == xa for an odd channel count: the caller zeroes that half through the window (wb), so the loaded
    // values are never touched here -- a prefetched half-window must stay un-consumed until after the stores of the
    // current frame are issued (vmcnt is in-order: consuming a load early also waits for every older store).
    if (interior) {
#pragma unroll
        for (int e = E0; e < E1; ++e) {
            const int n = lane + 64 * e;
            v[e - E0] = make_float2(xa[p0 + n], xb[p0 + n]);
        }
    } else {                                                               // first / last frames only
#pragma unroll
        for (int e = E0; e < E1; ++e) {
            const int n = lane + 64 * e;
            v[e - E0] = make_float2(load_padded(xa, p0 + n, L, pad_mode), load_padded(xb, p0 + n, L, pad_mode));
        }
    }
}

// x: [n_sig][chans][L] -> X: [n_sig][T][F][chans].  CHP = ceil(chans / 2) channel pairs per frame.
// A wave streams STFT_RUN consecutive frames of one signal group: the next frame's new half-window is
// requested before the current frame is transformed (the loads fly under the butterflies), the shared
// half-window is recycled in registers.
template <int N, int CHP>
__global__ DISCO_KERNEL_ALIGN __launch_bounds__(64 * STFT_WAVES) void k_stft(const float* __restrict__ x, c32* __restrict__ X,
                                                           const float* __restrict__ win, const c32* __restrict__ tw,
                                                           int chans, int L, int T, int pad_mode, int runs_per_sig,
                                                           long long n_witems, const int* __restrict__ lens, int sig_per_room) {
    constexpr int E = FftPlan<N>::E, F = N / 2 + 1, NJ = E / 2 + 1, EH = E / 2;
    __shared__ StftShared<N> sh;
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * STFT_WAVES + wave;          // (g, run)
    if (item >= n_witems) return;                  // no block-level synchronisation anywhere below
    const long long g = item / runs_per_sig;
    const int t0 = (int)(item % runs_per_sig) * STFT_RUN;
    // L, T: the pitch of the arrays; Lr, Tr: the room's own clip (disco_set_lengths; the same without lengths)
    const int Lr = room_length(lens, lens ? g / sig_per_room : 0, L), Tr = lens ? 1 + Lr / (N / 2) : T;
    if (lens) {                                    // frames at or beyond T_r do not exist: exact zeros, no sample touched
        for (int t = max(t0, Tr); t < min(T, t0 + STFT_RUN); ++t) {
            c32* Xo = X + ((g * T + t) * (long long)F) * chans;
            for (int i = lane; i < F * chans; i += 64) Xo[i] = make_float2(0.f, 0.f);
        }
        if (t0 >= Tr) return;
    }
    const int t1 = min(Tr, t0 + STFT_RUN);
    WaveTw<N> wtw;
    wtw.init(tw, lane);
    float w[E];
    load_window_half<N>(w, win, lane);
    const float* xa[CHP];
    const float* xb[CHP];
#pragma unroll
    for (int p = 0; p < CHP; ++p) {
        xa[p] = x + (g * chans + 2 * p) * (long long)L;
        xb[p] = (2 * p + 1 < chans) ? x + (g * chans + 2 * p + 1) * (long long)L : xa[p];
    }
    c32 raw[CHP][E];
#pragma unroll
    for (int p = 0; p < CHP; ++p) load_frame_slots<N, 0, E>(raw[p], xa[p], xb[p], t0, Lr, pad_mode, lane);
    for (int t = t0; t < t1; ++t) {
        c32 nxt[CHP][EH];
        {
            const int tn = min(t + 1, Tr - 1);             // clamped: harmless reload at the end of a run
#pragma unroll
            for (int p = 0; p < CHP; ++p) load_frame_slots<N, EH, E>(nxt[p], xa[p], xb[p], tn, Lr, pad_mode, lane);
        }
        c32 A[CHP][NJ], B[CHP][NJ];
#pragma unroll
        for (int p = 0; p < CHP; ++p) {
            c32 v[E];
            apply_window<N>(v, raw[p], w, 2 * p + 1 < chans);
            fft_wave<N>(v, wtw, sh.buf[wave], lane);
            rfft_pair_untangle<N>(v, sh.buf[wave], lane, [&](int j, int, c32 a, c32 b) {
                A[p][j] = a;
                B[p][j] = b;
            });
        }
        // Consume the prefetched half-window BEFORE this frame's stores are issued: vmcnt retires in order, so a wait
        // placed after the stores would also wait for them; placed here it only covers loads (and stores of the
        // previous frame, a whole transform old).
#pragma unroll
        for (int p = 0; p < CHP; ++p)
#pragma unroll
            for (int e = 0; e < EH; ++e) {
                DISCO_CONSUME(nxt[p][e].x);
                DISCO_CONSUME(nxt[p][e].y);
                raw[p][e] = raw[p][e + EH];
                raw[p][e + EH] = nxt[p][e];
            }
        {
            c32* Xo = X + ((g * T + t) * (long long)F) * chans;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (j < NJ - 1 || lane == 0) {
                    const int f = lane + 64 * j;
                    c32* o = Xo + (long long)f * chans;
                    if ((chans & 1) == 0) {
                        float4* o4 = reinterpret_cast<float4*>(o);      // (f*chans + 2p) * 8 B is 16-B aligned
#pragma unroll
                        for (int p = 0; p < CHP; ++p) o4[p] = make_float4(A[p][j].x, A[p][j].y, B[p][j].x, B[p][j].y);
                    } else {
#pragma unroll
                        for (int p = 0; p < CHP; ++p) {
                            o[2 * p] = A[p][j];
                            if (2 * p + 1 < chans) o[2 * p + 1] = B[p][j];
                        }
                    }
                }
            }
        }
    }
}

// More than 4 channels (and N = 1024 from 3 on): k_stft<N, CHP> keeps every channel pair's window AND spectrum of a frame in
// registers (N = 1024, CHP = 4: 256 VGPRs + 214 AGPR copies, one wave per SIMD -- 7.5 ms on the C5 batch).  Here the waves of a
// workgroup split the pairs instead: wave p transforms channel pair p of the same (signal group, run of frames) and parks its
// two spectra in column p of an LDS tile laid out exactly like the frame's [F][chans] block of X; after a barrier the whole
// workgroup copies the tile out linearly (1 KiB of consecutive bytes per wave store; storing each pair's 16 bytes per bin
// straight from its wave, at a pitch of chans * 8, measured 40 % SLOWER than k_stft: four partial writes per 64-byte line).
template <int N>
struct alignas(16) StftPairsShared {
    c32 buf[STFT_WAVES][fft_buf_len<N>()];
    c32 tile[N / 2 + 1][2 * STFT_WAVES];
};
// Where the 16-byte granule (bin f, channel pair p) of the tile lives, in granules.  Lane = bin, so a wave's ds_write_b128 puts
// 16 consecutive bins at a pitch of chp granules: with chp = 4 (or 2) only 4 (8) of the 16 granule slots of a 256-byte LDS row
// are hit -- a 4-way (2-way) bank conflict on every store (round 2's counters: 41 % of the kernel's LDS cycles).  XOR-ing the
// pair index with bits of the bin spreads the 16 bins over all 16 slots; the copy-out undoes it with the same expression, and
// its 16 consecutive granules still cover 16 different slots.
__device__ __forceinline__ int pairs_tile_slot(int f, int p, int chp) {
    const int sw = chp == 4 ? ((f >> 2) & 3) : (chp == 2 ? ((f >> 3) & 1) : 0);
    return f * chp + (p ^ sw);
}
// the same for a linear granule index i = f * chp + p (the copy-out's): no division
__device__ __forceinline__ int pairs_tile_slot_linear(int i, int chp) {
    return chp == 4 ? (i ^ ((i >> 4) & 3)) : (chp == 2 ? (i ^ ((i >> 4) & 1)) : i);
}

template <int N>
__global__ DISCO_KERNEL_ALIGN __launch_bounds__(64 * STFT_WAVES, 2) void k_stft_pairs(const float* __restrict__ x, c32* __restrict__ X,
                                                                    const float* __restrict__ win, const c32* __restrict__ tw,
                                                                    int chans, int L, int T, int pad_mode, int runs_per_sig,
                                                                    const int* __restrict__ lens, int sig_per_room) {
    constexpr int E = FftPlan<N>::E, F = N / 2 + 1, NJ = E / 2 + 1, EH = E / 2;
    __shared__ StftPairsShared<N> sh;
    const int wave = wave_id(), lane = threadIdx.x & 63, tid = threadIdx.x;
    const bool mine = 2 * wave < chans;            // waves without a pair still take part in the barriers and the copy
    const bool two = 2 * wave + 1 < chans;
    const int chp = (chans + 1) / 2;
    const long long g = blockIdx.x / runs_per_sig;
    const int t0 = (int)(blockIdx.x % runs_per_sig) * STFT_RUN;
    const int Lr = room_length(lens, lens ? g / sig_per_room : 0, L), Tr = lens ? 1 + Lr / (N / 2) : T;      // see k_stft
    if (lens) {                                    // workgroup-uniform, before the first barrier
        for (int t = max(t0, Tr); t < min(T, t0 + STFT_RUN); ++t) {
            c32* Xo = X + ((g * T + t) * (long long)F) * chans;
            for (int i = tid; i < F * chans; i += 64 * STFT_WAVES) Xo[i] = make_float2(0.f, 0.f);
        }
        if (t0 >= Tr) return;
    }
    const int t1 = min(Tr, t0 + STFT_RUN);
    WaveTw<N> wtw;
    wtw.init(tw, lane);
    float w[E];
    load_window_half<N>(w, win, lane);
    const float* xa = x + (g * chans + (mine ? 2 * wave : 0)) * (long long)L;
    const float* xb = two ? xa + L : xa;
    c32 raw[E];
    load_frame_slots<N, 0, E>(raw, xa, xb, t0, Lr, pad_mode, lane);
    c32* tile = &sh.tile[0][0];                    // row pitch 2 * chp: the frame's X block when chans is even
    for (int t = t0; t < t1; ++t) {
        c32 nxt[EH];
        load_frame_slots<N, EH, E>(nxt, xa, xb, min(t + 1, Tr - 1), Lr, pad_mode, lane);
        if (mine) {
            c32 v[E];
            apply_window<N>(v, raw, w, two);
            fft_wave<N>(v, wtw, sh.buf[wave], lane);
            rfft_pair_untangle<N>(v, sh.buf[wave], lane, [&](int, int f, c32 a, c32 b) {
                *reinterpret_cast<float4*>(&tile[pairs_tile_slot(f, wave, chp) * 2]) = make_float4(a.x, a.y, b.x, b.y);
            });
        }
#pragma unroll
        for (int e = 0; e < EH; ++e) {                 // consume the prefetch before the stores (see k_stft)
            DISCO_CONSUME(nxt[e].x);
            DISCO_CONSUME(nxt[e].y);
            raw[e] = raw[e + EH];
            raw[e + EH] = nxt[e];
        }
        __syncthreads();
        c32* Xo = X + ((g * T + t) * (long long)F) * chans;
        if ((chans & 1) == 0) {
            const float4* src = reinterpret_cast<const float4*>(tile);
            float4* dst = reinterpret_cast<float4*>(Xo);
            const int shift = (int)((reinterpret_cast<unsigned long long>(dst) >> 4) & 7);      // whole 128-byte lines per wave store (see k_stft_cov)
            for (int i = tid - shift; i < F * chp; i += 64 * STFT_WAVES)
                if (i >= 0) store_stream16(&dst[i], src[pairs_tile_slot_linear(i, chp)]);
        } else {
            for (int i = tid; i < F * chans; i += 64 * STFT_WAVES) {
                const int f = i / chans, c = i % chans;
                Xo[i] = tile[pairs_tile_slot(f, c >> 1, chp) * 2 + (c & 1)];
            }
        }
        __syncthreads();                               // the tile is rewritten by the next frame
    }
}

// tf_mask (dnn/utils.py:57-67) on one bin, right wherever the reference's float32 arithmetic is: over the whole float32 range of the
// inputs, with inf and NaN where np.abs / the float32 division put them and nowhere else.
__device__ __forceinline__ float ipow(float r, int p) {
    float m = r;
    for (int i = 1; i < p; ++i) m *= r;
    return p == 0 ? 1.f : m;
}
// |z| as np.abs(complex64) (a hypot): both parts are scaled by the power of two of the larger one before they are squared, so the
// sum of squares stays in [1/4, 2) -- no overflow above 1.8e19, no underflow below 1e-19, and v_sqrt_f32 (1 ulp, flushes
// denormals) never sees a denormal.  The scaling is exact; inf stays inf, a NaN part gives NaN, |0| = 0.  The larger part is squared
// first, so |S| and |i S| are one number however the compiler contracts the sum.
__device__ __forceinline__ float cmag(c32 z) {
    const float a = fabsf(z.x), b = fabsf(z.y);
    const bool sw = a < b;                                          // not fmaxf / fminf: they would drop a NaN part
    const float hi = sw ? b : a, lo = sw ? a : b;
    int e;
    (void)frexpf(hi, &e);                                           // 0 for 0, inf and NaN
    const float x = ldexpf(hi, -e), y = ldexpf(lo, -e);
    return ldexpf(__builtin_amdgcn_sqrtf(x * x + y * y), e);        // overflows to inf where the reference's hypot does
}
__device__ __forceinline__ float tf_mask_value(c32 S, c32 Nn, int mask_type, int mask_pow, float thr_lin) {
    const c32 O = mask_type == DISCO_MASK_IAM ? cadd(S, Nn) : Nn;           // the denominator: |S + N| or |N|
    const float ss = S.x * S.x + S.y * S.y, so = O.x * O.x + O.y * O.y;
    // The plain route -- v_sqrt_f32 of the sum of squares, v_rcp_f32 (1 ulp each) -- where both sums of squares lie within 2^+-100: no
    // overflow, no underflow, no denormal reaches either instruction, the EPS clamp (2^-52 < 2^-50) cannot bind, the quotient is normal.
    // Everywhere else, and for 'ibm' always: the scaled magnitudes and an IEEE division, the reference's own -- v_rcp_f32 flushes a denormal
    // reciprocal (|N| above 8.5e37) to zero, and its 1-ulp error decides an exact tie |S| = |N| of 'ibm' either way (a quarter of them wrongly).
    float q;
    if (mask_type != DISCO_MASK_IBM && fminf(ss, so) >= 0x1p-100f && fmaxf(ss, so) <= 0x1p100f) {
        q = __builtin_amdgcn_sqrtf(ss) * __builtin_amdgcn_rcpf(__builtin_amdgcn_sqrtf(so));
    } else {
        float ao = cmag(O);
        if (mask_type != DISCO_MASK_IAM) ao = ao < 2.220446049250313e-16f ? 2.220446049250313e-16f : ao;      // np.maximum: a NaN stays a NaN
        q = cmag(S) / ao;
    }
    const float xi = ipow(q, mask_pow);
    if (mask_type == DISCO_MASK_IAM) return xi;
    if (mask_type == DISCO_MASK_IBM) return xi >= thr_lin ? 1.f : 0.f;
    // xi / (1 + xi); an overflowing xi gives NaN exactly like the reference's inf / inf.  Beyond 2^64 the quotient rounds to 1, and
    // the reciprocal of 1 + xi would be flushed from 2^126 on: (xi - xi) + 1 is 1 for a finite xi and NaN for inf
    return xi > 0x1p64f ? (xi - xi) + 1.f : xi * __builtin_amdgcn_rcpf(1.f + xi);
}

// s_ref, n_ref: [n_sig][L] -> mask [n_sig][T][F]; the pair (s, n) shares one complex FFT.  Streams like k_stft.
template <int N>
__global__ DISCO_KERNEL_ALIGN __launch_bounds__(64 * STFT_WAVES) void k_mask_oracle(const float* __restrict__ s_ref, const float* __restrict__ n_ref,
                                                                  float* __restrict__ mask, const float* __restrict__ win,
                                                                  const c32* __restrict__ tw, int L, int T, int pad_mode,
                                                                  int mask_type, int mask_pow, float thr_lin, int runs_per_sig,
                                                                  long long n_witems, const int* __restrict__ lens, int sig_per_room) {
    constexpr int E = FftPlan<N>::E, F = N / 2 + 1, EH = E / 2;
    __shared__ StftShared<N> sh;
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * STFT_WAVES + wave;
    if (item >= n_witems) return;
    const long long g = item / runs_per_sig;
    const int t0 = (int)(item % runs_per_sig) * STFT_RUN;
    const int Lr = room_length(lens, lens ? g / sig_per_room : 0, L), Tr = lens ? 1 + Lr / (N / 2) : T;      // see k_stft
    if (lens) {                                    // the mask of a frame that does not exist is FORCED to zero ('iam' there is 0 / 0)
        for (int t = max(t0, Tr); t < min(T, t0 + STFT_RUN); ++t) {
            float* mo = mask + (g * T + t) * (long long)F;
            for (int i = lane; i < F; i += 64) mo[i] = 0.f;
        }
        if (t0 >= Tr) return;
    }
    const int t1 = min(Tr, t0 + STFT_RUN);
    WaveTw<N> wtw;
    wtw.init(tw, lane);
    float w[E];
    load_window_half<N>(w, win, lane);
    const float* xs = s_ref + g * (long long)L;
    const float* xn = n_ref + g * (long long)L;
    c32 raw[E];
    load_frame_slots<N, 0, E>(raw, xs, xn, t0, Lr, pad_mode, lane);
    for (int t = t0; t < t1; ++t) {
        c32 nxt[EH];
        load_frame_slots<N, EH, E>(nxt, xs, xn, min(t + 1, Tr - 1), Lr, pad_mode, lane);
        c32 v[E];
        apply_window<N>(v, raw, w, true);
        fft_wave<N>(v, wtw, sh.buf[wave], lane);
        float mval[EH + 1];
        rfft_pair_untangle<N>(v, sh.buf[wave], lane, [&](int j, int, c32 a, c32 b) {
            mval[j] = tf_mask_value(a, b, mask_type, mask_pow, thr_lin);
        });
#pragma unroll
        for (int e = 0; e < EH; ++e) {                 // consume the prefetch before the stores (see k_stft)
            DISCO_CONSUME(nxt[e].x);
            DISCO_CONSUME(nxt[e].y);
            raw[e] = raw[e + EH];
            raw[e + EH] = nxt[e];
        }
        float* mo = mask + (g * T + t) * (long long)F;
#pragma unroll
        for (int j = 0; j <= EH; ++j)
            if (j < EH || lane == 0) store_stream4(&mo[lane + 64 * j], mval[j]);
    }
}

// A meeting room of S talkers (get_masks, gen_meetit/convolve_signals.py:166-188): img [S][n_sig][L] -> masks [S][n_sig][T][F], mask i the
// tf_mask of talker i's image against the sum of the others, and optionally mix [n_sig][T][F], the spectrum of the sum of all images.
// With X_j the spectrum of image j: mix = ((X_0 + X_1) + X_2) + ..., N_i = the sum over j != i in ascending j (the transform is linear: the
// reference transforms the time-domain sums, the difference is rounding).  Streams like k_mask_oracle, with k_stft's register plan:
// talkers 2p and 2p + 1 share complex FFT p, NP = ceil(S / 2) transforms per frame (the last talker of an odd S rides alone, its partner
// slot is never read), and all S spectra of the frame stay in registers until its masks are stored -- no spectrum reaches memory but mix.
// PREFETCH: the next frame's new half-windows are requested before the transforms, as in k_mask_oracle; without it (the widest plans,
// where those registers are not to be had) after them.  The rules of per-room lengths are k_mask_oracle's.
constexpr bool source_masks_prefetch(int n, int np) { return n * np <= 2048; }
template <int N, int NP, bool PREFETCH>
__global__ DISCO_KERNEL_ALIGN __launch_bounds__(64 * STFT_WAVES) void k_source_masks(const float* __restrict__ img, float* __restrict__ masks,
                                                                   c32* __restrict__ mix, const float* __restrict__ win,
                                                                   const c32* __restrict__ tw, int S, long long n_sig, int L, int T,
                                                                   int pad_mode, int mask_type, int mask_pow, float thr_lin,
                                                                   int runs_per_sig, long long n_witems, const int* __restrict__ lens,
                                                                   int sig_per_room) {
    constexpr int E = FftPlan<N>::E, F = N / 2 + 1, EH = E / 2;
    __shared__ StftShared<N> sh;
    const int wave = wave_id(), lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * STFT_WAVES + wave;
    if (item >= n_witems) return;
    const long long g = item / runs_per_sig;
    const int t0 = (int)(item % runs_per_sig) * STFT_RUN;
    const int Lr = room_length(lens, lens ? g / sig_per_room : 0, L), Tr = lens ? 1 + Lr / (N / 2) : T;      // see k_stft
    if (lens) {                                    // frames the room does not have: masks and mix FORCED to zero, no sample touched
        for (int t = max(t0, Tr); t < min(T, t0 + STFT_RUN); ++t) {
            for (int i = 0; i < S; ++i) {
                float* mo = masks + ((i * n_sig + g) * T + t) * (long long)F;
                for (int f = lane; f < F; f += 64) mo[f] = 0.f;
            }
            if (mix) {
                c32* xo = mix + (g * T + t) * (long long)F;
                for (int f = lane; f < F; f += 64) xo[f] = make_float2(0.f, 0.f);
            }
        }
        if (t0 >= Tr) return;
    }
    const int t1 = min(Tr, t0 + STFT_RUN);
    WaveTw<N> wtw;
    wtw.init(tw, lane);
    float w[E];
    load_window_half<N>(w, win, lane);
    const float* xa[NP];
    const float* xb[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        xa[p] = img + ((2 * p) * n_sig + g) * (long long)L;
        xb[p] = (2 * p + 1 < S) ? img + ((2 * p + 1) * n_sig + g) * (long long)L : xa[p];
    }
    c32 raw[NP][E];
#pragma unroll
    for (int p = 0; p < NP; ++p) load_frame_slots<N, 0, E>(raw[p], xa[p], xb[p], t0, Lr, pad_mode, lane);
    for (int t = t0; t < t1; ++t) {
        const int tn = min(t + 1, Tr - 1);                 // clamped: harmless reload at the end of a run
        c32 nxt[NP][EH];
        if constexpr (PREFETCH) {
#pragma unroll
            for (int p = 0; p < NP; ++p) load_frame_slots<N, EH, E>(nxt[p], xa[p], xb[p], tn, Lr, pad_mode, lane);
        }
        c32 X[2 * NP][EH + 1];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            c32 v[E];
            apply_window<N>(v, raw[p], w, 2 * p + 1 < S);
            fft_wave<N>(v, wtw, sh.buf[wave], lane);
            rfft_pair_untangle<N>(v, sh.buf[wave], lane, [&](int j, int, c32 a, c32 b) {
                X[2 * p][j] = a;
                X[2 * p + 1][j] = b;
            });
        }
        if constexpr (!PREFETCH) {
#pragma unroll
            for (int p = 0; p < NP; ++p) load_frame_slots<N, EH, E>(nxt[p], xa[p], xb[p], tn, Lr, pad_mode, lane);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int e = 0; e < EH; ++e) {                 // consume the new half-windows before the stores (see k_stft)
                DISCO_CONSUME(nxt[p][e].x);
                DISCO_CONSUME(nxt[p][e].y);
                raw[p][e] = raw[p][e + EH];
                raw[p][e + EH] = nxt[p][e];
            }
        // the masks of the frame, talker by talker; slot EH (the Nyquist bin) is valid in lane 0 alone
#pragma unroll
        for (int i = 0; i < 2 * NP; ++i) {
            if (i < S) {                                   // wave-uniform
                float* mo = masks + ((i * n_sig + g) * T + t) * (long long)F;
#pragma unroll
                for (int j = 0; j <= EH; ++j) {
                    c32 others = X[i == 0 ? 1 : 0][j];
#pragma unroll
                    for (int q = (i == 0 ? 2 : 1); q < 2 * NP; ++q)
                        if (q != i && q < S) others = cadd(others, X[q][j]);
                    const float m = tf_mask_value(X[i][j], others, mask_type, mask_pow, thr_lin);
                    if (j < EH || lane == 0) store_stream4(&mo[lane + 64 * j], m);
                }
            }
        }
        if (mix) {
            c32* xo = mix + (g * T + t) * (long long)F;
#pragma unroll
            for (int j = 0; j <= EH; ++j) {
                c32 sum = X[0][j];
#pragma unroll
                for (int i = 1; i < 2 * NP; ++i)
                    if (i < S) sum = cadd(sum, X[i][j]);
                if (j < EH || lane == 0) xo[lane + 64 * j] = sum;
            }
        }
    }
}

// element i of a [n_sig][T][F] array lies in a frame its room does not have (per-room lengths; hop = F - 1)
__device__ __forceinline__ bool tf_beyond_room(const int* __restrict__ lens, long long i, int T, int F, int sig_per_room) {
    const long long gt = i / F;
    return (int)(gt % T) >= 1 + lens[(gt / T) / sig_per_room] / (F - 1);
}

// lens (per-room lengths, nullptr: none): the masks of [n_sig][T][F] arrays are forced to zero in the frames beyond a room's clip
static __global__ void k_tf_mask(const c32* __restrict__ S, const c32* __restrict__ Nn, float* __restrict__ mask,
                          long long n, int mask_type, int mask_pow, float thr_lin, const int* __restrict__ lens, int T, int F,
                          int sig_per_room) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float m = tf_mask_value(S[i], Nn[i], mask_type, mask_pow, thr_lin);
        mask[i] = (lens && tf_beyond_room(lens, i, T, F, sig_per_room)) ? 0.f : m;
    }
}

static __global__ void k_tf_mask_channel(const c32* __restrict__ S, const c32* __restrict__ Nn, float* __restrict__ mask, long long n, int M,
                                  int ch, int mask_type, int mask_pow, float thr_lin, const int* __restrict__ lens, int T, int F,
                                  int sig_per_room) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float m = tf_mask_value(S[i * M + ch], Nn[i * M + ch], mask_type, mask_pow, thr_lin);
        mask[i] = (lens && tf_beyond_room(lens, i, T, F, sig_per_room)) ? 0.f : m;
    }
}

// ---- iSTFT --------------------------------------------------------------------------------------------
// Z: [n_sig][T][F] -> out: [n_sig][L].  A block owns ISTFT_FRAMES consecutive frames of one signal (each wave
// inverts two frames with one complex FFT), overlap-adds them in LDS and emits the ISTFT_FRAMES - 1 hop
// segments that are complete inside the block; consecutive blocks overlap by one frame.
constexpr int ISTFT_FRAMES = 2 * STFT_WAVES;
constexpr int ISTFT_SEGS = ISTFT_FRAMES - 1;

template <int N>
struct IstftShared {
    float win[N];
    c32 buf[STFT_WAVES][fft_buf_len<N>()];     // after the transform each wave parks its two time frames here
};
template <int N>
__device__ __forceinline__ float* istft_frame(IstftShared<N>& sh, int j) {
    return reinterpret_cast<float*>(sh.buf[j >> 1]) + (j & 1) * N;
}

// SOLO: every wave inverts ONE frame per transform (the second slot of the pair stays empty) and a block owns STFT_WAVES frames.  Twice the
// transforms -- but a frame's samples then depend on its own spectrum only, not at rounding level on the partner it shared a transform
// with, which is what lets the STREAMING online path (disco_tango_online_stream) reproduce the whole-clip call bit for bit whatever the
// chunking: both online entry points invert this way (their overlap-add is 1 % of their time).
template <int N, bool SOLO = false>
__global__ DISCO_KERNEL_ALIGN __launch_bounds__(64 * STFT_WAVES) void k_istft(const c32* __restrict__ Z, float* __restrict__ out,
                                                            const float* __restrict__ win, const c32* __restrict__ tw,
                                                            int L, int T, int blocks_per_sig, const int* __restrict__ lens,
                                                            int sig_per_room) {
    constexpr int E = FftPlan<N>::E, F = N / 2 + 1, H = N / 2;
    constexpr int SEGS = SOLO ? STFT_WAVES - 1 : ISTFT_SEGS;
    __shared__ IstftShared<N> sh;
    for (int i = threadIdx.x; i < N; i += blockDim.x) sh.win[i] = win[i];
    const int wave = wave_id(), lane = threadIdx.x & 63;
    WaveTw<N> wtw;
    wtw.init(tw, lane);
    const long long g = blockIdx.x / blocks_per_sig;
    const int seg0 = (int)(blockIdx.x % blocks_per_sig) * SEGS;             // first output segment == first frame
    // L, T: the pitch of the arrays; Lr, Tr: the room's own clip (disco_set_lengths): its window sum is that of Tr frames, samples
    // at and beyond Lr are exact zeros
    const int Lr = room_length(lens, lens ? g / sig_per_room : 0, L), Tr = lens ? 1 + Lr / H : T;
    if (lens && seg0 >= Tr) {                      // (workgroup-uniform) nothing of this block exists: zeros, no spectrum touched
        float* oz = out + g * (long long)L;
        for (int i = threadIdx.x; i < SEGS * H; i += blockDim.x) {
            const long long pos = (long long)seg0 * H + i;
            if (pos < L) oz[pos] = 0.f;
        }
        return;
    }
    const int ta = SOLO ? seg0 + wave : seg0 + 2 * wave, tb = ta + 1;
    const c32* Za = Z + (g * T + ta) * (long long)F;
    const c32* Zb = Z + (g * T + tb) * (long long)F;
    const bool has_a = ta < Tr, has_b = !SOLO && tb < Tr;
    // V[n] = A~[n] + i B~[n] with A~, B~ the Hermitian extensions; the inverse transform is conj(FFT(conj V)) / N
    c32 v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int n = lane + 64 * e;
        const bool upper = n > N / 2;
        const int f = upper ? N - n : n;
        c32 a = has_a ? Za[f] : make_float2(0.f, 0.f);
        c32 b = has_b ? Zb[f] : make_float2(0.f, 0.f);
        if (f == 0 || f == N / 2) {      // irfft ignores the imaginary part of DC and Nyquist
            a.y = 0.f;
            b.y = 0.f;
        }
        if (upper) {
            a.y = -a.y;
            b.y = -b.y;
        }
        const c32 V = make_float2(a.x - b.y, a.y + b.x);
        v[e] = cconj(V);
    }
    fft_wave<N>(v, wtw, sh.buf[wave], lane);
    const float inv = 1.0f / N;
    __syncthreads();                                   // sh.win is loaded; every lane is past its last read of buf[wave]
    // frame slot of block-local frame j: SOLO keeps one frame per wave buffer, else two
    auto frame = [&](int j) { return SOLO ? reinterpret_cast<float*>(sh.buf[j]) : istft_frame<N>(sh, j); };
    float* fa = frame(SOLO ? wave : 2 * wave);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int n = lane + 64 * e;
        const float w = sh.win[n] * inv;
        fa[n] = v[e].x * w;                            // Re(conj(out)) =  out.x
        if constexpr (!SOLO) frame(2 * wave + 1)[n] = -v[e].y * w;       // Im(conj(out)) = -out.y
    }
    __syncthreads();
    float* o = out + g * (long long)L;
    for (int i = threadIdx.x; i < SEGS * H; i += blockDim.x) {
        const int j = i / H, n = i - j * H;
        const int seg = seg0 + j;
        const long long pos = (long long)seg * H + n;
        if (seg < T && pos < L) {
            const float w0 = sh.win[H + n], w1 = sh.win[n];
            float wss = w0 * w0;
            if (seg + 1 < Tr) wss += w1 * w1;
            float val = frame(j)[H + n] + frame(j + 1)[n];
            if (wss > 1.17549435e-38f) val /= wss;
            o[pos] = (lens && pos >= Lr) ? 0.f : val;
        }
    }
}

}  // namespace disco

namespace disco {

// ---- STFT + step-1 covariance in one pass over the samples ---------------------------------------------------
// tango.py:335 + 357-364: the spectra are needed twice right away (stored for step 2, and reduced into the local
// covariances), so the 4 waves of a workgroup stream 4 interleaved runs of frames of one node, park each
// frame's transforms (one per channel pair) in an LDS tile, and after a barrier the workgroup switches to one-thread-per-bin:
// every thread copies its share of the frame to X (coalesced 16-byte-per-lane wave stores) and folds its bin's M-vector into the
// P(P+1)/2 covariance accumulators it keeps in registers for the whole run.  Saves the separate covariance
// pass over X (8*M*F bytes per node-frame).
// frames per wave per workgroup are a launch parameter (`runw`; a workgroup covers 4 * runw frames): long runs amortise the
// first-frame load and the partial-sum write-out (80 is best at C3), short ones keep small batches spread over the chip

// The tile holds Z planes: the transform waves park the raw pair spectra Z (natural order, one conflict-free ds_write_b64 per slot) and
// whoever picks a bin up separates the two channels himself -- A = Z[f] + conj Z[N - f], B = -i (Z[f] - conj Z[N - f]): the very operations
// of rfft_pair_untangle on the very operands, so every spectrum and every sum is bit for bit what a tile of untangled rows would give.
// Against such a tile it saves, per transform, the 2 E ds_bpermute of the untangle and E/2 ds_write_b128 at a 32-byte pitch: ~280 -> ~180
// LDS cycles on the pipe that, with the VALU, bounds the STORE = false variant (profiles/r03_q_C2x4000_pmc_alu.json), and the untangle's
// registers in the phase that sets this kernel's register count.  (A swizzled tile like k_stft_pairs' was measured 8 % slower here.)
// ZPITCH: pitch of a pair plane: N + 16 complex, i.e. consecutive planes start 32 banks apart, so the copy-out's ds_read_b64 --
// consecutive lanes alternate between the planes of one bin -- never meet on a bank
template <int N>
constexpr int stft_cov_zpitch() { return N + 16; }
template <int N, int CHP>
struct alignas(16) StftCovShared {
    c32 buf[STFT_WAVES][fft_buf_len<N>()];
    c32 tile[STFT_WAVES][CHP * stft_cov_zpitch<N>()];
};

// 3 waves per SIMD (<= 168 VGPRs) is reachable for the common 512-point, M <= 4 shape and worth ~3 %; larger shapes keep
// whatever occupancy their register need allows
#ifndef DISCO_SC_WPE
#define DISCO_SC_WPE 3
#endif
// STORE = false: the spectra are reduced into the covariances and dropped (single-node path: the filter pass recomputes them
// from the samples, k_stft_apply_istft, instead of reading 8 M F bytes per node-frame back)
// PACK: the workspace layout of the whole path's fused route -- rows of F - 1 = N / 2 bins, [T][N / 2][M]: slot 0 of channel i holds
// (Re X[0][i], Re X[N / 2][i]).  DC and Nyquist of a real frame are real (the untangle gives their imaginary parts as exact zeros), so
// nothing is lost, and a row is 4 N M bytes -- a whole number of 128-byte lines, where the public row (8 M F bytes) starts 0 / 32 / 64 /
// 96 bytes into a line.  Only the addresses of the copy-out differ: the fold reads the LDS tile and forms the same sums in the same order.
template <int N, int M, bool STORE = true, bool PACK = false>
__global__ DISCO_KERNEL_ALIGN __launch_bounds__(64 * STFT_WAVES, (N == 512 && M <= 4) ? DISCO_SC_WPE : 1) void k_stft_cov(const float* __restrict__ x, const float* __restrict__ mask,
                                                               c32* __restrict__ X, float4* __restrict__ part,
                                                               const float* __restrict__ win, const c32* __restrict__ tw,
                                                               int L, int T, int pad_mode, int chunks, int runw,
                                                               const int* __restrict__ lens, int sig_per_room, int zero_beyond) {
    static_assert(STFT_WAVES == 4, "one bin per thread needs 4 waves for 256 bins");
    constexpr int E = FftPlan<N>::E, F = N / 2 + 1, EH = E / 2, CHP = (M + 1) / 2, MP = 2 * CHP;
    constexpr int NP = M * (M + 1) / 2;
    constexpr int FX = PACK ? F - 1 : F;           // bins of a stored row
    constexpr int BPT = (F - 1) / 256;             // bins per thread: 1 (N = 512) or 2 (N = 1024)
    constexpr int ZP = stft_cov_zpitch<N>();
    __shared__ StftCovShared<N, CHP> sh;
    // plane (frame of wave ww, pair p) = Z[0 .. N)
    auto zplane = [&](int ww, int p) { return &sh.tile[ww][p * ZP]; };
    const int tid = threadIdx.x, wave = wave_id(), lane = tid & 63;
    const long long g = blockIdx.x / chunks;
    const int c = (int)(blockIdx.x % chunks);
    const int tb = c * STFT_WAVES * runw;
    const int ts = tb + wave * runw;
    // L, T: the pitch of the arrays; Lr, Tr: the room's own clip (disco_set_lengths; the same without lengths).  Frames at or beyond Tr
    // enter no sum and, stored, are exact zeros; their samples and masks are never read.
    const int Lr = room_length(lens, lens ? g / sig_per_room : 0, L), Tr = lens ? 1 + Lr / (N / 2) : T;
    if (lens) {                                    // (workgroup-uniform, before the first barrier)
        const int tz0 = max(tb, Tr), tz1 = min(T, tb + STFT_WAVES * runw);
        // the frames of this chunk the room does not have: zeros, unless every reader of X knows the lengths itself (zero_beyond = 0: the
        // fused route of the whole path, where X never leaves the workspace -- the zeros would cost what the spectra cost to store)
        if (STORE && zero_beyond && tz0 < tz1) {
            c32* Xz = X + ((g * T + tz0) * (long long)FX) * M;
            const long long nz = (long long)(tz1 - tz0) * FX * M;
            for (long long i = tid; i < nz; i += 64 * STFT_WAVES) Xz[i] = make_float2(0.f, 0.f);
        }
        if (tb >= Tr) {                            // a chunk wholly in the padding: zero sums, no sample or mask touched
            float4* oz = part + ((g * chunks + c) * F) * (long long)NP;
            for (int i = tid; i < F * NP; i += 64 * STFT_WAVES) oz[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            return;
        }
    }
    const int te = min(Tr, ts + runw);
    WaveTw<N> wtw;
    wtw.init(tw, lane);
    float w[E];
    load_window_half<N>(w, win, lane);
    const float* xa[CHP];
    const float* xb[CHP];
#pragma unroll
    for (int p = 0; p < CHP; ++p) {
        xa[p] = x + (g * M + 2 * p) * (long long)L;
        xb[p] = (2 * p + 1 < M) ? x + (g * M + 2 * p + 1) * (long long)L : xa[p];
    }
    c32 raw[CHP][E];
#pragma unroll
    for (int p = 0; p < CHP; ++p) {
        if (ts < te) load_frame_slots<N, 0, E>(raw[p], xa[p], xb[p], ts, Lr, pad_mode, lane);
        else {
#pragma unroll
            for (int e = 0; e < E; ++e) raw[p][e] = make_float2(0.f, 0.f);
        }
    }
    c32 acc_s[BPT][NP], acc_n[BPT][NP];
#pragma unroll
    for (int b = 0; b < BPT; ++b)
#pragma unroll
        for (int q = 0; q < NP; ++q) acc_s[b][q] = acc_n[b][q] = make_float2(0.f, 0.f);
    // Nyquist bin: thread (q, which) with tid < 2*NP owns one complex entry of Rss (which = 0) or Rnn (1)
    c32 acc_ny = make_float2(0.f, 0.f);
    int ny_i = 0, ny_j = 0;
    {
        int q = tid >> 1, i = 0;
        while (i < M - 1 && q >= M - i) {
            q -= M - i;
            ++i;
        }
        ny_i = i;
        ny_j = i + q;
    }
    const float* mg = mask + g * T * (long long)F;
    for (int it = 0; it < runw; ++it) {
        const int t = ts + it;
        const bool valid = t < te;
        // masks of the 4 frames this thread will reduce after the barrier (requested early)
        float mv[STFT_WAVES][BPT], mny[STFT_WAVES];
#pragma unroll
        for (int ww = 0; ww < STFT_WAVES; ++ww) {
            const int t2 = min(tb + ww * runw + it, Tr - 1);         // clamped: unconditional loads, used only when valid
#pragma unroll
            for (int b = 0; b < BPT; ++b) mv[ww][b] = mg[(long long)t2 * F + tid + 256 * b];
            mny[ww] = mg[(long long)t2 * F + F - 1];
        }
        c32 nxt[CHP][EH];
        {
            const int tn = min(t + 1, Tr - 1);             // clamped: harmless reload at the end of a run
#pragma unroll
            for (int p = 0; p < CHP; ++p) load_frame_slots<N, EH, E>(nxt[p], xa[p], xb[p], tn, Lr, pad_mode, lane);
        }
        if (valid) {
#pragma unroll
            for (int p = 0; p < CHP; ++p) {
                c32 v[E];
                apply_window<N>(v, raw[p], w, 2 * p + 1 < M);
                fft_wave<N>(v, wtw, sh.buf[wave], lane);
                c32* zp = zplane(wave, p);
#pragma unroll
                for (int e = 0; e < E; ++e) zp[lane + 64 * e] = v[e];
            }
        }
#pragma unroll
        for (int p = 0; p < CHP; ++p)                   // consume the prefetch before the X stores below (see k_stft)
#pragma unroll
            for (int e = 0; e < EH; ++e) {
                DISCO_CONSUME(nxt[p][e].x);
                DISCO_CONSUME(nxt[p][e].y);
                raw[p][e] = raw[p][e + EH];
                raw[p][e + EH] = nxt[p][e];
            }
        __syncthreads();
        // ---- one thread per bin: copy out + reduce the (up to) 4 frames of this iteration
#pragma unroll
        for (int ww = 0; ww < STFT_WAVES; ++ww) {
            const int t2 = tb + ww * runw + it;
            if (t2 < min(Tr, tb + (ww + 1) * runw)) {         // workgroup-uniform
                c32* Xo = STORE ? X + ((g * T + t2) * (long long)FX) * M : nullptr;
                if constexpr (STORE && PACK && (M & 1) == 0) {
                    // packed rows begin on a line: a plain linear copy of (F - 1) * M / 2 granules; the granules of bin 0 carry the
                    // Nyquist bin's real parts where the (zero) imaginary parts of DC would go
                    float4* dst = reinterpret_cast<float4*>(Xo);
                    for (int i = tid; i < (F - 1) * CHP; i += 64 * STFT_WAVES) {
                        const int f = i / CHP, pp = i - f * CHP;
                        const c32* zp = zplane(ww, pp);
                        const c32 z = zp[f], zc = zp[(N - f) & (N - 1)];
                        const c32 a = cadd_conj(z, zc), b = csub_conj_mi(z, zc);
                        float4 q4 = make_float4(a.x, a.y, b.x, b.y);
                        if (f == 0) {
                            const c32 zq = zp[N / 2];
                            q4.y = cadd_conj(zq, zq).x;
                            q4.w = csub_conj_mi(zq, zq).x;
                        }
                        store_stream16(&dst[i], q4);
                    }
                } else if (STORE && (M & 1) == 0) {
                    // even M: the X row is F * CHP granules of 16 bytes, one per lane (granule i = bin i / CHP, pair i % CHP, untangled on
                    // the way out), so every wave store covers 1 KiB of consecutive bytes (a per-bin store would touch each 128-B line twice)
                    // The rows are 8 * M * F bytes long (8224 for M = 4), so they start 0 / 32 / 64 / 96 bytes into a 128-byte line: the
                    // copy is shifted by that much, every wave store then covers whole lines (PMC: stores that straddle lines
                    // at both ends cost a fill read per partial line, +2.8 GB of reads per C3 launch).
                    float4* dst = reinterpret_cast<float4*>(Xo);
                    const int shift = (int)((reinterpret_cast<unsigned long long>(dst) >> 4) & 7);
                    for (int i = tid - shift; i < F * CHP; i += 64 * STFT_WAVES)
                        if (i >= 0) {
                            const int f = i / CHP, pp = i - f * CHP;
                            const c32* zp = zplane(ww, pp);
                            const c32 z = zp[f], zc = zp[(N - f) & (N - 1)];
                            const c32 a = cadd_conj(z, zc), b = csub_conj_mi(z, zc);
                            store_stream16(&dst[i], make_float4(a.x, a.y, b.x, b.y));
                        }
                }
#pragma unroll
                for (int b = 0; b < BPT; ++b) {
                    const int f = tid + 256 * b;
                    c32 xv[MP];
#pragma unroll
                    for (int p = 0; p < CHP; ++p) {
                        const c32* zp = zplane(ww, p);
                        const c32 z = zp[f], zc = zp[(N - f) & (N - 1)];
                        xv[2 * p] = cadd_conj(z, zc);
                        xv[2 * p + 1] = csub_conj_mi(z, zc);
                    }
                    if (STORE && (M & 1) != 0) {
                        if (PACK && f == 0) {           // the real parts only: the other half of slot 0 is the Nyquist threads' (below)
#pragma unroll
                            for (int i = 0; i < M; ++i) reinterpret_cast<float*>(Xo)[2 * i] = xv[i].x;
                        } else {
#pragma unroll
                            for (int i = 0; i < M; ++i) Xo[(long long)f * M + i] = xv[i];
                        }
                    }
                    const float m = mv[ww][b], mc = 1.f - m;
                    cov_accumulate_shared<M>(xv, m * m, mc * mc, acc_s[b], acc_n[b]);
                }
                // Nyquist bin
                if (STORE && (M & 1) != 0 && tid < M) {
                    const c32 zq = zplane(ww, tid >> 1)[N / 2];
                    const c32 xq = (tid & 1) ? csub_conj_mi(zq, zq) : cadd_conj(zq, zq);
                    if constexpr (PACK) reinterpret_cast<float*>(Xo)[2 * tid + 1] = xq.x;
                    else Xo[(long long)(F - 1) * M + tid] = xq;
                }
                if (tid < 2 * NP) {
                    const float m = (tid & 1) ? 1.f - mny[ww] : mny[ww];
                    // channel i of the Nyquist bin from its pair's Z[N / 2] (its own partner)
                    const c32 zi = zplane(ww, ny_i >> 1)[N / 2], zj = zplane(ww, ny_j >> 1)[N / 2];
                    const c32 a = (ny_i & 1) ? csub_conj_mi(zi, zi) : cadd_conj(zi, zi);
                    const c32 b2 = (ny_j & 1) ? csub_conj_mi(zj, zj) : cadd_conj(zj, zj);
                    const float m2 = m * m;
                    acc_ny.x = fmaf(m2, a.x * b2.x + a.y * b2.y, acc_ny.x);
                    if (ny_i != ny_j) acc_ny.y = fmaf(m2, a.y * b2.x - a.x * b2.y, acc_ny.y);
                }
            }
        }
        __syncthreads();
    }
    float4* o = part + ((g * chunks + c) * F) * (long long)NP;
#pragma unroll
    for (int b = 0; b < BPT; ++b)
#pragma unroll
        for (int q = 0; q < NP; ++q)
            o[(long long)(tid + 256 * b) * NP + q] = make_float4(acc_s[b][q].x, acc_s[b][q].y, acc_n[b][q].x, acc_n[b][q].y);
    if (tid < 2 * NP) {
        float2* o2 = reinterpret_cast<float2*>(o + (long long)(F - 1) * NP + (tid >> 1));
        o2[tid & 1] = acc_ny;
    }
}

}  // namespace disco
