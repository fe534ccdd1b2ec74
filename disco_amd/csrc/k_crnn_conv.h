// First block of the CRNN's convolutional stack in ONE pass (dnn/models/crnn.py:9-52 via nn_structures.py CNN2d; tango.py:124-129):
//     Conv2d(C_in -> C_out, 3x3, padding (0, 1))  [BatchNorm2d folded into w, b by the caller]  ->  MaxPool2d((1, 4))
//     out[b][o][t][q] = b[o] + max_{j < 4} sum_{c, kt, kf} w[o][c][kt][kf] x[b][c][t + kt][4 q + j + kf - 1]      (x = 0 outside [0, F))
// The first block has 1 (step-1 network) or K (step-2 network) input channels and 32 outputs at 257 bins: 9 C_in multiply-adds per output,
// i.e. it is bound by its un-pooled OUTPUT -- 32 x 257 floats per frame and signal, 10.6 GB per 500 ten-second signals -- which a
// library convolution writes and the pooling pass reads back (MIOpen's kernel 12.3 ms + the pooling pass 4.7 ms of a 93 ms C4 step,
// profiles/r06_b_c4_profile.txt).  Here the un-pooled map never exists: a workgroup owns TT output frames of one signal, stages the
// TT + 2 input rows of every channel in LDS once (each input row serves three output rows), and a lane owns one pooled bin q of
// 8 output channels: 32 accumulators, the maximum over each four taken in registers.  Weights are wave-uniform (one wave = one group of
// output channels): scalar loads.  The later blocks (32 -> 64 -> 64 channels, 288 / 576 multiply-adds per output) stay with the library:
// its Winograd kernels do 2.25x fewer multiplications than any direct form on the float32 matrix cores could save.
#pragma once
#include "common.h"

namespace disco {

constexpr int CONV1_OCW = 8;        // output channels per lane (one wave = OCW channels x 64 pooled bins)
// row pitch in LDS: x[f] sits at position f + 4, so that the four inputs [4q, 4q + 4) of a lane are one aligned 16-byte read; positions 3 and
// F + 4 ... hold the zero padding.  The CRNN is defined for 257 bins (its output layer has 257 units): one pitch, static LDS.
constexpr int CONV1_FP = 264;       // F <= CONV1_FP - 5

// x [B][C][Tin][F], w [O][C][3][3], bias [O] -> out [B][O][Tin - 2][F / 4].  grid (ceil((Tin - 2) / TT), B, O / (OCW * waves)), block 64 * waves.
template <int C, int TT>
static __global__ __launch_bounds__(256) void k_conv3x3_pool4_direct(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                              float* __restrict__ out, int O, int Tin, int F) {
    constexpr int OCW = CONV1_OCW;
    const int FQ = F / 4;                                   // pooled bins (floor mode)
    constexpr int FP = CONV1_FP;
    __shared__ __attribute__((aligned(16))) float s_x[C * (TT + 2) * FP];
    const int b = blockIdx.y, t0 = blockIdx.x * TT;
    const int Tout = Tin - 2;
    const int rows = min(TT, Tout - t0) + 2;
    const float* xb = x + (long long)b * C * Tin * F;
    for (int i = threadIdx.x; i < C * (TT + 2) * FP; i += blockDim.x) {
        const int c = i / ((TT + 2) * FP), r = (i / FP) % (TT + 2), f = i % FP - 4;
        s_x[i] = (r < rows && f >= 0 && f < F) ? xb[((long long)c * Tin + t0 + r) * F + f] : 0.f;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int o0 = __builtin_amdgcn_readfirstlane((blockIdx.z * (blockDim.x >> 6) + (threadIdx.x >> 6)) * OCW);     // wave-uniform
    const float* wg = w + (long long)o0 * C * 9;
    float bo[OCW];
#pragma unroll
    for (int o = 0; o < OCW; ++o) bo[o] = bias[o0 + o];
    for (int q = lane; q < FQ; q += 64) {
        for (int tt = 0; tt < rows - 2; ++tt) {
            float acc[OCW][4];
#pragma unroll
            for (int o = 0; o < OCW; ++o)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[o][j] = 0.f;
            // one input channel at a time (NOT unrolled: its 72 weights are scalar registers; all C x 72 at once do not fit)
#pragma unroll 1
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int kt = 0; kt < 3; ++kt) {
                    const float* row = s_x + (c * (TT + 2) + tt + kt) * FP + 4 * q;
                    const float4 mid = *reinterpret_cast<const float4*>(row + 4);          // x[4q .. 4q + 3]
                    const float xv[6] = {row[3], mid.x, mid.y, mid.z, mid.w, row[8]};     // x[4q - 1 .. 4q + 4]
#pragma unroll
                    for (int o = 0; o < OCW; ++o) {
                        const float* wk = wg + ((o * C + c) * 3 + kt) * 3;
                        const float w0 = wk[0], w1 = wk[1], w2 = wk[2];
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[o][j] = fmaf(w2, xv[j + 2], fmaf(w1, xv[j + 1], fmaf(w0, xv[j], acc[o][j])));
                    }
                }
#pragma unroll
            for (int o = 0; o < OCW; ++o) {
                // torch.nn.MaxPool2d propagates NaN, fmaxf drops it: each candidate is tested on its own (k_maxpool_last4)
                const float mx = fmaxf(fmaxf(acc[o][0], acc[o][1]), fmaxf(acc[o][2], acc[o][3]));
                const bool nan = (acc[o][0] != acc[o][0]) | (acc[o][1] != acc[o][1]) | (acc[o][2] != acc[o][2]) | (acc[o][3] != acc[o][3]);
                out[(((long long)b * O + o0 + o) * Tout + t0 + tt) * FQ + q] = (nan ? __builtin_nanf("") : mx) + bo[o];
            }
        }
    }
}

// one element of the map: clip(|.|, lo, hi) of X's microphone (c == 0) or of the (c - 1)-th other node's Z, frame t of signal g = (room, node)
static __device__ __forceinline__ float crnn_feature_at(const c32* __restrict__ X, const c32* __restrict__ Z, long long g, int c, int t, int f, int K, int M,
                                                        int T, int F, int mic, float lo, float hi) {
    c32 a;
    if (c == 0) {
        a = X[((g * T + t) * F + f) * (long long)M + mic];
    } else {
        const int k = (int)(g % K), j = (c - 1) < k ? (c - 1) : c;            // the (c - 1)-th node other than k
        a = Z[(((g / K) * K + j) * T + t) * (long long)F + f];
    }
    const float m = cabs_fma(a);
    return m != m ? m : fminf(fmaxf(m, lo), hi);     // NaN passes, as np.clip / torch.clamp leave it (fmaxf would make it lo)
}

// The networks' input features in one pass (speech_enhancement/utils.py:69-138 prepare_data; tango.py:338, 391, 158-186): out [R K][C][pad_lo + T +
// pad_hi][F] float = clip(|.|, lo, hi) of, channel 0, microphone `mic` of the node's own spectra X [R][K][T][F][M] and, channels 1 ... K - 1 (C = K: the
// step-2 network), the compressed signals Z [R][K][T][F] of the OTHER nodes in node order (get_z_for_mask 'zs_hat'); zeros in the padding rows (the
// reference pads AFTER clipping).  Replaces torch's strided abs, the clamp, the per-node index copies and the pad: four to seven passes over the map.
static __global__ void k_crnn_features(const c32* __restrict__ X, const c32* __restrict__ Z, float* __restrict__ out, long long R, int K, int M, int T, int F,
                                       int C, int mic, int pad_lo, int Tp, float lo, float hi) {
    const long long total = R * K * C * Tp * F;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int f = (int)(i % F);
        long long q = i / F;
        const int tp = (int)(q % Tp);
        q /= Tp;
        const int c = (int)(q % C);
        const long long g = q / C;                          // (room, node)
        const int t = tp - pad_lo;
        float v = 0.f;
        if (t >= 0 && t < T) v = crnn_feature_at(X, Z, g, c, t, f, K, M, T, F, mic, lo, hi);
        out[i] = v;
    }
}

// The same map for a batch whose rooms differ in clip length: room r has frames[r] <= T frames; every row at or beyond that is an exact zero like the
// padding rows (the reference pads zeros AFTER the clip, so a missing frame is 0 and not `lo`), and what X / Z hold there is never read.
static __global__ void k_crnn_features_rooms(const c32* __restrict__ X, const c32* __restrict__ Z, const int* __restrict__ frames, float* __restrict__ out,
                                             long long R, int K, int M, int T, int F, int C, int mic, int pad_lo, int Tp, float lo, float hi) {
    const long long total = R * K * C * Tp * F;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int f = (int)(i % F);
        long long q = i / F;
        const int tp = (int)(q % Tp);
        q /= Tp;
        const int c = (int)(q % C);
        const long long g = q / C;                          // (room, node)
        const int t = tp - pad_lo;
        float v = 0.f;
        if (t >= 0 && t < T && t < frames[g / K]) v = crnn_feature_at(X, Z, g, c, t, f, K, M, T, F, mic, lo, hi);
        out[i] = v;
    }
}

}  // namespace disco
