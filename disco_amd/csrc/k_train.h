// Kernels of the CRNN training path (disco_amd/dnn/train.py): the GRU's pointwise forward that keeps what back-propagation needs, one step of
// back-propagation through time, the frame-selecting reconstruction loss and its gradient, and the batch gather from the spectra bank.
// The convolutions, BatchNorm, the GEMMs and the optimiser stay in PyTorch-ROCm; these are the pieces autograd would otherwise run as dozens
// of element-wise kernels per step, or (the gather) on the host.
#pragma once
#include <hip/hip_runtime.h>

namespace disco {

constexpr int TRAIN_LOSS_THREADS = 256;

// V consecutive floats: one 16-byte access (V = 4; the caller has checked the alignment) or one dword (V = 1)
template <int V>
__device__ __forceinline__ void ldv(float (&d)[V], const float* p) {
    if constexpr (V == 4) {
        const float4 t = *(const float4*)p;
        d[0] = t.x, d[1] = t.y, d[2] = t.z, d[3] = t.w;
    } else {
        d[0] = *p;
    }
}
template <int V>
__device__ __forceinline__ void stv(float* p, const float (&d)[V]) {
    if constexpr (V == 4)
        *(float4*)p = make_float4(d[0], d[1], d[2], d[3]);
    else
        *p = d[0];
}

// The two multiply-adds of a GRU step as k_gru_gates (k_apply.h) evaluates them.  That kernel writes `g + r * hn` and `(1.f - z) * nn + z * hp` and leaves
// them to hipcc's contraction, which fuses r hn into the sum and (1 - z) nn into the other product; WHICH of the two products of the second
// expression gets fused is the optimiser's choice from the shape of the surrounding code, and came out the other way round in this kernel.  The
// fused forms are therefore written out here, so that h_out has k_gru_gates' bits whatever surrounds them; the emulated build (HIPEMU) compiles
// both kernels with contraction off, where the plain expressions are the ones that agree.
__device__ __forceinline__ float gru_candidate_arg(float gn, float r, float hn) {
#ifdef HIPEMU
    return gn + r * hn;
#else
    return fmaf(r, hn, gn);
#endif
}
__device__ __forceinline__ float gru_blend(float z, float c, float hp) {
#ifdef HIPEMU
    return (1.f - z) * c + z * hp;
#else
    return fmaf(1.f - z, c, z * hp);
#endif
}

// k_gru_gates that also stores r, z, the candidate and gh_n: saved [n][4H] = [r | z | c | gh_n].  h_out is computed exactly as there -- same
// expressions in the same order, same expf / tanhf -- so that the two kernels give the same bits.
// V = 4: H, gi_stride multiples of 4 and every pointer 16-byte aligned.
template <int V>
static __global__ void k_gru_gates_train(const float* __restrict__ gi, long long gi_stride, const float* __restrict__ gh,
                                         const float* __restrict__ gh_bias, const float* h_prev, float* h_out, float* __restrict__ saved,
                                         long long n, int H) {
    const int Hv = H / V;
    const long long total = n * Hv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / Hv;
        const int c = (int)(i - row * Hv) * V;
        const float* g = gi + row * gi_stride;
        const float* q = gh ? gh + row * 3 * H : gh_bias;
        float gr[V], gz[V], gn[V], hr[V], hz[V], hn[V], hp[V], ro[V], zo[V], no[V], ho[V];
        ldv<V>(gr, g + c);
        ldv<V>(gz, g + H + c);
        ldv<V>(gn, g + 2 * H + c);
        ldv<V>(hr, q + c);
        ldv<V>(hz, q + H + c);
        ldv<V>(hn, q + 2 * H + c);
        if (h_prev) {
            ldv<V>(hp, h_prev + row * H + c);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) hp[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float r = 1.f / (1.f + expf(-(gr[j] + hr[j])));
            const float z = 1.f / (1.f + expf(-(gz[j] + hz[j])));
            const float nn = tanhf(gru_candidate_arg(gn[j], r, hn[j]));
            ho[j] = gru_blend(z, nn, hp[j]);
            ro[j] = r, zo[j] = z, no[j] = nn;
        }
        stv<V>(h_out + row * H + c, ho);
        float* sv = saved + row * 4 * H + c;
        stv<V>(sv, ro);
        stv<V>(sv + H, zo);
        stv<V>(sv + 2 * H, no);
        stv<V>(sv + 3 * H, hn);
    }
}

// One step of back-propagation through time.  With d = d_out + d_carry (either may be absent) and the step's saved [r | z | c | gh_n]:
//   dn = d (1 - z), dz = d (h_prev - c), d_h_direct = d z, da_n = dn (1 - c^2), da_z = dz z (1 - z), da_r = da_n gh_n r (1 - r)
//   d_gi = [da_r | da_z | da_n] (rows at d_gi_stride), d_gh = [da_r | da_z | da_n r] ([n][3H]), d_h_direct [n][H]
template <int V>
static __global__ void k_gru_gates_backward(const float* __restrict__ d_out, long long d_out_stride, const float* __restrict__ d_carry,
                                            const float* __restrict__ saved, const float* __restrict__ h_prev, float* __restrict__ d_gi,
                                            long long d_gi_stride, float* __restrict__ d_gh, float* __restrict__ d_h_direct, long long n, int H) {
    const int Hv = H / V;
    const long long total = n * Hv;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / Hv;
        const int c = (int)(i - row * Hv) * V;
        float d[V], dc[V], r[V], z[V], nn[V], hn[V], hp[V], ar[V], az[V], an[V], anr[V], dh[V];
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = dc[j] = hp[j] = 0.f;
        if (d_out) ldv<V>(d, d_out + row * d_out_stride + c);
        if (d_carry) ldv<V>(dc, d_carry + row * H + c);
        if (h_prev) ldv<V>(hp, h_prev + row * H + c);
        const float* sv = saved + row * 4 * H + c;
        ldv<V>(r, sv);
        ldv<V>(z, sv + H);
        ldv<V>(nn, sv + 2 * H);
        ldv<V>(hn, sv + 3 * H);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float dd = d[j] + dc[j];
            const float dn = dd * (1.f - z[j]);
            const float dz = dd * (hp[j] - nn[j]);
            dh[j] = dd * z[j];
            an[j] = dn * (1.f - nn[j] * nn[j]);
            az[j] = dz * z[j] * (1.f - z[j]);
            ar[j] = an[j] * hn[j] * r[j] * (1.f - r[j]);
            anr[j] = an[j] * r[j];
        }
        float* gi = d_gi + row * d_gi_stride + c;
        stv<V>(gi, ar);
        stv<V>(gi + H, az);
        stv<V>(gi + 2 * H, an);
        float* gh = d_gh + row * 3 * H + c;
        stv<V>(gh, ar);
        stv<V>(gh + H, az);
        stv<V>(gh + 2 * H, anr);
        stv<V>(d_h_direct + row * H + c, dh);
    }
}

// ---- reconstruction loss (dnn/engine/losses.py:4-25) on the loss frames (dnn/utils.py:212-246), nothing sliced out ----------------------------
// term(b, j, f) = ((est[b][j][f] - y[b][ff_in + j][f]) x[b][0][ff_in + j][f])^2, formed in float64; NaN terms are left out of sum and count.
struct LossTerm {
    double e, x;      // est - y, the weight
    __device__ __forceinline__ double value() const {
        const double t = e * x;
        return t * t;
    }
};
__device__ __forceinline__ LossTerm loss_term(const float* __restrict__ est, const float* __restrict__ y, const float* __restrict__ x, long long idx,
                                              int C, int W, int F, int ff_in, int n_out) {
    const long long bj = idx / F;
    const int f = (int)(idx - bj * F);
    const long long b = bj / n_out;
    const int j = (int)(bj - b * n_out);
    const long long fr = ff_in + j;
    LossTerm t;
    t.e = (double)est[idx] - (double)y[(b * W + fr) * F + f];
    t.x = (double)x[((b * C) * W + fr) * F + f];
    return t;
}

// the 256 values of a workgroup -> lane 0, in a fixed tree (the order depends on nothing but the thread index)
__device__ __forceinline__ void block_fold2(double& a, double& b) {
    __shared__ double sa[TRAIN_LOSS_THREADS], sb[TRAIN_LOSS_THREADS];
    const int t = threadIdx.x;
    sa[t] = a, sb[t] = b;
    __syncthreads();
    for (int w = TRAIN_LOSS_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) sa[t] += sa[t + w], sb[t] += sb[t + w];
        __syncthreads();
    }
    a = sa[0], b = sb[0];
    __syncthreads();
}

// per-workgroup partial sums: part[2 blockIdx] = (sum, count) of the terms idx = blockIdx * 256 + thread + k * gridDim * 256
static __global__ void __launch_bounds__(TRAIN_LOSS_THREADS)
k_recon_loss_partial(const float* __restrict__ est, const float* __restrict__ y, const float* __restrict__ x, long long total, int C, int W, int F,
                     int ff_in, int n_out, double* __restrict__ part) {
    double sum = 0.0, cnt = 0.0;
    for (long long i = (long long)blockIdx.x * TRAIN_LOSS_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * TRAIN_LOSS_THREADS) {
        const double v = loss_term(est, y, x, i, C, W, F, ff_in, n_out).value();
        if (v == v) {
            sum += v;
            cnt += 1.0;
        }
    }
    block_fold2(sum, cnt);
    if (threadIdx.x == 0) part[2 * blockIdx.x] = sum, part[2 * blockIdx.x + 1] = cnt;
}

// the one fold: sums[0] = sum, sums[1] = count.  One workgroup.
static __global__ void __launch_bounds__(TRAIN_LOSS_THREADS) k_recon_loss_fold(const double* __restrict__ part, int n_part, double* __restrict__ sums) {
    double sum = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < n_part; i += TRAIN_LOSS_THREADS) sum += part[2 * i], cnt += part[2 * i + 1];
    block_fold2(sum, cnt);
    if (threadIdx.x == 0) sums[0] = sum, sums[1] = cnt;
}

// d_est = g 2 (est - y) x^2 / count, formed in float64 and rounded once; +0 where the term is NaN
static __global__ void k_recon_loss_grad(const float* __restrict__ est, const float* __restrict__ y, const float* __restrict__ x, long long total, int C,
                                         int W, int F, int ff_in, int n_out, const double* __restrict__ sums, const float* __restrict__ g,
                                         float* __restrict__ d_est) {
    const double scale = 2.0 * (double)g[0] / sums[1];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const LossTerm t = loss_term(est, y, x, i, C, W, F, ff_in, n_out);
        const double v = t.value();
        d_est[i] = v == v ? (float)(scale * t.e * t.x * t.x) : 0.f;
    }
}

// ---- batch gather: bank [S][N][T][F], tab [B][C + 3] = (segment k, first frame m, C input rows, label row) -> x [B][C][W][F], y [B][W][F] --------
// Each (item, row) is one contiguous run of W F floats on both sides; a workgroup copies one run at a time, dword by dword (F = 257 leaves
// the runs 4-byte aligned only).  An entry out of range gives a run of zeros: nothing is read outside the bank.
static __global__ void k_train_batch(const float* __restrict__ bank, int S, long long N, int T, int F, const int* __restrict__ tab, long long B, int C,
                                     int W, float* __restrict__ x, float* __restrict__ y) {
    const long long runs = B * (C + 1);
    const int len = W * F;
    for (long long ir = blockIdx.x; ir < runs; ir += gridDim.x) {
        const long long item = ir / (C + 1);
        const int j = (int)(ir - item * (C + 1));
        const int* t = tab + item * (C + 3);
        const int k = t[0], m = t[1], row = t[2 + j];
        const bool ok = k >= 0 && k < N && m >= 0 && m <= T - W && row >= 0 && row < S;
        const float* src = ok ? bank + (((long long)row * N + k) * T + m) * F : nullptr;
        float* dst = j < C ? x + (item * C + j) * len : y + item * len;
        for (int e = threadIdx.x; e < len; e += blockDim.x) dst[e] = ok ? src[e] : 0.f;
    }
}

}  // namespace disco
