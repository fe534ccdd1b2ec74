// Shared device helpers for the DISCO MWF kernels (gfx950, wave64).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/disco_hip.h"

namespace disco {

typedef float2 c32;    // interleaved complex64, bit-compatible with disco_c32 / numpy complex64
typedef double2 c64;   // complex128

constexpr int WAVE = 64;

__device__ __forceinline__ c32 cmul(c32 a, c32 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// Complex add / sub as ONE packed instruction (v_pk_add_f32).  Measured on MI355X: the butterflies' adds packed this way
// are worth ~7 % on the FFT-only kernel; builds that also packed the MULTIPLIES (complex products with op_sel swizzles,
// packed covariance fma) measured 1.1-1.7x SLOWER per kernel (register-pair pressure, spills) and were dropped.
// DISCO_PK=0: all scalar (also what the g++ test build uses, ext_vector_type being a clang extension).
#ifndef DISCO_PK
#define DISCO_PK 1
#endif
#if DISCO_PK && defined(__clang__)
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ c32 cadd(c32 a, c32 b) {
    const v2f r = v2f{a.x, a.y} + v2f{b.x, b.y};
    return make_float2(r.x, r.y);
}
__device__ __forceinline__ c32 csub(c32 a, c32 b) {
    const v2f r = v2f{a.x, a.y} - v2f{b.x, b.y};
    return make_float2(r.x, r.y);
}
#else
__device__ __forceinline__ c32 cadd(c32 a, c32 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ c32 csub(c32 a, c32 b) { return make_float2(a.x - b.x, a.y - b.y); }
#endif
__device__ __forceinline__ c32 cconj(c32 a) { return make_float2(a.x, -a.y); }
// multiply by -i / +i
__device__ __forceinline__ c32 cmul_mi(c32 a) { return make_float2(a.y, -a.x); }
__device__ __forceinline__ c32 cmul_pi(c32 a) { return make_float2(-a.y, a.x); }

// |a| as the CRNN's features and the training bank take it (k_crnn_conv.h crnn_feature_at, k_bank.h): ONE expression, so that what the network
// sees in training is bit for bit what it sees at inference.  |a|^2 with its fma written out: hipcc's contraction chose
// fma(a.x, a.x, a.y a.y) for the plain sum of squares, but its choice follows the code around it.  NaN passes.
__device__ __forceinline__ float cabs_fma(c32 a) { return sqrtf(fmaf(a.x, a.x, a.y * a.y)); }

__device__ __forceinline__ c64 zmul(c64 a, c64 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// a * conj(b)
__device__ __forceinline__ c64 zmulc(c64 a, c64 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }
__device__ __forceinline__ c64 zadd(c64 a, c64 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ c64 zsub(c64 a, c64 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ c64 zscale(c64 a, double s) { return make_double2(a.x * s, a.y * s); }
// Fused complex multiply-adds: four float64 FMAs each (zsub(s, zmul(a, b)) is two multiplies, two FMAs and two subtractions -- the thread
// solver's Cholesky, whitening and substitutions are these; round 6: 6 460 -> ~5 800 instructions per online solve).
//   s - a b,   s - a conj(b),   s - conj(a) b,   s + a b,   s + conj(a) b
__device__ __forceinline__ c64 zfnma(c64 s, c64 a, c64 b) { return make_double2(fma(a.y, b.y, fma(-a.x, b.x, s.x)), fma(-a.y, b.x, fma(-a.x, b.y, s.y))); }
__device__ __forceinline__ c64 zfnmac(c64 s, c64 a, c64 b) { return make_double2(fma(-a.y, b.y, fma(-a.x, b.x, s.x)), fma(a.x, b.y, fma(-a.y, b.x, s.y))); }
__device__ __forceinline__ c64 zfnmca(c64 s, c64 a, c64 b) { return make_double2(fma(-a.y, b.y, fma(-a.x, b.x, s.x)), fma(a.y, b.x, fma(-a.x, b.y, s.y))); }
__device__ __forceinline__ c64 zfma(c64 s, c64 a, c64 b) { return make_double2(fma(-a.y, b.y, fma(a.x, b.x, s.x)), fma(a.y, b.x, fma(a.x, b.y, s.y))); }
__device__ __forceinline__ c64 zfmca(c64 s, c64 a, c64 b) { return make_double2(fma(a.y, b.y, fma(a.x, b.x, s.x)), fma(-a.y, b.x, fma(a.x, b.y, s.y))); }
// c ? a : b on VALUES (`c ? x : y` on two c64 lvalues selects an ADDRESS, which keeps both objects out of registers)
__device__ __forceinline__ c64 zsel(bool c, c64 a, c64 b) { return make_double2(c ? a.x : b.x, c ? a.y : b.y); }

// Pin the point where a prefetched value must have landed: an empty asm that "modifies" the register makes hipcc
// place the s_waitcnt for its load HERE instead of wherever register coalescing leaves the first real use
// (typically the loop back-edge, i.e. after -- and therefore behind -- the iteration's stores).
#ifndef DISCO_CONSUME
#define DISCO_CONSUME(x) asm volatile("" : "+v"(x))
#endif

// Code-motion fence for long unrolled straight-line code: memory accesses are not moved across it by any stage of
// hipcc (instruction selection linearises a basic block with every independent LDS load first -- all P^2/2 entries of a
// triangular factor, 4 registers each -- and only a memory-clobbering statement pins loads behind it; the scheduler
// barrier then keeps the arithmetic of one row from drifting into the next).  No instruction is emitted.
#if defined(__clang__)
#define DISCO_SCHED_FENCE()                       \
    do {                                          \
        asm volatile("" ::: "memory");            \
        __builtin_amdgcn_sched_barrier(0);        \
    } while (0)
#else
#define DISCO_SCHED_FENCE() asm volatile("" ::: "memory")
#endif

// Placement of the streaming kernels' code.  hipcc aligns a kernel to 256 bytes, so where it falls inside a 4-KiB page depends on
// every kernel defined before it.  Round 2, pass l: after the k_room.h kernels were added, k_step2_apply_istft<512, 4, 4> (sources
// unchanged, now 3584 instead of 512 bytes into its page) measured 4.79 / 4.88 ms per C3 launch on two boxes against 4.37-4.39 before;
// pinned to a page boundary it measured 4.45 ms on a third box -- and 4.85 ms on a fourth.  The box-to-box spread of that kernel is
// therefore as large as the suspected placement effect and the effect itself is NOT established; the hot kernels stay pinned to page
// boundaries because it costs nothing but padding and takes one variable out of every later comparison.
#if defined(__clang__)
#define DISCO_KERNEL_ALIGN __attribute__((aligned(4096)))
#else
#define DISCO_KERNEL_ALIGN
#endif

// x + the value of lane (lane ^ 1) / (lane ^ 2) of the same quad: DPP quad_perm moves ride the VALU (a few cycles; the
// ds_bpermute form of __shfl_xor is an LDS-crossbar round trip of ~100 cycles in the middle of a dependent chain)
template <int XOR>
__device__ __forceinline__ float quad_xor_add(float x) {
#if defined(__clang__)
    constexpr int ctrl = XOR == 1 ? 0xB1 : 0x4E;       // quad_perm [1,0,3,2] / [2,3,0,1]
    const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, 0xf, 0xf, false);
    return x + __int_as_float(y);
#else
    return x + __shfl_xor(x, XOR);
#endif
}

// Butterfly sum over a group of G lanes (G = 64: the wave); every lane of the group ends with the result.  The order of the additions
// is part of the result: a site that adds in another order, or reduces two values in one interleaved loop, keeps its own loop.
template <int G>
__device__ __forceinline__ double group_sum(double x) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) x += __shfl_xor(x, off, G);
    return x;
}

// LDS exchange fences.  The exchange buffers are WAVE-PRIVATE, so no s_barrier is needed: a wave's DS
// instructions execute in issue order, and all that has to be prevented is (a) the compiler moving a read
// above the writes it depends on through another lane, (b) a read issuing before this wave's own writes have
// been accepted.  RAW = `s_waitcnt lgkmcnt(0)` (0xC07F: vmcnt/expcnt untouched, so global prefetches stay in
// flight) + a scheduling barrier; WAR = scheduling barrier only.
#define DISCO_LDS_RAW()                       \
    do {                                      \
        __builtin_amdgcn_s_waitcnt(0xC07F);   \
        __builtin_amdgcn_wave_barrier();      \
    } while (0)
#define DISCO_LDS_WAR() __builtin_amdgcn_wave_barrier()

// Stores of data this pass will not read again and that is far larger than any cache (the spectra X: 20 GB per C3 step) are marked
// non-temporal (global_store ... nt): 7.10 -> 6.88 ms per C3 launch of k_stft_cov, same-box pairs (profiles/r03_y_*).  The mask and
// output-sample stores (store_stream4) are plain stores: the mark was tried there and not taken.
__device__ __forceinline__ void store_stream16(float4* p, const float4& v) {
#if defined(__clang__)
    typedef float v4f_ __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(v4f_{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f_*>(p));
#else
    *p = v;
#endif
}
__device__ __forceinline__ void store_stream4(float* p, const float v) { *p = v; }

// Which workgroup does what, where neighbouring logical items share lines (the nodes of a room read the same remote rows): the hardware
// deals consecutive workgroup ids round-robin to the N_XCD XCDs (one L2 each), so on a grid padded to a multiple of N_XCD (xcd_grid,
// host.h) id b takes logical item (b % N_XCD) * (grid / N_XCD) + b / N_XCD -- consecutive items run on ONE XCD.  The items at or beyond
// the real count are the padding: their workgroups return at once.
constexpr int N_XCD = 8;
__device__ __forceinline__ long long xcd_item() { return (long long)(blockIdx.x % N_XCD) * (gridDim.x / N_XCD) + blockIdx.x / N_XCD; }

// The wave index as a PROVABLY wave-uniform value: anything derived from threadIdx is divergent to hipcc, which
// then wraps every access guarded by a per-wave condition in exec-mask branches (one per load).
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Index of the [T][F] plane of (room r, GLOBAL node j) inside an array of exchanged signals Z.  The plain layout is [R][K]
// (zblk = K).  An all-gather over ranks that hold zblk nodes each delivers [K / zblk][R][zblk] -- rank-major -- and is consumed
// as it arrives when zblk says so (disco_set_z_blocks): no transposing copy between the collective and step 2.
__device__ __forceinline__ long long z_plane(long long r, int j, int K, long long R, int zblk) {
    (void)K;
    return ((long long)(j / zblk) * R + r) * zblk + (j % zblk);
}

// Per-room clip lengths (disco_set_lengths): `lens` is the context's device array of one length per room, nullptr for the uniform
// batch.  The room index must be wave-uniform (from blockIdx, or from wave_id()), so that the length comes through the scalar path
// and lives in an SGPR; readfirstlane states that for the value as well.  T_r = 1 + L_r / hop follows from it.
__device__ __forceinline__ int room_length(const int* __restrict__ lens, long long room, int Lmax) {
    return lens ? __builtin_amdgcn_readfirstlane(lens[room]) : Lmax;
}

// reflect / zero padded sample fetch, branch-free: p is the index into the un-padded signal of length L.
// The load is unconditional (clamped index); out-of-range samples of constant padding are zeroed by a select.
__device__ __forceinline__ float load_padded(const float* __restrict__ x, int p, int L, int pad_mode) {
    const bool outside = (p < 0) || (p >= L);
    int q = p < 0 ? -p : (p >= L ? 2 * (L - 1) - p : p);      // np.pad(mode='reflect')
    q = q < 0 ? 0 : (q >= L ? L - 1 : q);                      // keeps inputs shorter than the window in bounds
    const float v = x[q];
    return (outside && pad_mode != DISCO_PAD_REFLECT) ? 0.f : v;
}

}  // namespace disco
