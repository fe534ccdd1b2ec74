// From a run-time shape to a template instantiation: the ONE place where the host code turns "M = 4, K = 4, same mask, packed" into
// k<4, 4, true, true>.  Every api_*.hip launches through these helpers; a call site is a generic lambda that receives the matching
// entry as compile-time tags and names the kernel:
//     for_mkr(M, K - 1, [&](auto m, auto kr) { with_bool(skiploc, [&](auto skip) {
//         constexpr int M_ = decltype(m)::value, K_ = decltype(kr)::value + 1;
//         constexpr bool SKIPLOC = decltype(skip)::value;
//         hipLaunchKernelGGL(HIP_KERNEL_NAME(k<M_, K_, SKIPLOC>), grid, block, 0, st, a); }); });
// (The values are named before the launch: hipLaunchKernelGGL is a macro, and what the CPU test emulator makes of it sees the tags through
// one more capture, where decltype no longer gives the plain type.)
// A table helper returns whether the shape is in its table (the launch happened); with an empty callable it is the shape predicate.
// A new compile-time parameter of a kernel is one more with_bool / for_int around the launch, and an `if constexpr` inside the lambda
// is what keeps a combination from being instantiated.  The tables are the X-macro lists below, each expanded in this file only.
#pragma once
#include <type_traits>

// (M, KR) instantiation table: every split of P = M + KR <= 8 channels.
#define DISCO_FOR_MKR(X_) \
    X_(1, 0) X_(1, 1) X_(1, 2) X_(1, 3) X_(1, 4) X_(1, 5) X_(1, 6) X_(1, 7) \
    X_(2, 0) X_(2, 1) X_(2, 2) X_(2, 3) X_(2, 4) X_(2, 5) X_(2, 6)          \
    X_(3, 0) X_(3, 1) X_(3, 2) X_(3, 3) X_(3, 4) X_(3, 5)                   \
    X_(4, 0) X_(4, 1) X_(4, 2) X_(4, 3) X_(4, 4)                            \
    X_(5, 0) X_(5, 1) X_(5, 2) X_(5, 3)                                     \
    X_(6, 0) X_(6, 1) X_(6, 2)                                              \
    X_(7, 0) X_(7, 1)                                                       \
    X_(8, 0)
// (M, KR) shapes for which the block-partitioned kernels k_cov_split_lds / k_cov_loc_f64 are instantiated, one table per unit
// (api_cov_split_m8 / _m4 / _m2.hip): 9 <= M + KR <= 16, and the step-1 shapes (KR = 0) whose 2 * M(M+1)/2 complex accumulators no
// longer fit one thread without spilling (M >= 7)
#define DISCO_FOR_SPLIT_M8(X_) X_(7, 0) X_(8, 0) X_(8, 1) X_(8, 2) X_(8, 3) X_(8, 4) X_(8, 5) X_(8, 6) X_(8, 7) X_(8, 8)
#define DISCO_FOR_SPLIT_M4(X_) X_(4, 5) X_(4, 6) X_(4, 7) X_(4, 8) X_(4, 9) X_(4, 10) X_(4, 11) X_(4, 12)
#define DISCO_FOR_SPLIT_M2(X_) X_(2, 7) X_(2, 8) X_(2, 9) X_(2, 10) X_(2, 11) X_(2, 12) X_(2, 13) X_(2, 14)
// (M, KRT) of k_apply_mq: 4 or 8 microphones, the remote rows padded to KRT
#define DISCO_FOR_APPLY_MQ(X_) X_(4, 1) X_(4, 3) X_(4, 7) X_(4, 15) X_(8, 1) X_(8, 3) X_(8, 7) X_(8, 15)
// (M, K) shapes of the one-pass room covariance (wide shapes: P = M + K - 1 > 8)
#define DISCO_FOR_ROOM(X_) X_(8, 8) X_(8, 6) X_(8, 4) X_(8, 2) X_(4, 8) X_(4, 6)
// (M, K) shapes of the one-pass filter + iSTFT k_apply_istft_wide: the wide shapes of the room pass (the whole-path calls end in it) and the
// narrow 4-mic shapes a NODE SHARD needs it for (with all nodes of a room on the GPU those keep z on chip: k_step2_apply_istft)
#define DISCO_FOR_WIDE_ISTFT(X_) DISCO_FOR_ROOM(X_) X_(4, 4) X_(4, 3) X_(4, 2)

namespace disco_host {
template <int V>
using int_c = std::integral_constant<int, V>;

#define DISCO_TABLE_ENTRY_(A_, B_)        \
    if (a == A_ && b == B_) {             \
        fn(int_c<A_>{}, int_c<B_>{});     \
        return true;                      \
    }
#define DISCO_TABLE_WALK_(NAME_, TABLE_)  \
    template <class Fn>                   \
    bool NAME_(int a, int b, Fn&& fn) {   \
        TABLE_(DISCO_TABLE_ENTRY_)        \
        return false;                     \
    }
DISCO_TABLE_WALK_(for_mkr, DISCO_FOR_MKR)                   // (M, KR)
DISCO_TABLE_WALK_(for_split_m8, DISCO_FOR_SPLIT_M8)         // (M, KR)
DISCO_TABLE_WALK_(for_split_m4, DISCO_FOR_SPLIT_M4)
DISCO_TABLE_WALK_(for_split_m2, DISCO_FOR_SPLIT_M2)
DISCO_TABLE_WALK_(for_apply_mq, DISCO_FOR_APPLY_MQ)         // (M, KRT)
DISCO_TABLE_WALK_(for_room, DISCO_FOR_ROOM)                 // (M, K)
DISCO_TABLE_WALK_(for_wide_istft, DISCO_FOR_WIDE_ISTFT)     // (M, K)
#undef DISCO_TABLE_WALK_
#undef DISCO_TABLE_ENTRY_

// fn(int_c<v>) for LO <= v <= HI; false: v is outside
template <int LO, int HI, class Fn>
bool for_int(int v, Fn&& fn) {
    if constexpr (LO > HI) {
        return false;
    } else {
        if (v == LO) {
            fn(int_c<LO>{});
            return true;
        }
        return for_int<LO + 1, HI>(v, fn);
    }
}

// fn(std::true_type) or fn(std::false_type); its result is handed on
template <class Fn>
decltype(auto) with_bool(bool b, Fn&& fn) {
    if (b) return fn(std::true_type{});
    return fn(std::false_type{});
}
}  // namespace disco_host
