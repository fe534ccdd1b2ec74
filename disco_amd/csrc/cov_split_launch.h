// Launches of the block-partitioned covariance kernels k_cov_split_lds / k_cov_loc_f64 (k_cov.h), shared by api_cov_split_m*.hip:
// each of those units instantiates the shapes of ONE mic count (the kernels are large; three units build in parallel).
#pragma once
#include "host.h"
#include "k_cov.h"

namespace disco_host {
using namespace disco;

// Step-1 shapes (KR = 0, M >= 7) run k_cov_loc_f64: float64 accumulators, 2 * chunks partial blocks.  (Their float32 forms -- lanes = bins,
// or 4 / 8 time sub-chunks across the lanes, option "cov1_mode" of round 4 -- were what C5's distance from the float64 oracle followed and
// were removed in round 5: profiles/r04_c_c5_variants_cov1_f64.json.)
template <int M, int KR>
static void launch_cov_split(bool skiploc, unsigned nblk, hipStream_t st, const CovArgs& a) {
    // even M (every shape with remote rows, and the step-1 shape M = 8) with F - 1 a multiple of 64 (both FFT sizes of this library): frames
    // staged through LDS once per workgroup (k_cov.h; with remote rows 7.3 ms per C5 launch, the per-wave fetches of k_cov_split: 9.6 ms)
    if constexpr (M % 2 == 0) {
        if (KR > 0) {               // (a run-time test: k_cov_split_lds<8, 0, false> is built and never run)
            const unsigned nb = (unsigned)xcd_grid(nblk);      // see the kernel's id -> item map
            with_bool(skiploc, [&](auto skip) {
                constexpr bool SKIP = KR > 0 && decltype(skip)::value;
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_split_lds<M, KR, SKIP>), dim3(nb), dim3(64 * cov_split_waves<KR, SKIP>()), 0, st, a);
            });
            return;
        }
    }
    if constexpr (KR == 0)          // step-1 statistics of the wide shapes: float64 accumulators, (hi, lo) pairs of partial blocks
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cov_loc_f64<M>), dim3(nblk), dim3(256), 0, st, a);
}

// the three units: the launch of (M, KR) where it is one of the unit's shapes (dispatch.h: DISCO_FOR_SPLIT_M8 / M4 / M2), else false
bool launch_cov_split_m8(int M, int KR, bool skiploc, unsigned nblk, hipStream_t st, const CovArgs& a);
bool launch_cov_split_m4(int M, int KR, bool skiploc, unsigned nblk, hipStream_t st, const CovArgs& a);
bool launch_cov_split_m2(int M, int KR, bool skiploc, unsigned nblk, hipStream_t st, const CovArgs& a);
}  // namespace disco_host
