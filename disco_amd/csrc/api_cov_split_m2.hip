// libdisco_hip.so -- host side of the C ABI (gfx950 only): block-partitioned covariance kernels, shapes of table M2
#include "cov_split_launch.h"

namespace disco_host {
bool launch_cov_split_m2(int M, int KR, bool skiploc, unsigned nblk, hipStream_t st, const CovArgs& a) {
    return for_split_m2(M, KR, [&](auto m, auto kr) { launch_cov_split<decltype(m)::value, decltype(kr)::value>(skiploc, nblk, st, a); });
}
}  // namespace disco_host
