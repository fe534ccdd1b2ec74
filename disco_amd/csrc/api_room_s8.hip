// libdisco_hip.so -- host side of the C ABI (gfx950 only): the persistent room pass with 8 time sub-chunk(s) per workgroup
#include "room_launch.h"

namespace disco_host {
using namespace disco;
bool launch_room_s8(int M, int K, unsigned nwg, hipStream_t st, const RoomArgs& a) {
    return for_room(M, K, [&](auto m, auto k) {
        constexpr int M_ = decltype(m)::value, K_ = decltype(k)::value;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_room_cov_dma<M_, K_, 8>), dim3(nwg), dim3(RoomGeomS<M_, K_, 8>::NT), 0, st, a);
    });
}
}  // namespace disco_host
