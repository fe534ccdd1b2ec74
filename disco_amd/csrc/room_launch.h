// Launches of the persistent room pass k_room_cov_dma<M, K, SUB> (k_room.h): api_room_s8.hip instantiates the shapes (SUB = 8 time
// sub-chunks per workgroup; SUB = 4 was measured equally fast and less accurate -- profiles/r05_c5_accumulation.txt -- and removed).
#pragma once
#include "host.h"
#include "k_room.h"

namespace disco_host {
// the launch of (M, K) where it is a shape of the room pass (dispatch.h: DISCO_FOR_ROOM), else false
bool launch_room_s8(int M, int K, unsigned nwg, hipStream_t st, const disco::RoomArgs& a);
}  // namespace disco_host
