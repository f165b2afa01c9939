// net_f16.hpp -- launchers of the ONE-product kernels of the opt-in fp16 forward (net_f16.hip; see TrunkHLayerFn, NPROD = 1, in
// net_trunk_h16.hpp and boardh_body in net_board_h16.hpp). As net_w16.hpp: the instantiations live in their own translation unit so
// that they compile beside net.hip; the launchers take the argument blocks net.hip has filled in and return the HIP status of the
// attribute call / launch.
#pragma once

#include <hip/hip_runtime.h>

namespace ao {

struct TrunkHArgs;
struct BoardHArgs;

// resident trunk (k_trunk16h_f16 / k_trunk16hb_f16<B, 4, 0>), boards 3 .. 9; in_kind 2 = bit planes
hipError_t launch_trunk16h_f16(int device, int B, int in_kind, int groups, hipStream_t s, const TrunkHArgs& a);
// board-resident trunk (k_boardh_f16<B, 1 | 2>), boards 10 .. 15
hipError_t launch_boardh_f16(int device, int B, bool bits, dim3 grid, hipStream_t s, const BoardHArgs& a);

}  // namespace ao
