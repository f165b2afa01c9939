// net_f16.hpp -- launchers of the ONE-product kernels of the opt-in fp16 forward (net_f16.hip; see TrunkHLayerFn, NPROD = 1, in
// net_trunk_h16.hpp and boardh_body in net_board_h16.hpp). As net_w16.hpp: the instantiations live in their own translation unit so
// that they compile beside net.hip; the launchers take the argument blocks net.hip has filled in and return the HIP status of the
// attribute call / launch.
#pragma once

#include <hip/hip_runtime.h>

namespace ao {

struct TrunkHArgs;
struct BoardHArgs;
struct LayerHArgs;

// resident trunk (k_trunk16h_f16 / k_trunk16hb_f16<B, 4, 0>), boards 3 .. 9; in_kind 2 = bit planes
hipError_t launch_trunk16h_f16(int device, int B, int in_kind, int groups, hipStream_t s, const TrunkHArgs& a);
// board-resident trunk (k_boardh_f16<B, 1 | 2>), boards 10 .. 15
hipError_t launch_boardh_f16(int device, int B, bool bits, dim3 grid, hipStream_t s, const BoardHArgs& a);
// per-layer kernel (k_layer16h_f16<B, XT, 4, kind>, net_f16_layers.hip), boards 3 .. 15: XT = B up to 9, xt = 5 or 4 above; kind 0 a
// trunk layer, 1 conv1 on the fp32 plane batch, 2 conv1 on bit planes. AO_NET_PRECISION_FP16_ALL only.
hipError_t launch_layer16h_f16(int device, int B, int xt, int kind, dim3 grid, hipStream_t s, const LayerHArgs& a);

}  // namespace ao
