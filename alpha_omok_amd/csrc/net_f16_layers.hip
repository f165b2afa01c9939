// net_f16_layers.hip -- the one-product instantiations of the PER-LAYER kernel (k_layer16h_f16) and their launcher (net_f16.hpp).
//
// ao_net_precision(AO_NET_PRECISION_FP16_ALL): the fp16 forward of net_f16.hip for the batches that are planned onto neither the
// resident trunk nor k_boardh -- any board 3 .. 15 at any batch size, conv1 included (KIND 1 the fp32 plane batch, 2 the engine's
// bit planes, 0 a trunk layer). The same arithmetic: the weight operand fp16(w * 2^s), every stored activation rounded once to
// fp16 (to nearest even, after ReLU and the clamp at 65504), fp32 accumulation, BatchNorm and residual add; the heads
// (k_head_conv<2>, k_head_fc) read the rounded value. Same device code as k_layer16h (trunk_h_layer_tile, NPROD = 1), same LDS /
// HBM geometry with the low slots unused. A translation unit of its own so that its 57 kernels compile beside net_f16.hip.
// The reference's network is model.py:6-31,76-104 (PVNet, ResBlock).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/omok_hip.h"
#include "engine_types.hpp"
#include "net_device.hpp"
#include "net_common.hpp"
#include "net_trunk_f32.hpp"
#include "net_trunk_h16.hpp"
#include "net_f16.hpp"

namespace ao {

#if AO_KO == 0 && !AO_CONV1_SPLIT

namespace {
constexpr int kDev = 16;
// dynamic-LDS attribute set once per (device, board, XT == 4, KIND)
bool g_attr_layer[kDev][16][2][3];

template <typename K>
hipError_t set_lds(bool* done, K kernel, size_t lds) {
    if (*done) return hipSuccess;
    const hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (st == hipSuccess) *done = true;
    return st;
}

template <int W, int XT, int KIND>
hipError_t launch_one(int device, dim3 grid, hipStream_t s, const LayerHArgs& a) {
    constexpr int NX = (XT < W) ? XT + 2 : XT;
    constexpr size_t lds = static_cast<size_t>(2) * NX * 4 * 2 * 1024;   // two row buffers in the split forms' geometry
    const hipError_t st = set_lds(&g_attr_layer[device][W][XT == 4][KIND], &k_layer16h_f16<W, XT, 4, KIND>, lds);
    if (st != hipSuccess) return st;
    hipLaunchKernelGGL((k_layer16h_f16<W, XT, 4, KIND>), grid, dim3(512), lds, s, a);
    return hipGetLastError();
}

template <int W, int XT>
hipError_t launch_kind(int device, int kind, dim3 grid, hipStream_t s, const LayerHArgs& a) {
    switch (kind) {
        case 0: return launch_one<W, XT, 0>(device, grid, s, a);
        case 1: return launch_one<W, XT, 1>(device, grid, s, a);
        case 2: return launch_one<W, XT, 2>(device, grid, s, a);
        default: return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t launch_layer16h_f16(int device, int B, int xt, int kind, dim3 grid, hipStream_t s, const LayerHArgs& a) {
    if (device < 0 || device >= kDev) return hipErrorInvalidDevice;
    switch (B) {
#define AO_BW_CASE(W) case W: return launch_kind<W, W>(device, kind, grid, s, a);
        AO_BW_CASE(3) AO_BW_CASE(4) AO_BW_CASE(5) AO_BW_CASE(6) AO_BW_CASE(7) AO_BW_CASE(8) AO_BW_CASE(9)
#undef AO_BW_CASE
#define AO_BW_CASE(W) case W: return xt == 4 ? launch_kind<W, 4>(device, kind, grid, s, a) : launch_kind<W, 5>(device, kind, grid, s, a);
        AO_BW_CASE(10) AO_BW_CASE(11) AO_BW_CASE(12) AO_BW_CASE(13) AO_BW_CASE(14) AO_BW_CASE(15)
#undef AO_BW_CASE
        default: return hipErrorInvalidValue;
    }
}

#else   // timing knock-outs and the measured-neutral conv1 variant are experiments on the split forms only

hipError_t launch_layer16h_f16(int, int, int, int, dim3, hipStream_t, const LayerHArgs&) { return hipErrorNotSupported; }

#endif

}  // namespace ao
