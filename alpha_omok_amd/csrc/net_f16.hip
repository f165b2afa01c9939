// net_f16.hip -- the one-product instantiations of the two kernels that carry search at scale, and their launchers (net_f16.hpp).
//
// The opt-in fp16 forward (ao_net_precision(AO_NET_PRECISION_FP16)): plain fp16 operands with fp32 accumulation. Of
// x * w = xh*wh + xh*wl + xl*wh (net_trunk_h16.hpp) only xh*wh is issued: the weight operand is fp16(w * 2^s), the activation
// operand the activation rounded once to fp16 (to nearest even, after ReLU and the clamp at 65504), and everything downstream of a
// layer -- the next conv, the block's residual add, the heads -- reads that rounded value. BatchNorm, residual add, ReLU and the
// heads stay fp32. Same device code as the split forms (a template argument), same LDS / HBM geometry with the low slots unused.
// NOT fp32-equivalent: about 5e-3 in a logit on a realistic network. The reference's network is
// model.py:6-31,76-104 (PVNet, ResBlock).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/omok_hip.h"
#include "engine_types.hpp"
#include "net_device.hpp"
#include "net_common.hpp"
#include "net_trunk_f32.hpp"
#include "net_trunk_h16.hpp"
#include "net_board_h16.hpp"
#include "net_f16.hpp"

namespace ao {

#if AO_KO == 0 && AO_BKO == 0 && !AO_CONV1_SPLIT

namespace {
constexpr int kDev = 16;
// dynamic-LDS attribute set once per (device, kernel)
bool g_attr_trunk[kDev][16][2], g_attr_board[kDev][16][2];

template <typename K>
hipError_t set_lds(bool* done, K kernel, size_t lds) {
    if (*done) return hipSuccess;
    const hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (st == hipSuccess) *done = true;
    return st;
}
}  // namespace

hipError_t launch_trunk16h_f16(int device, int B, int in_kind, int groups, hipStream_t s, const TrunkHArgs& a) {
    if (device < 0 || device >= kDev) return hipErrorInvalidDevice;
    const int k = in_kind == 2 ? 1 : 0;
    switch (B) {
#define AO_BW_CASE(W)                                                                                                  \
    case W: {                                                                                                          \
        constexpr size_t heads_ = (static_cast<size_t>(3) * 128 + 16 * 3 * W * W + 8 * 16 * W * W + 8 * 16 * 128) * 4; \
        constexpr size_t rows_ = static_cast<size_t>(2) * W * 4 * 2 * 1024 + 64;                                       \
        constexpr size_t lds_ = (rows_ > heads_) ? rows_ : heads_;                                                     \
        hipError_t st = k ? set_lds(&g_attr_trunk[device][W][1], &k_trunk16hb_f16<W, 4, 0>, lds_)                      \
                          : set_lds(&g_attr_trunk[device][W][0], &k_trunk16h_f16<W, 4, 0>, lds_);                      \
        if (st != hipSuccess) return st;                                                                               \
        if (k) hipLaunchKernelGGL((k_trunk16hb_f16<W, 4, 0>), dim3(groups), dim3(512), lds_, s, a);                    \
        else hipLaunchKernelGGL((k_trunk16h_f16<W, 4, 0>), dim3(groups), dim3(512), lds_, s, a);                       \
    } break;
        AO_BW_CASE(3) AO_BW_CASE(4) AO_BW_CASE(5) AO_BW_CASE(6) AO_BW_CASE(7) AO_BW_CASE(8) AO_BW_CASE(9)
#undef AO_BW_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_boardh_f16(int device, int B, bool bits, dim3 grid, hipStream_t s, const BoardHArgs& a) {
    if (device < 0 || device >= kDev) return hipErrorInvalidDevice;
    switch (B) {
#define AO_BW_CASE(W)                                                                                                  \
    case W: {                                                                                                          \
        constexpr size_t lds_ = static_cast<size_t>(W) * 8 * 1024;                                                     \
        hipError_t st = bits ? set_lds(&g_attr_board[device][W][1], &k_boardh_f16<W, 2>, lds_)                         \
                             : set_lds(&g_attr_board[device][W][0], &k_boardh_f16<W, 1>, lds_);                        \
        if (st != hipSuccess) return st;                                                                               \
        if (bits) hipLaunchKernelGGL((k_boardh_f16<W, 2>), grid, dim3(512), lds_, s, a);                               \
        else hipLaunchKernelGGL((k_boardh_f16<W, 1>), grid, dim3(512), lds_, s, a);                                    \
    } break;
        AO_BW_CASE(10) AO_BW_CASE(11) AO_BW_CASE(12) AO_BW_CASE(13) AO_BW_CASE(14) AO_BW_CASE(15)
#undef AO_BW_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

#else   // timing knock-outs and the measured-neutral conv1 variant are experiments on the split forms only

hipError_t launch_trunk16h_f16(int, int, int, int, hipStream_t, const TrunkHArgs&) { return hipErrorNotSupported; }
hipError_t launch_boardh_f16(int, int, bool, dim3, hipStream_t, const BoardHArgs&) { return hipErrorNotSupported; }

#endif

}  // namespace ao
