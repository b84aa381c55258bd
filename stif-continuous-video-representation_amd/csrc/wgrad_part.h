// The partial-sum layout of the 64 -> 64 3x3 weight-gradient kernels and its reduction (device only): every
// persistent workgroup writes one PART-sized partial, a second launch adds the G partials in index order.  Shared by
// the conv weight gradient (conv_bwd.hip) and the deformable conv's (dcn_bwd.hip).
#pragma once
#include "stif_common.h"

namespace {

constexpr int GW_FLOATS = 64 * 64 * 9;
constexpr int PART = GW_FLOATS + 64;   // one workgroup's partial: [tap 9][co 64][ci 64] then the 64 bias sums

// gw / gb = the G partials summed in index order; gw stored OIHW
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ ws, int G, float* __restrict__ gw,
                                                      float* __restrict__ gb) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= PART) return;
  float s = 0.f;
#pragma unroll 8
  for (int g = 0; g < G; ++g) s += ws[(size_t)g * PART + idx];
  if (idx < GW_FLOATS) {
    const int tap = idx >> 12, co = (idx >> 6) & 63, ci = idx & 63;
    gw[(co * 64 + ci) * 9 + tap] = s;
  } else if (gb != nullptr) {
    gb[idx - GW_FLOATS] = s;
  }
}

}  // namespace
