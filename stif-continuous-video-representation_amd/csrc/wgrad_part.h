// The partial-sum layout of the 64 -> 64 3x3 weight-gradient kernels and its reduction (device only): every
// persistent workgroup writes one PART-sized partial per 64 x 64 channel block, a second launch adds each block's G
// partials in index order.  Shared by the conv weight gradient (conv_bwd.hip) and the deformable conv's (dcn_bwd.hip).
#pragma once
#include "stif_common.h"

namespace {

constexpr int GW_FLOATS = 64 * 64 * 9;
constexpr int PART = GW_FLOATS + 64;   // one workgroup's partial: [tap 9][co 64][ci 64] then the 64 bias sums

// gw / gb of every 64 x 64 block = its G partials summed in index order.  blockIdx.y = slice * nx + xi is the block of
// cout slice `slice` against input map xi, its partials block-major in the workspace; gw is stored OIHW with rows of
// 64 nx input channels, rows at or past cout are skipped, gb comes from the blocks of map 0.  The 64 -> 64 weight
// gradients are (nx, cout) = (1, 64) on a grid of one block.
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float* __restrict__ ws, int G, float* __restrict__ gw,
                                                      float* __restrict__ gb, int nx, int cout) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= PART) return;
  const int blk = blockIdx.y, slice = blk / nx, xi = blk - slice * nx;
  const float* p = ws + (size_t)blk * G * PART;
  float s = 0.f;
#pragma unroll 8
  for (int g = 0; g < G; ++g) s += p[(size_t)g * PART + idx];
  if (idx < GW_FLOATS) {
    const int tap = idx >> 12, co = slice * 64 + ((idx >> 6) & 63), ci = xi * 64 + (idx & 63);
    if (co < cout) gw[((size_t)co * 64 * nx + ci) * 9 + tap] = s;
  } else if (gb != nullptr && xi == 0) {
    const int co = slice * 64 + idx - GW_FLOATS;
    if (co < cout) gb[co] = s;
  }
}

}  // namespace
