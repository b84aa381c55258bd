// Backward of the 3x3 / stride-1 / 64 -> 64 'same' convolution (the 90 convs of the ResidualBlock_noBN trunks,
// module_util.py:34-52): the weight / bias gradient kernel and the Winograd weight packer on the device.  The data
// gradient needs no kernel of its own: it is stif_conv3x3_wino with the weight packed by
// stif_pack_conv_weight_dev(..., STIF_PACK_DGRAD) (transposed and rotated), DESIGN.md section 3j.
#include <algorithm>

#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

namespace {

// ---- weight gradient: gw[co][ci][kh][kw] = sum_{n,y,x} gy[n][y][x][co] * x[n][y+kh-1][x+kw-1][ci] ----
//
// A workgroup stages a TH x TW tile of gy and the matching x tile with its one-pixel halo in LDS (pixels outside
// the map are zeros, so partial tiles and the padding need no special case) and contracts over the tile's pixels
// on fp32 MFMA: D[co 32][ci 32] += A[co][pixel pair] * B[pixel pair][ci], A = the gy tile, B = the x tile shifted
// by the tap.  Wave w owns cout tile w >> 1 and cin tile w & 1 for all nine taps: 9 x 16 accumulator registers,
// kept across every tile the workgroup takes (static schedule: tiles b, b + G, b + 2G, ...).  One k step reads one
// gy value and nine x values per lane (ds_read_b32, lanes 0..31 on 32 consecutive channels: conflict-free) for
// nine MFMAs of 64 cycles each, so the loop is paced by the matrix pipe.  Two workgroups per CU: one fills its
// tile while the other computes.
#ifndef STIF_WGRAD_TH          // tile rows and workgroups per CU: overridable for A/B builds
#define STIF_WGRAD_TH 2
#define STIF_WGRAD_WG_PER_CU 2
#endif
constexpr int TH = STIF_WGRAD_TH, TW = 32;
constexpr int XH = TH + 2, XW = TW + 2;
constexpr int WG_PER_CU = STIF_WGRAD_WG_PER_CU;
constexpr int GW_FLOATS = 64 * 64 * 9;
constexpr int PART = GW_FLOATS + 64;   // one workgroup's partial: [tap 9][co 64][ci 64] then the 64 bias sums

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WG_PER_CU)))
void k_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ ws, long long x_item,
             long long gy_item, int H, int W, int tiles_x, int tiles_per_item, int ntiles) {
  __shared__ __attribute__((aligned(16))) float s_x[XH * XW * 64];
  __shared__ __attribute__((aligned(16))) float s_gy[TH * TW * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cot = wave >> 1, cit = wave & 1, l32 = lane & 31, hf = lane >> 5;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;   // sum of this lane's gy values: cout cot * 32 + l32, pixels of parity hf

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int n = t / tiles_per_item, rem = t - n * tiles_per_item, ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const float* xi = x + (size_t)n * x_item;
    const float* gi = gy + (size_t)n * gy_item;
    __syncthreads();   // the previous tile's reads are done
#pragma unroll
    for (int k = 0; k < (XH * XW * 16 + 255) / 256; ++k) {
      const int i = tid + k * 256;
      if (i < XH * XW * 16) {
        const int c4 = i & 15, p = i >> 4, py = p / XW, px = p - py * XW;
        const int yy = y0 + py - 1, xx = x0 + px - 1;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = ld4(xi + ((size_t)yy * W + xx) * 64 + c4 * 4);
        st4(s_x + p * 64 + c4 * 4, v);
      }
    }
#pragma unroll
    for (int k = 0; k < TH * TW * 16 / 256; ++k) {
      const int i = tid + k * 256;
      const int c4 = i & 15, p = i >> 4, py = p / TW, px = p - py * TW;
      const int yy = y0 + py, xx = x0 + px;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (yy < H && xx < W) v = ld4(gi + ((size_t)yy * W + xx) * 64 + c4 * 4);
      st4(s_gy + p * 64 + c4 * 4, v);
    }
    __syncthreads();
    // k step (r, xs): pixels (r, 2 xs + hf) of the tile; tap (kh, kw) reads x tile pixel (r + kh, 2 xs + hf + kw)
    const float* ap = s_gy + hf * 64 + cot * 32 + l32;
    const float* bp = s_x + hf * 64 + cit * 32 + l32;
#pragma unroll
    for (int r = 0; r < TH; ++r) {
#pragma unroll 2
      for (int xs = 0; xs < TW / 2; ++xs) {
        const float a = ap[(r * TW + 2 * xs) * 64];
        bsum += a;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw)
            acc[kh * 3 + kw] = mfma32(a, bp[((r + kh) * XW + 2 * xs + kw) * 64], acc[kh * 3 + kw]);
      }
    }
  }

  float* part = ws + (size_t)blockIdx.x * PART;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      part[t * 4096 + (cot * 32 + mfma_row(r, lane)) * 64 + cit * 32 + l32] = acc[t][r];
  const float other = __shfl_xor(bsum, 32);
  if (cit == 0 && hf == 0) part[GW_FLOATS + cot * 32 + l32] = bsum + other;
}

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

long long wgrad_tiles(int n, int H, int W) { return (long long)n * ((H + TH - 1) / TH) * ((W + TW - 1) / TW); }
// workgroups launched = partials reduced: a function of the shape and the device's CU count alone
int wgrad_grid(long long tiles) { return (int)std::min<long long>(tiles, (long long)WG_PER_CU * stif_num_cus()); }

// ---- Winograd weight packing on the device: the bytes of pack.cpp's pack_wino / pack_wino_f16x3 ----

// U = G g G^T in double with pack.cpp's wino_u addition order; every product is by 0, +-0.5 or 1 and therefore
// exact, so a contracted multiply-add rounds the same sum
__device__ void wino_u_dev(const float* g, double u[4][4]) {
  const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  double t[4][3];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int q = 0; q < 3; ++q) t[a][q] = G[a][0] * g[q] + G[a][1] * g[3 + q] + G[a][2] * g[6 + q];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) u[a][b] = t[a][0] * G[b][0] + t[a][1] * G[b][1] + t[a][2] * G[b][2];
}

// one thread per (packed cout, packed cin) of the 64 -> 64 weight; dgrad: the data gradient's weight
// w'[ci][co][kh][kw] = w[co][ci][2 - kh][2 - kw] with a zero bias
__global__ __launch_bounds__(256) void k_pack_wino(const float* __restrict__ w, const float* __restrict__ b,
                                                   float* __restrict__ w_dst, float* __restrict__ b_dst, int* status,
                                                   int f16, int dgrad) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int co = idx >> 6, ci = idx & 63;
  const float* src = w + (size_t)(dgrad ? ci * 64 + co : co * 64 + ci) * 9;
  float g[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) g[q] = src[dgrad ? 8 - q : q];
  double u[4][4];
  wino_u_dev(g, u);
  const int nt = co >> 5, l = (co & 31) + 32 * ((ci >> 2) & 1);
  if (!f16) {
    const int c = ci >> 3, e = ci & 3;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) w_dst[(((((size_t)c * 4 + i) * 4 + j) * 2 + nt) * 64 + l) * 4 + e] = (float)u[i][j];
  } else {
    const int q = ci >> 4, e = 4 * ((ci >> 3) & 1) + (ci & 3);
    _Float16* dst = reinterpret_cast<_Float16*>(w_dst);
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bad |= !(u[i][j] >= -65504.0 / 1024.0 && u[i][j] <= 65504.0 / 1024.0);
        const double v = u[i][j] * 1024.0;
        const _Float16 h = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (double)h);
        const size_t o = (((((size_t)q * 4 + i) * 4 + j) * 2 + nt) * 2) * 512 + l * 8 + e;
        dst[o] = h;
        dst[o + 512] = lo;
      }
    if (bad) atomicOr(status, STIF_STATUS_PACK_RANGE);
  }
  if (ci == 0) b_dst[co] = (dgrad || b == nullptr) ? 0.f : b[co];
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" size_t stif_conv3x3_wgrad_workspace_size(int n, int H, int W, int cin, int cout) {
  if (n < 1 || H < 1 || W < 1 || cin != 64 || cout != 64) return 0;
  const long long tiles = wgrad_tiles(n, H, W);
  if (tiles > 0x7fffffffLL) return 0;
  return (size_t)wgrad_grid(tiles) * PART * sizeof(float);
}

extern "C" int stif_conv3x3_wgrad(const stif_conv_wgrad_args* pa, void* stream) {
  if (!pa) return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: null args");
  const stif_conv_wgrad_args& a = *pa;
  if (!a.x || !a.gy || !a.gw) return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: null pointer (x, gy, gw)");
  if (a.n < 1 || a.H < 1 || a.W < 1) return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: n, H, W must be >= 1");
  if (a.cin != 64 || a.cout != 64)
    return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: unsupported channel counts (64 -> 64 only)");
  if (a.x_item < 0 || a.gy_item < 0) return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: negative item stride");
  if ((long long)a.H * a.W * 64 * 4 >= 0x7fffffffLL)
    return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: item larger than 2 GB (buffer addressing)");
  if (misaligned16(a.x) || misaligned16(a.gy) || a.x_item % 4 || a.gy_item % 4)
    return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: x / gy and their item strides must be 16-byte aligned");
  const long long tiles = wgrad_tiles(a.n, a.H, a.W);
  if (tiles > 0x7fffffffLL) return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: too many tiles");
  const int G = wgrad_grid(tiles);
  if (!a.workspace || a.workspace_bytes < (size_t)G * PART * sizeof(float))
    return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: workspace too small (stif_conv3x3_wgrad_workspace_size)");
  if (misaligned16(a.workspace))
    return stif_fail(STIF_E_INVALID, "stif_conv3x3_wgrad: workspace not 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int tiles_x = (a.W + TW - 1) / TW, tiles_per_item = tiles_x * ((a.H + TH - 1) / TH);
  float* ws = static_cast<float*>(a.workspace);
  hipLaunchKernelGGL(k_wgrad, dim3(G), dim3(256), 0, st, a.x, a.gy, ws, a.x_item, a.gy_item, a.H, a.W, tiles_x,
                     tiles_per_item, (int)tiles);
  if (int rc = stif_check_launch("stif_conv3x3_wgrad")) return rc;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((PART + 255) / 256), dim3(256), 0, st, ws, G, a.gw, a.gb);
  return stif_check_launch("stif_conv3x3_wgrad (reduce)");
}

extern "C" int stif_pack_conv_weight_dev(const float* w_oihw, const float* b, int cout, int cin, int ks, int mode,
                                         int flags, float* w_dst, float* b_dst, int* status, void* stream) {
  if (!w_oihw || !w_dst || !b_dst)
    return stif_fail(STIF_E_INVALID, "stif_pack_conv_weight_dev: null pointer (w_oihw, w_dst, b_dst)");
  if (mode != STIF_PACK_WINO && mode != (STIF_PACK_WINO | STIF_PACK_F16X3))
    return stif_fail(STIF_E_INVALID, "stif_pack_conv_weight_dev: unsupported mode (STIF_PACK_WINO [| STIF_PACK_F16X3] only)");
  if (ks != 3) return stif_fail(STIF_E_INVALID, "stif_pack_conv_weight_dev: winograd pack needs a 3x3 kernel");
  if (cin != 64 || cout != 64)
    return stif_fail(STIF_E_INVALID, "stif_pack_conv_weight_dev: unsupported channel counts (64 -> 64 only)");
  if (flags & ~STIF_PACK_DGRAD) return stif_fail(STIF_E_INVALID, "stif_pack_conv_weight_dev: unknown flags");
  const bool dgrad = (flags & STIF_PACK_DGRAD) != 0, f16 = (mode & STIF_PACK_F16X3) != 0;
  if (!b && !dgrad)
    return stif_fail(STIF_E_INVALID, "stif_pack_conv_weight_dev: null bias (allowed with STIF_PACK_DGRAD only)");
  if (f16 && !status)
    return stif_fail(STIF_E_INVALID, "stif_pack_conv_weight_dev: STIF_PACK_F16X3 needs a status word (range report)");
  hipLaunchKernelGGL(k_pack_wino, dim3(16), dim3(256), 0, static_cast<hipStream_t>(stream), w_oihw, b, w_dst, b_dst,
                     status, f16 ? 1 : 0, dgrad ? 1 : 0);
  return stif_check_launch("stif_pack_conv_weight_dev");
}
