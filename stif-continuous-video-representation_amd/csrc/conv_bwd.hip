// Backward of the 3x3 / stride-1 / 64 -> 64 'same' convolution (the 90 convs of the ResidualBlock_noBN trunks,
// module_util.py:34-52): the weight / bias gradient kernel and the Winograd weight packer on the device.  The data
// gradient needs no kernel of its own: it is stif_conv3x3_wino with the weight packed by
// stif_pack_conv_weight_dev(..., STIF_PACK_DGRAD) (transposed and rotated), DESIGN.md section 3j.
// And the backward of the frame encoder's other three convs: the weight gradient of the
// stride-2 convs (the same kernel, a template on the stride), their data gradient (a transposed conv, split by output
// parity), the weight gradient of conv_first (3 -> 64), and the STIF_PACK_PLAIN packer on the device.
// And what PCD_Align's backward lacked: the weight gradient in 64 x 64 channel blocks (the
// 128 -> 64 concatenation convs, the 64 -> 216 offset / mask conv), the adjoint of the x2 bilinear upsample, and the
// Winograd packer for a 64 x 64 block of a wider weight.
// The ConvLSTM cell's 128 -> 256 conv is eight more such blocks: (nx, gy_channels, cout) =
// (2, 256, 256) in the block weight gradient, a [256][128] weight in the block packer.
// The weight-gradient entries share one device body (wgrad_walk: k_wgrad<S> and k_wgrad_cat only pick their pointers
// and their gy view), one reduce (k_wgrad_reduce in wgrad_part.h, by block) and one checked launch (wgrad_run); the two
// Winograd device packers share pack_wino_run.
#include <algorithm>
#include <cstdio>

#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"
#include "wgrad_part.h"

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
// The tile of stride S (1: 'same', 2: the pyramid's down-sampling convs, pad 1): TH x TW output (gy) pixels and the
// S (TH - 1) + 3 rows x S (TW - 1) + 3 columns of x they read.  Stride 2 halves TW so that both tiles stay at
// ~50 KB (42,240 + 8,192 B) and two workgroups still share a CU.
template <int S>
struct WgradTile {
  static constexpr int TH = S == 1 ? STIF_WGRAD_TH : 2, TW = S == 1 ? 32 : 16;
  static constexpr int XH = S * (TH - 1) + 3, XW = S * (TW - 1) + 3;
};
constexpr int WG_PER_CU = STIF_WGRAD_WG_PER_CU;
// GW_FLOATS, PART (one workgroup's partial) and k_wgrad_reduce: wgrad_part.h

// The gy map a walk reads.  GyPlain: [Ho][Wo][64], every channel live -- pitch, offset and limit fold to constants.
// GySlice: 64 channels from co0 of a pixel pitch of gc floats; channels at or past cout are zeros in LDS, never loaded.
struct GyPlain {
  __device__ int pitch() const { return 64; }
  __device__ int offset() const { return 0; }
  __device__ bool live(int) const { return true; }
};
struct GySlice {
  int gc, co0, cout;
  __device__ int pitch() const { return gc; }
  __device__ int offset() const { return co0; }
  __device__ bool live(int c) const { return co0 + c < cout; }
};

// The tile walk of one 64 x 64 channel block: x is [H][W][64] per item, gy [Ho][Wo][view] -- the tiles walk gy -- and
// the workgroup's partial is the one of block `blk` (block-major in the workspace).
template <int S, class GyView>
__device__ __forceinline__ void wgrad_walk(const int tid, const GyView v, const float* x, const float* gy, float* ws,
                                           int blk, long long x_item, long long gy_item, int H, int W, int Ho, int Wo,
                                           int tiles_x, int tiles_per_item, int ntiles) {
  constexpr int TH = WgradTile<S>::TH, TW = WgradTile<S>::TW, XH = WgradTile<S>::XH, XW = WgradTile<S>::XW;
  __shared__ __attribute__((aligned(16))) float s_x[XH * XW * 64];
  __shared__ __attribute__((aligned(16))) float s_gy[TH * TW * 64];
  const int lane = tid & 63, wave = tid >> 6;
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
        const int yy = S * y0 + py - 1, xx = S * x0 + px - 1;
        f32x4 v4 = {0.f, 0.f, 0.f, 0.f};
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) v4 = ld4(xi + ((size_t)yy * W + xx) * 64 + c4 * 4);
        st4(s_x + p * 64 + c4 * 4, v4);
      }
    }
#pragma unroll
    for (int k = 0; k < TH * TW * 16 / 256; ++k) {
      const int i = tid + k * 256;
      const int c4 = i & 15, p = i >> 4, py = p / TW, px = p - py * TW;
      const int yy = y0 + py, xx = x0 + px;
      f32x4 v4 = {0.f, 0.f, 0.f, 0.f};
      if (yy < Ho && xx < Wo && v.live(c4 * 4)) v4 = ld4(gi + ((size_t)yy * Wo + xx) * v.pitch() + v.offset() + c4 * 4);
      st4(s_gy + p * 64 + c4 * 4, v4);
    }
    __syncthreads();
    // k step (r, xs): gy pixels (r, 2 xs + hf) of the tile; tap (kh, kw) reads x tile pixel
    // (S r + kh, S (2 xs + hf) + kw)
    const float* ap = s_gy + hf * 64 + cot * 32 + l32;
    const float* bp = s_x + S * hf * 64 + cit * 32 + l32;
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
            acc[kh * 3 + kw] = mfma32(a, bp[((S * r + kh) * XW + S * 2 * xs + kw) * 64], acc[kh * 3 + kw]);
      }
    }
  }

  float* part = ws + ((size_t)blk * gridDim.x + blockIdx.x) * PART;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      part[t * 4096 + (cot * 32 + mfma_row(r, lane)) * 64 + cit * 32 + l32] = acc[t][r];
  const float other = __shfl_xor(bsum, 32);
  if (cit == 0 && hf == 0) part[GW_FLOATS + cot * 32 + l32] = bsum + other;
}

template <int S>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WG_PER_CU)))
void k_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ ws, long long x_item,
             long long gy_item, int H, int W, int Ho, int Wo, int tiles_x, int tiles_per_item, int ntiles) {
  wgrad_walk<S>(threadIdx.x, GyPlain{}, x, gy, ws, 0, x_item, gy_item, H, W, Ho, Wo, tiles_x, tiles_per_item, ntiles);
}

// The weight gradient in 64 x 64 channel blocks: blockIdx.y = slice * nx + xi is the block of
// cout slice `slice` (gy channels 64 slice .. of a pixel pitch of gc floats) against the input map x[xi].  Every block
// is k_wgrad<1>'s walk -- the same tiles, grid, staging and k order, one partial per workgroup and block (block-major
// in the workspace) -- so its sums are the bits stif_conv3x3_wgrad computes for the same two 64-channel maps.  The x
// tile is staged once per block (four times for the 216 form): the loop is MFMA-paced.
struct WgradCat {
  const float* x[2];
  long long x_item[2];
  int nx, gc, cout;
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WG_PER_CU)))
void k_wgrad_cat(WgradCat c, const float* __restrict__ gy, float* __restrict__ ws, long long gy_item, int H, int W,
                 int tiles_x, int tiles_per_item, int ntiles) {
  const int blk = blockIdx.y, slice = blk / c.nx, xi = blk - slice * c.nx;
  wgrad_walk<1>(threadIdx.x, GySlice{c.gc, slice * 64, c.cout}, xi ? c.x[1] : c.x[0], gy, ws, blk,
                xi ? c.x_item[1] : c.x_item[0], gy_item, H, W, H, W, tiles_x, tiles_per_item, ntiles);
}

// tiles over the gy map of an x of H x W (stride 2: Ho = (H + 1) / 2, Wo = (W + 1) / 2)
template <int S>
long long wgrad_tiles(int n, int H, int W) {
  constexpr int TH = WgradTile<S>::TH, TW = WgradTile<S>::TW;
  const int Ho = (H + S - 1) / S, Wo = (W + S - 1) / S;
  return (long long)n * ((Ho + TH - 1) / TH) * ((Wo + TW - 1) / TW);
}
// workgroups launched = partials reduced: a function of the shape and the device's CU count alone
int wgrad_grid(long long tiles) { return (int)std::min<long long>(tiles, (long long)WG_PER_CU * stif_num_cus()); }

template <int S>
size_t wgrad_workspace_size(int n, int H, int W, int cin, int cout) {
  if (n < 1 || H < 1 || W < 1 || cin != 64 || cout != 64) return 0;
  const long long tiles = wgrad_tiles<S>(n, H, W);
  if (tiles > 0x7fffffffLL) return 0;
  return (size_t)wgrad_grid(tiles) * PART * sizeof(float);
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

int fail_as(const char* fn, const char* why) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  return stif_fail(STIF_E_INVALID, msg);
}

// the (cout slice, x map) blocks of a supported (nx, gy_channels, cout), 0 for anything else
int wgrad_cat_blocks(int nx, int gy_channels, int cout) {
  if (gy_channels == 64 && cout == 64 && (nx == 1 || nx == 2)) return nx;
  if (gy_channels == 256 && cout == 216 && nx == 1) return 4;
  if (gy_channels == 256 && cout == 256 && nx == 2) return 8;   // the ConvLSTM cell's 128 -> 256 conv
  return 0;
}

// Every weight-gradient entry: the checks, then the walk and the reduce.  `a` is the block form's arguments (the
// 64 -> 64 entries are its (1, 64, 64) case), `blocks` its block count or 0 for unsupported channel counts (`chans`
// says which are supported), `ptrs` names the pointers that must not be null; `fn` prefixes every message.  cat:
// k_wgrad_cat over the blocks (stride 1 only: it is k_wgrad<1>'s walk, so S = 1 with it), otherwise k_wgrad<S>.
template <int S>
int wgrad_run(const char* fn, const stif_conv_wgrad_cat_args& a, int blocks, bool cat, const char* ptrs,
              const char* chans, void* stream) {
  constexpr int TH = WgradTile<S>::TH, TW = WgradTile<S>::TW;
  char msg[160];
  if (!a.x[0] || !a.gy || !a.gw) return fail_as(fn, ptrs);
  if (a.n < 1 || a.H < 1 || a.W < 1) return fail_as(fn, "n, H, W must be >= 1");
  if (!blocks) return fail_as(fn, chans);
  const bool two = a.nx == 2;
  if (two && !a.x[1]) return fail_as(fn, "null pointer (x[1] with nx = 2)");
  if (a.x_item[0] < 0 || (two && a.x_item[1] < 0) || a.gy_item < 0) return fail_as(fn, "negative item stride");
  if ((long long)a.H * a.W * a.gy_channels * 4 >= 0x7fffffffLL)
    return fail_as(fn, "item larger than 2 GB (buffer addressing)");
  if (misaligned16(a.x[0]) || (two && misaligned16(a.x[1])) || misaligned16(a.gy) || a.x_item[0] % 4 ||
      (two && a.x_item[1] % 4) || a.gy_item % 4)
    return fail_as(fn, "x / gy and their item strides must be 16-byte aligned");
  const long long tiles = wgrad_tiles<S>(a.n, a.H, a.W);
  if (tiles > 0x7fffffffLL) return fail_as(fn, "too many tiles");
  const int G = wgrad_grid(tiles);
  if (!a.workspace || a.workspace_bytes < (size_t)blocks * G * PART * sizeof(float)) {
    snprintf(msg, sizeof msg, "workspace too small (%s_workspace_size)", fn);
    return fail_as(fn, msg);
  }
  if (misaligned16(a.workspace)) return fail_as(fn, "workspace not 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int Ho = (a.H + S - 1) / S, Wo = (a.W + S - 1) / S;
  const int tiles_x = (Wo + TW - 1) / TW, tiles_per_item = tiles_x * ((Ho + TH - 1) / TH);
  float* ws = static_cast<float*>(a.workspace);
  if (cat) {
    WgradCat c{{a.x[0], two ? a.x[1] : a.x[0]}, {a.x_item[0], two ? a.x_item[1] : a.x_item[0]}, a.nx, a.gy_channels,
               a.cout};
    hipLaunchKernelGGL(k_wgrad_cat, dim3(G, blocks), dim3(256), 0, st, c, a.gy, ws, a.gy_item, a.H, a.W, tiles_x,
                       tiles_per_item, (int)tiles);
  } else {
    hipLaunchKernelGGL(k_wgrad<S>, dim3(G), dim3(256), 0, st, a.x[0], a.gy, ws, a.x_item[0], a.gy_item, a.H, a.W, Ho,
                       Wo, tiles_x, tiles_per_item, (int)tiles);
  }
  if (int rc = stif_check_launch(fn)) return rc;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3((PART + 255) / 256, blocks), dim3(256), 0, st, ws, G, a.gw, a.gb, a.nx,
                     a.cout);
  snprintf(msg, sizeof msg, "%s (reduce)", fn);
  return stif_check_launch(msg);
}

// the 64 -> 64 entry of stride S
template <int S>
int wgrad_entry(const char* fn, const stif_conv_wgrad_args* pa, void* stream) {
  if (!pa) return fail_as(fn, "null args");
  stif_conv_wgrad_cat_args a{};
  a.x[0] = pa->x, a.gy = pa->gy, a.gw = pa->gw, a.gb = pa->gb;
  a.x_item[0] = pa->x_item, a.gy_item = pa->gy_item;
  a.n = pa->n, a.H = pa->H, a.W = pa->W, a.nx = 1, a.gy_channels = 64, a.cout = 64;
  a.workspace = pa->workspace, a.workspace_bytes = pa->workspace_bytes;
  return wgrad_run<S>(fn, a, pa->cin == 64 && pa->cout == 64, false, "null pointer (x, gy, gw)",
                      "unsupported channel counts (64 -> 64 only)", stream);
}

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

// one thread per (packed cout, packed cin) of a 64 -> 64 pack: the block of rows co0.. and columns ci0.. of the OIHW
// weight [cout][cin][3][3] (the whole weight for cout = cin = 64), rows at or past cout reading as zeros; dgrad:
// the data gradient's weight of that block, w'[ci][co][kh][kw] = w[co0 + co][ci0 + ci][2 - kh][2 - kw], and a zero
// bias
__global__ __launch_bounds__(256) void k_pack_wino(const float* __restrict__ w, const float* __restrict__ b,
                                                   float* __restrict__ w_dst, float* __restrict__ b_dst, int* status,
                                                   int f16, int dgrad, int cout, int cin, int co0, int ci0) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int co = idx >> 6, ci = idx & 63;
  const int row = co0 + (dgrad ? ci : co), col = ci0 + (dgrad ? co : ci);
  const float* src = w + ((size_t)row * cin + col) * 9;
  float g[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) g[q] = row < cout ? src[dgrad ? 8 - q : q] : 0.f;
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
  if (ci == 0) b_dst[co] = (dgrad || b == nullptr || co0 + co >= cout) ? 0.f : b[co0 + co];
}

// ---- the adjoint of the x2 bilinear upsample (align_corners = False), gather form ----
//
// Along an axis output 2 i is 0.25 x[i - 1] + 0.75 x[i] and output 2 i + 1 is 0.75 x[i] + 0.25 x[i + 1], with the
// neighbour clamped into the map at the two borders.  So x[i] receives 0.25, 0.75, 0.75, 0.25 of g[2 i - 1 .. 2 i + 2],
// and the clamped border's extra 0.25 g[0] (i = 0) and 0.25 g[2 n - 1] (i = n - 1) are exactly the out-of-range taps
// with their index clamped into [0, 2 n): one rule for every pixel, n = 1 included.  One thread owns four channels of
// one gx pixel: 16 float4 loads of gy (4 x 4 window, columns first), a fixed addition order, no atomics.
// grid (x blocks over w1 * c / 4, gx row, item)
__global__ __launch_bounds__(256) void k_up2_bwd(const float* __restrict__ gy, float* __restrict__ gx, int h1, int w1,
                                                 int c, float scale, long long gy_item, long long gx_item) {
  const int c4n = c >> 2, i = blockIdx.y, item = blockIdx.z;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= w1 * c4n) return;
  const int j = t / c4n, q = t - j * c4n, H = 2 * h1, W = 2 * w1;
  const float* src = gy + (size_t)item * gy_item + q * 4;
  int cols[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) cols[b] = min(max(2 * j - 1 + b, 0), W - 1);
  f32x4 r[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float* row = src + (size_t)min(max(2 * i - 1 + a, 0), H - 1) * W * c;
    const f32x4 v0 = ld4(row + (size_t)cols[0] * c), v1 = ld4(row + (size_t)cols[1] * c);
    const f32x4 v2 = ld4(row + (size_t)cols[2] * c), v3 = ld4(row + (size_t)cols[3] * c);
    r[a] = 0.25f * (v0 + v3) + 0.75f * (v1 + v2);
  }
  const f32x4 v = (0.25f * (r[0] + r[3]) + 0.75f * (r[1] + r[2])) * scale;
  st4(gx + (size_t)item * gx_item + ((size_t)i * w1 + j) * c + q * 4, v);
}

// ---- the direct-conv (STIF_PACK_PLAIN) packing on the device: the bytes of pack.cpp's plain loop, 64 -> 64 3x3 ----
// [chunk 8][tap 9][nt 2][lane 64][4]: one thread per destination element (a pure permutation)
__global__ __launch_bounds__(256) void k_pack_plain(const float* __restrict__ w, const float* __restrict__ b,
                                                    float* __restrict__ w_dst, float* __restrict__ b_dst) {
  const int idx = blockIdx.x * 256 + threadIdx.x;   // < 8 * 9 * 2 * 64 * 4 = 36864 = 144 blocks
  const int e = idx & 3, l = (idx >> 2) & 63, nt = (idx >> 8) & 1, ct = idx >> 9, c = ct / 9, t = ct - c * 9;
  const int co = nt * 32 + (l & 31), ci = c * 8 + 4 * (l >> 5) + e;
  w_dst[idx] = w[(co * 64 + ci) * 9 + t];
  if (idx < 64) b_dst[idx] = b == nullptr ? 0.f : b[idx];
}

// ---- stride-2 data gradient: gx = the transposed conv of gy, split by the parity of the gx pixel ----
//
// gx pixel (2 i + py, 2 j + px) takes tap (1, 1) of gy pixel (i, j) for (py, px) = (0, 0); taps (1, 0) / (1, 2) of
// (i, j + 1) / (i, j) for (0, 1); taps (0, 1) / (2, 1) of (i + 1, j) / (i, j) for (1, 0); and taps (0, 0), (0, 2),
// (2, 0), (2, 2) of (i + 1, j + 1), (i + 1, j), (i, j + 1), (i, j) for (1, 1): nine tap-GEMMs per gy pixel, the
// forward's multiply-adds, none on an inserted zero.  A workgroup stages DG_TH x DG_TW gy pixels with one halo row
// and column (zeros outside the map) in LDS, pixel-major with a 65-float pitch so that the 32 lanes of an A read
// (32 consecutive pixels, one cout) fall on 32 banks.  Wave w owns row w of the tile: 32 gy pixels x 4 phases x 2
// cin tiles = 128 accumulator registers.  The contraction runs over cout on fp32 MFMA, D[pixel 32][ci 32] +=
// A[pixel][co pair] * B[co pair][ci]; the raw OIHW weight streams through LDS in chunks of DG_CO couts
// ([tap][co][ci], transposed by the copy; 516-float tap pitch keeps the transposing writes to two per bank),
// double-buffered: the next chunk is fetched into registers before the current one is consumed.
constexpr int DG_TH = 4, DG_TW = 32, DG_GH = DG_TH + 1, DG_GW = DG_TW + 1, DG_PX = 65;
constexpr int DG_CO = 8, DG_TAP = DG_CO * 64 + 4, DG_CHUNK = DG_CO * 64 * 9, DG_LD = DG_CHUNK / 256;

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void k_dgrad_s2(const float* __restrict__ gy, const float* __restrict__ w, float* __restrict__ gx, long long gy_item,
                long long gx_item, int H, int W, int Ho, int Wo, int tiles_x, int tiles_per_item) {
  __shared__ float s_gy[DG_GH * DG_GW * DG_PX];
  __shared__ float s_w[2][9 * DG_TAP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hf = lane >> 5;
  const int t = blockIdx.x, n = t / tiles_per_item, rem = t - n * tiles_per_item, ty = rem / tiles_x;
  const int i0 = ty * DG_TH, j0 = (rem - ty * tiles_x) * DG_TW;
  const float* gi = gy + (size_t)n * gy_item;
#pragma unroll
  for (int k = 0; k < (DG_GH * DG_GW * 16 + 255) / 256; ++k) {
    const int i = tid + k * 256;
    if (i < DG_GH * DG_GW * 16) {
      const int c4 = i & 15, p = i >> 4, py = p / DG_GW, px = p - py * DG_GW;
      const int yy = i0 + py, xx = j0 + px;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (yy < Ho && xx < Wo) v = ld4(gi + ((size_t)yy * Wo + xx) * 64 + c4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s_gy[p * DG_PX + c4 * 4 + e] = v[e];
    }
  }
  float wr[DG_LD];   // the next weight chunk: DG_CO couts of w[co][ci][tap], contiguous in OIHW
#pragma unroll
  for (int k = 0; k < DG_LD; ++k) wr[k] = w[tid + k * 256];
#pragma unroll
  for (int k = 0; k < DG_LD; ++k) {
    const int e = tid + k * 256, q = e / 9;
    s_w[0][(e - q * 9) * DG_TAP + q] = wr[k];
  }
  __syncthreads();

  f32x16 acc[4][2];
#pragma unroll
  for (int ph = 0; ph < 4; ++ph)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ph][ct][r] = 0.f;

  const float* ap = s_gy + (wave * DG_GW + l32) * DG_PX + hf;
#pragma unroll 1
  for (int c = 0; c < 64 / DG_CO; ++c) {
    if (c + 1 < 64 / DG_CO) {
#pragma unroll
      for (int k = 0; k < DG_LD; ++k) wr[k] = w[(c + 1) * DG_CHUNK + tid + k * 256];
    }
    const float* wb = s_w[c & 1] + hf * 64 + l32;
#pragma unroll
    for (int kk = 0; kk < DG_CO / 2; ++kk) {
      const int co = c * DG_CO + 2 * kk;
      const float a00 = ap[co], a01 = ap[DG_PX + co], a10 = ap[DG_GW * DG_PX + co], a11 = ap[(DG_GW + 1) * DG_PX + co];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const float* bp = wb + 2 * kk * 64 + ct * 32;
        acc[0][ct] = mfma32(a00, bp[4 * DG_TAP], acc[0][ct]);
        acc[1][ct] = mfma32(a01, bp[3 * DG_TAP], acc[1][ct]);
        acc[2][ct] = mfma32(a10, bp[1 * DG_TAP], acc[2][ct]);
        acc[3][ct] = mfma32(a11, bp[0 * DG_TAP], acc[3][ct]);
        acc[1][ct] = mfma32(a00, bp[5 * DG_TAP], acc[1][ct]);
        acc[2][ct] = mfma32(a00, bp[7 * DG_TAP], acc[2][ct]);
        acc[3][ct] = mfma32(a10, bp[2 * DG_TAP], acc[3][ct]);
        acc[3][ct] = mfma32(a01, bp[6 * DG_TAP], acc[3][ct]);
        acc[3][ct] = mfma32(a00, bp[8 * DG_TAP], acc[3][ct]);
      }
    }
    if (c + 1 < 64 / DG_CO) {   // the other buffer was last read before the previous barrier
#pragma unroll
      for (int k = 0; k < DG_LD; ++k) {
        const int e = tid + k * 256, q = e / 9;
        s_w[(c + 1) & 1][(e - q * 9) * DG_TAP + q] = wr[k];
      }
    }
    __syncthreads();
  }

  // D[pixel = mfma_row][ci = l32]: rows / columns of gx past H / W (H = 2 Ho - 1) are not stored
  float* go = gx + (size_t)n * gx_item;
  const int i = i0 + wave;
#pragma unroll
  for (int ph = 0; ph < 4; ++ph) {
    const int y = 2 * i + (ph >> 1);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int xx = 2 * (j0 + mfma_row(r, lane)) + (ph & 1);
        if (y < H && xx < W) go[((size_t)y * W + xx) * 64 + ct * 32 + l32] = acc[ph][ct][r];
      }
  }
}

// ---- conv_first (3 -> 64) weight gradient: gw[co][c][kh][kw] = sum gy[n][y][x][co] * x[n][c][y+kh-1][x+kw-1] ----
//
// Per pixel the 27 input taps and a constant one form the row operand (row 27 yields gb), the 64 gy channels the
// column operand: D[row 32][co 32] += A[row][pixel pair] * B[pixel pair][co] on fp32 MFMA, operands straight from
// global memory (gy is read once, 256 B per pixel -- the kernel's cost; the frames are 12 B per pixel and cached).
// A wave takes runs of CF_WAVE_PX consecutive pixels of the flat [n][h][w] order, a workgroup CF_WG_PX, statically
// (chunks b, b + G, ...); the four waves' accumulators are added in wave order and written as one [28][64] partial.
constexpr int CF_PART = 28 * 64, CF_WAVE_PX = 128, CF_WG_PX = 4 * CF_WAVE_PX, CF_WG_PER_CU = 4;

__global__ __launch_bounds__(256) void k_cf_wgrad(const float* __restrict__ x, const float* __restrict__ gy,
                                                  float* __restrict__ ws, long long gy_item, int h, int w,
                                                  long long total, int nchunks) {
  __shared__ float s_part[4][32 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, hf = lane >> 5;
  const int c = l32 / 9, kh = (l32 - c * 9) / 3, kw = l32 - c * 9 - kh * 3;   // row l32 < 27: tap (c, kh, kw)
  const long long hw = (long long)h * w;
  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc0[r] = acc1[r] = 0.f;
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    long long p = (long long)ch * CF_WG_PX + wave * CF_WAVE_PX + hf;   // this lane's pixel of each pair
    if (p - hf >= total) continue;
    long long img = p / hw;
    int y = (int)((p - img * hw) / w), xq = (int)(p - img * hw - (long long)y * w);
#pragma unroll 8
    for (int ks = 0; ks < CF_WAVE_PX / 2; ++ks) {
      float a = 0.f, b0 = 0.f, b1 = 0.f;
      if (p < total) {
        const float* g = gy + (size_t)img * gy_item + ((size_t)y * w + xq) * 64 + l32;
        b0 = g[0];
        b1 = g[32];
        const int yy = y + kh - 1, xx = xq + kw - 1;
        if (l32 == 27) a = 1.f;
        else if (l32 < 27 && yy >= 0 && yy < h && xx >= 0 && xx < w) a = x[(((size_t)img * 3 + c) * h + yy) * w + xx];
      }
      acc0 = mfma32(a, b0, acc0);
      acc1 = mfma32(a, b1, acc1);
      // two pixels on, without a branch so that the loads of the unrolled steps are issued together: a step of 2
      // wraps a row at most twice (w = 1), and each row wrap an image at most once
      p += 2;
      xq += 2;
#pragma unroll
      for (int rep = 0; rep < 2; ++rep) {
        const int wx = xq >= w ? 1 : 0;
        xq -= wx * w;
        y += wx;
        const int wy = y >= h ? 1 : 0;
        y -= wy * h;
        img += wy;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    s_part[wave][mfma_row(r, lane) * 64 + l32] = acc0[r];
    s_part[wave][mfma_row(r, lane) * 64 + 32 + l32] = acc1[r];
  }
  __syncthreads();
  for (int idx = tid; idx < CF_PART; idx += 256)
    ws[(size_t)blockIdx.x * CF_PART + idx] = ((s_part[0][idx] + s_part[1][idx]) + s_part[2][idx]) + s_part[3][idx];
}

// gw [64][27] / gb = the G partials ([row 28][co 64]) summed in a fixed order: 16 threads per element, thread s adds
// the partials s, s + 16, s + 32, ... in index order, then one thread adds the 16 sums in slice order.  The order is
// a function of G alone; one thread per element (G dependent loads each) took longer than the partials kernel.
__global__ __launch_bounds__(256) void k_cf_wgrad_reduce(const float* __restrict__ ws, int G, float* __restrict__ gw,
                                                         float* __restrict__ gb) {
  __shared__ float s_sum[16][16];
  const int e = threadIdx.x & 15, sl = threadIdx.x >> 4, idx = blockIdx.x * 16 + e;   // CF_PART = 112 blocks x 16
  float s = 0.f;
#pragma unroll 8
  for (int g = sl; g < G; g += 16) s += ws[(size_t)g * CF_PART + idx];
  s_sum[sl][e] = s;
  __syncthreads();
  if (sl != 0) return;
  float t = s_sum[0][e];
#pragma unroll
  for (int k = 1; k < 16; ++k) t += s_sum[k][e];
  const int row = idx >> 6, co = idx & 63;
  if (row < 27) gw[co * 27 + row] = t;
  else if (gb != nullptr) gb[co] = t;
}

long long cf_chunks(int n, int h, int w) { return ((long long)n * h * w + CF_WG_PX - 1) / CF_WG_PX; }
int cf_grid(long long chunks) { return (int)std::min<long long>(chunks, (long long)CF_WG_PER_CU * stif_num_cus()); }

}  // namespace

extern "C" size_t stif_conv3x3_wgrad_workspace_size(int n, int H, int W, int cin, int cout) {
  return wgrad_workspace_size<1>(n, H, W, cin, cout);
}

extern "C" int stif_conv3x3_wgrad(const stif_conv_wgrad_args* pa, void* stream) {
  return wgrad_entry<1>("stif_conv3x3_wgrad", pa, stream);
}

extern "C" size_t stif_conv3x3s2_wgrad_workspace_size(int n, int H, int W, int cin, int cout) {
  return wgrad_workspace_size<2>(n, H, W, cin, cout);
}

extern "C" int stif_conv3x3s2_wgrad(const stif_conv_wgrad_args* pa, void* stream) {
  return wgrad_entry<2>("stif_conv3x3s2_wgrad", pa, stream);
}

extern "C" size_t stif_conv3x3_wgrad_cat_workspace_size(int n, int H, int W, int nx, int gy_channels, int cout) {
  return (size_t)wgrad_cat_blocks(nx, gy_channels, cout) * wgrad_workspace_size<1>(n, H, W, 64, 64);
}

extern "C" int stif_conv3x3_wgrad_cat(const stif_conv_wgrad_cat_args* pa, void* stream) {
  const char* fn = "stif_conv3x3_wgrad_cat";
  if (!pa) return fail_as(fn, "null args");
  return wgrad_run<1>(fn, *pa, wgrad_cat_blocks(pa->nx, pa->gy_channels, pa->cout), true, "null pointer (x[0], gy, gw)",
                      "unsupported channel counts (nx, gy_channels, cout: 2/64/64, 1/256/216, 1/64/64, 2/256/256)",
                      stream);
}

extern "C" int stif_upsample2x_bwd_nhwc(const float* gy, float* gx, int n, int h1, int w1, int c, float scale,
                                        long long gy_item, long long gx_item, void* stream) {
  const char* fn = "stif_upsample2x_bwd_nhwc";
  if (!gy || !gx) return fail_as(fn, "null pointer (gy, gx)");
  if (n < 1 || h1 < 1 || w1 < 1) return fail_as(fn, "n, h1, w1 must be >= 1");
  if (c < 4 || c % 4) return fail_as(fn, "c must be a positive multiple of 4");
  if (gy_item < 0 || gx_item < 0) return fail_as(fn, "negative item stride");
  if (misaligned16(gy) || misaligned16(gx) || gy_item % 4 || gx_item % 4)
    return fail_as(fn, "gy / gx and their item strides must be 16-byte aligned");
  if (n > 1 && gx_item < (long long)h1 * w1 * c) return fail_as(fn, "gx items overlap (gx_item < h1 * w1 * c)");
  if (h1 > 65535 || n > 65535 || (long long)w1 * (c / 4) > 0x7fffffffLL - 255)
    return fail_as(fn, "image too large for the row grid");
  const dim3 grid((unsigned)((w1 * (c / 4) + 255) / 256), (unsigned)h1, (unsigned)n);
  hipLaunchKernelGGL(k_up2_bwd, grid, dim3(256), 0, static_cast<hipStream_t>(stream), gy, gx, h1, w1, c, scale,
                     gy_item, gx_item);
  return stif_check_launch(fn);
}

extern "C" size_t stif_conv3x3s2_dgrad_workspace_size(int, int, int) { return 0; }   // the weight is transposed in flight

extern "C" int stif_conv3x3s2_dgrad(const float* gy, const float* w_oihw, float* gx, long long gy_item,
                                    long long gx_item, int n, int H, int W, void*, size_t, void* stream) {
  const char* fn = "stif_conv3x3s2_dgrad";
  if (!gy || !w_oihw || !gx) return fail_as(fn, "null pointer (gy, w_oihw, gx)");
  if (n < 1 || H < 1 || W < 1) return fail_as(fn, "n, H, W must be >= 1");
  if (gy_item < 0 || gx_item < 0) return fail_as(fn, "negative item stride");
  if ((long long)H * W * 64 * 4 >= 0x7fffffffLL) return fail_as(fn, "item larger than 2 GB (buffer addressing)");
  if (misaligned16(gy) || misaligned16(gx) || gy_item % 4 || gx_item % 4)
    return fail_as(fn, "gy / gx and their item strides must be 16-byte aligned");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int tiles_x = (Wo + DG_TW - 1) / DG_TW, tiles_per_item = tiles_x * ((Ho + DG_TH - 1) / DG_TH);
  const long long tiles = (long long)n * tiles_per_item;
  if (tiles > 0x7fffffffLL) return fail_as(fn, "too many tiles");
  hipLaunchKernelGGL(k_dgrad_s2, dim3((unsigned)tiles), dim3(256), 0, static_cast<hipStream_t>(stream), gy, w_oihw, gx,
                     gy_item, gx_item, H, W, Ho, Wo, tiles_x, tiles_per_item);
  return stif_check_launch(fn);
}

extern "C" size_t stif_conv_first_wgrad_workspace_size(int n, int h, int w) {
  if (n < 1 || h < 1 || w < 1) return 0;
  const long long chunks = cf_chunks(n, h, w);
  if (chunks > 0x7fffffffLL) return 0;
  return (size_t)cf_grid(chunks) * CF_PART * sizeof(float);
}

extern "C" int stif_conv_first_wgrad(const float* x_nchw, const float* gy, float* gw, float* gb, long long gy_item,
                                     int n, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "stif_conv_first_wgrad";
  if (!x_nchw || !gy || !gw) return fail_as(fn, "null pointer (x, gy, gw)");
  if (n < 1 || h < 1 || w < 1) return fail_as(fn, "n, H, W must be >= 1");
  if (gy_item < 0) return fail_as(fn, "negative item stride");
  if ((long long)h * w * 64 * 4 >= 0x7fffffffLL) return fail_as(fn, "item larger than 2 GB (buffer addressing)");
  if (misaligned16(gy) || gy_item % 4) return fail_as(fn, "gy and its item stride must be 16-byte aligned");
  const long long chunks = cf_chunks(n, h, w);
  if (chunks > 0x7fffffffLL) return fail_as(fn, "too many tiles");
  const int G = cf_grid(chunks);
  if (!workspace || workspace_bytes < (size_t)G * CF_PART * sizeof(float))
    return fail_as(fn, "workspace too small (stif_conv_first_wgrad_workspace_size)");
  if (misaligned16(workspace)) return fail_as(fn, "workspace not 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  hipLaunchKernelGGL(k_cf_wgrad, dim3(G), dim3(256), 0, st, x_nchw, gy, ws, gy_item, h, w, (long long)n * h * w,
                     (int)chunks);
  if (int rc = stif_check_launch(fn)) return rc;
  hipLaunchKernelGGL(k_cf_wgrad_reduce, dim3(CF_PART / 16), dim3(256), 0, st, ws, G, gw, gb);
  return stif_check_launch("stif_conv_first_wgrad (reduce)");
}

extern "C" int stif_pack_conv_plain_dev(const float* w_oihw, const float* b, int cout, int cin, int ks, float* w_dst,
                                        float* b_dst, void* stream) {
  const char* fn = "stif_pack_conv_plain_dev";
  if (!w_oihw || !w_dst || !b_dst) return fail_as(fn, "null pointer (w_oihw, w_dst, b_dst)");
  if (ks != 3) return fail_as(fn, "the device pack needs a 3x3 kernel");
  if (cin != 64 || cout != 64) return fail_as(fn, "unsupported channel counts (64 -> 64 only)");
  hipLaunchKernelGGL(k_pack_plain, dim3(64 * 64 * 9 / 256), dim3(256), 0, static_cast<hipStream_t>(stream), w_oihw, b,
                     w_dst, b_dst);
  return stif_check_launch(fn);
}

// The two Winograd device packers: the checks, then k_pack_wino on the 64 x 64 block at (co0, ci0) of the [cout][cin]
// weight.  `shape_err`: the entry's own refusal of its sizes, or null.
static int pack_wino_run(const char* fn, const char* shape_err, const float* w_oihw, const float* b, int cout, int cin,
                         int co0, int ci0, int mode, int flags, float* w_dst, float* b_dst, int* status, void* stream) {
  if (!w_oihw || !w_dst || !b_dst) return fail_as(fn, "null pointer (w_oihw, w_dst, b_dst)");
  if (mode != STIF_PACK_WINO && mode != (STIF_PACK_WINO | STIF_PACK_F16X3))
    return fail_as(fn, "unsupported mode (STIF_PACK_WINO [| STIF_PACK_F16X3] only)");
  if (shape_err) return fail_as(fn, shape_err);
  if (flags & ~STIF_PACK_DGRAD) return fail_as(fn, "unknown flags");
  const bool dgrad = (flags & STIF_PACK_DGRAD) != 0, f16 = (mode & STIF_PACK_F16X3) != 0;
  if (!b && !dgrad) return fail_as(fn, "null bias (allowed with STIF_PACK_DGRAD only)");
  if (f16 && !status) return fail_as(fn, "STIF_PACK_F16X3 needs a status word (range report)");
  hipLaunchKernelGGL(k_pack_wino, dim3(16), dim3(256), 0, static_cast<hipStream_t>(stream), w_oihw, b, w_dst, b_dst,
                     status, f16 ? 1 : 0, dgrad ? 1 : 0, cout, cin, co0, ci0);
  return stif_check_launch(fn);
}

extern "C" int stif_pack_conv_weight_dev(const float* w_oihw, const float* b, int cout, int cin, int ks, int mode,
                                         int flags, float* w_dst, float* b_dst, int* status, void* stream) {
  const char* err = ks != 3                    ? "winograd pack needs a 3x3 kernel"
                    : cin != 64 || cout != 64 ? "unsupported channel counts (64 -> 64 only)"
                                              : nullptr;
  return pack_wino_run("stif_pack_conv_weight_dev", err, w_oihw, b, 64, 64, 0, 0, mode, flags, w_dst, b_dst, status,
                       stream);
}

extern "C" int stif_pack_conv_block_dev(const float* w_oihw, const float* b, int cout, int cin, int co0, int ci0,
                                        int mode, int flags, float* w_dst, float* b_dst, int* status, void* stream) {
  const char* err = nullptr;
  if (((cout != 64 && cout != 216) || (cin != 64 && cin != 128)) && !(cout == 256 && cin == 128))
    err = "unsupported channel counts (cout 64 or 216 with cin 64 or 128, or 256 with 128)";
  else if (co0 < 0 || co0 % 64 || co0 >= cout || ci0 < 0 || ci0 % 64 || ci0 >= cin)
    err = "co0 / ci0 must be multiples of 64 inside the weight";
  return pack_wino_run("stif_pack_conv_block_dev", err, w_oihw, b, cout, cin, co0, ci0, mode, flags, w_dst, b_dst,
                       status, stream);
}
