// Backward of the 1x1 (64 | 64) -> 64 convolution on two inputs (fusion, Easy_PCD.fusion, ConvBLSTM.conv_1x1;
// Sakuya_arch_test.py:141, :254, :289), DESIGN.md section 3n: the weight / bias gradient kernel and the device packer
// of the layer.  The forward is stif_conv2d_nhwc (ks 1, in1_mode 1) on the pack written here; the data gradient of
// input k is the same entry point's fp32 1x1 64 -> 64 path on the STIF_PACK_DGRAD pack of that input half.
#include <algorithm>
#include <cstdio>

#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

namespace {

// ---- weight gradient: gw[co][64 k + ci] = sum_p gy[p][co] * x_k[p][ci], gb[co] = sum_p gy[p][co] ----
//
// The scheme of stif_conv3x3_wgrad without taps.  A workgroup takes chunks of PX consecutive pixels of one item
// (ceil(H W / PX) chunks per item, so no thread divides by H W; static schedule: chunks b, b + G, ...), stages the gy
// rows and the rows of every x map in LDS with 16-byte loads (pixels past the item's end are zeros; the next chunk is
// fetched into registers while this one is contracted) and contracts over the pixels on fp32 MFMA:
// D[co 32][ci 32] += A[co][pixel pair] * B[pixel pair][ci].  Wave w owns cout tile w >> 1 and cin tile w & 1 of every x map: 16 nx
// accumulator registers kept over all its chunks.  One k step is one gy read, nx x reads (ds_read_b32, 32 consecutive
// channels per lane half) and nx MFMAs; a pixel costs 256 (1 + nx) bytes of HBM, so the kernel is paced by memory.
// Every workgroup writes one partial [co 64][ci 64 nx] + 64 bias sums; k_c1_wgrad_reduce adds the G partials in a fixed
// order.  The grid is a function of the shape and the CU count alone: repeated calls give identical bits.
constexpr int C1_PX = 64, C1_WG_PER_CU = 3;

template <int NX>
__global__ __launch_bounds__(256) void k_c1_wgrad(const float* __restrict__ x0, const float* __restrict__ x1,
                                                  const float* __restrict__ gy, float* __restrict__ ws,
                                                  long long x0_item, long long x1_item, long long gy_item,
                                                  int hw, int chunks_per_item, int nchunks) {
  __shared__ __attribute__((aligned(16))) float s_gy[C1_PX * 64];
  __shared__ __attribute__((aligned(16))) float s_x[NX][C1_PX * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cot = wave >> 1, cit = wave & 1, l32 = lane & 31, hf = lane >> 5;
  f32x16 acc[NX];
#pragma unroll
  for (int k = 0; k < NX; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;
  float bsum = 0.f;   // sum of this lane's gy values: cout cot * 32 + l32, pixels of parity hf

  // this thread's share of a chunk: float4 c4 of pixels tid / 16 + 16 k, fetched into registers one chunk ahead so
  // that the loads of chunk b + G are in flight while chunk b is contracted
  constexpr int LD = C1_PX * 16 / 256;
  const int c4 = tid & 15;
  f32x4 rg[LD], r0[LD], r1[LD];
  auto fetch = [&](int ch) {
    const int item = ch / chunks_per_item, r_first = (ch - item * chunks_per_item) * C1_PX + (tid >> 4);
#pragma unroll
    for (int k = 0; k < LD; ++k) {
      const int r = r_first + 16 * k;
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      rg[k] = r0[k] = r1[k] = zero;
      if (r < hw) {
        rg[k] = ld4(gy + (size_t)item * gy_item + (size_t)r * 64 + c4 * 4);
        r0[k] = ld4(x0 + (size_t)item * x0_item + (size_t)r * 64 + c4 * 4);
        if (NX == 2) r1[k] = ld4(x1 + (size_t)item * x1_item + (size_t)r * 64 + c4 * 4);
      }
    }
  };
  if ((int)blockIdx.x < nchunks) fetch(blockIdx.x);

  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    __syncthreads();   // the previous chunk's reads are done
#pragma unroll
    for (int k = 0; k < LD; ++k) {
      const int px = (tid >> 4) + 16 * k;
      st4(s_gy + px * 64 + c4 * 4, rg[k]);
      st4(s_x[0] + px * 64 + c4 * 4, r0[k]);
      if (NX == 2) st4(s_x[NX - 1] + px * 64 + c4 * 4, r1[k]);
    }
    __syncthreads();
    if ((long long)ch + gridDim.x < nchunks) fetch(ch + (int)gridDim.x);
    const float* ap = s_gy + hf * 64 + cot * 32 + l32;
#pragma unroll 4
    for (int ks = 0; ks < C1_PX / 2; ++ks) {
      const float a = ap[ks * 128];
      bsum += a;
#pragma unroll
      for (int k = 0; k < NX; ++k) acc[k] = mfma32(a, s_x[k][(2 * ks + hf) * 64 + cit * 32 + l32], acc[k]);
    }
  }

  constexpr int PART1 = 64 * 64 * NX + 64;
  float* part = ws + (size_t)blockIdx.x * PART1;
#pragma unroll
  for (int k = 0; k < NX; ++k)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      part[(cot * 32 + mfma_row(r, lane)) * (64 * NX) + k * 64 + cit * 32 + l32] = acc[k][r];
  const float other = __shfl_xor(bsum, 32);
  if (cit == 0 && hf == 0) part[64 * 64 * NX + cot * 32 + l32] = bsum + other;
}

// gw [64][64 nx] (OIHW with 1x1 taps: the partial's own order) / gb = the G partials summed in a fixed order, as
// k_cf_wgrad_reduce (conv_bwd.hip): 16 threads per element, thread s adds the partials s, s + 16, s + 32, ... in index
// order, then one thread adds the 16 sums in slice order.  The order is a function of G alone.  `part` is a multiple
// of 16.
__global__ __launch_bounds__(256) void k_c1_wgrad_reduce(const float* __restrict__ ws, int G, int part,
                                                         float* __restrict__ gw, float* __restrict__ gb) {
  __shared__ float s_sum[16][16];
  const int e = threadIdx.x & 15, sl = threadIdx.x >> 4, idx = blockIdx.x * 16 + e;
  float s = 0.f;
#pragma unroll 8
  for (int g = sl; g < G; g += 16) s += ws[(size_t)g * part + idx];
  s_sum[sl][e] = s;
  __syncthreads();
  if (sl != 0) return;
  float t = s_sum[0][e];
#pragma unroll
  for (int k = 1; k < 16; ++k) t += s_sum[k][e];
  if (idx < part - 64) gw[idx] = t;
  else if (gb != nullptr) gb[idx - (part - 64)] = t;
}

long long c1_chunks_per_item(int H, int W) { return ((long long)H * W + C1_PX - 1) / C1_PX; }
long long c1_chunks(int n, int H, int W) { return (long long)n * c1_chunks_per_item(H, W); }
int c1_grid(long long chunks) { return (int)std::min<long long>(chunks, (long long)C1_WG_PER_CU * stif_num_cus()); }
size_t c1_part_floats(int nx) { return (size_t)64 * 64 * nx + 64; }

// ---- the device packer: the bytes of pack.cpp's STIF_PACK_PLAIN loop / pack_1x1_f16x3 for ks = 1, cout = 64 ----
// one thread per (packed cout co, packed cin ci) of a [64][CI] layer read from the OIHW weight [64][128]: plain
// w[co][ci]; dgrad (CI = 64) w'[co][ci] = w[ci][ci0 + co], the data gradient's layer of that input half, zero bias.
// fp32: [chunk CI / 8][nt 2][lane 64][4], lane l of nt holding cout nt * 32 + (l & 31), input channel
// chunk * 8 + 4 (l >> 5) + e.  f16x3: [chunk 8][nt 2][plane h|l][lane 64][8 halves] of w * 2^10, element e of lane l
// holding input channel 16 chunk + 8 (l >> 5) + e.
__global__ __launch_bounds__(256) void k_pack_1x1(const float* __restrict__ w, const float* __restrict__ b,
                                                  float* __restrict__ w_dst, float* __restrict__ b_dst, int* status,
                                                  int f16, int dgrad, int ci0, int CI) {
  const int idx = blockIdx.x * 256 + threadIdx.x;   // < 64 CI
  const int co = idx / CI, ci = idx - co * CI, nt = co >> 5;
  const float v = dgrad ? w[ci * 128 + ci0 + co] : w[co * 128 + ci];
  if (!f16) {
    const int c = ci >> 3, l = (co & 31) + 32 * ((ci >> 2) & 1), e = ci & 3;
    w_dst[((c * 2 + nt) * 64 + l) * 4 + e] = v;
  } else {
    const int c = ci >> 4, l = (co & 31) + 32 * ((ci >> 3) & 1), e = ci & 7;
    _Float16* dst = reinterpret_cast<_Float16*>(w_dst);
    const double x = (double)v * 1024.0;
    const _Float16 h = (_Float16)x;
    const _Float16 lo = (_Float16)(x - (double)h);
    const size_t o = ((((size_t)c * 2 + nt) * 2) * 64 + l) * 8 + e;
    dst[o] = h;
    dst[o + 512] = lo;
    if (!(v >= -65504.0f / 1024.0f && v <= 65504.0f / 1024.0f)) atomicOr(status, STIF_STATUS_PACK_RANGE);
  }
  if (ci == 0) b_dst[co] = (dgrad || b == nullptr) ? 0.f : b[co];
}

int fail_as(const char* fn, const char* why) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  return stif_fail(STIF_E_INVALID, msg);
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace

extern "C" size_t stif_conv1x1_wgrad_workspace_size(int n, int H, int W, int nx) {
  if (n < 1 || H < 1 || W < 1 || (nx != 1 && nx != 2)) return 0;
  const long long chunks = c1_chunks(n, H, W);
  if (chunks > 0x7fffffffLL) return 0;
  return (size_t)c1_grid(chunks) * c1_part_floats(nx) * sizeof(float);
}

extern "C" int stif_conv1x1_wgrad(const stif_conv_wgrad_cat_args* pa, void* stream) {
  const char* fn = "stif_conv1x1_wgrad";
  if (!pa) return fail_as(fn, "null args");
  const stif_conv_wgrad_cat_args& a = *pa;
  if (!a.x[0] || !a.gy || !a.gw) return fail_as(fn, "null pointer (x[0], gy, gw)");
  if (a.n < 1 || a.H < 1 || a.W < 1) return fail_as(fn, "n, H, W must be >= 1");
  if ((a.nx != 1 && a.nx != 2) || a.gy_channels != 64 || a.cout != 64)
    return fail_as(fn, "unsupported channel counts (nx 1 or 2, gy_channels = cout = 64)");
  const bool two = a.nx == 2;
  if (two && !a.x[1]) return fail_as(fn, "null pointer (x[1] with nx = 2)");
  if (a.x_item[0] < 0 || (two && a.x_item[1] < 0) || a.gy_item < 0) return fail_as(fn, "negative item stride");
  if ((long long)a.H * a.W * 64 * 4 >= 0x7fffffffLL) return fail_as(fn, "item larger than 2 GB (buffer addressing)");
  if (misaligned16(a.x[0]) || (two && misaligned16(a.x[1])) || misaligned16(a.gy) || a.x_item[0] % 4 ||
      (two && a.x_item[1] % 4) || a.gy_item % 4)
    return fail_as(fn, "x / gy and their item strides must be 16-byte aligned");
  const long long chunks = c1_chunks(a.n, a.H, a.W);
  if (chunks > 0x7fffffffLL) return fail_as(fn, "too many pixel chunks");
  const int G = c1_grid(chunks);
  const size_t part = c1_part_floats(a.nx);
  if (!a.workspace || a.workspace_bytes < (size_t)G * part * sizeof(float))
    return fail_as(fn, "workspace too small (stif_conv1x1_wgrad_workspace_size)");
  if (misaligned16(a.workspace)) return fail_as(fn, "workspace not 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(a.workspace);
  const int hw = a.H * a.W, cpi = (int)c1_chunks_per_item(a.H, a.W);   // H W 256 < 2^31: checked above
  if (two)
    hipLaunchKernelGGL(k_c1_wgrad<2>, dim3(G), dim3(256), 0, st, a.x[0], a.x[1], a.gy, ws, a.x_item[0], a.x_item[1],
                       a.gy_item, hw, cpi, (int)chunks);
  else
    hipLaunchKernelGGL(k_c1_wgrad<1>, dim3(G), dim3(256), 0, st, a.x[0], a.x[0], a.gy, ws, a.x_item[0], a.x_item[0],
                       a.gy_item, hw, cpi, (int)chunks);
  if (int rc = stif_check_launch(fn)) return rc;
  hipLaunchKernelGGL(k_c1_wgrad_reduce, dim3((unsigned)part / 16), dim3(256), 0, st, ws, G, (int)part, a.gw,
                     a.gb);
  return stif_check_launch("stif_conv1x1_wgrad (reduce)");
}

extern "C" int stif_pack_conv1x1_dev(const float* w_oihw, const float* b, int cout, int cin, int ci0, int mode,
                                     int flags, float* w_dst, float* b_dst, int* status, void* stream) {
  const char* fn = "stif_pack_conv1x1_dev";
  if (!w_oihw || !w_dst || !b_dst) return fail_as(fn, "null pointer (w_oihw, w_dst, b_dst)");
  if (mode != STIF_PACK_PLAIN && mode != (STIF_PACK_PLAIN | STIF_PACK_F16X3))
    return fail_as(fn, "unsupported mode (STIF_PACK_PLAIN [| STIF_PACK_F16X3] only)");
  if (cout != 64 || cin != 128) return fail_as(fn, "unsupported channel counts ((64 | 64) -> 64 only)");
  if (flags & ~STIF_PACK_DGRAD) return fail_as(fn, "unknown flags");
  const bool dgrad = (flags & STIF_PACK_DGRAD) != 0, f16 = (mode & STIF_PACK_F16X3) != 0;
  if (dgrad && f16) return fail_as(fn, "STIF_PACK_DGRAD packs the fp32 layer (mode STIF_PACK_PLAIN) only");
  if (dgrad ? (ci0 != 0 && ci0 != 64) : ci0 != 0)
    return fail_as(fn, "ci0 must be 0, or with STIF_PACK_DGRAD the input half 0 or 64");
  if (!b && !dgrad) return fail_as(fn, "null bias (allowed with STIF_PACK_DGRAD only)");
  if (f16 && !status) return fail_as(fn, "STIF_PACK_F16X3 needs a status word (range report)");
  const int CI = dgrad ? 64 : 128;
  hipLaunchKernelGGL(k_pack_1x1, dim3(64 * CI / 256), dim3(256), 0, static_cast<hipStream_t>(stream), w_oihw, b, w_dst,
                     b_dst, status, f16 ? 1 : 0, dgrad ? 1 : 0, ci0, CI);
  return stif_check_launch(fn);
}
