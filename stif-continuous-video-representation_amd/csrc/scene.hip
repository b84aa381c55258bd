// Scene-cut evidence for the video path: the sum of absolute differences of the 8-bit luma of every adjacent pair
// of n fp32 RGB frames, on the device (stif_amd.video turns the sums into cut decisions and repeats a real frame at
// a cut instead of interpolating across it).  One pass over the frames, bandwidth-bound like yuv.hip: a thread owns
// four neighbouring columns of one row and walks the frames, keeping the previous frame's four luma values in
// registers; it reads them as one 16-byte access per plane where the caller's pointer and strides allow it (a
// per-launch decision made on the host), as scalar accesses otherwise and at the right edge.
//
// After the quantisation to 8 bits everything is integer arithmetic, so the sums are exact, independent of the
// order of summation and of the launch geometry, and equal from call to call.  Workgroups write 64-bit partial sums
// to the workspace and a small second launch adds them (the scheme of k_metric_finish): no atomics, no zeroed
// output, no read-back.
#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

#include <algorithm>

namespace {

constexpr int GROUP = 8;          // pairs a thread accumulates in registers per walk (9 frames)
constexpr int MAX_BLOCKS = 4096;  // workgroups of the first launch: 16 per compute unit of a 256-CU device
constexpr int MAX_WALKS = 1024;   // gridDim.y: walks (groups of GROUP pairs) in flight; further ones are looped over

struct Scene {
  const float* rgb;
  long long item, plane, pitch;   // elements
  int n, H, W;
  unsigned long long* part;       // [n - 1][gridDim.x]
};

// The 8-bit luma of a pixel (BT.601 weights on the clamped channels; a NaN channel counts as 0).  No FMA
// contraction: the value is pinned to these operations, so that a host restatement gives the same integer.
STIF_DEV int luma8(float r, float g, float b) {
#pragma clang fp contract(off)
  r = fminf(fmaxf(r, 0.f), 1.f);
  g = fminf(fmaxf(g, 0.f), 1.f);
  b = fminf(fmaxf(b, 0.f), 1.f);
  const float y = (0.299f * r + 0.587f * g) + 0.114f * b;
  return min((int)rintf(y * 255.f), 255);
}

// the four luma values of columns x0 .. x0 + 3 of one row of one frame (columns >= nx: 0 in every frame)
template <bool VEC>
STIF_DEV void luma_row(const float* s, long long plane, int nx, int q[4]) {
  f32x4 R = {0.f, 0.f, 0.f, 0.f}, G = R, B = R;
  if (VEC && nx == 4) {
    R = ld4(s);
    G = ld4(s + plane);
    B = ld4(s + 2 * plane);
  } else {
    for (int k = 0; k < nx; ++k) {
      R[k] = s[k];
      G[k] = s[plane + k];
      B[k] = s[2 * plane + k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = luma8(R[k], G[k], B[k]);
}

// sum over the 64 lanes
STIF_DEV unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// part[pair][blockIdx.x] = the sum of |q_pair - q_pair+1| over the pixels this workgroup walks.  A walk covers
// GROUP pairs (GROUP + 1 frames, each read once); with more pairs than that, blockIdx.y strides over the walks and
// the frame two walks share is read by both.
// Overflow: one group of four pixels adds at most 4 * 255 = 1020 (the only 32-bit sum); the register sums, the
// partials and the totals are 64-bit and bounded by 255 H W <= 255 * 2^48 < 2^56 (the entry point rejects frames
// above 2^48 pixels).  An 8K pair going black to white is 8,460,288,000, above 2^32.
template <bool VEC>
__global__ __launch_bounds__(256) void k_scene_sad(Scene a) {
  __shared__ unsigned long long red[4][GROUP];
  const int gw = (a.W + 3) >> 2;
  const long long total = (long long)a.H * gw;
  const int pairs = a.n - 1, walks = (pairs + GROUP - 1) / GROUP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int walk = blockIdx.y; walk < walks; walk += gridDim.y) {
    const int i0 = walk * GROUP, np = min(GROUP, pairs - i0);
    unsigned long long acc[GROUP];
#pragma unroll
    for (int k = 0; k < GROUP; ++k) acc[k] = 0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
      const int g = (int)(e % gw);
      const long long y = e / gw;
      const int x0 = g * 4, nx = min(4, a.W - x0);
      const float* s = a.rgb + (long long)i0 * a.item + y * a.pitch + x0;
      int prev[4];
      luma_row<VEC>(s, a.plane, nx, prev);
#pragma unroll
      for (int k = 0; k < GROUP; ++k) {
        if (k >= np) continue;
        s += a.item;
        int q[4];
        luma_row<VEC>(s, a.plane, nx, q);
        unsigned d = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          d += (unsigned)abs(q[c] - prev[c]);
          prev[c] = q[c];
        }
        acc[k] += d;
      }
    }
#pragma unroll
    for (int k = 0; k < GROUP; ++k) {
      const unsigned long long v = wave_sum(acc[k]);
      if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < np)
      a.part[(size_t)(i0 + threadIdx.x) * gridDim.x + blockIdx.x] =
          red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    __syncthreads();
  }
}

// sad[pair] = the pair's `blocks` partials added: thread t takes partials t, t + 256, ... in turn, then a binary
// tree over the 256 threads
__global__ __launch_bounds__(256) void k_scene_finish(const unsigned long long* __restrict__ part, int blocks,
                                                      unsigned long long* __restrict__ sad) {
  __shared__ unsigned long long red[256];
  const int tid = threadIdx.x;
  const unsigned long long* src = part + (size_t)blockIdx.x * blocks;
  unsigned long long s = 0;
  for (int i = tid; i < blocks; i += 256) s += src[i];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) sad[blockIdx.x] = red[0];
}

// workgroups of the first launch: one thread per group of four columns of a row, at most MAX_BLOCKS (a fixed cap,
// so that the workspace size is a function of the shape alone)
long long scene_blocks(int H, int W) {
  const long long threads = (long long)H * ((W + 3) >> 2);
  return std::min<long long>((threads + 255) / 256, MAX_BLOCKS);
}

int fail(int code, const char* why) {
  char msg[160];
  snprintf(msg, sizeof msg, "stif_scene_sad: %s", why);
  return stif_fail(code, msg);
}

}  // namespace

extern "C" size_t stif_scene_workspace_size(int n, int H, int W) {
  if (n < 2 || H < 1 || W < 1) return 0;
  return (size_t)scene_blocks(H, W) * (size_t)(n - 1) * sizeof(unsigned long long);
}

extern "C" int stif_scene_sad(const float* rgb, long long item, long long plane, long long pitch, int n, int H,
                              int W, unsigned long long* sad, void* workspace, size_t workspace_bytes,
                              void* stream) {
  // every check comes before the first launch
  if (!rgb || !sad) return fail(STIF_E_INVALID, "rgb or sad is null");
  if (n < 2 || H < 1 || W < 1) return fail(STIF_E_INVALID, "n must be >= 2, H and W >= 1");
  if ((long long)H * W > (1LL << 48)) return fail(STIF_E_INVALID, "H W above 2^48 pixels");
  Scene a;
  a.rgb = rgb;
  a.n = n;
  a.H = H;
  a.W = W;
  // the addressing of stif_metric_args.pred: all zero = dense; otherwise rows, planes and items must not overlap
  if (item == 0 && plane == 0 && pitch == 0) {
    a.pitch = W;
    a.plane = (long long)H * W;
    a.item = 3 * a.plane;
  } else {
    const long long rows = (long long)(H - 1) * pitch + W;   // extent of one plane
    if (pitch < W || plane < rows || item < 2 * plane + rows)
      return fail(STIF_E_INVALID, "rgb strides: pitch below W or overlapping planes / items");
    a.pitch = pitch;
    a.plane = plane;
    a.item = item;
  }
  if ((uintptr_t)sad & 7) return fail(STIF_E_INVALID, "sad must be 8-byte aligned");
  if (!workspace || workspace_bytes < stif_scene_workspace_size(n, H, W))
    return fail(STIF_E_WORKSPACE, "workspace smaller than stif_scene_workspace_size");
  if ((uintptr_t)workspace & 7) return fail(STIF_E_INVALID, "workspace must be 8-byte aligned");
  a.part = (unsigned long long*)workspace;

  const bool vec = (((uintptr_t)rgb & 15) | ((uintptr_t)a.pitch & 3) | ((uintptr_t)a.plane & 3) |
                    ((uintptr_t)a.item & 3)) == 0;
  const int blocks = (int)scene_blocks(H, W), walks = (n - 1 + GROUP - 1) / GROUP;
  const dim3 grid((unsigned)blocks, (unsigned)std::min(walks, MAX_WALKS));
  hipStream_t st = (hipStream_t)stream;
  with_bool(vec, [&](auto v) {
    hipLaunchKernelGGL(k_scene_sad<decltype(v)::value>, grid, dim3(256), 0, st, a);
  });
  if (int rc = stif_check_launch("stif_scene_sad")) return rc;
  hipLaunchKernelGGL(k_scene_finish, dim3((unsigned)(n - 1)), dim3(256), 0, st,
                     (const unsigned long long*)a.part, blocks, sad);
  return stif_check_launch("stif_scene_sad (finish)");
}
