// The input builders of the decoder's three SIREN MLPs for training and their adjoints (DESIGN.md section 3o;
// Sakuya_arch_test.py:364-459 without the local ensemble).  Training materialises the MLP inputs in HBM, one fp32 row
// per HR pixel, so that siren_train.hip's layer GEMMs and their backward read plain matrices: these kernels only
// move memory.  Every index and clamp side comes from the host's per-row / per-column tables (coords.dec_tables) or,
// for the warped grids, from the expressions of decoder.hip (warp_grids, bilin_corners) in the reference's fp32.
#include <cstdio>

#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

namespace {

typedef stif_dec_train_geom Geom;
constexpr int X1_W = 208, X2_W = 264, X3_W = 528;   // row widths: 201, 263 and 525 inputs rounded up to 8

struct Pix {
  int b, qy, qx;
};
STIF_DEV Pix pix_of(long long n, int HH, int WW) {
  const long long r = n / WW;
  return {(int)(r / HH), (int)(r % HH), (int)(n % WW)};
}

// the bilinear corners of a normalised coordinate (ATen grid_sampler_2d, align_corners=False), as decoder.hip's
// bilin_corners with the one-dimensional weights and the corners' validity kept apart for the coordinate gradient
struct Cn {
  int x0, x1, y0, y1;
  float wx0, wx1, wy0, wy1;
  bool vx0, vx1, vy0, vy1;
};
STIF_DEV Cn corners(float gx, float gy, int Wd, int Hd) {
  const float ix = ((gx + 1.f) * (float)Wd - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)Hd - 1.f) / 2.f;
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
  Cn c;
  c.wx1 = ix - fx0, c.wx0 = (fx0 + 1.f) - ix;
  c.wy1 = iy - fy0, c.wy0 = (fy0 + 1.f) - iy;
  c.vx0 = x0 >= 0 && x0 < Wd, c.vx1 = x1 >= 0 && x1 < Wd;
  c.vy0 = y0 >= 0 && y0 < Hd, c.vy1 = y1 >= 0 && y1 < Hd;
  c.x0 = min(max(x0, 0), Wd - 1), c.x1 = min(max(x1, 0), Wd - 1);
  c.y0 = min(max(y0, 0), Hd - 1), c.y1 = min(max(y1, 0), Hd - 1);
  return c;
}

// one axis of a warped grid (warplayer.py:25-39 and the decoder's clamp, :428/:441): base + flow / ((n - 1) / 2),
// clamped to +-(1 - 1e-6); `pass`: the clamp hands the gradient on (torch.clamp: on the closed interval)
struct Warp {
  float g;
  bool pass;
};
STIF_DEV Warp warp_axis(float base, float f, int n) {
  const float lo = -1.f + 1e-6f, hi = 1.f - 1e-6f;
  const float u = base + f / (((float)n - 1.f) / 2.f);
  return {fminf(fmaxf(u, lo), hi), u >= lo && u <= hi};
}

// four channels of the bilinear sample of an NHWC map `C` channels wide
STIF_DEV f32x4 sample4(const float* map, int C, int Wd, const Cn& c, int ch) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (c.vy0 && c.vx0) s += (c.wx0 * c.wy0) * ld4(map + ((size_t)c.y0 * Wd + c.x0) * C + ch);
  if (c.vy0 && c.vx1) s += (c.wx1 * c.wy0) * ld4(map + ((size_t)c.y0 * Wd + c.x1) * C + ch);
  if (c.vy1 && c.vx0) s += (c.wx0 * c.wy1) * ld4(map + ((size_t)c.y1 * Wd + c.x0) * C + ch);
  if (c.vy1 && c.vx1) s += (c.wx1 * c.wy1) * ld4(map + ((size_t)c.y1 * Wd + c.x1) * C + ch);
  return s;
}
// the bilinear sample of one plane of the planar frames
STIF_DEV float sample1(const float* plane, int Wd, const Cn& c) {
  float s = 0.f;
  if (c.vy0 && c.vx0) s += (c.wx0 * c.wy0) * plane[c.y0 * Wd + c.x0];
  if (c.vy0 && c.vx1) s += (c.wx1 * c.wy0) * plane[c.y0 * Wd + c.x1];
  if (c.vy1 && c.vx0) s += (c.wx0 * c.wy1) * plane[c.y1 * Wd + c.x0];
  if (c.vy1 && c.vx1) s += (c.wx1 * c.wy1) * plane[c.y1 * Wd + c.x1];
  return s;
}

// ---- X1: nearest latent 192 | nearest frames 6 | rel_y, rel_x | t | zeros; one thread per float4 ----
__global__ __launch_bounds__(256) void k_x1_fwd(Geom g, float* __restrict__ x1, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long n = idx / (X1_W / 4);
  const int c4 = (int)(idx - n * (X1_W / 4));
  const Pix p = pix_of(n, g.HH, g.WW);
  const int iy = g.near_y[p.qy], ix = g.near_x[p.qx];
  const size_t plane = (size_t)g.H * g.W, px = (size_t)iy * g.W + ix;
  const float* fr = g.frames + (size_t)p.b * 6 * plane + px;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (c4 < 48) v = ld4(g.feat + ((size_t)p.b * plane + px) * 192 + c4 * 4);
  else if (c4 == 48) v = f32x4{fr[0], fr[plane], fr[2 * plane], fr[3 * plane]};
  else if (c4 == 49) v = f32x4{fr[4 * plane], fr[5 * plane], g.rel_y[p.qy], g.rel_x[p.qx]};
  else if (c4 == 50) v[0] = g.t[p.b];
  st4(x1 + (size_t)n * X1_W + c4 * 4, v);
}

// g_feat[b][iy][ix][:] = the sum of the g_X1 rows of the HR rectangle whose nearest LR pixel is (iy, ix): the nearest
// index is monotone per axis, so the rectangle is [first_y[iy], first_y[iy + 1]) x [first_x[ix], first_x[ix + 1]).
// One thread per float4 of g_feat, rows then columns in order.
__global__ __launch_bounds__(256) void k_x1_bwd(Geom g, const float* __restrict__ gx1, float* __restrict__ g_feat,
                                                long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long lp = idx / 48;
  const int c4 = (int)(idx - lp * 48);
  const int ix = (int)(lp % g.W), iy = (int)((lp / g.W) % g.H), b = (int)(lp / ((long long)g.W * g.H));
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int qy = g.near_y_first[iy]; qy < g.near_y_first[iy + 1]; ++qy)
    for (int qx = g.near_x_first[ix]; qx < g.near_x_first[ix + 1]; ++qx)
      s += ld4(gx1 + (((size_t)b * g.HH + qy) * g.WW + qx) * X1_W + c4 * 4);
  st4(g_feat + (size_t)lp * 192 + c4 * 4, s);
}

// ---- X2: HRfeat 64 | bilinear latent 192 | bilinear frames 6 | t | zero, at the fixed query grid (tables) ----
__global__ __launch_bounds__(256) void k_x2_fwd(Geom g, const float* __restrict__ hrfeat, float* __restrict__ x2,
                                                long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long n = idx / (X2_W / 4);
  const int c4 = (int)(idx - n * (X2_W / 4));
  const Pix p = pix_of(n, g.HH, g.WW);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (c4 < 16) {
    v = ld4(hrfeat + (size_t)n * 64 + c4 * 4);
  } else {
    // the tables carry clamped indices and weights that are zero for a corner outside the map
    Cn c;
    c.y0 = g.by0[p.qy], c.y1 = g.by1[p.qy], c.x0 = g.bx0[p.qx], c.x1 = g.bx1[p.qx];
    c.wy0 = g.wy0[p.qy], c.wy1 = g.wy1[p.qy], c.wx0 = g.wx0[p.qx], c.wx1 = g.wx1[p.qx];
    c.vx0 = c.vx1 = c.vy0 = c.vy1 = true;
    const size_t plane = (size_t)g.H * g.W;
    const float* fr = g.frames + (size_t)p.b * 6 * plane;
    if (c4 < 64) v = sample4(g.feat + (size_t)p.b * plane * 192, 192, g.W, c, (c4 - 16) * 4);
    else if (c4 == 64)
      v = f32x4{sample1(fr, g.W, c), sample1(fr + plane, g.W, c), sample1(fr + 2 * plane, g.W, c),
                sample1(fr + 3 * plane, g.W, c)};
    else
      v = f32x4{sample1(fr + 4 * plane, g.W, c), sample1(fr + 5 * plane, g.W, c), g.t[p.b], 0.f};
  }
  st4(x2 + (size_t)n * X2_W + c4 * 4, v);
}

__global__ __launch_bounds__(256) void k_x2_bwd_hr(const float* __restrict__ gx2, float* __restrict__ g_hr,
                                                   long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long n = idx >> 4;
  const int c4 = (int)(idx & 15);
  st4(g_hr + (size_t)n * 64 + c4 * 4, ld4(gx2 + (size_t)n * X2_W + c4 * 4));
}

// The adjoint of the fixed bilinear gather in gather form.  The gather is separable and its corner tables are
// monotone: LR row iy is the upper corner (weight wy0) of the HR rows [by0_first[iy], by0_first[iy + 1]) and the lower
// one (wy1) of [by1_first[iy], by1_first[iy + 1]), and the same along x.  One thread per float4 of g_feat adds its
// terms in a fixed order (side, row, side, column).
__global__ __launch_bounds__(256) void k_x2_bwd_feat(Geom g, const float* __restrict__ gx2, float* __restrict__ g_feat,
                                                     long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long lp = idx / 48;
  const int c4 = (int)(idx - lp * 48);
  const int ix = (int)(lp % g.W), iy = (int)((lp / g.W) % g.H), b = (int)(lp / ((long long)g.W * g.H));
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int sy = 0; sy < 2; ++sy) {
    const int* fy = sy ? g.by1_first : g.by0_first;
    const float* wy = sy ? g.wy1 : g.wy0;
    for (int qy = fy[iy]; qy < fy[iy + 1]; ++qy) {
      const float wyv = wy[qy];
      if (wyv == 0.f) continue;
      const float* row = gx2 + ((size_t)b * g.HH + qy) * g.WW * X2_W + 64 + c4 * 4;
#pragma unroll
      for (int sx = 0; sx < 2; ++sx) {
        const int* fx = sx ? g.bx1_first : g.bx0_first;
        const float* wx = sx ? g.wx1 : g.wx0;
        for (int qx = fx[ix]; qx < fx[ix + 1]; ++qx) s += (wx[qx] * wyv) * ld4(row + (size_t)qx * X2_W);
      }
    }
  }
  st4(g_feat + (size_t)lp * 192 + c4 * 4, s);
}

// ---- X3: HRfeat, latent and frames at the two warped grids | t | zeros ----
__global__ __launch_bounds__(256) void k_x3_fwd(Geom g, const float* __restrict__ hrfeat,
                                                const float* __restrict__ flow, float* __restrict__ x3,
                                                long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long long n = idx / (X3_W / 4);
  const int c4 = (int)(idx - n * (X3_W / 4));
  const Pix p = pix_of(n, g.HH, g.WW);
  const f32x4 fv = ld4(flow + (size_t)n * 4);
  const float bx = g.lin_x[p.qx], by = g.lin_y[p.qy];
  const float gx[2] = {warp_axis(bx, fv[0], g.WW).g, warp_axis(bx, fv[2], g.WW).g};
  const float gy[2] = {warp_axis(by, fv[1], g.HH).g, warp_axis(by, fv[3], g.HH).g};
  const size_t plane = (size_t)g.H * g.W;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (c4 < 32) {
    const int k = c4 >> 4;
    v = sample4(hrfeat + (size_t)p.b * g.HH * g.WW * 64, 64, g.WW, corners(gx[k], gy[k], g.WW, g.HH), (c4 & 15) * 4);
  } else if (c4 < 128) {
    const int k = c4 >= 80, cl = c4 - (k ? 80 : 32);
    v = sample4(g.feat + (size_t)p.b * plane * 192, 192, g.W, corners(gx[k], gy[k], g.W, g.H), cl * 4);
  } else if (c4 < 131) {
    // columns 512 .. 523: frames@grid1 0..5, frames@grid2 0..5
    const float* fr = g.frames + (size_t)p.b * 6 * plane;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = (c4 - 128) * 4 + e, k = col >= 6, ch = col - 6 * k;
      v[e] = sample1(fr + ch * plane, g.W, corners(gx[k], gy[k], g.W, g.H));
    }
  } else {
    v[0] = g.t[p.b];
  }
  st4(x3 + (size_t)n * X3_W + c4 * 4, v);
}

STIF_DEV float wave_sum(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// One lane's share of the backward of a bilinear sample of channel `ch`: adds g * weight into the in-bounds corners
// of `gmap` (one hardware fp32 atomic per lane, the wave covering consecutive channels of a row) and returns the
// derivative of the sample with respect to the un-normalised coordinates, times g.  A corner outside the map counts
// as zero.  `gmap` NULL: no scatter (the frames).
struct DXY {
  float dx, dy;
};
STIF_DEV DXY sample_bwd(const float* map, float* gmap, size_t stride, int Wd, const Cn& c, int ch, float gch) {
  const size_t o00 = ((size_t)c.y0 * Wd + c.x0) * stride + ch, o01 = ((size_t)c.y0 * Wd + c.x1) * stride + ch;
  const size_t o10 = ((size_t)c.y1 * Wd + c.x0) * stride + ch, o11 = ((size_t)c.y1 * Wd + c.x1) * stride + ch;
  const bool b00 = c.vy0 && c.vx0, b01 = c.vy0 && c.vx1, b10 = c.vy1 && c.vx0, b11 = c.vy1 && c.vx1;
  const float v00 = b00 ? map[o00] : 0.f, v01 = b01 ? map[o01] : 0.f;
  const float v10 = b10 ? map[o10] : 0.f, v11 = b11 ? map[o11] : 0.f;
  if (gmap != nullptr) {
    if (b00) unsafeAtomicAdd(gmap + o00, gch * (c.wx0 * c.wy0));
    if (b01) unsafeAtomicAdd(gmap + o01, gch * (c.wx1 * c.wy0));
    if (b10) unsafeAtomicAdd(gmap + o10, gch * (c.wx0 * c.wy1));
    if (b11) unsafeAtomicAdd(gmap + o11, gch * (c.wx1 * c.wy1));
  }
  return {gch * ((v01 - v00) * c.wy0 + (v11 - v10) * c.wy1), gch * ((v10 - v00) * c.wx0 + (v11 - v01) * c.wx1)};
}

// One wave per HR pixel: lane l takes channel l of HRfeat, channels l, l + 64, l + 128 of the latent and (l < 6)
// frame plane l, for both grids.  g_flow is the wave's sum of the coordinate gradients through ix = ((g + 1) n - 1) / 2
// (n the sampled map's size) and g = base + flow / ((NN - 1) / 2), zero where the clamp is active; one plain store.
// CONTRIB (stif_dec_x3_bwd_contrib): g_flow as above and no scatter.  Lanes 0..3 store corner
// `lane` of the wave's two samples on each lattice as a weight and a packed sort word (key << 32) | e,
// e = (n * 2 + grid) * 4 + corner, key = the corner's pixel row of the map or the map's pixel count for a corner
// outside it; stif_segsum adds w * g_x3 sub-rows per destination in a fixed order.
struct X3Contrib {
  float *w_hr, *w_lr;
  long long *words_hr, *words_lr;
};
// corner j of sample_bwd's order (b00, b01, b10, b11) on a map of B items of Hd x Wd pixels, item b
STIF_DEV void put_corner(const Cn& c, int j, int b, int B, int Hd, int Wd, long long e, float* w, long long* words) {
  const bool hy = j >> 1, hx = j & 1;
  const bool ok = (hy ? c.vy1 : c.vy0) && (hx ? c.vx1 : c.vx0);
  const int y = hy ? c.y1 : c.y0, x = hx ? c.x1 : c.x0;
  const long long key = ok ? ((long long)b * Hd + y) * Wd + x : (long long)B * Hd * Wd;
  w[e] = ok ? (hx ? c.wx1 : c.wx0) * (hy ? c.wy1 : c.wy0) : 0.f;
  words[e] = (key << 32) | e;
}

struct X3Scatter {};   // the atomic path: an empty last kernel argument, which moves no other argument

template <class CT>
__global__ __launch_bounds__(256) void k_x3_bwd(Geom g, const float* __restrict__ hrfeat,
                                                const float* __restrict__ flow, const float* __restrict__ gx3,
                                                float* __restrict__ g_flow, float* __restrict__ g_hr,
                                                float* __restrict__ g_feat, long long N, CT ct) {
  constexpr bool CONTRIB = std::is_same<CT, X3Contrib>::value;
  const int lane = threadIdx.x & 63;
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const Pix p = pix_of(n, g.HH, g.WW);
  const f32x4 fv = ld4(flow + (size_t)n * 4);
  const float bx = g.lin_x[p.qx], by = g.lin_y[p.qy];
  const size_t plane = (size_t)g.H * g.W, hr_item = (size_t)p.b * g.HH * g.WW * 64, lr_item = (size_t)p.b * plane * 192;
  const float* grow = gx3 + (size_t)n * X3_W;
  f32x4 res;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const Warp wx = warp_axis(bx, fv[2 * k], g.WW), wy = warp_axis(by, fv[2 * k + 1], g.HH);
    const Cn ch = corners(wx.g, wy.g, g.WW, g.HH), cl = corners(wx.g, wy.g, g.W, g.H);
    if constexpr (CONTRIB) {
      if (lane < 4) {
        const long long e = (n * 2 + k) * 4 + lane;
        put_corner(ch, lane, p.b, g.B, g.HH, g.WW, e, ct.w_hr, ct.words_hr);
        put_corner(cl, lane, p.b, g.B, g.H, g.W, e, ct.w_lr, ct.words_lr);
      }
    }
    float* const ghr = CONTRIB ? nullptr : g_hr + hr_item;
    float* const glr = CONTRIB ? nullptr : g_feat + lr_item;
    const DXY dh = sample_bwd(hrfeat + hr_item, ghr, 64, g.WW, ch, lane, grow[k * 64 + lane]);
    float lx = 0.f, ly = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int c = lane + 64 * j;
      const DXY d = sample_bwd(g.feat + lr_item, glr, 192, g.W, cl, c, grow[128 + k * 192 + c]);
      lx += d.dx, ly += d.dy;
    }
    if (lane < 6) {
      const DXY d = sample_bwd(g.frames + ((size_t)p.b * 6 + lane) * plane, nullptr, 1, g.W, cl, 0,
                               grow[512 + k * 6 + lane]);
      lx += d.dx, ly += d.dy;
    }
    const float tx = wave_sum(dh.dx * (0.5f * (float)g.WW) + lx * (0.5f * (float)g.W));
    const float ty = wave_sum(dh.dy * (0.5f * (float)g.HH) + ly * (0.5f * (float)g.H));
    res[2 * k] = wx.pass ? tx / (((float)g.WW - 1.f) / 2.f) : 0.f;
    res[2 * k + 1] = wy.pass ? ty / (((float)g.HH - 1.f) / 2.f) : 0.f;
  }
  if (lane == 0) st4(g_flow + (size_t)n * 4, res);
}

int fail_as(const char* fn, const char* why) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  return stif_fail(STIF_E_INVALID, msg);
}

// 0 and *N = B HH WW, or the status of the rejection
int check_geom(const char* fn, const Geom* g, long long* N) {
  if (!g) return fail_as(fn, "null geometry");
  if (g->B < 1 || g->H < 1 || g->W < 1) return fail_as(fn, "B, H, W must be >= 1");
  if (g->HH < 2 || g->WW < 2) return fail_as(fn, "HH and WW must be >= 2 (the warp grid divides by n - 1)");
  if (!g->feat || !g->frames || !g->t) return fail_as(fn, "null pointer (feat, frames, t)");
  if (!g->near_y || !g->near_x || !g->rel_y || !g->rel_x || !g->by0 || !g->by1 || !g->bx0 || !g->bx1 || !g->wy0 ||
      !g->wy1 || !g->wx0 || !g->wx1 || !g->lin_y || !g->lin_x)
    return fail_as(fn, "null table pointer");
  if (!g->near_y_first || !g->near_x_first || !g->by0_first || !g->by1_first || !g->bx0_first || !g->bx1_first)
    return fail_as(fn, "null inverse table pointer");
  *N = (long long)g->B * g->HH * g->WW;
  if (*N * (X3_W / 4) > 0x7fffffffLL || (long long)g->B * g->H * g->W * 48 > 0x7fffffffLL)
    return fail_as(fn, "more than 2^31 - 1 float4 of a matrix");
  return 0;
}

unsigned blocks_of(long long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

extern "C" int stif_dec_x1_fwd(const stif_dec_train_geom* g, float* x1, void* stream) {
  const char* fn = "stif_dec_x1_fwd";
  long long N;
  if (int rc = check_geom(fn, g, &N)) return rc;
  if (!x1) return fail_as(fn, "null pointer (x1)");
  const long long total = N * (X1_W / 4);
  hipLaunchKernelGGL(k_x1_fwd, dim3(blocks_of(total)), dim3(256), 0, static_cast<hipStream_t>(stream), *g, x1, total);
  return stif_check_launch(fn);
}

extern "C" int stif_dec_x1_bwd(const stif_dec_train_geom* g, const float* g_x1, float* g_feat, void* stream) {
  const char* fn = "stif_dec_x1_bwd";
  long long N;
  if (int rc = check_geom(fn, g, &N)) return rc;
  if (!g_x1 || !g_feat) return fail_as(fn, "null pointer (g_x1, g_feat)");
  const long long total = (long long)g->B * g->H * g->W * 48;
  hipLaunchKernelGGL(k_x1_bwd, dim3(blocks_of(total)), dim3(256), 0, static_cast<hipStream_t>(stream), *g, g_x1, g_feat,
                     total);
  return stif_check_launch(fn);
}

extern "C" int stif_dec_x2_fwd(const stif_dec_train_geom* g, const float* hrfeat, float* x2, void* stream) {
  const char* fn = "stif_dec_x2_fwd";
  long long N;
  if (int rc = check_geom(fn, g, &N)) return rc;
  if (!hrfeat || !x2) return fail_as(fn, "null pointer (hrfeat, x2)");
  const long long total = N * (X2_W / 4);
  hipLaunchKernelGGL(k_x2_fwd, dim3(blocks_of(total)), dim3(256), 0, static_cast<hipStream_t>(stream), *g, hrfeat, x2,
                     total);
  return stif_check_launch(fn);
}

extern "C" int stif_dec_x2_bwd(const stif_dec_train_geom* g, const float* g_x2, float* g_hrfeat, float* g_feat,
                               void* stream) {
  const char* fn = "stif_dec_x2_bwd";
  long long N;
  if (int rc = check_geom(fn, g, &N)) return rc;
  if (!g_x2 || !g_hrfeat || !g_feat) return fail_as(fn, "null pointer (g_x2, g_hrfeat, g_feat)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_x2_bwd_hr, dim3(blocks_of(N * 16)), dim3(256), 0, st, g_x2, g_hrfeat, N * 16);
  if (int rc = stif_check_launch(fn)) return rc;
  const long long total = (long long)g->B * g->H * g->W * 48;
  hipLaunchKernelGGL(k_x2_bwd_feat, dim3(blocks_of(total)), dim3(256), 0, st, *g, g_x2, g_feat, total);
  return stif_check_launch(fn);
}

extern "C" int stif_dec_x3_fwd(const stif_dec_train_geom* g, const float* hrfeat, const float* flow, float* x3,
                               void* stream) {
  const char* fn = "stif_dec_x3_fwd";
  long long N;
  if (int rc = check_geom(fn, g, &N)) return rc;
  if (!hrfeat || !flow || !x3) return fail_as(fn, "null pointer (hrfeat, flow, x3)");
  const long long total = N * (X3_W / 4);
  hipLaunchKernelGGL(k_x3_fwd, dim3(blocks_of(total)), dim3(256), 0, static_cast<hipStream_t>(stream), *g, hrfeat, flow,
                     x3, total);
  return stif_check_launch(fn);
}

extern "C" int stif_dec_x3_bwd(const stif_dec_train_geom* g, const float* hrfeat, const float* flow, const float* g_x3,
                               float* g_flow, float* g_hrfeat, float* g_feat, void* stream) {
  const char* fn = "stif_dec_x3_bwd";
  long long N;
  if (int rc = check_geom(fn, g, &N)) return rc;
  if (!hrfeat || !flow || !g_x3 || !g_flow || !g_hrfeat || !g_feat)
    return fail_as(fn, "null pointer (hrfeat, flow, g_x3, g_flow, g_hrfeat, g_feat)");
  hipLaunchKernelGGL(k_x3_bwd<X3Scatter>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     *g, hrfeat, flow, g_x3, g_flow, g_hrfeat, g_feat, N, X3Scatter{});
  return stif_check_launch(fn);
}

extern "C" int stif_dec_x3_bwd_contrib(const stif_dec_train_geom* g, const float* hrfeat, const float* flow,
                                       const float* g_x3, float* g_flow, float* w_hr, long long* words_hr,
                                       float* w_lr, long long* words_lr, void* stream) {
  const char* fn = "stif_dec_x3_bwd_contrib";
  long long N;
  if (int rc = check_geom(fn, g, &N)) return rc;
  if (!hrfeat || !flow || !g_x3 || !g_flow) return fail_as(fn, "null pointer (hrfeat, flow, g_x3, g_flow)");
  if (!w_hr || !words_hr || !w_lr || !words_lr) return fail_as(fn, "null pointer (w_hr, words_hr, w_lr, words_lr)");
  if (N > 0x7fffffffLL / 8) return fail_as(fn, "E = B * HH * WW * 8 must be < 2^31");
  if ((reinterpret_cast<uintptr_t>(words_hr) | reinterpret_cast<uintptr_t>(words_lr)) & 7)
    return fail_as(fn, "words_hr and words_lr must be 8-byte aligned");
  hipLaunchKernelGGL(k_x3_bwd<X3Contrib>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     *g, hrfeat, flow, g_x3, g_flow, static_cast<float*>(nullptr), static_cast<float*>(nullptr), N,
                     X3Contrib{w_hr, w_lr, words_hr, words_lr});
  return stif_check_launch(fn);
}
