// Implicit SIREN decoder of LunaTokis.decoding (Sakuya_arch_test.py:364-459) for gfx950.
//
// The reference materialises, per query time t, ~2,300 floats per HR pixel of
// grid_sample gathers and torch.cat results and runs three nn.Linear stacks over
// them.  Here the work is split into:
//   (0) an LR projection (stif_conv2d_nhwc, 1x1, 200 -> 256 channels): every linear
//       input block that is gathered from the LR maps (feat 192 + inp 6) is projected
//       once per LR pixel -- nearest/bilinear sampling commutes with a linear map,
//       so the per-HR-pixel work gathers 64-wide projections instead of 198-wide
//       inputs (P1 nearest, P2 bilinear at the HR centre, P3/P4 bilinear at the
//       warped grids);
//   (1) k_dec1: per HR pixel feat_imnet -> HRfeat (64) and flow_imnet -> flow (4);
//   (2) k_dec2: per HR pixel warpgrid (warplayer.py:25-39) + bilinear HRfeat at both
//       warped grids + encode_imnet -> RGB.
// Each wave owns 32 HR pixels (one per lane, both lane halves hold the same pixel);
// every SIREN layer is a chain of v_mfma_f32_32x32x2_f32 with features in the
// accumulator registers (layout in dec_layout.h), sin(30 z) applied in registers.
#include "dec_layout.h"
#include "stif_common.h"
#include "tuning.h"
#include "stif.h"
#include "abi_util.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <type_traits>

namespace {

using namespace stif_dec;

// F16 (stif_pack_dec_mlp_ex with STIF_CONV_F16X3): every 32x32 weight tile is a split-fp16 tile
// ([m][plane h|l][lane][8 halves], W * 2^10) and every register tile that feeds one is split too
// (x * 2^4, split_f16x3), so MFMA accumulators hold values x 2^14 -- everything added into them
// (gathered projections, bias terms, the fp32 image tiles, packed x 2^14) is scaled to match and
// every consumer unscales (ACC_S).
template <int F16>
struct XT;   // a 32-feature register tile as an MFMA B operand
template <>
struct XT<0> {
  f32x16 v;
};
template <>
struct XT<1> {
  f16x8 h[2], l[2];
};
template <int F16>
STIF_DEV XT<F16> xop(const f32x16& x) {
  XT<F16> o;
  if constexpr (F16) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
      split_f16x3(f32x4{x[8 * m], x[8 * m + 1], x[8 * m + 2], x[8 * m + 3]},
                  f32x4{x[8 * m + 4], x[8 * m + 5], x[8 * m + 6], x[8 * m + 7]}, o.h[m], o.l[m]);
  } else {
    o.v = x;
  }
  return o;
}
template <int F16>
constexpr float ACC_S = F16 ? F16X3_UNSCALE : 1.f;   // accumulator -> value
template <int F16>
constexpr float ACC_IN = F16 ? 16384.f : 1.f;        // value -> accumulator

// the 16 biases of one 32-feature register tile (features F(r, hf)) as 4 vector loads
struct Bias32 {
  f32x4 v[4];
};
STIF_DEV Bias32 bias_ld(const float* __restrict__ b, int hf) {
  Bias32 o;
#pragma unroll
  for (int v = 0; v < 4; ++v) o.v[v] = ld4(b + 8 * v + 4 * hf);
  return o;
}
// SineLayer: sin(30 * (z + b)) (SIREN.py:44-45, omega_0 = 30); the packed weights and biases of every
// sine layer carry the factor 30 (pack.cpp), so the kernel evaluates sin(z + b)
template <int F16>
STIF_DEV f32x16 bias_sin(f32x16 z, const Bias32& bb) {
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int e = 0; e < 4; ++e) z[4 * v + e] = siren_sin<F16>(fmaf(z[4 * v + e], ACC_S<F16>, bb.v[v][e]));
  return z;
}
template <int F16>
STIF_DEV f32x16 bias_sin(f32x16 z, const float* __restrict__ b, int hf) {
  return bias_sin<F16>(z, bias_ld(b, hf));
}

template <int F16>
STIF_DEV f32x16 bias_add(f32x16 z, const float* __restrict__ b, int hf) {
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const f32x4 bb = ld4(b + 8 * v + 4 * hf);
#pragma unroll
    for (int e = 0; e < 4; ++e) z[4 * v + e] = fmaf(z[4 * v + e], ACC_S<F16>, bb[e]);
  }
  return z;
}

struct Bilin {  // grid_sample bilinear corners (align_corners=False, zeros padding)
  int o00, o01, o10, o11;      // element offsets (pixel index)
  float w00, w01, w10, w11;    // weights, 0 for out-of-range corners
};

// ATen grid_sampler_2d bilinear: ix = ((x + 1) * W - 1) / 2, corner weights
// nw = (ix_se - ix) * (iy_se - iy), ...; corners outside the map contribute 0.
struct Corners {  // the same, as clamped corner columns / rows
  int cx0, cx1, cy0, cy1;
  float w00, w01, w10, w11;
};
STIF_DEV Corners bilin_corners(float gx, float gy, int Wd, int Hd) {
  const float ix = ((gx + 1.f) * (float)Wd - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)Hd - 1.f) / 2.f;
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
  const float wx1 = ix - fx0, wx0 = (fx0 + 1.f) - ix;
  const float wy1 = iy - fy0, wy0 = (fy0 + 1.f) - iy;
  const bool vx0 = x0 >= 0 && x0 < Wd, vx1 = x1 >= 0 && x1 < Wd;
  const bool vy0 = y0 >= 0 && y0 < Hd, vy1 = y1 >= 0 && y1 < Hd;
  const int cx0 = min(max(x0, 0), Wd - 1), cx1 = min(max(x1, 0), Wd - 1);
  const int cy0 = min(max(y0, 0), Hd - 1), cy1 = min(max(y1, 0), Hd - 1);
  Corners b;
  b.cx0 = cx0; b.cx1 = cx1; b.cy0 = cy0; b.cy1 = cy1;
  b.w00 = (vx0 && vy0) ? wx0 * wy0 : 0.f;
  b.w01 = (vx1 && vy0) ? wx1 * wy0 : 0.f;
  b.w10 = (vx0 && vy1) ? wx0 * wy1 : 0.f;
  b.w11 = (vx1 && vy1) ? wx1 * wy1 : 0.f;
  return b;
}
STIF_DEV Bilin bilin(float gx, float gy, int Wd, int Hd) {
  const Corners c = bilin_corners(gx, gy, Wd, Hd);
  Bilin b;
  b.o00 = c.cy0 * Wd + c.cx0; b.o01 = c.cy0 * Wd + c.cx1; b.o10 = c.cy1 * Wd + c.cx0; b.o11 = c.cy1 * Wd + c.cx1;
  b.w00 = c.w00; b.w01 = c.w01; b.w10 = c.w10; b.w11 = c.w11;
  return b;
}

// The corners of the HR pixel centre (row py, column px of the virtual grid) in a map `pitch` pixels wide, from the
// host's per-row / per-column tables (stif_dec_tables or stif_dec_image: by0 .. wx1)
template <class TAB>
STIF_DEV Bilin bilin_tab(const TAB& tb, int py, int px, int pitch) {
  Bilin b;
  // the table pointers as locals first: indexing tb.by0[py] .. directly compiles to the same code but for one
  // commuted v_add_u32 in 12 of the k_dec1 kernels, and this form keeps them instruction for instruction
  const int *by0 = tb.by0, *by1 = tb.by1, *bx0 = tb.bx0, *bx1 = tb.bx1;
  const float *wy0_ = tb.wy0, *wy1_ = tb.wy1, *wx0_ = tb.wx0, *wx1_ = tb.wx1;
  const int y0 = by0[py], y1 = by1[py], x0 = bx0[px], x1 = bx1[px];
  const float wy0 = wy0_[py], wy1 = wy1_[py], wx0 = wx0_[px], wx1 = wx1_[px];
  b.o00 = y0 * pitch + x0; b.o01 = y0 * pitch + x1; b.o10 = y1 * pitch + x0; b.o11 = y1 * pitch + x1;
  b.w00 = wx0 * wy0; b.w01 = wx1 * wy0; b.w10 = wx0 * wy1; b.w11 = wx1 * wy1;
  return b;
}

// Stage 2's two warped grids of one HR pixel: warpgrid (warplayer.py:25-39) = linspace base + flow / ((n - 1) / 2)
// over the virtual WW x HH grid, then the decoder's clamp to (-1 + 1e-6, 1 - 1e-6) (Sakuya_arch_test.py:428,441).
// The HRfeat corners stage 2 reads are bilin_corners(g, WW, HH) of these; k_dec_bounds reduces the box of the same
// expressions, so the two cannot drift apart.
struct WarpGrids {
  float g1x, g1y, g2x, g2y;
};
STIF_DEV WarpGrids warp_grids(const f32x4 fv, float bx, float by, int WW, int HH) {
  const float lo = -1.f + 1e-6f, hi = 1.f - 1e-6f;
  const float dx = ((float)WW - 1.f) / 2.f, dy = ((float)HH - 1.f) / 2.f;
  WarpGrids g;
  g.g1x = fminf(fmaxf(bx + fv[0] / dx, lo), hi), g.g1y = fminf(fmaxf(by + fv[1] / dy, lo), hi);
  g.g2x = fminf(fmaxf(bx + fv[2] / dx, lo), hi), g.g2y = fminf(fmaxf(by + fv[3] / dy, lo), hi);
  return g;
}

// The addressing forms of the pixel front end (pixel_of): the whole HH x WW grid, the query rectangle of a
// stif_dec_window, or a list of points (stif_dec_points).  The kernels take the form as a template argument; the
// bool WIN of the host code converts to the first two.
constexpr int GRID = 0, WINDOW = 1, PTS = 2;

// The range report of stage 2; the windowed and the point kernels OR bit 0 in, so that bilin_hr's bit 1 and the
// points' bit 3 survive it
template <bool OR>
STIF_DEV void report_range_w(int* status, bool bad) {
  if constexpr (OR) {
    if (status != nullptr && bad) atomicOr(status, 1);
  } else {
    report_range(status, bad);
  }
}

// The HRfeat gather of stage 2 at grid (gx, gy).  WINDOW: hrfeat holds the F rectangle of the grid, [fh][fw][64]; a
// corner outside it is clamped into it and reported (bit 1 of *status), so a too-small F gives a flagged wrong
// result and never an out-of-range read.  PTS: hrfeat holds the eight corner rows of every point, [npts][8][64] in
// k_dec_corners' order, and the corners of this grid are rows slot .. slot + 3 (slot = 8 p for grid 1, 8 p + 4 for
// grid 2) -- the offsets depend on nothing the kernel computes, the weights are bilin_corners' as everywhere.
template <int FORM>
STIF_DEV Bilin bilin_hr(float gx, float gy, int WW, int HH, const stif_dec_window& win, int* status, int slot = 0) {
  if constexpr (FORM == GRID) {
    return bilin(gx, gy, WW, HH);
  } else if constexpr (FORM == PTS) {
    const Corners c = bilin_corners(gx, gy, WW, HH);
    Bilin b;
    b.o00 = slot; b.o01 = slot + 1; b.o10 = slot + 2; b.o11 = slot + 3;
    b.w00 = c.w00; b.w01 = c.w01; b.w10 = c.w10; b.w11 = c.w11;
    return b;
  } else {
    const Corners c = bilin_corners(gx, gy, WW, HH);
    const int ry0 = c.cy0 - win.fy0, ry1 = c.cy1 - win.fy0, rx0 = c.cx0 - win.fx0, rx1 = c.cx1 - win.fx0;
    const int y0 = min(max(ry0, 0), win.fh - 1), y1 = min(max(ry1, 0), win.fh - 1);
    const int x0 = min(max(rx0, 0), win.fw - 1), x1 = min(max(rx1, 0), win.fw - 1);
    if (status != nullptr && (y0 != ry0 || y1 != ry1 || x0 != rx0 || x1 != rx1)) atomicOr(status, 2);
    Bilin b;
    b.o00 = y0 * win.fw + x0; b.o01 = y0 * win.fw + x1; b.o10 = y1 * win.fw + x0; b.o11 = y1 * win.fw + x1;
    b.w00 = c.w00; b.w01 = c.w01; b.w10 = c.w10; b.w11 = c.w11;
    return b;
  }
}

// bilinear sample of channel block [c0, c0+64) of an NHWC map with `stride` channels, into two register tiles
// (features F(r, hf) of each 32-block).  The 8 channel groups (4 corner loads, 16 VGPRs each) are loaded GPB at a
// time, all of a batch before its first blend: 8 / GPB memory latencies at 16 GPB VGPRs of loads in flight.
template <int GPB>
STIF_DEV void gather64(f32x16* dst, const float* __restrict__ base, int stride, int c0, const Bilin& b, int hf) {
  const int c = c0 + 4 * hf;
  const float* p00 = base + (size_t)b.o00 * stride + c;
  const float* p01 = base + (size_t)b.o01 * stride + c;
  const float* p10 = base + (size_t)b.o10 * stride + c;
  const float* p11 = base + (size_t)b.o11 * stride + c;
#pragma unroll
  for (int g0 = 0; g0 < 8; g0 += GPB) {
    f32x4 cr[GPB][4];
#pragma unroll
    for (int g = 0; g < GPB; ++g) {   // group g0 + g = (ot, v) = (>> 2, & 3): channels 8 (g0 + g) + 4 hf ..
      const int o = 8 * (g0 + g);
      cr[g][0] = ld4(p00 + o);
      cr[g][1] = ld4(p01 + o);
      cr[g][2] = ld4(p10 + o);
      cr[g][3] = ld4(p11 + o);
    }
#pragma unroll
    for (int g = 0; g < GPB; ++g) {
      f32x4 s = b.w00 * cr[g][0] + b.w01 * cr[g][1] + b.w10 * cr[g][2] + b.w11 * cr[g][3];
      // combine the corners here, in load order: otherwise the blend is sunk to the first use (past a
      // barrier) and all four corners of every channel stay live
      asm volatile("" : "+v"(s));
      const int gg = g0 + g;
#pragma unroll
      for (int e = 0; e < 4; ++e) dst[gg >> 2][4 * (gg & 3) + e] = s[e];
    }
    if constexpr (GPB < 8) asm volatile("" ::: "memory");   // the next batch's loads stay behind this one's blends
  }
}

// z[ot] += W_img . img: the 6 image channels (padded to 8) are one K chunk, so lane half h supplies
// channels 4h..4h+3 as the B operand of the first 4 MFMAs of a packed tile (features F(e, h), e < 4)
STIF_DEV void img_mma(f32x16* z, const float* __restrict__ wt, const f32x4 im4, int lane) {
#pragma unroll
  for (int ot = 0; ot < 2; ++ot) {
    const f32x4 w0 = ld4(wt + ot * T + lane * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) z[ot] = mfma32(w0[e], im4[e], z[ot]);
  }
}

// bilinear sample of channels 4h..4h+3 of a [ih][iw][8] high-resolution image
STIF_DEV f32x4 img_sample(const float* __restrict__ I, const Bilin& b, int hf) {
  const float* c = I + 4 * hf;
  return b.w00 * ld4(c + b.o00 * IMG_C) + b.w01 * ld4(c + b.o01 * IMG_C) + b.w10 * ld4(c + b.o10 * IMG_C) +
         b.w11 * ld4(c + b.o11 * IMG_C);
}

// The HR pixel a lane works on, in workgroups of NW waves at PPW pixels per wave (lane & (PPW - 1): the other lanes
// hold the same pixels).  The pixels are counted over the whole HH x WW grid or, WIN, over win's query rectangle
// (row-major per item); lanes past the end redo the last pixel and store nothing (valid).
// PTS: the pixels are the n * npts points of a stif_dec_points (item pc / npts, point pt = pc % npts); ly / lx are
// the point's row / column of the virtual grid, clamped into it (point_yx).
struct Pixel {
  bool valid;
  long long pc;     // index among all n * rows * columns pixels (PTS: n * npts points)
  int item, ly, lx; // item, row and column in the grid / rectangle
  int pt;           // PTS: the point's index in its item's list
};
// Row and column of point pt of `item`, clamped into the HH x WW grid: every table read and every address made from
// them stays inside its buffer whatever the list holds.  A clamp is reported as bit 3 (value 8) of *status.
STIF_DEV void point_yx(const stif_dec_points& pts, int item, int pt, int HH, int WW, int* status, int& y, int& x) {
  const int ry = pts.y[item * pts.y_item + pt], rx = pts.x[item * pts.x_item + pt];
  y = min(max(ry, 0), HH - 1), x = min(max(rx, 0), WW - 1);
  if (status != nullptr && (y != ry || x != rx)) atomicOr(status, 8);
}
template <int NW, int PPW, int FORM, class TQ>
STIF_DEV Pixel pixel_of(int wv, int lane, int n, int HH, int WW, const stif_dec_window& win, const TQ& tq,
                        int* status) {
  Pixel o;
  if constexpr (FORM == PTS) {
    const long long total = (long long)n * tq.npts;
    const long long p = ((long long)xcd_block(blockIdx.x, gridDim.x) * NW + wv) * PPW + (lane & (PPW - 1));
    o.valid = p < total;
    o.pc = o.valid ? p : total - 1;
    o.item = (int)(o.pc / tq.npts);
    o.pt = (int)(o.pc - (long long)o.item * tq.npts);
    point_yx(tq, o.item, o.pt, HH, WW, status, o.ly, o.lx);
  } else {
    constexpr bool WIN = FORM == WINDOW;
    const int GH = WIN ? win.hh : HH, GW = WIN ? win.ww : WW;   // the rectangle the pixels are counted over
    // the count before the lane's index, in this order: computed the other way round the existing kernels come out
    // with a different schedule and register allocation
    const long long total = (long long)n * GH * GW;
    const long long p = ((long long)xcd_block(blockIdx.x, gridDim.x) * NW + wv) * PPW + (lane & (PPW - 1));
    o.valid = p < total;
    o.pc = o.valid ? p : total - 1;
    o.item = (int)(o.pc / ((long long)GH * GW));
    const int rem = (int)(o.pc - (long long)o.item * GH * GW);
    o.ly = rem / GW, o.lx = rem - o.ly * GW;
    o.pt = 0;
  }
  return o;
}

// The query time of a pixel, by the kind TQ of the kernel's time argument.  0: one value per item, tq[item] (the
// scalar kernels).  1 (time field): every pixel its own, t[item * item + gy * row + gx * col] at row gy / column gx
// of the virtual grid -- strides in elements, 0 broadcasts.  2 (points): t[item * t_item + pt * t_point] of the
// stif_dec_points, which is the kernel's point list as well.  A tail lane redoes the last pixel (pixel_of), so its
// read is one a valid lane makes too.
template <int TQ>
struct TimeArg {
  typedef const float* __restrict__ type;
};
template <>
struct TimeArg<1> {
  typedef stif_dec_time type;
};
template <>
struct TimeArg<2> {
  typedef stif_dec_points type;
};
template <int FORM, bool TF>
constexpr int TQK = FORM == PTS ? 2 : TF ? 1 : 0;
template <int TQ>
STIF_DEV float time_at(const typename TimeArg<TQ>::type& tq, int item, int gy, int gx, int pt = 0) {
  if constexpr (TQ == 2) return tq.t[item * tq.t_item + pt * tq.t_point];
  else if constexpr (TQ == 1) return tq.t[item * tq.item + gy * tq.row + gx * tq.col];
  else return tq[item];
}

// The local ensemble's blend weight of decode bl.k at row gy / column gx of the virtual grid, as
// coords.ensemble_weights computes it in numpy's fp32: area_j = |rel_y_j rel_x_j| + 1e-9 of the four shifted
// queries, tot = ((a_0 + a_1) + a_2) + a_3, decode k weighted by the diagonally opposite area (3 - k) over tot.
// Every operation rounds on its own (no contraction) and the division is the correctly rounded one.
STIF_DEV float blend_weight(const stif_dec_blend& bl, int gy, int gx) {
#pragma clang fp contract(off)
  float a[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = __fadd_rn(fabsf(__fmul_rn(bl.rel_y[j][gy], bl.rel_x[j][gx])), 1e-9f);
  const float tot = __fadd_rn(__fadd_rn(__fadd_rn(a[0], a[1]), a[2]), a[3]);
  const float ak = bl.k == 0 ? a[3] : bl.k == 1 ? a[2] : bl.k == 2 ? a[1] : a[0];
  return __fdiv_rn(ak, tot);
}

// Stage 2's epilogue: the pixel's RGB (o4 + bias) into the NCHW output -- WIN: through win's output addressing --
// and, REPORT, the range report.  Stage 1's flow counts too: the warpgrid clamp maps a NaN flow to a finite grid,
// so an out-of-range flow_imnet operand would otherwise leave a finite but wrong pixel.
// BLEND (local ensemble, decode bl.k of four launched one after the other on one stream): the first launch
// (bl.accumulate = 0) stores w_k rgb without reading out, the others store fma(rgb, w_k, out), spelled out so that
// they cannot come out differently.  k_blend4 as the compiler builds it for gfx950 contracts
// `r = p0 w0; r += p1 w1` into fma(p0, w0, p1 * w1): its one rounded product is decode 1's, then come the fmas of
// decodes 0, 2 and 3 -- so launching the decodes in the order 1, 0, 2, 3 reproduces its bits (model.py does).
// The pixel's lane owns its three output elements: no atomics.
// PTS: the caller passes the [n][3][npts] output as a one-row grid (py = 0, px = the point, HH = 1, WW = npts) and,
// BLEND, the point's clamped row / column of the virtual grid (gy, gx), where its weight is taken.
template <int FORM, bool REPORT, bool BLEND = false>
STIF_DEV void store_rgb(float* __restrict__ out, const float* __restrict__ mlp, const float* o4, const f32x4 fv,
                        int item, int py, int px, int HH, int WW, const stif_dec_window& win, int* status,
                        const stif_dec_blend& bl, int gy = 0, int gx = 0) {
  constexpr bool WIN = FORM == WINDOW;
  static_assert(FORM != GRID || !BLEND, "the blending epilogue is the windowed and the point stages'");
  const size_t plane = WIN ? (size_t)win.out_plane : (size_t)HH * WW;
  float* o = WIN ? out + (size_t)item * win.out_item + (size_t)py * win.out_pitch + px
                 : out + (size_t)item * 3 * plane + (size_t)py * WW + px;
  bool bad = not_finite((fv[0] + fv[1]) + (fv[2] + fv[3]));
  float rgb[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rgb[c] = o4[c] + mlp[E_B4 + c];
    bad |= not_finite(rgb[c]);
    if constexpr (!BLEND) o[c * plane] = rgb[c];
  }
  if constexpr (BLEND) {
    const float wk = WIN ? blend_weight(bl, win.y0 + py, win.x0 + px) : blend_weight(bl, gy, gx);
    if (!bl.accumulate) {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane] = __fmul_rn(rgb[c], wk);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c * plane] = __fmaf_rn(rgb[c], wk, o[c * plane]);
    }
  }
  if constexpr (REPORT) report_range_w<FORM != GRID>(status, bad);
}

// ---- weight streaming: a workgroup consumes its MLP weight tiles segment by segment; each segment
// (a few 4-KB tiles: one layer, or one output tile's K-tiles) is LDS-DMA'd while the previous one
// is being consumed (double-buffered, one barrier per segment), and every wave reads its A
// operands from LDS -- one tile feeds 16 MFMAs in each wave of the workgroup.
// waves per workgroup of k_dec1: 4-wave workgroups, OCC1 (below) of them per CU -- 4 (36 KB LDS, <= 128 VGPRs
// each; the HRIMG variants 3: 52 KB, <= 168, and MODE 2 2: 69 KB): the waves sharing a SIMD come from different
// workgroups, so one's segment barrier, gather or sin stretch overlaps the others' MFMAs
constexpr int NW1 = 4;       // k_dec1 (8-wave workgroups at four waves per SIMD: +8 %, profiles/r06_dec_ab.log)
constexpr int DEC2_NW = 4;   // k_dec2: 8 layer-3 accumulator tiles (128 VGPRs) live
constexpr int DEC2_WPE = 2;  // waves per SIMD k_dec2 is register-budgeted for (2 workgroups/CU, 80 KB LDS each)
constexpr int SEG = 10;      // max tiles per segment (k_dec2)
constexpr int SEG1 = 8;      // max tiles per segment (k_dec1)

// Buffer loads with the tile offset in SGPRs: the per-lane operand is the same lane*16 for every
// tile (flat global_load_lds would keep a 64-bit VGPR address per hoisted tile live).
STIF_DEV void dec_dma(__amdgpu_buffer_rsrc_t rm, float* dst, int lane, int soff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rm, dst, 16, (unsigned)(lane * 16), soff, 0, 0);
}
template <int NW>
STIF_DEV void dma_tiles(float* dst, __amdgpu_buffer_rsrc_t rm, int src, int ntiles, int wv, int lane) {
  if ((ntiles * 4) % NW == 0) {
    // the same number of pieces per wave, known at compile time: the compiler counts them in vmcnt, so
    // waiting for a load issued before the DMA does not wait for the DMA
#pragma unroll
    for (int i = 0; i < ntiles * 4 / NW; ++i)
      dec_dma(rm, dst + (wv + i * NW) * 256, lane, (src + (wv + i * NW) * 256) * 4);
  } else {
    for (int k = wv; k < ntiles * 4; k += NW)
      dec_dma(rm, dst + k * 256, lane, (src + k * 256) * 4);
  }
}

STIF_DEV __amdgpu_buffer_rsrc_t mlp_rsrc(const float* mlp) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)mlp, (short)0, (int)(MLP_FLOATS * 4), 0x00020000);
}

// acc += W_tile . x, tile in LDS ([v][lane][4]), x = one 32-feature register tile
template <int F16>
STIF_DEV void tile_mma(f32x16& acc, const float* t, const XT<F16>& xt, int lane) {
  const float* b = t + lane * 4;
  if constexpr (F16) {
    // tile [m][plane][lane][8 halves]: element e of half-tile m = feature F(8m + e, lane >> 5)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const f16x8 ah = ldh8(b + (2 * m) * 256), al = ldh8(b + (2 * m + 1) * 256);
      acc = mfma16h(ah, xt.h[m], acc);
      acc = mfma16h(al, xt.h[m], acc);
      acc = mfma16h(ah, xt.l[m], acc);
    }
  } else {
    const f32x16& x = xt.v;
    const f32x4 w0 = ld4(b), w1 = ld4(b + 256), w2 = ld4(b + 512), w3 = ld4(b + 768);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma32(w0[e], x[e], acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma32(w1[e], x[4 + e], acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma32(w2[e], x[8 + e], acc);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = mfma32(w3[e], x[12 + e], acc);
  }
  // keep the compiler from hoisting the LDS reads of many tiles ahead (VGPR budget)
  __builtin_amdgcn_sched_barrier(0);
}

// o[c] += W[c][32 kt + F(r, hf)] . x[r] over this lane's 16 features of register tile kt (W: plain
// [NO][256] rows in LDS; the two lane halves read two addresses per instruction, a broadcast)
template <int NO>
STIF_DEV void narrow_dot(float* o, const float* W, int kt, const f32x16& x, int hf) {
#pragma unroll
  for (int c = 0; c < NO; ++c)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const f32x4 w = ld4(W + c * 256 + kt * 32 + 8 * v + 4 * hf);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[c] = fmaf(w[e], x[4 * v + e], o[c]);
    }
}

// MODE 0: feat_imnet + flow_imnet fused (the flow stage reads the pixel's own HRfeat);
// MODE 1: feat_imnet only; MODE 2: flow_imnet only, reading HRfeat at (hr_y, hr_x) of the query
// (local ensemble).  HRIMG: the flow stage's image input comes from the high-resolution image.
// OCC1, the workgroups per CU a k_dec1 instantiation is laid out for:
// 4 (MODE 0 / 1): 4-tile segments (36 KB of LDS) and 128 registers; flow layer 1 arrives after the last feat step
//   and flow segment 0 after flow layer 0.  C0 dec1 869 -> 758 us (2 -> 3, profiles/r04_dec1_occ_ab.log) -> 720 us
//   (3 -> 4; C2 11.6 -> 11.1 ms, profiles/r04_dec1_occ4_ab.log), all bit-identical
// 3 (the HRIMG variants, decoding_test's: at 128 registers their image gather spills): 6-tile segments (52 KB) and
//   a 168-register budget; flow layer 1's second output tile arrives after the last feat step
// 2 (MODE 2): 8-tile segments (69 KB), 256 registers
template <int MODE, bool HRIMG>
constexpr int OCC1 = MODE == 2 ? 2 : HRIMG ? 3 : 4;
template <int MODE, bool HRIMG>
constexpr int S1 = OCC1<MODE, HRIMG> == 4 ? 4 : OCC1<MODE, HRIMG> == 3 ? 6 : SEG1;
// WIN: the pixels are those of win's query rectangle (row-major, hh x ww per item); the tables are read at the
// pixel's row / column of the virtual grid, flow is written at the pixel's index in the rectangle and HRfeat at its
// place in win's F rectangle; the whole-grid instantiations (WIN false) never read win.  WIN and MODE 2: the
// remapped HRfeat row is read from the F layout, its index clamped into F and a clamp reported (bit 2 of *status,
// which no other instantiation touches), as bilin_hr does with bit 1.
// TF: the time-field variant (time_at), MODE 0 / 1 without the HR image only; everything else is the scalar twin's.
// FORM PTS (MODE 0 / 1, no HR image): the pixels are the points of tq, a stif_dec_points, each with its own time;
// HRfeat and flow are stored at the point's running index, the whole-grid layout over the point list; a row /
// column clamped into the grid is reported as bit 3 of *status (pixel_of).
// PTS and MODE 2 (the local ensemble's flow stage at the points, tb a shifted query's): hrfeat is the compact
// [n][npts][64] operand, row [item][pt] the HRfeat of the point's remapped pixel (k_dec_remap and a feat-only pass over
// the remapped list made it), so hr_y / hr_x are not read here.
template <int MODE, bool HRIMG, int F16, int FORM, bool TF = false>
__global__ __launch_bounds__(NW1 * 64) __attribute__((amdgpu_waves_per_eu(OCC1<MODE, HRIMG>))) void k_dec1(const float* __restrict__ proj, const float* __restrict__ mlp,
                                                     stif_dec_tables tb, stif_dec_image im,
                                                     typename TimeArg<TQK<FORM, TF>>::type tq, float* __restrict__ hrfeat,
                                                     float* __restrict__ flow, int n, int h, int w, int HH,
                                                     int WW, stif_dec_window win, int* status) {
  constexpr bool WIN = FORM == WINDOW;
  constexpr int TQ = TQK<FORM, TF>;
  static_assert(!(WIN && MODE == 2 && HRIMG), "the windowed flow-only stage takes no high-resolution image");
  static_assert(!TF || (MODE != 2 && !HRIMG), "a time field has no local-ensemble and no HR-image form");
  static_assert(FORM != PTS || (!HRIMG && !TF), "a point list has no HR-image and no time-field form");
  // two segment buffers of SEG1 tiles + the flow's last layer (plain [4][256], resident)
  constexpr bool OCC3 = S1<MODE, HRIMG> != SEG1;             // 3 or 4 workgroups per CU
  constexpr bool OCC4 = OCC1<MODE, HRIMG> == 4;
  __shared__ __attribute__((aligned(16))) float wbuf[2 * S1<MODE, HRIMG> * T + T];
  const int lane = threadIdx.x & 63, hf = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
  float* const B0 = wbuf;
  float* const B1 = wbuf + S1<MODE, HRIMG> * T;
  float* const W3V = wbuf + 2 * S1<MODE, HRIMG> * T;
  const __amdgpu_buffer_rsrc_t rm = mlp_rsrc(mlp);
  if (MODE != 1) dma_tiles<NW1>(W3V, rm, L_W3V, 1, wv, lane);
  // segment 0: feat layer 1 (4 tiles); segments 1..8: feat layer 2 tile kt + layer 3 (0, kt), (1, kt)
  if (MODE != 2) dma_tiles<NW1>(B0, rm, F_W1, 4, wv, lane);
  else {   // flow only: flow layers 0 / 1 straight into B1
    dma_tiles<NW1>(B1, rm, L_W0, 4, wv, lane);
    dma_tiles<NW1>(B1 + 4 * T, rm, L_W1, 4, wv, lane);
  }
  const Pixel pix = pixel_of<NW1, 32, FORM>(wv, lane, n, HH, WW, win, tq, status);
  const bool valid = pix.valid;
  const long long pc = pix.pc;
  const int item = pix.item;
  // row / column of the virtual grid
  const int py = WIN ? win.y0 + pix.ly : pix.ly, px = WIN ? win.x0 + pix.lx : pix.lx;
  // the scalar kernels load the item's time once; a time-field kernel reads its pixel's time where it is used (feat
  // layer 0, flow layer 0) and does not keep it in a register across the feat stage
  const float t = TF ? 0.f : time_at<TQ>(tq, item, py, px, pix.pt);
  auto time = [&]() {
    if constexpr (TF) return time_at<TQ>(tq, item, py, px);
    else return t;
  };
  const float* P = proj + (size_t)item * h * w * PROJ_C;

  f32x16 hr[2] = {f32x16{0}, f32x16{0}};
  f32x16 x1[2];
  if constexpr (MODE != 2) {
  // ---- feat_imnet layer 0: z = P1[nearest] + w_rel . rel + w_t * t  (bias folded into P1)
  f32x16 x0[2];
  {
    const float ry = tb.rel_y[py], rx = tb.rel_x[px], t = time();
    const float* p1 = P + ((size_t)tb.near_y[py] * w + tb.near_x[px]) * PROJ_C;
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int f = ot * 32 + 8 * v + 4 * hf;
        const f32x4 z = ld4(p1 + f) + ld4(mlp + F_WRY + f) * ry + ld4(mlp + F_WRX + f) * rx + ld4(mlp + F_WT + f) * t;
#pragma unroll
        for (int e = 0; e < 4; ++e) x0[ot][4 * v + e] = siren_sin<F16>(z[e]);
      }
  }
  auto seg_feat23 = [&](float* dst, int kt) {   // W2 rows kt (2 tiles), W3 (0, kt), (1, kt): 16 pieces, as one
    // loop with the same count on every wave (exact vmcnt bookkeeping)
#pragma unroll
    for (int r = 0; r < 16 / NW1; ++r) {
      const int i = wv + r * NW1, j = i >> 2;
      const int src = (j < 2 ? F_W2 + (kt * 2 + j) * T : F_W3 + ((j - 2) * 8 + kt) * T) + (i & 3) * 256;
      dec_dma(rm, dst + j * T + (i & 3) * 256, lane, src * 4);
    }
  };
  lds_dma_barrier();
  const Bias32 fb1[2] = {bias_ld(mlp + F_B1, hf), bias_ld(mlp + F_B1 + 32, hf)};   // before the DMA
  __builtin_amdgcn_sched_barrier(0);
  seg_feat23(B1, 0);
  // ---- layer 1: 64 -> 64
  {
    const XT<F16> xs[2] = {xop<F16>(x0[0]), xop<F16>(x0[1])};
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
      f32x16 acc = f32x16{0};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) tile_mma<F16>(acc, B0 + (ot * 2 + kt) * T, xs[kt], lane);
      x1[ot] = bias_sin<F16>(acc, fb1[ot]);
    }
  }
  // ---- layer 2 (64 -> 256, sine) streamed into layer 3 (256 -> 64, linear)
  const XT<F16> x1s[2] = {xop<F16>(x1[0]), xop<F16>(x1[1])};
  // the streamed steps (kt = 7 peeled: its DMA differs, and the loop's steps must all issue the same
  // number of DMA pieces for the compiler's vmcnt bookkeeping to stay exact across the back edge)
  auto feat_step = [&](int kt, bool last) {
    lds_dma_barrier();
    // this step's bias is loaded before the next segment's DMA is issued, so waiting for it does not
    // wait for the DMA (vmcnt counts in issue order)
    const Bias32 b2 = bias_ld(mlp + F_B2 + kt * 32, hf);
    __builtin_amdgcn_sched_barrier(0);
    float* cur = (kt & 1) ? B0 : B1;
    float* nxt = (kt & 1) ? B1 : B0;
    if (!last) seg_feat23(nxt, kt + 1);
    else {   // prefetch flow layer 0 (4 tiles) + layer 1 (4 tiles; OCC3: its first output tile)
      dma_tiles<NW1>(nxt, rm, L_W0, 4, wv, lane);
      if (!OCC4) dma_tiles<NW1>(nxt + 4 * T, rm, L_W1, OCC3 ? 2 : 4, wv, lane);
    }
    f32x16 acc = f32x16{0};
    tile_mma<F16>(acc, cur, x1s[0], lane);
    tile_mma<F16>(acc, cur + T, x1s[1], lane);
    const XT<F16> h2 = xop<F16>(bias_sin<F16>(acc, b2));
    tile_mma<F16>(hr[0], cur + 2 * T, h2, lane);
    tile_mma<F16>(hr[1], cur + 3 * T, h2, lane);
  };
#pragma unroll 1
  for (int kt = 0; kt < 7; ++kt) feat_step(kt, false);
  feat_step(7, true);
#pragma unroll
  for (int ot = 0; ot < 2; ++ot) hr[ot] = bias_add<F16>(hr[ot], mlp + F_B3 + ot * 32, hf);
  if (valid) {
    float* o = hrfeat + (WIN ? ((size_t)item * win.fh + (py - win.fy0)) * win.fw + (px - win.fx0) : (size_t)pc) * 64;
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        f32x4 s;
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = hr[ot][4 * v + e];
        st4(o + ot * 32 + 8 * v + 4 * hf, s);
      }
  }
  }   // MODE != 2
  if constexpr (MODE == 1) return;
  if constexpr (MODE == 2) {
    // the query's HRfeat operand: the HR pixel nearest to the shifted query (grid_sample nearest
    // of HRfeat at coord_, Sakuya_arch_test.py:1022-1025)
    Bilin b;
    if constexpr (FORM == PTS) {
      b.o00 = b.o01 = b.o10 = b.o11 = pix.pt;
    } else if constexpr (WIN) {
      const int ry = tb.hr_y[py] - win.fy0, rx = tb.hr_x[px] - win.fx0;
      const int y = min(max(ry, 0), win.fh - 1), x = min(max(rx, 0), win.fw - 1);
      if (status != nullptr && (y != ry || x != rx)) atomicOr(status, 4);
      b.o00 = b.o01 = b.o10 = b.o11 = y * win.fw + x;
    } else {
      b.o00 = b.o01 = b.o10 = b.o11 = tb.hr_y[py] * WW + tb.hr_x[px];
    }
    b.w00 = 1.f;
    b.w01 = b.w10 = b.w11 = 0.f;
    if constexpr (FORM == PTS)
      gather64<8>(hr, hrfeat + (size_t)item * tq.npts * 64, 64, 0, b, hf);
    else
      gather64<8>(hr, hrfeat + (size_t)item * (WIN ? (size_t)win.fh * win.fw : (size_t)HH * WW) * 64, 64, 0, b, hf);
  }

  // ---- flow_imnet layer 0: W[:, :64] . HRfeat + bilinear(P2 at the HR centre) + w_t * t + b
  f32x16 z[2];
  {
    const Bilin b = bilin_tab(tb, py, px, w);
    const float t = time();
    // loads in flight sized to the register budget: 8 corner loads (32 VGPRs, four memory latencies) at 128
    // registers, 16 (64 VGPRs, two latencies) at 168, all 32 (128 VGPRs, one latency) at 256
    if (OCC4) gather64<2>(z, P, PROJ_C, 64, b, hf);
    else if (OCC3) gather64<4>(z, P, PROJ_C, 64, b, hf);
    else gather64<8>(z, P, PROJ_C, 64, b, hf);
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int f = ot * 32 + 8 * v + 4 * hf;
        const f32x4 wt = ld4(mlp + L_WT + f), bb = ld4(mlp + L_B0 + f);
#pragma unroll
        for (int e = 0; e < 4; ++e) z[ot][4 * v + e] = (z[ot][4 * v + e] + (wt[e] * t + bb[e])) * ACC_IN<F16>;
      }
    if constexpr (HRIMG) {   // q_inp from the high-resolution image (decoding_test :515-518)
      const Bilin bi = bilin_tab(im, py, px, im.iw);
      img_mma(z, mlp + I_L, img_sample(im.img + (size_t)item * im.ih * im.iw * IMG_C, bi, hf), lane);
    }
  }
  // flow layers 0/1 live in B1 (prefetched during the last feat segment, or at the start)
  lds_dma_barrier();
  const Bias32 lb1[2] = {bias_ld(mlp + L_B1, hf), bias_ld(mlp + L_B1 + 32, hf)};   // before the DMA
  __builtin_amdgcn_sched_barrier(0);
  auto seg_flow23 = [&](float* dst, int kt) {   // W2 rows kt (2 tiles); W3 is resident (W3V)
    dma_tiles<NW1>(dst, rm, L_W2 + kt * 2 * T, 2, wv, lane);
  };
  // OCC3: layer 1's second output tile (2 tiles) into B0, segment 0 after it
  constexpr bool L1B0 = OCC3 && !OCC4 && MODE == 0;
  if (OCC4) dma_tiles<NW1>(B0, rm, L_W1, 4, wv, lane);   // all of layer 1 into B0; segment 0 later
  else {
    if (L1B0) dma_tiles<NW1>(B0, rm, L_W1 + 2 * T, 2, wv, lane);
    seg_flow23(B0 + (L1B0 ? 2 * T : 0), 0);
  }
  {
    const XT<F16> hs[2] = {xop<F16>(hr[0]), xop<F16>(hr[1])};
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) tile_mma<F16>(z[ot], B1 + (ot * 2 + kt) * T, hs[kt], lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) z[ot][r] = siren_sin<F16>(z[ot][r] * ACC_S<F16>);
    }
  }
  if (L1B0 || OCC4) lds_dma_barrier();   // layer 1 (OCC3: its second output tile) landed in B0
  if (OCC4) seg_flow23(B1, 0);             // every wave is done with layer 0's B1
  {
    const XT<F16> zs[2] = {xop<F16>(z[0]), xop<F16>(z[1])};
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
      f32x16 acc = f32x16{0};
      const float* w1t = OCC4 ? B0 + ot * 2 * T : (L1B0 && ot == 1) ? B0 : B1 + (4 + ot * 2) * T;
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) tile_mma<F16>(acc, w1t + kt * T, zs[kt], lane);
      x1[ot] = bias_sin<F16>(acc, lb1[ot]);
    }
  }
  const XT<F16> x1f[2] = {xop<F16>(x1[0]), xop<F16>(x1[1])};
  float fl[4] = {0.f, 0.f, 0.f, 0.f};
  auto flow_step = [&](int kt, bool last) {   // kt = 7 peeled (see feat_step)
    lds_dma_barrier();
    const Bias32 b2 = bias_ld(mlp + L_B2 + kt * 32, hf);   // before the DMA (see feat_step)
    __builtin_amdgcn_sched_barrier(0);
    // OCC4: segment 0 sits in B1, so the buffers alternate the other way round
    float* cur = OCC4 ? ((kt & 1) ? B0 : B1) : (kt & 1) ? B1 : (L1B0 && kt == 0 ? B0 + 2 * T : B0);
    float* nxt = OCC4 ? ((kt & 1) ? B1 : B0) : (kt & 1) ? B0 : B1;
    if (!last) seg_flow23(nxt, kt + 1);
    f32x16 acc = f32x16{0};
    tile_mma<F16>(acc, cur, x1f[0], lane);
    tile_mma<F16>(acc, cur + T, x1f[1], lane);
    const f32x16 h2 = bias_sin<F16>(acc, b2);
    narrow_dot<4>(fl, W3V, kt, h2, hf);   // flow_imnet.net.3 (256 -> 4, linear)
  };
#pragma unroll 1
  for (int kt = 0; kt < 7; ++kt) flow_step(kt, false);
  flow_step(7, true);
#pragma unroll
  for (int c = 0; c < 4; ++c) fl[c] += __shfl_xor(fl[c], 32);   // the other lane half's 128 features
  if (valid && hf == 0) {
    const f32x4 bb = ld4(mlp + L_B3);
    f32x4 s;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = fl[e] + bb[e];
    st4(flow + (size_t)pc * 4, s);
  }
}

// WIN: the pixels are those of win's query rectangle, flow is read at the
// pixel's index in the rectangle, the linspace base at its row / column of the virtual grid, HRfeat in win's F
// rectangle (bilin_hr) and the RGB goes through win's output addressing.
// FORM PTS: the pixels are the points of tq (flow at the point's index, the linspace base at its clamped row /
// column, its own time), hrfeat holds the points' corner rows [n][npts][8][64] (bilin_hr) and the RGB goes to
// out[item][c][point] -- BLEND: blended into it with the weight at the point's clamped row / column (store_rgb).
template <bool HRIMG, int F16, int FORM, bool BLEND = false, bool TF = false>   // TF: as k_dec1's
__global__ __launch_bounds__(DEC2_NW * 64) __attribute__((amdgpu_waves_per_eu(DEC2_WPE))) void k_dec2(const float* __restrict__ proj, const float* __restrict__ mlp,
                                                     const float* __restrict__ hrfeat, const float* __restrict__ flow,
                                                     stif_dec_tables tb, stif_dec_image im,
                                                     typename TimeArg<TQK<FORM, TF>>::type tq, float* __restrict__ out, int n,
                                                     int h, int w, int HH, int WW, int* status, stif_dec_window win,
                                                     stif_dec_blend bl) {
  constexpr bool WIN = FORM == WINDOW;
  constexpr int TQ = TQK<FORM, TF>;
  static_assert(!TF || (!HRIMG && !BLEND), "a time field has no HR-image and no blending form");
  static_assert(FORM != PTS || (!HRIMG && !TF), "a point list has no HR-image and no time-field form");
  __shared__ __attribute__((aligned(16))) float wbuf[2 * SEG * T];
  const int lane = threadIdx.x & 63, hf = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform
  float* const B0 = wbuf;
  float* const B1 = wbuf + SEG * T;
  const __amdgpu_buffer_rsrc_t rm = mlp_rsrc(mlp);
  // segments: [L0: 8 tiles] [L1: 4] then per layer-2 tile kt: [W2 rows kt (2) + W3 column kt (8)],
  // then [W4: 8]
  dma_tiles<DEC2_NW>(B0, rm, E_W0, 8, wv, lane);
  const Pixel pix = pixel_of<DEC2_NW, 32, FORM>(wv, lane, n, HH, WW, win, tq, status);
  const long long pc = pix.pc;
  const int item = pix.item, py = pix.ly, px = pix.lx;   // row / column in the rectangle
  const float t = time_at<TQ>(tq, item, WIN ? win.y0 + py : py, WIN ? win.x0 + px : px, pix.pt);
  const float* P = proj + (size_t)item * h * w * PROJ_C;
  const float* HRF = hrfeat + (WIN ? (size_t)item * win.fh * win.fw * 64 : (size_t)item * HH * WW * 64);
  if constexpr (FORM == PTS) HRF = hrfeat + (size_t)item * tq.npts * 8 * 64;   // eight corner rows per point

  // warpgrid and the decoder's clamp (warp_grids)
  const f32x4 fv = ld4(flow + (size_t)pc * 4);
  const float bx = tb.lin_x[WIN ? win.x0 + px : px], by = tb.lin_y[WIN ? win.y0 + py : py];
  const WarpGrids wg = warp_grids(fv, bx, by, WW, HH);

  // ---- encode_imnet layer 0: W[:, :128] . [q_feat1 | q_feat2] + P3(grid1) + P4(grid2) + w_t t + b
  f32x16 x0[2];
  {
    // four 64-channel bilinear gathers (32 x 16-B loads per lane each), consumed one at a time so
    // at most two 64-wide register tiles are live (2 waves/SIMD fit in 256 VGPRs); the compiler
    // barriers keep it from hoisting the next gather's loads over the current one
    f32x16 z[2], q[2];
    gather64<8>(z, P, PROJ_C, 128, bilin(wg.g1x, wg.g1y, w, h), hf);
    asm volatile("" ::: "memory");
    gather64<8>(q, P, PROJ_C, 192, bilin(wg.g2x, wg.g2y, w, h), hf);
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int f = ot * 32 + 8 * v + 4 * hf;
        const f32x4 wt = ld4(mlp + E_WT + f), bb = ld4(mlp + E_B0 + f);
#pragma unroll
        for (int e = 0; e < 4; ++e) z[ot][4 * v + e] = (z[ot][4 * v + e] + (q[ot][4 * v + e] + wt[e] * t + bb[e])) * ACC_IN<F16>;
      }
    if constexpr (HRIMG) {   // q_img1 / q_img2 from the high-resolution image (decoding_test :558-583)
      const float* I = im.img + (size_t)item * im.ih * im.iw * IMG_C;
      img_mma(z, mlp + I_E1, img_sample(I, bilin(wg.g1x, wg.g1y, im.iw, im.ih), hf), lane);
      img_mma(z, mlp + I_E2, img_sample(I, bilin(wg.g2x, wg.g2y, im.iw, im.ih), hf), lane);
    }
    asm volatile("" ::: "memory");
    gather64<8>(q, HRF, 64, 0, bilin_hr<FORM>(wg.g1x, wg.g1y, WW, HH, win, status, 8 * pix.pt), hf);   // q_feat1 -> W0 columns 0..63
    lds_dma_barrier();
    dma_tiles<DEC2_NW>(B1, rm, E_W1, 4, wv, lane);
    {
      const XT<F16> qs[2] = {xop<F16>(q[0]), xop<F16>(q[1])};
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) tile_mma<F16>(z[ot], B0 + (ot * 4 + kt) * T, qs[kt], lane);
    }
    asm volatile("" ::: "memory");
    gather64<8>(q, HRF, 64, 0, bilin_hr<FORM>(wg.g2x, wg.g2y, WW, HH, win, status, 8 * pix.pt + 4), hf);   // q_feat2 -> W0 columns 64..127
    const XT<F16> qs[2] = {xop<F16>(q[0]), xop<F16>(q[1])};
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
#pragma unroll
      for (int kt = 2; kt < 4; ++kt) tile_mma<F16>(z[ot], B0 + (ot * 4 + kt) * T, qs[kt - 2], lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) x0[ot][r] = siren_sin<F16>(z[ot][r] * ACC_S<F16>);
    }
  }
  lds_dma_barrier();
  const Bias32 eb1[2] = {bias_ld(mlp + E_B1, hf), bias_ld(mlp + E_B1 + 32, hf)};   // before the DMA
  __builtin_amdgcn_sched_barrier(0);
  // layer 2 (64 -> 256, sine) is streamed tile by tile into the 8 accumulators of layer 3 (256 -> 256):
  // segment kt = W2 rows of tile kt (2 tiles) + column kt of W3 (8 tiles)
  auto seg_l23 = [&](float* dst, int kt) {
    dma_tiles<DEC2_NW>(dst, rm, E_W2 + kt * 2 * T, 2, wv, lane);
#pragma unroll
    for (int ot = 0; ot < 8; ++ot) dma_tiles<DEC2_NW>(dst + (2 + ot) * T, rm, E_W3 + (ot * 8 + kt) * T, 1, wv, lane);
  };
  seg_l23(B0, 0);
  f32x16 x1[2];
  {
    const XT<F16> xs[2] = {xop<F16>(x0[0]), xop<F16>(x0[1])};
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
      f32x16 acc = f32x16{0};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) tile_mma<F16>(acc, B1 + (ot * 2 + kt) * T, xs[kt], lane);
      x1[ot] = bias_sin<F16>(acc, eb1[ot]);
    }
  }
  const XT<F16> x1s[2] = {xop<F16>(x1[0]), xop<F16>(x1[1])};
  f32x16 a3[8];   // layer 3's accumulators, fed by the streamed layer-2 tiles (seg_l23)
#pragma unroll
  for (int ot = 0; ot < 8; ++ot) a3[ot] = f32x16{0};
  auto l23_step = [&](int kt, bool last) {   // kt = 7 peeled (see k_dec1's feat_step)
    lds_dma_barrier();
    const Bias32 b2 = bias_ld(mlp + E_B2 + kt * 32, hf);   // before the DMA (see k_dec1)
    __builtin_amdgcn_sched_barrier(0);
    float* cur = (kt & 1) ? B1 : B0;
    float* nxt = (kt & 1) ? B0 : B1;
    if (!last) seg_l23(nxt, kt + 1);
    else dma_tiles<DEC2_NW>(nxt, rm, E_W4V, 1, wv, lane);
    f32x16 acc = f32x16{0};
    tile_mma<F16>(acc, cur, x1s[0], lane);
    tile_mma<F16>(acc, cur + T, x1s[1], lane);
    const XT<F16> h2 = xop<F16>(bias_sin<F16>(acc, b2));
#pragma unroll
    for (int ot = 0; ot < 8; ++ot) tile_mma<F16>(a3[ot], cur + (2 + ot) * T, h2, lane);
  };
#pragma unroll 1
  for (int kt = 0; kt < 7; ++kt) l23_step(kt, false);
  l23_step(7, true);
  // layer 3 sine streamed into layer 4 (256 -> 3, linear, VALU dot products); W4 sits in B0 as
  // plain rows, followed by the layer-3 biases (E_W4V_B3; kt = 7 prefetch)
  lds_dma_barrier();
  float o4[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    const f32x16 h3 = bias_sin<F16>(a3[kt], B0 + (E_W4V_B3 - E_W4V) + kt * 32, hf);
    narrow_dot<3>(o4, B0, kt, h3, hf);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) o4[c] += __shfl_xor(o4[c], 32);   // the other lane half's 128 features
  if (pix.valid && hf == 0) {
    if constexpr (FORM == PTS)
      store_rgb<PTS, F16 != 0, BLEND>(out, mlp, o4, fv, item, 0, pix.pt, 1, tq.npts, win, status, bl, pix.ly, pix.lx);
    else store_rgb<FORM, F16 != 0, BLEND>(out, mlp, o4, fv, item, py, px, HH, WW, win, status, bl);
  }
}


// ---------------------------------------------------------------------------------------------
// k_dec2q: stage 2 (split-fp16, LR-projection image inputs) at 16 pixels per wave on
// v_mfma_f32_16x16x32_f16.  Lane l = (p = l & 15: the wave's pixel, q = l >> 4).  A 32-feature register
// tile is two 16x16 accumulators: lane (p, q) holds features 16 s + 4 q + i (s = 0, 1; i = 0..3) of pixel
// p -- which is also the B-operand order of the next layer's K (dec_layout.h Q_*), so features stay in
// registers between layers as in k_dec2.  The layer-3 state halves (8 tiles x 8 floats = 64 VGPRs): 128 VGPRs,
// four waves per SIMD.
// Weight streaming (round 6): every workgroup streams the whole 372-KB weight set through its LDS, so the
// stream is paid once per workgroup; its memory traffic costs ~10 % of the kernel (profiles/r06_dec_probe3.log).
// Workgroups are 8 waves (128 pixels, two per CU; one 16-wave workgroup per CU streaming two layer-2 tiles per
// segment measured 27 % slower, profiles/r06_dec_ab.log) and a segment is the layer-2 / -3 weights of one layer-2
// tile kt (W2 rows kt + W3 column kt: 10 tiles), double-buffered in 2 x 40 KB: one barrier per kt.  Every wave
// issues the same number of LDS-DMA pieces per segment (5), so the compiler's vmcnt bookkeeping stays exact.
// Gathers: each lane fetches its own quarter of a 64-channel block (16 corner loads in flight).
constexpr int DEC2Q_NW = 8;   // waves per workgroup
constexpr int SEGQ = 10;      // tiles per segment
static_assert(SEGQ * 4 % DEC2Q_NW == 0, "k_dec2q: every wave issues the same number of LDS-DMA pieces");
static_assert(2 * SEGQ * T * 4 * 2 <= 160 * 1024, "k_dec2q: two workgroups per CU, their LDS within 160 KB");
struct R32 {
  f32x4 s[2];
};
struct XQ {
  f16x8 h, l;
};
STIF_DEV XQ xq(const R32& x) {
  XQ o;
  split_f16x3(x.s[0], x.s[1], o.h, o.l);
  return o;
}
STIF_DEV void tile_q(R32& acc, const float* t, const XQ& x, int lane) {
  const float* b = t + lane * 4;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const f16x8 ah = ldh8(b + (2 * s) * 256), al = ldh8(b + (2 * s + 1) * 256);
    acc.s[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, x.h, acc.s[s], 0, 0, 0);
    acc.s[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, x.h, acc.s[s], 0, 0, 0);
    acc.s[s] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, x.l, acc.s[s], 0, 0, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}
// this lane's biases of a register tile whose features start at b (they carry omega_0 / 2 pi, pack.cpp)
STIF_DEV R32 bias_q(const float* __restrict__ b, int q) {
  R32 o;
#pragma unroll
  for (int s = 0; s < 2; ++s) o.s[s] = ld4(b + 16 * s + 4 * q);
  return o;
}
// sin(z * 2^-14 + b) of a register tile, biases preloaded (bias_q)
STIF_DEV R32 bias_sin_q(const R32& z, const R32& bb) {
  R32 o;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int e = 0; e < 4; ++e) o.s[s][e] = siren_sin<1>(fmaf(z.s[s][e], ACC_S<1>, bb.s[s][e]));
  return o;
}
STIF_DEV R32 bias_sin_q(const R32& z, const float* __restrict__ b, int q) { return bias_sin_q(z, bias_q(b, q)); }
// bilinear sample of this lane's channels c0 + 32 ot + 16 s + 4 q .. + 3 (ot, s = 0, 1) of an NHWC map
STIF_DEV void gather_q(R32* dst, const float* __restrict__ base, int stride, int c0, const Bilin& b, int q) {
  const int c = c0 + 4 * q;
  const float* p00 = base + (size_t)b.o00 * stride + c;
  const float* p01 = base + (size_t)b.o01 * stride + c;
  const float* p10 = base + (size_t)b.o10 * stride + c;
  const float* p11 = base + (size_t)b.o11 * stride + c;
  f32x4 cr[4][4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {   // g = 2 ot + s: channel offset 16 g
    cr[g][0] = ld4(p00 + 16 * g);
    cr[g][1] = ld4(p01 + 16 * g);
    cr[g][2] = ld4(p10 + 16 * g);
    cr[g][3] = ld4(p11 + 16 * g);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    f32x4 v = b.w00 * cr[g][0] + b.w01 * cr[g][1] + b.w10 * cr[g][2] + b.w11 * cr[g][3];
    asm volatile("" : "+v"(v));
    dst[g >> 1].s[g & 1] = v;
  }
}

template <int FORM, bool BLEND = false, bool TF = false>   // FORM, BLEND, TF: as k_dec2's
__global__ __launch_bounds__(DEC2Q_NW * 64) __attribute__((amdgpu_waves_per_eu(4))) void k_dec2q(
    const float* __restrict__ proj, const float* __restrict__ mlp, const float* __restrict__ hrfeat,
    const float* __restrict__ flow, stif_dec_tables tb, typename TimeArg<TQK<FORM, TF>>::type tq,
    float* __restrict__ out, int n, int h, int w, int HH, int WW, int* status, stif_dec_window win, stif_dec_blend bl) {
  constexpr bool WIN = FORM == WINDOW;
  constexpr int TQ = TQK<FORM, TF>;
  static_assert(!TF || !BLEND, "a time field has no blending form");
  static_assert(FORM != PTS || !TF, "a point list has no time-field form");
  __shared__ __attribute__((aligned(16))) float wbuf[2 * SEGQ * T];
  const int lane = threadIdx.x & 63, q = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr int NW = DEC2Q_NW;
  float* const B0 = wbuf;
  float* const B1 = wbuf + SEGQ * T;
  const __amdgpu_buffer_rsrc_t rm = mlp_rsrc(mlp);
  // segments: [L0: 8 tiles] in B0, [L1: 4 tiles] in B1, then per layer-2 tile kt [W2 rows kt (2) | W3 column kt,
  // ot 0-7 (8)] alternating B0 / B1, then [W4 rows + B3]
  dma_tiles<NW>(B0, rm, Q_W0, 8, wv, lane);   // tile index 4 ot + kt
  auto seg_l23 = [&](float* dst, int kt) {
#pragma unroll
    for (int r = 0; r < SEGQ * 4 / NW; ++r) {
      const int i = wv + r * NW;                // piece i: tile j = i / 4 of the segment, quarter i % 4
      const int j = i >> 2;
      const int src = (j < 2 ? Q_W2 + (kt * 2 + j) * T : Q_W3 + ((j - 2) * 8 + kt) * T) + (i & 3) * 256;
      dec_dma(rm, dst + j * T + (i & 3) * 256, lane, src * 4);
    }
  };
  const Pixel pix = pixel_of<NW, 16, FORM>(wv, lane, n, HH, WW, win, tq, status);
  const long long pc = pix.pc;
  const int item = pix.item, py = pix.ly, px = pix.lx;   // row / column in the rectangle
  const float t = time_at<TQ>(tq, item, WIN ? win.y0 + py : py, WIN ? win.x0 + px : px, pix.pt);
  const float* P = proj + (size_t)item * h * w * PROJ_C;
  const float* HRF = hrfeat + (WIN ? (size_t)item * win.fh * win.fw * 64 : (size_t)item * HH * WW * 64);
  if constexpr (FORM == PTS) HRF = hrfeat + (size_t)item * tq.npts * 8 * 64;   // eight corner rows per point

  // warpgrid (warplayer.py:25-39) and the decoder's clamp (Sakuya_arch_test.py:428,441), as k_dec2
  const f32x4 fv = ld4(flow + (size_t)pc * 4);
  const float bx = tb.lin_x[WIN ? win.x0 + px : px], by = tb.lin_y[WIN ? win.y0 + py : py];
  const WarpGrids wg = warp_grids(fv, bx, by, WW, HH);

  // ---- encode_imnet layer 0: W[:, :128] . [q_feat1 | q_feat2] + P3(grid1) + P4(grid2) + w_t t + b
  R32 x0[2];
  {
    R32 z[2], g[2];
    gather_q(z, P, PROJ_C, 128, bilin(wg.g1x, wg.g1y, w, h), q);
    asm volatile("" ::: "memory");
    gather_q(g, P, PROJ_C, 192, bilin(wg.g2x, wg.g2y, w, h), q);
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int f = 32 * ot + 16 * s + 4 * q;
        const f32x4 wt = ld4(mlp + E_WT + f), bb = ld4(mlp + E_B0 + f);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          z[ot].s[s][e] = (z[ot].s[s][e] + (g[ot].s[s][e] + wt[e] * t + bb[e])) * ACC_IN<1>;
      }
    asm volatile("" ::: "memory");
    gather_q(g, HRF, 64, 0, bilin_hr<FORM>(wg.g1x, wg.g1y, WW, HH, win, status, 8 * pix.pt), q);   // q_feat1 -> W0 columns 0..63
    lds_dma_barrier();                                      // layer 0 landed in B0
    dma_tiles<NW>(B1, rm, Q_W1, 4, wv, lane);
    {
      const XQ qs[2] = {xq(g[0]), xq(g[1])};
#pragma unroll
      for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) tile_q(z[ot], B0 + (ot * 4 + kt) * T, qs[kt], lane);
    }
    asm volatile("" ::: "memory");
    gather_q(g, HRF, 64, 0, bilin_hr<FORM>(wg.g2x, wg.g2y, WW, HH, win, status, 8 * pix.pt + 4), q);   // q_feat2 -> W0 columns 64..127
    const XQ qs[2] = {xq(g[0]), xq(g[1])};
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
#pragma unroll
      for (int kt = 2; kt < 4; ++kt) tile_q(z[ot], B0 + (ot * 4 + kt) * T, qs[kt - 2], lane);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int e = 0; e < 4; ++e) x0[ot].s[s][e] = siren_sin<1>(z[ot].s[s][e] * ACC_S<1>);
    }
  }
  lds_dma_barrier();   // layer 1 landed in B1; every wave is done with layer 0's B0
  // layer-1 biases before the next segment's LDS-DMA: vmcnt counts in issue order, so a bias load issued
  // after the DMA would wait for the DMA too (as k_dec1 / k_dec2 do)
  const R32 eb1[2] = {bias_q(mlp + E_B1, q), bias_q(mlp + E_B1 + 32, q)};
  __builtin_amdgcn_sched_barrier(0);
  seg_l23(B0, 0);
  R32 x1[2];
  {
    const XQ xs[2] = {xq(x0[0]), xq(x0[1])};
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
      R32 acc;
      acc.s[0] = acc.s[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) tile_q(acc, B1 + (ot * 2 + kt) * T, xs[kt], lane);
      x1[ot] = bias_sin_q(acc, eb1[ot]);
    }
  }
  const XQ x1s[2] = {xq(x1[0]), xq(x1[1])};
  // layer 2 (64 -> 256, sine) streamed tile by tile into the 8 register tiles of layer 3 (256 -> 256)
  R32 a3[8];
#pragma unroll
  for (int ot = 0; ot < 8; ++ot) a3[ot].s[0] = a3[ot].s[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto l23_step = [&](int kt, bool last) {   // kt = 7 peeled (see k_dec1's feat_step)
    lds_dma_barrier();   // segment kt landed; every wave is done with the other buffer
    const R32 b2 = bias_q(mlp + E_B2 + kt * 32, q);   // before the DMA
    __builtin_amdgcn_sched_barrier(0);
    float* cur = (kt & 1) ? B1 : B0;
    float* nxt = (kt & 1) ? B0 : B1;
    if (!last) seg_l23(nxt, kt + 1);
    else dma_tiles<NW>(nxt, rm, E_W4V, 1, wv, lane);
    R32 acc;
    acc.s[0] = acc.s[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    tile_q(acc, cur, x1s[0], lane);
    tile_q(acc, cur + T, x1s[1], lane);
    const XQ h2 = xq(bias_sin_q(acc, b2));
#pragma unroll
    for (int ot = 0; ot < 8; ++ot) tile_q(a3[ot], cur + (2 + ot) * T, h2, lane);
  };
#pragma unroll 1
  for (int kt = 0; kt < 7; ++kt) l23_step(kt, false);
  l23_step(7, true);
  // layer 3 sine streamed into layer 4 (256 -> 3, VALU dot products over this lane's 64 features); W4 rows
  // and the layer-3 biases in B0, the buffer the last segment did not use (k_dec2's tile)
  lds_dma_barrier();
  float o4[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int kt = 0; kt < 8; ++kt) {
    const R32 h3 = bias_sin_q(a3[kt], B0 + (E_W4V_B3 - E_W4V) + kt * 32, q);
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const f32x4 wr = ld4(B0 + c * 256 + kt * 32 + 16 * s + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[c] = fmaf(wr[e], h3.s[s][e], o4[c]);
      }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {   // the other three lane groups' features
    o4[c] += __shfl_xor(o4[c], 16);
    o4[c] += __shfl_xor(o4[c], 32);
  }
  if (pix.valid && q == 0) {
    if constexpr (FORM == PTS)
      store_rgb<PTS, true, BLEND>(out, mlp, o4, fv, item, 0, pix.pt, 1, tq.npts, win, status, bl, pix.ly, pix.lx);
    else store_rgb<FORM, true, BLEND>(out, mlp, o4, fv, item, py, px, HH, WW, win, status, bl);
  }
}

// k_dec_bounds: the box (rows ymin..ymax, columns xmin..xmax of the virtual grid, inclusive) of every HRfeat corner
// stage 2 reads for win's query rectangle given its flow -- warp_grids + bilin_corners, the expressions of stage 2
// itself on the same operands, so the box is exact; corners of weight 0 count (stage 2 loads them).  One box for
// all n items: each lane folds its pixels, the wave reduces across lanes, lane 0 issues one atomic per bound.
__global__ void k_dec_bounds_init(int* __restrict__ box) {
  if (threadIdx.x < 4) box[threadIdx.x] = (threadIdx.x & 1) ? INT_MIN : INT_MAX;
}
__global__ __launch_bounds__(256) void k_dec_bounds(const float* __restrict__ flow, stif_dec_tables tb,
                                                    int* __restrict__ box, long long total, int HH, int WW,
                                                    stif_dec_window win) {
  int ymin = INT_MAX, ymax = INT_MIN, xmin = INT_MAX, xmax = INT_MIN;
  const int plane = win.hh * win.ww;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
    const int rem = (int)(p % plane);
    const int py = rem / win.ww, px = rem - py * win.ww;
    const WarpGrids g = warp_grids(ld4(flow + (size_t)p * 4), tb.lin_x[win.x0 + px], tb.lin_y[win.y0 + py], WW, HH);
    const Corners a = bilin_corners(g.g1x, g.g1y, WW, HH), b = bilin_corners(g.g2x, g.g2y, WW, HH);
    ymin = min(ymin, min(min(a.cy0, a.cy1), min(b.cy0, b.cy1)));
    ymax = max(ymax, max(max(a.cy0, a.cy1), max(b.cy0, b.cy1)));
    xmin = min(xmin, min(min(a.cx0, a.cx1), min(b.cx0, b.cx1)));
    xmax = max(xmax, max(max(a.cx0, a.cx1), max(b.cx0, b.cx1)));
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    ymin = min(ymin, __shfl_xor(ymin, m));
    ymax = max(ymax, __shfl_xor(ymax, m));
    xmin = min(xmin, __shfl_xor(xmin, m));
    xmax = max(xmax, __shfl_xor(xmax, m));
  }
  if ((threadIdx.x & 63) == 0 && ymin <= ymax) {   // a wave that saw no pixel has nothing to add
    atomicMin(box + 0, ymin);
    atomicMax(box + 1, ymax);
    atomicMin(box + 2, xmin);
    atomicMax(box + 3, xmax);
  }
}

// k_dec_corners: k_dec_bounds' sibling for point lists.  Per point, from its stage-1 flow: the eight HRfeat corner
// pixels stage 2 gathers -- warp_grids + bilin_corners on stage 2's operands -- written as a point list of 8 npts
// entries per item, slots 8 p + 0..3 the corners 00, 01, 10, 11 (row digit first) of grid 1 and 8 p + 4..7 those
// of grid 2, each with the point's time: a feat-only stage 1 over that list gives the [npts][8][64] rows bilin_hr's
// point form addresses.  Corners of weight 0 are written too (stage 2 loads them).
__global__ __launch_bounds__(256) void k_dec_corners(const float* __restrict__ flow, stif_dec_tables tb,
                                                     stif_dec_points pts, int* __restrict__ cy, int* __restrict__ cx,
                                                     float* __restrict__ ct, long long total, int HH, int WW,
                                                     int* status) {
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
    const int item = (int)(p / pts.npts), pt = (int)(p - (long long)item * pts.npts);
    int y, x;
    point_yx(pts, item, pt, HH, WW, status, y, x);
    const float t = time_at<2>(pts, item, y, x, pt);
    const WarpGrids g = warp_grids(ld4(flow + (size_t)p * 4), tb.lin_x[x], tb.lin_y[y], WW, HH);
    const Corners c[2] = {bilin_corners(g.g1x, g.g1y, WW, HH), bilin_corners(g.g2x, g.g2y, WW, HH)};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const Corners& a = c[k >> 2];
      cy[p * 8 + k] = (k & 2) ? a.cy1 : a.cy0;
      cx[p * 8 + k] = (k & 1) ? a.cx1 : a.cx0;
      ct[p * 8 + k] = t;
    }
  }
}

// k_dec_remap: the HR pixel whose HRfeat row the flow stage of a shifted query reads for every point (grid_sample
// nearest of HRfeat at the shifted coordinate: tb.hr_y / hr_x at the point's clamped row / column), as the row /
// column lists of the feat-only pass that computes those rows.  The tables hold indices of the grid, so the lists need
// no clamp of their own.
__global__ __launch_bounds__(256) void k_dec_remap(stif_dec_tables tb, stif_dec_points pts, int* __restrict__ ry,
                                                   int* __restrict__ rx, long long total, int HH, int WW,
                                                   int* status) {
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long long)gridDim.x * 256) {
    const int item = (int)(p / pts.npts), pt = (int)(p - (long long)item * pts.npts);
    int y, x;
    point_yx(pts, item, pt, HH, WW, status, y, x);
    ry[p] = tb.hr_y[y];
    rx[p] = tb.hr_x[x];
  }
}

__global__ __launch_bounds__(256) void k_pack_lr(const float* __restrict__ f0, const float* __restrict__ f1,
                                                 const float* __restrict__ f2, const float* __restrict__ x,
                                                 float* __restrict__ out, int n, int h, int w) {
  const long long npix = (long long)n * h * w;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < npix * 50; e += (long long)gridDim.x * 256) {
    const long long pix = e / 50;
    const int q = (int)(e - pix * 50);
    f32x4 v;
    if (q < 48) {
      const float* src = q < 16 ? f0 : (q < 32 ? f1 : f2);
      v = ld4(src + pix * 64 + (q & 15) * 4);
    } else {
      const int item = (int)(pix / ((long long)h * w));
      const long long yx = pix - (long long)item * h * w;
      const float* xi = x + (size_t)item * 6 * h * w + yx;   // [2][3][h][w] of this item
      const size_t pl = (size_t)h * w;
      if (q == 48) { v[0] = xi[0]; v[1] = xi[pl]; v[2] = xi[2 * pl]; v[3] = xi[3 * pl]; }
      else { v[0] = xi[4 * pl]; v[1] = xi[5 * pl]; v[2] = 0.f; v[3] = 0.f; }
    }
    st4(out + pix * SRC_C + q * 4, v);
  }
}

__global__ __launch_bounds__(256) void k_blend4(const float* __restrict__ p0, const float* __restrict__ p1,
                                                const float* __restrict__ p2, const float* __restrict__ p3,
                                                const float* __restrict__ w0, const float* __restrict__ w1,
                                                const float* __restrict__ w2, const float* __restrict__ w3,
                                                float* __restrict__ out, long long total, int plane) {
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int q = (int)(e % plane);
    float r = p0[e] * w0[q];   // ret = 0 + pred_0 * w_0 + ... in the reference's order (:1082-1084)
    r += p1[e] * w1[q];
    r += p2[e] * w2[q];
    r += p3[e] * w3[q];
    out[e] = r;
  }
}

bool tables_ok(const stif_dec_tables* t) {
  return t && t->near_y && t->rel_y && t->by0 && t->by1 && t->wy0 && t->wy1 && t->lin_y && t->near_x &&
         t->rel_x && t->bx0 && t->bx1 && t->wx0 && t->wx1 && t->lin_x;
}

}  // namespace

extern "C" int stif_dec_pack_lr(const float* f0, const float* f1, const float* f2, const float* x, float* out,
                                int n, int h, int w, void* stream) {
  if (!f0 || !f1 || !f2 || !x || !out || n < 1 || h < 1 || w < 1)
    return stif_fail(STIF_E_INVALID, "stif_dec_pack_lr: bad arguments");
  const long long work = (long long)n * h * w * 50;
  long long blocks = (work + 255) / 256;
  if (blocks > 1 << 16) blocks = 1 << 16;
  hipLaunchKernelGGL(k_pack_lr, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, f0, f1, f2, x, out, n, h,
                     w);
  return stif_check_launch("stif_dec_pack_lr");
}

namespace {

bool image_ok(const stif_dec_image* im) {
  return !im || (im->img && im->ih > 0 && im->iw > 0 && im->by0 && im->by1 && im->wy0 && im->wy1 && im->bx0 &&
                 im->bx1 && im->wx0 && im->wx1);
}

// ---- windowed decoding
bool rect_in(int y0, int x0, int hh, int ww, int HH, int WW) {
  return y0 >= 0 && x0 >= 0 && hh >= 1 && ww >= 1 && hh <= HH - y0 && ww <= WW - x0;
}

// the window with its defaults filled in (F = the query rectangle, dense output), or the reason it is invalid
const char* window_resolve(const stif_dec_window* in, int HH, int WW, stif_dec_window* o) {
  if (!in) return "null window";
  if (HH < 1 || WW < 1 || (long long)HH * WW > INT_MAX) return "bad virtual grid size";
  *o = *in;
  if (!rect_in(o->y0, o->x0, o->hh, o->ww, HH, WW)) return "the query rectangle is not inside the HH x WW grid";
  if (!o->fy0 && !o->fx0 && !o->fh && !o->fw) {
    o->fy0 = o->y0; o->fx0 = o->x0; o->fh = o->hh; o->fw = o->ww;
  }
  if (!rect_in(o->fy0, o->fx0, o->fh, o->fw, HH, WW)) return "the F rectangle is not inside the HH x WW grid";
  if (!o->out_item && !o->out_plane && !o->out_pitch) {
    o->out_pitch = o->ww;
    o->out_plane = (long long)o->hh * o->ww;
    o->out_item = 3 * o->out_plane;
  }
  if (o->out_pitch < o->ww) return "out_pitch < ww";
  if (o->out_plane < 1 || o->out_item < 1) return "out_item / out_plane must be positive";
  return nullptr;
}

bool f_holds_query(const stif_dec_window& wn) {
  return wn.fy0 <= wn.y0 && wn.fx0 <= wn.x0 && wn.y0 + wn.hh <= wn.fy0 + wn.fh && wn.x0 + wn.ww <= wn.fx0 + wn.fw;
}

int window_fail(const char* entry, const char* why) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", entry, why);
  return stif_fail(STIF_E_INVALID, msg);
}

template <int M>
using Mode = std::integral_constant<int, M>;

// the reason a stif_dec_blend is invalid, or null
const char* blend_invalid(const stif_dec_blend* b) {
  if (!b) return "null blend";
  if (b->k < 0 || b->k > 3) return "blend k outside 0..3";
  if (b->accumulate != 0 && b->accumulate != 1) return "blend accumulate must be 0 or 1";
  for (int j = 0; j < 4; ++j)
    if (!b->rel_y[j] || !b->rel_x[j]) return "blend with a null rel_y / rel_x table";
  return nullptr;
}

// the reason a time-field call is invalid before its generic argument check, or null
const char* time_field_invalid(const stif_dec_tables* tab, const stif_dec_image* img, const stif_dec_time* t) {
  if (img) return "a high-resolution image (img) has no time-field form: pass NULL";
  if (tab && (tab->hr_y || tab->hr_x)) return "tables with hr_y / hr_x (local ensemble) have no time-field form";
  if (!t || !t->t) return "null time field (t)";
  if (t->item < 0 || t->row < 0 || t->col < 0) return "negative time-field stride";
  return nullptr;
}

// the reason a point call is invalid after its generic argument check, or null
// shifted: the entry point takes the tables of a shifted query (the local ensemble's point stages)
const char* points_invalid(const stif_dec_tables* tab, const stif_dec_points* p, int n, int HH, int WW,
                           bool shifted = false) {
  if (!p || !p->y || !p->x || !p->t) return "null point list (pts or its y, x or t)";
  if (p->npts < 1) return "npts < 1";
  if (p->y_item < 0 || p->x_item < 0 || p->t_item < 0 || p->t_point < 0) return "negative point stride";
  if (n >= 1 && (long long)n * 8 * p->npts > INT_MAX) return "n * 8 * npts exceeds INT_MAX";
  if (!shifted && tab && (tab->hr_y || tab->hr_x))
    return "tables with hr_y / hr_x (local ensemble) have no point form";
  if (HH < 2 || WW < 2 || (long long)HH * WW > INT_MAX) return "bad virtual grid size";
  return nullptr;
}

// ---- One launcher per stage.  An entry point states its query -- whose pixels, which kind of time, which variant
// of the stage -- and dec_stage1 / dec_stage2 check it, resolve it and launch it.
struct TimeQ {   // the kernels' time argument, by kind (TimeArg): [n] times, a time field, or a point list
  int kind;
  const float* t = nullptr;
  const stif_dec_time* field = nullptr;
  const stif_dec_points* pts = nullptr;
  TimeQ(const float* v) : kind(0), t(v) {}
  TimeQ(const stif_dec_time* v) : kind(1), field(v) {}
  TimeQ(const stif_dec_points* v) : kind(2), pts(v) {}
};
template <int K>
auto time_arg(const TimeQ& q) {   // what the kernel takes by value; the checks have seen the pointer
  if constexpr (K == 2) return *q.pts;
  else if constexpr (K == 1) return *q.field;
  else return q.t;
}

struct Query {
  const char* me;                        // the entry point: the prefix of its messages
  TimeQ time;
  bool windowed = false;                 // the pixels are win's query rectangle (a point list is never windowed)
  const stif_dec_window* win = nullptr;
  bool flow_only = false;                // stage 1: the flow-only stage of a shifted query (MODE 2 over F / the points)
  bool blending = false;                 // stage 2: the local ensemble's epilogue, as `blend` says
  const stif_dec_blend* blend = nullptr;
  int form() const { return time.kind == 2 ? PTS : windowed ? WINDOW : GRID; }
  bool tf() const { return time.kind == 1; }
  // the two whole-grid scalar stages reject everything with one text, "<entry>: bad arguments"
  bool plain() const { return form() == GRID && !tf(); }
};

// The pixels of q: the window resolved into *wn (zeroes otherwise, which no kernel reads) and their number, or the
// reason they are invalid.  The plain stages' grid size is part of their one argument check.
const char* pixels_of(const Query& q, const stif_dec_tables* tab, int n, int HH, int WW, stif_dec_window* wn,
                      long long* total) {
  *wn = stif_dec_window{};
  if (q.form() == PTS) {
    if (const char* why = points_invalid(tab, q.time.pts, n, HH, WW, q.flow_only || q.blending)) return why;
    *total = (long long)n * q.time.pts->npts;
  } else if (q.form() == WINDOW) {
    if (const char* why = window_resolve(q.win, HH, WW, wn)) return why;
    *total = (long long)n * wn->hh * wn->ww;
  } else {
    if (q.tf() && (HH < 2 || WW < 2 || (long long)HH * WW > INT_MAX)) return "bad virtual grid size";
    *total = (long long)n * HH * WW;
  }
  return nullptr;
}

// The instantiations the entry points can reach; the rest the kernels' static_asserts refuse, or nothing asks for.
constexpr bool variant_exists(int form, bool blend, bool tf) {
  return !(tf && form == PTS) && (!blend || (form != GRID && !tf));
}
constexpr bool dec1_exists(int mode, bool hrimg, int form, bool tf) {
  if (form == PTS) return !tf && !hrimg;   // MODE 2: the local ensemble's flow stage over the compact operand
  if (tf) return mode != 2 && !hrimg;
  // the whole grid's feat-only pass is the first half of the remapped stage, which takes the image in its second
  return form == WINDOW ? !(mode == 2 && hrimg) : !(mode == 1 && hrimg);
}
constexpr bool dec2_exists(bool hrimg, bool f16, int form, bool blend, bool tf) {
  // f16x3 operands without an HR image are k_dec2q's
  return variant_exists(form, blend, tf) && (hrimg || !f16) && !(hrimg && (blend || tf || form == PTS));
}

// Stage 1.  A null flow is the feat-only pass (MODE 1), which the plain and the flow-only stage do not have.
// flow_only: flow_imnet over the query rectangle, its HRfeat operand the row of HR pixel (hr_y, hr_x) in the F
// layout; F need not hold the query rectangle, only the remap rectangle -- which the kernel enforces (clamp + bit 2
// of *status), since the tables live on the device.  flow_only over a point list: the operand of point p is row
// [item][p] of the compact hrfeat; the shifted tables are required as for the window and their remap is not read.
int dec_stage1(const Query& q, const float* proj, const float* mlp, const stif_dec_tables* tab,
               const stif_dec_image* img, float* hrfeat, float* flow, int n, int h, int w, int HH, int WW, int flags,
               int* status, void* stream) {
  const int form = q.form();
  if (q.tf())
    if (const char* why = time_field_invalid(tab, img, q.time.field)) return window_fail(q.me, why);
  bool ok = proj && mlp && tables_ok(tab) && (q.flow_only || image_ok(img)) && (q.time.kind || q.time.t) && hrfeat &&
            n >= 1 && h >= 1 && w >= 1;
  if (q.plain() || q.flow_only) ok = ok && flow;
  if (q.plain()) ok = ok && HH >= 2 && WW >= 2 && (!tab->hr_y) == (!tab->hr_x);
  if (!ok) return window_fail(q.me, q.plain() ? "bad arguments" : "bad arguments (null pointer or empty shape)");
  if (q.flow_only) {
    if (img) return window_fail(q.me, "a high-resolution image (img) is not supported here: pass NULL");
    if (!tab->hr_y || !tab->hr_x) return window_fail(q.me, "the tables carry no hr_y / hr_x remap (local ensemble)");
  } else if (form == WINDOW && (tab->hr_y || tab->hr_x)) {
    return window_fail(q.me, "tables with hr_y / hr_x (local ensemble) have no windowed form");
  }
  stif_dec_window wn;
  long long total;
  if (const char* why = pixels_of(q, tab, n, HH, WW, &wn, &total)) return window_fail(q.me, why);
  // every pixel of the query rectangle stores its HRfeat row into the F layout
  if (form == WINDOW && !q.flow_only && !f_holds_query(wn))
    return window_fail(q.me, "the F rectangle does not contain the query rectangle");
  const dim3 grid((unsigned)((total + NW1 * 32 - 1) / (NW1 * 32)));
  const stif_dec_image im = img ? *img : stif_dec_image{};
  auto launch = [&](auto mode, auto hrimg) {
    with_bool(flags & STIF_CONV_F16X3, [&](auto f16x3) {
      with_int<GRID, WINDOW, PTS>(form, [&](auto fm) {
        with_bool(q.tf(), [&](auto field) {
          constexpr int M = decltype(mode)::value, FM = decltype(fm)::value;
          constexpr bool H = decltype(hrimg)::value, TF = decltype(field)::value;
          if constexpr (dec1_exists(M, H, FM, TF))
            hipLaunchKernelGGL((k_dec1<M, H, decltype(f16x3)::value, FM, TF>), grid, dim3(NW1 * 64), 0,
                               (hipStream_t)stream, proj, mlp, *tab, im, time_arg<TQK<FM, TF>>(q.time), hrfeat, flow,
                               n, h, w, HH, WW, wn, status);
        });
      });
    });
  };
  if (q.flow_only) {   // MODE 2 only reads hrfeat
    launch(Mode<2>{}, std::false_type{});
  } else if (q.plain() && tab->hr_y) {   // remapped HRfeat operand: the whole HRfeat map first, then the flow stage
    launch(Mode<1>{}, std::false_type{});
    with_bool(img != nullptr, [&](auto hrimg) { launch(Mode<2>{}, hrimg); });
  } else {
    with_bool(img != nullptr, [&](auto hrimg) {
      if (!flow) launch(Mode<1>{}, hrimg);
      else launch(Mode<0>{}, hrimg);
    });
  }
  return stif_check_launch(q.me);
}

// Stage 2.  f16x3 operands without an HR image go to k_dec2q (16 pixels per wave, four waves per SIMD: C2 stage 2
// 17.55-17.79 -> 17.32-17.34 ms, profiles/r04_dec2q4_ab.log); the fp32 and the HR-image stages to k_dec2.
int dec_stage2(const Query& q, const float* proj, const float* mlp, const float* hrfeat, const float* flow,
               const stif_dec_tables* tab, const stif_dec_image* img, float* out, int n, int h, int w, int HH, int WW,
               int flags, int* status, void* stream) {
  if (q.blending) {
    if (const char* why = blend_invalid(q.blend)) return window_fail(q.me, why);
    if (img) return window_fail(q.me, "a high-resolution image (img) is not supported here: pass NULL");
  }
  if (q.tf())
    if (const char* why = time_field_invalid(tab, img, q.time.field)) return window_fail(q.me, why);
  bool ok = proj && mlp && hrfeat && flow && tables_ok(tab) && image_ok(img) && (q.time.kind || q.time.t) && out &&
            n >= 1 && h >= 1 && w >= 1;
  if (q.plain()) ok = ok && HH >= 2 && WW >= 2;
  if (!ok) return window_fail(q.me, q.plain() ? "bad arguments" : "bad arguments (null pointer or empty shape)");
  stif_dec_window wn;
  long long total;
  if (const char* why = pixels_of(q, tab, n, HH, WW, &wn, &total)) return window_fail(q.me, why);
  const bool f16 = flags & STIF_CONV_F16X3;
  auto grid = [&](int wg_pixels) { return dim3((unsigned)((total + wg_pixels - 1) / wg_pixels)); };
  hipStream_t st = (hipStream_t)stream;
  const stif_dec_image im = img ? *img : stif_dec_image{};
  const stif_dec_blend bl = q.blending ? *q.blend : stif_dec_blend{};
  with_int<GRID, WINDOW, PTS>(q.form(), [&](auto fm) {
    with_bool(q.tf(), [&](auto field) {
      with_bool(q.blending, [&](auto blend) {
        constexpr int FM = decltype(fm)::value;
        constexpr bool TF = decltype(field)::value, B = decltype(blend)::value;
        if (f16 && !img) {
          if constexpr (variant_exists(FM, B, TF))
            hipLaunchKernelGGL((k_dec2q<FM, B, TF>), grid(DEC2Q_NW * 16), dim3(DEC2Q_NW * 64), 0, st, proj, mlp, hrfeat,
                               flow, *tab, time_arg<TQK<FM, TF>>(q.time), out, n, h, w, HH, WW, status, wn, bl);
          return;
        }
        with_bool(img != nullptr, [&](auto hrimg) {
          with_bool(f16, [&](auto f16x3) {
            constexpr bool H = decltype(hrimg)::value, F = decltype(f16x3)::value;
            if constexpr (dec2_exists(H, F, FM, B, TF))
              hipLaunchKernelGGL((k_dec2<H, F, FM, B, TF>), grid(DEC2_NW * 32), dim3(DEC2_NW * 64), 0, st, proj, mlp,
                                 hrfeat, flow, *tab, im, time_arg<TQK<FM, TF>>(q.time), out, n, h, w, HH, WW, status,
                                 wn, bl);
          });
        });
      });
    });
  });
  return stif_check_launch(q.me);
}

}  // namespace

// ---- the stage entry points: each states its query and calls its stage's launcher
// status: stage 2 checks both stage-1 outputs it reads (flow, and HRfeat through the RGB; stif.h), so stage 1 has
// nothing to report outside the flow-only and the point form
extern "C" int stif_dec_stage1_ex(const float* proj, const float* mlp, const stif_dec_tables* tab,
                                  const stif_dec_image* img, const float* t, float* hrfeat, float* flow, int n, int h,
                                  int w, int HH, int WW, int flags, int* /*status*/, void* stream) {
  return dec_stage1({"stif_dec_stage1", t}, proj, mlp, tab, img, hrfeat, flow, n, h, w, HH, WW, flags, nullptr, stream);
}

extern "C" int stif_dec_stage1(const float* proj, const float* mlp, const stif_dec_tables* tab,
                               const stif_dec_image* img, const float* t, float* hrfeat, float* flow, int n, int h,
                               int w, int HH, int WW, void* stream) {
  return stif_dec_stage1_ex(proj, mlp, tab, img, t, hrfeat, flow, n, h, w, HH, WW, 0, nullptr, stream);
}

extern "C" int stif_dec_stage1_win(const float* proj, const float* mlp, const stif_dec_tables* tab,
                                   const stif_dec_image* img, const float* t, float* hrfeat, float* flow, int n, int h,
                                   int w, int HH, int WW, int flags, int* /*status*/, void* stream,
                                   const stif_dec_window* win) {
  return dec_stage1({"stif_dec_stage1_win", t, true, win}, proj, mlp, tab, img, hrfeat, flow, n, h, w, HH, WW, flags,
                    nullptr, stream);
}

extern "C" int stif_dec_flow_win(const float* proj, const float* mlp, const stif_dec_tables* tab,
                                 const stif_dec_image* img, const float* t, const float* hrfeat, float* flow, int n,
                                 int h, int w, int HH, int WW, int flags, int* status, void* stream,
                                 const stif_dec_window* win) {
  return dec_stage1({"stif_dec_flow_win", t, true, win, true}, proj, mlp, tab, img, const_cast<float*>(hrfeat), flow,
                    n, h, w, HH, WW, flags, status, stream);
}

extern "C" int stif_dec_stage1_tf(const float* proj, const float* mlp, const stif_dec_tables* tab,
                                  const stif_dec_image* img, const stif_dec_time* t, float* hrfeat, float* flow, int n,
                                  int h, int w, int HH, int WW, int flags, int* /*status*/, void* stream,
                                  const stif_dec_window* win) {
  return dec_stage1({"stif_dec_stage1_tf", t, win != nullptr, win}, proj, mlp, tab, img, hrfeat, flow, n, h, w, HH, WW,
                    flags, nullptr, stream);
}

extern "C" int stif_dec_stage1_pts(const float* proj, const float* mlp, const stif_dec_tables* tab,
                                   const stif_dec_points* pts, float* hrfeat, float* flow, int n, int h, int w, int HH,
                                   int WW, int flags, int* status, void* stream) {
  return dec_stage1({"stif_dec_stage1_pts", pts}, proj, mlp, tab, nullptr, hrfeat, flow, n, h, w, HH, WW, flags,
                    status, stream);
}

extern "C" int stif_dec_stage2_ex(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                                  const stif_dec_tables* tab, const stif_dec_image* img, const float* t, float* out,
                                  int n, int h, int w, int HH, int WW, int flags, int* status, void* stream) {
  return dec_stage2({"stif_dec_stage2", t}, proj, mlp, hrfeat, flow, tab, img, out, n, h, w, HH, WW, flags, status,
                    stream);
}

extern "C" int stif_dec_stage2(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                               const stif_dec_tables* tab, const stif_dec_image* img, const float* t, float* out, int n,
                               int h, int w, int HH, int WW, void* stream) {
  return stif_dec_stage2_ex(proj, mlp, hrfeat, flow, tab, img, t, out, n, h, w, HH, WW, 0, nullptr, stream);
}

extern "C" int stif_dec_stage2_win(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                                   const stif_dec_tables* tab, const stif_dec_image* img, const float* t, float* out,
                                   int n, int h, int w, int HH, int WW, int flags, int* status, void* stream,
                                   const stif_dec_window* win) {
  return dec_stage2({"stif_dec_stage2_win", t, true, win}, proj, mlp, hrfeat, flow, tab, img, out, n, h, w, HH, WW,
                    flags, status, stream);
}

extern "C" int stif_dec_stage2_blend_win(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                                         const stif_dec_tables* tab, const stif_dec_image* img, const float* t,
                                         float* out, int n, int h, int w, int HH, int WW, int flags, int* status,
                                         void* stream, const stif_dec_blend* blend, const stif_dec_window* win) {
  return dec_stage2({"stif_dec_stage2_blend_win", t, true, win, false, true, blend}, proj, mlp, hrfeat, flow, tab, img,
                    out, n, h, w, HH, WW, flags, status, stream);
}

extern "C" int stif_dec_stage2_tf(const float* proj, const float* mlp, const float* hrfeat, const float* flow,
                                  const stif_dec_tables* tab, const stif_dec_image* img, const stif_dec_time* t,
                                  float* out, int n, int h, int w, int HH, int WW, int flags, int* status, void* stream,
                                  const stif_dec_window* win) {
  return dec_stage2({"stif_dec_stage2_tf", t, win != nullptr, win}, proj, mlp, hrfeat, flow, tab, img, out, n, h, w,
                    HH, WW, flags, status, stream);
}

extern "C" int stif_dec_stage2_pts(const float* proj, const float* mlp, const float* hrfeat8, const float* flow,
                                   const stif_dec_tables* tab, const stif_dec_points* pts, float* out, int n, int h,
                                   int w, int HH, int WW, int flags, int* status, void* stream) {
  return dec_stage2({"stif_dec_stage2_pts", pts}, proj, mlp, hrfeat8, flow, tab, nullptr, out, n, h, w, HH, WW, flags,
                    status, stream);
}

extern "C" int stif_dec_corners_pts(const float* flow, const stif_dec_tables* tab, const stif_dec_points* pts, int* cy,
                                    int* cx, float* ct, int n, int HH, int WW, int* status, void* stream) {
  static const char* const me = "stif_dec_corners_pts";
  if (!flow || !tables_ok(tab) || !cy || !cx || !ct || n < 1)
    return window_fail(me, "bad arguments (null pointer or n < 1)");
  if (const char* why = points_invalid(tab, pts, n, HH, WW)) return window_fail(me, why);
  const long long total = (long long)n * pts->npts;
  const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_dec_corners, dim3(blocks), dim3(256), 0, (hipStream_t)stream, flow, *tab, *pts, cy, cx, ct,
                     total, HH, WW, status);
  return stif_check_launch(me);
}

// ---- the local ensemble at points: remap -> stif_dec_stage1_pts over the remapped list -> flow -> corners and their
// HRfeat (the plain point entry points) -> blending stage 2, per shift
extern "C" int stif_dec_remap_pts(const stif_dec_tables* tab, const stif_dec_points* pts, int* ry, int* rx, int n,
                                  int HH, int WW, int* status, void* stream) {
  static const char* const me = "stif_dec_remap_pts";
  if (!tables_ok(tab) || !ry || !rx || n < 1) return window_fail(me, "bad arguments (null pointer or n < 1)");
  if (!tab->hr_y || !tab->hr_x) return window_fail(me, "the tables carry no hr_y / hr_x remap (local ensemble)");
  if (const char* why = points_invalid(tab, pts, n, HH, WW, true)) return window_fail(me, why);
  const long long total = (long long)n * pts->npts;
  const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(k_dec_remap, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *tab, *pts, ry, rx, total, HH, WW,
                     status);
  return stif_check_launch(me);
}

extern "C" int stif_dec_flow_pts(const float* proj, const float* mlp, const stif_dec_tables* tab,
                                 const stif_dec_points* pts, const float* hrfeat, float* flow, int n, int h, int w,
                                 int HH, int WW, int flags, int* status, void* stream) {
  Query q{"stif_dec_flow_pts", pts};
  q.flow_only = true;
  return dec_stage1(q, proj, mlp, tab, nullptr, const_cast<float*>(hrfeat), flow, n, h, w, HH, WW, flags, status,
                    stream);
}

extern "C" int stif_dec_stage2_blend_pts(const float* proj, const float* mlp, const float* hrfeat8, const float* flow,
                                         const stif_dec_tables* tab, const stif_dec_points* pts, float* out, int n,
                                         int h, int w, int HH, int WW, int flags, int* status, void* stream,
                                         const stif_dec_blend* blend) {
  Query q{"stif_dec_stage2_blend_pts", pts};
  q.blending = true;
  q.blend = blend;
  return dec_stage2(q, proj, mlp, hrfeat8, flow, tab, nullptr, out, n, h, w, HH, WW, flags, status, stream);
}

extern "C" int stif_dec_bounds(const float* flow, const stif_dec_tables* tab, int* box, int n, int HH, int WW,
                               void* stream, const stif_dec_window* win) {
  static const char* const me = "stif_dec_bounds";
  if (!flow || !tables_ok(tab) || !box || n < 1) return window_fail(me, "bad arguments (null pointer or n < 1)");
  stif_dec_window wn;
  if (const char* why = window_resolve(win, HH, WW, &wn)) return window_fail(me, why);
  const long long total = (long long)n * wn.hh * wn.ww;
  const unsigned blocks = (unsigned)std::min<long long>((total + 255) / 256, 4096);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_dec_bounds_init, dim3(1), dim3(64), 0, st, box);
  hipLaunchKernelGGL(k_dec_bounds, dim3(blocks), dim3(256), 0, st, flow, *tab, box, total, HH, WW, wn);
  return stif_check_launch(me);
}

extern "C" int stif_dec_blend4(const float* const* pred, const float* const* wgt, float* out, int n, int HH, int WW,
                               void* stream) {
  if (!pred || !wgt || !out || n < 1 || HH < 1 || WW < 1) return stif_fail(STIF_E_INVALID, "stif_dec_blend4: bad arguments");
  for (int k = 0; k < 4; ++k)
    if (!pred[k] || !wgt[k]) return stif_fail(STIF_E_INVALID, "stif_dec_blend4: null input");
  const long long total = (long long)n * 3 * HH * WW;
  const long long blocks = std::min<long long>((total + 255) / 256, 1 << 16);
  hipLaunchKernelGGL(k_blend4, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pred[0], pred[1], pred[2],
                     pred[3], wgt[0], wgt[1], wgt[2], wgt[3], out, total, HH * WW);
  return stif_check_launch("stif_dec_blend4");
}
