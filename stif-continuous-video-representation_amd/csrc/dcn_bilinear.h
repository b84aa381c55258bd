// The DCNv2 sampling semantics, stated once (device only): dmcn_im2col_bilinear and the (-1, H) x (-1, W)
// gate of modulated_deformable_im2col_gpu_kernel (dcn_v2_im2col_cuda.cu:25-54, 173-176), with the
// reference's names and comparisons.  Every DCN kernel -- the fused NHWC kernels' tile sampler below,
// the drop-in's im2col and the training backward -- takes its corners from here.
#pragma once
#include "stif_common.h"

// a sampling position contributes only inside the open interval (-1, H) x (-1, W)
STIF_DEV bool dcn_gate(float h, float w, int H, int W) { return h > -1.f && w > -1.f && h < (float)H && w < (float)W; }

// The four bilinear corners of position (h, w): 1 = (h_low, w_low), 2 = (h_low, w_low + 1),
// 3 = (h_low + 1, w_low), 4 = (h_low + 1, w_low + 1) with weights hh hw, hh lw, lh hw, lh lw;
// b1()..b4(): the corner lies in the frame (a corner outside it reads as 0).  Functions, so that they are
// evaluated where they are used: the fused kernels need them on their fallback path only.
struct DcnCorners {
  int h_low, w_low, h_high, w_high, H, W;
  float lh, lw, hh, hw;
  STIF_DEV bool b1() const { return h_low >= 0 && w_low >= 0; }
  STIF_DEV bool b2() const { return h_low >= 0 && w_high <= W - 1; }
  STIF_DEV bool b3() const { return h_high <= H - 1 && w_low >= 0; }
  STIF_DEV bool b4() const { return h_high <= H - 1 && w_high <= W - 1; }
};
// FROM_LOW: the fraction as the reference writes it, lh = h - h_low (the scalar NCHW kernels: the integer
// corner converted back, nothing else kept); otherwise lh = h - floor(h) (the fused kernels: one
// conversion fewer per tap in their MFMA loops).  The same number wherever h_low fits an int.
template <bool FROM_LOW = false>
STIF_DEV DcnCorners dcn_corners(float h, float w, int H, int W) {
  DcnCorners c;
  const float fh = floorf(h), fw = floorf(w);
  c.lh = h - (FROM_LOW ? (float)(int)fh : fh);
  c.lw = w - (FROM_LOW ? (float)(int)fw : fw);
  c.hh = 1.f - c.lh;
  c.hw = 1.f - c.lw;
  c.h_low = (int)fh;
  c.w_low = (int)fw;
  c.h_high = c.h_low + 1;
  c.w_high = c.w_low + 1;
  c.H = H;
  c.W = W;
  return c;
}

// Bilinear sample at (h, w) of one lane's channels of an NHWC 64-channel map, from a staged LDS tile
// [row][QUADS channel quads][TP columns][4] of TR x TC pixels whose pixel (0, 0) is frame pixel
// (ty0, tx0) and which is zero outside the frame: a0 = quad q0, and with TWO a1 = quad q0 + 1.  The
// modulation m = `mask` where the sample counts (`valid`: the caller's dcn_gate and whatever else it
// requires, e.g. a pixel inside the map), 0 elsewhere, is folded into the corner weights.  The select
// stands here, behind the tile test, because that is where the fused kernels had it: taken at the call
// sites it reorders their tap loops (fp32 k_dcn 0.4 % slower).
// A valid sample whose corners leave the tile is read from the map itself (`img`,
// channels co .. co + 3 and, with TWO, co + 4 .. co + 7); the ballot keeps that path off waves that
// do not need it.
template <int QUADS, int TWO>
STIF_DEV void dcn_tile_sample(const float* st, int TR, int TC, int TP, int ty0, int tx0, int q0, const float* img,
                              int co, int H, int W, float h, float w, float mask, bool valid, f32x4& a0, f32x4& a1) {
  const DcnCorners c = dcn_corners(h, w, H, W);
  const int r0 = c.h_low - ty0, c0 = c.w_low - tx0;
  const bool in_tile = ((unsigned)r0 < (unsigned)(TR - 1)) & ((unsigned)c0 < (unsigned)(TC - 1));
  const float m = valid ? mask : 0.f;
  const float hm = c.hh * m, lm = c.lh * m;
  const float w1 = hm * c.hw, w2 = hm * c.lw, w3 = lm * c.hw, w4 = lm * c.lw;
  const float* p0 = st + (((in_tile ? r0 : 0) * QUADS + q0) * TP + (in_tile ? c0 : 0)) * 4;
  const float* p1 = p0 + QUADS * TP * 4;   // next row
  a0 = w1 * ld4(p0) + w2 * ld4(p0 + 4) + w3 * ld4(p1) + w4 * ld4(p1 + 4);
  if (TWO) a1 = w1 * ld4(p0 + TP * 4) + w2 * ld4(p0 + TP * 4 + 4) + w3 * ld4(p1 + TP * 4) + w4 * ld4(p1 + TP * 4 + 4);
  const bool fb = valid & !in_tile;
  if (__builtin_amdgcn_ballot_w64(fb)) {
    if (fb) {
      const bool b1 = c.b1(), b2 = c.b2(), b3 = c.b3(), b4 = c.b4();
      const float* q1 = img + ((size_t)c.h_low * W + c.w_low) * 64 + co;
      const float* q2 = img + ((size_t)c.h_low * W + c.w_high) * 64 + co;
      const float* q3 = img + ((size_t)c.h_high * W + c.w_low) * 64 + co;
      const float* q4 = img + ((size_t)c.h_high * W + c.w_high) * 64 + co;
      const f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
      a0 = w1 * (b1 ? ld4(q1) : z) + w2 * (b2 ? ld4(q2) : z) + w3 * (b3 ? ld4(q3) : z) + w4 * (b4 ? ld4(q4) : z);
      if (TWO)
        a1 = w1 * (b1 ? ld4(q1 + 4) : z) + w2 * (b2 ? ld4(q2 + 4) : z) + w3 * (b3 ? ld4(q3 + 4) : z) +
             w4 * (b4 ? ld4(q4 + 4) : z);
    }
  }
}
