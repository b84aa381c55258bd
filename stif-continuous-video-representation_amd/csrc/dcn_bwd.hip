// Backward of the fused modulated deformable conv stif_dcn_nhwc at the STIF shape (64 -> 64, 3x3, stride 1, pad 1,
// 8 deformable groups, NHWC), behind stif_dcn_bwd_nhwc, and the bridge stif_dcn_offmask_nhwc that turns the offset /
// mask conv's 256-channel map into the offmask the forward reads.  The mathematics is
// modulated_deformable_col2im / _col2im_coord (dcn_v2_im2col_cuda.cu:197-327) and dcn_v2_cuda_backward's weight and
// bias gradient (dcn_v2_cuda.cu:308-326), as dcn_v2.hip's drop-in states them; every corner comes from
// dcn_bilinear.h.  No columns buffer exists in either direction:
//   k_dcn_bwd_data  colg[p][c][k] = sum_co w[co][c][k] gout[p][co] on fp32 MFMA, one deformable group at a time, held
//                   in accumulators; the lane that owns (pixel, tap) turns its eight colg values into grad_offset,
//                   grad_mask (stored into g_om, one writer per element) and the g_in scatter (LDS tile, then one
//                   atomic flush per group); instantiated a second time as stif_dcn_bwd_contrib's kernel, which
//                   stores the scatter's terms for the ordered sum of segsum.hip instead
//   k_dcn_bwd_w     k_wgrad<1>'s scheme with the sampled, modulated columns as the B operand: persistent grid,
//                   [tap][co][ci] accumulators kept across tiles, one partial per workgroup, k_wgrad_reduce
// The `_ext` drop-in (NCHW, any geometry) stays dcn_v2.hip.
#include <algorithm>
#include <cstdio>

#include "abi_util.h"
#include "dcn_bilinear.h"
#include "stif.h"
#include "tuning.h"
#include "wgrad_part.h"

namespace {

constexpr int OMC = 216;    // offmask channels per pixel: [group][tap][dy, dx, mask]
constexpr int GOMC = 256;   // pixel pitch of om / g_om: 144 offsets, 72 masks, 40 pad channels

// four channels of gout with the activation's derivative folded in: LeakyReLU(0.1) keeps the sign of its argument,
// so the forward's output decides (g where out > 0, g * 0.1 elsewhere)
STIF_DEV f32x4 ld_gout(const float* gout, const float* out, bool lrelu) {
  f32x4 v = ld4(gout);
  if (lrelu) {
    const f32x4 o = ld4(out);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = o[e] > 0.f ? v[e] : v[e] * 0.1f;
  }
  return v;
}

// ---- data kernel: g_om and g_in ----
//
// A workgroup owns DB_TH rows x 32 columns of output pixels (the forward's tile), wave w row w, lane l pixel l & 31.
// The lane keeps its pixel's gout as the MFMA B operand for the whole kernel (32 registers: lane half h holds couts
// 32 h .. 32 h + 31, so K step s contracts couts s and 32 + s).  Per deformable group the 64 x 72 weight slice
// w[co][8 g .. 8 g + 7][tap] -- contiguous in OIHW -- is copied to LDS and D[(c, k) 96][pixel 32] += A[(c, k)][co]
// B[co][pixel] runs as three M tiles.  Row i of M tile t is channel (i & 3) + 4 ((i >> 3) & 1) of tap
// 4 t + 2 ((i >> 2) & 1) + (i >> 4) (taps past 8 are zero rows), which is chosen so that accumulator register
// c + 8 s of lane half h is channel c of tap 4 t + 2 h + s: each lane ends up with all eight channels of the taps it
// then samples (half 0: taps 0, 1, 4, 5, 8; half 1: taps 2, 3, 6, 7), and no colg value ever leaves its register.
// The g_in scatter goes to an LDS tile of the group's eight channels over the pixel tile grown by 1 + DCN_M pixels
// (ds_add_f32), flushed once per group with global fp32 atomics (neighbouring tiles overlap in the margin); a corner
// that leaves the tile goes to global atomics directly.  Elements that stayed zero are not flushed.
constexpr int DB_TH = 4, DB_TW = 32, DB_M = DCN_M;
constexpr int DB_TR = DB_TH + 2 + 2 * DB_M, DB_TC = DB_TW + 2 + 2 * DB_M, DB_TPX = DB_TR * DB_TC;

// CONTRIB (stif_dcn_bwd_contrib): the same front end, g_om included, but no scatter.  The lane
// stores its tap's contribution sub-row cm[p][g][k][8] = colg * m once, the four corner weights and the four packed
// sort words (key << 32) | e, e = ((p * 8 + g) * 9 + k) * 4 + corner, key = (corner pixel) * 8 + g or the sentinel
// n H W 8 for a corner that does not count; stif_segsum adds them per destination in a fixed order.
typedef long long i64x2 __attribute__((ext_vector_type(2)));
struct DcnContrib {
  float* cm;          // [n H W][8][9][8]
  float* wgt;         // [E]
  long long* words;   // [E]
};
struct DcnScatter {};   // the atomic path: an empty last kernel argument, which moves no other argument

template <class CT>
__global__ __launch_bounds__(64 * DB_TH) void k_dcn_bwd_data(stif_dcn_bwd_args a, int tiles_x, int tiles_per_item,
                                                             CT ct) {
  constexpr bool CONTRIB = std::is_same<CT, DcnContrib>::value;
  __shared__ __attribute__((aligned(16))) float s_w[64 * 72];   // [co][c][tap] of the group
  __shared__ float s_gi[CONTRIB ? 1 : 8 * DB_TPX];              // [c][tile pixel]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l32 = lane & 31, hf = lane >> 5;
  const int H = a.H, W = a.W;
  const int n = blockIdx.x / tiles_per_item, rem = blockIdx.x - n * tiles_per_item;
  const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
  const int oy0 = ty * DB_TH, ox0 = tx * DB_TW;
  const int ty0 = oy0 - 1 - DB_M, tx0 = ox0 - 1 - DB_M;   // tile origin (frame coords)
  const int oy = oy0 + wv, ox = ox0 + l32;
  const bool pix_ok = oy < H && ox < W;
  const size_t pix = (size_t)min(oy, H - 1) * W + min(ox, W - 1);
  const float* in = a.in + (size_t)n * a.in_item;
  const float* om = a.offmask + (size_t)n * a.om_item + pix * OMC;
  float* gin = a.g_in ? a.g_in + (size_t)n * a.gin_item : nullptr;
  float* gom = a.g_om ? a.g_om + (size_t)n * a.gom_item + pix * GOMC : nullptr;
  const bool lrelu = a.epi == STIF_EPI_LRELU;

  float gq[32];   // gout[pixel][32 hf + s]
  {
    const float* gp = a.gout + (size_t)n * a.gout_item + pix * 64 + hf * 32;
    const float* op = lrelu ? a.out + (size_t)n * a.out_item + pix * 64 + hf * 32 : nullptr;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (pix_ok) v = ld_gout(gp + 4 * q, op + 4 * q, lrelu);
#pragma unroll
      for (int e = 0; e < 4; ++e) gq[4 * q + e] = v[e];
    }
  }
  const int row_c = (l32 & 3) + 4 * ((l32 >> 3) & 1), row_tap = 2 * ((l32 >> 2) & 1) + (l32 >> 4);

  for (int g = 0; g < 8; ++g) {
    __syncthreads();   // the previous group's flush and A reads are done
    for (int i = tid; i < 64 * 18; i += 64 * DB_TH) {
      const int co = i / 18, q = i - co * 18;
      st4(s_w + co * 72 + q * 4, ld4(a.w + co * 576 + g * 72 + q * 4));
    }
    if (!CONTRIB && gin)
      for (int i = tid; i < 8 * DB_TPX; i += 64 * DB_TH) s_gi[i] = 0.f;
    __syncthreads();

    // (dy, dx, m) of this lane's taps, in flight while the MFMAs run (the loads below may not move across the
    // atomics on their own)
    float omv[5][3];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int tp = min(4 * (j >> 1) + 2 * hf + (j & 1), 8);
#pragma unroll
      for (int e = 0; e < 3; ++e) omv[j][e] = om[g * 27 + tp * 3 + e];
    }

    f32x16 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
      const int tap = 4 * t + row_tap;
      const bool row = tap < 9;
      const float* ap = s_w + hf * 32 * 72 + row_c * 9 + (row ? tap : 0);
#pragma unroll 8
      for (int s = 0; s < 32; ++s) {
        const float av = ap[s * 72];
        acc[t] = mfma32(row ? av : 0.f, gq[s], acc[t]);
      }
    }

#pragma unroll
    for (int t = 0; t < 3; ++t) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (4 * t + s > 8) continue;   // no lane has a tap there
        const int tap = 4 * t + 2 * hf + s;
        const bool mine = pix_ok && tap < 9;
        const int tp = min(tap, 8), ky = tp / 3, kx = tp - 3 * ky;
        const float* o = omv[2 * t + s];
        const float m = o[2];
        const float h_im = (float)(oy - 1 + ky) + o[0];
        const float w_im = (float)(ox - 1 + kx) + o[1];
        const bool valid = mine && dcn_gate(h_im, w_im, H, W);
        const DcnCorners c = dcn_corners(h_im, w_im, H, W);
        const bool b1 = valid && c.b1(), b2 = valid && c.b2(), b3 = valid && c.b3(), b4 = valid && c.b4();
        float col[8];
#pragma unroll
        for (int ch = 0; ch < 8; ++ch) col[ch] = acc[t][8 * s + ch];
        // the four corners' eight channels, loaded together from addresses clamped into the frame (one round trip
        // per tap); a corner that does not count is dropped by a select, not by its weight
        const int yl = min(max(c.h_low, 0), H - 1), yh = min(max(c.h_high, 0), H - 1);
        const int xl = min(max(c.w_low, 0), W - 1), xh = min(max(c.w_high, 0), W - 1);
        const float* img = in + g * 8;
        const float* q1 = img + ((size_t)yl * W + xl) * 64;
        const float* q2 = img + ((size_t)yl * W + xh) * 64;
        const float* q3 = img + ((size_t)yh * W + xl) * 64;
        const float* q4 = img + ((size_t)yh * W + xh) * 64;
        const f32x4 v1l = ld4(q1), v1h = ld4(q1 + 4), v2l = ld4(q2), v2h = ld4(q2 + 4);
        const f32x4 v3l = ld4(q3), v3h = ld4(q3 + 4), v4l = ld4(q4), v4h = ld4(q4 + 4);
        // d_k = sum_c colg[c] * corner_k[c]: the three gradients are combinations of the four dot products
        auto dot8 = [&](bool b, const f32x4& lo, const f32x4& hi) {
          float d = 0.f;
#pragma unroll
          for (int ch = 0; ch < 4; ++ch) d += col[ch] * lo[ch] + col[4 + ch] * hi[ch];
          return b ? d : 0.f;
        };
        const float d1 = dot8(b1, v1l, v1h), d2 = dot8(b2, v2l, v2h);
        const float d3 = dot8(b3, v3l, v3h), d4 = dot8(b4, v4l, v4h);
        if (gom && mine) {
          const float vh = c.hw * (d3 - d1) + c.lw * (d4 - d2);
          const float vw = c.hh * (d2 - d1) + c.lh * (d4 - d3);
          const float vm = c.hh * (c.hw * d1 + c.lw * d2) + c.lh * (c.hw * d3 + c.lw * d4);
          *reinterpret_cast<float2*>(gom + g * 18 + 2 * tap) = make_float2(vh * m, vw * m);
          gom[144 + g * 9 + tap] = vm * m * (1.f - m);
        }
        if constexpr (CONTRIB) {
          if (mine) {
            const size_t sub = (((size_t)n * H * W + pix) * 8 + g) * 9 + tap;
            const long long D = (long long)a.n * H * W * 8;
            const bool any = b1 || b2 || b3 || b4;
            f32x4 lo, hi;
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) lo[ch] = any ? col[ch] * m : 0.f, hi[ch] = any ? col[4 + ch] * m : 0.f;
            st4(ct.cm + sub * 8, lo);
            st4(ct.cm + sub * 8 + 4, hi);
            st4(ct.wgt + sub * 4, f32x4{b1 ? c.hh * c.hw : 0.f, b2 ? c.hh * c.lw : 0.f, b3 ? c.lh * c.hw : 0.f,
                                        b4 ? c.lh * c.lw : 0.f});
            auto word = [&](bool b, int y, int x, int j) {
              const long long key = b ? (((long long)n * H + y) * W + x) * 8 + g : D;
              return (key << 32) | (long long)(sub * 4 + j);
            };
            i64x2* wd = reinterpret_cast<i64x2*>(ct.words + sub * 4);   // two 16-byte stores
            wd[0] = i64x2{word(b1, c.h_low, c.w_low, 0), word(b2, c.h_low, c.w_high, 1)};
            wd[1] = i64x2{word(b3, c.h_high, c.w_low, 2), word(b4, c.h_high, c.w_high, 3)};
          }
        } else if (gin) {
          auto scatter = [&](bool b, int y, int x, float wt) {
            if (!b) return;
            const int r = y - ty0, cc = x - tx0;
            if ((unsigned)r < (unsigned)DB_TR && (unsigned)cc < (unsigned)DB_TC) {
              float* d = s_gi + r * DB_TC + cc;
#pragma unroll
              for (int ch = 0; ch < 8; ++ch) unsafeAtomicAdd(d + ch * DB_TPX, wt * (col[ch] * m));
            } else {
              float* d = gin + ((size_t)y * W + x) * 64 + g * 8;
#pragma unroll
              for (int ch = 0; ch < 8; ++ch) unsafeAtomicAdd(d + ch, wt * (col[ch] * m));
            }
          };
          scatter(b1, c.h_low, c.w_low, c.hh * c.hw);
          scatter(b2, c.h_low, c.w_high, c.hh * c.lw);
          scatter(b3, c.h_high, c.w_low, c.lh * c.hw);
          scatter(b4, c.h_high, c.w_high, c.lh * c.lw);
        }
      }
    }

    if (!CONTRIB && gin) {
      __syncthreads();
      for (int i = tid; i < 8 * DB_TPX; i += 64 * DB_TH) {
        const int ch = i & 7, p = i >> 3, r = p / DB_TC, cc = p - r * DB_TC;
        const int y = ty0 + r, x = tx0 + cc;
        const float v = s_gi[ch * DB_TPX + p];
        if (v != 0.f && y >= 0 && y < H && x >= 0 && x < W) unsafeAtomicAdd(gin + ((size_t)y * W + x) * 64 + g * 8 + ch, v);
      }
    }
  }

  if (a.g_om) {   // the pad channels 216..255 of the tile's pixels
    float* go = a.g_om + (size_t)n * a.gom_item;
    for (int i = tid; i < DB_TH * DB_TW * 10; i += 64 * DB_TH) {
      const int p = i / 10, q = i - p * 10, y = oy0 + (p >> 5), x = ox0 + (p & 31);
      if (y < H && x < W) st4(go + ((size_t)y * W + x) * GOMC + OMC + q * 4, f32x4{0.f, 0.f, 0.f, 0.f});
    }
  }
}

// ---- weight kernel: g_w and g_b ----
//
// k_wgrad<1> (conv_bwd.hip) with another B operand: the same 2 x 32-pixel tiles, persistent grid, wave -> (cout tile,
// cin tile) assignment, nine accumulators kept across tiles, partial layout and reduction.  Where k_wgrad reads the
// x tile shifted by the tap, this kernel reads cols[pixel][tap][ci] = m * bilinear sample of `in` at the tap's
// position, which the whole workgroup writes to LDS first, DW_PX pixels at a time: one thread per (pixel, group, tap)
// samples the group's eight channels from the map itself (16-B loads at addresses clamped into the frame, issued
// together; the corners of neighbouring taps and pixels share cache lines).
constexpr int DW_TH = 2, DW_TW = 32, DW_PX = 16, DW_WG_PER_CU = 2;

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DW_WG_PER_CU)))
void k_dcn_bwd_w(stif_dcn_bwd_args a, float* __restrict__ ws, int tiles_x, int tiles_per_item, int ntiles) {
  __shared__ __attribute__((aligned(16))) float s_col[DW_PX * 9 * 64];
  __shared__ __attribute__((aligned(16))) float s_gy[DW_TH * DW_TW * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cot = wave >> 1, cit = wave & 1, l32 = lane & 31, hf = lane >> 5;
  const int H = a.H, W = a.W;
  const bool lrelu = a.epi == STIF_EPI_LRELU;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;   // sum of this lane's gout values: cout cot * 32 + l32, pixels of parity hf

  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int n = t / tiles_per_item, rem = t - n * tiles_per_item, ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int y0 = ty * DW_TH, x0 = tx * DW_TW;
    const float* in = a.in + (size_t)n * a.in_item;
    const float* om = a.offmask + (size_t)n * a.om_item;
    const float* gi = a.gout + (size_t)n * a.gout_item;
    const float* oi = lrelu ? a.out + (size_t)n * a.out_item : nullptr;
    __syncthreads();   // the previous tile's reads are done
#pragma unroll
    for (int k = 0; k < DW_TH * DW_TW * 16 / 256; ++k) {
      const int i = tid + k * 256;
      const int c4 = i & 15, p = i >> 4, yy = y0 + (p >> 5), xx = x0 + (p & 31);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (yy < H && xx < W) {
        const size_t e = ((size_t)yy * W + xx) * 64 + c4 * 4;
        v = ld_gout(gi + e, oi + e, lrelu);
      }
      st4(s_gy + p * 64 + c4 * 4, v);
    }
    for (int ch = 0; ch < DW_TH * DW_TW / DW_PX; ++ch) {
      const int p0 = ch * DW_PX;   // first tile pixel of the pass
      if (ch) __syncthreads();     // the previous pass's B reads are done
      for (int task = tid; task < DW_PX * 72; task += 256) {
        const int px = task / 72, gk = task - px * 72, g = gk / 9, tap = gk - g * 9, ky = tap / 3, kx = tap - 3 * ky;
        const int p = p0 + px, yy = y0 + (p >> 5), xx = x0 + (p & 31);
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
        if (yy < H && xx < W) {
          const float* o = om + ((size_t)yy * W + xx) * OMC + gk * 3;
          const float h_im = (float)(yy - 1 + ky) + o[0];
          const float w_im = (float)(xx - 1 + kx) + o[1];
          if (dcn_gate(h_im, w_im, H, W)) {
            const DcnCorners c = dcn_corners(h_im, w_im, H, W);
            const float hm = c.hh * o[2], lm = c.lh * o[2];
            const float* img = in + g * 8;
            const int yl = max(c.h_low, 0), yh = min(c.h_high, H - 1), xl = max(c.w_low, 0), xh = min(c.w_high, W - 1);
            const float* q1 = img + ((size_t)yl * W + xl) * 64;
            const float* q2 = img + ((size_t)yl * W + xh) * 64;
            const float* q3 = img + ((size_t)yh * W + xl) * 64;
            const float* q4 = img + ((size_t)yh * W + xh) * 64;
            // loaded together from addresses clamped into the frame; a corner outside it gets weight 0 by a select
            const f32x4 v1l = ld4(q1), v1h = ld4(q1 + 4), v2l = ld4(q2), v2h = ld4(q2 + 4);
            const f32x4 v3l = ld4(q3), v3h = ld4(q3 + 4), v4l = ld4(q4), v4h = ld4(q4 + 4);
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const float w1 = hm * c.hw, w2 = hm * c.lw, w3 = lm * c.hw, w4 = lm * c.lw;
            const bool b1 = c.b1(), b2 = c.b2(), b3 = c.b3(), b4 = c.b4();
            lo = w1 * (b1 ? v1l : z) + w2 * (b2 ? v2l : z) + w3 * (b3 ? v3l : z) + w4 * (b4 ? v4l : z);
            hi = w1 * (b1 ? v1h : z) + w2 * (b2 ? v2h : z) + w3 * (b3 ? v3h : z) + w4 * (b4 ? v4h : z);
          }
        }
        st4(s_col + (px * 9 + tap) * 64 + g * 8, lo);
        st4(s_col + (px * 9 + tap) * 64 + g * 8 + 4, hi);
      }
      __syncthreads();
      // k step ks: tile pixels p0 + 2 ks + hf
      const float* ap = s_gy + (p0 + hf) * 64 + cot * 32 + l32;
      const float* bp = s_col + hf * 9 * 64 + cit * 32 + l32;
#pragma unroll 2
      for (int ks = 0; ks < DW_PX / 2; ++ks) {
        const float av = ap[2 * ks * 64];
        bsum += av;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc[tap] = mfma32(av, bp[(2 * ks * 9 + tap) * 64], acc[tap]);
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

// ---- om [n][H][W][256] -> offmask [n][H][W][216] ----
//
// One pass: a workgroup reads the 216 live channels of OMK_PX pixels with 16-B loads into LDS (sigmoidf_ on the mask
// logits, which are whole quads 36..53; the 40 pad channels are never read) and stores them permuted with 16-B
// stores.  Offsets pass through LDS untouched: bit copies.
constexpr int OMK_PX = 32, OMK_PITCH = OMC + 1;

__global__ __launch_bounds__(256) void k_dcn_offmask(const float* __restrict__ om, float* __restrict__ offmask,
                                                     long long om_item, long long out_item, int HW,
                                                     int blocks_per_item) {
  __shared__ float t[OMK_PX * OMK_PITCH];
  const int n = blockIdx.x / blocks_per_item, p0 = (blockIdx.x - n * blocks_per_item) * OMK_PX;
  const int npx = min(OMK_PX, HW - p0);
  const float* src = om + (size_t)n * om_item + (size_t)p0 * GOMC;
  float* dst = offmask + (size_t)n * out_item + (size_t)p0 * OMC;
  for (int i = threadIdx.x; i < npx * 54; i += 256) {
    const int px = i / 54, q = i - px * 54;
    f32x4 v = ld4(src + px * GOMC + q * 4);
    if (q >= 36) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = sigmoidf_(v[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) t[px * OMK_PITCH + q * 4 + e] = v[e];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < npx * 54; i += 256) {
    const int px = i / 54, q = i - px * 54;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = q * 4 + e, g = j / 27, r = j - g * 27, k = r / 3, c = r - 3 * k;
      v[e] = t[px * OMK_PITCH + (c < 2 ? g * 18 + 2 * k + c : 144 + g * 9 + k)];
    }
    st4(dst + px * OMC + q * 4, v);
  }
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

int fail_as(const char* fn, const char* why) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  return stif_fail(STIF_E_INVALID, msg);
}

long long tiles_of(int n, int H, int W, int th, int tw) {
  return (long long)n * ((H + th - 1) / th) * ((W + tw - 1) / tw);
}

}  // namespace

// the workgroups of the weight kernel write the partials k_wgrad<1>'s do, over the same tiles with the same grid
extern "C" size_t stif_dcn_bwd_workspace_size(int n, int H, int W) {
  return stif_conv3x3_wgrad_workspace_size(n, H, W, 64, 64);
}

extern "C" int stif_dcn_bwd_nhwc(const stif_dcn_bwd_args* pa, void* stream) {
  const char* fn = "stif_dcn_bwd_nhwc";
  if (!pa) return fail_as(fn, "null args");
  const stif_dcn_bwd_args& a = *pa;
  if (!a.in || !a.offmask || !a.w || !a.gout) return fail_as(fn, "null pointer (in, offmask, w, gout)");
  if (a.epi != STIF_EPI_NONE && a.epi != STIF_EPI_LRELU) return fail_as(fn, "epilogue must be NONE or LRELU");
  const bool lrelu = a.epi == STIF_EPI_LRELU;
  if (lrelu && !a.out) return fail_as(fn, "null pointer (out with STIF_EPI_LRELU)");
  if (!a.g_in && !a.g_om && !a.g_w) return fail_as(fn, "nothing to compute (g_in, g_om and g_w are all null)");
  if (a.g_b && !a.g_w) return fail_as(fn, "g_b without g_w");
  if (a.n < 1 || a.H < 1 || a.W < 1) return fail_as(fn, "n, H, W must be >= 1");
  if (a.in_item < 0 || a.om_item < 0 || a.gout_item < 0 || (lrelu && a.out_item < 0) || (a.g_in && a.gin_item < 0) ||
      (a.g_om && a.gom_item < 0))
    return fail_as(fn, "negative item stride");
  if ((long long)a.H * a.W * GOMC * 4 >= 0x7fffffffLL) return fail_as(fn, "item larger than 2 GB (buffer addressing)");
  if (misaligned16(a.in) || misaligned16(a.offmask) || misaligned16(a.w) || misaligned16(a.gout) ||
      (lrelu && misaligned16(a.out)) || misaligned16(a.g_in) || misaligned16(a.g_om) || a.in_item % 4 ||
      a.om_item % 4 || a.gout_item % 4 || (lrelu && a.out_item % 4) || (a.g_in && a.gin_item % 4) ||
      (a.g_om && a.gom_item % 4))
    return fail_as(fn, "maps, w and the item strides must be 16-byte aligned");
  const long long px = (long long)a.H * a.W;
  if (a.n > 1 && ((a.g_in && a.gin_item < px * 64) || (a.g_om && a.gom_item < px * GOMC)))
    return fail_as(fn, "g_in / g_om items overlap (gin_item < H * W * 64 or gom_item < H * W * 256)");
  const long long dtiles = tiles_of(a.n, a.H, a.W, DB_TH, DB_TW), wtiles = tiles_of(a.n, a.H, a.W, DW_TH, DW_TW);
  if (wtiles > 0x7fffffffLL) return fail_as(fn, "too many tiles");
  const int G = (int)std::min<long long>(wtiles, (long long)(stif_dcn_bwd_workspace_size(a.n, a.H, a.W) /
                                                             (PART * sizeof(float))));
  if (a.g_w) {
    if (G < 1 || !a.workspace || a.workspace_bytes < (size_t)G * PART * sizeof(float))
      return fail_as(fn, "workspace too small (stif_dcn_bwd_workspace_size)");
    if (misaligned16(a.workspace)) return fail_as(fn, "workspace not 16-byte aligned");
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.g_in) {   // the scatter adds into zeros, whatever the buffer held
    const size_t row = (size_t)px * 64 * sizeof(float);
    const hipError_t e = (a.n == 1 || a.gin_item == px * 64)
                             ? hipMemsetAsync(a.g_in, 0, row * a.n, st)
                             : hipMemset2DAsync(a.g_in, (size_t)a.gin_item * sizeof(float), 0, row, a.n, st);
    if (e != hipSuccess) return stif_fail(STIF_E_LAUNCH, "stif_dcn_bwd_nhwc: memset of g_in failed");
  }
  if (a.g_in || a.g_om) {
    const int tiles_x = (a.W + DB_TW - 1) / DB_TW, tiles_per_item = tiles_x * ((a.H + DB_TH - 1) / DB_TH);
    hipLaunchKernelGGL(k_dcn_bwd_data<DcnScatter>, dim3((unsigned)dtiles), dim3(64 * DB_TH), 0, st, a, tiles_x,
                       tiles_per_item, DcnScatter{});
    if (int rc = stif_check_launch("stif_dcn_bwd_nhwc (data)")) return rc;
  }
  if (a.g_w) {
    const int tiles_x = (a.W + DW_TW - 1) / DW_TW, tiles_per_item = tiles_x * ((a.H + DW_TH - 1) / DW_TH);
    float* ws = static_cast<float*>(a.workspace);
    hipLaunchKernelGGL(k_dcn_bwd_w, dim3(G), dim3(256), 0, st, a, ws, tiles_x, tiles_per_item, (int)wtiles);
    if (int rc = stif_check_launch("stif_dcn_bwd_nhwc (weight)")) return rc;
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((PART + 255) / 256), dim3(256), 0, st, ws, G, a.g_w, a.g_b, 1, 64);
    return stif_check_launch("stif_dcn_bwd_nhwc (reduce)");
  }
  return STIF_OK;
}

extern "C" int stif_dcn_bwd_contrib(const stif_dcn_bwd_contrib_args* pa, void* stream) {
  const char* fn = "stif_dcn_bwd_contrib";
  if (!pa) return fail_as(fn, "null args");
  const stif_dcn_bwd_contrib_args& c = *pa;
  if (!c.in || !c.offmask || !c.w || !c.gout) return fail_as(fn, "null pointer (in, offmask, w, gout)");
  if (!c.cm || !c.wgt || !c.words) return fail_as(fn, "null pointer (cm, wgt, words)");
  if (c.epi != STIF_EPI_NONE && c.epi != STIF_EPI_LRELU) return fail_as(fn, "epilogue must be NONE or LRELU");
  const bool lrelu = c.epi == STIF_EPI_LRELU;
  if (lrelu && !c.out) return fail_as(fn, "null pointer (out with STIF_EPI_LRELU)");
  if (c.n < 1 || c.H < 1 || c.W < 1) return fail_as(fn, "n, H, W must be >= 1");
  if (c.in_item < 0 || c.om_item < 0 || c.gout_item < 0 || (lrelu && c.out_item < 0) || (c.g_om && c.gom_item < 0))
    return fail_as(fn, "negative item stride");
  if ((long long)c.H * c.W * GOMC * 4 >= 0x7fffffffLL) return fail_as(fn, "item larger than 2 GB (buffer addressing)");
  const long long px = (long long)c.H * c.W;
  if (px * c.n > 0x7fffffffLL / 288) return fail_as(fn, "E = n * H * W * 288 must be < 2^31 (call it on fewer items)");
  if (misaligned16(c.in) || misaligned16(c.offmask) || misaligned16(c.w) || misaligned16(c.gout) ||
      (lrelu && misaligned16(c.out)) || misaligned16(c.g_om) || misaligned16(c.cm) || misaligned16(c.wgt) ||
      misaligned16(c.words) || c.in_item % 4 || c.om_item % 4 || c.gout_item % 4 || (lrelu && c.out_item % 4) ||
      (c.g_om && c.gom_item % 4))
    return fail_as(fn, "maps, w, cm, wgt, words and the item strides must be 16-byte aligned");
  if (c.n > 1 && c.g_om && c.gom_item < px * GOMC) return fail_as(fn, "g_om items overlap (gom_item < H * W * 256)");
  stif_dcn_bwd_args a = {};
  a.in = c.in, a.offmask = c.offmask, a.w = c.w, a.gout = c.gout, a.out = c.out, a.g_om = c.g_om;
  a.in_item = c.in_item, a.om_item = c.om_item, a.gout_item = c.gout_item, a.out_item = c.out_item;
  a.gom_item = c.gom_item, a.n = c.n, a.H = c.H, a.W = c.W, a.epi = c.epi;
  const long long dtiles = tiles_of(c.n, c.H, c.W, DB_TH, DB_TW);
  const int tiles_x = (c.W + DB_TW - 1) / DB_TW, tiles_per_item = tiles_x * ((c.H + DB_TH - 1) / DB_TH);
  hipLaunchKernelGGL(k_dcn_bwd_data<DcnContrib>, dim3((unsigned)dtiles), dim3(64 * DB_TH), 0,
                     static_cast<hipStream_t>(stream), a, tiles_x, tiles_per_item, DcnContrib{c.cm, c.wgt, c.words});
  return stif_check_launch(fn);
}

extern "C" int stif_dcn_offmask_nhwc(const float* om, float* offmask, long long om_item, long long offmask_item, int n,
                                     int H, int W, void* stream) {
  const char* fn = "stif_dcn_offmask_nhwc";
  if (!om || !offmask) return fail_as(fn, "null pointer (om, offmask)");
  if (n < 1 || H < 1 || W < 1) return fail_as(fn, "n, H, W must be >= 1");
  if (om_item < 0 || offmask_item < 0) return fail_as(fn, "negative item stride");
  if ((long long)H * W * GOMC * 4 >= 0x7fffffffLL) return fail_as(fn, "item larger than 2 GB (buffer addressing)");
  if (misaligned16(om) || misaligned16(offmask) || om_item % 4 || offmask_item % 4)
    return fail_as(fn, "om / offmask and their item strides must be 16-byte aligned");
  if (n > 1 && offmask_item < (long long)H * W * OMC) return fail_as(fn, "offmask items overlap (offmask_item < H * W * 216)");
  const int HW = H * W, blocks_per_item = (HW + OMK_PX - 1) / OMK_PX;
  if ((long long)blocks_per_item * n > 0x7fffffffLL) return fail_as(fn, "too many tiles");
  hipLaunchKernelGGL(k_dcn_offmask, dim3((unsigned)blocks_per_item * n), dim3(256), 0, static_cast<hipStream_t>(stream),
                     om, offmask, om_item, offmask_item, HW, blocks_per_item);
  return stif_check_launch(fn);
}
