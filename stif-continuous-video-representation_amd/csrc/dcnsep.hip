// Fused DCN_sep for gfx950: conv_offset_mask (64 -> 216, 3x3) + chunk / cat / sigmoid + the
// modulated deformable conv (64 -> 64, 3x3, 8 deformable groups) in one kernel; the 216-channel
// offset/mask map never reaches HBM.
//
// Reference: DCN_sep.forward (DCNv2/dcn_v2.py:127-140) -> _DCNv2 -> dcn_v2_cuda_forward
// (src/cuda/dcn_v2_cuda.cu:42-172) with the sampling of modulated_deformable_im2col_gpu_kernel /
// dmcn_im2col_bilinear (dcn_v2_im2col_cuda.cu:25-54,125-195).
//
// Workgroup = NW = 4 waves (two 80-KB workgroups per CU), tile = NW output rows x 32 columns,
// wave w = output row w (lane & 31 = column).  Lane half h works on the deformable groups h, h + 2,
// h + 4, h + 6 throughout.
//
// Phase 1, the offset/mask conv as a direct implicit GEMM with the WEIGHTS as the MFMA A operand:
// D[om row][pixel] += W[om row][k] X[k][pixel] on split-fp16 v_mfma_f32_32x32x16_f16 (f16x3, fp32
// accumulation), 216 rows in 7 M-tiles.  The rows are permuted at packing time (stif_pack_conv_weight,
// STIF_PACK_DCNSEP) so that the accumulator registers of lane (pixel p, half h) hold exactly the
// (dy, dx, mask) of every tap of its four groups -- the offsets go from the MFMA accumulators
// straight into the bilinear sampling, with no exchange, no LDS round trip and no HBM traffic.
// K = 36 steps (16-channel chunk c, tap t); per step a wave reads its pixels' 8 channels of the staged
// input halo (two ds_read_b128), splits them once and runs 3 MFMAs per M-tile (21 MFMAs per step;
// 112 accumulator VGPRs).  The input halo ((NW + 2) x 34 pixels, one 16-channel chunk, 80-B pixel pitch:
// conflict-free reads) and the packed weights of each step (a 3-slot ring) arrive by LDS-DMA ahead of
// use; one barrier per step.
//
// Phase 2, the deformable conv, two groups per K step: per group pair (2a, 2a + 1) the 16-channel input
// tile with a 2-px margin and the pair's weight fragments are LDS-DMA'd into one buffer while the CU's
// other workgroup computes (staging the next pair ahead in an 8-wave workgroup was 5 % slower in the C0
// step); for every tap t lane
// half h samples group 2a + h's 8 channels at its pixel (global fallback outside the margin) -- the 16
// K values of one 32x32x16 MFMA -- and runs 3 MFMAs per 32-cout half:
// 9 K steps per pair instead of 10 for two single groups (tap pairs); epilogue through LDS as k_dcn.
#include "abi_util.h"
#include "stif.h"
#include "dcn_bilinear.h"

#include <algorithm>

namespace {

constexpr int NW = 4;                         // waves = output rows per tile; two 80-KB workgroups per CU
constexpr int WPE = 2;                        // waves per SIMD the kernel is register-budgeted for
constexpr int TW = 32;                        // output columns per tile
// phase 1
constexpr int MT = 7;                         // offset/mask M-tiles (224 rows >= 216)
constexpr int HC1 = TW + 2;                   // halo columns (NW + 2 halo rows)
constexpr int PX_F = 20;                      // floats per staged halo pixel: 16 channels + 4 pad
constexpr int D_SLOTS = (NW + 2) * HC1 * 5;   // 16-B slots per data chunk
constexpr int D_INS = 16;                     // DMA instructions per data chunk (the last ones partly pad)
constexpr int D_F = D_INS * 256;              // floats per data buffer
constexpr int KSTEPS = 36;                    // k = 9 c + t: 16-channel chunk c, tap t
constexpr int WK_F = MT * 2 * 256;            // packed weights of one step: [M-tile][plane][lane][8 halves]
constexpr int WK_INS = 16;                    // DMA instructions per step (14 carry data)
constexpr int RING = 3;
// phase 2
constexpr int M = 2;                          // staged margin around the 3x3 footprint
constexpr int TR = NW + 2 + 2 * M, TC = TW + 2 + 2 * M, TP = TC;
constexpr int T_EL = TR * 4 * TP;             // 16-B elements of the staged tile: [row][channel quad][col]
constexpr int T_INST = (T_EL + 63) / 64;      // 24
constexpr int WP_F = 9 * 2 * 2 * 256;         // packed B fragments of one group pair (36 KB)
constexpr int P_INS = ((T_INST + WP_F / 256 + NW - 1) / NW) * NW;   // pair stage (tile + weights + pad)
static_assert(P_INS % NW == 0 && D_INS % NW == 0 && WK_INS % NW == 0, "stage sizes");
static_assert(D_SLOTS <= D_INS * 64 && MT * 2 <= WK_INS, "phase-1 stages");
// LDS map (floats).  Phase 1: data chunks D0, D1 and the weight ring (80 KB); phase 2: one pair buffer
// (tile XT, weights XW) over them.  The epilogue blocks reuse D0.
constexpr int PW_PAD_F = (P_INS - T_INST) * 256;    // pair weight region incl. the pad instructions
constexpr int OFF_D0 = 0, OFF_D1 = D_F, OFF_W = OFF_D1 + D_F;
constexpr int OFF_XT = 0, OFF_XW = T_INST * 256;
constexpr int LDS_F = OFF_W + RING * 4096;
static_assert(WK_F <= 4096 && NW * 1024 <= D_F && LDS_F * 4 <= 80 * 1024 && OFF_XW + PW_PAD_F <= LDS_F, "LDS map");

// vmcnt waits with an immediate operand (the counts are wave-uniform): phase 1 waits for everything, for
// all but the next step's weights, or for all but those and the side stage of the next data chunk
constexpr int WQ = WK_INS / NW;   // weight DMA instructions per wave and step
constexpr int DQ = D_INS / NW;    // data DMA instructions per wave and chunk
STIF_DEV void wait_vm(int n) {
  static_assert(WQ == 4 && WQ + DQ == 8, "wait_vm's immediates are WQ and WQ + DQ");
  switch (n) {
    case WQ: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case WQ + DQ: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

template <int EPI>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(WPE))) void k_dcn_sep(stif_dcn_sep_args a) {
  __shared__ __attribute__((aligned(16))) float smem[LDS_F];
  const int tid = threadIdx.x, lane = tid & 63, l32 = lane & 31, hf = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int H = a.H, W = a.W;
  const int tiles_x = (W + TW - 1) / TW, tiles = tiles_x * ((H + NW - 1) / NW);
  // one flat grid over (weight set, item, tile), XCD-aware: each XCD walks a contiguous tile range, so
  // the halos neighbouring tiles share are fetched into one L2
  const int L = xcd_block(blockIdx.x, gridDim.x);
  const int z = L / tiles, tl = L - z * tiles;
  const int tx = tl % tiles_x, ty = tl / tiles_x;
  const SetItem si = set_item_of(a.item_base, z);
  const int g = si.g, n = si.n;
  const float* fea = a.fea[g] + (size_t)n * a.fea_item;
  const float* in = a.in[g] + (size_t)n * a.in_item;
  const float* wt = a.w[g];
  const int oy0 = ty * NW, ox0 = tx * TW;
  const int oy = oy0 + wv, ox = ox0 + l32;
  const bool pix_ok = oy < H && ox < W;
  const unsigned img_bytes = (unsigned)((size_t)H * W * 64 * 4);
  const __amdgpu_buffer_rsrc_t rfea = __builtin_amdgcn_make_buffer_rsrc((void*)fea, (short)0, (int)img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void*)in, (short)0, (int)img_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rwom =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.w_om[g], (short)0, KSTEPS * WK_F * 4, 0x00020000);

  // ---------------------------------------------------------------- stages (LDS-DMA)
  // data chunk c (channels 16c..16c+15) of the 10 x 34 halo: slot s = pixel * 5 + sub (sub 4 = pad)
  auto stage_data = [&](int c, float* dst) {
#pragma unroll
    for (int j = 0; j < DQ; ++j) {
      const int i = wv + j * NW;
      const int s = i * 64 + lane;
      const int px = s / 5, sub = s - 5 * px;
      const int row = px / HC1, col = px - HC1 * row;
      const int y = oy0 - 1 + row, x = ox0 - 1 + col;
      const bool ok = (s < D_SLOTS) & (sub < 4) & ((unsigned)y < (unsigned)H) & ((unsigned)x < (unsigned)W);
      const unsigned voff = ok ? (unsigned)((((size_t)y * W + x) * 64 + 16 * c + 4 * sub) * 4) : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rfea, dst + i * 256, 16, voff, 0, 0, 0);
    }
  };
  // the packed weights of step k: 16 pieces, four per wave; the two past the step's 14 KB load zeros (issuing only
  // the 14 that carry data was not faster, profiles/r06_wtrim_ab.log)
  auto stage_w = [&](int k, int slot) {
    float* dst = smem + OFF_W + slot * 4096;
#pragma unroll
    for (int j = 0; j < WQ; ++j) {
      const int i = wv + j * NW;
      const unsigned voff = i < MT * 2 ? (unsigned)((k * WK_F + i * 256) * 4 + lane * 16) : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rwom, dst + i * 256, 16, voff, 0, 0, 0);
    }
  };
  // phase-2 stage of group pair pa: the [row][channel quad][col][4] tile of channels 16 pa .. 16 pa + 15
  // and the pair's B fragments (instructions 0..23 tile, 24..59 weights)
  const int ty0 = oy0 - 1 - M, tx0 = ox0 - 1 - M;
  auto stage_pair = [&](int pa, float* st, float* sw) {
    const float* wc = wt + (size_t)pa * WP_F;
#pragma unroll 1
    for (int j = 0; j < P_INS / NW; ++j) {
      const int i = wv + j * NW;   // wave-uniform
      if (i >= T_INST && i < T_INST + WP_F / 256) {
        __builtin_amdgcn_global_load_lds(wc + ((i - T_INST) * 64 + lane) * 4, sw + (i - T_INST) * 256, 16, 0, 0);
      } else {
        const int e = i * 64 + lane;
        const int col = e % TP, rq = e / TP, q = rq & 3, row = rq >> 2;
        const int y = ty0 + row, x = tx0 + col;
        const bool ok = (i < T_INST) & (e < T_EL) & ((unsigned)y < (unsigned)H) & ((unsigned)x < (unsigned)W);
        const unsigned voff = ok ? (unsigned)((((size_t)y * W + x) * 64 + pa * 16 + q * 4) * 4) : 0x80000000u;
        float* dst = i < T_INST ? st + i * 256 : sw + (i - T_INST) * 256;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, dst, 16, voff, 0, 0, 0);   // tile (pad pieces load nothing)
      }
    }
  };

  // ---------------------------------------------------------------- phase 1: offset/mask conv
  // the accumulators start at bias x 2^14 (the f16x3 scale): no bias pass between the phases.  Slot s =
  // 16 m + r of lane half h is packed row (r & 3) + 8 (r >> 2) + 4 h of M-tile m (stif_pack_conv_weight,
  // STIF_PACK_DCNSEP: bias [M-tile][32 rows], zero on the padding rows)
  f32x16 om[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const f32x4 bq = ld4(a.b_om[g] + m * 32 + 8 * v + 4 * hf) * (1.0f / F16X3_UNSCALE);
#pragma unroll
      for (int e = 0; e < 4; ++e) om[m][4 * v + e] = bq[e];
    }
  stage_data(0, smem + OFF_D0);
  stage_w(0, 0);
  stage_w(1, 1);
  // chunk loop at run time, taps unrolled: tap offsets, ring slots ((9 c + t) % 3 = t % 3) and the waits
  // are compile-time; the next tap's data fragment is read and split while this tap's MFMAs run, each
  // M-tile's weight fragments one M-tile ahead (scheduling barriers pin that order: the compiler would
  // sink each read next to its MFMAs and wait for it there)
  f16x8 dh, dl;
#pragma unroll 1
  for (int c = 0; c < KSTEPS / 9; ++c) {
    const float* dbuf = smem + ((c & 1) ? OFF_D1 : OFF_D0) + (wv * HC1 + l32) * PX_F + hf * 8;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int k = 9 * c + t;
      // this step's weights (and, at a chunk start, its data) landed in every wave; the DMA issued in the
      // last two steps (weights of k + 1, the side stage of tap 1) may stay in flight
      if (t == 2 || t == 3) wait_vm(c < 3 ? WQ + DQ : WQ);
      else if (t == 8 && c == 3) wait_vm(0);
      else wait_vm(WQ);
      // a bare s_barrier: __syncthreads()'s workgroup fence would wait for vmcnt(0), i.e. for the DMA of
      // the next two steps too.  Every LDS read of the step that frees a ring slot has returned (its
      // MFMAs consumed it), and LDS-DMA visibility is the vmcnt wait above.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      // the first weight fragments right after the barrier; this step's data fragment was read and split
      // during the previous step (a chunk's first tap: read now), so the MFMAs start at once, and the
      // next steps' LDS-DMA is issued behind the first M-tile's MFMAs
      const float* wb = smem + OFF_W + (t % RING) * 4096 + lane * 4;
      f16x8 wh[2], wl[2];
      wh[0] = ldh8(wb);
      wl[0] = ldh8(wb + 256);
      if (t == 0) {
        split_f16x3(ld4(dbuf), ld4(dbuf + 4), dh, dl);
      }
      f32x4 x0, x1;
#pragma unroll
      for (int q = 0; q < MT; ++q) {
        if (q + 1 < MT) {
          wh[(q + 1) & 1] = ldh8(wb + (2 * q + 2) * 256);
          wl[(q + 1) & 1] = ldh8(wb + (2 * q + 3) * 256);
        }
        __builtin_amdgcn_sched_barrier(0);
        om[q] = mfma16h(wh[q & 1], dh, om[q]);
        om[q] = mfma16h(wh[q & 1], dl, om[q]);
        om[q] = mfma16h(wl[q & 1], dh, om[q]);
        if (q == 0) {
          if (t < 7 || c < 3) stage_w(k + 2, (t + 2) % RING);
          if (t == 1 && c < 3) stage_data(c + 1, smem + (((c + 1) & 1) ? OFF_D1 : OFF_D0));
        }
        if (q == 1 && t < 8) {   // the next tap of the same chunk: its buffer is stable until the chunk ends
          const float* nb = dbuf + (((t + 1) / 3) * HC1 + (t + 1) % 3) * PX_F;
          x0 = ld4(nb);
          x1 = ld4(nb + 4);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (t < 8) split_f16x3(x0, x1, dh, dl);   // the next step's B operand
    }
  }
  // slot s = 16 m + r of lane half h = component s % 3 (dy, dx, mask) of tap (s % 27) / 3 of group
  // 2 (s / 27) + h, packed row (r & 3) + 8 (r >> 2) + 4 h of M-tile m; bias, unscale, sigmoid(mask)
  // (dcn_v2.py:134-138)
  // unscale, sigmoid(mask) (dcn_v2.py:134-138); the range check is one sum (a non-finite value makes it
  // non-finite) -- a per-value compare would hold 108 lane masks in SGPRs
  float chk = 0.f;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int s = 16 * m + r;
      if (s < 108) {
        float x = om[m][r] * F16X3_UNSCALE;
        chk += x;
        if (s % 3 == 2) x = sigmoid_fast(x);
        om[m][r] = x;
      }
    }
  }
  const bool bad = not_finite(chk);
  report_range(a.status, bad);

  // ---------------------------------------------------------------- phase 2: deformable conv
  // dcn_tile_sample of this lane half's group (channels 16 pa + 8 h .. + 7: a0 = quad 2h, a1 = quad 2h + 1)
  // at tap `tap` with offset (dy, dx) and modulation mk
  auto sample = [&](const float* st, int pa, int tap, float dy, float dx, float mk, f32x4& a0, f32x4& a1) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    const float h_im = (float)(oy - 1 + ky) + dy;
    const float w_im = (float)(ox - 1 + kx) + dx;
    const bool valid = pix_ok & dcn_gate(h_im, w_im, H, W);
    dcn_tile_sample<4, 1>(st, TR, TC, TP, ty0, tx0, 2 * hf, in, pa * 16 + hf * 8, H, W, h_im, w_im, mk, valid, a0,
                          a1);
  };

  // accumulators start at the DCN bias x 2^14 (lane = output channel)
  f32x16 acc0, acc1;
  {
    const float b0 = a.bias[g][l32] * (1.0f / F16X3_UNSCALE), b1 = a.bias[g][32 + l32] * (1.0f / F16X3_UNSCALE);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc0[r] = b0;
      acc1[r] = b1;
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the om biases loaded
  __syncthreads();                                    // phase-1 buffers free
#pragma unroll
  for (int pa = 0; pa < 4; ++pa) {
    // one buffer: this pair's stage lands while the other workgroup on the CU computes
    if (pa) __syncthreads();   // every wave is done with the previous pair's buffer
    stage_pair(pa, smem + OFF_XT, smem + OFF_XW);
    lds_dma_barrier();   // waiting in tap groups instead was 1 % slower
    const float* st = smem + OFF_XT;
    const float* sw = smem + OFF_XW;
    // a tap-level software pipeline (tap t + 1's corner reads issued before tap t's blend, one more
    // sample set live) measured 4 % faster in the C0 step but made the outputs depend on the launch's
    // timing at two waves per SIMD; not kept
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int s = 27 * pa + 3 * t;   // this lane half's group 2 pa + h, tap t: slots s .. s + 2
      f32x4 a0, a1;
      sample(st, pa, t, om[s / 16][s % 16], om[(s + 1) / 16][(s + 1) % 16], om[(s + 2) / 16][(s + 2) % 16], a0, a1);
      f16x8 ah, al;
      split_f16x3(a0, a1, ah, al);
      mfma_f16x3_2nt(ah, al, sw + t * 1024 + lane * 4, acc0, acc1);   // [tap][nt][plane][lane][8 halves]
      __builtin_amdgcn_sched_barrier(0);   // one tap's operands live at a time (VGPR budget)
    }
  }
  __syncthreads();   // the epilogue blocks overwrite the pair buffer
  // epilogue through a per-wave LDS block -> coalesced 16-B stores (k_dcn's)
  float* out = a.out[g] + (size_t)n * a.out_item;
  float* blk = smem + OFF_D0 + wv * 1024;
  float chk2 = 0.f;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float t = (nt ? acc1[r] : acc0[r]) * F16X3_UNSCALE;
      chk2 += t;
      if (EPI == STIF_EPI_LRELU) t = lrelu01(t);
      v[r] = t;
    }
    store_tile_rows(blk, lane, v, out, oy, ox0, H, W, 64, nt * 32);
  }
  report_range(a.status, not_finite(chk2));
}

}  // namespace

extern "C" int stif_dcn_sep_nhwc(const stif_dcn_sep_args* pa, void* stream) {
  if (!pa) return stif_fail(STIF_E_INVALID, "stif_dcn_sep_nhwc: null args");
  stif_dcn_sep_args a = *pa;   // the kernel's copy: the item table in the form it scans
  long long items;
  int most;
  if (const int rc = stif_item_table("stif_dcn_sep_nhwc", a.ngroups, a.nitems, a.item_base, &items, &most)) return rc;
  if (a.H < 1 || a.W < 1) return stif_fail(STIF_E_INVALID, "stif_dcn_sep_nhwc: bad sizes");
  if (!(a.flags & STIF_CONV_F16X3))
    return stif_fail(STIF_E_INVALID, "stif_dcn_sep_nhwc: split-fp16 operands only (flags = STIF_CONV_F16X3)");
  if ((long long)a.H * a.W * 64 * 4 >= 0x7fffffffLL)
    return stif_fail(STIF_E_INVALID, "stif_dcn_sep_nhwc: item larger than 2 GB (buffer addressing)");
  for (int i = 0; i < a.ngroups; ++i)
    if (!a.fea[i] || !a.in[i] || !a.w_om[i] || !a.b_om[i] || !a.w[i] || !a.bias[i] || !a.out[i])
      return stif_fail(STIF_E_INVALID, "stif_dcn_sep_nhwc: null tensor");
  const long long wgs = (long long)((a.W + TW - 1) / TW) * ((a.H + NW - 1) / NW) * items;
  if (wgs > 0x7fffffff) return stif_fail(STIF_E_INVALID, "stif_dcn_sep_nhwc: grid too large");
  dim3 grid((unsigned)wgs);
  if (a.epi == STIF_EPI_LRELU)
    hipLaunchKernelGGL(k_dcn_sep<STIF_EPI_LRELU>, grid, dim3(64 * NW), 0, (hipStream_t)stream, a);
  else if (a.epi == STIF_EPI_NONE)
    hipLaunchKernelGGL(k_dcn_sep<STIF_EPI_NONE>, grid, dim3(64 * NW), 0, (hipStream_t)stream, a);
  else
    return stif_fail(STIF_E_INVALID, "stif_dcn_sep_nhwc: epilogue must be NONE or LRELU");
  return stif_check_launch("stif_dcn_sep_nhwc");
}
