// Modulated deformable convolution (DCNv2) for gfx950: k_dcn, the fused STIF path (64 -> 64, 3x3,
// stride 1, pad 1, 8 deformable groups), behind stif_dcn_nhwc.
// Reference: DCN_sep.forward (DCNv2/dcn_v2.py:127-140) -> dcn_v2_cuda_forward
// (src/cuda/dcn_v2_cuda.cu:42-172) = im2col into an HBM columns buffer + batched
// SGEMM.  Here each workgroup owns 4 rows x 32 columns of output pixels; for each
// deformable group (= 8 input channels = one K chunk) it bilinearly samples the
// group's 9 taps straight into an LDS A-tile (semantics of
// modulated_deformable_im2col_gpu_kernel / dmcn_im2col_bilinear,
// dcn_v2_im2col_cuda.cu:25-54,125-195: dcn_bilinear.h), stages the group's weight slice, and
// contracts with fp32 MFMA.  The columns buffer never exists.
// The `_ext` drop-in (NCHW, any shape, forward and backward) is dcn_v2.hip; at the STIF shape it runs k_dcn.
#include "dcn_bilinear.h"
#include "tuning.h"
#include "stif.h"
#include "abi_util.h"

namespace {

constexpr int OMC = 216;  // offmask channels per pixel: [group][tap][dy, dx, mask]

// Workgroup: DCN_ROWS waves, MR output rows x 32 px per wave, all 64 output channels.  Per deformable
// group (= 8 input channels = one K chunk): the group's input tile with an M-pixel margin around the
// 3x3 footprint ([row][channel half][col][4], zero-filled outside the frame) and the group's
// weight fragments are LDS-DMA'd one chunk ahead (double-buffered).  Each lane then bilinearly
// samples its own MFMA A-fragment (pixel = lane & 31, channels 4h..4h+3) tap by tap from the
// tile -- falling back to global loads only when an offset leaves the margin -- so sampling
// (VALU + LDS) interleaves with the MFMAs and no sampled A tile ever round-trips memory.
// F16: the contraction on split-fp16 MFMA (stif_common.h split_f16x3): two taps per 32x32x16 MFMA,
// lane half h sampling tap 2p + h (tap 9 = 0) for all 8 channels of the group (elements 0..7), so
// each (pixel, tap) computes its bilinear weights once; weights packed STIF_PACK_PLAIN |
// STIF_PACK_F16X3 ([group][pair][nt][plane][lane][8 halves]).  On large maps each wave owns MR = 2
// output rows (two M-tiles): every B fragment read from LDS feeds both rows' MFMAs, which halves the
// weight traffic through LDS (the bilinear corner reads at data-dependent addresses conflict) and
// stages fewer halo pixels per output (with 8 waves: C0 L1 shape 342 -> 322 us); small maps keep
// MR = 1, where the halved grid would leave CUs idle.  The kernel is latency-bound (waves parked on
// memory waits and group barriers 43 % of their cycles, profiles/r02_dcn_sq_c0l1.txt), so two
// independent 4-wave workgroups per CU beat one 8-wave workgroup.
constexpr int DCN_ROWS = DCN_TH;   // waves per workgroup

// MR: output rows per wave (2 only with F16; the launcher picks it by grid size, see stif_dcn_nhwc)
template <int EPI, int F16, int MR = 1>
__global__ __launch_bounds__(64 * DCN_ROWS) void k_dcn(stif_dcn_args a) {
  static_assert(MR == 1 || F16, "two rows per wave: split-fp16 path only");
  constexpr int NW = DCN_ROWS, TH = NW * MR, M = DCN_M;
  constexpr int TR = TH + 2 + 2 * M, TC = 32 + 2 + 2 * M;   // tile rows / cols
  constexpr int TP = TC;                                     // column pitch of the staged tile (16-B slots)
  constexpr int T_EL = TR * 2 * TP;                          // 16-B elements
  constexpr int T_INST = (T_EL + 63) / 64;
  constexpr int T_F = T_INST * 256;
  constexpr int W_F = F16 ? 5 * 2 * 2 * 256 : 9 * 2 * 64 * 4;   // packed B fragments of one group
  constexpr int BUF_F = T_F + W_F;
  __shared__ __attribute__((aligned(16))) float smem[2 * BUF_F];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l32 = lane & 31, hf = lane >> 5;
  const int H = a.H, W = a.W;
  const int tiles_x = (W + 31) >> 5;
  const int bx = blockIdx.x;
  const int tx = bx % tiles_x, ty = bx / tiles_x;
  const SetItem si = set_item_of(a.item_base, blockIdx.z);
  const int g = si.g, n = si.n;
  const float* in = a.in[g] + (size_t)n * a.in_item;
  const float* om = a.offmask[g] + (size_t)n * a.om_item;
  const float* wt = a.w[g];
  const int oy0 = ty * TH, ox0 = tx * 32;
  const int ty0 = oy0 - 1 - M, tx0 = ox0 - 1 - M;           // tile origin (frame coords)
  const int ox = ox0 + l32;                                  // this lane's output column
  int oy[MR];
  bool pix_ok[MR];
  const float* omp[MR];
#pragma unroll
  for (int mr = 0; mr < MR; ++mr) {                          // this wave's output rows
    oy[mr] = oy0 + wv * MR + mr;
    pix_ok[mr] = oy[mr] < H && ox < W;
    omp[mr] = om + ((size_t)min(oy[mr], H - 1) * W + min(ox, W - 1)) * OMC;
  }
  const __amdgpu_buffer_rsrc_t rin =
      __builtin_amdgcn_make_buffer_rsrc((void*)in, (short)0, (int)((size_t)H * W * 64 * 4), 0x00020000);

  auto stage = [&](int dg, int buf) {
    float* st = smem + buf * BUF_F;
    float* sw = st + T_F;
    for (int i = wv; i < T_INST; i += NW) {
      const int e = i * 64 + lane;
      const int col = e % TP, rh = e / TP, h = rh & 1, row = rh >> 1;
      const int y = ty0 + row, x = tx0 + col;
      const bool ok = e < T_EL && col < TC && y >= 0 && y < H && x >= 0 && x < W;
      const unsigned voff = ok ? (unsigned)((((size_t)y * W + x) * 64 + dg * 8 + h * 4) * 4) : 0x80000000u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, st + i * 256, 16, voff, 0, 0, 0);
    }
    const float* wc = wt + (size_t)dg * W_F;   // packed [chunk][tap][nt][lane][4]
    for (int i = wv; i < W_F / 256; i += NW)
      __builtin_amdgcn_global_load_lds(wc + (i * 64 + lane) * 4, sw + i * 256, 16, 0, 0);
  };
  // offset/mask values of a group: all 27 (fp32 path), or (F16) the 5 taps 2p + h of this lane half
  // as [p][dy, dx, m] (tap 9 reads tap 8's values and is masked off)
  constexpr int NOM = F16 ? 15 : 27;
  auto om_load = [&](int dgi, int mr, float* o) {
#pragma unroll
    for (int k = 0; k < NOM; ++k) o[k] = omp[mr][dgi * 27 + k];
  };
  // F16 variant: a group's 27 offset/mask floats (108 B, dword-aligned) as 6 x 16-B + 1 x 12-B loads
  // per lane instead of 15 scalar loads; lane half h picks its taps 2p + h at the group switch
  typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
  typedef float f32x3u __attribute__((ext_vector_type(3), aligned(4)));
  auto om_raw = [&](int dgi, int mr, float* r) {
    const float* p = omp[mr] + dgi * 27;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const f32x4u v = *reinterpret_cast<const f32x4u*>(p + 4 * i);
      r[4 * i] = v[0]; r[4 * i + 1] = v[1]; r[4 * i + 2] = v[2]; r[4 * i + 3] = v[3];
    }
    const f32x3u v = *reinterpret_cast<const f32x3u*>(p + 24);
    r[24] = v[0]; r[25] = v[1]; r[26] = v[2];
  };
  auto om_pick = [&](const float* r, float* o) {
#pragma unroll
    for (int k = 0; k < 15; ++k) {
      const int i0 = 6 * (k / 3) + k % 3;
      o[k] = (k < 12 && hf) ? r[i0 + 3] : r[i0];
    }
  };
  float omr[MR][27];
  float omc[MR][NOM], omn[MR][NOM];
#pragma unroll
  for (int mr = 0; mr < MR; ++mr) {
    if constexpr (F16) {
      om_raw(0, mr, omr[mr]);
      om_pick(omr[mr], omc[mr]);
    } else {
      om_load(0, mr, omc[mr]);
    }
  }

  // dcn_tile_sample of the group's 8 channels (F16: a0 = channels 0-3, a1 = 4-7) or of this lane half's 4
  // channels (fp32: a0) at tap `tap` of row mr (tap 9, the F16 pairs' padding, counts as gated off)
  auto sample = [&](const float* st, int dg, int mr, int tap, const float* oc, f32x4& a0, f32x4& a1) {
    const int ky = tap / 3, kx = tap - 3 * ky;
    const float h_im = (float)(oy[mr] - 1 + ky) + oc[0];
    const float w_im = (float)(ox - 1 + kx) + oc[1];
    const bool valid = pix_ok[mr] & (tap < 9) & dcn_gate(h_im, w_im, H, W);
    const int hsel = F16 ? 0 : hf;
    dcn_tile_sample<2, F16>(st, TR, TC, TP, ty0, tx0, hsel, in, dg * 8 + hsel * 4, H, W, h_im, w_im, oc[2], valid,
                            a0, a1);
  };

  f32x16 acc0[MR], acc1[MR];
#pragma unroll
  for (int mr = 0; mr < MR; ++mr) acc0[mr] = acc1[mr] = f32x16{0};
  stage(0, 0);
  lds_dma_barrier();
  for (int dg = 0; dg < 8; ++dg) {
    if (dg + 1 < 8) {
      stage(dg + 1, (dg + 1) & 1);
#pragma unroll
      for (int mr = 0; mr < MR; ++mr) {
        if constexpr (F16) om_raw(dg + 1, mr, omr[mr]);
        else om_load(dg + 1, mr, omn[mr]);
      }
    }
    const float* st = smem + (dg & 1) * BUF_F;
    const float* sw = st + T_F;
    if constexpr (F16) {
      // tap pair p: lane half h samples tap 2p + h for all 8 channels of the group -- one bilinear
      // weight set per (pixel, tap) -- and supplies them as the 8 K values of its MFMA A operand; the
      // pair's B fragments (read once) feed both rows
#pragma unroll
      for (int pp = 0; pp < 5; ++pp) {
        f16x8 ah[MR], al[MR];
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) {
          f32x4 a0, a1;
          sample(st, dg, mr, 2 * pp + hf, omc[mr] + pp * 3, a0, a1);
          split_f16x3(a0, a1, ah[mr], al[mr]);
        }
        const F16x3Frag2 b = ldh8_2nt(sw + pp * 1024 + lane * 4);   // [pair][nt][plane][lane][8 halves]
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) mfma_f16x3_2nt(ah[mr], al[mr], b, acc0[mr], acc1[mr]);
      }
    } else {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        // modulated_deformable_im2col (dcn_v2_im2col_cuda.cu:158-192) for this lane's pixel / tap
        f32x4 av, unused;
        sample(st, dg, 0, tap, omc[0] + tap * 3, av, unused);
        const f32x4 b0 = ld4(sw + ((tap * 2 + 0) * 64 + lane) * 4);
        const f32x4 b1 = ld4(sw + ((tap * 2 + 1) * 64 + lane) * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc0[0] = mfma32(av[q], b0[q], acc0[0]);
          acc1[0] = mfma32(av[q], b1[q], acc1[0]);
        }
      }
    }
    if (dg + 1 < 8) {
#pragma unroll
      for (int mr = 0; mr < MR; ++mr) {
        if constexpr (F16) {
          om_pick(omr[mr], omc[mr]);
        } else {
#pragma unroll
          for (int k = 0; k < NOM; ++k) omc[mr][k] = omn[mr][k];
        }
      }
    }
    lds_dma_barrier();
  }
  // epilogue through a per-wave LDS block -> coalesced 16-B stores (see tile_to_lds)
  float* out = a.out[g] + (size_t)n * a.out_item;
  const float* bias = a.bias[g];
  float* blk = smem + wv * 1024;
#pragma unroll
  for (int mr = 0; mr < MR; ++mr) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const float bv = bias[nt * 32 + l32];
      f32x16 v;
      bool bad = false;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float t = (nt ? acc1[mr][r] : acc0[mr][r]) * (F16 ? F16X3_UNSCALE : 1.f) + bv;
        if (F16) bad |= not_finite(t);
        if (EPI == STIF_EPI_LRELU) t = lrelu01(t);
        v[r] = t;
      }
      if (F16) report_range(a.status, bad);
      store_tile_rows(blk, lane, v, out, oy[mr], ox0, H, W, 64, nt * 32);
    }
  }
}

}  // namespace

extern "C" int stif_dcn_nhwc(const stif_dcn_args* pa, void* stream) {
  if (!pa) return stif_fail(STIF_E_INVALID, "stif_dcn_nhwc: null args");
  stif_dcn_args a = *pa;   // the kernel's copy: the item table in the form it scans
  long long items;
  int most;
  if (const int rc = stif_item_table("stif_dcn_nhwc", a.ngroups, a.nitems, a.item_base, &items, &most)) return rc;
  if (a.H < 1 || a.W < 1) return stif_fail(STIF_E_INVALID, "stif_dcn_nhwc: bad sizes");
  if (items > 65535) return stif_fail(STIF_E_INVALID, "stif_dcn_nhwc: too many items (grid z)");
  if ((long long)a.H * a.W * 64 * 4 >= 0x7fffffffLL)
    return stif_fail(STIF_E_INVALID, "stif_dcn_nhwc: item larger than 2 GB (buffer addressing)");
  const bool f16 = a.flags & STIF_CONV_F16X3;
  // two rows per wave (8-row workgroups, two per CU) when that still gives >= 4 workgroups per CU
  const long long wg2 = (long long)((a.W + 31) / 32) * ((a.H + 2 * DCN_ROWS - 1) / (2 * DCN_ROWS)) * items;
  const bool mr2 = f16 && wg2 >= DCN_MR2_MIN;
  const int th = DCN_ROWS * (mr2 ? 2 : 1);   // output rows per workgroup
  dim3 grid(((a.W + 31) / 32) * ((a.H + th - 1) / th), 1, (unsigned)items);
  if (a.epi != STIF_EPI_NONE && a.epi != STIF_EPI_LRELU)
    return stif_fail(STIF_E_INVALID, "stif_dcn_nhwc: epilogue must be NONE or LRELU");
  with_bool(a.epi == STIF_EPI_LRELU, [&](auto lrelu) {
    with_bool(f16, [&](auto h) {
      with_bool(mr2, [&](auto two) {
        constexpr int EPI = decltype(lrelu)::value ? STIF_EPI_LRELU : STIF_EPI_NONE;
        constexpr int F16 = decltype(h)::value, MR = decltype(two)::value ? 2 : 1;
        if constexpr (F16 || MR == 1)   // mr2 implies f16
          hipLaunchKernelGGL((k_dcn<EPI, F16, MR>), grid, dim3(64 * DCN_ROWS), 0, (hipStream_t)stream, a);
      });
    });
  });
  return stif_check_launch("stif_dcn_nhwc");
}
