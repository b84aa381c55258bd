// PSNR / SSIM of decoded frames against ground truth, on the device (the reference scores on the host:
// myutils.test_metric_adobe_liif4x, myutils.py:1151-1174, through utils.util.tensor2img / calculate_psnr / ssim,
// util.py:105-174, and data.util.bgr2ycbcr, data/util.py:181-202; float form: myutils.calc_psnr, :269-271).
//
// One fused kernel, one pass: a 256-thread workgroup takes a 32 x 32 tile of one plane of one item (1 plane in Y
// mode, 3 in RGB mode), loads the tile plus a 5-pixel halo of both images (prediction through element strides,
// ground truth as uint8 BGR HWC with a row pitch), quantises the prediction as tensor2img does
// (rintf(clamp(o, 0, 1) * 255.f), fp32, half to even), converts to Y or takes the channel, and keeps both
// planes in LDS as doubles.  It sums the squared error of its own pixels, runs the separable 11-tap Gaussian
// (horizontal pass into LDS, vertical pass out of it) first on a, b and then on a^2, b^2, ab, evaluates the
// SSIM map at its centres whose window lies inside the image, and writes four partial sums.  Everything after
// the fp32 quantisation is fp64: E[x^2] - mu^2 at 255^2 cancels to ~4e-3 absolute in fp32 against C2 = 58.5.
// A second small launch adds each item's partials in a fixed order: no floating-point atomics, so two runs on
// the same inputs give the same bits.
//
// The float protocol (myutils.eval_metrics, myutils.py:234-241: calc_psnr beside ssim_matlab, :105-158) has its
// own kernel, k_metric_float, further down: the squared error of the unclamped floats, and the SSIM of the
// frames clamped to [0, 1] with an 11 x 11 x 11 window over (channel, row, column), replicate padding, every
// position a centre.
#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

#include <math.h>

#include <algorithm>

namespace {

constexpr int TH = 32, TW = 32;   // output tile (rows x columns)
constexpr int RAD = 5, TAPS = 11;
constexpr int AH = TH + 2 * RAD, AW = TW + 2 * RAD;   // tile + halo: 42 x 42

struct Window { double k[TAPS]; };

// cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 sigma^2)) scaled by the reciprocal of the sum
Window host_window() {
  Window w;
  double sum = 0.0;
  for (int i = 0; i < TAPS; ++i) {
    const double x = (double)(i - RAD);
    w.k[i] = exp(-(x * x) / 4.5);
    sum += w.k[i];
  }
  const double inv = 1.0 / sum;
  for (int i = 0; i < TAPS; ++i) w.k[i] *= inv;
  return w;
}

struct MetricParams {
  const float* pred;
  const unsigned char* gt_u8;
  const float* gt_f32;
  long long pred_item, pred_plane, pred_pitch;   // elements
  long long gt_item, gt_pitch;                   // bytes
  long long gtf_item, gtf_plane, gtf_pitch;      // elements
  int n, H, W, flags;
  int planes, tiles_x, tiles_y;
};

// tensor2img's quantisation: (clamp(o, 0, 1) * 255.0).round() in fp32 (numpy rounds half to even)
STIF_DEV float quant(float o) { return rintf(fminf(fmaxf(o, 0.f), 1.f) * 255.f); }
// bgr2ycbcr(only_y=True) on the 0..255 scale, not rounded.  No FMA contraction: the prediction's and the ground
// truth's luma must round the same way, so that equal pixels give a squared error of exactly 0 (PSNR inf)
STIF_DEV double luma(double b, double g, double r) {
#pragma clang fp contract(off)
  return (24.966 * b + 128.553 * g + 65.481 * r) / 255.0 + 16.0;
}

// C1 = (0.01 L)^2, C2 = (0.03 L)^2 for the data range L
STIF_DEV double ssim_point(double mu1, double mu2, double eaa, double ebb, double eab, double C1, double C2) {
#pragma clang fp contract(off)
  const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  const double s1 = eaa - mu1_sq, s2 = ebb - mu2_sq, s12 = eab - mu1_mu2;
  return ((2.0 * mu1_mu2 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
}

// sum over the 64 lanes in a fixed order
STIF_DEV double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// the block's four partial sums: the two sums added over the 256 threads in a fixed order, the two counts as given
STIF_DEV void block_partial(double sse, double ssum, double npix, double nwin, double (*sred)[2],
                            double* __restrict__ part) {
  const int tid = threadIdx.x;
  sse = wave_sum(sse);
  ssum = wave_sum(ssum);
  if ((tid & 63) == 0) {
    sred[tid >> 6][0] = sse;
    sred[tid >> 6][1] = ssum;
  }
  __syncthreads();
  if (tid == 0) {
    double* o = part + (size_t)blockIdx.x * 4;
    o[0] = (sred[0][0] + sred[1][0]) + (sred[2][0] + sred[3][0]);
    o[1] = npix;
    o[2] = (sred[0][1] + sred[1][1]) + (sred[2][1] + sred[3][1]);
    o[3] = nwin;
  }
}

typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int SAW = 64;   // row stride of the two planes in doubles (42 used)

// out = the 11-tap sums centred on columns c + 5 and c + 6 of a row, from the 12 doubles at row[0..11] (16-byte aligned)
STIF_DEV void row_pair(const double* row, const Window& win, f64x2& out) {
  double v[12];
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    const f64x2 t = *reinterpret_cast<const f64x2*>(row + 2 * m);
    v[2 * m] = t[0];
    v[2 * m + 1] = t[1];
  }
#pragma unroll
  for (int j = 0; j < TAPS; ++j) {
    out[0] += win.k[j] * v[j];
    out[1] += win.k[j] * v[j + 1];
  }
}

// out[0], out[1] = the 11-tap vertical sums of a column pair for two consecutive rows, from the 12 rows at `top`
// (row stride TW doubles)
STIF_DEV void col_pair(const double* top, const Window& win, f64x2 out[2]) {
  f64x2 v[12];
#pragma unroll
  for (int t = 0; t < 12; ++t) v[t] = *reinterpret_cast<const f64x2*>(top + t * TW);
  out[0] = f64x2{0.0, 0.0};
  out[1] = f64x2{0.0, 0.0};
#pragma unroll
  for (int j = 0; j < TAPS; ++j) {
    out[0] += win.k[j] * v[j];
    out[1] += win.k[j] * v[j + 1];
  }
}

// LDS: the two planes 2 x 42 rows x 64 doubles (43,008 B) + three filtered fields 3 x 42 x 32 doubles (32,256 B)
// + 64 B of wave sums = 75,328 B: two workgroups per CU.  The filter passes read and write pairs of adjacent
// doubles as 16-byte accesses (ds_read_b128 / ds_write_b128, 256 B/clk against 128 for the 8-byte pairs the
// compiler makes of scalar reads): lane l takes column pair l & 15 of row l >> 4 (+ a row offset), so each
// 16-lane group of a b128 access holds the 16 column pairs of one or two rows, 256 consecutive bytes modulo the
// row stride.  Both row strides (512 B and 256 B) are multiples of the 256-byte bank row, so those 16 addresses
// fall on 16 different 16-byte slots: no bank conflict.
__global__ __launch_bounds__(256, 2) void k_metric(MetricParams p, Window win, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double sa[AH][SAW];
  __shared__ __attribute__((aligned(16))) double sb[AH][SAW];
  __shared__ __attribute__((aligned(16))) double sh[3][AH][TW];
  __shared__ double sred[4][2];

  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int plane = b % p.planes;
  b /= p.planes;
  const int tx = b % p.tiles_x;
  b /= p.tiles_x;
  const int ty = b % p.tiles_y;
  const int item = b / p.tiles_y;
  const int y0 = ty * TH, x0 = tx * TW;
  const int H = p.H, W = p.W;
  const bool fl = (p.flags & STIF_METRIC_FLOAT) != 0;
  const bool ymode = (p.flags & STIF_METRIC_Y) != 0;
  // centres of this tile whose 11 x 11 window lies inside the image: rows [cy0, cy1), columns [cx0, cx1)
  const int cy0 = max(y0, RAD), cy1 = min(y0 + TH, H - RAD);
  const int cx0 = max(x0, RAD), cx1 = min(x0 + TW, W - RAD);
  const bool do_ssim = (p.flags & STIF_METRIC_SSIM) != 0 && cy1 > cy0 && cx1 > cx0;   // the same in every thread

  const float* pr = p.pred + (size_t)item * p.pred_item;
  const unsigned char* gu = fl ? nullptr : p.gt_u8 + (size_t)item * p.gt_item;
  const float* gf = fl ? p.gt_f32 + (size_t)item * p.gtf_item : nullptr;

  double sse = 0.0;
  for (int idx = tid; idx < AH * AW; idx += 256) {
    const int r = idx / AW, c = idx - r * AW;
    const int y = y0 - RAD + r, x = x0 - RAD + c;
    const bool own = r >= RAD && r < RAD + TH && c >= RAD && c < RAD + TW;
    double a = 0.0, g = 0.0;
    if (y >= 0 && y < H && x >= 0 && x < W && (own || do_ssim)) {
      const size_t po = (size_t)y * p.pred_pitch + x;
      if (fl) {
        a = (double)pr[(size_t)plane * p.pred_plane + po];
        g = (double)gf[(size_t)plane * p.gtf_plane + (size_t)y * p.gtf_pitch + x];
      } else {
        const unsigned char* gp = gu + (size_t)y * p.gt_pitch + (size_t)x * 3;
        if (ymode) {
          const float qr = quant(pr[po]), qg = quant(pr[(size_t)p.pred_plane + po]),
                      qb = quant(pr[2 * (size_t)p.pred_plane + po]);
          a = luma((double)qb, (double)qg, (double)qr);
          g = luma((double)gp[0], (double)gp[1], (double)gp[2]);
        } else {
          a = (double)quant(pr[(size_t)plane * p.pred_plane + po]);
          g = (double)gp[2 - plane];   // prediction planes are R, G, B; ground-truth bytes B, G, R
        }
      }
      if (own) {
        const double d = a - g;
        sse += d * d;
      }
    }
    sa[r][c] = a;
    sb[r][c] = g;
  }

  double ssum = 0.0;
  if (do_ssim) {
    __syncthreads();
    // Every thread filters pairs of adjacent columns: 12 doubles of a row give the two horizontal sums, 12 rows of
    // a column pair give two rows of vertical sums (four centres per thread), all through 16-byte LDS accesses.
    // horizontal pass of a, b over every halo row; field (r, c) is centred on image column x0 + c
    for (int it = tid; it < AH * (TW / 2); it += 256) {
      const int r = it >> 4, c = (it & 15) * 2;
      f64x2 ha = {0.0, 0.0}, hb = {0.0, 0.0};
      row_pair(&sa[r][c], win, ha);
      row_pair(&sb[r][c], win, hb);
      *reinterpret_cast<f64x2*>(&sh[0][r][c]) = ha;
      *reinterpret_cast<f64x2*>(&sh[1][r][c]) = hb;
    }
    __syncthreads();
    // vertical pass: thread t owns rows 2 (t >> 4), + 1 and columns 2 (t & 15), + 1 of the tile
    const int vr = (tid >> 4) * 2, vc = (tid & 15) * 2;
    f64x2 mu1[2], mu2[2];
    col_pair(&sh[0][vr][vc], win, mu1);
    col_pair(&sh[1][vr][vc], win, mu2);
    __syncthreads();
    for (int it = tid; it < AH * (TW / 2); it += 256) {
      const int r = it >> 4, c = (it & 15) * 2;
      double a[12], g[12];
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        const f64x2 va = *reinterpret_cast<const f64x2*>(&sa[r][c + 2 * m]);
        const f64x2 vg = *reinterpret_cast<const f64x2*>(&sb[r][c + 2 * m]);
        a[2 * m] = va[0];
        a[2 * m + 1] = va[1];
        g[2 * m] = vg[0];
        g[2 * m + 1] = vg[1];
      }
      f64x2 haa = {0.0, 0.0}, hbb = {0.0, 0.0}, hab = {0.0, 0.0};
      double paa = a[0] * a[0], pbb = g[0] * g[0], pab = a[0] * g[0];
#pragma unroll
      for (int j = 0; j < TAPS; ++j) {
        const double qaa = a[j + 1] * a[j + 1], qbb = g[j + 1] * g[j + 1], qab = a[j + 1] * g[j + 1];
        haa[0] += win.k[j] * paa;
        hbb[0] += win.k[j] * pbb;
        hab[0] += win.k[j] * pab;
        haa[1] += win.k[j] * qaa;
        hbb[1] += win.k[j] * qbb;
        hab[1] += win.k[j] * qab;
        paa = qaa;
        pbb = qbb;
        pab = qab;
      }
      *reinterpret_cast<f64x2*>(&sh[0][r][c]) = haa;
      *reinterpret_cast<f64x2*>(&sh[1][r][c]) = hbb;
      *reinterpret_cast<f64x2*>(&sh[2][r][c]) = hab;
    }
    __syncthreads();
    f64x2 eaa[2], ebb[2], eab[2];
    col_pair(&sh[0][vr][vc], win, eaa);
    col_pair(&sh[1][vr][vc], win, ebb);
    col_pair(&sh[2][vr][vc], win, eab);
#pragma unroll
    for (int dr = 0; dr < 2; ++dr)
#pragma unroll
      for (int dc = 0; dc < 2; ++dc) {
        const int y = y0 + vr + dr, x = x0 + vc + dc;
        if (y >= cy0 && y < cy1 && x >= cx0 && x < cx1)
          ssum += ssim_point(mu1[dr][dc], mu2[dr][dc], eaa[dr][dc], ebb[dr][dc], eab[dr][dc], 6.5025, 58.5225);
      }
  }

  const double npix = (double)(min(y0 + TH, H) - y0) * (double)(min(x0 + TW, W) - x0);
  block_partial(sse, ssum, npix, do_ssim ? (double)(cy1 - cy0) * (double)(cx1 - cx0) : 0.0, sred, part);
}

// out[item][0..3] = the item's `per_item` partials added in a fixed order: thread t takes partials t, t + 256, ...
// in turn, then a binary tree over the 256 threads
__global__ __launch_bounds__(256) void k_metric_finish(const double* __restrict__ part, int per_item,
                                                       double* __restrict__ out) {
  __shared__ double red[256][4];
  const int tid = threadIdx.x, item = blockIdx.x;
  const double* src = part + (size_t)item * per_item * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < per_item; i += 256) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += src[(size_t)i * 4 + k];
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[tid][k] = s[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[tid][k] += red[tid + w][k];
    }
    __syncthreads();
  }
  if (tid < 4) out[(size_t)item * 4 + tid] = red[0][tid];
}

// ---- the float protocol: calc_psnr + ssim_matlab (volume) / myutils.ssim (planar)
//
// With 3 channels, a radius of 5 and replicate padding, tap j of the depth pass for output channel d reads input
// channel clamp(d - 5 + j, 0, 2): the depth pass is a fixed 3 x 3 mix per pixel, row d = (k0 + .. + k[5-d],
// k[6-d], k[7-d] + .. + k10).  It is applied to each of the five fields a, b, a^2, b^2, ab (squares first, then
// the mix); the rest is the separable 2-D filter of k_metric.  Planar mode is the identity mix.
struct ChannelMix { double m[3][3]; };   // [output channel][input channel]

ChannelMix host_mix(int mode) {
  ChannelMix x = {};
  const Window w = host_window();
  for (int d = 0; d < 3; ++d) {
    if (mode == STIF_FSSIM_PLANAR) {
      x.m[d][d] = 1.0;
      continue;
    }
    for (int j = 0; j < TAPS; ++j) x.m[d][std::min(std::max(d - RAD + j, 0), 2)] += w.k[j];
  }
  return x;
}

struct FloatParams {
  const float* pred;
  const float* ref;
  long long pred_item, pred_plane, pred_pitch;   // elements
  long long ref_item, ref_plane, ref_pitch;      // elements
  int H, W, tiles_x, tiles_y;
};

// the same expression for every field, so that equal inputs give equal bits (SSIM exactly 1 for identical images)
STIF_DEV double mix3(double m0, double m1, double m2, double x0, double x1, double x2) {
  return m0 * x0 + m1 * x1 + m2 * x2;
}

constexpr int HALO_ITERS = (AH * AW + 255) / 256;   // 7 halo pixels per thread

// A 256-thread workgroup takes a 32 x 32 tile of one output channel d of one item.  It loads the tile plus a
// 5-pixel halo of all three channels of both images -- halo coordinates clamped to the image rectangle, which is
// the replicate padding -- into registers (42 floats per thread, all loads issued before the first use) and sums
// the squared error of its own pixels of channel d from the unclamped floats.  It clamps, converts to fp64 and
// mixes the five fields of its halo pixels once; they pass through two LDS planes in three filter rounds, (a, b),
// (a^2, b^2), (ab) -- the later ones wait in registers -- each filtered horizontally into LDS and vertically into
// registers, both passes through 16-byte LDS accesses with k_metric's lane layout; last the SSIM at every pixel
// of the tile inside the image.
// LDS: two planes 2 x 42 rows x 64 doubles (43,008 B) + two filtered fields 2 x 42 x 32 doubles (21,504 B) + the
// first round's means parked per thread, 4 x 256 x 16 B (16,384 B: with them in registers the kernel spilled at
// the 256 VGPRs of two waves per SIMD) + 64 B of wave sums = 80,960 B: two workgroups per CU (161,920 of
// 163,840 B).  All five fields in LDS at once are 139,840 B, one workgroup per CU: 1.56x slower.
__global__ __launch_bounds__(256, 2) void k_metric_float(FloatParams p, Window win, ChannelMix mix,
                                                         double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) double sa[AH][SAW];
  __shared__ __attribute__((aligned(16))) double sb[AH][SAW];
  __shared__ __attribute__((aligned(16))) double sh[2][AH][TW];
  __shared__ f64x2 smu[4][256];
  __shared__ double sred[4][2];

  const int tid = threadIdx.x;
  int b = blockIdx.x;
  const int d = b % 3;
  b /= 3;
  const int tx = b % p.tiles_x;
  b /= p.tiles_x;
  const int ty = b % p.tiles_y;
  const int item = b / p.tiles_y;
  const int y0 = ty * TH, x0 = tx * TW;
  const int H = p.H, W = p.W;
  const double m0 = mix.m[d][0], m1 = mix.m[d][1], m2 = mix.m[d][2];

  const float* pr = p.pred + (size_t)item * p.pred_item;
  const float* gr = p.ref + (size_t)item * p.ref_item;

  // every address is inside the image rectangle: rows and columns are clamped, and so is the index of the last,
  // partial round (its values are not used)
  float pv[HALO_ITERS][3], gv[HALO_ITERS][3];
#pragma unroll
  for (int it = 0; it < HALO_ITERS; ++it) {
    const int idx = min(tid + it * 256, AH * AW - 1);
    const int r = idx / AW, c = idx - r * AW;
    const int y = min(max(y0 - RAD + r, 0), H - 1), x = min(max(x0 - RAD + c, 0), W - 1);
    const size_t po = (size_t)y * p.pred_pitch + x, go = (size_t)y * p.ref_pitch + x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      pv[it][ch] = pr[(size_t)ch * p.pred_plane + po];
      gv[it][ch] = gr[(size_t)ch * p.ref_plane + go];
    }
  }

  double sse = 0.0;
#pragma unroll
  for (int it = 0; it < HALO_ITERS; ++it) {
    const int idx = tid + it * 256;
    const int r = idx / AW, c = idx - r * AW;
    if (r >= RAD && r < RAD + TH && c >= RAD && c < RAD + TW && y0 - RAD + r < H && x0 - RAD + c < W) {
      const float po = d == 0 ? pv[it][0] : d == 1 ? pv[it][1] : pv[it][2];
      const float go = d == 0 ? gv[it][0] : d == 1 ? gv[it][1] : gv[it][2];
      const double e = (double)po - (double)go;
      sse += e * e;
    }
  }

  // the five mixed fields of this thread's halo pixels (products first, then the mix): a, b go to LDS now, a^2,
  // b^2, ab wait in registers for their rounds
  double faa[HALO_ITERS], fbb[HALO_ITERS], fab[HALO_ITERS];
#pragma unroll
  for (int it = 0; it < HALO_ITERS; ++it) {
    double a[3], g[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      a[ch] = (double)fminf(fmaxf(pv[it][ch], 0.f), 1.f);
      g[ch] = (double)fminf(fmaxf(gv[it][ch], 0.f), 1.f);
    }
    faa[it] = mix3(m0, m1, m2, a[0] * a[0], a[1] * a[1], a[2] * a[2]);
    fbb[it] = mix3(m0, m1, m2, g[0] * g[0], g[1] * g[1], g[2] * g[2]);
    fab[it] = mix3(m0, m1, m2, a[0] * g[0], a[1] * g[1], a[2] * g[2]);
    const int idx = tid + it * 256;
    if (idx < AH * AW) {
      const int r = idx / AW, c = idx - r * AW;
      sa[r][c] = mix3(m0, m1, m2, a[0], a[1], a[2]);
      sb[r][c] = mix3(m0, m1, m2, g[0], g[1], g[2]);
    }
  }
  // fa into sa and, if given, fb into sb
  auto put = [&](const double* fa, const double* fb) {
#pragma unroll
    for (int it = 0; it < HALO_ITERS; ++it) {
      const int idx = tid + it * 256;
      if (idx < AH * AW) {
        const int r = idx / AW, c = idx - r * AW;
        sa[r][c] = fa[it];
        if (fb) sb[r][c] = fb[it];
      }
    }
  };
  // horizontal pass of sa (and sb) over every halo row into sh[0] (sh[1]); field (r, c) is centred on column x0 + c
  auto hpass = [&](bool both) {
    for (int it = tid; it < AH * (TW / 2); it += 256) {
      const int r = it >> 4, c = (it & 15) * 2;
      f64x2 h0 = {0.0, 0.0};
      row_pair(&sa[r][c], win, h0);
      *reinterpret_cast<f64x2*>(&sh[0][r][c]) = h0;
      if (both) {
        f64x2 h1 = {0.0, 0.0};
        row_pair(&sb[r][c], win, h1);
        *reinterpret_cast<f64x2*>(&sh[1][r][c]) = h1;
      }
    }
  };
  // vertical pass: thread t owns rows 2 (t >> 4), + 1 and columns 2 (t & 15), + 1 of the tile
  const int vr = (tid >> 4) * 2, vc = (tid & 15) * 2;
  f64x2 mu1[2], mu2[2], eaa[2], ebb[2], eab[2];

  __syncthreads();
  hpass(true);
  __syncthreads();
  put(faa, fbb);        // sa, sb were last read before the barrier above; sh is rewritten after the one below
  col_pair(&sh[0][vr][vc], win, mu1);
  col_pair(&sh[1][vr][vc], win, mu2);
#pragma unroll
  for (int k = 0; k < 2; ++k) {   // parked in the thread's own LDS slots until the last round: 16 registers
    smu[k][tid] = mu1[k];
    smu[2 + k][tid] = mu2[k];
  }
  __syncthreads();
  hpass(true);
  __syncthreads();
  put(fab, nullptr);
  col_pair(&sh[0][vr][vc], win, eaa);
  col_pair(&sh[1][vr][vc], win, ebb);
  __syncthreads();
  hpass(false);
  __syncthreads();
  col_pair(&sh[0][vr][vc], win, eab);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    mu1[k] = smu[k][tid];
    mu2[k] = smu[2 + k][tid];
  }

  double ssum = 0.0;
#pragma unroll
  for (int dr = 0; dr < 2; ++dr)
#pragma unroll
    for (int dc = 0; dc < 2; ++dc) {
      if (y0 + vr + dr < H && x0 + vc + dc < W)   // every pixel is a centre; data range 1: C1 = 1e-4, C2 = 9e-4
        ssum += ssim_point(mu1[dr][dc], mu2[dr][dc], eaa[dr][dc], ebb[dr][dc], eab[dr][dc], 1e-4, 9e-4);
    }

  const double npix = (double)(min(y0 + TH, H) - y0) * (double)(min(x0 + TW, W) - x0);
  block_partial(sse, ssum, npix, npix, sred, part);
}

// tiles of a float-protocol call (three blocks per tile); false when the sizes or the mode are not valid
bool float_grid(int n, int H, int W, int mode, int* tiles_x, int* tiles_y, long long* blocks) {
  if (n < 1 || H < TAPS || W < TAPS) return false;
  if (mode != STIF_FSSIM_VOLUME && mode != STIF_FSSIM_PLANAR) return false;
  *tiles_x = (W + TW - 1) / TW;
  *tiles_y = (H + TH - 1) / TH;
  *blocks = (long long)n * 3 * *tiles_x * *tiles_y;
  return *blocks <= 0x7fffffffLL;
}

// planar fp32 [n][3][H][W] addressing: all zero = dense; otherwise rows, planes and items must not overlap
bool planar_strides(int n, long long H, long long W, long long item, long long plane, long long pitch,
                    long long* o_item, long long* o_plane, long long* o_pitch) {
  if (item == 0 && plane == 0 && pitch == 0) {
    *o_pitch = W;
    *o_plane = H * W;
    *o_item = 3 * H * W;
    return true;
  }
  const long long rows = (H - 1) * pitch + W;   // extent of one plane
  if (pitch < W || plane < rows || (n > 1 && item < 2 * plane + rows)) return false;
  *o_item = item;
  *o_plane = plane;
  *o_pitch = pitch;
  return true;
}

// tiles and planes of a call; false when the sizes or flags are not valid
bool metric_grid(int n, int H, int W, int flags, int* planes, int* tiles_x, int* tiles_y, long long* blocks) {
  if (n < 1 || H < 1 || W < 1) return false;
  if (flags & ~(STIF_METRIC_Y | STIF_METRIC_SSIM | STIF_METRIC_FLOAT)) return false;
  if ((flags & STIF_METRIC_FLOAT) && (flags & (STIF_METRIC_Y | STIF_METRIC_SSIM))) return false;
  *planes = (flags & STIF_METRIC_Y) ? 1 : 3;
  *tiles_x = (W + TW - 1) / TW;
  *tiles_y = (H + TH - 1) / TH;
  *blocks = (long long)n * *planes * *tiles_x * *tiles_y;
  return *blocks <= 0x7fffffffLL;
}

}  // namespace

extern "C" int stif_metric_window(double k[11]) {
  if (!k) return stif_fail(STIF_E_INVALID, "stif_metric_window: null pointer");
  const Window w = host_window();
  for (int i = 0; i < TAPS; ++i) k[i] = w.k[i];
  return STIF_OK;
}

extern "C" size_t stif_metric_workspace_size(int n, int H, int W, int flags) {
  int planes, tiles_x, tiles_y;
  long long blocks;
  if (!metric_grid(n, H, W, flags, &planes, &tiles_x, &tiles_y, &blocks)) return 0;
  return (size_t)blocks * 4 * sizeof(double);
}

extern "C" int stif_metric_psnr_ssim(const stif_metric_args* a, double* out, void* workspace, size_t workspace_bytes,
                                     void* stream) {
  // every check comes before the first launch
  if (!a || !out) return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: null args or out");
  if (a->n < 1 || a->H < 1 || a->W < 1) return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: n, H, W must be >= 1");
  if (a->flags & ~(STIF_METRIC_Y | STIF_METRIC_SSIM | STIF_METRIC_FLOAT))
    return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: unknown flag");
  const bool fl = (a->flags & STIF_METRIC_FLOAT) != 0;
  if (fl && (a->flags & (STIF_METRIC_Y | STIF_METRIC_SSIM)))
    return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: STIF_METRIC_FLOAT excludes STIF_METRIC_Y and STIF_METRIC_SSIM");
  if (!a->pred) return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: pred is null");
  if (fl ? !a->gt_f32 : !a->gt_u8)
    return stif_fail(STIF_E_INVALID, fl ? "stif_metric_psnr_ssim: float mode needs gt_f32" : "stif_metric_psnr_ssim: gt_u8 is null");
  int planes, tiles_x, tiles_y;
  long long blocks;
  if (!metric_grid(a->n, a->H, a->W, a->flags, &planes, &tiles_x, &tiles_y, &blocks))
    return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: too many tiles for one launch");
  const long long H = a->H, W = a->W;

  MetricParams p;
  p.pred = a->pred;
  p.gt_u8 = a->gt_u8;
  p.gt_f32 = a->gt_f32;
  if (!planar_strides(a->n, H, W, a->pred_item, a->pred_plane, a->pred_pitch, &p.pred_item, &p.pred_plane,
                      &p.pred_pitch))
    return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: pred strides: pitch < W or overlapping planes / items");
  p.gt_item = p.gt_pitch = 0;
  p.gtf_item = p.gtf_plane = p.gtf_pitch = 0;
  if (fl) {
    if (!planar_strides(a->n, H, W, a->gtf_item, a->gtf_plane, a->gtf_pitch, &p.gtf_item, &p.gtf_plane, &p.gtf_pitch))
      return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: gt_f32 strides: pitch < W or overlapping planes / items");
  } else if (a->gt_item == 0 && a->gt_pitch == 0) {
    p.gt_pitch = 3 * W;
    p.gt_item = 3 * W * H;
  } else {
    if (a->gt_pitch < 3 * W || (a->n > 1 && a->gt_item < (H - 1) * a->gt_pitch + 3 * W))
      return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: gt_u8 strides: pitch < 3 W or overlapping items");
    p.gt_pitch = a->gt_pitch;
    p.gt_item = a->gt_item;
  }
  const size_t need = (size_t)blocks * 4 * sizeof(double);
  if (!workspace || workspace_bytes < need)
    return stif_fail(STIF_E_WORKSPACE, "stif_metric_psnr_ssim: workspace smaller than stif_metric_workspace_size");
  if (((uintptr_t)workspace & 7) || ((uintptr_t)out & 7))
    return stif_fail(STIF_E_INVALID, "stif_metric_psnr_ssim: out and workspace must be 8-byte aligned");
  p.n = a->n;
  p.H = a->H;
  p.W = a->W;
  p.flags = a->flags;
  p.planes = planes;
  p.tiles_x = tiles_x;
  p.tiles_y = tiles_y;

  double* part = (double*)workspace;
  hipLaunchKernelGGL(k_metric, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, host_window(), part);
  int rc = stif_check_launch("stif_metric_psnr_ssim");
  if (rc) return rc;
  hipLaunchKernelGGL(k_metric_finish, dim3((unsigned)a->n), dim3(256), 0, (hipStream_t)stream, (const double*)part,
                     planes * tiles_x * tiles_y, out);
  return stif_check_launch("stif_metric_psnr_ssim (finish)");
}

extern "C" size_t stif_metric_float_workspace_size(int n, int H, int W, int mode) {
  int tiles_x, tiles_y;
  long long blocks;
  if (!float_grid(n, H, W, mode, &tiles_x, &tiles_y, &blocks)) return 0;
  return (size_t)blocks * 4 * sizeof(double);
}

extern "C" int stif_metric_float(const stif_metric_args* a, int mode, double* out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  // every check comes before the first launch
  if (!a || !out) return stif_fail(STIF_E_INVALID, "stif_metric_float: null args or out");
  if (a->n < 1) return stif_fail(STIF_E_INVALID, "stif_metric_float: n must be >= 1");
  if (a->H < TAPS || a->W < TAPS)
    return stif_fail(STIF_E_INVALID, "stif_metric_float: H and W must be >= 11 (the reference's smaller window for "
                                     "smaller images is not reproduced)");
  if (mode != STIF_FSSIM_VOLUME && mode != STIF_FSSIM_PLANAR)
    return stif_fail(STIF_E_INVALID, "stif_metric_float: mode must be STIF_FSSIM_VOLUME or STIF_FSSIM_PLANAR");
  if (a->flags != 0 && a->flags != STIF_METRIC_FLOAT)
    return stif_fail(STIF_E_INVALID, "stif_metric_float: flags must be 0 or STIF_METRIC_FLOAT");
  if (!a->pred || !a->gt_f32) return stif_fail(STIF_E_INVALID, "stif_metric_float: pred or gt_f32 is null");
  int tiles_x, tiles_y;
  long long blocks;
  if (!float_grid(a->n, a->H, a->W, mode, &tiles_x, &tiles_y, &blocks))
    return stif_fail(STIF_E_INVALID, "stif_metric_float: too many tiles for one launch");
  FloatParams p;
  p.pred = a->pred;
  p.ref = a->gt_f32;
  if (!planar_strides(a->n, a->H, a->W, a->pred_item, a->pred_plane, a->pred_pitch, &p.pred_item, &p.pred_plane,
                      &p.pred_pitch))
    return stif_fail(STIF_E_INVALID, "stif_metric_float: pred strides: pitch < W or overlapping planes / items");
  if (!planar_strides(a->n, a->H, a->W, a->gtf_item, a->gtf_plane, a->gtf_pitch, &p.ref_item, &p.ref_plane,
                      &p.ref_pitch))
    return stif_fail(STIF_E_INVALID, "stif_metric_float: gt_f32 strides: pitch < W or overlapping planes / items");
  const size_t need = (size_t)blocks * 4 * sizeof(double);
  if (!workspace || workspace_bytes < need)
    return stif_fail(STIF_E_WORKSPACE, "stif_metric_float: workspace smaller than stif_metric_float_workspace_size");
  if (((uintptr_t)workspace & 7) || ((uintptr_t)out & 7))
    return stif_fail(STIF_E_INVALID, "stif_metric_float: out and workspace must be 8-byte aligned");
  p.H = a->H;
  p.W = a->W;
  p.tiles_x = tiles_x;
  p.tiles_y = tiles_y;

  double* part = (double*)workspace;
  hipLaunchKernelGGL(k_metric_float, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, host_window(),
                     host_mix(mode), part);
  int rc = stif_check_launch("stif_metric_float");
  if (rc) return rc;
  hipLaunchKernelGGL(k_metric_finish, dim3((unsigned)a->n), dim3(256), 0, (hipStream_t)stream, (const double*)part,
                     3 * tiles_x * tiles_y, out);
  return stif_check_launch("stif_metric_float (finish)");
}
