// Drop-in for the DCNv2 extension `_ext` (NCHW, any shape) on gfx950: stif_dcn_v2_forward and
// stif_dcn_v2_backward.
// Forward: the STIF shape runs k_dcn (dcn.hip, through stif_dcn_nhwc) between NCHW <-> NHWC transposes
// (weights packed on the device); any other shape an im2col kernel into a caller workspace + an
// fp32-MFMA GEMM with the bias added at its store, per sample (dcn_v2_cuda_forward, dcn_v2_cuda.cu:42-172).
// Backward: dcn_v2_cuda_backward per sample (dcn_v2_cuda.cu:197-333), every shape on the generic kernels.
// The sampling semantics are dcn_bilinear.h's.
#include "dcn_bilinear.h"
#include "stif.h"
#include "abi_util.h"

#include <algorithm>
#include <cstdio>
#include <initializer_list>

namespace {

struct DcnGeom {
  int C, H, W, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, dg;
};

// ------------------------------------------------------------------ generic path
// columns[c*K + k][ho*Wo + wo] of one sample, exactly the reference's im2col layout (dcn_v2_cuda.cu:90).
__global__ __launch_bounds__(256) void k_im2col(const float* __restrict__ im, const float* __restrict__ off,
                                                const float* __restrict__ msk, float* __restrict__ col, DcnGeom G) {
  const int H = G.H, W = G.W, Ho = G.Ho, Wo = G.Wo;
  const long long n = (long long)G.C * Ho * Wo;
  const int K = G.kh * G.kw;
  const int cpg = G.C / G.dg;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
    const int wo = (int)(idx % Wo);
    const int ho = (int)((idx / Wo) % Ho);
    const int c = (int)(idx / ((long long)Wo * Ho));
    const int g = c / cpg;
    const int h_in = ho * G.sh - G.ph, w_in = wo * G.sw - G.pw;
    const float* img = im + (size_t)c * H * W;
    const float* o = off + (size_t)g * 2 * K * Ho * Wo;
    const float* m = msk + (size_t)g * K * Ho * Wo;
    float* cp = col + ((size_t)c * K) * Ho * Wo + (size_t)ho * Wo + wo;
    for (int i = 0; i < G.kh; ++i)
      for (int j = 0; j < G.kw; ++j) {
        const int k = i * G.kw + j;
        const float oh = o[((size_t)2 * k * Ho + ho) * Wo + wo];
        const float ow = o[((size_t)(2 * k + 1) * Ho + ho) * Wo + wo];
        const float mk = m[((size_t)k * Ho + ho) * Wo + wo];
        const float h = (float)(h_in + i * G.dh) + oh;
        const float w = (float)(w_in + j * G.dw) + ow;
        float val = 0.f;
        if (dcn_gate(h, w, H, W)) {
          const DcnCorners q = dcn_corners<true>(h, w, H, W);
          const float v1 = q.b1() ? img[(size_t)q.h_low * W + q.w_low] : 0.f;
          const float v2 = q.b2() ? img[(size_t)q.h_low * W + q.w_high] : 0.f;
          const float v3 = q.b3() ? img[(size_t)q.h_high * W + q.w_low] : 0.f;
          const float v4 = q.b4() ? img[(size_t)q.h_high * W + q.w_high] : 0.f;
          val = q.hh * q.hw * v1 + q.hh * q.lw * v2 + q.lh * q.hw * v3 + q.lh * q.lw * v4;
        }
        cp[(size_t)k * Ho * Wo] = val * mk;
      }
  }
}

// C[m][n] = sum_k A(m, k) B(k, n) (+ bias[m] when bias) (+ C[m][n] when acc_c): A(m, k) = A[m sam + k sak],
// B(k, n) = B[k sbk + n sbn]; 64 x 64 tile per workgroup on fp32 MFMA (exact fp32 products, fp32 sums); the
// tile loads follow the unit-stride dimension of each operand so they coalesce.
__global__ __launch_bounds__(256) void k_sgemm(const float* __restrict__ A, long long sam, long long sak,
                                               const float* __restrict__ Bm, long long sbk, long long sbn,
                                               float* __restrict__ Cm, long long ldc, int M, int N, int K, int acc_c,
                                               const float* __restrict__ bias) {
  constexpr int LS = 12;
  __shared__ __attribute__((aligned(16))) float sA[64 * LS];
  __shared__ __attribute__((aligned(16))) float sB[64 * LS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l32 = lane & 31, hf = lane >> 5;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int mi = wv >> 1, ni = wv & 1;
  const bool a_m = sam == 1, b_n = sbn == 1;
  f32x16 acc = f32x16{0};
  for (int k0 = 0; k0 < K; k0 += 8) {
    for (int e = tid; e < 512; e += 256) {
      const int r = a_m ? (e & 63) : (e >> 3), kk = a_m ? (e >> 6) : (e & 7);
      const int m = m0 + r, k = k0 + kk;
      sA[r * LS + kk] = (m < M && k < K) ? A[(long long)m * sam + (long long)k * sak] : 0.f;
      const int c = b_n ? (e & 63) : (e >> 3), kb = b_n ? (e >> 6) : (e & 7);
      const int n = n0 + c, kq = k0 + kb;
      sB[c * LS + kb] = (kq < K && n < N) ? Bm[(long long)kq * sbk + (long long)n * sbn] : 0.f;
    }
    __syncthreads();
    const f32x4 av = ld4(sA + (mi * 32 + l32) * LS + hf * 4);
    const f32x4 bv = ld4(sB + (ni * 32 + l32) * LS + hf * 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = mfma32(av[q], bv[q], acc);
    __syncthreads();
  }
  const int n = n0 + ni * 32 + l32;
  if (n >= N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + mi * 32 + mfma_row(r, lane);
    if (m < M) {
      float* c = Cm + (long long)m * ldc + n;
      const float v = bias ? acc[r] + bias[m] : acc[r];
      *c = acc_c ? *c + v : v;
    }
  }
}

// ------------------------------------------------------------------ forward, STIF shape
// [R][Cc] -> [Cc][R] per batch item (NCHW <-> NHWC of one item), 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void k_transpose(const float* __restrict__ src, float* __restrict__ dst, int R, int Cc) {
  __shared__ float t[32][33];
  const int b = blockIdx.z;
  const float* s = src + (size_t)b * R * Cc;
  float* d = dst + (size_t)b * R * Cc;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + 8 * k, c = c0 + tx;
    t[ty + 8 * k][tx] = (r < R && c < Cc) ? s[(size_t)r * Cc + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + 8 * k, r = r0 + tx;
    if (c < Cc && r < R) d[(size_t)c * R + r] = t[tx][ty + 8 * k];
  }
}

// offset [b][8*18][HW] + mask [b][8*9][HW] (NCHW, reference channel order: offset (g, tap k) at
// g*18 + 2k (+1 for w), mask at g*9 + k; dcn_v2_im2col_cuda.cu:160-167) -> the fused kernel's offmask
// [b][HW][216] = [group][tap][dy, dx, mask], 64 pixels per workgroup through LDS
__global__ __launch_bounds__(256) void k_offmask_nchw(const float* __restrict__ off, const float* __restrict__ msk,
                                                      float* __restrict__ om, int HW) {
  __shared__ float t[64 * 217];
  const int b = blockIdx.y, p0 = blockIdx.x * 64;
  const float* ob = off + (size_t)b * 144 * HW;
  const float* mb = msk + (size_t)b * 72 * HW;
  for (int i = threadIdx.x; i < 216 * 64; i += 256) {
    const int j = i >> 6, px = i & 63, p = p0 + px;   // packed channel j, pixel
    const int g = j / 27, k = (j % 27) / 3, e = j % 3;
    float v = 0.f;
    if (p < HW) v = e < 2 ? ob[(size_t)(g * 18 + 2 * k + e) * HW + p] : mb[(size_t)(g * 9 + k) * HW + p];
    t[px * 217 + j] = v;
  }
  __syncthreads();
  float* ow = om + ((size_t)b * HW + p0) * 216;
  const int npx = min(64, HW - p0);
  for (int i = threadIdx.x; i < npx * 216; i += 256) ow[i] = t[(i / 216) * 217 + i % 216];
}

// nn.Conv2d weight [64][64][3][3] + bias -> the STIF_PACK_PLAIN layout k_dcn<.., 0> reads:
// [chunk 8][tap 9][nt 2][lane 64][4], lane l of nt = cout nt*32 + (l & 31), channels chunk*8 + 4(l >> 5) + e
__global__ __launch_bounds__(256) void k_pack_dcn_w(const float* __restrict__ w, const float* __restrict__ b,
                                                    float* __restrict__ wp, float* __restrict__ bp) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // 8 * 9 * 2 * 64 * 4 = 36864
  if (i < 36864) {
    const int e = i & 3, l = (i >> 2) & 63, nt = (i >> 8) & 1, t = (i >> 9) % 9, c = (i >> 9) / 9;
    const int co = nt * 32 + (l & 31), ci = c * 8 + 4 * (l >> 5) + e;
    wp[i] = w[(co * 64 + ci) * 9 + t];
  }
  if (i < 64) bp[i] = b[i];
}

// ------------------------------------------------------------------ backward (drop-in _ext.dcn_v2_backward)
// sampling position of tap k at output pixel p and its gate (dcn_v2_im2col_cuda.cu:173-176)
STIF_DEV bool dcn_pos(const DcnGeom& G, const float* off, int g, int k, int p, float& h, float& w) {
  const int K = G.kh * G.kw, P = G.Ho * G.Wo;
  const int ho = p / G.Wo, wo = p - ho * G.Wo, i = k / G.kw, j = k - i * G.kw;
  h = (float)(ho * G.sh - G.ph + i * G.dh) + off[((size_t)g * 2 * K + 2 * k) * P + p];
  w = (float)(wo * G.sw - G.pw + j * G.dw) + off[((size_t)g * 2 * K + 2 * k + 1) * P + p];
  return dcn_gate(h, w, G.H, G.W);
}

// grad_offset / grad_mask of one sample (modulated_deformable_col2im_coord, dcn_v2_im2col_cuda.cu:256-327):
// one thread per (group, tap, pixel) computes both coordinate gradients and the mask gradient in one
// pass over the group's channels (the reference runs one thread per offset channel)
__global__ __launch_bounds__(256) void k_dcn_bwd_coord(const float* __restrict__ colg, const float* __restrict__ im,
                                                       const float* __restrict__ off, const float* __restrict__ msk,
                                                       float* __restrict__ goff, float* __restrict__ gmsk, DcnGeom G) {
  const int K = G.kh * G.kw, P = G.Ho * G.Wo, cpg = G.C / G.dg;
  const long long n = (long long)G.dg * K * P;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
    const int p = (int)(idx % P), k = (int)((idx / P) % K), g = (int)(idx / ((long long)P * K));
    float h, w, vh = 0.f, vw = 0.f, vm = 0.f;
    if (dcn_pos(G, off, g, k, p, h, w)) {
      const DcnCorners q = dcn_corners<true>(h, w, G.H, G.W);
      const float lh = q.lh, lw = q.lw, hh = q.hh, hw = q.hw;
      const bool b1 = q.b1(), b2 = q.b2(), b3 = q.b3(), b4 = q.b4();
      const size_t o1 = (size_t)q.h_low * G.W + q.w_low;
      for (int c = 0; c < cpg; ++c) {
        const float* img = im + (size_t)(g * cpg + c) * G.H * G.W;
        const float v1 = b1 ? img[o1] : 0.f, v2 = b2 ? img[o1 + 1] : 0.f;
        const float v3 = b3 ? img[o1 + G.W] : 0.f, v4 = b4 ? img[o1 + G.W + 1] : 0.f;
        const float col = colg[((size_t)(g * cpg + c) * K + k) * P + p];
        vh += col * (-hw * v1 - lw * v2 + hw * v3 + lw * v4);
        vw += col * (-hh * v1 + hh * v2 - lh * v3 + lh * v4);
        vm += col * (hh * hw * v1 + hh * lw * v2 + lh * hw * v3 + lh * lw * v4);
      }
    }
    const float m = msk[((size_t)g * K + k) * P + p];
    goff[((size_t)g * 2 * K + 2 * k) * P + p] = vh * m;
    goff[((size_t)g * 2 * K + 2 * k + 1) * P + p] = vw * m;
    gmsk[((size_t)g * K + k) * P + p] = vm;
  }
}

// grad_input of one sample (modulated_deformable_col2im, dcn_v2_im2col_cuda.cu:197-254): col * mask
// added into the in-bounds bilinear corners (hardware fp32 atomics; the reference uses atomicAdd too)
__global__ __launch_bounds__(256) void k_dcn_bwd_col2im(const float* __restrict__ colg, const float* __restrict__ off,
                                                        const float* __restrict__ msk, float* __restrict__ gin,
                                                        DcnGeom G) {
  const int K = G.kh * G.kw, P = G.Ho * G.Wo, cpg = G.C / G.dg;
  const long long n = (long long)G.C * K * P;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < n; idx += (long long)gridDim.x * 256) {
    const int p = (int)(idx % P), k = (int)((idx / P) % K), c = (int)(idx / ((long long)P * K));
    const int g = c / cpg;
    float h, w;
    if (!dcn_pos(G, off, g, k, p, h, w)) continue;
    const float coef = colg[idx] * msk[((size_t)g * K + k) * P + p];
    const DcnCorners q = dcn_corners<true>(h, w, G.H, G.W);
    float* gi = gin + (size_t)c * G.H * G.W;
    if (q.b1()) unsafeAtomicAdd(gi + (size_t)q.h_low * G.W + q.w_low, q.hh * q.hw * coef);
    if (q.b2()) unsafeAtomicAdd(gi + (size_t)q.h_low * G.W + q.w_high, q.hh * q.lw * coef);
    if (q.b3()) unsafeAtomicAdd(gi + (size_t)q.h_high * G.W + q.w_low, q.lh * q.hw * coef);
    if (q.b4()) unsafeAtomicAdd(gi + (size_t)q.h_high * G.W + q.w_high, q.lh * q.lw * coef);
  }
}

// grad_bias[co] += sum_p grad_out[co][p] of one sample (dcn_v2_cuda.cu:320-326); one workgroup per co
__global__ __launch_bounds__(256) void k_dcn_bwd_bias(const float* __restrict__ go, float* __restrict__ gb, int P) {
  __shared__ float red[256];
  const int co = blockIdx.x;
  float s = 0.f;
  for (int p = threadIdx.x; p < P; p += 256) s += go[(size_t)co * P + p];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) gb[co] += red[0];
}

// ------------------------------------------------------------------ host
bool stif_dcn_shape(int channels, int channels_out, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                    int dg, int height, int width) {
  return channels == 64 && channels_out == 64 && kh == 3 && kw == 3 && sh == 1 && sw == 1 && ph == 1 && pw == 1 &&
         dh == 1 && dw == 1 && dg == 8 && (long long)height * width * 216 * 4 < 0x7fffffffLL;
}
constexpr size_t DCN_WPACK = 36864, DCN_BPACK = 64;

bool dcn_dims(int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int* Ho, int* Wo) {
  *Ho = (H + 2 * ph - (dh * (kh - 1) + 1)) / sh + 1;
  *Wo = (W + 2 * pw - (dw * (kw - 1) + 1)) / sw + 1;
  return *Ho > 0 && *Wo > 0;
}

unsigned dcn_blocks(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 1 << 20); }

// The argument checks of both entry points; they mirror dcn_v2_cuda_forward's / dcn_v2_cuda_backward's
// AT_ASSERTMs (dcn_v2_cuda.cu:60-84, 216-240).  G comes in with the caller's arguments; Ho and Wo are set here.
// ws_size: the entry point's own stif_dcn_v2_*workspace_size.
typedef size_t (*dcn_ws_fn)(int, int, int, int, int, int, int, int, int, int, int, int, int, int);
int dcn_v2_check(const char* name, std::initializer_list<const void*> tensors, int batch, int channels_out,
                 dcn_ws_fn ws_size, const void* workspace, size_t workspace_bytes, DcnGeom& G) {
  auto fail = [&](int code, const char* why) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s: %s", name, why);
    return stif_fail(code, msg);
  };
  for (const void* t : tensors)
    if (!t) return fail(STIF_E_INVALID, "null tensor");
  if (batch < 1 || G.C < 1 || channels_out < 1 || G.kh < 1 || G.kw < 1 || G.sh < 1 || G.sw < 1 || G.dh < 1 ||
      G.dw < 1 || G.dg < 1 || G.C % G.dg)
    return fail(STIF_E_INVALID, "invalid shape arguments");
  if (!dcn_dims(G.H, G.W, G.kh, G.kw, G.sh, G.sw, G.ph, G.pw, G.dh, G.dw, &G.Ho, &G.Wo))
    return fail(STIF_E_INVALID, "empty output");
  const size_t need =
      ws_size(batch, G.C, G.H, G.W, channels_out, G.kh, G.kw, G.sh, G.sw, G.ph, G.pw, G.dh, G.dw, G.dg);
  if (!workspace || workspace_bytes < need) return fail(STIF_E_WORKSPACE, "workspace too small");
  return STIF_OK;
}

}  // namespace

extern "C" size_t stif_dcn_v2_workspace_size(int batch, int channels, int height, int width, int channels_out,
                                             int kernel_h, int kernel_w, int stride_h, int stride_w, int pad_h,
                                             int pad_w, int dilation_h, int dilation_w, int deformable_group) {
  int Ho, Wo;
  if (!dcn_dims(height, width, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, &Ho,
                &Wo))
    return 0;
  if (stif_dcn_shape(channels, channels_out, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                     dilation_w, deformable_group, height, width))
    return ((size_t)batch * height * width * (64 + 216 + 64) + DCN_WPACK + DCN_BPACK) * sizeof(float);
  // generic: the reference's per-sample columns buffer [c * kh * kw][ho * wo] (dcn_v2_cuda.cu:90, one sample)
  return (size_t)channels * kernel_h * kernel_w * Ho * Wo * sizeof(float);
}

extern "C" int stif_dcn_v2_forward(const float* input, const float* weight, const float* bias, const float* offset,
                                   const float* mask, float* output, int batch, int channels, int height, int width,
                                   int channels_out, int kernel_h, int kernel_w, int stride_h, int stride_w,
                                   int pad_h, int pad_w, int dilation_h, int dilation_w, int deformable_group,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  DcnGeom G{channels, height, width, 0, 0, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
            dilation_h, dilation_w, deformable_group};
  if (int rc = dcn_v2_check("dcn_v2_forward", {input, weight, bias, offset, mask, output}, batch, channels_out,
                            stif_dcn_v2_workspace_size, workspace, workspace_bytes, G))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  if (stif_dcn_shape(channels, channels_out, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                     dilation_w, deformable_group, height, width)) {
    // every DCN_sep of LunaTokis: NCHW -> NHWC, offset/mask -> offmask, weights packed on the device,
    // the fused im2col-free kernel (fp32 MFMA), NHWC -> NCHW
    const int HW = height * width;
    float* in_nhwc = (float*)workspace;
    float* om = in_nhwc + (size_t)batch * HW * 64;
    float* out_nhwc = om + (size_t)batch * HW * 216;
    float* wp = out_nhwc + (size_t)batch * HW * 64;
    float* bp = wp + DCN_WPACK;
    hipLaunchKernelGGL(k_transpose, dim3((HW + 31) / 32, 2, batch), dim3(256), 0, st, input, in_nhwc, 64, HW);
    hipLaunchKernelGGL(k_offmask_nchw, dim3((HW + 63) / 64, batch), dim3(256), 0, st, offset, mask, om, HW);
    hipLaunchKernelGGL(k_pack_dcn_w, dim3((unsigned)(DCN_WPACK / 256)), dim3(256), 0, st, weight, bias, wp, bp);
    int rc = stif_check_launch("dcn_v2_forward/layout");
    if (rc) return rc;
    stif_dcn_args a{};
    a.in[0] = in_nhwc;
    a.offmask[0] = om;
    a.w[0] = wp;
    a.bias[0] = bp;
    a.out[0] = out_nhwc;
    a.in_item = (long long)HW * 64;
    a.om_item = (long long)HW * 216;
    a.out_item = (long long)HW * 64;
    a.ngroups = 1;
    a.nitems = batch;
    a.H = height;
    a.W = width;
    a.epi = STIF_EPI_NONE;
    a.flags = 0;
    a.status = nullptr;
    rc = stif_dcn_nhwc(&a, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_transpose, dim3(2, (HW + 31) / 32, batch), dim3(256), 0, st, out_nhwc, output, HW, 64);
    return stif_check_launch("dcn_v2_forward/out");
  }
  // any other shape: im2col + GEMM one sample at a time (dcn_v2_cuda_forward's per-sample columns)
  float* cols = (float*)workspace;
  const int K = channels * kernel_h * kernel_w, N = G.Ho * G.Wo;
  for (int b = 0; b < batch; ++b) {
    hipLaunchKernelGGL(k_im2col, dim3(dcn_blocks((long long)channels * N)), dim3(256), 0, st,
                       input + (size_t)b * channels * height * width,
                       offset + (size_t)b * deformable_group * 2 * kernel_h * kernel_w * N,
                       mask + (size_t)b * deformable_group * kernel_h * kernel_w * N, cols, G);
    int rc = stif_check_launch("dcn_v2_forward/im2col");
    if (rc) return rc;
    // out[m][p] = bias[m] + sum_k weight[m][k] cols[k][p]
    hipLaunchKernelGGL(k_sgemm, dim3((N + 63) / 64, (channels_out + 63) / 64), dim3(256), 0, st, weight, (long long)K,
                       1LL, cols, (long long)N, 1LL, output + (size_t)b * channels_out * N, (long long)N, channels_out,
                       N, K, 0, bias);
    rc = stif_check_launch("dcn_v2_forward/gemm");
    if (rc) return rc;
  }
  return STIF_OK;
}

extern "C" size_t stif_dcn_v2_backward_workspace_size(int batch, int channels, int height, int width,
                                                      int channels_out, int kernel_h, int kernel_w, int stride_h,
                                                      int stride_w, int pad_h, int pad_w, int dilation_h,
                                                      int dilation_w, int deformable_group) {
  (void)batch;
  (void)channels_out;
  (void)deformable_group;
  int Ho, Wo;
  if (!dcn_dims(height, width, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, &Ho,
                &Wo))
    return 0;
  // the reference's per-sample columns buffer (dcn_v2_cuda.cu:242): first the columns gradient, then
  // the forward columns for grad_weight
  return (size_t)channels * kernel_h * kernel_w * Ho * Wo * sizeof(float);
}

extern "C" int stif_dcn_v2_backward(const float* input, const float* weight, const float* bias, const float* offset,
                                    const float* mask, const float* grad_output, float* grad_input, float* grad_offset,
                                    float* grad_mask, float* grad_weight, float* grad_bias, int batch, int channels,
                                    int height, int width, int channels_out, int kernel_h, int kernel_w,
                                    int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w,
                                    int deformable_group, void* workspace, size_t workspace_bytes, void* stream) {
  DcnGeom G{channels, height, width, 0, 0, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
            dilation_h, dilation_w, deformable_group};
  if (int rc = dcn_v2_check("dcn_v2_backward",
                            {input, weight, bias, offset, mask, grad_output, grad_input, grad_offset, grad_mask,
                             grad_weight, grad_bias},
                            batch, channels_out, stif_dcn_v2_backward_workspace_size, workspace, workspace_bytes, G))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const int K = kernel_h * kernel_w, P = G.Ho * G.Wo, CK = channels * K;
  const size_t in_n = (size_t)channels * height * width;
  if (hipMemsetAsync(grad_input, 0, (size_t)batch * in_n * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(grad_weight, 0, (size_t)channels_out * CK * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(grad_bias, 0, (size_t)channels_out * sizeof(float), st) != hipSuccess)
    return stif_fail(STIF_E_LAUNCH, "dcn_v2_backward: memset failed");
  float* cols = (float*)workspace;
  for (int b = 0; b < batch; ++b) {
    const float* in_b = input + (size_t)b * in_n;
    const float* off_b = offset + (size_t)b * deformable_group * 2 * K * P;
    const float* msk_b = mask + (size_t)b * deformable_group * K * P;
    const float* go_b = grad_output + (size_t)b * channels_out * P;
    // columns gradient [c*K + k][p] = sum_co W[co][c*K + k] grad_out[co][p] (dcn_v2_cuda.cu:274-277)
    hipLaunchKernelGGL(k_sgemm, dim3((P + 63) / 64, (CK + 63) / 64), dim3(256), 0, st, weight, 1LL, (long long)CK,
                       go_b, (long long)P, 1LL, cols, (long long)P, CK, P, channels_out, 0, nullptr);
    hipLaunchKernelGGL(k_dcn_bwd_coord, dim3(dcn_blocks((long long)deformable_group * K * P)), dim3(256), 0, st, cols,
                       in_b, off_b, msk_b, grad_offset + (size_t)b * deformable_group * 2 * K * P,
                       grad_mask + (size_t)b * deformable_group * K * P, G);
    hipLaunchKernelGGL(k_dcn_bwd_col2im, dim3(dcn_blocks((long long)CK * P)), dim3(256), 0, st, cols, off_b, msk_b,
                       grad_input + (size_t)b * in_n, G);
    // forward columns, then grad_weight[co][c*K + k] += sum_p grad_out[co][p] cols[c*K + k][p] (:308-315)
    hipLaunchKernelGGL(k_im2col, dim3(dcn_blocks((long long)channels * P)), dim3(256), 0, st, in_b, off_b, msk_b, cols,
                       G);
    hipLaunchKernelGGL(k_sgemm, dim3((CK + 63) / 64, (channels_out + 63) / 64), dim3(256), 0, st, go_b, (long long)P,
                       1LL, cols, 1LL, (long long)P, grad_weight, (long long)CK, channels_out, CK, P, 1, nullptr);
    hipLaunchKernelGGL(k_dcn_bwd_bias, dim3(channels_out), dim3(256), 0, st, go_b, grad_bias, P);
    const int rc = stif_check_launch("dcn_v2_backward");
    if (rc) return rc;
  }
  return STIF_OK;
}
