// The SIREN MLPs of the decoder for training (feat_imnet, flow_imnet, encode_imnet; SIREN.py:74-79), DESIGN.md
// section 3o: the forward that keeps the pre-activations, and the backward.  One layer is one GEMM on fp32 MFMA over
// row-major matrices in HBM, one row per HR pixel:
//   forward   z_l = a_{l-1} W_l^T + b_l,  a_l = sin(30 z_l) (applied by the next layer's loads; never stored),
//   data      g_z_{l-1} = (g_z_l W_l) * 30 cos(30 z_{l-1})   (the cosine in the epilogue, from the saved z),
//   weights   g_W_l = g_z_l^T a_{l-1},  g_b_l = column sums of g_z_l   (a_{l-1} = sin(30 z_{l-1}) on load).
// The weights are the parameter tensors themselves, row-major [cout_l][cin_l] fp32; nothing is packed.
#include <algorithm>
#include <cstdio>

#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

namespace {

constexpr int ST_T = 64;           // rows of X per workgroup: the row tile (stif.h STIF_SIREN_ROW_TILE)
constexpr int ST_KC = 32;          // K values staged per step
constexpr int ST_LDP = ST_KC + 1;  // LDS row pitch: lane l reads row l & 31, so an odd pitch is conflict-free
constexpr int ST_WG_PER_CU = 2;    // weight pass: workgroups per CU over all 64 x 64 blocks of a layer
static_assert(ST_T == STIF_SIREN_ROW_TILE, "stif.h names the row tile");

// cos(x) with the argument reduction and the polynomials of stif_sin_poly (quadrant reduction by pi/2, 3-part
// Cody-Waite constant exact for |x| < 6400): the quadrant picks the other polynomial and the sign of q + 1.
STIF_DEV float siren_cos_poly(float x) {
  const float qm = fmaf(x, 0.636619772367581343076f, 12582912.0f);
  const float q = qm - 12582912.0f;
  float r = fmaf(q, -1.5703125f, x);
  r = fmaf(q, -4.837512969970703125e-4f, r);
  r = fmaf(q, -7.54978995489188216e-8f, r);
  const float s = r * r;
  const float ps = fmaf(fmaf(fmaf(fmaf(s, 2.75573192e-6f, -1.98412698e-4f), s, 8.33333333e-3f), s, -1.66666667e-1f) * s, r, r);
  const float pc = fmaf(fmaf(fmaf(fmaf(s, 2.48015873e-5f, -1.38888889e-3f), s, 4.16666667e-2f), s, -0.5f), s, 1.0f);
  const int qi = (int)q;
  const float v = (qi & 1) ? ps : pc;
  return ((qi + 1) & 2) ? -v : v;
}

// four consecutive floats of a row of `ncols` valid columns from column `col`; columns past the end read as zero.
// `vec`: the row base and pitch are 16-B aligned (col is a multiple of 4)
STIF_DEV f32x4 ld4_cols(const float* row, int col, int ncols, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (vec && col + 4 <= ncols) return ld4(row + col);
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (col + e < ncols) v[e] = row[col + e];
  return v;
}

// ---- the layer GEMM: C[row][j] = epi(sum_k act(A[row][k]) * B(k, j)) ----
// A workgroup owns ST_T rows and 64 NCB columns; wave w the 32 rows of tile w >> 1 and the 32 columns w & 1 of every
// 64-column block: NCB accumulator tiles.  Per step of ST_KC k values the A tile (with sin(30 .) applied when SIN) and
// the weight tile are staged in LDS, then 16 MFMA k steps.  TRANS = 0: B(k, j) = W[j][k] (forward); TRANS = 1:
// B(k, j) = W[k][j] (data gradient).  EPI 0: + bias[j]; EPI 1: * 30 cos(30 Zp[row][j]); EPI 2: as is, and columns
// ncols .. nstore - 1 of C are written as zeros (the pad columns of g_X).
struct GemmP {
  const float* A; long long lda; int K; int avec;
  const float* W; int ldw;
  const float* bias;
  const float* Zp; long long ldz;
  float* C; long long ldc; int ncols, nstore;
  int n;
};

template <int NCB, bool SIN, bool TRANS, int EPI>
__global__ __launch_bounds__(256) void k_siren_gemm(GemmP p) {
  __shared__ float s_a[ST_T * ST_LDP];
  __shared__ float s_w[64 * NCB * ST_LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rt = wave >> 1, ct = wave & 1, l32 = lane & 31, hf = lane >> 5;
  const long long row0 = (long long)blockIdx.x * ST_T;
  const int j0 = blockIdx.y * 64 * NCB;
  f32x16 acc[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  for (int kc = 0; kc < p.K; kc += ST_KC) {
    __syncthreads();   // the previous step's reads are done
    {
      const int r = tid >> 3, c4 = tid & 7;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = r + 32 * i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + row < p.n) v = ld4_cols(p.A + (size_t)(row0 + row) * p.lda, kc + c4 * 4, p.K, p.avec != 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) s_a[row * ST_LDP + c4 * 4 + e] = SIN ? stif_sin_poly(30.f * v[e]) : v[e];
      }
    }
    if (!TRANS) {
      const int r = tid >> 3, k4 = (tid & 7) * 4;
#pragma unroll
      for (int i = 0; i < 2 * NCB; ++i) {
        const int jj = r + 32 * i, j = j0 + jj;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = kc + k4 + e;
          s_w[jj * ST_LDP + k4 + e] = (j < p.ncols && k < p.K) ? p.W[(size_t)j * p.ldw + k] : 0.f;
        }
      }
    } else {
      const int kk0 = tid >> 6, jl = tid & 63;
#pragma unroll
      for (int c = 0; c < NCB; ++c) {
        const int jj = c * 64 + jl, j = j0 + jj;
#pragma unroll
        for (int i = 0; i < ST_KC / 4; ++i) {
          const int kk = kk0 + 4 * i, k = kc + kk;
          s_w[jj * ST_LDP + kk] = (j < p.ncols && k < p.K) ? p.W[(size_t)k * p.ldw + j] : 0.f;
        }
      }
    }
    __syncthreads();
    const float* ap = s_a + (rt * 32 + l32) * ST_LDP + hf;
    const float* wp = s_w + (ct * 32 + l32) * ST_LDP + hf;
#pragma unroll 4
    for (int ks = 0; ks < ST_KC / 2; ++ks) {
      const float a = ap[2 * ks];
#pragma unroll
      for (int c = 0; c < NCB; ++c) acc[c] = mfma32(a, wp[c * 64 * ST_LDP + 2 * ks], acc[c]);
    }
  }

#pragma unroll
  for (int c = 0; c < NCB; ++c) {
    const int j = j0 + c * 64 + ct * 32 + l32;
    const float bj = (EPI == 0 && j < p.ncols) ? p.bias[j] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = row0 + rt * 32 + mfma_row(r, lane);
      if (row >= p.n) continue;
      if (j < p.ncols) {
        float v = acc[c][r];
        if (EPI == 0) v += bj;
        if (EPI == 1) v *= 30.f * siren_cos_poly(30.f * p.Zp[(size_t)row * p.ldz + j]);
        p.C[(size_t)row * p.ldc + j] = v;
      } else if (EPI == 2 && j < p.nstore) {
        p.C[(size_t)row * p.ldc + j] = 0.f;
      }
    }
  }
}

template <int NCB, bool SIN, bool TRANS, int EPI>
int launch_gemm(const char* fn, const GemmP& p, hipStream_t st) {
  const int span = EPI == 2 ? p.nstore : p.ncols;
  const dim3 grid((unsigned)(((long long)p.n + ST_T - 1) / ST_T), (unsigned)((span + 64 * NCB - 1) / (64 * NCB)));
  hipLaunchKernelGGL((k_siren_gemm<NCB, SIN, TRANS, EPI>), grid, dim3(256), 0, st, p);
  return stif_check_launch(fn);
}

// ---- the weight pass: one 64 x 64 block (cout block cb, cin block ib) of g_W_l per workgroup column ----
// stif_conv1x1_wgrad's scheme for one x map, generalised to any block of a [co_n][ci_n] layer: workgroup (g, blk)
// takes the 64-row chunks g, g + G, ... of the rows, stages the 64 g_z columns and the 64 activation columns of its
// block in LDS (rows past n and columns past the layer's are zeros; sin(30 .) applied to the activations on load when
// SIN) and contracts over the rows: D[co 32][ci 32] += g_z[row pair][co] * a[row pair][ci].  Every workgroup writes one
// partial [64][64] + 64 column sums; k_siren_wgrad_reduce adds the G partials of a block in a fixed order.
constexpr int ST_PART = 64 * 64 + 64;

struct WgradP {
  const float* G; long long ldg; int co_n; int gvec;
  const float* A; long long lda; int ci_n; int avec;
  float* ws;
  int n, nchunks, nci_blk;
};

template <bool SIN>
__global__ __launch_bounds__(256) void k_siren_wgrad(WgradP p) {
  __shared__ __attribute__((aligned(16))) float s_g[ST_T * 64];
  __shared__ __attribute__((aligned(16))) float s_x[ST_T * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cot = wave >> 1, cit = wave & 1, l32 = lane & 31, hf = lane >> 5;
  const int blk = blockIdx.y, cb = blk / p.nci_blk, ib = blk - cb * p.nci_blk;
  const int co0 = cb * 64, ci0 = ib * 64;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float bsum = 0.f;   // sum of this lane's g_z values: column co0 + cot * 32 + l32, rows of parity hf

  const int c4 = tid & 15;
  for (int ch = blockIdx.x; ch < p.nchunks; ch += gridDim.x) {
    __syncthreads();   // the previous chunk's reads are done
#pragma unroll
    for (int k = 0; k < ST_T / 16; ++k) {
      const int r = (tid >> 4) + 16 * k;
      const long long row = (long long)ch * ST_T + r;
      f32x4 g = {0.f, 0.f, 0.f, 0.f}, x = {0.f, 0.f, 0.f, 0.f};
      if (row < p.n) {
        g = ld4_cols(p.G + (size_t)row * p.ldg, co0 + c4 * 4, p.co_n, p.gvec != 0);
        x = ld4_cols(p.A + (size_t)row * p.lda, ci0 + c4 * 4, p.ci_n, p.avec != 0);
        if (SIN) {
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = (ci0 + c4 * 4 + e < p.ci_n) ? stif_sin_poly(30.f * x[e]) : 0.f;
        }
      }
      st4(s_g + r * 64 + c4 * 4, g);
      st4(s_x + r * 64 + c4 * 4, x);
    }
    __syncthreads();
    const float* ap = s_g + hf * 64 + cot * 32 + l32;
    const float* bp = s_x + hf * 64 + cit * 32 + l32;
#pragma unroll 4
    for (int ks = 0; ks < ST_T / 2; ++ks) {
      const float a = ap[ks * 128];
      bsum += a;
      acc = mfma32(a, bp[ks * 128], acc);
    }
  }

  float* part = p.ws + ((size_t)blk * gridDim.x + blockIdx.x) * ST_PART;
#pragma unroll
  for (int r = 0; r < 16; ++r) part[(cot * 32 + mfma_row(r, lane)) * 64 + cit * 32 + l32] = acc[r];
  const float other = __shfl_xor(bsum, 32);
  if (cit == 0 && hf == 0) part[64 * 64 + cot * 32 + l32] = bsum + other;
}

// g_W / g_b = the G partials of every block summed in a fixed order (k_c1_wgrad_reduce's: sixteen interleaved
// index-ordered slices, then the slices in order); the order is a function of G alone.  grid (ST_PART / 16, blocks).
__global__ __launch_bounds__(256) void k_siren_wgrad_reduce(const float* __restrict__ ws, int G, int nci_blk, int co_n,
                                                            int ci_n, float* __restrict__ gw, float* __restrict__ gb) {
  __shared__ float s_sum[16][16];
  const int e = threadIdx.x & 15, sl = threadIdx.x >> 4, idx = blockIdx.x * 16 + e;
  const int blk = blockIdx.y, cb = blk / nci_blk, ib = blk - cb * nci_blk;
  const float* base = ws + (size_t)blk * G * ST_PART;
  float s = 0.f;
#pragma unroll 8
  for (int g = sl; g < G; g += 16) s += base[(size_t)g * ST_PART + idx];
  s_sum[sl][e] = s;
  __syncthreads();
  if (sl != 0) return;
  float t = s_sum[0][e];
#pragma unroll
  for (int k = 1; k < 16; ++k) t += s_sum[k][e];
  if (idx < 64 * 64) {
    const int co = cb * 64 + (idx >> 6), ci = ib * 64 + (idx & 63);
    if (co < co_n && ci < ci_n) gw[(size_t)co * ci_n + ci] = t;
  } else {
    const int co = cb * 64 + idx - 64 * 64;
    if (ib == 0 && co < co_n) gb[co] = t;
  }
}

int wgrad_blocks(int co_n, int ci_n) { return ((co_n + 63) / 64) * ((ci_n + 63) / 64); }
long long row_chunks(int n) { return ((long long)n + ST_T - 1) / ST_T; }
// the launch rule of the weight pass: a function of the row count, the layer's shape and the CU count alone
int wgrad_grid(int n, int co_n, int ci_n) {
  const long long per = std::max(1, ST_WG_PER_CU * stif_num_cus() / wgrad_blocks(co_n, ci_n));
  return (int)std::min<long long>(row_chunks(n), per);
}

int fail_as(const char* fn, const char* why) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  return stif_fail(STIF_E_INVALID, msg);
}
bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

struct Net {
  int nl;            // layers, the final linear one included
  int cin[5], cout[5], zoff[5], zw;
};

// the checks shared by the forward and the backward; fills `net`
const char* check_common(const stif_siren_args* pa, Net& net) {
  if (!pa) return "null args";
  const stif_siren_args& a = *pa;
  if (a.n < 1) return "n must be >= 1";
  if (a.nsine != 3 && a.nsine != 4) return "nsine must be 3 or 4";
  static const int want[4] = {64, 64, 256, 256};
  for (int l = 0; l < 4; ++l)
    if (a.width[l] != (l < a.nsine ? want[l] : 0)) return "unsupported widths ((64, 64, 256) or (64, 64, 256, 256))";
  if (a.cout != 64 && a.cout != 4 && a.cout != 3) return "cout must be 64, 4 or 3";
  if (a.cin < 1 || a.cin > STIF_SIREN_MAX_CIN) return "cin outside [1, 528]";
  const int kp = (a.cin + 7) / 8 * 8;
  if (!a.x || !a.z) return "null pointer (x, z)";
  if (a.x_stride < kp || a.x_stride % 8) return "x_stride must be a multiple of 8 and at least cin rounded up to 8";
  if (misaligned16(a.x) || misaligned16(a.z)) return "x and z must be 16-byte aligned";
  net.nl = a.nsine + 1;
  net.zw = 0;
  for (int l = 0; l < net.nl; ++l) {
    if (!a.w[l] || !a.b[l]) return "null pointer (w[l], b[l])";
    net.cin[l] = l == 0 ? a.cin : a.width[l - 1];
    net.cout[l] = l < a.nsine ? a.width[l] : a.cout;
    net.zoff[l] = net.zw;
    if (l < a.nsine) net.zw += a.width[l];
  }
  return nullptr;
}

}  // namespace

extern "C" int stif_siren_wgrad_grid(int n, int cout, int cin) {
  if (n < 1 || cout < 1 || cout > 256 || cin < 1 || cin > STIF_SIREN_MAX_CIN) return 0;
  return wgrad_grid(n, cout, cin);
}

extern "C" size_t stif_siren_bwd_workspace_size(int n, int nsine) {
  if (n < 1 || (nsine != 3 && nsine != 4)) return 0;
  const size_t zw = nsine == 3 ? 384 : 640;
  // g_z of every sine layer, then the partials of the layer with the most workgroups: blocks x grid is at most
  // max(blocks, ST_WG_PER_CU CUs) and no layer has more than 16 blocks (256 x 256), 9 for the 525 inputs
  const size_t wgs = (size_t)std::max(16, ST_WG_PER_CU * stif_num_cus());
  return ((size_t)n * zw + wgs * ST_PART) * sizeof(float);
}

extern "C" int stif_siren_fwd(const stif_siren_args* pa, void* stream) {
  const char* fn = "stif_siren_fwd";
  Net net;
  if (const char* why = check_common(pa, net)) return fail_as(fn, why);
  const stif_siren_args& a = *pa;
  if (!a.y) return fail_as(fn, "null pointer (y)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  for (int l = 0; l < net.nl; ++l) {
    GemmP p = {};
    p.A = l == 0 ? a.x : a.z + net.zoff[l - 1];
    p.lda = l == 0 ? a.x_stride : net.zw;
    p.K = net.cin[l];
    p.avec = 1;
    p.W = a.w[l], p.ldw = net.cin[l], p.bias = a.b[l];
    const bool last = l == net.nl - 1;
    p.C = last ? a.y : a.z + net.zoff[l];
    p.ldc = last ? a.cout : net.zw;
    p.ncols = p.nstore = net.cout[l];
    p.n = a.n;
    int rc;
    if (l == 0) rc = launch_gemm<1, false, false, 0>(fn, p, st);
    else if (net.cout[l] == 256) rc = launch_gemm<4, true, false, 0>(fn, p, st);
    else rc = launch_gemm<1, true, false, 0>(fn, p, st);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int stif_siren_bwd(const stif_siren_args* pa, void* stream) {
  const char* fn = "stif_siren_bwd";
  Net net;
  if (const char* why = check_common(pa, net)) return fail_as(fn, why);
  const stif_siren_args& a = *pa;
  if (!a.g_y) return fail_as(fn, "null pointer (g_y)");
  for (int l = 0; l < net.nl; ++l)
    if (!a.g_w[l] || !a.g_b[l]) return fail_as(fn, "null pointer (g_w[l], g_b[l])");
  const int kp = (a.cin + 7) / 8 * 8;
  if (a.g_x && (a.gx_stride < kp || a.gx_stride % 8))
    return fail_as(fn, "gx_stride must be a multiple of 8 and at least cin rounded up to 8");
  if (a.g_x && misaligned16(a.g_x)) return fail_as(fn, "g_x must be 16-byte aligned");
  if (!a.workspace || a.workspace_bytes < stif_siren_bwd_workspace_size(a.n, a.nsine))
    return fail_as(fn, "workspace too small (stif_siren_bwd_workspace_size)");
  if (misaligned16(a.workspace)) return fail_as(fn, "workspace not 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* gz = static_cast<float*>(a.workspace);            // [n][zw], the layout of z
  float* part = gz + (size_t)a.n * net.zw;
  const int nchunks = (int)row_chunks(a.n);
  for (int l = net.nl - 1; l >= 0; --l) {
    const bool last = l == net.nl - 1;
    const float* g = last ? a.g_y : gz + net.zoff[l];
    const long long ldg = last ? a.cout : net.zw;
    const int gvec = (ldg % 4 == 0 && !misaligned16(g)) ? 1 : 0;
    {
      WgradP w = {};
      w.G = g, w.ldg = ldg, w.co_n = net.cout[l], w.gvec = gvec;
      w.A = l == 0 ? a.x : a.z + net.zoff[l - 1];
      w.lda = l == 0 ? a.x_stride : net.zw;
      w.ci_n = net.cin[l], w.avec = 1;
      w.ws = part, w.n = a.n, w.nchunks = nchunks, w.nci_blk = (net.cin[l] + 63) / 64;
      const int blocks = wgrad_blocks(net.cout[l], net.cin[l]), G = wgrad_grid(a.n, net.cout[l], net.cin[l]);
      if (l == 0) hipLaunchKernelGGL(k_siren_wgrad<false>, dim3(G, blocks), dim3(256), 0, st, w);
      else hipLaunchKernelGGL(k_siren_wgrad<true>, dim3(G, blocks), dim3(256), 0, st, w);
      if (int rc = stif_check_launch("stif_siren_bwd (weights)")) return rc;
      hipLaunchKernelGGL(k_siren_wgrad_reduce, dim3(ST_PART / 16, blocks), dim3(256), 0, st, part, G, w.nci_blk,
                         net.cout[l], net.cin[l], a.g_w[l], a.g_b[l]);
      if (int rc = stif_check_launch("stif_siren_bwd (reduce)")) return rc;
    }
    if (l == 0 && !a.g_x) break;
    GemmP p = {};
    p.A = g, p.lda = ldg, p.K = net.cout[l], p.avec = gvec;
    p.W = a.w[l], p.ldw = net.cin[l];
    p.n = a.n;
    int rc;
    if (l == 0) {
      p.C = a.g_x, p.ldc = a.gx_stride, p.ncols = a.cin, p.nstore = kp;
      rc = launch_gemm<4, false, true, 2>(fn, p, st);
    } else {
      p.Zp = a.z + net.zoff[l - 1], p.ldz = net.zw;
      p.C = gz + net.zoff[l - 1], p.ldc = net.zw, p.ncols = p.nstore = net.cin[l];
      rc = net.cin[l] == 256 ? launch_gemm<4, false, true, 1>(fn, p, st) : launch_gemm<1, false, true, 1>(fn, p, st);
    }
    if (rc) return rc;
  }
  return 0;
}
