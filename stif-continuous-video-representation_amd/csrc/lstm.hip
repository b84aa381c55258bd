// The ConvLSTM cell's gate arithmetic for training (convlstm.py:44-57), forward and backward, on the pre-activation
// map the 128 -> 256 conv writes with STIF_EPI_NONE.  pre is [n][H][W][256] in the reference's
// row order, channel gate * 64 + h with gates i, f, o, g; the states are [n][H][W][64]:
//   c_next = s(f) c_cur + s(i) tanh(g),   h_next = s(o) tanh(c_next).
// The forward keeps nothing but its inputs: the backward recomputes the four gates and tanh(c_next) from pre and
// c_cur (five transcendentals per element against five more maps written and read back).
// Both kernels are elementwise and paced by memory: one thread owns four hidden channels of one pixel, every access
// is a 16-byte vector, the 16 threads of a pixel cover each 256-byte gate row in order.  No atomics.
#include <cstdio>

#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

namespace {

// 1 / (1 + e^-x): e^-x overflows to +inf for x < -88.7 and the quotient is then +0, the limit; never NaN
STIF_DEV float gate_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
STIF_DEV f32x4 sigmoid4(f32x4 v) {
  return {gate_sigmoid(v[0]), gate_sigmoid(v[1]), gate_sigmoid(v[2]), gate_sigmoid(v[3])};
}
// the library's tanhf saturates to +-1 (no e^2x quotient)
STIF_DEV f32x4 tanh4(f32x4 v) { return {tanhf(v[0]), tanhf(v[1]), tanhf(v[2]), tanhf(v[3])}; }

struct GateIdx {
  long long item;
  size_t px;   // pixel of the item
  int q;       // hidden channels 4 q .. 4 q + 3
};
// thread idx of the flat (item, pixel, channel quad) order; per_item = H W 16
STIF_DEV GateIdx gate_idx(long long idx, long long per_item) {
  const long long item = idx / per_item, r = idx - item * per_item;
  return {item, (size_t)(r >> 4), (int)(r & 15)};
}

__global__ __launch_bounds__(256) void k_lstm_gates(const float* __restrict__ pre, const float* __restrict__ c_cur,
                                                    float* __restrict__ h_next, float* __restrict__ c_next,
                                                    long long total, long long per_item, long long pre_item,
                                                    long long c_item, long long h_item, long long cn_item) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const GateIdx t = gate_idx(idx, per_item);
  const float* p = pre + (size_t)t.item * pre_item + t.px * 256 + t.q * 4;
  const size_t so = t.px * 64 + t.q * 4;
  const f32x4 gi = sigmoid4(ld4(p)), gf = sigmoid4(ld4(p + 64)), go = sigmoid4(ld4(p + 128)), gg = tanh4(ld4(p + 192));
  const f32x4 cn = gf * ld4(c_cur + (size_t)t.item * c_item + so) + gi * gg;
  st4(c_next + (size_t)t.item * cn_item + so, cn);
  st4(h_next + (size_t)t.item * h_item + so, go * tanh4(cn));
}

// dc = g_c_next + g_h o (1 - tanh^2 c_next); g_pre (i, f, o, g) = dc g i (1 - i), dc c_cur f (1 - f),
// g_h tanh(c_next) o (1 - o), dc i (1 - g^2); g_c_cur = dc f.  g_h / g_c_next null: zeros; g_c_cur null: not stored.
__global__ __launch_bounds__(256) void k_lstm_gates_bwd(const float* __restrict__ pre, const float* __restrict__ c_cur,
                                                        const float* __restrict__ g_h, const float* __restrict__ g_cn,
                                                        float* __restrict__ g_pre, float* __restrict__ g_cc,
                                                        long long total, long long per_item, long long pre_item,
                                                        long long c_item, long long gh_item, long long gcn_item,
                                                        long long gpre_item, long long gcc_item) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const GateIdx t = gate_idx(idx, per_item);
  const float* p = pre + (size_t)t.item * pre_item + t.px * 256 + t.q * 4;
  const size_t so = t.px * 64 + t.q * 4;
  const f32x4 gi = sigmoid4(ld4(p)), gf = sigmoid4(ld4(p + 64)), go = sigmoid4(ld4(p + 128)), gg = tanh4(ld4(p + 192));
  const f32x4 cc = ld4(c_cur + (size_t)t.item * c_item + so);
  const f32x4 th = tanh4(gf * cc + gi * gg);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 gh = g_h != nullptr ? ld4(g_h + (size_t)t.item * gh_item + so) : zero;
  f32x4 dc = gh * go * (1.0f - th * th);
  if (g_cn != nullptr) dc += ld4(g_cn + (size_t)t.item * gcn_item + so);
  float* gp = g_pre + (size_t)t.item * gpre_item + t.px * 256 + t.q * 4;
  st4(gp, dc * gg * gi * (1.0f - gi));
  st4(gp + 64, dc * cc * gf * (1.0f - gf));
  st4(gp + 128, gh * th * go * (1.0f - go));
  st4(gp + 192, dc * gi * (1.0f - gg * gg));
  if (g_cc != nullptr) st4(g_cc + (size_t)t.item * gcc_item + so, dc * gf);
}

int fail_as(const char* fn, const char* why) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  return stif_fail(STIF_E_INVALID, msg);
}

bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// what both entry points check of their sizes; `blocks` = the grid
int check_sizes(const char* fn, int n, int H, int W, long long* total, long long* per_item, unsigned* blocks) {
  if (n < 1 || H < 1 || W < 1) return fail_as(fn, "n, H, W must be >= 1");
  if ((long long)H * W * 256 * 4 >= 0x7fffffffLL) return fail_as(fn, "item larger than 2 GB (buffer addressing)");
  *per_item = (long long)H * W * 16;
  *total = *per_item * n;
  const long long nb = (*total + 255) / 256;
  if (nb > 0x7fffffffLL) return fail_as(fn, "too many pixels for one grid");
  *blocks = (unsigned)nb;
  return STIF_OK;
}

}  // namespace

extern "C" int stif_lstm_gates_nhwc(const float* pre, const float* c_cur, float* h_next, float* c_next, int n, int H,
                                    int W, long long pre_item, long long c_item, long long h_item, long long cn_item,
                                    void* stream) {
  const char* fn = "stif_lstm_gates_nhwc";
  if (!pre || !c_cur || !h_next || !c_next) return fail_as(fn, "null pointer (pre, c_cur, h_next, c_next)");
  long long total, per_item;
  unsigned blocks;
  if (int rc = check_sizes(fn, n, H, W, &total, &per_item, &blocks)) return rc;
  if (pre_item < 0 || c_item < 0 || h_item < 0 || cn_item < 0) return fail_as(fn, "negative item stride");
  if (misaligned16(pre) || misaligned16(c_cur) || misaligned16(h_next) || misaligned16(c_next) || pre_item % 4 ||
      c_item % 4 || h_item % 4 || cn_item % 4)
    return fail_as(fn, "the maps and their item strides must be 16-byte aligned");
  const long long hw = (long long)H * W;
  if (n > 1 && (h_item < hw * 64 || cn_item < hw * 64))
    return fail_as(fn, "output items overlap (h_item, cn_item < H * W * 64)");
  hipLaunchKernelGGL(k_lstm_gates, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), pre, c_cur, h_next,
                     c_next, total, per_item, pre_item, c_item, h_item, cn_item);
  return stif_check_launch(fn);
}

extern "C" int stif_lstm_gates_bwd_nhwc(const float* pre, const float* c_cur, const float* g_h, const float* g_c_next,
                                        float* g_pre, float* g_c_cur, int n, int H, int W, long long pre_item,
                                        long long c_item, long long gh_item, long long gcn_item, long long gpre_item,
                                        long long gcc_item, void* stream) {
  const char* fn = "stif_lstm_gates_bwd_nhwc";
  if (!pre || !c_cur || !g_pre) return fail_as(fn, "null pointer (pre, c_cur, g_pre)");
  if (!g_h && !g_c_next) return fail_as(fn, "g_h and g_c_next are both null (nothing to propagate)");
  long long total, per_item;
  unsigned blocks;
  if (int rc = check_sizes(fn, n, H, W, &total, &per_item, &blocks)) return rc;
  if (pre_item < 0 || c_item < 0 || (g_h && gh_item < 0) || (g_c_next && gcn_item < 0) || gpre_item < 0 ||
      (g_c_cur && gcc_item < 0))
    return fail_as(fn, "negative item stride");
  if (misaligned16(pre) || misaligned16(c_cur) || misaligned16(g_h) || misaligned16(g_c_next) || misaligned16(g_pre) ||
      misaligned16(g_c_cur) || pre_item % 4 || c_item % 4 || (g_h && gh_item % 4) || (g_c_next && gcn_item % 4) ||
      gpre_item % 4 || (g_c_cur && gcc_item % 4))
    return fail_as(fn, "the maps and their item strides must be 16-byte aligned");
  const long long hw = (long long)H * W;
  if (n > 1 && (gpre_item < hw * 256 || (g_c_cur && gcc_item < hw * 64)))
    return fail_as(fn, "output items overlap (gpre_item < H * W * 256 or gcc_item < H * W * 64)");
  hipLaunchKernelGGL(k_lstm_gates_bwd, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), pre, c_cur, g_h,
                     g_c_next, g_pre, g_c_cur, total, per_item, pre_item, c_item, gh_item, gcn_item, gpre_item,
                     gcc_item);
  return stif_check_launch(fn);
}
