// The ordered segment sum behind the deterministic training path: stif_segsum.  A scatter-add
// whose contributions were stored once with plain stores (stif_dcn_bwd_contrib, stif_dec_x3_bwd_contrib) and whose
// packed words (key << 32) | entry were sorted becomes a gather: every destination row walks its own segment of the
// sorted list in ascending entry order.  No floating-point atomic exists in this file and no value depends on the
// arrival order of anything.
//
// The value (stif.h states it in full): entries of one destination in ascending entry id, cut into chunks of
// SEG_CHUNK; inside a chunk acc = acc + (w * v) from +0.0f, the multiply and the add both rounded (not fused); the
// row's value is the first chunk's partial plus the following partials in chunk order.  The chunk rule leaves room
// for giving one long list to several waves; this kernel gives a row's float4 to one lane, which walks the whole list.
#include <cstdint>
#include <cstdio>

#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

namespace {

constexpr int SEG_CHUNK = 512, SEG_BATCH = 4;

// acc + (w * v) as two rounded operations: the build contracts a * b + c to one fma by default, and so it does
// __fadd_rn(acc, __fmul_rn(w, v)); the pragma keeps the multiply and the add apart
STIF_DEV f32x4 mul_then_add(f32x4 acc, float w, f32x4 v) {
#pragma clang fp contract(off)
  const f32x4 p = w * v;
  return acc + p;
}
STIF_DEV f32x4 add4(f32x4 a, f32x4 b) {
#pragma clang fp contract(off)
  return a + b;
}

// One lane per float4 of dst: row d = idx / C4, channels 4 (idx % C4) ..; the C4 lanes of a row read the same sorted
// word and weight (one address per row) and consecutive 16 bytes of the source sub-row.  Indices are not trusted: the
// segment bounds are clamped into [0, E], the loop runs over at most E entries, and an entry id >= E is skipped.
template <int C>
__global__ __launch_bounds__(256) void k_segsum(float* __restrict__ dst, const float* __restrict__ src,
                                                long long row_stride, int K, int col0, const float* __restrict__ w,
                                                const long long* __restrict__ sorted, const long long* __restrict__ seg,
                                                long long D, long long E) {
  constexpr int C4 = C / 4;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= D * C4) return;
  const long long d = idx / C4;
  const int c = (int)(idx - d * C4) * 4;
  const long long s0 = min(max(seg[d], 0LL), E), s1 = min(max(seg[d + 1], 0LL), E);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 total = zero, part = zero;
  int in_chunk = 0;
  bool first = true;
  // SEG_BATCH entries at a time: their words, then their weights and sub-rows, are loaded together (an entry that
  // does not count loads entry 0, a valid address, and is dropped), then added one by one in list order -- the walk is
  // a chain of dependent gathers otherwise
  for (long long i = s0; i < s1; i += SEG_BATCH) {
    unsigned e[SEG_BATCH];
    bool ok[SEG_BATCH];
    float wv[SEG_BATCH];
    f32x4 v[SEG_BATCH];
#pragma unroll
    for (int u = 0; u < SEG_BATCH; ++u) {
      const unsigned long long id = (unsigned long long)sorted[min(i + u, s1 - 1)] & 0xffffffffULL;
      ok[u] = i + u < s1 && id < (unsigned long long)E;
      e[u] = ok[u] ? (unsigned)id : 0u;
    }
#pragma unroll
    for (int u = 0; u < SEG_BATCH; ++u) {
      const unsigned sub = e[u] >> 2, row = sub / (unsigned)K, k = sub - row * (unsigned)K;   // 32-bit division
      wv[u] = w[e[u]];
      v[u] = ld4(src + (long long)row * row_stride + ((long long)k * C + col0 + c));
    }
#pragma unroll
    for (int u = 0; u < SEG_BATCH; ++u) {
      if (!ok[u]) continue;
      part = mul_then_add(part, wv[u], v[u]);
      if (++in_chunk == SEG_CHUNK) {
        total = first ? part : add4(total, part);
        first = false, part = zero, in_chunk = 0;
      }
    }
  }
  if (in_chunk || first) total = first ? part : add4(total, part);
  st4(dst + d * C + c, total);
}

bool misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int fail_as(const char* fn, const char* why) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  return stif_fail(STIF_E_INVALID, msg);
}

}  // namespace

extern "C" int stif_segsum(float* dst, const float* src, long long row_stride, int K, int col0, const float* w,
                           const long long* sorted, const long long* seg, long long D, long long E, int C,
                           void* stream) {
  const char* fn = "stif_segsum";
  if (!dst || !src || !w || !sorted || !seg) return fail_as(fn, "null pointer (dst, src, w, sorted, seg)");
  if (C != 8 && C != 64 && C != 192) return fail_as(fn, "C must be 8, 64 or 192");
  if (D < 1 || E < 1 || K < 1) return fail_as(fn, "D, E, K must be >= 1");
  if (E > 0x7fffffffLL) return fail_as(fn, "E must be < 2^31 (entry ids are the low 32 bits of the packed words)");
  if (D > 0x7fffffffLL) return fail_as(fn, "D must be < 2^31 (keys are the high 32 bits of the packed words)");
  if (col0 < 0 || col0 % 4 || row_stride % 4)
    return fail_as(fn, "col0 must be >= 0, col0 and row_stride multiples of 4 (16-byte loads)");
  if (row_stride < (long long)K * C + col0) return fail_as(fn, "row_stride < K * C + col0 (sub-rows leave the row)");
  if (misaligned(dst, 15) || misaligned(src, 15)) return fail_as(fn, "dst and src must be 16-byte aligned");
  if (misaligned(w, 3) || misaligned(sorted, 7) || misaligned(seg, 7))
    return fail_as(fn, "w must be 4-byte, sorted and seg 8-byte aligned");
  const long long blocks = (D * (C / 4) + 255) / 256;
  if (blocks > 0x7fffffffLL) return fail_as(fn, "too many workgroups (D * C / 4 / 256 >= 2^31)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_int<8, 64, 192>(C, [&](auto c) {
    hipLaunchKernelGGL(k_segsum<decltype(c)::value>, dim3((unsigned)blocks), dim3(256), 0, st, dst, src, row_stride, K,
                       col0, w, sorted, seg, D, E);
  });
  return stif_check_launch(fn);
}
