// The two kernels that touch every gradient byte of a data-parallel step: stif_grad_pack gathers
// the model's fp32 gradient tensors into one contiguous arena in a single launch, and stif_rank_sum adds the R rows of
// an all-gathered slab in rank order.  Both are one pass over about the parameter count in floats: plain loops over a
// fixed grid with 16-byte accesses, no LDS, no atomics, and no floating-point operation besides stif_rank_sum's adds.
#include <cstdint>
#include <cstdio>

#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

namespace {

constexpr int CHUNK = STIF_GRAD_CHUNK;   // floats per chunk: one float4 per lane of a 256-lane workgroup
constexpr int PACK_GRID = 2048, SUM_GRID = 2048;
static_assert(CHUNK == 256 * 4, "one float4 per lane and chunk");

STIF_DEV long long clampll(long long v, long long lo, long long hi) { return min(max(v, lo), hi); }

// Chunk c of the launch belongs to the last segment whose chunk0 is <= c (segments without chunks, n = 0, are passed
// over); chunks past the last segment's cover the arena's tail.  Every workgroup takes a contiguous run of chunks:
// it finds the segment of its first chunk by bisection (c and the table are the same for every lane, so this is
// scalar work) and walks the table forward from there, so that the chain of dependent table loads is paid once per
// workgroup and not once per chunk.  Nothing read from the table is trusted: the chunk count is clamped to what nseg
// segments inside the arena can have, the segment index only grows and stays inside [0, nseg), and a lane stores only
// a whole float4 inside [0, arena_floats) at a non-negative multiple-of-4 offset.  Only the source addresses are the
// caller's word alone.
__global__ __launch_bounds__(256) void k_grad_pack(const stif_grad_seg* __restrict__ segs, int nseg,
                                                   float* __restrict__ arena, long long A) {
  constexpr long long NONE = 0x7fffffffffffffffLL;
  const long long most = A / CHUNK + nseg + 1;
  const stif_grad_seg last = segs[nseg - 1];
  const long long last_r4 = (clampll(last.n, 0, A) + 3) & ~3LL;
  const long long total = clampll(last.chunk0 + (last_r4 + CHUNK - 1) / CHUNK, 0, most);
  const long long end = clampll(last.dst, 0, A) + last_r4;   // A is a multiple of 4, so tail0 is one and <= A
  const long long tail0 = end < A ? ((end + 3) & ~3LL) : A;
  const long long all = total + (A - tail0 + CHUNK - 1) / CHUNK;
  const long long per = (all + gridDim.x - 1) / gridDim.x;
  const long long c0 = blockIdx.x * per, c1 = min(c0 + per, all);
  if (c0 >= c1) return;
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].chunk0 <= c0) lo = mid;
    else hi = mid - 1;
  }
  stif_grad_seg s = segs[lo];
  long long next0 = lo + 1 < nseg ? segs[lo + 1].chunk0 : NONE;   // where the following segment's chunks begin
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (long long c = c0; c < c1; ++c) {
    if (c >= total) {   // the tail: +0.0 up to arena_floats
      const long long d = tail0 + (c - total) * CHUNK + threadIdx.x * 4;
      if (d + 4 <= A) st4(arena + d, zero);
      continue;
    }
    if (c >= next0) {   // at most nseg - 1 advances over the whole walk
      do {
        ++lo;
        next0 = lo + 1 < nseg ? segs[lo + 1].chunk0 : NONE;
      } while (c >= next0);
      s = segs[lo];
    }
    const long long k = c - s.chunk0;
    if (k < 0 || k > most || s.n < 1 || s.dst < 0 || (s.dst & 3)) continue;
    const long long off = k * CHUNK + threadIdx.x * 4;   // floats into the segment
    if (off >= s.n || s.dst > A - 4 - off) continue;     // off < n rounded up to 4, since off is a multiple of 4
    const float* src = s.src + off;
    f32x4 v;
    if (off + 4 <= s.n && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
      v = ld4(src);
    } else {   // a source that is only 4-byte aligned, or the segment's last floats: dwords, +0.0 in the gap
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = off + e < s.n ? src[e] : 0.f;
    }
    st4(arena + s.dst + off, v);
  }
}

// dst[i] = ((slab[0][i] + slab[1][i]) + ...) + slab[R-1][i]: one float4 per lane, the rows four at a time so that the
// loads of a batch are in flight together, the adds one by one in rank order.  There is no multiply to contract
// with; the pragma states the intent all the same.
__global__ __launch_bounds__(256) void k_rank_sum(const float* __restrict__ slab, long long row, int R,
                                                  float* __restrict__ dst, long long n4) {
#pragma clang fp contract(off)
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long long)gridDim.x * 256) {
    const float* p = slab + q * 4;
    f32x4 acc = ld4(p);
    int r = 1;
    for (; r + 4 <= R; r += 4) {
      const f32x4 a = ld4(p + r * row), b = ld4(p + (r + 1) * row), c = ld4(p + (r + 2) * row),
                  d = ld4(p + (r + 3) * row);
      acc = acc + a;
      acc = acc + b;
      acc = acc + c;
      acc = acc + d;
    }
    for (; r < R; ++r) acc = acc + ld4(p + r * row);
    st4(dst + q * 4, acc);
  }
}

bool misaligned(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int fail_as(const char* fn, const char* why) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  return stif_fail(STIF_E_INVALID, msg);
}

}  // namespace

extern "C" int stif_grad_pack(const stif_grad_seg* segs_dev, int nseg, float* arena, long long arena_floats,
                              void* stream) {
  const char* fn = "stif_grad_pack";
  if (!segs_dev || !arena) return fail_as(fn, "null pointer (segs_dev, arena)");
  if (nseg < 1) return fail_as(fn, "nseg must be >= 1");
  if (nseg > STIF_GRAD_MAX_SEGS) return fail_as(fn, "nseg above STIF_GRAD_MAX_SEGS");
  if (misaligned(arena, 15)) return fail_as(fn, "arena must be 16-byte aligned");
  if (misaligned(segs_dev, 7)) return fail_as(fn, "segs_dev must be 8-byte aligned");
  if (arena_floats < 4 || arena_floats % 4) return fail_as(fn, "arena_floats must be a positive multiple of 4");
  if (arena_floats > 0x7fffffffLL) return fail_as(fn, "arena_floats must be <= 2^31 - 1");
  const long long most = 2 * (arena_floats / CHUNK + 1) + nseg;   // segment chunks and tail chunks
  const unsigned grid = (unsigned)(most < PACK_GRID ? most : PACK_GRID);
  hipLaunchKernelGGL(k_grad_pack, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), segs_dev, nseg, arena,
                     arena_floats);
  return stif_check_launch(fn);
}

extern "C" int stif_rank_sum(const float* slab, long long row_floats, int R, float* dst, long long n, void* stream) {
  const char* fn = "stif_rank_sum";
  if (!slab || !dst) return fail_as(fn, "null pointer (slab, dst)");
  if (R < 1 || R > STIF_RANK_SUM_MAX_RANKS) return fail_as(fn, "R must be in 1 .. 64");
  if (n < 4 || n % 4) return fail_as(fn, "n must be a positive multiple of 4");
  if (n > 0x7fffffffLL) return fail_as(fn, "n must be <= 2^31 - 1");
  if (row_floats < n) return fail_as(fn, "row_floats < n");
  if (row_floats % 4) return fail_as(fn, "row_floats must be a multiple of 4 (16-byte rows)");
  if (row_floats > 0x7fffffffLL) return fail_as(fn, "row_floats must be <= 2^31 - 1");
  if (misaligned(slab, 15) || misaligned(dst, 15)) return fail_as(fn, "slab and dst must be 16-byte aligned");
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(slab), d0 = reinterpret_cast<uintptr_t>(dst);
  const uintptr_t s1 = s0 + 4 * (uintptr_t)((R - 1) * row_floats + n), d1 = d0 + 4 * (uintptr_t)n;
  if (d0 < s1 && s0 < d1) return fail_as(fn, "dst overlaps slab");
  const long long n4 = n / 4, blocks = (n4 + 255) / 256;
  const unsigned grid = (unsigned)(blocks < SUM_GRID ? blocks : SUM_GRID);
  hipLaunchKernelGGL(k_rank_sum, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), slab, row_floats, R, dst,
                     n4);
  return stif_check_launch(fn);
}
