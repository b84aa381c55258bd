// Planar Y'CbCr <-> the model's fp32 RGB planes, on the device: the two ends of the video path (stif_amd.y4m reads
// and writes raw YUV4MPEG2 frames; stif_amd.video.render_y4m chains reader -> stif_yuv_to_rgb -> LunaTokis ->
// stif_rgb_to_yuv -> writer).  Both kernels are one pass over the frames and bandwidth-bound: a thread owns four
// neighbouring luma columns of one (rgb_to_yuv) or two (yuv_to_rgb) rows of chroma boxes, reads / writes them as
// one 16-byte fp32 access per plane and row and one 2- to 8-byte access of samples where the caller's pointers and
// strides allow it (a per-launch decision made on the host), scalar accesses otherwise and at the right edge.
//
// Sample model (ITU-R BT.601 / BT.709, no transfer function: samples are display-referred):
//   Y' = Kr R + Kg G + Kb B,  Cb = (B - Y') / (2 (1 - Kb)),  Cr = (R - Y') / (2 (1 - Kr)),
//   luma sample = yoff + yrange Y', chroma sample = 2^(depth-1) + crange C, with (yoff, yrange, crange) =
//   (16, 219, 224) 2^(depth-8) in limited range and (0, 2^depth - 1, 2^depth - 1) in full range.
// Chroma siting: a chroma sample sits at the centre of its box of luma pixels (the JPEG / MPEG-1 siting) for every
// subsampled layout; see stif.h for what that means for 420mpeg2 / 420paldv streams.
#include "abi_util.h"
#include "stif.h"
#include "stif_common.h"

#include <algorithm>
#include <math.h>

namespace {

template <typename T> using vec4 = T __attribute__((ext_vector_type(4)));
template <typename T> using vec2 = T __attribute__((ext_vector_type(2)));
template <typename T, int N> using vecn = T __attribute__((ext_vector_type(N)));

struct Planes {
  unsigned char* y;                   // planes of frame 0
  unsigned char* u;
  unsigned char* v;
  long long pitch_y, pitch_c, frame;  // bytes
  float* rgb;
  long long item, plane, pitch;       // elements
  int n, W, H, CW, CH, sx, sy;
};

struct ToRgb {
  Planes p;
  float yoff, ysc, coff, csc;   // Y' = (sample - yoff) * ysc, C = (sample - coff) * csc
  float rv, gu, gv, bu;         // R = Y' + rv Cr, G = Y' - gu Cb - gv Cr, B = Y' + bu Cb
};

struct ToYuv {
  Planes p;
  double kr, kg, kb, icb, icr;  // icb = 1 / (2 (1 - Kb)), icr = 1 / (2 (1 - Kr))
  double yoff, yrange, coff, crange, maxv;
};

template <typename T>
STIF_DEV float sample(const unsigned char* row, int x) {
  return (float)reinterpret_cast<const T*>(row)[x];
}

STIF_DEV float unit(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// n planar frames -> fp32 RGB planes in [0, 1].  Chroma: bilinear between the two nearest chroma samples of each
// subsampled axis, weights 3/4 and 1/4, edge samples replicated -- on integer samples of at most 16 bits every
// product and sum of the interpolation is exact in fp32 (20 significant bits), so the only roundings are those of
// the range expansion and the matrix.
// A thread owns 4 luma columns of two chroma rows (4 luma rows in 4:2:0, 2 otherwise): it reads the chroma rows above
// and below (sy) and one column on either side (SX) once for all of its pixels, and neighbouring lanes store
// neighbouring 16-byte pieces of a row.  Two other splits were measured on 8 frames of 1080p:
// a thread per 4 x 1 pixels (16 single-sample chroma loads each: 51 us at 8 bits, 58 us at 10) and a thread per
// 8 x 2 pixels (fewest loads, but a lane's two 16-byte stores per row leave every wave-level store half
// coalesced: 48 / 49 us); this one takes 40 / 42 us.
template <typename T, int SX, bool VEC>
__global__ __launch_bounds__(256) void k_yuv_to_rgb(ToRgb a) {
  const Planes& p = a.p;
  const int ry = 2 << p.sy;                                  // luma rows of a thread
  const int gw = (p.W + 3) >> 2, gh = (p.H + ry - 1) / ry;
  const long long total = (long long)p.n * gh * gw;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int g = (int)(e % gw);
    const long long r = e / gw;
    const int rq = (int)(r % gh);
    const long long i = r / gh;
    const int x0 = g * 4, nx = min(4, p.W - x0);
    const int y0 = rq * ry, ny = min(ry, p.H - y0);
    const bool vec = VEC && nx == 4;
    const long long fo = i * p.frame;

    // chroma rows 2 rq - 1 .. 2 rq + 2 (sy; else the two rows y0, y0 + 1), columns (x0 >> SX) - SX .. + 3 - SX,
    // all clamped into the plane
    const int kc0 = (x0 >> SX) - SX;
    float cu[4][4], cv[4][4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      if (rr >= 2 && !p.sy) continue;
      const int cy = min(max(p.sy ? 2 * rq - 1 + rr : y0 + rr, 0), p.CH - 1);
      const unsigned char* ur = p.u + fo + (long long)cy * p.pitch_c;
      const unsigned char* vr = p.v + fo + (long long)cy * p.pitch_c;
      if (vec && SX) {   // columns 2 g, 2 g + 1 exist (the group's four luma columns do) and are read as a pair
        const vec2<T> tu = reinterpret_cast<const vec2<T>*>(ur)[g], tv = reinterpret_cast<const vec2<T>*>(vr)[g];
        const int lo = max(kc0, 0), hi = min(kc0 + 3, p.CW - 1);
        cu[rr][0] = sample<T>(ur, lo);
        cv[rr][0] = sample<T>(vr, lo);
        cu[rr][1] = (float)tu[0];
        cv[rr][1] = (float)tv[0];
        cu[rr][2] = (float)tu[1];
        cv[rr][2] = (float)tv[1];
        cu[rr][3] = sample<T>(ur, hi);
        cv[rr][3] = sample<T>(vr, hi);
      } else if (vec) {
        const vec4<T> tu = reinterpret_cast<const vec4<T>*>(ur)[g], tv = reinterpret_cast<const vec4<T>*>(vr)[g];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          cu[rr][k] = (float)tu[k];
          cv[rr][k] = (float)tv[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int kx = min(max(kc0 + k, 0), p.CW - 1);
          cu[rr][k] = sample<T>(ur, kx);
          cv[rr][k] = sample<T>(vr, kx);
        }
      }
    }

#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
      if (dy >= ny) continue;
      const int y = y0 + dy;
      const unsigned char* ly = p.y + fo + (long long)y * p.pitch_y;
      float Y[4];
      if (vec) {
        const vec4<T> t = reinterpret_cast<const vec4<T>*>(ly)[g];
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = (float)t[k];
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) Y[k] = k < nx ? sample<T>(ly, x0 + k) : 0.f;
      }
      // vertically: luma row 2 c lies a quarter above the centre of chroma row c = cu[1 + (dy >> 1)], row 2 c + 1 below
      const int c = 1 + (dy >> 1), o = (dy & 1) ? c + 1 : c - 1;
      float u[4], v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        u[k] = p.sy ? 0.75f * cu[c][k] + 0.25f * cu[o][k] : cu[dy & 1][k];
        v[k] = p.sy ? 0.75f * cv[c][k] + 0.25f * cv[o][k] : cv[dy & 1][k];
      }
      f32x4 R, G, B;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float U = u[k], V = v[k];
        if (SX) {   // pixel x0 + k lies in chroma column (x0 >> 1) + (k >> 1) = u[1 + (k >> 1)], a quarter from its centre
          const int cc = 1 + (k >> 1), oo = (k & 1) ? cc + 1 : cc - 1;
          U = 0.75f * u[cc] + 0.25f * u[oo];
          V = 0.75f * v[cc] + 0.25f * v[oo];
        }
        const float yy = (Y[k] - a.yoff) * a.ysc, cb = (U - a.coff) * a.csc, cr = (V - a.coff) * a.csc;
        R[k] = unit(fmaf(a.rv, cr, yy));
        G[k] = unit(fmaf(-a.gv, cr, fmaf(-a.gu, cb, yy)));
        B[k] = unit(fmaf(a.bu, cb, yy));
      }
      float* out = p.rgb + i * p.item + (long long)y * p.pitch + x0;
      if (vec) {
        st4(out, R);
        st4(out + p.plane, G);
        st4(out + 2 * p.plane, B);
      } else {
        for (int k = 0; k < nx; ++k) {
          out[k] = R[k];
          out[p.plane + k] = G[k];
          out[2 * p.plane + k] = B[k];
        }
      }
    }
  }
}

STIF_DEV float round_even(float v) { return rintf(v); }
STIF_DEV double round_even(double v) { return rint(v); }

template <typename T, typename A>
STIF_DEV T quantise(A v, A maxv) {
  const A q = round_even(v);
  return (T)(q < (A)0 ? (A)0 : q > maxv ? maxv : q);
}

// n fp32 RGB frames (unclamped, strided) -> planar frames.  A thread owns four luma columns of one row of chroma
// boxes (1 << sy luma rows): it writes their luma samples and the chroma samples of the boxes they form, each the
// mean of Cb / Cr over the box's pixels that exist, taken before the quantisation.  A is the arithmetic type: fp32
// up to 10 bits, where its rounding error before the quantisation is ~2e-4 of a sample step; fp64 above, where
// fp32 (4e-3 of a step at 16 bits) would move values that are nowhere near a tie.
template <typename T, typename A, bool VEC>
__global__ __launch_bounds__(256) void k_rgb_to_yuv(ToYuv a) {
  const Planes& p = a.p;
  const int gw = (p.W + 3) >> 2, gh = p.sy ? p.CH : p.H;
  const long long total = (long long)p.n * gh * gw;
  const A kr = (A)a.kr, kg = (A)a.kg, kb = (A)a.kb, icb = (A)a.icb, icr = (A)a.icr;
  const A yoff = (A)a.yoff, yrange = (A)a.yrange, coff = (A)a.coff, crange = (A)a.crange, maxv = (A)a.maxv;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int g = (int)(e % gw);
    const long long r = e / gw;
    const int rg = (int)(r % gh);
    const long long i = r / gh;
    const int x0 = g * 4, nx = min(4, p.W - x0);
    const int y0 = rg << p.sy, ny = min(1 << p.sy, p.H - y0);
    const bool vec = VEC && nx == 4;
    const long long fo = i * p.frame;

    A su[4] = {0, 0, 0, 0}, sv[4] = {0, 0, 0, 0};   // Cb, Cr of each column summed over the box rows
    for (int dy = 0; dy < ny; ++dy) {
      const float* s = p.rgb + i * p.item + (long long)(y0 + dy) * p.pitch + x0;
      f32x4 R = {0.f, 0.f, 0.f, 0.f}, G = R, B = R;
      if (vec) {
        R = ld4(s);
        G = ld4(s + p.plane);
        B = ld4(s + 2 * p.plane);
      } else {
        for (int k = 0; k < nx; ++k) {
          R[k] = s[k];
          G[k] = s[p.plane + k];
          B[k] = s[2 * p.plane + k];
        }
      }
      vec4<T> q;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const A rr = (A)unit(R[k]), gg = (A)unit(G[k]), bb = (A)unit(B[k]);
        const A yy = kr * rr + kg * gg + kb * bb;
        su[k] += (bb - yy) * icb;
        sv[k] += (rr - yy) * icr;
        q[k] = quantise<T, A>(yoff + yrange * yy, maxv);
      }
      unsigned char* ly = p.y + fo + (long long)(y0 + dy) * p.pitch_y;
      if (vec) {
        reinterpret_cast<vec4<T>*>(ly)[g] = q;
      } else {
        for (int k = 0; k < nx; ++k) reinterpret_cast<T*>(ly)[x0 + k] = q[k];
      }
    }

    const long long co = fo + (long long)rg * p.pitch_c;   // chroma row: rg = y0 >> sy
    T* pu = reinterpret_cast<T*>(p.u + co);
    T* pv = reinterpret_cast<T*>(p.v + co);
    if (p.sx) {
      vec2<T> qu, qv;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool two = 2 * j + 1 < nx;             // the box's second column exists
        const A inv = (A)1 / (A)((two ? 2 : 1) * ny);
        qu[j] = quantise<T, A>(coff + crange * ((su[2 * j] + (two ? su[2 * j + 1] : (A)0)) * inv), maxv);
        qv[j] = quantise<T, A>(coff + crange * ((sv[2 * j] + (two ? sv[2 * j + 1] : (A)0)) * inv), maxv);
      }
      const int cx0 = x0 >> 1;
      if (vec) {
        reinterpret_cast<vec2<T>*>(pu)[g] = qu;
        reinterpret_cast<vec2<T>*>(pv)[g] = qv;
      } else {
        for (int j = 0; 2 * j < nx; ++j) {
          pu[cx0 + j] = qu[j];
          pv[cx0 + j] = qv[j];
        }
      }
    } else {
      const A inv = (A)1 / (A)ny;
      vec4<T> qu, qv;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        qu[k] = quantise<T, A>(coff + crange * (su[k] * inv), maxv);
        qv[k] = quantise<T, A>(coff + crange * (sv[k] * inv), maxv);
      }
      if (vec) {
        reinterpret_cast<vec4<T>*>(pu)[g] = qu;
        reinterpret_cast<vec4<T>*>(pv)[g] = qv;
      } else {
        for (int k = 0; k < nx; ++k) {
          pu[x0 + k] = qu[k];
          pv[x0 + k] = qv[k];
        }
      }
    }
  }
}

struct Coeffs { double kr, kg, kb, yoff, yrange, coff, crange, maxv; };

// Checks a format and the plane pointers, resolves the zero (dense) strides; align_y / align_c: the alignment in
// samples (a power of two, at most 8) that every row start of the luma / chroma planes of every frame has, for the
// kernels' vector sample accesses.  Returns NULL or the error text.
const char* resolve(const stif_yuv_format* f, const void* y, const void* u, const void* v, int n, Planes* p,
                    Coeffs* c, int* align_y, int* align_c) {
  if (!f) return "format is null";
  if (!y || !u || !v) return "a plane pointer is null";
  if (n < 1 || f->width < 1 || f->height < 1) return "n, width and height must be >= 1";
  if ((f->sub_x | 1) != 1 || (f->sub_y | 1) != 1) return "sub_x and sub_y must be 0 or 1";
  if (f->depth < 8 || f->depth > 16) return "depth must be 8..16";
  if (f->matrix != STIF_YUV_BT601 && f->matrix != STIF_YUV_BT709) return "matrix must be STIF_YUV_BT601 or STIF_YUV_BT709";
  if ((f->full_range | 1) != 1) return "full_range must be 0 or 1";
  const long long bps = f->depth > 8 ? 2 : 1;
  p->W = f->width;
  p->H = f->height;
  p->sx = f->sub_x;
  p->sy = f->sub_y;
  p->CW = (f->width + f->sub_x) >> f->sub_x;
  p->CH = (f->height + f->sub_y) >> f->sub_y;
  p->n = n;
  const long long row_y = p->W * bps, row_c = p->CW * bps;
  if (f->pitch_y < 0 || f->pitch_c < 0 || f->frame_stride < 0) return "negative pitch or frame stride";
  if ((f->pitch_y && f->pitch_y < row_y) || (f->pitch_c && f->pitch_c < row_c)) return "pitch below the row length";
  p->pitch_y = f->pitch_y ? f->pitch_y : row_y;
  p->pitch_c = f->pitch_c ? f->pitch_c : row_c;
  const long long ext_y = (p->H - 1) * p->pitch_y + row_y, ext_c = (p->CH - 1) * p->pitch_c + row_c;
  p->frame = f->frame_stride ? f->frame_stride : p->H * p->pitch_y + 2 * p->CH * p->pitch_c;
  if (n > 1 && p->frame < std::max(ext_y, ext_c)) return "frame stride below the extent of a plane";
  p->y = (unsigned char*)y;
  p->u = (unsigned char*)u;
  p->v = (unsigned char*)v;
  const uintptr_t all = (uintptr_t)y | (uintptr_t)u | (uintptr_t)v | (uintptr_t)p->pitch_y | (uintptr_t)p->pitch_c |
                        (n > 1 ? (uintptr_t)p->frame : 0);
  if (bps == 2 && (all & 1)) return "16-bit samples need 2-byte aligned planes, pitches and frame stride";
  const uintptr_t lum = (uintptr_t)y | (uintptr_t)p->pitch_y | (n > 1 ? (uintptr_t)p->frame : 0);
  const uintptr_t chr = (uintptr_t)u | (uintptr_t)v | (uintptr_t)p->pitch_c | (n > 1 ? (uintptr_t)p->frame : 0);
  *align_y = *align_c = 1;
  while (*align_y < 8 && (lum & (2 * *align_y * bps - 1)) == 0) *align_y *= 2;
  while (*align_c < 8 && (chr & (2 * *align_c * bps - 1)) == 0) *align_c *= 2;

  const bool hd = f->matrix == STIF_YUV_BT709;
  c->kr = hd ? 0.2126 : 0.299;
  c->kb = hd ? 0.0722 : 0.114;
  c->kg = 1.0 - c->kr - c->kb;
  const double up = (double)(1 << (f->depth - 8));
  c->maxv = (double)((1 << f->depth) - 1);
  c->yoff = f->full_range ? 0.0 : 16.0 * up;
  c->yrange = f->full_range ? c->maxv : 219.0 * up;
  c->crange = f->full_range ? c->maxv : 224.0 * up;
  c->coff = 128.0 * up;
  return nullptr;
}

// fp32 RGB planes [n][3][H][W] through element strides: all zero = dense; otherwise rows, planes and items must
// not overlap (the rule of stif_metric_args.pred)
bool rgb_strides(const Planes& p, long long item, long long plane, long long pitch, long long* o_item,
                 long long* o_plane, long long* o_pitch) {
  const long long H = p.H, W = p.W;
  if (item == 0 && plane == 0 && pitch == 0) {
    *o_pitch = W;
    *o_plane = H * W;
    *o_item = 3 * H * W;
    return true;
  }
  const long long rows = (H - 1) * pitch + W;
  if (pitch < W || plane < rows || (p.n > 1 && item < 2 * plane + rows)) return false;
  *o_item = item;
  *o_plane = plane;
  *o_pitch = pitch;
  return true;
}

bool rgb_vec(const Planes& p) {
  return (((uintptr_t)p.rgb & 15) | ((uintptr_t)p.pitch & 3) | ((uintptr_t)p.plane & 3) |
          (p.n > 1 ? (uintptr_t)p.item & 3 : 0)) == 0;
}

unsigned grid_for(long long threads) {
  // grid-stride kernels: enough workgroups to fill the device a few times over, never more than the work
  const long long cap = (long long)stif_num_cus() * 16;
  return (unsigned)std::max<long long>(1, std::min<long long>((threads + 255) / 256, cap));
}

int fail(const char* fn, const char* why) {
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", fn, why);
  return stif_fail(STIF_E_INVALID, msg);
}

}  // namespace

extern "C" int stif_yuv_to_rgb(const stif_yuv_format* fmt, const void* y, const void* u, const void* v, int n,
                               float* out, long long out_item, long long out_plane, long long out_pitch,
                               void* stream) {
  ToRgb a;
  Coeffs c;
  int align_y, align_c;
  if (const char* why = resolve(fmt, y, u, v, n, &a.p, &c, &align_y, &align_c)) return fail("stif_yuv_to_rgb", why);
  if (!out) return fail("stif_yuv_to_rgb", "out is null");
  if (!rgb_strides(a.p, out_item, out_plane, out_pitch, &a.p.item, &a.p.plane, &a.p.pitch))
    return fail("stif_yuv_to_rgb", "out strides: pitch below the row length or overlapping planes / items");
  a.p.rgb = out;
  const bool vec = align_y >= 4 && align_c >= (4 >> a.p.sx) && rgb_vec(a.p);
  a.yoff = (float)c.yoff;
  a.ysc = (float)(1.0 / c.yrange);
  a.coff = (float)c.coff;
  a.csc = (float)(1.0 / c.crange);
  a.rv = (float)(2.0 * (1.0 - c.kr));
  a.bu = (float)(2.0 * (1.0 - c.kb));
  a.gv = (float)(c.kr * 2.0 * (1.0 - c.kr) / c.kg);
  a.gu = (float)(c.kb * 2.0 * (1.0 - c.kb) / c.kg);
  const int ry = 2 << a.p.sy;
  const long long threads = (long long)n * ((a.p.H + ry - 1) / ry) * ((a.p.W + 3) >> 2);
  const dim3 grid(grid_for(threads)), block(256);
  hipStream_t st = (hipStream_t)stream;
  void (*kernel)(ToRgb);
  if (fmt->depth > 8) {
    if (a.p.sx) kernel = vec ? k_yuv_to_rgb<uint16_t, 1, true> : k_yuv_to_rgb<uint16_t, 1, false>;
    else kernel = vec ? k_yuv_to_rgb<uint16_t, 0, true> : k_yuv_to_rgb<uint16_t, 0, false>;
  } else {
    if (a.p.sx) kernel = vec ? k_yuv_to_rgb<uint8_t, 1, true> : k_yuv_to_rgb<uint8_t, 1, false>;
    else kernel = vec ? k_yuv_to_rgb<uint8_t, 0, true> : k_yuv_to_rgb<uint8_t, 0, false>;
  }
  hipLaunchKernelGGL(kernel, grid, block, 0, st, a);
  return stif_check_launch("stif_yuv_to_rgb");
}

extern "C" int stif_rgb_to_yuv(const stif_yuv_format* fmt, const float* rgb, long long rgb_item, long long rgb_plane,
                               long long rgb_pitch, int n, void* y, void* u, void* v, void* stream) {
  ToYuv a;
  Coeffs c;
  int align_y, align_c;
  if (const char* why = resolve(fmt, y, u, v, n, &a.p, &c, &align_y, &align_c)) return fail("stif_rgb_to_yuv", why);
  if (!rgb) return fail("stif_rgb_to_yuv", "rgb is null");
  if (!rgb_strides(a.p, rgb_item, rgb_plane, rgb_pitch, &a.p.item, &a.p.plane, &a.p.pitch))
    return fail("stif_rgb_to_yuv", "rgb strides: pitch below the row length or overlapping planes / items");
  a.p.rgb = const_cast<float*>(rgb);
  const bool vec = align_y >= 4 && align_c >= (4 >> a.p.sx) && rgb_vec(a.p);
  a.kr = c.kr;
  a.kg = c.kg;
  a.kb = c.kb;
  a.icb = 1.0 / (2.0 * (1.0 - c.kb));
  a.icr = 1.0 / (2.0 * (1.0 - c.kr));
  a.yoff = c.yoff;
  a.yrange = c.yrange;
  a.coff = c.coff;
  a.crange = c.crange;
  a.maxv = c.maxv;
  const long long threads = (long long)n * (a.p.sy ? a.p.CH : a.p.H) * ((a.p.W + 3) >> 2);
  const dim3 grid(grid_for(threads)), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (fmt->depth > 10) {
    if (vec) hipLaunchKernelGGL((k_rgb_to_yuv<uint16_t, double, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_rgb_to_yuv<uint16_t, double, false>), grid, block, 0, st, a);
  } else if (fmt->depth > 8) {
    if (vec) hipLaunchKernelGGL((k_rgb_to_yuv<uint16_t, float, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_rgb_to_yuv<uint16_t, float, false>), grid, block, 0, st, a);
  } else {
    if (vec) hipLaunchKernelGGL((k_rgb_to_yuv<uint8_t, float, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_rgb_to_yuv<uint8_t, float, false>), grid, block, 0, st, a);
  }
  return stif_check_launch("stif_rgb_to_yuv");
}
