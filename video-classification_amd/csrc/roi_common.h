// What roi_resize.hip (sfk_roi_resize, _pool, _ragged) and roi_warp.hip (their _warp siblings, include/sfk_roi_warp.h) share:
// the host's translation of the pool and arena descriptors and the checks and launch plumbing of the two launchers; on the
// device, where a source frame lies (roi_frame), the box clamp, torch's tap arithmetic at an integer index, and the staging
// of a source window's bytes in LDS.  roi_resize.hip is compiled with the default contraction and roi_warp.hip with
// contraction off: everything here is integer or address code, or names its rounding (__f*_rn, __fmaf_rn), so it means the
// same in both.
#pragma once
#include <math.h>

#include "sfk_common.h"
#include "sfk_roi_pool.h"
#include "sfk_roi_ragged.h"

namespace {

// where the kernel's source frames lie
constexpr int kStacked = 0, kPool = 1, kRagged = 2;

// what the _pool and _ragged entry points add to the descriptor the kernel reads.  Pool: d.src = pool + c0, d.st =
// frame_stride, d.sh = row_stride, d.sw = pixel_pitch, d.sc = 1 and d.sn is unused.  Ragged: d.src = arena + c0, (d.h, d.w) =
// (max_h, max_w), d.sw = pixel_pitch, d.sc = 1 and d.sn, d.st, d.sh are unused (a row is w_n * pixel_pitch bytes)
struct RoiSrc {
  const int32_t* index;
  int frames, fill;
  const int64_t* offset;
  const int32_t* hw;
  int64_t arena_bytes;
};

// ---- host: the six entry points' descriptors -> the sfk_roi_desc and RoiSrc the kernels read

// the fields every descriptor of the family names alike; crop and pad stay zero (the plain entry points set them)
template <typename Desc>
inline sfk_roi_desc roi_desc_of(const Desc& d) {
  sfk_roi_desc r{};
  r.struct_size = sizeof(sfk_roi_desc);
  r.antialias = d.antialias;
  r.n = d.n, r.t = d.t, r.c = d.c;
  r.out_h = d.out_h, r.out_w = d.out_w;
  r.lut = d.lut, r.box = d.box;
  r.dst_dtype = d.dst_dtype, r.dst = d.dst;
  r.dn = d.dn, r.dt = d.dt, r.dc = d.dc, r.dh = d.dh, r.c_off = d.c_off;
  return r;
}

// a strided source under another descriptor type (sfk_roi_warp_desc)
template <typename Desc>
inline sfk_roi_desc roi_from_strided(const Desc& d) {
  sfk_roi_desc r = roi_desc_of(d);
  r.src = d.src;
  r.sn = d.sn, r.st = d.st, r.sh = d.sh, r.sw = d.sw, r.sc = d.sc;
  r.h = d.h, r.w = d.w;
  return r;
}

// the pool's own checks, then its frames as a strided source plus the index table (sfk_roi_pool_desc, sfk_roi_pool_warp_desc)
template <typename Desc>
inline int roi_from_pool(const Desc& d, sfk_roi_desc* r, RoiSrc* p) {
  if (!d.pool || !d.index || d.frames <= 0) return SFK_ERR_INVALID;
  if (d.frame_stride < 0 || d.row_stride < 0 || d.c0 < 0) return SFK_ERR_INVALID;
  if ((int64_t)d.pixel_pitch < (int64_t)d.c0 + d.c) return SFK_ERR_INVALID;
  if (d.fill < 0 || d.fill > 255) return SFK_ERR_INVALID;
  *r = roi_desc_of(d);
  r->src = d.pool + d.c0;
  r->sn = 0, r->st = d.frame_stride, r->sh = d.row_stride, r->sw = d.pixel_pitch, r->sc = 1;
  r->h = d.h, r->w = d.w;
  *p = RoiSrc{d.index, d.frames, d.fill, nullptr, nullptr, 0};
  return SFK_OK;
}

// the arena's own checks, then its descriptor (sfk_roi_ragged_desc, sfk_roi_ragged_warp_desc)
template <typename Desc>
inline int roi_from_ragged(const Desc& d, sfk_roi_desc* r, RoiSrc* p) {
  if (!d.arena || !d.offset || !d.hw || d.max_h <= 0 || d.max_w <= 0) return SFK_ERR_INVALID;
  if (d.arena_bytes <= 0 || (d.arena_bytes & 3) || ((uintptr_t)d.arena & 3) || d.c0 < 0) return SFK_ERR_INVALID;
  if ((int64_t)d.pixel_pitch < (int64_t)d.c0 + d.c) return SFK_ERR_INVALID;
  if (d.fill < 0 || d.fill > 255) return SFK_ERR_INVALID;
  *r = roi_desc_of(d);
  r->src = d.arena + d.c0;
  r->sn = 0, r->st = 0, r->sh = 0, r->sw = d.pixel_pitch, r->sc = 1;
  r->h = d.max_h, r->w = d.max_w;
  *p = RoiSrc{nullptr, 0, d.fill, d.offset, d.hw, d.arena_bytes};
  return SFK_OK;
}

// ---- host: what the two launchers share

// every check of the translated descriptor that roi_resize() and roi_warp() both make (each entry point has checked its own
// struct_size and its own source first).  The launcher's own check (pad, warp) returns SFK_ERR_INVALID and goes before this
// call: every check that preceded it here returns SFK_ERR_INVALID too, so no descriptor's code depends on its place.
inline int roi_check(const sfk_roi_desc* d) {
  if (!d->src || !d->lut || !d->box || !d->dst) return SFK_ERR_INVALID;
  if (d->n <= 0 || d->t <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0 || d->out_h <= 0 || d->out_w <= 0) return SFK_ERR_INVALID;
  if (d->sn < 0 || d->st < 0 || d->sh < 0 || d->sw < 0 || d->sc < 0 || d->dn < 0 || d->dt < 0 || d->dc < 0 || d->dh < 0)
    return SFK_ERR_INVALID;
  if ((d->antialias != 0 && d->antialias != 1) || d->c_off < 0) return SFK_ERR_INVALID;
  if (d->dst_dtype != SFK_F32 && d->dst_dtype != SFK_BF16) return SFK_ERR_INVALID;
  if (d->c > SFK_ROI_MAX_C || (d->sc == 1 && d->sw > 4096)) return SFK_ERR_UNSUPPORTED;
  if ((double)d->h / d->out_h > SFK_ROI_MAX_RATIO || (double)d->w / d->out_w > SFK_ROI_MAX_RATIO) return SFK_ERR_UNSUPPORTED;
  return SFK_OK;
}

// worst-case taps of one axis: the box never exceeds its frame, so its ratio never exceeds frame / out
inline int roi_max_taps(int frame, int out, int aa) {
  const double s = (double)frame / out;
  return aa ? (int)ceil(s > 1.0 ? s : 1.0) * 2 + 1 : 2;
}

// the grid is (tiles, t, n)
inline bool roi_grid_fits(int64_t tiles, const sfk_roi_desc* d) { return tiles <= 0x7fffffff && d->t <= 65535 && d->n <= 65535; }

// the instantiation K<D, SRC> of a kernel template for a destination type and a source kind
#define SFK_ROI_KERNEL(K, dst_dtype, src)                                                                                  \
  ((src) == kRagged ? ((dst_dtype) == SFK_BF16 ? K<bf16_t, kRagged> : K<float, kRagged>)                                    \
   : (src) == kPool ? ((dst_dtype) == SFK_BF16 ? K<bf16_t, kPool> : K<float, kPool>)                                        \
                    : ((dst_dtype) == SFK_BF16 ? K<bf16_t, kStacked> : K<float, kStacked>))

// ---- device

// Where frame (n, t) lies: its extent (the descriptor's, or the clip's own rectangle), its row stride, its first byte, and
// whether it is missing (a missing frame's `first` is the source's own first byte and is never read).  The table rows are
// read once per workgroup and are block-uniform.
struct RoiFrame {
  int H, W;
  int64_t rstride;
  const uint8_t* first;
  bool miss;
};

template <int SRC>
__device__ __forceinline__ RoiFrame roi_frame(const sfk_roi_desc& d, const RoiSrc& p, int n, int t) {
  RoiFrame f{d.h, d.w, d.sh, d.src, false};
  if (SRC == kRagged) {
    // a frame is missing unless it lies in the arena whole: no product here can overflow (h_n * w_n < 2^62, and the bytes
    // left after o are divided, not the rectangle multiplied)
    const int hn = p.hw[2 * (int64_t)n], wn = p.hw[2 * (int64_t)n + 1];
    const int64_t o = p.offset[(int64_t)n * d.t + t];
    f.H = min(max(hn, 1), d.h);
    f.W = min(max(wn, 1), d.w);
    f.miss = o < 0 || hn != f.H || wn != f.W || o > p.arena_bytes || (int64_t)hn * wn > (p.arena_bytes - o) / d.sw;
    f.rstride = (int64_t)f.W * d.sw;
    f.first += f.miss ? 0 : o;                            // 64-bit: an arena may exceed 2^31 bytes
  } else if (SRC == kPool) {
    const int i = p.index[(int64_t)n * d.t + t];
    f.miss = i < 0 || i >= p.frames;
    f.first += (int64_t)(f.miss ? 0 : i) * d.st;          // 64-bit: a pool may exceed 2^31 bytes
  } else {
    f.first += n * d.sn + t * d.st;
  }
  return f;
}

// clip n's box, clamped the way a Python slice clamps it: its corner and its extent, at least one pixel inside H x W
struct RoiBox {
  int x1, y1, bw, bh;
};

__device__ __forceinline__ RoiBox roi_box(const sfk_roi_desc& d, int n, int H, int W) {
  const int32_t* bx = d.box + 4 * (int64_t)n;
  const int x1 = min(max(bx[0], 0), W - 1), y1 = min(max(bx[1], 0), H - 1);
  const int x2 = min(max(bx[2], x1 + 1), W), y2 = min(max(bx[3], y1 + 1), H);
  return RoiBox{x1, y1, x2 - x1, y2 - y1};
}

// Taps of resized index i (0 <= i < out) over a source extent of `in` pixels: up to K (index, weight) pairs, unused ones
// (index = first index, weight 0).  Exactly torch's CPU arithmetic (aten/src/ATen/native/cpu/UpSampleKernel.cpp).
__device__ inline void roi_taps(int i, int in, int out, int aa, int K, int* idx, float* wt) {
  const float scale = (float)in / (float)out;
  if (!aa) {
    int i0, i1;
    float l0, l1;
    if (in == out) {
      i0 = i1 = i;
      l0 = 1.f;
      l1 = 0.f;
    } else {
      float src = __fmaf_rn(scale, (float)i + 0.5f, -0.5f);
      if (src < 0.f) src = 0.f;
      i0 = min((int)floorf(src), in - 1);
      l1 = fminf(fmaxf(__fsub_rn(src, (float)i0), 0.f), 1.f);
      i1 = i0 + (i0 < in - 1 ? 1 : 0);
      l0 = __fsub_rn(1.f, l1);
    }
    idx[0] = i0;
    wt[0] = l0;
    idx[1] = i1;
    wt[1] = l1;
    for (int k = 2; k < K; ++k) { idx[k] = i0; wt[k] = 0.f; }
    return;
  }
  if (in == out) {                 // torch skips the axis: identity
    idx[0] = i;
    wt[0] = 1.f;
    for (int k = 1; k < K; ++k) { idx[k] = i; wt[k] = 0.f; }
    return;
  }
  const float support = scale >= 1.f ? scale : 1.f;
  const int max_k = min((int)ceilf(support) * 2 + 1, K);
  const float invscale = scale >= 1.f ? (float)(1.0 / (double)scale) : 1.f;
  const float center = (float)((double)scale * ((double)i + 0.5));
  const int xmin = max((int)((double)__fsub_rn(center, support) + 0.5), 0);
  int xsize = min((int)((double)__fadd_rn(center, support) + 0.5), in) - xmin;
  xsize = min(max(xsize, 0), max_k);
  float total = 0.f;
  for (int k = 0; k < K; ++k) {
    float w = 0.f;
    if (k < xsize) {
      const float x = fabsf((float)(((double)__fsub_rn((float)(k + xmin), center) + 0.5) * (double)invscale));
      w = x < 1.f ? (float)(1.0 - (double)x) : 0.f;
      total = __fadd_rn(total, w);
    }
    wt[k] = w;
    idx[k] = k < xsize ? xmin + k : xmin;
  }
  if (total != 0.f)
    for (int k = 0; k < xsize; ++k) wt[k] = __fdiv_rn(wt[k], total);
  if (xsize == 0) idx[0] = min(max(xmin, 0), in - 1);
  for (int k = 0; k < K; ++k) idx[k] = min(max(idx[k], 0), in - 1);
}

// Stage nrow rows x ncol pixels x C channels of source bytes, from `base` (the first byte of the window's first pixel) with
// row stride rstride, in LDS as sb[(row * SP + col) * C + ch]; all threads of the workgroup call it.  A missing frame (a
// pool's or an arena's) is staged as dwords of the fill byte (sb is 16-byte aligned) and reads nothing; a source whose
// pixel's channels are adjacent (HWC; a pool's and an arena's frames always are) is read as aligned dwords that each hold at
// least one byte of a pixel of the window, any other byte by byte.
template <int SRC>
__device__ __forceinline__ void roi_stage(unsigned char* sb, int SP, int C, const uint8_t* base, int64_t rstride,
                                          const sfk_roi_desc& d, bool miss, int fill, int nrow, int ncol, int tid, int threads) {
  if (SRC != kStacked && miss) {
    const uint32_t v = 0x01010101u * (uint32_t)fill;
    const int nd = (nrow * SP * C + 3) >> 2;
    for (int q = tid; q < nd; q += threads) reinterpret_cast<uint32_t*>(sb)[q] = v;
  } else if (SRC != kStacked || (d.sc == 1 && d.sw >= C)) {
    // one aligned dword per lane over each row's bytes [first pixel, last pixel's channel C-1]: every dword holds at
    // least one byte of an in-frame pixel of the window
    const int pitch = (int)d.sw;
    const int rbytes = (ncol - 1) * pitch + C;
    for (int r = 0; r < nrow; ++r) {
      const uint8_t* rp = base + (int64_t)r * rstride;
      const uintptr_t a0 = (uintptr_t)rp & ~(uintptr_t)3;
      const int nd = (int)(((uintptr_t)rp + rbytes + 3 - a0) >> 2);
      for (int q = tid; q < nd; q += threads) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(a0 + 4 * (uintptr_t)q);
        // byte offsets within the row window are < SP * pitch: 32-bit, one division per dword, then a walk
        const int off0 = (int)((int64_t)(a0 + 4 * (uintptr_t)q) - (int64_t)(uintptr_t)rp);
        const int o = max(off0, 0);
        int px = o / pitch, ch = o - px * pitch;
#pragma unroll
        for (int b = max(-off0, 0); b < 4; ++b) {
          if (off0 + b >= rbytes) break;
          if (ch < C) sb[(r * SP + px) * C + ch] = (unsigned char)(v >> (8 * b));
          if (++ch == pitch) { ch = 0; ++px; }
        }
      }
    }
  } else {
    const int total = nrow * ncol * C;
    for (int e = tid; e < total; e += threads) {
      const int ch = e % C, px = (e / C) % ncol, r = e / (C * ncol);
      sb[(r * SP + px) * C + ch] = base[(int64_t)r * d.sh + (int64_t)px * d.sw + (int64_t)ch * d.sc];
    }
  }
}

}  // namespace
