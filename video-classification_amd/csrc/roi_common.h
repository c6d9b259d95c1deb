// What roi_resize.hip (sfk_roi_resize, _pool, _ragged) and roi_warp.hip (their _warp siblings, include/sfk_roi_warp.h) share:
// where the source frames lie, torch's tap arithmetic at an integer index, and the staging of a source window's bytes in LDS.
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
