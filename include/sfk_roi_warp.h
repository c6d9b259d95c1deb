/*
 * sfk_roi_warp.h -- C ABI of the random affine augmentation of the v2 part-box trainer (libsfk.so, gfx950), kept beside
 * include/sfk.h, include/sfk_v2.h, include/sfk_roi_pool.h, include/sfk_roi_ragged.h and the other side headers so those headers
 * and the ABI lock stay as they are.  The conventions of sfk_v2.h apply: asynchronous on the caller's stream, no allocation,
 * no synchronisation, a negative sfk_status for a bad descriptor before any launch, no environment reads, safe to capture
 * into a hipGraph.
 *
 * sfk_roi_resize_warp, sfk_roi_resize_pool_warp, sfk_roi_resize_ragged_warp -- sfk_roi_resize, sfk_roi_resize_pool and
 * sfk_roi_resize_ragged can only shift the resized clip by whole pixels (crop, pad).  These are their siblings that sample
 * the resized clip through a 2 x 3 matrix per clip: rotation, scale, shear, flip and translation of the S x S image the
 * resize WOULD write, without writing it -- the v2 clip exists only as the output of a resize of a per-clip box, so one
 * launch evaluates the resize's own interpolant at real-valued positions.  They are to the three resizes what
 * sfk_u8_pool_gather_warp (include/sfk_warp.h) is to the crop gather.  Each descriptor is its sibling's with
 * `const float* warp` in place of crop and pad; the source addressing, the box clamp, lut, fill, a MISSING frame, dst and
 * c_off mean what they mean there.  The three entry points share one kernel; the source addressing is a compile-time switch.
 *
 * Contract.  Every fp32 operation below is individually rounded, in exactly this order (the source is compiled with
 * contraction off); an fma(...) is one fused operation with one rounding.  For clip n, M = warp[n] = (a, b, c, d, e, f) and
 * (x1, y1, x2, y2) = box[n] clamped as sfk_roi_resize clamps it, of extent (bh, bw) = (y2 - y1, x2 - x1).  For output pixel
 * (x, y):
 *     u = (a*x + b*y) + c                        v = (d*x + e*y) + f              position in the RESIZED out_h x out_w image
 *     if !(u >= -0.5 && u <= out_w - 0.5 && v >= -0.5 && v <= out_h - 0.5):   out = 0, nothing is loaded     (a NaN falls here)
 * Otherwise the column taps are sfk_roi_resize's (torch's CPU arithmetic of F.interpolate(bilinear, align_corners=False))
 * evaluated at the real position u in place of the integer output index, with in = bw, out = out_w and scale =
 * (float)in / (float)out; the row taps the same with v, bh and out_h.
 *   antialias = 0:  src = fma(scale, u + 0.5f, -0.5f), 0 if negative;  i0 = min(floor(src), in - 1);
 *                   l1 = min(max(src - i0, 0), 1);  i1 = i0 + (i0 < in - 1);  l0 = 1 - l1;  taps (i0, l0), (i1, l1)
 *   antialias = 1:  _upsample_bilinear2d_aa's mixed float / double arithmetic:
 *                   support = scale >= 1 ? scale : 1;  invscale = scale >= 1 ? (float)(1.0 / (double)scale) : 1
 *                   center = (float)((double)scale * ((double)u + 0.5))
 *                   xmin = max((int)((double)(center - support) + 0.5), 0)
 *                   xsize = min(max(min((int)((double)(center + support) + 0.5), in) - xmin, 0), 2 * ceil(support) + 1)
 *                   w_k = (t = |(float)(((double)((float)(k + xmin) - center) + 0.5) * (double)invscale)|) < 1
 *                         ? (float)(1.0 - (double)t) : 0,   k = 0 .. xsize - 1;   total = ((w_0 + w_1) + ...) in fp32
 *                   taps (min(xmin + k, in - 1), total != 0 ? w_k / total : w_k)
 *                   The support comes from the box / output ratio ALONE: the matrix's own minification does not widen it
 *                   (a matrix that shrinks the image samples the resized image sparsely, as sfk_u8_pool_gather_warp does).
 * The `in == out` shortcuts of the integer resize are dropped; the general formulas give the same values at integer
 * positions.  With byte(r, i) the source byte of row y1 + r, column x1 + i of the frame (the fill byte in a missing frame):
 *     h_r = fma(lut[byte(r, i_k)], wx_k, ... fma(lut[byte(r, i_1)], wx_1, lut[byte(r, i_0)] * wx_0))      per row tap r
 *     out[n][t][ch][y][x] = fma(h_{r_k}, wy_k, ... fma(h_{r_1}, wy_1, h_{r_0} * wy_0))
 * in tap order: the first product rounded on its own, every further tap ONE fused multiply-add (a tap of weight 0 may be
 * skipped: it cannot change the value).  This is the arithmetic and the order of sfk_roi_resize's horizontal and vertical
 * passes as they are compiled (their product-then-sum pairs contract to v_fmac), which the defining property below needs.
 * A bf16 dst is the fp32 result rounded to nearest even.  The edge of the resized image is HARD, there is no blending toward zero: RandomCrop's edge is hard too, and
 * the resized image has no neighbour to blend toward without a second interpolation.
 *
 * The defining property: a row (1, 0, left - pad, 0, 1, top - pad) reproduces the sibling launch with crop = (top, left)
 * and that pad bit for bit, in both antialias modes, both dtypes and all three sources.
 *
 * EVERY table content, finite or not, is memory-safe: the float-to-int conversions happen only after the range test has
 * bounded their arguments, every tap index is clamped into the clamped box before it meets an address, a missing frame reads
 * nothing and a tile whose pixels all fail the range test reads nothing.  The warp, box, index, offset and hw CONTENTS are
 * read on the device when the launch runs, so a captured graph follows new tables written into the same buffers.  All
 * offsets are 64-bit.  No atomics; bit-reproducible.
 *
 * Kernel shape.  One launch; a workgroup of 256 threads owns an output tile of SFK_ROI_WARP_TILE_H x SFK_ROI_WARP_TILE_W
 * pixels of one (n, t) and all c channels.  u and v are monotone in x and in y, rounding included, so their values at the
 * four corners of the tile bound them over the tile; the taps of those bounds bound the tile's source window, whose bytes are
 * staged through LDS as sfk_roi_resize stages its own (aligned dwords for sources whose channels are adjacent).  Tap indices
 * and weights are computed once per pixel, kept in LDS and shared by the channels; lut lives in LDS; stores run along output
 * rows.  A window of more than SFK_ROI_WARP_LDS_BYTES, or a tile with a corner position that is not finite, makes the whole
 * workgroup take its taps from global memory instead -- the same arithmetic, a block-uniform branch.
 *
 * Host-side rejections, with no launch, are the sibling's with its codes (minus pad), plus SFK_ERR_INVALID for a NULL warp;
 * the limits SFK_ROI_MAX_RATIO and SFK_ROI_MAX_C of include/sfk_v2.h hold unchanged.
 */
#ifndef SFK_ROI_WARP_H
#define SFK_ROI_WARP_H

#include "sfk_roi_pool.h"
#include "sfk_roi_ragged.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_ROI_WARP_ABI_VERSION 1
#define SFK_ROI_WARP_TILE_H 16                 /* output rows of one workgroup's tile */
#define SFK_ROI_WARP_TILE_W 32                 /* output columns of it */
#define SFK_ROI_WARP_LDS_BYTES (24 * 1024)     /* the most source bytes a workgroup stages */

typedef struct {
  uint32_t struct_size;      /* sizeof(sfk_roi_warp_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t antialias;         /* 0 | 1 */
  const uint8_t* src;        /* byte (n, t, y, x, c) at src[n*sn + t*st + y*sh + x*sw + c*sc] */
  int64_t sn, st, sh, sw, sc;
  int32_t n, t, h, w, c;
  int32_t out_h, out_w;      /* resized (and sampled) extent */
  const float* lut;          /* device float[256] */
  const int32_t* box;        /* device int32 [n][4] = (x1, y1, x2, y2) */
  const float* warp;         /* device float [n][6] = (a, b, c, d, e, f) of clip n, any values */
  int32_t dst_dtype;         /* SFK_F32 | SFK_BF16 */
  int32_t reserved0;
  void* dst;                 /* element (n, t, c, y, x) at dst[n*dn + t*dt + (c_off + c)*dc + y*dh + x] */
  int64_t dn, dt, dc, dh;
  int32_t c_off, reserved1;
} sfk_roi_warp_desc;

typedef struct {
  uint32_t struct_size;               /* sizeof(sfk_roi_pool_warp_desc) */
  int32_t  antialias;
  const uint8_t* pool;                /* byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch] */
  int64_t  frame_stride, row_stride;
  int32_t  pixel_pitch;
  int32_t  frames;
  int32_t  h, w, c0, c;
  int32_t  n, t;
  const int32_t* index;               /* device int32 [n][t]; outside [0, frames): missing */
  const float*   lut;
  const int32_t* box;
  const float*   warp;                /* device float [n][6] */
  int32_t  fill;                      /* 0..255: the byte every pixel of a missing frame has */
  int32_t  out_h, out_w;
  int32_t  dst_dtype;
  void*    dst;
  int64_t  dn, dt, dc, dh;
  int32_t  c_off;
} sfk_roi_pool_warp_desc;

typedef struct {
  uint32_t struct_size;               /* sizeof(sfk_roi_ragged_warp_desc) */
  int32_t  antialias;
  const uint8_t* arena;               /* 4-byte aligned */
  int64_t  arena_bytes;               /* > 0, a multiple of 4 */
  int32_t  pixel_pitch;
  int32_t  c0, c;
  int32_t  n, t;
  int32_t  max_h, max_w;
  const int64_t* offset;              /* device int64 [n][t]; a frame not wholly inside the arena is missing */
  const int32_t* hw;                  /* device int32 [n][2] = (h_n, w_n) */
  const float*   lut;
  const int32_t* box;                 /* in the rectangle's coordinates */
  const float*   warp;                /* device float [n][6] */
  int32_t  fill;
  int32_t  out_h, out_w;
  int32_t  dst_dtype;
  void*    dst;
  int64_t  dn, dt, dc, dh;
  int32_t  c_off;
} sfk_roi_ragged_warp_desc;

int sfk_roi_warp_abi_version(void);
int sfk_roi_resize_warp(const sfk_roi_warp_desc* d, sfk_stream_t stream);
int sfk_roi_resize_pool_warp(const sfk_roi_pool_warp_desc* d, sfk_stream_t stream);
int sfk_roi_resize_ragged_warp(const sfk_roi_ragged_warp_desc* d, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_ROI_WARP_H */
