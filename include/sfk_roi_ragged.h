/*
 * sfk_roi_ragged.h -- C ABI of the v2 part-box trainer's box-cropped device-resident train set (libsfk.so, gfx950), kept
 * beside include/sfk.h, include/sfk_v2.h, include/sfk_roi_pool.h and the other side headers so those headers and the ABI lock
 * stay as they are.  The conventions of sfk_v2.h apply: asynchronous on the caller's stream, no allocation, no
 * synchronisation, a negative sfk_status for a bad descriptor before any launch, no environment reads, safe to capture into a
 * hipGraph.
 *
 * sfk_roi_resize_ragged -- sfk_roi_resize (include/sfk_v2.h) reading its source frames from a BYTE ARENA in which every
 * clip's frames are stored cropped to that clip's own rectangle: a clip never reads outside its part box, so a video need
 * only keep the union of its frames' boxes, and frames of different clips then differ in shape.  Each frame is h_n x w_n
 * pixels of pixel_pitch contiguous bytes, rows packed (row stride w_n * pixel_pitch), at any byte offset.  For clip n and
 * frame t let o = offset[n][t] and (h_n, w_n) = hw[n]:
 *     valid = o >= 0 && 1 <= h_n <= max_h && 1 <= w_n <= max_w && o + h_n*w_n*pixel_pitch <= arena_bytes      (64-bit)
 *     valid:      v[y][x] = lut[arena[o + (y*w_n + x)*pixel_pitch + c0 + ch]]
 *     otherwise:  v[y][x] = lut[fill]        (a MISSING frame: the constant image of byte fill; the arena is not read)
 * and everything from there on is sfk_roi_resize's contract word for word with (h, w) = (h_n, w_n): (x1, y1, x2, y2) =
 * box[n], in the rectangle's coordinates, clamped the way a Python slice clamps it, r = F.interpolate(v[y1:y2, x1:x2],
 * (out_h, out_w), bilinear, align_corners=False, antialias) in torch's CPU arithmetic, the crop shift (top[n] - pad,
 * left[n] - pad) with zeros outside the resized image, a bf16 destination rounded to nearest even, and element
 * (n, t, ch, y, x) at dst[n*dn + t*dt + (c_off + ch)*dc + y*dh + x].  Where hw[n] itself is out of range (every frame of
 * that clip is then missing) the box is clamped into (min(max(h_n, 1), max_h), min(max(w_n, 1), max_w)).  The result is
 * bit-identical to sfk_roi_resize run clip by clip on that clip's frames stacked as (1, t, h_n, w_n, pixel_pitch), a missing
 * frame stacked as fill bytes: the entry points share one kernel, whose source addressing is a compile-time switch.
 *
 * Every value of offset, hw, box and crop is memory-safe: the validity test above is made in 64-bit arithmetic that cannot
 * overflow, a box is clamped into its rectangle before it meets an address, and every LDS index is clamped to what was
 * staged.  The source bytes are read as aligned dwords that each hold at least one byte of a pixel of a valid frame; as
 * arena is 4-byte aligned and arena_bytes a multiple of 4, every load lies inside [arena, arena + arena_bytes).  The
 * CONTENTS of offset, hw, box and crop are read on the device when the launch runs, so a captured graph follows new tables
 * written into the same buffers.  hw[n] and offset[n][t] are read once per workgroup.  No atomics; bit-reproducible.
 *
 * Host-side rejections, with no launch: everything sfk_roi_resize_pool rejects, with its codes, the frame extent being
 * (max_h, max_w) -- SFK_ERR_INVALID for a wrong struct_size, a NULL arena, offset, hw, lut, box or dst, arena_bytes <= 0 or
 * not a multiple of 4, an arena that is not 4-byte aligned, a non-positive n, t, max_h, max_w, c, out_h or out_w, a negative
 * c0, dn, dt, dc or dh, pixel_pitch < c0 + c, fill outside 0..255, antialias not 0 or 1, pad < 0, c_off < 0 or a dst dtype
 * that is neither f32 nor bf16; SFK_ERR_UNSUPPORTED for c > SFK_ROI_MAX_C, pixel_pitch > 4096, a worst-case reduction
 * max_h/out_h or max_w/out_w above SFK_ROI_MAX_RATIO, or a tile that does not fit the LDS.  The tile is sized from
 * (max_h, max_w): pass the largest rectangle of the batch, not of the data set.
 */
#ifndef SFK_ROI_RAGGED_H
#define SFK_ROI_RAGGED_H

#include "sfk_v2.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_ROI_RAGGED_ABI_VERSION 1

typedef struct {
  uint32_t struct_size;               /* sizeof(sfk_roi_ragged_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t  antialias;                 /* 0 | 1: F.interpolate(..., antialias=) */
  const uint8_t* arena;               /* 4-byte aligned; byte (y, x, ch) of a frame at offset o: arena[o + (y*w_n + x)*pixel_pitch + c0 + ch] */
  int64_t  arena_bytes;               /* > 0, a multiple of 4 */
  int32_t  pixel_pitch;               /* bytes, >= c0 + c */
  int32_t  c0, c;                     /* first channel, channels */
  int32_t  n, t;                      /* clips, frames per clip */
  int32_t  max_h, max_w;              /* no stored rectangle is larger; sizes the tile */
  const int64_t* offset;              /* device int64 [n][t]: byte offset of the frame's first byte; negative: missing */
  const int32_t* hw;                  /* device int32 [n][2] = (h_n, w_n), the stored rectangle of every frame of clip n */
  const float*   lut;                 /* device float[256]: the value of byte u */
  const int32_t* box;                 /* device int32 [n][4] = (x1, y1, x2, y2), Python slice bounds in the rectangle */
  const int32_t* crop;                /* device int32 [n][2] = (top, left), or NULL (no crop) */
  int32_t  pad;                       /* crop padding; unused when crop == NULL */
  int32_t  fill;                      /* 0..255: the byte every pixel of a missing frame has */
  int32_t  out_h, out_w;              /* resized extent */
  int32_t  dst_dtype;                 /* SFK_F32 | SFK_BF16 */
  void*    dst;                       /* element (n, t, ch, y, x) at dst[n*dn + t*dt + (c_off + ch)*dc + y*dh + x] */
  int64_t  dn, dt, dc, dh;
  int32_t  c_off;
} sfk_roi_ragged_desc;

int sfk_roi_ragged_abi_version(void);
int sfk_roi_resize_ragged(const sfk_roi_ragged_desc* d, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_ROI_RAGGED_H */
