/*
 * sfk_roi_pool.h -- C ABI of the v2 part-box trainer's device-resident train set (libsfk.so, gfx950), kept beside
 * include/sfk.h, include/sfk_v2.h, include/sfk_pool.h, include/sfk_resident.h and the other side headers so those headers
 * and the ABI lock stay as they are.  The conventions of sfk_v2.h apply: asynchronous on the caller's stream, no allocation,
 * no synchronisation, a negative sfk_status for a bad descriptor before any launch, no environment reads, safe to capture
 * into a hipGraph.
 *
 * sfk_roi_resize_pool -- sfk_roi_resize (include/sfk_v2.h) reading its source frames from a frame pool through a table of
 * frame indices, as sfk_u8_pool_gather (include/sfk_pool.h) reads its own: once the uncropped (h, w, 7) frames of the v2
 * train videos lie in a pool on the device, the cropped, resized clips of a train step need no upload.  For clip n and
 * frame t let f = index[n][t]:
 *     0 <= f < frames:  v[y][x] = lut[pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch]]
 *     otherwise:        v[y][x] = lut[fill]            (a MISSING frame: the constant image of byte fill; the pool is not read)
 * and everything from there on is sfk_roi_resize's contract word for word: (x1, y1, x2, y2) = box[n] clamped the way a
 * Python slice clamps it, r = F.interpolate(v[y1:y2, x1:x2], (out_h, out_w), bilinear, align_corners=False, antialias) in
 * torch's CPU arithmetic, the crop shift (top[n] - pad, left[n] - pad) with zeros outside the resized image, a bf16
 * destination rounded to nearest even, and element (n, t, ch, y, x) at dst[n*dn + t*dt + (c_off + ch)*dc + y*dh + x].  The
 * result is bit-identical to sfk_roi_resize run on the same frames stacked clip by clip (a missing frame stacked as a frame
 * of fill bytes): the two entry points share one kernel, whose source addressing is a compile-time switch.
 *
 * Every value of index, box and crop is memory-safe: an index outside [0, frames) reads nothing from the pool, a box is
 * clamped into its frame before it meets an address, and every LDS index is clamped to what was staged.  As in
 * sfk_roi_resize, the source bytes are read as aligned dwords that each hold at least one byte of an in-frame pixel of the
 * window.  The CONTENTS of index, box and crop are read on the device when the launch runs, so a captured graph follows new
 * tables written into the same buffers.  index[n][t] is read once per workgroup; all offsets are 64-bit (a pool may exceed
 * 2^31 bytes).  No atomics; bit-reproducible.
 *
 * Host-side rejections, with no launch: SFK_ERR_INVALID for a wrong struct_size, a NULL pool, index, lut, box or dst, a
 * non-positive frames, n, t, h, w, c, out_h or out_w, a negative frame_stride, row_stride, c0, dn, dt, dc or dh,
 * pixel_pitch < c0 + c, fill outside 0..255, antialias not 0 or 1, pad < 0, c_off < 0 or a dst dtype that is neither f32 nor
 * bf16; SFK_ERR_UNSUPPORTED for what sfk_roi_resize does not support: c > SFK_ROI_MAX_C, pixel_pitch > 4096, a worst-case
 * reduction h/out_h or w/out_w above SFK_ROI_MAX_RATIO, or a tile that does not fit the LDS.
 */
#ifndef SFK_ROI_POOL_H
#define SFK_ROI_POOL_H

#include "sfk_v2.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_ROI_POOL_ABI_VERSION 1

typedef struct {
  uint32_t struct_size;               /* sizeof(sfk_roi_pool_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t  antialias;                 /* 0 | 1: F.interpolate(..., antialias=) */
  const uint8_t* pool;                /* byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch] */
  int64_t  frame_stride, row_stride;  /* bytes */
  int32_t  pixel_pitch;               /* bytes, >= c0 + c */
  int32_t  frames;                    /* frames in the pool */
  int32_t  h, w, c0, c;               /* frame height, frame width, first channel, channels */
  int32_t  n, t;                      /* clips, frames per clip */
  const int32_t* index;               /* device int32 [n][t]: pool frame of clip n, time t; outside [0, frames): missing */
  const float*   lut;                 /* device float[256]: the value of byte u */
  const int32_t* box;                 /* device int32 [n][4] = (x1, y1, x2, y2), Python slice bounds */
  const int32_t* crop;                /* device int32 [n][2] = (top, left), or NULL (no crop) */
  int32_t  pad;                       /* crop padding; unused when crop == NULL */
  int32_t  fill;                      /* 0..255: the byte every pixel of a missing frame has */
  int32_t  out_h, out_w;              /* resized extent */
  int32_t  dst_dtype;                 /* SFK_F32 | SFK_BF16 */
  void*    dst;                       /* element (n, t, ch, y, x) at dst[n*dn + t*dt + (c_off + ch)*dc + y*dh + x] */
  int64_t  dn, dt, dc, dh;
  int32_t  c_off;
} sfk_roi_pool_desc;

int sfk_roi_pool_abi_version(void);
int sfk_roi_resize_pool(const sfk_roi_pool_desc* d, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_ROI_POOL_H */
