/*
 * sfk_pool.h -- C ABI of the pooled evaluation input (libsfk.so, gfx950), kept beside include/sfk.h, include/sfk_stem2d.h,
 * include/sfk_u8stem.h, include/sfk_v2.h and include/sfk_aug.h so those headers and the ABI lock stay as they are.
 * The conventions of sfk_aug.h apply: asynchronous on the caller's stream, no allocation, no synchronisation, a negative
 * sfk_status for a bad descriptor before any launch, no environment reads, safe to capture into a hipGraph.
 *
 * sfk_u8_pool_gather -- the uniform windows of a test video (dataset/chalearn_dataset.py:131-140 of the reference) overlap:
 * at CLIP_LEN 20 and stride 4 a frame belongs to five windows.  The frames of a video are therefore uploaded ONCE, as a
 * pool of uint8 HWC frames, and this kernel builds the (n, t, c, h, w) float clip batch from the pool and a table of frame
 * indices:
 *     out[n][t][ch][y][x] = lut[ pool byte (index[n][t], y, x, ch) ]
 * with byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch].  The values are the ones
 * sfk_u8_normalize_crop (include/sfk.h) writes, without a crop, from the same frames stacked clip by clip, bit for bit.
 *
 * An index outside [0, frames) names a MISSING frame: every element of that (n, t) slab is lut[fill] and the pool is not
 * read (the reference's "frame file missing -> constant 127 image", :116).  No index value can make the kernel read outside
 * the pool.  The index CONTENTS are read on the device when the launch runs, so a captured graph follows new windows
 * written into the same buffer.  There is no crop: test and valid clips have none.  sfk_u8_pool_gather_crop
 * (include/sfk_resident.h) is this entry point with one; the two share one kernel, the crop a compile-time switch of it.
 *
 * One launch, one output row (all c channels) per workgroup of 256 threads: the row's source bytes, from the first byte of
 * channel c0 of its first pixel to the last byte of channel c0 + c - 1 of its last pixel, are staged through LDS -- as
 * 16-byte loads wherever a whole 16-byte-aligned unit lies inside that span, byte by byte at its two ends; no byte outside
 * the span is read -- and the c planes are written contiguously, as 16-byte stores when w is a multiple of 16 / sizeof
 * (element).  All offsets are 64-bit: a pool may be larger than 2^31 bytes.  No atomics; bit-reproducible.
 *
 * Host-side rejections, with no launch: SFK_ERR_INVALID for a wrong struct_size, a NULL pool, index, lut or out, a
 * non-positive frames, h, w, c, n or t, a negative frame_stride, row_stride or c0, pixel_pitch < c0 + c, fill outside
 * 0..255, an out_dtype that is neither f32 nor bf16, or an out that is not 16-byte aligned; SFK_ERR_UNSUPPORTED for more
 * than SFK_POOL_MAX_BLOCKS workgroups (n * t * h) or a staged row span, (w - 1)*pixel_pitch + c, of more than
 * SFK_POOL_MAX_ROW_BYTES bytes.
 */
#ifndef SFK_POOL_H
#define SFK_POOL_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_POOL_ABI_VERSION 1
#define SFK_POOL_MAX_BLOCKS (1 << 23)        /* workgroups of one launch: n * t * h */
#define SFK_POOL_MAX_ROW_BYTES (60 * 1024)   /* (w - 1)*pixel_pitch + c: what the LDS staging of one row holds */

typedef struct {
  uint32_t struct_size;               /* sizeof(sfk_pool_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t  out_dtype;                 /* SFK_F32 | SFK_BF16 */
  const uint8_t* pool;                /* byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch] */
  int64_t  frame_stride, row_stride;  /* bytes */
  int32_t  pixel_pitch;               /* bytes, >= c0 + c */
  int32_t  frames;                    /* frames in the pool */
  int32_t  h, w, c0, c;
  int32_t  n, t;
  const int32_t* index;               /* device int32 [n][t]: pool frame of clip n, time t */
  const float*   lut;                 /* device float[256] */
  int32_t  fill;                      /* 0..255: the byte every pixel of a missing frame has */
  void*    out;                       /* [n][t][c][h][w], contiguous, 16-byte aligned */
} sfk_pool_desc;

int sfk_pool_abi_version(void);
int sfk_u8_pool_gather(const sfk_pool_desc* d, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_POOL_H */
