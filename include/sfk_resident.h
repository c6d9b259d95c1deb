/*
 * sfk_resident.h -- C ABI of the device-resident train set (libsfk.so, gfx950), kept beside include/sfk.h,
 * include/sfk_stem2d.h, include/sfk_u8stem.h, include/sfk_v2.h, include/sfk_aug.h, include/sfk_pool.h and
 * include/sfk_resize.h so those headers and the ABI lock stay as they are.  The conventions of sfk_pool.h apply: asynchronous
 * on the caller's stream, no allocation, no synchronisation, a negative sfk_status for a bad descriptor before any launch, no
 * environment reads, safe to capture into a hipGraph.
 *
 * sfk_u8_pool_gather_crop -- the train loop draws one random window per video per epoch (dataset/chalearn_dataset.py:123-129
 * of the reference) and crops it at random (RandomCrop(size, padding = size // 10), :73-85).  Once the frames of the train
 * videos lie in a pool on the device (sfk_pool.h), a train batch needs no upload: this kernel builds the normalised, CROPPED
 * (n, t, c, h, w) float clip batch from the pool, a table of frame indices and a table of crop offsets in one pass:
 *     ys = y + top[n] - pad,  xs = x + left[n] - pad          (crop == NULL: ys = y, xs = x)
 *     inside = 0 <= ys < h && 0 <= xs < w
 *     out[n][t][ch][y][x] = !inside                    ? 0
 *                         : index[n][t] in [0, frames) ? lut[ pool byte (index[n][t], ys, xs, c0 + ch) ]
 *                         :                              lut[fill]
 * with byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch] and (top, left) = crop[n].  The
 * values are the ones sfk_u8_normalize_crop (include/sfk.h) writes, with the same crop and pad, from the same frames stacked
 * clip by clip, bit for bit: a MISSING frame (an index outside [0, frames)) is the reference's constant-127 image (:116),
 * normalised and then zero-padded by the crop like any other frame.  With crop == NULL it is sfk_u8_pool_gather, bit for bit
 * and launch for launch: the two entry points share one kernel, whose crop is a compile-time switch taken from crop != NULL.
 *
 * Every crop value and every index value is memory-safe: a row or a column wholly outside the frame writes zeros and reads
 * nothing, a missing frame reads nothing, and no byte outside the needed part of the source row's span -- from the first byte
 * of channel c0 of the first source pixel some output pixel maps to, to the last byte of channel c0 + c - 1 of the last such
 * pixel -- is read.  The crop and index CONTENTS are read on the device when the launch runs, so a captured graph follows new
 * tables written into the same buffers.
 *
 * One launch, one output row (all c channels) per workgroup of 256 threads, index[n][t] and crop[n] read once per workgroup;
 * the needed source bytes of row ys are staged through LDS in 16-byte units at the 16-byte phase LDS and global addresses
 * share (byte by byte at the two ends), and the c planes are written contiguously, as 16-byte stores when w is a multiple of
 * 16 / sizeof(element): the x shift only moves the source, the output keeps its alignment.  All offsets are 64-bit.  No
 * atomics; bit-reproducible.
 *
 * Host-side rejections, with no launch, are sfk_u8_pool_gather's: SFK_ERR_INVALID for a wrong struct_size, a NULL pool, index,
 * lut or out, a non-positive frames, h, w, c, n or t, a negative frame_stride, row_stride or c0, pixel_pitch < c0 + c, fill
 * outside 0..255, an out_dtype that is neither f32 nor bf16, or an out that is not 16-byte aligned -- and a negative pad;
 * SFK_ERR_UNSUPPORTED for more than SFK_POOL_MAX_BLOCKS workgroups (n * t * h) or a staged row span, (w - 1)*pixel_pitch + c,
 * of more than SFK_POOL_MAX_ROW_BYTES bytes.
 */
#ifndef SFK_RESIDENT_H
#define SFK_RESIDENT_H

#include "sfk_pool.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_RESIDENT_ABI_VERSION 1

typedef struct {
  uint32_t struct_size;               /* sizeof(sfk_pool_crop_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t  out_dtype;                 /* SFK_F32 | SFK_BF16 */
  const uint8_t* pool;                /* byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch] */
  int64_t  frame_stride, row_stride;  /* bytes */
  int32_t  pixel_pitch;               /* bytes, >= c0 + c */
  int32_t  frames;                    /* frames in the pool */
  int32_t  h, w, c0, c;
  int32_t  n, t;
  const int32_t* index;               /* device int32 [n][t]: pool frame of clip n, time t */
  const float*   lut;                 /* device float[256] */
  const int32_t* crop;                /* device int32 [n][2] = (top, left) of clip n, any values; NULL: no crop */
  int32_t  fill;                      /* 0..255: the byte every pixel of a missing frame has */
  int32_t  pad;                       /* >= 0: RandomCrop's padding; ignored when crop is NULL */
  void*    out;                       /* [n][t][c][h][w], contiguous, 16-byte aligned */
} sfk_pool_crop_desc;

int sfk_resident_abi_version(void);
int sfk_u8_pool_gather_crop(const sfk_pool_crop_desc* d, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_RESIDENT_H */
