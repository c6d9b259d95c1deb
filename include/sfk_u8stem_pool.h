/*
 * sfk_u8stem_pool.h -- C ABI of the stem convolutions that read their uint8 frames out of the frame pool (libsfk.so, gfx950),
 * kept beside include/sfk.h, include/sfk_stem2d.h, include/sfk_u8stem.h, include/sfk_pool.h and include/sfk_resident.h so those
 * headers and the ABI lock stay as they are.  The conventions of sfk_pool.h apply: asynchronous on the caller's stream, no
 * allocation, no synchronisation, a negative sfk_status for a bad descriptor before any launch, no environment reads, safe to
 * capture into a hipGraph.
 *
 * sfk_u8_pool_gather_crop (include/sfk_resident.h) builds the normalised, cropped (n, t, c, h, w) float clip batch from a pool
 * of uint8 HWC frames, a table of frame indices and a table of crop offsets; the float stems then read that clip.  These entry
 * points are the sfk_u8stem_* kernels (include/sfk_u8stem.h) with the pool's index table in their frame addressing: they do
 * the gather while they stage the stem's input patch, so the float clip is never written.  Element (n, ci, tt, y, x) of the
 * virtual clip the stem convolves is what sfk_u8_pool_gather_crop writes for (n, tt, c0 + ci, y, x):
 *     ys = y + top[n] - pad,  xs = x + left[n] - pad          (crop == NULL: ys = y, xs = x)
 *     inside = 0 <= ys < h && 0 <= xs < w
 *     x[n][ci][tt][y][x] = !inside                     ? 0
 *                        : index[n][tt] in [0, frames) ? lut[ pool byte (index[n][tt], ys, xs, c0 + ci) ]
 *                        :                               lut[fill]
 * with byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + ch] and (top, left) = crop[n].  A MISSING
 * frame (an index outside [0, frames)) is the reference's constant-127 image, normalised and then zero-padded by the crop like
 * any other frame; the stem's own zero padding (spatial, and temporal for kt > 1) applies around the virtual clip as usual.
 * The 3-D stems' own t_index (PackPathway) selects tt first: frame(t) = t_index ? t_index[t] : t, and the pool index is applied
 * to the selected frame, index[n][frame(t)].
 *
 * Every index value and every crop value is memory-safe: a missing frame reads nothing of its own (its masked loads read
 * frame 0 of the pool), out-of-frame elements are masked and their loads read an in-pool pixel instead; every load is a byte,
 * or an aligned dword holding a byte, of channels c0 .. c0 + c - 1 of a pixel of a frame in [0, frames).  No byte outside the
 * pool's allocation is read and nothing is written to it.  All pool offsets are 64-bit: a pool may be larger than 2^32 bytes.
 * The index and crop CONTENTS are read on the device when the launch runs, so a captured graph follows new tables written into
 * the same buffers; the index of a frame is read once per plane (once per frame tap where whole pixels are staged), not per
 * element.
 *
 * The forward output and the BatchNorm partial sums are bit-identical to sfk_u8stem_* on the same frames stacked clip by clip
 * (a missing frame stacked as the constant image of byte fill), and so to sfk_u8_pool_gather_crop (f32 out) followed by the
 * float entry point.  The filter gradients add split sums with fp32 atomics, so they match to fp32 rounding.
 *
 * Filter layout, output map, stats layout and row count are those of the float entry points, as in sfk_u8stem.h:
 *   sfk_u8pstem_conv_*  = sfk_u8stem_conv_*  (Conv3d (kt,7,7), t_len logical frames);
 *   sfk_u8pstem2d_*     = sfk_u8stem2d_*     (Conv2d over the T*C stacked planes, plane t*C + c = frame t, channel c).
 * Host-side rejections, with no launch, are the union of sfk_u8stem_*'s and sfk_u8_pool_gather_crop's: SFK_ERR_INVALID for a
 * wrong struct_size, a NULL pool, index or lut, a non-positive frames, h, w, c, n or t, a negative frame_stride, row_stride,
 * c0 or pad, pixel_pitch < c0 + c, fill outside 0..255, an n other than the output map's, and whatever the float entry points
 * call invalid (a NULL filter / dw, a bad map, an even kt, an output extent that does not follow from h, w and the logical
 * clip length); SFK_ERR_UNSUPPORTED where the float entry points return it (cout > 64, cout % 4, misalignment, more than
 * 4096 planes for the 2-D stem).
 */
#ifndef SFK_U8STEM_POOL_H
#define SFK_U8STEM_POOL_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_U8STEM_POOL_ABI_VERSION 1

typedef struct {
  uint32_t struct_size;               /* sizeof(sfk_u8_pool_clip) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t  reserved0;                 /* 0 */
  const uint8_t* pool;               /* byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + ch] */
  int64_t  frame_stride, row_stride;  /* bytes */
  int32_t  pixel_pitch;               /* bytes, >= c0 + c */
  int32_t  frames;                    /* frames in the pool */
  int32_t  c0, c;                     /* the channels the stem reads: c0 .. c0 + c - 1 */
  int32_t  n, t, h, w;                /* clips, frames per clip, frame height, frame width */
  const int32_t* index;               /* device int32 [n][t]: pool frame of clip n, time t; outside [0, frames): missing */
  const float*   lut;                 /* device float[256] */
  const int32_t* crop;                /* device int32 [n][2] = (top, left) of clip n, any values; NULL: no crop */
  int32_t  pad;                       /* >= 0: RandomCrop's padding; ignored when crop is NULL */
  int32_t  fill;                      /* 0..255: the byte every pixel of a missing frame has */
} sfk_u8_pool_clip;

int sfk_u8stem_pool_abi_version(void);
int sfk_u8pstem_conv_fwd(const sfk_u8_pool_clip* x, const int32_t* t_index, int32_t t_len, int32_t kt, const void* w,
                         const sfk_fmap* y, float* stats, sfk_stream_t stream);
int sfk_u8pstem_conv_wgrad(const sfk_u8_pool_clip* x, const int32_t* t_index, int32_t t_len, int32_t kt, const sfk_fmap* dy,
                           float* dw, sfk_stream_t stream);
int sfk_u8pstem2d_fwd(const sfk_u8_pool_clip* x, const void* w, const sfk_fmap* y, float* stats, sfk_stream_t stream);
int sfk_u8pstem2d_wgrad(const sfk_u8_pool_clip* x, const sfk_fmap* dy, float* dw, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_U8STEM_POOL_H */
