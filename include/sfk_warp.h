/*
 * sfk_warp.h -- C ABI of the random affine augmentation (libsfk.so, gfx950), kept beside include/sfk.h and the other side
 * headers so those headers and the ABI lock stay as they are.  The conventions of sfk_pool.h apply: asynchronous on the
 * caller's stream, no allocation, no synchronisation, a negative sfk_status for a bad descriptor before any launch, no
 * environment reads, safe to capture into a hipGraph.
 *
 * sfk_u8_pool_gather_warp -- sfk_u8_pool_gather_crop (include/sfk_resident.h) can only shift a clip by whole pixels.  This
 * is its sibling that samples every clip through a 2 x 3 matrix of its own: rotation, scale, shear, flip and translation of
 * the normalised (n, t, c, h, w) float clip, written where the clip is first written, with no second clip.  The crop is the
 * special case "identity plus integer translation", and those rows reproduce sfk_u8_pool_gather_crop bit for bit.
 *
 * Contract.  Per clip n, M = warp[n] = (a, b, c, d, e, f) maps OUTPUT pixel (x, y) to a source position.  Every operation
 * below is an individually rounded fp32 operation, in exactly this order (the source is compiled with contraction off):
 *     xs = (a*x + b*y) + c                      ys = (d*x + e*y) + f
 *     if !(xs > -1 && xs < w && ys > -1 && ys < h):   out = 0, nothing is loaded            (a NaN falls here)
 *     x0 = floor(xs), fx = xs - x0              y0 = floor(ys), fy = ys - y0
 *     v(yy, xx) = 0 <= yy < h && 0 <= xx < w ? (index[n][t] in [0, frames) ? lut[pool byte (index[n][t], yy, xx, c0 + ch)]
 *                                                                           : lut[fill])
 *                                            : 0
 *     top = v(y0, x0) + fx*(v(y0, x0+1) - v(y0, x0));   bot = v(y0+1, x0) + fx*(v(y0+1, x0+1) - v(y0+1, x0))
 *     out[n][t][ch][y][x] = top + fy*(bot - top)
 * with byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch].  This is bilinear sampling with
 * padding_mode = 'zeros' and align_corners = False in pixel-index coordinates; the zeros are those of the NORMALISED tensor,
 * as RandomCrop's are; a MISSING frame (an index outside [0, frames)) is the constant image of byte fill, normalised and then
 * zero-padded like any other.  A bf16 out is the fp32 result rounded to nearest even.  The float-to-int conversion happens
 * only after the range test.  index == NULL names frame n*t + tt: a stacked (N, T, h, w, P) batch is a pool that needs no
 * table.
 *
 * EVERY table content, finite or not, is memory-safe.  The only global reads of frame bytes are (1) the staging of a box
 * whose corners are integers clamped to [0, w-1] x [0, h-1] before they meet an address, row by row from the first byte of
 * channel c0 of its first pixel to the last byte of channel c0 + c - 1 of its last, and (2) single bytes of channels
 * [c0, c0 + c) of a pixel whose integer coordinates passed 0 <= xx < w, 0 <= yy < h.  A missing frame and a tile with no tap
 * inside the frame read nothing.  The warp and index CONTENTS are read on the device when the launch runs, so a captured
 * graph follows new tables written into the same buffers.
 *
 * Kernel shape.  One launch; a workgroup of 256 threads owns an output tile of SFK_WARP_TILE_H x SFK_WARP_TILE_W pixels of
 * one (n, t) and all c channels.  It evaluates the contract's (xs, ys) at the four corners of its tile -- each coordinate is
 * monotone in x and in y, rounding included, so the corners bound the tile -- and stages that source box's bytes through LDS
 * in 16-byte units at the 16-byte phase LDS and global addresses share, as sfk_u8_pool_gather_crop stages its row.  The
 * four taps of every channel are then read from LDS through LDS copies of lut (eight, interleaved, so that lanes seldom meet
 * on a bank), and the c planes are written as contiguous runs of the tile's width, as 16-byte stores when w is a multiple of
 * 16 / sizeof(element), whatever the matrix (a thread samples four pixels; for bf16 two neighbouring lanes trade halves of two
 * channels).  A tile whose corners say that every tap lies inside the frame samples without a single test.  A box that
 * needs more than the launch's staging bytes (SFK_WARP_LDS_BYTES at most: strong minification), or whose corners are not
 * all numbers, makes the whole workgroup take its taps from global memory instead, with the same arithmetic.
 * sfk_warp_fallback_tiles says on the host, from the matrix alone, how many tiles of a frame do.  All offsets are 64-bit.
 * No atomics; bit-reproducible.
 *
 * Host-side rejections, with no launch, are sfk_u8_pool_gather_crop's, minus pad, plus a NULL warp: SFK_ERR_INVALID for a
 * wrong struct_size, a NULL pool, lut, warp or out (index may be NULL), a non-positive frames, h, w, c, n or t, a negative
 * frame_stride, row_stride or c0, pixel_pitch < c0 + c, fill outside 0..255, an out_dtype that is neither f32 nor bf16, or
 * an out that is not 16-byte aligned; SFK_ERR_UNSUPPORTED for more than SFK_WARP_MAX_BLOCKS workgroups (n * t * tiles).
 */
#ifndef SFK_WARP_H
#define SFK_WARP_H

#include "sfk_pool.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_WARP_ABI_VERSION 1
#define SFK_WARP_TILE_H 16                   /* output rows of one workgroup's tile */
#define SFK_WARP_TILE_W 32                   /* output columns of it */
#define SFK_WARP_LDS_BYTES (32 * 1024)       /* the most a workgroup stages; with the table's 8 KB, four workgroups per CU */
#define SFK_WARP_MAX_BLOCKS (1 << 23)        /* workgroups of one launch: n * t * ceil(h / TILE_H) * ceil(w / TILE_W) */

typedef struct {
  uint32_t struct_size;               /* sizeof(sfk_pool_warp_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t  out_dtype;                 /* SFK_F32 | SFK_BF16 */
  const uint8_t* pool;                /* byte (f, y, x, ch) at pool[f*frame_stride + y*row_stride + x*pixel_pitch + c0 + ch] */
  int64_t  frame_stride, row_stride;  /* bytes */
  int32_t  pixel_pitch;               /* bytes, >= c0 + c */
  int32_t  frames;                    /* frames in the pool */
  int32_t  h, w, c0, c;
  int32_t  n, t;
  const int32_t* index;               /* device int32 [n][t]: pool frame of clip n, time t; NULL: frame n*t + tt */
  const float*   lut;                 /* device float[256] */
  const float*   warp;                /* device float [n][6] = (a, b, c, d, e, f) of clip n, any values */
  int32_t  fill;                      /* 0..255: the byte every pixel of a missing frame has */
  void*    out;                      /* [n][t][c][h][w], contiguous, 16-byte aligned */
} sfk_pool_warp_desc;

int sfk_warp_abi_version(void);
int sfk_u8_pool_gather_warp(const sfk_pool_warp_desc* d, sfk_stream_t stream);
/* Host only, launches nothing: how many of the ceil(h / TILE_H) * ceil(w / TILE_W) tiles of an h x w frame with this pixel
 * pitch and channel count take their taps from global memory under the HOST matrix m[6] (a tile with no tap inside the frame
 * stages nothing and is not counted); SFK_ERR_INVALID for a NULL m, a non-positive h, w or c, or pixel_pitch < c,
 * SFK_ERR_UNSUPPORTED for more than SFK_WARP_MAX_BLOCKS tiles. */
int sfk_warp_fallback_tiles(int32_t h, int32_t w, int32_t pixel_pitch, int32_t c, const float* m);

#ifdef __cplusplus
}
#endif
#endif /* SFK_WARP_H */
