/*
 * sfk_resize.h -- C ABI of the v1 loader's pad + bicubic resize (libsfk.so, gfx950), kept beside include/sfk.h,
 * include/sfk_stem2d.h, include/sfk_u8stem.h, include/sfk_v2.h, include/sfk_aug.h and include/sfk_pool.h so those headers
 * and the ABI lock stay as they are.  The conventions of sfk_pool.h apply: asynchronous on the caller's stream, no
 * allocation, no synchronisation, a negative sfk_status for a bad descriptor before any launch, no environment reads, safe
 * to capture into a hipGraph.
 *
 * sfk_u8_pad_resize_cubic -- the reference's _pad_resize_img (dataset/chalearn_dataset.py:60-71): a crop of h x w pixels
 * and c channels is zero-padded to a square about its centre and resized to size x size with a 4x4-tap cubic (A = -0.75,
 * no antialiasing).  The crops of a batch arrive at their native, ragged sizes, end to end in ONE byte buffer, with a
 * device table of byte offsets and (h, w) pairs; frame f is written as contiguous HWC (size, size, c) uint8 at
 * out + f*out_frame_stride -- a run of FramePool arena slots, or an (N, T, size, size, c) clip.
 *
 * The arithmetic is integer, from 11-bit fixed-point coefficients, and is the specification (tests/ref_resize.py restates
 * it in numpy).  For a frame (h, w, c):
 *     m = max(h, w), nx = (m - w) / 2, ny = (m - h) / 2;  sq(Y, X, ch) = src(Y - ny, X - nx, ch) inside the source
 *     rectangle, else 0 (the square is never materialised).
 *   per axis, for d in 0 .. size-1 (one table for both axes: the square has side m):
 *     f = (float)((d + 0.5) * ((double)m / size) - 0.5)   -- the expression in double, then rounded to float
 *     s = floorf(f), t = f - s                             -- float
 *     k0 = ((A*(t+1) - 5*A)*(t+1) + 8*A)*(t+1) - 4*A       -- float, in this order, every operation rounded on its own
 *     k1 = ((A+2)*t - (A+3))*t*t + 1                          (no FMA contraction)
 *     k2 = ((A+2)*(1-t) - (A+3))*(1-t)*(1-t) + 1
 *     k3 = 1 - k0 - k1 - k2
 *     q_j = (int)rintf(k_j * 2048.f)                       -- round half to even; the four need not sum to 2048
 *     taps at clip(s - 1 + j, 0, m - 1), j = 0..3          -- clipped against the SQUARE: a replicated border tap may
 *                                                             lie in the zero padding
 *   V = sum_i sum_j qy_i * qx_j * sq(Y_i, X_j, ch);  out = clamp((V + (1 << 21)) >> 22, 0, 255), arithmetic shift.
 * Nothing is rounded in between and |V| < 2^31, so the kernel sums rows first in int32.  With m == size the output is the
 * zero-padded source, bit for bit.  Parity with cv2.resize(INTER_CUBIC) itself is unpinned.
 *
 * A MISSING frame -- h <= 0 or w <= 0 in the table, h or w above max_side, or a byte span [offset, offset + h*w*c) that is
 * not inside [0, src_bytes) -- has every output byte equal to fill, and the source is not read for it.  No table content
 * can make the kernel read outside src or write outside the frame's size*size*c output bytes.  The table CONTENTS are read
 * on the device when the launch runs, so a captured graph follows new contents written into the same buffers.
 *
 * One launch, one output row (all c channels) per workgroup of 256 threads.  The row's four source rows are staged in LDS
 * -- as 16-byte loads wherever a whole 16-byte-aligned unit lies inside the row's w*c bytes, byte by byte at its two ends;
 * no byte outside the frame's span is read --, combined into one int32 row of the square's m pixels (zeros in the padding columns),
 * filtered horizontally from LDS, and stored as 16-byte units wherever one lies inside the output row.  All offsets are
 * 64-bit: src may be larger than 2^31 bytes.  No atomics; bit-reproducible.
 *
 * Host-side rejections, with no launch: SFK_ERR_INVALID for a wrong struct_size, a NULL src, offset, hw or out, a
 * non-positive frames, c, size or max_side, a negative src_bytes, out_frame_stride < size*size*c, or fill outside 0..255;
 * SFK_ERR_UNSUPPORTED for more than SFK_RESIZE_MAX_BLOCKS workgroups (frames * size), or when the LDS one workgroup needs,
 * SFK_RESIZE_LDS_BYTES(max_side, c, size), exceeds SFK_RESIZE_MAX_LDS_BYTES (size 192 with c 21 fits up to max_side 666).
 */
#ifndef SFK_RESIZE_H
#define SFK_RESIZE_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_RESIZE_ABI_VERSION 1
#define SFK_RESIZE_MAX_BLOCKS (1 << 23)          /* workgroups of one launch: frames * size */
#define SFK_RESIZE_MAX_LDS_BYTES (128 * 1024)    /* what one workgroup may hold of the CU's 160 KiB */
/* the int32 row (c rounded up to a multiple of 4 per pixel), the four staged source rows (each behind a shift of up to 15
 * bytes, plus one spare unit), the staged output row and the tap table (four int32 offsets, four int32 coefficients and s
 * per output coordinate) */
#define SFK_RESIZE_ROW16(bytes) (((int64_t)(bytes) + 15 + 15) / 16 * 16)
#define SFK_RESIZE_LDS_BYTES(max_side, c, size)                                                                   \
  ((int64_t)(max_side) * (((c) + 3) / 4) * 16 + 4 * (SFK_RESIZE_ROW16((int64_t)(max_side) * (c)) + 16) +         \
   SFK_RESIZE_ROW16((int64_t)(size) * (c)) + (int64_t)(size) * 36)

typedef struct {
  uint32_t struct_size;               /* sizeof(sfk_resize_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t  fill;                      /* 0..255: every output byte of a missing frame */
  const uint8_t* src;                 /* the frames' HWC bytes (pixel pitch c), each frame contiguous */
  int64_t  src_bytes;                 /* bytes of src: a frame whose span is not inside [0, src_bytes) is missing */
  const int64_t* offset;              /* device int64 [frames]: first byte of frame f in src */
  const int32_t* hw;                  /* device int32 [frames][2]: (h, w) of frame f; h <= 0 or w <= 0 is missing */
  int32_t  frames;
  int32_t  c;
  int32_t  size;                      /* S: the output frames are (S, S, c) */
  int32_t  max_side;                  /* the LDS staging is sized for it: a frame with h or w above it is missing */
  uint8_t* out;                       /* frame f at out + f*out_frame_stride, contiguous HWC */
  int64_t  out_frame_stride;          /* bytes, >= size*size*c */
} sfk_resize_desc;

int sfk_resize_abi_version(void);
int sfk_u8_pad_resize_cubic(const sfk_resize_desc* d, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_RESIZE_H */
