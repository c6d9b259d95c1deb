/*
 * sfk_v2.h -- C ABI of the v2 part-box trainer's two extra steps (libsfk.so, gfx950), kept beside include/sfk.h,
 * include/sfk_stem2d.h and include/sfk_u8stem.h so those headers and the ABI lock stay as they are.  The same conventions
 * apply: asynchronous on the caller's stream, no allocation, a negative sfk_status for a bad descriptor before any launch,
 * safe to capture into a hipGraph.
 *
 * sfk_roi_resize -- the part-box crop, uint8 -> float conversion and bilinear resize of the reference's v2 loader
 * (new_feature_test.py: ChalearnGestureDataset._features_from_indices + _preprocess), on the device.  Per clip n, frame t
 * and channel c, with (x1, y1, x2, y2) = box[n] and v[y][x] = lut[src[n*sn + t*st + y*sh + x*sw + c*sc]]:
 *     r   = F.interpolate(v[y1:y2, x1:x2][None, None], (out_h, out_w), mode='bilinear', align_corners=False,
 *                         antialias=antialias)[0, 0]                                   (torch's CPU arithmetic, fp32)
 *     crop == NULL: dst(n, t, c, y, x) = r[y][x]
 *     crop != NULL: y' = y + top[n] - pad, x' = x + left[n] - pad
 *                   dst(n, t, c, y, x) = (0 <= y' < out_h && 0 <= x' < out_w) ? r[y'][x'] : 0
 * (the crop is sfk_u8_normalize_crop's RandomCrop(out, padding = pad) shift); dst(n, t, c, y, x) is
 * dst[n*dn + t*dt + (c_off + c)*dc + y*dh + x] in elements of dst_dtype; a bf16 destination gets r rounded to nearest even.
 * The contract holds for 0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h.  Other box contents are clamped the way a Python slice
 * clamps them (x1 to [0, w-1], x2 to [x1+1, w], y likewise), so every load is of an in-frame byte, or an aligned dword that
 * holds one; the values are then unspecified but finite.  The box and crop CONTENTS are read at run time, so a captured
 * graph follows new boxes written into the same buffers.
 *
 * Host-side rejections, with no launch: SFK_ERR_INVALID for a wrong struct_size, a NULL src, lut, box or dst, a
 * non-positive extent, a negative stride, antialias not 0 or 1, pad < 0, c_off < 0 or a dst dtype that is neither f32 nor
 * bf16; SFK_ERR_UNSUPPORTED for c > SFK_ROI_MAX_C, a pixel pitch sw > 4096 with sc == 1, or a worst-case reduction
 * h/out_h or w/out_w above SFK_ROI_MAX_RATIO (a box never exceeds its frame, so these bound the filter taps of every box).
 *
 * sfk_sgd -- torch.optim.SGD(params, lr, momentum, dampening, nesterov, weight_decay=0, foreach=False) over one flat fp32
 * parameter arena, in torch's operation order without contraction:
 *     g' = g * grad_scale;  buf = g' (step 1) | momentum*buf + (1 - dampening)*g';  d = nesterov ? g' + momentum*buf : buf;
 *     p -= lr * d      (momentum == 0: d = g', buf untouched)
 * step[0] is incremented on the device first and step 1 is decided from it, so a replayed graph stays correct.
 * If shadow != NULL the updated parameters are also written in shadow_dtype (bf16 rounds to nearest even).
 * SFK_ERR_INVALID: a NULL p, g or step, a NULL buf with momentum != 0, count <= 0, a bad shadow dtype.
 */
#ifndef SFK_V2_H
#define SFK_V2_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_V2_ABI_VERSION 1
#define SFK_ROI_MAX_RATIO 8   /* largest supported reduction per axis: 17 antialiasing taps */
#define SFK_ROI_MAX_C 16      /* largest channel count of one launch */

typedef struct {
  uint32_t struct_size;      /* sizeof(sfk_roi_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t antialias;         /* 0 | 1: F.interpolate(..., antialias=) */
  const uint8_t* src;        /* byte (n, t, y, x, c) at src[n*sn + t*st + y*sh + x*sw + c*sc] */
  int64_t sn, st, sh, sw, sc;
  int32_t n, t, h, w, c;     /* clips, frames, frame height, frame width, channels */
  int32_t out_h, out_w;      /* resized extent */
  const float* lut;          /* device, float[256]: the value of byte u */
  const int32_t* box;        /* device, int32 [n][4] = (x1, y1, x2, y2), Python slice bounds */
  const int32_t* crop;       /* device, int32 [n][2] = (top, left), or NULL (no crop) */
  int32_t pad;               /* crop padding; unused when crop == NULL */
  int32_t dst_dtype;         /* SFK_F32 | SFK_BF16 */
  void* dst;                 /* element (n, t, c, y, x) at dst[n*dn + t*dt + (c_off + c)*dc + y*dh + x] */
  int64_t dn, dt, dc, dh;
  int32_t c_off, reserved0;
} sfk_roi_desc;

int sfk_v2_abi_version(void);
int sfk_roi_resize(const sfk_roi_desc* d, sfk_stream_t stream);
int sfk_sgd(float* p, const float* g, float* buf, int64_t count, float lr, float momentum, float dampening,
            int32_t nesterov, float grad_scale, int64_t* step, void* shadow, int32_t shadow_dtype, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_V2_H */
