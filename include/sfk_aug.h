/*
 * sfk_aug.h -- C ABI of the device-side train-time colour augmentation (libsfk.so, gfx950), kept beside include/sfk.h,
 * include/sfk_stem2d.h, include/sfk_u8stem.h and include/sfk_v2.h so those headers and the ABI lock stay as they are.
 * The conventions of sfk_v2.h apply: asynchronous on the caller's stream, no allocation, no synchronisation, a negative
 * sfk_status for a bad descriptor before any launch, safe to capture into a hipGraph.
 *
 * sfk_color_jitter -- torchvision's float-tensor ColorJitter.forward (dataset/chalearn_dataset.py:48-50 of the reference)
 * on the three colour planes of every (T, 3, H, W) clip of a batch, IN PLACE.  One parameter set per clip applies to all
 * of its frames.  All arithmetic is fp32, in torch's operation order, without contraction.
 *
 * Storage: element (n, t, c, y, x) is x[n*sn + t*st + (c_off + c)*sc + y*sh + x] in elements of dtype, c = 0, 1, 2; with
 * bgr == 0 the planes are R, G, B, with bgr == 1 they are B, G, R.  A stored value s stands for the image value
 * v = s*std + mean (the loader's Normalize undone); the result is written back as (v - mean)/std.  A bf16 clip is read as
 * bf16 and written rounded to nearest even.  Nothing else of the tensor is touched.
 *
 * params[n] = { order[0..3], b, c, s, h } (floats).  For clip n, walk order[0..3]: op id 0 brightness, 1 contrast,
 * 2 saturation, 3 hue; any other value (such as -1) skips the slot.  With blend(a, b, f) = clamp(f*a + (1 - f)*b, 0, 1)
 * and gray = 0.2989 r + 0.587 g + 0.114 b:
 *     brightness: blend(x, 0, b)
 *     contrast:   blend(x, m, c), m = the mean of gray over that ONE frame, of the image as it stands when the op is reached
 *     saturation: blend(x, gray, s)
 *     hue:        torchvision's _rgb2hsv (eqc = max == min, s = cr / (eqc ? 1 : max), the three (max - .)/cr terms,
 *                 h = fmod((hr + hg + hb)/6 + 1, 1)), then h = (h + hf) mod 1 (torch's remainder), then _hsv2rgb
 *                 (i = floor(6h), f = 6h - i, p, q, t clamped to [0, 1], sextant select on i mod 6)
 * The input is not clamped; only the ops clamp.  The params CONTENTS are read on the device when the launch runs, so a
 * captured graph follows new draws written into the same buffer.
 *
 * Two launches behind the one entry point.  Pass 1 writes, for every frame of a clip whose order holds a contrast op,
 * partial sums of gray (taken after the ops that precede contrast) to fixed slots of `workspace`; pass 2 adds them in a
 * fixed order and applies the four ops.  There are no float atomics: the result is bit-reproducible from run to run, and
 * the chunking depends on (h, w) only, so the mean does not depend on the clip's dtype.  Rows whose first element is
 * 16-byte aligned are read and written as 16-byte vectors, 8 pixels a lane; other rows and the last w mod 8 pixels of a
 * row one element at a time.
 *
 * Host-side rejections, with no launch: SFK_ERR_INVALID for a wrong struct_size, a NULL x, params or workspace, a
 * non-positive extent, a negative stride or c_off, bgr not 0 or 1, std <= 0 or a dtype that is neither f32 nor bf16;
 * SFK_ERR_UNSUPPORTED for a frame of more than SFK_JITTER_MAX_FRAME_PIXELS pixels or more than SFK_JITTER_MAX_BLOCKS
 * workgroups (n * t * ceil(h * ceil(w/8) / SFK_JITTER_CHUNK_UNITS)).  sfk_color_jitter_workspace_bytes returns the same
 * statuses (negative) for such extents.
 */
#ifndef SFK_AUG_H
#define SFK_AUG_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_AUG_ABI_VERSION 1
#define SFK_JITTER_CHUNK_UNITS 512             /* 8-pixel units of one frame whose gray sum is one workspace slot */
#define SFK_JITTER_MAX_FRAME_PIXELS (1 << 26)  /* h * w of one frame: unit indices stay far inside 32 bits */
#define SFK_JITTER_MAX_BLOCKS (1 << 23)        /* workgroups of one launch */

typedef struct {
  uint32_t struct_size;      /* sizeof(sfk_jitter_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t dtype;             /* SFK_F32 | SFK_BF16, jittered IN PLACE */
  void* x;                   /* element (n, t, c, y, x) at x[n*sn + t*st + (c_off + c)*sc + y*sh + x], c = 0, 1, 2 */
  int64_t sn, st, sc, sh;
  int32_t n, t, h, w;        /* clips, frames, frame height, frame width */
  int32_t c_off, bgr;        /* bgr 0: planes are R, G, B; 1: B, G, R */
  float mean, std;           /* stored s <-> image value v = s*std + mean */
  const float* params;       /* device, float [n][8]: order[4] (op ids as floats), then the factors b, c, s, h */
  float* workspace;          /* device, sfk_color_jitter_workspace_bytes(n, t, h, w) bytes */
} sfk_jitter_desc;

int sfk_aug_abi_version(void);
int64_t sfk_color_jitter_workspace_bytes(int32_t n, int32_t t, int32_t h, int32_t w);
int sfk_color_jitter(const sfk_jitter_desc* d, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_AUG_H */
