/*
 * sfk_u8stem.h -- C ABI of the stem convolutions that read the loader's uint8 frames directly (libsfk.so, gfx950), kept
 * beside include/sfk.h and include/sfk_stem2d.h so those headers and the ABI lock stay as they are.  The same conventions
 * apply (asynchronous on the caller's stream, no allocation, negative sfk_status on a bad descriptor, safe to capture
 * into a hipGraph).
 *
 * sfk_u8_normalize_crop (include/sfk.h) turns HWC uint8 frames into the normalised, randomly cropped float clip the stems
 * then read.  These entry points do that transform while they stage the stem's input patch, so the float clip is never
 * written.  Element (n, c, t, h, w) of the virtual clip the stem convolves (h in [0, h), w in [0, w) of the frame) is
 *     crop == NULL: lut[src[n*sn + t*st + h*sh + w*sw + c0 + c]]
 *     crop != NULL: y = h + top[n] - pad, x = w + left[n] - pad
 *                   (0 <= y < h && 0 <= x < w) ? lut[src[n*sn + t*st + y*sh + x*sw + c0 + c]] : 0
 * i.e. sfk_u8_normalize_crop's formula read in place; the stem's own zero padding applies around it as usual.  Any crop
 * value is memory-safe: out-of-frame elements are masked and their loads read an in-frame pixel instead; every load is a
 * byte, or an aligned dword holding a byte, of an in-frame pixel's channels c0 .. c0 + c - 1.  The crop CONTENTS
 * are read at run time, so a captured graph follows new offsets written into the same buffer.
 *
 * lut[u] is the f32 value sfk_u8_normalize_crop writes for byte u; the stems convert it to the compute dtype on staging
 * exactly as they convert an f32 clip, so the forward output and the BatchNorm partial sums are bit-identical to
 * sfk_u8_normalize_crop (f32 out) followed by the float entry point.  The filter gradients add split sums with fp32
 * atomics, so they match to fp32 rounding.
 *
 * Filter layout, output map, stats layout and row count (sfk_stem_conv_tiles / sfk_stem2d_tiles, sfk_bn_finalize) are
 * those of the float entry points:
 *   sfk_u8stem_conv_*  = sfk_stem_conv_*  (Conv3d (kt,7,7), frame(t) = t_index ? t_index[t] : t, t_len logical frames);
 *   sfk_u8stem2d_*     = sfk_stem2d_*     (Conv2d over the T*C stacked planes, plane t*C + c = frame t, channel c).
 * Host-side rejections, with no launch: SFK_ERR_INVALID for a wrong struct_size, a NULL src or lut, pad < 0, c0 < 0,
 * c0 + c beyond the pixel pitch sw, a negative stride or a non-positive extent; SFK_ERR_UNSUPPORTED where the float entry
 * points return it (cout > 64, cout % 4, misalignment).
 */
#ifndef SFK_U8STEM_H
#define SFK_U8STEM_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_U8STEM_ABI_VERSION 1

typedef struct {
  uint32_t struct_size;  /* sizeof(sfk_u8_clip) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t pad;           /* RandomCrop padding (size // 10); unused when crop == NULL */
  const uint8_t* src;    /* byte (n, t, y, x, ch) at src[n*sn + t*st + y*sh + x*sw + ch]: HWC frames, channel stride 1 */
  int64_t sn, st, sh, sw; /* byte strides; sw is the pixel pitch (channels per pixel) */
  int32_t c0, c;         /* the channels the stem reads: c0 .. c0 + c - 1 */
  int32_t n, t, h, w;    /* clips, frames, frame height, frame width */
  const float* lut;      /* device, float[256] */
  const int32_t* crop;   /* device, [n][2] = (top, left), or NULL (no crop) */
} sfk_u8_clip;

int sfk_u8stem_abi_version(void);
int sfk_u8stem_conv_fwd(const sfk_u8_clip* x, const int32_t* t_index, int32_t t_len, int32_t kt, const void* w,
                        const sfk_fmap* y, float* stats, sfk_stream_t stream);
int sfk_u8stem_conv_wgrad(const sfk_u8_clip* x, const int32_t* t_index, int32_t t_len, int32_t kt, const sfk_fmap* dy,
                          float* dw, sfk_stream_t stream);
int sfk_u8stem2d_fwd(const sfk_u8_clip* x, const void* w, const sfk_fmap* y, float* stats, sfk_stream_t stream);
int sfk_u8stem2d_wgrad(const sfk_u8_clip* x, const sfk_fmap* dy, float* dw, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_U8STEM_H */
