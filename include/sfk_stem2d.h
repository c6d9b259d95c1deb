/*
 * sfk_stem2d.h -- C ABI of the frames-as-channels stem (libsfk.so, gfx950), kept beside include/sfk.h so that header and
 * its ABI lock stay as they are.  The same conventions apply (asynchronous on the caller's stream, no allocation, negative
 * sfk_status on a bad descriptor, safe to capture into a hipGraph).
 *
 * The reference's `res2d` model (torchvision ResNet-50, train.py:64-76) replaces conv1 by Conv2d(T*C, 64, 7, 2, 3,
 * bias=False) and feeds it the clip's T frames of C = 5 channels (BGR+UV) stacked on the channel axis:
 *     y[n, co, ho, wo] = sum_{t,c,kh,kw} w[co, t*C + c, kh, kw] * x[n, t, c, 2ho-3+kh, 2wo-3+kw]
 * The clip is read in place through element strides (the loader's (N,T,21,H,W) memory sliced to [:, :, :5], or any
 * (N, T*C, H, W) tensor expressed as st = C*s_channel, sc = s_channel); neither the slice nor the reshape is copied.
 *
 * Filter layout: the stem layout of sfk_stem_conv_fwd with kt = T frames and cin = C,
 *     w[co][((t*C + c)*7 + kh)*8 + kw],  kw padded 7 -> 8 (zero),  row length kp = sfk_stem_kp(C, T) (zero tail).
 * Output: one output frame (t = 1) of the channels-last sfk_fmap, ho = (h_in - 1)/2 + 1, wo = (w_in - 1)/2 + 1,
 * cout channels (cout % 4 == 0, cout <= 64), bf16 or f32.
 * stats: optional [sfk_stem2d_tiles(...)][cout][2] BatchNorm partial sums (sum, sum of squares), the layout
 * sfk_bn_finalize consumes.
 * Filter gradient: dw [cout][kp] fp32 is OVERWRITTEN (zeroed on the stream, then split sums over pixel ranges are added
 * with fp32 atomics: the summation order of the splits is not fixed, so dW is reproducible to rounding, not bit-exact).
 */
#ifndef SFK_STEM2D_H
#define SFK_STEM2D_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_STEM2D_ABI_VERSION 1

typedef struct {
  uint32_t struct_size; /* sizeof(sfk_stem2d_src) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t src_dtype;    /* sfk_dtype of the clip */
  const void* src;      /* element (n, t, c, h, w) at src[n*sn + t*st + c*sc + h*sh + w*sw] */
  int64_t sn, st, sc, sh, sw;
  int32_t n, t, c, h_in, w_in; /* t frames of c channels each: t*c input planes */
  int32_t reserved0;
} sfk_stem2d_src;

int sfk_stem2d_abi_version(void);
int sfk_stem2d_tiles(const sfk_stem2d_src* s, const sfk_fmap* y);
int sfk_stem2d_fwd(const sfk_stem2d_src* s, const void* w, const sfk_fmap* y, float* stats, sfk_stream_t stream);
int sfk_stem2d_wgrad(const sfk_stem2d_src* s, const sfk_fmap* dy, float* dw, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_STEM2D_H */
