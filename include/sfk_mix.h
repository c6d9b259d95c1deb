/*
 * sfk_mix.h -- C ABI of the device-side batch mixing (Mixup, CutMix) and of the soft-target loss that goes with it
 * (libsfk.so, gfx950), kept beside include/sfk.h and include/sfk_aug.h so those headers and the ABI lock stay as they are.
 * The conventions of sfk_aug.h apply: asynchronous on the caller's stream, no allocation, no synchronisation, a negative
 * sfk_status for a bad descriptor before any launch, safe to capture into a hipGraph.  The CONTENTS of the mix table are
 * read on the device when the launch runs, so a captured graph follows new draws written into the same buffer.
 *
 * The mix table: device float [n][8], one row per clip, integers stored as floats (as sfk_jitter_desc.params does):
 *     { partner, lam, y0, x0, y1, x1, weight, reserved }
 * partner is the clip this one is mixed with, lam the blend factor, [y0, y1) x [x0, x1) the box pasted from the partner
 * (the same box in every frame and channel of the clip; empty when y1 <= y0 or x1 <= x0), weight the share of the clip's
 * own label in the loss target.  The identity row is { n, 1, 0, 0, 0, 0, 1, 0 } (n: the row's own index).
 *
 * sfk_clip_mix -- mixes the clips of a batch IN PLACE.  Storage as in sfk_jitter_desc: element (n, t, c, y, x) is
 * x[n*sn + t*st + (c_off + c)*sc + y*sh + x] in elements of dtype, c = 0 .. c-1: all c channels from c_off are mixed.
 * With p = partner[n], lam = row[n].lam, om = 1.0f - lam (fp32) and x' the partner's value BEFORE the launch:
 *     inside the row's box   out = x'
 *     elsewhere              out = lam * x + om * x'     (both products and the sum each rounded to fp32, no contraction)
 * A bf16 clip is read as bf16 and written rounded to nearest even.  Both members of a pair are computed from the values
 * both held before the launch, by the lane that loaded them; each member uses its OWN row, and the two rows may differ.
 *   - An element whose result is its own value by construction is not written: lam == 1 outside the box, and every
 *     element of a clip whose partner is itself.
 *   - A pair whose two rows both have lam == 1 and an empty box is neither loaded nor written.
 *   - Nothing outside the c channels is touched: no other channel, no gap between clips, nothing past the last clip.
 *   - Memory safety does not depend on the table.  A row is treated as identity, and its clip left as it is, when its
 *     partner is outside [0, n) or is not mutual (partner[partner[n]] != n).  Box bounds are clamped to the frame.
 *   - No atomics, no LDS reduction, no workgroup waits for another: the result is bit-reproducible.  Indexing is 64-bit.
 * A row of w elements is cut into units of 16 bytes (4 f32 or 8 bf16; the last unit of a row may be short).  A full unit
 * whose two addresses (the clip's and the partner's) are 16-byte aligned, and which lies wholly inside or wholly outside
 * each member's box, moves as 16-byte vectors; any other unit one element at a time.  The grid is sized from the extents
 * alone: n * ceil(t*c*h*ceil(w/V) / SFK_MIX_CHUNK_UNITS) workgroups; a workgroup whose clip is not the lower member of
 * a valid pair, or whose chunk neither row changes, leaves on a uniform branch.
 *
 * Host-side rejections, with no launch: SFK_ERR_INVALID for a wrong struct_size, a NULL x or rows, a non-positive
 * extent, a negative stride or c_off, or a dtype that is neither f32 nor bf16; SFK_ERR_UNSUPPORTED for a clip of more than
 * SFK_MIX_MAX_CLIP_UNITS units or a launch of more than SFK_MIX_MAX_BLOCKS workgroups.
 *
 * sfk_softmax_ce_mix -- sfk_softmax_ce (include/sfk.h) with a soft target.  rows: the mix table, or NULL (every row is
 * identity).  With y1 = labels[n], y2 = labels[partner[n]] (a partner outside [0, n) means n itself), w = weight[n],
 * eps = smoothing and lse = log(sum_j exp(z_j)):
 *     t_k     = (1 - eps) (w [k == y1] + (1 - w) [k == y2]) + eps / K
 *     loss_n  = (1 - eps) (w (lse - z_y1) + (1 - w) (lse - z_y2)) + (eps / K) (K lse - sum_k z_k)
 *     dlogits = (softmax - t) / n * gscale
 * which is torch's F.cross_entropy(z, prob_target, label_smoothing = eps).  loss_out and loss_sum accumulate the batch
 * mean as sfk_softmax_ce does; correct counts argmax == (w >= 0.5 ? y1 : y2), taking the first maximum.  One workgroup
 * per row; the sum_k z_k reduction runs only when eps > 0.  With eps == 0 and identity rows (or rows == NULL), dlogits
 * and correct are bit-identical to sfk_softmax_ce: the same reductions, and t evaluates to exactly 1 and 0.
 * SFK_ERR_INVALID for a NULL logits or labels, n <= 0, k <= 0, or smoothing outside [0, 1).
 */
#ifndef SFK_MIX_H
#define SFK_MIX_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_MIX_ABI_VERSION 1
#define SFK_MIX_ROW_FLOATS 8                 /* floats of one row of the mix table */
#define SFK_MIX_CHUNK_UNITS 1024             /* 16-byte units of one clip that one workgroup owns */
#define SFK_MIX_MAX_CLIP_UNITS (1 << 30)     /* t * c * h * ceil(w / V) of one clip: unit indices stay inside 32 bits */
#define SFK_MIX_MAX_BLOCKS (1 << 23)         /* workgroups of one launch */

typedef struct {
  uint32_t struct_size;      /* sizeof(sfk_mix_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t dtype;             /* SFK_F32 | SFK_BF16, mixed IN PLACE */
  void* x;                   /* element (n, t, c, y, x) at x[n*sn + t*st + (c_off + c)*sc + y*sh + x] */
  int64_t sn, st, sc, sh;
  int32_t n, t, c, h, w;     /* clips, frames, mixed channels, frame height, frame width */
  int32_t c_off;             /* first mixed channel */
  const float* rows;         /* device, float [n][8]: partner, lam, y0, x0, y1, x1, weight, reserved */
} sfk_mix_desc;

int sfk_mix_abi_version(void);
int sfk_clip_mix(const sfk_mix_desc* d, sfk_stream_t stream);
int sfk_softmax_ce_mix(const float* logits, const int64_t* labels, const float* rows, float smoothing, int32_t n, int32_t k,
                       float gscale, float* dlogits, float* loss_out, float* loss_sum, int32_t* correct,
                       sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_MIX_H */
