/*
 * sfk_optim.h -- C ABI of the scheduled optimizer step (libsfk.so, gfx950), kept beside include/sfk.h and include/sfk_v2.h
 * so those headers, sfk_adam, sfk_sgd and the ABI lock stay as they are.  The same conventions apply: asynchronous on the
 * caller's stream, no allocation, a negative sfk_status for a bad argument before any launch, safe to capture into a hipGraph.
 *
 * The hyper-parameter block sfk_optim_hp is shared by sfk_adam_hp and sfk_sgd_hp:
 *   lr_table     device float[lr_len].  step[0] is incremented on the device first (as sfk_adam / sfk_sgd do); with s the
 *                value after the increment (1-based), the rate of this step is lr = lr_table[min(max(s, 1), lr_len) - 1].
 *                The table is read when the launch RUNS, so a captured graph follows the schedule with no host traffic.
 *   weight_decay wd, by value.
 *   decay_mode   SFK_DECAY_NONE; SFK_DECAY_L2: g' += wd * p (torch.optim.Adam / SGD(weight_decay=));
 *                SFK_DECAY_DECOUPLED: p *= 1 - lr*wd before the update (torch.optim.AdamW).
 *   decay_count  elements [0, decay_count) of the launched slice decay, the rest do not (the boundary is decided per
 *                element).  An entry with p = 0 and g = 0 stays 0 under either mode.
 *   clip_coef    device float[1] (sfk_grad_norm's out + 1), or NULL: no clipping.
 *
 * sfk_adam_hp -- sfk_adam with the block above.  Per element e, every product, sum, quotient and root rounded on its own to
 * float32 (nothing is contracted into an FMA), in torch's single-tensor order:
 *     g' = (g * grad_scale) * clip_coef[0]               (the second product only when clip_coef != NULL)
 *     e < decay_count, L2:        g' = g' + wd * p
 *     e < decay_count, decoupled: p  = p * f32(1 - lr*wd)                               (1 - lr*wd formed in double)
 *     m = b1*m + (1 - b1)*g';   v = b2*v + ((1 - b2)*g')*g'
 *     p = p + (-f32(lr / bc1)) * (m / (sqrt(v) * f32(1 / sqrt(bc2)) + eps)),   bc_i = f32(1 - beta_i^s) from a double pow
 * (the reciprocal of sqrt(bc2) is formed once per launch, as sfk_adam forms it: one division per element)
 * If shadow != NULL the updated parameters are also written in shadow_dtype (bf16 rounds to nearest even).
 *
 * sfk_sgd_hp -- sfk_sgd (include/sfk_v2.h) with the block above: g' as above (SFK_DECAY_NONE or SFK_DECAY_L2), then
 *     buf = g' (s == 1) | momentum*buf + (1 - dampening)*g';  d = nesterov ? g' + momentum*buf : buf;  p = p + (-lr)*d
 * torch has no decoupled SGD: SFK_DECAY_DECOUPLED is SFK_ERR_INVALID.
 *
 * sfk_grad_norm -- torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2, error_if_nonfinite=False) over one flat
 * gradient arena:
 *     out[0] = f32(sqrt(sum_e f64(f32(g[e] * grad_scale))^2))            (squares accumulated in double)
 *     out[1] = c > 1 ? 1 : c,  c = max_norm / (out[0] + 1e-6)            (float32; a NaN norm gives a NaN coefficient,
 *                                                                          an infinite one gives 0, as torch's clamp does)
 * Two launches: sfk_grad_norm_parts(count) workgroups each leave one double in partials[], then one workgroup folds the rows
 * in a fixed order.  The number of rows depends on count alone, nothing is accumulated with atomics and no workgroup waits
 * for another, so the result is the same bits on every run and every device.  The caller owns partials
 * (double[sfk_grad_norm_parts(count)], 8-byte aligned).
 *
 * Host-side rejections, with no launch: SFK_ERR_INVALID for a NULL hp, a wrong struct_size, a NULL lr_table, lr_len <= 0,
 * decay_count outside [0, count], a decay_mode outside 0..2 (0..1 for sfk_sgd_hp), a NULL p, g, m, v or step, a NULL buf
 * with momentum != 0, count <= 0, a bad shadow dtype; for sfk_grad_norm a NULL g, partials or out, count <= 0, or a max_norm
 * that is negative or NaN.  sfk_grad_norm_parts(count <= 0) is SFK_ERR_INVALID.
 *
 * Unlike sfk_adam the pointers need not be 16-byte aligned: an unaligned slice takes the scalar path.
 */
#ifndef SFK_OPTIM_H
#define SFK_OPTIM_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_OPTIM_ABI_VERSION 1
#define SFK_DECAY_NONE 0
#define SFK_DECAY_L2 1
#define SFK_DECAY_DECOUPLED 2
#define SFK_GRAD_NORM_MAX_PARTS 2048   /* the largest value sfk_grad_norm_parts returns */

typedef struct {
  uint32_t struct_size;      /* sizeof(sfk_optim_hp) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t decay_mode;        /* SFK_DECAY_* */
  const float* lr_table;     /* device, float[lr_len] */
  int64_t lr_len;
  int64_t decay_count;       /* elements [0, decay_count) of the launched slice decay */
  const float* clip_coef;    /* device, float[1], or NULL */
  float weight_decay;
  int32_t reserved0;
} sfk_optim_hp;

int sfk_optim_abi_version(void);
int sfk_adam_hp(float* p, const float* g, float* m, float* v, int64_t count, const sfk_optim_hp* hp, float beta1,
                float beta2, float eps, float grad_scale, int64_t* step, void* shadow, int32_t shadow_dtype,
                sfk_stream_t stream);
int sfk_sgd_hp(float* p, const float* g, float* buf, int64_t count, const sfk_optim_hp* hp, float momentum, float dampening,
               int32_t nesterov, float grad_scale, int64_t* step, void* shadow, int32_t shadow_dtype, sfk_stream_t stream);
int sfk_grad_norm_parts(int64_t count);
int sfk_grad_norm(const float* g, int64_t count, float grad_scale, float max_norm, double* partials, float* out,
                  sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_OPTIM_H */
