/*
 * sfk_ema.h -- C ABI of the device-side exponential moving average of the weights (libsfk.so, gfx950), kept beside
 * include/sfk.h, include/sfk_aug.h and include/sfk_mix.h so those headers and the ABI lock stay as they are.  The
 * conventions of sfk_aug.h apply: asynchronous on the caller's stream, no allocation, no synchronisation, a negative
 * sfk_status for a bad descriptor before any launch, safe to capture into a hipGraph.  64-bit indexing, no atomics, no
 * workgroup waits for another: the result is bit-reproducible.
 *
 * One descriptor serves both entry points: the live arena p and the average e (fp32, count elements each) and a device
 * table of ntensors small tensors that live outside the arena (the BatchNorm running means and variances), each a live
 * tensor src and its average dst of n elements.
 *
 * sfk_ema_update -- step[0] is incremented first (a one-lane launch of its own, as sfk_adam_hp does); with t the
 * incremented value the rate is
 *     d_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay          (formed in double: timm's ModelEmaV2 warm-up)
 *     w   = (float)(1.0 - d_t)
 * and for every arena element and every element of every table tensor
 *     e = e + w * (p - e)          (the difference, the product and the sum each rounded to fp32, no contraction)
 * which is torch.lerp(e, p, w)'s formula for w < 0.5.  p and every src are only read; nothing outside [0, count) of e
 * and the dst tensors is written.  The counter lives on the device, so a replayed graph follows the warm-up.
 *
 * sfk_ema_swap -- exchanges p[i] and e[i] over the arena, and src and dst of every table tensor, bit for bit (data is
 * moved, not computed on: NaN payloads survive).  Each lane reads both sides and writes both, so there is no third
 * buffer.  step is neither read nor touched (it may be NULL here).  Two swaps are the identity.  src is WRITTEN by this
 * entry point, which is why sfk_ema_tensor.src and sfk_ema_desc.p carry no const.
 *
 * One launch covers the arena and the table: the first ntensors workgroups own one table tensor each, element by element
 * (an entry with n <= 0 is skipped); workgroup ntensors + b, b < ceil(count / SFK_EMA_TILE), owns arena elements
 * [b * SFK_EMA_TILE, (b + 1) * SFK_EMA_TILE), four 16-byte units per lane, all loaded before the first store, when p
 * and e are both 16-byte aligned; element by element otherwise and for the last count % 4 elements.  The grid has no cap
 * and the kernel no loop over tiles.  The CONTENTS of the table are read on the device when the launch runs; its pointers are
 * the caller's responsibility.
 *
 * Host-side rejections, with no launch: SFK_ERR_INVALID for a NULL descriptor, a wrong struct_size, a NULL p or e, a
 * NULL step (sfk_ema_update only), count <= 0, ntensors < 0 or > SFK_EMA_MAX_TENSORS, ntensors > 0 with a NULL table,
 * and (sfk_ema_update only) a decay outside [0, 1) or NaN; SFK_ERR_UNSUPPORTED for a count of more than
 * SFK_EMA_MAX_COUNT elements.
 */
#ifndef SFK_EMA_H
#define SFK_EMA_H

#include "sfk.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_EMA_ABI_VERSION 1
#define SFK_EMA_TILE 4096                    /* arena elements one workgroup owns */
#define SFK_EMA_MAX_TENSORS 4096             /* entries of the table */
#define SFK_EMA_MAX_COUNT (1ll << 42)        /* arena elements: the grid stays inside 31 bits */

typedef struct {
  float* src;                /* the live tensor: read by sfk_ema_update, exchanged with dst by sfk_ema_swap */
  float* dst;                /* its average */
  int32_t n;                 /* elements */
  int32_t reserved0;
} sfk_ema_tensor;

typedef struct {
  uint32_t struct_size;      /* sizeof(sfk_ema_desc) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t warmup;            /* nonzero: d_t = min(decay, (1 + t) / (10 + t)) */
  float* p;                  /* the live arena: read by sfk_ema_update, exchanged with e by sfk_ema_swap */
  float* e;                  /* the average */
  int64_t count;             /* elements of p and of e */
  sfk_ema_tensor* table;     /* device, ntensors entries; may be NULL when ntensors == 0 */
  int32_t ntensors;
  int32_t reserved0;
  double decay;              /* in [0, 1) */
  int64_t* step;             /* device counter, incremented by sfk_ema_update */
} sfk_ema_desc;

int sfk_ema_abi_version(void);
int sfk_ema_update(const sfk_ema_desc* d, sfk_stream_t stream);
int sfk_ema_swap(const sfk_ema_desc* d, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_EMA_H */
