/*
 * sfk_groups.h -- C ABI of the grouped optimizer step (libsfk.so, gfx950): parameter groups with their own learning-rate row
 * and weight decay, and frozen ranges, over one flat arena.  Kept beside include/sfk_optim.h so that header, sfk.h and the
 * ABI lock stay as they are.  The same conventions apply: asynchronous on the caller's stream, no allocation, a negative
 * sfk_status for a bad argument before any launch, safe to capture into a hipGraph.
 *
 * Data model.  A launch gets a table of SEGMENTS and a table of GROUPS.
 *   segment  {begin, end, tile0, group, decay}: arena elements [begin, end) belong to `group`; `decay` != 0 marks them for the
 *            launch's decay_mode.  Segments are sorted and disjoint, 0 <= begin < end <= count; a boundary may fall on any
 *            element (membership is decided per element).  AN ELEMENT COVERED BY NO SEGMENT IS FROZEN: its p, m, v / buf and
 *            shadow keep their bits and are not loaded.
 *            tile0 is the number of 1024-element arena tiles ([1024 t, 1024 (t+1))) the earlier segments touch, a tile that
 *            two segments share counted once for each: tile0[0] = 0, tile0[k+1] = tile0[k] + ((end_k - 1) >> 10) -
 *            (begin_k >> 10) + 1.  sfk_groups_prepare fills it.  The update kernels run one workgroup per (segment, tile)
 *            pair, so a launch costs what it covers, not what the arena holds; more than 2^31 - 1 pairs is SFK_ERR_INVALID.
 *   group j  {row j of lr_rows, a device float[ngroups][lr_len]; weight_decay[j], a device float[ngroups]}.  The caller forms
 *            the rows as f32(lr_table[k] * lr_mult) and the decays as f32(wd * wd_mult) on the host: the kernels multiply
 *            nothing new in.
 *   decay_mode (SFK_DECAY_*, include/sfk_optim.h) and clip_coef are per launch.
 * The tables live in device memory the caller keeps alive; segs_host is a host mirror of segs that the entry points validate
 * (the device copy is not read on the host).
 *
 * sfk_adam_groups / sfk_sgd_groups -- step[0] is incremented once per launch, first, also when no element is covered.
 * CONTRACT: for every segment [b, e) of group j the result is bit-identical to sfk_adam_hp (sfk_sgd_hp) on the slice [b, e)
 * with lr_table = row j, weight_decay = weight_decay[j], the launch's decay_mode, decay_count = decay ? e - b : 0, the same
 * clip_coef and a step counter holding the same value.  (Every product, sum, quotient and root is rounded on its own; the
 * per-element code is the one sfk_adam_hp / sfk_sgd_hp run, csrc/optim_elem.h.)
 *
 * sfk_grad_norm_groups -- CONTRACT: out and partials are bit-identical to sfk_grad_norm on a copy of g whose uncovered
 * elements are zeroed (torch's clip_grad_norm_ never sees a parameter without a gradient).  Rows as
 * sfk_grad_norm_parts(count).  Uncovered elements are not loaded: a NaN there does not show.  Only begin and end of the
 * segments are read.
 *
 * Host-side rejections, with no launch: SFK_ERR_INVALID for everything include/sfk_optim.h rejects (a NULL p, g, m, v or step,
 * count <= 0, a bad decay_mode or shadow dtype, ...), a NULL hp, a wrong struct_size, nsegs < 0 or above SFK_GROUPS_MAX_SEGS,
 * ngroups < 1 or above SFK_GROUPS_MAX_GROUPS, NULL lr_rows or weight_decay, lr_len <= 0, with nsegs > 0 a NULL segs or
 * segs_host, unsorted or overlapping segments, begin >= end, a segment outside [0, count], a group index outside
 * [0, ngroups), a tile0 that is not the prefix above.  nsegs == 0 (everything frozen) is valid.
 *
 * The pointers need not be 16-byte aligned: 4 elements at a multiple of 4 that lie inside one segment move as one 16-byte
 * access when every arena pointer is 16-byte aligned, everything else takes the scalar path.
 */
#ifndef SFK_GROUPS_H
#define SFK_GROUPS_H

#include "sfk_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SFK_GROUPS_ABI_VERSION 1
#define SFK_GROUPS_MAX_SEGS 2048     /* SlowFast-R50 has 110 conv+BN layers: a few hundred ranges at the most */
#define SFK_GROUPS_MAX_GROUPS 64
#define SFK_GROUPS_TILE 1024         /* arena elements per tile */

typedef struct {
  int64_t begin, end;        /* arena elements [begin, end) */
  int64_t tile0;             /* tiles touched by the segments before this one (sfk_groups_prepare) */
  int32_t group;             /* row of lr_rows / entry of weight_decay */
  int32_t decay;             /* != 0: the launch's decay_mode applies */
} sfk_group_seg;

typedef struct {
  uint32_t struct_size;      /* sizeof(sfk_groups_hp) of the caller's layout: anything else is SFK_ERR_INVALID */
  int32_t decay_mode;        /* SFK_DECAY_* */
  const sfk_group_seg* segs;        /* device, [nsegs] */
  const sfk_group_seg* segs_host;   /* host mirror of segs, validated */
  int32_t nsegs;
  int32_t ngroups;
  const float* lr_rows;      /* device, float[ngroups][lr_len] */
  int64_t lr_len;
  const float* weight_decay; /* device, float[ngroups] */
  const float* clip_coef;    /* device, float[1], or NULL */
} sfk_groups_hp;

int sfk_groups_abi_version(void);
/* validates begin/end/group of segs_host[0 .. nsegs) against count and ngroups and fills tile0; returns the total number of
 * tiles (>= 0) or a negative status */
int64_t sfk_groups_prepare(sfk_group_seg* segs_host, int32_t nsegs, int64_t count, int32_t ngroups);
int sfk_adam_groups(float* p, const float* g, float* m, float* v, int64_t count, const sfk_groups_hp* hp, float beta1,
                    float beta2, float eps, float grad_scale, int64_t* step, void* shadow, int32_t shadow_dtype,
                    sfk_stream_t stream);
int sfk_sgd_groups(float* p, const float* g, float* buf, int64_t count, const sfk_groups_hp* hp, float momentum,
                   float dampening, int32_t nesterov, float grad_scale, int64_t* step, void* shadow, int32_t shadow_dtype,
                   sfk_stream_t stream);
int sfk_grad_norm_groups(const float* g, int64_t count, const sfk_group_seg* segs, const sfk_group_seg* segs_host,
                         int32_t nsegs, float grad_scale, float max_norm, double* partials, float* out, sfk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SFK_GROUPS_H */
