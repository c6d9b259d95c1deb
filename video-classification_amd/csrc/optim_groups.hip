// include/sfk_groups.h: sfk_adam_groups, sfk_sgd_groups and sfk_grad_norm_groups -- the optimizer step and the gradient norm
// over parameter groups and frozen ranges.  The per-element arithmetic is optim_elem.h's, the one sfk_adam_hp / sfk_sgd_hp
// run, so a segment's result is the bits of an _hp launch on that slice.
//
// Update kernels.  The grid is what the segments cover: the host numbers the (segment, 1024-element arena tile) pairs
// (sfk_group_seg.tile0 is the prefix), workgroup t takes pair t and finds its segment with one uniform binary search (every
// lane reads the same addresses; nothing is looked up per element) whose dependent reads run under the prologue.  One pair per
// workgroup, no grid-stride loop: under sfk_adam_hp's grid cap the second trip of a workgroup cost 14-18 % at the production
// arena; more than 2^31 - 1 pairs (2^41 elements) is SFK_ERR_INVALID.  Inside the tile a
// lane owns the 4 elements at a multiple of 4, as in the _hp kernels: one 16-byte access when they lie inside the segment and
// the arena pointers are 16-byte aligned, the scalar path at segment edges.  The per-group constants (rate, 1 - lr*wd, wd)
// are formed once per workgroup by lanes 0 .. ngroups-1 and kept in LDS.  No atomics, no workgroup waits for another.
//
// Norm kernel.  Bit-identity with sfk_grad_norm fixes which row and lane an element is summed in, so the grid is
// sfk_grad_norm_parts(count) as there; the segment bounds go to LDS once per workgroup and a lane looks its 4 elements up
// there, loading only what is covered.  A skipped element is a skipped fma(0, 0, acc), which leaves acc as it is.
#include "optim_elem.h"
#include "sfk_groups.h"

namespace {

constexpr int kTileShift = 10;
constexpr int64_t kMaxTiles = 0x7fffffff;    // one workgroup per (segment, tile) pair: the grid's x extent
static_assert((1 << kTileShift) == SFK_GROUPS_TILE, "tile size");

struct GroupArgs {
  const sfk_group_seg* segs;
  const float* lr_rows;
  const float* wds;
  const float* clip_coef;
  int64_t lr_len;
  int nsegs;
  int ngroups;
  int mode;
};

// the part of the arena trip t covers: segment k = the last one with tile0 <= t, its tile (begin >> 10) + t - tile0
struct Trip {
  int64_t lo, hi, base;     // elements [lo, hi) of the tile that starts at base
  int group;
  bool decay;
};

__device__ __forceinline__ Trip find_trip(const GroupArgs& a, int64_t t) {
  int lo = 0, hi = a.nsegs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.segs[mid].tile0 <= t) lo = mid; else hi = mid - 1;
  }
  const sfk_group_seg s = a.segs[lo];
  Trip r;
  r.base = ((s.begin >> kTileShift) + (t - s.tile0)) << kTileShift;
  r.lo = s.begin > r.base ? s.begin : r.base;
  r.hi = s.end < r.base + SFK_GROUPS_TILE ? s.end : r.base + SFK_GROUPS_TILE;
  r.group = s.group;
  r.decay = s.decay != 0 && a.mode != SFK_DECAY_NONE;
  return r;
}

template <typename S>
__global__ __launch_bounds__(256) void adam_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, GroupArgs a,
                                                          float b1, float b2, float eps, float gscale, const int64_t* step,
                                                          S* __restrict__ shadow) {
  __shared__ float s_neg[SFK_GROUPS_MAX_GROUPS], s_mul[SFK_GROUPS_MAX_GROUPS], s_wd[SFK_GROUPS_MAX_GROUPS];
  __shared__ float s_inv;
  const Trip cur = find_trip(a, blockIdx.x);  // gridDim.x == tiles; the lookup's dependent reads run under the prologue
  if ((int)threadIdx.x < a.ngroups) {
    const int j = threadIdx.x;
    const int64_t s = step[0];
    HpArgs row;
    row.lr_table = a.lr_rows + (int64_t)j * a.lr_len, row.lr_len = a.lr_len;
    const float lr = hp_lr(row, s);
    const float wd = a.wds[j];
    const float bc1 = (float)(1.0 - pow((double)b1, (double)s));
    const float bc2 = (float)(1.0 - pow((double)b2, (double)s));
    s_neg[j] = -__fdiv_rn(lr, bc1);
    s_mul[j] = (float)(1.0 - (double)lr * (double)wd);
    s_wd[j] = wd;
    if (j == 0) s_inv = __fdiv_rn(1.f, __fsqrt_rn(bc2));
  }
  __syncthreads();
  AdamConst c;
  c.b1 = b1, c.b2 = b2, c.one_m_b1 = rn_add(1.f, -b1), c.one_m_b2 = rn_add(1.f, -b2), c.eps = eps;
  c.inv_sqrt_bc2 = s_inv;
  HpArgs h;
  h.lr_table = nullptr, h.lr_len = 0, h.decay_count = 0, h.clip_coef = a.clip_coef, h.mode = a.mode;
  const bool clip = a.clip_coef != nullptr;
  const float coef = clip ? a.clip_coef[0] : 1.f;
  const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
  {
    c.neg_step_size = s_neg[cur.group], c.decay_mul = s_mul[cur.group];
    h.wd = s_wd[cur.group];
    const int64_t i = cur.base + (int64_t)threadIdx.x * 4;
    if (aligned && i >= cur.lo && i + 4 <= cur.hi) {
      float4 pv = *reinterpret_cast<float4*>(p + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 mv = *reinterpret_cast<float4*>(m + i);
      float4 vv = *reinterpret_cast<float4*>(v + i);
      float* pp = reinterpret_cast<float*>(&pv);
      const float* gp = reinterpret_cast<const float*>(&gv);
      float* mp = reinterpret_cast<float*>(&mv);
      float* vp = reinterpret_cast<float*>(&vv);
#pragma unroll
      for (int j = 0; j < 4; ++j) adam_hp_one(pp[j], gp[j], mp[j], vp[j], cur.decay, c, h, gscale, clip, coef);
      *reinterpret_cast<float4*>(p + i) = pv;
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(v + i) = vv;
      if (shadow) {
#pragma unroll
        for (int j = 0; j < 4; ++j) shadow[i + j] = (S)pp[j];
      }
    } else {
      const int64_t e0 = i > cur.lo ? i : cur.lo;
      const int64_t e1 = i + 4 < cur.hi ? i + 4 : cur.hi;
      for (int64_t e = e0; e < e1; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_hp_one(pe, g[e], me, ve, cur.decay, c, h, gscale, clip, coef);
        p[e] = pe, m[e] = me, v[e] = ve;
        if (shadow) shadow[e] = (S)pe;
      }
    }
  }
}

template <typename S>
__global__ __launch_bounds__(256) void sgd_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ buf, GroupArgs a, float mom, float one_m_damp,
                                                         int nesterov, float gscale, const int64_t* step,
                                                         S* __restrict__ shadow) {
  __shared__ float s_neg[SFK_GROUPS_MAX_GROUPS], s_wd[SFK_GROUPS_MAX_GROUPS];
  const Trip cur = find_trip(a, blockIdx.x);  // as in adam_groups_kernel
  const int64_t s = step[0];
  if ((int)threadIdx.x < a.ngroups) {
    const int j = threadIdx.x;
    HpArgs row;
    row.lr_table = a.lr_rows + (int64_t)j * a.lr_len, row.lr_len = a.lr_len;
    s_neg[j] = -hp_lr(row, s);
    s_wd[j] = a.wds[j];
  }
  __syncthreads();
  const bool first = s == 1;
  HpArgs h;
  h.lr_table = nullptr, h.lr_len = 0, h.decay_count = 0, h.clip_coef = a.clip_coef, h.mode = a.mode;
  const bool clip = a.clip_coef != nullptr;
  const float coef = clip ? a.clip_coef[0] : 1.f;
  const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)(buf ? buf : p))) & 15) == 0;
  {
    const float neg_lr = s_neg[cur.group];
    h.wd = s_wd[cur.group];
    const bool decay = cur.decay && a.mode == SFK_DECAY_L2;
    const int64_t i = cur.base + (int64_t)threadIdx.x * 4;
    if (aligned && i >= cur.lo && i + 4 <= cur.hi) {
      float4 pv = *reinterpret_cast<float4*>(p + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 bv = buf ? *reinterpret_cast<float4*>(buf + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float* pp = reinterpret_cast<float*>(&pv);
      const float* gp = reinterpret_cast<const float*>(&gv);
      float* bp = reinterpret_cast<float*>(&bv);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pp[j] = sgd_hp_one(pp[j], gp[j], buf ? bp + j : nullptr, first, decay, neg_lr, mom, one_m_damp, nesterov, h, gscale,
                           clip, coef);
      *reinterpret_cast<float4*>(p + i) = pv;
      if (buf) *reinterpret_cast<float4*>(buf + i) = bv;
      if (shadow) {
#pragma unroll
        for (int j = 0; j < 4; ++j) shadow[i + j] = (S)pp[j];
      }
    } else {
      const int64_t e0 = i > cur.lo ? i : cur.lo;
      const int64_t e1 = i + 4 < cur.hi ? i + 4 : cur.hi;
      for (int64_t e = e0; e < e1; ++e) {
        const float pe = sgd_hp_one(p[e], g[e], buf ? buf + e : nullptr, first, decay, neg_lr, mom, one_m_damp, nesterov, h,
                                    gscale, clip, coef);
        p[e] = pe;
        if (shadow) shadow[e] = (S)pe;
      }
    }
  }
}

// sfk_grad_norm's rows kernel (same grid, same element -> (row, lane, order) map) that loads covered elements only.
// Dynamic LDS: int64 begin[nsegs], end[nsegs].
__global__ __launch_bounds__(256) void grad_norm_groups_rows_kernel(const float* __restrict__ g, int64_t count,
                                                                    const sfk_group_seg* __restrict__ segs, int nsegs,
                                                                    float gscale, double* __restrict__ partials) {
  __shared__ double red[256];
  extern __shared__ __align__(8) int64_t s_bounds[];
  int64_t* s_begin = s_bounds;
  int64_t* s_end = s_bounds + nsegs;
  for (int k = threadIdx.x; k < nsegs; k += 256) s_begin[k] = segs[k].begin, s_end[k] = segs[k].end;
  __syncthreads();
  const bool aligned = (((uintptr_t)g) & 15) == 0;
  double acc = 0.0;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < count; i += (int64_t)gridDim.x * 1024) {
    int lo = 0, hi = nsegs;                 // the first segment with end > i (nsegs: none)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_end[mid] > i) hi = mid; else lo = mid + 1;
    }
    int k = lo;
    if (k >= nsegs || s_begin[k] >= i + 4) continue;
    if (aligned && s_begin[k] <= i && i + 4 <= s_end[k]) {       // i + 4 <= end <= count
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      const float* gp = reinterpret_cast<const float*>(&gv);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double x = (double)rn_mul(gp[j], gscale);
        acc = fma(x, x, acc);
      }
    } else {
      const int64_t e1 = i + 4 < count ? i + 4 : count;
      for (int64_t e = i; e < e1; ++e) {
        while (k < nsegs && s_end[k] <= e) ++k;
        if (k >= nsegs) break;
        if (s_begin[k] > e) continue;
        const double x = (double)rn_mul(g[e], gscale);
        acc = fma(x, x, acc);
      }
    }
  }
  const double t = block_sum_256(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// begin/end/group of the host mirror against count and ngroups (ngroups < 0: groups not checked); the total tiles, or -1
inline int64_t walk_segs(const sfk_group_seg* segs, int nsegs, int64_t count, int ngroups, bool check_tile0,
                         sfk_group_seg* fill) {
  int64_t prev_end = 0, tiles = 0;
  for (int k = 0; k < nsegs; ++k) {
    const sfk_group_seg& s = segs[k];
    if (s.begin < prev_end || s.begin >= s.end || s.end > count) return -1;
    if (ngroups >= 0 && (s.group < 0 || s.group >= ngroups)) return -1;
    if (fill) fill[k].tile0 = tiles;
    else if (check_tile0 && s.tile0 != tiles) return -1;
    tiles += ((s.end - 1) >> kTileShift) - (s.begin >> kTileShift) + 1;
    prev_end = s.end;
  }
  return tiles;
}

// everything the host can check of sfk_groups_hp; the total tiles (0 with no segment), or -1
inline int64_t groups_ok(const sfk_groups_hp* hp, int64_t count, int max_mode) {
  if (!hp || hp->struct_size != sizeof(sfk_groups_hp)) return -1;
  if (hp->decay_mode < 0 || hp->decay_mode > max_mode) return -1;
  if (hp->nsegs < 0 || hp->nsegs > SFK_GROUPS_MAX_SEGS) return -1;
  if (hp->ngroups < 1 || hp->ngroups > SFK_GROUPS_MAX_GROUPS) return -1;
  if (!hp->lr_rows || !hp->weight_decay || hp->lr_len <= 0) return -1;
  if (hp->nsegs > 0 && (!hp->segs || !hp->segs_host)) return -1;
  const int64_t tiles = walk_segs(hp->segs_host, hp->nsegs, count, hp->ngroups, true, nullptr);
  return tiles > kMaxTiles ? -1 : tiles;
}

inline GroupArgs group_args(const sfk_groups_hp* hp) {
  GroupArgs a;
  a.segs = hp->segs, a.lr_rows = hp->lr_rows, a.wds = hp->weight_decay, a.clip_coef = hp->clip_coef;
  a.lr_len = hp->lr_len, a.nsegs = hp->nsegs, a.ngroups = hp->ngroups, a.mode = hp->decay_mode;
  return a;
}


}  // namespace

extern "C" int sfk_groups_abi_version(void) { return SFK_GROUPS_ABI_VERSION; }

extern "C" int64_t sfk_groups_prepare(sfk_group_seg* segs_host, int32_t nsegs, int64_t count, int32_t ngroups) {
  if (nsegs < 0 || nsegs > SFK_GROUPS_MAX_SEGS || count <= 0 || ngroups < 1 || ngroups > SFK_GROUPS_MAX_GROUPS)
    return SFK_ERR_INVALID;
  if (nsegs > 0 && !segs_host) return SFK_ERR_INVALID;
  if (walk_segs(segs_host, nsegs, count, ngroups, false, nullptr) < 0) return SFK_ERR_INVALID;     // nothing filled on error
  return walk_segs(segs_host, nsegs, count, ngroups, false, segs_host);
}

extern "C" int sfk_adam_groups(float* p, const float* g, float* m, float* v, int64_t count, const sfk_groups_hp* hp,
                               float beta1, float beta2, float eps, float grad_scale, int64_t* step, void* shadow,
                               int32_t shadow_dtype, sfk_stream_t stream) {
  if (!p || !g || !m || !v || !step || count <= 0) return SFK_ERR_INVALID;
  const int64_t tiles = groups_ok(hp, count, SFK_DECAY_DECOUPLED);
  if (tiles < 0) return SFK_ERR_INVALID;
  if (shadow && shadow_dtype != SFK_F32 && shadow_dtype != SFK_BF16) return SFK_ERR_INVALID;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(optim_step_inc_kernel, dim3(1), dim3(1), 0, s, step);
  if (tiles > 0) {
    const GroupArgs a = group_args(hp);
    const dim3 grid((unsigned)tiles), blk(256);
    if (shadow && shadow_dtype == SFK_BF16)
      hipLaunchKernelGGL(adam_groups_kernel<bf16_t>, grid, blk, 0, s, p, g, m, v, a, beta1, beta2, eps, grad_scale, step,
                         static_cast<bf16_t*>(shadow));
    else
      hipLaunchKernelGGL(adam_groups_kernel<float>, grid, blk, 0, s, p, g, m, v, a, beta1, beta2, eps, grad_scale, step,
                         static_cast<float*>(shadow));
  }
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_sgd_groups(float* p, const float* g, float* buf, int64_t count, const sfk_groups_hp* hp, float momentum,
                              float dampening, int32_t nesterov, float grad_scale, int64_t* step, void* shadow,
                              int32_t shadow_dtype, sfk_stream_t stream) {
  if (!p || !g || !step || count <= 0 || (momentum != 0.f && !buf)) return SFK_ERR_INVALID;
  const int64_t tiles = groups_ok(hp, count, SFK_DECAY_L2);        // torch has no decoupled SGD
  if (tiles < 0) return SFK_ERR_INVALID;
  if (shadow && shadow_dtype != SFK_F32 && shadow_dtype != SFK_BF16) return SFK_ERR_INVALID;
  float* b = momentum != 0.f ? buf : nullptr;        // torch keeps no momentum buffer without momentum
  const float one_m_damp = (float)(1.0 - (double)dampening);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(optim_step_inc_kernel, dim3(1), dim3(1), 0, s, step);
  if (tiles > 0) {
    const GroupArgs a = group_args(hp);
    const dim3 grid((unsigned)tiles), blk(256);
    if (shadow && shadow_dtype == SFK_BF16)
      hipLaunchKernelGGL(sgd_groups_kernel<bf16_t>, grid, blk, 0, s, p, g, b, a, momentum, one_m_damp, nesterov ? 1 : 0,
                         grad_scale, step, static_cast<bf16_t*>(shadow));
    else
      hipLaunchKernelGGL(sgd_groups_kernel<float>, grid, blk, 0, s, p, g, b, a, momentum, one_m_damp, nesterov ? 1 : 0,
                         grad_scale, step, static_cast<float*>(shadow));
  }
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_grad_norm_groups(const float* g, int64_t count, const sfk_group_seg* segs,
                                    const sfk_group_seg* segs_host, int32_t nsegs, float grad_scale, float max_norm,
                                    double* partials, float* out, sfk_stream_t stream) {
  if (!g || !partials || !out || count <= 0 || !(max_norm >= 0.f)) return SFK_ERR_INVALID;
  if (((uintptr_t)partials) & 7) return SFK_ERR_INVALID;
  if (nsegs < 0 || nsegs > SFK_GROUPS_MAX_SEGS || (nsegs > 0 && (!segs || !segs_host))) return SFK_ERR_INVALID;
  if (walk_segs(segs_host, nsegs, count, -1, false, nullptr) < 0) return SFK_ERR_INVALID;
  const int rows = norm_rows(count);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(grad_norm_groups_rows_kernel, dim3((unsigned)rows), dim3(256), (size_t)nsegs * 2 * sizeof(int64_t), s, g,
                     count, segs, nsegs, grad_scale, partials);
  hipLaunchKernelGGL(grad_norm_fold_kernel, dim3(1), dim3(256), 0, s, partials, rows, max_norm, out);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}
