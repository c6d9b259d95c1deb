// The per-element arithmetic and the small helpers shared by optim_sched.hip (include/sfk_optim.h) and optim_groups.hip
// (include/sfk_groups.h): stated once, so the grouped launches cannot drift from sfk_adam_hp / sfk_sgd_hp / sfk_grad_norm.
// Every product and sum is rounded on its own (rn_mul / rn_add below), in torch's operation order.
#ifndef SFK_OPTIM_ELEM_H
#define SFK_OPTIM_ELEM_H
#include "sfk_common.h"
#include "sfk_optim.h"

// HIP's __fmul_rn / __fadd_rn are plain * and + defined where contraction is allowed, and the compiler did fuse them into
// FMAs after inlining (v_pk_fma_f32 in the _hp kernels), differently from kernel to kernel.  The rule "every product and sum
// rounded on its own" -- and with it the bit-identity of a grouped launch with the _hp launch on a slice -- needs products
// and sums formed HERE, with contraction switched off for everything that includes this header.
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float rn_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float rn_add(float a, float b) { return a + b; }

constexpr int kGridCap = 16384;          // workgroups of the update kernels (x 1024 elements per trip)
constexpr int64_t kNormRowElems = 4096;  // elements per partial row below the row cap

__global__ void optim_step_inc_kernel(int64_t* step) { step[0] += 1; }

// the by-value part of sfk_optim_hp, as the kernels take it
struct HpArgs {
  const float* lr_table;
  int64_t lr_len;
  int64_t decay_count;
  const float* clip_coef;
  float wd;
  int mode;
};

// uniform per workgroup: every lane reads the same addresses
__device__ __forceinline__ float hp_lr(const HpArgs& h, int64_t s) {
  int64_t i = s < 1 ? 1 : s;
  if (i > h.lr_len) i = h.lr_len;
  return h.lr_table[i - 1];
}

__device__ __forceinline__ float hp_grad(float g, float p, float gscale, bool clip, float coef, bool l2, float wd) {
  float gs = rn_mul(g, gscale);
  if (clip) gs = rn_mul(gs, coef);
  if (l2) gs = rn_add(gs, rn_mul(wd, p));
  return gs;
}

struct AdamConst {
  float b1, b2, one_m_b1, one_m_b2, eps, neg_step_size, inv_sqrt_bc2, decay_mul;
};

__device__ __forceinline__ void adam_hp_one(float& p, float g, float& m, float& v, bool decay, const AdamConst& c,
                                            const HpArgs& h, float gscale, bool clip, float coef) {
  const float gs = hp_grad(g, p, gscale, clip, coef, decay && h.mode == SFK_DECAY_L2, h.wd);
  float pp = p;
  if (decay && h.mode == SFK_DECAY_DECOUPLED) pp = rn_mul(pp, c.decay_mul);
  m = rn_add(rn_mul(c.b1, m), rn_mul(c.one_m_b1, gs));
  v = rn_add(rn_mul(c.b2, v), rn_mul(rn_mul(c.one_m_b2, gs), gs));
  const float den = rn_add(rn_mul(__fsqrt_rn(v), c.inv_sqrt_bc2), c.eps);
  p = rn_add(pp, rn_mul(c.neg_step_size, __fdiv_rn(m, den)));
}

__device__ __forceinline__ float sgd_hp_one(float p, float g, float* buf, bool first, bool decay, float neg_lr, float mom,
                                            float one_m_damp, bool nesterov, const HpArgs& h, float gscale, bool clip,
                                            float coef) {
  const float gs = hp_grad(g, p, gscale, clip, coef, decay, h.wd);
  float d = gs;
  if (buf) {
    const float b = first ? gs : rn_add(rn_mul(mom, *buf), rn_mul(one_m_damp, gs));
    *buf = b;
    d = nesterov ? rn_add(gs, rn_mul(mom, b)) : b;
  }
  return rn_add(p, rn_mul(neg_lr, d));
}

// fixed-order tree over the 256 lanes' doubles: the same association on every run
__device__ __forceinline__ double block_sum_256(double x, double* red) {
  red[threadIdx.x] = x;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void grad_norm_fold_kernel(const double* __restrict__ partials, int rows, float max_norm,
                                                             float* __restrict__ out) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) acc += partials[r];
  const double t = block_sum_256(acc, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(t);
    const float c = __fdiv_rn(max_norm, rn_add(norm, 1e-6f));
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;          // a NaN coefficient stays NaN (torch.clamp)
  }
}

inline unsigned update_grid(int64_t count) {
  int64_t b = (count + 1023) / 1024;
  if (b > kGridCap) b = kGridCap;
  return (unsigned)(b < 1 ? 1 : b);
}

inline int norm_rows(int64_t count) {
  int64_t r = (count + kNormRowElems - 1) / kNormRowElems;
  if (r > SFK_GRAD_NORM_MAX_PARTS) r = SFK_GRAD_NORM_MAX_PARTS;
  return (int)(r < 1 ? 1 : r);
}

}  // namespace
#endif  // SFK_OPTIM_ELEM_H
