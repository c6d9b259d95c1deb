// include/sfk_optim.h: sfk_adam_hp and sfk_sgd_hp (the optimizer step with a device-side learning-rate table, weight decay
// and a clipping coefficient) and sfk_grad_norm (the global gradient norm behind that coefficient).  One streaming pass
// each, built like sgd.hip: 16-byte loads and stores where every arena pointer of the slice is 16-byte aligned, a scalar
// path otherwise and for the last count % 4 elements, a grid-stride loop under a grid cap.  Every product and sum is rounded
// on its own (rn_mul / rn_add of optim_elem.h, compiled with contraction off), in torch's operation order: nothing becomes an FMA.
#include "optim_elem.h"

namespace {

template <typename S>
__global__ __launch_bounds__(256) void adam_hp_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v, int64_t count,
                                                      HpArgs h, float b1, float b2, float eps, float gscale,
                                                      const int64_t* step, S* __restrict__ shadow) {
  __shared__ float sc[3];
  if (threadIdx.x == 0) {
    const int64_t s = step[0];
    const float lr = hp_lr(h, s);
    const float bc1 = (float)(1.0 - pow((double)b1, (double)s));
    const float bc2 = (float)(1.0 - pow((double)b2, (double)s));
    sc[0] = -__fdiv_rn(lr, bc1);
    sc[1] = __fdiv_rn(1.f, __fsqrt_rn(bc2));     // as sfk_adam: one division per element, not two
    sc[2] = (float)(1.0 - (double)lr * (double)h.wd);
  }
  __syncthreads();
  AdamConst c;
  c.b1 = b1, c.b2 = b2, c.one_m_b1 = rn_add(1.f, -b1), c.one_m_b2 = rn_add(1.f, -b2), c.eps = eps;
  c.neg_step_size = sc[0], c.inv_sqrt_bc2 = sc[1], c.decay_mul = sc[2];
  const bool clip = h.clip_coef != nullptr;
  const float coef = clip ? h.clip_coef[0] : 1.f;
  const int64_t dc = h.mode == SFK_DECAY_NONE ? 0 : h.decay_count;
  const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < count; i += (int64_t)gridDim.x * 1024) {
    if (aligned && i + 3 < count) {
      float4 pv = *reinterpret_cast<float4*>(p + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 mv = *reinterpret_cast<float4*>(m + i);
      float4 vv = *reinterpret_cast<float4*>(v + i);
      float* pp = reinterpret_cast<float*>(&pv);
      const float* gp = reinterpret_cast<const float*>(&gv);
      float* mp = reinterpret_cast<float*>(&mv);
      float* vp = reinterpret_cast<float*>(&vv);
#pragma unroll
      for (int j = 0; j < 4; ++j) adam_hp_one(pp[j], gp[j], mp[j], vp[j], i + j < dc, c, h, gscale, clip, coef);
      *reinterpret_cast<float4*>(p + i) = pv;
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(v + i) = vv;
      if (shadow) {
#pragma unroll
        for (int j = 0; j < 4; ++j) shadow[i + j] = (S)pp[j];
      }
    } else {
      const int64_t e1 = i + 4 < count ? i + 4 : count;
      for (int64_t e = i; e < e1; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_hp_one(pe, g[e], me, ve, e < dc, c, h, gscale, clip, coef);
        p[e] = pe, m[e] = me, v[e] = ve;
        if (shadow) shadow[e] = (S)pe;
      }
    }
  }
}


template <typename S>
__global__ __launch_bounds__(256) void sgd_hp_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ buf, int64_t count, HpArgs h, float mom,
                                                     float one_m_damp, int nesterov, float gscale, const int64_t* step,
                                                     S* __restrict__ shadow) {
  const int64_t s = step[0];
  const bool first = s == 1;
  const float neg_lr = -hp_lr(h, s);
  const bool clip = h.clip_coef != nullptr;
  const float coef = clip ? h.clip_coef[0] : 1.f;
  const int64_t dc = h.mode == SFK_DECAY_L2 ? h.decay_count : 0;
  const bool aligned = ((((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)(buf ? buf : p))) & 15) == 0;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < count; i += (int64_t)gridDim.x * 1024) {
    if (aligned && i + 3 < count) {
      float4 pv = *reinterpret_cast<float4*>(p + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 bv = buf ? *reinterpret_cast<float4*>(buf + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float* pp = reinterpret_cast<float*>(&pv);
      const float* gp = reinterpret_cast<const float*>(&gv);
      float* bp = reinterpret_cast<float*>(&bv);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        pp[j] = sgd_hp_one(pp[j], gp[j], buf ? bp + j : nullptr, first, i + j < dc, neg_lr, mom, one_m_damp, nesterov, h,
                           gscale, clip, coef);
      *reinterpret_cast<float4*>(p + i) = pv;
      if (buf) *reinterpret_cast<float4*>(buf + i) = bv;
      if (shadow) {
#pragma unroll
        for (int j = 0; j < 4; ++j) shadow[i + j] = (S)pp[j];
      }
    } else {
      const int64_t e1 = i + 4 < count ? i + 4 : count;
      for (int64_t e = i; e < e1; ++e) {
        const float pe = sgd_hp_one(p[e], g[e], buf ? buf + e : nullptr, first, e < dc, neg_lr, mom, one_m_damp, nesterov, h,
                                    gscale, clip, coef);
        p[e] = pe;
        if (shadow) shadow[e] = (S)pe;
      }
    }
  }
}


// row b = the sum over the elements its 256 lanes meet in the grid-stride loop, 4 consecutive elements per lane and trip
__global__ __launch_bounds__(256) void grad_norm_rows_kernel(const float* __restrict__ g, int64_t count, float gscale,
                                                             double* __restrict__ partials) {
  __shared__ double red[256];
  const bool aligned = (((uintptr_t)g) & 15) == 0;
  double acc = 0.0;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < count; i += (int64_t)gridDim.x * 1024) {
    if (aligned && i + 3 < count) {
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
        const double x = (double)rn_mul(g[e], gscale);
        acc = fma(x, x, acc);
      }
    }
  }
  const double t = block_sum_256(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}


inline bool hp_ok(const sfk_optim_hp* hp, int64_t count, int max_mode) {
  if (!hp || hp->struct_size != sizeof(sfk_optim_hp)) return false;
  if (!hp->lr_table || hp->lr_len <= 0) return false;
  if (hp->decay_mode < 0 || hp->decay_mode > max_mode) return false;
  if (hp->decay_count < 0 || hp->decay_count > count) return false;
  return true;
}

inline HpArgs hp_args(const sfk_optim_hp* hp) {
  HpArgs h;
  h.lr_table = hp->lr_table, h.lr_len = hp->lr_len, h.decay_count = hp->decay_count, h.clip_coef = hp->clip_coef;
  h.wd = hp->weight_decay, h.mode = hp->decay_mode;
  return h;
}

}  // namespace

extern "C" int sfk_optim_abi_version(void) { return SFK_OPTIM_ABI_VERSION; }

extern "C" int sfk_adam_hp(float* p, const float* g, float* m, float* v, int64_t count, const sfk_optim_hp* hp, float beta1,
                           float beta2, float eps, float grad_scale, int64_t* step, void* shadow, int32_t shadow_dtype,
                           sfk_stream_t stream) {
  if (!p || !g || !m || !v || !step || count <= 0) return SFK_ERR_INVALID;
  if (!hp_ok(hp, count, SFK_DECAY_DECOUPLED)) return SFK_ERR_INVALID;
  if (shadow && shadow_dtype != SFK_F32 && shadow_dtype != SFK_BF16) return SFK_ERR_INVALID;
  const HpArgs h = hp_args(hp);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(optim_step_inc_kernel, dim3(1), dim3(1), 0, s, step);
  const dim3 grid(update_grid(count)), blk(256);
  if (shadow && shadow_dtype == SFK_BF16)
    hipLaunchKernelGGL(adam_hp_kernel<bf16_t>, grid, blk, 0, s, p, g, m, v, count, h, beta1, beta2, eps, grad_scale, step,
                       static_cast<bf16_t*>(shadow));
  else
    hipLaunchKernelGGL(adam_hp_kernel<float>, grid, blk, 0, s, p, g, m, v, count, h, beta1, beta2, eps, grad_scale, step,
                       static_cast<float*>(shadow));
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_sgd_hp(float* p, const float* g, float* buf, int64_t count, const sfk_optim_hp* hp, float momentum,
                          float dampening, int32_t nesterov, float grad_scale, int64_t* step, void* shadow,
                          int32_t shadow_dtype, sfk_stream_t stream) {
  if (!p || !g || !step || count <= 0 || (momentum != 0.f && !buf)) return SFK_ERR_INVALID;
  if (!hp_ok(hp, count, SFK_DECAY_L2)) return SFK_ERR_INVALID;       // torch has no decoupled SGD
  if (shadow && shadow_dtype != SFK_F32 && shadow_dtype != SFK_BF16) return SFK_ERR_INVALID;
  const HpArgs h = hp_args(hp);
  float* b = momentum != 0.f ? buf : nullptr;        // torch keeps no momentum buffer without momentum
  const float one_m_damp = (float)(1.0 - (double)dampening);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(optim_step_inc_kernel, dim3(1), dim3(1), 0, s, step);
  const dim3 grid(update_grid(count)), blk(256);
  if (shadow && shadow_dtype == SFK_BF16)
    hipLaunchKernelGGL(sgd_hp_kernel<bf16_t>, grid, blk, 0, s, p, g, b, count, h, momentum, one_m_damp, nesterov ? 1 : 0,
                       grad_scale, step, static_cast<bf16_t*>(shadow));
  else
    hipLaunchKernelGGL(sgd_hp_kernel<float>, grid, blk, 0, s, p, g, b, count, h, momentum, one_m_damp, nesterov ? 1 : 0,
                       grad_scale, step, static_cast<float*>(shadow));
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_grad_norm_parts(int64_t count) {
  if (count <= 0) return SFK_ERR_INVALID;
  return norm_rows(count);
}

extern "C" int sfk_grad_norm(const float* g, int64_t count, float grad_scale, float max_norm, double* partials, float* out,
                             sfk_stream_t stream) {
  if (!g || !partials || !out || count <= 0 || !(max_norm >= 0.f)) return SFK_ERR_INVALID;
  if (((uintptr_t)partials) & 7) return SFK_ERR_INVALID;
  const int rows = norm_rows(count);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(grad_norm_rows_kernel, dim3((unsigned)rows), dim3(256), 0, s, g, count, grad_scale, partials);
  hipLaunchKernelGGL(grad_norm_fold_kernel, dim3(1), dim3(256), 0, s, partials, rows, max_norm, out);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}
