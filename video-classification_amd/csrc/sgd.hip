// sfk_sgd (include/sfk_v2.h): torch.optim.SGD(momentum, dampening, nesterov, weight_decay=0, foreach=False) over the
// flat fp32 parameter arena, built like sfk_adam (optim_misc.hip).  Every product and sum is rounded on its own
// (__fmul_rn / __fadd_rn), in torch's operation order, so nothing is contracted into an FMA.
#include "sfk_common.h"
#include "sfk_v2.h"

namespace {

__global__ void sgd_step_inc_kernel(int64_t* step) { step[0] += 1; }

__device__ __forceinline__ float sgd_one(float p, float g, float* buf, bool first, float lr, float mom, float one_m_damp,
                                         bool nesterov, float gscale) {
  const float gs = __fmul_rn(g, gscale);
  float d = gs;
  if (buf) {
    const float b = first ? gs : __fadd_rn(__fmul_rn(mom, *buf), __fmul_rn(one_m_damp, gs));
    *buf = b;
    d = nesterov ? __fadd_rn(gs, __fmul_rn(mom, b)) : b;
  }
  return __fadd_rn(p, __fmul_rn(-lr, d));
}

template <typename S>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                  float* __restrict__ buf, int64_t count, float lr, float mom,
                                                  float one_m_damp, int nesterov, float gscale,
                                                  const int64_t* step, S* __restrict__ shadow) {
  const bool first = step[0] == 1;
  for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i < count; i += (int64_t)gridDim.x * 1024) {
    if (i + 3 < count && (((uintptr_t)(p + i) | (uintptr_t)(g + i) | (uintptr_t)(buf ? buf + i : p + i)) & 15) == 0) {
      float4 pv = *reinterpret_cast<float4*>(p + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 bv = buf ? *reinterpret_cast<float4*>(buf + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      float* pp = reinterpret_cast<float*>(&pv);
      const float* gp = reinterpret_cast<const float*>(&gv);
      float* bp = reinterpret_cast<float*>(&bv);
#pragma unroll
      for (int j = 0; j < 4; ++j) pp[j] = sgd_one(pp[j], gp[j], buf ? bp + j : nullptr, first, lr, mom, one_m_damp, nesterov, gscale);
      *reinterpret_cast<float4*>(p + i) = pv;
      if (buf) *reinterpret_cast<float4*>(buf + i) = bv;
      if (shadow) {
#pragma unroll
        for (int j = 0; j < 4; ++j) shadow[i + j] = (S)pp[j];
      }
    } else {
      const int64_t e1 = i + 4 < count ? i + 4 : count;
      for (int64_t e = i; e < e1; ++e) {
        p[e] = sgd_one(p[e], g[e], buf ? buf + e : nullptr, first, lr, mom, one_m_damp, nesterov, gscale);
        if (shadow) shadow[e] = (S)p[e];
      }
    }
  }
}

inline unsigned sgd_grid(int64_t count) {
  int64_t b = (count + 1023) / 1024;
  if (b > 16384) b = 16384;
  return (unsigned)(b < 1 ? 1 : b);
}

}  // namespace

extern "C" int sfk_sgd(float* p, const float* g, float* buf, int64_t count, float lr, float momentum, float dampening,
                       int32_t nesterov, float grad_scale, int64_t* step, void* shadow, int32_t shadow_dtype,
                       sfk_stream_t stream) {
  if (!p || !g || !step || count <= 0 || (momentum != 0.f && !buf)) return SFK_ERR_INVALID;
  if (shadow && shadow_dtype != SFK_F32 && shadow_dtype != SFK_BF16) return SFK_ERR_INVALID;
  float* b = momentum != 0.f ? buf : nullptr;        // torch keeps no momentum buffer without momentum
  const float one_m_damp = (float)(1.0 - (double)dampening);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sgd_step_inc_kernel, dim3(1), dim3(1), 0, s, step);
  const dim3 grid(sgd_grid(count)), blk(256);
  if (shadow && shadow_dtype == SFK_BF16)
    hipLaunchKernelGGL(sgd_kernel<bf16_t>, grid, blk, 0, s, p, g, b, count, lr, momentum, one_m_damp, nesterov ? 1 : 0,
                       grad_scale, step, static_cast<bf16_t*>(shadow));
  else
    hipLaunchKernelGGL(sgd_kernel<float>, grid, blk, 0, s, p, g, b, count, lr, momentum, one_m_damp, nesterov ? 1 : 0,
                       grad_scale, step, static_cast<float*>(shadow));
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}
