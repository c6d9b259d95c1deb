// sfk_softmax_ce_mix (include/sfk_mix.h): sfk_softmax_ce (pool_head.hip) with a soft target -- two labels with a weight
// (the mix table of sfk_clip_mix) plus the label-smoothing mass.  One workgroup per row, the maximum and the normaliser
// reduced exactly as softmax_ce_kernel reduces them, so with smoothing 0 and an identity row dlogits and correct carry
// that kernel's bits.  The third reduction, sum_k (z_k - max), feeds the smoothing term only and runs only when eps > 0:
//     (eps / K) (K lse - sum_k z_k) = (eps / K) (K log(sum_j exp(z_j - max)) - sum_k (z_k - max))
// (taken about the maximum, so a common shift of the logits does not cancel in fp32).  A label whose weight is exactly 0
// contributes nothing to the loss, whatever its logit.
#include <math.h>

#include "sfk_common.h"
#include "sfk_mix.h"

#pragma clang fp contract(off)

namespace {

__global__ __launch_bounds__(256) void softmax_ce_mix_kernel(const float* logits, const int64_t* labels, const float* rows,
                                                             float eps, int n, int k, float gscale, float* dlogits,
                                                             float* loss_out, float* loss_sum, int* correct) {
  __shared__ float sred[256];
  __shared__ int sidx[256];
  const int ni = blockIdx.x, tid = threadIdx.x;
  const float* lp = logits + (int64_t)ni * k;
  float mx = -INFINITY;
  int mi = 0x7fffffff;
  for (int i = tid; i < k; i += 256) {
    const float v = lp[i];
    if (v > mx) { mx = v; mi = i; }  // strided scan keeps the first index per thread
  }
  sred[tid] = mx;
  sidx[tid] = mi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      const float o = sred[tid + s];
      const int oi = sidx[tid + s];
      if (o > sred[tid] || (o == sred[tid] && oi < sidx[tid])) { sred[tid] = o; sidx[tid] = oi; }
    }
    __syncthreads();
  }
  mx = sred[0];
  const int amax = sidx[0];
  __syncthreads();
  float se = 0.f;
  for (int i = tid; i < k; i += 256) se += expf(lp[i] - mx);
  sred[tid] = se;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sred[tid] += sred[tid + s];
    __syncthreads();
  }
  se = sred[0];
  float sd = 0.f;                     // sum_k (z_k - max)
  if (eps > 0.f) {                    // (uniform: eps is a kernel argument)
    __syncthreads();
    for (int i = tid; i < k; i += 256) sd += lp[i] - mx;
    sred[tid] = sd;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) sred[tid] += sred[tid + s];
      __syncthreads();
    }
    sd = sred[0];
  }
  int p = ni;
  float w = 1.f;
  if (rows) {
    const float pf = rows[SFK_MIX_ROW_FLOATS * (int64_t)ni];
    if (pf >= 0.f && pf < (float)n) p = (int)pf;
    w = rows[SFK_MIX_ROW_FLOATS * (int64_t)ni + 6];
  }
  const int y1 = (int)labels[ni], y2 = (int)labels[p];
  const float ow = 1.f - w, keep = 1.f - eps, mass = eps / (float)k;
  const float inv_n = 1.f / (float)n;
  if (dlogits)
    for (int i = tid; i < k; i += 256) {
      const float t = keep * ((i == y1 ? w : 0.f) + (i == y2 ? ow : 0.f)) + mass;
      dlogits[(int64_t)ni * k + i] = (expf(lp[i] - mx) / se - t) * inv_n * gscale;
    }
  if (tid == 0) {
    const float lse0 = logf(se);
    const float l1 = w != 0.f ? w * (lse0 + mx - lp[y1]) : 0.f;
    const float l2 = ow != 0.f ? ow * (lse0 + mx - lp[y2]) : 0.f;
    float loss = keep * (l1 + l2);
    if (eps > 0.f) loss = loss + mass * ((float)k * lse0 - sd);
    loss = loss * inv_n;
    if (loss_out) atomicAdd(loss_out, loss);
    if (loss_sum) atomicAdd(loss_sum, loss);
    if (correct && amax == (w >= 0.5f ? y1 : y2)) atomicAdd(correct, 1);
  }
}

}  // namespace

extern "C" int sfk_softmax_ce_mix(const float* logits, const int64_t* labels, const float* rows, float smoothing, int32_t n,
                                  int32_t k, float gscale, float* dlogits, float* loss_out, float* loss_sum,
                                  int32_t* correct, sfk_stream_t stream) {
  if (!logits || !labels || n <= 0 || k <= 0) return SFK_ERR_INVALID;
  if (!(smoothing >= 0.f && smoothing < 1.f)) return SFK_ERR_INVALID;
  hipLaunchKernelGGL(softmax_ce_mix_kernel, dim3((unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream), logits,
                     labels, rows, smoothing, n, k, gscale, dlogits, loss_out, loss_sum, correct);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}
