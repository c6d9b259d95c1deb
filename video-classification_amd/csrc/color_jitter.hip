// sfk_color_jitter (include/sfk_aug.h): torchvision's float-tensor ColorJitter on three colour planes of every clip, in place.
//
// A frame is cut into units of 8 consecutive pixels of one row (the last unit of a row may be short), unit u = row *
// ceil(w/8) + group; a workgroup of 256 lanes owns SFK_JITTER_CHUNK_UNITS = 512 consecutive units of one frame, lane l the
// units l and 256 + l of the chunk.  That cut depends on (h, w) only -- not on the dtype, the strides or the alignment -- so
// the order in which gray values are summed is the same for every clip of that geometry:
//   pass 1  each lane sums the gray of its units' pixels left to right, unit after unit, the workgroup folds the 256 lane
//           sums in a fixed LDS tree and writes workspace[frame * chunks + chunk].  Gray is taken after the ops that precede
//           contrast in the clip's order; workgroups of a clip without a contrast op exit after reading params.
//   pass 2  every workgroup of a frame adds that frame's `chunks` partials (lane l those with index l mod 256, in rising
//           order, then the same tree), divides by h*w and applies the four ops to its units.
// A unit whose three plane addresses are 16-byte aligned and that is full moves as 16-byte vectors (two float4 or one
// bf16x8 per plane); any other unit one element at a time.  Both ways feed the same per-pixel arithmetic, written without
// contraction so that the f32 and bf16 instantiations round alike.  Every branch on an op id is per clip: wave-uniform.
#include <math.h>

#include "sfk_common.h"
#include "sfk_aug.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kUnit = 8;
constexpr int kUnitsPerLane = SFK_JITTER_CHUNK_UNITS / kThreads;
static_assert(SFK_JITTER_CHUNK_UNITS % kThreads == 0, "a chunk is a whole number of units per lane");

struct JitGeo {
  FastDiv groups, chunks, t;   // units of a row; chunks of a frame; frames of a clip
  uint32_t units;              // units of a frame
  float count;                 // (float)(h * w)
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
// fmod(x, 1): the fraction keeps x's sign and is always representable, so this is exact
__device__ __forceinline__ float fmod1(float x) { return x - truncf(x); }

__device__ __forceinline__ void hue_op(float& r, float& g, float& b, float hf) {
  // _rgb2hsv
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eqc = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eqc ? 1.f : maxc);
  const float crd = eqc ? 1.f : cr;
  const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
  const bool mr = maxc == r, mg = maxc == g;
  const float hr = mr ? bc - gc : 0.f;
  const float hg = (mg && !mr) ? 2.f + rc - bc : 0.f;
  const float hb = (!mg && !mr) ? 4.f + gc - rc : 0.f;
  float h = fmod1((hr + hg + hb) / 6.f + 1.f);
  // (h + hf) % 1.0, torch's remainder: the result takes the divisor's sign
  float m = fmod1(h + hf);
  if (m < 0.f) m += 1.f;
  h = m;
  // _hsv2rgb
  const float v = maxc;
  const float h6 = h * 6.f;
  const float fl = floorf(h6);
  const float f = h6 - fl;
  const int i = (int)fl % 6;
  const float p = clamp01(v * (1.f - s));
  const float q = clamp01(v * (1.f - s * f));
  const float t = clamp01(v * (1.f - s * (1.f - f)));
  r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : i == 5 ? v : 0.f;
  g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : i == 5 ? p : 0.f;
  b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : i == 5 ? q : 0.f;
}

// slots [0, s1) of the clip's order P[0..3] on the 8 pixels of a unit; `gm` is the frame's gray mean (contrast only)
__device__ __forceinline__ void run_slots(float (&r)[kUnit], float (&g)[kUnit], float (&b)[kUnit], const float (&P)[8], int s1,
                                          float gm) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s >= s1) break;
    const float id = P[s];
    if (id == 0.f) {
      const float f = P[4];
#pragma unroll
      for (int j = 0; j < kUnit; ++j) { r[j] = clamp01(f * r[j]); g[j] = clamp01(f * g[j]); b[j] = clamp01(f * b[j]); }
    } else if (id == 1.f) {
      const float f = P[5], o = (1.f - f) * gm;
#pragma unroll
      for (int j = 0; j < kUnit; ++j) { r[j] = clamp01(f * r[j] + o); g[j] = clamp01(f * g[j] + o); b[j] = clamp01(f * b[j] + o); }
    } else if (id == 2.f) {
      const float f = P[6], of = 1.f - f;
#pragma unroll
      for (int j = 0; j < kUnit; ++j) {
        const float o = of * gray_of(r[j], g[j], b[j]);
        r[j] = clamp01(f * r[j] + o); g[j] = clamp01(f * g[j] + o); b[j] = clamp01(f * b[j] + o);
      }
    } else if (id == 3.f) {
      const float f = P[7];
#pragma unroll
      for (int j = 0; j < kUnit; ++j) hue_op(r[j], g[j], b[j], f);
    }
  }
}

// the fixed tree over the workgroup's 256 lane values; every lane returns the total
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
  const float total = red[0];
  __syncthreads();
  return total;
}

template <typename T>
__device__ __forceinline__ void load_plane(const T* p, bool vec, int cnt, float mean, float std, float (&v)[kUnit]) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < kUnit / DT<T>::VEC; ++q) {
      Vec16<T> x;
      x.load(p + q * DT<T>::VEC);
#pragma unroll
      for (int j = 0; j < DT<T>::VEC; ++j) v[q * DT<T>::VEC + j] = x.get(j) * std + mean;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kUnit; ++j) v[j] = (j < cnt ? (float)p[j] : 0.f) * std + mean;
  }
}

template <typename T>
__device__ __forceinline__ void store_plane(T* p, bool vec, int cnt, float mean, float std, const float (&v)[kUnit]) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < kUnit / DT<T>::VEC; ++q) {
      Vec16<T> x;
#pragma unroll
      for (int j = 0; j < DT<T>::VEC; ++j) x.set(j, (v[q * DT<T>::VEC + j] - mean) / std);
      x.store(p + q * DT<T>::VEC);
    }
  } else {
#pragma unroll
    for (int j = 0; j < kUnit; ++j)
      if (j < cnt) p[j] = (T)((v[j] - mean) / std);
  }
}

template <typename T, bool kPass1>
__global__ __launch_bounds__(kThreads) void color_jitter_kernel(sfk_jitter_desc d, JitGeo geo) {
  __shared__ float red[kThreads];
  const int tid = threadIdx.x;
  uint32_t frame, chunk, n, t;
  geo.chunks.divmod(blockIdx.x, frame, chunk);
  geo.t.divmod(frame, n, t);
  float P[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) P[i] = d.params[8 * (int64_t)n + i];
  int cpos = 4;                                   // the slot of the (first) contrast op
#pragma unroll
  for (int s = 3; s >= 0; --s)
    if (P[s] == 1.f) cpos = s;
  if (kPass1 && cpos == 4) return;

  float* slots = d.workspace + (int64_t)frame * geo.chunks.d;
  float gm = 0.f;
  if (!kPass1 && cpos < 4) {
    float acc = 0.f;
    for (uint32_t i = tid; i < geo.chunks.d; i += kThreads) acc = acc + slots[i];
    gm = block_sum(acc, red) / geo.count;
  }

  T* base = static_cast<T*>(d.x) + (int64_t)n * d.sn + (int64_t)t * d.st;
  const int64_t pr = (int64_t)(d.c_off + (d.bgr ? 2 : 0)) * d.sc, pg = (int64_t)(d.c_off + 1) * d.sc,
                pb = (int64_t)(d.c_off + (d.bgr ? 0 : 2)) * d.sc;
  float acc = 0.f;
  for (int k = 0; k < kUnitsPerLane; ++k) {
    const uint32_t u = chunk * SFK_JITTER_CHUNK_UNITS + k * kThreads + tid;
    if (u >= geo.units) continue;
    uint32_t y, gq;
    geo.groups.divmod(u, y, gq);
    const int x0 = (int)gq * kUnit;
    const int cnt = min(kUnit, d.w - x0);
    T* row = base + (int64_t)y * d.sh + x0;
    T *qr = row + pr, *qg = row + pg, *qb = row + pb;
    const bool vec = cnt == kUnit && ((((uintptr_t)qr) | ((uintptr_t)qg) | ((uintptr_t)qb)) & 15) == 0;
    float r[kUnit], g[kUnit], b[kUnit];
    load_plane<T>(qr, vec, cnt, d.mean, d.std, r);
    load_plane<T>(qg, vec, cnt, d.mean, d.std, g);
    load_plane<T>(qb, vec, cnt, d.mean, d.std, b);
    if (kPass1) {
      run_slots(r, g, b, P, cpos, 0.f);
      float us = 0.f;
#pragma unroll
      for (int j = 0; j < kUnit; ++j)
        if (j < cnt) us = us + gray_of(r[j], g[j], b[j]);
      acc = acc + us;
    } else {
      run_slots(r, g, b, P, 4, gm);
      store_plane<T>(qr, vec, cnt, d.mean, d.std, r);
      store_plane<T>(qg, vec, cnt, d.mean, d.std, g);
      store_plane<T>(qb, vec, cnt, d.mean, d.std, b);
    }
  }
  if (kPass1) {
    const float total = block_sum(acc, red);
    if (tid == 0) slots[chunk] = total;
  }
}

// SFK_OK and the geometry, or the status the extents earn
int jitter_geo(int32_t n, int32_t t, int32_t h, int32_t w, JitGeo* g, int64_t* blocks) {
  if (n <= 0 || t <= 0 || h <= 0 || w <= 0) return SFK_ERR_INVALID;
  if ((int64_t)h * w > SFK_JITTER_MAX_FRAME_PIXELS) return SFK_ERR_UNSUPPORTED;
  const int32_t groups = (w + kUnit - 1) / kUnit;
  const int64_t units = (int64_t)h * groups;
  const int64_t chunks = (units + SFK_JITTER_CHUNK_UNITS - 1) / SFK_JITTER_CHUNK_UNITS;
  const int64_t frames = (int64_t)n * t;
  if (frames > SFK_JITTER_MAX_BLOCKS || frames * chunks > SFK_JITTER_MAX_BLOCKS) return SFK_ERR_UNSUPPORTED;
  g->groups.set(groups);
  g->chunks.set((int32_t)chunks);
  g->t.set(t);
  g->units = (uint32_t)units;
  g->count = (float)((int64_t)h * w);
  *blocks = frames * chunks;
  return SFK_OK;
}

}  // namespace

extern "C" int64_t sfk_color_jitter_workspace_bytes(int32_t n, int32_t t, int32_t h, int32_t w) {
  JitGeo g;
  int64_t blocks = 0;
  const int st = jitter_geo(n, t, h, w, &g, &blocks);
  return st != SFK_OK ? st : blocks * (int64_t)sizeof(float);
}

extern "C" int sfk_color_jitter(const sfk_jitter_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_jitter_desc)) return SFK_ERR_INVALID;
  if (!d->x || !d->params || !d->workspace) return SFK_ERR_INVALID;
  if (d->sn < 0 || d->st < 0 || d->sc < 0 || d->sh < 0 || d->c_off < 0) return SFK_ERR_INVALID;
  if ((d->bgr != 0 && d->bgr != 1) || !(d->std > 0.f)) return SFK_ERR_INVALID;
  if (d->dtype != SFK_F32 && d->dtype != SFK_BF16) return SFK_ERR_INVALID;
  JitGeo g;
  int64_t blocks = 0;
  const int st = jitter_geo(d->n, d->t, d->h, d->w, &g, &blocks);
  if (st != SFK_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)blocks), block(kThreads);
  if (d->dtype == SFK_BF16) {
    hipLaunchKernelGGL((color_jitter_kernel<bf16_t, true>), grid, block, 0, s, *d, g);
    hipLaunchKernelGGL((color_jitter_kernel<bf16_t, false>), grid, block, 0, s, *d, g);
  } else {
    hipLaunchKernelGGL((color_jitter_kernel<float, true>), grid, block, 0, s, *d, g);
    hipLaunchKernelGGL((color_jitter_kernel<float, false>), grid, block, 0, s, *d, g);
  }
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_aug_abi_version(void) { return SFK_AUG_ABI_VERSION; }
