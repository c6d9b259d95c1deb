// include/sfk_ema.h: sfk_ema_update (e = e + w * (p - e) over the parameter arena and a table of small tensors, w from a
// step counter on the device) and sfk_ema_swap (the bits of p and e, and of every table pair, exchanged).  One streaming
// pass each.  The first ntensors workgroups own one table tensor each, element by element (at most a few thousand
// elements; first in the grid so that their short dependent loops run beside the streaming workgroups, not behind them).
// Every later workgroup owns SFK_EMA_TILE = 4096 consecutive arena elements: lane l the 16-byte units l, 256 + l, 512 + l,
// 768 + l of the tile, the loads of all four issued before the first store, where p and e are both 16-byte aligned; the
// arena's last tile, a unit of an unaligned arena, and the last count % 4 elements, go unit by unit.  No grid cap and
// no loop over tiles (DESIGN.md section 18 measured one tile per workgroup ahead of a capped grid-stride loop for the
// optimizer passes).  The update's three operations are rn_add / rn_mul of optim_elem.h, compiled with contraction off.
#include "optim_elem.h"
#include "sfk_ema.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnits = SFK_EMA_TILE / (kThreads * 4);     // 16-byte units of a lane
static_assert(SFK_EMA_TILE % (kThreads * 4) == 0, "a tile is a whole number of 16-byte units per lane");

// uniform over the launch: every lane forms the same w from the same counter
__device__ __forceinline__ float ema_weight(const int64_t* step, double decay, int warmup) {
  const int64_t t = step[0];
  double d = decay;
  if (warmup) {
    const double r = (1.0 + (double)t) / (10.0 + (double)t);
    d = r < d ? r : d;
  }
  return (float)(1.0 - d);
}

// native vectors: the non-temporal builtins take them, and HIP's uint4 class kept the swap's units in LDS and scratch
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float ema_one(float e, float p, float w) { return rn_add(e, rn_mul(w, rn_add(p, -e))); }

__global__ __launch_bounds__(kThreads) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ e,
                                                              int64_t count, unsigned ntensors,
                                                              const sfk_ema_tensor* __restrict__ table, double decay,
                                                              int warmup, const int64_t* __restrict__ step) {
  const int tid = threadIdx.x;
  __shared__ float ws;                                      // w, formed by lane 0 while the workgroup's loads are in flight
  if (blockIdx.x < ntensors) {                              // one table tensor (first in the grid: their short dependent
    const sfk_ema_tensor t = table[blockIdx.x];             // loops run beside the streaming workgroups, not behind them)
    const float w = ema_weight(step, decay, warmup);
    for (int i = tid; i < t.n; i += kThreads) t.dst[i] = ema_one(t.dst[i], t.src[i], w);
    return;
  }
  const int64_t base = (int64_t)(blockIdx.x - ntensors) * SFK_EMA_TILE;
  const bool aligned = ((((uintptr_t)p) | ((uintptr_t)e)) & 15) == 0;
  if (aligned && base + SFK_EMA_TILE <= count) {            // a whole aligned tile (uniform): eight loads, then four stores
    // non-temporal accesses: nobody reads the average soon, and the arena is far larger than the caches (measured: 0.0705
    // against 0.0764 ms at the benchmark arena)
    f32x4 pv[kUnits], ev[kUnits];
#pragma unroll
    for (int k = 0; k < kUnits; ++k) {
      const int64_t i = base + (int64_t)(k * kThreads + tid) * 4;
      pv[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + i));
      ev[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(e + i));
    }
    if (tid == 0) ws = ema_weight(step, decay, warmup);
    __syncthreads();
    const float w = ws;
#pragma unroll
    for (int k = 0; k < kUnits; ++k) {
      const int64_t i = base + (int64_t)(k * kThreads + tid) * 4;
      f32x4 o;
      o.x = ema_one(ev[k].x, pv[k].x, w);
      o.y = ema_one(ev[k].y, pv[k].y, w);
      o.z = ema_one(ev[k].z, pv[k].z, w);
      o.w = ema_one(ev[k].w, pv[k].w, w);
      __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(e + i));
    }
    return;
  }
  // the arena's last tile, or an arena off 16-byte alignment: unit by unit
  const float w = ema_weight(step, decay, warmup);
  for (int k = 0; k < kUnits; ++k) {
    const int64_t i = base + (int64_t)(k * kThreads + tid) * 4;
    if (aligned && i + 3 < count) {
      const float4 pv = *reinterpret_cast<const float4*>(p + i);
      const float4 ev = *reinterpret_cast<const float4*>(e + i);
      float4 o;
      o.x = ema_one(ev.x, pv.x, w);
      o.y = ema_one(ev.y, pv.y, w);
      o.z = ema_one(ev.z, pv.z, w);
      o.w = ema_one(ev.w, pv.w, w);
      *reinterpret_cast<float4*>(e + i) = o;
    } else {
      const int64_t e1 = i + 4 < count ? i + 4 : count;
      for (int64_t j = i; j < e1; ++j) e[j] = ema_one(e[j], p[j], w);
    }
  }
}

__global__ __launch_bounds__(kThreads) void ema_swap_kernel(uint32_t* __restrict__ p, uint32_t* __restrict__ e, int64_t count,
                                                            unsigned ntensors, const sfk_ema_tensor* __restrict__ table) {
  const int tid = threadIdx.x;
  if (blockIdx.x < ntensors) {
    const sfk_ema_tensor t = table[blockIdx.x];
    uint32_t* a = reinterpret_cast<uint32_t*>(t.src);
    uint32_t* b = reinterpret_cast<uint32_t*>(t.dst);
    for (int i = tid; i < t.n; i += kThreads) {
      const uint32_t x = a[i], y = b[i];
      a[i] = y;
      b[i] = x;
    }
    return;
  }
  const int64_t base = (int64_t)(blockIdx.x - ntensors) * SFK_EMA_TILE;
  const bool aligned = ((((uintptr_t)p) | ((uintptr_t)e)) & 15) == 0;
  if (aligned && base + SFK_EMA_TILE <= count) {            // a whole aligned tile (uniform): eight loads, then eight stores
    u32x4 pv[kUnits], ev[kUnits];
#pragma unroll
    for (int k = 0; k < kUnits; ++k) {
      const int64_t i = base + (int64_t)(k * kThreads + tid) * 4;
      pv[k] = *reinterpret_cast<const u32x4*>(p + i);
      ev[k] = *reinterpret_cast<const u32x4*>(e + i);
    }
#pragma unroll
    for (int k = 0; k < kUnits; ++k) {
      const int64_t i = base + (int64_t)(k * kThreads + tid) * 4;
      *reinterpret_cast<u32x4*>(p + i) = ev[k];
      *reinterpret_cast<u32x4*>(e + i) = pv[k];
    }
    return;
  }
  for (int k = 0; k < kUnits; ++k) {
    const int64_t i = base + (int64_t)(k * kThreads + tid) * 4;
    if (aligned && i + 3 < count) {
      const u32x4 pv = *reinterpret_cast<const u32x4*>(p + i);
      const u32x4 ev = *reinterpret_cast<const u32x4*>(e + i);
      *reinterpret_cast<u32x4*>(p + i) = ev;
      *reinterpret_cast<u32x4*>(e + i) = pv;
    } else {
      const int64_t e1 = i + 4 < count ? i + 4 : count;
      for (int64_t j = i; j < e1; ++j) {
        const uint32_t x = p[j], y = e[j];
        p[j] = y;
        e[j] = x;
      }
    }
  }
}

// what both entry points refuse; SFK_OK when the arena and the table can be launched
inline int ema_desc_status(const sfk_ema_desc* d) {
  if (!d || d->struct_size != sizeof(sfk_ema_desc)) return SFK_ERR_INVALID;
  if (!d->p || !d->e || d->count <= 0) return SFK_ERR_INVALID;
  if (d->ntensors < 0 || d->ntensors > SFK_EMA_MAX_TENSORS) return SFK_ERR_INVALID;
  if (d->ntensors > 0 && !d->table) return SFK_ERR_INVALID;
  if (d->count > SFK_EMA_MAX_COUNT) return SFK_ERR_UNSUPPORTED;
  return SFK_OK;
}

inline unsigned ema_tiles(int64_t count) { return (unsigned)((count + SFK_EMA_TILE - 1) / SFK_EMA_TILE); }

}  // namespace

extern "C" int sfk_ema_abi_version(void) { return SFK_EMA_ABI_VERSION; }

extern "C" int sfk_ema_update(const sfk_ema_desc* d, sfk_stream_t stream) {
  const int st = ema_desc_status(d);
  if (st != SFK_OK) return st;
  if (!d->step || !(d->decay >= 0.0 && d->decay < 1.0)) return SFK_ERR_INVALID;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned tiles = ema_tiles(d->count);
  hipLaunchKernelGGL(optim_step_inc_kernel, dim3(1), dim3(1), 0, s, d->step);
  hipLaunchKernelGGL(ema_update_kernel, dim3(tiles + (unsigned)d->ntensors), dim3(kThreads), 0, s, d->p, d->e, d->count,
                     (unsigned)d->ntensors, d->table, d->decay, d->warmup ? 1 : 0, d->step);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_ema_swap(const sfk_ema_desc* d, sfk_stream_t stream) {
  const int st = ema_desc_status(d);
  if (st != SFK_OK) return st;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned tiles = ema_tiles(d->count);
  hipLaunchKernelGGL(ema_swap_kernel, dim3(tiles + (unsigned)d->ntensors), dim3(kThreads), 0, s,
                     reinterpret_cast<uint32_t*>(d->p), reinterpret_cast<uint32_t*>(d->e), d->count, (unsigned)d->ntensors, d->table);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}
