// What stem_conv.hip and stem2d.hip share of the layer that reads a clip into a 16x16 output tile's LDS patch -- f32 / bf16
// elements through strides, or the loader's HWC uint8 frames through a 256-entry f32 table with a per-clip crop shift
// (include/sfk_u8stem.h), stacked or in a frame pool (include/sfk_u8stem_pool.h):
//   device  the tile / patch geometry, ldsrc, plane_store, and the MFMA operand fragments both files build from the patch
//           (Frag, F8, store4);
//   host    U8View, the one description of either uint8 descriptor that both files' fill functions start from.
// NOT here: PatchSlots (a thread's source offsets of a tile) and plane_fetch (a plane's loads).  Each file keeps its own copy
// on purpose; they differ in ONE thing, where a masked slot's offset becomes 0 (stem2d.hip: when set_tile stores it;
// stem_conv.hip: when plane_fetch / stage_u8_pixels add it to the plane's base).  Both are safe -- no address is ever formed
// from a masked slot's coordinates -- but the generated kernels are not indifferent to it.  Measured on an MI355X with either
// form in a shared header: stem_conv's form in stem2d.hip changes all 16 of its kernels (float sources 20 % faster, the uint8
// filter gradients 1.5 - 2.5 % slower: outside the run-to-run spread); stem2d's form in stem_conv.hip changes 72 kernels,
// all of them longer, the uint8 filter gradients with SGPR spills they did not have, among them the slow stem's filter gradient
// of every training step (1702 -> 1741 instructions; not timed).  A new source kind edits both copies, and which plane a
// patch comes from is each file's own plane_base anyway.
#pragma once
#include "sfk_common.h"

namespace {

constexpr int TS = 16;            // output tile edge (pixels)
constexpr int PR = 2 * TS + 5;    // patch rows  (37)
constexpr int PC = 40;            // patch cols  (2*15 + 7 + 1 = 38 used, padded)
constexpr int PLANE = PR * PC;    // 1480 elements per (frame, channel) plane

template <typename S> __device__ __forceinline__ float ldsrc(const void* p, int64_t off);
template <> __device__ __forceinline__ float ldsrc<float>(const void* p, int64_t off) { return static_cast<const float*>(p)[off]; }
template <> __device__ __forceinline__ float ldsrc<bf16_t>(const void* p, int64_t off) { return (float)static_cast<const bf16_t*>(p)[off]; }

// The patch of one plane is NSLOT slots per thread.  A thread's slots have the same (row, col) for every plane and tile, so
// their source offsets are computed once per tile and the loads of a plane (or several planes) are issued back to back --
// the loader is latency-bound otherwise.
constexpr int NSLOT = (PLANE + 255) / 256;   // 6

template <typename T>
__device__ __forceinline__ void plane_store(T* patch, const float (&v)[NSLOT]) {
#pragma unroll
  for (int i = 0; i < NSLOT; ++i) {
    const int e = threadIdx.x + 256 * i;
    if (e < PLANE) patch[e] = (T)v[i];
  }
}

// ------------------------------------------------------------------------------------------ MFMA operands
// 8 consecutive K elements of one lane, built from the LDS patch and the staged filter / dY rows: bf16 (one 16x16x32 MFMA)
// or f32 (eight 16x16x4)
template <typename T> struct Frag;
template <> struct Frag<bf16_t> {
  typedef bf16x8 ab;
  static __device__ __forceinline__ ab run8(const bf16_t* p) {   // 8 consecutive elements, 4-byte aligned
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    uint4 v = make_uint4(q[0], q[1], q[2], q[3]);
    return *reinterpret_cast<ab*>(&v);
  }
  static __device__ __forceinline__ ab ld16(const bf16_t* p) { return *reinterpret_cast<const ab*>(p); }
  static __device__ __forceinline__ void zero(ab& v) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16_t)0.f;
  }
  static __device__ __forceinline__ void set(ab& v, int i, float f) { v[i] = (bf16_t)f; }
  static __device__ __forceinline__ void mma(f32x4& acc, const ab& a, const ab& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  }
};
struct F8 { float v[8]; };
template <> struct Frag<float> {
  typedef F8 ab;
  static __device__ __forceinline__ ab run8(const float* p) {    // 8 consecutive floats, 8-byte aligned
    ab r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float2 t = *reinterpret_cast<const float2*>(p + 2 * i);
      r.v[2 * i] = t.x; r.v[2 * i + 1] = t.y;
    }
    return r;
  }
  static __device__ __forceinline__ ab ld16(const float* p) { return run8(p); }
  static __device__ __forceinline__ void zero(ab& v) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v.v[i] = 0.f;
  }
  static __device__ __forceinline__ void set(ab& v, int i, float f) { v.v[i] = f; }
  static __device__ __forceinline__ void mma(f32x4& acc, const ab& a, const ab& b) {
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[s], b.v[s], acc, 0, 0, 0);
  }
};

__device__ __forceinline__ void store4(float* p, const f32x4& v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void store4(bf16_t* p, const f32x4& v) {
  bf16x4 o;
  o[0] = (bf16_t)v[0]; o[1] = (bf16_t)v[1]; o[2] = (bf16_t)v[2]; o[3] = (bf16_t)v[3];
  *reinterpret_cast<bf16x4*>(p) = o;
}

// ------------------------------------------------------------------------------------------ host
// The logical (n, c, t, h, w) clip of an sfk_u8_clip or an sfk_u8_pool_clip as the kernels index it: channel c of pixel
// (h, w) of frame t at byte src[n*sn + t*st + h*sh + w*sw + c] (src includes c0; the channel stride is 1).  Pooled: src is
// the pool, sn = 0, and frame t of clip n is pool frame pindex[n][t] (plane_base's lookup).
struct U8View {
  const uint8_t* src;
  int64_t sn, st, sh, sw;
  int n, c, t, h, w;
  const float* lut;
  const int32_t* crop;
  int pad;
  const int32_t* pindex;          // null: the frames are stacked
  int pframes, pfill;
};

inline int sfk_u8_view(const sfk_u8_clip* x, U8View& v) {
  if (!sfk_u8_clip_ok(x)) return SFK_ERR_INVALID;
  v = U8View{x->src + x->c0, x->sn, x->st, x->sh, x->sw, x->n, x->c, x->t, x->h, x->w, x->lut, x->crop, x->pad, nullptr, 0, 0};
  return SFK_OK;
}

inline int sfk_u8_view(const sfk_u8_pool_clip* x, U8View& v) {
  if (!sfk_u8_pool_clip_ok(x)) return SFK_ERR_INVALID;
  v = U8View{x->pool + x->c0, 0, x->frame_stride, x->row_stride, x->pixel_pitch, x->n, x->c, x->t, x->h, x->w,
             x->lut, x->crop, x->pad, x->index, x->frames, x->fill};
  return SFK_OK;
}

// the fields of K that only a uint8 source sets (the file's own fill has set the geometry and cleared these)
template <typename K>
inline void sfk_u8_view_tail(const U8View& v, K& k) {
  k.lut = v.lut; k.crop = v.crop; k.pad = v.pad;
  k.pindex = v.pindex; k.pframes = v.pframes; k.pfill = v.pfill;
}

}  // namespace
