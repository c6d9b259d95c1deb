// sfk_stem2d_fwd / sfk_stem2d_wgrad: the frames-as-channels stem of the res2d model (include/sfk_stem2d.h).
//
// Conv2d(T*C, cout, 7, 2, 3) over the clip's T frames of C channels, read in place through element strides.  With
// T = 10, C = 5 the reduction is K = 50 planes x 7 x 8 = 2800 (kw padded 7 -> 8): neither the patch of a tile
// (50 x 1480 elements) nor the filter (64 x 2816) fits in LDS, so the forward streams K in chunks of CP input planes.
//   K order = ((t*C + c)*7 + kh)*8 + kw (the stem layout of sfk_stem_conv_fwd): the 8 consecutive k of one lane are 8
//   consecutive input columns 2*wo .. 2*wo+7 of one patch row -> one 4-byte aligned LDS run.
//   forward : block = one 16x16 output tile x all cout (<= 64).  Per chunk: the CP planes' input patches and the
//             matching [64][CP*7*8] filter slice are staged in LDS; the NEXT chunk's global loads are issued into
//             registers before the current chunk's MFMAs (bf16: two LDS buffers, one barrier per chunk; f32: one buffer).
//             A = filter rows (co), B = patch runs (pixel on the lane); D[co][pixel].  BatchNorm partial sums per tile.
//   wgrad   : pixels are the reduction.  Block = (one input plane, a range of tiles): dY tile transposed into LDS
//             ([co][pixel]), the plane's patch beside it; A = 8 consecutive pixels of one co, B = the patch values of the
//             same 8 pixels for one (kh, kw).  dW[cout][plane][7][8] stays in registers over the tile range and is added
//             to dw with fp32 atomics (dw zeroed on the stream first).
// Both kernels also read the loader's HWC uint8 frames through a 256-entry f32 table with a per-clip crop shift
// (S = U8Lut, include/sfk_u8stem.h): the normalised, cropped float clip is then never written.
// The tile / patch geometry (TS, PR, PC, PLANE, NSLOT), ldsrc, plane_store, the MFMA operand fragments (Frag, store4) and the
// host's view of a uint8 source are stem_src.h's, shared with stem_conv.hip; the source offsets of a tile and the loads of a
// plane (PatchSlots, plane_fetch) are this file's own -- see stem_src.h for why.
#include "sfk_common.h"
#include "sfk_stem2d.h"
#include "stem_src.h"

namespace {

constexpr int CP = 4;             // planes per forward chunk: 28 filter rows = 7 K-steps of 32
constexpr int CR = CP * 7;
constexpr int WROW = CR * 8 + 8;  // staged filter row (+16 B for bf16: spreads the 16-byte reads over banks)
constexpr int WSEG = 64 * CR / 256;          // 8-element filter segments per thread and chunk (7)
constexpr int DTW = 256 + 8;      // transposed dY tile row (pixels)

struct S2K {
  const void* src;
  int64_t sn, st, sc, sh, sw;
  int n, t, c, h_in, w_in;
  int planes, kp, cout;
  int ho, wo, tiles_h, tiles_w, ntiles;
  FastDiv dtw, dth, dc, dpc;
  const void* w;
  void* y;                        // forward output / wgrad dY
  int yld, yoff;
  float* stats;
  float* dw;
  int tiles_per_block;
  const float* lut;               // S = U8Lut: value of each source byte (sc = 1: channel c at byte c)
  const int32_t* crop;            // S = U8Lut: [n][2] (top, left) or null; the frame pixel of (hi, wi) is (hi + top - pad, wi + left - pad)
  int pad;
  const int32_t* pindex;          // pooled S (include/sfk_u8stem_pool.h): [n][t] pool frame of (clip, frame); src is the pool, sn = 0
  int pframes;                    // pooled S: frames in the pool; an index outside [0, pframes) names a missing frame
  int pfill;                      // pooled S: the byte every pixel of a missing frame has
};

// (stem_conv.hip has the same struct with the masking at the use; keep the two in step otherwise)
struct PatchSlots {
  int64_t off[NSLOT];   // hi*sh + wi*sw of the current tile, 0 where !ok: readers add it to the plane's base as it is
  bool ok[NSLOT];
  template <typename S>
  __device__ __forceinline__ void set_tile(const S2K& k, int n, int ho0, int wo0) {
    // uint8 source: the crop shifts clip n's frame under the virtual clip; slots whose shifted pixel is outside the frame
    // are masked like the conv's own padding (any crop value is safe: their loads read the plane's first byte)
    int64_t dy = 0, dx = 0;
    if constexpr (sfk_is_u8<S>) {
      if (k.crop) {
        dy = (int64_t)k.crop[2 * n] - k.pad;
        dx = (int64_t)k.crop[2 * n + 1] - k.pad;
      }
    }
#pragma unroll
    for (int i = 0; i < NSLOT; ++i) {
      const int e = threadIdx.x + 256 * i;
      uint32_t r, c;
      k.dpc.divmod((uint32_t)e, r, c);
      const int hi = 2 * ho0 - 3 + (int)r, wi = 2 * wo0 - 3 + (int)c;
      if constexpr (sfk_is_u8<S>) {
        const int64_t y = hi + dy, x = wi + dx;
        ok[i] = e < PLANE && (unsigned)hi < (unsigned)k.h_in && (unsigned)wi < (unsigned)k.w_in &&
                (uint64_t)y < (uint64_t)k.h_in && (uint64_t)x < (uint64_t)k.w_in;
        off[i] = ok[i] ? y * k.sh + x * k.sw : 0;
      } else {
        ok[i] = e < PLANE && (unsigned)hi < (unsigned)k.h_in && (unsigned)wi < (unsigned)k.w_in;
        off[i] = ok[i] ? (int64_t)hi * k.sh + (int64_t)wi * k.sw : 0;
      }
    }
  }
};

// source offset of input plane pl = t*C + c of clip n; SFK_PLANE_PAD (-1) past the last plane.  Pooled S: frame t goes
// through the pool's index table (one lookup per plane, wave-uniform), and a frame that is not in the pool is the third
// state, SFK_PLANE_MISSING.
template <typename S = float>
__device__ __forceinline__ int64_t plane_base(const S2K& k, int pl, int n) {
  if (pl >= k.planes) return SFK_PLANE_PAD;
  uint32_t t, c;
  k.dc.divmod((uint32_t)pl, t, c);
  if constexpr (sfk_is_pool<S>) {
    const int slot = k.pindex[(int64_t)n * k.t + (int)t];
    if ((unsigned)slot >= (unsigned)k.pframes) return SFK_PLANE_MISSING;
    return (int64_t)slot * k.st + (int64_t)c * k.sc;
  } else {
    return (int64_t)n * k.sn + (int64_t)t * k.st + (int64_t)c * k.sc;
  }
}

// lut: S = U8Lut, the block's LDS copy of the table (one gather per element from LDS instead of a second global round trip)
template <typename S>
__device__ __forceinline__ void plane_fetch(const S2K& k, const PatchSlots& ps, int64_t base, float (&v)[NSLOT],
                                            const float* lut = nullptr) {
  const bool bok = base >= 0;              // branch-free: padding slots read the plane's first element, zeroed by a select
  const int64_t b = bok ? base : 0;
  // pooled S: a missing frame's slots load a byte of pool frame 0 like padding does, and a select puts the fill byte in its
  // place in front of the table lookup -- lut[fill] wherever the slot is inside the conv input and the crop
  const bool miss = sfk_is_pool<S> && base == SFK_PLANE_MISSING;
  const bool live = sfk_is_pool<S> ? (bok || miss) : bok;
#pragma unroll
  for (int i = 0; i < NSLOT; ++i) {
    float x;
    if constexpr (sfk_is_pool<S>) {
      const uint32_t u = static_cast<const uint8_t*>(k.src)[b + ps.off[i]];
      x = lut[miss ? (uint32_t)k.pfill : u];
    } else if constexpr (sfk_is_u8<S>) x = lut[static_cast<const uint8_t*>(k.src)[b + ps.off[i]]];   // the table's f32, as the float clip holds it
    else x = ldsrc<S>(k.src, b + ps.off[i]);
    v[i] = (live && ps.ok[i]) ? x : 0.f;
  }
}

__device__ __forceinline__ void tile_coords(const S2K& k, int tile, int& n, int& ho0, int& wo0) {
  uint32_t q1, tw, n_, th;
  k.dtw.divmod((uint32_t)tile, q1, tw);
  k.dth.divmod(q1, n_, th);
  n = (int)n_; ho0 = (int)th * TS; wo0 = (int)tw * TS;
}

// ------------------------------------------------------------------------------------------ forward
// grid = tiles; one 16x16 output tile per block, wave w owns output rows 4w..4w+3, all 64 (padded) output channels.
template <typename T, typename S, int NB>
__global__ __launch_bounds__(256) void stem2d_fwd_kernel(const S2K k) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* wl = reinterpret_cast<T*>(smem);                         // [NB][64][WROW]
  T* patch = wl + NB * 64 * WROW;                             // [NB][CP][PLANE]
  float* red = reinterpret_cast<float*>(patch + NB * CP * PLANE);   // [4 waves][64][2]
  float* lut = red + 4 * 64 * 2;                              // S = U8Lut: [256]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  if constexpr (sfk_is_u8<S>) {
    lut[tid] = k.lut[tid];
    __syncthreads();
  }
  const int tile = blockIdx.x;
  int n, ho0, wo0;
  tile_coords(k, tile, n, ho0, wo0);
  PatchSlots ps;
  ps.set_tile<S>(k, n, ho0, wo0);
  const T* wp = static_cast<const T*>(k.w);
  const int krows8 = k.kp / 8;                                // 8-element rows of the global filter row

  float pv[CP][NSLOT];
  typename Frag<T>::ab wv[WSEG];
  auto fetch = [&](int c) {
    int64_t base[CP];
#pragma unroll
    for (int q = 0; q < CP; ++q) base[q] = plane_base<S>(k, c * CP + q, n);
#pragma unroll
    for (int q = 0; q < CP; ++q) plane_fetch<S>(k, ps, base[q], pv[q], lut);
#pragma unroll
    for (int e = 0; e < WSEG; ++e) {
      const int idx = tid + 256 * e, row = idx / CR, seg = idx - row * CR, r8 = c * CR + seg;
      if (row < k.cout && r8 < krows8) wv[e] = Frag<T>::ld16(wp + (int64_t)row * k.kp + r8 * 8);
      else Frag<T>::zero(wv[e]);
    }
  };
  auto put = [&](int b) {
#pragma unroll
    for (int q = 0; q < CP; ++q) plane_store<T>(patch + (b * CP + q) * PLANE, pv[q]);
#pragma unroll
    for (int e = 0; e < WSEG; ++e) {
      const int idx = tid + 256 * e, row = idx / CR, seg = idx - row * CR;
      *reinterpret_cast<typename Frag<T>::ab*>(wl + (b * 64 + row) * WROW + seg * 8) = wv[e];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = (k.planes + CP - 1) / CP;
  fetch(0);
  for (int c = 0; c < nchunks; ++c) {
    const int b = NB == 2 ? (c & 1) : 0;
    put(b);
    __syncthreads();                                          // chunk c staged (NB = 2: and chunk c-1's buffer free again)
    if (c + 1 < nchunks) fetch(c + 1);                        // in flight under this chunk's MFMAs
    const int np = min(CP, k.planes - c * CP), rows = 7 * np, steps = (rows + 3) / 4;
    for (int s = 0; s < steps; ++s) {
      int rk = 4 * s + g;                                     // K row of this lane group in the chunk: (plane, kh)
      if (rk >= rows) rk = rows - 1;                          // padded rows multiply zero filter rows; keep the read in bounds
      const int pln = rk / 7, kh = rk - 7 * pln;
      const T* prow = patch + (b * CP + pln) * PLANE + kh * PC + 2 * l15;
      typename Frag<T>::ab a[4], bb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = Frag<T>::ld16(wl + (b * 64 + 16 * i + l15) * WROW + 32 * s + 8 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) bb[j] = Frag<T>::run8(prow + 2 * (4 * wave + j) * PC);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) Frag<T>::mma(acc[i][j], a[i], bb[j]);
    }
    if (NB == 1) __syncthreads();                             // one buffer: everyone is done reading it
  }

  // epilogue: lane holds co = 16i + 4g + r for pixel (row 4*wave + j, col l15)
  T* yp = static_cast<T*>(k.y);
  const int wo = wo0 + l15;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ho = ho0 + 4 * wave + j;
    if (!(ho < k.ho && wo < k.wo)) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};   // outside the map: not stored, not counted
      continue;
    }
    const int64_t poff = (((int64_t)n * k.ho + ho) * k.wo + wo) * k.yld + k.yoff;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int co = 16 * i + 4 * g;
      if (co < k.cout) store4(yp + poff + co, acc[i][j]);
    }
  }
  if (k.stats) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = acc[i][j][r];
          s1 += v;
          s2 += v * v;
        }
#pragma unroll
        for (int sft = 1; sft < 16; sft <<= 1) {
          s1 += __shfl_xor(s1, sft);
          s2 += __shfl_xor(s2, sft);
        }
        if (l15 == 0) {
          const int col = 16 * i + 4 * g + r;
          red[(wave * 64 + col) * 2 + 0] = s1;
          red[(wave * 64 + col) * 2 + 1] = s2;
        }
      }
    }
    __syncthreads();
    if (tid < k.cout) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int w_ = 0; w_ < 4; ++w_) {
        s1 += red[(w_ * 64 + tid) * 2 + 0];
        s2 += red[(w_ * 64 + tid) * 2 + 1];
      }
      float* o = k.stats + ((int64_t)tile * k.cout + tid) * 2;
      o[0] = s1;
      o[1] = s2;
    }
  }
}

// ------------------------------------------------------------------------------------------ filter gradient
// grid = (plane, tile range).  Wave w owns filter columns 16w..16w+15 = (kh = 2w + l15/8, kw = l15%8) of the plane (kh = 7
// is padding), all 64 output channels.  K-step s of a tile = pixels 32s..32s+31 = output rows 2s, 2s+1.
template <typename T, typename S>
__global__ __launch_bounds__(256) void stem2d_wgrad_kernel(const S2K k) {
  constexpr int VEC = DT<T>::VEC;
  __shared__ __attribute__((aligned(16))) T dyt[64 * DTW];   // [co][pixel of the tile]
  __shared__ __attribute__((aligned(16))) T patch[PLANE];
  __shared__ float lut[sfk_is_u8<S> ? 256 : 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  if constexpr (sfk_is_u8<S>) {
    lut[tid] = k.lut[tid];
    __syncthreads();
  }
  const int pl = blockIdx.x;
  const int tile0 = blockIdx.y * k.tiles_per_block;
  const int tile1 = min(k.ntiles, tile0 + k.tiles_per_block);
  const int kh = 2 * wave + (l15 >> 3), kw = l15 & 7;
  const T* dy = static_cast<const T*>(k.y);
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  PatchSlots ps;
  for (int tile = tile0; tile < tile1; ++tile) {
    int n, ho0, wo0;
    tile_coords(k, tile, n, ho0, wo0);
    ps.set_tile<S>(k, n, ho0, wo0);
    float v[NSLOT];
    plane_fetch<S>(k, ps, plane_base<S>(k, pl, n), v, lut);
    // dY of pixel tid of the tile (zero outside the map and for co >= cout)
    const int ho = ho0 + (tid >> 4), wo = wo0 + (tid & 15);
    const bool pok = ho < k.ho && wo < k.wo;
    Vec16<T> d[64 / VEC];
    const int64_t poff = (((int64_t)n * k.ho + (pok ? ho : 0)) * k.wo + (pok ? wo : 0)) * k.yld + k.yoff;
#pragma unroll
    for (int q = 0; q < 64 / VEC; ++q) {
      if (pok && q * VEC < k.cout) d[q].load(dy + poff + q * VEC);
      else d[q].zero();
    }
    __syncthreads();                                          // previous tile's LDS reads are done
    plane_store<T>(patch, v);
#pragma unroll
    for (int q = 0; q < 64 / VEC; ++q)
#pragma unroll
      for (int e = 0; e < VEC; ++e) dyt[(q * VEC + e) * DTW + tid] = (T)d[q].get(e);
    __syncthreads();
#pragma unroll 2
    for (int s = 0; s < 8; ++s) {
      const int pr = 2 * s + (g >> 1), pc0 = 8 * (g & 1);    // this lane group's 8 pixels: row pr, cols pc0..pc0+7
      typename Frag<T>::ab bv;
      if (kh < 7) {
        const T* prow = patch + (2 * pr + kh) * PC + 2 * pc0 + kw;
#pragma unroll
        for (int e = 0; e < 8; ++e) Frag<T>::set(bv, e, (float)prow[2 * e]);
      } else {
        Frag<T>::zero(bv);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const typename Frag<T>::ab a = Frag<T>::ld16(dyt + (16 * i + l15) * DTW + 32 * s + 8 * g);
        Frag<T>::mma(acc[i], a, bv);
      }
    }
  }
  // lane holds dW[co = 16i + 4g + r][kh][kw]
  if (kh < 7 && kw < 7) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = 16 * i + 4 * g + r;
        if (co < k.cout) unsafeAtomicAdd(k.dw + (int64_t)co * k.kp + (pl * 7 + kh) * 8 + kw, acc[i][r]);
      }
  }
}

constexpr int LDS_FWD = 64 * WROW * 2 * 2 + CP * PLANE * 2 * 2 + 4 * 64 * 2 * 4;   // 85120 B either way (bf16 x 2 buffers, f32 x 1)
constexpr int LDS_LUT = 256 * 4;                                                   // + the table of the uint8 source

// bytes: the source is a uint8 view (src_dtype is not read)
int fill(const sfk_stem2d_src* s, const sfk_fmap* y, S2K& k, bool bytes = false) {
  if (!s || !y || s->struct_size != sizeof(sfk_stem2d_src)) return SFK_ERR_INVALID;
  if (!s->src || !sfk_fmap_ok(y)) return SFK_ERR_INVALID;
  if (!bytes && s->src_dtype != SFK_F32 && s->src_dtype != SFK_BF16) return SFK_ERR_INVALID;
  if (s->n <= 0 || s->t <= 0 || s->c <= 0 || s->h_in <= 0 || s->w_in <= 0) return SFK_ERR_INVALID;
  if (s->sn < 0 || s->st < 0 || s->sc < 0 || s->sh < 0 || s->sw < 0) return SFK_ERR_INVALID;
  const int ho = (s->h_in + 6 - 7) / 2 + 1, wo = (s->w_in + 6 - 7) / 2 + 1;
  if (y->n != s->n || y->t != 1 || y->h != ho || y->w != wo) return SFK_ERR_INVALID;
  if (y->c % 4 || y->c > 64 || !sfk_fmap_vec_ok(y)) return SFK_ERR_UNSUPPORTED;
  const int64_t planes = (int64_t)s->t * s->c;
  if (planes > 4096) return SFK_ERR_UNSUPPORTED;
  const int64_t ntiles = (int64_t)s->n * ((ho + TS - 1) / TS) * ((wo + TS - 1) / TS);
  if (ntiles >= (1ll << 31) || sfk_fmap_pixels(y) * y->ld >= (1ll << 62)) return SFK_ERR_UNSUPPORTED;
  k = S2K{};
  k.src = s->src;
  k.sn = s->sn; k.st = s->st; k.sc = s->sc; k.sh = s->sh; k.sw = s->sw;
  k.n = s->n; k.t = s->t; k.c = s->c; k.h_in = s->h_in; k.w_in = s->w_in;
  k.planes = (int)planes;
  k.kp = (int)((planes * 7 + 3) / 4 * 4 * 8);
  k.cout = y->c;
  k.ho = ho; k.wo = wo;
  k.tiles_h = (ho + TS - 1) / TS; k.tiles_w = (wo + TS - 1) / TS;
  k.ntiles = (int)ntiles;
  k.dtw.set(k.tiles_w); k.dth.set(k.tiles_h); k.dc.set(s->c); k.dpc.set(PC);
  k.y = y->ptr; k.yld = y->ld; k.yoff = y->c_off;
  k.lut = nullptr; k.crop = nullptr; k.pad = 0;
  return SFK_OK;
}

// S2K of a source descriptor under a map: an sfk_stem2d_src as it is ...
int fill_src(const sfk_stem2d_src* s, const sfk_fmap* y, S2K& k) { return fill(s, y, k); }

// ... and either uint8 descriptor through its view (stem_src.h): channel c at byte c of the view's src
template <typename X>
int fill_src(const X* x, const sfk_fmap* y, S2K& k) {
  U8View v;
  if (sfk_u8_view(x, v) != SFK_OK) return SFK_ERR_INVALID;
  sfk_stem2d_src s{};
  s.struct_size = sizeof(sfk_stem2d_src);
  s.src = v.src;
  s.sn = v.sn; s.st = v.st; s.sc = 1; s.sh = v.sh; s.sw = v.sw;
  s.n = v.n; s.t = v.t; s.c = v.c; s.h_in = v.h; s.w_in = v.w;
  const int st = fill(&s, y, k, true);
  if (st == SFK_OK) sfk_u8_view_tail(v, k);
  return st;
}

template <typename S>
int launch_fwd(const S2K& k, const sfk_fmap* y, hipStream_t hs) {
  const dim3 grid((unsigned)k.ntiles), block(256);
  const int lds = LDS_FWD + (sfk_is_u8<S> ? LDS_LUT : 0);
#define SFK_S2_FWD(T, NB)                                                                                               \
  do {                                                                                                                  \
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stem2d_fwd_kernel<T, S, NB>),                             \
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);                                         \
    hipLaunchKernelGGL((stem2d_fwd_kernel<T, S, NB>), grid, block, lds, hs, k);                                         \
  } while (0)
  if (y->dtype == SFK_BF16) SFK_S2_FWD(bf16_t, 2);
  else SFK_S2_FWD(float, 1);
#undef SFK_S2_FWD
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

template <typename S>
int launch_wgrad(S2K& k, const sfk_fmap* dy, hipStream_t hs) {
  if (hipMemsetAsync(k.dw, 0, (size_t)k.cout * k.kp * sizeof(float), hs) != hipSuccess) return SFK_ERR_LAUNCH;
  // about 2048 blocks: planes x tile ranges
  int split = (2048 + k.planes - 1) / k.planes;
  if (split > k.ntiles) split = k.ntiles;
  k.tiles_per_block = (k.ntiles + split - 1) / split;
  split = (k.ntiles + k.tiles_per_block - 1) / k.tiles_per_block;
  const dim3 grid((unsigned)k.planes, (unsigned)split), block(256);
  if (dy->dtype == SFK_BF16) hipLaunchKernelGGL((stem2d_wgrad_kernel<bf16_t, S>), grid, block, 0, hs, k);
  else hipLaunchKernelGGL((stem2d_wgrad_kernel<float, S>), grid, block, 0, hs, k);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

// The entry points over a source descriptor X read as source tag S: the argument checks in their order (the map before
// the filter), then the launch
template <typename S, typename X>
int stem2d_fwd(const X* x, const void* w, const sfk_fmap* y, float* stats, sfk_stream_t stream) {
  S2K k;
  const int st = fill_src(x, y, k);
  if (st != SFK_OK) return st;
  if (!w) return SFK_ERR_INVALID;
  if ((((uintptr_t)w) & 15) != 0) return SFK_ERR_UNSUPPORTED;
  k.w = w;
  k.stats = stats;
  return launch_fwd<S>(k, y, static_cast<hipStream_t>(stream));
}

template <typename S, typename X>
int stem2d_wgrad(const X* x, const sfk_fmap* dy, float* dw, sfk_stream_t stream) {
  S2K k;
  const int st = fill_src(x, dy, k);
  if (st != SFK_OK) return st;
  if (!dw) return SFK_ERR_INVALID;
  k.dw = dw;
  return launch_wgrad<S>(k, dy, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" int sfk_stem2d_abi_version(void) { return SFK_STEM2D_ABI_VERSION; }

extern "C" int sfk_stem2d_tiles(const sfk_stem2d_src* s, const sfk_fmap* y) {
  S2K k;
  const int st = fill(s, y, k);
  return st != SFK_OK ? st : k.ntiles;
}

// (a null or mistyped s: either instantiation's fill refuses it)
extern "C" int sfk_stem2d_fwd(const sfk_stem2d_src* s, const void* w, const sfk_fmap* y, float* stats, sfk_stream_t stream) {
  return s && s->src_dtype == SFK_BF16 ? stem2d_fwd<bf16_t>(s, w, y, stats, stream) : stem2d_fwd<float>(s, w, y, stats, stream);
}

extern "C" int sfk_stem2d_wgrad(const sfk_stem2d_src* s, const sfk_fmap* dy, float* dw, sfk_stream_t stream) {
  return s && s->src_dtype == SFK_BF16 ? stem2d_wgrad<bf16_t>(s, dy, dw, stream) : stem2d_wgrad<float>(s, dy, dw, stream);
}

// ------------------------------------------------------------------------------------------ uint8 frames (sfk_u8stem.h)
extern "C" int sfk_u8stem2d_fwd(const sfk_u8_clip* x, const void* w, const sfk_fmap* y, float* stats, sfk_stream_t stream) {
  return stem2d_fwd<U8Lut>(x, w, y, stats, stream);
}

extern "C" int sfk_u8stem2d_wgrad(const sfk_u8_clip* x, const sfk_fmap* dy, float* dw, sfk_stream_t stream) {
  return stem2d_wgrad<U8Lut>(x, dy, dw, stream);
}

// ------------------------------------------------------------------------------------------ uint8 frames in a frame pool (sfk_u8stem_pool.h)
extern "C" int sfk_u8pstem2d_fwd(const sfk_u8_pool_clip* x, const void* w, const sfk_fmap* y, float* stats, sfk_stream_t stream) {
  return stem2d_fwd<U8PoolLut>(x, w, y, stats, stream);
}

extern "C" int sfk_u8pstem2d_wgrad(const sfk_u8_pool_clip* x, const sfk_fmap* dy, float* dw, sfk_stream_t stream) {
  return stem2d_wgrad<U8PoolLut>(x, dy, dw, stream);
}
