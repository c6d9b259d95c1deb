// sfk_u8_pool_gather_warp (include/sfk_warp.h): the normalised (n, t, c, h, w) clip batch built from a pool of uint8 HWC
// frames, every clip sampled bilinearly through a 2 x 3 matrix of its own (rotation, scale, shear, flip, translation), zeros
// outside the frame.  The sibling of u8_pool_gather.hip's kernel, which can only shift; integer-translation rows reproduce
// that kernel bit for bit.  The header states the contract; every product, sum and difference of it is rounded on its own, so
// contraction is off for this file, as in optim_elem.h.
#include <math.h>

#include "sfk_common.h"
#include "sfk_warp.h"

#pragma clang fp contract(off)

namespace {

constexpr int TH = SFK_WARP_TILE_H, TW = SFK_WARP_TILE_W;
constexpr int LUT_COPIES = 8;                            // lut[e] at s_lut[e*8 + (lane & 7)]: lanes 8 apart alone can meet on a bank
constexpr int LUT_BYTES = 256 * LUT_COPIES * (int)sizeof(float);   // the LDS copies of lut, ahead of the staged box
constexpr int PX = 4;                                    // pixels of one thread, consecutive in x
enum { MODE_LDS = 0, MODE_GLOBAL = 1, MODE_CONST = 2 };  // where a tile's taps come from: the staged box, global memory, nowhere

struct Mat { float a, b, c, d, e, f; };

// the contract's source position of output pixel (x, y): three roundings per coordinate, in this order
__host__ __device__ __forceinline__ void warp_xy(const Mat& m, int x, int y, float& xs, float& ys) {
  const float xf = (float)x, yf = (float)y;
  xs = (m.a * xf + m.b * yf) + m.c;
  ys = (m.d * xf + m.e * yf) + m.f;
}

// LDS bytes of one staged row of `cols` pixels: its span, (cols - 1)*pitch + c, behind a shift of up to 15 bytes, in 16-byte units
__host__ __device__ __forceinline__ int64_t stage_row_bytes(int cols, int pitch, int c) {
  return (((int64_t)(cols - 1) * pitch + c) + 15 + 15) / 16 * 16;
}
// what a launch stages at most: the whole frame when that is less than SFK_WARP_LDS_BYTES
__host__ __device__ __forceinline__ int64_t stage_budget(int h, int w, int pitch, int c) {
  const int64_t full = (int64_t)h * stage_row_bytes(w, pitch, c);
  return full < SFK_WARP_LDS_BYTES ? full : SFK_WARP_LDS_BYTES;
}

// source pixels [bx0, bx0 + cols) x [by0, by0 + rows), rs LDS bytes a row; inner: every tap of every pixel of the tile lies in the frame
struct Box { int mode, bx0, by0, cols, rows; int64_t rs; bool inner; };

// The source box of output tile [tx0, tx1] x [ty0, ty1] (inclusive).  fl(a*x) is monotone in x, a sum with a fixed term and its
// rounding are monotone, so xs and ys are monotone in x at fixed y and in y at fixed x -- overflow to an infinity included --
// and their extremes over the tile are at its corners.  A NaN inside the tile needs inf - inf, whose two infinities are then
// also met at a corner, so corners that are all numbers bound a tile of numbers.  Every tap that lies in the frame then lies in
// [floor(lo), floor(hi) + 1], clipped to the frame.  The box is made of INTEGERS clamped to the frame before anything is
// addressed with them, so no matrix can move the staging out of the frame, whatever the reasoning above is worth.
// MODE_CONST: no pixel of the tile passes the range test (all zeros).  MODE_GLOBAL: a corner is NaN, or the box needs more
// than budget bytes: the taps are taken from global memory, each behind its own integer in-frame test.
__host__ __device__ inline Box tile_box(const Mat& m, int tx0, int ty0, int tx1, int ty1, int h, int w, int pitch, int c,
                                        int64_t budget) {
  float xs[4], ys[4];
  warp_xy(m, tx0, ty0, xs[0], ys[0]);
  warp_xy(m, tx1, ty0, xs[1], ys[1]);
  warp_xy(m, tx0, ty1, xs[2], ys[2]);
  warp_xy(m, tx1, ty1, xs[3], ys[3]);
  float xlo = xs[0], xhi = xs[0], ylo = ys[0], yhi = ys[0];
  bool nan = false;
  for (int k = 0; k < 4; ++k) {
    nan = nan || !(xs[k] == xs[k]) || !(ys[k] == ys[k]);
    xlo = xs[k] < xlo ? xs[k] : xlo;
    xhi = xs[k] > xhi ? xs[k] : xhi;
    ylo = ys[k] < ylo ? ys[k] : ylo;
    yhi = ys[k] > yhi ? ys[k] : yhi;
  }
  Box b = {MODE_GLOBAL, 0, 0, 0, 0, 0, false};
  if (nan) return b;
  const float wf = (float)w, hf = (float)h;
  if (!(xhi > -1.f && xlo < wf && yhi > -1.f && ylo < hf)) {
    b.mode = MODE_CONST;
    return b;
  }
  b.inner = xlo >= 0.f && xhi < wf - 1.f && ylo >= 0.f && yhi < hf - 1.f;      // floor >= 0 and floor + 1 <= w - 1 for every pixel
  // conversions only of values known to lie in (-1, w) resp. (-1, h)
  int bx0 = xlo <= 0.f ? 0 : (int)floorf(xlo), bx1 = xhi >= wf - 1.f ? w - 1 : (int)floorf(xhi) + 1;
  int by0 = ylo <= 0.f ? 0 : (int)floorf(ylo), by1 = yhi >= hf - 1.f ? h - 1 : (int)floorf(yhi) + 1;
  bx0 = bx0 < 0 ? 0 : bx0 > w - 1 ? w - 1 : bx0;
  by0 = by0 < 0 ? 0 : by0 > h - 1 ? h - 1 : by0;
  bx1 = bx1 < bx0 ? bx0 : bx1 > w - 1 ? w - 1 : bx1;
  by1 = by1 < by0 ? by0 : by1 > h - 1 ? h - 1 : by1;
  b.bx0 = bx0, b.by0 = by0, b.cols = bx1 - bx0 + 1, b.rows = by1 - by0 + 1;
  b.rs = stage_row_bytes(b.cols, pitch, c);
  b.mode = (int64_t)b.rows * b.rs <= budget ? MODE_LDS : MODE_GLOBAL;
  return b;
}

// What the sampling of one tile reads its taps through.  off: the tap's byte offset, channel included -- into the staged box
// (MODE_LDS), from the frame's byte (0, 0, c0) (MODE_GLOBAL).  A tap outside the frame is 0.  From global memory it is not
// read; from the staged box byte 0 is read in its place and dropped, which keeps the LDS path free of branches.  MASKED ==
// false (the tile's corners say that every tap of every pixel lies in the frame): no test at all.
template <int MODE, bool MASKED, typename OffT>
struct Taps {
  const uint8_t* base;        // the staged box | the frame's byte (0, 0, c0) | unused
  const float* s_lut;         // this lane's copy of the table: entry e at s_lut[e * LUT_COPIES]
  float fv;                   // lut[fill]: every tap of a missing frame
  __device__ __forceinline__ float operator()(bool valid, OffT off) const {
    if (MODE == MODE_CONST) return valid ? fv : 0.f;
    if (MODE == MODE_GLOBAL) return valid ? s_lut[(int)base[off] * LUT_COPIES] : 0.f;
    if (!MASKED) return s_lut[(int)base[off] * LUT_COPIES];
    const float v = s_lut[(int)base[valid ? off : (OffT)0] * LUT_COPIES];
    return valid ? v : 0.f;
  }
};

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// One thread: PX consecutive pixels of one tile row, every parts-th channel (bf16: channel pair) from `part`.  The pixels' tap
// offsets, masks and fractions are formed once and serve all its channels.  f32: the four values are one 16-byte store.  bf16:
// four values are 8 bytes, so a thread samples TWO channels a turn and trades one of them with the lane beside it, which holds
// the other half of the same 8 pixels: the even lane stores the first channel's 16 bytes, the odd lane the second's.
template <typename T, int MODE, bool MASKED, typename OffT>
__device__ __forceinline__ void sample(const Taps<MODE, MASKED, OffT>& taps, const Mat& m, int x, int y, int h, int w, int pitch, int c,
                                       int part, int parts, int bx0, int by0, int rs, int s0, int rsl, int64_t row_stride,
                                       T* __restrict__ op, int64_t plane) {
  constexpr int V = PX, VS = DT<T>::VEC;               // pixels a thread, elements a 16-byte store
  const float wf = (float)w, hf = (float)h;
  float fx[V], fy[V];
  OffT o0[V], o1[V];          // the taps of column x0 in rows y0 and y0 + 1, channel 0; column x0 + 1 is pitch further
  unsigned mask[V];           // bit 0: (y0, x0) lies in the frame, 1: (y0, x0 + 1), 2: (y0 + 1, x0), 3: (y0 + 1, x0 + 1)
#pragma unroll
  for (int k = 0; k < V; ++k) {
    fx[k] = 0.f, fy[k] = 0.f, o0[k] = 0, o1[k] = 0, mask[k] = 0;
    float xs, ys;
    warp_xy(m, x + k, y, xs, ys);
    if (!MASKED || (x + k < w && xs > -1.f && xs < wf && ys > -1.f && ys < hf)) {
      const float xf0 = floorf(xs), yf0 = floorf(ys);
      fx[k] = xs - xf0, fy[k] = ys - yf0;
      const int ix = (int)xf0, iy = (int)yf0;          // in [-1, w - 1] and [-1, h - 1]
      const bool xa = ix >= 0, xb = ix + 1 < w, ya = iy >= 0, yb = iy + 1 < h;
      mask[k] = !MASKED ? 15u
                        : (unsigned)(ya && xa) | (unsigned)(ya && xb) << 1 | (unsigned)(yb && xa) << 2 | (unsigned)(yb && xb) << 3;
      if (MODE == MODE_LDS) {                          // row r of the box lies at r*rs + its own 16-byte phase
        const int r0 = iy - by0, r1 = r0 + 1, dx = (ix - bx0) * pitch;
        o0[k] = (OffT)(r0 * rs + ((s0 + r0 * rsl) & 15) + dx);
        o1[k] = (OffT)(r1 * rs + ((s0 + r1 * rsl) & 15) + dx);
      } else if (MODE == MODE_GLOBAL) {
        o0[k] = (OffT)((int64_t)iy * row_stride + (int64_t)ix * pitch);
        o1[k] = (OffT)(o0[k] + row_stride);
      }
    }
  }
  auto value = [&](int k, int ch) -> float {
    const float v00 = taps(mask[k] & 1u, o0[k] + ch), v01 = taps(mask[k] & 2u, o0[k] + pitch + ch);
    const float v10 = taps(mask[k] & 4u, o1[k] + ch), v11 = taps(mask[k] & 8u, o1[k] + pitch + ch);
    const float top = v00 + fx[k] * (v01 - v00);
    const float bot = v10 + fx[k] * (v11 - v10);
    return top + fy[k] * (bot - top);
  };
  const bool vec = w % VS == 0;                        // every VS-group of a row starts 16-byte aligned (out is, and w % VS == 0)
  if (VS == 2 * V && vec) {
    // bf16.  The lanes 2j and 2j + 1 hold pixels [x, x + 4) and [x + 4, x + 8) of one row (w % 8 == 0: both or neither are inside
    // the frame) and run this loop together: `part` is uniform in a wave.
    const bool odd = threadIdx.x & 1;
    for (int ch = 2 * part; ch < c; ch += 2 * parts) {
      const bool two = ch + 1 < c;                     // (uniform: the last turn of an odd channel count has no second channel)
      bf16x4 pa, pb;
#pragma unroll
      for (int k = 0; k < V; ++k) pa[k] = (bf16_t)value(k, ch);
#pragma unroll
      for (int k = 0; k < V; ++k) pb[k] = (bf16_t)(two ? value(k, ch + 1) : 0.f);
      const u32x2 a = __builtin_bit_cast(u32x2, pa), b = __builtin_bit_cast(u32x2, pb);
      const u32x2 send = odd ? a : b;
      const u32x2 recv = {(unsigned)__shfl_xor((int)send[0], 1), (unsigned)__shfl_xor((int)send[1], 1)};
      if (!odd) {
        *reinterpret_cast<u32x4*>(op + (int64_t)ch * plane) = u32x4{a[0], a[1], recv[0], recv[1]};
      } else if (two) {
        *reinterpret_cast<u32x4*>(op - V + (int64_t)(ch + 1) * plane) = u32x4{recv[0], recv[1], b[0], b[1]};
      }
    }
    return;
  }
  for (int ch = part; ch < c; ch += parts) {
    float r[V];
#pragma unroll
    for (int k = 0; k < V; ++k) r[k] = value(k, ch);
    T* o = op + (int64_t)ch * plane;
    if (VS == V && vec) {
      Vec16<T> v;
#pragma unroll
      for (int k = 0; k < V; ++k) v.set(k, r[k]);
      v.store(o);
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (x + k < w) o[k] = (T)r[k];
    }
  }
}

// One output tile of TH x TW pixels of one (n, t), all c channels, per block.  index[n][t], warp[n] and everything derived
// from them are block-uniform.
template <typename T>
__global__ __launch_bounds__(256) void u8_pool_warp_kernel(const uint8_t* __restrict__ pool, int64_t frame_stride,
                                                           int64_t row_stride, int pitch, int frames, int t, int h, int w, int c0,
                                                           int c, const int32_t* __restrict__ index,
                                                           const float* __restrict__ warp, const float* __restrict__ lut, int fill,
                                                           int tiles_x, int tiles_y, int budget, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float* s_lut = reinterpret_cast<float*>(smem);
  uint8_t* stage = smem + LUT_BYTES;
#pragma unroll
  for (int i = threadIdx.x; i < 256 * LUT_COPIES; i += 256) s_lut[i] = lut[i / LUT_COPIES];
  const int b = blockIdx.x;
  const int tx = b % tiles_x, ty = (b / tiles_x) % tiles_y, nt = b / (tiles_x * tiles_y);
  const int f = index ? index[nt] : nt;                 // NULL: the stacked batch's own frame
  const bool miss = f < 0 || f >= frames;
  const float* mp = warp + (int64_t)(nt / t) * 6;
  const Mat m = {mp[0], mp[1], mp[2], mp[3], mp[4], mp[5]};
  const int tx0 = tx * TW, ty0 = ty * TH;
  const int tx1 = (tx0 + TW < w ? tx0 + TW : w) - 1, ty1 = (ty0 + TH < h ? ty0 + TH : h) - 1;
  const Box box = tile_box(m, tx0, ty0, tx1, ty1, h, w, pitch, c, budget);
  const int mode = miss ? MODE_CONST : box.mode;        // a missing frame reads nothing
  const uint8_t* fb = pool;
  int s0 = 0;
  const int rsl = (int)(row_stride & 15);
  if (mode != MODE_CONST) fb = pool + (int64_t)f * frame_stride + c0;          // byte (f, 0, 0, c0)
  if (mode == MODE_LDS) {
    // rows [by0, by0 + rows) of the box, each from channel c0 of pixel bx0 to channel c0 + c - 1 of pixel bx0 + cols - 1: one
    // wave a row, 16-byte units at the phase LDS and global addresses share, byte by byte at the two ends
    const int64_t span = (int64_t)(box.cols - 1) * pitch + c;
    const uint8_t* sp0 = fb + (int64_t)box.by0 * row_stride + (int64_t)box.bx0 * pitch;
    s0 = (int)(reinterpret_cast<uintptr_t>(sp0) & 15);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wave; r < box.rows; r += 4) {
      const uint8_t* sp = sp0 + (int64_t)r * row_stride;
      const int shift = (s0 + r * rsl) & 15;            // = sp & 15
      uint8_t* row = stage + (int64_t)r * box.rs;
      const int64_t end = (int64_t)shift + span;        // staged bytes are row[shift .. end), end <= rs
      for (int64_t i = (int64_t)lane * 16; i < end; i += 64 * 16) {
        if (i >= shift && i + 16 <= end) {
          *reinterpret_cast<uint4*>(row + i) = *reinterpret_cast<const uint4*>(sp + (i - shift));
        } else {
          const int64_t j0 = i < shift ? shift : i, j1 = i + 16 < end ? i + 16 : end;
          for (int64_t j = j0; j < j1; ++j) row[j] = sp[j - shift];
        }
      }
    }
  }
  __syncthreads();
  constexpr int V = PX, GX = TW / V, G = TH * GX, P = 256 / G;                // pixel groups of a tile, channel parts
  const int g = threadIdx.x % G, part = threadIdx.x / G;
  const int x = tx0 + (g % GX) * V, y = ty0 + g / GX;
  if (x >= w || y >= h) return;
  const int64_t plane = (int64_t)h * w;
  T* op = out + (int64_t)nt * c * plane + (int64_t)y * w + x;                 // element (ch, x + k) at op[ch*plane + k]
  const float fv = s_lut[fill * LUT_COPIES];
  const float* my_lut = s_lut + (threadIdx.x & (LUT_COPIES - 1));
  if (mode == MODE_LDS && box.inner && w % DT<T>::VEC == 0) {    // the common tile: inside the frame, no test left
    sample<T, MODE_LDS, false, int>(Taps<MODE_LDS, false, int>{stage, my_lut, fv}, m, x, y, h, w, pitch, c, part, P, box.bx0,
                                    box.by0, (int)box.rs, s0, rsl, row_stride, op, plane);
  } else if (mode == MODE_LDS) {
    sample<T, MODE_LDS, true, int>(Taps<MODE_LDS, true, int>{stage, my_lut, fv}, m, x, y, h, w, pitch, c, part, P, box.bx0,
                                   box.by0, (int)box.rs, s0, rsl, row_stride, op, plane);
  } else if (mode == MODE_GLOBAL) {
    sample<T, MODE_GLOBAL, true, int64_t>(Taps<MODE_GLOBAL, true, int64_t>{fb, my_lut, fv}, m, x, y, h, w, pitch, c, part, P, 0, 0,
                                          0, 0, 0, row_stride, op, plane);
  } else {
    sample<T, MODE_CONST, true, int>(Taps<MODE_CONST, true, int>{nullptr, my_lut, fv}, m, x, y, h, w, pitch, c, part, P, 0, 0, 0, 0,
                                     0, row_stride, op, plane);
  }
}

template <typename T>
void launch(dim3 grid, size_t lds, hipStream_t s, const sfk_pool_warp_desc* d, int tiles_x, int tiles_y, int budget) {
  hipLaunchKernelGGL((u8_pool_warp_kernel<T>), grid, dim3(256), lds, s, d->pool, d->frame_stride, d->row_stride, d->pixel_pitch,
                     d->frames, d->t, d->h, d->w, d->c0, d->c, d->index, d->warp, d->lut, d->fill, tiles_x, tiles_y, budget,
                     (T*)d->out);
}

}  // namespace

extern "C" int sfk_u8_pool_gather_warp(const sfk_pool_warp_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_pool_warp_desc)) return SFK_ERR_INVALID;
  if (!d->pool || !d->lut || !d->warp || !d->out) return SFK_ERR_INVALID;                  // index may be NULL
  if (d->frames <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0 || d->n <= 0 || d->t <= 0) return SFK_ERR_INVALID;
  if (d->frame_stride < 0 || d->row_stride < 0 || d->c0 < 0) return SFK_ERR_INVALID;
  if ((int64_t)d->pixel_pitch < (int64_t)d->c0 + d->c) return SFK_ERR_INVALID;
  if (d->fill < 0 || d->fill > 255) return SFK_ERR_INVALID;
  if (d->out_dtype != SFK_F32 && d->out_dtype != SFK_BF16) return SFK_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(d->out) & 15) return SFK_ERR_INVALID;
  const int tiles_x = (int)(((int64_t)d->w + TW - 1) / TW), tiles_y = (int)(((int64_t)d->h + TH - 1) / TH);
  int64_t blocks = (int64_t)d->n * d->t;                // each factor is below 2^31 and each product is tested before the next
  if (blocks > SFK_WARP_MAX_BLOCKS) return SFK_ERR_UNSUPPORTED;
  blocks *= tiles_y;
  if (blocks > SFK_WARP_MAX_BLOCKS) return SFK_ERR_UNSUPPORTED;
  blocks *= tiles_x;
  if (blocks > SFK_WARP_MAX_BLOCKS) return SFK_ERR_UNSUPPORTED;
  const int budget = (int)stage_budget(d->h, d->w, d->pixel_pitch, d->c);
  (d->out_dtype == SFK_BF16 ? launch<bf16_t> : launch<float>)(dim3((unsigned)blocks), (size_t)LUT_BYTES + (size_t)budget,
                                                              static_cast<hipStream_t>(stream), d, tiles_x, tiles_y, budget);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_warp_fallback_tiles(int32_t h, int32_t w, int32_t pixel_pitch, int32_t c, const float* mh) {
  if (!mh || h <= 0 || w <= 0 || c <= 0 || pixel_pitch < c) return SFK_ERR_INVALID;
  if ((((int64_t)h + TH - 1) / TH) * (((int64_t)w + TW - 1) / TW) > SFK_WARP_MAX_BLOCKS) return SFK_ERR_UNSUPPORTED;
  const Mat m = {mh[0], mh[1], mh[2], mh[3], mh[4], mh[5]};
  const int64_t budget = stage_budget(h, w, pixel_pitch, c);
  int count = 0;
  for (int ty0 = 0; ty0 < h; ty0 += TH)
    for (int tx0 = 0; tx0 < w; tx0 += TW) {
      const int tx1 = (tx0 + TW < w ? tx0 + TW : w) - 1, ty1 = (ty0 + TH < h ? ty0 + TH : h) - 1;
      count += tile_box(m, tx0, ty0, tx1, ty1, h, w, pixel_pitch, c, budget).mode == MODE_GLOBAL;
    }
  return count;
}

extern "C" int sfk_warp_abi_version(void) { return SFK_WARP_ABI_VERSION; }
