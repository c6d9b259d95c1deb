// sfk_u8_pad_resize_cubic (include/sfk_resize.h): the v1 loader's zero-pad-to-square + 4x4-tap cubic resize of ragged uint8
// HWC crops, in integers from 11-bit fixed-point coefficients.  The header is the specification; tests/ref_resize.py
// restates it in numpy and every GPU comparison is bit-exact.
#include "sfk_common.h"
#include "sfk_resize.h"

namespace {

// The taps of output coordinate d on a square of side m resized to size: s (the taps are clip(s - 1 + j, 0, m - 1)) and the
// four coefficients in 1/2048.  Double for the coordinate, float for the cubic, every operation rounded on its own: the
// pragma keeps the compiler from contracting a multiply and an add into an FMA (HIP's __fmul_rn / __fadd_rn are plain
// operators and would be contracted under the default -ffp-contract=fast-honor-pragmas).
__device__ __forceinline__ void cubic_taps(int d, int m, int size, int& s, int q[4]) {
#pragma clang fp contract(off)
  const double scale = (double)m / (double)size;
  const double fd = ((double)d + 0.5) * scale;
  const float f = (float)(fd - 0.5);
  const float fl = floorf(f);
  const float t = f - fl;
  s = (int)fl;
  const float A = -0.75f;
  const float u = t + 1.f, v = 1.f - t;
  float k[4];
  k[0] = ((A * u - 5.f * A) * u + 8.f * A) * u - 4.f * A;
  k[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  k[2] = ((A + 2.f) * v - (A + 3.f)) * v * v + 1.f;
  k[3] = 1.f - k[0] - k[1] - k[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = (int)rintf(k[j] * 2048.f);
}

__device__ __forceinline__ int clipi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Dynamic LDS, in this order (SFK_RESIZE_LDS_BYTES), cp = c rounded up to a multiple of 4:
//   acc  int32[max_side*cp]  the vertically filtered row: pixel X of the padded square at acc[X*cp .. X*cp + c), so that four
//                            channels of a pixel are one aligned 16-byte LDS access (the cp - c tail columns hold rubbish)
//   raw  4 x uint8[raw_b]    the four source rows; row i's byte k at raw_i[shift_i + k], shift_i = its address & 15, so that
//                            LDS and global addresses share their 16-byte phase (as u8_pool_gather.hip stages its row)
//   obuf uint8[ROW16(S*c)]   the output row, byte e at obuf[oshift + e], oshift = the output row's address & 15
//   xt   int4[S][2]          per output coordinate: the four taps' offsets X_j*cp into acc, and the four coefficients
//   xs   int32[S]            per output coordinate: s, unclipped (the row pass reads entry y of the same table)
// One output row per block; everything that decides a branch around a barrier is block-uniform.  A thread works on four
// channels of one pixel at a time (gdiv divides by cp / 4, the groups of a pixel).
__global__ __launch_bounds__(256) void u8_pad_resize_cubic_kernel(const uint8_t* __restrict__ src, int64_t src_bytes,
                                                                  const int64_t* __restrict__ offset,
                                                                  const int32_t* __restrict__ hw, int c, FastDiv gdiv, int size,
                                                                  int max_side, int fill, uint8_t* __restrict__ out,
                                                                  int64_t out_frame_stride, int raw_b) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int cp = (c + 3) & ~3, gpp = cp >> 2;
  const int sc = size * c;
  int32_t* acc = reinterpret_cast<int32_t*>(lds);
  uint8_t* raw = lds + (size_t)max_side * cp * 4;
  uint8_t* obuf = raw + (size_t)4 * raw_b;
  int4* xt = reinterpret_cast<int4*>(obuf + (sc + 15 + 15) / 16 * 16);
  int32_t* xs = reinterpret_cast<int32_t*>(xt + 2 * size);

  const int tid = threadIdx.x;
  const int y = blockIdx.x % size;
  const int f = blockIdx.x / size;
  const int h = hw[2 * f], w = hw[2 * f + 1];
  const int64_t off = offset[f];
  uint8_t* op = out + (int64_t)f * out_frame_stride + (int64_t)y * sc;
  const int oshift = (int)(reinterpret_cast<uintptr_t>(op) & 15);
  bool miss = h <= 0 || w <= 0 || h > max_side || w > max_side || off < 0;
  if (!miss) miss = off > src_bytes || (int64_t)h * w * c > src_bytes - off;

  if (miss) {
    for (int e = tid; e < sc; e += 256) obuf[oshift + e] = (uint8_t)fill;
  } else {
    const int m = h > w ? h : w;
    const int nx = (m - w) / 2, ny = (m - h) / 2;
    const int wc = w * c;
    for (int d = tid; d < size; d += 256) {
      int s, q[4];
      cubic_taps(d, m, size, s, q);
      xt[2 * d] = make_int4(clipi(s - 1, 0, m - 1) * cp, clipi(s, 0, m - 1) * cp, clipi(s + 1, 0, m - 1) * cp,
                            clipi(s + 2, 0, m - 1) * cp);
      xt[2 * d + 1] = make_int4(q[0], q[1], q[2], q[3]);
      xs[d] = s;
    }
    __syncthreads();
    // this row's taps are entry y of the table (one table for both axes); block-uniform, so kept in scalar registers
    const int sy = __builtin_amdgcn_readfirstlane(xs[y]);
    const int4 qrow = xt[2 * y + 1];
    int qy[4] = {qrow.x, qrow.y, qrow.z, qrow.w};
    // stage the source rows that exist.  Row i's bytes are split into the fa_i bytes before its first 16-byte-aligned address,
    // nu_i whole aligned units and a tail of fewer than 16 bytes; a thread loads its unit of ALL rows before it stores any, and
    // the at most 15 + 15 edge bytes of a row go one byte per thread (the last 32 threads), so that a row costs one memory
    // latency, not one per byte.  A tap row in the zero padding is not read.
    int shift[4], base[4], fa[4], nu[4];
    bool ok[4];
    const uint8_t* sp[4];
    int live = -1, live_shift = 0, live_base = 0;           // a row that is staged, if any
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int sr = clipi(sy - 1 + i, 0, m - 1) - ny;
      ok[i] = sr >= 0 && sr < h;
      sp[i] = src + off + (int64_t)(ok[i] ? sr : 0) * wc;
      shift[i] = (int)(reinterpret_cast<uintptr_t>(sp[i]) & 15);
      base[i] = i * raw_b;
      fa[i] = (16 - shift[i]) & 15;
      if (fa[i] > wc) fa[i] = wc;
      nu[i] = (wc - fa[i]) >> 4;
      if (ok[i]) live = i, live_shift = shift[i], live_base = base[i];
    }
    for (int u = tid; u < (wc >> 4); u += 256) {            // (wc >> 4 >= every nu_i)
      const bool p0 = ok[0] && u < nu[0], p1 = ok[1] && u < nu[1], p2 = ok[2] && u < nu[2], p3 = ok[3] && u < nu[3];
      uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0, v2 = v0, v3 = v0;
      if (p0) v0 = *reinterpret_cast<const uint4*>(sp[0] + fa[0] + 16 * u);
      if (p1) v1 = *reinterpret_cast<const uint4*>(sp[1] + fa[1] + 16 * u);
      if (p2) v2 = *reinterpret_cast<const uint4*>(sp[2] + fa[2] + 16 * u);
      if (p3) v3 = *reinterpret_cast<const uint4*>(sp[3] + fa[3] + 16 * u);
      if (p0) *reinterpret_cast<uint4*>(raw + base[0] + shift[0] + fa[0] + 16 * u) = v0;
      if (p1) *reinterpret_cast<uint4*>(raw + base[1] + shift[1] + fa[1] + 16 * u) = v1;
      if (p2) *reinterpret_cast<uint4*>(raw + base[2] + shift[2] + fa[2] + 16 * u) = v2;
      if (p3) *reinterpret_cast<uint4*>(raw + base[3] + shift[3] + fa[3] + 16 * u) = v3;
    }
    if (tid >= 224) {
      const int e = tid - 224;                              // 0..15: a byte of the head, 16..31: a byte of the tail
      uint8_t v[4];
      int k[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        k[i] = e < 16 ? (e < fa[i] ? e : -1) : (fa[i] + 16 * nu[i] + e - 16 < wc ? fa[i] + 16 * nu[i] + e - 16 : -1);
        if (!ok[i]) k[i] = -1;
        if (k[i] >= 0) v[i] = sp[i][k[i]];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k[i] >= 0) raw[base[i] + shift[i] + k[i]] = v[i];
    }
    // a row that was not staged contributes nothing: its coefficient becomes 0 and it reads the bytes of one that was, so
    // that the pass below has no branch per row
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      qy[i] = ok[i] ? __builtin_amdgcn_readfirstlane(qy[i]) : 0;
      if (!ok[i]) shift[i] = live_shift, base[i] = live_base;
    }
    __syncthreads();
    // vertical pass: four channels of one pixel per thread and step.  The four bytes may run up to three bytes past the
    // pixel (into the next pixel, or into the row buffer's spare unit after the last one): those land in the tail columns
    for (int t = tid; t < m * gpp; t += 256) {
      const int X = (int)gdiv.div((uint32_t)t), ch0 = (t - X * gpp) * 4;
      int a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      if (live >= 0 && X >= nx && X < nx + w) {
        const int k0 = (X - nx) * c + ch0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int at = shift[i] + k0;
          const uint32_t* rw = reinterpret_cast<const uint32_t*>(raw + base[i]) + (at >> 2);
          const uint64_t two = ((uint64_t)rw[1] << 32) | rw[0];             // the spare unit keeps rw[1] inside the row
          const uint32_t b4 = (uint32_t)(two >> (8 * (at & 3)));
          a0 += __mul24(qy[i], (int)(b4 & 255));                            // 13-bit coefficient x byte: 24-bit multiplies
          a1 += __mul24(qy[i], (int)((b4 >> 8) & 255));
          a2 += __mul24(qy[i], (int)((b4 >> 16) & 255));
          a3 += __mul24(qy[i], (int)(b4 >> 24));
        }
      }
      *reinterpret_cast<int4*>(acc + X * cp + ch0) = make_int4(a0, a1, a2, a3);
    }
    __syncthreads();
    // horizontal pass: four channels of one output pixel per thread and step; consecutive threads read consecutive 16-byte
    // units of acc.  |acc| <= 255 * 2818 < 2^23 and |q| < 2^12: 24-bit multiplies, the low 32 bits of each product are exact
    for (int t = tid; t < size * gpp; t += 256) {
      const int x = (int)gdiv.div((uint32_t)t), ch0 = (t - x * gpp) * 4;
      const int4 o = xt[2 * x], q = xt[2 * x + 1];
      const int4 p0 = *reinterpret_cast<const int4*>(acc + o.x + ch0), p1 = *reinterpret_cast<const int4*>(acc + o.y + ch0);
      const int4 p2 = *reinterpret_cast<const int4*>(acc + o.z + ch0), p3 = *reinterpret_cast<const int4*>(acc + o.w + ch0);
      int v[4];
      v[0] = __mul24(q.x, p0.x) + __mul24(q.y, p1.x) + __mul24(q.z, p2.x) + __mul24(q.w, p3.x);
      v[1] = __mul24(q.x, p0.y) + __mul24(q.y, p1.y) + __mul24(q.z, p2.y) + __mul24(q.w, p3.y);
      v[2] = __mul24(q.x, p0.z) + __mul24(q.y, p1.z) + __mul24(q.z, p2.z) + __mul24(q.w, p3.z);
      v[3] = __mul24(q.x, p0.w) + __mul24(q.y, p1.w) + __mul24(q.z, p2.w) + __mul24(q.w, p3.w);
      uint8_t* ob = obuf + oshift + x * c + ch0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ch0 + e < c) ob[e] = (uint8_t)clipi((v[e] + (1 << 21)) >> 22, 0, 255);
    }
  }
  __syncthreads();
  {                                                         // the row's bytes are obuf[oshift .. oshift + sc)
    int ofa = (16 - oshift) & 15;
    if (ofa > sc) ofa = sc;
    const int onu = (sc - ofa) >> 4;
    for (int u = tid; u < onu; u += 256)
      *reinterpret_cast<uint4*>(op + ofa + 16 * u) = *reinterpret_cast<const uint4*>(obuf + oshift + ofa + 16 * u);
    if (tid >= 224) {                                       // the edges, one byte per thread
      const int e = tid - 224;
      const int k = e < 16 ? (e < ofa ? e : -1) : (ofa + 16 * onu + e - 16 < sc ? ofa + 16 * onu + e - 16 : -1);
      if (k >= 0) op[k] = obuf[oshift + k];
    }
  }
}

}  // namespace

extern "C" int sfk_u8_pad_resize_cubic(const sfk_resize_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_resize_desc)) return SFK_ERR_INVALID;
  if (!d->src || !d->offset || !d->hw || !d->out) return SFK_ERR_INVALID;
  if (d->frames <= 0 || d->c <= 0 || d->size <= 0 || d->max_side <= 0 || d->src_bytes < 0) return SFK_ERR_INVALID;
  if (d->out_frame_stride < (int64_t)d->size * d->size * d->c) return SFK_ERR_INVALID;
  if (d->fill < 0 || d->fill > 255) return SFK_ERR_INVALID;
  const int64_t blocks = (int64_t)d->frames * d->size;
  const int64_t lds = SFK_RESIZE_LDS_BYTES(d->max_side, d->c, d->size);
  if (blocks > SFK_RESIZE_MAX_BLOCKS || lds > SFK_RESIZE_MAX_LDS_BYTES) return SFK_ERR_UNSUPPORTED;
  const int raw_b = (int)(SFK_RESIZE_ROW16((int64_t)d->max_side * d->c) + 16);
  static bool attr_set = false;             // > 64 KB of dynamic LDS needs the opt-in (idempotent, set once per process)
  if (lds > 64 * 1024 && !attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&u8_pad_resize_cubic_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, SFK_RESIZE_MAX_LDS_BYTES) != hipSuccess)
      return SFK_ERR_LAUNCH;
    attr_set = true;
  }
  FastDiv gdiv;
  gdiv.set((d->c + 3) / 4);
  hipLaunchKernelGGL(u8_pad_resize_cubic_kernel, dim3((unsigned)blocks), dim3(256), (size_t)lds,
                     static_cast<hipStream_t>(stream), d->src, d->src_bytes, d->offset, d->hw, d->c, gdiv, d->size, d->max_side,
                     d->fill, d->out, d->out_frame_stride, raw_b);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_resize_abi_version(void) { return SFK_RESIZE_ABI_VERSION; }
