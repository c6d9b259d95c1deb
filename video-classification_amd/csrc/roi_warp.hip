// sfk_roi_resize_warp, sfk_roi_resize_pool_warp, sfk_roi_resize_ragged_warp (include/sfk_roi_warp.h): the part-box crop +
// uint8 table lookup + bilinear resize of roi_resize.hip sampled through a 2 x 3 matrix per clip, one launch per batch.  The
// header states the contract; every product, sum and difference of it is rounded on its own, so contraction is off for this
// file and the operations are written as plain operators (the __fmul_rn / __fadd_rn of the HIP headers are inline functions
// compiled under the headers' own contraction mode and fuse after inlining); the fused operations the contract does name --
// the source index, and every tap after the first of a weighted sum, which is how roi_resize_kernel's passes are compiled --
// are explicit __fmaf_rn.  The three entry points share one kernel and one launcher; the source addressing is a compile-time
// switch, as in roi_resize.hip; where a frame lies, the box clamp and the byte staging are roi_common.h's, shared with it.
//
// One workgroup owns a tile of TILE_H x TILE_W destination pixels of one (clip, frame), all channels:
//   1. it reads the clip's box and matrix, evaluates the contract's (u, v) at the tile's four corners -- each is monotone in
//      x and in y, rounding included, so the corners bound the tile -- and takes the taps of those bounds, clamped into the
//      range test's interval, as the source window of the tile;
//   2. it stages that window's bytes in LDS (roi_stage), unless the frame is missing (a single LDS byte of fill stands for
//      the whole frame, nothing is read), no pixel of the tile can pass the range test (nothing is read), or the window
//      exceeds SFK_ROI_WARP_LDS_BYTES or a corner is not finite (the taps then come from global memory);
//   3. every thread computes the tap span and the weights of its pixel once, keeps the weights in its own LDS column
//      (w[k * 256 + tid]: no bank conflict) and accumulates all channels tap by tap in the sibling's order.
// Every tap index is clamped into the clamped box and, on the staged path, into the staged window, so no table content can
// make a read leave the frame or the LDS.
#include "roi_common.h"
#include "sfk_roi_warp.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kTH = SFK_ROI_WARP_TILE_H, kTW = SFK_ROI_WARP_TILE_W;
constexpr int kStage = SFK_ROI_WARP_LDS_BYTES;
static_assert(kTW == 32 && (kTH * kTW) % kThreads == 0, "a thread's pixels are tid + k * 256 of the tile, 32 to a row");

struct RoiWarpGeo {
  int KH, KW;                 // worst-case taps per axis (of the frame / output ratio, as roi_resize sizes them)
  int col_tiles;
  int off_xw, off_yw, off_sb;
};

// the contract's position of output pixel (x, y) along one axis: three roundings, in this order
__device__ __forceinline__ float warp_pos(float a, float b, float c, int x, int y) {
  return (a * (float)x + b * (float)y) + c;                     // contraction is off: two products, two sums
}

// The taps of real position p (which has passed the range test: -0.5 <= p <= out - 0.5) over a source extent of `in`
// pixels: indices min(first + k, in - 1), k < count, their weights written to w[k * kThreads] (nothing is written with w ==
// nullptr: the span alone).  roi_taps' arithmetic with p in place of the integer index and without its in == out shortcuts.
__device__ __forceinline__ void warp_taps(float p, int in, int out, int aa, int K, float* w, int& first, int& count) {
  const float scale = (float)in / (float)out;
  if (!aa) {
    float src = __fmaf_rn(scale, p + 0.5f, -0.5f);
    if (src < 0.f) src = 0.f;
    const int i0 = min((int)floorf(src), in - 1);
    const float l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
    first = i0;
    count = 2;
    if (w) {
      w[0] = 1.f - l1;
      w[kThreads] = l1;
    }
    return;
  }
  const float support = scale >= 1.f ? scale : 1.f;
  const int max_k = min((int)ceilf(support) * 2 + 1, K);
  const float invscale = scale >= 1.f ? (float)(1.0 / (double)scale) : 1.f;
  const float center = (float)((double)scale * ((double)p + 0.5));
  const int xmin = min(max((int)((double)(center - support) + 0.5), 0), in - 1);
  int xsize = min((int)((double)(center + support) + 0.5), in) - xmin;
  xsize = min(max(xsize, 0), max_k);
  first = xmin;
  count = xsize;
  if (!w) return;
  float total = 0.f;
  for (int k = 0; k < xsize; ++k) {
    const float x = fabsf((float)(((double)((float)(k + xmin) - center) + 0.5) * (double)invscale));
    const float wk = x < 1.f ? (float)(1.0 - (double)x) : 0.f;
    total = total + wk;
    w[k * kThreads] = wk;
  }
  if (total != 0.f)
    for (int k = 0; k < xsize; ++k) w[k * kThreads] = w[k * kThreads] / total;
}

template <typename D, int SRC>
__global__ __launch_bounds__(kThreads) void roi_warp_kernel(sfk_roi_desc d, const float* __restrict__ warp, RoiWarpGeo g, RoiSrc p) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* lut = reinterpret_cast<float*>(smem);
  float* xw = reinterpret_cast<float*>(smem + g.off_xw) + threadIdx.x;
  float* yw = reinterpret_cast<float*>(smem + g.off_yw) + threadIdx.x;
  unsigned char* sb = smem + g.off_sb;

  const int tid = threadIdx.x;
  const int n = blockIdx.z, t = blockIdx.y;
  const int tr = blockIdx.x / g.col_tiles, tc = blockIdx.x - tr * g.col_tiles;
  const int Y0 = tr * kTH, X0 = tc * kTW;
  const int Bv = min(kTH, d.out_h - Y0), TWv = min(kTW, d.out_w - X0);
  const int C = d.c, aa = d.antialias;

  const RoiFrame f = roi_frame<SRC>(d, p, n, t);
  const RoiBox b = roi_box(d, n, f.H, f.W);
  const int bw = b.bw, bh = b.bh;
  const float* m = warp + 6 * (int64_t)n;
  const float ma = m[0], mb = m[1], mc = m[2], md = m[3], me = m[4], mf = m[5];
  const float umax_ok = (float)d.out_w - 0.5f, vmax_ok = (float)d.out_h - 0.5f;

  for (int e = tid; e < 256; e += kThreads) lut[e] = d.lut[e];

  // 1. the tile's bounds from its corners (block-uniform)
  const int XL = X0 + TWv - 1, YL = Y0 + Bv - 1;
  const float u00 = warp_pos(ma, mb, mc, X0, Y0), u01 = warp_pos(ma, mb, mc, XL, Y0);
  const float u10 = warp_pos(ma, mb, mc, X0, YL), u11 = warp_pos(ma, mb, mc, XL, YL);
  const float v00 = warp_pos(md, me, mf, X0, Y0), v01 = warp_pos(md, me, mf, XL, Y0);
  const float v10 = warp_pos(md, me, mf, X0, YL), v11 = warp_pos(md, me, mf, XL, YL);
  const bool finite = isfinite(u00) && isfinite(u01) && isfinite(u10) && isfinite(u11) && isfinite(v00) && isfinite(v01) &&
                      isfinite(v10) && isfinite(v11);
  const float ulo = fmaxf(fminf(fminf(u00, u01), fminf(u10, u11)), -0.5f);
  const float uhi = fminf(fmaxf(fmaxf(u00, u01), fmaxf(u10, u11)), umax_ok);
  const float vlo = fmaxf(fminf(fminf(v00, v01), fminf(v10, v11)), -0.5f);
  const float vhi = fminf(fmaxf(fmaxf(v00, v01), fmaxf(v10, v11)), vmax_ok);
  const bool outside = finite && (ulo > uhi || vlo > vhi);      // no pixel of the tile can pass the range test

  // 2. where the taps come from: base[row * rs + col * cs + ch * chs], row and col relative to (oy, ox) and clamped to
  //    [0, rmax] x [0, cmax]; base is LDS (staged window, or the one fill byte of a missing frame) or the frame itself
  const unsigned char* base = sb;
  int64_t rs = 0, cs = 0, chs = 0;
  int oy = 0, ox = 0, rmax = 0, cmax = 0;
  if (SRC != kStacked && f.miss) {
    if (tid == 0) sb[0] = (unsigned char)p.fill;
  } else if (!outside) {
    bool staged = false;
    if (finite) {
      int xlo, ylo, f2, c2;
      warp_taps(ulo, bw, d.out_w, aa, g.KW, nullptr, xlo, c2);
      warp_taps(uhi, bw, d.out_w, aa, g.KW, nullptr, f2, c2);
      const int xhi = min(f2 + max(c2, 1) - 1, bw - 1);
      warp_taps(vlo, bh, d.out_h, aa, g.KH, nullptr, ylo, c2);
      warp_taps(vhi, bh, d.out_h, aa, g.KH, nullptr, f2, c2);
      const int yhi = min(f2 + max(c2, 1) - 1, bh - 1);
      const int ncol = max(xhi - xlo + 1, 1), nrow = max(yhi - ylo + 1, 1);
      if ((int64_t)nrow * ncol * C <= kStage) {
        const uint8_t* wbase = f.first + (int64_t)(b.y1 + ylo) * f.rstride + (int64_t)(b.x1 + xlo) * d.sw;
        roi_stage<SRC>(sb, ncol, C, wbase, f.rstride, d, false, 0, nrow, ncol, tid, kThreads);
        staged = true;
        rs = (int64_t)ncol * C, cs = C, chs = 1;
        oy = ylo, ox = xlo, rmax = nrow - 1, cmax = ncol - 1;
      }
    }
    if (!staged) {
      base = f.first + (int64_t)b.y1 * f.rstride + (int64_t)b.x1 * d.sw;
      rs = f.rstride, cs = d.sw, chs = d.sc;
      rmax = bh - 1, cmax = bw - 1;
    }
  }
  __syncthreads();

  // 3. the pixels: tid + k * 256 of the tile, 32 to a row, so a wavefront stores two runs of 32 along destination rows
  for (int q = tid; q < kTH * kTW; q += kThreads) {
    const int yy = q >> 5, xx = q & 31;
    if (yy >= Bv || xx >= TWv) continue;
    float acc[SFK_ROI_MAX_C];
#pragma unroll
    for (int ch = 0; ch < SFK_ROI_MAX_C; ++ch) acc[ch] = 0.f;
    const float u = warp_pos(ma, mb, mc, X0 + xx, Y0 + yy), v = warp_pos(md, me, mf, X0 + xx, Y0 + yy);
    if (!outside && u >= -0.5f && u <= umax_ok && v >= -0.5f && v <= vmax_ok) {
      int xf, xn, yf, yn;
      warp_taps(u, bw, d.out_w, aa, g.KW, xw, xf, xn);
      warp_taps(v, bh, d.out_h, aa, g.KH, yw, yf, yn);
      for (int r = 0; r < yn; ++r) {
        const int row = min(max(min(yf + r, bh - 1) - oy, 0), rmax);
        const unsigned char* rp = base + (int64_t)row * rs;
        const float wy = yw[r * kThreads];
        float h[SFK_ROI_MAX_C];
#pragma unroll
        for (int ch = 0; ch < SFK_ROI_MAX_C; ++ch) h[ch] = 0.f;
        for (int k = 0; k < xn; ++k) {
          const int col = min(max(min(xf + k, bw - 1) - ox, 0), cmax);
          const unsigned char* pp = rp + (int64_t)col * cs;
          const float wx = xw[k * kThreads];
#pragma unroll
          for (int ch = 0; ch < SFK_ROI_MAX_C; ++ch) {
            if (ch < C) {
              const float lv = lut[pp[ch * chs]];
              h[ch] = k == 0 ? lv * wx : __fmaf_rn(lv, wx, h[ch]);
            }
          }
        }
#pragma unroll
        for (int ch = 0; ch < SFK_ROI_MAX_C; ++ch) {
          if (ch < C) {
            acc[ch] = r == 0 ? h[ch] * wy : __fmaf_rn(h[ch], wy, acc[ch]);
          }
        }
      }
    }
    D* o = static_cast<D*>(d.dst) + n * d.dn + t * d.dt + (int64_t)d.c_off * d.dc + (int64_t)(Y0 + yy) * d.dh + X0 + xx;
#pragma unroll
    for (int ch = 0; ch < SFK_ROI_MAX_C; ++ch)
      if (ch < C) o[(int64_t)ch * d.dc] = (D)acc[ch];
  }
}

// the host-side checks the three entry points share (roi_check, and warp; each checks its own struct_size and its own source
// first), then the launch: roi_resize's, with warp in place of crop and pad
int roi_warp(const sfk_roi_desc* d, const float* warp, int src, const RoiSrc* p, sfk_stream_t stream) {
  if (!warp) return SFK_ERR_INVALID;
  if (const int st = roi_check(d)) return st;
  RoiWarpGeo g{};
  g.KH = roi_max_taps(d->h, d->out_h, d->antialias);
  g.KW = roi_max_taps(d->w, d->out_w, d->antialias);
  const int row_tiles = (d->out_h + kTH - 1) / kTH;
  g.col_tiles = (d->out_w + kTW - 1) / kTW;
  g.off_xw = 256 * 4;
  g.off_yw = g.off_xw + g.KW * kThreads * 4;
  g.off_sb = g.off_yw + g.KH * kThreads * 4;
  const int lds = g.off_sb + kStage;                      // at most 1 + 34 + 24 KiB
  const int64_t tiles = (int64_t)row_tiles * g.col_tiles;
  if (!roi_grid_fits(tiles, d)) return SFK_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)tiles, (unsigned)d->t, (unsigned)d->n);
  hipLaunchKernelGGL(SFK_ROI_KERNEL(roi_warp_kernel, d->dst_dtype, src), grid, dim3(kThreads), lds,
                     static_cast<hipStream_t>(stream), *d, warp, g, p ? *p : RoiSrc{});
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

}  // namespace

extern "C" int sfk_roi_resize_warp(const sfk_roi_warp_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_roi_warp_desc)) return SFK_ERR_INVALID;
  const sfk_roi_desc r = roi_from_strided(*d);
  return roi_warp(&r, d->warp, kStacked, nullptr, stream);
}

extern "C" int sfk_roi_resize_pool_warp(const sfk_roi_pool_warp_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_roi_pool_warp_desc)) return SFK_ERR_INVALID;
  sfk_roi_desc r;
  RoiSrc p;
  if (const int st = roi_from_pool(*d, &r, &p)) return st;
  return roi_warp(&r, d->warp, kPool, &p, stream);
}

extern "C" int sfk_roi_resize_ragged_warp(const sfk_roi_ragged_warp_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_roi_ragged_warp_desc)) return SFK_ERR_INVALID;
  sfk_roi_desc r;
  RoiSrc p;
  if (const int st = roi_from_ragged(*d, &r, &p)) return st;
  return roi_warp(&r, d->warp, kRagged, &p, stream);
}

extern "C" int sfk_roi_warp_abi_version(void) { return SFK_ROI_WARP_ABI_VERSION; }
