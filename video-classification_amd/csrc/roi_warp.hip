// sfk_roi_resize_warp, sfk_roi_resize_pool_warp, sfk_roi_resize_ragged_warp (include/sfk_roi_warp.h): the part-box crop +
// uint8 table lookup + bilinear resize of roi_resize.hip sampled through a 2 x 3 matrix per clip, one launch per batch.  The
// header states the contract; every product, sum and difference of it is rounded on its own, so contraction is off for this
// file and the operations are written as plain operators (the __fmul_rn / __fadd_rn of the HIP headers are inline functions
// compiled under the headers' own contraction mode and fuse after inlining); the fused operations the contract does name --
// the source index, and every tap after the first of a weighted sum, which is how roi_resize_kernel's passes are compiled --
// are explicit __fmaf_rn.  The three entry points share one kernel and one launcher; the source addressing is a compile-time
// switch, as in roi_resize.hip, whose RoiSrc, box clamp and byte staging (roi_common.h) are used here.
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

  // the frame extent, row stride and first byte, and whether the frame is missing: roi_resize_kernel's, word for word
  int H = d.h, W = d.w;
  int64_t rstride = d.sh;
  const uint8_t* frame = d.src;
  bool miss = false;
  if (SRC == kRagged) {
    const int hn = p.hw[2 * (int64_t)n], wn = p.hw[2 * (int64_t)n + 1];
    const int64_t o = p.offset[(int64_t)n * d.t + t];
    H = min(max(hn, 1), d.h);
    W = min(max(wn, 1), d.w);
    miss = o < 0 || hn != H || wn != W || o > p.arena_bytes || (int64_t)hn * wn > (p.arena_bytes - o) / d.sw;
    rstride = (int64_t)W * d.sw;
    frame += miss ? 0 : o;
  } else if (SRC == kPool) {
    const int f = p.index[(int64_t)n * d.t + t];
    miss = f < 0 || f >= p.frames;
    frame += (int64_t)(miss ? 0 : f) * d.st;
  } else {
    frame += n * d.sn + t * d.st;
  }

  // the box, clamped the way a Python slice clamps it
  const int32_t* bx = d.box + 4 * (int64_t)n;
  const int x1 = min(max(bx[0], 0), W - 1), y1 = min(max(bx[1], 0), H - 1);
  const int x2 = min(max(bx[2], x1 + 1), W), y2 = min(max(bx[3], y1 + 1), H);
  const int bw = x2 - x1, bh = y2 - y1;
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
  if (SRC != kStacked && miss) {
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
        const uint8_t* wbase = frame + (int64_t)(y1 + ylo) * rstride + (int64_t)(x1 + xlo) * d.sw;
        roi_stage<SRC>(sb, ncol, C, wbase, rstride, d, false, 0, nrow, ncol, tid, kThreads);
        staged = true;
        rs = (int64_t)ncol * C, cs = C, chs = 1;
        oy = ylo, ox = xlo, rmax = nrow - 1, cmax = ncol - 1;
      }
    }
    if (!staged) {
      base = frame + (int64_t)y1 * rstride + (int64_t)x1 * d.sw;
      rs = rstride, cs = d.sw, chs = d.sc;
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

// every host-side check the three entry points share (each checks its own struct_size and its own source first), then the
// launch: roi_resize's, with warp in place of crop and pad
int roi_warp(const sfk_roi_desc* d, const float* warp, int src, const RoiSrc* p, sfk_stream_t stream) {
  if (!d->src || !d->lut || !d->box || !d->dst || !warp) return SFK_ERR_INVALID;
  if (d->n <= 0 || d->t <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0 || d->out_h <= 0 || d->out_w <= 0) return SFK_ERR_INVALID;
  if (d->sn < 0 || d->st < 0 || d->sh < 0 || d->sw < 0 || d->sc < 0 || d->dn < 0 || d->dt < 0 || d->dc < 0 || d->dh < 0)
    return SFK_ERR_INVALID;
  if ((d->antialias != 0 && d->antialias != 1) || d->c_off < 0) return SFK_ERR_INVALID;
  if (d->dst_dtype != SFK_F32 && d->dst_dtype != SFK_BF16) return SFK_ERR_INVALID;
  if (d->c > SFK_ROI_MAX_C || (d->sc == 1 && d->sw > 4096)) return SFK_ERR_UNSUPPORTED;
  const double sh = (double)d->h / d->out_h, sw = (double)d->w / d->out_w;
  if (sh > SFK_ROI_MAX_RATIO || sw > SFK_ROI_MAX_RATIO) return SFK_ERR_UNSUPPORTED;
  // worst-case taps: the box never exceeds its frame, so its ratio never exceeds sh / sw
  RoiWarpGeo g{};
  g.KH = d->antialias ? (int)ceil(sh > 1.0 ? sh : 1.0) * 2 + 1 : 2;
  g.KW = d->antialias ? (int)ceil(sw > 1.0 ? sw : 1.0) * 2 + 1 : 2;
  const int row_tiles = (d->out_h + kTH - 1) / kTH;
  g.col_tiles = (d->out_w + kTW - 1) / kTW;
  g.off_xw = 256 * 4;
  g.off_yw = g.off_xw + g.KW * kThreads * 4;
  g.off_sb = g.off_yw + g.KH * kThreads * 4;
  const int lds = g.off_sb + kStage;                      // at most 1 + 34 + 24 KiB
  const int64_t tiles = (int64_t)row_tiles * g.col_tiles;
  if (tiles > 0x7fffffff || d->t > 65535 || d->n > 65535) return SFK_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)tiles, (unsigned)d->t, (unsigned)d->n);
  const bool bf = d->dst_dtype == SFK_BF16;
  const auto kernel = src == kRagged ? (bf ? roi_warp_kernel<bf16_t, kRagged> : roi_warp_kernel<float, kRagged>)
                      : src == kPool ? (bf ? roi_warp_kernel<bf16_t, kPool> : roi_warp_kernel<float, kPool>)
                                     : (bf ? roi_warp_kernel<bf16_t, kStacked> : roi_warp_kernel<float, kStacked>);
  hipLaunchKernelGGL(kernel, grid, dim3(kThreads), lds, s, *d, warp, g, p ? *p : RoiSrc{});
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

}  // namespace

extern "C" int sfk_roi_resize_warp(const sfk_roi_warp_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_roi_warp_desc)) return SFK_ERR_INVALID;
  sfk_roi_desc r{};
  r.struct_size = sizeof(sfk_roi_desc);
  r.antialias = d->antialias;
  r.src = d->src;
  r.sn = d->sn, r.st = d->st, r.sh = d->sh, r.sw = d->sw, r.sc = d->sc;
  r.n = d->n, r.t = d->t, r.h = d->h, r.w = d->w, r.c = d->c;
  r.out_h = d->out_h, r.out_w = d->out_w;
  r.lut = d->lut, r.box = d->box;
  r.dst_dtype = d->dst_dtype, r.dst = d->dst;
  r.dn = d->dn, r.dt = d->dt, r.dc = d->dc, r.dh = d->dh, r.c_off = d->c_off;
  return roi_warp(&r, d->warp, kStacked, nullptr, stream);
}

extern "C" int sfk_roi_resize_pool_warp(const sfk_roi_pool_warp_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_roi_pool_warp_desc)) return SFK_ERR_INVALID;
  if (!d->pool || !d->index || d->frames <= 0) return SFK_ERR_INVALID;
  if (d->frame_stride < 0 || d->row_stride < 0 || d->c0 < 0) return SFK_ERR_INVALID;
  if ((int64_t)d->pixel_pitch < (int64_t)d->c0 + d->c) return SFK_ERR_INVALID;
  if (d->fill < 0 || d->fill > 255) return SFK_ERR_INVALID;
  sfk_roi_desc r{};
  r.struct_size = sizeof(sfk_roi_desc);
  r.antialias = d->antialias;
  r.src = d->pool + d->c0;
  r.sn = 0, r.st = d->frame_stride, r.sh = d->row_stride, r.sw = d->pixel_pitch, r.sc = 1;
  r.n = d->n, r.t = d->t, r.h = d->h, r.w = d->w, r.c = d->c;
  r.out_h = d->out_h, r.out_w = d->out_w;
  r.lut = d->lut, r.box = d->box;
  r.dst_dtype = d->dst_dtype, r.dst = d->dst;
  r.dn = d->dn, r.dt = d->dt, r.dc = d->dc, r.dh = d->dh, r.c_off = d->c_off;
  const RoiSrc p{d->index, d->frames, d->fill, nullptr, nullptr, 0};
  return roi_warp(&r, d->warp, kPool, &p, stream);
}

extern "C" int sfk_roi_resize_ragged_warp(const sfk_roi_ragged_warp_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_roi_ragged_warp_desc)) return SFK_ERR_INVALID;
  if (!d->arena || !d->offset || !d->hw || d->max_h <= 0 || d->max_w <= 0) return SFK_ERR_INVALID;
  if (d->arena_bytes <= 0 || (d->arena_bytes & 3) || ((uintptr_t)d->arena & 3) || d->c0 < 0) return SFK_ERR_INVALID;
  if ((int64_t)d->pixel_pitch < (int64_t)d->c0 + d->c) return SFK_ERR_INVALID;
  if (d->fill < 0 || d->fill > 255) return SFK_ERR_INVALID;
  sfk_roi_desc r{};
  r.struct_size = sizeof(sfk_roi_desc);
  r.antialias = d->antialias;
  r.src = d->arena + d->c0;
  r.sn = 0, r.st = 0, r.sh = 0, r.sw = d->pixel_pitch, r.sc = 1;
  r.n = d->n, r.t = d->t, r.h = d->max_h, r.w = d->max_w, r.c = d->c;
  r.out_h = d->out_h, r.out_w = d->out_w;
  r.lut = d->lut, r.box = d->box;
  r.dst_dtype = d->dst_dtype, r.dst = d->dst;
  r.dn = d->dn, r.dt = d->dt, r.dc = d->dc, r.dh = d->dh, r.c_off = d->c_off;
  const RoiSrc p{nullptr, 0, d->fill, d->offset, d->hw, d->arena_bytes};
  return roi_warp(&r, d->warp, kRagged, &p, stream);
}

extern "C" int sfk_roi_warp_abi_version(void) { return SFK_ROI_WARP_ABI_VERSION; }
