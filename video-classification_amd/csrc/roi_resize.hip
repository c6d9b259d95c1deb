// sfk_roi_resize (include/sfk_v2.h): part-box crop + uint8 table lookup + separable bilinear resize (F.interpolate,
// align_corners=False, with or without antialiasing) + optional RandomCrop shift, one launch per batch -- and
// sfk_roi_resize_pool (include/sfk_roi_pool.h): the same from frames that lie in a pool, picked by a table of frame indices --
// and sfk_roi_resize_ragged (include/sfk_roi_ragged.h): the same from frames stored cropped to their clip's own rectangle in a
// byte arena, picked by a table of byte offsets.  The three entry points share one kernel and one launcher; the source
// addressing is a compile-time switch.
//
// One workgroup owns a tile of B destination rows x TW destination columns of one (clip, frame), all channels:
//   1. it reads the clip's box (and crop), builds the tap index / weight tables of its TW columns and B rows in LDS with
//      torch's CPU arithmetic (upsample_bilinear2d's fused source index; _upsample_bilinear2d_aa's mixed float/double
//      weights), and the byte table;
//   2. it stages the source bytes its taps touch -- R rows x SP columns x c channels -- in LDS, as aligned dwords when the
//      channels of a pixel are adjacent (HWC; a pool's and an arena's frames always are), as bytes otherwise (planar); a
//      pooled frame whose index is outside the pool, or an arena frame that does not lie in the arena, is staged as bytes of
//      `fill` and reads nothing;
//   3. horizontal pass: R x c x TW fp32 band in LDS (taps in torch's order, no contraction);
//   4. vertical pass: one coalesced row store per (channel, row), zeros where the crop shift leaves the resized image.
// The host sizes B, TW, R and SP from the worst-case ratio frame / output (of a ragged batch: its largest rectangle), so
// every box fits its LDS; the kernel still clamps every LDS index to what it staged, so a box the host did not foresee can
// neither write out of bounds nor read unstaged memory.
#include "roi_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTaps = 2 * SFK_ROI_MAX_RATIO + 1;
constexpr int kLdsBudget = 64 * 1024;
// a ragged batch is sized from its own largest rectangle, which may admit a taller tile than the whole frame would; a tile
// is taken only if three workgroups of it still share a CU's 160 KiB (10 x 20 clips of 240 x 320 to 192^2 with rectangles up
// to 209 x 292: B 16 at 61 872 bytes, two workgroups a CU, ran 0.715 ms; B 8 at 38 992 bytes, four a CU, runs 0.454 ms)
constexpr int kRaggedLdsBudget = 160 * 1024 / 3;

struct RoiGeo {
  int B, TW, R, SP, KH, KW;
  int row_tiles, col_tiles;
  int off_lut, off_xw, off_xi, off_yw, off_yi, off_sb, off_tmp, lds;
};

inline int align16(int v) { return (v + 15) & ~15; }

RoiGeo roi_layout(int B, int TW, int c, int KH, int KW, double sh, double sw, int out_h, int out_w) {
  RoiGeo g;
  g.B = B;
  g.TW = TW;
  g.KH = KH;
  g.KW = KW;
  g.R = (int)floor((B - 1) * sh) + KH + 2;
  g.SP = (int)floor((TW - 1) * sw) + KW + 2;
  g.row_tiles = (out_h + B - 1) / B;
  g.col_tiles = (out_w + TW - 1) / TW;
  int o = 0;
  g.off_lut = o; o += 256 * 4;
  g.off_xw = o;  o += align16(TW * KW * 4);
  g.off_xi = o;  o += align16(TW * KW * 4);
  g.off_yw = o;  o += align16(B * KH * 4);
  g.off_yi = o;  o += align16(B * KH * 4);
  g.off_tmp = o; o += align16(g.R * c * TW * 4);
  g.off_sb = o;  o += align16(g.R * g.SP * c);
  g.lds = o;
  return g;
}

template <typename D, int SRC>
__global__ __launch_bounds__(kThreads) void roi_resize_kernel(sfk_roi_desc d, RoiGeo g, RoiSrc p) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* lut = reinterpret_cast<float*>(smem + g.off_lut);
  float* xw = reinterpret_cast<float*>(smem + g.off_xw);
  int* xi = reinterpret_cast<int*>(smem + g.off_xi);
  float* yw = reinterpret_cast<float*>(smem + g.off_yw);
  int* yi = reinterpret_cast<int*>(smem + g.off_yi);
  float* tmp = reinterpret_cast<float*>(smem + g.off_tmp);
  unsigned char* sb = smem + g.off_sb;

  const int tid = threadIdx.x;
  const int n = blockIdx.z, t = blockIdx.y;
  const int tr = blockIdx.x / g.col_tiles, tc = blockIdx.x - tr * g.col_tiles;
  const int Y0 = tr * g.B, X0 = tc * g.TW;
  const int Bv = min(g.B, d.out_h - Y0), TWv = min(g.TW, d.out_w - X0);
  const int C = d.c, KH = g.KH, KW = g.KW;

  const RoiFrame f = roi_frame<SRC>(d, p, n, t);
  const RoiBox b = roi_box(d, n, f.H, f.W);
  const int bw = b.bw, bh = b.bh;
  int dy = 0, dx = 0;
  if (d.crop) {
    dy = d.crop[2 * (int64_t)n] - d.pad;
    dx = d.crop[2 * (int64_t)n + 1] - d.pad;
  }

  // 1. tables (source indices relative to the box) and the byte table
  for (int e = tid; e < 256; e += kThreads) lut[e] = d.lut[e];
  if (tid < g.TW) {
    const int r = min(max(X0 + min(tid, TWv - 1) + dx, 0), d.out_w - 1);
    int id[kMaxTaps];
    float w[kMaxTaps];
    roi_taps(r, bw, d.out_w, d.antialias, KW, id, w);
    for (int k = 0; k < KW; ++k) { xi[tid * KW + k] = id[k]; xw[tid * KW + k] = w[k]; }
  } else if (tid >= 64 && tid < 64 + g.B) {
    const int j = tid - 64;
    const int r = min(max(Y0 + min(j, Bv - 1) + dy, 0), d.out_h - 1);
    int id[kMaxTaps];
    float w[kMaxTaps];
    roi_taps(r, bh, d.out_h, d.antialias, KH, id, w);
    for (int k = 0; k < KH; ++k) { yi[j * KH + k] = id[k]; yw[j * KH + k] = w[k]; }
  }
  __syncthreads();
  // the source window the taps touch (indices are monotonic in the output index; the first tap is the smallest)
  int xlo = xi[0], xhi = xi[0], ylo = yi[0], yhi = yi[0];
  for (int k = 0; k < KW; ++k) xhi = max(xhi, xi[(TWv - 1) * KW + k]);
  for (int k = 0; k < KH; ++k) yhi = max(yhi, yi[(Bv - 1) * KH + k]);
  const int ncol = min(xhi - xlo + 1, g.SP), nrow = min(yhi - ylo + 1, g.R);

  // 2. stage the window's bytes: sb[(row * SP + col) * C + ch]
  const uint8_t* base = f.first + (int64_t)(b.y1 + ylo) * f.rstride + (int64_t)(b.x1 + xlo) * d.sw;
  roi_stage<SRC>(sb, g.SP, C, base, f.rstride, d, f.miss, p.fill, nrow, ncol, tid, kThreads);
  __syncthreads();

  // 3. horizontal pass: tmp[(row * C + ch) * TW + j]
  {
    const int total = nrow * C * TWv;
    for (int e = tid; e < total; e += kThreads) {
      const int j = e % TWv, rc = e / TWv;
      const int ch = rc % C, r = rc / C;
      const unsigned char* row = sb + r * g.SP * C + ch;
      float acc = 0.f;
      for (int k = 0; k < KW; ++k) {
        const int col = min(max(xi[j * KW + k] - xlo, 0), ncol - 1);
        const float p = __fmul_rn(lut[row[col * C]], xw[j * KW + k]);
        acc = k == 0 ? p : __fadd_rn(acc, p);
      }
      tmp[(r * C + ch) * g.TW + j] = acc;
    }
  }
  __syncthreads();

  // 4. vertical pass and the stores, one destination row of one channel plane per TW lanes
  {
    const int total = C * Bv * TWv;
    for (int e = tid; e < total; e += kThreads) {
      const int j = e % TWv, rc = e / TWv;
      const int yy = rc % Bv, ch = rc / Bv;
      float acc = 0.f;
      for (int k = 0; k < KH; ++k) {
        const int r = min(max(yi[yy * KH + k] - ylo, 0), nrow - 1);
        const float p = __fmul_rn(tmp[(r * C + ch) * g.TW + j], yw[yy * KH + k]);
        acc = k == 0 ? p : __fadd_rn(acc, p);
      }
      const int ry = Y0 + yy + dy, rx = X0 + j + dx;
      if (ry < 0 || ry >= d.out_h || rx < 0 || rx >= d.out_w) acc = 0.f;
      D* o = static_cast<D*>(d.dst) + n * d.dn + t * d.dt + (int64_t)(d.c_off + ch) * d.dc + (int64_t)(Y0 + yy) * d.dh + X0 + j;
      *o = (D)acc;
    }
  }
}

// the host-side checks the three entry points share (roi_check, and pad; each checks its own struct_size and its own source
// first), then the launch: p == nullptr is sfk_roi_resize's strided source, otherwise the pool's or the arena's
int roi_resize(const sfk_roi_desc* d, int src, const RoiSrc* p, sfk_stream_t stream) {
  if (d->pad < 0) return SFK_ERR_INVALID;
  if (const int st = roi_check(d)) return st;
  const double sh = (double)d->h / d->out_h, sw = (double)d->w / d->out_w;
  const int KH = roi_max_taps(d->h, d->out_h, d->antialias), KW = roi_max_taps(d->w, d->out_w, d->antialias);
  const double spans_h = sh > 1.0 ? sh : 1.0, spans_w = sw > 1.0 ? sw : 1.0;
  RoiGeo g{};
  bool ok = false;
  for (int budget : {src == kRagged ? kRaggedLdsBudget : kLdsBudget, kLdsBudget}) {
    for (int TW : {64, 32, 16}) {
      for (int B : {16, 8, 4, 2, 1}) {
        g = roi_layout(B, TW, d->c, KH, KW, spans_h, spans_w, d->out_h, d->out_w);
        if (g.lds <= budget) { ok = true; break; }
      }
      if (ok) break;
    }
    if (ok) break;
  }
  if (!ok) return SFK_ERR_UNSUPPORTED;
  const int64_t tiles = (int64_t)g.row_tiles * g.col_tiles;
  if (!roi_grid_fits(tiles, d)) return SFK_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)tiles, (unsigned)d->t, (unsigned)d->n);
  hipLaunchKernelGGL(SFK_ROI_KERNEL(roi_resize_kernel, d->dst_dtype, src), grid, dim3(kThreads), g.lds,
                     static_cast<hipStream_t>(stream), *d, g, p ? *p : RoiSrc{});
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

}  // namespace

extern "C" int sfk_roi_resize(const sfk_roi_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_roi_desc)) return SFK_ERR_INVALID;
  return roi_resize(d, kStacked, nullptr, stream);
}

extern "C" int sfk_roi_resize_pool(const sfk_roi_pool_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_roi_pool_desc)) return SFK_ERR_INVALID;
  sfk_roi_desc r;
  RoiSrc p;
  if (const int st = roi_from_pool(*d, &r, &p)) return st;
  r.crop = d->crop, r.pad = d->pad;
  return roi_resize(&r, kPool, &p, stream);
}

extern "C" int sfk_roi_resize_ragged(const sfk_roi_ragged_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_roi_ragged_desc)) return SFK_ERR_INVALID;
  sfk_roi_desc r;
  RoiSrc p;
  if (const int st = roi_from_ragged(*d, &r, &p)) return st;
  r.crop = d->crop, r.pad = d->pad;
  return roi_resize(&r, kRagged, &p, stream);
}

extern "C" int sfk_roi_pool_abi_version(void) { return SFK_ROI_POOL_ABI_VERSION; }
extern "C" int sfk_roi_ragged_abi_version(void) { return SFK_ROI_RAGGED_ABI_VERSION; }
extern "C" int sfk_v2_abi_version(void) { return SFK_V2_ABI_VERSION; }
