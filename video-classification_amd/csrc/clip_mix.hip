// sfk_clip_mix (include/sfk_mix.h): Mixup / CutMix of the clips of a batch with their partners, in place.
//
// The pairing is an involution (a row counts only when partner[partner[n]] == n), so one lane can own one position of BOTH
// members of a pair: it loads the two values, forms the two results from them and writes the two back.  That is one read
// and one write of the clip and no second buffer.  The workgroups of the LOWER member of a pair do the work, those of the
// upper member and of every clip without a valid partner leave at once.
//
// The c channels of a clip are t*c*h rows of w elements; a row is cut into units of V = 16 bytes / sizeof(T) elements (the
// last one may be short), unit u = ((t*c + ch)*h + y) * ceil(w/V) + group.  A workgroup of 256 lanes owns
// SFK_MIX_CHUNK_UNITS = 1024 consecutive units, lane l the units l, 256 + l, 512 + l, 768 + l of the chunk.  A unit that
// neither row changes (lam == 1 and the unit outside the box, for both members) is not loaded; a chunk made of such units
// only (the rows above and below both boxes) is left by the whole workgroup.  A full unit with both addresses 16-byte
// aligned that lies wholly inside or outside each box moves as 16-byte vectors: the four loads of a lane's units are
// issued before the first store.  Every other unit goes element by element.  Both ways run the same arithmetic, written
// without contraction, so the f32 and bf16 instantiations round alike.  Every branch on the table is per pair: uniform.
#include "sfk_common.h"
#include "sfk_mix.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kUnitsPerLane = SFK_MIX_CHUNK_UNITS / kThreads;
static_assert(SFK_MIX_CHUNK_UNITS % kThreads == 0, "a chunk is a whole number of units per lane");

struct MixGeo {
  FastDiv chunks, groups, h, c;   // chunks of a clip; units of a row; rows of a plane; planes of a frame
  uint32_t units;                 // units of a clip
};

// one row of the table as the kernel uses it: the box clamped to the frame, all zero when it is empty
struct MixRow {
  float lam, om;
  int y0, x0, y1, x1;
  bool blend, box;
};

__device__ __forceinline__ int clampi(float v, int hi) { return (int)fminf(fmaxf(v, 0.f), (float)hi); }   // NaN -> 0

__device__ __forceinline__ MixRow read_row(const float* r, int h, int w) {
  MixRow m;
  m.lam = r[1];
  m.om = 1.0f - m.lam;
  m.blend = !(m.lam == 1.0f);
  m.y0 = clampi(r[2], h); m.x0 = clampi(r[3], w); m.y1 = clampi(r[4], h); m.x1 = clampi(r[5], w);
  m.box = m.y1 > m.y0 && m.x1 > m.x0;
  if (!m.box) m.y0 = m.x0 = m.y1 = m.x1 = 0;
  return m;
}

// the partner of row i, or -1 when the table names none inside [0, n)
__device__ __forceinline__ int partner_of(const float* rows, int i, int n) {
  const float pf = rows[SFK_MIX_ROW_FLOATS * (int64_t)i];
  return (pf >= 0.f && pf < (float)n) ? (int)pf : -1;
}

__device__ __forceinline__ float mix1(const MixRow& m, bool in, float own, float other) {
  return in ? other : m.lam * own + m.om * other;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void clip_mix_kernel(sfk_mix_desc d, MixGeo geo) {
  constexpr int V = DT<T>::VEC;
  const int tid = threadIdx.x;
  uint32_t ua, chunk;
  geo.chunks.divmod(blockIdx.x, ua, chunk);
  const int a = (int)ua;
  const int p = partner_of(d.rows, a, d.n);
  if (p <= a) return;                                   // no partner in range, itself, or the upper member of its pair
  if (partner_of(d.rows, p, d.n) != a) return;          // not mutual
  const MixRow A = read_row(d.rows + SFK_MIX_ROW_FLOATS * (int64_t)a, d.h, d.w);
  const MixRow B = read_row(d.rows + SFK_MIX_ROW_FLOATS * (int64_t)p, d.h, d.w);
  if (!A.blend && !B.blend) {
    if (!A.box && !B.box) return;                       // both rows leave their clips as they are
    // only the boxes change: leave when no row of this chunk crosses either of them
    const int ylo = A.box ? (B.box ? min(A.y0, B.y0) : A.y0) : B.y0;
    const int yhi = A.box ? (B.box ? max(A.y1, B.y1) : A.y1) : B.y1;
    const uint32_t u0 = chunk * SFK_MIX_CHUNK_UNITS, u1 = min(u0 + SFK_MIX_CHUNK_UNITS, geo.units) - 1;
    const uint32_t r0 = geo.groups.div(u0), r1 = geo.groups.div(u1);
    if (r1 - r0 + 1 < geo.h.d) {
      uint32_t q0, q1, ya, yb;
      geo.h.divmod(r0, q0, ya);
      geo.h.divmod(r1, q1, yb);
      const bool hit = q0 == q1 ? ((int)ya < yhi && (int)yb >= ylo) : ((int)ya < yhi || (int)yb >= ylo);
      if (!hit) return;
    }
  }

  T* base = static_cast<T*>(d.x);
  T* ca = base + (int64_t)a * d.sn;
  T* cb = base + (int64_t)p * d.sn;

  int64_t off[kUnitsPerLane];
  int mode[kUnitsPerLane];                // 0: nothing to do, 1: vectors, 2: element by element
  int yy[kUnitsPerLane], xx[kUnitsPerLane];
  bool ina[kUnitsPerLane], inb[kUnitsPerLane];   // vectors: the whole unit is inside A's / B's box
  Vec16<T> va[kUnitsPerLane], vb[kUnitsPerLane];
#pragma unroll
  for (int k = 0; k < kUnitsPerLane; ++k) {
    mode[k] = 0;
    const uint32_t u = chunk * SFK_MIX_CHUNK_UNITS + k * kThreads + tid;
    if (u >= geo.units) continue;
    uint32_t r, gq, tc, y, t, ch;
    geo.groups.divmod(u, r, gq);
    geo.h.divmod(r, tc, y);
    geo.c.divmod(tc, t, ch);
    const int x0 = (int)gq * V, x1 = min(x0 + V, d.w);
    // the part of the unit inside each box: [a0, a1) and [b0, b1)
    const bool rowa = A.box && (int)y >= A.y0 && (int)y < A.y1, rowb = B.box && (int)y >= B.y0 && (int)y < B.y1;
    const int a0 = max(A.x0, x0), a1 = min(A.x1, x1), b0 = max(B.x0, x0), b1 = min(B.x1, x1);
    const bool a_none = !rowa || a1 <= a0, b_none = !rowb || b1 <= b0;
    const bool a_all = !a_none && a0 == x0 && a1 == x1, b_all = !b_none && b0 == x0 && b1 == x1;
    if (!A.blend && !B.blend && a_none && b_none) continue;
    off[k] = (int64_t)t * d.st + (int64_t)(d.c_off + (int)ch) * d.sc + (int64_t)y * d.sh + x0;
    yy[k] = (int)y;
    xx[k] = x0;
    ina[k] = a_all;
    inb[k] = b_all;
    const bool vec = x1 - x0 == V && ((((uintptr_t)(ca + off[k])) | ((uintptr_t)(cb + off[k]))) & 15) == 0 &&
                     (a_none || a_all) && (b_none || b_all);
    mode[k] = vec ? 1 : 2;
    if (vec) {
      va[k].load(ca + off[k]);
      vb[k].load(cb + off[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < kUnitsPerLane; ++k) {
    if (mode[k] == 1) {
      Vec16<T> oa, ob;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float xa = va[k].get(j), xb = vb[k].get(j);
        oa.set(j, mix1(A, ina[k], xa, xb));
        ob.set(j, mix1(B, inb[k], xb, xa));
      }
      if (A.blend || ina[k]) oa.store(ca + off[k]);
      if (B.blend || inb[k]) ob.store(cb + off[k]);
    } else if (mode[k] == 2) {
      T* pa = ca + off[k];
      T* pb = cb + off[k];
      const bool rowa = A.box && yy[k] >= A.y0 && yy[k] < A.y1, rowb = B.box && yy[k] >= B.y0 && yy[k] < B.y1;
      const int cnt = min(V, d.w - xx[k]);
      for (int j = 0; j < cnt; ++j) {
        const int x = xx[k] + j;
        const bool ia = rowa && x >= A.x0 && x < A.x1, ib = rowb && x >= B.x0 && x < B.x1;
        const bool wa = A.blend || ia, wb = B.blend || ib;
        if (!wa && !wb) continue;
        const float xa = (float)pa[j], xb = (float)pb[j];
        if (wa) pa[j] = (T)mix1(A, ia, xa, xb);
        if (wb) pb[j] = (T)mix1(B, ib, xb, xa);
      }
    }
  }
}

}  // namespace

extern "C" int sfk_clip_mix(const sfk_mix_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_mix_desc)) return SFK_ERR_INVALID;
  if (!d->x || !d->rows) return SFK_ERR_INVALID;
  if (d->n <= 0 || d->t <= 0 || d->c <= 0 || d->h <= 0 || d->w <= 0) return SFK_ERR_INVALID;
  if (d->sn < 0 || d->st < 0 || d->sc < 0 || d->sh < 0 || d->c_off < 0) return SFK_ERR_INVALID;
  if (d->dtype != SFK_F32 && d->dtype != SFK_BF16) return SFK_ERR_INVALID;
  const int32_t v = sfk_vec_of(d->dtype);
  const int32_t groups = (d->w + v - 1) / v;
  const int64_t rows = (int64_t)d->t * d->c * d->h;
  if (rows > SFK_MIX_MAX_CLIP_UNITS || rows * groups > SFK_MIX_MAX_CLIP_UNITS) return SFK_ERR_UNSUPPORTED;
  const int64_t units = rows * groups;
  const int64_t chunks = (units + SFK_MIX_CHUNK_UNITS - 1) / SFK_MIX_CHUNK_UNITS;
  if (d->n > SFK_MIX_MAX_BLOCKS || d->n * chunks > SFK_MIX_MAX_BLOCKS) return SFK_ERR_UNSUPPORTED;
  MixGeo g;
  g.chunks.set((int32_t)chunks);
  g.groups.set(groups);
  g.h.set(d->h);
  g.c.set(d->c);
  g.units = (uint32_t)units;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)(d->n * chunks)), block(kThreads);
  if (d->dtype == SFK_BF16)
    hipLaunchKernelGGL((clip_mix_kernel<bf16_t>), grid, block, 0, s, *d, g);
  else
    hipLaunchKernelGGL((clip_mix_kernel<float>), grid, block, 0, s, *d, g);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_mix_abi_version(void) { return SFK_MIX_ABI_VERSION; }
