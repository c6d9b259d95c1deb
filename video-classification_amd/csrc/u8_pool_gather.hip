// sfk_u8_pool_gather (include/sfk_pool.h) and sfk_u8_pool_gather_crop (include/sfk_resident.h): the normalised (n, t, c, h, w)
// clip batch built on the device from ONE pool of uint8 HWC frames and a table of frame indices -- the overlapping uniform
// windows of a test video, or, with a table of crop offsets, the randomly cropped clips of a train step.  The two entry points
// share one kernel and one launcher; the crop is a compile-time switch.  Same values as sfk_u8_normalize_crop (eval_input.hip)
// writes from the stacked clips; that kernel stays: its locked signature has no index table, and it is the faster of the
// two on the recorded f32 crop row.
#include "sfk_common.h"
#include "sfk_resident.h"

namespace {

// One output row (all c channels) per block.  Output pixel x of the row reads source pixel x + dx of source row ys, dx =
// left - pad; the output pixels that land inside the frame are x in [x_lo, x_hi), their source pixels [x_lo + dx, x_hi + dx).
// Only the bytes of those pixels, [sp, sp + span) with sp = the first byte of channel c0 of source pixel x_lo + dx and span =
// (x_hi - x_lo - 1)*pitch + c, are staged, at row[shift ..], shift = sp & 15, so that LDS and global addresses share their
// 16-byte phase: every 16-byte unit wholly inside the span is one vector load whatever the row's alignment and the crop, and
// only the (up to two) partial units at the ends go byte by byte.  A row outside the frame, an empty column range or a
// missing frame (index outside [0, frames)) reads nothing.  The offsets are clamped in 64 bits BEFORE they meet an address, so
// no crop value can move a read or an LDS access out of its span.
// CROP == false (the launcher's choice when crop == NULL): ys = y, dx = 0 and the range is the whole row, [0, w), with no per-pixel test left.
template <typename T, bool CROP>
__global__ __launch_bounds__(256) void u8_pool_gather_kernel(const uint8_t* __restrict__ pool, int64_t frame_stride,
                                                             int64_t row_stride, int pitch, int frames, int t, int h, int w,
                                                             int c0, int c, const int32_t* __restrict__ index,
                                                             const int32_t* __restrict__ crop, int pad,
                                                             const float* __restrict__ lut, int fill, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t row[];
  __shared__ float s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  const int y = blockIdx.x % h;
  const int nt = blockIdx.x / h;            // n*t + frame slot
  const int f = index[nt];                  // read once per block; block-uniform
  int64_t ys = y, dx = 0;
  int x_lo = 0, x_hi = w;                   // output pixels [x_lo, x_hi) are inside the frame
  bool row_ok = true;
  if (CROP) {                               // crop is not NULL; read once per block; block-uniform
    const int ni = nt / t;
    ys += (int64_t)crop[2 * ni] - pad;
    dx = (int64_t)crop[2 * ni + 1] - pad;
    const int64_t lo = -dx, hi = (int64_t)w - dx;
    x_lo = (int)(lo < 0 ? 0 : lo > w ? w : lo);
    x_hi = (int)(hi < 0 ? 0 : hi > w ? w : hi);
    row_ok = ys >= 0 && ys < h && x_lo < x_hi;
  }
  const bool miss = f < 0 || f >= frames;
  int shift = 0;
  if (row_ok && !miss) {
    const uint8_t* sp = pool + (int64_t)f * frame_stride + ys * row_stride + ((int64_t)x_lo + dx) * pitch + c0;
    shift = (int)(reinterpret_cast<uintptr_t>(sp) & 15);
    const int64_t end = (int64_t)shift + (int64_t)(x_hi - x_lo - 1) * pitch + c;   // staged bytes are row[shift .. end)
    for (int64_t i = (int64_t)threadIdx.x * 16; i < end; i += 256 * 16) {
      if (i >= shift && i + 16 <= end) {
        *reinterpret_cast<uint4*>(row + i) = *reinterpret_cast<const uint4*>(sp + (i - shift));
      } else {
        const int64_t j0 = i < shift ? shift : i, j1 = i + 16 < end ? i + 16 : end;
        for (int64_t j = j0; j < j1; ++j) row[j] = sp[j - shift];
      }
    }
  }
  __syncthreads();
  const float fv = s_lut[fill];
  const uint8_t* px = row + shift;          // byte (x, ch), x_lo <= x < x_hi, at px[(x - x_lo)*pitch + ch]
  // zero outside the frame, lut[fill] for a missing frame, else the LUT of the staged byte
  auto value = [&](int ch, int x) -> float {
    if (CROP && !(row_ok && x >= x_lo && x < x_hi)) return 0.f;
    return miss ? fv : s_lut[px[(x - x_lo) * pitch + ch]];
  };
  const int64_t plane = (int64_t)h * w;
  T* op = out + (int64_t)nt * c * plane + (int64_t)y * w;                   // element (ch, x) at op[ch*plane + x]
  constexpr int V = DT<T>::VEC;
  if (w % V == 0) {                         // every V-group of a row starts 16-byte aligned (out is, and w % V == 0)
    const int wv = w / V;
    for (int e = threadIdx.x; e < c * wv; e += 256) {
      const int ch = e / wv, x0 = (e % wv) * V;
      Vec16<T> v;
#pragma unroll
      for (int k = 0; k < V; ++k) v.set(k, value(ch, x0 + k));
      v.store(op + ch * plane + x0);
    }
  } else {
    for (int e = threadIdx.x; e < c * w; e += 256) {
      const int ch = e / w, x = e % w;
      op[ch * plane + x] = (T)value(ch, x);
    }
  }
}

template <typename T, bool CROP>
void launch(dim3 grid, size_t lds, hipStream_t s, const uint8_t* pool, int64_t frame_stride, int64_t row_stride, int pitch,
            int frames, int t, int h, int w, int c0, int c, const int32_t* index, const int32_t* crop, int pad,
            const float* lut, int fill, void* out) {
  hipLaunchKernelGGL((u8_pool_gather_kernel<T, CROP>), grid, dim3(256), lds, s, pool, frame_stride, row_stride, pitch, frames,
                     t, h, w, c0, c, index, crop, pad, lut, fill, (T*)out);
}

// every host-side check of both entry points (but struct_size, each its own), then the launch: CROP from crop != NULL
int pool_gather(int out_dtype, const uint8_t* pool, int64_t frame_stride, int64_t row_stride, int pitch, int frames, int h,
                int w, int c0, int c, int n, int t, const int32_t* index, const float* lut, const int32_t* crop, int fill,
                int pad, void* out, sfk_stream_t stream) {
  if (!pool || !index || !lut || !out) return SFK_ERR_INVALID;
  if (frames <= 0 || h <= 0 || w <= 0 || c <= 0 || n <= 0 || t <= 0) return SFK_ERR_INVALID;
  if (frame_stride < 0 || row_stride < 0 || c0 < 0 || pad < 0) return SFK_ERR_INVALID;
  if ((int64_t)pitch < (int64_t)c0 + c) return SFK_ERR_INVALID;
  if (fill < 0 || fill > 255) return SFK_ERR_INVALID;
  if (out_dtype != SFK_F32 && out_dtype != SFK_BF16) return SFK_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(out) & 15) return SFK_ERR_INVALID;
  const int64_t blocks = (int64_t)n * t * h;
  const int64_t span = (int64_t)(w - 1) * pitch + c;
  if (blocks > SFK_POOL_MAX_BLOCKS || span > SFK_POOL_MAX_ROW_BYTES) return SFK_ERR_UNSUPPORTED;
  const size_t lds = ((size_t)span + 15 + 15) / 16 * 16;                    // the widest span behind a shift of up to 15 bytes
  const bool bf = out_dtype == SFK_BF16;
  (crop ? (bf ? launch<bf16_t, true> : launch<float, true>) : (bf ? launch<bf16_t, false> : launch<float, false>))(
      dim3((unsigned)blocks), lds, static_cast<hipStream_t>(stream), pool, frame_stride, row_stride, pitch, frames, t, h, w, c0,
      c, index, crop, pad, lut, fill, out);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

}  // namespace

extern "C" int sfk_u8_pool_gather(const sfk_pool_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_pool_desc)) return SFK_ERR_INVALID;
  return pool_gather(d->out_dtype, d->pool, d->frame_stride, d->row_stride, d->pixel_pitch, d->frames, d->h, d->w, d->c0, d->c,
                     d->n, d->t, d->index, d->lut, nullptr, d->fill, 0, d->out, stream);
}

extern "C" int sfk_u8_pool_gather_crop(const sfk_pool_crop_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_pool_crop_desc)) return SFK_ERR_INVALID;
  return pool_gather(d->out_dtype, d->pool, d->frame_stride, d->row_stride, d->pixel_pitch, d->frames, d->h, d->w, d->c0, d->c,
                     d->n, d->t, d->index, d->lut, d->crop, d->fill, d->pad, d->out, stream);
}

extern "C" int sfk_pool_abi_version(void) { return SFK_POOL_ABI_VERSION; }
extern "C" int sfk_resident_abi_version(void) { return SFK_RESIDENT_ABI_VERSION; }
