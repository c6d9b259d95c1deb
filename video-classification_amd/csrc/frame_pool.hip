// sfk_u8_pool_gather (include/sfk_pool.h): the (n, t, c, h, w) clip batch of a test video's overlapping uniform windows,
// built on the device from ONE pool of its uint8 HWC frames and a table of frame indices.  Same values as
// sfk_u8_normalize_crop (eval_input.hip) writes from the stacked clips; the kernel stands alone so that one stays as it is.
#include "sfk_common.h"
#include "sfk_pool.h"

namespace {

// One output row (all c channels) per block.  The row's source bytes [sp, sp + span), sp = the first byte of channel c0 of
// pixel 0, span = (w - 1)*pitch + c, are staged at row[shift ..], shift = sp & 15, so that LDS and global addresses share
// their 16-byte phase: every 16-byte unit that lies wholly inside the span is one vector load whatever the row's
// alignment, and only the (up to two) partial units at the ends go byte by byte.  Nothing outside the span is read.
// A missing frame (index outside [0, frames)) reads nothing and writes lut[fill].
template <typename T>
__global__ __launch_bounds__(256) void u8_pool_gather_kernel(const uint8_t* __restrict__ pool, int64_t frame_stride,
                                                             int64_t row_stride, int pitch, int frames, int h, int w, int c0,
                                                             int c, const int32_t* __restrict__ index,
                                                             const float* __restrict__ lut, int fill, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t row[];
  __shared__ float s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  const int y = blockIdx.x % h;
  const int nt = blockIdx.x / h;            // n*t + frame slot
  const int f = index[nt];                  // read once per block; block-uniform
  const bool miss = f < 0 || f >= frames;
  int shift = 0;
  if (!miss) {
    const uint8_t* sp = pool + (int64_t)f * frame_stride + (int64_t)y * row_stride + c0;
    shift = (int)(reinterpret_cast<uintptr_t>(sp) & 15);
    const int64_t end = (int64_t)shift + (int64_t)(w - 1) * pitch + c;      // staged bytes are row[shift .. end)
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
  const uint8_t* px = row + shift;          // byte (x, ch) at px[x*pitch + ch]
  const int64_t plane = (int64_t)h * w;
  T* op = out + (int64_t)nt * c * plane + (int64_t)y * w;                   // element (ch, x) at op[ch*plane + x]
  constexpr int V = DT<T>::VEC;
  if (w % V == 0) {                         // every V-group of a row starts 16-byte aligned (out is, and w % V == 0)
    const int wv = w / V;
    for (int e = threadIdx.x; e < c * wv; e += 256) {
      const int ch = e / wv, x0 = (e % wv) * V;
      Vec16<T> v;
#pragma unroll
      for (int k = 0; k < V; ++k) v.set(k, miss ? fv : s_lut[px[(x0 + k) * pitch + ch]]);
      v.store(op + ch * plane + x0);
    }
  } else {
    for (int e = threadIdx.x; e < c * w; e += 256) {
      const int ch = e / w, x = e % w;
      op[ch * plane + x] = (T)(miss ? fv : s_lut[px[x * pitch + ch]]);
    }
  }
}

}  // namespace

extern "C" int sfk_u8_pool_gather(const sfk_pool_desc* d, sfk_stream_t stream) {
  if (!d || d->struct_size != sizeof(sfk_pool_desc)) return SFK_ERR_INVALID;
  if (!d->pool || !d->index || !d->lut || !d->out) return SFK_ERR_INVALID;
  if (d->frames <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0 || d->n <= 0 || d->t <= 0) return SFK_ERR_INVALID;
  if (d->frame_stride < 0 || d->row_stride < 0 || d->c0 < 0) return SFK_ERR_INVALID;
  if ((int64_t)d->pixel_pitch < (int64_t)d->c0 + d->c) return SFK_ERR_INVALID;
  if (d->fill < 0 || d->fill > 255) return SFK_ERR_INVALID;
  if (d->out_dtype != SFK_F32 && d->out_dtype != SFK_BF16) return SFK_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(d->out) & 15) return SFK_ERR_INVALID;
  const int64_t blocks = (int64_t)d->n * d->t * d->h;
  const int64_t span = (int64_t)(d->w - 1) * d->pixel_pitch + d->c;
  if (blocks > SFK_POOL_MAX_BLOCKS || span > SFK_POOL_MAX_ROW_BYTES) return SFK_ERR_UNSUPPORTED;
  const size_t lds = ((size_t)span + 15 + 15) / 16 * 16;                    // the span behind a shift of up to 15 bytes
  const dim3 grid((unsigned)blocks);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (d->out_dtype == SFK_BF16)
    hipLaunchKernelGGL(u8_pool_gather_kernel<bf16_t>, grid, dim3(256), lds, s, d->pool, d->frame_stride, d->row_stride,
                       d->pixel_pitch, d->frames, d->h, d->w, d->c0, d->c, d->index, d->lut, d->fill, (bf16_t*)d->out);
  else
    hipLaunchKernelGGL(u8_pool_gather_kernel<float>, grid, dim3(256), lds, s, d->pool, d->frame_stride, d->row_stride,
                       d->pixel_pitch, d->frames, d->h, d->w, d->c0, d->c, d->index, d->lut, d->fill, (float*)d->out);
  SFK_CHECK_LAUNCH();
  return SFK_OK;
}

extern "C" int sfk_pool_abi_version(void) { return SFK_POOL_ABI_VERSION; }
