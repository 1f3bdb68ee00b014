// Training-data image preprocessing on the device (gfx950): the reference's crop chain
// (utils/image/common.py:12-77: BOX halvings, one BICUBIC resize, crop; :103-114: flips / transpose) on uint8
// HWC images, bit-exact to Pillow's 8-bit resampling (Resample.c: ImagingResampleHorizontal_8bpc /
// ImagingResampleVertical_8bpc). The host computes Pillow's coefficient tables (precompute_coeffs +
// normalize_coeffs_8bpc, 22 fractional bits); the kernels only evaluate
//     out = clip8((2^21 + sum_t kk[o][t] * px[bounds[o][0] + t]) >> 22)
// in int32 (255 * sum|kk| < 2^31 for BOX and BICUBIC), so the result does not depend on the summation order.
// Memory- and launch-bound: no MFMA, a few launches per image.
#include "common.h"
#include "../../include/rdeic_hip.h"

namespace {

constexpr int PREC = 22;
constexpr int H_TP = 64;  // output pixels per block of the horizontal pass
constexpr int H_R = 4;    // rows per block of the horizontal pass (they share the staged coefficient rows)

__device__ __forceinline__ uint32_t clip8(int acc) { return (uint32_t)min(max(acc >> PREC, 0), 255); }

// Vertical pass. A row is a flat byte array: output byte (y, c) = sum_t kk[y][t] * src[(ymin + t), c]. One output
// row per block row, so bounds / kk are wave-uniform. A thread owns the 4 bytes of one dword of the source row
// (dword loads when `fast & 1`: base and stride 4-aligned); the window's partial head and tail dwords, and every
// column of an unaligned source, go byte by byte. `fast & 2`: the destination takes dword stores.
__global__ void __launch_bounds__(256)
resample_v_kernel(const uint8_t* __restrict__ src, long sstride, int src_row0, int src_rows,
                  const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int y0, int cb0, int ncb,
                  uint8_t* __restrict__ dst, long dstride, int fast) {
  const int y = y0 + blockIdx.y;
  const int ymin = bounds[2 * y];
  const int cnt = min(bounds[2 * y + 1], ksize);
  const int* __restrict__ k = kk + (long)y * ksize;
  const int a = (cb0 & ~3) + 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int lo = max(a, cb0), hi = min(a + 4, cb0 + ncb);
  if (lo >= hi) return;
  uint8_t* __restrict__ out = dst + (long)blockIdx.y * dstride + (lo - cb0);
  if ((fast & 1) && hi - lo == 4) {
    int acc0 = 1 << (PREC - 1), acc1 = acc0, acc2 = acc0, acc3 = acc0;
    for (int t = 0; t < cnt; ++t) {
      const int r = ymin + t - src_row0;
      if ((unsigned)r >= (unsigned)src_rows) continue;  // tables are trusted; a bad one must still not fault
      const uint32_t v = *reinterpret_cast<const uint32_t*>(src + (long)r * sstride + a);
      const int c = k[t];
      acc0 += c * (int)(v & 255u);
      acc1 += c * (int)((v >> 8) & 255u);
      acc2 += c * (int)((v >> 16) & 255u);
      acc3 += c * (int)(v >> 24);
    }
    const uint32_t o = clip8(acc0) | (clip8(acc1) << 8) | (clip8(acc2) << 16) | (clip8(acc3) << 24);
    if (fast & 2) {
      *reinterpret_cast<uint32_t*>(out) = o;
    } else {
      out[0] = (uint8_t)o, out[1] = (uint8_t)(o >> 8), out[2] = (uint8_t)(o >> 16), out[3] = (uint8_t)(o >> 24);
    }
    return;
  }
  for (int c = lo; c < hi; ++c) {
    int acc = 1 << (PREC - 1);
    for (int t = 0; t < cnt; ++t) {
      const int r = ymin + t - src_row0;
      if ((unsigned)r >= (unsigned)src_rows) continue;
      acc += k[t] * (int)src[(long)r * sstride + c];
    }
    out[c - lo] = (uint8_t)clip8(acc);
  }
}

// Horizontal pass. Every output pixel has its own tap window, so a block stages in LDS the coefficient rows of
// its H_TP output pixels and, for each of its H_R rows, the source segment those pixels read (global dwords to
// LDS dwords; the segment's unaligned head and tail byte by byte). A thread then produces 4 consecutive output
// bytes. LDS: kk[H_TP][ksize] | bounds[H_TP][2] | seg[H_R][pitch], pitch = round4(3 * seg_max) + 4.
__global__ void __launch_bounds__(256)
resample_h_kernel(const uint8_t* __restrict__ src, long sstride, int src_w, const int* __restrict__ bounds,
                  const int* __restrict__ kk, int ksize, int seg_max, int pitch, int y0, int nrows, int x0, int npix,
                  uint8_t* __restrict__ dst, long dstride, int fast) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* kks = reinterpret_cast<int*>(smem);
  int* bnd = kks + H_TP * ksize;
  uint8_t* seg = reinterpret_cast<uint8_t*>(bnd + 2 * H_TP);
  const int tid = threadIdx.x;
  const int xa = x0 + blockIdx.x * H_TP;
  const int tp = min(H_TP, x0 + npix - xa);
  const int ya = y0 + blockIdx.y * H_R;
  const int rows = min(H_R, y0 + nrows - ya);
  for (int i = tid; i < tp * ksize; i += blockDim.x) kks[i] = kk[(long)xa * ksize + i];
  for (int i = tid; i < tp * 2; i += blockDim.x) bnd[i] = bounds[2 * xa + i];
  // xmin and xmin + xmax both grow with the output index: the block reads [first xmin, last end)
  const int s0 = min(max(bounds[2 * xa], 0), src_w);
  const int s1 = min(max(bounds[2 * (xa + tp - 1)] + bounds[2 * (xa + tp - 1) + 1], s0), src_w);
  const int seglen = min(s1 - s0, seg_max);
  const int nb = seglen * 3;
  for (int r = 0; r < rows; ++r) {
    const uint8_t* g = src + (long)(ya + r) * sstride + (long)s0 * 3;
    const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 3);  // LDS keeps the global dword phase
    uint8_t* l = seg + r * pitch + mis;
    const int head = min((4 - mis) & 3, nb);
    const int ndw = (nb - head) >> 2;
    for (int i = tid; i < head; i += blockDim.x) l[i] = g[i];
    const uint32_t* g4 = reinterpret_cast<const uint32_t*>(g + head);
    uint32_t* l4 = reinterpret_cast<uint32_t*>(l + head);
    for (int j = tid; j < ndw; j += blockDim.x) l4[j] = g4[j];
    for (int i = head + 4 * ndw + tid; i < nb; i += blockDim.x) l[i] = g[i];
  }
  __syncthreads();
  if (seglen <= 0) return;
  const int tb = tp * 3, quads = (tb + 3) >> 2;
  for (int it = tid; it < quads * rows; it += blockDim.x) {
    const int r = it / quads, e0 = (it - r * quads) * 4;
    const int mis = (int)(reinterpret_cast<uintptr_t>(src + (long)(ya + r) * sstride + (long)s0 * 3) & 3);
    const uint8_t* l = seg + r * pitch + mis;
    const int ne = min(4, tb - e0);
    uint32_t o = 0;
    for (int q = 0; q < ne; ++q) {
      const int e = e0 + q, p = e / 3, c = e - 3 * p;
      const int xmin = bnd[2 * p] - s0, cnt = min(bnd[2 * p + 1], ksize);
      int acc = 1 << (PREC - 1);
      for (int t = 0; t < cnt; ++t) {
        const int idx = min(max(xmin + t, 0), seglen - 1);
        acc += kks[p * ksize + t] * (int)l[idx * 3 + c];
      }
      o |= clip8(acc) << (8 * q);
    }
    uint8_t* out = dst + (long)(ya - y0 + r) * dstride + (long)(xa - x0) * 3 + e0;
    if ((fast & 2) && ne == 4) {
      *reinterpret_cast<uint32_t*>(out) = o;
    } else {
      for (int q = 0; q < ne; ++q) out[q] = (uint8_t)(o >> (8 * q));
    }
  }
}

// Crop, flips and transpose in the reference's order (crop; cv2.flip 1; cv2.flip 0; transpose(1, 0, 2)) as one
// gather: out[i][j] = win[vflip ? h-1-y : y][hflip ? w-1-x : x], (y, x) = transpose ? (j, i) : (i, j). A thread
// writes 4 consecutive bytes of the dense [oh][ow][3] output.
__global__ void __launch_bounds__(256)
crop_flip_kernel(const uint8_t* __restrict__ src, long sstride, int cy, int cx, int h, int w, int hflip, int vflip,
                 int tr, uint8_t* __restrict__ dst, int aligned) {
  const int oh = tr ? w : h, ow = tr ? h : w;
  const long total = (long)oh * ow * 3;
  const long e0 = 4 * (blockIdx.x * (long)blockDim.x + threadIdx.x);
  if (e0 >= total) return;
  const int ne = (int)min(4L, total - e0);
  uint32_t o = 0;
  for (int q = 0; q < ne; ++q) {
    const long e = e0 + q;
    const long px = e / 3;
    const int c = (int)(e - 3 * px);
    const int i = (int)(px / ow), j = (int)(px - (long)i * ow);
    int y = tr ? j : i, x = tr ? i : j;
    if (vflip) y = h - 1 - y;
    if (hflip) x = w - 1 - x;
    o |= (uint32_t)src[(long)(cy + y) * sstride + (long)(cx + x) * 3 + c] << (8 * q);
  }
  if (aligned && ne == 4) {
    *reinterpret_cast<uint32_t*>(dst + e0) = o;
  } else {
    for (int q = 0; q < ne; ++q) dst[e0 + q] = (uint8_t)(o >> (8 * q));
  }
}

inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" int rdeic_resample_v_u8(const uint8_t* src, int64_t src_stride, int32_t src_row_bytes, int32_t src_row0,
                                   int32_t src_rows, const int32_t* bounds, const int32_t* kk, int32_t ksize,
                                   int32_t out_size, int32_t y0, int32_t nrows, int32_t cb0, int32_t ncb,
                                   uint8_t* dst, int64_t dst_stride, void* stream) {
  if (!src || !bounds || !kk || !dst || ksize <= 0 || src_rows <= 0 || src_row_bytes <= 0 ||
      src_stride < src_row_bytes || y0 < 0 || nrows <= 0 || nrows > 65535 || (int64_t)y0 + nrows > out_size ||
      cb0 < 0 || ncb <= 0 || (int64_t)cb0 + ncb > src_row_bytes || dst_stride < ncb)
    return RDEIC_EINVAL;
  const int fast = ((al4(src) && (src_stride & 3) == 0) ? 1 : 0) |
                   ((al4(dst) && (dst_stride & 3) == 0 && (cb0 & 3) == 0) ? 2 : 0);
  const int ndw = (cb0 + ncb + 3) / 4 - cb0 / 4;
  hipLaunchKernelGGL(resample_v_kernel, dim3(cdiv(ndw, 256), nrows), dim3(256), 0, (hipStream_t)stream, src,
                     (long)src_stride, src_row0, src_rows, bounds, kk, ksize, y0, cb0, ncb, dst, (long)dst_stride,
                     fast);
  return launch_status();
}

extern "C" int rdeic_resample_h_u8(const uint8_t* src, int64_t src_stride, int32_t src_h, int32_t src_w,
                                   const int32_t* bounds, const int32_t* kk, int32_t ksize, int32_t out_size, int32_t seg_max, int32_t y0,
                                   int32_t nrows, int32_t x0, int32_t npix, uint8_t* dst, int64_t dst_stride,
                                   void* stream) {
  if (!src || !bounds || !kk || !dst || ksize <= 0 || src_w <= 0 || src_stride < (int64_t)src_w * 3 || seg_max <= 0 ||
      y0 < 0 || nrows <= 0 || (int64_t)y0 + nrows > src_h || x0 < 0 || npix <= 0 ||
      (int64_t)x0 + npix > out_size || dst_stride < (int64_t)npix * 3)
    return RDEIC_EINVAL;
  const int pitch = ((seg_max * 3 + 3) & ~3) + 4;
  const size_t lds = (size_t)H_TP * ksize * 4 + H_TP * 8 + (size_t)H_R * pitch;
  const int gy = cdiv(nrows, H_R);
  if (lds > 64 * 1024 || gy > 65535) return RDEIC_EINVAL;
  const int fast = (al4(dst) && (dst_stride & 3) == 0) ? 2 : 0;
  hipLaunchKernelGGL(resample_h_kernel, dim3(cdiv(npix, H_TP), gy), dim3(256), lds, (hipStream_t)stream, src,
                     (long)src_stride, src_w, bounds, kk, ksize, seg_max, pitch, y0, nrows, x0, npix, dst,
                     (long)dst_stride, fast);
  return launch_status();
}

extern "C" int rdeic_crop_flip_u8(const uint8_t* src, int64_t src_stride, int32_t src_h, int32_t src_w,
                                  int32_t crop_y, int32_t crop_x, int32_t h, int32_t w, int32_t hflip, int32_t vflip,
                                  int32_t transpose, uint8_t* dst, void* stream) {
  if (!src || !dst || h <= 0 || w <= 0 || crop_y < 0 || crop_x < 0 || (int64_t)crop_y + h > src_h ||
      (int64_t)crop_x + w > src_w || src_stride < (int64_t)src_w * 3)
    return RDEIC_EINVAL;
  const long quads = ((long)h * w * 3 + 3) / 4;
  hipLaunchKernelGGL(crop_flip_kernel, dim3(cdiv(quads, 256)), dim3(256), 0, (hipStream_t)stream, src,
                     (long)src_stride, crop_y, crop_x, h, w, hflip ? 1 : 0, vflip ? 1 : 0, transpose ? 1 : 0, dst,
                     al4(dst) ? 1 : 0);
  return launch_status();
}
