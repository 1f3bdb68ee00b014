// LPIPS (Zhang et al. 2018, v0.1) on the device: the three kernels around the fp32 backbone convs
// (reference model/lpips.py; the network table, the weights and the chunking live in rdeic_amd/lpips.py).
//
//   * prep: uint8 RGB [n][h][w][3] -> fp32 NHWC [n][h][w][4], channels 0..2 the ScalingLayer for inputs in
//     [0, 1] (model/lpips.py:108-126): (((v / 255) * 2 - 1) - shift_c) / scale_c, evaluated in that order
//     in fp32 (this TU is built with -ffp-contract=off); channel 3 is zero, so conv1 takes the 16-byte gather;
//   * max pool: window k, stride s, no padding, floor mode (torchvision AlexNet 3/2, VGG16 2/2);
//   * layer distance (model/lpips.py:81-85, 226-232: normalize_tensor, squared difference, the 1x1 `lin`
//     conv and spatial_average in one pass): per image
//         mean_p sum_c lin_c (a_pc / (|a_p| + 1e-10) - b_pc / (|b_p| + 1e-10))^2.
//     A quarter wave (one 16-lane DPP row) per pixel keeps both feature vectors in registers (c <= 512: at
//     most 8 float4 per lane per map), reduces the two norms across its 16 lanes and forms the difference
//     directly: the expanded form
//     S_aa/na^2 - 2 S_ab/(na nb) + S_bb/nb^2 cancels catastrophically for near-identical images. An all-zero
//     feature vector gives 0 / 1e-10 = 0. Blocks of LD_PPB pixels write one partial each; a finalize kernel
//     adds an image's partials in a fixed order in fp64. The grid of an image depends on (hw, c) alone, so a
//     score does not depend on the batch and repeats bit for bit.
//
// Every offset is 64-bit.
#include <algorithm>

#include "common.h"
#include "../../include/rdeic_hip.h"

namespace {

constexpr int LD_PPB = 32;     // pixels per block of the layer distance: 16 quarter waves, 2 pixels each
constexpr int LD_MAXC = 512;   // 8 float4 per lane per map

struct Affine3 { float shift[3], scale[3]; };

__global__ __launch_bounds__(256) void lpips_prep_kernel(const uint8_t* __restrict__ img, long npix, Affine3 af,
                                                         float* __restrict__ out) {
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const uint8_t* s = img + p * 3;
    f32x4 v;
    v.x = ((((float)s[0] / 255.f) * 2.f - 1.f) - af.shift[0]) / af.scale[0];
    v.y = ((((float)s[1] / 255.f) * 2.f - 1.f) - af.shift[1]) / af.scale[1];
    v.z = ((((float)s[2] / 255.f) * 2.f - 1.f) - af.shift[2]) / af.scale[2];
    v.w = 0.f;
    *reinterpret_cast<f32x4*>(out + p * 4) = v;
  }
}

// torch's max_pool2d comparison: a NaN wins and stays
__device__ __forceinline__ float pool_max(float m, float v) { return (v > m || v != v) ? v : m; }

// one thread per V output channels of one output pixel; V = 4 needs c, both ld % 4 == 0 and 16-byte bases
template <int V>
__global__ __launch_bounds__(256) void maxpool_kernel(const float* __restrict__ in, int h, int w, int c, int ld_in,
                                                      int k, int s, int ho, int wo, float* __restrict__ out,
                                                      int ld_out, long total) {
  const int cv = c / V;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ch = (int)(i % cv) * V;
    const long op = i / cv;  // output pixel over the batch
    const int ox = (int)(op % wo);
    const long t = op / wo;
    const int oy = (int)(t % ho);
    const long img = t / ho;
    const float* base = in + ((img * h + (long)oy * s) * w + (long)ox * s) * ld_in + ch;
    float m[V];
#pragma unroll
    for (int e = 0; e < V; ++e) m[e] = base[e];
    for (int dy = 0; dy < k; ++dy)
      for (int dx = 0; dx < k; ++dx) {
        const float* q = base + ((long)dy * w + dx) * ld_in;
        if constexpr (V == 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(q);
          m[0] = pool_max(m[0], v.x); m[1] = pool_max(m[1], v.y);
          m[2] = pool_max(m[2], v.z); m[3] = pool_max(m[3], v.w);
        } else {
          m[0] = pool_max(m[0], q[0]);
        }
      }
    float* o = out + op * ld_out + ch;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(o) = f32x4{m[0], m[1], m[2], m[3]};
    else o[0] = m[0];
  }
}

// Lane l (0..15) of the pixel's quarter wave holds channels (l + 16 j) * 4 + e, j < NJ = c / 64, e < 4: 256
// contiguous bytes per pixel per load instruction. The mapping (and so the summation order) is a function of c
// alone; WIDE only says the 4 values may come in one 16-byte load (ld % 4 == 0, aligned bases).
template <bool WIDE>
__device__ __forceinline__ f32x4 load4(const float* __restrict__ p) {
  if constexpr (WIDE) return *reinterpret_cast<const f32x4*>(p);
  else return f32x4{p[0], p[1], p[2], p[3]};
}

// sum over the 16 lanes of a quarter wave (butterfly: every lane ends with the same bits)
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}

// grid (blocks per image, n); part[img][block] = sum over the block's pixels of the pixel distance.
// Quarter wave g (0..15) of the block takes pixels p0 + g and p0 + 16 + g, in that order; for c <= 256 the loads
// of both are issued before the first reduction. A pixel past the image's last loads nothing and contributes
// 0 / (0 + 1e-10) = 0, so the shuffles run under no divergent branch.
template <int NJ, bool WIDE>
__global__ __launch_bounds__(256) void layer_dist_kernel(const float* __restrict__ f0, int ld0,
                                                         const float* __restrict__ f1, int ld1,
                                                         const float* __restrict__ lin, long hw,
                                                         float* __restrict__ part) {
  constexpr int R = LD_PPB / 16;        // pixels per quarter wave
  constexpr int U = NJ <= 4 ? R : 1;    // of them in flight at once
  __shared__ float red[16];
  const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
  const long img = blockIdx.y;
  const long p0 = (long)blockIdx.x * LD_PPB;
  f32x4 wl[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wl[j] = load4<WIDE>(lin + (l + 16 * j) * 4);
  float acc = 0.f;  // this quarter wave's pixels, in order
#pragma unroll
  for (int r = 0; r < R; r += U) {
    f32x4 a[U][NJ], b[U][NJ];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long q = p0 + 16 * (r + u) + g;
      const bool in = q < hw;
      const float* pa = f0 + (img * hw + (in ? q : 0)) * ld0;
      const float* pb = f1 + (img * hw + (in ? q : 0)) * ld1;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        a[u][j] = in ? load4<WIDE>(pa + (l + 16 * j) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        b[u][j] = in ? load4<WIDE>(pb + (l + 16 * j) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        sa += a[u][j].x * a[u][j].x; sa += a[u][j].y * a[u][j].y; sa += a[u][j].z * a[u][j].z; sa += a[u][j].w * a[u][j].w;
        sb += b[u][j].x * b[u][j].x; sb += b[u][j].y * b[u][j].y; sb += b[u][j].z * b[u][j].z; sb += b[u][j].w * b[u][j].w;
      }
      const float na = sqrtf(row_sum(sa)) + 1e-10f, nb = sqrtf(row_sum(sb)) + 1e-10f;
      float d2 = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const f32x4 d = a[u][j] / na - b[u][j] / nb;
        d2 += wl[j].x * (d.x * d.x); d2 += wl[j].y * (d.y * d.y); d2 += wl[j].z * (d.z * d.z); d2 += wl[j].w * (d.w * d.w);
      }
      acc += row_sum(d2);
    }
  }
  if (l == 0) red[g] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) s += red[i];
    part[img * gridDim.x + blockIdx.x] = s;
  }
}

// one block per image: out[img] (+)= sum of the image's partials (fp64, fixed order) / hw
__global__ __launch_bounds__(256) void layer_dist_finalize_kernel(const float* __restrict__ part, long nblk, double hw,
                                                                  int accumulate, float* __restrict__ out) {
  __shared__ double red[4];
  const long img = blockIdx.x;
  const int t = threadIdx.x;
  double s = 0.0;
  for (long i = t; i < nblk; i += 256) s += (double)part[img * nblk + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    const float v = (float)(((red[0] + red[1]) + (red[2] + red[3])) / hw);
    out[img] = accumulate ? out[img] + v : v;
  }
}

template <int NJ>
void launch_layer_dist(bool wide, dim3 grid, hipStream_t s, const float* f0, int ld0, const float* f1, int ld1,
                       const float* lin, long hw, float* part) {
  if (wide) hipLaunchKernelGGL((layer_dist_kernel<NJ, true>), grid, dim3(256), 0, s, f0, ld0, f1, ld1, lin, hw, part);
  else hipLaunchKernelGGL((layer_dist_kernel<NJ, false>), grid, dim3(256), 0, s, f0, ld0, f1, ld1, lin, hw, part);
}

}  // namespace

extern "C" int rdeic_lpips_prep(const uint8_t* img, int32_t n, int32_t h, int32_t w, float* out, void* stream) {
  if (!img || !out || n <= 0 || h <= 0 || w <= 0 || ((uintptr_t)out) % 16) return RDEIC_EINVAL;
  const long npix = (long)n * h * w;
  const Affine3 af = {{-0.030f, -0.088f, -0.188f}, {0.458f, 0.448f, 0.450f}};
  hipLaunchKernelGGL(lpips_prep_kernel, dim3((unsigned)std::min<long>((npix + 255) / 256, 65536)), dim3(256), 0,
                     (hipStream_t)stream, img, npix, af, out);
  return launch_status();
}

extern "C" int rdeic_maxpool2d(const float* in, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_in, int32_t k,
                               int32_t s, float* out, int32_t ld_out, void* stream) {
  if (!in || !out || n <= 0 || c <= 0 || k <= 0 || s <= 0 || h < k || w < k || ld_in < c || ld_out < c)
    return RDEIC_EINVAL;
  const int ho = (h - k) / s + 1, wo = (w - k) / s + 1;
  const bool v4 = c % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && ((uintptr_t)in) % 16 == 0 &&
                  ((uintptr_t)out) % 16 == 0;
  const long total = (long)n * ho * wo * (v4 ? c / 4 : c);
  const dim3 grid((unsigned)std::min<long>((total + 255) / 256, 1L << 20));
  if (v4)
    hipLaunchKernelGGL(maxpool_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, in, h, w, c, ld_in, k, s, ho, wo,
                       out, ld_out, total);
  else
    hipLaunchKernelGGL(maxpool_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, in, h, w, c, ld_in, k, s, ho, wo,
                       out, ld_out, total);
  return launch_status();
}

extern "C" size_t rdeic_lpips_layer_ws_floats(int32_t n, int64_t hw, int32_t c) {
  if (n <= 0 || hw <= 0 || c <= 0) return 0;
  return (size_t)n * (size_t)((hw + LD_PPB - 1) / LD_PPB);
}

extern "C" int rdeic_lpips_layer(const float* f0, int32_t ld0, const float* f1, int32_t ld1, const float* lin,
                                 int32_t n, int64_t hw, int32_t c, int32_t accumulate, float* ws, size_t ws_floats,
                                 float* out, void* stream) {
  if (!f0 || !f1 || !lin || !ws || !out || n <= 0 || hw <= 0 || c <= 0 || c % 64 || c > LD_MAXC || ld0 < c ||
      ld1 < c || n > 65535)
    return RDEIC_EINVAL;
  if (ws_floats < rdeic_lpips_layer_ws_floats(n, hw, c)) return RDEIC_ENOSPC;
  const long nblk = (hw + LD_PPB - 1) / LD_PPB;
  if (nblk > 0x7fffffffL) return RDEIC_EINVAL;
  const bool wide = ld0 % 4 == 0 && ld1 % 4 == 0 && !(((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)lin) & 15);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nblk, n);
  switch (c / 64) {
    case 1: launch_layer_dist<1>(wide, grid, s, f0, ld0, f1, ld1, lin, hw, ws); break;
    case 2: launch_layer_dist<2>(wide, grid, s, f0, ld0, f1, ld1, lin, hw, ws); break;
    case 3: launch_layer_dist<3>(wide, grid, s, f0, ld0, f1, ld1, lin, hw, ws); break;
    case 4: launch_layer_dist<4>(wide, grid, s, f0, ld0, f1, ld1, lin, hw, ws); break;
    case 5: launch_layer_dist<5>(wide, grid, s, f0, ld0, f1, ld1, lin, hw, ws); break;
    case 6: launch_layer_dist<6>(wide, grid, s, f0, ld0, f1, ld1, lin, hw, ws); break;
    case 7: launch_layer_dist<7>(wide, grid, s, f0, ld0, f1, ld1, lin, hw, ws); break;
    default: launch_layer_dist<8>(wide, grid, s, f0, ld0, f1, ld1, lin, hw, ws); break;
  }
  hipLaunchKernelGGL(layer_dist_finalize_kernel, dim3(n), dim3(256), 0, s, ws, nblk, (double)hw, accumulate, out);
  return launch_status();
}
