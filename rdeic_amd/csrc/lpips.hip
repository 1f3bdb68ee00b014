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
// The backward of the training loss (rdeic_amd/lpips.py, LPIPS.loss), prediction side only:
//   * float prep: NHWC fp32 / bf16 images in [-1, 1] (the reference's inp_range) -> the same 4-channel fp32
//     tensor, (v - shift_c) / scale_c;
//   * layer-distance backward: with r = |f0_p|, s = r + 1e-10, n0 = f0 / s, n1 likewise and G the upstream
//     gradient of the image's score, g_c = 2 lin_c (n0_c - n1_c) G / hw and
//     df0_c = g_c / s - f0_c (sum_c g_c f0_c) / (r s^2), in the forward's quarter-wave-per-pixel layout.
//     An all-zero pixel of f0 (r = 0, where the norm has no derivative and g_c / 1e-10 would be of the
//     order 1e10) gets exactly 0: the taps are ReLU outputs, whose mask removes that gradient anyway;
//   * max-pool backward in gather form: an input element adds the gradients of the windows that cover it
//     and whose first maximum (row-major scan, strict >) it is, in output row-major order;
//   * strided conv input gradient for cin <= 4 in gather form (AlexNet's 11x11 / 4 conv1): a quarter wave
//     per input pixel, the lanes over cout, the ReLU mask of the conv's output and the prep backward
//     (divide by scale_c, drop channel 3, the caller's pixel stride and dtype) fused in.
// None uses an atomic: every output element is one fixed-order sum, so two runs agree bit for bit.
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

// one thread per V output channels of one output pixel; V = 4 needs c, both ld % 4 == 0 and 16-byte bases.
// The p = 0, max-only case of fid.hip's pool2d_kernel (the same bits); kept because it measured faster.
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

template <typename T>
__global__ __launch_bounds__(256) void lpips_prep_float_kernel(const T* __restrict__ img, int ld, long npix, Affine3 af,
                                                               float* __restrict__ out) {
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const T* s = img + p * ld;
    f32x4 v;
    v.x = (to_f32(s[0]) - af.shift[0]) / af.scale[0];
    v.y = (to_f32(s[1]) - af.shift[1]) / af.scale[1];
    v.z = (to_f32(s[2]) - af.shift[2]) / af.scale[2];
    v.w = 0.f;
    *reinterpret_cast<f32x4*>(out + p * 4) = v;
  }
}

template <bool WIDE>
__device__ __forceinline__ void store4(float* __restrict__ p, f32x4 v) {
  if constexpr (WIDE) *reinterpret_cast<f32x4*>(p) = v;
  else { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
}

// grid (blocks per image, n), the forward's pixel and channel mapping; df0 (+)= the gradient of the pixel's
// distance with respect to f0. gs[img] is the upstream gradient of the image's score.
template <int NJ, bool WIDE>
__global__ __launch_bounds__(256) void layer_dist_bwd_kernel(const float* __restrict__ f0, int ld0,
                                                             const float* __restrict__ f1, int ld1,
                                                             const float* __restrict__ lin,
                                                             const float* __restrict__ gs, long hw, int accumulate,
                                                             float* __restrict__ df0, int ldd) {
  constexpr int R = LD_PPB / 16;
  const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
  const long img = blockIdx.y;
  const long p0 = (long)blockIdx.x * LD_PPB;
  const float gscale = 2.f * gs[img] / (float)hw;
  f32x4 wl[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wl[j] = load4<WIDE>(lin + (l + 16 * j) * 4);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long q = p0 + 16 * r + g;
    const bool in = q < hw;
    const float* pa = f0 + (img * hw + (in ? q : 0)) * ld0;
    const float* pb = f1 + (img * hw + (in ? q : 0)) * ld1;
    f32x4 a[NJ], b[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      a[j] = in ? load4<WIDE>(pa + (l + 16 * j) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
      b[j] = in ? load4<WIDE>(pb + (l + 16 * j) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      sa += a[j].x * a[j].x; sa += a[j].y * a[j].y; sa += a[j].z * a[j].z; sa += a[j].w * a[j].w;
      sb += b[j].x * b[j].x; sb += b[j].y * b[j].y; sb += b[j].z * b[j].z; sb += b[j].w * b[j].w;
    }
    const float ra = sqrtf(row_sum(sa));
    const float na = ra + 1e-10f, nb = sqrtf(row_sum(sb)) + 1e-10f;
    f32x4 gc[NJ];
    float dot = 0.f;  // sum_c g_c f0_c
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      gc[j] = wl[j] * (a[j] / na - b[j] / nb) * gscale;
      dot += gc[j].x * a[j].x; dot += gc[j].y * a[j].y; dot += gc[j].z * a[j].z; dot += gc[j].w * a[j].w;
    }
    dot = row_sum(dot);
    const bool live = ra > 0.f;
    const float k2 = live ? dot / (ra * (na * na)) : 0.f;
    if (in) {
      float* pd = df0 + (img * hw + q) * ldd;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        f32x4 d = live ? gc[j] / na - a[j] * k2 : f32x4{0.f, 0.f, 0.f, 0.f};
        float* o = pd + (l + 16 * j) * 4;
        if (accumulate) d = load4<WIDE>(o) + d;
        store4<WIDE>(o, d);
      }
    }
  }
}

template <int NJ>
void launch_layer_dist_bwd(bool wide, dim3 grid, hipStream_t s, const float* f0, int ld0, const float* f1, int ld1,
                           const float* lin, const float* gs, long hw, int accumulate, float* df0, int ldd) {
  if (wide)
    hipLaunchKernelGGL((layer_dist_bwd_kernel<NJ, true>), grid, dim3(256), 0, s, f0, ld0, f1, ld1, lin, gs, hw,
                       accumulate, df0, ldd);
  else
    hipLaunchKernelGGL((layer_dist_bwd_kernel<NJ, false>), grid, dim3(256), 0, s, f0, ld0, f1, ld1, lin, gs, hw,
                       accumulate, df0, ldd);
}

// one thread per V channels of one input pixel (channel fastest; V = 4 needs c, every ld % 4 == 0 and 16-byte
// bases, as the forward). The windows that cover (iy, ix) are oy in [ceil((iy - k + 1) / s), iy / s] within
// [0, ho), ox likewise; each is scanned as the forward scans it (torch: a later value replaces the maximum when
// it is greater, or a NaN).
template <int V>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ in, int h, int w, int c, int ld_in,
                                                          const float* __restrict__ dy, int ld_dy, int k, int s,
                                                          int ho, int wo, float* __restrict__ dx, int ld_dx,
                                                          long total) {
  const int cv = c / V;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ch = (int)(i % cv) * V;
    const long ip = i / cv;  // input pixel over the batch
    const int ix = (int)(ip % w);
    const long t = ip / w;
    const int iy = (int)(t % h);
    const long img = t / h;
    const int oy0 = iy >= k ? (iy - k) / s + 1 : 0, oy1 = min(iy / s, ho - 1);
    const int ox0 = ix >= k ? (ix - k) / s + 1 : 0, ox1 = min(ix / s, wo - 1);
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy)
      for (int ox = ox0; ox <= ox1; ++ox) {
        const float* base = in + ((img * h + (long)oy * s) * w + (long)ox * s) * ld_in + ch;
        float m[V];
        int am[V];
#pragma unroll
        for (int e = 0; e < V; ++e) { m[e] = base[e]; am[e] = 0; }
        for (int dyy = 0; dyy < k; ++dyy)
          for (int dxx = 0; dxx < k; ++dxx) {
            const float* q = base + ((long)dyy * w + dxx) * ld_in;
            float ve[V];
            if constexpr (V == 4) {
              const f32x4 v = *reinterpret_cast<const f32x4*>(q);
              ve[0] = v.x; ve[1] = v.y; ve[2] = v.z; ve[3] = v.w;
            } else {
              ve[0] = q[0];
            }
#pragma unroll
            for (int e = 0; e < V; ++e)
              if (ve[e] > m[e] || ve[e] != ve[e]) { m[e] = ve[e]; am[e] = dyy * k + dxx; }
          }
        const int mine = (iy - oy * s) * k + (ix - ox * s);
        const float* g = dy + ((img * ho + oy) * wo + ox) * ld_dy + ch;
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (am[e] == mine) acc[e] += g[e];
      }
    float* o = dx + ip * ld_dx + ch;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    else o[0] = acc[0];
  }
}

// A quarter wave per input pixel (16 pixels per block); lane l takes the output channels 4 (l + 16 j) + e.
// wt is [kh][kw][cin][cout] (cout contiguous). For input pixel (y, x) the taps are ky = (y + pad) % stride +
// i stride < kh with oy = (y + pad - ky) / stride in [0, ho), kx likewise, visited in ascending (ky, kx); a lane
// adds its channels in ascending order and the 16 lanes are added by butterfly, so the order is fixed.
// z (optional): the conv's output after the ReLU; the gradient passes where z > 0.
// PREP: out channel ci < 3 = sum / scale_ci in T with pixel stride ld_dx; else cin fp32 / bf16 channels.
template <typename T, int CIN>
__global__ __launch_bounds__(256) void conv_dgrad_small_kernel(const float* __restrict__ dz, int ld_dz,
                                                               const float* __restrict__ z, int ld_z,
                                                               const float* __restrict__ wt, int h, int w, int cout,
                                                               int kh, int kw, int stride, int pad, int ho, int wo,
                                                               int prep, Affine3 af, T* __restrict__ dx, int ld_dx,
                                                               long npix) {
  const int l = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c4 = cout / 4;
  for (long base = blockIdx.x * 16L; base < npix; base += (long)gridDim.x * 16) {
    const long q = base + g;
    const bool in = q < npix;
    const long qq = in ? q : 0;
    const int x = (int)(qq % w);
    const long t = qq / w;
    const int y = (int)(t % h);
    const long img = t / h;
    float acc[CIN];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) acc[ci] = 0.f;
    if (in) {
      for (int ky = (y + pad) % stride; ky < kh && ky <= y + pad; ky += stride) {
        const int oy = (y + pad - ky) / stride;
        if (oy >= ho) continue;
        for (int kx = (x + pad) % stride; kx < kw && kx <= x + pad; kx += stride) {
          const int ox = (x + pad - kx) / stride;
          if (ox >= wo) continue;
          const long op = (img * ho + oy) * wo + ox;
          const float* pg = dz + op * ld_dz;
          const float* pz = z ? z + op * ld_z : nullptr;
          const float* pw = wt + (long)(ky * kw + kx) * CIN * cout;
          for (int j = l; j < c4; j += 16) {
            f32x4 gv = *reinterpret_cast<const f32x4*>(pg + j * 4);
            if (pz) {
              const f32x4 zv = *reinterpret_cast<const f32x4*>(pz + j * 4);
              gv.x = zv.x > 0.f ? gv.x : 0.f; gv.y = zv.y > 0.f ? gv.y : 0.f;
              gv.z = zv.z > 0.f ? gv.z : 0.f; gv.w = zv.w > 0.f ? gv.w : 0.f;
            }
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) {
              const f32x4 wv = *reinterpret_cast<const f32x4*>(pw + (long)ci * cout + j * 4);
              acc[ci] += gv.x * wv.x; acc[ci] += gv.y * wv.y; acc[ci] += gv.z * wv.z; acc[ci] += gv.w * wv.w;
            }
          }
        }
      }
    }
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) acc[ci] = row_sum(acc[ci]);
    if (in && l == 0) {
      T* o = dx + q * ld_dx;
      if (prep) {
#pragma unroll
        for (int ci = 0; ci < (CIN < 3 ? CIN : 3); ++ci) o[ci] = from_f32<T>(acc[ci] / af.scale[ci]);
      } else {
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) o[ci] = from_f32<T>(acc[ci]);
      }
    }
  }
}

template <typename T>
void launch_dgrad_small(int cin, dim3 grid, hipStream_t s, const float* dz, int ld_dz, const float* z, int ld_z,
                        const float* wt, int h, int w, int cout, int kh, int kw, int stride, int pad, int ho, int wo,
                        int prep, Affine3 af, T* dx, int ld_dx, long npix) {
#define RDEIC_DGS(C)                                                                                              \
  hipLaunchKernelGGL((conv_dgrad_small_kernel<T, C>), grid, dim3(256), 0, s, dz, ld_dz, z, ld_z, wt, h, w, cout, kh, \
                     kw, stride, pad, ho, wo, prep, af, dx, ld_dx, npix)
  switch (cin) {
    case 1: RDEIC_DGS(1); break;
    case 2: RDEIC_DGS(2); break;
    case 3: RDEIC_DGS(3); break;
    default: RDEIC_DGS(4); break;
  }
#undef RDEIC_DGS
}

constexpr Affine3 LPIPS_AFFINE = {{-0.030f, -0.088f, -0.188f}, {0.458f, 0.448f, 0.450f}};

}  // namespace

extern "C" int rdeic_lpips_prep(const uint8_t* img, int32_t n, int32_t h, int32_t w, float* out, void* stream) {
  if (!img || !out || n <= 0 || h <= 0 || w <= 0 || ((uintptr_t)out) % 16) return RDEIC_EINVAL;
  const long npix = (long)n * h * w;
  const Affine3 af = LPIPS_AFFINE;
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

extern "C" int rdeic_lpips_prep_float(const void* img, int32_t ld, int32_t dtype, int64_t npix, float* out,
                                      void* stream) {
  if (!img || !out || npix <= 0 || ld < 3 || dtype < 0 || dtype > 1 || ((uintptr_t)out) % 16) return RDEIC_EINVAL;
  const dim3 grid((unsigned)std::min<long>((npix + 255) / 256, 65536));
  if (dtype == 1)
    hipLaunchKernelGGL(lpips_prep_float_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)img, ld,
                       (long)npix, LPIPS_AFFINE, out);
  else
    hipLaunchKernelGGL(lpips_prep_float_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)img, ld,
                       (long)npix, LPIPS_AFFINE, out);
  return launch_status();
}

extern "C" int rdeic_lpips_layer_bwd(const float* f0, int32_t ld0, const float* f1, int32_t ld1, const float* lin,
                                     const float* gscore, int32_t n, int64_t hw, int32_t c, int32_t accumulate,
                                     float* df0, int32_t ldd, void* stream) {
  if (!f0 || !f1 || !lin || !gscore || !df0 || n <= 0 || hw <= 0 || c <= 0 || c % 64 || c > LD_MAXC || ld0 < c ||
      ld1 < c || ldd < c || n > 65535)
    return RDEIC_EINVAL;
  const long nblk = (hw + LD_PPB - 1) / LD_PPB;
  if (nblk > 0x7fffffffL) return RDEIC_EINVAL;
  const bool wide = ld0 % 4 == 0 && ld1 % 4 == 0 && ldd % 4 == 0 &&
                    !(((uintptr_t)f0 | (uintptr_t)f1 | (uintptr_t)lin | (uintptr_t)df0) & 15);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)nblk, n);
#define RDEIC_LDB(NJ) launch_layer_dist_bwd<NJ>(wide, grid, s, f0, ld0, f1, ld1, lin, gscore, hw, accumulate, df0, ldd)
  switch (c / 64) {
    case 1: RDEIC_LDB(1); break;
    case 2: RDEIC_LDB(2); break;
    case 3: RDEIC_LDB(3); break;
    case 4: RDEIC_LDB(4); break;
    case 5: RDEIC_LDB(5); break;
    case 6: RDEIC_LDB(6); break;
    case 7: RDEIC_LDB(7); break;
    default: RDEIC_LDB(8); break;
  }
#undef RDEIC_LDB
  return launch_status();
}

extern "C" int rdeic_maxpool2d_bwd(const float* in, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_in,
                                   const float* dy, int32_t ld_dy, int32_t k, int32_t s, float* dx, int32_t ld_dx,
                                   void* stream) {
  if (!in || !dy || !dx || n <= 0 || c <= 0 || k <= 0 || s <= 0 || h < k || w < k || ld_in < c || ld_dy < c ||
      ld_dx < c)
    return RDEIC_EINVAL;
  const int ho = (h - k) / s + 1, wo = (w - k) / s + 1;
  const bool v4 = c % 4 == 0 && ld_in % 4 == 0 && ld_dy % 4 == 0 && ld_dx % 4 == 0 &&
                  !(((uintptr_t)in | (uintptr_t)dy | (uintptr_t)dx) & 15);
  const long total = (long)n * h * w * (v4 ? c / 4 : c);
  const dim3 grid((unsigned)std::min<long>((total + 255) / 256, 1L << 20));
  if (v4)
    hipLaunchKernelGGL(maxpool_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, in, h, w, c, ld_in, dy, ld_dy, k,
                       s, ho, wo, dx, ld_dx, total);
  else
    hipLaunchKernelGGL(maxpool_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, in, h, w, c, ld_in, dy, ld_dy, k,
                       s, ho, wo, dx, ld_dx, total);
  return launch_status();
}

extern "C" int rdeic_conv_dgrad_small(const float* dz, int32_t ld_dz, const float* z, int32_t ld_z, const float* wt,
                                      int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t kh,
                                      int32_t kw, int32_t stride, int32_t pad, int32_t prep_bwd, void* dx,
                                      int32_t ld_dx, int32_t dx_dtype, void* stream) {
  if (!dz || !wt || !dx || n <= 0 || h <= 0 || w <= 0 || cin <= 0 || cin > 4 || cout <= 0 || cout % 4 || kh <= 0 ||
      kw <= 0 || stride <= 0 || pad < 0 || h + 2 * pad < kh || w + 2 * pad < kw || ld_dz < cout || ld_dz % 4 ||
      (z && (ld_z < cout || ld_z % 4)) || ld_dx < (prep_bwd ? std::min(cin, 3) : cin) || dx_dtype < 0 ||
      dx_dtype > 1 || (((uintptr_t)dz | (uintptr_t)z | (uintptr_t)wt) & 15))
    return RDEIC_EINVAL;
  const int ho = (h + 2 * pad - kh) / stride + 1, wo = (w + 2 * pad - kw) / stride + 1;
  const long npix = (long)n * h * w;
  const dim3 grid((unsigned)std::min<long>((npix + 15) / 16, 1L << 20));
  hipStream_t s = (hipStream_t)stream;
  if (dx_dtype == 1)
    launch_dgrad_small<bf16>(cin, grid, s, dz, ld_dz, z, ld_z, wt, h, w, cout, kh, kw, stride, pad, ho, wo, prep_bwd,
                             LPIPS_AFFINE, (bf16*)dx, ld_dx, npix);
  else
    launch_dgrad_small<float>(cin, grid, s, dz, ld_dz, z, ld_z, wt, h, w, cout, kh, kw, stride, pad, ho, wo, prep_bwd,
                              LPIPS_AFFINE, (float*)dx, ld_dx, npix);
  return launch_status();
}
