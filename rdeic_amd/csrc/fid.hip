// FID / KID on the device: the kernels around the fp32 InceptionV3 convs (the layer table, the weights, the
// chunking and the host-side scores live in rdeic_amd/fid.py; the convs run on the library's fp32 route).
//
//   * prep: uint8 RGB [n][h][w][3] -> fp32 [n][oh][ow][4]: v / 255, bilinear resize (align_corners = false, no
//     antialiasing), then 2 v - 1; channel 3 is zero, so conv 0 takes the 16-byte gather. Per axis, in fp32 and in
//     this order (this TU is built with -ffp-contract=off; the scale in / out is divided once on the host):
//         s = max((d + 0.5) * scale - 0.5, 0),  i0 = floor(s),  i1 = min(i0 + 1, in - 1),  t = s - i0,
//         row = (1 - tx) * v[i0] + tx * v[i1],  out = (1 - ty) * row0 + ty * row1.
//     With in == out, s == d and t == 0 exactly, so the pixel comes out as (v / 255) * 2 - 1 bit for bit;
//   * pool2d: window k, stride s, symmetric padding p, floor mode, max (padding counts as -inf: a tap outside the
//     map is skipped) or average over the in-bounds taps (count_include_pad = false). Taps in row-major order;
//   * global average pool: [n][hw][c] -> [n][c]. A thread adds its pixels in index order in fp64; the GAP_L pixel
//     lanes of a channel are then added in lane order, the mean is divided in fp64 and rounded to fp32 once;
//   * feature moments: sum[c] and outer[c][c] = sum_k x_k x_k^T of [rows][c] features in fp64. An fp32 x fp32
//     product is exact in fp64 and the rows are added in index order, so every element is one fixed-order sum.
//     64 x 64 output tiles of the upper triangle, a panel of MOM_KP rows of both column blocks in LDS, a 4 x 4
//     register tile per thread; an off-diagonal tile is stored twice (outer[i][j] and outer[j][i] from one
//     register), a diagonal tile computes x_ki * x_kj and x_kj * x_ki in the same row order: the same bits.
//
// Every offset is 64-bit; no kernel uses an atomic; no result depends on the batch it was computed in.
#include <algorithm>
#include <math.h>

#include "common.h"
#include "../../include/rdeic_hip.h"

namespace {

// ---------------------------------------------------------------- prep
struct Src { int i0, i1; float t; };

__device__ __forceinline__ Src src_index(int d, float scale, int in) {
  float s = ((float)d + 0.5f) * scale - 0.5f;
  s = s < 0.f ? 0.f : s;
  Src r;
  r.i0 = (int)floorf(s);
  if (r.i0 > in - 1) r.i0 = in - 1;  // (never: s < in - 0.5 for out >= 1; keeps the gather in bounds regardless)
  r.i1 = r.i0 + 1 < in ? r.i0 + 1 : in - 1;
  r.t = s - (float)r.i0;
  return r;
}

__global__ __launch_bounds__(256) void fid_prep_kernel(const uint8_t* __restrict__ img, int h, int w, int oh, int ow,
                                                       float sy, float sx, long total, float* __restrict__ out) {
  for (long p = blockIdx.x * 256L + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
    const int ox = (int)(p % ow);
    const long t = p / ow;
    const int oy = (int)(t % oh);
    const long n = t / oh;
    const Src y = src_index(oy, sy, h), x = src_index(ox, sx, w);
    const uint8_t* b = img + n * h * w * 3;
    const uint8_t* p00 = b + ((long)y.i0 * w + x.i0) * 3;
    const uint8_t* p01 = b + ((long)y.i0 * w + x.i1) * 3;
    const uint8_t* p10 = b + ((long)y.i1 * w + x.i0) * 3;
    const uint8_t* p11 = b + ((long)y.i1 * w + x.i1) * 3;
    const float ux = 1.f - x.t, uy = 1.f - y.t;
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v00 = (float)p00[c] / 255.f, v01 = (float)p01[c] / 255.f;
      const float v10 = (float)p10[c] / 255.f, v11 = (float)p11[c] / 255.f;
      const float r0 = ux * v00 + x.t * v01;
      const float r1 = ux * v10 + x.t * v11;
      const float v = uy * r0 + y.t * r1;
      r[c] = v * 2.f - 1.f;
    }
    *reinterpret_cast<f32x4*>(out + p * 4) = f32x4{r[0], r[1], r[2], 0.f};
  }
}

// ---------------------------------------------------------------- pool2d
// one thread per V channels of one output pixel; V = 4 needs c, both ld % 4 == 0 and 16-byte bases
template <int V, bool AVG>
__global__ __launch_bounds__(256) void pool2d_kernel(const float* __restrict__ in, int h, int w, int c, int ld_in,
                                                     int k, int s, int p, int ho, int wo, float* __restrict__ out,
                                                     int ld_out, long total) {
  const int cv = c / V;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ch = (int)(i % cv) * V;
    const long op = i / cv;  // output pixel over the batch
    const int ox = (int)(op % wo);
    const long t = op / wo;
    const int oy = (int)(t % ho);
    const long img = t / ho;
    float m[V];
#pragma unroll
    for (int e = 0; e < V; ++e) m[e] = AVG ? 0.f : -INFINITY;
    int taps = 0;
    for (int dy = 0; dy < k; ++dy) {
      const int iy = oy * s - p + dy;
      if (iy < 0 || iy >= h) continue;
      for (int dx = 0; dx < k; ++dx) {
        const int ix = ox * s - p + dx;
        if (ix < 0 || ix >= w) continue;
        ++taps;
        const float* q = in + ((img * h + iy) * w + ix) * ld_in + ch;
        if constexpr (V == 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(q);
          if constexpr (AVG) {
            m[0] += v.x; m[1] += v.y; m[2] += v.z; m[3] += v.w;
          } else {
            m[0] = pool_max(m[0], v.x); m[1] = pool_max(m[1], v.y);
            m[2] = pool_max(m[2], v.z); m[3] = pool_max(m[3], v.w);
          }
        } else {
          if constexpr (AVG) m[0] += q[0];
          else m[0] = pool_max(m[0], q[0]);
        }
      }
    }
    if constexpr (AVG) {
      const float div = (float)taps;  // >= 1: 2 p <= k, so every window holds an in-bounds tap
#pragma unroll
      for (int e = 0; e < V; ++e) m[e] = m[e] / div;
    }
    float* o = out + op * ld_out + ch;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(o) = f32x4{m[0], m[1], m[2], m[3]};
    else o[0] = m[0];
  }
}

// ---------------------------------------------------------------- global average pool
constexpr int GAP_TX = 64;  // channel groups (of 4) across a block
constexpr int GAP_L = 4;    // pixel lanes: lane l adds the pixels l, l + GAP_L, ... in order

// grid (channel blocks, n), 256 threads = GAP_L pixel lanes (one wave each) by GAP_TX channel groups
template <bool WIDE>
__global__ __launch_bounds__(256) void global_avgpool_kernel(const float* __restrict__ x, int ld, long hw, int c,
                                                             float* __restrict__ out) {
  __shared__ double sm[GAP_L][GAP_TX][4];
  const int cx = threadIdx.x % GAP_TX, l = threadIdx.x / GAP_TX;
  const long img = blockIdx.y;
  const int ch = (blockIdx.x * GAP_TX + cx) * 4;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if (ch < c) {
    const float* b = x + img * hw * ld + ch;
    for (long p = l; p < hw; p += GAP_L) {
      const f32x4 v = ld4<WIDE>(b + p * ld, c, ch);
      s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z; s[3] += (double)v.w;
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) sm[l][cx][e] = s[e];
  __syncthreads();
  if (l != 0 || ch >= c) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    double v = sm[0][cx][e];
    for (int j = 1; j < GAP_L; ++j) v += sm[j][cx][e];
    if (ch + e < c) out[img * c + ch + e] = (float)(v / (double)hw);
  }
}

// ---------------------------------------------------------------- feature moments
constexpr int MOM_T = 64;   // output tile edge
constexpr int MOM_KP = 32;  // rows per LDS panel

// sum[ch] (+)= sum_k x[k][ch], rows in index order; one thread per channel
__global__ __launch_bounds__(256) void feat_sum_kernel(const float* __restrict__ x, long rows, int c, int ld,
                                                       int accumulate, double* __restrict__ sum) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  double s = 0.0;
  for (long k = 0; k < rows; ++k) s += (double)x[k * ld + ch];
  sum[ch] = accumulate ? sum[ch] + s : s;
}

// grid (tiles, tiles); block (bi, bj) with bi <= bj owns outer[bi * 64 ..][bj * 64 ..] and its mirror.
// Thread (ty, tx) = (tid / 16, tid % 16) holds rows ty * 4 .. + 3 by columns tx * 4 .. + 3 of the tile.
__global__ __launch_bounds__(256) void feat_outer_kernel(const float* __restrict__ x, long rows, int c, int ld,
                                                         int accumulate, double* __restrict__ outer) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ f32x4 As[MOM_KP][MOM_T / 4], Bs[MOM_KP][MOM_T / 4];
  const int tid = threadIdx.x, tx = tid % 16, ty = tid / 16;
  const int i0 = blockIdx.x * MOM_T, j0 = blockIdx.y * MOM_T;
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  for (long k0 = 0; k0 < rows; k0 += MOM_KP) {
    const int kn = rows - k0 < MOM_KP ? (int)(rows - k0) : MOM_KP;
    // stage: MOM_KP rows x 16 float4 of each column block, zeros past the rows / past c (c % 4 == 0)
#pragma unroll
    for (int r = 0; r < MOM_KP * (MOM_T / 4) / 256; ++r) {
      const int idx = tid + 256 * r;
      const int kr = idx / (MOM_T / 4), q = idx % (MOM_T / 4);
      f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
      if (kr < kn) {
        const float* row = x + (k0 + kr) * ld;
        if (i0 + q * 4 < c) va = *reinterpret_cast<const f32x4*>(row + i0 + q * 4);
        if (j0 + q * 4 < c) vb = *reinterpret_cast<const f32x4*>(row + j0 + q * 4);
      }
      As[kr][q] = va;
      Bs[kr][q] = vb;
    }
    __syncthreads();
    for (int k = 0; k < kn; ++k) {
      const f32x4 a = As[k][ty], b = Bs[k][tx];
      const double ad[4] = {(double)a.x, (double)a.y, (double)a.z, (double)a.w};
      const double bd[4] = {(double)b.x, (double)b.y, (double)b.z, (double)b.w};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] += ad[u] * bd[v];
    }
    __syncthreads();
  }
  const bool diag = blockIdx.x == blockIdx.y;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + ty * 4 + u;
    if (i >= c) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + tx * 4 + v;
      if (j >= c) continue;
      double* o = outer + (long)i * c + j;
      const double r = accumulate ? *o + acc[u][v] : acc[u][v];
      *o = r;
      if (!diag) outer[(long)j * c + i] = r;  // the mirror held the same bits before: the same bits after
    }
  }
}

}  // namespace

extern "C" int rdeic_fid_prep(const uint8_t* img, int32_t n, int32_t h, int32_t w, int32_t oh, int32_t ow, float* out,
                              void* stream) {
  if (!img || !out || n <= 0 || h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || ((uintptr_t)out & 15)) return RDEIC_EINVAL;
  const long total = (long)n * oh * ow;
  const float sy = (float)h / (float)oh, sx = (float)w / (float)ow;
  hipLaunchKernelGGL(fid_prep_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 65536)), dim3(256), 0,
                     (hipStream_t)stream, img, h, w, oh, ow, sy, sx, total, out);
  return launch_status();
}

extern "C" int rdeic_pool2d(const float* in, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_in, int32_t k,
                            int32_t s, int32_t p, int32_t mode, float* out, int32_t ld_out, void* stream) {
  if (!in || !out || n <= 0 || h <= 0 || w <= 0 || c <= 0 || k <= 0 || s <= 0 || p < 0 || 2 * p > k ||
      h + 2 * p < k || w + 2 * p < k || ld_in < c || ld_out < c || (mode != RDEIC_POOL_MAX && mode != RDEIC_POOL_AVG))
    return RDEIC_EINVAL;
  const int ho = (h + 2 * p - k) / s + 1, wo = (w + 2 * p - k) / s + 1;
  const bool v4 = c % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && !(((uintptr_t)in | (uintptr_t)out) & 15);
  const long total = (long)n * ho * wo * (v4 ? c / 4 : c);
  const dim3 grid((unsigned)std::min<long>((total + 255) / 256, 1L << 20));
  hipStream_t st = (hipStream_t)stream;
  if (mode == RDEIC_POOL_MAX) {
    if (v4)
      hipLaunchKernelGGL((pool2d_kernel<4, false>), grid, dim3(256), 0, st, in, h, w, c, ld_in, k, s, p, ho, wo, out,
                         ld_out, total);
    else
      hipLaunchKernelGGL((pool2d_kernel<1, false>), grid, dim3(256), 0, st, in, h, w, c, ld_in, k, s, p, ho, wo, out,
                         ld_out, total);
  } else {
    if (v4)
      hipLaunchKernelGGL((pool2d_kernel<4, true>), grid, dim3(256), 0, st, in, h, w, c, ld_in, k, s, p, ho, wo, out,
                         ld_out, total);
    else
      hipLaunchKernelGGL((pool2d_kernel<1, true>), grid, dim3(256), 0, st, in, h, w, c, ld_in, k, s, p, ho, wo, out,
                         ld_out, total);
  }
  return launch_status();
}

extern "C" int rdeic_global_avgpool(const float* x, int32_t ld, int32_t n, int64_t hw, int32_t c, float* out,
                                    void* stream) {
  if (!x || !out || n <= 0 || n > 65535 || hw <= 0 || c <= 0 || ld < c) return RDEIC_EINVAL;
  const int cgroups = (c + 3) / 4;
  const dim3 grid((unsigned)((cgroups + GAP_TX - 1) / GAP_TX), n);
  const bool wide = c % 4 == 0 && ld % 4 == 0 && !((uintptr_t)x & 15);
  if (wide)
    hipLaunchKernelGGL(global_avgpool_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, ld, (long)hw, c, out);
  else
    hipLaunchKernelGGL(global_avgpool_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, ld, (long)hw, c, out);
  return launch_status();
}

extern "C" int rdeic_feat_moments(const float* x, int64_t rows, int32_t c, int32_t ld, int32_t accumulate,
                                  double* sum, double* outer, void* stream) {
  if (!x || !sum || !outer || rows <= 0 || c <= 0 || c > 2048 || c % 4 || ld < c || ld % 4 || ((uintptr_t)x & 15))
    return RDEIC_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(feat_sum_kernel, dim3((c + 255) / 256), dim3(256), 0, st, x, (long)rows, c, ld, accumulate, sum);
  const int tiles = (c + MOM_T - 1) / MOM_T;
  hipLaunchKernelGGL(feat_outer_kernel, dim3(tiles, tiles), dim3(256), 0, st, x, (long)rows, c, ld, accumulate, outer);
  return launch_status();
}
