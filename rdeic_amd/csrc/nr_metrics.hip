// No-reference image quality on the device: the per-pixel passes and region reductions of NIQE
// (Mittal, Soundararajan, Bovik 2013) and BRISQUE (Mittal, Moorthy, Bovik 2012) on uint8 RGB
// reconstructions, as the reference's out-of-domain evaluation reports them (pyiqa "niqe" /
// "brisque", experiments/run_ood.py:93-127; pyiqa is not in this image, so the algorithms are
// restated from their published definitions with the conventions below — parity unpinned, see
// DESIGN.md §20). The host (rdeic_amd/metrics.py) fits the AGGD parameters from the moments.
//
// Per image and per scale s = 0, 1:
//   * Y = rint(255 * (0.299 R + 0.587 G + 0.114 B)), R, G, B in [0, 1] (rgb_to_y_kernel's expression),
//     of the top-left hc x wc crop (NIQE: multiples of 96; BRISQUE: the whole image);
//   * MSCN: mu = G * Y, sigma = sqrt(|G * Y^2 - mu^2|), M = (Y - mu) / (sigma + 1), G the 7x7
//     Gaussian (sigma 7/6, sum 1) applied separably with a replicate border, fp32, through LDS.
//     The tile filters Z = Y - Y(tile origin) instead of Y (integers: exact): mu_Z = mu - shift and
//     the variance is shift-invariant, so M is the same up to rounding, a constant image gives
//     M == 0 exactly, and flat regions lose no bits to the E[Y^2] - mu^2 cancellation;
//   * scale 1 runs on the half-size plane of the un-normalised Y: the antialiased bicubic (a = -0.5)
//     resize by exactly 1/2, the separable 8-tap filter [-3 -9 29 111 111 29 -9 -3] / 256 on inputs
//     2i-3 .. 2i+4, symmetric reflection at the border, vertical pass then horizontal, fp32;
//   * region moments: per region (96x96 / 48x48 blocks, or the whole plane) and per map — M and
//     M * roll(M, d) for d = (0,1), (1,0), (1,1), (1,-1), the roll circular WITHIN the region —
//     (n_neg, n_pos, sum x^2 | x<0, sum x^2 | x>0, sum |x|, sum x^2). A region is cut into row bands,
//     one workgroup each; a band writes fp32 partials and a finalize kernel adds the bands in order
//     in fp64. No atomics: bit-identical from run to run.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "../../include/rdeic_hip.h"

namespace {

constexpr int NR_R = 3, NR_W = 7;            // Gaussian radius, width
constexpr int NR_TW = 64, NR_TH = 16;        // MSCN outputs per block
constexpr int NR_IW = NR_TW + 2 * NR_R, NR_IH = NR_TH + 2 * NR_R;
constexpr int DS_TW = 64, DS_TH = 16;        // half-size outputs per block
constexpr int DS_IW = 2 * DS_TW + 6, DS_IH = 2 * DS_TH + 6;
constexpr int NR_MAPS = 5, NR_MOM = 6, NR_VALS = NR_MAPS * NR_MOM;
constexpr int NR_BAND_PIX = 4096;            // pixels per moment workgroup (whole rows of a region)

struct NrWin { float g[NR_W]; };

// Y of the top-left hc x wc crop of each RGB u8 image [n][h][w][3] -> y [n][hc][wc]
__global__ __launch_bounds__(256) void nr_luma_kernel(const uint8_t* __restrict__ rgb, int h, int w, int hc, int wc,
                                                      float* __restrict__ y) {
  const long img = blockIdx.y;
  const long npix = (long)hc * wc;
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const int r = (int)(p / wc), c = (int)(p - (long)r * wc);
    const uint8_t* px = rgb + ((img * h + r) * (long)w + c) * 3;
    const float l = (px[0] / 255.f) * 0.299f + (px[1] / 255.f) * 0.587f + (px[2] / 255.f) * 0.114f;
    y[img * npix + p] = rintf(l * 255.f);
  }
}

// grid (tiles_x, tiles_y, n): m [n][h][w] = MSCN of y [n][h][w]
__global__ __launch_bounds__(256) void nr_mscn_kernel(const float* __restrict__ y, int h, int w, NrWin win,
                                                      float* __restrict__ m) {
  __shared__ float sz[NR_IH][NR_IW];
  __shared__ float hq[2][NR_IH][NR_TW];  // horizontal passes of z, z^2
  const int x0 = blockIdx.x * NR_TW, y0 = blockIdx.y * NR_TH;
  const long img = blockIdx.z;
  const float* py = y + img * h * w;
  const int t = threadIdx.x;
  const float shift = py[(long)y0 * w + x0];  // the tile origin is always inside the plane
  for (int i = t; i < NR_IH * NR_IW; i += 256) {
    const int r = i / NR_IW, c = i - r * NR_IW;
    const int gy = min(max(y0 + r - NR_R, 0), h - 1), gx = min(max(x0 + c - NR_R, 0), w - 1);  // replicate
    sz[r][c] = py[(long)gy * w + gx] - shift;
  }
  __syncthreads();
  for (int i = t; i < NR_IH * NR_TW; i += 256) {
    const int r = i / NR_TW, c = i - r * NR_TW;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < NR_W; ++k) {
      const float g = win.g[k], v = sz[r][c + k];
      a = fmaf(g, v, a);
      b = fmaf(g, v * v, b);
    }
    hq[0][r][c] = a;
    hq[1][r][c] = b;
  }
  __syncthreads();
  for (int i = t; i < NR_TH * NR_TW; i += 256) {
    const int r = i / NR_TW, c = i - r * NR_TW;
    if (y0 + r >= h || x0 + c >= w) continue;
    float mu = 0.f, e2 = 0.f;
#pragma unroll
    for (int k = 0; k < NR_W; ++k) {
      const float g = win.g[k];
      mu = fmaf(g, hq[0][r + k][c], mu);
      e2 = fmaf(g, hq[1][r + k][c], e2);
    }
    const float sigma = sqrtf(fabsf(e2 - mu * mu));
    m[img * h * w + (long)(y0 + r) * w + (x0 + c)] = (sz[r + NR_R][c + NR_R] - mu) / (sigma + 1.f);
  }
}

__device__ __forceinline__ int reflect_sym(int i, int n) {
  i = i < 0 ? -i - 1 : i;
  i = i >= n ? 2 * n - 1 - i : i;
  return min(max(i, 0), n - 1);  // tiles past the plane's edge only (their outputs are not written)
}

// grid (tiles_x, tiles_y, n): out [n][h/2][w/2] = the 8-tap half-size plane of in [n][h][w] (h, w even)
__global__ __launch_bounds__(256) void nr_half_kernel(const float* __restrict__ in, int h, int w,
                                                      float* __restrict__ out) {
  __shared__ float si[DS_IH][DS_IW];
  __shared__ float sv[DS_TH][DS_IW];  // vertical pass
  const float tap[8] = {-3.f / 256.f, -9.f / 256.f, 29.f / 256.f, 111.f / 256.f,
                        111.f / 256.f, 29.f / 256.f, -9.f / 256.f, -3.f / 256.f};
  const int ho = h / 2, wo = w / 2;
  const int ox0 = blockIdx.x * DS_TW, oy0 = blockIdx.y * DS_TH;
  const long img = blockIdx.z;
  const float* pi = in + img * h * w;
  const int t = threadIdx.x;
  for (int i = t; i < DS_IH * DS_IW; i += 256) {
    const int r = i / DS_IW, c = i - r * DS_IW;
    const int gy = reflect_sym(2 * oy0 - 3 + r, h), gx = reflect_sym(2 * ox0 - 3 + c, w);
    si[r][c] = pi[(long)gy * w + gx];
  }
  __syncthreads();
  for (int i = t; i < DS_TH * DS_IW; i += 256) {
    const int r = i / DS_IW, c = i - r * DS_IW;
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) a = fmaf(tap[k], si[2 * r + k][c], a);
    sv[r][c] = a;
  }
  __syncthreads();
  for (int i = t; i < DS_TH * DS_TW; i += 256) {
    const int r = i / DS_TW, c = i - r * DS_TW;
    if (oy0 + r >= ho || ox0 + c >= wo) continue;
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) a = fmaf(tap[k], sv[r][2 * c + k], a);
    out[img * ho * wo + (long)(oy0 + r) * wo + (ox0 + c)] = a;
  }
}

__device__ __forceinline__ void nr_accum(float x, float* a) {
  const float sq = x * x;
  const bool neg = x < 0.f, pos = x > 0.f;
  a[0] += neg ? 1.f : 0.f;
  a[1] += pos ? 1.f : 0.f;
  a[2] += neg ? sq : 0.f;
  a[3] += pos ? sq : 0.f;
  a[4] += fabsf(x);
  a[5] += sq;
}

// grid (bands, regions, n); regions = (h / bh) * (w / bw) row-major. Band b covers rows [b * rb, min(bh, (b+1) rb))
// of its region. part [n][regions][bands][30].
__global__ __launch_bounds__(256) void nr_moments_kernel(const float* __restrict__ m, int h, int w, int bh, int bw,
                                                         int rb, float* __restrict__ part) {
  __shared__ float red[4][NR_VALS];
  const int band = blockIdx.x, region = blockIdx.y;
  const long img = blockIdx.z;
  const int rx = w / bw;
  const int by0 = (region / rx) * bh, bx0 = (region % rx) * bw;
  const float* pm = m + img * h * w + (long)by0 * w + bx0;  // region origin
  const int r0 = band * rb, rows = min(rb, bh - r0);
  const int t = threadIdx.x;
  float acc[NR_VALS];
#pragma unroll
  for (int k = 0; k < NR_VALS; ++k) acc[k] = 0.f;
  for (int i = t; i < rows * bw; i += 256) {
    const int yy = r0 + i / bw, xx = i % bw;
    const int yu = yy == 0 ? bh - 1 : yy - 1;       // (y - 1) mod bh
    const int xl = xx == 0 ? bw - 1 : xx - 1;       // (x - 1) mod bw
    const int xr = xx == bw - 1 ? 0 : xx + 1;       // (x + 1) mod bw
    const float v = pm[(long)yy * w + xx];
    nr_accum(v, acc);
    nr_accum(v * pm[(long)yy * w + xl], acc + 6);   // d = (0, 1)
    nr_accum(v * pm[(long)yu * w + xx], acc + 12);  // d = (1, 0)
    nr_accum(v * pm[(long)yu * w + xl], acc + 18);  // d = (1, 1)
    nr_accum(v * pm[(long)yu * w + xr], acc + 24);  // d = (1, -1)
  }
  // fixed-order block reduction: lanes (butterfly), then the 4 waves in order
#pragma unroll
  for (int k = 0; k < NR_VALS; ++k) {
    const float s = warp_sum(acc[k]);
    if ((t & 63) == 0) red[t >> 6][k] = s;
  }
  __syncthreads();
  if (t < NR_VALS) {
    const long slot = (img * gridDim.y + region) * gridDim.x + band;
    part[slot * NR_VALS + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
  }
}

// one thread per (image, region, value): the bands in order, fp64
__global__ __launch_bounds__(256) void nr_finalize_kernel(const float* __restrict__ part, long count, int bands,
                                                          double* __restrict__ out) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= count) return;
  const long reg = i / NR_VALS;
  const int k = (int)(i - reg * NR_VALS);
  double s = 0.0;
  for (int b = 0; b < bands; ++b) s += (double)part[(reg * bands + b) * NR_VALS + k];
  out[i] = s;
}

NrWin nr_window() {
  NrWin w;
  double g[NR_W], sum = 0.0;
  const double sg = 7.0 / 6.0;
  for (int i = 0; i < NR_W; ++i) {
    const double d = i - NR_R;
    g[i] = std::exp(-d * d / (2.0 * sg * sg));
    sum += g[i];
  }
  for (int i = 0; i < NR_W; ++i) w.g[i] = (float)(g[i] / sum);
  return w;
}

struct NrGeom {
  int hc, wc, bh, bw;  // crop, scale-0 region
  int regions;
  int rb0, bands0, rb1, bands1;
  size_t plane, part;  // floats per image plane at scale 0; partial floats
};

int band_rows(int bh, int bw) { return std::max(1, std::min(bh, NR_BAND_PIX / bw)); }

bool nr_geom(int n, int h, int w, int block, NrGeom* g) {
  if (n <= 0 || h <= 0 || w <= 0 || (block != 0 && block != 96)) return false;
  if (block) {
    g->hc = h / block * block;
    g->wc = w / block * block;
    g->bh = g->bw = block;
    if (g->hc == 0 || g->wc == 0) return false;
  } else {
    if (h % 2 || w % 2 || h < 8 || w < 8) return false;
    g->hc = g->bh = h;
    g->wc = g->bw = w;
  }
  g->regions = (g->hc / g->bh) * (g->wc / g->bw);
  g->rb0 = band_rows(g->bh, g->bw);
  g->bands0 = cdiv(g->bh, g->rb0);
  g->rb1 = band_rows(g->bh / 2, g->bw / 2);
  g->bands1 = cdiv(g->bh / 2, g->rb1);
  g->plane = (size_t)g->hc * g->wc;
  g->part = (size_t)n * g->regions * std::max(g->bands0, g->bands1) * NR_VALS;
  return true;
}

}  // namespace

extern "C" size_t rdeic_nr_moments_ws_floats(int32_t n, int32_t h, int32_t w, int32_t block) {
  NrGeom g;
  if (!nr_geom(n, h, w, block, &g)) return 0;
  return (size_t)n * g.plane * 2 + (size_t)n * (g.plane / 4) * 2 + g.part;
}

extern "C" int rdeic_nr_moments(const uint8_t* rgb, int32_t n, int32_t h, int32_t w, int32_t block, float* ws,
                                size_t ws_floats, double* out_scale0, double* out_scale1, void* stream) {
  NrGeom g;
  if (!rgb || !ws || !out_scale0 || !out_scale1 || !nr_geom(n, h, w, block, &g)) return RDEIC_EINVAL;
  if (n > 65535 || g.regions > 65535) return RDEIC_EINVAL;
  if (ws_floats < rdeic_nr_moments_ws_floats(n, h, w, block)) return RDEIC_ENOSPC;
  hipStream_t s = (hipStream_t)stream;
  const NrWin win = nr_window();
  float* y0 = ws;
  float* m0 = y0 + (size_t)n * g.plane;
  float* y1 = m0 + (size_t)n * g.plane;
  float* m1 = y1 + (size_t)n * (g.plane / 4);
  float* part = m1 + (size_t)n * (g.plane / 4);
  const int h1 = g.hc / 2, w1 = g.wc / 2;
  hipLaunchKernelGGL(nr_luma_kernel, dim3((unsigned)std::min<long>(((long)g.plane + 255) / 256, 1024), n), dim3(256),
                     0, s, rgb, h, w, g.hc, g.wc, y0);
  hipLaunchKernelGGL(nr_mscn_kernel, dim3(cdiv(g.wc, NR_TW), cdiv(g.hc, NR_TH), n), dim3(256), 0, s, y0, g.hc, g.wc,
                     win, m0);
  hipLaunchKernelGGL(nr_half_kernel, dim3(cdiv(w1, DS_TW), cdiv(h1, DS_TH), n), dim3(256), 0, s, y0, g.hc, g.wc, y1);
  const long count = (long)n * g.regions * NR_VALS;
  hipLaunchKernelGGL(nr_moments_kernel, dim3(g.bands0, g.regions, n), dim3(256), 0, s, m0, g.hc, g.wc, g.bh, g.bw,
                     g.rb0, part);
  hipLaunchKernelGGL(nr_finalize_kernel, dim3(cdiv(count, 256)), dim3(256), 0, s, part, count, g.bands0, out_scale0);
  hipLaunchKernelGGL(nr_mscn_kernel, dim3(cdiv(w1, NR_TW), cdiv(h1, NR_TH), n), dim3(256), 0, s, y1, h1, w1, win, m1);
  hipLaunchKernelGGL(nr_moments_kernel, dim3(g.bands1, g.regions, n), dim3(256), 0, s, m1, h1, w1, g.bh / 2, g.bw / 2,
                     g.rb1, part);
  hipLaunchKernelGGL(nr_finalize_kernel, dim3(cdiv(count, 256)), dim3(256), 0, s, part, count, g.bands1, out_scale1);
  return launch_status();
}
