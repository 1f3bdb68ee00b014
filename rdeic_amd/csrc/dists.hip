// DISTS (Ding et al. 2020) on the device: the kernels around the fp32 VGG16 backbone convs (the network table,
// the weights and the chunking live in rdeic_amd/dists.py; the backbone is the one LPIPS("vgg") runs).
//
//   * prep: uint8 RGB [n][h][w][3] -> two fp32 NHWC [n][h][w][4] tensors in one pass: the raw v / 255 (tap 0)
//     and the normalised (v / 255 - mean_c) / std_c, evaluated in that order in fp32 (this TU is built with
//     -ffp-contract=off). Channel 3 of both is zero, so conv 0 takes the 16-byte gather;
//   * L2 pool: out = sqrt(depthwise_conv(x * x, g, stride 2, zero padding 1) + 1e-12), g = [[1,2,1],[2,4,2],
//     [1,2,1]] / 16, output size ceil(h / 2) x ceil(w / 2). The border is handled by bounds: a tap outside the
//     map adds nothing. The weights are powers of two, so x * x carries the only rounding of a term;
//   * moments: for two maps [n][hw][c] the per-image, per-channel mx, my, vx, vy, cxy (biased) in fp64, in two
//     passes. Pass 1 sums x and y; the finalize gives the fp64 means and their fp32 roundings kx, ky. Pass 2
//     sums (x - kx)^2, (y - ky)^2 and (x - kx)(y - ky), and the finalize removes the shift:
//         vx = S_xx / hw - (mx - kx)^2,  cxy = S_xy / hw - (mx - kx)(my - ky).
//     The shift is within half an ulp of the mean, so nothing cancels (the raw form sum x^2 - (sum x)^2 / hw
//     loses everything for a feature with a large mean and a small spread). The three second moments go
//     through one code path: two identical maps give vx == vy == cxy bit for bit.
//     A thread adds MOM_RUN products in fp32 before it folds them into its fp64 sums; everything across
//     threads, waves and blocks is fp64 in a fixed order (the finalizes add a channel's block partials over
//     16 chunk lanes, then the lanes in order). No atomics. An image's partial grid is a function of (hw, c)
//     alone, so its moments do not depend on the batch and repeat bit for bit;
//   * score: per image sum_c alpha_c S1_c + beta_c S2_c of one tap in fp64, fixed order,
//         S1 = (2 mx my + c1) / (mx^2 + my^2 + c1),  S2 = (2 cxy + c2) / (vx + vy + c2),  c1 = c2 = 1e-6.
//
// Every offset is 64-bit.
#include <algorithm>

#include "common.h"
#include "../../include/rdeic_hip.h"

namespace {

constexpr int MOM_RUN = 8;    // fp32 terms a thread adds before folding into fp64
constexpr int MOM_RUNS = 4;   // runs per thread: MOM_RUN * MOM_RUNS pixels per thread row
constexpr int MOM_MAXTX = 64;  // channel groups (of 4) across a block, at most one wave's width

struct Affine3 { float mean[3], std[3]; };
constexpr Affine3 DISTS_AFFINE = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};

__global__ __launch_bounds__(256) void dists_prep_kernel(const uint8_t* __restrict__ img, long npix, Affine3 af,
                                                         float* __restrict__ raw, float* __restrict__ norm) {
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const uint8_t* s = img + p * 3;
    f32x4 r, v;
    r.x = (float)s[0] / 255.f;
    r.y = (float)s[1] / 255.f;
    r.z = (float)s[2] / 255.f;
    r.w = 0.f;
    v.x = (r.x - af.mean[0]) / af.std[0];
    v.y = (r.y - af.mean[1]) / af.std[1];
    v.z = (r.z - af.mean[2]) / af.std[2];
    v.w = 0.f;
    *reinterpret_cast<f32x4*>(raw + p * 4) = r;
    *reinterpret_cast<f32x4*>(norm + p * 4) = v;
  }
}

// one thread per V channels of one output pixel; V = 4 needs c, both ld % 4 == 0 and 16-byte bases.
// Taps in row-major order; a tap outside the map is skipped (zero padding).
template <int V>
__global__ __launch_bounds__(256) void l2pool_kernel(const float* __restrict__ in, int h, int w, int c, int ld_in,
                                                     int ho, int wo, float* __restrict__ out, int ld_out,
                                                     long total) {
  const int cv = c / V;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ch = (int)(i % cv) * V;
    const long op = i / cv;  // output pixel over the batch
    const int ox = (int)(op % wo);
    const long t = op / wo;
    const int oy = (int)(t % ho);
    const long img = t / ho;
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = 2 * oy - 1 + dy;
      if (iy < 0 || iy >= h) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int ix = 2 * ox - 1 + dx;
        if (ix < 0 || ix >= w) continue;
        const float g = (dy == 1 ? 2.f : 1.f) * (dx == 1 ? 2.f : 1.f) * 0.0625f;
        const float* q = in + ((img * h + iy) * w + ix) * ld_in + ch;
        if constexpr (V == 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(q);
          acc[0] += g * (v.x * v.x); acc[1] += g * (v.y * v.y);
          acc[2] += g * (v.z * v.z); acc[3] += g * (v.w * v.w);
        } else {
          acc[0] += g * (q[0] * q[0]);
        }
      }
    }
    float* o = out + op * ld_out + ch;
    if constexpr (V == 4)
      *reinterpret_cast<f32x4*>(o) = f32x4{sqrtf(acc[0] + 1e-12f), sqrtf(acc[1] + 1e-12f), sqrtf(acc[2] + 1e-12f),
                                           sqrtf(acc[3] + 1e-12f)};
    else
      o[0] = sqrtf(acc[0] + 1e-12f);
  }
}

// The block geometry of the moment passes, a function of c alone: tx channel groups of 4 (a power of two, at
// most 64) by ty = 256 / tx pixel rows; a block covers ty * MOM_RUN * MOM_RUNS pixels of one image.
struct MomGeom { int tx, ty, cgroups, cblocks; long ppb, nchunk; };

MomGeom mom_geom(long hw, int c) {
  MomGeom g;
  g.cgroups = (c + 3) / 4;
  g.tx = 1;
  while (g.tx < g.cgroups && g.tx < MOM_MAXTX) g.tx *= 2;
  g.ty = 256 / g.tx;
  g.cblocks = (g.cgroups + g.tx - 1) / g.tx;
  g.ppb = (long)g.ty * MOM_RUN * MOM_RUNS;
  g.nchunk = (hw + g.ppb - 1) / g.ppb;
  return g;
}

// Adds the Q x 4 fp64 sums of the block's threads that share a channel group, in a fixed order: the butterfly
// over the pixel rows inside a wave (lanes tx apart), then the four waves in order. Returns true for the
// threads (wave 0, lane < tx) that hold the result.
template <int Q>
__device__ __forceinline__ bool mom_block_sum(double (&s)[Q][4], int tx, double* sm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e)
      for (int o = 32; o >= tx; o >>= 1) s[q][e] += __shfl_xor(s[q][e], o, 64);
  if (lane < tx) {
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) sm[((wave * MOM_MAXTX + lane) * Q + q) * 4 + e] = s[q][e];
  }
  __syncthreads();
  const bool owner = wave == 0 && lane < tx;
  if (owner) {
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double v = sm[((0 * MOM_MAXTX + lane) * Q + q) * 4 + e];
        for (int wv = 1; wv < 4; ++wv) v += sm[((wv * MOM_MAXTX + lane) * Q + q) * 4 + e];
        s[q][e] = v;
      }
  }
  return owner;
}

// grid (pixel chunks, channel blocks, n). tx == 64: every wave is one pixel row and the in-wave butterfly is
// empty; tx < 64: a wave holds 64 / tx rows. Thread (cx, py) takes the pixels p0 + py + ty * r, r < RUN * RUNS.
// PASS 1: part1[img][chunk][2][c] = sum x, sum y. PASS 2: part2[img][chunk][3][c] = the shifted second moments,
// shift[img][2][c] (fp64 holding fp32 values) the shifts.
template <int PASS, bool WIDE>
__global__ __launch_bounds__(256) void dists_moments_kernel(const float* __restrict__ x, int ldx,
                                                            const float* __restrict__ y, int ldy, long hw, int c,
                                                            int tx, const double* __restrict__ shift,
                                                            double* __restrict__ part) {
  constexpr int Q = PASS == 1 ? 2 : 3;
  __shared__ double sm[4 * MOM_MAXTX * Q * 4];
  const int ty = 256 / tx;
  const int cx = threadIdx.x & (tx - 1), py = threadIdx.x / tx;
  const long img = blockIdx.z;
  const int cg = blockIdx.y * tx + cx;
  const int ch = cg * 4;
  const bool live = ch < c;
  const long p0 = (long)blockIdx.x * ty * (MOM_RUN * MOM_RUNS);
  double s[Q][4];
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) s[q][e] = 0.0;
  f32x4 kx = {0.f, 0.f, 0.f, 0.f}, ky = {0.f, 0.f, 0.f, 0.f};
  if (PASS == 2 && live) {
    const double* sh = shift + img * 2 * c;
    float k0[4], k1[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      k0[e] = ch + e < c ? (float)sh[ch + e] : 0.f;
      k1[e] = ch + e < c ? (float)sh[c + ch + e] : 0.f;
    }
    kx = f32x4{k0[0], k0[1], k0[2], k0[3]};
    ky = f32x4{k1[0], k1[1], k1[2], k1[3]};
  }
  if (live) {
    const float* bx = x + img * hw * ldx + ch;
    const float* by = y + img * hw * ldy + ch;
#pragma unroll 1  // 2 * MOM_RUN float4 loads in flight per thread are enough; more only costs occupancy
    for (int run = 0; run < MOM_RUNS; ++run) {
      f32x4 a[MOM_RUN], b[MOM_RUN];
      bool in[MOM_RUN];
#pragma unroll
      for (int r = 0; r < MOM_RUN; ++r) {
        const long p = p0 + py + (long)ty * (run * MOM_RUN + r);
        in[r] = p < hw;
        const long pp = in[r] ? p : 0;
        a[r] = ld4<WIDE>(bx + pp * ldx, c, ch);
        b[r] = ld4<WIDE>(by + pp * ldy, c, ch);
      }
      f32x4 f[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) f[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < MOM_RUN; ++r) {
        if (!in[r]) continue;
        if constexpr (PASS == 1) {
          f[0] += a[r];
          f[1] += b[r];
        } else {
          const f32x4 da = a[r] - kx, db = b[r] - ky;
          f[0] += da * da;
          f[1] += db * db;
          f[2] += da * db;
        }
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        s[q][0] += (double)f[q].x; s[q][1] += (double)f[q].y; s[q][2] += (double)f[q].z; s[q][3] += (double)f[q].w;
      }
    }
  }
  const bool owner = mom_block_sum<Q>(s, tx, sm);
  if (owner && live) {
    double* o = part + ((img * gridDim.x + blockIdx.x) * Q) * c;
#pragma unroll
    for (int q = 0; q < Q; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ch + e < c) o[(long)q * c + ch + e] = s[q][e];
  }
}

// The finalizes: grid (channel blocks of FIN_C, n), 256 threads = FIN_K chunk lanes by FIN_C channels. Lane kl adds
// the chunks kl, kl + FIN_K, ... of its channel in order in fp64 (one thread per channel over hundreds of chunks
// is a chain of dependent loads as long as a pass itself); the FIN_K lane sums are then added in lane order. The
// order is a function of the chunk count alone.
constexpr int FIN_C = 16, FIN_K = 16;

template <int Q>
__device__ __forceinline__ bool fin_chunk_sum(const double* __restrict__ part, long nchunk, int c, int ch,
                                              double (&s)[Q], double* sm) {
  const int cl = threadIdx.x % FIN_C, kl = threadIdx.x / FIN_C;
#pragma unroll
  for (int q = 0; q < Q; ++q) s[q] = 0.0;
  if (ch < c) {
#pragma unroll 4
    for (long k = kl; k < nchunk; k += FIN_K) {
#pragma unroll
      for (int q = 0; q < Q; ++q) s[q] += part[(k * Q + q) * c + ch];
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) sm[(kl * FIN_C + cl) * Q + q] = s[q];
  __syncthreads();
  if (kl != 0 || ch >= c) return false;
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    double v = sm[cl * Q + q];
    for (int j = 1; j < FIN_K; ++j) v += sm[(j * FIN_C + cl) * Q + q];
    s[q] = v;
  }
  return true;
}

// mean[img][2][c] = the fp64 means, shift[img][2][c] = their fp32 roundings
__global__ __launch_bounds__(256) void dists_mean_finalize_kernel(const double* __restrict__ part, long nchunk, int c,
                                                                  double hw, double* __restrict__ mean,
                                                                  double* __restrict__ shift) {
  __shared__ double sm[FIN_K * FIN_C * 2];
  const long img = blockIdx.y;
  const int ch = blockIdx.x * FIN_C + threadIdx.x % FIN_C;
  double s[2];
  if (!fin_chunk_sum<2>(part + img * nchunk * 2 * c, nchunk, c, ch, s, sm)) return;
  const double mx = s[0] / hw, my = s[1] / hw;
  mean[img * 2 * c + ch] = mx;
  mean[img * 2 * c + c + ch] = my;
  shift[img * 2 * c + ch] = (double)(float)mx;
  shift[img * 2 * c + c + ch] = (double)(float)my;
}

// out[img][5][c] = mx, my, vx, vy, cxy
__global__ __launch_bounds__(256) void dists_moment_finalize_kernel(const double* __restrict__ part, long nchunk,
                                                                    int c, double hw, const double* __restrict__ mean,
                                                                    const double* __restrict__ shift,
                                                                    double* __restrict__ out) {
  __shared__ double sm[FIN_K * FIN_C * 3];
  const long img = blockIdx.y;
  const int ch = blockIdx.x * FIN_C + threadIdx.x % FIN_C;
  double s[3];
  if (!fin_chunk_sum<3>(part + img * nchunk * 3 * c, nchunk, c, ch, s, sm)) return;
  const double mx = mean[img * 2 * c + ch], my = mean[img * 2 * c + c + ch];
  const double ex = mx - shift[img * 2 * c + ch], ey = my - shift[img * 2 * c + c + ch];
  double* o = out + img * 5 * c + ch;
  o[0] = mx;
  o[c] = my;
  o[2L * c] = s[0] / hw - ex * ex;
  o[3L * c] = s[1] / hw - ey * ey;
  o[4L * c] = s[2] / hw - ex * ey;
}

// one block per image: out[img] (+)= sum_c alpha_c S1_c + beta_c S2_c, a thread's channels in ascending order,
// then the butterfly and the four waves
__global__ __launch_bounds__(256) void dists_score_kernel(const double* __restrict__ mom,
                                                          const double* __restrict__ alpha,
                                                          const double* __restrict__ beta, int c, int accumulate,
                                                          double* __restrict__ out) {
  __shared__ double red[4];
  const long img = blockIdx.x;
  const int t = threadIdx.x;
  const double* m = mom + img * 5 * c;
  const double c1 = 1e-6, c2 = 1e-6;
  double s = 0.0;
  for (int ch = t; ch < c; ch += 256) {
    const double mx = m[ch], my = m[c + ch], vx = m[2L * c + ch], vy = m[3L * c + ch], cxy = m[4L * c + ch];
    const double s1 = (2.0 * (mx * my) + c1) / ((mx * mx + my * my) + c1);
    const double s2 = (2.0 * cxy + c2) / ((vx + vy) + c2);
    s += alpha[ch] * s1 + beta[ch] * s2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((t & 63) == 0) red[t >> 6] = s;
  __syncthreads();
  if (t == 0) {
    const double v = (red[0] + red[1]) + (red[2] + red[3]);
    out[img] = accumulate ? out[img] + v : v;
  }
}

template <int PASS>
void launch_moments(bool wide, dim3 grid, hipStream_t s, const float* x, int ldx, const float* y, int ldy, long hw,
                    int c, int tx, const double* shift, double* part) {
  if (wide)
    hipLaunchKernelGGL((dists_moments_kernel<PASS, true>), grid, dim3(256), 0, s, x, ldx, y, ldy, hw, c, tx, shift,
                       part);
  else
    hipLaunchKernelGGL((dists_moments_kernel<PASS, false>), grid, dim3(256), 0, s, x, ldx, y, ldy, hw, c, tx, shift,
                       part);
}

// ---------------------------------------------------------------- the training loss (DISTS.loss) and its backward
// prep of float images in [-1, 1]: r = v * 0.5f + 0.5f (a multiply, then an add), norm = (r - mean_c) / std_c
template <typename T>
__global__ __launch_bounds__(256) void dists_prep_float_kernel(const T* __restrict__ img, int ld, long npix,
                                                               Affine3 af, float* __restrict__ raw,
                                                               float* __restrict__ norm) {
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const T* s = img + p * ld;
    f32x4 r, v;
    r.x = to_f32(s[0]) * 0.5f + 0.5f;
    r.y = to_f32(s[1]) * 0.5f + 0.5f;
    r.z = to_f32(s[2]) * 0.5f + 0.5f;
    r.w = 0.f;
    v.x = (r.x - af.mean[0]) / af.std[0];
    v.y = (r.y - af.mean[1]) / af.std[1];
    v.z = (r.z - af.mean[2]) / af.std[2];
    v.w = 0.f;
    *reinterpret_cast<f32x4*>(raw + p * 4) = r;
    *reinterpret_cast<f32x4*>(norm + p * 4) = v;
  }
}

// dpred_c = 0.5f * (dnorm_c / std_c + draw_c): the two gradients that reach the image, in the caller's dtype
template <typename T>
__global__ __launch_bounds__(256) void dists_prep_bwd_kernel(const float* __restrict__ dnorm, int ldn,
                                                             const float* __restrict__ draw, int ldr, long npix,
                                                             Affine3 af, T* __restrict__ dpred, int ldp) {
  for (long p = blockIdx.x * 256L + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(dnorm + p * ldn);
    const f32x4 b = *reinterpret_cast<const f32x4*>(draw + p * ldr);
    T* o = dpred + p * ldp;
    o[0] = from_f32<T>(0.5f * (a.x / af.std[0] + b.x));
    o[1] = from_f32<T>(0.5f * (a.y / af.std[1] + b.y));
    o[2] = from_f32<T>(0.5f * (a.z / af.std[2] + b.z));
  }
}

// The L2 pool's input gradient in gather form: one thread per V channels of one input pixel. Input row iy lies in
// the windows oy with 2 oy - 1 + d == iy: one (d = 1) for an even row, two (d = 2 at oy = (iy - 1) / 2, then d = 0
// at oy = (iy + 1) / 2) for an odd one, columns likewise, visited in output row-major order; a window outside
// the output is skipped. y is the stored forward output (>= 1e-6), so x == 0 gives exactly 0.
template <int V>
__global__ __launch_bounds__(256) void l2pool_bwd_kernel(const float* __restrict__ x, int h, int w, int c, int ldx,
                                                         const float* __restrict__ y, int ldy,
                                                         const float* __restrict__ dy, int lddy, int ho, int wo,
                                                         float* __restrict__ dx, int lddx, long total) {
  const int cv = c / V;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int ch = (int)(i % cv) * V;
    const long ip = i / cv;  // input pixel over the batch
    const int ix = (int)(ip % w);
    const long t = ip / w;
    const int iy = (int)(t % h);
    const long img = t / h;
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    const int ny = (iy & 1) ? 2 : 1, nx = (ix & 1) ? 2 : 1;
    for (int a = 0; a < ny; ++a) {
      const int oy = (iy & 1) ? (iy - 1) / 2 + a : iy / 2;
      if (oy >= ho) continue;
      for (int b = 0; b < nx; ++b) {
        const int ox = (ix & 1) ? (ix - 1) / 2 + b : ix / 2;
        if (ox >= wo) continue;
        const float g = ((iy & 1) ? 1.f : 2.f) * ((ix & 1) ? 1.f : 2.f) * 0.0625f;
        const long op = (img * ho + oy) * wo + ox;
        const float* qy = y + op * ldy + ch;
        const float* qd = dy + op * lddy + ch;
        if constexpr (V == 4) {
          const f32x4 yv = *reinterpret_cast<const f32x4*>(qy);
          const f32x4 dv = *reinterpret_cast<const f32x4*>(qd);
          acc[0] += g * (dv.x / yv.x); acc[1] += g * (dv.y / yv.y);
          acc[2] += g * (dv.z / yv.z); acc[3] += g * (dv.w / yv.w);
        } else {
          acc[0] += g * (qd[0] / qy[0]);
        }
      }
    }
    const float* qx = x + ip * ldx + ch;
    float* o = dx + ip * lddx + ch;
    if constexpr (V == 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(qx);
      *reinterpret_cast<f32x4*>(o) = f32x4{xv.x * acc[0], xv.y * acc[1], xv.z * acc[2], xv.w * acc[3]};
    } else {
      o[0] = qx[0] * acc[0];
    }
  }
}

// The tap score's backward, part 1: one thread per (image, channel), fp64. With g = gs[img] (the upstream gradient
// of the image's score), S1, S2 as in the score kernel, den1 = mx^2 + my^2 + c1, den2 = vx + vy + c2:
//   d / d x_p = A + B (y_p - my) + C (x_p - mx),
//   A = g alpha (2 my - 2 mx S1) / (den1 hw),  B = 2 g beta / (den2 hw),  C = -B S2.
// The apply kernel subtracts the metric's fp32 shifts kx = (float)mx, ky = (float)my, so what is stored is
// coef[img][5][c] = A + B (ky - my) + C (kx - mx), B, C, kx, ky. Two identical maps give S1 == S2 == 1 exactly,
// so A == 0 and C == -B, and with contraction off the two shift products cancel exactly.
__global__ __launch_bounds__(256) void dists_score_bwd_kernel(const double* __restrict__ mom,
                                                              const double* __restrict__ alpha,
                                                              const double* __restrict__ beta,
                                                              const double* __restrict__ gs, int c, double hw,
                                                              double* __restrict__ coef) {
  const long img = blockIdx.y;
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  const double* m = mom + img * 5 * c;
  const double c1 = 1e-6, c2 = 1e-6, g = gs[img];
  const double mx = m[ch], my = m[c + ch], vx = m[2L * c + ch], vy = m[3L * c + ch], cxy = m[4L * c + ch];
  const double den1 = (mx * mx + my * my) + c1, den2 = (vx + vy) + c2;
  const double s1 = (2.0 * (mx * my) + c1) / den1;
  const double s2 = (2.0 * cxy + c2) / den2;
  const double A = g * alpha[ch] * (2.0 * my - 2.0 * mx * s1) / (den1 * hw);
  const double B = 2.0 * g * beta[ch] / (den2 * hw);
  const double C = -B * s2;
  const double kx = (double)(float)mx, ky = (double)(float)my;
  double* o = coef + img * 5 * c + ch;
  o[0] = (A + B * (ky - my)) + C * (kx - mx);
  o[c] = B;
  o[2L * c] = C;
  o[3L * c] = kx;
  o[4L * c] = ky;
}

// Part 2, element-wise: grid (pixel chunks, channel blocks, n) with the moment passes' thread mapping (tx channel
// groups of 4 by ty pixel rows). A thread holds its channels' coefficients and walks TAPB_RUN pixels;
// dx (+)= (float)((A + B (double)(y - ky)) + C (double)(x - kx)), the differences in fp32 as the metric takes them.
constexpr int TAPB_RUN = 8;

template <bool WIDE>
__global__ __launch_bounds__(256) void dists_tap_bwd_kernel(const float* __restrict__ x, int ldx,
                                                            const float* __restrict__ y, int ldy,
                                                            const double* __restrict__ coef, long hw, int c, int tx,
                                                            int accumulate, float* __restrict__ dx, int ldd) {
  const int ty = 256 / tx;
  const int cx = threadIdx.x & (tx - 1), py = threadIdx.x / tx;
  const long img = blockIdx.z;
  const int ch = (blockIdx.y * tx + cx) * 4;
  if (ch >= c) return;
  const double* cf = coef + img * 5 * c;
  double A[4], B[4], C[4];
  float kx[4], ky[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool in = ch + e < c;
    A[e] = in ? cf[ch + e] : 0.0;
    B[e] = in ? cf[c + ch + e] : 0.0;
    C[e] = in ? cf[2L * c + ch + e] : 0.0;
    kx[e] = in ? (float)cf[3L * c + ch + e] : 0.f;
    ky[e] = in ? (float)cf[4L * c + ch + e] : 0.f;
  }
  const float* bx = x + img * hw * ldx + ch;
  const float* by = y + img * hw * ldy + ch;
  float* bd = dx + img * hw * ldd + ch;
  const long p0 = (long)blockIdx.x * ty * TAPB_RUN;
#pragma unroll
  for (int r = 0; r < TAPB_RUN; ++r) {
    const long p = p0 + py + (long)ty * r;
    if (p >= hw) break;
    const f32x4 a = ld4<WIDE>(bx + p * ldx, c, ch);
    const f32x4 b = ld4<WIDE>(by + p * ldy, c, ch);
    const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o[e] = (float)((A[e] + B[e] * (double)(bv[e] - ky[e])) + C[e] * (double)(av[e] - kx[e]));
    float* q = bd + p * ldd;
    if constexpr (WIDE) {
      f32x4 v = {o[0], o[1], o[2], o[3]};
      if (accumulate) v += *reinterpret_cast<const f32x4*>(q);
      *reinterpret_cast<f32x4*>(q) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ch + e < c) q[e] = accumulate ? q[e] + o[e] : o[e];
    }
  }
}

}  // namespace

extern "C" int rdeic_dists_prep_float(const void* img, int32_t ld, int32_t dtype, int64_t npix, float* raw,
                                      float* norm, void* stream) {
  if (!img || !raw || !norm || npix <= 0 || ld < 3 || dtype < 0 || dtype > 1 ||
      (((uintptr_t)raw | (uintptr_t)norm) & 15))
    return RDEIC_EINVAL;
  const dim3 grid((unsigned)std::min<long>((npix + 255) / 256, 65536));
  if (dtype == 1)
    hipLaunchKernelGGL(dists_prep_float_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16*)img, ld,
                       (long)npix, DISTS_AFFINE, raw, norm);
  else
    hipLaunchKernelGGL(dists_prep_float_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)img, ld,
                       (long)npix, DISTS_AFFINE, raw, norm);
  return launch_status();
}

extern "C" int rdeic_dists_prep_bwd(const float* dnorm, int32_t ld_dnorm, const float* draw, int32_t ld_draw,
                                    int64_t npix, void* dpred, int32_t ld_dpred, int32_t dtype, void* stream) {
  if (!dnorm || !draw || !dpred || npix <= 0 || ld_dnorm < 4 || ld_draw < 4 || ld_dnorm % 4 || ld_draw % 4 ||
      ld_dpred < 3 || dtype < 0 || dtype > 1 || (((uintptr_t)dnorm | (uintptr_t)draw) & 15))
    return RDEIC_EINVAL;
  const dim3 grid((unsigned)std::min<long>((npix + 255) / 256, 65536));
  if (dtype == 1)
    hipLaunchKernelGGL(dists_prep_bwd_kernel<bf16>, grid, dim3(256), 0, (hipStream_t)stream, dnorm, ld_dnorm, draw,
                       ld_draw, (long)npix, DISTS_AFFINE, (bf16*)dpred, ld_dpred);
  else
    hipLaunchKernelGGL(dists_prep_bwd_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, dnorm, ld_dnorm, draw,
                       ld_draw, (long)npix, DISTS_AFFINE, (float*)dpred, ld_dpred);
  return launch_status();
}

extern "C" int rdeic_dists_l2pool_bwd(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_x,
                                      const float* y, int32_t ld_y, const float* dy, int32_t ld_dy, float* dx,
                                      int32_t ld_dx, void* stream) {
  if (!x || !y || !dy || !dx || n <= 0 || h <= 0 || w <= 0 || c <= 0 || ld_x < c || ld_y < c || ld_dy < c ||
      ld_dx < c)
    return RDEIC_EINVAL;
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const bool v4 = c % 4 == 0 && ld_x % 4 == 0 && ld_y % 4 == 0 && ld_dy % 4 == 0 && ld_dx % 4 == 0 &&
                  !(((uintptr_t)x | (uintptr_t)y | (uintptr_t)dy | (uintptr_t)dx) & 15);
  const long total = (long)n * h * w * (v4 ? c / 4 : c);
  const dim3 grid((unsigned)std::min<long>((total + 255) / 256, 1L << 20));
  if (v4)
    hipLaunchKernelGGL(l2pool_bwd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, h, w, c, ld_x, y, ld_y, dy,
                       ld_dy, ho, wo, dx, ld_dx, total);
  else
    hipLaunchKernelGGL(l2pool_bwd_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, h, w, c, ld_x, y, ld_y, dy,
                       ld_dy, ho, wo, dx, ld_dx, total);
  return launch_status();
}

extern "C" int rdeic_dists_score_bwd(const double* mom, const double* alpha, const double* beta, const double* gs,
                                     int32_t n, int64_t hw, int32_t c, double* coef, void* stream) {
  if (!mom || !alpha || !beta || !gs || !coef || n <= 0 || n > 65535 || hw <= 0 || c <= 0) return RDEIC_EINVAL;
  hipLaunchKernelGGL(dists_score_bwd_kernel, dim3((unsigned)((c + 255) / 256), n), dim3(256), 0, (hipStream_t)stream,
                     mom, alpha, beta, gs, c, (double)hw, coef);
  return launch_status();
}

extern "C" int rdeic_dists_tap_bwd(const float* x, int32_t ldx, const float* y, int32_t ldy, const double* coef,
                                   int32_t n, int64_t hw, int32_t c, int32_t accumulate, float* dx, int32_t ld_dx,
                                   void* stream) {
  if (!x || !y || !coef || !dx || n <= 0 || n > 65535 || hw <= 0 || c <= 0 || ldx < c || ldy < c || ld_dx < c)
    return RDEIC_EINVAL;
  const MomGeom g = mom_geom(hw, c);  // tx, ty and the channel blocks; the pixel chunks are this kernel's own
  const long nchunk = (hw + (long)g.ty * TAPB_RUN - 1) / ((long)g.ty * TAPB_RUN);
  if (nchunk > 0x7fffffffL || g.cblocks > 65535) return RDEIC_EINVAL;
  const bool wide = c % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && ld_dx % 4 == 0 &&
                    !(((uintptr_t)x | (uintptr_t)y | (uintptr_t)dx) & 15);
  const dim3 grid((unsigned)nchunk, g.cblocks, n);
  if (wide)
    hipLaunchKernelGGL(dists_tap_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, coef,
                       (long)hw, c, g.tx, accumulate, dx, ld_dx);
  else
    hipLaunchKernelGGL(dists_tap_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, coef,
                       (long)hw, c, g.tx, accumulate, dx, ld_dx);
  return launch_status();
}

extern "C" int rdeic_dists_prep(const uint8_t* img, int32_t n, int32_t h, int32_t w, float* raw, float* norm,
                                void* stream) {
  if (!img || !raw || !norm || n <= 0 || h <= 0 || w <= 0 || (((uintptr_t)raw | (uintptr_t)norm) & 15))
    return RDEIC_EINVAL;
  const long npix = (long)n * h * w;
  hipLaunchKernelGGL(dists_prep_kernel, dim3((unsigned)std::min<long>((npix + 255) / 256, 65536)), dim3(256), 0,
                     (hipStream_t)stream, img, npix, DISTS_AFFINE, raw, norm);
  return launch_status();
}

extern "C" int rdeic_dists_l2pool(const float* in, int32_t n, int32_t h, int32_t w, int32_t c, int32_t ld_in,
                                  float* out, int32_t ld_out, void* stream) {
  if (!in || !out || n <= 0 || h <= 0 || w <= 0 || c <= 0 || ld_in < c || ld_out < c) return RDEIC_EINVAL;
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const bool v4 = c % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && !(((uintptr_t)in | (uintptr_t)out) & 15);
  const long total = (long)n * ho * wo * (v4 ? c / 4 : c);
  const dim3 grid((unsigned)std::min<long>((total + 255) / 256, 1L << 20));
  if (v4)
    hipLaunchKernelGGL(l2pool_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, in, h, w, c, ld_in, ho, wo, out,
                       ld_out, total);
  else
    hipLaunchKernelGGL(l2pool_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, in, h, w, c, ld_in, ho, wo, out,
                       ld_out, total);
  return launch_status();
}

extern "C" size_t rdeic_dists_moments_ws_doubles(int32_t n, int64_t hw, int32_t c) {
  if (n <= 0 || hw <= 0 || c <= 0) return 0;
  const MomGeom g = mom_geom(hw, c);
  return (size_t)n * ((size_t)g.nchunk * 5 + 4) * (size_t)c;
}

extern "C" int rdeic_dists_moments(const float* x, int32_t ldx, const float* y, int32_t ldy, int32_t n, int64_t hw,
                                   int32_t c, double* ws, size_t ws_doubles, double* out, void* stream) {
  if (!x || !y || !ws || !out || n <= 0 || n > 65535 || hw <= 0 || c <= 0 || ldx < c || ldy < c)
    return RDEIC_EINVAL;
  if (ws_doubles < rdeic_dists_moments_ws_doubles(n, hw, c)) return RDEIC_ENOSPC;
  const MomGeom g = mom_geom(hw, c);
  if (g.nchunk > 0x7fffffffL || g.cblocks > 65535) return RDEIC_EINVAL;
  const bool wide = c % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && !(((uintptr_t)x | (uintptr_t)y) & 15);
  double* part1 = ws;                                     // [n][nchunk][2][c]
  double* part2 = part1 + (size_t)n * g.nchunk * 2 * c;   // [n][nchunk][3][c]
  double* mean = part2 + (size_t)n * g.nchunk * 3 * c;    // [n][2][c]
  double* shift = mean + (size_t)n * 2 * c;               // [n][2][c]
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)g.nchunk, g.cblocks, n);
  const dim3 fgrid((unsigned)((c + FIN_C - 1) / FIN_C), n);
  launch_moments<1>(wide, grid, s, x, ldx, y, ldy, hw, c, g.tx, nullptr, part1);
  hipLaunchKernelGGL(dists_mean_finalize_kernel, fgrid, dim3(256), 0, s, part1, g.nchunk, c, (double)hw, mean, shift);
  launch_moments<2>(wide, grid, s, x, ldx, y, ldy, hw, c, g.tx, shift, part2);
  hipLaunchKernelGGL(dists_moment_finalize_kernel, fgrid, dim3(256), 0, s, part2, g.nchunk, c, (double)hw, mean, shift,
                     out);
  return launch_status();
}

extern "C" int rdeic_dists_score(const double* mom, const double* alpha, const double* beta, int32_t n, int32_t c,
                                 int32_t accumulate, double* out, void* stream) {
  if (!mom || !alpha || !beta || !out || n <= 0 || c <= 0) return RDEIC_EINVAL;
  hipLaunchKernelGGL(dists_score_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, mom, alpha, beta, c, accumulate,
                     out);
  return launch_status();
}
