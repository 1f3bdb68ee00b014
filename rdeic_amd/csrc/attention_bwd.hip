// Flash attention for the fine-tune step (bf16, head dim 16 / 64): a forward that also returns the
// log-sum-exp of every query row, and a backward that recomputes P = exp(scale S - lse) from Q, K and
// that LSE. No [Lq][Lk] tensor is written by either.
//
// Structure of the backward: two sweeps (no float atomics, no hand-off between workgroups, so the
// gradients are bit-reproducible):
//   delta kernel  delta_i = sum_d dO_id O_id (fp32), one thread per (image, query, head)
//   dK/dV kernel  one workgroup owns 64 keys (16 per wave) and sweeps the queries in 64-row tiles
//   dQ kernel     one workgroup owns 64 queries (16 per wave) and sweeps the keys in 64-row tiles
// With few key blocks (cross-attention, Lk = 77) the dK/dV query sweep is cut into chunks; each chunk
// writes fp32 partial slabs and a small kernel adds them in chunk order.
//
// MFMA shapes: D[row = 4 (lane >> 4) + reg][col = lane & 15] for both
//   v_mfma_f32_16x16x16_bf16  A[row = lane & 15][k = 4 (lane >> 4) + j], B[k = 4 (lane >> 4) + j][col = lane & 15]
//   v_mfma_f32_16x16x32_bf16  the same with 8 (lane >> 4) + j, j < 8
// A D tile holds 4 consecutive rows per lane. When the NEXT product sums over that row index, two D
// tiles (rows 32 u .. 32 u + 15 and 32 u + 16 .. 32 u + 31) packed to bf16 are its 16x16x32 B operand
// with k slot 8 g + j = row 32 u + 16 (j >> 2) + 4 g + (j & 3); the other operand is read in the same k
// order, so P and dS never leave the registers:
//   forward / dQ  S^T = K Q^T (query on the lane; row statistics are per-lane scalars), then
//                 O^T += V^T P^T, dQ^T += K^T dS^T
//   dK/dV         S = Q K^T, dP = dO V^T (key on the lane), then dV^T += dO^T P, dK^T += Q^T dS
// The swept operand is staged in LDS once per tile, row-major for the first products (one 16- or
// 8-byte read per fragment) and transposed for the second ones (two 8-byte reads). The next tile's
// global loads are issued into registers before the current tile's products and stored to LDS after
// them, so their latency hides behind the MFMAs even at one workgroup per CU.
#include "common.h"
#include "../../include/rdeic_hip.h"
#include "prof.h"

namespace {

typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int FT = 64;       // rows (queries or keys) per tile and per workgroup
constexpr int TS = FT + 4;   // row stride of a transposed tile [dh][FT] (elements; 8-byte aligned rows)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

__device__ __forceinline__ f32x4 mma32(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ bf16x4 cvt4(f32x4 v) { return bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]}; }
// the B operand of a second product from the D tiles of row groups 32 u (lo) and 32 u + 16 (hi)
__device__ __forceinline__ bf16x8 pack8(f32x4 lo, f32x4 hi) {
  return __builtin_shufflevector(cvt4(lo), cvt4(hi), 0, 1, 2, 3, 4, 5, 6, 7);
}
// ... and its A operand: row d of a transposed tile, in the same k order
__device__ __forceinline__ bf16x8 lds_t(const bf16* tr, int d, int u, int g) {
  const bf16* p = tr + d * TS + 32 * u + 4 * g;
  return __builtin_shufflevector(*(const bf16x4*)p, *(const bf16x4*)(p + 16), 0, 1, 2, 3, 4, 5, 6, 7);
}

// The first products (reduction over the head dim): 16x16x32 steps at dh = 64, one 16x16x16 at dh = 16.
// Row-major tiles have a row stride of DH + 8 elements (16-byte aligned rows).
template <int DH> struct First;
template <> struct First<64> {
  typedef bf16x8 frag;
  static constexpr int NK = 2;
  // global rows are 16-byte aligned by the entry's pointer / stride rules
  static __device__ __forceinline__ frag global(const bf16* row, int kk, int g, bool ok) {
    return ok ? *(const bf16x8*)(row + kk * 32 + 8 * g) : bf16x8{};
  }
  static __device__ __forceinline__ frag lds(const bf16* row, int kk, int g) {
    return *(const bf16x8*)(row + kk * 32 + 8 * g);
  }
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) { return mma32(a, b, c); }
};
template <> struct First<16> {
  typedef s16x4 frag;
  static constexpr int NK = 1;
  static __device__ __forceinline__ frag global(const bf16* row, int kk, int g, bool ok) {
    return ok ? *(const s16x4*)(row + 4 * g) : s16x4{0, 0, 0, 0};
  }
  static __device__ __forceinline__ frag lds(const bf16* row, int kk, int g) { return *(const s16x4*)(row + 4 * g); }
  static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
  }
};

// Rows [row0, row0 + 64) of a [nrows][ld] matrix (dh columns), one 16-byte chunk per thread and step:
// load() into registers (rows >= nrows: zeros, never read), store() to LDS row-major rm[64][DH + 8] and /
// or transposed tr[DH][TS]. Chunk -> (row, column chunk): with a transposed copy the row is the fastest
// index (a wave's 2-byte transposed writes are consecutive: no bank conflict), else the column chunk
// (coalesced rows).
template <int DH, bool TR> struct Tile {
  static constexpr int CPR = DH / 8;                           // chunks per row
  static constexpr int N = (FT * CPR + 255) / 256;             // chunks per thread
  bf16x8 x[N];
  static __device__ __forceinline__ int row_of(int c) { return TR ? c % FT : c / CPR; }
  static __device__ __forceinline__ int chunk_of(int c) { return TR ? c / FT : c % CPR; }
  __device__ __forceinline__ void load(const bf16* g, int ld, int row0, int nrows) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = threadIdx.x + 256 * i;
      x[i] = bf16x8{};
      if (c < FT * CPR && row0 + row_of(c) < nrows)
        x[i] = *(const bf16x8*)(g + (long)(row0 + row_of(c)) * ld + chunk_of(c) * 8);
    }
  }
  template <bool RM> __device__ __forceinline__ void store(bf16* rm, bf16* tr) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = threadIdx.x + 256 * i;
      if (c >= FT * CPR) continue;
      const int r = row_of(c), cc = chunk_of(c);
      if constexpr (RM) *(bf16x8*)(rm + r * (DH + 8) + cc * 8) = x[i];
      if constexpr (TR) {
#pragma unroll
        for (int j = 0; j < 8; ++j) tr[(cc * 8 + j) * TS + r] = x[i][j];
      }
    }
  }
};

// --------------------------------------------------------------------------------------- forward
template <int DH>
__global__ __launch_bounds__(256) void fa_fwd_kernel(const bf16* __restrict__ q, int ldq, const bf16* __restrict__ k,
                                                     int ldk, const bf16* __restrict__ v, int ldv,
                                                     bf16* __restrict__ o, int ldo, float* __restrict__ lse, int heads,
                                                     int lq, int lk, float sl2) {
  typedef First<DH> F;
  constexpr int ND = DH / 16, RS = DH + 8;
  __shared__ __attribute__((aligned(16))) bf16 Ks[FT * RS];
  __shared__ __attribute__((aligned(16))) bf16 Vt[DH * TS];
  const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int qi = blockIdx.x * FT + wave * 16 + c;  // this lane's query
  const bool qok = qi < lq;
  const bf16* qb = q + (long)b * lq * ldq + h * DH;
  const bf16* kb = k + (long)b * lk * ldk + h * DH;
  const bf16* vb = v + (long)b * lk * ldv + h * DH;
  typename F::frag qf[F::NK];
#pragma unroll
  for (int kk = 0; kk < F::NK; ++kk) qf[kk] = F::global(qb + (long)qi * ldq, kk, g, qok);
  f32x4 oacc[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;  // running max (log2 domain, scaled) and sum
  Tile<DH, false> kr;
  Tile<DH, true> vr;
  kr.load(kb, ldk, 0, lk);
  vr.load(vb, ldv, 0, lk);
  for (int j0 = 0; j0 < lk; j0 += FT) {
    __syncthreads();
    kr.template store<true>(Ks, nullptr);
    vr.template store<false>(nullptr, Vt);
    __syncthreads();
    if (j0 + FT < lk) {
      kr.load(kb, ldk, j0 + FT, lk);
      vr.load(vb, ldv, j0 + FT, lk);
    }
    f32x4 s[4];  // s[js][r] = S[qi][j0 + 16 js + 4 g + r]
    float mx = -INFINITY;
#pragma unroll
    for (int js = 0; js < 4; ++js) {
      s[js] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < F::NK; ++kk) s[js] = F::mma(F::lds(Ks + (js * 16 + c) * RS, kk, g), qf[kk], s[js]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[js][r] = (j0 + js * 16 + 4 * g + r < lk) ? s[js][r] * sl2 : -INFINITY;
        mx = fmaxf(mx, s[js][r]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);  // finite: key j0 of every tile is in range
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    float ps = 0.f;
#pragma unroll
    for (int js = 0; js < 4; ++js) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[js][r] = __builtin_amdgcn_exp2f(s[js][r] - mn);
        ps += s[js][r];
      }
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;
    const bf16x8 pf[2] = {pack8(s[0], s[1]), pack8(s[2], s[3])};
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      oacc[dt] *= alpha;
#pragma unroll
      for (int u = 0; u < 2; ++u) oacc[dt] = mma32(lds_t(Vt, dt * 16 + c, u, g), pf[u], oacc[dt]);
    }
  }
  if (!qok) return;
  const float inv = 1.0f / l;
  bf16* ob = o + ((long)b * lq + qi) * ldo + h * DH;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) *(bf16x4*)(ob + dt * 16 + 4 * g) = cvt4(oacc[dt] * inv);
  if (g == 0) lse[(long)bh * lq + qi] = (m + __builtin_amdgcn_logf(l)) * LN2;  // v_log_f32 is log2
}

// ---------------------------------------------------------------------------------------- delta
// delta[(b heads + h) lq + i] = sum_d dO[b, i, h, d] O[b, i, h, d]; the head is the fastest thread index
template <int DH>
__global__ __launch_bounds__(256) void fa_delta_kernel(const bf16* __restrict__ o, int ldo, const bf16* __restrict__ d_o,
                                                       int lddo, float* __restrict__ delta, int heads, int lq,
                                                       long total) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int h = (int)(t % heads);
  const long row = t / heads;  // b lq + i
  const long b = row / lq, i = row % lq;
  const bf16* op = o + row * ldo + h * DH;
  const bf16* dp = d_o + row * lddo + h * DH;
  float acc = 0.f;
#pragma unroll
  for (int cc = 0; cc < DH / 8; ++cc) {
    const bf16x8 x = *(const bf16x8*)(op + cc * 8), y = *(const bf16x8*)(dp + cc * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_fmaf((float)x[j], (float)y[j], acc);
  }
  delta[(b * heads + h) * lq + i] = acc;
}

// ------------------------------------------------------------------------------- backward: dK, dV
// grid (key blocks, batch * heads, query chunks). chunks == 1: bf16 dK / dV; else fp32 slabs
// part[which][chunk][bh][key][d] (which 0 = dK, 1 = dV), summed by fa_slab_sum_kernel.
template <int DH>
__global__ __launch_bounds__(256) void fa_bwd_dkv_kernel(const bf16* __restrict__ q, int ldq, const bf16* __restrict__ k,
                                                         int ldk, const bf16* __restrict__ v, int ldv,
                                                         const bf16* __restrict__ d_o, int lddo,
                                                         const float* __restrict__ lse, const float* __restrict__ delta,
                                                         bf16* __restrict__ dk, int lddk, bf16* __restrict__ dv, int lddv,
                                                         float* __restrict__ part, int heads, int lq, int lk, float scale,
                                                         int q_per_chunk) {
  typedef First<DH> F;
  constexpr int ND = DH / 16, RS = DH + 8;
  __shared__ __attribute__((aligned(16))) bf16 Qs[FT * RS];
  __shared__ __attribute__((aligned(16))) bf16 Os[FT * RS];
  __shared__ __attribute__((aligned(16))) bf16 Qt[DH * TS];
  __shared__ __attribute__((aligned(16))) bf16 Ot[DH * TS];
  __shared__ __attribute__((aligned(16))) float lse2s[FT];
  __shared__ __attribute__((aligned(16))) float dls[FT];
  const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int kj = blockIdx.x * FT + wave * 16 + c;  // this lane's key
  const bool kok = kj < lk;
  const float sl2 = scale * LOG2E;
  const bf16* qb = q + (long)b * lq * ldq + h * DH;
  const bf16* dob = d_o + (long)b * lq * lddo + h * DH;
  const bf16* kb = k + (long)b * lk * ldk + h * DH;
  const bf16* vb = v + (long)b * lk * ldv + h * DH;
  typename F::frag kf[F::NK], vf[F::NK];
#pragma unroll
  for (int kk = 0; kk < F::NK; ++kk) {
    kf[kk] = F::global(kb + (long)kj * ldk, kk, g, kok);
    vf[kk] = F::global(vb + (long)kj * ldv, kk, g, kok);
  }
  f32x4 dka[ND], dva[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) dka[dt] = dva[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ibeg = blockIdx.z * q_per_chunk;
  const int iend = ibeg + q_per_chunk < lq ? ibeg + q_per_chunk : lq;
  Tile<DH, true> qr, dor;
  float lse_r = 0.f, dl_r = 0.f;  // threads < 64: the row constants of the tile in flight
  auto load_rows = [&](int i0) {
    qr.load(qb, ldq, i0, lq);
    dor.load(dob, lddo, i0, lq);
    if (threadIdx.x < FT) {
      const bool ok = i0 + (int)threadIdx.x < lq;
      lse_r = ok ? lse[(long)bh * lq + i0 + threadIdx.x] * LOG2E : 0.f;
      dl_r = ok ? delta[(long)bh * lq + i0 + threadIdx.x] : 0.f;
    }
  };
  load_rows(ibeg);
  for (int i0 = ibeg; i0 < iend; i0 += FT) {
    __syncthreads();
    qr.template store<true>(Qs, Qt);
    dor.template store<true>(Os, Ot);
    if (threadIdx.x < FT) {
      lse2s[threadIdx.x] = lse_r;
      dls[threadIdx.x] = dl_r;
    }
    __syncthreads();
    if (i0 + FT < iend) load_rows(i0 + FT);
    f32x4 p[4], ds[4];  // [is][r]: query i0 + 16 is + 4 g + r, key kj
#pragma unroll
    for (int is = 0; is < 4; ++is) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < F::NK; ++kk) {
        s = F::mma(F::lds(Qs + (is * 16 + c) * RS, kk, g), kf[kk], s);
        dp = F::mma(F::lds(Os + (is * 16 + c) * RS, kk, g), vf[kk], dp);
      }
      const f32x4 l4 = *(const f32x4*)(lse2s + is * 16 + 4 * g);
      const f32x4 d4 = *(const f32x4*)(dls + is * 16 + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = kok && (i0 + is * 16 + 4 * g + r < lq);
        p[is][r] = ok ? __builtin_amdgcn_exp2f(s[r] * sl2 - l4[r]) : 0.f;
        ds[is][r] = p[is][r] * (dp[r] - d4[r]) * scale;
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8 pf = pack8(p[2 * u], p[2 * u + 1]), dsf = pack8(ds[2 * u], ds[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) {
        dva[dt] = mma32(lds_t(Ot, dt * 16 + c, u, g), pf, dva[dt]);
        dka[dt] = mma32(lds_t(Qt, dt * 16 + c, u, g), dsf, dka[dt]);
      }
    }
  }
  if (!kok) return;
  if (gridDim.z == 1) {
    bf16* dkp = dk + ((long)b * lk + kj) * lddk + h * DH;
    bf16* dvp = dv + ((long)b * lk + kj) * lddv + h * DH;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      *(bf16x4*)(dkp + dt * 16 + 4 * g) = cvt4(dka[dt]);
      *(bf16x4*)(dvp + dt * 16 + 4 * g) = cvt4(dva[dt]);
    }
    return;
  }
  const long plane = (long)gridDim.y * lk * DH;  // one chunk's [bh][key][d]
  float* pk = part + (long)blockIdx.z * plane + ((long)bh * lk + kj) * DH;
  float* pv = pk + (long)gridDim.z * plane;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) {
    *(f32x4*)(pk + dt * 16 + 4 * g) = dka[dt];
    *(f32x4*)(pv + dt * 16 + 4 * g) = dva[dt];
  }
}

// sums the dK / dV slabs in chunk order; one thread per 4 consecutive d. blockIdx.y: 0 = dK, 1 = dV
template <int DH>
__global__ __launch_bounds__(256) void fa_slab_sum_kernel(const float* __restrict__ part, int chunks,
                                                          bf16* __restrict__ dk, int lddk, bf16* __restrict__ dv,
                                                          int lddv, int heads, int lk, long plane) {
  const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e >= plane) return;
  const float* src = part + (long)blockIdx.y * chunks * plane + e;
  f32x4 acc = *(const f32x4*)src;
  for (int ch = 1; ch < chunks; ++ch) acc += *(const f32x4*)(src + (long)ch * plane);
  const int d = (int)(e % DH);
  const long row = e / DH;  // bh lk + key
  const long bh = row / lk, key = row % lk;
  const long b = bh / heads, h = bh % heads;
  bf16* dst = blockIdx.y ? dv + (b * lk + key) * lddv + h * DH + d : dk + (b * lk + key) * lddk + h * DH + d;
  *(bf16x4*)dst = cvt4(acc);
}

// ----------------------------------------------------------------------------------- backward: dQ
template <int DH>
__global__ __launch_bounds__(256) void fa_bwd_dq_kernel(const bf16* __restrict__ q, int ldq, const bf16* __restrict__ k,
                                                        int ldk, const bf16* __restrict__ v, int ldv,
                                                        const bf16* __restrict__ d_o, int lddo,
                                                        const float* __restrict__ lse, const float* __restrict__ delta,
                                                        bf16* __restrict__ dq, int lddq, int heads, int lq, int lk,
                                                        float scale) {
  typedef First<DH> F;
  constexpr int ND = DH / 16, RS = DH + 8;
  __shared__ __attribute__((aligned(16))) bf16 Ks[FT * RS];
  __shared__ __attribute__((aligned(16))) bf16 Vs[FT * RS];
  __shared__ __attribute__((aligned(16))) bf16 Kt[DH * TS];
  const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int qi = blockIdx.x * FT + wave * 16 + c;  // this lane's query
  const bool qok = qi < lq;
  const float sl2 = scale * LOG2E;
  const bf16* kb = k + (long)b * lk * ldk + h * DH;
  const bf16* vb = v + (long)b * lk * ldv + h * DH;
  typename F::frag qf[F::NK], dof[F::NK];
#pragma unroll
  for (int kk = 0; kk < F::NK; ++kk) {
    qf[kk] = F::global(q + ((long)b * lq + qi) * ldq + h * DH, kk, g, qok);
    dof[kk] = F::global(d_o + ((long)b * lq + qi) * lddo + h * DH, kk, g, qok);
  }
  const float lse2 = qok ? lse[(long)bh * lq + qi] * LOG2E : 0.f;
  const float dl = qok ? delta[(long)bh * lq + qi] : 0.f;
  f32x4 dqa[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) dqa[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  Tile<DH, true> kr;
  Tile<DH, false> vr;
  kr.load(kb, ldk, 0, lk);
  vr.load(vb, ldv, 0, lk);
  for (int j0 = 0; j0 < lk; j0 += FT) {
    __syncthreads();
    kr.template store<true>(Ks, Kt);
    vr.template store<true>(Vs, nullptr);
    __syncthreads();
    if (j0 + FT < lk) {
      kr.load(kb, ldk, j0 + FT, lk);
      vr.load(vb, ldv, j0 + FT, lk);
    }
    f32x4 ds[4];  // [js][r]: query qi, key j0 + 16 js + 4 g + r
#pragma unroll
    for (int js = 0; js < 4; ++js) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < F::NK; ++kk) {
        s = F::mma(F::lds(Ks + (js * 16 + c) * RS, kk, g), qf[kk], s);
        dp = F::mma(F::lds(Vs + (js * 16 + c) * RS, kk, g), dof[kk], dp);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = qok && (j0 + js * 16 + 4 * g + r < lk);
        const float p = ok ? __builtin_amdgcn_exp2f(s[r] * sl2 - lse2) : 0.f;
        ds[js][r] = p * (dp[r] - dl) * scale;
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16x8 dsf = pack8(ds[2 * u], ds[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) dqa[dt] = mma32(lds_t(Kt, dt * 16 + c, u, g), dsf, dqa[dt]);
    }
  }
  if (!qok) return;
  bf16* dqp = dq + ((long)b * lq + qi) * lddq + h * DH;
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) *(bf16x4*)(dqp + dt * 16 + 4 * g) = cvt4(dqa[dt]);
}

// ----------------------------------------------------------------------------------------- host
// Query chunks of the dK/dV sweep. Split only when the key blocks alone leave most of the chip idle
// (fewer than 64 workgroups on 256 CUs), towards ~256 workgroups. max_chunks (what the workspace is
// sized for) is monotone in lq; the launched count never exceeds it.
struct BwdPlan {
  int max_chunks, chunks, q_per_chunk;
  size_t delta_floats, slab_floats;
};

BwdPlan bwd_plan(int batch, int heads, int lq, int lk, int dh) {
  BwdPlan p;
  const long groups = (long)cdiv(lk, FT) * batch * heads;
  const int qtiles = cdiv(lq, FT);
  long want = groups >= 64 ? 1 : (256 + groups - 1) / groups;
  p.max_chunks = (int)(want < qtiles ? want : qtiles);
  const int tiles_per = cdiv(qtiles, p.max_chunks);
  p.chunks = cdiv(qtiles, tiles_per);
  p.q_per_chunk = tiles_per * FT;
  p.delta_floats = ((size_t)batch * heads * lq + 3) / 4 * 4;  // the slabs after it stay 16-byte aligned
  p.slab_floats = p.max_chunks > 1 ? (size_t)2 * p.max_chunks * batch * heads * lk * dh : 0;
  return p;
}

bool in_ok(const void* p, int ld) { return p && ld % 8 == 0 && ((uintptr_t)p) % 16 == 0; }
bool out_ok(const void* p, int ld) { return ld % 4 == 0 && ((uintptr_t)p) % 8 == 0; }
bool dims_ok(int batch, int heads, int lq, int lk, int dh, int dtype) {
  return dtype == 1 && (dh == 16 || dh == 64) && batch > 0 && heads > 0 && lq > 0 && lk > 0 &&
         (long)batch * heads <= 65535;
}
long long shape_key(int batch, int heads, int lq, int lk, int dh) {
  return ((long long)(dh & 0xffff) << 48) | ((long long)(lq < 0xffff ? lq : 0xffff) << 32) |
         ((long long)(lk < 0xffff ? lk : 0xffff) << 16) | (batch * heads < 0xffff ? batch * heads : 0xffff);
}

template <int DH>
int launch_fwd(const bf16* q, int ldq, const bf16* k, int ldk, const bf16* v, int ldv, bf16* o, int ldo, float* lse,
               int batch, int heads, int lq, int lk, float scale, hipStream_t s) {
  hipLaunchKernelGGL(fa_fwd_kernel<DH>, dim3(cdiv(lq, FT), batch * heads), dim3(256), 0, s, q, ldq, k, ldk, v, ldv, o,
                     ldo, lse, heads, lq, lk, scale * LOG2E);
  return launch_status();
}

template <int DH>
int launch_bwd(const bf16* q, int ldq, const bf16* k, int ldk, const bf16* v, int ldv, const bf16* o, int ldo,
               const bf16* d_o, int lddo, const float* lse, bf16* dq, int lddq, bf16* dk, int lddk, bf16* dv, int lddv,
               float* ws, const BwdPlan& p, int batch, int heads, int lq, int lk, float scale, hipStream_t s) {
  float* delta = ws;
  float* part = ws + p.delta_floats;
  const long rows = (long)batch * lq * heads;
  hipLaunchKernelGGL(fa_delta_kernel<DH>, dim3(cdiv(rows, 256)), dim3(256), 0, s, o, ldo, d_o, lddo, delta, heads, lq,
                     rows);
  if (dk) {
    hipLaunchKernelGGL(fa_bwd_dkv_kernel<DH>, dim3(cdiv(lk, FT), batch * heads, p.chunks), dim3(256), 0, s, q, ldq, k,
                       ldk, v, ldv, d_o, lddo, lse, delta, dk, lddk, dv, lddv, part, heads, lq, lk, scale,
                       p.q_per_chunk);
    if (p.chunks > 1) {
      const long plane = (long)batch * heads * lk * DH;
      hipLaunchKernelGGL(fa_slab_sum_kernel<DH>, dim3(cdiv(plane / 4, 256), 2), dim3(256), 0, s, part, p.chunks, dk,
                         lddk, dv, lddv, heads, lk, plane);
    }
  }
  if (dq)
    hipLaunchKernelGGL(fa_bwd_dq_kernel<DH>, dim3(cdiv(lq, FT), batch * heads), dim3(256), 0, s, q, ldq, k, ldk, v, ldv,
                       d_o, lddo, lse, delta, dq, lddq, heads, lq, lk, scale);
  return launch_status();
}

}  // namespace

extern "C" int rdeic_attention_fwd_lse(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v,
                                       int32_t ldv, void* o, int32_t ldo, float* lse, int32_t batch, int32_t heads,
                                       int32_t lq, int32_t lk, int32_t dh, float scale, int32_t dtype, void* stream) {
  if (!dims_ok(batch, heads, lq, lk, dh, dtype) || !in_ok(q, ldq) || !in_ok(k, ldk) || !in_ok(v, ldv) || !o ||
      !out_ok(o, ldo) || !lse || ((uintptr_t)lse) % 4)
    return RDEIC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(s, dh >= 64 ? RDEIC_PROF_ATTN : RDEIC_PROF_ATTN_SMALL, 4.0 * batch * heads * (double)lq * lk * dh,
               shape_key(batch, heads, lq, lk, dh));
  if (dh == 64)
    return launch_fwd<64>((const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, (bf16*)o, ldo, lse, batch,
                          heads, lq, lk, scale, s);
  return launch_fwd<16>((const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, (bf16*)o, ldo, lse, batch, heads,
                        lq, lk, scale, s);
}

extern "C" size_t rdeic_attention_bwd_workspace(int32_t batch, int32_t heads, int32_t lq, int32_t lk, int32_t dh) {
  if (batch <= 0 || heads <= 0 || lq <= 0 || lk <= 0 || dh <= 0) return 0;
  const BwdPlan p = bwd_plan(batch, heads, lq, lk, dh);
  return (p.delta_floats + p.slab_floats) * sizeof(float);
}

extern "C" int rdeic_attention_bwd(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv,
                                   const void* o, int32_t ldo, const void* d_o, int32_t lddo, const float* lse,
                                   void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv, int32_t lddv, void* ws,
                                   size_t ws_bytes, int32_t batch, int32_t heads, int32_t lq, int32_t lk, int32_t dh,
                                   float scale, int32_t dtype, void* stream) {
  if (!dims_ok(batch, heads, lq, lk, dh, dtype) || !in_ok(q, ldq) || !in_ok(k, ldk) || !in_ok(v, ldv) ||
      !in_ok(o, ldo) || !in_ok(d_o, lddo) || !lse || ((uintptr_t)lse) % 4)
    return RDEIC_EINVAL;
  if ((dk == nullptr) != (dv == nullptr) || (!dq && !dk)) return RDEIC_EINVAL;  // dK and dV come as a pair
  if ((dq && !out_ok(dq, lddq)) || (dk && (!out_ok(dk, lddk) || !out_ok(dv, lddv)))) return RDEIC_EINVAL;
  if (!ws || ((uintptr_t)ws) % 16 || ws_bytes < rdeic_attention_bwd_workspace(batch, heads, lq, lk, dh))
    return RDEIC_EINVAL;
  const BwdPlan p = bwd_plan(batch, heads, lq, lk, dh);
  hipStream_t s = (hipStream_t)stream;
  ProfScope ps(s, dh >= 64 ? RDEIC_PROF_ATTN : RDEIC_PROF_ATTN_SMALL, 10.0 * batch * heads * (double)lq * lk * dh,
               shape_key(batch, heads, lq, lk, dh));
  if (dh == 64)
    return launch_bwd<64>((const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, (const bf16*)o, ldo,
                          (const bf16*)d_o, lddo, lse, (bf16*)dq, lddq, (bf16*)dk, lddk, (bf16*)dv, lddv, (float*)ws, p,
                          batch, heads, lq, lk, scale, s);
  return launch_bwd<16>((const bf16*)q, ldq, (const bf16*)k, ldk, (const bf16*)v, ldv, (const bf16*)o, ldo,
                        (const bf16*)d_o, lddo, lse, (bf16*)dq, lddq, (bf16*)dk, lddk, (bf16*)dv, lddv, (float*)ws, p,
                        batch, heads, lq, lk, scale, s);
}
