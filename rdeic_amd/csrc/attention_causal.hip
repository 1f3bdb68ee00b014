// The two device primitives of the OpenCLIP text tower (rdeic_amd/text.py) that the rest of the library lacks:
// causal self-attention, head dim 64, and the token + positional embedding.
//
// Causal attention: softmax_{j <= i}(q_i . k_j * scale) v_j per (batch, head), the mask open_clip builds with
// build_attention_mask (upper-triangular -inf, no padding mask; ldm/modules/encoders/modules.py:216-233).
// The form is attn64_kernel's (attention.hip): S^T = K Q^T, so an MFMA output lane holds ONE query
// (lane & 15) and 4 keys; online softmax in the exp2 domain in fp32; P stays in registers as the B operand of
// O^T += V^T P^T (keys of a k-step in the MFMA's own output order); no score matrix in memory.
//
// One workgroup = 4 waves = 64 consecutive queries of one (batch, head); a wave owns 16. Key tiles are 64
// wide and aligned with the query blocks, so block x needs exactly tiles 0 .. x: tiles above the block's
// last query are neither loaded nor multiplied, tiles below its first query need no mask, and only the
// diagonal tile (and a tile that crosses l) is masked, by select, before the row max. K (row-major) and
// V^T of a tile are staged through registers into one LDS buffer, the next tile's global loads in flight
// during the current tile's math (two barriers per tile, no inline asm, no counted waits).
//
// Why the running max is finite from the first tile on: tiles run from key 0, and key 0 is visible to every
// query row (0 <= i, and 0 < l), padded rows included. So after tile 0 every lane's m is a finite score,
// exp2(m_old - m_new) is exp2(-inf - finite) = 0 there and finite - finite afterwards: never inf - inf.
//
// bf16 (dtype 1): v_mfma_f32_16x16x32_bf16, fp32 accumulation, P rounded to bf16 for the PV product (the row
// sum takes the unrounded fp32 P, as attn64_kernel). fp32 (dtype 0): v_mfma_f32_16x16x4_f32 throughout.
// A (batch, head)'s output depends on nothing but its own rows: no atomics, no split over keys, the tile
// order fixed, so runs repeat bit for bit and a row alone equals the row inside any batch.
#include "common.h"
#include "../../include/rdeic_hip.h"
#include "prof.h"

#include <type_traits>

namespace {

constexpr int AC_Q = 64;  // queries per block = keys per tile

template <typename T>
__global__ __launch_bounds__(256) void attn_causal_kernel(const T* __restrict__ q, int ldq, const T* __restrict__ k,
                                                          int ldk, const T* __restrict__ v, int ldv,
                                                          T* __restrict__ o, int ldo, int heads, int l,
                                                          float scale_log2) {
  constexpr bool BF = sizeof(T) == 2;
  constexpr int EPC = 16 / sizeof(T);     // elements per 16-byte chunk
  constexpr int ROW = 64 + EPC;           // LDS row stride of the K and V^T tiles (144 B / 272 B)
  constexpr int CPR = 64 / EPC;           // chunks per K / V row
  constexpr int NPT = 64 * CPR / 256;     // staged chunks per thread (2 / 4)
  constexpr int NQF = BF ? 2 : 16;        // Q fragments per lane
  typedef typename std::conditional<BF, bf16x8, float>::type frag_t;

  __shared__ __attribute__((aligned(16))) T Ks[64 * ROW];  // [key][d]
  __shared__ __attribute__((aligned(16))) T Vt[64 * ROW];  // [d][key]

  const int bh = blockIdx.y;
  const int b = bh / heads, h = bh - b * heads;
  const int q0 = blockIdx.x * AC_Q;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const T* qb = q + (long)b * l * ldq + h * 64;
  const T* kb = k + (long)b * l * ldk + h * 64;
  const T* vb = v + (long)b * l * ldv + h * 64;
  const int qw = q0 + wave * 16;      // this wave's first query
  const int qq = qw + lr;             // this lane's query
  const bool live = qw < l;           // wave-uniform: a wave of padding rows only stages

  // Q as the B operand: bf16 lane (query lr, g) holds d = 32 hd + 8g .. +8; fp32 d = 4s + g
  frag_t qf[NQF];
  {
    const T* qrow = qb + (long)min(qq, l - 1) * ldq;  // a valid row always; padding rows are zeroed
#pragma unroll
    for (int s = 0; s < NQF; ++s) {
      if constexpr (BF) {
        bf16x8 z = *reinterpret_cast<const bf16x8*>(qrow + 32 * s + 8 * g);
        if (qq >= l) {
#pragma unroll
          for (int e = 0; e < 8; ++e) z[e] = (bf16)0.f;
        }
        qf[s] = z;
      } else {
        qf[s] = qq < l ? qrow[4 * s + g] : 0.f;
      }
    }
  }

  // staging: K chunk c = tid + 256 j is (key c / CPR, d-chunk c % CPR). V: bf16 packs a key pair per 32-bit
  // LDS store (thread = key pair tid & 31, d-chunk tid >> 5, as attn64_kernel); fp32 uses K's assignment.
  // Loads always address a valid row (clamped); keys >= l are zeroed by value select, never read as data.
  uint4 kreg[NPT], vreg[NPT];
  auto fetch = [&](int key0) {
    const uint4 zz = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const int c = tid + 256 * j;
      const int kk = key0 + c / CPR;
      kreg[j] = *reinterpret_cast<const uint4*>(kb + (long)min(kk, l - 1) * ldk + (c % CPR) * EPC);
      if (kk >= l) kreg[j] = zz;
      const int vk = BF ? key0 + 2 * (tid & 31) + j : kk;
      const int vc = BF ? tid >> 5 : c % CPR;
      vreg[j] = *reinterpret_cast<const uint4*>(vb + (long)min(vk, l - 1) * ldv + vc * EPC);
      if (vk >= l) vreg[j] = zz;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const int c = tid + 256 * j;
      *reinterpret_cast<uint4*>(&Ks[(c / CPR) * ROW + (c % CPR) * EPC]) = kreg[j];
    }
    if constexpr (BF) {
      const int kp = tid & 31, vc = tid >> 5;
      const uint32_t wa[4] = {vreg[0].x, vreg[0].y, vreg[0].z, vreg[0].w};
      const uint32_t wb[4] = {vreg[1].x, vreg[1].y, vreg[1].z, vreg[1].w};
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        uint32_t* dst = reinterpret_cast<uint32_t*>(&Vt[(vc * 8 + 2 * w) * ROW + 2 * kp]);
        dst[0] = (wa[w] & 0xffffu) | (wb[w] << 16);                // d = 8vc + 2w: (key 2kp, 2kp + 1)
        dst[ROW / 2] = (wa[w] >> 16) | (wb[w] & 0xffff0000u);      // d = 8vc + 2w + 1
      }
    } else {
#pragma unroll
      for (int j = 0; j < NPT; ++j) {
        const int c = tid + 256 * j;
        const int kr = c / CPR, d0 = (c % CPR) * 4;
        const float ve[4] = {__uint_as_float(vreg[j].x), __uint_as_float(vreg[j].y), __uint_as_float(vreg[j].z),
                             __uint_as_float(vreg[j].w)};
#pragma unroll
        for (int e = 0; e < 4; ++e) Vt[(d0 + e) * ROW + kr] = ve[e];
      }
    }
  };

  f32x4 oacc[4];  // O^T: lane (query lr, g) holds d = 16 dt + 4g + i
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) oacc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  const int ntiles = blockIdx.x + 1;  // tile x is the diagonal one; its first key q0 < l
  fetch(0);
  for (int kt = 0; kt < ntiles; ++kt) {
    const int key0 = kt * 64;
    __syncthreads();  // every wave is done reading the previous tile
    store();
    __syncthreads();
    if (kt + 1 < ntiles) fetch(key0 + 64);
    if (!live) continue;

    // ---- S^T[key 16t + 4g + i][query lr]
    f32x4 st[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (BF) {
        const bf16* kr = &Ks[(16 * t + lr) * ROW + 8 * g];
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kr), qf[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(kr + 32), qf[1], acc, 0, 0, 0);
      } else {
        const float* kr = &Ks[(16 * t + lr) * ROW + g];
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kr[4 * s], qf[s], acc, 0, 0, 0);
      }
      st[t] = acc * scale_log2;
    }
    // ---- mask by select, before the max: only a tile that reaches past the wave's first query or past l
    if (key0 + 63 > qw || key0 + 64 > l) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = key0 + 16 * t + 4 * g + i;
          if (key > qq || key >= l) st[t][i] = -INFINITY;
        }
    }
    // ---- online softmax for the lane's query (its 16 keys here, the other 48 in lanes lr + 16 / 32 / 48)
    float mx = st[0][0];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) mx = fmaxf(mx, st[t][i]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mnew = fmaxf(m_run, mx);  // finite: see the header (key 0 is in tile 0 and masked for no row)
    const float alpha = __builtin_amdgcn_exp2f(m_run - mnew);
    m_run = mnew;
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        st[t][i] = __builtin_amdgcn_exp2f(st[t][i] - mnew);
        ps += st[t][i];
      }
    l_run = l_run * alpha + ps;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] *= alpha;

    // ---- O^T[d][query] += V^T P^T
    if constexpr (BF) {
      // k slot 8g + j of k-step c <-> key 32c + 16 (j >> 2) + 4g + (j & 3): P as the MFMA left it
      bf16x8 pf[2];
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[c][j] = (bf16)st[2 * c + (j >> 2)][j & 3];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16* vr = &Vt[(16 * dt + lr) * ROW + 4 * g];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const bf16x4 lo = *reinterpret_cast<const bf16x4*>(vr + 32 * c);
          const bf16x4 hi = *reinterpret_cast<const bf16x4*>(vr + 32 * c + 16);
          const bf16x8 vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[c], oacc[dt], 0, 0, 0);
        }
      }
    } else {
      // k slot g of k-step (t, i) <-> key 16t + 4g + i
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const f32x4 vf = *reinterpret_cast<const f32x4*>(&Vt[(16 * dt + lr) * ROW + 16 * t + 4 * g]);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[i], st[t][i], oacc[dt], 0, 0, 0);
        }
      }
    }
  }

  // ---- finalize; rows at or beyond l are never stored
  l_run += __shfl_xor(l_run, 16, 64);
  l_run += __shfl_xor(l_run, 32, 64);
  if (live && qq < l) {
    const float inv = 1.f / l_run;
    T* orow = o + ((long)b * l + qq) * ldo + h * 64;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      if constexpr (BF) {
        bf16x4 ov;
#pragma unroll
        for (int i = 0; i < 4; ++i) ov[i] = (bf16)(oacc[dt][i] * inv);
        *reinterpret_cast<bf16x4*>(orow + 16 * dt + 4 * g) = ov;
      } else {
        *reinterpret_cast<f32x4*>(orow + 16 * dt + 4 * g) = oacc[dt] * inv;
      }
    }
  }
}

// x[r][c] = token_embedding[tokens[r]][c] + positional_embedding[r % context][c], summed in fp32
template <typename T>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const float* __restrict__ table, int ld_table,
                                                           const float* __restrict__ pos, int ld_pos,
                                                           const int32_t* __restrict__ tokens, long rows, int context,
                                                           int width, T* __restrict__ out, int ld_out) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= rows * width) return;
  const long r = i / width;
  const int c = (int)(i - r * width);
  out[r * ld_out + c] = from_f32<T>(table[(long)tokens[r] * ld_table + c] + pos[(r % context) * (long)ld_pos + c]);
}

}  // namespace

extern "C" int rdeic_attention_causal(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v,
                                      int32_t ldv, void* o, int32_t ldo, int32_t batch, int32_t heads, int32_t l,
                                      int32_t dh, float scale, int32_t dtype, void* stream) {
  if (!q || !k || !v || !o || batch <= 0 || heads <= 0 || l <= 0 || dh != 64) return RDEIC_EINVAL;
  if (dtype != 0 && dtype != 1) return RDEIC_EINVAL;
  const int epc = dtype == 1 ? 8 : 4;
  if (ldq % epc || ldk % epc || ldv % epc || ((uintptr_t)k) % 16 || ((uintptr_t)v) % 16 || ((uintptr_t)q) % 16)
    return RDEIC_EINVAL;
  // the output rows are written as 4-element vectors (8 B bf16, 16 B fp32)
  if (ldo % 4 || ((uintptr_t)o) % (dtype == 1 ? 8 : 16)) return RDEIC_EINVAL;
  if ((long)batch * heads > 65535) return RDEIC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long long key = ((long long)(dh & 0xffff) << 48) | ((long long)(l < 0xffff ? l : 0xffff) << 32) |
                        ((long long)(l < 0xffff ? l : 0xffff) << 16) | (batch * heads);
  ProfScope ps(s, RDEIC_PROF_ATTN, 4.0 * batch * heads * dh * ((double)l * (l + 1) / 2), key);
  const dim3 grid((l + AC_Q - 1) / AC_Q, batch * heads);
  const float sl2 = scale * 1.4426950408889634f;
  if (dtype == 1)
    hipLaunchKernelGGL(attn_causal_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)q, ldq, (const bf16*)k, ldk,
                       (const bf16*)v, ldv, (bf16*)o, ldo, heads, l, sl2);
  else
    hipLaunchKernelGGL(attn_causal_kernel<float>, grid, dim3(256), 0, s, (const float*)q, ldq, (const float*)k, ldk,
                       (const float*)v, ldv, (float*)o, ldo, heads, l, sl2);
  return launch_status();
}

extern "C" int rdeic_embed_tokens(const float* table, int32_t ld_table, const float* pos, int32_t ld_pos,
                                  const int32_t* tokens, int32_t batch, int32_t context, int32_t width, void* out,
                                  int32_t ld_out, int32_t dtype, void* stream) {
  if (!table || !pos || !tokens || !out || batch <= 0 || context <= 0 || width <= 0 || ld_table < width ||
      ld_pos < width || ld_out < width)
    return RDEIC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)batch * context;
  const long g = (rows * width + 255) / 256;
  if (g > 0x7fffffffl) return RDEIC_EINVAL;
  if (dtype == 1)
    hipLaunchKernelGGL(embed_tokens_kernel<bf16>, dim3((unsigned)g), dim3(256), 0, s, table, ld_table, pos, ld_pos,
                       tokens, rows, context, width, (bf16*)out, ld_out);
  else
    hipLaunchKernelGGL(embed_tokens_kernel<float>, dim3((unsigned)g), dim3(256), 0, s, table, ld_table, pos, ld_pos,
                       tokens, rows, context, width, (float*)out, ld_out);
  return launch_status();
}
