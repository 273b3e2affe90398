// Fused multi-head self-attention for short sequences: non-causal, unmasked, no dropout; head width D = 64,
// 1 <= L <= 256; bf16 operands, fp32 accumulation.  Two chained MFMA products with a row softmax between them; the
// probabilities never leave registers, and the backward recomputes them from the saved row log-sum-exp.
//
// Layouts (no transpose or split pass anywhere):
//   qkv   bf16 [B][L][3][H][64]   the [B L, 3 H 64] output of the qkv linear; row (b, l), slot s, head h is 128 bytes
//   o     bf16 [B][L][H][64]      the [B L, H 64] input of the projection linear (dout alike)
//   dqkv  bf16 [B][L][3][H][64]   every element written exactly once
//   lse   fp32 [B][H][L]          natural-log sum-exp of the scaled scores of a row
//
// Work split.  One 256-thread workgroup (4 waves) owns one (b, h); wave w owns the 16-row tiles w, w + 4, ...
// LDS.  Each operand of the head is an image [R][128 B], R = L rounded up to 32 rows (the second product consumes the
//   other side in pairs of 16-row tiles, so whole pairs are kept: at most 16 rows more than a round-up to 16), rows
//   L .. R - 1 zero, so that a zero probability never multiplies a NaN.  Rows come from global memory as 16 bytes per
//   lane, 8 lanes per 128-byte head row.  The 16-byte chunk c of row r sits at chunk position c ^ swz(r),
//   swz(r) = 2 ((r >> 1) & 3) ^ ((r >> 3) & 1): the 128-byte-row swizzle of k_wgrad_pp (the 32 lanes of one cycle of a
//   transposing read take 8 consecutive rows x 32 B: 64 distinct banks) with bit 3 of the row in chunk bit 0, which
//   also separates rows r and r + 8 of the 16-row ds_read_b128 fragment reads.  Forward: K and V (64 KB at L = 256);
//   backward: Q, K, V, dO, and per row delta and lse (130 KB at L = 256).
// Forward, k_attn_fwd.  For a query tile the wave computes the transposed score tiles S^T = K Q^T with
//   v_mfma_f32_16x16x32_bf16: keys on the M side (A fragments from the K image by ds_read_b128), queries on the N side
//   (B fragments: two 16-byte global loads per lane, kept for the tile).  Lane (g, j) then holds query j and keys
//   16 t + 4 g + e of key tile t: the whole row is resident (64 VGPRs at 256 keys), so the softmax is scale, mask keys
//   >= L to -inf, max over the registers and the 4 lane groups (ds_swizzle, ds_bpermute), exp2 with the scale folded
//   into log2(e), sum: no online rescaling.  Tiles 2 p and 2 p + 1 of a lane, rounded to bf16, are one B operand of
//   O^T = V^T P^T whose k order is keys 32 p + 4 g + e, then 32 p + 16 + 4 g + e: exactly the order in which two
//   ds_read_b64_tr_b16 of the key-major V image deliver the V^T A fragment (ops_wgrad.hip's K permutation).  1 / sum
//   is applied to the 64 x 16 fp32 output tile.  The kernel is instantiated for 3, 7 and 8 key pairs (L <= 96, 224,
//   256), so a short sequence does not pay the registers of a long one.
// Backward, k_attn_bwd.  One launch.  Prologue: the four images, delta_i = sum_d dO_i O_i (fp32, 8 lanes per row summed
//   by a fixed butterfly) and lse * log2(e) to LDS.  Phase A: a wave owns a query tile and walks the keys in pairs of
//   tiles: S^T and dP^T = V dO^T with the forward's lane map, P = exp2(S - lse), dS = P (dP - delta), dQ^T += K^T dS^T
//   (K^T by transposing reads), scale * dQ stored.  Phase B: a wave owns a key tile and walks the queries: the same code
//   with the roles swapped (S = Q K^T, dP = dO V^T; lse and delta per element instead of per lane), dV^T += dO^T P,
//   dK^T += Q^T dS, dV and scale * dK stored.  S is computed twice (two extra products of seven); in exchange every
//   output element has one owner: no atomics, no cross-wave reduction, one summation order, bitwise repeatable.
//   P and dS are rounded to bf16 where they become MFMA operands; everything else is fp32.
#pragma once
#include "ops_nn.hip"
#include "ops_wgrad.hip"

namespace dca {
namespace ops {

constexpr int AT_NT = 256, AT_ROW = 128;  // threads; bytes of a head row
constexpr float AT_LOG2E = 1.4426950408889634f, AT_LN2 = 0.6931471805599453f;

inline int at_rows(int L) { return (L + 31) & ~31; }
inline int at_fwd_lds(int L) { return 2 * at_rows(L) * AT_ROW; }
inline int at_bwd_lds(int L) { return 4 * at_rows(L) * AT_ROW + 2 * at_rows(L) * (int)sizeof(float); }

__device__ __forceinline__ int at_off(int r, int byte) {  // of byte `byte` of row r in an image
  const int swz = (2 * ((r >> 1) & 3)) ^ ((r >> 3) & 1);
  return r * AT_ROW + ((((byte >> 4) ^ swz) << 4) | (byte & 15));
}
__device__ __forceinline__ float at_x16(float x) {  // the value of lane ^ 16
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, x), 0x401F));
}
__device__ __forceinline__ float at_x32(float x) { return __shfl_xor(x, 32); }
__device__ __forceinline__ s16x8 at_ld(const char* img, int r, int byte) { return *(const s16x8*)(img + at_off(r, byte)); }
// A fragment of the transposed image: lane (g, 4 ra + rp): column 16 m + 4 ra + rp, k = rows r0 + 4 g + e, then + 16
__device__ __forceinline__ s16x8 at_ld_tr(const char* img, int row, int byte) {
  const char* p = img + at_off(row, byte);
  const s16x4 lo = lds_tr16(p), hi = lds_tr16(p + 16 * AT_ROW);  // (swz(r + 16) == swz(r))
  return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ void at_st4(bf16_t* p, const f32x4& v, float f) {
  const unsigned short h0 = f2bf_rne(v[0] * f), h1 = f2bf_rne(v[1] * f), h2 = f2bf_rne(v[2] * f), h3 = f2bf_rne(v[3] * f);
  *(uint2*)p = uint2{h0 | ((unsigned)h1 << 16), h2 | ((unsigned)h3 << 16)};
}

// Rows 0 .. R - 1 of one image from rows of `stride` elements at src; rows >= L are zero.  R * 8 is a multiple of 256.
__device__ __forceinline__ void at_stage(char* img, const bf16_t* src, size_t stride, int L, int R) {
  for (int e = threadIdx.x; e < R * 8; e += AT_NT) {
    const int r = e >> 3, ch = e & 7;
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (r < L) v = *(const uint4*)(src + (size_t)r * stride + 8 * ch);
    *(uint4*)(img + at_off(r, 16 * ch)) = v;
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_attn_fwd<NP>: o = softmax(scale q k^T) v and lse, for L <= 32 NP.  grid B * H; dynamic LDS at_fwd_lds(L).
// sl2 = scale * log2(e).
// ---------------------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(AT_NT) k_attn_fwd(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ o,
                                                    float* __restrict__ lse, int L, int H, float sl2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, g = lane >> 4;
  const int ra = j >> 2, rp = j & 3;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int np = (L + 31) >> 5, R = 32 * np, nt = (L + 15) >> 4;
  char* ks = smem;
  char* vs = smem + R * AT_ROW;
  const size_t rs = (size_t)3 * H * 64;
  const bf16_t* qb = qkv + ((size_t)b * L * 3 * H + h) * 64;
  at_stage(ks, qb + (size_t)H * 64, rs, L, R);
  at_stage(vs, qb + (size_t)2 * H * 64, rs, L, R);
  __syncthreads();
  for (int qt = w; qt < nt; qt += 4) {
    const int row = 16 * qt + j;
    s16x8 qf[2] = {s16x8{}, s16x8{}};
    if (row < L) {
      qf[0] = *(const s16x8*)(qb + (size_t)row * rs + 8 * g);
      qf[1] = *(const s16x8*)(qb + (size_t)row * rs + 32 + 8 * g);
    }
    f32x4 s[2 * NP];
    float m = -INFINITY;
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (p < np) {
#pragma unroll
        for (int t = 2 * p; t < 2 * p + 2; ++t) {
          f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_ld(ks, 16 * t + j, 64 * kk + 16 * g), qf[kk], acc, 0, 0, 0);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[e] = 16 * t + 4 * g + e < L ? acc[e] * sl2 : -INFINITY;
            m = fmaxf(m, acc[e]);
          }
          s[t] = acc;
        }
      }
    m = fmaxf(m, at_x16(m));
    m = fmaxf(m, at_x32(m));
    float sum = 0.f;
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (p < np) {
#pragma unroll
        for (int t = 2 * p; t < 2 * p + 2; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            s[t][e] = __builtin_amdgcn_exp2f(s[t][e] - m);
            sum += s[t][e];
          }
      }
    sum += at_x16(sum);
    sum += at_x32(sum);
    f32x4 acc[4];
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) acc[mm] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (p < np) {
        s16x8 pf;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pf[e] = (short)f2bf_rne(s[2 * p][e]);
          pf[4 + e] = (short)f2bf_rne(s[2 * p + 1][e]);
        }
#pragma unroll
        for (int mm = 0; mm < 4; ++mm)
          acc[mm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_ld_tr(vs, 32 * p + 4 * g + ra, 32 * mm + 8 * rp), pf,
                                                            acc[mm], 0, 0, 0);
      }
    // lane (g, j): query j, d = 16 mm + 4 g + e
    if (row < L) {
      const float inv = 1.f / sum;
      bf16_t* op = o + (((size_t)b * L + row) * H + h) * 64 + 4 * g;
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) at_st4(op + 16 * mm, acc[mm], inv);
      if (g == 0) lse[((size_t)b * H + h) * L + row] = (m + log2f(sum)) * AT_LN2;
    }
  }
}

template <int NP>
inline hipError_t at_fwd_launch(const void* qkv, void* o, float* lse, int B, int L, int H, float scale, void* stream) {
  const int lds = at_fwd_lds(L);
  const hipError_t e =
      hipFuncSetAttribute((const void*)k_attn_fwd<NP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_attn_fwd<NP>), dim3((unsigned)B * (unsigned)H), dim3(AT_NT), lds, (hipStream_t)stream,
                     (const bf16_t*)qkv, (bf16_t*)o, lse, L, H, scale * AT_LOG2E);
  return hipGetLastError();
}

// One phase of the backward over the LDS images.  KEYS = false (phase A): own = query tiles, other = keys; KEYS = true
// (phase B): own = key tiles, other = queries.  Score tile: the other side on M, so lane (g, j) holds own row j and
// other rows 16 t + 4 g + e.
template <bool KEYS>
__device__ __forceinline__ void at_bwd_phase(const char* qs, const char* ks, const char* vs, const char* dos,
                                             const float* lse2, const float* dl, bf16_t* dst, size_t rs, int L, int np,
                                             int nt, float scale, float sl2, int w, int lane) {
  const int j = lane & 15, g = lane >> 4, ra = j >> 2, rp = j & 3;
  const char* m1 = KEYS ? qs : ks;   // M side of the score product
  const char* m2 = KEYS ? dos : vs;  // M side of dP
  const char* n1 = KEYS ? ks : qs;
  const char* n2 = KEYS ? vs : dos;
  for (int ot = w; ot < nt; ot += 4) {
    const int orow = 16 * ot + j;
    s16x8 f1[2], f2[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      f1[kk] = at_ld(n1, orow, 64 * kk + 16 * g);
      f2[kk] = at_ld(n2, orow, 64 * kk + 16 * g);
    }
    const float lse_o = lse2[orow], dl_o = dl[orow];
    f32x4 acc[KEYS ? 8 : 4];
#pragma unroll
    for (int mm = 0; mm < (KEYS ? 8 : 4); ++mm) acc[mm] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < np; ++p) {
      s16x8 pf, dsf;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int t = 2 * p + hh;
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_ld(m1, 16 * t + j, 64 * kk + 16 * g), f1[kk], s, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_ld(m2, 16 * t + j, 64 * kk + 16 * g), f2[kk], dp, 0, 0, 0);
        }
        f32x4 ls = f32x4{lse_o, lse_o, lse_o, lse_o}, dd = f32x4{dl_o, dl_o, dl_o, dl_o};
        if (KEYS) {
          ls = *(const f32x4*)(lse2 + 16 * t + 4 * g);
          dd = *(const f32x4*)(dl + 16 * t + 4 * g);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {  // (rows >= L: a key is masked here, a query has lse = +inf)
          const float pe = 16 * t + 4 * g + e < L ? __builtin_amdgcn_exp2f(s[e] * sl2 - ls[e]) : 0.f;
          pf[4 * hh + e] = (short)f2bf_rne(pe);
          dsf[4 * hh + e] = (short)f2bf_rne(pe * (dp[e] - dd[e]));
        }
      }
      const int r0 = 32 * p + 4 * g + ra;
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) {
        if (KEYS) {
          acc[mm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_ld_tr(dos, r0, 32 * mm + 8 * rp), pf, acc[mm], 0, 0, 0);
          acc[4 + mm] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_ld_tr(qs, r0, 32 * mm + 8 * rp), dsf, acc[4 + mm], 0, 0, 0);
        } else {
          acc[mm] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(at_ld_tr(ks, r0, 32 * mm + 8 * rp), dsf, acc[mm], 0, 0, 0);
        }
      }
    }
    // lane (g, j): own row j, d = 16 mm + 4 g + e; dst: slot 0 of (b, 0, h)
    if (orow < L) {
      bf16_t* op = dst + (size_t)orow * rs + 4 * g;
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) {
        if (KEYS) {
          at_st4(op + 2 * (rs / 3) + 16 * mm, acc[mm], 1.f);        // dV
          at_st4(op + (rs / 3) + 16 * mm, acc[4 + mm], scale);      // dK
        } else {
          at_st4(op + 16 * mm, acc[mm], scale);                     // dQ
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_attn_bwd: dqkv from qkv, o, lse and dout.  grid B * H; dynamic LDS at_bwd_lds(L).
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(AT_NT) k_attn_bwd(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ o,
                                                    const float* __restrict__ lse, const bf16_t* __restrict__ dout,
                                                    bf16_t* __restrict__ dqkv, int L, int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const int np = (L + 31) >> 5, R = 32 * np, nt = (L + 15) >> 4;
  char* qs = smem;
  char* ks = qs + R * AT_ROW;
  char* vs = ks + R * AT_ROW;
  char* dos = vs + R * AT_ROW;
  float* lse2 = (float*)(dos + R * AT_ROW);
  float* dl = lse2 + R;
  const size_t rs = (size_t)3 * H * 64, os = (size_t)H * 64;
  const size_t qoff = ((size_t)b * L * 3 * H + h) * 64, ooff = ((size_t)b * L * H + h) * 64;
  at_stage(qs, qkv + qoff, rs, L, R);
  at_stage(ks, qkv + qoff + os, rs, L, R);
  at_stage(vs, qkv + qoff + 2 * os, rs, L, R);
  for (int e = threadIdx.x; e < R * 8; e += AT_NT) {  // dO, delta and lse; every lane of a wave takes every trip
    const int r = e >> 3, ch = e & 7;
    uint4 dv = uint4{0u, 0u, 0u, 0u}, ov = uint4{0u, 0u, 0u, 0u};
    if (r < L) {
      dv = *(const uint4*)(dout + ooff + (size_t)r * os + 8 * ch);
      ov = *(const uint4*)(o + ooff + (size_t)r * os + 8 * ch);
    }
    *(uint4*)(dos + at_off(r, 16 * ch)) = dv;
    const unsigned dw[4] = {dv.x, dv.y, dv.z, dv.w}, ow[4] = {ov.x, ov.y, ov.z, ov.w};
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      d += bf2f((unsigned short)dw[i]) * bf2f((unsigned short)ow[i]);
      d += bf2f((unsigned short)(dw[i] >> 16)) * bf2f((unsigned short)(ow[i] >> 16));
    }
    d += __shfl_xor(d, 1);
    d += __shfl_xor(d, 2);
    d += __shfl_xor(d, 4);
    if (ch == 0) dl[r] = d;
    if (ch == 1) lse2[r] = r < L ? lse[((size_t)b * H + h) * L + r] * AT_LOG2E : INFINITY;
  }
  __syncthreads();
  const float sl2 = scale * AT_LOG2E;
  at_bwd_phase<false>(qs, ks, vs, dos, lse2, dl, dqkv + qoff, rs, L, np, nt, scale, sl2, w, lane);
  at_bwd_phase<true>(qs, ks, vs, dos, lse2, dl, dqkv + qoff, rs, L, np, nt, scale, sl2, w, lane);
}

}  // namespace ops
}  // namespace dca
