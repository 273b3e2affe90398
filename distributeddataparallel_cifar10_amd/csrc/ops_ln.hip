// Row-wise kernels of the transformer path: LayerNorm fused with the residual add that feeds it, and GELU fused with
// the preamble of a GEMM layer's backward.  bf16 in and out, fp32 arithmetic, fp32 master gamma / beta (no bf16 copies).
// No float atomics anywhere; every sum has one fixed order, so two launches are bitwise equal.
//
// LayerNorm.  A row of C = 8 nch elements (64 <= C <= 2048) is nch 16-byte chunks.  It is owned by a lane group of
//   G = 8, 16, 32 or 64 lanes and lives in registers from one global read: lane j of the group holds chunks j, j + G,
//   ... (CPL of them, at most 4), so each of the CPL load instructions of a group is one contiguous 16 G byte segment.
//   G is the narrowest group that needs at most 3 chunks per lane, else 64 (ln_pick: 192 -> 8 x 3, 384 -> 16 x 3,
//   768 -> 32 x 3, 1024 -> 64 x 2, 2048 -> 64 x 4); chunks past nch (C = 200: 25 chunks on 16 x 2) are masked: loaded
//   as zero, excluded from the variance, never stored.  The kernels are instantiated on (G, CPL), so a narrow row
//   does not pay a wide row's registers.  A 256-thread workgroup holds 256 / G groups, which walk the rows with a grid
//   stride.  Sums over a row are a per-lane sum in register order, then an xor butterfly over the group's lanes (every
//   lane ends with the same bits): no LDS.
// k_ln_fwd: hsum = bf16(x + delta) (written only when delta is given; x and delta are rows of stride ldx of which the
//   first C elements are read), mean and rstd of the *rounded* hsum -- the tensor the backward rereads -- with the
//   variance as the centred second pass over the registers, y = bf16((hsum - mean) rstd gamma + beta), stats [M][2].
// k_ln_bwd: xhat from h (stride ldh) and stats; g = dy gamma, a = mean(g), b = mean(g xhat),
//   dx = bf16(rstd (g - a - xhat b) + dres): dres is the gradient arriving along the skip path, so the residual join
//   costs no pass of its own.  Each lane carries fp32 dgamma / dbeta partials of its own columns down the rows it
//   walks.  At the end the groups of a wave are combined by the butterfly continued over lane bits >= G, the 4 waves
//   through LDS ([4][2][C] floats, summed wave 0 .. 3), and the workgroup writes one slab row [2][C].  The launcher
//   caps the number of workgroups, hence slabs.
// k_ln_colsum: out[c] (+)= sum of the slab rows in slab order, a second small launch of ceil(cols / 64) workgroups.
//   A second launch instead of k_dy_prep's "last workgroup behind a ticket": the last workgroup alone would read
//   slabs x 2 C floats (4 MB at C = 2048 and 256 slabs) through one compute unit, while the launch spreads the columns
//   over 2 C / 64 workgroups and needs neither device-scope atomics nor zeroed ticket words.
// GELU, exact erf form.  k_gelu_fwd: a = bf16(gelu(z)), 16 bytes per lane.  k_gelu_bwd: dz = dy (Phi(z) + z phi(z)) as
//   the bf16 operand of the layer's two backward GEMMs, and the column sums of the unrounded fp32 dz (the bias
//   gradient): a workgroup is 32 lanes x 8 columns (512 contiguous bytes of a row) by 8 row lanes over a chunk of
//   rows; the 8 row lanes are summed through LDS in order, one partial row per chunk, then k_ln_colsum (optionally
//   accumulating into a flat gradient view).  dy is fp32 or bf16.
#pragma once
#include "ops_nn.hip"

namespace dca {
namespace ops {

constexpr int LN_NT = 256;

// group width and chunks per lane for rows of C elements
inline void ln_pick(int C, int* G, int* cpl) {
  const int nch = C >> 3;
  for (int g = 8; g <= 32; g <<= 1)
    if ((nch + g - 1) / g <= 3) {
      *G = g, *cpl = (nch + g - 1) / g;
      return;
    }
  *G = 64, *cpl = (nch + 63) / 64;
}
inline int ln_bwd_lds(int C) { return 4 * 2 * C * (int)sizeof(float); }

template <int FROM, int TO>
__device__ __forceinline__ float ln_xsum(float v) {  // xor butterfly over the lane bits FROM <= bit < TO
#pragma unroll
  for (int o = FROM; o < TO; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ void ln_ld8(const float* p, float* f) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
}

template <int G, int CPL>
__global__ void __launch_bounds__(LN_NT) k_ln_fwd(const bf16_t* __restrict__ x, const bf16_t* __restrict__ delta,
                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                  bf16_t* __restrict__ hsum, bf16_t* __restrict__ y,
                                                  float* __restrict__ stats, int M, int C, int ldx, float eps) {
  constexpr int GPW = LN_NT / G;
  const int j = threadIdx.x % G, gid = threadIdx.x / G, nch = C >> 3;
  const float inv = 1.f / (float)C;
  float ga[CPL][8], be[CPL][8];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int ch = j + k * G;
#pragma unroll
    for (int e = 0; e < 8; ++e) ga[k][e] = be[k][e] = 0.f;
    if (ch < nch) ln_ld8(gamma + 8 * ch, ga[k]), ln_ld8(beta + 8 * ch, be[k]);
  }
  for (int row = blockIdx.x * GPW + gid; row < M; row += gridDim.x * GPW) {
    const size_t in = (size_t)row * ldx, out = (size_t)row * C;
    uint4 ux[CPL], ud[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int ch = j + k * G;
      ux[k] = ud[k] = uint4{0u, 0u, 0u, 0u};
      if (ch < nch) {
        ux[k] = *(const uint4*)(x + in + 8 * ch);
        if (delta != nullptr) ud[k] = *(const uint4*)(delta + in + 8 * ch);
      }
    }
    float v[CPL][8], s = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      unpack8(ux[k], v[k]);
      if (delta != nullptr) {
        float d[8];
        unpack8(ud[k], d);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[k][e] = rbf16(v[k][e] + d[e]);
        if (j + k * G < nch) *(uint4*)(hsum + out + 8 * (j + k * G)) = pack8(v[k]);
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) s += v[k][e];
    }
    const float mean = ln_xsum<1, G>(s) * inv;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const bool live = j + k * G < nch;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[k][e] = live ? v[k][e] - mean : 0.f;
        q += v[k][e] * v[k][e];
      }
    }
    const float rstd = 1.f / sqrtf(ln_xsum<1, G>(q) * inv + eps);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      if (j + k * G >= nch) continue;
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = v[k][e] * rstd * ga[k][e] + be[k][e];
      *(uint4*)(y + out + 8 * (j + k * G)) = pack8(o);
    }
    if (j == 0) *(float2*)(stats + 2 * (size_t)row) = float2{mean, rstd};
  }
}

template <int G, int CPL>
__global__ void __launch_bounds__(LN_NT) k_ln_bwd(const bf16_t* __restrict__ h, int ldh, const bf16_t* __restrict__ dy,
                                                  const bf16_t* __restrict__ dres, const float* __restrict__ gamma,
                                                  const float* __restrict__ stats, bf16_t* __restrict__ dx,
                                                  float* __restrict__ part, int M, int C) {
  extern __shared__ float ln_red[];  // [4 waves][2][C]
  constexpr int GPW = LN_NT / G;
  const int j = threadIdx.x % G, gid = threadIdx.x / G, nch = C >> 3;
  const float inv = 1.f / (float)C;
  float ga[CPL][8], dg[CPL][8], db[CPL][8];
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
    const int ch = j + k * G;
#pragma unroll
    for (int e = 0; e < 8; ++e) ga[k][e] = dg[k][e] = db[k][e] = 0.f;
    if (ch < nch) ln_ld8(gamma + 8 * ch, ga[k]);
  }
  for (int row = blockIdx.x * GPW + gid; row < M; row += gridDim.x * GPW) {
    const size_t in = (size_t)row * ldh, out = (size_t)row * C;
    uint4 uh[CPL], uy[CPL], ur[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const int ch = j + k * G;
      uh[k] = uy[k] = ur[k] = uint4{0u, 0u, 0u, 0u};
      if (ch < nch) {
        uh[k] = *(const uint4*)(h + in + 8 * ch);
        uy[k] = *(const uint4*)(dy + out + 8 * ch);
        if (dres != nullptr) ur[k] = *(const uint4*)(dres + out + 8 * ch);
      }
    }
    const float2 st = *(const float2*)(stats + 2 * (size_t)row);  // (mean, rstd)
    float xh[CPL][8], g[CPL][8], a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {  // (a masked chunk has dy = 0: it adds nothing to any sum)
      unpack8(uh[k], xh[k]);
      unpack8(uy[k], g[k]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xh[k][e] = (xh[k][e] - st.x) * st.y;
        dg[k][e] += g[k][e] * xh[k][e];
        db[k][e] += g[k][e];
        g[k][e] *= ga[k][e];
        a += g[k][e];
        b += g[k][e] * xh[k][e];
      }
    }
    a = ln_xsum<1, G>(a) * inv;
    b = ln_xsum<1, G>(b) * inv;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      if (j + k * G >= nch) continue;
      float r[8], o[8];
      unpack8(ur[k], r);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = st.y * (g[k][e] - a - xh[k][e] * b) + r[e];
      *(uint4*)(dx + out + 8 * (j + k * G)) = pack8(o);
    }
  }
  // the groups of a wave (lane bits >= G), then the 4 waves through LDS in wave order
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < CPL; ++k) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      dg[k][e] = ln_xsum<G, 64>(dg[k][e]);
      db[k][e] = ln_xsum<G, 64>(db[k][e]);
    }
    const int ch = lane + k * G;
    if (lane < G && ch < nch) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        ln_red[(2 * wave) * C + 8 * ch + e] = dg[k][e];
        ln_red[(2 * wave + 1) * C + 8 * ch + e] = db[k][e];
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += LN_NT)
    part[(size_t)blockIdx.x * 2 * C + i] = ((ln_red[i] + ln_red[2 * C + i]) + ln_red[4 * C + i]) + ln_red[6 * C + i];
}

// out[c] (+)= part[0][c] + part[1][c] + ... (nparts rows of ncols floats): 64 columns x 4 lanes per workgroup, each
// lane a quarter of the rows in order, the quarters combined in order
__global__ void __launch_bounds__(256) k_ln_colsum(const float* __restrict__ part, int nparts, int ncols,
                                                  float* __restrict__ out, int accumulate) {
  __shared__ float red[256];
  const int t = threadIdx.x, c = blockIdx.x * 64 + (t & 63), qt = t >> 6;
  const int per = (nparts + 3) >> 2, b0 = qt * per, b1 = b0 + per < nparts ? b0 + per : nparts;
  float a = 0.f;
  if (c < ncols) {
#pragma unroll 8
    for (int b = b0; b < b1; ++b) a += part[(size_t)b * ncols + c];
  }
  red[t] = a;
  __syncthreads();
  if (t < 64 && c < ncols) {
    const float s = ((red[t] + red[t + 64]) + red[t + 128]) + red[t + 192];
    out[c] = accumulate ? out[c] + s : s;
  }
}

constexpr float GELU_RSQRT2 = 0.70710678118654752f, GELU_RSQRT2PI = 0.39894228040143268f;

__global__ void __launch_bounds__(256) k_gelu_fwd(const bf16_t* __restrict__ z, bf16_t* __restrict__ a, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float v[8];
    unpack8(*(const uint4*)(z + 8 * i), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.5f * v[e] * (1.f + erff(v[e] * GELU_RSQRT2));
    *(uint4*)(a + 8 * i) = pack8(v);
  }
}

// grid (ceil(N / 256), chunks of rpb rows); part [gridDim.y][N]
template <typename TD>
__global__ void __launch_bounds__(256) k_gelu_bwd(const TD* __restrict__ dy, const bf16_t* __restrict__ z,
                                                 bf16_t* __restrict__ dz, float* __restrict__ part, int R, int N,
                                                 int rpb) {
  __shared__ float red[8][256];
  const int t = threadIdx.x, cl = t & 31, rl = t >> 5, c0 = blockIdx.x * 256 + 8 * cl;
  const int r0 = blockIdx.y * rpb, r1 = r0 + rpb < R ? r0 + rpb : R;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (c0 < N) {
    for (int r = r0 + rl; r < r1; r += 8) {
      const size_t o = (size_t)r * N + c0;
      float d[8], v[8];
      if constexpr (sizeof(TD) == 2) unpack8(*(const uint4*)(dy + o), d);
      else ln_ld8((const float*)dy + o, d);
      unpack8(*(const uint4*)(z + o), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float cdf = 0.5f * (1.f + erff(v[e] * GELU_RSQRT2));
        d[e] *= cdf + v[e] * GELU_RSQRT2PI * __expf(-0.5f * v[e] * v[e]);
        acc[e] += d[e];
      }
      *(uint4*)(dz + o) = pack8(d);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][8 * cl + e] = acc[e];
  __syncthreads();
  const int c = blockIdx.x * 256 + t;
  if (c < N) {
    float s = red[0][t];
#pragma unroll
    for (int q = 1; q < 8; ++q) s += red[q][t];
    part[(size_t)blockIdx.y * N + c] = s;
  }
}

template <int G, int CPL>
inline hipError_t ln_fwd_launch(const void* x, const void* delta, const float* gamma, const float* beta, void* hsum,
                                void* y, float* stats, int M, int C, int ldx, float eps, int max_wg, void* stream) {
  const int gpw = LN_NT / G, grid = std::max(1, std::min((M + gpw - 1) / gpw, max_wg));
  hipLaunchKernelGGL((k_ln_fwd<G, CPL>), dim3(grid), dim3(LN_NT), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (const bf16_t*)delta, gamma, beta, (bf16_t*)hsum, (bf16_t*)y, stats, M, C, ldx, eps);
  return hipGetLastError();
}

// *slabs: in, the most workgroups; out, the workgroups launched = slab rows written
template <int G, int CPL>
inline hipError_t ln_bwd_launch(const void* h, int ldh, const void* dy, const void* dres, const float* gamma,
                                const float* stats, void* dx, float* part, int M, int C, int* slabs, void* stream) {
  const int gpw = LN_NT / G, grid = std::max(1, std::min((M + gpw - 1) / gpw, *slabs)), lds = ln_bwd_lds(C);
  if (lds > 32768) {
    const hipError_t e = hipFuncSetAttribute((const void*)k_ln_bwd<G, CPL>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_ln_bwd<G, CPL>), dim3(grid), dim3(LN_NT), lds, (hipStream_t)stream, (const bf16_t*)h, ldh,
                     (const bf16_t*)dy, (const bf16_t*)dres, gamma, stats, (bf16_t*)dx, part, M, C);
  *slabs = grid;
  return hipGetLastError();
}

// the (G, CPL) pairs ln_pick can return
#define LN_DISPATCH(G, cpl, CALL, bad)                                                              \
  switch ((G) * 8 + (cpl)) {                                                                        \
    case 8 * 8 + 1: CALL(8, 1); break;    case 8 * 8 + 2: CALL(8, 2); break;                        \
    case 8 * 8 + 3: CALL(8, 3); break;    case 16 * 8 + 2: CALL(16, 2); break;                      \
    case 16 * 8 + 3: CALL(16, 3); break;  case 32 * 8 + 2: CALL(32, 2); break;                      \
    case 32 * 8 + 3: CALL(32, 3); break;  case 64 * 8 + 2: CALL(64, 2); break;                      \
    case 64 * 8 + 3: CALL(64, 3); break;  case 64 * 8 + 4: CALL(64, 4); break;                      \
    default: bad;                                                                                   \
  }

}  // namespace ops
}  // namespace dca
