// Fused NetResDeep training step for CDNA4 (gfx950 / MI355X).
//
// One training step = 23 dependent kernels (world_size 1), all captured in one hipGraph by engine.cpp:
//   k_stem_block0           : uint8 gather + normalise + conv1+bias+ReLU+maxpool (MFMA) -> x0, then trunk conv 0
//   k_fwd_block  (i=1..9)   : finalise BN(i-1) batch stats, apply BN+ReLU+residual while staging the LDS tile,
//                             trunk conv i on MFMA, per-tile BN partials (mean, M2) in the epilogue
//   k_head1                 : BN(9)+ReLU+residual, maxpool, per-tile partial fc1 (each tile owns a K-slice of W1)
//   k_head2                 : fc1 finish+ReLU, fc2, cross-entropy fwd+bwd, fc bwd to the tile's pooled features,
//                             maxpool bwd -> g10, first BN-backward partial sums
//   k_bwd_block  (i=9..0)   : BN-backward (grid-wide sums finalised in the prologue) -> dgrad conv on MFMA
//                             (+ residual), next block's BN-backward partials in the epilogue; horizontally fused
//                             extra workgroups compute the wgrad of block i+1 (or the fc1/fc2 grads for i=9);
//                             i=0 also does the stem backward and block-0 wgrad in-tile
//   k_reduce                : deterministic reduction of the wgrad partial slabs, SGD (fused at world_size 1),
//                             rebuild of the MFMA-layout weight copies, loss/cursor bookkeeping
// With world_size > 1, k_reduce only writes gradients; engine.cpp all-reduces them over RCCL (bucket A overlaps
// the trunk backward) and k_apply_sgd updates.
//
// Latency discipline: every kernel issues ALL of its global loads (tiles, BN partials, weights) before its first
// use of any of them, so a kernel pays ~one memory round trip, not one per loop iteration.
//
// Reference semantics mirrored: model/resnet.py:5-37 (weight-shared ResBlock, skip after ReLU), main.py:27-39
// (SGD lr, CrossEntropy mean), BatchNorm2d train-mode statistics and running-stat EMA applied 10x per forward.
#include "common.h"

namespace dca {

// ------------------------------------------------------------------------------------------------------------
// LDS record helpers.  A "record" is the 32 channels of one pixel (or of one weight row): 8 chunks of 16 B in
// fp32 mode, 4 chunks in bf16 mode.  Chunks are XOR-swizzled by a per-record key so that the 16-lane groups of
// ds_read_b128 (16 different pixels, same chunk) spread over all 64 banks.
// ------------------------------------------------------------------------------------------------------------
template <bool BF> struct Rec {
  static constexpr int NCH = BF ? 4 : 8;
  static constexpr int BYTES = NCH * 16;
  static constexpr int ESZ = BF ? 2 : 4;
};
template <bool BF> __device__ __forceinline__ int swz(int key) {
  if constexpr (BF) return (0x1230 >> (((key >> 2) & 3) << 2)) & 3;  // G = {0,3,2,1}
  else return key & 7;
}
template <bool BF> __device__ __forceinline__ int rec_off(int rec, int key, int chunk) {
  return ((rec * Rec<BF>::NCH) + (chunk ^ swz<BF>(key))) << 4;
}
__device__ __forceinline__ unsigned pk2(float a, float b) {
  return (unsigned)bfbits(a) | ((unsigned)bfbits(b) << 16);
}
__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// store 4 consecutive channels (4*c4 .. 4*c4+3) into a record
template <bool BF> __device__ __forceinline__ void st4_rec(char* base, int rec, int key, int c4, f32x4 v) {
  if constexpr (BF) {
    const int off = rec_off<BF>(rec, key, c4 >> 1) + ((c4 & 1) << 3);
    uint2 p;
    p.x = pk2(v.x, v.y);
    p.y = pk2(v.z, v.w);
    *(uint2*)(base + off) = p;
  } else {
    *(f32x4*)(base + rec_off<BF>(rec, key, c4)) = v;
  }
}
// store one channel into a record
template <bool BF> __device__ __forceinline__ void st1_rec(char* base, int rec, int key, int ch, float v) {
  if constexpr (BF) {
    *(unsigned short*)(base + rec_off<BF>(rec, key, ch >> 3) + ((ch & 7) << 1)) = bfbits(v);
  } else {
    *(float*)(base + rec_off<BF>(rec, key, ch >> 2) + ((ch & 3) << 2)) = v;
  }
}
// zero the 16-B chunks of `nrec` records starting at record `rec0`, every `stride` records
template <bool BF> __device__ __forceinline__ void zero_recs(char* base, int rec0, int nrec, int stride) {
  for (int idx = threadIdx.x; idx < nrec * Rec<BF>::NCH; idx += NT) {
    const int r = rec0 + (idx / Rec<BF>::NCH) * stride;
    *(uint4*)(base + ((r * Rec<BF>::NCH + idx % Rec<BF>::NCH) << 4)) = uint4{0u, 0u, 0u, 0u};
  }
}
// derived weight [9][32 out][32 in] (plain, compute type) -> swizzled LDS records (key = out).
// Split in two so the global loads can be issued together with a kernel's other prologue loads.
template <bool BF> struct WStage {
  static constexpr int N = 288 * Rec<BF>::NCH, M = (N + NT - 1) / NT;
  uint4 v[M];
};
template <bool BF> __device__ __forceinline__ void wstage_load(WStage<BF>& w, const void* src) {
  const uint4* s = (const uint4*)src;
#pragma unroll
  for (int m = 0; m < WStage<BF>::M; ++m) {
    const int idx = threadIdx.x + NT * m;
    if (idx < WStage<BF>::N) w.v[m] = s[idx];
  }
}
template <bool BF> __device__ __forceinline__ void wstage_store(const WStage<BF>& w, char* ws) {
#pragma unroll
  for (int m = 0; m < WStage<BF>::M; ++m) {
    const int idx = threadIdx.x + NT * m;
    if (idx < WStage<BF>::N) {
      const int rec = idx / Rec<BF>::NCH, ch = idx % Rec<BF>::NCH;
      *(uint4*)(ws + rec_off<BF>(rec, rec & 31, ch)) = w.v[m];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// 3x3 / pad-1 / 32->32 convolution of an R-row tile on MFMA.
//   xs: (R+2) x 18 records (halo rows/cols, zero padded), ws: 9 taps x 32 output-channel records.
//   Wave w owns output tiles t = w + 4j (row t>>1, output-channel half t&1); one 16x16 MFMA tile =
//   16 pixels of one row x 16 output channels.  acc[j][i] = out[row][pixel 4q+i][16h + (lane&15)].
// bf16: v_mfma_f32_16x16x32_bf16, one MFMA per tap (K = 32 input channels).
// fp32: v_mfma_f32_16x16x4_f32 (exact fp32), K permuted so each lane reads 4 consecutive channels with one
//       ds_read_b128 that feeds 4 MFMAs (k-slot q of step s <-> channel 16hf + 4q + s, same on A and B).
// ------------------------------------------------------------------------------------------------------------
template <bool BF, int R>
__device__ __forceinline__ void conv_core(const char* xs, const char* ws, f32x4 (&acc)[R / 2], int wave, int lane) {
  const int c = lane & 15, q = lane >> 4;
#pragma unroll
  for (int j = 0; j < R / 2; ++j) acc[j] = z4();
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int kh = tap / 3, kw = tap % 3;
#pragma unroll
    for (int j = 0; j < R / 2; ++j) {
      const int tt = wave + 4 * j, rr = tt >> 1, h = tt & 1;
      const int col = c + kw, rec = (rr + kh) * 18 + col;
      const int wrec = tap * 32 + h * 16 + c;
      if constexpr (BF) {
        const bf16x8 a = *(const bf16x8*)(xs + rec_off<BF>(rec, col, q));
        const bf16x8 b = *(const bf16x8*)(ws + rec_off<BF>(wrec, h * 16 + c, q));
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
      } else {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const f32x4 a = *(const f32x4*)(xs + rec_off<BF>(rec, col, 4 * hf + q));
          const f32x4 b = *(const f32x4*)(ws + rec_off<BF>(wrec, h * 16 + c, 4 * hf + q));
          acc[j] = mfma4(a.x, b.x, acc[j]);
          acc[j] = mfma4(a.y, b.y, acc[j]);
          acc[j] = mfma4(a.z, b.z, acc[j]);
          acc[j] = mfma4(a.w, b.w, acc[j]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// Weight-gradient GEMM of the shared trunk conv over a ROWS x 16 pixel tile:
//   dW[co][ci][tap] += sum_p dy[p][co] * x[p + off(tap)][ci]
// dyT: [32 co][DS] (pixel-contiguous), xT: [3 kw][32 ci][XS] with xT[kw][ci][r][c] = x[r-1][c+kw-1].
// 36 output tiles (2 co halves x 9 taps x 2 ci halves), 9 per wave; written as raw MFMA fragments
// (tile, lane, reg) to a private slab -> fully coalesced f32x4 stores, reduced later by k_reduce.
// ------------------------------------------------------------------------------------------------------------
template <bool BF, int ROWS>
__device__ __forceinline__ void wgrad_core(const char* dyT, int DS, const char* xT, int XS, float* slab, int wave,
                                           int lane) {
  constexpr int ESZ = Rec<BF>::ESZ;
  const int c = lane & 15, q = lane >> 4;
  f32x4 acc[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) acc[j] = z4();
  if constexpr (BF) {
#pragma unroll 2
    for (int s = 0; s < ROWS / 2; ++s) {
      const int row = 2 * s + (q >> 1), c0 = 8 * (q & 1);
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const int tt = wave + 4 * j, mt = tt & 1, nt = tt >> 1, tap = nt >> 1, cih = nt & 1;
        const int kh = tap / 3, kw = tap % 3;
        const bf16x8 a = *(const bf16x8*)(dyT + ((16 * mt + c) * DS + row * 16 + c0) * ESZ);
        const bf16x8 b = *(const bf16x8*)(xT + ((kw * 32 + 16 * cih + c) * XS + (row + kh) * 16 + c0) * ESZ);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
      }
    }
  } else {
    for (int row = 0; row < ROWS; ++row) {
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const int tt = wave + 4 * j, mt = tt & 1, nt = tt >> 1, tap = nt >> 1, cih = nt & 1;
        const int kh = tap / 3, kw = tap % 3;
        const f32x4 a = *(const f32x4*)(dyT + ((16 * mt + c) * DS + row * 16 + 4 * q) * ESZ);
        const f32x4 b = *(const f32x4*)(xT + ((kw * 32 + 16 * cih + c) * XS + (row + kh) * 16 + 4 * q) * ESZ);
        acc[j] = mfma4(a.x, b.x, acc[j]);
        acc[j] = mfma4(a.y, b.y, acc[j]);
        acc[j] = mfma4(a.z, b.z, acc[j]);
        acc[j] = mfma4(a.w, b.w, acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) st4(slab + (((wave + 4 * j) * 64 + lane) << 2), acc[j]);
}

// ------------------------------------------------------------------------------------------------------------
// BatchNorm statistics (deterministic, fixed order).  A block's per-tile partials are float2 per channel; thread t
// owns float4 #(t + 256 m) = channels 2(t&15), 2(t&15)+1 of tile (t>>4) + 16 m.  parts_load issues the loads
// (in flight together with the kernel's other prologue loads), *_finish consumes them.
// ------------------------------------------------------------------------------------------------------------
struct Parts {
  f32x4 v[8];
};
__device__ __forceinline__ void parts_load(Parts& P, const float2* part, int nparts) {
  const f32x4* p4 = (const f32x4*)part;
  const int n4 = nparts * 16;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int idx = threadIdx.x + NT * m;
    P.v[m] = idx < n4 ? p4[idx] : z4();
  }
}
// forward: per-tile (mean m_w, M2_w) over `cnt` pixels each -> batch mean and biased variance.
// Division-free single pass with a per-channel shift K = m_0 (tile 0's mean, loaded by every thread):
//   S1 = sum (m_w - K), S2 = sum (m_w - K)^2, Q = sum M2_w
//   mean = K + S1/n,  M2 = Q + cnt * (S2 - S1^2/n)          (n = nparts; exact algebra, no cancellation
// beyond the spread of the tile means around K).  red: RED_F floats.
__device__ void fstats_finish(const Parts& P, const float2* part, int nparts, float cnt, float* red, float* s_mean,
                              float* s_var) {
  const int t = threadIdx.x, grp = t >> 4, cp = t & 15;
  const int n4 = nparts * 16;
  const f32x4* p4 = (const f32x4*)part;
  const f32x4 k4 = p4[cp];  // tile 0, channels 2cp, 2cp+1 (same lines as thread cp's first load)
  float s10 = 0.f, s20 = 0.f, q0 = 0.f, s11 = 0.f, s21 = 0.f, q1 = 0.f;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    if (t + NT * m < n4) {
      const float d0 = P.v[m].x - k4.x, d1 = P.v[m].z - k4.z;
      s10 += d0;
      s20 += d0 * d0;
      q0 += P.v[m].y;
      s11 += d1;
      s21 += d1 * d1;
      q1 += P.v[m].w;
    }
  }
  for (int idx = 8 * NT + t; idx < n4; idx += NT) {  // more than 128 tiles (batch > 32): rare slow path
    const f32x4 v = p4[idx];
    const float d0 = v.x - k4.x, d1 = v.z - k4.z;
    s10 += d0;
    s20 += d0 * d0;
    q0 += v.y;
    s11 += d1;
    s21 += d1 * d1;
    q1 += v.w;
  }
  red[grp * 32 + 2 * cp] = s10;
  red[grp * 32 + 2 * cp + 1] = s11;
  red[512 + grp * 32 + 2 * cp] = s20;
  red[512 + grp * 32 + 2 * cp + 1] = s21;
  red[1024 + grp * 32 + 2 * cp] = q0;
  red[1024 + grp * 32 + 2 * cp + 1] = q1;
  if (t < 16) {
    red[1536 + 2 * t] = k4.x;  // shifts for the finishing threads
    red[1536 + 2 * t + 1] = k4.z;
  }
  __syncthreads();
  if (t < 32) {
    float s1 = 0.f, s2 = 0.f, q = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      s1 += red[g * 32 + t];
      s2 += red[512 + g * 32 + t];
      q += red[1024 + g * 32 + t];
    }
    const float inv_n = 1.f / (float)nparts;
    const float m2 = q + cnt * (s2 - s1 * s1 * inv_n);
    s_mean[t] = red[1536 + t] + s1 * inv_n;
    s_var[t] = fmaxf(m2, 0.f) * inv_n / cnt;
  }
  __syncthreads();
}
// backward: per-tile (sum dz, sum dz*xhat) -> totals.  red: 1024 floats.
__device__ void bsums_finish(const Parts& P, const float2* part, int nparts, float* red, float* s_a, float* s_b) {
  const int t = threadIdx.x, grp = t >> 4, cp = t & 15;
  const int n4 = nparts * 16;
  float a0 = 0.f, b0 = 0.f, a1 = 0.f, b1 = 0.f;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    if (t + NT * m < n4) {
      a0 += P.v[m].x;
      b0 += P.v[m].y;
      a1 += P.v[m].z;
      b1 += P.v[m].w;
    }
  }
  const f32x4* p4 = (const f32x4*)part;
  for (int idx = 8 * NT + t; idx < n4; idx += NT) {
    const f32x4 v = p4[idx];
    a0 += v.x;
    b0 += v.y;
    a1 += v.z;
    b1 += v.w;
  }
  red[grp * 32 + 2 * cp] = a0;
  red[grp * 32 + 2 * cp + 1] = a1;
  red[512 + grp * 32 + 2 * cp] = b0;
  red[512 + grp * 32 + 2 * cp + 1] = b1;
  __syncthreads();
  if (t < 32) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      a += red[g * 32 + t];
      b += red[512 + g * 32 + t];
    }
    s_a[t] = a;
    s_b[t] = b;
  }
  __syncthreads();
}
// running-stat EMA of one BN application (reference: nn.BatchNorm2d momentum 0.1, unbiased running_var)
__device__ __forceinline__ void bn_running_update(const Ctx& cx, int t, float mean, float var_b, bool from_base) {
  const float ntot = (float)cx.B * 256.f;
  const float unb = var_b * ntot / (ntot - 1.f);
  const float rm0 = from_base ? cx.rs_base[t] : cx.rm[t];
  const float rv0 = from_base ? cx.rs_base[32 + t] : cx.rv[t];
  const float m = cx.bn_mom;
  cx.rm[t] = rm0 * (1.f - m) + mean * m;
  cx.rv[t] = rv0 * (1.f - m) + unb * m;
}

// forward epilogue: store y tile, per-tile BN partials (mean, M2) for this tile's R*16 pixels
template <int R>
__device__ __forceinline__ void fwd_epilogue(const f32x4 (&acc)[R / 2], float* ytile, float2* part, float* red,
                                             float* s_tmp, int wave, int lane) {
  const int t = threadIdx.x, c = lane & 15, q = lane >> 4;
#pragma unroll
  for (int j = 0; j < R / 2; ++j) {
    const int tt = wave + 4 * j, rr = tt >> 1, ch = 16 * (tt & 1) + c;
    float* yp = ytile + (rr * 16 + 4 * q) * 32 + ch;
    yp[0] = acc[j].x;
    yp[32] = acc[j].y;
    yp[64] = acc[j].z;
    yp[96] = acc[j].w;
    float s = acc[j].x + acc[j].y + acc[j].z + acc[j].w;
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (q == 0) red[tt * 16 + c] = s;
  }
  __syncthreads();
  if (t < 32) {
    const int h = t >> 4, cc = t & 15;
    float s = 0.f;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) s += red[(rr * 2 + h) * 16 + cc];
    s_tmp[t] = s / (float)(R * 16);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < R / 2; ++j) {
    const int tt = wave + 4 * j, ch = 16 * (tt & 1) + c;
    const float m = s_tmp[ch];
    const float d0 = acc[j].x - m, d1 = acc[j].y - m, d2 = acc[j].z - m, d3 = acc[j].w - m;
    float s = d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (q == 0) red[tt * 16 + c] = s;
  }
  __syncthreads();
  if (t < 32) {
    const int h = t >> 4, cc = t & 15;
    float s = 0.f;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) s += red[(rr * 2 + h) * 16 + cc];
    part[t] = make_float2(s_tmp[t], s);
  }
}

__device__ __forceinline__ size_t act_off(int blk, int B) { return (size_t)blk * B * 8192; }

// normalise one CIFAR byte (ToTensor + Normalize, reference main.py:55-57)
__device__ __forceinline__ float norm_px(unsigned byte, int ch) {
  const float mean = ch == 0 ? 0.4915f : (ch == 1 ? 0.4823f : 0.4468f);
  const float stdv = ch == 0 ? 0.2470f : (ch == 1 ? 0.2435f : 0.2616f);
  return ((float)byte / 255.f - mean) / stdv;
}
// Stage NROWS input rows (image rows y0 .. y0+NROWS-1, zero outside [0,32)) of the 3 channels into an LDS
// float tile [3][NROWS][34] with zero pad columns 0 and 33.  Loads are 4-byte words, all issued up front.
template <int NROWS>
struct InRows {
  static constexpr int NW = 3 * NROWS * 8, M = (NW + NT - 1) / NT;
  unsigned w[M];
};
template <int NROWS>
__device__ __forceinline__ void inrows_load(InRows<NROWS>& I, const uint8_t* img, int y0) {
  const unsigned* s = (const unsigned*)img;
#pragma unroll
  for (int m = 0; m < InRows<NROWS>::M; ++m) {
    const int idx = threadIdx.x + NT * m;
    const int ch = idx / (NROWS * 8), ir = (idx >> 3) % NROWS, wd = idx & 7, y = y0 + ir;
    I.w[m] = (idx < InRows<NROWS>::NW && y >= 0 && y < 32) ? s[(ch * 1024 + y * 32) / 4 + wd] : 0u;
  }
}
template <int NROWS>
__device__ __forceinline__ void inrows_store(const InRows<NROWS>& I, float* xin, int y0) {
  constexpr int IW = 34;
  for (int idx = threadIdx.x; idx < 3 * NROWS * 2; idx += NT) xin[(idx >> 1) * IW + (idx & 1) * 33] = 0.f;
#pragma unroll
  for (int m = 0; m < InRows<NROWS>::M; ++m) {
    const int idx = threadIdx.x + NT * m;
    if (idx >= InRows<NROWS>::NW) continue;
    const int ch = idx / (NROWS * 8), ir = (idx >> 3) % NROWS, wd = idx & 7, y = y0 + ir;
    const bool v = y >= 0 && y < 32;
    float* dst = xin + (ch * NROWS + ir) * IW + 1 + 4 * wd;
#pragma unroll
    for (int b = 0; b < 4; ++b) dst[b] = v ? norm_px((I.w[m] >> (8 * b)) & 255u, ch) : 0.f;
  }
}

// ============================================================================================================
// Forward, block 0: stem (gather+normalise+conv1+bias+ReLU+maxpool) fused with the first trunk conv.
// ============================================================================================================
template <bool BF, int R>
__global__ void __launch_bounds__(NT) k_stem_block0(Ctx cx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int RR = R + 2, IR = 2 * RR + 2, IW = 34, RB = Rec<BF>::BYTES, TPI = 16 / R;
  using TA = typename std::conditional<BF, unsigned short, float>::type;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, c = lane & 15, q = lane >> 4;
  const int wg = blockIdx.x, n = wg / TPI, r0 = (wg % TPI) * R;
  char* ws = smem;
  char* xs = ws + 288 * RB;
  float* xin = (float*)(xs + RR * 18 * RB);   // [3][IR][IW]
  TA* swl = (TA*)(xin + 3 * IR * IW);         // [32][32]
  float* s_bias = (float*)(swl + 32 * 32);
  float* red = s_bias + 32;
  float* s_tmp = red + RED_F;
  DCA_STAMP(cx, 0, wg, 0);

  // ---- issue every global load ----
  InRows<IR> I;
  inrows_load<IR>(I, cx.data + (size_t)sample_id(cx, n) * 3072, 2 * r0 - 3);
  WStage<BF> W;
  wstage_load<BF>(W, cx.wt_f);
  constexpr int NSW = 32 * 32 * (int)sizeof(TA) / 16;
  uint4 swv = uint4{0u, 0u, 0u, 0u};
  if (t < NSW) swv = ((const uint4*)cx.sw)[t];
  const float bias_v = t < 32 ? cx.params[OFF_C1B + t] : 0.f;
  // ---- LDS fills ----
  inrows_store<IR>(I, xin, 2 * r0 - 3);
  wstage_store<BF>(W, ws);
  if (t < NSW) ((uint4*)swl)[t] = swv;
  if (t < 32) s_bias[t] = bias_v;
  zero_recs<BF>(xs, 0, RR, 18);
  zero_recs<BF>(xs, 17, RR, 18);
  __syncthreads();
  DCA_STAMP(cx, 0, wg, 1);

  // per-lane im2col offsets (k = ci*9 + kh*3 + kw)
  constexpr int NK = BF ? 8 : 7;
  int koff[NK];
  bool kval[NK];
#pragma unroll
  for (int s = 0; s < NK; ++s) {
    const int k = BF ? 8 * q + s : 4 * s + q;
    kval[s] = k < 27;
    const int ci = k / 9, kh = (k % 9) / 3, kw = k % 3;
    koff[s] = kval[s] ? ci * IR * IW + kh * IW + kw : 0;
  }
  float* X0 = cx.X + (size_t)n * 8192;
  uint8_t* code_out = cx.SCODE + (size_t)n * 8192;
  for (int u = wave; u < 4 * RR; u += 4) {
    const int prl = u >> 2, chalf = (u >> 1) & 1, h = u & 1;
    const int co = 16 * h + c;
    const int base0 = (2 * prl) * IW + 16 * chalf + c;
    f32x4 a0 = z4(), a1 = z4();
    if constexpr (BF) {
      const bf16x8 b = *(const bf16x8*)(swl + co * 32 + 8 * q);
      bf16x8 v0, v1;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        v0[s] = (__bf16)(kval[s] ? xin[koff[s] + base0] : 0.f);
        v1[s] = (__bf16)(kval[s] ? xin[koff[s] + base0 + IW] : 0.f);
      }
      a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v0, b, a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(v1, b, a1, 0, 0, 0);
    } else {
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        const float bw = kval[s] ? swl[co * 32 + 4 * s + q] : 0.f;
        const float v0 = kval[s] ? xin[koff[s] + base0] : 0.f;
        const float v1 = kval[s] ? xin[koff[s] + base0 + IW] : 0.f;
        a0 = mfma4(v0, bw, a0);
        a1 = mfma4(v1, bw, a1);
      }
    }
    const float bias = s_bias[co];
    const int pr_img = r0 - 1 + prl;
    const bool rvalid = pr_img >= 0 && pr_img < 16;
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      const float v00 = fmaxf(a0[2 * pp] + bias, 0.f), v01 = fmaxf(a0[2 * pp + 1] + bias, 0.f);
      const float v10 = fmaxf(a1[2 * pp] + bias, 0.f), v11 = fmaxf(a1[2 * pp + 1] + bias, 0.f);
      float best = v00;
      int code = 0;
      if (v01 > best) { best = v01; code = 1; }
      if (v10 > best) { best = v10; code = 2; }
      if (v11 > best) { best = v11; code = 3; }
      if (best > 0.f) code |= 4;
      const int pc = 8 * chalf + 2 * q + pp;
      st1_rec<BF>(xs, prl * 18 + pc + 1, pc + 1, co, rvalid ? best : 0.f);
      if (prl >= 1 && prl <= R) {
        X0[(pr_img * 16 + pc) * 32 + co] = best;
        code_out[(pr_img * 16 + pc) * 32 + co] = (uint8_t)code;
      }
    }
  }
  __syncthreads();
  DCA_STAMP(cx, 0, wg, 3);
  f32x4 acc[R / 2];
  conv_core<BF, R>(xs, ws, acc, wave, lane);
  DCA_STAMP(cx, 0, wg, 4);
  fwd_epilogue<R>(acc, cx.Y + (size_t)n * 8192 + r0 * 512, cx.FPART + (size_t)wg * 32, red, s_tmp, wave, lane);
  DCA_STAMP(cx, 0, wg, 5);
}

// ============================================================================================================
// Forward, blocks 1..9: x_i = relu(BN(y_{i-1})) + x_{i-1} staged into LDS, then y_i = conv(x_i).
// ============================================================================================================
template <bool BF, int R>
__global__ void __launch_bounds__(NT) k_fwd_block(Ctx cx, int i) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int RR = R + 2, TPI = 16 / R, NF = RR * 128 / NT, RB = Rec<BF>::BYTES;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int wg = blockIdx.x, n = wg / TPI, r0 = (wg % TPI) * R;
  const int nparts = cx.B * TPI;
  char* ws = smem;
  char* xs = ws + 288 * RB;
  float* red = (float*)(xs + RR * 18 * RB);
  float* s_mean = red + RED_F;
  float* s_var = s_mean + 32;
  float* s_scale = s_var + 32;
  float* s_shift = s_scale + 32;
  DCA_STAMP(cx, i, wg, 0);

  // ---- issue every global load ----
  const float* Yp = cx.Y + act_off(i - 1, cx.B) + (size_t)n * 8192;
  const float* Xp = cx.X + act_off(i - 1, cx.B) + (size_t)n * 8192;
  f32x4 yv[NF], xv[NF];
#pragma unroll
  for (int m = 0; m < NF; ++m) {
    const int f = t + NT * m, tr = f >> 7, col = (f >> 3) & 15, c4 = f & 7, row = r0 - 1 + tr;
    if (row >= 0 && row < 16) {
      const int off = (row * 16 + col) * 32 + 4 * c4;
      yv[m] = ld4(Yp + off);
      xv[m] = ld4(Xp + off);
    } else {
      yv[m] = z4();
      xv[m] = z4();
    }
  }
  const float2* fpart = cx.FPART + (size_t)(i - 1) * cx.pstride * 32;
  Parts P;
  parts_load(P, fpart, nparts);
  WStage<BF> W;
  wstage_load<BF>(W, cx.wt_f);
  const float gam = t < 32 ? cx.params[OFF_BNW + t] : 0.f, bet = t < 32 ? cx.params[OFF_BNB + t] : 0.f;
  // ---- use ----
  wstage_store<BF>(W, ws);
  DCA_STAMP(cx, i, wg, 1);
  zero_recs<BF>(xs, 0, RR, 18);
  zero_recs<BF>(xs, 17, RR, 18);
  fstats_finish(P, fpart, nparts, (float)(R * 16), red, s_mean, s_var);
  DCA_STAMP(cx, i, wg, 2);
  if (t < 32) {
    const float mean = s_mean[t], var = s_var[t], invstd = rsqrtf(var + cx.bn_eps);
    s_scale[t] = gam * invstd;
    s_shift[t] = bet - mean * gam * invstd;
    if (wg == 0) {
      cx.STATS[(i - 1) * 32 + t] = make_float2(mean, invstd);
      bn_running_update(cx, t, mean, var, (i == 1) && cx.ws > 1);
      if (t == 0) *cx.nbt += 1;
    }
  }
  __syncthreads();
  float* Xo = cx.X + act_off(i, cx.B) + (size_t)n * 8192;
#pragma unroll
  for (int m = 0; m < NF; ++m) {
    const int f = t + NT * m, tr = f >> 7, col = (f >> 3) & 15, c4 = f & 7, row = r0 - 1 + tr;
    f32x4 xn = z4();
    if (row >= 0 && row < 16) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = 4 * c4 + e;
        xn[e] = fmaxf(yv[m][e] * s_scale[ch] + s_shift[ch], 0.f) + xv[m][e];
      }
      if (tr >= 1 && tr <= R) st4(Xo + (row * 16 + col) * 32 + 4 * c4, xn);
    }
    st4_rec<BF>(xs, tr * 18 + col + 1, col + 1, c4, xn);
  }
  __syncthreads();
  DCA_STAMP(cx, i, wg, 3);
  f32x4 acc[R / 2];
  conv_core<BF, R>(xs, ws, acc, wave, lane);
  DCA_STAMP(cx, i, wg, 4);
  fwd_epilogue<R>(acc, cx.Y + act_off(i, cx.B) + (size_t)n * 8192 + r0 * 512,
                  cx.FPART + ((size_t)i * cx.pstride + wg) * 32, red, s_mean, wave, lane);
  DCA_STAMP(cx, i, wg, 5);
}

// ============================================================================================================
// Head, part 1 (one workgroup per trunk tile = R/2 pooled rows of one image):
//   x10 = relu(BN9(y9)) + x9 -> 2x2 max-pool -> partial fc1 over this tile's 128R pooled features.
// Each tile reads only its K-slice of W1 (16R KB), so W1 is streamed by B*TPI CUs instead of re-read by B.
// ============================================================================================================
template <int R>
__global__ void __launch_bounds__(NT) k_head1(Ctx cx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TPI = 16 / R, NO = R / 2, F4 = 4 * R;  // F4: pooled features per channel in this tile
  const int t = threadIdx.x;
  const int wg = blockIdx.x, n = wg / TPI, r0 = (wg % TPI) * R;
  const int nparts = cx.B * TPI;
  float* x10 = (float*)smem;       // [16R px][32]
  float* Ps = x10 + R * 512;       // [32 ch][4R]
  float* red = Ps + 128 * R;
  float* s_mean = red + RED_F;
  float* s_var = s_mean + 32;
  float* s_scale = s_var + 32;
  float* s_shift = s_scale + 32;
  DCA_STAMP(cx, 10, wg, 0);

  const size_t toff = act_off(9, cx.B) + (size_t)n * 8192 + r0 * 512;
  f32x4 yv[NO], xv[NO];
#pragma unroll
  for (int m = 0; m < NO; ++m) {
    yv[m] = ld4(cx.Y + toff + 4 * (t + NT * m));
    xv[m] = ld4(cx.X + toff + 4 * (t + NT * m));
  }
  const float2* fpart = cx.FPART + (size_t)9 * cx.pstride * 32;
  Parts P;
  parts_load(P, fpart, nparts);
  const int j = t >> 3, s8 = t & 7;
  f32x4 w1v[4 * R];
#pragma unroll
  for (int cc = 0; cc < 4; ++cc)
#pragma unroll
    for (int r = 0; r < R; ++r)
      w1v[cc * R + r] = ld4(cx.params + OFF_FC1W + j * 2048 + (4 * s8 + cc) * 64 + 4 * r0 + 4 * r);
  const float gam = t < 32 ? cx.params[OFF_BNW + t] : 0.f, bet = t < 32 ? cx.params[OFF_BNB + t] : 0.f;

  fstats_finish(P, fpart, nparts, (float)(R * 16), red, s_mean, s_var);
  if (t < 32) {
    const float mean = s_mean[t], var = s_var[t], invstd = rsqrtf(var + cx.bn_eps);
    s_scale[t] = gam * invstd;
    s_shift[t] = bet - mean * gam * invstd;
    if (wg == 0) {
      cx.STATS[9 * 32 + t] = make_float2(mean, invstd);
      bn_running_update(cx, t, mean, var, false);
      if (t == 0) *cx.nbt += 1;
    }
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NO; ++m) {
    const int f = t + NT * m, c4 = f & 7;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaxf(yv[m][e] * s_scale[4 * c4 + e] + s_shift[4 * c4 + e], 0.f) + xv[m][e];
    st4(x10 + 4 * f, o);
  }
  __syncthreads();
  // 2x2 max-pool, first-max tie break (PyTorch scan order); NCHW-flatten index c*64 + ph*8 + pw
#pragma unroll
  for (int m = 0; m < NO; ++m) {
    const int o = t + NT * m, ch = o & 31, pp = o >> 5, pr = pp >> 3, pw = pp & 7;
    const int p00 = ((2 * pr) * 16 + 2 * pw) * 32 + ch;
    const float v00 = x10[p00], v01 = x10[p00 + 32], v10 = x10[p00 + 512], v11 = x10[p00 + 544];
    float best = v00;
    int id = 0;
    if (v01 > best) { best = v01; id = 1; }
    if (v10 > best) { best = v10; id = 2; }
    if (v11 > best) { best = v11; id = 3; }
    Ps[ch * F4 + pp] = best;
    cx.HCODE[(size_t)n * 2048 + ((r0 / 2) * 8 + pp) * 32 + ch] = (uint8_t)id;
    cx.HP[(size_t)n * 2048 + ch * 64 + (r0 / 2) * 8 + pp] = best;
  }
  __syncthreads();
  float acc = 0.f;
#pragma unroll
  for (int cc = 0; cc < 4; ++cc)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const f32x4 p4 = ld4(Ps + (4 * s8 + cc) * F4 + 4 * r);
      const f32x4 w4 = w1v[cc * R + r];
      acc += w4.x * p4.x + w4.y * p4.y + w4.z * p4.z + w4.w * p4.w;
    }
  acc += __shfl_xor(acc, 1);
  acc += __shfl_xor(acc, 2);
  acc += __shfl_xor(acc, 4);
  if (s8 == 0) cx.HPART[(size_t)wg * 32 + j] = acc;
  DCA_STAMP(cx, 10, wg, 5);
}

// ============================================================================================================
// Head, part 2 (same tiling): fc1 finish + ReLU, fc2, cross-entropy fwd/bwd, dh, dp = W1_slice^T dh,
// max-pool backward -> g10 (own rows), dz9 = g10*[z9>0] and the tile's BN-backward partial sums.
// ============================================================================================================
template <int R>
__global__ void __launch_bounds__(NT) k_head2(Ctx cx) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TPI = 16 / R, NO = R / 2, F4 = 4 * R, U = R / 2;  // U: pooled features per thread
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wg = blockIdx.x, n = wg / TPI, r0 = (wg % TPI) * R;
  float* s_hp = (float*)smem;      // [TPI][32]
  float* s_w2 = s_hp + 256;        // [10][32]
  float* s_h = s_w2 + 320;         // [32]
  float* s_dh = s_h + 32;          // [32]
  float* s_lg = s_dh + 32;         // [16]
  float* s_dl = s_lg + 16;         // [16]
  uint8_t* s_code = (uint8_t*)(s_dl + 16);  // [4R pooled px][32]
  float* s_dp = (float*)(s_code + 128 * R); // [32 ch][4R]
  float* red = s_dp + 128 * R;
  float* s_mean = red + RED_F;
  float* s_inv = s_mean + 32;
  float* s_scale = s_inv + 32;
  float* s_shift = s_scale + 32;
  DCA_STAMP(cx, 11, wg, 0);

  // ---- issue every global load ----
  const float hp = t < TPI * 32 ? cx.HPART[(size_t)n * TPI * 32 + t] : 0.f;
  const f32x4 w2v = t < 80 ? ld4(cx.params + OFF_FC2W + 4 * t) : z4();
  const float b1 = t < 32 ? cx.params[OFF_FC1B + t] : 0.f;
  const float b2 = t < 10 ? cx.params[OFF_FC2B + t] : 0.f;
  const int label = t == 0 ? cx.labels[sample_id(cx, n)] : 0;
  const unsigned codew = t < 32 * R ? ((const unsigned*)(cx.HCODE + (size_t)n * 2048 + (r0 / 2) * 256))[t] : 0u;
  const size_t toff = act_off(9, cx.B) + (size_t)n * 8192 + r0 * 512;
  f32x4 yv[NO];
#pragma unroll
  for (int m = 0; m < NO; ++m) yv[m] = ld4(cx.Y + toff + 4 * (t + NT * m));
  const float2 st = t < 32 ? cx.STATS[9 * 32 + t] : make_float2(0.f, 0.f);
  const float gam = t < 32 ? cx.params[OFF_BNW + t] : 0.f, bet = t < 32 ? cx.params[OFF_BNB + t] : 0.f;
  const int u0 = t * U, cu = u0 / F4, vu = u0 % F4;
  const float* w1p = cx.params + OFF_FC1W + cu * 64 + 4 * r0 + vu;
  float w1v[32][U];
#pragma unroll
  for (int jj = 0; jj < 32; ++jj)
#pragma unroll
    for (int uu = 0; uu < U; ++uu) w1v[jj][uu] = w1p[jj * 2048 + uu];
  // ---- use ----
  s_hp[t] = hp;
  if (t < 80) st4(s_w2 + 4 * t, w2v);
  if (t < 32 * R) ((unsigned*)s_code)[t] = codew;
  if (t < 32) {
    s_mean[t] = st.x;
    s_inv[t] = st.y;
    s_scale[t] = gam * st.y;
    s_shift[t] = bet - st.x * gam * st.y;
  }
  __syncthreads();
  if (t < 32) {
    float h = b1;
#pragma unroll
    for (int k = 0; k < TPI; ++k) h += s_hp[k * 32 + t];
    s_h[t] = h;
  }
  __syncthreads();
  if (t < 10) {
    float s = b2;
#pragma unroll 8
    for (int jj = 0; jj < 32; ++jj) s += s_w2[t * 32 + jj] * fmaxf(s_h[jj], 0.f);
    s_lg[t] = s;
  }
  __syncthreads();
  const bool lead = (wg % TPI) == 0;
  if (t == 0) {
    float mx = s_lg[0];
    for (int o = 1; o < 10; ++o) mx = fmaxf(mx, s_lg[o]);
    float se = 0.f;
    for (int o = 0; o < 10; ++o) se += expf(s_lg[o] - mx);
    const float lse = mx + logf(se);
    if (lead) cx.HLOSS[n] = lse - s_lg[label];
    const float invB = 1.f / (float)cx.B;
    for (int o = 0; o < 10; ++o) s_dl[o] = (expf(s_lg[o] - lse) - (o == label ? 1.f : 0.f)) * invB;
  }
  __syncthreads();
  if (t < 32) {
    float s = 0.f;
#pragma unroll
    for (int o = 0; o < 10; ++o) s += s_w2[o * 32 + t] * s_dl[o];
    const float h = s_h[t];
    const float dh = h > 0.f ? s : 0.f;
    s_dh[t] = dh;
    if (lead) {
      cx.HDH[n * 32 + t] = dh;
      cx.HH[n * 32 + t] = fmaxf(h, 0.f);
      if (t < 10) cx.HDL[n * 10 + t] = s_dl[t];
    }
  }
  __syncthreads();
#pragma unroll
  for (int uu = 0; uu < U; ++uu) {
    float s = 0.f;
#pragma unroll
    for (int jj = 0; jj < 32; ++jj) s += w1v[jj][uu] * s_dh[jj];
    s_dp[u0 + uu] = s;
  }
  __syncthreads();
  float* G0 = cx.G + (size_t)n * 8192 + r0 * 512;  // ping-pong slot 0 holds g10
  f32x4 sa = z4(), sb = z4();
#pragma unroll
  for (int m = 0; m < NO; ++m) {
    const int f = t + NT * m, p = f >> 3, c4 = f & 7, lr = p >> 4, col = p & 15;
    const int pp = (lr >> 1) * 8 + (col >> 1), pos = (lr & 1) * 2 + (col & 1);
    f32x4 g;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ch = 4 * c4 + e;
      g[e] = (s_code[pp * 32 + ch] == pos) ? s_dp[ch * F4 + pp] : 0.f;
      const float y = yv[m][e];
      const float z = y * s_scale[ch] + s_shift[ch];
      const float dz = z > 0.f ? g[e] : 0.f;
      sa[e] += dz;
      sb[e] += dz * (y - s_mean[ch]) * s_inv[ch];
    }
    st4(G0 + 4 * f, g);
  }
  // reduce over the threads sharing channel group c4 = t & 7
#pragma unroll
  for (int o = 8; o <= 32; o <<= 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sa[e] += __shfl_xor(sa[e], o);
      sb[e] += __shfl_xor(sb[e], o);
    }
  }
  if (lane < 8) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[wave * 32 + 4 * lane + e] = sa[e];
      red[128 + wave * 32 + 4 * lane + e] = sb[e];
    }
  }
  __syncthreads();
  if (t < 32) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      a += red[w * 32 + t];
      b += red[128 + w * 32 + t];
    }
    cx.BPART[(size_t)wg * 32 + t] = make_float2(a, b);
  }
  DCA_STAMP(cx, 11, wg, 5);
}

// ============================================================================================================
// Backward workgroup roles
// ============================================================================================================
// fc1/fc2 weight gradients from the head's saved per-image vectors (sum over the batch, fixed order).
// Workgroup f owns fc1 columns 64f .. 64f+63; the batch vectors are staged in LDS with one load round trip.
__device__ void fc_grads_role(const Ctx& cx, int f, char* smem) {
  const int t = threadIdx.x, B = cx.B;
  float* dh_s = (float*)smem;   // [B][32]
  float* p_s = dh_s + 64 * 32;  // [B][64]
  float* hh_s = p_s + 64 * 64;  // [B][32]
  float* dl_s = hh_s + 64 * 32; // [B][16]
  f32x4 dh4[2], p4[4], hh4[2];
  float dlv[3];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int idx = t + NT * m;
    dh4[m] = idx < B * 8 ? ld4(cx.HDH + 4 * idx) : z4();
    hh4[m] = (f == 0 && idx < B * 8) ? ld4(cx.HH + 4 * idx) : z4();
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int idx = t + NT * m, b = idx >> 4, k4 = idx & 15;
    p4[m] = idx < B * 16 ? ld4(cx.HP + (size_t)b * 2048 + 64 * f + 4 * k4) : z4();
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const int idx = t + NT * m;
    dlv[m] = (f == 0 && idx < B * 10) ? cx.HDL[idx] : 0.f;
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int idx = t + NT * m;
    if (idx < B * 8) {
      st4(dh_s + 4 * idx, dh4[m]);
      st4(hh_s + 4 * idx, hh4[m]);
    }
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int idx = t + NT * m;
    if (idx < B * 16) st4(p_s + 4 * idx, p4[m]);
  }
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const int idx = t + NT * m;
    if (idx < B * 10) dl_s[(idx / 10) * 16 + idx % 10] = dlv[m];
  }
  __syncthreads();
  const int j = t >> 3, kk = 8 * (t & 7);
  f32x4 a0 = z4(), a1 = z4();
  for (int b = 0; b < B; ++b) {
    const float dh = dh_s[b * 32 + j];
    a0 += dh * ld4(p_s + b * 64 + kk);
    a1 += dh * ld4(p_s + b * 64 + kk + 4);
  }
  st4(cx.grads + OFF_FC1W + j * 2048 + 64 * f + kk, a0);
  st4(cx.grads + OFF_FC1W + j * 2048 + 64 * f + kk + 4, a1);
  if (f == 0) {
    for (int idx = t; idx < 32 + 320 + 10; idx += NT) {
      float s = 0.f;
      if (idx < 32) {
        for (int b = 0; b < B; ++b) s += dh_s[b * 32 + idx];
        cx.grads[OFF_FC1B + idx] = s;
      } else if (idx < 352) {
        const int o = (idx - 32) >> 5, jj = (idx - 32) & 31;
        for (int b = 0; b < B; ++b) s += dl_s[b * 16 + o] * hh_s[b * 32 + jj];
        cx.grads[OFF_FC2W + o * 32 + jj] = s;
      } else {
        const int o = idx - 352;
        for (int b = 0; b < B; ++b) s += dl_s[b * 16 + o];
        cx.grads[OFF_FC2B + o] = s;
      }
    }
  }
}

// wgrad of trunk block `blk` over RW rows of one image, from DY[blk] and X[blk] (stored by earlier kernels)
template <bool BF, int RW>
__device__ void wgrad_role(const Ctx& cx, int blk, int wv, char* smem) {
  constexpr int ESZ = Rec<BF>::ESZ, PADE = 16 / ESZ;
  constexpr int DS = RW * 16 + PADE, XS = (RW + 2) * 16 + PADE;
  constexpr int ND = RW / 2, NX = (RW + 2) / 2;  // float4 loads per thread
  using TA = typename std::conditional<BF, unsigned short, float>::type;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int n = wv / (16 / RW), r0 = (wv % (16 / RW)) * RW;
  TA* dyT = (TA*)smem;
  TA* xT = dyT + 32 * DS;
  const float* dyp = cx.DY + act_off(blk, cx.B) + (size_t)n * 8192 + r0 * 512;
  const float* xp = cx.X + act_off(blk, cx.B) + (size_t)n * 8192;
  f32x4 dv[ND], xv[NX];
#pragma unroll
  for (int m = 0; m < ND; ++m) dv[m] = ld4(dyp + 4 * (t + NT * m));
#pragma unroll
  for (int m = 0; m < NX; ++m) {
    const int f = t + NT * m, tr = f >> 7, row = r0 - 1 + tr;
    xv[m] = (row >= 0 && row < 16) ? ld4(xp + (row * 16 + ((f >> 3) & 15)) * 32 + 4 * (f & 7)) : z4();
  }
  for (int idx = t; idx < 3 * 32 * XS * ESZ / 16; idx += NT) ((uint4*)xT)[idx] = uint4{0u, 0u, 0u, 0u};
  __syncthreads();
#pragma unroll
  for (int m = 0; m < ND; ++m) {
    const int f = t + NT * m, pix = f >> 3, c4 = f & 7;
#pragma unroll
    for (int e = 0; e < 4; ++e) dyT[(4 * c4 + e) * DS + pix] = BF ? (TA)bfbits(dv[m][e]) : (TA)dv[m][e];
  }
#pragma unroll
  for (int m = 0; m < NX; ++m) {
    const int f = t + NT * m, tr = f >> 7, col = (f >> 3) & 15, c4 = f & 7, row = r0 - 1 + tr;
    if (row < 0 || row >= 16) continue;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int cc = col + 1 - kw;
      if (cc < 0 || cc >= 16) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        xT[(kw * 32 + 4 * c4 + e) * XS + tr * 16 + cc] = BF ? (TA)bfbits(xv[m][e]) : (TA)xv[m][e];
    }
  }
  __syncthreads();
  const int nw_blk = cx.B * (16 / RW);
  wgrad_core<BF, RW>((const char*)dyT, DS, (const char*)xT, XS,
                     cx.WSLAB + ((size_t)(blk - 1) * nw_blk + wv) * WSLAB_N, wave, lane);
}

// dgrad role: BN-backward of block i -> dgrad conv -> g_i; epilogue prepares block i-1 (or the stem, i == 0)
template <bool BF, int R, int RW>
__device__ void dgrad_role(const Ctx& cx, int i, int wg, char* smem) {
  constexpr int RR = R + 2, TPI = 16 / R, NF = RR * 128 / NT, RB = Rec<BF>::BYTES, NO = R / 2;
  constexpr int ESZ = Rec<BF>::ESZ, PADE = 16 / ESZ;
  constexpr int DS0 = R * 16 + PADE, XS0 = RR * 16 + PADE;          // block-0 in-tile wgrad
  constexpr int IRb = 2 * R + 2, IW = 34, DSP = 2 * R * 32 + PADE;   // stem backward
  using TA = typename std::conditional<BF, unsigned short, float>::type;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, c = lane & 15, q = lane >> 4;
  const int n = wg / TPI, r0 = (wg % TPI) * R;
  const int nparts = cx.B * TPI;
  const int rd = (9 - i) & 1, wr = (10 - i) & 1;

  char* ws = smem;
  char* dys = ws + 288 * RB;
  float* gown = (float*)(dys + RR * 18 * RB);  // [R*16][32]
  float* yprev = gown + R * 512;               // [R*16][32]
  float* red = yprev + R * 512;                // [RED_F]
  float* s_a = red + RED_F;
  float* s_b = s_a + 32;
  float* s_mean = s_b + 32;
  float* s_inv = s_mean + 32;
  float* s_scale = s_inv + 32;
  float* s_shift = s_scale + 32;
  float* s_k1 = s_shift + 32;
  float* s_pm = s_k1 + 32;
  float* s_pi = s_pm + 32;
  float* s_gam = s_pi + 32;
  float* s_bet = s_gam + 32;
  char* ext = (char*)(s_bet + 32);              // block-0 extras
  TA* dyT = (TA*)ext;                           // [32][DS0]
  TA* xT = dyT + 32 * DS0;                      // [3][32][XS0]
  float* xin = (float*)(xT + 3 * 32 * XS0);     // [3][IRb][IW]
  TA* dsT = (TA*)(xin + 3 * IRb * IW);          // [32][DSP]

  // ---- issue every global load ----
  const size_t img = (size_t)n * 8192;
  const float* gin = cx.G + (size_t)rd * cx.B * 8192 + img;
  const float* yi = cx.Y + act_off(i, cx.B) + img;
  const float* x0p = cx.X + img;  // block 0 input (in-tile wgrad, i == 0)
  f32x4 gv[NF], yv[NF], xv[NF];
#pragma unroll
  for (int m = 0; m < NF; ++m) {
    const int f = t + NT * m, tr = f >> 7, col = (f >> 3) & 15, c4 = f & 7, row = r0 - 1 + tr;
    const bool ok = row >= 0 && row < 16;
    const int off = (row * 16 + col) * 32 + 4 * c4;
    gv[m] = ok ? ld4(gin + off) : z4();
    yv[m] = ok ? ld4(yi + off) : z4();
    xv[m] = (ok && i == 0) ? ld4(x0p + off) : z4();
  }
  f32x4 ypv[NO];
  {
    const float* yp = cx.Y + act_off(i > 0 ? i - 1 : 0, cx.B) + img + r0 * 512;
#pragma unroll
    for (int m = 0; m < NO; ++m) ypv[m] = i >= 1 ? ld4(yp + 4 * (t + NT * m)) : z4();
  }
  const float2* bpart = cx.BPART + (size_t)rd * cx.pstride * 32;
  Parts P;
  parts_load(P, bpart, nparts);
  WStage<BF> W;
  wstage_load<BF>(W, cx.wt_d);
  float2 st = make_float2(0.f, 0.f), stp = make_float2(0.f, 0.f);
  float gam = 0.f, bet = 0.f, pgw = 0.f, pgb = 0.f;
  if (t < 32) {
    st = cx.STATS[i * 32 + t];
    if (i >= 1) stp = cx.STATS[(i - 1) * 32 + t];
    gam = cx.params[OFF_BNW + t];
    bet = cx.params[OFF_BNB + t];
    if (wg == 0 && i != 9) {
      pgw = cx.grads[OFF_BNW + t];
      pgb = cx.grads[OFF_BNB + t];
    }
  }
  InRows<IRb> I;
  if (i == 0) inrows_load<IRb>(I, cx.data + (size_t)sample_id(cx, n) * 3072, 2 * r0 - 1);
  uint8_t codes[NO][4];
  if (i == 0) {
    const uint8_t* codep = cx.SCODE + img + r0 * 512;
#pragma unroll
    for (int j = 0; j < NO; ++j)
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int tt = wave + 4 * j, rr = tt >> 1, ch = 16 * (tt & 1) + c;
        codes[j][ii] = codep[(rr * 16 + 4 * q + ii) * 32 + ch];
      }
  }
  // ---- LDS fills ----
  wstage_store<BF>(W, ws);
  zero_recs<BF>(dys, 0, RR, 18);
  zero_recs<BF>(dys, 17, RR, 18);
#pragma unroll
  for (int m = 0; m < NO; ++m) st4(yprev + 4 * (t + NT * m), ypv[m]);
  if (i == 0) {
    for (int idx = t; idx < 3 * 32 * XS0 * ESZ / 16; idx += NT) ((uint4*)xT)[idx] = uint4{0u, 0u, 0u, 0u};
    for (int idx = t; idx < 32 * DSP * ESZ / 16; idx += NT) ((uint4*)dsT)[idx] = uint4{0u, 0u, 0u, 0u};
    inrows_store<IRb>(I, xin, 2 * r0 - 1);
  }
  DCA_STAMP(cx, 21 - i, wg, 1);
  bsums_finish(P, bpart, nparts, red, s_a, s_b);
  DCA_STAMP(cx, 21 - i, wg, 2);
  if (t < 32) {
    const float N = (float)cx.B * 256.f;
    s_mean[t] = st.x;
    s_inv[t] = st.y;
    s_scale[t] = gam * st.y;
    s_shift[t] = bet - st.x * gam * st.y;
    s_k1[t] = gam * st.y / N;
    s_gam[t] = gam;
    s_bet[t] = bet;
    s_pm[t] = stp.x;
    s_pi[t] = stp.y;
    if (wg == 0) {  // shared BN affine grads accumulate over the 10 applications
      cx.grads[OFF_BNW + t] = pgw + s_b[t];
      cx.grads[OFF_BNB + t] = pgb + s_a[t];
    }
  }
  __syncthreads();
  {
    const float N = (float)cx.B * 256.f;
    float* dyo = cx.DY + act_off(i, cx.B) + img;
#pragma unroll
    for (int m = 0; m < NF; ++m) {
      const int f = t + NT * m, tr = f >> 7, col = (f >> 3) & 15, c4 = f & 7, row = r0 - 1 + tr;
      f32x4 dy = z4();
      if (row >= 0 && row < 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ch = 4 * c4 + e;
          const float y = yv[m][e];
          const float xh = (y - s_mean[ch]) * s_inv[ch];
          const float z = y * s_scale[ch] + s_shift[ch];
          const float dz = z > 0.f ? gv[m][e] : 0.f;
          dy[e] = s_k1[ch] * (N * dz - s_a[ch] - xh * s_b[ch]);
        }
        if (tr >= 1 && tr <= R) {
          const int po = ((tr - 1) * 16 + col) * 32 + 4 * c4;
          st4(gown + po, gv[m]);
          if (i >= 1) st4(dyo + (row * 16 + col) * 32 + 4 * c4, dy);
          else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              dyT[(4 * c4 + e) * DS0 + (tr - 1) * 16 + col] = BF ? (TA)bfbits(dy[e]) : (TA)dy[e];
          }
        }
        if (i == 0) {
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const int cc = col + 1 - kw;
            if (cc < 0 || cc >= 16) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e)
              xT[(kw * 32 + 4 * c4 + e) * XS0 + tr * 16 + cc] = BF ? (TA)bfbits(xv[m][e]) : (TA)xv[m][e];
          }
        }
      }
      st4_rec<BF>(dys, tr * 18 + col + 1, col + 1, c4, dy);
    }
  }
  __syncthreads();
  DCA_STAMP(cx, 21 - i, wg, 3);
  f32x4 acc[R / 2];
  conv_core<BF, R>(dys, ws, acc, wave, lane);
  DCA_STAMP(cx, 21 - i, wg, 4);

  if (i >= 1) {
    float* gout = cx.G + (size_t)wr * cx.B * 8192 + img + r0 * 512;
#pragma unroll
    for (int j = 0; j < R / 2; ++j) {
      const int tt = wave + 4 * j, rr = tt >> 1, ch = 16 * (tt & 1) + c;
      const float scp = s_gam[ch] * s_pi[ch], shp = s_bet[ch] - s_pm[ch] * s_gam[ch] * s_pi[ch];
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int po = (rr * 16 + 4 * q + ii) * 32 + ch;
        const float g = gown[po] + acc[j][ii];
        gout[po] = g;
        const float y = yprev[po];
        const float z = y * scp + shp;
        const float dz = z > 0.f ? g : 0.f;
        sa += dz;
        sb += dz * (y - s_pm[ch]) * s_pi[ch];
      }
      sa += __shfl_xor(sa, 16);
      sa += __shfl_xor(sa, 32);
      sb += __shfl_xor(sb, 16);
      sb += __shfl_xor(sb, 32);
      if (q == 0) {
        red[tt * 16 + c] = sa;
        red[256 + tt * 16 + c] = sb;
      }
    }
    __syncthreads();
    if (t < 32) {
      const int h = t >> 4, cc = t & 15;
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        sa += red[(rr * 2 + h) * 16 + cc];
        sb += red[256 + (rr * 2 + h) * 16 + cc];
      }
      cx.BPART[((size_t)wr * cx.pstride + wg) * 32 + t] = make_float2(sa, sb);
    }
    return;
  }

  // ---- i == 0: stem backward (maxpool-bwd routed by the saved argmax, ReLU mask) + stem & block-0 wgrads ----
#pragma unroll
  for (int j = 0; j < R / 2; ++j) {
    const int tt = wave + 4 * j, rr = tt >> 1, ch = 16 * (tt & 1) + c;
    float db = 0.f;
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
      const int col = 4 * q + ii, po = (rr * 16 + col) * 32 + ch;
      const float g = gown[po] + acc[j][ii];
      const int code = codes[j][ii];
      if (code & 4) {
        const int pos = code & 3;
        const int sr = 2 * rr + (pos >> 1), sc = 2 * col + (pos & 1);
        dsT[ch * DSP + sr * 32 + sc] = BF ? (TA)bfbits(g) : (TA)g;
        db += g;
      }
    }
    db += __shfl_xor(db, 16);
    db += __shfl_xor(db, 32);
    if (q == 0) red[tt * 16 + c] = db;
  }
  __syncthreads();
  float* sslab = cx.SSLAB + (size_t)wg * SSLAB_N;
  if (t < 32) {
    const int h = t >> 4, cc = t & 15;
    float s = 0.f;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) s += red[(rr * 2 + h) * 16 + cc];
    sslab[1024 + t] = s;
  }
  // stem wgrad: D[co][k] = sum_p ds[p][co] * im2col[p][k]; wave -> tile (mt = wave&1, nt = wave>>1)
  {
    const int mt = wave & 1, nt = wave >> 1, kidx = 16 * nt + c, co = 16 * mt + c;
    const bool kv = kidx < 27;
    const int ci = kidx / 9, kh = (kidx % 9) / 3, kw = kidx % 3;
    const float* xb = xin + (kv ? ci * IRb * IW + kh * IW + kw : 0);
    f32x4 acc2 = z4();
    for (int s = 0; s < 2 * R; ++s) {
      if constexpr (BF) {
        const bf16x8 a = *(const bf16x8*)(dsT + co * DSP + s * 32 + 8 * q);
        bf16x8 b;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) b[jj] = (__bf16)(kv ? xb[s * IW + 8 * q + jj] : 0.f);
        acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc2, 0, 0, 0);
      } else {
#pragma unroll
        for (int b2 = 0; b2 < 2; ++b2) {
          const f32x4 a = *(const f32x4*)(dsT + co * DSP + s * 32 + 16 * b2 + 4 * q);
#pragma unroll
          for (int st2 = 0; st2 < 4; ++st2) {
            const float bv = kv ? xb[s * IW + 16 * b2 + 4 * q + st2] : 0.f;
            acc2 = mfma4(a[st2], bv, acc2);
          }
        }
      }
    }
    st4(sslab + ((wave * 64 + lane) << 2), acc2);
  }
  // block-0 trunk wgrad, in tile
  const int nw_blk = cx.B * (16 / RW);
  wgrad_core<BF, R>((const char*)dyT, DS0, (const char*)xT, XS0, cx.WSLAB + ((size_t)9 * nw_blk + wg) * WSLAB_N,
                    wave, lane);
}

template <bool BF, int R, int RW>
__global__ void __launch_bounds__(NT) k_bwd_block(Ctx cx, int i) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nparts = cx.B * (16 / R);
  int bid = blockIdx.x;
  DCA_STAMP(cx, 21 - i, blockIdx.x, 0);
  if (bid < nparts) {
    dgrad_role<BF, R, RW>(cx, i, bid, smem);
  } else {
    bid -= nparts;
    if (i == 9) fc_grads_role(cx, bid, smem);
    else wgrad_role<BF, RW>(cx, i + 1, bid, smem);
  }
  DCA_STAMP(cx, 21 - i, blockIdx.x, 5);
}

// ============================================================================================================
// Gradient reduction + (optionally fused) SGD + derived weight layouts + bookkeeping.
// ============================================================================================================
template <bool BF>
__device__ __forceinline__ void put_w(void* dst, int idx, float w) {
  if constexpr (BF) ((unsigned short*)dst)[idx] = bfbits(w);
  else ((float*)dst)[idx] = w;
}

template <bool BF>
__global__ void __launch_bounds__(NT) k_reduce(Ctx cx, int nslab, int nsslab) {
  __shared__ f32x4 red[NT];
  const int t = threadIdx.x, bid = blockIdx.x;
  DCA_STAMP(cx, 22, bid, 0);
  if (bid < N_TRUNK_RED_WG + N_STEM_RED_WG) {
    const bool stem = bid >= N_TRUNK_RED_WG;
    const int chunk = stem ? bid - N_TRUNK_RED_WG : bid;
    const int slot = t & 7, grp = t >> 3, e0 = chunk * RED_CHUNK + slot * 4;
    const float* src = stem ? cx.SSLAB : cx.WSLAB;
    const int stride = stem ? SSLAB_N : WSLAB_N, cnt = stem ? nsslab : nslab;
    f32x4 s = z4();
    for (int k0 = grp; k0 < cnt; k0 += 32 * 8) {  // 8 slab loads in flight per thread
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + 32 * u;
        v[u] = k < cnt ? ld4(src + (size_t)k * stride + e0) : z4();
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    red[t] = s;
    __syncthreads();
    if (t < 8) {
      f32x4 tot = z4();
#pragma unroll
      for (int g = 0; g < 32; ++g) tot += red[g * 8 + t];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int e = chunk * RED_CHUNK + t * 4 + ii;
        int pidx = -1, kind = 0, d0 = 0, d1 = 0;
        if (!stem) {
          const int tt = e >> 8, ln = (e >> 2) & 63, mt = tt & 1, nt = tt >> 1, tap = nt >> 1, cih = nt & 1;
          const int co = 16 * mt + 4 * (ln >> 4) + ii, ci = 16 * cih + (ln & 15);
          pidx = OFF_CONVW + co * 288 + ci * 9 + tap;
          kind = 1;
          d0 = (tap * 32 + co) * 32 + ci;
          d1 = ((8 - tap) * 32 + ci) * 32 + co;
        } else if (e < 1024) {
          const int tt = e >> 8, ln = (e >> 2) & 63, mt = tt & 1, nt = tt >> 1;
          const int co = 16 * mt + 4 * (ln >> 4) + ii, k = 16 * nt + (ln & 15);
          if (k < 27) {
            pidx = OFF_C1W + co * 27 + k;
            kind = 2;
            d0 = co * 32 + k;
          }
        } else if (e < 1056) {
          pidx = OFF_C1B + (e - 1024);
        }
        if (pidx < 0) continue;
        const float g = tot[ii];
        cx.grads[pidx] = g;
        if (cx.fuse_sgd) {
          const float w = cx.params[pidx] - cx.lr * g;
          cx.params[pidx] = w;
          if (kind == 1) {
            put_w<BF>(cx.wt_f, d0, w);
            put_w<BF>(cx.wt_d, d1, w);
          } else if (kind == 2) {
            put_w<BF>(cx.sw, d0, w);
          }
        }
      }
    }
    return;
  }
  const int ob = bid - N_TRUNK_RED_WG - N_STEM_RED_WG;
  const int nother = gridDim.x - N_TRUNK_RED_WG - N_STEM_RED_WG - 1;
  if (ob < nother) {  // SGD of fc1/fc2/BN (their grads were written directly by the backward kernels)
    constexpr int NA = BUCKET_A_END / 4, NBN = (OFF_C1W - OFF_BNW) / 4;
    for (int v = ob * NT + t; v < NA + NBN; v += nother * NT) {
      const int e = v < NA ? 4 * v : OFF_BNW + 4 * (v - NA);
      const f32x4 g = ld4(cx.grads + e);
      st4(cx.params + e, ld4(cx.params + e) - cx.lr * g);
    }
    return;
  }
  // bookkeeping workgroup: batch-mean loss (fixed-order reduction), cursor, step counter, CC4 segment
  {
    float* rl = (float*)red;
    float v = 0.f;
    for (int b = t; b < cx.B; b += NT) v += cx.HLOSS[b];
    rl[t] = v;
    __syncthreads();
    if (t == 0) {
      float s = 0.f;
      for (int k = 0; k < NT && k < cx.B; ++k) s += rl[k];
      *cx.loss_acc += (double)(s / (float)cx.B);
      *cx.cursor += cx.B;
      *cx.step_count += 1;
    }
  }
  if (!cx.fuse_sgd && t < 64) {  // CC4: rank 0's running stats ride the bucket-B all-reduce (others add 0)
    const float v = t < 32 ? cx.rm[t] : cx.rv[t - 32];
    cx.grads[OFF_RS + t] = cx.rank == 0 ? v : 0.f;
  }
}

// Kernel-layout copies of flat parameter e (value w): bf16 fc1 for the persistent head, the forward / dgrad
// conv weight tiles, the stem weight (plain and as MFMA B fragments).  Other parameters have no copy.
// Each engine sets only the copies its kernels read; the others are null (kernel-argument pointers, so these tests
// are uniform branches).
template <bool BF>
__device__ __forceinline__ void derive_param(const Ctx& cx, int e, float w) {
  if (e < OFF_FC1W + 65536) {
    if (cx.w1b) ((unsigned short*)cx.w1b)[e - OFF_FC1W] = bfbits(w);  // bf16 fc1 copy (sliced engine's head)
  } else if (e >= OFF_CONVW && e < OFF_CONVW + 9216) {
    if (cx.wt_f) {
      const int r = e - OFF_CONVW, co = r / 288, ci = (r / 9) % 32, tap = r % 9;
      put_w<BF>(cx.wt_f, (tap * 32 + co) * 32 + ci, w);
      put_w<BF>(cx.wt_d, ((8 - tap) * 32 + ci) * 32 + co, w);
    }
  } else if (e >= OFF_C1W && e < OFF_C1W + 864) {
    const int r = e - OFF_C1W, co = r / 27, k = r % 27;
    if (cx.sw) put_w<BF>(cx.sw, co * 32 + k, w);
    if (cx.swf) ((unsigned short*)cx.swf)[swf_slot(co, k)] = bfbits(w);
  }
  if (cx.pkw != nullptr) {  // hi / lo bf16 splits for the sliced persistent engine
    const unsigned short hi = bfbits(w), lo = bfbits(w - __uint_as_float((unsigned)hi << 16));
    if (e >= OFF_CONVW && e < OFF_CONVW + 9216) {
      const int r = e - OFF_CONVW, co = r / 288, ci = (r / 9) % 32, tap = r % 9;
      const int fo = pkw_elem(tap * 32 + co, ci), dofs = PKW_DGRAD + pkw_elem((8 - tap) * 32 + ci, co);
      cx.pkw[fo] = hi;
      cx.pkw[PKW_PLANE + fo] = lo;
      cx.pkw[dofs] = hi;
      cx.pkw[PKW_PLANE + dofs] = lo;
    } else if (e >= OFF_C1W && e < OFF_C1W + 864) {
      const int r = e - OFF_C1W, slot = swf_slot(r / 27, r % 27);
      cx.pkw[PKW_STEM + slot] = hi;
      cx.pkw[PKW_STEM + 1536 + slot] = lo;
    }
  }
}

// SGD after the gradient all-reduce (world_size > 1), or mode 0 = derive weight layouts / init state only.
template <bool BF>
__global__ void __launch_bounds__(NT) k_apply_sgd(Ctx cx, int mode) {
  const int gid = blockIdx.x * NT + threadIdx.x, gsz = gridDim.x * NT;
  for (int e = gid; e < OFF_RS; e += gsz) {
    float w = cx.params[e];
    if (mode) {
      w -= cx.lr * cx.grads[e] * cx.inv_ws;
      cx.params[e] = w;
    }
    derive_param<BF>(cx, e, w);
  }
  if (gid < 64) {
    if (mode) cx.rs_base[gid] = cx.grads[OFF_RS + gid];
    else cx.rs_base[gid] = gid < 32 ? cx.rm[gid] : cx.rv[gid - 32];
  }
  if (!mode && gid < 32 * 5 && cx.sw) put_w<BF>(cx.sw, (gid / 5) * 32 + 27 + gid % 5, 0.f);
  if (!mode && gid < 2 * 3 * 64 * 4 && cx.swf) {  // never-written zero slots of the stem fragments (4th channel, taps 9..11)
    const int ci = gid & 3, lane = (gid >> 2) & 63, m = (gid >> 8) % 3, tap = 4 * m + (lane >> 4);
    if (ci == 3 || tap >= 9) ((unsigned short*)cx.swf)[gid] = 0;
  }
}

}  // namespace dca
