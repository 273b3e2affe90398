// Depthwise 7 x 7 convolution (groups == C, pad 3, stride 1) with an optional bias over NHWC bf16 activations,
// C % 8 == 0, rows of at most 64 pixels: the depthwise layer of every ConvNeXt block up to a 256 input.  49
// multiply-adds per output element and no reduction over channels, so, as at 3 x 3 (ops_dwconv.hip), no MFMA fits
// (there is no K dimension) and the math is fp32 VALU on two-channel pairs (v_pk_fma_f32).
//
// Why not the 3 x 3 design.  That kernel gives a thread a 16-byte chunk of 8 channels and keeps its 9 x 8 weights in
//   registers; at 7 x 7 that is 392 weight registers plus 7 carried rows.  Reading the weights from LDS at every tap
//   instead makes LDS the bound (about 100 16-byte reads against 196 packed FMAs per input row, four SIMDs on one port).
// Work split.  A thread owns ONE channel pair (4 bytes) of one output column for the workgroup's lifetime: 49 weights
//   as fp32 pairs (98 registers; fp32 master weight rounded to bf16 RNE, no packed operand, no pack launch), seven
//   carried output rows (14) and the seven taps of the current input row (14).  A workgroup of 256 threads owns a slab
//   of CP = 4, 8, 16 or 32 channel pairs (8 / 16 / 32 / 64 channels) x 256 / CP columns and a range of units, a unit
//   being a strip of consecutive output rows of one image.  CP follows the row width so that the columns cover the row
//   without leaving most of the workgroup idle: 4 x 64 up to 64 pixels, 8 x 32 up to 32, 16 x 16 up to 16 and 32 x 8
//   up to 8 (ConvNeXt's 56 / 28 / 14 / 7: 88 % of the lanes active at every stage), and no wider than the channels.
//   Lanes run pair-fastest, so the 4-byte bf16x2 stores of CP neighbouring lanes form 16- to 128-byte segments.
//   A slab's weights are contiguous, so they are fetched coalesced into LDS once and each thread takes its 98 from
//   there (98 strided global loads per thread cost the 64-channel form 20 us).  Workgroups are numbered slab-fastest
//   in a logical id (d7_block) that puts the slabs of one unit on one XCD: they share every cache line of the unit's
//   input rows, and each XCD has its own L2 (96 x 56 x 56 forward at batch 256: 333 -> 180 us with both changes).
//   Resources (gfx950, no scratch): forward 168 VGPRs / 3 waves per SIMD at CP = 4, 174 / 2 otherwise; weight gradient
//   172 - 184 / 2.  Asking for 3 waves everywhere spilled 8 - 52 bytes per lane, so no occupancy is requested.
// Row reuse.  Input row r feeds output rows r - 3 .. r + 3, so a thread reads a row's seven taps once (7 ds_read_b32)
//   and issues 49 packed FMAs into its seven carried sums; the sum of output row r - 3 is then complete and stored.
//   An output row costs 7 LDS reads, not 49.  The carried sums rotate through seven register slots; the row loop is
//   unrolled by seven so that every slot index is a constant.  Every output sums its taps in the order kh, kw, then
//   the bias, one fixed order: a launch repeats bit for bit.  Rows outside the image (and the strip's tail) skip their
//   FMAs: at the 7- and 14-row stages the padding rows cost nothing.
// LDS.  A ring of 14 slots = 2 groups of 7 input rows: one group is read while the next is stored.  Because the sums
//   are carried, an input row is read in one step only, so nothing older has to stay.  A slot is pixel-major,
//   [COLS + 6 positions][CP pairs][4 B]: pixel iw at position iw + 3, three zero positions on each side, so the tap loop
//   has no boundary branch.  A row is at most 64 pieces of 16 bytes whatever the form, so a whole group of 7 rows is
//   fetched by two coalesced 16-byte buffer loads per thread, issued one group (seven rows of math) ahead of its use;
//   rows and pixels outside the image read zero through the descriptor.  One barrier per seven rows.
//   Banks: a thread reads tap kw at (col + kw) * 4 CP + 4 pair; the 64 lanes of a wave are 64 / CP consecutive
//   columns x CP pairs = 256 contiguous bytes = the 64 banks once each, for every tap shift.
// Units.  At batch 256 every stage has 3072 slab-images, so a unit is a whole image (one strip): no halo row is read
//   twice, re-read overhead 0 %.  Smaller batches split an image into strips of at least 8 rows until about 768 units
//   exist; a strip re-reads its 6 halo rows (6 / (rows + 6) of its input, at most 43 % at 8 rows).
// Input gradient.  Stride 1 and symmetric padding: the forward kernel over dY with the taps flipped (tap 48 - t) and no
//   bias.  Every dX element is written exactly once: no memset.
// Weight and bias gradient.  k_dwconv7x7_wgrad: the same ring of x rows; a thread keeps 49 (+ 1) pair sums over all its
//   units (100 registers) and a window of the last seven dY values of its own column (read straight from global memory,
//   4 bytes per thread, seven rows ahead).  Input row r meets dY rows r + 3 - kh: again 7 LDS reads and 49 packed FMAs
//   per row.  The columns of a channel pair are summed through LDS in column order into slab `workgroup` of an fp32
//   workspace [slabs][C][50] (49 taps, then the column sum of dY for the bias), and k_dwconv7_wgrad_reduce sums the
//   slabs in index order into torch's [C][1][7][7] and [C] (beta 1: onto what is there).  No float atomics.
#pragma once
#include "ops_dwconv.hip"

namespace dca {
namespace ops {

constexpr unsigned D7_OOB = 0xfffffff0u;  // past every buffer of fewer than 2^31 bf16 elements
constexpr int D7_WS = 50;                 // workspace floats per channel: 49 taps + the bias

struct D7Geom {
  int N, H, W, C;
  int strips;  // units per image
};

template <int LP>
struct D7Plan {
  static constexpr int CP = 1 << LP, COLS = DW_NT >> LP;  // channel pairs per slab; thread columns (widest row)
  static constexpr int CHUNKS = CP / 4;                   // 16-byte pieces per pixel
  static constexpr int PX = 4 * CP, SLOT = (COLS + 6) * PX, GROUP = 7 * SLOT;
  static constexpr int RING = 2 * GROUP;
};

// Rows r0 .. r0 + 6 of image n (those inside the image and below rlim): at most 7 x 64 pieces of 16 B, 2 per thread.
template <int LP>
__device__ __forceinline__ void d7_group_load(dw_v4u (&st)[2], const __amdgpu_buffer_rsrc_t& rs, const D7Geom& g, int n,
                                              int r0, int rlim, int c0, int nchunk) {
  using P = D7Plan<LP>;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int e = threadIdx.x + DW_NT * j, k = e >> 6, idx = e & 63, px = idx >> (LP - 2), ch = idx & (P::CHUNKS - 1);
    const int r = r0 + k;
    const bool ok = k < 7 && r >= 0 && r < g.H && r < rlim && px < g.W && ch < nchunk;
    const unsigned o = ok ? ((unsigned)((n * g.H + r) * g.W + px) * (unsigned)g.C + (unsigned)(c0 + 8 * ch)) * 2u
                          : D7_OOB;
    st[j] = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
  }
}
template <int LP>
__device__ __forceinline__ void d7_group_store(const dw_v4u (&st)[2], char* group, int W, int nchunk) {
  using P = D7Plan<LP>;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int e = threadIdx.x + DW_NT * j, k = e >> 6, idx = e & 63, px = idx >> (LP - 2), ch = idx & (P::CHUNKS - 1);
    if (k < 7 && px < W && ch < nchunk) *(dw_v4u*)(group + k * P::SLOT + (px + 3) * P::PX + ch * 16) = st[j];
  }
}
// The logical workgroup id.  Consecutive hardware ids go round the 8 XCDs (each with its own L2); the slabs of one
// unit share every cache line of its input rows, so they are given hardware ids that land on one XCD.
__device__ __forceinline__ int d7_block() {
  const int G = gridDim.x;
  return G % 8 ? (int)blockIdx.x : (int)(blockIdx.x % 8) * (G / 8) + (int)(blockIdx.x / 8);
}
__device__ __forceinline__ dw_f2 d7_cvt(unsigned v) {  // bf16x2 -> fp32 pair
  return dw_f2{__uint_as_float(v << 16), __uint_as_float(v & 0xffff0000u)};
}
// The seven taps of one slot row for this thread's pair and column
template <int LP>
__device__ __forceinline__ void d7_taps(dw_f2 (&t)[7], const char* p) {
#pragma unroll
  for (int kw = 0; kw < 7; ++kw) t[kw] = d7_cvt(*(const unsigned*)(p + kw * D7Plan<LP>::PX));
}

// ---------------------------------------------------------------------------------------------------------
// k_dwconv7x7_fwd: y = bf16(conv(x) + bias) (bias or null).  flip: the input gradient (x = dY, bias null).
// grid: (workgroups per slab) x slabs, slab fastest; requirements as dwconv7_rule (ops_api.hip), W <= COLS.
// ---------------------------------------------------------------------------------------------------------
template <int LP>
__global__ void __launch_bounds__(DW_NT) k_dwconv7x7_fwd(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                         D7Geom g, int flip) {
  using P = D7Plan<LP>;
  __shared__ __attribute__((aligned(16))) char smem[P::RING];
  const int pair = threadIdx.x & (P::CP - 1), col = threadIdx.x >> LP;
  const int nslab = (g.C + 2 * P::CP - 1) / (2 * P::CP);
  const int bid = d7_block(), slab = bid % nslab, vid = bid / nslab, grid = gridDim.x / nslab;
  const int c0 = 2 * P::CP * slab, nchunk = min(P::CHUNKS, (g.C - c0) / 8), cb = c0 + 2 * pair;
  const bool active = cb < g.C && col < g.W;
  const int U = g.N * g.strips;
  const int u_beg = (int)((long long)vid * U / grid), u_end = (int)((long long)(vid + 1) * U / grid);
  // the slab's weights [channels][49] are contiguous: fetched coalesced into the ring's memory, then each thread's 98
  float* wl = (float*)smem;
  for (int e = threadIdx.x; e < min(2 * P::CP, g.C - c0) * 49; e += DW_NT) wl[e] = w[c0 * 49 + e];
  __syncthreads();
  dw_f2 wv[49];
#pragma unroll
  for (int t = 0; t < 49; ++t) {
    const int ti = flip ? 48 - t : t;
    wv[t] = cb < g.C ? dw_f2{bf2f(f2bf_rne(wl[2 * pair * 49 + ti])), bf2f(f2bf_rne(wl[(2 * pair + 1) * 49 + ti]))}
                     : dw_f2{0.f, 0.f};
  }
  __syncthreads();
  for (int e = threadIdx.x; e < P::RING / 16; e += DW_NT) *(dw_v4u*)(smem + e * 16) = dw_v4u{0u, 0u, 0u, 0u};
  const dw_f2 bv = bias && cb < g.C ? dw_f2{bias[cb], bias[cb + 1]} : dw_f2{0.f, 0.f};
  const unsigned bytes = (unsigned)((long long)g.N * g.H * g.W * g.C * 2);
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)x, (short)0, (int)bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc((void*)y, (short)0, (int)bytes, 0x00020000);
  const int toff = col * P::PX + pair * 4;  // this thread's byte offset inside a slot, before the tap
  dw_v4u st[2];
  dw_f2 acc[7];  // slot (i - kh) % 7: the sum of output row o_beg + i - kh, i the input row's index in the strip
  for (int u = u_beg; u < u_end; ++u) {
    const int n = u / g.strips, sidx = u - n * g.strips;
    const int o_beg = (int)((long long)sidx * g.H / g.strips), o_end = (int)((long long)(sidx + 1) * g.H / g.strips);
    const int nrows = o_end - o_beg + 6, ngroups = (nrows + 6) / 7, r_beg = o_beg - 3;  // input rows r_beg + i
#pragma unroll
    for (int s = 0; s < 7; ++s) acc[s] = dw_f2{0.f, 0.f};
    d7_group_load<LP>(st, xrs, g, n, r_beg, o_end + 3, c0, nchunk);
    __syncthreads();  // the ring is zeroed / the previous unit's reads are done
    d7_group_store<LP>(st, smem, g.W, nchunk);
    __syncthreads();
    for (int gi = 0; gi < ngroups; ++gi) {
      const bool pre = gi + 1 < ngroups;
      if (pre) d7_group_load<LP>(st, xrs, g, n, r_beg + 7 * (gi + 1), o_end + 3, c0, nchunk);
      const char* grp = smem + (gi & 1) * P::GROUP + toff;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const int i = 7 * gi + k, r = r_beg + i;
        if (i < nrows) {
          if (r >= 0 && r < g.H) {
            dw_f2 t[7];
            d7_taps<LP>(t, grp + k * P::SLOT);
#pragma unroll
            for (int kh = 0; kh < 7; ++kh)
#pragma unroll
              for (int kw = 0; kw < 7; ++kw)
                acc[(k - kh + 7) % 7] = __builtin_elementwise_fma(wv[kh * 7 + kw], t[kw], acc[(k - kh + 7) % 7]);
          }
          if (i >= 6 && active) {  // output row o_beg + i - 6 has had kh = 6
            const dw_f2 v = acc[(k + 1) % 7] + bv;
            __builtin_amdgcn_raw_buffer_store_b32(
                (unsigned)f2bf_rne(v[0]) | ((unsigned)f2bf_rne(v[1]) << 16), yrs,
                ((unsigned)((n * g.H + o_beg + i - 6) * g.W + col) * (unsigned)g.C + (unsigned)cb) * 2u, 0, 0);
          }
          acc[(k + 1) % 7] = dw_f2{0.f, 0.f};  // the slot of the row that starts with the next input row
        }
      }
      if (pre) d7_group_store<LP>(st, smem + ((gi + 1) & 1) * P::GROUP, g.W, nchunk);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_dwconv7x7_wgrad: per channel and tap the sum of x * dy, and the sum of dy, over the workgroup's pixels, to slab
// `workgroup` of ws[slabs][C][50] fp32.  grid as k_dwconv7x7_fwd.
// ---------------------------------------------------------------------------------------------------------
template <int LP>
__global__ void __launch_bounds__(DW_NT) k_dwconv7x7_wgrad(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                           float* __restrict__ ws, D7Geom g) {
  using P = D7Plan<LP>;
  constexpr int SUMB = DW_NT * 20 * 4;  // the column sum's buffer: 10 pair values of every thread
  __shared__ __attribute__((aligned(16))) char smem[P::RING > SUMB ? P::RING : SUMB];
  const int pair = threadIdx.x & (P::CP - 1), col = threadIdx.x >> LP;
  const int nslab = (g.C + 2 * P::CP - 1) / (2 * P::CP);
  const int bid = d7_block(), slab = bid % nslab, vid = bid / nslab, grid = gridDim.x / nslab;
  const int c0 = 2 * P::CP * slab, nchunk = min(P::CHUNKS, (g.C - c0) / 8), cb = c0 + 2 * pair;
  const bool active = cb < g.C && col < g.W;
  const int U = g.N * g.strips;
  const int u_beg = (int)((long long)vid * U / grid), u_end = (int)((long long)(vid + 1) * U / grid);
  for (int e = threadIdx.x; e < P::RING / 16; e += DW_NT) *(dw_v4u*)(smem + e * 16) = dw_v4u{0u, 0u, 0u, 0u};
  const unsigned bytes = (unsigned)((long long)g.N * g.H * g.W * g.C * 2);
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)x, (short)0, (int)bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc((void*)dy, (short)0, (int)bytes, 0x00020000);
  const int toff = col * P::PX + pair * 4;
  dw_f2 acc[D7_WS];
#pragma unroll
  for (int t = 0; t < D7_WS; ++t) acc[t] = dw_f2{0.f, 0.f};
  dw_v4u st[2];
  dw_f2 win[7];     // slot q % 7: this column's dY of output row o_beg + q, for the seven rows an input row meets
  unsigned nxt[7];  // slot q % 7: dY of row o_beg + q as loaded (bf16x2), seven rows ahead
  for (int u = u_beg; u < u_end; ++u) {
    const int n = u / g.strips, sidx = u - n * g.strips;
    const int o_beg = (int)((long long)sidx * g.H / g.strips), o_end = (int)((long long)(sidx + 1) * g.H / g.strips);
    const int len = o_end - o_beg, nrows = len + 6, ngroups = (nrows + 6) / 7, r_beg = o_beg - 3;
    auto dy_load = [&](int q) {  // rows past the strip belong to another unit: zero
      const bool ok = active && q < len;
      return __builtin_amdgcn_raw_buffer_load_b32(
          drs, ok ? ((unsigned)((n * g.H + o_beg + q) * g.W + col) * (unsigned)g.C + (unsigned)cb) * 2u : D7_OOB, 0, 0);
    };
#pragma unroll
    for (int s = 0; s < 7; ++s) {
      win[s] = dw_f2{0.f, 0.f};
      nxt[s] = dy_load(s);
    }
    d7_group_load<LP>(st, xrs, g, n, r_beg, o_end + 3, c0, nchunk);
    __syncthreads();
    d7_group_store<LP>(st, smem, g.W, nchunk);
    __syncthreads();
    for (int gi = 0; gi < ngroups; ++gi) {
      const bool pre = gi + 1 < ngroups;
      if (pre) d7_group_load<LP>(st, xrs, g, n, r_beg + 7 * (gi + 1), o_end + 3, c0, nchunk);
      const char* grp = smem + (gi & 1) * P::GROUP + toff;
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const int i = 7 * gi + k, r = r_beg + i;
        if (i < nrows) {
          win[k] = d7_cvt(nxt[k]);  // dY row o_beg + i enters (kh = 0); it leaves after input row i + 6
          acc[49] += win[k];
          nxt[k] = dy_load(i + 7);
          if (r >= 0 && r < g.H) {
            dw_f2 t[7];
            d7_taps<LP>(t, grp + k * P::SLOT);
#pragma unroll
            for (int kh = 0; kh < 7; ++kh)
#pragma unroll
              for (int kw = 0; kw < 7; ++kw)
                acc[kh * 7 + kw] = __builtin_elementwise_fma(t[kw], win[(k - kh + 7) % 7], acc[kh * 7 + kw]);
          }
        }
      }
      if (pre) d7_group_store<LP>(st, smem + ((gi + 1) & 1) * P::GROUP, g.W, nchunk);
      __syncthreads();
    }
  }
  // the columns of each channel in column order, ten values at a time: buf[col][10][2 CP channels]
  float* buf = (float*)smem;
#pragma unroll
  for (int b = 0; b < D7_WS / 10; ++b) {
    __syncthreads();  // (whatever read this memory before is done)
#pragma unroll
    for (int j = 0; j < 10; ++j)
      *(dw_f2*)(buf + (col * 10 + j) * 2 * P::CP + 2 * pair) = acc[b * 10 + j];
    __syncthreads();
    for (int s = threadIdx.x; s < 20 * P::CP; s += DW_NT) {
      const int j = s / (2 * P::CP), pe = s % (2 * P::CP);
      float r = 0.f;
      for (int c = 0; c < P::COLS; ++c) r += buf[(c * 10 + j) * 2 * P::CP + pe];
      if (c0 + pe < g.C) ws[((size_t)vid * g.C + c0 + pe) * D7_WS + b * 10 + j] = r;
    }
  }
}

// dw[c][tap] (torch [C][1][7][7]) and db[c] (or null) = (beta ? what is there : 0) + sum over slabs, in slab order
__global__ void __launch_bounds__(256) k_dwconv7_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ dw,
                                                              float* __restrict__ db, int C, int slabs, int beta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * D7_WS) return;
  const int c = i / D7_WS, t = i - c * D7_WS;
  float* dst = t < 49 ? dw + c * 49 + t : (db ? db + c : nullptr);
  if (!dst) return;
  float s = 0.f;
  for (int v = 0; v < slabs; ++v) s += ws[(size_t)v * C * D7_WS + i];
  *dst = beta ? *dst + s : s;
}

}  // namespace ops
}  // namespace dca
