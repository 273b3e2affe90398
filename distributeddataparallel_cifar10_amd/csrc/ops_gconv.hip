// Grouped 3 x 3 convolution (pad 1, stride 1 or 2) over NHWC bf16 activations, Cin = Cout = C, Cg = C / groups in
// {4, 8, 16, 32}, input rows of at most 64 pixels: every 3 x 3 of ResNeXt-50 32x4d.  Per group the conv is a GEMM
// with N = Cg, so the dense row-ring kernels would run 32 tiny GEMMs or multiply a weight matrix that is 97 % zeros;
// these kernels are bound by their bytes (x read once, y written once) and split the work by channel instead.
//
// Work split.  The unit of channels is a block of 16: for Cg <= 16 it holds 16 / Cg whole groups (its 16 outputs read
//   its own 16 inputs through a block-diagonal 16 x 16 matrix per tap), for Cg = 32 a group is two output blocks over
//   32 inputs.  A workgroup of 4 waves owns a slab of 64 channels (wave w: output block w of the slab; fewer at a
//   ragged end) and a range of units, a unit being a strip of consecutive output rows of one image.  The math is
//   v_mfma_f32_16x16x32_bf16 with the weights as the A operand (16 output channels x K) and 16 consecutive output
//   pixels as the B operand: K = 2 taps x 16 channels (5 MFMAs per tile, the tenth tap zero) or, Cg = 32, one tap x 32
//   channels (9 MFMAs).  The packed weight operands (k_gconv_pack) stay in registers for the workgroup's lifetime.
// LDS.  A ring of input rows (4 slots at stride 1: three rows and the prefetched one; 5 at stride 2, which advances
//   two rows per output row), each row loaded from global memory once per unit with coalesced 16-byte loads.  A slot is
//   block-major, [4 blocks][66 pixels][32 B]: pixel iw of a row sits at position iw + 1, positions 0 and W + 1 and a
//   whole slot of a row outside the image are zero, so the MFMA loop has no boundary branch.  At stride 2 a slot is
//   split by the parity of the position (even ones first, 33 each), so a tap's 16 pixels are again consecutive.  A
//   ds_read_b128 of lane (q, j) takes 16 B of pixel j + shift, half q & 1 of the 32-B pixel; lane quarters q and q ^ 1
//   share the tap, so a group of 8 + 8 lanes reads 16 pixels' alternating halves: 256 distinct, contiguous-by-32 bytes
//   -- the pattern of k_conv_s2d_rows, conflict-free for every shift and, by the parity split, for both strides.  The
//   transposing reads of the weight gradient take 8 consecutive pixels x 32 B per 32-lane half: 256 contiguous bytes.
// Input gradient.  Stride 1 is the forward kernel on the second packed operand (taps flipped, in / out transposed
//   inside each group).  Stride 2 is the same kernel over the zero-dilated dY: the ring loader puts dY[oh][ow] at row
//   2 oh, position 2 ow + 1 and zeros elsewhere (loads through an offset past the descriptor), so dX is a gather with
//   one fixed summation order, no col2im, no atomics and no dY . W^T matrix; odd H and W need nothing special.
// Weight gradient.  k_gconv3x3_wgrad: the MFMA K runs over 32 output pixels; the dY fragment (16 outputs) and per tap
//   the X fragment (16 inputs, shifted) are read with ds_read_b64_tr_b16 (lane 4 ra + rp of group q addresses pixel
//   4 q + ra, bytes 8 rp: as k_wgrad_s2d_rows); 9 (Cg = 32: 18) accumulator tiles per wave live over the workgroup's
//   whole unit range and go to slab `workgroup` of an fp32 workspace [slabs][C / 16][NIB][9][16][16].
//   k_gconv_wgrad_reduce sums the slabs in index order and scatters the Cg x Cg diagonal blocks into torch's
//   [C][Cg][3][3] layout (beta = 1: accumulated into it).  No floating-point atomics anywhere.
#pragma once
#include "ops_nn.hip"
#include "ops_wgrad.hip"

namespace dca {
namespace ops {

constexpr int GC_SPX = 66, GC_PLANE = 33;          // positions per slot row; per parity plane at stride 2
constexpr int GC_BLK = GC_SPX * 32, GC_SLOT = 4 * GC_BLK;
constexpr int GC_DBLK = 64 * 32, GC_DY = 4 * GC_DBLK;  // weight gradient: one dY row, block-major
constexpr int GC_NT = 256;

struct GconvGeom {
  int N, H, W, C;    // the (for the dilated form: virtual) input grid and the channels
  int Ho, Wo;        // output grid
  int Hs, Ws;        // rows / pixels of the source tensor (H, W; dilated: those of dY)
  int strips;        // units per image
  int nparts;        // rows of the statistics buffer / slabs of the weight-gradient workspace
};

template <int S>
__device__ __forceinline__ int gc_pos(int pp) {  // slot position of padded pixel pp = iw + 1
  return S == 1 ? pp : (pp & 1) * GC_PLANE + (pp >> 1);
}
template <int S>
__device__ __forceinline__ int gc_tap(int kw) {  // position of output pixel 0's tap kw; pixel ow adds ow
  return S == 1 ? kw : (kw & 1) * GC_PLANE + (kw >> 1);
}
template <int S>
struct GcRing {
  static constexpr int NSLOT = S == 1 ? 4 : 5, NEW = S;  // slots; rows fetched per output row
};

typedef unsigned gc_v4u __attribute__((ext_vector_type(4)));
typedef unsigned gc_v2u __attribute__((ext_vector_type(2)));
constexpr unsigned GC_OOB = 0x80000000u;

// One input row (image n, row ih of the H x W grid) of the slab's channels: W x 8 pieces of 16 B, 2 per thread.
template <bool DIL>
__device__ __forceinline__ void gc_row_load(gc_v4u (&st)[2], const __amdgpu_buffer_rsrc_t& rs, const GconvGeom& g,
                                            int n, int ih, int c0, int nchunk) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = threadIdx.x + GC_NT * i, px = e >> 3, ch = e & 7;
    bool ok = ih >= 0 && ih < g.H && px < g.W && ch < nchunk;
    int sr = ih, sp = px;
    if (DIL) {
      ok = ok && !(ih & 1) && !(px & 1);
      sr = ih >> 1;
      sp = px >> 1;
    }
    const unsigned o = ok ? ((unsigned)((n * g.Hs + sr) * g.Ws + sp) * (unsigned)g.C + (unsigned)(c0 + 8 * ch)) * 2u
                          : GC_OOB;
    st[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
  }
}
template <int S>
__device__ __forceinline__ void gc_row_store(const gc_v4u (&st)[2], char* slot, int W, int nchunk) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = threadIdx.x + GC_NT * i, px = e >> 3, ch = e & 7;
    if (px < W && ch < nchunk) *(gc_v4u*)(slot + (ch >> 1) * GC_BLK + gc_pos<S>(px + 1) * 32 + (ch & 1) * 16) = st[i];
  }
}

__device__ __forceinline__ float gc_rowsum16(float x) {  // lane 15 of each 16-lane row: the row's sum
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x111, 0xf, 0xf, true));
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x112, 0xf, 0xf, true));
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x114, 0xf, 0xf, true));
  x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x118, 0xf, 0xf, true));
  return x;
}

// ---------------------------------------------------------------------------------------------------------
// k_gconv3x3_rows: y = conv(x) in bf16 (RNE) and, with `part`, the BN partial sums of k_conv3x3_rows' contract: row
// `workgroup` of part[nparts][C][2] holds sum(out - shift[c]) and its square over the workgroup's pixels, rows from
// gridDim.x to nparts - 1 are zeroed.  DIL: the stride-2 input gradient (x = dY on the dilated grid, STRIDE = 1).
// grid (workgroups over units, 64-channel slabs); requirements as gconv_rule (ops_api.hip), gridDim.x <= nparts.
// ---------------------------------------------------------------------------------------------------------
template <int STRIDE, bool CG32, bool DIL = false>
__global__ void __launch_bounds__(GC_NT) k_gconv3x3_rows(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wpk,
                                                         bf16_t* __restrict__ y, float* __restrict__ part,
                                                         const float* __restrict__ shift, GconvGeom g) {
  using R = GcRing<STRIDE>;
  constexpr int NS = CG32 ? 9 : 5;
  __shared__ __attribute__((aligned(16))) char smem[R::NSLOT * GC_SLOT];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
  const int c0 = 64 * blockIdx.y, nblk = min(4, (g.C - c0) / 16), nchunk = 2 * nblk;
  const bool active = w < nblk;
  const int grid = gridDim.x, vid = blockIdx.x, U = g.N * g.strips;
  const int u_beg = (int)((long long)vid * U / grid), u_end = (int)((long long)(vid + 1) * U / grid);
  for (int e = threadIdx.x; e < R::NSLOT * GC_SLOT / 16; e += GC_NT) *(gc_v4u*)(smem + e * 16) = gc_v4u{0u, 0u, 0u, 0u};
  // weights: lane (q, j) of slice s holds output channel j of the block, k = 8 q .. + 7 (k_gconv_pack's order)
  s16x8 wf[NS];
  int koff[NS], khs[NS];  // per slice: this lane's LDS offset inside a slot, and its kernel row
  const int gb = c0 / 16 + w;  // global block
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    wf[s] = active ? *(const s16x8*)((const char*)wpk + ((size_t)(gb * NS + s) * 64 + lane) * 16) : s16x8{};
    const int tap = CG32 ? s : min(2 * s + (q >> 1), 8);  // (the tenth tap's weights are zero)
    const int ib = CG32 ? ((w & ~1) + (q >> 1)) : w;
    khs[s] = tap / 3;
    koff[s] = ib * GC_BLK + (gc_tap<STRIDE>(tap % 3) + j) * 32 + (q & 1) * 16;
  }
  float sh[4], s1[4], sq[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sh[e] = (part && active) ? shift[c0 + 16 * w + 4 * q + e] : 0.f;
    s1[e] = sq[e] = 0.f;
  }
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)x, (short)0, (int)((long long)g.N * g.Hs * g.Ws * g.C * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)y, (short)0, (int)((long long)g.N * g.Ho * g.Wo * g.C * 2), 0x00020000);
  const int NF = (g.Wo + 15) / 16;
  gc_v4u st[R::NEW][2];
  for (int u = u_beg; u < u_end; ++u) {
    const int n = u / g.strips, sidx = u - n * g.strips;
    const int o_beg = (int)((long long)sidx * g.Ho / g.strips), o_end = (int)((long long)(sidx + 1) * g.Ho / g.strips);
    __syncthreads();  // the ring is zeroed / the previous unit's reads are done
    for (int d = -1; d <= 1; ++d) {
      const int ih = STRIDE * o_beg + d;
      gc_row_load<DIL>(st[0], xrs, g, n, ih, c0, nchunk);
      gc_row_store<STRIDE>(st[0], smem + ((ih + 1) % R::NSLOT) * GC_SLOT, g.W, nchunk);
    }
    __syncthreads();
    for (int oh = o_beg; oh < o_end; ++oh) {
      const bool pre = oh + 1 < o_end;
      if (pre) {
#pragma unroll
        for (int d = 0; d < R::NEW; ++d) gc_row_load<DIL>(st[d], xrs, g, n, STRIDE * oh + 2 + d, c0, nchunk);
      }
      if (active) {
        const int rb0 = ((STRIDE * oh) % R::NSLOT) * GC_SLOT, rb1 = ((STRIDE * oh + 1) % R::NSLOT) * GC_SLOT,
                  rb2 = ((STRIDE * oh + 2) % R::NSLOT) * GC_SLOT;
        for (int f = 0; f < NF; ++f) {
          f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            const int rb = khs[s] == 0 ? rb0 : (khs[s] == 1 ? rb1 : rb2);
            const s16x8 a = *(const s16x8*)(smem + rb + koff[s] + f * 512);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[s], a, acc, 0, 0, 0);
          }
          // lane (q, j): channels c0 + 16 w + 4 q + e of output pixel 16 f + j
          const int ow = 16 * f + j;
          unsigned short hv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            hv[e] = f2bf_rne(acc[e]);
            const float d = ow < g.Wo ? bf2f(hv[e]) - sh[e] : 0.f;
            s1[e] += d;
            sq[e] += d * d;
          }
          const unsigned o = ow < g.Wo ? ((unsigned)((n * g.Ho + oh) * g.Wo + ow) * (unsigned)g.C +
                                          (unsigned)(c0 + 16 * w + 4 * q)) * 2u
                                       : GC_OOB;
          __builtin_amdgcn_raw_buffer_store_b64(
              gc_v2u{hv[0] | ((unsigned)hv[1] << 16), hv[2] | ((unsigned)hv[3] << 16)}, yrs, o, 0, 0);
        }
      }
      if (pre) {
#pragma unroll
        for (int d = 0; d < R::NEW; ++d)  // slots of rows no longer read (the ring holds NSLOT consecutive rows)
          gc_row_store<STRIDE>(st[d], smem + ((STRIDE * oh + 3 + d) % R::NSLOT) * GC_SLOT, g.W, nchunk);
      }
      __syncthreads();
    }
  }
  if (part) {
    const __amdgpu_buffer_rsrc_t prs =
        __builtin_amdgcn_make_buffer_rsrc((void*)part, (short)0, (int)((long long)g.nparts * g.C * 8), 0x00020000);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float a = gc_rowsum16(s1[e]), b = gc_rowsum16(sq[e]);
      if (active && j == 15)
        __builtin_amdgcn_raw_buffer_store_b64(gc_v2u{__float_as_uint(a), __float_as_uint(b)}, prs,
                                              ((unsigned)vid * g.C + c0 + 16u * w + 4u * q + e) * 8u, 0, 0);
    }
    for (int row = grid + vid; row < g.nparts; row += grid)
      if ((int)threadIdx.x < 16 * nblk)
        __builtin_amdgcn_raw_buffer_store_b64(gc_v2u{0u, 0u}, prs, ((unsigned)row * g.C + c0 + threadIdx.x) * 8u, 0, 0);
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_gconv3x3_wgrad: per output block (wave) and tap, the 16 (out) x 16 (in) sums over the workgroup's pixels, to slab
// blockIdx.x of ws[slabs][C / 16][NIB][9][16][16] fp32 (NIB = 2 input blocks for Cg = 32, else 1).
// ---------------------------------------------------------------------------------------------------------
template <int STRIDE, bool CG32>
__global__ void __launch_bounds__(GC_NT) k_gconv3x3_wgrad(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                          float* __restrict__ ws, GconvGeom g) {
  using R = GcRing<STRIDE>;
  constexpr int NIB = CG32 ? 2 : 1;
  __shared__ __attribute__((aligned(16))) char smem[R::NSLOT * GC_SLOT + 2 * GC_DY];
  char* dyb = smem + R::NSLOT * GC_SLOT;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), j = lane & 15, q = lane >> 4;
  const int ra = j >> 2, rp = j & 3;  // transposed read: lane 4 ra + rp of its group addresses pixel row ra, bytes 8 rp
  const int c0 = 64 * blockIdx.y, nblk = min(4, (g.C - c0) / 16), nchunk = 2 * nblk;
  const bool active = w < nblk;
  const int grid = gridDim.x, vid = blockIdx.x, U = g.N * g.strips;
  const int u_beg = (int)((long long)vid * U / grid), u_end = (int)((long long)(vid + 1) * U / grid);
  for (int e = threadIdx.x; e < (R::NSLOT * GC_SLOT + 2 * GC_DY) / 16; e += GC_NT)
    *(gc_v4u*)(smem + e * 16) = gc_v4u{0u, 0u, 0u, 0u};
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)x, (short)0, (int)((long long)g.N * g.H * g.W * g.C * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)dy, (short)0, (int)((long long)g.N * g.Ho * g.Wo * g.C * 2), 0x00020000);
  auto d_load = [&](gc_v4u(&v)[2], int n, int oh) {  // dY row (n, oh): Wo x 8 pieces
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = threadIdx.x + GC_NT * i, px = e >> 3, ch = e & 7;
      const unsigned o = (oh < g.Ho && px < g.Wo && ch < nchunk)
                             ? ((unsigned)((n * g.Ho + oh) * g.Wo + px) * (unsigned)g.C + (unsigned)(c0 + 8 * ch)) * 2u
                             : GC_OOB;
      v[i] = __builtin_amdgcn_raw_buffer_load_b128(drs, o, 0, 0);
    }
  };
  auto d_store = [&](const gc_v4u(&v)[2], char* db) {  // (pixels from Wo on stay zero)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = threadIdx.x + GC_NT * i, px = e >> 3, ch = e & 7;
      if (px < g.Wo && ch < nchunk) *(gc_v4u*)(db + (ch >> 1) * GC_DBLK + px * 32 + (ch & 1) * 16) = v[i];
    }
  };
  auto frag = [&](const char* base, int p0) {  // K order: e < 4 pixel p0 + e, e >= 4 pixel p0 + 16 + e - 4 (p0 incl. 4 q)
    const s16x4 lo = lds_tr16(base + (p0 + ra) * 32 + 8 * rp), hi = lds_tr16(base + (p0 + 16 + ra) * 32 + 8 * rp);
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  f32x4 acc[NIB][9];
#pragma unroll
  for (int b = 0; b < NIB; ++b)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[b][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int NPC = (g.Wo + 31) / 32;
  const int xb0 = CG32 ? (w & ~1) : w;  // first input block of this wave's output block
  gc_v4u st[R::NEW][2], ds[2];
  int it = 0;
  for (int u = u_beg; u < u_end; ++u) {
    const int n = u / g.strips, sidx = u - n * g.strips;
    const int o_beg = (int)((long long)sidx * g.Ho / g.strips), o_end = (int)((long long)(sidx + 1) * g.Ho / g.strips);
    __syncthreads();
    for (int d = -1; d <= 1; ++d) {
      const int ih = STRIDE * o_beg + d;
      gc_row_load<false>(st[0], xrs, g, n, ih, c0, nchunk);
      gc_row_store<STRIDE>(st[0], smem + ((ih + 1) % R::NSLOT) * GC_SLOT, g.W, nchunk);
    }
    d_load(ds, n, o_beg);
    d_store(ds, dyb + (it & 1) * GC_DY);
    __syncthreads();
    for (int oh = o_beg; oh < o_end; ++oh, ++it) {
      const bool pre = oh + 1 < o_end;
      if (pre) {
#pragma unroll
        for (int d = 0; d < R::NEW; ++d) gc_row_load<false>(st[d], xrs, g, n, STRIDE * oh + 2 + d, c0, nchunk);
        d_load(ds, n, oh + 1);
      }
      if (active) {
        const char* db = dyb + (it & 1) * GC_DY + w * GC_DBLK;
        for (int pc = 0; pc < NPC; ++pc) {
          const int p0 = 32 * pc + 4 * q;
          const s16x8 a = frag(db, p0);
#pragma unroll
          for (int kh = 0; kh < 3; ++kh) {
            const char* sl = smem + ((STRIDE * oh + kh) % R::NSLOT) * GC_SLOT;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
              for (int b = 0; b < NIB; ++b) {
                const s16x8 xf = frag(sl + (xb0 + b) * GC_BLK, gc_tap<STRIDE>(kw) + p0);
                acc[b][kh * 3 + kw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, xf, acc[b][kh * 3 + kw], 0, 0, 0);
              }
          }
        }
      }
      if (pre) {
#pragma unroll
        for (int d = 0; d < R::NEW; ++d)
          gc_row_store<STRIDE>(st[d], smem + ((STRIDE * oh + 3 + d) % R::NSLOT) * GC_SLOT, g.W, nchunk);
        d_store(ds, dyb + ((it + 1) & 1) * GC_DY);  // the other dY buffer, last read by the previous output row
      }
      __syncthreads();
    }
  }
  // lane (q, j) of tile (b, t): output channel 4 q + e, input channel j of input block b, tap t
  if (active) {
    float* o = ws + (((size_t)vid * (g.C / 16) + c0 / 16 + w) * NIB) * 9 * 256;
#pragma unroll
    for (int b = 0; b < NIB; ++b)
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[(b * 9 + t) * 256 + (4 * q + e) * 16 + j] = acc[b][t][e];
  }
}

// dw[co][ci][tap] (torch [C][Cg][3][3]) = (beta ? dw : 0) + sum over slabs, in slab order, of the diagonal block entry
__global__ void __launch_bounds__(256) k_gconv_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ dw,
                                                            int C, int Cg, int slabs, int beta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * Cg * 9) return;
  const int tap = i % 9, ci = (i / 9) % Cg, co = i / (9 * Cg);
  const int nib = Cg == 32 ? 2 : 1, o = co & 15;
  const int b = Cg == 32 ? ci >> 4 : 0, in = Cg == 32 ? (ci & 15) : (o / Cg) * Cg + ci;
  const size_t slab = (size_t)(C / 16) * nib * 9 * 256;
  const float* p = ws + (((size_t)(co >> 4) * nib + b) * 9 + tap) * 256 + o * 16 + in;
  float s = 0.f;
  for (int v = 0; v < slabs; ++v) s += p[v * slab];
  dw[i] = beta ? dw[i] + s : s;
}

// The two bf16 MFMA weight operands from the fp32 master w[C][Cg][3][3], one 16-byte piece per thread: piece
// ((block * NS + s) * 64 + lane) holds, for lane (q, j), row j and k = 8 q .. + 7 of slice s:
//   forward  row = output channel 16 block + j; Cg <= 16: tap 2 s + (q >> 1), input 8 (q & 1) + e of the block (zero
//            outside the row's group, and for tap 9); Cg = 32: tap s, input 8 q + e of the group;
//   dgrad    row = input channel 16 block + j, k = output channels alike, the tap flipped (8 - tap).
__global__ void __launch_bounds__(256) k_gconv_pack(const float* __restrict__ w, bf16_t* __restrict__ fwd,
                                                    bf16_t* __restrict__ dgrad, int C, int Cg) {
  const int ns = Cg == 32 ? 9 : 5, per = (C / 16) * ns * 64;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * per) return;
  const bool dg = i >= per;
  const int p = dg ? i - per : i, lane = p & 63, s = (p >> 6) % ns, blk = (p >> 6) / ns, j = lane & 15, q = lane >> 4;
  unsigned short h[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int tap = Cg == 32 ? s : 2 * s + (q >> 1);
    const int row = 16 * blk + j;                                                    // fwd: out; dgrad: in
    const int col = Cg == 32 ? (row / 32) * 32 + 8 * q + e : 16 * blk + 8 * (q & 1) + e;  // fwd: in; dgrad: out
    float v = 0.f;
    if (tap < 9 && row / Cg == col / Cg) {
      const int co = dg ? col : row, ci = (dg ? row : col) % Cg, t = dg ? 8 - tap : tap;
      v = w[((size_t)co * Cg + ci) * 9 + t];
    }
    h[e] = f2bf_rne(v);
  }
  *(uint4*)((dg ? dgrad : fwd) + (size_t)p * 8) =
      uint4{h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16),
            h[6] | ((unsigned)h[7] << 16)};
}

}  // namespace ops
}  // namespace dca
