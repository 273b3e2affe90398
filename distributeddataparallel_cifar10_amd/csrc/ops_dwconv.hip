// Depthwise 3 x 3 convolution (groups == C, pad 1, stride 1 or 2) over NHWC bf16 activations, C % 8 == 0, input rows
// of at most 128 pixels: every depthwise layer of MobileNetV1 at a 224 input.  There is no reduction over channels: 9
// multiply-adds per output element, bound by its bytes (x read once, y written once).  No matrix instruction fits (an
// MFMA needs a K dimension; a 16 x 16 block-diagonal tile at Cg = 1 is 94 % zeros), so the math is fp32 VALU on
// two-channel pairs (v_pk_fma_f32 / v_pk_mul_f32) and the design is about moving each byte once.
//
// Work split.  The unit of channels is the 16-byte chunk of 8.  A workgroup of 256 threads owns a slab of CH = 4, 8 or
//   16 chunks (32 / 64 / 128 channels) and a range of units, a unit being a strip of consecutive output rows of one
//   image.  Thread t owns chunk t % CH and output column t / CH for the workgroup's lifetime; its 9 x 8 weights are
//   read from the fp32 master weight, rounded to bf16 (RNE) and kept as fp32 in registers (no packed operand, no pack
//   launch).  CH follows the row width so that the 256 / CH columns cover the row: 4 chunks x 64 columns up to 64
//   output pixels, the same with two columns per thread (NC = 2: col and col + 64) up to 128, 8 x 32 and 16 x 16 for
//   the narrow, channel-rich layers (28, 14 and 7 pixels), whose rows would leave three quarters of a 64-column
//   workgroup idle.  The slab is 32 channels at W = 128 so that the ring (33 KB at stride 1, 42 KB at stride 2) lets
//   three workgroups share a CU's 160 KB; a 64-channel slab would allow one at stride 2.
//   Workgroups are numbered slab-fastest, so the slabs that share an input row's cache lines run at the same time.
// LDS.  A ring of input rows (4 slots at stride 1, 5 at stride 2, prefetched one output row ahead), each row fetched
//   once per unit with coalesced 16-byte buffer loads; a row or pixel outside the image returns zero through the
//   descriptor.  A slot is pixel-major, [W + 2 positions][CH chunks][16 B]: pixel iw sits at position iw + 1,
//   positions 0 and W + 1 and the rows outside the image are zero, so the tap loop has no boundary branch.  At stride
//   2 a slot is split by the parity of the position (DwPlan::pos / tap, as gc_pos / gc_tap), so a tap's pixels are
//   consecutive again.  Banks: a thread reads a tap with ds_read_b128 at (tap + col) * 16 CH + 16 chunk; 16 consecutive
//   lanes are 16 / CH consecutive columns x CH chunks = 256 contiguous bytes = the 64 banks once each, for every tap
//   shift and, by the parity split, both strides.
// Row reuse.  Walking down its column a thread carries partial sums, not taps: at stride 1 the new input row oh + 1
//   finishes output row oh (kh = 2), continues oh + 1 (kh = 1) and starts oh + 2 (kh = 0), so an output row costs three
//   LDS reads, not nine, and the carried state is 16 registers per column where two rows of taps would be 48.  At
//   stride 2 row 2 oh + 1 finishes oh and starts oh + 1: two rows read per output row, not three.  Every output sums
//   its taps in the order kh, kw; every pass has one fixed order, so a step repeats bit for bit.  No atomics.
// BN partial sums (ST): the contract of k_gconv3x3_rows / k_conv3x3_rows.  A thread accumulates sum(out - shift) and
//   its square for its 8 channels over its pixels (out: the bf16-rounded value); the columns of a chunk are summed
//   through LDS in column order (dw_chunk_sum: 8 segments, then the 8 segment sums).
// Input gradient.  Stride 1: the forward kernel with the taps flipped (a flipped weight read).  Stride 2
//   (k_dwconv3x3_dgrad2): a gather over dY by parity tap sets.  dX row ih takes kh = 1 from dY row ih / 2 when even,
//   kh = 0 from (ih + 1) / 2 and kh = 2 from (ih - 1) / 2 when odd; columns alike, so a dX pixel costs 1, 2, 2 or 4
//   taps.  A workgroup walks dY rows r: dX rows 2 r and 2 r + 1 (parity is workgroup-uniform), thread column j writes
//   dX columns 2 j, then 2 j + 1 (a wave stores one column parity at a time), from dY positions j and j + 1 of rows r
//   (carried in registers) and r + 1.  Rows / columns H, W past an odd size are simply not written; dY row Ho reads as
//   zero through the descriptor.  Every dX element is written exactly once: no memset, no col2im.
// Weight gradient.  k_dwconv3x3_wgrad: the x ring plus a double-buffered dY row; a thread keeps 9 x 8 fp32 sums over
//   all its units, the columns of a chunk are summed through LDS in column order into slab `workgroup` of an fp32
//   workspace [slabs][C][9], and k_dwconv_wgrad_reduce sums the slabs in index order into torch's [C][1][3][3].
#pragma once
#include "ops_nn.hip"

namespace dca {
namespace ops {

constexpr int DW_NT = 256;
constexpr unsigned DW_OOB = 0x80000000u;
typedef float dw_f2 __attribute__((ext_vector_type(2)));
typedef unsigned dw_v4u __attribute__((ext_vector_type(4)));
typedef unsigned dw_v2u __attribute__((ext_vector_type(2)));

struct DwGeom {
  int N, H, W, C;  // input grid and channels
  int Ho, Wo;      // output grid
  int strips;      // units per image
  int nparts;      // rows of the statistics buffer / slabs of the weight-gradient workspace
};

template <int S, int LC, int NC>
struct DwPlan {
  static constexpr int CH = 1 << LC, COLS = DW_NT >> LC;       // chunks per slab; thread columns
  static constexpr int WMAX = S == 1 ? NC * COLS : 2 * COLS;   // widest input row (W * CH <= 512 pieces)
  static constexpr int WOMAX = NC * COLS;                      // widest output row
  static constexpr int PLANE = WMAX / 2 + 1, SPX = S == 1 ? WMAX + 2 : 2 * PLANE;
  static constexpr int PX = 16 * CH, SLOT = SPX * PX;          // bytes per position; per slot
  static constexpr int NSLOT = S == 1 ? 4 : 5, NEW = S;        // slots; rows fetched per output row
  static constexpr int DYB = WOMAX * PX;                       // weight gradient: one dY row
  __device__ static __forceinline__ int pos(int pp) {          // slot position of padded pixel pp = iw + 1
    return S == 1 ? pp : (pp & 1) * PLANE + (pp >> 1);
  }
  __device__ static __forceinline__ int tap(int kw) {          // position of output pixel 0's tap kw; pixel ow adds ow
    return S == 1 ? kw : (kw & 1) * PLANE + (kw >> 1);
  }
};

// One row (image n, row r of a rows x width grid) of the slab's channels: width x CH pieces of 16 B, 2 per thread.
template <int LC>
__device__ __forceinline__ void dw_row_load(dw_v4u (&st)[2], const __amdgpu_buffer_rsrc_t& rs, int rows, int width,
                                            int C, int n, int r, int c0, int nchunk) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = threadIdx.x + DW_NT * i, px = e >> LC, ch = e & ((1 << LC) - 1);
    const bool ok = r >= 0 && r < rows && px < width && ch < nchunk;
    const unsigned o = ok ? ((unsigned)((n * rows + r) * width + px) * (unsigned)C + (unsigned)(c0 + 8 * ch)) * 2u
                          : DW_OOB;
    st[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
  }
}
template <class P, int LC>
__device__ __forceinline__ void dw_row_store(const dw_v4u (&st)[2], char* slot, int width, int nchunk) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = threadIdx.x + DW_NT * i, px = e >> LC, ch = e & ((1 << LC) - 1);
    if (px < width && ch < nchunk) *(dw_v4u*)(slot + P::pos(px + 1) * P::PX + ch * 16) = st[i];
  }
}

__device__ __forceinline__ void dw_cvt(dw_f2 (&f)[4], const dw_v4u v) {  // 8 bf16 -> 4 fp32 pairs
#pragma unroll
  for (int k = 0; k < 4; ++k) f[k] = dw_f2{__uint_as_float(v[k] << 16), __uint_as_float(v[k] & 0xffff0000u)};
}
// The three taps (kw 0, 1, 2) of one slot row as fp32; a += w[0] * tap 0 + w[1] * tap 1 + w[2] * tap 2, in that order
template <class P>
__device__ __forceinline__ void dw_taps(dw_f2 (&t)[3][4], const char* p) {
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) dw_cvt(t[kw], *(const dw_v4u*)(p + P::tap(kw) * P::PX));
}
__device__ __forceinline__ void dw_fma3(dw_f2 (&a)[4], const dw_f2 (*w)[4], const dw_f2 (&t)[3][4]) {
#pragma unroll
  for (int kw = 0; kw < 3; ++kw)
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = __builtin_elementwise_fma(w[kw][k], t[kw][k], a[k]);
}

// The thread's 9 x 8 weights: fp32 master w[C][1][3][3] rounded to bf16 (RNE); flip: tap 8 - t (stride-1 dgrad)
__device__ __forceinline__ void dw_weights(dw_f2 (&wv)[9][4], const float* __restrict__ w, int cb, bool active,
                                           int flip) {
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ti = flip ? 8 - t : t;
      wv[t][k] = active ? dw_f2{bf2f(f2bf_rne(w[(cb + 2 * k) * 9 + ti])), bf2f(f2bf_rne(w[(cb + 2 * k + 1) * 9 + ti]))}
                        : dw_f2{0.f, 0.f};
    }
}

// Sum of v[i] over the 256 / CH threads (columns) of each chunk, in column order: 8 segments of consecutive columns,
// then the 8 segment sums.  Thread tid < 8 CH receives the sum of chunk tid / 8, element tid % 8.  buf: 12 KB of LDS.
template <int LC>
__device__ __forceinline__ float dw_chunk_sum(float* buf, const float (&v)[8]) {
  constexpr int CH = 1 << LC, COLS = DW_NT >> LC, NVAL = 8 * CH, SEG = COLS / 8;
  const int chunk = threadIdx.x & (CH - 1), col = threadIdx.x >> LC;
  __syncthreads();  // (whatever read this memory before is done)
#pragma unroll
  for (int i = 0; i < 8; ++i) buf[col * NVAL + chunk * 8 + i] = v[i];
  __syncthreads();
  for (int it = threadIdx.x; it < 8 * NVAL; it += DW_NT) {
    const int val = it % NVAL, seg = it / NVAL;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < SEG; ++k) s += buf[(seg * SEG + k) * NVAL + val];
    buf[DW_NT * 8 + seg * NVAL + val] = s;
  }
  __syncthreads();
  float r = 0.f;
  if ((int)threadIdx.x < NVAL)
#pragma unroll
    for (int seg = 0; seg < 8; ++seg) r += buf[DW_NT * 8 + seg * NVAL + threadIdx.x];
  return r;
}

// ---------------------------------------------------------------------------------------------------------
// k_dwconv3x3_rows: y = conv(x) in bf16 (RNE) and, ST, the BN partial sums: row `workgroup` of part[nparts][C][2]
// holds sum(out - shift[c]) and its square over the workgroup's pixels, rows from the workgroups per slab to
// nparts - 1 are zeroed.  flip: the stride-1 input gradient (x = dY).  grid: (workgroups per slab) x slabs, slab
// fastest; requirements as dwconv_rule (ops_api.hip), workgroups per slab <= nparts, W <= WMAX, Wo <= WOMAX.
// ---------------------------------------------------------------------------------------------------------
template <int S, int LC, int NC, bool ST>
__global__ void __launch_bounds__(DW_NT, NC == 1 ? 3 : 2) k_dwconv3x3_rows(const bf16_t* __restrict__ x, const float* __restrict__ w,
                                                          bf16_t* __restrict__ y, float* __restrict__ part,
                                                          const float* __restrict__ shift, DwGeom g, int flip) {
  using P = DwPlan<S, LC, NC>;
  __shared__ __attribute__((aligned(16))) char smem[P::NSLOT * P::SLOT];
  const int chunk = threadIdx.x & (P::CH - 1), col = threadIdx.x >> LC;
  const int nslab = (g.C + 8 * P::CH - 1) / (8 * P::CH);
  const int slab = blockIdx.x % nslab, vid = blockIdx.x / nslab, grid = gridDim.x / nslab;
  const int c0 = 8 * P::CH * slab, nchunk = min(P::CH, (g.C - c0) / 8), cb = c0 + 8 * chunk;
  const bool active = chunk < nchunk;
  const int U = g.N * g.strips;
  const int u_beg = (int)((long long)vid * U / grid), u_end = (int)((long long)(vid + 1) * U / grid);
  for (int e = threadIdx.x; e < P::NSLOT * P::SLOT / 16; e += DW_NT) *(dw_v4u*)(smem + e * 16) = dw_v4u{0u, 0u, 0u, 0u};
  dw_f2 wv[9][4];
  dw_weights(wv, w, cb, active, flip);
  float sh[8], s1[8], sq[8];
  if (ST) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sh[e] = active ? shift[cb + e] : 0.f;
      s1[e] = sq[e] = 0.f;
    }
  }
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)x, (short)0, (int)((long long)g.N * g.H * g.W * g.C * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)y, (short)0, (int)((long long)g.N * g.Ho * g.Wo * g.C * 2), 0x00020000);
  const int toff = col * P::PX + chunk * 16;  // this thread's byte offset inside a slot, before the tap
  dw_v4u st[P::NEW][2];
  dw_f2 ca[NC][4], cn[NC][4];  // carried partial sums: of output row oh; stride 1: of row oh + 1
  for (int u = u_beg; u < u_end; ++u) {
    const int n = u / g.strips, sidx = u - n * g.strips;
    const int o_beg = (int)((long long)sidx * g.Ho / g.strips), o_end = (int)((long long)(sidx + 1) * g.Ho / g.strips);
    __syncthreads();  // the ring is zeroed / the previous unit's reads are done
    for (int d = -1; d <= 1; ++d) {
      const int ih = S * o_beg + d;
      dw_row_load<LC>(st[0], xrs, g.H, g.W, g.C, n, ih, c0, nchunk);
      dw_row_store<P, LC>(st[0], smem + ((ih + 1) % P::NSLOT) * P::SLOT, g.W, nchunk);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NC; ++k) {  // rows S o_beg - 1 (kh 0) and, stride 1, o_beg (kh 1; kh 0 of the next row)
      const char* p = smem + toff + k * P::COLS * P::PX;
#pragma unroll
      for (int q = 0; q < 4; ++q) ca[k][q] = cn[k][q] = dw_f2{0.f, 0.f};
      dw_f2 t[3][4];
      dw_taps<P>(t, p + ((S * o_beg) % P::NSLOT) * P::SLOT);
      dw_fma3(ca[k], &wv[0], t);
      if (S == 1) {
        dw_taps<P>(t, p + ((o_beg + 1) % P::NSLOT) * P::SLOT);
        dw_fma3(ca[k], &wv[3], t);
        dw_fma3(cn[k], &wv[0], t);
      }
    }
    for (int oh = o_beg; oh < o_end; ++oh) {
      const bool pre = oh + 1 < o_end;
      if (pre) {
#pragma unroll
        for (int d = 0; d < P::NEW; ++d) dw_row_load<LC>(st[d], xrs, g.H, g.W, g.C, n, S * oh + 2 + d, c0, nchunk);
      }
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int ow = col + k * P::COLS;
        if (active && ow < g.Wo) {
          const char* p = smem + toff + k * P::COLS * P::PX;
          dw_f2 t[3][4];
          if (S == 2) {
            dw_taps<P>(t, p + ((S * oh + 1) % P::NSLOT) * P::SLOT);  // input row 2 oh: kh 1
            dw_fma3(ca[k], &wv[3], t);
          }
          dw_taps<P>(t, p + ((S * oh + 2) % P::NSLOT) * P::SLOT);  // input row S oh + 1: kh 2, finishes row oh
          dw_fma3(ca[k], &wv[6], t);
          unsigned short hv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            hv[e] = f2bf_rne(ca[k][e >> 1][e & 1]);
            if (ST) {
              const float d = bf2f(hv[e]) - sh[e];
              s1[e] += d;
              sq[e] += d * d;
            }
          }
          __builtin_amdgcn_raw_buffer_store_b128(
              dw_v4u{hv[0] | ((unsigned)hv[1] << 16), hv[2] | ((unsigned)hv[3] << 16), hv[4] | ((unsigned)hv[5] << 16),
                     hv[6] | ((unsigned)hv[7] << 16)},
              yrs, ((unsigned)((n * g.Ho + oh) * g.Wo + ow) * (unsigned)g.C + (unsigned)cb) * 2u, 0, 0);
#pragma unroll
          for (int q = 0; q < 4; ++q) {  // the same row continues oh + 1 (stride 1: kh 1, and starts oh + 2)
            ca[k][q] = S == 1 ? cn[k][q] : dw_f2{0.f, 0.f};
            cn[k][q] = dw_f2{0.f, 0.f};
          }
          if (S == 1) {
            dw_fma3(ca[k], &wv[3], t);
            dw_fma3(cn[k], &wv[0], t);
          } else {
            dw_fma3(ca[k], &wv[0], t);
          }
        }
      }
      if (pre) {
#pragma unroll
        for (int d = 0; d < P::NEW; ++d)  // slots of rows no longer read (the ring holds NSLOT consecutive rows)
          dw_row_store<P, LC>(st[d], smem + ((S * oh + 3 + d) % P::NSLOT) * P::SLOT, g.W, nchunk);
      }
      __syncthreads();
    }
  }
  if (ST) {
    const __amdgpu_buffer_rsrc_t prs =
        __builtin_amdgcn_make_buffer_rsrc((void*)part, (short)0, (int)((long long)g.nparts * g.C * 8), 0x00020000);
    const float a = dw_chunk_sum<LC>((float*)smem, s1);
    const float b = dw_chunk_sum<LC>((float*)smem, sq);
    if ((int)threadIdx.x < 8 * nchunk) {
      __builtin_amdgcn_raw_buffer_store_b64(dw_v2u{__float_as_uint(a), __float_as_uint(b)}, prs,
                                            ((unsigned)vid * g.C + c0 + threadIdx.x) * 8u, 0, 0);
      for (int row = grid + vid; row < g.nparts; row += grid)
        __builtin_amdgcn_raw_buffer_store_b64(dw_v2u{0u, 0u}, prs, ((unsigned)row * g.C + c0 + threadIdx.x) * 8u, 0, 0);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_dwconv3x3_dgrad2: the stride-2 input gradient dx [N][H][W][C] from dy [N][Ho][Wo][C] by parity tap sets (header).
// A unit is a strip of dY rows r: dX rows 2 r and 2 r + 1.  Thread column j: dX columns 2 j and 2 j + 1, so
// W <= 2 * (256 / CH).  A slot is [Wo + 2 positions][CH][16 B] of one dY row, pixel ow at position ow + 1.
// ---------------------------------------------------------------------------------------------------------
template <int LC>
__global__ void __launch_bounds__(DW_NT) k_dwconv3x3_dgrad2(const bf16_t* __restrict__ dy, const float* __restrict__ w,
                                                            bf16_t* __restrict__ dx, DwGeom g) {
  using P = DwPlan<1, LC, 1>;  // (the stride-1 slot: COLS + 2 positions)
  __shared__ __attribute__((aligned(16))) char smem[4 * P::SLOT];
  const int chunk = threadIdx.x & (P::CH - 1), j = threadIdx.x >> LC;
  const int nslab = (g.C + 8 * P::CH - 1) / (8 * P::CH);
  const int slab = blockIdx.x % nslab, vid = blockIdx.x / nslab, grid = gridDim.x / nslab;
  const int c0 = 8 * P::CH * slab, nchunk = min(P::CH, (g.C - c0) / 8), cb = c0 + 8 * chunk;
  const bool active = chunk < nchunk && 2 * j < g.W, odd = 2 * j + 1 < g.W;
  const int U = g.N * g.strips;
  const int u_beg = (int)((long long)vid * U / grid), u_end = (int)((long long)(vid + 1) * U / grid);
  for (int e = threadIdx.x; e < 4 * P::SLOT / 16; e += DW_NT) *(dw_v4u*)(smem + e * 16) = dw_v4u{0u, 0u, 0u, 0u};
  dw_f2 wv[9][4];
  dw_weights(wv, w, cb, chunk < nchunk, 0);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)dy, (short)0, (int)((long long)g.N * g.Ho * g.Wo * g.C * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)dx, (short)0, (int)((long long)g.N * g.H * g.W * g.C * 2), 0x00020000);
  const int toff = (j + 1) * P::PX + chunk * 16;  // dY pixel j; pixel j + 1 is one position on
  auto emit = [&](const dw_f2(&v)[4], int n, int ih, int iw) {
    unsigned short hv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) hv[e] = f2bf_rne(v[e >> 1][e & 1]);
    __builtin_amdgcn_raw_buffer_store_b128(
        dw_v4u{hv[0] | ((unsigned)hv[1] << 16), hv[2] | ((unsigned)hv[3] << 16), hv[4] | ((unsigned)hv[5] << 16),
               hv[6] | ((unsigned)hv[7] << 16)},
        xrs, ((unsigned)((n * g.H + ih) * g.W + iw) * (unsigned)g.C + (unsigned)cb) * 2u, 0, 0);
  };
  dw_v4u st[2];
  dw_f2 cur[2][4], nxt[2][4];  // dY pixels j, j + 1 of rows r and r + 1
  for (int u = u_beg; u < u_end; ++u) {
    const int n = u / g.strips, sidx = u - n * g.strips;
    const int o_beg = (int)((long long)sidx * g.Ho / g.strips), o_end = (int)((long long)(sidx + 1) * g.Ho / g.strips);
    __syncthreads();
    for (int d = 0; d < 2; ++d) {
      dw_row_load<LC>(st, drs, g.Ho, g.Wo, g.C, n, o_beg + d, c0, nchunk);
      dw_row_store<P, LC>(st, smem + ((o_beg + d) & 3) * P::SLOT, g.Wo, nchunk);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) dw_cvt(cur[i], *(const dw_v4u*)(smem + (o_beg & 3) * P::SLOT + toff + i * P::PX));
    for (int r = o_beg; r < o_end; ++r) {
      const bool pre = r + 1 < o_end;
      if (pre) dw_row_load<LC>(st, drs, g.Ho, g.Wo, g.C, n, r + 2, c0, nchunk);
#pragma unroll
      for (int i = 0; i < 2; ++i) dw_cvt(nxt[i], *(const dw_v4u*)(smem + ((r + 1) & 3) * P::SLOT + toff + i * P::PX));
      if (active) {
        dw_f2 v[4];
        // row 2 r (even: kh 1, dY row r); columns 2 j (kw 1, pixel j), then 2 j + 1 (kw 0: pixel j + 1; kw 2: pixel j)
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = wv[4][q] * cur[0][q];
        emit(v, n, 2 * r, 2 * j);
        if (odd) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = __builtin_elementwise_fma(wv[5][q], cur[0][q], wv[3][q] * cur[1][q]);
          emit(v, n, 2 * r, 2 * j + 1);
        }
        if (2 * r + 1 < g.H) {  // row 2 r + 1 (odd: kh 0, dY row r + 1; kh 2, dY row r)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = __builtin_elementwise_fma(wv[7][q], cur[0][q], wv[1][q] * nxt[0][q]);
          emit(v, n, 2 * r + 1, 2 * j);
          if (odd) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              dw_f2 a = wv[0][q] * nxt[1][q];
              a = __builtin_elementwise_fma(wv[2][q], nxt[0][q], a);
              a = __builtin_elementwise_fma(wv[6][q], cur[1][q], a);
              v[q] = __builtin_elementwise_fma(wv[8][q], cur[0][q], a);
            }
            emit(v, n, 2 * r + 1, 2 * j + 1);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[i][q] = nxt[i][q];
      if (pre) dw_row_store<P, LC>(st, smem + ((r + 2) & 3) * P::SLOT, g.Wo, nchunk);  // the slot of row r - 2
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_dwconv3x3_wgrad: per channel and tap the sum of x * dy over the workgroup's pixels, to slab `workgroup` of
// ws[slabs][C][9] fp32.  grid as k_dwconv3x3_rows.
// ---------------------------------------------------------------------------------------------------------
template <int S, int LC, int NC>
__global__ void __launch_bounds__(DW_NT) k_dwconv3x3_wgrad(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                           float* __restrict__ ws, DwGeom g) {
  using P = DwPlan<S, LC, NC>;
  __shared__ __attribute__((aligned(16))) char smem[P::NSLOT * P::SLOT + 2 * P::DYB];
  char* dyb = smem + P::NSLOT * P::SLOT;
  const int chunk = threadIdx.x & (P::CH - 1), col = threadIdx.x >> LC;
  const int nslab = (g.C + 8 * P::CH - 1) / (8 * P::CH);
  const int slab = blockIdx.x % nslab, vid = blockIdx.x / nslab, grid = gridDim.x / nslab;
  const int c0 = 8 * P::CH * slab, nchunk = min(P::CH, (g.C - c0) / 8);
  const bool active = chunk < nchunk;
  const int U = g.N * g.strips;
  const int u_beg = (int)((long long)vid * U / grid), u_end = (int)((long long)(vid + 1) * U / grid);
  for (int e = threadIdx.x; e < (P::NSLOT * P::SLOT + 2 * P::DYB) / 16; e += DW_NT)
    *(dw_v4u*)(smem + e * 16) = dw_v4u{0u, 0u, 0u, 0u};
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)x, (short)0, (int)((long long)g.N * g.H * g.W * g.C * 2), 0x00020000);
  const __amdgpu_buffer_rsrc_t drs = __builtin_amdgcn_make_buffer_rsrc(
      (void*)dy, (short)0, (int)((long long)g.N * g.Ho * g.Wo * g.C * 2), 0x00020000);
  auto d_store = [&](const dw_v4u(&v)[2], char* db) {  // dY pixel ow at position ow (pixels from Wo on stay zero)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = threadIdx.x + DW_NT * i, px = e >> LC, ch = e & (P::CH - 1);
      if (px < g.Wo && ch < nchunk) *(dw_v4u*)(db + px * P::PX + ch * 16) = v[i];
    }
  };
  dw_f2 acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[t][q] = dw_f2{0.f, 0.f};
  const int toff = col * P::PX + chunk * 16;
  dw_v4u st[P::NEW][2], ds[2];
  int it = 0;
  for (int u = u_beg; u < u_end; ++u) {
    const int n = u / g.strips, sidx = u - n * g.strips;
    const int o_beg = (int)((long long)sidx * g.Ho / g.strips), o_end = (int)((long long)(sidx + 1) * g.Ho / g.strips);
    __syncthreads();
    for (int d = -1; d <= 1; ++d) {
      const int ih = S * o_beg + d;
      dw_row_load<LC>(st[0], xrs, g.H, g.W, g.C, n, ih, c0, nchunk);
      dw_row_store<P, LC>(st[0], smem + ((ih + 1) % P::NSLOT) * P::SLOT, g.W, nchunk);
    }
    dw_row_load<LC>(ds, drs, g.Ho, g.Wo, g.C, n, o_beg, c0, nchunk);
    d_store(ds, dyb + (it & 1) * P::DYB);
    __syncthreads();
    for (int oh = o_beg; oh < o_end; ++oh, ++it) {
      const bool pre = oh + 1 < o_end;
      if (pre) {
#pragma unroll
        for (int d = 0; d < P::NEW; ++d) dw_row_load<LC>(st[d], xrs, g.H, g.W, g.C, n, S * oh + 2 + d, c0, nchunk);
        dw_row_load<LC>(ds, drs, g.Ho, g.Wo, g.C, n, oh + 1, c0, nchunk);
      }
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int ow = col + k * P::COLS;
        if (active && ow < g.Wo) {
          dw_f2 d[4];
          dw_cvt(d, *(const dw_v4u*)(dyb + (it & 1) * P::DYB + toff + k * P::COLS * P::PX));
#pragma unroll
          for (int kh = 0; kh < 3; ++kh) {
            const char* p = smem + ((S * oh + kh) % P::NSLOT) * P::SLOT + toff + k * P::COLS * P::PX;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
              dw_f2 t[4];
              dw_cvt(t, *(const dw_v4u*)(p + P::tap(kw) * P::PX));
#pragma unroll
              for (int q = 0; q < 4; ++q) acc[kh * 3 + kw][q] = __builtin_elementwise_fma(t[q], d[q], acc[kh * 3 + kw][q]);
            }
          }
        }
      }
      if (pre) {
#pragma unroll
        for (int d = 0; d < P::NEW; ++d)
          dw_row_store<P, LC>(st[d], smem + ((S * oh + 3 + d) % P::NSLOT) * P::SLOT, g.W, nchunk);
        d_store(ds, dyb + ((it + 1) & 1) * P::DYB);  // the other dY buffer, last read by the previous output row
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = acc[t][e >> 1][e & 1];
    const float r = dw_chunk_sum<LC>((float*)smem, v);
    if ((int)threadIdx.x < 8 * nchunk) ws[((size_t)vid * g.C + c0 + threadIdx.x) * 9 + t] = r;
  }
}

// dw[c][tap] (torch [C][1][3][3]) = (beta ? dw : 0) + sum over slabs, in slab order
__global__ void __launch_bounds__(256) k_dwconv_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ dw, int C,
                                                             int slabs, int beta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * 9) return;
  float s = 0.f;
  for (int v = 0; v < slabs; ++v) s += ws[(size_t)v * C * 9 + i];
  dw[i] = beta ? dw[i] + s : s;
}

}  // namespace ops
}  // namespace dca
