// Operand machinery shared by the sliced training step (netresdeep_pks.hip) and the eval-mode forward
// (netresdeep_eval.hip): the 64-B swizzled bf16 records of the 3x3 conv operands, the B-fragment load, the
// v_mfma_f32_16x16x32_bf16 product (plain bf16 or 3xbf16), the cross-lane sums and the LDS barrier.
// Everything is __forceinline__: moving it here changes no generated code.
#pragma once
#include "common.h"

namespace dca {
namespace pks {

constexpr int RB = 64;                 // bf16 record: 32 channels, 16-B chunks swizzled (rec_chunk)

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__device__ __forceinline__ unsigned short bf_lo(float v, unsigned short hi) {
  return bfbits(v - __uint_as_float((unsigned)hi << 16));
}
// Record layout of the conv operands (inputs XR, weights WT): record r = 32 bf16 channels = four 16-B chunks; chunk
// q of record r sits at chunk position q ^ 2((r >> 2) & 1).  An MFMA operand read (ds_read_b128, lane 16q + c
// reads chunk q of record base + c) then touches 16 distinct 16-B bank groups in each of the instruction's four
// 16-lane groups, for ANY base (an unswizzled record stride cannot: 80-B records conflicted 2-way).
__device__ __forceinline__ int rec_chunk(int rec, int q) { return ((rec << 6) | (q << 4)) ^ ((rec & 4) << 3); }
__device__ __forceinline__ int rec_elem(int rec, int ch) { return rec_chunk(rec, ch >> 3) + ((ch & 7) << 1); }
// one value into channel `ch` of record `rec` (both planes; `plane` = byte offset of the lo plane)
template <int P>
__device__ __forceinline__ void st1r(char* xr, int plane, int rec, int ch, float v) {
  const unsigned short hi = bfbits(v);
  const int o = rec_elem(rec, ch);
  *(unsigned short*)(xr + o) = hi;
  if constexpr (P == 1) *(unsigned short*)(xr + plane + o) = bf_lo(v, hi);
}
template <int P>
__device__ __forceinline__ f32x4 mma3(const bf16x8& ah, const bf16x8& al, const bf16x8& bh, const bf16x8& bl,
                                      f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
  if constexpr (P == 1) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
  }
  return acc;
}

// The B fragments of one conv weight (9 taps, lane 16q + c: record tap*32 + 16h + c, chunk q).  P = 0 keeps them
// in registers for a whole pass (forward / backward): the conv then reads only its A operand from LDS.
__device__ __forceinline__ int wrec_off(int h, int lane) {
  return rec_chunk(16 * h + (lane & 15), lane >> 4);  // + tap * 32 * RB (a multiple of 8 records: same swizzle)
}
__device__ __forceinline__ void load_bfrag(const char* wt, int h, int lane, bf16x8 (&bw)[9]) {
  const char* bb = wt + wrec_off(h, lane);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) bw[tap] = *(const bf16x8*)(bb + tap * 32 * RB);
}
// a + a[lane ^ 16], then + the same of lane ^ 32: the value every lane of a 16-lane column group ends with, summed in
// the order of two __shfl_xor steps (bitwise the same; fp addition is commutative) but on the gfx950 cross-row VALU
// swaps (v_permlane16_swap / v_permlane32_swap) instead of two dependent ds_bpermute LDS round trips
__device__ __forceinline__ float xsum_rows(float a) {
  const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(a), false, false);
  a = __uint_as_float(p[0]) + __uint_as_float(p[1]);
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(a), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// sum over the 16 lanes of a row, every lane ending with it: the xor-1 / 2 / 4 / 8 butterfly of __shfl_xor (the same
// pairings, so bitwise the same sums) on DPP lane moves -- quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror,
// row_mirror -- instead of four dependent ds_bpermute round trips
__device__ __forceinline__ float xsum_row16(float a) {
  a += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), 0xB1, 0xF, 0xF, false));
  a += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), 0x4E, 0xF, 0xF, false));
  a += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), 0x141, 0xF, 0xF, false));
  a += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), 0x140, 0xF, 0xF, false));
  return a;
}

}  // namespace pks
}  // namespace dca
