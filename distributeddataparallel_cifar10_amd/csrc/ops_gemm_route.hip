// GEMM dispatch of the ops layer (included by ops_api.hip after the kernels): the table of kernel instantiations and
// gemm_route(), the rule that picks one of them and its launch geometry for a GemmArgs.  gemm_route makes no HIP call
// and reads no environment variable, so it is tested without a device (dca_ops_gemm_route, tests/test_native_build.py
// against tests/golden/gemm_routes.json); docs/ARCHITECTURE.md "GEMM dispatch" follows the route_* functions' order.
#pragma once

// Every GEMM kernel instantiation, once: X(id, dynamic-LDS limit to raise (0: the default 64 KiB is enough), kernel).
// Every one takes a single GemmArgs.  The order within a family is what the route functions' id arithmetic assumes.
#define GLDS_LIMIT(BNV) (4 * GemmTile<BNV>::BUF)
#define STREAM_LIMIT (2 * (2 * G_TILE_BYTES + 8192) + 2 * 2048 * 4)
#define GEMM_KERNELS(X)                                                        \
  X(K_GEMM_128, GemmTile<128>::LDS, k_gemm<false, 128>)                        \
  X(K_GEMM_128_F8, GemmTile<128>::LDS, k_gemm<true, 128>)                      \
  X(K_GEMM_64, GemmTile<64>::LDS, k_gemm<false, 64>)                           \
  X(K_GEMM_64_F8, GemmTile<64>::LDS, k_gemm<true, 64>)                         \
  X(K_GLDS_128_W4, GLDS_LIMIT(128), k_gemm_glds<false, 128, 4>)                \
  X(K_GLDS_128_W8, GLDS_LIMIT(128), k_gemm_glds<false, 128, 8>)                \
  X(K_GLDS_128_F8_W4, GLDS_LIMIT(128), k_gemm_glds<true, 128, 4>)              \
  X(K_GLDS_128_F8_W8, GLDS_LIMIT(128), k_gemm_glds<true, 128, 8>)              \
  X(K_GLDS_64_W4, GLDS_LIMIT(64), k_gemm_glds<false, 64, 4>)                   \
  X(K_GLDS_64_W8, GLDS_LIMIT(64), k_gemm_glds<false, 64, 8>)                   \
  X(K_GLDS_64_F8_W4, GLDS_LIMIT(64), k_gemm_glds<true, 64, 4>)                 \
  X(K_GLDS_64_F8_W8, GLDS_LIMIT(64), k_gemm_glds<true, 64, 8>)                 \
  X(K_PP_256, PpTile<256>::LDS, k_gemm_pp<256>)                                \
  X(K_PP4, PP4_LDS, k_gemm_pp4<false>)                                         \
  X(K_PP4_CONV, PP4_LDS, k_gemm_pp4<true>)                                     \
  X(K_STREAM_1, STREAM_LIMIT, k_gemm_stream<2, 1, false>)                      \
  X(K_STREAM_2, STREAM_LIMIT, k_gemm_stream<2, 2, false>)                      \
  X(K_STREAM_CONV_1, STREAM_LIMIT, k_gemm_stream<2, 1, true>)                  \
  X(K_STREAM_CONV_2, STREAM_LIMIT, k_gemm_stream<2, 2, true>)                  \
  X(K_WGRAD_64_64, (WgradTile<64, 64, 2>::LDS), k_wgrad<64, 64, 2>)            \
  X(K_WGRAD_64_128, (WgradTile<64, 128, 1>::LDS), k_wgrad<64, 128, 1>)         \
  X(K_WGRAD_128_64, (WgradTile<128, 64, 4>::LDS), k_wgrad<128, 64, 4>)         \
  X(K_WGRAD_128_128, (WgradTile<128, 128, 2>::LDS), k_wgrad<128, 128, 2>)      \
  X(K_WGRAD_PP_SW, WpTile<128>::LDS, k_wgrad_pp<128, true>)                    \
  X(K_WGRAD_PP_128, WpTile<128>::LDS, k_wgrad_pp<128, false>)                  \
  X(K_WGRAD_PP_256, WpTile<256>::LDS, k_wgrad_pp<256, false>)                  \
  X(K_WGRAD3X3_1, 0, k_wgrad3x3_rows<1>)                                     \
  X(K_WGRAD3X3_2, 0, k_wgrad3x3_rows<2>)                                     \
  X(K_WGRAD3X3_128, 0, k_wgrad3x3_rows<1, 128>)                               \
  X(K_WGRAD_S2D_1, 0, k_wgrad_s2d_rows<1>)                                     \
  X(K_WGRAD_S2D_2, 0, k_wgrad_s2d_rows<2>)                                     \
  X(K_WGRAD_S2D_3, 0, k_wgrad_s2d_rows<3>)                                     \
  X(K_WGRAD_S2D_4, 0, k_wgrad_s2d_rows<4>)                                     \
  X(K_CONV_ROWS128_1, 0, k_conv3x3_rows<1, 128>)                               \
  X(K_CONV_ROWS128_2, 0, k_conv3x3_rows<2, 128>)                               \
  X(K_CONV_ROWS_1, 0, k_conv3x3_rows<1>)                                       \
  X(K_CONV_ROWS_2, 0, k_conv3x3_rows<2>)                                       \
  X(K_CONV_ROWS_3, 0, k_conv3x3_rows<3>)                                       \
  X(K_CONV_ROWS_4, 0, k_conv3x3_rows<4>)                                       \
  X(K_CONV_S2D_1, 0, k_conv_s2d_rows<1>)                                       \
  X(K_CONV_S2D_2, 0, k_conv_s2d_rows<2>)                                       \
  X(K_CONV_S2D_3, 0, k_conv_s2d_rows<3>)                                       \
  X(K_CONV_S2D_4, 0, k_conv_s2d_rows<4>)                                       \
  X(K_CONV_S2D_5, 0, k_conv_s2d_rows<5>)                                       \
  X(K_CONV_S2D_6, 0, k_conv_s2d_rows<6>)                                       \
  X(K_CONV_S2D_7, 0, k_conv_s2d_rows<7>)                                       \
  X(K_CONV_S2D_8, 0, k_conv_s2d_rows<8>)                                       \
  X(K_DIRECT_STEM, 0, k_direct_conv<16, 4, 4>)                                 \
  X(K_DIRECT_3X3, (DirectConv<64, 3, 3>::LDS), k_direct_conv<64, 3, 3>)

enum GemmKernel {
#define X(ID, LIM, ...) ID,
  GEMM_KERNELS(X)
#undef X
  K_COUNT
};
inline const char* const GEMM_KERNEL_NAMES[K_COUNT] = {
#define X(ID, LIM, ...) #__VA_ARGS__,
    GEMM_KERNELS(X)
#undef X
};

// What dca_ops_gemm does for one GemmArgs.  Must match ops/_native.py::GemmRoute.
struct GemmRoute {
  int kernel;        // GemmKernel
  const char* name;  // GEMM_KERNEL_NAMES[kernel]
  int grid_x, grid_y, block, lds;
  int splits, k_per_split, single, stages;  // the GemmArgs fields the kernel is launched with
  int masked_copy;                          // k_masked_copy first (beta_src / beta_mask then cleared)
  int reduce;                               // k_gemm_splitk_reduce after
};

namespace route {
using namespace dca::ops;
#define ROUTE_REQUIRE(c, msg) \
  do {                        \
    if (!(c)) return msg;     \
  } while (0)

// glds single-buffer mode (32 KiB LDS: ~1.5x the resident workgroups) for short K: K-tiles per split <= 9.
// Batch-256 census vs double-buffered: K <= 576 0.78-0.91x time, K = 1152 0.93x, K = 1024-4608 0.97-1.23x.
constexpr int GLDS_SINGLE_NK = 9;
// register-staged kernel: single LDS buffer up to this many K-tiles per split
constexpr int REG_SINGLE_NK = 4;
// glds K pipeline: 2 LDS buffers (3-4 measured 1.4-1.6x slower on the long-K shapes: fewer resident waves)
constexpr int GLDS_STAGES = 2;

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int ring_nf(int nf, int max) { return nf >= 1 && nf < max ? nf : max; }  // row fragments: the kernels' NF
inline void launch(GemmRoute* r, int kernel, long grid_x, int grid_y, int block, int lds) {
  r->kernel = kernel;
  r->grid_x = (int)grid_x, r->grid_y = grid_y;
  r->block = block, r->lds = lds;
}

// ---- 1. weight-gradient row-ring kernels (g is a weight gradient: see gemm_route) -------------------------------
// the 64-channel 3 x 3 / pad 1 weight gradient on rows <= 64 pixels: the row-ring kernel (k_wgrad3x3_rows), one
// split slab per workgroup
inline bool route_wgrad_rows64(GemmArgs& g, int ncu, GemmRoute* r) {
  if (!(g.conv == 2 && g.cC == 64 && g.cKH == 3 && g.cKW == 3 && g.cP == 1 && g.cS == 1 && g.cW <= 64 &&
        g.cHo == g.cH && g.cWo == g.cW && g.M == 64 && g.N == 576 && g.K == g.cN * g.cH * g.cW && g.lda % 8 == 0 &&
        g.lda >= 64 && aligned16(g.A) && aligned16(g.B) && (long long)g.cN * g.cH * g.cW * g.lda * 2 < (1LL << 31) &&
        (long long)g.cN * g.cH * g.cW * 128 < (1LL << 31)))
    return false;
  const long cg = std::min<long>(std::min<long>(g.splits, 2L * ncu), (long)g.cN * g.cH);
  g.splits = (int)cg;
  launch(r, g.cW <= 32 ? K_WGRAD3X3_1 : K_WGRAD3X3_2, cg, 1, CR_NT, WR_LDS);
  return true;
}
// the 128-channel 3 x 3 / pad 1 weight gradient on rows <= 32 pixels (layer 2): k_wgrad3x3_rows<1, 128>,
// two workgroups (output-channel halves) per split slab, one workgroup per CU
inline bool route_wgrad_rows128(GemmArgs& g, int ncu, GemmRoute* r) {
  if (!(g.conv == 2 && g.cC == 128 && g.cKH == 3 && g.cKW == 3 && g.cP == 1 && g.cS == 1 && g.cW <= 32 &&
        g.cHo == g.cH && g.cWo == g.cW && g.M == 128 && g.N == 1152 && g.K == g.cN * g.cH * g.cW && g.lda % 8 == 0 &&
        g.lda >= 128 && aligned16(g.A) && aligned16(g.B) && (long long)g.cN * g.cH * g.cW * g.lda * 2 < (1LL << 31) &&
        (long long)g.cN * g.cH * g.cW * 256 < (1LL << 31)))
    return false;
  const long cg = std::min<long>(std::min<long>(g.splits, ncu / 2), (long)g.cN * g.cH);
  g.splits = (int)cg;
  launch(r, K_WGRAD3X3_128, 2 * cg, 1, WgradRows<128>::NT, WgradRows<128>::LDS);
  return true;
}
// the space-to-depth stem's weight gradient (4 x 4 taps over 16 channels) on rows <= 128 input pixels:
// k_wgrad_s2d_rows, one split slab per workgroup
inline bool route_wgrad_s2d(GemmArgs& g, int ncu, GemmRoute* r) {
  if (!(g.conv == 2 && g.cC == 16 && g.cKH == 4 && g.cKW == 4 && g.cP == 0 && g.cS == 1 && g.cW <= 128 &&
        g.cHo == g.cH - 3 && g.cWo == g.cW - 3 && g.M == 64 && g.N == 256 && g.K == g.cN * g.cHo * g.cWo &&
        g.lda % 8 == 0 && g.lda >= 64 && aligned16(g.A) && aligned16(g.B) &&
        (long long)g.cN * g.cHo * g.cWo * g.lda * 2 < (1LL << 31) && (long long)g.cN * g.cH * g.cW * 32 < (1LL << 31)))
    return false;
  const long cg = std::min<long>(std::min<long>(g.splits, 3L * ncu), (long)g.cN * g.cHo);
  g.splits = (int)cg;
  launch(r, K_WGRAD_S2D_1 + ring_nf((g.cWo + 31) >> 5, 4) - 1, cg, 1, CR_NT, WS_LDS);
  return true;
}
// ---- 2. k_wgrad_pp ----------------------------------------------------------------------------------------------
// weight gradients with M >= 256 (and the swapped 1x1 forms) on the ping-pong LDS-DMA kernel k_wgrad_pp
// (0.71-0.92x the k_wgrad time on every routed shape); the 64-wide / swapped implicit forms stay on k_wgrad
// (1.4-1.7x slower on k_wgrad_pp, profiles/wgrad_pp_r3.log).
// The larger of M (output channels) / N (input channels x taps) goes along its 256-row side
// (SW: N), the smaller one as a 256 / 128 column tile; 32-bit operand offsets, 16-B aligned rows.  The split
// count is cut to about one workgroup per CU (one fits per CU).  Shape rule from bench/wgrad_bench.py at batch
// 256 (profiles/wgrad_pp_r3.log): M >= 256, N >= 128 -> 0.71-0.92x the k_wgrad time (3x3 256x2304x50176 123.4
// -> 92.1 us); swapped only for plain (1x1) operands with 64 < M <= 128 (0.89-0.92x); the swapped implicit 3x3
// convolutions (1.5-1.7x) and the 64-wide column tile (1.0-1.7x) measured slower and stay on k_wgrad
inline bool route_wgrad_pp(GemmArgs& g, GemmRoute* r) {
  const long long a_by = (long long)g.K * g.lda * 2;
  const long long b_by = g.conv == 2 ? (long long)g.cN * g.cH * g.cW * g.cC * 2 : (long long)g.K * g.ldb * 2;
  const bool sw = g.M < 256;
  const int big = sw ? g.N : g.M, small = sw ? g.M : g.N;
  const bool pp_shape = sw ? (g.conv != 2 && small > 64 && small <= 128 && big >= 256) : (big >= 256 && small >= 128);
  if (!(pp_shape && a_by < (1LL << 31) && b_by < (1LL << 31) && aligned16(g.A) && aligned16(g.B) &&
        (g.conv != 2 || g.cC % 8 == 0)))
    return false;
  const int pbn = sw ? 128 : ((small % 256 == 0 || small > 1024) ? 256 : 128);
  const long tiles = (long)((big + WP_BM - 1) / WP_BM) * ((small + pbn - 1) / pbn);
  const long want = std::max<long>(1, (256 + tiles - 1) / tiles);
  if (want < g.splits) {  // fewer, longer splits (the slab was sized for g.splits: smaller is fine)
    int kps = (int)((g.K + want - 1) / want);
    kps = (kps + WP_KT - 1) / WP_KT * WP_KT;
    g.k_per_split = kps;
    g.splits = (g.K + kps - 1) / kps;
  }
  // (the four-slot k32 ring schedule of k_gemm_pp4 measured 20-30 % slower here: each interval would carry
  // 24 transposed fragment reads and 6 DMA pieces, longer than the other group's 32 MFMAs;
  // profiles/gemm_ring_ab_r7.log)
  launch(r, sw ? K_WGRAD_PP_SW : pbn == 256 ? K_WGRAD_PP_256 : K_WGRAD_PP_128, tiles * g.splits, 1, WP_NT,
         pbn == 256 ? WpTile<256>::LDS : WpTile<128>::LDS);
  return true;
}
// ---- 3. k_wgrad: every other weight gradient -------------------------------------------------------------------
inline const char* route_wgrad(GemmArgs& g, GemmRoute* r) {
  const int bm = g.M <= 64 ? 64 : 128, bn = g.N <= 64 ? 64 : 128;
  const long items = (long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn) * g.splits;
  ROUTE_REQUIRE(items < (1L << 31), "gemm: too many work items");
  // single-buffer weight-gradient kernel: the loop is latency-bound, so more resident workgroups per CU win
  // (batch-256 census: M = 64 weight gradients 845 -> 580 us, 835 -> 556 us): half the tile's LDS
  g.single = 1;
  constexpr int lds[4] = {WgradTile<64, 64, 2>::LDS >> 1, WgradTile<64, 128, 1>::LDS >> 1,
                          WgradTile<128, 64, 4>::LDS >> 1, WgradTile<128, 128, 2>::LDS >> 1};
  const int v = 2 * (bm == 128) + (bn == 128);
  launch(r, K_WGRAD_64_64 + v, items, 1, 256, lds[v]);
  return nullptr;
}
// ---- 4. forward row-ring kernels ---------------------------------------------------------------------------------
// the 128-channel 3 x 3 / pad 1 convs on rows <= 32 pixels (ResNet-50's layer 2 at 28 x 28, forward and input
// gradient) -> the row-ring kernel k_conv3x3_rows<NF, 128> (one 8-wave workgroup per CU)
inline bool route_conv_rows128(const GemmArgs& g, int ncu, GemmRoute* r) {
  if (!(g.conv == 1 && g.cC == 128 && g.cKH == 3 && g.cKW == 3 && g.cP == 1 && g.cS == 1 && g.cW <= 32 &&
        g.cHo == g.cH && g.cWo == g.cW && g.N == 128 && g.K == 1152 && !g.fp8 && !g.tb && g.splits == 1 &&
        g.wperm_T <= 0 && g.orow_S <= 0 && g.out_bf16 && !g.relu && g.beta == 0.f && !g.beta_mask && g.ldb >= g.K &&
        g.ldb % 8 == 0 && g.ldc >= 128 && g.ldc % 8 == 0 && aligned16(g.A) && aligned16(g.B) && aligned16(g.C) &&
        (long long)g.cN * g.cH * g.cW * 256 < (1LL << 31) && (long long)g.M * g.ldc * 2 < (1LL << 31) &&
        g.M < (1 << 24)))
    return false;
  long cg = std::min<long>(ncu, (long)g.cN * g.cH);
  if (g.col_stats) cg = std::min<long>(cg, (g.M + GBM - 1) / GBM);
  launch(r, g.cW <= 16 ? K_CONV_ROWS128_1 : K_CONV_ROWS128_2, cg, 1, RowConv<128>::NT, RowConv<128>::LDS);
  return true;
}
// stride-1 implicit convs with 64 outputs on narrow input rows: the space-to-depth ResNet stem (4 x 4 taps over 16
// channels) and the 64-channel 3 x 3 / pad 1 convolutions (layer 1 forward and input gradient); what the row-ring
// forms below and k_direct_conv all need
inline bool dc_stem(const GemmArgs& g) { return g.cC == 16 && g.cKH == 4 && g.cKW == 4 && g.cP == 0; }
inline bool dc_3x3(const GemmArgs& g) { return g.cC == 64 && g.cKH == 3 && g.cKW == 3 && g.cP == 1; }
inline bool direct_conv_ok(const GemmArgs& g) {
  // (the kernel loops over the compile-time K = KH KW C: an mnk override or a padded K must not reach it)
  return g.conv == 1 && (dc_stem(g) || dc_3x3(g)) && g.K == g.cKH * g.cKW * g.cC && g.cS == 1 && g.N == 64 &&
         !g.fp8 && !g.tb && g.splits == 1 && g.wperm_T <= 0 && g.orow_S <= 0 && g.out_bf16 && !g.relu &&
         g.beta == 0.f && !g.beta_mask && g.ldb >= g.K && g.ldb % 8 == 0 && g.ldc >= 64 && g.ldc % 8 == 0 &&
         aligned16(g.A) && aligned16(g.B) && aligned16(g.C) && (long long)g.cN * g.cH * g.cW * g.cC * 2 < (1LL << 31) &&
         (long long)g.M * g.ldc * 2 < (1LL << 31) && g.M < (1 << 24);
}
// the row-ring forms (k_conv3x3_rows on rows <= 64 pixels: the layer-1 shapes; k_conv_s2d_rows on rows <= 128: the
// stem), three workgroups per CU over the image rows
inline bool route_conv_rows(const GemmArgs& g, int ncu, GemmRoute* r) {
  const bool r3 = dc_3x3(g) && g.cW <= 64;
  if (!(direct_conv_ok(g) && (r3 || (dc_stem(g) && g.cW <= 128)))) return false;
  long cg = std::min<long>(3L * ncu, (long)g.cN * (r3 ? g.cH : g.cHo));
  if (g.col_stats) cg = std::min<long>(cg, (g.M + GBM - 1) / GBM);  // one statistics row per workgroup
  if (r3) launch(r, K_CONV_ROWS_1 + ring_nf((g.cW + 15) >> 4, 4) - 1, cg, 1, CR_NT, CR_LDS);
  else launch(r, K_CONV_S2D_1 + ring_nf((g.cWo + 15) >> 4, 8) - 1, cg, 1, CR_NT, CS_LDS);
  return true;
}
// ---- 5. k_direct_conv: the same convs on wider rows --------------------------------------------------------------
inline bool route_direct_conv(const GemmArgs& g, int ncu, GemmRoute* r) {
  if (!direct_conv_ok(g)) return false;
  const long blocks = (g.M + GBM - 1) / GBM;
  long grid = std::min<long>(2L * ncu, (blocks + 7) / 8 * 8);
  grid = std::max<long>(8, grid / 8 * 8);
  if (dc_stem(g)) launch(r, K_DIRECT_STEM, grid, 1, DC_NT, DirectConv<16, 4, 4>::LDS);
  else launch(r, K_DIRECT_3X3, grid, 1, DC_NT, DirectConv<64, 3, 3>::LDS);
  return true;
}
// ---- 6. k_gemm_stream --------------------------------------------------------------------------------------------
// persistent stream kernel (k_gemm_stream), bf16 -> bf16, K % 64 == 0, no split / remap / ReLU:
//   plain NT, N % 128 == 0: by default for K <= 512 and M >= 16384, accumulating (beta) calls only for K <= 128
//     (the output-heavy 1x1 convolutions and their input gradients; profiles/gemm_shortk_r2.log);
//   N = 64: 256 x 64 tiles (802816 x 64 x 256: 123.4 -> 109.1 us);
//   implicit conv with C % 64 == 0, N = 128: M >= 16384 (ResNet-50's layer-2 3x3 convolutions and their input
//     gradients: 129.5 -> 117.5 us at batch 256).  The N = 64 conv stays on the one-tile kernel unless forced
//     (DCA_OPS_STREAM=1, diagnostic): 174 us there, 218 us with 128 x 64 stream tiles, 283 us with 256 x 64
//   the strided 1x1 (downsample) convs with N % 128 == 0 and M >= 16384 (256x56x56x256 -> 512: 177 -> 126 us,
//     256x28x28x512 -> 1024: 116 -> 101 us; 256x14x14x1024 -> 2048, M = 12544, stays on pp4: 82 vs 95 us;
//     profiles/stream_downsample_ab_r8f.log)
// sk (DCA_OPS_STREAM): 0 never, 1 every eligible shape, 2 the shape rule
inline bool route_stream(const GemmArgs& g, int ncu, int sk, GemmRoute* r) {
  const bool conv = g.conv == 1;
  const long long ab = conv ? (long long)g.cN * g.cH * g.cW * g.cC * 2 : ((long long)(g.M - 1) * g.lda + g.K) * 2;
  const long long bb = ((long long)(g.N - 1) * g.ldb + g.K) * 2;
  const long long cbytes = (long long)g.M * g.ldc * 2;
  const int mw = g.N % 128 == 0 ? 1 : 2;  // 128 x 128 tiles, or 256 x 64 for N % 128 == 64
  const bool shape_ok = conv ? (g.cC % 64 == 0 && g.cKH * g.cKW <= 32 &&
                                (g.N == 64 || g.N == 128 || (g.cKH * g.cKW == 1 && g.N % 128 == 0)) &&
                                g.orow_S <= 0 &&
                                g.M < (1 << 24) &&
                                (sk == 1 || (sk == 2 && g.M >= 16384 &&
                                             (g.N == 128 || (g.cKH * g.cKW == 1 && g.N % 128 == 0)))))
                             : (g.conv == 0 && !g.ta && g.lda % 8 == 0 && g.lda >= g.K &&
                                (g.N % 128 == 0 || g.N == 64) &&
                                (sk == 1 || (g.K <= 512 && g.M >= 16384 &&
                                             (g.beta == 0.f || g.K <= 128 || (g.beta_mask && g.K <= 256)))));
  const bool st_ok = sk != 0 && shape_ok && !g.fp8 && !g.tb && g.splits == 1 && g.wperm_T <= 0 && g.orow_S <= 0 &&
                     !(conv && g.beta_mask) &&
                     !g.relu && g.out_bf16 && g.N % 64 == 0 && g.N <= 2048 && g.K % 64 == 0 &&
                     g.K > 0 && g.M > 0 && g.ldb % 8 == 0 && g.ldc % 8 == 0 && g.ldb >= g.K && g.ldc >= g.N &&
                     aligned16(g.A) && aligned16(g.B) && aligned16(g.C) &&
                     ab < (1LL << 31) && bb < (1LL << 31) && cbytes < (1LL << 31) &&
                     (long long)((g.M + GBM - 1) / GBM) * g.N * 8 < (1LL << 31);
  if (!st_ok) return false;
  const long tiles = (long)((g.M + GBM * mw - 1) / (GBM * mw)) * (g.N / (128 / mw));
  long grid = std::min<long>(2L * ncu, (tiles + 7) / 8 * 8);  // two resident workgroups per CU
  grid = std::max<long>(8, grid / 8 * 8);
  const int lds = 2 * (GBM * mw * 128 + (128 / mw) * 128) + 2 * g.N * 4;  // 2 x (A | B) + bias | shift
  launch(r, K_STREAM_1 + 2 * conv + (mw - 1), grid, 1, ST_NT, lds);
  return true;
}
// ---- 7. k_gemm_pp4 / k_gemm_pp -----------------------------------------------------------------------------------
// ping-pong 256 x 256 kernel: bf16, K-contiguous operands (plain or the C % 64 implicit conv), no split-K / row
// remap / fused BN-backward statistics, 16-B aligned rows, operands addressable with 32-bit offsets
inline bool route_pingpong(const GemmArgs& g, GemmRoute* r) {
  const long long ab = g.conv == 1 ? (long long)g.cN * g.cH * g.cW * g.cC * 2 : ((long long)(g.M - 1) * g.lda + g.K) * 2;
  const long long bb = ((long long)(g.N - 1) * g.ldb + g.K) * 2;
  // shape rule (no wasted MFMA columns, >= 160 of the 256 CUs busy, K >= 1024 to amortise the pipeline fill and
  // the 256-row epilogue): measured 4096^3 779 -> 1037 TF, 3x3 conv 256x14x14x256 109 -> 81.6 us; the ResNet-50
  // batch-256 census (profiles/gemm_pingpong_r2.log) loses on N = 128 (+54 %), 98-tile grids (+38 %) and
  // K = 256 (+20 %), wins on 50176 x 256 x {1024, 2304} (-8 %, -21 %)
  // N % 256 != 0 (e.g. 128): the 256 x 128 tile
  const int ppbn = g.N % 256 == 0 ? 256 : 128;
  const long pp_tiles = (long)((g.M + PP_BM - 1) / PP_BM) * ((g.N + ppbn - 1) / ppbn);
  // (a 256 x 128 tile measured slower than the 128 x 128 kernels on every ResNet-50 N = 128 shape, +12-18 %:
  // 16 MFMAs per barrier interval do not cover the other group's fragment loads; removed in round 5)
  // with k_gemm_pp4 the rule also takes 512 <= K < 1024 (12544 x 2048 x 512 53.3 -> 46.1 us, 12544 x 1024 x 512
  // 34.8 -> 25.4; below 160 tiles it still loses to the 128 x 128 kernels: profiles/gemm_ring_ab_r7.log)
  const bool pp_shape = ppbn == 256 && pp_tiles >= 160 && g.K >= 512;
  const bool pp = pp_shape && !g.fp8 && !g.ta && !g.tb && g.splits == 1 && g.wperm_T <= 0 && g.orow_S <= 0 &&
                  g.M >= 256 && g.N >= 128 && g.K >= 256 && ab < (1LL << 31) && bb < (1LL << 31) &&
                  (long)g.ldb * 2 % 16 == 0 && aligned16(g.A) && aligned16(g.B) &&
                  (g.conv == 1 ? (g.cC % 64 == 0 && g.cKH * g.cKW <= 32 && g.M < (1 << 24))
                               : (g.conv == 0 && (long)g.lda * 2 % 16 == 0 && (long)g.K * 2 % 16 == 0));
  if (!pp) return false;
  // K % 64 == 0: the four-slot k32 ring form (k_gemm_pp4); else the two-buffer k_gemm_pp
  if (g.K % 64 == 0) launch(r, g.conv == 1 ? K_PP4_CONV : K_PP4, pp_tiles, 1, PP_NT, PP4_LDS);
  else launch(r, K_PP_256, pp_tiles, 1, PP_NT, PpTile<256>::LDS);
  return true;
}
// ---- 8. k_gemm_glds / k_gemm: everything else --------------------------------------------------------------------
inline void route_tile(GemmArgs& g, int kt, GemmRoute* r) {
  // narrow N (<= 64) with a K-contiguous B operand: the 128x64 tile
  const bool narrow = g.N <= 64 && !g.tb && g.conv != 2;
  const int bn = narrow ? 64 : 128;
  const int tiles = ((g.M + GBM - 1) / GBM) * ((g.N + bn - 1) / bn);
  g.single = g.k_per_split <= REG_SINGLE_NK * kt ? 1 : 0;  // short K: one buffer, 2x workgroups per CU
  // K-contiguous operands with 16-B aligned rows: direct global -> LDS staging (k_gemm_glds)
  const int esz = g.fp8 ? 1 : 2;
  // (measured, bench/gemm_bench.py: +18..100 % on plain NT GEMMs; bf16 implicit convs only when C % 64 == 0 (one
  // tap per K-tile: a wave-uniform decode; neutral at batch 64, +2..6 % per conv GEMM at batch 256); fp8 implicit
  // convs always (the register-staged fp8 kernel needs 219 VGPRs: one wave per SIMD); narrow (128 x 64) short-K
  // GEMMs too: 0.89-0.90x the register-staged time at batch 256 (802816 x 64 x {64, 256}))
  const bool glds = !g.ta && !g.tb &&
                    (g.conv == 1 ? (g.fp8 || g.cC % 64 == 0)
                                 : (g.conv == 0 && (long)g.lda * esz % 16 == 0 && (long)g.K * esz % 16 == 0)) &&
                    (long)g.ldb * esz % 16 == 0 && aligned16(g.A) && aligned16(g.B);
  if (!glds) {
    launch(r, K_GEMM_128 + 2 * narrow + (g.fp8 != 0), tiles, g.splits, GT,
           narrow ? (g.single ? GemmTile<64>::LDS_SINGLE : GemmTile<64>::LDS)
                  : (g.single ? GemmTile<128>::LDS_SINGLE : GemmTile<128>::LDS));
    return;
  }
  g.single = g.k_per_split <= GLDS_SINGLE_NK * kt ? 1 : 0;
  g.stages = g.single ? 1 : GLDS_STAGES;
  // 8 waves (4 per SIMD at 2 workgroups per CU) for the double-buffered long-K loops: 0.92-0.95x time on the
  // batch-256 long-K convs; the single-buffer short-K launches keep 4 (8 measured 1.13-1.41x there)
  const bool w8 = !g.single;
  const int nt = w8 ? 512 : 256;
  // the epilogue's column-statistics combine uses (threads / (BN / 8)) x BN float2 of LDS
  const int lds = narrow ? std::max(g.single ? GemmTile<64>::LDS_SINGLE : g.stages * GemmTile<64>::BUF, nt / 8 * 64 * 8)
                         : std::max(g.single ? GemmTile<128>::LDS_SINGLE : g.stages * GemmTile<128>::BUF,
                                    nt / 16 * 128 * 8);
  launch(r, K_GLDS_128_W4 + 4 * narrow + 2 * (g.fp8 != 0) + w8, tiles, g.splits, nt, lds);
}
}  // namespace route

// The kernel, launch geometry and rewritten GemmArgs fields for one GEMM on a device of `ncu` compute units;
// stream_mode is DCA_OPS_STREAM (route_stream).  An error string for a shape the kernels cannot take, else null.
inline const char* gemm_route(const GemmArgs& a, int ncu, int stream_mode, GemmRoute* r) {
  using namespace route;
  GemmArgs g = a;
  ROUTE_REQUIRE(g.M > 0 && g.N > 0 && g.K > 0, "gemm: empty problem");
  ROUTE_REQUIRE(!g.fp8 || (!g.ta && !g.tb), "gemm: fp8 operands must be K-contiguous (ta = tb = 0)");
  ROUTE_REQUIRE(!g.fp8 || (g.K % 16 == 0 && (g.conv == 1 || g.lda % 16 == 0) && g.ldb % 16 == 0),
                "gemm: fp8 needs K, lda, ldb % 16 == 0");
  ROUTE_REQUIRE(g.conv == 1 || g.ta || g.lda >= g.K, "gemm: lda < K");
  ROUTE_REQUIRE(g.conv == 2 || !g.tb || g.ldb >= g.N, "gemm: ldb < N (transposed B)");
  ROUTE_REQUIRE(g.conv == 2 || g.tb || g.ldb >= g.K, "gemm: ldb < K");
  ROUTE_REQUIRE(g.conv == 1 || !g.ta || g.lda >= g.M, "gemm: lda < M (transposed A)");
  ROUTE_REQUIRE(g.ldc >= g.N, "gemm: ldc < N");
  ROUTE_REQUIRE(g.conv >= 0 && g.conv <= 2, "gemm: bad conv mode");
  ROUTE_REQUIRE(g.conv != 1 || g.K < (1 << 24), "gemm: implicit conv K >= 2^24");
  if (g.conv) {
    ROUTE_REQUIRE(g.cC > 0 && (g.fp8 ? (g.conv == 1 && g.cC % 16 == 0) : g.cC % 8 == 0),
                  "gemm: implicit conv needs C % 8 == 0 (bf16) or an fp8 forward with C % 16 == 0");
    // a sub-pixel input-gradient class (orow_S > 0) relies on the gather's bounds checks for its one-sided
    // padding, so its output grid is only bounded; otherwise the usual convolution arithmetic
    ROUTE_REQUIRE(g.orow_S > 0 ? (g.conv == 1 && g.cHo >= 1 && g.cWo >= 1 && g.cHo <= g.cH && g.cWo <= g.cW)
                               : (g.cHo == (g.cH + 2 * g.cP - g.cKH) / g.cS + 1 && g.cWo == (g.cW + 2 * g.cP - g.cKW) / g.cS + 1),
                  "gemm: inconsistent conv geometry");
    const long pix = (long)g.cN * g.cHo * g.cWo, kc = (long)g.cKH * g.cKW * g.cC;
    ROUTE_REQUIRE(g.conv != 1 || (g.M == pix && g.K == kc && !g.ta), "gemm: conv A shape mismatch");
    ROUTE_REQUIRE(g.conv != 2 || (g.K == pix && g.N == kc && !g.tb), "gemm: conv B shape mismatch");
  }
  ROUTE_REQUIRE(!g.col_stats || (g.stats_shift && g.splits <= 1), "gemm: column stats need a shift and no split-K");
  ROUTE_REQUIRE(!g.beta_mask || (g.beta_src && g.beta_src != g.C && g.beta != 0.f && g.out_bf16 && !g.ta &&
                                 g.splits <= 1 && g.wperm_T <= 0 && g.orow_S <= 0 && g.N % 8 == 0 && g.ldc % 8 == 0 &&
                                 ((uintptr_t)g.beta_src & 15) == 0),
                "gemm: a masked accumulation source needs a separate 16-B aligned bf16 source, beta != 0 and a plain "
                "bf16 output with N, ldc % 8 == 0");
  ROUTE_REQUIRE(g.orow_S <= 0 || (g.splits <= 1 && g.wperm_T <= 0 && g.orow_Ho > 0 && g.orow_Wo > 0 &&
                                  (long)g.orow_Ho * g.orow_Wo > 0 && g.M % ((long)g.orow_Ho * g.orow_Wo) == 0 &&
                                  g.orow_S * (g.orow_Ho - 1) + g.orow_ph < g.orow_H &&
                                  g.orow_S * (g.orow_Wo - 1) + g.orow_pw < g.orow_W),
                "gemm: output row remap needs the epilogue path and a consistent pixel grid");
  const int kt = GBK_BYTES / (g.fp8 ? 1 : 2);
  if (g.splits < 1) g.splits = 1;
  ROUTE_REQUIRE(g.wperm_T <= 0 || (g.ws && !g.col_stats && g.wperm_C > 0 && g.wperm_Cpad >= g.wperm_C),
                "gemm: weight-layout remap needs a workspace and no column stats");
  if (g.splits > 1) {
    ROUTE_REQUIRE(g.ws != nullptr, "gemm: split-K needs a workspace");
    int kps = (g.K + g.splits - 1) / g.splits;
    kps = (kps + kt - 1) / kt * kt;
    g.k_per_split = kps;
    g.splits = (g.K + kps - 1) / kps;
  } else {
    g.k_per_split = g.K;
  }
  r->masked_copy = r->reduce = 0;
  // weight gradients (both operands pixel-major, bf16, 16-B aligned channel rows): the transposed-read kernels,
  // always through the slab + reduce pass
  const bool wgrad = !g.fp8 && g.ta && (g.tb || g.conv == 2) && g.M % 8 == 0 && g.N % 8 == 0 && g.lda % 8 == 0 &&
                     (g.conv == 2 || g.ldb % 8 == 0) && g.ws != nullptr;
  if (wgrad) {
    ROUTE_REQUIRE(g.conv != 2 || (long)g.cN * g.cHo * g.cWo < (1L << 24), "gemm: weight-gradient pixel count >= 2^24");
    r->reduce = 1;
    if (!(route_wgrad_rows64(g, ncu, r) || route_wgrad_rows128(g, ncu, r) || route_wgrad_s2d(g, ncu, r) ||
          route_wgrad_pp(g, r)))
      if (const char* e = route_wgrad(g, r)) return e;
  } else if (!(route_conv_rows128(g, ncu, r) || route_conv_rows(g, ncu, r) || route_direct_conv(g, ncu, r) ||
               route_stream(g, ncu, stream_mode, r))) {
    // the other kernels read C_old from C: the masked source is materialised there first (k_masked_copy)
    r->masked_copy = g.beta_mask != nullptr;
    if (!route_pingpong(g, r)) {
      route_tile(g, kt, r);
      r->reduce = g.splits > 1 || g.wperm_T > 0;
    }
  }
  r->name = GEMM_KERNEL_NAMES[r->kernel];
  r->splits = g.splits;
  r->k_per_split = g.k_per_split;
  r->single = g.single;
  r->stages = g.stages;
  return nullptr;
}
