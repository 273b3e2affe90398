// C ABI of the ops layer (libdca_ops.so), driven from ops/_native.py with torch-allocated tensors and the
// caller's HIP stream.  Every entry point validates what the kernels assume about shapes before launching
// (a bad shape is an error string, never an out-of-bounds access on the GPU).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <cstdlib>
#include <cstdint>

#include "ops_nn.hip"
#include "ops_wgrad.hip"

namespace {
thread_local std::string g_err;
#define OPCK(x)                                              \
  do {                                                       \
    hipError_t e_ = (x);                                     \
    if (e_ != hipSuccess) {                                  \
      g_err = std::string(#x) + ": " + hipGetErrorString(e_); \
      return -1;                                             \
    }                                                        \
  } while (0)
#define REQUIRE(c, msg)  \
  do {                   \
    if (!(c)) {          \
      g_err = msg;       \
      return -1;         \
    }                    \
  } while (0)

inline int grid_for(long work, int per_block = 256, int cap = 8192) {
  long b = (work + per_block - 1) / per_block;
  return (int)std::max(1L, std::min(b, (long)cap));
}
// Dispatch policy.  Every rule was chosen by measurement (docs/ARCHITECTURE.md "GEMM dispatch") and lives in
// ops_gemm_route.hip; the A/B environment switches are gone, except DCA_OPS_STREAM, kept as the diagnostic A/B of the
// persistent short-K kernel that is still being tuned (0 never, 1 every eligible shape, unset: the shape rule).
inline int getenv_stream() {  // persistent short-K GEMM (k_gemm_stream): DCA_OPS_STREAM = 0 never, 1 whenever
  static const int v = [] {    // eligible, 2 (default) by the shape rule (route_stream)
    const char* e = getenv("DCA_OPS_STREAM");
    return e ? atoi(e) : 2;
  }();
  return v;
}
// Compute units of the current device, cached per device id (racing first calls store the same value)
int cu_count(int* ncu) {
  static std::atomic<int> cache[64];
  int dev = 0;
  OPCK(hipGetDevice(&dev));
  const bool cached = dev >= 0 && dev < 64;
  *ncu = cached ? cache[dev].load(std::memory_order_relaxed) : 0;
  if (!*ncu) {
    OPCK(hipDeviceGetAttribute(ncu, hipDeviceAttributeMultiprocessorCount, dev));
    if (cached) cache[dev].store(*ncu, std::memory_order_relaxed);
  }
  return 0;
}
// finalize threads per workgroup: 1024 when one workgroup reduces one channel's partial rows (C < 256)
#define BN_FIN_NTH(CW) ((CW) == 1 ? 1024 : 256)

// Per-shape policy of the BN passes, all of it in bn_plan below: a pure function of the shape and the fused form (no
// HIP call, no environment), exported as dca_ops_bn_plan and tested against a hand-written table on the CPU
// (tests/test_native_build.py); every launcher below takes its kernel and grid from the plan.
//   lanes          16 channel lanes (256 contiguous bytes per row and wave instruction) when C % 128 == 0, else 8
//   forward apply  tensors of >= 2^26 elements (16 lanes) stream with non-temporal loads / stores and take 128 rows
//                  per workgroup; every other tensor the default cache policy and BN_ROWS = 256 rows
//   backward stats non-temporal under the same rule; always BN_ROWS rows (one partial row per workgroup)
//   backward apply 16 lanes and >= 2^25 elements: 128 rows per workgroup (twice the workgroups) and non-temporal;
//                  else 256 rows and the default policy
//   bwd_mode       how dz is recovered: the stored mask when there is one, else recomputed (BWD_RES for
//                  ReLU(bn + r), BWD_RELU for the other ReLU forms), BWD_PLAIN without ReLU; -1 where
//                  dca_ops_bn_bwd rejects the form (a join without ReLU, a mask on any other form than
//                  ReLU(bn + r) or the plain BN that feeds one)
//   raff           the residual's own BN applied on the fly (BnRes), res_mode 2 only
// Measured on bench/micro/bn_micro.hip (profiles/bn_micro_r4s.log; same box, ResNet-50 batch-256 shapes): NT
// statistics 181.6 -> 145.5 us, residual apply 251.6 -> 209.5 us at 802816 x 256; backward apply 104.5 -> 84.2 us
// at 50176 x 1024.  Smaller tensors are re-read while still in the Infinity Cache.  Same box, whole step: 10,292 ->
// 10,494 img/s (profiles/resnet50_bntune_ab_r4t.log).
using namespace dca::ops;
struct BnPlan {  // must match ops/_native.py::BnPlan
  int lanes;                       // 8 | 16
  int apply_rows, apply_nt, raff;  // k_bn_apply<lanes, apply_rows, apply_nt, raff>
  int bwd_mode;                    // BWD_PLAIN..BWD_MASK, -1: no backward for this form
  int bwd_stats_nt;                // k_bn_bwd_stats<lanes, bwd_mode, bwd_stats_nt>
  int bwd_rows, bwd_apply_nt;      // k_bn_bwd_apply<lanes, bwd_mode, bwd_rows, bwd_apply_nt>
};
// nullptr and *out, or the reason the shape is rejected
inline const char* bn_plan(long M, int C, int relu, int res_mode, int has_mask, int raff, BnPlan* out) {
  if (M < 1 || C < 8 || C % 8 != 0) return "bn: M >= 1 rows of C channels, C a multiple of 8";
  if (res_mode < 0 || res_mode > 2) return "bn: res_mode is 0, 1 or 2";
  if (raff && res_mode != 2) return "bn: an on-the-fly residual BN needs res_mode 2";
  const bool wide = C % 128 == 0;
  const bool nt = wide && M * C >= (1L << 26), fine = wide && M * C >= (1L << 25);
  BnPlan p;
  p.lanes = wide ? 16 : 8;
  p.apply_rows = nt ? 128 : BN_ROWS;
  p.apply_nt = nt;
  p.raff = raff != 0;
  if (res_mode == 2 && !relu) p.bwd_mode = -1;
  else if (has_mask) p.bwd_mode = (relu && res_mode == 2) || (!relu && res_mode == 0) ? BWD_MASK : -1;
  else if (relu) p.bwd_mode = res_mode == 2 ? BWD_RES : BWD_RELU;
  else p.bwd_mode = BWD_PLAIN;
  p.bwd_stats_nt = nt;
  p.bwd_rows = fine ? 128 : BN_ROWS;
  p.bwd_apply_nt = fine;
  *out = p;
  return nullptr;
}
inline dim3 bn_grid(const BnPlan& p, long M, int C, int rows) {
  return dim3((unsigned)((C + 8 * p.lanes - 1) / (8 * p.lanes)), (unsigned)((M + rows - 1) / rows));
}
template <int CL, typename... A>
void bn_stats_launch_t(const BnPlan& p, dim3 g, hipStream_t st, A... a) {
#define BST(MO)                                                                                          \
  if (p.bwd_stats_nt) hipLaunchKernelGGL((k_bn_bwd_stats<CL, MO, true>), g, dim3(256), 0, st, a...);     \
  else hipLaunchKernelGGL((k_bn_bwd_stats<CL, MO, false>), g, dim3(256), 0, st, a...)
  switch (p.bwd_mode) {
    case BWD_PLAIN: BST(BWD_PLAIN); break;
    case BWD_RELU: BST(BWD_RELU); break;
    case BWD_RES: BST(BWD_RES); break;
    default: BST(BWD_MASK); break;
  }
#undef BST
}
template <typename... A>
void bn_stats_launch(const BnPlan& p, long M, int C, hipStream_t st, A... a) {
  const dim3 g = bn_grid(p, M, C, BN_ROWS);
  if (p.lanes == 16) bn_stats_launch_t<16>(p, g, st, a...);
  else bn_stats_launch_t<8>(p, g, st, a...);
}
template <int CL, typename... A>
void bn_bwd_apply_launch_t(const BnPlan& p, dim3 g, hipStream_t st, A... a) {
#define BAP(MO)                                                                                                \
  if (p.bwd_rows == 128) hipLaunchKernelGGL((k_bn_bwd_apply<CL, MO, 128, true>), g, dim3(256), 0, st, a...);   \
  else hipLaunchKernelGGL((k_bn_bwd_apply<CL, MO, BN_ROWS, false>), g, dim3(256), 0, st, a...)
  switch (p.bwd_mode) {
    case BWD_PLAIN: BAP(BWD_PLAIN); break;
    case BWD_RELU: BAP(BWD_RELU); break;
    case BWD_RES: BAP(BWD_RES); break;
    default: BAP(BWD_MASK); break;
  }
#undef BAP
}
template <typename... A>
void bn_bwd_apply_launch(const BnPlan& p, long M, int C, hipStream_t st, A... a) {
  const dim3 g = bn_grid(p, M, C, p.bwd_rows);
  if (p.lanes == 16) bn_bwd_apply_launch_t<16>(p, g, st, a...);
  else bn_bwd_apply_launch_t<8>(p, g, st, a...);
}
template <bool RAFF, typename... A>
void bn_apply_launch_t(const BnPlan& p, dim3 g, hipStream_t st, A... a) {
  if (p.lanes == 8) hipLaunchKernelGGL((k_bn_apply<8, BN_ROWS, false, RAFF>), g, dim3(256), 0, st, a...);
  else if (p.apply_nt) hipLaunchKernelGGL((k_bn_apply<16, 128, true, RAFF>), g, dim3(256), 0, st, a...);
  else hipLaunchKernelGGL((k_bn_apply<16, BN_ROWS, false, RAFF>), g, dim3(256), 0, st, a...);
}
// (the residual's on-the-fly BN -- the last argument, BnRes, the plan's raff -- selects its own instantiation)
template <typename... A>
void bn_apply_launch(const BnPlan& p, long M, int C, hipStream_t st, A... a) {
  const dim3 g = bn_grid(p, M, C, p.apply_rows);
  if (p.raff) bn_apply_launch_t<true>(p, g, st, a...);
  else bn_apply_launch_t<false>(p, g, st, a...);
}
// BN partial-row reduction (MODE 0 forward statistics, MODE 1 backward sums): with ticket words (ceil(C / 64), zero)
// the coalesced ticketed kernel (k_bn_fin_ticket; the partial rows are overwritten), else the per-channel one
template <int MODE>
void bn_fin_launch(float* part, int nparts, long M, int C, float* a0, float* a1, float* out, float eps, float momentum,
                   int accumulate, unsigned* ticket, hipStream_t st) {
  if (ticket) {
    const int rpb = bn_fin_rpb(nparts);
    const dim3 grid((unsigned)((C + 63) / 64), (unsigned)((nparts + rpb - 1) / rpb));
    hipLaunchKernelGGL((k_bn_fin_ticket<MODE>), grid, dim3(256), 0, st, (float2*)part, nparts, rpb, (int)M, C, a0, a1,
                       (float2*)out, eps, momentum, accumulate, ticket);
    return;
  }
  if constexpr (MODE == 0) {
#define FIN(CW) hipLaunchKernelGGL((k_bn_finalize<CW, BN_FIN_NTH(CW)>), dim3((C + CW - 1) / CW), dim3(BN_FIN_NTH(CW)), 0, \
                                   st, (const float2*)part, nparts, (int)M, C, a0, a1, (float2*)out, eps, momentum)
    BN_FIN_DISPATCH(C, FIN);
#undef FIN
  } else {
#define FIN(CW) hipLaunchKernelGGL((k_bn_bwd_finalize<CW, BN_FIN_NTH(CW)>), dim3((C + CW - 1) / CW), dim3(BN_FIN_NTH(CW)), \
                                   0, st, (const float2*)part, nparts, C, a0, a1, (float2*)out, accumulate)
    BN_FIN_DISPATCH(C, FIN);
#undef FIN
  }
}
}  // namespace

using namespace dca::ops;
#include "ops_gemm_route.hip"
#include "ops_roi.hip"
#include "ops_gconv.hip"
#include "ops_dwconv.hip"
#include "ops_dwconv7.hip"
#include "ops_se.hip"
#include "ops_attn.hip"
#include "ops_ln.hip"

namespace {
thread_local GemmRoute g_route = {};      // of this thread's last dca_ops_gemm (dca_ops_gemm_last_route)
std::atomic<bool> g_lds_raised{false};    // the table's dynamic-LDS limits are set (dca_ops_gemm, once)
}  // namespace

extern "C" {

const char* dca_ops_last_error() { return g_err.c_str(); }
int dca_ops_abi_version() { return 23; }

// The BN rule alone, callable with no device: the kernels dca_ops_bn_fwd / _fwd_parts / _eval / _bwd launch for M rows
// of C channels in this fused form (has_mask: a ReLU bit mask is stored / read; raff: on-the-fly residual BN); -1
// with the error set for a shape it rejects.  Must match ops/_native.py::BnPlan.
int dca_ops_bn_plan(long M, int C, int relu, int res_mode, int has_mask, int raff, BnPlan* out) {
  const char* e = bn_plan(M, C, relu, res_mode, has_mask, raff, out);
  REQUIRE(!e, e);
  return 0;
}

// The rule alone, callable with no device: the route dca_ops_gemm would take on a device of ncu compute units under
// DCA_OPS_STREAM = stream_mode; -1 with the error set for a shape it rejects.  Must match ops/_native.py::GemmRoute.
int dca_ops_gemm_route(const GemmArgs* a, int ncu, int stream_mode, GemmRoute* out) {
  const char* e = gemm_route(*a, ncu, stream_mode, out);
  REQUIRE(!e, e);
  return 0;
}
// The route of this thread's last successful dca_ops_gemm
int dca_ops_gemm_last_route(GemmRoute* out) {
  REQUIRE(g_route.name, "gemm: no GEMM launched on this thread yet");
  *out = g_route;
  return 0;
}

// Must match ops/_native.py::GemmArgs.
int dca_ops_gemm(const GemmArgs* a, void* stream) {
  GemmArgs g = *a;
  hipStream_t st = (hipStream_t)stream;
  int ncu = 0;
  if (cu_count(&ncu)) return -1;
  GemmRoute r;
  const char* e = gemm_route(g, ncu, getenv_stream(), &r);
  REQUIRE(!e, e);
  if (!g_lds_raised.load(std::memory_order_acquire)) {  // once: the kernels that need more than 64 KiB of LDS
#define X(ID, LIM, ...) \
  if (LIM) OPCK(hipFuncSetAttribute((const void*)__VA_ARGS__, hipFuncAttributeMaxDynamicSharedMemorySize, LIM));
    GEMM_KERNELS(X)
#undef X
    g_lds_raised.store(true, std::memory_order_release);
  }
  g.splits = r.splits;
  g.k_per_split = r.k_per_split;
  g.single = r.single;
  g.stages = r.stages;
  if (r.masked_copy) {
    hipLaunchKernelGGL(k_masked_copy, dim3(grid_for((long)g.M * (g.N / 8), 256, 4096)), dim3(256), 0, st,
                       (const unsigned short*)g.beta_src, g.beta_mask, (unsigned short*)g.C, g.M, g.N, g.ldc);
    g.beta_mask = nullptr;
    g.beta_src = nullptr;
  }
  const dim3 grid(r.grid_x, r.grid_y), blk(r.block);
  switch (r.kernel) {
#define X(ID, LIM, ...) \
  case ID: hipLaunchKernelGGL((__VA_ARGS__), grid, blk, r.lds, st, g); break;
    GEMM_KERNELS(X)
#undef X
  }
  if (r.reduce)
    hipLaunchKernelGGL(k_gemm_splitk_reduce, dim3(grid_for((long)g.M * g.N, RED_EL, 4096)), dim3(256), 0, st, g);
  OPCK(hipGetLastError());
  g_route = r;
  return 0;
}

int dca_ops_im2col(const void* x, void* cols, const ConvGeom* geom, void* stream) {
  const ConvGeom g = *geom;
  REQUIRE(g.Kp % 8 == 0 && g.Kp >= g.K && g.K == g.KH * g.KW * g.C, "im2col: bad column geometry");
  const long work = (long)g.N * g.Ho * g.Wo * (g.Kp / 8);
  hipLaunchKernelGGL(k_im2col, dim3(grid_for(work)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                     (bf16_t*)cols, g);
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_col2im(const void* dcols, void* dx, const ConvGeom* geom, int accumulate, void* stream) {
  const ConvGeom g = *geom;
  REQUIRE(g.Kp % 8 == 0 && g.Kp >= g.K, "col2im: bad column geometry");
  hipLaunchKernelGGL(k_col2im, dim3(grid_for((long)g.N * g.H * g.W * g.C / ((g.C & 7) == 0 ? 8 : 1))), dim3(256), 0,
                     (hipStream_t)stream,
                     (const bf16_t*)dcols, (bf16_t*)dx, g, accumulate);
  OPCK(hipGetLastError());
  return 0;
}

// BatchNorm train forward fused with ReLU / residual.  part: [ceil(M/256)][C] float2 scratch; stats: [C] float2
// (mean, invstd) kept for the backward.  momentum 0: running stats untouched (but still the shift).
int dca_ops_bn_fwd(const void* x, const void* r, void* out, float* part, float* stats, const float* gamma,
                   const float* beta, float* rm, float* rv, long M, int C, float eps, float momentum, int relu,
                   int res_mode, unsigned* ticket, void* stream) {
  BnPlan p;
  const char* e = bn_plan(M, C, relu, res_mode, 0, 0, &p);
  REQUIRE(!e, e);
  REQUIRE(res_mode == 0 || r != nullptr, "bn: residual missing");
  hipStream_t st = (hipStream_t)stream;
  const int nparts = (int)((M + BN_ROWS - 1) / BN_ROWS);
  hipLaunchKernelGGL(k_bn_stats, dim3((C + 63) / 64, nparts), dim3(256), 0, st, (const bf16_t*)x, rm, (float2*)part,
                     (int)M, C);
  bn_fin_launch<0>(part, nparts, M, C, rm, rv, stats, eps, momentum, 0, ticket, st);
  bn_apply_launch(p, M, C, st, (const bf16_t*)x, (const bf16_t*)r,
                     (bf16_t*)out, (const float2*)stats, gamma, beta, M, C, relu, res_mode, (uint8_t*)nullptr,
                     (const float*)nullptr, (unsigned*)nullptr, (uint8_t*)nullptr, BnRes{});
  OPCK(hipGetLastError());
  return 0;
}

// BatchNorm forward when the per-tile column partials were produced by the GEMM epilogue (col_stats): finalize
// over `nparts` partial rows + apply.
// q / amax_prev / amax_out (optional): also write an fp8 copy of the output with delayed scaling (k_bn_apply);
// amax_out is zeroed here first.
// mask (optional, res_mode 2 + ReLU): [M C / 8] bytes, the ReLU mask for dca_ops_bn_bwd.
// out == nullptr: statistics only (a BN whose consumer applies it on the fly, BnRes).  rstats / rgamma / rbeta
// (optional, res_mode 2): r is the raw input of another training BN with these statistics, applied on the fly.
int dca_ops_bn_fwd_parts(const void* x, const void* r, void* out, float* part, int nparts, float* stats,
                         const float* gamma, const float* beta, float* rm, float* rv, long M, int C, float eps,
                         float momentum, int relu, int res_mode, void* q, const float* amax_prev, unsigned* amax_out,
                         void* mask, const float* rstats, const float* rgamma, const float* rbeta, unsigned* ticket,
                         void* stream) {
  REQUIRE(!rstats || (res_mode == 2 && rgamma && rbeta), "bn: an on-the-fly residual BN needs res_mode 2");
  BnPlan p;
  const char* e = bn_plan(M, C, relu, res_mode, mask != nullptr, rstats != nullptr, &p);
  REQUIRE(!e, e);
  REQUIRE(res_mode == 0 || r != nullptr, "bn: residual missing");
  REQUIRE(!q || (amax_prev && amax_out), "bn: fp8 output needs amax_prev and amax_out");
  REQUIRE(!mask || (relu && res_mode == 2), "bn: the stored mask is for ReLU(bn + r)");
  hipStream_t st = (hipStream_t)stream;
  REQUIRE(out || (!q && !mask), "bn: statistics only: no fp8 copy / mask");
  if (q) OPCK(hipMemsetAsync(amax_out, 0, sizeof(unsigned), st));
  bn_fin_launch<0>(part, nparts, M, C, rm, rv, stats, eps, momentum, 0, ticket, st);
  if (out)
    bn_apply_launch(p, M, C, st, (const bf16_t*)x, (const bf16_t*)r,
                    (bf16_t*)out, (const float2*)stats, gamma, beta, M, C, relu, res_mode, (uint8_t*)q, amax_prev,
                    amax_out, (uint8_t*)mask, BnRes{(const float2*)rstats, rgamma, rbeta});
  OPCK(hipGetLastError());
  return 0;
}

// BatchNorm in eval mode (inference) fused with ReLU / residual: normalises with the running statistics.
// stats: [C] float2 scratch (mean, invstd).  No running-stat update.
int dca_ops_bn_eval(const void* x, const void* r, void* out, float* stats, const float* gamma, const float* beta,
                    const float* rm, const float* rv, long M, int C, float eps, int relu, int res_mode, void* stream) {
  BnPlan p;
  const char* e = bn_plan(M, C, relu, res_mode, 0, 0, &p);
  REQUIRE(!e, e);
  REQUIRE(res_mode == 0 || r != nullptr, "bn: residual missing");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_bn_eval_stats, dim3((C + 255) / 256), dim3(256), 0, st, rm, rv, (float2*)stats, C, eps);
  bn_apply_launch(p, M, C, st, (const bf16_t*)x, (const bf16_t*)r,
                     (bf16_t*)out, (const float2*)stats, gamma, beta, M, C, relu, res_mode, (uint8_t*)nullptr,
                     (const float*)nullptr, (unsigned*)nullptr, (uint8_t*)nullptr, BnRes{});
  OPCK(hipGetLastError());
  return 0;
}

// mask (optional): the forward's ReLU bit mask (dca_ops_bn_fwd_parts); r is then not read.
int dca_ops_bn_bwd(const void* dy, const void* x, const void* r, const float* stats, const float* gamma,
                   const float* beta, float* part, float* sums, float* dgamma, float* dbeta, void* dx, void* dr,
                   long M, int C, int relu, int res_mode, int accumulate, const void* mask, unsigned* ticket,
                   void* stream) {
  BnPlan p;
  const char* e = bn_plan(M, C, relu, res_mode, mask != nullptr, 0, &p);
  REQUIRE(!e, e);
  // dr (= dz) may be omitted with the mask: the residual's consumer then reads dy and the mask itself
  REQUIRE(res_mode != 2 || mask != nullptr || (r != nullptr && dr != nullptr), "bn bwd: residual tensors missing");
  // mask: ReLU(bn + r)'s own stored mask (relu, res_mode 2), or -- a plain BN whose output is that r (ResNet
  // downsample branch: no relu, res_mode 0) -- the consumer's mask applied to the consumer's dout, passed as dy
  REQUIRE(!mask || (relu && res_mode == 2) || (!relu && res_mode == 0), "bn bwd: unsupported mask use");
  REQUIRE(res_mode != 2 || relu, "bn bwd: a residual join without ReLU is not supported");
  REQUIRE(p.bwd_mode >= 0, "bn bwd: unsupported form");
  hipStream_t st = (hipStream_t)stream;
  const int nparts = (int)((M + BN_ROWS - 1) / BN_ROWS);
  bn_stats_launch(p, M, C, st, (const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)r, (const float2*)stats, gamma,
                  beta, (float2*)part, (int)M, C, (const uint8_t*)mask);
  bn_fin_launch<1>(part, nparts, M, C, dgamma, dbeta, sums, 0.f, 0.f, accumulate, ticket, st);
  bn_bwd_apply_launch(p, M, C, st, (const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)r, (const float2*)stats,
                      gamma, beta, (const float2*)sums, (bf16_t*)dx, (bf16_t*)dr, M, C, (const uint8_t*)mask);
  OPCK(hipGetLastError());
  return 0;
}

// 32-bit pool indexing when every element offset of the input and output (plus one grid stride of slack for the
// loop counter) stays below 2^31
inline bool pool_idx32(const PoolGeom& g) {
  const long in = (long)g.N * g.H * g.W * g.C, out = (long)g.N * g.Ho * g.Wo * g.C;
  return std::max(in, out) + 8192L * 256 < (1L << 31);
}
// 3x3/2 max-pool specialisations: unrolled forward, output-driven backward (324 -> 107 us backward at batch 256)
inline bool pool_k3s2(const PoolGeom& g) {
  return g.K == 3 && g.S == 2 && g.P == 1 && g.H == 2 * g.Ho && g.W == 2 * g.Wo && g.C % 8 == 0;
}

int dca_ops_maxpool_fwd(const void* x, void* y, void* arg, const PoolGeom* geom, void* stream) {
  const PoolGeom g = *geom;
  REQUIRE(g.K * g.K <= 255 && g.K > 0 && g.S > 0, "maxpool: bad window");
  if (pool_k3s2(g)) {
    const dim3 grid(grid_for((long)g.N * g.Ho * g.Wo * g.C / 8));
    if (pool_idx32(g))
      hipLaunchKernelGGL(k_maxpool_fwd_k3s2<unsigned>, grid, dim3(256), 0, (hipStream_t)stream,
                         (const bf16_t*)x, (bf16_t*)y, (uint8_t*)arg, g);
    else
      hipLaunchKernelGGL(k_maxpool_fwd_k3s2<long>, grid, dim3(256), 0, (hipStream_t)stream,
                         (const bf16_t*)x, (bf16_t*)y, (uint8_t*)arg, g);
    OPCK(hipGetLastError());
    return 0;
  }
  const dim3 grid(grid_for((long)g.N * g.Ho * g.Wo * g.C / ((g.C & 7) == 0 ? 8 : 1)));
  if (pool_idx32(g))
    hipLaunchKernelGGL(k_maxpool_fwd<unsigned>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (bf16_t*)y, (uint8_t*)arg, g);
  else
    hipLaunchKernelGGL(k_maxpool_fwd<long>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (bf16_t*)y, (uint8_t*)arg, g);
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_maxpool_bwd(const void* dy, const void* arg, void* dx, const PoolGeom* geom, void* stream) {
  const PoolGeom g = *geom;
  if (pool_k3s2(g)) {
    const dim3 grid(grid_for((long)g.N * g.Ho * g.Wo * g.C / 8));
    if (pool_idx32(g))
      hipLaunchKernelGGL(k_maxpool_bwd_k3s2<unsigned>, grid, dim3(256), 0, (hipStream_t)stream,
                         (const bf16_t*)dy, (const uint8_t*)arg, (bf16_t*)dx, g);
    else
      hipLaunchKernelGGL(k_maxpool_bwd_k3s2<long>, grid, dim3(256), 0, (hipStream_t)stream,
                         (const bf16_t*)dy, (const uint8_t*)arg, (bf16_t*)dx, g);
    OPCK(hipGetLastError());
    return 0;
  }
  const dim3 grid(grid_for((long)g.N * g.H * g.W * g.C / ((g.C & 7) == 0 ? 8 : 1)));
  if (pool_idx32(g))
    hipLaunchKernelGGL(k_maxpool_bwd<unsigned>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)dy, (const uint8_t*)arg, (bf16_t*)dx, g);
  else
    hipLaunchKernelGGL(k_maxpool_bwd<long>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)dy, (const uint8_t*)arg, (bf16_t*)dx, g);
  OPCK(hipGetLastError());
  return 0;
}

// The ResNet stem's BatchNorm + ReLU + 3x3/2/1 max pool as one pass over the conv output y [N][H][W][C] (H = 2 Ho,
// W = 2 Wo, C % 64 == 0), the BN column partials coming from the conv GEMM's epilogue (col_stats): finalize + fused
// apply-and-pool into out / arg [N][Ho][Wo][C] (k_bn_pool_fwd).  Same values as dca_ops_bn_fwd_parts followed by
// dca_ops_maxpool_fwd, without the activation in between.
inline bool bn_pool_ok(const PoolGeom& g) {
  return g.K == 3 && g.S == 2 && g.P == 1 && g.H == 2 * g.Ho && g.W == 2 * g.Wo && g.C % 64 == 0 && pool_idx32(g);
}
int dca_ops_bn_pool_fwd_parts(const void* y, float* part, int nparts, float* stats, const float* gamma,
                              const float* beta, float* rm, float* rv, float eps, float momentum, void* out, void* arg,
                              const PoolGeom* geom, unsigned* ticket, void* stream) {
  const PoolGeom g = *geom;
  REQUIRE(bn_pool_ok(g), "bn_pool: 3x3/2/1 pool with H = 2 Ho, W = 2 Wo, C % 64 == 0, 32-bit offsets");
  hipStream_t st = (hipStream_t)stream;
  const long M = (long)g.N * g.H * g.W;
  bn_fin_launch<0>(part, nparts, M, g.C, rm, rv, stats, eps, momentum, 0, ticket, st);
  hipLaunchKernelGGL(k_bn_pool_fwd<unsigned>, dim3(grid_for((long)g.N * g.Ho * g.Wo * g.C / 8)), dim3(256), 0, st,
                     (const bf16_t*)y, (bf16_t*)out, (uint8_t*)arg, g, (const float2*)stats, gamma, beta);
  OPCK(hipGetLastError());
  return 0;
}
// Its backward from the pooled gradient dp and the argmax bytes: dx = d(conv output); dgamma / dbeta written, or
// accumulated (flat gradient sinks).  part: [part_rows >= ceil(N Ho Wo / BNP_OPB)][C] float2 scratch (the row
// count the caller allocated), sums: [C] float2.
int dca_ops_bn_pool_bwd(const void* dp, const void* arg, const void* y, const float* stats, const float* gamma,
                        const float* beta, float* part, int part_rows, float* sums, float* dgamma, float* dbeta,
                        void* dx, int accumulate, const PoolGeom* geom, unsigned* ticket, void* stream) {
  const PoolGeom g = *geom;
  REQUIRE(bn_pool_ok(g), "bn_pool: 3x3/2/1 pool with H = 2 Ho, W = 2 Wo, C % 64 == 0, 32-bit offsets");
  hipStream_t st = (hipStream_t)stream;
  const long npo = (long)g.N * g.Ho * g.Wo;
  const int nparts = (int)((npo + BNP_OPB - 1) / BNP_OPB);
  REQUIRE(part_rows >= nparts, "bn_pool bwd: part holds fewer than ceil(N Ho Wo / BNP_OPB) rows");
  hipLaunchKernelGGL(k_bn_pool_bwd_stats<unsigned>, dim3(g.C / 64, nparts), dim3(256), 0, st, (const bf16_t*)dp,
                     (const uint8_t*)arg, (const bf16_t*)y, (const float2*)stats, gamma, beta, (float2*)part, g);
  bn_fin_launch<1>(part, nparts, (long)g.N * g.H * g.W, g.C, dgamma, dbeta, sums, 0.f, 0.f, accumulate, ticket, st);
  hipLaunchKernelGGL(k_bn_pool_bwd_apply<unsigned>, dim3(grid_for(npo * g.C / 8)), dim3(256), 0, st,
                     (const bf16_t*)dp, (const uint8_t*)arg, (const bf16_t*)y, (const float2*)stats, gamma, beta,
                     (const float2*)sums, (bf16_t*)dx, g);
  OPCK(hipGetLastError());
  return 0;
}

// y: fp32 [N][C], or bf16 with out_bf16 (the fc GEMM operand directly)
int dca_ops_avgpool_fwd(const void* x, void* y, int N, int HW, int C, int out_bf16, void* stream) {
  const dim3 grid((C + 255) / 256, N);
  if (out_bf16)
    hipLaunchKernelGGL(k_avgpool_fwd<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)y,
                       N, HW, C);
  else
    hipLaunchKernelGGL(k_avgpool_fwd<float>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (float*)y, N,
                       HW, C);
  OPCK(hipGetLastError());
  return 0;
}

// dy: fp32 [N][C], or bf16 with dy_bf16
int dca_ops_avgpool_bwd(const void* dy, void* dx, int N, int HW, int C, int dy_bf16, void* stream) {
  const bool v8 = C % 8 == 0 && (long)N * HW * C + 8192L * 256 * 8 < (1L << 31);
  REQUIRE(v8 || !dy_bf16, "avgpool_bwd: a bf16 dy needs C % 8 == 0");
  if (v8 && dy_bf16)
    hipLaunchKernelGGL(k_avgpool_bwd8<bf16_t>, dim3(grid_for((long)N * HW * C / 8)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)dy, (bf16_t*)dx, N, HW, C);
  else if (v8)
    hipLaunchKernelGGL(k_avgpool_bwd8<float>, dim3(grid_for((long)N * HW * C / 8)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)dy, (bf16_t*)dx, N, HW, C);
  else
    hipLaunchKernelGGL(k_avgpool_bwd, dim3(grid_for((long)N * HW * C)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)dy, (bf16_t*)dx, N, HW, C);
  OPCK(hipGetLastError());
  return 0;
}

// loss_mean / ticket (optional, both or neither): the batch-mean loss written in the same launch
int dca_ops_cross_entropy(const float* logits, const long* labels, float* loss, float* dlogits, int B, int K,
                          float grad_scale, float* loss_mean, unsigned* ticket, void* stream) {
  REQUIRE(B > 0 && K > 0, "cross_entropy: empty input");
  REQUIRE((loss_mean == nullptr) == (ticket == nullptr), "cross_entropy: loss_mean needs a ticket word");
  hipLaunchKernelGGL(k_cross_entropy, dim3(B), dim3(64), 0, (hipStream_t)stream, logits, labels, loss, dlogits, B, K,
                     grad_scale, loss_mean, ticket);
  OPCK(hipGetLastError());
  return 0;
}

// zero `bytes` bytes on the stream (a gradient buffer before the backward): the runtime's fill, no ATen kernel
int dca_ops_zero(void* p, long bytes, void* stream) {
  OPCK(hipMemsetAsync(p, 0, (size_t)bytes, (hipStream_t)stream));
  return 0;
}

int dca_ops_scale_dev(const float* x, const float* s, float* out, long n, void* stream) {
  hipLaunchKernelGGL(k_scale_dev, dim3(grid_for(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x, s, out, n);
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_cast_bf16(const float* x, void* y, long n, void* stream) {
  hipLaunchKernelGGL(k_cast_bf16, dim3(grid_for(n, 256, 2048)), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, n);
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_gather_cols(const float* src, int S, const long* idx, int L, float* out, int rows, int accumulate,
                        void* stream) {
  REQUIRE(rows > 0 && L > 0 && (long)rows * L < (1L << 31), "gather_cols: bad shape");
  hipLaunchKernelGGL(k_gather_cols, dim3(grid_for((long)rows * L, 256, 1024)), dim3(256), 0, (hipStream_t)stream, src, S,
                     idx, L, out, rows, accumulate);
  OPCK(hipGetLastError());
  return 0;
}

// ptrs: device array of n int64 pointers
int dca_ops_add_i64(void* ptrs, int n, void* stream) {
  REQUIRE(n > 0, "add_i64: empty");
  hipLaunchKernelGGL(k_add_i64, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long* const*)ptrs, n);
  OPCK(hipGetLastError());
  return 0;
}

// dy [R][N] (dy_bf16: bf16, else fp32), y: optional ReLU mask source [R][N] (y_bf16: bf16, else fp32); dyb: optional
// bf16 copy of the masked dy; db [N] fp32 column sums; part: nchunk * N floats; ticket: ceil(N / 64) zeroed device
// words.
int dca_ops_dy_prep(const void* dy, int dy_bf16, const void* y, int y_bf16, void* dyb, float* part, float* db,
                    unsigned* ticket, long R, int N, int nchunk, int accumulate, void* stream) {
  REQUIRE(R > 0 && N > 0 && nchunk > 0 && nchunk <= 65535 && R < (1L << 31), "dy_prep: bad shape");
  const int rpb = (int)((R + nchunk - 1) / nchunk);
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((N + 63) / 64, nchunk), b(256);
#define DYP(TD, TY) \
  hipLaunchKernelGGL((k_dy_prep<TD, TY>), g, b, 0, st, (const TD*)dy, (const TY*)y, (bf16_t*)dyb, part, db, ticket, \
                     (int)R, N, rpb, accumulate)
  if (dy_bf16 && y_bf16) DYP(bf16_t, bf16_t);
  else if (dy_bf16) DYP(bf16_t, float);
  else if (y_bf16) DYP(float, bf16_t);
  else DYP(float, float);
#undef DYP
  OPCK(hipGetLastError());
  return 0;
}

// first: device int (1 on the first momentum step); cleared after the update.  gscale: device float the gradient is
// multiplied by first (dca_ops_clip_coef's coefficient), or null.
int dca_ops_sgd(float* p, const float* g, float* buf, long n, float lr, float mu, float wd, int* first,
                const float* gscale, void* stream) {
  REQUIRE(mu == 0.f || buf != nullptr, "sgd: momentum buffer missing");
  hipStream_t st = (hipStream_t)stream;
  auto* k = gscale ? k_sgd<true> : k_sgd<false>;
  hipLaunchKernelGGL(k, dim3(grid_for(n, 256, 2048)), dim3(256), 0, st, p, g, buf, n, lr, mu, wd, first, gscale);
  if (first) hipLaunchKernelGGL(k_clear_flag, dim3(1), dim3(1), 0, st, first);
  OPCK(hipGetLastError());
  return 0;
}

// Adam (decoupled 0) / AdamW (1) over the flat fp32 slices p / g / m / v of n elements.  state: three device doubles
// {steps taken, beta1^steps, beta2^steps} ({0, 1, 1} at the start); this update is step `steps taken + 1`.  advance
// != 0: the state moves on one step after the update (the last -- or only -- update of an optimiser step).  n == 0
// with advance: the state alone.  gscale: device float the gradient is multiplied by first (dca_ops_clip_coef's
// coefficient), or null.
int dca_ops_adam(float* p, const float* g, float* m, float* v, long n, float lr, double beta1, double beta2, double eps,
                 float wd, int decoupled, double* state, int advance, const float* gscale, void* stream) {
  REQUIRE(state != nullptr, "adam: step state missing");
  REQUIRE(n >= 0 && (n == 0 || (p && g && m && v)), "adam: buffer missing");
  REQUIRE(beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1., "adam: the betas must lie in [0, 1)");
  REQUIRE(eps > 0. && (float)eps > 0.f && eps < 3e38, "adam: eps must be positive");
  REQUIRE(wd >= 0.f, "adam: weight decay must not be negative");
  hipStream_t st = (hipStream_t)stream;
  if (n > 0) {
    auto* k = decoupled ? k_adam<true, false> : k_adam<false, false>;
    if (gscale) k = decoupled ? k_adam<true, true> : k_adam<false, true>;
    // one float4 per thread up to 512 workgroups (two per CU), grid-stride beyond
    hipLaunchKernelGGL(k, dim3(grid_for((n + 3) / 4, 256, 512)), dim3(256), 0, st, p, g, m, v, n, lr, beta1, beta2,
                       (float)eps, wd, (const double*)state, gscale);
  }
  if (advance) hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(1), 0, st, state, beta1, beta2);
  OPCK(hipGetLastError());
  return 0;
}

// Global gradient-norm clipping of the flat fp32 slice g of n elements (k_sqnorm_part + k_clip_coef): state, 8-byte
// aligned device memory of dca_ops_clip_state_words() doubles, holds {norm (double), coef (float) | clipped count
// (uint32)} in its first two words and the partial sums behind them.  The coefficient, for the gscale of dca_ops_sgd /
// dca_ops_adam, is the float at byte 8.  No host synchronisation.
int dca_ops_clip_state_words(void) { return 2 + SQN_PARTS; }
int dca_ops_clip_coef(const float* g, long n, float max_norm, double* state, void* stream) {
  static_assert(sizeof(ClipState) == 16 && offsetof(ClipState, coef) == 8, "ClipState is the state's first two words");
  REQUIRE(state != nullptr && ((uintptr_t)state % 8) == 0, "clip_coef: state missing or misaligned");
  REQUIRE(n >= 0 && (n == 0 || g) && ((uintptr_t)g % 4) == 0, "clip_coef: bad gradient slice");
  REQUIRE(max_norm > 0.f, "clip_coef: max_norm must be positive");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_sqnorm_part, dim3(SQN_PARTS), dim3(256), 0, st, g, n, state + 2);
  hipLaunchKernelGGL(k_clip_coef, dim3(1), dim3(64), 0, st, (const double*)(state + 2), SQN_PARTS, max_norm,
                     (ClipState*)state);
  OPCK(hipGetLastError());
  return 0;
}

// Gradient accumulation over the flat fp32 slices acc / g of n elements (k_grad_accum): acc = first ? g : acc + g;
// scaled != 0: acc = g = that sum * scale.  acc and g must not overlap.
int dca_ops_grad_accum(float* acc, float* g, long n, int first, int scaled, float scale, void* stream) {
  REQUIRE(n >= 0 && (n == 0 || (acc && g)), "grad_accum: buffer missing");
  REQUIRE(((uintptr_t)acc % 4) == 0 && ((uintptr_t)g % 4) == 0, "grad_accum: misaligned slice");
  REQUIRE(n == 0 || acc + n <= g || g + n <= acc, "grad_accum: acc and g overlap");
  if (n == 0) return 0;
  // one float4 per thread up to 512 workgroups (two per CU), grid-stride beyond
  hipLaunchKernelGGL(k_grad_accum, dim3(grid_for((n + 3) / 4, 256, 512)), dim3(256), 0, (hipStream_t)stream, acc, g, n,
                     first, scaled, scale);
  OPCK(hipGetLastError());
  return 0;
}

// x (fp32 if is_f32 else bf16, n elements) -> q fp8 e4m3; amax_bits: device uint, zeroed here first.
int dca_ops_quant_fp8(const void* x, int is_f32, long n, void* q, unsigned* amax_bits, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  OPCK(hipMemsetAsync(amax_bits, 0, sizeof(unsigned), st));
  const int grid = grid_for(n, 256, 1024);
  if (is_f32) {
    hipLaunchKernelGGL(k_amax<float>, dim3(grid), dim3(256), 0, st, (const float*)x, n, amax_bits);
    hipLaunchKernelGGL(k_quant_fp8<float>, dim3(grid_for(n / 4 + 1)), dim3(256), 0, st, (const float*)x,
                       (uint8_t*)q, n, amax_bits);
  } else {
    hipLaunchKernelGGL(k_amax<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, n, amax_bits);
    hipLaunchKernelGGL(k_quant_fp8<bf16_t>, dim3(grid_for(n / 4 + 1)), dim3(256), 0, st, (const bf16_t*)x,
                       (uint8_t*)q, n, amax_bits);
  }
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_fp8_alpha(const unsigned* amax_a, const unsigned* amax_b, float extra, float* alpha, void* stream) {
  hipLaunchKernelGGL(k_fp8_alpha, dim3(1), dim3(1), 0, (hipStream_t)stream, amax_a, amax_b, extra, alpha);
  OPCK(hipGetLastError());
  return 0;
}

// descs: device array of nd PackDesc (ops/functional.py WeightPack); amax: n_amax device words zeroed first.
int dca_ops_pack_weights(const void* descs, int nd, int blocks_per_layer, unsigned* amax, int n_amax, void* stream) {
  REQUIRE(nd > 0 && blocks_per_layer > 0, "pack_weights: empty");
  REQUIRE(blocks_per_layer <= 4096, "pack_weights: at most 4096 blocks per layer (32-bit grid-stride indices)");
  hipStream_t st = (hipStream_t)stream;
  if (n_amax > 0) OPCK(hipMemsetAsync(amax, 0, sizeof(unsigned) * n_amax, st));
  const dim3 grid(blocks_per_layer, nd);
  hipLaunchKernelGGL(k_pack_weights, grid, dim3(256), 0, st, (const PackDesc*)descs);
  if (n_amax > 0) hipLaunchKernelGGL(k_pack_fp8, grid, dim3(256), 0, st, (const PackDesc*)descs);
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_pack_desc_size() { return (int)sizeof(PackDesc); }

int dca_ops_nchw_to_nhwc8(const float* x, void* y, int N, int C, long HW, void* stream) {
  REQUIRE(C > 0 && C <= 8, "nchw_to_nhwc8: 1..8 channels");
  hipLaunchKernelGGL(k_nchw_to_nhwc8, dim3(grid_for((long)N * HW)), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y,
                     N, C, HW);
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_nchw_to_s2d16(const float* x, void* y, int N, int C, int H, int W, int Hs, int Ws, int P, void* stream) {
  REQUIRE(C > 0 && C <= 4 && P >= 0 && Hs > 0 && Ws > 0, "nchw_to_s2d16: 1..4 channels");
  hipLaunchKernelGGL(k_nchw_to_s2d16, dim3(grid_for((long)N * Hs * Ws)), dim3(256), 0, (hipStream_t)stream, x,
                     (bf16_t*)y, N, C, H, W, Hs, Ws, P);
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_pack_gather(const void* descs, int nd, int blocks, void* stream) {
  REQUIRE(nd > 0 && blocks > 0, "pack_gather: empty");
  hipLaunchKernelGGL(k_pack_gather, dim3(blocks, nd), dim3(256), 0, (hipStream_t)stream, (const GatherDesc*)descs);
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_gather_desc_size() { return (int)sizeof(GatherDesc); }

// ROI-align (ops_roi.hip).  feat / dfeat: dense NHWC bf16 [B][h][w][C]; boxes: N rows of 5 floats (batch index, x1,
// y1, x2, y2 in input pixels); out / dout: dense bf16 [N][k][k][C] (ops/functional.py checks that the tensors are
// contiguous).  Any box values are safe: the kernels clamp every index.  N == 0: the forward does nothing, the backward
// writes zeros.
static const char* roi_rule(int B, int h, int w, int C, int N, int k, float stride) {
  if (B <= 0 || h <= 0 || w <= 0 || C <= 0 || N < 0) return "roi_align: bad shape";
  if (C % 8) return "roi_align: C % 8 != 0";
  if (k < 1 || k > ROI_KMAX) return "roi_align: bins outside 1..8";
  if (h > ROI_HWMAX || w > ROI_HWMAX) return "roi_align: feature map larger than 64 x 64";
  if (!(stride > 0.f)) return "roi_align: stride must be positive";
  if ((long)B * h * w * C >= (1L << 31) || (long)N * k * k * C >= (1L << 31)) return "roi_align: 2^31 elements or more";
  if ((C + 255) / 256 > 65535 || B > 65535) return "roi_align: more than 65535 images or 256-channel slabs (grid.y)";
  return nullptr;
}
static const char* roi_check(const void* feat, const void* boxes, const void* out, int B, int h, int w, int C, int N,
                             int k, float stride) {
  if (const char* e = roi_rule(B, h, w, C, N, k, stride)) return e;
  if (!feat || (N > 0 && (!boxes || !out))) return "roi_align: buffer missing";
  if ((uintptr_t)feat % 16 || (uintptr_t)out % 16 || (uintptr_t)boxes % 4) return "roi_align: misaligned buffer";
  return nullptr;
}

// The shape rule alone, callable with no device (ops/functional.py roi_align_ok): -1 with the error set for a shape the
// two launchers reject
int dca_ops_roi_align_rule(int B, int h, int w, int C, int N, int k, float stride) {
  const char* e = roi_rule(B, h, w, C, N, k, stride);
  REQUIRE(!e, e);
  return 0;
}

int dca_ops_roi_align_fwd(const void* feat, const float* boxes, void* out, int B, int h, int w, int C, int N, int k,
                          float stride, void* stream) {
  const char* e = roi_check(feat, boxes, out, B, h, w, C, N, k, stride);
  REQUIRE(!e, e);
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_roi_align_fwd, dim3(N, (C + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)feat, boxes, (bf16_t*)out, RoiGeom{B, h, w, C, N, k, stride});
  OPCK(hipGetLastError());
  return 0;
}

int dca_ops_roi_align_bwd(const void* dout, const float* boxes, void* dfeat, int B, int h, int w, int C, int N, int k,
                          float stride, void* stream) {
  const char* e = roi_check(dfeat, boxes, dout, B, h, w, C, N, k, stride);
  REQUIRE(!e, e);
  hipLaunchKernelGGL(k_roi_align_bwd, dim3((C + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dout,
                     boxes, (bf16_t*)dfeat, RoiGeom{B, h, w, C, N, k, stride});
  OPCK(hipGetLastError());
  return 0;
}

// Grouped 3 x 3 convolution (ops_gconv.hip).  x / dx: dense NHWC bf16 [N][H][W][C]; y / dy: [N][Ho][Wo][C]; w / dw: fp32
// [C][C / groups][3][3]; the packed operands: (C / 16) * (Cg == 32 ? 9 : 5) * 1024 bytes each.
static const char* gconv_rule(int N, int H, int W, int Cin, int Cout, int groups, int KH, int KW, int stride, int pad) {
  static const char* rule =
      "gconv: the grouped-convolution rule is 3x3, pad 1, stride 1 or 2, Cin == Cout == C, C % 16 == 0, "
      "C / groups in {4, 8, 16, 32}, input rows of at most 64 pixels, fewer than 2^30 input elements (32-bit byte "
      "offsets; the output is never larger)";
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || groups <= 1) return rule;
  if (KH != 3 || KW != 3 || pad != 1 || (stride != 1 && stride != 2)) return rule;
  if (Cin != Cout || Cin % 16 || Cin % groups) return rule;
  const int cg = Cin / groups;
  if (cg != 4 && cg != 8 && cg != 16 && cg != 32) return rule;
  if (W > 64) return rule;
  if ((long)N * H * W * Cin >= (1L << 30)) return rule;  // (N * strips <= 4 N < 2^31 workgroups follows)
  return nullptr;
}
int dca_ops_gconv_rule(int N, int H, int W, int Cin, int Cout, int groups, int KH, int KW, int stride, int pad) {
  const char* e = gconv_rule(N, H, W, Cin, Cout, groups, KH, KW, stride, pad);
  REQUIRE(!e, e);
  return 0;
}
static GconvGeom gconv_geom(int N, int H, int W, int C, int stride, int nparts) {
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  return GconvGeom{N, H, W, C, Ho, Wo, H, W, std::min(4, (Ho + 1) / 2), nparts};
}

int dca_ops_gconv_pack(const float* w, void* fwd, void* dgrad, int C, int groups, void* stream) {
  const char* e = gconv_rule(1, 1, 1, C, C, groups, 3, 3, 1, 1);
  REQUIRE(!e, e);
  REQUIRE(w && fwd && dgrad && (uintptr_t)fwd % 16 == 0 && (uintptr_t)dgrad % 16 == 0, "gconv_pack: bad buffer");
  const int cg = C / groups, n = 2 * (C / 16) * (cg == 32 ? 9 : 5) * 64;
  hipLaunchKernelGGL(k_gconv_pack, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, (bf16_t*)fwd,
                     (bf16_t*)dgrad, C, cg);
  OPCK(hipGetLastError());
  return 0;
}

// Forward.  part (or null): [nparts][C][2] fp32 BN partial sums of (y - shift[c]), every row written; nparts also
// bounds the workgroups per 64-channel slab (>= 1).
int dca_ops_gconv_fwd(const void* x, const void* wpk, void* y, float* part, const float* shift, int nparts, int N,
                      int H, int W, int C, int groups, int stride, void* stream) {
  const char* e = gconv_rule(N, H, W, C, C, groups, 3, 3, stride, 1);
  REQUIRE(!e, e);
  REQUIRE(x && wpk && y && nparts >= 1 && (!part || shift), "gconv_fwd: buffer missing or nparts < 1");
  REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)wpk % 16 == 0 && (uintptr_t)y % 8 == 0, "gconv_fwd: misaligned buffer");
  const GconvGeom g = gconv_geom(N, H, W, C, stride, nparts);
  const dim3 grid(std::min(N * g.strips, nparts), (C + 63) / 64);
  const bool c32 = C / groups == 32;
#define GC_FWD(S, B)                                                                                          \
  hipLaunchKernelGGL((k_gconv3x3_rows<S, B, false>), grid, dim3(GC_NT), 0, (hipStream_t)stream, (const bf16_t*)x, \
                     (const bf16_t*)wpk, (bf16_t*)y, part, shift, g)
  if (stride == 1) { if (c32) GC_FWD(1, true); else GC_FWD(1, false); }
  else { if (c32) GC_FWD(2, true); else GC_FWD(2, false); }
#undef GC_FWD
  OPCK(hipGetLastError());
  return 0;
}

// Input gradient dx [N][H][W][C] from dy [N][Ho][Wo][C] and the packed dgrad operand (H, W: the forward's input).
int dca_ops_gconv_dgrad(const void* dy, const void* wpk, void* dx, int N, int H, int W, int C, int groups, int stride,
                        void* stream) {
  const char* e = gconv_rule(N, H, W, C, C, groups, 3, 3, stride, 1);
  REQUIRE(!e, e);
  REQUIRE(dy && wpk && dx, "gconv_dgrad: buffer missing");
  REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)wpk % 16 == 0 && (uintptr_t)dx % 8 == 0,
          "gconv_dgrad: misaligned buffer");
  GconvGeom g = gconv_geom(N, H, W, C, 1, 1);  // a stride-1 conv over the H x W grid
  g.Hs = (H - 1) / stride + 1;
  g.Ws = (W - 1) / stride + 1;
  const dim3 grid(N * g.strips, (C + 63) / 64);
  const bool c32 = C / groups == 32;
#define GC_DG(B, D)                                                                                           \
  hipLaunchKernelGGL((k_gconv3x3_rows<1, B, D>), grid, dim3(GC_NT), 0, (hipStream_t)stream, (const bf16_t*)dy, \
                     (const bf16_t*)wpk, (bf16_t*)dx, (float*)nullptr, (const float*)nullptr, g)
  if (stride == 1) { if (c32) GC_DG(true, false); else GC_DG(false, false); }
  else { if (c32) GC_DG(true, true); else GC_DG(false, true); }
#undef GC_DG
  OPCK(hipGetLastError());
  return 0;
}

// Weight gradient dw [C][C / groups][3][3] fp32 (beta 1: accumulated into dw).  ws: slabs * C * 144 * (Cg == 32 ? 2 : 1)
// floats; slabs (>= 1) bounds the workgroups per 64-channel slab.
int dca_ops_gconv_wgrad(const void* x, const void* dy, float* ws, int slabs, float* dw, int beta, int N, int H, int W,
                        int C, int groups, int stride, void* stream) {
  const char* e = gconv_rule(N, H, W, C, C, groups, 3, 3, stride, 1);
  REQUIRE(!e, e);
  REQUIRE(x && dy && ws && dw && slabs >= 1 && (beta == 0 || beta == 1), "gconv_wgrad: buffer missing, slabs < 1 or beta");
  REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)dy % 16 == 0, "gconv_wgrad: misaligned buffer");
  const GconvGeom g = gconv_geom(N, H, W, C, stride, slabs);
  const int used = std::min(N * g.strips, slabs), cg = C / groups;
  const dim3 grid(used, (C + 63) / 64);
#define GC_WG(S, B)                                                                                        \
  hipLaunchKernelGGL((k_gconv3x3_wgrad<S, B>), grid, dim3(GC_NT), 0, (hipStream_t)stream, (const bf16_t*)x, \
                     (const bf16_t*)dy, ws, g)
  if (stride == 1) { if (cg == 32) GC_WG(1, true); else GC_WG(1, false); }
  else { if (cg == 32) GC_WG(2, true); else GC_WG(2, false); }
#undef GC_WG
  OPCK(hipGetLastError());
  hipLaunchKernelGGL(k_gconv_wgrad_reduce, dim3((C * cg * 9 + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const float*)ws, dw, C, cg, used, beta);
  OPCK(hipGetLastError());
  return 0;
}

// Depthwise 3 x 3 convolution (ops_dwconv.hip).  x / dx: dense NHWC bf16 [N][H][W][C]; y / dy: [N][Ho][Wo][C]; w / dw:
// the fp32 master weight [C][1][3][3], read directly (rounded to bf16 in the kernels): there is no packed operand.
static const char* dwconv_rule(int N, int H, int W, int Cin, int Cout, int groups, int KH, int KW, int stride, int pad) {
  static const char* rule =
      "dwconv: the depthwise-convolution rule is 3x3, pad 1, stride 1 or 2, Cin == Cout == groups == C, C % 8 == 0, "
      "input rows of 1 to 128 pixels, fewer than 2^30 input elements (32-bit byte offsets; the output is never larger)";
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0) return rule;
  if (KH != 3 || KW != 3 || pad != 1 || (stride != 1 && stride != 2)) return rule;
  if (Cin != Cout || Cin != groups || Cin % 8) return rule;
  if (W > 128) return rule;
  if ((long)N * H * W * Cin >= (1L << 30)) return rule;  // (4 N workgroups x C / 32 slabs < 2^31 follows)
  return nullptr;
}
int dca_ops_dwconv_rule(int N, int H, int W, int Cin, int Cout, int groups, int KH, int KW, int stride, int pad) {
  const char* e = dwconv_rule(N, H, W, Cin, Cout, groups, KH, KW, stride, pad);
  REQUIRE(!e, e);
  return 0;
}
static DwGeom dwconv_geom(int N, int H, int W, int C, int stride, int nparts) {
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  return DwGeom{N, H, W, C, Ho, Wo, std::min(4, (Ho + 1) / 2), nparts};
}
// The work split of a W-pixel input row (ops_dwconv.hip, DwPlan): log2 of the chunks per slab and the columns per
// thread.  The widest slab whose 256 / CH columns still cover the row (stride 2 and its dgrad: half the row), and
// no wider than the channels there are.  wmax: the widest row a 4-chunk slab with one column per thread takes.
static void dwconv_plan(int W, int C, int wmax, int* lc, int* nc) {
  *nc = W > wmax ? 2 : 1;
  *lc = 2;
  if (W <= wmax / 2 && C >= 64) *lc = 3;
  if (W <= wmax / 4 && C >= 128) *lc = 4;
}
#define DW_PLAN_SWITCH(lc, nc, M) \
  do {                            \
    if (lc == 4) M(4, 1);         \
    else if (lc == 3) M(3, 1);    \
    else if (nc == 1) M(2, 1);    \
    else M(2, 2);                 \
  } while (0)
#define DW_LC_SWITCH(lc, M)    \
  do {                         \
    if (lc == 4) M(4, 1);      \
    else if (lc == 3) M(3, 1); \
    else M(2, 1);              \
  } while (0)

static void dwconv_rows_launch(const void* x, const float* w, void* y, float* part, const float* shift, const DwGeom& g,
                               int stride, int flip, hipStream_t stream) {
  int lc, nc;
  dwconv_plan(g.W, g.C, stride == 1 ? 64 : 128, &lc, &nc);
  const int nslab = (g.C + (8 << lc) - 1) / (8 << lc);
  const dim3 grid((unsigned)std::min(g.N * g.strips, g.nparts) * nslab);
#define DW_ROWS(S, LC, NC, ST)                                                                          \
  hipLaunchKernelGGL((k_dwconv3x3_rows<S, LC, NC, ST>), grid, dim3(DW_NT), 0, stream, (const bf16_t*)x, w, \
                     (bf16_t*)y, part, shift, g, flip)
#define DW_S1T(LC, NC) DW_ROWS(1, LC, NC, true)
#define DW_S1F(LC, NC) DW_ROWS(1, LC, NC, false)
#define DW_S2T(LC, NC) DW_ROWS(2, LC, 1, true)
#define DW_S2F(LC, NC) DW_ROWS(2, LC, 1, false)
  if (stride == 1) { if (part) DW_PLAN_SWITCH(lc, nc, DW_S1T); else DW_PLAN_SWITCH(lc, nc, DW_S1F); }
  else { if (part) DW_LC_SWITCH(lc, DW_S2T); else DW_LC_SWITCH(lc, DW_S2F); }
#undef DW_S1T
#undef DW_S1F
#undef DW_S2T
#undef DW_S2F
#undef DW_ROWS
}

// Forward.  part (or null): [nparts][C][2] fp32 BN partial sums of (y - shift[c]), every row written; nparts also
// bounds the workgroups per slab (>= 1).
int dca_ops_dwconv_fwd(const void* x, const float* w, void* y, float* part, const float* shift, int nparts, int N,
                       int H, int W, int C, int groups, int stride, void* stream) {
  const char* e = dwconv_rule(N, H, W, C, C, groups, 3, 3, stride, 1);
  REQUIRE(!e, e);
  REQUIRE(x && w && y && nparts >= 1 && (!part || shift), "dwconv_fwd: buffer missing or nparts < 1");
  REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0 && (uintptr_t)part % 8 == 0, "dwconv_fwd: misaligned buffer");
  dwconv_rows_launch(x, w, y, part, shift, dwconv_geom(N, H, W, C, stride, nparts), stride, 0, (hipStream_t)stream);
  OPCK(hipGetLastError());
  return 0;
}

// Input gradient dx [N][H][W][C] from dy [N][Ho][Wo][C] and the master weight (H, W: the forward's input).
int dca_ops_dwconv_dgrad(const void* dy, const float* w, void* dx, int N, int H, int W, int C, int groups, int stride,
                         void* stream) {
  const char* e = dwconv_rule(N, H, W, C, C, groups, 3, 3, stride, 1);
  REQUIRE(!e, e);
  REQUIRE(dy && w && dx, "dwconv_dgrad: buffer missing");
  REQUIRE((uintptr_t)dy % 16 == 0 && (uintptr_t)dx % 16 == 0, "dwconv_dgrad: misaligned buffer");
  if (stride == 1) {  // the forward kernel over dY, taps flipped
    // workgroups per slab: about 2048 32-channel workgroups in all (each reads its 9 x 8 weights once), as the
    // forward's default nparts in ops/functional.py
    const int strips = std::min(4, (H + 1) / 2), wgs = std::min(N * strips, std::max(1, 2048 * 32 / C));
    dwconv_rows_launch(dy, w, dx, nullptr, nullptr, dwconv_geom(N, H, W, C, 1, wgs), 1, 1, (hipStream_t)stream);
  } else {
    const DwGeom g = dwconv_geom(N, H, W, C, 2, 1);  // units: strips of dY rows
    int lc, nc;
    dwconv_plan(W, C, 128, &lc, &nc);
    const int nslab = (C + (8 << lc) - 1) / (8 << lc);
    const dim3 grid((unsigned)(N * g.strips) * nslab);
#define DW_DG2(LC, NC) \
  hipLaunchKernelGGL((k_dwconv3x3_dgrad2<LC>), grid, dim3(DW_NT), 0, (hipStream_t)stream, (const bf16_t*)dy, w, (bf16_t*)dx, g)
    DW_LC_SWITCH(lc, DW_DG2);
#undef DW_DG2
  }
  OPCK(hipGetLastError());
  return 0;
}

// Weight gradient dw [C][1][3][3] fp32 (beta 1: accumulated into dw).  ws: slabs * C * 9 floats; slabs (>= 1) bounds
// the workgroups per channel slab.
int dca_ops_dwconv_wgrad(const void* x, const void* dy, float* ws, int slabs, float* dw, int beta, int N, int H, int W,
                         int C, int groups, int stride, void* stream) {
  const char* e = dwconv_rule(N, H, W, C, C, groups, 3, 3, stride, 1);
  REQUIRE(!e, e);
  REQUIRE(x && dy && ws && dw && slabs >= 1 && (beta == 0 || beta == 1), "dwconv_wgrad: buffer missing, slabs < 1 or beta");
  REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)dy % 16 == 0, "dwconv_wgrad: misaligned buffer");
  const DwGeom g = dwconv_geom(N, H, W, C, stride, slabs);
  const int used = std::min(N * g.strips, slabs);
  int lc, nc;
  dwconv_plan(W, C, stride == 1 ? 64 : 128, &lc, &nc);
  const int nslab = (C + (8 << lc) - 1) / (8 << lc);
  const dim3 grid((unsigned)used * nslab);
#define DW_WG1(LC, NC) \
  hipLaunchKernelGGL((k_dwconv3x3_wgrad<1, LC, NC>), grid, dim3(DW_NT), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)dy, ws, g)
#define DW_WG2(LC, NC) \
  hipLaunchKernelGGL((k_dwconv3x3_wgrad<2, LC, 1>), grid, dim3(DW_NT), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)dy, ws, g)
  if (stride == 1) DW_PLAN_SWITCH(lc, nc, DW_WG1); else DW_LC_SWITCH(lc, DW_WG2);
#undef DW_WG1
#undef DW_WG2
  OPCK(hipGetLastError());
  hipLaunchKernelGGL(k_dwconv_wgrad_reduce, dim3((C * 9 + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const float*)ws, dw, C, used, beta);
  OPCK(hipGetLastError());
  return 0;
}

// Depthwise 7 x 7 convolution (ops_dwconv7.hip).  x / y / dy / dx: dense NHWC bf16 [N][H][W][C]; w / dw: the fp32 master
// weight [C][1][7][7], read directly (rounded to bf16 in the kernels): there is no packed operand; bias / db: fp32 [C].
static const char* dwconv7_rule(int N, int H, int W, int Cin, int Cout, int groups, int KH, int KW, int stride, int pad) {
  static const char* rule =
      "dwconv7: the depthwise 7x7 convolution rule is 7x7, pad 3, stride 1, Cin == Cout == groups == C, C % 8 == 0, "
      "rows of 1 to 64 pixels, fewer than 2^31 elements (32-bit byte offsets) and 16-byte aligned activations";
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0) return rule;
  if (KH != 7 || KW != 7 || pad != 3 || stride != 1) return rule;
  if (Cin != Cout || Cin != groups || Cin % 8) return rule;
  if (W > 64) return rule;
  if ((long)N * H * W * Cin >= (1L << 31)) return rule;
  return nullptr;
}
int dca_ops_dwconv7_rule(int N, int H, int W, int Cin, int Cout, int groups, int KH, int KW, int stride, int pad) {
  const char* e = dwconv7_rule(N, H, W, Cin, Cout, groups, KH, KW, stride, pad);
  REQUIRE(!e, e);
  return 0;
}
// The work split (ops_dwconv7.hip, D7Plan): log2 of the channel pairs per slab, the widest whose 256 / CP columns
// cover the row and no wider than the channels; and the strips per image: whole images when they give about 768 units
// (three workgroups on each of 256 CUs), else strips of at least 8 rows.
static D7Geom dwconv7_geom(int N, int H, int W, int C, int* lp) {
  *lp = W > 32 ? 2 : W > 16 ? 3 : W > 8 ? 4 : 5;
  while (*lp > 2 && (2 << *lp) > C) --*lp;
  const long units = (long)N * ((C + (2 << *lp) - 1) / (2 << *lp));
  const int strips = (int)std::max(1L, std::min((768 + units - 1) / units, (long)std::max(1, H / 8)));
  return D7Geom{N, H, W, C, strips};
}
#define D7_LP_SWITCH(lp, M) \
  do {                      \
    if (lp == 5) M(5);      \
    else if (lp == 4) M(4); \
    else if (lp == 3) M(3); \
    else M(2);              \
  } while (0)

// Forward y = bf16(conv(x) + bias) (bias or null); flip 1: the input gradient (x = dy, y = dx, bias null).
int dca_ops_dwconv7_fwd(const void* x, const float* w, const float* bias, void* y, int N, int H, int W, int C, int flip,
                        void* stream) {
  const char* e = dwconv7_rule(N, H, W, C, C, C, 7, 7, 1, 3);
  REQUIRE(!e, e);
  REQUIRE(x && w && y && (flip == 0 || (flip == 1 && !bias)), "dwconv7_fwd: buffer missing, or flip with a bias");
  REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0, "dwconv7_fwd: misaligned buffer");
  int lp;
  const D7Geom g = dwconv7_geom(N, H, W, C, &lp);
  // about 1536 workgroups in all: each reads its 98 weights once and then walks two or more units
  const int nslab = (C + (2 << lp) - 1) / (2 << lp), wgs = std::min(N * g.strips, std::max(1, 1536 / nslab));
  const dim3 grid((unsigned)wgs * nslab);
#define D7_FWD(LP)                                                                                              \
  hipLaunchKernelGGL((k_dwconv7x7_fwd<LP>), grid, dim3(DW_NT), 0, (hipStream_t)stream, (const bf16_t*)x, w, bias, \
                     (bf16_t*)y, g, flip)
  D7_LP_SWITCH(lp, D7_FWD);
#undef D7_FWD
  OPCK(hipGetLastError());
  return 0;
}

// Weight gradient dw [C][1][7][7] and bias gradient db [C] (or null), fp32 (beta 1: accumulated into both).  ws:
// slabs * C * 50 floats; slabs (>= 1) bounds the workgroups per channel slab.
int dca_ops_dwconv7_wgrad(const void* x, const void* dy, float* ws, int slabs, float* dw, float* db, int beta, int N,
                          int H, int W, int C, void* stream) {
  const char* e = dwconv7_rule(N, H, W, C, C, C, 7, 7, 1, 3);
  REQUIRE(!e, e);
  REQUIRE(x && dy && ws && dw && slabs >= 1 && (beta == 0 || beta == 1), "dwconv7_wgrad: buffer missing, slabs < 1 or beta");
  REQUIRE((uintptr_t)x % 16 == 0 && (uintptr_t)dy % 16 == 0, "dwconv7_wgrad: misaligned buffer");
  int lp;
  const D7Geom g = dwconv7_geom(N, H, W, C, &lp);
  const int nslab = (C + (2 << lp) - 1) / (2 << lp), used = std::min(N * g.strips, slabs);
  const dim3 grid((unsigned)used * nslab);
#define D7_WG(LP) \
  hipLaunchKernelGGL((k_dwconv7x7_wgrad<LP>), grid, dim3(DW_NT), 0, (hipStream_t)stream, (const bf16_t*)x, (const bf16_t*)dy, ws, g)
  D7_LP_SWITCH(lp, D7_WG);
#undef D7_WG
  OPCK(hipGetLastError());
  hipLaunchKernelGGL(k_dwconv7_wgrad_reduce, dim3((C * D7_WS + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     (const float*)ws, dw, db, C, used, beta);
  OPCK(hipGetLastError());
  return 0;
}

// Squeeze-and-excitation (ops_se.hip).  u / idt / out / dout / didt / du: dense NHWC bf16 [N][H][W][C]; z / dz: fp32
// [N][C] gate logits; s / ds: [N][C], bf16 or fp32 by flag.
static const char* se_rule(int N, int H, int W, int C) {
  static const char* rule =
      "se: the squeeze-and-excitation rule is dense NHWC bf16 with N, H, W, C >= 1, C % 8 == 0 and fewer than 2^31 "
      "elements";
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return rule;
  if ((long)N * H * W * C >= (1L << 31)) return rule;  // (P = H W and N x slabs fit an int)
  return nullptr;
}
int dca_ops_se_rule(int N, int H, int W, int C) {
  const char* e = se_rule(N, H, W, C);
  REQUIRE(!e, e);
  return 0;
}
// log2 of the chunks per slab (ops_se.hip, SePlan): the lanes (256 / CH) do not outnumber the pixels, and a slab is no
// wider than the channels fill twice
static int se_lc(int P, int C) { return P <= 64 && C >= 256 ? 5 : (P <= 256 && C >= 128 ? 4 : 3); }
#define SE_LAUNCH(K, P, C, N, stream, ...)                                                                        \
  do {                                                                                                            \
    const int lc_ = se_lc(P, C);                                                                                  \
    const dim3 grid_((unsigned)(N) * (unsigned)(((C) + (8 << lc_) - 1) / (8 << lc_)));                            \
    if (lc_ == 5) hipLaunchKernelGGL((K<5>), grid_, dim3(SE_NT), 0, (hipStream_t)(stream), __VA_ARGS__);          \
    else if (lc_ == 4) hipLaunchKernelGGL((K<4>), grid_, dim3(SE_NT), 0, (hipStream_t)(stream), __VA_ARGS__);     \
    else hipLaunchKernelGGL((K<3>), grid_, dim3(SE_NT), 0, (hipStream_t)(stream), __VA_ARGS__);                   \
    OPCK(hipGetLastError());                                                                                      \
  } while (0)
#define SE_ALIGNED(p) ((uintptr_t)(p) % 16 == 0)

// s[n][c] = mean over the H W pixels of u (out_bf16: bf16, else fp32)
int dca_ops_se_squeeze(const void* u, void* s, int out_bf16, int N, int H, int W, int C, void* stream) {
  const char* e = se_rule(N, H, W, C);
  REQUIRE(!e, e);
  REQUIRE(u && s, "se_squeeze: buffer missing");
  REQUIRE(SE_ALIGNED(u) && SE_ALIGNED(s), "se_squeeze: misaligned buffer");
  SE_LAUNCH(k_se_squeeze, H * W, C, N, stream, (const bf16_t*)u, s, H * W, C, out_bf16);
  return 0;
}

// out = ReLU(u * sigmoid(z)[n][c] + idt)
int dca_ops_se_scale_fwd(const void* u, const float* z, const void* idt, void* out, int N, int H, int W, int C,
                         void* stream) {
  const char* e = se_rule(N, H, W, C);
  REQUIRE(!e, e);
  REQUIRE(u && z && idt && out, "se_scale_fwd: buffer missing");
  REQUIRE(SE_ALIGNED(u) && SE_ALIGNED(idt) && SE_ALIGNED(out) && SE_ALIGNED(z), "se_scale_fwd: misaligned buffer");
  SE_LAUNCH(k_se_scale_fwd, H * W, C, N, stream, (const bf16_t*)u, z, (const bf16_t*)idt, (bf16_t*)out, H * W, C);
  return 0;
}

// didt = dout * [out > 0]; dz[n][c] = g (1 - g) sum over the pixels of didt * u
int dca_ops_se_bwd_reduce(const void* dout, const void* out, const void* u, const float* z, void* didt, float* dz,
                          int N, int H, int W, int C, void* stream) {
  const char* e = se_rule(N, H, W, C);
  REQUIRE(!e, e);
  REQUIRE(dout && out && u && z && didt && dz, "se_bwd_reduce: buffer missing");
  REQUIRE(SE_ALIGNED(dout) && SE_ALIGNED(out) && SE_ALIGNED(u) && SE_ALIGNED(didt) && SE_ALIGNED(z) && SE_ALIGNED(dz),
          "se_bwd_reduce: misaligned buffer");
  SE_LAUNCH(k_se_bwd_reduce, H * W, C, N, stream, (const bf16_t*)dout, (const bf16_t*)out, (const bf16_t*)u, z,
            (bf16_t*)didt, dz, H * W, C);
  return 0;
}

// du = dout * [out > 0] * g[n][c] + ds[n][c] / (H W) (ds_bf16: ds is bf16, else fp32)
int dca_ops_se_bwd_apply(const void* dout, const void* out, const float* z, const void* ds, int ds_bf16, void* du,
                         int N, int H, int W, int C, void* stream) {
  const char* e = se_rule(N, H, W, C);
  REQUIRE(!e, e);
  REQUIRE(dout && out && z && ds && du, "se_bwd_apply: buffer missing");
  REQUIRE(SE_ALIGNED(dout) && SE_ALIGNED(out) && SE_ALIGNED(du) && SE_ALIGNED(z) && SE_ALIGNED(ds),
          "se_bwd_apply: misaligned buffer");
  SE_LAUNCH(k_se_bwd_apply, H * W, C, N, stream, (const bf16_t*)dout, (const bf16_t*)out, z, ds, (bf16_t*)du, H * W, C,
            ds_bf16);
  return 0;
}


// Fused multi-head self-attention (ops_attn.hip).  qkv / dqkv: bf16 [B][L][3][H][D]; o / dout: bf16 [B][L][H][D]; lse:
// fp32 [B][H][L].
static const char* attn_rule(int B, int L, int H, int D) {
  static const char* rule =
      "attn: the attention rule is dense bf16 qkv [B, L, 3, H, D] with D == 64, 1 <= L <= 256, B, H >= 1 and fewer "
      "than 2^31 elements";
  if (B <= 0 || H <= 0 || D != 64 || L < 1 || L > 256) return rule;
  if ((long)B * L * 3 * H * D >= (1L << 31)) return rule;  // (B * H fits the grid, element offsets fit 32 bits)
  return nullptr;
}
int dca_ops_attn_rule(int B, int L, int H, int D) {
  const char* e = attn_rule(B, L, H, D);
  REQUIRE(!e, e);
  return 0;
}
#define ATTN_ALIGNED(p) ((uintptr_t)(p) % 16 == 0)
// o = softmax(scale q k^T) v per (b, h), lse = the rows' log-sum-exp of the scaled scores
int dca_ops_attn_fwd(const void* qkv, void* o, float* lse, int B, int L, int H, int D, float scale, void* stream) {
  const char* e = attn_rule(B, L, H, D);
  REQUIRE(!e, e);
  REQUIRE(qkv && o && lse, "attn_fwd: buffer missing");
  REQUIRE(ATTN_ALIGNED(qkv) && ATTN_ALIGNED(o) && ATTN_ALIGNED(lse), "attn_fwd: misaligned buffer");
  if (L <= 96) OPCK(at_fwd_launch<3>(qkv, o, lse, B, L, H, scale, stream));
  else if (L <= 224) OPCK(at_fwd_launch<7>(qkv, o, lse, B, L, H, scale, stream));
  else OPCK(at_fwd_launch<8>(qkv, o, lse, B, L, H, scale, stream));
  return 0;
}

// dqkv (every element written once) from the forward's operands, o, lse and dout
int dca_ops_attn_bwd(const void* qkv, const void* o, const float* lse, const void* dout, void* dqkv, int B, int L,
                     int H, int D, float scale, void* stream) {
  const char* e = attn_rule(B, L, H, D);
  REQUIRE(!e, e);
  REQUIRE(qkv && o && lse && dout && dqkv, "attn_bwd: buffer missing");
  REQUIRE(ATTN_ALIGNED(qkv) && ATTN_ALIGNED(o) && ATTN_ALIGNED(lse) && ATTN_ALIGNED(dout) && ATTN_ALIGNED(dqkv),
          "attn_bwd: misaligned buffer");
  const int lds = at_bwd_lds(L);
  OPCK(hipFuncSetAttribute((const void*)k_attn_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(k_attn_bwd, dim3((unsigned)B * (unsigned)H), dim3(AT_NT), lds, (hipStream_t)stream,
                     (const bf16_t*)qkv, (const bf16_t*)o, lse, (const bf16_t*)dout, (bf16_t*)dqkv, L, H, scale);
  OPCK(hipGetLastError());
  return 0;
}

// Fused residual-add LayerNorm and GELU (ops_ln.hip).  Rows are bf16, gamma / beta the fp32 master parameters.
static const char* ln_rule(long M, int C, int ldx) {
  static const char* rule =
      "ln: the LayerNorm rule is bf16 rows [M][ldx] of which the first C elements are read, with C % 8 == 0, "
      "64 <= C <= 2048, ldx >= C, ldx % 8 == 0, M >= 1, fewer than 2^31 elements and 16-byte aligned bases";
  if (C % 8 || C < 64 || C > 2048 || ldx < C || ldx % 8 || M < 1) return rule;
  if (M * (long)ldx >= (1L << 31)) return rule;
  return nullptr;
}
static const char* gelu_rule(long R, int N) {
  static const char* rule =
      "gelu: the GELU rule is dense bf16 [R][N] with N % 8 == 0, R, N >= 1, fewer than 2^31 elements and 16-byte "
      "aligned bases";
  if (R < 1 || N < 1 || N % 8 || R * (long)N >= (1L << 31)) return rule;
  return nullptr;
}
int dca_ops_ln_rule(long M, int C, int ldx) {
  const char* e = ln_rule(M, C, ldx);
  REQUIRE(!e, e);
  return 0;
}
int dca_ops_gelu_rule(long R, int N) {
  const char* e = gelu_rule(R, N);
  REQUIRE(!e, e);
  return 0;
}
#define LN_ALIGNED(p) ((uintptr_t)(p) % 16 == 0)
// x, delta (optional): rows of stride ldx; hsum (written only with delta), y: [M][C]; stats: fp32 [M][2] (mean, rstd);
// max_wg: the most workgroups
int dca_ops_ln_fwd(const void* x, const void* delta, const float* gamma, const float* beta, void* hsum, void* y,
                   float* stats, long M, int C, int ldx, float eps, int max_wg, void* stream) {
  const char* e = ln_rule(M, C, ldx);
  REQUIRE(!e, e);
  REQUIRE(x && gamma && beta && y && stats && (!delta || hsum) && max_wg >= 1, "ln_fwd: buffer missing");
  REQUIRE(LN_ALIGNED(x) && LN_ALIGNED(delta) && LN_ALIGNED(gamma) && LN_ALIGNED(beta) && LN_ALIGNED(hsum) &&
              LN_ALIGNED(y) && LN_ALIGNED(stats), e = ln_rule(0, 0, 0));
  int G, cpl;
  ln_pick(C, &G, &cpl);
#define LN_CALL(g, c) OPCK((ln_fwd_launch<g, c>(x, delta, gamma, beta, hsum, y, stats, (int)M, C, ldx, eps, max_wg, stream)))
  LN_DISPATCH(G, cpl, LN_CALL, REQUIRE(false, "ln_fwd: no kernel for this row width"));
#undef LN_CALL
  return 0;
}

// h: the forward's hsum (or its x when there was no delta), rows of stride ldh; dy, dres (optional), dx: [M][C];
// part: slabs * 2 * C floats; dgb: fp32 [2][C] = (dgamma, dbeta)
int dca_ops_ln_bwd(const void* h, int ldh, const void* dy, const void* dres, const float* gamma, const float* stats,
                   void* dx, float* part, float* dgb, long M, int C, int slabs, void* stream) {
  const char* e = ln_rule(M, C, ldh);
  REQUIRE(!e, e);
  REQUIRE(h && dy && gamma && stats && dx && part && dgb && slabs >= 1, "ln_bwd: buffer missing");
  REQUIRE(LN_ALIGNED(h) && LN_ALIGNED(dy) && LN_ALIGNED(dres) && LN_ALIGNED(gamma) && LN_ALIGNED(stats) &&
              LN_ALIGNED(dx) && LN_ALIGNED(part) && LN_ALIGNED(dgb), e = ln_rule(0, 0, 0));
  int G, cpl;
  ln_pick(C, &G, &cpl);
#define LN_CALL(g, c) OPCK((ln_bwd_launch<g, c>(h, ldh, dy, dres, gamma, stats, dx, part, (int)M, C, &slabs, stream)))
  LN_DISPATCH(G, cpl, LN_CALL, REQUIRE(false, "ln_bwd: no kernel for this row width"));
#undef LN_CALL
  hipLaunchKernelGGL(k_ln_colsum, dim3((2 * C + 63) / 64), dim3(256), 0, (hipStream_t)stream, (const float*)part, slabs,
                     2 * C, dgb, 0);
  OPCK(hipGetLastError());
  return 0;
}

// a = bf16(gelu(z)), z and a dense bf16 [R][N]
int dca_ops_gelu_fwd(const void* z, void* a, long R, int N, void* stream) {
  const char* e = gelu_rule(R, N);
  REQUIRE(!e, e);
  REQUIRE(z && a, "gelu_fwd: buffer missing");
  REQUIRE(LN_ALIGNED(z) && LN_ALIGNED(a), e = gelu_rule(0, 0));
  const long n8 = R * N / 8;
  hipLaunchKernelGGL(k_gelu_fwd, dim3(grid_for(n8, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)z, (bf16_t*)a, n8);
  OPCK(hipGetLastError());
  return 0;
}

// dz = bf16(dy gelu'(z)) and db [N] (+)= the column sums of the fp32 dz.  dy [R][N] fp32 or bf16 (dy_bf16); part:
// nchunk * N floats
int dca_ops_gelu_bwd(const void* dy, int dy_bf16, const void* z, void* dz, float* part, float* db, long R, int N,
                     int nchunk, int accumulate, void* stream) {
  const char* e = gelu_rule(R, N);
  REQUIRE(!e, e);
  REQUIRE(dy && z && dz && part && db && nchunk >= 1 && nchunk <= 65535, "gelu_bwd: buffer missing");
  REQUIRE(LN_ALIGNED(dy) && LN_ALIGNED(z) && LN_ALIGNED(dz) && LN_ALIGNED(part), e = gelu_rule(0, 0));
  const int rpb = (int)((R + nchunk - 1) / nchunk), chunks = (int)((R + rpb - 1) / rpb);
  const dim3 g((N + 255) / 256, chunks), b(256);
  hipStream_t st = (hipStream_t)stream;
  if (dy_bf16)
    hipLaunchKernelGGL((k_gelu_bwd<bf16_t>), g, b, 0, st, (const bf16_t*)dy, (const bf16_t*)z, (bf16_t*)dz, part,
                       (int)R, N, rpb);
  else
    hipLaunchKernelGGL((k_gelu_bwd<float>), g, b, 0, st, (const float*)dy, (const bf16_t*)z, (bf16_t*)dz, part, (int)R,
                       N, rpb);
  OPCK(hipGetLastError());
  hipLaunchKernelGGL(k_ln_colsum, dim3((N + 63) / 64), dim3(256), 0, st, (const float*)part, chunks, N, db, accumulate);
  OPCK(hipGetLastError());
  return 0;
}

}  // extern "C"
