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

namespace {
thread_local GemmRoute g_route = {};      // of this thread's last dca_ops_gemm (dca_ops_gemm_last_route)
std::atomic<bool> g_lds_raised{false};    // the table's dynamic-LDS limits are set (dca_ops_gemm, once)
}  // namespace

extern "C" {

const char* dca_ops_last_error() { return g_err.c_str(); }
int dca_ops_abi_version() { return 16; }

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

}  // extern "C"
