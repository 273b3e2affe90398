// Native runtime of the NetResDeep training engine: owns the device workspace, enqueues the fused kernel
// sequence of one training step, captures it (including the RCCL gradient collectives) into a hipGraph per
// batch size and replays it.  Exposed to Python through a small C ABI (ctypes), see runtime/engine.py.
//
// DDP semantics (reference main.py:63, torch DDP):
//   * gradients are averaged over ranks: sum all-reduce + 1/world_size scaling fused into the SGD kernel;
//   * bucket A (fc1/fc2, 86.6 % of the bytes) is all-reduced on a comm stream while the 10 trunk backward kernels
//     run (the reference's single 25 MiB bucket gives zero overlap);
//   * bucket B (trunk conv, BN affine, stem) carries rank 0's BN running statistics in a 64-float tail segment,
//     which replaces DDP's per-forward buffer broadcast (CC4) at zero extra collective latency.
#include <rccl/rccl.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "netresdeep_kernels.hip"
#include "optimizer.h"
#include "xgmi_allreduce.hip"
#include "netresdeep_pks.hip"
#include "netresdeep_eval.hip"
#include "engine_plan.h"

namespace {

thread_local std::string g_err;

#define HIPCK(x)                                                                   \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      g_err = std::string(#x) + ": " + hipGetErrorString(e_);                      \
      return -1;                                                                   \
    }                                                                              \
  } while (0)
#define NCCK(x)                                                                    \
  do {                                                                             \
    ncclResult_t r_ = (x);                                                         \
    if (r_ != ncclSuccess) {                                                       \
      g_err = std::string(#x) + ": " + ncclGetErrorString(r_);                     \
      return -1;                                                                   \
    }                                                                              \
  } while (0)

}  // namespace

extern "C" {

// Must match runtime/engine.py::_DcaInit field by field.
struct DcaInit {
  float* params;
  float* grads;
  float* rm;
  float* rv;
  long long* nbt;
  const uint8_t* data;
  const int* labels;
  int n_data;
  int bmax;
  int bf16;
  int rows;  // trunk tile rows R (2 or 4)
  float lr;
  float bn_mom;
  float bn_eps;
  int world_size;
  int rank;
  const char* nccl_id;  // 128 bytes (world_size > 1)
  int persistent;       // 1: the one-launch image-sliced persistent step kernel (netresdeep_pks.hip)
  int debug;            // persistent engine: also store X / DY / G / conv1 pre-activations for diagnostics
  int comm_mode;        // world_size > 1: 0 = RCCL inside the step; 1 = external (host drives the all-reduce
                        // between dca_engine_run_part(.., 1) and (.., 2); test/debug path, no RCCL communicator);
                        // 2 = xGMI one-shot (peer-to-peer reads of IPC-mapped gradient slabs, fused with SGD)
  int force_comm;       // comm_mode 0 at world_size 1: still run the RCCL all-reduce + averaging SGD (tests)
  int auto_engine;      // the persistent engine was chosen automatically: keep one workgroup of co-residency
                        // slack (else the caller asked for it explicitly and may use every CU)
  int loopback;         // world_size 1, comm_mode 2: run the xGMI exchange path with this rank as its own single
                        // peer (uncached region, slab write-through, flags, peer reads, averaging SGD), so the
                        // protocol's per-step cost is measurable on one device (bench.py --loopback)
};

}  // extern "C"

namespace dca {

struct Engine {
  DcaInit in{};
  Ctx base{};
  int R = 4, RW = 16, TPI = 4;
  bool bf = true;
  hipStream_t st = nullptr, cst = nullptr;
  hipEvent_t evA = nullptr, evB = nullptr, evC = nullptr;
  char* wsp = nullptr;
  size_t ws_bytes = 0;
  int* indices = nullptr;
  int n_indices = 0;
  // dca_engine_run_checked: pinned host copies of the two error words per in-flight chunk + their events
  unsigned* err_host = nullptr;  // [CHK_RING][2]
  hipEvent_t chk_ev[4] = {};
  ncclComm_t comm = nullptr;
  // comm_mode 2 (xGMI one-shot): this rank's shared region and every rank's mapping of it
  char* xregion = nullptr;
  xg::Peers peers{};
  bool peers_open = false;
  unsigned long long ar_deadline = 300ull * 100000000ull;  // 300 s in 100 MHz ticks (a peer may be in host code)
  std::map<int, hipGraphExec_t> graphs;
  bool persistent = false;  // the image-sliced persistent step kernel (netresdeep_pks.hip; default)
  pks::Args qa{};
  bool comm_on = false;  // the step ends with a gradient collective (dca::comm_on: world_size > 1, or force_comm)
  int per_cu = 0, ncu = 0;  // persistent engine: step workgroups per CU (occupancy) and CUs of the device
  int staged_b = 0;  // persistent engine: batch slots of the current staging parity that hold the next batch
  int last_b = 0;    // batch size of the last enqueued step (BN slots are re-zeroed when it changes)
  int fc_in_step = 1;  // the fc1 / fc-tail gradient segments run on the step kernel's fc workers (pks::N_FCW extra
                       // workgroups beside the backward); off: in the reduction kernel.  Off whenever the step and
                       // its fc workers would exceed the co-resident budget, and when xGMI peers share this device
  int shared_device = 0;  // set by the host: number of xGMI ranks on this device (shared-GPU rehearsal; 0/1: not
                          // shared): the coarse 107-segment layout, and fc workers only when every co-scheduled
                          // grid fits (fc_in_step_for), so a spinning kernel always leaves CUs for a peer's step
  // The workspace: one table drives allocation, offsets, the name lookup and the pointer binding (alloc_workspace)
  struct Region {
    const char* name;
    size_t bytes;
    void** dst;           // the Ctx / pks::Args / Peers field that points at the region (null: reached by name only)
    char* ptr = nullptr;  // 256-byte aligned, in table order
  };
  std::vector<Region> regions;
  // kernel entry points for the selected (BF, R, RW) instantiation; their LDS sizes are the plan's (engine_plan.h)
  void (*kstep)(Ctx, pks::Args, pks::RedAr) = nullptr;
  void (*kxgmi)(Ctx, xg::Peers, const float*, float*, unsigned*, int, unsigned long long) = nullptr;
  void (*kstem)(Ctx) = nullptr;
  void (*kfwd)(Ctx, int) = nullptr;
  void (*khead1)(Ctx) = nullptr;
  void (*khead2)(Ctx) = nullptr;
  void (*kbwd)(Ctx, int) = nullptr;
  void (*kred)(Ctx, int, int) = nullptr;
  void (*kapply)(Ctx, int) = nullptr;
  // optimiser pass (optimizer.hip; dca_engine_set_optimizer).  Off: every step applies its own plain SGD as before.
  // On: the step takes the "split" form -- gradient reduced (and all-reduced) into cx.grads unapplied, then k_apply_opt
  bool opt_on = false;
  OptDev* optdev = nullptr;     // device copy: hyper-parameters, step counter, ticket
  OptDev opt{};                 // host mirror of the hyper-parameters (step / ticket live on the device only)
  float* lr_table = nullptr;    // device learning-rate table (owned)
  bool ema_on = false;          // the pass runs in its EMA form (dca_engine_set_ema; opt.ema is then set)
  bool clip_on = false;         // the pass runs in its CLIP form behind k_grad_sqnorm (dca_engine_set_clip)
  bool acc_on = false;          // the pass runs in its ACC form behind k_grad_accum (dca_engine_set_accum)
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The kernels chosen by the dtype alone (named in this order, the compiler keeps the code object's kernel order)
static void bind_dtype_kernels(Engine* e) {
  e->kstep = e->bf ? pks::k_pks_step<0> : pks::k_pks_step<1>;
  e->kxgmi = e->bf ? xg::k_xgmi_ar_sgd<true> : xg::k_xgmi_ar_sgd<false>;
}
template <bool BF, int R, int RW>
static void bind_kernels(Engine* e) {
  e->kstem = k_stem_block0<BF, R>;
  e->kfwd = k_fwd_block<BF, R>;
  e->khead1 = k_head1<R>;
  e->khead2 = k_head2<R>;
  e->kbwd = k_bwd_block<BF, R, RW>;
  e->kred = k_reduce<BF>;
  e->kapply = k_apply_sgd<BF>;
}

// What the step plan reads of this engine (engine_plan.h)
static PlanIn plan_in(const Engine* e) {
  const DcaInit& in = e->in;
  PlanIn p{};
  p.persistent = e->persistent;
  p.bf16 = e->bf;
  p.rows = in.rows;
  p.world_size = in.world_size;
  p.comm_mode = in.comm_mode;
  p.force_comm = in.force_comm;
  p.loopback = in.loopback;
  p.opt_on = e->opt_on;
  p.shared_device = e->shared_device;
  p.fc_in_step = e->fc_in_step;
  p.per_cu = e->per_cu;
  p.ncu = e->ncu;
  p.full_device = !in.auto_engine;
  p.bmax = in.bmax;
  return p;
}
// engine_plan with the engine's error convention: -1 and the reason in g_err when the step cannot run
static int plan_step(const PlanIn& in, int B, int part, StepPlan* p) {
  if (const char* why = engine_plan(in, B, part, p)) {
    g_err = why;
    return -1;
  }
  return 0;
}

static int alloc_workspace(Engine* e) {
  const size_t bmax = e->in.bmax;
  const size_t pstride = bmax * e->TPI;
  const size_t nslab = 9 * bmax * (16 / e->RW) + pstride;
  const size_t esz = e->bf ? 2 : 4;
  Ctx& c = e->base;
  pks::Args& qa = e->qa;
#define TO(field) (void**)&(field)
  e->regions = {
      {"X", 10 * bmax * 8192 * 4, TO(c.X)},
      {"Y", 10 * bmax * 8192 * 4, TO(c.Y)},
      {"DY", 10 * bmax * 8192 * 4, TO(c.DY)},
      {"G", 2 * bmax * 8192 * 4, TO(c.G)},
      {"SCODE", bmax * 8192, TO(c.SCODE)},
      {"FPART", 10 * pstride * 32 * 8, TO(c.FPART)},
      {"STATS", 10 * 32 * 8, TO(c.STATS)},
      {"BPART", 2 * pstride * 32 * 8, TO(c.BPART)},
      {"WSLAB", nslab * WSLAB_N * 4, TO(c.WSLAB)},
      {"SSLAB", pstride * SSLAB_N * 4, TO(c.SSLAB)},
      {"HP", bmax * 2048 * 4, TO(c.HP)},
      {"HH", bmax * 32 * 4, TO(c.HH)},
      {"HDH", bmax * 32 * 4, TO(c.HDH)},
      {"HDL", bmax * 16 * 4, TO(c.HDL)},
      {"HLOSS", bmax * 4, TO(c.HLOSS)},
      {"HPART", pstride * 32 * 4, TO(c.HPART)},
      {"HCODE", bmax * 2048, TO(c.HCODE)},
      {"WT_F", 9216 * esz, TO(c.wt_f)},
      {"WT_D", 9216 * esz, TO(c.wt_d)},
      {"SW", 1024 * esz, TO(c.sw)},
      {"RS_BASE", 64 * 4, TO(c.rs_base)},
      {"CURSOR", 16, TO(c.cursor)},
      {"STEPS", 16, TO(c.step_count)},
      {"LOSS", 16, TO(c.loss_acc)},
      {"STAMPS", 32 * 256 * 8 * 2 * 8, TO(c.stamps)},
      {"EPOCH", 16, TO(qa.epoch)},
      {"ERR", 16, TO(qa.err)},
      {"TSLAB", bmax * pks::S * WSLAB_N * 4, TO(qa.tslab)},
      {"BNG", 64 * 4, TO(qa.bng)},
      {"W1B", 65536 * 2, TO(c.w1b)},
      {"SIMG", 2 * 64 * 3072, TO(qa.simg)},
      {"SLAB", 2 * 64 * 4, TO(qa.slab)},
      {"COMMT", 16, TO(e->peers.ticks)},
      {"PKW", PKW_N * 2, TO(c.pkw)},
      {"PKS_GRAN", 2 * (size_t)pks::LMAX * pks::GSTR * 8, TO(qa.gran)},
      {"PKS_YH", 10 * (size_t)pks::LMAX * 2 * 512 * 4, TO(qa.yh)},
      {"PKS_BNX", 2 * (size_t)pks::LMAX * 64 * 4, TO(qa.bnx)},
      {"PKS_HDONE", (size_t)pks::LMAX * 8, TO(qa.hdone)},  // head-done granules
      {"C1", e->in.debug ? bmax * 32 * 1024 * 4 : 16, TO(qa.c1)},
  };
#undef TO
  size_t total = 0;
  for (auto& r : e->regions) total += align_up(r.bytes, 256);
  HIPCK(hipMalloc(&e->wsp, total));
  HIPCK(hipMemset(e->wsp, 0, total));
  e->ws_bytes = total;
  size_t off = 0;
  for (auto& r : e->regions) {
    r.ptr = e->wsp + off;
    if (r.dst) *r.dst = r.ptr;
    off += align_up(r.bytes, 256);
  }
  c.pstride = (int)pstride;
  qa.debug = e->in.debug;
  // derived weight copies: each engine writes only the layouts its kernels read (derive_param skips null ones)
  c.swf = nullptr;
  if (e->persistent) c.wt_f = c.wt_d = c.sw = nullptr;
  else c.w1b = c.pkw = nullptr;
  return 0;
}

static int set_lds_limits(Engine* e) {
  const MkLds L = mk_lds(e->bf, e->R);
  const int lds[] = {L.stem, L.fwd, L.head1, L.head2, std::max(std::max(L.dgrad, L.dgrad0), std::max(L.wgrad, L.fc)),
                     e->bf ? pks::Plan<0>::TOTAL : pks::Plan<1>::TOTAL};
  const void* fn[] = {(const void*)e->kstem,  (const void*)e->kfwd, (const void*)e->khead1,
                      (const void*)e->khead2, (const void*)e->kbwd, (const void*)e->kstep};
  for (int i = 0; i < 6; ++i) HIPCK(hipFuncSetAttribute(fn[i], hipFuncAttributeMaxDynamicSharedMemorySize, lds[i]));
  return 0;
}

// comm_mode 2: the one-shot xGMI all-reduce of `src` over the peers P.  sgd 1: fused with the averaging SGD (replaces
// all-reduce + k_apply_sgd); sgd 0: the sum (CC4 tail included) lands in dst
static void launch_xgmi(Engine* e, const Ctx& cx, const xg::Peers& P, const float* src, float* dst, int sgd,
                        unsigned long long deadline) {
  hipLaunchKernelGGL(e->kxgmi, dim3(xg::AR_NB), dim3(xg::AR_T), 0, e->st, cx, P, src, dst, e->qa.err + 1, sgd, deadline);
}
// A step's xGMI all-reduce of its gradient.  apply: with the averaging SGD; else summed into dst (optimiser mode:
// cx.grads, k_apply_opt follows)
static int enqueue_xgmi(Engine* e, const Ctx& cx, float* dst, int apply) {
  launch_xgmi(e, cx, e->peers, cx.grads, dst, apply, e->ar_deadline);
  HIPCK(hipGetLastError());
  return 0;
}

// The optimiser pass over the flat buffer (momentum, weight decay, the step's learning rate; derived weight copies;
// CC4 base) -- in place of the step's own SGD when an optimiser is set.
static int enqueue_opt_pass(Engine* e, const Ctx& cx) {
  if (e->clip_on) HIPCK(launch_grad_sqnorm(cx, e->opt.part, e->st));  // the CLIP form reads its partials
  if (e->opt.rule != dca::OPT_SGD) {
    HIPCK(launch_apply_adam(e->bf, e->ema_on, e->opt.rule == dca::OPT_ADAMW, e->clip_on, e->acc_on, cx, e->optdev,
                            e->st));
    return 0;
  }
  HIPCK(launch_apply_opt(e->bf, e->ema_on, e->clip_on, e->acc_on, cx, e->optdev, e->st));
  return 0;
}
// With accumulation on, k_grad_accum first folds the step's gradient into opt.acc, and the norm kernel and the pass
// read that buffer in the gradient's place: the same kernels on a Ctx whose `grads` points at it (cx.grads keeps
// the micro-step's own gradient).
static int enqueue_apply_opt(Engine* e, const Ctx& cx) {
  if (!e->acc_on) return enqueue_opt_pass(e, cx);
  HIPCK(launch_grad_accum(cx, e->optdev, e->st));
  Ctx ax = cx;
  ax.grads = e->opt.acc;
  return enqueue_opt_pass(e, ax);
}

// RCCL, multi-kernel engine: bucket B (everything behind bucket A) is all-reduced on the comm stream once the
// reduction has written it, and the step's stream waits for it
static int enqueue_bucket_b(Engine* e, const Ctx& cx) {
  HIPCK(hipEventRecord(e->evB, e->st));
  HIPCK(hipStreamWaitEvent(e->cst, e->evB, 0));
  NCCK(ncclAllReduce(cx.grads + OFF_CONVW, cx.grads + OFF_CONVW, FLAT_N - OFF_CONVW, ncclFloat32, ncclSum, e->comm,
                     e->cst));
  HIPCK(hipEventRecord(e->evC, e->cst));
  HIPCK(hipStreamWaitEvent(e->st, e->evC, 0));
  return 0;
}

// What follows the gradient reduction (StepTail): the collective on the reduced gradient, then the update.  RCCL: the
// sliced engine all-reduces the whole buffer on its own stream; the multi-kernel engine has bucket A in flight
// already (enqueue_step) and adds bucket B.
static int enqueue_tail(Engine* e, const Ctx& cx, int tail) {
  if (tail == TAIL_XGMI_SGD) return enqueue_xgmi(e, cx, nullptr, 1);
  if (tail == TAIL_XGMI_OPT && enqueue_xgmi(e, cx, cx.grads, 0)) return -1;
  if (tail == TAIL_RCCL_SGD || tail == TAIL_RCCL_OPT) {
    if (e->persistent) NCCK(ncclAllReduce(cx.grads, cx.grads, FLAT_N, ncclFloat32, ncclSum, e->comm, e->st));
    else if (enqueue_bucket_b(e, cx)) return -1;
  }
  if (tail == TAIL_XGMI_OPT || tail == TAIL_RCCL_OPT || tail == TAIL_OPT) return enqueue_apply_opt(e, cx);
  if (tail == TAIL_RCCL_SGD || tail == TAIL_SGD) hipLaunchKernelGGL(e->kapply, dim3(64), dim3(NT), 0, e->st, cx, 1);
  HIPCK(hipGetLastError());
  return 0;
}

// The segment arguments of a sliced launch (pks::RedAr): the peers' regions, the exchange's error word and deadline,
// the segment mode, the flags word and the segment layout.
static pks::RedAr red_args(const Engine* e, int mode, int flags, int seg_ch, unsigned long long deadline) {
  pks::RedAr ra{};
  ra.peers = e->peers;
  ra.err = e->qa.err + 1;
  ra.deadline = deadline;
  ra.mode = mode;
  ra.fc_in_step = flags;
  ra.seg_ch = seg_ch;
  return ra;
}
// Mode 3, the exchange self-test: the pattern `src` travels through the segments' protocol into `dst` (outside the
// training comm-time counters)
static pks::RedAr selftest_redar(const Engine* e, const float* src, float* dst, int flags,
                                 unsigned long long deadline) {
  pks::RedAr ra = red_args(e, 3, flags, seg_ch(plan_in(e)), deadline);
  ra.peers.ticks = nullptr;
  ra.st_src = src;
  ra.st_dst = dst;
  ra.st_n = FLAT_N;
  return ra;
}

// The sliced engine's reduction kernel in the plan's form (k_pks_reduce_ar<0|1|2>)
static void launch_reduce_ar(Engine* e, int form, int grid, int lds, const Ctx& cx, int nslab, const pks::RedAr& ra) {
  auto* k = pks::k_pks_reduce_ar<1>;
  if (form == 2) k = pks::k_pks_reduce_ar<2>;
  if (form == 0) k = pks::k_pks_reduce_ar<0>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(256), lds, e->st, cx, e->qa, nslab, ra);
}
// The same kernel as the self-test runs it: every segment exchanged in the reduction kernel, batch 1
static void launch_selftest_reduce(Engine* e, const pks::RedAr& ra) {
  Ctx cx = e->base;
  cx.B = 1;
  launch_reduce_ar(e, 0, reduce_grid(plan_in(e), pks::seg_layout(ra.seg_ch).nseg), pks::stage_floats(1) * 4, cx, 1, ra);
}

// Enqueue one training step for batch B on e->st (and e->cst for the multi-kernel engine's collectives): plan, then
// launch what the plan says.  `part`: see engine_plan.
static int enqueue_step(Engine* e, int B, int part = 0) {
  StepPlan p;
  if (plan_step(plan_in(e), B, part, &p)) return -1;
  if (part != 2 && e->comm_on && e->in.comm_mode == 2 && !e->peers_open) {
    g_err = "xGMI all-reduce: peers not mapped (call dca_engine_ipc_open first)";
    return -1;
  }
  Ctx cx = e->base;
  cx.B = B;
  if (e->persistent) {
    // the sliced step kernel, then ONE kernel for reduction + all-reduce + SGD (mode: see k_pks_reduce_ar); its
    // segments + its bookkeeping, epoch and cursor advanced by one step
    if (part != 2) {
      pks::RedAr ra = red_args(e, p.mode, pks::ra_flags(p.fc, 0, 0), p.seg_ch, e->ar_deadline);
      hipLaunchKernelGGL(e->kstep, dim3(p.step_grid), dim3(p.step_block), p.step_lds, e->st, cx, e->qa, ra);
      HIPCK(hipGetLastError());
      ra.fc_in_step = pks::ra_flags(p.fc, 0, 1);
      launch_reduce_ar(e, p.reduce_form, p.reduce_grid, p.reduce_lds, cx, B * pks::S, ra);
    }
    return enqueue_tail(e, cx, p.tail);
  }
  if (e->opt_on) cx.fuse_sgd = 0;  // k_reduce writes the gradient only; k_apply_opt applies it
  if (part != 2) {
    const dim3 blk(NT), fgrid(p.fwd_grid);
    hipLaunchKernelGGL(e->kstem, fgrid, blk, p.stem_lds, e->st, cx);
    for (int i = 1; i < NBLK; ++i) hipLaunchKernelGGL(e->kfwd, fgrid, blk, p.fwd_lds, e->st, cx, i);
    hipLaunchKernelGGL(e->khead1, fgrid, blk, p.head1_lds, e->st, cx);
    hipLaunchKernelGGL(e->khead2, fgrid, blk, p.head2_lds, e->st, cx);
    for (int i = NBLK - 1; i >= 0; --i) {
      const bool top = i == NBLK - 1;
      hipLaunchKernelGGL(e->kbwd, dim3(top ? p.bwd9_grid : p.bwd_grid), blk,
                         top ? p.bwd9_lds : (i ? p.bwd_lds : p.bwd0_lds), e->st, cx, i);
      if (top && p.overlap_a) {  // bucket A ready: overlap its all-reduce with the trunk bwd
        HIPCK(hipEventRecord(e->evA, e->st));
        HIPCK(hipStreamWaitEvent(e->cst, e->evA, 0));
        NCCK(ncclAllReduce(cx.grads, cx.grads, BUCKET_A_END, ncclFloat32, ncclSum, e->comm, e->cst));
      }
    }
    hipLaunchKernelGGL(e->kred, dim3(p.reduce_grid), blk, 0, e->st, cx, p.nslab, p.nparts);
  }
  return enqueue_tail(e, cx, p.tail);
}

}  // namespace dca


using dca::Engine;

extern "C" {

const char* dca_last_error() { return g_err.c_str(); }

int dca_abi_version() { return 10; }  // bump with every DcaInit / signature change

int dca_nccl_unique_id(char* out128) {
  ncclUniqueId id;
  NCCK(ncclGetUniqueId(&id));
  static_assert(sizeof(ncclUniqueId) == 128, "unexpected ncclUniqueId size");
  memcpy(out128, &id, 128);
  return 0;
}

static int prime_ids(Engine* e);
static void engine_free(Engine* e);

// Body of dca_engine_create; on failure the caller frees whatever was acquired (engine_free handles a partially
// built engine), so every early return of HIPCK / NCCK is leak-free.
static int engine_init(Engine* e, const DcaInit* in, int n_indices) {
  e->in = *in;
  e->bf = in->bf16 != 0;
  e->R = in->rows;
  e->RW = e->bf ? 16 : 8;
  if (in->bmax < 1 || in->bmax > dca::BMAX_LIMIT) {
    g_err = "batch_max must be in [1, 64]";
    return -1;
  }
  if (e->R != 2 && e->R != 4) {
    g_err = "rows must be 2 or 4";
    return -1;
  }
  e->TPI = 16 / e->R;
  e->persistent = in->persistent != 0;
  if (in->loopback && (in->world_size != 1 || in->comm_mode != 2)) {
    g_err = "loopback needs world_size 1 and comm_mode 2 (xGMI)";
    return -1;
  }
  e->comm_on = dca::comm_on(dca::plan_in(e));
  if (e->bf && e->R == 4) dca::bind_kernels<true, 4, 16>(e);
  else if (e->bf) dca::bind_kernels<true, 2, 16>(e);
  else if (e->R == 4) dca::bind_kernels<false, 4, 8>(e);
  else dca::bind_kernels<false, 2, 8>(e);
  dca::bind_dtype_kernels(e);
  if (dca::set_lds_limits(e)) return -1;
  if (e->persistent) {
    // Co-residency: the persistent step spins on in-kernel exchanges, so every one of its bmax workgroups must be
    // resident at once.  The occupancy answer can be one block per CU high near register edges (MI355X guide,
    // Residency): require a margin of one block per CU below it.
    int dev = 0, ncu = 0, per_cu = 0;
    HIPCK(hipGetDevice(&dev));
    HIPCK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    HIPCK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &per_cu, (const void*)e->kstep, dca::pks::NTH, e->bf ? dca::pks::Plan<0>::TOTAL : dca::pks::Plan<1>::TOTAL));
    // one step workgroup per CU (256 VGPRs): a grid of every CU would leave no slack for anything else on the
    // device (another stream's kernel, another process), so an automatically chosen engine keeps a margin of one
    // workgroup -- batch 64 (256 workgroups) then falls back to the multi-kernel engine with a warning; an
    // explicit persistent=True may use every CU (coresident_budget)
    e->per_cu = per_cu;
    e->ncu = ncu;
    const int need = dca::pks_live(in->bmax);
    if (dca::share_budget(dca::plan_in(e)) < need) {
      g_err = "persistent engine: " + std::to_string(need) + " workgroups cannot all be resident (" +
              std::to_string(per_cu) + " per CU x " + std::to_string(ncu) + " CUs); use the multi-kernel engine";
      return -1;
    }
    if (const char* fo = getenv("DCA_PKS_FC_IN_STEP")) e->fc_in_step = fo[0] != '0';
  }
  HIPCK(hipStreamCreateWithFlags(&e->st, hipStreamNonBlocking));
  HIPCK(hipStreamCreateWithFlags(&e->cst, hipStreamNonBlocking));
  HIPCK(hipEventCreateWithFlags(&e->evA, hipEventDisableTiming));
  HIPCK(hipEventCreateWithFlags(&e->evB, hipEventDisableTiming));
  HIPCK(hipEventCreateWithFlags(&e->evC, hipEventDisableTiming));
  for (auto& ev : e->chk_ev) HIPCK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  HIPCK(hipHostMalloc((void**)&e->err_host, 4 * 2 * sizeof(unsigned), hipHostMallocDefault));
  memset(e->err_host, 0, 4 * 2 * sizeof(unsigned));
  if (dca::alloc_workspace(e)) return -1;
  e->n_indices = n_indices;
  HIPCK(hipMalloc(&e->indices, sizeof(int) * (size_t)std::max(n_indices, 1)));
  HIPCK(hipMemset(e->indices, 0, sizeof(int) * (size_t)std::max(n_indices, 1)));
  dca::Ctx& c = e->base;
  c.ws = in->world_size;
  c.rank = in->rank;
  c.fuse_sgd = e->comm_on ? 0 : 1;
  c.lr = in->lr;
  c.bn_mom = in->bn_mom;
  c.bn_eps = in->bn_eps;
  c.inv_ws = 1.f / (float)in->world_size;
  c.params = in->params;
  c.grads = in->grads;
  c.rm = in->rm;
  c.rv = in->rv;
  c.nbt = in->nbt;
  c.data = in->data;
  c.labels = in->labels;
  c.indices = e->indices;
  c.n_data = in->n_data;
  c.n_idx = std::max(n_indices, 1);
  if ((in->world_size > 1 || in->loopback) && in->comm_mode == 2) {
    if (in->world_size > dca::xg::MAXR) {
      g_err = "xGMI all-reduce: world_size > 8 (one node) -- use RCCL";
      return -1;
    }
    // uncached device memory: peers read it over xGMI and no L2 may hold a stale line of it
    // two halves: [0, REGION_BYTES) k_xgmi_ar_sgd (multi-kernel / per-image engines); [REGION_BYTES, 2x) the
    // sliced engine's fused reduce + all-reduce (own flags and slabs: their epochs never mix)
    if (hipExtMallocWithFlags((void**)&e->xregion, 2 * dca::xg::REGION_BYTES, hipDeviceMallocUncached) != hipSuccess) {
      (void)hipGetLastError();
      HIPCK(hipMalloc(&e->xregion, 2 * dca::xg::REGION_BYTES));
    }
    HIPCK(hipMemset(e->xregion, 0, 2 * dca::xg::REGION_BYTES));
    HIPCK(hipDeviceSynchronize());
    const char* dl = getenv("DCA_XGMI_TIMEOUT_S");
    if (dl) e->ar_deadline = (unsigned long long)(atof(dl) * 1e8);
    if (in->loopback) {  // the rank is its own (only) peer: no IPC mapping
      e->peers.base[0] = e->xregion;
      e->peers_open = true;
    }
  }
  if (e->comm_on && in->comm_mode == 0) {
    ncclUniqueId id;
    if (in->world_size == 1) NCCK(ncclGetUniqueId(&id));  // force_comm: a private 1-rank communicator
    else memcpy(&id, in->nccl_id, 128);
    NCCK(ncclCommInitRank(&e->comm, in->world_size, id, in->rank));
  }
  if (prime_ids(e)) return -1;
  HIPCK(hipStreamSynchronize(e->st));
  return 0;
}

int dca_engine_create(const DcaInit* in, int n_indices, void** out) {
  Engine* e = new Engine();
  if (engine_init(e, in, n_indices)) {
    const std::string err = g_err;
    engine_free(e);
    g_err = err;
    return -1;
  }
  *out = e;
  return 0;
}

// Release everything an Engine holds; safe on a partially initialised engine.
static void engine_free(Engine* e) {
  if (e->st) (void)hipStreamSynchronize(e->st);
  if (e->cst) (void)hipStreamSynchronize(e->cst);
  for (auto& kv : e->graphs) (void)hipGraphExecDestroy(kv.second);
  if (e->comm) (void)ncclCommDestroy(e->comm);
  for (int q = 0; q < dca::xg::MAXR; ++q)
    if (e->peers_open && !e->in.loopback && q != e->in.rank && q < e->in.world_size && e->peers.base[q])
      (void)hipIpcCloseMemHandle(e->peers.base[q]);
  if (e->xregion) (void)hipFree(e->xregion);
  if (e->wsp) (void)hipFree(e->wsp);
  if (e->optdev) (void)hipFree(e->optdev);
  if (e->lr_table) (void)hipFree(e->lr_table);
  if (e->indices) (void)hipFree(e->indices);
  if (e->err_host) (void)hipHostFree(e->err_host);
  for (auto& ev : e->chk_ev)
    if (ev) (void)hipEventDestroy(ev);
  if (e->evA) (void)hipEventDestroy(e->evA);
  if (e->evB) (void)hipEventDestroy(e->evB);
  if (e->evC) (void)hipEventDestroy(e->evC);
  if (e->st) (void)hipStreamDestroy(e->st);
  if (e->cst) (void)hipStreamDestroy(e->cst);
  delete e;
}

int dca_engine_destroy(void* h) {
  if (h) engine_free((Engine*)h);
  return 0;
}

// Rebuild the MFMA-layout weight copies from the fp32 parameters (after init / load_state_dict / broadcast)
// and snapshot the running stats as the rank-0 base.  Synchronous.
int dca_engine_derive(void* h) {
  Engine* e = (Engine*)h;
  hipLaunchKernelGGL(e->kapply, dim3(64), dim3(dca::NT), 0, e->st, e->base, 0);
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(e->st));
  return 0;
}

// persistent engine: the batch ids of the next step are produced by the previous step; re-derive them whenever
// the host moves the cursor or replaces the index list
static int prime_ids(Engine* e) {
  if (!e->persistent) return 0;  // the multi-kernel engine gathers its batch inside the stem kernel
  hipLaunchKernelGGL(dca::pks::k_pks_prime, dim3(64), dim3(256), 0, e->st, e->base, e->qa);
  HIPCK(hipGetLastError());
  e->staged_b = 64;
  return 0;
}
// A persistent step of batch B stages only B slots of the next batch; a following larger batch re-primes.
static int ensure_staged(Engine* e, int B) {
  if (e->persistent && B > e->staged_b && prime_ids(e)) return -1;
  if (e->persistent) e->staged_b = B;
  // sliced engine: a workgroup absent from the last steps (smaller batch) left BN slots whose 2-bit tags could
  // match again; zeroed slots (tag 0) never match (bn_tag)
  if (e->persistent && B != e->last_b) {
    HIPCK(hipMemsetAsync(e->qa.bnx, 0, 2 * (size_t)dca::pks::LMAX * 64 * 4, e->st));
  }
  e->last_b = B;
  return 0;
}

int dca_engine_set_indices(void* h, const int* host_idx, int n) {
  Engine* e = (Engine*)h;
  if (n > e->n_indices) {
    g_err = "too many indices";
    return -1;
  }
  HIPCK(hipMemcpyAsync(e->indices, host_idx, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, e->st));
  if (prime_ids(e)) return -1;
  HIPCK(hipStreamSynchronize(e->st));
  return 0;
}

int dca_engine_set_cursor(void* h, int v) {
  Engine* e = (Engine*)h;
  HIPCK(hipMemcpyAsync(e->base.cursor, &v, sizeof(int), hipMemcpyHostToDevice, e->st));
  if (prime_ids(e)) return -1;
  HIPCK(hipStreamSynchronize(e->st));
  return 0;
}

// Seed the step epoch (and, xGMI, every exchange flag of this rank's region) -- the epoch-wrap test hook: e.g.
// EPOCH_WRAP - 3 and 2^32 - 3, so the next steps cross both wraps (pks::EPOCH_WRAP for the device epoch: staging
// parity, BN tags, granule tags; 2^32 for the per-segment / per-workgroup exchange flags).  Every tag holder whose
// validity depends on the epoch (BN partial slots, halo / head granules, head-done granules) is zeroed, because an
// arbitrary jump could make a stale slot's tag match (a zero tag never does); the next batch is re-staged into the
// new epoch's parity.  xGMI: collective -- every rank seeds the same flag value while no rank is stepping (barrier
// before and after), since peers write into this rank's flag area.  Synchronous.
int dca_engine_set_epoch(void* h, int device_epoch, int flag_epoch) {
  Engine* e = (Engine*)h;
  if (!e->persistent) {
    g_err = "set_epoch: the sliced (persistent) engine only";
    return -1;
  }
  if (device_epoch < 0 || (unsigned)device_epoch >= dca::pks::EPOCH_WRAP) {
    g_err = "set_epoch: device epoch outside [0, EPOCH_WRAP)";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  HIPCK(hipMemcpy(e->qa.epoch, &device_epoch, sizeof(int), hipMemcpyHostToDevice));
  HIPCK(hipMemset(e->qa.gran, 0, 2 * (size_t)dca::pks::LMAX * dca::pks::GSTR * 8));
  HIPCK(hipMemset(e->qa.bnx, 0, 2 * (size_t)dca::pks::LMAX * 64 * 4));
  HIPCK(hipMemset(e->qa.hdone, 0, (size_t)dca::pks::LMAX * 8));
  if (e->xregion) {
    std::vector<int> f(dca::xg::FLAG_BYTES / 4, flag_epoch);
    HIPCK(hipMemcpy(e->xregion, f.data(), dca::xg::FLAG_BYTES, hipMemcpyHostToDevice));                 // k_xgmi_ar_sgd
    HIPCK(hipMemcpy(e->xregion + dca::xg::REGION_BYTES, f.data(), dca::xg::FLAG_BYTES, hipMemcpyHostToDevice));  // segments
  }
  if (prime_ids(e)) return -1;
  HIPCK(hipStreamSynchronize(e->st));
  return 0;
}

// The current device epoch (synchronous).
int dca_engine_epoch(void* h, int* out) {
  Engine* e = (Engine*)h;
  HIPCK(hipStreamSynchronize(e->st));
  HIPCK(hipMemcpy(out, e->qa.epoch, sizeof(int), hipMemcpyDeviceToHost));
  return 0;
}

// Device-side error flags: flags[0] of the persistent engine (bit r: BN exchange round r timed out),
// flags[1] of the xGMI all-reduce (bit 31: a peer-flag wait timed out).  Synchronises; reset clears them.
int dca_engine_errors(void* h, unsigned* flags, int reset) {
  Engine* e = (Engine*)h;
  HIPCK(hipStreamSynchronize(e->st));
  HIPCK(hipMemcpy(flags, e->qa.err, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));
  if (reset) HIPCK(hipMemset(e->qa.err, 0, 2 * sizeof(unsigned)));
  return 0;
}

// Read (and optionally reset) the device-side loss accumulator.  Synchronises the engine stream.
int dca_engine_read_loss(void* h, double* loss, int* steps, int reset) {
  Engine* e = (Engine*)h;
  HIPCK(hipStreamSynchronize(e->st));
  HIPCK(hipMemcpy(loss, e->base.loss_acc, sizeof(double), hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(steps, e->base.step_count, sizeof(int), hipMemcpyDeviceToHost));
  if (reset) {
    HIPCK(hipMemset(e->base.loss_acc, 0, sizeof(double)));
    HIPCK(hipMemset(e->base.step_count, 0, sizeof(int)));
  }
  return 0;
}

// Enqueue `nsteps` training steps of batch B.  use_graph: replay a captured hipGraph (captured on first use).
constexpr int GRAPH_CHUNK = 16;  // steps per graph replay (remainders: 8 / 4 / 2 / 1-step graphs, <= 4 extra launches)

// The executable graph of `chunk` consecutive steps of batch B (captured and instantiated on first use).
static hipGraphExec_t capture_graph(Engine* e, int B, int chunk) {
  const int key = B * 1024 + chunk;
  auto it = e->graphs.find(key);
  if (it != e->graphs.end()) return it->second;
  hipGraph_t g;
  hipError_t ec = hipStreamBeginCapture(e->st, hipStreamCaptureModeThreadLocal);
  if (ec != hipSuccess) {
    g_err = std::string("hipStreamBeginCapture: ") + hipGetErrorString(ec);
    return nullptr;
  }
  int rc = 0;
  for (int s = 0; s < chunk && !rc; ++s) rc = dca::enqueue_step(e, B);
  ec = hipStreamEndCapture(e->st, &g);
  if (rc) {
    if (ec == hipSuccess) (void)hipGraphDestroy(g);
    return nullptr;
  }
  if (ec != hipSuccess) {
    g_err = std::string("hipStreamEndCapture: ") + hipGetErrorString(ec);
    return nullptr;
  }
  hipGraphExec_t ex;
  ec = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ec != hipSuccess) {
    g_err = std::string("hipGraphInstantiate: ") + hipGetErrorString(ec);
    return nullptr;
  }
  // upload now (stream-ordered), so the first replay -- possibly inside a timed region -- does not pay it
  ec = hipGraphUpload(ex, e->st);
  if (ec != hipSuccess) {
    (void)hipGraphExecDestroy(ex);
    g_err = std::string("hipGraphUpload: ") + hipGetErrorString(ec);
    return nullptr;
  }
  e->graphs.emplace(key, ex);
  return ex;
}

// The argument checks dca_engine_run, _run_checked and _precapture share (external_ok: comm_mode 1 is no error here)
static int check_run_args(const Engine* e, int B, int nsteps, bool external_ok = false) {
  if (B < 1 || B > e->in.bmax || nsteps < 0) {
    g_err = "batch out of range";
    return -1;
  }
  if (!external_ok && e->in.world_size > 1 && e->in.comm_mode == 1) {
    g_err = "comm_mode 1 (external all-reduce): drive steps with dca_engine_run_part";
    return -1;
  }
  return 0;
}

// Graph chunk sizes of `nsteps` steps in launch order: first_chunk-step graphs, then the halves down to 1 (<= 4
// extra launches for the remainder).  Steps are replayed from graphs holding several consecutive steps (the data
// cursor / batch ids advance on the device, so consecutive steps need no host input): launching one graph per step
// leaves a ~5-8 us gap between graph launches on the GPU (rocprofv3, profiles/), inside a graph consecutive kernels
// are back to back.
static std::vector<int> chunk_order(int nsteps, int first_chunk) {
  std::vector<int> order;
  for (int chunk = first_chunk; chunk >= 1; chunk /= 2)
    for (; nsteps >= chunk; nsteps -= chunk) order.push_back(chunk);
  return order;
}

int dca_engine_run(void* h, int B, int nsteps, int use_graph) {
  Engine* e = (Engine*)h;
  if (check_run_args(e, B, 0)) return -1;
  if (nsteps > 0 && ensure_staged(e, B)) return -1;
  if (!use_graph) {
    for (int s = 0; s < nsteps; ++s)
      if (dca::enqueue_step(e, B)) return -1;
    return 0;
  }
  for (const int chunk : chunk_order(nsteps, GRAPH_CHUNK)) {
    hipGraphExec_t ex = capture_graph(e, B, chunk);
    if (ex == nullptr) return -1;
    HIPCK(hipGraphLaunch(ex, e->st));
  }
  return 0;
}

// dca_engine_run with the device error words checked after EVERY graph chunk, without stalling the GPU: behind each
// chunk an async copy of the two words into pinned host memory and an event; before launching chunk k + 2 the host
// waits for chunk k's event (chunk k + 1 keeps the GPU busy meanwhile) and reads its words.  An exchange timeout
// (BN exchange of the step, or a peer that stopped stepping in the xGMI all-reduce) therefore stops the run within
// two 8-step chunks (< 16 steps) instead of at the epoch end; after the first timed-out wait the kernels do not wait
// again (fail fast on the error word), so those steps are quick.  Returns 0, or 1 when an error word was set (*steps_done:
// steps of the chunks enqueued before stopping; the words stay set for dca_engine_errors); -1 on a HIP error.
// Synchronous: the stream is drained before returning.
int dca_engine_run_checked(void* h, int B, int nsteps, int* steps_done) {
  Engine* e = (Engine*)h;
  constexpr int RING = 4;
  *steps_done = 0;
  if (check_run_args(e, B, nsteps)) return -1;
  if (nsteps > 0 && ensure_staged(e, B)) return -1;
  // 8-step chunks: a failure is seen within < 16 steps (2 chunks in flight)
  const std::vector<int> order = chunk_order(nsteps, 8);
  int launched = 0, rc = 0;
  size_t k = 0, checked = 0;
  auto check = [&](size_t j) -> int {  // chunk j's words (its event first)
    hipEvent_t ev = e->chk_ev[j % RING];
    if (hipEventSynchronize(ev) != hipSuccess) return -1;
    const unsigned* w = e->err_host + 2 * (j % RING);
    return (w[0] | w[1]) ? 1 : 0;
  };
  for (; k < order.size(); ++k) {
    if (k >= 2) {  // keep <= 2 chunks in flight behind the check
      const int r = check(checked++);
      if (r < 0) HIPCK(hipGetLastError());
      if (r) {
        rc = 1;
        break;
      }
    }
    hipGraphExec_t ex = capture_graph(e, B, order[k]);
    if (ex == nullptr) return -1;
    HIPCK(hipGraphLaunch(ex, e->st));
    HIPCK(hipMemcpyAsync(e->err_host + 2 * (k % RING), e->qa.err, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, e->st));
    HIPCK(hipEventRecord(e->chk_ev[k % RING], e->st));
    launched += order[k];
  }
  while (rc == 0 && checked < k) {
    const int r = check(checked++);
    if (r < 0) HIPCK(hipGetLastError());
    if (r) rc = 1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  *steps_done = launched;
  return rc;
}

// Capture (without running) the graphs dca_engine_run replays for batch B, so a later timed run never pays
// capture + instantiate.  Synchronous.
int dca_engine_precapture(void* h, int B) {
  Engine* e = (Engine*)h;
  if (check_run_args(e, B, 0, true)) return -1;
  if (e->in.world_size > 1 && e->in.comm_mode == 1) return 0;  // external all-reduce: eager only
  for (const int chunk : chunk_order(2 * GRAPH_CHUNK - 1, GRAPH_CHUNK))  // one graph of each size: 16, 8, 4, 2, 1
    if (capture_graph(e, B, chunk) == nullptr) return -1;
  HIPCK(hipStreamSynchronize(e->st));
  return 0;
}

// Time spent inside the gradient all-reduce kernel (xGMI path: workgroup 0 of k_xgmi_ar_sgd, entry to exit,
// including the wait for the slowest peer), summed since the last reset: microseconds and calls.
int dca_engine_comm_time(void* h, double* us, long long* calls, int reset) {
  Engine* e = (Engine*)h;
  HIPCK(hipStreamSynchronize(e->st));
  unsigned long long v[2] = {0, 0};
  HIPCK(hipMemcpy(v, e->peers.ticks, sizeof(v), hipMemcpyDeviceToHost));
  *us = (double)v[0] / 100.0;  // s_memrealtime: 100 MHz
  *calls = (long long)v[1];
  if (reset) HIPCK(hipMemset(e->peers.ticks, 0, sizeof(v)));
  return 0;
}

// comm_mode 2: the IPC handle (64 bytes) of this rank's shared region, to be all-gathered by the host.
int dca_engine_ipc_handle(void* h, char* out64) {
  Engine* e = (Engine*)h;
  if (!e->xregion) {
    g_err = "ipc_handle: engine not created with comm_mode 2";
    return -1;
  }
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "unexpected hipIpcMemHandle_t size");
  hipIpcMemHandle_t hd;
  HIPCK(hipIpcGetMemHandle(&hd, e->xregion));
  memcpy(out64, &hd, 64);
  return 0;
}

// comm_mode 2: map every peer's region (`all` = world_size handles of 64 bytes, in rank order).
int dca_engine_ipc_open(void* h, const char* all, int world) {
  Engine* e = (Engine*)h;
  if (!e->xregion || world != e->in.world_size) {
    g_err = "ipc_open: engine not created with comm_mode 2, or world size mismatch";
    return -1;
  }
  for (int q = 0; q < world; ++q) {
    if (q == e->in.rank) {
      e->peers.base[q] = e->xregion;
      continue;
    }
    hipIpcMemHandle_t hd;
    memcpy(&hd, all + 64 * q, 64);
    void* p = nullptr;
    HIPCK(hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess));
    e->peers.base[q] = (char*)p;
  }
  e->peers_open = true;
  return 0;
}

// comm_mode 2 self-test: one all-reduce (no SGD) of `n = FLAT_N` floats from device `src` into device `dst`
// through the same protocol, epochs and slabs as a training step.  Collective: every rank must call it.
// timeout_s bounds the flag waits; returns 1 in *timed_out when a wait expired.  Synchronous.
int dca_engine_ipc_selftest(void* h, const float* src, float* dst, float timeout_s, int* timed_out) {
  Engine* e = (Engine*)h;
  if (!e->peers_open) {
    g_err = "ipc_selftest: peers not mapped";
    return -1;
  }
  HIPCK(hipMemsetAsync(e->qa.err + 1, 0, sizeof(unsigned), e->st));
  const unsigned long long dl = (unsigned long long)((double)timeout_s * 1e8);
  if (e->persistent) {  // the path a sliced training step uses: per-segment exchange inside the fused reduce kernel
    dca::launch_selftest_reduce(e, dca::selftest_redar(e, src, dst, 0, dl));  // (flags 0: every segment)
  } else {
    dca::xg::Peers P = e->peers;
    P.ticks = nullptr;  // a self-test is not training-step communication (metrics)
    dca::launch_xgmi(e, e->base, P, src, dst, 0, dl);
  }
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(e->st));
  unsigned f = 0;
  HIPCK(hipMemcpy(&f, e->qa.err + 1, sizeof(unsigned), hipMemcpyDeviceToHost));
  HIPCK(hipMemset(e->qa.err + 1, 0, sizeof(unsigned)));
  *timed_out = (f & 0x80000000u) ? 1 : 0;
  return 0;
}

// comm_mode 2, sliced engine: the same collective self-test through the STEP kernel's fc workers (the in-step
// exchange of the fc1 blocks and the fc tail that runs beside the trunk backward): k_pks_step launched with batch 0,
// i.e. N_FCW fc workers and no step workgroups, in self-test mode.  Only the fc segments' slab range is written to
// dst: [*lo, *hi).  Each fc worker waits only for the same segment of its peers, so ranks sharing a device need no
// co-residency budget here.  Collective; synchronous.
int dca_engine_ipc_selftest_fc(void* h, const float* src, float* dst, float timeout_s, int* timed_out, int* lo,
                               int* hi) {
  Engine* e = (Engine*)h;
  if (!e->peers_open || !e->persistent) {
    g_err = "ipc_selftest_fc: needs the sliced engine with mapped peers";
    return -1;
  }
  HIPCK(hipMemsetAsync(e->qa.err, 0, 2 * sizeof(unsigned), e->st));
  const dca::pks::RedAr ra = dca::selftest_redar(e, src, dst, 1, (unsigned long long)((double)timeout_s * 1e8));
  dca::Ctx cx = e->base;
  cx.B = 0;  // no step workgroups: the whole grid is fc workers
  // one workgroup per fc segment, or (ranks sharing the device) the rank's CU budget: every rank's workgroup f waits
  // for its peers' workgroup f, so all ranks' grids must be co-resident (a step-kernel workgroup takes a whole CU)
  const dim3 grid(std::min(dca::pks::N_FCW, dca::share_budget(dca::plan_in(e))));
  hipLaunchKernelGGL(e->kstep, grid, dim3(dca::pks::NTH), e->bf ? dca::pks::Plan<0>::TOTAL : dca::pks::Plan<1>::TOTAL,
                     e->st, cx, e->qa, ra);
  HIPCK(hipGetLastError());
  HIPCK(hipStreamSynchronize(e->st));
  unsigned f[2] = {0, 0};
  HIPCK(hipMemcpy(f, e->qa.err, sizeof(f), hipMemcpyDeviceToHost));
  HIPCK(hipMemset(e->qa.err, 0, sizeof(f)));
  *timed_out = ((f[1] & 0x80000000u) || f[0]) ? 1 : 0;
  const dca::pks::SegLayout L = dca::pks::seg_layout(ra.seg_ch);
  *lo = L.off_fc1;
  *hi = std::min(L.off_fct + 362, (int)dca::FLAT_N);
  return 0;
}

// comm_mode 2 protocol latency: `iters` back-to-back all-reduces (no SGD) of FLAT_N floats; writes the mean
// microseconds per all-reduce (HIP events around the loop).  Collective: every rank must call it.
int dca_engine_ipc_bench(void* h, const float* src, float* dst, int iters, float* us) {
  Engine* e = (Engine*)h;
  if (!e->peers_open || iters < 1) {
    g_err = "ipc_bench: peers not mapped or iters < 1";
    return -1;
  }
  hipEvent_t a, b;
  HIPCK(hipEventCreate(&a));
  HIPCK(hipEventCreate(&b));
  HIPCK(hipEventRecord(a, e->st));
  dca::xg::Peers P = e->peers;
  P.ticks = nullptr;  // benchmark traffic stays out of the training comm-time counters
  // sliced engine: the exchange a sliced training step runs: every gradient segment, self-test mode
  const dca::pks::RedAr ra = dca::selftest_redar(e, src, dst, 0, e->ar_deadline);
  for (int i = 0; i < iters; ++i) {
    if (e->persistent) dca::launch_selftest_reduce(e, ra);
    else dca::launch_xgmi(e, e->base, P, src, dst, 0, e->ar_deadline);
  }
  HIPCK(hipEventRecord(b, e->st));
  HIPCK(hipEventSynchronize(b));
  float ms = 0.f;
  HIPCK(hipEventElapsedTime(&ms, a, b));
  *us = 1e3f * ms / (float)iters;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return 0;
}

// comm_mode 1: one part of a step, eager (see engine_plan)
int dca_engine_run_part(void* h, int B, int part) {
  Engine* e = (Engine*)h;
  if (B < 1 || B > e->in.bmax || part < 1 || part > 2 || e->in.world_size < 2 || e->in.comm_mode != 1) {
    g_err = "run_part: needs world_size > 1, comm_mode 1, part 1 or 2, batch in range";
    return -1;
  }
  if (part == 1 && ensure_staged(e, B)) return -1;
  return dca::enqueue_step(e, B, part);
}

int dca_engine_sync(void* h) {
  Engine* e = (Engine*)h;
  HIPCK(hipStreamSynchronize(e->st));
  HIPCK(hipStreamSynchronize(e->cst));
  return 0;
}

// Drop the captured step graphs (the step's kernel chain is about to change).  The stream must be idle.
static void drop_graphs(Engine* e) {
  for (auto& kv : e->graphs) (void)hipGraphExecDestroy(kv.second);
  e->graphs.clear();
}

// Sliced engine: the host reports that `n` xGMI ranks share this device (shared-GPU rehearsal; the largest such
// count over all devices, so every rank picks the same layout): the coarse gradient-segment layout and the
// co-residency rule of fc_in_step_for.  Collective in effect: every rank must make the same call before
// stepping.  Drops the captured graphs.
int dca_engine_set_shared_device(void* h, int n) {
  Engine* e = (Engine*)h;
  if (e->persistent && n > 1) {
    const int budget = dca::coresident_budget(e->per_cu, e->ncu, n, false);
    if (dca::pks_live(e->in.bmax) > budget) {
      g_err = "shared device: " + std::to_string(n) + " ranks x " + std::to_string(dca::pks_live(e->in.bmax)) +
              " step workgroups (batch_max " + std::to_string(e->in.bmax) + ") exceed the per-rank co-residency budget " +
              "of " + std::to_string(budget) + " of the device's " + std::to_string(e->per_cu * e->ncu) +
              " workgroup slots (one kept free); use batch_max <= " + std::to_string(budget / dca::pks::S);
      return -1;
    }
  }
  HIPCK(hipStreamSynchronize(e->st));
  drop_graphs(e);
  e->shared_device = n > 1 ? n : 0;
  return 0;
}

// Optimiser of the fused step: SGD with momentum `mu` and weight decay `wd` (optimizer.hip).  `momentum_buf`: flat
// fp32 [FLAT_ALLOC] device buffer owned by the caller (layout of params / grads; the caller zeroes or restores it);
// null turns the optimiser off again (the step's own plain SGD).  The learning rate is the engine's constant one until
// dca_engine_set_lr_table installs a table; the step counter starts at 0.  Turning the mode on or off drops the
// captured graphs (a different kernel chain); new mu / wd values on an engine already in optimiser mode reach the
// captured graphs as they are (device memory).  Synchronous.
int dca_engine_set_optimizer(void* h, float* momentum_buf, float mu, float wd) {
  Engine* e = (Engine*)h;
  if (momentum_buf && (!(mu >= 0.f) || !(wd >= 0.f))) {
    g_err = "set_optimizer: momentum and weight decay must not be negative";
    return -1;
  }
  if (momentum_buf && ((uintptr_t)momentum_buf % 16)) {
    g_err = "set_optimizer: the momentum buffer must be 16-byte aligned";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  const bool on = momentum_buf != nullptr;
  if (on != e->opt_on) drop_graphs(e);
  e->opt_on = false;  // (on again below, once the device block is complete)
  if (!on) {  // the EMA form, the CLIP form and the Adam rule go with the pass
    e->ema_on = false;
    e->clip_on = false;
    e->acc_on = false;
    e->opt.part = nullptr;
    e->opt.acc = nullptr;
    e->opt.ema = nullptr;
    e->opt.rule = dca::OPT_SGD;
    e->opt.v = nullptr;
    return 0;
  }
  if (e->optdev == nullptr) {  // first use: step 0, ticket 0, no table
    e->opt = dca::OptDev{};
    e->opt.lr_const = e->in.lr;
    e->opt.buf = momentum_buf;
    e->opt.mu = mu;
    e->opt.wd = wd;
    e->opt.b1p = e->opt.b2p = 1.0;  // beta^0
    dca::OptDev* d = nullptr;
    HIPCK(hipMalloc((void**)&d, sizeof(dca::OptDev)));
    if (hipMemcpy(d, &e->opt, sizeof(dca::OptDev), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      g_err = "set_optimizer: copy failed";
      return -1;
    }
    e->optdev = d;
  } else {  // keep the device's step counter
    e->opt.buf = momentum_buf;
    e->opt.mu = mu;
    e->opt.wd = wd;
    HIPCK(hipMemcpy(e->optdev, &e->opt, offsetof(dca::OptDev, step), hipMemcpyHostToDevice));
  }
  e->opt_on = true;
  return 0;
}

// Per-step learning rates of the optimiser pass: step k uses values[min(k, n - 1)]; n = 0 returns to the engine's
// constant learning rate.  Captured graphs pick the new table up without re-capture.  Synchronous.
int dca_engine_set_lr_table(void* h, const float* values, int n) {
  Engine* e = (Engine*)h;
  if (!e->opt_on) {
    g_err = "set_lr_table: no optimiser set (dca_engine_set_optimizer first)";
    return -1;
  }
  if (n < 0 || (n > 0 && !values)) {
    g_err = "set_lr_table: bad table";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  float* tab = nullptr;
  if (n > 0) {
    HIPCK(hipMalloc((void**)&tab, sizeof(float) * (size_t)n));
    if (hipMemcpy(tab, values, sizeof(float) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(tab);
      g_err = "set_lr_table: copy failed";
      return -1;
    }
  }
  float* old = e->lr_table;
  e->lr_table = tab;
  e->opt.lr_table = tab;
  e->opt.n_table = n;
  HIPCK(hipMemcpy(e->optdev, &e->opt, offsetof(dca::OptDev, step), hipMemcpyHostToDevice));
  if (old) (void)hipFree(old);
  return 0;
}

// EMA form of the optimiser pass: after every update the pass also averages the model into `ema_buf`, a flat fp32
// [FLAT_ALLOC] device buffer owned by the caller in the gradient buffer's layout (the caller fills it with the model
// to start from): e = p' + d * (e - p') over the parameters and over running_mean | running_var, d = `decay` or, with
// `warmup`, min(decay, (1 + k) / (10 + k)) at optimiser step k.  Needs the optimiser on; null turns the form off.
// Switching it on or off drops the captured graphs (another kernel); a new decay, warm-up flag or buffer on a running
// EMA reaches them as it is (device memory).  Synchronous.
int dca_engine_set_ema(void* h, float* ema_buf, float decay, int warmup) {
  Engine* e = (Engine*)h;
  if (!e->opt_on) {
    g_err = "set_ema: no optimiser set (dca_engine_set_optimizer first)";
    return -1;
  }
  if (ema_buf && !(decay >= 0.f && decay < 1.f)) {
    g_err = "set_ema: the decay must lie in [0, 1)";
    return -1;
  }
  if (ema_buf && ((uintptr_t)ema_buf % 16)) {
    g_err = "set_ema: the EMA buffer must be 16-byte aligned";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  const bool on = ema_buf != nullptr;
  if (on != e->ema_on) drop_graphs(e);
  e->ema_on = false;  // (on again below, once the device block holds the buffer)
  e->opt.ema = ema_buf;
  e->opt.ema_decay = on ? decay : 0.f;
  e->opt.ema_warmup = on && warmup ? 1 : 0;
  HIPCK(hipMemcpy(e->optdev, &e->opt, offsetof(dca::OptDev, step), hipMemcpyHostToDevice));
  e->ema_on = on;
  return 0;
}

// CLIP form of the optimiser pass: every update first scales the averaged gradient to a global L2 norm of at most
// `max_norm` (torch.nn.utils.clip_grad_norm_; optimizer.hip).  `part_buf`: dca_engine_clip_parts() doubles of device
// memory owned by the caller (8-byte aligned; workspace of the norm kernel).  Needs the optimiser on; null turns the
// form off.  Switching it on or off drops the captured graphs (one more launch); a new max_norm on a running CLIP form
// reaches them as it is (device memory).  Synchronous.
int dca_engine_set_clip(void* h, double* part_buf, float max_norm) {
  Engine* e = (Engine*)h;
  if (!e->opt_on) {
    g_err = "set_clip: no optimiser set (dca_engine_set_optimizer first)";
    return -1;
  }
  if (part_buf && !(max_norm > 0.f)) {
    g_err = "set_clip: max_norm must be positive";
    return -1;
  }
  if (part_buf && ((uintptr_t)part_buf % 8)) {
    g_err = "set_clip: the partial-sum buffer must be 8-byte aligned";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  const bool on = part_buf != nullptr;
  if (on != e->clip_on) drop_graphs(e);
  e->clip_on = false;  // (on again below, once the device block holds the buffer)
  e->opt.part = part_buf;
  e->opt.max_norm = on ? max_norm : 0.f;
  HIPCK(hipMemcpy(e->optdev, &e->opt, offsetof(dca::OptDev, step), hipMemcpyHostToDevice));
  e->clip_on = on;
  return 0;
}

// Doubles in the workspace dca_engine_set_clip takes.
int dca_engine_clip_parts(void) { return dca::OPT_PARTS; }

// What the CLIP form recorded: *gnorm <- the last update's gradient norm before clipping (0 before the first),
// *n_clipped <- updates whose norm exceeded max_norm since the last reset; reset != 0 clears that counter.  Synchronous.
int dca_engine_clip_state(void* h, double* gnorm, int* n_clipped, int reset) {
  Engine* e = (Engine*)h;
  if (!e->opt_on || !e->clip_on || !gnorm || !n_clipped) {
    g_err = "clip_state: clipping is not on (dca_engine_set_clip first)";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  unsigned n = 0;
  HIPCK(hipMemcpy(gnorm, &e->optdev->gnorm, sizeof(double), hipMemcpyDeviceToHost));
  HIPCK(hipMemcpy(&n, &e->optdev->n_clipped, sizeof(unsigned), hipMemcpyDeviceToHost));
  *n_clipped = (int)(n & 0x7fffffffu);
  if (reset) HIPCK(hipMemset(&e->optdev->n_clipped, 0, sizeof(unsigned)));
  return 0;
}

// ACC form of the optimiser pass: gradient accumulation.  Every step's summed gradient is folded into `acc_buf` by
// k_grad_accum, and only every `k`-th step's pass updates the model, on the mean of the window (optimizer.hip).
// `acc_buf`: flat fp32 [FLAT_ALLOC] device buffer owned by the caller (16-byte aligned; a window's first step
// overwrites it, so it needs no clearing).  Needs the optimiser on; null turns the form off.  Switching it on or off
// drops the captured graphs (one more launch, another form of the pass); a new `k` on a running ACC form reaches them
// as it is (device memory).  Every call restarts the window: the phase returns to 0.  Synchronous.
int dca_engine_set_accum(void* h, float* acc_buf, int k) {
  Engine* e = (Engine*)h;
  if (!e->opt_on) {
    g_err = "set_accum: no optimiser set (dca_engine_set_optimizer first)";
    return -1;
  }
  if (acc_buf && k < 1) {
    g_err = "set_accum: the number of accumulated steps must be at least 1";
    return -1;
  }
  if (acc_buf && ((uintptr_t)acc_buf % 16)) {
    g_err = "set_accum: the accumulation buffer must be 16-byte aligned";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  const bool on = acc_buf != nullptr;
  if (on != e->acc_on) drop_graphs(e);
  e->acc_on = false;  // (on again below, once the device block holds the buffer)
  e->opt.acc = acc_buf;
  e->opt.acc_k = on ? k : 0;
  e->opt.inv_k = on ? 1.f / (float)k : 0.f;
  HIPCK(hipMemcpy(e->optdev, &e->opt, offsetof(dca::OptDev, step), hipMemcpyHostToDevice));
  const int zero[2] = {0, 0};
  static_assert(offsetof(dca::OptDev, apply) == offsetof(dca::OptDev, micro) + sizeof(int), "micro | apply: one copy");
  HIPCK(hipMemcpy(&e->optdev->micro, zero, sizeof(zero), hipMemcpyHostToDevice));
  e->acc_on = on;
  return 0;
}

// The window phase of the ACC form: micro-steps already folded into the current window, in [0, k).  set = 0: *value <-
// phase; set = 1: phase <- *value (resume in mid-window; the accumulation buffer is the caller's to restore).
// Synchronous.
int dca_engine_accum_phase(void* h, int set, int* value) {
  Engine* e = (Engine*)h;
  if (!e->opt_on || !e->acc_on || !value) {
    g_err = "accum_phase: accumulation is not on (dca_engine_set_accum first)";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  if (set) {
    if (*value < 0 || *value >= e->opt.acc_k) {
      g_err = "accum_phase: the phase must lie in [0, accumulated steps)";
      return -1;
    }
    HIPCK(hipMemcpy(&e->optdev->micro, value, sizeof(int), hipMemcpyHostToDevice));
  } else {
    HIPCK(hipMemcpy(value, &e->optdev->micro, sizeof(int), hipMemcpyDeviceToHost));
  }
  return 0;
}

// The Adam rule's running products beta1^step and beta2^step, recomputed for the device's step counter (after the
// counter or the betas were set).  The stream must be idle.
static int refresh_adam_products(Engine* e) {
  int step = 0;
  HIPCK(hipMemcpy(&step, &e->optdev->step, sizeof(int), hipMemcpyDeviceToHost));
  const double prod[2] = {dca::adam_product(e->opt.beta1, step), dca::adam_product(e->opt.beta2, step)};
  static_assert(offsetof(dca::OptDev, b2p) == offsetof(dca::OptDev, b1p) + sizeof(double), "b1p | b2p are one copy");
  HIPCK(hipMemcpy(&e->optdev->b1p, prod, sizeof(prod), hipMemcpyHostToDevice));
  return 0;
}

// Update rule of the optimiser pass: Adam (`decoupled` 0: torch.optim.Adam, the weight decay of
// dca_engine_set_optimizer as an L2 term of the gradient) or AdamW (1: decay applied to the parameter), amsgrad off
// (optimizer.hip, k_apply_adam).  `v_buf`: flat fp32 [FLAT_ALLOC] device buffer owned by the caller for the second
// moment (zeroed or restored by the caller); the momentum buffer of dca_engine_set_optimizer is the first moment and
// its `mu` is not used.  Needs the optimiser on; null switches back to SGD.  Changing the rule drops the captured
// graphs (another kernel); new betas / eps on an engine already in that rule reach them as they are (device memory).
// Synchronous.
int dca_engine_set_adam(void* h, float* v_buf, double beta1, double beta2, double eps, int decoupled) {
  Engine* e = (Engine*)h;
  if (!e->opt_on) {
    g_err = "set_adam: no optimiser set (dca_engine_set_optimizer first)";
    return -1;
  }
  if (v_buf && (!(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.))) {
    g_err = "set_adam: the betas must lie in [0, 1)";
    return -1;
  }
  if (v_buf && (!(eps > 0.) || !((float)eps > 0.f) || !(eps < 3e38))) {
    g_err = "set_adam: eps must be positive (and a normal fp32 value)";
    return -1;
  }
  if (v_buf && ((uintptr_t)v_buf % 16)) {
    g_err = "set_adam: the second-moment buffer must be 16-byte aligned";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  const int rule = !v_buf ? dca::OPT_SGD : decoupled ? dca::OPT_ADAMW : dca::OPT_ADAM;
  if (rule != e->opt.rule) drop_graphs(e);
  e->opt.v = v_buf;
  e->opt.beta1 = v_buf ? beta1 : 0.;
  e->opt.beta2 = v_buf ? beta2 : 0.;
  e->opt.beta2f = (float)e->opt.beta2;
  e->opt.omb1 = v_buf ? (float)(1. - beta1) : 0.f;
  e->opt.omb2 = v_buf ? (float)(1. - beta2) : 0.f;
  e->opt.eps = v_buf ? (float)eps : 0.f;
  e->opt.rule = rule;
  HIPCK(hipMemcpy(e->optdev, &e->opt, offsetof(dca::OptDev, step), hipMemcpyHostToDevice));
  if (rule != dca::OPT_SGD) return refresh_adam_products(e);
  return 0;
}

// The optimiser pass's own step counter (it indexes the learning-rate table; unlike the loss step count it is never
// reset by a loss read).  set = 0: *value <- counter; set = 1: counter <- *value (resume; under an Adam
// rule the running products beta^step follow it).  Synchronous.
int dca_engine_opt_step(void* h, int set, int* value) {
  Engine* e = (Engine*)h;
  if (!e->opt_on || !value) {
    g_err = "opt_step: no optimiser set";
    return -1;
  }
  HIPCK(hipStreamSynchronize(e->st));
  if (set) {
    if (*value < 0) {
      g_err = "opt_step: negative step";
      return -1;
    }
    HIPCK(hipMemcpy(&e->optdev->step, value, sizeof(int), hipMemcpyHostToDevice));
    if (e->opt.rule != dca::OPT_SGD) return refresh_adam_products(e);
  } else {
    HIPCK(hipMemcpy(value, &e->optdev->step, sizeof(int), hipMemcpyDeviceToHost));
  }
  return 0;
}

// Sliced engine: 1 if a step at batch B runs the fc gradient segments on the step kernel's fc workers.
int dca_engine_fc_in_step(void* h, int B) {
  Engine* e = (Engine*)h;
  return e->persistent && dca::fc_in_step_for(dca::plan_in(e), B) ? 1 : 0;
}

// The step plan (engine_plan.h) of any configuration: needs no engine and no device.  0, or -1 with the reason the
// step cannot run in dca_last_error.
int dca_engine_step_plan(const PlanIn* in, int B, int part, StepPlan* out) {
  return dca::plan_step(*in, B, part, out);
}

// What the step plan reads of this engine: dca_engine_step_plan(out, B, part, ..) is the plan of its next step.
void dca_engine_plan_in(void* h, PlanIn* out) { *out = dca::plan_in((Engine*)h); }


// Handle of the engine stream (so Python can order torch work against it).
void* dca_engine_stream(void* h) { return ((Engine*)h)->st; }

// Device pointer of a named workspace region (tests / debugging).
void* dca_engine_region(void* h, const char* name) {
  Engine* e = (Engine*)h;
  for (const auto& r : e->regions)
    if (!strcmp(r.name, name)) return r.ptr;
  return nullptr;
}

size_t dca_engine_workspace_bytes(void* h) { return ((Engine*)h)->ws_bytes; }

// 0: multi-kernel engine; 2: persistent, image-sliced (S workgroups per image).  (1, the retired
// one-workgroup-per-image kernel, is never returned.)
int dca_engine_kind(void* h) {
  Engine* e = (Engine*)h;
  return e->persistent ? 2 : 0;
}

// Must match runtime/evaluate.py::_DcaEvalArgs field by field.
struct DcaEvalArgs {
  const float* conv1_w;  // [32][3][3][3]   fp32 master tensors (not the engine's derived copies), device pointers
  const float* conv1_b;  // [32]
  const float* conv_w;   // [32][32][3][3]  the one shared trunk conv
  const float* bn_w;     // [32]
  const float* bn_b;     // [32]
  const float* bn_rm;    // [32] running_mean
  const float* bn_rv;    // [32] running_var
  const float* fc1_w;    // [32][2048]      (16-byte aligned)
  const float* fc1_b;    // [32]
  const float* fc2_w;    // [10][32]
  const float* fc2_b;    // [10]
  float bn_eps;
  const uint8_t* data;   // [n_data][3][32][32]
  const int* labels;     // [n_data]
  int n_data;
  const int* indices;    // [n] device int32 (clamped into [0, n_data) by the kernel)
  int n;
  int bf16;              // 1: bf16 conv operands + bf16 fc1 weight; 0: 3xbf16 conv, fp32 conv1 / fc1
  int max_workgroups;    // 0: every workgroup slot of the device
  float* logits;         // [n][10] or null
  int* pred;             // [n]
  float* loss;           // [n]
};

// Eval-mode forward of `n` gathered images (netresdeep_eval.hip), enqueued on `stream`.  Everything is validated on
// the host before any device call: a bad argument returns -1 with a message and launches nothing.
int dca_eval_netresdeep(const DcaEvalArgs* a, void* stream) {
  if (!a) {
    g_err = "dca_eval_netresdeep: null argument block";
    return -1;
  }
  const void* ptrs[] = {a->conv1_w, a->conv1_b, a->conv_w, a->bn_w,   a->bn_b, a->bn_rm,   a->bn_rv, a->fc1_w,
                        a->fc1_b,   a->fc2_w,   a->fc2_b,  a->data,   a->labels, a->indices, a->pred, a->loss};
  const char* names[] = {"conv1_w", "conv1_b", "conv_w", "bn_w", "bn_b",   "bn_rm",   "bn_rv", "fc1_w",
                         "fc1_b",   "fc2_w",   "fc2_b",  "data", "labels", "indices", "pred",  "loss"};
  for (int i = 0; i < 16; ++i) {
    if (!ptrs[i]) {
      g_err = std::string("dca_eval_netresdeep: null pointer: ") + names[i];
      return -1;
    }
    // fc1_w is read in 16-byte pieces; every other tensor in 4-byte words (the image bytes too)
    const uintptr_t align = i == 7 ? 16 : 4;
    if ((uintptr_t)ptrs[i] % align) {
      g_err = std::string("dca_eval_netresdeep: misaligned pointer: ") + names[i];
      return -1;
    }
  }
  if (a->logits && (uintptr_t)a->logits % 4) {
    g_err = "dca_eval_netresdeep: misaligned pointer: logits";
    return -1;
  }
  if (a->n <= 0 || a->n_data <= 0) {
    g_err = "dca_eval_netresdeep: n and n_data must be positive";
    return -1;
  }
  if (a->max_workgroups < 0 || !(a->bn_eps >= 0.f)) {
    g_err = "dca_eval_netresdeep: max_workgroups and bn_eps must not be negative";
    return -1;
  }
  const int P = a->bf16 ? 0 : 1;
  int dev = 0;
  HIPCK(hipGetDevice(&dev));
  int grid = a->max_workgroups > 0 ? a->max_workgroups : dca::nrd_eval::default_workgroups(P, dev);
  if (grid > a->n) grid = a->n;
  dca::nrd_eval::Args ka{a->conv1_w, a->conv1_b, a->conv_w, a->bn_w, a->bn_b, a->bn_rm, a->bn_rv, a->fc1_w, a->fc1_b,
                         a->fc2_w,   a->fc2_b,   a->bn_eps, a->data, a->labels, a->n_data, a->indices, a->n,
                         a->logits,  a->pred,    a->loss};
  hipStream_t st = (hipStream_t)stream;
  if (P == 0) hipLaunchKernelGGL(dca::nrd_eval::k_nrd_eval<0>, dim3(grid), dim3(dca::nrd_eval::NTH), 0, st, ka);
  else hipLaunchKernelGGL(dca::nrd_eval::k_nrd_eval<1>, dim3(grid), dim3(dca::nrd_eval::NTH), 0, st, ka);
  HIPCK(hipGetLastError());
  return 0;
}

}  // extern "C"
