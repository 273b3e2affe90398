// The step plan: every launch decision of one training step, as a pure function of plain integers -- no HIP call and
// no getenv, so the rule is tested without a device (tests/test_native_build.py, dca_engine_step_plan).  engine.hip
// includes this after the kernel sources, whose host-callable constants (pks::S, pks::N_FCW, pks::seg_layout,
// LdsPlan, ...) it reads; it then launches what a StepPlan says.
#pragma once

#include <algorithm>
#include <string>

extern "C" {

// What the rule depends on.  Must match runtime/native.py::PlanIn field by field.
struct PlanIn {
  int persistent;     // the sliced persistent engine (else the multi-kernel engine)
  int bf16;
  int rows;           // multi-kernel engine: trunk tile rows R (2 or 4)
  int world_size;
  int comm_mode;      // DcaInit::comm_mode: 0 RCCL, 1 external (host all-reduce between parts 1 and 2), 2 xGMI
  int force_comm;
  int loopback;
  int opt_on;         // the optimiser pass replaces the step's own SGD
  int shared_device;  // xGMI ranks on this device (0 / 1: not shared)
  int fc_in_step;     // DCA_PKS_FC_IN_STEP as read at create time
  int per_cu, ncu;    // step workgroups per CU (occupancy) and CUs of the device
  int full_device;    // the caller asked for the sliced engine explicitly: no slack CU
  int bmax;
};

// What follows the gradient reduction.
enum StepTail {
  TAIL_NONE = 0,      // nothing: the reduction applied the SGD itself (or part 1: the host all-reduces next)
  TAIL_RCCL_SGD = 1,  // RCCL all-reduce, k_apply_sgd
  TAIL_SGD = 2,       // k_apply_sgd only (part 2)
  TAIL_XGMI_OPT = 3,  // xGMI sum into the gradient, optimiser pass
  TAIL_RCCL_OPT = 4,  // RCCL all-reduce, optimiser pass
  TAIL_OPT = 5,       // optimiser pass only
  TAIL_XGMI_SGD = 6,  // multi-kernel engine: the one-shot xGMI all-reduce fused with the averaging SGD
};

// Must match runtime/native.py::StepPlan field by field.
struct StepPlan {
  int tail;         // StepTail
  int reduce_grid;  // 0 for part 2
  // sliced engine
  int budget;       // spinning workgroups this rank may hold resident
  int step_grid;    // 0 for part 2
  int step_block, step_lds;
  int fc;           // the fc gradient segments run on the step kernel's fc workers
  int mode;         // segment mode (train_mode)
  int seg_ch;
  int reduce_form;  // k_pks_reduce_ar<0|1|2>
  int reduce_lds;
  // multi-kernel engine
  int nparts, nslab;
  int fwd_grid;               // stem, forward blocks and both head kernels
  int bwd9_grid, bwd_grid;    // backward of block 9 (+ the fc workgroups) / of blocks 8..0 (+ the wgrad workgroups)
  int stem_lds, fwd_lds, head1_lds, head2_lds, bwd9_lds, bwd_lds, bwd0_lds;
  int overlap_a;              // bucket A is all-reduced on the side stream beside the trunk backward
};

}  // extern "C"

namespace dca {

// grid of the sliced step: S workgroups per image, image slots rounded up to a multiple of 8 (see k_pks_step)
static int pks_grid(int B) { return (B + 7) / 8 * 8 * pks::S; }
// the step workgroups that stay resident and spin in its exchanges (the padding ids of pks_grid exit at once)
static int pks_live(int B) { return B * pks::S; }

// Co-residency budget: how many spinning workgroups ONE rank may have resident at once -- one rule for a device of
// its own and a device shared by n ranks (the shared-GPU rehearsal).  Every workgroup of a persistent grid must be
// resident together; the occupancy answer can be one block per CU high near register edges (MI355X guide,
// Residency), so a margin stays free: one block per CU when several fit, else one CU -- unless the caller asked
// for the whole (dedicated) device explicitly.  Ranks sharing the device split what is left evenly: a rank's step
// (+ fc workers) and its reduction grid stay within its share, so a late rank always finds room for its step
// however the others are spread over their steps and reductions.  (Before round 5 the shared share was
// slots / n with no margin; 8 ranks x batch 8 filled it exactly and a BN exchange timed out.)
// Mirrored in Python: runtime/engine.py coresident_budget (CPU-tested).
static int coresident_budget(int per_cu, int ncu, int n_share, bool full_device) {
  const int slots = per_cu * ncu;
  const int margin = per_cu > 1 ? ncu : (full_device && n_share <= 1 ? 0 : 1);
  return (slots - margin) / std::max(n_share, 1);
}
// A rank's budget: the whole device's (minus the slack CU of an automatically chosen engine), or its share
static int share_budget(const PlanIn& in) {
  return coresident_budget(in.per_cu, in.ncu, in.shared_device > 1 ? in.shared_device : 1,
                           in.shared_device > 1 ? false : in.full_device != 0);
}
// gradient-segment layout (pks::seg_layout): trunk / conv1 chunks of 128 elements, 256 on a shared device (fewer
// reduction workgroups: they must leave CUs for a peer's step)
static int seg_ch(const PlanIn& in) { return in.shared_device > 1 ? 256 : 128; }

// Whether the step at batch B runs the fc gradient segments on fc workers (the live step + N_FCW fits the budget).
static bool fc_in_step_for(const PlanIn& in, int B) {
  return in.fc_in_step && pks_live(B) + pks::N_FCW <= share_budget(in);
}
// Reduction grid: one workgroup per segment + the bookkeeping one; shared device: capped at the rank's budget
// (k_pks_reduce_ar then loops over the segments).
static int reduce_grid(const PlanIn& in, int nred_plus) {
  return in.shared_device > 1 ? std::min(nred_plus, share_budget(in)) : nred_plus;
}

// The step ends with a gradient collective + an averaging update.  force_comm runs that path at world_size 1 (a
// 1-rank RCCL communicator) so the graph-captured collective is testable on one GPU; loopback does the same for the
// xGMI exchange (this rank as its only peer).
static bool comm_on(const PlanIn& in) {
  return in.world_size > 1 || (in.force_comm && in.comm_mode == 0) || in.loopback;
}
// Segment mode of a training step: 0 fused SGD (world size 1), 1 gradient only (RCCL / host all-reduce, or the
// optimiser pass: fc workers included), 2 the xGMI exchange + averaging SGD.
static int train_mode(const PlanIn& in) {
  if (in.opt_on) return 1;
  if (!comm_on(in)) return 0;
  return in.comm_mode == 2 ? 2 : 1;
}

// Dynamic LDS of the multi-kernel engine's kernels for the (BF, R, RW) instantiation bind_kernels selects
struct MkLds {
  int stem, fwd, head1, head2, dgrad, dgrad0, wgrad, fc;
};
template <bool BF, int R, int RW>
constexpr MkLds mk_lds_of() {
  using L = LdsPlan<BF, R, RW>;
  return MkLds{(int)L::stem,  (int)L::fwd,    (int)L::head1, (int)L::head2,
               (int)L::dgrad, (int)L::dgrad0, (int)L::wgrad, (int)L::fc};
}
static MkLds mk_lds(int bf16, int rows) {
  if (bf16) return rows == 4 ? mk_lds_of<true, 4, 16>() : mk_lds_of<true, 2, 16>();
  return rows == 4 ? mk_lds_of<false, 4, 8>() : mk_lds_of<false, 2, 8>();
}

// The plan of one step at batch B.  part: 0 the whole step; 1 up to (not including) the gradient all-reduce; 2 what
// follows it -- parts 1 / 2 exist for comm_mode 1, where the host runs the all-reduce in between.  Returns null, or
// the reason the step cannot run.  In the order a step is enqueued:
static const char* engine_plan(const PlanIn& in, int B, int part, StepPlan* out) {
  thread_local std::string err;
  if (B < 1 || B > in.bmax) return "batch out of range";
  if (part < 0 || part > 2 || (part && !(in.world_size > 1 && in.comm_mode == 1)))
    return "run_part: needs world_size > 1, comm_mode 1, part 1 or 2, batch in range";
  StepPlan p{};
  const bool comm = comm_on(in), xgmi = comm && in.comm_mode == 2;
  if (in.persistent) {
    // 1. co-residency: every live workgroup of the step must fit the rank's budget at once
    p.budget = share_budget(in);
    if (pks_live(B) > p.budget) {
      err = "persistent engine: " + std::to_string(pks_live(B)) + " step workgroups (batch " + std::to_string(B) +
            ") exceed the co-residency budget of " + std::to_string(p.budget) + " per rank";
      return err.c_str();
    }
    // 2. the step kernel: its grid, and the fc workers beside it when they fit too
    p.fc = fc_in_step_for(in, B);
    p.mode = train_mode(in);
    p.seg_ch = seg_ch(in);
    p.step_grid = part == 2 ? 0 : pks_grid(B) + (p.fc ? pks::N_FCW : 0);
    p.step_block = pks::NTH;
    p.step_lds = in.bf16 ? pks::Plan<0>::TOTAL : pks::Plan<1>::TOTAL;
    // 3. the reduction kernel: the lean forms (no fc segments, one exchange mode) at world size 1 and for the xGMI
    // exchange (also on a shared device, so the multi-rank rehearsals run the form a multi-GPU node runs)
    p.reduce_form = !p.fc ? 0 : (p.mode == 0 ? 1 : (p.mode == 2 ? 2 : 0));
    p.reduce_grid = part == 2 ? 0 : reduce_grid(in, pks::reduce_segments(p.fc, p.seg_ch) + 1);
    p.reduce_lds = pks::stage_floats(B) * 4;
  } else {
    // 1.-2. the kernel chain: stem, 9 forward blocks, 2 head kernels, 10 backward blocks (block 9 also computes the
    // fc gradients, the others the weight gradient of the block above), each with the LDS of what it runs
    const int tpi = 16 / in.rows, nw = B * (16 / (in.bf16 ? 16 : 8));
    const MkLds L = mk_lds(in.bf16, in.rows);
    p.nparts = B * tpi;
    p.nslab = 9 * nw + p.nparts;
    p.fwd_grid = p.nparts;
    p.bwd9_grid = p.nparts + N_FC_WG;
    p.bwd_grid = p.nparts + nw;
    p.stem_lds = L.stem;
    p.fwd_lds = L.fwd;
    p.head1_lds = L.head1;
    p.head2_lds = L.head2;
    p.bwd9_lds = std::max(L.dgrad, L.fc);
    p.bwd_lds = std::max(L.dgrad, L.wgrad);
    p.bwd0_lds = std::max(L.dgrad0, L.wgrad);
    p.overlap_a = comm && part == 0 && in.comm_mode == 0;
    // 3. k_reduce: the trunk and stem slabs, + the other tensors' workgroups when it applies the SGD itself
    const bool fuse_sgd = !comm && !in.opt_on;
    p.reduce_grid = part == 2 ? 0 : N_TRUNK_RED_WG + N_STEM_RED_WG + (fuse_sgd ? 64 : 0) + 1;
  }
  // 4. the tail: the collective on the reduced gradient, then the update
  if (part == 1) p.tail = TAIL_NONE;
  else if (part == 2) p.tail = in.opt_on ? TAIL_OPT : TAIL_SGD;
  else if (in.opt_on) p.tail = xgmi ? TAIL_XGMI_OPT : (comm ? TAIL_RCCL_OPT : TAIL_OPT);
  else if (xgmi) p.tail = in.persistent ? TAIL_NONE : TAIL_XGMI_SGD;  // (sliced: inside the reduction, mode 2)
  else p.tail = comm ? TAIL_RCCL_SGD : TAIL_NONE;
  *out = p;
  return nullptr;
}

}  // namespace dca
