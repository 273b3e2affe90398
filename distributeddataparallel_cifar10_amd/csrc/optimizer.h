// Interface of the optimiser pass (optimizer.hip): the device-memory block of its hyper-parameters and the host
// launcher.  The pass is a translation unit (and so a code object) of its own inside the engine library: the code
// object of engine.hip -- the step kernels -- stays byte for byte what it is without the pass.
#pragma once
#include "common.h"

namespace dca {

constexpr int OPT_V4 = OFF_RS / 4;              // 19019 float4 (every tensor starts 16-byte aligned)
constexpr int OPT_NB = (OPT_V4 + NT - 1) / NT;  // 75 workgroups, one float4 per thread
constexpr int OPT_PARTS = OPT_NB;               // doubles in the clipping workspace: one partial per workgroup

struct OptDev {
  const float* lr_table;  // [n_table] per-step learning rates (device), or null
  float* buf;             // momentum buffer, flat fp32 [FLAT_ALLOC] (same layout as params / grads)
  int n_table;
  float lr_const;         // the learning rate without a table
  float mu, wd;
  float* ema;             // EMA form: the averaged model, flat fp32 [FLAT_ALLOC] (the gradient buffer's layout:
                          // parameters in [0, OFF_RS), running_mean | running_var in [OFF_RS, OFF_RS + 64)), or null
  float ema_decay;        // in [0, 1)
  int ema_warmup;         // != 0: update k uses min(ema_decay, (1 + k) / (10 + k))
  // Adam forms (k_apply_adam; dca_engine_set_adam): `buf` is the first moment m, `v` the second
  float* v;               // second moment, flat fp32 [FLAT_ALLOC], or null
  double beta1, beta2;    // as given (the running products below are their powers)
  float beta2f;           // (float)beta2: v' = beta2f * v + omb2 * g'^2
  float omb1, omb2;       // (float)(1 - beta1), (float)(1 - beta2), rounded once from the doubles
  float eps;
  int rule;               // OPT_SGD, OPT_ADAM (weight decay as an L2 term), OPT_ADAMW (decoupled)
  // CLIP forms (dca_engine_set_clip): the averaged gradient is scaled to an L2 norm of at most max_norm
  float max_norm;         // > 0
  double* part;           // [OPT_PARTS] k_grad_sqnorm's partial sums of squares (device, owned by the caller), or null
  // ACC forms (dca_engine_set_accum): k_grad_accum sums acc_k steps' gradients into `acc`; the pass applies the mean
  float* acc;             // accumulated gradient, flat fp32 [FLAT_ALLOC] (the gradient buffer's layout), or null
  int acc_k;              // micro-steps per optimiser step (>= 1)
  float inv_k;            // fp32(1 / acc_k)
  // ---- everything above is set by the host (copied up to offsetof(OptDev, step)); below: device state ----
  int step;               // optimiser steps taken (device counter)
  unsigned ticket;        // workgroups that have finished reading `step` in the current launch
  double b1p, b2p;        // beta1^step, beta2^step: running products, multiplied once per Adam launch by the workgroup
                          // that advances `step`; the host sets them (adam_products) whenever it sets `step`
  double gnorm;           // CLIP forms: the last launch's gradient norm, before clipping
  unsigned n_clipped;     // CLIP forms: launches whose norm exceeded max_norm (the host resets it)
  int micro;              // ACC forms: micro-steps already summed into `acc` in the current window, in [0, acc_k)
  int apply;              // ACC forms: k_grad_accum's word to the kernels behind it: 1 on a window's last micro-step
  unsigned acc_ticket;    // ACC forms: workgroups of k_grad_accum that have finished reading `micro`
};
enum { OPT_SGD = 0, OPT_ADAM = 1, OPT_ADAMW = 2 };

// beta^step as the device forms it: `step` successive double multiplications (so a restored step gives the bits an
// uninterrupted run holds).
inline double adam_product(double beta, int step) {
  double b = 1.0;
  for (int i = 0; i < step && b != 0.0; ++i) b *= beta;
  return b;
}

// Enqueue k_apply_opt<bf, ema, clip> on `st`: one pass over the flat buffer [0, OFF_RS); ema: the form that also
// updates od->ema (which must then be set); clip: the form that scales the gradient by the coefficient it forms from
// od->part (launch_grad_sqnorm goes first on the same stream).  Returns the launch's hipError_t.
// acc: the form that does nothing but the CC4 copy unless od->apply is set (launch_grad_accum goes first on the same
// stream, and cx.grads points at od->acc).
hipError_t launch_apply_opt(bool bf, bool ema, bool clip, bool acc, const Ctx& cx, OptDev* od, hipStream_t st);
// The same for the Adam forms, k_apply_adam<bf, ema, decoupled, clip, acc> (od->v set, od->rule OPT_ADAM / OPT_ADAMW).
hipError_t launch_apply_adam(bool bf, bool ema, bool decoupled, bool clip, bool acc, const Ctx& cx, OptDev* od,
                             hipStream_t st);
// Enqueue k_grad_sqnorm: part[OPT_PARTS] <- the partial sums of squares of the averaged gradient in cx.grads.
hipError_t launch_grad_sqnorm(const Ctx& cx, double* part, hipStream_t st);
// Enqueue k_grad_accum: od->acc <- the window's running sum with cx.grads added (overwritten on the window's first
// micro-step, scaled by od->inv_k on its last), the CC4 tail copied; od->micro advances, od->apply says whether the
// window is complete.  cx.grads is only read.
hipError_t launch_grad_accum(const Ctx& cx, OptDev* od, hipStream_t st);

}  // namespace dca
