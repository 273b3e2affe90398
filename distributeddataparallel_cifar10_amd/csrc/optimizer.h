// Interface of the optimiser pass (optimizer.hip): the device-memory block of its hyper-parameters and the host
// launcher.  The pass is a translation unit (and so a code object) of its own inside the engine library: the code
// object of engine.hip -- the step kernels -- stays byte for byte what it is without the pass.
#pragma once
#include "common.h"

namespace dca {

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
  int step;               // optimiser steps taken (device counter)
  unsigned ticket;        // workgroups that have finished reading `step` in the current launch
};

// Enqueue k_apply_opt<bf, ema> on `st`: one pass over the flat buffer [0, OFF_RS); ema: the form that also updates
// od->ema (which must then be set).  Returns the launch's hipError_t.
hipError_t launch_apply_opt(bool bf, bool ema, const Ctx& cx, OptDev* od, hipStream_t st);

}  // namespace dca
