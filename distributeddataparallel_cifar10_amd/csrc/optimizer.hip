// The optimiser pass of the NetResDeep engine: SGD with momentum and weight decay on a per-step learning rate, as
// one kernel over the flat parameter buffer.  It runs after the step's gradient has been reduced (and, world size
// > 1, all-reduced) into cx.grads WITHOUT being applied: the sliced engine's mode 1, the multi-kernel engine's
// fuse_sgd = 0, k_xgmi_ar_sgd with sgd = 0 (engine.hip, "split" step form).
//
// Arithmetic per element, three fused multiply-adds in this order (g: the summed gradient, p: the parameter):
//   d   = fmaf(wd, p, g * inv_ws)      averaged gradient + weight decay
//   buf = fmaf(mu, buf, d)             momentum buffer (starts at zero: the first update equals d)
//   p   = fmaf(-lr, buf, p)
// i.e. torch.optim.SGD(momentum = mu, weight_decay = wd), dampening 0, decay on all nine tensors.  With mu = wd = 0
// and inv_ws = 1 it is the fused step's fmaf(-lr, g, p) exactly (d = g, buf = g).
//
// The hyper-parameters live in device memory (OptDev), not in the kernel arguments, so a captured step graph picks
// up a new learning-rate table, momentum or decay without re-capture.  The learning rate of a launch is
// lr_table[min(step, n_table - 1)] (lr_const without a table); `step` is the pass's own device counter (the
// engine's step_count is cleared at every epoch's loss read) and advances once per launch, by the workgroup that
// takes the last ticket -- every workgroup reads `step` before it takes its ticket.
//
// The EMA form (k_apply_opt<BF, true>; dca_engine_set_ema) also keeps an exponential moving average of the model in a
// second flat buffer of the gradient buffer's layout: with the fresh p in registers, e = fmaf(d, e - p, p) over
// [0, OFF_RS), and the same update of cx.rm | cx.rv (the module's running statistics as the step left them) into
// [OFF_RS, OFF_RS + 64) by the 64 threads that write the CC4 base.  d = ema_decay, or with warm-up
// min(ema_decay, (1 + step) / (10 + step)), computed by thread 0 from the `step` it reads anyway.  The form without
// EMA compiles to what the pass was before the EMA form existed.
// The Adam forms (k_apply_adam<BF, EMA, DECOUPLED>; dca_engine_set_adam) are kernels of their own further down: the
// SGD forms do not change with them.
// The CLIP forms (k_apply_opt<BF, EMA, true>, k_apply_adam<BF, EMA, DECOUPLED, true>; dca_engine_set_clip) clip the
// averaged gradient to a global L2 norm first, torch.nn.utils.clip_grad_norm_ before optimizer.step():
//   x    = fp32(g * inv_ws)
//   N    = sqrt(sum (double)x * (double)x)   over the 76,074 parameter elements (the CC4 tail and the two pad floats
//                                            behind fc2.bias are left out by index)
//   c    = (float)(max_norm / (N + 1e-6))    in double, rounded once
//   coef = c < 1 ? c : (c != c ? c : 1)      torch's clamp(max = 1): a NaN stays a NaN
//   x'   = x * coef                          one more fp32 multiplication (never contracted into what follows);
//                                            coef == 1 leaves x bit for bit
// and x' takes the place of g * inv_ws above and in the Adam arithmetic below (weight decay is added after clipping).
// Two launches in stream order: k_grad_sqnorm, the pass's launch shape, writes one double partial per workgroup
// (every (double)x * (double)x is exact, the partial is a fixed-order wave + LDS reduction: no floating-point
// atomics); thread 0 of every workgroup of the CLIP form then sums the OPT_NB partials in index order and shares coef
// through LDS, and thread 0 of workgroup 0 records od->gnorm = N and counts the clipped steps in od->n_clipped.  No
// grid-wide wait inside one kernel: ranks that share a device must never spin on each other's workgroups.  The forms
// without CLIP compile to what they were before it existed.
// A translation unit of its own (see optimizer.h); derive_param comes from netresdeep_kernels.hip.
#include "netresdeep_kernels.hip"
#include "optimizer.h"

namespace dca {

static_assert(OFF_RS % 4 == 0, "the parameter range must be float4 granular");
static_assert(OPT_NB * NT >= OPT_V4 && OPT_NB == OPT_PARTS, "one float4 per thread, one partial per workgroup");

// a * b rounded to fp32 on its own: never contracted with an addition that uses it
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// Thread 0 of a CLIP form: the norm from the partials (index order), the coefficient; workgroup 0 records both.
__device__ __forceinline__ float clip_coef(OptDev* od) {
  const double* part = od->part;
  double s = 0.;
#pragma unroll
  for (int i = 0; i < OPT_NB; ++i) s += part[i];
  const double n = __builtin_sqrt(s);
  const float c = (float)((double)od->max_norm / (n + 1e-6));
  if (blockIdx.x == 0) {
    od->gnorm = n;
    if (c < 1.f) od->n_clipped = od->n_clipped + 1u;
  }
  return c < 1.f ? c : (c != c ? c : 1.f);
}

// Head of an ACC form: whether k_grad_accum, in front of this launch, completed a window (od->apply, read by thread 0
// and shared through LDS).  If not, the workgroup only installs the CC4 base from the accumulated buffer's tail (the
// latest micro-step's, cx.grads being od->acc here) and the caller returns: no sweep, no EMA, no ticket, no counter.
__device__ __forceinline__ bool acc_window_complete(const Ctx& cx, const OptDev* od, int t, int v) {
  __shared__ int s_apply;
  if (t == 0) s_apply = od->apply;
  __syncthreads();
  if (s_apply) return true;
  if (cx.ws > 1 && v < 64) cx.rs_base[v] = cx.grads[OFF_RS + v];
  return false;
}

template <bool BF, bool EMA, bool CLIP, bool ACC>
__global__ void __launch_bounds__(NT) k_apply_opt(Ctx cx, OptDev* od) {
  __shared__ float s_lr;
  __shared__ int s_step;
  __shared__ float s_ema;  // (EMA form only: unused, and so not allocated, in the other)
  __shared__ float s_coef; // (CLIP form only)
  const int t = threadIdx.x, v = blockIdx.x * NT + t;
  if constexpr (ACC) {
    if (!acc_window_complete(cx, od, t, v)) return;
  }
  if (t == 0) {
    const int st = __hip_atomic_load(&od->step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int n = od->n_table;
    s_step = st;
    s_lr = n > 0 ? od->lr_table[st < n - 1 ? (st < 0 ? 0 : st) : n - 1] : od->lr_const;
    if constexpr (EMA) {
      float d = od->ema_decay;
      if (od->ema_warmup) {
        const float k = (float)(st < 0 ? 0 : st);
        d = fminf(d, (1.f + k) / (10.f + k));
      }
      s_ema = d;
    }
    if constexpr (CLIP) s_coef = clip_coef(od);
  }
  const float mu = od->mu, wd = od->wd;
  float* mbuf = od->buf;
  float* ebuf = nullptr;
  if constexpr (EMA) ebuf = od->ema;
  __syncthreads();
  const float lr = s_lr;
  float coef = 1.f;
  if constexpr (CLIP) coef = s_coef;
  if (v < OPT_V4) {
    const int e0 = 4 * v;
    const f32x4 g = *(const f32x4*)(cx.grads + e0);
    f32x4 p = *(const f32x4*)(cx.params + e0);
    f32x4 m = *(const f32x4*)(mbuf + e0);
    f32x4 a;
    if constexpr (EMA) a = *(const f32x4*)(ebuf + e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float x = g[k] * cx.inv_ws;
      if constexpr (CLIP) x = mul_rn(x, coef);
      const float d = __builtin_fmaf(wd, p[k], x);
      m[k] = __builtin_fmaf(mu, m[k], d);
      p[k] = __builtin_fmaf(-lr, m[k], p[k]);
    }
    *(f32x4*)(mbuf + e0) = m;
    *(f32x4*)(cx.params + e0) = p;
    if constexpr (EMA) {
      const float dk = s_ema;
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = __builtin_fmaf(dk, a[k] - p[k], p[k]);
      *(f32x4*)(ebuf + e0) = a;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) derive_param<BF>(cx, e0 + k, p[k]);
  }
  // CC4: rank 0's running statistics (the tail of the all-reduced buffer) become every rank's base
  if (cx.ws > 1 && v < 64) cx.rs_base[v] = cx.grads[OFF_RS + v];
  if constexpr (EMA) {  // the averaged running statistics: rm | rv into the layout's CC4 tail, nothing beyond it
    if (v < 64) {
      float* er = ebuf + OFF_RS + v;
      const float s = v < 32 ? cx.rm[v] : cx.rv[v - 32];
      *er = __builtin_fmaf(s_ema, *er - s, s);
    }
  }
  if (t == 0) {  // the last workgroup to arrive advances the step (all have read it: their tickets are taken after)
    const unsigned prev = __hip_atomic_fetch_add(&od->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store(&od->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int st = s_step;
      __hip_atomic_store(&od->step, st < 0x7fffffff ? st + 1 : st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// The Adam forms of the pass (dca_engine_set_adam): torch.optim.Adam (DECOUPLED false: weight decay as an L2 term of
// the gradient) and AdamW (true: decay applied to the parameter), amsgrad off.  The same sweep, launch shape, learning
// rate, step counter, derived copies, CC4 copy and EMA update as k_apply_opt; od->buf is the first moment m and od->v
// the second.  Per element, fp32 with IEEE sqrt and division (t = step + 1):
//   g' = g * inv_ws                    (Adam: g' = fmaf(wd, p, g * inv_ws))
//   p0 = p                             (AdamW: p0 = fmaf(-(lr * wd), p, p))
//   m  = fmaf(omb1, g' - m, m)         omb1 = (float)(1 - beta1)
//   v  = fmaf(beta2f, v, (omb2 * g') * g')
//   p  = fmaf(-ss, m / fmaf(sqrtf(v), c2, eps), p0)
// with ss = lr / (1 - beta1^t) and c2 = 1 / sqrt(1 - beta2^t) formed in double by thread 0 from the running products
// od->b1p = beta1^step, od->b2p = beta2^step (no pow: one multiplication each) and shared as floats.  The workgroup
// that advances `step` also stores the new products.  The pads between tensors (g = p = m = v = 0) stay exactly 0:
// m / (0 + eps) = 0.
template <bool BF, bool EMA, bool DECOUPLED, bool CLIP, bool ACC>
__global__ void __launch_bounds__(NT) k_apply_adam(Ctx cx, OptDev* od) {
  __shared__ float s_lr, s_ss, s_c2;
  __shared__ float s_ema;  // (EMA form only)
  __shared__ float s_coef; // (CLIP form only)
  const int t = threadIdx.x, v = blockIdx.x * NT + t;
  if constexpr (ACC) {
    if (!acc_window_complete(cx, od, t, v)) return;
  }
  int st0 = 0;             // thread 0: the step and the products of this launch (t = step + 1)
  double b1t = 0., b2t = 0.;
  if (t == 0) {
    const int st = __hip_atomic_load(&od->step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int n = od->n_table;
    st0 = st;
    const float lr = n > 0 ? od->lr_table[st < n - 1 ? (st < 0 ? 0 : st) : n - 1] : od->lr_const;
    b1t = __hip_atomic_load(&od->b1p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * od->beta1;
    b2t = __hip_atomic_load(&od->b2p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * od->beta2;
    s_lr = lr;
    s_ss = (float)((double)lr / (1.0 - b1t));
    s_c2 = (float)(1.0 / __builtin_sqrt(1.0 - b2t));
    if constexpr (EMA) {
      float d = od->ema_decay;
      if (od->ema_warmup) {
        const float k = (float)(st < 0 ? 0 : st);
        d = fminf(d, (1.f + k) / (10.f + k));
      }
      s_ema = d;
    }
    if constexpr (CLIP) s_coef = clip_coef(od);
  }
  const float wd = od->wd, omb1 = od->omb1, omb2 = od->omb2, beta2 = od->beta2f, eps = od->eps;
  float* mbuf = od->buf;
  float* vbuf = od->v;
  float* ebuf = nullptr;
  if constexpr (EMA) ebuf = od->ema;
  __syncthreads();
  const float ss = s_ss, c2 = s_c2;
  float coef = 1.f;
  if constexpr (CLIP) coef = s_coef;
  if (v < OPT_V4) {
    const int e0 = 4 * v;
    const f32x4 g = *(const f32x4*)(cx.grads + e0);
    f32x4 p = *(const f32x4*)(cx.params + e0);
    f32x4 m = *(const f32x4*)(mbuf + e0);
    f32x4 s = *(const f32x4*)(vbuf + e0);
    f32x4 a;
    if constexpr (EMA) a = *(const f32x4*)(ebuf + e0);
    float lw = 0.f;
    if constexpr (DECOUPLED) lw = s_lr * wd;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gg = g[k] * cx.inv_ws;
      if constexpr (CLIP) gg = mul_rn(gg, coef);
      float p0 = p[k];
      if constexpr (DECOUPLED) p0 = __builtin_fmaf(-lw, p0, p0);
      else gg = __builtin_fmaf(wd, p0, gg);
      m[k] = __builtin_fmaf(omb1, gg - m[k], m[k]);
      s[k] = __builtin_fmaf(beta2, s[k], (omb2 * gg) * gg);
      p[k] = __builtin_fmaf(-ss, m[k] / __builtin_fmaf(__builtin_sqrtf(s[k]), c2, eps), p0);
    }
    *(f32x4*)(mbuf + e0) = m;
    *(f32x4*)(vbuf + e0) = s;
    *(f32x4*)(cx.params + e0) = p;
    if constexpr (EMA) {
      const float dk = s_ema;
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = __builtin_fmaf(dk, a[k] - p[k], p[k]);
      *(f32x4*)(ebuf + e0) = a;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) derive_param<BF>(cx, e0 + k, p[k]);
  }
  // CC4: rank 0's running statistics (the tail of the all-reduced buffer) become every rank's base
  if (cx.ws > 1 && v < 64) cx.rs_base[v] = cx.grads[OFF_RS + v];
  if constexpr (EMA) {  // the averaged running statistics, as in k_apply_opt
    if (v < 64) {
      float* er = ebuf + OFF_RS + v;
      const float r = v < 32 ? cx.rm[v] : cx.rv[v - 32];
      *er = __builtin_fmaf(s_ema, *er - r, r);
    }
  }
  if (t == 0) {  // the last workgroup to arrive advances the step and the products (all have read them)
    const unsigned prev = __hip_atomic_fetch_add(&od->ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store(&od->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (st0 < 0x7fffffff) {
        __hip_atomic_store(&od->b1p, b1t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&od->b2p, b2t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&od->step, st0 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

// The launchers name the forms without CLIP first, in the order they always had, and the CLIP forms and k_grad_sqnorm
// behind them: the compiler keeps that order in the code object, so the forms without CLIP stay where they were.  The
// ACC forms and k_grad_accum follow behind those, at the end of the file, for the same reason.
typedef void (*OptKernel)(Ctx, OptDev*);
static OptKernel adam_clip_kernel(bool bf, bool ema, bool decoupled);
static OptKernel opt_clip_kernel(bool bf, bool ema);
static OptKernel adam_acc_kernel(bool bf, bool ema, bool decoupled, bool clip);
static OptKernel opt_acc_kernel(bool bf, bool ema, bool clip);

hipError_t launch_apply_adam(bool bf, bool ema, bool decoupled, bool clip, bool acc, const Ctx& cx, OptDev* od,
                             hipStream_t st) {
  OptKernel k = nullptr;
#define DCA_ADAM(B, E, D) if (bf == B && ema == E && decoupled == D) k = k_apply_adam<B, E, D, false, false>
  DCA_ADAM(false, false, false); DCA_ADAM(false, false, true); DCA_ADAM(false, true, false); DCA_ADAM(false, true, true);
  DCA_ADAM(true, false, false); DCA_ADAM(true, false, true); DCA_ADAM(true, true, false); DCA_ADAM(true, true, true);
#undef DCA_ADAM
  if (clip) k = adam_clip_kernel(bf, ema, decoupled);
  if (acc) k = adam_acc_kernel(bf, ema, decoupled, clip);
  hipLaunchKernelGGL(k, dim3(OPT_NB), dim3(NT), 0, st, cx, od);
  return hipGetLastError();
}

hipError_t launch_apply_opt(bool bf, bool ema, bool clip, bool acc, const Ctx& cx, OptDev* od, hipStream_t st) {
  OptKernel k = bf ? k_apply_opt<true, false, false, false> : k_apply_opt<false, false, false, false>;
  if (ema) k = bf ? k_apply_opt<true, true, false, false> : k_apply_opt<false, true, false, false>;
  if (clip) k = opt_clip_kernel(bf, ema);
  if (acc) k = opt_acc_kernel(bf, ema, clip);
  hipLaunchKernelGGL(k, dim3(OPT_NB), dim3(NT), 0, st, cx, od);
  return hipGetLastError();
}

static OptKernel adam_clip_kernel(bool bf, bool ema, bool decoupled) {
  OptKernel k = nullptr;
#define DCA_ADAM(B, E, D) if (bf == B && ema == E && decoupled == D) k = k_apply_adam<B, E, D, true, false>
  DCA_ADAM(false, false, false); DCA_ADAM(false, false, true); DCA_ADAM(false, true, false); DCA_ADAM(false, true, true);
  DCA_ADAM(true, false, false); DCA_ADAM(true, false, true); DCA_ADAM(true, true, false); DCA_ADAM(true, true, true);
#undef DCA_ADAM
  return k;
}

static OptKernel opt_clip_kernel(bool bf, bool ema) {
  if (ema) return bf ? k_apply_opt<true, true, true, false> : k_apply_opt<false, true, true, false>;
  return bf ? k_apply_opt<true, false, true, false> : k_apply_opt<false, false, true, false>;
}

// The squared L2 norm of the averaged gradient x = fp32(g * inv_ws) over the parameter elements of cx.grads, as
// OPT_NB double partials: part[b] is workgroup b's sum, lanes combined by a butterfly within each wave and the four
// waves in order through LDS -- the same bits on every launch.
constexpr int OPT_PAD0 = OFF_FC2B + 10;  // 65898, 65899: the two pad floats behind fc2.bias
// (A template only so that the compiler emits it where it is first named, behind the kernels that were here before.)
template <int = 0>
__global__ void __launch_bounds__(NT) k_grad_sqnorm(Ctx cx, double* __restrict__ part) {
  __shared__ double s_w[NT / 64];
  const int t = threadIdx.x, v = blockIdx.x * NT + t;
  double a = 0.;
  if (v < OPT_V4) {
    const int e0 = 4 * v;
    const f32x4 g = *(const f32x4*)(cx.grads + e0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x = g[k] * cx.inv_ws;
      const double d = (double)x;
      if (e0 + k != OPT_PAD0 && e0 + k != OPT_PAD0 + 1) a += d * d;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
  if ((t & 63) == 0) s_w[t >> 6] = a;
  __syncthreads();
  if (t == 0) part[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

hipError_t launch_grad_sqnorm(const Ctx& cx, double* part, hipStream_t st) {
  hipLaunchKernelGGL(k_grad_sqnorm<>, dim3(OPT_NB), dim3(NT), 0, st, cx, part);
  return hipGetLastError();
}

// The ACC forms (k_apply_opt<BF, EMA, CLIP, true>, k_apply_adam<BF, EMA, DECOUPLED, CLIP, true>; dca_engine_set_accum):
// gradient accumulation over od->acc_k micro-steps.  k_grad_accum runs in front of k_grad_sqnorm and the pass on every
// micro-step and keeps the window's sum in od->acc, per element in fp32 and in this order:
//   acc = g_1;  acc = acc + g_k (k = 2 .. K);  on the K-th: G = mul_rn(acc, inv_k), inv_k = fp32(1 / K)
// -- the first micro-step of a window overwrites, so nothing of the window before (or of a poisoned buffer) survives.
// k_grad_sqnorm and the pass are then launched with a Ctx whose `grads` is od->acc, so G takes the gradient's place in
// everything downstream; on the other micro-steps the pass's ACC form returns after its CC4 copy (acc_window_complete).
// The window phase od->micro and K live in device memory: a captured step graph is the same for every phase.
static OptKernel adam_acc_kernel(bool bf, bool ema, bool decoupled, bool clip) {
  OptKernel k = nullptr;
#define DCA_ADAM(B, E, D)                                         \
  if (bf == B && ema == E && decoupled == D)                      \
  k = clip ? k_apply_adam<B, E, D, true, true> : k_apply_adam<B, E, D, false, true>
  DCA_ADAM(false, false, false); DCA_ADAM(false, false, true); DCA_ADAM(false, true, false); DCA_ADAM(false, true, true);
  DCA_ADAM(true, false, false); DCA_ADAM(true, false, true); DCA_ADAM(true, true, false); DCA_ADAM(true, true, true);
#undef DCA_ADAM
  return k;
}

static OptKernel opt_acc_kernel(bool bf, bool ema, bool clip) {
  OptKernel k = nullptr;
#define DCA_OPT(B, E, C) if (bf == B && ema == E && clip == C) k = k_apply_opt<B, E, C, true>
  DCA_OPT(false, false, false); DCA_OPT(false, false, true); DCA_OPT(false, true, false); DCA_OPT(false, true, true);
  DCA_OPT(true, false, false); DCA_OPT(true, false, true); DCA_OPT(true, true, false); DCA_OPT(true, true, true);
#undef DCA_OPT
  return k;
}

// One float4 per thread over [0, OFF_RS), the pass's launch shape; thread 0 of each workgroup reads the phase and K and
// shares them through LDS.  The CC4 tail [OFF_RS, OFF_RS + 64) -- rank 0's running statistics, not a gradient -- is
// copied on every micro-step, never summed.  cx.grads is only read.  The workgroup that takes the last ticket advances
// the phase (every workgroup has read it: the tickets are taken after) and tells the kernels behind this one whether
// the window is complete.  No floating-point atomics, no grid-wide wait.
// (A template only so that the compiler emits it where it is first named, behind the kernels that were here before.)
template <int = 0>
__global__ void __launch_bounds__(NT) k_grad_accum(Ctx cx, OptDev* od) {
  __shared__ int s_micro, s_k;
  __shared__ float s_inv;
  const int t = threadIdx.x, v = blockIdx.x * NT + t;
  if (t == 0) {
    s_micro = __hip_atomic_load(&od->micro, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_k = od->acc_k;
    s_inv = od->inv_k;
  }
  float* acc = od->acc;
  __syncthreads();
  const int micro = s_micro;
  const bool last = micro >= s_k - 1;
  if (v < OPT_V4) {
    const int e0 = 4 * v;
    f32x4 a = *(const f32x4*)(cx.grads + e0);
    if (micro > 0) {
      const f32x4 s = *(const f32x4*)(acc + e0);
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = s[k] + a[k];
    }
    if (last) {
      const float inv = s_inv;
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = mul_rn(a[k], inv);
    }
    *(f32x4*)(acc + e0) = a;
  }
  if (v < 64) acc[OFF_RS + v] = cx.grads[OFF_RS + v];
  if (t == 0) {
    const unsigned prev = __hip_atomic_fetch_add(&od->acc_ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store(&od->acc_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&od->micro, last ? 0 : micro + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&od->apply, last ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

hipError_t launch_grad_accum(const Ctx& cx, OptDev* od, hipStream_t st) {
  hipLaunchKernelGGL(k_grad_accum<>, dim3(OPT_NB), dim3(NT), 0, st, cx, od);
  return hipGetLastError();
}

}  // namespace dca
