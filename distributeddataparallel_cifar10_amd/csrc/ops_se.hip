// Squeeze-and-excitation (Hu et al.) over NHWC bf16 activations u [N][P][C], P = H W pixels, C % 8 == 0: the per-image
// channel mean (squeeze), the gated residual join out = ReLU(u * g[n][c] + idt) with g = sigmoid(z), and their
// backward.  Every kernel is bound by its bytes (squeeze 1 x, scale 3 x, backward reduce 4 x, backward apply 3 x the
// activation), so the design is about touching each byte once with 16-byte accesses.  No matrix instruction fits:
// there is no K dimension (a per-channel sum over pixels and a per-channel scale), so the math is fp32 VALU.
//
// Work split (one for all four kernels).  The unit of channels is the 16-byte chunk of 8.  A workgroup of 256 threads
//   owns one image and a slab of CH = 8, 16 or 32 chunks (64 / 128 / 256 channels); thread t owns chunk t % CH and
//   pixel lane t / CH of the L = 256 / CH lanes and walks pixels lane, lane + L, ... in increasing order.  A wave
//   instruction therefore reads 64 / CH pixels x 16 CH contiguous bytes (128, 256 or 512: whole cache lines).  CH
//   follows P so that the lanes do not outnumber the pixels: 8 x 32 lanes for the wide maps (56 x 56, 28 x 28), 16 x 16
//   up to 256 pixels (14 x 14), 32 x 8 up to 64 (7 x 7: an eighth of the lane-iterations idle, where 16 or 32 lanes would idle a quarter), and never more
//   chunks than the channels fill twice.  One workgroup covers all of P: at batch 256 the four SE-ResNet-50 shapes are
//   1024 (56 x 56 x 256) or 2048 workgroups.  Workgroups are numbered slab-fastest, so the slabs that share a pixel's
//   bytes run at the same time.  The walk is unrolled by four pixels so that a thread keeps four (reduce: twelve)
//   16-byte loads in flight.
// Reductions (squeeze, backward reduce).  A thread keeps 8 fp32 sums over its pixels; the lanes of a chunk are summed
//   through LDS in lane order (dw_chunk_sum of ops_dwconv.hip: 8 segments of consecutive lanes, then the 8 segment
//   sums).  No atomics, one fixed order: a step repeats bit for bit.
// The gate.  g = 1 / (1 + exp(-z)) in fp32 from the fp32 logits z [N][C], computed by each thread once for its 8
//   channels (per image and chunk, not per pixel); there is no sigmoid pass and g is never stored.
// Backward.  With m = [out > 0] (read from the saved output: no mask tensor):
//   k_se_bwd_reduce  one pass over dout, out, u: writes didt = dout m (exact in bf16) and reduces t = sum_p dout m u,
//                    dz = t g (1 - g).
//   k_se_bwd_apply   du = dout m g + ds / P, ds [N][C] being the gradient of the squeezed mean (known only after the gate
//                    MLP's backward): the only write of du, so the gate path and the pooling path never meet in an add.
#pragma once
#include "ops_dwconv.hip"

namespace dca {
namespace ops {

constexpr int SE_NT = 256;

template <int LC>
struct SePlan {  // the thread's place in workgroup blockIdx.x of image-major, slab-fastest numbering
  static constexpr int CH = 1 << LC, L = SE_NT >> LC;
  int n, lane, cb;  // image; pixel lane; first channel of the thread's chunk
  bool active;      // the chunk exists (the last slab may be ragged)
  __device__ __forceinline__ SePlan(int C) {
    const int nslab = (C + 8 * CH - 1) / (8 * CH);
    n = blockIdx.x / nslab;
    lane = threadIdx.x >> LC;
    cb = 8 * (CH * (blockIdx.x % nslab) + (threadIdx.x & (CH - 1)));
    active = cb < C;
  }
  // 16-byte piece index of pixel p (pieces of 8 channels; N P C < 2^31 elements)
  __device__ __forceinline__ long at(int p, int P, int C) const { return (((long)n * P + p) * C + cb) >> 3; }
};

// g[8] of the thread's chunk from the logits z [N][C]
__device__ __forceinline__ void se_gate(float (&g)[8], const float* __restrict__ z, long o) {
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] = 1.f / (1.f + expf(-z[o + j]));
}
__device__ __forceinline__ void se_vec8(float (&v)[8], const void* __restrict__ p, long o, int is_bf16) {  // [N][C] operand
  if (is_bf16) {
    unpack8(*(const uint4*)((const bf16_t*)p + o), v);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ((const float*)p)[o + j];
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_se_squeeze: s[n][c] = (1 / P) sum_p u[n][p][c], written as bf16 (RNE; the operand of the following GEMM) or fp32.
// grid: N x ceil(C / (8 CH)); requirements as se_rule (ops_api.hip).
// ---------------------------------------------------------------------------------------------------------
template <int LC>
__global__ void __launch_bounds__(SE_NT) k_se_squeeze(const bf16_t* __restrict__ u, void* __restrict__ s, int P, int C,
                                                      int out_bf16) {
  using T = SePlan<LC>;
  __shared__ float buf[SE_NT * 8 + 64 * T::CH];
  const T t(C);
  const uint4* __restrict__ u4 = (const uint4*)u;
  const long step = (long)T::L * (C >> 3);
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, f[8];
  if (t.active) {
    int p = t.lane;
    long o = t.at(p, P, C);
    for (; p + 3 * T::L < P; p += 4 * T::L, o += 4 * step) {
      const uint4 v0 = u4[o], v1 = u4[o + step], v2 = u4[o + 2 * step], v3 = u4[o + 3 * step];
      const uint4 v[4] = {v0, v1, v2, v3};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unpack8(v[i], f);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += f[j];
      }
    }
    for (; p < P; p += T::L, o += step) {
      unpack8(u4[o], f);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += f[j];
    }
  }
  const float r = dw_chunk_sum<LC>(buf, a);  // thread tid < 8 CH: channel tid of the slab
  const int c = t.cb - 8 * (threadIdx.x & (T::CH - 1)) + threadIdx.x;
  if ((int)threadIdx.x < 8 * T::CH && c < C) {
    const float m = r / (float)P;
    if (out_bf16) ((bf16_t*)s)[(long)t.n * C + c] = f2bf_rne(m);
    else ((float*)s)[(long)t.n * C + c] = m;
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_se_scale_fwd: out = bf16_rne(max(u * g[n][c] + idt, 0)) (one fp32 FMA), g from z.  Grid as k_se_squeeze.
// ---------------------------------------------------------------------------------------------------------
template <int LC>
__global__ void __launch_bounds__(SE_NT) k_se_scale_fwd(const bf16_t* __restrict__ u, const float* __restrict__ z,
                                                        const bf16_t* __restrict__ idt, bf16_t* __restrict__ out,
                                                        int P, int C) {
  using T = SePlan<LC>;
  const T t(C);
  if (!t.active) return;
  const uint4* __restrict__ u4 = (const uint4*)u;
  const uint4* __restrict__ i4 = (const uint4*)idt;
  uint4* __restrict__ o4 = (uint4*)out;
  const long step = (long)T::L * (C >> 3);
  float g[8], fu[8], fi[8];
  se_gate(g, z, (long)t.n * C + t.cb);
  int p = t.lane;
  long o = t.at(p, P, C);
  for (; p + 3 * T::L < P; p += 4 * T::L, o += 4 * step) {
    const uint4 a[4] = {u4[o], u4[o + step], u4[o + 2 * step], u4[o + 3 * step]};
    const uint4 b[4] = {i4[o], i4[o + step], i4[o + 2 * step], i4[o + 3 * step]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unpack8(a[i], fu);
      unpack8(b[i], fi);
#pragma unroll
      for (int j = 0; j < 8; ++j) fu[j] = fmaxf(fmaf(fu[j], g[j], fi[j]), 0.f);
      o4[o + i * step] = pack8(fu);
    }
  }
  for (; p < P; p += T::L, o += step) {
    unpack8(u4[o], fu);
    unpack8(i4[o], fi);
#pragma unroll
    for (int j = 0; j < 8; ++j) fu[j] = fmaxf(fmaf(fu[j], g[j], fi[j]), 0.f);
    o4[o] = pack8(fu);
  }
}

// dout * [out > 0] of 8 channels: a select, so the bf16 bits of dout pass through unchanged
__device__ __forceinline__ void se_masked(float (&d)[8], const uint4 vd, const uint4 vo) {
  float fo[8];
  unpack8(vd, d);
  unpack8(vo, fo);
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = fo[j] > 0.f ? d[j] : 0.f;
}

// ---------------------------------------------------------------------------------------------------------
// k_se_bwd_reduce: didt = dout * [out > 0] (bf16, exact) and dz[n][c] = g (1 - g) sum_p didt * u (fp32; the products
// are exact, the sum in the fixed order of the skeleton).  Grid as k_se_squeeze.
// ---------------------------------------------------------------------------------------------------------
template <int LC>
__global__ void __launch_bounds__(SE_NT) k_se_bwd_reduce(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ out,
                                                         const bf16_t* __restrict__ u, const float* __restrict__ z,
                                                         bf16_t* __restrict__ didt, float* __restrict__ dz, int P,
                                                         int C) {
  using T = SePlan<LC>;
  __shared__ float buf[SE_NT * 8 + 64 * T::CH];
  const T t(C);
  const uint4* __restrict__ d4 = (const uint4*)dout;
  const uint4* __restrict__ o4 = (const uint4*)out;
  const uint4* __restrict__ u4 = (const uint4*)u;
  uint4* __restrict__ i4 = (uint4*)didt;
  const long step = (long)T::L * (C >> 3);
  float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, d[8], fu[8];
  if (t.active) {
    int p = t.lane;
    long o = t.at(p, P, C);
    for (; p + 3 * T::L < P; p += 4 * T::L, o += 4 * step) {
      const uint4 vd[4] = {d4[o], d4[o + step], d4[o + 2 * step], d4[o + 3 * step]};
      const uint4 vo[4] = {o4[o], o4[o + step], o4[o + 2 * step], o4[o + 3 * step]};
      const uint4 vu[4] = {u4[o], u4[o + step], u4[o + 2 * step], u4[o + 3 * step]};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        se_masked(d, vd[i], vo[i]);
        unpack8(vu[i], fu);
        i4[o + i * step] = pack8(d);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = fmaf(d[j], fu[j], a[j]);
      }
    }
    for (; p < P; p += T::L, o += step) {
      se_masked(d, d4[o], o4[o]);
      unpack8(u4[o], fu);
      i4[o] = pack8(d);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] = fmaf(d[j], fu[j], a[j]);
    }
  }
  const float r = dw_chunk_sum<LC>(buf, a);
  const int c = t.cb - 8 * (threadIdx.x & (T::CH - 1)) + threadIdx.x;
  if ((int)threadIdx.x < 8 * T::CH && c < C) {
    const long o = (long)t.n * C + c;
    const float g = 1.f / (1.f + expf(-z[o]));
    dz[o] = r * g * (1.f - g);
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_se_bwd_apply: du = bf16_rne(dout * [out > 0] * g[n][c] + ds[n][c] / P) (one fp32 FMA), ds bf16 or fp32.  Grid as
// k_se_squeeze.
// ---------------------------------------------------------------------------------------------------------
template <int LC>
__global__ void __launch_bounds__(SE_NT) k_se_bwd_apply(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ out,
                                                        const float* __restrict__ z, const void* __restrict__ ds,
                                                        bf16_t* __restrict__ du, int P, int C, int ds_bf16) {
  using T = SePlan<LC>;
  const T t(C);
  if (!t.active) return;
  const uint4* __restrict__ d4 = (const uint4*)dout;
  const uint4* __restrict__ o4 = (const uint4*)out;
  uint4* __restrict__ x4 = (uint4*)du;
  const long step = (long)T::L * (C >> 3);
  float g[8], m[8], d[8];
  se_gate(g, z, (long)t.n * C + t.cb);
  se_vec8(m, ds, (long)t.n * C + t.cb, ds_bf16);
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] = m[j] / (float)P;
  int p = t.lane;
  long o = t.at(p, P, C);
  for (; p + 3 * T::L < P; p += 4 * T::L, o += 4 * step) {
    const uint4 vd[4] = {d4[o], d4[o + step], d4[o + 2 * step], d4[o + 3 * step]};
    const uint4 vo[4] = {o4[o], o4[o + step], o4[o + 2 * step], o4[o + 3 * step]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      se_masked(d, vd[i], vo[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = fmaf(d[j], g[j], m[j]);
      x4[o + i * step] = pack8(d);
    }
  }
  for (; p < P; p += T::L, o += step) {
    se_masked(d, d4[o], o4[o]);
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = fmaf(d[j], g[j], m[j]);
    x4[o] = pack8(d);
  }
}

}  // namespace ops
}  // namespace dca
