// ROI-align over a channels-last bf16 feature map (apps/ppe.py ResNet101ROI.roi_align is the definition): one sample
// per bin, align_corners = False, clamped at the border.  For a box (b, x1, y1, x2, y2) in input pixels, k bins and
// feature stride s, bin column j (rows alike) samples the feature map at
//
//   xs = x1 + (x2 - x1) * ((j + 0.5) / k),   ix = clamp(xs / s - 0.5, 0, w - 1),   x0 = floor(ix),   fx = ix - x0
//
// with weight 1 - fx on pixel x0 and fx on pixel min(x0 + 1, w - 1) (fx is 0 whenever that index was clamped), and
// out[n, i, j, :] is the 2 x 2 blend.  Every product above is rounded to fp32 on its own, in this order, so for a
// power-of-two s and k and boxes on a dyadic lattice the coordinates and weights are exact.
//
// No input value moves an index outside its tensor: the batch index and the coordinates are clamped as floats (NaN
// goes to the lower bound) and again as integers after the conversion.
//
// Forward  k_roi_align_fwd: a workgroup owns (box, slab of 256 channels).  2k lanes compute the box's 2k x and 2k y
//   taps once into LDS; then lane = (bin of 8, 16-byte channel chunk of 32): four 16-byte loads, the blend in fp32,
//   one 16-byte store per bin.
// Backward k_roi_align_bwd: the gather form.  A workgroup owns (image, slab of 64 channels), a lane owns up to ROI_IT
//   (pixel, 16-byte channel chunk) items of a tile of 32 * ROI_IT pixels.  It walks the box table in index order; for
//   each box of its image it builds the separable dense tables WY[k][h], WX[k][w] (the weight of bin row i on pixel
//   row py, ...) in LDS, and every lane adds sum_i sum_j WY[i][py] WX[j][px] dout[n, i, j, chunk] into its fp32
//   registers, skipping zero weights.  Every pixel of the image is written exactly once (zeros where no box reaches
//   it): no atomics, no memset, no second pass, and a summation order -- boxes ascending, then i, then j -- that does
//   not depend on the grid or on timing.
#pragma once
#include "ops_nn.hip"

namespace dca {
namespace ops {

constexpr int ROI_KMAX = 8;    // bins per side
// Feature rows / columns (the LDS tables of the backward).  The backward holds a tile of 128 pixels in registers and
// walks the box table, rebuilding the tables, once per tile: once at the application's 8 x 10, up to 32 times at
// 64 x 64, where a pixel tile in the grid would be the better split.
constexpr int ROI_HWMAX = 64;
constexpr int ROI_IT = 4;      // backward: items per lane and pixel tile

struct RoiGeom {
  int B, h, w, C;  // feature map
  int N, k;        // boxes, bins per side
  float stride;
};

// fp32 -> index in [0, hi]: clamped as a float first (NaN and -inf go to 0, +inf to hi), and again after the conversion
__device__ __forceinline__ int roi_index(float f, int hi) {
  const int i = (int)fminf(fmaxf(f, 0.f), (float)hi);
  return min(max(i, 0), hi);
}

// The two taps of bin j of k along one axis of a box side [lo, hi]: pixels i0 / i1 (of `dim`) with weights 1 - f / f
__device__ __forceinline__ void roi_tap(float lo, float hi, int j, int k, float stride, int dim, int& i0, int& i1,
                                        float& f) {
#pragma clang fp contract(off)
  const float t = ((float)j + 0.5f) / (float)k;
  const float xs = lo + (hi - lo) * t;
  const float ix = fminf(fmaxf(xs / stride - 0.5f, 0.f), (float)(dim - 1));  // NaN -> 0
  i0 = roi_index(floorf(ix), dim - 1);
  f = ix - (float)i0;
  i1 = min(i0 + 1, dim - 1);
}

// Both kernels are built without the packed fp32 instructions (what -Xclang -target-feature -Xclang -packed-fp32-ops
// does for a whole file; an attribute here, so that the rest of the library compiles as before).  They move bytes, not
// flops, so packed math buys nothing, and its even-aligned register pairs cost registers: with it the compiler reports
// 48 VGPRs for the forward and 91 VGPRs, occupancy 5 for the backward; without it 43, and 71 at occupancy 7.  The
// results are the same either way (fma and mul round alike in both forms).
#define ROI_KERNEL __global__ __attribute__((target("no-packed-fp32-ops"))) void __launch_bounds__(256)

// grid (N, ceil(C / 256)), 256 threads
ROI_KERNEL k_roi_align_fwd(const bf16_t* __restrict__ feat, const float* __restrict__ boxes,
                           bf16_t* __restrict__ out, RoiGeom g) {
  __shared__ int s_i0[2][ROI_KMAX], s_i1[2][ROI_KMAX];  // [0]: x taps, [1]: y taps
  __shared__ float s_f[2][ROI_KMAX];
  const int n = blockIdx.x, tid = threadIdx.x, k = g.k;
  const float* bx = boxes + 5l * n;
  if (tid < 2 * k) {
    const int ax = tid >= k, j = tid - ax * k;
    roi_tap(bx[1 + ax], bx[3 + ax], j, k, g.stride, ax ? g.h : g.w, s_i0[ax][j], s_i1[ax][j], s_f[ax][j]);
  }
  __syncthreads();
  const int c = (blockIdx.y * 32 + (tid & 31)) * 8;
  if (c >= g.C) return;
  const bf16_t* img = feat + (long)roi_index(bx[0], g.B - 1) * g.h * g.w * g.C + c;
  for (int bin = tid >> 5; bin < k * k; bin += 8) {
    const int i = bin / k, j = bin - i * k;
    const float fy = s_f[1][i], fx = s_f[0][j];
    const long r0 = (long)s_i0[1][i] * g.w, r1 = (long)s_i1[1][i] * g.w;
    const int x0 = s_i0[0][j], x1 = s_i1[0][j];
    float a[8], b[8], cc[8], d[8], o[8];
    unpack8(*(const uint4*)(img + (r0 + x0) * g.C), a);
    unpack8(*(const uint4*)(img + (r0 + x1) * g.C), b);
    unpack8(*(const uint4*)(img + (r1 + x0) * g.C), cc);
    unpack8(*(const uint4*)(img + (r1 + x1) * g.C), d);
    const float w00 = (1.f - fy) * (1.f - fx), w01 = (1.f - fy) * fx, w10 = fy * (1.f - fx), w11 = fy * fx;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = fmaf(w11, d[e], fmaf(w10, cc[e], fmaf(w01, b[e], w00 * a[e])));
    *(uint4*)(out + ((long)n * k * k + bin) * g.C + c) = pack8(o);
  }
}

// grid (ceil(C / 64), B), 256 threads
ROI_KERNEL k_roi_align_bwd(const bf16_t* __restrict__ dout, const float* __restrict__ boxes,
                           bf16_t* __restrict__ dfeat, RoiGeom g) {
  __shared__ float WY[ROI_KMAX][ROI_HWMAX], WX[ROI_KMAX][ROI_HWMAX];
  const int b = blockIdx.y, tid = threadIdx.x, k = g.k, hw = g.h * g.w;
  const int c = (blockIdx.x * 8 + (tid & 7)) * 8;
  const bool lane_on = c < g.C;
  for (int tile = 0; tile < hw; tile += 32 * ROI_IT) {
    float acc[ROI_IT][8];
    int py[ROI_IT], px[ROI_IT];  // py < 0: no pixel
#pragma unroll
    for (int m = 0; m < ROI_IT; ++m) {
      const int p = tile + m * 32 + (tid >> 3);
      py[m] = p < hw && lane_on ? p / g.w : -1;
      px[m] = p - (p / g.w) * g.w;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[m][e] = 0.f;
    }
    for (int n = 0; n < g.N; ++n) {
      const float* bx = boxes + 5l * n;
      if (roi_index(bx[0], g.B - 1) != b) continue;  // uniform over the workgroup
      __syncthreads();  // the previous box's tables are no longer read
      for (int t = tid; t < k * (g.h + g.w); t += 256) {
        const int ax = t >= k * g.w, u = t - ax * k * g.w, dim = ax ? g.h : g.w;
        const int j = u / dim, q = u - j * dim;
        int i0, i1;
        float f;
        roi_tap(bx[1 + ax], bx[3 + ax], j, k, g.stride, dim, i0, i1, f);
        (ax ? WY : WX)[j][q] = (q == i0 ? 1.f - f : 0.f) + (q == i1 ? f : 0.f);
      }
      __syncthreads();
      const bf16_t* dn = dout + (long)n * k * k * g.C + c;
#pragma unroll
      for (int m = 0; m < ROI_IT; ++m) {
        if (py[m] < 0) continue;
        for (int i = 0; i < k; ++i) {
          const float wy = WY[i][py[m]];
          if (wy == 0.f) continue;
          for (int j = 0; j < k; ++j) {
            const float wgt = wy * WX[j][px[m]];
            if (wgt == 0.f) continue;
            float d[8];
            unpack8(*(const uint4*)(dn + (long)(i * k + j) * g.C), d);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[m][e] = fmaf(wgt, d[e], acc[m][e]);
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < ROI_IT; ++m)
      if (py[m] >= 0) *(uint4*)(dfeat + ((long)b * hw + py[m] * g.w + px[m]) * g.C + c) = pack8(acc[m]);
  }
}

#undef ROI_KERNEL

}  // namespace ops
}  // namespace dca
