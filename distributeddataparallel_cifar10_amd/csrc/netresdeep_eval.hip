// Eval-mode NetResDeep forward for CDNA4 (gfx950 / MI355X): ONE workgroup per image, persistent over a strided
// list of images, no communication between workgroups of any kind (so any grid size is legal and the results do not
// depend on it).  With running statistics BatchNorm is a fixed per-channel affine, so none of the step kernel's
// exchanges (BN partials, halo rows) exist here; what is shared with it is the operand machinery of pks_ops.h.
//
//   gather uint8 image -> normalise -> conv1 + bias + ReLU + 2x2 max-pool (VALU, 3.6 % of the FLOPs)
//   -> 10 x  x = relu(scale * conv(x) + shift) + x   (MFMA; x stays in fp32 registers, its bf16 records in LDS)
//   -> 2x2 max-pool -> fc1 + ReLU -> fc2 -> logits, argmax, cross-entropy     (per-image outputs, no atomics)
//
// The workgroup builds its operands from the fp32 master tensors once per launch (9,216 + 864 weights, BN scale /
// shift) and keeps them in LDS for every image it processes (the trunk B fragments in registers for an image's 10
// blocks).  The fc1 weight (256 KB fp32) does not fit beside them: it is read from L2 for every image (16-B loads,
// 256 B contiguous per 16-lane group).
//
// Precision P as in netresdeep_pks.hip: 0 = bf16 conv operands (activations and weights) and bf16 fc1 weight, fp32
// everything else; 1 = 3xbf16 trunk conv, fp32 conv1 and fc1.
//
// Element ownership (C layout of v_mfma_f32_16x16x32_bf16): 8 waves = (4-row group g) x (channel half h); thread
// (wave 4h + g, lane 16q + c) owns pixels (row 4g + r, col 4q + i), channel 16h + c, for r, i in 0..3 (16 values).
#include "pks_ops.h"

namespace dca {
namespace nrd_eval {

using pks::RB;

constexpr int NW = 8;          // waves per workgroup
constexpr int NTH = 64 * NW;   // threads per workgroup
static_assert(NTH == 512, "thread maps: 4 row groups x 2 channel halves; 768 input words = 512 + 256");

struct Args {
  const float *c1w, *c1b, *cw, *bnw, *bnb, *rm, *rv, *f1w, *f1b, *f2w, *f2b;
  float bn_eps;
  const uint8_t* data;  // [n_data][3][32][32]
  const int* labels;    // [n_data]
  int n_data;
  const int* indices;   // [n] (null: image k is data[k])
  int n;
  float* logits;        // [n][10] or null
  int* pred;            // [n]
  float* loss;          // [n]
};

// ---- LDS plan (bytes; every region 16-byte aligned) ---------------------------------------------------------
template <int P>
struct Plan {
  static constexpr int NP = P + 1;                      // precision planes: hi (+ lo)
  static constexpr int WT_PL = 288 * RB;                // trunk conv weight records [tap][co] x 32 ci
  static constexpr int O_WT = 0;
  static constexpr int XR_PL = 18 * 18 * RB;            // conv input records, rows -1..16, cols -1..16 (zero border)
  static constexpr int O_XR = O_WT + NP * WT_PL;
  static constexpr int IN_S = 36;                       // input row stride (floats): image col x at x + 1
  static constexpr int IN_CH = 34 * IN_S;               // rows -1..32
  static constexpr int O_IN = O_XR + NP * XR_PL;        // [3][34][IN_S] f32 normalised input (zero border)
  static constexpr int C1_S = 28;                       // conv1 weight row: 27 taps (ci*9 + kh*3 + kw) + bias
  static constexpr int O_C1 = O_IN + 3 * IN_CH * 4;     // [32][C1_S] f32
  static constexpr int O_BN = O_C1 + 32 * C1_S * 4;     // [32] scale | [32] shift
  static constexpr int O_PF = O_BN + 256;               // [2048] f32 pooled features (fc1 input)
  static constexpr int O_H = O_PF + 2048 * 4;           // [32] relu(fc1) | [16] logits
  static constexpr int TOTAL = O_H + 256;
};
static_assert(Plan<0>::TOTAL == 66144 && Plan<1>::TOTAL == 105312, "the documented LDS sizes");
static_assert(2 * Plan<0>::TOTAL <= 160 * 1024, "bf16: two workgroups per CU");
static_assert(Plan<1>::TOTAL <= 160 * 1024, "fp32: one workgroup per CU");
static_assert(Plan<0>::O_XR % 16 == 0 && Plan<0>::O_IN % 16 == 0 && Plan<0>::O_C1 % 16 == 0 && Plan<0>::O_PF % 16 == 0 &&
                  Plan<1>::O_XR % 16 == 0 && Plan<1>::O_IN % 16 == 0 && Plan<1>::O_C1 % 16 == 0 &&
                  Plan<1>::O_PF % 16 == 0 && (Plan<0>::IN_S * 4) % 16 == 0,
              "16-byte aligned regions and input rows");

__device__ __forceinline__ float bf_round(float v) { return __uint_as_float((unsigned)bfbits(v) << 16); }

// image index -> dataset row, clamped like sample_id: a bad index must never fault the device
__device__ __forceinline__ int image_id(const Args& a, int k) {
  const int id = a.indices ? a.indices[k] : k;
  return id < 0 ? 0 : (id >= a.n_data ? a.n_data - 1 : id);
}
// The 768 4-byte words of image `id` ([3][32][32] uint8) over the 512 threads: word t, and word 512 + t for t < 256
__device__ __forceinline__ uint2 image_words(const Args& a, int id, int t) {
  const unsigned* src = (const unsigned*)(a.data + (size_t)id * 3072);
  return uint2{src[t], t < 256 ? src[512 + t] : 0u};
}
// word w of the image, normalised, into XIN (P = 0: rounded to bf16, so the fp32 products below are the MFMA's)
template <int P>
__device__ __forceinline__ void stage_word(float* xin, int w, unsigned word) {
  using PL = Plan<P>;
  const int ch = w >> 8, row = (w >> 3) & 31, x0 = 4 * (w & 7);
  float* dst = xin + ch * PL::IN_CH + (row + 1) * PL::IN_S + x0 + 1;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const float v = norm_px((word >> (8 * b)) & 255u, ch);
    dst[b] = P == 0 ? bf_round(v) : v;
  }
}

// 3x3 conv of this wave's 4 output rows (image rows 4g .. 4g+3), output channels 16h .. 16h+15, on MFMA.  Each of the
// 6 x 3 A operands (input row 4g-1+ir, column shift kw) is read from LDS once and feeds up to three output rows, so
// LDS reads (18 per plane) stay below the MFMA time; the B fragments come from registers (bw hi, bwl lo for P = 1).
template <int P>
__device__ __forceinline__ void conv_rows4(const char* xr, const bf16x8 (&bw)[9], const bf16x8 (&bwl)[9], int g, int lane,
                                           f32x4 (&y)[4]) {
  using PL = Plan<P>;
  const int c = lane & 15, q = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) y[r] = z4();
#pragma unroll
  for (int ir = 0; ir < 6; ++ir) {
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int ao = pks::rec_chunk((4 * g + ir) * 18 + kw + c, q);
      const bf16x8 a = *(const bf16x8*)(xr + ao);
      bf16x8 al = a;
      if constexpr (P == 1) al = *(const bf16x8*)(xr + PL::XR_PL + ao);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kh = ir - r;
        if (kh < 0 || kh > 2) continue;
        y[r] = pks::mma3<P>(a, al, bw[kh * 3 + kw], P == 1 ? bwl[kh * 3 + kw] : bw[kh * 3 + kw], y[r]);
      }
    }
  }
}

template <int P>
__global__ void __launch_bounds__(NTH, P == 0 ? 4 : 2) k_nrd_eval(Args a) {
  using PL = Plan<P>;
  __shared__ __attribute__((aligned(16))) char lds[PL::TOTAL];
  char* const WT = lds + PL::O_WT;
  char* const XR = lds + PL::O_XR;
  float* const XIN = (float*)(lds + PL::O_IN);
  float* const C1 = (float*)(lds + PL::O_C1);
  float* const BN = (float*)(lds + PL::O_BN);
  float* const PF = (float*)(lds + PL::O_PF);
  float* const HB = (float*)(lds + PL::O_H);

  const int t = threadIdx.x, lane = t & 63, c = lane & 15, q = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6), g = wv & 3, h = wv >> 2;
  const int co = 16 * h + c;

  // ---- once per workgroup: operands from the fp32 master tensors, zeroed borders ------------------------------
  for (int i = t; i < (PL::O_C1 - PL::O_XR) / 16; i += NTH) ((uint4*)XR)[i] = uint4{0u, 0u, 0u, 0u};  // XR and XIN
  for (int i = t; i < 9216; i += NTH) {  // [co][ci][tap] -> record tap*32 + co, element ci
    const int o = i / 288, ci = (i / 9) & 31, tap = i % 9;
    pks::st1r<P>(WT, PL::WT_PL, tap * 32 + o, ci, a.cw[i]);
  }
  for (int i = t; i < 864; i += NTH) {
    const float w = a.c1w[i];
    C1[(i / 27) * PL::C1_S + i % 27] = P == 0 ? bf_round(w) : w;
  }
  if (t < 32) {
    C1[t * PL::C1_S + 27] = a.c1b[t];
    const float scale = a.bnw[t] * rsqrtf(a.rv[t] + a.bn_eps);
    BN[t] = scale;
    BN[32 + t] = a.bnb[t] - a.rm[t] * scale;
  }
  int img = blockIdx.x;
  uint2 words = img < a.n ? image_words(a, image_id(a, img), t) : uint2{0u, 0u};
  pks::lds_barrier();
  const float scale = BN[co], shift = BN[32 + co];

  for (; img < a.n; img += gridDim.x) {
    const int id = image_id(a, img);
    int label = a.labels[id];
    label = label < 0 ? 0 : (label > 9 ? 9 : label);
    // ---- input: this thread's words, normalised, into XIN (the previous image's readers passed >= 20 barriers)
    stage_word<P>(XIN, t, words.x);
    if (t < 256) stage_word<P>(XIN, 512 + t, words.y);
    pks::lds_barrier();
    // the next image's bytes travel while this one is computed
    if (img + (int)gridDim.x < a.n) words = image_words(a, image_id(a, img + gridDim.x), t);

    // ---- stem: conv1 + bias + ReLU + 2x2 max-pool; pooled rows 4g .. 4g+3, pooled cols 4q .. 4q+3, channel co
    float x[4][4];
    {
      float w1[27];
#pragma unroll
      for (int k = 0; k < 27; ++k) w1[k] = C1[co * PL::C1_S + k];
      const float bias = C1[co * PL::C1_S + 27];
#pragma unroll
      for (int pr = 0; pr < 4; ++pr) {
        const int R = 4 * g + pr;  // conv rows 2R, 2R+1 <- input rows 2R-1 .. 2R+2 = XIN rows 2R .. 2R+3
        float acc[2][8];
#pragma unroll
        for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
          for (int b = 0; b < 8; ++b) acc[r2][b] = 0.f;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
#pragma unroll
          for (int ir = 0; ir < 4; ++ir) {
            const float* src = XIN + ci * PL::IN_CH + (2 * R + ir) * PL::IN_S + 8 * q;  // image cols 8q-1 .. 8q+8
            const f32x4 u0 = *(const f32x4*)src, u1 = *(const f32x4*)(src + 4);
            const float2 u2 = *(const float2*)(src + 8);
            const float in[10] = {u0[0], u0[1], u0[2], u0[3], u1[0], u1[1], u1[2], u1[3], u2.x, u2.y};
#pragma unroll
            for (int r2 = 0; r2 < 2; ++r2) {
              const int kh = ir - r2;
              if (kh < 0 || kh > 2) continue;
#pragma unroll
              for (int kw = 0; kw < 3; ++kw) {
                const float w = w1[ci * 9 + kh * 3 + kw];
#pragma unroll
                for (int b = 0; b < 8; ++b) acc[r2][b] = fmaf(w, in[b + kw], acc[r2][b]);
              }
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float m = fmaxf(fmaxf(acc[0][2 * i], acc[0][2 * i + 1]), fmaxf(acc[1][2 * i], acc[1][2 * i + 1]));
          x[pr][i] = fmaxf(m + bias, 0.f);  // relu and + bias are monotone: pool first
        }
        __builtin_amdgcn_sched_barrier(0);  // one pooled row at a time: its 12 input rows are not hoisted across
      }
    }

    // ---- trunk: 10 applications of the one shared block ---------------------------------------------------
    // XR's last readers (block 9 of the previous image) are behind that block's second barrier.  The B
    // fragments stay in registers for the 10 blocks (re-read from WT per image: the stem needs the registers)
    bf16x8 bw[9], bwl[9];
    pks::load_bfrag(WT, h, lane, bw);
    if constexpr (P == 1) pks::load_bfrag(WT + PL::WT_PL, h, lane, bwl);
#pragma unroll 1
    for (int blk = 0; blk < NBLK; ++blk) {
      // the 16 + 18 swizzled record addresses are re-derived per block from an opaque copy of the lane id: kept live
      // from the kernel's start (loop-invariant) they cost the registers that put the bf16 kernel into scratch
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int cl = 16 * h + (ln & 15), ql = ln >> 4;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) pks::st1r<P>(XR, PL::XR_PL, (4 * g + r + 1) * 18 + 4 * ql + i + 1, cl, x[r][i]);
      pks::lds_barrier();
      f32x4 y[4];
      conv_rows4<P>(XR, bw, bwl, g, ln, y);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) x[r][i] += fmaxf(fmaf(scale, y[r][i], shift), 0.f);
      pks::lds_barrier();  // every wave has read XR
    }

    // ---- head: 2x2 max-pool -> fc1 + ReLU -> fc2 -> argmax, cross-entropy --------------------------------------
#pragma unroll
    for (int r2 = 0; r2 < 2; ++r2)
#pragma unroll
      for (int b = 0; b < 2; ++b)
        PF[co * 64 + (2 * g + r2) * 8 + 2 * q + b] = fmaxf(fmaxf(x[2 * r2][2 * b], x[2 * r2][2 * b + 1]),
                                                           fmaxf(x[2 * r2 + 1][2 * b], x[2 * r2 + 1][2 * b + 1]));
    pks::lds_barrier();
    {  // fc1: output j = t / 16, the 16 lanes of a row split the 2048 features in 16-B pieces (fc1 weight from L2)
      const int j = t >> 4, part = t & 15;
      const float* wrow = a.f1w + j * 2048 + 4 * part;
      float s = 0.f;
#pragma unroll 8
      for (int k = 0; k < 32; ++k) {
        f32x4 w = *(const f32x4*)(wrow + 64 * k);
        const f32x4 p = *(const f32x4*)(PF + 64 * k + 4 * part);
        if constexpr (P == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) w[e] = bf_round(w[e]);
        }
        s = fmaf(w[0], p[0], s);
        s = fmaf(w[1], p[1], s);
        s = fmaf(w[2], p[2], s);
        s = fmaf(w[3], p[3], s);
      }
      s = pks::xsum_row16(s);
      if (part == 0) HB[j] = fmaxf(s + a.f1b[j], 0.f);
    }
    pks::lds_barrier();
    if (wv == 0) {
      float* LG = HB + 32;
      if (lane < 10) {
        float s = a.f2b[lane];
#pragma unroll
        for (int j = 0; j < 32; ++j) s = fmaf(a.f2w[lane * 32 + j], HB[j], s);
        LG[lane] = s;
        if (a.logits) a.logits[(size_t)img * 10 + lane] = s;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave: its own LDS writes, in order
      if (lane == 0) {
        float m = LG[0];
        int am = 0;
#pragma unroll
        for (int k = 1; k < 10; ++k)
          if (LG[k] > m) {  // strict: ties keep the lowest index
            m = LG[k];
            am = k;
          }
        float s = 0.f;  // sum over k != argmax of exp(l_k - max): loss = (max - l_label) + log1p(s), no cancellation
#pragma unroll
        for (int k = 0; k < 10; ++k) s += k == am ? 0.f : expf(LG[k] - m);
        a.pred[img] = am;
        a.loss[img] = (m - LG[label]) + log1pf(s);
      }
    }
    // HB / LG are next written after the next image's barriers; wave 0 reaches them only after this point
  }
}

inline int default_workgroups(int P, int device) {
  int ncu = 0, per_cu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
  const void* f = P == 0 ? (const void*)k_nrd_eval<0> : (const void*)k_nrd_eval<1>;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, NTH, 0) != hipSuccess || per_cu <= 0) per_cu = 1;
  return ncu * per_cu;
}

}  // namespace nrd_eval
}  // namespace dca
