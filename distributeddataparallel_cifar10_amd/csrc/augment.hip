// On-device training augmentation of the uint8 dataset: random crop (zero padding `pad`) followed by a horizontal
// flip, torchvision's RandomCrop(32, padding = pad) + RandomHorizontalFlip() on the image before Normalize.  One
// bandwidth-bound pass rewrites the rows an epoch will read: dst[id] = T(src[id]) for every listed id, so the step
// kernels (which read the dataset through one pointer) need no change -- a translation unit and code object of its
// own, like optimizer.hip.
//
// The draw is stateless and keyed by the sample id (data/augment.py is the definition, this file matches it bit for
// bit):
//   k  = fmix32(fmix32(id * 0x9E3779B9 + seed) ^ (epoch * 0x85EBCA77))
//   dx = mulhi(fmix32(k + 1), 2 pad + 1), dy = mulhi(fmix32(k + 2), 2 pad + 1), f = fmix32(k + 3) >> 31
//   out[c][y][x] = P[c][y + dy][(f ? 31 - x : x) + dx]          P: the image zero-padded by `pad` on every side
//
// Work shape: one wave per channel of one image (1 KiB): lane = (row y, half h), one 16-byte output chunk per lane.
// dx, dy and f are wave-uniform (the hash runs on the scalar side).  Every global access is an aligned 16-byte load
// or store: a lane loads its 32-byte source row as two uint4 and builds its chunk in registers -- the row, extended by
// 8 zero bytes on both sides, shifted by dx - pad bytes; a flipped chunk is the byte-reversed chunk of the other
// half.  Rows that fall into the padding store zeros and load nothing.  No LDS, no byte-granular access.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

namespace dca {

constexpr int AUG_IMAGE = 3 * 32 * 32;        // bytes per image
constexpr int AUG_IPB = 2;                    // images per workgroup
constexpr int AUG_NT = AUG_IPB * 3 * 64;      // 384 threads: one wave per (image, channel)
constexpr int AUG_MAX_GRID = 256 * 5;         // 5 workgroups of 384 threads per CU; more images: grid-stride
constexpr int AUG_PAD_MAX = 8;

__host__ __device__ inline uint32_t aug_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

struct AugDraw {
  int dy, dx, f;
};

__host__ __device__ inline AugDraw aug_draw(uint32_t id, uint32_t seed, uint32_t epoch, int pad, int flip) {
  uint32_t k = aug_fmix32(id * 0x9E3779B9u + seed);
  k = aug_fmix32(k ^ (epoch * 0x85EBCA77u));
  const uint64_t span = 2 * (uint64_t)pad + 1;
  AugDraw d;
  d.dx = (int)((aug_fmix32(k + 1) * span) >> 32);
  d.dy = (int)((aug_fmix32(k + 2) * span) >> 32);
  d.f = flip ? (int)(aug_fmix32(k + 3) >> 31) : 0;
  return d;
}

// low dword of {hi, lo} >> 8 b, b in [0, 3]
__host__ __device__ inline uint32_t aug_align(uint32_t hi, uint32_t lo, uint32_t b) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * b));
}

// The 16 output bytes of half `h` (x = 16 h .. 16 h + 15) of one row: out[x] = S[(f ? 31 - x : x) + s], S the source
// row (r0 = bytes 0..15, r1 = bytes 16..31) and zero outside it; s = dx - pad in [-8, 8].  `s` and `f` are
// wave-uniform; only `h` differs between lanes.
__host__ __device__ inline uint4 aug_chunk(uint4 r0, uint4 r1, int h, int s, int f) {
  // E = 8 zero bytes, S, 20 zero bytes (13 dwords); W = E from byte 16 hh on, hh the half read (the other one when
  // flipped); the unflipped chunk is W[s + 8 .. s + 24)
  const bool hi = (h ^ f) != 0;
  uint32_t w[9];
  w[0] = hi ? r0.z : 0u;
  w[1] = hi ? r0.w : 0u;
  w[2] = hi ? r1.x : r0.x;
  w[3] = hi ? r1.y : r0.y;
  w[4] = hi ? r1.z : r0.z;
  w[5] = hi ? r1.w : r0.w;
  w[6] = hi ? 0u : r1.x;
  w[7] = hi ? 0u : r1.y;
  w[8] = hi ? 0u : r1.z;
  const uint32_t o = (uint32_t)(s + 8), b = o & 3u;
  uint4 c;
#define DCA_AUG_CASE(Q)                                                               \
  case Q:                                                                             \
    c = make_uint4(aug_align(w[Q + 1], w[Q], b), aug_align(w[Q + 2], w[Q + 1], b),    \
                   aug_align(w[Q + 3], w[Q + 2], b), aug_align(w[Q + 4], w[Q + 3], b)); \
    break;
  switch (o >> 2) {  // wave-uniform: a scalar branch, constant register indices in every arm
    DCA_AUG_CASE(0)
    DCA_AUG_CASE(1)
    DCA_AUG_CASE(2)
    DCA_AUG_CASE(3)
    default:  // o = 16 (b = 0): W[16 .. 32)
      c = make_uint4(w[4], w[5], w[6], w[7]);
      break;
  }
#undef DCA_AUG_CASE
  if (f) c = make_uint4(__builtin_bswap32(c.w), __builtin_bswap32(c.z), __builtin_bswap32(c.y), __builtin_bswap32(c.x));
  return c;
}

__global__ void __launch_bounds__(AUG_NT) k_augment_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const int* __restrict__ ids, int n, int n_rows, uint32_t seed,
                                                       uint32_t epoch, int pad, int flip) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int slot = wave / 3, ch = wave - 3 * slot;
  const int lane = threadIdx.x & 63, y = lane >> 1, h = lane & 1;
  for (int i = blockIdx.x * AUG_IPB + slot; i < n; i += gridDim.x * AUG_IPB) {
    const int id = __builtin_amdgcn_readfirstlane(ids ? ids[i] : i);
    if ((unsigned)id >= (unsigned)n_rows) continue;  // never write outside dst (the host API checks its ids)
    const AugDraw d = aug_draw((uint32_t)id, seed, epoch, pad, flip);
    const size_t plane = (size_t)id * AUG_IMAGE + (size_t)ch * 1024;
    const int sy = y + d.dy - pad;
    uint4 out = make_uint4(0u, 0u, 0u, 0u);
    if ((unsigned)sy < 32u) {
      const uint4* row = (const uint4*)(src + plane + sy * 32);
      out = aug_chunk(row[0], row[1], h, d.dx - pad, d.f);
    }
    *(uint4*)(dst + plane + y * 32 + h * 16) = out;
  }
}

}  // namespace dca

namespace {
thread_local std::string g_aug_err;

int aug_fail(const std::string& why) {
  g_aug_err = "dca_augment_u8: " + why;
  return -1;
}
}  // namespace

extern "C" {

// The reason of the last -1 of dca_augment_u8 on this thread (the pass is independent of the engine, whose own error
// string lives in engine.hip).
const char* dca_augment_last_error() { return g_aug_err.c_str(); }

// dst[id] = T(src[id]) for the `n` ids in `ids` (device int32; null: ids 0 .. n - 1), both datasets uint8
// [n_rows][3][32][32], enqueued on `stream`.  Duplicate ids write identical bytes.  Returns 0, or -1 with the reason
// in dca_augment_last_error() and nothing launched.
int dca_augment_u8(const uint8_t* src, uint8_t* dst, const int* ids, int n, int n_rows, unsigned seed, unsigned epoch,
                   int pad, int flip, hipStream_t stream) {
  if (!src || !dst) return aug_fail("null dataset pointer");
  if (((uintptr_t)src | (uintptr_t)dst) & 15) return aug_fail("dataset pointers must be 16-byte aligned");
  if ((uintptr_t)ids & 3) return aug_fail("misaligned id list");
  if (n_rows <= 0) return aug_fail("n_rows must be positive");
  if (n < 0 || (!ids && n > n_rows)) return aug_fail("n must be in [0, n_rows] without an id list, >= 0 with one");
  if (pad < 0 || pad > dca::AUG_PAD_MAX) return aug_fail("pad must be in [0, 8]");
  const size_t bytes = (size_t)n_rows * dca::AUG_IMAGE;
  const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst;
  if (s < d + bytes && d < s + bytes) return aug_fail("src and dst overlap");
  if (n == 0) return 0;
  const int blocks = (n + dca::AUG_IPB - 1) / dca::AUG_IPB;
  const int grid = blocks < dca::AUG_MAX_GRID ? blocks : dca::AUG_MAX_GRID;
  hipLaunchKernelGGL(dca::k_augment_u8, dim3(grid), dim3(dca::AUG_NT), 0, stream, src, dst, ids, n, n_rows, seed, epoch,
                     pad, flip ? 1 : 0);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return aug_fail(std::string("launch: ") + hipGetErrorString(e));
  return 0;
}

}  // extern "C"
