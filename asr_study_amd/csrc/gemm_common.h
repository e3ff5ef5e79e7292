// What the three sources of the GEMM family share: gemm.hip (asr_gemm: the exact-fp32 kernel and
// the split-fp16 kernels that convert per tile), gemm_hl.hip (asr_gemm_hl: the kernels on packed
// planes) and pack.hip (asr_pack_hl, asr_absmax, asr_colsum).
#pragma once
#include "common.h"
#include <mutex>

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using hx8 = __attribute__((ext_vector_type(8))) _Float16;
using hx4 = __attribute__((ext_vector_type(4))) _Float16;
using u32x4g = __attribute__((ext_vector_type(4))) unsigned;

constexpr int HBK = 32;                      // K slab of every split-fp16 kernel
constexpr unsigned kOob = 0xFFFFFFF0u;       // buffer-load offset past any operand: reads zeros

// row % period; the period is n_pad (a multiple of 16, in practice a power of two)
__device__ __forceinline__ int mod_period(int row, int period) {
  return (period & (period - 1)) == 0 ? (row & (period - 1)) : row % period;
}

struct Epilogue {
  float* C; int ldc;
  float alpha, beta;
  const float* bias;
  const float* c_scale; int c_period, c_ld;
  float* partial;      // split-K: raw accumulators go here ([split][M][N])
  float clamp_hi;      // > 0 (segmented gemm_hlx only): C = min(max(., 0), clamp_hi)
};

// One element of the epilogue: (v alpha + bias) * mask + beta * old C, v the raw sum at (row, col);
// old points at the element of C (read only with beta != 0).  ep_apply4: four columns from col on.
__device__ __forceinline__ float ep_apply(const Epilogue ep, int row, int col, float v,
                                          const float* old) {
  v *= ep.alpha;
  if (ep.bias) v += ep.bias[col];
  if (ep.c_scale) v *= ep.c_scale[(size_t)mod_period(row, ep.c_period) * ep.c_ld + col];
  if (ep.beta != 0.f) v += ep.beta * *old;
  return v;
}
__device__ __forceinline__ float4 ep_apply4(const Epilogue ep, int row, int col, float4 v,
                                            const float4* old) {
  v.x *= ep.alpha; v.y *= ep.alpha; v.z *= ep.alpha; v.w *= ep.alpha;
  if (ep.bias) {
    v.x += ep.bias[col]; v.y += ep.bias[col + 1]; v.z += ep.bias[col + 2]; v.w += ep.bias[col + 3];
  }
  if (ep.c_scale) {
    const float* m = ep.c_scale + (size_t)mod_period(row, ep.c_period) * ep.c_ld + col;
    v.x *= m[0]; v.y *= m[1]; v.z *= m[2]; v.w *= m[3];
  }
  if (ep.beta != 0.f) {
    const float4 o = *old;
    v.x += ep.beta * o.x; v.y += ep.beta * o.y; v.z += ep.beta * o.z; v.w += ep.beta * o.w;
  }
  return v;
}

__device__ __forceinline__ float pow2_scale(const float* absmax) {
  // 2^(9 - e) with max = f * 2^e, f in [0.5, 1): max*scale in [2^8, 2^9)
  if (absmax == nullptr) return 1.f;
  const unsigned b = __float_as_uint(*absmax);
  int e = (int)((b >> 23) & 0xff) - 126;
  if ((b & 0x7fffffffu) == 0u) return 1.f;
  int k = 9 - e;
  k = k > 100 ? 100 : (k < -100 ? -100 : k);
  return __uint_as_float((unsigned)(127 + k) << 23);
}

// half index of hi[row][k] in interleaved (hi, lo) planes of ld reduction indices per row (the
// layout is described at the head of gemm_hl.hip); lo is 16 halfs further on
__device__ __forceinline__ size_t hl_index(int row, int k, int ld) {
  return (size_t)row * (2 * (size_t)ld) + (size_t)(k >> 4) * 32 + (k & 15);
}

// blockIdx.x -> (row tile, column tile, K split).  The dispatcher deals consecutive
// workgroup ids round-robin over the 8 XCDs (id % 8), each with its own 4 MB L2, so
// every XCD gets a CONTIGUOUS range of an ordering in which the ~64 workgroups it runs
// at a time form a compact (8 row tiles x 8 column tiles) block of one K split: their
// A / B panels are fetched into that L2 once and shared.
struct TileId { int tm, tn, z; };
__device__ __forceinline__ TileId tile_of_id(int id, int TM, int TN, int splits) {
  constexpr int kXcd = 8, GM = 8;
  const int total = TM * TN * splits;
  const int q = total / kXcd, r = total % kXcd;       // bijective for any total
  const int xcd = id % kXcd, idx = id / kXcd;
  const int g = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  const int tiles = TM * TN;
  TileId t;
  t.z = g / tiles;
  const int rem = g - t.z * tiles;
  const int band = rem / (GM * TN);                   // band of GM row tiles
  const int in_band = rem - band * (GM * TN);
  const int rows_here = (TM - band * GM) < GM ? (TM - band * GM) : GM;
  t.tm = band * GM + in_band % rows_here;
  t.tn = in_band / rows_here;
  return t;
}
__device__ __forceinline__ TileId tile_of_block(int TM, int TN, int splits) {
  return tile_of_id((int)blockIdx.x, TM, TN, splits);
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Dynamic-LDS "ballast" for the small helper kernels that run on the weight-gradient
// stream beside a BPTT kernel: a recurrent workgroup reserves 96 KB of its CU's 160 KB,
// so a helper asking for 80 KB can never be placed on the same CU and steal issue slots
// from its one-wave-per-SIMD critical path.
static inline size_t lds_ballast(const void* kernel) {
  const size_t bytes = 80 * 1024;
  (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  return bytes;
}

// ---- host plumbing of asr_gemm and asr_gemm_hl

// (asr_gemm_args and asr_gemm_hl_args name the epilogue's fields alike)
template <class Args>
static inline Epilogue make_epilogue(const Args* a) {
  Epilogue ep;
  ep.C = a->C; ep.ldc = a->ldc; ep.alpha = a->alpha; ep.beta = a->beta; ep.bias = a->bias;
  ep.c_scale = a->c_scale; ep.c_period = a->c_scale_period > 0 ? a->c_scale_period : 1;
  ep.c_ld = a->c_scale_ld; ep.partial = nullptr; ep.clamp_hi = 0.f;
  return ep;
}

// The K split of a launch: split_k ranges of *k_per_split indices, whole slabs each (vector loads
// along K need 4-aligned range starts), cut down to the ranges that have work.
static inline int split_plan(int K, int split_k, int slab, int* k_per_split) {
  int splits = split_k > 1 ? split_k : 1;
  int kps = (K + splits - 1) / splits;
  kps = (kps + slab - 1) / slab * slab;
  if (kps < slab) kps = slab;
  while (splits > 1 && (size_t)(splits - 1) * kps >= (size_t)K) --splits;
  *k_per_split = kps;
  return splits;
}

// A split launch writes its raw sums to the workspace ([split][rows][N]); ASR_OK if that fits.
static inline int splitk_workspace(const char* who, int splits, size_t rows, int N, void* workspace,
                                   size_t ws_bytes, Epilogue* ep) {
  if (splits <= 1) return ASR_OK;
  const size_t need = (size_t)splits * rows * N * sizeof(float);
  if (!workspace || ws_bytes < need) {
    asr_set_error("%s: split-K workspace %zu < %zu bytes", who, ws_bytes, need);
    return ASR_ERR_WORKSPACE;
  }
  ep->partial = reinterpret_cast<float*>(workspace);
  return ASR_OK;
}

// More than 64 KB of dynamic LDS has to be asked for, once per kernel AND device (the attribute
// belongs to the device's copy of the function).
static inline hipError_t set_dynamic_lds_once(const void* kernel, size_t bytes) {
  static std::mutex mu;
  static const void* done[16][16];
  static int n[16] = {0};
  int dev = 0;
  const bool keyed = hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 16;
  std::lock_guard<std::mutex> lock(mu);
  if (keyed)
    for (int i = 0; i < n[dev]; ++i)
      if (done[dev][i] == kernel) return hipSuccess;
  const hipError_t e =
      hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess && keyed && n[dev] < 16) done[dev][n[dev]++] = kernel;
  return e;
}

// The tail of a split launch (gemm.hip): sums the partials in a fixed order and applies the
// epilogue, on 16-byte quads where the layout allows it; the caller checks the launch.
void launch_splitk_reduce(const float* partial, int splits, int M, int N, Epilogue ep,
                          hipStream_t stream);
