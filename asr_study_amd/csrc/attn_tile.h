// attn_tile.h -- the 64 x 64 tile pieces the attention kernels share (attention.hip,
// rel_attention.hip): a workgroup of 256 threads (16 x 16), tiles of 64 rows at a pitch of dh + 4
// floats in LDS ((dh + 4) / 4 is odd: the 16 lanes of a row group read 16-byte pieces of 16
// different rows without a bank conflict), a 64 x 64 score tile in registers, 4 x 4 per thread
// (rows 4 ty + i, columns tx + 16 j), which goes through LDS once (pitch 68) for the second
// product (64 x dh, 4 x dh / 16 per thread).
#pragma once
#include "vec4.h"

namespace {

constexpr int AT_TILE = 64;               // Bq = Bk
constexpr int AT_THREADS = 256;
constexpr int AT_PP = AT_TILE + 4;        // pitch of the probability tile
constexpr float AT_LOG2E = 1.4426950408889634f;
constexpr float AT_LN2 = 0.6931471805599453f;

__device__ __forceinline__ float at_max16(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, ASR_WAVE));
  return v;
}
__device__ __forceinline__ float at_sum16(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, ASR_WAVE);
  return v;
}

// rows [r0, r0 + 64) of one column block of a slab -> LDS tile (64, DH + 4); rows >= r_end: zeros
template <int DH>
__device__ __forceinline__ void at_load_tile(float* tile, const float* src, size_t row_stride,
                                             int r0, int r_end, int tid) {
  constexpr int V = DH / 4, DP = DH + 4;
#pragma unroll
  for (int e = tid; e < AT_TILE * V; e += AT_THREADS) {
    const int r = e / V, c = (e - r * V) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < r_end) v = ld4(src + (size_t)(r0 + r) * row_stride + c);
    st4(tile + r * DP + c, v);
  }
}

// acc[i][j] = A[4 ty + i] . B[tx + 16 j] over DH columns
template <int DH>
__device__ __forceinline__ void at_dot(const float* A, const float* B, int ty, int tx,
                                       float (&acc)[4][4]) {
  constexpr int DP = DH + 4;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
#pragma unroll 4
  for (int d = 0; d < DH; d += 4) {
    float4 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = ld4(A + (4 * ty + i) * DP + d);
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = ld4(B + (tx + 16 * j) * DP + d);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = fmaf(a[i].x, b[j].x, acc[i][j]);
        acc[i][j] = fmaf(a[i].y, b[j].y, acc[i][j]);
        acc[i][j] = fmaf(a[i].z, b[j].z, acc[i][j]);
        acc[i][j] = fmaf(a[i].w, b[j].w, acc[i][j]);
      }
  }
}

// o[i][jj] += sum_k P[4 ty + i][k] B[k][tx + 16 jj], k ascending
template <int DH>
__device__ __forceinline__ void at_acc(const float* P, const float* B, int ty, int tx,
                                       float (&o)[4][DH / 16]) {
  constexpr int DP = DH + 4, NJ = DH / 16;
#pragma unroll 2
  for (int k = 0; k < AT_TILE; k += 4) {
    float4 p[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = ld4(P + (4 * ty + i) * AT_PP + k);
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      const float b0 = B[(k + 0) * DP + tx + 16 * jj], b1 = B[(k + 1) * DP + tx + 16 * jj];
      const float b2 = B[(k + 2) * DP + tx + 16 * jj], b3 = B[(k + 3) * DP + tx + 16 * jj];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o[i][jj] = fmaf(p[i].x, b0, o[i][jj]);
        o[i][jj] = fmaf(p[i].y, b1, o[i][jj]);
        o[i][jj] = fmaf(p[i].z, b2, o[i][jj]);
        o[i][jj] = fmaf(p[i].w, b3, o[i][jj]);
      }
    }
  }
}

__device__ __forceinline__ void at_put_tile(float* P, const float (&s)[4][4], int ty, int tx) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) P[(4 * ty + i) * AT_PP + tx + 16 * j] = s[i][j];
}

// zeros into columns [c0, c0 + w) of rows [r0, min(r0 + 64, r_end)) of a slab (any w >= 0)
__device__ __forceinline__ void at_zero_cols(float* dst, size_t row_stride, int r0, int r_end,
                                             int c0, int w, int tid) {
  for (int e = tid; e < AT_TILE * w; e += AT_THREADS) {
    const int r = e / w, c = e - r * w;
    if (r0 + r < r_end) dst[(size_t)(r0 + r) * row_stride + c0 + c] = 0.f;
  }
}

__device__ __forceinline__ int at_len(const int* lens, int n, int T) {
  int len = lens ? lens[n] : T;
  // the engine refuses lengths outside 1 .. T on the host (Model._key_lens); a direct caller's
  // are clamped here, so that no length can index out of bounds
  return len < 1 ? 1 : (len > T ? T : len);
}

// THE WINDOW (K25), defined here once for attention.hip, rel_attention.hip and their plans.
// Three integers: chunk >= 1; left >= -1 frames (-1: unlimited); right >= 0 frames.  For query
// frame t let c0 = (t / chunk) * chunk.  Key u is visible to t iff lo(t) <= u < hi(t) and
// u < lens[n], with
//   hi(t) = c0 + chunk + right            lo(t) = left < 0 ? 0 : max(0, c0 - left)
// chunk 1, right 0 is the causal mask (a finite left: a sliding window); chunk 1, right R a
// symmetric window; chunk C chunk-wise attention with a look-ahead of chunk - 1 + right frames,
// which does not grow with depth.  lo and hi are non-decreasing in t, and lo(t + 1) <= c0(t) +
// chunk <= hi(t): the keys the queries qa .. qb see together are the ONE range [lo(qa), hi(qb)),
// which is what the tile ranges below rely on.  hi saturates at INT_MAX.
__host__ __device__ __forceinline__ bool at_win_ok(const asr_attn_window* w) {
  return w != nullptr && w->chunk >= 1 && w->left >= -1 && w->right >= 0;
}
__host__ __device__ __forceinline__ int at_win_lo(const asr_attn_window& w, int t) {
  const int c0 = t / w.chunk * w.chunk;
  return (w.left < 0 || c0 < w.left) ? 0 : c0 - w.left;
}
__host__ __device__ __forceinline__ int at_win_hi(const asr_attn_window& w, int t) {
  const long long hi = (long long)(t / w.chunk * w.chunk) + w.chunk + w.right;
  return hi > 0x7fffffffLL ? 0x7fffffff : (int)hi;
}
// The key tiles the query tile at q0 (queries q0 .. min(q0 + 63, T - 1)) visits: k0 = *kb,
// *kb + 64, ... while k0 < *ke -- those that meet [lo(q0), min(hi(last query), len)); none when
// *kb >= *ke (every row of the tile is then empty).
__host__ __device__ __forceinline__ void at_win_keys(const asr_attn_window& w, int q0, int T,
                                                     int len, int* kb, int* ke) {
  const int ql = q0 + AT_TILE - 1 < T ? q0 + AT_TILE - 1 : T - 1;
  const int hi = at_win_hi(w, ql);
  *kb = at_win_lo(w, q0) / AT_TILE * AT_TILE;
  *ke = hi < len ? hi : len;
}
// Whether the queries qa .. qb and the key tile at k0 hold a visible pair (the length aside):
// the test of the passes that own a key tile and walk query tiles.
__host__ __device__ __forceinline__ bool at_win_pair(const asr_attn_window& w, int qa, int qb,
                                                     int k0) {
  return at_win_lo(w, qa) <= k0 + AT_TILE - 1 && at_win_hi(w, qb) > k0;
}
// (query tile, key tile) pairs one (sample, head) of the forward launch visits, lens == NULL
inline long long at_win_tile_pairs(const asr_attn_window& w, int T) {
  long long pairs = 0;
  for (int q0 = 0; q0 < T; q0 += AT_TILE) {
    int kb, ke;
    at_win_keys(w, q0, T, T, &kb, &ke);
    if (ke > kb) pairs += (ke - kb + AT_TILE - 1) / AT_TILE;
  }
  return pairs;
}

bool at_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename K>
int at_allow_lds(K kernel, size_t bytes) {
  ASR_CHECK_HIP(hipFuncSetAttribute((const void*)kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return ASR_OK;
}

}  // namespace
