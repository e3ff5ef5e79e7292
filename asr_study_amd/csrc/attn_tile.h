// attn_tile.h -- the 64 x 64 tile pieces of the attention kernels (attn_core.h: the passes that
// attention.hip and rel_attention.hip instantiate; rel_attention.hip: its dpos pass), the window,
// the ring and the checks of a streaming call: a workgroup of 256 threads (16 x 16), tiles of 64
// rows at a pitch of dh + 4 floats in LDS ((dh + 4) / 4 is odd: the 16 lanes of a row group read
// 16-byte pieces of 16 different rows without a bank conflict), a 64 x 64 score tile in registers,
// 4 x 4 per thread (rows 4 ty + i, columns tx + 16 j), which goes through LDS once (pitch 68) for
// the second product (64 x dh, 4 x dh / 16 per thread).
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

// The running softmax of the forward kernels over one key tile: s holds the tile's scaled scores
// of rows 4 ty + i (a key that is not visible: -inf) and leaves as p = exp2(s - max); m, l are the
// rows' running maximum and sum, o their running output, rescaled by alpha.  GUARD (under a
// window): a row may have seen no key yet (m, mx both -inf), and exp2f(-inf - -inf) is NaN, so 0
// is subtracted then -- alpha = 0 scales sums that are 0, every p = exp2f(-inf) = 0, l stays 0.
// Without it the maximum is finite: key k0 of every tile is a valid one.
template <int NJ, bool GUARD>
__device__ __forceinline__ void at_softmax_tile(float (&s)[4][4], float (&m)[4], float (&l)[4],
                                                float (&o)[4][NJ]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float mx = asr_neg_inf();
#pragma unroll
    for (int j = 0; j < 4; ++j) mx = fmaxf(mx, s[i][j]);
    mx = fmaxf(m[i], at_max16(mx));
    float mref = mx;
    if constexpr (GUARD) mref = mx == asr_neg_inf() ? 0.f : mx;
    const float alpha = exp2f(m[i] - mref);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[i][j] = exp2f(s[i][j] - mref);
      sum += s[i][j];
    }
    l[i] = fmaf(l[i], alpha, at_sum16(sum));
    m[i] = mx;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) o[i][jj] *= alpha;
  }
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

// THE WINDOW (K25), defined here once for the kernels of attn_core.h and rel_attention.hip and
// for the plans.
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

// THE RING (K26), defined here once for the streaming forward of attn_core.h and its plan.  A ring
// is a slab (R, n_pad, ld): absolute frame u of the stream lives in ring row u % R.  R is a
// multiple of 64, so a 64-frame tile that starts at an absolute multiple of 64 is contiguous in
// the ring and at_load_tile reads it through a shifted base pointer.  A call states the absolute
// index t0 of its first new frame and their count Tq; the caller has put the new frames into the
// ring beforehand.  The first key tile the call walks starts at lo(t0) / 64 * 64, the last frame
// it holds is t0 + Tq - 1: the ring is valid for the call iff R >= at_ring_need.  Rows that hold
// frames below a query's lo are stale (older frames, or the zeros the owner filled the ring with):
// finite, and they meet p = exactly 0 only.
__host__ __device__ __forceinline__ long long at_ring_need(const asr_attn_window& w, int t0,
                                                           int Tq) {
  return (long long)t0 + Tq - at_win_lo(w, t0) / AT_TILE * AT_TILE;
}
// The smallest ring that is valid for EVERY t0 >= 0 and every count up to Tq: never more than
// left + chunk - 1 + Tq + 63 rounded up to 64 (t0 - lo(t0) <= left + chunk - 1, lo % 64 <= 63),
// less where chunk and left keep lo(t0) % 64 away from 63.  lo(t0) % 64 has a period of at most 64
// chunks once c0 >= left, and the last frame of a chunk is the worst t0 of that chunk.
inline int at_ring_rows(const asr_attn_window& w, int Tq) {
  long long need = 0;
  const long long chunks = (long long)w.left / w.chunk + AT_TILE + 2;
  for (long long m = 0; m < chunks; ++m) {
    const long long n = at_ring_need(w, (int)(m * w.chunk + w.chunk - 1), Tq);
    need = n > need ? n : need;
  }
  return (int)((need + AT_TILE - 1) / AT_TILE * AT_TILE);
}
// what a streaming call needs of its window and ring: a bounded left context, no right context
// (a key past the newest frame does not exist yet)
__host__ __device__ __forceinline__ bool at_stream_win_ok(const asr_attn_window* w) {
  return at_win_ok(w) && w->left >= 0 && w->right == 0 && w->chunk <= (1 << 20) &&
         w->left <= (1 << 20);
}

bool at_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// What is wrong with a streaming call (asr_attn_stream_fwd, asr_relattn_stream_fwd: rel, with
// dh <= max_dh), or nullptr: checked on the host before any device call.
inline const char* at_stream_bad(const asr_attn_stream_args* a, const asr_attn_window* w,
                                 int max_dh, bool rel) {
  if (!at_stream_win_ok(w)) return "bad window (chunk >= 1, left >= 0, right = 0)";
  if (a == nullptr || a->Tq < 1 || a->N < 1 || a->n_pad < a->N || a->n_pad > 65535)
    return "bad geometry (Tq >= 1, 1 <= N <= n_pad <= 65535)";
  if (a->heads < 1 || a->heads > 65535 || a->dh < 16 || a->dh > max_dh || (a->dh & 15))
    return "bad geometry (heads >= 1, dh a multiple of 16 within the kernel's range)";
  const long long D = (long long)a->heads * a->dh;
  if ((a->ld & 3) || a->ld < D || (a->ld_kv & 3) || a->ld_kv < 2 * D || (a->ld_out & 3) ||
      a->ld_out < D)
    return "bad geometry (ld >= heads dh, ld_kv >= 2 heads dh, ld_out >= heads dh, multiples of 4)";
  if (a->t0 < 0 || (long long)a->t0 + a->Tq > 0x7fffffffLL - 2 * AT_TILE - w->chunk)
    return "bad geometry (t0 >= 0, t0 + Tq below 2^31)";
  if (a->R < AT_TILE || (a->R % AT_TILE) || a->R < at_ring_need(*w, a->t0, a->Tq))
    return "bad ring (R a multiple of 64, R >= t0 + Tq - lo(t0) / 64 * 64)";
  if (!(a->scale > 0.f && a->scale < 1e30f)) return "bad scale";
  if (!a->q || !a->ring || !a->kv_len || !a->out || a->out == a->q)
    return "q, ring, kv_len and out are required";
  if (!at_aligned(a->q) || !at_aligned(a->ring) || !at_aligned(a->out))
    return "q, ring, out 16-byte aligned";
  if (rel) {
    if (a->P < (long long)w->left + w->chunk || (a->ld_pos & 3) || a->ld_pos < D ||
        (2LL * a->P - 1) * a->ld_pos > 0x7fffffffLL)
      return "bad table (P >= left + chunk rows each side, ld_pos >= heads dh, a multiple of 4)";
    if (!a->pos || !a->bias_u || !a->bias_v || !at_aligned(a->pos))
      return "pos (16-byte aligned), bias_u and bias_v are required";
  }
  return nullptr;
}

template <typename K>
int at_allow_lds(K kernel, size_t bytes) {
  ASR_CHECK_HIP(hipFuncSetAttribute((const void*)kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return ASR_OK;
}

}  // namespace
