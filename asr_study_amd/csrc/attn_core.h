// attn_core.h -- the attention passes, each written ONCE for the plain form (K21, attention.hip),
// the relative form (K24, rel_attention.hip) and the streaming forms (K26) of both: the forward
// pass, backward pass 1 (D and dQ) and backward pass 2 (dK, dV) as kernel templates on
//   DH      the head size;
//   WIN     under the window of attn_tile.h (K25); without it w is not read;
//   REL     with the relative term: the staged band of the position table, the two biases;
//   STREAM  (forward only, implies WIN) the queries of one chunk against THE RING of attn_tile.h;
//   CROSS   (plain form only) queries and keys of two sequences: Tq query rows against Tk keys, the
//           keys and their gradients in slabs of their own, and a query-row mask (qlens);
// and the host path they share: the geometry, the dispatch over dh, the launchers, the plan.
// Every difference between the forms is an `if constexpr`: an instantiation holds the code of its
// own form only (no ring modulo in a whole-utterance kernel; no band, no cP, not the barrier that
// protects G and the plain LDS layout in a plain one).  The running softmax, the visibility
// select, the order of every sum and the epilogues exist once, so a streamed row equals the
// whole-utterance row, and a windowed kernel whose window hides nothing the unwindowed one, bit
// for bit BY CONSTRUCTION: they are the same source lines.  The tile pieces are attn_tile.h's.
#pragma once
#include <type_traits>

#include "attn_tile.h"

namespace {

constexpr int AT_MAX_DH = 128;
constexpr int RA_MAX_DH = 64;             // the relative family: see rel_attention.hip
constexpr int RA_SMALL = 384;             // floats: cP / cK [128] | Ls [64] | Ds [64] | two vectors [128]

#define AT_WIN_TEXT "chunk >= 1, left >= -1 (-1: unlimited), right >= 0"

// One call's geometry.  The QUERY SOURCE is a slab (T, n_pad, ld) whose row 0 is the absolute frame
// t0; the KEY SOURCE a slab of rows ld_kv floats per sample apart, [K | V] in D columns each, in
// which the absolute frame u lives in row u (whole utterance: the K block of qkv, ld_kv = ld, t0 =
// 0) or in row u % R (the ring).  The position table has 2 P - 1 rows, row r + P - 1 the relative
// index r (whole utterance: P = T).
// CROSS: T counts the queries, Tk the keys (every other form has T of both and never reads Tk);
// the key source is a slab (Tk, n_pad, ld_kv) of its own, and so is its gradient.
struct AtGeo {
  int T, N, n_pad, heads, ld, ld_out, ld_pos;
  float c2;         // scale * log2(e)
  float scale;
  int ld_kv, R, t0, P;
  int Tk;
};

// CROSS: the valid query rows of sample n, qlens[n] clamped to 0 .. T (T without qlens).  A row at
// or past it is a padding query: out = lse = exactly 0, and it adds exactly 0 to every gradient
// (K25's rule for a row with no visible key), by selects on the row index.
__device__ __forceinline__ int at_qlen(const int* qlens, int n, int T) {
  const int len = qlens ? qlens[n] : T;
  return len < 0 ? 0 : (len > T ? T : len);
}

// rows [r0, r0 + 64) of a column block -> LDS tile (64, DH + 4), plus the vector `add` (LDS, DH
// floats, or nullptr); rows outside [0, r_end) are zeros (r0 may be negative)
template <int DH>
__device__ __forceinline__ void ra_load_rows(float* tile, const float* src, size_t row_stride,
                                             int r0, int r_end, const float* add, int tid) {
  constexpr int V = DH / 4, DP = DH + 4;
#pragma unroll
  for (int e = tid; e < AT_TILE * V; e += AT_THREADS) {
    const int r = e / V, c = (e - r * V) * 4, rr = r0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rr >= 0 && rr < r_end) {
      v = ld4(src + (size_t)rr * row_stride + c);
      if (add != nullptr) v = add4(v, ld4(add + c));
    }
    st4(tile + r * DP + c, v);
  }
}

template <int DH>
__device__ __forceinline__ float ra_rowdot(const float* row, const float* vec) {
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < DH; d += 4) {
    const float4 a = ld4(row + d), b = ld4(vec + d);
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    acc = fmaf(a.w, b.w, acc);
  }
  return acc;
}

// the two bias vectors of head h into LDS: va = a, vd = b - a
template <int DH>
__device__ __forceinline__ void ra_load_bias(float* va, float* vd, const float* a, const float* b,
                                             int tid) {
  if (tid < DH) {
    const float x = a[tid];
    va[tid] = x;
    vd[tid] = b[tid] - x;
  }
}

// G (64 x 128) = Qs Band^T, every element stored at Ps[row][row - b + 63] when that is a column
template <int DH>
__device__ __forceinline__ void ra_band_scores(const float* Qs, const float* Bs, float* Ps, int ty,
                                               int tx) {
  constexpr int DP = DH + 4;
#pragma unroll 1
  for (int hf = 0; hf < 2; ++hf) {
    float gq[4][4];
    at_dot<DH>(Qs, Bs + hf * AT_TILE * DP, ty, tx, gq);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 4 * ty + i, col = row - (64 * hf + tx + 16 * j) + 63;
        if (col >= 0 && col < AT_TILE) Ps[row * AT_PP + col] = gq[i][j];
      }
  }
}

// THE FORWARD PASS: a workgroup owns up to 64 consecutive queries (rows r0 .. of the query source,
// the absolute frames q0 ..) of one (sample, head) and walks the absolute 64-aligned key tiles in
// ascending order.  STREAM: a row's running maximum and sum depend only on how its visible keys
// are split into tiles and on each key's column inside its tile, and a tile without a visible key
// for the row is an exact no-op (alpha = 1, or 0 on sums that are 0); stale ring rows and band rows
// outside the table (staged as zeros) meet masked pairs only; lens is kv_len (a key at or past
// t0 + T does not exist yet and is never visible); no lse.  CROSS: the keys are rows 0 .. Tk - 1
// of their own slab; rows n >= N of lse are written (zeros) too.
template <int DH, bool WIN, bool REL, bool STREAM, bool CROSS = false>
__global__ __launch_bounds__(AT_THREADS) void attn_fwd_kernel(
    const float* __restrict__ q, const float* __restrict__ kv, const int* __restrict__ lens,
    const int* __restrict__ qlens, const float* __restrict__ pos,
    const float* __restrict__ bias_u,
    const float* __restrict__ bias_v, float* __restrict__ out, float* __restrict__ lse, AtGeo g,
    asr_attn_window w) {
  static_assert(WIN || !STREAM, "a streaming call has a window");
  static_assert(!CROSS || !(WIN || REL || STREAM), "the cross form is the plain one");
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 at_lds4[];
  float* Qs = reinterpret_cast<float*>(at_lds4);
  float* Ks = Qs + AT_TILE * DP;
  float* Vs = Ks + AT_TILE * DP;
  float* Bs = Vs + AT_TILE * DP;            // REL: 128 band rows
  float* Ps = Bs + (REL ? 2 * AT_TILE * DP : 0);
  float* cP = Ps + AT_TILE * AT_PP;         // REL (as vu, vd)
  float* vu = cP + 256, *vd = vu + 64;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int r0 = blockIdx.x * AT_TILE, h = blockIdx.y, n = blockIdx.z;
  const int D = g.heads * DH;
  const size_t rs = (size_t)g.n_pad * g.ld, rsk = (size_t)g.n_pad * g.ld_kv;
  const size_t rso = (size_t)g.n_pad * g.ld_out;
  float* o_base = out + (size_t)n * g.ld_out;
  if (h == 0) at_zero_cols(o_base, rso, r0, g.T, D, g.ld_out - D, tid);
  if (n >= g.N) {
    at_zero_cols(o_base, rso, r0, g.T, h * DH, DH, tid);
    if constexpr (CROSS)
      if (lse != nullptr && tid < AT_TILE && r0 + tid < g.T)
        lse[((size_t)(r0 + tid) * g.n_pad + n) * g.heads + h] = 0.f;
    return;
  }
  int qend = g.T;                           // one past the last valid query row
  if constexpr (CROSS) qend = at_qlen(qlens, n, g.T);
  const float* qbase = q + (size_t)n * g.ld + h * DH;
  const float* kbase = kv + (size_t)n * g.ld_kv + h * DH;
  const float* pos_h = pos + h * DH;
  int q0 = r0, t_end = g.T;                 // the absolute frame of row r0; one past the last query
  if constexpr (STREAM) q0 += g.t0, t_end += g.t0;
  const int len = at_len(lens, n, CROSS ? g.Tk : t_end);
  if constexpr (REL) {
    ra_load_bias<DH>(vu, vd, bias_u + h * DH, bias_v + h * DH, tid);
    __syncthreads();
    ra_load_rows<DH>(Qs, qbase, rs, r0, g.T, vu, tid);
  } else {
    at_load_tile<DH>(Qs, qbase, rs, r0, qend, tid);
  }
  float m[4], l[4], o[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m[i] = asr_neg_inf();
    l[i] = 0.f;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) o[i][jj] = 0.f;
  }
  int kb = 0, ke = len, wlo[4], whi[4];     // key tiles to visit; the visible keys of row i
  if constexpr (WIN) {
    at_win_keys(w, q0, t_end, len, &kb, &ke);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wlo[i] = at_win_lo(w, q0 + 4 * ty + i);
      whi[i] = min(at_win_hi(w, q0 + 4 * ty + i), len);
    }
  }
  for (int k0 = kb; k0 < ke; k0 += AT_TILE) {
    // the tile's first row in the key source (k0 and R are multiples of 64: 64 consecutive ring
    // rows); rows that hold frames >= len: zeros
    if constexpr (STREAM) {
      const float* tile = kbase + (size_t)(k0 % g.R) * rsk;
      at_load_tile<DH>(Ks, tile, rsk, 0, len - k0, tid);
      at_load_tile<DH>(Vs, tile + D, rsk, 0, len - k0, tid);
    } else {
      at_load_tile<DH>(Ks, kbase, rsk, k0, len, tid);
      at_load_tile<DH>(Vs, kbase + D, rsk, k0, len, tid);
    }
    if constexpr (REL) {
      // (a whole utterance's P is its T: read as T, the compiler sees ONE number, and the
      // registers of these instantiations stay what they were with a kernel of their own)
      const int P = STREAM ? g.P : g.T;
      const int pr0 = q0 - k0 - 63 + P - 1;             // table row of band row 0
      ra_load_rows<DH>(Bs, pos_h, g.ld_pos, pr0, 2 * P - 1, nullptr, tid);
      ra_load_rows<DH>(Bs + AT_TILE * DP, pos_h, g.ld_pos, pr0 + 64, 2 * P - 1, nullptr, tid);
    }
    __syncthreads();
    if constexpr (REL)
      if (tid < 128) cP[tid] = ra_rowdot<DH>(Bs + tid * DP, vd);
    float s[4][4];
    at_dot<DH>(Qs, Ks, ty, tx, s);
    if constexpr (REL) {
      ra_band_scores<DH>(Qs, Bs, Ps, ty, tx);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * ty + i;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = tx + 16 * j;
        const float sp = REL ? Ps[row * AT_PP + col] + cP[row - col + 63] : 0.f;
        bool vis = k0 + col < len;
        if constexpr (WIN) vis = k0 + col >= wlo[i] && k0 + col < whi[i];
        s[i][j] = vis ? (REL ? s[i][j] + sp : s[i][j]) * g.c2 : asr_neg_inf();
      }
    }
    at_softmax_tile<NJ, WIN>(s, m, l, o);
    if constexpr (REL) __syncthreads();     // (every G read before P overwrites it)
    at_put_tile(Ps, s, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Vs, ty, tx, o);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + 4 * ty + i;
    if (r >= g.T) continue;
    float* orow = o_base + (size_t)r * rso + h * DH;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      float v = o[i][jj] / l[i];
      if constexpr (WIN) v = l[i] == 0.f ? 0.f : v;      // a row with no visible key: out = lse = 0
      if constexpr (CROSS) v = r < qend ? v : 0.f;       // a padding query: likewise
      orow[tx + 16 * jj] = v;
    }
    if constexpr (!STREAM) {
      if (lse != nullptr && tx == 0) {
        float v = (m[i] + log2f(l[i])) * AT_LN2;
        if constexpr (WIN) v = l[i] == 0.f ? 0.f : v;
        if constexpr (CROSS) v = r < qend ? v : 0.f;
        lse[((size_t)r * g.n_pad + n) * g.heads + h] = v;
      }
    }
  }
}

// BACKWARD PASS 1: D = dout . out (to dvec, laid out like lse) and dQ, per query tile.  REL:
// dQ = dQ_c + dQ_p, the content and position parts; dQ_c -> slab_c, dQ_p -> slab_p (T, n_pad, D).
// q / dq are the query source and its gradient (rows ld floats apart), kv the [K | V] columns of
// the key source: q + D of the one qkv slab, or (CROSS) a slab of its own with rows ld_kv apart,
// in which case the pad columns of dq (>= D) are written as zeros here.
template <int DH, bool WIN, bool REL, bool CROSS = false>
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_dq_kernel(
    const float* __restrict__ q, const float* __restrict__ kv, const int* __restrict__ lens,
    const int* __restrict__ qlens, const float* __restrict__ pos,
    const float* __restrict__ bias_u, const float* __restrict__ bias_v,
    const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ dout,
    float* __restrict__ dq_out, float* __restrict__ dvec, float* __restrict__ slab_c,
    float* __restrict__ slab_p, AtGeo g, asr_attn_window w) {
  static_assert(!CROSS || !(WIN || REL), "the cross form is the plain one");
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 at_lds4[];
  float* Qs = reinterpret_cast<float*>(at_lds4);
  float* Gs = Qs + AT_TILE * DP;            // dO tile
  float* Ks = Gs + AT_TILE * DP;
  float* Vs = Ks + AT_TILE * DP;
  float* Bs = Vs + AT_TILE * DP;            // REL: 128 band rows
  float* Ps = Bs + (REL ? 2 * AT_TILE * DP : 0);
  float* P2 = Ps + AT_TILE * AT_PP;         // REL (as cP, vu, vd): dS of a band half by band row
  float* cP = P2 + AT_TILE * AT_PP;
  float* vu = cP + 256, *vd = vu + 64;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int q0 = blockIdx.x * AT_TILE, h = blockIdx.y, n = blockIdx.z;
  const int D = g.heads * DH;
  const size_t rs = (size_t)g.n_pad * g.ld, rso = (size_t)g.n_pad * g.ld_out;
  const size_t rsd = (size_t)g.n_pad * D;
  const int ldk = CROSS ? g.ld_kv : g.ld;
  const size_t rsk = CROSS ? (size_t)g.n_pad * g.ld_kv : rs;
  float* dq_base = dq_out + (size_t)n * g.ld;
  float* sc_base = slab_c + (size_t)n * D + h * DH;
  float* sp_base = slab_p + (size_t)n * D + h * DH;
  if constexpr (CROSS)
    if (h == 0) at_zero_cols(dq_base, rs, q0, g.T, D, g.ld - D, tid);
  if (n >= g.N) {
    at_zero_cols(dq_base, rs, q0, g.T, h * DH, DH, tid);
    if constexpr (REL) {
      at_zero_cols(sc_base, rsd, q0, g.T, 0, DH, tid);
      at_zero_cols(sp_base, rsd, q0, g.T, 0, DH, tid);
    }
    return;
  }
  const float* base = q + (size_t)n * g.ld + h * DH;
  const float* kbase = kv + (size_t)n * ldk + h * DH;
  const float* do_base = dout + (size_t)n * g.ld_out + h * DH;
  const float* o_base = out + (size_t)n * g.ld_out + h * DH;
  const float* pos_h = pos + h * DH;
  const int len = at_len(lens, n, CROSS ? g.Tk : g.T);
  int qend = g.T;                           // one past the last valid query row
  if constexpr (CROSS) qend = at_qlen(qlens, n, g.T);
  if constexpr (REL) {
    ra_load_bias<DH>(vu, vd, bias_u + h * DH, bias_v + h * DH, tid);
    __syncthreads();
    ra_load_rows<DH>(Qs, base, rs, q0, g.T, vu, tid);
  } else {
    at_load_tile<DH>(Qs, base, rs, q0, qend, tid);
  }
  at_load_tile<DH>(Gs, do_base, rso, q0, qend, tid);
  __syncthreads();
  float lse2[4], dsum[4], dq[4][NJ], dqp[4][NJ];         // dqp: REL
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = q0 + 4 * ty + i;
    float acc = 0.f;
    if (t < qend) {
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj)
        acc = fmaf(Gs[(4 * ty + i) * DP + tx + 16 * jj], o_base[(size_t)t * rso + tx + 16 * jj], acc);
    }
    dsum[i] = at_sum16(acc);
    const size_t li = ((size_t)(t < g.T ? t : 0) * g.n_pad + n) * g.heads + h;
    lse2[i] = lse[li] * AT_LOG2E;
    if (t < g.T && tx == 0) dvec[li] = dsum[i];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) dq[i][jj] = dqp[i][jj] = 0.f;
  }
  int kb = 0, ke = len, wlo[4], whi[4];     // key tiles to visit; the visible keys of row i
  if constexpr (WIN) {
    at_win_keys(w, q0, g.T, len, &kb, &ke);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wlo[i] = at_win_lo(w, q0 + 4 * ty + i);
      whi[i] = min(at_win_hi(w, q0 + 4 * ty + i), len);
    }
  }
  for (int k0 = kb; k0 < ke; k0 += AT_TILE) {
    at_load_tile<DH>(Ks, kbase, rsk, k0, len, tid);
    at_load_tile<DH>(Vs, kbase + D, rsk, k0, len, tid);
    if constexpr (REL) {
      const int pr0 = q0 - k0 - 63 + g.T - 1;
      ra_load_rows<DH>(Bs, pos_h, g.ld_pos, pr0, 2 * g.T - 1, nullptr, tid);
      ra_load_rows<DH>(Bs + AT_TILE * DP, pos_h, g.ld_pos, pr0 + 64, 2 * g.T - 1, nullptr, tid);
    }
    __syncthreads();
    if constexpr (REL)
      if (tid < 128) cP[tid] = ra_rowdot<DH>(Bs + tid * DP, vd);
    float s[4][4], dp[4][4];
    at_dot<DH>(Qs, Ks, ty, tx, s);
    at_dot<DH>(Gs, Vs, ty, tx, dp);
    if constexpr (REL) {
      ra_band_scores<DH>(Qs, Bs, Ps, ty, tx);
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 4 * ty + i, col = tx + 16 * j;
        const float sp = REL ? Ps[row * AT_PP + col] + cP[row - col + 63] : 0.f;
        bool vis = k0 + col < len;
        if constexpr (WIN) vis = k0 + col >= wlo[i] && k0 + col < whi[i];
        if constexpr (CROSS) vis = vis && q0 + row < qend;
        const float p = vis ? exp2f(fmaf(REL ? s[i][j] + sp : s[i][j], g.c2, -lse2[i])) : 0.f;
        s[i][j] = p * (dp[i][j] - dsum[i]) * g.scale;
      }
    if constexpr (REL) __syncthreads();     // (every G read before dS overwrites it)
    at_put_tile(Ps, s, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Ks, ty, tx, dq);
    if constexpr (REL) {
#pragma unroll 1
      for (int hf = 0; hf < 2; ++hf) {      // dQ_p += dG_half Band_half, dG[row][b] = dS[row][row - b + 63]
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int row = 4 * ty + i, bb = tx + 16 * j, col = row - (64 * hf + bb) + 63;
            P2[row * AT_PP + bb] = (col >= 0 && col < AT_TILE) ? Ps[row * AT_PP + col] : 0.f;
          }
        __syncthreads();
        at_acc<DH>(P2, Bs + hf * AT_TILE * DP, ty, tx, dqp);
        __syncthreads();
      }
    } else {
      __syncthreads();
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = q0 + 4 * ty + i;
    if (t >= g.T) continue;
    float* row = dq_base + (size_t)t * rs + h * DH;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      if constexpr (REL) {
        row[tx + 16 * jj] = dq[i][jj] + dqp[i][jj];
        sc_base[(size_t)t * rsd + tx + 16 * jj] = dq[i][jj];
        sp_base[(size_t)t * rsd + tx + 16 * jj] = dqp[i][jj];
      } else {
        row[tx + 16 * jj] = dq[i][jj];
      }
    }
  }
}

// BACKWARD PASS 2: dK and dV of one key tile over all query tiles (query tiles ascending).  REL:
// Qs holds q + b_u, so dK sees it.  kv / dkv are the [K | V] columns of the key source and of its
// gradient: q + D and dq + D of the qkv / dqkv slabs, or (CROSS) slabs (Tk, n_pad, ld_kv) of
// their own; the columns behind dV are written as zeros here.
template <int DH, bool WIN, bool REL, bool CROSS = false>
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_dkv_kernel(
    const float* __restrict__ q, const float* __restrict__ kv, const int* __restrict__ lens,
    const int* __restrict__ qlens, const float* __restrict__ pos,
    const float* __restrict__ bias_u, const float* __restrict__ bias_v,
    const float* __restrict__ lse, const float* __restrict__ dout, float* __restrict__ dkv,
    const float* __restrict__ dvec, AtGeo g, asr_attn_window w) {
  static_assert(!CROSS || !(WIN || REL), "the cross form is the plain one");
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 at_lds4[];
  float* Ks = reinterpret_cast<float*>(at_lds4);
  float* Vs = Ks + AT_TILE * DP;
  float* Qs = Vs + AT_TILE * DP;
  float* Gs = Qs + AT_TILE * DP;            // dO tile
  float* Bs = Gs + AT_TILE * DP;            // REL: 128 band rows
  float* Ps = Bs + (REL ? 2 * AT_TILE * DP : 0);
  float* cP = Ps + AT_TILE * AT_PP;         // REL: 128 floats
  float* Ls = cP + (REL ? 128 : 0);         // lse (base 2) of the query tile
  float* Ds = Ls + AT_TILE;                 // D of the query tile
  float* vu = Ds + AT_TILE, *vd = vu + 64;  // REL
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int k0 = blockIdx.x * AT_TILE, h = blockIdx.y, n = blockIdx.z;
  const int D = g.heads * DH;
  const size_t rs = (size_t)g.n_pad * g.ld, rso = (size_t)g.n_pad * g.ld_out;
  const int Tk = CROSS ? g.Tk : g.T, ldk = CROSS ? g.ld_kv : g.ld;
  const size_t rsk = CROSS ? (size_t)g.n_pad * g.ld_kv : rs;
  float* d_base = dkv + (size_t)n * ldk;
  if (h == 0) at_zero_cols(d_base, rsk, k0, Tk, 2 * D, ldk - (CROSS ? 2 : 3) * D, tid);
  const int len = n < g.N ? at_len(lens, n, Tk) : 0;
  if (k0 >= len) {          // a padding sample, or a tile of masked keys only
    at_zero_cols(d_base, rsk, k0, Tk, h * DH, DH, tid);
    at_zero_cols(d_base, rsk, k0, Tk, D + h * DH, DH, tid);
    return;
  }
  const float* base = q + (size_t)n * g.ld + h * DH;
  const float* kbase = kv + (size_t)n * ldk + h * DH;
  const float* do_base = dout + (size_t)n * g.ld_out + h * DH;
  const float* pos_h = pos + h * DH;
  int qend = g.T;                           // one past the last valid query row
  if constexpr (CROSS) qend = at_qlen(qlens, n, g.T);
  if constexpr (REL) ra_load_bias<DH>(vu, vd, bias_u + h * DH, bias_v + h * DH, tid);
  at_load_tile<DH>(Ks, kbase, rsk, k0, len, tid);
  at_load_tile<DH>(Vs, kbase + D, rsk, k0, len, tid);
  if constexpr (REL) __syncthreads();       // (vu before the first query tile adds it)
  float dk[4][NJ], dv[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) dk[i][jj] = dv[i][jj] = 0.f;
  for (int q0 = 0; q0 < qend; q0 += AT_TILE) {
    int qlo[4], qhi[4];                     // the visible keys of query tx + 16 j
    if constexpr (WIN) {
      // only the query tiles that see a key of this tile: one contiguous range, lo and hi being
      // monotone (a tile no query sees accumulates nothing: exact zeros)
      if (!at_win_pair(w, q0, min(q0 + AT_TILE, g.T) - 1, k0)) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        qlo[j] = at_win_lo(w, q0 + tx + 16 * j);
        qhi[j] = at_win_hi(w, q0 + tx + 16 * j);
      }
    }
    if constexpr (REL) {
      ra_load_rows<DH>(Qs, base, rs, q0, g.T, vu, tid);
    } else {
      at_load_tile<DH>(Qs, base, rs, q0, qend, tid);
    }
    at_load_tile<DH>(Gs, do_base, rso, q0, qend, tid);
    if constexpr (REL) {
      const int pr0 = q0 - k0 - 63 + g.T - 1;
      ra_load_rows<DH>(Bs, pos_h, g.ld_pos, pr0, 2 * g.T - 1, nullptr, tid);
      ra_load_rows<DH>(Bs + AT_TILE * DP, pos_h, g.ld_pos, pr0 + 64, 2 * g.T - 1, nullptr, tid);
    }
    if (tid < AT_TILE) {
      const int t = q0 + tid;
      const size_t li = ((size_t)(t < g.T ? t : 0) * g.n_pad + n) * g.heads + h;
      Ls[tid] = lse[li] * AT_LOG2E;
      Ds[tid] = dvec[li];
    }
    __syncthreads();
    if constexpr (REL)
      if (tid < 128) cP[tid] = ra_rowdot<DH>(Bs + tid * DP, vd);
    float s[4][4], dp[4][4];
    at_dot<DH>(Ks, Qs, ty, tx, s);          // s[i][j]: key 4 ty + i, query tx + 16 j
    at_dot<DH>(Vs, Gs, ty, tx, dp);
    if constexpr (REL) {
#pragma unroll 1
      for (int hf = 0; hf < 2; ++hf) {      // G^T: band row 64 hf + 4 ty + i, query tx + 16 j
        float gq[4][4];
        at_dot<DH>(Bs + hf * AT_TILE * DP, Qs, ty, tx, gq);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = tx + 16 * j, kk = q - (64 * hf + 4 * ty + i) + 63;
            if (kk >= 0 && kk < AT_TILE) Ps[kk * AT_PP + q] = gq[i][j];
          }
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = tx + 16 * j, kk = 4 * ty + i;
        bool live = (k0 + kk < len) && (q0 + q < qend);
        if constexpr (WIN) live = live && k0 + kk >= qlo[j] && k0 + kk < qhi[j];
        const float sp = REL ? Ps[kk * AT_PP + q] + cP[q - kk + 63] : 0.f;
        s[i][j] = live ? exp2f(fmaf(REL ? s[i][j] + sp : s[i][j], g.c2, -Ls[q])) : 0.f;
        dp[i][j] = s[i][j] * (dp[i][j] - Ds[q]) * g.scale;
      }
    if constexpr (REL) __syncthreads();     // (every G read before P overwrites it)
    at_put_tile(Ps, s, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Gs, ty, tx, dv);
    __syncthreads();
    at_put_tile(Ps, dp, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Qs, ty, tx, dk);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = k0 + 4 * ty + i;
    if (u >= Tk) continue;
    float* row = d_base + (size_t)u * rsk + h * DH;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {       // (rows u >= len accumulated p = 0 only: exact zeros)
      row[tx + 16 * jj] = dk[i][jj];
      row[D + tx + 16 * jj] = dv[i][jj];
    }
  }
}

// ------------------------------------------------------------------------------ the host path
// LDS bytes of a pass: 0 forward, 1 dQ, 2 dK / dV (3, the relative family's dpos, is
// rel_attention.hip's)
template <bool REL>
size_t at_lds_bytes(int dh, int pass) {
  const size_t tile = (size_t)AT_TILE * (dh + 4) * sizeof(float);
  const size_t p = (size_t)AT_TILE * AT_PP * sizeof(float);
  if constexpr (REL) {
    const size_t small = RA_SMALL * sizeof(float);
    return pass == 0 ? 5 * tile + p + small : 6 * tile + (pass == 1 ? 2 : 1) * p + small;
  }
  return pass ? 4 * tile + p + 2 * AT_TILE * sizeof(float) : 3 * tile + p;
}

// the geometry of a whole-utterance call, from asr_attn_args or asr_relattn_args
template <typename Args>
AtGeo at_geo(const Args* a, int ld_pos) {
  AtGeo g;
  g.T = a->T, g.N = a->N, g.n_pad = a->n_pad, g.heads = a->heads, g.ld = a->ld, g.ld_kv = a->ld;
  g.ld_out = a->ld_out, g.ld_pos = ld_pos, g.R = 0, g.t0 = 0, g.P = a->T, g.Tk = a->T;
  g.scale = a->scale, g.c2 = a->scale * AT_LOG2E;
  return g;
}
// ... and of a streaming call
inline AtGeo at_geo(const asr_attn_stream_args* a) {
  AtGeo g;
  g.T = a->Tq, g.N = a->N, g.n_pad = a->n_pad, g.heads = a->heads, g.ld = a->ld;
  g.ld_kv = a->ld_kv, g.ld_out = a->ld_out, g.ld_pos = a->ld_pos, g.R = a->R, g.t0 = a->t0;
  g.P = a->P, g.Tk = 0, g.scale = a->scale, g.c2 = a->scale * AT_LOG2E;
  return g;
}
// ... and of a cross call
inline AtGeo at_geo(const asr_attn_cross_args* a) {
  AtGeo g;
  g.T = a->Tq, g.Tk = a->Tk, g.N = a->N, g.n_pad = a->n_pad, g.heads = a->heads, g.ld = a->ld_q;
  g.ld_kv = a->ld_kv, g.ld_out = a->ld_out, g.ld_pos = 0, g.R = 0, g.t0 = 0, g.P = 0;
  g.scale = a->scale, g.c2 = a->scale * AT_LOG2E;
  return g;
}

// one workgroup per 64 rows of a side: the queries (forward, pass 1) or the keys (pass 2)
inline dim3 at_grid(const AtGeo& g, int rows) {
  return dim3((rows + AT_TILE - 1) / AT_TILE, g.heads, g.n_pad);
}

// bq, bk, blocks of a plan (any pointer may be NULL)
inline void at_plan(int T, int heads, int n_pad, int* bq, int* bk, int* blocks) {
  if (bq) *bq = AT_TILE;
  if (bk) *bk = AT_TILE;
  if (blocks) *blocks = (T + AT_TILE - 1) / AT_TILE * heads * n_pad;
}

// launch(DH as a std::integral_constant) for the head size dh, one of 16, 32 .. MAX_DH (the
// callers have checked it): the ONE dispatch, which instantiates a family's kernels up to its
// own MAX_DH only
template <int MAX_DH, int DH = 16, typename F>
int at_dispatch(int dh, F&& launch) {
  if constexpr (DH >= MAX_DH) {
    return launch(std::integral_constant<int, MAX_DH>{});
  } else {
    if (dh == DH) return launch(std::integral_constant<int, DH>{});
    return at_dispatch<MAX_DH, DH + 16>(dh, launch);
  }
}

// The forward launch of every form: w == nullptr: the unwindowed kernels (not for STREAM; CROSS
// has no other).  qlens: CROSS only.
template <bool REL, bool STREAM, bool CROSS = false>
int at_launch_fwd(const float* q, const float* kv, const int* lens, const int* qlens,
                  const float* pos, const float* bias_u, const float* bias_v, float* out,
                  float* lse, const AtGeo& g, int dh, const asr_attn_window* w,
                  asr_stream_t stream) {
  const size_t lds = at_lds_bytes<REL>(dh, 0);
  const asr_attn_window win = w ? *w : asr_attn_window{1, -1, 0};
  auto go = [&](auto kernel) -> int {
    if (at_allow_lds(kernel, lds) != ASR_OK) return ASR_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel, at_grid(g, g.T), dim3(AT_THREADS), lds, (hipStream_t)stream, q, kv,
                       lens, qlens, pos, bias_u, bias_v, out, lse, g, win);
    ASR_CHECK_LAUNCH();
    return ASR_OK;
  };
  return at_dispatch<REL ? RA_MAX_DH : AT_MAX_DH>(dh, [&](auto c) -> int {
    constexpr int DH = decltype(c)::value;
    if constexpr (CROSS) {
      return go(attn_fwd_kernel<DH, false, false, false, true>);
    } else if constexpr (STREAM) {
      return go(attn_fwd_kernel<DH, true, REL, true>);
    } else {
      return w ? go(attn_fwd_kernel<DH, true, REL, false>)
               : go(attn_fwd_kernel<DH, false, REL, false>);
    }
  });
}

// The launches of backward passes 1 and 2 (plain: pos .. bias_v, slab_c, slab_p are nullptr).
// One qkv slab: kv = q + D, dkv = dq + D.  qlens: CROSS only.
template <bool REL, bool CROSS = false>
int at_launch_bwd(const float* q, const float* kv, const int* lens, const int* qlens,
                  const float* pos, const float* bias_u, const float* bias_v, const float* out,
                  const float* lse, const float* dout, float* dq, float* dkv, float* dvec,
                  float* slab_c, float* slab_p, const AtGeo& g, int dh, const asr_attn_window* w,
                  asr_stream_t stream) {
  const size_t lds1 = at_lds_bytes<REL>(dh, 1), lds2 = at_lds_bytes<REL>(dh, 2);
  const asr_attn_window win = w ? *w : asr_attn_window{1, -1, 0};
  hipStream_t s = (hipStream_t)stream;
  auto go = [&](auto dq_kernel, auto dkv_kernel) -> int {
    if (at_allow_lds(dq_kernel, lds1) != ASR_OK) return ASR_ERR_LAUNCH;
    if (at_allow_lds(dkv_kernel, lds2) != ASR_OK) return ASR_ERR_LAUNCH;
    hipLaunchKernelGGL(dq_kernel, at_grid(g, g.T), dim3(AT_THREADS), lds1, s, q, kv, lens, qlens,
                       pos, bias_u, bias_v, out, lse, dout, dq, dvec, slab_c, slab_p, g, win);
    hipLaunchKernelGGL(dkv_kernel, at_grid(g, CROSS ? g.Tk : g.T), dim3(AT_THREADS), lds2, s, q, kv,
                       lens, qlens, pos, bias_u, bias_v, lse, dout, dkv, (const float*)dvec, g, win);
    ASR_CHECK_LAUNCH();
    return ASR_OK;
  };
  return at_dispatch<REL ? RA_MAX_DH : AT_MAX_DH>(dh, [&](auto c) -> int {
    constexpr int DH = decltype(c)::value;
    if constexpr (CROSS) {
      return go(attn_bwd_dq_kernel<DH, false, false, true>,
                attn_bwd_dkv_kernel<DH, false, false, true>);
    } else {
      return w ? go(attn_bwd_dq_kernel<DH, true, REL>, attn_bwd_dkv_kernel<DH, true, REL>)
               : go(attn_bwd_dq_kernel<DH, false, REL>, attn_bwd_dkv_kernel<DH, false, REL>);
    }
  });
}

}  // namespace
