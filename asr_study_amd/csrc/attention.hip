// K21 multi-head self-attention core (softmax(scale Q K^T) V, key-masked by length), forward and
// backward, fused, and the sinusoidal positional-encoding add.
//
// qkv is a time-major slab (T, n_pad, ld >= 3D), column blocks [Q | K | V] of D = heads * dh
// columns each, head h in columns h dh .. (h + 1) dh - 1 of its block: what one x @ W_qkv + b_qkv
// GEMM writes.  For every real sample n < N, head h and query frame t (ALL T frames are queries):
//   s[t,u] = scale q_t . k_u for u < lens[n] (u < T without lens), p = softmax_u(s), keys
//   u >= lens[n] carry probability exactly 0, out_t = sum_u p[t,u] v_u, lse_t = log sum_u exp s.
// Backward, with D_t = dout_t . out_t:  dV = P^T dO,  dS = P (.) (dO V^T - D),  dQ = scale dS K,
// dK = scale dS^T Q; masked keys get dK = dV = exactly 0.  Rows n >= N and the pad columns of
// out / dqkv are written as exact zeros.
//
// ARITHMETIC: exact fp32 -- every product is an fmaf on fp32 operands with fp32 accumulation
// (vector FMAs, which the compiler packs two to a v_pk_fma_f32 where it can; no MFMA, no split
// planes); exponentials are base 2 (v_exp_f32) on scores pre-multiplied by scale log2(e), as
// ctc.hip does.
//
// TILING: a workgroup of 256 threads (16 x 16) owns a 64-row tile of one (sample, head) and
// streams 64-row tiles of the other side through LDS; T is not bounded by LDS.  A tile row is
// dh + 4 floats apart ((dh + 4) / 4 is odd: the 16 lanes of a row group read 16-byte pieces of 16
// different rows without a bank conflict).  A 64 x 64 score tile lives in registers, 4 x 4 per
// thread (rows 4 ty + i, columns tx + 16 j); the row statistics are xor butterflies over the 16
// tx lanes; the tile then goes through LDS once for the second product (64 x dh, 4 x dh / 16 per
// thread).  The T x T matrix never reaches HBM: the forward keeps the running maximum / sum, the
// backward recomputes p = exp2(s - lse) from the saved lse.
//   forward:  grid (query tiles, heads, n_pad); key tiles up to lens[n].
//   backward: (1) the same grid over query tiles: D (to the workspace) and dQ;
//             (2) grid (key tiles, heads, n_pad): dK and dV over all query tiles.
// Every output element is written by exactly one thread, which adds its terms in one fixed
// order: no float atomics, repeats are bit-identical.  No workgroup waits on another one.
// The tile pieces (loads, the two products, the butterflies) are in attn_tile.h, which
// rel_attention.hip shares.
//
// K25, THE WINDOW (asr_attn_win_*; defined once in attn_tile.h): chunk >= 1, left >= -1 frames
// (-1: unlimited), right >= 0 frames.  For query frame t, c0 = (t / chunk) * chunk, key u is
// visible iff lo(t) <= u < hi(t) and u < lens[n], hi(t) = c0 + chunk + right, lo(t) = left < 0 ?
// 0 : max(0, c0 - left).  The kernels are templates on a bool: without the window they are the
// code above, bit for bit.  With it the mask stays a select (a key outside meets p = exactly 0
// only) and the loops visit only the tiles that hold a visible pair:
//   forward, dQ: the key tiles that meet [lo(q0), min(hi(last query of the tile), len));
//   dK / dV:     the query tiles with lo(first) <= k0 + 63 and hi(last) > k0 (lo, hi monotone:
//                one contiguous range; a key tile no query sees writes exact zeros).
// A row with NO visible key (a padding query with lo(t) >= len) has out = lse = exactly 0: the
// forward guards exp2f(-inf - -inf) and the division by l = 0; the backward recomputes p = 0 for
// it everywhere, so dQ_t = 0 and it adds nothing to dK, dV.
#include "attn_tile.h"

namespace {

struct AtGeo {
  int T, N, n_pad, heads, ld, ld_out;
  float c2;         // scale * log2(e)
  float scale;
};

// WIN: under the window w of attn_tile.h (K25); without it w is not read and the code is the
// unwindowed kernel's, instruction for instruction.
template <int DH, bool WIN>
__global__ __launch_bounds__(AT_THREADS) void attn_fwd_kernel(const float* __restrict__ qkv,
                                                              const int* __restrict__ lens,
                                                              float* __restrict__ out,
                                                              float* __restrict__ lse, AtGeo g,
                                                              asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 at_lds4[];
  float* Qs = reinterpret_cast<float*>(at_lds4);
  float* Ks = Qs + AT_TILE * DP;
  float* Vs = Ks + AT_TILE * DP;
  float* Ps = Vs + AT_TILE * DP;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int q0 = blockIdx.x * AT_TILE, h = blockIdx.y, n = blockIdx.z;
  const int D = g.heads * DH;
  const size_t rs = (size_t)g.n_pad * g.ld, rso = (size_t)g.n_pad * g.ld_out;
  float* o_base = out + (size_t)n * g.ld_out;
  if (h == 0) at_zero_cols(o_base, rso, q0, g.T, D, g.ld_out - D, tid);
  if (n >= g.N) {
    at_zero_cols(o_base, rso, q0, g.T, h * DH, DH, tid);
    return;
  }
  const float* base = qkv + (size_t)n * g.ld + h * DH;
  const int len = at_len(lens, n, g.T);
  at_load_tile<DH>(Qs, base, rs, q0, g.T, tid);
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
    at_win_keys(w, q0, g.T, len, &kb, &ke);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wlo[i] = at_win_lo(w, q0 + 4 * ty + i);
      whi[i] = min(at_win_hi(w, q0 + 4 * ty + i), len);
    }
  }
  for (int k0 = kb; k0 < ke; k0 += AT_TILE) {
    at_load_tile<DH>(Ks, base + D, rs, k0, len, tid);
    at_load_tile<DH>(Vs, base + 2 * D, rs, k0, len, tid);
    __syncthreads();
    float s[4][4];
    at_dot<DH>(Qs, Ks, ty, tx, s);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int u = k0 + tx + 16 * j;
        bool vis = u < len;
        if constexpr (WIN) vis = u >= wlo[i] && u < whi[i];
        s[i][j] = vis ? s[i][j] * g.c2 : asr_neg_inf();
      }
    at_softmax_tile<NJ, WIN>(s, m, l, o);
    at_put_tile(Ps, s, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Vs, ty, tx, o);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = q0 + 4 * ty + i;
    if (t >= g.T) continue;
    float* orow = o_base + (size_t)t * rso + h * DH;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      float v = o[i][jj] / l[i];
      if constexpr (WIN) v = l[i] == 0.f ? 0.f : v;      // a row with no visible key: out = lse = 0
      orow[tx + 16 * jj] = v;
    }
    if (lse != nullptr && tx == 0) {
      float v = (m[i] + log2f(l[i])) * AT_LN2;
      if constexpr (WIN) v = l[i] == 0.f ? 0.f : v;
      lse[((size_t)t * g.n_pad + n) * g.heads + h] = v;
    }
  }
}

// K26, the streaming forward: the queries [t0, t0 + Tq) of the windowed forward above, Q from the
// chunk's slab (Tq, n_pad, ld), K and V from THE RING of attn_tile.h, columns [K | V] of
// (R, n_pad, ld_kv).  A workgroup owns up to 64 consecutive new queries and walks the ABSOLUTE
// 64-aligned key tiles asr_attn_win_fwd walks: a row's running maximum and sum depend only on how
// its visible keys are split into tiles and on each key's column inside its tile, and a tile
// without a visible key for the row is an exact no-op (alpha = 1, or 0 on sums that are 0), so
// the rows come out bit for bit as from the whole-utterance call.  kv_len[n] (device int32, the
// absolute frames of stream n that are valid so far) plays the part of lens; a key at or past
// t0 + Tq does not exist yet and is never visible.  No lse.
struct AtsGeo {
  int Tq, N, n_pad, heads, ld, ld_kv, ld_out, R, t0;
  float c2;         // scale * log2(e)
};

__device__ __forceinline__ int ats_len(const int* kv_len, int n, int end) {
  const int len = kv_len[n];
  return len < 1 ? 1 : (len > end ? end : len);       // (as at_len)
}

template <int DH>
__global__ __launch_bounds__(AT_THREADS) void attn_stream_kernel(const float* __restrict__ q,
                                                                 const float* __restrict__ ring,
                                                                 const int* __restrict__ kv_len,
                                                                 float* __restrict__ out,
                                                                 AtsGeo g, asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 at_lds4[];
  float* Qs = reinterpret_cast<float*>(at_lds4);
  float* Ks = Qs + AT_TILE * DP;
  float* Vs = Ks + AT_TILE * DP;
  float* Ps = Vs + AT_TILE * DP;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int r0 = blockIdx.x * AT_TILE, h = blockIdx.y, n = blockIdx.z;   // r0: row of the chunk
  const int D = g.heads * DH;
  const size_t rs = (size_t)g.n_pad * g.ld, rsk = (size_t)g.n_pad * g.ld_kv;
  const size_t rso = (size_t)g.n_pad * g.ld_out;
  float* o_base = out + (size_t)n * g.ld_out;
  if (h == 0) at_zero_cols(o_base, rso, r0, g.Tq, D, g.ld_out - D, tid);
  if (n >= g.N) {
    at_zero_cols(o_base, rso, r0, g.Tq, h * DH, DH, tid);
    return;
  }
  const float* kbase = ring + (size_t)n * g.ld_kv + h * DH;
  const int len = ats_len(kv_len, n, g.t0 + g.Tq);
  at_load_tile<DH>(Qs, q + (size_t)n * g.ld + h * DH, rs, r0, g.Tq, tid);
  float m[4], l[4], o[4][NJ];
  int wlo[4], whi[4];                       // the visible keys of row i
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m[i] = asr_neg_inf();
    l[i] = 0.f;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) o[i][jj] = 0.f;
    wlo[i] = at_win_lo(w, g.t0 + r0 + 4 * ty + i);
    whi[i] = min(at_win_hi(w, g.t0 + r0 + 4 * ty + i), len);
  }
  const int qa = g.t0 + r0, qb = g.t0 + min(r0 + AT_TILE, g.Tq) - 1;
  const int kb = at_win_lo(w, qa) / AT_TILE * AT_TILE, ke = min(at_win_hi(w, qb), len);
  for (int k0 = kb; k0 < ke; k0 += AT_TILE) {
    // (k0 and R are multiples of 64: the tile is 64 consecutive ring rows; rows >= len: zeros)
    const float* tile = kbase + (size_t)(k0 % g.R) * rsk;
    at_load_tile<DH>(Ks, tile, rsk, 0, len - k0, tid);
    at_load_tile<DH>(Vs, tile + D, rsk, 0, len - k0, tid);
    __syncthreads();
    float s[4][4];
    at_dot<DH>(Qs, Ks, ty, tx, s);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int u = k0 + tx + 16 * j;
        s[i][j] = (u >= wlo[i] && u < whi[i]) ? s[i][j] * g.c2 : asr_neg_inf();
      }
    at_softmax_tile<NJ, true>(s, m, l, o);
    at_put_tile(Ps, s, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Vs, ty, tx, o);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + 4 * ty + i;
    if (r >= g.Tq) continue;
    float* orow = o_base + (size_t)r * rso + h * DH;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) orow[tx + 16 * jj] = l[i] == 0.f ? 0.f : o[i][jj] / l[i];
  }
}

// backward pass 1: D = dout . out (to dvec, laid out like lse) and dQ, per query tile
template <int DH, bool WIN>
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_dq_kernel(
    const float* __restrict__ qkv, const int* __restrict__ lens, const float* __restrict__ out,
    const float* __restrict__ lse, const float* __restrict__ dout, float* __restrict__ dqkv,
    float* __restrict__ dvec, AtGeo g, asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 at_lds4[];
  float* Qs = reinterpret_cast<float*>(at_lds4);
  float* Gs = Qs + AT_TILE * DP;            // dO tile
  float* Ks = Gs + AT_TILE * DP;
  float* Vs = Ks + AT_TILE * DP;
  float* Ps = Vs + AT_TILE * DP;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int q0 = blockIdx.x * AT_TILE, h = blockIdx.y, n = blockIdx.z;
  const int D = g.heads * DH;
  const size_t rs = (size_t)g.n_pad * g.ld, rso = (size_t)g.n_pad * g.ld_out;
  float* dq_base = dqkv + (size_t)n * g.ld;
  if (n >= g.N) {
    at_zero_cols(dq_base, rs, q0, g.T, h * DH, DH, tid);
    return;
  }
  const float* base = qkv + (size_t)n * g.ld + h * DH;
  const float* do_base = dout + (size_t)n * g.ld_out + h * DH;
  const float* o_base = out + (size_t)n * g.ld_out + h * DH;
  const int len = at_len(lens, n, g.T);
  at_load_tile<DH>(Qs, base, rs, q0, g.T, tid);
  at_load_tile<DH>(Gs, do_base, rso, q0, g.T, tid);
  __syncthreads();
  float lse2[4], dsum[4], dq[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = q0 + 4 * ty + i;
    float acc = 0.f;
    if (t < g.T) {
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj)
        acc = fmaf(Gs[(4 * ty + i) * DP + tx + 16 * jj], o_base[(size_t)t * rso + tx + 16 * jj], acc);
    }
    dsum[i] = at_sum16(acc);
    const size_t li = ((size_t)(t < g.T ? t : 0) * g.n_pad + n) * g.heads + h;
    lse2[i] = lse[li] * AT_LOG2E;
    if (t < g.T && tx == 0) dvec[li] = dsum[i];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) dq[i][jj] = 0.f;
  }
  int kb = 0, ke = len, wlo[4], whi[4];     // as in the forward pass
  if constexpr (WIN) {
    at_win_keys(w, q0, g.T, len, &kb, &ke);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wlo[i] = at_win_lo(w, q0 + 4 * ty + i);
      whi[i] = min(at_win_hi(w, q0 + 4 * ty + i), len);
    }
  }
  for (int k0 = kb; k0 < ke; k0 += AT_TILE) {
    at_load_tile<DH>(Ks, base + D, rs, k0, len, tid);
    at_load_tile<DH>(Vs, base + 2 * D, rs, k0, len, tid);
    __syncthreads();
    float s[4][4], dp[4][4];
    at_dot<DH>(Qs, Ks, ty, tx, s);
    at_dot<DH>(Gs, Vs, ty, tx, dp);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int u = k0 + tx + 16 * j;
        bool vis = u < len;
        if constexpr (WIN) vis = u >= wlo[i] && u < whi[i];
        const float p = vis ? exp2f(fmaf(s[i][j], g.c2, -lse2[i])) : 0.f;
        s[i][j] = p * (dp[i][j] - dsum[i]) * g.scale;
      }
    at_put_tile(Ps, s, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Ks, ty, tx, dq);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = q0 + 4 * ty + i;
    if (t >= g.T) continue;
    float* row = dq_base + (size_t)t * rs + h * DH;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) row[tx + 16 * jj] = dq[i][jj];
  }
}

// backward pass 2: dK and dV of one key tile over all query tiles (query tiles ascending)
template <int DH, bool WIN>
__global__ __launch_bounds__(AT_THREADS) void attn_bwd_dkv_kernel(
    const float* __restrict__ qkv, const int* __restrict__ lens, const float* __restrict__ lse,
    const float* __restrict__ dout, float* __restrict__ dqkv, const float* __restrict__ dvec,
    AtGeo g, asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 at_lds4[];
  float* Ks = reinterpret_cast<float*>(at_lds4);
  float* Vs = Ks + AT_TILE * DP;
  float* Qs = Vs + AT_TILE * DP;
  float* Gs = Qs + AT_TILE * DP;            // dO tile
  float* Ps = Gs + AT_TILE * DP;
  float* Ls = Ps + AT_TILE * AT_PP;         // lse (base 2) of the query tile
  float* Ds = Ls + AT_TILE;                 // D of the query tile
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int k0 = blockIdx.x * AT_TILE, h = blockIdx.y, n = blockIdx.z;
  const int D = g.heads * DH;
  const size_t rs = (size_t)g.n_pad * g.ld, rso = (size_t)g.n_pad * g.ld_out;
  float* d_base = dqkv + (size_t)n * g.ld;
  if (h == 0) at_zero_cols(d_base, rs, k0, g.T, 3 * D, g.ld - 3 * D, tid);
  const int len = n < g.N ? at_len(lens, n, g.T) : 0;
  if (k0 >= len) {          // a padding sample, or a tile of masked keys only
    at_zero_cols(d_base, rs, k0, g.T, D + h * DH, DH, tid);
    at_zero_cols(d_base, rs, k0, g.T, 2 * D + h * DH, DH, tid);
    return;
  }
  const float* base = qkv + (size_t)n * g.ld + h * DH;
  const float* do_base = dout + (size_t)n * g.ld_out + h * DH;
  at_load_tile<DH>(Ks, base + D, rs, k0, len, tid);
  at_load_tile<DH>(Vs, base + 2 * D, rs, k0, len, tid);
  float dk[4][NJ], dv[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) dk[i][jj] = dv[i][jj] = 0.f;
  for (int q0 = 0; q0 < g.T; q0 += AT_TILE) {
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
    at_load_tile<DH>(Qs, base, rs, q0, g.T, tid);
    at_load_tile<DH>(Gs, do_base, rso, q0, g.T, tid);
    if (tid < AT_TILE) {
      const int t = q0 + tid;
      const size_t li = ((size_t)(t < g.T ? t : 0) * g.n_pad + n) * g.heads + h;
      Ls[tid] = lse[li] * AT_LOG2E;
      Ds[tid] = dvec[li];
    }
    __syncthreads();
    float s[4][4], dp[4][4];
    at_dot<DH>(Ks, Qs, ty, tx, s);          // s[i][j]: key 4 ty + i, query tx + 16 j
    at_dot<DH>(Vs, Gs, ty, tx, dp);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = tx + 16 * j;
        bool live = (k0 + 4 * ty + i < len) && (q0 + q < g.T);
        if constexpr (WIN) live = live && k0 + 4 * ty + i >= qlo[j] && k0 + 4 * ty + i < qhi[j];
        s[i][j] = live ? exp2f(fmaf(s[i][j], g.c2, -Ls[q])) : 0.f;
        dp[i][j] = s[i][j] * (dp[i][j] - Ds[q]) * g.scale;
      }
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
    if (u >= g.T) continue;
    float* row = d_base + (size_t)u * rs + h * DH;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {       // (rows u >= len accumulated p = 0 only: exact zeros)
      row[D + tx + 16 * jj] = dk[i][jj];
      row[2 * D + tx + 16 * jj] = dv[i][jj];
    }
  }
}

__global__ __launch_bounds__(256) void posenc_add_kernel(const float* __restrict__ x,
                                                        const float* __restrict__ pe,
                                                        float* __restrict__ y, long long total,
                                                        int N, int n_pad, int D, int ld) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int f = (int)(e % ld);
    const long long row = e / ld;
    const int n = (int)(row % n_pad);
    const long long t = row / n_pad;
    y[e] = (n < N && f < D) ? x[e] + pe[t * D + f] : 0.f;
  }
}

bool at_geo_ok(const asr_attn_args* a) {
  if (a == nullptr || a->T < 1 || a->N < 1 || a->n_pad < a->N || a->n_pad > 65535) return false;
  if (a->heads < 1 || a->heads > 65535 || a->dh < 16 || a->dh > 128 || (a->dh & 15)) return false;
  const long long D = (long long)a->heads * a->dh;
  if ((a->ld & 3) || a->ld < 3 * D || (a->ld_out & 3) || a->ld_out < D) return false;
  return a->scale > 0.f && a->scale < 1e30f;
}

size_t at_lds_bytes(int dh, int backward) {
  const size_t tile = (size_t)AT_TILE * (dh + 4) * sizeof(float);
  const size_t p = (size_t)AT_TILE * AT_PP * sizeof(float);
  return backward ? 4 * tile + p + 2 * AT_TILE * sizeof(float) : 3 * tile + p;
}

AtGeo at_geo(const asr_attn_args* a) {
  AtGeo g;
  g.T = a->T, g.N = a->N, g.n_pad = a->n_pad, g.heads = a->heads, g.ld = a->ld;
  g.ld_out = a->ld_out, g.scale = a->scale, g.c2 = a->scale * AT_LOG2E;
  return g;
}

}  // namespace

#define AT_DISPATCH(LAUNCH)                         \
  switch (a->dh) {                                  \
    case 16: LAUNCH(16); break;                     \
    case 32: LAUNCH(32); break;                     \
    case 48: LAUNCH(48); break;                     \
    case 64: LAUNCH(64); break;                     \
    case 80: LAUNCH(80); break;                     \
    case 96: LAUNCH(96); break;                     \
    case 112: LAUNCH(112); break;                   \
    default: LAUNCH(128); break;                    \
  }

extern "C" size_t asr_attn_workspace_bytes(const asr_attn_args* a) {
  if (!at_geo_ok(a)) return 0;
  return asr_align_up((size_t)a->T * a->n_pad * a->heads * sizeof(float), 256);
}

extern "C" int asr_attn_plan(const asr_attn_args* a, int backward, int* bq, int* bk, int* blocks,
                             int* lds_bytes) {
  ASR_CHECK_ARG(at_geo_ok(a), "attn_plan: bad geometry (dh a multiple of 16 in 16..128, heads "
                              ">= 1, ld >= 3 heads dh, ld_out >= heads dh, both multiples of 4)");
  if (bq) *bq = AT_TILE;
  if (bk) *bk = AT_TILE;
  if (blocks) *blocks = (a->T + AT_TILE - 1) / AT_TILE * a->heads * a->n_pad;
  if (lds_bytes) *lds_bytes = (int)at_lds_bytes(a->dh, backward);
  return ASR_OK;
}

#define AT_WIN_TEXT "chunk >= 1, left >= -1 (-1: unlimited), right >= 0"

extern "C" int asr_attn_win_plan(const asr_attn_args* a, const asr_attn_window* w, int backward,
                                 int* bq, int* bk, int* blocks, int* lds_bytes,
                                 long long* tile_pairs) {
  ASR_CHECK_ARG(at_win_ok(w), "attn_win_plan: bad window (" AT_WIN_TEXT ")");
  const int rc = asr_attn_plan(a, backward, bq, bk, blocks, lds_bytes);
  if (rc == ASR_OK && tile_pairs) *tile_pairs = at_win_tile_pairs(*w, a->T);
  return rc;
}

// w == nullptr: the unwindowed kernels
static int at_fwd(const asr_attn_args* a, const asr_attn_window* w, asr_stream_t stream) {
  ASR_CHECK_ARG(at_geo_ok(a), "attn_fwd: bad geometry (T %d N %d n_pad %d heads %d dh %d ld %d "
                "ld_out %d; dh a multiple of 16 in 16..128, ld >= 3 heads dh, ld_out >= heads dh, "
                "both multiples of 4)", a ? a->T : 0, a ? a->N : 0, a ? a->n_pad : 0,
                a ? a->heads : 0, a ? a->dh : 0, a ? a->ld : 0, a ? a->ld_out : 0);
  ASR_CHECK_ARG(a->qkv && a->out && a->out != a->qkv, "attn_fwd: qkv and out are required");
  ASR_CHECK_ARG(at_aligned(a->qkv) && at_aligned(a->out), "attn_fwd: qkv, out 16-byte aligned");
  const AtGeo g = at_geo(a);
  const dim3 grid((a->T + AT_TILE - 1) / AT_TILE, a->heads, a->n_pad);
  const size_t lds = at_lds_bytes(a->dh, 0);
  const asr_attn_window win = w ? *w : asr_attn_window{1, -1, 0};
#define AT_FWD_W(DH, WIN)                                                                       \
  {                                                                                             \
    if (at_allow_lds(attn_fwd_kernel<DH, WIN>, lds) != ASR_OK) return ASR_ERR_LAUNCH;           \
    hipLaunchKernelGGL((attn_fwd_kernel<DH, WIN>), grid, dim3(AT_THREADS), lds,                 \
                       (hipStream_t)stream, a->qkv, a->lens, a->out, a->lse, g, win);           \
  }
#define AT_FWD(DH) \
  if (w) AT_FWD_W(DH, true) else AT_FWD_W(DH, false)
  AT_DISPATCH(AT_FWD)
#undef AT_FWD
#undef AT_FWD_W
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_attn_fwd(const asr_attn_args* a, asr_stream_t stream) {
  return at_fwd(a, nullptr, stream);
}

extern "C" int asr_attn_win_fwd(const asr_attn_args* a, const asr_attn_window* w,
                                asr_stream_t stream) {
  ASR_CHECK_ARG(at_win_ok(w), "attn_win_fwd: bad window (" AT_WIN_TEXT ")");
  return at_fwd(a, w, stream);
}

static int at_bwd(const asr_attn_args* a, const asr_attn_window* w, void* workspace,
                  size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(at_geo_ok(a), "attn_bwd: bad geometry (T %d N %d n_pad %d heads %d dh %d ld %d "
                "ld_out %d)", a ? a->T : 0, a ? a->N : 0, a ? a->n_pad : 0, a ? a->heads : 0,
                a ? a->dh : 0, a ? a->ld : 0, a ? a->ld_out : 0);
  ASR_CHECK_ARG(a->qkv && a->out && a->lse && a->dout && a->dqkv && a->dqkv != a->qkv,
                "attn_bwd: qkv, out, lse, dout and dqkv are required");
  ASR_CHECK_ARG(at_aligned(a->qkv) && at_aligned(a->dout) && at_aligned(a->dqkv),
                "attn_bwd: qkv, dout, dqkv 16-byte aligned");
  const size_t need = asr_attn_workspace_bytes(a);
  if (workspace == nullptr || ws_bytes < need) {
    asr_set_error("attn_bwd: workspace too small (%zu bytes needed)", need);
    return ASR_ERR_WORKSPACE;
  }
  const AtGeo g = at_geo(a);
  float* dvec = (float*)workspace;
  const dim3 grid((a->T + AT_TILE - 1) / AT_TILE, a->heads, a->n_pad);
  const size_t lds = at_lds_bytes(a->dh, 1);
  hipStream_t s = (hipStream_t)stream;
  const asr_attn_window win = w ? *w : asr_attn_window{1, -1, 0};
#define AT_BWD_W(DH, WIN)                                                                       \
  {                                                                                             \
    if (at_allow_lds(attn_bwd_dq_kernel<DH, WIN>, lds) != ASR_OK) return ASR_ERR_LAUNCH;        \
    if (at_allow_lds(attn_bwd_dkv_kernel<DH, WIN>, lds) != ASR_OK) return ASR_ERR_LAUNCH;       \
    hipLaunchKernelGGL((attn_bwd_dq_kernel<DH, WIN>), grid, dim3(AT_THREADS), lds, s, a->qkv,   \
                       a->lens, a->out, a->lse, a->dout, a->dqkv, dvec, g, win);                \
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<DH, WIN>), grid, dim3(AT_THREADS), lds, s, a->qkv,  \
                       a->lens, a->lse, a->dout, a->dqkv, dvec, g, win);                        \
  }
#define AT_BWD(DH) \
  if (w) AT_BWD_W(DH, true) else AT_BWD_W(DH, false)
  AT_DISPATCH(AT_BWD)
#undef AT_BWD
#undef AT_BWD_W
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_attn_bwd(const asr_attn_args* a, void* workspace, size_t ws_bytes,
                            asr_stream_t stream) {
  return at_bwd(a, nullptr, workspace, ws_bytes, stream);
}

extern "C" int asr_attn_win_bwd(const asr_attn_args* a, const asr_attn_window* w, void* workspace,
                                size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(at_win_ok(w), "attn_win_bwd: bad window (" AT_WIN_TEXT ")");
  return at_bwd(a, w, workspace, ws_bytes, stream);
}

extern "C" int asr_attn_stream_plan(const asr_attn_window* w, int max_tq, int* ring_rows) {
  ASR_CHECK_ARG(at_stream_win_ok(w) && max_tq >= 1 && max_tq <= (1 << 20),
                "attn_stream_plan: bad window (chunk >= 1, left >= 0, right = 0) or max_tq %d",
                max_tq);
  if (ring_rows) *ring_rows = at_ring_rows(*w, max_tq);
  return ASR_OK;
}

extern "C" int asr_attn_stream_fwd(const asr_attn_stream_args* a, const asr_attn_window* w,
                                   asr_stream_t stream) {
  const char* bad = at_stream_bad(a, w, 128, false);
  ASR_CHECK_ARG(bad == nullptr, "attn_stream_fwd: %s", bad);
  AtsGeo g;
  g.Tq = a->Tq, g.N = a->N, g.n_pad = a->n_pad, g.heads = a->heads, g.ld = a->ld;
  g.ld_kv = a->ld_kv, g.ld_out = a->ld_out, g.R = a->R, g.t0 = a->t0;
  g.c2 = a->scale * AT_LOG2E;
  const dim3 grid((a->Tq + AT_TILE - 1) / AT_TILE, a->heads, a->n_pad);
  const size_t lds = at_lds_bytes(a->dh, 0);
#define AT_STREAM(DH)                                                                           \
  {                                                                                             \
    if (at_allow_lds(attn_stream_kernel<DH>, lds) != ASR_OK) return ASR_ERR_LAUNCH;             \
    hipLaunchKernelGGL((attn_stream_kernel<DH>), grid, dim3(AT_THREADS), lds,                   \
                       (hipStream_t)stream, a->q, a->ring, a->kv_len, a->out, g, *w);           \
  }
  AT_DISPATCH(AT_STREAM)
#undef AT_STREAM
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_posenc_add(const float* x, const float* pe, float* y, int T, int N, int n_pad,
                              int D, int ld, asr_stream_t stream) {
  ASR_CHECK_ARG(x && pe && y, "posenc_add: x, pe, y are required");
  ASR_CHECK_ARG(T >= 1 && N >= 1 && n_pad >= N && D >= 1 && ld >= D,
                "posenc_add: bad geometry (T %d N %d n_pad %d D %d ld %d)", T, N, n_pad, D, ld);
  const long long total = (long long)T * n_pad * ld;
  const long long want = (total + 255) / 256;
  const int blocks = (int)(want < 4096 ? want : 4096);
  hipLaunchKernelGGL(posenc_add_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, pe, y,
                     total, N, n_pad, D, ld);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
