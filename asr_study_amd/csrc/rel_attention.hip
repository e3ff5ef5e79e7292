// K24 relative positional multi-head self-attention core (Transformer-XL, arXiv 1901.02860 3.3,
// as the Conformer uses it, arXiv 2005.08100 2.1), forward and backward, fused.
//
// qkv, lens, out, lse, dout, dqkv are those of attention.hip.  pos is the projected relative
// table (2T - 1, ld_pos >= D): row r + T - 1 holds pos_r for the RELATIVE INDEX r = t - u, QUERY
// FRAME MINUS KEY FRAME (positive when the key lies in the past); head h reads columns
// h dh .. (h + 1) dh - 1.  bias_u, bias_v (D each) are the two position biases.  For every real
// sample n < N, head h and query frame t (all T frames are queries; only keys are masked):
//   s[t,u] = scale ((q_t + b_u) . k_u + (q_t + b_v) . pos_{t-u})   for u < lens[n]
//   p = softmax_u(s), out_t = sum_u p[t,u] v_u, lse_t = log sum_u exp s[t,u]
// Backward, with dS = P (.) (dO V^T - D_t), D_t = dout_t . out_t:
//   dq_t = scale sum_u dS[t,u] (k_u + pos_{t-u})      dk_u = scale sum_t dS[t,u] (q_t + b_u)
//   dv = P^T dO                                       db_u = scale sum_{n,t,u} dS[t,u] k_u
//   db_v = scale sum_{n,t,u} dS[t,u] pos_{t-u}
//   dpos_r = scale sum_n sum_{t-u=r, u<len_n} dS[t,u] (q_t + b_v)
// Masked keys get dK = dV = exactly 0; rows n >= N and pad columns are written as exact zeros;
// dpos rows no valid (t, u) pair reaches are exact zeros.
//
// ARITHMETIC and TILING are attention.hip's (attn_tile.h): exact fp32 FMAs, base-2
// exponentials, 64 x 64 score tiles in registers.  What is new is the BAND: for a query tile at
// t0 and a key tile at u0 the relative indices span 127 rows of pos, t0 - u0 - 63 .. t0 - u0 + 63.
// Those rows (128, the last unused) are staged in LDS, G = Q' Band^T (64 x 128) is computed with
// the same at_dot as the content term, two 64-row halves, and every element G[row][b] is WRITTEN
// to LDS at its key column col = row - b + 63 when that lies in the tile (a skew on the way in:
// the probability tile's buffer, pitch 68, is the target, and the read back is the plain
// row-major one of at_put_tile; half of G falls outside and is never stored).  The two biases
// are folded: the Q tile is staged as q + b_u (so the content product and dK see q + b_u), and
// the position product adds one scalar per band row, (b_v - b_u) . pos_b.  dh 16 .. 64: with the
// band (two more tiles) dh 80 .. 128 does not fit the 160 KB of a CU in the backward passes and
// is refused (ASR_ERR_INVALID).
//   forward:  grid (query tiles, heads, n_pad).
//   backward: (1) grid (query tiles, heads, n_pad): D, and dQ = dQ_c + dQ_p -- the content and
//                 position parts also go to two workspace slabs, whose column sums are db_u, db_v;
//             (2) grid (key tiles, heads, n_pad): dK, dV over all query tiles;
//             (3) grid (64-row tiles of the table, heads, N): per-sample partials of dpos in the
//                 workspace.  For a key tile the queries of a band tile form a window of 128
//                 frames starting at u0 + r0; it is walked as two 64-frame halves, in each of
//                 which one triangle of the 64 x 64 pairs belongs to the band tile.
//             then asr_colsum adds the partials over n in a fixed order and sums the two slabs.
// Every output element is written by exactly one thread in one fixed order: no float atomics,
// repeats are bit-identical; no workgroup waits on another one.
//
// K25, THE WINDOW (asr_relattn_win_*): the definition of attn_tile.h (key u visible to query t iff
// lo(t) <= u < hi(t) and u < lens[n]), the empty-row rule and the tile ranges of passes (1), (2)
// and the forward are attention.hip's.  Pass (3) applies the window in its `live` predicate and
// skips the (key tile, query half) pairs that hold no visible pair; a visible pair has t - u in
// [-(chunk - 1 + right), left + chunk - 1] (left unlimited: T - 1), so a table tile wholly outside
// that range writes zeros without a walk, and the rows outside it are exact zeros in any tile.
// dbias_u and dbias_v are column sums of the masked dQ parts.  "Window" names this mask; "band"
// stays the staged rows of the position table.  Templates on a bool: without the window the code
// above, bit for bit.
#include "attn_tile.h"

namespace {

constexpr int RA_MAX_DH = 64;
constexpr int RA_SMALL = 384;             // floats: cP / cK [128] | Ls [64] | Ds [64] | two vectors [128]

struct RaGeo {
  int T, N, n_pad, heads, ld, ld_out, ld_pos;
  float c2;         // scale * log2(e)
  float scale;
};

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

// WIN (here and below): under the window w of attn_tile.h (K25); without it w is not read and
// the code is the unwindowed kernel's.
template <int DH, bool WIN>
__global__ __launch_bounds__(AT_THREADS) void relattn_fwd_kernel(
    const float* __restrict__ qkv, const int* __restrict__ lens, const float* __restrict__ pos,
    const float* __restrict__ bias_u, const float* __restrict__ bias_v, float* __restrict__ out,
    float* __restrict__ lse, RaGeo g, asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 ra_lds4[];
  float* Qs = reinterpret_cast<float*>(ra_lds4);
  float* Ks = Qs + AT_TILE * DP;
  float* Vs = Ks + AT_TILE * DP;
  float* Bs = Vs + AT_TILE * DP;            // 128 band rows
  float* Ps = Bs + 2 * AT_TILE * DP;
  float* cP = Ps + AT_TILE * AT_PP;
  float* vu = cP + 256, *vd = vu + 64;
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
  const float* pos_h = pos + h * DH;
  const int len = at_len(lens, n, g.T);
  ra_load_bias<DH>(vu, vd, bias_u + h * DH, bias_v + h * DH, tid);
  __syncthreads();
  ra_load_rows<DH>(Qs, base, rs, q0, g.T, vu, tid);
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
    const int pr0 = q0 - k0 - 63 + g.T - 1;           // table row of band row 0
    at_load_tile<DH>(Ks, base + D, rs, k0, len, tid);
    at_load_tile<DH>(Vs, base + 2 * D, rs, k0, len, tid);
    ra_load_rows<DH>(Bs, pos_h, g.ld_pos, pr0, 2 * g.T - 1, nullptr, tid);
    ra_load_rows<DH>(Bs + AT_TILE * DP, pos_h, g.ld_pos, pr0 + 64, 2 * g.T - 1, nullptr, tid);
    __syncthreads();
    if (tid < 128) cP[tid] = ra_rowdot<DH>(Bs + tid * DP, vd);
    float s[4][4];
    at_dot<DH>(Qs, Ks, ty, tx, s);
    ra_band_scores<DH>(Qs, Bs, Ps, ty, tx);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * ty + i;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = tx + 16 * j;
        const float sp = Ps[row * AT_PP + col] + cP[row - col + 63];
        bool vis = k0 + col < len;
        if constexpr (WIN) vis = k0 + col >= wlo[i] && k0 + col < whi[i];
        s[i][j] = vis ? (s[i][j] + sp) * g.c2 : asr_neg_inf();
      }
    }
    at_softmax_tile<NJ, WIN>(s, m, l, o);
    __syncthreads();                        // (every G read before P overwrites it)
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

// K26, the streaming forward: attn_stream_kernel of attention.hip (Q from the chunk's slab, K and
// V from THE RING of attn_tile.h, the absolute 64-aligned key tiles of the whole-utterance call,
// kv_len for lens) with the relative term.  pos is a table of 2P - 1 rows, row r + P - 1 the
// relative index r, P >= left + chunk: it covers every visible pair (0 <= t - u <= left + chunk
// - 1) and does not depend on how long the stream runs.  Band rows outside the table are staged
// as zeros, here as in the whole-utterance call, and meet masked pairs only; a band element is one
// at_dot chain over a query row and a table row, wherever the rows sit in their tiles, so the
// rows come out bit for bit as from asr_relattn_win_fwd on the same projected table values.
struct RasGeo {
  int Tq, N, n_pad, heads, ld, ld_kv, ld_out, R, t0, P, ld_pos;
  float c2;         // scale * log2(e)
};

template <int DH>
__global__ __launch_bounds__(AT_THREADS) void relattn_stream_kernel(
    const float* __restrict__ q, const float* __restrict__ ring, const int* __restrict__ kv_len,
    const float* __restrict__ pos, const float* __restrict__ bias_u,
    const float* __restrict__ bias_v, float* __restrict__ out, RasGeo g, asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 ra_lds4[];
  float* Qs = reinterpret_cast<float*>(ra_lds4);
  float* Ks = Qs + AT_TILE * DP;
  float* Vs = Ks + AT_TILE * DP;
  float* Bs = Vs + AT_TILE * DP;            // 128 band rows
  float* Ps = Bs + 2 * AT_TILE * DP;
  float* cP = Ps + AT_TILE * AT_PP;
  float* vu = cP + 256, *vd = vu + 64;
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
  const float* pos_h = pos + h * DH;
  int len = kv_len[n];
  len = len < 1 ? 1 : (len > g.t0 + g.Tq ? g.t0 + g.Tq : len);      // (as at_len)
  ra_load_bias<DH>(vu, vd, bias_u + h * DH, bias_v + h * DH, tid);
  __syncthreads();
  ra_load_rows<DH>(Qs, q + (size_t)n * g.ld + h * DH, rs, r0, g.Tq, vu, tid);
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
    const int pr0 = qa - k0 - 63 + g.P - 1;           // table row of band row 0
    // (k0 and R are multiples of 64: the tile is 64 consecutive ring rows; rows >= len: zeros)
    const float* tile = kbase + (size_t)(k0 % g.R) * rsk;
    at_load_tile<DH>(Ks, tile, rsk, 0, len - k0, tid);
    at_load_tile<DH>(Vs, tile + D, rsk, 0, len - k0, tid);
    ra_load_rows<DH>(Bs, pos_h, g.ld_pos, pr0, 2 * g.P - 1, nullptr, tid);
    ra_load_rows<DH>(Bs + AT_TILE * DP, pos_h, g.ld_pos, pr0 + 64, 2 * g.P - 1, nullptr, tid);
    __syncthreads();
    if (tid < 128) cP[tid] = ra_rowdot<DH>(Bs + tid * DP, vd);
    float s[4][4];
    at_dot<DH>(Qs, Ks, ty, tx, s);
    ra_band_scores<DH>(Qs, Bs, Ps, ty, tx);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * ty + i;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = tx + 16 * j;
        const float sp = Ps[row * AT_PP + col] + cP[row - col + 63];
        const bool vis = k0 + col >= wlo[i] && k0 + col < whi[i];
        s[i][j] = vis ? (s[i][j] + sp) * g.c2 : asr_neg_inf();
      }
    }
    at_softmax_tile<NJ, true>(s, m, l, o);
    __syncthreads();                        // (every G read before P overwrites it)
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

// backward pass 1: D (to dvec), dQ = dQ_c + dQ_p; dQ_c -> slab_c, dQ_p -> slab_p (T, n_pad, D)
template <int DH, bool WIN>
__global__ __launch_bounds__(AT_THREADS) void relattn_bwd_dq_kernel(
    const float* __restrict__ qkv, const int* __restrict__ lens, const float* __restrict__ pos,
    const float* __restrict__ bias_u, const float* __restrict__ bias_v,
    const float* __restrict__ out, const float* __restrict__ lse, const float* __restrict__ dout,
    float* __restrict__ dqkv, float* __restrict__ dvec, float* __restrict__ slab_c,
    float* __restrict__ slab_p, RaGeo g, asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 ra_lds4[];
  float* Qs = reinterpret_cast<float*>(ra_lds4);
  float* Gs = Qs + AT_TILE * DP;            // dO tile
  float* Ks = Gs + AT_TILE * DP;
  float* Vs = Ks + AT_TILE * DP;
  float* Bs = Vs + AT_TILE * DP;            // 128 band rows
  float* Ps = Bs + 2 * AT_TILE * DP;
  float* P2 = Ps + AT_TILE * AT_PP;         // dS of one band half, columns = band rows
  float* cP = P2 + AT_TILE * AT_PP;
  float* vu = cP + 256, *vd = vu + 64;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int q0 = blockIdx.x * AT_TILE, h = blockIdx.y, n = blockIdx.z;
  const int D = g.heads * DH;
  const size_t rs = (size_t)g.n_pad * g.ld, rso = (size_t)g.n_pad * g.ld_out;
  const size_t rsd = (size_t)g.n_pad * D;
  float* dq_base = dqkv + (size_t)n * g.ld;
  float* sc_base = slab_c + (size_t)n * D + h * DH;
  float* sp_base = slab_p + (size_t)n * D + h * DH;
  if (n >= g.N) {
    at_zero_cols(dq_base, rs, q0, g.T, h * DH, DH, tid);
    at_zero_cols(sc_base, rsd, q0, g.T, 0, DH, tid);
    at_zero_cols(sp_base, rsd, q0, g.T, 0, DH, tid);
    return;
  }
  const float* base = qkv + (size_t)n * g.ld + h * DH;
  const float* do_base = dout + (size_t)n * g.ld_out + h * DH;
  const float* o_base = out + (size_t)n * g.ld_out + h * DH;
  const float* pos_h = pos + h * DH;
  const int len = at_len(lens, n, g.T);
  ra_load_bias<DH>(vu, vd, bias_u + h * DH, bias_v + h * DH, tid);
  __syncthreads();
  ra_load_rows<DH>(Qs, base, rs, q0, g.T, vu, tid);
  at_load_tile<DH>(Gs, do_base, rso, q0, g.T, tid);
  __syncthreads();
  float lse2[4], dsum[4], dqc[4][NJ], dqp[4][NJ];
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
    for (int jj = 0; jj < NJ; ++jj) dqc[i][jj] = dqp[i][jj] = 0.f;
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
    const int pr0 = q0 - k0 - 63 + g.T - 1;
    at_load_tile<DH>(Ks, base + D, rs, k0, len, tid);
    at_load_tile<DH>(Vs, base + 2 * D, rs, k0, len, tid);
    ra_load_rows<DH>(Bs, pos_h, g.ld_pos, pr0, 2 * g.T - 1, nullptr, tid);
    ra_load_rows<DH>(Bs + AT_TILE * DP, pos_h, g.ld_pos, pr0 + 64, 2 * g.T - 1, nullptr, tid);
    __syncthreads();
    if (tid < 128) cP[tid] = ra_rowdot<DH>(Bs + tid * DP, vd);
    float s[4][4], dp[4][4];
    at_dot<DH>(Qs, Ks, ty, tx, s);
    at_dot<DH>(Gs, Vs, ty, tx, dp);
    ra_band_scores<DH>(Qs, Bs, Ps, ty, tx);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = 4 * ty + i, col = tx + 16 * j;
        const float st = s[i][j] + (Ps[row * AT_PP + col] + cP[row - col + 63]);
        bool vis = k0 + col < len;
        if constexpr (WIN) vis = k0 + col >= wlo[i] && k0 + col < whi[i];
        const float p = vis ? exp2f(fmaf(st, g.c2, -lse2[i])) : 0.f;
        s[i][j] = p * (dp[i][j] - dsum[i]) * g.scale;
      }
    __syncthreads();
    at_put_tile(Ps, s, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Ks, ty, tx, dqc);
#pragma unroll 1
    for (int hf = 0; hf < 2; ++hf) {        // dQ_p += dG_half Band_half, dG[row][b] = dS[row][row - b + 63]
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
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int t = q0 + 4 * ty + i;
    if (t >= g.T) continue;
    float* row = dq_base + (size_t)t * rs + h * DH;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
      row[tx + 16 * jj] = dqc[i][jj] + dqp[i][jj];
      sc_base[(size_t)t * rsd + tx + 16 * jj] = dqc[i][jj];
      sp_base[(size_t)t * rsd + tx + 16 * jj] = dqp[i][jj];
    }
  }
}

// backward pass 2: dK and dV of one key tile over all query tiles (query tiles ascending)
template <int DH, bool WIN>
__global__ __launch_bounds__(AT_THREADS) void relattn_bwd_dkv_kernel(
    const float* __restrict__ qkv, const int* __restrict__ lens, const float* __restrict__ pos,
    const float* __restrict__ bias_u, const float* __restrict__ bias_v,
    const float* __restrict__ lse, const float* __restrict__ dout, float* __restrict__ dqkv,
    const float* __restrict__ dvec, RaGeo g, asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 ra_lds4[];
  float* Ks = reinterpret_cast<float*>(ra_lds4);
  float* Vs = Ks + AT_TILE * DP;
  float* Qs = Vs + AT_TILE * DP;
  float* Gs = Qs + AT_TILE * DP;            // dO tile
  float* Bs = Gs + AT_TILE * DP;            // 128 band rows
  float* Ps = Bs + 2 * AT_TILE * DP;
  float* cP = Ps + AT_TILE * AT_PP;
  float* Ls = cP + 128;                     // lse (base 2) of the query tile
  float* Ds = Ls + AT_TILE;                 // D of the query tile
  float* vu = Ds + AT_TILE, *vd = vu + 64;
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
  const float* pos_h = pos + h * DH;
  ra_load_bias<DH>(vu, vd, bias_u + h * DH, bias_v + h * DH, tid);
  at_load_tile<DH>(Ks, base + D, rs, k0, len, tid);
  at_load_tile<DH>(Vs, base + 2 * D, rs, k0, len, tid);
  __syncthreads();
  float dk[4][NJ], dv[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) dk[i][jj] = dv[i][jj] = 0.f;
  for (int q0 = 0; q0 < g.T; q0 += AT_TILE) {
    int qlo[4], qhi[4];                     // the visible keys of query tx + 16 j
    if constexpr (WIN) {
      // only the query tiles that see a key of this tile: one contiguous range
      if (!at_win_pair(w, q0, min(q0 + AT_TILE, g.T) - 1, k0)) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        qlo[j] = at_win_lo(w, q0 + tx + 16 * j);
        qhi[j] = at_win_hi(w, q0 + tx + 16 * j);
      }
    }
    const int pr0 = q0 - k0 - 63 + g.T - 1;
    ra_load_rows<DH>(Qs, base, rs, q0, g.T, vu, tid);
    at_load_tile<DH>(Gs, do_base, rso, q0, g.T, tid);
    ra_load_rows<DH>(Bs, pos_h, g.ld_pos, pr0, 2 * g.T - 1, nullptr, tid);
    ra_load_rows<DH>(Bs + AT_TILE * DP, pos_h, g.ld_pos, pr0 + 64, 2 * g.T - 1, nullptr, tid);
    if (tid < AT_TILE) {
      const int t = q0 + tid;
      const size_t li = ((size_t)(t < g.T ? t : 0) * g.n_pad + n) * g.heads + h;
      Ls[tid] = lse[li] * AT_LOG2E;
      Ds[tid] = dvec[li];
    }
    __syncthreads();
    if (tid < 128) cP[tid] = ra_rowdot<DH>(Bs + tid * DP, vd);
    float s[4][4], dp[4][4];
    at_dot<DH>(Ks, Qs, ty, tx, s);          // s[i][j]: key 4 ty + i, query tx + 16 j
    at_dot<DH>(Vs, Gs, ty, tx, dp);
#pragma unroll 1
    for (int hf = 0; hf < 2; ++hf) {        // G^T: band row 64 hf + 4 ty + i, query tx + 16 j
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
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = tx + 16 * j, kk = 4 * ty + i;
        bool live = (k0 + kk < len) && (q0 + q < g.T);
        if constexpr (WIN) live = live && k0 + kk >= qlo[j] && k0 + kk < qhi[j];
        const float st = s[i][j] + (Ps[kk * AT_PP + q] + cP[q - kk + 63]);
        s[i][j] = live ? exp2f(fmaf(st, g.c2, -Ls[q])) : 0.f;
        dp[i][j] = s[i][j] * (dp[i][j] - Ds[q]) * g.scale;
      }
    __syncthreads();
    at_put_tile(Ps, s, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Gs, ty, tx, dv);
    __syncthreads();
    at_put_tile(Ps, dp, ty, tx);
    __syncthreads();
    at_acc<DH>(Ps, Qs, ty, tx, dk);         // Qs holds q + b_u
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

// backward pass 3: the partial of sample n of the table rows [64 m, 64 m + 64), i.e. the relative
// indices r0 + b with r0 = 64 m - (T - 1); part is (N, 2T - 1, ld_pos)
template <int DH, bool WIN>
__global__ __launch_bounds__(AT_THREADS) void relattn_bwd_dpos_kernel(
    const float* __restrict__ qkv, const int* __restrict__ lens, const float* __restrict__ pos,
    const float* __restrict__ bias_u, const float* __restrict__ bias_v,
    const float* __restrict__ lse, const float* __restrict__ dout, const float* __restrict__ dvec,
    float* __restrict__ part, RaGeo g, asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 ra_lds4[];
  float* Bs = reinterpret_cast<float*>(ra_lds4);   // the 64 rows of this band tile
  float* Ks = Bs + AT_TILE * DP;
  float* Vs = Ks + AT_TILE * DP;
  float* Qs = Vs + AT_TILE * DP;            // q + b_v
  float* Gs = Qs + AT_TILE * DP;            // dO tile
  float* Ps = Gs + AT_TILE * DP;
  float* cK = Ps + AT_TILE * AT_PP;
  float* Ls = cK + 128;
  float* Ds = Ls + AT_TILE;
  float* vv = Ds + AT_TILE, *vd = vv + 64;  // b_v, b_u - b_v
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int m0 = blockIdx.x * AT_TILE, h = blockIdx.y, n = blockIdx.z;
  const int D = g.heads * DH, rows = 2 * g.T - 1;
  const int r0 = m0 - (g.T - 1);
  const size_t rs = (size_t)g.n_pad * g.ld, rso = (size_t)g.n_pad * g.ld_out;
  float* p_base = part + (size_t)n * rows * g.ld_pos;
  if (h == 0) at_zero_cols(p_base, g.ld_pos, m0, rows, D, g.ld_pos - D, tid);
  const float* base = qkv + (size_t)n * g.ld + h * DH;
  const float* do_base = dout + (size_t)n * g.ld_out + h * DH;
  const int len = at_len(lens, n, g.T);
  ra_load_bias<DH>(vv, vd, bias_v + h * DH, bias_u + h * DH, tid);
  ra_load_rows<DH>(Bs, pos + h * DH, g.ld_pos, m0, rows, nullptr, tid);
  __syncthreads();
  float acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) acc[i][jj] = 0.f;
  // under a window a pair (t, u) is visible only for t - u in [-(chunk - 1 + right), left + chunk
  // - 1] (left unlimited: T - 1): a table tile wholly outside that range is all zeros, no walk
  bool dead = false;
  if constexpr (WIN)
    dead = r0 + AT_TILE - 1 + (long long)w.chunk - 1 + w.right < 0 ||
           (w.left >= 0 && r0 + 1 > (long long)w.left + w.chunk);
  for (int k0 = 0; !dead && k0 < len; k0 += AT_TILE) {
    // the queries t = u + r of this key tile and band tile: a window of 128 frames from k0 + r0
    if (k0 + r0 + 127 < 0 || k0 + r0 >= g.T) continue;
    at_load_tile<DH>(Ks, base + D, rs, k0, len, tid);
    at_load_tile<DH>(Vs, base + 2 * D, rs, k0, len, tid);
#pragma unroll 1
    for (int hf = 0; hf < 2; ++hf) {
      const int tw = k0 + r0 + 64 * hf;
      if (tw + 63 < 0 || tw >= g.T) continue;
      int wlo[4], whi[4];                   // the visible keys of query tw + 4 ty + i
      if constexpr (WIN) {
        if (!at_win_pair(w, max(tw, 0), min(tw + AT_TILE, g.T) - 1, k0)) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          wlo[i] = at_win_lo(w, max(tw + 4 * ty + i, 0));
          whi[i] = at_win_hi(w, max(tw + 4 * ty + i, 0));
        }
      }
      ra_load_rows<DH>(Qs, base, rs, tw, g.T, vv, tid);
      ra_load_rows<DH>(Gs, do_base, rso, tw, g.T, nullptr, tid);
      if (tid < AT_TILE) {
        const int t = tw + tid;
        const bool in = t >= 0 && t < g.T;
        const size_t li = ((size_t)(in ? t : 0) * g.n_pad + n) * g.heads + h;
        Ls[tid] = in ? lse[li] * AT_LOG2E : 0.f;
        Ds[tid] = in ? dvec[li] : 0.f;
      }
      __syncthreads();
      if (tid < AT_TILE) cK[tid] = ra_rowdot<DH>(Ks + tid * DP, vd);
      float s[4][4], dp[4][4];
      at_dot<DH>(Qs, Ks, ty, tx, s);        // s[i][j]: query tw + 4 ty + i, key k0 + tx + 16 j
      at_dot<DH>(Gs, Vs, ty, tx, dp);
      {
        float gq[4][4];                     // query 4 ty + i, band row tx + 16 j
        at_dot<DH>(Qs, Bs, ty, tx, gq);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = 4 * ty + i, kk = 64 * hf + q - (tx + 16 * j);
            if (kk >= 0 && kk < AT_TILE) Ps[q * AT_PP + kk] = gq[i][j];
          }
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q = 4 * ty + i, kk = tx + 16 * j, b = 64 * hf + q - kk;
          bool live = b >= 0 && b < AT_TILE && k0 + kk < len && tw + q >= 0 && tw + q < g.T;
          if constexpr (WIN) live = live && k0 + kk >= wlo[i] && k0 + kk < whi[i];
          const float st = s[i][j] + (Ps[q * AT_PP + kk] + cK[kk]);
          const float p = live ? exp2f(fmaf(st, g.c2, -Ls[q])) : 0.f;
          s[i][j] = p * (dp[i][j] - Ds[q]) * g.scale;
        }
      __syncthreads();
      // dG^T: band row b, query q; the pairs outside the band tile fill the other triangle with 0
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q = 4 * ty + i, kk = tx + 16 * j, b = 64 * hf + q - kk;
          const bool in = b >= 0 && b < AT_TILE;
          Ps[(in ? b : kk) * AT_PP + q] = in ? s[i][j] : 0.f;
        }
      __syncthreads();
      at_acc<DH>(Ps, Qs, ty, tx, acc);      // acc[band row 4 ty + i] += dG^T (q + b_v)
      __syncthreads();
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = m0 + 4 * ty + i;
    if (r >= rows) continue;
    float* row = p_base + (size_t)r * g.ld_pos + h * DH;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) row[tx + 16 * jj] = acc[i][jj];
  }
}

bool ra_geo_ok(const asr_relattn_args* a) {
  if (a == nullptr || a->T < 1 || a->N < 1 || a->n_pad < a->N || a->n_pad > 65535) return false;
  if (a->heads < 1 || a->heads > 65535 || a->dh < 16 || a->dh > RA_MAX_DH || (a->dh & 15))
    return false;
  const long long D = (long long)a->heads * a->dh;
  if ((a->ld & 3) || a->ld < 3 * D || (a->ld_out & 3) || a->ld_out < D) return false;
  if ((a->ld_pos & 3) || a->ld_pos < D) return false;
  if ((2LL * a->T - 1) * a->ld_pos > 0x7fffffffLL || (long long)a->T * a->n_pad > 0x7fffffffLL)
    return false;
  return a->scale > 0.f && a->scale < 1e30f;
}

// pass: 0 forward, 1 dQ, 2 dK / dV, 3 dpos
size_t ra_lds_bytes(int dh, int pass) {
  const size_t tile = (size_t)AT_TILE * (dh + 4) * sizeof(float);
  const size_t p = (size_t)AT_TILE * AT_PP * sizeof(float);
  const size_t small = RA_SMALL * sizeof(float);
  switch (pass) {
    case 0: return 5 * tile + p + small;
    case 1: return 6 * tile + 2 * p + small;
    case 2: return 6 * tile + p + small;
    default: return 5 * tile + p + small;
  }
}

struct RaWs {
  size_t dvec, slab_c, slab_p, part, colsum, colsum_bytes, end;
};

RaWs ra_ws(const asr_relattn_args* a) {
  RaWs w;
  const size_t D = (size_t)a->heads * a->dh, rows = (size_t)a->T * a->n_pad;
  const size_t pcols = (size_t)(2 * a->T - 1) * a->ld_pos;
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t o = off;
    off += asr_align_up(bytes, 256);
    return o;
  };
  w.dvec = take(rows * a->heads * sizeof(float));
  w.slab_c = take(rows * D * sizeof(float));
  w.slab_p = take(rows * D * sizeof(float));
  w.part = take((size_t)a->N * pcols * sizeof(float));
  const size_t c1 = asr_colsum_workspace_bytes((int)rows, (int)D);
  const size_t c2 = asr_colsum_workspace_bytes(a->N, (int)pcols);
  w.colsum_bytes = c1 > c2 ? c1 : c2;
  w.colsum = take(w.colsum_bytes);
  w.end = off;
  return w;
}

RaGeo ra_geo(const asr_relattn_args* a) {
  RaGeo g;
  g.T = a->T, g.N = a->N, g.n_pad = a->n_pad, g.heads = a->heads, g.ld = a->ld;
  g.ld_out = a->ld_out, g.ld_pos = a->ld_pos, g.scale = a->scale, g.c2 = a->scale * AT_LOG2E;
  return g;
}

}  // namespace

#define RA_GEO_TEXT "dh a multiple of 16 in 16..64 (the band tiles of the relative term leave " \
                    "no room in LDS for dh 80..128), heads >= 1, ld >= 3 heads dh, ld_out >= "   \
                    "heads dh, ld_pos >= heads dh, all multiples of 4"

#define RA_DISPATCH(LAUNCH)                         \
  switch (a->dh) {                                  \
    case 16: LAUNCH(16); break;                     \
    case 32: LAUNCH(32); break;                     \
    case 48: LAUNCH(48); break;                     \
    default: LAUNCH(64); break;                     \
  }

extern "C" size_t asr_relattn_workspace_bytes(const asr_relattn_args* a) {
  if (!ra_geo_ok(a)) return 0;
  return ra_ws(a).end;
}

extern "C" int asr_relattn_plan(const asr_relattn_args* a, int backward, int* bq, int* bk,
                                int* blocks, int* lds_bytes) {
  ASR_CHECK_ARG(ra_geo_ok(a), "relattn_plan: bad geometry (" RA_GEO_TEXT ")");
  if (bq) *bq = AT_TILE;
  if (bk) *bk = AT_TILE;
  if (blocks) *blocks = (a->T + AT_TILE - 1) / AT_TILE * a->heads * a->n_pad;
  if (lds_bytes) {
    size_t lds = backward ? 0 : ra_lds_bytes(a->dh, 0);     // backward: the largest pass
    for (int pass = 1; backward && pass <= 3; ++pass)
      if (ra_lds_bytes(a->dh, pass) > lds) lds = ra_lds_bytes(a->dh, pass);
    *lds_bytes = (int)lds;
  }
  return ASR_OK;
}

#define RA_WIN_TEXT "chunk >= 1, left >= -1 (-1: unlimited), right >= 0"

extern "C" int asr_relattn_win_plan(const asr_relattn_args* a, const asr_attn_window* w,
                                    int backward, int* bq, int* bk, int* blocks, int* lds_bytes,
                                    long long* tile_pairs) {
  ASR_CHECK_ARG(at_win_ok(w), "relattn_win_plan: bad window (" RA_WIN_TEXT ")");
  const int rc = asr_relattn_plan(a, backward, bq, bk, blocks, lds_bytes);
  if (rc == ASR_OK && tile_pairs) *tile_pairs = at_win_tile_pairs(*w, a->T);
  return rc;
}

// w == nullptr: the unwindowed kernels
static int ra_fwd(const asr_relattn_args* a, const asr_attn_window* w, asr_stream_t stream) {
  ASR_CHECK_ARG(ra_geo_ok(a), "relattn_fwd: bad geometry (T %d N %d n_pad %d heads %d dh %d ld %d "
                "ld_out %d ld_pos %d; " RA_GEO_TEXT ")", a ? a->T : 0, a ? a->N : 0,
                a ? a->n_pad : 0, a ? a->heads : 0, a ? a->dh : 0, a ? a->ld : 0,
                a ? a->ld_out : 0, a ? a->ld_pos : 0);
  ASR_CHECK_ARG(a->qkv && a->out && a->out != a->qkv && a->pos && a->bias_u && a->bias_v,
                "relattn_fwd: qkv, out, pos, bias_u and bias_v are required");
  ASR_CHECK_ARG(at_aligned(a->qkv) && at_aligned(a->out) && at_aligned(a->pos),
                "relattn_fwd: qkv, out, pos 16-byte aligned");
  const RaGeo g = ra_geo(a);
  const dim3 grid((a->T + AT_TILE - 1) / AT_TILE, a->heads, a->n_pad);
  const size_t lds = ra_lds_bytes(a->dh, 0);
  const asr_attn_window win = w ? *w : asr_attn_window{1, -1, 0};
#define RA_FWD_W(DH, WIN)                                                                       \
  {                                                                                             \
    if (at_allow_lds(relattn_fwd_kernel<DH, WIN>, lds) != ASR_OK) return ASR_ERR_LAUNCH;        \
    hipLaunchKernelGGL((relattn_fwd_kernel<DH, WIN>), grid, dim3(AT_THREADS), lds,              \
                       (hipStream_t)stream, a->qkv, a->lens, a->pos, a->bias_u, a->bias_v,      \
                       a->out, a->lse, g, win);                                                 \
  }
#define RA_FWD(DH) \
  if (w) RA_FWD_W(DH, true) else RA_FWD_W(DH, false)
  RA_DISPATCH(RA_FWD)
#undef RA_FWD
#undef RA_FWD_W
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_relattn_fwd(const asr_relattn_args* a, asr_stream_t stream) {
  return ra_fwd(a, nullptr, stream);
}

extern "C" int asr_relattn_win_fwd(const asr_relattn_args* a, const asr_attn_window* w,
                                   asr_stream_t stream) {
  ASR_CHECK_ARG(at_win_ok(w), "relattn_win_fwd: bad window (" RA_WIN_TEXT ")");
  return ra_fwd(a, w, stream);
}

extern "C" int asr_relattn_stream_fwd(const asr_attn_stream_args* a, const asr_attn_window* w,
                                      asr_stream_t stream) {
  const char* bad = at_stream_bad(a, w, RA_MAX_DH, true);
  ASR_CHECK_ARG(bad == nullptr, "relattn_stream_fwd: %s", bad);
  RasGeo g;
  g.Tq = a->Tq, g.N = a->N, g.n_pad = a->n_pad, g.heads = a->heads, g.ld = a->ld;
  g.ld_kv = a->ld_kv, g.ld_out = a->ld_out, g.R = a->R, g.t0 = a->t0, g.P = a->P;
  g.ld_pos = a->ld_pos, g.c2 = a->scale * AT_LOG2E;
  const dim3 grid((a->Tq + AT_TILE - 1) / AT_TILE, a->heads, a->n_pad);
  const size_t lds = ra_lds_bytes(a->dh, 0);
#define RA_STREAM(DH)                                                                           \
  {                                                                                             \
    if (at_allow_lds(relattn_stream_kernel<DH>, lds) != ASR_OK) return ASR_ERR_LAUNCH;          \
    hipLaunchKernelGGL((relattn_stream_kernel<DH>), grid, dim3(AT_THREADS), lds,                \
                       (hipStream_t)stream, a->q, a->ring, a->kv_len, a->pos, a->bias_u,        \
                       a->bias_v, a->out, g, *w);                                               \
  }
  RA_DISPATCH(RA_STREAM)
#undef RA_STREAM
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

static int ra_bwd(const asr_relattn_args* a, const asr_attn_window* wp, void* workspace,
                  size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(ra_geo_ok(a), "relattn_bwd: bad geometry (T %d N %d n_pad %d heads %d dh %d ld %d "
                "ld_out %d ld_pos %d; " RA_GEO_TEXT ")", a ? a->T : 0, a ? a->N : 0,
                a ? a->n_pad : 0, a ? a->heads : 0, a ? a->dh : 0, a ? a->ld : 0,
                a ? a->ld_out : 0, a ? a->ld_pos : 0);
  ASR_CHECK_ARG(a->qkv && a->out && a->lse && a->dout && a->dqkv && a->dqkv != a->qkv && a->pos &&
                a->bias_u && a->bias_v && a->dpos && a->dbias_u && a->dbias_v,
                "relattn_bwd: qkv, out, lse, dout, dqkv, pos, bias_u, bias_v, dpos, dbias_u and "
                "dbias_v are required");
  ASR_CHECK_ARG(at_aligned(a->qkv) && at_aligned(a->dout) && at_aligned(a->dqkv) &&
                at_aligned(a->pos), "relattn_bwd: qkv, dout, dqkv, pos 16-byte aligned");
  const RaWs w = ra_ws(a);
  if (workspace == nullptr || ws_bytes < w.end) {
    asr_set_error("relattn_bwd: workspace too small (%zu bytes needed)", w.end);
    return ASR_ERR_WORKSPACE;
  }
  const RaGeo g = ra_geo(a);
  char* ws = (char*)workspace;
  float* dvec = (float*)(ws + w.dvec);
  float* slab_c = (float*)(ws + w.slab_c);
  float* slab_p = (float*)(ws + w.slab_p);
  float* part = (float*)(ws + w.part);
  const int tiles = (a->T + AT_TILE - 1) / AT_TILE, rows = 2 * a->T - 1;
  const dim3 grid(tiles, a->heads, a->n_pad);
  const dim3 grid_pos((rows + AT_TILE - 1) / AT_TILE, a->heads, a->N);
  const size_t lds1 = ra_lds_bytes(a->dh, 1), lds2 = ra_lds_bytes(a->dh, 2);
  const size_t lds3 = ra_lds_bytes(a->dh, 3);
  hipStream_t s = (hipStream_t)stream;
  const asr_attn_window win = wp ? *wp : asr_attn_window{1, -1, 0};
#define RA_BWD_W(DH, WIN)                                                                        \
  {                                                                                              \
    if (at_allow_lds(relattn_bwd_dq_kernel<DH, WIN>, lds1) != ASR_OK) return ASR_ERR_LAUNCH;     \
    if (at_allow_lds(relattn_bwd_dkv_kernel<DH, WIN>, lds2) != ASR_OK) return ASR_ERR_LAUNCH;    \
    if (at_allow_lds(relattn_bwd_dpos_kernel<DH, WIN>, lds3) != ASR_OK) return ASR_ERR_LAUNCH;   \
    hipLaunchKernelGGL((relattn_bwd_dq_kernel<DH, WIN>), grid, dim3(AT_THREADS), lds1, s,        \
                       a->qkv, a->lens, a->pos, a->bias_u, a->bias_v, a->out, a->lse, a->dout,   \
                       a->dqkv, dvec, slab_c, slab_p, g, win);                                   \
    hipLaunchKernelGGL((relattn_bwd_dkv_kernel<DH, WIN>), grid, dim3(AT_THREADS), lds2, s,       \
                       a->qkv, a->lens, a->pos, a->bias_u, a->bias_v, a->lse, a->dout, a->dqkv,  \
                       dvec, g, win);                                                            \
    hipLaunchKernelGGL((relattn_bwd_dpos_kernel<DH, WIN>), grid_pos, dim3(AT_THREADS), lds3, s,  \
                       a->qkv, a->lens, a->pos, a->bias_u, a->bias_v, a->lse, a->dout, dvec,     \
                       part, g, win);                                                            \
  }
#define RA_BWD(DH) \
  if (wp) RA_BWD_W(DH, true) else RA_BWD_W(DH, false)
  RA_DISPATCH(RA_BWD)
#undef RA_BWD
#undef RA_BWD_W
  ASR_CHECK_LAUNCH();
  const int D = a->heads * a->dh, M = a->T * a->n_pad;
  int rc = asr_colsum(slab_c, M, D, D, a->dbias_u, 0.f, ws + w.colsum, w.colsum_bytes, stream);
  if (rc != ASR_OK) return rc;
  rc = asr_colsum(slab_p, M, D, D, a->dbias_v, 0.f, ws + w.colsum, w.colsum_bytes, stream);
  if (rc != ASR_OK) return rc;
  return asr_colsum(part, a->N, rows * a->ld_pos, rows * a->ld_pos, a->dpos, 0.f, ws + w.colsum,
                    w.colsum_bytes, stream);
}

extern "C" int asr_relattn_bwd(const asr_relattn_args* a, void* workspace, size_t ws_bytes,
                               asr_stream_t stream) {
  return ra_bwd(a, nullptr, workspace, ws_bytes, stream);
}

extern "C" int asr_relattn_win_bwd(const asr_relattn_args* a, const asr_attn_window* w,
                                   void* workspace, size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(at_win_ok(w), "relattn_win_bwd: bad window (" RA_WIN_TEXT ")");
  return ra_bwd(a, w, workspace, ws_bytes, stream);
}
