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
// exponentials, 64 x 64 score tiles in registers.  The forward pass and passes (1) and (2) ARE
// attention.hip's: the kernels of attn_core.h with REL = true, which adds what is described here
// under `if constexpr`; pass (3) is this family's alone and lives in this file with the
// argument checks, the workspace and the entry points of asr_relattn_*.
// What is new is the BAND: for a query tile at
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
//
// K26, THE STREAMING FORWARD (asr_relattn_stream_fwd): the forward kernel of attn_core.h with
// REL and STREAM (Q from the chunk's slab, K and V from THE RING of attn_tile.h, the absolute
// 64-aligned key tiles of the whole-utterance call, kv_len for lens).  pos is a table of 2P - 1
// rows, row r + P - 1 the relative index r, P >= left + chunk: it covers every visible pair
// (0 <= t - u <= left + chunk - 1) and does not depend on how long the stream runs.  Band rows
// outside the table are staged as zeros, here as in the whole-utterance call, and meet masked
// pairs only; a band element is one at_dot chain over a query row and a table row, wherever the
// rows sit in their tiles, so the rows come out bit for bit as from asr_relattn_win_fwd on the
// same projected table values.
#include "attn_core.h"

namespace {

// backward pass 3: the partial of sample n of the table rows [64 m, 64 m + 64), i.e. the relative
// indices r0 + b with r0 = 64 m - (T - 1); part is (N, 2T - 1, ld_pos)
template <int DH, bool WIN>
__global__ __launch_bounds__(AT_THREADS) void relattn_bwd_dpos_kernel(
    const float* __restrict__ qkv, const int* __restrict__ lens, const float* __restrict__ pos,
    const float* __restrict__ bias_u, const float* __restrict__ bias_v,
    const float* __restrict__ lse, const float* __restrict__ dout, const float* __restrict__ dvec,
    float* __restrict__ part, AtGeo g, asr_attn_window w) {
  constexpr int DP = DH + 4, NJ = DH / 16;
  extern __shared__ float4 at_lds4[];
  float* Bs = reinterpret_cast<float*>(at_lds4);   // the 64 rows of this band tile
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

// LDS bytes of pass 3 (dpos); the other passes: at_lds_bytes<true> of attn_core.h
size_t ra_dpos_lds_bytes(int dh) {
  return 5 * (size_t)AT_TILE * (dh + 4) * sizeof(float) + (size_t)AT_TILE * AT_PP * sizeof(float) +
         RA_SMALL * sizeof(float);
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

}  // namespace

#define RA_GEO_TEXT "dh a multiple of 16 in 16..64 (the band tiles of the relative term leave " \
                    "no room in LDS for dh 80..128), heads >= 1, ld >= 3 heads dh, ld_out >= "   \
                    "heads dh, ld_pos >= heads dh, all multiples of 4"

extern "C" size_t asr_relattn_workspace_bytes(const asr_relattn_args* a) {
  if (!ra_geo_ok(a)) return 0;
  return ra_ws(a).end;
}

extern "C" int asr_relattn_plan(const asr_relattn_args* a, int backward, int* bq, int* bk,
                                int* blocks, int* lds_bytes) {
  ASR_CHECK_ARG(ra_geo_ok(a), "relattn_plan: bad geometry (" RA_GEO_TEXT ")");
  at_plan(a->T, a->heads, a->n_pad, bq, bk, blocks);
  if (lds_bytes) {
    size_t lds = backward ? ra_dpos_lds_bytes(a->dh) : at_lds_bytes<true>(a->dh, 0);
    for (int pass = 1; backward && pass <= 2; ++pass)        // backward: the largest pass
      if (at_lds_bytes<true>(a->dh, pass) > lds) lds = at_lds_bytes<true>(a->dh, pass);
    *lds_bytes = (int)lds;
  }
  return ASR_OK;
}

extern "C" int asr_relattn_win_plan(const asr_relattn_args* a, const asr_attn_window* w,
                                    int backward, int* bq, int* bk, int* blocks, int* lds_bytes,
                                    long long* tile_pairs) {
  ASR_CHECK_ARG(at_win_ok(w), "relattn_win_plan: bad window (" AT_WIN_TEXT ")");
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
  return at_launch_fwd<true, false>(a->qkv, a->qkv + a->heads * a->dh, a->lens, nullptr, a->pos,
                                    a->bias_u, a->bias_v, a->out, a->lse, at_geo(a, a->ld_pos),
                                    a->dh, w, stream);
}

extern "C" int asr_relattn_fwd(const asr_relattn_args* a, asr_stream_t stream) {
  return ra_fwd(a, nullptr, stream);
}

extern "C" int asr_relattn_win_fwd(const asr_relattn_args* a, const asr_attn_window* w,
                                   asr_stream_t stream) {
  ASR_CHECK_ARG(at_win_ok(w), "relattn_win_fwd: bad window (" AT_WIN_TEXT ")");
  return ra_fwd(a, w, stream);
}

extern "C" int asr_relattn_stream_fwd(const asr_attn_stream_args* a, const asr_attn_window* w,
                                      asr_stream_t stream) {
  const char* bad = at_stream_bad(a, w, RA_MAX_DH, true);
  ASR_CHECK_ARG(bad == nullptr, "relattn_stream_fwd: %s", bad);
  return at_launch_fwd<true, true>(a->q, a->ring, a->kv_len, nullptr, a->pos, a->bias_u,
                                   a->bias_v, a->out, nullptr, at_geo(a), a->dh, w, stream);
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
  const AtGeo g = at_geo(a, a->ld_pos);
  char* ws = (char*)workspace;
  float* dvec = (float*)(ws + w.dvec);
  float* slab_c = (float*)(ws + w.slab_c);
  float* slab_p = (float*)(ws + w.slab_p);
  float* part = (float*)(ws + w.part);
  const int rows = 2 * a->T - 1;
  const int D = a->heads * a->dh, M = a->T * a->n_pad;
  int rc = at_launch_bwd<true>(a->qkv, a->qkv + D, a->lens, nullptr, a->pos, a->bias_u, a->bias_v,
                               a->out, a->lse, a->dout, a->dqkv, a->dqkv + D, dvec, slab_c, slab_p,
                               g, a->dh, wp, stream);
  if (rc != ASR_OK) return rc;
  const dim3 grid_pos((rows + AT_TILE - 1) / AT_TILE, a->heads, a->N);
  const size_t lds3 = ra_dpos_lds_bytes(a->dh);
  const asr_attn_window win = wp ? *wp : asr_attn_window{1, -1, 0};
  auto go = [&](auto kernel) -> int {
    if (at_allow_lds(kernel, lds3) != ASR_OK) return ASR_ERR_LAUNCH;
    hipLaunchKernelGGL(kernel, grid_pos, dim3(AT_THREADS), lds3, (hipStream_t)stream, a->qkv,
                       a->lens, a->pos, a->bias_u, a->bias_v, (const float*)a->lse, a->dout,
                       (const float*)dvec, part, g, win);
    ASR_CHECK_LAUNCH();
    return ASR_OK;
  };
  rc = at_dispatch<RA_MAX_DH>(a->dh, [&](auto c) -> int {
    constexpr int DH = decltype(c)::value;
    return wp ? go(relattn_bwd_dpos_kernel<DH, true>) : go(relattn_bwd_dpos_kernel<DH, false>);
  });
  if (rc != ASR_OK) return rc;
  rc = asr_colsum(slab_c, M, D, D, a->dbias_u, 0.f, ws + w.colsum, w.colsum_bytes, stream);
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
  ASR_CHECK_ARG(at_win_ok(w), "relattn_win_bwd: bad window (" AT_WIN_TEXT ")");
  return ra_bwd(a, w, workspace, ws_bytes, stream);
}
