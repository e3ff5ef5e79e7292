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
// THE KERNELS are not in this file: the forward pass, pass (1) and pass (2) are written once in
// attn_core.h for this family, the relative one (rel_attention.hip) and the streaming forms of
// both; this file instantiates them with REL = false and holds the argument checks and entry
// points of asr_attn_*.  The tile pieces (loads, the two products, the butterflies) are in
// attn_tile.h.
//
// K25, THE WINDOW (asr_attn_win_*; defined once in attn_tile.h): chunk >= 1, left >= -1 frames
// (-1: unlimited), right >= 0 frames.  For query frame t, c0 = (t / chunk) * chunk, key u is
// visible iff lo(t) <= u < hi(t) and u < lens[n], hi(t) = c0 + chunk + right, lo(t) = left < 0 ?
// 0 : max(0, c0 - left).  The kernels are templates on a bool (WIN): without the window they are
// the code above, bit for bit.  With it the mask stays a select (a key outside meets p = exactly 0
// only) and the loops visit only the tiles that hold a visible pair:
//   forward, dQ: the key tiles that meet [lo(q0), min(hi(last query of the tile), len));
//   dK / dV:     the query tiles with lo(first) <= k0 + 63 and hi(last) > k0 (lo, hi monotone:
//                one contiguous range; a key tile no query sees writes exact zeros).
// A row with NO visible key (a padding query with lo(t) >= len) has out = lse = exactly 0: the
// forward guards exp2f(-inf - -inf) and the division by l = 0; the backward recomputes p = 0 for
// it everywhere, so dQ_t = 0 and it adds nothing to dK, dV.
//
// K26, THE STREAMING FORWARD (asr_attn_stream_fwd): the queries [t0, t0 + Tq) of the windowed
// forward, Q from the chunk's slab (Tq, n_pad, ld), K and V from THE RING of attn_tile.h, columns
// [K | V] of (R, n_pad, ld_kv); kv_len[n] (device int32, the absolute frames of stream n that are
// valid so far) plays the part of lens.  It is the forward kernel of attn_core.h with STREAM =
// true: the rows come out bit for bit as from asr_attn_win_fwd because they run the same lines.
#include "attn_core.h"

namespace {

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
  if (a->heads < 1 || a->heads > 65535 || a->dh < 16 || a->dh > AT_MAX_DH || (a->dh & 15))
    return false;
  const long long D = (long long)a->heads * a->dh;
  if ((a->ld & 3) || a->ld < 3 * D || (a->ld_out & 3) || a->ld_out < D) return false;
  return a->scale > 0.f && a->scale < 1e30f;
}

}  // namespace

extern "C" size_t asr_attn_workspace_bytes(const asr_attn_args* a) {
  if (!at_geo_ok(a)) return 0;
  return asr_align_up((size_t)a->T * a->n_pad * a->heads * sizeof(float), 256);
}

extern "C" int asr_attn_plan(const asr_attn_args* a, int backward, int* bq, int* bk, int* blocks,
                             int* lds_bytes) {
  ASR_CHECK_ARG(at_geo_ok(a), "attn_plan: bad geometry (dh a multiple of 16 in 16..128, heads "
                              ">= 1, ld >= 3 heads dh, ld_out >= heads dh, both multiples of 4)");
  at_plan(a->T, a->heads, a->n_pad, bq, bk, blocks);
  if (lds_bytes) *lds_bytes = (int)at_lds_bytes<false>(a->dh, backward);
  return ASR_OK;
}

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
  return at_launch_fwd<false, false>(a->qkv, a->qkv + a->heads * a->dh, a->lens, nullptr, nullptr,
                                     nullptr, nullptr, a->out, a->lse, at_geo(a, 0), a->dh, w,
                                     stream);
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
  const int D = a->heads * a->dh;
  return at_launch_bwd<false>(a->qkv, a->qkv + D, a->lens, nullptr, nullptr, nullptr, nullptr,
                              a->out, a->lse, a->dout, a->dqkv, a->dqkv + D, (float*)workspace,
                              nullptr, nullptr, at_geo(a, 0), a->dh, w, stream);
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
  const char* bad = at_stream_bad(a, w, AT_MAX_DH, false);
  ASR_CHECK_ARG(bad == nullptr, "attn_stream_fwd: %s", bad);
  return at_launch_fwd<false, true>(a->q, a->ring, a->kv_len, nullptr, nullptr, nullptr, nullptr,
                                    a->out, nullptr, at_geo(a), a->dh, w, stream);
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
