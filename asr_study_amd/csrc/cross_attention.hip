// K32 cross-attention core: softmax(scale Q K^T) V with the queries and the keys in two slabs of
// two lengths, forward and backward -- what an attention decoder runs between its label history
// and the encoder's frames.
//
// q (Tq, n_pad, ld_q >= D) holds Q in its first D = heads * dh columns, kv (Tk, n_pad, ld_kv >=
// 2D) holds [K | V].  Keys u >= k_lens[n] carry probability exactly 0 and get dK = dV = exactly
// 0; a query row t >= q_lens[n] has out = lse = exactly 0 and adds exactly 0 to every gradient.
//
// THE KERNELS are not in this file: they are the forward pass, pass (1) (D and dQ per query tile)
// and pass (2) (dK and dV per key tile) of attn_core.h with CROSS = true, i.e. the lines
// attention.hip runs, with Tk beside T in the geometry, the key source and its gradient behind
// pointers and strides of their own, and the query-row mask as one more select.  Grids:
//   forward, pass (1): (ceil(Tq / 64), heads, n_pad);  pass (2): (ceil(Tk / 64), heads, n_pad).
// The tile layout is K21's, so LDS per workgroup is at_lds_bytes<false>: 3 tiles + the score tile
// forward, 4 tiles + the score tile + 2 x 64 floats backward (dh 64: 69.6 KB / 87.6 KB, two and
// one workgroups per CU of 160 KB; dh 128: 118.8 KB / 153.1 KB, one) -- exactly what the
// self-attention instantiations have.  Tq = 1 (the decode step) runs one query tile per (sample,
// head) of which 63 rows are zeros.
#include "attn_core.h"

namespace {

bool ca_geo_ok(const asr_attn_cross_args* a) {
  if (a == nullptr || a->Tq < 1 || a->Tk < 1 || a->N < 1 || a->n_pad < a->N || a->n_pad > 65535)
    return false;
  if (a->heads < 1 || a->heads > 65535 || a->dh < 16 || a->dh > AT_MAX_DH || (a->dh & 15))
    return false;
  const long long D = (long long)a->heads * a->dh;
  if ((a->ld_q & 3) || a->ld_q < D || (a->ld_kv & 3) || a->ld_kv < 2 * D || (a->ld_out & 3) ||
      a->ld_out < D)
    return false;
  return a->scale > 0.f && a->scale < 1e30f;
}

#define CA_GEO_TEXT "Tq %d Tk %d N %d n_pad %d heads %d dh %d ld_q %d ld_kv %d ld_out %d; Tq, Tk " \
                    ">= 1, 1 <= N <= n_pad <= 65535, dh a multiple of 16 in 16..128, ld_q >= "     \
                    "heads dh, ld_kv >= 2 heads dh, ld_out >= heads dh, multiples of 4"
#define CA_GEO_ARGS(a)                                                                        \
  a ? a->Tq : 0, a ? a->Tk : 0, a ? a->N : 0, a ? a->n_pad : 0, a ? a->heads : 0, a ? a->dh : 0, \
      a ? a->ld_q : 0, a ? a->ld_kv : 0, a ? a->ld_out : 0

}  // namespace

extern "C" size_t asr_attn_cross_workspace_bytes(const asr_attn_cross_args* a) {
  if (!ca_geo_ok(a)) return 0;
  return asr_align_up((size_t)a->Tq * a->n_pad * a->heads * sizeof(float), 256);
}

extern "C" int asr_attn_cross_fwd(const asr_attn_cross_args* a, asr_stream_t stream) {
  ASR_CHECK_ARG(ca_geo_ok(a), "attn_cross_fwd: bad geometry (" CA_GEO_TEXT ")", CA_GEO_ARGS(a));
  ASR_CHECK_ARG(a->q && a->kv && a->out && a->out != a->q && a->out != a->kv,
                "attn_cross_fwd: q, kv and out are required");
  ASR_CHECK_ARG(at_aligned(a->q) && at_aligned(a->kv) && at_aligned(a->out),
                "attn_cross_fwd: q, kv, out 16-byte aligned");
  return at_launch_fwd<false, false, true>(a->q, a->kv, a->k_lens, a->q_lens, nullptr, nullptr,
                                           nullptr, a->out, a->lse, at_geo(a), a->dh, nullptr,
                                           stream);
}

extern "C" int asr_attn_cross_bwd(const asr_attn_cross_args* a, void* workspace, size_t ws_bytes,
                                  asr_stream_t stream) {
  ASR_CHECK_ARG(ca_geo_ok(a), "attn_cross_bwd: bad geometry (" CA_GEO_TEXT ")", CA_GEO_ARGS(a));
  ASR_CHECK_ARG(a->q && a->kv && a->out && a->lse && a->dout && a->dq && a->dkv &&
                    a->dq != a->q && a->dkv != a->kv,
                "attn_cross_bwd: q, kv, out, lse, dout, dq and dkv are required");
  ASR_CHECK_ARG(at_aligned(a->q) && at_aligned(a->kv) && at_aligned(a->dout) &&
                    at_aligned(a->dq) && at_aligned(a->dkv),
                "attn_cross_bwd: q, kv, dout, dq, dkv 16-byte aligned");
  const size_t need = asr_attn_cross_workspace_bytes(a);
  if (workspace == nullptr || ws_bytes < need) {
    asr_set_error("attn_cross_bwd: workspace too small (%zu bytes needed)", need);
    return ASR_ERR_WORKSPACE;
  }
  return at_launch_bwd<false, true>(a->q, a->kv, a->k_lens, a->q_lens, nullptr, nullptr, nullptr,
                                    a->out, a->lse, a->dout, a->dq, a->dkv, (float*)workspace,
                                    nullptr, nullptr, at_geo(a), a->dh, nullptr, stream);
}
