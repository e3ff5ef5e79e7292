// gru.hip -- the Keras-1.2.2 GRU recurrence (consume_less='gpu') of a Bidirectional layer (K16,
// include/asr_hip.h), forward and BPTT, both directions per launch.  Per direction, in processing
// order, with m = h_prev (.) B_U, hs(a) = clip(0.2 a + 0.5, 0, 1), U = [U_z | U_r | U_h] (H, 3H):
//   z = hs(zx_z + m U_z)   r = hs(zx_r + m U_r)   hh = act(zx_h + (r (.) m) U_h)
//   h = z (.) h_prev + (1 - z) (.) hh
// zx = x @ W + b comes from the GEMMs, and so do dW, dU, dx; this file owns the sequential part.
//
// A step has TWO dependent reductions (hh needs r, which needs the first product), so the
// stepwise form is two launches per step:
//   forward  A: m against the 2H columns [U_z | U_r]; epilogue writes z, r and r (.) m
//            B: r (.) m against U_h; epilogue writes hh and h
//   BPTT     A: da_h against U_h^T (q); epilogue writes da_r = q (.) m (.) hs'(r) and q (.) r
//            B: [da_z | da_r] against [U_z | U_r]^T (2H long); epilogue forms the carry
//               g z + (q r + product) (.) B_U and, from it, da_h and da_z of the NEXT step, so
//               the element-wise head of a step rides in the tail of the one before it.
// There is no persistent form (asr_gru_args.mode 2 is an argument error): DESIGN.md 15.
//
// Geometry and reduction: RecTile of rec_tile.h (NR batch rows x J output columns per workgroup,
// chunked operand in LDS, 4 x 4 register tiles, fixed-order cross-wave sum).  This file keeps
// what is the GRU's own: the address set-up of the four phases and their epilogues.
// The activation slopes of BPTT are read from the SAVED gates (hs' = 0.2 on 0 < gate < 1, else 0;
// act' from hh alone).
//
// The UNIDIRECTIONAL form (K28, asr_gru_uni_*) is the same step kernel with ND = 1 direction in
// every slab instead of 2: direction 0's addresses with the direction axis taken out, the same
// tile plan, chunk order and cross-wave sum, so with no initial state it gives direction 0's bits.
// Its forward pass may start from a state h0 (n_pad, H) -- step 0 then reads h0 where step s > 0
// reads h[s - 1], by the same code -- and the epilogue of the last phase-B launch also writes
// h[T - 1] to h_last: a sequence cut in two calls is the one call bit for bit.
#include "rec_tile.h"

namespace {

enum { kFwdA = 0, kFwdB = 1, kBwdA = 2, kBwdB = 3 };

struct GruParams {
  int T, n_pad, Hp;
  int act;
  float clip;
  int s;                   // the FORWARD step index this launch belongs to (kBwdB: T = prologue)
  // (2: the ND directions of the kernel; the unidirectional form has no such axis)
  const float* U;          // fwd: U (2, Hp, 3Hp); BPTT: U^T (2, 3Hp, Hp)
  const float* mask_u;     // (2, n_pad, Hp) or null
  const float* zx;         // fwd (T, n_pad, 2, 3Hp)
  float* h;                // (T, n_pad, 2, Hp)
  float* gates;            // (T, n_pad, 2, 3Hp): z | r | hh
  float* rm;               // (T, n_pad, 2, Hp): r (.) m
  const float* h0;         // ND = 1, fwd: (n_pad, Hp) state before frame 0, or null (zeros)
  float* h_last;           // ND = 1, fwd: (n_pad, Hp) <- h[T - 1], or null
  const float* dy;         // BPTT
  long long dy_ld;
  int dy_dstride;
  float* da;               // BPTT (T, n_pad, 2, 3Hp): da_z | da_r | da_h
  float* gbuf;             // BPTT workspace (n_pad, 2, Hp): g = dy + carry of the current step
  float* qr;               // BPTT workspace (n_pad, 2, Hp): q (.) r
};

template <int NR, int PH, int ND>
__global__ void __launch_bounds__(kThreads)
gru_step_kernel(GruParams p) {
  using Tile = RecTile<NR>;
  constexpr int J = Tile::J;
  __shared__ __attribute__((aligned(16))) float lds[Tile::kLdsFloats];

  const int tid = threadIdx.x;
  const int jb = blockIdx.x, nt = blockIdx.y, d = blockIdx.z;
  const int Hp = p.Hp, n_pad = p.n_pad, T = p.T, s = p.s;
  const int j0 = jb * J, n0 = nt * NR;
  const float* mu = p.mask_u ? p.mask_u + ((size_t)d * n_pad + n0) * Hp : nullptr;
  // times of forward steps s, s - 1, s - 2 of this direction (d = 1 walks time downwards)
  const int t = d == 0 ? s : T - 1 - s;
  const int tp = d == 0 ? t - 1 : t + 1;
  const int tpp = d == 0 ? t - 2 : t + 2;
  const size_t row0 = (size_t)t * n_pad + n0;          // (kBwdB prologue, s == T: not used)
  const size_t rowp0 = (size_t)tp * n_pad + n0;

  // the reduction of this phase: operand rows (stride op_ld, K long), matrix rows (stride ldm),
  // nout output columns in all
  const float* op = nullptr;
  const float* mat = nullptr;
  size_t op_ld = 0;
  int K = Hp, ldm = Hp, nout = Hp;
  // forward: the state the step starts from, rows n0 .. of (., Hp) at stride hp_ld -- h of the
  // step before or, at step 0 of the unidirectional form, h0; null: zeros
  const float* hprev = nullptr;
  size_t hp_ld = 0;
  if (s > 0) {
    hprev = p.h + (rowp0 * ND + d) * Hp; hp_ld = ND * (size_t)Hp;
  } else if (ND == 1 && p.h0 != nullptr) {
    hprev = p.h0 + (size_t)n0 * Hp; hp_ld = Hp;
  }
  bool skip = s == 0;                      // h_prev = 0: every product of the step is 0
  if (PH == kFwdA) {
    op = hprev; op_ld = hp_ld;
    mat = p.U + (size_t)d * Hp * 3 * Hp; ldm = 3 * Hp; nout = 2 * Hp;
    skip = hprev == nullptr;
  } else if (PH == kFwdB) {
    op = p.rm + (row0 * ND + d) * Hp; op_ld = ND * (size_t)Hp;
    mat = p.U + (size_t)d * Hp * 3 * Hp + 2 * Hp; ldm = 3 * Hp;
    skip = hprev == nullptr;
  } else if (PH == kBwdA) {
    op = p.da + (row0 * ND + d) * 3 * Hp + 2 * Hp; op_ld = 3 * ND * (size_t)Hp;
    mat = p.U + ((size_t)d * 3 * Hp + 2 * Hp) * Hp;
  } else {
    op = p.da + (row0 * ND + d) * 3 * Hp; op_ld = 3 * ND * (size_t)Hp;
    mat = p.U + (size_t)d * 3 * Hp * Hp; K = 2 * Hp;
    skip = s >= T;
  }

  // epilogue ownership: row en, columns ej .. ej + 3 of the tile
  const int en = (4 * tid) / J, ej = (4 * tid) % J;
  const int jg = j0 + ej;
  const bool eown = jg < nout;

  float4 r = zero4();
  if (!skip) {
    float acc[4][4];
    Tile::template reduce<PH == kFwdA>(                  // kFwdA: m = h_prev (.) B_U
        lds, op, op_ld, K, mat, ldm, mu, Hp,
        [&](int jj) { return j0 + jj < nout ? j0 + jj : -1; }, acc);
    Tile::spill(lds, acc);
    r = Tile::total(lds, en, ej);
  }
  if (!eown) return;

  const size_t row = row0 + en, rowp = rowp0 + en;
  if (PH == kFwdA) {
    // columns [0, Hp): z; [Hp, 2Hp): r (a float4 never straddles the two: Hp % 4 == 0)
    const size_t o = (row * ND + d) * 3 * Hp + jg;
    const float4 zx = ld4(p.zx + o);
    const float4 g = make_float4(hard_sigmoid(zx.x + r.x), hard_sigmoid(zx.y + r.y),
                                 hard_sigmoid(zx.z + r.z), hard_sigmoid(zx.w + r.w));
    st4(p.gates + o, g);
    if (jg >= Hp) {
      const int j = jg - Hp;
      float4 m = zero4();
      if (hprev != nullptr) {
        m = ld4(hprev + en * hp_ld + j);
        if (mu != nullptr) m = mul4(m, ld4(mu + (size_t)en * Hp + j));
      }
      st4(p.rm + (row * ND + d) * Hp + j, mul4(g, m));
    }
  } else if (PH == kFwdB) {
    const size_t og = (row * ND + d) * 3 * Hp, oh = (row * ND + d) * Hp + jg;
    const float4 zx = ld4(p.zx + og + 2 * Hp + jg);
    const float4 z = ld4(p.gates + og + jg);
    const float4 hp = hprev != nullptr ? ld4(hprev + en * hp_ld + jg) : zero4();
    const float4 hh = make_float4(rec_act(p.act, p.clip, zx.x + r.x), rec_act(p.act, p.clip, zx.y + r.y),
                                  rec_act(p.act, p.clip, zx.z + r.z), rec_act(p.act, p.clip, zx.w + r.w));
    st4(p.gates + og + 2 * Hp + jg, hh);
    const float4 hn = make_float4(z.x * hp.x + (1.f - z.x) * hh.x, z.y * hp.y + (1.f - z.y) * hh.y,
                                  z.z * hp.z + (1.f - z.z) * hh.z, z.w * hp.w + (1.f - z.w) * hh.w);
    st4(p.h + oh, hn);
    if (ND == 1 && s == T - 1 && p.h_last != nullptr)
      st4(p.h_last + (size_t)(n0 + en) * Hp + jg, hn);
  } else if (PH == kBwdA) {
    // q = r (the product); da_r = q (.) m (.) hs'(r gate); q (.) r gate kept for phase B
    const size_t og = (row * ND + d) * 3 * Hp + Hp + jg;
    const float4 rg = ld4(p.gates + og);
    float4 m = zero4();
    if (s > 0) {
      m = ld4(p.h + (rowp * ND + d) * Hp + jg);
      if (mu != nullptr) m = mul4(m, ld4(mu + (size_t)en * Hp + jg));
    }
    st4(p.da + og, make_float4(r.x * m.x * hs_slope(rg.x), r.y * m.y * hs_slope(rg.y),
                               r.z * m.z * hs_slope(rg.z), r.w * m.w * hs_slope(rg.w)));
    st4(p.qr + ((size_t)(n0 + en) * ND + d) * Hp + jg, mul4(r, rg));
  } else {
    const size_t ow = ((size_t)(n0 + en) * ND + d) * Hp + jg;
    float4 carry = zero4();
    if (s < T) {
      const float4 qr = ld4(p.qr + ow), g = ld4(p.gbuf + ow);
      const float4 z = ld4(p.gates + (row * ND + d) * 3 * Hp + jg);
      float4 dm = make_float4(qr.x + r.x, qr.y + r.y, qr.z + r.z, qr.w + r.w);
      if (mu != nullptr) dm = mul4(dm, ld4(mu + (size_t)en * Hp + jg));
      carry = make_float4(g.x * z.x + dm.x, g.y * z.y + dm.y, g.z * z.z + dm.z, g.w * z.w + dm.w);
    }
    // the element-wise head of the next BPTT step (forward step s - 1, time tp)
    const size_t og = (rowp * ND + d) * 3 * Hp;
    const float4 dy = ld4(p.dy + rowp * p.dy_ld + (size_t)d * p.dy_dstride + jg);
    const float4 g = make_float4(dy.x + carry.x, dy.y + carry.y, dy.z + carry.z, dy.w + carry.w);
    const float4 z = ld4(p.gates + og + jg), hh = ld4(p.gates + og + 2 * Hp + jg);
    const float4 hp = s - 1 > 0 ? ld4(p.h + (((size_t)tpp * n_pad + n0 + en) * ND + d) * Hp + jg)
                                : zero4();
    st4(p.da + og + 2 * Hp + jg,
        make_float4(g.x * (1.f - z.x) * rec_slope(p.act, p.clip, hh.x),
                    g.y * (1.f - z.y) * rec_slope(p.act, p.clip, hh.y),
                    g.z * (1.f - z.z) * rec_slope(p.act, p.clip, hh.z),
                    g.w * (1.f - z.w) * rec_slope(p.act, p.clip, hh.w)));
    st4(p.da + og + jg,
        make_float4(g.x * (hp.x - hh.x) * hs_slope(z.x), g.y * (hp.y - hh.y) * hs_slope(z.y),
                    g.z * (hp.z - hh.z) * hs_slope(z.z), g.w * (hp.w - hh.w) * hs_slope(z.w)));
    st4(p.gbuf + ow, g);
  }
}

// ---- host side -------------------------------------------------------------------------------
// What a call is, whichever args block it came in (asr_gru_args: nd = 2; asr_gru_uni_args: nd = 1).
struct GruCall {
  const char* pfx;
  int nd, T, n_pad, H, act;
  float clip;
  const float *U, *mask_u, *zx, *h0, *dy;
  float *h, *gates, *rm, *y_sum, *h_last, *da, *db_part, *dz_absmax;
  long long dy_ld;
  int dy_dstride;
};

// the checks of rec_check_args, then the fields both args blocks share
template <class Args>
int gru_call_common(const char* pfx, int nd, const Args* a, GruCall* c) {
  const int rc = rec_check_args(pfx, a, false);
  if (rc != ASR_OK) return rc;
  *c = GruCall();
  c->pfx = pfx; c->nd = nd;
  c->T = a->T; c->n_pad = a->n_pad; c->H = a->H; c->act = a->activation; c->clip = a->clip;
  c->U = a->U; c->mask_u = a->mask_u; c->zx = a->zx; c->h = a->h; c->gates = a->gates;
  c->rm = a->rm; c->dy = a->dy; c->dy_ld = a->dy_ld; c->da = a->da; c->db_part = a->db_part;
  c->dz_absmax = a->dz_absmax;
  return ASR_OK;
}

int gru_call(const asr_gru_args* a, GruCall* c) {
  const int rc = gru_call_common("gru", 2, a, c);
  if (rc != ASR_OK) return rc;
  c->y_sum = a->y_sum; c->dy_dstride = a->dy_dir_stride;
  return ASR_OK;
}

int gru_call(const asr_gru_uni_args* a, GruCall* c) {
  const int rc = gru_call_common("gru_uni", 1, a, c);
  if (rc != ASR_OK) return rc;
  c->h0 = a->h0; c->h_last = a->h_last;
  return ASR_OK;
}

// the tile plan depends on (n_pad, H) alone: one direction's is the bidirectional one's, with
// half the workgroups
RecPlan make_gru_plan(const GruCall& c, bool bwd) {
  // the widest launch: forward phase A has 2H output columns, every other phase H
  RecPlan pl = rec_plan(c.n_pad, bwd ? c.H : 2 * c.H, c.nd);
  if (bwd) {
    pl.ut_bytes = asr_align_up((size_t)c.nd * 3 * c.H * c.H * sizeof(float), 256);
    pl.vec_bytes = asr_align_up((size_t)c.n_pad * c.nd * c.H * sizeof(float), 256);
  }
  return pl;
}

size_t gru_ws_bytes(const RecPlan& pl) { return 256 + pl.ut_bytes + 2 * pl.vec_bytes; }

template <int NR, int ND>
int gru_launch(int ph, const GruParams& p, int ncols, int nbt, hipStream_t stream) {
  constexpr int J = RecTile<NR>::J;
  const dim3 grid((ncols + J - 1) / J, nbt, ND);
  switch (ph) {
    case kFwdA: hipLaunchKernelGGL((gru_step_kernel<NR, kFwdA, ND>), grid, dim3(kThreads), 0, stream, p); break;
    case kFwdB: hipLaunchKernelGGL((gru_step_kernel<NR, kFwdB, ND>), grid, dim3(kThreads), 0, stream, p); break;
    case kBwdA: hipLaunchKernelGGL((gru_step_kernel<NR, kBwdA, ND>), grid, dim3(kThreads), 0, stream, p); break;
    default:    hipLaunchKernelGGL((gru_step_kernel<NR, kBwdB, ND>), grid, dim3(kThreads), 0, stream, p); break;
  }
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

int gru_phase(const RecPlan& pl, int nd, int ph, const GruParams& p, int ncols, hipStream_t stream) {
  return rec_with_rows(pl.NR, [&](auto nr) {
    constexpr int NR = decltype(nr)::value;
    return nd == 1 ? gru_launch<NR, 1>(ph, p, ncols, pl.NBT, stream)
                   : gru_launch<NR, 2>(ph, p, ncols, pl.NBT, stream);
  });
}

// every argument error is refused here, before the first device call
int gru_run(const GruCall& c, bool bwd, void* workspace, size_t ws_bytes, hipStream_t stream) {
  const RecPlan pl = make_gru_plan(c, bwd);
  const int nd = c.nd;
  int rc = rec_check_ws(c.pfx, workspace, ws_bytes, gru_ws_bytes(pl));
  if (rc != ASR_OK) return rc;
  ASR_CHECK_ARG(c.U && c.h && c.gates, "%s: U, h and gates are required", c.pfx);
  if (bwd) ASR_CHECK_ARG(c.dy && c.da && c.dy_ld >= c.H && c.dy_ld % 4 == 0 &&
                         c.dy_dstride % 4 == 0,
                         "%s: BPTT needs dy (dy_ld >= H, a multiple of 4) and da", c.pfx);
  else ASR_CHECK_ARG(c.zx && c.rm, "%s: the forward pass needs zx and rm", c.pfx);
  ASR_CHECK_ARG(c.h_last == nullptr || c.h_last != c.h0, "%s: h_last aliases h0 (a call leaves "
                "the state it starts from intact: keep two buffers and swap them)", c.pfx);
  ASR_CHECK_ARG(!bwd || (c.h0 == nullptr && c.h_last == nullptr), "%s: BPTT takes no h0 / h_last "
                "(training starts from the zero state)", c.pfx);
  char* ws = static_cast<char*>(workspace);
  const int H = c.H, T = c.T;
  GruParams p;
  p.T = T; p.n_pad = c.n_pad; p.Hp = H;
  p.act = c.act; p.clip = c.clip;
  p.mask_u = c.mask_u; p.zx = c.zx; p.h = c.h; p.gates = c.gates; p.rm = c.rm;
  p.h0 = c.h0; p.h_last = c.h_last;
  p.dy = c.dy; p.dy_ld = c.dy_ld; p.dy_dstride = c.dy_dstride;
  p.da = c.da;
  p.gbuf = reinterpret_cast<float*>(ws + 256 + pl.ut_bytes);
  p.qr = reinterpret_cast<float*>(ws + 256 + pl.ut_bytes + pl.vec_bytes);
  if (!bwd) {
    p.U = c.U;
    for (int s = 0; s < T; ++s) {
      p.s = s;
      if ((rc = gru_phase(pl, nd, kFwdA, p, 2 * H, stream)) != ASR_OK) return rc;
      if ((rc = gru_phase(pl, nd, kFwdB, p, H, stream)) != ASR_OK) return rc;
    }
    if (c.y_sum) return rec_sum(c.h, c.y_sum, (long long)T * c.n_pad, H, stream);
    return ASR_OK;
  }
  float* Ut = reinterpret_cast<float*>(ws + 256);
  if ((rc = rec_transpose(c.U, Ut, nd, H, 3 * H, stream)) != ASR_OK) return rc;
  p.U = Ut;
  // phase B of step s also prepares da_h, da_z of step s - 1: s = T is the prologue (carry 0)
  p.s = T;
  if ((rc = gru_phase(pl, nd, kBwdB, p, H, stream)) != ASR_OK) return rc;
  for (int s = T - 1; s >= 0; --s) {
    p.s = s;
    if ((rc = gru_phase(pl, nd, kBwdA, p, H, stream)) != ASR_OK) return rc;
    if (s > 0 && (rc = gru_phase(pl, nd, kBwdB, p, H, stream)) != ASR_OK) return rc;
  }
  if (c.db_part || c.dz_absmax)
    return nd == 1 ? rec_dbias<1>(c.da, c.db_part, c.dz_absmax, T, c.n_pad, 1, 3 * H, stream)
                   : rec_dbias<2>(c.da, c.db_part, c.dz_absmax, T, c.n_pad, 1, 3 * H, stream);
  return ASR_OK;
}

template <class Args>
size_t gru_ws_of(const Args* a, int backward) {
  GruCall c;
  if (gru_call(a, &c) != ASR_OK) return 0;
  return gru_ws_bytes(make_gru_plan(c, backward != 0));
}

template <class Args>
int gru_run_of(const Args* a, bool bwd, void* workspace, size_t ws_bytes, asr_stream_t stream) {
  GruCall c;
  const int rc = gru_call(a, &c);
  if (rc != ASR_OK) return rc;
  return gru_run(c, bwd, workspace, ws_bytes, (hipStream_t)stream);
}

template <class Args>
int gru_plan_of(const Args* a, int backward, int* persistent, int* rows, int* units, int* blocks) {
  GruCall c;
  const int rc = gru_call(a, &c);
  if (rc != ASR_OK) return rc;
  const RecPlan pl = make_gru_plan(c, backward != 0);
  return rec_plan_out(pl, pl.J, persistent, rows, units, blocks);
}

}  // namespace

extern "C" size_t asr_gru_workspace_bytes(const asr_gru_args* a, int backward) {
  return gru_ws_of(a, backward);
}

extern "C" int asr_gru_seq_fwd(const asr_gru_args* a, void* workspace, size_t ws_bytes,
                               asr_stream_t stream) {
  return gru_run_of(a, false, workspace, ws_bytes, stream);
}

extern "C" int asr_gru_seq_bwd(const asr_gru_args* a, void* workspace, size_t ws_bytes,
                               asr_stream_t stream) {
  return gru_run_of(a, true, workspace, ws_bytes, stream);
}

extern "C" int asr_gru_plan(const asr_gru_args* a, int backward, int* persistent, int* rows,
                            int* units, int* blocks) {
  return gru_plan_of(a, backward, persistent, rows, units, blocks);
}

extern "C" size_t asr_gru_uni_workspace_bytes(const asr_gru_uni_args* a, int backward) {
  return gru_ws_of(a, backward);
}

extern "C" int asr_gru_uni_seq_fwd(const asr_gru_uni_args* a, void* workspace, size_t ws_bytes,
                                   asr_stream_t stream) {
  return gru_run_of(a, false, workspace, ws_bytes, stream);
}

extern "C" int asr_gru_uni_seq_bwd(const asr_gru_uni_args* a, void* workspace, size_t ws_bytes,
                                   asr_stream_t stream) {
  return gru_run_of(a, true, workspace, ws_bytes, stream);
}

extern "C" int asr_gru_uni_plan(const asr_gru_uni_args* a, int backward, int* persistent,
                                int* rows, int* units, int* blocks) {
  return gru_plan_of(a, backward, persistent, rows, units, blocks);
}
