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
#include "rec_tile.h"

namespace {

enum { kFwdA = 0, kFwdB = 1, kBwdA = 2, kBwdB = 3 };

struct GruParams {
  int T, n_pad, Hp;
  int act;
  float clip;
  int s;                   // the FORWARD step index this launch belongs to (kBwdB: T = prologue)
  const float* U;          // fwd: U (2, Hp, 3Hp); BPTT: U^T (2, 3Hp, Hp)
  const float* mask_u;     // (2, n_pad, Hp) or null
  const float* zx;         // fwd (T, n_pad, 2, 3Hp)
  float* h;                // (T, n_pad, 2, Hp)
  float* gates;            // (T, n_pad, 2, 3Hp): z | r | hh
  float* rm;               // (T, n_pad, 2, Hp): r (.) m
  const float* dy;         // BPTT
  long long dy_ld;
  int dy_dstride;
  float* da;               // BPTT (T, n_pad, 2, 3Hp): da_z | da_r | da_h
  float* gbuf;             // BPTT workspace (n_pad, 2, Hp): g = dy + carry of the current step
  float* qr;               // BPTT workspace (n_pad, 2, Hp): q (.) r
};

template <int NR, int PH>
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
  bool skip = s == 0;                      // h_prev = 0: every product of the step is 0
  if (PH == kFwdA) {
    op = p.h + (rowp0 * 2 + d) * Hp; op_ld = 2 * (size_t)Hp;
    mat = p.U + (size_t)d * Hp * 3 * Hp; ldm = 3 * Hp; nout = 2 * Hp;
  } else if (PH == kFwdB) {
    op = p.rm + (row0 * 2 + d) * Hp; op_ld = 2 * (size_t)Hp;
    mat = p.U + (size_t)d * Hp * 3 * Hp + 2 * Hp; ldm = 3 * Hp;
  } else if (PH == kBwdA) {
    op = p.da + (row0 * 2 + d) * 3 * Hp + 2 * Hp; op_ld = 6 * (size_t)Hp;
    mat = p.U + ((size_t)d * 3 * Hp + 2 * Hp) * Hp;
  } else {
    op = p.da + (row0 * 2 + d) * 3 * Hp; op_ld = 6 * (size_t)Hp;
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
    const size_t o = (row * 2 + d) * 3 * Hp + jg;
    const float4 zx = ld4(p.zx + o);
    const float4 g = make_float4(hard_sigmoid(zx.x + r.x), hard_sigmoid(zx.y + r.y),
                                 hard_sigmoid(zx.z + r.z), hard_sigmoid(zx.w + r.w));
    st4(p.gates + o, g);
    if (jg >= Hp) {
      const int j = jg - Hp;
      float4 m = zero4();
      if (s > 0) {
        m = ld4(p.h + (rowp * 2 + d) * Hp + j);
        if (mu != nullptr) m = mul4(m, ld4(mu + (size_t)en * Hp + j));
      }
      st4(p.rm + (row * 2 + d) * Hp + j, mul4(g, m));
    }
  } else if (PH == kFwdB) {
    const size_t og = (row * 2 + d) * 3 * Hp, oh = (row * 2 + d) * Hp + jg;
    const float4 zx = ld4(p.zx + og + 2 * Hp + jg);
    const float4 z = ld4(p.gates + og + jg);
    const float4 hp = s > 0 ? ld4(p.h + (rowp * 2 + d) * Hp + jg) : zero4();
    const float4 hh = make_float4(rec_act(p.act, p.clip, zx.x + r.x), rec_act(p.act, p.clip, zx.y + r.y),
                                  rec_act(p.act, p.clip, zx.z + r.z), rec_act(p.act, p.clip, zx.w + r.w));
    st4(p.gates + og + 2 * Hp + jg, hh);
    st4(p.h + oh, make_float4(z.x * hp.x + (1.f - z.x) * hh.x, z.y * hp.y + (1.f - z.y) * hh.y,
                              z.z * hp.z + (1.f - z.z) * hh.z, z.w * hp.w + (1.f - z.w) * hh.w));
  } else if (PH == kBwdA) {
    // q = r (the product); da_r = q (.) m (.) hs'(r gate); q (.) r gate kept for phase B
    const size_t og = (row * 2 + d) * 3 * Hp + Hp + jg;
    const float4 rg = ld4(p.gates + og);
    float4 m = zero4();
    if (s > 0) {
      m = ld4(p.h + (rowp * 2 + d) * Hp + jg);
      if (mu != nullptr) m = mul4(m, ld4(mu + (size_t)en * Hp + jg));
    }
    st4(p.da + og, make_float4(r.x * m.x * hs_slope(rg.x), r.y * m.y * hs_slope(rg.y),
                               r.z * m.z * hs_slope(rg.z), r.w * m.w * hs_slope(rg.w)));
    st4(p.qr + ((size_t)(n0 + en) * 2 + d) * Hp + jg, mul4(r, rg));
  } else {
    const size_t ow = ((size_t)(n0 + en) * 2 + d) * Hp + jg;
    float4 carry = zero4();
    if (s < T) {
      const float4 qr = ld4(p.qr + ow), g = ld4(p.gbuf + ow);
      const float4 z = ld4(p.gates + (row * 2 + d) * 3 * Hp + jg);
      float4 dm = make_float4(qr.x + r.x, qr.y + r.y, qr.z + r.z, qr.w + r.w);
      if (mu != nullptr) dm = mul4(dm, ld4(mu + (size_t)en * Hp + jg));
      carry = make_float4(g.x * z.x + dm.x, g.y * z.y + dm.y, g.z * z.z + dm.z, g.w * z.w + dm.w);
    }
    // the element-wise head of the next BPTT step (forward step s - 1, time tp)
    const size_t og = (rowp * 2 + d) * 3 * Hp;
    const float4 dy = ld4(p.dy + rowp * p.dy_ld + (size_t)d * p.dy_dstride + jg);
    const float4 g = make_float4(dy.x + carry.x, dy.y + carry.y, dy.z + carry.z, dy.w + carry.w);
    const float4 z = ld4(p.gates + og + jg), hh = ld4(p.gates + og + 2 * Hp + jg);
    const float4 hp = s - 1 > 0 ? ld4(p.h + (((size_t)tpp * n_pad + n0 + en) * 2 + d) * Hp + jg)
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
struct GruPlan {
  int NR, J, NBT, blocks;
  size_t ut_bytes, vec_bytes;
};

int make_gru_plan(const asr_gru_args* a, bool bwd, GruPlan* pl) {
  const int rc = rec_check_args("gru", a, false);
  if (rc != ASR_OK) return rc;
  pl->NR = rec_rows(a->n_pad);
  pl->J = 1024 / pl->NR;
  pl->NBT = a->n_pad / pl->NR;
  // the widest launch: forward phase A has 2H output columns, every other phase H
  pl->blocks = ((bwd ? a->H : 2 * a->H) + pl->J - 1) / pl->J * pl->NBT * 2;
  pl->ut_bytes = bwd ? asr_align_up((size_t)2 * 3 * a->H * a->H * sizeof(float), 256) : 0;
  pl->vec_bytes = bwd ? asr_align_up((size_t)a->n_pad * 2 * a->H * sizeof(float), 256) : 0;
  return ASR_OK;
}

size_t gru_ws_bytes(const GruPlan& pl) { return 256 + pl.ut_bytes + 2 * pl.vec_bytes; }

template <int NR>
int gru_launch(int ph, const GruParams& p, int ncols, int nbt, hipStream_t stream) {
  constexpr int J = RecTile<NR>::J;
  const dim3 grid((ncols + J - 1) / J, nbt, 2);
  switch (ph) {
    case kFwdA: hipLaunchKernelGGL((gru_step_kernel<NR, kFwdA>), grid, dim3(kThreads), 0, stream, p); break;
    case kFwdB: hipLaunchKernelGGL((gru_step_kernel<NR, kFwdB>), grid, dim3(kThreads), 0, stream, p); break;
    case kBwdA: hipLaunchKernelGGL((gru_step_kernel<NR, kBwdA>), grid, dim3(kThreads), 0, stream, p); break;
    default:    hipLaunchKernelGGL((gru_step_kernel<NR, kBwdB>), grid, dim3(kThreads), 0, stream, p); break;
  }
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

int gru_phase(const GruPlan& pl, int ph, const GruParams& p, int ncols, hipStream_t stream) {
  return rec_with_rows(pl.NR, [&](auto nr) {
    return gru_launch<decltype(nr)::value>(ph, p, ncols, pl.NBT, stream);
  });
}

int gru_run(const asr_gru_args* a, bool bwd, void* workspace, size_t ws_bytes, hipStream_t stream) {
  GruPlan pl;
  int rc = make_gru_plan(a, bwd, &pl);
  if (rc != ASR_OK) return rc;
  const size_t need = gru_ws_bytes(pl);
  ASR_CHECK_ARG(workspace != nullptr && ws_bytes >= need, "gru: workspace %zu bytes < %zu",
                ws_bytes, need);
  ASR_CHECK_ARG(a->U && a->h && a->gates, "gru: U, h and gates are required");
  if (bwd) ASR_CHECK_ARG(a->dy && a->da && a->dy_ld >= a->H && a->dy_ld % 4 == 0 &&
                         a->dy_dir_stride % 4 == 0,
                         "gru: BPTT needs dy (dy_ld >= H, a multiple of 4) and da");
  else ASR_CHECK_ARG(a->zx && a->rm, "gru: the forward pass needs zx and rm");
  char* ws = static_cast<char*>(workspace);
  const int H = a->H, T = a->T;
  GruParams p;
  p.T = T; p.n_pad = a->n_pad; p.Hp = H;
  p.act = a->activation; p.clip = a->clip;
  p.mask_u = a->mask_u; p.zx = a->zx; p.h = a->h; p.gates = a->gates; p.rm = a->rm;
  p.dy = a->dy; p.dy_ld = a->dy_ld; p.dy_dstride = a->dy_dir_stride;
  p.da = a->da;
  p.gbuf = reinterpret_cast<float*>(ws + 256 + pl.ut_bytes);
  p.qr = reinterpret_cast<float*>(ws + 256 + pl.ut_bytes + pl.vec_bytes);
  if (!bwd) {
    p.U = a->U;
    for (int s = 0; s < T; ++s) {
      p.s = s;
      if ((rc = gru_phase(pl, kFwdA, p, 2 * H, stream)) != ASR_OK) return rc;
      if ((rc = gru_phase(pl, kFwdB, p, H, stream)) != ASR_OK) return rc;
    }
    if (a->y_sum) return rec_sum(a->h, a->y_sum, (long long)T * a->n_pad, H, stream);
    return ASR_OK;
  }
  float* Ut = reinterpret_cast<float*>(ws + 256);
  if ((rc = rec_transpose(a->U, Ut, 2, H, 3 * H, stream)) != ASR_OK) return rc;
  p.U = Ut;
  // phase B of step s also prepares da_h, da_z of step s - 1: s = T is the prologue (carry 0)
  p.s = T;
  if ((rc = gru_phase(pl, kBwdB, p, H, stream)) != ASR_OK) return rc;
  for (int s = T - 1; s >= 0; --s) {
    p.s = s;
    if ((rc = gru_phase(pl, kBwdA, p, H, stream)) != ASR_OK) return rc;
    if (s > 0 && (rc = gru_phase(pl, kBwdB, p, H, stream)) != ASR_OK) return rc;
  }
  if (a->db_part || a->dz_absmax)
    return rec_dbias(a->da, a->db_part, a->dz_absmax, T, a->n_pad, 1, 3 * H, stream);
  return ASR_OK;
}

}  // namespace

extern "C" size_t asr_gru_workspace_bytes(const asr_gru_args* a, int backward) {
  GruPlan pl;
  if (make_gru_plan(a, backward != 0, &pl) != ASR_OK) return 0;
  return gru_ws_bytes(pl);
}

extern "C" int asr_gru_seq_fwd(const asr_gru_args* a, void* workspace, size_t ws_bytes,
                               asr_stream_t stream) {
  return gru_run(a, false, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int asr_gru_seq_bwd(const asr_gru_args* a, void* workspace, size_t ws_bytes,
                               asr_stream_t stream) {
  return gru_run(a, true, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int asr_gru_plan(const asr_gru_args* a, int backward, int* persistent, int* rows,
                            int* units, int* blocks) {
  GruPlan pl;
  const int rc = make_gru_plan(a, backward != 0, &pl);
  if (rc != ASR_OK) return rc;
  if (persistent) *persistent = 0;
  if (rows) *rows = pl.NR;
  if (units) *units = pl.J;
  if (blocks) *blocks = pl.blocks;
  return ASR_OK;
}
