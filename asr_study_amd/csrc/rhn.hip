// rhn.hip -- the Recurrent Highway Network recurrence (Zilly et al. 2016, the reference's RHN
// layer) of a Bidirectional layer (K17, include/asr_hip.h), forward and BPTT, both directions per
// launch.  Per direction, in processing order, depth L, C = 2 (coupled) or 3 column blocks
// h | t | [c], hs(a) = clip(0.2 a + 0.5, 0, 1), s the state carried in (0 at the first frame):
//   for l in 0 .. L-1:
//     a  = (l == 0 ? zx_t : 0) + (s (.) B_U[l]) U_l + b_l
//     hh = act(a_h)   tg = hs(a_t)   cg = coupled ? 1 - tg : hs(a_c)
//     s  = hh tg + s cg                                  (the carry uses the UNMASKED s)
//   y_t = s
// zx = x @ W comes from the GEMMs, and so do dW, dU_l, dx; this file owns the sequential part.
//
// A time step is L micro-steps, each with ONE reduction, so the stepwise form is one launch per
// micro-step: L T launches forward; BPTT a prologue (the element-wise head of the last micro-step)
// and L T - 1 reductions, each of which forms, in its epilogue, the gradient of the state below
// and from it the da of the level below (the previous frame's level L-1 when l = 0: that is where
// dy enters).  There is no persistent form (asr_rhn_args.mode 2 is an argument error).
//
// Geometry and reduction: RecTile of rec_tile.h (NR batch rows x J tile columns per workgroup,
// chunked operand in LDS, 4 x 4 register tiles, fixed-order cross-wave sum).
// Its own: the forward epilogue needs a_h, a_t (and a_c) of the SAME column, so the J tile
// columns are G groups of JB = J / G neighbouring columns, group g taken from block g of U_l:
// G = 2 when coupled; G = 4 with the fourth group idle when not (J is no multiple of 3).  The
// forward pass reads a copy of U made once per call in the workspace, in which the C JB columns
// of a tile lie side by side (a row of a tile is then one 48 / 64-byte piece instead of C pieces
// Hp floats apart; measured faster than index arithmetic into U itself).  BPTT
// reduces da^l (C H long) against U_l^T (copied once per call as well) with J plain columns.
// The slopes of BPTT are read from the SAVED gates (hs' = 0.2 on 0 < gate < 1, else 0; act' from
// hh alone).
#include "rec_tile.h"

namespace {

enum { kFwd = 0, kBwd = 1 };

struct RhnParams {
  int T, n_pad, Hp, L;
  int act;
  float clip;
  int s, l;                // the FORWARD step and level this launch belongs to (kBwd: s = T is the
                           // prologue, which reduces nothing)
  const float* U;          // fwd: the tile-interleaved copy (2, L, Hp, tiles C JB); BPTT: U^T
                           // (2, L, C Hp, Hp)
  const float* b;          // (2, L, C Hp)
  const float* mask_u;     // (2, L, n_pad, Hp) or null
  const float* zx;         // fwd (T, n_pad, 2, C Hp)
  float* h;                // (L, T, n_pad, 2, Hp)
  float* gates;            // (L, T, n_pad, 2, C Hp): hh | tg | [cg]
  const float* dy;         // BPTT
  long long dy_ld;
  int dy_dstride;
  float* da;               // BPTT (L, T, n_pad, 2, C Hp)
  float* gbuf;             // BPTT workspace (n_pad, 2, Hp): gradient of the state last formed
};

// da of one level from the gradient g of the state it wrote, its saved gates and the state sp it
// read; written to the C blocks at `o` (block stride Hp)
template <int C>
__device__ __forceinline__ void rhn_da(const RhnParams& p, float* o, float4 g, float4 sp) {
  const int Hp = p.Hp;
  const float4 hh = ld4(p.gates + (o - p.da)), tg = ld4(p.gates + (o - p.da) + Hp);
  st4(o, make_float4(g.x * tg.x * rec_slope(p.act, p.clip, hh.x),
                     g.y * tg.y * rec_slope(p.act, p.clip, hh.y),
                     g.z * tg.z * rec_slope(p.act, p.clip, hh.z),
                     g.w * tg.w * rec_slope(p.act, p.clip, hh.w)));
  if (C == 2) {
    st4(o + Hp, make_float4(g.x * (hh.x - sp.x) * hs_slope(tg.x), g.y * (hh.y - sp.y) * hs_slope(tg.y),
                            g.z * (hh.z - sp.z) * hs_slope(tg.z), g.w * (hh.w - sp.w) * hs_slope(tg.w)));
  } else {
    const float4 cg = ld4(p.gates + (o - p.da) + 2 * Hp);
    st4(o + Hp, make_float4(g.x * hh.x * hs_slope(tg.x), g.y * hh.y * hs_slope(tg.y),
                            g.z * hh.z * hs_slope(tg.z), g.w * hh.w * hs_slope(tg.w)));
    st4(o + 2 * Hp, make_float4(g.x * sp.x * hs_slope(cg.x), g.y * sp.y * hs_slope(cg.y),
                                g.z * sp.z * hs_slope(cg.z), g.w * sp.w * hs_slope(cg.w)));
  }
}

template <int NR, int PH, int C>
__global__ void __launch_bounds__(kThreads)
rhn_step_kernel(RhnParams p) {
  using Tile = RecTile<NR>;
  constexpr int J = Tile::J;
  constexpr int G = PH == kFwd ? (C == 2 ? 2 : 4) : 1;     // column groups of the tile
  constexpr int JB = J / G;                                // neighbouring columns per group
  __shared__ __attribute__((aligned(16))) float lds[Tile::kLdsFloats];

  const int tid = threadIdx.x;
  const int jb = blockIdx.x, nt = blockIdx.y, d = blockIdx.z;
  const int Hp = p.Hp, n_pad = p.n_pad, T = p.T, L = p.L, s = p.s, l = p.l;
  const int j0 = jb * JB, n0 = nt * NR;
  const int W = C * Hp;                    // gate row of one direction
  const float* mu = p.mask_u ? p.mask_u + (((size_t)d * L + l) * n_pad + n0) * Hp : nullptr;
  // no reduction: the first forward micro-step reads the state 0 (the product is 0), and the
  // BPTT prologue (s = T) has nothing above it
  const bool skip = PH == kFwd ? (s == 0 && l == 0) : s >= T;
  // frame of forward step s of this direction (d = 1 walks time downwards), and of s - 1; frames
  // that do not exist (the prologue's own, the one before the first) are never read: their
  // indices are held at a valid frame so that no address is formed outside the slabs
  const int t = (PH == kBwd && skip) ? 0 : (d == 0 ? s : T - 1 - s);
  const int tp = d == 0 ? t - 1 : t + 1;
  // the state level l reads: level l - 1 of the same frame, or level L - 1 of the frame before
  const int lr = l > 0 ? l - 1 : L - 1, tr = (l > 0 || skip) ? t : tp;
  const size_t row0 = ((size_t)l * T + t) * n_pad + n0;
  const size_t rowr0 = ((size_t)lr * T + tr) * n_pad + n0;

  const float* op = nullptr;
  const float* mat = nullptr;
  size_t op_ld = 0;
  int K = Hp, ldm = Hp;
  if (PH == kFwd) {
    op = p.h + (rowr0 * 2 + d) * Hp; op_ld = 2 * (size_t)Hp;
    ldm = (int)gridDim.x * C * JB;                          // tiles x (C groups of JB columns)
    mat = p.U + ((size_t)d * L + l) * Hp * ldm;
  } else {
    op = p.da + (row0 * 2 + d) * W; op_ld = 2 * (size_t)W;
    mat = p.U + ((size_t)d * L + l) * W * Hp; K = W;
  }

  // epilogue ownership: row en, columns ej .. ej + 3 of a group (forward: NR * JB / 4 threads)
  const int en = (4 * tid) / JB, ej = (4 * tid) % JB;
  const int jg = j0 + ej;
  const bool eown = en < NR && jg < Hp;

  float4 r[PH == kFwd ? C : 1];
#pragma unroll
  for (int g = 0; g < (PH == kFwd ? C : 1); ++g) r[g] = zero4();
  if (!skip) {
    float acc[4][4];
    // tile column jj = group g, column jc of it: block g of U_l, column j0 + jc (forward: at
    // jb C JB + g JB + jc of the interleaved copy)
    auto ucol = [&](int jj) {
      const int g = jj / JB, jc = jj % JB;
      if (g >= C || j0 + jc >= Hp) return -1;
      return PH == kFwd ? jb * (C * JB) + g * JB + jc : j0 + jc;
    };
    // forward: m = s (.) B_U[l]
    Tile::template reduce<PH == kFwd>(lds, op, op_ld, K, mat, ldm, mu, Hp, ucol, acc);
    Tile::spill(lds, acc);
    if (en < NR) {
#pragma unroll
      for (int g = 0; g < (PH == kFwd ? C : 1); ++g) r[g] = Tile::total(lds, en, g * JB + ej);
    }
  }
  if (!eown) return;

  if (PH == kFwd) {
    const size_t row = row0 + en;
    const size_t og = (row * 2 + d) * W + jg;
    const float* b = p.b + ((size_t)d * L + l) * W + jg;
    const float* zx = p.zx + (((size_t)t * n_pad + n0 + en) * 2 + d) * W + jg;
    float4 a[C];
#pragma unroll
    for (int g = 0; g < C; ++g) {
      a[g] = add4(r[g], ld4(b + g * Hp));
      if (l == 0) a[g] = add4(a[g], ld4(zx + g * Hp));
    }
    const float4 sp = skip ? zero4() : ld4(p.h + ((rowr0 + en) * 2 + d) * Hp + jg);
    const float4 hh = make_float4(rec_act(p.act, p.clip, a[0].x), rec_act(p.act, p.clip, a[0].y),
                                  rec_act(p.act, p.clip, a[0].z), rec_act(p.act, p.clip, a[0].w));
    const float4 tg = make_float4(hard_sigmoid(a[1].x), hard_sigmoid(a[1].y),
                                  hard_sigmoid(a[1].z), hard_sigmoid(a[1].w));
    float4 cg;
    if (C == 2) cg = make_float4(1.f - tg.x, 1.f - tg.y, 1.f - tg.z, 1.f - tg.w);
    else cg = make_float4(hard_sigmoid(a[C - 1].x), hard_sigmoid(a[C - 1].y),
                          hard_sigmoid(a[C - 1].z), hard_sigmoid(a[C - 1].w));
    st4(p.gates + og, hh);
    st4(p.gates + og + Hp, tg);
    if (C == 3) st4(p.gates + og + 2 * Hp, cg);
    st4(p.h + (row * 2 + d) * Hp + jg,
        make_float4(hh.x * tg.x + sp.x * cg.x, hh.y * tg.y + sp.y * cg.y,
                    hh.z * tg.z + sp.z * cg.z, hh.w * tg.w + sp.w * cg.w));
  } else {
    const size_t ow = ((size_t)(n0 + en) * 2 + d) * Hp + jg;
    // the level below, whose da this epilogue forms: (l - 1, s), or (L - 1, s - 1) under level 0;
    // the prologue forms the last micro-step's
    const int lb = (s >= T || l == 0) ? L - 1 : l - 1;
    const int sb = s >= T ? T - 1 : (l == 0 ? s - 1 : s);
    const int tb = d == 0 ? sb : T - 1 - sb;
    const int tbp = d == 0 ? tb - 1 : tb + 1;
    float4 g = zero4();
    if (s < T) {
      // gradient of the state level l read: g cg + (da U_l^T) (.) B_U[l]
      const size_t og = ((row0 + en) * 2 + d) * W + jg;
      float4 cg;
      if (C == 2) {
        const float4 tg = ld4(p.gates + og + Hp);
        cg = make_float4(1.f - tg.x, 1.f - tg.y, 1.f - tg.z, 1.f - tg.w);
      } else {
        cg = ld4(p.gates + og + 2 * Hp);
      }
      float4 dm = r[0];
      if (mu != nullptr) dm = mul4(dm, ld4(mu + (size_t)en * Hp + jg));
      const float4 gw = ld4(p.gbuf + ow);
      g = make_float4(gw.x * cg.x + dm.x, gw.y * cg.y + dm.y, gw.z * cg.z + dm.z,
                      gw.w * cg.w + dm.w);
    }
    const size_t nb = (size_t)tb * n_pad + n0 + en;
    if (lb == L - 1)                                    // the layer output: dy enters
      g = add4(g, ld4(p.dy + nb * p.dy_ld + (size_t)d * p.dy_dstride + jg));
    // the state level lb read
    float4 sp = zero4();
    if (lb > 0) sp = ld4(p.h + ((((size_t)(lb - 1) * T + tb) * n_pad + n0 + en) * 2 + d) * Hp + jg);
    else if (sb > 0) sp = ld4(p.h + ((((size_t)(L - 1) * T + tbp) * n_pad + n0 + en) * 2 + d) * Hp + jg);
    rhn_da<C>(p, p.da + ((((size_t)lb * T + tb) * n_pad + n0 + en) * 2 + d) * W + jg, g, sp);
    st4(p.gbuf + ow, g);
  }
}

// U (Z, Hp, C Hp), blocks h | t | [c] -> (Z, Hp, tiles C JB): per tile of JB state columns its C
// groups side by side (zeros past Hp); Z = 2 L, n = all floats of the copy
__global__ void rhn_interleave_kernel(const float* __restrict__ U, float* __restrict__ Ui, int Hp, int C,
                               int JB, long long n) {
  const int ld = (Hp + JB - 1) / JB * C * JB;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const long long zk = i / ld;
    const int c = (int)(i % ld);
    const int jbk = c / (C * JB), g = (c % (C * JB)) / JB, jc = c % JB;
    const int j = jbk * JB + jc;
    Ui[i] = j < Hp ? U[zk * (C * Hp) + g * Hp + j] : 0.f;
  }
}

// ---- host side -------------------------------------------------------------------------------
// ut_bytes: the copy of U (forward: interleaved, BPTT: U^T); vec_bytes: gbuf
struct RhnPlan : RecPlan {
  int JB, C;                              // a workgroup's units; column blocks per unit
  size_t ui_floats;
};

int make_rhn_plan(const asr_rhn_args* a, bool bwd, RhnPlan* pl) {
  const int rc = rec_check_args("rhn", a, false);
  if (rc != ASR_OK) return rc;
  ASR_CHECK_ARG(a->depth >= 1, "rhn: depth %d < 1", a->depth);
  ASR_CHECK_ARG(a->coupling == 0 || a->coupling == 1, "rhn: coupling %d (0 or 1)", a->coupling);
  // a forward workgroup owns JB = J / k units (their C <= k column blocks fill its J tile columns)
  const int k = bwd ? 1 : (a->coupling ? 2 : 4);
  static_cast<RecPlan&>(*pl) = rec_plan(a->n_pad, k * a->H, 2);
  pl->C = a->coupling ? 2 : 3;
  pl->JB = pl->J / k;
  pl->ut_bytes = bwd ? asr_align_up((size_t)2 * a->depth * pl->C * a->H * a->H * sizeof(float), 256) : 0;
  pl->ui_floats = (size_t)2 * a->depth * a->H * ((a->H + pl->JB - 1) / pl->JB * pl->C * pl->JB);
  if (!bwd) pl->ut_bytes = asr_align_up(pl->ui_floats * sizeof(float), 256);
  pl->vec_bytes = bwd ? asr_align_up((size_t)a->n_pad * 2 * a->H * sizeof(float), 256) : 0;
  return ASR_OK;
}

size_t rhn_ws_bytes(const RhnPlan& pl) { return 256 + pl.ut_bytes + pl.vec_bytes; }

template <int NR, int C>
int rhn_launch(bool bwd, const RhnParams& p, int jb, int nbt, hipStream_t stream) {
  const dim3 grid((p.Hp + jb - 1) / jb, nbt, 2);
  if (bwd) hipLaunchKernelGGL((rhn_step_kernel<NR, kBwd, C>), grid, dim3(kThreads), 0, stream, p);
  else hipLaunchKernelGGL((rhn_step_kernel<NR, kFwd, C>), grid, dim3(kThreads), 0, stream, p);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

template <int C>
int rhn_step_c(const RhnPlan& pl, bool bwd, const RhnParams& p, hipStream_t stream) {
  return rec_with_rows(pl.NR, [&](auto nr) {
    return rhn_launch<decltype(nr)::value, C>(bwd, p, pl.JB, pl.NBT, stream);
  });
}

int rhn_step(const RhnPlan& pl, bool bwd, const RhnParams& p, hipStream_t stream) {
  return pl.C == 2 ? rhn_step_c<2>(pl, bwd, p, stream) : rhn_step_c<3>(pl, bwd, p, stream);
}

int rhn_run(const asr_rhn_args* a, bool bwd, void* workspace, size_t ws_bytes, hipStream_t stream) {
  RhnPlan pl;
  int rc = make_rhn_plan(a, bwd, &pl);
  if (rc != ASR_OK) return rc;
  if ((rc = rec_check_ws("rhn", workspace, ws_bytes, rhn_ws_bytes(pl))) != ASR_OK) return rc;
  ASR_CHECK_ARG(a->U && a->h && a->gates, "rhn: U, h and gates are required");
  if (bwd) ASR_CHECK_ARG(a->dy && a->da && a->dy_ld >= a->H && a->dy_ld % 4 == 0 &&
                         a->dy_dir_stride % 4 == 0,
                         "rhn: BPTT needs dy (dy_ld >= H, a multiple of 4) and da");
  else ASR_CHECK_ARG(a->zx && a->b, "rhn: the forward pass needs zx and b");
  char* ws = static_cast<char*>(workspace);
  const int H = a->H, T = a->T, L = a->depth, W = pl.C * H;
  RhnParams p;
  p.T = T; p.n_pad = a->n_pad; p.Hp = H; p.L = L;
  p.act = a->activation; p.clip = a->clip;
  p.b = a->b; p.mask_u = a->mask_u; p.zx = a->zx; p.h = a->h; p.gates = a->gates;
  p.dy = a->dy; p.dy_ld = a->dy_ld; p.dy_dstride = a->dy_dir_stride;
  p.da = a->da;
  p.gbuf = reinterpret_cast<float*>(ws + 256 + pl.ut_bytes);
  if (!bwd) {
    float* Ui = reinterpret_cast<float*>(ws + 256);
    const int nblk = (int)((pl.ui_floats + 255) / 256 < 2048 ? (pl.ui_floats + 255) / 256 : 2048);
    hipLaunchKernelGGL(rhn_interleave_kernel, dim3(nblk), dim3(256), 0, stream, a->U, Ui, H, pl.C,
                       pl.JB, (long long)pl.ui_floats);
    ASR_CHECK_LAUNCH();
    p.U = Ui;
    for (int s = 0; s < T; ++s)
      for (int l = 0; l < L; ++l) {
        p.s = s; p.l = l;
        if ((rc = rhn_step(pl, false, p, stream)) != ASR_OK) return rc;
      }
    if (a->y_sum) {
      const long long rows = (long long)T * a->n_pad;
      return rec_sum(a->h + (size_t)(L - 1) * rows * 2 * H, a->y_sum, rows, H, stream);
    }
    return ASR_OK;
  }
  float* Ut = reinterpret_cast<float*>(ws + 256);
  if ((rc = rec_transpose(a->U, Ut, 2 * L, H, W, stream)) != ASR_OK) return rc;
  p.U = Ut;
  // every launch also forms the da of the level below: s = T is the prologue (nothing above)
  p.s = T; p.l = 0;
  if ((rc = rhn_step(pl, true, p, stream)) != ASR_OK) return rc;
  for (int s = T - 1; s >= 0; --s)
    for (int l = L - 1; l >= 0; --l) {
      if (s == 0 && l == 0) break;                      // nothing below the first micro-step
      p.s = s; p.l = l;
      if ((rc = rhn_step(pl, true, p, stream)) != ASR_OK) return rc;
    }
  if (a->db_part || a->dz_absmax)
    return rec_dbias(a->da, a->db_part, a->dz_absmax, T, a->n_pad, L, W, stream);
  return ASR_OK;
}

}  // namespace

extern "C" size_t asr_rhn_workspace_bytes(const asr_rhn_args* a, int backward) {
  RhnPlan pl;
  if (make_rhn_plan(a, backward != 0, &pl) != ASR_OK) return 0;
  return rhn_ws_bytes(pl);
}

extern "C" int asr_rhn_seq_fwd(const asr_rhn_args* a, void* workspace, size_t ws_bytes,
                               asr_stream_t stream) {
  return rhn_run(a, false, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int asr_rhn_seq_bwd(const asr_rhn_args* a, void* workspace, size_t ws_bytes,
                               asr_stream_t stream) {
  return rhn_run(a, true, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int asr_rhn_plan(const asr_rhn_args* a, int backward, int* persistent, int* rows,
                            int* units, int* blocks) {
  RhnPlan pl;
  const int rc = make_rhn_plan(a, backward != 0, &pl);
  if (rc != ASR_OK) return rc;
  return rec_plan_out(pl, pl.JB, persistent, rows, units, blocks);
}
