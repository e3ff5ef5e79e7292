// lstm_uni.hip -- the UNIDIRECTIONAL LSTM recurrence with a carried state (K29, DESIGN.md §29;
// asr_lstm_uni_*): a bare LSTM(H)(x), frames 0 .. T-1 in order.  The plain cell of the reference
// (core/layers.py:432-469 without mi, zoneout or layer normalisation), with m = h_prev (.) B_U:
//     z = zx + m @ U        zx = (x (.) B_W) @ W + b from the GEMM
//     i, f, o = hard_sigmoid(z_i, z_f, z_o)      g = act(z_c)
//     c = f c_prev + i g    h = o act(c)
// This is NOT the persistent hand-off kernel of lstm_fwd.hip / lstm_bwd.hip (two directions per
// launch, split-fp16 MFMA, h0 = c0 = 0): it is a stepwise kernel on the reduction core of
// rec_tile.h -- one launch per frame in either pass, exact fp32 FMAs in a fixed order, no float
// atomics, no workgroup waiting on another.
//
// Layouts are the project's LSTM gate layout, unit-major / gate-minor, without a direction axis:
// U (H, 4H) as [k][unit * 4 + gate], gates i, f, c, o; zx, gates, dz (T, n_pad, 4H); h, cell
// (T, n_pad, H).  A float4 of four tile columns is then one unit's four gates, so the thread that
// owns it in the forward epilogue needs nothing from another thread.
//
// Forward, frame t: the operand is h[t - 1] (masked while it is staged) against the 4H columns
// of U; the epilogue reads zx and c[t - 1] and writes gates (post-activation, for BPTT), cell, h.
// Frame 0 reads the state (h0, c0) through the same pointer-and-stride code that reads h[t - 1],
// cell[t - 1] at t > 0 (null: zeros, and the product is skipped), and the epilogue of the launch
// for t = T - 1 stores h and c a second time into (h_last, c_last): a sequence cut into two
// calls is the one call bit for bit.
//
// BPTT, frame t (T - 1 down to 0): dz[t + 1] (K = 4H) against U^T (4H, H), transposed once per
// call.  The thread that owns (row, units j .. j + 3) forms dh = dy[t] + product (.) B_U and
// dc = dc_carry + dh o act'(act(c)), writes the sixteen dz[t] of its four units and hands
// dc_carry = dc f on through a (n_pad, H) workspace vector that the same thread reads in the
// next launch.  The launch for t = T - 1 skips the product.  Slopes come from the SAVED values:
// hs' from the saved gate, act' from the saved g and from act(c) recomputed from cell.
#include "rec_tile.h"

namespace {

constexpr int kLstmUniActs = 7;            // ids 0 .. 6 of asr_lstm_args.activation

struct LstmUniParams {
  int T, n_pad, H;
  int act;
  int t;                   // the frame of this launch
  const float* U;          // fwd: U (H, 4H); BPTT: U^T (4H, H)
  const float* mask_u;     // (n_pad, H) or null
  const float* zx;         // fwd (T, n_pad, 4H)
  float* h;                // (T, n_pad, H)
  float* cell;             // (T, n_pad, H)
  float* gates;            // (T, n_pad, 4H): i, f, g, o per unit
  const float* h0;         // fwd: (n_pad, H) state before frame 0, or null (zeros); c0 with it
  const float* c0;
  float* h_last;           // fwd: (n_pad, H) <- h[T - 1], or null; c_last with it
  float* c_last;
  const float* dy;         // BPTT
  long long dy_ld;
  float* dz;               // BPTT (T, n_pad, 4H)
  float* dc;               // BPTT workspace (n_pad, H): dc (.) f of the frame after
};

template <int NR>
__global__ void __launch_bounds__(kThreads)
lstm_uni_fwd_kernel(LstmUniParams p) {
  using Tile = RecTile<NR>;
  constexpr int J = Tile::J;
  __shared__ __attribute__((aligned(16))) float lds[Tile::kLdsFloats];

  const int tid = threadIdx.x;
  const int H = p.H, G = 4 * p.H, n_pad = p.n_pad, t = p.t;
  const int j0 = blockIdx.x * J, n0 = blockIdx.y * NR;
  const size_t row0 = (size_t)t * n_pad + n0;
  // the state the frame starts from, rows n0 .. of (., H) at stride H: frame t - 1 of the
  // slabs or, at frame 0, (h0, c0); null: zeros
  const float* hprev = nullptr;
  const float* cprev = nullptr;
  if (t > 0) {
    hprev = p.h + (row0 - n_pad) * H; cprev = p.cell + (row0 - n_pad) * H;
  } else if (p.h0 != nullptr) {
    hprev = p.h0 + (size_t)n0 * H; cprev = p.c0 + (size_t)n0 * H;
  }

  // epilogue ownership: row en, tile columns ej .. ej + 3 = the four gates of unit u
  const int en = (4 * tid) / J, ej = (4 * tid) % J;
  const int jg = j0 + ej;

  float4 r = zero4();
  if (hprev != nullptr) {                  // (block-uniform)
    float acc[4][4];
    Tile::template reduce<true>(           // m = h_prev (.) B_U
        lds, hprev, (size_t)H, H, p.U, G, p.mask_u ? p.mask_u + (size_t)n0 * H : nullptr, H,
        [&](int jj) { return j0 + jj < G ? j0 + jj : -1; }, acc);
    Tile::spill(lds, acc);
    r = Tile::total(lds, en, ej);
  }
  if (jg >= G) return;

  const size_t row = row0 + en;
  const int u = jg >> 2;
  const float4 zx = ld4(p.zx + row * G + jg);
  const float i = hard_sigmoid(zx.x + r.x), f = hard_sigmoid(zx.y + r.y);
  const float g = asr_act_apply(p.act, zx.z + r.z), o = hard_sigmoid(zx.w + r.w);
  const float cp = cprev != nullptr ? cprev[(size_t)en * H + u] : 0.f;
  const float c = f * cp + i * g;
  const float hn = o * asr_act_apply(p.act, c);
  st4(p.gates + row * G + jg, make_float4(i, f, g, o));
  p.cell[row * H + u] = c;
  p.h[row * H + u] = hn;
  if (t == p.T - 1 && p.h_last != nullptr) {
    p.h_last[(size_t)(n0 + en) * H + u] = hn;
    p.c_last[(size_t)(n0 + en) * H + u] = c;
  }
}

template <int NR>
__global__ void __launch_bounds__(kThreads)
lstm_uni_bwd_kernel(LstmUniParams p) {
  using Tile = RecTile<NR>;
  constexpr int J = Tile::J;
  __shared__ __attribute__((aligned(16))) float lds[Tile::kLdsFloats];

  const int tid = threadIdx.x;
  const int H = p.H, G = 4 * p.H, n_pad = p.n_pad, t = p.t;
  const int j0 = blockIdx.x * J, n0 = blockIdx.y * NR;
  const size_t row0 = (size_t)t * n_pad + n0;
  const bool last = t == p.T - 1;          // no frame after it: dh = dy, dc_carry = 0

  // epilogue ownership: row en, units jg .. jg + 3
  const int en = (4 * tid) / J, ej = (4 * tid) % J;
  const int jg = j0 + ej;

  float4 r = zero4();
  if (!last) {
    float acc[4][4];
    Tile::template reduce<false>(
        lds, p.dz + (row0 + n_pad) * G, (size_t)G, G, p.U, H, nullptr, 0,
        [&](int jj) { return j0 + jj < H ? j0 + jj : -1; }, acc);
    Tile::spill(lds, acc);
    r = Tile::total(lds, en, ej);
  }
  if (jg >= H) return;

  const size_t row = row0 + en;
  const size_t ow = (size_t)(n0 + en) * H + jg;
  if (p.mask_u != nullptr) r = mul4(r, ld4(p.mask_u + ow));
  const float4 dh = add4(ld4(p.dy + row * p.dy_ld + jg), r);
  const float4 c = ld4(p.cell + row * H + jg);
  const float4 cp = t > 0 ? ld4(p.cell + (row - n_pad) * H + jg) : zero4();
  const float4 carry = last ? zero4() : ld4(p.dc + ow);
  float nc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 gt = ld4(p.gates + row * G + 4 * (jg + k));       // i, f, g, o of unit jg + k
    const float dhk = f4get(dh, k);
    const float tc = asr_act_apply(p.act, f4get(c, k));
    const float dc = f4get(carry, k) + dhk * gt.w * asr_act_slope(p.act, tc);
    st4(p.dz + row * G + 4 * (jg + k),
        make_float4(dc * gt.z * hs_slope(gt.x), dc * f4get(cp, k) * hs_slope(gt.y),
                    dc * gt.x * asr_act_slope(p.act, gt.z), dhk * tc * hs_slope(gt.w)));
    nc[k] = dc * gt.y;
  }
  st4(p.dc + ow, make_float4(nc[0], nc[1], nc[2], nc[3]));
}

// ---- host side -------------------------------------------------------------------------------
// the checks every entry point starts with (the plan and the workspace size too): those of
// rec_check_args under the LSTM's activation ids, then the state pairs
int lstm_uni_check(const asr_lstm_uni_args* a) {
  const int rc = rec_check_args("lstm_uni", a, false,
                                [](const char* pfx, const asr_lstm_uni_args* a) -> int {
    ASR_CHECK_ARG(a->activation >= 0 && a->activation < kLstmUniActs, "%s: activation id %d (0 "
                  "tanh, 1 relu, 2 sigmoid, 3 hard_sigmoid, 4 linear, 5 softsign, 6 softplus)", pfx,
                  a->activation);
    return ASR_OK;
  });
  if (rc != ASR_OK) return rc;
  ASR_CHECK_ARG((a->h0 == nullptr) == (a->c0 == nullptr), "lstm_uni: h0 and c0 come together "
                "(both, or neither for the zero state)");
  ASR_CHECK_ARG((a->h_last == nullptr) == (a->c_last == nullptr), "lstm_uni: h_last and c_last "
                "come together (both or neither)");
  ASR_CHECK_ARG(a->h_last == nullptr ||
                (a->h_last != a->c_last && a->h_last != a->h0 && a->h_last != a->c0 &&
                 a->c_last != a->h0 && a->c_last != a->c0),
                "lstm_uni: h_last / c_last alias h0 / c0 or each other (a call leaves the state "
                "it starts from intact: keep two buffers of each and swap them)");
  return ASR_OK;
}

RecPlan make_lstm_uni_plan(const asr_lstm_uni_args* a, bool bwd) {
  // forward: 4H gate columns; BPTT: H units
  RecPlan pl = rec_plan(a->n_pad, bwd ? a->H : 4 * a->H, 1);
  if (bwd) {
    pl.ut_bytes = asr_align_up((size_t)4 * a->H * a->H * sizeof(float), 256);
    pl.vec_bytes = asr_align_up((size_t)a->n_pad * a->H * sizeof(float), 256);
  }
  return pl;
}

size_t lstm_uni_ws_bytes(const RecPlan& pl) { return 256 + pl.ut_bytes + pl.vec_bytes; }

template <int NR>
int lstm_uni_launch(bool bwd, const LstmUniParams& p, int nbt, hipStream_t stream) {
  constexpr int J = RecTile<NR>::J;
  const dim3 grid(((bwd ? p.H : 4 * p.H) + J - 1) / J, nbt);
  if (bwd) hipLaunchKernelGGL(lstm_uni_bwd_kernel<NR>, grid, dim3(kThreads), 0, stream, p);
  else hipLaunchKernelGGL(lstm_uni_fwd_kernel<NR>, grid, dim3(kThreads), 0, stream, p);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

// every argument error is refused here, before the first device call
int lstm_uni_run(const asr_lstm_uni_args* a, bool bwd, void* workspace, size_t ws_bytes,
                 hipStream_t stream) {
  int rc = lstm_uni_check(a);
  if (rc != ASR_OK) return rc;
  const RecPlan pl = make_lstm_uni_plan(a, bwd);
  if ((rc = rec_check_ws("lstm_uni", workspace, ws_bytes, lstm_uni_ws_bytes(pl))) != ASR_OK)
    return rc;
  ASR_CHECK_ARG(a->U && a->h && a->cell && a->gates, "lstm_uni: U, h, cell and gates are required");
  if (bwd) ASR_CHECK_ARG(a->dy && a->dz && a->dy_ld >= a->H && a->dy_ld % 4 == 0,
                         "lstm_uni: BPTT needs dy (dy_ld >= H, a multiple of 4) and dz");
  else ASR_CHECK_ARG(a->zx, "lstm_uni: the forward pass needs zx");
  ASR_CHECK_ARG(!bwd || (a->h0 == nullptr && a->h_last == nullptr), "lstm_uni: BPTT takes no "
                "h0 / c0 / h_last / c_last (training starts from the zero state)");
  char* ws = static_cast<char*>(workspace);
  const int H = a->H, T = a->T;
  LstmUniParams p;
  p.T = T; p.n_pad = a->n_pad; p.H = H; p.act = a->activation; p.t = 0;
  p.U = a->U; p.mask_u = a->mask_u; p.zx = a->zx; p.h = a->h; p.cell = a->cell;
  p.gates = a->gates;
  p.h0 = a->h0; p.c0 = a->c0; p.h_last = a->h_last; p.c_last = a->c_last;
  p.dy = a->dy; p.dy_ld = a->dy_ld; p.dz = a->dz;
  p.dc = reinterpret_cast<float*>(ws + 256 + pl.ut_bytes);
  auto frame = [&](int t) {
    p.t = t;
    return rec_with_rows(pl.NR, [&](auto nr) {
      return lstm_uni_launch<decltype(nr)::value>(bwd, p, pl.NBT, stream);
    });
  };
  if (!bwd) {
    for (int t = 0; t < T; ++t)
      if ((rc = frame(t)) != ASR_OK) return rc;
    return ASR_OK;
  }
  float* Ut = reinterpret_cast<float*>(ws + 256);
  if ((rc = rec_transpose(a->U, Ut, 1, H, 4 * H, stream)) != ASR_OK) return rc;
  p.U = Ut;
  for (int t = T - 1; t >= 0; --t)
    if ((rc = frame(t)) != ASR_OK) return rc;
  if (a->db_part || a->dz_absmax)
    return rec_dbias<1>(a->dz, a->db_part, a->dz_absmax, T, a->n_pad, 1, 4 * H, stream);
  return ASR_OK;
}

}  // namespace

extern "C" size_t asr_lstm_uni_workspace_bytes(const asr_lstm_uni_args* a, int backward) {
  if (lstm_uni_check(a) != ASR_OK) return 0;
  return lstm_uni_ws_bytes(make_lstm_uni_plan(a, backward != 0));
}

extern "C" int asr_lstm_uni_seq_fwd(const asr_lstm_uni_args* a, void* workspace, size_t ws_bytes,
                                    asr_stream_t stream) {
  return lstm_uni_run(a, false, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int asr_lstm_uni_seq_bwd(const asr_lstm_uni_args* a, void* workspace, size_t ws_bytes,
                                    asr_stream_t stream) {
  return lstm_uni_run(a, true, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int asr_lstm_uni_plan(const asr_lstm_uni_args* a, int backward, int* persistent,
                                 int* rows, int* units, int* blocks) {
  const int rc = lstm_uni_check(a);
  if (rc != ASR_OK) return rc;
  const RecPlan pl = make_lstm_uni_plan(a, backward != 0);
  return rec_plan_out(pl, pl.J, persistent, rows, units, blocks);
}
