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
// Geometry, as rnn.hip: a workgroup (256 threads) owns NR batch rows x J output columns of one
// direction, NR * J = 1024, NR = 64 / 32 / 16 (the largest that divides n_pad).  The reduction
// runs in chunks of 256: the chunk's operand is staged in LDS row by row (coalesced 1 KB reads, rows
// padded by 4 floats so that the 16 lanes of a quarter-wave hit distinct banks), the four waves
// split the chunk, every lane keeps a 4 x 4 register tile and consumes four reduction indices
// per pass, the next chunk is in flight meanwhile.
// Products are exact fp32 FMAs.  The activation slopes of BPTT are read from the SAVED gates
// (hs' = 0.2 on 0 < gate < 1, else 0; act' from hh alone).  No float atomics: repeats are
// bit-identical.
#include "lstm_common.h"

namespace {

constexpr int kKc = 256;                   // reduction chunk
constexpr int kActClipped = 7;
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

__device__ __forceinline__ float gru_act(int id, float clip, float z) {
  if (id == kActClipped) return fminf(fmaxf(z, 0.f), clip);
  return asr_act_apply(id, z);
}
__device__ __forceinline__ float gru_slope(int id, float clip, float h) {
  if (id == kActClipped) return (h > 0.f && h < clip) ? 1.f : 0.f;
  return asr_act_slope(id, h);
}
__device__ __forceinline__ float hs(float a) { return fminf(fmaxf(0.2f * a + 0.5f, 0.f), 1.f); }
__device__ __forceinline__ float hs_slope(float g) { return (g > 0.f && g < 1.f) ? 0.2f : 0.f; }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) {
  return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

template <int NR, int PH>
__global__ void __launch_bounds__(kThreads)
gru_step_kernel(GruParams p) {
  constexpr int J = 1024 / NR;
  constexpr int KP = kKc + 4;              // padded LDS row of the operand (bank spread)
  constexpr int NQ = NR / 4;
  constexpr int OPV = NR * kKc / 4 / kThreads;
  constexpr int UV = kKc * J / 4 / kThreads;
  __shared__ __attribute__((aligned(16))) float lds[NR * KP + kKc * J];
  float* opS = lds;                        // [NR][KP]: row n, reduction index minor
  float* Us = lds + NR * KP;               // [kKc][J]
  float* red = lds;                        // [4][NR][J] after the last chunk (aliases opS)

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
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
  const int nchunks = (K + kKc - 1) / kKc;

  // epilogue ownership: row en, columns ej .. ej + 3 of the tile
  const int en = (4 * tid) / J, ej = (4 * tid) % J;
  const int jg = j0 + ej;
  const bool eown = jg < nout;
  // compute ownership: rows nq + NQ i (i < 4: neighbouring lanes read neighbouring LDS rows,
  // whose padded stride spreads them over the banks), columns 4 jq .. +3, reduction quarter w
  const int nq = lane % NQ, jq = lane / NQ;

  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

  if (!skip) {
    float4 cop[OPV], cu[UV];
    auto load = [&](int c) {
      const int kc = c * kKc;
#pragma unroll
      for (int i = 0; i < OPV; ++i) {
        // a wave reads one row's whole chunk (1 KB, contiguous)
        const int idx = tid + i * kThreads;
        const int n = idx / (kKc / 4), k = kc + 4 * (idx % (kKc / 4));
        cop[i] = k < K ? ld4(op + (size_t)n * op_ld + k) : zero4();
      }
#pragma unroll
      for (int i = 0; i < UV; ++i) {
        const int idx = tid + i * kThreads;
        const int jj = 4 * (idx % (J / 4)), k = kc + idx / (J / 4);
        cu[i] = (k < K && j0 + jj < nout) ? ld4(mat + (size_t)k * ldm + j0 + jj) : zero4();
      }
    };
    load(0);
    for (int c = 0; c < nchunks; ++c) {
      __syncthreads();                                 // previous chunk fully consumed
      const int kc = c * kKc;
#pragma unroll
      for (int i = 0; i < OPV; ++i) {
        const int idx = tid + i * kThreads;
        const int n = idx / (kKc / 4), kl = 4 * (idx % (kKc / 4));
        float4 v = cop[i];
        if (PH == kFwdA && mu != nullptr && kc + kl < K)      // m = h_prev (.) B_U
          v = mul4(v, ld4(mu + (size_t)n * Hp + kc + kl));
        st4(opS + n * KP + kl, v);
      }
#pragma unroll
      for (int i = 0; i < UV; ++i) {
        const int idx = tid + i * kThreads;
        const int jj = 4 * (idx % (J / 4)), kl = idx / (J / 4);
        st4(Us + kl * J + jj, cu[i]);
      }
      __syncthreads();
      if (c + 1 < nchunks) load(c + 1);                // in flight while this chunk reduces
      const int kw = w * (kKc / 4);
#pragma unroll 2
      for (int kk = 0; kk < kKc / 4; kk += 4) {
        float av[4][4], bv[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float4 a = ld4(opS + (nq + NQ * i) * KP + kw + kk);
          av[i][0] = a.x; av[i][1] = a.y; av[i][2] = a.z; av[i][3] = a.w;
          const float4 b = ld4(Us + (kw + kk + i) * J + 4 * jq);
          bv[i][0] = b.x; bv[i][1] = b.y; bv[i][2] = b.z; bv[i][3] = b.w;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i][q], bv[q][j], acc[i][j]);
      }
    }
  }
  float4 r = zero4();
  if (!skip) {
    // cross-wave sum of the four reduction quarters (fixed order)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
      st4(red + (w * NR + nq + NQ * i) * J + 4 * jq,
          make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]));
    __syncthreads();
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float4 v = ld4(red + (ww * NR + en) * J + ej);
      r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
    }
  }
  if (!eown) return;

  const size_t row = row0 + en, rowp = rowp0 + en;
  if (PH == kFwdA) {
    // columns [0, Hp): z; [Hp, 2Hp): r (a float4 never straddles the two: Hp % 4 == 0)
    const size_t o = (row * 2 + d) * 3 * Hp + jg;
    const float4 zx = ld4(p.zx + o);
    const float4 g = make_float4(hs(zx.x + r.x), hs(zx.y + r.y), hs(zx.z + r.z), hs(zx.w + r.w));
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
    const float4 hh = make_float4(gru_act(p.act, p.clip, zx.x + r.x), gru_act(p.act, p.clip, zx.y + r.y),
                                  gru_act(p.act, p.clip, zx.z + r.z), gru_act(p.act, p.clip, zx.w + r.w));
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
        make_float4(g.x * (1.f - z.x) * gru_slope(p.act, p.clip, hh.x),
                    g.y * (1.f - z.y) * gru_slope(p.act, p.clip, hh.y),
                    g.z * (1.f - z.z) * gru_slope(p.act, p.clip, hh.z),
                    g.w * (1.f - z.w) * gru_slope(p.act, p.clip, hh.w)));
    st4(p.da + og + jg,
        make_float4(g.x * (hp.x - hh.x) * hs_slope(z.x), g.y * (hp.y - hh.y) * hs_slope(z.y),
                    g.z * (hp.z - hh.z) * hs_slope(z.z), g.w * (hp.w - hh.w) * hs_slope(z.w)));
    st4(p.gbuf + ow, g);
  }
}

// U (2, Hp, 3Hp) -> U^T (2, 3Hp, Hp)
__global__ void gru_transpose_kernel(const float* __restrict__ U, float* __restrict__ Ut, int Hp) {
  __shared__ float tile[32][33];
  const int d = blockIdx.z, R = Hp, Cc = 3 * Hp;
  const float* src = U + (size_t)d * R * Cc;
  float* dst = Ut + (size_t)d * R * Cc;
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int r = by + i, c = bx + threadIdx.x;
    if (r < R && c < Cc) tile[i][threadIdx.x] = src[(size_t)r * Cc + c];
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += 8) {
    const int r = bx + i, c = by + threadIdx.x;
    if (r < Cc && c < R) dst[(size_t)r * R + c] = tile[threadIdx.x][i];
  }
}

// y_sum (T, n_pad, Hp) = h[:, :, 0] + h[:, :, 1] (merge_mode='sum')
__global__ void gru_sum_kernel(const float4* __restrict__ h, float4* __restrict__ y, long long rows,
                               int hq) {
  const long long n = rows * hq;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / hq, q = i % hq;
    const float4 a = h[(r * 2) * hq + q], b = h[(r * 2 + 1) * hq + q];
    y[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
}

// db_part (n_pad / 16, 2, 3Hp): sums of da over the 16 rows of a batch tile and all frames, in a
// fixed order (16 columns x 16 interleaved slices per workgroup, the slices added in sequence);
// max |da| beside it.
__global__ void __launch_bounds__(kThreads)
gru_dbias_kernel(const float* __restrict__ da, float* __restrict__ db_part, unsigned* dz_absmax,
                 int T, int n_pad, int Hp) {
  __shared__ float part[16][17];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const int tile = blockIdx.y, d = blockIdx.z, W = 3 * Hp;
  float sum = 0.f, mx = 0.f;
  if (c < W) {
    for (int i = sl; i < T * 16; i += 16) {
      const int t = i >> 4, n = tile * 16 + (i & 15);
      const float v = da[(((size_t)t * n_pad + n) * 2 + d) * W + c];
      sum += v;
      mx = fmaxf(mx, fabsf(v));
    }
  }
  part[sl][cl] = sum;
  __syncthreads();
  if (sl == 0 && c < W && db_part != nullptr) {
    float tot = 0.f;
    for (int k = 0; k < 16; ++k) tot += part[k][cl];
    db_part[((size_t)tile * 2 + d) * W + c] = tot;
  }
  if (dz_absmax != nullptr) {
    mx = asr_wave_max(mx);
    if ((threadIdx.x & 63) == 0) atomicMax(dz_absmax, __float_as_uint(mx));
  }
}

// ---- host side -------------------------------------------------------------------------------
struct GruPlan {
  int NR, J, NBT, blocks;
  size_t ut_bytes, vec_bytes;
};

bool act_ok(int id) { return id == 0 || id == 1 || id == 4 || id == kActClipped; }

int make_gru_plan(const asr_gru_args* a, bool bwd, GruPlan* pl) {
  ASR_CHECK_ARG(a != nullptr, "gru: null arguments");
  ASR_CHECK_ARG(a->T >= 1 && a->n_pad >= 16 && a->n_pad % 16 == 0 && a->H >= 4 && a->H % 4 == 0,
                "gru: T >= 1, n_pad a multiple of 16, H a positive multiple of 4 (T=%d n_pad=%d H=%d)",
                a->T, a->n_pad, a->H);
  ASR_CHECK_ARG(a->mode == 0 || a->mode == 1, "gru: mode %d: only the stepwise form exists "
                "(0 = the plan's form, 1 = stepwise)", a->mode);
  ASR_CHECK_ARG(act_ok(a->activation), "gru: activation id %d (tanh 0, relu 1, linear 4, "
                "clipped relu 7)", a->activation);
  ASR_CHECK_ARG(a->activation != kActClipped || a->clip > 0.f, "gru: clipped relu needs clip > 0");
  pl->NR = a->n_pad % 64 == 0 ? 64 : (a->n_pad % 32 == 0 ? 32 : 16);
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
  constexpr int J = 1024 / NR;
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
  return pl.NR == 64 ? gru_launch<64>(ph, p, ncols, pl.NBT, stream)
       : pl.NR == 32 ? gru_launch<32>(ph, p, ncols, pl.NBT, stream)
                     : gru_launch<16>(ph, p, ncols, pl.NBT, stream);
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
    if (a->y_sum) {
      const long long rows = (long long)T * a->n_pad;
      const long long n4 = rows * (H / 4);
      const int blocks = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
      hipLaunchKernelGGL(gru_sum_kernel, dim3(blocks), dim3(256), 0, stream,
                         reinterpret_cast<const float4*>(a->h), reinterpret_cast<float4*>(a->y_sum),
                         rows, H / 4);
      ASR_CHECK_LAUNCH();
    }
    return ASR_OK;
  }
  float* Ut = reinterpret_cast<float*>(ws + 256);
  hipLaunchKernelGGL(gru_transpose_kernel, dim3((3 * H + 31) / 32, (H + 31) / 32, 2), dim3(32, 8),
                     0, stream, a->U, Ut, H);
  ASR_CHECK_LAUNCH();
  p.U = Ut;
  // phase B of step s also prepares da_h, da_z of step s - 1: s = T is the prologue (carry 0)
  p.s = T;
  if ((rc = gru_phase(pl, kBwdB, p, H, stream)) != ASR_OK) return rc;
  for (int s = T - 1; s >= 0; --s) {
    p.s = s;
    if ((rc = gru_phase(pl, kBwdA, p, H, stream)) != ASR_OK) return rc;
    if (s > 0 && (rc = gru_phase(pl, kBwdB, p, H, stream)) != ASR_OK) return rc;
  }
  if (a->db_part || a->dz_absmax) {
    if (a->dz_absmax) ASR_CHECK_HIP(hipMemsetAsync(a->dz_absmax, 0, sizeof(float), stream));
    hipLaunchKernelGGL(gru_dbias_kernel, dim3((3 * H + 15) / 16, a->n_pad / 16, 2), dim3(kThreads),
                       0, stream, a->da, a->db_part, reinterpret_cast<unsigned*>(a->dz_absmax), T,
                       a->n_pad, H);
    ASR_CHECK_LAUNCH();
  }
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
