// rnn.hip -- the Keras-1.2.2 SimpleRNN recurrence of a Bidirectional layer (K14, include/asr_hip.h):
// forward h_t = act(zx_t + (h_{t-1} (.) B_U) @ U) and BPTT dz_t = (dy_t + (dz_{t+1} @ U^T) (.) B_U)
// (.) act'(h_t), both directions in one launch.  zx = x @ W + b comes from the GEMMs, and so do
// dW, dU, dx; this file owns the sequential part only.
//
// Geometry.  A workgroup (256 threads) owns NR batch rows x J units of one direction, NR * J =
// 1024 outputs: NR = 64 / 32 / 16 (the largest that divides n_pad), J = 1024 / NR.  Per step it
// reduces the operand (h_{t-1}, or dz of the previous BPTT step: NR x Hp) against its J columns of
// U (or U^T) in chunks of 256 along the reduction: the chunk's operand is staged transposed in
// LDS, the four waves split the chunk, every lane keeps a 4 x 4 register tile, and the chunk after
// it is already in flight (registers) while the current one is reduced.  A cross-wave sum in LDS
// ends the step.  Products are exact fp32 FMAs (no split operands, no scales, no range limit:
// |h| is unbounded with relu / linear and dz with every activation).
//
// Two launch forms (asr_rnn_args.mode, asr_rnn_plan):
//  * stepwise: one launch per step, both directions; the operand is read from the h / dz slab.
//  * persistent: one launch for the whole sequence; the P = ceil(Hp / J) workgroups of a chain
//    (direction x batch tile) hand the operand over through a two-slot exchange buffer of tagged
//    words (lstm_common.h: tag_word / tags_ok, 16-byte SC1 buffer loads and stores), every poll
//    bounded by the wall clock.  A workgroup that gives up marks the sticky timeout word at the
//    head of the workspace (same contract as asr_lstm_status) and runs on without waiting.
//    It needs every workgroup resident at once: the plan picks it only if the launch has at most
//    one workgroup per CU.
//
// Activation ids (asr_rnn_args.activation): 0 tanh, 1 relu, 4 linear (asr_act_apply), 7 clipped
// ReLU min(max(z, 0), clip).  The BPTT derivative is taken from h alone; the clipped ReLU's is 1 on
// 0 < h < clip and 0 elsewhere (csrc/conv.hip's convention: the two end points count as clipped).
//
// rec_tile.h gives the activation pair, the U transpose, the direction sum and the argument checks.
// The reduction is not RecTile's: it stages the operand transposed and polls a tagged exchange.
#include "rec_tile.h"

namespace {

struct RnnParams {
  int T, n_pad, Hp, NBT, P;
  int act;
  float clip;
  int s_begin, s_count;
  long long spin;
  const float* U;          // fwd: U (2, Hp, Hp) [k][j]; BPTT: U^T (2, Hp, Hp) [k][j] = U[j][k]
  const float* mask_u;     // (2, n_pad, Hp) or null
  const float* zx;         // fwd (T, n_pad, 2, Hp)
  float* h;                // (T, n_pad, 2, Hp): fwd writes, BPTT reads
  const float* dy;         // BPTT
  long long dy_ld;
  int dy_dstride;
  float* dz;               // BPTT (T, n_pad, 2, Hp)
  float* db_part;          // BPTT optional (n_pad / 16, 2, Hp)
  unsigned* dz_absmax;     // BPTT optional (float bits)
  unsigned* xbuf;          // persistent: [2 * NBT chains][2 slots][NR][Hp] tagged words
  int* status;
};

// One operand chunk (NR rows x kKc reduction columns) and one U chunk (kKc x J), as float4
// registers of this thread: OPV + UV of them.
template <int NR>
struct Chunk {
  static constexpr int J = 1024 / NR;
  static constexpr int OPV = NR * kKc / 4 / kThreads;
  static constexpr int UV = kKc * J / 4 / kThreads;
  float4 op[OPV];
  float4 u[UV];
};

template <int NR, bool BWD, bool PERSIST>
__global__ void __launch_bounds__(kThreads)
rnn_seq_kernel(RnnParams p) {
  constexpr int J = 1024 / NR;
  constexpr int NRP = NR + 4;              // padded LDS row of the transposed operand
  constexpr int NQ = NR / 4;
  constexpr int OPV = Chunk<NR>::OPV, UV = Chunk<NR>::UV;
  __shared__ __attribute__((aligned(16))) float lds[kKc * NRP + kKc * J];
  float* opT = lds;                        // [kKc][NRP]
  float* Us = lds + kKc * NRP;             // [kKc][J]
  float* red = lds;                        // [4][NR][J] after the last chunk (aliases opT)

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int jb = blockIdx.x, nt = blockIdx.y, d = blockIdx.z;
  const int Hp = p.Hp, n_pad = p.n_pad, T = p.T;
  const int j0 = jb * J, n0 = nt * NR;
  const int nchunks = (Hp + kKc - 1) / kKc;
  const float* Ud = p.U + (size_t)d * Hp * Hp;
  const float* mu = p.mask_u ? p.mask_u + (size_t)d * n_pad * Hp : nullptr;
  const int chain = d * p.NBT + nt;
  const unsigned slot_words = (unsigned)NR * Hp;
  unsigned* xch = PERSIST ? p.xbuf + (size_t)chain * 2 * slot_words : nullptr;
  bool dead = false;

  // epilogue ownership: row en, units ej .. ej + 3 of the tile
  const int en = (4 * tid) / J, ej = (4 * tid) % J;
  const int jg = j0 + ej;
  const bool eown = jg < Hp;
  float4 dbs = make_float4(0.f, 0.f, 0.f, 0.f);
  float zmax = 0.f;
  // compute ownership: rows 4 nq .. +3, units 4 jq .. +3, reduction quarter w of a chunk
  const int nq = lane % NQ, jq = lane / NQ;

  for (int s = p.s_begin; s < p.s_begin + p.s_count; ++s) {
    // processing order: forward pass d = 0 runs t = 0 .. T-1, d = 1 backwards; BPTT reverses both
    const int t = (d == 0) == !BWD ? s : T - 1 - s;
    const int tp = (d == 0) == !BWD ? t - 1 : t + 1;      // time of the operand (step s - 1)
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

    if (s > 0) {
      const float* src = BWD ? p.dz : p.h;                 // stepwise: the slab
      const unsigned tag = (unsigned)((s - 1) >> 1) & 1u;
      __amdgpu_buffer_rsrc_t rsrc;
      if (PERSIST)
        rsrc = __builtin_amdgcn_make_buffer_rsrc(xch + (size_t)((s - 1) & 1) * slot_words, 0,
                                                 slot_words * 4, 0x00020000);
      Chunk<NR> cur;
      auto load = [&](int c, Chunk<NR>& ch) {
        const int kc = c * kKc;
#pragma unroll
        for (int i = 0; i < OPV; ++i) {
          // consecutive threads: consecutive rows (conflict-free transposed LDS writes)
          const int idx = tid + i * kThreads;
          const int n = idx % NR, k = kc + 4 * (idx / NR);
          if (k < Hp) {
            if (PERSIST) {
              const u32x4 v = xload<false>(rsrc, (unsigned)(n * Hp + k) * 4u);
              ch.op[i] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]),
                                     __uint_as_float(v[2]), __uint_as_float(v[3]));
            } else {
              ch.op[i] = *reinterpret_cast<const float4*>(
                  src + ((size_t)(tp * n_pad + n0 + n) * 2 + d) * Hp + k);
            }
          } else {
            ch.op[i] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
#pragma unroll
        for (int i = 0; i < UV; ++i) {
          const int idx = tid + i * kThreads;
          const int jj = 4 * (idx % (J / 4)), k = kc + idx / (J / 4);
          ch.u[i] = (k < Hp && j0 + jj < Hp)
                        ? *reinterpret_cast<const float4*>(Ud + (size_t)k * Hp + j0 + jj)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      };
      // persistent: re-poll the operand words that do not carry this step's tag yet
      auto settle = [&](int c, Chunk<NR>& ch) {
        if (!PERSIST) return;
        const int kc = c * kKc;
        long long t0 = 0;
        bool timing = false;
        for (;;) {
          bool ok = true;
#pragma unroll
          for (int i = 0; i < OPV; ++i) {
            const int idx = tid + i * kThreads;
            const int n = idx % NR, k = kc + 4 * (idx / NR);
            if (k >= Hp) continue;
            u32x4 v = {__float_as_uint(ch.op[i].x), __float_as_uint(ch.op[i].y),
                       __float_as_uint(ch.op[i].z), __float_as_uint(ch.op[i].w)};
            if (!tags_ok(v, tag)) {
              ok = false;
              v = xload<false>(rsrc, (unsigned)(n * Hp + k) * 4u);
              ch.op[i] = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]),
                                     __uint_as_float(v[2]), __uint_as_float(v[3]));
            }
          }
          if (ok || dead) return;
          if (!timing) { t0 = wall_clock64(); timing = true; }
          else if (wall_clock64() - t0 > p.spin) {
            dead = true;
            mark_timeout(p.status);
            return;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      };
      load(0, cur);
      for (int c = 0; c < nchunks; ++c) {
        settle(c, cur);
        __syncthreads();                                 // previous chunk fully consumed
        const int kc = c * kKc;
#pragma unroll
        for (int i = 0; i < OPV; ++i) {
          const int idx = tid + i * kThreads;
          const int n = idx % NR, kl = 4 * (idx / NR);
          float4 v = cur.op[i];
          if (!BWD && mu != nullptr && kc + kl < Hp) {   // forward: h_{t-1} (.) B_U
            const float4 m = *reinterpret_cast<const float4*>(mu + (size_t)(n0 + n) * Hp + kc + kl);
            v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
          }
          opT[(kl + 0) * NRP + n] = v.x;
          opT[(kl + 1) * NRP + n] = v.y;
          opT[(kl + 2) * NRP + n] = v.z;
          opT[(kl + 3) * NRP + n] = v.w;
        }
#pragma unroll
        for (int i = 0; i < UV; ++i) {
          const int idx = tid + i * kThreads;
          const int jj = 4 * (idx % (J / 4)), kl = idx / (J / 4);
          *reinterpret_cast<float4*>(Us + kl * J + jj) = cur.u[i];
        }
        __syncthreads();
        if (c + 1 < nchunks) load(c + 1, cur);           // in flight while this chunk reduces
        const int kw = w * (kKc / 4);
#pragma unroll 8
        for (int kk = 0; kk < kKc / 4; ++kk) {
          const float4 a = *reinterpret_cast<const float4*>(opT + (kw + kk) * NRP + 4 * nq);
          const float4 b = *reinterpret_cast<const float4*>(Us + (kw + kk) * J + 4 * jq);
          const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
      }
    }
    // cross-wave sum of the four reduction quarters
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
      *reinterpret_cast<float4*>(red + (w * NR + 4 * nq + i) * J + 4 * jq) =
          make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
    __syncthreads();
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float4 v = *reinterpret_cast<const float4*>(red + (ww * NR + en) * J + ej);
      r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
    }
    if (eown) {
      const size_t row = (size_t)(t * n_pad + n0 + en);
      const size_t o = (row * 2 + d) * Hp + jg;
      float4 out;
      if (!BWD) {
        const float4 z = *reinterpret_cast<const float4*>(p.zx + o);
        out = make_float4(rec_act(p.act, p.clip, z.x + r.x), rec_act(p.act, p.clip, z.y + r.y),
                          rec_act(p.act, p.clip, z.z + r.z), rec_act(p.act, p.clip, z.w + r.w));
        *reinterpret_cast<float4*>(p.h + o) = out;
      } else {
        if (mu != nullptr) {                             // d h_{t-1} = (dz @ U^T) (.) B_U
          const float4 m = *reinterpret_cast<const float4*>(mu + (size_t)(n0 + en) * Hp + jg);
          r.x *= m.x; r.y *= m.y; r.z *= m.z; r.w *= m.w;
        }
        const float4 g = *reinterpret_cast<const float4*>(p.dy + row * p.dy_ld +
                                                          (size_t)d * p.dy_dstride + jg);
        const float4 hv = *reinterpret_cast<const float4*>(p.h + o);
        out = make_float4((g.x + r.x) * rec_slope(p.act, p.clip, hv.x),
                          (g.y + r.y) * rec_slope(p.act, p.clip, hv.y),
                          (g.z + r.z) * rec_slope(p.act, p.clip, hv.z),
                          (g.w + r.w) * rec_slope(p.act, p.clip, hv.w));
        *reinterpret_cast<float4*>(p.dz + o) = out;
        dbs.x += out.x; dbs.y += out.y; dbs.z += out.z; dbs.w += out.w;
        zmax = fmaxf(zmax, fmaxf(fmaxf(fabsf(out.x), fabsf(out.y)), fmaxf(fabsf(out.z), fabsf(out.w))));
      }
      if (PERSIST && s + 1 < p.s_begin + p.s_count) {
        const unsigned tag = (unsigned)(s >> 1) & 1u;
        const u32x4 v = {tag_word(out.x, tag), tag_word(out.y, tag), tag_word(out.z, tag),
                         tag_word(out.w, tag)};
        const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(
            xch + (size_t)(s & 1) * slot_words, 0, slot_words * 4, 0x00020000);
        xstore<false>(v, wr, (unsigned)(en * Hp + jg) * 4u);
      }
    }
  }
  if (BWD) {
    if (p.dz_absmax != nullptr) {
      const float m = asr_wave_max(zmax);
      if (lane == 0) atomicMax(p.dz_absmax, __float_as_uint(m));
    }
    if (p.db_part != nullptr) {
      // per 16-row batch tile: the sums of dz over its rows (and this launch's steps)
      __syncthreads();
      *reinterpret_cast<float4*>(red + en * J + ej) = dbs;
      __syncthreads();
      if (tid < (NR / 16) * J) {
        const int tile = tid / J, j = tid % J;
        if (j0 + j < Hp) {
          float sum = 0.f;
          for (int n = 0; n < 16; ++n) sum += red[(tile * 16 + n) * J + j];
          float* dst = p.db_part + ((size_t)(n0 / 16 + tile) * 2 + d) * Hp + j0 + j;
          *dst += sum;
        }
      }
    }
  }
}

__global__ void act_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n,
                               int act, float clip) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    y[i] = rec_act(act, clip, x[i]);
}

__global__ void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                               float* __restrict__ dx, long long n, int act, float clip) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    dx[i] = dy[i] * rec_slope(act, clip, y[i]);
}

// ---- host side -------------------------------------------------------------------------------
constexpr size_t kHeadBytes = 2 * kStickyInts * sizeof(int);     // sticky block + status block

struct RnnPlan {
  int NR, J, P, NBT, blocks;
  bool persistent;
  size_t ut_bytes, x_bytes;
};

int rnn_num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
      return 0;
    cus = prop.multiProcessorCount;
  }
  return cus;
}

int make_rnn_plan(const asr_rnn_args* a, bool bwd, RnnPlan* pl) {
  const int rc = rec_check_args("rnn", a, true);
  if (rc != ASR_OK) return rc;
  pl->NR = rec_rows(a->n_pad);
  pl->J = 1024 / pl->NR;
  pl->P = (a->H + pl->J - 1) / pl->J;
  pl->NBT = a->n_pad / pl->NR;
  pl->blocks = pl->P * pl->NBT * 2;
  const int cus = rnn_num_cus();
  // every workgroup of a persistent launch must be resident at once: one per CU at most.
  // The default (mode 0) follows the measurements of DESIGN.md 13: ASR_RNN_PERSISTENT=1 lets
  // mode 0 pick the persistent form wherever it is resident.
  const bool resident = cus > 0 && pl->blocks <= cus && a->T > 1;
  const char* env = getenv("ASR_RNN_PERSISTENT");
  const bool pick = env != nullptr && env[0] == '1';
  if (a->mode == 2)
    ASR_CHECK_ARG(resident, "rnn: the persistent form needs %d resident workgroups (%d CUs)",
                  pl->blocks, cus);
  pl->persistent = a->mode == 2 || (a->mode == 0 && resident && pick);
  pl->ut_bytes = bwd ? asr_align_up((size_t)2 * a->H * a->H * sizeof(float), 256) : 0;
  pl->x_bytes = pl->persistent ? (size_t)2 * pl->NBT * 2 * pl->NR * a->H * sizeof(unsigned) : 0;
  return ASR_OK;
}

template <int NR>
void* pick_kernel(bool bwd, bool persistent) {
  if (bwd) return persistent ? (void*)rnn_seq_kernel<NR, true, true> : (void*)rnn_seq_kernel<NR, true, false>;
  return persistent ? (void*)rnn_seq_kernel<NR, false, true> : (void*)rnn_seq_kernel<NR, false, false>;
}

int rnn_run(const asr_rnn_args* a, bool bwd, void* workspace, size_t ws_bytes, hipStream_t stream) {
  RnnPlan pl;
  int rc = make_rnn_plan(a, bwd, &pl);
  if (rc != ASR_OK) return rc;
  rc = rec_check_ws("rnn", workspace, ws_bytes, kHeadBytes + pl.ut_bytes + pl.x_bytes);
  if (rc != ASR_OK) return rc;
  ASR_CHECK_ARG(a->U && a->h, "rnn: U and h are required");
  if (bwd) ASR_CHECK_ARG(a->dy && a->dz && a->dy_ld >= a->H, "rnn: BPTT needs dy (dy_ld >= H) and dz");
  else ASR_CHECK_ARG(a->zx != nullptr, "rnn: the forward pass needs zx");
  char* ws = static_cast<char*>(workspace);
  RnnParams p;
  p.T = a->T; p.n_pad = a->n_pad; p.Hp = a->H; p.NBT = pl.NBT; p.P = pl.P;
  p.act = a->activation; p.clip = a->clip;
  p.mask_u = a->mask_u; p.zx = a->zx; p.h = a->h;
  p.dy = a->dy; p.dy_ld = a->dy_ld; p.dy_dstride = a->dy_dir_stride;
  p.dz = a->dz; p.db_part = a->db_part;
  p.dz_absmax = reinterpret_cast<unsigned*>(a->dz_absmax);
  p.status = reinterpret_cast<int*>(ws + kStickyInts * sizeof(int));
  p.xbuf = reinterpret_cast<unsigned*>(ws + kHeadBytes + pl.ut_bytes);
  const char* spin = getenv("ASR_RNN_SPIN_MS");
  p.spin = (long long)(spin ? atoi(spin) : 600) * 100000LL;
  // status block of this call to 0 (the sticky word in front of it stays), exchange slots to
  // all-ones (tag 1: no step has tag 1 in its slot before it is written)
  ASR_CHECK_HIP(hipMemsetAsync(p.status, 0, kStickyInts * sizeof(int), stream));
  if (pl.persistent) ASR_CHECK_HIP(hipMemsetAsync(p.xbuf, 0xFF, pl.x_bytes, stream));
  if (bwd) {
    float* Ut = reinterpret_cast<float*>(ws + kHeadBytes);
    if ((rc = rec_transpose(a->U, Ut, 2, a->H, a->H, stream)) != ASR_OK) return rc;
    p.U = Ut;
    if (a->db_part)
      ASR_CHECK_HIP(hipMemsetAsync(a->db_part, 0, (size_t)(a->n_pad / 16) * 2 * a->H * sizeof(float), stream));
    if (a->dz_absmax) ASR_CHECK_HIP(hipMemsetAsync(a->dz_absmax, 0, sizeof(float), stream));
  } else {
    p.U = a->U;
  }
  void* k = rec_with_rows(pl.NR, [&](auto nr) {
    return pick_kernel<decltype(nr)::value>(bwd, pl.persistent);
  });
  const dim3 grid(pl.P, pl.NBT, 2);
  const int per_launch = pl.persistent ? a->T : 1;
  for (int s0 = 0; s0 < a->T; s0 += per_launch) {
    p.s_begin = s0;
    p.s_count = per_launch;
    void* args[] = {&p};
    ASR_CHECK_HIP(hipLaunchKernel(k, grid, dim3(kThreads), args, 0, stream));
  }
  if (!bwd && a->y_sum)
    return rec_sum(a->h, a->y_sum, (long long)a->T * a->n_pad, a->H, stream);
  return ASR_OK;
}

}  // namespace

extern "C" size_t asr_rnn_workspace_bytes(const asr_rnn_args* a, int backward) {
  RnnPlan pl;
  if (make_rnn_plan(a, backward != 0, &pl) != ASR_OK) return 0;
  return kHeadBytes + pl.ut_bytes + pl.x_bytes;
}

extern "C" int asr_rnn_seq_fwd(const asr_rnn_args* a, void* workspace, size_t ws_bytes,
                               asr_stream_t stream) {
  return rnn_run(a, false, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int asr_rnn_seq_bwd(const asr_rnn_args* a, void* workspace, size_t ws_bytes,
                               asr_stream_t stream) {
  return rnn_run(a, true, workspace, ws_bytes, (hipStream_t)stream);
}

extern "C" int asr_rnn_plan(const asr_rnn_args* a, int backward, int* persistent, int* rows,
                            int* units, int* blocks) {
  RnnPlan pl;
  const int rc = make_rnn_plan(a, backward != 0, &pl);
  if (rc != ASR_OK) return rc;
  if (persistent) *persistent = pl.persistent ? 1 : 0;
  if (rows) *rows = pl.NR;
  if (units) *units = pl.J;
  if (blocks) *blocks = pl.blocks;
  return ASR_OK;
}

extern "C" int asr_activation_fwd(const float* x, float* y, int64_t n, int activation, float clip,
                                  asr_stream_t stream) {
  ASR_CHECK_ARG(x && y && n >= 0 && rec_act_ok(activation), "activation_fwd: bad arguments");
  if (n == 0) return ASR_OK;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(act_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, y,
                     (long long)n, activation, clip);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_activation_bwd(const float* dy, const float* y, float* dx, int64_t n,
                                  int activation, float clip, asr_stream_t stream) {
  ASR_CHECK_ARG(dy && y && dx && n >= 0 && rec_act_ok(activation), "activation_bwd: bad arguments");
  if (n == 0) return ASR_OK;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(act_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dy, y, dx,
                     (long long)n, activation, clip);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
