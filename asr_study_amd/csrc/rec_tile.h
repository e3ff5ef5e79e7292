// rec_tile.h -- what the stepwise recurrences of gru.hip, rhn.hip and lstm_uni.hip share (and, of
// the small pieces, rnn.hip): the reduction of one workgroup tile, the helper kernels around a
// sequence and the host side of their plans: the tile set-up (RecPlan), the answer of
// asr_*_plan, the workspace-size check and the argument checks (lstm_uni.hip, whose activation ids
// are the LSTM's 0..6, passes its own activation rule).
//
// Geometry of a tile (RecTile<NR>): a workgroup (256 threads) owns NR batch rows x J tile columns
// of one direction, NR * J = 1024, NR = 64 / 32 / 16 (the largest that divides n_pad).  The
// reduction runs in chunks of kKc = 256: the chunk's operand is staged in LDS row by row
// (coalesced 1 KB reads, rows padded by 4 floats so that the 16 lanes of a quarter-wave hit
// distinct banks), the four waves split the chunk, every lane keeps a 4 x 4 register tile and
// consumes four reduction indices per pass, and the next chunk is in flight (registers)
// meanwhile.  A cross-wave sum through LDS, in a fixed order, ends it.  Products are exact fp32
// FMAs; no float atomics: repeats are bit-identical.
#pragma once
#include "lstm_common.h"
#include "vec4.h"

namespace {

constexpr int kKc = 256;                   // reduction chunk
constexpr int kActClipped = 7;             // clipped ReLU min(max(z, 0), clip)

// Activation ids 0 tanh, 1 relu, 4 linear (asr_act_apply) and 7; the BPTT slope is taken from the
// output alone, the clipped ReLU's is 1 on 0 < h < clip and 0 elsewhere (the end points count as
// clipped).  hard_sigmoid (lstm_common.h) is the gate; its slope is read from the saved gate.
__device__ __forceinline__ float rec_act(int id, float clip, float z) {
  if (id == kActClipped) return fminf(fmaxf(z, 0.f), clip);
  return asr_act_apply(id, z);
}
__device__ __forceinline__ float rec_slope(int id, float clip, float h) {
  if (id == kActClipped) return (h > 0.f && h < clip) ? 1.f : 0.f;
  return asr_act_slope(id, h);
}
__device__ __forceinline__ float hs_slope(float g) { return (g > 0.f && g < 1.f) ? 0.2f : 0.f; }

template <int NR>
struct RecTile {
  static constexpr int J = 1024 / NR;      // tile columns
  static constexpr int KP = kKc + 4;       // padded LDS row of the operand (bank spread)
  static constexpr int NQ = NR / 4;
  static constexpr int OPV = NR * kKc / 4 / kThreads;      // float4 of a chunk per thread: operand
  static constexpr int UV = kKc * J / 4 / kThreads;        // ... and matrix
  // lds: [NR][KP] operand (row n, reduction index minor), then [kKc][J] matrix; after the last
  // chunk the head is reused as red [4][NR][J]
  static constexpr int kLdsFloats = NR * KP + kKc * J;

  // acc (rows nq + NQ i, tile columns 4 jq .. +3, reduction quarter w of every chunk) <- this
  // wave's share of op (NR rows, stride op_ld, K long) times mat (K rows, stride ldm).
  // ucol(jj): the column of mat that tile column jj (a multiple of 4) reads, or -1 for zeros.
  // MASKED: the operand is multiplied by mu (row stride mu_ld, may be null) while it is staged.
  template <bool MASKED, class UCol>
  static __device__ __forceinline__ void reduce(float* lds, const float* op, size_t op_ld, int K,
                                                const float* mat, int ldm, const float* mu,
                                                int mu_ld, UCol ucol, float (&acc)[4][4]) {
    float* opS = lds;
    float* Us = lds + NR * KP;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // neighbouring lanes read neighbouring LDS rows: the padded stride spreads them over the banks
    const int nq = lane % NQ, jq = lane / NQ;
    const int nchunks = (K + kKc - 1) / kKc;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
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
        const int col = ucol(jj);
        cu[i] = (k < K && col >= 0) ? ld4(mat + (size_t)k * ldm + col) : zero4();
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
        if (MASKED && mu != nullptr && kc + kl < K)
          v = mul4(v, ld4(mu + (size_t)n * mu_ld + kc + kl));
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

  // red [4][NR][J] <- the four waves' acc (red aliases the operand: the first barrier ends its use)
  static __device__ __forceinline__ void spill(float* red, const float (&acc)[4][4]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nq = lane % NQ, jq = lane / NQ;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
      st4(red + (w * NR + nq + NQ * i) * J + 4 * jq,
          make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]));
    __syncthreads();
  }

  // row en, tile columns col .. col + 3: the four reduction quarters added in wave order
  static __device__ __forceinline__ float4 total(const float* red, int en, int col) {
    float4 r = zero4();
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) r = add4(r, ld4(red + (ww * NR + en) * J + col));
    return r;
  }
};

// U (Z, R, Cc) -> U^T (Z, Cc, R), Z = blockIdx.z
__global__ void rec_transpose_kernel(const float* __restrict__ U, float* __restrict__ Ut, int R,
                                     int Cc) {
  __shared__ float tile[32][33];
  const float* src = U + (size_t)blockIdx.z * R * Cc;
  float* dst = Ut + (size_t)blockIdx.z * R * Cc;
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

// y_sum (rows, hq) = h[:, 0] + h[:, 1] of h (rows, 2, hq), in float4 (merge_mode='sum')
__global__ void rec_sum_kernel(const float4* __restrict__ h, float4* __restrict__ y, long long rows,
                               int hq) {
  const long long n = rows * hq;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / hq, q = i % hq;
    const float4 a = h[(r * 2) * hq + q], b = h[(r * 2 + 1) * hq + q];
    y[i] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  }
}

// db_part (n_pad / 16, ND, L, W): sums of da (L, T, n_pad, ND, W) over the 16 rows of a batch tile
// and all frames of a level, in a fixed order (16 columns x 16 interleaved slices per workgroup,
// the slices added in sequence); max |da| beside it.  blockIdx.z = d * L + l.  ND: directions in
// the slabs, 2 or (the unidirectional GRU) 1; a direction's sums do not depend on it.
template <int ND>
__global__ void __launch_bounds__(kThreads)
rec_dbias_kernel(const float* __restrict__ da, float* __restrict__ db_part, unsigned* dz_absmax,
                 int T, int n_pad, int L, int W) {
  __shared__ float part[16][17];
  const int cl = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cl;
  const int tile = blockIdx.y, d = blockIdx.z / L, l = blockIdx.z % L;
  float sum = 0.f, mx = 0.f;
  if (c < W) {
    for (int i = sl; i < T * 16; i += 16) {
      const int t = i >> 4, n = tile * 16 + (i & 15);
      const float v = da[((((size_t)l * T + t) * n_pad + n) * ND + d) * W + c];
      sum += v;
      mx = fmaxf(mx, fabsf(v));
    }
  }
  part[sl][cl] = sum;
  __syncthreads();
  if (sl == 0 && c < W && db_part != nullptr) {
    float tot = 0.f;
    for (int k = 0; k < 16; ++k) tot += part[k][cl];
    db_part[(((size_t)tile * ND + d) * L + l) * W + c] = tot;
  }
  if (dz_absmax != nullptr) {
    mx = asr_wave_max(mx);
    if ((threadIdx.x & 63) == 0) atomicMax(dz_absmax, __float_as_uint(mx));
  }
}

// ---- host side -------------------------------------------------------------------------------
inline int rec_transpose(const float* U, float* Ut, int Z, int R, int Cc, hipStream_t stream) {
  hipLaunchKernelGGL(rec_transpose_kernel, dim3((Cc + 31) / 32, (R + 31) / 32, Z), dim3(32, 8), 0,
                     stream, U, Ut, R, Cc);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

inline int rec_sum(const float* h, float* y_sum, long long rows, int H, hipStream_t stream) {
  const long long n4 = rows * (H / 4);
  const int blocks = (int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048);
  hipLaunchKernelGGL(rec_sum_kernel, dim3(blocks), dim3(256), 0, stream,
                     reinterpret_cast<const float4*>(h), reinterpret_cast<float4*>(y_sum), rows,
                     H / 4);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

// db_part and / or dz_absmax (either may be null, not both) of da (L, T, n_pad, ND, W)
template <int ND = 2>
inline int rec_dbias(const float* da, float* db_part, float* dz_absmax, int T, int n_pad, int L,
                     int W, hipStream_t stream) {
  if (dz_absmax) ASR_CHECK_HIP(hipMemsetAsync(dz_absmax, 0, sizeof(float), stream));
  hipLaunchKernelGGL(rec_dbias_kernel<ND>, dim3((W + 15) / 16, n_pad / 16, ND * L), dim3(kThreads),
                     0, stream, da, db_part, reinterpret_cast<unsigned*>(dz_absmax), T, n_pad, L, W);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

inline int rec_rows(int n_pad) { return n_pad % 64 == 0 ? 64 : (n_pad % 32 == 0 ? 32 : 16); }

// f(std::integral_constant<int, NR>) for the NR that rec_rows picked
template <class F>
auto rec_with_rows(int NR, F&& f) {
  return NR == 64 ? f(std::integral_constant<int, 64>()) : NR == 32
       ? f(std::integral_constant<int, 32>()) : f(std::integral_constant<int, 16>());
}

// The tile set-up of a stepwise recurrence (gru.hip, rhn.hip, lstm_uni.hip): it depends on n_pad,
// the column count of the widest launch and the directions nd alone.  ut_bytes (BPTT: U^T) and
// vec_bytes (BPTT: a vector the steps hand on) are the caller's to fill; they stay 0 otherwise.
struct RecPlan {
  int NR, J, NBT, blocks;
  size_t ut_bytes, vec_bytes;
};

inline RecPlan rec_plan(int n_pad, int cols, int nd) {
  const int NR = rec_rows(n_pad), J = 1024 / NR, NBT = n_pad / NR;
  return RecPlan{NR, J, NBT, (cols + J - 1) / J * NBT * nd, 0, 0};
}

// the out-parameters of asr_*_plan for a stepwise form; units: the tile columns of a workgroup
inline int rec_plan_out(const RecPlan& pl, int units_of, int* persistent, int* rows, int* units,
                        int* blocks) {
  if (persistent) *persistent = 0;
  if (rows) *rows = pl.NR;
  if (units) *units = units_of;
  if (blocks) *blocks = pl.blocks;
  return ASR_OK;
}

inline int rec_check_ws(const char* pfx, const void* workspace, size_t ws_bytes, size_t need) {
  ASR_CHECK_ARG(workspace != nullptr && ws_bytes >= need, "%s: workspace %zu bytes < %zu", pfx,
                ws_bytes, need);
  return ASR_OK;
}

inline bool rec_act_ok(int id) { return id == 0 || id == 1 || id == 4 || id == kActClipped; }

// the activation rule of asr_rnn_args / asr_gru_args / asr_gru_uni_args / asr_rhn_args
struct RecActRule {
  template <class Args>
  int operator()(const char* pfx, const Args* a) const {
    ASR_CHECK_ARG(rec_act_ok(a->activation), "%s: activation id %d (tanh 0, relu 1, linear 4, "
                  "clipped relu 7)", pfx, a->activation);
    ASR_CHECK_ARG(a->activation != kActClipped || a->clip > 0.f, "%s: clipped relu needs clip > 0",
                  pfx);
    return ASR_OK;
  }
};

// the checks every plan starts with (the args blocks share these fields): the geometry, the mode
// (persistent_form: mode 2 exists), then the activation by the rule act_ok(pfx, a)
template <class Args, class ActRule = RecActRule>
int rec_check_args(const char* pfx, const Args* a, bool persistent_form,
                   ActRule act_ok = ActRule()) {
  ASR_CHECK_ARG(a != nullptr, "%s: null arguments", pfx);
  ASR_CHECK_ARG(a->T >= 1 && a->n_pad >= 16 && a->n_pad % 16 == 0 && a->H >= 4 && a->H % 4 == 0,
                "%s: T >= 1, n_pad a multiple of 16, H a positive multiple of 4 (T=%d n_pad=%d H=%d)",
                pfx, a->T, a->n_pad, a->H);
  if (persistent_form)
    ASR_CHECK_ARG(a->mode >= 0 && a->mode <= 2, "%s: mode %d not in 0..2", pfx, a->mode);
  else
    ASR_CHECK_ARG(a->mode == 0 || a->mode == 1, "%s: mode %d: only the stepwise form exists "
                  "(0 = the plan's form, 1 = stepwise)", pfx, a->mode);
  return act_ok(pfx, a);
}

}  // namespace
