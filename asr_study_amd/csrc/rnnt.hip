// K31 RNN-Transducer (Graves, arXiv 1211.3711): fused joint + lattice loss + gradients, one step
// of frame-synchronous greedy decoding, and two row helpers -- gfx950.
//
//   z(n,t,u,:) = tanh(enc(t,n,:) + pred(u,n,:)) W_out + b_out,  lp = log_softmax(z),
//   alpha(t,u) = lse(alpha(t-1,u) + lp_blank(t-1,u), alpha(t,u-1) + lp_y(t,u-1)),
//   loss_n = -(alpha(T_n-1,U_n) + lp_blank(T_n-1,U_n));  tests/rnnt_oracle.py restates it.
//
// Neither the hidden tensor (t,u,j) nor the logits (t,u,c) nor their gradients are ever written:
// a lattice cell is recomputed where it is needed.  The workspace holds four floats per cell
// (lp_blank, lp_y, alpha~, beta~), two float64 offsets per anti-diagonal, and kSlabs partial
// (J + 1, CP) slabs of dW_out / db_out.
//
//   phase 1  rnnt_lp_kernel     one thread per cell, 16 x 16 cells per workgroup, W_out staged
//            through LDS 64 rows at a time, C accumulators in registers; leaves lp_blank, lp_y
//   phase 2  rnnt_chain_kernel  one workgroup per (utterance, direction), lane u holds cell
//            (d - u, u) of anti-diagonal d = t + u; the neighbour lane comes by one DPP wave
//            shift, across waves through one LDS word per wave.  Every 4 diagonals the row is
//            re-centred on its maximum; what was removed is summed in float64 (A_d, B_d).
//   phase 3  rnnt_bwd_kernel<AX> recomputes the cell, forms dz in registers from
//            alpha~ + beta~ + (float)(A_d + B_d' - logZ), then dh = dz W_out^T and dpre = dh (1-h^2).
//            AX = 0: a workgroup OWNS 16 frames of one utterance and walks the label positions:
//            d_enc(t) = sum_u in a fixed order (16-lane DPP row sum, then tile after tile).  The same
//            pass sums h (x) dz and dz into the workgroup's own slab (the grid is kSlabs
//            workgroups that take (utterance, frame tile) items in a fixed stride); a last kernel
//            adds the slabs in index order.  AX = 1: a workgroup owns 16 label positions and
//            walks the frames: d_pred(u) = sum_t.  No float atomics anywhere: every result is the
//            same bits on every run.
//
// Layout of the per-cell arrays: SKEWED, index (n, d, u) with d = t + u, so the chains read and
// write one contiguous row per step.
// (the pieces this joint shares with the attention decoder's, aed.hip: joint_common.h)
#include "joint_common.h"

namespace {

constexpr int TS = 16;        // cells per tile side
constexpr int KJ = 64;        // rows of W_out (and columns of the enc / pred tiles) staged at once
constexpr int SJ = 16;        // of those, rows per pass of the dW_out accumulation
constexpr int kSlabs = 256;   // workgroups of the d_enc pass = partial dW_out slabs
constexpr int kRecentre = 4;  // diagonals between two re-centrings
constexpr int kMaxT = 1000000; // frames: ceil(T / 16) frame tiles are one grid dimension (<= 65535)

__device__ __forceinline__ float wave_shift_up(float v, float fill) {      // lane i <- lane i-1
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v),
                                                    0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_shift_down(float v, float fill) {    // lane i <- lane i+1
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v),
                                                    0x130, 0xf, 0xf, false));
}

// Sum over a DPP row (16 neighbouring lanes, one owned row or column of a cell tile): four
// row_shr adds on the vector ALU, lanes shifted in from outside the row read 0; the LAST lane
// of the row holds ((v15 + v14) + (v13 + v12)) + ... in that fixed order.
template <int SHR>
__device__ __forceinline__ float row_shr(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + SHR, 0xf, 0xf,
                                                    true));
}
__device__ __forceinline__ float row16_sum(float v) {
  v += row_shr<1>(v);
  v += row_shr<2>(v);
  v += row_shr<4>(v);
  v += row_shr<8>(v);
  return v;
}

__host__ __device__ inline int pad4(int x) { return (x + 3) / 4 * 4; }

__device__ __forceinline__ void clamp_lens(const int* seq_len, const int* label_len, int n, int T,
                                           int U1, int& Tn, int& Un) {
  Tn = seq_len[n];
  Tn = Tn < 1 ? 1 : (Tn > T ? T : Tn);
  Un = label_len[n];
  Un = Un < 0 ? 0 : (Un > U1 - 1 ? U1 - 1 : Un);
}

// ---- LDS staging of one KJ-row pass: W_out rows j0.., and those columns of 16 enc rows (frames
// t0..) and 16 pred rows (positions u0..) of utterance n.  Whatever lies outside is 0.
template <int CP>
__device__ __forceinline__ void stage(float* Ws, float* fs, float* gs,
                                      const float* __restrict__ enc,
                                      const float* __restrict__ pred,
                                      const float* __restrict__ W, int n, int n_pad, int J, int C,
                                      int T, int U1, int t0, int u0, int j0) {
  const int Jp = pad4(J);
  for (int i = threadIdx.x; i < KJ * CP; i += 256) {
    const int j = j0 + i / CP, c = i % CP;
    Ws[i] = (j < J && c < C) ? W[(size_t)j * C + c] : 0.f;
  }
  for (int i = threadIdx.x; i < TS * KJ; i += 256) {
    const int r = i / KJ, jj = i % KJ, j = j0 + jj;
    const int t = t0 + r, u = u0 + r;
    fs[r * (KJ + 1) + jj] = (t < T && j < J) ? enc[((size_t)t * n_pad + n) * Jp + j] : 0.f;
    gs[r * (KJ + 1) + jj] = (u < U1 && j < J) ? pred[((size_t)u * n_pad + n) * Jp + j] : 0.f;
  }
}

// ---- the logits of this thread's cell (local frame lt, local position lu); all 256 threads call
template <int CP>
__device__ __forceinline__ void cell_logits(float (&acc)[CP], float* Ws, float* fs, float* gs,
                                            const float* __restrict__ enc,
                                            const float* __restrict__ pred,
                                            const float* __restrict__ W,
                                            const float* __restrict__ b, int n, int n_pad, int J,
                                            int C, int T, int U1, int t0, int u0, int lt, int lu) {
#pragma unroll
  for (int c = 0; c < CP; ++c) acc[c] = 0.f;
  for (int j0 = 0; j0 < J; j0 += KJ) {
    __syncthreads();
    stage<CP>(Ws, fs, gs, enc, pred, W, n, n_pad, J, C, T, U1, t0, u0, j0);
    __syncthreads();
    const float* fr = fs + lt * (KJ + 1);
    const float* gr = gs + lu * (KJ + 1);
#pragma unroll 4
    for (int jj = 0; jj < KJ; ++jj) {
      const float h = joint_tanh(fr[jj] + gr[jj]);
      const float4* w4 = reinterpret_cast<const float4*>(Ws + jj * CP);
#pragma unroll
      for (int q = 0; q < CP / 4; ++q) {
        const float4 w = w4[q];
        acc[4 * q + 0] = fmaf(h, w.x, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(h, w.y, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(h, w.z, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(h, w.w, acc[4 * q + 3]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CP; ++c) acc[c] = c < C ? acc[c] + b[c] : kNegInf;
}

template <int CP>
__device__ __forceinline__ float logits_lse(const float (&z)[CP]) {
  float m = z[0];
#pragma unroll
  for (int c = 1; c < CP; ++c) m = fmaxf(m, z[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) s += __expf(z[c] - m);
  return m + __logf(s);
}
template <int CP>
__device__ __forceinline__ float pick(const float (&z)[CP], int k) {
  // (a chain of selects on registers; written as a maximum so that it is not turned into an
  // indexed read of a private array)
  float v = kNegInf;
#pragma unroll
  for (int c = 0; c < CP; ++c) v = fmaxf(v, c == k ? z[c] : kNegInf);
  return v;
}

// ---------------------------------------------------------------------------
// phase 1: lp_blank, lp_y of every cell t < T_n, u <= U_n.  grid (u tiles, t tiles, N)
template <int CP>
__global__ void __launch_bounds__(256)
rnnt_lp_kernel(const float* __restrict__ enc, const float* __restrict__ pred,
               const float* __restrict__ W, const float* __restrict__ b,
               const int* __restrict__ labels, const int* __restrict__ label_len,
               const int* __restrict__ seq_len, int T, int U1, int n_pad, int J, int C,
               int l_max, float* __restrict__ lpb, float* __restrict__ lpy) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Ws = lds;
  float* fs = Ws + KJ * CP;
  float* gs = fs + TS * (KJ + 1);
  const int n = blockIdx.z, t0 = blockIdx.y * TS, u0 = blockIdx.x * TS;
  int Tn, Un;
  clamp_lens(seq_len, label_len, n, T, U1, Tn, Un);
  if (t0 >= Tn || u0 > Un) return;
  const int lt = threadIdx.x / TS, lu = threadIdx.x % TS;
  const int t = t0 + lt, u = u0 + lu;
  float z[CP];
  cell_logits<CP>(z, Ws, fs, gs, enc, pred, W, b, n, n_pad, J, C, T, U1, t0, u0, lt, lu);
  if (t < Tn && u <= Un) {
    const float lse = logits_lse<CP>(z);
    const size_t idx = ((size_t)n * (T + U1 - 1) + (t + u)) * U1 + u;
    lpb[idx] = pick<CP>(z, C - 1) - lse;
    lpy[idx] = u < Un ? pick<CP>(z, label_at(labels, n, l_max, u, C)) - lse : kNegInf;
  }
}

// ---------------------------------------------------------------------------
// phase 2: the alpha chain (dir 0) and the beta chain (dir 1) of one utterance.  NW waves.
template <int NW>
struct Chain {
  float* xch;      // [2][NW] boundary lanes, [NW] maxima
  int lane, wave;
  __device__ __forceinline__ float block_max(float v) {
    v = asr_wave_max(v);
    if (NW == 1) return v;
    float* mx = xch + 2 * NW;
    if (lane == 0) mx[wave] = v;
    __syncthreads();
    float m = mx[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) m = fmaxf(m, mx[w]);
    __syncthreads();
    return m;
  }
  // lane u of the workgroup receives lane u - 1 (up) / u + 1 (down); -inf past the ends
  __device__ __forceinline__ float shift(float v, bool up, int step) {
    float r = up ? wave_shift_up(v, kNegInf) : wave_shift_down(v, kNegInf);
    if (NW == 1) return r;
    float* x = xch + (step & 1) * NW;
    if (lane == (up ? 63 : 0)) x[wave] = v;
    __syncthreads();
    if (up) { if (lane == 0 && wave > 0) r = x[wave - 1]; }
    else if (lane == 63 && wave < NW - 1) r = x[wave + 1];
    return r;
  }
};

template <int NW>
__global__ void __launch_bounds__(64 * NW)
rnnt_chain_kernel(const float* __restrict__ lpb, const float* __restrict__ lpy,
                  const int* __restrict__ label_len, const int* __restrict__ seq_len, int T,
                  int U1, float* __restrict__ alpha, float* __restrict__ beta,
                  double* __restrict__ Aoff, double* __restrict__ Boff,
                  double* __restrict__ logz, float* __restrict__ loss, int do_beta) {
  __shared__ float xch[3 * NW];
  Chain<NW> ch;
  ch.xch = xch;
  ch.lane = threadIdx.x & 63;
  ch.wave = threadIdx.x >> 6;
  const int u = threadIdx.x;
  const int n = do_beta ? (blockIdx.x >> 1) : blockIdx.x;
  const int dir = do_beta ? (blockIdx.x & 1) : 0;
  int Tn, Un;
  clamp_lens(seq_len, label_len, n, T, U1, Tn, Un);
  const int D = Tn - 1 + Un;                    // the last anti-diagonal
  const int D1 = T + U1 - 1;
  const size_t base = (size_t)n * D1 * U1;
  const bool lane_ok = u < U1;
  const int uc = lane_ok ? u : 0;
  double off = 0.0;
  // the two log-probabilities of this lane's cell on diagonal d (whatever is there if the cell
  // is outside the lattice: the callers select)
  auto cell_ok = [&](int d) { const int t = d - u; return lane_ok && t >= 0 && t < Tn && u <= Un; };
  if (dir == 0) {
    float v = u == 0 ? 0.f : kNegInf;           // alpha~ on diagonal 0
    if (lane_ok) alpha[base + u] = v;
    if (u == 0) Aoff[(size_t)n * (D1 + 1)] = 0.0;
    float pb = lpb[base + uc], py = lpy[base + uc];
    for (int d = 0; d < D; ++d) {
      // prefetch diagonal d + 1 while this step computes
      const size_t nx = base + (size_t)(d + 1) * U1 + uc;
      const float npb = lpb[nx], npy = lpy[nx];
      const bool ok = cell_ok(d);
      const float a = ok ? v + pb : kNegInf;
      const float bb = (ok && u < Un) ? v + py : kNegInf;
      const float bs = ch.shift(bb, true, d);
      v = cell_ok(d + 1) ? asr_lse2(a, bs) : kNegInf;
      if ((d + 1) % kRecentre == 0) {
        const float m = ch.block_max(v);
        v -= m;
        off += (double)m;
      }
      if (lane_ok) alpha[nx] = v;
      if (u == 0) Aoff[(size_t)n * (D1 + 1) + d + 1] = off;
      pb = npb; py = npy;
    }
    if (u == Un) {
      const double lz = (double)(v + pb) + off;      // pb = lp_blank(T_n - 1, U_n)
      logz[n] = lz;
      loss[n] = (float)(-lz);
    }
  } else {
    float v = u == Un ? 0.f : kNegInf;          // the virtual cell (T_n, U_n) on diagonal D + 1
    if (u == 0) Boff[(size_t)n * (D1 + 1) + D + 1] = 0.0;
    size_t ix = base + (size_t)D * U1 + uc;
    float pb = lpb[ix], py = lpy[ix];
    for (int d = D; d >= 0; --d) {
      const size_t nx = base + (size_t)(d > 0 ? d - 1 : 0) * U1 + uc;
      const float npb = lpb[nx], npy = lpy[nx];
      const float sd = ch.shift(v, false, d);
      const bool ok = cell_ok(d);
      v = ok ? asr_lse2(v + pb, u < Un ? sd + py : kNegInf) : kNegInf;
      if (d % kRecentre == 0) {
        const float m = ch.block_max(v);
        v -= m;
        off += (double)m;
      }
      if (lane_ok) beta[ix] = v;
      if (u == 0) Boff[(size_t)n * (D1 + 1) + d] = off;
      ix = nx; pb = npb; py = npy;
    }
  }
}

// ---------------------------------------------------------------------------
// phase 3.  AX = 0: owner = 16 frames (a), reduced = label positions (r); AX = 1 the other way.
// thread = cell (a = tid / 16, r = tid % 16), so the reduced axis is 16 neighbouring lanes.
template <int CP, int AX>
__global__ void __launch_bounds__(256)
rnnt_bwd_kernel(const float* __restrict__ enc, const float* __restrict__ pred,
                const float* __restrict__ W, const float* __restrict__ b,
                const int* __restrict__ labels, const int* __restrict__ label_len,
                const int* __restrict__ seq_len, int T, int U1, int N, int n_pad, int J, int C,
                int l_max, float scale, const float* __restrict__ lpb,
                const float* __restrict__ lpy, const float* __restrict__ alpha,
                const float* __restrict__ beta, const double* __restrict__ Aoff,
                const double* __restrict__ Boff, const double* __restrict__ logz,
                float* __restrict__ d_out, float* __restrict__ slabs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Ws = lds;
  float* fs = Ws + KJ * CP;
  float* gs = fs + TS * (KJ + 1);
  float* oacc = gs + TS * (KJ + 1);             // [16][J] sums of the owned rows
  float* hs = oacc + TS * pad4(J);              // [256][SJ + 1]   (AX = 0)
  float* dzs = hs + 256 * (SJ + 1) + 3;         // [256][CP]       (AX = 0)
  dzs = lds + ((dzs - lds) / 4) * 4;            // (16-byte aligned)
  constexpr int CPT = CP / 16;
  const int tid = threadIdx.x;
  const int la = tid / TS, lr = tid % TS;
  const int Jp = pad4(J);
  const int D1 = T + U1 - 1;
  const int n_own = AX == 0 ? (T + TS - 1) / TS : (U1 + TS - 1) / TS;
  float* slab = nullptr;
  if (AX == 0) {
    // this workgroup's dW_out / db_out partial: rows 0..J-1 = dW_out, row J = db_out.  A thread
    // owns the entries (j = tid % 16 mod 16, classes (tid / 16) CPT ..) for the whole kernel.
    slab = slabs + (size_t)blockIdx.x * (J + 1) * CP;
    for (int j = lr; j <= J; j += SJ)
#pragma unroll
      for (int k = 0; k < CPT; ++k) slab[(size_t)j * CP + la * CPT + k] = 0.f;
  }
  for (int item = blockIdx.x; item < N * n_own; item += gridDim.x) {
    const int n = item / n_own, o0 = (item % n_own) * TS;
    int Tn, Un;
    clamp_lens(seq_len, label_len, n, T, U1, Tn, Un);
    if (AX == 0 ? o0 >= Tn : o0 > Un) continue;
    const int r_end = AX == 0 ? Un + 1 : Tn;    // reduced positions 0 .. r_end - 1
    __syncthreads();
    for (int i = tid; i < TS * Jp; i += 256) oacc[i] = 0.f;
    const double lz = logz[n];
    for (int r0 = 0; r0 < r_end; r0 += TS) {
      const int t0 = AX == 0 ? o0 : r0, u0 = AX == 0 ? r0 : o0;
      const int lt = AX == 0 ? la : lr, lu = AX == 0 ? lr : la;
      const int t = t0 + lt, u = u0 + lu;
      float z[CP];
      cell_logits<CP>(z, Ws, fs, gs, enc, pred, W, b, n, n_pad, J, C, T, U1, t0, u0, lt, lu);
      // ---- dz of this cell (in place), 0 outside the lattice
      if (t < Tn && u <= Un) {
        const float lse = logits_lse<CP>(z);
        const int d = t + u;
        const size_t idx = ((size_t)n * D1 + d) * U1 + u;
        const double* A = Aoff + (size_t)n * (D1 + 1);
        const double* B = Boff + (size_t)n * (D1 + 1);
        const float al = alpha[idx];
        const float e0 = (float)(A[d] + B[d] - lz);
        const float e1 = (float)(A[d] + B[d + 1] - lz);
        const float occ = __expf(al + beta[idx] + e0);
        float gb = 0.f, gy = 0.f;
        if (t + 1 < Tn) gb = __expf((al + beta[idx + U1]) + lpb[idx] + e1);
        else if (u == Un) gb = __expf(al + lpb[idx] + e1);
        int y = -1;
        if (u < Un) {
          y = label_at(labels, n, l_max, u, C);
          gy = __expf((al + beta[idx + U1 + 1]) + lpy[idx] + e1);
        }
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          float g = occ * __expf(z[c] - lse);
          g -= c == C - 1 ? gb : 0.f;
          g -= c == y ? gy : 0.f;
          z[c] = c < C ? scale * g : 0.f;
        }
      } else {
#pragma unroll
        for (int c = 0; c < CP; ++c) z[c] = 0.f;
      }
      if (AX == 0) {
        float4* o = reinterpret_cast<float4*>(dzs + tid * CP);
#pragma unroll
        for (int q = 0; q < CP / 4; ++q)
          o[q] = make_float4(z[4 * q], z[4 * q + 1], z[4 * q + 2], z[4 * q + 3]);
      }
      // ---- dh = dz W_out^T, dpre = dh (1 - h^2), summed over the 16 reduced lanes; AX = 0 also
      // h (x) dz, with the virtual row j = J (h = 1) giving db_out
      const int j_end = AX == 0 ? J + 1 : J;
      for (int j0 = 0; j0 < j_end; j0 += KJ) {
        __syncthreads();
        stage<CP>(Ws, fs, gs, enc, pred, W, n, n_pad, J, C, T, U1, t0, u0, j0);
        __syncthreads();
        const float* fr = fs + lt * (KJ + 1);
        const float* gr = gs + lu * (KJ + 1);
        for (int s0 = 0; s0 < KJ && j0 + s0 < j_end; s0 += SJ) {
#pragma unroll 4
          for (int jl = 0; jl < SJ; ++jl) {
            const int jj = s0 + jl, j = j0 + jj;
            const float h = joint_tanh(fr[jj] + gr[jj]);
            const float4* w4 = reinterpret_cast<const float4*>(Ws + jj * CP);
            float dh0 = 0.f, dh1 = 0.f;
#pragma unroll
            for (int q = 0; q < CP / 4; ++q) {
              const float4 w = w4[q];
              dh0 = fmaf(z[4 * q + 0], w.x, dh0);
              dh1 = fmaf(z[4 * q + 1], w.y, dh1);
              dh0 = fmaf(z[4 * q + 2], w.z, dh0);
              dh1 = fmaf(z[4 * q + 3], w.w, dh1);
            }
            float v = (dh0 + dh1) * (1.f - h * h);
            v = row16_sum(v);
            if (lr == TS - 1 && j < J) oacc[la * Jp + j] += v;
            if (AX == 0) hs[tid * (SJ + 1) + jl] = j < J ? h : (j == J ? 1.f : 0.f);
          }
          if (AX == 0) {
            __syncthreads();
            // thread (row lr of this pass, classes la CPT ..): sum over the tile's 256 cells
            // (four interleaved partial sums per entry, added in a fixed order: the loop is
            // bound by the latency of its dependent FMAs otherwise)
            float aw4[4][CPT];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int k = 0; k < CPT; ++k) aw4[q][k] = 0.f;
#pragma unroll 2
            for (int cell = 0; cell < 256; cell += 4) {
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const float hv = hs[(cell + q) * (SJ + 1) + lr];
                const float* dzr = dzs + (cell + q) * CP + la * CPT;
#pragma unroll
                for (int k = 0; k < CPT; ++k) aw4[q][k] = fmaf(hv, dzr[k], aw4[q][k]);
              }
            }
            float aw[CPT];
#pragma unroll
            for (int k = 0; k < CPT; ++k) aw[k] = (aw4[0][k] + aw4[1][k]) + (aw4[2][k] + aw4[3][k]);
            const int j = j0 + s0 + lr;
            if (j <= J) {
#pragma unroll
              for (int k = 0; k < CPT; ++k) slab[(size_t)j * CP + la * CPT + k] += aw[k];
            }
            __syncthreads();
          }
        }
      }
    }
    __syncthreads();
    // ---- the owned rows: written once, rows outside the lattice keep the caller's zeros
    for (int i = tid; i < TS * J; i += 256) {
      const int a = i / J, j = i % J, o = o0 + a;
      if (AX == 0 ? o < Tn : o <= Un)
        d_out[((size_t)o * n_pad + n) * Jp + j] = oacc[a * Jp + j];
    }
  }
}

// ---------------------------------------------------------------------------
// one iteration of greedy decoding: one wave per utterance
__global__ void __launch_bounds__(64)
rnnt_greedy_kernel(const float* __restrict__ enc, const float* __restrict__ g_cur,
                   const float* __restrict__ W, const float* __restrict__ b,
                   const int* __restrict__ seq_len, int T, int n_pad, int J, int C,
                   int max_symbols, int cap, int ld_next, int* __restrict__ t_ptr,
                   int* __restrict__ n_sym, int* __restrict__ decoded,
                   int* __restrict__ decoded_len, int* __restrict__ advance,
                   float* __restrict__ x_next, int* __restrict__ active) {
  __shared__ float hsh[512];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int Jp = pad4(J);
  int Tn = seq_len[n];
  Tn = Tn < 0 ? 0 : (Tn > T ? T : Tn);
  const int t = t_ptr[n];
  float* xr = x_next + (size_t)n * ld_next;
  for (int c = lane; c < ld_next; c += 64) xr[c] = 0.f;
  if (t < 0 || t >= Tn) {                       // the utterance has ended
    if (lane == 0) advance[n] = 0;
    return;
  }
  const float* f = enc + ((size_t)t * n_pad + n) * Jp;
  const float* g = g_cur + (size_t)n * Jp;
  for (int j = lane; j < J; j += 64) hsh[j] = joint_tanh(f[j] + g[j]);
  __syncthreads();
  float z = kNegInf;
  if (lane < C) {
    float s = 0.f;
    for (int j = 0; j < J; ++j) s = fmaf(hsh[j], W[(size_t)j * C + lane], s);
    z = s + b[lane];
  }
  // first-max arg-max over the lanes
  int k = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float zo = __shfl_xor(z, o, 64);
    const int ko = __shfl_xor(k, o, 64);
    if (zo > z || (zo == z && ko < k)) { z = zo; k = ko; }
  }
  if (lane == 0) {
    const int ns = n_sym[n];
    if (k != C - 1 && ns < max_symbols) {
      const int len = decoded_len[n];
      if (len < cap) decoded[(size_t)n * cap + len] = k;
      decoded_len[n] = len + 1 < cap ? len + 1 : cap;
      n_sym[n] = ns + 1;
      advance[n] = 1;
      if (k < ld_next) xr[k] = 1.f;
      atomicAdd(active, 1);
    } else {
      t_ptr[n] = t + 1;
      n_sym[n] = 0;
      advance[n] = 0;
      if (t + 1 < Tn) atomicAdd(active, 1);
    }
  }
}

// out (U1, n_pad, ld): row (u, n) = e_{y_u} for 1 <= u <= U_n, n < N, else 0
__global__ void __launch_bounds__(256)
rnnt_onehot_kernel(const int* __restrict__ labels, const int* __restrict__ label_len, int U1,
                   int N, int n_pad, int l_max, int width, int ld, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)U1 * n_pad * ld) return;
  const int k = (int)(i % ld);
  const int n = (int)((i / ld) % n_pad);
  const int u = (int)(i / ((size_t)ld * n_pad));
  float v = 0.f;
  if (n < N && u >= 1 && k < width) {
    int Un = label_len[n];
    Un = Un > l_max ? l_max : Un;
    if (u <= Un && labels[(size_t)n * l_max + u - 1] == k) v = 1.f;
  }
  out[i] = v;
}

__global__ void __launch_bounds__(256)
rnnt_rows_select_kernel(const int* __restrict__ mask, const float* a, const float* b, float* out,
                        int N, int n_pad, int width) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n_pad * width) return;
  const int n = (int)(i / width);
  const bool m = n < N && mask[n] != 0;
  out[i] = m ? a[i] : b[i];
}

struct WsLayout {
  size_t cell, offs, lz, slabs, total;
};
bool ws_layout(int T, int U1, int N, int n_pad, int J, int C, WsLayout* w) {
  if (T < 1 || U1 < 1 || U1 > 256 || N < 1 || n_pad < N || J < 1 || J > 512 || C < 2 || C > 64 ||
      T > kMaxT)
    return false;
  const size_t D1 = (size_t)T + U1 - 1;
  w->cell = asr_align_up((size_t)N * D1 * U1 * sizeof(float), 256);
  w->offs = asr_align_up((size_t)N * (D1 + 1) * sizeof(double), 256);
  w->lz = asr_align_up((size_t)N * sizeof(double), 256);
  w->slabs = asr_align_up((size_t)kSlabs * (J + 1) * class_pad(C) * sizeof(float), 256);
  w->total = 4 * w->cell + 2 * w->offs + w->lz + w->slabs;
  return true;
}

template <int CP>
int launch_joint(const float* enc, const float* pred, const float* W, const float* b,
                 const int* labels, const int* label_len, const int* seq_len, int T, int U1,
                 int N, int n_pad, int J, int C, int l_max, float scale, float* lpb, float* lpy,
                 float* alpha, float* beta, double* Aoff, double* Boff, double* logz, float* loss,
                 float* d_enc, float* d_pred, float* dW, float* db, float* slabs,
                 hipStream_t stream) {
  const int Jp = pad4(J);
  const size_t lds_fwd = (size_t)(KJ * CP + 2 * TS * (KJ + 1)) * sizeof(float);
  const size_t lds_b1 = lds_fwd + (size_t)(TS * Jp + 4) * sizeof(float);
  const size_t lds_b0 = lds_b1 + (size_t)(256 * (SJ + 1) + 256 * CP) * sizeof(float);
  const bool grads = d_enc != nullptr;
  const dim3 g1((U1 + TS - 1) / TS, (T + TS - 1) / TS, N);
  hipLaunchKernelGGL(rnnt_lp_kernel<CP>, g1, dim3(256), lds_fwd, stream, enc, pred, W, b, labels,
                     label_len, seq_len, T, U1, n_pad, J, C, l_max, lpb, lpy);
  ASR_CHECK_LAUNCH();
  const dim3 g2(grads ? 2 * N : N);
#define LAUNCH_CHAIN(NW)                                                                       \
  hipLaunchKernelGGL(rnnt_chain_kernel<NW>, g2, dim3(64 * NW), 0, stream, lpb, lpy, label_len, \
                     seq_len, T, U1, alpha, beta, Aoff, Boff, logz, loss, grads ? 1 : 0)
  if (U1 <= 64) LAUNCH_CHAIN(1);
  else if (U1 <= 128) LAUNCH_CHAIN(2);
  else LAUNCH_CHAIN(4);
#undef LAUNCH_CHAIN
  ASR_CHECK_LAUNCH();
  if (!grads) return ASR_OK;
  ASR_CHECK_HIP(hipMemsetAsync(d_enc, 0, (size_t)T * n_pad * Jp * sizeof(float), stream));
  ASR_CHECK_HIP(hipMemsetAsync(d_pred, 0, (size_t)U1 * n_pad * Jp * sizeof(float), stream));
  // (once per instance, for the largest J: the call itself stays a sequence of stream operations)
  static bool lds_opted_in = false;
  if (!lds_opted_in) {
    const int lds_max = (int)((KJ * CP + 2 * TS * (KJ + 1) + TS * 512 + 4 + 256 * (SJ + 1) +
                               256 * CP) * sizeof(float));
    ASR_CHECK_HIP(hipFuncSetAttribute((const void*)rnnt_bwd_kernel<CP, 0>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    lds_opted_in = true;
  }
  hipLaunchKernelGGL((rnnt_bwd_kernel<CP, 0>), dim3(kSlabs), dim3(256), lds_b0, stream, enc, pred,
                     W, b, labels, label_len, seq_len, T, U1, N, n_pad, J, C, l_max, scale, lpb,
                     lpy, alpha, beta, Aoff, Boff, logz, d_enc, slabs);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL((rnnt_bwd_kernel<CP, 1>), dim3(N * ((U1 + TS - 1) / TS)), dim3(256), lds_b1,
                     stream, enc, pred, W, b, labels, label_len, seq_len, T, U1, N, n_pad, J, C,
                     l_max, scale, lpb, lpy, alpha, beta, Aoff, Boff, logz, d_pred,
                     (float*)nullptr);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(joint_slab_sum_kernel, dim3(((J + 1) * C + 255) / 256), dim3(256), 0, stream,
                     slabs, kSlabs, J, C, CP, dW, db);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

}  // namespace

extern "C" size_t asr_rnnt_workspace_bytes(int T, int U1, int N, int n_pad, int J, int C) {
  WsLayout w;
  return ws_layout(T, U1, N, n_pad, J, C, &w) ? w.total : 0;
}

extern "C" int asr_rnnt_loss_grad(const float* enc, const float* pred, const float* W_out,
                                  const float* b_out, const int* labels, const int* label_len,
                                  const int* seq_len, int T, int U1, int N, int n_pad, int J,
                                  int C, int l_max, float grad_scale, float* loss, float* d_enc,
                                  float* d_pred, float* dW_out, float* db_out, void* workspace,
                                  size_t ws_bytes, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(enc && pred && W_out && b_out && label_len && seq_len && loss,
                "rnnt_loss_grad: null pointer");
  ASR_CHECK_ARG(T >= 1 && T <= kMaxT && N >= 1 && N <= 65535 && n_pad >= N &&
                    n_pad % 16 == 0,
                "rnnt_loss_grad: bad shape T=%d N=%d n_pad=%d", T, N, n_pad);
  ASR_CHECK_ARG(J >= 1 && J <= 512, "rnnt_loss_grad: J=%d (1 .. 512)", J);
  ASR_CHECK_ARG(C >= 2 && C <= 64, "rnnt_loss_grad: C=%d (2 .. 64)", C);
  ASR_CHECK_ARG(l_max >= 0 && l_max <= 255 && U1 == l_max + 1,
                "rnnt_loss_grad: l_max=%d (0 .. 255), U1=%d (l_max + 1)", l_max, U1);
  ASR_CHECK_ARG(labels || l_max == 0, "rnnt_loss_grad: null labels");
  const int ng = (d_enc != nullptr) + (d_pred != nullptr) + (dW_out != nullptr) +
                 (db_out != nullptr);
  ASR_CHECK_ARG(ng == 0 || ng == 4,
                "rnnt_loss_grad: the four gradient pointers are all NULL (loss only) or all set");
  ASR_CHECK_ARG(!d_enc || (d_enc != enc && d_pred != pred && d_enc != d_pred),
                "rnnt_loss_grad: a gradient must not alias its input");
  WsLayout w;
  ws_layout(T, U1, N, n_pad, J, C, &w);
  if (!workspace || ws_bytes < w.total) {
    asr_set_error("rnnt_loss_grad: workspace %zu < %zu bytes", ws_bytes, w.total);
    return ASR_ERR_WORKSPACE;
  }
  ASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "rnnt_loss_grad: workspace alignment");
  char* p = reinterpret_cast<char*>(workspace);
  float* lpb = reinterpret_cast<float*>(p);
  float* lpy = reinterpret_cast<float*>(p + w.cell);
  float* alpha = reinterpret_cast<float*>(p + 2 * w.cell);
  float* beta = reinterpret_cast<float*>(p + 3 * w.cell);
  double* Aoff = reinterpret_cast<double*>(p + 4 * w.cell);
  double* Boff = reinterpret_cast<double*>(p + 4 * w.cell + w.offs);
  double* logz = reinterpret_cast<double*>(p + 4 * w.cell + 2 * w.offs);
  float* slabs = reinterpret_cast<float*>(p + 4 * w.cell + 2 * w.offs + w.lz);
#define JOINT(CP)                                                                               \
  return launch_joint<CP>(enc, pred, W_out, b_out, labels, label_len, seq_len, T, U1, N, n_pad, \
                          J, C, l_max, grad_scale, lpb, lpy, alpha, beta, Aoff, Boff, logz,     \
                          loss, d_enc, d_pred, dW_out, db_out, slabs, stream)
  switch (class_pad(C)) {
    case 16: JOINT(16);
    case 32: JOINT(32);
    default: JOINT(64);
  }
#undef JOINT
}

extern "C" int asr_rnnt_greedy_step(const float* enc, const float* g_cur, const float* W_out,
                                    const float* b_out, const int* seq_len, int T, int N,
                                    int n_pad, int J, int C, int max_symbols, int cap,
                                    int ld_next, int* t_ptr, int* n_sym, int* decoded,
                                    int* decoded_len, int* advance, float* x_next, int* active,
                                    asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(enc && g_cur && W_out && b_out && seq_len && t_ptr && n_sym && decoded &&
                    decoded_len && advance && x_next && active,
                "rnnt_greedy_step: null pointer");
  ASR_CHECK_ARG(T >= 1 && N >= 1 && n_pad >= N && n_pad % 16 == 0,
                "rnnt_greedy_step: bad shape T=%d N=%d n_pad=%d", T, N, n_pad);
  ASR_CHECK_ARG(J >= 1 && J <= 512 && C >= 2 && C <= 64,
                "rnnt_greedy_step: J=%d (1 .. 512), C=%d (2 .. 64)", J, C);
  ASR_CHECK_ARG(max_symbols >= 1 && cap >= 1 && ld_next >= C - 1,
                "rnnt_greedy_step: max_symbols=%d, cap=%d, ld_next=%d (>= C - 1)", max_symbols,
                cap, ld_next);
  ASR_CHECK_HIP(hipMemsetAsync(active, 0, sizeof(int), stream));
  hipLaunchKernelGGL(rnnt_greedy_kernel, dim3(N), dim3(64), 0, stream, enc, g_cur, W_out, b_out,
                     seq_len, T, n_pad, J, C, max_symbols, cap, ld_next, t_ptr, n_sym, decoded,
                     decoded_len, advance, x_next, active);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_onehot_rows(const int* labels, const int* label_len, int U1, int N, int n_pad,
                               int l_max, int width, int ld, float* out, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(label_len && out && (labels || l_max == 0), "onehot_rows: null pointer");
  ASR_CHECK_ARG(U1 >= 1 && U1 == l_max + 1 && N >= 1 && n_pad >= N && width >= 1 && ld >= width,
                "onehot_rows: bad shape U1=%d l_max=%d N=%d n_pad=%d width=%d ld=%d", U1, l_max,
                N, n_pad, width, ld);
  const size_t total = (size_t)U1 * n_pad * ld;
  ASR_CHECK_ARG(total < ((size_t)1 << 38), "onehot_rows: slab too large");
  hipLaunchKernelGGL(rnnt_onehot_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     stream, labels, label_len, U1, N, n_pad, l_max, width, ld, out);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_rows_select(const int* mask, const float* a, const float* b, float* out, int N,
                               int n_pad, int width, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(mask && a && b && out, "rows_select: null pointer");
  ASR_CHECK_ARG(N >= 0 && n_pad >= N && n_pad >= 1 && width >= 1,
                "rows_select: bad shape N=%d n_pad=%d width=%d", N, n_pad, width);
  const size_t total = (size_t)n_pad * width;
  hipLaunchKernelGGL(rnnt_rows_select_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     stream, mask, a, b, out, N, n_pad, width);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
