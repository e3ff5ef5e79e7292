// K15 BatchNormalization (Keras 1.2.2, mode 0, axis -1) over a time-major slab (T, n_pad, ld).
//
// Training: y = gamma * (x - mu) * invstd + beta, mu / var the biased moments of every real row
// (n < N of each frame, all T frames) per channel; channel = column % C (C == W: a plain 2-D
// tensor; C < W: the (N, T, F, C) conv image, W = F * C).  Inference: the same map with the
// running moments.  Backward: dbeta = sum dy, dgamma = sum dy * xhat, dx = gamma * invstd *
// (dy - mean(dy) - xhat * mean(dy * xhat)).  An optional clip fuses a following clipped ReLU
// (forward min(max(y, 0), clip); backward masks dy with 0 < y < clip, y recomputed from x).
//
// Every pass walks the slab with one 16-byte column group per thread: a workgroup is rw row
// lanes x cw column lanes (cw float4 groups = a tile of 4 * cw columns), so a thread's channel
// coefficients are loaded once.  Reductions: each thread sums its rows in fp64 (statistics
// shifted by the row-0 value of the channel), the workgroup folds its row lanes -- and, for the
// conv image, the columns of one channel -- in LDS in a fixed order, writes one partial per
// (partition, tile, slot), and a finalize kernel adds the partials in a fixed order.  No float
// atomics: two identical calls give identical bits.  Padding rows (n >= N) and padding columns
// (W <= col < ld) of y and dx are written as zeros.
#include "common.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_TARGET_BLOCKS = 1024;

struct BnGeo {
  int cw, rw, tw, ntiles, slots, P, grouped;
  long long nreal, rpp;   // real rows, real rows per partition
};

bool bn_geo(int T, int N, int n_pad, int ld, int W, int C, BnGeo* g) {
  if (T < 1 || N < 1 || n_pad < N || ld < 4 || (ld & 3) || W < 1 || W > ld || C < 1) return false;
  g->grouped = C < W;
  if (g->grouped) {
    // the conv image: no pad columns, 16-byte groups never straddle two channels
    if (W != ld || W % C || (C & 3) || C > 256) return false;
    const int q = C / 4;
    g->cw = (64 / q) * q;
    if (g->cw > ld / 4) g->cw = ld / 4;
  } else {
    if (C != W) return false;
    g->cw = ld / 4 < 64 ? ld / 4 : 64;
  }
  g->rw = BN_THREADS / g->cw;
  g->tw = 4 * g->cw;
  g->ntiles = (ld + g->tw - 1) / g->tw;
  g->slots = g->grouped ? C : g->tw;
  g->nreal = (long long)T * N;
  long long p = (BN_TARGET_BLOCKS + g->ntiles - 1) / g->ntiles;
  const long long pmax = (g->nreal + g->rw - 1) / g->rw;
  if (p > pmax) p = pmax;
  if (p < 1) p = 1;
  g->P = (int)p;
  g->rpp = (g->nreal + p - 1) / p;
  return true;
}

size_t bn_partial_bytes(const BnGeo& g) {
  return asr_align_up((size_t)g.P * g.ntiles * g.slots * 2 * sizeof(double), 256);
}

// grid-stride geometry of the element-wise passes: (ntiles, py) workgroups over all T * n_pad rows
int bn_apply_py(const BnGeo& g, long long rows) {
  long long py = (2 * BN_TARGET_BLOCKS + g.ntiles - 1) / g.ntiles;
  const long long pmax = (rows + g.rw - 1) / g.rw;
  if (py > pmax) py = pmax;
  return (int)(py < 1 ? 1 : py);
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float f4get(const float4& v, int k) {
  return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w));
}

// Sums of one thread's column group over its rows, folded over the workgroup's row lanes (and
// over the channel's columns for the conv image), written as one partial per slot.
// mode 0: statistics (x - shift, (x - shift)^2); mode 1: backward (dy', dy' * xhat).
template <int MODE>
__global__ void __launch_bounds__(BN_THREADS)
bn_reduce_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                 const float* __restrict__ gamma, const float* __restrict__ beta,
                 const float* __restrict__ stats, int N, int n_pad, int ld, int W, int C,
                 int cw, int rw, int tw, int ntiles, int slots, int grouped, long long nreal,
                 long long rpp, float clip, double2* __restrict__ part) {
  __shared__ double red[2][BN_THREADS * 4];
  const int tid = threadIdx.x, tile = blockIdx.x, p = blockIdx.y;
  const int cl = tid % cw, rl = tid / cw;
  const int col = tile * tw + cl * 4;
  const bool act = rl < rw && col < ld;
  double s1[4] = {0., 0., 0., 0.}, s2[4] = {0., 0., 0., 0.};
  if (act) {
    const int ch = grouped ? col % C : col;     // channel of the group's first column
    const long long i0 = (long long)p * rpp;
    long long i1 = i0 + rpp;
    if (i1 > nreal) i1 = nreal;
    if (MODE == 0) {
      const float4 k = ld4(x + ch);           // row 0 (frame 0, sample 0) is always real
      for (long long i = i0 + rl; i < i1; i += rw) {
        const long long t = i / N, n = i - t * N;
        const float4 v = ld4(x + (size_t)(t * n_pad + n) * ld + col);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double d = (double)f4get(v, q) - (double)f4get(k, q);
          s1[q] += d;
          s2[q] = fma(d, d, s2[q]);
        }
      }
    } else {
      // (scalar loads: C need not be a multiple of 4, pad columns have no coefficients)
      float mh[4], ml[4], is[4], ga[4], be[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = col + q < W ? ch + q : 0;
        mh[q] = stats[c];
        ml[q] = stats[C + c];
        is[q] = stats[2 * C + c];
        ga[q] = gamma[c];
        be[q] = beta[c];
      }
      for (long long i = i0 + rl; i < i1; i += rw) {
        const long long t = i / N, n = i - t * N;
        const size_t o = (size_t)(t * n_pad + n) * ld + col;
        const float4 v = ld4(x + o), g = ld4(dy + o);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float xc = (f4get(v, q) - mh[q]) - ml[q];
          const float xh = xc * is[q];
          float d = f4get(g, q);
          if (clip > 0.f) {
            const float z = fmaf(xc, is[q] * ga[q], be[q]);
            d = (z > 0.f && z < clip) ? d : 0.f;
          }
          s1[q] += (double)d;
          s2[q] = fma((double)d, (double)xh, s2[q]);
        }
      }
    }
  }
  if (rl < rw) {      // (rw * tw <= 4 * BN_THREADS; idle lanes past rw own no slot)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      red[0][rl * tw + cl * 4 + q] = act ? s1[q] : 0.;
      red[1][rl * tw + cl * 4 + q] = act ? s2[q] : 0.;
    }
  }
  __syncthreads();
  // fold the row lanes: thread j owns column j of the tile (fixed order)
  double a = 0., b = 0.;
  if (tid < tw) {
    for (int r = 0; r < rw; ++r) {
      a += red[0][r * tw + tid];
      b += red[1][r * tw + tid];
    }
  }
  __syncthreads();
  double2* out = part + ((size_t)p * ntiles + tile) * slots;
  if (!grouped) {
    if (tid < tw) out[tid] = make_double2(a, b);
    return;
  }
  // the conv image: fold the tile's columns of each channel (fixed order)
  if (tid < tw) {
    red[0][tid] = a;
    red[1][tid] = b;
  }
  __syncthreads();
  if (tid < C) {
    int cols = ld - tile * tw;
    if (cols > tw) cols = tw;
    double u = 0., v = 0.;
    for (int j = tid; j < cols; j += C) {
      u += red[0][j];
      v += red[1][j];
    }
    out[tid] = make_double2(u, v);
  }
}

// One wave per channel: adds the partials in a fixed order.
// mode 0 -> stats [mean_hi | mean_lo | invstd | var] (4C floats) and the optional moments of the
// running update [w, 0, 0, 0 | w * d (C) | w * (var + d^2) (C)], d = mean - shift.
// mode 1 -> dgamma, dbeta and coef [mean(dy') | mean(dy' * xhat)] (2C floats).
template <int MODE>
__global__ void bn_finalize_kernel(const double2* __restrict__ part, const float* __restrict__ x,
                                   int C, int W, int ntiles, int tw, int slots, int P,
                                   int grouped, double cnt, float eps, float* __restrict__ stats,
                                   float* __restrict__ moments, const float* __restrict__ shift,
                                   float weight, float* __restrict__ dgamma,
                                   float* __restrict__ dbeta, float* __restrict__ coef) {
  // one wave per channel: lane l adds partials l, l + 64, ... in order, then a fixed xor tree
  const int c = blockIdx.x, lane = threadIdx.x;
  double a = 0., b = 0.;
  if (grouped) {
    for (int k = lane; k < P * ntiles; k += ASR_WAVE) {
      const double2 v = part[(size_t)k * slots + c];
      a += v.x;
      b += v.y;
    }
  } else {
    const int t = c / tw, s = c % tw;
    for (int p = lane; p < P; p += ASR_WAVE) {
      const double2 v = part[((size_t)p * ntiles + t) * slots + s];
      a += v.x;
      b += v.y;
    }
  }
  a = asr_wave_sum_d(a);
  b = asr_wave_sum_d(b);
  if (lane != 0) return;
  if (MODE == 0) {
    const double dm = a / cnt;
    const double mean = (double)x[c] + dm;
    double var = b / cnt - dm * dm;
    var = var > 0. ? var : 0.;
    const float mh = (float)mean;
    stats[c] = mh;
    stats[C + c] = (float)(mean - (double)mh);
    stats[2 * C + c] = (float)(1.0 / sqrt(var + (double)eps));
    stats[3 * C + c] = (float)var;
    if (moments != nullptr) {
      const double d = mean - (double)(shift != nullptr ? shift[c] : mh);
      moments[4 + c] = (float)((double)weight * d);
      moments[4 + C + c] = (float)((double)weight * (var + d * d));
      if (c == 0) {
        moments[0] = weight;
        moments[1] = moments[2] = moments[3] = 0.f;
      }
    }
  } else {
    dbeta[c] = (float)a;
    dgamma[c] = (float)b;
    coef[c] = (float)(a / cnt);
    coef[C + c] = (float)(b / cnt);
  }
  (void)W;
}

// Element-wise passes over all T * n_pad rows.  MODE 0: training apply (stats), 1: inference
// apply (running mean / variance), 2: backward dx (stats + coef).
template <int MODE>
__global__ void __launch_bounds__(BN_THREADS)
bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                const float* __restrict__ gamma, const float* __restrict__ beta,
                const float* __restrict__ stats, const float* __restrict__ rmean,
                const float* __restrict__ rvar, const float* __restrict__ coef,
                float* __restrict__ out, int N, int n_pad, int ld, int W, int C, int cw, int rw,
                int tw, int grouped, long long rows, float eps, float clip) {
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int cl = tid % cw, rl = tid / cw;
  const int col = tile * tw + cl * 4;
  if (rl >= rw || col >= ld) return;
  const int ch = grouped ? col % C : col;
  // the thread's four columns: coefficients (pad columns W <= col < ld: written as zeros)
  float mh[4], ml[4], is[4], ga[4], be[4], cb[4], cc[4];
  bool ok[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    ok[q] = col + q < W;
    const int c = ok[q] ? ch + q : 0;
    ga[q] = gamma[c];
    be[q] = beta[c];
    if (MODE == 1) {
      mh[q] = rmean[c];
      ml[q] = 0.f;
      is[q] = 1.f / sqrtf(rvar[c] + eps);
    } else {
      mh[q] = stats[c];
      ml[q] = stats[C + c];
      is[q] = stats[2 * C + c];
    }
    if (MODE == 2) {
      cb[q] = coef[c];
      cc[q] = coef[C + c];
    }
  }
  const long long step = (long long)rw * gridDim.y;
  for (long long r = (long long)blockIdx.y * rw + rl; r < rows; r += step) {
    const size_t o = (size_t)r * ld + col;
    const int n = (int)(r % n_pad);
    float res[4] = {0.f, 0.f, 0.f, 0.f};
    if (n < N) {
      const float4 v = ld4(x + o);
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
      if (MODE == 2) g = ld4(dy + o);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float xc = (f4get(v, q) - mh[q]) - ml[q];
        const float a = is[q] * ga[q];
        const float z = fmaf(xc, a, be[q]);
        if (MODE == 2) {
          float d = f4get(g, q);
          if (clip > 0.f) d = (z > 0.f && z < clip) ? d : 0.f;
          const float xh = xc * is[q];
          res[q] = ok[q] ? a * ((d - cb[q]) - xh * cc[q]) : 0.f;
        } else {
          const float y = clip > 0.f ? fminf(fmaxf(z, 0.f), clip) : z;
          res[q] = ok[q] ? y : 0.f;
        }
      }
    }
    st4(out + o, make_float4(res[0], res[1], res[2], res[3]));
  }
}

__device__ __forceinline__ bool bn_flag(const int* f) { return f != nullptr && *f != 0; }

__global__ void bn_update_kernel(float* __restrict__ rmean, float* __restrict__ rvar,
                                 const float* __restrict__ moments,
                                 const float* __restrict__ shift, int C, float momentum,
                                 const int* fa, const int* fb, const int* fc, const int* fd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  // a vetoed step (any timeout word / all-reduced flag slot set) leaves the statistics alone
  if (bn_flag(fa) || bn_flag(fb) || bn_flag(fc) || bn_flag(fd)) return;
  const double w = (double)moments[0];
  if (!(w > 0.)) return;
  const double d = (double)moments[4 + c] / w;
  const double r = (double)(shift != nullptr ? shift[c] : rmean[c]);
  double var = (double)moments[4 + C + c] / w - d * d;
  var = var > 0. ? var : 0.;
  const float mom = momentum, one_m = 1.f - momentum;
  const float bm = (float)(r + d), bv = (float)var;
  rmean[c] = mom * rmean[c] + one_m * bm;
  rvar[c] = mom * rvar[c] + one_m * bv;
}

// ---------------------------------------------------------------------------------------------
// K18 sequence-wise BatchNormalization of a recurrent layer's input projection p (T, n_pad, ld),
// W real columns, one channel per column (cell-agnostic: only the slab width is known here).
// The statistics are taken over the VALID rows (n < N, t < min(len_n, T)); every real row (n < N,
// all T frames) is normalised with them, so time-padding frames contribute nothing to mu / var
// but still get a value.  Backward: dbeta = sum_R da, dgamma = sum_R da * xhat, dp = gamma *
// invstd * (da - [valid] (dbeta / |V| + xhat * dgamma / |V|)).  Same workgroup geometry, fp64
// partials and fixed-order folds as K15 above (the plain 2-D case, C == W).
// stats (4W + 4 floats): [mean_hi | mean_lo | invstd | var | |V|, 0, 0, 0].

__device__ __forceinline__ int seqbn_len(const int* __restrict__ lens, int n, int T) {
  if (lens == nullptr) return T;
  const int l = lens[n];
  return l < 0 ? 0 : (l > T ? T : l);
}

// mode 0: statistics over V (p - shift, (p - shift)^2), shift = row (0, 0) of the column;
// mode 1: backward sums over R (da, da * xhat).
template <int MODE>
__global__ void __launch_bounds__(BN_THREADS)
seqbn_reduce_kernel(const float* __restrict__ p, const float* __restrict__ da,
                    const float* __restrict__ stats, const int* __restrict__ lens, int T, int N,
                    int n_pad, int ld, int W, int cw, int rw, int tw, int ntiles,
                    long long nreal, long long rpp, double2* __restrict__ part) {
  __shared__ double red[2][BN_THREADS * 4];
  const int tid = threadIdx.x, tile = blockIdx.x, pt = blockIdx.y;
  const int cl = tid % cw, rl = tid / cw;
  const int col = tile * tw + cl * 4;
  const bool act = rl < rw && col < ld;
  double s1[4] = {0., 0., 0., 0.}, s2[4] = {0., 0., 0., 0.};
  if (act) {
    const long long i0 = (long long)pt * rpp;
    long long i1 = i0 + rpp;
    if (i1 > nreal) i1 = nreal;
    if (MODE == 0) {
      const float4 k = ld4(p + col);
      for (long long i = i0 + rl; i < i1; i += rw) {
        const long long t = i / N;
        const int n = (int)(i - t * N);
        if (t >= seqbn_len(lens, n, T)) continue;
        const float4 v = ld4(p + (size_t)(t * n_pad + n) * ld + col);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double d = (double)f4get(v, q) - (double)f4get(k, q);
          s1[q] += d;
          s2[q] = fma(d, d, s2[q]);
        }
      }
    } else {
      float mh[4], ml[4], is[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = col + q < W ? col + q : 0;
        mh[q] = stats[c];
        ml[q] = stats[W + c];
        is[q] = stats[2 * W + c];
      }
      for (long long i = i0 + rl; i < i1; i += rw) {
        const long long t = i / N, n = i - t * N;
        const size_t o = (size_t)(t * n_pad + n) * ld + col;
        const float4 v = ld4(p + o), g = ld4(da + o);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float xh = ((f4get(v, q) - mh[q]) - ml[q]) * is[q];
          const float d = f4get(g, q);
          s1[q] += (double)d;
          s2[q] = fma((double)d, (double)xh, s2[q]);
        }
      }
    }
  }
  if (rl < rw) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      red[0][rl * tw + cl * 4 + q] = act ? s1[q] : 0.;
      red[1][rl * tw + cl * 4 + q] = act ? s2[q] : 0.;
    }
  }
  __syncthreads();
  // fold the row lanes: thread j owns column j of the tile (fixed order)
  if (tid < tw) {
    double a = 0., b = 0.;
    for (int r = 0; r < rw; ++r) {
      a += red[0][r * tw + tid];
      b += red[1][r * tw + tid];
    }
    part[((size_t)pt * ntiles + tile) * tw + tid] = make_double2(a, b);
  }
}

// One wave per column: adds the partials in a fixed order.
// mode 0 -> stats and the optional moments block [w, 0, 0, 0 | w d (W) | w (var + d^2) (W)],
// w = weight * |V| (|V| counted here from the lengths), d = mean - shift.
// mode 1 -> dgamma, dbeta (optional) and coef [sum da / |V| | sum da * xhat / |V|] (2W floats).
template <int MODE>
__global__ void seqbn_finalize_kernel(const double2* __restrict__ part,
                                      const float* __restrict__ p, const int* __restrict__ lens,
                                      int T, int N, int W, int ntiles, int tw, int P, float eps,
                                      float* __restrict__ stats, float* __restrict__ moments,
                                      const float* __restrict__ shift, float weight,
                                      float* __restrict__ dgamma, float* __restrict__ dbeta,
                                      float* __restrict__ coef) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const int t = c / tw, s = c % tw;
  double a = 0., b = 0.;
  for (int q = lane; q < P; q += ASR_WAVE) {
    const double2 v = part[((size_t)q * ntiles + t) * tw + s];
    a += v.x;
    b += v.y;
  }
  a = asr_wave_sum_d(a);
  b = asr_wave_sum_d(b);
  if (MODE == 0) {
    double nv = 0.;                 // |V| (integers: exact in any order)
    for (int n = lane; n < N; n += ASR_WAVE) nv += (double)seqbn_len(lens, n, T);
    nv = asr_wave_sum_d(nv);
    if (lane != 0) return;
    const double cnt = nv > 0. ? nv : 1.;
    const double dm = a / cnt;
    const double mean = (double)p[c] + dm;
    double var = b / cnt - dm * dm;
    var = var > 0. ? var : 0.;
    const float mh = (float)mean;
    stats[c] = mh;
    stats[W + c] = (float)(mean - (double)mh);
    stats[2 * W + c] = (float)(1.0 / sqrt(var + (double)eps));
    stats[3 * W + c] = (float)var;
    if (c == 0) {
      stats[4 * W] = (float)nv;
      stats[4 * W + 1] = stats[4 * W + 2] = stats[4 * W + 3] = 0.f;
    }
    if (moments != nullptr) {
      const double w = (double)weight * nv;
      const double d = mean - (double)(shift != nullptr ? shift[c] : mh);
      moments[4 + c] = (float)(w * d);
      moments[4 + W + c] = (float)(w * (var + d * d));
      if (c == 0) {
        moments[0] = (float)w;
        moments[1] = moments[2] = moments[3] = 0.f;
      }
    }
  } else {
    if (lane != 0) return;
    const double nv = (double)stats[4 * W];
    const double cnt = nv > 0. ? nv : 1.;
    dgamma[c] = (float)b;
    if (dbeta != nullptr) dbeta[c] = (float)a;
    coef[c] = (float)(a / cnt);
    coef[W + c] = (float)(b / cnt);
  }
}

// Element-wise passes over all T * n_pad rows.  MODE 0: training apply (stats), 1: inference
// apply (running mean / variance), 2: backward dp (stats + coef; the valid / padded split) and
// max |dp| (bits of a non-negative float: an integer atomicMax, order-independent).
template <int MODE>
__global__ void __launch_bounds__(BN_THREADS)
seqbn_apply_kernel(const float* __restrict__ p, const float* __restrict__ da,
                   const float* __restrict__ gamma, const float* __restrict__ beta,
                   const float* __restrict__ stats, const float* __restrict__ rmean,
                   const float* __restrict__ rvar, const float* __restrict__ coef,
                   const int* __restrict__ lens, float* __restrict__ out,
                   unsigned* __restrict__ absmax, int T, int N, int n_pad, int ld, int W, int cw,
                   int rw, int tw, long long rows, float eps) {
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int cl = tid % cw, rl = tid / cw;
  const int col = tile * tw + cl * 4;
  float mx = 0.f;
  if (rl < rw && col < ld) {
    // the thread's four columns: coefficients (pad columns W <= col < ld: written as zeros)
    float mh[4], ml[4], sc[4], is[4], be[4], cb[4], cc[4];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ok[q] = col + q < W;
      const int c = ok[q] ? col + q : 0;
      be[q] = MODE == 2 ? 0.f : beta[c];
      if (MODE == 1) {
        mh[q] = rmean[c];
        ml[q] = 0.f;
        is[q] = 1.f / sqrtf(rvar[c] + eps);
      } else {
        mh[q] = stats[c];
        ml[q] = stats[W + c];
        is[q] = stats[2 * W + c];
      }
      sc[q] = is[q] * gamma[c];
      if (MODE == 2) {
        cb[q] = coef[c];
        cc[q] = coef[W + c];
      }
    }
    const long long step = (long long)rw * gridDim.y;
    for (long long r = (long long)blockIdx.y * rw + rl; r < rows; r += step) {
      const size_t o = (size_t)r * ld + col;
      const long long t = r / n_pad;
      const int n = (int)(r - t * n_pad);
      float res[4] = {0.f, 0.f, 0.f, 0.f};
      if (n < N) {
        const float4 v = ld4(p + o);
        if (MODE == 2) {
          const float4 g = ld4(da + o);
          const bool valid = t < seqbn_len(lens, n, T);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float xh = ((f4get(v, q) - mh[q]) - ml[q]) * is[q];
            const float d = f4get(g, q);
            const float e = valid ? (d - cb[q]) - xh * cc[q] : d;
            res[q] = ok[q] ? sc[q] * e : 0.f;
            mx = fmaxf(mx, fabsf(res[q]));
          }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float xc = (f4get(v, q) - mh[q]) - ml[q];
            res[q] = ok[q] ? fmaf(xc, sc[q], be[q]) : 0.f;
          }
        }
      }
      st4(out + o, make_float4(res[0], res[1], res[2], res[3]));
    }
  }
  if (MODE == 2 && absmax != nullptr) {
    mx = asr_wave_max(mx);
    if ((tid & (ASR_WAVE - 1)) == 0 && mx > 0.f) atomicMax(absmax, __float_as_uint(mx));
  }
}

}  // namespace

extern "C" size_t asr_bn_workspace_bytes(int T, int N, int n_pad, int ld, int W, int C) {
  BnGeo g;
  if (!bn_geo(T, N, n_pad, ld, W, C, &g)) return 0;
  return bn_partial_bytes(g) + asr_align_up((size_t)2 * C * sizeof(float), 256);
}

#define BN_GEO_OR_FAIL(what)                                                                   \
  BnGeo g;                                                                                     \
  ASR_CHECK_ARG(bn_geo(T, N, n_pad, ld, W, C, &g),                                             \
                what ": bad geometry (T %d N %d n_pad %d ld %d W %d C %d)", T, N, n_pad, ld, W, \
                C);                                                                            \
  ASR_CHECK_ARG(ws_bytes >= asr_bn_workspace_bytes(T, N, n_pad, ld, W, C) && workspace,        \
                what ": workspace too small")

extern "C" int asr_bn_fwd_train(const float* x, float* y, const float* gamma, const float* beta,
                                float* stats, float* moments, const float* shift, float weight,
                                int T, int N, int n_pad, int ld, int W, int C, float eps,
                                float clip, void* workspace, size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(x && y && gamma && beta && stats && eps > 0.f && clip >= 0.f,
                "bn_fwd_train: bad arguments");
  BN_GEO_OR_FAIL("bn_fwd_train");
  hipStream_t s = (hipStream_t)stream;
  double2* part = (double2*)workspace;
  hipLaunchKernelGGL(bn_reduce_kernel<0>, dim3(g.ntiles, g.P), dim3(BN_THREADS), 0, s, x,
                     nullptr, nullptr, nullptr, nullptr, N, n_pad, ld, W, C, g.cw, g.rw, g.tw,
                     g.ntiles, g.slots, g.grouped, g.nreal, g.rpp, 0.f, part);
  ASR_CHECK_LAUNCH();
  const double cnt = (double)g.nreal * (W / C);
  hipLaunchKernelGGL(bn_finalize_kernel<0>, dim3(C), dim3(ASR_WAVE), 0, s, part, x, C,
                     W, g.ntiles, g.tw, g.slots, g.P, g.grouped, cnt, eps, stats, moments, shift,
                     weight, nullptr, nullptr, nullptr);
  ASR_CHECK_LAUNCH();
  const long long rows = (long long)T * n_pad;
  hipLaunchKernelGGL(bn_apply_kernel<0>, dim3(g.ntiles, bn_apply_py(g, rows)), dim3(BN_THREADS),
                     0, s, x, nullptr, gamma, beta, stats, nullptr, nullptr, nullptr, y, N, n_pad,
                     ld, W, C, g.cw, g.rw, g.tw, g.grouped, rows, eps, clip);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_bn_fwd_infer(const float* x, float* y, const float* gamma, const float* beta,
                                const float* running_mean, const float* running_var, int T, int N,
                                int n_pad, int ld, int W, int C, float eps, float clip,
                                asr_stream_t stream) {
  ASR_CHECK_ARG(x && y && gamma && beta && running_mean && running_var && eps > 0.f &&
                    clip >= 0.f,
                "bn_fwd_infer: bad arguments");
  BnGeo g;
  ASR_CHECK_ARG(bn_geo(T, N, n_pad, ld, W, C, &g), "bn_fwd_infer: bad geometry");
  const long long rows = (long long)T * n_pad;
  hipLaunchKernelGGL(bn_apply_kernel<1>, dim3(g.ntiles, bn_apply_py(g, rows)), dim3(BN_THREADS),
                     0, (hipStream_t)stream, x, nullptr, gamma, beta, nullptr, running_mean,
                     running_var, nullptr, y, N, n_pad, ld, W, C, g.cw, g.rw, g.tw, g.grouped,
                     rows, eps, clip);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_bn_bwd(const float* x, const float* dy, const float* gamma, const float* beta,
                          const float* stats, float* dx, float* dgamma, float* dbeta, int T,
                          int N, int n_pad, int ld, int W, int C, float clip, void* workspace,
                          size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(x && dy && gamma && beta && stats && dgamma && dbeta && clip >= 0.f,
                "bn_bwd: bad arguments");
  ASR_CHECK_ARG(dx != dy && dx != x, "bn_bwd: dx must not alias x or dy");
  BN_GEO_OR_FAIL("bn_bwd");
  hipStream_t s = (hipStream_t)stream;
  double2* part = (double2*)workspace;
  float* coef = (float*)((char*)workspace + bn_partial_bytes(g));
  hipLaunchKernelGGL(bn_reduce_kernel<1>, dim3(g.ntiles, g.P), dim3(BN_THREADS), 0, s, x, dy,
                     gamma, beta, stats, N, n_pad, ld, W, C, g.cw, g.rw, g.tw, g.ntiles, g.slots,
                     g.grouped, g.nreal, g.rpp, clip, part);
  ASR_CHECK_LAUNCH();
  const double cnt = (double)g.nreal * (W / C);
  hipLaunchKernelGGL(bn_finalize_kernel<1>, dim3(C), dim3(ASR_WAVE), 0, s, part, x, C,
                     W, g.ntiles, g.tw, g.slots, g.P, g.grouped, cnt, 0.f, nullptr, nullptr,
                     nullptr, 0.f, dgamma, dbeta, coef);
  ASR_CHECK_LAUNCH();
  if (dx == nullptr) return ASR_OK;
  const long long rows = (long long)T * n_pad;
  hipLaunchKernelGGL(bn_apply_kernel<2>, dim3(g.ntiles, bn_apply_py(g, rows)), dim3(BN_THREADS),
                     0, s, x, dy, gamma, beta, stats, nullptr, nullptr, coef, dx, N, n_pad, ld,
                     W, C, g.cw, g.rw, g.tw, g.grouped, rows, 0.f, clip);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_bn_update_running(float* running_mean, float* running_var,
                                     const float* moments, const float* shift, int C,
                                     float momentum, const int* flag_a, const int* flag_b,
                                     const int* flag_c, const int* flag_d, asr_stream_t stream) {
  ASR_CHECK_ARG(running_mean && running_var && moments && C > 0 && momentum >= 0.f &&
                    momentum <= 1.f,
                "bn_update_running: bad arguments");
  hipLaunchKernelGGL(bn_update_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     running_mean, running_var, moments, shift, C, momentum, flag_a, flag_b,
                     flag_c, flag_d);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

// ------------------------------------------------------------------------------- K18 entry points
extern "C" size_t asr_seqbn_workspace_bytes(int T, int N, int n_pad, int ld, int W) {
  BnGeo g;
  if (!bn_geo(T, N, n_pad, ld, W, W, &g)) return 0;
  return bn_partial_bytes(g) + asr_align_up((size_t)2 * W * sizeof(float), 256);
}

#define SEQBN_GEO_OR_FAIL(what)                                                                \
  BnGeo g;                                                                                     \
  ASR_CHECK_ARG(bn_geo(T, N, n_pad, ld, W, W, &g),                                             \
                what ": bad geometry (T %d N %d n_pad %d ld %d W %d)", T, N, n_pad, ld, W);    \
  ASR_CHECK_ARG(ws_bytes >= asr_seqbn_workspace_bytes(T, N, n_pad, ld, W) && workspace,        \
                what ": workspace too small")

extern "C" int asr_seqbn_fwd_train(const float* p, float* y, const float* gamma,
                                   const float* beta, const int* lens, float* stats,
                                   float* moments, const float* shift, float weight, int T, int N,
                                   int n_pad, int ld, int W, float eps, void* workspace,
                                   size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(p && y && gamma && beta && stats && eps > 0.f && weight >= 0.f,
                "seqbn_fwd_train: bad arguments");
  SEQBN_GEO_OR_FAIL("seqbn_fwd_train");
  hipStream_t s = (hipStream_t)stream;
  double2* part = (double2*)workspace;
  hipLaunchKernelGGL(seqbn_reduce_kernel<0>, dim3(g.ntiles, g.P), dim3(BN_THREADS), 0, s, p,
                     nullptr, nullptr, lens, T, N, n_pad, ld, W, g.cw, g.rw, g.tw, g.ntiles,
                     g.nreal, g.rpp, part);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(seqbn_finalize_kernel<0>, dim3(W), dim3(ASR_WAVE), 0, s, part, p, lens, T,
                     N, W, g.ntiles, g.tw, g.P, eps, stats, moments, shift, weight, nullptr,
                     nullptr, nullptr);
  ASR_CHECK_LAUNCH();
  const long long rows = (long long)T * n_pad;
  hipLaunchKernelGGL(seqbn_apply_kernel<0>, dim3(g.ntiles, bn_apply_py(g, rows)),
                     dim3(BN_THREADS), 0, s, p, nullptr, gamma, beta, stats, nullptr, nullptr,
                     nullptr, nullptr, y, nullptr, T, N, n_pad, ld, W, g.cw, g.rw, g.tw, rows,
                     eps);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_seqbn_fwd_infer(const float* p, float* y, const float* gamma,
                                   const float* beta, const float* running_mean,
                                   const float* running_var, int T, int N, int n_pad, int ld,
                                   int W, float eps, asr_stream_t stream) {
  ASR_CHECK_ARG(p && y && gamma && beta && running_mean && running_var && eps > 0.f,
                "seqbn_fwd_infer: bad arguments");
  BnGeo g;
  ASR_CHECK_ARG(bn_geo(T, N, n_pad, ld, W, W, &g), "seqbn_fwd_infer: bad geometry");
  const long long rows = (long long)T * n_pad;
  hipLaunchKernelGGL(seqbn_apply_kernel<1>, dim3(g.ntiles, bn_apply_py(g, rows)),
                     dim3(BN_THREADS), 0, (hipStream_t)stream, p, nullptr, gamma, beta, nullptr,
                     running_mean, running_var, nullptr, nullptr, y, nullptr, T, N, n_pad, ld, W,
                     g.cw, g.rw, g.tw, rows, eps);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_seqbn_bwd(const float* p, const float* da, const float* gamma,
                             const int* lens, const float* stats, float* dp, float* dgamma,
                             float* dbeta, float* dp_absmax, int T, int N, int n_pad, int ld,
                             int W, void* workspace, size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(p && da && gamma && stats && dp && dgamma, "seqbn_bwd: bad arguments");
  ASR_CHECK_ARG(dp != da && dp != p, "seqbn_bwd: dp must not alias p or da");
  SEQBN_GEO_OR_FAIL("seqbn_bwd");
  hipStream_t s = (hipStream_t)stream;
  double2* part = (double2*)workspace;
  float* coef = (float*)((char*)workspace + bn_partial_bytes(g));
  hipLaunchKernelGGL(seqbn_reduce_kernel<1>, dim3(g.ntiles, g.P), dim3(BN_THREADS), 0, s, p, da,
                     stats, nullptr, T, N, n_pad, ld, W, g.cw, g.rw, g.tw, g.ntiles, g.nreal,
                     g.rpp, part);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(seqbn_finalize_kernel<1>, dim3(W), dim3(ASR_WAVE), 0, s, part, p, nullptr,
                     T, N, W, g.ntiles, g.tw, g.P, 0.f, const_cast<float*>(stats), nullptr,
                     nullptr, 0.f, dgamma, dbeta, coef);
  ASR_CHECK_LAUNCH();
  if (dp_absmax) ASR_CHECK_HIP(hipMemsetAsync(dp_absmax, 0, sizeof(float), s));
  const long long rows = (long long)T * n_pad;
  hipLaunchKernelGGL(seqbn_apply_kernel<2>, dim3(g.ntiles, bn_apply_py(g, rows)),
                     dim3(BN_THREADS), 0, s, p, da, gamma, nullptr, stats, nullptr, nullptr, coef,
                     lens, dp, reinterpret_cast<unsigned*>(dp_absmax), T, N, n_pad, ld, W, g.cw,
                     g.rw, g.tw, rows, 0.f);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
