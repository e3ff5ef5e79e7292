// K15 BatchNormalization (Keras 1.2.2, mode 0, axis -1) over a time-major slab (T, n_pad, ld), and
// K18, the sequence-wise BatchNormalization of a recurrent layer's input projection: one kernel
// family (reduce, finalize, apply) behind both sets of entry points.
//
// Training: y = gamma * (x - mu) * invstd + beta, mu / var the biased moments of every real row
// (n < N of each frame, all T frames) per channel; channel = column % C (C == W: a plain 2-D
// tensor; C < W: the (N, T, F, C) conv image, W = F * C).  Inference: the same map with the
// running moments.  Backward: dbeta = sum dy, dgamma = sum dy * xhat, dx = gamma * invstd *
// (dy - mean(dy) - xhat * mean(dy * xhat)).  An optional clip fuses a following clipped ReLU
// (forward min(max(y, 0), clip); backward masks dy with 0 < y < clip, y recomputed from x).
//
// What a caller may turn on, each on its own:
//   channel grouping  C < W, the conv image (K15 only asks for it);
//   clip              the fused clipped ReLU (K15 only asks for it);
//   lengths           the statistics are taken over the VALID rows only (n < N, t < min(len_n, T));
//                     every real row is still normalised with them, so time-padding frames
//                     contribute nothing to mu / var but get a value.  Backward: dx = gamma *
//                     invstd * (dy - [valid] (dbeta / |V| + xhat * dgamma / |V|)), the sums over
//                     all real rows.  lens == NULL: every frame is valid;
//   counted rows      |V| is counted on the device from the lengths and kept behind the
//                     statistics: stats (4C + 4 floats) = [mean_hi | mean_lo | invstd | var |
//                     |V|, 0, 0, 0]; the moments are weighted by weight * |V|.  Without it the
//                     count comes from the host and stats has 4C floats;
//   max |dx|          of the backward pass (bits of a non-negative float: an integer atomicMax,
//                     order-independent).
// K18 is lengths + counted rows + max |dp| on an ungrouped slab (C == W) without clip.
//
// Every pass walks the slab with one 16-byte column group per thread: a workgroup is rw row
// lanes x cw column lanes (cw float4 groups = a tile of 4 * cw columns), so a thread's channel
// coefficients are loaded once.  Reductions: each thread sums its rows in fp64 (statistics
// shifted by the row-0 value of the channel), the workgroup folds its row lanes -- and, for the
// conv image, the columns of one channel -- in LDS in a fixed order, writes one partial per
// (partition, tile, slot), and a finalize kernel adds the partials in a fixed order.  No float
// atomics: two identical calls give identical bits.  Padding rows (n >= N) and padding columns
// (W <= col < ld) of y and dx are written as zeros.
#include "vec4.h"

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

// valid frames of sample n: len_n clamped to 0 .. T; all T without lengths
__device__ __forceinline__ int bn_len(const int* __restrict__ lens, int n, int T) {
  if (lens == nullptr) return T;
  const int l = lens[n];
  return l < 0 ? 0 : (l > T ? T : l);
}

// Sums of one thread's column group over its rows, folded over the workgroup's row lanes (and
// over the channel's columns for the conv image), written as one partial per slot.
// mode 0: statistics (x - shift, (x - shift)^2), shift = row (0, 0) of the column; LENS: over the
// valid rows only (a compile-time policy: without it the inner loop has no length load);
// mode 1: backward (dy', dy' * xhat) over all real rows.
template <int MODE, bool LENS>
__global__ void __launch_bounds__(BN_THREADS)
bn_reduce_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                 const float* __restrict__ gamma, const float* __restrict__ beta,
                 const float* __restrict__ stats, const int* __restrict__ lens, int T, int N,
                 int n_pad, int ld, int W, int C, int cw, int rw, int tw, int ntiles, int slots,
                 int grouped, long long nreal, long long rpp, float clip,
                 double2* __restrict__ part) {
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
        if (LENS && t >= bn_len(lens, (int)n, T)) continue;   // (skipped before its load)
        const float4 v = ld4(x + (size_t)(t * n_pad + n) * ld + col);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double d = (double)f4get(v, q) - (double)f4get(k, q);
          s1[q] += d;
          s2[q] = fma(d, d, s2[q]);
        }
      }
    } else {
      // (scalar loads: C need not be a multiple of 4, pad columns have no coefficients;
      // gamma / beta are needed for the clip mask alone and may be NULL without it)
      float mh[4], ml[4], is[4], ga[4], be[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = col + q < W ? ch + q : 0;
        mh[q] = stats[c];
        ml[q] = stats[C + c];
        is[q] = stats[2 * C + c];
        ga[q] = clip > 0.f ? gamma[c] : 0.f;
        be[q] = clip > 0.f ? beta[c] : 0.f;
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
// mode 1 -> dgamma, dbeta (optional) and coef [sum dy' / cnt | sum dy' * xhat / cnt] (2C floats).
// COUNTED: cnt is not the host's but max(|V|, 1), |V| counted here from the lengths in mode 0,
// kept in stats[4C .. 4C + 3] and read back from there in mode 1; w = weight * |V|.
template <int MODE, bool COUNTED>
__global__ void bn_finalize_kernel(const double2* __restrict__ part, const float* __restrict__ x,
                                   const int* __restrict__ lens, int T, int N, int C, int W,
                                   int ntiles, int tw, int slots, int P, int grouped, double cnt,
                                   float eps, float* __restrict__ stats,
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
  double nv = 1.;
  if (COUNTED && MODE == 0) {
    // |V| of a channel: the valid rows times its W / C columns (integers: exact in any order);
    // all 64 lanes take part in the wave sum, so it stands before the lanes past 0 leave
    nv = 0.;
    for (int n = lane; n < N; n += ASR_WAVE) nv += (double)bn_len(lens, n, T);
    nv = asr_wave_sum_d(nv) * (double)(W / C);
  }
  if (lane != 0) return;
  if (COUNTED) {
    if (MODE == 1) nv = (double)stats[4 * C];
    cnt = nv > 0. ? nv : 1.;
  }
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
    if (COUNTED && c == 0) {
      stats[4 * C] = (float)nv;
      stats[4 * C + 1] = stats[4 * C + 2] = stats[4 * C + 3] = 0.f;
    }
    if (moments != nullptr) {
      const double w = (double)weight * nv;   // (nv = 1 where the rows are not counted: exact)
      const double d = mean - (double)(shift != nullptr ? shift[c] : mh);
      moments[4 + c] = (float)(w * d);
      moments[4 + C + c] = (float)(w * (var + d * d));
      if (c == 0) {
        moments[0] = (float)w;
        moments[1] = moments[2] = moments[3] = 0.f;
      }
    }
  } else {
    dgamma[c] = (float)b;
    if (dbeta != nullptr) dbeta[c] = (float)a;
    coef[c] = (float)(a / cnt);
    coef[C + c] = (float)(b / cnt);
  }
}

// Element-wise passes over all T * n_pad rows.  MODE 0: training apply (stats), 1: inference
// apply (running mean / variance), 2: backward dx (stats + coef); of the backward pass, LENS:
// the valid / padded split of the lengths, ABSMAX: max |dx|.
template <int MODE, bool LENS, bool ABSMAX>
__global__ void __launch_bounds__(BN_THREADS)
bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                const float* __restrict__ gamma, const float* __restrict__ beta,
                const float* __restrict__ stats, const float* __restrict__ rmean,
                const float* __restrict__ rvar, const float* __restrict__ coef,
                const int* __restrict__ lens, float* __restrict__ out,
                unsigned* __restrict__ absmax, int T, int N, int n_pad, int ld, int W, int C,
                int cw, int rw, int tw, int grouped, long long rows, float eps, float clip) {
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int cl = tid % cw, rl = tid / cw;
  const int col = tile * tw + cl * 4;
  float mx = 0.f;
  // (idle threads skip the walk, not the kernel: the wave maximum below needs every lane)
  if (rl < rw && col < ld) {
    const int ch = grouped ? col % C : col;
    // the thread's four columns: coefficients (pad columns W <= col < ld: written as zeros);
    // the backward pass needs beta for the clip mask alone, and it may be NULL without it
    float mh[4], ml[4], is[4], sc[4], be[4], cb[4], cc[4];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ok[q] = col + q < W;
      const int c = ok[q] ? ch + q : 0;
      be[q] = (MODE == 2 && !(clip > 0.f)) ? 0.f : beta[c];
      if (MODE == 1) {
        mh[q] = rmean[c];
        ml[q] = 0.f;
        is[q] = 1.f / sqrtf(rvar[c] + eps);
      } else {
        mh[q] = stats[c];
        ml[q] = stats[C + c];
        is[q] = stats[2 * C + c];
      }
      sc[q] = is[q] * gamma[c];
      if (MODE == 2) {
        cb[q] = coef[c];
        cc[q] = coef[C + c];
      }
    }
    const long long step = (long long)rw * gridDim.y;
    for (long long r = (long long)blockIdx.y * rw + rl; r < rows; r += step) {
      const size_t o = (size_t)r * ld + col;
      const long long t = r / n_pad;
      const int n = (int)(r - t * n_pad);
      float res[4] = {0.f, 0.f, 0.f, 0.f};
      if (n < N) {
        const float4 v = ld4(x + o);
        if (MODE == 2) {
          const float4 g = ld4(dy + o);
          const bool valid = !LENS || t < bn_len(lens, n, T);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float xc = (f4get(v, q) - mh[q]) - ml[q];
            const float xh = xc * is[q];
            float d = f4get(g, q);
            if (clip > 0.f) {
              const float z = fmaf(xc, sc[q], be[q]);
              d = (z > 0.f && z < clip) ? d : 0.f;
            }
            const float e = valid ? (d - cb[q]) - xh * cc[q] : d;
            res[q] = ok[q] ? sc[q] * e : 0.f;
            if (ABSMAX) mx = fmaxf(mx, fabsf(res[q]));
          }
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float xc = (f4get(v, q) - mh[q]) - ml[q];
            const float z = fmaf(xc, sc[q], be[q]);
            const float y = clip > 0.f ? fminf(fmaxf(z, 0.f), clip) : z;
            res[q] = ok[q] ? y : 0.f;
          }
        }
      }
      st4(out + o, make_float4(res[0], res[1], res[2], res[3]));
    }
  }
  if (ABSMAX) {
    mx = asr_wave_max(mx);
    if ((tid & (ASR_WAVE - 1)) == 0 && mx > 0.f) atomicMax(absmax, __float_as_uint(mx));
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

// The three launch sequences behind the entry points (arguments checked by the caller).
// COUNTED as in bn_finalize_kernel; lens == NULL takes the instantiations without a length load.
template <bool COUNTED>
int bn_launch_fwd_train(const float* x, float* y, const float* gamma, const float* beta,
                        const int* lens, float* stats, float* moments, const float* shift,
                        float weight, int T, int N, int n_pad, int ld, int W, int C, float eps,
                        float clip, const BnGeo& g, void* workspace, hipStream_t s) {
  double2* part = (double2*)workspace;
  const auto reduce = lens ? bn_reduce_kernel<0, true> : bn_reduce_kernel<0, false>;
  hipLaunchKernelGGL(reduce, dim3(g.ntiles, g.P), dim3(BN_THREADS), 0, s, x, nullptr, nullptr,
                     nullptr, nullptr, lens, T, N, n_pad, ld, W, C, g.cw, g.rw, g.tw, g.ntiles,
                     g.slots, g.grouped, g.nreal, g.rpp, 0.f, part);
  ASR_CHECK_LAUNCH();
  const double cnt = (double)g.nreal * (W / C);
  hipLaunchKernelGGL((bn_finalize_kernel<0, COUNTED>), dim3(C), dim3(ASR_WAVE), 0, s, part, x,
                     lens, T, N, C, W, g.ntiles, g.tw, g.slots, g.P, g.grouped, cnt, eps, stats,
                     moments, shift, weight, nullptr, nullptr, nullptr);
  ASR_CHECK_LAUNCH();
  const long long rows = (long long)T * n_pad;
  hipLaunchKernelGGL((bn_apply_kernel<0, false, false>), dim3(g.ntiles, bn_apply_py(g, rows)),
                     dim3(BN_THREADS), 0, s, x, nullptr, gamma, beta, stats, nullptr, nullptr,
                     nullptr, nullptr, y, nullptr, T, N, n_pad, ld, W, C, g.cw, g.rw, g.tw,
                     g.grouped, rows, eps, clip);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

int bn_launch_fwd_infer(const float* x, float* y, const float* gamma, const float* beta,
                        const float* running_mean, const float* running_var, int T, int N,
                        int n_pad, int ld, int W, int C, float eps, float clip, const BnGeo& g,
                        hipStream_t s) {
  const long long rows = (long long)T * n_pad;
  hipLaunchKernelGGL((bn_apply_kernel<1, false, false>), dim3(g.ntiles, bn_apply_py(g, rows)),
                     dim3(BN_THREADS), 0, s, x, nullptr, gamma, beta, nullptr, running_mean,
                     running_var, nullptr, nullptr, y, nullptr, T, N, n_pad, ld, W, C, g.cw, g.rw,
                     g.tw, g.grouped, rows, eps, clip);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

// beta may be NULL where clip == 0; dbeta, dx and dx_absmax where they are not wanted
template <bool COUNTED>
int bn_launch_bwd(const float* x, const float* dy, const float* gamma, const float* beta,
                  const int* lens, const float* stats, float* dx, float* dgamma, float* dbeta,
                  float* dx_absmax, int T, int N, int n_pad, int ld, int W, int C, float clip,
                  const BnGeo& g, void* workspace, hipStream_t s) {
  double2* part = (double2*)workspace;
  float* coef = (float*)((char*)workspace + bn_partial_bytes(g));
  hipLaunchKernelGGL((bn_reduce_kernel<1, false>), dim3(g.ntiles, g.P), dim3(BN_THREADS), 0, s, x,
                     dy, gamma, beta, stats, nullptr, T, N, n_pad, ld, W, C, g.cw, g.rw, g.tw,
                     g.ntiles, g.slots, g.grouped, g.nreal, g.rpp, clip, part);
  ASR_CHECK_LAUNCH();
  const double cnt = (double)g.nreal * (W / C);
  hipLaunchKernelGGL((bn_finalize_kernel<1, COUNTED>), dim3(C), dim3(ASR_WAVE), 0, s, part, x,
                     nullptr, T, N, C, W, g.ntiles, g.tw, g.slots, g.P, g.grouped, cnt, 0.f,
                     const_cast<float*>(stats), nullptr, nullptr, 0.f, dgamma, dbeta, coef);
  ASR_CHECK_LAUNCH();
  if (dx == nullptr) return ASR_OK;
  if (dx_absmax) ASR_CHECK_HIP(hipMemsetAsync(dx_absmax, 0, sizeof(float), s));
  const auto apply =
      lens ? (dx_absmax ? bn_apply_kernel<2, true, true> : bn_apply_kernel<2, true, false>)
           : (dx_absmax ? bn_apply_kernel<2, false, true> : bn_apply_kernel<2, false, false>);
  const long long rows = (long long)T * n_pad;
  hipLaunchKernelGGL(apply, dim3(g.ntiles, bn_apply_py(g, rows)), dim3(BN_THREADS), 0, s, x, dy,
                     gamma, beta, stats, nullptr, nullptr, coef, lens, dx,
                     reinterpret_cast<unsigned*>(dx_absmax), T, N, n_pad, ld, W, C, g.cw, g.rw,
                     g.tw, g.grouped, rows, 0.f, clip);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
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
  return bn_launch_fwd_train<false>(x, y, gamma, beta, nullptr, stats, moments, shift, weight, T,
                                    N, n_pad, ld, W, C, eps, clip, g, workspace,
                                    (hipStream_t)stream);
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
  return bn_launch_fwd_infer(x, y, gamma, beta, running_mean, running_var, T, N, n_pad, ld, W, C,
                             eps, clip, g, (hipStream_t)stream);
}

extern "C" int asr_bn_bwd(const float* x, const float* dy, const float* gamma, const float* beta,
                          const float* stats, float* dx, float* dgamma, float* dbeta, int T,
                          int N, int n_pad, int ld, int W, int C, float clip, void* workspace,
                          size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(x && dy && gamma && beta && stats && dgamma && dbeta && clip >= 0.f,
                "bn_bwd: bad arguments");
  ASR_CHECK_ARG(dx != dy && dx != x, "bn_bwd: dx must not alias x or dy");
  BN_GEO_OR_FAIL("bn_bwd");
  return bn_launch_bwd<false>(x, dy, gamma, beta, nullptr, stats, dx, dgamma, dbeta, nullptr, T,
                              N, n_pad, ld, W, C, clip, g, workspace, (hipStream_t)stream);
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
// p (T, n_pad, ld) with W real columns, one channel per column (cell-agnostic: only the slab
// width is known here): lengths, counted rows, no grouping, no clip.
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
  return bn_launch_fwd_train<true>(p, y, gamma, beta, lens, stats, moments, shift, weight, T, N,
                                   n_pad, ld, W, W, eps, 0.f, g, workspace, (hipStream_t)stream);
}

extern "C" int asr_seqbn_fwd_infer(const float* p, float* y, const float* gamma,
                                   const float* beta, const float* running_mean,
                                   const float* running_var, int T, int N, int n_pad, int ld,
                                   int W, float eps, asr_stream_t stream) {
  ASR_CHECK_ARG(p && y && gamma && beta && running_mean && running_var && eps > 0.f,
                "seqbn_fwd_infer: bad arguments");
  BnGeo g;
  ASR_CHECK_ARG(bn_geo(T, N, n_pad, ld, W, W, &g), "seqbn_fwd_infer: bad geometry");
  return bn_launch_fwd_infer(p, y, gamma, beta, running_mean, running_var, T, N, n_pad, ld, W, W,
                             eps, 0.f, g, (hipStream_t)stream);
}

extern "C" int asr_seqbn_bwd(const float* p, const float* da, const float* gamma,
                             const int* lens, const float* stats, float* dp, float* dgamma,
                             float* dbeta, float* dp_absmax, int T, int N, int n_pad, int ld,
                             int W, void* workspace, size_t ws_bytes, asr_stream_t stream) {
  ASR_CHECK_ARG(p && da && gamma && stats && dp && dgamma, "seqbn_bwd: bad arguments");
  ASR_CHECK_ARG(dp != da && dp != p, "seqbn_bwd: dp must not alias p or da");
  SEQBN_GEO_OR_FAIL("seqbn_bwd");
  return bn_launch_bwd<true>(p, da, gamma, nullptr, lens, stats, dp, dgamma, dbeta, dp_absmax, T,
                             N, n_pad, ld, W, W, 0.f, g, workspace, (hipStream_t)stream);
}
