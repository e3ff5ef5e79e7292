// K20 LayerNormalization over the feature axis of a time-major slab (T, n_pad, ld).
//
// For every real row (n < N of each frame): y = (x - mu) * r * gain + bias with mu and the biased
// variance taken over the row's REAL columns, r = 1 / sqrt(var + eps).  The real columns are
// `segs` blocks of H columns at a stride of Hp (Hp a multiple of 4, segs * Hp <= ld): one block
// for a Dense / conv / summed output, two behind a concatenating recurrent layer whose
// directions are padded apart.  Pad columns may hold anything: they are never read into a sum,
// and y / dx are written as zeros there and in the padding rows n >= N.
// Backward: xhat = (x - mu) r, g = gain dy, dx = r (g - mean(g) - xhat mean(g xhat)), dgain =
// sum_rows dy xhat, dbias = sum_rows dy.
//
// Geometry: a row is held by LPR lanes of one wave (4, 16 or 64; 64 / LPR rows per wave), each
// lane keeps VPL 16-byte column groups in registers (VPL > 1 only with LPR = 64: up to 16, i.e.
// 4096 columns).  The row is loaded ONCE: the mean, the centred sum of squares and the output
// all come from the resident registers (sum (x - mu)^2, never E[x^2] - mu^2; the mean itself is
// refined by the mean of the first residuals, so a large offset costs one rounding of mu and no
// more).  Row reductions are xor butterflies over the LPR lanes (every lane ends with the same
// bits).  Waves walk the rows grid-stride.  The backward pass keeps per-lane column sums of
// dy xhat and dy over the wave's rows, folds the row groups of a wave by shuffles and the waves
// of a workgroup through LDS one after the other, writes one partial per workgroup, and a
// finishing kernel adds the partials in a fixed order.  No float atomics anywhere: two
// identical calls give identical bits.
#include "vec4.h"

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_WAVES = LN_THREADS / ASR_WAVE;
constexpr int LN_MAX_LD = 4096;           // 64 lanes x 16 groups x 4 columns
constexpr int LN_FWD_BLOCKS = 2048;
constexpr int LN_BWD_BLOCKS = 512;        // = partials of dgain / dbias
constexpr int LN_FIN_COLS = 16;           // finishing kernel: 16 columns x 64 slices of partials

struct LnGeo {
  int lpr, vpl;
  long long rows, groups;   // T * n_pad; row groups of 4 waves each (workgroups needed)
};

bool ln_geo(int T, int N, int n_pad, int ld, int H, int Hp, int segs, LnGeo* g) {
  if (T < 1 || N < 1 || n_pad < N || ld < 4 || (ld & 3) || ld > LN_MAX_LD) return false;
  if (H < 1 || Hp < H || (Hp & 3) || segs < 1 || (long long)segs * Hp > ld) return false;
  const int nvec = ld / 4;
  g->lpr = nvec <= 4 ? 4 : (nvec <= 16 ? 16 : 64);
  g->vpl = 1;
  while (g->vpl * 64 < nvec) g->vpl *= 2;
  g->rows = (long long)T * n_pad;
  const int rpb = LN_WAVES * (ASR_WAVE / g->lpr);
  g->groups = (g->rows + rpb - 1) / rpb;
  return true;
}

int ln_blocks(const LnGeo& g, int cap) { return (int)(g.groups < cap ? g.groups : cap); }

size_t ln_partial_bytes(const LnGeo& g, int ld) {
  return asr_align_up((size_t)ln_blocks(g, LN_BWD_BLOCKS) * 2 * ld * sizeof(float), 256);
}

template <int LPR>
__device__ __forceinline__ float ln_row_sum(float v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, ASR_WAVE);
  return v;
}

// Leading real columns (0..4) of the lane's column group v, -1 for a group past the row's end.
// A group never straddles two blocks (Hp % 4 == 0) and a block's real columns are its first H.
template <int LPR, int VPL>
__device__ __forceinline__ void ln_columns(int sub, int ld, int H, int Hp, int segs, int (&nr)[VPL]) {
#pragma unroll
  for (int v = 0; v < VPL; ++v) {
    const int c = (v * LPR + sub) * 4;
    if (c >= ld) { nr[v] = -1; continue; }
    const int seg = c / Hp;
    const int k = seg < segs ? H - (c - seg * Hp) : 0;
    nr[v] = k < 0 ? 0 : (k > 4 ? 4 : k);
  }
}

template <int LPR, int VPL>
__global__ void __launch_bounds__(LN_THREADS)
ln_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ gain,
              const float* __restrict__ bias, float* __restrict__ stats, long long rows, int N,
              int n_pad, int ld, int H, int Hp, int segs, float inv_cnt, float eps) {
  constexpr int RPW = ASR_WAVE / LPR;
  const int lane = threadIdx.x & (ASR_WAVE - 1), wave = threadIdx.x / ASR_WAVE;
  const int sub = lane % LPR, grp = lane / LPR;
  int nr[VPL];
  ln_columns<LPR, VPL>(sub, ld, H, Hp, segs, nr);
  const long long stride = (long long)gridDim.x * LN_WAVES * RPW;
  for (long long r0 = ((long long)blockIdx.x * LN_WAVES + wave) * RPW; r0 < rows; r0 += stride) {
    const long long r = r0 + grp;
    const bool live = r < rows;
    const bool real = live && (int)(r % n_pad) < N;
    const size_t base = (size_t)(live ? r : 0) * ld;
    float xv[VPL][4];
    float s = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (real && nr[v] > 0) t = ld4(x + base + (size_t)(v * LPR + sub) * 4);
      xv[v][0] = t.x; xv[v][1] = t.y; xv[v][2] = t.z; xv[v][3] = t.w;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q >= nr[v]) xv[v][q] = 0.f;
        s += xv[v][q];
      }
    }
    const float m0 = ln_row_sum<LPR>(s) * inv_cnt;
    s = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xv[v][q] = q < nr[v] ? xv[v][q] - m0 : 0.f;
        s += xv[v][q];
      }
    const float m1 = ln_row_sum<LPR>(s) * inv_cnt;      // (what rounding left of the mean)
    s = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xv[v][q] = q < nr[v] ? xv[v][q] - m1 : 0.f;
        s = fmaf(xv[v][q], xv[v][q], s);
      }
    const float rs = 1.f / sqrtf(ln_row_sum<LPR>(s) * inv_cnt + eps);
    if (real && sub == 0 && stats != nullptr)
      *reinterpret_cast<float2*>(stats + 2 * (size_t)r) = make_float2(m0 + m1, rs);
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      if (!live || nr[v] < 0) continue;
      const size_t c = (size_t)(v * LPR + sub) * 4;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
      if (real && nr[v] > 0) {
        const float4 g = ld4(gain + c), b = ld4(bias + c);
        const float gg[4] = {g.x, g.y, g.z, g.w}, bb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < nr[v]) o[q] = fmaf(xv[v][q] * rs, gg[q], bb[q]);
      }
      st4(y + base + c, make_float4(o[0], o[1], o[2], o[3]));
    }
  }
}

template <int LPR, int VPL>
__global__ void __launch_bounds__(LN_THREADS)
ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
              const float* __restrict__ gain, const float* __restrict__ stats,
              float* __restrict__ dx, float* __restrict__ part, long long rows, int N, int n_pad,
              int ld, int H, int Hp, int segs, float inv_cnt) {
  constexpr int RPW = ASR_WAVE / LPR;
  extern __shared__ float ln_sm[];          // dgain (ld) | dbias (ld) of the workgroup
  const int lane = threadIdx.x & (ASR_WAVE - 1), wave = threadIdx.x / ASR_WAVE;
  const int sub = lane % LPR, grp = lane / LPR;
  int nr[VPL];
  ln_columns<LPR, VPL>(sub, ld, H, Hp, segs, nr);
  float ag[VPL][4], ab[VPL][4];
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int q = 0; q < 4; ++q) ag[v][q] = ab[v][q] = 0.f;
  const long long stride = (long long)gridDim.x * LN_WAVES * RPW;
  for (long long r0 = ((long long)blockIdx.x * LN_WAVES + wave) * RPW; r0 < rows; r0 += stride) {
    const long long r = r0 + grp;
    const bool live = r < rows;
    const bool real = live && (int)(r % n_pad) < N;
    const size_t base = (size_t)(live ? r : 0) * ld;
    float2 st = make_float2(0.f, 0.f);
    if (real) st = *reinterpret_cast<const float2*>(stats + 2 * (size_t)r);
    float xh[VPL][4], gd[VPL][4];           // xhat and gain * dy (zeros off the real columns)
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), d = a, g = a;
      if (real && nr[v] > 0) {
        const size_t c = (size_t)(v * LPR + sub) * 4;
        a = ld4(x + base + c);
        d = ld4(dy + base + c);
        g = ld4(gain + c);
      }
      const float aa[4] = {a.x, a.y, a.z, a.w}, dd[4] = {d.x, d.y, d.z, d.w},
                  gg[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool on = real && q < nr[v];
        xh[v][q] = on ? (aa[q] - st.x) * st.y : 0.f;
        const float dq = on ? dd[q] : 0.f;
        gd[v][q] = on ? gg[q] * dq : 0.f;
        ag[v][q] = fmaf(dq, xh[v][q], ag[v][q]);
        ab[v][q] += dq;
        s1 += gd[v][q];
        s2 = fmaf(gd[v][q], xh[v][q], s2);
      }
    }
    if (dx == nullptr) continue;            // (uniform: no input gradient wanted)
    const float m1 = ln_row_sum<LPR>(s1) * inv_cnt, m2 = ln_row_sum<LPR>(s2) * inv_cnt;
#pragma unroll
    for (int v = 0; v < VPL; ++v) {
      if (!live || nr[v] < 0) continue;
      float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (real && q < nr[v]) o[q] = st.y * ((gd[v][q] - m1) - xh[v][q] * m2);
      st4(dx + base + (size_t)(v * LPR + sub) * 4, make_float4(o[0], o[1], o[2], o[3]));
    }
  }
  // the row groups of the wave (lanes that hold the same columns), then the waves one by one
#pragma unroll
  for (int v = 0; v < VPL; ++v)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int o = LPR; o < ASR_WAVE; o <<= 1) {
        ag[v][q] += __shfl_xor(ag[v][q], o, ASR_WAVE);
        ab[v][q] += __shfl_xor(ab[v][q], o, ASR_WAVE);
      }
  for (int w = 0; w < LN_WAVES; ++w) {
    if (wave == w && grp == 0) {
#pragma unroll
      for (int v = 0; v < VPL; ++v) {
        if (nr[v] < 0) continue;
        const int c = (v * LPR + sub) * 4;
        float4 a = make_float4(ag[v][0], ag[v][1], ag[v][2], ag[v][3]);
        float4 b = make_float4(ab[v][0], ab[v][1], ab[v][2], ab[v][3]);
        if (w > 0) {
          const float4 pa = ld4(ln_sm + c), pb = ld4(ln_sm + ld + c);
          a = make_float4(pa.x + a.x, pa.y + a.y, pa.z + a.z, pa.w + a.w);
          b = make_float4(pb.x + b.x, pb.y + b.y, pb.z + b.z, pb.w + b.w);
        }
        st4(ln_sm + c, a);
        st4(ln_sm + ld + c, b);
      }
    }
    __syncthreads();
  }
  float* out = part + (size_t)blockIdx.x * 2 * ld;
  for (int i = threadIdx.x; i < 2 * ld; i += LN_THREADS) out[i] = ln_sm[i];
}

// dgain[c] = sum_p part[p][0][c], dbias[c] = sum_p part[p][1][c].  A workgroup owns 16 columns:
// 4 lanes of 16-byte groups x 64 slices of the partials (slice s adds p = s, s + 64, ... in
// order, its loads independent of each other), the slices are then added in order out of LDS.
__global__ void __launch_bounds__(LN_THREADS)
ln_finish_kernel(const float* __restrict__ part, int P, int ld, float* __restrict__ dgain,
                 float* __restrict__ dbias) {
  constexpr int CG = LN_FIN_COLS / 4, SL = LN_THREADS / CG;
  __shared__ __align__(16) float red[2][SL][LN_FIN_COLS];
  const int cg = threadIdx.x % CG, sl = threadIdx.x / CG;
  const int col = blockIdx.x * LN_FIN_COLS + cg * 4;        // (ld % 4 == 0: a group is whole)
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (col < ld) {
#pragma unroll 4
    for (int p = sl; p < P; p += SL) {
      const float* q = part + (size_t)p * 2 * ld + col;
      const float4 u = ld4(q), v = ld4(q + ld);
      a = make_float4(a.x + u.x, a.y + u.y, a.z + u.z, a.w + u.w);
      b = make_float4(b.x + v.x, b.y + v.y, b.z + v.z, b.w + v.w);
    }
  }
  st4(&red[0][sl][cg * 4], a);
  st4(&red[1][sl][cg * 4], b);
  __syncthreads();
  if (threadIdx.x < 2 * LN_FIN_COLS) {
    const int which = threadIdx.x / LN_FIN_COLS, c = threadIdx.x % LN_FIN_COLS;
    float s = 0.f;
    for (int k = 0; k < SL; ++k) s += red[which][k][c];
    const int oc = blockIdx.x * LN_FIN_COLS + c;
    if (oc < ld) (which ? dbias : dgain)[oc] = s;
  }
}

bool ln_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t asr_ln_workspace_bytes(int T, int N, int n_pad, int ld, int H, int Hp,
                                         int segs) {
  LnGeo g;
  if (!ln_geo(T, N, n_pad, ld, H, Hp, segs, &g)) return 0;
  return ln_partial_bytes(g, ld);
}

extern "C" int asr_ln_max_width(void) { return LN_MAX_LD; }

#define LN_GEO_OR_FAIL(what)                                                                  \
  LnGeo g;                                                                                    \
  ASR_CHECK_ARG(ln_geo(T, N, n_pad, ld, H, Hp, segs, &g),                                     \
                what ": bad geometry (T %d N %d n_pad %d ld %d H %d Hp %d segs %d; ld a "     \
                     "multiple of 4, at most %d, Hp a multiple of 4, segs * Hp <= ld)",       \
                T, N, n_pad, ld, H, Hp, segs, LN_MAX_LD)

// one instantiation per (lanes per row, column groups per lane) the geometry can choose
#define LN_DISPATCH(LAUNCH)                                   \
  do {                                                        \
    if (g.lpr == 4) { LAUNCH(4, 1); }                         \
    else if (g.lpr == 16) { LAUNCH(16, 1); }                  \
    else if (g.vpl == 1) { LAUNCH(64, 1); }                   \
    else if (g.vpl == 2) { LAUNCH(64, 2); }                   \
    else if (g.vpl == 4) { LAUNCH(64, 4); }                   \
    else if (g.vpl == 8) { LAUNCH(64, 8); }                   \
    else { LAUNCH(64, 16); }                                  \
  } while (0)

extern "C" int asr_ln_fwd(const float* x, float* y, const float* gain, const float* bias,
                          float* stats, int T, int N, int n_pad, int ld, int H, int Hp, int segs,
                          float eps, asr_stream_t stream) {
  ASR_CHECK_ARG(x && y && gain && bias && eps > 0.f, "ln_fwd: bad arguments");
  ASR_CHECK_ARG(y != x, "ln_fwd: y must not alias x");
  ASR_CHECK_ARG(ln_aligned(x) && ln_aligned(y) && ln_aligned(gain) && ln_aligned(bias) &&
                    ((uintptr_t)stats & 7) == 0,
                "ln_fwd: x, y, gain, bias must be 16-byte aligned (stats 8-byte)");
  LN_GEO_OR_FAIL("ln_fwd");
  const float inv_cnt = 1.f / (float)((long long)segs * H);
  const int blocks = ln_blocks(g, LN_FWD_BLOCKS);
#define LN_FWD(LPR, VPL)                                                                         \
  hipLaunchKernelGGL((ln_fwd_kernel<LPR, VPL>), dim3(blocks), dim3(LN_THREADS), 0,               \
                     (hipStream_t)stream, x, y, gain, bias, stats, g.rows, N, n_pad, ld, H, Hp,  \
                     segs, inv_cnt, eps)
  LN_DISPATCH(LN_FWD);
#undef LN_FWD
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_ln_bwd(const float* x, const float* dy, const float* gain, const float* stats,
                          float* dx, float* dgain, float* dbias, int T, int N, int n_pad, int ld,
                          int H, int Hp, int segs, void* workspace, size_t ws_bytes,
                          asr_stream_t stream) {
  ASR_CHECK_ARG(x && dy && gain && stats && dgain && dbias, "ln_bwd: bad arguments");
  ASR_CHECK_ARG(dx != x && dx != dy, "ln_bwd: dx must not alias x or dy");
  ASR_CHECK_ARG(ln_aligned(x) && ln_aligned(dy) && ln_aligned(gain) && ln_aligned(dx) &&
                    ((uintptr_t)stats & 7) == 0 && ln_aligned(workspace),
                "ln_bwd: x, dy, gain, dx, workspace must be 16-byte aligned (stats 8-byte)");
  LN_GEO_OR_FAIL("ln_bwd");
  if (workspace == nullptr || ws_bytes < ln_partial_bytes(g, ld)) {
    asr_set_error("ln_bwd: workspace too small (%zu bytes needed)", ln_partial_bytes(g, ld));
    return ASR_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  const float inv_cnt = 1.f / (float)((long long)segs * H);
  const int blocks = ln_blocks(g, LN_BWD_BLOCKS);
  const size_t lds = (size_t)2 * ld * sizeof(float);
#define LN_BWD(LPR, VPL)                                                                         \
  hipLaunchKernelGGL((ln_bwd_kernel<LPR, VPL>), dim3(blocks), dim3(LN_THREADS), lds, s, x, dy,   \
                     gain, stats, dx, part, g.rows, N, n_pad, ld, H, Hp, segs, inv_cnt)
  LN_DISPATCH(LN_BWD);
#undef LN_BWD
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(ln_finish_kernel, dim3((ld + LN_FIN_COLS - 1) / LN_FIN_COLS),
                     dim3(LN_THREADS), 0, s, part, blocks, ld, dgain, dbias);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
