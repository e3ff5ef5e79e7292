// K23 SpecAugment (arXiv 1904.08779) on the input slab -- gfx950.
//
// One pass over the (T, n_pad, ld) time-major slab: a piecewise-linear time warp, mF frequency
// masks and mT time masks per utterance, drawn from the library's Philox-4x32-10 streams
// (random.hip; key = the 64-bit seed, counter = (block, stream id, step, block >> 32)).  Sample n
// owns the B = 1 + ceil((mF + mT) / 2) blocks from n * B on: block 0 draws the warp (word 0 the
// centre, word 1 the displacement), mask m (frequency masks first) takes block 1 + m / 2, words
// 2 (m % 2) (width) and 2 (m % 2) + 1 (start).  rand(word, K) = umulhi(word, K) in [0, K): exact
// integers, which tests/specaugment_oracle.py reproduces with 64-bit products.  The semantics are
// in include/asr_hip.h and DESIGN.md section 23.
//
// Shape: one launch.  A workgroup owns a tile of TC frames x NS samples (whole rows: contiguous
// NS * ld floats per frame) and
//   1. draws the parameters of its NS samples into LDS (one thread per warp draw / mask: at most
//      NS * 65 Philox blocks per workgroup, a few thousand VALU instructions against >= 20 KB
//      moved: no table in HBM, no second launch, no workspace argument),
//   2. forms one descriptor per row of the tile (source frames i0 / i1 and the fraction of the
//      warp, by ONE 64-bit division per row; the time-mask flag) and, for F <= 1024, one bit per
//      column and sample for the frequency masks (wider slabs walk the masks per element),
//   3. streams the tile: 16 bytes per lane where ld % 4 == 0, one 32-bit division per access.
// A masked element is a select, never a product; what is not augmented is copied bit for bit.
// Memory-bound: one read and one write of the slab; warped rows read two neighbouring source
// rows of the same sample, which neighbouring tiles read too (L2).
#include "philox.h"

namespace {

constexpr int NS = 8;             // samples per tile
constexpr int TC = 8;             // frames per tile
constexpr int ROWS = NS * TC;
constexpr int MAX_MASKS = 64;     // mF + mT
constexpr int FM_WORDS = 32;      // the frequency masks as a bitmap of the columns < 32 * FM_WORDS

enum { ROW_PRESENT = 1, ROW_VALID = 2, ROW_WARP = 4, ROW_TMASK = 8 };

__device__ __forceinline__ int rand_below(unsigned word, int k) {
  return (int)__umulhi(word, (unsigned)k);
}

struct Policy {
  int W, mF, Fw, mT, Tw;
  float p, mask_value;
};

template <int V>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  } else {
    v[0] = *p;
  }
}

template <int V>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[V]) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}

template <int V>
__global__ void __launch_bounds__(256)
specaug_kernel(const float* __restrict__ in, float* __restrict__ out,
               const int* __restrict__ lens, int T, int N, int n_pad, int F, int ld, Policy q,
               unsigned k0, unsigned k1, unsigned stream_id, unsigned step,
               int* __restrict__ params_out) {
  __shared__ int s_len[NS], s_c[NS], s_cp[NS];
  __shared__ int s_lo[NS][MAX_MASKS], s_hi[NS][MAX_MASKS];     // mask m covers [lo, hi)
  __shared__ int s_i0[ROWS], s_i1[ROWS], s_flag[ROWS];
  __shared__ float s_frac[ROWS];
  __shared__ unsigned s_fm[NS][FM_WORDS];

  const int tid = threadIdx.x;
  const int t_base = blockIdx.x * TC, n_base = blockIdx.y * NS;
  const int nm = q.mF + q.mT;
  const int B = 1 + (nm + 1) / 2;
  const bool emit = params_out != nullptr && blockIdx.x == 0;
  const bool bitmap = F <= 32 * FM_WORDS;       // (wider: the masks are walked per element)

  // 1. the draws of this tile's samples: entry 0 of a sample is its warp, entry 1 + m its mask m
  for (int j = tid; j < NS * (nm + 1); j += 256) {
    const int s = j / (nm + 1), k = j - s * (nm + 1), n = n_base + s;
    const bool real = n < N;
    int len = 0;
    if (real) len = lens ? min(max(lens[n], 0), T) : T;
    const unsigned long long blk = (unsigned long long)n * (unsigned)B + (k ? 1 + (k - 1) / 2 : 0);
    const Philox r = philox4x32_10((unsigned)blk, stream_id, step, (unsigned)(blk >> 32), k0, k1);
    int* po = emit && real ? params_out + (long long)n * (2 + 2 * nm) : nullptr;
    if (k == 0) {
      int c = -1, cp = -1;
      const int Wn = min(q.W, (len - 1) / 2);
      if (real && Wn > 0) {
        c = Wn + rand_below(r.c[0], len - 2 * Wn);
        cp = c + rand_below(r.c[1], 2 * Wn + 1) - Wn;
      }
      s_len[s] = len; s_c[s] = c; s_cp[s] = cp;
      if (po) { po[0] = c; po[1] = cp; }
    } else {
      const int m = k - 1;
      const unsigned wa = (m & 1) ? r.c[2] : r.c[0], wb = (m & 1) ? r.c[3] : r.c[1];
      int width, start;
      if (m < q.mF) {
        width = rand_below(wa, min(q.Fw, F) + 1);
        start = rand_below(wb, F - width + 1);
      } else {
        const int cap = min(min(q.Tw > 0 ? q.Tw : len, (int)floorf(q.p * (float)len)), len);
        width = rand_below(wa, cap + 1);
        start = rand_below(wb, len - width + 1);
      }
      s_lo[s][m] = start; s_hi[s][m] = start + width;
      if (po) { po[2 + 2 * m] = width; po[3 + 2 * m] = start; }
    }
  }
  __syncthreads();

  // 2. one descriptor per row (frame, sample) of the tile
  if (tid < ROWS) {
    const int s = tid % NS, t = t_base + tid / NS, n = n_base + s;
    int flag = 0, i0 = t, i1 = t;
    float frac = 0.f;
    if (t < T && n < n_pad) {
      flag = ROW_PRESENT;
      const int len = s_len[s];
      if (n < N && t < len) {
        flag |= ROW_VALID;
        const int c = s_c[s], cp = s_cp[s];
        if (c >= 0) {
          // t < c': source position t c / c'; else c + (t - c') (len - c) / (len - c').  No zero
          // denominator: the first branch needs c' > t >= 0, and c' <= len - 1.
          flag |= ROW_WARP;
          long long num, den;
          int base;
          if (t < cp) { num = (long long)t * c; den = cp; base = 0; }
          else { num = (long long)(t - cp) * (len - c); den = len - cp; base = c; }
          const long long quo = num / den;
          i0 = base + (int)quo;
          i1 = min(i0 + 1, len - 1);
          frac = (float)(int)(num - quo * den) / (float)(int)den;
        }
        for (int m = q.mF; m < nm; ++m)
          if (t >= s_lo[s][m] && t < s_hi[s][m]) flag |= ROW_TMASK;
      }
    }
    s_i0[tid] = i0; s_i1[tid] = i1; s_frac[tid] = frac; s_flag[tid] = flag;
  }
  // ... and the frequency masks of each sample as one bit per column
  if (bitmap) {
    for (int j = tid; j < NS * FM_WORDS; j += 256) {
      const int s = j / FM_WORDS, c0 = 32 * (j % FM_WORDS);
      unsigned bits = 0;
      for (int m = 0; m < q.mF; ++m) {
        const int a = max(s_lo[s][m] - c0, 0), b = min(s_hi[s][m] - c0, 32);
        if (a < b) bits |= (b - a == 32 ? ~0u : (1u << (b - a)) - 1u) << a;
      }
      s_fm[s][j % FM_WORDS] = bits;
    }
  }
  __syncthreads();

  // 3. the tile, V floats per access
  const int ldv = ld / V;
  for (int e = tid; e < ROWS * ldv; e += 256) {
    const int row = e / ldv, col = (e - row * ldv) * V;
    const int flag = s_flag[row];
    if (!flag) continue;
    const int s = row % NS, t = t_base + row / NS, n = n_base + s;
    const size_t off = ((size_t)t * n_pad + n) * ld + col;
    float y[V];
    if (!(flag & ROW_VALID)) {              // frames past the length, rows n >= N: bit for bit
      load_vec<V>(in + off, y);
      store_vec<V>(out + off, y);
      continue;
    }
    const bool edge = col + V > F;          // holds pad columns (col >= F): those are copied
    if ((flag & ROW_TMASK) && !edge) {
#pragma unroll
      for (int j = 0; j < V; ++j) y[j] = q.mask_value;
      store_vec<V>(out + off, y);
      continue;
    }
    if (!(flag & ROW_WARP) || edge) load_vec<V>(in + off, y);
    if ((flag & ROW_WARP) && col < F) {
      float a[V], b[V];
      load_vec<V>(in + ((size_t)s_i0[row] * n_pad + n) * ld + col, a);
      load_vec<V>(in + ((size_t)s_i1[row] * n_pad + n) * ld + col, b);
      const float frac = s_frac[row];
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (col + j < F) y[j] = a[j] + frac * (b[j] - a[j]);
    }
    // (a 16-byte group starts at a multiple of 4: its bits lie in one word of the bitmap)
    unsigned fbits = 0;
    if (bitmap) {
      if (col < F) fbits = s_fm[s][col >> 5] >> (col & 31);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j)
        for (int m = 0; m < q.mF; ++m)
          if (col + j >= s_lo[s][m] && col + j < s_hi[s][m]) fbits |= 1u << j;
    }
    if (flag & ROW_TMASK) fbits = ~0u;
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (((fbits >> j) & 1u) && col + j < F) y[j] = q.mask_value;
    store_vec<V>(out + off, y);
  }
}

}  // namespace

extern "C" int asr_specaug_apply(const float* in, float* out, const int* lens, int T, int N,
                                 int n_pad, int F, int ld, int W, int mF, int Fw, int mT, int Tw,
                                 float p, float mask_value, uint64_t seed, uint32_t stream_id,
                                 uint32_t step, int* params_out, asr_stream_t stream) {
  ASR_CHECK_ARG(in && out && in != out, "specaug_apply: in and out must be two buffers");
  ASR_CHECK_ARG(T >= 1 && N >= 0 && n_pad >= 1 && N <= n_pad && F >= 1,
                "specaug_apply: bad shape (T %d, N %d, n_pad %d, F %d)", T, N, n_pad, F);
  ASR_CHECK_ARG(ld >= F && ld <= (1 << 24), "specaug_apply: ld %d (F %d .. 2^24)", ld, F);
  ASR_CHECK_ARG(W >= 0 && mF >= 0 && Fw >= 0 && mT >= 0 && Tw >= 0,
                "specaug_apply: negative count or width");
  ASR_CHECK_ARG(mF <= MAX_MASKS && mT <= MAX_MASKS && mF + mT <= MAX_MASKS,
                "specaug_apply: %d + %d masks (at most %d)", mF, mT, MAX_MASKS);
  ASR_CHECK_ARG(p >= 0.f && p <= 1.f, "specaug_apply: p must be in [0, 1]");
  const uintptr_t slabs = reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out);
  ASR_CHECK_ARG((slabs & (ld % 4 == 0 ? 15 : 3)) == 0,
                "specaug_apply: in / out alignment (16 bytes where ld %% 4 == 0)");
  ASR_CHECK_ARG(((reinterpret_cast<uintptr_t>(lens) | reinterpret_cast<uintptr_t>(params_out)) & 3)
                    == 0, "specaug_apply: lens / params_out alignment");
  const long long gy = ((long long)n_pad + NS - 1) / NS;
  ASR_CHECK_ARG(gy <= 65535, "specaug_apply: n_pad %d (at most %d)", n_pad, 65535 * NS);
  const dim3 grid((unsigned)(((long long)T + TC - 1) / TC), (unsigned)gy);
  Policy q;
  q.W = W; q.mF = mF; q.Fw = Fw; q.mT = mT; q.Tw = Tw; q.p = p; q.mask_value = mask_value;
  const unsigned k0 = (unsigned)(seed & 0xffffffffu), k1 = (unsigned)(seed >> 32);
  if (ld % 4 == 0)
    hipLaunchKernelGGL(specaug_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, in, out, lens,
                       T, N, n_pad, F, ld, q, k0, k1, stream_id, step, params_out);
  else
    hipLaunchKernelGGL(specaug_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, in, out, lens,
                       T, N, n_pad, F, ld, q, k0, k1, stream_id, step, params_out);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
