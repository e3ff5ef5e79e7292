// K33 time reduction by frame stacking: k consecutive frames of a time-major slab become one
// frame of k times the width, and the exact adjoint.  Pure data movement, exact by construction.
//
//   x (T, n_pad, ld_in), y (To, n_pad, ld_out), To = ceil(T / k), F <= ld_in, k F <= ld_out
//   len_n = clamp(lens[n], 0, T) for n < N; T for n >= N or lens == NULL
//   y[to, n, j F + f] = x[to k + j, n, f]   where j < k, f < F and to k + j < len_n, else 0
//   y[to, n, c] = 0                         for k F <= c < ld_out
//   dx[t, n, f] = dy[t / k, n, (t % k) F + f]   where f < F and t < len_n, else 0
//   dx[t, n, c] = 0                             for F <= c < ld_in
// Columns >= F of x and columns >= k F of dy are never read.  A frame at or past len_n is never
// read either (the mask is a select), so what a slab holds behind an utterance cannot reach a
// valid output frame, and len_n <= T keeps every read inside the slab.
//
// Launch: one item per four OUTPUT columns (a 16-byte store; both leading dimensions are
// multiples of 4), a grid capped at 4096 workgroups of 256 threads, a grid-stride loop: the shape
// of the flat kernels of dwconv.hip (ew_blocks).  F % 4 == 0: a column group lies inside one
// source frame and is one 16-byte load; any other F (MFCC-39): four scalar loads, each with its
// own source frame.  Every output element is written exactly once by exactly one thread: no
// atomics, no workspace, no workgroup waits on another, repeats are bit-identical.
#include "vec4.h"

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_MAX_BLOCKS = 4096;
constexpr int TS_MIN_K = 2, TS_MAX_K = 8;

__device__ __forceinline__ int ts_len(const int* __restrict__ lens, int n, int N, int T) {
  if (lens == nullptr || n >= N) return T;
  const int l = lens[n];
  return l < 0 ? 0 : (l > T ? T : l);
}

template <bool VEC>
__global__ void __launch_bounds__(TS_THREADS)
ts_fwd_kernel(const float* __restrict__ x, const int* __restrict__ lens, float* __restrict__ y,
              int T, int To, int N, int n_pad, int F, int ld_in, int ld_out, int k) {
  const int g4 = ld_out / 4, kF = k * F;
  const int64_t total = (int64_t)To * n_pad * g4, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t row = i / g4;                 // to * n_pad + n
    const int c = (int)(i - row * g4) * 4;
    const int to = (int)(row / n_pad), n = (int)(row - (int64_t)to * n_pad);
    float4 o = zero4();
    if (c < kF) {
      const int len = ts_len(lens, n, N, T);
      if (VEC) {
        const int j = c / F, t = to * k + j;
        if (t < len) o = ld4(x + ((int64_t)t * n_pad + n) * ld_in + (c - j * F));
      } else {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ce = c + e, j = ce / F, t = to * k + j;
          v[e] = (ce < kF && t < len) ? x[((int64_t)t * n_pad + n) * ld_in + (ce - j * F)] : 0.f;
        }
        o = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    st4(y + row * ld_out + c, o);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(TS_THREADS)
ts_bwd_kernel(const float* __restrict__ dy, const int* __restrict__ lens, float* __restrict__ dx,
              int T, int N, int n_pad, int F, int ld_in, int ld_out, int k) {
  const int g4 = ld_in / 4;
  const int64_t total = (int64_t)T * n_pad * g4, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t row = i / g4;                 // t * n_pad + n
    const int c = (int)(i - row * g4) * 4;
    const int t = (int)(row / n_pad), n = (int)(row - (int64_t)t * n_pad);
    float4 o = zero4();
    if (c < F && t < ts_len(lens, n, N, T)) {
      const int to = t / k, j = t - to * k;
      const float* src = dy + ((int64_t)to * n_pad + n) * ld_out + j * F + c;
      if (VEC) {
        o = ld4(src);
      } else {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < F ? src[e] : 0.f;
        o = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    st4(dx + row * ld_in + c, o);
  }
}

bool ts_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned ts_blocks(int64_t items) {
  int64_t b = (items + TS_THREADS - 1) / TS_THREADS;
  return (unsigned)(b < 1 ? 1 : (b > TS_MAX_BLOCKS ? TS_MAX_BLOCKS : b));
}

}  // namespace

#define TS_GEO_OR_FAIL(what)                                                                     \
  ASR_CHECK_ARG(T >= 1 && k >= TS_MIN_K && k <= TS_MAX_K && F >= 1 && ld_in >= F &&              \
                    (long long)ld_out >= (long long)k * F && !(ld_in & 3) && !(ld_out & 3) &&    \
                    n_pad >= 16 && !(n_pad & 15) && N >= 1 && N <= n_pad,                        \
                what ": bad geometry (T %d N %d n_pad %d F %d ld_in %d ld_out %d k %d; k in "    \
                     "%d..%d, F >= 1, ld_in >= F, ld_out >= k F, both multiples of 4, n_pad a "  \
                     "multiple of 16, 1 <= N <= n_pad)",                                         \
                T, N, n_pad, F, ld_in, ld_out, k, TS_MIN_K, TS_MAX_K)

extern "C" int asr_time_stack_fwd(const float* x, const int* lens, float* y, int T, int N,
                                  int n_pad, int F, int ld_in, int ld_out, int k,
                                  asr_stream_t stream) {
  TS_GEO_OR_FAIL("time_stack_fwd");
  ASR_CHECK_ARG(x && y && y != x, "time_stack_fwd: x and y are required (y != x)");
  ASR_CHECK_ARG(ts_aligned(x) && ts_aligned(y), "time_stack_fwd: x, y must be 16-byte aligned");
  const int To = (T + k - 1) / k;
  const unsigned blocks = ts_blocks((int64_t)To * n_pad * (ld_out / 4));
  if (F % 4 == 0)
    hipLaunchKernelGGL(ts_fwd_kernel<true>, dim3(blocks), dim3(TS_THREADS), 0,
                       (hipStream_t)stream, x, lens, y, T, To, N, n_pad, F, ld_in, ld_out, k);
  else
    hipLaunchKernelGGL(ts_fwd_kernel<false>, dim3(blocks), dim3(TS_THREADS), 0,
                       (hipStream_t)stream, x, lens, y, T, To, N, n_pad, F, ld_in, ld_out, k);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_time_stack_bwd(const float* dy, const int* lens, float* dx, int T, int N,
                                  int n_pad, int F, int ld_in, int ld_out, int k,
                                  asr_stream_t stream) {
  TS_GEO_OR_FAIL("time_stack_bwd");
  ASR_CHECK_ARG(dy && dx && dx != dy, "time_stack_bwd: dy and dx are required (dx != dy)");
  ASR_CHECK_ARG(ts_aligned(dy) && ts_aligned(dx),
                "time_stack_bwd: dy, dx must be 16-byte aligned");
  const unsigned blocks = ts_blocks((int64_t)T * n_pad * (ld_in / 4));
  if (F % 4 == 0)
    hipLaunchKernelGGL(ts_bwd_kernel<true>, dim3(blocks), dim3(TS_THREADS), 0,
                       (hipStream_t)stream, dy, lens, dx, T, N, n_pad, F, ld_in, ld_out, k);
  else
    hipLaunchKernelGGL(ts_bwd_kernel<false>, dim3(blocks), dim3(TS_THREADS), 0,
                       (hipStream_t)stream, dy, lens, dx, T, N, n_pad, F, ld_in, ld_out, k);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
