// K22 depthwise 1-D convolution over the time axis of a time-major slab (T, n_pad, ld), plus the
// two element-wise pairs of a Conformer block (GLU, Swish).  Exact fp32.
//
// Cross-correlation, k odd, w (k, C) tap major, p the LEFT PADDING: (k - 1) / 2 ('same', the
// asr_dwconv1d_fwd / _bwd entry points) or any 0 <= p <= k - 1 (asr_dwconv1d_pad_*; p = k - 1 is
// the causal convolution: no output frame reads a later input frame):
//   xm[u, n, c] = x[u, n, c] if 0 <= u < len_n else 0             (lens == NULL: len_n = T)
//   y[t, n, c]  = b[c] + sum_j w[j, c] xm[t + j - p, n, c]        every t < T, n < N, c < C
//   dx[u]       = sum_j w[j, c] dy[u - j + p]  for u < len_n, exactly 0 for u >= len_n
//   dw[j, c]    = sum_{t, n < N} dy[t, n, c] xm[t + j - p, n, c],   db[c] = sum_{t, n < N} dy
// The mask is a select: nothing a frame >= len_n holds can reach an output.  len_n is clamped to
// 0 .. T.  Rows n >= N and columns C <= col < ld of y and dx are written as exact zeros and are
// never read into a sum (they may hold anything in x and dy).
//
// Geometry.  The filter acts along t only, so a frame of the slab is one row of n_pad * ld
// independent columns; column q belongs to sample q / ld and channel q % ld.  A workgroup owns
// 16 neighbouring 16-byte column groups (256 bytes of every frame) and a tile of DW_TT = 64 frames.
// It stages the DW_TT + k - 1 frames of the tile and its halo (masked) into LDS, 256 bytes a row,
// and the filter taps of its columns beside them.  Thread (cg, ts) of the 16 x 16 keeps four
// consecutive output frames of column group cg in registers; for each tap it reads the tap and
// ONE new frame from LDS (the other three frames of its window are still in registers): two
// ds_read_b128 for 16 FMAs.  The 16 lanes of one ds_read_b128 lane group read 256 contiguous
// bytes or two rows' disjoint halves of the 64 banks: no conflicts.  dx is the same kernel with
// the taps reversed, no mask on its input and the mask on its output.
// dw / db: the same tiles plus the dy tile in LDS; thread (cg, js) keeps the RR = ceil(k / 16)
// consecutive taps js RR .. js RR + RR - 1 of column group cg and walks the tile's 64 frames with
// the same kind of register window (one dy and one x read per frame for 4 RR FMAs).  A workgroup
// walks every S-th tile of its columns and writes one partial per (segment, tap, column); a
// finishing kernel adds the partials of a channel over segments and samples in a fixed order.
// No float atomics: two identical calls give identical bits.  No workgroup waits on another.
#include "vec4.h"

namespace {

constexpr int DW_THREADS = 256;
constexpr int DW_CG = 16;                 // 16-byte column groups of a workgroup
constexpr int DW_TS = DW_THREADS / DW_CG; // time slots (forward) / tap slots (weight gradient)
constexpr int DW_R = 4;                   // output frames a thread keeps
constexpr int DW_TT = DW_TS * DW_R;       // 64 frames per tile
constexpr int DW_MAXK = 63;
constexpr int DW_TAPS = (DW_MAXK + DW_TS - 1) / DW_TS;   // most taps a thread of the dw kernel keeps
static_assert(DW_TAPS == 4, "dw_wgrad_kernel is instantiated for 1 .. 4 taps per thread");
constexpr int DW_WG_BLOCKS = 1024;        // workgroups the weight-gradient launch aims at
constexpr float DW_LOG2E = 1.4426950408889634f;

struct DwGeo {
  int T, N, n_pad, C, ld, k, p;
  long long W;              // floats of a frame: n_pad * ld
  int chunks, tiles, S;     // column chunks, time tiles, time segments of the weight gradient
};

bool dw_geo(int T, int N, int n_pad, int C, int ld, int k, DwGeo* g) {
  if (T < 1 || N < 1 || n_pad < N) return false;
  if (k < 1 || k > DW_MAXK || !(k & 1)) return false;
  if (C < 4 || (C & 3) || ld < C || (ld & 3)) return false;
  g->T = T, g->N = N, g->n_pad = n_pad, g->C = C, g->ld = ld, g->k = k, g->p = (k - 1) / 2;
  g->W = (long long)n_pad * ld;
  const long long chunks = (g->W / 4 + DW_CG - 1) / DW_CG;
  if (chunks > 0x7fffffffLL) return false;
  g->chunks = (int)chunks;
  g->tiles = (T + DW_TT - 1) / DW_TT;
  if (g->tiles > 65535) return false;
  int S = DW_WG_BLOCKS / g->chunks;
  S = S < 1 ? 1 : S;
  g->S = S < g->tiles ? S : g->tiles;
  return true;
}

size_t dw_ws_bytes(const DwGeo& g) {
  return asr_align_up((size_t)g.S * (g.k + 1) * (size_t)g.W * sizeof(float), 256);
}
size_t dw_lds_fwd(const DwGeo& g) { return (size_t)(DW_TT + 2 * g.k - 1) * DW_CG * 16; }
size_t dw_lds_bwd(const DwGeo& g) { return (size_t)(2 * DW_TT + g.k - 1) * DW_CG * 16; }

// What a thread knows of its column group: the sample, the channel, whether it is real.
struct DwCol {
  long long col;      // first float of the group within a frame
  int c, len;         // channel, valid frames of the sample (clamped to 0 .. T)
  bool in, real;      // inside the frame; a real sample's real channels
};

__device__ __forceinline__ DwCol dw_column(int cg, int T, int N, int C, int ld, long long W,
                                           const int* __restrict__ lens) {
  DwCol q;
  q.col = ((long long)blockIdx.x * DW_CG + cg) * 4;
  q.in = q.col < W;
  const int n = (int)(q.col / ld);
  q.c = (int)(q.col - (long long)n * ld);
  q.real = q.in && n < N && q.c < C;
  q.len = T;
  if (q.real && lens != nullptr) {
    const int l = lens[n];
    q.len = l < 0 ? 0 : (l > T ? T : l);
  }
  return q;
}

// rows frames from u0 on of this thread's column group -> dst[r * DW_CG + cg], zero where the
// column is not real or the frame is outside 0 .. lim - 1.  tid / DW_CG is the first row.
__device__ __forceinline__ void dw_stage(float4* __restrict__ dst, const float* __restrict__ src,
                                         const DwCol& q, int cg, long long W, int u0, int rows,
                                         int lim) {
  for (int r = threadIdx.x / DW_CG; r < rows; r += DW_TS) {
    const int u = u0 + r;
    float4 v = zero4();
    if (q.real && u >= 0 && u < lim) v = ld4(src + (size_t)u * W + q.col);
    dst[r * DW_CG + cg] = v;
  }
}

// acc[r] += sum_j Ws[j] Xs[ts * DW_R + r + j], j ascending: the register window of the forward
// kernels (one tap and ONE new frame read per tap)
__device__ __forceinline__ void dw_taps(const float4* __restrict__ Xs,
                                        const float4* __restrict__ Ws, int cg, int ts, int k,
                                        float4 (&acc)[DW_R]) {
  const float4* xr = Xs + (ts * DW_R) * DW_CG + cg;
  float4 x0 = xr[0], x1 = xr[DW_CG], x2 = xr[2 * DW_CG];
#pragma unroll 4
  for (int j = 0; j < k; ++j) {
    const float4 wv = Ws[j * DW_CG + cg];
    const float4 x3 = xr[(j + 3) * DW_CG];        // (row ts * 4 + j + 3 <= DW_TT + k - 2)
    acc[0] = fma4(wv, x0, acc[0]);
    acc[1] = fma4(wv, x1, acc[1]);
    acc[2] = fma4(wv, x2, acc[2]);
    acc[3] = fma4(wv, x3, acc[3]);
    x0 = x1, x1 = x2, x2 = x3;
  }
}

// out[t] = bias + sum_j w'[j] in_m[t + j - p] over the tile, p the left padding; flip: w'[j] = w[k - 1 - j] (the input
// gradient).  mask_in: the input's frames >= len are zeros; mask_out: the output's are.
__global__ void __launch_bounds__(DW_THREADS)
dw_conv_kernel(const float* __restrict__ in, const float* __restrict__ w,
               const float* __restrict__ bias, const int* __restrict__ lens,
               float* __restrict__ out, int T, int N, int C, int ld, long long W, int k, int p,
               int flip, int mask_in, int mask_out) {
  extern __shared__ float4 dw_sm[];
  const int rows = DW_TT + k - 1;
  float4* Xs = dw_sm;                       // rows x DW_CG
  float4* Ws = dw_sm + rows * DW_CG;        // k x DW_CG
  const int cg = threadIdx.x % DW_CG, ts = threadIdx.x / DW_CG;
  const int t0 = blockIdx.y * DW_TT;
  const DwCol q = dw_column(cg, T, N, C, ld, W, lens);
  // (columns ascend with the sample: a chunk that starts in the padding rows holds nothing real)
  const bool any_real = ((long long)blockIdx.x * DW_CG * 4) / ld < N;
  float4 acc[DW_R];
#pragma unroll
  for (int r = 0; r < DW_R; ++r) acc[r] = zero4();
  if (any_real) {
    dw_stage(Xs, in, q, cg, W, t0 - p, rows, mask_in ? q.len : T);
    for (int j = ts; j < k; j += DW_TS)
      Ws[j * DW_CG + cg] = q.real ? ld4(w + (size_t)(flip ? k - 1 - j : j) * C + q.c) : zero4();
    __syncthreads();
    if (q.real && bias != nullptr) {
      const float4 b = ld4(bias + q.c);
#pragma unroll
      for (int r = 0; r < DW_R; ++r) acc[r] = b;
    }
    dw_taps(Xs, Ws, cg, ts, k, acc);
  }
  if (!q.in) return;
#pragma unroll
  for (int r = 0; r < DW_R; ++r) {
    const int t = t0 + ts * DW_R + r;
    if (t >= T) break;
    const bool on = q.real && (!mask_out || t < q.len);
    st4(out + (size_t)t * W + q.col, on ? acc[r] : zero4());
  }
}

// K26, the streaming causal convolution: the output frames [t0, t0 + Tq) of dw_conv_kernel with
// p = k - 1, whose input is a ring (Rc >= k - 1 + Tq, n_pad, ld) that holds absolute frame u in
// row u % Rc (rows are indexed one by one: Rc need not be a multiple of anything).  Frames < 0
// and frames >= lens[n] (absolute, clamped to 0 .. t0 + Tq) are zeros by a select.  The same
// tiles, the same taps in the same order: bit for bit the rows of the whole-utterance call.
__global__ void __launch_bounds__(DW_THREADS)
dw_stream_kernel(const float* __restrict__ ring, const float* __restrict__ w,
                 const float* __restrict__ bias, const int* __restrict__ lens,
                 float* __restrict__ out, int Tq, int N, int C, int ld, long long W, int k, int Rc,
                 int t0) {
  extern __shared__ float4 dw_sm[];
  const int rows = DW_TT + k - 1;
  float4* Xs = dw_sm;                       // rows x DW_CG
  float4* Ws = dw_sm + rows * DW_CG;        // k x DW_CG
  const int cg = threadIdx.x % DW_CG, ts = threadIdx.x / DW_CG;
  const int r0 = blockIdx.y * DW_TT;        // first output row of the tile within the chunk
  const DwCol q = dw_column(cg, t0 + Tq, N, C, ld, W, lens);
  const bool any_real = ((long long)blockIdx.x * DW_CG * 4) / ld < N;
  float4 acc[DW_R];
#pragma unroll
  for (int r = 0; r < DW_R; ++r) acc[r] = zero4();
  if (any_real) {
    for (int r = ts; r < rows; r += DW_TS) {
      const int u = t0 + r0 + r - (k - 1);
      float4 v = zero4();
      if (q.real && u >= 0 && u < q.len) v = ld4(ring + (size_t)(u % Rc) * W + q.col);
      Xs[r * DW_CG + cg] = v;
    }
    for (int j = ts; j < k; j += DW_TS)
      Ws[j * DW_CG + cg] = q.real ? ld4(w + (size_t)j * C + q.c) : zero4();
    __syncthreads();
    if (q.real) {
      const float4 b = ld4(bias + q.c);
#pragma unroll
      for (int r = 0; r < DW_R; ++r) acc[r] = b;
    }
    dw_taps(Xs, Ws, cg, ts, k, acc);
  }
  if (!q.in) return;
#pragma unroll
  for (int r = 0; r < DW_R; ++r) {
    const int t = r0 + ts * DW_R + r;
    if (t >= Tq) break;
    st4(out + (size_t)t * W + q.col, q.real ? acc[r] : zero4());
  }
}

// part[(seg * (k + 1) + j) * W + col] = sum over the segment's tiles of dy[t] xm[t + j - p]
// (j < k) and of dy[t] (j = k), per column.  RR = ceil(k / DW_TS) taps per thread.
template <int RR>
__global__ void __launch_bounds__(DW_THREADS)
dw_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                const int* __restrict__ lens, float* __restrict__ part, int T, int N, int C,
                int ld, long long W, int k, int p, int tiles, int S) {
  extern __shared__ float4 dw_sm[];
  const int rows = DW_TT + k - 1;
  float4* Xs = dw_sm;                       // rows x DW_CG
  float4* Ds = dw_sm + rows * DW_CG;        // DW_TT x DW_CG
  const int cg = threadIdx.x % DW_CG, js = threadIdx.x / DW_CG;
  const DwCol q = dw_column(cg, T, N, C, ld, W, lens);
  const bool any_real = ((long long)blockIdx.x * DW_CG * 4) / ld < N;
  float4 acc[RR], accb = zero4();
#pragma unroll
  for (int r = 0; r < RR; ++r) acc[r] = zero4();
  if (any_real) {
    for (int tile = blockIdx.y; tile < tiles; tile += S) {
      const int t0 = tile * DW_TT;
      dw_stage(Xs, x, q, cg, W, t0 - p, rows, q.len);
      dw_stage(Ds, dy, q, cg, W, t0, DW_TT, T);
      __syncthreads();
      // the window: xw[r] = row t + js RR + r.  A tap j >= k (the last threads' when 16 RR > k)
      // reads up to 15 rows past Xs, inside Ds (64 rows): its sum is never stored.
      const float4* xr = Xs + (js * RR) * DW_CG + cg;
      float4 xw[RR];
#pragma unroll
      for (int r = 0; r + 1 < RR; ++r) xw[r] = xr[r * DW_CG];
#pragma unroll 4
      for (int t = 0; t < DW_TT; ++t) {
        const float4 d = Ds[t * DW_CG + cg];
        if (js == 0) accb = make_float4(accb.x + d.x, accb.y + d.y, accb.z + d.z, accb.w + d.w);
        xw[RR - 1] = xr[(t + RR - 1) * DW_CG];
#pragma unroll
        for (int r = 0; r < RR; ++r) acc[r] = fma4(d, xw[r], acc[r]);
#pragma unroll
        for (int r = 0; r + 1 < RR; ++r) xw[r] = xw[r + 1];
      }
      __syncthreads();
    }
  }
  if (!q.in) return;
  float* o = part + (size_t)blockIdx.y * (k + 1) * W + q.col;
#pragma unroll
  for (int r = 0; r < RR; ++r)
    if (js * RR + r < k) st4(o + (size_t)(js * RR + r) * W, acc[r]);
  if (js == 0) st4(o + (size_t)k * W, accb);
}

// dw[j, c] (j < k) or db[c] (j = k) = sum over (segment, sample) of the partials, in a fixed
// order: a workgroup owns one j and 16 channel groups, 16 slices take every 16th item each, the
// slices are then added in order out of LDS.
__global__ void __launch_bounds__(DW_THREADS)
dw_finish_kernel(const float* __restrict__ part, int S, int N, int C, int ld, long long W, int k,
                 float* __restrict__ dw, float* __restrict__ db) {
  __shared__ float4 red[DW_TS][DW_CG];
  const int cg = threadIdx.x % DW_CG, sl = threadIdx.x / DW_CG;
  const int j = blockIdx.x, c = (blockIdx.y * DW_CG + cg) * 4;
  float4 a = zero4();
  if (c < C) {
    const int items = S * N;
#pragma unroll 4
    for (int i = sl; i < items; i += DW_TS) {
      const int seg = i / N, n = i - seg * N;
      const float4 v = ld4(part + ((size_t)seg * (k + 1) + j) * W + (size_t)n * ld + c);
      a = make_float4(a.x + v.x, a.y + v.y, a.z + v.z, a.w + v.w);
    }
  }
  red[sl][cg] = a;
  __syncthreads();
  if (sl == 0 && c < C) {
    float4 s = red[0][cg];
    for (int i = 1; i < DW_TS; ++i) {
      const float4 v = red[i][cg];
      s = make_float4(s.x + v.x, s.y + v.y, s.z + v.z, s.w + v.w);
    }
    st4(j < k ? dw + (size_t)j * C + c : db + c, s);
  }
}

// ---------------------------------------------------------------------------- GLU, Swish
// sigma(x) and 1 - sigma(x) without overflow: e = 2^(-|x| log2 e) in (0, 1].
__device__ __forceinline__ void dw_sigmoid(float x, float* s, float* one_minus_s) {
  const float e = exp2f(-fabsf(x) * DW_LOG2E);
  const float r = 1.f / (1.f + e), er = e * r;
  *s = x >= 0.f ? r : er;
  *one_minus_s = x >= 0.f ? er : r;
}
__device__ __forceinline__ float dw_swish(float x) {
  float s, u;
  dw_sigmoid(x, &s, &u);
  return x * s;
}
__device__ __forceinline__ float dw_swish_grad(float x, float dy) {
  float s, u;
  dw_sigmoid(x, &s, &u);
  return dy * (s * fmaf(x, u, 1.f));
}
__device__ __forceinline__ float dw_glu(float a, float g) {
  float s, u;
  dw_sigmoid(g, &s, &u);
  return a * s;
}

__global__ void __launch_bounds__(256)
swish_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, n4 = n / 4;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = i0; i < n4; i += stride) {
    const float4 v = ld4(x + 4 * i);
    st4(y + 4 * i, make_float4(dw_swish(v.x), dw_swish(v.y), dw_swish(v.z), dw_swish(v.w)));
  }
  for (int64_t i = n4 * 4 + i0; i < n; i += stride) y[i] = dw_swish(x[i]);
}

__global__ void __launch_bounds__(256)
swish_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                 float* __restrict__ dx, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, n4 = n / 4;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = i0; i < n4; i += stride) {
    const float4 v = ld4(x + 4 * i), d = ld4(dy + 4 * i);
    st4(dx + 4 * i, make_float4(dw_swish_grad(v.x, d.x), dw_swish_grad(v.y, d.y),
                                dw_swish_grad(v.z, d.z), dw_swish_grad(v.w, d.w)));
  }
  for (int64_t i = n4 * 4 + i0; i < n; i += stride) dx[i] = dw_swish_grad(x[i], dy[i]);
}

// y (rows, ld_out): columns < C = a sigma(g), the others 0; a = x[:, :C], g = x[:, C:2C].
__global__ void __launch_bounds__(256)
glu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t rows, int C, int ld_in,
               int ld_out) {
  const int g4 = ld_out / 4;
  const int64_t total = rows * g4, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t row = i / g4;
    const int c = (int)(i - row * g4) * 4;
    float4 o = zero4();
    if (c < C) {
      const float4 a = ld4(x + row * ld_in + c), g = ld4(x + row * ld_in + C + c);
      o = make_float4(dw_glu(a.x, g.x), dw_glu(a.y, g.y), dw_glu(a.z, g.z), dw_glu(a.w, g.w));
    }
    st4(y + row * ld_out + c, o);
  }
}

__device__ __forceinline__ void dw_glu_grad(float a, float g, float dy, float* da, float* dg) {
  float s, u;
  dw_sigmoid(g, &s, &u);
  *da = dy * s;
  *dg = dy * a * (s * u);
}

// dx (rows, ld_in): [da | dg | zeros] from x and dy (rows, ld_out).
__global__ void __launch_bounds__(256)
glu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
               float* __restrict__ dx, int64_t rows, int C, int ld_in, int ld_out) {
  const int g4 = ld_in / 4;
  const int64_t total = rows * g4, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t row = i / g4;
    const int col = (int)(i - row * g4) * 4;
    float4 o = zero4();
    if (col < 2 * C) {
      const bool gate = col >= C;
      const int c = gate ? col - C : col;
      const float4 a = ld4(x + row * ld_in + c), g = ld4(x + row * ld_in + C + c);
      const float4 d = ld4(dy + row * ld_out + c);
      float da[4], dg[4];
      dw_glu_grad(a.x, g.x, d.x, &da[0], &dg[0]);
      dw_glu_grad(a.y, g.y, d.y, &da[1], &dg[1]);
      dw_glu_grad(a.z, g.z, d.z, &da[2], &dg[2]);
      dw_glu_grad(a.w, g.w, d.w, &da[3], &dg[3]);
      o = gate ? make_float4(dg[0], dg[1], dg[2], dg[3]) : make_float4(da[0], da[1], da[2], da[3]);
    }
    st4(dx + row * ld_in + col, o);
  }
}

bool dw_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned ew_blocks(int64_t items) {
  int64_t b = (items + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

#define DW_GEO_OR_FAIL(what)                                                                   \
  DwGeo g;                                                                                     \
  ASR_CHECK_ARG(dw_geo(T, N, n_pad, C, ld, k, &g),                                             \
                what ": bad geometry (T %d N %d n_pad %d C %d ld %d k %d; k odd in 1..%d, C "  \
                     "and ld multiples of 4, ld >= C, 1 <= N <= n_pad)",                       \
                T, N, n_pad, C, ld, k, DW_MAXK)

extern "C" size_t asr_dwconv1d_workspace_bytes(int T, int N, int n_pad, int C, int ld, int k) {
  DwGeo g;
  if (!dw_geo(T, N, n_pad, C, ld, k, &g)) return 0;
  return dw_ws_bytes(g);
}

extern "C" int asr_dwconv1d_plan(int T, int N, int n_pad, int C, int ld, int k, int backward,
                                 int* tile, int* blocks, int* lds_bytes) {
  DW_GEO_OR_FAIL("dwconv1d_plan");
  if (tile) *tile = DW_TT;
  if (blocks) *blocks = backward ? g.chunks * g.S : g.chunks * g.tiles;
  if (lds_bytes) *lds_bytes = (int)(backward ? dw_lds_bwd(g) : dw_lds_fwd(g));
  return ASR_OK;
}

#define DW_PAD_OR_FAIL(what)                                                                   \
  ASR_CHECK_ARG(pad_left >= 0 && pad_left <= k - 1,                                            \
                what ": pad_left %d outside 0 .. k - 1 = %d", pad_left, k - 1)

extern "C" int asr_dwconv1d_pad_fwd(const float* x, const float* w, const float* b,
                                    const int* lens, float* y, int T, int N, int n_pad, int C,
                                    int ld, int k, int pad_left, asr_stream_t stream) {
  DW_GEO_OR_FAIL("dwconv1d_fwd");
  DW_PAD_OR_FAIL("dwconv1d_fwd");
  ASR_CHECK_ARG(x && w && b && y && y != x, "dwconv1d_fwd: x, w, b, y are required (y != x)");
  ASR_CHECK_ARG(dw_aligned(x) && dw_aligned(w) && dw_aligned(b) && dw_aligned(y),
                "dwconv1d_fwd: x, w, b, y must be 16-byte aligned");
  hipLaunchKernelGGL(dw_conv_kernel, dim3(g.chunks, g.tiles), dim3(DW_THREADS), dw_lds_fwd(g),
                     (hipStream_t)stream, x, w, b, lens, y, T, N, C, ld, g.W, k, pad_left, 0, 1,
                     0);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_dwconv1d_stream_fwd(const float* ring, const float* w, const float* b,
                                       const int* lens, float* y, int Tq, int N, int n_pad, int C,
                                       int ld, int k, int ring_rows, int t0,
                                       asr_stream_t stream) {
  const int T = Tq;
  DW_GEO_OR_FAIL("dwconv1d_stream_fwd");
  ASR_CHECK_ARG(t0 >= 0 && (long long)t0 + Tq <= 0x7fffffffLL - DW_TT - DW_MAXK,
                "dwconv1d_stream_fwd: t0 %d (>= 0, t0 + Tq below 2^31)", t0);
  ASR_CHECK_ARG(ring_rows >= k - 1 + Tq, "dwconv1d_stream_fwd: a ring of %d rows (k - 1 + Tq = "
                "%d needed)", ring_rows, k - 1 + Tq);
  ASR_CHECK_ARG(ring && w && b && lens && y && y != ring,
                "dwconv1d_stream_fwd: ring, w, b, lens, y are required (y != ring)");
  ASR_CHECK_ARG(dw_aligned(ring) && dw_aligned(w) && dw_aligned(b) && dw_aligned(y),
                "dwconv1d_stream_fwd: ring, w, b, y must be 16-byte aligned");
  hipLaunchKernelGGL(dw_stream_kernel, dim3(g.chunks, g.tiles), dim3(DW_THREADS), dw_lds_fwd(g),
                     (hipStream_t)stream, ring, w, b, lens, y, Tq, N, C, ld, g.W, k, ring_rows,
                     t0);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_dwconv1d_fwd(const float* x, const float* w, const float* b, const int* lens,
                                float* y, int T, int N, int n_pad, int C, int ld, int k,
                                asr_stream_t stream) {
  return asr_dwconv1d_pad_fwd(x, w, b, lens, y, T, N, n_pad, C, ld, k, (k - 1) / 2, stream);
}

extern "C" int asr_dwconv1d_pad_bwd(const float* x, const float* w, const float* dy,
                                    const int* lens, float* dx, float* dw, float* db, int T, int N,
                                    int n_pad, int C, int ld, int k, int pad_left, void* workspace,
                                    size_t ws_bytes, asr_stream_t stream) {
  DW_GEO_OR_FAIL("dwconv1d_bwd");
  DW_PAD_OR_FAIL("dwconv1d_bwd");
  ASR_CHECK_ARG(x && w && dy && dw && db, "dwconv1d_bwd: x, w, dy, dw, db are required");
  ASR_CHECK_ARG(dx != x && dx != dy, "dwconv1d_bwd: dx must not alias x or dy");
  ASR_CHECK_ARG(dw_aligned(x) && dw_aligned(w) && dw_aligned(dy) && dw_aligned(dx) &&
                    dw_aligned(dw) && dw_aligned(db) && dw_aligned(workspace),
                "dwconv1d_bwd: x, w, dy, dx, dw, db, workspace must be 16-byte aligned");
  if (workspace == nullptr || ws_bytes < dw_ws_bytes(g)) {
    asr_set_error("dwconv1d_bwd: workspace too small (%zu bytes needed)", dw_ws_bytes(g));
    return ASR_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)workspace;
  if (dx != nullptr) {
    hipLaunchKernelGGL(dw_conv_kernel, dim3(g.chunks, g.tiles), dim3(DW_THREADS), dw_lds_fwd(g),
                       s, dy, w, (const float*)nullptr, lens, dx, T, N, C, ld, g.W, k,
                       k - 1 - pad_left, 1, 0, 1);
    ASR_CHECK_LAUNCH();
  }
#define DW_WGRAD(RR)                                                                              \
  hipLaunchKernelGGL(dw_wgrad_kernel<RR>, dim3(g.chunks, g.S), dim3(DW_THREADS), dw_lds_bwd(g),   \
                     s, x, dy, lens, part, T, N, C, ld, g.W, k, pad_left, g.tiles, g.S)
  switch ((k + DW_TS - 1) / DW_TS) {        // taps per thread: 1 .. DW_TAPS
    case 1: DW_WGRAD(1); break;
    case 2: DW_WGRAD(2); break;
    case 3: DW_WGRAD(3); break;
    default: DW_WGRAD(4); break;
  }
#undef DW_WGRAD
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(dw_finish_kernel, dim3(k + 1, (C / 4 + DW_CG - 1) / DW_CG),
                     dim3(DW_THREADS), 0, s, part, g.S, N, C, ld, g.W, k, dw, db);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_dwconv1d_bwd(const float* x, const float* w, const float* dy, const int* lens,
                                float* dx, float* dw, float* db, int T, int N, int n_pad, int C,
                                int ld, int k, void* workspace, size_t ws_bytes,
                                asr_stream_t stream) {
  return asr_dwconv1d_pad_bwd(x, w, dy, lens, dx, dw, db, T, N, n_pad, C, ld, k, (k - 1) / 2,
                              workspace, ws_bytes, stream);
}

extern "C" int asr_swish_fwd(const float* x, float* y, int64_t n, asr_stream_t stream) {
  ASR_CHECK_ARG(x && y && n > 0, "swish_fwd: bad arguments");
  ASR_CHECK_ARG(dw_aligned(x) && dw_aligned(y), "swish_fwd: 16-byte alignment");
  hipLaunchKernelGGL(swish_fwd_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream,
                     x, y, n);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_swish_bwd(const float* x, const float* dy, float* dx, int64_t n,
                             asr_stream_t stream) {
  ASR_CHECK_ARG(x && dy && dx && n > 0, "swish_bwd: bad arguments");
  ASR_CHECK_ARG(dw_aligned(x) && dw_aligned(dy) && dw_aligned(dx), "swish_bwd: 16-byte alignment");
  hipLaunchKernelGGL(swish_bwd_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream,
                     x, dy, dx, n);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

#define GLU_GEO_OR_FAIL(what)                                                                   \
  ASR_CHECK_ARG(rows > 0 && C >= 4 && !(C & 3) && ld_in >= 2 * (int64_t)C && !(ld_in & 3) &&    \
                    ld_out >= C && !(ld_out & 3),                                               \
                what ": bad geometry (rows %lld C %d ld_in %d ld_out %d; C, ld_in, ld_out "     \
                     "multiples of 4, ld_in >= 2 C, ld_out >= C)",                              \
                (long long)rows, C, ld_in, ld_out)

extern "C" int asr_glu_fwd(const float* x, float* y, int64_t rows, int C, int ld_in, int ld_out,
                           asr_stream_t stream) {
  GLU_GEO_OR_FAIL("glu_fwd");
  ASR_CHECK_ARG(x && y && y != x, "glu_fwd: x and y are required (y != x)");
  ASR_CHECK_ARG(dw_aligned(x) && dw_aligned(y), "glu_fwd: 16-byte alignment");
  hipLaunchKernelGGL(glu_fwd_kernel, dim3(ew_blocks(rows * (ld_out / 4))), dim3(256), 0,
                     (hipStream_t)stream, x, y, rows, C, ld_in, ld_out);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_glu_bwd(const float* x, const float* dy, float* dx, int64_t rows, int C,
                           int ld_in, int ld_out, asr_stream_t stream) {
  GLU_GEO_OR_FAIL("glu_bwd");
  ASR_CHECK_ARG(x && dy && dx && dx != x && dx != dy, "glu_bwd: x, dy, dx are required");
  ASR_CHECK_ARG(dw_aligned(x) && dw_aligned(dy) && dw_aligned(dx), "glu_bwd: 16-byte alignment");
  hipLaunchKernelGGL(glu_bwd_kernel, dim3(ew_blocks(rows * (ld_in / 4))), dim3(256), 0,
                     (hipStream_t)stream, x, dy, dx, rows, C, ld_in, ld_out);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
