// K4/K6 fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32) + column sum -- gfx950.
//
// Replaces the hoisted input->4H gate matmul K.dot(x*B_W, W) (core/layers.py:439),
// TimeDistributed(Dense) (core/models.py:278-279) and their gradients.  fp32 in /
// fp32 accumulate MFMA is bit-identical to an fmaf chain, so the 1e-4 parity
// budget is untouched (there is no xf32/TF32 path on gfx950).
//
// Tiling: 128x128x16 block tile, 256 threads = 4 waves in a 2x2 grid, each wave
// owns a 64x64 sub-tile = 2x2 MFMA tiles of 32x32 (64 accumulator VGPRs).  Both
// operands are staged K-MAJOR in LDS (As[k][m], Bs[k][n], row pad 4) so that the
// MFMA fragment reads (lane l -> [k = 2kk + l/32][l%32]) are conflict-free
// ds_read_b32; whichever of the four storage orders the caller has is transposed
// on the way in (16-byte global loads; ds_write_b128 for mn-contiguous sources,
// 2-way (free) ds_write_b32 for k-contiguous ones).  Global->register prefetch of
// tile k+1 overlaps the 32 MFMAs of tile k; one barrier per K step.
// Variational-dropout masks (core/models.py:265-266) are applied in the loader
// (A side) or the epilogue (C side), bias in the epilogue.  Split-K writes
// per-split partials and reduces them in a fixed order (deterministic).
// The kernels on packed planes are in gemm_hl.hip, the packs and flat reductions in pack.hip.
#include "gemm_common.h"

namespace {

constexpr int BM = 128, BN = 128, PAD = 4;
constexpr int LDS_LD = BM + PAD;   // BM == BN

struct TileSrc {
  const float* p;      // base pointer
  int ld;              // leading dimension of the storage
  int mn_contig;       // 1: storage is (K, MN) row-major; 0: (MN, K) row-major
  int mn_total, k_total;
  const float* scale;  // optional mask over storage (row % period, col)
  int period, scale_ld;
  int vec_ok;          // 16-byte aligned rows
  int scale_vec;       // mask rows 16-byte aligned as well
};

// Loads the (BK x 128) tile starting at (k0, mn0) into BK/8 float4 registers.
template <int BK>
__device__ __forceinline__ void tile_load(const TileSrc& s, int k0, int mn0, int k_end,
                                          float4 (&r)[BK / 8]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < BK / 8; ++it) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (s.mn_contig) {
      const int kk = (tid >> 5) + 8 * it;
      const int mn = mn0 + 4 * (tid & 31);
      const int k = k0 + kk;
      if (k < k_end) {
        const float* src = s.p + (size_t)k * s.ld + mn;
        if (s.vec_ok && mn + 3 < s.mn_total) {
          const float4 q = *reinterpret_cast<const float4*>(src);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (mn + e < s.mn_total) v[e] = src[e];
        }
        if (s.scale) {
          const float* sc = s.scale + (size_t)mod_period(k, s.period) * s.scale_ld + mn;
          if (s.scale_vec && mn + 3 < s.mn_total) {
            const float4 q = *reinterpret_cast<const float4*>(sc);
            v[0] *= q.x; v[1] *= q.y; v[2] *= q.z; v[3] *= q.w;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (mn + e < s.mn_total) v[e] *= sc[e];
          }
        }
      }
    } else {
      // BK/4 float4 per row; thread -> (row, k-quad)
      constexpr int QPR = BK / 4;                 // k-quads per row
      const int e = tid + 256 * it;
      const int mn = mn0 + e / QPR;
      const int k = k0 + 4 * (e % QPR);
      if (mn < s.mn_total) {
        const float* src = s.p + (size_t)mn * s.ld + k;
        if (s.vec_ok && k + 3 < k_end) {
          const float4 q = *reinterpret_cast<const float4*>(src);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (k + e < k_end) v[e] = src[e];
        }
        if (s.scale) {
          const float* sc = s.scale + (size_t)mod_period(mn, s.period) * s.scale_ld + k;
          if (s.scale_vec && k + 3 < k_end) {
            const float4 q = *reinterpret_cast<const float4*>(sc);
            v[0] *= q.x; v[1] *= q.y; v[2] *= q.z; v[3] *= q.w;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (k + e < k_end) v[e] *= sc[e];
          }
        }
      }
    }
    r[it] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

template <int BK>
__device__ __forceinline__ void tile_store(int mn_contig, const float4 (&r)[BK / 8],
                                           float (*S)[LDS_LD]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < BK / 8; ++it) {
    if (mn_contig) {
      const int kk = (tid >> 5) + 8 * it;
      *reinterpret_cast<float4*>(&S[kk][4 * (tid & 31)]) = r[it];
    } else {
      constexpr int QPR = BK / 4;
      const int e = tid + 256 * it;
      const int mn = e / QPR;
      const int kb = 4 * (e % QPR);
      S[kb + 0][mn] = r[it].x;
      S[kb + 1][mn] = r[it].y;
      S[kb + 2][mn] = r[it].z;
      S[kb + 3][mn] = r[it].w;
    }
  }
}

// ---- a wave's 64 x 64 share of the 128 x 128 tile: 2 x 2 MFMA tiles of 32 x 32, the same in the
//      three kernels of this file
__device__ __forceinline__ void acc_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// The bound-checked epilogue of the wave's share at (row0, col0): acc * unscale goes to split z of
// the partial sums or through the element epilogue to C.  C/D layout of the 32x32 MFMA:
// col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).
__device__ __forceinline__ void store_tiles_32x32(const f32x16 (&acc)[2][2], const Epilogue ep,
                                                  int M, int N, int row0, int col0, int z,
                                                  float unscale, int lane) {
  const int lcol = lane & 31, lhalf = lane >> 5;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = col0 + j * 32 + lcol;
      if (col >= N) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = row0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
        if (row >= M) continue;
        const float v = acc[i][j][e] * unscale;
        if (ep.partial) {
          ep.partial[((size_t)z * M + row) * N + col] = v;
        } else {
          float* dst = ep.C + (size_t)row * ep.ldc + col;
          *dst = ep_apply(ep, row, col, v, dst);
        }
      }
    }
}

template <int BK>
__global__ void __launch_bounds__(256)
gemm_f32_mfma_kernel(TileSrc A, TileSrc B, int M, int N, int K, int k_per_split,
                     Epilogue ep) {
  __shared__ __attribute__((aligned(16))) float As[2][BK][LDS_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDS_LD];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int k_begin = blockIdx.z * k_per_split;
  int k_end = k_begin + k_per_split;
  if (k_end > K) k_end = K;

  f32x16 acc[2][2];
  acc_zero(acc);

  float4 ra[BK / 8], rb[BK / 8];
  const int nk = (k_end - k_begin + BK - 1) / BK;
  if (nk > 0) {
    tile_load<BK>(A, k_begin, m0, k_end, ra);
    tile_load<BK>(B, k_begin, n0, k_end, rb);
    tile_store<BK>(A.mn_contig, ra, As[0]);
    tile_store<BK>(B.mn_contig, rb, Bs[0]);
  }
  __syncthreads();
  const int lrow = lane >> 5, lcol = lane & 31;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      tile_load<BK>(A, k_begin + (kt + 1) * BK, m0, k_end, ra);
      tile_load<BK>(B, k_begin + (kt + 1) * BK, n0, k_end, rb);
    }
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
      float a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = As[cur][2 * kk + lrow][wm * 64 + i * 32 + lcol];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = Bs[cur][2 * kk + lrow][wn * 64 + j * 32 + lcol];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) {
      tile_store<BK>(A.mn_contig, ra, As[cur ^ 1]);
      tile_store<BK>(B.mn_contig, rb, Bs[cur ^ 1]);
    }
    __syncthreads();
  }
  store_tiles_32x32(acc, ep, M, N, m0 + wm * 64, n0 + wn * 64, blockIdx.z, 1.f, lane);
}

__global__ void __launch_bounds__(256)
gemm_splitk_reduce_kernel(const float* __restrict__ partial, int splits, int M, int N,
                          Epilogue ep) {
  const size_t total = (size_t)M * N;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (size_t)gridDim.x * blockDim.x) {
    const int row = (int)(e / N), col = (int)(e % N);
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += partial[(size_t)s * total + e];
    float* dst = ep.C + (size_t)row * ep.ldc + col;
    *dst = ep_apply(ep, row, col, v, dst);
  }
}

// The same on whole 16-byte quads (N, ldc multiples of 4, 16-byte aligned arrays: every weight
// gradient of the step).  The scalar form keeps 4 bytes per load in flight and sat at 2.2 TB/s.
__global__ void __launch_bounds__(256)
gemm_splitk_reduce4_kernel(const float* __restrict__ partial, int splits, int M, int N,
                           Epilogue ep) {
  const size_t total4 = (size_t)M * N / 4;
  const float4* p4 = reinterpret_cast<const float4*>(partial);
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total4;
       q += (size_t)gridDim.x * blockDim.x) {
    const size_t e = q * 4;
    const int row = (int)(e / N), col = (int)(e % N);
    float4 v = p4[q];
    for (int s = 1; s < splits; ++s) {            // (fixed order: deterministic)
      const float4 t = p4[(size_t)s * total4 + q];
      v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
    }
    float4* dst = reinterpret_cast<float4*>(ep.C + (size_t)row * ep.ldc + col);
    *dst = ep_apply4(ep, row, col, v, dst);
  }
}

// ===========================================================================
// Split-fp16 GEMM: every fp32 operand element x is staged in LDS as
// hi = fp16(x*s), lo = fp16(x*s - hi) (s = per-tensor power of two that maps max|x|
// into [2^8, 2^9): 22 mantissa bits for elements within 2^-10 of the maximum, an
// absolute resolution of 2^-32 of the maximum below that -- fp16 subnormals are
// kept) and the product is accumulated in fp32 as hi*hi + hi*lo + lo*hi with three
// v_mfma_f32_32x32x16_f16 per K=16 slab instead of eight v_mfma_f32_32x32x2_f32:
// 16x the MFMA rate for 3x the MFMAs.  The dropped lo*lo term is 2^-22 relative.
// Tile 128x128x32, 4 waves (2x2, 64x64 each), both operands K-contiguous in LDS
// ([mn][32 + 8 pad] halfs -> conflict-free ds_read_b128), register prefetch of the
// next tile + double-buffered LDS, one barrier per K=32 step.
constexpr int HLD = HBK + 8;                 // halfs per LDS row (80 bytes)

// 16 fp32 values of one thread's share of a tile -> (hi, lo) halfs, [4 rows][4 k]
struct Frag16 { float v[4][4]; };   // v[r][c]: r = mn offset (0..3), c = k offset (0..3)

__device__ __forceinline__ void h_tile_load(const TileSrc& s, int k0, int mn0, int k_end,
                                            Frag16 (&f)[1]) {
  // mn-contiguous source: thread owns k rows 4kq..4kq+3 x mn 4mq..4mq+3
  // k-contiguous source:  thread owns mn rows r0 + {0,32,64,96}... see below
  const int tid = threadIdx.x;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) f[0].v[r][c] = 0.f;
  if (s.mn_contig) {
    const int kq = tid >> 5, mq = tid & 31;
    const int mn = mn0 + 4 * mq;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = k0 + 4 * kq + c;
      if (k < k_end) {
        const float* src = s.p + (size_t)k * s.ld + mn;
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        if (s.vec_ok && mn + 3 < s.mn_total) {
          const float4 q = *reinterpret_cast<const float4*>(src);
          t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (mn + e < s.mn_total) t[e] = src[e];
        }
        if (s.scale) {
          const float* sc = s.scale + (size_t)mod_period(k, s.period) * s.scale_ld + mn;
          if (s.scale_vec && mn + 3 < s.mn_total) {
            const float4 q = *reinterpret_cast<const float4*>(sc);
            t[0] *= q.x; t[1] *= q.y; t[2] *= q.z; t[3] *= q.w;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (mn + e < s.mn_total) t[e] *= sc[e];
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) f[0].v[r][c] = t[r];
      }
    }
  } else {
    // 128 rows x 8 k-quads = 1024 float4; thread takes rows (tid>>3) + 32*r, quad tid&7
    const int kq = tid & 7;
    const int k = k0 + 4 * kq;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int mn = mn0 + (tid >> 3) + 32 * r;
      if (mn < s.mn_total) {
        const float* src = s.p + (size_t)mn * s.ld + k;
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        if (s.vec_ok && k + 3 < k_end) {
          const float4 q = *reinterpret_cast<const float4*>(src);
          t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) if (k + e < k_end) t[e] = src[e];
        }
        if (s.scale) {
          const float* sc = s.scale + (size_t)mod_period(mn, s.period) * s.scale_ld + k;
          if (s.scale_vec && k + 3 < k_end) {
            const float4 q = *reinterpret_cast<const float4*>(sc);
            t[0] *= q.x; t[1] *= q.y; t[2] *= q.z; t[3] *= q.w;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) if (k + e < k_end) t[e] *= sc[e];
          }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) f[0].v[r][c] = t[c];
      }
    }
  }
}

// tile row (0..31) of a thread for a k-contiguous operand: the two rows that share a
// 16-lane ds_write_b64 group are 4 apart (80-byte rows -> banks 16 apart: no overlap)
__device__ __forceinline__ int kc_row() {
  const int rr = threadIdx.x >> 3;
  return (rr & ~7) | ((rr & 1) << 2) | ((rr >> 1) & 3);
}

__device__ __forceinline__ void h_tile_store(int mn_contig, const Frag16 (&f)[1], float scale,
                                             _Float16 (*Shi)[HLD], _Float16 (*Slo)[HLD],
                                             int kq = -1) {
  const int tid = threadIdx.x;
  const int krow = kq < 0 ? (tid >> 3) : kc_row();   // fast path passes kq >= 0
  if (kq < 0) kq = tid >> 5;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    hx4 hi, lo;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float x = f[0].v[r][c] * scale;
      const _Float16 h = (_Float16)x;
      hi[c] = h;
      lo[c] = (_Float16)(x - (float)h);
    }
    int row, col;
    if (mn_contig) { row = 4 * (tid & 31) + r; col = 4 * kq; }
    else { row = krow + 32 * r; col = 4 * (tid & 7); }
    *reinterpret_cast<hx4*>(&Shi[row][col]) = hi;
    *reinterpret_cast<hx4*>(&Slo[row][col]) = lo;
  }
}

// One K = 32 slab of the tile out of LDS, in two halves of 16: the wave's 2 x 2 fragments of both
// planes, then the three products of every accumulator (al*bh, ah*bl, ah*bh: the small cross terms
// first) in term-major order: consecutive MFMAs go to four different accumulators, so none waits
// for the previous one's result.
__device__ __forceinline__ void f16x2_slab(f32x16 (&am)[2][2], const _Float16 (*Ah)[HLD],
                                           const _Float16 (*Al)[HLD], const _Float16 (*Bh)[HLD],
                                           const _Float16 (*Bl)[HLD], int wm, int wn, int lane) {
  const int lrow = lane & 31, lk = 8 * (lane >> 5);
#pragma unroll
  for (int ks = 0; ks < HBK / 16; ++ks) {
    hx8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ah[i] = *reinterpret_cast<const hx8*>(&Ah[wm * 64 + i * 32 + lrow][16 * ks + lk]);
      al[i] = *reinterpret_cast<const hx8*>(&Al[wm * 64 + i * 32 + lrow][16 * ks + lk]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      bh[j] = *reinterpret_cast<const hx8*>(&Bh[wn * 64 + j * 32 + lrow][16 * ks + lk]);
      bl[j] = *reinterpret_cast<const hx8*>(&Bl[wn * 64 + j * 32 + lrow][16 * ks + lk]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        am[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], am[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        am[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], am[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        am[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], am[i][j], 0, 0, 0);
  }
}

struct HScales { const float* a_absmax; const float* b_absmax; };

__global__ void __launch_bounds__(256)
gemm_f16x2_kernel(TileSrc A, TileSrc B, int M, int N, int K, int k_per_split, Epilogue ep,
                  HScales hs) {
  extern __shared__ __attribute__((aligned(16))) _Float16 hsm[];
  // [buf 2][A_hi, A_lo, B_hi, B_lo][128][HLD]
  auto tile = [&](int buf, int which) {
    return reinterpret_cast<_Float16 (*)[HLD]>(hsm + ((size_t)(buf * 4 + which) * 128) * HLD);
  };
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int k_begin = blockIdx.z * k_per_split;
  int k_end = k_begin + k_per_split;
  if (k_end > K) k_end = K;
  const float sa = pow2_scale(hs.a_absmax), sb = pow2_scale(hs.b_absmax);

  f32x16 am[2][2];
  acc_zero(am);

  Frag16 fa[1], fb[1];
  const int nk = (k_end - k_begin + HBK - 1) / HBK;
  if (nk > 0) {
    h_tile_load(A, k_begin, m0, k_end, fa);
    h_tile_load(B, k_begin, n0, k_end, fb);
    h_tile_store(A.mn_contig, fa, sa, tile(0, 0), tile(0, 1));
    h_tile_store(B.mn_contig, fb, sb, tile(0, 2), tile(0, 3));
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      h_tile_load(A, k_begin + (kt + 1) * HBK, m0, k_end, fa);
      h_tile_load(B, k_begin + (kt + 1) * HBK, n0, k_end, fb);
    }
    f16x2_slab(am, tile(cur, 0), tile(cur, 1), tile(cur, 2), tile(cur, 3), wm, wn, lane);
    if (kt + 1 < nk) {
      h_tile_store(A.mn_contig, fa, sa, tile(cur ^ 1, 0), tile(cur ^ 1, 1));
      h_tile_store(B.mn_contig, fb, sb, tile(cur ^ 1, 2), tile(cur ^ 1, 3));
    }
    __syncthreads();
  }
  store_tiles_32x32(am, ep, M, N, m0 + wm * 64, n0 + wn * 64, blockIdx.z, 1.f / (sa * sb), lane);
}

// ---------------------------------------------------------------------------
// Fast path of the split-fp16 GEMM: the same tile / MFMA / LDS scheme with a
// BRANCH-FREE K loop.  All global reads are 16-byte buffer loads through a
// descriptor whose extent is the operand's; rows or K positions outside the problem
// get an out-of-range offset and come back as zeros, so the loop body is straight
// line code the compiler can software-pipeline (the generic kernel's per-element
// bound checks cost ~370 branches and ~110 waits per K slab).  Workgroups are mapped
// XCD-aware (see tile_of_block).  Preconditions (checked by the host, which otherwise
// falls back to the generic kernel): 16-byte aligned rows, K % 4 == 0, an
// mn-contiguous operand has mn % 4 == 0, extents < 4 GiB, mask period a power of two.
struct FastSrc {
  const float* p; int ld, mn_total;
  unsigned extent;                 // bytes addressable from p
  const float* scale; int pmask, scale_ld; unsigned scale_extent;
};

// k quad (0..7) of a thread for an mn-contiguous operand.  Rotating it with the column
// quad makes the 16 lanes that share a ds_write_b64 cycle hit 16 different bank pairs
// when they store their transposed 4x4 blocks ([mn][k] rows are 80 bytes apart, so
// unrotated lanes 4 rows apart collide 8-way); global reads stay 32-byte contiguous
// per lane pair and whole lines per workgroup.
__device__ __forceinline__ int mn_kquad() {
  const int tid = threadIdx.x;
  return ((tid >> 5) + ((tid & 31) >> 1)) & 7;
}

template <bool MN, bool MASK>
struct FastLoader {
  __amdgpu_buffer_rsrc_t rsrc, mrsrc;
  unsigned off[4], moff[4];        // byte offsets of this thread's four loads at k_begin
  unsigned step;                   // bytes per K slab
  int k0, k_end;                   // this thread's first K index, slab range end
  int pmask, scale_ld, mn;

  __device__ __forceinline__ void init(const FastSrc& s, int mn0, int k_begin, int kend) {
    const int tid = threadIdx.x;
    rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(s.p), 0, s.extent, 0x00020000);
    if (MASK)
      mrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(s.scale), 0, s.scale_extent,
                                                0x00020000);
    k_end = kend;
    pmask = s.pmask; scale_ld = s.scale_ld;
    if (MN) {        // storage (K, MN): thread = k rows 4*kq+c, columns 4*(tid&31)..+3
      k0 = k_begin + 4 * mn_kquad();
      mn = mn0 + 4 * (tid & 31);
      const bool ok = mn + 3 < s.mn_total;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        off[c] = ok ? (unsigned)(((size_t)(k0 + c) * s.ld + mn) * 4) : kOob;
      step = (unsigned)(HBK * s.ld * 4);
    } else {         // storage (MN, K): thread = rows kc_row()+32r, k quad tid&7
      k0 = k_begin + 4 * (tid & 7);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mn0 + kc_row() + 32 * r;
        off[r] = row < s.mn_total ? (unsigned)(((size_t)row * s.ld + k0) * 4) : kOob;
        if (MASK) moff[r] = (unsigned)(((size_t)(row & s.pmask) * s.scale_ld + k0) * 4);
      }
      step = (unsigned)(HBK * 4);
    }
  }

  // Issues the loads only; the mask (if any) lands in fm and is applied by apply_mask()
  // right before the values are needed, so nothing here waits on memory.
  __device__ __forceinline__ void load(int kt, Frag16 (&f)[1], Frag16 (&fm)[1]) const {
    float4 q[4], m[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + kt * HBK + (MN ? i : 0);
      const bool ok = k < k_end && off[i] != kOob;
      const unsigned o = ok ? off[i] + (unsigned)kt * step : kOob;
      q[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, 0, 0));
      if (MASK) {
        const unsigned mraw = MN ? (unsigned)(((size_t)(k & pmask) * scale_ld + mn) * 4)
                                 : moff[i] + (unsigned)kt * step;
        const unsigned mo = ok ? mraw : kOob;
        m[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(mrsrc, mo, 0, 0));
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (MN) {      // load i = k row c: element e belongs to tile row e
        f[0].v[0][i] = q[i].x; f[0].v[1][i] = q[i].y; f[0].v[2][i] = q[i].z; f[0].v[3][i] = q[i].w;
        if (MASK) {
          fm[0].v[0][i] = m[i].x; fm[0].v[1][i] = m[i].y; fm[0].v[2][i] = m[i].z;
          fm[0].v[3][i] = m[i].w;
        }
      } else {       // load i = tile row r: elements are 4 consecutive k
        f[0].v[i][0] = q[i].x; f[0].v[i][1] = q[i].y; f[0].v[i][2] = q[i].z; f[0].v[i][3] = q[i].w;
        if (MASK) {
          fm[0].v[i][0] = m[i].x; fm[0].v[i][1] = m[i].y; fm[0].v[i][2] = m[i].z;
          fm[0].v[i][3] = m[i].w;
        }
      }
    }
  }
  __device__ __forceinline__ static void apply_mask(Frag16 (&f)[1], const Frag16 (&fm)[1]) {
    if (!MASK) return;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) f[0].v[r][c] *= fm[0].v[r][c];
  }
};

// (The kernel keeps its own text of the slab and of the edge epilogue, the same as f16x2_slab and
// store_tiles_32x32: through the shared functions the compiler scheduled its K loop differently
// and the cfg3 x@W shape timed 1.2 % slower, outside the run-to-run spread.)
// NBUF = 2: double-buffered LDS (80 KB: 2 workgroups per CU, one barrier per slab);
// NBUF = 1: one LDS buffer (40 KB: 4 workgroups per CU, two barriers per slab).
template <bool AMN, bool BMN, bool MASK, int NBUF>
__global__ void __launch_bounds__(256)
gemm_f16x2_fast_kernel(FastSrc A, FastSrc B, int M, int N, int K, int k_per_split, int splits,
                       Epilogue ep, HScales hs) {
  extern __shared__ __attribute__((aligned(16))) _Float16 hsm[];
  // [buf 2][A_hi, A_lo, B_hi, B_lo][128][HLD]
  auto tile = [&](int buf, int which) {
    return reinterpret_cast<_Float16 (*)[HLD]>(hsm + ((size_t)(buf * 4 + which) * 128) * HLD);
  };
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const TileId tb = tile_of_block((M + BM - 1) / BM, (N + BN - 1) / BN, splits);
  const int m0 = tb.tm * BM, n0 = tb.tn * BN;
  const int k_begin = tb.z * k_per_split;
  int k_end = k_begin + k_per_split;
  if (k_end > K) k_end = K;
  const float sa = pow2_scale(hs.a_absmax), sb = pow2_scale(hs.b_absmax);

  f32x16 am[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) am[i][j][e] = 0.f;

  const int kq_rot = mn_kquad();
  FastLoader<AMN, MASK> la;
  FastLoader<BMN, false> lb;
  la.init(A, m0, k_begin, k_end);
  lb.init(B, n0, k_begin, k_end);
  // Two register sets: while slab kt is multiplied out of LDS, slab kt+1 (loaded one
  // iteration ago) is converted into the other LDS buffer and the loads of slab kt+2
  // are already in flight -- a full iteration of latency cover.
  Frag16 fa0[1], fb0[1], fa1[1], fb1[1], fm0[1], fm1[1], fmb[1];
  const int nk = (k_end - k_begin + HBK - 1) / HBK;
  la.load(0, fa0, fm0);
  lb.load(0, fb0, fmb);
  la.load(1, fa1, fm1);
  lb.load(1, fb1, fmb);
  la.apply_mask(fa0, fm0);
  h_tile_store(AMN, fa0, sa, tile(0, 0), tile(0, 1), kq_rot);
  h_tile_store(BMN, fb0, sb, tile(0, 2), tile(0, 3), kq_rot);
  __syncthreads();
  const int lrow = lane & 31, lk = 8 * (lane >> 5);
  auto slab = [&](int kt, Frag16 (&fl_a)[1], Frag16 (&fl_m)[1], Frag16 (&fl_b)[1],
                  Frag16 (&fs_a)[1], Frag16 (&fs_m)[1], Frag16 (&fs_b)[1]) {
    const int cur = NBUF == 2 ? (kt & 1) : 0;
    const int nxt = NBUF == 2 ? (cur ^ 1) : 0;
    // past the last slab every offset is out of range: those loads return zeros, unused
    la.load(kt + 2, fl_a, fl_m);
    lb.load(kt + 2, fl_b, fmb);
    _Float16 (*Ah)[HLD] = tile(cur, 0);
    _Float16 (*Al)[HLD] = tile(cur, 1);
    _Float16 (*Bh)[HLD] = tile(cur, 2);
    _Float16 (*Bl)[HLD] = tile(cur, 3);
#pragma unroll
    for (int ks = 0; ks < HBK / 16; ++ks) {
      hx8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ah[i] = *reinterpret_cast<const hx8*>(&Ah[wm * 64 + i * 32 + lrow][16 * ks + lk]);
        al[i] = *reinterpret_cast<const hx8*>(&Al[wm * 64 + i * 32 + lrow][16 * ks + lk]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        bh[j] = *reinterpret_cast<const hx8*>(&Bh[wn * 64 + j * 32 + lrow][16 * ks + lk]);
        bl[j] = *reinterpret_cast<const hx8*>(&Bl[wn * 64 + j * 32 + lrow][16 * ks + lk]);
      }
      // term-major order: consecutive MFMAs go to four different accumulators, so none
      // waits for the previous one's result (the small cross terms first)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          am[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], am[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          am[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], am[i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          am[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], am[i][j], 0, 0, 0);
    }
    la.apply_mask(fs_a, fs_m);
    if (NBUF == 1) __syncthreads();          // every wave has read the slab
    h_tile_store(AMN, fs_a, sa, tile(nxt, 0), tile(nxt, 1), kq_rot);
    h_tile_store(BMN, fs_b, sb, tile(nxt, 2), tile(nxt, 3), kq_rot);
    __syncthreads();
  };
  for (int kt = 0; kt < nk; kt += 2) {
    slab(kt, fa0, fm0, fb0, fa1, fm1, fb1);     // loads slab kt+2 -> set 0, stores set 1
    if (kt + 1 < nk) slab(kt + 1, fa1, fm1, fb1, fa0, fm0, fb0);
  }
  const float unscale = 1.f / (sa * sb);
  const int lcol = lane & 31, lhalf = lane >> 5;
  if (m0 + BM <= M && n0 + BN <= N) {
    // interior tile: no per-element bound checks, so the 16 loads of a fragment (mask,
    // old C) are issued back to back before the first is needed
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 64 + j * 32 + lcol;
        const int row0 = m0 + wm * 64 + i * 32 + 4 * lhalf;
        if (ep.partial) {
          float* dst = ep.partial + ((size_t)tb.z * M + row0) * N + col;
#pragma unroll
          for (int e = 0; e < 16; ++e)
            dst[(size_t)((e & 3) + 8 * (e >> 2)) * N] = am[i][j][e] * unscale;
          continue;
        }
        float* dst = ep.C + (size_t)row0 * ep.ldc + col;
        const float bias = ep.bias ? ep.bias[col] : 0.f;
        float old[16], msk[16];
        const bool use_old = ep.beta != 0.f;
        const bool use_msk = ep.c_scale != nullptr;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int dr = (e & 3) + 8 * (e >> 2);
          old[e] = use_old ? dst[(size_t)dr * ep.ldc] : 0.f;
          msk[e] = use_msk ? ep.c_scale[(size_t)mod_period(row0 + dr, ep.c_period) * ep.c_ld + col]
                           : 1.f;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int dr = (e & 3) + 8 * (e >> 2);
          const float v = (am[i][j][e] * unscale * ep.alpha + bias) * msk[e];
          dst[(size_t)dr * ep.ldc] = use_old ? v + ep.beta * old[e] : v;
        }
      }
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 64 + j * 32 + lcol;
      if (col >= N) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lhalf;
        if (row >= M) continue;
        float v = am[i][j][e] * unscale;
        if (ep.partial) {
          ep.partial[((size_t)tb.z * M + row) * N + col] = v;
        } else {
          v *= ep.alpha;
          float* dst = ep.C + (size_t)row * ep.ldc + col;
          if (ep.bias) v += ep.bias[col];
          if (ep.c_scale) v *= ep.c_scale[(size_t)mod_period(row, ep.c_period) * ep.c_ld + col];
          if (ep.beta != 0.f) v += ep.beta * *dst;
          *dst = v;
        }
      }
    }
}

}  // namespace

void launch_splitk_reduce(const float* partial, int splits, int M, int N, Epilogue ep,
                          hipStream_t stream) {
  ep.partial = nullptr;
  const size_t total = (size_t)M * N;
  const bool quads = (N & 3) == 0 && (ep.ldc & 3) == 0 && aligned16(ep.C) && aligned16(partial);
  const size_t items = quads ? total / 4 : total;
  int blocks = (int)((items + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  auto kernel = quads ? gemm_splitk_reduce4_kernel : gemm_splitk_reduce_kernel;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds_ballast((const void*)kernel), stream,
                     partial, splits, M, N, ep);
}

extern "C" size_t asr_gemm_workspace_bytes(const asr_gemm_args* a) {
  if (!a || a->split_k <= 1) return 0;
  return asr_align_up((size_t)a->split_k * a->M * a->N * sizeof(float), 256);
}

extern "C" int asr_gemm(const asr_gemm_args* a, void* workspace, size_t ws_bytes,
                        asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(a && a->A && a->B && a->C, "gemm: null pointer");
  ASR_CHECK_ARG(a->M > 0 && a->N > 0 && a->K >= 0, "gemm: bad shape %d %d %d", a->M, a->N, a->K);
  TileSrc A, B;
  A.p = a->A; A.ld = a->lda; A.mn_contig = a->trans_a ? 1 : 0;
  A.mn_total = a->M; A.k_total = a->K;
  A.scale = a->a_scale; A.period = a->a_scale_period > 0 ? a->a_scale_period : 1;
  A.scale_ld = a->a_scale_ld;
  A.scale_vec = a->a_scale && (a->a_scale_ld % 4 == 0) && aligned16(a->a_scale);
  A.vec_ok = (a->lda % 4 == 0) && aligned16(a->A);
  B.p = a->B; B.ld = a->ldb; B.mn_contig = a->trans_b ? 0 : 1;
  B.mn_total = a->N; B.k_total = a->K;
  B.scale = nullptr; B.period = 1; B.scale_ld = 0; B.scale_vec = 0;
  B.vec_ok = (a->ldb % 4 == 0) && aligned16(a->B);
  ASR_CHECK_ARG(a->lda >= (a->trans_a ? a->M : a->K), "gemm: lda too small");
  ASR_CHECK_ARG(a->ldb >= (a->trans_b ? a->K : a->N), "gemm: ldb too small");
  ASR_CHECK_ARG(a->ldc >= a->N, "gemm: ldc too small");
  static const int prec_env = [] { const char* v = getenv("ASR_GEMM_PREC"); return v ? atoi(v) : 1; }();
  const int prec = a->precision == 0 ? 0 : (a->precision == 1 ? 1 : prec_env);
  const bool f16 = prec == 1 && a->K >= 32;    // split-fp16 path: K slabs of 32; exact fp32: of 16
  int kps = 0;
  const int splits = split_plan(a->K, a->split_k, f16 ? HBK : 16, &kps);
  Epilogue ep = make_epilogue(a);
  if (int rc = splitk_workspace("gemm", splits, a->M, a->N, workspace, ws_bytes, &ep)) return rc;
  const dim3 grid((a->N + BN - 1) / BN, (a->M + BM - 1) / BM, splits);
  if (f16) {
    const size_t shm = (size_t)2 * 4 * 128 * HLD * sizeof(_Float16);
    HScales hs{a->a_absmax, a->b_absmax};
    // fast (branch-free) kernel when the geometry allows 16-byte buffer loads throughout
    auto extent = [](const TileSrc& t) {
      return t.mn_contig ? ((size_t)(t.k_total - 1) * t.ld + t.mn_total) * 4
                         : ((size_t)(t.mn_total - 1) * t.ld + t.k_total) * 4;
    };
    const size_t lim = ((size_t)1 << 32) - ((size_t)1 << 20);
    const bool pow2 = (A.period & (A.period - 1)) == 0;
    const size_t mask_ext = A.scale ? ((size_t)(A.period - 1) * A.scale_ld +
                                       (A.mn_contig ? A.mn_total : A.k_total)) * 4 : 0;
    const bool fast = A.vec_ok && B.vec_ok && a->K % 4 == 0 &&
                      (!A.mn_contig || a->M % 4 == 0) && (!B.mn_contig || a->N % 4 == 0) &&
                      extent(A) < lim && extent(B) < lim &&
                      (!A.scale || (A.scale_vec && pow2 && mask_ext < lim));
    if (fast) {
      FastSrc fa_, fb_;
      fa_.p = A.p; fa_.ld = A.ld; fa_.mn_total = A.mn_total; fa_.extent = (unsigned)extent(A);
      fa_.scale = A.scale; fa_.pmask = A.period - 1; fa_.scale_ld = A.scale_ld;
      fa_.scale_extent = (unsigned)mask_ext;
      fb_.p = B.p; fb_.ld = B.ld; fb_.mn_total = B.mn_total; fb_.extent = (unsigned)extent(B);
      fb_.scale = nullptr; fb_.pmask = 0; fb_.scale_ld = 0; fb_.scale_extent = 0;
      // kernel variants: [A mn-contiguous][B mn-contiguous][A masked]
      typedef void (*fast_t)(FastSrc, FastSrc, int, int, int, int, int, Epilogue, HScales);
      static const fast_t kern[2][2][2] = {
          {{gemm_f16x2_fast_kernel<false, false, false, 2>, gemm_f16x2_fast_kernel<false, false, true, 2>},
           {gemm_f16x2_fast_kernel<false, true, false, 2>, gemm_f16x2_fast_kernel<false, true, true, 2>}},
          {{gemm_f16x2_fast_kernel<true, false, false, 2>, gemm_f16x2_fast_kernel<true, false, true, 2>},
           {gemm_f16x2_fast_kernel<true, true, false, 2>, gemm_f16x2_fast_kernel<true, true, true, 2>}}};
      const fast_t k = kern[A.mn_contig][B.mn_contig][A.scale ? 1 : 0];
      ASR_CHECK_HIP(set_dynamic_lds_once((const void*)k, shm));
      hipLaunchKernelGGL(k, dim3(grid.x * grid.y * splits), dim3(256), shm, stream, fa_, fb_, a->M,
                         a->N, a->K, kps, splits, ep, hs);
    } else {
      ASR_CHECK_HIP(set_dynamic_lds_once((const void*)gemm_f16x2_kernel, shm));
      hipLaunchKernelGGL(gemm_f16x2_kernel, grid, dim3(256), shm, stream, A, B, a->M, a->N, a->K,
                         kps, ep, hs);
    }
  } else
    hipLaunchKernelGGL(gemm_f32_mfma_kernel<16>, grid, dim3(256), 0, stream, A, B, a->M, a->N,
                       a->K, kps, ep);
  ASR_CHECK_LAUNCH();
  if (splits > 1) {
    launch_splitk_reduce(ep.partial, splits, a->M, a->N, ep, stream);
    ASR_CHECK_LAUNCH();
  }
  return ASR_OK;
}
