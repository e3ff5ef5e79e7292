// asr_gemm_hl: the split-fp16 GEMM on PACKED planes -- gemm_hlx_kernel (row-major, k-major and
// segmented forms, two tiles), the DMA-staged k-major big tile gemm_hlt_dma_kernel and the
// persistent row-major form gemm_hlp_kernel.  asr_pack_hl
// (pack.hip) makes the planes; the split-K partials are reduced by gemm.hip's kernels.
//
// ===========================================================================
// Packed split-fp16 operands ("hl" planes): convert once, multiply many times.
//
// gemm_f16x2_fast_kernel splits every fp32 element into hi/lo halfs INSIDE its K loop
// (~140 VALU per 24 MFMAs and slab), and a tile of an operand is re-read -- and re-split --
// by every workgroup of its row / column band (a dz element ~20 times per step).  Here the
// split happens once per tensor: pack_hl_kernel writes two fp16 planes hi = fp16(x*s),
// lo = fp16(x*s - hi) (s = the per-tensor power of two of pow2_scale; variational-dropout
// masks are multiplied in BEFORE the split, in fp32, so the GEMM needs no mask path) with the
// source's columns ("r" planes: (rows, ldk_r)) or rows ("c" planes: (cols, ldk_c)) contiguous:
//   x, y (.) B_U, dz: "r" planes only.  x@W and dz@W^T reduce over their columns (row-major
//     form of the GEMM); the weight gradients x^T dz and h^T dz reduce over their ROWS and read
//     the same planes transposed out of LDS (k_major form, HlLoaderT) -- the second
//     orientation was a third of the pack passes' bytes;
//   W: both ("c" = the B operand of x@W, "r" = the B operand of dz@W^T).
// A plane row holds ldk reduction indices (ldk % 32 == 0, zero padded).  The two planes are ONE
// array, interleaved in groups of 16 indices: a row is 2 ldk halfs,
//   half [32 g, 32 g + 16)      = hi[16 g .. 16 g + 15]
//   half [32 g + 16, 32 g + 32) = lo[16 g .. 16 g + 15]
// so the 32-deep K slab of a row -- both planes -- is ONE 128-byte line.  (With separate
// planes a slab touched half of a line in each, the other halves belonging to the next slab,
// by which time the 32 KB L1 had long turned over: every line crossed L2 -> L1 twice.)  A
// reduction offset is a multiple of 16 (a group).  gemm_hlx_kernel is then a
// plain fp16 GEMM with three MFMAs per fragment pair and fp32 accumulation: 16-byte global
// loads -> ds_write_b128 -> ds_read_b128 (ds_read_b64_tr_b16 in the k_major form) ->
// v_mfma_f32_16x16x32_f16, no VALU in the K loop besides addresses.
#include "gemm_common.h"
#include <atomic>
#include <mutex>

namespace {

struct HlSrc {
  const _Float16* p;      // interleaved planes, offset to (first row, first reduction group)
  int ld;                 // plane columns per row: a row is 2 ld halfs (hi and lo)
  int rows;               // MN extent (plane rows in the row-major form, columns in k_major)
  unsigned extent;        // bytes addressable from p
};
// Segmented reduction range of the row-major A operand (asr_gemm_hl_args.a_seg_k): the K range
// is the concatenation of segments of seg_k indices (a multiple of 32: whole slabs), segment i
// read from the planes shifted by a byte offset -- the implicit im2col over time of
// asr_conv2d_*: tap dt of a filter reads the activation planes dt frames further on.  The
// loader adds adj[slab / slabs_per_segment] (= the segment's byte shift minus the bytes the
// running reduction offset has advanced by then) to its offset; slab / sps is a multiply-shift
// with a magic the host verified over the launch's slab range.  magic = 0: no segments.
struct HlSeg {
  unsigned magic;
  unsigned batch;          // k_major only: > 1 = a batch of GEMMs sharing B (asr_gemm_hl_args.batch):
  unsigned adj[16];        //   adj[b] = byte offset of A_b; else the segments' offset corrections
};

// ---------------------------------------------------------------------------
// The packed-plane kernel.  256 x 256 x 32 tile by default (outputs of at least 256 x 256).
// With 128 x 128 tiles both split-fp16 GEMMs sit at ~250 TF/s algorithmic whatever the K loop
// costs: a workgroup moves 32 KB from L2 per 1 MFLOP (32 flop/B), i.e. ~7.5 TB/s at that
// rate, with an L2 hit rate of ~72 % -- the loop is fed at the L2 / fabric rate.  A 256 x 256
// tile halves the bytes per flop.  512 threads = 8 waves (2 x 4, 128 x 64 each = 8 x 4 MFMA
// tiles of 16 x 16, 128 accumulator registers); LDS image per plane [256 rows][32 halfs]
// (64-byte rows; 4 planes x 2 buffers = 128 KB) with the 16-byte chunk index XOR-swizzled by a
// permutation of (row >> 2) & 3, which makes both the ds_write_b128 of the staging pass and the
// ds_read_b128 of the 16 x 32 fragments bank-conflict free (lane groups of
// MI355X_MICROARCH.md "LDS"; checked exhaustively when the layout was chosen).
//
// The kernel runs at the 1400 W package power cap (tools/clock_probe.py): what it sustains is
// set by energy per flop, not by issue slots.  v_mfma_f32_16x16x32_f16 sustains 2.0 PFLOP/s on
// random operands at the cap (shader clock 2.04 GHz) where v_mfma_f32_32x32x16_f16 sustains
// 1.66 (1.80 GHz) -- tools/micro/mfma_power.hip -- so the tile is built from the 16 x 16 shape.

__device__ __forceinline__ int hl256_slot(int row, int kc) {      // half index in a plane
  return row * 32 + ((kc ^ ((0x78 >> (2 * ((row >> 2) & 3))) & 3)) << 3);    // 0, 2, 3, 1
}

template <int NT, bool SEG = false>
struct HlLoaderX {
  // One operand's share of a K slab: (NT / 2) rows x 128 bytes (the row's line: hi and lo of 32
  // reduction indices) = 4 NT 16-byte chunks; thread t takes chunks t + NT i, i < 4: row
  // (t >> 3) + (NT / 8) i, chunk t & 7 of the line -- a wave instruction reads 8 whole lines.
  // Chunk c of a line is reduction chunk 2 (c >> 2) + (c & 1) of plane (c >> 1) & 1.  One
  // offset register: the four rows are a uniform stride apart (scalar offset operand, which
  // the descriptor's range check does not see: rows past the operand and the reduction tail
  // are compares that send the lane's offset out of range -> zeros).
  __amdgpu_buffer_rsrc_t rs;
  unsigned off;            // bytes: (row0 + t >> 3, first reduction group) + 16 (t & 7)
  unsigned row_step;       // bytes between the thread's consecutive chunks: NT / 8 rows
  int kq;                  // first reduction index of the thread's chunk within a slab
  int depth;               // reduction indices from the first slab on
  int rows_left;           // operand rows from the thread's first one on
  int g0;                  // index of the first slab (kb / 32): segments count from k = 0
  const HlSeg* sg;         // segmented reduction range (kernel argument), or its magic is 0
  __device__ __forceinline__ void init(const HlSrc& s, int row0, int kb, int ke,
                                       const HlSeg* seg = nullptr) {
    const int tid = threadIdx.x;
    rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(s.p), 0, s.extent, 0x00020000);
    const int c = tid & 7;
    kq = 16 * (c >> 2) + 8 * (c & 1);
    depth = ke - kb;
    rows_left = s.rows - row0 - (tid >> 3);
    off = (unsigned)((hl_index(row0 + (tid >> 3), kb, s.ld) + 8 * c) * 2);
    row_step = (unsigned)(NT / 8) * (unsigned)s.ld * 4u;
    g0 = kb / HBK;
    sg = seg;
  }
  // (the address arithmetic apart from the loads: VALU at the head of an MFMA phase is slow)
  __device__ __forceinline__ void offsets(int kt, unsigned (&o)[4]) const {
    unsigned base = off + (unsigned)(kt * HBK * 4);
    if constexpr (SEG)                         // uniform: scalar multiply-shift + one scalar load
      base += sg->adj[((unsigned)(g0 + kt) * sg->magic) >> 20];
    const unsigned ok = kt * HBK + kq < depth ? base : kOob;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = i * (NT / 8) < rows_left ? ok : kOob;
  }
  __device__ __forceinline__ void issue(const unsigned (&o)[4], u32x4g (&v)[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, o[i], i * row_step, 0);
  }
  __device__ __forceinline__ void load(int kt, u32x4g (&v)[4]) const {
    unsigned o[4];
    offsets(kt, o);
    issue(o, v);
  }
  __device__ __forceinline__ static void store(const u32x4g (&v)[4], _Float16* Shi, _Float16* Slo) {
    const int tid = threadIdx.x;
    const int c = tid & 7;
    _Float16* dst = ((c >> 1) & 1 ? Slo : Shi) + hl256_slot(tid >> 3, 2 * (c >> 2) + (c & 1));
#pragma unroll
    for (int i = 0; i < 4; ++i)       // + NT / 8 rows: the same swizzle (NT / 8 is a multiple of 16)
      *reinterpret_cast<u32x4g*>(dst + i * (NT / 8) * 32) = v[i];
  }
};

// K-MAJOR operands (asr_gemm_hl_args.k_major): the weight gradients x^T dz and h^T dz reduce over
// the ROWS of their operands, i.e. they can read the same (rows, cols) planes as x@W and
// dz@W^T if the fragments are transposed on the way out of LDS -- ds_read_b64_tr_b16 -- and the
// second orientation of x, y and dz is never packed (a third of the pack passes' bytes).
// A slab is 32 plane rows (reduction indices) x TM2 columns: per row TM2 / 16 groups of
// (16 hi, 16 lo) = 4 TM2 contiguous bytes; a wave's load instruction reads one whole row.
// LDS image per operand: one SUBTILE per (column group, plane): [32 k][16 columns] halfs,
// 32-byte rows, 1 KB, the layout ds_read_b64_tr_b16 reads conflict-free (guide T10): lane
// l = 16 g + c of a read at byte 8 l receives column c of rows 4 g .. 4 g + 3.  Two reads (rows
// 0..15, rows 16..31) give a lane the reduction indices {4 g .., 16 + 4 g ..}: a permutation of
// the MFMA's k order that both operands share, so the products are unchanged.  Subtiles are
// 1056 bytes apart: the 8 lanes of a staging ds_write_b128 group hold 4 subtiles x 2 halves of
// one row, and 32-byte steps spread them over all banks.
constexpr int kSubtile = 1056;                       // bytes
template <int NT>
struct HlLoaderT {
  static constexpr int CPR = NT / 8;                 // 16-byte chunks per slab row (tile / 4)
  __amdgpu_buffer_rsrc_t rs;
  unsigned off;            // bytes: (first row + t / CPR, tile's first column group) + 16 (t % CPR)
  unsigned row_step;       // bytes between the thread's consecutive chunks: 8 rows
  unsigned slab_step;      // bytes per slab: 32 rows
  int rows_left;           // reduction rows from the thread's first one on (slab 0)
  __device__ __forceinline__ void init(const HlSrc& s, int col0, int kb, int ke) {
    const int tid = threadIdx.x;
    rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(s.p), 0, s.extent, 0x00020000);
    const unsigned pitch = (unsigned)s.ld * 4u;      // bytes per plane row (hi + lo)
    const int r = tid / CPR, c = tid % CPR;
    rows_left = ke - kb - r;
    // (column groups past the operand's M / N extent: out of range -> zeros; the last group
    // may hold columns past it, which feed only output rows / columns that are never stored)
    const bool col_ok = col0 + 16 * (c >> 2) < ((s.rows + 15) & ~15);
    off = col_ok ? (unsigned)(kb + r) * pitch + (unsigned)col0 * 4u + 16u * c : kOob;
    row_step = 8u * pitch;
    slab_step = 32u * pitch;
  }
  __device__ __forceinline__ void offsets(int kt, unsigned (&o)[4]) const {
    const unsigned ok = off == kOob ? kOob : off + (unsigned)kt * slab_step;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = kt * HBK + 8 * i < rows_left ? ok : kOob;
  }
  __device__ __forceinline__ void issue(const unsigned (&o)[4], u32x4g (&v)[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      v[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, o[i], i * row_step, 0);
  }
  __device__ __forceinline__ void load(int kt, u32x4g (&v)[4]) const {
    unsigned o[4];
    offsets(kt, o);
    issue(o, v);
  }
  // chunk c of row r: column group c >> 2, plane (c >> 1) & 1 -> subtile c >> 1, its half c & 1
  __device__ __forceinline__ static void store(const u32x4g (&v)[4], char* image) {
    const int tid = threadIdx.x;
    const int r = tid / CPR, c = tid % CPR;
    char* dst = image + (c >> 1) * kSubtile + r * 32 + (c & 1) * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4g*>(dst + i * 256) = v[i];
  }
  // the 16 (columns of group `grp`) x 32 (k) fragment of one plane as the MFMA wants it
  __device__ __forceinline__ static hx8 fragment(const char* image, int grp, int plane, int lane) {
    typedef short s4 __attribute__((__vector_size__(4 * sizeof(short))));
    const char* q = image + (grp * 2 + plane) * kSubtile + lane * 8;
    const s4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s4*)(q));
    const s4 t2 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s4*)(q + 512));
    const hx4 a = __builtin_bit_cast(hx4, t1), b = __builtin_bit_cast(hx4, t2);
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  }
};

// The epilogue of one output tile of gemm_hlx_kernel / gemm_hlp_kernel: lane = (row frow of a
// 16 x 16 tile, its columns 4 fk .. 4 fk + 3); z = the split (partial sums) the tile belongs to.
template <int MI, int NJ, bool SEG>
__device__ __forceinline__ void hlx_epilogue(const f32x4 (&am)[2 * MI][2 * NJ], const Epilogue ep,
                                             int M, int N, int m0, int n0, int z, float unscale,
                                             int wm, int wn, int frow, int fk, int TM2, int TN2) {
  constexpr int RB = 2 * MI, CB = 2 * NJ;
  const int row_w = m0 + wm * (32 * MI) + frow;      // + 16 i
  const int col_w = n0 + wn * (32 * NJ) + 4 * fk;    // + 16 j
  const bool interior = m0 + TM2 <= M && n0 + TN2 <= N;
  // 16-byte stores need 16-byte aligned rows
  const bool vec_c = (ep.ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(ep.C) & 15) == 0;
  // The epilogue is 1/5 of a K = 1024 tile if it is written element by element with its
  // options tested inside (hipcc branches around every optional load and waits for it): the
  // variants are separated OUTSIDE the element loops, the interior ones are straight-line code.
  if (interior && ep.partial && (N & 3) == 0) {                 // split-K partial sums
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        float* dst = ep.partial + ((size_t)z * M + row_w + 16 * i) * N + col_w + 16 * j;
        *reinterpret_cast<f32x4*>(dst) = am[i][j] * unscale;
      }
    return;
  }
  const bool use_old = ep.beta != 0.f;
  const bool use_msk = ep.c_scale != nullptr;
  if (interior && !ep.partial && vec_c && !use_old && !use_msk) {      // C = alpha A B^T + bias
    const float sc = unscale * ep.alpha;
    f32x4 bias[CB];
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      bias[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ep.bias)
#pragma unroll
        for (int e = 0; e < 4; ++e) bias[j][e] = ep.bias[col_w + 16 * j + e];
    }
    if constexpr (SEG) {
      if (ep.clamp_hi > 0.f) {          // the convolution's clipped ReLU, fused
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
          for (int j = 0; j < CB; ++j) {
            float* dst = ep.C + (size_t)(row_w + 16 * i) * ep.ldc + col_w + 16 * j;
            f32x4 v = am[i][j] * sc + bias[j];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fminf(fmaxf(v[e], 0.f), ep.clamp_hi);
            *reinterpret_cast<f32x4*>(dst) = v;
          }
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        float* dst = ep.C + (size_t)(row_w + 16 * i) * ep.ldc + col_w + 16 * j;
        *reinterpret_cast<f32x4*>(dst) = am[i][j] * sc + bias[j];
      }
    return;
  }
  const bool vec_m = !use_msk || ((ep.c_ld & 3) == 0 && (reinterpret_cast<uintptr_t>(ep.c_scale) & 15) == 0);
  if (interior && !ep.partial && vec_c && vec_m) {   // with old C and / or a row mask: loads first
#pragma unroll
    for (int i = 0; i < RB; ++i) {
      const int row = row_w + 16 * i;
      f32x4 old[CB], msk[CB];
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        old[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        msk[j] = f32x4{1.f, 1.f, 1.f, 1.f};
      }
      if (use_old) {
#pragma unroll
        for (int j = 0; j < CB; ++j)
          old[j] = *reinterpret_cast<const f32x4*>(ep.C + (size_t)row * ep.ldc + col_w + 16 * j);
      }
      if (use_msk) {
        const float* mrow = ep.c_scale + (size_t)mod_period(row, ep.c_period) * ep.c_ld;
#pragma unroll
        for (int j = 0; j < CB; ++j)
          msk[j] = *reinterpret_cast<const f32x4*>(mrow + col_w + 16 * j);
      }
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        f32x4 bias = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ep.bias)
#pragma unroll
          for (int e = 0; e < 4; ++e) bias[e] = ep.bias[col_w + 16 * j + e];
        float* dst = ep.C + (size_t)row * ep.ldc + col_w + 16 * j;
        *reinterpret_cast<f32x4*>(dst) = (am[i][j] * (unscale * ep.alpha) + bias) * msk[j] + ep.beta * old[j];
      }
    }
    return;
  }
  // edge tiles (and unaligned outputs): per-element bound checks
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int row = row_w + 16 * i;
      if (row >= M) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = col_w + 16 * j + e;
        if (col >= N) continue;
        if (ep.partial) {
          ep.partial[((size_t)z * M + row) * N + col] = am[i][j][e] * unscale;
          continue;
        }
        // (not ep_apply: this form contracts to one fused multiply-add with the bias, ep_apply's
        // rounds the product first -- sharing it would change result bits)
        float* dst = ep.C + (size_t)row * ep.ldc + col;
        float v = am[i][j][e] * unscale * ep.alpha + (ep.bias ? ep.bias[col] : 0.f);
        if (use_msk) v *= ep.c_scale[(size_t)mod_period(row, ep.c_period) * ep.c_ld + col];
        if (use_old) v += ep.beta * *dst;
        if constexpr (SEG) {
          if (ep.clamp_hi > 0.f) v = fminf(fmaxf(v, 0.f), ep.clamp_hi);
        }
        *dst = v;
      }
    }
}

// One half-step (hf = 0, 1) of the ping-pong K loop of gemm_hlx_kernel and gemm_hlp_kernel: read the
// fragments of half of the wave's rows (and, the first time, of all its columns), a workgroup
// barrier, 12 MI NJ MFMAs on them with -- in the first half -- the staging traffic interleaved, and
// a second barrier.  What the kernels do differently is passed in:
//   km_frags()        the k-major fragment reads (KM; the row-major ones are here);
//   offsets(oa, ob)   the buffer offsets of the loads two slabs ahead;
//   stage(oa, ob)     stores the slab held in registers to the other LDS buffer and issues those loads;
//   stamp(i)          the phase profile;  after_first()  runs behind the first half's closing barrier.
// Every wave executes exactly two barriers per call.
template <int MI, int NJ, bool KM, class KmFrags, class Offsets, class Stage, class Stamp, class After>
__device__ __forceinline__ void hl_half_step(int hf, f32x4 (&am)[2 * MI][2 * NJ], hx8 (&fah)[MI],
                                             hx8 (&fal)[MI], hx8 (&fbh)[2 * NJ], hx8 (&fbl)[2 * NJ],
                                             const _Float16* Ah, const _Float16* Al,
                                             const _Float16* Bh, const _Float16* Bl, int wm, int wn,
                                             int frow, int fk, KmFrags km_frags, Offsets offsets,
                                             Stage stage, Stamp stamp, After after_first) {
  constexpr int CB = 2 * NJ;
  if constexpr (KM) {
    km_frags();
  } else {
    if (hf == 0) {
#pragma unroll
      for (int j = 0; j < CB; ++j) {
        const int slot = hl256_slot(wn * (32 * NJ) + j * 16 + frow, fk);
        fbh[j] = *reinterpret_cast<const hx8*>(Bh + slot);
        fbl[j] = *reinterpret_cast<const hx8*>(Bl + slot);
      }
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int slot = hl256_slot(wm * (32 * MI) + (hf * MI + i) * 16 + frow, fk);
      fah[i] = *reinterpret_cast<const hx8*>(Ah + slot);
      fal[i] = *reinterpret_cast<const hx8*>(Al + slot);
    }
  }
  unsigned oa[4], ob[4];
  if (hf == 0) {
    offsets(oa, ob);
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(oa[i]), "+v"(ob[i]));
  }
  __builtin_amdgcn_sched_barrier(0);
  stamp(0);
  __syncthreads();
  stamp(1);
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_setprio(1);
  // the staging traffic rides in the issue gaps of this phase's MFMAs (16 cycles of pipe
  // per MFMA, ~4 of issue): the 8 LDS writes of slab kt+1 first -- each frees its
  // registers -- then the 8 loads of slab kt+2 into them; the read phases stay bare.
  // Past the last slab every offset is out of range: those loads return zeros, unused.
  if (hf == 0) stage(oa, ob);
  // term-major order: consecutive MFMAs go to MI CB different accumulators
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < CB; ++j)
      am[hf * MI + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[j], fal[i], am[hf * MI + i][j], 0, 0, 0);
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < CB; ++j)
      am[hf * MI + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbl[j], fah[i], am[hf * MI + i][j], 0, 0, 0);
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < CB; ++j)
      am[hf * MI + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[j], fah[i], am[hf * MI + i][j], 0, 0, 0);
  if (hf == 0) {
    constexpr int NM = 3 * MI * CB;                    // MFMAs of the phase: 48 or 24
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, NM >= 48 ? 2 : 1, 0);   // MFMA
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                  // DS write
    }
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, NM >= 48 ? 4 : 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                  // VMEM read
    }
  }
  __builtin_amdgcn_s_setprio(0);
  __builtin_amdgcn_sched_barrier(0);
  stamp(hf == 0 ? 2 : 3);
  __syncthreads();
  stamp(4);
  __builtin_amdgcn_sched_barrier(0);
  if (hf == 0) after_first();
}

// WN waves across the columns (2 rows of waves); a wave owns 32 MI x 32 NJ of the tile as
// RB x CB = 2 MI x 2 NJ MFMA tiles of 16 x 16: the square tile is 64 MI = 32 NJ WN wide and
// every thread stages four 16-byte chunks per operand.
//   <4, 4, 2>: 256 x 256, 512 threads, 128 KB LDS -- the main kernel;
//   <2, 2, 2>: 128 x 128, 256 threads,  64 KB LDS -- small outputs, and the one that fits on a
//              CU BESIDE a recurrent workgroup (96 KB + 64 KB of LDS, 2 + 1 waves per SIMD).
// The MFMA takes the fragment of B (16 columns of C) as its first operand and the fragment of A
// (16 rows of C) as its second: a lane then holds FOUR CONSECUTIVE COLUMNS of one row of C
// (row = lane & 15, columns 4 (lane >> 4) ..), and the epilogue is 16-byte stores.
//
// Debug (asr_gemm_hl_profile): shader clocks per phase of the K loop, summed over the slabs of
// workgroup 0 of a launch, per wave: 0 fragment reads, 1 barrier before the MFMAs, 2 MFMAs of
// the first half of the rows (with the staging traffic), 3 MFMAs of the second half, 4 barrier
// behind the MFMAs, 5 the prologue; 6 = the K loop in ticks of the 100 MHz real-time counter.
__device__ int g_hl_prof_on = 0;
__device__ long long g_hl_prof[8][8];

template <int WN, int MI, int NJ, bool KM, bool SEG = false>
__global__ void __launch_bounds__(128 * WN)
gemm_hlx_kernel(HlSrc A, HlSrc B, int M, int N, int K, int k_per_split, int splits,
                Epilogue ep, const float* __restrict__ a_scale,
                const float* __restrict__ b_scale, HlSeg seg) {
  constexpr int NT = 128 * WN, TM2 = 64 * MI, TN2 = 32 * NJ * WN;
  constexpr int RB = 2 * MI, CB = 2 * NJ;           // 16 x 16 tiles per wave: rows x columns
  static_assert(TM2 == TN2 && TM2 * 8 == 4 * NT, "square tile, four chunks per thread and operand");
  // KM: the operands are K-major planes (rows = reduction index), HlLoaderT; else HlLoaderX
  // SEG: A's reduction range is segmented (HlSeg; the conv2d entry points) -- its own
  // instantiation, so that the plain kernels' K loop is untouched
  using Loader = std::conditional_t<KM, HlLoaderT<NT>, HlLoaderX<NT>>;
  using LoaderA = std::conditional_t<KM, HlLoaderT<NT>, HlLoaderX<NT, SEG>>;
  extern __shared__ __attribute__((aligned(16))) _Float16 hsm[];
  constexpr int kOpBytes = (TM2 / 16) * 2 * kSubtile;          // KM: one operand's slab image
  auto opimg = [&](int buf, int which) {
    return reinterpret_cast<char*>(hsm) + (size_t)(buf * 2 + which) * kOpBytes;
  };
  // halfs per plane: + 64 bytes, so that a row's hi and lo chunks (one 8-lane group of the
  // staging ds_write_b128) fall into different banks
  constexpr int kPlane = TM2 * 32 + 32;
  auto plane = [&](int buf, int which) { return hsm + (size_t)(buf * 4 + which) * kPlane; };
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;          // 2 x WN waves, (32 MI) x (32 NJ) each
  // (K-major batches: z = split * batch + b, so that the split-K partials of all batch members
  // form ONE ([split][batch * M][N]) array and the plain reduce kernel folds them)
  const int nbatch = (KM && seg.batch > 1u) ? (int)seg.batch : 1;
  const TileId tb = tile_of_block((M + TM2 - 1) / TM2, (N + TN2 - 1) / TN2, splits * nbatch);
  const int m0 = tb.tm * TM2, n0 = tb.tn * TN2;
  const int zb = tb.z % nbatch;
  const int k_begin = (tb.z / nbatch) * k_per_split;
  int k_end = k_begin + k_per_split;
  if (k_end > K) k_end = K;
  const float sa = a_scale ? *a_scale : 1.f, sb = b_scale ? *b_scale : 1.f;
  if constexpr (KM) {
    if (nbatch > 1) {       // member zb: A shifted by its byte offset, C by zb x M rows
      const unsigned o = seg.adj[zb];
      A.p = reinterpret_cast<const _Float16*>(reinterpret_cast<const char*>(A.p) + o);
      A.extent -= o;
      ep.C += (size_t)zb * M * ep.ldc;
    }
  }

  f32x4 am[RB][CB];
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < CB; ++j) am[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const bool prof = g_hl_prof_on != 0 && blockIdx.x == 0;
  long long pt[6] = {0, 0, 0, 0, 0, 0};
  long long plast = prof ? (long long)__builtin_readcyclecounter() : 0;
  auto stamp = [&](int i) {
    if (prof) {
      const long long now = (long long)__builtin_readcyclecounter();
      pt[i] += now - plast;
      plast = now;
    }
  };
  LoaderA la;
  Loader lb;
  if constexpr (KM) la.init(A, m0, k_begin, k_end);
  else la.init(A, m0, k_begin, k_end, &seg);
  lb.init(B, n0, k_begin, k_end);
  // One register set, two slabs ahead: at the top of step kt the registers hold slab kt+1
  // (issued a whole step earlier, so it has landed); it is written to the LDS buffer the
  // barrier at the end of step kt-1 released, and the loads of slab kt+2 are issued at once --
  // they fly across this step's 96 MFMAs per wave AND its barriers (plain buffer loads, no
  // vmcnt wait at the barrier).  The scheduling fence keeps the compiler from sinking the
  // loads to their use, which would expose the whole L2/HBM latency every step.
  u32x4g av[4], bv[4];
  const int nk = (k_end - k_begin + HBK - 1) / HBK;
  la.load(0, av);
  lb.load(0, bv);
  if constexpr (KM) {
    Loader::store(av, opimg(0, 0));
    Loader::store(bv, opimg(0, 1));
  } else {
    Loader::store(av, plane(0, 0), plane(0, 1));
    Loader::store(bv, plane(0, 2), plane(0, 3));
  }
  la.load(1, av);
  lb.load(1, bv);
  __syncthreads();
  const int frow = lane & 15, fk = lane >> 4;       // fragment: row of its 16, 16-byte K chunk
  // Ping-pong: a step is four phases -- read the fragments of half of the wave's rows (and, the
  // first time, of all its columns), 12 MI NJ MFMAs on them (with, in the first half, the LDS
  // writes of the next slab and the loads of the one after interleaved), and again for the
  // other rows -- each closed by a workgroup barrier.  The second row of
  // waves (wm = 1; waves w and w+4 share a SIMD) runs ONE BARRIER LATE, so on every SIMD one
  // wave multiplies while the other reads: the matrix pipe no longer idles through the LDS
  // round trips of two waves in lockstep.  Buffer hazards with the one-phase lag: a slab's
  // buffer is last read three phases (>= one barrier) before either row rewrites it, and is
  // first read three phases after the later row wrote it.
  if (wm == 1) __builtin_amdgcn_s_barrier();
  stamp(5);
  const long long real0 = prof ? (long long)__builtin_amdgcn_s_memrealtime() : 0;   // 100 MHz
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1, nxt = cur ^ 1;
    hx8 fah[MI], fal[MI], fbh[CB], fbl[CB];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
      hl_half_step<MI, NJ, KM>(
          hf, am, fah, fal, fbh, fbl, plane(cur, 0), plane(cur, 1), plane(cur, 2), plane(cur, 3), wm,
          wn, frow, fk,
          [&]() {                                   // the k-major fragments
            if constexpr (KM) {
              if (hf == 0) {
#pragma unroll
                for (int j = 0; j < CB; ++j) {
                  fbh[j] = Loader::fragment(opimg(cur, 1), wn * CB + j, 0, lane);
                  fbl[j] = Loader::fragment(opimg(cur, 1), wn * CB + j, 1, lane);
                }
              }
#pragma unroll
              for (int i = 0; i < MI; ++i) {
                fah[i] = Loader::fragment(opimg(cur, 0), wm * RB + hf * MI + i, 0, lane);
                fal[i] = Loader::fragment(opimg(cur, 0), wm * RB + hf * MI + i, 1, lane);
              }
            }
          },
          [&](unsigned (&oa)[4], unsigned (&ob)[4]) {
            la.offsets(kt + 2, oa);
            lb.offsets(kt + 2, ob);
          },
          [&](const unsigned (&oa)[4], const unsigned (&ob)[4]) {
            if constexpr (KM) {
              Loader::store(av, opimg(nxt, 0));
              Loader::store(bv, opimg(nxt, 1));
            } else {
              Loader::store(av, plane(nxt, 0), plane(nxt, 1));
              Loader::store(bv, plane(nxt, 2), plane(nxt, 3));
            }
            la.issue(oa, av);
            lb.issue(ob, bv);
          },
          stamp, []() {});
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();
  if (prof && lane == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) g_hl_prof[wave][i] = pt[i];
    g_hl_prof[wave][6] = (long long)__builtin_amdgcn_s_memrealtime() - real0;
  }
  // ---- epilogue
  hlx_epilogue<MI, NJ, SEG>(am, ep, M, N, m0, n0, tb.z, 1.f / (sa * sb), wm, wn, frow, fk, TM2, TN2);
}

// The DMA-staged K-MAJOR kernel: gemm_hlx_kernel<4, 4, 2, true> with its operands staged from
// global memory straight into LDS (buffer_load_dwordx4 ... lds): the same eight 16-byte loads per
// thread and slab, no staging registers, no ds_write_b128 pass.  Tiles, splits, batches, products,
// their order per accumulator, the k permutation both operands share and the epilogue are those of
// the register-staged kernel: results are BIT-IDENTICAL (tests/test_gpu_gemm_km_dma.py).
//
// LDS image (tests/test_gemm_km_dma_layout_model.py is the model these expressions are copied
// from).  A slab row of an operand is 1 KB: 16 column groups of (16 hi, 16 lo) = 64 chunks of 16
// bytes.  Per buffer and operand four REGIONS of [32 k][256 bytes]: region R holds column groups
// 4 R .. 4 R + 3 -- for A the 64 columns wave row R >> 1 reads in half-step R & 1, for B the 64
// columns of wave column R.  One wave instruction writes 64 x 16 bytes contiguously at M0, so a
// region is filled in 1 KB pieces of four rows and the swizzle sits on the SOURCE side: lane p of
// piece q fetches row 4 q + (p >> 4), chunk (p & 15) ^ ((row & 7) << 1) of the region's 16 --
// sixteen lanes still read 256 contiguous bytes, an instruction eight whole lines.  A lane of
// ds_read_b64_tr_b16 supplies row lane >> 2 (+ 16), four columns of group (gq, plane), at
// 256 row + ((16 ((lane >> 1 & 1) ^ (row & 7) << 1) + 8 (lane & 1)) ^ (64 gq + 32 plane)): the
// eight rows of a 32-lane half fall into the eight 32-byte windows of the bank row, no conflicts;
// each lane receives the halfs HlLoaderT::fragment gives it.  A wave stages piece `wave` of B's
// four regions and, out of ITS OWN wave row's columns, pieces wn and wn + 4 of region A0 (half-step
// 0) and of A1 -- so an A region has one wave row as writer and reader, only B is shared across
// the stagger, and all of a wave's pieces have q & 1 = wn & 1: one offset register per operand.
// The scalar offset (the piece's rows, the region's columns, the slab) is outside the descriptor's
// range check: rows past the reduction range and column groups past the operand are compares
// that send the lane's offset out of range, and the DMA then stores zeros.
//
// Phase table of a step kt (local phases of a wave; the second wave row runs one barrier late, so
// its phase p is global phase p + 1).  Buffer kt & 1 is the one this step reads AND restages:
//   0  tr-read B[kt], A0[kt]; lgkmcnt(0)                                              barrier
//   1  MFMAs of half 0;  issue A0[kt+2] (2 pieces: last read in phase 0 of this row, retired)   barrier
//   2  tr-read A1[kt]; lgkmcnt(0); vmcnt(2): everything up to A1[kt+1] has landed -- B[kt+1],
//      A0[kt+1], A1[kt+1] -- only this step's A0[kt+2] stays in flight                barrier
//   3  MFMAs of half 1;  issue B[kt+2] (4), A1[kt+2] (2)                             barrier
// Writes after reads: B[kt] is last read in global phase 4 kt + 1 (second row, retired before its
// barrier) and restaged from global phase 4 kt + 3 on; A1[kt] is read in phase 2 and restaged in
// phase 3 of the same row, A0[kt] read in phase 0 and restaged in phase 1.  Reads after writes:
// slab kt + 1 is first read in global phase 4 kt + 4 (A regions: local phase 4 kt + 4 of the row
// that staged them); every wave has waited for its pieces before the barrier that ends its local
// phase 4 kt + 2, i.e. global phase 4 kt + 2 or 4 kt + 3, which every reader has passed by then.
// Loads fly for three phases (B, A1) and five (A0); the wait is never vmcnt(0) inside the loop.
// Raw s_barrier throughout: __syncthreads() would drain the DMAs.  Past the last slab of the range every lane is
// out of range, so any number of slabs is computed correctly; the host sends ranges shorter than
// kKmDmaMinSlabs -- the two slabs the prologue stages whole -- to the register-staged kernel.
constexpr int kKmDmaMinSlabs = 2;
template <int WN, int MI, int NJ>
__global__ void __launch_bounds__(128 * WN)
gemm_hlt_dma_kernel(HlSrc A, HlSrc B, int M, int N, int K, int k_per_split, int splits,
                    Epilogue ep, const float* __restrict__ a_scale,
                    const float* __restrict__ b_scale, HlSeg seg) {
  static_assert(WN == 4 && MI == 4 && NJ == 2, "the piece map is that of the 256 x 256 tile");
  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef short s4 __attribute__((__vector_size__(4 * sizeof(short))));
  constexpr int TM2 = 64 * MI, TN2 = 32 * NJ * WN, RB = 2 * MI, CB = 2 * NJ;
  constexpr int kRegion = 32 * 256, kImg = 4 * kRegion;          // one operand's slab image: 32 KB
  extern __shared__ __attribute__((aligned(16))) _Float16 hsm[];
  char* lds = reinterpret_cast<char*>(hsm);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int nbatch = seg.batch > 1u ? (int)seg.batch : 1;
  const TileId tb = tile_of_block((M + TM2 - 1) / TM2, (N + TN2 - 1) / TN2, splits * nbatch);
  const int m0 = tb.tm * TM2, n0 = tb.tn * TN2;
  const int zb = tb.z % nbatch;
  const int k_begin = (tb.z / nbatch) * k_per_split;
  int k_end = k_begin + k_per_split;
  if (k_end > K) k_end = K;
  const int depth = k_end - k_begin;
  const int nk = (depth + HBK - 1) / HBK;
  const float sa = a_scale ? *a_scale : 1.f, sb = b_scale ? *b_scale : 1.f;
  if (nbatch > 1) {         // member zb: A shifted by its byte offset, C by zb x M rows
    const unsigned o = seg.adj[zb];
    A.p = reinterpret_cast<const _Float16*>(reinterpret_cast<const char*>(A.p) + o);
    A.extent -= o;
    ep.C += (size_t)zb * M * ep.ldc;
  }

  // ---- load cursor: slab lkt; uniform except one offset per operand
  const int r4 = lane >> 4;
  const int cs = (lane & 15) ^ ((((wn & 1) << 2) | r4) << 1);    // the region chunk this lane fetches
  const unsigned pitchA = (unsigned)A.ld * 4u, pitchB = (unsigned)B.ld * 4u;
  const unsigned offA = (unsigned)r4 * pitchA + 16u * cs;
  const unsigned offB = (unsigned)r4 * pitchB + 16u * cs;
  // (the tile's first slab and column: scalar, with the piece's rows and the region's columns)
  const unsigned baseA = (unsigned)k_begin * pitchA + (unsigned)m0 * 4u;
  const unsigned baseB = (unsigned)k_begin * pitchB + (unsigned)n0 * 4u;
  const int ca_end = ((A.rows + 15) & ~15) - m0 - 16 * (cs >> 2);   // region column 64 R < this: in
  const int cb_end = ((B.rows + 15) & ~15) - n0 - 16 * (cs >> 2);
  const __amdgpu_buffer_rsrc_t rsA =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(A.p), 0, A.extent, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsB =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(B.p), 0, B.extent, 0x00020000);
  int lkt = 0;
  auto pieceA = [&](int q) { return wn + 4 * q; };               // of region 2 wm + h
  // (rows past the reduction range and column groups past the operand: out of range -> zeros)
  auto offs_a = [&](int h, unsigned (&o)[2]) {
    const unsigned a0 = 64 * (2 * wm + h) < ca_end ? offA : kOob;
#pragma unroll
    for (int q = 0; q < 2; ++q) o[q] = lkt * HBK + 4 * pieceA(q) + r4 < depth ? a0 : kOob;
  };
  auto offs_b = [&](unsigned (&o)[4]) {
    const unsigned b0 = lkt * HBK + 4 * wave + r4 < depth ? offB : kOob;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = 64 * i < cb_end ? b0 : kOob;
  };
  auto issue_a = [&](int h, const unsigned (&o)[2], char* img) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rsA, (lds_ptr)(img + kRegion * (2 * wm + h) + 1024 * pieceA(q)), 16, o[q],
          baseA + (unsigned)(lkt * HBK + 4 * pieceA(q)) * pitchA + 256u * (unsigned)(2 * wm + h), 0, 0);
  };
  auto issue_b = [&](const unsigned (&o)[4], char* img) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rsB, (lds_ptr)(img + kImg + kRegion * i + 1024 * wave), 16, o[i],
          baseB + (unsigned)(lkt * HBK + 4 * wave) * pitchB + 256u * (unsigned)i, 0, 0);
  };

  f32x4 am[RB][CB];
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < CB; ++j) am[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // ---- prologue: slabs 0 and 1 whole
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    unsigned o0[2], o1[2], ob[4];
    offs_a(0, o0);
    offs_a(1, o1);
    offs_b(ob);
    char* img = lds + s * 2 * kImg;
    issue_a(0, o0, img);
    issue_b(ob, img);
    issue_a(1, o1, img);
    ++lkt;
  }
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");              // slab 0 has landed
  __builtin_amdgcn_s_barrier();
  // fragment byte within a region: frx[2 gq + plane] for the lane's 8 bytes of group gq of a plane
  // (an XOR of 64 gq + 32 plane on the group-0 hi-plane byte).  The transposing reads are written
  // as assembly: behind the builtin the compiler cannot tell the image from the pieces still in
  // flight and puts vmcnt(0) in front of every read phase.  Their results are waited for by the
  // lgkmcnt(0) that closes the read phase, which the MFMAs cannot be moved across.
  const int frow = lane >> 2;
  const unsigned lds0 = (unsigned)(size_t)(lds_ptr)lds;
  unsigned frx[8];
#pragma unroll
  for (int c = 0; c < 8; ++c)
    frx[c] = lds0 + (unsigned)((256 * frow + 16 * (((lane >> 1) & 1) ^ ((frow & 7) << 1)) + 8 * (lane & 1)) ^
                               (32 * c));
  auto fragment = [&](unsigned region, int gq, int plane) {
    const unsigned q = frx[2 * gq + plane] + region;
    s4 t1, t2;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(t1) : "v"(q) : "memory");
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:4096" : "=v"(t2) : "v"(q) : "memory");
    const hx4 a = __builtin_bit_cast(hx4, t1), b = __builtin_bit_cast(hx4, t2);
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
  };
  if (wm == 1) __builtin_amdgcn_s_barrier();      // the second wave row runs one barrier late
  for (int kt = 0; kt < nk; ++kt) {
    const unsigned bufo = (unsigned)(kt & 1) * 2u * kImg;
    char* img = lds + bufo;                       // lkt = kt + 2: the slab this step restages
    hx8 fah[MI], fal[MI], fbh[CB], fbl[CB];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      // ---- read phase
      if (hf == 0) {
#pragma unroll
        for (int j = 0; j < CB; ++j) {
          fbh[j] = fragment(bufo + kImg + kRegion * wn, j, 0);
          fbl[j] = fragment(bufo + kImg + kRegion * wn, j, 1);
        }
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        fah[i] = fragment(bufo + kRegion * (2 * wm + hf), i, 0);
        fal[i] = fragment(bufo + kRegion * (2 * wm + hf), i, 1);
      }
      unsigned oa[2], ob[4];
      offs_a(hf, oa);
      asm volatile("" : "+v"(oa[0]), "+v"(oa[1]));
      if (hf == 1) {
        offs_b(ob);
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(ob[i]));
      }
      __builtin_amdgcn_sched_barrier(0);
      if (hf == 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---- MFMA phase, this step's DMA pieces in its issue gaps
      __builtin_amdgcn_s_setprio(1);
      if (hf == 1) issue_b(ob, img);
      issue_a(hf, oa, img);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j)
          am[hf * MI + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[j], fal[i], am[hf * MI + i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j)
          am[hf * MI + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbl[j], fah[i], am[hf * MI + i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j)
          am[hf * MI + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[j], fah[i], am[hf * MI + i][j], 0, 0, 0);
      if (hf == 0) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);               // MFMA
          __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);                // VMEM: one piece
        }
      } else {
#pragma unroll
        for (int g = 0; g < 6; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
          __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    ++lkt;
  }
  // the pieces issued past the last slab (out of range, zeros) must land before the LDS is given up
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wm == 0) __builtin_amdgcn_s_barrier();
  // ---- epilogue
  hlx_epilogue<MI, NJ, false>(am, ep, M, N, m0, n0, tb.z, 1.f / (sa * sb), wm, wn, lane & 15,
                              lane >> 4, TM2, TN2);
}


// The DMA-staged tile walk of gemm_hlp_kernel<.., DMA = true>: the operands go from global memory
// straight into LDS (buffer_load_dwordx4 ... lds), no staging registers, no ds_write pass.
//
// LDS image (tests/test_gemm_dma_layout_model.py is the model these expressions are copied from):
// per buffer and operand [256 rows][128 bytes] -- a row's slab line, hi and lo planes together --
// with the 16-byte chunk index XORed by (row >> 1) & 7.  One wave instruction writes 64 x 16 bytes
// contiguously at M0, so the image is filled in 1 KB pieces of 8 rows and the swizzle sits on the
// SOURCE side: lane p of piece P fetches row 8 P + (p >> 3), chunk (p & 7) ^ swizzle -- eight lanes
// still read one whole 128-byte line.  A fragment lane reads (row, plane, reduction chunk fk) at
// 128 row + 16 ((4 (fk >> 1) + 2 plane + (fk & 1)) ^ (row >> 1) & 7): conflict-free in the lane
// groups ds_read_b128 is serviced in.  A wave stages four pieces of B (8 i + wave) and four of A
// out of ITS OWN wave row's rows: two of the 64 rows read in half-step 0 (region A0), two of those
// read in half-step 1 (A1) -- so an A region has one wave row as writer and reader, and only B is
// shared across the stagger.
//
// Phase table of a step kt (local phases of a wave; the second wave row runs one barrier late, so
// its phase p is global phase p + 1).  Buffer kt & 1 is the one this step reads AND restages:
//   0  ds_read B[kt], A0[kt]; lgkmcnt(0)                                     barrier
//   1  MFMAs of half 0;  issue A0[kt+2] (2 pieces: last read in phase 0 of this row, retired)   barrier
//   2  ds_read A1[kt]; lgkmcnt(0); vmcnt(2): everything up to A1[kt+1] has landed -- B[kt+1],
//      A0[kt+1], A1[kt+1] -- only this step's A0[kt+2] stays in flight                barrier
//   3  MFMAs of half 1;  issue B[kt+2] (4), A1[kt+2] (2)                             barrier
// Writes after reads: B[kt] is last read in global phase 4 kt + 1 (second row, retired before its
// barrier) and restaged from global phase 4 kt + 3 on; A1[kt] is read in phase 2 and restaged in
// phase 3 of the same row.  Reads after writes: slab kt + 1 is first read in global phase 4 kt + 4
// (A regions: local phase 4 kt + 4 of the row that staged them); every wave has waited for its
// pieces before its local barrier 4 kt + 3, i.e. global barrier 4 kt + 3 or 4 kt + 4, which every
// reader has passed by then.  Loads fly for three phases (B, A1) and five (A0); the wait is never
// vmcnt(0) inside the loop.  Raw s_barrier throughout: __syncthreads() would drain the DMAs.
// The cursor is two slabs ahead, so the next tile's id must be known at step nk - 2: K >= 4 slabs.
template <int WN, int MI, int NJ>
__device__ __forceinline__ void hlp_dma_tiles(const HlSrc& A, const HlSrc& B, int M, int N, int K,
                                              const Epilogue ep, float unscale,
                                              unsigned* __restrict__ ctl, char* lds, int* mbox,
                                              int vt) {
  static_assert(WN == 4 && MI == 4 && NJ == 2, "the piece map is that of the 256 x 256 tile");
  typedef __attribute__((address_space(3))) void* lds_ptr;
  constexpr int TM2 = 64 * MI, TN2 = 32 * NJ * WN, RB = 2 * MI, CB = 2 * NJ;
  constexpr int kImg = TM2 * 128;                               // one operand's slab image: 32 KB
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int TMc = (M + TM2 - 1) / TM2, TNc = (N + TN2 - 1) / TN2, total = TMc * TNc;
  const int xcd = (int)(blockIdx.x % 8u);
  const int nk = (K + HBK - 1) / HBK;

  // ---- load cursor: tile, slab lkt of it; uniform except one offset per operand
  const int l8 = lane >> 3;
  const int cs = (lane & 7) ^ ((l8 >> 1) | ((wn & 1) << 2));    // the line chunk this lane fetches
  const int kq = 16 * (cs >> 2) + 8 * (cs & 1);
  const unsigned pitchA = (unsigned)A.ld * 4u, pitchB = (unsigned)B.ld * 4u;
  const unsigned offA = (unsigned)l8 * pitchA + 16u * cs;
  const unsigned offB = (unsigned)l8 * pitchB + 16u * cs;
  auto pieceA = [&](int h, int q) { return wm * 16 + 8 * h + 4 * q + wn; };
  auto pieceB = [&](int i) { return 8 * i + wave; };
  __amdgpu_buffer_rsrc_t rsA, rsB;
  int ra_left = 0, rb_left = 0, lkt = 0;
  int v_nxt = total;
  auto setup = [&](int v) {
    if (v < total) {
      const TileId t = tile_of_id(v, TMc, TNc, 1);
      const unsigned ba = (unsigned)(t.tm * TM2) * pitchA;
      const unsigned bb = (unsigned)(t.tn * TN2) * pitchB;
      rsA = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<char*>(reinterpret_cast<const char*>(A.p)) + ba, 0, A.extent - ba, 0x00020000);
      rsB = __builtin_amdgcn_make_buffer_rsrc(
          const_cast<char*>(reinterpret_cast<const char*>(B.p)) + bb, 0, B.extent - bb, 0x00020000);
      ra_left = M - t.tm * TM2;
      rb_left = N - t.tn * TN2;
    } else {                                     // past the last tile: every offset out of range
      ra_left = 0;
      rb_left = 0;
    }
  };
  auto advance = [&]() {
    if (++lkt == nk) {
      lkt = 0;
      setup(v_nxt);
    }
  };
  // (rows past the operand and the reduction tail send the lane's offset out of range: zeros)
  auto offs_a = [&](int h, unsigned (&o)[2]) {
    const unsigned a0 = lkt * HBK + kq < K ? offA : kOob;
#pragma unroll
    for (int q = 0; q < 2; ++q) o[q] = 8 * pieceA(h, q) + l8 < ra_left ? a0 : kOob;
  };
  auto offs_b = [&](unsigned (&o)[4]) {
    const unsigned b0 = lkt * HBK + kq < K ? offB : kOob;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = 8 * pieceB(i) + l8 < rb_left ? b0 : kOob;
  };
  auto issue_a = [&](int h, const unsigned (&o)[2], char* img) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rsA, (lds_ptr)(img + 1024 * pieceA(h, q)), 16, o[q],
          (unsigned)(8 * pieceA(h, q)) * pitchA + (unsigned)(lkt * HBK * 4), 0, 0);
  };
  auto issue_b = [&](const unsigned (&o)[4], char* img) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rsB, (lds_ptr)(img + kImg + 1024 * pieceB(i)), 16, o[i],
          (unsigned)(8 * pieceB(i)) * pitchB + (unsigned)(lkt * HBK * 4), 0, 0);
  };
  rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(A.p), 0, A.extent, 0x00020000);
  rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(B.p), 0, B.extent, 0x00020000);
  setup(vt);

  f32x4 am[RB][CB];
#pragma unroll
  for (int i = 0; i < RB; ++i)
#pragma unroll
    for (int j = 0; j < CB; ++j) am[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // ---- prologue: slabs 0 and 1 whole (K >= 4 slabs: the cursor stays in this tile)
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    unsigned o0[2], o1[2], ob[4];
    offs_a(0, o0);
    offs_a(1, o1);
    offs_b(ob);
    char* img = lds + s * 2 * kImg;
    issue_a(0, o0, img);
    issue_b(ob, img);
    issue_a(1, o1, img);
    if (s == 0) ++lkt;
  }
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");              // slab 0 has landed
  __builtin_amdgcn_s_barrier();
  const int frow = lane & 15, fk = lane >> 4;
  // fragment byte within the image, hi plane; the lo plane is 32 bytes (two chunks) away
  const int fro = 128 * frow + 16 * (((4 * (fk >> 1) + (fk & 1)) ^ (frow >> 1)) & 7);
  const int frl = fro ^ 32;
  TileId tc = tile_of_id(vt, TMc, TNc, 1);
  int m0 = tc.tm * TM2, n0 = tc.tn * TN2;
  unsigned pending = 0u;
  int ti = 0, kt = 0, cur = 0;
  if (wm == 1) __builtin_amdgcn_s_barrier();      // the second wave row runs one barrier late
  for (;;) {
    if (kt == 0) {
      if (tid == 0) pending = atomicAdd(&ctl[xcd], 1u);
    } else if (kt == 1) {
      if (tid == 0) mbox[(ti + 1) & 1] = (int)(pending * 8u) + xcd;
    } else if (kt == 2) {
      v_nxt = __builtin_amdgcn_readfirstlane(mbox[(ti + 1) & 1]);
    }
    advance();                                    // the cursor: slab kt + 2 (of the next tile)
    char* img = lds + cur * 2 * kImg;
    const char* fa = img + 128 * (wm * (32 * MI));
    const char* fb = img + kImg + 128 * (wn * (32 * NJ));
    hx8 fah[MI], fal[MI], fbh[CB], fbl[CB];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      // ---- read phase
      if (hf == 0) {
#pragma unroll
        for (int j = 0; j < CB; ++j) {
          fbh[j] = *reinterpret_cast<const hx8*>(fb + 2048 * j + fro);
          fbl[j] = *reinterpret_cast<const hx8*>(fb + 2048 * j + frl);
        }
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        fah[i] = *reinterpret_cast<const hx8*>(fa + 2048 * (hf * MI + i) + fro);
        fal[i] = *reinterpret_cast<const hx8*>(fa + 2048 * (hf * MI + i) + frl);
      }
      unsigned oa[2], ob[4];
      offs_a(hf, oa);
      asm volatile("" : "+v"(oa[0]), "+v"(oa[1]));
      if (hf == 1) {
        offs_b(ob);
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(ob[i]));
      }
      __builtin_amdgcn_sched_barrier(0);
      if (hf == 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---- MFMA phase, this step's DMA pieces in its issue gaps
      __builtin_amdgcn_s_setprio(1);
      if (hf == 1) issue_b(ob, img);
      issue_a(hf, oa, img);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j)
          am[hf * MI + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[j], fal[i], am[hf * MI + i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j)
          am[hf * MI + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbl[j], fah[i], am[hf * MI + i][j], 0, 0, 0);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j)
          am[hf * MI + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fbh[j], fah[i], am[hf * MI + i][j], 0, 0, 0);
      if (hf == 0) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);               // MFMA
          __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);                // VMEM: one piece
        }
      } else {
#pragma unroll
        for (int g = 0; g < 6; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
          __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    cur ^= 1;
    if (++kt == nk) {
      // ---- a finished tile: epilogue behind the closing barrier, accumulators back to zero
      int fr = lane & 15, fq = lane >> 4;
      asm volatile("" : "+v"(fr), "+v"(fq));
      hlx_epilogue<MI, NJ, false>(am, ep, M, N, m0, n0, 0, unscale, wm, wn, fr, fq, TM2, TN2);
#pragma unroll
      for (int i = 0; i < RB; ++i)
#pragma unroll
        for (int j = 0; j < CB; ++j) am[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      kt = 0;
      ++ti;
      vt = v_nxt;
      if (vt >= total) break;
      tc = tile_of_id(vt, TMc, TNc, 1);
      m0 = tc.tm * TM2;
      n0 = tc.tn * TN2;
    }
  }
  // the pieces issued past the last tile (out of range, zeros) must land before the LDS is given up
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (wm == 0) __builtin_amdgcn_s_barrier();
}

// PERSISTENT row-major form (gemm_hlp_kernel; round 6).  The 256 x 256 tile of the plain kernel
// pays ~17 us per output tile around its K loop -- the dispatch of a new workgroup onto a CU whose
// LDS and registers the previous one filled, a cold prologue (two dependent L2 / HBM round
// trips), 256 KB of epilogue stores that must drain before the workgroup may end -- which is
// 19 % of a K = 1024 tile (x@W: 73 us of K loop) and 5 % of a K = 4096 one (dX); measured as
// 1.447 / 1.245 ms for the two shapes of equal flops.  Here ONE workgroup per CU walks tiles:
// the K loop never stops -- the loads two slabs ahead run on into the NEXT tile's first slabs
// (a load cursor of its own: per-tile buffer descriptor and row bounds in SGPRs, the thread's
// offsets are tile-invariant), the epilogue of a finished tile is issued at the top of the next
// tile's first step, i.e. behind the closing barrier, where its VALU work and stores overlap the
// MFMA phase of the other wave row of the ping-pong, and the accumulators are cleared there.
// Products and their order within a tile are those of gemm_hlx_kernel: results are BIT-IDENTICAL
// (tests/test_gpu_gemm.py::test_gemm_hl_persistent_form_is_bit_identical).  Tiles are handed out dynamically, per XCD, in the order of
// tile_of_block (ctl[x] = next index of XCD x's contiguous range: L2 locality as before, and a
// CU that starts late -- a kernel of another stream still on it -- simply takes fewer tiles);
// the id of the next tile is fetched by thread 0 at a tile's first step, posted in LDS at the
// second and read by all at the third (needs K >= 4 slabs).  ctl[8] counts finished workgroups
// (atomicInc wraps it to 0); the last one clears ctl[0..7]: a control block is reusable by the
// next launch without a memset.
// DMA = true: the same walk with the operands staged by LDS-DMA (hlp_dma_tiles above; its own LDS
// image, cursor and K loop; tile hand-out, epilogue and every product as here).  The host picks the
// instantiation per launch (ASR_GEMM_DMA); the register-staged one is the code below, unchanged.
template <int WN, int MI, int NJ, bool DMA = false>
__global__ void __launch_bounds__(128 * WN)
gemm_hlp_kernel(HlSrc A, HlSrc B, int M, int N, int K, Epilogue ep,
                const float* __restrict__ a_scale, const float* __restrict__ b_scale,
                unsigned* __restrict__ ctl) {
  constexpr int NT = 128 * WN, TM2 = 64 * MI, TN2 = 32 * NJ * WN;
  constexpr int RB = 2 * MI, CB = 2 * NJ;
  static_assert(TM2 == TN2 && TM2 * 8 == 4 * NT, "square tile, four chunks per thread and operand");
  extern __shared__ __attribute__((aligned(16))) _Float16 hsm[];
  constexpr int kPlane = TM2 * 32 + 32;
  auto plane = [&](int buf, int which) { return hsm + (size_t)(buf * 4 + which) * kPlane; };
  int* mbox = reinterpret_cast<int*>(hsm + (size_t)8 * kPlane);     // two tile-id slots
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int TMc = (M + TM2 - 1) / TM2, TNc = (N + TN2 - 1) / TN2, total = TMc * TNc;
  const int xcd = (int)(blockIdx.x % 8u);
  const int nk = (K + HBK - 1) / HBK;
  const float sa = a_scale ? *a_scale : 1.f, sb = b_scale ? *b_scale : 1.f;
  const float unscale = 1.f / (sa * sb);

  if (tid == 0) mbox[0] = (int)(atomicAdd(&ctl[xcd], 1u) * 8u) + xcd;
  __syncthreads();
  int vt = __builtin_amdgcn_readfirstlane(mbox[0]);          // the tile being multiplied
  int v_nxt = total;                                           // the one after it (known from kt = 2)
  if constexpr (DMA) {
    if (vt < total)
      hlp_dma_tiles<WN, MI, NJ>(A, B, M, N, K, ep, unscale, ctl, reinterpret_cast<char*>(hsm), mbox, vt);
  } else if (vt < total) {
    // ---- load cursor: tile lv, slab lkt of it; everything uniform except the two offsets
    const int c8 = tid & 7, r8 = tid >> 3;
    const int kq = 16 * (c8 >> 2) + 8 * (c8 & 1);
    const unsigned offA = (unsigned)r8 * (unsigned)A.ld * 4u + 16u * c8;
    const unsigned offB = (unsigned)r8 * (unsigned)B.ld * 4u + 16u * c8;
    const unsigned stepA = (unsigned)(NT / 8) * (unsigned)A.ld * 4u;
    const unsigned stepB = (unsigned)(NT / 8) * (unsigned)B.ld * 4u;
    __amdgpu_buffer_rsrc_t rsA, rsB;
    int ra_left = 0, rb_left = 0, lkt = 0;
    auto setup = [&](int v) {
      if (v < total) {
        const TileId t = tile_of_id(v, TMc, TNc, 1);
        const unsigned ba = (unsigned)(t.tm * TM2) * (unsigned)A.ld * 4u;
        const unsigned bb = (unsigned)(t.tn * TN2) * (unsigned)B.ld * 4u;
        rsA = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(A.p)) + ba, 0, A.extent - ba, 0x00020000);
        rsB = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char*>(reinterpret_cast<const char*>(B.p)) + bb, 0, B.extent - bb, 0x00020000);
        ra_left = M - t.tm * TM2;
        rb_left = N - t.tn * TN2;
      } else {                                   // past the last tile: every offset out of range
        ra_left = 0;
        rb_left = 0;
      }
    };
    auto offsets = [&](unsigned (&oa)[4], unsigned (&ob)[4]) {
      const bool kin = lkt * HBK + kq < K;
      const unsigned a0 = kin ? offA + (unsigned)(lkt * HBK * 4) : kOob;
      const unsigned b0 = kin ? offB + (unsigned)(lkt * HBK * 4) : kOob;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        oa[i] = r8 + i * (NT / 8) < ra_left ? a0 : kOob;
        ob[i] = r8 + i * (NT / 8) < rb_left ? b0 : kOob;
      }
    };
    auto issue = [&](const unsigned (&oa)[4], const unsigned (&ob)[4], u32x4g (&av)[4],
                     u32x4g (&bv)[4]) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        av[i] = __builtin_amdgcn_raw_buffer_load_b128(rsA, oa[i], i * stepA, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        bv[i] = __builtin_amdgcn_raw_buffer_load_b128(rsB, ob[i], i * stepB, 0);
    };
    auto advance = [&]() {                       // to the next slab (of the next tile)
      if (++lkt == nk) {
        lkt = 0;
        setup(v_nxt);
      }
    };
    rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(A.p), 0, A.extent, 0x00020000);
    rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16*>(B.p), 0, B.extent, 0x00020000);
    setup(vt);

    f32x4 am[RB][CB];
#pragma unroll
    for (int i = 0; i < RB; ++i)
#pragma unroll
      for (int j = 0; j < CB; ++j) am[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4g av[4], bv[4];
    {
      unsigned oa[4], ob[4];
      offsets(oa, ob);
      issue(oa, ob, av, bv);
      advance();
      HlLoaderX<NT>::store(av, plane(0, 0), plane(0, 1));
      HlLoaderX<NT>::store(bv, plane(0, 2), plane(0, 3));
      offsets(oa, ob);
      issue(oa, ob, av, bv);
      advance();
    }
    __syncthreads();
    const int frow = lane & 15, fk = lane >> 4;
    TileId tc = tile_of_id(vt, TMc, TNc, 1);
    int m0 = tc.tm * TM2, n0 = tc.tn * TN2;
    unsigned pending = 0u;                        // thread 0: the fetched index of the next tile
    int ti = 0;                                   // tiles this workgroup has started
    int kt = 0;
    int cur = 0;
    if (wm == 1) __builtin_amdgcn_s_barrier();    // the second wave row runs one barrier late
    for (;;) {
      // ---- the id of the next tile: fetched, posted, read (one step each)
      if (kt == 0) {
        if (tid == 0) pending = atomicAdd(&ctl[xcd], 1u);
      } else if (kt == 1) {
        if (tid == 0) mbox[(ti + 1) & 1] = (int)(pending * 8u) + xcd;
      } else if (kt == 2) {
        v_nxt = __builtin_amdgcn_readfirstlane(mbox[(ti + 1) & 1]);
      }
      const int nxt = cur ^ 1;
      hx8 fah[MI], fal[MI], fbh[CB], fbl[CB];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
        hl_half_step<MI, NJ, false>(
            hf, am, fah, fal, fbh, fbl, plane(cur, 0), plane(cur, 1), plane(cur, 2), plane(cur, 3),
            wm, wn, frow, fk, []() {}, offsets,
            [&](const unsigned (&oa)[4], const unsigned (&ob)[4]) {
              HlLoaderX<NT>::store(av, plane(nxt, 0), plane(nxt, 1));
              HlLoaderX<NT>::store(bv, plane(nxt, 2), plane(nxt, 3));
              issue(oa, ob, av, bv);
            },
            [](int) {}, advance);            // (scalar: the cursor's next slab / tile)
      cur = nxt;
      if (++kt == nk) {
        // ---- a finished tile: its epilogue here, behind the closing barrier -- the other wave
        // row's MFMA phase runs meanwhile -- and the accumulators start the next tile at zero
        // (its lane coordinates are made opaque HERE: the address arithmetic they feed must not
        // be hoisted out of the K loop, where every register is taken)
        int fr = lane & 15, fq = lane >> 4;
        asm volatile("" : "+v"(fr), "+v"(fq));
        hlx_epilogue<MI, NJ, false>(am, ep, M, N, m0, n0, 0, unscale, wm, wn, fr, fq, TM2, TN2);
#pragma unroll
        for (int i = 0; i < RB; ++i)
#pragma unroll
          for (int j = 0; j < CB; ++j) am[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        kt = 0;
        ++ti;
        vt = v_nxt;
        if (vt >= total) break;
        tc = tile_of_id(vt, TMc, TNc, 1);
        m0 = tc.tm * TM2;
        n0 = tc.tn * TN2;
      }
    }
    if (wm == 0) __builtin_amdgcn_s_barrier();
  }
  // ---- the last workgroup to finish re-arms the control block
  if (tid == 0) {
    const unsigned done = atomicInc(&ctl[8], gridDim.x - 1u);
    if (done == gridDim.x - 1u) {
#pragma unroll
      for (int i = 0; i < 8; ++i) atomicExch(&ctl[i], 0u);
    }
  }
}

}  // namespace

// Debug: enable != 0 arms the phase profile of the next asr_gemm_hl launches;
// out64 (may be NULL) receives the 8 waves x 8 phases of the last armed launch's workgroup 0.
extern "C" int asr_gemm_hl_profile(int enable, long long* out64, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_HIP(hipStreamSynchronize(stream));
  if (out64) ASR_CHECK_HIP(hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_hl_prof), sizeof(long long) * 64));
  ASR_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_hl_prof_on), &enable, sizeof(int)));
  return ASR_OK;
}


// ---- host side of the persistent form: control blocks (9 words each, zero between launches:
// the kernel re-arms its block itself), handed out round-robin from a ring per device so that
// launches in flight on different streams never share one
static bool hlp_enabled() {
  const char* v = getenv("ASR_GEMM_PERSIST");
  return !(v && *v == '0');
}
static int hlp_num_cu() {
  static int ncu[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
  if (!ncu[dev]) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
    ncu[dev] = prop.multiProcessorCount;
  }
  return ncu[dev];
}
// (a __device__ array: zero at module load, one instance per device, no allocation -- the library
// still owns no device memory it had to ask for)
constexpr int kHlpRing = 256, kHlpWords = 16;
__device__ unsigned g_hlp_ctl[kHlpRing * kHlpWords];
// A slot belongs to the STREAM that first asked for one: launches of one stream run one after the
// other and the kernel re-arms its block, so they can share it; launches of different streams
// never do, however many are in flight.  (A round-robin over the ring handed a block out again
// after kHlpRing launches whether or not its first user had finished.)  nullptr -- the plain
// kernel runs -- once kHlpRing different streams of a device have asked.
static unsigned* hlp_control_block(hipStream_t stream) {
  static unsigned* ring[16] = {nullptr};
  static hipStream_t owner[16][kHlpRing];
  static int used[16] = {0};
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  if (!ring[dev]) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_hlp_ctl)) != hipSuccess || !p) return nullptr;
    ring[dev] = reinterpret_cast<unsigned*>(p);
  }
  int slot = 0;
  while (slot < used[dev] && owner[dev][slot] != stream) ++slot;
  if (slot == used[dev]) {
    if (slot == kHlpRing) return nullptr;
    owner[dev][used[dev]++] = stream;
  }
  return ring[dev] + (size_t)slot * kHlpWords;
}
// ASR_GEMM_DMA: 1 (the default: DESIGN.md 6) = the DMA-staged persistent form wherever the
// persistent form runs, 0 = the register-staged one, 2 = the DMA-staged one for EVERY plain
// row-major launch of the big tile with K >= 4 slabs, however few tiles (tests: small shapes)
static int hlp_dma_mode() {
  const char* v = getenv("ASR_GEMM_DMA");
  if (!v || !*v) return 1;
  return *v == '0' ? 0 : (*v == '2' ? 2 : 1);
}
// ASR_GEMM_KM_DMA: 1 (the default: DESIGN.md 6) = gemm_hlt_dma_kernel wherever the big-tile k_major
// kernel runs with at least kKmDmaMinSlabs slabs per split, 0 = the register-staged kernel
// everywhere.  Read per call, like ASR_GEMM_DMA (bit-identical results: the switch changes time only)
static bool km_dma_enabled() {
  const char* v = getenv("ASR_GEMM_KM_DMA");
  return !(v && *v == '0');
}

extern "C" size_t asr_gemm_hl_workspace_bytes(const asr_gemm_hl_args* a) {
  if (!a) return 0;
  int kps = 0;
  const int splits = split_plan(a->K, a->split_k, HBK, &kps);
  if (splits <= 1) return 0;
  const size_t nbatch = a->batch > 1 ? a->batch : 1;
  return asr_align_up((size_t)splits * nbatch * a->M * a->N * sizeof(float), 256);
}

extern "C" int asr_gemm_hl(const asr_gemm_hl_args* a, void* workspace, size_t ws_bytes,
                           asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(a && a->a_hl && a->b_hl && a->C, "gemm_hl: null pointer");
  ASR_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0 && (a->k_major || a->K % 8 == 0),
                "gemm_hl: bad shape %d %d %d (K must be a multiple of 8)", a->M, a->N, a->K);
  const bool km = a->k_major != 0;
  if (km)
    ASR_CHECK_ARG(a->lda >= a->M && a->ldb >= a->N && a->lda % 16 == 0 && a->ldb % 16 == 0 &&
                  a->ldc >= a->N, "gemm_hl (k_major): bad leading dimensions");
  else
  ASR_CHECK_ARG((a->lda >= a->K || a->a_seg_k > 0) && a->ldb >= a->K && a->lda % 16 == 0 &&
                a->ldb % 16 == 0 && a->ldc >= a->N,
                "gemm_hl: bad leading dimensions (multiples of 16: whole (hi, lo) groups)");
  ASR_CHECK_ARG((reinterpret_cast<uintptr_t>(a->a_hl) & 63) == 0 &&
                (reinterpret_cast<uintptr_t>(a->b_hl) & 63) == 0,
                "gemm_hl: planes must start at a reduction group (64-byte aligned)");
  // bytes from the first row's first group to the end of the last row's last group
  // (k_major: K plane rows of 4 ld bytes, the last one up to the operand's last column group)
  const size_t ext_a = km ? ((size_t)(a->K - 1) * a->lda + (size_t)((a->M + 15) / 16) * 16) * 4
                          : ((size_t)(a->M - 1) * 2 * a->lda + (size_t)((a->K + 15) / 16) * 32) * 2;
  const size_t ext_b = km ? ((size_t)(a->K - 1) * a->ldb + (size_t)((a->N + 15) / 16) * 16) * 4
                          : ((size_t)(a->N - 1) * 2 * a->ldb + (size_t)((a->K + 15) / 16) * 32) * 2;
  // (32-bit offsets; a tile's rows past the operand are computed before they are masked)
  const size_t lim = ((size_t)1 << 32) - ((size_t)1 << 20);
  ASR_CHECK_ARG(ext_a + (size_t)1024 * a->lda * 4 < lim && ext_b + (size_t)1024 * a->ldb * 4 < lim,
                "gemm_hl: operand larger than 4 GiB");
  int kps = 0;
  const int splits = split_plan(a->K, a->split_k, HBK, &kps);
  const int nbatch = a->batch > 1 ? a->batch : 1;
  Epilogue ep = make_epilogue(a);
  if (int rc = splitk_workspace("gemm_hl", splits, (size_t)nbatch * a->M, a->N, workspace, ws_bytes,
                                &ep))
    return rc;
  if (a->clamp_hi > 0.f) {
    ASR_CHECK_ARG(a->a_seg_k > 0 && a->beta == 0.f && !a->c_scale && splits == 1,
                  "gemm_hl: clamp_hi needs the segmented form, beta = 0, no mask, no split");
    ep.clamp_hi = a->clamp_hi;
  }
  HlSeg seg;
  seg.magic = 0u;
  seg.batch = 0u;
  for (int i = 0; i < 16; ++i) seg.adj[i] = 0u;
  size_t ext_a_seg = ext_a;
  if (nbatch > 1) {
    // batch of k_major GEMMs sharing B: C_b = A_b^T B, A_b = a_hl shifted by a_batch_row[b] rows
    ASR_CHECK_ARG(km && nbatch <= 16 && a->a_seg_k == 0 && a->beta == 0.f && !a->bias && !a->c_scale,
                  "gemm_hl: a batch needs the k_major form, <= 16 members, no beta / bias / mask");
    long long max_row = 0;
    for (int b = 0; b < nbatch; ++b) {
      ASR_CHECK_ARG(a->a_batch_row[b] >= 0, "gemm_hl: negative batch row shift");
      if (a->a_batch_row[b] > max_row) max_row = a->a_batch_row[b];
      seg.adj[b] = (unsigned)((unsigned long long)a->a_batch_row[b] * (unsigned long long)a->lda * 4ull);
    }
    seg.batch = (unsigned)nbatch;
    ext_a_seg = ext_a + (size_t)max_row * a->lda * 4;
    ASR_CHECK_ARG(ext_a_seg + (size_t)1024 * a->lda * 4 < lim, "gemm_hl: operand larger than 4 GiB");
  }
  if (a->a_seg_k > 0) {
    // A's reduction range = n segments of a_seg_k indices, segment i shifted by a_seg_row[i]
    // plane rows (>= 0: the caller points a_hl at the lowest row any segment reads)
    ASR_CHECK_ARG(!km && a->a_seg_k % HBK == 0 && a->K % a->a_seg_k == 0 &&
                  a->K / a->a_seg_k <= 16 && a->lda >= a->a_seg_k,
                  "gemm_hl: segments need the row-major form, a_seg_k %% 32 == 0, K = n * a_seg_k, n <= 16");
    const int nseg = a->K / a->a_seg_k, sps = a->a_seg_k / HBK;
    seg.magic = (1u << 20) / (unsigned)sps + 1u;
    for (int g = 0; g < a->K / HBK; ++g)
      ASR_CHECK_ARG((int)(((unsigned)g * seg.magic) >> 20) == g / sps, "gemm_hl: segment magic");
    long long max_row = 0;
    for (int i = 0; i < nseg; ++i) {
      ASR_CHECK_ARG(a->a_seg_row[i] >= 0, "gemm_hl: negative segment row shift");
      if (a->a_seg_row[i] > max_row) max_row = a->a_seg_row[i];
      // bytes: the segment's row shift minus what the running reduction offset has advanced
      const long long adj = a->a_seg_row[i] * (long long)a->lda * 4 - (long long)i * a->a_seg_k * 4;
      seg.adj[i] = (unsigned)(unsigned long long)adj;
    }
    ext_a_seg = ((size_t)(a->M - 1 + max_row) * 2 * a->lda + (size_t)(a->a_seg_k / 16) * 32) * 2;
    ASR_CHECK_ARG(ext_a_seg + (size_t)1024 * a->lda * 4 < lim, "gemm_hl: operand larger than 4 GiB");
  }
  HlSrc A, B;
  A.p = reinterpret_cast<const _Float16*>(a->a_hl);
  A.ld = a->lda; A.rows = a->M; A.extent = (unsigned)ext_a_seg;
  B.p = reinterpret_cast<const _Float16*>(a->b_hl);
  B.ld = a->ldb; B.rows = a->N; B.extent = (unsigned)ext_b;
  // tile: 256 x 256 (512 threads, 128 KB LDS) for outputs of at least that size, else 128 x 128
  // (256 threads, 64 KB; asr_gemm_hl_args.tile = 128 forces it)
  const bool big = a->tile != 128 && a->M >= 256 && a->N >= 256;
  const int tl = big ? 256 : 128;
  const size_t shm = km ? (size_t)2 * 2 * (tl / 16) * 2 * kSubtile
                        : (size_t)2 * 4 * (tl * 32 + 32) * sizeof(_Float16);
  const int total = ((a->M + tl - 1) / tl) * ((a->N + tl - 1) / tl) * splits * nbatch;
  const bool segd = seg.magic != 0u;
  // kernel variants: [tile 256 / 128][row-major / k-major / row-major with a segmented A]
  typedef void (*hlx_t)(HlSrc, HlSrc, int, int, int, int, int, Epilogue, const float*, const float*,
                        HlSeg);
  static const hlx_t kern[2][3] = {
      {gemm_hlx_kernel<4, 4, 2, false>, gemm_hlx_kernel<4, 4, 2, true>,
       gemm_hlx_kernel<4, 4, 2, false, true>},
      {gemm_hlx_kernel<2, 2, 2, false>, gemm_hlx_kernel<2, 2, 2, true>,
       gemm_hlx_kernel<2, 2, 2, false, true>}};
  const int vi = big ? 0 : 1, vj = km ? 1 : (segd ? 2 : 0);
  // the persistent form (gemm_hlp_kernel): plain row-major launches of the big tile with at
  // least two tiles per CU and five slabs per tile; ASR_GEMM_PERSIST=0 keeps the plain kernel
  // (bit-identical results: the switch changes time only)
  unsigned* ctl = nullptr;
  int grid_p = 0;
  // ASR_GEMM_DMA picks the staging of the persistent form (hlp_dma_mode; bit-identical as well)
  const int dma = hlp_dma_mode();
  if (!km && !segd && splits == 1 && nbatch == 1 && big && hlp_enabled() &&
      a->K >= (dma ? 3 * HBK + 1 : 5 * HBK)) {
    const int ncu = hlp_num_cu();
    grid_p = ncu / 8 * 8;
    if (grid_p >= 8 && (total >= 2 * grid_p || dma == 2)) ctl = hlp_control_block(stream);
  }
  if (ctl) {
    const size_t shm_p = shm + 16;
    auto kern_p = dma ? gemm_hlp_kernel<4, 4, 2, true> : gemm_hlp_kernel<4, 4, 2, false>;
    ASR_CHECK_HIP(set_dynamic_lds_once((const void*)kern_p, shm_p));
    hipLaunchKernelGGL(kern_p, dim3(grid_p), dim3(512), shm_p, stream, A, B, a->M, a->N, a->K, ep,
                       a->a_scale, a->b_scale, ctl);
  } else {
    // the k_major big tile: DMA-staged (its own LDS image, 128 KB) unless switched off or the
    // reduction range of a split is shorter than its prologue
    const bool km_dma = km && big && kps >= kKmDmaMinSlabs * HBK && a->K >= kKmDmaMinSlabs * HBK &&
                        km_dma_enabled();
    const hlx_t kern_x = km_dma ? gemm_hlt_dma_kernel<4, 4, 2> : kern[vi][vj];
    const size_t shm_x = km_dma ? (size_t)2 * 2 * 4 * 32 * 256 : shm;
    ASR_CHECK_HIP(set_dynamic_lds_once((const void*)kern_x, shm_x));
    hipLaunchKernelGGL(kern_x, dim3(total), dim3(big ? 512 : 256), shm_x, stream, A, B, a->M,
                       a->N, a->K, kps, splits, ep, a->a_scale, a->b_scale, seg);
  }
  ASR_CHECK_LAUNCH();
  if (splits > 1) {
    launch_splitk_reduce(ep.partial, splits, a->M * nbatch, a->N, ep, stream);
    ASR_CHECK_LAUNCH();
  }
  return ASR_OK;
}
