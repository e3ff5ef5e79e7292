// K1-K3 MFCC / log-mel front-end -- gfx950.
//
// Replaces preprocessing/audio.py (FBank/MFCC/LogFbank._call, _postprocessing,
// _standarize) and preprocessing/audio_utils.py (preemphasis, framesig, powspec,
// delta) of the reference; tested against oracle/frontend.py, which is pinned
// bit-for-bit on the reference's own NumPy code.
//
// Kernel 1 (fe_frames_kernel): one 64-lane wave per frame.  Pre-emphasis, zero
//   padded framing and the Hamming window are applied while the 400 samples are
//   read (coalesced); the 512-point real FFT is a 256-point complex radix-4
//   Stockham FFT (4 stages x one butterfly per lane) in LDS plus the real-FFT
//   split; power spectrum, frame energy, the (sparse) triangular mel filters,
//   log and the 13-column DCT (lifter folded into the table) all stay in LDS /
//   registers.  Only T x (13 | nfilt[+1]) base features are written.  This per-frame chain
//   runs in FLOAT64 (tables included): the reference computes in float64, and a float32
//   FFT leaves ~1e-7 x the frame's largest bin as absolute error in every bin, which under
//   a nearly empty narrow mel filter became 3.6e-4 after log and standardisation; in float64
//   the standardised features agree with the reference to ~1e-5 (test bar: 1e-4).  The
//   kernel is ~0.3 ms of a 50 ms step, so the fp64 rate is irrelevant.
// Kernel 2 (fe_finalize_kernel), float64 too (the base features stay float64 in the
//   workspace; only the standardised output is float32): one workgroup per utterance.  Deltas and
//   delta-deltas (edge-replicated, audio_utils.py:153-173), stride / context
//   stacking, per-column mean / population-std (float64 accumulators, wave
//   shuffles + LDS) and the normalised write into the time-major (T, N, F) slab,
//   zero-filled past the utterance (pad_sequences 'post').
#include "common.h"

namespace {

constexpr int NFFT = 512;
constexpr int NBINS = NFFT / 2 + 1;     // 257
constexpr int FRAMES_PER_WAVE = 4;
constexpr int WAVES = 4;
constexpr int FRAMES_PER_BLOCK = FRAMES_PER_WAVE * WAVES;
constexpr double kF64Eps = 2.220446049250313e-16;   // np.finfo(float).eps
constexpr int kMelLd = 128;             // filters per row of the transposed mel table
constexpr int kMelPasses = kMelLd / 64;
// workspace tail: twiddles (385 double2) + the transposed compact mel table (<= 257 rows)
constexpr size_t kTwBytes = 6400;                                // 385 double2 -> multiple of 256
constexpr size_t kMelTBytes = (size_t)NBINS * kMelLd * sizeof(double);

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// Tables of one call: the FFT twiddles, and the mel matrix in the arrangement the frame
// kernel walks: mel_t[i][jf] = mel[jf][lo_jf + i] for i < hi_jf - lo_jf, else 0 (rows up to the
// widest filter; columns up to kMelLd).  One workgroup.
__global__ void __launch_bounds__(256)
fe_prepare_kernel(int num_filt, const double* __restrict__ mel, const int* __restrict__ mel_range,
                  double2* __restrict__ tw_tab, double* __restrict__ mel_t) {
  __shared__ int s_w[256];
  const int tid = threadIdx.x;
  for (int m = tid; m <= 384; m += 256) {
    double s, c;
    sincospi(-(double)m / 256.0, &s, &c);         // angle = -2 pi m / 512
    tw_tab[m] = make_double2(c, s);
  }
  int wmax = 0;
  for (int jf = tid; jf < num_filt; jf += 256) {
    const int wd = mel_range[2 * jf + 1] - mel_range[2 * jf];
    wmax = wd > wmax ? wd : wmax;
  }
  s_w[tid] = wmax;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) s_w[tid] = s_w[tid] > s_w[tid + st] ? s_w[tid] : s_w[tid + st];
    __syncthreads();
  }
  wmax = s_w[0] < NBINS ? s_w[0] : NBINS;
  for (int e = tid; e < wmax * kMelLd; e += 256) {
    const int i = e / kMelLd, jf = e % kMelLd;
    double v = 0.0;
    if (jf < num_filt) {
      const int lo = mel_range[2 * jf], hi = mel_range[2 * jf + 1];
      if (lo + i < hi && lo + i < NBINS) v = mel[(size_t)jf * NBINS + lo + i];
    }
    mel_t[e] = v;
  }
}

__global__ void __launch_bounds__(256)
fe_frames_kernel(asr_frontend_cfg cfg, const float* __restrict__ audio,
                 const int* __restrict__ offsets, const int* __restrict__ lengths,
                 const double* __restrict__ window, const double* __restrict__ mel,
                 const int* __restrict__ mel_range, const double* __restrict__ dct,
                 double* __restrict__ base, int max_frames, int fb,
                 const double2* __restrict__ tw_tab, const double* __restrict__ mel_t,
                 int has_prev, const int* __restrict__ frame_count) {
  // has_prev / frame_count are the resumed form's (asr_frontend_stream): the sample in front of
  // an utterance's first one exists (at audio[off - 1]: the pre-emphasis of sample 0 reads it),
  // and utterance u computes frame_count[u] frames, not the zero-padded count of its length.
  __shared__ double2 tw[384 + 1];                // e^{-2 pi i m / 512}, m = 0..384
  __shared__ double2 buf[WAVES][2][256];         // ping-pong complex buffers
  __shared__ double pspec[WAVES][NBINS + 3];
  __shared__ double lmel[WAVES][128];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int utt = blockIdx.y;
  const int len = lengths[utt];
  const int off = offsets[utt];
  int nframes = 1;
  if (len > cfg.frame_len)
    nframes = 1 + (len - cfg.frame_len + cfg.frame_step - 1) / cfg.frame_step;
  if (frame_count) nframes = frame_count[utt];
  const int f_block = blockIdx.x * FRAMES_PER_BLOCK;
  if (f_block >= nframes) return;                 // uniform per block

  for (int m = tid; m <= 384; m += 256) tw[m] = tw_tab[m];    // (fe_prepare_kernel)
  // this lane's mel filters (lane, lane + 64): first bin, width, and the width the wave
  // walks (its widest filter): the same for every frame
  int mlo[kMelPasses], mwave[kMelPasses];
#pragma unroll
  for (int ps = 0; ps < kMelPasses; ++ps) {
    const int jf = lane + 64 * ps;
    const bool has = jf < cfg.num_filt;
    mlo[ps] = has ? mel_range[2 * jf] : 0;
    const int width = has ? mel_range[2 * jf + 1] - mlo[ps] : 0;
    mwave[ps] = __builtin_amdgcn_readfirstlane((int)asr_wave_max((float)width));
  }
  __syncthreads();

  double* real_in = reinterpret_cast<double*>(&buf[w][0][0]);   // 512 reals == 256 complex
  // The samples of a frame (and their predecessors, for the pre-emphasis) are fetched into
  // registers one frame AHEAD: the loads of frame fi + 1 fly under the FFT of frame fi.  (Loaded
  // where they were used, a frame waited for 8 dependent round trips to HBM / L2: 11 us per
  // frame and wave, most of the kernel.)
  float xs[NFFT / 64], xq[NFFT / 64];
  auto fetch = [&](int f) {
    const int s0 = f * cfg.frame_step;
    const bool live = f < nframes;
#pragma unroll
    for (int q = 0; q < NFFT / 64; ++q) {
      const int i = lane + 64 * q, idx = s0 + i;
      const bool in = live && i < cfg.frame_len && idx < len;
      xs[q] = in ? audio[off + idx] : 0.f;
      xq[q] = (in && (idx > 0 || has_prev)) ? audio[off + idx - 1] : 0.f;
    }
  };
  fetch(f_block + w * FRAMES_PER_WAVE);
  for (int fi = 0; fi < FRAMES_PER_WAVE; ++fi) {
    const int f = f_block + w * FRAMES_PER_WAVE + fi;
    const bool live = f < nframes;
    // ---- pre-emphasis + window (zero padded to 512)
    const int s0 = f * cfg.frame_step;
#pragma unroll
    for (int q = 0; q < NFFT / 64; ++q) {
      const int i = lane + 64 * q, idx = s0 + i;
      double v = 0.0;
      if (live && i < cfg.frame_len && idx < len) {
        const double x = (double)xs[q], xp = (double)xq[q];
        v = ((idx > 0 || has_prev) ? x - cfg.pre_emph * xp : x) * window[i];
      }
      real_in[i] = v;
    }
    if (fi + 1 < FRAMES_PER_WAVE) fetch(f + 1);
    __syncthreads();
    // ---- 256-point complex FFT, radix-4 Stockham, Ns = 1, 4, 16, 64
    int cur = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int Ns = 1 << (2 * s);
      const double2* in = buf[w][cur];
      double2* out = buf[w][cur ^ 1];
      const int j = lane;
      const int k = j & (Ns - 1);
      double2 v0 = in[j], v1 = in[j + 64], v2 = in[j + 128], v3 = in[j + 192];
      if (s > 0) {
        const int tstep = (128 / Ns) * k;        // index into tw (512-based): 2*(64/Ns)*k
        v1 = cmul(v1, tw[tstep]);
        v2 = cmul(v2, tw[2 * tstep]);
        v3 = cmul(v3, tw[3 * tstep]);
      }
      const double2 t0 = make_double2(v0.x + v2.x, v0.y + v2.y);
      const double2 t1 = make_double2(v0.x - v2.x, v0.y - v2.y);
      const double2 t2 = make_double2(v1.x + v3.x, v1.y + v3.y);
      const double2 d = make_double2(v1.x - v3.x, v1.y - v3.y);
      const double2 t3 = make_double2(d.y, -d.x);  // -i * (v1 - v3)
      const int base_idx = ((j - k) << 2) + k;   // (j / Ns) * Ns * 4 + k
      out[base_idx] = make_double2(t0.x + t2.x, t0.y + t2.y);
      out[base_idx + Ns] = make_double2(t1.x + t3.x, t1.y + t3.y);
      out[base_idx + 2 * Ns] = make_double2(t0.x - t2.x, t0.y - t2.y);
      out[base_idx + 3 * Ns] = make_double2(t1.x - t3.x, t1.y - t3.y);
      cur ^= 1;
      __syncthreads();
    }
    // ---- real-FFT split + power spectrum / nfft, frame energy
    const double2* Z = buf[w][cur];
    double esum = 0.0;
    for (int k = lane; k < NBINS; k += 64) {
      const double2 zk = Z[k & 255];
      const double2 zc = Z[(256 - k) & 255];
      const double2 zn = make_double2(zc.x, -zc.y);                 // conj
      const double2 e = make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y + zn.y));
      const double2 dd = make_double2(zk.x - zn.x, zk.y - zn.y);
      const double2 o = make_double2(0.5 * dd.y, -0.5 * dd.x);      // -i/2 * (zk - zn)
      const double2 wo = cmul(tw[k], o);
      const double xr = e.x + wo.x, xi = e.y + wo.y;
      const double p = (xr * xr + xi * xi) * (1.0 / NFFT);
      pspec[w][k] = p;
      esum += p;
    }
    esum = asr_wave_sum_d(esum);
    if (esum == 0.0) esum = kF64Eps;
    __syncthreads();
    // ---- mel filterbank (triangles are sparse: only [lo, hi) bins) + log
    // filter jf = sum over its bins lo .. hi-1, in that order; the weights come from the
    // transposed compact table mel_t[i][jf] = mel[jf][lo + i] (0 from the filter's width on:
    // adding x * 0 changes nothing), so that the loop is uniform over the wave, its loads
    // coalesced and independent of each other (the per-lane `for k in [lo, hi)` over the dense
    // rows was a chain of dependent L1 round trips: the slowest part of the kernel)
#pragma unroll
    for (int ps = 0; ps < kMelPasses; ++ps) {
      const int jf = lane + 64 * ps;
      if (64 * ps >= cfg.num_filt) break;
      double acc = 0.0;
      const double* wt = mel_t + jf;
#pragma unroll 4
      for (int i = 0; i < mwave[ps]; ++i) {
        int k = mlo[ps] + i;
        k = k < NBINS ? k : NBINS - 1;
        acc += pspec[w][k] * wt[(size_t)i * kMelLd];
      }
      if (jf < cfg.num_filt) {
        if (acc == 0.0) acc = kF64Eps;
        lmel[w][jf] = log(acc);
      }
    }
    __syncthreads();
    // ---- write base features
    if (live) {
      double* row = base + ((size_t)utt * max_frames + f) * fb;
      const double le = log(esum + cfg.eps);
      if (cfg.kind == 0) {
        for (int c = lane; c < cfg.num_cep; c += 64) {
          double acc = 0.0;
          for (int jf = 0; jf < cfg.num_filt; ++jf)
            acc += lmel[w][jf] * dct[jf * cfg.num_cep + c];
          if (c == 0 && cfg.append_energy) acc = le;
          row[c] = acc;
        }
      } else {
        for (int c = lane; c < cfg.num_filt; c += 64) row[c] = lmel[w][c];
        if (cfg.append_energy && lane == 0) row[cfg.num_filt] = le;
      }
    }
    __syncthreads();
  }
}

// full[t][0:fb] = base, [fb:2fb] = delta, [2fb:3fb] = delta-delta
__device__ __forceinline__ double delta_at(const double* __restrict__ x, int ld, int T, int t,
                                           int c) {
  // sum_{n=-2..2} n * x[clamp(t+n)] / 10, same association order as the reference
  double acc = 0.0;
#pragma unroll
  for (int n = -2; n <= 2; ++n) {
    int tt = t + n;
    tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
    acc += (double)n * x[(size_t)tt * ld + c];
  }
  return acc / 10.0;
}

// Workgroup (utterance, block of CX output columns): 1024 / CX row walkers per column.  (One
// workgroup per utterance walked 62 rows per thread and pass on 64 of the 256 CUs.)  CX = 16
// for wide outputs (64-byte runs of the slab rows: 80 log-mel columns 141 -> 39 us), 8 for
// narrow ones (more workgroups: 39 MFCC columns 69 -> 36 us).
constexpr int kFinalizeThreads = 1024;

template <int CX>
__global__ void __launch_bounds__(1024)
fe_finalize_kernel(asr_frontend_cfg cfg, const int* __restrict__ lengths,
                   double* __restrict__ full, int max_frames, int fb, int ffull,
                   float* __restrict__ out, int t_out, int n_pad, int f_out,
                   int* __restrict__ out_frames) {
  constexpr int TY = kFinalizeThreads / CX;
  const int utt = blockIdx.x;
  const int c0 = blockIdx.y * CX;
  const int tid = threadIdx.x;
  const int cx = tid % CX, ty = tid / CX;
  const int len = lengths[utt];
  int T = 1;
  if (len > cfg.frame_len) T = 1 + (len - cfg.frame_len + cfg.frame_step - 1) / cfg.frame_step;
  if (T > max_frames) T = max_frames;
  double* x = full + (size_t)utt * max_frames * ffull;
  const int col = c0 + cx;                    // this thread's output column
  const int cfull = col % ffull;              // ... is column cfull of the (base | d | dd) rows
  // ---- deltas of the columns this workgroup reads (global scratch, visible block-wide after
  // the barriers).  A delta-delta column needs its delta column, which another workgroup may
  // own: this one computes it as well (workgroups that share a column write equal values).
  if (cfg.d) {
    const bool mine = col < f_out && cfull >= fb;
    const int dcol = cfull >= 2 * fb ? cfull - fb : cfull;        // the delta column involved
    if (mine)
      for (int t = ty; t < T; t += TY) x[(size_t)t * ffull + dcol] = delta_at(x, ffull, T, t, dcol - fb);
    __syncthreads();
    if (mine && cfull >= 2 * fb)
      for (int t = ty; t < T; t += TY)
        x[(size_t)t * ffull + cfull] = delta_at(x + fb, ffull, T, t, cfull - 2 * fb);
    __syncthreads();
  }
  const int stride = cfg.stride < 1 ? 1 : cfg.stride;
  const int Ts = (T + stride - 1) / stride;       // frames after feats[::stride]
  auto get = [&](int ts) -> double {
    const int cslot = col / ffull;
    const int src = ts + cslot - cfg.num_context;
    if (src < 0 || src >= Ts) return 0.0;
    return x[(size_t)(src * stride) * ffull + cfull];
  };
  // ---- column statistics: thread (cx, ty) walks t = ty, ty+TY, ... of column c0 + cx
  __shared__ double s_sum[TY][CX];
  __shared__ double s_sq[TY][CX];
  __shared__ double s_mx[TY][CX];
  __shared__ double s_mean[CX];
  __shared__ double s_inv[CX];
  double sum = 0.0, mn = 1e300, mx = -1e300;
  if (col < f_out)
    for (int ts = ty; ts < Ts; ts += TY) {
      const double v = get(ts);
      sum += v;
      mn = v < mn ? v : mn;
      mx = v > mx ? v : mx;
    }
  s_sum[ty][cx] = sum;
  s_sq[ty][cx] = mn;            // (s_sq doubles as scratch for the column minimum ...)
  s_mx[ty][cx] = mx;
  __syncthreads();
  double mean = 0.0;
  if (col < f_out) {
    double tot = 0.0, lo = 1e300, hi = -1e300;
    for (int i = 0; i < TY; ++i) {
      tot += s_sum[i][cx];
      lo = s_sq[i][cx] < lo ? s_sq[i][cx] : lo;
      hi = s_mx[i][cx] > hi ? s_mx[i][cx] : hi;
    }
    // a constant column (an empty mel filter: log(eps) in every frame) has exactly its
    // value as mean -- NumPy's pairwise sum of equal terms is exact there -- so that it
    // standardises to exactly 0
    mean = lo == hi ? lo : tot / Ts;
  }
  __syncthreads();              // (... before s_sq is reused for the squares)
  double sq = 0.0;
  if (col < f_out)
    for (int ts = ty; ts < Ts; ts += TY) {
      const double dlt = get(ts) - mean;
      sq += dlt * dlt;
    }
  s_sq[ty][cx] = sq;
  __syncthreads();
  if (ty == 0 && col < f_out) {
    double tot = 0.0;
    for (int i = 0; i < TY; ++i) tot += s_sq[i][cx];
    const double var = tot / Ts;
    s_mean[cx] = cfg.mean_norm ? mean : 0.0;
    // (without mean_norm the std is still taken about the true mean -- np.std -- only the
    // shift is skipped)
    const double sd = sqrt(var);
    s_inv[cx] = cfg.var_norm ? sd + cfg.eps : 1.0;     // the divisor (audio.py:70-75)
  }
  __syncthreads();
  if (col < f_out) {
    const double mu = s_mean[cx], den = s_inv[cx];
    for (int ts = ty; ts < t_out; ts += TY) {
      float v = 0.f;
      if (ts < Ts) v = (float)((get(ts) - mu) / den);
      out[((size_t)ts * n_pad + utt) * f_out + col] = v;
    }
  }
  if (tid == 0 && blockIdx.y == 0 && out_frames) out_frames[utt] = Ts < t_out ? Ts : t_out;
}

__global__ void fe_zero_pad_rows_kernel(float* __restrict__ out, int t_out, int n_utt,
                                        int n_pad, int f_out) {
  // rows n in [n_utt, n_pad) of every time step are batch padding: zero them.
  const int padn = n_pad - n_utt;
  const size_t total = (size_t)t_out * padn * f_out;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % f_out);
    const size_t r = e / f_out;
    const int n = n_utt + (int)(r % padn);
    const int t = (int)(r / padn);
    out[((size_t)t * n_pad + n) * f_out + c] = 0.f;
  }
}

int base_cols(const asr_frontend_cfg* cfg) {
  return cfg->kind == 0 ? cfg->num_cep : cfg->num_filt + (cfg->append_energy ? 1 : 0);
}

// ------------------------------------------------------------------------------------------
// Running (causal) normalisation, norm_mode = 1, and the resumed front-end.
//
// Both forms -- the batch call over a whole utterance and asr_frontend_stream over the frames
// that became final in one call -- walk the kept frames of one (utterance, output column) in
// order, one thread each, through fe_value_at and fe_running_step.  They differ only in where a
// base-feature row comes from: the workspace of the call (FeRowsBatch), or the ring of the last
// 2 la + 1 rows of the stream and the rows the call computed (FeRowsStream).
struct FeRowsBatch {
  const double* x;
  int ld;
  __device__ __forceinline__ double at(int r, int b) const { return x[(size_t)r * ld + b]; }
};

struct FeRowsStream {
  const double* ring;      // row r < c0 at ring[r % R]
  const double* fresh;     // row r >= c0 at fresh[r - c0]
  int c0, R, fb;
  __device__ __forceinline__ double at(int r, int b) const {
    return r >= c0 ? fresh[(size_t)(r - c0) * fb + b] : ring[(size_t)(r % R) * fb + b];
  }
};

// delta_at over a row accessor.  n * x is exact for n = -2 .. 2, so that a contraction of
// acc + n * x into an fma cannot change a bit: both forms give the same value.
template <class Rows>
__device__ __forceinline__ double fe_delta5(const Rows& rows, int T, int t, int b) {
  double acc = 0.0;
#pragma unroll
  for (int n = -2; n <= 2; ++n) {
    int tt = t + n;
    tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
    acc += (double)n * rows.at(tt, b);
  }
  return acc / 10.0;
}

// Column (part, b) of frame t of the (base | delta | delta-delta) row of an utterance of T
// frames, from its base rows alone (edge-replicated at 0 and T - 1 like delta_at).
template <class Rows>
__device__ __forceinline__ double fe_value_at(const Rows& rows, int T, int t, int part, int b) {
  if (part == 0) return rows.at(t, b);
  if (part == 1) return fe_delta5(rows, T, t, b);
  double acc = 0.0;
#pragma unroll
  for (int n = -2; n <= 2; ++n) {
    int tt = t + n;
    tt = tt < 0 ? 0 : (tt >= T ? T - 1 : tt);
    acc += (double)n * fe_delta5(rows, T, tt, b);
  }
  return acc / 10.0;
}

// One step of Welford's recursion and the normalised value of kept frame n - 1.  The product
// and the sum of the M2 update are rounded separately (__dmul_rn / __dadd_rn are never
// contracted), as NumPy rounds them.
__device__ __forceinline__ float fe_running_step(double x, double n, double& mean, double& m2,
                                                 int mean_norm, int var_norm, double eps) {
  const double dlt = x - mean;
  mean = mean + dlt / n;
  m2 = __dadd_rn(m2, __dmul_rn(dlt, x - mean));
  const double sd = sqrt(m2 / n);
  return (float)((x - (mean_norm ? mean : 0.0)) / (var_norm ? sd + eps : 1.0));
}

// Workgroup = one wave: 64 adjacent output columns of one utterance (coalesced workspace reads
// and slab writes); each thread walks its column's kept frames in order.
__global__ void __launch_bounds__(64)
fe_finalize_running_kernel(asr_frontend_cfg cfg, const int* __restrict__ lengths,
                           const double* __restrict__ full, int max_frames, int fb, int ffull,
                           float* __restrict__ out, int t_out, int n_pad, int f_out,
                           int* __restrict__ out_frames) {
  const int utt = blockIdx.y;
  const int col = blockIdx.x * 64 + threadIdx.x;
  const int len = lengths[utt];
  int T = 1;
  if (len > cfg.frame_len) T = 1 + (len - cfg.frame_len + cfg.frame_step - 1) / cfg.frame_step;
  if (T > max_frames) T = max_frames;
  const int stride = cfg.stride < 1 ? 1 : cfg.stride;
  const int Ts = (T + stride - 1) / stride;
  const int lim = Ts < t_out ? Ts : t_out;
  if (col < f_out) {
    const FeRowsBatch rows{full + (size_t)utt * max_frames * ffull, ffull};
    const int part = col / fb, b = col % fb;
    double mean = 0.0, m2 = 0.0;
    for (int ts = 0; ts < lim; ++ts) {
      const double x = fe_value_at(rows, T, ts * stride, part, b);
      out[((size_t)ts * n_pad + utt) * f_out + col] =
          fe_running_step(x, (double)(ts + 1), mean, m2, cfg.mean_norm, cfg.var_norm, cfg.eps);
    }
    for (int ts = lim; ts < t_out; ++ts) out[((size_t)ts * n_pad + utt) * f_out + col] = 0.f;
  }
  if (col == 0 && out_frames) out_frames[utt] = lim;
}

// ---- the resumed front-end.  Device state of n_streams streams (each part 256-byte aligned):
//   counters  int   [N][4]           valid samples seen, base frames computed, kept rows emitted
//   carry     float [N][L]           [0] the sample in front of the carry, [1 ..] the carry
//   ring      double[N][R][fb]       base rows r of the last R = 2 la + 1 at slot r % R
//   stats     double[N][2][f_out]    mean and M2 of every output column
//   tw, mel_t                        fe_prepare_kernel's tables (built by the reset)
struct FeStreamLayout {
  int L, R, fb, f_out, la;
  size_t counters, carry, ring, stats, tw, melt, total;
};

FeStreamLayout fe_stream_layout(const asr_frontend_cfg* cfg, int n) {
  FeStreamLayout l;
  l.L = cfg->frame_len;
  l.la = 2 * (cfg->d ? 1 : 0) + 2 * ((cfg->d && cfg->dd) ? 1 : 0);
  l.R = 2 * l.la + 1;
  l.fb = base_cols(cfg);
  l.f_out = l.fb * (1 + (cfg->d ? 1 : 0) + ((cfg->d && cfg->dd) ? 1 : 0));
  size_t o = 0;
  l.counters = o; o += asr_align_up((size_t)n * 4 * sizeof(int), 256);
  l.carry = o;    o += asr_align_up((size_t)n * l.L * sizeof(float), 256);
  l.ring = o;     o += asr_align_up((size_t)n * l.R * l.fb * sizeof(double), 256);
  l.stats = o;    o += asr_align_up((size_t)n * 2 * l.f_out * sizeof(double), 256);
  l.tw = o;       o += kTwBytes;
  l.melt = o;     o += kMelTBytes;
  l.total = o;
  return l;
}

__host__ __device__ inline int fe_complete_frames(int s, int frame_len, int frame_step) {
  return s < frame_len ? 0 : 1 + (s - frame_len) / frame_step;
}

__host__ __device__ inline int fe_padded_frames(int s, int frame_len, int frame_step) {
  return s <= frame_len ? 1 : 1 + (s - frame_len + frame_step - 1) / frame_step;
}

// The signal of this call per stream, contiguous: [predecessor | carry | new valid samples], and
// the plan {c0, c1, carry_len, new_valid} the later kernels of the call read (the counters are
// only written by the commit kernel, after everything has read the plan).
__global__ void __launch_bounds__(256)
fe_stream_gather_kernel(asr_frontend_cfg cfg, const int* __restrict__ counters,
                        const float* __restrict__ carry, const float* __restrict__ audio,
                        int n_samples, const int* __restrict__ ended, int s_before, int s_after,
                        int max_new, float* __restrict__ sig, int sig_ld, int* __restrict__ plan,
                        int* __restrict__ offsets, int* __restrict__ lengths,
                        int* __restrict__ nframes) {
  const int i = blockIdx.y;
  const int L = cfg.frame_len;
  const int seen = counters[4 * i], c0 = counters[4 * i + 1];
  const int n = ended ? ended[i] : -1;
  const bool is_ended = n >= 0 && n <= s_after;
  const int valid_after = is_ended ? n : s_after;
  int new_valid = valid_after - s_before;
  new_valid = new_valid < 0 ? 0 : (new_valid > n_samples ? n_samples : new_valid);
  int carry_len = seen - c0 * cfg.frame_step;
  carry_len = carry_len < 0 ? 0 : (carry_len > L - 1 ? L - 1 : carry_len);
  int c1 = is_ended ? fe_padded_frames(n, L, cfg.frame_step)
                    : fe_complete_frames(s_after, L, cfg.frame_step);
  c1 = c1 < c0 ? c0 : (c1 > c0 + max_new ? c0 + max_new : c1);
  const int total = carry_len + new_valid;
  for (int j = blockIdx.x * 256 + threadIdx.x; j <= total; j += gridDim.x * 256) {
    float v;
    if (j <= carry_len) v = carry[(size_t)i * L + j];
    else v = audio[(size_t)i * n_samples + (j - 1 - carry_len)];
    sig[(size_t)i * sig_ld + j] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    plan[4 * i] = c0;
    plan[4 * i + 1] = c1;
    plan[4 * i + 2] = carry_len;
    plan[4 * i + 3] = new_valid;
    offsets[i] = i * sig_ld + 1;
    lengths[i] = total;
    nframes[i] = c1 - c0;
  }
}

// The kept frames [lo, hi) (unstrided indices) of every stream into out rows 0 ..: a frame the
// stream does not have (past its end) is a zero row.
__global__ void __launch_bounds__(64)
fe_stream_finalize_kernel(asr_frontend_cfg cfg, const int* __restrict__ ended,
                          const int* __restrict__ plan, const double* __restrict__ ring,
                          const double* __restrict__ fresh, int max_new, int fb, int R, int la,
                          double* __restrict__ stats, float* __restrict__ out, int n_pad,
                          int f_out, int lo, int hi, int s_after) {
  const int i = blockIdx.y;
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col >= f_out) return;
  const int c0 = plan[4 * i], c1 = plan[4 * i + 1];
  const int n = ended ? ended[i] : -1;
  const bool is_ended = n >= 0 && n <= s_after;
  const int avail = is_ended ? c1 : c1 - la;
  const FeRowsStream rows{ring + (size_t)i * R * fb, fresh + (size_t)i * max_new * fb, c0, R, fb};
  const int part = col / fb, b = col % fb;
  const int stride = cfg.stride < 1 ? 1 : cfg.stride;
  double* st = stats + (size_t)i * 2 * f_out;
  double mean = st[col], m2 = st[f_out + col];
  const int t0 = (lo + stride - 1) / stride;
  for (int ts = t0; ts * stride < hi; ++ts) {
    const int f = ts * stride;
    float v = 0.f;
    if (f < avail)
      v = fe_running_step(fe_value_at(rows, c1, f, part, b), (double)(ts + 1), mean, m2,
                          cfg.mean_norm, cfg.var_norm, cfg.eps);
    out[((size_t)(ts - t0) * n_pad + i) * f_out + col] = v;
  }
  st[col] = mean;
  st[f_out + col] = m2;
}

// What the next call resumes from: the samples behind the last computed frame's step, the one in
// front of them, the last R base rows, the counters.
__global__ void __launch_bounds__(256)
fe_stream_commit_kernel(asr_frontend_cfg cfg, const int* __restrict__ ended,
                        const int* __restrict__ plan, const float* __restrict__ sig, int sig_ld,
                        const double* __restrict__ fresh, int max_new, int fb, int R, int la,
                        int* __restrict__ counters, float* __restrict__ carry,
                        double* __restrict__ ring, int s_after, int hi) {
  const int i = blockIdx.y;
  const int L = cfg.frame_len;
  const int c0 = plan[4 * i], c1 = plan[4 * i + 1];
  const int total = plan[4 * i + 2] + plan[4 * i + 3];
  const int adv = (c1 - c0) * cfg.frame_step;
  int keep = total - adv;
  keep = keep < 0 ? 0 : (keep > L - 1 ? L - 1 : keep);
  const int gtid = blockIdx.x * 256 + threadIdx.x, gs = gridDim.x * 256;
  for (int j = gtid; j <= keep; j += gs)
    carry[(size_t)i * L + j] = adv + j <= total ? sig[(size_t)i * sig_ld + adv + j] : 0.f;
  const int nr = c1 - c0 < R ? c1 - c0 : R;
  for (int e = gtid; e < nr * fb; e += gs) {
    const int r = c1 - nr + e / fb, b = e % fb;
    ring[((size_t)i * R + r % R) * fb + b] = fresh[((size_t)i * max_new + (r - c0)) * fb + b];
  }
  if (gtid == 0) {
    const int n = ended ? ended[i] : -1;
    const bool is_ended = n >= 0 && n <= s_after;
    const int stride = cfg.stride < 1 ? 1 : cfg.stride;
    int avail = is_ended ? c1 : c1 - la;
    avail = avail < hi ? avail : hi;
    counters[4 * i] = is_ended ? n : s_after;
    counters[4 * i + 1] = c1;
    counters[4 * i + 2] = avail > 0 ? (avail + stride - 1) / stride : 0;
  }
}

int fe_check_cfg(const asr_frontend_cfg* cfg, bool has_dct) {
  ASR_CHECK_ARG(cfg->nfft == NFFT, "frontend: nfft must be 512 (got %d)", cfg->nfft);
  ASR_CHECK_ARG(cfg->frame_len > 0 && cfg->frame_len <= NFFT && cfg->frame_step > 0,
                "frontend: bad frame_len/frame_step");
  ASR_CHECK_ARG(cfg->num_filt > 0 && cfg->num_filt <= 128, "frontend: num_filt > 128");
  ASR_CHECK_ARG(cfg->kind == 1 || (cfg->num_cep > 0 && cfg->num_cep <= 64 && has_dct),
                "frontend: bad num_cep / missing dct");
  ASR_CHECK_ARG(cfg->norm_mode == 0 || cfg->norm_mode == 1,
                "frontend: norm_mode %d (0 = utterance, 1 = running)", cfg->norm_mode);
  ASR_CHECK_ARG(cfg->norm_mode == 0 || cfg->num_context == 0,
                "frontend: running normalisation does not take context stacking "
                "(num_context %d)", cfg->num_context);
  return ASR_OK;
}

// host_state (int64): [0] samples fed, [1] first frame not yet emitted, [2] kept rows emitted,
// [3] n_streams; per stream [4 + 2 i] its length (-1: not ended), [5 + 2 i] frames computed
constexpr int kHostHead = 4;

}  // namespace

extern "C" int asr_frontend_num_frames(int samples, int frame_len, int frame_step) {
  if (samples <= frame_len) return 1;
  return 1 + (samples - frame_len + frame_step - 1) / frame_step;
}

extern "C" int asr_frontend_num_feats(const asr_frontend_cfg* cfg) {
  return base_cols(cfg) * (1 + (cfg->d ? 1 : 0) + ((cfg->d && cfg->dd) ? 1 : 0));
}

extern "C" size_t asr_frontend_workspace_bytes(const asr_frontend_cfg* cfg, int n_utt,
                                               int max_frames) {
  return asr_align_up((size_t)n_utt * max_frames * asr_frontend_num_feats(cfg) *
                          sizeof(double), 256) + kTwBytes + kMelTBytes;
}

extern "C" int asr_frontend_features(const asr_frontend_cfg* cfg, const float* audio,
                                     const int* offsets, const int* lengths,
                                     const int* host_lengths, int n_utt, int n_pad,
                                     const double* window, const double* mel,
                                     const int* mel_range, const double* dct,
                                     float* out, int t_out, int* out_frames,
                                     void* workspace, size_t ws_bytes,
                                     asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(cfg && audio && offsets && lengths && host_lengths && window && mel &&
                    mel_range && out && workspace, "frontend: null pointer");
  if (const int rc = fe_check_cfg(cfg, dct != nullptr)) return rc;
  ASR_CHECK_ARG(n_utt > 0 && n_pad >= n_utt && t_out > 0, "frontend: bad batch shape");
  int max_frames = 1;
  for (int i = 0; i < n_utt; ++i) {
    ASR_CHECK_ARG(host_lengths[i] > 1, "frontend: utterance %d has < 2 samples", i);
    const int nf = asr_frontend_num_frames(host_lengths[i], cfg->frame_len, cfg->frame_step);
    if (nf > max_frames) max_frames = nf;
  }
  const int fb = base_cols(cfg);
  const int ffull = asr_frontend_num_feats(cfg);
  const int f_out = ffull * (2 * cfg->num_context + 1);
  const size_t need = asr_frontend_workspace_bytes(cfg, n_utt, max_frames);
  if (ws_bytes < need) {
    asr_set_error("frontend: workspace %zu < %zu bytes", ws_bytes, need);
    return ASR_ERR_WORKSPACE;
  }
  double* full = reinterpret_cast<double*>(workspace);
  char* tail = reinterpret_cast<char*>(workspace) + (need - kTwBytes - kMelTBytes);
  double2* tw_tab = reinterpret_cast<double2*>(tail);
  double* mel_t = reinterpret_cast<double*>(tail + kTwBytes);
  hipLaunchKernelGGL(fe_prepare_kernel, dim3(1), dim3(256), 0, stream, cfg->num_filt, mel,
                     mel_range, tw_tab, mel_t);
  ASR_CHECK_LAUNCH();
  dim3 grid((max_frames + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK, n_utt);
  hipLaunchKernelGGL(fe_frames_kernel, grid, dim3(256), 0, stream, *cfg, audio, offsets,
                     lengths, window, mel, mel_range, dct, full, max_frames, ffull, tw_tab, mel_t, 0,
                     (const int*)nullptr);
  ASR_CHECK_LAUNCH();
  if (cfg->norm_mode == 1)
    hipLaunchKernelGGL(fe_finalize_running_kernel, dim3((f_out + 63) / 64, n_utt), dim3(64), 0,
                       stream, *cfg, lengths, full, max_frames, fb, ffull, out, t_out, n_pad,
                       f_out, out_frames);
  else if (f_out >= 64)
    hipLaunchKernelGGL(fe_finalize_kernel<16>, dim3(n_utt, (f_out + 15) / 16),
                       dim3(kFinalizeThreads), 0, stream, *cfg, lengths, full, max_frames, fb,
                       ffull, out, t_out, n_pad, f_out, out_frames);
  else
    hipLaunchKernelGGL(fe_finalize_kernel<8>, dim3(n_utt, (f_out + 7) / 8),
                       dim3(kFinalizeThreads), 0, stream, *cfg, lengths, full, max_frames, fb,
                       ffull, out, t_out, n_pad, f_out, out_frames);
  ASR_CHECK_LAUNCH();
  if (n_pad > n_utt) {
    hipLaunchKernelGGL(fe_zero_pad_rows_kernel, dim3(256), dim3(256), 0, stream, out, t_out,
                       n_utt, n_pad, f_out);
    ASR_CHECK_LAUNCH();
  }
  return ASR_OK;
}

// ------------------------------------------------------------------------ the resumed form
namespace {

int fe_stream_check_cfg(const asr_frontend_cfg* cfg, int n_streams) {
  ASR_CHECK_ARG(cfg, "frontend stream: null cfg");
  if (const int rc = fe_check_cfg(cfg, true)) return rc;     // (the call checks its dct itself)
  ASR_CHECK_ARG(cfg->norm_mode == 1,
                "frontend stream: norm_mode must be 1 (running): whole-utterance statistics "
                "need the end of the utterance");
  ASR_CHECK_ARG(cfg->frame_step <= cfg->frame_len,
                "frontend stream: frame_step %d > frame_len %d", cfg->frame_step, cfg->frame_len);
  ASR_CHECK_ARG(n_streams > 0, "frontend stream: n_streams %d", n_streams);
  return ASR_OK;
}

// most frames one call of n_samples new samples can complete for a stream
int fe_stream_frame_cap(const asr_frontend_cfg* cfg, int n_samples) {
  return (cfg->frame_len - 1 + n_samples) / cfg->frame_step + 2;
}

struct FeStreamWs {
  size_t sig, ints, fresh, total;
  int sig_ld, cap;
};

FeStreamWs fe_stream_ws(const asr_frontend_cfg* cfg, int n, int n_samples) {
  FeStreamWs w;
  w.sig_ld = cfg->frame_len + n_samples;
  w.cap = fe_stream_frame_cap(cfg, n_samples);
  size_t o = 0;
  w.sig = o;   o += asr_align_up((size_t)n * w.sig_ld * sizeof(float), 256);
  w.ints = o;  o += asr_align_up((size_t)n * 7 * sizeof(int), 256);
  w.fresh = o; o += asr_align_up((size_t)n * w.cap * base_cols(cfg) * sizeof(double), 256);
  w.total = o;
  return w;
}

}  // namespace

extern "C" size_t asr_frontend_stream_state_bytes(const asr_frontend_cfg* cfg, int n_streams) {
  if (!cfg || n_streams < 1) return 0;
  return fe_stream_layout(cfg, n_streams).total;
}

extern "C" int asr_frontend_stream_host_ints(int n_streams) {
  return n_streams < 1 ? 0 : kHostHead + 2 * n_streams;
}

extern "C" size_t asr_frontend_stream_workspace_bytes(const asr_frontend_cfg* cfg, int n_streams,
                                                      int n_samples) {
  if (!cfg || n_streams < 1 || n_samples < 0 || cfg->frame_step < 1) return 0;
  return fe_stream_ws(cfg, n_streams, n_samples).total;
}

extern "C" int asr_frontend_stream_reset(const asr_frontend_cfg* cfg, void* state,
                                         long long* host_state, int n_streams,
                                         const double* mel, const int* mel_range,
                                         asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = fe_stream_check_cfg(cfg, n_streams)) return rc;
  ASR_CHECK_ARG(state && host_state && mel && mel_range, "frontend stream: null pointer");
  const FeStreamLayout l = fe_stream_layout(cfg, n_streams);
  char* base = reinterpret_cast<char*>(state);
  ASR_CHECK_HIP(hipMemsetAsync(state, 0, l.tw, stream));
  hipLaunchKernelGGL(fe_prepare_kernel, dim3(1), dim3(256), 0, stream, cfg->num_filt, mel,
                     mel_range, reinterpret_cast<double2*>(base + l.tw),
                     reinterpret_cast<double*>(base + l.melt));
  ASR_CHECK_LAUNCH();
  host_state[0] = host_state[1] = host_state[2] = 0;
  host_state[3] = n_streams;
  for (int i = 0; i < n_streams; ++i) {
    host_state[kHostHead + 2 * i] = -1;
    host_state[kHostHead + 2 * i + 1] = 0;
  }
  return ASR_OK;
}

extern "C" int asr_frontend_stream(const asr_frontend_cfg* cfg, void* state,
                                   long long* host_state, const float* audio, int n_samples,
                                   const int* ended_total, const int* host_ended_total,
                                   int n_streams, int n_pad, const double* window,
                                   const double* mel, const int* mel_range, const double* dct,
                                   float* out, int t_cap, int* frames_lo, int* frames_hi,
                                   void* workspace, size_t ws_bytes, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (const int rc = fe_stream_check_cfg(cfg, n_streams)) return rc;
  ASR_CHECK_ARG(state && host_state && window && mel && mel_range && frames_lo && frames_hi &&
                    workspace && (cfg->kind == 1 || dct), "frontend stream: null pointer");
  ASR_CHECK_ARG(n_samples >= 0 && (n_samples == 0 || audio), "frontend stream: bad audio");
  ASR_CHECK_ARG(n_pad >= n_streams && t_cap >= 0 && (t_cap == 0 || out),
                "frontend stream: bad output shape");
  ASR_CHECK_ARG((ended_total == nullptr) == (host_ended_total == nullptr),
                "frontend stream: ended_total on the device and on the host go together");
  ASR_CHECK_ARG(host_state[3] == n_streams,
                "frontend stream: the state was reset for %lld streams, not %d", host_state[3],
                n_streams);
  const int L = cfg->frame_len, S = cfg->frame_step;
  const long long s_before = host_state[0];
  ASR_CHECK_ARG(s_before + n_samples < (1ll << 30), "frontend stream: more than 2^30 samples");
  const int s0 = (int)s_before, s1 = s0 + n_samples;
  const FeStreamLayout l = fe_stream_layout(cfg, n_streams);
  // ---- the plan of the call: integers only, and nothing is changed before it is whole
  bool live = false;
  int max_new = 0, longest = 0, c0_new = -1;
  for (int i = 0; i < n_streams; ++i) {
    const long long known = host_state[kHostHead + 2 * i];
    const int c0 = (int)host_state[kHostHead + 2 * i + 1];
    const int e = host_ended_total ? host_ended_total[i] : -1;
    int c1;
    if (known >= 0) {
      ASR_CHECK_ARG(e == known, "frontend stream: stream %d ended at %lld samples, now %d is "
                    "given", i, known, e);
      c1 = c0;
    } else if (e >= 0) {
      ASR_CHECK_ARG(e >= 2 && e >= s0 && e <= s1,
                    "frontend stream: stream %d: the length %d is given with the call whose "
                    "samples reach it (%d .. %d) and is at least 2", i, e, s0, s1);
      c1 = fe_padded_frames(e, L, S);
    } else {
      live = true;
      c1 = fe_complete_frames(s1, L, S);
    }
    if (c1 > c0) {
      ASR_CHECK_ARG(c0_new < 0 || c0_new == c0, "frontend stream: the streams are out of step");
      c0_new = c0;
    }
    max_new = c1 - c0 > max_new ? c1 - c0 : max_new;
    longest = c1 > longest ? c1 : longest;
  }
  const int lo = (int)host_state[1];
  int hi = live ? fe_complete_frames(s1, L, S) - l.la : longest;
  hi = hi < lo ? lo : hi;
  const int stride = cfg->stride < 1 ? 1 : cfg->stride;
  const int t0 = (lo + stride - 1) / stride, t1 = (hi + stride - 1) / stride;
  ASR_CHECK_ARG(t1 - t0 <= t_cap, "frontend stream: the call emits %d rows, out has %d",
                t1 - t0, t_cap);
  const FeStreamWs w = fe_stream_ws(cfg, n_streams, n_samples);
  ASR_CHECK_ARG(max_new <= w.cap, "frontend stream: %d new frames of one stream", max_new);
  if (ws_bytes < w.total) {
    asr_set_error("frontend stream: workspace %zu < %zu bytes", ws_bytes, w.total);
    return ASR_ERR_WORKSPACE;
  }
  // ---- launches
  char* sb = reinterpret_cast<char*>(state);
  char* wb = reinterpret_cast<char*>(workspace);
  int* counters = reinterpret_cast<int*>(sb + l.counters);
  float* carry = reinterpret_cast<float*>(sb + l.carry);
  double* ring = reinterpret_cast<double*>(sb + l.ring);
  double* stats = reinterpret_cast<double*>(sb + l.stats);
  float* sig = reinterpret_cast<float*>(wb + w.sig);
  int* plan = reinterpret_cast<int*>(wb + w.ints);
  int* offsets = plan + 4 * n_streams;
  int* lengths = offsets + n_streams;
  int* nframes = lengths + n_streams;
  double* fresh = reinterpret_cast<double*>(wb + w.fresh);
  const int fcap = max_new > 0 ? max_new : 1;       // row count of `fresh` per stream
  if (n_samples > 0 || max_new > 0 || t1 > t0) {
    hipLaunchKernelGGL(fe_stream_gather_kernel, dim3((w.sig_ld + 255) / 256, n_streams),
                       dim3(256), 0, stream, *cfg, counters, carry, audio, n_samples,
                       ended_total, s0, s1, max_new, sig, w.sig_ld, plan, offsets, lengths,
                       nframes);
    ASR_CHECK_LAUNCH();
  }
  if (max_new > 0) {
    hipLaunchKernelGGL(fe_frames_kernel,
                       dim3((max_new + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK, n_streams),
                       dim3(256), 0, stream, *cfg, sig, offsets, lengths, window, mel, mel_range,
                       dct, fresh, fcap, l.fb, reinterpret_cast<const double2*>(sb + l.tw),
                       reinterpret_cast<const double*>(sb + l.melt), c0_new > 0 ? 1 : 0,
                       nframes);
    ASR_CHECK_LAUNCH();
  }
  if (t1 > t0) {
    hipLaunchKernelGGL(fe_stream_finalize_kernel, dim3((l.f_out + 63) / 64, n_streams), dim3(64),
                       0, stream, *cfg, ended_total, plan, ring, fresh, fcap, l.fb, l.R, l.la,
                       stats, out, n_pad, l.f_out, lo, hi, s1);
    ASR_CHECK_LAUNCH();
    if (n_pad > n_streams) {
      hipLaunchKernelGGL(fe_zero_pad_rows_kernel, dim3(256), dim3(256), 0, stream, out, t1 - t0,
                         n_streams, n_pad, l.f_out);
      ASR_CHECK_LAUNCH();
    }
  }
  if (n_samples > 0 || max_new > 0 || t1 > t0) {
    hipLaunchKernelGGL(fe_stream_commit_kernel, dim3(2, n_streams), dim3(256), 0, stream, *cfg,
                       ended_total, plan, sig, w.sig_ld, fresh, fcap, l.fb, l.R, l.la, counters,
                       carry, ring, s1, hi);
    ASR_CHECK_LAUNCH();
  }
  // ---- the host's counts
  host_state[0] = s1;
  host_state[1] = hi;
  host_state[2] = t1;
  for (int i = 0; i < n_streams; ++i) {
    const int e = host_ended_total ? host_ended_total[i] : -1;
    if (host_state[kHostHead + 2 * i] >= 0) continue;
    if (e >= 0) {
      host_state[kHostHead + 2 * i] = e;
      host_state[kHostHead + 2 * i + 1] = fe_padded_frames(e, L, S);
    } else {
      host_state[kHostHead + 2 * i + 1] = fe_complete_frames(s1, L, S);
    }
  }
  *frames_lo = t0;
  *frames_hi = t1;
  return ASR_OK;
}
