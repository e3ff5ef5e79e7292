/* asr_hip.h -- C ABI of libasr_hip.so: the MI355X (gfx950) kernels behind the
 * asr-study acoustic-training hot path (MFCC/log-mel -> BiLSTM stack -> CTC).
 *
 * The reference (igormq/asr-study) has NO native/FFI boundary: every op on this
 * path is a Keras-1.2.2 / TensorFlow-1.3.0 / NumPy call made from Python.  Each
 * entry point below therefore cites the reference call site whose arithmetic it
 * replaces (paths relative to the reference checkout); INTEGRATION.md shows the
 * ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C types only; device pointers are raw addresses (from
 *    torch.Tensor.data_ptr() on the Python side); no torch types anywhere.
 *  - the CALLER owns all memory.  Scratch space is sized by the matching
 *    *_workspace_bytes() query and passed in; the library never allocates
 *    persistent device memory.
 *  - all work is enqueued on the given hipStream_t (passed as void*); no entry
 *    point synchronises the device unless its comment says so.
 *  - every function returns 0 on success or a negative asr_status; the message
 *    is available from asr_last_error() (thread-local).
 *  - activations are TIME-MAJOR slabs (T, Npad, feat) float32, Npad = batch
 *    rounded up to a multiple of 16 (rows n >= N are padding and carry zeros).
 *  - fused gate layout: every (.., 4H) gate axis is ordered unit-major,
 *    gate-minor: column = unit*4 + gate, gate in {0:i, 1:f, 2:c, 3:o}
 *    (Keras' consume_less='gpu' layout is gate-major: column = gate*H + unit;
 *    core/layers.py:447-450.  The Python host converts at the checkpoint edge.)
 */
#ifndef ASR_HIP_H
#define ASR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* asr_stream_t; /* hipStream_t */

enum asr_status {
  ASR_OK = 0,
  ASR_ERR_INVALID = -1,   /* bad argument / unsupported shape            */
  ASR_ERR_WORKSPACE = -2, /* workspace too small                         */
  ASR_ERR_LAUNCH = -3,    /* HIP launch or runtime error                 */
  ASR_ERR_TIMEOUT = -4,   /* persistent kernel gave up on a bounded spin */
  ASR_ERR_RESIDENCY = -5  /* persistent grid would not be co-resident    */
};

const char* asr_last_error(void);
/* ABI version of THIS header: bumped whenever an argument struct grows or changes meaning (no
 * struct carries a size field).  A caller checks asr_version() == ASR_HIP_ABI_VERSION right
 * after loading the library (asr_study_amd/_lib.py does) and refuses a mismatch.
 * 100: rounds 1-4.  105: asr_lstm_args +compact +activation +fwd_units, asr_pack_args +mask2
 * +r2_hl, asr_lstm_ln_args +activation.  106: asr_lstm_args +dz_hl +dz_bound +dz_scale_out.
 * 107: asr_rnn_args and the asr_rnn_* / asr_activation_* entry points (K14); the asr_bn_*
 * entry points (K15: plain scalar arguments, no struct, so the version stays); asr_gru_args
 * and the asr_gru_* entry points (K16: additions only, no existing layout changes); asr_rhn_args
 * and the asr_rhn_* entry points (K17: additions only as well); the asr_seqbn_* entry points
 * (K18: plain scalar arguments again); the asr_dwconv1d_* / asr_glu_* / asr_swish_* entry points
 * (K22: plain scalar arguments, additions only); asr_specaug_apply (K23: likewise);
 * asr_relattn_args and asr_relattn_* (K24), asr_attn_window and the asr_attn_win_* /
 * asr_relattn_win_* / asr_dwconv1d_pad_* entry points (K25): additions only as well;
 * asr_attn_stream_args, asr_ring_put, asr_attn_stream_*, asr_relattn_stream_fwd,
 * asr_dwconv1d_stream_fwd and asr_ctc_greedy_stream (K26): additions only again;
 * asr_ctc_beam_stream, asr_ctc_beam_lm_stream and their two size functions (K27): likewise;
 * asr_gru_uni_args and the asr_gru_uni_* entry points (K28): additions only;
 * asr_lstm_uni_args and the asr_lstm_uni_* entry points (K29): additions only;
 * asr_frontend_cfg.norm_mode (the former `reserved`, same layout) and the
 * asr_frontend_stream* entry points (K30): additions only -- but the field is
 * now READ: a caller that left `reserved` uninitialised must set it to 0,
 * any value other than 0 or 1 is ASR_ERR_INVALID;
 * asr_rnnt_workspace_bytes, asr_rnnt_loss_grad, asr_rnnt_greedy_step, asr_onehot_rows and
 * asr_rows_select (K31: plain scalar arguments, additions only);
 * asr_attn_cross_args, asr_attn_cross_* and the asr_aed_* entry points (K32: a new struct and
 * plain scalar arguments, additions only);
 * asr_time_stack_fwd / _bwd (K33: plain scalar arguments, additions only). */
#define ASR_HIP_ABI_VERSION 107
int asr_version(void);
/* Device facts the host needs for sizing persistent grids (CU count etc). */
int asr_device_info(int* num_cus, int* lds_bytes_per_cu, char* arch, int arch_len);

/* ------------------------------------------------------------------------ */
/* K1-K3  Front-end.  Replaces preprocessing/audio.py:223-253 (FBank._call:  */
/* preemphasis, framing, Hamming, |rFFT|^2/nfft, energy, mel filterbank),    */
/* :339-367 (MFCC._call: log, DCT-II ortho, lifter, c0<-log energy, deltas), */
/* :404-442 (LogFbank._call), :77-150 (_postprocessing: stride / context)    */
/* and :70-75 (_standarize) together with preprocessing/audio_utils.py       */
/* :17-50,:98-120,:143-173.                                                  */
/* ------------------------------------------------------------------------ */
typedef struct asr_frontend_cfg {
  int kind;          /* 0 = MFCC, 1 = LogFbank                               */
  int frame_len;     /* round_half_up(win_len*fs)   (400)                    */
  int frame_step;    /* round_half_up(win_step*fs)  (160)                    */
  int nfft;          /* 512 (must be 512 in this build)                      */
  int num_filt;      /* 40 / 80 (<= 128)                                     */
  int num_cep;       /* 13 (MFCC only, <= 64)                                */
  int append_energy; /* MFCC: c0 <- log(energy+eps); LogFbank: extra column  */
  int d, dd;         /* append deltas / delta-deltas                         */
  int stride;        /* keep every stride-th frame                           */
  int num_context;   /* +-context frame stacking (zero rows off the edges)   */
  int mean_norm, var_norm;
  int norm_mode;     /* 0 = whole-utterance statistics, 1 = running (causal):  */
                     /* Welford's recursion over the kept frames, see below    */
  double pre_emph;   /* 0.97 -- float64: the per-frame chain runs in float64 */
  double eps;        /* 1e-8                                                 */
} asr_frontend_cfg;

/* Number of frames for a signal of `samples` samples (audio_utils.py:29-32). */
int asr_frontend_num_frames(int samples, int frame_len, int frame_step);
/* Feature columns produced per frame BEFORE context stacking ((1+d+dd)*base). */
int asr_frontend_num_feats(const asr_frontend_cfg* cfg);
size_t asr_frontend_workspace_bytes(const asr_frontend_cfg* cfg, int n_utt,
                                    int max_frames);
/* audio: concatenated float32 samples; offsets[i]/lengths[i] (device int32)
 * delimit utterance i.  window (frame_len), mel (num_filt x (nfft/2+1), dense
 * row-major, from audio.py:255-277 computed on the host in float64), mel_range
 * (num_filt x {first, last+1} non-zero bin of each filter, device int32), dct
 * (num_filt x num_cep: scipy DCT-II 'ortho' with the lifter folded in; MFCC
 * only) are FLOAT64 device tables (the reference computes in float64; see
 * csrc/frontend.hip).  out is the float32 (T_out, n_pad, F_out) time-major
 * slab (row stride n_pad*F_out), zero-filled past each utterance's frames
 * (pad_sequences(padding='post'), datasets/dataset_generator.py:227);
 * out_frames[i] (device int32) receives the frame count after striding.
 * host_lengths mirrors `lengths` on the host (grid sizing; no device sync). */
int asr_frontend_features(const asr_frontend_cfg* cfg, const float* audio,
                          const int* offsets, const int* lengths,
                          const int* host_lengths, int n_utt, int n_pad,
                          const double* window, const double* mel,
                          const int* mel_range, const double* dct, float* out,
                          int t_out,
                          int* out_frames, void* workspace, size_t ws_bytes,
                          asr_stream_t stream);

/* K30  Running normalisation and the resumed front-end.
 *
 * cfg->norm_mode = 1 (num_context must be 0): per utterance and output column,
 * over the rows kept after feats[::stride], kept frame t = 0, 1, ... with value
 * x_t (float64):  n = t + 1;  d = x_t - mean;  mean += d / n;
 * M2 += d * (x_t - mean);  sd = sqrt(M2 / n);
 * out_t = (x_t - (mean_norm ? mean : 0)) / (var_norm ? sd + eps : 1).
 * asr_frontend_features takes it as it takes norm_mode = 0.
 *
 * asr_frontend_stream is the same computation resumed across calls that each
 * bring n_samples new samples of every one of n_streams streams (lock-step):
 * the rows it emits, concatenated, are bit for bit the rows of
 * asr_frontend_features with norm_mode = 1 on the whole signals.  norm_mode = 0
 * is refused (ASR_ERR_INVALID): whole-utterance statistics need the end of the
 * utterance.  frame_step <= frame_len.
 *   state       device memory of asr_frontend_stream_state_bytes: per stream the
 *               sample in front of the carry, the carried samples that do not
 *               complete a frame yet (< frame_len), the counts of samples seen,
 *               frames computed and rows emitted, the ring of the last
 *               2 la + 1 base-feature rows (la = 2 d + 2 dd, what the deltas
 *               look ahead), mean and M2 of every output column; and the FFT
 *               twiddles and the transposed mel table, built by the reset.
 *   host_state  asr_frontend_stream_host_ints(n_streams) int64 of the caller's:
 *               the same counts on the host.  Which frames a call emits is
 *               integer arithmetic on them; no call reads the device.
 *   audio       (n_streams, n_samples) float32, device.  n_samples may be 0.
 *   ended_total / host_ended_total   device and host int32 per stream (both or
 *               neither): -1, or the stream's total length in samples from the
 *               call on whose samples reach it (samples_fed <= total <=
 *               samples_fed + n_samples at that call; >= 2), in every later
 *               call too.  Samples past it are ignored.
 * After S samples a stream that has not ended has F(S) = 0 if S < frame_len else
 * 1 + (S - frame_len) / frame_step complete frames, and its frame f is final once
 * f + la < F(S); all asr_frontend_num_frames(total) frames of an ended stream are
 * final (tail zero-padded, deltas edge-replicated, as the batch call).  A call
 * emits, for every stream, the kept frames of the window [lo, hi) that became
 * final for the streams still running (hi = the largest frame count once all
 * have ended): out[(t, stream, col)], t < *frames_hi - *frames_lo <= t_cap, the
 * kept rows *frames_lo .. *frames_hi - 1 of every stream (host ints; zero rows
 * past a stream's end; batch-padding rows zero).  Launches: gather, frames,
 * finalize, commit (+ the padding rows); a call that completes no frame and
 * emits none runs gather and commit only. */
size_t asr_frontend_stream_state_bytes(const asr_frontend_cfg* cfg, int n_streams);
int asr_frontend_stream_host_ints(int n_streams);
size_t asr_frontend_stream_workspace_bytes(const asr_frontend_cfg* cfg, int n_streams,
                                           int n_samples);
/* Zero-fills the state, builds its tables (mel, mel_range as above). */
int asr_frontend_stream_reset(const asr_frontend_cfg* cfg, void* state,
                              long long* host_state, int n_streams,
                              const double* mel, const int* mel_range,
                              asr_stream_t stream);
int asr_frontend_stream(const asr_frontend_cfg* cfg, void* state, long long* host_state,
                        const float* audio, int n_samples, const int* ended_total,
                        const int* host_ended_total, int n_streams, int n_pad,
                        const double* window, const double* mel, const int* mel_range,
                        const double* dct, float* out, int t_cap, int* frames_lo,
                        int* frames_hi, void* workspace, size_t ws_bytes,
                        asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K4/K6  fp32 MFMA GEMM.  Replaces K.dot(x*B_W, W) (core/layers.py:439,     */
/* hoisted out of the time loop), TimeDistributed(Dense) (core/models.py     */
/* :278-279) and their tf.gradients.                                         */
/*   C[M,N] = c_scale (.) (alpha * (opA(A) (.) a_scale) @ opB(B) + bias[N])  */
/*            + beta * C.    trans_a: A is stored (K,M) row-major; trans_b: B */
/*   is stored (N,K) row-major.  a_scale / c_scale: optional (period, M or K */
/*   / N) variational-dropout masks indexed by (row % period); pass NULL.    */
/* split_k > 1 needs workspace of split_k*M*N floats (deterministic reduce). */
/* ------------------------------------------------------------------------ */
typedef struct asr_gemm_args {
  int M, N, K;
  int trans_a, trans_b;
  const float* A; int lda;
  const float* B; int ldb;
  float* C; int ldc;
  float alpha, beta;
  const float* bias;       /* (N) added to every row, or NULL                */
  const float* a_scale;    /* (period x Kdim-or-Mdim) mask on A rows or NULL */
  int a_scale_period;      /* row index modulo this selects the mask row     */
  int a_scale_ld;
  const float* c_scale;    /* (period x N) mask on C rows, or NULL           */
  int c_scale_period;
  int c_scale_ld;
  int split_k;             /* 0/1 = none                                     */
  /* arithmetic: 0 = exact fp32 MFMA; 1 = split-fp16 MFMA (hi + lo/2048, 22-bit   */
  /* mantissa, fp32 accumulate); -1 = library default (env ASR_GEMM_PREC, 1).    */
  int precision;
  /* split-fp16 only: device floats holding max|A| / max|B| (asr_absmax) used to */
  /* pick a power-of-two pre-scale so tiny gradients stay in fp16 range; NULL=1. */
  const float* a_absmax;
  const float* b_absmax;
} asr_gemm_args;
size_t asr_gemm_workspace_bytes(const asr_gemm_args* a);
int asr_gemm(const asr_gemm_args* a, void* workspace, size_t ws_bytes,
             asr_stream_t stream);
/* ------------------------------------------------------------------------ */
/* K4/K6 with operands converted ONCE: packed split-fp16 planes.  asr_pack_hl  */
/* turns an fp32 matrix (rows, cols) -- optionally times a variational-dropout */
/* mask[(row % period), col] (core/models.py:265-266), applied in fp32 before   */
/* the split -- into two fp16 planes hi = fp16(x*s), lo = fp16(x*s - hi) with   */
/* s = the power of two that maps *absmax into [2^8, 2^9) (1 if absmax is       */
/* NULL), in either or both orientations:                                       */
/*   r planes (rows, ldk_r): the reduction index of the later GEMM = columns,   */
/*   c planes (cols, ldk_c): the reduction index = rows (weight gradients);     */
/* ldk_* = the extent rounded up to a multiple of 32 halfs, zero padded.  The   */
/* scale is written to *scale_out (device float).  asr_gemm_hl then computes    */
/*   C[M,N] = alpha/(sa*sb) * (Ah Bh^T + Ah Bl^T + Al Bh^T) (+bias) (*c_scale)  */
/*            + beta*C                                                          */
/* from A planes (M, lda) and B planes (N, ldb), reduction index contiguous in  */
/* both, fp32 accumulation (2^-22 relative per product: the arithmetic of       */
/* asr_gemm precision 1 without its per-tile conversions).  A sub-matrix is a   */
/* pointer offset (64-byte aligned: a whole (hi, lo) group) with the same       */
/* leading dimension; K % 8 == 0; lda % 16 == 0 and ldb % 16 == 0.              */
/* ------------------------------------------------------------------------ */
typedef struct asr_pack_args {
  const float* src; int rows, cols, ld;
  const float* mask; int mask_period, mask_ld;   /* or NULL; row period (any n_pad)   */
  const float* absmax;                           /* device float, or NULL (scale 1)   */
  float* scale_out;                              /* device float, or NULL             */
  void* r_hl; int ldk_r;                         /* (rows, 2 ldk_r) halfs, or NULL    */
  void* c_hl; int ldk_c;                         /* (cols, 2 ldk_c) halfs, or NULL    */
  /* optional: a SECOND set of row planes r2_hl (geometry of r_hl) of the same source under   */
  /* mask2 (period / ld of mask) -- the two directions' dropout masks of a BiLSTM input, the  */
  /* source read once; both sets share the scale.  NULL = one set.                            */
  const float* mask2; void* r2_hl;
} asr_pack_args;
int asr_pack_hl(const asr_pack_args* a, asr_stream_t stream);
/* Debug: arm (enable != 0) / read the K-loop phase profile of asr_gemm_hl's workgroup 0:      */
/* out64 = 8 waves x 8 phases of shader clocks (fragment reads, barrier, MFMAs first half,    */
/* MFMAs second half, barrier, prologue, the K loop in 100 MHz real-time ticks, unused);      */
/* NULL to only arm / disarm.                                                                 */
int asr_gemm_hl_profile(int enable, long long* out64, asr_stream_t stream);
typedef struct asr_gemm_hl_args {
  int M, N, K;
  const void* a_hl; int lda;                     /* interleaved planes; reduction     */
  const void* b_hl; int ldb;                     /* indices per row (a row = 2 ld halfs) */
  const float* a_scale; const float* b_scale;    /* device floats (asr_pack_hl) or NULL */
  float* C; int ldc;
  float alpha, beta;
  const float* bias;                             /* (N) or NULL                       */
  const float* c_scale; int c_scale_period; int c_scale_ld;   /* mask on C rows or NULL */
  int split_k;                                   /* 0/1 = none                        */
  int tile;                                      /* 0 = library default (256 x 256 for  */
                                                 /* outputs that large), 128 = the      */
                                                 /* 128 x 128 kernel: 4 waves, 80 KB    */
                                                 /* LDS, co-resident with a recurrent   */
                                                 /* workgroup that reserves no LDS      */
  int k_major;                                   /* != 0: C = A^T B from planes whose   */
                                                 /* ROWS are the reduction index: a_hl   */
                                                 /* (K rows, lda >= M columns), b_hl (K  */
                                                 /* rows, ldb >= N columns) -- x^T dz,   */
                                                 /* h^T dz on the planes x@W / dz@W^T    */
                                                 /* use (no second orientation packed);  */
                                                 /* a sub-matrix = pointer to (first row,*/
                                                 /* first column group of 16)            */
  /* Segmented reduction range of A (row-major form only; 0 = none): K = n * a_seg_k, n <= 16,  */
  /* a_seg_k % 32 == 0; reduction indices [i a_seg_k, (i+1) a_seg_k) are read from columns      */
  /* [0, a_seg_k) of the planes a_seg_row[i] (>= 0) rows further down: C = sum_i A_i B_i^T with */
  /* A_i = a_hl shifted by a_seg_row[i] rows -- the implicit im2col over time of asr_conv2d_*   */
  /* (tap i of a filter reads the activation slab i frames on).  lda >= a_seg_k.                 */
  int a_seg_k;
  long long a_seg_row[16];
  /* Batch (k_major form only; 0 / 1 = none): `batch` <= 16 GEMMs that share B in one launch,  */
  /* C_b = A_b^T B with A_b = a_hl shifted by a_batch_row[b] (>= 0) plane rows and C_b = C +   */
  /* b * M * ldc (the members' outputs are consecutive row blocks); no beta / bias / mask.     */
  /* The per-tap weight gradients of asr_conv2d_wgrad.  split_k applies to every member; the   */
  /* workspace is split_k * batch * M * N floats.                                              */
  int batch;
  long long a_batch_row[16];
  /* > 0 (segmented form only; beta = 0, no mask): C = min(max(alpha A B^T + bias, 0), clamp_hi) */
  /* -- the clipped ReLU of asr_conv2d_fwd applied where the tile is still in registers.         */
  float clamp_hi;
} asr_gemm_hl_args;
size_t asr_gemm_hl_workspace_bytes(const asr_gemm_hl_args* a);
int asr_gemm_hl(const asr_gemm_hl_args* a, void* workspace, size_t ws_bytes,
                asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K13  2-D convolution front-end of BASELINE.json configs[2] ("DeepSpeech2-   */
/* style 5xBiLSTM(512) + 2 conv front-end").  NO REFERENCE COUNTERPART: the    */
/* reference lists Deep Speech 2 as TODO (README.md:118) and its deep_speech   */
/* factory (core/models.py:148-214) is dead code without convolutions; the op  */
/* is defined here as Keras-1.2.2 Convolution2D(nb_filter, nb_row, nb_col,     */
/* subsample=(st, sf), border_mode='same', dim_ordering='tf') on the           */
/* (N, T, F, C) view of the feature slab, followed by a clipped ReLU           */
/* min(max(z, 0), clip) (the reference's clipped_relu, core/models.py:116).    */
/* 'same' = TensorFlow's rule: out = ceil(in / stride), pad_total =            */
/* max((out - 1) stride + k - in, 0), pad_before = pad_total / 2.              */
/*                                                                              */
/* Layout: activations are time-major slabs (T, n_pad, F*C), channel minor     */
/* (feature index f*C + c) -- Reshape((T, F*C)) of the Keras tensor is the     */
/* identity; W is (kt, kf, C_in, C_out) row-major (Keras 'tf' kernel), bias    */
/* (C_out).  The convolution over FREQUENCY is folded into a banded matrix     */
/* per time tap (band[dt][(fi,ci)][(fo,co)] = W[dt][fi - sf fo + pf][ci][co]), */
/* the convolution over TIME is the segmented reduction of asr_gemm_hl: tap dt */
/* reads the packed activation planes dt frames further on (implicit im2col);  */
/* the products run on the packed split-fp16 MFMA kernel of K4.  kt <= 16.     */
/*   fwd  : z = conv(x, W) + b   (kept for the backward pass),  y = act(z)     */
/*   dgrad: dx = conv^T(dy (.) act'(z), W)                                      */
/*   wgrad: dW = x (*) (dy (.) act'(z)),  db = sum over rows and fo            */
/* The workspace keeps the packed planes of x (written by fwd) and of           */
/* dz = dy (.) act'(z) (written by whichever of dgrad / wgrad runs first);     */
/* reuse_x / reuse_dz = 1 tell a later call on the SAME workspace to skip the  */
/* pack (the host runs fwd ... dgrad, wgrad per layer with its own workspace). */
/* ------------------------------------------------------------------------ */
typedef struct asr_conv2d_args {
  int T_in, n_pad, F_in, C_in;   /* input slab (T_in, n_pad, F_in*C_in)              */
  int C_out, kt, kf, st, sf;     /* filter and strides (time, frequency)            */
  float clip;                    /* clipped-ReLU ceiling (20); <= 0: linear output  */
  const float* x;                /* fwd, wgrad                                      */
  const float* W;                /* (kt, kf, C_in, C_out)                           */
  const float* bias;             /* (C_out)                                         */
  float* z;                      /* (T_out, n_pad, F_out*C_out): fwd out, bwd in.   */
                                 /* fwd with clip > 0: NULL (or == y) fuses the     */
                                 /* clipped ReLU into the GEMM epilogue -- only y   */
                                 /* is written; bwd then takes y here (the mask     */
                                 /* 0 < z < clip reads the same from y)             */
  float* y;                      /* fwd out (may be NULL when clip <= 0: y = z)     */
  const float* dy;               /* dgrad / wgrad in, shape of z                    */
  float* dx;                     /* dgrad out, shape of x                           */
  float* dW;                     /* wgrad out, shape of W                           */
  float* db;                     /* wgrad out (C_out)                               */
  int reuse_x, reuse_dz;
  const float* x_absmax;         /* device float >= max|x| (the previous layer's    */
                                 /* clip), or NULL: measured with asr_absmax        */
} asr_conv2d_args;
/* Streams: the block GEMMs of one forward / dgrad call may be issued on two streams of the   */
/* library's own beside `stream` (forked behind everything enqueued on it, joined before the   */
/* call returns): to the caller the call is ordered on `stream` like any other.              */
/* T_out = ceil(T_in / st), F_out = ceil(F_in / sf). */
int asr_conv2d_out_shape(const asr_conv2d_args* a, int* T_out, int* F_out);
size_t asr_conv2d_workspace_bytes(const asr_conv2d_args* a);
int asr_conv2d_fwd(const asr_conv2d_args* a, void* workspace, size_t ws_bytes,
                   asr_stream_t stream);
int asr_conv2d_dgrad(const asr_conv2d_args* a, void* workspace, size_t ws_bytes,
                     asr_stream_t stream);
int asr_conv2d_wgrad(const asr_conv2d_args* a, void* workspace, size_t ws_bytes,
                     asr_stream_t stream);

/* out[0] = max |x[i]| over a 16-byte aligned flat tensor (HBM-bound).         */
int asr_absmax(const float* x, int64_t n, float* out, asr_stream_t stream);
/* out[n] = beta*out[n] + sum_m X[m, n]  (bias gradients; X read once,       */
/* float64 accumulation, fixed-order two-stage reduce).                      */
size_t asr_colsum_workspace_bytes(int M, int N);
int asr_colsum(const float* X, int M, int N, int ldx, float* out, float beta,
               void* workspace, size_t ws_bytes, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K5  Recurrent LSTM sequence kernels (both directions of one Bidirectional */
/* layer per call).  Replace core/layers.py:432-469 (LSTM.step) iterated by  */
/* Keras K.rnn, and its BPTT.  Gate math: i,f,o = hard_sigmoid = clip(.2x+.5, */
/* 0,1); c = f*c + i*tanh(z_c); h = o*tanh(c); h0 = c0 = 0; the reverse      */
/* direction walks the PADDED slab from T-1 down to 0 (no Masking).          */
/* ------------------------------------------------------------------------ */
typedef struct asr_lstm_args {
  int T, n_pad, H;     /* n_pad % 16 == 0, H % 4 == 0                        */
  int mode;            /* 0 = persistent (default), 1 = one launch per step  */
  const float* U;      /* (2, H, 4H)  [dir][k][unit*4+gate]                  */
  const float* mask_u; /* (2, n_pad, H) variational mask B_U or NULL         */
  /* forward: zx (T, n_pad, 2, 4H) = x@W+b precomputed; outputs y (T, n_pad, */
  /* 2H) = [h_fwd | h_bwd], cell (T, n_pad, 2, H), gates (T, n_pad, 2, 4H)   */
  /* post-activation (kept for BPTT).                                        */
  const float* zx;
  float* y;
  float* cell;
  float* gates;
  /* backward: dy (T, n_pad, 2H) in; dz (T, n_pad, 2, 4H) out.               */
  const float* dy;
  float* dz;
  /* backward, optional: receives max |dz| (one device float; used as the     */
  /* split-fp16 GEMM pre-scale of the gradient operand), or NULL.             */
  float* dz_absmax;
  /* Optional step range: process recurrence steps [step_begin, step_begin +  */
  /* step_count) only (step s is frame s of the forward direction and frame   */
  /* T-1-s of the backward one; BPTT walks them in the opposite order).  A    */
  /* sequence is processed by calls with consecutive ranges starting at 0 on  */
  /* the SAME workspace and stream order; step_count = 0 means all T steps.   */
  /* Lets the caller overlap the GEMMs that feed / consume the outer frames   */
  /* with the recurrence over the inner ones.                                 */
  int step_begin, step_count;
  /* Optional cell variants of the reference's LSTM override (core/layers.py:432-469);  */
  /* all NULL = the plain cell.  Frames are indexed by t (slab row), not by step.       */
  /* mi: multiplicative integration z = alpha*Wx*Uh + beta1*Uh + beta2*Wx + b           */
  /*     (:441-443): (2, 4, 4H) = per direction alpha, beta1, beta2, b (unit-major,     */
  /*     gate-minor); zx must then be x@W WITHOUT the bias.  uh (T, n_pad, 2, 4H)       */
  /*     receives h_prev@U in the forward call and is read back by the backward call,   */
  /*     which also needs wx (= the forward zx) and writes dwx (T, n_pad, 2, 4H) =      */
  /*     d/d(x@W) -- dz then holds d/d(h_prev@U) -- and dmi (n_pad/16, 2, 4, 4H), the   */
  /*     per-batch-tile sums of d alpha, d beta1, d beta2, d b (sum over axis 0).       */
  /* zone_c / zone_h: zoneout (:457-467), new = prev + k*(candidate - prev) with the    */
  /*     coefficient k (T, 2, H): the per-frame keep mask in training, 1 - level at     */
  /*     test time.                                                                     */
  const float* mi;
  float* uh;
  const float* zone_c;
  const float* zone_h;
  const float* wx;
  float* dwx;
  float* dmi;
  /* backward, optional: db_part (n_pad/16, 2, 4H) receives, per batch tile, the sum of dz    */
  /* over the tile's samples and over all steps (+= across the slices of a sequence): the     */
  /* bias gradient is its sum over axis 0, so no pass over the dz slab is needed for it.      */
  /* With mi set the same sums are dmi[:, :, 3].                                              */
  float* db_part;
  /* forward, optional: number of real rows of the batch (0 = all n_pad).  n_valid == 1    */
  /* (predict.py decodes one utterance per call) selects a tile-free exact-fp32 kernel     */
  /* that reads and writes ROW 0 of the slabs only; the padding rows are left untouched.   */
  int n_valid;
  /* LDS a recurrent workgroup reserves, in KB (0 = 96: alone on its CU beside 80 KB GEMM    */
  /* workgroups).  80 = two recurrent workgroups per CU, for launches on a stream confined   */
  /* to half of the CUs (asr_stream_create_cu_mask): the recurrence is latency-bound, so two */
  /* chains interleave on one CU while the other half of the chip runs GEMMs.                */
  int lds_reserve_kb;
  /* backward, optional: 1 = the COMPACT launch geometry of the plain cell at H = 256 / 512   */
  /* in persistent mode: a chain is H/32 workgroups instead of H/16 (each owns twice the      */
  /* outputs), so a layer occupies half as many CUs (128 of 256 at H = 512, 64 utterances) at */
  /* a longer step; the caller runs the weight-gradient GEMMs of the layer above on the CUs   */
  /* left free.  Gate gradients are bit-identical to the default geometry.  Ignored where the */
  /* compact kernel does not exist (other H, cell variants, stepwise mode, forward).          */
  int compact;
  /* The reference LSTM's `activation` hyper-parameter (core/layers.py:452, :463: cell         */
  /* candidate g = act(z_c), output h = o * act(c); brsmv1 passes it on, core/models.py:220):  */
  /* 0 tanh (default), 1 relu, 2 sigmoid, 3 hard_sigmoid, 4 linear, 5 softsign, 6 softplus     */
  /* (Keras-1.2.2 names).  Anything but 0 runs on the variant kernels (as mi / zoneout do).    */
  int activation;
  /* forward, optional: units per workgroup of the wide kernels -- 0 = the library decides     */
  /* (eight at H = 256 where the layer then leaves half of the CUs free), 8 / 16 = force.      */
  /* Slices of one sequence may differ (same exchange layout): the host runs the slice that    */
  /* has GEMMs beside it on the geometry that occupies fewer CUs.  Results do not depend on it. */
  int fwd_units;
  /* backward, optional: dz_hl != NULL makes BPTT write the gate gradients as the PACKED PLANES  */
  /* of asr_pack_hl ((T n_pad) rows x 8H reduction indices: row = frame * n_pad + sample, the    */
  /* r-plane layout, ld = 8H) INSTEAD of the fp32 slab dz (which may then be NULL): a thread's   */
  /* 16 gate gradients are exactly one (16 hi, 16 lo) group at the byte offset of its fp32       */
  /* values, so the kernel stores the same 64 bytes either way and the separate pack pass over   */
  /* dz (2.1 GB per layer at H = 512, 64 utterances) disappears.  The planes' power-of-two       */
  /* scale must be known BEFORE the pass: it is asr_pack_hl's scale of *dz_bound (a device       */
  /* float >= the max |dz| this call will produce, e.g. 64 x the previous training step's        */
  /* maximum -- asr_lstm_dz_guard maintains it), written to *dz_scale_out for asr_gemm_hl.  The  */
  /* kernel then also splits dz with THAT scale for its own dz @ U^T products (instead of a      */
  /* per-sample scale): same 2^-22 product accuracy while max |dz| stays within                  */
  /* [2^-11, 2^7] x bound.  Exists on the two-dimensional-split kernels only                    */
  /* (asr_lstm_dz_hl_supported); dz_absmax and db_part work as before.                          */
  void* dz_hl;
  const float* dz_bound;
  float* dz_scale_out;
} asr_lstm_args;
/* 1 if asr_lstm_seq_bwd would honour a->dz_hl for this geometry / mode / arithmetic, else 0.   */
int asr_lstm_dz_hl_supported(const asr_lstm_args* a);
/* Keeps a layer's *dz_bound in step with the measured *dz_absmax of the pass just enqueued     */
/* (device-side, no synchronisation): with M = max * scale(bound), the bound is kept while M    */
/* stays in [2^-1, 2^6) (so that identical inputs see identical scales); otherwise it becomes    */
/* 64 * max when the maximum shrank and sqrt(bound * 64 * max) when it grew (a spike is usually  */
/* gone a step later; persistent growth settles within three steps).  planes_used != 0: the     */
/* pass wrote planes with this bound -- if M                                                    */
/* left [2^-7, 2^15] (fp16 overflow of the hi plane at 2^16, precision loss below) the sticky   */
/* timeout flag of `bwd_workspace` is raised, i.e. the step is vetoed and re-run exactly like   */
/* a step whose persistent kernel gave up (asr_lstm_status).                                    */
int asr_lstm_dz_guard(const float* dz_absmax, float* dz_bound, int planes_used,
                      void* bwd_workspace, asr_stream_t stream);
size_t asr_lstm_workspace_bytes(const asr_lstm_args* a, int backward);
int asr_lstm_seq_fwd(const asr_lstm_args* a, void* workspace, size_t ws_bytes,
                     asr_stream_t stream);
int asr_lstm_seq_bwd(const asr_lstm_args* a, void* workspace, size_t ws_bytes,
                     asr_stream_t stream);
/* Synchronises `stream`, then returns 0 or ASR_ERR_TIMEOUT if a persistent
 * kernel that used this workspace abandoned a bounded spin (results invalid)
 * in ANY call since the previous asr_lstm_status on it: the first int of the
 * workspace is a sticky flag that only this function clears (the workspace's
 * first 256 bytes must therefore be zero before its first use).  A host that
 * never wants to synchronise may instead copy that int back with its own
 * asynchronous readback once per training step.                             */
int asr_lstm_status(const void* workspace, asr_stream_t stream);
/* Launch plan the library would use (diagnostics / DESIGN.md numbers).       */
int asr_lstm_plan(const asr_lstm_args* a, int backward, int* k_split,
                  int* k_per_lane, int* blocks, int* chains_per_launch);
/* Synchronises `stream`; number of chains of the last call on this workspace
 * that ran on the same-XCD (L2) transport (diagnostic), or a negative status. */
int asr_lstm_fast_chains(const void* workspace, asr_stream_t stream);
/* Debug: hand-off timeline of the last forward launch made under ASR_LSTM_DBG & 128:       */
/* out[((block*4 + wave)*16 + step)*2 + {0 data arrived, 1 published}], 100 MHz ticks.      */
int asr_lstm_trace(long long* out, size_t n_words, asr_stream_t stream);
/* Debug (env ASR_LSTM_DBG & 32): per-phase shader-clock ticks of workgroup 0 of the
 * last call's first chain, summed over its steps: 4 waves x 6 phases {arithmetic
 * before the gather, waiting for it, arithmetic behind it, barrier, products +
 * publish, issuing the next gather}.                                           */
int asr_lstm_profile(const void* workspace, asr_stream_t stream, long long* out24);

/* ------------------------------------------------------------------------ */
/* K14 SimpleRNN recurrence of a Bidirectional layer (Keras 1.2.2            */
/* SimpleRNN.step: h_t = act(x_t W + b + h_{t-1} U); csrc/rnn.hip).          */
/* Forward: h = act(zx + (h_prev (.) mask_u) @ U) with zx = x @ W + b from   */
/* the GEMMs; direction 1 walks the padded slab from T-1 down to 0 and its   */
/* h stays in frame order.  BPTT: dz = (dy + (dz_next @ U^T) (.) mask_u)     */
/* (.) act'(h), act' from h alone (clipped relu: 1 on 0 < h < clip).  dW,    */
/* dU, db, dx come from asr_gemm / asr_colsum.  Exact fp32 products.         */
/* ------------------------------------------------------------------------ */
#define ASR_ACT_CLIPPED_RELU 7
typedef struct asr_rnn_args {
  int T, n_pad, H;       /* H: padded width, a multiple of 4; n_pad a multiple of 16    */
  int mode;              /* 0 = the plan's form, 1 = stepwise (one launch per step),    */
                         /* 2 = persistent (ASR_ERR_INVALID if it would not be resident) */
  int activation;        /* 0 tanh, 1 relu, 4 linear, ASR_ACT_CLIPPED_RELU              */
  float clip;            /* max_value of the clipped relu                               */
  const float* U;        /* (2, H, H) per direction, Keras [in][out]                    */
  const float* mask_u;   /* optional (2, n_pad, H) B_U, constant over time               */
  const float* zx;       /* forward: (T, n_pad, 2, H) = x @ W + b                        */
  float* h;              /* (T, n_pad, 2, H): forward writes it, BPTT reads it           */
  float* y_sum;          /* forward, optional: (T, n_pad, H) = h_f + h_b ('sum' merge)   */
  const float* dy;       /* BPTT: gradient of the layer output, row (t, n) at dy_ld      */
  int dy_ld;             /*   floats per (t, n) row: 2H (concat) or H (sum)              */
  int dy_dir_stride;     /*   floats between the two directions' dy: H (concat), 0 (sum) */
  float* dz;             /* BPTT: (T, n_pad, 2, H) gradient of the pre-activation        */
  float* db_part;        /* BPTT, optional: (n_pad/16, 2, H) per-batch-tile sums of dz   */
  float* dz_absmax;      /* BPTT, optional: max |dz| (written, not accumulated)          */
} asr_rnn_args;
/* Workspace: the first 256 bytes hold a sticky timeout word with the contract of            */
/* asr_lstm_status (which may be called on it); zero them before the first use.              */
size_t asr_rnn_workspace_bytes(const asr_rnn_args* a, int backward);
int asr_rnn_seq_fwd(const asr_rnn_args* a, void* workspace, size_t ws_bytes,
                    asr_stream_t stream);
int asr_rnn_seq_bwd(const asr_rnn_args* a, void* workspace, size_t ws_bytes,
                    asr_stream_t stream);
/* The form the library would run (persistent 1 / stepwise 0) and its geometry: batch rows    */
/* and units per workgroup, workgroups per launch (both directions).                          */
int asr_rnn_plan(const asr_rnn_args* a, int backward, int* persistent, int* rows, int* units,
                 int* blocks);
/* Element-wise Activation layer: y = act(x); dx = dy (.) act'(y) (ids as asr_rnn_args).      */
int asr_activation_fwd(const float* x, float* y, int64_t n, int activation, float clip,
                       asr_stream_t stream);
int asr_activation_bwd(const float* dy, const float* y, float* dx, int64_t n, int activation,
                       float clip, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K16 GRU recurrence of a Bidirectional layer (Keras 1.2.2 GRU.step,        */
/* consume_less='gpu', inner_activation='hard_sigmoid'; csrc/gru.hip).       */
/* U = [U_z | U_r | U_h] (H, 3H) per direction, zx = x @ W + b in the same   */
/* column order, m = h_prev (.) mask_u, hs(a) = clip(0.2 a + 0.5, 0, 1):     */
/*   z = hs(zx_z + m U_z), r = hs(zx_r + m U_r), hh = act(zx_h + (r (.) m)   */
/*   U_h), h = z (.) h_prev + (1 - z) (.) hh   (reset gate BEFORE the        */
/* product).  Direction 1 walks the padded slab from T-1 down to 0; all      */
/* slabs stay in frame order.  BPTT, g = dy + carry:                         */
/*   da_h = g (1 - z) act'(hh), da_z = g (h_prev - hh) hs'(z),               */
/*   q = da_h U_h^T, da_r = q m hs'(r),                                      */
/*   carry = g z + (q r + [da_z | da_r] [U_z | U_r]^T) (.) mask_u            */
/* with hs' = 0.2 where 0 < gate < 1 else 0, read from the SAVED gates, and  */
/* act' from hh alone.  dW, dU (dU_z, dU_r from m, dU_h from rm), db, dx     */
/* come from asr_gemm / asr_colsum.  Exact fp32 products, no float atomics   */
/* (repeats are bit-identical).  Stepwise only: two launches per step.       */
/* ------------------------------------------------------------------------ */
typedef struct asr_gru_args {
  int T, n_pad, H;       /* H: padded width, a multiple of 4; n_pad a multiple of 16    */
  int mode;              /* 0 = the plan's form, 1 = stepwise; 2 (persistent) does not   */
                         /* exist for this cell: ASR_ERR_INVALID                         */
  int activation;        /* 0 tanh, 1 relu, 4 linear, ASR_ACT_CLIPPED_RELU              */
  float clip;            /* max_value of the clipped relu                               */
  const float* U;        /* (2, H, 3H) per direction, Keras [in][out], blocks z, r, h   */
  const float* mask_u;   /* optional (2, n_pad, H) B_U, constant over time               */
  const float* zx;       /* forward: (T, n_pad, 2, 3H) = x @ W + b                       */
  float* h;              /* (T, n_pad, 2, H): forward writes it, BPTT reads it           */
  float* gates;          /* (T, n_pad, 2, 3H) z | r | hh: forward writes, BPTT reads     */
  float* rm;             /* forward: (T, n_pad, 2, H) r (.) m, written (left operand of  */
                         /*   dU_h; 0 at each direction's first processed frame)         */
  float* y_sum;          /* forward, optional: (T, n_pad, H) = h_f + h_b ('sum' merge)   */
  const float* dy;       /* BPTT: gradient of the layer output, row (t, n) at dy_ld      */
  int dy_ld;             /*   floats per (t, n) row: 2H (concat) or H (sum)              */
  int dy_dir_stride;     /*   floats between the two directions' dy: H (concat), 0 (sum) */
  float* da;             /* BPTT: (T, n_pad, 2, 3H) da_z | da_r | da_h                   */
  float* db_part;        /* BPTT, optional: (n_pad/16, 2, 3H) per-batch-tile sums of da  */
  float* dz_absmax;      /* BPTT, optional: max |da| (written, not accumulated)          */
} asr_gru_args;
/* Workspace: scratch only (BPTT: U^T and two (n_pad, 2, H) vectors); no status words.       */
size_t asr_gru_workspace_bytes(const asr_gru_args* a, int backward);
int asr_gru_seq_fwd(const asr_gru_args* a, void* workspace, size_t ws_bytes,
                    asr_stream_t stream);
int asr_gru_seq_bwd(const asr_gru_args* a, void* workspace, size_t ws_bytes,
                    asr_stream_t stream);
/* The form the library runs (persistent: always 0) and its geometry: batch rows and output   */
/* columns per workgroup, workgroups of the widest launch of a step (both directions).        */
int asr_gru_plan(const asr_gru_args* a, int backward, int* persistent, int* rows, int* units,
                 int* blocks);

/* ------------------------------------------------------------------------ */
/* K28 UNIDIRECTIONAL GRU recurrence with a carried state (csrc/gru.hip: the */
/* K16 step kernel with one direction in every slab).  The cell, BPTT and    */
/* the saved slopes are K16's; frames run 0 .. T-1 in order and no slab has  */
/* a direction axis.  The tile plan is the one asr_gru_plan gives for the    */
/* same (n_pad, H), so with h0 = NULL every output equals direction 0 of the */
/* K16 call on the same operands bit for bit.                                */
/* The forward pass may start from a state: h0 is h before frame 0 (NULL:    */
/* zeros, and frame 0 skips its two products as K16 does), and h_last, when  */
/* given, receives h[T-1] from the epilogue of the last launch (no extra     */
/* launch).  Frame 0 reads h0 by the code that reads h[t-1] at t > 0, so one */
/* call over T frames and two calls over [0, k) and [k, T) with h0 = the     */
/* first call's h_last give the same bits.  h_last == h0 is refused: a call  */
/* leaves the state it starts from intact (it can be repeated), and a caller */
/* keeps two buffers and swaps them.  BPTT starts from the zero state: it    */
/* takes neither.  Stepwise only: two launches per frame, no float atomics.  */
/* Every argument error (H % 4, n_pad % 16, T < 1, a missing pointer, the    */
/* alias, mode 2, an unknown activation, a short workspace) is refused with  */
/* ASR_ERR_INVALID before any device call.                                   */
/* ------------------------------------------------------------------------ */
typedef struct asr_gru_uni_args {
  int T, n_pad, H;       /* as asr_gru_args                                             */
  int mode;              /* 0 = the plan's form, 1 = stepwise; 2: ASR_ERR_INVALID        */
  int activation;        /* 0 tanh, 1 relu, 4 linear, ASR_ACT_CLIPPED_RELU              */
  float clip;            /* max_value of the clipped relu                               */
  const float* U;        /* (H, 3H), Keras [in][out], blocks z, r, h                    */
  const float* mask_u;   /* optional (n_pad, H) B_U, constant over time                  */
  const float* zx;       /* forward: (T, n_pad, 3H) = x @ W + b                          */
  float* h;              /* (T, n_pad, H): forward writes it, BPTT reads it              */
  float* gates;          /* (T, n_pad, 3H) z | r | hh: forward writes, BPTT reads        */
  float* rm;             /* forward: (T, n_pad, H) r (.) m, written (left operand of     */
                         /*   dU_h)                                                      */
  const float* h0;       /* forward, optional: (n_pad, H) state before frame 0           */
  float* h_last;         /* forward, optional: (n_pad, H) <- h[T-1]; never h0            */
  const float* dy;       /* BPTT: gradient of the layer output, row (t, n) at dy_ld      */
  int dy_ld;             /*   floats per (t, n) row, >= H, a multiple of 4               */
  float* da;             /* BPTT: (T, n_pad, 3H) da_z | da_r | da_h                      */
  float* db_part;        /* BPTT, optional: (n_pad/16, 3H) per-batch-tile sums of da     */
  float* dz_absmax;      /* BPTT, optional: max |da| (written, not accumulated)          */
} asr_gru_uni_args;
/* Workspace: scratch only (BPTT: U^T and two (n_pad, H) vectors); no status words.          */
size_t asr_gru_uni_workspace_bytes(const asr_gru_uni_args* a, int backward);
int asr_gru_uni_seq_fwd(const asr_gru_uni_args* a, void* workspace, size_t ws_bytes,
                        asr_stream_t stream);
int asr_gru_uni_seq_bwd(const asr_gru_uni_args* a, void* workspace, size_t ws_bytes,
                        asr_stream_t stream);
/* As asr_gru_plan: the same rows and units, half the workgroups.                             */
int asr_gru_uni_plan(const asr_gru_uni_args* a, int backward, int* persistent, int* rows,
                     int* units, int* blocks);

/* ------------------------------------------------------------------------ */
/* K29 UNIDIRECTIONAL LSTM recurrence with a carried state                   */
/* (csrc/lstm_uni.hip; a bare LSTM(H)(x), brsmv1(bidirectional=False)).      */
/* The plain cell of the reference (core/layers.py:432-469 without mi,       */
/* zoneout or layer normalisation), one direction, frames 0 .. T-1 in order, */
/* with m = h_prev (.) B_U:                                                  */
/*     z = zx + m @ U;  i, f, o = hard_sigmoid;  g = act(z_c);               */
/*     c = f c_prev + i g;  h = o act(c).                                    */
/* NOT the persistent kernels of asr_lstm_seq_*: a stepwise kernel on the    */
/* reduction core of csrc/rec_tile.h, ONE launch per frame in either pass,   */
/* exact fp32 FMAs in a fixed order, no float atomics, no workgroup waiting  */
/* on another, no status words.  Layouts are the LSTM gate layout, unit-     */
/* major / gate-minor ([unit * 4 + gate], gates i, f, c, o), and no slab has */
/* a direction axis.                                                         */
/* The forward pass may start from a state: (h0, c0) are h and c before      */
/* frame 0 (both or neither; NULL: zeros), and (h_last, c_last), both or     */
/* neither, receive h[T-1] and cell[T-1] from the epilogue of the last       */
/* launch (no extra launch).  Frame 0 reads the state by the code that reads */
/* h[t-1], cell[t-1] at t > 0, so one call over T frames and two calls over  */
/* [0, k) and [k, T) that hand the state on give the same bits.  Any alias   */
/* between {h_last, c_last} and {h0, c0} is refused: a call leaves the state */
/* it starts from intact (it can be repeated); a caller keeps two buffers of */
/* each and swaps them.  BPTT starts from the zero state: it takes none.     */
/* Every argument error (H % 4, n_pad % 16, T < 1, mode 2, an activation id  */
/* outside 0..6, a missing U / h / cell / gates / zx / dy / dz, a dy_ld      */
/* below H or no multiple of 4, half a state pair, an aliased state, a state */
/* given to BPTT, a short workspace) is refused with ASR_ERR_INVALID and a   */
/* message before any device call.                                           */
/* ------------------------------------------------------------------------ */
typedef struct asr_lstm_uni_args {
  int T, n_pad, H;       /* frames, padded batch (multiple of 16), units (multiple of 4) */
  int mode;              /* 0 = the plan's form, 1 = stepwise; 2: ASR_ERR_INVALID        */
  int activation;        /* as asr_lstm_args.activation: 0 tanh .. 6 softplus            */
  const float* U;        /* (H, 4H), [k][unit * 4 + gate]                                */
  const float* mask_u;   /* optional (n_pad, H) B_U, constant over time                  */
  const float* zx;       /* forward: (T, n_pad, 4H) = x @ W + b                          */
  float* h;              /* (T, n_pad, H): forward writes it                             */
  float* cell;           /* (T, n_pad, H): forward writes it, BPTT reads it              */
  float* gates;          /* (T, n_pad, 4H) post-activation i, f, g, o: forward writes,   */
                         /*   BPTT reads                                                 */
  const float* h0;       /* forward, optional: (n_pad, H) h before frame 0 ...           */
  const float* c0;       /*   ... and c before frame 0 (both or neither)                 */
  float* h_last;         /* forward, optional: (n_pad, H) <- h[T-1] ...                  */
  float* c_last;         /*   ... and <- cell[T-1] (both or neither; never h0 / c0)      */
  const float* dy;       /* BPTT: gradient of the layer output, row (t, n) at dy_ld      */
  int dy_ld;             /*   floats per (t, n) row, >= H, a multiple of 4               */
  float* dz;             /* BPTT: (T, n_pad, 4H) gradient of the gate pre-activations    */
  float* db_part;        /* BPTT, optional: (n_pad/16, 4H) per-batch-tile sums of dz     */
  float* dz_absmax;      /* BPTT, optional: max |dz| (written, not accumulated)          */
} asr_lstm_uni_args;
/* Workspace: scratch only (BPTT: U^T and one (n_pad, H) vector); no status words.           */
size_t asr_lstm_uni_workspace_bytes(const asr_lstm_uni_args* a, int backward);
int asr_lstm_uni_seq_fwd(const asr_lstm_uni_args* a, void* workspace, size_t ws_bytes,
                         asr_stream_t stream);
int asr_lstm_uni_seq_bwd(const asr_lstm_uni_args* a, void* workspace, size_t ws_bytes,
                         asr_stream_t stream);
/* The launch geometry: *persistent = 0, *rows = batch rows and *units = tile columns of a    */
/* workgroup (rows x units = 1024), *blocks = workgroups per launch (forward: 4H gate         */
/* columns; BPTT: H units).                                                                   */
int asr_lstm_uni_plan(const asr_lstm_uni_args* a, int backward, int* persistent, int* rows,
                      int* units, int* blocks);

/* ------------------------------------------------------------------------ */
/* K17 Recurrent Highway Network recurrence of a Bidirectional layer (Zilly  */
/* et al. 2016; the reference's RHN layer, core/layers.py:92-353;            */
/* csrc/rhn.hip).  depth L >= 1, C = 2 column blocks h | t when coupling,    */
/* C = 3 (h | t | c) otherwise.  Per direction U_l (H, C H) and b_l (C H),   */
/* l = 0 .. L-1; zx = x @ W (NO bias) in the same column order;              */
/* hs(a) = clip(0.2 a + 0.5, 0, 1); s the state carried in (0 at the         */
/* direction's first processed frame):                                       */
/*   for l in 0 .. L-1:                                                      */
/*     a  = (l == 0 ? zx_t : 0) + (s (.) mask_u[l]) U_l + b_l                */
/*     hh = act(a_h), tg = hs(a_t), cg = coupling ? 1 - tg : hs(a_c)         */
/*     s  = hh tg + s cg          (the carry uses the UNMASKED s)            */
/*   y_t = s                      (the state after level L-1)                */
/* Direction 1 walks the padded slab from T-1 down to 0; all slabs stay in   */
/* frame order.  BPTT, g = gradient of the state a level wrote (dy_t is      */
/* added at level L-1 of every frame), s_prev the state that level read:     */
/*   da_h = g tg act'(hh)                                                    */
/*   da_t = g (hh - s_prev) hs'(tg)   (coupling; else g hh hs'(tg))          */
/*   da_c = g s_prev hs'(cg)          (no coupling only)                     */
/*   g_prev = g cg + (da U_l^T) (.) mask_u[l]                                */
/* with hs' = 0.2 where 0 < gate < 1 else 0, read from the SAVED gates, and  */
/* act' from hh alone.  dW, dU_l, db_l, dx come from asr_gemm / asr_colsum.  */
/* Exact fp32 products, no float atomics (repeats are bit-identical).        */
/* Stepwise only: one launch per level and frame.  The saved tensors are     */
/* level-major, so every level is an ordinary time-major slab.               */
/* ------------------------------------------------------------------------ */
typedef struct asr_rhn_args {
  int T, n_pad, H;       /* H: padded width, a multiple of 4; n_pad a multiple of 16    */
  int depth;             /* L >= 1 highway levels per frame                             */
  int coupling;          /* 1: cg = 1 - tg, C = 2 blocks; 0: own carry gate, C = 3      */
  int mode;              /* 0 = the plan's form, 1 = stepwise; 2 (persistent) does not   */
                         /* exist for this cell: ASR_ERR_INVALID                         */
  int activation;        /* 0 tanh, 1 relu, 4 linear, ASR_ACT_CLIPPED_RELU              */
  float clip;            /* max_value of the clipped relu                               */
  const float* U;        /* (2, L, H, C H): per direction and level, [in][out]          */
  const float* b;        /* (2, L, C H); forward only                                   */
  const float* mask_u;   /* optional (2, L, n_pad, H) B_U: one mask per level, constant  */
                         /*   over time                                                  */
  const float* zx;       /* forward: (T, n_pad, 2, C H) = x @ W                          */
  float* h;              /* (L, T, n_pad, 2, H) states of every level: forward writes,   */
                         /*   BPTT reads; slab L-1 is the layer output                   */
  float* gates;          /* (L, T, n_pad, 2, C H) hh | tg | [cg]: forward writes, BPTT   */
                         /*   reads                                                      */
  float* y_sum;          /* forward, optional: (T, n_pad, H) = y_f + y_b ('sum' merge)   */
  const float* dy;       /* BPTT: gradient of the layer output, row (t, n) at dy_ld      */
  int dy_ld;             /*   floats per (t, n) row: 2H (concat) or H (sum)              */
  int dy_dir_stride;     /*   floats between the two directions' dy: H (concat), 0 (sum) */
  float* da;             /* BPTT: (L, T, n_pad, 2, C H) da_h | da_t | [da_c]             */
  float* db_part;        /* BPTT, optional: (n_pad/16, 2, L, C H) per-batch-tile sums    */
  float* dz_absmax;      /* BPTT, optional: max |da| (written, not accumulated)          */
} asr_rhn_args;
/* Workspace: scratch only (forward: a tile-interleaved copy of every U_l; BPTT: every U_l^T  */
/* and one (n_pad, 2, H) vector).                                                             */
size_t asr_rhn_workspace_bytes(const asr_rhn_args* a, int backward);
int asr_rhn_seq_fwd(const asr_rhn_args* a, void* workspace, size_t ws_bytes,
                    asr_stream_t stream);
int asr_rhn_seq_bwd(const asr_rhn_args* a, void* workspace, size_t ws_bytes,
                    asr_stream_t stream);
/* The form the library runs (persistent: always 0) and its geometry: batch rows and state    */
/* columns per workgroup, workgroups of a launch (both directions).                           */
int asr_rhn_plan(const asr_rhn_args* a, int backward, int* persistent, int* rows, int* units,
                 int* blocks);

/* ------------------------------------------------------------------------ */
/* K15 BatchNormalization (Keras 1.2.2, mode 0, axis -1; csrc/batchnorm.hip) */
/* over a time-major slab x (T, n_pad, ld), ld a multiple of 4, 16-byte     */
/* aligned.  Columns [0, W) are normalised, [W, ld) and the padding rows     */
/* n >= N of y / dx are written as zeros.  channel = column % C: C == W is a */
/* plain (N, T, W) tensor, C < W the (N, T, F, C) conv image (W = F * C, no  */
/* pad columns, C a multiple of 4, at most 256).  Statistics over every real */
/* row of all T frames, biased variance, fp64 partials added in a fixed      */
/* order (no float atomics: bit-identical repeats).                          */
/*  stats (4C floats): [mean_hi | mean_lo | 1/sqrt(var + eps) | var], the    */
/*    mean split into two floats (x - mean stays exact for large means).     */
/*  moments (4 + 2C floats, optional): [w, 0, 0, 0 | w d | w (var + d^2)],   */
/*    d = mean - shift[c] (shift NULL: the batch mean itself).  Sums of such */
/*    blocks over data-parallel ranks (w = real frames of the rank, shift =  */
/*    the rank-invariant running mean) are the moments of the union batch.  */
/*  clip > 0 fuses a following clipped ReLU: y = min(max(y, 0), clip); the   */
/*    backward masks dy with 0 < y < clip (y recomputed from x).             */
/* ------------------------------------------------------------------------ */
size_t asr_bn_workspace_bytes(int T, int N, int n_pad, int ld, int W, int C);
int asr_bn_fwd_train(const float* x, float* y, const float* gamma, const float* beta,
                     float* stats, float* moments, const float* shift, float weight, int T, int N,
                     int n_pad, int ld, int W, int C, float eps, float clip, void* workspace,
                     size_t ws_bytes, asr_stream_t stream);
/* y = gamma (x - running_mean) / sqrt(running_var + eps) + beta (no workspace).              */
int asr_bn_fwd_infer(const float* x, float* y, const float* gamma, const float* beta,
                     const float* running_mean, const float* running_var, int T, int N, int n_pad,
                     int ld, int W, int C, float eps, float clip, asr_stream_t stream);
/* dgamma / dbeta (C floats) are written, not accumulated; dx may be NULL (no input gradient). */
int asr_bn_bwd(const float* x, const float* dy, const float* gamma, const float* beta,
               const float* stats, float* dx, float* dgamma, float* dbeta, int T, int N,
               int n_pad, int ld, int W, int C, float clip, void* workspace, size_t ws_bytes,
               asr_stream_t stream);
/* r <- momentum r + (1 - momentum) batch for the running mean and variance (no debias), the   */
/* batch moments taken from `moments` (shift as given to asr_bn_fwd_train; NULL: the running   */
/* mean).  Skipped on the device when moments[0] <= 0 or when any of the four flag words (device */
/* ints, NULL allowed; the sticky timeout words / all-reduced flag slots asr_optim_guard reads) */
/* holds a non-zero bit pattern: a vetoed step leaves the statistics alone.                     */
int asr_bn_update_running(float* running_mean, float* running_var, const float* moments,
                          const float* shift, int C, float momentum, const int* flag_a,
                          const int* flag_b, const int* flag_c, const int* flag_d,
                          asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K18 sequence-wise BatchNormalization of a recurrent layer's input         */
/* projection (arXiv 1510.01378), csrc/batchnorm.hip.  p, y, da, dp are      */
/* time-major slabs (T, n_pad, ld) with W <= ld real columns, one channel    */
/* per column; lens (N device ints, NULL: every frame) holds each sample's   */
/* length on this time axis, clamped to [0, T] inside.  The statistics are   */
/* taken over the VALID rows (n < N, t < len_n) only; every real row (n < N, */
/* all T frames) is normalised with them.  Rows n >= N and pad columns of y  */
/* and dp are written as zeros.  No float atomics: bit-identical repeats.    */
/*  stats (4W + 4 floats): [mean_hi | mean_lo | 1/sqrt(var + eps) | var |    */
/*    |V|, 0, 0, 0], |V| the number of valid rows.                           */
/*  moments (4 + 2W floats, optional): the block of asr_bn_fwd_train with    */
/*    w = weight * |V|, for asr_bn_update_running (C = W).                   */
/*  asr_seqbn_bwd: dgamma = sum da * xhat and dbeta = sum da (optional) over */
/*    every real row, written, not accumulated; dp = gamma invstd (da -      */
/*    [row valid] (dbeta + xhat dgamma) / |V|); dp_absmax (optional) <- max  */
/*    |dp|.  xhat is recomputed from p and stats, never from y.              */
/* ------------------------------------------------------------------------ */
size_t asr_seqbn_workspace_bytes(int T, int N, int n_pad, int ld, int W);
int asr_seqbn_fwd_train(const float* p, float* y, const float* gamma, const float* beta,
                        const int* lens, float* stats, float* moments, const float* shift,
                        float weight, int T, int N, int n_pad, int ld, int W, float eps,
                        void* workspace, size_t ws_bytes, asr_stream_t stream);
int asr_seqbn_fwd_infer(const float* p, float* y, const float* gamma, const float* beta,
                        const float* running_mean, const float* running_var, int T, int N,
                        int n_pad, int ld, int W, float eps, asr_stream_t stream);
int asr_seqbn_bwd(const float* p, const float* da, const float* gamma, const int* lens,
                  const float* stats, float* dp, float* dgamma, float* dbeta, float* dp_absmax,
                  int T, int N, int n_pad, int ld, int W, void* workspace, size_t ws_bytes,
                  asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K20 LayerNormalization over the feature axis (arXiv 1607.06450;           */
/* csrc/layernorm.hip).  x, y, dy, dx are time-major slabs (T, n_pad, ld),   */
/* ld a multiple of 4 and at most asr_ln_max_width() (4096), 16-byte         */
/* aligned.  The real columns of a row are `segs` blocks of H columns at a   */
/* stride of Hp (Hp a multiple of 4, H <= Hp, segs * Hp <= ld); every other  */
/* column is padding, may hold anything and is never read into a sum.  Per   */
/* real row (n < N of every frame): y = (x - mu) r gain + bias, mu and the   */
/* BIASED variance over the segs * H real columns, r = 1 / sqrt(var + eps).  */
/* Pad columns and the padding rows n >= N of y / dx are written as zeros.   */
/*  gain, bias, dgain, dbias: ld floats, indexed by physical column.         */
/*  stats (2 T n_pad floats; NULL in asr_ln_fwd: not kept): (mu, r) of row   */
/*    t * n_pad + n, written for the real rows only.                         */
/*  asr_ln_bwd: dx = r (g - mean(g) - xhat mean(g xhat)) with xhat = (x -    */
/*    mu) r and g = gain dy (NULL: no input gradient); dgain = sum dy xhat   */
/*    and dbias = sum dy over the real rows, WRITTEN, not accumulated (zeros */
/*    in the pad columns).  Per-workgroup partials in the workspace, added   */
/*    in a fixed order: no float atomics, bit-identical repeats.             */
/* Plain scalar arguments, no struct: the ABI version stays.                 */
/* ------------------------------------------------------------------------ */
int asr_ln_max_width(void);
size_t asr_ln_workspace_bytes(int T, int N, int n_pad, int ld, int H, int Hp, int segs);
int asr_ln_fwd(const float* x, float* y, const float* gain, const float* bias, float* stats,
               int T, int N, int n_pad, int ld, int H, int Hp, int segs, float eps,
               asr_stream_t stream);
int asr_ln_bwd(const float* x, const float* dy, const float* gain, const float* stats, float* dx,
               float* dgain, float* dbias, int T, int N, int n_pad, int ld, int H, int Hp,
               int segs, void* workspace, size_t ws_bytes, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K21 multi-head self-attention core, fused, forward and backward           */
/* (arXiv 1706.03762; csrc/attention.hip).  qkv is a time-major slab         */
/* (T, n_pad, ld >= 3D), column blocks [Q | K | V] of D = heads * dh columns */
/* each, head h in columns h dh .. (h + 1) dh - 1 of its block (what one     */
/* x @ W_qkv + b_qkv GEMM writes).  For every real sample n < N, head h and  */
/* query frame t (all T frames are queries; only keys are masked):           */
/*   s[t,u] = scale q_t . k_u   for u < lens[n]  (u < T when lens is NULL)   */
/*   p      = softmax_u(s)      keys u >= lens[n] carry probability exactly 0*/
/*   out_t  = sum_u p[t,u] v_u,   lse_t = log sum_u exp s[t,u]               */
/* Backward, with D_t = dout_t . out_t:  dV = P^T dO,                        */
/*   dS = P (.) (dO V^T - D),  dQ = scale dS K,  dK = scale dS^T Q;          */
/*   masked keys get dK = dV = exactly 0.                                    */
/* Rows n >= N and the pad columns (>= D of out, >= 3D of dqkv) are written  */
/* as exact zeros.  The T x T scores never reach memory: 64-frame query and  */
/* key tiles go through LDS with a running maximum / sum (forward) or p      */
/* recomputed from lse (backward).  Exact fp32 products (FMA), fp32 sums,    */
/* base-2 exponentials; no float atomics (bit-identical repeats); no         */
/* workgroup waits on another.  dh a multiple of 16 in 16 .. 128, heads >= 1,*/
/* any T >= 1, ld and ld_out multiples of 4, 16-byte aligned slabs; anything */
/* else is ASR_ERR_INVALID.                                                  */
/* ------------------------------------------------------------------------ */
typedef struct asr_attn_args {
  int T, N, n_pad;       /* frames, real samples, padded samples per frame               */
  int heads, dh;         /* D = heads * dh                                               */
  int ld, ld_out;        /* floats per (t, n) row of qkv / dqkv and of out / dout        */
  float scale;           /* of the scores, usually 1 / sqrt(dh)                          */
  const float* qkv;      /* (T, n_pad, ld)                                               */
  const int* lens;       /* optional device int32 (N): 1 <= lens[n] <= T valid keys      */
                         /*   (a value outside is clamped into that range)               */
  float* out;            /* (T, n_pad, ld_out): forward writes it, backward reads it     */
  float* lse;            /* (T, n_pad, heads): forward writes it when not NULL (real     */
                         /*   samples only), backward reads it                           */
  const float* dout;     /* backward: (T, n_pad, ld_out)                                 */
  float* dqkv;           /* backward: (T, n_pad, ld), dQ | dK | dV                       */
} asr_attn_args;
/* Workspace of asr_attn_bwd (D of every row); 0 for a geometry that is refused.             */
size_t asr_attn_workspace_bytes(const asr_attn_args* a);
int asr_attn_fwd(const asr_attn_args* a, asr_stream_t stream);
int asr_attn_bwd(const asr_attn_args* a, void* workspace, size_t ws_bytes, asr_stream_t stream);
/* The geometry the library runs: query and key tile lengths, workgroups of one launch, LDS   */
/* bytes per workgroup (any pointer may be NULL).                                             */
int asr_attn_plan(const asr_attn_args* a, int backward, int* bq, int* bk, int* blocks,
                  int* lds_bytes);
/* K25 limited-context attention: K21 (and, below, K24) under a WINDOW of three integers,      */
/*   chunk >= 1;  left >= -1 frames (-1: unlimited);  right >= 0 frames.                      */
/* For query frame t let c0 = (t / chunk) * chunk.  Key u is visible to t iff                 */
/*   lo(t) <= u < hi(t)  and  u < lens[n],   hi(t) = c0 + chunk + right,                      */
/*                                           lo(t) = left < 0 ? 0 : max(0, c0 - left).        */
/* chunk 1, right 0 is the causal mask (a finite left: a sliding window); chunk 1, right R a  */
/* symmetric window; chunk C chunk-wise attention, whose look-ahead chunk - 1 + right does    */
/* not grow with depth.  lo and hi are non-decreasing in t.  Every other key carries          */
/* probability exactly 0 (a select: nothing it holds reaches a result).  A row with NO        */
/* visible key (a time-padding query with lo(t) >= lens[n]) has out_t = exactly 0 and lse_t = */
/* exactly 0 and adds exactly 0 to every gradient (dQ_t = 0).  A key no query sees gets dK =  */
/* dV = exactly 0.  A workgroup visits only the tiles that hold a visible (query, key) pair:  */
/* for a query tile the key tiles that meet [lo(first query), min(hi(last query), len)), for  */
/* a key tile at k0 the query tiles with lo(first) <= k0 + 63 and hi(last) > k0 -- one        */
/* contiguous range each.  The argument struct, the workspace and everything else are those   */
/* of the unwindowed calls, whose results do not change.  chunk < 1, left < -1, right < 0 or  */
/* a NULL window: ASR_ERR_INVALID before any device call.                                     */
typedef struct asr_attn_window { int chunk, left, right; } asr_attn_window;
int asr_attn_win_fwd(const asr_attn_args* a, const asr_attn_window* w, asr_stream_t stream);
int asr_attn_win_bwd(const asr_attn_args* a, const asr_attn_window* w, void* workspace,
                     size_t ws_bytes, asr_stream_t stream);
/* asr_attn_plan, and tile_pairs: the (query tile, key tile) pairs one (sample, head) of the  */
/* forward launch visits when lens is NULL, from the helper the kernels take their loop       */
/* bounds from (any pointer may be NULL).                                                     */
int asr_attn_win_plan(const asr_attn_args* a, const asr_attn_window* w, int backward, int* bq,
                      int* bk, int* blocks, int* lds_bytes, long long* tile_pairs);
/* Sinusoidal positional encoding added to a slab: y[t, n, f] = x[t, n, f] + pe[t, f] for    */
/* n < N and f < D, zeros elsewhere; x, y (T, n_pad, ld >= D), pe (T, D) with                 */
/* pe[t, 2i] = sin(t / 10000^(2i / D)), pe[t, 2i + 1] = cos(t / 10000^(2i / D)), computed by  */
/* the caller (in float64, rounded once).  Its backward pass is the identity.                */
int asr_posenc_add(const float* x, const float* pe, float* y, int T, int N, int n_pad, int D,
                   int ld, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K24 relative positional self-attention core, fused, forward and backward  */
/* (arXiv 1901.02860 3.3 as used by arXiv 2005.08100 2.1;                    */
/* csrc/rel_attention.hip).  qkv, lens, out, lse, dout, dqkv and every       */
/* convention of K21 carry over.  pos is the projected relative table        */
/* (2T - 1, ld_pos >= D): row r + T - 1 holds pos_r, where the RELATIVE      */
/* INDEX is r = t - u, QUERY FRAME MINUS KEY FRAME (positive when the key    */
/* lies in the past), r = -(T - 1) .. T - 1; head h reads columns            */
/* h dh .. (h + 1) dh - 1.  bias_u, bias_v (D each): the position biases.    */
/*   s[t,u] = scale ((q_t + b_u) . k_u + (q_t + b_v) . pos_{t-u}), u < len_n */
/*   p = softmax_u(s),  out_t = sum_u p[t,u] v_u,  lse_t = log sum_u exp s   */
/* Backward, dS = P (.) (dO V^T - D_t):                                      */
/*   dq_t = scale sum_u dS[t,u] (k_u + pos_{t-u})                            */
/*   dk_u = scale sum_t dS[t,u] (q_t + b_u),  dv = P^T dO                    */
/*   dbias_u = scale sum_{n,t,u} dS[t,u] k_u                                 */
/*   dbias_v = scale sum_{n,t,u} dS[t,u] pos_{t-u}                           */
/*   dpos_r  = scale sum_n sum_{t-u=r, u<len_n} dS[t,u] (q_t + b_v)          */
/* dqkv, dpos, dbias_u, dbias_v are sums over all real samples and all T     */
/* query frames, WRITTEN, not accumulated; dpos rows that no valid (t, u)    */
/* pair reaches and its pad columns are exact zeros.  Neither the T x T      */
/* scores nor a T x (2T - 1) intermediate reaches memory.  No float atomics: */
/* per-sample partials of dpos and the two parts of dQ go through the        */
/* workspace and are added in a fixed order (asr_colsum).                    */
/* dh a multiple of 16 in 16 .. 64: the band of pos rows a tile pair needs   */
/* takes two more LDS tiles, with which dh 80 .. 128 does not fit the 160 KB */
/* of a CU in the backward passes; it is refused (ASR_ERR_INVALID), like any */
/* other invalid geometry, before anything touches a device.                 */
/* A new struct and new entry points only: the ABI version stays.            */
/* ------------------------------------------------------------------------ */
typedef struct asr_relattn_args {
  int T, N, n_pad;       /* frames, real samples, padded samples per frame               */
  int heads, dh;         /* D = heads * dh                                               */
  int ld, ld_out;        /* floats per (t, n) row of qkv / dqkv and of out / dout        */
  int ld_pos;            /* floats per row of pos / dpos, >= D, a multiple of 4          */
  float scale;           /* of the scores, usually 1 / sqrt(dh)                          */
  const float* qkv;      /* (T, n_pad, ld)                                               */
  const int* lens;       /* optional device int32 (N), clamped to 1 .. T                 */
  float* out;            /* (T, n_pad, ld_out)                                           */
  float* lse;            /* (T, n_pad, heads)                                            */
  const float* dout;     /* backward: (T, n_pad, ld_out)                                 */
  float* dqkv;           /* backward: (T, n_pad, ld), dQ | dK | dV                       */
  const float* pos;      /* (2T - 1, ld_pos), 16-byte aligned                            */
  const float* bias_u;   /* (D)                                                          */
  const float* bias_v;   /* (D)                                                          */
  float* dpos;           /* backward: (2T - 1, ld_pos), contiguous                       */
  float* dbias_u;        /* backward: (D)                                                */
  float* dbias_v;        /* backward: (D)                                                */
} asr_relattn_args;
/* Workspace of asr_relattn_bwd (D of every row, the two dQ slabs, the per-sample partials    */
/* of dpos, the column-sum partials); 0 for a geometry that is refused.                       */
size_t asr_relattn_workspace_bytes(const asr_relattn_args* a);
int asr_relattn_fwd(const asr_relattn_args* a, asr_stream_t stream);
int asr_relattn_bwd(const asr_relattn_args* a, void* workspace, size_t ws_bytes,
                    asr_stream_t stream);
/* Tile lengths, workgroups of the forward (or dQ / dK dV) launch and LDS bytes per workgroup */
/* (backward: of the largest of its three passes); any pointer may be NULL.                   */
int asr_relattn_plan(const asr_relattn_args* a, int backward, int* bq, int* bk, int* blocks,
                     int* lds_bytes);
/* K25 under a window (asr_attn_window above: the same definition, the same empty-row rule,   */
/* the same tile ranges).  dpos follows the masked dS: its rows with a relative index outside */
/* [-(chunk - 1 + right), left + chunk - 1] (left unlimited: T - 1 on that side) are exact    */
/* zeros, and a 64-row tile of the table wholly outside that range is written without a walk  */
/* over the keys; dbias_u and dbias_v follow as well.                                         */
int asr_relattn_win_fwd(const asr_relattn_args* a, const asr_attn_window* w, asr_stream_t stream);
int asr_relattn_win_bwd(const asr_relattn_args* a, const asr_attn_window* w, void* workspace,
                        size_t ws_bytes, asr_stream_t stream);
int asr_relattn_win_plan(const asr_relattn_args* a, const asr_attn_window* w, int backward,
                         int* bq, int* bk, int* blocks, int* lds_bytes, long long* tile_pairs);

/* ------------------------------------------------------------------------ */
/* K22 depthwise 1-D convolution over the time axis of a time-major slab     */
/* (T, n_pad, ld >= C), and the element-wise pairs of a Conformer block      */
/* (arXiv 2005.08100; csrc/dwconv.hip).  Cross-correlation, 'same' padding,  */
/* k odd in 1 .. 63, p = (k - 1) / 2, w (k, C) tap major, b (C):             */
/*   xm[u,n,c] = x[u,n,c] if 0 <= u < lens[n] else 0   (lens NULL: all T)    */
/*   y[t,n,c]  = b[c] + sum_j w[j,c] xm[t + j - p, n, c]   for EVERY t < T   */
/*   dx[u]     = sum_j w[j,c] dy[u - j + p] for u < lens[n], exactly 0 past  */
/*   dw[j,c]   = sum_{t, n < N} dy[t,n,c] xm[t + j - p, n, c]                */
/*   db[c]     = sum_{t, n < N} dy[t,n,c]                                    */
/* The mask is a select (nothing a frame >= lens[n] holds reaches an         */
/* output); lens (device int32, N) is clamped to 0 .. T.  Rows n >= N and    */
/* columns C <= col < ld of y and dx are written as exact zeros and never    */
/* read.  dw (k, C) and db (C) are WRITTEN (as asr_ln_bwd writes dgain and   */
/* dbias): per-workgroup partials in the workspace, added in a fixed order.  */
/* Exact fp32 FMAs, no float atomics (bit-identical repeats), no workgroup   */
/* waits on another.  C and ld multiples of 4, 16-byte aligned pointers;     */
/* anything else is ASR_ERR_INVALID before any device call.                  */
/* ------------------------------------------------------------------------ */
/* Workspace of asr_dwconv1d_bwd; 0 for a geometry that is refused.           */
size_t asr_dwconv1d_workspace_bytes(int T, int N, int n_pad, int C, int ld, int k);
/* The geometry the library runs: frames per time tile, workgroups of the     */
/* forward (backward = 0) or weight-gradient (1) launch, LDS bytes per        */
/* workgroup (any pointer may be NULL).                                       */
int asr_dwconv1d_plan(int T, int N, int n_pad, int C, int ld, int k, int backward, int* tile,
                      int* blocks, int* lds_bytes);
int asr_dwconv1d_fwd(const float* x, const float* w, const float* b, const int* lens, float* y,
                     int T, int N, int n_pad, int C, int ld, int k, asr_stream_t stream);
/* dx may be NULL (no input gradient wanted). */
int asr_dwconv1d_bwd(const float* x, const float* w, const float* dy, const int* lens, float* dx,
                     float* dw, float* db, int T, int N, int n_pad, int C, int ld, int k,
                     void* workspace, size_t ws_bytes, asr_stream_t stream);
/* The same with the left padding as an argument, 0 <= pad_left <= k - 1:                     */
/*   y[t] = b + sum_j w[j] xm[t + j - pad_left],  dx[u] = sum_j w[j] dy[u - j + pad_left],    */
/*   dw[j] = sum dy[t] xm[t + j - pad_left]                                                   */
/* (the input gradient is the flipped filter with padding k - 1 - pad_left).  pad_left =      */
/* k - 1 is the CAUSAL convolution: no output frame reads a later input frame.  pad_left =    */
/* (k - 1) / 2 is asr_dwconv1d_fwd / _bwd, bit for bit (they are this call).  The length      */
/* mask, the workspace, the plan and the order of the dw / db partials do not depend on it.   */
int asr_dwconv1d_pad_fwd(const float* x, const float* w, const float* b, const int* lens,
                         float* y, int T, int N, int n_pad, int C, int ld, int k, int pad_left,
                         asr_stream_t stream);
int asr_dwconv1d_pad_bwd(const float* x, const float* w, const float* dy, const int* lens,
                         float* dx, float* dw, float* db, int T, int N, int n_pad, int C, int ld,
                         int k, int pad_left, void* workspace, size_t ws_bytes,
                         asr_stream_t stream);
/* Gated linear unit over rows of ld_in >= 2C floats: y[r, c] = x[r, c] sigma(x[r, C + c]) for  */
/* c < C, zeros in C <= c < ld_out; backward recomputes sigma from x: dx[r, c] = dy sigma(g),   */
/* dx[r, C + c] = dy a sigma(g) (1 - sigma(g)), zeros in 2C <= c < ld_in.  C, ld_in, ld_out     */
/* multiples of 4.                                                                            */
int asr_glu_fwd(const float* x, float* y, int64_t rows, int C, int ld_in, int ld_out,
                asr_stream_t stream);
int asr_glu_bwd(const float* x, const float* dy, float* dx, int64_t rows, int C, int ld_in,
                int ld_out, asr_stream_t stream);
/* Swish: y = x sigma(x); dx = dy sigma(x) (1 + x (1 - sigma(x))), read from the INPUT x (the  */
/* derivative is not a function of y).  Finite for every finite x.                            */
int asr_swish_fwd(const float* x, float* y, int64_t n, asr_stream_t stream);
int asr_swish_bwd(const float* x, const float* dy, float* dx, int64_t n, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K26 cached chunk-by-chunk (streaming) inference: the forward passes of    */
/* K25's bounded-look-ahead stages on a few NEW frames of a stream, the past */
/* kept in rings by the caller (csrc/attn_tile.h states the convention once).*/
/* Forward only.  Every slab is time major, (frames, n_pad, ld).             */
/*                                                                           */
/* THE RING is a slab (R, n_pad, ld): absolute frame u of the stream lives   */
/* in ring row u % R.  A call states the absolute index t0 of its first new  */
/* frame and the count Tq of new frames, which the caller has put into the   */
/* ring beforehand (asr_ring_put).  For the attention calls R is a multiple  */
/* of 64, so that a 64-frame key tile that starts at an absolute multiple of */
/* 64 is contiguous in the ring, and the ring is valid for a call iff        */
/*   R >= t0 + Tq - (lo(t0) / 64) * 64            (lo of asr_attn_window)    */
/* asr_attn_stream_plan returns the smallest R that is valid for every t0    */
/* and every Tq <= max_tq: at most left + chunk - 1 + max_tq + 63 rounded up */
/* to 64.  Ring rows that hold frames below a query's lo are stale; they     */
/* meet probability exactly 0 and must be FINITE (0 * NaN would reach the    */
/* sum): the owner zero-fills a ring when it creates or resets it.           */
/* All of them refuse bad geometry with ASR_ERR_INVALID before any device    */
/* call; no float atomics; no workgroup waits on another.  New entry points  */
/* and one new struct only: the ABI version stays.                           */
/* ------------------------------------------------------------------------ */
/* Rows [0, Tq) of the columns [col0, col0 + cols) of src (Tq, n_pad, ld_src) into the columns */
/* [0, cols) of the ring rows (t0 + i) % ring_rows of ring (ring_rows, n_pad, ld_ring), all    */
/* n_pad samples, the wrap included.  Tq <= ring_rows; col0, cols, ld_src, ld_ring multiples   */
/* of 4; 16-byte aligned pointers.  Used for the [K | V] columns of a qkv chunk (col0 = D,     */
/* cols = 2 D) and for the input of the depthwise convolution.                                 */
int asr_ring_put(const float* src, float* ring, int Tq, int n_pad, int ld_src, int col0, int cols,
                 int ld_ring, int ring_rows, int t0, asr_stream_t stream);
typedef struct asr_attn_stream_args {
  int Tq, N, n_pad;      /* new frames, real streams, padded streams per frame             */
  int heads, dh;         /* D = heads * dh                                                 */
  int ld, ld_kv, ld_out; /* floats per row of q (>= D), of the ring (>= 2 D), of out (>= D) */
  int R, t0;             /* ring rows; absolute index of the first new frame               */
  int P, ld_pos;         /* relative form only: the table's half length and row pitch      */
  float scale;           /* of the scores, usually 1 / sqrt(dh)                            */
  const float* q;        /* (Tq, n_pad, ld): Q in columns [0, D) (a qkv chunk serves)      */
  const float* ring;     /* (R, n_pad, ld_kv): [K | V], the new frames already put         */
  const int* kv_len;     /* device int32 (N): absolute frames of stream n valid so far,    */
                         /*   the part lens plays in asr_attn_win_fwd; clamped to          */
                         /*   1 .. t0 + Tq (a key at or past t0 + Tq does not exist yet)   */
  float* out;            /* (Tq, n_pad, ld_out)                                            */
  const float* pos;      /* relative form only: (2P - 1, ld_pos), row r + P - 1 holds the  */
                         /*   relative index r = t - u; P >= left + chunk                  */
  const float* bias_u;   /* relative form only: (D)                                        */
  const float* bias_v;   /* relative form only: (D)                                        */
} asr_attn_stream_args;
/* asr_attn_win_fwd for the queries [t0, t0 + Tq) under a window with left >= 0 and right = 0: */
/* the visibility rule of K25 on absolute frame numbers, out = exactly 0 for a row with no     */
/* visible key, exact zeros in the rows n >= N and the pad columns of out, no lse.  The kernel */
/* walks the absolute 64-aligned key tiles the whole-utterance call walks, so the rows are     */
/* those of asr_attn_win_fwd on the whole qkv slab BIT FOR BIT, provided every key a query     */
/* sees is in the ring: a call ends at a multiple of chunk or at the end of the stream.  Any   */
/* Tq >= 1 (64 queries per workgroup).                                                         */
int asr_attn_stream_plan(const asr_attn_window* w, int max_tq, int* ring_rows);
int asr_attn_stream_fwd(const asr_attn_stream_args* a, const asr_attn_window* w,
                        asr_stream_t stream);
/* The same for K24 (asr_relattn_win_fwd; dh 16 .. 64).  The table does not depend on how long */
/* the stream runs: its rows are those of the whole-utterance table at the same relative       */
/* index.  Band rows a tile pair stages from outside the table are zeros and meet masked pairs */
/* only.  Bit for bit the rows of asr_relattn_win_fwd on the same table values.                */
int asr_relattn_stream_fwd(const asr_attn_stream_args* a, const asr_attn_window* w,
                           asr_stream_t stream);
/* asr_dwconv1d_pad_fwd with pad_left = k - 1 for the output frames [t0, t0 + Tq): y (Tq,      */
/* n_pad, ld); the input is a ring (ring_rows >= k - 1 + Tq, n_pad, ld) indexed row by row     */
/* (ring_rows need not be a multiple of anything); frames < 0 and frames >= lens[n] (device    */
/* int32 (N), ABSOLUTE, required, clamped to 0 .. t0 + Tq) are zeros by a select.  The taps    */
/* are added in the order of the whole-utterance call: its rows bit for bit.                   */
int asr_dwconv1d_stream_fwd(const float* ring, const float* w, const float* b, const int* lens,
                            float* y, int Tq, int N, int n_pad, int C, int ld, int k,
                            int ring_rows, int t0, asr_stream_t stream);
/* asr_ctc_greedy over one chunk of a stream's logits (T, n_pad, C); seq_len (N): the valid    */
/* frames of THIS chunk.  state (device int32, N) holds the arg-max of the stream's last valid */
/* frame, -1 before the first one; the call reads and updates it, so a repeat across the       */
/* boundary is merged.  decoded (N, T) receives the labels this chunk adds (padded with -1),   */
/* decoded_len (N) their count.                                                                */
int asr_ctc_greedy_stream(const float* logits, const int* seq_len, int* state, int T, int N,
                          int n_pad, int C, int* decoded, int* decoded_len, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K27 The device beam search (K9: asr_ctc_beam_device, asr_ctc_beam_lm_device) over a stream, */
/* one chunk (Tq, n_pad, C) of logits per call; chunk_len (device int32, N): the valid frames  */
/* of THIS chunk, 0 .. Tq.  The same kernel, resumable: any split of a stream into chunks ends */
/* with the branch table, the tree, the string and the score of one whole-utterance call over  */
/* the concatenated frames, bit for bit.                                                        */
/*   state      N records of asr_ctc_beam_stream_state_bytes / N bytes each: 8 int32 (nb,       */
/*              nblocks, frames_done, stable_node, overflow, 3 spare), then b_ob, b_ol, b_ot    */
/*              (beam_width float64 each), b_node, b_par and -- LM -- b_ctx (beam_width int32   */
/*              each).  ALL ZEROS = a fresh stream.  A record belongs to one (C, beam_width,    */
/*              max_frames, lm) and to one record of the workspace; one that cannot be that     */
/*              geometry's (nb outside 0 .. beam_width, more blocks than the frames left have   */
/*              room for) is left as it is, its overflow field set, and answered with the empty */
/*              hypothesis.                                                                     */
/*   workspace  the prefix tree, sized as asr_ctc_beam_device's for T = max_frames (about       */
/*              max_frames * beam_width * (C - 1) * 8 bytes per stream); never needs a fill,    */
/*              but must keep its contents between the calls of a stream.  Its head holds the   */
/*              work counters of asr_ctc_beam_device_counters, summed over the stream's calls,  */
/*              and an eighth int64: the 100 MHz ticks of the stable-prefix walk.               */
/*   A stream takes at most max_frames frames in all: what a chunk holds beyond is not          */
/*   processed and sets the record's overflow field.  chunk_len 0 leaves the record as it is.   */
/*   decoded (N, max_frames) padded with -1, decoded_len, log_score (N): the CURRENT best       */
/*   hypothesis; stable_len (N): how many of its labels are final -- the labels on the path     */
/*   from the root to the deepest common ancestor of all beam entries (merged as decoded is),   */
/*   a prefix of every later hypothesis of the stream that never shrinks.                       */
/* The size functions return 0 for bad arguments and where max_frames * beam_width * (C - 1)    */
/* does not fit the int32 node ids.  ASR_ERR_INVALID, before any device call: a null pointer,   */
/* Tq < 1 or > max_frames, C > 64, beam_width outside 1 .. 1024, a buffer that is too small.    */
size_t asr_ctc_beam_stream_state_bytes(int N, int C, int beam_width, int lm);
size_t asr_ctc_beam_stream_workspace_bytes(int max_frames, int N, int C, int beam_width, int lm);
int asr_ctc_beam_stream(const float* logits, const int* chunk_len, int Tq, int N, int n_pad,
                        int C, int beam_width, int merge_repeated, int max_frames, void* state,
                        size_t state_bytes, void* workspace, size_t ws_bytes, int* decoded,
                        int* decoded_len, int* stable_len, float* log_score,
                        asr_stream_t stream);
int asr_ctc_beam_lm_stream(const float* logits, const int* chunk_len, int Tq, int N, int n_pad,
                           int C, int beam_width, int merge_repeated, const float* w, int order,
                           int max_frames, void* state, size_t state_bytes, void* workspace,
                           size_t ws_bytes, int* decoded, int* decoded_len, int* stable_len,
                           float* log_score, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K23 SpecAugment (arXiv 1904.08779; csrc/specaug.hip) of an input slab     */
/* `in` (T, n_pad, ld) time-major with F <= ld real columns into `out` (the  */
/* same shape, ANOTHER buffer): per utterance n < N a piecewise-linear time  */
/* warp, mF frequency masks and mT time masks, drawn from the K12 streams.   */
/* len = lens[n] clamped to 0 .. T (lens NULL: T).  rand(w, K) = the high    */
/* 32 bits of w * K, an integer in [0, K).  Sample n owns the B = 1 +        */
/* ceil((mF + mT) / 2) Philox blocks from n * B on (counter and key as K12): */
/* block 0 = the warp (word 0 the centre, word 1 the displacement); mask m   */
/* (frequency masks first, then time masks) = block 1 + m / 2, word 2 (m %   */
/* 2) its width and word 2 (m % 2) + 1 its start.                            */
/*   warp : Wn = min(W, (len - 1) / 2); none if Wn = 0; else                 */
/*          c = Wn + rand(w0, len - 2 Wn), c' = c + rand(w1, 2 Wn + 1) - Wn; */
/*          output frame t < c' reads source position t c / c', frame c' <=  */
/*          t < len reads c + (t - c') (len - c) / (len - c'); a position    */
/*          base + num / den is i = base + num div den (64-bit integers),    */
/*          frac = (float)(num mod den) / (float)den, and                    */
/*          y = x[i] + frac (x[min(i + 1, len - 1)] - x[i])                  */
/*   freq : f = rand(., min(Fw, F) + 1), f0 = rand(., F - f + 1): columns    */
/*          f0 <= col < f0 + f of every frame t < len become mask_value      */
/*   time : cap = min(Tw > 0 ? Tw : len, (int)floorf(p * (float)len), len),  */
/*          tau = rand(., cap + 1), t0 = rand(., len - tau + 1): frames t0   */
/*          <= t < t0 + tau become mask_value (columns < F)                  */
/* The warp comes first, then the masks; a masked element is a SELECT (a     */
/* non-finite input under a mask comes out as exactly mask_value).  Frames   */
/* t >= len, rows n >= N and columns col >= F are copied bit for bit.        */
/* params_out (device int32, N x (2 + 2 (mF + mT)), or NULL) receives per    */
/* sample (c, c', f_0, f0_0, ..., tau_0, t0_0, ...); c = c' = -1: no warp.   */
/* One launch, no workspace, no atomics, no workgroup waits on another.      */
/* ASR_ERR_INVALID before any device call: a NULL or aliased slab, ld < F, a */
/* negative count or width, N > n_pad, p outside [0, 1], mF + mT > 64,       */
/* misalignment (in / out: 16 bytes where ld % 4 == 0, else 4).              */
/* ------------------------------------------------------------------------ */
int asr_specaug_apply(const float* in, float* out, const int* lens, int T, int N, int n_pad,
                      int F, int ld, int W, int mF, int Fw, int mT, int Tw, float p,
                      float mask_value, uint64_t seed, uint32_t stream_id, uint32_t step,
                      int* params_out, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K31 RNN-Transducer (Graves, arXiv 1211.3711; csrc/rnnt.hip; no reference  */
/* counterpart).  U1 = l_max + 1 label positions, position 0 = start of the  */
/* sequence; blank = C - 1.  enc (T, n_pad, Jp), pred (U1, n_pad, Jp), Jp =  */
/* J rounded up to 4, time-major float32; W_out (J, C) row-major, b_out (C). */
/*   z(n,t,u,:) = tanh(enc(t,n,:) + pred(u,n,:)) W_out + b_out               */
/*   lp = log_softmax(z);  alpha(0,0) = 0;  alpha(t,u) = logsumexp(          */
/*     alpha(t-1,u) + lp_blank(t-1,u), alpha(t,u-1) + lp_{y_u}(t,u-1))       */
/*   loss[n] = -(alpha(T_n-1,U_n) + lp_blank(T_n-1,U_n)), natural log, T_n = */
/*   seq_len[n] clamped to 1 .. T, U_n = label_len[n] clamped to 0 .. l_max. */
/* d_enc / d_pred (the shapes of enc / pred), dW_out, db_out = grad_scale *  */
/* d sum_n loss_n / d(.), WRITTEN (not accumulated); d_enc is 0 at frames    */
/* t >= T_n, d_pred at positions u > U_n, both in rows n >= N and in columns */
/* >= J.  The four gradient pointers are all NULL (loss only) or all set.    */
/* Rows n >= N of enc / pred are never read.  No float atomics: the same     */
/* bits on every run.  The workspace needs no initialisation; it holds four  */
/* floats per lattice cell and 256 partial (J + 1, 16 / 32 / 64) slabs of    */
/* dW_out / db_out, never a (t, u, j) or (t, u, c) tensor.  alpha / beta are */
/* re-centred on their anti-diagonal's maximum every 4 diagonals, the        */
/* removed amount summed in float64.  ASR_ERR_INVALID before any device      */
/* call: a NULL pointer, T outside 1 .. 1000000, J outside 1 .. 512, C       */
/* outside 2 .. 64, l_max                                                    */
/* outside 0 .. 255, U1 != l_max + 1, n_pad % 16 != 0 or < N (the size       */
/* function returns 0 for those).                                            */
/* ------------------------------------------------------------------------ */
size_t asr_rnnt_workspace_bytes(int T, int U1, int N, int n_pad, int J, int C);
int asr_rnnt_loss_grad(const float* enc, const float* pred, const float* W_out,
                       const float* b_out, const int* labels, const int* label_len,
                       const int* seq_len, int T, int U1, int N, int n_pad, int J, int C,
                       int l_max, float grad_scale, float* loss, float* d_enc, float* d_pred,
                       float* dW_out, float* db_out, void* workspace, size_t ws_bytes,
                       asr_stream_t stream);
/* One iteration of frame-synchronous greedy decoding for all utterances.    */
/* Row n is active while t_ptr[n] < seq_len[n] (clamped to 0 .. T).  An      */
/* active row evaluates the joint cell (enc(t_ptr[n], n, :), g_cur(n, :))    */
/* and takes the first-max arg-max k.  k a label and n_sym[n] < max_symbols: */
/* decoded[n, decoded_len[n]++] = k (dropped past cap), n_sym[n]++,          */
/* advance[n] = 1, x_next(n, :) = e_k.  Otherwise (blank, or max_symbols     */
/* labels already emitted in this frame): t_ptr[n]++, n_sym[n] = 0,          */
/* advance[n] = 0.  x_next (n < N, ld_next >= C - 1 columns) is 0 elsewhere; */
/* an ended row gets advance 0 and nothing else.  *active = the rows still   */
/* active AFTER this call.  t_ptr, n_sym, decoded_len: device int32 (N),     */
/* zeroed by the caller before the first call.                               */
int asr_rnnt_greedy_step(const float* enc, const float* g_cur, const float* W_out,
                         const float* b_out, const int* seq_len, int T, int N, int n_pad,
                         int J, int C, int max_symbols, int cap, int ld_next, int* t_ptr,
                         int* n_sym, int* decoded, int* decoded_len, int* advance,
                         float* x_next, int* active, asr_stream_t stream);
/* The predictor's input slab out (U1, n_pad, ld): row (u, n) = the unit     */
/* vector of label y_u = labels[n, u - 1] for 1 <= u <= label_len[n], n < N, */
/* within `width` columns; all other rows (u = 0, padding) and columns 0.    */
int asr_onehot_rows(const int* labels, const int* label_len, int U1, int N, int n_pad,
                    int l_max, int width, int ld, float* out, asr_stream_t stream);
/* out[n, :] = mask[n] != 0 (n < N) ? a[n, :] : b[n, :] over (n_pad, width); */
/* out may be a or b.                                                        */
int asr_rows_select(const int* mask, const float* a, const float* b, float* out, int N,
                    int n_pad, int width, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K32 attention encoder-decoder (no reference counterpart): the cross-      */
/* attention core (csrc/cross_attention.hip) and the decoder's fused joint + */
/* softmax cross-entropy (csrc/aed.hip).                                     */
/*                                                                           */
/* CROSS-ATTENTION: K21 with the queries and the keys in two slabs of two    */
/* lengths.  q (Tq, n_pad, ld_q >= D) holds Q in its first D = heads * dh    */
/* columns, kv (Tk, n_pad, ld_kv >= 2D) holds [K | V]; head h in columns     */
/* h dh .. of each block.  For n < N, head h, query row t < q_lens[n]:       */
/*   s[t,u] = scale q_t . k_u  for u < k_lens[n],  p = softmax_u(s),         */
/*   out_t = sum_u p[t,u] v_u,  lse_t = log sum_u exp s[t,u];                */
/* masked keys carry probability exactly 0 and get dK = dV = exactly 0.  A   */
/* query row t >= q_lens[n] has out = lse = exactly 0 and adds exactly 0 to  */
/* every gradient (K25's rule for a row with no visible key); its dQ is 0.   */
/* Rows n >= N of out, lse, dq, dkv and the pad columns (>= D of out and dq, */
/* >= 2D of dkv) are written as exact zeros.  The kernels are the passes of  */
/* K21 (csrc/attn_core.h, CROSS = true): the same arithmetic in the same     */
/* order, so with Tq = Tk, q_lens = NULL and q, kv the column blocks of one  */
/* qkv slab the results equal asr_attn_fwd / asr_attn_bwd bit for bit.       */
/* Exact fp32 FMAs, base-2 exponentials, no float atomics, no workgroup      */
/* waits on another.  dh a multiple of 16 in 16 .. 128, any Tq, Tk >= 1 (Tq  */
/* = 1: the decode step), 1 <= N <= n_pad <= 65535, ld_* multiples of 4,     */
/* 16-byte aligned slabs; anything else is ASR_ERR_INVALID before any device */
/* call (the size function returns 0).                                       */
/* ------------------------------------------------------------------------ */
typedef struct asr_attn_cross_args {
  int Tq, Tk, N, n_pad, heads, dh;
  int ld_q, ld_kv, ld_out;   /* floats per row of q / dq, of kv / dkv, of out / dout          */
  float scale;               /* of the scores, usually 1 / sqrt(dh)                          */
  const float* q;            /* (Tq, n_pad, ld_q)                                            */
  const float* kv;           /* (Tk, n_pad, ld_kv)                                           */
  const int* q_lens;         /* optional device int32 (N): valid query rows, clamped to      */
                             /*   0 .. Tq                                                    */
  const int* k_lens;         /* optional device int32 (N): valid keys, clamped to 1 .. Tk    */
  float* out;                /* (Tq, n_pad, ld_out): forward writes it, backward reads it    */
  float* lse;                /* (Tq, n_pad, heads): forward writes it when not NULL,         */
                             /*   backward reads it                                          */
  const float* dout;         /* backward: (Tq, n_pad, ld_out)                                */
  float* dq;                 /* backward: (Tq, n_pad, ld_q)                                  */
  float* dkv;                /* backward: (Tk, n_pad, ld_kv), dK | dV                        */
} asr_attn_cross_args;
/* Workspace of asr_attn_cross_bwd (D of every query row); 0 for a refused geometry.         */
size_t asr_attn_cross_workspace_bytes(const asr_attn_cross_args* a);
int asr_attn_cross_fwd(const asr_attn_cross_args* a, asr_stream_t stream);
int asr_attn_cross_bwd(const asr_attn_cross_args* a, void* workspace, size_t ws_bytes,
                       asr_stream_t stream);
/* THE DECODER'S JOINT + CROSS-ENTROPY.  ctx, q (U1, n_pad, J) time-major    */
/* float32 (the attention context and the predictor's query projection), J a */
/* multiple of 4; W_out (J, C) row-major, b_out (C); U1 = l_max + 1 label    */
/* positions, U_n = label_len[n] clamped to 0 .. l_max.  Per row (u, n),     */
/* n < N, 0 <= u <= U_n:                                                     */
/*   h = tanh(ctx + q),  z = h W_out + b_out,  lp = log_softmax(z),          */
/*   target = labels[n, u] for u < U_n (a value outside 0 .. C - 2 counts as */
/*   C - 1), EOS = C - 1 for u = U_n (the class the CTC models give blank),  */
/*   loss[n] = sum_u -((1 - eps) lp[target] + eps mean_c lp[c]),  eps in     */
/*   [0, 1) the label smoothing; natural log; rows added in ascending u.     */
/* d_ctx, d_q (both WRITTEN with the same values: d loss / d(ctx + q)),      */
/* dW_out, db_out = grad_scale * d sum_n loss_n / d(.); rows u > U_n and     */
/* rows n >= N of d_ctx / d_q are exact zeros.  The four gradient pointers   */
/* are all NULL (loss only) or all set.  dW_out / db_out: every workgroup    */
/* sums its rows in a fixed order into a partial (J + 1, 16 / 32 / 64) slab, */
/* the slabs are added in index order; no float atomics, the same bits on    */
/* every run.  The workspace needs no initialisation.  ASR_ERR_INVALID       */
/* before any device call: a NULL pointer, J outside 4 .. 512 or no multiple */
/* of 4, C outside 2 .. 64, l_max outside 0 .. 255, U1 != l_max + 1, n_pad   */
/* % 16 != 0 or < N, eps outside [0, 1) (the size function returns 0).       */
size_t asr_aed_workspace_bytes(int U1, int N, int n_pad, int J, int C);
int asr_aed_loss_grad(const float* ctx, const float* q, const float* W_out, const float* b_out,
                      const int* labels, const int* label_len, int U1, int N, int n_pad, int J,
                      int C, int l_max, float eps, float grad_scale, float* loss, float* d_ctx,
                      float* d_q, float* dW_out, float* db_out, void* workspace, size_t ws_bytes,
                      asr_stream_t stream);
/* One iteration of label-synchronous greedy decoding for all utterances,    */
/* one wave per utterance.  A row with finished[n] != 0 gets advance[n] = 0  */
/* and nothing else.  Any other row evaluates the joint of ctx(n, :) and     */
/* q(n, :) (both (n_pad, J)) and takes the first-max arg-max k.  k = EOS     */
/* (C - 1), or decoded_len[n] >= max_labels: finished[n] = 1, advance[n] =   */
/* 0.  Otherwise decoded[n, decoded_len[n]++] = k (dropped past cap),        */
/* advance[n] = 1, x_next(n, :) = e_k, and the row counts as active unless   */
/* it has just reached max_labels (then finished[n] = 1).  x_next (n < N,    */
/* ld_next >= C - 1 columns) is 0 elsewhere.  *active = the rows still       */
/* active AFTER this call.  finished, decoded_len: device int32 (N), zeroed  */
/* by the caller before the first call.                                      */
int asr_aed_greedy_step(const float* ctx, const float* q, const float* W_out,
                        const float* b_out, int N, int n_pad, int J, int C, int max_labels,
                        int cap, int ld_next, int* finished, int* decoded, int* decoded_len,
                        int* advance, float* x_next, int* active, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K33 time reduction by frame stacking (csrc/timestack.hip; no reference    */
/* counterpart): k consecutive frames of a time-major slab become one frame  */
/* of k times the width (the pyramid of arXiv 1508.01211, the time-reduction */
/* layer of RNN-T encoders, the stacked input frames of LSTM-CTC), and the   */
/* exact adjoint.  x (T, n_pad, ld_in), y (To, n_pad, ld_out), To = ceil(T / */
/* k); len_n = lens[n] (device int32, N) clamped to 0 .. T for n < N, T for  */
/* n >= N or lens NULL:                                                      */
/*   y[to, n, j F + f] = x[to k + j, n, f]  for j < k, f < F where           */
/*                       to k + j < len_n, else 0; 0 in k F <= c < ld_out    */
/*   dx[t, n, f] = dy[t / k, n, (t % k) F + f]  for f < F where t < len_n,   */
/*                 else 0; 0 in F <= c < ld_in                               */
/* The mask is a select: no frame >= len_n and no column >= F of x (>= k F   */
/* of dy) is read.  Every element of y / dx is written exactly once: no      */
/* atomics, no workspace, bit-identical repeats.  k in 2 .. 8, F >= 1 (F a   */
/* multiple of 4: 16-byte loads; else scalar loads), ld_in >= F, ld_out >=   */
/* k F, both multiples of 4, n_pad a multiple of 16, 1 <= N <= n_pad,        */
/* 16-byte aligned pointers that do not alias; anything else is              */
/* ASR_ERR_INVALID before any device call.                                   */
/* ------------------------------------------------------------------------ */
int asr_time_stack_fwd(const float* x, const int* lens, float* y, int T, int N, int n_pad,
                       int F, int ld_in, int ld_out, int k, asr_stream_t stream);
int asr_time_stack_bwd(const float* dy, const int* lens, float* dx, int T, int N, int n_pad,
                       int F, int ld_in, int ld_out, int k, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K7  CTC loss + gradient.  Replaces core/ctc_utils.py:60-70 ->             */
/* tf.nn.ctc_loss (blank = C-1, internal softmax, ctc_merge_repeated=True).  */
/* logits/grad: (T, n_pad, C) time-major.  labels (N, l_max) int32 padded,   */
/* label_len/seq_len (N) int32, all on the device.  loss[n] = -log p(l|x);   */
/* grad = grad_scale * d loss_n / d logits, 0 for t >= seq_len[n] and for    */
/* padding rows n >= N.  An infeasible target yields loss = +inf, grad = 0   */
/* (the host raises the TF error before launching).  grad may be NULL (loss  */
/* only) and must NOT alias logits (the gradient kernel re-reads the logits  */
/* of neighbouring frames while other waves write grad): ASR_ERR_INVALID.    */
/* ------------------------------------------------------------------------ */
size_t asr_ctc_workspace_bytes(int T, int N, int n_pad, int C, int l_max);
int asr_ctc_loss_grad(const float* logits, const int* labels,
                      const int* label_len, const int* seq_len, int T, int N,
                      int n_pad, int C, int l_max, float grad_scale,
                      float* loss, float* grad, void* workspace,
                      size_t ws_bytes, asr_stream_t stream);

/* K8  Greedy decode.  Replaces core/ctc_utils.py:42 ->                      */
/* tf.nn.ctc_greedy_decoder (first-max argmax, merge repeats, drop blank).   */
/* decoded (N, T) int32 padded with -1; decoded_len (N).                     */
int asr_ctc_greedy(const float* logits, const int* seq_len, int T, int N,
                   int n_pad, int C, int* decoded, int* decoded_len,
                   asr_stream_t stream);

/* K9  Beam search (host side of the library; logits already on the host).   */
/* Replaces core/ctc_utils.py:48-50 -> tf.nn.ctc_beam_search_decoder         */
/* (top_paths=1, merge_repeated as given).  logits (T, n_pad, C) HOST float. */
int asr_ctc_beam_search_host(const float* logits_host, const int* seq_len_host,
                             int T, int N, int n_pad, int C, int beam_width,
                             int merge_repeated, int* decoded, int* decoded_len,
                             float* log_score);

/* K9  Beam search on the device (same algorithm, arithmetic and tie-breaking as the host    */
/* form; logits (T, n_pad, C) and seq_len are DEVICE pointers, as asr_ctc_greedy takes them;  */
/* decoded (N, T) int32 padded with -1, decoded_len (N), log_score (N) or NULL: device).     */
/* One workgroup per utterance; C <= 64, beam_width <= 1024.  The workspace holds the prefix  */
/* tree (its size is the hard bound T * beam_width child blocks per utterance; no init).      */
size_t asr_ctc_beam_device_workspace_bytes(int T, int N, int C, int beam_width);
int asr_ctc_beam_device(const float* logits, const int* seq_len, int T, int N, int n_pad, int C,
                        int beam_width, int merge_repeated, int* decoded, int* decoded_len,
                        float* log_score, void* workspace, size_t ws_bytes, asr_stream_t stream);

/* Work counters of one utterance of the LAST asr_ctc_beam_device call on this workspace     */
/* (synchronises the stream): out7 = 100 MHz ticks in the four phases of a frame (branch      */
/* update, ranking, turns, hand-over), expanding turns, insertions, child blocks allocated.   */
int asr_ctc_beam_device_counters(const void* workspace, int T, int N, int C, int beam_width,
                                 int utterance, long long* out7, asr_stream_t stream);

/* K9  Beam search with a character language model.  w is the FUSED float32 table            */
/* alpha * log P(label | context) + beta of shape (n_ctx, C - 1), n_ctx = C^(order - 1), order  */
/* 1 .. 5, n_ctx * (C - 1) <= INT_MAX; the context index is the last order - 1 labels read as   */
/* base-C digits, oldest first, the digit C - 1 standing for "before the sentence".  w[ctx of   */
/* the parent prefix][label] is added where TensorFlow's decoder calls its scorer: when a       */
/* branch's label path is fed from its parent and when a child is first offered.  Everything    */
/* else (candidate tests, eviction, tie-breaking, the emitted score, merge_repeated) is the     */
/* plain decoder's; an all-zero table gives its results bit for bit.  Host form: every pointer  */
/* is a HOST pointer; device form: every pointer is a DEVICE pointer, same limits as            */
/* asr_ctc_beam_device, its own workspace size and counters.                                    */
int asr_ctc_beam_lm_host(const float* logits_host, const int* seq_len_host, int T, int N,
                         int n_pad, int C, int beam_width, int merge_repeated,
                         const float* w_host, int order, int* decoded, int* decoded_len,
                         float* log_score);
size_t asr_ctc_beam_lm_device_workspace_bytes(int T, int N, int C, int beam_width);
int asr_ctc_beam_lm_device(const float* logits, const int* seq_len, int T, int N, int n_pad,
                           int C, int beam_width, int merge_repeated, const float* w, int order,
                           int* decoded, int* decoded_len, float* log_score, void* workspace,
                           size_t ws_bytes, asr_stream_t stream);
int asr_ctc_beam_lm_device_counters(const void* workspace, int T, int N, int C, int beam_width,
                                    int utterance, long long* out7, asr_stream_t stream);

/* K19 CTC forced alignment: the most probable alignment of a KNOWN transcript (Viterbi over   */
/* the CTC lattice of 2 L + 1 states: even s a blank, odd s label (s - 1) / 2; moves 0, 1, and  */
/* 2 onto a label that differs from the previous one; end state 2 L or 2 L - 1).  Arguments as  */
/* asr_ctc_loss_grad (blank = C - 1, seq_len clamped to [1, T], l_max <= 511).  path (N, T)     */
/* int32: the lattice state of every frame t < seq_len[n], -1 beyond it and on the whole row    */
/* when no alignment exists; score (N): natural-log probability of that path, -inf when none.  */
/* Ties: the smaller move wins (stay, then 1, then 2), and state 2 L ends the path when it is   */
/* at least as good as 2 L - 1.  The workspace need not be initialised.  The host form takes    */
/* HOST pointers throughout and computes in float32, one utterance per host thread.            */
size_t asr_ctc_align_workspace_bytes(int T, int N, int n_pad, int C, int l_max);
int asr_ctc_align(const float* logits, const int* labels, const int* label_len,
                  const int* seq_len, int T, int N, int n_pad, int C, int l_max, int* path,
                  float* score, void* workspace, size_t ws_bytes, asr_stream_t stream);
int asr_ctc_align_host(const float* logits_host, const int* labels, const int* label_len,
                       const int* seq_len, int T, int N, int n_pad, int C, int l_max,
                       int* path, float* score);

/* K10 Edit distance (host).  Replaces core/metrics.py:8 -> tf.edit_distance */
/* (normalize=True).  Ragged inputs as (N, max) padded + lengths.            */
int asr_edit_distance_host(const int* hyp, const int* hyp_len, int hyp_ld,
                           const int* truth, const int* truth_len, int truth_ld,
                           int N, float* out_normalized);

/* ------------------------------------------------------------------------ */
/* K11 Optimiser.  Replaces Keras Adam/SGD with clipnorm (train.py:133-137)  */
/* and the l2 regularisers (core/models.py:263-264,279).  params/grads/m/v   */
/* are flat float32 buffers of n elements; segments (n_seg x {int64 offset,  */
/* int64 len, float l2, float pad}) give the per-tensor l2 coefficient.      */
/* Step 1 writes norm_out[0] = ||g + 2*l2*p||_2 and norm_out[1] = sum l2*p^2 */
/* (both float64, device).  Step 2 applies the update using norm_out[0]      */
/* without a host round trip.                                                */
/* ------------------------------------------------------------------------ */
typedef struct asr_segment {
  int64_t offset;
  int64_t len;
  float l2;
  float reserved;
} asr_segment;
size_t asr_optim_workspace_bytes(int64_t n);
int asr_grad_norm(const float* params, const float* grads, int64_t n,
                  const asr_segment* segments_dev, int n_seg, double* norm_out,
                  void* workspace, size_t ws_bytes, asr_stream_t stream);
int asr_adam_step(float* params, const float* grads, float* m, float* v,
                  int64_t n, const asr_segment* segments_dev, int n_seg,
                  const double* norm_dev, float clipnorm, float lr, float beta1,
                  float beta2, float eps, int step, asr_stream_t stream);
int asr_sgd_step(float* params, const float* grads, float* vel, int64_t n,
                 const asr_segment* segments_dev, int n_seg,
                 const double* norm_dev, float clipnorm, float lr,
                 float momentum, asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K5-LN  Layer-normalised LSTM cell (layer_norm option of the reference's    */
/* override: core/layers.py:407-436, 460-462; core/layers_utils.py:16-19):    */
/* LN over the 4H row of h_prev@U, of x@W, and over the H row of the cell     */
/* state that feeds the output (the carried c stays un-normalised); combines  */
/* with multiplicative integration and zoneout.  Generic path: one workgroup  */
/* per (sample, direction) row and step (see csrc/lstm_ln.hip), several times */
/* slower than the persistent kernels.  cellp (2, 34H) per direction: alpha,  */
/* beta1, beta2, b (4H each; alpha/beta ignored unless has_mi), gain/bias of  */
/* LN(h@U) and of LN(x@W) (4H each), gain/bias of LN(c) (H each).  wx = x@W   */
/* WITHOUT bias.  Backward writes duh / dwx = d/d(raw h@U) / d/d(raw x@W) and */
/* dparams (n_pad, 2, 34H): per-row sums of the cellp gradients (sum axis 0). */
/* ------------------------------------------------------------------------ */
typedef struct asr_lstm_ln_args {
  int T, n_pad, H;       /* n_pad % 16 == 0, H % 4 == 0, H <= 512              */
  int has_mi;
  const float* U;        /* (2, H, 4H)                                         */
  const float* mask_u;   /* (2, n_pad, H) or NULL                              */
  const float* cellp;    /* (2, 34H)                                           */
  const float* zone_c;   /* (T, 2, H) or NULL                                  */
  const float* zone_h;
  const float* wx;       /* (T, n_pad, 2, 4H)                                  */
  float* uh;             /* (T, n_pad, 2, 4H) raw h_prev@U: fwd out, bwd in     */
  float* y;              /* (T, n_pad, 2H)                                     */
  float* cell;           /* (T, n_pad, 2, H)                                   */
  float* gates;          /* (T, n_pad, 2, 4H)                                  */
  const float* dy;       /* backward: (T, n_pad, 2H)                           */
  float* duh;            /* backward out                                       */
  float* dwx;            /* backward out                                       */
  float* dparams;        /* backward out                                       */
  int activation;        /* as asr_lstm_args.activation (0 = tanh)             */
} asr_lstm_ln_args;
size_t asr_lstm_ln_workspace_bytes(const asr_lstm_ln_args* a);
int asr_lstm_ln_seq_fwd(const asr_lstm_ln_args* a, asr_stream_t stream);
int asr_lstm_ln_seq_bwd(const asr_lstm_ln_args* a, void* workspace, size_t ws_bytes,
                        asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* C1  Gradient all-reduce (RCCL over xGMI).                                   */
/* One communicator per process / GPU: rank 0 calls asr_comm_unique_id and     */
/* ships the ASR_COMM_ID_BYTES to the other ranks by any side channel; every   */
/* rank then calls asr_comm_init with the HIP device already selected.         */
/* asr_comm_allreduce_sum sums n floats over the ranks in place, enqueued on    */
/* the given stream.  librccl is resolved with dlopen at first use.  This IS    */
/* the collective path of the shipped Python host (parallel.CapiComm: gradient  */
/* all-reduce, parameter broadcast, metric sums); torch.distributed only ships  */
/* the id bytes.                                                                */
/* ------------------------------------------------------------------------ */
#define ASR_COMM_ID_BYTES 128
typedef void* asr_comm_t;
int asr_comm_unique_id(void* id_out);
int asr_comm_init(const void* id, int rank, int world, asr_comm_t* comm_out);
int asr_comm_allreduce_sum(asr_comm_t comm, float* buf, int64_t n, asr_stream_t stream);
int asr_comm_destroy(asr_comm_t comm);

/* out[i] = a * x[i] + b * y[i] (out may alias x or y).  The residual connection of    */
/* brsmv1(residual=...): keras merge([new_o, o], mode='sum' | 'ave'),                 */
/* core/models.py:273-276, and its gradient accumulation.                            */
int asr_axpby(int64_t n, float a, const float* x, float b, const float* y, float* out,
              asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* Operation-level entry points: one per role on the training path, expressed */
/* on the general entry points above (csrc/roles.cpp; no further kernels).    */
/* ------------------------------------------------------------------------ */
/* K1-K3 by feature class: preprocessing/audio.py:309-367 (MFCC; cfg->kind    */
/* must be 0) and :394-442 (LogFbank; cfg->kind must be 1, no DCT table).     */
/* Arguments as asr_frontend_features.                                        */
int asr_frontend_mfcc_batch(const asr_frontend_cfg* cfg, const float* audio,
                            const int* offsets, const int* lengths,
                            const int* host_lengths, int n_utt, int n_pad,
                            const double* window, const double* mel,
                            const int* mel_range, const double* dct, float* out,
                            int t_out, int* out_frames, void* workspace,
                            size_t ws_bytes, asr_stream_t stream);
int asr_frontend_logfbank_batch(const asr_frontend_cfg* cfg, const float* audio,
                                const int* offsets, const int* lengths,
                                const int* host_lengths, int n_utt, int n_pad,
                                const double* window, const double* mel,
                                const int* mel_range, float* out, int t_out,
                                int* out_frames, void* workspace, size_t ws_bytes,
                                asr_stream_t stream);

/* K4/K6 the three GEMMs of one LSTM layer's input projection                 */
/* (core/layers.py:439, K.dot(x * B_W[0], self.W), hoisted out of the time    */
/* loop) over `rows` slab rows (whole frames of n_pad samples when a mask is  */
/* given; mask row = slab row % n_pad):                                       */
/*   fwd  : zx = (x (.) B_W) @ W + bias                                       */
/*   dgrad: dx = dx_beta * dx + (dz @ W^T) (.) B_W                            */
/*   wgrad: dW = (x (.) B_W)^T @ dz ;  db = column sums of dz (if db != NULL) */
/* gate_dim is the number of gate columns this call covers (4H for one        */
/* direction -- each direction of a Bidirectional layer has its own B_W --    */
/* or 8H for both when mask_w is NULL); ldw / ldz are the row strides of W /  */
/* dW and of zx / dz (8H in the engine's fused two-direction layout).         */
typedef struct asr_gate_gemm_args {
  int rows, n_pad, in_dim, gate_dim;
  const float* x;  int ldx;   /* (rows, in_dim)                               */
  const float* W;  int ldw;   /* (in_dim, gate_dim)                           */
  const float* bias;          /* (gate_dim) or NULL (fwd)                     */
  const float* mask_w;        /* (n_pad, in_dim) variational mask or NULL     */
  float* zx;       int ldz;   /* fwd out (rows, gate_dim)                     */
  const float* dz;            /* dgrad / wgrad in, row stride ldz             */
  const float* dz_absmax;     /* device max|dz| (split-fp16 pre-scale) / NULL */
  float* dx;                  /* dgrad out (rows, in_dim), row stride ldx     */
  float dx_beta;              /* 0, or 1 to add the second direction's term   */
  float* dW;                  /* wgrad out (in_dim, gate_dim), row stride ldw */
  float* db;                  /* wgrad out (gate_dim) or NULL                 */
  int split_k;                /* wgrad: split the long `rows` reduction       */
  int precision;              /* as asr_gemm_args.precision (-1 = default)    */
} asr_gate_gemm_args;
/* role: 0 = fwd, 1 = dgrad, 2 = wgrad. */
size_t asr_gemm_gate_workspace_bytes(const asr_gate_gemm_args* g, int role);
int asr_gemm_gate_fwd(const asr_gate_gemm_args* g, void* workspace, size_t ws_bytes,
                      asr_stream_t stream);
int asr_gemm_gate_dgrad(const asr_gate_gemm_args* g, void* workspace, size_t ws_bytes,
                        asr_stream_t stream);
int asr_gemm_gate_wgrad(const asr_gate_gemm_args* g, void* workspace, size_t ws_bytes,
                        asr_stream_t stream);

/* ------------------------------------------------------------------------ */
/* K12 counter-based random numbers for the training-time noise of the path:  */
/* replaces the TF random ops behind GaussianNoise (core/models.py:250-251),  */
/* the input Dropout (:257-258), the variational dropout masks B_W / B_U      */
/* (:265-266; one mask per batch, inverted scaling) and the zoneout keep      */
/* masks (core/layers_utils.py:34-42).  Philox-4x32-10; key = seed, counter = */
/* (block, stream_id, step, block >> 32); element 4b+j = word j of block b.   */
/* Stateless: (seed, stream_id, step) fully determine the tensor.             */
/*   asr_dropout_masks : out[i] = u_i >= p ? scale : 0, u = (word >> 8) 2^-24 */
/*   asr_dropout_apply : out = in * that mask (mask_out receives it, or NULL) */
/*   asr_gaussian_noise: out = in + sigma * N(0,1) (Box-Muller; in may be     */
/*                       NULL = pure noise, or equal to out)                  */
/*   asr_random_words  : the raw 32-bit words (tests)                         */
/*   asr_mul           : out = x * y elementwise (mask applied to a gradient) */
/* All pointers 16-byte aligned device memory.                                */
/* ------------------------------------------------------------------------ */
int asr_dropout_masks(float* out, int64_t n, float p, float scale, uint64_t seed,
                      uint32_t stream_id, uint32_t step, asr_stream_t stream);
int asr_dropout_apply(const float* in, float* out, float* mask_out, int64_t n, float p,
                      float scale, uint64_t seed, uint32_t stream_id, uint32_t step,
                      asr_stream_t stream);
int asr_gaussian_noise(const float* in, float* out, int64_t n, float sigma, uint64_t seed,
                       uint32_t stream_id, uint32_t step, asr_stream_t stream);
int asr_random_words(unsigned* out, int64_t n, uint64_t seed, uint32_t stream_id, uint32_t step,
                     asr_stream_t stream);
int asr_mul(int64_t n, const float* x, const float* y, float* out, asr_stream_t stream);

/* A stream whose kernels run only on the compute units set in `mask` (bit i of word i/32 =  */
/* CU i; hipExtStreamCreateWithCUMask): partitions the chip between the latency-bound        */
/* recurrences and the GEMMs that run beside them.  Destroy with asr_stream_destroy.         */
int asr_stream_create_cu_mask(const uint32_t* mask, int words, asr_stream_t* stream_out);
int asr_stream_destroy(asr_stream_t stream);

/* K9 / K10 under their operation names (same arguments as the *_host forms).  */
int asr_ctc_beam(const float* logits_host, const int* seq_len_host, int T, int N,
                 int n_pad, int C, int beam_width, int merge_repeated, int* decoded,
                 int* decoded_len, float* log_score);
int asr_edit_distance(const int* hyp, const int* hyp_len, int hyp_ld,
                      const int* truth, const int* truth_len, int truth_ld, int N,
                      float* out_normalized);

/* Device-side veto of the NEXT update (no host round trip): if *flag_a or *flag_b (device    */
/* ints, either may be NULL) is non-zero -- e.g. the sticky timeout words at the head of the   */
/* recurrent kernels' workspaces -- norm_dev[0] becomes -1 and asr_adam_step / asr_sgd_step     */
/* given that norm return without touching parameters or state.  Enqueue it between            */
/* asr_grad_norm and the step; the host sees the flag at its next (lagged) check, switches to   */
/* the stepwise recurrent kernels (mode 1) and goes on with intact weights.                     */
int asr_optim_guard(double* norm_dev, const int* flag_a, const int* flag_b, asr_stream_t stream);
/* Data parallel, the veto has to be collective (a rank that skips an update the others apply   */
/* diverges): out2[0] / out2[1] <- 1.0f where *flag_a / *flag_b is set, else 0.0f.  The host     */
/* keeps out2 directly behind the flat gradient buffer, so the gradient all-reduce (C1, a sum)  */
/* carries the flags of every rank to every rank, and then passes out2, out2 + 1 to              */
/* asr_optim_guard (which tests for any non-zero bit pattern).                                   */
int asr_timeout_flags(const int* flag_a, const int* flag_b, float* out2, asr_stream_t stream);
/* Test / diagnosis only: occupies `blocks` workgroups of 256 threads with lds_bytes of LDS     */
/* each for `seconds` (<= 5) of wall clock on `stream` -- the stand-in for a foreign kernel (an  */
/* RCCL collective) that takes compute units while a persistent recurrence needs them all.       */
int asr_debug_occupy(int blocks, int lds_bytes, double seconds, asr_stream_t stream);

/* K11 one call per optimiser step: global gradient norm (written to norm_out  */
/* as asr_grad_norm does) followed by the clipped Adam / SGD update, both      */
/* enqueued on `stream`; workspace from asr_optim_workspace_bytes(n).          */
int asr_clip_adam_step(float* params, const float* grads, float* m, float* v,
                       int64_t n, const asr_segment* segments_dev, int n_seg,
                       double* norm_out, float clipnorm, float lr, float beta1,
                       float beta2, float eps, int step, void* workspace,
                       size_t ws_bytes, asr_stream_t stream);
int asr_clip_sgd_step(float* params, const float* grads, float* vel, int64_t n,
                      const asr_segment* segments_dev, int n_seg, double* norm_out,
                      float clipnorm, float lr, float momentum, void* workspace,
                      size_t ws_bytes, asr_stream_t stream);

/* C1 asr_comm_allreduce_sum under the name the scope table uses.             */
int asr_comm_allreduce(asr_comm_t comm, float* buf, int64_t n, asr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ASR_HIP_H */
