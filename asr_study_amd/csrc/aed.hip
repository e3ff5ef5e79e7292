// K32 attention encoder-decoder: the decoder's fused joint + softmax cross-entropy with all its
// gradients, and one step of label-synchronous greedy decoding -- gfx950.  The counterpart of
// rnnt.hip for a model whose decoder row (u, n) sees ONE context vector instead of every frame:
//
//   h = tanh(ctx(u,n,:) + q(u,n,:)),  z = h W_out + b_out,  lp = log_softmax(z),
//   target(u) = y_{u+1} for u < U_n, EOS = C - 1 for u = U_n,
//   loss_n = sum_{u <= U_n} -((1 - eps) lp[target] + eps mean_c lp[c]);  tests/aed_oracle.py
//   restates it.
//
// Neither h nor the logits nor their gradients are written: a row is one wave's registers and a
// few hundred bytes of LDS.
//
//   aed_rows_kernel  a workgroup is 4 waves; it takes GROUPS of 4 consecutive rows r = n U1 + u
//            (one row per wave) in a fixed stride over the grid.  Per row: h (lane j, j + 64 ..)
//            to LDS, z_c on lane c (j ascending, one fmaf each), the softmax by xor butterflies,
//            the row's loss to the workspace, dz_c to LDS, dh_j = dz W_out[j,:]^T (c ascending),
//            d_ctx = d_q = dh (1 - h^2).  A row outside the lattice (u > U_n, n >= N) writes
//            zeros.  Then all 256 threads add the group's four h (x) dz to the workgroup's
//            partial slab (J + 1, CP) IN LDS -- thread e owns entries e, e + 256, .. and adds the
//            rows in index order; row J (h = 1) is db_out.  At the end the slab goes to the
//            workspace.
//   joint_slab_sum_kernel (joint_common.h) adds the slabs in index order;
//   aed_loss_sum_kernel   adds an utterance's row losses in ascending u.
// No float atomics anywhere: every result is the same bits on every run.
#include "joint_common.h"

namespace {

constexpr int kRowsPerGroup = 4;      // waves of a workgroup = rows in flight
constexpr int kMaxSlabs = 256;        // workgroups of the rows pass = partial dW_out slabs
constexpr int kMaxJ = 512, kMaxC = 64, kMaxLabels = 255;

// z (this lane's logit, -inf on lanes >= C) from the row's h in LDS
__device__ __forceinline__ float joint_logit(const float* h, const float* __restrict__ W,
                                             const float* __restrict__ b, int J, int C,
                                             int lane) {
  if (lane >= C) return kNegInf;
  float s = 0.f;
  for (int j = 0; j < J; ++j) s = fmaf(h[j], W[(size_t)j * C + lane], s);
  return s + b[lane];
}

__global__ void __launch_bounds__(64 * kRowsPerGroup)
aed_rows_kernel(const float* __restrict__ ctx, const float* __restrict__ q,
                const float* __restrict__ W, const float* __restrict__ b,
                const int* __restrict__ labels, const int* __restrict__ label_len, int U1, int N,
                int n_pad, int J, int C, int CP, int l_max, float eps, float scale,
                float* __restrict__ row_loss, float* __restrict__ d_ctx, float* __restrict__ d_q,
                float* __restrict__ slabs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* hs = lds;                                  // [4][J + 1]: h, then the 1 of db_out
  float* dzs = hs + kRowsPerGroup * (J + 1);        // [4][CP]
  float* slab = dzs + kRowsPerGroup * CP;           // [(J + 1) CP]   (with gradients only)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool grads = d_ctx != nullptr;
  const int rows = U1 * n_pad, groups = (rows + kRowsPerGroup - 1) / kRowsPerGroup;
  const int entries = (J + 1) * CP;
  if (grads)
    for (int e = tid; e < entries; e += 256) slab[e] = 0.f;
  float* hw = hs + wave * (J + 1);
  float* dzw = dzs + wave * CP;
  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    const int r = grp * kRowsPerGroup + wave;
    const int n = r / U1, u = r - n * U1;
    int Un = 0;
    if (r < rows && n < N) {
      Un = label_len[n];
      Un = Un < 0 ? 0 : (Un > l_max ? l_max : Un);
    }
    const bool live = r < rows && n < N && u <= Un;
    const size_t off = ((size_t)u * n_pad + n) * J;
    __syncthreads();                                // (the previous group's slab pass read hs, dzs)
    for (int j = lane; j < J; j += 64) hw[j] = live ? joint_tanh(ctx[off + j] + q[off + j]) : 0.f;
    if (lane == 0) hw[J] = live ? 1.f : 0.f;
    __syncthreads();
    float dz = 0.f;
    if (live) {                                     // (wave-uniform)
      const float z = joint_logit(hw, W, b, J, C, lane);
      const float m = asr_wave_max(z);
      const float ex = __expf(z - m);               // 0 on lanes >= C
      const float sum = asr_wave_sum(ex);
      const float lp = lane < C ? z - (m + __logf(sum)) : 0.f;
      const int tgt = u < Un ? label_at(labels, n, l_max, u, C) : C - 1;
      const float lp_t = asr_wave_sum(lane == tgt ? lp : 0.f);
      const float lp_mean = asr_wave_sum(lp) / (float)C;
      if (lane == 0) row_loss[(size_t)n * U1 + u] = -((1.f - eps) * lp_t + eps * lp_mean);
      if (lane < C)
        dz = scale * (ex / sum - (lane == tgt ? 1.f - eps : 0.f) - eps / (float)C);
    } else if (lane == 0 && r < rows && n < N) {
      row_loss[(size_t)n * U1 + u] = 0.f;
    }
    if (!grads) continue;
    if (lane < CP) dzw[lane] = dz;
    __syncthreads();
    if (r < rows) {
      for (int j = lane; j < J; j += 64) {
        float dh = 0.f;
        if (live) {
          const float* wr = W + (size_t)j * C;
          for (int c = 0; c < C; ++c) dh = fmaf(dzw[c], wr[c], dh);
          const float h = hw[j];
          dh *= 1.f - h * h;
        }
        d_ctx[off + j] = dh;
        d_q[off + j] = dh;
      }
    }
    __syncthreads();
    for (int e = tid; e < entries; e += 256) {
      const int j = e / CP, c = e - j * CP;
      float s = slab[e];
#pragma unroll
      for (int w = 0; w < kRowsPerGroup; ++w) s = fmaf(hs[w * (J + 1) + j], dzs[w * CP + c], s);
      slab[e] = s;
    }
  }
  if (grads) {
    float* out = slabs + (size_t)blockIdx.x * entries;
    for (int e = tid; e < entries; e += 256) out[e] = slab[e];
  }
}

__global__ void __launch_bounds__(256)
aed_loss_sum_kernel(const float* __restrict__ row_loss, const int* __restrict__ label_len, int U1,
                    int N, int l_max, float* __restrict__ loss) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  int Un = label_len[n];
  Un = Un < 0 ? 0 : (Un > l_max ? l_max : Un);
  float s = 0.f;
  for (int u = 0; u <= Un; ++u) s += row_loss[(size_t)n * U1 + u];
  loss[n] = s;
}

// one iteration of greedy decoding: one wave per utterance
__global__ void __launch_bounds__(64)
aed_greedy_kernel(const float* __restrict__ ctx, const float* __restrict__ q,
                  const float* __restrict__ W, const float* __restrict__ b, int J, int C,
                  int max_labels, int cap, int ld_next, int* __restrict__ finished,
                  int* __restrict__ decoded, int* __restrict__ decoded_len,
                  int* __restrict__ advance, float* __restrict__ x_next,
                  int* __restrict__ active) {
  __shared__ float hsh[kMaxJ];
  const int n = blockIdx.x, lane = threadIdx.x;
  float* xr = x_next + (size_t)n * ld_next;
  for (int c = lane; c < ld_next; c += 64) xr[c] = 0.f;
  if (finished[n] != 0) {
    if (lane == 0) advance[n] = 0;
    return;
  }
  const float* f = ctx + (size_t)n * J;
  const float* g = q + (size_t)n * J;
  for (int j = lane; j < J; j += 64) hsh[j] = joint_tanh(f[j] + g[j]);
  __syncthreads();
  float z = joint_logit(hsh, W, b, J, C, lane);
  // first-max arg-max over the lanes
  int k = lane;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float zo = __shfl_xor(z, o, 64);
    const int ko = __shfl_xor(k, o, 64);
    if (zo > z || (zo == z && ko < k)) { z = zo; k = ko; }
  }
  if (lane == 0) {
    const int len = decoded_len[n];
    if (k == C - 1 || len >= max_labels) {
      finished[n] = 1;
      advance[n] = 0;
    } else {
      if (len < cap) decoded[(size_t)n * cap + len] = k;
      decoded_len[n] = len + 1 < cap ? len + 1 : cap;
      advance[n] = 1;
      if (k < ld_next) xr[k] = 1.f;
      if (len + 1 >= max_labels) finished[n] = 1;
      else atomicAdd(active, 1);
    }
  }
}

struct AedWs {
  size_t rows, slabs, total;
  int nslabs;
};
bool aed_ws(int U1, int N, int n_pad, int J, int C, AedWs* w) {
  if (U1 < 1 || U1 > kMaxLabels + 1 || N < 1 || N > 65535 || n_pad < N || n_pad % 16 != 0 ||
      J < 4 || J > kMaxJ || (J & 3) || C < 2 || C > kMaxC)
    return false;
  const int groups = (U1 * n_pad + kRowsPerGroup - 1) / kRowsPerGroup;
  w->nslabs = groups < kMaxSlabs ? groups : kMaxSlabs;
  w->rows = asr_align_up((size_t)N * U1 * sizeof(float), 256);
  w->slabs = asr_align_up((size_t)w->nslabs * (J + 1) * class_pad(C) * sizeof(float), 256);
  w->total = w->rows + w->slabs;
  return true;
}

}  // namespace

extern "C" size_t asr_aed_workspace_bytes(int U1, int N, int n_pad, int J, int C) {
  AedWs w;
  return aed_ws(U1, N, n_pad, J, C, &w) ? w.total : 0;
}

extern "C" int asr_aed_loss_grad(const float* ctx, const float* q, const float* W_out,
                                 const float* b_out, const int* labels, const int* label_len,
                                 int U1, int N, int n_pad, int J, int C, int l_max, float eps,
                                 float grad_scale, float* loss, float* d_ctx, float* d_q,
                                 float* dW_out, float* db_out, void* workspace, size_t ws_bytes,
                                 asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(ctx && q && W_out && b_out && label_len && loss, "aed_loss_grad: null pointer");
  ASR_CHECK_ARG(N >= 1 && N <= 65535 && n_pad >= N && n_pad % 16 == 0,
                "aed_loss_grad: bad shape N=%d n_pad=%d", N, n_pad);
  ASR_CHECK_ARG(J >= 4 && J <= kMaxJ && (J & 3) == 0,
                "aed_loss_grad: J=%d (a multiple of 4 in 4 .. 512)", J);
  ASR_CHECK_ARG(C >= 2 && C <= kMaxC, "aed_loss_grad: C=%d (2 .. 64)", C);
  ASR_CHECK_ARG(l_max >= 0 && l_max <= kMaxLabels && U1 == l_max + 1,
                "aed_loss_grad: l_max=%d (0 .. 255), U1=%d (l_max + 1)", l_max, U1);
  ASR_CHECK_ARG(labels || l_max == 0, "aed_loss_grad: null labels");
  ASR_CHECK_ARG(eps >= 0.f && eps < 1.f, "aed_loss_grad: eps=%g (0 <= eps < 1)", (double)eps);
  const int ng = (d_ctx != nullptr) + (d_q != nullptr) + (dW_out != nullptr) +
                 (db_out != nullptr);
  ASR_CHECK_ARG(ng == 0 || ng == 4,
                "aed_loss_grad: the four gradient pointers are all NULL (loss only) or all set");
  ASR_CHECK_ARG(!d_ctx || (d_ctx != ctx && d_ctx != q && d_q != ctx && d_q != q && d_ctx != d_q),
                "aed_loss_grad: a gradient must not alias an input or the other gradient");
  AedWs w;
  aed_ws(U1, N, n_pad, J, C, &w);
  if (!workspace || ws_bytes < w.total) {
    asr_set_error("aed_loss_grad: workspace %zu < %zu bytes", ws_bytes, w.total);
    return ASR_ERR_WORKSPACE;
  }
  ASR_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "aed_loss_grad: workspace alignment");
  float* row_loss = reinterpret_cast<float*>(workspace);
  float* slabs = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + w.rows);
  const bool grads = d_ctx != nullptr;
  const int CP = class_pad(C);
  const size_t lds = (size_t)(kRowsPerGroup * (J + 1 + CP) + (grads ? (J + 1) * CP : 0)) *
                     sizeof(float);
  // (once per instance, for the largest J and C: the call stays a sequence of stream operations)
  static bool lds_opted_in = false;
  if (!lds_opted_in) {
    const int lds_max = (int)((kRowsPerGroup * (kMaxJ + 1 + kMaxC) + (kMaxJ + 1) * kMaxC) *
                              sizeof(float));
    ASR_CHECK_HIP(hipFuncSetAttribute((const void*)aed_rows_kernel,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    lds_opted_in = true;
  }
  hipLaunchKernelGGL(aed_rows_kernel, dim3(w.nslabs), dim3(64 * kRowsPerGroup), lds, stream, ctx,
                     q, W_out, b_out, labels, label_len, U1, N, n_pad, J, C, CP, l_max, eps,
                     grad_scale, row_loss, d_ctx, d_q, slabs);
  ASR_CHECK_LAUNCH();
  hipLaunchKernelGGL(aed_loss_sum_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, row_loss,
                     label_len, U1, N, l_max, loss);
  ASR_CHECK_LAUNCH();
  if (!grads) return ASR_OK;
  hipLaunchKernelGGL(joint_slab_sum_kernel, dim3(((J + 1) * C + 255) / 256), dim3(256), 0, stream,
                     slabs, w.nslabs, J, C, CP, dW_out, db_out);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}

extern "C" int asr_aed_greedy_step(const float* ctx, const float* q, const float* W_out,
                                   const float* b_out, int N, int n_pad, int J, int C,
                                   int max_labels, int cap, int ld_next, int* finished,
                                   int* decoded, int* decoded_len, int* advance, float* x_next,
                                   int* active, asr_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  ASR_CHECK_ARG(ctx && q && W_out && b_out && finished && decoded && decoded_len && advance &&
                    x_next && active,
                "aed_greedy_step: null pointer");
  ASR_CHECK_ARG(N >= 1 && N <= 65535 && n_pad >= N && n_pad % 16 == 0,
                "aed_greedy_step: bad shape N=%d n_pad=%d", N, n_pad);
  ASR_CHECK_ARG(J >= 4 && J <= kMaxJ && (J & 3) == 0 && C >= 2 && C <= kMaxC,
                "aed_greedy_step: J=%d (a multiple of 4 in 4 .. 512), C=%d (2 .. 64)", J, C);
  ASR_CHECK_ARG(max_labels >= 1 && cap >= 1 && ld_next >= C - 1,
                "aed_greedy_step: max_labels=%d, cap=%d, ld_next=%d (>= C - 1)", max_labels, cap,
                ld_next);
  ASR_CHECK_HIP(hipMemsetAsync(active, 0, sizeof(int), stream));
  hipLaunchKernelGGL(aed_greedy_kernel, dim3(N), dim3(64), 0, stream, ctx, q, W_out, b_out, J, C,
                     max_labels, cap, ld_next, finished, decoded, decoded_len, advance, x_next,
                     active);
  ASR_CHECK_LAUNCH();
  return ASR_OK;
}
