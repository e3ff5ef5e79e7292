// joint_common.h -- what the two label-synchronous joints share: the transducer's (K31, rnnt.hip)
// and the attention decoder's (K32, aed.hip).  Both compute tanh(a + b) W_out + b_out over C <= 64
// classes padded to 16 / 32 / 64, and both leave dW_out / db_out as per-workgroup partial slabs
// (J + 1, CP) -- rows 0 .. J - 1 = dW_out, row J = db_out -- which ONE kernel adds in index order.
#pragma once
#include "common.h"

namespace {

constexpr float kNegInf = -__builtin_huge_valf();

// tanh to a few ulp of 1 (absolute): what the joint needs of it, h and 1 - h^2 are O(1) factors
__device__ __forceinline__ float joint_tanh(float x) {
  x = fminf(fmaxf(x, -15.f), 15.f);
  return 1.f - __fdividef(2.f, __expf(2.f * x) + 1.f);
}

inline int class_pad(int C) { return C <= 16 ? 16 : (C <= 32 ? 32 : 64); }

__device__ __forceinline__ int label_at(const int* __restrict__ labels, int n, int l_max, int u,
                                        int C) {
  const int y = labels[(size_t)n * l_max + u];
  return (y < 0 || y >= C) ? C - 1 : y;
}

// dW_out (J, C) and db_out (C): the slabs added in index order
__global__ void __launch_bounds__(256)
joint_slab_sum_kernel(const float* __restrict__ slabs, int nslabs, int J, int C, int CP,
                      float* __restrict__ dW, float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (J + 1) * C) return;
  const int j = i / C, c = i % C;
  float s = 0.f;
  for (int g = 0; g < nslabs; ++g) s += slabs[((size_t)g * (J + 1) + j) * CP + c];
  if (j < J) dW[(size_t)j * C + c] = s;
  else db[c] = s;
}

}  // namespace
