// Helpers shared by the norm-table kernels (ds_normtab.hip, ds_groupnorm.hip): the fp64 recombination of a producer's tile
// statistics and the activation exponent of a table (layout and rationale: ds_normtab.hip).
#pragma once
#include "ds_common.h"

namespace ds_nt {

__device__ __forceinline__ double group_sum_d(double v, int width) {
  for (int o = width >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void acc_tile(const float4 v, double& s, double& q) {
  const double K = v.x, S = v.y, Q = v.z, n = v.w;
  s += n * K + S;
  q += Q + 2.0 * K * S + n * K * K;
}

// 2^-k for a bound U on the activation's argument: U * 2^k in [2^13, 2^14); |k| <= 80 keeps 2^-(wshift + k) a normal float for
// every weight shift (|wshift| <= 40)
__device__ __forceinline__ float inv_scale_of(float U) {
  const unsigned bits = __builtin_bit_cast(unsigned, U);
  const int e = (int)((bits >> 23) & 0xffu);
  int k = (e == 0 || e == 255) ? 0 : 140 - e;
  k = k > 80 ? 80 : (k < -80 ? -80 : k);
  return __builtin_bit_cast(float, (unsigned)(127 - k) << 23);
}

}  // namespace ds_nt
