// Device helpers shared by the streaming (one read, one write) kernels and by every epilogue that reports a maximum: the 16-byte
// float vector, SiLU, the full-wave butterflies, and the two commits of a per-sample maximum into an "amax" slot
// (include/diffsci_hip.h: int32 slots holding float bits, zeroed or merged into).  The pieces of the fp16x3 arithmetic are in
// ds_h3_common.h.  A kernel file defines no helper another file could use: it goes here or there, and the file says `using`.
#pragma once
#include <hip/hip_runtime.h>

namespace ds {

typedef float f32x4 __attribute__((ext_vector_type(4)));   // native vector: HIP's float4 struct defeats SROA in the MFMA kernels

__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }

__device__ __forceinline__ float amax4(f32x4 v) {
  return fmaxf(fmaxf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)), fmaxf(__builtin_fabsf(v.z), __builtin_fabsf(v.w)));
}

// Full-wave butterflies: all 64 lanes call, every lane gets the result.  (Narrower groups: ds_nt::group_sum_d.)
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Merge a wave's maximum m (>= 0 in every lane's view; all 64 lanes call) into *slot: non-negative floats order like their bits,
// and fmaxf drops NaNs.  Two forms.  `always` issues one atomicMax per wave: the conv / attention epilogues, ds_amax, ds_tokens,
// ds_groupnorm and ds_resample.  `if_greater` skips the atomic when the slot already covers the wave's maximum: a slot only grows,
// and atomics on one address serialise in L2 (measured at ~0.3 us each: 4.8 ms for the 16 384 waves per sample of a
// [32, 64, 128, 128] launch), while the agent-scope load in front is an ordinary L2 read, and a stale smaller value only costs a
// redundant atomic.  Among n waves a new maximum is seen about ln n times, so nearly every wave skips: ds_convit.
// The two compile to different code.  Moving a kernel from one form to the other is a performance change to be measured on its
// own, not a tidying: until then each kernel keeps the form it was written and timed with.
__device__ __forceinline__ void wave_commit_max_always(unsigned* slot, float m) {
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) atomicMax(slot, __builtin_bit_cast(unsigned, m));
}
__device__ __forceinline__ void wave_commit_max_if_greater(unsigned* slot, float m) {
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) {
    const unsigned bits = __builtin_bit_cast(unsigned, m);
    if (bits > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, bits);
  }
}

}  // namespace ds
