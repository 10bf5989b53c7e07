// Device helpers shared by the streaming (one read, one write) kernels: 16-byte vectors, SiLU, and the commit of a per-sample
// maximum into an "amax" slot (include/diffsci_hip.h: int32 slots holding float bits, zeroed or merged into).
#pragma once
#include <hip/hip_runtime.h>

namespace ds {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float silu(float v) { return v / (1.0f + expf(-v)); }

__device__ __forceinline__ float amax4(f32x4 v) {
  return fmaxf(fmaxf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)), fmaxf(__builtin_fabsf(v.z), __builtin_fabsf(v.w)));
}

// Merge a wave's maximum m (>= 0 in every lane's view; all 64 lanes call) into *slot.  A slot only grows, so a wave whose maximum
// the slot already covers skips the atomic: atomics on one address serialise in L2 (measured at ~0.3 us each: 4.8 ms for the
// 16 384 waves per sample of a [32, 64, 128, 128] launch), while the agent-scope load in front is an ordinary L2 read, and a stale
// smaller value only costs a redundant atomic.  Among n waves a new maximum is seen about ln n times, so nearly every wave skips.
__device__ __forceinline__ void wave_commit_max(unsigned* slot, float m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) {
    const unsigned bits = __builtin_bit_cast(unsigned, m);                         // non-negative floats order like their bits
    if (bits > __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(slot, bits);
  }
}

}  // namespace ds
