// Device and launch helpers shared by the stepper kernels (ds_step.hip) and the stochastic-interpolant inpainting step
// (ds_inpaint.hip): the drift / score arithmetic in the reference's operation order, the counter-based noise stream, the
// non-finite check of the range guard, and the grid / vector-width decisions of a streaming launch.  Every translation unit that
// includes this gets its own copy (anonymous namespace); compile with -ffp-contract=off.
#pragma once
#include "ds_common.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float score_of(float x, float f, float fu, bool has_u, const ds_eval_coef& k) {
  float F = f;
  if (has_u) F = k.one_minus_guidance * fu + k.guidance * f;
  float so = k.c_out * F;
  float D = so + k.c_skip * x;
  return (D - x) / k.sigma_sq;
}

__device__ __forceinline__ float drift(float x, float f, float fu, bool has_u, const ds_eval_coef& k) {
  if (k.input_kind == DS_IN_DRIFT) return f;
  if (k.input_kind == DS_IN_FLOW) {              // f is a flow field v(x, t) (flowfield.py:441-458)
    float F = f;
    if (has_u) F = k.one_minus_guidance * fu + k.guidance * f;
    return k.neg_mult * (F / k.sigma_sq);
  }
  if (k.scaled) {                                // non-constant scaling (VP), schedulers.py:275-293
    const float xs = x / k.scale;                // score_fn(x / s, sigma)
    const float score = (k.input_kind == DS_IN_SCORE) ? f : score_of(xs, f, fu, has_u, k);
    float d = k.scale_mult * x + k.neg_mult * score;          // scale_multiplier*x - multiplier*score
    if (k.stochastic) d = d + k.neg_lang * score;             // -(langevin * 1/s * score)
    return d;
  }
  float score = (k.input_kind == DS_IN_SCORE) ? f : score_of(x, f, fu, has_u, k);
  float d = k.neg_mult * score;
  if (k.stochastic) d = d + k.neg_lang * score;
  return d;
}

// the next evaluation's network input: c_in * x, or c_in * (x / s) under a non-constant scaling
__device__ __forceinline__ float next_input(float r, float c_in_next, float next_scale) {
  return (next_scale == 1.0f || next_scale == 0.0f) ? c_in_next * r : c_in_next * (r / next_scale);   // 0: a zero-initialised struct
}

// the range guard's result check folded into the run's last step (nets/precision.py): inf / NaN in what this lane wrote raises
// the word; one atomic per wave that saw any, none on a finite run
__device__ __forceinline__ bool not_finite(float v) { return !(__builtin_fabsf(v) <= 3.402823466e+38f); }
__device__ __forceinline__ void raise_nonfinite(unsigned* word, bool bad) {
  if (word == nullptr) return;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(bad);                 // called outside the loops: all lanes arrive
  if (m != 0ull && (int)(threadIdx.x & 63) == __builtin_ctzll(m)) atomicOr(word, 1u);
}

inline int grid_for(size_t n4) {
  size_t g = (n4 + kThreads - 1) / kThreads;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

// ---- counter-based noise: Philox4x32-10 + Box-Muller (the in-kernel eps of SURVEY 8a6 / 8b) ----------------
// eps for element e of step j comes from counter  state[1] + offset_j + e/4  under key state[0]; its four 32-bit
// outputs give the four normals of elements 4*(e/4) .. 4*(e/4)+3.  Nothing depends on the launch geometry, so
// a replay with the same (seed, offset) reproduces the draw bit for bit and the launch is graph-capturable:
// (seed, base offset) live in device memory, the per-step offset is a by-value argument.
// oracle/philox_ref.py restates this stream in numpy.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}

__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = (float)a * 2.3283064365386963e-10f + 1.1641532182693481e-10f;   // (0, 1]
  const float u2 = (float)b * 2.3283064365386963e-10f;                               // [0, 1]
  const float rad = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * u2, &sn, &cs);
  z0 = rad * cs;
  z1 = rad * sn;
}

__device__ __forceinline__ float4 philox_normal4_at(unsigned long long seed, unsigned long long ctr) {
  const uint4 r = philox4x32_10(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u),
                                make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  float4 z;
  box_muller(r.x, r.y, z.x, z.y);
  box_muller(r.z, r.w, z.z, z.w);
  return z;
}

__device__ __forceinline__ float4 philox_normal4(const unsigned long long* __restrict__ state, unsigned long long offset,
                                                 size_t i4) {
  return philox_normal4_at(state[0], state[1] + offset + (unsigned long long)i4);
}

__device__ __forceinline__ float philox_normal1(const unsigned long long* __restrict__ state, unsigned long long offset,
                                                size_t e) {
  const float4 z = philox_normal4(state, offset, e >> 2);
  const int j = (int)(e & 3);
  return j == 0 ? z.x : j == 1 ? z.y : j == 2 ? z.z : z.w;
}

inline bool blends(int input_kind) { return input_kind == DS_IN_NETWORK || input_kind == DS_IN_FLOW; }

// float4 iterations of a launch: n/4 when every (non-NULL) pointer is 16-byte aligned, else 0 -- the kernels'
// scalar grid-stride tail then covers everything (odd-sized states: history[i] / eps[i] slices of [B,2] toys with
// odd B, per-sample views x[b] of 3x3 fields, ...; the reference accepts any shape).
inline size_t vec4_count(size_t n, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs)
    if (p && (reinterpret_cast<uintptr_t>(p) & 15u)) return 0;
  return n / 4;
}
inline int grid_elems(size_t n4, size_t n) { return grid_for(n4 ? n4 : (n + 3) / 4); }

}  // namespace
