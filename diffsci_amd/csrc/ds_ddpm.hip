// The discrete DDPM / DDIM step (diffsci/models/ddpm/v2/integrators.py): one HBM-bound pass over the state, 12 bytes per
// element (read x, read F, write x'); the network input of the next evaluation is the state itself, so nothing else is written.
//
// Arithmetic is written in the reference's own operation order (one rounding per op, no FMA contraction: the file is compiled
// with -ffp-contract=off); each step's scalars are one fp32 value apiece, computed on the host with the reference's tensor
// operations, so that given the same F and the same draw every result is bit-identical to the reference's torch fp32 path:
//   classical    r = c1*(x - c0*f) + c2*e                               integrators.py:98,105
//   generalized  x0 = (x - f*c0)/c1;  r = (c2*x0 + c3*f) + c4*e         integrators.py:203-209
//   forward      r = c0*x + c1*e                                        integrators.py:120-121, 222-224
// Without noise the last term is dropped: it is +-0 in the reference (sigma = 0 times a finite draw) and leaves the sum's value.
// Layout: flat fp32; 16 B per lane per access (float4), grid-stride, the grid of ds_stepmath.h.
#include "ds_common.h"
#include "ds_stepmath.h"

namespace {

template <int FORM, bool HAS_EPS>
__device__ __forceinline__ float ddpm_one(float x, float f, float e, const ds_ddpm_coef& k) {
  float r;
  if (FORM == DS_DDPM_CLASSICAL) {
    const float d = x - k.c0 * f;
    r = k.c1 * d;
    if (HAS_EPS) r = r + k.c2 * e;
  } else if (FORM == DS_DDPM_GENERALIZED) {
    const float x0 = (x - f * k.c0) / k.c1;
    r = k.c2 * x0 + k.c3 * f;
    if (HAS_EPS) r = r + k.c4 * e;
  } else {
    r = k.c0 * x;
    if (HAS_EPS) r = r + k.c1 * e;
  }
  return r;
}

template <int FORM, int NOISE>          // NOISE: 0 none, 1 injected eps, 2 in-kernel Philox
__global__ __launch_bounds__(kThreads) void k_ddpm_step(float* x_out, const float* x, const float* __restrict__ f,
                                                        const float* __restrict__ eps, const unsigned long long* rng,
                                                        unsigned long long rng_offset, ds_ddpm_coef k, size_t n4, size_t n) {
  constexpr bool HAS_EPS = NOISE != 0;
  constexpr bool HAS_F = FORM != DS_DDPM_FORWARD;
  size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  size_t stride = (size_t)gridDim.x * kThreads;
  bool bad = false;
  for (; i < n4; i += stride) {
    float4 vx = reinterpret_cast<const float4*>(x)[i];
    float4 vf = make_float4(0, 0, 0, 0), ve = make_float4(0, 0, 0, 0);
    if (HAS_F) vf = reinterpret_cast<const float4*>(f)[i];
    if (NOISE == 1) ve = reinterpret_cast<const float4*>(eps)[i];
    if (NOISE == 2) ve = philox_normal4(rng, rng_offset, i);
    float4 o;
    o.x = ddpm_one<FORM, HAS_EPS>(vx.x, vf.x, ve.x, k);
    o.y = ddpm_one<FORM, HAS_EPS>(vx.y, vf.y, ve.y, k);
    o.z = ddpm_one<FORM, HAS_EPS>(vx.z, vf.z, ve.z, k);
    o.w = ddpm_one<FORM, HAS_EPS>(vx.w, vf.w, ve.w, k);
    bad = bad || not_finite(o.x) || not_finite(o.y) || not_finite(o.z) || not_finite(o.w);
    reinterpret_cast<float4*>(x_out)[i] = o;
  }
  // tail (n not a multiple of 4), or everything when a pointer is not 16-byte aligned (n4 = 0)
  for (size_t t = n4 * 4 + (size_t)blockIdx.x * kThreads + threadIdx.x; t < n; t += stride) {
    const float e = NOISE == 1 ? eps[t] : NOISE == 2 ? philox_normal1(rng, rng_offset, t) : 0.f;
    const float o = ddpm_one<FORM, HAS_EPS>(x[t], HAS_F ? f[t] : 0.f, e, k);
    bad = bad || not_finite(o);
    x_out[t] = o;
  }
  raise_nonfinite(k.nonfinite, bad);
}

}  // namespace

extern "C" {

int ds_ddpm_step(float* x_out, const float* x, const float* f, const ds_ddpm_coef* k, const float* eps,
                 const uint64_t* philox_state, uint64_t philox_offset, size_t n, void* stream, int flags) {
  const int form = flags & DS_DDPM_FORM_MASK, noise = flags & DS_DDPM_NOISE_MASK;
  DS_REQUIRE((flags & ~(DS_DDPM_FORM_MASK | DS_DDPM_NOISE_MASK)) == 0 && form <= DS_DDPM_FORWARD &&
                 (noise == 0 || noise == DS_DDPM_NOISE_EPS || noise == DS_DDPM_NOISE_PHILOX),
             DS_ERR_SHAPE, "ds_ddpm_step: undefined flags 0x%x", flags);
  DS_REQUIRE(x_out && x && k, DS_ERR_NULL, "ds_ddpm_step: NULL pointer");
  DS_REQUIRE(f || form == DS_DDPM_FORWARD, DS_ERR_NULL, "ds_ddpm_step: the backward forms read the network output f");
  DS_REQUIRE((noise == DS_DDPM_NOISE_EPS) == (eps != nullptr), DS_ERR_NULL, "ds_ddpm_step: eps goes with DS_DDPM_NOISE_EPS");
  DS_REQUIRE((noise == DS_DDPM_NOISE_PHILOX) == (philox_state != nullptr), DS_ERR_NULL,
             "ds_ddpm_step: philox_state goes with DS_DDPM_NOISE_PHILOX");
  DS_REQUIRE((reinterpret_cast<uintptr_t>(philox_state) & 7u) == 0, DS_ERR_SHAPE, "ds_ddpm_step: state must be 8-byte aligned");
  if (n == 0) return DS_OK;
  if (form == DS_DDPM_FORWARD) f = nullptr;
  const size_t n4 = vec4_count(n, {x_out, x, f, eps});
  dim3 g(grid_elems(n4, n)), b(kThreads);
  hipStream_t s = ds::as_stream(stream);
  const unsigned long long* rng = reinterpret_cast<const unsigned long long*>(philox_state);
  const unsigned long long off = (unsigned long long)philox_offset;
#define L(F, E) hipLaunchKernelGGL((k_ddpm_step<F, E>), g, b, 0, s, x_out, x, f, eps, rng, off, *k, n4, n)
#define LN(F) do { if (noise == DS_DDPM_NOISE_EPS) L(F, 1); else if (noise == DS_DDPM_NOISE_PHILOX) L(F, 2); else L(F, 0); } while (0)
  if (form == DS_DDPM_CLASSICAL) LN(DS_DDPM_CLASSICAL);
  else if (form == DS_DDPM_GENERALIZED) LN(DS_DDPM_GENERALIZED);
  else LN(DS_DDPM_FORWARD);
#undef LN
#undef L
  DS_CHECK_LAUNCH("ds_ddpm_step");
  return DS_OK;
}

}  // extern "C"
