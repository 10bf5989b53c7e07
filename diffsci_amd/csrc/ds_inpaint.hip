// One inner iteration of SIModule.inpaint after the network call (reference flowfield.py:783-793, 546-641), in one pass over
// the state: the Euler-Maruyama step of the stochastic interpolant, the re-imposition of the known region, the optional
// RePaint jump back, and the scaled network input of the next evaluation.  State x [B, n]; the known data x_orig [n] (network
// space) and the mask m [n] are shared by the batch.  In the reference's operation order (one rounding per operation; the file
// is compiled with -ffp-contract=off), the arithmetic of k_drift, k_axpby, k_div_scalar and k_mask_blend back to back:
//   v     = drift(x, F[, Fu])                                              flowfield.py:441-458
//   score = (alpha*v + (-alpha')*x) / (sigma*(alpha'*sigma - alpha*sigma'))   flowfield.py:483-501
//   x1    = (x + dt*(v + (-(0.5*omega))*score)) + sqrt(omega*|dt|)*eps_a   flowfield.py:783-793       eps_a [B, n]
//   patch = alpha_n*x_orig + sigma_n*eps_b                                 flowfield.py:620-624       eps_b [n], one draw per position
//   out   = x1*(1 - m) + patch*m                                           DS_SI_BLEND
//   out   = (alpha_c*out + sigma_c*eps_c)*(1 - m) + (alpha_c*x_orig + sigma_c*eps_d)*m   DS_SI_RENOISE   eps_c [B, n], eps_d [n]
//   xin   = c_in(next evaluation) * out
// Without DS_SI_BLEND this is the plain Euler-Maruyama step of integrate_flow_field(noise_injection=True).
//
// Noise: four injected buffers, or the counter stream of ds_step.hip (ds_stepmath.h; oracle/philox_ref.py restates it).  With
// cB = ceil(B*n / 4) and c1 = ceil(n / 4) counters per draw, a launch at offset o reads, in the order the reference draws,
//   eps_a  element e of [B, n]   counter o + e/4,                  output e%4
//   eps_b  position p of [n]     counter o + cB + p/4,             output p%4      (DS_SI_BLEND)
//   eps_c  element e             counter o + cB + c1 + e/4,        output e%4      (DS_SI_RENOISE)
//   eps_d  position p            counter o + 2*cB + c1 + p/4,      output p%4      (DS_SI_RENOISE)
// so a launch consumes cB, cB + c1 or 2*(cB + c1) counters (ds_si_inpaint_counters); the caller advances o by that.
//
// Layout: flat fp32, 16 B per lane per access, grid-stride, <= 2048 workgroups.  The 16-byte path needs n % 4 == 0 -- a 4-vector
// then lies inside one sample, at position (e % n) of x_orig, the mask and the per-position draws -- and aligned pointers; any
// other launch takes the element-wise path for everything.
#include "ds_common.h"
#include "ds_stepmath.h"

namespace {

struct noise_src {
  const float* a; const float* b; const float* c; const float* d;       // injected
  const unsigned long long* rng;                                         // or the Philox state
  unsigned long long oa, ob, oc, od;
};

template <bool HAS_U, int MODE>        // MODE: 0 step only, 1 + blend, 2 + blend, jump back, blend
__device__ __forceinline__ void si_one(float x, float f, float fu, float m, float xo, float ea, float eb, float ec, float ed,
                                       const ds_eval_coef& k, const ds_si_step& s, float& out, float& xin) {
  const float v = drift(x, f, fu, HAS_U, k);
  const float num = s.score_a * v + s.score_b * x;
  const float score = num / s.score_den;
  const float d = v + s.neg_half_omega * score;
  float r = x + s.dt * d;
  r = r + s.noise_coef * ea;
  if (MODE >= 1) {
    const float patch = s.patch_alpha * xo + s.patch_sigma * eb;
    const float a = r * (1.0f - m);
    r = a + patch * m;
  }
  if (MODE == 2) {
    r = s.jump_alpha * r + s.jump_sigma * ec;
    const float patch = s.jump_alpha * xo + s.jump_sigma * ed;
    const float a = r * (1.0f - m);
    r = a + patch * m;
  }
  out = r;
  xin = next_input(r, s.c_in_next, k.next_scale);
}

template <bool HAS_U, bool PHILOX, int MODE>
__global__ __launch_bounds__(kThreads) void k_si_inpaint(float* x_out, float* xin_out, const float* x, const float* __restrict__ f,
                                                         const float* __restrict__ fu, const float* __restrict__ x_orig,
                                                         const float* __restrict__ mask, noise_src z, ds_eval_coef k, ds_si_step s,
                                                         size_t nps, size_t n4, size_t n) {
  size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * kThreads;
  const size_t nps4 = nps / 4;                                          // the 16-byte path runs only when nps % 4 == 0
  bool bad = false;
  const float4 zero = make_float4(0, 0, 0, 0);
  // the vector's place p = i mod nps4 in x_orig / mask / eps_b / eps_d: one modulo before the loop, then carried along
  size_t p = n4 ? i % nps4 : 0;
  const size_t pstep = n4 ? stride % nps4 : 0;
  for (; i < n4; i += stride, p = (p + pstep >= nps4 ? p + pstep - nps4 : p + pstep)) {
    const float4 vx = reinterpret_cast<const float4*>(x)[i];
    const float4 vf = reinterpret_cast<const float4*>(f)[i];
    float4 vu = zero, vm = zero, vo = zero, ea, eb = zero, ec = zero, ed = zero;
    if (HAS_U) vu = reinterpret_cast<const float4*>(fu)[i];
    ea = PHILOX ? philox_normal4(z.rng, z.oa, i) : reinterpret_cast<const float4*>(z.a)[i];
    if (MODE >= 1) {
      vm = reinterpret_cast<const float4*>(mask)[p];
      vo = reinterpret_cast<const float4*>(x_orig)[p];
      eb = PHILOX ? philox_normal4(z.rng, z.ob, p) : reinterpret_cast<const float4*>(z.b)[p];
    }
    if (MODE == 2) {
      ec = PHILOX ? philox_normal4(z.rng, z.oc, i) : reinterpret_cast<const float4*>(z.c)[i];
      ed = PHILOX ? philox_normal4(z.rng, z.od, p) : reinterpret_cast<const float4*>(z.d)[p];
    }
    float4 o, q;
    si_one<HAS_U, MODE>(vx.x, vf.x, vu.x, vm.x, vo.x, ea.x, eb.x, ec.x, ed.x, k, s, o.x, q.x);
    si_one<HAS_U, MODE>(vx.y, vf.y, vu.y, vm.y, vo.y, ea.y, eb.y, ec.y, ed.y, k, s, o.y, q.y);
    si_one<HAS_U, MODE>(vx.z, vf.z, vu.z, vm.z, vo.z, ea.z, eb.z, ec.z, ed.z, k, s, o.z, q.z);
    si_one<HAS_U, MODE>(vx.w, vf.w, vu.w, vm.w, vo.w, ea.w, eb.w, ec.w, ed.w, k, s, o.w, q.w);
    bad = bad || not_finite(o.x) || not_finite(o.y) || not_finite(o.z) || not_finite(o.w);
    if (x_out) reinterpret_cast<float4*>(x_out)[i] = o;
    if (xin_out) {
      reinterpret_cast<float4*>(xin_out)[i] = q;
      if (k.xin_copies == 2) reinterpret_cast<float4*>(xin_out + n)[i] = q;       // the batched-guidance evaluation reads [2B, ...]
    }
  }
  size_t t = n4 * 4 + (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t qstep = stride % nps;
  for (size_t p = t % nps; t < n; t += stride, p = (p + qstep >= nps ? p + qstep - nps : p + qstep)) {
    float m = 0.f, xo = 0.f, eb = 0.f, ec = 0.f, ed = 0.f;
    const float ea = PHILOX ? philox_normal1(z.rng, z.oa, t) : z.a[t];
    if (MODE >= 1) {
      m = mask[p];
      xo = x_orig[p];
      eb = PHILOX ? philox_normal1(z.rng, z.ob, p) : z.b[p];
    }
    if (MODE == 2) {
      ec = PHILOX ? philox_normal1(z.rng, z.oc, t) : z.c[t];
      ed = PHILOX ? philox_normal1(z.rng, z.od, p) : z.d[p];
    }
    float o, q;
    si_one<HAS_U, MODE>(x[t], f[t], HAS_U ? fu[t] : 0.f, m, xo, ea, eb, ec, ed, k, s, o, q);
    bad = bad || not_finite(o);
    if (x_out) x_out[t] = o;
    if (xin_out) {
      xin_out[t] = q;
      if (k.xin_copies == 2) xin_out[n + t] = q;
    }
  }
  raise_nonfinite(k.nonfinite, bad);
}

template <bool HAS_U, bool PHILOX>
void launch_mode(int mode, dim3 g, hipStream_t st, float* x_out, float* xin_out, const float* x, const float* f, const float* fu,
                 const float* x_orig, const float* mask, const noise_src& z, const ds_eval_coef& k, const ds_si_step& s, size_t nps,
                 size_t n4, size_t n) {
#define L(M) hipLaunchKernelGGL((k_si_inpaint<HAS_U, PHILOX, M>), g, dim3(kThreads), 0, st, x_out, xin_out, x, f, fu, x_orig, mask, z, k, s, nps, n4, n)
  if (mode == 2) L(2); else if (mode == 1) L(1); else L(0);
#undef L
}

}  // namespace

extern "C" {

uint64_t ds_si_inpaint_counters(int B, size_t n_per_sample, int flags) {
  if (B <= 0 || n_per_sample == 0) return 0;
  const uint64_t cB = ((uint64_t)B * n_per_sample + 3) / 4, c1 = ((uint64_t)n_per_sample + 3) / 4;
  return (flags & DS_SI_RENOISE) ? 2 * (cB + c1) : (flags & DS_SI_BLEND) ? cB + c1 : cB;
}

int ds_si_inpaint_step(float* x_out, float* xin_out, const float* x, const float* f, const float* fu, const ds_eval_coef* k,
                       const ds_si_step* s, const float* x_orig, const float* mask, const float* eps_step, const float* eps_patch,
                       const float* eps_jump, const float* eps_jump_patch, const uint64_t* philox_state, uint64_t philox_offset,
                       int B, size_t n_per_sample, void* stream, int flags) {
  DS_REQUIRE(x && f && k && s, DS_ERR_NULL, "ds_si_inpaint_step: NULL pointer");
  DS_REQUIRE(x_out || xin_out, DS_ERR_NULL, "ds_si_inpaint_step: no output requested");
  DS_REQUIRE((flags & ~(DS_SI_BLEND | DS_SI_RENOISE)) == 0 && !((flags & DS_SI_RENOISE) && !(flags & DS_SI_BLEND)), DS_ERR_SHAPE,
             "ds_si_inpaint_step: flags %d (DS_SI_RENOISE goes with DS_SI_BLEND)", flags);
  const int mode = (flags & DS_SI_RENOISE) ? 2 : (flags & DS_SI_BLEND) ? 1 : 0;
  DS_REQUIRE(B >= 0 && n_per_sample > 0, DS_ERR_SHAPE, "ds_si_inpaint_step: bad shape B=%d", B);
  DS_REQUIRE(mode == 0 || (x_orig && mask), DS_ERR_NULL, "ds_si_inpaint_step: the blend needs x_orig and mask");
  const bool injected = eps_step != nullptr;
  DS_REQUIRE(injected != (philox_state != nullptr), DS_ERR_NULL,
             "ds_si_inpaint_step: exactly one of eps_step (injected noise) and philox_state (in-kernel noise) must be given");
  DS_REQUIRE(!injected || ((mode < 1 || eps_patch) && (mode < 2 || (eps_jump && eps_jump_patch))), DS_ERR_NULL,
             "ds_si_inpaint_step: injected noise needs every draw of the mode (%d)", mode);
  DS_REQUIRE((reinterpret_cast<uintptr_t>(philox_state) & 7u) == 0, DS_ERR_SHAPE, "ds_si_inpaint_step: state must be 8-byte aligned");
  DS_REQUIRE(blends(k->input_kind), DS_ERR_SHAPE, "ds_si_inpaint_step: input must be a network output or a flow field");
  DS_REQUIRE(k->xin_copies >= 0 && k->xin_copies <= 2, DS_ERR_SHAPE, "ds_si_inpaint_step: xin_copies %d", k->xin_copies);
  DS_REQUIRE(s->score_den != 0.0f, DS_ERR_SHAPE, "ds_si_inpaint_step: the score's denominator is 0");
  if (B == 0) return DS_OK;
  DS_REQUIRE(n_per_sample <= SIZE_MAX / (size_t)B, DS_ERR_SHAPE, "ds_si_inpaint_step: B * n_per_sample overflows");
  const size_t n = (size_t)B * n_per_sample;
  const size_t n4 = (n_per_sample & 3) ? 0
                                       : vec4_count(n, {x_out, xin_out, x, f, fu, x_orig, mask, eps_step, eps_patch, eps_jump, eps_jump_patch});
  const unsigned long long cB = (n + 3) / 4, c1 = (n_per_sample + 3) / 4, o = (unsigned long long)philox_offset;
  noise_src z;
  z.a = eps_step; z.b = eps_patch; z.c = eps_jump; z.d = eps_jump_patch;
  z.rng = reinterpret_cast<const unsigned long long*>(philox_state);
  z.oa = o; z.ob = o + cB; z.oc = o + cB + c1; z.od = o + 2 * cB + c1;
  const dim3 g(grid_elems(n4, n));
  hipStream_t st = ds::as_stream(stream);
  if (fu) {
    if (injected) launch_mode<true, false>(mode, g, st, x_out, xin_out, x, f, fu, x_orig, mask, z, *k, *s, n_per_sample, n4, n);
    else launch_mode<true, true>(mode, g, st, x_out, xin_out, x, f, fu, x_orig, mask, z, *k, *s, n_per_sample, n4, n);
  } else {
    if (injected) launch_mode<false, false>(mode, g, st, x_out, xin_out, x, f, fu, x_orig, mask, z, *k, *s, n_per_sample, n4, n);
    else launch_mode<false, true>(mode, g, st, x_out, xin_out, x, f, fu, x_orig, mask, z, *k, *s, n_per_sample, n4, n);
  }
  DS_CHECK_LAUNCH("ds_si_inpaint_step");
  return DS_OK;
}

}  // extern "C"
