// Resampling by any integer factor f, the route of ADM blocks with image_sample_factor != 2 (make_downsample / make_upsample,
// adm.py:361-383: AvgPool{2,3}d(kernel_size=f), Upsample(scale_factor=f, mode='nearest')).  Factor 2 keeps its fused loaders
// and parity kernels; these run as standalone passes between the norm and a plain convolution.
//   ds_avgpool3d_f  volumes [planes, D, H, W] -> [planes, D/f, H/f, W/f] (floor), sum in torch's (z, y, x) order, / f^3.
//                   (Fields pool inside ds_gnorm1_apply_poolf, kind 2 for the raw residual input.)
//   ds_maxpool_f    fields and volumes [planes, (D,) H, W] -> floor(/ f), the max of each window in torch's (z, y, x) order with
//                   its NaN rule (v > m || isnan(v), from -inf): the route of PUNetG's DownSampler with transition_scale_factor
//                   != 2 (MaxPool{2,3}d(f), commonlayers.py:25-81).  Bit-identical to F.max_pool{2,3}d.
//   ds_upsample_f   fields and volumes, out[.., z, y, x] = x[.., z/f, y/f, x/f].  A store-bound copy: each thread writes
//                   16 bytes along W when W*f allows, reading its (at most 4) sources from the row just read by its
//                   neighbours (L1 / L2 hits), so every source element leaves HBM once per output row.
//   ds_cornerpool_f fields and volumes, out[b, c, o] = x[b or 0, c, o * f] (+ te[b or 0, c]): CornerPool{2,3}d(f) of a field-valued
//                   conditional embedding with the time embedding added on the way (PUNetG's per-voxel time shifts), and the
//                   per-sample max |out| for the fp16x3 1x1 convolution that reads it.  The same store-bound shape as
//                   ds_upsample_f with the gather on the read side: for f >= 2 a thread's four sources are f floats apart.
#include "ds_common.h"

namespace {

constexpr int NT = 256;
constexpr size_t MAX_BLOCKS = 2048;          // memory-bound: about 8 blocks per CU, grid-stride the rest

// one thread per output voxel; VLOAD: f and W multiples of 4, x 16-byte aligned (each window row is f/4 float4 loads)
template <bool VLOAD>
__global__ __launch_bounds__(NT) void k_avgpool3d_f(float* __restrict__ out, const float* __restrict__ x, int Di, int Hi, int Wi,
                                                    unsigned Do, unsigned Ho, unsigned Wo, int f, unsigned total) {
  const float div = (float)(f * f * f);
  for (unsigned i = blockIdx.x * NT + threadIdx.x; i < total; i += gridDim.x * NT) {     // 32-bit indices: the host checks total
    const unsigned xo = i % Wo, t0 = i / Wo;
    const unsigned yo = t0 % Ho, t = t0 / Ho;
    const unsigned zo = t % Do;
    const size_t plane = t / Do;
    const float* p = x + ((plane * Di + (size_t)zo * f) * Hi + (size_t)yo * f) * Wi + (size_t)xo * f;
    float s = 0.f;
    for (int dz = 0; dz < f; ++dz) {
      for (int dy = 0; dy < f; ++dy) {
        const float* r = p + ((size_t)dz * Hi + dy) * Wi;
        if (VLOAD) {
          for (int dx = 0; dx < f; dx += 4) {
            const float4 v = *reinterpret_cast<const float4*>(r + dx);
            s = s + v.x; s = s + v.y; s = s + v.z; s = s + v.w;
          }
        } else {
          for (int dx = 0; dx < f; ++dx) s = s + r[dx];
        }
      }
    }
    out[i] = s / div;
  }
}

// VEC output floats per thread along W (4: Wo % 4 == 0 and out 16-byte aligned).  Index arithmetic in 32 bits: the host
// checks that the number of VEC-wide units fits.  fd: the depth factor (f for volumes, 1 for fields, whose depth axis is a batch).
template <int VEC>
__global__ __launch_bounds__(NT) void k_upsample_f(float* __restrict__ out, const float* __restrict__ x, int Di, int Hi, int Wi,
                                                   unsigned Do, unsigned Ho, unsigned wq, unsigned f, unsigned fd, unsigned total) {
  for (unsigned i = blockIdx.x * NT + threadIdx.x; i < total; i += gridDim.x * NT) {
    const unsigned xq = i % wq, row = i / wq;
    const unsigned yo = row % Ho, t = row / Ho;
    const unsigned zo = t % Do, plane = t / Do;
    const float* src = x + (((size_t)plane * Di + zo / fd) * Hi + yo / f) * Wi;
    unsigned xs = (VEC * xq) / f, r = VEC * xq - xs * f;
    if (VEC == 4) {
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = src[xs];
        if (++r == f) { r = 0; ++xs; }
      }
      *reinterpret_cast<float4*>(out + (size_t)i * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      out[i] = src[xs];
    }
  }
}

// max of v into m with torch's NaN rule (a NaN replaces anything; nothing replaces a NaN)
__device__ __forceinline__ void max_into(float& m, float v) {
  if (v > m || isnan(v)) m = v;
}

// VEC output floats per thread along W (4: Wo % 4 == 0 and out 16-byte aligned), consecutive lanes on consecutive outputs, so a
// wave's window rows are one contiguous span of 64 * VEC * f floats.  F: the factor at compile time (2, 3, 4) or 0 (read from f):
// with F known every row span of a thread (VEC * F floats) is loaded before any of it is compared, so a thread keeps all of them in
// flight instead of one load per loop trip.  VLOAD: the row span is whole float4s (VEC * f and Wi multiples of 4, x 16-byte
// aligned).  fd: the depth factor (f for volumes, 1 for fields).  32-bit indices: the host checks total.
template <int F, int VEC, bool VLOAD>
__global__ __launch_bounds__(NT) void k_maxpool_f(float* __restrict__ out, const float* __restrict__ x, int Di, int Hi, int Wi,
                                                  unsigned Do, unsigned Ho, unsigned wq, int f_rt, int fd, unsigned total) {
  const int f = F > 0 ? F : f_rt;
  for (unsigned i = blockIdx.x * NT + threadIdx.x; i < total; i += gridDim.x * NT) {
    const unsigned xq = i % wq, row = i / wq;
    const unsigned yo = row % Ho, t = row / Ho;
    const unsigned zo = t % Do, plane = t / Do;
    const float* p = x + (((size_t)plane * Di + (size_t)zo * fd) * Hi + (size_t)yo * f) * Wi + (size_t)xq * VEC * f;
    float m[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) m[k] = -INFINITY;
    for (int dz = 0; dz < fd; ++dz) {
      if constexpr (F > 0) {
        constexpr int S = VEC * F;                       // floats per window row of this thread
        float v[F][S];
#pragma unroll
        for (int dy = 0; dy < F; ++dy) {
          const float* r = p + ((size_t)dz * Hi + dy) * Wi;
          if constexpr (VLOAD) {
#pragma unroll
            for (int q = 0; q < S / 4; ++q) {
              const float4 w = *reinterpret_cast<const float4*>(r + 4 * q);
              v[dy][4 * q] = w.x; v[dy][4 * q + 1] = w.y; v[dy][4 * q + 2] = w.z; v[dy][4 * q + 3] = w.w;
            }
          } else {
#pragma unroll
            for (int q = 0; q < S; ++q) v[dy][q] = r[q];
          }
        }
#pragma unroll
        for (int dy = 0; dy < F; ++dy)                    // each window in (y, x) order, as torch
#pragma unroll
          for (int k = 0; k < VEC; ++k)
#pragma unroll
            for (int dx = 0; dx < F; ++dx) max_into(m[k], v[dy][k * F + dx]);
      } else {
        for (int dy = 0; dy < f; ++dy) {
          const float* r = p + ((size_t)dz * Hi + dy) * Wi;
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const float* rk = r + k * f;
            if constexpr (VLOAD) {                         // here f itself is a multiple of 4
              for (int dx = 0; dx < f; dx += 4) {
                const float4 w = *reinterpret_cast<const float4*>(rk + dx);
                max_into(m[k], w.x); max_into(m[k], w.y); max_into(m[k], w.z); max_into(m[k], w.w);
              }
            } else {
              for (int dx = 0; dx < f; ++dx) max_into(m[k], rk[dx]);
            }
          }
        }
      }
    }
    if (VEC == 4)
      *reinterpret_cast<float4*>(out + (size_t)i * 4) = make_float4(m[0], m[1], m[2], m[3]);
    else
      out[i] = m[0];
  }
}

// Corner pooling with an optional per-(sample, channel) addend: out[b, c, z, y, x] = x[b or 0, c, z*fd, y*f, x*f] (+ te[b or 0, c]).
// grid (blocks per sample, B): a block stays inside one sample, so its maximum |out| goes to that sample's amax slot with one
// atomicMax per wave (the merge rule of k_absmax_rows: fmaxf drops NaNs, non-negative floats order like their bits).
// VEC output floats per thread along W (4: Wo % 4 == 0 and out 16-byte aligned); VLOAD: f == 1 with x's rows whole aligned float4s.
// xs / ts: the batch strides of x and te in floats (0: one sample shared by the batch).  `per` = C * Do * Ho * wq units per sample
// fits 32 bits (the host checks).  ADD = false is a pure copy (-0.0 stays -0.0).
template <int VEC, bool VLOAD, bool ADD>
__global__ __launch_bounds__(NT) void k_cornerpool_f(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ te,
                                                     unsigned* __restrict__ out_amax, size_t xs, size_t ts, int Di, int Hi, int Wi,
                                                     unsigned Do, unsigned Ho, unsigned wq, unsigned f, unsigned fd, unsigned per) {
  const unsigned b = blockIdx.y;
  const float* xb = x + (size_t)b * xs;
  const float* tb = ADD ? te + (size_t)b * ts : nullptr;
  float* ob = out + (size_t)b * per * VEC;
  float m = 0.f;
  for (unsigned i = blockIdx.x * NT + threadIdx.x; i < per; i += gridDim.x * NT) {
    const unsigned xq = i % wq, row = i / wq;
    const unsigned yo = row % Ho, t = row / Ho;
    const unsigned zo = t % Do, c = t / Do;
    const float* src = xb + (((size_t)c * Di + (size_t)zo * fd) * Hi + (size_t)yo * f) * Wi + (size_t)xq * VEC * f;
    const float a = ADD ? tb[c] : 0.f;
    if (VEC == 4) {
      float v[4];
      if (VLOAD) {
        const float4 w = *reinterpret_cast<const float4*>(src);
        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = src[(size_t)k * f];
      }
      if (ADD) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] + a;
      }
      *reinterpret_cast<float4*>(ob + (size_t)i * 4) = make_float4(v[0], v[1], v[2], v[3]);
      m = fmaxf(m, fmaxf(fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])), fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3]))));
    } else {
      float v = src[0];
      if (ADD) v = v + a;
      ob[i] = v;
      m = fmaxf(m, __builtin_fabsf(v));
    }
  }
  if (out_amax) {                                   // uniform: every lane of the block reaches the shuffles
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(out_amax + b, __builtin_bit_cast(unsigned, m));
  }
}

}  // namespace

extern "C" int ds_cornerpool_f(float* out, const float* x, const float* te, unsigned* out_amax, int B, int C, int Di, int Hi, int Wi,
                               int factor, int volume, int x_batch, int te_batch, void* stream) {
  DS_REQUIRE(out && x, DS_ERR_NULL, "ds_cornerpool_f: NULL pointer");
  DS_REQUIRE(B >= 0 && B < 65536 && C > 0 && Di > 0 && Hi > 0 && Wi > 0, DS_ERR_SHAPE, "ds_cornerpool_f: bad shape");
  DS_REQUIRE(factor >= 1 && (volume == 0 || volume == 1), DS_ERR_UNSUPPORTED, "ds_cornerpool_f: factor %d volume %d", factor, volume);
  DS_REQUIRE((x_batch == 1 || x_batch == B) && (!te || te_batch == 1 || te_batch == B), DS_ERR_SHAPE,
             "ds_cornerpool_f: x_batch %d / te_batch %d must be 1 or B = %d", x_batch, te_batch, B);
  const int fd = volume ? factor : 1;
  DS_REQUIRE(Di % fd == 0 && Hi % factor == 0 && Wi % factor == 0, DS_ERR_SHAPE,
             "ds_cornerpool_f: every pooled side must divide by the factor %d (D=%d H=%d W=%d volume=%d)", factor, Di, Hi, Wi, volume);
  if (B == 0) return DS_OK;
  const int Do = Di / fd, Ho = Hi / factor, Wo = Wi / factor;
  const bool vec = Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const bool vload = vec && factor == 1 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0;       // Wi == Wo: rows are whole float4s
  const size_t wq = vec ? Wo / 4 : Wo;
  const size_t per = (size_t)C * Do * Ho * wq;
  DS_REQUIRE(per < (1ull << 32) - (size_t)MAX_BLOCKS * NT, DS_ERR_SHAPE, "ds_cornerpool_f: sample too large (%zu stores)", per);
  size_t g = (per + NT - 1) / NT;
  const size_t most = MAX_BLOCKS / (size_t)B > 0 ? MAX_BLOCKS / (size_t)B : 1;
  if (g > most) g = most;
  const size_t xs = x_batch == 1 ? 0 : (size_t)C * Di * Hi * Wi;
  const size_t ts = te && te_batch != 1 ? (size_t)C : 0;
  hipStream_t s = ds::as_stream(stream);
#define DS_CORNERPOOL_LAUNCH(V, L, A)                                                                                          \
  hipLaunchKernelGGL((k_cornerpool_f<V, L, A>), dim3((unsigned)g, (unsigned)B), dim3(NT), 0, s, out, x, te, out_amax, xs, ts, \
                     Di, Hi, Wi, (unsigned)Do, (unsigned)Ho, (unsigned)wq, (unsigned)factor, (unsigned)fd, (unsigned)per)
#define DS_CORNERPOOL_ADD(A)               \
  do {                                     \
    if (vload)                             \
      DS_CORNERPOOL_LAUNCH(4, true, A);    \
    else if (vec)                          \
      DS_CORNERPOOL_LAUNCH(4, false, A);   \
    else                                   \
      DS_CORNERPOOL_LAUNCH(1, false, A);   \
  } while (0)
  if (te)
    DS_CORNERPOOL_ADD(true);
  else
    DS_CORNERPOOL_ADD(false);
#undef DS_CORNERPOOL_ADD
#undef DS_CORNERPOOL_LAUNCH
  DS_CHECK_LAUNCH("ds_cornerpool_f");
  return DS_OK;
}

extern "C" int ds_avgpool3d_f(float* out, const float* x, int planes, int Di, int Hi, int Wi, int factor, void* stream) {
  DS_REQUIRE(out && x, DS_ERR_NULL, "ds_avgpool3d_f: NULL pointer");
  DS_REQUIRE(planes >= 0 && Di > 0 && Hi > 0 && Wi > 0, DS_ERR_SHAPE, "ds_avgpool3d_f: bad shape");
  DS_REQUIRE(factor >= 1 && factor <= Di && factor <= Hi && factor <= Wi, DS_ERR_SHAPE,
             "ds_avgpool3d_f: factor %d must be in [1, min(D, H, W)] (D=%d H=%d W=%d)", factor, Di, Hi, Wi);
  const int Do = Di / factor, Ho = Hi / factor, Wo = Wi / factor;
  const size_t total = (size_t)planes * Do * Ho * Wo;
  if (total == 0) return DS_OK;
  DS_REQUIRE(total < (1ull << 32) - (size_t)MAX_BLOCKS * NT, DS_ERR_SHAPE, "ds_avgpool3d_f: output too large (%zu floats)", total);
  size_t g = (total + NT - 1) / NT;
  if (g > MAX_BLOCKS) g = MAX_BLOCKS;
  const bool vload = factor % 4 == 0 && Wi % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
  hipStream_t s = ds::as_stream(stream);
  if (vload)
    hipLaunchKernelGGL(k_avgpool3d_f<true>, dim3((unsigned)g), dim3(NT), 0, s, out, x, Di, Hi, Wi, (unsigned)Do, (unsigned)Ho,
                       (unsigned)Wo, factor, (unsigned)total);
  else
    hipLaunchKernelGGL(k_avgpool3d_f<false>, dim3((unsigned)g), dim3(NT), 0, s, out, x, Di, Hi, Wi, (unsigned)Do, (unsigned)Ho,
                       (unsigned)Wo, factor, (unsigned)total);
  DS_CHECK_LAUNCH("ds_avgpool3d_f");
  return DS_OK;
}

extern "C" int ds_upsample_f(float* out, const float* x, int planes, int Di, int Hi, int Wi, int factor, int volume,
                             void* stream) {
  DS_REQUIRE(out && x, DS_ERR_NULL, "ds_upsample_f: NULL pointer");
  DS_REQUIRE(planes >= 0 && Di > 0 && Hi > 0 && Wi > 0, DS_ERR_SHAPE, "ds_upsample_f: bad shape");
  DS_REQUIRE(factor >= 1 && (volume == 0 || volume == 1), DS_ERR_UNSUPPORTED, "ds_upsample_f: factor %d volume %d", factor, volume);
  const int fd = volume ? factor : 1;
  const size_t Do = (size_t)Di * fd, Ho = (size_t)Hi * factor, Wo = (size_t)Wi * factor;
  DS_REQUIRE(Do < (1u << 31) && Ho < (1u << 31) && Wo < (1u << 31), DS_ERR_SHAPE, "ds_upsample_f: output too large");
  if (planes == 0) return DS_OK;
  const bool vec = Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const size_t wq = vec ? Wo / 4 : Wo;
  const size_t total = (size_t)planes * Do * Ho * wq;
  DS_REQUIRE(total < (1ull << 32) - (size_t)MAX_BLOCKS * NT, DS_ERR_SHAPE, "ds_upsample_f: output too large (%zu stores)", total);
  size_t g = (total + NT - 1) / NT;
  if (g > MAX_BLOCKS) g = MAX_BLOCKS;
  hipStream_t s = ds::as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(k_upsample_f<4>, dim3((unsigned)g), dim3(NT), 0, s, out, x, Di, Hi, Wi, (unsigned)Do, (unsigned)Ho,
                       (unsigned)wq, (unsigned)factor, (unsigned)fd, (unsigned)total);
  else
    hipLaunchKernelGGL(k_upsample_f<1>, dim3((unsigned)g), dim3(NT), 0, s, out, x, Di, Hi, Wi, (unsigned)Do, (unsigned)Ho,
                       (unsigned)wq, (unsigned)factor, (unsigned)fd, (unsigned)total);
  DS_CHECK_LAUNCH("ds_upsample_f");
  return DS_OK;
}

extern "C" int ds_maxpool_f(float* out, const float* x, int planes, int Di, int Hi, int Wi, int factor, int volume, void* stream) {
  DS_REQUIRE(out && x, DS_ERR_NULL, "ds_maxpool_f: NULL pointer");
  DS_REQUIRE(planes >= 0 && Di > 0 && Hi > 0 && Wi > 0, DS_ERR_SHAPE, "ds_maxpool_f: bad shape");
  DS_REQUIRE(volume == 0 || volume == 1, DS_ERR_UNSUPPORTED, "ds_maxpool_f: volume %d", volume);
  const int fd = volume ? factor : 1;
  DS_REQUIRE(factor >= 1 && fd <= Di && factor <= Hi && factor <= Wi, DS_ERR_SHAPE,
             "ds_maxpool_f: factor %d must be in [1, the smallest pooled side] (D=%d H=%d W=%d volume=%d)", factor, Di, Hi, Wi,
             volume);
  const int Do = Di / fd, Ho = Hi / factor, Wo = Wi / factor;
  if (planes == 0) return DS_OK;
  const bool vec = Wo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
  const int fc = factor >= 2 && factor <= 4 ? factor : 0;              // the factors with a compile-time kernel
  // float4 row loads: a thread's row span (vec ? 4 : 1) * factor floats with a compile-time factor, each output's f floats otherwise
  const int unit = fc ? (vec ? 4 : 1) * fc : factor;
  const bool vload = unit % 4 == 0 && Wi % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
  const size_t wq = vec ? Wo / 4 : Wo;
  const size_t total = (size_t)planes * Do * Ho * wq;
  DS_REQUIRE(total < (1ull << 32) - (size_t)MAX_BLOCKS * NT, DS_ERR_SHAPE, "ds_maxpool_f: output too large (%zu stores)", total);
  size_t g = (total + NT - 1) / NT;
  if (g > MAX_BLOCKS) g = MAX_BLOCKS;
  hipStream_t s = ds::as_stream(stream);
#define DS_MAXPOOL_LAUNCH(F, V, L)                                                                                              \
  hipLaunchKernelGGL((k_maxpool_f<F, V, L>), dim3((unsigned)g), dim3(NT), 0, s, out, x, Di, Hi, Wi, (unsigned)Do, (unsigned)Ho, \
                     (unsigned)wq, factor, fd, (unsigned)total)
#define DS_MAXPOOL_VEC(F)                   \
  do {                                      \
    if (vec && vload)                       \
      DS_MAXPOOL_LAUNCH(F, 4, true);        \
    else if (vec)                           \
      DS_MAXPOOL_LAUNCH(F, 4, false);       \
    else if (vload)                         \
      DS_MAXPOOL_LAUNCH(F, 1, true);        \
    else                                    \
      DS_MAXPOOL_LAUNCH(F, 1, false);       \
  } while (0)
  switch (fc) {
    case 2: DS_MAXPOOL_VEC(2); break;
    case 3: DS_MAXPOOL_VEC(3); break;
    case 4: DS_MAXPOOL_VEC(4); break;
    default: DS_MAXPOOL_VEC(0); break;
  }
#undef DS_MAXPOOL_VEC
#undef DS_MAXPOOL_LAUNCH
  DS_CHECK_LAUNCH("ds_maxpool_f");
  return DS_OK;
}
