// Resampling by any integer factor f, the route of ADM blocks with image_sample_factor != 2 (make_downsample / make_upsample,
// adm.py:361-383: AvgPool{2,3}d(kernel_size=f), Upsample(scale_factor=f, mode='nearest')).  Factor 2 keeps its fused loaders
// and parity kernels; these run as standalone passes between the norm and a plain convolution.
//   ds_avgpool3d_f  volumes [planes, D, H, W] -> [planes, D/f, H/f, W/f] (floor), sum in torch's (z, y, x) order, / f^3.
//                   (Fields pool inside ds_gnorm1_apply_poolf, kind 2 for the raw residual input.)
//   ds_upsample_f   fields and volumes, out[.., z, y, x] = x[.., z/f, y/f, x/f].  A store-bound copy: each thread writes
//                   16 bytes along W when W*f allows, reading its (at most 4) sources from the row just read by its
//                   neighbours (L1 / L2 hits), so every source element leaves HBM once per output row.
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

}  // namespace

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
