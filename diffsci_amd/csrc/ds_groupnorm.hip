// GroupNorm(G, C) with several channels per group -- the normalisation of the LDM AutoencoderKL decoder
// (autoencoderldm2d.py:17-21: GroupNorm(32, C), eps 1e-6, affine), on fields and volumes alike: x is [B, C, N] with the N positions
// of a channel contiguous and group g = c / (C / G), so a group is one contiguous run of (C/G) * N floats.
//   ds_groupnorm_stats        (mean, rstd) per (sample, group): the per-sample reduction of ds_gnorm1_stats on the [B*G] view
//   ds_groupnorm_apply        one HBM pass (8 B/elt): (x - mean[b,g]) * rstd[b,g] * w[c] + b[c], then SiLU when act = 1
//   ds_groupnorm_stats_tiles  the same pairs without a pass over x, from the tile statistics its producing convolution left
//   ds_groupnorm_table        the consuming convolution's loader table (M, A, C, 2^-k) (ds_normtab.hip), from tile statistics or
//                             from plain (mean, rstd) pairs: the normalised tensor is never written to or read from HBM
// Sums are fp64 in a fixed order (thread-strided terms, a butterfly over the wave, the waves through LDS in index order):
// results are reproducible bit for bit.  Arithmetic is one rounding per operation (-ffp-contract=off).
#include "ds_normtab_common.h"
#include "ds_stream.h"

namespace {

using ds::amax4;
using ds::f32x4;
using ds::silu;
using ds::wave_max;
using ds_nt::acc_tile;
using ds_nt::group_sum_d;
using ds_nt::inv_scale_of;
constexpr int NT = 256;
constexpr int MAX_CHUNKS = 64;       // workgroups per channel row: the rest of a plane is grid-strided
constexpr int TT = 1024;             // table kernel: one workgroup per sample
constexpr int MAXG = 1024;

template <int ACT>
__device__ __forceinline__ float apply1(float x, float mean, float rstd, float w, float b) {
  const float v = (x - mean) * rstd * w + b;
  return ACT ? silu(v) : v;
}

// grid (position chunks, C, B): a workgroup serves one channel row, so the group's (mean, rstd) and the channel's affine pair
// are wave-uniform loads and no index is divided per element; one thread = VEC (4 or 1) consecutive positions per iteration
template <int VEC, int ACT>
__global__ __launch_bounds__(NT) void k_gn_apply(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ stats,
                                                 const float* __restrict__ w, const float* __restrict__ bias, int G, int cpg,
                                                 unsigned nv, size_t plane, unsigned* __restrict__ out_amax) {
  __shared__ float red[NT / 64];
  const int c = blockIdx.y, b = blockIdx.z, C = gridDim.y;
  const size_t row = ((size_t)b * C + c) * plane;
  const float* src = x + row;
  float* dst = out + row;
  const float* st = stats + ((size_t)b * G + c / cpg) * 2;
  const float mean = st[0], rstd = st[1];
  const float wc = w ? w[c] : 1.f, bc = bias ? bias[c] : 0.f;
  float m = 0.f;
  for (unsigned i = blockIdx.x * NT + threadIdx.x; i < nv; i += gridDim.x * NT) {
    if constexpr (VEC == 4) {
      f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)i * 4);
      v.x = apply1<ACT>(v.x, mean, rstd, wc, bc); v.y = apply1<ACT>(v.y, mean, rstd, wc, bc);
      v.z = apply1<ACT>(v.z, mean, rstd, wc, bc); v.w = apply1<ACT>(v.w, mean, rstd, wc, bc);
      m = fmaxf(m, amax4(v));
      *reinterpret_cast<f32x4*>(dst + (size_t)i * 4) = v;
    } else {
      const float v = apply1<ACT>(src[i], mean, rstd, wc, bc);
      m = fmaxf(m, __builtin_fabsf(v));
      dst[i] = v;
    }
  }
  if (out_amax) {                                   // one merge per workgroup: the maximum does not depend on the order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < NT / 64; ++k) m = fmaxf(m, red[k]);
      atomicMax(out_amax + b, __builtin_bit_cast(unsigned, m));     // non-negative floats order like their bits
    }
  }
}

// (mean, rstd, sqrt(sum of squared deviations)) of one group from sum x and sum x^2 -- k_g1_final's arithmetic
__device__ __forceinline__ void finish_group(double s, double q, double inv_n, float eps, float& mean_f, float& rstd_f, float& dev_f) {
  const double mean = s * inv_n;
  double var = q * inv_n - mean * mean;
  if (var < 0.0) var = 0.0;
  mean_f = (float)mean;
  rstd_f = 1.0f / sqrtf((float)var + eps);
  dev_f = (float)sqrt(var / inv_n) * 1.0000005f;
}

// grid (G, B): the cpg * ntiles float4 entries of a group are contiguous in [B, C, ntiles, 4]
__global__ __launch_bounds__(NT) void k_gn_stats_tiles(float* __restrict__ stats, const float* __restrict__ ts, int G, int per_group,
                                                       double inv_n, float eps) {
  __shared__ double red[2][NT / 64];
  const int g = blockIdx.x, b = blockIdx.y;
  const float4* p = reinterpret_cast<const float4*>(ts) + ((size_t)b * G + g) * per_group;
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < per_group; i += NT) acc_tile(p[i], s, q);
  s = group_sum_d(s, 64);
  q = group_sum_d(q, 64);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tsum = 0.0, tq = 0.0;
    for (int k = 0; k < NT / 64; ++k) { tsum += red[0][k]; tq += red[1][k]; }
    float mean, rstd, dev;
    finish_group(tsum, tq, inv_n, eps, mean, rstd, dev);
    stats[((size_t)b * G + g) * 2 + 0] = mean;
    stats[((size_t)b * G + g) * 2 + 1] = rstd;
  }
}

// one workgroup per sample.  Phase 1: a wave per group (groups wave, wave + 16, ...) recombines the group's tile statistics, or
// the first G threads take the given (mean, rstd) pairs; phase 2: a thread per channel writes its row and the sample's bound
// U = max_c |A_c| sqrt(n_g var_g) + |C_c| gives the fourth column (ds_normtab.hip)
__global__ __launch_bounds__(TT) void k_gn_table(float* __restrict__ table, const float* __restrict__ ts, const float* __restrict__ stats,
                                                 const float* __restrict__ w, const float* __restrict__ bias, int C, int G, int cpg,
                                                 int ntiles, double inv_n, float eps) {
  __shared__ float st[3][MAXG];
  __shared__ unsigned smax;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) smax = 0u;
  if (ts) {
    const int per_group = cpg * ntiles, lane = threadIdx.x & 63;
    for (int g = threadIdx.x >> 6; g < G; g += TT / 64) {
      const float4* p = reinterpret_cast<const float4*>(ts) + ((size_t)b * G + g) * per_group;
      double s = 0.0, q = 0.0;
      for (int i = lane; i < per_group; i += 64) acc_tile(p[i], s, q);
      s = group_sum_d(s, 64);
      q = group_sum_d(q, 64);
      if (lane == 0) finish_group(s, q, inv_n, eps, st[0][g], st[1][g], st[2][g]);
    }
  } else {
    for (int g = threadIdx.x; g < G; g += TT) {
      const float mean = stats[((size_t)b * G + g) * 2], rstd = stats[((size_t)b * G + g) * 2 + 1];
      // var + eps = 1 / rstd^2 up to the roundings of rstd: an upper bound of var is all the exponent needs
      float var = 1.0f / (rstd * rstd) * 1.000001f - eps;
      if (!(var > 0.f)) var = 0.f;
      st[0][g] = mean; st[1][g] = rstd;
      st[2][g] = (float)sqrt((double)var / inv_n) * 1.0000005f;
    }
  }
  __syncthreads();
  const int Cpad = (C + 15) / 16 * 16;
  float4* rows = reinterpret_cast<float4*>(table) + (size_t)b * Cpad;
  float U = 0.f;
  for (int c = threadIdx.x; c < Cpad; c += TT) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);                   // rows past C: the zero padding of the last 16-channel chunk
    if (c < C) {
      const int g = c / cpg;
      o.x = st[0][g]; o.y = st[1][g] * (w ? w[c] : 1.f); o.z = bias ? bias[c] : 0.f;
      U = fmaxf(U, fabsf(o.y) * st[2][g] + fabsf(o.z));
    }
    rows[c] = o;
  }
  U = wave_max(U);
  if ((threadIdx.x & 63) == 0 && U > 0.f) atomicMax(&smax, __builtin_bit_cast(unsigned, U));    // LDS
  __syncthreads();
  const float inv = inv_scale_of(__builtin_bit_cast(float, smax));
  for (int c = threadIdx.x; c < Cpad; c += TT) reinterpret_cast<float*>(rows + c)[3] = inv;     // padded rows too: the loader reads any row's
}

}  // namespace

extern "C" {

int ds_groupnorm_stats(float* stats, void* workspace, const float* x, int B, int C, int G, int N, float eps, void* stream) {
  DS_REQUIRE(B >= 0 && C > 0 && G > 0 && N > 0, DS_ERR_SHAPE, "ds_groupnorm_stats: bad shape B=%d C=%d G=%d N=%d", B, C, G, N);
  DS_REQUIRE(C % G == 0, DS_ERR_SHAPE, "ds_groupnorm_stats: C=%d is not a multiple of G=%d", C, G);
  DS_REQUIRE((long long)B * G < 65536, DS_ERR_SHAPE, "ds_groupnorm_stats: B*G=%lld groups (at most 65535)", (long long)B * G);
  DS_REQUIRE((long long)(C / G) * N < (1ll << 31), DS_ERR_SHAPE, "ds_groupnorm_stats: a group exceeds 2^31 floats");
  // in NCHW a group is one contiguous run: GroupNorm(1, C/G) statistics of the [B*G, C/G, N] view
  return ds_gnorm1_stats(stats, workspace, x, B * G, C / G, N, eps, 0, stream);
}

int ds_groupnorm_apply(float* out, const float* x, const float* stats, const float* w, const float* b, int B, int C, int G, int N,
                       int act, unsigned* out_amax, void* stream) {
  DS_REQUIRE(out && x && stats, DS_ERR_NULL, "ds_groupnorm_apply: NULL pointer");
  DS_REQUIRE(B >= 0 && B < 65536 && C > 0 && C < 65536 && G > 0 && N > 0, DS_ERR_SHAPE,
             "ds_groupnorm_apply: bad shape B=%d C=%d G=%d N=%d (B, C at most 65535)", B, C, G, N);
  DS_REQUIRE(C % G == 0, DS_ERR_SHAPE, "ds_groupnorm_apply: C=%d is not a multiple of G=%d", C, G);
  DS_REQUIRE(act == 0 || act == 1, DS_ERR_UNSUPPORTED, "ds_groupnorm_apply: act %d (0 none, 1 SiLU)", act);
  if (B == 0) return DS_OK;
  // 16-byte path when every channel row starts 16-byte aligned; scalar path otherwise (tiny / odd planes)
  const bool vec = N % 4 == 0 && ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(x)) & 15u) == 0;
  const unsigned nv = (unsigned)(vec ? N / 4 : N);
  unsigned gx = (nv + NT - 1) / NT;                       // position chunks of a row: the rest of a large plane is grid-strided
  if (gx > (unsigned)MAX_CHUNKS) gx = MAX_CHUNKS;
  const dim3 grid(gx, (unsigned)C, (unsigned)B);
  hipStream_t s = ds::as_stream(stream);
#define L(V, A) hipLaunchKernelGGL((k_gn_apply<V, A>), grid, dim3(NT), 0, s, out, x, stats, w, b, G, C / G, nv, (size_t)N, out_amax)
  if (vec) { if (act) L(4, 1); else L(4, 0); }
  else { if (act) L(1, 1); else L(1, 0); }
#undef L
  DS_CHECK_LAUNCH("ds_groupnorm_apply");
  return DS_OK;
}

int ds_groupnorm_stats_tiles(float* stats, const float* tile_stats, int B, int C, int G, int ntiles, long long count, float eps,
                             void* stream) {
  DS_REQUIRE(stats && tile_stats, DS_ERR_NULL, "ds_groupnorm_stats_tiles: NULL pointer");
  DS_REQUIRE(B >= 0 && B < 65536 && C > 0 && G > 0 && ntiles > 0 && count > 0, DS_ERR_SHAPE, "ds_groupnorm_stats_tiles: bad shape");
  DS_REQUIRE(C % G == 0, DS_ERR_SHAPE, "ds_groupnorm_stats_tiles: C=%d is not a multiple of G=%d", C, G);
  DS_REQUIRE((long long)(C / G) * ntiles < (1ll << 31), DS_ERR_SHAPE, "ds_groupnorm_stats_tiles: too many tiles per group");
  DS_REQUIRE((reinterpret_cast<uintptr_t>(tile_stats) & 15u) == 0, DS_ERR_SHAPE, "ds_groupnorm_stats_tiles: tile statistics must be 16-byte aligned");
  if (B == 0) return DS_OK;
  hipLaunchKernelGGL(k_gn_stats_tiles, dim3((unsigned)G, (unsigned)B), dim3(NT), 0, ds::as_stream(stream), stats, tile_stats, G,
                     (C / G) * ntiles, 1.0 / ((double)count * (C / G)), eps);
  DS_CHECK_LAUNCH("ds_groupnorm_stats_tiles");
  return DS_OK;
}

int ds_groupnorm_table(float* table, const float* tile_stats, const float* stats, const float* w, const float* b, int B, int C, int G,
                       int ntiles, long long count, float eps, void* stream) {
  DS_REQUIRE(table, DS_ERR_NULL, "ds_groupnorm_table: NULL pointer");
  DS_REQUIRE((tile_stats == nullptr) != (stats == nullptr), DS_ERR_NULL, "ds_groupnorm_table: give tile_stats or stats, not both");
  DS_REQUIRE(B >= 0 && C > 0 && G > 0 && G <= MAXG && count > 0 && (stats || ntiles > 0), DS_ERR_SHAPE,
             "ds_groupnorm_table: bad shape B=%d C=%d G=%d (at most %d groups) ntiles=%d", B, C, G, MAXG, ntiles);
  DS_REQUIRE(C % G == 0, DS_ERR_SHAPE, "ds_groupnorm_table: C=%d is not a multiple of G=%d", C, G);
  DS_REQUIRE(!tile_stats || (long long)(C / G) * ntiles < (1ll << 31), DS_ERR_SHAPE, "ds_groupnorm_table: too many tiles per group");
  DS_REQUIRE(((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(tile_stats)) & 15u) == 0, DS_ERR_SHAPE,
             "ds_groupnorm_table: table and tile statistics must be 16-byte aligned");
  if (B == 0) return DS_OK;
  hipLaunchKernelGGL(k_gn_table, dim3((unsigned)B), dim3(TT), 0, ds::as_stream(stream), table, tile_stats, stats, w, b, C, G, C / G,
                     ntiles, 1.0 / ((double)count * (C / G)), eps);
  DS_CHECK_LAUNCH("ds_groupnorm_table");
  return DS_OK;
}

}  // extern "C"
