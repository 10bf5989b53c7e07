// Box copies between a dense and a periodic tensor, fp32, plane by plane.
// k_box_copy3d, the gather -- the source wraps:
//   dst[n, d0+i, d1+j, d2+k] = src[n, (s0+i) mod S0, (s1+j) mod S1, (s2+k) mod S2]      0 <= i < L0, j < L1, k < L2
// over [N, S0, S1, S2] -> [N, D0, D1, D2].  The modulus is Euclidean (negative starts), a box may span several periods of an axis,
// the destination box never wraps.  The chunked volume decode (diffsci_amd/extra/chunk_decode.py) gathers a halo window of a
// stage buffer into a contiguous tile and places a tile's valid centre in the next stage buffer with it; the tiled volume
// sampling (diffsci_amd/extra/fillinginpainting.py) gathers a cube's noise, known data and mask.
// k_box_scatter3d, the scatter -- the destination wraps, the box lies inside src, and is no longer than a destination axis: the
// tiled volume sampling writes a generated cube back into a periodic volume.  Both are copies: bit-exact.
//
// Memory-bound, so the shape is that of ds_upsample_f: a thread owns four consecutive floats of the inner axis.  A wave owns whole
// box rows -- 64 / LPR of them, LPR the power of two that covers a row's quads (at most 64; longer rows loop) -- so the row
// decomposition and the two outer moduli cost once per (lane, row) and the inner loop carries one 32-bit modulus per quad.  A quad
// moves as one 16-byte load and one 16-byte store when its four sources do not cross the period and both addresses are 16-byte
// aligned; any other quad (a wrap inside it, a ragged tail, an odd start) takes four element loads and stores in the same launch.
// Offsets: ds_window.h (size_t products; checked on the host by tools/box_index_check.cpp).
#include "ds_common.h"
#include "ds_window.h"

namespace {

constexpr int NT = 256;
constexpr unsigned MAX_BLOCKS = 2048;          // memory-bound: grid-stride the rest

__global__ __launch_bounds__(NT) void k_box_copy3d(float* __restrict__ dst, const float* __restrict__ src, ds_box_geom g,
                                                   unsigned planes, unsigned rows, unsigned quads, unsigned lpr_shift) {
  const unsigned lpr = 1u << lpr_shift;                                  // lanes per row
  const unsigned rpb = NT >> lpr_shift;                                  // rows per block
  const unsigned sub = threadIdx.x >> lpr_shift, ql = threadIdx.x & (lpr - 1);
  for (unsigned n = blockIdx.y; n < planes; n += gridDim.y) {
    for (unsigned rp = blockIdx.x * rpb + sub; rp < rows; rp += gridDim.x * rpb) {     // rows < 2^31, the stride <= 2^20
      size_t so, dx;
      ds_box_row_offsets(g, n, rp, &so, &dx);
      const float* srow = src + so;
      float* drow = dst + dx;
      for (unsigned q = ql; q < quads; q += lpr) {
        const unsigned k = 4 * q;
        const unsigned c = ds_box_src_col(g, k);
        const float* sp = srow + c;
        float* dp = drow + k;
        const bool whole = k + 4 <= g.L2 && c + 4 <= g.S2;
        if (whole && ((reinterpret_cast<uintptr_t>(sp) | reinterpret_cast<uintptr_t>(dp)) & 15u) == 0) {
          *reinterpret_cast<float4*>(dp) = *reinterpret_cast<const float4*>(sp);
        } else {
          const unsigned m = g.L2 - k < 4 ? g.L2 - k : 4;
          float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (unsigned e = 0; e < 4; ++e)
            if (e < m) v[e] = srow[whole ? c + e : ds_box_src_col(g, k + e)];
#pragma unroll
          for (unsigned e = 0; e < 4; ++e)
            if (e < m) dp[e] = v[e];
        }
      }
    }
  }
}

// The scatter: dst[n, (d0+i) mod D0, (d1+j) mod D1, (d2+k) mod D2] = src[n, s0+i, s1+j, s2+k] -- the box lies inside src, the
// destination wraps (the tiled volume sampling writes a generated cube back into a periodic volume).  The same geometry with the
// roles exchanged: g.S*, g.s* describe the periodic tensor (here dst), g.D*, g.d* the dense one (here src).  L* <= D* per axis
// (checked by the caller), so no destination element is written twice.
__global__ __launch_bounds__(NT) void k_box_scatter3d(float* __restrict__ dst, const float* __restrict__ src, ds_box_geom g,
                                                      unsigned planes, unsigned rows, unsigned quads, unsigned lpr_shift) {
  const unsigned lpr = 1u << lpr_shift;
  const unsigned rpb = NT >> lpr_shift;
  const unsigned sub = threadIdx.x >> lpr_shift, ql = threadIdx.x & (lpr - 1);
  for (unsigned n = blockIdx.y; n < planes; n += gridDim.y) {
    for (unsigned rp = blockIdx.x * rpb + sub; rp < rows; rp += gridDim.x * rpb) {
      size_t wo, ux;
      ds_box_row_offsets(g, n, rp, &wo, &ux);                              // wo: the wrapped row of dst; ux: the box row's first source
      float* drow = dst + wo;
      const float* srow = src + ux;
      for (unsigned q = ql; q < quads; q += lpr) {
        const unsigned k = 4 * q;
        const unsigned c = ds_box_src_col(g, k);
        const float* sp = srow + k;
        float* dp = drow + c;
        const bool whole = k + 4 <= g.L2 && c + 4 <= g.S2;
        if (whole && ((reinterpret_cast<uintptr_t>(sp) | reinterpret_cast<uintptr_t>(dp)) & 15u) == 0) {
          *reinterpret_cast<float4*>(dp) = *reinterpret_cast<const float4*>(sp);
        } else {
          const unsigned m = g.L2 - k < 4 ? g.L2 - k : 4;
          float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (unsigned e = 0; e < 4; ++e)
            if (e < m) v[e] = sp[e];
#pragma unroll
          for (unsigned e = 0; e < 4; ++e)
            if (e < m) drow[whole ? c + e : ds_box_src_col(g, k + e)] = v[e];
        }
      }
    }
  }
}

// rows of a box over the planes: the launch geometry both kernels share
inline void box_launch_shape(int planes, int L0, int L1, int L2, unsigned* rows, unsigned* quads, unsigned* shift, dim3* grid) {
  *rows = (unsigned)L0 * (unsigned)L1;
  *quads = ((unsigned)L2 + 3) / 4;
  unsigned sh = 0;                                                       // lanes per row: 1 .. 64
  while (sh < 6 && (1u << sh) < *quads) ++sh;
  *shift = sh;
  const unsigned rpb = NT >> sh;
  const unsigned gy = (unsigned)planes < 1024u ? (unsigned)planes : 1024u;
  unsigned gx = (*rows + rpb - 1) / rpb;
  const unsigned most = MAX_BLOCKS / gy > 0 ? MAX_BLOCKS / gy : 1;
  if (gx > most) gx = most;
  *grid = dim3(gx, gy);
}

}  // namespace

extern "C" int ds_box_copy3d(float* dst, const float* src, int planes, int S0, int S1, int S2, long long s0, long long s1,
                             long long s2, int D0, int D1, int D2, int d0, int d1, int d2, int L0, int L1, int L2, void* stream) {
  DS_REQUIRE(dst && src, DS_ERR_NULL, "ds_box_copy3d: NULL pointer");
  DS_REQUIRE(planes >= 0 && S0 > 0 && S1 > 0 && S2 > 0 && D0 > 0 && D1 > 0 && D2 > 0, DS_ERR_SHAPE, "ds_box_copy3d: bad shape");
  DS_REQUIRE(L0 >= 0 && L1 >= 0 && L2 >= 0, DS_ERR_SHAPE, "ds_box_copy3d: negative box (%d, %d, %d)", L0, L1, L2);
  DS_REQUIRE(d0 >= 0 && d1 >= 0 && d2 >= 0 && (long long)d0 + L0 <= D0 && (long long)d1 + L1 <= D1 && (long long)d2 + L2 <= D2,
             DS_ERR_SHAPE, "ds_box_copy3d: destination box start (%d, %d, %d) size (%d, %d, %d) leaves dst (%d, %d, %d)", d0, d1, d2,
             L0, L1, L2, D0, D1, D2);
  if (planes == 0 || L0 == 0 || L1 == 0 || L2 == 0) return DS_OK;
  DS_REQUIRE((long long)L0 * L1 < (1ll << 31) - (long long)MAX_BLOCKS * NT, DS_ERR_SHAPE,
             "ds_box_copy3d: %d x %d box rows per plane exceed 31 bits", L0, L1);
  const ds_box_geom g = ds_box_make_geom(S0, S1, S2, s0, s1, s2, D0, D1, D2, d0, d1, d2, L0, L1, L2);
  unsigned rows, quads, shift;
  dim3 grid;
  box_launch_shape(planes, L0, L1, L2, &rows, &quads, &shift, &grid);
  hipLaunchKernelGGL(k_box_copy3d, grid, dim3(NT), 0, ds::as_stream(stream), dst, src, g, (unsigned)planes, rows, quads, shift);
  DS_CHECK_LAUNCH("ds_box_copy3d");
  return DS_OK;
}

extern "C" int ds_box_scatter3d(float* dst, const float* src, int planes, int D0, int D1, int D2, long long d0, long long d1,
                                long long d2, int S0, int S1, int S2, int s0, int s1, int s2, int L0, int L1, int L2, void* stream,
                                int flags) {
  DS_REQUIRE(dst && src, DS_ERR_NULL, "ds_box_scatter3d: NULL pointer");
  DS_REQUIRE(flags == 0, DS_ERR_SHAPE, "ds_box_scatter3d: flags %d (none are defined)", flags);
  DS_REQUIRE(planes >= 0 && S0 > 0 && S1 > 0 && S2 > 0 && D0 > 0 && D1 > 0 && D2 > 0, DS_ERR_SHAPE, "ds_box_scatter3d: bad shape");
  DS_REQUIRE(L0 >= 0 && L1 >= 0 && L2 >= 0, DS_ERR_SHAPE, "ds_box_scatter3d: negative box (%d, %d, %d)", L0, L1, L2);
  DS_REQUIRE(s0 >= 0 && s1 >= 0 && s2 >= 0 && (long long)s0 + L0 <= S0 && (long long)s1 + L1 <= S1 && (long long)s2 + L2 <= S2,
             DS_ERR_SHAPE, "ds_box_scatter3d: source box start (%d, %d, %d) size (%d, %d, %d) leaves src (%d, %d, %d)", s0, s1, s2,
             L0, L1, L2, S0, S1, S2);
  DS_REQUIRE(L0 <= D0 && L1 <= D1 && L2 <= D2, DS_ERR_SHAPE,
             "ds_box_scatter3d: box (%d, %d, %d) longer than a destination axis (%d, %d, %d): a periodic write of more than one period",
             L0, L1, L2, D0, D1, D2);
  if (planes == 0 || L0 == 0 || L1 == 0 || L2 == 0) return DS_OK;
  DS_REQUIRE((long long)L0 * L1 < (1ll << 31) - (long long)MAX_BLOCKS * NT, DS_ERR_SHAPE,
             "ds_box_scatter3d: %d x %d box rows per plane exceed 31 bits", L0, L1);
  // the periodic tensor takes the geometry's S / s slots, the dense one its D / d slots (ds_window.h)
  const ds_box_geom g = ds_box_make_geom(D0, D1, D2, d0, d1, d2, S0, S1, S2, s0, s1, s2, L0, L1, L2);
  unsigned rows, quads, shift;
  dim3 grid;
  box_launch_shape(planes, L0, L1, L2, &rows, &quads, &shift, &grid);
  hipLaunchKernelGGL(k_box_scatter3d, grid, dim3(NT), 0, ds::as_stream(stream), dst, src, g, (unsigned)planes, rows, quads, shift);
  DS_CHECK_LAUNCH("ds_box_scatter3d");
  return DS_OK;
}
