// Box copy with a periodic source, the data movement of the chunked volume decode (diffsci_amd/extra/chunk_decode.py):
//   dst[n, d0+i, d1+j, d2+k] = src[n, (s0+i) mod S0, (s1+j) mod S1, (s2+k) mod S2]      0 <= i < L0, j < L1, k < L2
// over fp32 [N, S0, S1, S2] -> [N, D0, D1, D2].  The modulus is Euclidean (negative starts), a box may span several periods of an
// axis, the destination box never wraps.  Gather: a halo window of a stage buffer into a contiguous tile (d = 0, D = L).  Scatter:
// a tile's valid centre into the next stage buffer (the source in range).  A copy: bit-exact.
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
  const unsigned rows = (unsigned)L0 * (unsigned)L1;
  const unsigned quads = ((unsigned)L2 + 3) / 4;
  unsigned shift = 0;                                                    // lanes per row: 1 .. 64
  while (shift < 6 && (1u << shift) < quads) ++shift;
  const unsigned rpb = NT >> shift;
  const unsigned gy = (unsigned)planes < 1024u ? (unsigned)planes : 1024u;
  unsigned gx = (rows + rpb - 1) / rpb;
  const unsigned most = MAX_BLOCKS / gy > 0 ? MAX_BLOCKS / gy : 1;
  if (gx > most) gx = most;
  hipLaunchKernelGGL(k_box_copy3d, dim3(gx, gy), dim3(NT), 0, ds::as_stream(stream), dst, src, g, (unsigned)planes, rows, quads,
                     shift);
  DS_CHECK_LAUNCH("ds_box_copy3d");
  return DS_OK;
}
