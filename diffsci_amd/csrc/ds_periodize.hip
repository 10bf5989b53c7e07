// The output side of DiffusionPeriodizer (periodizer.py:103-199), fp32, one pass: crop the centre of the network's output on the
// periodically expanded state and cross-fade opposite borders with cosine weights,
//   out [N, A0, A1, A2]  <-  y [N, A0+2p0, A1+2p1, A2+2p2]
// crop_center, then cosine_blend_boundaries: the axes in tensor order, a later axis blending what the earlier one blended.  On an
// active axis (bw > 0 and 2 bw < A) position q with m = min(q, A-1-q) < bw becomes
//   v'(q) = fl( fl(w[m] * v(q)) + fl( fl(1 - w[m]) * v(A-1-q) ) )
// from the axis' pre-blend values (the reference forms both strips before it assigns either); every other position, and every
// position of an inactive axis, keeps v(q).  A corner therefore reads 8 elements of y, an edge 4, a face 2, the interior 1; no
// cropped intermediate exists.  The products and the sum are rounded separately (__fmul_rn / __fadd_rn: no FMA contraction), in
// the reference's order, so with the reference's weight table w[i] = 0.5 (1 - cos(pi (i + 0.5) / bw)) -- built on the host, passed
// per axis -- the result is the reference's fp32 result bit for bit.
//
// Memory-bound, and shaped as ds_window.hip's copies: a thread owns four consecutive floats of the inner axis, a wave whole rows.
// A quad outside every strip moves as one 16-byte load and store when both addresses allow; a quad in a strip, a ragged tail or a
// misaligned row takes the element path in the same launch.  Offsets: ds_periodize.h (size_t products; checked on the host by
// tools/periodize_index_check.cpp).
#include "ds_common.h"
#include "ds_periodize.h"

namespace {

constexpr int NT = 256;
constexpr unsigned MAX_BLOCKS = 2048;          // memory-bound: grid-stride the rest

__device__ __forceinline__ float pz_blend(float w, float a, float b) {
  return __fadd_rn(__fmul_rn(w, a), __fmul_rn(__fsub_rn(1.0f, w), b));
}

// the value at (i, j, k) of plane n after the crop and the blend of axis 0
__device__ __forceinline__ float pz_axis0(const float* __restrict__ y, const ds_periodize_geom& g, const float* __restrict__ w0,
                                          uint32_t n, uint32_t i, uint32_t j, uint32_t k) {
  const float v = y[ds_periodize_src(g, n, i, j, k)];
  const uint32_t m = ds_periodize_depth(g.A0, i);
  if (m >= g.bw0) return v;
  return pz_blend(w0[m], v, y[ds_periodize_src(g, n, ds_periodize_mirror(g.A0, i), j, k)]);
}

// ... after the blends of axes 0 and 1
__device__ __forceinline__ float pz_axis1(const float* __restrict__ y, const ds_periodize_geom& g, const float* __restrict__ w0,
                                          const float* __restrict__ w1, uint32_t n, uint32_t i, uint32_t j, uint32_t k) {
  const float v = pz_axis0(y, g, w0, n, i, j, k);
  const uint32_t m = ds_periodize_depth(g.A1, j);
  if (m >= g.bw1) return v;
  return pz_blend(w1[m], v, pz_axis0(y, g, w0, n, i, ds_periodize_mirror(g.A1, j), k));
}

// ... after all three
__device__ __forceinline__ float pz_axis2(const float* __restrict__ y, const ds_periodize_geom& g, const float* __restrict__ w0,
                                          const float* __restrict__ w1, const float* __restrict__ w2, uint32_t n, uint32_t i,
                                          uint32_t j, uint32_t k) {
  const float v = pz_axis1(y, g, w0, w1, n, i, j, k);
  const uint32_t m = ds_periodize_depth(g.A2, k);
  if (m >= g.bw2) return v;
  return pz_blend(w2[m], v, pz_axis1(y, g, w0, w1, n, i, j, ds_periodize_mirror(g.A2, k)));
}

__global__ __launch_bounds__(NT) void k_crop_blend(float* __restrict__ out, const float* __restrict__ y, ds_periodize_geom g,
                                                   const float* __restrict__ w0, const float* __restrict__ w1,
                                                   const float* __restrict__ w2, unsigned planes, unsigned rows, unsigned quads,
                                                   unsigned lpr_shift) {
  const unsigned lpr = 1u << lpr_shift;                                  // lanes per row
  const unsigned rpb = NT >> lpr_shift;                                  // rows per block
  const unsigned sub = threadIdx.x >> lpr_shift, ql = threadIdx.x & (lpr - 1);
  for (unsigned n = blockIdx.y; n < planes; n += gridDim.y) {
    for (unsigned rp = blockIdx.x * rpb + sub; rp < rows; rp += gridDim.x * rpb) {     // rows < 2^31, the stride <= 2^20
      uint32_t i, j;
      float* drow = out + ds_periodize_dst_row(g, n, rp, &i, &j);
      const float* srow = y + ds_periodize_src(g, n, i, j, 0);
      const bool row_plain = ds_periodize_depth(g.A0, i) >= g.bw0 && ds_periodize_depth(g.A1, j) >= g.bw1;
      for (unsigned q = ql; q < quads; q += lpr) {
        const unsigned k = 4 * q;
        const float* sp = srow + k;
        float* dp = drow + k;
        // whole, and outside the strips of axis 2: bw2 <= k and k + 3 <= A2 - 1 - bw2 (2 bw2 < A2, so no term is negative)
        const bool plain = row_plain && k + 4 <= g.A2 - g.bw2 && k >= g.bw2;
        if (plain && ((reinterpret_cast<uintptr_t>(sp) | reinterpret_cast<uintptr_t>(dp)) & 15u) == 0) {
          *reinterpret_cast<float4*>(dp) = *reinterpret_cast<const float4*>(sp);
        } else {
          const unsigned m = g.A2 - k < 4 ? g.A2 - k : 4;
          float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (unsigned e = 0; e < 4; ++e)
            if (e < m) v[e] = plain ? sp[e] : pz_axis2(y, g, w0, w1, w2, n, i, j, k + e);
#pragma unroll
          for (unsigned e = 0; e < 4; ++e)
            if (e < m) dp[e] = v[e];
        }
      }
    }
  }
}

}  // namespace

extern "C" int ds_crop_blend(float* out, const float* y, int planes, int A0, int A1, int A2, int p0, int p1, int p2, int bw0, int bw1,
                             int bw2, const float* w0, const float* w1, const float* w2, void* stream, int flags) {
  DS_REQUIRE(out && y, DS_ERR_NULL, "ds_crop_blend: NULL pointer");
  DS_REQUIRE(flags == 0, DS_ERR_UNSUPPORTED, "ds_crop_blend: flags %d (none are defined)", flags);
  DS_REQUIRE(planes >= 0 && A0 > 0 && A1 > 0 && A2 > 0, DS_ERR_SHAPE, "ds_crop_blend: bad shape (%d planes of %d x %d x %d)", planes,
             A0, A1, A2);
  DS_REQUIRE(p0 >= 0 && p1 >= 0 && p2 >= 0, DS_ERR_SHAPE, "ds_crop_blend: negative pad (%d, %d, %d)", p0, p1, p2);
  DS_REQUIRE(bw0 >= 0 && bw1 >= 0 && bw2 >= 0, DS_ERR_SHAPE, "ds_crop_blend: negative blend width (%d, %d, %d)", bw0, bw1, bw2);
  DS_REQUIRE((long long)A0 + 2ll * p0 < (1ll << 31) && (long long)A1 + 2ll * p1 < (1ll << 31) && (long long)A2 + 2ll * p2 < (1ll << 31),
             DS_ERR_SHAPE, "ds_crop_blend: an expanded axis exceeds 31 bits");
  DS_REQUIRE((long long)A0 * A1 < (1ll << 31) - (long long)MAX_BLOCKS * NT, DS_ERR_SHAPE,
             "ds_crop_blend: %d x %d rows per plane exceed 31 bits", A0, A1);
  const ds_periodize_geom g = ds_periodize_make_geom(A0, A1, A2, p0, p1, p2, bw0, bw1, bw2);
  DS_REQUIRE((!g.bw0 || w0) && (!g.bw1 || w1) && (!g.bw2 || w2), DS_ERR_SHAPE,
             "ds_crop_blend: an axis that is blended (widths %u, %u, %u) has no weight table", g.bw0, g.bw1, g.bw2);
  if (planes == 0) return DS_OK;
  {
    const uintptr_t ob = reinterpret_cast<uintptr_t>(out), yb = reinterpret_cast<uintptr_t>(y);
    const size_t on = (size_t)planes * g.A0 * g.A1 * g.A2 * sizeof(float), yn = (size_t)planes * g.E0 * g.E1 * g.E2 * sizeof(float);
    DS_REQUIRE(ob + on <= yb || yb + yn <= ob, DS_ERR_SHAPE, "ds_crop_blend: out and y overlap");
  }
  const unsigned rows = g.A0 * g.A1, quads = (g.A2 + 3) / 4;
  unsigned shift = 0;                                                    // lanes per row: 1 .. 64
  while (shift < 6 && (1u << shift) < quads) ++shift;
  const unsigned rpb = NT >> shift;
  // The grid is capped and the kernel loops: at most 1024 planes in grid.y (the plane loop strides the rest) and at most
  // MAX_BLOCKS workgroups in all (the row loop strides the rest); rows longer than 64 quads loop inside a wave.
  const unsigned gy = (unsigned)planes < 1024u ? (unsigned)planes : 1024u;
  unsigned gx = (rows + rpb - 1) / rpb;
  const unsigned most = MAX_BLOCKS / gy > 0 ? MAX_BLOCKS / gy : 1;
  if (gx > most) gx = most;
  hipLaunchKernelGGL(k_crop_blend, dim3(gx, gy), dim3(NT), 0, ds::as_stream(stream), out, y, g, w0, w1, w2, (unsigned)planes, rows,
                     quads, shift);
  DS_CHECK_LAUNCH("ds_crop_blend");
  return DS_OK;
}
