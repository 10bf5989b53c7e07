// Offset arithmetic of ds_crop_blend (ds_periodize.hip), host and device: the one place where an output coordinate becomes an
// element offset of the expanded tensor.  Tensors are fp32, dense: the expanded y [N, A0+2p0, A1+2p1, A2+2p2] and the cropped
// out [N, A0, A1, A2].  Every per-axis quantity fits 31 bits; every product of plane, row and column is formed in size_t (an
// expanded 1024^3 volume of a few channels is past 2^32 elements).
//
// tools/periodize_index_check.cpp compiles this header with the host compiler and compares it with an independent restatement
// at extents whose offsets pass 2^31 and 2^32.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ds_window.h"       // DS_WINDOW_HD

// A*: the cropped extents; E* = A* + 2 p*: the expanded ones; p*: the pad per side; bw*: the blend width of an ACTIVE axis, 0 for
// an axis that is skipped (bw <= 0 or 2 bw >= A: ds_periodize_width).
struct ds_periodize_geom {
  uint32_t A0, A1, A2;
  uint32_t E0, E1, E2;
  uint32_t p0, p1, p2;
  uint32_t bw0, bw1, bw2;
};

// The width the kernel blends axis of extent A with: bw when the axis is active (bw > 0 and 2 bw < A), else 0 -- the reference's
// two `continue`s (periodizer.py:148-156).
DS_WINDOW_HD inline uint32_t ds_periodize_width(long long A, long long bw) { return bw > 0 && 2 * bw < A ? (uint32_t)bw : 0u; }

inline ds_periodize_geom ds_periodize_make_geom(int A0, int A1, int A2, int p0, int p1, int p2, int bw0, int bw1, int bw2) {
  ds_periodize_geom g;
  g.A0 = (uint32_t)A0; g.A1 = (uint32_t)A1; g.A2 = (uint32_t)A2;
  g.p0 = (uint32_t)p0; g.p1 = (uint32_t)p1; g.p2 = (uint32_t)p2;
  g.E0 = g.A0 + 2u * g.p0; g.E1 = g.A1 + 2u * g.p1; g.E2 = g.A2 + 2u * g.p2;
  g.bw0 = ds_periodize_width(A0, bw0); g.bw1 = ds_periodize_width(A1, bw1); g.bw2 = ds_periodize_width(A2, bw2);
  return g;
}

// The position across the axis that position q (q < A) is blended with.
DS_WINDOW_HD inline uint32_t ds_periodize_mirror(uint32_t A, uint32_t q) { return A - 1u - q; }

// Distance of q from the nearer end of the axis: the index of its weight, and < bw exactly inside the two strips.
DS_WINDOW_HD inline uint32_t ds_periodize_depth(uint32_t A, uint32_t q) {
  const uint32_t r = A - 1u - q;
  return q < r ? q : r;
}

// Element offset in y of the value that the crop puts at out[n, i, j, k].
DS_WINDOW_HD inline size_t ds_periodize_src(const ds_periodize_geom& g, uint32_t n, uint32_t i, uint32_t j, uint32_t k) {
  return (((size_t)n * g.E0 + (g.p0 + i)) * g.E1 + (g.p1 + j)) * g.E2 + (g.p2 + k);
}

// Output row `rp` of plane n (rp = i * A1 + j, rp < A0 * A1 < 2^31): its coordinates and the offset of its first element in out.
DS_WINDOW_HD inline size_t ds_periodize_dst_row(const ds_periodize_geom& g, uint32_t n, uint32_t rp, uint32_t* i, uint32_t* j) {
  *i = rp / g.A1;
  *j = rp - *i * g.A1;
  return ((size_t)n * g.A0 * g.A1 + rp) * g.A2;
}
