// Offset arithmetic of ds_box_copy3d (ds_window.hip), host and device: the one place where a box coordinate becomes an element
// offset.  Tensors are fp32 [N, S0, S1, S2] (source, periodic in its three spatial axes) and [N, D0, D1, D2] (destination, never
// wrapped).  Every per-axis quantity fits 31 bits; every product of plane, row and column is formed in size_t, because a whole
// stage of a chunked decode (32 channels at 1024^3: 3.4e10 elements) is far past 2^32.
//
// tools/box_index_check.cpp compiles this header with the host compiler and compares it with an independent restatement:
// negative starts, boxes of several periods, offsets past 2^31 and 2^32.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DS_WINDOW_HD __host__ __device__
#else
#define DS_WINDOW_HD
#endif

// s*: the source start per axis, already reduced to [0, S*) by ds_box_wrap; d*: the destination start; L*: the box.
struct ds_box_geom {
  uint32_t S0, S1, S2;
  uint32_t D0, D1, D2;
  uint32_t s0, s1, s2;
  uint32_t d0, d1, d2;
  uint32_t L0, L1, L2;
};

// v mod S with the sign of S (Euclidean: the result is in [0, S) for any v); S > 0.
DS_WINDOW_HD inline uint32_t ds_box_wrap(long long v, long long S) {
  const long long r = v % S;
  return (uint32_t)(r < 0 ? r + S : r);
}

// The geometry of one copy from the C ABI's arguments (the caller has checked 0 < S*, D* < 2^31, the box inside dst).
inline ds_box_geom ds_box_make_geom(int S0, int S1, int S2, long long s0, long long s1, long long s2, int D0, int D1, int D2, int d0,
                                    int d1, int d2, int L0, int L1, int L2) {
  ds_box_geom g;
  g.S0 = (uint32_t)S0; g.S1 = (uint32_t)S1; g.S2 = (uint32_t)S2;
  g.D0 = (uint32_t)D0; g.D1 = (uint32_t)D1; g.D2 = (uint32_t)D2;
  g.s0 = ds_box_wrap(s0, S0); g.s1 = ds_box_wrap(s1, S1); g.s2 = ds_box_wrap(s2, S2);
  g.d0 = (uint32_t)d0; g.d1 = (uint32_t)d1; g.d2 = (uint32_t)d2;
  g.L0 = (uint32_t)L0; g.L1 = (uint32_t)L1; g.L2 = (uint32_t)L2;
  return g;
}

// Source column of box column k (k < L2 < 2^31 and s2 < S2 < 2^31, so the sum fits 32 unsigned bits).
DS_WINDOW_HD inline uint32_t ds_box_src_col(const ds_box_geom& g, uint32_t k) { return (g.s2 + k) % g.S2; }

// Box row `rp` of plane n (rp = i * L1 + j, rp < L0 * L1 < 2^31): the element offsets of the source row's column 0 and of the
// destination element that receives box column 0.  The two outer moduli of a row are taken here, once.
DS_WINDOW_HD inline void ds_box_row_offsets(const ds_box_geom& g, uint32_t n, uint32_t rp, size_t* src_row, size_t* dst_first) {
  const uint32_t i = rp / g.L1, j = rp - i * g.L1;
  const uint32_t a0 = (g.s0 + i) % g.S0, a1 = (g.s1 + j) % g.S1;
  *src_row = (((size_t)n * g.S0 + a0) * g.S1 + a1) * g.S2;
  *dst_first = (((size_t)n * g.D0 + (g.d0 + i)) * g.D1 + (g.d1 + j)) * g.D2 + g.d2;
}
