// Host check of diffsci_amd/csrc/ds_window.h, the offset arithmetic of ds_box_copy3d: built with the host compiler, no GPU.
//
//     c++ -std=c++17 -O1 -Wall -fsanitize=address,undefined -o /tmp/box_index_check tools/box_index_check.cpp && /tmp/box_index_check
//
// The header's offsets (32-bit axis indices, unsigned moduli after one Euclidean reduction of the start, Horner products in size_t)
// are compared with an independent restatement: 128-bit integers, the period removed by floor division, strides multiplied out.
//   1. small boxes, every element: negative starts, boxes of several periods, an inner axis of size 1, a scatter to a far corner
//      -- and the copy itself replayed on host arrays against a loop that wraps by repeated addition / subtraction;
//   2. large tensors, sampled elements: [2, 1024, 1024, 1025] (offsets past 2^31), [32, 1024, 1024, 1024] (past 2^32, up to
//      3.4e10), windows that wrap around the last corner; each sampled offset must also stay inside its tensor.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../diffsci_amd/csrc/ds_window.h"

typedef __int128 i128;

static i128 floor_mod(i128 v, i128 S) {
  i128 q = v / S;
  if ((v % S != 0) && ((v < 0) != (S < 0))) --q;          // floor division
  return v - q * S;
}

struct Case {
  int planes, S[3];
  long long s[3];
  int D[3], d[3], L[3];
};

static int failures = 0;

static void expect(bool ok, const char* what, const Case& c, long long n, long long i, long long j, long long k) {
  if (ok) return;
  if (++failures <= 10)
    std::fprintf(stderr, "FAIL %s: S=(%d,%d,%d) s=(%lld,%lld,%lld) at n=%lld i=%lld j=%lld k=%lld\n", what, c.S[0], c.S[1], c.S[2],
                 c.s[0], c.s[1], c.s[2], n, i, j, k);
}

static void check_element(const Case& c, const ds_box_geom& g, long long n, long long i, long long j, long long k) {
  size_t so, dx;
  ds_box_row_offsets(g, (uint32_t)n, (uint32_t)(i * c.L[1] + j), &so, &dx);
  const size_t got_src = so + ds_box_src_col(g, (uint32_t)k), got_dst = dx + (size_t)k;
  const i128 st2 = 1, st1 = (i128)c.S[2], st0 = st1 * c.S[1], stn = st0 * c.S[0];
  const i128 want_src = n * stn + floor_mod((i128)c.s[0] + i, c.S[0]) * st0 + floor_mod((i128)c.s[1] + j, c.S[1]) * st1 +
                        floor_mod((i128)c.s[2] + k, c.S[2]) * st2;
  const i128 dt1 = (i128)c.D[2], dt0 = dt1 * c.D[1], dtn = dt0 * c.D[0];
  const i128 want_dst = n * dtn + ((i128)c.d[0] + i) * dt0 + ((i128)c.d[1] + j) * dt1 + ((i128)c.d[2] + k);
  expect((i128)got_src == want_src, "source offset", c, n, i, j, k);
  expect((i128)got_dst == want_dst, "destination offset", c, n, i, j, k);
  expect((i128)got_src < stn * c.planes, "source offset inside src", c, n, i, j, k);
  expect((i128)got_dst < dtn * c.planes, "destination offset inside dst", c, n, i, j, k);
}

static ds_box_geom geom(const Case& c) {
  return ds_box_make_geom(c.S[0], c.S[1], c.S[2], c.s[0], c.s[1], c.s[2], c.D[0], c.D[1], c.D[2], c.d[0], c.d[1], c.d[2], c.L[0],
                          c.L[1], c.L[2]);
}

static long long slow_wrap(long long v, long long S) {
  while (v < 0) v += S;
  while (v >= S) v -= S;
  return v;
}

// every element of a small case, then the copy on host arrays
static void small(const Case& c) {
  const ds_box_geom g = geom(c);
  const size_t ns = (size_t)c.planes * c.S[0] * c.S[1] * c.S[2], nd = (size_t)c.planes * c.D[0] * c.D[1] * c.D[2];
  std::vector<float> src(ns), got(nd, -7.f), want(nd, -7.f);
  for (size_t e = 0; e < ns; ++e) src[e] = (float)e;
  for (long long n = 0; n < c.planes; ++n)
    for (long long i = 0; i < c.L[0]; ++i)
      for (long long j = 0; j < c.L[1]; ++j) {
        size_t so, dx;
        ds_box_row_offsets(g, (uint32_t)n, (uint32_t)(i * c.L[1] + j), &so, &dx);
        for (long long k = 0; k < c.L[2]; ++k) {
          check_element(c, g, n, i, j, k);
          got.at(dx + k) = src.at(so + ds_box_src_col(g, (uint32_t)k));
          const long long a0 = slow_wrap(c.s[0] + i, c.S[0]), a1 = slow_wrap(c.s[1] + j, c.S[1]), a2 = slow_wrap(c.s[2] + k, c.S[2]);
          want.at(((n * c.D[0] + c.d[0] + i) * c.D[1] + c.d[1] + j) * c.D[2] + c.d[2] + k) =
              src.at(((n * c.S[0] + a0) * c.S[1] + a1) * c.S[2] + a2);
        }
      }
  if (got != want) {
    ++failures;
    std::fprintf(stderr, "FAIL copy replay: S=(%d,%d,%d)\n", c.S[0], c.S[1], c.S[2]);
  }
}

// the corners and a pseudo-random sample of a large case
static void large(const Case& c) {
  const ds_box_geom g = geom(c);
  unsigned long long state = 0x9E3779B97F4A7C15ull;
  auto next = [&](long long m) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (long long)((state >> 33) % (unsigned long long)m);
  };
  for (long long n : {0ll, (long long)c.planes - 1})
    for (long long i : {0ll, (long long)c.L[0] - 1})
      for (long long j : {0ll, (long long)c.L[1] - 1})
        for (long long k : {0ll, (long long)c.L[2] - 1}) check_element(c, g, n, i, j, k);
  for (int t = 0; t < 200000; ++t) check_element(c, g, next(c.planes), next(c.L[0]), next(c.L[1]), next(c.L[2]));
}

int main() {
  // wrap itself
  for (long long S : {1ll, 3ll, 5ll, 1025ll, 2147483647ll})
    for (long long v : {-4294967301ll, -2147483649ll, -11ll, -5ll, -1ll, 0ll, 1ll, 4ll, 5ll, 23ll, 2147483647ll, 4294967301ll})
      if ((i128)ds_box_wrap(v, S) != floor_mod(v, S)) {
        ++failures;
        std::fprintf(stderr, "FAIL ds_box_wrap(%lld, %lld)\n", v, S);
      }
  const Case smalls[] = {
      {6, {3, 5, 7}, {-4, -11, -3}, {10, 23, 9}, {0, 0, 0}, {10, 23, 9}},          // several periods on every axis
      {2, {4, 8, 64}, {0, 0, 0}, {4, 8, 64}, {0, 0, 0}, {4, 8, 64}},               // the identity
      {2, {4, 8, 64}, {1, -2, -6}, {4, 8, 64}, {0, 0, 0}, {4, 8, 64}},             // a wrap inside the inner axis
      {3, {5, 6, 10}, {2, 1, 3}, {7, 9, 13}, {5, 6, 8}, {2, 3, 5}},                // a scatter to the far corner
      {2, {2, 2, 1}, {0, 0, -1}, {2, 2, 3}, {0, 0, 0}, {2, 2, 3}},                 // an inner axis of size 1
      {1, {5, 5, 5}, {-5, -10, 12}, {15, 15, 15}, {0, 0, 0}, {15, 15, 15}},        // slice(-5, 10) of a size-5 axis
      {2, {6, 4, 9}, {-1000003, 999999, -17}, {9, 9, 31}, {1, 2, 3}, {8, 7, 28}},  // far starts
  };
  for (const Case& c : smalls) small(c);
  const Case larges[] = {
      // scatter into, and gather around, the last corner of plane 1: offsets past 2^31
      {2, {2, 3, 5}, {0, 0, 0}, {1024, 1024, 1025}, {1022, 1021, 1020}, {2, 3, 5}},
      {2, {1024, 1024, 1025}, {1022, 1021, 1020}, {4, 6, 10}, {0, 0, 0}, {4, 6, 10}},
      {2, {1024, 1024, 1025}, {-3, -2, -5}, {1030, 1029, 1040}, {0, 0, 0}, {1030, 1029, 1040}},
      // a 32-channel stage at 1024^3: offsets past 2^32, up to 3.4e10
      {32, {1024, 1024, 1024}, {-9, 1015, -4}, {146, 146, 146}, {0, 0, 0}, {146, 146, 146}},
      {32, {146, 146, 146}, {9, 9, 9}, {1024, 1024, 1024}, {896, 896, 896}, {128, 128, 128}},
      {32, {1024, 1024, 1024}, {-1024, -2048, 1000}, {1024, 1024, 1024}, {0, 0, 0}, {1024, 1024, 1024}},
  };
  for (const Case& c : larges) large(c);
  if (failures) {
    std::fprintf(stderr, "box_index_check: %d failures\n", failures);
    return 1;
  }
  std::printf("box_index_check: ok (%zu small cases element by element, %zu large cases sampled)\n",
              sizeof(smalls) / sizeof(smalls[0]), sizeof(larges) / sizeof(larges[0]));
  return 0;
}
