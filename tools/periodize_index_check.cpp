// Host check of diffsci_amd/csrc/ds_periodize.h, the offset arithmetic of ds_crop_blend: built with the host compiler, no GPU.
//
//     c++ -std=c++17 -O1 -Wall -ffp-contract=off -fsanitize=address,undefined -o /tmp/pz_check tools/periodize_index_check.cpp
//     /tmp/pz_check
//
// The header's offsets (32-bit axis indices, Horner products in size_t) are compared with an independent restatement: 128-bit
// integers, strides multiplied out.
//   1. small cases, every element: the offsets, and the whole crop-and-blend replayed on host arrays through the header's depth /
//      mirror / width functions (recursively, as the kernel reads) against the reference's own sequence -- crop into a copy, then
//      per axis form both strips from the pre-blend values and assign them -- in the same fp32 operations, so the two must agree
//      bit for bit: skipped axes (width 0, 2 bw == A, 2 bw > A), strips that meet around one centre element, pads of 0;
//   2. large tensors, sampled elements: offsets past 2^31 and past 2^32, each of which must also stay inside its tensor.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../diffsci_amd/csrc/ds_periodize.h"

typedef __int128 i128;

struct Case {
  int planes, A[3], p[3], bw[3];
};

static int failures = 0;

static void expect(bool ok, const char* what, const Case& c, long long n, long long i, long long j, long long k) {
  if (ok) return;
  if (++failures <= 10)
    std::fprintf(stderr, "FAIL %s: A=(%d,%d,%d) p=(%d,%d,%d) at n=%lld i=%lld j=%lld k=%lld\n", what, c.A[0], c.A[1], c.A[2], c.p[0],
                 c.p[1], c.p[2], n, i, j, k);
}

static ds_periodize_geom geom(const Case& c) {
  return ds_periodize_make_geom(c.A[0], c.A[1], c.A[2], c.p[0], c.p[1], c.p[2], c.bw[0], c.bw[1], c.bw[2]);
}

static void check_element(const Case& c, const ds_periodize_geom& g, long long n, long long i, long long j, long long k) {
  const i128 E0 = (i128)c.A[0] + 2 * (i128)c.p[0], E1 = (i128)c.A[1] + 2 * (i128)c.p[1], E2 = (i128)c.A[2] + 2 * (i128)c.p[2];
  const i128 want_src = n * (E0 * E1 * E2) + (c.p[0] + i) * (E1 * E2) + (c.p[1] + j) * E2 + (c.p[2] + k);
  const i128 want_dst = n * ((i128)c.A[0] * c.A[1] * c.A[2]) + i * ((i128)c.A[1] * c.A[2]) + j * (i128)c.A[2] + k;
  const size_t got_src = ds_periodize_src(g, (uint32_t)n, (uint32_t)i, (uint32_t)j, (uint32_t)k);
  uint32_t gi, gj;
  const size_t got_dst = ds_periodize_dst_row(g, (uint32_t)n, (uint32_t)(i * c.A[1] + j), &gi, &gj) + (size_t)k;
  expect((i128)got_src == want_src, "source offset", c, n, i, j, k);
  expect((i128)got_dst == want_dst, "destination offset", c, n, i, j, k);
  expect(gi == (uint32_t)i && gj == (uint32_t)j, "row coordinates", c, n, i, j, k);
  expect((i128)got_src < E0 * E1 * E2 * c.planes, "source offset inside y", c, n, i, j, k);
  expect((i128)got_dst < (i128)c.A[0] * c.A[1] * c.A[2] * c.planes, "destination offset inside out", c, n, i, j, k);
  // the mirrored partners the blend reads lie inside the crop as well
  expect(ds_periodize_mirror(g.A0, (uint32_t)i) < g.A0 && ds_periodize_mirror(g.A1, (uint32_t)j) < g.A1 &&
             ds_periodize_mirror(g.A2, (uint32_t)k) < g.A2, "mirror inside the axis", c, n, i, j, k);
}

static float blend(float w, float a, float b) {
  const float wa = w * a, om = 1.0f - w;
  const float ob = om * b;
  return wa + ob;
}

// the kernel's reading order, through the header
struct Reader {
  const ds_periodize_geom& g;
  const std::vector<float>& y;
  const std::vector<float>* w;
  float axis0(uint32_t n, uint32_t i, uint32_t j, uint32_t k) const {
    const float v = y.at(ds_periodize_src(g, n, i, j, k));
    const uint32_t m = ds_periodize_depth(g.A0, i);
    return m >= g.bw0 ? v : blend(w[0].at(m), v, y.at(ds_periodize_src(g, n, ds_periodize_mirror(g.A0, i), j, k)));
  }
  float axis1(uint32_t n, uint32_t i, uint32_t j, uint32_t k) const {
    const float v = axis0(n, i, j, k);
    const uint32_t m = ds_periodize_depth(g.A1, j);
    return m >= g.bw1 ? v : blend(w[1].at(m), v, axis0(n, i, ds_periodize_mirror(g.A1, j), k));
  }
  float axis2(uint32_t n, uint32_t i, uint32_t j, uint32_t k) const {
    const float v = axis1(n, i, j, k);
    const uint32_t m = ds_periodize_depth(g.A2, k);
    return m >= g.bw2 ? v : blend(w[2].at(m), v, axis1(n, i, j, ds_periodize_mirror(g.A2, k)));
  }
};

// every element of a small case, then the crop and blend on host arrays
static void small(const Case& c) {
  const ds_periodize_geom g = geom(c);
  const long long E[3] = {c.A[0] + 2ll * c.p[0], c.A[1] + 2ll * c.p[1], c.A[2] + 2ll * c.p[2]};
  const size_t ny = (size_t)c.planes * E[0] * E[1] * E[2], no = (size_t)c.planes * c.A[0] * c.A[1] * c.A[2];
  std::vector<float> y(ny), got(no, -7.f), want(no, -7.f), w[3];
  unsigned long long state = 12345;
  for (size_t e = 0; e < ny; ++e) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    y[e] = (float)((long long)(state >> 40) % 2001 - 1000) / 256.0f;
  }
  for (int a = 0; a < 3; ++a)
    for (int t = 0; t < c.bw[a]; ++t) w[a].push_back((float)(0.5 * (1.0 - std::cos(M_PI * (t + 0.5) / c.bw[a]))));
  const Reader r{g, y, w};
  for (long long n = 0; n < c.planes; ++n)
    for (long long i = 0; i < c.A[0]; ++i)
      for (long long j = 0; j < c.A[1]; ++j) {
        uint32_t gi, gj;
        const size_t row = ds_periodize_dst_row(g, (uint32_t)n, (uint32_t)(i * c.A[1] + j), &gi, &gj);
        for (long long k = 0; k < c.A[2]; ++k) {
          check_element(c, g, n, i, j, k);
          got.at(row + k) = r.axis2((uint32_t)n, (uint32_t)i, (uint32_t)j, (uint32_t)k);
          want.at(((n * c.A[0] + i) * c.A[1] + j) * c.A[2] + k) =
              y.at(((n * E[0] + c.p[0] + i) * E[1] + c.p[1] + j) * E[2] + c.p[2] + k);
        }
      }
  // the reference's sequence on the cropped copy: per axis, both strips from the pre-blend values, then assigned
  for (int a = 0; a < 3; ++a) {
    const long long bw = c.bw[a], A = c.A[a];
    if (bw <= 0 || 2 * bw >= A) continue;
    const std::vector<float> before = want;
    const long long stride = a == 0 ? (long long)c.A[1] * c.A[2] : a == 1 ? c.A[2] : 1;
    for (size_t e = 0; e < no; ++e) {
      const long long q = (long long)(e / stride) % A;
      if (q < bw)
        want[e] = blend(w[a][q], before[e], before[e + (A - 1 - 2 * q) * stride]);
      else if (q >= A - bw)
        want[e] = blend(w[a][A - 1 - q], before[e], before[e - (2 * q - (A - 1)) * stride]);
    }
  }
  if (std::memcmp(got.data(), want.data(), no * sizeof(float)) != 0) {
    ++failures;
    std::fprintf(stderr, "FAIL crop-and-blend replay: A=(%d,%d,%d) bw=(%d,%d,%d)\n", c.A[0], c.A[1], c.A[2], c.bw[0], c.bw[1], c.bw[2]);
  }
}

// the corners and a pseudo-random sample of a large case
static void large(const Case& c) {
  const ds_periodize_geom g = geom(c);
  unsigned long long state = 0x9E3779B97F4A7C15ull;
  auto next = [&](long long m) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (long long)((state >> 33) % (unsigned long long)m);
  };
  for (long long n : {0ll, (long long)c.planes - 1})
    for (long long i : {0ll, (long long)c.A[0] - 1})
      for (long long j : {0ll, (long long)c.A[1] - 1})
        for (long long k : {0ll, (long long)c.A[2] - 1}) check_element(c, g, n, i, j, k);
  for (int t = 0; t < 200000; ++t) check_element(c, g, next(c.planes), next(c.A[0]), next(c.A[1]), next(c.A[2]));
}

int main() {
  // the skip rule
  const long long rule[][3] = {{9, 4, 4}, {8, 4, 0}, {8, 3, 3}, {7, 4, 0}, {5, 0, 0}, {5, -2, 0}, {1, 1, 0}, {3, 1, 1}};
  for (const auto& r : rule)
    if (ds_periodize_width(r[0], r[1]) != (uint32_t)r[2]) {
      ++failures;
      std::fprintf(stderr, "FAIL ds_periodize_width(%lld, %lld)\n", r[0], r[1]);
    }
  const Case smalls[] = {
      {2, {5, 6, 7}, {2, 0, 3}, {2, 1, 3}},        // three active axes: 8-input corners
      {2, {4, 4, 8}, {2, 2, 2}, {2, 2, 3}},        // 2 bw == A on two axes: skipped
      {3, {1, 6, 7}, {0, 1, 2}, {0, 2, 3}},        // a field
      {2, {1, 5, 9}, {0, 0, 0}, {0, 4, 4}},        // 2 bw > A skipped; 2 bw = 8 < 9: the strips meet around one centre column
      {1, {8, 8, 8}, {4, 4, 4}, {0, 0, 0}},        // a pure crop
      {2, {3, 5, 4}, {5, 0, 1}, {1, 2, 1}},        // a pad longer than the axis
  };
  for (const Case& c : smalls) small(c);
  const Case larges[] = {
      {2, {1024, 1024, 1025}, {3, 2, 5}, {8, 8, 8}},             // offsets past 2^31 in out, and in y
      {4, {1, 30000, 30001}, {0, 64, 64}, {0, 8, 8}},            // a field: 3.6e9 elements
      {32, {960, 960, 960}, {32, 32, 32}, {8, 8, 8}},            // a 32-channel volume expanded to 1024^3: past 2^32, up to 3.4e10
      {3, {1024, 1024, 1024}, {0, 0, 512}, {16, 0, 511}},        // one pad only
  };
  for (const Case& c : larges) large(c);
  if (failures) {
    std::fprintf(stderr, "periodize_index_check: %d failures\n", failures);
    return 1;
  }
  std::printf("periodize_index_check: ok (%zu small cases element by element, %zu large cases sampled)\n",
              sizeof(smalls) / sizeof(smalls[0]), sizeof(larges) / sizeof(larges[0]));
  return 0;
}
