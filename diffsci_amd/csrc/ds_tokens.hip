// Token-wise layers of the DiffusionTransformer score network (difftransformer.py): LayerNorm over the embedding axis with adaLN
// modulation, the gated residual, patch embed / unembed, and the MLP's SiLU.  Tensors are fp32, channel-major [B, E, L] with the
// L tokens contiguous -- the layout the 1x1 convolutions and the attention kernels read -- so "a token" is a column of E values
// L floats apart, and every kernel here puts its lanes along L: a wave reads and writes contiguous segments of the rows.
//
// Modulation rows (shift / scale / gate) are slices of a [rows, 6E] table: the caller passes the pointer of the slice for sample 0
// and the stride in floats between samples (0: one row shared by the batch), the convention of ds_gnorm1_apply's FiLM rows.
//
// Everything is HBM-bound: one read and one write of the tensor (two reads for the gate), no matrix cores.  Arithmetic is
// one rounding per operation (-ffp-contract=off), the patch linears are fmaf chains in k order.
#include "ds_common.h"
#include "ds_stream.h"

namespace {

using ds::f32x4;
using ds::silu;
using ds::wave_commit_max_always;
constexpr int NT = 256;

// ---- LayerNorm(E) + adaLN modulation ------------------------------------------------------------------------------------------
// A workgroup owns 32 consecutive tokens of one sample: TX = 32 / VEC lanes along the tokens (VEC = 4: 16-byte loads, L % 4 == 0;
// VEC = 1 otherwise), TY = 256 / TX groups across the channels, thread (tx, ty) holding rows ty, ty + TY, ... in registers (NR of
// them: the tensor is read once).  Statistics are centred in two steps.  The token's first channel K = x[b, 0, l] is a pivot only
// for a first estimate of the mean, m1 = fl(K + sum(x - K) / E); the registers then hold d = x - m1 instead of x, mean - m1 =
// sum(d) / E, and var = sum((d - (mean - m1))^2) / E in a last pass over the registers -- no E[x^2] - mean^2, and the deviations are
// never rounded to the magnitude of x: a token at 1e4 +- 1 keeps its 24 bits of the +- 1 (m1 is within a deviation of the mean, so
// x - m1 is exact there).  Holding x - K itself would round every channel to ulp(K), which is ruinous when channel 0 is an outlier
// (a "massive activation" of 1e6 among values of order one); m1 is off by at most the rounding of x - K averaged over E, and
// x - m1 is rounded at the ulp of the deviation itself, the floor of any fp32 LayerNorm.  Each of the three
// reductions is a pairwise tree in a fixed order: the thread's NR terms by halves (tree_rows; a running sum of 64 or 128 terms
// loses what a dominant first term's ulp hides from every later one), a butterfly over the TY groups of the wave, the four waves
// through LDS -- the result is the same bits from run to run.
template <int LO, int N, class F>
__device__ __forceinline__ float tree_rows(const F& term) {       // term(LO) + ... + term(LO + N - 1), N a power of two
  if constexpr (N == 1) return term(LO);
  else return tree_rows<LO, N / 2>(term) + tree_rows<LO + N / 2, N / 2>(term);
}

template <int VEC, int NR>
__global__ __launch_bounds__(NT) void k_token_ln(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ w,
                                                 const float* __restrict__ bias, const float* __restrict__ mscale,
                                                 const float* __restrict__ mshift, int mstride, int E, int L, float eps,
                                                 unsigned* __restrict__ out_amax) {
  constexpr int TX = 32 / VEC, TY = NT / TX;
  __shared__ float red[3][4][32];
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int l0 = blockIdx.x * 32 + tx * VEC;
  const bool live = l0 < L;                              // VEC = 4: L % 4 == 0, so a group of four tokens is whole or absent
  const float* xb = x + (size_t)b * E * L + l0;
  float d[NR][VEC], K[VEC], s[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) K[j] = 0.f;
  if (live) {
    if constexpr (VEC == 4) {
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(xb);
      K[0] = k4.x, K[1] = k4.y, K[2] = k4.z, K[3] = k4.w;
    } else {
      K[0] = xb[0];
    }
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int e = ty + r * TY;
#pragma unroll
    for (int j = 0; j < VEC; ++j) d[r][j] = K[j];        // rows past E and dead tokens add x - K = 0
    if (live && e < E) {
      if constexpr (VEC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xb + (size_t)e * L);
        d[r][0] = v.x, d[r][1] = v.y, d[r][2] = v.z, d[r][3] = v.w;
      } else {
        d[r][0] = xb[(size_t)e * L];
      }
    }
  }
  const float inv_e = 1.0f / (float)E;
  float dm[VEC], rstd[VEC];
#pragma unroll
  for (int pass = 0; pass < 3; ++pass) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if (pass == 0) {
        s[j] = tree_rows<0, NR>([&](int r) { return d[r][j] - K[j]; });
      } else if (pass == 1) {                            // dm holds m1 here: the registers now hold x - m1, 0 in the rows past E
#pragma unroll
        for (int r = 0; r < NR; ++r) d[r][j] = ty + r * TY < E ? d[r][j] - dm[j] : 0.f;
        s[j] = tree_rows<0, NR>([&](int r) { return d[r][j]; });
      } else {
        s[j] = tree_rows<0, NR>([&](int r) {
          const float c = d[r][j] - dm[j];
          return ty + r * TY < E ? c * c : 0.f;
        });
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
#pragma unroll
      for (int o = TX; o < 64; o <<= 1) s[j] += __shfl_xor(s[j], o, 64);
    }
    if ((threadIdx.x & 63) < TX) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) red[pass][wave][tx * VEC + j] = s[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int t = tx * VEC + j;
      const float tot = ((red[pass][0][t] + red[pass][1][t]) + red[pass][2][t]) + red[pass][3][t];
      if (pass == 0) dm[j] = K[j] + tot * inv_e;         // m1
      else if (pass == 1) dm[j] = tot * inv_e;           // mean - m1
      else rstd[j] = 1.0f / sqrtf(tot * inv_e + eps);
    }
  }
  float amax = 0.f;
  if (live) {
    float* ob = out + (size_t)b * E * L + l0;
    const float* sc = mscale ? mscale + (size_t)b * mstride : nullptr;
    const float* sh = mshift ? mshift + (size_t)b * mstride : nullptr;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int e = ty + r * TY;
      if (e < E) {
        const float we = w ? w[e] : 1.0f, be = bias ? bias[e] : 0.f;
        const float one_sc = 1.0f + (sc ? sc[e] : 0.f), she = sh ? sh[e] : 0.f;
        float y[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float n = ((d[r][j] - dm[j]) * rstd[j]) * we + be;
          y[j] = n * one_sc + she;
          amax = fmaxf(amax, __builtin_fabsf(y[j]));
        }
        if constexpr (VEC == 4) {
          f32x4 v;
          v.x = y[0], v.y = y[1], v.z = y[2], v.w = y[3];
          *reinterpret_cast<f32x4*>(ob + (size_t)e * L) = v;
        } else {
          ob[(size_t)e * L] = y[0];
        }
      }
    }
  }
  if (out_amax) wave_commit_max_always(out_amax + b, amax);
}

// ---- gated residual: out = x + gate[b, e] * y (a rounded product, then a rounded sum) -------------------------------------------
// One row (b, e) of L floats per group of `tpr` threads (a power of two <= 256 chosen on the host from L), 256 / tpr rows per block.
template <int VEC>
__global__ __launch_bounds__(NT) void k_token_gate(float* out, const float* x, const float* __restrict__ y,
                                                   const float* __restrict__ gate, int gstride, int rows, int E, int L, int tpr_log2) {
  const int tpr = 1 << tpr_log2;
  const int row = blockIdx.x * (NT >> tpr_log2) + (threadIdx.x >> tpr_log2);
  if (row >= rows) return;
  const int b = row / E, e = row - b * E;
  const float g = gate[(size_t)b * gstride + e];
  const size_t base = (size_t)row * L;
  for (int c = (threadIdx.x & (tpr - 1)) * VEC; c < L; c += tpr * VEC) {
    if constexpr (VEC == 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(x + base + c);
      const f32x4 yv = *reinterpret_cast<const f32x4*>(y + base + c);
      f32x4 o;
      o.x = xv.x + g * yv.x, o.y = xv.y + g * yv.y, o.z = xv.z + g * yv.z, o.w = xv.w + g * yv.w;
      *reinterpret_cast<f32x4*>(out + base + c) = o;
    } else {
      out[base + c] = x[base + c] + g * y[base + c];
    }
  }
}

// ---- SiLU of [B, n] with the per-sample max |out| (the MLP's hidden layer feeds an fp16x3 launch) ------------------------------
template <int VEC>
__global__ __launch_bounds__(NT) void k_silu_amax(float* out, const float* x, size_t n, unsigned* __restrict__ out_amax) {
  const size_t base = (size_t)blockIdx.y * n;
  float m = 0.f;
  for (size_t i = ((size_t)blockIdx.x * NT + threadIdx.x) * VEC; i < n; i += (size_t)gridDim.x * NT * VEC) {
    if constexpr (VEC == 4) {
      f32x4 v = *reinterpret_cast<const f32x4*>(x + base + i);
      v.x = silu(v.x), v.y = silu(v.y), v.z = silu(v.z), v.w = silu(v.w);
      m = fmaxf(m, fmaxf(fmaxf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)), fmaxf(__builtin_fabsf(v.z), __builtin_fabsf(v.w))));
      *reinterpret_cast<f32x4*>(out + base + i) = v;
    } else {
      const float v = silu(x[base + i]);
      m = fmaxf(m, __builtin_fabsf(v));
      out[base + i] = v;
    }
  }
  if (out_amax) wave_commit_max_always(out_amax + blockIdx.y, m);
}

// ---- patch embed: out[b, e, l] = bias[e] + sum_k W[e, k] * x[b, c, h p + p1, w p + p2], k = (c p + p1) p + p2, l = h Wp + w -----
// One thread per token (tokens of the whole batch flattened, so small L still fills the waves) and 16 output channels per
// workgroup row: the K patch values are gathered once per thread (the input is E / K times smaller than the output and stays in
// cache), the 16 accumulators are fmaf chains in k order, W is read through wave-uniform addresses, stores are contiguous along l.
constexpr int EC = 16;
__global__ __launch_bounds__(NT) void k_patch_embed(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ W,
                                                    const float* __restrict__ bias, int B, int C, int H, int Wd, int p, int E) {
  const int Hp = H / p, Wp = Wd / p, L = Hp * Wp, K = C * p * p;
  const long long g = (long long)blockIdx.x * NT + threadIdx.x;
  if (g >= (long long)B * L) return;
  const int b = (int)(g / L), l = (int)(g - (long long)b * L);
  const int h = l / Wp, wq = l - h * Wp;
  const int e0 = blockIdx.y * EC;
  const float* xb = x + ((size_t)b * C * H + (size_t)h * p) * Wd + (size_t)wq * p;
  float acc[EC];
#pragma unroll
  for (int j = 0; j < EC; ++j) acc[j] = 0.f;
  int k = 0;
  for (int c = 0; c < C; ++c)
    for (int p1 = 0; p1 < p; ++p1)
      for (int p2 = 0; p2 < p; ++p2, ++k) {
        const float v = xb[((size_t)c * H + p1) * Wd + p2];
#pragma unroll
        for (int j = 0; j < EC; ++j) {
          const int e = e0 + j < E ? e0 + j : E - 1;
          acc[j] = fmaf(W[(size_t)e * K + k], v, acc[j]);
        }
      }
#pragma unroll
  for (int j = 0; j < EC; ++j) {
    const int e = e0 + j;
    if (e < E) out[((size_t)b * E + e) * L + l] = acc[j] + (bias ? bias[e] : 0.f);
  }
}

// ---- patch unembed: y[b, c, h p + p1, w p + p2] = bias[k] + sum_e W[k, e] * x[b, e, l], written as NCHW ------------------------------
// 64 tokens per workgroup (flattened over the batch), the E axis split over its four waves: wave g runs the fmaf chains of its
// quarter of the channels for 16 outputs k per token (blockIdx.y: chunks of 16 k; K = 16 at the defaults, so x is read once), the
// four partial sums meet in LDS and are added in wave order, then the bias.  Reads are contiguous along l; the writes are the
// scatter into the image (p floats apart across lanes), a K / E fraction of the traffic.
constexpr int KC = 16;
__global__ __launch_bounds__(NT) void k_patch_unembed(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ W,
                                                      const float* __restrict__ bias, int B, int C, int H, int Wd, int p, int E) {
  __shared__ float red[4][KC][64];
  const int Hp = H / p, Wp = Wd / p, L = Hp * Wp, K = C * p * p;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long g = (long long)blockIdx.x * 64 + lane;
  const bool live = g < (long long)B * L;
  const int b = live ? (int)(g / L) : 0, l = live ? (int)(g - (long long)b * L) : 0;
  const int k0 = blockIdx.y * KC;
  const int eq = (E + 3) / 4, ea = wave * eq, eb = ea + eq < E ? ea + eq : E;
  float acc[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) acc[j] = 0.f;
  if (live) {
    const float* xb = x + (size_t)b * E * L + l;
    for (int e = ea; e < eb; ++e) {
      const float v = xb[(size_t)e * L];
#pragma unroll
      for (int j = 0; j < KC; ++j) {
        const int k = k0 + j < K ? k0 + j : K - 1;
        acc[j] = fmaf(W[(size_t)k * E + e], v, acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < KC; ++j) red[wave][j][lane] = acc[j];
  __syncthreads();
  if (!live) return;
  const int h = l / Wp, wq = l - h * Wp;
  for (int j = wave; j < KC; j += 4) {
    const int k = k0 + j;
    if (k >= K) break;
    const float v = (((red[0][j][lane] + red[1][j][lane]) + red[2][j][lane]) + red[3][j][lane]) + (bias ? bias[k] : 0.f);
    const int c = k / (p * p), r = k - c * p * p, p1 = r / p, p2 = r - p1 * p;
    y[(((size_t)b * C + c) * H + (size_t)h * p + p1) * Wd + (size_t)wq * p + p2] = v;
  }
}

template <int VEC>
int launch_ln(float* out, const float* x, const float* w, const float* b, const float* sc, const float* sh, int stride, int B, int E,
              int L, float eps, unsigned* out_amax, hipStream_t st) {
  constexpr int TY = NT / (32 / VEC);
  const int nr = (E + TY - 1) / TY;
  const dim3 grid((unsigned)((L + 31) / 32), (unsigned)B);
#define DS_LN_CASE(N)                                                                                                       \
  if (nr <= N) {                                                                                                            \
    hipLaunchKernelGGL((k_token_ln<VEC, N>), grid, dim3(NT), 0, st, out, x, w, b, sc, sh, stride, E, L, eps, out_amax);        \
    return DS_OK;                                                                                                           \
  }
  DS_LN_CASE(2)
  DS_LN_CASE(4)
  DS_LN_CASE(8)
  DS_LN_CASE(16)
  DS_LN_CASE(32)
  if constexpr (VEC == 1) {
    DS_LN_CASE(64)
    DS_LN_CASE(128)
  }
#undef DS_LN_CASE
  return DS_ERR_UNSUPPORTED;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

bool patch_shape_ok(int B, int C, int H, int W, int p, int E) {
  return B >= 0 && C > 0 && H > 0 && W > 0 && p > 0 && E > 0 && H % p == 0 && W % p == 0 && (long long)C * p * p < (1 << 20) &&
         (long long)B * C * H * W < ((long long)1 << 40);
}

}  // namespace

extern "C" {

int ds_token_layernorm(float* out, const float* x, const float* w, const float* b, const float* mod_scale, const float* mod_shift,
                       int mod_stride, int B, int E, int L, float eps, unsigned* out_amax, void* stream) {
  DS_REQUIRE(out && x, DS_ERR_NULL, "ds_token_layernorm: NULL pointer");
  DS_REQUIRE(B >= 0 && B < 65536 && E > 0 && L > 0, DS_ERR_SHAPE, "ds_token_layernorm: bad shape B=%d E=%d L=%d", B, E, L);
  DS_REQUIRE(E <= 1024, DS_ERR_UNSUPPORTED, "ds_token_layernorm: E=%d: a token's channels are held in registers, E <= 1024", E);
  DS_REQUIRE(mod_stride >= 0, DS_ERR_SHAPE, "ds_token_layernorm: mod_stride=%d", mod_stride);
  if (B == 0) return DS_OK;
  hipStream_t st = ds::as_stream(stream);
  const bool vec = L % 4 == 0 && aligned16(out) && aligned16(x);
  const int rc = vec ? launch_ln<4>(out, x, w, b, mod_scale, mod_shift, mod_stride, B, E, L, eps, out_amax, st)
                     : launch_ln<1>(out, x, w, b, mod_scale, mod_shift, mod_stride, B, E, L, eps, out_amax, st);
  DS_REQUIRE(rc == DS_OK, rc, "ds_token_layernorm: no kernel for E=%d", E);
  DS_CHECK_LAUNCH("ds_token_layernorm");
  return DS_OK;
}

int ds_token_gate(float* out, const float* x, const float* y, const float* gate, int gate_stride, int B, int E, int L, void* stream) {
  DS_REQUIRE(out && x && y && gate, DS_ERR_NULL, "ds_token_gate: NULL pointer");
  DS_REQUIRE(B >= 0 && E > 0 && L > 0 && (long long)B * E < ((long long)1 << 31), DS_ERR_SHAPE, "ds_token_gate: bad shape B=%d E=%d L=%d",
             B, E, L);
  DS_REQUIRE(gate_stride >= 0, DS_ERR_SHAPE, "ds_token_gate: gate_stride=%d", gate_stride);
  if (B == 0) return DS_OK;
  const bool vec = L % 4 == 0 && aligned16(out) && aligned16(x) && aligned16(y);
  const int per = vec ? (L + 3) / 4 : L;          // threads a row can use
  int tl = 0;
  while (tl < 8 && (1 << tl) < per) ++tl;
  const int rows = B * E, rpb = NT >> tl;
  const dim3 grid((unsigned)((rows + rpb - 1) / rpb));
  if (vec) hipLaunchKernelGGL(k_token_gate<4>, grid, dim3(NT), 0, ds::as_stream(stream), out, x, y, gate, gate_stride, rows, E, L, tl);
  else hipLaunchKernelGGL(k_token_gate<1>, grid, dim3(NT), 0, ds::as_stream(stream), out, x, y, gate, gate_stride, rows, E, L, tl);
  DS_CHECK_LAUNCH("ds_token_gate");
  return DS_OK;
}

int ds_silu_amax(float* out, const float* x, int B, size_t n_per_sample, unsigned* out_amax, void* stream) {
  DS_REQUIRE(out && x, DS_ERR_NULL, "ds_silu_amax: NULL pointer");
  DS_REQUIRE(B >= 0 && B < 65536, DS_ERR_SHAPE, "ds_silu_amax: B=%d", B);
  if (B == 0 || n_per_sample == 0) return DS_OK;
  const bool vec = n_per_sample % 4 == 0 && aligned16(out) && aligned16(x);
  size_t per = (n_per_sample + (size_t)NT * 16 - 1) / ((size_t)NT * 16);
  const size_t want = (size_t)4096 / (size_t)B + 1;
  if (per > want) per = want;
  const dim3 grid((unsigned)per, (unsigned)B);
  if (vec) hipLaunchKernelGGL(k_silu_amax<4>, grid, dim3(NT), 0, ds::as_stream(stream), out, x, n_per_sample, out_amax);
  else hipLaunchKernelGGL(k_silu_amax<1>, grid, dim3(NT), 0, ds::as_stream(stream), out, x, n_per_sample, out_amax);
  DS_CHECK_LAUNCH("ds_silu_amax");
  return DS_OK;
}

int ds_patch_embed(float* out, const float* x, const float* w, const float* bias, int B, int C, int H, int W, int patch, int E,
                   void* stream) {
  DS_REQUIRE(out && x && w, DS_ERR_NULL, "ds_patch_embed: NULL pointer");
  DS_REQUIRE(patch_shape_ok(B, C, H, W, patch, E), DS_ERR_SHAPE, "ds_patch_embed: bad shape B=%d C=%d H=%d W=%d patch=%d E=%d", B, C, H, W,
             patch, E);
  DS_REQUIRE((E + EC - 1) / EC < 65536, DS_ERR_SHAPE, "ds_patch_embed: E=%d exceeds grid.y", E);
  if (B == 0) return DS_OK;
  const long long tokens = (long long)B * (H / patch) * (W / patch);
  const dim3 grid((unsigned)((tokens + NT - 1) / NT), (unsigned)((E + EC - 1) / EC));
  hipLaunchKernelGGL(k_patch_embed, grid, dim3(NT), 0, ds::as_stream(stream), out, x, w, bias, B, C, H, W, patch, E);
  DS_CHECK_LAUNCH("ds_patch_embed");
  return DS_OK;
}

int ds_patch_unembed(float* y, const float* x, const float* w, const float* bias, int B, int C, int H, int W, int patch, int E,
                     void* stream) {
  DS_REQUIRE(y && x && w, DS_ERR_NULL, "ds_patch_unembed: NULL pointer");
  DS_REQUIRE(patch_shape_ok(B, C, H, W, patch, E), DS_ERR_SHAPE, "ds_patch_unembed: bad shape B=%d C=%d H=%d W=%d patch=%d E=%d", B, C, H,
             W, patch, E);
  const int K = C * patch * patch;
  DS_REQUIRE((K + KC - 1) / KC < 65536, DS_ERR_SHAPE, "ds_patch_unembed: C * patch^2 = %d exceeds grid.y", K);
  if (B == 0) return DS_OK;
  const long long tokens = (long long)B * (H / patch) * (W / patch);
  const dim3 grid((unsigned)((tokens + 63) / 64), (unsigned)((K + KC - 1) / KC));
  hipLaunchKernelGGL(k_patch_unembed, grid, dim3(NT), 0, ds::as_stream(stream), y, x, w, bias, B, C, H, W, patch, E);
  DS_CHECK_LAUNCH("ds_patch_unembed");
  return DS_OK;
}

}  // extern "C"
