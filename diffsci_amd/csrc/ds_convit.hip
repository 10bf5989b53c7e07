// Streaming layers of the ConVit score network (convit.py): the per-pixel channel RMS norm with its embedding row and the
// average pooling in front of the attention, RoPE on the pooled grid, bilinear upsampling, the depthwise convolution + SiLU, the
// SwiGLU gate and the fusion blend.  Tensors are fp32 [B, E, H, W] (channel-major: a pixel's channels are H*W floats apart), so
// every kernel puts its lanes along the pixels, as ds_tokens.hip does along the tokens.
//
// Streaming kernels: one read and one write of the tensor, no matrix cores.  Arithmetic is one rounding per operation
// (-ffp-contract=off); the depthwise taps are an fmaf chain in (dy, dx) order.  Kernels whose result feeds an fp16x3 launch merge
// the per-sample max |out| into zeroed int32 slots (float bits), the convention of ds_conv_epilogue.h, through
// ds::wave_commit_max_if_greater (ds_stream.h), which skips the atomic when the slot already covers the wave's maximum: an
// unconditional atomicMax per wave on the sample's one address serialises in L2 and bounded every one of these kernels
// (DESIGN 4.19).
//
// Every entry point closes its argument list with a flags word after the stream (none are defined: pass 0).
#include "ds_common.h"
#include "ds_stream.h"

namespace {

using ds::amax4;
using ds::f32x4;
using ds::silu;
using ds::wave_commit_max_if_greater;
constexpr int NT = 256;

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// grid.x of a grid-stride kernel over `items` work items of one sample (grid.y = B): enough blocks to fill the chip, no more
unsigned stream_blocks(size_t items, int B) {
  size_t per = (items + (size_t)NT * 4 - 1) / ((size_t)NT * 4);
  const size_t want = (size_t)4096 / (size_t)(B > 0 ? B : 1) + 1;
  if (per > want) per = want;
  return (unsigned)(per ? per : 1);
}

// ---- ChannelRMSNorm + embedding row (+ AvgPool2d(f)) ---------------------------------------------------------------------------
// out = x / sqrt(mean_c(x^2) + eps) * w[c] + mod[b, c], then the mean over f x f pixels when f > 1.  The layout of k_token_ln:
// a workgroup owns 32 pixels of one sample, TX = 32 / VEC lanes along them (VEC = 4: 16-byte accesses, f = 1, H*W % 4 == 0),
// TY = 256 / TX groups across the channels, thread (tx, ty) holding channels ty, ty + TY, ... in registers -- the tensor is read
// once.  Partial sums of squares: NR terms in the thread, a butterfly over the TY groups of the wave, the four waves through LDS in
// a fixed order.
// f > 1 (VEC = 1, f = 2 or 4): the 32 pixels are 32 / f^2 output pixels of one output row, the f^2 inputs of an output pixel on
// consecutive lanes (lane = o * f^2 + dy * f + dx), so the pooling is a butterfly over f^2 lanes of normalised values that never
// leave the registers; lane dy = dx = 0 writes.  f = 1 is the same map with the image taken as one row of H*W pixels.
template <int VEC, int NR>
__global__ __launch_bounds__(NT) void k_channel_rms(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ mod, int mstride, int E, int H, int W, int lf, float eps,
                                                    unsigned* __restrict__ out_amax) {
  constexpr int TX = 32 / VEC, TY = NT / TX;
  __shared__ float red[4][32];
  const int tx = threadIdx.x % TX, ty = threadIdx.x / TX, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int f = 1 << lf, f2 = f * f;
  const int OW = W >> lf, OH = H >> lf;
  const int opb = 32 >> (2 * lf);                       // output pixels of a workgroup
  const int tpr = (OW + opb - 1) / opb;                 // workgroups per output row
  const int oy = blockIdx.x / tpr, tile = blockIdx.x - oy * tpr;
  const int q = (tx * VEC) & (f2 - 1), dy = q >> lf, dx = q & (f - 1);
  const int ox = tile * opb + ((tx * VEC) >> (2 * lf));
  const bool live = ox < OW;                            // VEC = 4: f = 1 and OW % 4 == 0, so a group of four pixels is whole or absent
  const size_t HW = (size_t)H * W;
  const float* xb = x + (size_t)b * E * HW + (size_t)(oy * f + dy) * W + (size_t)ox * f + dx;
  float v[NR][VEC], s[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s[j] = 0.f;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int e = ty + r * TY;
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[r][j] = 0.f;
    if (live && e < E) {
      if constexpr (VEC == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(xb + (size_t)e * HW);
        v[r][0] = t.x, v[r][1] = t.y, v[r][2] = t.z, v[r][3] = t.w;
      } else {
        v[r][0] = xb[(size_t)e * HW];
      }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] += v[r][j] * v[r][j];
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
#pragma unroll
    for (int o = TX; o < 64; o <<= 1) s[j] += __shfl_xor(s[j], o, 64);
  }
  if ((threadIdx.x & 63) < TX) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) red[wave][tx * VEC + j] = s[j];
  }
  __syncthreads();
  float norm[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int t = tx * VEC + j;
    const float tot = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    norm[j] = sqrtf(tot / (float)E + eps);
  }
  float amax = 0.f;
  float* ob = out + (size_t)b * E * OH * OW + (size_t)oy * OW + ox;
  const float* mb = mod ? mod + (size_t)b * mstride : nullptr;
  const float inv = 1.0f / (float)f2;
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int e = ty + r * TY;
    const bool on = live && e < E;
    const float we = (on && w) ? w[e] : 1.0f, me = (on && mb) ? mb[e] : 0.f;
    float y[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      y[j] = v[r][j] / norm[j];
      if (w) y[j] = y[j] * we;
      if (mb) y[j] = y[j] + me;
    }
    if constexpr (VEC == 1) {
      if (lf > 0) {                                      // every lane of the wave takes part: dead lanes carry zeros
        for (int o = 1; o < f2; o <<= 1) y[0] += __shfl_xor(y[0], o, 64);
        y[0] = y[0] * inv;
      }
    }
    if (on) {
      if constexpr (VEC == 4) {
        f32x4 t;
        t.x = y[0], t.y = y[1], t.z = y[2], t.w = y[3];
        amax = fmaxf(amax, amax4(t));
        *reinterpret_cast<f32x4*>(ob + (size_t)e * OH * OW) = t;
      } else if (q == 0) {
        amax = fmaxf(amax, __builtin_fabsf(y[0]));
        ob[(size_t)e * OH * OW] = y[0];
      }
    }
  }
  if (out_amax) wave_commit_max_if_greater(out_amax + b, amax);
}

template <int VEC>
int launch_rms(float* out, const float* x, const float* w, const float* mod, int mstride, int B, int E, int H, int W, int lf, float eps,
               unsigned* out_amax, hipStream_t st) {
  constexpr int TY = NT / (32 / VEC);
  const int nr = (E + TY - 1) / TY;
  const int OW = W >> lf, OH = H >> lf, opb = 32 >> (2 * lf);
  const long long blocks = (long long)OH * ((OW + opb - 1) / opb);
  if (blocks <= 0 || blocks >= ((long long)1 << 31)) return DS_ERR_SHAPE;
  const dim3 grid((unsigned)blocks, (unsigned)B);
#define DS_RMS_CASE(N)                                                                                                          \
  if (nr <= N) {                                                                                                                \
    hipLaunchKernelGGL((k_channel_rms<VEC, N>), grid, dim3(NT), 0, st, out, x, w, mod, mstride, E, H, W, lf, eps, out_amax);      \
    return DS_OK;                                                                                                               \
  }
  DS_RMS_CASE(2)
  DS_RMS_CASE(4)
  DS_RMS_CASE(8)
  DS_RMS_CASE(16)
  DS_RMS_CASE(32)
  if constexpr (VEC == 1) {
    DS_RMS_CASE(64)
    DS_RMS_CASE(128)
  }
#undef DS_RMS_CASE
  return DS_ERR_UNSUPPORTED;
}

// ---- RoPE on the q and k thirds of qkv [B, 3E, L], in place, and the amax pair of the attention -------------------------------------
// A work row of sample b is a pair of channel rows (2j, 2j + 1), j < E, of the q | k thirds -- rotated by the angle of (position,
// j mod dh/2) -- or one row of the v third, which is only read for its maximum.  `tpr` threads (a power of two chosen on the host
// from L) walk a row; cos_sin [L, dh/2, 2] is read through the caches (it is E / dh times smaller than q | k).
template <int VEC>
__global__ __launch_bounds__(NT) void k_rope2d(float* qkv, const float* __restrict__ cs, int B, int E, int L, int hd2, int tpr_log2,
                                               unsigned* __restrict__ out_amax) {
  const int tpr = 1 << tpr_log2;
  const int row = blockIdx.x * (NT >> tpr_log2) + (threadIdx.x >> tpr_log2);
  const int b = blockIdx.y;
  float mqk = 0.f, mv = 0.f;
  if (row < E) {
    const int i = row % hd2;
    float* pa = qkv + ((size_t)b * 3 * E + 2 * (size_t)row) * L;
    float* pb = pa + L;
    for (int c = (threadIdx.x & (tpr - 1)) * VEC; c < L; c += tpr * VEC) {
      float a[VEC], d[VEC];
      if constexpr (VEC == 4) {
        const f32x4 av = *reinterpret_cast<const f32x4*>(pa + c), dv = *reinterpret_cast<const f32x4*>(pb + c);
        a[0] = av.x, a[1] = av.y, a[2] = av.z, a[3] = av.w;
        d[0] = dv.x, d[1] = dv.y, d[2] = dv.z, d[3] = dv.w;
      } else {
        a[0] = pa[c], d[0] = pb[c];
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float* t = cs + ((size_t)(c + j) * hd2 + i) * 2;
        const float co = t[0], si = t[1];
        const float ra = a[j] * co - d[j] * si, rd = a[j] * si + d[j] * co;
        a[j] = ra, d[j] = rd;
        mqk = fmaxf(mqk, fmaxf(__builtin_fabsf(ra), __builtin_fabsf(rd)));
      }
      if constexpr (VEC == 4) {
        f32x4 av, dv;
        av.x = a[0], av.y = a[1], av.z = a[2], av.w = a[3];
        dv.x = d[0], dv.y = d[1], dv.z = d[2], dv.w = d[3];
        *reinterpret_cast<f32x4*>(pa + c) = av;
        *reinterpret_cast<f32x4*>(pb + c) = dv;
      } else {
        pa[c] = a[0], pb[c] = d[0];
      }
    }
  } else if (row < 2 * E) {
    const float* pv = qkv + ((size_t)b * 3 * E + (size_t)(E + row)) * L;      // row 2E + (row - E)
    for (int c = (threadIdx.x & (tpr - 1)) * VEC; c < L; c += tpr * VEC) {
      if constexpr (VEC == 4) mv = fmaxf(mv, amax4(*reinterpret_cast<const f32x4*>(pv + c)));
      else mv = fmaxf(mv, __builtin_fabsf(pv[c]));
    }
  }
  if (out_amax) {                                       // merged maxima: a wave that saw no row of a kind commits 0
    wave_commit_max_if_greater(out_amax + b, mqk);
    wave_commit_max_if_greater(out_amax + B + b, mv);
  }
}

// ---- F.interpolate(scale_factor=f, mode="bilinear", align_corners=False) of [planes, H, W] ------------------------------------------
// src = max((dst + 0.5) / f - 0.5, 0), lower index floor(src), upper index clamped to the last, weights (1 - t, t); the four taps
// are combined as torch does: hy0 * (wx0 * x00 + wx1 * x01) + hy1 * (wx0 * x10 + wx1 * x11).  A thread writes VEC outputs of a row
// (16-byte stores); the reads are f^2 times fewer than the writes and come through the caches.
__device__ __forceinline__ void src_index(int dst, float rscale, int n, int& i0, int& i1, float& t) {
  const float s = fmaxf(rscale * ((float)dst + 0.5f) - 0.5f, 0.f);
  i0 = (int)s;
  if (i0 > n - 1) i0 = n - 1;
  i1 = i0 < n - 1 ? i0 + 1 : i0;
  t = fminf(fmaxf(s - (float)i0, 0.f), 1.0f);
}

template <int VEC>
__global__ __launch_bounds__(NT) void k_upsample_bilinear(float* __restrict__ out, const float* __restrict__ x, long long planes, int H,
                                                          int W, int f, float rscale) {
  const int OH = H * f, OW = W * f, OWV = OW / VEC;
  const long long total = planes * OH * OWV;
  for (long long g = (long long)blockIdx.x * NT + threadIdx.x; g < total; g += (long long)gridDim.x * NT) {
    const int xq = (int)(g % OWV);
    const long long t = g / OWV;
    const int oy = (int)(t % OH);
    const long long pl = t / OH;
    int y0, y1;
    float ty;
    src_index(oy, rscale, H, y0, y1, ty);
    const float hy1 = ty, hy0 = 1.0f - ty;
    const float* r0 = x + ((size_t)pl * H + y0) * W;
    const float* r1 = x + ((size_t)pl * H + y1) * W;
    float y[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      int x0, x1;
      float tx;
      src_index(xq * VEC + j, rscale, W, x0, x1, tx);
      const float wx1 = tx, wx0 = 1.0f - tx;
      y[j] = hy0 * (wx0 * r0[x0] + wx1 * r0[x1]) + hy1 * (wx0 * r1[x0] + wx1 * r1[x1]);
    }
    float* o = out + ((size_t)pl * OH + oy) * OW + (size_t)xq * VEC;
    if constexpr (VEC == 4) {
      f32x4 v;
      v.x = y[0], v.y = y[1], v.z = y[2], v.w = y[3];
      *reinterpret_cast<f32x4*>(o) = v;
    } else {
      o[0] = y[0];
    }
  }
}

// ---- SiLU(depthwise k x k 'same' convolution + bias) -------------------------------------------------------------------------------------
// A workgroup computes an 8 x 32 tile of one plane (b, e) from its zero-padded halo staged in LDS (read once from memory); a thread
// one output: the k^2 taps as an fmaf chain in (dy, dx) order over LDS (rows of 32 + k - 1 floats: the two 32-lane halves of a
// wave read different rows, no bank conflict inside a half), then the bias, then SiLU.
constexpr int DTH = 8, DTW = 32, DKMAX = 7;
__global__ __launch_bounds__(NT) void k_depthwise_silu(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, int E, int H, int W, int k, int tiles_x,
                                                       int tiles_y, unsigned* __restrict__ out_amax) {
  __shared__ float tile[(DTH + DKMAX - 1) * (DTW + DKMAX - 1)];
  __shared__ float wk[DKMAX * DKMAX];
  const int tiles = tiles_x * tiles_y;
  const long long plane = (long long)blockIdx.x / tiles;
  const int t = (int)((long long)blockIdx.x - plane * tiles);
  const int tyi = t / tiles_x, txi = t - tyi * tiles_x;
  const int e = (int)(plane % E), b = (int)(plane / E);
  const int r = k >> 1, tw = DTW + 2 * r, th = DTH + 2 * r;
  const int y0 = tyi * DTH, x0 = txi * DTW;
  const float* xp = x + (size_t)plane * H * W;
  for (int i = threadIdx.x; i < th * tw; i += NT) {
    const int ly = i / tw, lx = i - ly * tw;
    const int gy = y0 + ly - r, gx = x0 + lx - r;
    tile[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xp[(size_t)gy * W + gx] : 0.f;
  }
  if ((int)threadIdx.x < k * k) wk[threadIdx.x] = w[(size_t)e * k * k + threadIdx.x];
  __syncthreads();
  const int ly = threadIdx.x / DTW, lx = threadIdx.x % DTW;
  const int oy = y0 + ly, ox = x0 + lx;
  float acc = 0.f;
  for (int dy = 0; dy < k; ++dy)
    for (int dx = 0; dx < k; ++dx) acc = fmaf(tile[(ly + dy) * tw + lx + dx], wk[dy * k + dx], acc);
  const float v = silu(acc + (bias ? bias[e] : 0.f));
  float m = 0.f;
  if (oy < H && ox < W) {
    out[(size_t)plane * H * W + (size_t)oy * W + ox] = v;
    m = __builtin_fabsf(v);
  }
  if (out_amax) wave_commit_max_if_greater(out_amax + b, m);
}

// ---- SwiGLU gate: out[b, j] = SiLU(ag[b, j]) * ag[b, n + j], j < n = C * spatial (ag [B, 2C, ...]) ---------------------------------------
template <int VEC>
__global__ __launch_bounds__(NT) void k_swiglu(float* __restrict__ out, const float* __restrict__ ag, size_t n,
                                               unsigned* __restrict__ out_amax) {
  const float* a = ag + (size_t)blockIdx.y * 2 * n;
  const float* g = a + n;
  float* o = out + (size_t)blockIdx.y * n;
  float m = 0.f;
  for (size_t i = ((size_t)blockIdx.x * NT + threadIdx.x) * VEC; i < n; i += (size_t)gridDim.x * NT * VEC) {
    if constexpr (VEC == 4) {
      f32x4 v = *reinterpret_cast<const f32x4*>(a + i);
      const f32x4 u = *reinterpret_cast<const f32x4*>(g + i);
      v.x = silu(v.x) * u.x, v.y = silu(v.y) * u.y, v.z = silu(v.z) * u.z, v.w = silu(v.w) * u.w;
      m = fmaxf(m, amax4(v));
      *reinterpret_cast<f32x4*>(o + i) = v;
    } else {
      const float v = silu(a[i]) * g[i];
      m = fmaxf(m, __builtin_fabsf(v));
      o[i] = v;
    }
  }
  if (out_amax) wave_commit_max_if_greater(out_amax + blockIdx.y, m);
}

// ---- fusion blend: out = ((1 - s) * u + s * xc) + x0, s a device scalar (convit.py:629-631) ------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(NT) void k_blend(float* out, const float* __restrict__ u, const float* __restrict__ xc, const float* x0,
                                              const float* __restrict__ sp, size_t n) {
  const float s = sp[0], c = 1.0f - s;
  for (size_t i = ((size_t)blockIdx.x * NT + threadIdx.x) * VEC; i < n; i += (size_t)gridDim.x * NT * VEC) {
    if constexpr (VEC == 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(u + i), d = *reinterpret_cast<const f32x4*>(xc + i);
      const f32x4 r = *reinterpret_cast<const f32x4*>(x0 + i);
      f32x4 o;
      o.x = (c * a.x + s * d.x) + r.x, o.y = (c * a.y + s * d.y) + r.y, o.z = (c * a.z + s * d.z) + r.z, o.w = (c * a.w + s * d.w) + r.w;
      *reinterpret_cast<f32x4*>(out + i) = o;
    } else {
      out[i] = (c * u[i] + s * xc[i]) + x0[i];
    }
  }
}

}  // namespace

extern "C" {

int ds_channel_rmsnorm(float* out, const float* x, const float* w, const float* mod, int mod_stride, int B, int E, int H, int W, int pool,
                       float eps, unsigned* out_amax, void* stream, int flags) {
  DS_REQUIRE(flags == 0, DS_ERR_SHAPE, "ds_channel_rmsnorm: flags %d (none are defined)", flags);
  DS_REQUIRE(out && x, DS_ERR_NULL, "ds_channel_rmsnorm: NULL pointer");
  DS_REQUIRE(B >= 0 && B < 65536 && E > 0 && H > 0 && W > 0 && (long long)H * W < ((long long)1 << 31), DS_ERR_SHAPE,
             "ds_channel_rmsnorm: bad shape B=%d E=%d H=%d W=%d", B, E, H, W);
  DS_REQUIRE(E <= 1024, DS_ERR_UNSUPPORTED, "ds_channel_rmsnorm: E=%d: a pixel's channels are held in registers, E <= 1024", E);
  DS_REQUIRE(pool == 1 || pool == 2 || pool == 4, DS_ERR_UNSUPPORTED,
             "ds_channel_rmsnorm: pool=%d: the fused pooling takes factors 1, 2 and 4 (pool the result of pool=1 otherwise)", pool);
  DS_REQUIRE(pool <= H && pool <= W, DS_ERR_SHAPE, "ds_channel_rmsnorm: pool=%d exceeds the field %dx%d", pool, H, W);
  DS_REQUIRE(mod_stride >= 0, DS_ERR_SHAPE, "ds_channel_rmsnorm: mod_stride=%d", mod_stride);
  if (B == 0) return DS_OK;
  hipStream_t st = ds::as_stream(stream);
  int rc;
  if (pool == 1) {                                      // the image as one row of H*W pixels
    const int L = H * W;
    const bool vec = L % 4 == 0 && aligned16(out) && aligned16(x);
    rc = vec ? launch_rms<4>(out, x, w, mod, mod_stride, B, E, 1, L, 0, eps, out_amax, st)
             : launch_rms<1>(out, x, w, mod, mod_stride, B, E, 1, L, 0, eps, out_amax, st);
  } else {
    rc = launch_rms<1>(out, x, w, mod, mod_stride, B, E, H, W, pool == 2 ? 1 : 2, eps, out_amax, st);
  }
  DS_REQUIRE(rc == DS_OK, rc, "ds_channel_rmsnorm: no kernel for E=%d H=%d W=%d pool=%d", E, H, W, pool);
  DS_CHECK_LAUNCH("ds_channel_rmsnorm");
  return DS_OK;
}

int ds_rope2d(float* qkv, const float* cos_sin, int B, int E, int heads, int L, unsigned* out_amax, void* stream, int flags) {
  DS_REQUIRE(flags == 0, DS_ERR_SHAPE, "ds_rope2d: flags %d (none are defined)", flags);
  DS_REQUIRE(qkv && cos_sin, DS_ERR_NULL, "ds_rope2d: NULL pointer");
  DS_REQUIRE(B >= 0 && B < 65536 && E > 0 && L > 0 && heads > 0 && E <= (1 << 20), DS_ERR_SHAPE,
             "ds_rope2d: bad shape B=%d E=%d heads=%d L=%d", B, E, heads, L);
  DS_REQUIRE(E % heads == 0 && (E / heads) % 2 == 0, DS_ERR_SHAPE, "ds_rope2d: E=%d heads=%d: the head width must be even", E, heads);
  if (B == 0) return DS_OK;
  const bool vec = L % 4 == 0 && aligned16(qkv);
  const int per = vec ? L / 4 : L;                      // threads a row can use
  int tl = 0;
  while (tl < 8 && (1 << tl) < per) ++tl;
  const int rows = 2 * E, rpb = NT >> tl;
  const dim3 grid((unsigned)((rows + rpb - 1) / rpb), (unsigned)B);
  hipStream_t st = ds::as_stream(stream);
  if (vec) hipLaunchKernelGGL(k_rope2d<4>, grid, dim3(NT), 0, st, qkv, cos_sin, B, E, L, E / heads / 2, tl, out_amax);
  else hipLaunchKernelGGL(k_rope2d<1>, grid, dim3(NT), 0, st, qkv, cos_sin, B, E, L, E / heads / 2, tl, out_amax);
  DS_CHECK_LAUNCH("ds_rope2d");
  return DS_OK;
}

int ds_upsample_bilinear(float* out, const float* x, int planes, int H, int W, int factor, void* stream, int flags) {
  DS_REQUIRE(flags == 0, DS_ERR_SHAPE, "ds_upsample_bilinear: flags %d (none are defined)", flags);
  DS_REQUIRE(out && x, DS_ERR_NULL, "ds_upsample_bilinear: NULL pointer");
  DS_REQUIRE(planes >= 0 && H > 0 && W > 0 && factor >= 1 && (long long)H * factor < (1 << 30) && (long long)W * factor < (1 << 30),
             DS_ERR_SHAPE, "ds_upsample_bilinear: bad shape planes=%d H=%d W=%d factor=%d", planes, H, W, factor);
  if (planes == 0) return DS_OK;
  const long long OW = (long long)W * factor;
  const bool vec = OW % 4 == 0 && aligned16(out);
  const long long total = (long long)planes * H * factor * (vec ? OW / 4 : OW);
  long long blocks = (total + NT - 1) / NT;
  if (blocks > 8192) blocks = 8192;
  const float rscale = 1.0f / (float)factor;
  hipStream_t st = ds::as_stream(stream);
  if (vec) hipLaunchKernelGGL(k_upsample_bilinear<4>, dim3((unsigned)blocks), dim3(NT), 0, st, out, x, (long long)planes, H, W, factor, rscale);
  else hipLaunchKernelGGL(k_upsample_bilinear<1>, dim3((unsigned)blocks), dim3(NT), 0, st, out, x, (long long)planes, H, W, factor, rscale);
  DS_CHECK_LAUNCH("ds_upsample_bilinear");
  return DS_OK;
}

int ds_depthwise_conv_silu(float* out, const float* x, const float* w, const float* bias, int B, int E, int H, int W, int ks,
                           unsigned* out_amax, void* stream, int flags) {
  DS_REQUIRE(flags == 0, DS_ERR_SHAPE, "ds_depthwise_conv_silu: flags %d (none are defined)", flags);
  DS_REQUIRE(out && x && w, DS_ERR_NULL, "ds_depthwise_conv_silu: NULL pointer");
  DS_REQUIRE(B >= 0 && B < 65536 && E > 0 && H > 0 && W > 0, DS_ERR_SHAPE, "ds_depthwise_conv_silu: bad shape B=%d E=%d H=%d W=%d", B, E, H, W);
  DS_REQUIRE(ks >= 1 && ks <= DKMAX && ks % 2 == 1, DS_ERR_UNSUPPORTED, "ds_depthwise_conv_silu: kernel size %d: odd sizes up to %d", ks,
             DKMAX);
  if (B == 0) return DS_OK;
  const int tiles_x = (W + DTW - 1) / DTW, tiles_y = (H + DTH - 1) / DTH;
  const long long blocks = (long long)B * E * tiles_x * tiles_y;
  DS_REQUIRE((long long)tiles_x * tiles_y < (1 << 30) && blocks < ((long long)1 << 31), DS_ERR_SHAPE,
             "ds_depthwise_conv_silu: B=%d E=%d H=%d W=%d exceeds the grid", B, E, H, W);
  hipLaunchKernelGGL(k_depthwise_silu, dim3((unsigned)blocks), dim3(NT), 0, ds::as_stream(stream), out, x, w, bias, E, H, W, ks, tiles_x,
                     tiles_y, out_amax);
  DS_CHECK_LAUNCH("ds_depthwise_conv_silu");
  return DS_OK;
}

int ds_swiglu(float* out, const float* ag, int B, size_t n_per_sample, unsigned* out_amax, void* stream, int flags) {
  DS_REQUIRE(flags == 0, DS_ERR_SHAPE, "ds_swiglu: flags %d (none are defined)", flags);
  DS_REQUIRE(out && ag, DS_ERR_NULL, "ds_swiglu: NULL pointer");
  DS_REQUIRE(B >= 0 && B < 65536, DS_ERR_SHAPE, "ds_swiglu: B=%d", B);
  if (B == 0 || n_per_sample == 0) return DS_OK;
  const bool vec = n_per_sample % 4 == 0 && aligned16(out) && aligned16(ag);
  const dim3 grid(stream_blocks(n_per_sample, B), (unsigned)B);
  if (vec) hipLaunchKernelGGL(k_swiglu<4>, grid, dim3(NT), 0, ds::as_stream(stream), out, ag, n_per_sample, out_amax);
  else hipLaunchKernelGGL(k_swiglu<1>, grid, dim3(NT), 0, ds::as_stream(stream), out, ag, n_per_sample, out_amax);
  DS_CHECK_LAUNCH("ds_swiglu");
  return DS_OK;
}

int ds_convit_blend(float* out, const float* u, const float* xc, const float* x0, const float* s, size_t n, void* stream, int flags) {
  DS_REQUIRE(flags == 0, DS_ERR_SHAPE, "ds_convit_blend: flags %d (none are defined)", flags);
  DS_REQUIRE(out && u && xc && x0 && s, DS_ERR_NULL, "ds_convit_blend: NULL pointer");
  if (n == 0) return DS_OK;
  const bool vec = n % 4 == 0 && aligned16(out) && aligned16(u) && aligned16(xc) && aligned16(x0);
  const dim3 grid(stream_blocks(n, 1));
  if (vec) hipLaunchKernelGGL(k_blend<4>, grid, dim3(NT), 0, ds::as_stream(stream), out, u, xc, x0, s, n);
  else hipLaunchKernelGGL(k_blend<1>, grid, dim3(NT), 0, ds::as_stream(stream), out, u, xc, x0, s, n);
  DS_CHECK_LAUNCH("ds_convit_blend");
  return DS_OK;
}

}  // extern "C"
