// Stride-2 3x3(x3) convolution with zero padding at the far end only: VAENet's Downsample (vaenet.py:662-673),
//   out[b,co,i,j] = bias[co] + sum w[co,ci,ky,kx] * x[b,ci,2i+ky,2j+kx],  x = 0 where an index reaches Hin / Win,
// output side Hin/2 (floor) for every Hin >= 2.
//
// k_conv_s2h: fp32 accuracy on the fp16 matrix cores (the fp16x3 split of ds_conv3h.hip: x = hi + lo, lo*hi + hi*lo + hi*hi on
// v_mfma_f32_32x32x16_f16, weights in ds_conv2d_h3_pack_weights' packing, the per-sample activation exponent and the shared
// epilogue of ds_conv_epilogue.h).  Workgroup = 4 waves, tile = 64 channels x 8 rows x 32 columns of the OUTPUT, each wave the
// whole channel tile for two rows, as in ds_conv3h.hip -- so the epilogue is the same code.  What differs is the patch:
// 8 x 32 outputs read 17 x 65 inputs, and a tap's 32 positions are every SECOND column.  The patch is therefore stored
// de-interleaved, [piece][h][row 17][column parity 2][33] vectors of 8 channels: tap (ky, kx) of output (i, j) reads row
// 2i + ky, parity kx & 1, index j + (kx >> 1) -- 32 consecutive 16-byte vectors per ds_read_b128, conflict-free, and no
// instruction is spent on the three quarters of the stride-1 result that a subsampling route throws away.
// LDS: patch 4 x 1122 vectors (71,808 B) + the chunk's three weight slabs (36,864 B) + bias (512 B) = 109,184 B: one workgroup
// per CU.  One 16-channel chunk at a time, single-buffered: stage (global -> split -> LDS), barrier, 9 taps x 12 MFMAs per wave,
// barrier.  No tile statistics: the consumer's norm takes its statistics from a pass over the output.
//
// The batch is addressed through (nin, so, si): output sample n reads input sample (n / nin) * so + (n % nin) * si (and that
// entry of in_amax) -- fields pass (1, 1, 0)-like identity, the depth taps of a volume (slice-major copy, ops.conv3d_s2) pass
// (Dout, D + 2, 2): every second slice, without a gather pass.
//
// k_conv_s2_direct / k_conv3d_s2_direct: exact fp32 FMA chains (channels outer, taps inner) for thin layers and the
// non-fp16x3 precisions; four output channels per thread, weights through wave-uniform scalar loads.
#include "ds_common.h"
#include "ds_conv3h_args.h"

namespace {

using namespace ds_conv3;

constexpr int S2_TH = 8, S2_TW = 32;                      // output tile
constexpr int S2_PR = 2 * S2_TH + 1, S2_PC = 2 * S2_TW + 1;   // input patch: 17 rows x 65 columns
constexpr int S2_HALF = S2_TW + 1;                        // vectors per (row, column parity): 33
constexpr int S2_NPOS = S2_PR * 2 * S2_HALF;              // vectors per (piece, h) image: 1122
constexpr int S2_XVEC = 4 * S2_NPOS;                      // [piece][h][NPOS]
constexpr int S2_WVEC = 3 * WSLAB_VEC;                    // the chunk's three (ky) slabs
constexpr int S2_STAGE_BYTES = (S2_XVEC + S2_WVEC) * 16;  // 108,672
constexpr int S2_LDS_BYTES = S2_STAGE_BYTES + 128 * 4;
constexpr int S2_ITEMS = 2 * S2_PR * S2_PC;               // (h, patch position) staging items: 2210
constexpr int S2_XI = (S2_ITEMS + NT - 1) / NT;           // per thread: 9
static_assert(4 * 64 * 2 * 32 * 4 <= S2_STAGE_BYTES, "the epilogue's four wave tiles fit the dead staging area");
static_assert(S2_LDS_BYTES <= 160 * 1024, "LDS of one CU");

struct ConvS2Args {
  float* out;
  const float* in;
  const u32x4* wp;
  const float* bias;
  const float* res1;
  const unsigned* in_amax;
  unsigned* out_amax;
  int wshift;
  int Cin, Cout, Hin, Win, H, W;      // H, W: the output's
  int tiles_x, n_chunks;
  int nin, so, si;                    // input sample of output sample n: (n / nin) * so + (n % nin) * si
};

__global__ __launch_bounds__(NT) void k_conv_s2h(const ConvS2Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* Xs = reinterpret_cast<u32x4*>(smem);
  u32x4* Ws = Xs + S2_XVEC;
  float* BS = reinterpret_cast<float*>(smem + S2_STAGE_BYTES);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int cot = blockIdx.x, b = blockIdx.z;
  const int ty = (int)blockIdx.y / a.tiles_x, tx = (int)blockIdx.y - ty * a.tiles_x;
  const int x0 = tx * S2_TW, y0 = ty * S2_TH;           // output coordinates
  const int HWin = a.Hin * a.Win;
  const int bin = (b / a.nin) * a.so + (b % a.nin) * a.si;
  const float* in_b = a.in + (size_t)bin * a.Cin * HWin;
  const u32x4* wp = a.wp + (size_t)cot * a.n_chunks * S2_WVEC;

  // staging plan: item -> (h, patch row, patch column); the global offset is in bounds for every item
  int xoff[S2_XI], xlds[S2_XI];
  unsigned xvalid = 0, xlive = 0;
#pragma unroll
  for (int i = 0; i < S2_XI; ++i) {
    const int item = i * NT + tid;
    const bool live = item < S2_ITEMS;
    const int it = live ? item : 0;
    const int h = it / (S2_PR * S2_PC), p = it - h * (S2_PR * S2_PC);
    const int r = p / S2_PC, c = p - r * S2_PC;
    const int gy = 2 * y0 + r, gx = 2 * x0 + c;
    const bool ok = live && gy < a.Hin && gx < a.Win;
    xoff[i] = ok ? gy * a.Win + gx : 0;               // the channel is added per element (ragged last chunk)
    xlds[i] = h * S2_NPOS + (r * 2 + (c & 1)) * S2_HALF + (c >> 1);
    if (ok) xvalid |= 1u << i;
    if (live) xlive |= 1u << i;
  }
  const unsigned amax_bits = ds_epi::act_bits(a.in_amax, bin);
  const float bias_shift = ds_epi::fetch_bias_shift(a.bias, nullptr, 0, b, cot * COT, a.Cout);
  const ds_epi::ActScale ascale = ds_epi::act_scale_of(amax_bits, a.wshift);
  ds_epi::commit_bias_shift(BS, bias_shift);           // published by the first chunk's barrier

  f32x16 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[m][r][q] = 0.f;

  const int wave_row = 2 * wv;
  for (int chunk = 0; chunk < a.n_chunks; ++chunk) {
    const int cbase = chunk * KC;
    const int nch = a.Cin - cbase < KC ? a.Cin - cbase : KC;
    const float* src = in_b + (size_t)cbase * HWin;
    if (chunk > 0) __syncthreads();                    // the previous chunk's operands are consumed
    // weights: the chunk's three slabs, 9 vectors per thread
    {
      const u32x4* wsrc = wp + (size_t)chunk * S2_WVEC;
      u32x4 wr[S2_WVEC / NT];
#pragma unroll
      for (int i = 0; i < S2_WVEC / NT; ++i) wr[i] = wsrc[i * NT + tid];
#pragma unroll
      for (int i = 0; i < S2_WVEC / NT; ++i) Ws[i * NT + tid] = wr[i];
    }
    // patch: three items' loads in flight at a time, then split and store
#pragma unroll
    for (int i0 = 0; i0 < S2_XI; i0 += 3) {
      float xr[3][8];
#pragma unroll
      for (int ii = 0; ii < 3; ++ii) {
        const int i = i0 + ii;
        const int h = (i * NT + tid) >= S2_PR * S2_PC ? 1 : 0;
        const float* p0 = src + xoff[i];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int c = 8 * h + k;
          xr[ii][k] = p0[(size_t)(c < nch ? c : 0) * HWin];
        }
      }
#pragma unroll
      for (int ii = 0; ii < 3; ++ii) {
        const int i = i0 + ii;
        if ((xlive >> i) & 1u) {
          const int h = (i * NT + tid) >= S2_PR * S2_PC ? 1 : 0;
          const bool ok = (xvalid >> i) & 1u;
          u32x4 qh, ql;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float v0 = (ok && 8 * h + 2 * k < nch) ? xr[ii][2 * k] * ascale.in_scale : 0.f;         // exact: power of two
            const float v1 = (ok && 8 * h + 2 * k + 1 < nch) ? xr[ii][2 * k + 1] * ascale.in_scale : 0.f;
            unsigned ph, pl;
            split2(v0, v1, ph, pl);
            qh[k] = ph; ql[k] = pl;
          }
          Xs[xlds[i]] = qh;                            // piece 0
          Xs[2 * S2_NPOS + xlds[i]] = ql;              // piece 1
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        f16x8 fa[2][2], fb[2][2];                      // [piece][m] weights, [piece][r] input
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
          for (int m = 0; m < 2; ++m)
            fa[p][m] = *reinterpret_cast<const f16x8*>(&Ws[ky * WSLAB_VEC + ((p * 3 + kx) * 2 + lh) * COT + 32 * m + li]);
#pragma unroll
          for (int r = 0; r < 2; ++r)
            fb[p][r] = *reinterpret_cast<const f16x8*>(
                &Xs[(p * 2 + lh) * S2_NPOS + ((2 * (wave_row + r) + ky) * 2 + (kx & 1)) * S2_HALF + li + (kx >> 1)]);
        }
        constexpr int PA[3] = {1, 0, 0};
        constexpr int PB[3] = {0, 1, 0};
#pragma unroll
        for (int t = 0; t < 3; ++t)                    // lo*hi, hi*lo, hi*hi
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 2; ++r)
              acc[m][r] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[PA[t]][m], fb[PB[t]][r], acc[m][r], 0, 0, 0);
      }
  }
  __syncthreads();                                     // staging is dead: each wave takes a private 16 KiB of it
  ds_epi::Args e;
  e.out = a.out; e.bias = a.bias; e.shift = nullptr; e.res1 = a.res1; e.res2 = nullptr; e.res1_up = 0;
  e.unscale = ds_epi::unscale_from_in(ascale.in_scale, a.wshift);
  e.shift_stride = 0;
  e.out_amax = a.out_amax ? a.out_amax + b : nullptr;
  e.b = b; e.co_base = cot * COT; e.y0 = y0 + wave_row; e.x0 = x0;
  e.Cout = a.Cout; e.H = a.H; e.W = a.W;
  e.tile_stats = nullptr; e.tile = 0; e.ntiles = 0; e.pa = 0; e.pb = 0;
  float* tile = reinterpret_cast<float*>(smem) + wv * (64 * 2 * 32);
  ds_epi::store_tile<false, 2>(acc, tile, BS, e);
}

// ---- exact fp32: one thread = one output position x 4 output channels -------------------------------------------------
constexpr int DCO = 4;

__global__ __launch_bounds__(256) void k_conv_s2_direct(float* out, const float* __restrict__ in, const float* w,
                                                        const float* __restrict__ bias, const float* res1, int Cin, int Cout,
                                                        int Hin, int Win, int H, int W, int cogs) {
  const int b = (int)blockIdx.y / cogs, co0 = ((int)blockIdx.y - b * cogs) * DCO;
  const int pos = blockIdx.x * 256 + threadIdx.x;
  if (pos >= H * W) return;
  const int i = pos / W, j = pos - i * W;
  const size_t HWin = (size_t)Hin * Win;
  const float* in_b = in + (size_t)b * Cin * HWin;
  typedef const __attribute__((address_space(4))) float* cptr;
  cptr wc = (cptr)w;
  int off[9];
  bool ok[9];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int gy = 2 * i + ky, gx = 2 * j + kx;
      ok[ky * 3 + kx] = gy < Hin && gx < Win;
      off[ky * 3 + kx] = ok[ky * 3 + kx] ? gy * Win + gx : 0;
    }
  float acc[DCO] = {0.f, 0.f, 0.f, 0.f};
  for (int ci = 0; ci < Cin; ++ci) {
    const float* p = in_b + (size_t)ci * HWin;
    float v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) v[t] = ok[t] ? p[off[t]] : 0.f;
#pragma unroll
    for (int c = 0; c < DCO; ++c) {
      const int co = co0 + c < Cout ? co0 + c : Cout - 1;          // uniform; the surplus channels are not stored
      cptr wk = wc + ((size_t)co * Cin + ci) * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[c] = __builtin_fmaf(wk[t], v[t], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < DCO; ++c) {
    const int co = co0 + c;
    if (co < Cout) {
      const size_t idx = ((size_t)b * Cout + co) * ((size_t)H * W) + pos;
      float r = acc[c] + (bias ? bias[co] : 0.f);
      if (res1) r = r + res1[idx];
      out[idx] = r;
    }
  }
}

__global__ __launch_bounds__(256) void k_conv3d_s2_direct(float* out, const float* __restrict__ in, const float* w,
                                                          const float* __restrict__ bias, const float* res1, int Cin, int Cout,
                                                          int Din, int Hin, int Win, int D, int H, int W, int cogs) {
  const int b = (int)blockIdx.y / cogs, co0 = ((int)blockIdx.y - b * cogs) * DCO;
  const size_t vol = (size_t)D * H * W;
  const size_t pos = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pos >= vol) return;
  const int k = (int)(pos / ((size_t)H * W));
  const int rem = (int)(pos - (size_t)k * H * W);
  const int i = rem / W, j = rem - i * W;
  const size_t HWin = (size_t)Hin * Win, Vin = (size_t)Din * HWin;
  const float* in_b = in + (size_t)b * Cin * Vin;
  typedef const __attribute__((address_space(4))) float* cptr;
  cptr wc = (cptr)w;
  int off[9];
  bool ok[9];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int gy = 2 * i + ky, gx = 2 * j + kx;
      ok[ky * 3 + kx] = gy < Hin && gx < Win;
      off[ky * 3 + kx] = ok[ky * 3 + kx] ? gy * Win + gx : 0;
    }
  float acc[DCO] = {0.f, 0.f, 0.f, 0.f};
  for (int ci = 0; ci < Cin; ++ci) {
#pragma unroll
    for (int kz = 0; kz < 3; ++kz) {
      const int gz = 2 * k + kz;
      const bool okz = gz < Din;
      const float* p = in_b + (size_t)ci * Vin + (size_t)(okz ? gz : 0) * HWin;
      float v[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) v[t] = (okz && ok[t]) ? p[off[t]] : 0.f;
#pragma unroll
      for (int c = 0; c < DCO; ++c) {
        const int co = co0 + c < Cout ? co0 + c : Cout - 1;
        cptr wk = wc + (((size_t)co * Cin + ci) * 3 + kz) * 9;
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[c] = __builtin_fmaf(wk[t], v[t], acc[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < DCO; ++c) {
    const int co = co0 + c;
    if (co < Cout) {
      const size_t idx = ((size_t)b * Cout + co) * vol + pos;
      float r = acc[c] + (bias ? bias[co] : 0.f);
      if (res1) r = r + res1[idx];
      out[idx] = r;
    }
  }
}

}  // namespace

extern "C" {

int ds_conv2d_s2_h3(float* out, const float* in, const void* w_packed, int wshift, const float* bias, const float* res1, int B,
                    int Cin, int Cout, int Hin, int Win, int nin, int so, int si, const unsigned* in_amax, unsigned* out_amax,
                    void* stream) {
  DS_REQUIRE(out && in && w_packed, DS_ERR_NULL, "ds_conv2d_s2_h3: NULL pointer");
  DS_REQUIRE(B >= 0 && Cin > 0 && Cout > 0 && Hin >= 2 && Win >= 2, DS_ERR_SHAPE,
             "ds_conv2d_s2_h3: bad shape B=%d Cin=%d Cout=%d Hin=%d Win=%d (sides of at least 2)", B, Cin, Cout, Hin, Win);
  DS_REQUIRE(nin >= 1 && so >= 0 && si >= 0, DS_ERR_SHAPE, "ds_conv2d_s2_h3: sample map (nin=%d, so=%d, si=%d)", nin, so, si);
  DS_REQUIRE((reinterpret_cast<uintptr_t>(w_packed) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0 &&
                 (reinterpret_cast<uintptr_t>(res1) & 15u) == 0,
             DS_ERR_SHAPE, "ds_conv2d_s2_h3: out, res1 and w_packed must be 16-byte aligned");
  DS_REQUIRE(wshift >= -40 && wshift <= 40, DS_ERR_SHAPE, "ds_conv2d_s2_h3: wshift %d out of range", wshift);
  DS_REQUIRE((long long)Cin * Hin * Win < (1ll << 31), DS_ERR_SHAPE, "ds_conv2d_s2_h3: per-sample input exceeds 2^31 floats");
  if (B == 0) return DS_OK;
  ConvS2Args a;
  a.out = out; a.in = in; a.wp = reinterpret_cast<const u32x4*>(w_packed); a.bias = bias; a.res1 = res1;
  a.in_amax = in_amax; a.out_amax = out_amax; a.wshift = wshift;
  a.Cin = Cin; a.Cout = Cout; a.Hin = Hin; a.Win = Win; a.H = Hin / 2; a.W = Win / 2;
  a.tiles_x = (a.W + S2_TW - 1) / S2_TW;
  const int tiles_y = (a.H + S2_TH - 1) / S2_TH;
  a.n_chunks = (Cin + KC - 1) / KC;
  a.nin = nin; a.so = so; a.si = si;
  const long long tiles = (long long)a.tiles_x * tiles_y;
  DS_REQUIRE(tiles < 65536 && B < 65536, DS_ERR_SHAPE, "ds_conv2d_s2_h3: %lld pixel tiles x %d samples exceed the grid limits", tiles, B);
  const int rc = ds::ensure_dynamic_lds<&k_conv_s2h>(S2_LDS_BYTES, "hipFuncSetAttribute(conv_s2h)");
  if (rc != DS_OK) return rc;
  hipLaunchKernelGGL(k_conv_s2h, dim3((unsigned)((Cout + COT - 1) / COT), (unsigned)tiles, (unsigned)B), dim3(NT), S2_LDS_BYTES,
                     ds::as_stream(stream), a);
  DS_CHECK_LAUNCH("ds_conv2d_s2_h3");
  return DS_OK;
}

int ds_conv2d_s2_direct(float* out, const float* in, const float* w, const float* bias, const float* res1, int B, int Cin, int Cout,
                        int Hin, int Win, void* stream) {
  DS_REQUIRE(out && in && w, DS_ERR_NULL, "ds_conv2d_s2_direct: NULL pointer");
  DS_REQUIRE(B >= 0 && Cin > 0 && Cout > 0 && Hin >= 2 && Win >= 2, DS_ERR_SHAPE,
             "ds_conv2d_s2_direct: bad shape B=%d Cin=%d Cout=%d Hin=%d Win=%d (sides of at least 2)", B, Cin, Cout, Hin, Win);
  DS_REQUIRE((long long)Hin * Win < (1ll << 31), DS_ERR_SHAPE, "ds_conv2d_s2_direct: plane exceeds 2^31 floats");
  if (B == 0) return DS_OK;
  const int H = Hin / 2, W = Win / 2, cogs = (Cout + DCO - 1) / DCO;
  DS_REQUIRE((long long)B * cogs < 65536, DS_ERR_SHAPE, "ds_conv2d_s2_direct: B * ceil(Cout/4) must stay below 65536");
  hipLaunchKernelGGL(k_conv_s2_direct, dim3((unsigned)((H * W + 255) / 256), (unsigned)(B * cogs)), dim3(256), 0,
                     ds::as_stream(stream), out, in, w, bias, res1, Cin, Cout, Hin, Win, H, W, cogs);
  DS_CHECK_LAUNCH("ds_conv2d_s2_direct");
  return DS_OK;
}

int ds_conv3d_s2_direct(float* out, const float* in, const float* w, const float* bias, const float* res1, int B, int Cin, int Cout,
                        int Din, int Hin, int Win, void* stream) {
  DS_REQUIRE(out && in && w, DS_ERR_NULL, "ds_conv3d_s2_direct: NULL pointer");
  DS_REQUIRE(B >= 0 && Cin > 0 && Cout > 0 && Din >= 2 && Hin >= 2 && Win >= 2, DS_ERR_SHAPE,
             "ds_conv3d_s2_direct: bad shape B=%d Cin=%d Cout=%d Din=%d Hin=%d Win=%d (sides of at least 2)", B, Cin, Cout, Din, Hin, Win);
  DS_REQUIRE((long long)Hin * Win < (1ll << 31), DS_ERR_SHAPE, "ds_conv3d_s2_direct: plane exceeds 2^31 floats");
  if (B == 0) return DS_OK;
  const int D = Din / 2, H = Hin / 2, W = Win / 2, cogs = (Cout + DCO - 1) / DCO;
  const long long vol = (long long)D * H * W;
  DS_REQUIRE((long long)B * cogs < 65536 && (vol + 255) / 256 < (1ll << 31), DS_ERR_SHAPE,
             "ds_conv3d_s2_direct: B * ceil(Cout/4) must stay below 65536");
  hipLaunchKernelGGL(k_conv3d_s2_direct, dim3((unsigned)((vol + 255) / 256), (unsigned)(B * cogs)), dim3(256), 0,
                     ds::as_stream(stream), out, in, w, bias, res1, Cin, Cout, Din, Hin, Win, D, H, W, cogs);
  DS_CHECK_LAUNCH("ds_conv3d_s2_direct");
  return DS_OK;
}

}  // extern "C"
