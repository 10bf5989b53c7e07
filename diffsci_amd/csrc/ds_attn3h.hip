// Single-head self-attention on the fp16 matrix cores with fp32 accuracy ("fp16x3", the scheme of
// ds_conv3h.hip): every fp32 operand of the two products
//     S^T = K (Q/sqrt(E))^T          O^T += V^T P^T
// is split into fp16 hi + lo pieces and lo*hi + hi*lo + hi*hi are accumulated in fp32 by
// v_mfma_f32_32x32x16_f16.  Softmax statistics, the running maximum / sum and the rescaling of O
// stay in fp32 on the accumulators.  Domain: |q|, |k|, |v| < 65504 and not far below 1 -- or, with in_amax [2][B] (the
// per-sample max |q, k| and max |v| the in-projection left, ds_conv_epilogue.h), any magnitude: q and k are staged times
// 2^kqk, v times 2^kv, S is read back times 2^-2kqk inside the softmax's FMA and O times 2^-kv with the final 1 / l.
// The kernels carry one exponent row each for q, k and v (q times 2^aq, k times 2^ak, S times 2^-(aq+ak)); the qkv entry
// points hand their one q-and-k row to both, ds_attention_h3_xkv hands three.
//
// Layout: operands arrive channel-major ([B, 3E, L], what the 1x1 projections write) and the
// output is channel-major ([B, E, L]).  The regrouping the MFMA wants happens while staging:
//   K tile  -> LDS [piece][d-group of 8][key 32][8 d]      (A operand of S^T: lane = key)
//   V tile  -> LDS [piece][key-group of 8][d E][8 keys]    (A operand of O^T: lane = d)
//   Q       -> registers, [k-slab of 16 d][piece]           (B operand of S^T: lane = query)
// each item being 8 global loads (a 128-byte-coalesced column walk) + one exact split + one
// ds_write_b128 per piece.  P never touches LDS: the 32x32 accumulator holds, for the lane's
// query, keys (r&3)+8(r>>2)+4h in register r of lane half h; packing pairs to fp16 and two
// v_permlane32_swap per 16-key slab and piece turn that into the B operand of the next MFMA.
//
// Two staging forms.  IMG = false: every workgroup loads its K / V tiles as fp32, splits them and writes the LDS
// images itself (no workspace; every tile is split once per 128-query block of the sample).  IMG = true: a pre-pass
// (k_attn_images) splits K and V ONCE per sample into global images that already have the LDS layout, and the
// attention kernel stages a tile with eight 1-KiB LDS-DMA instructions per wave and operand -- no staging registers,
// no split VALU work in the loop.  At L = 4096 a tile is otherwise re-split by 32 workgroups.
//
// Workgroup = 4 waves x 32 queries; key tiles of 32.  K and V tiles are double-buffered in LDS
// (4 x 32 KiB at E = 256) -- one barrier per tile.  Q (E/2 regs), O (E/2 regs) live in the 512-entry unified
// register file (one wave per SIMD): O and the S accumulators in its accumulator half, where only matrix instructions
// reach them, Q in the vector half.  IMG = false stages one tile ahead through ONE set of 32 registers: the next K tile
// is loaded under the S^T product and written out before the softmax, the next V tile is loaded under the softmax / O^T
// product.
//
// The tile loop of the image form (one wave per SIMD: whatever the wave waits for, the matrix pipe waits for too).
// Tile kb runs, in this order: the LDS-DMA of K(kb+2) and V(kb+1); the test of the deferred rescale on a maximum the
// previous tile already reduced; the S^T product of tile kb+1 in ET groups of six matrix instructions, each group's K
// fragments read from LDS while the group before it computes, with the softmax of tile kb (exp2, the fp16 split of P, the
// lane swaps) cut into 24 steps that are handed out over those groups; the O^T product of tile kb in items of three matrix
// instructions whose V fragments are read two items ahead, with the sum of the two S chains and the next tile's maximum
// under its first items.  The last tile is peeled off, so that every other tile issues its successor's S^T product
// unconditionally and that product shares a basic block with the softmax it hides.  The rescale of O is a cold branch
// that works on the accumulator registers in place (rescale_O).  Same arithmetic in the same order as IMG = false: the
// two forms agree bit for bit.
//
// Multi-head (nn.MultiheadAttention(E, H), ds_attention_h3_heads): the same kernels with a (sample, head) grid row and the head
// width d = E / H as the template width; see MH below.
#include <cstdlib>

#include "ds_common.h"
#include "ds_conv_epilogue.h"
#include "ds_h3_common.h"

namespace {

using ds::f32x4;
using ds::wave_max;
using ds_epi::f32x16;
using ds_h3::f16x8;
using ds_h3::split2;
using ds_h3::u32x4;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int NT = 256;
constexpr int KB = 32;       // keys per tile
constexpr float RESCALE_T = 8.0f;

// e^x for the softmax numerators (x <= RESCALE_T): one FMA and the hardware exp2 (1 ulp; the argument's rounding adds
// |x| * 2^-24 relative, i.e. < 1e-6 wherever the result is not negligible) instead of libm's range-reduced expf
constexpr float LOG2E = 1.44269504088896341f;

__device__ __forceinline__ f16x8 as_f16x8(u32x4 v) { return __builtin_bit_cast(f16x8, v); }

// MH (multi-head): grid.y runs over (sample, head) rows b * heads + h, E below is the head width d, and the head reads
// rows [h d, (h+1) d) of each third of qkv [B, 3 heads d, L] and writes rows [h d, (h+1) d) of out [B, heads d, L].
// MH = false is the single-head kernel exactly (heads = 1, nb = gridDim.y: the compiler sees the same code).
template <int ET, bool IMG, bool MH>
__global__ __launch_bounds__(NT) void k_attn3h(float* out, const float* __restrict__ q, size_t q_bs,
                                               const u32x4* __restrict__ kimg, const u32x4* __restrict__ vimg, int L, int heads,
                                               float scale, float thr, const unsigned* q_amax, const unsigned* k_amax,
                                               const unsigned* v_amax, unsigned* out_amax) {
  constexpr int E = 32 * ET;                         // the head width
  constexpr int NDG = E / 8;                         // d-groups of 8
  constexpr int NS = E / 16;                         // k-slabs of the S^T product
  constexpr int KITEMS = NDG * KB;                   // (d-group, key) items per K tile
  constexpr int KI = (KITEMS + NT - 1) / NT;
  constexpr int VITEMS = E * 4;                      // (d, key-group) items per V tile
  constexpr int VI = (VITEMS + NT - 1) / NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int KVEC = 2 * NDG * KB;                 // vectors per K buffer  [piece][dg][key]
  constexpr int VVEC = 2 * 4 * E;                    // vectors per V buffer  [piece][kg][d]
  u32x4* Kbuf = reinterpret_cast<u32x4*>(smem);      // [2][KVEC]
  u32x4* Vbuf = Kbuf + 2 * KVEC;                     // [2][VVEC]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  // XCD-aware order (see ds_conv3h.hip): the query blocks of one sample stream the same K / V tiles; keep them on
  // one XCD so that after the first block the tiles come from its L2
  unsigned qblk, b_u;
  {
    const unsigned nx = gridDim.x;
    const unsigned id = blockIdx.x + nx * blockIdx.y;
    const unsigned total = nx * gridDim.y;
    const unsigned per = total >> 3, rem = total & 7u;
    const unsigned xcd = id & 7u, k = id >> 3;
    const unsigned logical = xcd * per + (xcd < rem ? xcd : rem) + k;
    qblk = logical % nx;
    b_u = logical / nx;                              // the (sample, head) row
  }
  const int row = (int)b_u;
  const int b = MH ? row / heads : row, h = MH ? row - b * heads : 0;
  const int Etot = MH ? E * heads : E;               // channels of one third of qkv
  const int q0_raw = ((int)qblk * 4 + wv) * 32;
  const bool active = q0_raw < L;                    // a wave past the last query block recomputes
  const int q0 = active ? q0_raw : L - 32;           // the last block and does not store (no branches
                                                     // around the MFMA pipeline: they cost registers)
  // q: the queries [.., E tot, L] with batch stride q_bs.  IMG reads nothing else from it; the form that stages in the workgroup
  // reads K and V behind Q, i.e. q is qkv [B, 3 Etot, L]
  const float* Qt = q + (size_t)b * q_bs + (size_t)h * E * L;
  const float* Kt = Qt + (size_t)Etot * L;
  const float* Vt = Kt + (size_t)Etot * L;
  // the sample's activation exponents (0 without a row): q times 2^aq, k times 2^ak, v times 2^av; S times 2^-(aq+ak), O times
  // 2^-av -- all exact
  const unsigned q_bits = ds_epi::act_bits(q_amax, b), k_bits = ds_epi::act_bits(k_amax, b), v_bits = ds_epi::act_bits(v_amax, b);
  const int aq = ds_epi::act_exponent_of(q_bits, -60, 60);           // the three loads are in flight together: one round trip
  const int ak = ds_epi::act_exponent_of(k_bits, -60, 60);
  const int av = ds_epi::act_exponent_of(v_bits, -120, 120);
  const float a_in = ds_epi::pow2f(ak), v_in = ds_epi::pow2f(av);
  const float s_un = ds_epi::pow2f(-(aq + ak)), o_un = ds_epi::pow2f(-av);
  scale = ds_epi::mul_pow2(scale, aq);

  // ---- Q fragments: lane (query li, half lh) holds d = 16s + 8lh + 0..7, scaled, split ----
  u32x4 qh[NS], ql[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
      v[k] = Qt[(size_t)(16 * s + 8 * lh + k) * L + q0 + li] * scale;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned h, l;
      split2(v[2 * k], v[2 * k + 1], h, l);
      qh[s][k] = h; ql[s][k] = l;
    }
  }

  f32x16 O[ET];
#pragma unroll
  for (int t = 0; t < ET; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) O[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  static_assert(KI * 8 == VI * 8, "K and V staging share one register set");
  float sr[KI][8];                                   // staging registers (K tile, then V tile)
  // Addresses are (wave-uniform row base) + (32-bit per-lane offset): the scalar-base load form
  // keeps them out of the vector registers (hoisted 64-bit per-load addresses cost 80 VGPRs).
  unsigned koff[KI], voff[VI];
#pragma unroll
  for (int i = 0; i < KI; ++i) {
    const int e = tid + NT * i;
    const int dg = (e / KB) % NDG, key = e % KB;            // % NDG keeps tail lanes in bounds
    koff[i] = (unsigned)(8 * dg) * (unsigned)L + (unsigned)key;
  }
#pragma unroll
  for (int i = 0; i < VI; ++i) {
    const int e = tid + NT * i;
    const int d = (e >> 2) % E, kg = e & 3;
    voff[i] = (unsigned)d * (unsigned)L + (unsigned)(8 * kg);
  }
  auto k_load = [&](int key0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float* row = Kt + (size_t)k * L + key0;         // uniform
#pragma unroll
      for (int i = 0; i < KI; ++i) sr[i][k] = row[koff[i]];
    }
  };
  auto k_store = [&](u32x4* Ks) {
#pragma unroll
    for (int i = 0; i < KI; ++i) {
      const int e = tid + NT * i;
      if (NT * (i + 1) <= KITEMS || e < KITEMS) {
        u32x4 h, l;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          unsigned a, c;
          split2(sr[i][2 * k] * a_in, sr[i][2 * k + 1] * a_in, a, c);
          h[k] = a; l[k] = c;
        }
        Ks[e] = h;                         // e = dg*32 + key
        Ks[NDG * KB + e] = l;
      }
    }
  };
  auto v_load = [&](int key0) {
    const float* base = Vt + key0;                           // uniform
#pragma unroll
    for (int i = 0; i < VI; ++i) {
      const float* p = base + voff[i];
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(p);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) { sr[i][k] = v0[k]; sr[i][4 + k] = v1[k]; }
    }
  };
  auto v_store = [&](u32x4* Vs) {
#pragma unroll
    for (int i = 0; i < VI; ++i) {
      const int e = tid + NT * i;
      if (NT * (i + 1) <= VITEMS || e < VITEMS) {
        const int d = e >> 2, kg = e & 3;
        u32x4 h, l;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          unsigned a, c;
          split2(sr[i][2 * k] * v_in, sr[i][2 * k + 1] * v_in, a, c);
          h[k] = a; l[k] = c;
        }
        Vs[kg * E + d] = h;
        Vs[4 * E + kg * E + d] = l;
      }
    }
  };

  const int nkb = L / KB;
  // IMG: tile kb of sample b as LDS-ready images; a tile = KVEC (= VVEC = 8E) vectors = 2*ET 1-KiB pieces per wave
  static_assert(KVEC == VVEC && KVEC % (64 * 4) == 0, "image tiles are whole LDS-DMA pieces per wave");
  const u32x4* kimg_b = IMG ? kimg + (size_t)row * nkb * KVEC : nullptr;
  const u32x4* vimg_b = IMG ? vimg + (size_t)row * nkb * VVEC : nullptr;
  static_assert(KVEC / 256 == ET, "one LDS-DMA piece per wave, operand and group of the S^T product");
  auto dma_piece = [&](u32x4* dst, const u32x4* src, int i) __attribute__((always_inline)) {
    const int k = wv + 4 * i;                        // wave-uniform piece
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + 64 * k + lane),
                                     (__attribute__((address_space(3))) void*)(dst + 64 * k), 16, 0, 0);
  };
  auto dma = [&](u32x4* dst, const u32x4* src) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < ET; ++i) dma_piece(dst, src, i);
  };
  // ---- the two matrix products and the softmax between them, shared by both staging forms ----
  // S^T[key][query] as two accumulation chains (even / odd 16-wide d slabs) S0 + S1, which the caller sums.  The ET groups of
  // six matrix instructions are one scheduling region each: a group's four K fragments are read from LDS while the group before
  // it computes (one wave per SIMD: an LDS round trip that a matrix instruction waits for is idle matrix time), and under(g)
  // is vector work of the caller's that the scheduler may spread under group g's matrix instructions.
  auto qk = [&](const u32x4* Ks, f32x16& S0, f32x16& S1, auto&& under) __attribute__((always_inline)) {
    f16x8 fr[2][4];                                  // [buffer][ah, al, bh, bl]
    auto frags = [&](int s, f16x8* f) __attribute__((always_inline)) {
      f[0] = as_f16x8(Ks[(2 * s + lh) * KB + li]);
      f[1] = as_f16x8(Ks[NDG * KB + (2 * s + lh) * KB + li]);
      f[2] = as_f16x8(Ks[(2 * s + 2 + lh) * KB + li]);
      f[3] = as_f16x8(Ks[NDG * KB + (2 * s + 2 + lh) * KB + li]);
    };
#pragma unroll
    for (int r = 0; r < 16; ++r) { S0[r] = 0.f; S1[r] = 0.f; }
    frags(0, fr[0]);
#pragma unroll
    for (int s = 0; s < NS; s += 2) {
      const int g = s >> 1;
      if (s + 2 < NS) frags(s + 2, fr[(g + 1) & 1]);
      const f16x8 ah = fr[g & 1][0], al = fr[g & 1][1], bh = fr[g & 1][2], bl = fr[g & 1][3];
      S0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, as_f16x8(qh[s]), S0, 0, 0, 0);
      S1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, as_f16x8(qh[s + 1]), S1, 0, 0, 0);
      S0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, as_f16x8(ql[s]), S0, 0, 0, 0);
      S1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, as_f16x8(ql[s + 1]), S1, 0, 0, 0);
      S0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, as_f16x8(qh[s]), S0, 0, 0, 0);
      S1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, as_f16x8(qh[s + 1]), S1, 0, 0, 0);
      under(g);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // a tile's largest logit per query (= per lane; the two halves combined with one shuffle)
  auto tile_max = [&](const f32x16& S) __attribute__((always_inline)) {
    float mx = S[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, S[r]);
    return fmaxf(mx, __shfl_xor(mx, 32, 64)) * s_un;
  };
  // O *= alpha, in the rarely taken branch of the deferred rescale.  Written on the accumulator registers themselves: as a
  // plain multiply the compiler copies all of O out of them at the top of EVERY tile (16 ET v_accvgpr_read per tile, and
  // as many vector registers held through the S^T product) so that the branch finds them in place.  The matrix
  // instructions that wrote O were issued before the barrier that ended the previous tile; the s_nop covers what is left
  // of the last one's passes where nothing else lies between (the compiler sees no hazard inside an asm block).
  auto rescale_O = [&](float alpha) __attribute__((always_inline)) {
    asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
#pragma unroll
    for (int t = 0; t < ET; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float o = O[t][r], tmp;
        asm volatile("v_accvgpr_read_b32 %1, %0\n\tv_mul_f32 %1, %1, %2\n\tv_accvgpr_write_b32 %0, %1" : "+a"(o), "=&v"(tmp) : "v"(alpha));
        O[t][r] = o;
      }
    asm volatile("s_nop 3" ::: "memory");
  };
  if constexpr (IMG) {
    // Software pipeline (one wave per SIMD: nothing else hides the softmax; the header comment has the order): tile kb
    // issues the matrix instructions of S(kb+1) with the vector instructions of softmax(S(kb)) under them, then the O^T
    // product of tile kb.  K therefore runs one tile ahead of V: K(kb+2) -> K buffer kb&1 (last read for S(kb) in
    // iteration kb-1), V(kb+1) -> V buffer (kb+1)&1 (last read in iteration kb-1).
    dma(Kbuf, kimg_b);
    dma(Vbuf, vimg_b);
    if (nkb > 1) dma(Kbuf + KVEC, kimg_b + KVEC);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x16 S, Sn0, Sn1;
    qk(Kbuf, Sn0, Sn1, [](int) {});
    S = Sn0 + Sn1;
    float mx = tile_max(S);
    // One tile.  `last` is a literal at both call sites: every tile but the last runs the S^T product of its successor
    // unconditionally, so that product and this tile's softmax are ONE basic block the scheduler can interleave.
    auto tile = [&](int kb, const bool last) __attribute__((always_inline)) {
      const u32x4* Vs = Vbuf + (kb & 1) * VVEC;
      // K(kb+2) and V(kb+1) travel as one LDS-DMA piece each under every group of the S^T product below: the 2 ET pieces of
      // a wave issued back to back keep it at the address path's 64 B/clk (a quarter of the tile's matrix time at E = 256)
      // before its first matrix instruction.  The tile before the last has no K(kb+2): it fetches the last tile's K once
      // more, into the buffer nobody reads again, instead of a branch that would split the block.
      u32x4* Kd = Kbuf + (kb & 1) * KVEC;
      u32x4* Vd = Vbuf + ((kb + 1) & 1) * VVEC;
      const u32x4* Kg = kimg_b + (size_t)min(kb + 2, nkb - 1) * KVEC;
      const u32x4* Vg = vimg_b + (size_t)min(kb + 1, nkb - 1) * VVEC;
      // the deferred rescale (see the other form), decided on the maximum the previous iteration left: a compare and a
      // branch here, not a reduction.  Cold: O stays in the accumulator registers around it.
      if (__builtin_expect(__any(mx > m_run + thr), 0)) {
        const float m_new = fmaxf(m_run, mx);
        const float alpha = expf(m_run - m_new);
        l_run = l_run * alpha;
        m_run = m_new;
        rescale_O(alpha);
      }
      // ---- online softmax of tile kb (vector pipe), in 24 steps: e^(S - m) of the 16 registers, then the fp16 split of the 8
      // register pairs, each 16-key slab's lane swaps behind its fourth pair.  Same operations in the same order as the other form.
      float rs = 0.f;
      const float mneg = -m_run;
      unsigned ph[2][4], pl[2][4];
      auto softmax_step = [&](int i) __attribute__((always_inline)) {
        if (i < 16) {
          S[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[i], s_un, mneg) * LOG2E);     // the difference first: see the other form
          rs += S[i];
        } else {
          const int t = (i - 16) >> 2, k = (i - 16) & 3;
          split2(S[8 * t + 2 * k], S[8 * t + 2 * k + 1], ph[t][k], pl[t][k]);
          if (k == 3) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
              u32x2 r = __builtin_amdgcn_permlane32_swap(ph[t][j], ph[t][2 + j], false, false);
              ph[t][j] = r[0]; ph[t][2 + j] = r[1];
              r = __builtin_amdgcn_permlane32_swap(pl[t][j], pl[t][2 + j], false, false);
              pl[t][j] = r[0]; pl[t][2 + j] = r[1];
            }
          }
        }
      };
      // V fragments [vh, vl] of item i = (t, slab): read two items (six matrix instructions) ahead
      constexpr int NI = 2 * ET;
      f16x8 vf[3][2];
      auto vfrags = [&](int i, f16x8* f) __attribute__((always_inline)) {
        const int t = i >> 1, sl = i & 1;
        f[0] = as_f16x8(Vs[(2 * sl + lh) * E + 32 * t + li]);
        f[1] = as_f16x8(Vs[4 * E + (2 * sl + lh) * E + 32 * t + li]);
      };
      if (!last) {
        // matrix pipe: the S^T product of tile kb + 1, with 24 / ET softmax steps of tile kb under each of its groups
        qk(Kbuf + ((kb + 1) & 1) * KVEC, Sn0, Sn1, [&](int g) __attribute__((always_inline)) {
#pragma unroll
          for (int i = 24 * g / ET; i < 24 * (g + 1) / ET; ++i) softmax_step(i);
          dma_piece(Kd, Kg, g);
          dma_piece(Vd, Vg, g);
          if (g == ET - 1) { vfrags(0, vf[0]); vfrags(1, vf[1]); }
        });
      } else {
#pragma unroll
        for (int i = 0; i < 24; ++i) softmax_step(i);
        vfrags(0, vf[0]); vfrags(1, vf[1]);
      }
      rs += __shfl_xor(rs, 32, 64);
      l_run = l_run + rs;
      const u32x4 ph0{ph[0][0], ph[0][1], ph[0][2], ph[0][3]}, pl0{pl[0][0], pl[0][1], pl[0][2], pl[0][3]};
      const u32x4 ph1{ph[1][0], ph[1][1], ph[1][2], ph[1][3]}, pl1{pl[1][0], pl[1][1], pl[1][2], pl[1][3]};
      // ---- O^T[d][query] += V^T P^T: one scheduling region per item of three matrix instructions ----
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        if (i + 2 < NI) vfrags(i + 2, vf[(i + 2) % 3]);
        const f16x8 vh = vf[i % 3][0], vl = vf[i % 3][1];
        const f16x8 bh = as_f16x8((i & 1) ? ph1 : ph0), bl = as_f16x8((i & 1) ? pl1 : pl0);
        O[i >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, bh, O[i >> 1], 0, 0, 0);
        O[i >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, bl, O[i >> 1], 0, 0, 0);
        O[i >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, bh, O[i >> 1], 0, 0, 0);
        // the next tile's logits and their maximum: vector work under the O^T product, three matrix instructions after the
        // S^T product's last
        if (!last && i == 1) {
          S = Sn0 + Sn1;
          mx = tile_max(S);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    };
    for (int kb = 0; kb + 1 < nkb; ++kb) tile(kb, false);
    tile(nkb - 1, true);
  } else {
  k_load(0);
  k_store(Kbuf);
  v_load(0);
  v_store(Vbuf);
  __syncthreads();
  for (int kb = 0; kb < nkb; ++kb) {
    const bool more = kb + 1 < nkb;
    const u32x4* Ks = Kbuf + (kb & 1) * KVEC;
    const u32x4* Vs = Vbuf + (kb & 1) * VVEC;
    u32x4* Kn = Kbuf + ((kb + 1) & 1) * KVEC;
    u32x4* Vn = Vbuf + ((kb + 1) & 1) * VVEC;
    if (more) k_load((kb + 1) * KB);                 // flies under the S^T product
    f32x16 S;
    {
      // ---- S^T[key][query]: the same two chains, in the same order, as qk() above (the two forms agree bit for bit) ----
      f32x16 S1;
#pragma unroll
      for (int r = 0; r < 16; ++r) { S[r] = 0.f; S1[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < NS; s += 2) {
        const f16x8 ah = as_f16x8(Ks[(2 * s + lh) * KB + li]);
        const f16x8 al = as_f16x8(Ks[NDG * KB + (2 * s + lh) * KB + li]);
        const f16x8 bh = as_f16x8(Ks[(2 * s + 2 + lh) * KB + li]);
        const f16x8 bl = as_f16x8(Ks[NDG * KB + (2 * s + 2 + lh) * KB + li]);
        S = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, as_f16x8(qh[s]), S, 0, 0, 0);
        S1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(bl, as_f16x8(qh[s + 1]), S1, 0, 0, 0);
        S = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, as_f16x8(ql[s]), S, 0, 0, 0);
        S1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, as_f16x8(ql[s + 1]), S1, 0, 0, 0);
        S = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, as_f16x8(qh[s]), S, 0, 0, 0);
        S1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(bh, as_f16x8(qh[s + 1]), S1, 0, 0, 0);
        // bound the operand look-ahead: without a fence the scheduler hoists all 2*NS fragment
        // reads (128 registers at E = 256) in front of the first MFMA
        if ((s & 2) == 2) __builtin_amdgcn_sched_barrier(0);
      }
      S = S + S1;
    }
    if (!IMG && more) {
      k_store(Kn);                                   // the other K buffer: last read two tiles ago
      v_load((kb + 1) * KB);                         // flies under the softmax and the O^T product
    }
    {
      // ---- online softmax (fp32, per query = per lane; halves combined with one shuffle) ----
      const float mx = tile_max(S);
      // Deferred rescaling: O and l are kept relative to a reference maximum m_run that only moves
      // when some query's block maximum exceeds it by more than RESCALE_T (so P <= e^RESCALE_T,
      // far inside fp16's range for the hi piece).  The O-wide multiply then sits in a rarely
      // taken, wave-uniform branch instead of on every tile's critical path.
      if (__builtin_expect(__any(mx > m_run + thr), 0)) {
        const float m_new = fmaxf(m_run, mx);
        const float alpha = expf(m_run - m_new);      // exp(-inf) = 0 on the first tile (O = 0, l = 0)
        l_run = l_run * alpha;
        m_run = m_new;
        rescale_O(alpha);
      }
      float rs = 0.f;
      const float mneg = -m_run;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // e^(S - m): the difference FIRST (one fma with the logits' power of two: exact for nearby values), then log2(e) and the
        // hardware exp2.  [fma(S, log2 e, -m log2 e) saves an instruction but rounds m log2 e on its own: at logits of 1e12 -- an
        // untrained network's -- that is off by 1e5, the exponent overflows and the sample turns into NaN where the reference's
        // softmax is a finite one-hot.]
        S[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(S[r], s_un, mneg) * LOG2E);
        rs += S[r];
      }
      rs += __shfl_xor(rs, 32, 64);
      l_run = l_run + rs;
      // ---- P^T as B operand: per 16-key slab, registers 8t..8t+7 -> [A0 A1 B0 B1] + half swap ----
      u32x4 ph[2], pl[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        unsigned h[4], l[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) split2(S[8 * t + 2 * k], S[8 * t + 2 * k + 1], h[k], l[k]);
        // h[0],h[1] = u=0 (keys 16t + 4*half + 0..3); h[2],h[3] = u=1 (keys 16t + 8 + 4*half + 0..3)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          u32x2 r = __builtin_amdgcn_permlane32_swap(h[k], h[2 + k], false, false);
          h[k] = r[0]; h[2 + k] = r[1];
          r = __builtin_amdgcn_permlane32_swap(l[k], l[2 + k], false, false);
          l[k] = r[0]; l[2 + k] = r[1];
        }
        ph[t] = u32x4{h[0], h[1], h[2], h[3]};
        pl[t] = u32x4{l[0], l[1], l[2], l[3]};
      }
      // ---- O^T[d][query] += V^T P^T ----
#pragma unroll
      for (int t = 0; t < ET; ++t) {
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          const f16x8 vh = as_f16x8(Vs[(2 * sl + lh) * E + 32 * t + li]);
          const f16x8 vl = as_f16x8(Vs[4 * E + (2 * sl + lh) * E + 32 * t + li]);
          O[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, as_f16x8(ph[sl]), O[t], 0, 0, 0);
          O[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, as_f16x8(pl[sl]), O[t], 0, 0, 0);
          O[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, as_f16x8(ph[sl]), O[t], 0, 0, 0);
        }
        if ((t & 1) == 1) __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (more) v_store(Vn);
    __syncthreads();
  }
  }   // staging form
  float amax = 0.f;
  if (active) {
    const float inv = (1.0f / l_run) * o_un;
    float* ob = out + ((size_t)b * Etot + (size_t)h * E) * L;
#pragma unroll
    for (int t = 0; t < ET; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int d = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float o = O[t][r] * inv;
        ob[(size_t)d * L + q0 + li] = o;
        amax = fmaxf(amax, __builtin_fabsf(o));
      }
  }
  if (out_amax) ds::wave_commit_max_always(out_amax + b, amax);
}

// Pre-pass of the IMG form: one workgroup per (key tile, sample) writes the tile's K and V images
//   K [piece][d-group][key 32][8 d]   V [piece][key-group][d][8 keys]        (the LDS layouts above)
// with the split every attention workgroup would otherwise redo.  Reads K, V once (8 B/elt), writes as many bytes.
// ksrc / vsrc: the keys and the values [.., E tot, L] with batch strides k_bs / v_bs -- two thirds of qkv, or (ds_attention_h3_xkv)
// one tensor x for both, whose second walk over the same 32-key tile mostly hits cache.
// MH: one workgroup per (key tile, sample, head), images ordered by the (sample, head) row as the attention kernel reads them.
template <int ET, bool MH>
__global__ __launch_bounds__(NT) void k_attn_images(u32x4* __restrict__ kimg, u32x4* __restrict__ vimg,
                                                   const float* __restrict__ ksrc, size_t k_bs, const float* __restrict__ vsrc,
                                                   size_t v_bs, int L, int heads, const unsigned* k_amax, const unsigned* v_amax) {
  constexpr int E = 32 * ET, NDG = E / 8;
  constexpr int KITEMS = NDG * KB, VITEMS = E * 4;
  const int tid = threadIdx.x, kb = blockIdx.x, row = blockIdx.y, nkb = L / KB;
  const int b = MH ? row / heads : row, h = MH ? row - b * heads : 0;
  const float a_in = ds_epi::pow2f(ds_epi::act_exponent_of(ds_epi::act_bits(k_amax, b), -60, 60));        // the attention kernel's exponents
  const float v_in = ds_epi::pow2f(ds_epi::act_exponent_of(ds_epi::act_bits(v_amax, b), -120, 120));
  const float* Kt = ksrc + (size_t)b * k_bs + (size_t)h * E * L + (size_t)kb * KB;
  const float* Vt = vsrc + (size_t)b * v_bs + (size_t)h * E * L + (size_t)kb * KB;
  u32x4* Kd = kimg + ((size_t)row * nkb + kb) * (2 * KITEMS);
  u32x4* Vd = vimg + ((size_t)row * nkb + kb) * (2 * VITEMS);
  for (int e = tid; e < KITEMS; e += NT) {
    const int dg = e / KB, key = e % KB;
    u32x4 h, l;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      unsigned a, c;
      split2(Kt[(size_t)(8 * dg + 2 * k) * L + key] * a_in, Kt[(size_t)(8 * dg + 2 * k + 1) * L + key] * a_in, a, c);
      h[k] = a; l[k] = c;
    }
    Kd[e] = h;
    Kd[KITEMS + e] = l;
  }
  for (int e = tid; e < VITEMS; e += NT) {
    const int d = e >> 2, kg = e & 3;
    const float* p = Vt + (size_t)d * L + 8 * kg;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(p) * v_in, v1 = *reinterpret_cast<const f32x4*>(p + 4) * v_in;
    u32x4 h, l;
    unsigned a, c;
    split2(v0[0], v0[1], a, c); h[0] = a; l[0] = c;
    split2(v0[2], v0[3], a, c); h[1] = a; l[1] = c;
    split2(v1[0], v1[1], a, c); h[2] = a; l[2] = c;
    split2(v1[2], v1[3], a, c); h[3] = a; l[3] = c;
    Vd[kg * E + d] = h;
    Vd[VITEMS + kg * E + d] = l;
  }
}

// What the two kernels read: queries, keys and values [B, heads * E, L] by base and batch stride (in floats), and the exponent row
// [B] of each (NULL: none).
struct AttnSrc {
  const float *q, *k, *v;
  size_t q_bs, k_bs, v_bs;
  const unsigned *q_amax, *k_amax, *v_amax;
};
// qkv [B, 3 Etot, L] with in_amax [2][B]: one row for q and k, one for v
AttnSrc qkv_src(const float* qkv, int B, int Etot, int L, const unsigned* in_amax) {
  const size_t third = (size_t)Etot * L;
  return AttnSrc{qkv, qkv + third, qkv + 2 * third, 3 * third, 3 * third, 3 * third, in_amax, in_amax, in_amax ? in_amax + B : nullptr};
}

template <int ET, bool IMG, bool MH>
int launch_attn3h(float* out, const AttnSrc& a, void* workspace, int B, int heads, int L, float scale, unsigned* out_amax,
                  hipStream_t s) {
  constexpr int E = 32 * ET;                                              // the head width
  const size_t lds = (size_t)2 * (2 * (E / 8) * KB + 2 * 4 * E) * 16;    // K and V, double-buffered
  if (lds > 48 * 1024) {
    const int rc = ds::ensure_dynamic_lds<&k_attn3h<ET, IMG, MH>>((int)lds, "hipFuncSetAttribute(attn3h)");
    if (rc != DS_OK) return rc;
  }
  const int rows = B * heads;                                             // (sample, head) rows
  u32x4* kimg = nullptr;
  u32x4* vimg = nullptr;
  if (IMG) {
    kimg = reinterpret_cast<u32x4*>(workspace);
    vimg = kimg + (size_t)rows * L * (E / 4);                             // K images: rows * (L/32) tiles * 8E vectors
    hipLaunchKernelGGL((k_attn_images<ET, MH>), dim3(L / KB, rows), dim3(NT), 0, s, kimg, vimg, a.k, a.k_bs, a.v, a.v_bs, L, heads,
                       a.k_amax, a.v_amax);
    DS_CHECK_LAUNCH("ds_attention_h3 (images)");
  }
  dim3 g((L + 127) / 128, rows);
  hipLaunchKernelGGL((k_attn3h<ET, IMG, MH>), g, dim3(NT), lds, s, out, a.q, a.q_bs, kimg, vimg, L, heads, scale, RESCALE_T,
                     a.q_amax, a.k_amax, a.v_amax, out_amax);
  DS_CHECK_LAUNCH("ds_attention_h3");
  return DS_OK;
}

// Single head.  The image form reads a.q, a.k and a.v where they are; the other form reads K and V behind Q (a = qkv_src).
template <bool IMG>
int attention_h3_src(float* out, const AttnSrc& a, void* workspace, int B, int E, int L, unsigned* out_amax, hipStream_t s) {
  const float scale = (float)sqrt(1.0 / (double)E);
  switch (E) {
    case 32: return launch_attn3h<1, IMG, false>(out, a, workspace, B, 1, L, scale, out_amax, s);
    case 64: return launch_attn3h<2, IMG, false>(out, a, workspace, B, 1, L, scale, out_amax, s);
    case 128: return launch_attn3h<4, IMG, false>(out, a, workspace, B, 1, L, scale, out_amax, s);
    case 256: return launch_attn3h<8, IMG, false>(out, a, workspace, B, 1, L, scale, out_amax, s);
    default:
      ds::set_error("ds_attention_h3: E=%d unsupported (32, 64, 128, 256)", E);
      return DS_ERR_UNSUPPORTED;
  }
}

template <bool IMG>
int attention_h3(float* out, const float* qkv, void* workspace, int B, int E, int L, const unsigned* in_amax, unsigned* out_amax,
                 void* stream) {
  DS_REQUIRE(out && qkv, DS_ERR_NULL, "ds_attention_h3: NULL pointer");
  DS_REQUIRE(B >= 0 && E > 0 && L > 0, DS_ERR_SHAPE, "ds_attention_h3: bad shape B=%d E=%d L=%d", B, E, L);
  DS_REQUIRE(L % 32 == 0, DS_ERR_UNSUPPORTED, "ds_attention_h3: L=%d must be a multiple of 32", L);
  DS_REQUIRE(B < 65536 && L / 32 < 65536 * 32, DS_ERR_SHAPE, "ds_attention_h3: B=%d exceeds grid.y", B);
  DS_REQUIRE((reinterpret_cast<uintptr_t>(qkv) & 15u) == 0, DS_ERR_SHAPE, "ds_attention_h3: qkv must be 16-byte aligned");
  DS_REQUIRE(!IMG || (workspace && (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0), DS_ERR_NULL,
             "ds_attention_h3_ws: a 16-byte aligned workspace of ds_attention_h3_workspace_bytes(B, E, L) bytes is required");
  if (B == 0) return DS_OK;
  return attention_h3_src<IMG>(out, qkv_src(qkv, B, E, L, in_amax), workspace, B, E, L, out_amax, ds::as_stream(stream));
}

bool mfma_head_width(int d) { return d == 32 || d == 64 || d == 128 || d == 256; }

// Generic multi-head attention for head widths the MFMA tiling does not take (d not in {32, 64, 128, 256}) or sequence
// lengths that are not a multiple of 32: one wave per (query, sample, head), exact fp32.  The scores are one
// d-term FMA chain per key (lane = key); the softmax sum and every output channel are per-lane partial sums over the
// keys lane, lane + 64, ... combined by a butterfly -- a correctness path, whose error stays near torch's at L = 4096.
__global__ __launch_bounds__(64) void k_attn_heads_generic(float* out, const float* __restrict__ qkv, int d, int heads, int L,
                                                           float scale) {
  extern __shared__ float sm[];                      // [d] scaled query, then [L] probabilities
  float* qs = sm;
  float* ps = sm + d;
  const int q = blockIdx.x, row = blockIdx.y, lane = threadIdx.x;
  const int b = row / heads, h = row - b * heads, Etot = d * heads;
  const float* Qt = qkv + ((size_t)b * 3 * Etot + (size_t)h * d) * L;
  const float* Kt = Qt + (size_t)Etot * L;
  const float* Vt = Kt + (size_t)Etot * L;
  for (int c = lane; c < d; c += 64) qs[c] = Qt[(size_t)c * L + q] * scale;
  __syncthreads();
  float mx = -INFINITY;
  for (int k = lane; k < L; k += 64) {
    float sc = 0.f;
    for (int c = 0; c < d; ++c) sc = fmaf(qs[c], Kt[(size_t)c * L + k], sc);
    ps[k] = sc;
    mx = fmaxf(mx, sc);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int k = lane; k < L; k += 64) {
    const float p = expf(ps[k] - mx);
    ps[k] = p;
    sum += p;
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  __syncthreads();
  const float inv = 1.0f / sum;
  float* ob = out + ((size_t)b * Etot + (size_t)h * d) * L;
  for (int c = 0; c < d; ++c) {
    const float* v = Vt + (size_t)c * L;
    float acc = 0.f;
    for (int k = lane; k < L; k += 64) acc = fmaf(ps[k], v[k], acc);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) ob[(size_t)c * L + q] = acc * inv;
  }
}

int heads_generic(float* out, const float* qkv, int B, int E, int heads, int L, hipStream_t s) {
  const int d = E / heads;
  const size_t lds = (size_t)(d + L) * sizeof(float);
  DS_REQUIRE(lds <= 64 * 1024, DS_ERR_UNSUPPORTED, "ds_attention_heads_generic: d + L = %d is too large for the generic path", d + L);
  if (B == 0) return DS_OK;
  if (lds > 48 * 1024) {                             // set once, at the cap: the size varies with L
    const int rc = ds::ensure_dynamic_lds<&k_attn_heads_generic>(64 * 1024, "hipFuncSetAttribute(attn_heads_generic)");
    if (rc != DS_OK) return rc;
  }
  const float scale = (float)sqrt(1.0 / (double)d);
  hipLaunchKernelGGL(k_attn_heads_generic, dim3(L, B * heads), dim3(64), lds, s, out, qkv, d, heads, L, scale);
  DS_CHECK_LAUNCH("ds_attention_heads_generic");
  return DS_OK;
}

}  // namespace

extern "C" int ds_attention_h3(float* out, const float* qkv, int B, int E, int L, const unsigned* in_amax, unsigned* out_amax,
                               void* stream) {
  return attention_h3<false>(out, qkv, nullptr, B, E, L, in_amax, out_amax, stream);
}

extern "C" size_t ds_attention_h3_workspace_bytes(int B, int E, int L) {
  if (B <= 0 || E <= 0 || L <= 0) return 0;
  return (size_t)B * L * E * 8;                      // K and V images: 2 pieces x 2 bytes per element, each
}

extern "C" int ds_attention_h3_ws(float* out, const float* qkv, void* workspace, int B, int E, int L, const unsigned* in_amax,
                                  unsigned* out_amax, void* stream) {
  return attention_h3<true>(out, qkv, workspace, B, E, L, in_amax, out_amax, stream);
}

extern "C" int ds_attention_h3_xkv(float* out, const float* q, const float* x, void* workspace, int B, int E, int L,
                                   const unsigned* q_amax, const unsigned* k_amax, const unsigned* v_amax, unsigned* out_amax,
                                   void* stream, int flags) {
  DS_REQUIRE(out && q && x, DS_ERR_NULL, "ds_attention_h3_xkv: NULL pointer");
  DS_REQUIRE(flags == 0, DS_ERR_UNSUPPORTED, "ds_attention_h3_xkv: flags=%d must be 0", flags);
  DS_REQUIRE(B >= 0 && E > 0 && L > 0, DS_ERR_SHAPE, "ds_attention_h3_xkv: bad shape B=%d E=%d L=%d", B, E, L);
  DS_REQUIRE(L % 32 == 0, DS_ERR_UNSUPPORTED, "ds_attention_h3_xkv: L=%d must be a multiple of 32", L);
  DS_REQUIRE(B < 65536 && L / 32 < 65536 * 32, DS_ERR_SHAPE, "ds_attention_h3_xkv: B=%d exceeds grid.y", B);
  DS_REQUIRE(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(x)) & 15u) == 0, DS_ERR_SHAPE,
             "ds_attention_h3_xkv: q and x must be 16-byte aligned");
  DS_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, DS_ERR_NULL,
             "ds_attention_h3_xkv: a 16-byte aligned workspace of ds_attention_h3_workspace_bytes(B, E, L) bytes is required");
  if (B == 0) return DS_OK;
  const size_t bs = (size_t)E * L;
  return attention_h3_src<true>(out, AttnSrc{q, x, x, bs, bs, bs, q_amax, k_amax, v_amax}, workspace, B, E, L, out_amax,
                                ds::as_stream(stream));
}

extern "C" size_t ds_attention_h3_heads_workspace_bytes(int B, int E, int heads, int L) {
  if (B <= 0 || E <= 0 || L <= 0 || heads <= 0 || E % heads || !mfma_head_width(E / heads) || L % 32) return 0;
  return (size_t)B * L * E * 8;                      // the images of every (sample, head) row: as many bytes as one head of E
}

extern "C" int ds_attention_h3_heads(float* out, const float* qkv, void* workspace, int B, int E, int heads, int L,
                                     const unsigned* in_amax, unsigned* out_amax, void* stream) {
  DS_REQUIRE(out && qkv, DS_ERR_NULL, "ds_attention_h3_heads: NULL pointer");
  DS_REQUIRE(B >= 0 && E > 0 && L > 0 && heads > 0, DS_ERR_SHAPE, "ds_attention_h3_heads: bad shape B=%d E=%d heads=%d L=%d",
             B, E, heads, L);
  DS_REQUIRE(E % heads == 0, DS_ERR_SHAPE, "ds_attention_h3_heads: E=%d is not a multiple of heads=%d", E, heads);
  DS_REQUIRE((size_t)B * heads < 65536, DS_ERR_SHAPE, "ds_attention_h3_heads: B*heads=%lld exceeds grid.y", (long long)B * heads);
  if (heads == 1) {                                  // the single-head entry points, unchanged
    if (workspace) return attention_h3<true>(out, qkv, workspace, B, E, L, in_amax, out_amax, stream);
    return attention_h3<false>(out, qkv, nullptr, B, E, L, in_amax, out_amax, stream);
  }
  if (B == 0) return DS_OK;
  const int d = E / heads;
  const float scale = (float)sqrt(1.0 / (double)d);
  hipStream_t s = ds::as_stream(stream);
  if (!mfma_head_width(d) || L % 32) {
    DS_REQUIRE(out_amax == nullptr, DS_ERR_UNSUPPORTED,
               "ds_attention_h3_heads: out_amax needs a head width in {32, 64, 128, 256} and L a multiple of 32 (reduce with "
               "ds_absmax_rows instead)");
    return heads_generic(out, qkv, B, E, heads, L, s);
  }
  DS_REQUIRE((reinterpret_cast<uintptr_t>(qkv) & 15u) == 0, DS_ERR_SHAPE, "ds_attention_h3_heads: qkv must be 16-byte aligned");
  DS_REQUIRE(!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) == 0, DS_ERR_SHAPE,
             "ds_attention_h3_heads: the workspace must be 16-byte aligned");
  const bool img = workspace != nullptr;
  const AttnSrc a = qkv_src(qkv, B, E, L, in_amax);
  switch (d) {
    case 32: return img ? launch_attn3h<1, true, true>(out, a, workspace, B, heads, L, scale, out_amax, s)
                        : launch_attn3h<1, false, true>(out, a, nullptr, B, heads, L, scale, out_amax, s);
    case 64: return img ? launch_attn3h<2, true, true>(out, a, workspace, B, heads, L, scale, out_amax, s)
                        : launch_attn3h<2, false, true>(out, a, nullptr, B, heads, L, scale, out_amax, s);
    case 128: return img ? launch_attn3h<4, true, true>(out, a, workspace, B, heads, L, scale, out_amax, s)
                         : launch_attn3h<4, false, true>(out, a, nullptr, B, heads, L, scale, out_amax, s);
    default: return img ? launch_attn3h<8, true, true>(out, a, workspace, B, heads, L, scale, out_amax, s)
                        : launch_attn3h<8, false, true>(out, a, nullptr, B, heads, L, scale, out_amax, s);
  }
}

extern "C" int ds_attention_heads_generic(float* out, const float* qkv, int B, int E, int heads, int L, void* stream) {
  DS_REQUIRE(out && qkv, DS_ERR_NULL, "ds_attention_heads_generic: NULL pointer");
  DS_REQUIRE(B >= 0 && E > 0 && L > 0 && heads > 0, DS_ERR_SHAPE, "ds_attention_heads_generic: bad shape B=%d E=%d heads=%d L=%d",
             B, E, heads, L);
  DS_REQUIRE(E % heads == 0, DS_ERR_SHAPE, "ds_attention_heads_generic: E=%d is not a multiple of heads=%d", E, heads);
  DS_REQUIRE((size_t)B * heads < 65536, DS_ERR_SHAPE, "ds_attention_heads_generic: B*heads=%lld exceeds grid.y",
             (long long)B * heads);
  return heads_generic(out, qkv, B, E, heads, L, ds::as_stream(stream));
}
