// codenet_pointwise.hip -- the pointwise (1x1) convolutions of the fused schedule on a channels-last activation
// A [M][C] -> R [M][Co] (gfx950): f32 MFMA (pw3, pws), int8 MFMA on codes (pwi8, pwi8h, pwi8s) and the exact bf16 x 3
// split (pwb3, pwd3), each with bias / BN, ReLU and the QuantAct range of its output in the epilogue.  One launcher,
// cdn::launch_pointwise, shared by the stage schedule (codenet_fused.hip), the layers around it (codenet_layers.hip goes
// through the entry points below) and the detection heads.
#include "cdn_common.h"

#include <algorithm>
#include <type_traits>

// In-kernel phase stamps (-DCDN_STAMPS, see codenet_fused.hip): this file owns region 2; a __device__ array cannot be
// shared between translation units without -fgpu-rdc, so cdn_debug_read_stamps gathers it through the two functions.
#ifdef CDN_STAMPS
__device__ unsigned long long cdn_pw_stamps[2048 * 8];
#define CDN_STAMPR(R, I)                                                                              \
  do {                                                                                                \
    static_assert((R) == 2, "the pointwise kernels stamp region 2");                                  \
    if (threadIdx.x == 0)                                                                             \
      cdn_pw_stamps[((blockIdx.y * gridDim.x + blockIdx.x) & 2047) * 8 + (I)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
int cdn::read_pointwise_stamps(unsigned long long *host_dst) {
  return (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(cdn_pw_stamps), sizeof(unsigned long long) * 2048 * 8);
}
int cdn::clear_pointwise_stamps() {
  void *p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(cdn_pw_stamps)) != hipSuccess) return 1;
  return (int)hipMemset(p, 0, sizeof(unsigned long long) * 2048 * 8);
}
#else
#define CDN_STAMPR(R, I) do { } while (0)
#endif

namespace {

using cdn::fake_quant;
using cdn::glds16;
using cdn::kMaxGrid;
using cdn::lds_addr_uniform;

// ------------------------------------------------------------------------------------------
// pw2: R[m][co] = act( sum_c Aq[m][c] * Wp[co][c] + ... ),  m = n*HW + p  (channels-last both
// sides, the batch folds into M).  f32 MFMA 32x32x2 (exact f32).  A is optionally
// fake-quantised while it is staged.  Tile 128 (m) x BN (co) x 16 (k); 4 waves stacked in m,
// each holding BN/32 accumulators.  LDS rows have an odd stride (17) so the operand read
// `[row = lane&31][k = lane>>5]` is conflict-free with K-contiguous global loads on both sides.
// MFMA maps: A[i=l&31][k=l>>5], B[k=l>>5][j=l&31], D col=l&31, row=(r&3)+8*(r>>2)+4*(l>>5).
// Here i <-> pixel, j <-> co, so every accumulator register stores 128 contiguous bytes.
// ------------------------------------------------------------------------------------------
using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kPwBK = 32, kPwLD = 33;

// Software-pipelined: while the MFMAs of k-tile t run out of LDS buffer t&1, the global loads of
// k-tile t+1 are in flight into registers; they are fake-quantised (A) and written to buffer
// (t+1)&1 after the MFMAs, so there is ONE barrier per 32-deep k-tile and the load latency, the
// quantisation VALU work and the LDS writes all sit behind matrix work.  All operand fragments
// of a k-tile are read from LDS up front, then the MFMAs issue back to back.
// Workgroup = 4 waves arranged WGM (m) x 4/WGM (n); every wave owns TM x TN accumulators of 32x32.
// FAST: C % 32 == 0 (no k guards, 16-byte loads); otherwise guarded scalar loads.
template <int BM, int BN, int WGM, bool AQ, bool FAST>
__global__ void __launch_bounds__(256)
pw3_kernel(const float *__restrict__ A, const unsigned *__restrict__ aq,
           const float *__restrict__ Wp, const float *__restrict__ bias,
           const float *__restrict__ ep_scale, const float *__restrict__ ep_shift,
           float *__restrict__ R, cdn::QUpdate qu, long M, int C, int Co, int relu,
           int only_if_wide, int lda, int ldo) {
  if (only_if_wide && !aq[6]) return;   // fallback launch behind pwi8_kernel: nothing to do
  constexpr int WGN = 4 / WGM;
  constexpr int TM = BM / (WGM * 32), TN = BN / (WGN * 32);
  constexpr int AI = BM * 8 / 256, BI = BN * 8 / 256;   // float4 loads per thread per k-tile
  static_assert(TM >= 1 && TN >= 1 && AI >= 1 && BI >= 1, "tile too small for 256 threads");
  __shared__ float As[2][BM * kPwLD];
  __shared__ float Bs[2][BN * kPwLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave / WGN) * TM * 32, wn = (wave % WGN) * TN * 32;
  float qs = 1.f, qz = 0.f;
  if (AQ) {
    qs = reinterpret_cast<const float *>(aq)[2];
    qz = reinterpret_cast<const float *>(aq)[3];
  }
  // workgroups walk the (m, n) tiles with a grid stride: the full-size launch visits one tile each,
  // the fallback launch behind pwi8_kernel is a small grid (an EMPTY full-size launch still costs
  // 4.3 us of workgroup dispatch inside the graph)
  const long ntm = (M + BM - 1) / BM, ntiles = ntm * ((Co + BN - 1) / BN);
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
  const long m0 = (tile % ntm) * BM;
  const int n0 = (int)(tile / ntm) * BN;
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16){0};
  const int lr = tid >> 3, lk = (tid & 7) * 4;   // staging: row lr + 32*i, k quad lk
  const bool vec4 = !FAST && (C & 3) == 0 && (lda & 3) == 0 &&
                    ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(Wp)) & 15) == 0;
  const bool vec2 = !FAST && !vec4 && (C & 1) == 0 && (lda & 1) == 0 &&
                    (reinterpret_cast<uintptr_t>(A) & 7) == 0;
  float4 a[AI], b[BI];
  // FAST path: rows beyond M / Co are clamped to a valid row (their results are never stored)
  const float *arow[AI];
  const float *brow[BI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    long m = m0 + lr + 32 * i;
    if (m > M - 1) m = M - 1;
    arow[i] = A + m * lda + lk;
  }
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    int co = n0 + lr + 32 * i;
    if (co > Co - 1) co = Co - 1;
    brow[i] = Wp + (long)co * C + lk;
  }

  auto load_tile = [&](int k0) {
    if (FAST) {
#pragma unroll
      for (int i = 0; i < AI; ++i) a[i] = *reinterpret_cast<const float4 *>(arow[i] + k0);
#pragma unroll
      for (int i = 0; i < BI; ++i) b[i] = *reinterpret_cast<const float4 *>(brow[i] + k0);
    } else if (vec4) {      // C % 4 == 0, 16-byte aligned rows: whole quads are in or out of the k range
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      const bool in = k0 + lk < C;
#pragma unroll
      for (int i = 0; i < AI; ++i) a[i] = in ? *reinterpret_cast<const float4 *>(arow[i] + k0) : z;
#pragma unroll
      for (int i = 0; i < BI; ++i) b[i] = in ? *reinterpret_cast<const float4 *>(brow[i] + k0) : z;
    } else {
      if (vec2) {           // C % 2 == 0, 8-byte aligned rows (a unit's second half at channel 58)
        const float2 z = make_float2(0.f, 0.f);
        const int k = k0 + lk;
#pragma unroll
        for (int i = 0; i < AI; ++i) {
          const float2 lo = (k < C) ? *reinterpret_cast<const float2 *>(arow[i] + k0) : z;
          const float2 hi = (k + 2 < C) ? *reinterpret_cast<const float2 *>(arow[i] + k0 + 2) : z;
          a[i] = make_float4(lo.x, lo.y, hi.x, hi.y);
        }
      } else {
#pragma unroll
        for (int i = 0; i < AI; ++i) {
          const int k = k0 + lk;
          a[i].x = (k + 0 < C) ? arow[i][k0 + 0] : 0.0f;
          a[i].y = (k + 1 < C) ? arow[i][k0 + 1] : 0.0f;
          a[i].z = (k + 2 < C) ? arow[i][k0 + 2] : 0.0f;
          a[i].w = (k + 3 < C) ? arow[i][k0 + 3] : 0.0f;
        }
      }
#pragma unroll
      for (int i = 0; i < BI; ++i) {
        const int k = k0 + lk;
        b[i].x = (k + 0 < C) ? brow[i][k0 + 0] : 0.0f;
        b[i].y = (k + 1 < C) ? brow[i][k0 + 1] : 0.0f;
        b[i].z = (k + 2 < C) ? brow[i][k0 + 2] : 0.0f;
        b[i].w = (k + 3 < C) ? brow[i][k0 + 3] : 0.0f;
      }
    }
  };
  auto store_tile = [&](int buf, int k0) {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      float4 v = a[i];
      if (AQ) {
        if (FAST) {
          v.x = fake_quant(v.x, qs, qz);
          v.y = fake_quant(v.y, qs, qz);
          v.z = fake_quant(v.z, qs, qz);
          v.w = fake_quant(v.w, qs, qz);
        } else {   // keep the zero padding of the k tail exact
          const int k = k0 + lk;
          v.x = (k + 0 < C) ? fake_quant(v.x, qs, qz) : 0.0f;
          v.y = (k + 1 < C) ? fake_quant(v.y, qs, qz) : 0.0f;
          v.z = (k + 2 < C) ? fake_quant(v.z, qs, qz) : 0.0f;
          v.w = (k + 3 < C) ? fake_quant(v.w, qs, qz) : 0.0f;
        }
      }
      float *p = &As[buf][(lr + 32 * i) * kPwLD + lk];
      p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      float *p = &Bs[buf][(lr + 32 * i) * kPwLD + lk];
      p[0] = b[i].x; p[1] = b[i].y; p[2] = b[i].z; p[3] = b[i].w;
    }
  };

  load_tile(0);
  store_tile(0, 0);
  __syncthreads();
  const int nk = (C + kPwBK - 1) / kPwBK;
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    if (t + 1 < nk) load_tile((t + 1) * kPwBK);
    // all fragments of this k-tile, then the MFMAs back to back
    float av[kPwBK / 2][TM], bv[kPwBK / 2][TN];
#pragma unroll
    for (int kk = 0; kk < kPwBK / 2; ++kk) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
        av[kk][i] = As[buf][(wm + i * 32 + (lane & 31)) * kPwLD + 2 * kk + (lane >> 5)];
#pragma unroll
      for (int j = 0; j < TN; ++j)
        bv[kk][j] = Bs[buf][(wn + j * 32 + (lane & 31)) * kPwLD + 2 * kk + (lane >> 5)];
    }
#pragma unroll
    for (int kk = 0; kk < kPwBK / 2; ++kk)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk][i], bv[kk][j], acc[i][j], 0, 0, 0);
    if (t + 1 < nk) store_tile(buf ^ 1, (t + 1) * kPwBK);
    __syncthreads();
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int co = n0 + wn + j * 32 + (lane & 31);
    float bsv = 0.f, es = 1.f, eh = 0.f;
    if (co < Co) {
      if (bias) bsv = bias[co];
      if (ep_scale) {
        es = ep_scale[co];
        eh = ep_shift[co];
      }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < M && co < Co) {
          float v = acc[i][j][r] + bsv;
          if (ep_scale) v = fmaf(v, es, eh);
          if (relu) v = cdn::relu_keep_nan(v);
          R[m * ldo + co] = v;
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          has_nan |= (v != v);
        }
      }
  }
  }   // tile loop
  if (qu.tracks())   // (block_minmax_finish syncs before reusing As as scratch)
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.x, gridDim.x, qu, &As[0][0]);
}

// ------------------------------------------------------------------------------------------
// pws: the f32 pointwise conv for launches with FEW output tiles (round 5; cfg2's stage 0: M = 2048 rows, K = 1024,
// Co = 256 -- pw3_kernel's 64 x 128 tiles are 64 workgroups on 256 CUs, each a chain of 32 dependent k tiles with 32
// MFMAs of 64 cycles per wave and tile: 27 us of matrix time on a quarter of the SIMDs, 47 us measured).
// Every WAVE owns one 32 (m) x 32*TN (co) output tile over a k range and runs its own pipeline -- no workgroup barrier
// in the k loop: 32-k windows of both operands (32 + 32 TN rows x 128 B) are fetched by LDS-DMA
// (global_load_lds_dwordx4: 8 lanes per row = whole 128-byte lines, no VGPRs) into a wave-private LDS ring R - 1
// windows ahead, read back in MFMA layout (lane (i = l & 31, h = l >> 5) takes the 16 consecutive k values
// [16 h, 16 h + 16) of row i as four ds_read_b128; a sum over k does not care which of the two k slots of
// v_mfma_f32_32x32x2_f32 a k lands in, only that A and B agree) and multiplied.  The DMA's LDS side is lane-linear
// (rows of exactly 128 B), so the 16-byte chunks of a row are stored XOR-swizzled -- chunk c of row r at position
// c ^ ((r >> 1) & 7), applied to the per-lane SOURCE address -- which makes the fragment reads conflict-free.
// (First form of this kernel, measured: lanes loading their 64-byte operand pieces straight from global memory -- every
// load instruction touched 32 lines for 16 bytes each; 15.3 us at cfg2's stage 0 and SLOWER, 18.3 us, with three windows
// in flight instead of one: bound by the texture path's line touches, not by latency or matrix time.)
// The four waves of a workgroup are
//   KS = 4: the four quarters of K of ONE tile (wave w: [w K/4, (w+1) K/4)); the partial tiles are added through LDS in
//           a FIXED order ((w0 + w1) + (w2 + w3)) -- for launches whose tiles alone would not give every SIMD a wave;
//   KS = 1: four consecutive m tiles, the whole K each; accumulators go straight to the epilogue.
// The launcher picks the widest tile and the least splitting that still gives >= 4 waves per CU.  Reproducible bit for
// bit from call to call; against pw3_kernel the k order differs (fp32 re-association; the fp32 path's parity bound is
// 1e-3 against the oracle).  Workgroups that share A rows (the co tiles of one m block) get ids 8 apart = the same XCD
// under round-robin dispatch, so an A block is fetched into one L2.
// Needs K % (32 KS) == 0 and 16-byte aligned rows; plain f32 operands (no quantise-on-load).
// ------------------------------------------------------------------------------------------
// Sum over the 32 lanes of each wave half (pws_sum32: the total arrives in lanes 16-31 / 48-63) or over the wave
// (pws_sum64: lanes 48-63) on the VALU's DPP path -- quad_perm xor 1, xor 2, row_ror 4, row_ror 8, row_bcast15
// [, row_bcast31]: five / six moves + adds per value in ONE fixed order, where a __shfl_xor tree is as many ds_bpermute
// round trips through the LDS crossbar (measured: +2.8 us on a 13-us launch for 16 rows x 5 steps per wave).
__device__ __forceinline__ float pws_dpp(float v, const int ctrl) {
  switch (ctrl) {      // (the DPP control is an immediate)
    case 0: return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
    case 1: return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));
    case 2: return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));
    case 3: return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));
    case 4: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));
    default: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));
  }
}
__device__ __forceinline__ float pws_sum32(float v) {
  v += pws_dpp(v, 0);
  v += pws_dpp(v, 1);
  v += pws_dpp(v, 2);
  v += pws_dpp(v, 3);       // every lane: the sum of its 16-lane row
  v += pws_dpp(v, 4);       // rows 1 and 3: + the row in front of them
  return v;
}
__device__ __forceinline__ float pws_sum64(float v) {
  v = pws_sum32(v);
  v += pws_dpp(v, 5);       // row 3: + lane 31's total of the first half
  return v;
}

constexpr int kPwsLD = 72;      // floats per LDS row of a partial tile: the two lane halves (rows 4 apart) hit disjoint banks
template <int TN> struct PwsGeom {
  static constexpr int R = TN == 2 ? 3 : 4;                 // ring slots per wave
  static constexpr int kSlot = (32 + 32 * TN) * 128;        // bytes per window: A rows, then B rows, 128 B each
  static constexpr int kRing = R * kSlot;
  static constexpr int kLds = 4 * kRing;                    // 144 KB (TN = 2) / 128 KB (TN = 1)
};

template <int TN, int KS>
__global__ void __launch_bounds__(256)
pws_kernel(const float *__restrict__ A, const float *__restrict__ Wp, const float *__restrict__ bias,
           const float *__restrict__ ep_scale, const float *__restrict__ ep_shift, float *__restrict__ R,
           cdn::QUpdate qu, long M, int K, int Co, int relu, int lda, int ldo, const float *__restrict__ nws,
           float *__restrict__ sparts) {
  // nws / sparts (round 6, chained fp32 stages): nws [Co] = the NEXT stage's conv_scale weights; this workgroup's column
  // tile leaves sparts[nt][m] = sum over its columns of out[m][co] * nws[co] (lane tree in a fixed order), which the
  // next stage's gather sums over the tiles in plane order (cdn::ScaleFromSums::fparts) -- the separate scale launch of
  // a stage whose input has no QuantAct in front of it (the fp32 model) is gone.
  using G = PwsGeom<TN>;
  constexpr int BN = 32 * TN;
  constexpr int BM = KS == 4 ? 32 : 128;          // rows of A per workgroup
  constexpr int NL = 4 + 4 * TN;                  // DMA instructions per window and wave
  static_assert(BN <= 64 && (KS == 1 || KS == 4) && 32 * kPwsLD * 4 <= G::kRing, "partial tile aliases the ring");
  extern __shared__ float4 pws_lds[];
  char *lds = reinterpret_cast<char *>(pws_lds);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 31, h = lane >> 5;
  const int ntm = (int)((M + BM - 1) / BM), ntn = (Co + BN - 1) / BN;
  // (m block, n tile) of this workgroup: within the part of the m range that is a multiple of 8 blocks, the n tiles of
  // one m block are 8 ids apart (same XCD); the remainder is mapped plainly.  A bijection on the grid.
  int mt, nt;
  {
    const int b = blockIdx.x, full_m = ntm & ~7, full = full_m * ntn;
    if (b < full) {
      mt = (b & 7) + 8 * (b / (8 * ntn));
      nt = (b >> 3) % ntn;
    } else {
      const int rem = ntm - full_m, q = b - full;
      mt = full_m + q % rem;
      nt = q / rem;
    }
  }
  const long m0 = (long)mt * BM + (KS == 4 ? 0 : 32 * w);      // first row of this WAVE's tile (wave-uniform)
  const int n0 = nt * BN;
  const int Kw = KS == 4 ? K >> 2 : K, kbase = KS == 4 ? w * Kw : 0;
  // ---- DMA side: lane <-> (row 8 u + (l >> 3), 16-byte chunk l & 7) of instruction u; rows beyond M / Co are clamped
  const float *abase = A + (m0 < M ? m0 : M - 1) * lda + kbase;          // wave-uniform bases, 32-bit lane offsets
  const float *bbase = Wp + (long)n0 * K + kbase;
  const int dr = lane >> 3, dc = lane & 7;
  unsigned aoff[4], boff[TN][4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = 8 * u + dr;
    const long rmax = M - 1 - m0;                                         // last valid row of this tile (may be < 0)
    const int rl = (int)(rmax < 0 ? 0 : (row < rmax ? row : rmax));
    aoff[u] = (unsigned)rl * (unsigned)lda * 4u + (unsigned)((dc ^ ((row >> 1) & 7)) * 16);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int cmax = Co - 1 - n0 - 32 * j;
      const int cl = cmax < 0 ? -32 * j : (row < cmax ? row : cmax);      // (cmax < 0: the whole co tile is padding)
      boff[j][u] = (unsigned)(32 * j + cl) * (unsigned)K * 4u + (unsigned)((dc ^ ((row >> 1) & 7)) * 16);
    }
  }
  const unsigned ring = lds_addr_uniform(lds) + (unsigned)w * G::kRing;
  auto issue = [&](int t) {
    const unsigned dst = ring + (unsigned)(t % G::R) * G::kSlot, koff = (unsigned)t * 128u;
#pragma unroll
    for (int u = 0; u < 4; ++u) glds16(abase, aoff[u] + koff, dst + u * 1024);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int u = 0; u < 4; ++u) glds16(bbase, boff[j][u] + koff, dst + 4096 + j * 4096 + u * 1024);
  };
  // ---- MFMA side
  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) acc[j] = (f32x16){0};
  const char *wring = lds + w * G::kRing;
  const int frow = i * 128, fsw = (i >> 1) & 7;
  const int nit = Kw >> 5;
  int issued = 0;
  for (; issued < G::R - 1 && issued < nit; ++issued) issue(issued);
  for (int t = 0; t < nit; ++t) {
    if (issued < nit) issue(issued++);
    // windows t .. issued - 1 are in flight (NL DMAs each, completing in order): wait for window t
    switch (issued - 1 - t) {
      case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
      case 1: if (NL == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
      case 2: if (NL == 12) asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;      // (TN = 1, three windows behind this one)
    }
    const char *slot = wring + (t % G::R) * G::kSlot;
    float4 fa[4], fb[TN][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pos = ((4 * h + q) ^ fsw) * 16;
      fa[q] = *reinterpret_cast<const float4 *>(slot + frow + pos);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j][q] = *reinterpret_cast<const float4 *>(slot + 4096 + j * 4096 + frow + pos);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float ae[4] = {fa[q].x, fa[q].y, fa[q].z, fa[q].w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const float be = e == 0 ? fb[j][q].x : e == 1 ? fb[j][q].y : e == 2 ? fb[j][q].z : fb[j][q].w;
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(ae[e], be, acc[j], 0, 0, 0);
        }
    }
  }
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  if (KS == 4) {
    // ---- the four k slices of the tile through LDS (each wave's partial tile over its own, drained ring), added in a
    //      fixed order
    float *Pw = reinterpret_cast<float *>(lds + w * G::kRing);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        Pw[((r & 3) + 8 * (r >> 2) + 4 * h) * kPwsLD + j * 32 + i] = acc[j][r];
    __syncthreads();
    constexpr int RPT = 32 * BN / 256;            // rows per thread: thread <-> one column, RPT consecutive rows
    const int col = tid % BN, r0 = (tid / BN) * RPT;
    const int co = n0 + col;
    float bsv = 0.f, es = 1.f, eh = 0.f;
    if (co < Co) {
      if (bias) bsv = bias[co];
      if (ep_scale) {
        es = ep_scale[co];
        eh = ep_shift[co];
      }
    }
    const float *P0 = reinterpret_cast<const float *>(lds), *P1 = reinterpret_cast<const float *>(lds + G::kRing),
                *P2 = reinterpret_cast<const float *>(lds + 2 * G::kRing),
                *P3 = reinterpret_cast<const float *>(lds + 3 * G::kRing);
    float v[RPT];
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
      const int o = (r0 + rr) * kPwsLD + col;
      v[rr] = ((P0[o] + P1[o]) + (P2[o] + P3[o])) + bsv;
      if (ep_scale) v[rr] = fmaf(v[rr], es, eh);
      if (relu) v[rr] = cdn::relu_keep_nan(v[rr]);
    }
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr)
      if (m0 + r0 + rr < M && co < Co) {
        R[(m0 + r0 + rr) * ldo + co] = v[rr];
        mn = fminf(mn, v[rr]);
        mx = fmaxf(mx, v[rr]);
        has_nan |= (v[rr] != v[rr]);
      }
    if (sparts) {           // (wave-uniform) thread <-> column: the BN lanes of a row group hold one row each step
      const float wn = co < Co ? nws[co] : 0.0f;
#pragma unroll
      for (int rr = 0; rr < RPT; ++rr) {
        float t = co < Co ? v[rr] * wn : 0.0f;
        t = BN == 64 ? pws_sum64(t) : pws_sum32(t);
        if (col == BN - 1 && m0 + r0 + rr < M) sparts[(long)nt * M + m0 + r0 + rr] = t;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int co = n0 + j * 32 + i;
      float bsv = 0.f, es = 1.f, eh = 0.f;
      if (co < Co) {
        if (bias) bsv = bias[co];
        if (ep_scale) {
          es = ep_scale[co];
          eh = ep_shift[co];
        }
      }
      const float wn = (sparts && co < Co) ? nws[co] : 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long m = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        float v = acc[j][r] + bsv;
        if (ep_scale) v = fmaf(v, es, eh);
        if (relu) v = cdn::relu_keep_nan(v);
        if (m < M && co < Co) {
          R[m * ldo + co] = v;
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          has_nan |= (v != v);
        }
        // (the accumulator is free now: it carries this lane's term of the row's partial sum, the 32-column sub-tiles in
        // j order)
        if (sparts) {
          const float term = co < Co ? v * wn : 0.0f;
          acc[0][r] = j == 0 ? term : acc[0][r] + term;
        }
      }
    }
    if (sparts) {           // lane <-> column i of the 32-column sub-tiles; the two lane halves hold different rows
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float t = pws_sum32(acc[0][r]);
        const long m = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (i == 31 && m < M) sparts[(long)nt * M + m] = t;
      }
    }
  }
  if (qu.tracks()) {
    __syncthreads();      // (the scratch of block_minmax_finish aliases wave 0's ring / partial tile)
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.x, gridDim.x, qu, reinterpret_cast<float *>(lds));
  }
}

// ------------------------------------------------------------------------------------------
// pwi8: the W4A8 pointwise conv on INTEGER CODES with v_mfma_i32_32x32x32_i8.
//   levels   L = q + zp,  q = round(sc*d - zp)  (QuantAct codes, NOT clamped by the reference)
//   weights  qw in [-8, 7], W' = qw / sw[co]     (per-channel symmetric 4 bit)
//   y[m][co] = sum_c (L/sc)*(qw/sw) + b = (sum_c L*qw) / (sc*sw[co]) + b      -- exact integer sum
// a = L - 128 is in [-128,127] for in-range data but the tracked range lags the batch, so codes a
// few LSB outside int8 are routine.  Instead of a second accumulator the K dimension is doubled:
//   a = 16*a1 + a0,  a0 in [0,15], a1 in [-128,127]   (|a| <= 2039: x up to 8x outside the range;
//                                                     beyond that the code saturates)
//   sum a*qw = sum a0*qw + sum a1*(16*qw),   16*qw in [-128,112] is still int8.
// sum L*qw = sum a*qw + 128*colsum(qw).  All integer arithmetic is exact; the only roundings are
// the final fp32 scale and bias add.  Operand lane map: lane (r = l&31, h = l>>5) supplies 16
// consecutive k bytes [16h, 16h+16) of its row's 32-byte k-step for BOTH operands (any k order works as long as A
// and B agree; checked with exact integer data, tools/probes/probe_i8.hip); C/D map as f32.
// WB = 8 (W8A8: qw in [-128, 127], the caller says so with CDN_W_CODES_8BIT): 16*qw no longer fits a byte, so the factor
// 16 moves off the weight plane -- the a1 products get an accumulator of their own and the epilogue forms
// acc_lo + 16*acc_hi in int32 in front of the unchanged expression.  Bound (state word 6 clear, C <= 4096, which the
// launcher checks): |sum a0*qw| <= 15*128*4096 < 2^23, 16*|sum a1*qw| <= 16*128*128*4096 = 2^30, their sum is
// sum (L-128)*qw with |L-128| <= 2040: <= 2040*128*4096 = 1 069 547 520, and |128*colsum| <= 128*128*4096 = 2^26 on top:
// every intermediate stays below 2^31.  No B1 plane in LDS.  WB = 4 is the code it was.
// Tried in round 3 and removed (source kept in tools/probes/archive/pwi8r_kernel.inc): the same kernel with the raw fp32 A / int8 B tiles fetched by
// global_load_lds into a 3-slot LDS ring two tiles ahead (counted vmcnt, no compiler-visible load in the k loop,
// bit-identical results) -- stage 0 (K = 1024) 39.7 vs 38.3 us, stage 1 (K = 256, only two 72-KB workgroups per CU
// instead of four) 31.6 vs 23.6 us: the k loop is not waiting for its global loads.
// ------------------------------------------------------------------------------------------
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;
constexpr int kI8LD = 48;   // bytes per LDS row: 32 k + 16 pad -> conflict-free ds_read_b128
constexpr int kMixedMaxC = 512;   // channels of a mixed-generation input (per-channel state table in LDS)

// The rare branch of the int8 pointwise kernels: this batch's codes are too wide for the nibble split (state[6]), so
// it runs on f32 MFMA with the fake-quantised weights Wp.  As / Bs: BM x 17 / BN x 17 floats of LDS, red: scratch of
// block_minmax_finish.
template <int BM, int BN, int WGM>
__device__ __forceinline__ void pwi8_wide_path(const float *__restrict__ A, const float *__restrict__ Wp,
                                               const float *__restrict__ bias, float *__restrict__ R,
                                               const cdn::QUpdate &qu, long M, int C, int Co, int relu, int lda,
                                               int ldo, const int *__restrict__ omap, float qs, float qz,
                                               float *As, float *Bs, float *red, long m0, int n_first, int nrep, int pidx,
                                               int npart) {
  // the workgroup's tile: rows [m0, m0 + BM), nrep column tiles of BN from n_first on, walked one after the other
  // (pwi8s_kernel: all its columns); Co: one past the last column it may touch; pidx / npart: its range partial
  constexpr int WGN = 4 / WGM;
  constexpr int TM = BM / (WGM * 32), TN = BN / (WGN * 32);
  constexpr int LDF = 17;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave / WGN) * TM * 32, wn = (wave % WGN) * TN * 32;
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  for (int rep = 0; rep < nrep; ++rep) {
    const int n0 = n_first + rep * BN;
    if (rep) __syncthreads();
    f32x16 accf[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) accf[i][j] = (f32x16){0};
    for (int k0 = 0; k0 < C; k0 += 16) {
      for (int q = tid; q < (BM + BN) * 4; q += 256) {     // one k quad of one row per item
        const bool isA = q < BM * 4;
        const int row = (isA ? q : q - BM * 4) >> 2, kq = (q & 3) * 4;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (isA) {
          const long m = min(m0 + row, M - 1);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k0 + kq + e < C) v[e] = fake_quant(A[m * lda + k0 + kq + e], qs, qz);
        } else {
          const int co = min(n0 + row, Co - 1);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k0 + kq + e < C) v[e] = Wp[(long)co * C + k0 + kq + e];
        }
        float *dst = (isA ? As : Bs) + row * LDF + kq;
#pragma unroll
        for (int e = 0; e < 4; ++e) dst[e] = v[e];
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        float av[TM], bv[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) av[i] = As[(wm + i * 32 + (lane & 31)) * LDF + 2 * kk + (lane >> 5)];
#pragma unroll
        for (int j = 0; j < TN; ++j) bv[j] = Bs[(wn + j * 32 + (lane & 31)) * LDF + 2 * kk + (lane >> 5)];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            accf[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], accf[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int co = n0 + wn + j * 32 + (lane & 31);
      const float bsv = (co < Co && bias) ? bias[co] : 0.f;
      const int oc = (co < Co && omap) ? omap[co] : co;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const long m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          if (m < M && co < Co) {
            float v = accf[i][j][r] + bsv;
            if (relu) v = cdn::relu_keep_nan(v);
            if (R) R[m * ldo + oc] = v;
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
            has_nan |= (v != v);
          }
        }
    }
  }
  if (qu.tracks())
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), pidx, npart, qu, red);
}

// (round 6: the kernel body as a device function of (m0, n0, partial index, partial count), so that the detection heads'
// launch -- three 64-column problems on one A operand, pwi8h_kernel below -- maps its workgroups itself)
template <int BM, int BN, int WGM, bool FAST, int WB = 4>
__device__ __forceinline__ void
pwi8_body(const float *__restrict__ A, const unsigned *__restrict__ aq,
          const signed char *__restrict__ Wq, const float *__restrict__ wscale,
          const int *__restrict__ wsum, const float *__restrict__ Wp,
          const float *__restrict__ bias, float *__restrict__ R,
          const cdn::QUpdate &qu, long M, int C, int Cpad, int Co, int relu, int lda,
          int ldo, const int *__restrict__ omap, int Cw, const long m0, const int n0, const int pidx, const int npart) {
  // C: the K extent of the int8 path (the channels of A, or its padded row length when the pad repeats a real channel
  // against zero weight codes); Cw: the logical channel count = row length of the f32 weights Wp (wide-code branch)
  constexpr int WGN = 4 / WGM;
  constexpr int TM = BM / (WGM * 32), TN = BN / (WGN * 32);
  constexpr int AI = BM * 8 / 256;        // float4 loads of A per thread per k-tile
  constexpr int BI = (BN * 2 + 255) / 256;  // 16-byte loads of W per thread per k-tile
  __shared__ __attribute__((aligned(16))) unsigned char A0[2][BM * kI8LD];
  __shared__ __attribute__((aligned(16))) unsigned char A1[2][BM * kI8LD];
  __shared__ __attribute__((aligned(16))) unsigned char B0[2][BN * kI8LD];
  static_assert(WB == 4 || WB == 8, "weight code width: 4 (16*qw plane) or 8 (second accumulator)");
  __shared__ __attribute__((aligned(16))) unsigned char B1[WB == 4 ? 2 : 1][WB == 4 ? BN * kI8LD : 16];
  CDN_STAMPR(2, 0);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave / WGN) * TM * 32, wn = (wave % WGN) * TN * 32;
  // Round 6: the first k tile and the epilogue constants go out BEFORE the input quantiser's state is read -- the branch
  // on its wide-code flag below needs the state, and with the loads behind that branch every workgroup began with one
  // memory round trip for three words and only then asked for its data (a second trip; the workgroups of these launches
  // live for two to eight k tiles).  The wide path ignores what was loaded.
  const int lr = tid >> 3, lk = (tid & 7) * 4;      // A staging: row lr + 32*i, k quad lk
  const bool vec4 = !FAST && (C & 3) == 0 && (lda & 3) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
  const int br = tid >> 1, bh = (tid & 1) * 16;     // B staging: row br + 128*i, 16-byte half bh
  float4 a[AI];
  i32x4 b[BI];
  const float *arow[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    long m = m0 + lr + 32 * i;
    if (m > M - 1) m = M - 1;
    arow[i] = A + m * lda + lk;
  }
  auto load_tile = [&](int k0) {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      if (FAST) {
        a[i] = *reinterpret_cast<const float4 *>(arow[i] + k0);
      } else if (vec4) {
        a[i] = (k0 + lk < C) ? *reinterpret_cast<const float4 *>(arow[i] + k0)
                             : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        const int k = k0 + lk;
        a[i].x = (k + 0 < C) ? arow[i][k0 + 0] : 0.0f;
        a[i].y = (k + 1 < C) ? arow[i][k0 + 1] : 0.0f;
        a[i].z = (k + 2 < C) ? arow[i][k0 + 2] : 0.0f;
        a[i].w = (k + 3 < C) ? arow[i][k0 + 3] : 0.0f;
      }
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      int co = n0 + br + 128 * i;
      if (co > Co - 1) co = Co - 1;
      b[i] = *reinterpret_cast<const i32x4 *>(Wq + (long)co * Cpad + k0 + bh);
    }
  };
  // (128-row tiles keep the old order: their 16 + 8 registers of tile and row pointers live across the branch took the
  // kernel from 108 to 140 VGPRs = from four to three workgroups per CU; they serve the small-M launches only)
  constexpr bool kEarly = BM <= 64;
  if (kEarly) load_tile(0);
  // Epilogue constants of this lane's TN output columns, requested NOW (branch-free, clamped column): read after
  // the k loop they were 2 dependent round trips per column with the workgroup idle (the ISA waited for bias /
  // scale / colsum, then for the channel map), ~3 us at the end of every launch.
  float e_bias[TN], e_ws[TN];
  int e_sum[TN], e_oc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int co = n0 + wn + j * 32 + (lane & 31);
    const int cc = min(co, Co - 1);
    e_ws[j] = wscale[cc];
    e_sum[j] = wsum[cc];
    e_bias[j] = 0.f;
    e_oc[j] = co;
  }
  if (bias) {
#pragma unroll
    for (int j = 0; j < TN; ++j) e_bias[j] = bias[min(n0 + wn + j * 32 + (lane & 31), Co - 1)];
  }
  if (omap) {
#pragma unroll
    for (int j = 0; j < TN; ++j) e_oc[j] = omap[min(n0 + wn + j * 32 + (lane & 31), Co - 1)];
  }
  const float qs = reinterpret_cast<const float *>(aq)[2];
  const float qz = reinterpret_cast<const float *>(aq)[3];
  if (__builtin_amdgcn_readfirstlane((int)aq[6])) {      // (workgroup-uniform; said so: the loads above stay live past this branch)
    // Codes too wide for the nibble split (the tracked range is far narrower than the batch: the first
    // ~100 calls of a fresh EMA): this batch runs on f32 MFMA with the fake-quantised weights, inside
    // the same launch (a separate fallback launch costs 4.3 us per stage even when it has nothing to
    // do).  Simple single-buffered 16-deep k-tiles in the int8 path's LDS arrays: the rare path.
    static_assert(BM * 17 * 4 <= 2 * BM * kI8LD && BN * 17 * 4 <= 2 * BN * kI8LD, "LDS reuse");
    pwi8_wide_path<BM, BN, WGM>(A, Wp, bias, R, qu, M, Cw, Co, relu, lda, ldo, omap, qs, qz,
                                reinterpret_cast<float *>(&A0[0][0]), reinterpret_cast<float *>(&B0[0][0]),
                                reinterpret_cast<float *>(&A1[0][0]), m0, n0, 1, pidx, npart);
    return;
  }
  // as_uint(t + 1.5*2^23) = 0x4B400000 + rint(t) for |t| < 2^22 (guaranteed when state[6] == 0)
  const int ioff = (int)qz + (2048 - 128) - 0x4B400000;
  i32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (i32x16){0};
  i32x16 acch[WB == 8 ? TM : 1][WB == 8 ? TN : 1];      // WB = 8: the sums of the a1 plane
  if constexpr (WB == 8) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acch[i][j] = (i32x16){0};
  }
  auto ucode = [&](float v, bool live) -> unsigned {
#pragma clang fp contract(off)
#if defined(CDN_DIAG) && CDN_DIAG == 7   // diagnostic build: no fp32 -> code arithmetic (wrong results)
    return (__float_as_uint(v) & 0xfffu) | 8u;
#endif
    // t = sc*d - zp (two roundings, as the reference); rint(t) by the 1.5*2^23 trick; then integer:
    // u = rint(t) + zp - 128 + 2048 in [8, 4087]
    const float y_p = qs * v;      // (plain operators under fp contract(off): two roundings, cdn_common.h)
  const float y = (y_p - qz) + 12582912.0f;
    int u = (int)__float_as_uint(y) + ioff;
    u = min(max(u, 8), 4087);       // |L - 128| <= 2040: never active unless state[6] lied
    return live ? (unsigned)u : 2048u;
  };
  auto store_tile = [&](int buf, int k0) {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      const int k = k0 + lk;
      const unsigned u0 = ucode(a[i].x, FAST || k + 0 < C), u1 = ucode(a[i].y, FAST || k + 1 < C);
      const unsigned u2 = ucode(a[i].z, FAST || k + 2 < C), u3 = ucode(a[i].w, FAST || k + 3 < C);
      const unsigned p01 = u0 | (u1 << 16), p23 = u2 | (u3 << 16);
      // a0 = u & 15 in [0,15];  a1 = (u >> 4) - 128 (byte ^ 0x80);  bytes {p01.b0, p01.b2, p23.b0, p23.b2}
      const unsigned lo = __builtin_amdgcn_perm(p23, p01, 0x06040200u) & 0x0F0F0F0Fu;
      const unsigned hi = __builtin_amdgcn_perm(p23 >> 4, p01 >> 4, 0x06040200u) ^ 0x80808080u;
      *reinterpret_cast<unsigned *>(&A0[buf][(lr + 32 * i) * kI8LD + lk]) = lo;
      *reinterpret_cast<unsigned *>(&A1[buf][(lr + 32 * i) * kI8LD + lk]) = hi;
    }
#pragma unroll
    for (int i = 0; i < BI; ++i)
      if (br + 128 * i < BN) {
        *reinterpret_cast<i32x4 *>(&B0[buf][(br + 128 * i) * kI8LD + bh]) = b[i];
        if constexpr (WB == 4) {
          i32x4 s16;   // 16*qw per byte: shift each byte left by 4 (qw in [-8,7] -> no carry loss)
#pragma unroll
          for (int e = 0; e < 4; ++e) s16[e] = (int)(((unsigned)b[i][e] << 4) & 0xF0F0F0F0u);
          *reinterpret_cast<i32x4 *>(&B1[buf][(br + 128 * i) * kI8LD + bh]) = s16;
        }
      }
  };

  if (!kEarly) load_tile(0);
  store_tile(0, 0);
  __syncthreads();
  CDN_STAMPR(2, 1);
  const int nk = (C + 31) / 32;   // (Cpad >= 32 * nk: the weight rows are zero padded to 64)
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    if (t + 1 < nk) load_tile((t + 1) * 32);
    i32x4 a0[TM], a1[TM], b0[TN], b1[TN];
    const int fo = (lane & 31) * kI8LD + (lane >> 5) * 16;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      a0[i] = *reinterpret_cast<const i32x4 *>(&A0[buf][(wm + i * 32) * kI8LD + fo]);
      a1[i] = *reinterpret_cast<const i32x4 *>(&A1[buf][(wm + i * 32) * kI8LD + fo]);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      b0[j] = *reinterpret_cast<const i32x4 *>(&B0[buf][(wn + j * 32) * kI8LD + fo]);
      if constexpr (WB == 4) b1[j] = *reinterpret_cast<const i32x4 *>(&B1[buf][(wn + j * 32) * kI8LD + fo]);
    }
    // (low nibbles for every accumulator, then the high parts: two MFMAs into the same accumulator back to back
    // wait for each other; the integer sum does not depend on the order)
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0[i], b0[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        if constexpr (WB == 4) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1[i], b1[j], acc[i][j], 0, 0, 0);
        else acch[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1[i], b0[j], acch[i][j], 0, 0, 0);
      }
    if (t + 1 < nk) store_tile(buf ^ 1, (t + 1) * 32);
    __syncthreads();
  }
  CDN_STAMPR(2, 2);
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int co = n0 + wn + j * 32 + (lane & 31);
    const float bsv = e_bias[j], rinv = __fdiv_rn(1.0f, __fmul_rn(qs, e_ws[j]));
    const int t128 = 128 * e_sum[j], oc = e_oc[j];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < M && co < Co) {
          int sum = acc[i][j][r];
          if constexpr (WB == 8) sum += 16 * acch[i][j][r];      // (exact: see the bound in the header)
          float v = fmaf((float)(sum + t128), rinv, bsv);
          if (relu) v = cdn::relu_keep_nan(v);
          if (R) R[m * ldo + oc] = v;                          // (R == NULL: range-only pass)
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          has_nan |= (v != v);
        }
      }
  }
  CDN_STAMPR(2, 3);
  if (qu.tracks())
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), pidx, npart, qu,
                             reinterpret_cast<float *>(&A0[0][0]));
  CDN_STAMPR(2, 4);
}

template <int BM, int BN, int WGM, bool FAST>
__global__ void __launch_bounds__(256)
pwi8_kernel(const float *__restrict__ A, const unsigned *__restrict__ aq,
            const signed char *__restrict__ Wq, const float *__restrict__ wscale,
            const int *__restrict__ wsum, const float *__restrict__ Wp,
            const float *__restrict__ bias, float *__restrict__ R,
            cdn::QUpdate qu, long M, int C, int Cpad, int Co, int relu, int lda,
            int ldo, const int *__restrict__ omap, int Cw) {
  pwi8_body<BM, BN, WGM, FAST>(A, aq, Wq, wscale, wsum, Wp, bias, R, qu, M, C, Cpad, Co, relu, lda, ldo, omap, Cw,
                               (long)blockIdx.x * BM, blockIdx.y * BN, blockIdx.y * gridDim.x + blockIdx.x,
                               gridDim.x * gridDim.y);
}

// the same body on 8-bit weight codes (CDN_W_CODES_8BIT).  A kernel of its own name: the 4-bit instantiations above keep
// their symbols, their registers and their LDS
template <int BM, int BN, int WGM, bool FAST>
__global__ void __launch_bounds__(256)
pwi8w_kernel(const float *__restrict__ A, const unsigned *__restrict__ aq,
             const signed char *__restrict__ Wq, const float *__restrict__ wscale,
             const int *__restrict__ wsum, const float *__restrict__ Wp,
             const float *__restrict__ bias, float *__restrict__ R,
             cdn::QUpdate qu, long M, int C, int Cpad, int Co, int relu, int lda,
             int ldo, const int *__restrict__ omap, int Cw) {
  pwi8_body<BM, BN, WGM, FAST, 8>(A, aq, Wq, wscale, wsum, Wp, bias, R, qu, M, C, Cpad, Co, relu, lda, ldo, omap, Cw,
                                  (long)blockIdx.x * BM, blockIdx.y * BN, blockIdx.y * gridDim.x + blockIdx.x,
                                  gridDim.x * gridDim.y);
}

// pwi8h_kernel (round 6; VERDICT r5 "next" #1a): the FIRST 1x1 convs of the detection heads -- NH problems of 64 output
// columns each on ONE A operand (the last stage's output r, 67 MB at batch 64, which three separate launches on three
// streams read three times) -- as one launch.  Weights / scales / column sums / biases are the heads' concatenated
// (row h * 64 + co); head h writes its own [M][64] buffer R + h * head_stride (omap: column -> column % 64) and updates
// its own QuantAct (qus.q[h], own arrival counters: the range epilogue per column group).  A 1-D grid: the NH workgroups
// of one 64-row block get ids 8 apart -- one XCD under round-robin dispatch, dispatched together -- so the second and
// third reading of the rows are L2 hits.  Same body, same sums: bit-identical to the per-head launches.
struct QUpdateN {
  cdn::QUpdate q[4];
};
template <int NH, int WB = 4>
__global__ void __launch_bounds__(256)
pwi8h_kernel(const float *__restrict__ A, const unsigned *__restrict__ aq, const signed char *__restrict__ Wq,
             const float *__restrict__ wscale, const int *__restrict__ wsum, const float *__restrict__ Wp,
             const float *__restrict__ bias, float *__restrict__ R, QUpdateN qus, long M, int C, int Cpad,
             int relu, int lda, const int *__restrict__ omap, long head_stride) {
  const int ntm = (int)((M + 63) / 64), grp = 8 * NH, b = blockIdx.x, full = (ntm / 8) * grp;
  int mt, head;
  if (b < full) {
    const int lid = b % grp;
    head = lid >> 3;
    mt = (b - lid) / NH + (lid & 7);
  } else {
    const int q = b - full, rem = ntm - (full / NH);
    head = q / rem;
    mt = full / NH + q % rem;
  }
  pwi8_body<64, 64, 2, true, WB>(A, aq, Wq, wscale, wsum, Wp, bias, R + (long)head * head_stride, qus.q[head],
                                 M, C, Cpad, 64 * NH, relu, lda, 64, omap, C, (long)mt * 64, head * 64, mt, ntm);
}


// ------------------------------------------------------------------------------------------
// pwi8s_kernel (round 5): pwi8_kernel's arithmetic as a STREAMING kernel for long-K launches (stage 0: K = 1024) --
// pws_kernel's structure.  tools/probes/probe_rowstream.hip: the stage-0 pointwise's 67-MB A operand can be read in
// 12-15 us (4.3-5.4 TB/s) whatever the ring depth; pwi8_kernel takes 36 us there because each of its 32 dependent k
// tiles is the serial sum of a global round trip, the fp32 -> code conversion, LDS writes, a barrier, LDS reads and the
// MFMAs, with two workgroups per CU to overlap (DESIGN_HISTORY section 4.1).  Here a workgroup owns a 32-row block x
// 32 TN columns, its four WAVES are the four quarters of K and each runs its own pipeline without workgroup barriers:
//   A   32 rows x 32 k of fp32 d per window by LDS-DMA into a wave-private ring of RR = 2 windows, one window ahead
//       (whole 128-byte lines, XOR-swizzled source chunks: pws_kernel); the fragment -- lane (i, h): k in
//       [16 h, 16 h + 16) of row i -- is read as four ds_read_b128 and converted IN REGISTERS to the two nibble operands
//       (pwi8_kernel's ucode / perm expressions: every element is converted once per workgroup);
//   B   the weight codes from a K-BLOCKED copy [window][column][32 B] (behind the row-major codes, made by the host:
//       CDN_X_WCODES_KB): the operand of a 32-column tile is one fully coalesced 1-KB load per window, straight into
//       registers, one window ahead; 16 * qw by a byte shift.
// The int32 partial sums of the four k quarters are added through LDS (exact: order-independent).  Same integer sums
// and the same epilogue expression as pwi8_kernel: bit-identical outputs and ranges (tests/test_gpu_parity.py).
// ncg = 2 (Co = 256): two workgroups per row block, 128 columns each, 8 ids apart -- the same XCD, dispatched
// together, so the second reading of the A rows is an L2 hit.
// Round 7: 36 KB of LDS (the epilogue's partial sums, which alias the four 8-KB rings) and 128 registers -- four
// workgroups per CU, so the 1024 workgroups of CoDeNet1x's stage 0 are all resident (cdn_codenet_pwi8s_resident_workgroups;
// before: rings of three windows, 48 KB, 160 registers, three per CU = 768 + a second round of 256).  Measured, three
// interleaved rounds on one box: the launch 31.5 -> 31.1 us, the step 0.2532 -> 0.2506 ms; a ring of five HALF windows
// (40 KB, three halves in flight) 31.5 us.  In-kernel stamps of that form: every workgroup starts within 0.6 us, but its
// k loop takes 21.2 us instead of 11.5 -- sixteen waves per CU stream the 67 MB hardly faster than twelve did, and in
// lockstep no epilogue overlaps a k loop (DESIGN.md sections 4.8 and 8).
// Wide codes (state[6]): pwi8_wide_path.
// vmcnt discipline: the weight loads are inline asm as well.  A compiler-visible load in this loop is waited for
// with a count the compiler derives WITHOUT the DMAs it cannot see, and in-order completion then makes every such
// wait a wait for the newest DMA (first version: 33 us).  Their destination registers are released by an empty asm
// that names them right behind the explicit s_waitcnt, and loaded UNCONDITIONALLY inside the loop (the last steps are
// peeled) -- a conditional load makes the register a phi, and the copy the compiler then inserts reads it before the
// wait (second version: wrong sums); tools/check_asm_loads.py scans the ISA for exactly that.
// ------------------------------------------------------------------------------------------
// dynamic LDS of a workgroup: the epilogue's partial sums [4 waves][64 columns][32 + 4 rows] of int32 (36 KB), which alias
// the four rings of two 4-KB windows (32 KB) and the wide path's tiles
constexpr int kPwi8sLds = 4 * 64 * 36 * 4;
// the int8 part of pwi8s_kernel (a function of its own so that the kernel is a plain if / else of the two paths: with
// the wide branch written as an early return in front of it the compiler saw that branch's pending stores on a path
// into the prologue below and put an s_waitcnt vmcnt(0) between the first weight loads -- i.e. behind the first DMAs)
template <int TN, int RR>
__device__ __forceinline__ void pwi8s_body(const float *__restrict__ A, const signed char *__restrict__ Wkb,
                                           const float *__restrict__ wscale, const int *__restrict__ wsum,
                                           const float *__restrict__ bias, float *__restrict__ R,
                                           const cdn::QUpdate &qu, long M, int K, int Co, int relu, int lda, int ldo,
                                           const int *__restrict__ omap, int ncg, long m0, int cb, float qs, float qz,
                                           char *lds) {
  constexpr int kRing = RR * 4096;                   // windows of 32 rows x 32 k of fp32
  // Nothing is in flight here, and the compiler is told so with a REAL s_waitcnt vmcnt(0) (the builtin, which its
  // wait-count bookkeeping sees): the structurised control flow has an edge from the end of the wide branch to this
  // block, and for the stores pending on that edge it otherwise puts its own vmcnt(0) in front of the first asm load
  // that overwrites one of their registers -- in the middle of the prologue, behind the first DMAs.
  __builtin_amdgcn_s_waitcnt(0x0F70);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 31, h = lane >> 5;
  const int Cot = 32 * TN * ncg;                     // columns per window of the k-blocked codes (zero rows behind Co)
  // (wave-uniform values of the conversion in scalar registers, said so: as vector registers they were two of the 128)
  const int ioff = __builtin_amdgcn_readfirstlane((int)qz + (2048 - 128) - 0x4B400000);
  const int umax = __builtin_amdgcn_readfirstlane(4087);
  // k windows (32 channels) of this wave: whole PAIRS of windows, the first (K / 64) % 4 waves one pair more -- every
  // wave runs an even number of steps (the two weight-register sets alternate without a copy)
  const int pairs = K >> 6;
  const int nit = 2 * ((pairs >> 2) + (w < (pairs & 3) ? 1 : 0));
  const int win0 = 2 * (w * (pairs >> 2) + min(w, pairs & 3)), kbase = 32 * win0;
  // ---- A: DMA side --------------------------------------------------------------------------------------------------
  const float *abase = A + m0 * lda + kbase;
  unsigned aoff[4];
  {
    const int dr = lane >> 3, dc = lane & 7;
    const long rmax = M - 1 - m0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = 8 * u + dr;
      const int rl = (int)(row < rmax ? row : rmax);
      aoff[u] = (unsigned)rl * (unsigned)lda * 4u + (unsigned)((dc ^ ((row >> 1) & 7)) * 16);
      // one register per offset for the whole kernel: left alone, the compiler keeps a second, differently derived copy
      // for the peeled steps (128 registers are four workgroups per CU, and that copy was the difference)
      asm volatile("" : "+v"(aoff[u]));
    }
  }
  const unsigned ring = cdn::lds_addr_uniform(lds) + (unsigned)w * kRing;
  auto issue = [&](int t) {
    const unsigned dst = ring + (unsigned)(t % RR) * 4096;
#pragma unroll
    // (the window's k offset goes into the wave-uniform base: added to the lanes' offsets it made the compiler keep a
    // second, advancing copy of them for the loop, and the originals were spilled across it)
    for (int u = 0; u < 4; ++u) cdn::glds16(abase + t * 32, aoff[u], dst + u * 1024);
  };
  // ---- B: one coalesced 16-byte load per lane, tile and window (inline asm: see the header) -----------------------------
  const unsigned long long wb = (unsigned long long)(Wkb + ((long)win0 * Cot + cb) * 32);
  const unsigned wlo = __builtin_amdgcn_readfirstlane((unsigned)wb), whi = __builtin_amdgcn_readfirstlane((unsigned)(wb >> 32));
  const unsigned long long wbu = ((unsigned long long)whi << 32) | wlo;
  const unsigned bo0 = (unsigned)(i * 32 + 16 * h), wstep = (unsigned)Cot * 32u;
  i32x4 bA[TN], bB[TN];
  auto loadB = [&](i32x4 (&b)[TN], int t) {
    static_assert(TN <= 4, "one offset register: the tiles of a window within the 13-bit immediate");
    const unsigned v0 = bo0 + (unsigned)t * wstep;
#pragma unroll
    for (int j = 0; j < TN; ++j)
      asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(b[j]) : "v"(v0), "s"(wbu), "n"(1024 * j) : "memory");
  };
  auto release = [&](i32x4 (&b)[TN]) {      // names the registers a wait has made valid: no use moves above this point
    if constexpr (TN == 4)
      asm volatile("" : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3 % TN]));
    else
      asm volatile("" : "+v"(b[0]), "+v"(b[1]));
  };
  auto ucode = [&](float v) -> unsigned {
#pragma clang fp contract(off)
    const float y_p = qs * v;      // (two roundings, as the reference: see pwi8_kernel)
    const float y = (y_p - qz) + 12582912.0f;
    int u = (int)__float_as_uint(y) + ioff;
    u = min(max(u, 8), umax);
    return (unsigned)u;
  };
  i32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) acc[j] = (i32x16){0};
  const char *wring = lds + w * kRing;
  // the fragment's four chunks within a window (as aoff: one register each for the loop and the peeled step alike)
  unsigned foff[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    foff[q] = (unsigned)(i * 128 + ((4 * h + q) ^ ((i >> 1) & 7)) * 16);
    asm volatile("" : "+v"(foff[q]));
  }
  // issue order (vmcnt counts DMAs and loads alike, completing in order):
  //   B(0), A(0) | step t: B(t+1), A(t+1), wait, compute(t)
  // Step t reads the slot of window t while window t + 1 lands in the other one, which step t - 1 read: behind A(t) --
  // and B(t), older still -- there are B(t+1) and A(t+1), TN + 4 in the loop.
  static_assert(RR == 2, "prologue, look-ahead and the peeled step are written for a ring of two windows");
  CDN_STAMPR(2, 1);      // (in front of the first DMA: a store here would be one more count behind every wait)
  loadB(bA, 0);
  issue(0);
  auto step = [&](int t, i32x4 (&bcur)[TN], i32x4 (&bnxt)[TN], auto more) {
    constexpr int MORE = decltype(more)::value;      // a window behind this one: its weights and its DMAs go out first
    if constexpr (MORE) {
      loadB(bnxt, t + 1);
      issue(t + 1);
    }
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((TN + 4) * MORE) : "memory");
    release(bcur);
    const char *slot = wring + (t % RR) * 4096;
    i32x4 a0, a1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = *reinterpret_cast<const float4 *>(slot + foff[q]);
      const unsigned u0 = ucode(v.x), u1 = ucode(v.y), u2 = ucode(v.z), u3 = ucode(v.w);
      const unsigned p01 = u0 | (u1 << 16), p23 = u2 | (u3 << 16);
      a0[q] = (int)(__builtin_amdgcn_perm(p23, p01, 0x06040200u) & 0x0F0F0F0Fu);
      a1[q] = (int)(__builtin_amdgcn_perm(p23 >> 4, p01 >> 4, 0x06040200u) ^ 0x80808080u);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bcur[j], acc[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      i32x4 s16;
#pragma unroll
      for (int e = 0; e < 4; ++e) s16[e] = (int)(((unsigned)bcur[j][e] << 4) & 0xF0F0F0F0u);
      acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, s16, acc[j], 0, 0, 0);
    }
  };
  // nit is even and >= 2: every step but the last fetches the window and the weights one ahead; the last step is peeled
  // with its own (static) count -- no branch and no register copy anywhere near a wait
  {
    const std::true_type y;
    const std::false_type n;
    int t = 0;
    for (; t + 2 < nit; t += 2) {
      step(t, bA, bB, y);
      step(t + 1, bB, bA, y);
    }
    step(t, bA, bB, y);
    step(t + 1, bB, bA, n);      // nothing behind
  }
  CDN_STAMPR(2, 2);
  // ---- epilogue: the four k quarters' int32 partial tiles through LDS (exact), two 32-column tiles per round ----------
  // P[wave][column][row], rows contiguous: a lane's four consecutive accumulator registers are four consecutive rows
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  {
    // the epilogue's indices from a thread id the compiler cannot look through: derived from the one above, their
    // addresses are computed in front of the k loop and held in registers across it
    int etid = tid;
    asm volatile("" : "+v"(etid));
    const int tid = etid, i = tid & 31, h = (tid >> 5) & 1, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int *P = reinterpret_cast<int *>(lds);
    constexpr int PLD = 36;                           // ints per column: 32 rows + 4 (16-byte aligned, bank-staggered)
    static_assert(4 * 64 * PLD * 4 == kPwi8sLds && 4 * kRing <= kPwi8sLds, "the partial sums alias the rings");
    const int col = tid & 63, r0 = (tid >> 6) * 8;
    for (int j0 = 0; j0 < TN; j0 += 2) {
      __syncthreads();                                // (rings drained / the previous round's sums read)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const i32x16 &c = acc[j0 + jj];
          *reinterpret_cast<i32x4 *>(&P[((w * 64) + jj * 32 + i) * PLD + 8 * g + 4 * h]) =
              (i32x4){c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]};
        }
      __syncthreads();
      const int co = cb + j0 * 32 + col;
      if (co < Co) {
        const float bsv = bias ? bias[co] : 0.0f;
        const float rinv = __fdiv_rn(1.0f, __fmul_rn(qs, wscale[co]));
        const int t128 = 128 * wsum[co], oc = omap ? omap[co] : co;
        i32x4 s[2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          const i32x4 p0 = *reinterpret_cast<const i32x4 *>(&P[(0 * 64 + col) * PLD + r0 + 4 * hh]);
          const i32x4 p1 = *reinterpret_cast<const i32x4 *>(&P[(1 * 64 + col) * PLD + r0 + 4 * hh]);
          const i32x4 p2 = *reinterpret_cast<const i32x4 *>(&P[(2 * 64 + col) * PLD + r0 + 4 * hh]);
          const i32x4 p3 = *reinterpret_cast<const i32x4 *>(&P[(3 * 64 + col) * PLD + r0 + 4 * hh]);
          s[hh] = (p0 + p1) + (p2 + p3);
        }
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
          const int row = r0 + rr;
          if (m0 + row < M) {
            float v = fmaf((float)(s[rr >> 2][rr & 3] + t128), rinv, bsv);
            if (relu) v = cdn::relu_keep_nan(v);
            if (R) R[(m0 + row) * ldo + oc] = v;
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
            has_nan |= (v != v);
          }
        }
      }
    }
  }
  CDN_STAMPR(2, 3);
  if (qu.tracks()) {
    __syncthreads();
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.x, gridDim.x, qu,
                             reinterpret_cast<float *>(lds));
  }
  CDN_STAMPR(2, 4);
}

template <int TN, int RR>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
pwi8s_kernel(const float *__restrict__ A, const unsigned *__restrict__ aq, const signed char *__restrict__ Wkb,
             const float *__restrict__ wscale, const int *__restrict__ wsum, const float *__restrict__ Wp,
             const float *__restrict__ bias, float *__restrict__ R, cdn::QUpdate qu, long M, int K,
             int Co, int relu, int lda, int ldo, const int *__restrict__ omap, int Cw, int ncg) {
  extern __shared__ float4 p8_lds[];
  char *lds = reinterpret_cast<char *>(p8_lds);
  CDN_STAMPR(2, 0);
  // workgroup -> (row block, column group): the ncg workgroups of a row block are 8 ids apart (one XCD)
  int rb = blockIdx.x, cg = 0;
  if (ncg == 2) {
    const int nrb8 = (int)((gridDim.x >> 1) & ~7u), b = blockIdx.x;
    if (b < 2 * nrb8) { rb = ((b >> 4) << 3) | (b & 7); cg = (b >> 3) & 1; }
    else { rb = nrb8 + ((b - 2 * nrb8) >> 1); cg = b & 1; }
  }
  const long m0 = (long)rb * 32;
  const int cb = cg * 32 * TN;                       // first column of this workgroup
  const float qs = reinterpret_cast<const float *>(aq)[2];
  const float qz = reinterpret_cast<const float *>(aq)[3];
  if (aq[6] == 0) {
    pwi8s_body<TN, RR>(A, Wkb, wscale, wsum, bias, R, qu, M, K, Co, relu, lda, ldo, omap, ncg, m0, cb, qs, qz, lds);
  } else {      // codes too wide for the nibble split: this batch on f32 MFMA (the rare path, as in pwi8_kernel)
    float *fl = reinterpret_cast<float *>(lds);
    const int cend = min(Co, cb + 32 * TN);
    pwi8_wide_path<32, 128, 1>(A, Wp, bias, R, qu, M, Cw, cend, relu, lda, ldo, omap, qs, qz, fl, fl + 32 * 17,
                               fl + (32 + 128) * 17, m0, cb, (32 * TN + 127) / 128, (int)blockIdx.x, (int)gridDim.x);
  }
}
// ------------------------------------------------------------------------------------------
// pwb3: the integer-weight (W4 / W8) pointwise conv on FINAL (already fake-quantised, or fp32) activations -- the first 1x1 of a
// ShuffleNetV2 unit, whose input channels carry different generations of the layer's running QuantAct and
// so have no common integer grid.  Exact products on the bf16 matrix cores:
//   x = hi + mid + lo   (three bf16 terms by truncation: 8 + 8 + 8 significant bits, the split is EXACT)
//   weights  qw (int8: [-8, 7] in the W4A8 network, [-128, 127] at W8A8) are exact in bf16,  W' = qw / sw[co]
//   y[m][co] = (sum_c hi*qw + sum_c mid*qw + sum_c lo*qw) / sw[co] + b
// every product is exact in fp32 and the accumulation is fp32, as in the f32 MFMA kernel, at 3 of the
// 16x faster v_mfma_f32_32x32x16_bf16 per 16 k instead of 8 v_mfma_f32_32x32x2f32 (measured: the f32 form
// was matrix-core bound at conv5, 191 us for 15.6 GFLOP).  Operand lane map: lane (r = l&31, h = l>>5)
// holds k = 8h..8h+7 of row r.  LDS rows: 32 k (64 B) + 16 B pad = 80 B, conflict-free ds_read_b128.
// One LDS buffer + register prefetch of the next k-tile (two barriers per tile; 35-40 KiB per workgroup).
// ------------------------------------------------------------------------------------------
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
constexpr int kB3LD = 80;

template <int BM, int BN, int WGM>
__global__ void __launch_bounds__(256)
pwb3_kernel(const float *__restrict__ A, const unsigned *__restrict__ aq,
            const signed char *__restrict__ Wq, const float *__restrict__ wscale,
            const float *__restrict__ bias, float *__restrict__ R, cdn::QUpdate qu,
            long M, int C, int Cpad, int Co, int relu, int lda, int ldo,
            const unsigned char *__restrict__ agen, const int *__restrict__ omap) {
  constexpr int WGN = 4 / WGM;
  constexpr int TM = BM / (WGM * 32), TN = BN / (WGN * 32);
  constexpr int AI = BM * 8 / 256;          // float4 loads of A per thread per k-tile
  constexpr int BI = (BN * 2 + 255) / 256;  // 16-byte loads of W per thread per k-tile
  // agen != NULL: channel c of A is fake-quantised with the QuantAct state aq + 8 * agen[c] (the
  // generations of a layer's running block-output QuantAct)
  __shared__ float2 qt[kMixedMaxC];
  __shared__ __attribute__((aligned(16))) unsigned char Ah[BM * kB3LD];
  __shared__ __attribute__((aligned(16))) unsigned char Am[BM * kB3LD];
  __shared__ __attribute__((aligned(16))) unsigned char Al[BM * kB3LD];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[BN * kB3LD];
  const long m0 = (long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave / WGN) * TM * 32, wn = (wave % WGN) * TN * 32;
  const bool has_q = aq != nullptr;
  const bool mixed = agen != nullptr;
  float qs = 1.f, qz = 0.f;
  if (has_q && !mixed) {
    qs = reinterpret_cast<const float *>(aq)[2];
    qz = reinterpret_cast<const float *>(aq)[3];
  }
  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x16){0};
  const int lr = tid >> 3, lk = (tid & 7) * 4;      // A staging: row lr + 32*i, k quad lk
  const bool vec4 = (C & 3) == 0 && (lda & 3) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
  const bool vec2 = !vec4 && (C & 1) == 0 && (lda & 1) == 0 && (reinterpret_cast<uintptr_t>(A) & 7) == 0;
  const int br = tid >> 1, bh = (tid & 1) * 16;     // B staging: row br + 128*i, 16 codes from bh
  float4 a[AI];
  i32x4 b[BI];
  const float *arow[AI];
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    long m = m0 + lr + 32 * i;
    if (m > M - 1) m = M - 1;
    arow[i] = A + m * lda + lk;
  }
  auto load_tile = [&](int k0) {
    const int k = k0 + lk;
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      if (vec4) {
        a[i] = (k < C) ? *reinterpret_cast<const float4 *>(arow[i] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
      } else if (vec2) {
        const float2 z = make_float2(0.f, 0.f);
        const float2 lo = (k < C) ? *reinterpret_cast<const float2 *>(arow[i] + k0) : z;
        const float2 hi = (k + 2 < C) ? *reinterpret_cast<const float2 *>(arow[i] + k0 + 2) : z;
        a[i] = make_float4(lo.x, lo.y, hi.x, hi.y);
      } else {
        a[i].x = (k + 0 < C) ? arow[i][k0 + 0] : 0.0f;
        a[i].y = (k + 1 < C) ? arow[i][k0 + 1] : 0.0f;
        a[i].z = (k + 2 < C) ? arow[i][k0 + 2] : 0.0f;
        a[i].w = (k + 3 < C) ? arow[i][k0 + 3] : 0.0f;
      }
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      int co = n0 + br + 128 * i;
      if (co > Co - 1) co = Co - 1;
      b[i] = *reinterpret_cast<const i32x4 *>(Wq + (long)co * Cpad + k0 + bh);
    }
  };
  // (a.hi16 << 16) | b.hi16
  auto pack_hi = [](unsigned a_, unsigned b_) -> unsigned { return __builtin_amdgcn_perm(a_, b_, 0x07060302u); };
  auto store_tile = [&](int k0) {
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      float v[4] = {a[i].x, a[i].y, a[i].z, a[i].w};
      unsigned hb[4], mb[4], lb[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (mixed) {
          const float2 q2 = qt[min(k0 + lk + e, C - 1)];
          v[e] = (k0 + lk + e < C) ? fake_quant(v[e], q2.x, q2.y) : 0.0f;
        } else if (has_q) {
          v[e] = (k0 + lk + e < C) ? fake_quant(v[e], qs, qz) : 0.0f;
        }
        hb[e] = __float_as_uint(v[e]);
        const float r1 = __fsub_rn(v[e], __uint_as_float(hb[e] & 0xFFFF0000u));   // exact
        mb[e] = __float_as_uint(r1);
        lb[e] = __float_as_uint(__fsub_rn(r1, __uint_as_float(mb[e] & 0xFFFF0000u)));   // exact, <= 8 bits
      }
      const int o = (lr + 32 * i) * kB3LD + lk * 2;
      *reinterpret_cast<uint2 *>(&Ah[o]) = make_uint2(pack_hi(hb[1], hb[0]), pack_hi(hb[3], hb[2]));
      *reinterpret_cast<uint2 *>(&Am[o]) = make_uint2(pack_hi(mb[1], mb[0]), pack_hi(mb[3], mb[2]));
      *reinterpret_cast<uint2 *>(&Al[o]) = make_uint2(pack_hi(lb[1], lb[0]), pack_hi(lb[3], lb[2]));
    }
#pragma unroll
    for (int i = 0; i < BI; ++i)
      if (br + 128 * i < BN) {
        unsigned w[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int word = b[i][e];
          const unsigned f0 = __float_as_uint((float)((word << 24) >> 24));
          const unsigned f1 = __float_as_uint((float)((word << 16) >> 24));
          const unsigned f2 = __float_as_uint((float)((word << 8) >> 24));
          const unsigned f3 = __float_as_uint((float)(word >> 24));
          w[2 * e] = pack_hi(f1, f0);
          w[2 * e + 1] = pack_hi(f3, f2);
        }
        unsigned char *dstp = &Bs[(br + 128 * i) * kB3LD + bh * 2];
        *reinterpret_cast<i32x4 *>(dstp) = (i32x4){(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
        *reinterpret_cast<i32x4 *>(dstp + 16) = (i32x4){(int)w[4], (int)w[5], (int)w[6], (int)w[7]};
      }
  };

  const int nk = (C + 31) / 32;   // (Cpad >= 32 * nk: the weight rows are zero padded to 64)
  load_tile(0);
  if (mixed) {
    for (int c = tid; c < C; c += 256) {
      const float *sp = reinterpret_cast<const float *>(aq) + cdn::kQStateWords * (agen[c] == 255 ? 0 : agen[c]);   // (255: unused channel)
      qt[c] = make_float2(sp[2], sp[3]);
    }
    __syncthreads();
  }
  for (int t = 0; t < nk; ++t) {
    if (t) __syncthreads();       // the previous tile's fragment reads are done
    store_tile(t * 32);
    __syncthreads();
    if (t + 1 < nk) load_tile((t + 1) * 32);
    const int fo = (lane & 31) * kB3LD + (lane >> 5) * 16;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fh[TM], fm[TM], fl[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int o = (wm + i * 32) * kB3LD + fo + ks * 32;
        fh[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const i32x4 *>(&Ah[o]));
        fm[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const i32x4 *>(&Am[o]));
        fl[i] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const i32x4 *>(&Al[o]));
      }
#pragma unroll
      for (int j = 0; j < TN; ++j)
        fb[j] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const i32x4 *>(&Bs[(wn + j * 32) * kB3LD + fo + ks * 32]));
      // smallest terms first
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl[i], fb[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fm[i], fb[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh[i], fb[j], acc[i][j], 0, 0, 0);
        }
    }
  }
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int co = n0 + wn + j * 32 + (lane & 31);
    float bsv = 0.f, rinv = 0.f;
    int oc = co;
    if (co < Co) {
      if (bias) bsv = bias[co];
      rinv = __fdiv_rn(1.0f, wscale[co]);
      if (omap) oc = omap[co];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long m = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < M && co < Co) {
          float v = fmaf(acc[i][j][r], rinv, bsv);
          if (relu) v = cdn::relu_keep_nan(v);
          R[m * ldo + oc] = v;
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          has_nan |= (v != v);
        }
      }
  }
  if (qu.tracks())
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x,
                             gridDim.x * gridDim.y, qu, reinterpret_cast<float *>(&Ah[0]));
}

// ------------------------------------------------------------------------------------------
// pwd3: the same arithmetic as pwb3 (exact bf16 x 3 split against int8 weight codes of any width) as a STREAMING
// kernel for the shapes of the ShuffleNetV2 units (Co <= a few hundred, C <= 512): in pwb3 no two waves
// share a row of A (each wave owns 32 rows x the whole N tile), so staging A through LDS only re-shapes it
// -- and costs two barriers per 32 k with the load latency exposed between them (measured 44 us for
// 91 MB at layer 2).  Here a lane loads its MFMA operand straight from global memory: lane (r = l&31,
// h = l>>5) owns k = 32w + 16h .. + 15 of row r in window w -- 64 contiguous bytes, four dwordx4 loads
// (the k order inside a window is free as long as B agrees) -- two windows ahead in registers, no LDS,
// no barrier in the k loop.  B (the N tile's codes as bf16, [n][k]) and the per-channel quantiser table
// are staged in LDS once per workgroup.  A workgroup = 4 waves = 4 x 32 rows, one N tile of 32*TN columns.
// Fake-quantisation while loading: n = rint(s*x - z) + z (integer valued), x' = n / s by Markstein's
// sequence q0 = n*r, q = fma(fma(-q0, s, n), r, q0) with r = RN(1/s): the correctly rounded quotient in
// 3 instructions instead of the ~10 of the IEEE expansion (this loop is VALU-bound next to the MFMAs).
// ------------------------------------------------------------------------------------------
// (blockDim.x = 256, or 512 where the B tile leaves room for only ONE workgroup per CU -- layer4: 125 KB -- so that the CU
// still runs two waves per SIMD behind one staged tile: round 4)
template <int TN>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(TN == 2 ? 3 : 2, TN == 2 ? 3 : 2)))
pwd3_kernel(const float *__restrict__ A, const unsigned *__restrict__ aq,
            const signed char *__restrict__ Wq, const float *__restrict__ wscale,
            const float *__restrict__ bias, float *__restrict__ R, cdn::QUpdate qu,
            long M, int C, int Cpad, int Co, int relu, int lda, int ldo,
            const unsigned char *__restrict__ agen, const int *__restrict__ omap, int ngen) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  CDN_STAMPR(2, 0);
  const int nwin = (C + 31) >> 5, Kp = nwin * 32;
  const int ldb = Kp * 2 + 16;                               // bytes per B row: conflict-free ds_read_b128
  // quantiser table: three float arrays [Kp] (s | z | 1/s): a lane reads its 16 channels of a window as 4 + 4 + 4
  // ds_read_b128 issued together (one {s, z, r} record per channel cost 16 reads, each waited for: 1600 cycles
  // per half window in the ISA)
  float *qtab = reinterpret_cast<float *>(smem + (size_t)32 * TN * ldb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nthr = (int)blockDim.x, nwv = nthr >> 6;
  const int n0 = blockIdx.y * 32 * TN;
  const bool has_q = aq != nullptr;
  auto pack_hi = [](unsigned a_, unsigned b_) -> unsigned { return __builtin_amdgcn_perm(a_, b_, 0x07060302u); };

  // ---- A stream: a wave walks the 32-row blocks rb = first, first + stride, ...; its windows (rb, w) form
  // one sequence that is prefetched PF windows ahead across block boundaries -------------------------
  const long nrb = (M + 31) >> 5;
  const long rb_first = (long)blockIdx.x * nwv + wave, rb_stride = (long)gridDim.x * nwv;
  constexpr int PF = 2;
  float4 buf[PF][4];
  long prb = rb_first;         // block and window of the NEXT prefetch
  // Round 4: only the 32-channel windows in which THIS column tile has a non-zero weight code are streamed.  In the
  // shuffle-free layout the pass-through half of a unit's input row meets zero weight columns (FusedBackbone.
  // _mixed_plan); its slots form a few runs, so 1-7 of the 4 / 8 / 15 windows of a layer-1 / 2 / 3 row hold nothing
  // but zeros: x * 0 adds an exact zero to every accumulator, skipping the window is bit-identical, and the A stream
  // (and the chain of dependent window loads) shrinks by that share.  The host marks such columns with generation 255 in
  // the per-unit a_gen array (FusedBackbone._mixed_plan); the mask is built from those bytes in the table staging.
  __shared__ unsigned s_wmask;
  if (tid == 0) s_wmask = 0u;
  // Round 6: everything of the prologue that depends on nothing is ISSUED here -- the first pass of the B tile's weight
  // codes and the epilogue's per-column constants -- so that their round trip runs under the generation bytes' and the
  // quantiser states' (two dependent trips) instead of after them: the prologue was three to four round trips of
  // ~2 us each with every workgroup of the launch (one resident set) waiting at the same time.
  const int chunks = Kp >> 4;                                // 16-code chunks per row
  const int nitems = 32 * TN * chunks;
  i32x4 cw0[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int q = tid + nthr * u;
    const int r_ = q / chunks, ch = q - r_ * chunks;
    cw0[u] = (i32x4){0, 0, 0, 0};
    if (q < nitems && n0 + r_ < Co) cw0[u] = *reinterpret_cast<const i32x4 *>(Wq + (long)(n0 + r_) * Cpad + ch * 16);
  }
  float bsv[TN], rinv[TN], ws_[TN];
  int oc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {                             // branch-free, clamped column
    const int cc = min(n0 + j * 32 + (lane & 31), Co - 1);
    ws_[j] = wscale[cc];
    bsv[j] = bias ? bias[cc] : 0.f;
    oc[j] = omap ? omap[cc] : cc;
  }
  // ngen in 1 .. 16 (the caller says how many generations a_qstate holds): ALL their states and the first pass of
  // generation bytes go out in the same round trip and the table is filled from LDS -- without it the states are loaded
  // at addresses the generation bytes give: a second, dependent trip
  __shared__ float2 s_states[16];
  const bool pre_states = has_q && agen != nullptr && ngen >= 1 && ngen <= 16;
  int gen0[2] = {0, 0};
  if (pre_states) {
#pragma unroll
    for (int u = 0; u < 2; ++u) gen0[u] = agen[min(tid + nthr * u, C - 1)];
    if (tid < 16)
      s_states[tid] = *reinterpret_cast<const float2 *>(reinterpret_cast<const float *>(aq) +
                                                        cdn::kQStateWords * min(tid, ngen - 1) + 2);
  }
  __syncthreads();                    // (before the other waves OR their bits in)
  unsigned wmask = 0u, prem = 0u;     // the tile's window set; windows of the current block not yet prefetched
  auto load_next = [&](float4 (&d)[4]) {
    const bool live = prb < nrb;
    const long row = min(prb * 32 + (lane & 31), M - 1);
    const int pw_ = __builtin_ctz(prem);
    const int k = 32 * pw_ + 16 * (lane >> 5);
    // unconditional loads from clamped addresses (C % 4 == 0, C >= 4), zeroed afterwards: a load under a
    // per-lane condition is a branch + a wait of its own in the ISA
    const float *rowp = A + row * lda;
    float4 t4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) t4[i] = *reinterpret_cast<const float4 *>(rowp + min(k + 4 * i, C - 4));
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = (live && k + 4 * i < C) ? t4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    prem &= prem - 1;
    if (prem == 0u) {
      prem = wmask;
      prb += rb_stride;
    }
  };

  // ---- quantiser table and B tile -> LDS (loads batched: the prologue is latency, not work) -----------
  if (has_q) {
    // (a table entry per channel; both generation bytes first, then both states: 2 round trips per pass)
    for (int c0_ = 0; c0_ < Kp; c0_ += 2 * nthr) {
      float4 te[2];
      int gen[2] = {0, 0};
      if (agen) {
#pragma unroll
        for (int u = 0; u < 2; ++u) gen[u] = (pre_states && c0_ == 0) ? gen0[u] : agen[min(c0_ + tid + nthr * u, C - 1)];
#pragma unroll
        for (int u = 0; u < 2; ++u) {         // generation 255 = "this column meets only zero weight codes" (host)
          const int c = c0_ + tid + nthr * u;
          // a wave's 64 channels are two windows: one LDS atomic per wave (one per channel was ~1000 atomics on one word)
          const bool live = c < C && gen[u] != 255;
          const unsigned long long lv = __ballot(live);
          const int w0 = (c0_ + (tid & ~63) + nthr * u) >> 5;
          const unsigned bits = ((lv & 0xffffffffull) ? 1u << w0 : 0u) | ((lv >> 32) ? 2u << w0 : 0u);
          if (lane == 0 && bits) atomicOr(&s_wmask, bits);
          if (gen[u] == 255) gen[u] = 0;
        }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const float2 sz2 = pre_states ? s_states[min(gen[u], 15)]
                                      : *reinterpret_cast<const float2 *>(reinterpret_cast<const float *>(aq) +
                                                                          cdn::kQStateWords * gen[u] + 2);
        te[u] = make_float4(sz2.x, sz2.y, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int c = c0_ + tid + nthr * u;
        if (c < Kp) {
          qtab[c] = te[u].x;
          qtab[Kp + c] = te[u].y;
          qtab[2 * Kp + c] = c < C ? __fdiv_rn(1.0f, te[u].x) : 0.0f;
        }
      }
    }
  }
  // the window set is known after ONE round trip (the generation bytes): the A stream starts here, beside the staging of
  // the B tile below
  __syncthreads();
  wmask = (has_q && agen) ? __builtin_amdgcn_readfirstlane(s_wmask) : 0u;
  if (wmask == 0u) wmask = nwin >= 32 ? 0xffffffffu : ((1u << nwin) - 1u);      // no mask given: every window
#if defined(CDN_NO_WSKIP)               // A/B build: every window, as in round 3
  wmask = nwin >= 32 ? 0xffffffffu : ((1u << nwin) - 1u);
#endif
  prem = wmask;
  const int nlist = __builtin_popcount(wmask);
#pragma unroll
  for (int p_ = 0; p_ < PF; ++p_) load_next(buf[p_]);
  for (int q0 = tid; q0 < nitems; q0 += nthr * 4) {
    i32x4 cw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + nthr * u;
      const int r_ = q / chunks, ch = q - r_ * chunks;
      cw[u] = cw0[u];                                          // (first pass: loaded at the top of the kernel)
      if (q0 != tid) {
        cw[u] = (i32x4){0, 0, 0, 0};
        if (q < nitems && n0 + r_ < Co)
          cw[u] = *reinterpret_cast<const i32x4 *>(Wq + (long)(n0 + r_) * Cpad + ch * 16);
      }
    }

#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + nthr * u;
      if (q < nitems) {
        const int r_ = q / chunks, ch = q - r_ * chunks;
        unsigned w8[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int word = cw[u][e];
          const unsigned f0 = __float_as_uint((float)((word << 24) >> 24));
          const unsigned f1 = __float_as_uint((float)((word << 16) >> 24));
          const unsigned f2 = __float_as_uint((float)((word << 8) >> 24));
          const unsigned f3 = __float_as_uint((float)(word >> 24));
          w8[2 * e] = pack_hi(f1, f0);
          w8[2 * e + 1] = pack_hi(f3, f2);
        }
        unsigned char *dp = smem + (size_t)r_ * ldb + ch * 32;
        *reinterpret_cast<i32x4 *>(dp) = (i32x4){(int)w8[0], (int)w8[1], (int)w8[2], (int)w8[3]};
        *reinterpret_cast<i32x4 *>(dp + 16) = (i32x4){(int)w8[4], (int)w8[5], (int)w8[6], (int)w8[7]};
      }
    }
  }
  // epilogue constants of this lane's TN output columns (loaded at the top of the kernel)
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const bool live = n0 + j * 32 + (lane & 31) < Co;
    rinv[j] = live ? __fdiv_rn(1.0f, ws_[j]) : 0.f;
    if (!live) {
      bsv[j] = 0.f;
      oc[j] = -1;                                             // dead column
    }
  }
  __syncthreads();
  CDN_STAMPR(2, 1);

  const unsigned char *bbase = smem + (size_t)(lane & 31) * ldb + 32 * (lane >> 5);
  const float *qrow = qtab + 16 * (lane >> 5);
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not

  for (long rb = rb_first; rb < nrb; rb += rb_stride) {
    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[j] = (f32x16){0};
    unsigned crem = wmask;                                      // windows of this block not yet computed
    for (int w0 = 0; w0 < nlist; w0 += PF) {
#pragma unroll
      for (int p_ = 0; p_ < PF; ++p_) {
        if (w0 + p_ < nlist) {                                  // wave-uniform
          const int w = __builtin_ctz(crem);
          crem &= crem - 1;
          float v[16];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            v[4 * i] = buf[p_][i].x; v[4 * i + 1] = buf[p_][i].y;
            v[4 * i + 2] = buf[p_][i].z; v[4 * i + 3] = buf[p_][i].w;
          }
          load_next(buf[p_]);
          unsigned hb[16], mb[16], lb[16];
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {                      // 8 channels at a time: 6 table reads in flight
            float ts[8], tz[8], tr[8];
            if (has_q) {
#pragma unroll
              for (int i = 0; i < 2; ++i) {
                const float4 s4 = *reinterpret_cast<const float4 *>(qrow + 32 * w + 8 * hh + 4 * i);
                const float4 z4 = *reinterpret_cast<const float4 *>(qrow + Kp + 32 * w + 8 * hh + 4 * i);
                const float4 r4 = *reinterpret_cast<const float4 *>(qrow + 2 * Kp + 32 * w + 8 * hh + 4 * i);
                ts[4 * i] = s4.x; ts[4 * i + 1] = s4.y; ts[4 * i + 2] = s4.z; ts[4 * i + 3] = s4.w;
                tz[4 * i] = z4.x; tz[4 * i + 1] = z4.y; tz[4 * i + 2] = z4.z; tz[4 * i + 3] = z4.w;
                tr[4 * i] = r4.x; tr[4 * i + 1] = r4.y; tr[4 * i + 2] = r4.z; tr[4 * i + 3] = r4.w;
              }
            }
#pragma unroll
            for (int e8 = 0; e8 < 8; ++e8) {
              const int e = 8 * hh + e8;
              float x = v[e];
              if (has_q) {
#pragma clang fp contract(off)
                const float sx = ts[e8] * x;
                const float n = rintf(sx - tz[e8]) + tz[e8];
                const float q0 = __fmul_rn(n, tr[e8]);
                x = fmaf(fmaf(-q0, ts[e8], n), tr[e8], q0);
              }
              hb[e] = __float_as_uint(x);
              const float r1 = __fsub_rn(x, __uint_as_float(hb[e] & 0xFFFF0000u));
              mb[e] = __float_as_uint(r1);
              lb[e] = __float_as_uint(__fsub_rn(r1, __uint_as_float(mb[e] & 0xFFFF0000u)));
            }
          }
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            i32x4 ph, pm, pl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              ph[e] = (int)pack_hi(hb[8 * ks + 2 * e + 1], hb[8 * ks + 2 * e]);
              pm[e] = (int)pack_hi(mb[8 * ks + 2 * e + 1], mb[8 * ks + 2 * e]);
              pl[e] = (int)pack_hi(lb[8 * ks + 2 * e + 1], lb[8 * ks + 2 * e]);
            }
            const bf16x8 fh = __builtin_bit_cast(bf16x8, ph), fm = __builtin_bit_cast(bf16x8, pm),
                         fl = __builtin_bit_cast(bf16x8, pl);
            // lo, mid, hi terms in this order into every accumulator (the fp32 sums are those of the j-major
            // form), but interleaved over the TN accumulators: three MFMAs into one accumulator back to back stall
            // (TN = 2 sits at its 168-VGPR cap for three waves per SIMD: one B fragment at a time there)
            if constexpr (TN >= 4) {
              bf16x8 fb[TN];
#pragma unroll
              for (int j = 0; j < TN; ++j)
                fb[j] = __builtin_bit_cast(
                    bf16x8, *reinterpret_cast<const i32x4 *>(bbase + (size_t)j * 32 * ldb + 64 * w + 16 * ks));
#pragma unroll
              for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, fb[j], acc[j], 0, 0, 0);
#pragma unroll
              for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fm, fb[j], acc[j], 0, 0, 0);
#pragma unroll
              for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, fb[j], acc[j], 0, 0, 0);
            } else {
#pragma unroll
              for (int j = 0; j < TN; ++j) {
                const bf16x8 fb = __builtin_bit_cast(
                    bf16x8, *reinterpret_cast<const i32x4 *>(bbase + (size_t)j * 32 * ldb + 64 * w + 16 * ks));
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, fb, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fm, fb, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, fb, acc[j], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    if (rb == rb_first) CDN_STAMPR(2, 2);
    // The prefetch stream alternates between the two buffers item by item, the loop above indexes them by the
    // window's position in its pair (static register indexing).  With an ODD number of windows per block the two
    // disagree from the second block of a wave on (window 0 of the next block sits in buf[1]): swap them.  Without
    // this, layer4 (K = 464: 15 windows) computed every second 32-row block of a wave from swapped k windows
    // whenever a wave walked more than one block (M > 8192 rows: batch 64 at 512 x 512 only; found by
    // tests/test_harness.py::test_whole_network_512_batch64_fused_vs_module_path in round 3).
    if (nlist & 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4 t = buf[0][i];
        buf[0][i] = buf[1][i];
        buf[1][i] = t;
      }
    }
    const long mb0 = rb * 32;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long m = mb0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < M && oc[j] >= 0) {
          float v = fmaf(acc[j][r], rinv[j], bsv[j]);
          if (relu) v = cdn::relu_keep_nan(v);
          R[m * ldo + oc[j]] = v;
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          has_nan |= (v != v);
        }
      }
  }
  CDN_STAMPR(2, 3);
  if (qu.tracks())
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x,
                             gridDim.x * gridDim.y, qu, reinterpret_cast<float *>(smem));
  CDN_STAMPR(2, 4);
}

}  // namespace

// Pointwise (1x1) convolution on a channels-last activation A [M][C] -> R [M][Co]: int8 MFMA on codes
// when the A quantiser state and the integer weights are given, f32 MFMA otherwise.  Shared by the
// stage schedule and the stand-alone entry point (detection heads).
// pws_kernel instead of pw3_kernel: plain f32 operands, K a multiple of 32 with 16-byte aligned rows, and a launch
// whose pw3 tiling (64- or 128-row tiles x 128 / 64 columns) would leave the chip with at most one workgroup per CU
// -- the latency-chain regime (cfg2: all three stages).  CDN_PWS_MAX_TILES: A/B switch.
#ifndef CDN_PWS_MAX_TILES
#define CDN_PWS_MAX_TILES (cdn::kCUs)
#endif
static bool pws_applies(long M, int64_t K, int64_t Co, int64_t lda, const float *a, const float *w) {
  if (K < 32 || (K & 31) || (lda & 3) || ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w)) & 15))
    return false;
  const long tiles = cdn::ceil_div(M, Co > 64 ? 64 : 128) * cdn::ceil_div(Co, Co > 64 ? 128 : 64);
  return tiles <= (long)CDN_PWS_MAX_TILES && cdn::ceil_div(M, 32) * cdn::ceil_div(Co, 32) <= (1L << 20);
}

// tile width (TN) and K split (KS) of pws_kernel as TN * 10 + KS: the widest tile and the least K splitting that give
// >= 4 waves per CU -- (64 columns, whole K), (32, whole K), (64, K / 4), (32, K / 4)
static int pws_choice(long M, int64_t C, int64_t Co) {
  const long want = 4L * cdn::kCUs, mt32 = cdn::ceil_div(M, 32);
  const long w21 = mt32 * cdn::ceil_div(Co, 64), w11 = mt32 * cdn::ceil_div(Co, 32);
  const bool can_split = (C & 127) == 0;
  if (w21 >= want || (!can_split && Co > 32)) return 21;
  if (w11 >= want || !can_split) return 11;
  if (4 * w21 >= want) return 24;
  return 14;
}

// pwi8s_kernel instead of pwi8_kernel: K >= 512 whole 64-channel blocks (every wave an even number of >= 2 windows),
// Co <= 256, the k-blocked copy of the codes given (CDN_X_WCODES_KB).  Measured (round 5, one box, interleaved):
// CoDeNet1x stage 0 (16384 x 1024 -> 256) 37.5 -> 31 us, CoDeNet2x stage 0 (8192 x 2176 -> 256) 47.6 -> 25.9 us.
// CDN_NO_PWI8S: A/B switch.
static int64_t wcodes_kb_columns(int64_t Kpad, int64_t Co) {
#if defined(CDN_NO_PWI8S)
  return 0;
#endif
  if (Kpad < 512 || (Kpad & 63) || Co > 256 || Co < 1) return 0;
  return Co <= 64 ? 64 : Co <= 128 ? 128 : 256;
}
static bool pwi8s_applies(long M, int64_t Kt, int Cpad, int64_t Co, bool pw_fast, const signed char *w_kb) {
  return w_kb != nullptr && pw_fast && Kt == Cpad && wcodes_kb_columns(Kt, Co) != 0 && M >= 1 &&
         2 * cdn::ceil_div(M, 32) <= (long)kMaxGrid;
}
// the streaming kernel's instantiation for Co columns (its dynamic LDS: kPwi8sLds)
using Pwi8sKernel = decltype(&pwi8s_kernel<4, 2>);
static Pwi8sKernel pwi8s_choice(int64_t Co) { return Co <= 64 ? pwi8s_kernel<2, 2> : pwi8s_kernel<4, 2>; }
// diagnostics: workgroups of that instantiation the runtime keeps resident per CU at the launch's LDS size (0: no
// streaming kernel for this Co, negative: the runtime's error)
extern "C" int cdn_codenet_pwi8s_resident_workgroups(int64_t Co) {
  if (Co < 1 || Co > 256) return 0;
  int n = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void *)pwi8s_choice(Co), 256, kPwi8sLds);
  return e == hipSuccess ? n : -(int)e;
}
extern "C" int64_t cdn_codenet_wcodes_kb_columns(int64_t C, int64_t Co) {
  return C > 0 ? wcodes_kb_columns((C + 63) / 64 * 64, Co) : 0;
}
extern "C" int64_t cdn_codenet_wcodes_kb_offset(int64_t C, int64_t Co) {
  return C > 0 && Co > 0 ? (Co * ((C + 63) / 64 * 64) + 255) / 256 * 256 : 0;
}

// The tile of the tiled int8 pointwise (pwi8_kernel / pwi8w_kernel) for M rows, K = Kt and Co columns, as
// rows * 1000 + columns: launch_pointwise switches on it and cdn_codenet_pointwise_i8_tile answers it to tests.
// Co > 64: 64-row tiles (36 KiB LDS, 112 VGPRs: four workgroups per CU; measured at stage 1
// 26.3 us vs 30.6 us with 128-row tiles; 32-row tiles change nothing at stage 0: 40.2 vs 40.7 us)
// round 4: when 64-row tiles leave the chip with at most ONE workgroup per CU (CoDeNet2x stage 0 at 32 images:
// M = 8192, K = 2176 -- a chain of 68 dependent k tiles per workgroup and nothing beside it), 32-row tiles give
// every CU two chains to interleave
// ... and 32-row tiles for the K < 256 launches of layers 2-3 (unit exits, the stride-2 units' branch convs; round 4):
// whole network 2.564 / 2.603 -> 2.544 / 2.533 ms on one box.  NOT for K = 256 (stage 1 of the deform path: 0.2442 ->
// 0.2500 ms per step with them) and not at K >= 512, where nothing moved.
// Co <= 64 (layer 1's units, the heads' first conv, stage 2): 64 x 64 tiles on the large-M launches (round 4).  Alone
// on the GPU the 128 x 64 tiles are as fast (33.1 vs 31.6 us at 262 144 x 58 -> 58, 38.4 vs 39.9 at K = 128), inside
// the network -- beside the other branch / the other heads -- the smaller tiles are worth 38 us per batch (whole
// network 2.594-2.599 -> 2.552-2.561 ms, three interleaved pairs on one box; the deform step itself: unchanged)
static int pwi8_tile(long M, int64_t Kt, int64_t Co) {
  if (Co > 64) {
#if !defined(CDN_NO_PWI32)
    if (cdn::ceil_div(M, 64) * cdn::ceil_div(Co, 128) <= cdn::kCUs && Kt >= 1024) return 32128;
#endif
#if !defined(CDN_PWI_NO_32ROWS)
    if (Kt < 256) return 32128;
#endif
    return 64128;
  }
#if !defined(CDN_PWI_NO_64X64)
  if (M >= 65536) return 64064;
#endif
  return 128064;
}
// diagnostics / tests: the tile (rows * 1000 + columns) the tiled int8 pointwise takes for a dense [M][C] input; the
// same for 4- and 8-bit codes (8-bit codes never take the streaming kernel, which this does not describe)
extern "C" int cdn_codenet_pointwise_i8_tile(int64_t M, int64_t C, int64_t Co) {
  return (M > 0 && C > 0 && Co > 0) ? pwi8_tile((long)M, C, Co) : 0;
}

// planes of partial sums a chained fp32 pointwise of this shape leaves (cdn_codenet_stage_chain_parts): the column tiles
// of pws_kernel, 0 when the launch would not take that kernel
int cdn::pointwise_chain_parts(long M, int64_t C, int64_t Co) {
  if (!pws_applies(M, C, Co, C, nullptr, nullptr)) return 0;
  return (int)cdn::ceil_div(Co, 32 * (pws_choice(M, C, Co) / 10));
}

int cdn::launch_pointwise(const cdn::PwCall &p) {
  const long M = p.M;
  const int64_t C = p.C, Co = p.Co, lda = p.lda ? p.lda : C, ldo = p.ldo ? p.ldo : Co;
  hipStream_t st = p.st;
  // tile choice: keep >= 2 workgroups per CU when M is small (stage 0), wide N tiles otherwise
  const int pw_bn = Co > 64 ? 128 : 64;
  const int pw_bm = (Co > 64 && cdn::ceil_div(M, 128) * cdn::ceil_div(Co, 128) <= cdn::kCUs) ? 64 : 128;
  const int n_wg_r = (int)(cdn::ceil_div(M, pw_bm) * cdn::ceil_div(Co, pw_bn));
  CDN_REQUIRE(n_wg_r <= kMaxGrid, CDN_ERR_UNSUPPORTED, "too many pointwise workgroups");
  const int64_t Kt = p.a_padded ? lda : C;
  const bool pw_fast = (Kt % 32) == 0 && (lda & 3) == 0 && (reinterpret_cast<uintptr_t>(p.a) & 15) == 0;
#define CDN_PW1(BM_, BN_, WGM_, AQ_, FAST_)                                                      \
  pw3_kernel<BM_, BN_, WGM_, AQ_, FAST_><<<(unsigned)std::min<long>(                             \
      cdn::ceil_div(M, BM_) * cdn::ceil_div(Co, BN_), only_if_wide ? 2L * cdn::kCUs : (1L << 30)), 256, 0, st>>>( \
      p.a, p.a_state, p.w, p.bias, p.ep_scale, p.ep_shift, p.out, p.qu, M, (int)C, (int)Co, p.relu, only_if_wide, \
      (int)lda, (int)ldo)
#define CDN_PW(BM_, BN_, WGM_, AQ_)                                       \
  do {                                                                    \
    if (pw_fast) CDN_PW1(BM_, BN_, WGM_, AQ_, true);                      \
    else CDN_PW1(BM_, BN_, WGM_, AQ_, false);                             \
  } while (0)
  CDN_REQUIRE(p.w_bits == 4 || p.w_bits == 8, CDN_ERR_ARG, "weight code width must be 4 or 8");
  const bool use_i8 = p.w_codes != nullptr && p.a_state != nullptr && p.ep_scale == nullptr && p.a_gen == nullptr;
  // final-valued input (no QuantAct state to derive integer codes from) with integer weight codes (any int8 value:
  // |q| <= 128 is exact in bf16): exact bf16 x 3 split instead of f32 MFMA
  const bool use_b3 = p.w_codes != nullptr && p.ep_scale == nullptr && p.w_scale != nullptr &&
                      (p.a_gen != nullptr || p.a_state == nullptr);
  CDN_REQUIRE(p.a_gen == nullptr || (use_b3 && p.a_state != nullptr && C <= kMixedMaxC), CDN_ERR_UNSUPPORTED,
              "a mixed-generation input needs the states, the integer weight codes and C <= %d", kMixedMaxC);
  CDN_REQUIRE(p.out_map == nullptr || use_i8 || use_b3, CDN_ERR_UNSUPPORTED,
              "an output channel map needs the integer weight codes");
  const int only_if_wide = 0;
  if (use_i8) {
    CDN_REQUIRE(p.w_scale && p.w_colsum, CDN_ERR_ARG, "int8 pointwise needs scale and colsum");
    CDN_REQUIRE((reinterpret_cast<uintptr_t>(p.w_codes) & 15) == 0, CDN_ERR_ARG,
                "w_pw_codes must be 16-byte aligned");
    const int Cpad = (int)((C + 63) / 64 * 64);
    CDN_REQUIRE(!p.a_padded || lda == Cpad, CDN_ERR_ARG, "a padded A has round_up(C, 64) floats per row");
    cdn::ProfScope ps(cdn::kProfPointwise, p.ptag, st);
#define CDN_PWI(BM_, BN_, WGM_)                                                                            \
  do {                                                                                                     \
    dim3 g((unsigned)cdn::ceil_div(M, BM_), (unsigned)cdn::ceil_div(Co, BN_));                             \
    auto kern = pw_fast ? pwi8_kernel<BM_, BN_, WGM_, true> : pwi8_kernel<BM_, BN_, WGM_, false>;          \
    if (p.w_bits == 8) kern = pw_fast ? pwi8w_kernel<BM_, BN_, WGM_, true> : pwi8w_kernel<BM_, BN_, WGM_, false>; \
    kern<<<g, 256, 0, st>>>(p.a, p.a_state, p.w_codes, p.w_scale, p.w_colsum, p.w, p.bias, p.out, p.qu, M, \
                            (int)Kt, Cpad, (int)Co, p.relu, (int)lda, (int)ldo, p.out_map, (int)C);        \
  } while (0)
    // 8-bit codes: the bound of the second accumulator (pwi8_body) is stated for K <= 4096
    CDN_REQUIRE(p.w_bits != 8 || Kt <= 4096, CDN_ERR_UNSUPPORTED, "8-bit weight codes need C <= 4096 (got %lld)",
                (long long)Kt);
    // long-K launches with the k-blocked copy of the codes at hand (the fused stage, stage 0): the streaming kernel.
    // 4-bit codes only: its two accumulator sets for 8-bit codes are 2 x 64 registers at TN = 4 -- all 128 a wave has
    // at the four workgroups per CU the kernel is built around -- so 8-bit long-K launches take the tiled kernel below
    // (the k-blocked copy, when given, is simply not read)
    if (p.w_bits != 8 && pwi8s_applies(M, Kt, Cpad, Co, pw_fast, p.w_kb)) {
      const long nrb = cdn::ceil_div(M, 32);
      const int ncg = Co > 128 ? 2 : 1;
      const unsigned grid = (unsigned)(nrb * ncg);
      auto kern = pwi8s_choice(Co);
      constexpr int kLds = kPwi8sLds;
      kern<<<grid, 256, kLds, st>>>(p.a, p.a_state, p.w_kb, p.w_scale, p.w_colsum, p.w, p.bias, p.out, p.qu, M, (int)Kt,
                                    (int)Co, p.relu, (int)lda, (int)ldo, p.out_map, (int)C, ncg);
      return cdn::check_launch("codenet int8 pointwise (streaming)");
    }
    switch (pwi8_tile(M, Kt, Co)) {      // (the reasons and the measurements: pwi8_tile)
      case 32128: CDN_PWI(32, 128, 1); break;
      case 64128: CDN_PWI(64, 128, 2); break;
      case 64064: CDN_PWI(64, 64, 2); break;
      default: CDN_PWI(128, 64, 4); break;
    }
#undef CDN_PWI
    // (wide codes, state[6] != 0, are handled by the f32 branch inside pwi8_kernel)
  } else if (use_b3) {
    CDN_REQUIRE((reinterpret_cast<uintptr_t>(p.w_codes) & 15) == 0, CDN_ERR_ARG,
                "w_pw_codes must be 16-byte aligned");
    const int Cpad = (int)((C + 63) / 64 * 64);
    cdn::ProfScope ps(cdn::kProfPointwise, p.ptag, st);
#define CDN_PWB(BM_, BN_, WGM_)                                                                           \
  do {                                                                                                    \
    dim3 g((unsigned)cdn::ceil_div(M, BM_), (unsigned)cdn::ceil_div(Co, BN_));                            \
    pwb3_kernel<BM_, BN_, WGM_><<<g, 256, 0, st>>>(p.a, p.a_state, p.w_codes, p.w_scale, p.bias, p.out, p.qu, M, \
                                                   (int)C, Cpad, (int)Co, p.relu, (int)lda, (int)ldo, p.a_gen,   \
                                                   p.out_map);                                            \
  } while (0)
    // streaming form when the rows are 16-byte aligned quads and the N tile's weights fit in LDS
    int tn = Co > 64 ? 4 : 2;
    const int Kp = (int)((C + 31) / 32 * 32);
#if !defined(CDN_PWD3_NO_TN2_SMALLM)
    // Round 6: 64-column tiles where the 128-column tile's B (> 80 KB: K = 464) leaves ONE workgroup per CU and M is too
    // small for its 512-thread form -- layer 4's units at batch 64 ran 256 four-wave workgroups, one wave per SIMD; with
    // 64 columns two workgroups share a CU and the grid doubles (the A rows are read four times instead of twice, from
    // L2): 16384 x 464 -> 232 38.0 -> 35.6 us, whole network 2.509 -> 2.495 ms (three interleaved pairs)
    if (tn == 4 && (size_t)32 * 4 * (Kp * 2 + 16) + (size_t)Kp * 16 > 80 * 1024 &&
        cdn::ceil_div(M, 256) * cdn::ceil_div(Co, 128) < cdn::kCUs)
      tn = 2;
#endif
    const size_t lds_d3 = (size_t)32 * tn * (Kp * 2 + 16) + (size_t)Kp * 16;
    const long nblk_d3 = cdn::ceil_div(M, 128) * cdn::ceil_div(Co, 32 * tn);
    if ((C & 3) == 0 && (lda & 3) == 0 && (reinterpret_cast<uintptr_t>(p.a) & 15) == 0 &&
        lds_d3 <= 150 * 1024 && nblk_d3 <= kMaxGrid) {
      // persistent: as many workgroups as stay resident (VGPRs, LDS), each walks row blocks
      const unsigned ny = (unsigned)cdn::ceil_div(Co, 32 * tn);
      const long per_cu = std::min<long>(tn == 2 ? 3 : 2, (long)(160 * 1024 / (lds_d3 + 512)));   // 168 / 256 VGPRs
      const long gx = std::max<long>(1, std::min<long>(cdn::ceil_div(M, 128), per_cu * cdn::kCUs / ny));
      dim3 g((unsigned)gx, ny);
      auto kern = tn == 4 ? pwd3_kernel<4> : pwd3_kernel<2>;
      (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_d3);
      // one workgroup per CU (a B tile above 80 KB: layer4): 8 waves behind the one staged tile instead of 4
#if defined(CDN_PWD3_256)
      const int d3_threads = 256;
#else
      // (only where 256-row workgroups still fill the chip: layer 3's units have 64 x 2 of them and keep 256 threads)
      const int d3_threads = (per_cu == 1 && cdn::ceil_div(M, 256) * ny >= cdn::kCUs) ? 512 : 256;
#endif
      const long gx2 = std::max<long>(1, std::min<long>(cdn::ceil_div(M, d3_threads / 2), per_cu * cdn::kCUs / ny));
      g = dim3((unsigned)gx2, ny);
      kern<<<g, d3_threads, lds_d3, st>>>(p.a, p.a_state, p.w_codes, p.w_scale, p.bias, p.out, p.qu, M, (int)C, Cpad,
                                          (int)Co, p.relu, (int)lda, (int)ldo, p.a_gen, p.out_map, p.n_gens);
    } else if (pw_bn == 128 && pw_bm == 64) CDN_PWB(64, 128, 2);
    else if (pw_bn == 128) CDN_PWB(128, 128, 4);
    else CDN_PWB(128, 64, 4);
#undef CDN_PWB
  } else if (!p.a_state && p.a_gen == nullptr && p.out_map == nullptr && !p.a_padded &&
             pws_applies(M, C, Co, lda, p.a, p.w)) {
    // few output tiles: streaming waves (pws_kernel) -- the widest tile and the least K splitting that give >= 4 waves
    // per CU: (64 columns, whole K), (32, whole K), (64, K / 4), (32, K / 4)
    cdn::ProfScope ps(cdn::kProfPointwise, p.ptag, st);
#define CDN_PWS(TN_, KS_)                                                                                         \
  do {                                                                                                            \
    auto kern = pws_kernel<TN_, KS_>;                                                                             \
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, PwsGeom<TN_>::kLds); \
    kern<<<(unsigned)(cdn::ceil_div(M, KS_ == 4 ? 32 : 128) * cdn::ceil_div(Co, 32 * TN_)), 256, PwsGeom<TN_>::kLds, st>>>( \
        p.a, p.w, p.bias, p.ep_scale, p.ep_shift, p.out, p.qu, M, (int)C, (int)Co, p.relu, (int)lda, (int)ldo,    \
        p.next_ws, p.sparts);                                                                                     \
  } while (0)
    const int choice = pws_choice(M, C, Co);
    if (choice == 21) CDN_PWS(2, 1);
    else if (choice == 11) CDN_PWS(1, 1);
    else if (choice == 24) CDN_PWS(2, 4);
    else CDN_PWS(1, 4);
#undef CDN_PWS
  } else if (p.sparts) {
    return cdn::fail(CDN_ERR_UNSUPPORTED, "chained scale sums need the streaming f32 pointwise (cdn_codenet_stage_chain_parts)");
  } else {
    cdn::ProfScope ps(cdn::kProfPointwise, p.ptag, st);
    if (pw_bn == 128 && pw_bm == 64) {
      if (p.a_state) CDN_PW(64, 128, 2, true); else CDN_PW(64, 128, 2, false);
    } else if (pw_bn == 128) {
      if (p.a_state) CDN_PW(128, 128, 4, true); else CDN_PW(128, 128, 4, false);
    } else {
      if (p.a_state) CDN_PW(128, 64, 4, true); else CDN_PW(128, 64, 4, false);
    }
  }
#undef CDN_PW
#undef CDN_PW1
  return cdn::check_launch("codenet fused pointwise");
}

extern "C" int cdn_codenet_pointwise_nhwc_forward(
    const float *a, const void *a_qstate, int64_t M, int64_t C, int64_t Co, int64_t lda, int64_t ldo,
    const float *w,
    const signed char *w_codes, const float *w_scale, const int *w_colsum, const float *bias,
    const float *ep_scale, const float *ep_shift, int relu, float *r_min, float *r_max, void *r_state,
    int bits, double momentum, int running, void *workspace, size_t workspace_bytes, float *out,
    void *stream) {
  return cdn_codenet_pointwise_mixed_forward(a, a_qstate, nullptr, M, C, Co, lda, ldo, w, w_codes, w_scale,
                                             w_colsum, bias, ep_scale, ep_shift, relu, nullptr, r_min, r_max,
                                             r_state, bits, momentum, running, workspace, workspace_bytes,
                                             out, stream);
}

extern "C" int cdn_codenet_pointwise_mixed_forward(
    const float *a, const void *a_qstate, const unsigned char *a_gen, int64_t M, int64_t C, int64_t Co,
    int64_t lda, int64_t ldo, const float *w, const signed char *w_codes, const float *w_scale,
    const int *w_colsum, const float *bias, const float *ep_scale, const float *ep_shift, int relu,
    const int *out_map, float *r_min, float *r_max, void *r_state, int bits, double momentum, int running,
    void *workspace, size_t workspace_bytes, float *out, void *stream) {
  return cdn_codenet_pointwise_mixed_forward_n(a, a_qstate, a_gen, 0, M, C, Co, lda, ldo, w, w_codes, w_scale, w_colsum,
                                               bias, ep_scale, ep_shift, relu, out_map, r_min, r_max, r_state, bits,
                                               momentum, running, workspace, workspace_bytes, out, stream);
}

extern "C" int cdn_codenet_pointwise_mixed_forward_n(
    const float *a, const void *a_qstate, const unsigned char *a_gen, int n_gens, int64_t M, int64_t C, int64_t Co,
    int64_t lda, int64_t ldo, const float *w, const signed char *w_codes, const float *w_scale,
    const int *w_colsum, const float *bias, const float *ep_scale, const float *ep_shift, int relu,
    const int *out_map, float *r_min, float *r_max, void *r_state, int bits, double momentum, int running,
    void *workspace, size_t workspace_bytes, float *out, void *stream) {
  CDN_REQUIRE(a && w, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(n_gens >= 0, CDN_ERR_ARG, "n_gens must be >= 0 (0: unknown)");
  // relu | CDN_W_CODES_8BIT: w_codes may hold any int8 value (W8A8); without it the int8 kernels assume |q| <= 8
  const int w_bits = (relu & CDN_W_CODES_8BIT) ? 8 : 4;
  relu &= ~CDN_W_CODES_8BIT;
  CDN_REQUIRE(w_bits == 4 || w_codes, CDN_ERR_ARG, "CDN_W_CODES_8BIT without w_codes");
  // out == NULL: RANGE-ONLY pass (round 4) -- the kernel computes everything and stores nothing; only the int8 kernel
  // on one input state implements it
  CDN_REQUIRE(out || (r_state && a_qstate && !a_gen && w_codes && !ep_scale), CDN_ERR_ARG,
              "a range-only pass (out == NULL) needs the output QuantAct and the int8 form");
  CDN_REQUIRE(a_gen == nullptr || a_qstate != nullptr, CDN_ERR_ARG, "a_gen needs the states in a_qstate");
  CDN_REQUIRE(M > 0 && C > 0 && Co > 0 && M * std::max(C, Co) < (1ll << 31), CDN_ERR_ARG, "bad size");
  CDN_REQUIRE((ep_scale == nullptr) == (ep_shift == nullptr), CDN_ERR_ARG,
              "ep_scale / ep_shift must both be set or both be NULL");
  CDN_REQUIRE((r_state == nullptr) == (r_min == nullptr) && (r_state == nullptr) == (r_max == nullptr),
              CDN_ERR_ARG, "the output QuantAct needs x_min, x_max and state together");
  CDN_REQUIRE((reinterpret_cast<uintptr_t>(a) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
              CDN_ERR_ARG, "a / out must be 4-byte aligned");
  CDN_REQUIRE((lda == 0 || lda >= C) && (ldo == 0 || ldo >= Co), CDN_ERR_ARG,
              "row strides must be 0 (dense) or >= the channel counts");
  CDN_REQUIRE(M * std::max(lda, ldo) < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  unsigned *arrive = r_state ? cdn::aux_workspace(workspace, workspace_bytes) : nullptr;
  CDN_REQUIRE(!r_state || arrive, CDN_ERR_WORKSPACE, "workspace missing, too small or not 256-byte aligned");
  cdn::PwCall pw{};
  pw.a = a;
  pw.a_state = static_cast<unsigned *>(const_cast<void *>(a_qstate));
  pw.M = (long)M;
  pw.C = C;
  pw.Co = Co;
  pw.w = w;
  pw.w_codes = w_codes;
  pw.w_scale = w_scale;
  pw.w_colsum = w_colsum;
  pw.bias = bias;
  pw.ep_scale = ep_scale;
  pw.ep_shift = ep_shift;
  pw.relu = relu;
  pw.out = out;
  pw.qu = cdn::make_qupdate(r_min, r_max, r_state, arrive, bits, momentum, running);
  pw.st = cdn::as_stream(stream);
  pw.lda = lda;
  pw.ldo = ldo;
  pw.a_gen = a_gen;
  pw.out_map = out_map;
  pw.n_gens = n_gens;
  pw.w_bits = w_bits;
  return cdn::launch_pointwise(pw);
}

// The first 1x1 convs of NH detection heads (64 -> 64 each, one shared input) as ONE launch: pwi8h_kernel.
extern "C" int cdn_codenet_heads_pointwise_supported(int64_t M, int64_t C, int n_heads) {
  return (M > 0 && C >= 32 && (C & 31) == 0 && n_heads >= 2 && n_heads <= 4 && M * 64 * n_heads < (1ll << 31) &&
          cdn::ceil_div(M, 64) <= kMaxGrid) ? 1 : 0;
}

extern "C" int cdn_codenet_heads_pointwise_forward(
    const float *a, const void *a_qstate, int64_t M, int64_t C, int n_heads, const float *w,
    const signed char *w_codes, const float *w_scale, const int *w_colsum, const float *bias, int relu,
    float *const *r_min, float *const *r_max, void *const *r_state, int bits, double momentum, int running,
    void *const *workspaces, size_t workspace_bytes, const int *out_map, float *out, int64_t head_stride, void *stream) {
  CDN_REQUIRE(a && a_qstate && w && w_codes && w_scale && w_colsum && r_min && r_max && r_state && workspaces && out_map &&
                  out,
              CDN_ERR_ARG, "null pointer");
  const int w_bits = (relu & CDN_W_CODES_8BIT) ? 8 : 4;      // (as in cdn_codenet_pointwise_nhwc_forward)
  relu &= ~CDN_W_CODES_8BIT;
  CDN_REQUIRE(w_bits == 4 || C <= 4096, CDN_ERR_UNSUPPORTED, "8-bit weight codes need C <= 4096 (got %lld)", (long long)C);
  CDN_REQUIRE(cdn_codenet_heads_pointwise_supported(M, C, n_heads), CDN_ERR_UNSUPPORTED,
              "heads launch: 2-4 heads of 64 columns, C %% 32 == 0 (cdn_codenet_heads_pointwise_supported)");
  CDN_REQUIRE(bits >= 2 && bits <= 16, CDN_ERR_ARG, "bits must be in [2,16], got %d", bits);
  CDN_REQUIRE(head_stride >= M * 64 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w_codes)) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(out) & 3) == 0,
              CDN_ERR_ARG, "head_stride >= M * 64; a / w_codes 16-byte aligned");
  QUpdateN qus;
  for (int h = 0; h < 4; ++h) {
    const int j = h < n_heads ? h : 0;
    CDN_REQUIRE(r_min[j] && r_max[j] && r_state[j] && workspaces[j], CDN_ERR_ARG, "null pointer in head %d", j);
    unsigned *arrive = cdn::aux_workspace(workspaces[j], workspace_bytes);
    CDN_REQUIRE(arrive, CDN_ERR_WORKSPACE, "workspace of head %d missing, too small or not 256-byte aligned", j);
    qus.q[h] = cdn::make_qupdate(r_min[j], r_max[j], r_state[j], arrive, bits, momentum, running);
  }
  const int Cpad = (int)((C + 63) / 64 * 64);
  const unsigned grid = (unsigned)(cdn::ceil_div(M, 64) * n_heads);
  hipStream_t st = cdn::as_stream(stream);
  const unsigned *aq = static_cast<const unsigned *>(a_qstate);
#define CDN_PWH(NH_)                                                                                                \
  do {                                                                                                              \
    auto kern = w_bits == 8 ? pwi8h_kernel<NH_, 8> : pwi8h_kernel<NH_, 4>;                                          \
    kern<<<grid, 256, 0, st>>>(a, aq, w_codes, w_scale, w_colsum, w, bias, out, qus, (long)M, (int)C, Cpad, relu,   \
                               (int)C, out_map, (long)head_stride);                                                 \
  } while (0)
  if (n_heads == 2) CDN_PWH(2);
  else if (n_heads == 3) CDN_PWH(3);
  else CDN_PWH(4);
#undef CDN_PWH
  return cdn::check_launch("codenet heads pointwise");
}
