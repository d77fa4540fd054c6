// codenet_fused.hip -- one CoDeNet up-sampling stage as a fused kernel schedule (gfx950).
//
// What the reference runs per stage (W4A8: quant_modules.py:668-671 + quantize_model.py:79-81;
// fp32: modules/dcn_deform_conv.py:323-330 + shufflenetv2_dcn.py:303-308):
//     conv_scale -> Hardtanh -> [QuantAct] -> deform depthwise 3x3 -> [QuantAct] ->
//     conv_channel (+BN) -> ReLU -> [QuantAct] -> Upsample x2
// as ~12 framework ops with every tensor round-tripping through memory.  Here a stage is
//     scale (+min/max)  ->  [range update]  ->  gather/depthwise (+min/max)  ->  [range update]
//     ->  pointwise MFMA (+bias/BN, ReLU, min/max)  ->  [range update]
// with * QuantAct min/max reductions folded into the producing kernel's epilogue,
//      * fake-quantisation applied by the CONSUMER while it loads (same fp32 expression, so the
//        values are bit-identical to materialising them),
//      * the nearest x2 up-sampling folded into the consumer's addressing (the stage input is
//        kept at half resolution; scale prediction runs at half resolution: 4x less work),
//      * channels-last intermediates so every wave access is a contiguous row.
//
// gather/depthwise kernel (dw2): lane <-> 4 channels, 16 (or 8) lanes <-> one output pixel.
// The low-resolution input plane of CCH channels lives in LDS as [cell][CCH] rows with a zero
// border; a tap corner is ONE ds_read_b128 per lane.  With CCH = 64 a row is exactly the 64 LDS
// banks, so bank == channel and the read is conflict-free for ANY data-dependent cell -- the
// per-lane-column conflicts of the NCHW kernel (codenet_stage.hip) cannot occur.
//
// This file: scale, gather, unpack, the stage entry points and the launchers the frozen-range schedule shares.  The
// pointwise kernels and their launcher (cdn::launch_pointwise) live in codenet_pointwise.hip.
#include "cdn_common.h"

#include <algorithm>
#include <type_traits>
#include <cstdlib>

// In-kernel phase stamps for tools/probes/probe_dw.hip (which includes this file with
// -DCDN_STAMPS): thread 0 of every workgroup records s_memrealtime (100 MHz) at phase boundaries.
#ifdef CDN_STAMPS
// regions: 0 scale, 1 gather, 2 pointwise; 2048 workgroups x 8 stamps each.  A __device__ array cannot be shared between
// translation units without -fgpu-rdc: this file owns regions 0 and 1 and the per-wave gather end times of workgroup 0,
// codenet_pointwise.hip region 2; the host buffer keeps the layout [3 regions][64 wave slots].
__device__ unsigned long long cdn_stamps[2 * 2048 * 8 + 64];
#define CDN_STAMPR(R, I)                                                                 \
  do {                                                                                   \
    static_assert((R) < 2, "region 2 belongs to codenet_pointwise.hip");                 \
    if (threadIdx.x == 0)                                                                \
      cdn_stamps[(R) * 16384 + (((blockIdx.y * gridDim.x + blockIdx.x) & 2047) * 8 + (I))] = \
          __builtin_amdgcn_s_memrealtime();                                              \
  } while (0)
extern "C" int cdn_debug_read_stamps(unsigned long long *host_dst) {
  constexpr size_t kWord = sizeof(unsigned long long);
  int rc = (int)hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(cdn_stamps), kWord * 2 * 16384);
  if (!rc) rc = cdn::read_pointwise_stamps(host_dst + 2 * 16384);
  if (!rc) rc = (int)hipMemcpyFromSymbol(host_dst + 3 * 16384, HIP_SYMBOL(cdn_stamps), kWord * 64, kWord * 2 * 16384);
  return rc;
}
extern "C" int cdn_debug_clear_stamps(void) {
  void *p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(cdn_stamps)) != hipSuccess) return 1;
  const int rc = (int)hipMemset(p, 0, sizeof(unsigned long long) * (2 * 2048 * 8 + 64));
  return rc ? rc : cdn::clear_pointwise_stamps();
}
#define CDN_STAMP_WAVE()                                                                   \
  do {                                                                                     \
    if ((threadIdx.x & 63) == 0 && blockIdx.x == 0 && blockIdx.y == 0)                     \
      cdn_stamps[2 * 16384 + (threadIdx.x >> 6)] = __builtin_amdgcn_s_memrealtime();       \
  } while (0)
#else
#define CDN_STAMPR(R, I) do { } while (0)
#define CDN_STAMP_WAVE() do { } while (0)
#endif
#define CDN_STAMP(I) CDN_STAMPR(1, I)

namespace {

using cdn::fake_quant;

struct Axis {
  int i0;
  float w0, w1;
  bool ok;
};

// Same fp32 position arithmetic as the reference pipeline `h_in + i*dil + anchor*(s-1)`
// (_kernel.cu:226 with modules/dcn_deform_conv.py:325); see codenet_stage.hip.
__device__ __forceinline__ Axis make_axis(int base, float off, int size) {
  Axis a;
  const float pos = (float)base + off;
  a.ok = pos > -1.0f && pos < (float)size;
  const float fl = floorf(pos);
  a.i0 = (int)fl;
  const float l = pos - fl;
  a.w1 = l;
  a.w0 = 1.0f - l;
  if (!a.ok) {
    a.i0 = 0;
    a.w0 = 0.0f;
    a.w1 = 0.0f;
  }
  return a;
}

// (Code8, make_code8, act_code8: the byte codes of the frozen-range schedule, cdn_common.h)
using cdn::BadMask;
using cdn::Code8;
using cdn::act_code8;
using cdn::make_code8;
__device__ __forceinline__ unsigned pack_code8(const float4 &v, const Code8 &c, BadMask &bad) {
  return (unsigned)(act_code8(v.x, c, bad) & 0xff) | ((unsigned)(act_code8(v.y, c, bad) & 0xff) << 8) |
         ((unsigned)(act_code8(v.z, c, bad) & 0xff) << 16) | ((unsigned)act_code8(v.w, c, bad) << 24);
}
// Workgroups are dealt to the 8 XCDs round-robin in launch order, and each XCD has its own L2.  With byte
// tensors a 32- or 64-channel chunk is 32 / 64 bytes of every 128-byte line, so the chunk workgroups of ONE image
// must share an L2 or every line crosses the fabric once per chunk (PMC: 33 MB read for the 8 MB stage-2 input,
// and partial-line writes of d from different XCDs).  Remap (chunk, image) so that XCD k walks the images
// [k*N/8, (k+1)*N/8) chunk by chunk; identity when the grid is not a multiple of 8.  Scalar arithmetic only.
__device__ __forceinline__ void xcd_remap(int &chunk, int &n) {
  const int nch = gridDim.x, total = gridDim.x * gridDim.y;
  if (total & 7) return;
  const int id = blockIdx.y * nch + blockIdx.x;
  const int item = (id & 7) * (total >> 3) + (id >> 3);
  n = item / nch;
  chunk = item - n * nch;
}

// running extremes of a float4 of accumulators: two three-operand instructions per side.  (fminf / fmaxf make the
// compiler quiet each operand first -- v_max_f32 x, x -- which was 16 of the 40 min/max instructions per gather step;
// the operands here are fma results, never signalling NaNs.)
__device__ __forceinline__ float min3f(float a, float b, float c) {
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float max3f(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// (No NaN flag here: the gather kernels are VALU-bound and a compare per output pair cost 15 % of them -- measured.  A NaN
// of d comes from a NaN of x, the weights or s: the gather kernels test what they STAGE instead -- memory-bound phases --
// and a tensor that is NaN throughout, the usual state behind a poisoned range, reduces to the empty pair (+inf, -inf),
// which the range update reads as NaN: cdn_common.h.)
__device__ __forceinline__ void track4(const float4 &a, float &mn, float &mn2, float &mx, float &mx2) {
  mn = min3f(mn, a.x, a.y);
  mn2 = min3f(mn2, a.z, a.w);
  mx = max3f(mx, a.x, a.y);
  mx2 = max3f(mx2, a.z, a.w);
}

// four stored codes -> the fake-quantised values (q + zp) / scale (Markstein division, bit-identical to
// cdn::fake_quant_r of the pre-quantisation value that produced the code)
__device__ __forceinline__ float4 unpack_code8(unsigned u, float scale, float zp, float r) {
  float4 t;
  const float l0 = __fadd_rn((float)(int)(signed char)(u & 0xff), zp), l1 = __fadd_rn((float)(int)(signed char)((u >> 8) & 0xff), zp);
  const float l2 = __fadd_rn((float)(int)(signed char)((u >> 16) & 0xff), zp), l3 = __fadd_rn((float)(int)(signed char)(u >> 24), zp);
  float q0 = __fmul_rn(l0, r); t.x = fmaf(fmaf(-q0, scale, l0), r, q0);
  q0 = __fmul_rn(l1, r); t.y = fmaf(fmaf(-q0, scale, l1), r, q0);
  q0 = __fmul_rn(l2, r); t.z = fmaf(fmaf(-q0, scale, l2), r, q0);
  q0 = __fmul_rn(l3, r); t.w = fmaf(fmaf(-q0, scale, l3), r, q0);
  return t;
}

// ------------------------------------------------------------------------------------------
// scale, NCHW input (stage 0 of the model: x comes from the PyTorch backbone).
// s[n,p] = clamp(b + sum_c w[c]*x[n,c,p]); block min/max -> state.
// ------------------------------------------------------------------------------------------
constexpr int kScaleWaves = 16;
__global__ void __launch_bounds__(kScaleWaves * 64)
scale_nchw_kernel(const float *__restrict__ x, const float *__restrict__ w,
                  const float *__restrict__ b, float *__restrict__ s, cdn::QUpdate qu,
                  int C, int HW, float lo, float hi) {
  CDN_STAMPR(0, 0);
  // 16 waves x 64 pixels: wave v reduces channels v, v+16, ... with 4 loads in flight per lane
  // (~16 KB of 256-byte rows in flight per workgroup) -- the HBM-bound C -> 1 reduction.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * 64 + lane;
  const int n = blockIdx.y;
  const bool live = p < HW;
  const float *xp = x + (long)n * C * HW + (live ? p : 0);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int c = wave;
  constexpr int S = kScaleWaves;
  // 16 loads in flight per lane (one 16-wave workgroup per CU: 8 in flight left the kernel at 2.7 TB/s); the
  // accumulation order is that of the 4-wide loop below (a0 takes c, c + 4S, ...), so the sums are bit-identical
  // to it whatever the unroll
  for (; c + 15 * S < C; c += 16 * S) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = xp[(long)(c + u * S) * HW];
#pragma unroll
    for (int u = 0; u < 16; u += 4) {
      a0 = fmaf(w[c + u * S], v[u], a0);
      a1 = fmaf(w[c + (u + 1) * S], v[u + 1], a1);
      a2 = fmaf(w[c + (u + 2) * S], v[u + 2], a2);
      a3 = fmaf(w[c + (u + 3) * S], v[u + 3], a3);
    }
  }
  for (; c + 3 * S < C; c += 4 * S) {
    const float v0 = xp[(long)c * HW], v1 = xp[(long)(c + S) * HW];
    const float v2 = xp[(long)(c + 2 * S) * HW], v3 = xp[(long)(c + 3 * S) * HW];
    a0 = fmaf(w[c], v0, a0);
    a1 = fmaf(w[c + S], v1, a1);
    a2 = fmaf(w[c + 2 * S], v2, a2);
    a3 = fmaf(w[c + 3 * S], v3, a3);
  }
  for (; c < C; c += S) a0 = fmaf(w[c], xp[(long)c * HW], a0);
  __shared__ float red[kScaleWaves][64];
  red[wave][lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  if (wave == 0) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kScaleWaves; ++i) v += red[i][lane];
    v += b ? b[0] : 0.0f;
    v = cdn::clamp_keep_nan(v, lo, hi);
    if (live) {
      s[(long)n * HW + p] = v;
      mn = mx = v;
      has_nan = (v != v);
    }
  }
  CDN_STAMPR(0, 2);
  if (qu.tracks())
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x,
                             gridDim.x * gridDim.y, qu, &red[0][0]);
  CDN_STAMPR(0, 3);
}

// ------------------------------------------------------------------------------------------
// scale, channels-last input x[pix][C] (stored resolution), optional fake-quant on load.
// One wave per pixel step; lane covers channels 4*lane + 256*j (float4 loads: C % 4 == 0).
// ------------------------------------------------------------------------------------------
template <bool XQ, bool X8 = false>      // X8: x is a byte tensor of codes of the quantiser xq (see Code8)
__global__ void __launch_bounds__(256)
scale_nhwc_kernel(const float *__restrict__ x, const unsigned *__restrict__ xq,
                  const float *__restrict__ w, const float *__restrict__ b, float *__restrict__ s,
                  cdn::QUpdate qu, int C, long npix, float lo, float hi) {
  __shared__ float red[12];
  CDN_STAMPR(0, 0);
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * 4;
  float qs = 1.f, qz = 0.f, qr_ = 1.f;
  if (XQ) {
    qs = reinterpret_cast<const float *>(xq)[2];
    qr_ = __fdiv_rn(1.0f, qs);   // Markstein division in fake_quant_r
    qz = reinterpret_cast<const float *>(xq)[3];
  }
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  // one pixel's dot product (a wave: 64 lanes x 4 channels per round); `take` loads, `dot` consumes -- two pixels'
  // loads are issued before either is consumed (round 5: at stage 1 every wave has exactly two pixels, and the
  // second load used to wait behind the first one's reduction: one memory latency instead of two per launch)
  auto take = [&](long p, int c) -> float4 {
    if (X8)
      return unpack_code8(*reinterpret_cast<const unsigned *>(reinterpret_cast<const signed char *>(x) + p * C + c), qs, qz,
                          qr_);
    return *reinterpret_cast<const float4 *>(x + p * C + c);
  };
  auto dot = [&](float4 v, int c, float acc) -> float {
    const float4 ww = *reinterpret_cast<const float4 *>(w + c);
    if (XQ && !X8) {
      v.x = cdn::fake_quant_r(v.x, qs, qz, qr_);
      v.y = cdn::fake_quant_r(v.y, qs, qz, qr_);
      v.z = cdn::fake_quant_r(v.z, qs, qz, qr_);
      v.w = cdn::fake_quant_r(v.w, qs, qz, qr_);
    }
    acc = fmaf(ww.x, v.x, acc);
    acc = fmaf(ww.y, v.y, acc);
    acc = fmaf(ww.z, v.z, acc);
    return fmaf(ww.w, v.w, acc);
  };
  auto finish = [&](float acc, long p) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
    float v = acc + (b ? b[0] : 0.0f);
    v = cdn::clamp_keep_nan(v, lo, hi);
    if (lane == 0) s[p] = v;
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
    has_nan |= (v != v);
  };
  long p = wave;
  for (; p + nwaves < npix; p += 2 * nwaves) {
    const long p2 = p + nwaves;
    float a0 = 0.f, a1 = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
      const float4 v0 = take(p, c), v1 = take(p2, c);
      a0 = dot(v0, c, a0);
      a1 = dot(v1, c, a1);
    }
    finish(a0, p);
    finish(a1, p2);
  }
  if (p < npix) {
    float acc = 0.f;
    for (int c = lane * 4; c < C; c += 256) acc = dot(take(p, c), c, acc);
    finish(acc, p);
  }
  CDN_STAMPR(0, 2);
  if (qu.tracks()) cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.x, gridDim.x, qu, red);
  CDN_STAMPR(0, 3);
}

// ------------------------------------------------------------------------------------------
// scale, channels-last input, C <= 256: one workgroup = 64 consecutive pixels.  Phase 1 streams the
// tile's 64*C floats as fully coalesced 16-byte loads, ALL of a thread's loads (C/16 <= 16) in flight
// before the first use; each is fake-quantised, dotted with its 4 weights and parked in LDS
// part[pixel][C/4].  Phase 2: 4 threads per pixel sum the partials (conflict-free: row stride
// = 4 mod 32 banks).  Used for large planes only (see the launch site).
// ------------------------------------------------------------------------------------------
constexpr int kScaleTilePix = 64;
template <bool XQ, bool X8 = false>
__global__ void __launch_bounds__(256)
scale_nhwc_tile_kernel(const float *__restrict__ x, const unsigned *__restrict__ xq,
                       const float *__restrict__ w, const float *__restrict__ b,
                       float *__restrict__ s, cdn::QUpdate qu, int C, long npix,
                       float lo, float hi) {
  extern __shared__ float part[];     // [64][LD], then 16 floats of reduction scratch
  CDN_STAMPR(0, 0);
  const int CQ = C >> 2;
  const int LD = ((CQ + 31) & ~31) + 4;
  float *red = part + kScaleTilePix * LD;
  const long pix0 = (long)blockIdx.x * kScaleTilePix;
  const int tile_pix = (int)min((long)kScaleTilePix, npix - pix0);
  const int total = tile_pix * CQ;    // float4 items of this tile
  float qs = 1.f, qz = 0.f, qr_ = 1.f;
  if (XQ) {
    qs = reinterpret_cast<const float *>(xq)[2];
    qr_ = __fdiv_rn(1.0f, qs);   // Markstein division in fake_quant_r
    qz = reinterpret_cast<const float *>(xq)[3];
  }
  const float4 *xt = reinterpret_cast<const float4 *>(x + (X8 ? 0 : pix0 * C));
  const unsigned *xt8 = reinterpret_cast<const unsigned *>(reinterpret_cast<const signed char *>(x) + pix0 * C);
  const float4 *w4 = reinterpret_cast<const float4 *>(w);
  constexpr int U = 16;               // 64 * 64 / 256: every load of a C = 256 tile in flight
  float4 v[U];
  unsigned v8[X8 ? U : 1];
#pragma unroll
  for (int i = 0; i < U; ++i) {
    const int q = threadIdx.x + 256 * i;
    if (X8) v8[X8 ? i : 0] = q < total ? xt8[q] : 0u;
    else v[i] = q < total ? xt[q] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int i = 0; i < U; ++i) {
    const int q = threadIdx.x + 256 * i;
    if (q < total) {
      const int pix = q / CQ, cq = q - pix * CQ;
      const float4 ww = w4[cq];
      float4 t = X8 ? unpack_code8(v8[X8 ? i : 0], qs, qz, qr_) : v[i];
      if (XQ && !X8) {
        t.x = cdn::fake_quant_r(t.x, qs, qz, qr_);
        t.y = cdn::fake_quant_r(t.y, qs, qz, qr_);
        t.z = cdn::fake_quant_r(t.z, qs, qz, qr_);
        t.w = cdn::fake_quant_r(t.w, qs, qz, qr_);
      }
      part[pix * LD + cq] = fmaf(ww.w, t.w, fmaf(ww.z, t.z, fmaf(ww.y, t.y, ww.x * t.x)));
    }
  }
  __syncthreads();
  const int pix = threadIdx.x >> 2, k = threadIdx.x & 3;
  float acc = 0.f;
  if (pix < tile_pix)
    for (int i = k; i < CQ; i += 4) acc += part[pix * LD + i];
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  if (pix < tile_pix) {
    float r = acc + (b ? b[0] : 0.0f);
    r = cdn::clamp_keep_nan(r, lo, hi);
    if (k == 0) s[pix0 + pix] = r;
    mn = mx = r;
    has_nan = (r != r);
  }
  CDN_STAMPR(0, 2);
  if (qu.tracks()) cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.x, gridDim.x, qu, red);
  CDN_STAMPR(0, 3);
}

// ------------------------------------------------------------------------------------------
// dw2: gather + depthwise 3x3, lanes <-> channels.  See file header.
//   x        stage input at STORED resolution (Hl x Wl = (H>>up) x (W>>up)):
//            NHWC_IN ? [n][Hl*Wl][C] : [n][C][Hl*Wl]
//   s_raw    [n][Hl*Wl]  (scale at stored resolution; up-sampling replicates it)
//   d        [n][H*W][C] channels-last output at stage resolution
// ------------------------------------------------------------------------------------------
// (row_fetch / fetch_record / owner_item: the DPP record fetch lives in cdn_common.h, shared with the gather backward)
using cdn::fetch_record;
using cdn::owner_item;
#ifndef CDN_DPP16
#define CDN_DPP16 1      // DPP fetch when an item spans a whole 16-lane row (CCH = 64)
#endif
#ifndef CDN_DPP8
#define CDN_DPP8 1       // DPP fetch for 8-lane items (CCH = 32): two movs per value (1.8 us per step ahead of
                         // ds_bpermute once the tap math was factored; it made no difference before)
#endif
template <int LPP>
constexpr bool use_dpp() { return (LPP == 16 && CDN_DPP16) || (LPP == 8 && CDN_DPP8); }

constexpr int kDw2MaxThreads = 1024;   // workgroup size is chosen per launch (512 or 1024)

// The gather + depthwise of one staged plane:
// img = [(Hl+1)*(Wl+1)][CCH] cells with the zero row / column, wl = [CCH][9] weights, sl = scale plane.
// OUT8: d is a byte tensor of codes (see Code8) instead of fp32; mn / mx are not tracked.
// The input is at the resolution of the output (up-sampled inputs go to dw2u_kernel): img has a zero cell in front
// of it, so the corner columns i0, i0 + 1 of a tap are adjacent cells for every i0 in [-1, W - 1].
template <int CCH, bool OUT8>
__device__ __forceinline__ void dw2_gather(const float4 *img, const float *wl, const float *sl,
                                           float *__restrict__ d, int n, int c0, int C, int H, int W,
                                           int kWaves, float &mn, float &mx, bool &has_nan,
                                           const Code8 *c8 = nullptr, BadMask *bad = nullptr) {
  constexpr bool ADJ = true;
  constexpr int up = 0;
  constexpr int LPP = CCH / 4;     // lanes per pixel
  constexpr int PPW = 64 / LPP;    // pixels per wave step
  const int tid = threadIdx.x;
  const int Hl = H >> up, Wl = W >> up;
  const int HW = H * W;
  const int Wc = Wl + 1;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int lane = tid & 63, wave = tid >> 6;
  const int cq = lane % LPP, sub = lane / LPP;
  float wk[9][4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k][e] = wl[(cq * 4 + e) * 9 + k];

  // byte offsets: row part + column part; out-of-image coordinates select the zero row / column
  const int rstride = Wc * LPP * 16;
  auto row_off = [&](int yy) { return (((unsigned)yy < (unsigned)H) ? (yy >> up) : Hl) * rstride; };
  constexpr int kCell = LPP * 16;
  auto col_off = [&](int xx) {
    if (ADJ) return xx * kCell;                 // xx in [-1, W - 1]: as it is
    return (((unsigned)xx < (unsigned)W) ? (xx >> up) : Wl) * kCell;
  };
  const char *imgb = reinterpret_cast<const char *>(img) + cq * 16;

  const bool vec_store = ((C & 3) == 0);
  // The kernel is VALU-issue bound and the tap geometry is the bulk of the VALU work, so it is
  // computed ONCE per pixel: in the geometry phase lane i owns pixel pb+i (64 different pixels
  // per wave instruction instead of 16 lanes repeating the same pixel); in the gather phase the
  // LPP lanes of an output pixel fetch that pixel's 16-word record from its owner lane with DPP row broadcasts
  // (fetch_record; no LDS storage, no LDS pipeline) and only add offsets, mix and accumulate.
  // every wave owns a contiguous pixel range (a multiple of PPW), so all waves gather even when the
  // plane has fewer than 64 pixels per wave (stage 0: 256 pixels over 8 waves)
  const int ppw = ((HW + kWaves - 1) / kWaves + PPW - 1) / PPW * PPW;
  const int p_begin = wave * ppw, p_end = min(HW, p_begin + ppw);
  for (int pb = p_begin; pb < p_end; pb += 64) {
    // ---- geometry phase ------------------------------------------------------------------
    int g_r[5], g_c[5];
    float g_w[8];
    {
      const int p = min(pb + (use_dpp<LPP>() ? owner_item<LPP>(lane) : lane), HW - 1);
      const int h = p / W, w = p - h * W;
      const float t = sl[(h >> up) * Wl + (w >> up)] - 1.0f;
      const Axis ya = make_axis(h - 1, -t, H), yb = make_axis(h + 1, t, H);
      const Axis xa = make_axis(w - 1, -t, W), xb = make_axis(w + 1, t, W);
      g_r[0] = row_off(ya.i0); g_r[1] = row_off(ya.i0 + 1);
      g_r[2] = row_off(yb.i0); g_r[3] = row_off(yb.i0 + 1);
      g_r[4] = row_off(h);
      g_c[0] = col_off(xa.i0); g_c[1] = ADJ ? 0 : col_off(xa.i0 + 1);
      g_c[2] = col_off(xb.i0); g_c[3] = ADJ ? 0 : col_off(xb.i0 + 1);
      g_c[4] = col_off(w);
      g_w[0] = ya.w0; g_w[1] = ya.w1; g_w[2] = yb.w0; g_w[3] = yb.w1;
      g_w[4] = xa.w0; g_w[5] = xa.w1; g_w[6] = xb.w0; g_w[7] = xb.w1;
    }
    // ---- gather phase: PPW pixels per step ---------------------------------------------------
#pragma unroll 1
    for (int j = 0; j < 64 / PPW; ++j) {
      const int src = j * PPW + sub;          // owner lane of this lane's pixel
      const int p = pb + src;
      int r[5], c[5];
      float wt[8];
#if defined(CDN_DIAG) && CDN_DIAG == 1   // diagnostic build: no cross-lane fetch (wrong results)
#pragma unroll
      for (int q = 0; q < 5; ++q) { r[q] = g_r[q]; c[q] = g_c[q]; }
#pragma unroll
      for (int q = 0; q < 8; ++q) wt[q] = g_w[q];
      (void)src;
#else
      if (use_dpp<LPP>() && ADJ) {
        int gi[8] = {g_r[0], g_r[1], g_r[2], g_r[3], g_r[4], g_c[0], g_c[2], g_c[4]}, oi[8];
        fetch_record<LPP == 8>(j, gi, g_w, oi, wt);
#pragma unroll
        for (int q = 0; q < 5; ++q) r[q] = oi[q];
        c[0] = oi[5]; c[2] = oi[6]; c[4] = oi[7];
      } else if (use_dpp<LPP>()) {
        int gi[10], oi[10];
#pragma unroll
        for (int q = 0; q < 5; ++q) { gi[q] = g_r[q]; gi[5 + q] = g_c[q]; }
        fetch_record<LPP == 8>(j, gi, g_w, oi, wt);
#pragma unroll
        for (int q = 0; q < 5; ++q) { r[q] = oi[q]; c[q] = oi[5 + q]; }
      } else {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
          r[q] = __shfl(g_r[q], src, 64);
          if (!ADJ || !(q & 1)) c[q] = __shfl(g_c[q], src, 64);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) wt[q] = __shfl(g_w[q], src, 64);
      }
      if (ADJ) { c[1] = c[0] + kCell; c[3] = c[2] + kCell; }   // (folded into the reads' immediate offsets)
#endif
      if (pb + j * PPW >= p_end) break;       // wave-uniform: whole step beyond this wave's range
      float4 acc = z4;
#if defined(CDN_DIAG) && CDN_DIAG == 2   // diagnostic build: no LDS cell reads (wrong results)
#define CDN_RD(O) make_float4(__int_as_float(O), 1.f, 2.f, 3.f)
#else
#define CDN_RD(O) (*reinterpret_cast<const float4 *>(imgb + (O)))
#endif
#define CDN_WACC(K, TV)                     \
  acc.x = fmaf(wk[K][0], TV.x, acc.x);      \
  acc.y = fmaf(wk[K][1], TV.y, acc.y);      \
  acc.z = fmaf(wk[K][2], TV.z, acc.z);      \
  acc.w = fmaf(wk[K][3], TV.w, acc.w);
      // the 25 cell offsets of the step: taps 0..8 in order, corner taps (r0c0, r0c1, r1c0, r1c1)
      const int o[25] = {r[0] + c[0], r[0] + c[1], r[1] + c[0], r[1] + c[1],      // tap 0
                         r[0] + c[4], r[1] + c[4],                                // tap 1
                         r[0] + c[2], r[0] + c[3], r[1] + c[2], r[1] + c[3],      // tap 2
                         r[4] + c[0], r[4] + c[1],                                // tap 3
                         r[4] + c[4],                                             // tap 4
                         r[4] + c[2], r[4] + c[3],                                // tap 5
                         r[2] + c[0], r[2] + c[1], r[3] + c[0], r[3] + c[1],      // tap 6
                         r[2] + c[4], r[3] + c[4],                                // tap 7
                         r[2] + c[2], r[2] + c[3], r[3] + c[2], r[3] + c[3]};     // tap 8
      // Reads are issued at their use: under the 128-VGPR cap of the 16-waves-per-CU launch the compiler keeps 2-4 in
      // flight.  (Tried and removed: all 25 reads of a step in flight at <= 256 threads / 256 VGPRs, and a rolling
      // window of 13 -- both slower in the pipeline)
#define CDN_VAL(I) CDN_RD(o[I])
      // corner taps: cells I..I+3, axis weights (Y0,Y1) x (X0,X1)
#define CDN_TAP4(I, Y0, Y1, X0, X1, K)                                    \
  {                                                                       \
    const float4 v00 = CDN_VAL(I), v01 = CDN_VAL(I + 1);                  \
    const float4 v10 = CDN_VAL(I + 2), v11 = CDN_VAL(I + 3);              \
    const float w00 = Y0 * X0, w01 = Y0 * X1, w10 = Y1 * X0, w11 = Y1 * X1; \
    float4 tv;                                                            \
    tv.x = ((w00 * v00.x + w01 * v01.x) + w10 * v10.x) + w11 * v11.x;     \
    tv.y = ((w00 * v00.y + w01 * v01.y) + w10 * v10.y) + w11 * v11.y;     \
    tv.z = ((w00 * v00.z + w01 * v01.z) + w10 * v10.z) + w11 * v11.z;     \
    tv.w = ((w00 * v00.w + w01 * v01.w) + w10 * v10.w) + w11 * v11.w;     \
    CDN_WACC(K, tv)                                                       \
  }
      // edge taps: one axis exact, cells I, I+1 with weights (A0, A1)
#define CDN_TAP2(I, A0, A1, K)                      \
  {                                                 \
    const float4 v0 = CDN_VAL(I), v1 = CDN_VAL(I + 1); \
    float4 tv;                                      \
    tv.x = A0 * v0.x + A1 * v1.x;                   \
    tv.y = A0 * v0.y + A1 * v1.y;                   \
    tv.z = A0 * v0.z + A1 * v1.z;                   \
    tv.w = A0 * v0.w + A1 * v1.w;                   \
    CDN_WACC(K, tv)                                 \
  }
      CDN_TAP4(0, wt[0], wt[1], wt[4], wt[5], 0)
      CDN_TAP2(4, wt[0], wt[1], 1)
      CDN_TAP4(6, wt[0], wt[1], wt[6], wt[7], 2)
      CDN_TAP2(10, wt[4], wt[5], 3)
      {
        const float4 vc = CDN_VAL(12);
        CDN_WACC(4, vc)
      }
      CDN_TAP2(13, wt[6], wt[7], 5)
      CDN_TAP4(15, wt[2], wt[3], wt[4], wt[5], 6)
      CDN_TAP2(19, wt[2], wt[3], 7)
      CDN_TAP4(21, wt[2], wt[3], wt[6], wt[7], 8)
#undef CDN_VAL
#undef CDN_TAP4
#undef CDN_TAP2
#undef CDN_WACC
#undef CDN_RD
      if (OUT8) {
        if (p < p_end && c0 + cq * 4 + 3 < C)       // (C % 4 == 0 is checked by the host)
          reinterpret_cast<unsigned *>(reinterpret_cast<signed char *>(d) + ((long)n * HW + p) * C + c0)[cq] =
              pack_code8(acc, *c8, *bad);
      } else if (p < p_end) {
        float *dp = d + ((long)n * HW + p) * C + c0 + cq * 4;
        const int cbase = c0 + cq * 4;
        if (vec_store && cbase + 3 < C) {
#if defined(CDN_DIAG) && CDN_DIAG == 5   // diagnostic build: no global store of d (wrong results)
          if (acc.x == 1234.5f)
#endif
          *reinterpret_cast<float4 *>(dp) = acc;
          track4(acc, mn, mn, mx, mx);      // one pair: the kernel sits at its 128-VGPR cap
        } else {
          const float av[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cbase + e < C) {
              dp[e] = av[e];
              mn = fminf(mn, av[e]);
              mx = fmaxf(mx, av[e]);
              has_nan |= (av[e] != av[e]);
            }
        }
      }
    }
  }
}

// X8 (with NHWC_IN and XQ): x is a byte tensor of codes of the quantiser xq.  OUT8: d is a byte tensor of codes
// of the quantiser qu.state (frozen: no range tracking, qu.counters is null) and `oflow` is the overflow flag word, set
// when a code saturated; oflow is null for fp32 output.
template <int CCH, bool NHWC_IN, bool XQ, bool SQ, int MAXT, bool X8 = false, bool OUT8 = false>
__global__ void __launch_bounds__(MAXT)
dw2_kernel(const float *__restrict__ x, const unsigned *__restrict__ xq,
           const float *__restrict__ s_raw, const unsigned *__restrict__ sq,
           const float *__restrict__ wd, float *__restrict__ d, unsigned *oflow, cdn::QUpdate qu,
           int C, int H, int W, int up) {
  static_assert(!X8 || (NHWC_IN && XQ), "codes come channels-last with their quantiser state");
  // LDS: [(Hl+1)*(Wl+1)][CCH] image cells; row Hl and column Wl are ZERO and every out-of-image
  // corner coordinate maps there (per-corner zeroing of the reference, _kernel.cu:97-108) -- a
  // cell address is just row offset + column offset, no bounds test and no clamp per corner.
  // Then the chunk's depthwise weights [CCH][9], the scale plane [Hl*Wl], reduction scratch.
  // In front of the image: ONE zero cell, so that cell (r, -1) -- the cell in front of row r -- is always zero
  // (the zero column of row r - 1, or that leading cell): with up == 0 the two corner columns i0, i0 + 1 of a tap
  // are adjacent cells for every i0 in [-1, W - 1] and the gather fetches one column offset per tap class.
  extern __shared__ float4 img_lds[];
  CDN_STAMP(0);
  constexpr int LPP = CCH / 4;     // lanes per pixel
  float4 *img = img_lds + LPP;
  const int kDw2Threads = blockDim.x, kWaves = kDw2Threads / 64;
  const int Hl = H >> up, Wl = W >> up;
  const int HWl = Hl * Wl;
  int n = blockIdx.y, chunk = blockIdx.x;
  if (X8 || OUT8) xcd_remap(chunk, n);
  const int c0 = chunk * CCH;
  const int tid = threadIdx.x;
  const int Wc = Wl + 1;                       // cells per LDS row
  const int cells = (Hl + 1) * Wc;
  float *wl = reinterpret_cast<float *>(img + (size_t)cells * LPP);
  float *sl = wl + CCH * 9;
  float *red = sl + HWl;
  float xs = 1.f, xz = 0.f, ss = 1.f, sz = 0.f, xr_ = 1.f;
  if (XQ) {
    xs = reinterpret_cast<const float *>(xq)[2];
    xr_ = __fdiv_rn(1.0f, xs);   // Markstein division in fake_quant_r
    xz = reinterpret_cast<const float *>(xq)[3];
  }
  if (SQ) {
    ss = reinterpret_cast<const float *>(sq)[2];
    sz = reinterpret_cast<const float *>(sq)[3];
  }
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int q = tid; q < (Wc + Hl) * LPP; q += kDw2Threads) {   // zero row, then zero column
    const int i = q / LPP;
    const int cell = i < Wc ? Hl * Wc + i : (i - Wc) * Wc + Wl;
    img[cell * LPP + (q % LPP)] = z4;
  }
  if (tid < LPP) img_lds[tid] = z4;                            // the leading zero cell
  // the chunk's depthwise weights and the scale plane are requested BEFORE the image (one element per thread;
  // stored to LDS after it), so their round trips overlap the image's instead of following it
  const float w_pre = (tid < CCH * 9 && c0 + tid / 9 < C) ? wd[(long)c0 * 9 + tid] : 0.0f;
  const float s_pre = tid < HWl ? s_raw[(long)n * HWl + tid] : 0.0f;
  // ---- stage the image -------------------------------------------------------------------
  // All of a thread's global loads of a batch are issued before the first one is used (kStageU in
  // flight per thread); a plain loop leaves ONE dependent load per thread in flight and the
  // staging then costs a full HBM round trip per iteration (measured: 21 of 58 us at stage 0).
  constexpr int kStageU = 8;
  // a NaN of d comes from a NaN of what is staged here (x, the weights): tested in this memory-bound phase, not per output
  bool has_nan = (w_pre != w_pre);
  if (X8) {
    const signed char *xg = reinterpret_cast<const signed char *>(x) + (long)n * HWl * C + c0;
    const int total = HWl * LPP;
    for (int base = 0; base < total; base += kDw2Threads * kStageU) {
      unsigned v[kStageU];
#pragma unroll
      for (int u = 0; u < kStageU; ++u) {
        const int q = base + u * kDw2Threads + tid;
        const int pix = q / LPP, cq = q % LPP;
        v[u] = 0u;
        if (q < total && c0 + cq * 4 + 3 < C) v[u] = *reinterpret_cast<const unsigned *>(xg + (long)pix * C + cq * 4);
      }
#pragma unroll
      for (int u = 0; u < kStageU; ++u) {
        const int q = base + u * kDw2Threads + tid;
        const int pix = q / LPP, cq = q % LPP;
        if (q < total)
          img[((pix / Wl) * Wc + (pix % Wl)) * LPP + cq] =
              (c0 + cq * 4 + 3 < C) ? unpack_code8(v[u], xs, xz, xr_) : z4;
      }
    }
  } else if (NHWC_IN) {
    const float *xg = x + (long)n * HWl * C + c0;
    const int total = HWl * LPP;
    for (int base = 0; base < total; base += kDw2Threads * kStageU) {
      float4 v[kStageU];
#pragma unroll
      for (int u = 0; u < kStageU; ++u) {
        const int q = base + u * kDw2Threads + tid;
        const int pix = q / LPP, cq = q % LPP;
        v[u] = z4;
        if (q < total && c0 + cq * 4 + 3 < C)
          v[u] = *reinterpret_cast<const float4 *>(xg + (long)pix * C + cq * 4);
      }
#pragma unroll
      for (int u = 0; u < kStageU; ++u) {
        const int q = base + u * kDw2Threads + tid;
        const int pix = q / LPP, cq = q % LPP;
        if (q < total) {
          float4 t = v[u];
          if (XQ) {
            t.x = cdn::fake_quant_r(t.x, xs, xz, xr_);
            t.y = cdn::fake_quant_r(t.y, xs, xz, xr_);
            t.z = cdn::fake_quant_r(t.z, xs, xz, xr_);
            t.w = cdn::fake_quant_r(t.w, xs, xz, xr_);
          }
          has_nan |= __builtin_isunordered(t.x, t.y) | __builtin_isunordered(t.z, t.w);
          img[((pix / Wl) * Wc + (pix % Wl)) * LPP + cq] = t;
        }
      }
    }
  } else {
    // lane <-> channel so the four scalar LDS stores of a wave hit consecutive banks
    float *imgf = reinterpret_cast<float *>(img);
    const int quads = (HWl + 3) >> 2;
    const int total = quads * CCH;
    if ((HWl & 3) == 0) {
      for (int base = 0; base < total; base += kDw2Threads * kStageU) {
        float4 v[kStageU];
#pragma unroll
        for (int u = 0; u < kStageU; ++u) {
          const int q = base + u * kDw2Threads + tid;
          const int cl = q % CCH, j = q / CCH;
          const int c = min(c0 + cl, C - 1), jj = min(j, quads - 1);   // clamped: always a valid load
          v[u] = *reinterpret_cast<const float4 *>(x + ((long)n * C + c) * HWl + jj * 4);
        }
#pragma unroll
        for (int u = 0; u < kStageU; ++u) {
          const int q = base + u * kDw2Threads + tid;
          const int cl = q % CCH, j = q / CCH;
          if (q < total) {
            const bool live = c0 + cl < C;
            const float e4[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int pix = j * 4 + e;
              const float t = XQ ? cdn::fake_quant_r(e4[e], xs, xz, xr_) : e4[e];
              has_nan |= live && (t != t);
              imgf[((pix / Wl) * Wc + (pix % Wl)) * CCH + cl] = live ? t : 0.0f;
            }
          }
        }
      }
    } else {
      for (int q = tid; q < total; q += kDw2Threads) {
        const int cl = q % CCH, j = q / CCH;
        const int c = c0 + cl;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < C) {
          const float *xp = x + ((long)n * C + c) * HWl + j * 4;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (j * 4 + e < HWl) v[e] = xp[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int pix = j * 4 + e;
          if (pix < HWl) {
            const float t = XQ ? cdn::fake_quant_r(v[e], xs, xz, xr_) : v[e];
            has_nan |= (t != t);
            imgf[((pix / Wl) * Wc + (pix % Wl)) * CCH + cl] = t;
          }
        }
      }
    }
  }
  // ---- chunk weights (coalesced) and the (fake-quantised) scale plane: first element per thread prefetched ----
  if (tid < CCH * 9) wl[tid] = w_pre;
  for (int q = tid + kDw2Threads; q < CCH * 9; q += kDw2Threads)
    wl[q] = (c0 + q / 9 < C) ? wd[(long)c0 * 9 + q] : 0.0f;
  if (tid < HWl) sl[tid] = SQ ? fake_quant(s_pre, ss, sz) : s_pre;
  for (int q = tid + kDw2Threads; q < HWl; q += kDw2Threads) {
    float sv = s_raw[(long)n * HWl + q];
    if (SQ) sv = fake_quant(sv, ss, sz);
    sl[q] = sv;
  }
  CDN_STAMP(1);
  __syncthreads();
  CDN_STAMP(2);
  float mn = INFINITY, mx = -INFINITY;
  if (OUT8) {
    BadMask bad = 0;
    const Code8 c8 = make_code8(qu.state, bad);
    dw2_gather<CCH, true>(img, wl, sl, d, n, c0, C, H, W, kWaves, mn, mx, has_nan, &c8, &bad);
    if (bad) atomicOr(oflow, 1u);
    return;
  }
  dw2_gather<CCH, false>(img, wl, sl, d, n, c0, C, H, W, kWaves, mn, mx, has_nan);
  CDN_STAMP_WAVE();
  CDN_STAMP(3);
  if (qu.tracks())
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x,
                             gridDim.x * gridDim.y, qu, red);
  CDN_STAMP(4);
}

// ------------------------------------------------------------------------------------------
// dw0p: PERSISTENT form of dw2_kernel<64> for an NCHW fp32 input at output resolution (stage 0 of the model),
// with the next item's input in flight by LDS-DMA while the current item is gathered.
//
// dw2_kernel runs stage 0 as two rounds of two 512-thread workgroups per CU that stage (HBM) and gather (LDS / VALU)
// in lock-step: HBM idles during the gather and the SIMDs idle during staging (in-kernel stamps).
// A register-staged double buffer cannot be built under the 128-VGPR cap of 16 waves per CU.  Here ONE 1024-thread
// workgroup per CU walks over its items (image n, 64-channel chunk):
//
//   raw   [64][HW] floats  <- global_load_lds_dwordx4 (no VGPRs): an item's 64 channel planes are ONE contiguous
//                             64*HW*4-byte block of the NCHW tensor; 1-KB pieces, each lane's 16 bytes = 4 pixels of a
//                             channel, stored at slot (quad ^ (channel & 15)) of the channel's row -- the XOR is
//                             applied to the per-lane SOURCE address (the DMA's LDS side is lane-linear), so that
//   img   [cell][64]       <- the transposing pass (lane <-> channel: ds_read_b128 of raw, four ds_write_b32 into the
//                             [cell][channel] image the gather wants) reads 16 different 16-byte bank groups per
//                             hardware lane group and writes 32 consecutive banks: conflict-free both ways;
//   wl, sl (two sets)      <- global_load_lds_dword: the chunk's depthwise weights and the image's scale plane.
//
//   per item:  wait for this item's DMA | barrier | raw -> img (+ fake-quant of s) | barrier |
//              issue the NEXT item's DMA into raw / the other (wl, sl) set | gather this item (dw2_gather, unchanged).
//
// Same arithmetic as dw2_kernel (same staged values, same gather routine): results are bit-identical to it.
// Needs W % 4 == 0, H*W a power of two >= 64 (whole 1-KB pieces per channel group, shifts instead of divisions in the
// per-step DMA issue), C % 64 == 0.
// ------------------------------------------------------------------------------------------
// LDS-DMA as inline asm, on purpose: with __builtin_amdgcn_global_load_lds the compiler orders every later LDS
// read of the wave behind the pending DMA (it cannot prove that the gather's image reads do not alias the raw
// buffer being filled) and emits s_waitcnt vmcnt(0) right after the issue -- the next item's transfer was then
// fully exposed (in-kernel stamps: 9.0 / 11.6 / 13.8 us per item with the DMA "in flight" against 4.5 us for the last
// item without one).  The asm form is invisible to that bookkeeping; completion is waited for explicitly
// (s_waitcnt vmcnt(0) + barrier at the top of every item).  M0 = wave-uniform LDS byte address of the piece, the
// lane's 16 (4) bytes land at M0 + lane * 16 (4); M0 is saved and restored (compiler-reserved register).
// (glds16 / glds4 / lds_addr_uniform: cdn_common.h, shared with the training path's pointwise kernel)
using cdn::glds16;
using cdn::glds4;
using cdn::lds_addr_uniform;

template <bool SQ, bool OUT8>
__global__ void __launch_bounds__(1024)
dw0p_kernel(const float *__restrict__ x, const float *__restrict__ s_raw, const unsigned *__restrict__ sq,
            const float *__restrict__ wd, float *__restrict__ d, unsigned *oflow, cdn::QUpdate qu,
            int C, int H, int W, int nitems, int Cx) {
  // Cx = channels of x / wd; C = row length of d, a multiple of 64 >= Cx.  Cx < C (round 4: CoDeNet2x, 2153 = 33 * 64 +
  // 41): the last chunk is RAGGED -- its missing planes and weights are fetched from the chunk's LAST REAL channel
  // (clamped source addresses: no read outside the tensors, no predicated DMA), so the pad channels of d are exact
  // duplicates of channel Cx - 1: the {min, max} of d are unchanged and the pointwise kernel multiplies them by its
  // zero-padded weight codes.
  extern __shared__ float4 img_lds[];
  CDN_STAMP(0);
  constexpr int CCH = 64, LPP = 16, kWaves = 16;
  const int HW = H * W, Wc = W + 1, cells = (H + 1) * Wc;
  const int Q = HW >> 2;                      // 16-byte quads per channel plane
  const int nchunk = C / CCH;
  float4 *img = img_lds + LPP;
  float *raw = reinterpret_cast<float *>(img + (size_t)cells * LPP);
  float *wl0 = raw + CCH * HW;                // two sets of [64][9]
  float *sl0 = wl0 + 2 * CCH * 9;             // two sets of [HW]
  float *red = sl0 + 2 * HW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float ss = 1.f, sz = 0.f;
  if (SQ) {
    ss = reinterpret_cast<const float *>(sq)[2];
    sz = reinterpret_cast<const float *>(sq)[3];
  }
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int q = tid; q < (Wc + H) * LPP; q += 1024) {   // zero row, then zero column: written once
    const int i = q / LPP;
    const int cell = i < Wc ? H * Wc + i : (i - Wc) * Wc + W;
    img[cell * LPP + (q % LPP)] = z4;
  }
  if (tid < LPP) img_lds[tid] = z4;                    // the leading zero cell

  const int npiece_w = CCH * 9 / 64, npiece_s = HW / 64;
  const unsigned raw_a = lds_addr_uniform(raw), wl_a = lds_addr_uniform(wl0), sl_a = lds_addr_uniform(sl0);
  // DMA of one item = Q 1-KB pieces of the raw buffer (wave w: pieces w, w + 16, ...) + the small pieces (weights,
  // scale plane).  issue_step(item, set, k): the wave's k-th raw piece, and with k == 0 its small piece.
  const int qsh = 31 - __builtin_clz(Q);                           // Q is a power of two (host check)
  auto issue_step = [&](int item, int set, int k) {
    const int n = item / nchunk, chunk = item - n * nchunk;
    const int piece = __builtin_amdgcn_readfirstlane(wave + kWaves * k);
    if (piece < Q) {                                               // Q pieces of 1 KB = 64 * HW * 4 bytes
      const int idx = piece * 64 + lane;                           // 16-byte slot of the raw buffer
      const int c = idx >> qsh, slot = idx & (Q - 1);
      const int cs = min(c, Cx - 1 - chunk * CCH);                 // ragged last chunk: the last real channel again
#if defined(CDN_DIAG) && CDN_DIAG == 8   // diagnostic build: every item reads the planes of item 0 (wrong results)
      glds16(x, (unsigned)(((cs << qsh) + (slot ^ (c & 15))) << 4), raw_a + piece * 1024);
#else
      glds16(x + ((long)n * Cx + (long)chunk * CCH) * HW, (unsigned)(((cs << qsh) + (slot ^ (c & 15))) << 4),
             raw_a + piece * 1024);
#endif
    }
    if (k == 0)
      for (int sp = wave; sp < npiece_w + npiece_s; sp += kWaves) {
        if (sp < npiece_w) {
          // (ragged last chunk: weight 9 c + k of a pad channel c comes from the last real channel)
          const int wi = sp * 64 + lane, wc = wi / 9, wlast = Cx - 1 - chunk * CCH;
          const int wsrc = wc <= wlast ? wi : wlast * 9 + (wi - wc * 9);
          glds4(wd + (long)chunk * CCH * 9, (unsigned)wsrc * 4, wl_a + (set * CCH * 9 + sp * 64) * 4);
        }
        else
          glds4(s_raw + (long)n * HW + (sp - npiece_w) * 64, lane * 4, sl_a + (set * HW + (sp - npiece_w) * 64) * 4);
      }
  };
  const int npieces = (Q + kWaves - 1) / kWaves;                   // raw pieces per wave
  auto issue = [&](int item, int set, int k0) {
    for (int k = k0; k < max(npieces, 1); ++k) issue_step(item, set, k);
  };
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  BadMask bad = 0;
  Code8 c8 = {1.f, 0.f};
  if (OUT8) c8 = make_code8(qu.state, bad);
  // (tried: s_setprio(1) for the second-dispatched half of the waves -- 0.2514 vs 0.2508 ms per step, nothing)
  int item = blockIdx.x, set = 0;
  if (item < nitems) issue(item, 0, 0);
  for (; item < nitems; item += gridDim.x, set ^= 1) {
    const int n = item / nchunk, chunk = item - n * nchunk;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the item's DMA have landed ...
    __syncthreads();       // ... everybody's have, and everybody is done with img and the other (wl, sl) set
    CDN_STAMP(1);
    if (item == (int)blockIdx.x) CDN_STAMP(5);
    // ---- raw -> img: lane <-> channel, wave w takes quads w, w + 16, ... -----------------------------------
    float *imgf = reinterpret_cast<float *>(img);
    int ln = lane;
    asm volatile("" : "+v"(ln));
    for (int qd = wave; qd < Q; qd += kWaves) {
      const float4 v = *reinterpret_cast<const float4 *>(raw + (ln * Q + (qd ^ (ln & 15))) * 4);
      const int p = qd * 4, row = p / W, col = p - row * W;         // W % 4 == 0: one row
      float *dst = imgf + (row * Wc + col) * CCH + ln;
      dst[0] = v.x; dst[CCH] = v.y; dst[2 * CCH] = v.z; dst[3 * CCH] = v.w;
      has_nan |= __builtin_isunordered(v.x, v.y) | __builtin_isunordered(v.z, v.w);   // (see track4: x is tested where it is staged)
    }
    float *sl = sl0 + set * HW;
    if (SQ) for (int q = tid; q < HW; q += 1024) sl[q] = fake_quant(sl[q], ss, sz);
    __syncthreads();
    CDN_STAMP(2);
    // the NEXT item's transfer: in flight during the gather below.  (Issuing one raw piece per gather step instead of
    // the 64-KB burst was built and measured: no difference, 0.2521 vs 0.2524 ms per step, and the hook cost the
    // byte-code instantiation 20 spilled VGPRs.)
    const int nxt = item + gridDim.x;
    if (nxt < nitems) issue(nxt, set ^ 1, 0);
    if (OUT8) dw2_gather<CCH, true>(img, wl0 + set * CCH * 9, sl, d, n, chunk * CCH, C, H, W, kWaves, mn, mx, has_nan, &c8, &bad);
    else dw2_gather<CCH, false>(img, wl0 + set * CCH * 9, sl, d, n, chunk * CCH, C, H, W, kWaves, mn, mx, has_nan);
    CDN_STAMP(3);
    if (item == (int)blockIdx.x) CDN_STAMP(6);
    if (item == (int)(blockIdx.x + gridDim.x)) CDN_STAMP(7);
  }
  if (OUT8) {
    if (bad) atomicOr(oflow, 1u);
    return;
  }
  if (qu.tracks()) cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.x, gridDim.x, qu, red);
  CDN_STAMP(4);
}

// ------------------------------------------------------------------------------------------
// dw2u: the gather + depthwise kernel for an UP-SAMPLED input (up = 1, channels-last, stages >= 1),
// processing one 2x2 block of output pixels -- one stored pixel (Y,X) -- per lane group.
//
// The four output pixels of a block share the scale s (it is predicted at the stored resolution),
// so their tap positions are translates of each other by one output pixel = half a stored cell.
// Along one axis the 2+2 bilinear corners of the two pixels fall into at most TWO consecutive
// stored cells {cb, cb+1}: a corner tap needs 2x2 = 4 cell reads for the WHOLE block instead of 16,
// an edge tap 2 instead of 8, the centre tap 1 instead of 4 -- 25 ds_read_b128 per 16 outputs/lane
// instead of 100, and one geometry record per block instead of four.  Each pixel keeps its own
// fp32 corner weights (positions bit-identical to the reference pipeline); they are folded onto the
// two cells per axis, W[slot] = sum of the corner weights that land in that cell.  (If fp32 rounding
// makes a pixel's far corner land one cell further -- its weight is then ~1 ulp -- it is folded
// into slot 1; the effect is below 1e-6 of the value.)
// ------------------------------------------------------------------------------------------
struct AxisRaw {
  int fl;      // floor(pos), NOT parked
  float w0, w1;  // corner weights, zero when the sample is out of range on this axis
};

__device__ __forceinline__ AxisRaw make_axis_raw(int base, float off, int size) {
  AxisRaw a;
  const float pos = (float)base + off;
  const bool ok = pos > -1.0f && pos < (float)size;
  const float fl = floorf(pos);
  // clamp the index so far-out-of-range positions (|s| is not bounded by this kernel) stay sane
  a.fl = (int)fminf(fmaxf(fl, -4.0f), (float)size + 4.0f);
  const float l = pos - fl;
  a.w1 = ok ? l : 0.0f;
  a.w0 = ok ? 1.0f - l : 0.0f;
  return a;
}

// Fold the two pixels (a: lower coordinate, b = a + 1) of one axis class onto cells {cb, cb+1}.
// out[0..1] = pixel a's slot weights, out[2..3] = pixel b's.  Returns cb (stored-cell index).
__device__ __forceinline__ int fold_axis(const AxisRaw &a, const AxisRaw &b, float *out) {
  const int cb = a.fl >> 1;
  const int sa1 = min(max(((a.fl + 1) >> 1) - cb, 0), 1);
  const int sb0 = min(max((b.fl >> 1) - cb, 0), 1);
  const int sb1 = min(max(((b.fl + 1) >> 1) - cb, 0), 1);
  out[0] = a.w0 + (sa1 == 0 ? a.w1 : 0.0f);
  out[1] = (sa1 == 1 ? a.w1 : 0.0f);
  out[2] = (sb0 == 0 ? b.w0 : 0.0f) + (sb1 == 0 ? b.w1 : 0.0f);
  out[3] = (sb0 == 1 ? b.w0 : 0.0f) + (sb1 == 1 ? b.w1 : 0.0f);
  return cb;
}

#ifndef CDN_UNEVEN_SPLIT
#define CDN_UNEVEN_SPLIT 1
#endif
constexpr bool kUnevenSplit = CDN_UNEVEN_SPLIT != 0;

template <int CCH, bool XQ, bool SQ, bool X8 = false, bool OUT8 = false>   // X8 / OUT8: see dw2_kernel
__global__ void __launch_bounds__(512)   // ~250 VGPRs: 2 waves/SIMD (168 spills and is 2.5x slower)
dw2u_kernel(const float *__restrict__ x, const unsigned *__restrict__ xq,
            const float *__restrict__ s_raw, const unsigned *__restrict__ sq,
            const float *__restrict__ wd, float *__restrict__ d, unsigned *oflow, cdn::QUpdate qu,
            int C, int H, int W, cdn::ScaleFromSums si) {
  static_assert(!X8 || XQ, "codes come with their quantiser state");
  // LDS: one ZERO cell, then the image as in dw2_kernel.  Cell (r, -1) is the cell in front of row r: the zero
  // column of row r - 1, or the leading zero cell for r = 0 -- so column -1 needs no parking and the two cells
  // {cb, cb + 1} of a column class are ALWAYS adjacent: one offset per class, the second read is the first plus
  // an immediate.
  extern __shared__ float4 img_lds[];
  CDN_STAMP(0);
  constexpr int LPP = CCH / 4;     // lanes per block (one float4 of channels each)
  float4 *img = img_lds + LPP;
  constexpr int PPW = 64 / LPP;    // blocks per wave step
  const int nthreads = blockDim.x, nwaves = nthreads / 64;
  const int Hl = H >> 1, Wl = W >> 1;
  const int HWl = Hl * Wl, HW = H * W;
  int n = blockIdx.y, chunk = blockIdx.x;
  if (X8 || OUT8) xcd_remap(chunk, n);
  const int c0 = chunk * CCH;
  const int tid = threadIdx.x;
  const int Wc = Wl + 1;
  const int cells = (Hl + 1) * Wc;
  float *wl = reinterpret_cast<float *>(img + (size_t)cells * LPP);
  float *sl = wl + CCH * 9;
  float *red = sl + HWl;
  float xs = 1.f, xz = 0.f, ss = 1.f, sz = 0.f, xr_ = 1.f;
  if (XQ) {
    xs = reinterpret_cast<const float *>(xq)[2];
    xr_ = __fdiv_rn(1.0f, xs);   // Markstein division in fake_quant_r
    xz = reinterpret_cast<const float *>(xq)[3];
  }
  if (SQ) {
    ss = reinterpret_cast<const float *>(sq)[2];
    sz = reinterpret_cast<const float *>(sq)[3];
  }
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int q = tid; q < (Wc + Hl) * LPP; q += nthreads) {   // zero row, then zero column
    const int i = q / LPP;
    const int cell = i < Wc ? Hl * Wc + i : (i - Wc) * Wc + Wl;
    img[cell * LPP + (q % LPP)] = z4;
  }
  if (tid < LPP) img_lds[tid] = z4;                          // the leading zero cell
  // weights and scale plane requested before the image (see dw2_kernel)
  const float w_pre = (tid < CCH * 9 && c0 + tid / 9 < C) ? wd[(long)c0 * 9 + tid] : 0.0f;
  // scale plane: from the scale kernel, or (frozen chained stages) from the producer's exact integer sums --
  // s_raw = clamp(bias + sums / (sw * sc_x)): ONE rounding of the exact sum instead of the fp32 sum of C products
  float s_inv = 0.f, s_b = 0.f;
  if (XQ && si.sums) {
    s_inv = __fdiv_rn(1.0f, __fmul_rn(si.sw[0], xs));
    s_b = si.bias ? si.bias[0] : 0.0f;
  }
  const float f_b = (si.fparts && si.bias) ? si.bias[0] : 0.0f;
  const long f_stride = (long)gridDim.y * HWl;               // one plane of partial sums: every stored pixel of the batch
  auto s_at = [&](int q) -> float {
    if (XQ && si.sums) return fminf(fmaxf(fmaf((float)si.sums[(long)n * HWl + q], s_inv, s_b), si.lo), si.hi);
    if (!XQ && !SQ && si.fparts) {      // fp32 chained stages: the producer's per-column-tile partial sums, in plane order
      const float *fp = si.fparts + (long)n * HWl + q;
      float a = fp[0];
      for (int j = 1; j < si.nparts; ++j) a += fp[j * f_stride];
      return cdn::clamp_keep_nan(a + f_b, si.lo, si.hi);
    }
    return s_raw[(long)n * HWl + q];
  };
  const float s_pre = tid < HWl ? s_at(tid) : 0.0f;
  if (X8) {
    constexpr int kStageU = 8;
    const signed char *xg = reinterpret_cast<const signed char *>(x) + (long)n * HWl * C + c0;
    const int total = HWl * LPP;
    for (int base = 0; base < total; base += nthreads * kStageU) {
      unsigned v[kStageU];
#pragma unroll
      for (int u = 0; u < kStageU; ++u) {
        const int q = base + u * nthreads + tid;
        const int pix = q / LPP, cq4 = q % LPP;
        v[u] = 0u;
        if (q < total && c0 + cq4 * 4 + 3 < C) v[u] = *reinterpret_cast<const unsigned *>(xg + (long)pix * C + cq4 * 4);
      }
#pragma unroll
      for (int u = 0; u < kStageU; ++u) {
        const int q = base + u * nthreads + tid;
        const int pix = q / LPP, cq4 = q % LPP;
        if (q < total)
          img[((pix / Wl) * Wc + (pix % Wl)) * LPP + cq4] =
              (c0 + cq4 * 4 + 3 < C) ? unpack_code8(v[u], xs, xz, xr_) : z4;
      }
    }
  } else {
    // batched: kStageU loads per thread in flight (see dw2_kernel)
    constexpr int kStageU = 8;
    const float *xg = x + (long)n * HWl * C + c0;
    const int total = HWl * LPP;
    for (int base = 0; base < total; base += nthreads * kStageU) {
      float4 v[kStageU];
#pragma unroll
      for (int u = 0; u < kStageU; ++u) {
        const int q = base + u * nthreads + tid;
        const int pix = q / LPP, cq4 = q % LPP;
        v[u] = z4;
        if (q < total && c0 + cq4 * 4 + 3 < C)
          v[u] = *reinterpret_cast<const float4 *>(xg + (long)pix * C + cq4 * 4);
      }
#pragma unroll
      for (int u = 0; u < kStageU; ++u) {
        const int q = base + u * nthreads + tid;
        const int pix = q / LPP, cq4 = q % LPP;
        if (q < total) {
          float4 t = v[u];
          if (XQ) {
            t.x = cdn::fake_quant_r(t.x, xs, xz, xr_);
            t.y = cdn::fake_quant_r(t.y, xs, xz, xr_);
            t.z = cdn::fake_quant_r(t.z, xs, xz, xr_);
            t.w = cdn::fake_quant_r(t.w, xs, xz, xr_);
          }
          img[((pix / Wl) * Wc + (pix % Wl)) * LPP + cq4] = t;
        }
      }
    }
  }
  if (tid < CCH * 9) wl[tid] = w_pre;
  for (int q = tid + nthreads; q < CCH * 9; q += nthreads)
    wl[q] = (c0 + q / 9 < C) ? wd[(long)c0 * 9 + q] : 0.0f;
  if (tid < HWl) sl[tid] = SQ ? fake_quant(s_pre, ss, sz) : s_pre;
  for (int q = tid + nthreads; q < HWl; q += nthreads) {
    float sv = s_at(q);
    if (SQ) sv = fake_quant(sv, ss, sz);
    sl[q] = sv;
  }
  CDN_STAMP(1);
  __syncthreads();
  CDN_STAMP(2);
  const int lane = tid & 63, wave = tid >> 6;
  const int cq = lane % LPP, sub = lane / LPP;
  float wk[9][4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k][e] = wl[(cq * 4 + e) * 9 + k];

  const int rstride = Wc * LPP * 16;
  // stored-cell index -> byte offset (out-of-image cells select the zero row / column)
  auto row_off = [&](int cy) { return (((unsigned)cy < (unsigned)Hl) ? cy : Hl) * rstride; };
  // first cell of a column class: cb in [-1, Wl - 1] as it is (cells cb, cb + 1 lie in [-1, Wl]); outside that
  // range every weight of the class is zero (fold_axis), any pair of cells will do
  constexpr int kCell = LPP * 16;
  auto col_off = [&](int cb) { return min(max(cb, -1), Wl - 1) * kCell; };
  const char *imgb = reinterpret_cast<const char *>(img) + cq * 16;
#if defined(CDN_DIAG) && CDN_DIAG == 2   // diagnostic build: no LDS cell reads (wrong results)
#define CDN_RD(O) make_float4(__int_as_float(O), 1.f, 2.f, 3.f)
#else
#define CDN_RD(O) (*reinterpret_cast<const float4 *>(imgb + (O)))
#endif

  float mn = INFINITY, mx = -INFINITY, mn2 = INFINITY, mx2 = -INFINITY;

  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  BadMask bad = 0;
  Code8 c8 = {1.f, 0.f};
  if (OUT8) c8 = make_code8(qu.state, bad);
  const bool vec_store = ((C & 3) == 0);
  // every wave owns a contiguous range of blocks (= stored pixels).  The second-dispatched half of the waves
  // (4..7) loses the oldest-first arbitration of VALU / LDS issue on every step and finishes ~30 % later than the
  // first half on equal ranges (in-kernel per-wave stamps: 20.2 vs 26.0 us at stage 2); with >= 12 steps per wave
  // the first half therefore takes 9/16 of the steps.  (Fixed assignment: results do not depend on it.)
  int b_begin, b_end;
  {
    const int steps = (HWl + PPW - 1) / PPW, half = nwaves / 2;
    if (kUnevenSplit && (nwaves & 1) == 0 && steps >= 12 * nwaves) {
      const int old_each = (steps * 9 / 16 + half - 1) / half;           // steps per wave, first half
      const int old_total = min(steps, old_each * half);
      const int young_each = (steps - old_total + half - 1) / half;
      const int s0 = wave < half ? wave * old_each : old_total + (wave - half) * young_each;
      const int s1 = wave < half ? min(old_total, s0 + old_each) : s0 + young_each;
      b_begin = min(HWl, s0 * PPW);
      b_end = min(HWl, s1 * PPW);
    } else {
      const int bpw = ((HWl + nwaves - 1) / nwaves + PPW - 1) / PPW * PPW;
      b_begin = min(HWl, wave * bpw);
      b_end = min(HWl, b_begin + bpw);
    }
  }
  for (int bb = b_begin; bb < b_end; bb += 64) {
    // ---- geometry phase: lane i owns block bb + i -----------------------------------------------
    int g_o[9];       // byte offsets: rows {ya: r0,r1; yb: r0,r1; mid}, cols {xa, xb: first cell; mid}; [8]: the
                      // block's first output pixel 2Y * W + 2X
    float g_w[16];    // slot weights [class ya,yb,xa,xb][pixel a/b][slot 0/1]
    {
      const int blk = min(bb + (use_dpp<LPP>() ? owner_item<LPP>(lane) : lane), HWl - 1);
      const int Y = blk / Wl, X = blk - Y * Wl;
      const int h0 = 2 * Y, w0 = 2 * X;
      const float t = sl[blk] - 1.0f;
      // tap row i = 0: pos = (h - 1) - t ; i = 2: pos = (h + 1) + t ; pixel rows h0 and h0 + 1
      const AxisRaw ya_a = make_axis_raw(h0 - 1, -t, H), ya_b = make_axis_raw(h0, -t, H);
      const AxisRaw yb_a = make_axis_raw(h0 + 1, t, H), yb_b = make_axis_raw(h0 + 2, t, H);
      const AxisRaw xa_a = make_axis_raw(w0 - 1, -t, W), xa_b = make_axis_raw(w0, -t, W);
      const AxisRaw xb_a = make_axis_raw(w0 + 1, t, W), xb_b = make_axis_raw(w0 + 2, t, W);
      const int rya = fold_axis(ya_a, ya_b, &g_w[0]);
      const int ryb = fold_axis(yb_a, yb_b, &g_w[4]);
      const int cxa = fold_axis(xa_a, xa_b, &g_w[8]);
      const int cxb = fold_axis(xb_a, xb_b, &g_w[12]);
      g_o[0] = row_off(rya); g_o[1] = row_off(rya + 1);
      g_o[2] = row_off(ryb); g_o[3] = row_off(ryb + 1);
      g_o[4] = row_off(Y);
      g_o[5] = col_off(cxa);
      g_o[6] = col_off(cxb);
      g_o[7] = X * kCell;
      g_o[8] = h0 * W + w0;
    }
    // ---- gather phase: PPW blocks per step -----------------------------------------------------
#pragma unroll 1
    for (int j = 0; j < 64 / PPW; ++j) {
      const int src = j * PPW + sub;
      const int blk = bb + src;
      int o[9];
      float w[16];
      if (use_dpp<LPP>()) {
        fetch_record<LPP == 8>(j, g_o, g_w, o, w);
      } else {
#pragma unroll
        for (int q = 0; q < 9; ++q) o[q] = __shfl(g_o[q], src, 64);
#pragma unroll
        for (int q = 0; q < 16; ++q) w[q] = __shfl(g_w[q], src, 64);
      }
      if (bb + j * PPW >= b_end) break;     // wave-uniform
      // The nine taps factor over the block: the three taps of a row class (ya: taps 0-2, exact row: 3-5, yb: 6-8)
      // read the same cell rows, a pixel's corner weights are (row weight) x (column weight), and the column
      // weights do not depend on py nor the row weights on px.  So per cell row: column-mix the five cells for
      // px = 0, 1 and fold the three depthwise weights (7 fma per component and px); then row-mix the two cell
      // rows into the four accumulators (2 fma each).  86 fma per component and block instead of 148
      // (+ 64 scalar weight products) when every tap of every pixel is mixed on its own.
      float4 acc[2][2];     // [py][px]
      auto row_taps = [&](int ro, int K0, float4 (&U)[2]) {
        const int oa = ro + o[5], ob = ro + o[6];
        const float4 va0 = CDN_RD(oa), va1 = CDN_RD(oa + kCell);
        const float4 vc = CDN_RD(ro + o[7]);
        const float4 vb0 = CDN_RD(ob), vb1 = CDN_RD(ob + kCell);
        const float4 t = make_float4(wk[K0 + 1][0] * vc.x, wk[K0 + 1][1] * vc.y, wk[K0 + 1][2] * vc.z,
                                     wk[K0 + 1][3] * vc.w);
#pragma unroll
        for (int px = 0; px < 2; ++px) {
          const float a0 = w[8 + 2 * px], a1 = w[8 + 2 * px + 1], b0 = w[12 + 2 * px], b1 = w[12 + 2 * px + 1];
          float4 ua, ub;
          ua.x = fmaf(a1, va1.x, a0 * va0.x); ua.y = fmaf(a1, va1.y, a0 * va0.y);
          ua.z = fmaf(a1, va1.z, a0 * va0.z); ua.w = fmaf(a1, va1.w, a0 * va0.w);
          ub.x = fmaf(b1, vb1.x, b0 * vb0.x); ub.y = fmaf(b1, vb1.y, b0 * vb0.y);
          ub.z = fmaf(b1, vb1.z, b0 * vb0.z); ub.w = fmaf(b1, vb1.w, b0 * vb0.w);
          U[px].x = fmaf(wk[K0][0], ua.x, fmaf(wk[K0 + 2][0], ub.x, t.x));
          U[px].y = fmaf(wk[K0][1], ua.y, fmaf(wk[K0 + 2][1], ub.y, t.y));
          U[px].z = fmaf(wk[K0][2], ua.z, fmaf(wk[K0 + 2][2], ub.z, t.z));
          U[px].w = fmaf(wk[K0][3], ua.w, fmaf(wk[K0 + 2][3], ub.w, t.w));
        }
      };
      {
        float4 M[2];
        row_taps(o[4], 3, M);                      // exact row Y: the same sum for py = 0, 1
        acc[0][0] = acc[1][0] = M[0];
        acc[0][1] = acc[1][1] = M[1];
      }
#pragma unroll
      for (int cls = 0; cls < 2; ++cls) {          // ya (offsets o[0..1], weights w[0..3]), yb (o[2..3], w[4..7])
        float4 U0[2], U1[2];
        row_taps(o[2 * cls], 6 * cls, U0);
        row_taps(o[2 * cls + 1], 6 * cls, U1);
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
          for (int px = 0; px < 2; ++px) {
            const float r0 = w[4 * cls + 2 * py], r1 = w[4 * cls + 2 * py + 1];
            float4 &A = acc[py][px];
            A.x = fmaf(r0, U0[px].x, fmaf(r1, U1[px].x, A.x));
            A.y = fmaf(r0, U0[px].y, fmaf(r1, U1[px].y, A.y));
            A.z = fmaf(r0, U0[px].z, fmaf(r1, U1[px].z, A.z));
            A.w = fmaf(r0, U0[px].w, fmaf(r1, U1[px].w, A.w));
          }
      }
      if (blk < b_end) {
        const int cbase = c0 + cq * 4;
        const long e0 = ((long)n * HW + o[8]) * C + cbase;    // element index of the block's first output pixel
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
          for (int px = 0; px < 2; ++px) {
            const float4 a = acc[py][px];
            const long e = e0 + (long)(py * W + px) * C;
            float *dp = d + e;
            if (OUT8) {
              if (cbase + 3 < C)
                *reinterpret_cast<unsigned *>(reinterpret_cast<signed char *>(d) + e) = pack_code8(a, c8, bad);
            } else if (vec_store && cbase + 3 < C) {
              *reinterpret_cast<float4 *>(dp) = a;
              track4(a, mn, mn2, mx, mx2);
            } else {
              const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (cbase + e < C) {
                  dp[e] = av[e];
                  mn = fminf(mn, av[e]);
                  mx = fmaxf(mx, av[e]);
                  has_nan |= (av[e] != av[e]);
                }
            }
          }
      }
    }
  }
#undef CDN_RD
  if (OUT8) {
    if (bad) atomicOr(oflow, 1u);
    return;
  }
  mn = fminf(mn, mn2);
  mx = fmaxf(mx, mx2);
  CDN_STAMP_WAVE();
  CDN_STAMP(3);
  if (qu.tracks())
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x,
                             gridDim.x * gridDim.y, qu, red);
  CDN_STAMP(4);
}

// ------------------------------------------------------------------------------------------
// Final materialisation for the consumer outside the fused path (the detection heads):
// out[n][c][2h+dy][2w+dx] = fq(r[n][h*W+w][c])   (nearest x2, NCHW, optional fake-quant).
// One workgroup = (n, one stored row h): reads W*C contiguous floats, transposes through LDS,
// writes 2 output rows per channel.  up == 0 writes the same resolution (plain NHWC -> NCHW).
// ------------------------------------------------------------------------------------------
template <bool RQ>
__global__ void __launch_bounds__(256)
unpack_kernel(const float *__restrict__ r, const unsigned *__restrict__ rq, float *__restrict__ out,
              int C, int H, int W, int up) {
  extern __shared__ float tile[];  // [W][C+1]
  const int n = blockIdx.y, h = blockIdx.x;
  const int ld = C + 1;
  float qs = 1.f, qz = 0.f, qr_ = 1.f;
  if (RQ) {
    qs = reinterpret_cast<const float *>(rq)[2];
    qr_ = __fdiv_rn(1.0f, qs);   // Markstein division in fake_quant_r
    qz = reinterpret_cast<const float *>(rq)[3];
  }
  const float *rp = r + ((long)n * H + h) * W * C;
  if ((C & 3) == 0) {
    for (int q = threadIdx.x; q < W * C / 4; q += 256) {
      const int px = (q * 4) / C, c = q * 4 - px * C;
      float4 v = *reinterpret_cast<const float4 *>(rp + (long)q * 4);
      if (RQ) {
        v.x = cdn::fake_quant_r(v.x, qs, qz, qr_);
        v.y = cdn::fake_quant_r(v.y, qs, qz, qr_);
        v.z = cdn::fake_quant_r(v.z, qs, qz, qr_);
        v.w = cdn::fake_quant_r(v.w, qs, qz, qr_);
      }
      float *tp = tile + px * ld + c;
      tp[0] = v.x; tp[1] = v.y; tp[2] = v.z; tp[3] = v.w;
    }
  } else {
    for (int q = threadIdx.x; q < W * C; q += 256) {
      const int px = q / C, c = q - px * C;
      float v = rp[q];
      if (RQ) v = cdn::fake_quant_r(v, qs, qz, qr_);
      tile[px * ld + c] = v;
    }
  }
  __syncthreads();
  const int f = 1 << up;
  const int Wo = W * f, Ho = H * f;
  if ((Wo & 3) == 0) {   // 16-byte stores: 4 consecutive output columns per thread
    const int wq = Wo >> 2, per_c = f * wq;
    for (int q = threadIdx.x; q < C * per_c; q += 256) {
      const int c = q / per_c, rem = q - c * per_c;
      const int dy = rem / wq, xo = (rem - dy * wq) * 4;
      float4 v;
      v.x = tile[((xo + 0) >> up) * ld + c];
      v.y = tile[((xo + 1) >> up) * ld + c];
      v.z = tile[((xo + 2) >> up) * ld + c];
      v.w = tile[((xo + 3) >> up) * ld + c];
      *reinterpret_cast<float4 *>(out + (((long)n * C + c) * Ho + h * f + dy) * Wo + xo) = v;
    }
  } else {
    const int per_c = f * Wo;
    for (int q = threadIdx.x; q < C * per_c; q += 256) {
      const int c = q / per_c, rem = q - c * per_c;
      const int dy = rem / Wo, xo = rem - dy * Wo;
      out[(((long)n * C + c) * Ho + h * f + dy) * Wo + xo] = tile[(xo >> up) * ld + c];
    }
  }
}

using cdn::kMaxGrid;

// dynamic LDS of dw2_kernel / dw2u_kernel: the leading zero cell (dw2u), (Hl+1) x (Wl+1) cells of CCH floats, the
// chunk's depthwise weights, the scale plane, reduction scratch
static size_t dw2_lds_bytes(int Hl, int Wl, int CCH) {
  return ((size_t)CCH + (size_t)(Hl + 1) * (Wl + 1) * CCH + (size_t)CCH * 9 + (size_t)Hl * Wl +
          2 * kDw2MaxThreads / 64 + 4) * sizeof(float);
}

// gather schedule for an NCHW input (`gmode`, a PER-CALL argument: bits 8-9 of the stage entry points' layout
// argument, CDN_X_GATHER_* in codenet_dcn.h; the library keeps no process-wide setting): 0 = automatic (persistent
// LDS-DMA kernel where it applies), 1 = always the per-item kernels (dw2_kernel), 2 = persistent wherever its shape
// conditions hold (also on small grids)

static size_t dw0p_lds_bytes(int H, int W) {
  return ((size_t)64 + (size_t)(H + 1) * (W + 1) * 64 + (size_t)64 * H * W + 2 * 64 * 9 + 2 * (size_t)H * W +
          2 * 16 + 4) * sizeof(float);
}
// shape conditions of dw0p_kernel (see there)
static bool dw0p_applies(int C, int H, int W) {      // C: the row length of d (a multiple of 64 >= the channels of x)
  const int HW = H * W;
  return (W & 3) == 0 && (HW & 63) == 0 && (HW & (HW - 1)) == 0 && (C & 63) == 0 &&
         dw0p_lds_bytes(H, W) <= 160 * 1024;
}
template <bool OUT8>
static int launch_dw0p(const float *x, const float *s_raw, const unsigned *sq, const float *wd, float *d,
                       unsigned *oflow, cdn::QUpdate qu, int N, int C, int H, int W, hipStream_t st, int Cx = 0) {
  if (Cx == 0) Cx = C;
  const int nitems = N * (C / 64);
  const int grid = std::min(nitems, cdn::kCUs);
  const size_t lds = dw0p_lds_bytes(H, W);
#define CDN_GOP(SQ_)                                                                                      \
  {                                                                                                       \
    auto kern = dw0p_kernel<SQ_, OUT8>;                                                                   \
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);  \
    kern<<<grid, 1024, lds, st>>>(x, s_raw, sq, wd, d, oflow, qu, C, H, W, nitems, Cx);                   \
  }
  if (sq) CDN_GOP(true)
  else CDN_GOP(false)
#undef CDN_GOP
  return cdn::check_launch("codenet fused dw (persistent)");
}

// ------------------------------------------------------------------------------------------
// dwg: the gather + depthwise for stored planes that do NOT fit LDS even in 8-channel chunks (inputs above
// ~1100 px; round 4, VERDICT r3 missing #5): no staging, the four corners of every tap are read from global
// memory / L2 with bounds tests -- dw_kernel<false> of the module path (codenet_stage.hip) in the fused
// schedule's layout: channels-last d, x NCHW or channels-last (optionally stored at half resolution and
// fake-quantised while loading), s fake-quantised while loading, range epilogue.  A size fallback: one lane per
// (pixel, channel quad), the per-channel expressions of dw_kernel in the same order.
// ------------------------------------------------------------------------------------------
template <bool NHWC_IN, bool XQ, bool SQ>
__global__ void __launch_bounds__(256)
dwg_kernel(const float *__restrict__ x, const unsigned *__restrict__ xq, const float *__restrict__ s_raw,
           const unsigned *__restrict__ sq, const float *__restrict__ wd, float *__restrict__ d,
           cdn::QUpdate qu, int C, int H, int W, int up, long total) {
  __shared__ float red[16];
  const int Hl = H >> up, Wl = W >> up, HWl = Hl * Wl, HW = H * W, CQ = (C + 3) >> 2;
  float xs = 1.f, xz = 0.f, xr_ = 1.f, ss = 1.f, sz = 0.f;
  if (XQ) {
    xs = reinterpret_cast<const float *>(xq)[2];
    xz = reinterpret_cast<const float *>(xq)[3];
    xr_ = __fdiv_rn(1.0f, xs);
  }
  if (SQ) {
    ss = reinterpret_cast<const float *>(sq)[2];
    sz = reinterpret_cast<const float *>(sq)[3];
  }
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
    const int cq = (int)(q % CQ);
    const long pn = q / CQ;
    const int n = (int)(pn / HW), p = (int)(pn - (long)n * HW);
    const int h = p / W, w = p - h * W, c = cq * 4;
    const int nc = min(4, C - c);
    float sv = s_raw[(long)n * HWl + (h >> up) * Wl + (w >> up)];
    if (SQ) sv = fake_quant(sv, ss, sz);
    const float t = sv - 1.0f;
    const Axis ya = make_axis(h - 1, -t, H), yb = make_axis(h + 1, t, H);
    const Axis xa = make_axis(w - 1, -t, W), xb = make_axis(w + 1, t, W);
    Axis ym, xm;
    ym.i0 = h; ym.w0 = 1.0f; ym.w1 = 0.0f; ym.ok = true;
    xm.i0 = w; xm.w0 = 1.0f; xm.w1 = 0.0f; xm.ok = true;
    // the four channels of full-resolution cell (yy, xx): zero outside the image
    auto rd = [&](int yy, int xx) __attribute__((always_inline)) -> float4 {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const int cell = (yy >> up) * Wl + (xx >> up);
        if (NHWC_IN) {
          if (nc == 4) {
            v = *reinterpret_cast<const float4 *>(x + ((long)n * HWl + cell) * C + c);
          } else {
            const float *xp = x + ((long)n * HWl + cell) * C + c;
            v.x = xp[0];
            if (nc > 1) v.y = xp[1];
            if (nc > 2) v.z = xp[2];
          }
        } else {
          const float *xp = x + ((long)n * C + c) * HWl + cell;
          v.x = xp[0];
          if (nc > 1) v.y = xp[HWl];
          if (nc > 2) v.z = xp[2 * (long)HWl];
          if (nc > 3) v.w = xp[3 * (long)HWl];
        }
        if (XQ) {
          v.x = cdn::fake_quant_r(v.x, xs, xz, xr_);
          v.y = cdn::fake_quant_r(v.y, xs, xz, xr_);
          v.z = cdn::fake_quant_r(v.z, xs, xz, xr_);
          v.w = cdn::fake_quant_r(v.w, xs, xz, xr_);
        }
      }
      return v;
    };
    auto tap = [&](const Axis &Y, const Axis &X) __attribute__((always_inline)) -> float4 {
      const float4 v00 = rd(Y.i0, X.i0), v01 = rd(Y.i0, X.i0 + 1), v10 = rd(Y.i0 + 1, X.i0), v11 = rd(Y.i0 + 1, X.i0 + 1);
      const float w00 = Y.w0 * X.w0, w01 = Y.w0 * X.w1, w10 = Y.w1 * X.w0, w11 = Y.w1 * X.w1;
      float4 r;
      r.x = (w00 * v00.x + w01 * v01.x) + w10 * v10.x + w11 * v11.x;
      r.y = (w00 * v00.y + w01 * v01.y) + w10 * v10.y + w11 * v11.y;
      r.z = (w00 * v00.z + w01 * v01.z) + w10 * v10.z + w11 * v11.z;
      r.w = (w00 * v00.w + w01 * v01.w) + w10 * v10.w + w11 * v11.w;
      return r;
    };
    const float4 v[9] = {tap(ya, xa), tap(ya, xm), tap(ya, xb), tap(ym, xa), rd(h, w), tap(ym, xb),
                         tap(yb, xa), tap(yb, xm), tap(yb, xb)};
    float acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float *wk = wd + (long)min(c + e, C - 1) * 9;
      const float ve[9] = {(&v[0].x)[e], (&v[1].x)[e], (&v[2].x)[e], (&v[3].x)[e], (&v[4].x)[e],
                           (&v[5].x)[e], (&v[6].x)[e], (&v[7].x)[e], (&v[8].x)[e]};
      float a = wk[0] * ve[0];
#pragma unroll
      for (int k = 1; k < 9; ++k) a = fmaf(wk[k], ve[k], a);
      acc[e] = a;
    }
    float *dp = d + ((long)n * HW + p) * C + c;
    if (nc == 4 && (C & 3) == 0) {
      *reinterpret_cast<float4 *>(dp) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
      for (int e = 0; e < nc; ++e) dp[e] = acc[e];
    }
    for (int e = 0; e < nc; ++e) {
      mn = fminf(mn, acc[e]);
      mx = fmaxf(mx, acc[e]);
      has_nan |= (acc[e] != acc[e]);
    }
  }
  if (qu.tracks()) cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.x, gridDim.x, qu, red);
}

int launch_dwg(bool nhwc, const float *x, const unsigned *xq, const float *s_raw, const unsigned *sq, const float *wd,
               float *d, cdn::QUpdate qu, int N, int C, int H, int W, int up, hipStream_t st) {
  const long total = (long)N * H * W * ((C + 3) / 4);
  const unsigned blocks = (unsigned)std::min<long>(cdn::ceil_div(total, 256), kMaxGrid);
#define CDN_GOG(NH, XQ_, SQ_) dwg_kernel<NH, XQ_, SQ_><<<blocks, 256, 0, st>>>(x, xq, s_raw, sq, wd, d, qu, C, H, W, up, total)
  const bool XQ = xq != nullptr, SQ = sq != nullptr;
  if (nhwc) {
    if (XQ && SQ) CDN_GOG(true, true, true);
    else if (XQ) CDN_GOG(true, true, false);
    else if (SQ) CDN_GOG(true, false, true);
    else CDN_GOG(true, false, false);
  } else {
    if (SQ) CDN_GOG(false, false, true);
    else CDN_GOG(false, false, false);
  }
#undef CDN_GOG
  return cdn::check_launch("codenet fused dw (global gather)");
}

// ---- the launch of the LDS-resident gather, decided once for both schedules -------------------------------------
// nhwc / up / xq_given: how x is stored; gmode: the per-call schedule choice above; ldd: the row length of d when the
// caller pads it (> C), else anything <= C
struct GatherPlan {
  int cch;            // channels per workgroup: the LDS-fit chunk (stage_channel_chunk), then thinned; 0: the stored
                      // plane does not fit LDS even in 8-channel chunks (nothing else is set)
  bool grid_ok;       // at most kMaxGrid workgroups (nothing below is set otherwise)
  bool persistent;    // dw0p_kernel over whole 64-channel items instead of the per-item kernels
  int threads;        // workgroup of dw2_kernel (dw2u_kernel always runs 512 threads)
  size_t lds;
  dim3 grid;
};
GatherPlan plan_gather(int64_t N, int64_t C, int H, int W, int up, bool nhwc, int gmode, bool xq_given, int64_t ldd) {
  GatherPlan p{};
  const int Hl = H >> up, Wl = W >> up;
  p.cch = (Hl <= 4096 && Wl <= 4096) ? cdn::stage_channel_chunk(Hl, Wl) : 0;
  if (p.cch == 0) return p;
  p.cch = cdn::thin_channel_chunk(p.cch, C, N);
  const int64_t nwg = cdn::ceil_div(C, p.cch) * N;
  p.grid_ok = nwg <= kMaxGrid;
  if (!p.grid_ok) return p;
  p.grid = dim3((unsigned)cdn::ceil_div(C, p.cch), (unsigned)N);
  p.lds = dw2_lds_bytes(Hl, Wl, p.cch);
  // d with rows padded to a multiple of 64 channels (stage_pads_d decides; a ragged channel count, CoDeNet2x); NCHW
  // input at output resolution (stage 0): the persistent LDS-DMA form once every CU gets >= 2 items to pipeline
  p.persistent = ldd > C || (p.cch == 64 && !nhwc && up == 0 && !xq_given && gmode != 1 && dw0p_applies((int)C, H, W) &&
                             (gmode == 2 || nwg >= 2L * cdn::kCUs));
  // two 512-thread workgroups per CU when LDS allows and the grid is large enough to fill them
  // (staging of one overlaps compute of the other); otherwise one 1024-thread workgroup per CU.
  // (tried and removed: two 256-thread workgroups per CU at up to 256 VGPRs with all 25 reads of a step in flight,
  // 62 us vs 56 us at stage 0; a persistent, double-buffered form -- next item's global loads in flight during
  // the gather -- 66 us: at 2 waves/SIMD the per-step LDS latency chain is exposed.  DESIGN.md section 4.1)
  p.threads = (p.lds * 2 <= 160 * 1024 && nwg >= 2L * cdn::kCUs) ? 512 : 1024;
  return p;
}

// one per-item gather launch of the plan: KERN is a dw2_kernel / dw2u_kernel instantiation, the trailing arguments its own
#define CDN_GATHER(KERN, THREADS, ...)                                                                       \
  {                                                                                                          \
    auto kern = KERN;                                                                                        \
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gp.lds);  \
    kern<<<gp.grid, THREADS, gp.lds, st>>>(__VA_ARGS__);                                                     \
  }

// the per-item kernels of the running-range schedule (fp32 d, range epilogue)
template <int CCH>
int launch_dw2(const GatherPlan &gp, bool nhwc, const float *x, const unsigned *xq, const float *s_raw,
               const unsigned *sq, const float *wd, float *d, cdn::QUpdate qu, int C, int H, int W, int up,
               hipStream_t st,
               cdn::ScaleFromSums si = cdn::ScaleFromSums{nullptr, nullptr, nullptr, 0.f, 0.f, nullptr, 0}) {
#define CDN_GO(NH, XQ_, SQ_) \
  CDN_GATHER((dw2_kernel<CCH, NH, XQ_, SQ_, kDw2MaxThreads>), gp.threads, x, xq, s_raw, sq, wd, d, nullptr, qu, C, H, W, up)
#define CDN_GOU(XQ_, SQ_) CDN_GATHER((dw2u_kernel<CCH, XQ_, SQ_>), 512, x, xq, s_raw, sq, wd, d, nullptr, qu, C, H, W, si)
  const bool XQ = xq != nullptr, SQ = sq != nullptr;
  if (nhwc && up == 1) {   // 2x2-block kernel for up-sampled inputs
    if (XQ && SQ) CDN_GOU(true, true)
    else if (XQ) CDN_GOU(true, false)
    else if (SQ) CDN_GOU(false, true)
    else CDN_GOU(false, false)
  } else if (nhwc) {
    if (XQ && SQ) CDN_GO(true, true, true)
    else if (XQ) CDN_GO(true, true, false)
    else if (SQ) CDN_GO(true, false, true)
    else CDN_GO(true, false, false)
  } else {
    if (XQ && SQ) CDN_GO(false, true, true)
    else if (XQ) CDN_GO(false, true, false)
    else if (SQ) CDN_GO(false, false, true)
    else CDN_GO(false, false, false)
  }
#undef CDN_GOU
#undef CDN_GO
  return cdn::check_launch("codenet fused dw");
}

// the per-item kernels of the frozen-range schedule (codenet_frozen.hip): byte codes of d, and of x with x_kind 2
template <int CCH>
int launch_frozen_dw_t(const GatherPlan &gp, const float *x, int x_kind, const unsigned *xq, const float *s_raw,
                       const unsigned *sq, const float *wd, float *d8, unsigned *oflow, cdn::QUpdate qu, int C, int H,
                       int W, int up, hipStream_t st, cdn::ScaleFromSums si) {
#define CDN_FGO(KERN, THREADS, LAST) CDN_GATHER(KERN, THREADS, x, xq, s_raw, sq, wd, d8, oflow, qu, C, H, W, LAST)
  if (x_kind != 0 && up == 1) {
    if (x_kind == 2) CDN_FGO((dw2u_kernel<CCH, true, true, true, true>), 512, si)
    else CDN_FGO((dw2u_kernel<CCH, true, true, false, true>), 512, si)
  } else if (x_kind == 2) {
    CDN_FGO((dw2_kernel<CCH, true, true, true, kDw2MaxThreads, true, true>), gp.threads, up)
  } else if (x_kind == 1) {
    CDN_FGO((dw2_kernel<CCH, true, true, true, kDw2MaxThreads, false, true>), gp.threads, up)
  } else {
    CDN_FGO((dw2_kernel<CCH, false, false, true, kDw2MaxThreads, false, true>), gp.threads, up)
  }
#undef CDN_FGO
  return cdn::check_launch("codenet frozen gather");
}
#undef CDN_GATHER

// ---- the scale launch both schedules share.  x_form: 0 = fp32 final values, 1 = fp32 pre-quantisation values + their
// quantiser state xq (channels-last only), 2 = byte codes of the quantiser xq (channels-last only).  One kernel choice, so
// that the frozen schedule forms every fp32 sum in the order of the running one (bit-identical s_raw and d codes).  The
// caller names the launch in its own cdn::check_launch.
void launch_scale(const float *x, bool nhwc, int x_form, const unsigned *xq, const float *w_scale, const float *b_scale,
                  float *s_raw, int64_t N, int64_t C, int64_t HWl, float lo, float hi, const cdn::QUpdate &qu,
                  hipStream_t st) {
  const long npix = (long)(N * HWl);
  if (!nhwc) {
    dim3 grid((unsigned)cdn::ceil_div(HWl, 64), (unsigned)N);
    scale_nchw_kernel<<<grid, kScaleWaves * 64, 0, st>>>(x, w_scale, b_scale, s_raw, qu, (int)C, (int)HWl, lo, hi);
  } else if (C <= 256 && npix >= 32768 && cdn::ceil_div(npix, kScaleTilePix) <= kMaxGrid) {
    // tiled kernel for large planes (measured: 18 vs 22 us at 65536 pixels x 128 channels; the
    // wave-per-pixel kernel is ahead at 16384 x 256: 13.7 vs 15.0 us)
    const int blocks = (int)cdn::ceil_div(npix, kScaleTilePix);
    const int CQ = (int)C >> 2, LD = ((CQ + 31) & ~31) + 4;
    const size_t lds = ((size_t)kScaleTilePix * LD + 16) * sizeof(float);
    auto kern = x_form == 2 ? scale_nhwc_tile_kernel<true, true>
                : x_form == 1 ? scale_nhwc_tile_kernel<true> : scale_nhwc_tile_kernel<false>;
    kern<<<blocks, 256, lds, st>>>(x, x_form ? xq : nullptr, w_scale, b_scale, s_raw, qu, (int)C, npix, lo, hi);
  } else {
    const int blocks = (int)std::min<long>(cdn::ceil_div(npix, 4), (long)cdn::kCUs * 8);
    auto kern = x_form == 2 ? scale_nhwc_kernel<true, true> : x_form == 1 ? scale_nhwc_kernel<true> : scale_nhwc_kernel<false>;
    kern<<<blocks, 256, 0, st>>>(x, x_form ? xq : nullptr, w_scale, b_scale, s_raw, qu, (int)C, npix, lo, hi);
  }
}

}  // namespace

// ---- launchers of the frozen-range schedule (codenet_frozen.hip): the same scale / gather kernels with byte
// codes on one or both sides.  x_kind: 0 = NCHW fp32 final values, 1 = channels-last fp32 pre-quantisation
// values + their quantiser state xq, 2 = channels-last byte codes of the quantiser xq.
int cdn::launch_frozen_scale(const void *x, int x_kind, const unsigned *xq, const float *w_scale,
                             const float *b_scale, float *s_raw, int64_t N, int64_t C, int64_t HWl, float lo,
                             float hi, hipStream_t st) {
  launch_scale(static_cast<const float *>(x), x_kind != 0, x_kind, xq, w_scale, b_scale, s_raw, N, C, HWl, lo, hi,
               cdn::no_qupdate(), st);
  return cdn::check_launch("codenet frozen scale");
}

// The gather's channel chunk for THIS launch: the LDS-fit chunk (stage_channel_chunk), thinned while the grid is below one
// workgroup per CU.  cfg2 (32 images of 256 x 256) ran stage 1 on 128 and stage 2 on 64 workgroups of 64 channels -- half
// and a quarter of the GPU (in-kernel stamps, round 6); with chunks of 32 / 16: gather 13.0 -> 11.4 and 21.6 -> 12.7 us,
// step 0.0937 -> 0.0835 ms; CoDeNet2x at 32 images per GPU 0.2154 -> 0.2026 ms.  Thinner than one workgroup per CU, or
// chunks of 8, lose again (0.0866 / 0.0909).  The gather is per channel: the chunking changes no value.
#ifndef CDN_THIN_CHUNK_MIN
#define CDN_THIN_CHUNK_MIN 16      // (64 and 32 channels fetch the tap record with DPP, 16 and 8 with ds_bpermute)
#endif
#ifndef CDN_THIN_CHUNK_FILL
#define CDN_THIN_CHUNK_FILL 1      // workgroups per CU the thinning aims at (A/B: 2 loses at every shape tried)
#endif
int cdn::thin_channel_chunk(int cch, int64_t C, int64_t N) {
#ifndef CDN_NO_THIN_CHUNKS
  while (cch > CDN_THIN_CHUNK_MIN && cdn::ceil_div(C, (int64_t)cch) * N < (int64_t)CDN_THIN_CHUNK_FILL * cdn::kCUs) cch >>= 1;
#endif
  return cch;
}

int cdn::launch_frozen_dw(const void *x, int x_kind, const unsigned *xq, const float *s_raw, const unsigned *sq,
                          const float *wd, signed char *d8, unsigned *dstate, unsigned *oflow, int N, int C, int H,
                          int W, int up, hipStream_t st, cdn::ScaleFromSums si, int gmode) {
  if (si.sums && !(x_kind != 0 && up == 1))
    return cdn::fail(CDN_ERR_UNSUPPORTED, "scale sums are consumed by the up-sampled channels-last gather only");
  const GatherPlan gp = plan_gather(N, C, H, W, up, x_kind != 0, gmode, xq != nullptr, 0);
  if (gp.cch == 0) return cdn::fail(CDN_ERR_UNSUPPORTED, "stored plane too large for the LDS-resident gather");
  if (!gp.grid_ok) return cdn::fail(CDN_ERR_UNSUPPORTED, "too many workgroups");
  const float *xf = static_cast<const float *>(x);
  float *df = reinterpret_cast<float *>(d8);
  const cdn::QUpdate qu{nullptr, nullptr, dstate, nullptr, 0.f, 0.f, 8, 0};      // (the kernels read the frozen state of d)
  if (gp.persistent) return launch_dw0p<true>(xf, s_raw, sq, wd, df, oflow, qu, N, C, H, W, st);
  auto fn = gp.cch == 64 ? launch_frozen_dw_t<64> : gp.cch == 32 ? launch_frozen_dw_t<32>
            : gp.cch == 16 ? launch_frozen_dw_t<16> : launch_frozen_dw_t<8>;
  return fn(gp, xf, x_kind, xq, s_raw, sq, wd, df, oflow, qu, C, H, W, up, st, si);
}

// --act-percentile (CDN_X_ACT_PERCENTILE): the radix select's histograms + the two order statistics it returns
constexpr int64_t kPctBytes = 32 * 1024;

// Range commit of a percentile QuantAct: the producer (launched with running = 0) left the batch's TRUE extremes in
// state words [4], [5]; the range follows the order statistics `pct` (quant_modules.py:203-219), the code-width flag
// the extremes.
__global__ void quantact_commit_percentile_kernel(cdn::QUpdate u, const float *__restrict__ pct) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const float *sf = reinterpret_cast<const float *>(u.state);
    cdn::quantact_update_device(u, pct[0], pct[1], true, false, 0.f, 0.f, true, sf[4], sf[5]);
  }
}

extern "C" int cdn_quantact_commit_range(float *x_min, float *x_max, void *state, const float *range, int bits,
                                         double momentum, int running, void *stream) {
  CDN_REQUIRE(x_min && x_max && state && range, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(bits >= 2 && bits <= 16, CDN_ERR_ARG, "bits out of range");
  const cdn::QUpdate u = cdn::make_qupdate(x_min, x_max, state, nullptr, bits, momentum, running);
  quantact_commit_percentile_kernel<<<1, 64, 0, cdn::as_stream(stream)>>>(u, range);
  return cdn::check_launch("quantact commit range");
}

// Workspace of the fused stage, every region rounded up to 256 bytes: s_raw [N*HWl] fp32, d [N*H*W*Cd] fp32 (rows of d
// may be padded to whole 64-channel chunks), the percentile scratch, 3 reserved regions (ABI 1: nothing reads or writes
// them) and 3 sets of arrival counters -- these in the LAST bytes of the workspace the caller gave (it zeroes them once).
struct StageWorkspace {
  int64_t s_raw, d, pct;      // byte offsets
  int64_t arrive[3];          // byte offsets of the counters of s, d, r: counted back from workspace_bytes
  int64_t bytes;              // the size cdn_codenet_stage_workspace_bytes reports
};
static StageWorkspace stage_workspace(int64_t N, int64_t C, int64_t H, int64_t W, int x_up, size_t workspace_bytes) {
  auto r = [](int64_t b) { return (b + 255) / 256 * 256; };
  const int64_t HWl = (H >> x_up) * (W >> x_up), Cd = (C + 63) / 64 * 64, arr = r(cdn::kArriveWords * 4);
  StageWorkspace w;
  w.s_raw = 0;
  w.d = r(N * HWl * 4);
  w.pct = w.d + r(N * H * W * Cd * 4);
  w.bytes = w.pct + r(kPctBytes) + 3 * r((int64_t)cdn::kReservedRegionBytes) + 3 * arr;
  for (int i = 0; i < 3; ++i) w.arrive[i] = (int64_t)(workspace_bytes / 256 * 256) - (3 - i) * arr;
  return w;
}

extern "C" size_t cdn_codenet_stage_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W,
                                                    int x_up) {
  return (size_t)stage_workspace(N, C, H, W, x_up, 0).bytes;
}

// LDS budget of the gather kernel decides the channel chunk: 64 or 32 channels x the whole stored plane at the
// BASELINE resolutions (planes up to 34 x 34, inputs up to 544 px); larger planes keep the whole-plane form -- the tap
// offsets reach +-8 pixels, so a spatial tile would need a +-9-cell halo and re-read 2-2.6x the bytes -- with thinner
// chunks: 16 channels (4 lanes per pixel, planes up to ~49 x 49) or 8 (2 lanes per pixel, up to ~69 x 69, inputs up to
// ~1100 px).  Thin chunks fetch the tap record with ds_bpermute instead of DPP and read 64- / 32-byte pieces of every
// cell row (bank conflicts, partial lines): a size fallback, not a tuned path.  0: the plane does not fit.
int cdn::stage_channel_chunk(int Hl, int Wl) {
  const size_t cells = (size_t)(Hl + 1) * (Wl + 1) + 1;   // + the zero row and zero column, + the leading zero cell
  const long lds_max = 160 * 1024 - 64 * 9 * 4 - 256 - (long)Hl * Wl * 4;   // scale plane, weights, scratch
  if (lds_max <= 0) return 0;
  for (int cch = 64; cch >= 8; cch >>= 1)
    if (cells * cch * 4 <= (size_t)lds_max) return cch;
  return 0;
}

// shape conditions every form of the fused stage shares (stage_fused_forward_impl reports them one by one)
static bool stage_shape_ok(int64_t N, int64_t C, int64_t H, int64_t W, int x_nhwc, int x_up) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || (x_up != 0 && x_up != 1)) return false;
  if (x_up && ((H & 1) || (W & 1))) return false;
  if (x_nhwc && (C & 3)) return false;
  if (x_up && !x_nhwc) return false;
  if (N > 65535 || N * C * H * W >= (1ll << 31)) return false;
  return (H >> x_up) <= 4096 && (W >> x_up) <= 4096;
}

extern "C" int cdn_codenet_stage_supported(int64_t N, int64_t C, int64_t H, int64_t W, int x_nhwc, int x_up) {
  if (!stage_shape_ok(N, C, H, W, x_nhwc, x_up)) return 0;
  const int cch = cdn::stage_channel_chunk((int)(H >> x_up), (int)(W >> x_up));
  return cch != 0 && cdn::ceil_div(C, cch) * N <= kMaxGrid;
}

// cdn_codenet_stage_fused_forward's own limits: as above, plus the global-memory gather for stored planes that do not
// fit LDS (round 4) -- any plane the 32-bit element counts allow.
extern "C" int cdn_codenet_stage_fused_supported(int64_t N, int64_t C, int64_t H, int64_t W, int x_nhwc, int x_up) {
  if (cdn_codenet_stage_supported(N, C, H, W, x_nhwc, x_up)) return 1;
  if (!stage_shape_ok(N, C, H, W, x_nhwc, x_up)) return 0;
  return cdn::stage_channel_chunk((int)(H >> x_up), (int)(W >> x_up)) == 0;      // (too many chunk workgroups: no)
}

// Rows of d padded to whole 64-channel chunks?  (NCHW input with a ragged channel count feeding the int8 pointwise.)
static bool stage_pads_d(int64_t N, int64_t C, int64_t H, int64_t W, int x_nhwc, int x_up, int gmode, bool int8_pw) {
  const int64_t Cd = (C + 63) / 64 * 64;
  return !x_nhwc && x_up == 0 && Cd != C && gmode != 1 && int8_pw && cdn::stage_channel_chunk((int)H, (int)W) == 64 &&
         dw0p_applies((int)Cd, (int)H, (int)W) && N * Cd * H * W < (1ll << 31);
}

// Diagnostics / tests: where cdn_codenet_stage_fused_forward leaves its two intermediates in the workspace -- the
// clamped scale plane s (pre-quantisation, [N][stored pixels]) at byte offset 0 and the gather output d
// (pre-quantisation, channels-last rows of *d_row_floats floats, of which the first C are the channels) at
// *d_offset_bytes.  int8_pointwise: the call passes the integer form of the pointwise weights and a d quantiser
// (W4A8 without --act-percentile).  Both stay valid until the next call that uses the workspace.
extern "C" int cdn_codenet_stage_fused_intermediates(int64_t N, int64_t C, int64_t H, int64_t W, int x_nhwc, int x_up,
                                                     int int8_pointwise, int64_t *d_offset_bytes,
                                                     int64_t *d_row_floats) {
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && d_offset_bytes && d_row_floats, CDN_ERR_ARG, "bad argument");
  const int gmode = (x_nhwc & CDN_X_GATHER_MASK) >> 8;
  *d_offset_bytes = stage_workspace(N, C, H, W, x_up, 0).d;
  *d_row_floats = stage_pads_d(N, C, H, W, x_nhwc & 1, x_up, gmode, int8_pointwise != 0 && !(x_nhwc & CDN_X_ACT_PERCENTILE))
                      ? (C + 63) / 64 * 64 : C;
  return CDN_OK;
}

// parts_in / n_parts_in: the scale prediction of THIS stage as the previous stage's partial sums (no scale launch);
// next_w_scale / parts_out: leave the next stage's partial sums (cdn_codenet_stage_fused_forward_chain)
static int stage_fused_forward_impl(
    const float *x, int x_nhwc, int x_up, const void *x_qstate, int64_t N, int64_t C, int64_t Co,
    int64_t H, int64_t W, const float *w_scale, const float *b_scale, float lo, float hi,
    const float *w_dw, const float *w_pw, const signed char *w_pw_codes, const float *w_pw_scale,
    const int *w_pw_colsum, const float *bias_pw, const float *ep_scale, const float *ep_shift,
    int relu, float *s_min, float *s_max, void *s_state, float *d_min,
    float *d_max, void *d_state, float *r_min, float *r_max, void *r_state, int bits,
    double momentum, int running, void *workspace, size_t workspace_bytes, float *r_out,
    void *stream, const float *parts_in, int n_parts_in, const float *next_w_scale, float *parts_out) {
  CDN_REQUIRE(x && w_scale && w_dw && w_pw && r_out && workspace, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && Co > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE((x_nhwc & ~(1 | CDN_X_GATHER_MASK | CDN_X_ACT_PERCENTILE | CDN_X_WCODES_KB | CDN_X_DEFER_RANGE |
                          CDN_X_PHASE_MASK | CDN_W_CODES_8BIT)) == 0 &&
                  ((x_nhwc & CDN_X_GATHER_MASK) >> 8) <= 2, CDN_ERR_ARG,
              "x_nhwc: 0 / 1, optionally | CDN_X_GATHER_PER_ITEM or CDN_X_GATHER_PERSISTENT, | CDN_X_ACT_PERCENTILE, "
              "| CDN_X_WCODES_KB, | CDN_X_DEFER_RANGE, | CDN_X_PHASE_*, | CDN_W_CODES_8BIT");
  const int w_bits = (x_nhwc & CDN_W_CODES_8BIT) ? 8 : 4;      // width of w_pw_codes the caller vouches for
  CDN_REQUIRE(w_bits == 4 || w_pw_codes, CDN_ERR_ARG, "CDN_W_CODES_8BIT without w_pw_codes");
  // split call (multi-process global ranges): which steps run, and whether the producers only measure
  const int phases = (x_nhwc & CDN_X_PHASE_MASK) ? (x_nhwc & CDN_X_PHASE_MASK) : CDN_X_PHASE_MASK;
  const bool defer = (x_nhwc & CDN_X_DEFER_RANGE) != 0;
  CDN_REQUIRE(!defer || (running != 0 && s_state && d_state && r_state && !(x_nhwc & CDN_X_ACT_PERCENTILE)), CDN_ERR_ARG,
              "CDN_X_DEFER_RANGE needs running != 0 and the three QuantActs, and excludes CDN_X_ACT_PERCENTILE");
  const int gmode = (x_nhwc & CDN_X_GATHER_MASK) >> 8;      // per-call schedule choice (tests); no library state
  // the k-blocked copy of the weight codes behind the row-major ones (the streaming int8 pointwise kernel)
  CDN_REQUIRE(!(x_nhwc & CDN_X_WCODES_KB) || (w_pw_codes && cdn_codenet_wcodes_kb_columns(C, Co) != 0), CDN_ERR_ARG,
              "CDN_X_WCODES_KB: no k-blocked form for C = %lld, Co = %lld (cdn_codenet_wcodes_kb_columns)",
              (long long)C, (long long)Co);
  const signed char *w_kb = (x_nhwc & CDN_X_WCODES_KB) ? w_pw_codes + cdn_codenet_wcodes_kb_offset(C, Co) : nullptr;
  // --act-percentile: the three QuantActs follow the 0.1 % / 99.9 % order statistics of their input instead of its
  // extremes (only while the ranges are tracked)
  const bool pct = (x_nhwc & CDN_X_ACT_PERCENTILE) != 0 && running != 0;
  x_nhwc &= 1;
  CDN_REQUIRE(!pct || (s_state && d_state && r_state), CDN_ERR_ARG, "CDN_X_ACT_PERCENTILE needs the three QuantActs");
  CDN_REQUIRE(x_up == 0 || x_up == 1, CDN_ERR_ARG, "x_up must be 0 or 1");
  CDN_REQUIRE(!x_up || ((H & 1) == 0 && (W & 1) == 0), CDN_ERR_SHAPE,
              "x_up needs even H, W (got %lld x %lld)", (long long)H, (long long)W);
  CDN_REQUIRE((ep_scale == nullptr) == (ep_shift == nullptr), CDN_ERR_ARG,
              "ep_scale / ep_shift must both be set or both be NULL");
  CDN_REQUIRE((s_state == nullptr) == (s_min == nullptr) && (s_state == nullptr) == (s_max == nullptr) &&
                  (d_state == nullptr) == (d_min == nullptr) && (d_state == nullptr) == (d_max == nullptr) &&
                  (r_state == nullptr) == (r_min == nullptr) && (r_state == nullptr) == (r_max == nullptr),
              CDN_ERR_ARG, "each QuantAct needs x_min, x_max and state together");
  CDN_REQUIRE(!x_nhwc || (C & 3) == 0, CDN_ERR_UNSUPPORTED,
              "channels-last input needs C %% 4 == 0 (got %lld)", (long long)C);
  CDN_REQUIRE(x_up == 0 || x_nhwc, CDN_ERR_UNSUPPORTED, "an up-sampled input must be channels-last");
  CDN_REQUIRE(N <= 65535 && N * C * H * W < (1ll << 31) && N * Co * H * W < (1ll << 31),
              CDN_ERR_UNSUPPORTED, "shape too large");
  CDN_REQUIRE(workspace_bytes >= cdn_codenet_stage_workspace_bytes(N, C, H, W, x_up),
              CDN_ERR_WORKSPACE, "workspace too small");
  CDN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0 &&
                  (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(r_out) & 15) == 0,
              CDN_ERR_ARG, "x / r_out must be 16-byte and workspace 256-byte aligned");
  hipStream_t st = cdn::as_stream(stream);
  const int64_t HWl = (H >> x_up) * (W >> x_up);
  const StageWorkspace wl = stage_workspace(N, C, H, W, x_up, workspace_bytes);
  char *wsp = static_cast<char *>(workspace);
  float *s_raw = reinterpret_cast<float *>(wsp + wl.s_raw);
  float *d = reinterpret_cast<float *>(wsp + wl.d);
  // Rows of d: C floats, or -- NCHW input with a ragged channel count feeding the int8 pointwise (CoDeNet2x stage 0,
  // C = 2153; round 4) -- padded to the next multiple of 64 so that the persistent LDS-DMA gather (whole 64-channel
  // chunks, 16-byte stores) and the int8 pointwise's 16-byte row loads apply; the pad channels duplicate channel
  // C - 1 and meet zero weight codes (see dw0p_kernel).  Same values as the unpadded schedule, bit for bit.
  const int64_t Cd = (C + 63) / 64 * 64;
  const bool pad_d = !pct && stage_pads_d(N, C, H, W, x_nhwc, x_up, gmode,
                                          w_pw_codes != nullptr && d_state != nullptr && ep_scale == nullptr &&
                                              w_pw_scale != nullptr && w_pw_colsum != nullptr);
  const int64_t ldd = pad_d ? Cd : C;
  char *pct_ws = wsp + wl.pct;
  float *pct_out = reinterpret_cast<float *>(pct_ws + kPctBytes - 256);
  auto arrive = [&](int i, const void *state) {      // the arrival counters of QuantAct i, when it is given
    return state ? reinterpret_cast<unsigned *>(wsp + wl.arrive[i]) : nullptr;
  };
  unsigned *sst = static_cast<unsigned *>(s_state), *dst = static_cast<unsigned *>(d_state);
  const unsigned *xq = static_cast<const unsigned *>(x_qstate);

  // cch == 0: the stored plane does not fit LDS even in 8-channel chunks -> the global-memory gather (dwg_kernel)
  const GatherPlan gp = plan_gather(N, C, (int)H, (int)W, x_up, x_nhwc != 0, gmode, xq != nullptr, ldd);
  CDN_REQUIRE(gp.cch != 0 || xq == nullptr || x_nhwc, CDN_ERR_UNSUPPORTED, "quant-on-load needs a channels-last input");

  // Range tracking runs inside the producing kernels (last workgroup to finish), see
  // cdn::block_minmax_finish: no separate update launches.
  // (percentile: the producers only measure -- running = 0 leaves the range alone and parks the extremes in the
  // state --, the commit follows each of them)
  const int prun = (pct || defer) ? 0 : running;
  // a producer measures its output (QUpdate::tracks) iff the QuantAct behind it is given.  d: always when given -- the
  // batch extremes also gate the int8 path
  const cdn::QUpdate qu_s = cdn::make_qupdate(s_min, s_max, s_state, arrive(0, s_state), bits, momentum, prun);
  const cdn::QUpdate qu_d = cdn::make_qupdate(d_min, d_max, d_state, arrive(1, d_state), bits, momentum, prun);
  const cdn::QUpdate qu_r = cdn::make_qupdate(r_min, r_max, r_state, arrive(2, r_state), bits, momentum, prun);
  // t holds n / rep elements, each standing for `rep` equal elements of the tensor the reference ranks (rep = 4: the
  // scale plane of an up-sampled input is computed at stored resolution; nearest x2 replicates every value four times)
  auto commit_percentile = [&](const float *t, int64_t n, int rep, const cdn::QUpdate &qu) -> int {
    // the reference's ranks: round(n * 0.1 * 0.01), round(n * 99.9 * 0.01), Python's round (half to even)
    int64_t k_lo = (int64_t)std::nearbyint(((double)n * 0.1) * 0.01);
    int64_t k_hi = (int64_t)std::nearbyint(((double)n * 99.9) * 0.01);
    CDN_REQUIRE(k_lo >= 1 && k_hi <= n, CDN_ERR_UNSUPPORTED,
                "kthvalue(): selected number k out of range (a tensor of %lld elements has no 0.1 %% order statistic)",
                (long long)n);
    k_lo = (k_lo + rep - 1) / rep;             // the k-th smallest of the replicated multiset
    k_hi = (k_hi + rep - 1) / rep;
    n /= rep;
    int rc2 = cdn_kth_values(t, n, k_lo, k_hi, pct_out, pct_out + 1, pct_ws, (size_t)(kPctBytes - 256), stream);
    if (rc2) return rc2;
    cdn::QUpdate q2 = qu;
    q2.running = running;
    quantact_commit_percentile_kernel<<<1, 64, 0, st>>>(q2, pct_out);
    return cdn::check_launch("codenet fused percentile commit");
  };
  const int ptag = (int)(H > 0xffff ? 0xffff : H);
  int rc = 0;
  // 1. scale prediction at stored resolution (+ min/max of s)
  if (parts_in) {
    CDN_REQUIRE(n_parts_in >= 1 && !s_state && !xq && x_nhwc && x_up && !pct && !defer && gp.cch != 0,
                CDN_ERR_UNSUPPORTED, "scale partial sums feed the LDS gather of an up-sampled channels-last fp32 input only");
  } else if (phases & CDN_X_PHASE_SCALE) {
    // (the running schedule's own limits of the NCHW form; scale_nchw_kernel itself runs on any grid)
    CDN_REQUIRE(x_nhwc || xq == nullptr, CDN_ERR_UNSUPPORTED, "quant-on-load needs a channels-last input");
    CDN_REQUIRE(x_nhwc || cdn::ceil_div(HWl, 64) * N <= kMaxGrid, CDN_ERR_UNSUPPORTED, "too many scale workgroups");
    {
      cdn::ProfScope ps(cdn::kProfScale, ptag, st);
      launch_scale(x, x_nhwc != 0, xq ? 1 : 0, xq, w_scale, b_scale, s_raw, N, C, HWl, lo, hi, qu_s, st);
    }
    rc = cdn::check_launch("codenet fused scale");
    if (rc) return rc;
    if (pct && (rc = commit_percentile(s_raw, N * H * W, x_up ? 4 : 1, qu_s))) return rc;
  }
  // 2. gather + depthwise (+ min/max of d)
  if (!(phases & CDN_X_PHASE_GATHER)) {
  } else if (gp.cch == 0) {
    cdn::ProfScope ps(cdn::kProfDw, ptag, st);
    rc = launch_dwg(x_nhwc != 0, x, xq, s_raw, sst, w_dw, d, qu_d, (int)N, (int)C, (int)H, (int)W, x_up, st);
  } else {
    // (few workgroups -- cfg2: 32 images of 256 x 256 -- run thinner chunks: cdn::thin_channel_chunk)
    CDN_REQUIRE(gp.grid_ok, CDN_ERR_UNSUPPORTED, "too many gather workgroups");
    cdn::ProfScope ps(cdn::kProfDw, ptag, st);
    if (gp.persistent) {      // (padded rows of d: the kernel walks ldd channels and reads the C of x)
      rc = launch_dw0p<false>(x, s_raw, sst, w_dw, d, nullptr, qu_d, (int)N, (int)ldd, (int)H, (int)W, st, (int)C);
    } else {
      auto fn = gp.cch == 64 ? launch_dw2<64> : gp.cch == 32 ? launch_dw2<32> : gp.cch == 16 ? launch_dw2<16> : launch_dw2<8>;
      rc = fn(gp, x_nhwc != 0, x, xq, s_raw, sst, w_dw, d, qu_d, (int)C, (int)H, (int)W, x_up, st,
              cdn::ScaleFromSums{nullptr, nullptr, b_scale, lo, hi, parts_in, n_parts_in});
    }
  }
  if (rc) return rc;
  if (pct && (phases & CDN_X_PHASE_GATHER) && (rc = commit_percentile(d, N * H * W * C, 1, qu_d))) return rc;
  if (!(phases & CDN_X_PHASE_POINTWISE)) return CDN_OK;
  // 3. pointwise MFMA (+ bias / affine / ReLU, min/max of the result)
  cdn::PwCall pw{};
  pw.a = d;
  pw.a_state = dst;
  pw.M = (long)(N * H * W);
  pw.C = C;
  pw.Co = Co;
  pw.w = w_pw;
  pw.w_codes = w_pw_codes;
  pw.w_scale = w_pw_scale;
  pw.w_colsum = w_pw_colsum;
  pw.bias = bias_pw;
  pw.ep_scale = ep_scale;
  pw.ep_shift = ep_shift;
  pw.relu = relu;
  pw.out = r_out;
  pw.qu = qu_r;
  pw.ptag = ptag;
  pw.st = st;
  pw.lda = pad_d ? ldd : 0;
  pw.a_padded = pad_d;
  pw.w_kb = w_kb;
  pw.w_bits = w_bits;
  pw.next_ws = next_w_scale;
  pw.sparts = parts_out;
  rc = cdn::launch_pointwise(pw);
  if (rc) return rc;
  if (pct) rc = commit_percentile(r_out, N * H * W * Co, 1, qu_r);
  return rc;
}

extern "C" int cdn_codenet_stage_fused_forward(
    const float *x, int x_nhwc, int x_up, const void *x_qstate, int64_t N, int64_t C, int64_t Co,
    int64_t H, int64_t W, const float *w_scale, const float *b_scale, float lo, float hi,
    const float *w_dw, const float *w_pw, const signed char *w_pw_codes, const float *w_pw_scale,
    const int *w_pw_colsum, const float *bias_pw, const float *ep_scale, const float *ep_shift,
    int relu, float *s_min, float *s_max, void *s_state, float *d_min,
    float *d_max, void *d_state, float *r_min, float *r_max, void *r_state, int bits,
    double momentum, int running, void *workspace, size_t workspace_bytes, float *r_out,
    void *stream) {
  return stage_fused_forward_impl(x, x_nhwc, x_up, x_qstate, N, C, Co, H, W, w_scale, b_scale, lo, hi, w_dw, w_pw,
                                  w_pw_codes, w_pw_scale, w_pw_colsum, bias_pw, ep_scale, ep_shift, relu, s_min, s_max,
                                  s_state, d_min, d_max, d_state, r_min, r_max, r_state, bits, momentum, running,
                                  workspace, workspace_bytes, r_out, stream, nullptr, 0, nullptr, nullptr);
}

// Chained fp32 stages (round 6): number of partial-sum planes the pointwise conv of a stage (N, C -> Co, H x W) leaves for
// the next stage's scale prediction -- 0 when this stage's pointwise is not the streaming f32 kernel (pws_kernel) or the
// next stage (Co channels at 2H x 2W, up-sampled channels-last input) has no LDS-resident gather.
extern "C" int cdn_codenet_stage_chain_parts(int64_t N, int64_t C, int64_t Co, int64_t H, int64_t W) {
  if (N <= 0 || C <= 0 || Co <= 0 || H <= 0 || W <= 0 || N > 65535) return 0;
  if (H > 4096 || W > 4096 || cdn::stage_channel_chunk((int)H, (int)W) == 0) return 0;      // (the next stage's stored plane)
  return cdn::pointwise_chain_parts((long)(N * H * W), C, Co);
}

extern "C" int cdn_codenet_stage_fused_forward_chain(
    const float *x, int x_nhwc, int x_up, const void *x_qstate, int64_t N, int64_t C, int64_t Co,
    int64_t H, int64_t W, const float *w_scale, const float *b_scale, float lo, float hi,
    const float *w_dw, const float *w_pw, const float *bias_pw, const float *ep_scale, const float *ep_shift,
    int relu, void *workspace, size_t workspace_bytes, float *r_out, const float *parts_in, int n_parts_in,
    const float *next_w_scale, float *parts_out, void *stream) {
  CDN_REQUIRE((next_w_scale == nullptr) == (parts_out == nullptr), CDN_ERR_ARG,
              "next_w_scale and parts_out come together");
  CDN_REQUIRE(!parts_out || cdn_codenet_stage_chain_parts(N, C, Co, H, W) != 0, CDN_ERR_UNSUPPORTED,
              "no chained form for this stage (cdn_codenet_stage_chain_parts)");
  return stage_fused_forward_impl(x, x_nhwc, x_up, x_qstate, N, C, Co, H, W, w_scale, b_scale, lo, hi, w_dw, w_pw,
                                  nullptr, nullptr, nullptr, bias_pw, ep_scale, ep_shift, relu, nullptr, nullptr,
                                  nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 8, 0.99, 0,
                                  workspace, workspace_bytes, r_out, stream, parts_in, n_parts_in, next_w_scale,
                                  parts_out);
}

extern "C" int cdn_codenet_unpack_nchw(const float *r_nhwc, const void *r_qstate, float *out_nchw,
                                       int64_t N, int64_t C, int64_t H, int64_t W, int up,
                                       void *stream) {
  CDN_REQUIRE(r_nhwc && out_nchw, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && (up == 0 || up == 1), CDN_ERR_ARG, "bad size");
  CDN_REQUIRE(N <= 65535 && H <= 65535 && (size_t)W * (C + 1) * 4 <= 150 * 1024, CDN_ERR_UNSUPPORTED,
              "row of %lld pixels x %lld channels does not fit the LDS transpose tile", (long long)W,
              (long long)C);
  hipStream_t st = cdn::as_stream(stream);
  const size_t lds = (size_t)W * (C + 1) * sizeof(float);
  if (lds > 64 * 1024) {
    (void)hipFuncSetAttribute((const void *)unpack_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void *)unpack_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  }
  dim3 grid((unsigned)H, (unsigned)N);
  cdn::ProfScope ps(cdn::kProfUnpack, (int)(H > 0xffff ? 0xffff : H), st);
  if (r_qstate)
    unpack_kernel<true><<<grid, 256, lds, st>>>(r_nhwc, static_cast<const unsigned *>(r_qstate),
                                               out_nchw, (int)C, (int)H, (int)W, up);
  else
    unpack_kernel<false><<<grid, 256, lds, st>>>(r_nhwc, nullptr, out_nchw, (int)C, (int)H, (int)W, up);
  return cdn::check_launch("codenet unpack");
}

// ---- stand-alone entry points for the layers around the hot path (detection heads) ------------
extern "C" size_t cdn_codenet_aux_workspace_bytes(void) { return cdn::aux_workspace_bytes(); }
