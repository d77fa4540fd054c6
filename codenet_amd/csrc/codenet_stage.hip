// codenet_stage.hip -- CoDeNet fast paths for gfx950 (MI355X), f32.
//
// The co-designed deformable convolution
// (lib/models/external/modules/dcn_deform_conv.py:285-330) is
//     s = Hardtanh(-7,8)(conv1x1(x; C->1)+b) ; offset = anchor*(s-1)
//     d = depthwise 3x3 deformable conv(x, offset) ; y = conv1x1(d; C->Co)
// so all C channels of a pixel share ONE scalar s: the 3x3 stencil is dilated by s.  The
// kernels here exploit that: the 18-channel offset tensor and the im2col
// column buffer of the reference (dcn_deform_conv_cuda.cpp:196-235) never exist.
//
//   scale_kernel      HBM-bound C->1 reduction, lanes along pixels (coalesced), C split over
//                     the 4 waves of a workgroup, reduced through LDS.
//   dw_kernel         bilinear gather + depthwise 3x3: whole (n,c) planes staged in LDS with a
//                     one-pixel zero border (per-corner zeroing == border reads), tap
//                     geometry computed once per pixel and reused over the staged channels.
//   pointwise_kernel  Y[n] = Wp . D[n] on v_mfma_f32_32x32x2_f32 (exact f32), LDS-tiled.
#include "cdn_common.h"

#include <cstdlib>

namespace {

// ------------------------------------------------------------------------------------------
// Tap geometry shared by forward and backward.  For row class r in {0,2} (i = 0 / i = 2):
//   pos = float(h - 1 + i) + (i-1) * t,  t = s - 1   (bit-identical to the reference's
//   `h_in + i*dilation_h + offset_h` with offset = anchor*(s-1), _kernel.cu:226)
// ------------------------------------------------------------------------------------------
struct Axis {
  int i0;      // floor(pos)
  float w0;    // weight of i0   (1 - frac), zeroed when the sample is out of range
  float w1;    // weight of i0+1 (frac)
  bool ok;     // pos > -1 && pos < size   (_kernel.cu:228, per axis)
};

__device__ __forceinline__ Axis make_axis(int base, float off, int size) {
  Axis a;
  const float pos = (float)base + off;
  a.ok = pos > -1.0f && pos < (float)size;
  const float fl = floorf(pos);
  a.i0 = (int)fl;
  const float l = pos - fl;
  a.w1 = l;
  a.w0 = 1.0f - l;
  if (!a.ok) {  // park out-of-range samples on a readable location with zero weight
    a.i0 = 0;
    a.w0 = 0.0f;
    a.w1 = 0.0f;
  }
  return a;
}

// Bilinear sums with ONE spelled-out association (round 5).  Written with plain operators, `a*b + c*d + ...` is contracted
// into fused multiply-adds at the compiler's discretion, and the choice differed between the two instantiations of
// dw4_kernel: the stored-resolution form and the form on the materialised up-sampled tensor -- documented as
// bit-identical -- were 1 ulp apart on 4 % of the outputs (seen when a changed summation order in scale_kernel moved
// the data: a single flipped code behind them failed test_stored_resolution_stages_equal_the_upsampled_path).
__device__ __forceinline__ float bil4(float w00, float v00, float w01, float v01, float w10, float v10, float w11,
                                      float v11) {
  return fmaf(w11, v11, fmaf(w10, v10, fmaf(w01, v01, w00 * v00)));
}
__device__ __forceinline__ float lin2(float w0, float v0, float w1, float v1) { return fmaf(w1, v1, w0 * v0); }

// ------------------------------------------------------------------------------------------
// scale_kernel: s[n,p] = clamp(b + sum_c w[c] * x[n,c,p], lo, hi)
// grid = (ceil(HW/64), N), block = kSclWaves waves of 64 pixels; wave v reduces channels v, v + kSclWaves, ... with 16
// loads in flight per lane when the channel count allows (round 5: the fused schedule's scale_nchw_kernel structure --
// four waves with four loads each left the C -> 1 reduction of the QAT step's stage 0 at 1.3 TB/s, 25 us for 33.5 MB).
// ------------------------------------------------------------------------------------------
constexpr int kSclWaves = 16;
__global__ void __launch_bounds__(kSclWaves * 64)
scale_kernel(const float *__restrict__ x, const float *__restrict__ w,
             const float *__restrict__ b, float *__restrict__ s, int C, int HW, float lo,
             float hi, float2 *__restrict__ mm, cdn::QUpdate qu, unsigned *__restrict__ state_copy) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.x * 64 + lane;
  const int n = blockIdx.y;
  const bool live = p < HW;
  const float *xp = x + (long)n * C * HW + (live ? p : 0);
  constexpr int S = kSclWaves;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
  int c = wave;
  for (; c + 15 * S < C; c += 16 * S) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = xp[(long)(c + u * S) * HW];
#pragma unroll
    for (int u = 0; u < 16; u += 4) {
      acc0 = fmaf(w[c + u * S], v[u], acc0);
      acc1 = fmaf(w[c + (u + 1) * S], v[u + 1], acc1);
      acc2 = fmaf(w[c + (u + 2) * S], v[u + 2], acc2);
      acc3 = fmaf(w[c + (u + 3) * S], v[u + 3], acc3);
    }
  }
  for (; c + 3 * S < C; c += 4 * S) {
    const float v0 = xp[(long)c * HW], v1 = xp[(long)(c + S) * HW];
    const float v2 = xp[(long)(c + 2 * S) * HW], v3 = xp[(long)(c + 3 * S) * HW];
    acc0 = fmaf(w[c], v0, acc0);
    acc1 = fmaf(w[c + S], v1, acc1);
    acc2 = fmaf(w[c + 2 * S], v2, acc2);
    acc3 = fmaf(w[c + 3 * S], v3, acc3);
  }
  for (; c < C; c += S) acc0 = fmaf(w[c], xp[(long)c * HW], acc0);
  __shared__ float red[kSclWaves][64];
  red[wave][lane] = (acc0 + acc1) + (acc2 + acc3);
  __syncthreads();
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  if (wave == 0 && live) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kSclWaves; ++i) v += red[i][lane];
    v += b ? b[0] : 0.0f;
    v = cdn::clamp_keep_nan(v, lo, hi);  // Hardtanh(lo, hi), modules/dcn_deform_conv.py:304-305
    s[(long)n * HW + p] = v;
    mn = mx = v;
    has_nan = (v != v);
  }
  // training path: this workgroup's {min, max} of what it wrote, for the QuantAct behind it (no separate range pass)
  // (round 6: qu.counters != NULL -- the LAST workgroup to arrive runs the QuantAct's range update itself, as the fused
  // inference schedule does: no update launch behind this kernel)
  if (qu.counters) {
    __syncthreads();
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x,
                             gridDim.x * gridDim.y, qu, &red[0][0]);
    cdn::last_block_state_copy(qu, state_copy, &red[0][0]);
  } else if (mm) {
    __syncthreads();
    cdn::block_minmax_store(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), &mm[blockIdx.y * gridDim.x + blockIdx.x], &red[0][0]);
  }
}

// ------------------------------------------------------------------------------------------
// dw_kernel: d[n,c,h,w] = sum_{i,j} wd[c,i,j] * bilinear(x[n,c], h+(i-1)+(i-1)t, w+(j-1)+(j-1)t)
// One workgroup = (n, CC consecutive channels, whole HxW plane).  Planes live in LDS as
// (H+2)x(W+2) with a zero border, so the four corner reads never need a bounds test.
// ------------------------------------------------------------------------------------------
constexpr int kDwThreads = 256;

template <bool LDS>
__global__ void __launch_bounds__(kDwThreads)
dw_kernel(const float *__restrict__ x, const float *__restrict__ s, const float *__restrict__ wd,
          float *__restrict__ d, int C, int H, int W, int CC, float2 *__restrict__ mm) {
  extern __shared__ float smem[];
  __shared__ float red_mm[8];
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  const int HW = H * W;
  const int Wp = W + 2, Hp = H + 2;
  const int pstride = Hp * Wp;
  const int n = blockIdx.y;
  const int c0 = blockIdx.x * CC;
  const int cc = min(CC, C - c0);
  const float *xg = x + ((long)n * C + c0) * HW;
  float *wl = smem;                       // [CC][9] depthwise weights
  float *planes = smem + ((CC * 9 + 3) & ~3);  // [CC][Hp][Wp]
  for (int q = threadIdx.x; q < cc * 9; q += kDwThreads) wl[q] = wd[(long)c0 * 9 + q];
  if (LDS) {
    for (int q = threadIdx.x; q < cc * pstride; q += kDwThreads) planes[q] = 0.0f;
    __syncthreads();
    for (int q = threadIdx.x; q < cc * HW; q += kDwThreads) {
      const int ch = q / HW, r = q - ch * HW;
      const int yy = r / W, xx = r - yy * W;
      planes[ch * pstride + (yy + 1) * Wp + xx + 1] = xg[q];
    }
  }
  __syncthreads();

  for (int p = threadIdx.x; p < HW; p += kDwThreads) {
    const int h = p / W, w = p - h * W;
    const float t = s[(long)n * HW + p] - 1.0f;
    // anchor * (s-1): -t for i=0 / j=0, +t for i=2 / j=2, exactly 0 for the middle row/column
    const Axis ya = make_axis(h - 1, -t, H), yb = make_axis(h + 1, t, H);
    const Axis xa = make_axis(w - 1, -t, W), xb = make_axis(w + 1, t, W);
    // corner taps: k = 0 (ya,xa), 2 (ya,xb), 6 (yb,xa), 8 (yb,xb)
    const int b00 = (ya.i0 + 1) * Wp + xa.i0 + 1, b02 = (ya.i0 + 1) * Wp + xb.i0 + 1;
    const int b20 = (yb.i0 + 1) * Wp + xa.i0 + 1, b22 = (yb.i0 + 1) * Wp + xb.i0 + 1;
    // edge taps: k = 1 (ya, w), 7 (yb, w), 3 (h, xa), 5 (h, xb); centre k = 4 (h, w)
    const int b01 = (ya.i0 + 1) * Wp + w + 1, b21 = (yb.i0 + 1) * Wp + w + 1;
    const int b10 = (h + 1) * Wp + xa.i0 + 1, b12 = (h + 1) * Wp + xb.i0 + 1;
    const int b11 = (h + 1) * Wp + w + 1;
    for (int ch = 0; ch < cc; ++ch) {
      const float *wk = wl + ch * 9;
      float acc;
      if (LDS) {
        const float *pl = planes + ch * pstride;
#define CDN_CORNER(B, Y, X)                                                                   \
  bil4(Y.w0 * X.w0, pl[B], Y.w0 * X.w1, pl[B + 1], Y.w1 * X.w0, pl[B + Wp], Y.w1 * X.w1, pl[B + Wp + 1])
        const float v0 = CDN_CORNER(b00, ya, xa);
        const float v2 = CDN_CORNER(b02, ya, xb);
        const float v6 = CDN_CORNER(b20, yb, xa);
        const float v8 = CDN_CORNER(b22, yb, xb);
#undef CDN_CORNER
        const float v1 = lin2(ya.w0, pl[b01], ya.w1, pl[b01 + Wp]);
        const float v7 = lin2(yb.w0, pl[b21], yb.w1, pl[b21 + Wp]);
        const float v3 = lin2(xa.w0, pl[b10], xa.w1, pl[b10 + 1]);
        const float v5 = lin2(xb.w0, pl[b12], xb.w1, pl[b12 + 1]);
        const float v4 = pl[b11];
        acc = wk[0] * v0;
        acc = fmaf(wk[1], v1, acc);
        acc = fmaf(wk[2], v2, acc);
        acc = fmaf(wk[3], v3, acc);
        acc = fmaf(wk[4], v4, acc);
        acc = fmaf(wk[5], v5, acc);
        acc = fmaf(wk[6], v6, acc);
        acc = fmaf(wk[7], v7, acc);
        acc = fmaf(wk[8], v8, acc);
      } else {
        // planes too large for LDS: gather straight from global / L2 with bounds tests
        const float *pl = xg + (long)ch * HW;
        auto rd = [&](int yy, int xx) -> float {
          return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? pl[yy * W + xx] : 0.0f;
        };
        auto tap = [&](const Axis &Y, const Axis &X) -> float {
          return bil4(Y.w0 * X.w0, rd(Y.i0, X.i0), Y.w0 * X.w1, rd(Y.i0, X.i0 + 1), Y.w1 * X.w0, rd(Y.i0 + 1, X.i0),
                      Y.w1 * X.w1, rd(Y.i0 + 1, X.i0 + 1));
        };
        auto tap_v = [&](const Axis &Y) -> float { return lin2(Y.w0, rd(Y.i0, w), Y.w1, rd(Y.i0 + 1, w)); };
        auto tap_h = [&](const Axis &X) -> float { return lin2(X.w0, rd(h, X.i0), X.w1, rd(h, X.i0 + 1)); };
        acc = wk[0] * tap(ya, xa);
        acc = fmaf(wk[1], tap_v(ya), acc);
        acc = fmaf(wk[2], tap(ya, xb), acc);
        acc = fmaf(wk[3], tap_h(xa), acc);
        acc = fmaf(wk[4], pl[p], acc);
        acc = fmaf(wk[5], tap_h(xb), acc);
        acc = fmaf(wk[6], tap(yb, xa), acc);
        acc = fmaf(wk[7], tap_v(yb), acc);
        acc = fmaf(wk[8], tap(yb, xb), acc);
      }
      d[((long)n * C + c0 + ch) * HW + p] = acc;
      mn = fminf(mn, acc);
      mx = fmaxf(mx, acc);
      has_nan |= (acc != acc);
    }
  }
  if (mm) cdn::block_minmax_store(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), &mm[blockIdx.y * gridDim.x + blockIdx.x], red_mm);
}

// ------------------------------------------------------------------------------------------
// dw4_kernel (round 3): dw_kernel's LDS form with the planes interleaved in channel QUADS -- [CC / 4][Hp][Wp][4] -- so a
// lane fetches the four channels of a cell with ONE ds_read_b128 where dw_kernel issues four ds_read_b32 (25 instead
// of 100 LDS reads per pixel and quad; consecutive lanes = consecutive pixels read consecutive 16-byte cells).  Same
// per-channel expressions in the same order: bit-identical to dw_kernel.  C % 4 == 0, CC % 4 == 0.
// ------------------------------------------------------------------------------------------
// UP (round 4, stages 1-2 of the QAT step): x and s are given at STORED resolution -- x [N][C][H/2][W/2] is the tensor
// whose nearest x2 up-sampling the stage reads, s [N][H/2][W/2] is constant over each 2x2 block (a 1x1 conv of a
// replicated tensor) -- and the planes in LDS are the stored ones: the full-resolution corner (yy, xx) is the stored
// cell (yy >> 1, xx >> 1).  Same per-pixel expressions on the same values: d is bit-identical to the kernel run on the
// materialised up-sampled tensor, which is never written or read (4x less staging, 4x less LDS per channel).
template <bool UP>
__global__ void __launch_bounds__(kDwThreads)
dw4_kernel(const float *__restrict__ x, const float *__restrict__ s, const float *__restrict__ wd,
           float *__restrict__ d, int C, int H, int W, int CC, float2 *__restrict__ mm, cdn::QUpdate qu,
           unsigned *__restrict__ state_copy) {
  extern __shared__ float smem[];
  __shared__ float red_mm[16];
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  const int HW = H * W;
  const int Hl = UP ? H >> 1 : H, Wl = UP ? W >> 1 : W;   // resolution of the planes in LDS
  const int HWl = Hl * Wl;
  const int Wp = Wl + 2, Hp = Hl + 2;
  const int pstride = Hp * Wp;
  const int n = blockIdx.y;
  const int c0 = blockIdx.x * CC;
  const int cc = min(CC, C - c0);                         // (a multiple of 4)
  const float *xg = x + ((long)n * C + c0) * HWl;
  float *wl = smem;                                       // [CC][9] depthwise weights
  float4 *planes = reinterpret_cast<float4 *>(smem + ((CC * 9 + 3) & ~3));   // [CC / 4][Hp][Wp] of channel quads
  for (int q = threadIdx.x; q < cc * 9; q += kDwThreads) wl[q] = wd[(long)c0 * 9 + q];
  for (int q = threadIdx.x; q < (cc >> 2) * pstride; q += kDwThreads) planes[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  for (int q = threadIdx.x; q < cc * HWl; q += kDwThreads) {
    const int ch = q / HWl, r = q - ch * HWl;
    const int yy = r / Wl, xx = r - yy * Wl;
    reinterpret_cast<float *>(planes)[(((ch >> 2) * pstride + (yy + 1) * Wp + xx + 1) << 2) + (ch & 3)] = xg[q];
  }
  __syncthreads();
  for (int p = threadIdx.x; p < HW; p += kDwThreads) {
    const int h = p / W, w = p - h * W;
    const float t = (UP ? s[(long)n * HWl + (h >> 1) * Wl + (w >> 1)] : s[(long)n * HW + p]) - 1.0f;
    const Axis ya = make_axis(h - 1, -t, H), yb = make_axis(h + 1, t, H);
    const Axis xa = make_axis(w - 1, -t, W), xb = make_axis(w + 1, t, W);
    // row / column of a full-resolution index in the bordered LDS plane, and the step to the next corner
    auto cell = [&](int i) { return (UP ? (i >> 1) : i) + 1; };
    auto step = [&](int i) { return UP ? ((i + 1) >> 1) - (i >> 1) : 1; };
    const int rya = cell(ya.i0) * Wp, ryb = cell(yb.i0) * Wp, rh = cell(h) * Wp;
    const int cxa = cell(xa.i0), cxb = cell(xb.i0), cw = cell(w);
    const int dya = step(ya.i0) * Wp, dyb = step(yb.i0) * Wp, dxa = step(xa.i0), dxb = step(xb.i0);
    const int b00 = rya + cxa, b02 = rya + cxb;
    const int b20 = ryb + cxa, b22 = ryb + cxb;
    const int b01 = rya + cw, b21 = ryb + cw;
    const int b10 = rh + cxa, b12 = rh + cxb;
    const int b11 = rh + cw;
    // the products of the corner weights, once per pixel (dw_kernel forms the same products per channel)
    const float aa00 = ya.w0 * xa.w0, aa01 = ya.w0 * xa.w1, aa10 = ya.w1 * xa.w0, aa11 = ya.w1 * xa.w1;
    const float ab00 = ya.w0 * xb.w0, ab01 = ya.w0 * xb.w1, ab10 = ya.w1 * xb.w0, ab11 = ya.w1 * xb.w1;
    const float ba00 = yb.w0 * xa.w0, ba01 = yb.w0 * xa.w1, ba10 = yb.w1 * xa.w0, ba11 = yb.w1 * xa.w1;
    const float bb00 = yb.w0 * xb.w0, bb01 = yb.w0 * xb.w1, bb10 = yb.w1 * xb.w0, bb11 = yb.w1 * xb.w1;
    for (int g = 0; g < (cc >> 2); ++g) {
      const float4 *pl = planes + g * pstride;
      const float4 c00 = pl[b00], c01 = pl[b00 + dxa], c02 = pl[b00 + dya], c03 = pl[b00 + dya + dxa];
      const float4 c20 = pl[b02], c21 = pl[b02 + dxb], c22 = pl[b02 + dya], c23 = pl[b02 + dya + dxb];
      const float4 c60 = pl[b20], c61 = pl[b20 + dxa], c62 = pl[b20 + dyb], c63 = pl[b20 + dyb + dxa];
      const float4 c80 = pl[b22], c81 = pl[b22 + dxb], c82 = pl[b22 + dyb], c83 = pl[b22 + dyb + dxb];
      const float4 e10 = pl[b01], e11 = pl[b01 + dya], e70 = pl[b21], e71 = pl[b21 + dyb];
      const float4 e30 = pl[b10], e31 = pl[b10 + dxa], e50 = pl[b12], e51 = pl[b12 + dxb];
      const float4 ctr = pl[b11];
#define CDN_DW4_CH(E, OFF)                                                                             \
      {                                                                                                  \
        const float *wk = wl + (4 * g + OFF) * 9;                                                        \
        const float v0 = bil4(aa00, c00.E, aa01, c01.E, aa10, c02.E, aa11, c03.E);                       \
        const float v2 = bil4(ab00, c20.E, ab01, c21.E, ab10, c22.E, ab11, c23.E);                       \
        const float v6 = bil4(ba00, c60.E, ba01, c61.E, ba10, c62.E, ba11, c63.E);                       \
        const float v8 = bil4(bb00, c80.E, bb01, c81.E, bb10, c82.E, bb11, c83.E);                       \
        const float v1 = lin2(ya.w0, e10.E, ya.w1, e11.E);                                               \
        const float v7 = lin2(yb.w0, e70.E, yb.w1, e71.E);                                               \
        const float v3 = lin2(xa.w0, e30.E, xa.w1, e31.E);                                               \
        const float v5 = lin2(xb.w0, e50.E, xb.w1, e51.E);                                               \
        float acc = wk[0] * v0;                                                                          \
        acc = fmaf(wk[1], v1, acc);                                                                      \
        acc = fmaf(wk[2], v2, acc);                                                                      \
        acc = fmaf(wk[3], v3, acc);                                                                      \
        acc = fmaf(wk[4], ctr.E, acc);                                                                   \
        acc = fmaf(wk[5], v5, acc);                                                                      \
        acc = fmaf(wk[6], v6, acc);                                                                      \
        acc = fmaf(wk[7], v7, acc);                                                                      \
        acc = fmaf(wk[8], v8, acc);                                                                      \
        d[((long)n * C + c0 + 4 * g + OFF) * HW + p] = acc;                                              \
        mn = fminf(mn, acc);                                                                             \
        mx = fmaxf(mx, acc);                                                                             \
        has_nan |= (acc != acc); \
      }
      CDN_DW4_CH(x, 0)
      CDN_DW4_CH(y, 1)
      CDN_DW4_CH(z, 2)
      CDN_DW4_CH(w, 3)
#undef CDN_DW4_CH
    }
  }
  if (qu.counters) {
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x,
                             gridDim.x * gridDim.y, qu, red_mm);
    cdn::last_block_state_copy(qu, state_copy, red_mm);
  } else if (mm) cdn::block_minmax_store(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), &mm[blockIdx.y * gridDim.x + blockIdx.x], red_mm);
}

// ------------------------------------------------------------------------------------------
// dw_bwd_kernel: backward of dw_kernel for one (n, CC channels, plane) workgroup.
//   grad_x : the <=25 bilinear corner contributions of every (pixel, channel) are summed
//            with LDS float atomics into a zero-bordered LDS image of the plane (the border
//            absorbs out-of-image corners), then stored once -- no global atomics, no
//            5x5 window scan (reference: _kernel.cu:278-334, global atomicAdd :329).
//   grad_s : dL/ds = sum_c sum_k g*wd[c,k] * ((i-1)*dS/dy + (j-1)*dS/dx), i.e. the reference's
//            18-channel grad_offset (_kernel.cu:372-435) contracted with anchor_offset
//            (autograd of modules/dcn_deform_conv.py:325); one global atomic per
//            (pixel, channel-chunk).
//   grad_w : sum_{n,p} g * S_k  (cpp:456-462), wave-reduced, LDS-accumulated, then one global
//            atomic per (workgroup, c, k).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ void __launch_bounds__(kDwThreads)
dw_bwd_kernel(const float *__restrict__ x, const float *__restrict__ s,
              const float *__restrict__ wd, const float *__restrict__ gd,
              float *__restrict__ gx, float *__restrict__ gs, float *__restrict__ gw, int C, int H,
              int W, int CC) {
  extern __shared__ float smem[];
  const int HW = H * W;
  const int Wp = W + 2, Hp = H + 2;
  const int pstride = Hp * Wp;
  const int n = blockIdx.y;
  const int c0 = blockIdx.x * CC;
  const int cc = min(CC, C - c0);
  const int lane = threadIdx.x & 63;
  const float *xg = x + ((long)n * C + c0) * HW;
  const float *gdg = gd + ((long)n * C + c0) * HW;
  const int wsz = (CC * 9 + 3) & ~3;
  float *wl = smem;                 // [CC][9] weights
  float *gwl = smem + wsz;          // [CC][9] grad_w accumulators
  float *xpl = smem + 2 * wsz;      // [CC][Hp][Wp] x, zero border
  float *gpl = xpl + CC * pstride;  // [CC][Hp][Wp] grad_x accumulators
  for (int q = threadIdx.x; q < cc * 9; q += kDwThreads) {
    wl[q] = wd[(long)c0 * 9 + q];
    gwl[q] = 0.0f;
  }
  for (int q = threadIdx.x; q < cc * pstride; q += kDwThreads) {
    xpl[q] = 0.0f;
    gpl[q] = 0.0f;
  }
  __syncthreads();
  for (int q = threadIdx.x; q < cc * HW; q += kDwThreads) {
    const int ch = q / HW, r = q - ch * HW;
    const int yy = r / W, xx = r - yy * W;
    xpl[ch * pstride + (yy + 1) * Wp + xx + 1] = xg[q];
  }
  __syncthreads();

  const int iters = (HW + kDwThreads - 1) / kDwThreads;
  for (int it = 0; it < iters; ++it) {
    const int p = it * kDwThreads + threadIdx.x;
    const bool live = p < HW;
    const int pp = live ? p : 0;
    const int h = pp / W, w = pp - h * W;
    const float t = s[(long)n * HW + pp] - 1.0f;
    const Axis ya = make_axis(h - 1, -t, H), yb = make_axis(h + 1, t, H);
    const Axis xa = make_axis(w - 1, -t, W), xb = make_axis(w + 1, t, W);
    Axis ym, xm;
    ym.i0 = h; ym.w0 = 1.0f; ym.w1 = 0.0f; ym.ok = true;
    xm.i0 = w; xm.w0 = 1.0f; xm.w1 = 0.0f; xm.ok = true;
    float gs_acc = 0.0f;
    for (int ch = 0; ch < cc; ++ch) {
      const float *pl = xpl + ch * pstride;
      float *gl = gpl + ch * pstride;
      const float *wk = wl + ch * 9;
      const float g = live ? gdg[(long)ch * HW + pp] : 0.0f;
      // tap(Y, X, ay, ax, k): value S, scatter g*wk*weights, accumulate ds and grad_w
      auto tap = [&](const Axis &Y, const Axis &X, float ay, float ax, int k) {
        const int b = (Y.i0 + 1) * Wp + X.i0 + 1;
        const float v00 = pl[b], v01 = pl[b + 1], v10 = pl[b + Wp], v11 = pl[b + Wp + 1];
        const float w00 = Y.w0 * X.w0, w01 = Y.w0 * X.w1, w10 = Y.w1 * X.w0, w11 = Y.w1 * X.w1;
        const float S = (w00 * v00 + w01 * v01) + w10 * v10 + w11 * v11;
        const float gk = g * wk[k];
        if (gx != nullptr && gk != 0.0f) {
          atomicAdd(&gl[b], w00 * gk);
          atomicAdd(&gl[b + 1], w01 * gk);
          atomicAdd(&gl[b + Wp], w10 * gk);
          atomicAdd(&gl[b + Wp + 1], w11 * gk);
        }
        const float okf = (Y.ok && X.ok) ? 1.0f : 0.0f;
        const float dSdy = X.w0 * (v10 - v00) + X.w1 * (v11 - v01);
        const float dSdx = Y.w0 * (v01 - v00) + Y.w1 * (v11 - v10);
        gs_acc += okf * gk * (ay * dSdy + ax * dSdx);
        return S;
      };
      float S[9];
      S[0] = tap(ya, xa, -1.f, -1.f, 0);
      S[1] = tap(ya, xm, -1.f, 0.f, 1);
      S[2] = tap(ya, xb, -1.f, 1.f, 2);
      S[3] = tap(ym, xa, 0.f, -1.f, 3);
      S[4] = tap(ym, xm, 0.f, 0.f, 4);
      S[5] = tap(ym, xb, 0.f, 1.f, 5);
      S[6] = tap(yb, xa, 1.f, -1.f, 6);
      S[7] = tap(yb, xm, 1.f, 0.f, 7);
      S[8] = tap(yb, xb, 1.f, 1.f, 8);
      if (gw != nullptr) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const float r = wave_sum(g * S[k]);
          if (lane == 0) atomicAdd(&gwl[ch * 9 + k], r);
        }
      }
    }
    if (gs != nullptr && live) atomicAdd(&gs[(long)n * HW + p], gs_acc);
  }
  __syncthreads();
  if (gx != nullptr) {
    float *gxg = gx + ((long)n * C + c0) * HW;
    for (int q = threadIdx.x; q < cc * HW; q += kDwThreads) {
      const int ch = q / HW, r = q - ch * HW;
      const int yy = r / W, xx = r - yy * W;
      gxg[q] = gpl[ch * pstride + (yy + 1) * Wp + xx + 1];
    }
  }
  if (gw != nullptr)
    for (int q = threadIdx.x; q < cc * 9; q += kDwThreads) atomicAdd(&gw[(long)c0 * 9 + q], gwl[q]);
}

// ------------------------------------------------------------------------------------------
// dw_bwd2_kernel: backward of the gather/depthwise with lanes <-> channels (the mapping of the
// fused forward kernel, codenet_fused.hip): workgroup = (n, CCH channels, whole plane).
//   * x (fp32) and the grad_x accumulator live in LDS as [(H+1)(W+1) cells][CCH] with a zero row /
//     zero column that absorbs every out-of-image corner;
//   * grad_x is scattered with INTEGER LDS atomics on 64-bit fixed point: on gfx950 ds_add_f32
//     sustains only 0.33 lane-ops/clk/CU against 9.1 for ds_add_u64 and 13.2 for ds_add_u32
//     (tools/probes/probe_lds_atomics.hip), and the float version of this kernel spent 88 % of
//     its time in them.  Contributions are scaled by 2^S with S chosen per workgroup from
//     max|grad_d| * max|w| so that the largest one is ~2^40 (>= 2^22 adds of headroom, resolution
//     2^-40 of the workgroup maximum -- finer than fp32), summed exactly and converted back once:
//     the sum is order-independent, so grad_x is bitwise reproducible (the reference's float
//     atomics, _kernel.cu:329, are not);
//   * grad_w accumulates in lane-private registers over all pixels (a lane IS a channel): no
//     per-element cross-lane reduction, one LDS add per lane at the end;
//   * grad_s is reduced over the CCH lanes of a pixel with xor shuffles, one global atomic per
//     (pixel, channel chunk).
// CCH is the largest of {32,16,8,4,2} whose images (4 + 8 bytes per cell and channel) fit LDS.
// Tried in round 2 and reverted: a lane owning 2-4 consecutive channels of its pixel (tap geometry, corner
// weights and cell addresses once per lane instead of once per channel: ~40 % fewer VALU instructions).  Slower at
// every stage shape (64 x 64 plane 458 -> 636 us, 16 x 16 x 1024 channels 250 -> 282 us): the kernel is bound by
// the LDS atomics' bank conflicts, not by instruction issue, and with fewer lanes per pixel one wave instruction
// scatters to twice as many unrelated cells.
// Tried in round 3 and removed: lanes <-> PIXELS with the same integer atomics on [channel][cell] planes (tap geometry
// once per lane, reused over the chunk's channels; grad_w wave-reduced).  grad_x bit-identical (the fixed-point sum is
// order-independent), 1.4-1.6 x SLOWER at every shape (16 x 16 x 1024 ch: 210 -> 328 us, 32 x 32 x 256: 232 -> 313,
// 64 x 64 x 128: 443 -> 648): the cells under 64 neighbouring pixels of one tap crowd into a few banks / the same
// addresses, where the lanes of one pixel's channels hit 64 distinct consecutive words.
// ------------------------------------------------------------------------------------------
template <int CCH>
__global__ void __launch_bounds__(1024)
dw_bwd2_kernel(const float *__restrict__ x, const float *__restrict__ s,
               const float *__restrict__ wd, const float *__restrict__ gd, float *__restrict__ gx,
               float *__restrict__ gs, float *__restrict__ gw, int C, int H, int W, long gs_chunk_stride) {
  extern __shared__ unsigned long long smem64[];
  constexpr int PPW = 64 / CCH;                  // pixels per wave step
  const int nthreads = blockDim.x, nwaves = nthreads / 64;
  const int HW = H * W, Wc = W + 1;
  const int cells = (H + 1) * Wc;
  const int n = blockIdx.y, c0 = blockIdx.x * CCH;
  const int tid = threadIdx.x;
  unsigned long long *gimg = smem64;                                   // [cells][CCH] fixed point
  float *ximg = reinterpret_cast<float *>(smem64 + (size_t)cells * CCH);  // [cells][CCH]
  float *gwl = ximg + (size_t)cells * CCH;                             // [CCH][9]
  float *red = gwl + CCH * 9;                                          // [nwaves + 1]
  for (int q = tid; q < cells * CCH; q += nthreads) {
    ximg[q] = 0.0f;
    gimg[q] = 0ull;
  }
  for (int q = tid; q < CCH * 9; q += nthreads) gwl[q] = 0.0f;
  // ---- fixed-point scale of this workgroup: max |grad_d| over its slice, max |w| over its chunk --
  // (integer maxima of the |.| bit images: a NaN in grad_d or the weights PROPAGATES -- fmaxf would drop it -- and the
  // chunk's grad_x then comes out NaN like the reference's float atomics, not as a finite fixed-point sum)
  float gmax = 0.0f;
  {
    const int cc = min(CCH, C - c0);
    const float *gp = gd + ((long)n * C + c0) * HW;
    unsigned gb = 0u, wb = 0u;
    for (int q = tid; q < cc * HW; q += nthreads) gb = max(gb, cdn::absbits(gp[q]));
    for (int q = tid; q < cc * 9; q += nthreads) wb = max(wb, cdn::absbits(wd[(long)c0 * 9 + q]));
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      gb = max(gb, (unsigned)__shfl_xor((int)gb, m, 64));
      wb = max(wb, (unsigned)__shfl_xor((int)wb, m, 64));
    }
    __syncthreads();   // (also orders the zero fill above)
    if ((tid & 63) == 0) {
      red[2 * (tid >> 6)] = __uint_as_float(gb);
      red[2 * (tid >> 6) + 1] = __uint_as_float(wb);
    }
    __syncthreads();
    gb = wb = 0u;
    for (int i = 0; i < nwaves; ++i) {
      gb = max(gb, __float_as_uint(red[2 * i]));
      wb = max(wb, __float_as_uint(red[2 * i + 1]));
    }
    gmax = __uint_as_float(gb) * __uint_as_float(wb);      // bound of |bilinear weight * g * w|; NaN / Inf when either holds one
  }
  const bool poisoned = !(gmax < INFINITY);                 // workgroup-uniform
  int e = 0;
  (void)frexpf(gmax, &e);                 // gmax < 2^e
  if (!(gmax > 0.0f) || poisoned) e = 0;
  // 2^(40-e) and 2^(e-40) must both be finite, normal floats: for gradients below ~2^-86 the scale would
  // overflow to inf (0 * inf = NaN in the scatter); clamp -- such contributions keep >= 2^-126 resolution
  e = max(-86, min(e, 126 + 40));
  const float scale = ldexpf(1.0f, 40 - e), inv_scale = ldexpf(1.0f, e - 40);
  {   // stage x: lane <-> channel, 4 pixels per thread, conflict-free scalar LDS stores
    const int quads = (HW + 3) >> 2;
    for (int q = tid; q < quads * CCH; q += nthreads) {
      const int cl = q % CCH, j = q / CCH;
      if (c0 + cl < C) {
        const float *xp = x + ((long)n * C + c0 + cl) * HW + j * 4;
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const int pix = j * 4 + e4;
          if (pix < HW) ximg[((pix / W) * Wc + (pix % W)) * CCH + cl] = xp[e4];
        }
      }
    }
  }
  __syncthreads();
#if defined(CDN_DIAG) && CDN_DIAG == 3   // diagnostic build: no LDS atomics (wrong grad_x)
  float *gx_ = gx; gx = nullptr;
#endif
  const int lane = tid & 63, wave = tid >> 6;
  const int cl = lane % CCH, sub = lane / CCH;
  const bool ch_ok = c0 + cl < C;
  float wk[9], gwa[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    wk[k] = ch_ok ? wd[(long)(c0 + cl) * 9 + k] : 0.0f;
    gwa[k] = 0.0f;
  }
  // (24-bit multiply: v_mul_u32_u24 is full rate, v_mul_lo_u32 a quarter of it; offsets are far below 2^24)
  auto row_off = [&](int yy) { return (int)__umul24((unsigned)(((unsigned)yy < (unsigned)H) ? yy : H), (unsigned)(Wc * CCH)); };
  auto col_off0 = [&](int xx) { return (((unsigned)xx < (unsigned)W) ? xx : W) * CCH; };     // (+ the lane's channel)
  auto scatter_s = [&](int o, float cs) {      // cs: the contribution already times the fixed-point scale
    atomicAdd(&gimg[o], cdn::fixed_rn(cs));
  };

  // One step = PPW pixels x CCH channels.  rec: what a step needs of its pixel -- everything that does not depend on the
  // channel: five row offsets (ya.i0, ya.i0 + 1, yb.i0, yb.i0 + 1, h), five column offsets (xa.i0, xa.i0 + 1, xb.i0,
  // xb.i0 + 1, w; without the lane's channel), the pixel index (-1: beyond the plane), eight axis weights and the four
  // in-range flags as 0 / 1 floats.
  struct Rec {
    int r[5], c[5], p;
    float w[8], ok[4];
  };
  auto geometry = [&](int p) {       // the reference's sampling geometry of pixel p (_kernel.cu:220-232)
    Rec g;
    const bool live = p < HW;
    const int pp = live ? p : 0;
    const int h = pp / W, w = pp - h * W;
    const float t = s[(long)n * HW + pp] - 1.0f;
    const Axis ya = make_axis(h - 1, -t, H), yb = make_axis(h + 1, t, H);
    const Axis xa = make_axis(w - 1, -t, W), xb = make_axis(w + 1, t, W);
    g.r[0] = row_off(ya.i0); g.r[1] = row_off(ya.i0 + 1); g.r[2] = row_off(yb.i0); g.r[3] = row_off(yb.i0 + 1);
    g.r[4] = row_off(h);
    g.c[0] = col_off0(xa.i0); g.c[1] = col_off0(xa.i0 + 1); g.c[2] = col_off0(xb.i0); g.c[3] = col_off0(xb.i0 + 1);
    g.c[4] = col_off0(w);
    g.p = live ? p : -1;
    g.w[0] = ya.w0; g.w[1] = ya.w1; g.w[2] = yb.w0; g.w[3] = yb.w1;
    g.w[4] = xa.w0; g.w[5] = xa.w1; g.w[6] = xb.w0; g.w[7] = xb.w1;
    g.ok[0] = ya.ok ? 1.0f : 0.0f; g.ok[1] = yb.ok ? 1.0f : 0.0f;
    g.ok[2] = xa.ok ? 1.0f : 0.0f; g.ok[3] = xb.ok ? 1.0f : 0.0f;
    return g;
  };
  auto step = [&](const Rec &R) {
    const bool live = R.p >= 0;
    const int pp = live ? R.p : 0;
    const float g = (live && ch_ok) ? gd[((long)n * C + c0 + cl) * HW + pp] : 0.0f;
    const float gsc = g * scale;            // (power-of-two scale: commutes with the roundings of the products below)
    float gs_acc = 0.0f;
    int c[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) c[q] = R.c[q] + cl;
    // corner tap: rows (ra, ra + 1 -> offsets r0, r1), columns (q0, q1), axis weights (y0, y1) x (x0, x1)
    auto tap = [&](int r0, int r1, int q0, int q1, float y0, float y1, float x0, float x1, float okf, float ay,
                   float ax, int k) {
      const int o00 = r0 + q0, o01 = r0 + q1, o10 = r1 + q0, o11 = r1 + q1;
      const float v00 = ximg[o00], v01 = ximg[o01], v10 = ximg[o10], v11 = ximg[o11];
      const float w00 = y0 * x0, w01 = y0 * x1, w10 = y1 * x0, w11 = y1 * x1;
      const float S = (w00 * v00 + w01 * v01) + w10 * v10 + w11 * v11;
      const float gk = g * wk[k];
      if (gx != nullptr) {
        const float gks = gsc * wk[k];
        scatter_s(o00, w00 * gks);
        scatter_s(o01, w01 * gks);
        scatter_s(o10, w10 * gks);
        scatter_s(o11, w11 * gks);
      }
      const float dSdy = x0 * (v10 - v00) + x1 * (v11 - v01);
      const float dSdx = y0 * (v01 - v00) + y1 * (v11 - v10);
      gs_acc += okf * gk * (ay * dSdy + ax * dSdx);
      gwa[k] = fmaf(g, S, gwa[k]);
    };
    // edge taps touch only the two cells with non-zero weight: (o0, o1) with weights (a0, a1)
    auto tap2 = [&](int o0, int o1, float a0, float a1, float okf, float sign, int k) {
      const float v0 = ximg[o0], v1 = ximg[o1];
      const float gk = g * wk[k];
      if (gx != nullptr) {
        const float gks = gsc * wk[k];
        scatter_s(o0, a0 * gks);
        scatter_s(o1, a1 * gks);
      }
      gs_acc += okf * gk * sign * (v1 - v0);
      gwa[k] = fmaf(g, a0 * v0 + a1 * v1, gwa[k]);
    };
    const float *w8 = R.w;
    tap(R.r[0], R.r[1], c[0], c[1], w8[0], w8[1], w8[4], w8[5], R.ok[0] * R.ok[2], -1.f, -1.f, 0);
    tap2(R.r[0] + c[4], R.r[1] + c[4], w8[0], w8[1], R.ok[0], -1.f, 1);
    tap(R.r[0], R.r[1], c[2], c[3], w8[0], w8[1], w8[6], w8[7], R.ok[0] * R.ok[3], -1.f, 1.f, 2);
    tap2(R.r[4] + c[0], R.r[4] + c[1], w8[4], w8[5], R.ok[2], -1.f, 3);
    {
      const int o = R.r[4] + c[4];
      if (gx != nullptr) scatter_s(o, gsc * wk[4]);
      gwa[4] = fmaf(g, ximg[o], gwa[4]);
    }
    tap2(R.r[4] + c[2], R.r[4] + c[3], w8[6], w8[7], R.ok[3], 1.f, 5);
    tap(R.r[2], R.r[3], c[0], c[1], w8[2], w8[3], w8[4], w8[5], R.ok[1] * R.ok[2], 1.f, -1.f, 6);
    tap2(R.r[2] + c[4], R.r[3] + c[4], w8[2], w8[3], R.ok[1], 1.f, 7);
    tap(R.r[2], R.r[3], c[2], c[3], w8[2], w8[3], w8[6], w8[7], R.ok[1] * R.ok[3], 1.f, 1.f, 8);
    if (gs != nullptr) {
#pragma unroll
      for (int m = CCH / 2; m > 0; m >>= 1) gs_acc += __shfl_xor(gs_acc, m, 64);
      if (cl == 0 && live) {
        if (gs_chunk_stride) gs[(long)blockIdx.x * gs_chunk_stride + (long)n * HW + R.p] = gs_acc;
        else atomicAdd(&gs[(long)n * HW + R.p], gs_acc);
      }
    }
  };
  if (CCH == 16 || CCH == 8) {
    // The kernel is VALU-bound (profiles/r05/dwbwd_pmc.txt: VALU busy 0.80 of the kernel's cycles, LDS 0.2) and a
    // third of its VALU work was the tap geometry, which every one of a pixel's CCH lanes repeated.  Geometry phase:
    // lane <-> pixel, one record per lane for a batch of 64 pixels = 64 / PPW steps; in step j the lanes of a pixel fetch
    // its record from the owner lane with DPP row broadcasts (cdn::fetch_record: VALU moves, no LDS).
    constexpr int LPP = CCH, SPB = 64 / PPW;      // lanes per pixel; steps per batch
    const int nsteps = (HW + nwaves * PPW - 1) / (nwaves * PPW);
    for (int sb = 0; sb < nsteps; sb += SPB) {
      const int own = cdn::owner_item<LPP>(lane);                  // = j * PPW + group
      const Rec G = geometry((wave + (sb + own / PPW) * nwaves) * PPW + own % PPW);
#pragma unroll 1
      for (int j = 0; j < SPB && sb + j < nsteps; ++j) {
        int gi[11] = {G.r[0], G.r[1], G.r[2], G.r[3], G.r[4], G.c[0], G.c[1], G.c[2], G.c[3], G.c[4], G.p}, oi[11];
        float gf[12] = {G.w[0], G.w[1], G.w[2], G.w[3], G.w[4], G.w[5], G.w[6], G.w[7], G.ok[0], G.ok[1], G.ok[2],
                        G.ok[3]}, of[12];
        cdn::fetch_record<LPP == 8>(j, gi, gf, oi, of);
        Rec R;
#pragma unroll
        for (int q = 0; q < 5; ++q) { R.r[q] = oi[q]; R.c[q] = oi[5 + q]; }
        R.p = oi[10];
#pragma unroll
        for (int q = 0; q < 8; ++q) R.w[q] = of[q];
#pragma unroll
        for (int q = 0; q < 4; ++q) R.ok[q] = of[8 + q];
        step(R);
      }
    }
  } else {
    for (int p0 = wave * PPW; p0 < HW; p0 += nwaves * PPW) step(geometry(p0 + sub));
  }
  if (gw != nullptr && gs_chunk_stride) {
    // reproducible: lanes of one channel by a shuffle tree, waves in wave order (gww: LDS the host adds for this form)
    float *gww = red + 32;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      float v = ch_ok ? gwa[k] : 0.0f;
#pragma unroll
      for (int m = CCH; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
      if (lane < CCH) gww[(wave * CCH + cl) * 9 + k] = v;
    }
    __syncthreads();
    for (int q = tid; q < CCH * 9; q += nthreads) {
      float v = 0.0f;
      for (int wv = 0; wv < nwaves; ++wv) v += gww[wv * CCH * 9 + q];
      gwl[q] = v;
    }
  } else if (gw != nullptr && ch_ok) {
#pragma unroll
    for (int k = 0; k < 9; ++k) atomicAdd(&gwl[cl * 9 + k], gwa[k]);   // 9 per lane, once
  }
#if defined(CDN_DIAG) && CDN_DIAG == 3
  gx = gx_;
#endif
  __syncthreads();
  if (gx != nullptr) {
    const int quads = (HW + 3) >> 2;
    const bool vec = (HW & 3) == 0;
    for (int q = tid; q < quads * CCH; q += nthreads) {
      const int c = q % CCH, j = q / CCH;
      if (c0 + c >= C) continue;
      float v[4];
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const int pix = min(j * 4 + e4, HW - 1);
        v[e4] = poisoned ? __uint_as_float(0x7fc00000u)
                         : __ll2float_rn((long long)gimg[((pix / W) * Wc + (pix % W)) * CCH + c]) * inv_scale;
      }
      float *gp = gx + ((long)n * C + c0 + c) * HW + j * 4;
      if (vec) {
        *reinterpret_cast<float4 *>(gp) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4)
          if (j * 4 + e4 < HW) gp[e4] = v[e4];
      }
    }
  }
  if (gw != nullptr)
    for (int q = tid; q < CCH * 9; q += nthreads)
      if (c0 + q / 9 < C) {
        if (gs_chunk_stride) gw[(long)n * C * 9 + (long)c0 * 9 + q] = gwl[q];
        else atomicAdd(&gw[(long)c0 * 9 + q], gwl[q]);
      }
}

// ------------------------------------------------------------------------------------------
// dw_bwd2u_kernel (round 4; VERDICT r3 "next" #3): the backward of the gather for a stage whose input is the nearest x2
// up-sampling of a STORED tensor x [N][C][H/2][W/2] with a scale plane s [N][H/2][W/2] that is constant over each 2x2
// block of output pixels (stages 1-2 of the QAT step: the stage input is the replicated output of ReLU -> QuantAct ->
// Upsample and s is a 1x1 conv of it).  dw_bwd2_kernel's structure -- lanes <-> channels, x and the 64-bit fixed-point
// grad_x accumulator as [cell][CCH] LDS images -- at STORED resolution, one 2x2 block of output pixels per lane step:
//   * the four pixels share s, so along an axis their 2 + 2 bilinear corners fall onto at most two consecutive stored
//     cells (make_fold): a corner tap scatters 2 x 2 stored cells for the whole block instead of 16 full-resolution
//     ones, an edge tap 2 instead of 8, the centre 1 instead of 4 -- 25 LDS atomics (and 25 LDS reads) per block and
//     channel instead of 100, on images a quarter of the size (4x the channels per workgroup);
//   * the gradient is accumulated with respect to the STORED tensor directly (the 2x2 sum of the up-sampling backward
//     happens in registers / in the accumulator), grad_s with respect to the stored scale plane;
//   * every pixel keeps its own fp32 corner weights (positions are those of the full-resolution kernel, bit for bit);
//     the four pixels' contributions to a stored cell are added in fp32 before the fixed-point conversion (the
//     full-resolution kernel converts each one), so grad_x agrees with it to fp32 rounding, not bit for bit.
// A pair of pixels whose floor indices differ by 2 (pos0 just below an integer, pos1 rounded up to the next one: the
// second pixel sits exactly on a grid line) does not fold onto two cells for its one-sided derivative; such a block
// (about one in 10^7 axis evaluations) is processed pixel by pixel in four passes of the same code.
// ------------------------------------------------------------------------------------------
struct Fold {
  int k;            // stored index of window slot 0 (-1 .. size/2 - 1); slot 1 = k + 1
  float r[2][2];    // r[p][slot]: weight of pixel p on the window slot (0 where p is out of range)
  float dd[2];      // 1 when pixel p's two corners ARE the two window slots (dS/dpos = V[1] - V[0]) and p is in range
  bool good;
};

__device__ __forceinline__ Fold make_fold(const Axis &a0, const Axis &a1) {
  Fold f;
  const int k = (a0.ok ? a0.i0 : a1.i0) >> 1;     // (both parked at 0 with zero weights when neither is in range)
  f.k = k;
  f.good = true;
  const Axis *ax[2] = {&a0, &a1};
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const Axis &a = *ax[p];
    const int s0 = (a.i0 >> 1) - k, s1 = ((a.i0 + 1) >> 1) - k;
    f.r[p][0] = (s0 == 0 ? a.w0 : 0.0f) + (s1 == 0 ? a.w1 : 0.0f);
    f.r[p][1] = (s0 == 1 ? a.w0 : 0.0f) + (s1 == 1 ? a.w1 : 0.0f);
    f.dd[p] = (a.ok && s1 != s0) ? 1.0f : 0.0f;
    if (a.ok && (s0 < 0 || s1 > 1)) f.good = false;
  }
  return f;
}

template <int CCH, int MAXT>
__global__ void __launch_bounds__(MAXT)
dw_bwd2u_kernel(const float *__restrict__ x, const float *__restrict__ s, const float *__restrict__ wd,
                const float *__restrict__ gd, float *__restrict__ gx, float *__restrict__ gs,
                float *__restrict__ gw, int C, int H, int W, long gs_chunk_stride) {
  // gs_chunk_stride != 0 (round 5, the REPRODUCIBLE form): grad_s and grad_w leave the kernel as per-workgroup partials --
  // gs[chunk * stride + n * HWs + p] and gw[n * C * 9 + ...], plain stores, every element exactly once -- and a
  // fixed-order reduction follows (dw_bwd_reduce_kernel); the per-channel sums over a workgroup's lanes and waves are a
  // shuffle tree and a wave-ordered loop instead of float atomics.  0: float atomics into zero-filled gs / gw.
  extern __shared__ unsigned long long smem64[];
  constexpr int PPW = 64 / CCH;                  // 2x2 blocks per wave step
  const int nthreads = blockDim.x, nwaves = nthreads / 64;
  const int Hs = H >> 1, Ws = W >> 1, HWs = Hs * Ws, HW = H * W;
  const int Wc = Ws + 1;
  const int cells = (Hs + 1) * Wc;
  const int n = blockIdx.y, c0 = blockIdx.x * CCH;
  const int tid = threadIdx.x;
  unsigned long long *gimg = smem64;                                      // [cells][CCH] fixed point
  float *ximg = reinterpret_cast<float *>(smem64 + (size_t)cells * CCH);  // [cells][CCH]
  float *gwl = ximg + (size_t)cells * CCH;                                // [CCH][9]
  float *red = gwl + CCH * 9;                                             // [2 * nwaves]
  for (int q = tid; q < cells * CCH; q += nthreads) {
    ximg[q] = 0.0f;
    gimg[q] = 0ull;
  }
  for (int q = tid; q < CCH * 9; q += nthreads) gwl[q] = 0.0f;
  float gmax = 0.0f;      // (NaN-propagating integer maxima, as in dw_bwd2_kernel)
  {
    const int cc = min(CCH, C - c0);
    const float *gp = gd + ((long)n * C + c0) * HW;
    unsigned gb = 0u, wb = 0u;
    for (int q = tid; q < cc * HW; q += nthreads) gb = max(gb, cdn::absbits(gp[q]));
    for (int q = tid; q < cc * 9; q += nthreads) wb = max(wb, cdn::absbits(wd[(long)c0 * 9 + q]));
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      gb = max(gb, (unsigned)__shfl_xor((int)gb, m, 64));
      wb = max(wb, (unsigned)__shfl_xor((int)wb, m, 64));
    }
    __syncthreads();   // (also orders the zero fill above)
    if ((tid & 63) == 0) {
      red[2 * (tid >> 6)] = __uint_as_float(gb);
      red[2 * (tid >> 6) + 1] = __uint_as_float(wb);
    }
    __syncthreads();
    gb = wb = 0u;
    for (int i = 0; i < nwaves; ++i) {
      gb = max(gb, __float_as_uint(red[2 * i]));
      wb = max(wb, __float_as_uint(red[2 * i + 1]));
    }
    // bound of one scattered value: four pixels' |bilinear weight * g * w| folded onto a cell
    gmax = __uint_as_float(gb) * (4.0f * __uint_as_float(wb));
  }
  const bool poisoned = !(gmax < INFINITY);
  int e = 0;
  (void)frexpf(gmax, &e);
  if (!(gmax > 0.0f) || poisoned) e = 0;
  e = max(-86, min(e, 126 + 40));
  const float scale = ldexpf(1.0f, 40 - e), inv_scale = ldexpf(1.0f, e - 40);
  {   // stage the stored planes: lane <-> channel, 4 stored pixels per thread
    const int quads = (HWs + 3) >> 2;
    for (int q = tid; q < quads * CCH; q += nthreads) {
      const int cl = q % CCH, j = q / CCH;
      if (c0 + cl < C) {
        const float *xp = x + ((long)n * C + c0 + cl) * HWs + j * 4;
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4) {
          const int pix = j * 4 + e4;
          if (pix < HWs) ximg[((pix / Ws) * Wc + (pix % Ws)) * CCH + cl] = xp[e4];
        }
      }
    }
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int cl = lane % CCH, sub = lane / CCH;
  const bool ch_ok = c0 + cl < C;
  float wk[9], gwa[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    wk[k] = ch_ok ? wd[(long)(c0 + cl) * 9 + k] : 0.0f;
    gwa[k] = 0.0f;
  }
  // stored row / column index -> LDS offset; every index outside the stored plane is the zero row / zero column
  // (24-bit multiply: v_mul_u32_u24 is full rate, v_mul_lo_u32 a quarter of it; offsets are far below 2^24)
  auto row_off = [&](int yy) { return (int)__umul24((unsigned)(((unsigned)yy < (unsigned)Hs) ? yy : Hs), (unsigned)(Wc * CCH)); };
  auto col_off = [&](int xx) { return (((unsigned)xx < (unsigned)Ws) ? xx : Ws) * CCH + cl; };
  auto scatter = [&](int o, float c) {
    atomicAdd(&gimg[o], cdn::fixed_rn(c * scale));
  };

  for (int b0 = wave * PPW; b0 < HWs; b0 += nwaves * PPW) {
    const int b = b0 + sub;
    const bool live = b < HWs;
    const int bb = live ? b : 0;
    const int hs = bb / Ws, ws = bb - hs * Ws;
    const int h = 2 * hs, w = 2 * ws;
    const float t = s[(long)n * HWs + bb] - 1.0f;
    float gfull[2][2];
    {
      const float *gp = gd + ((long)n * C + c0 + cl) * HW + (long)h * W + w;
      const bool on = live && ch_ok;
      const float2 g0 = on ? *reinterpret_cast<const float2 *>(gp) : make_float2(0.f, 0.f);
      const float2 g1 = on ? *reinterpret_cast<const float2 *>(gp + W) : make_float2(0.f, 0.f);
      gfull[0][0] = g0.x; gfull[0][1] = g0.y; gfull[1][0] = g1.x; gfull[1][1] = g1.y;
    }
    float gs_acc = 0.0f;
    int npass = 1;                               // pass 0: the whole block; passes 1..4 (rare, see the header): one pixel each
    for (int ps = 0; ps < npass; ++ps) {
      const int only = ps - 1, opy = only >> 1, opx = only & 1;
      Fold fya, fyb, fxa, fxb;
      float g[2][2];
      float oky[2][2], okx[2][2];                // [a / b][pixel]: in-range flags of the pass' pixels
      {
        Axis ay_[2], by_[2], ax_[2], bx_[2];     // (temporaries of this pass: nothing of them stays live over the taps)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          ay_[p] = make_axis(h + p - 1, -t, H);
          by_[p] = make_axis(h + p + 1, t, H);
          ax_[p] = make_axis(w + p - 1, -t, W);
          bx_[p] = make_axis(w + p + 1, t, W);
          if (only >= 0 && p != opy) {
            ay_[p].ok = false; ay_[p].i0 = 0; ay_[p].w0 = 0.f; ay_[p].w1 = 0.f;
            by_[p].ok = false; by_[p].i0 = 0; by_[p].w0 = 0.f; by_[p].w1 = 0.f;
          }
          if (only >= 0 && p != opx) {
            ax_[p].ok = false; ax_[p].i0 = 0; ax_[p].w0 = 0.f; ax_[p].w1 = 0.f;
            bx_[p].ok = false; bx_[p].i0 = 0; bx_[p].w0 = 0.f; bx_[p].w1 = 0.f;
          }
          oky[0][p] = ay_[p].ok ? 1.f : 0.f; oky[1][p] = by_[p].ok ? 1.f : 0.f;
          okx[0][p] = ax_[p].ok ? 1.f : 0.f; okx[1][p] = bx_[p].ok ? 1.f : 0.f;
        }
        fya = make_fold(ay_[0], ay_[1]); fyb = make_fold(by_[0], by_[1]);
        fxa = make_fold(ax_[0], ax_[1]); fxb = make_fold(bx_[0], bx_[1]);
      }
      if (ps == 0 && !(fya.good && fyb.good && fxa.good && fxb.good)) {
        npass = 5;
        continue;
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        g[p][0] = (only < 0 || (p == opy && opx == 0)) ? gfull[p][0] : 0.f;
        g[p][1] = (only < 0 || (p == opy && opx == 1)) ? gfull[p][1] : 0.f;
      }
      // ---- corner tap: rows folded by FY, columns by FX
      auto tap = [&](const Fold &FY, const Fold &FX, const float (&OY)[2], const float (&OX)[2], float ay, float ax,
                     int k) {
        const int r0 = row_off(FY.k), r1 = row_off(FY.k + 1);
        const int q0 = col_off(FX.k), q1 = col_off(FX.k + 1);
        const float v00 = ximg[r0 + q0], v01 = ximg[r0 + q1], v10 = ximg[r1 + q0], v11 = ximg[r1 + q1];
        // G[r][c] = sum_py sum_px FY.r[py][r] * FX.r[px][c] * g[py][px]
        const float t00 = FX.r[0][0] * g[0][0] + FX.r[1][0] * g[0][1], t01 = FX.r[0][1] * g[0][0] + FX.r[1][1] * g[0][1];
        const float t10 = FX.r[0][0] * g[1][0] + FX.r[1][0] * g[1][1], t11 = FX.r[0][1] * g[1][0] + FX.r[1][1] * g[1][1];
        const float G00 = FY.r[0][0] * t00 + FY.r[1][0] * t10, G01 = FY.r[0][0] * t01 + FY.r[1][0] * t11;
        const float G10 = FY.r[0][1] * t00 + FY.r[1][1] * t10, G11 = FY.r[0][1] * t01 + FY.r[1][1] * t11;
        if (gx != nullptr) {
          scatter(r0 + q0, G00 * wk[k]);
          scatter(r0 + q1, G01 * wk[k]);
          scatter(r1 + q0, G10 * wk[k]);
          scatter(r1 + q1, G11 * wk[k]);
        }
        gwa[k] += (G00 * v00 + G01 * v01) + (G10 * v10 + G11 * v11);
        // dS/dy of pixel (py, px) = FY.dd[py] * sum_c FX.r[px][c] * (V[1][c] - V[0][c]); dS/dx likewise
        const float dv0 = v10 - v00, dv1 = v11 - v01, dh0 = v01 - v00, dh1 = v11 - v10;
        const float dy0 = FX.r[0][0] * dv0 + FX.r[0][1] * dv1, dy1 = FX.r[1][0] * dv0 + FX.r[1][1] * dv1;   // by px
        const float dx0 = FY.r[0][0] * dh0 + FY.r[0][1] * dh1, dx1 = FY.r[1][0] * dh0 + FY.r[1][1] * dh1;   // by py
        float acc = 0.0f;
        acc += OY[0] * OX[0] * g[0][0] * (ay * FY.dd[0] * dy0 + ax * FX.dd[0] * dx0);
        acc += OY[0] * OX[1] * g[0][1] * (ay * FY.dd[0] * dy1 + ax * FX.dd[1] * dx0);
        acc += OY[1] * OX[0] * g[1][0] * (ay * FY.dd[1] * dy0 + ax * FX.dd[0] * dx1);
        acc += OY[1] * OX[1] * g[1][1] * (ay * FY.dd[1] * dy1 + ax * FX.dd[1] * dx1);
        gs_acc += acc * wk[k];
      };
      // ---- edge taps: one axis exact (the pixel's own row / column = the block's stored row / column)
      auto tap_v = [&](const Fold &FY, const float (&OY)[2], float ay, int k) {     // column exact
        const int r0 = row_off(FY.k), r1 = row_off(FY.k + 1), q0 = col_off(ws);
        const float v0 = ximg[r0 + q0], v1 = ximg[r1 + q0];
        const float s0 = g[0][0] + g[0][1], s1 = g[1][0] + g[1][1];               // over px
        const float G0 = FY.r[0][0] * s0 + FY.r[1][0] * s1, G1 = FY.r[0][1] * s0 + FY.r[1][1] * s1;
        if (gx != nullptr) {
          scatter(r0 + q0, G0 * wk[k]);
          scatter(r1 + q0, G1 * wk[k]);
        }
        gwa[k] += G0 * v0 + G1 * v1;
        gs_acc += wk[k] * ay * (v1 - v0) * (OY[0] * FY.dd[0] * s0 + OY[1] * FY.dd[1] * s1);
      };
      auto tap_h = [&](const Fold &FX, const float (&OX)[2], float ax, int k) {     // row exact
        const int r0 = row_off(hs), q0 = col_off(FX.k), q1 = col_off(FX.k + 1);
        const float v0 = ximg[r0 + q0], v1 = ximg[r0 + q1];
        const float s0 = g[0][0] + g[1][0], s1 = g[0][1] + g[1][1];               // over py
        const float G0 = FX.r[0][0] * s0 + FX.r[1][0] * s1, G1 = FX.r[0][1] * s0 + FX.r[1][1] * s1;
        if (gx != nullptr) {
          scatter(r0 + q0, G0 * wk[k]);
          scatter(r0 + q1, G1 * wk[k]);
        }
        gwa[k] += G0 * v0 + G1 * v1;
        gs_acc += wk[k] * ax * (v1 - v0) * (OX[0] * FX.dd[0] * s0 + OX[1] * FX.dd[1] * s1);
      };
      tap(fya, fxa, oky[0], okx[0], -1.f, -1.f, 0);
      tap_v(fya, oky[0], -1.f, 1);
      tap(fya, fxb, oky[0], okx[1], -1.f, 1.f, 2);
      tap_h(fxa, okx[0], -1.f, 3);
      {
        const int o = row_off(hs) + col_off(ws);
        const float sg = (g[0][0] + g[0][1]) + (g[1][0] + g[1][1]);
        if (gx != nullptr) scatter(o, sg * wk[4]);
        gwa[4] = fmaf(sg, ximg[o], gwa[4]);
      }
      tap_h(fxb, okx[1], 1.f, 5);
      tap(fyb, fxa, oky[1], okx[0], 1.f, -1.f, 6);
      tap_v(fyb, oky[1], 1.f, 7);
      tap(fyb, fxb, oky[1], okx[1], 1.f, 1.f, 8);
    }
    if (gs != nullptr) {
#pragma unroll
      for (int m = CCH / 2; m > 0; m >>= 1) gs_acc += __shfl_xor(gs_acc, m, 64);
      if (cl == 0 && live) {
        if (gs_chunk_stride) gs[(long)blockIdx.x * gs_chunk_stride + (long)n * HWs + b] = gs_acc;
        else atomicAdd(&gs[(long)n * HWs + b], gs_acc);
      }
    }
  }
  if (gw != nullptr && gs_chunk_stride) {
    // reproducible: lanes of one channel by a shuffle tree, waves in wave order (gww: LDS the host adds for this form)
    float *gww = red + 32;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      float v = ch_ok ? gwa[k] : 0.0f;
#pragma unroll
      for (int m = CCH; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
      if (lane < CCH) gww[(wave * CCH + cl) * 9 + k] = v;
    }
    __syncthreads();
    for (int q = tid; q < CCH * 9; q += nthreads) {
      float v = 0.0f;
      for (int wv = 0; wv < nwaves; ++wv) v += gww[wv * CCH * 9 + q];
      gwl[q] = v;
    }
  } else if (gw != nullptr && ch_ok) {
#pragma unroll
    for (int k = 0; k < 9; ++k) atomicAdd(&gwl[cl * 9 + k], gwa[k]);
  }
  __syncthreads();
  if (gx != nullptr) {
    const int quads = (HWs + 3) >> 2;
    const bool vec = (HWs & 3) == 0;
    for (int q = tid; q < quads * CCH; q += nthreads) {
      const int c = q % CCH, j = q / CCH;
      if (c0 + c >= C) continue;
      float v[4];
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const int pix = min(j * 4 + e4, HWs - 1);
        v[e4] = poisoned ? __uint_as_float(0x7fc00000u)
                         : __ll2float_rn((long long)gimg[((pix / Ws) * Wc + (pix % Ws)) * CCH + c]) * inv_scale;
      }
      float *gp = gx + ((long)n * C + c0 + c) * HWs + j * 4;
      if (vec) {
        *reinterpret_cast<float4 *>(gp) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int e4 = 0; e4 < 4; ++e4)
          if (j * 4 + e4 < HWs) gp[e4] = v[e4];
      }
    }
  }
  if (gw != nullptr)
    for (int q = tid; q < CCH * 9; q += nthreads)
      if (c0 + q / 9 < C) {
        if (gs_chunk_stride) gw[(long)n * C * 9 + (long)c0 * 9 + q] = gwl[q];
        else atomicAdd(&gw[(long)c0 * 9 + q], gwl[q]);
      }
}

// ------------------------------------------------------------------------------------------
// pointwise_kernel: Y[n] (Co x HW) = Wp (Co x C) . D[n] (C x HW) on v_mfma_f32_32x32x2_f32.
// Workgroup tile 64 (co) x 64 (pixels), 4 waves, each owning one 32x32 accumulator tile;
// K tiles of 16 staged through LDS as As[k][m] / Bs[k][n] so both operand reads are
// conflict-free (lane l reads [k = l>>5][l & 31]).
// Operand maps (cdna_hip_programming.md section 3): A[i = l&31][k = l>>5], B[k = l>>5][j = l&31];
// C/D: col = l&31, row = (r&3) + 8*(r>>2) + 4*(l>>5).
// ------------------------------------------------------------------------------------------
using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kPwBM = 64, kPwBN = 64, kPwBK = 32;

__global__ void __launch_bounds__(256)
pointwise_kernel(const float *__restrict__ D, const float *__restrict__ Wp,
                 const float *__restrict__ bias, const float *__restrict__ ep_scale,
                 const float *__restrict__ ep_shift, float *__restrict__ Y, int C, int Co, int HW,
                 int relu, float2 *__restrict__ mm, const unsigned *__restrict__ dq, long d_pitch, long y_pitch) {
  // d_pitch / y_pitch: elements between the images of D / Y (C * HW / Co * HW for whole tensors; larger where D or Y is a
  // channel slice of a wider NCHW tensor, cdn_codenet_pointwise_forward_pitched)
  // K tiles of 32, the NEXT tile's global loads (4 x 16 B per thread) in flight behind the 16 MFMAs of the
  // current one: with one 16-deep tile and no prefetch every tile paid a full global-load latency (50 TF at
  // the stage-0 shape; the QAT step runs this kernel six times: forward and data gradient of three stages)
  __shared__ float As[kPwBK][kPwBM + 4];
  __shared__ __attribute__((aligned(16))) float Bs[kPwBK][kPwBN + 4];
  const int n = blockIdx.z;
  const int m0 = blockIdx.y * kPwBM, p0 = blockIdx.x * kPwBN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const float *Dn = D + (long)n * d_pitch;
  f32x16 acc = {0};
  // staging: A tile 64(m) x 32(k): thread -> (m = tid>>2, 8 consecutive k from (tid&3)*8)
  //          B tile 32(k) x 64(n): thread -> (k = tid>>4 and +16, 4 pixels from (tid&15)*4)
  const int am = tid >> 2, ak = (tid & 3) * 8;
  const int bk = tid >> 4, bn = (tid & 15) * 4;
  // 16-byte loads only when the rows are 16-byte aligned: the public entry point puts no alignment requirement on
  // w_pw / d (a weight view at a 4-byte offset takes the scalar path)
  const bool hw4 = (HW & 3) == 0 && (d_pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(D) & 15) == 0;
  const bool c4 = (C & 3) == 0 && (reinterpret_cast<uintptr_t>(Wp) & 15) == 0;
  float a[8], b[8];
  // dq != NULL (training path): D holds PRE-quantisation values and is fake-quantised with that QuantAct state while
  // loading -- the values a separate fake-quant pass would have stored (fq(0) = 0: padding stays zero)
  float dqs = 1.f, dqz = 0.f, dqr = 1.f;
  if (dq) {
    dqs = reinterpret_cast<const float *>(dq)[2];
    dqz = reinterpret_cast<const float *>(dq)[3];
    dqr = __fdiv_rn(1.0f, dqs);
  }
  // fast: whole tiles, 16-byte aligned rows (every stage shape of the QAT step) -- four unconditional 16-byte loads
  // per thread and k tile, no bounds tests: the general form below compiles to a branch and a wait per piece
  const bool fast = hw4 && c4 && (C % kPwBK) == 0 && (HW % kPwBN) == 0 && (Co % kPwBM) == 0;
  auto load = [&](int k0) {
    const int m = m0 + am;
    if (fast) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 v = *reinterpret_cast<const float4 *>(Wp + (long)m * C + k0 + ak + 4 * h);
        a[4 * h] = v.x; a[4 * h + 1] = v.y; a[4 * h + 2] = v.z; a[4 * h + 3] = v.w;
        const float4 u = *reinterpret_cast<const float4 *>(Dn + (long)(k0 + bk + 16 * h) * HW + p0 + bn);
        b[4 * h] = u.x; b[4 * h + 1] = u.y; b[4 * h + 2] = u.z; b[4 * h + 3] = u.w;
      }
      return;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = k0 + ak + 4 * h;
      if (m < Co && c4 && k + 3 < C) {
        const float4 v = *reinterpret_cast<const float4 *>(Wp + (long)m * C + k);
        a[4 * h] = v.x; a[4 * h + 1] = v.y; a[4 * h + 2] = v.z; a[4 * h + 3] = v.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) a[4 * h + q] = (m < Co && k + q < C) ? Wp[(long)m * C + k + q] : 0.0f;
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = k0 + bk + 16 * h, p = p0 + bn;
      if (k < C && hw4 && p + 3 < HW) {
        const float4 v = *reinterpret_cast<const float4 *>(Dn + (long)k * HW + p);
        b[4 * h] = v.x; b[4 * h + 1] = v.y; b[4 * h + 2] = v.z; b[4 * h + 3] = v.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) b[4 * h + q] = (k < C && p + q < HW) ? Dn[(long)k * HW + p + q] : 0.0f;
      }
    }
  };
  load(0);
  for (int k0 = 0; k0 < C; k0 += kPwBK) {
    __syncthreads();  // previous tile fully consumed
    // (the fake-quantisation of the training path is applied HERE, when the tile is parked: inside load() it consumed
    // the prefetched values at once, so the loads of the next tile were waited for in front of the MFMAs they were meant
    // to hide behind)
    if (dq) {
#pragma unroll
      for (int q = 0; q < 8; ++q) b[q] = cdn::fake_quant_r(b[q], dqs, dqz, dqr);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) As[ak + q][am] = a[q];
#pragma unroll
    for (int h = 0; h < 2; ++h)
      *reinterpret_cast<float4 *>(&Bs[bk + 16 * h][bn]) = make_float4(b[4 * h], b[4 * h + 1], b[4 * h + 2], b[4 * h + 3]);
    __syncthreads();
    if (k0 + kPwBK < C) load(k0 + kPwBK);
#pragma unroll
    for (int kk = 0; kk < kPwBK; kk += 2) {
      const float av = As[kk + (lane >> 5)][wm + (lane & 31)];
      const float bv = Bs[kk + (lane >> 5)][wn + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
  }
  const int col = p0 + wn + (lane & 31);
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < Co && col < HW) {
      float v = acc[r];
      if (bias) v += bias[row];
      if (ep_scale) v = fmaf(v, ep_scale[row], ep_shift[row]);
      if (relu) v = cdn::relu_keep_nan(v);
      Y[(long)n * y_pitch + (long)row * HW + col] = v;
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
      has_nan |= (v != v);
    }
  }
  if (mm) {
    __syncthreads();      // (As is free: every wave has left the k loop)
    cdn::block_minmax_store(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), &mm[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x], &As[0][0]);
  }
}

// (Round 5, built and measured: a streaming form of this kernel -- pws_kernel's structure, every wave a 32 x 64 tile over
// the whole K fed by a wave-private LDS-DMA ring, persistent over pixel tiles -- bit-reproducible and correct, 57 / 34 / 39
// / 63 / 38 / 46 us at the QAT step's six launches against 71 / 32 / 42 / 62 / 36 / 44 us for this kernel and no change of
// the step (1.389-1.398 vs 1.385-1.387 ms, three interleaved pairs): at 32 x 64 outputs per wave the operands cross
// L2 -> LDS three times as often per MAC as with this kernel's shared 64 x 64 tiles.  Removed.)
}  // namespace

// The three forward kernels of the stage optionally leave one {min, max} pair per workgroup of the tensor they wrote
// (`partials`, *_range_partials(...) float2 entries): the training path's QuantAct behind them reduces those instead of
// re-reading the tensor (cdn_quantact_forward_partials / cdn_quantact_relu_up2_forward_partials).
static const cdn::QUpdate kNoUpdate = cdn::no_qupdate();

// qu (round 6): the QuantAct behind the kernel, updated by its last workgroup (cdn_codenet_*_forward_update)
static int scale_forward_impl(const float *x, const float *w_scale, const float *b_scale, float *s, int64_t N,
                              int64_t C, int64_t H, int64_t W, float lo, float hi, float *partials, void *stream,
                              const cdn::QUpdate *qu = nullptr, unsigned *qu_copy = nullptr) {
  CDN_REQUIRE(x && w_scale && s, CDN_ERR_ARG, "null tensor pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N <= 65535 && C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  const int HW = (int)(H * W);
  dim3 grid((unsigned)cdn::ceil_div(HW, 64), (unsigned)N);
  scale_kernel<<<grid, kSclWaves * 64, 0, cdn::as_stream(stream)>>>(x, w_scale, b_scale, s, (int)C, HW, lo, hi,
                                                         reinterpret_cast<float2 *>(partials), qu ? *qu : kNoUpdate, qu_copy);
  return cdn::check_launch("codenet scale forward");
}

extern "C" int cdn_codenet_scale_forward(const float *x, const float *w_scale,
                                         const float *b_scale, float *s, int64_t N, int64_t C,
                                         int64_t H, int64_t W, float lo, float hi, void *stream) {
  return scale_forward_impl(x, w_scale, b_scale, s, N, C, H, W, lo, hi, nullptr, stream);
}

extern "C" int64_t cdn_codenet_scale_range_partials(int64_t N, int64_t H, int64_t W) {
  return (N > 0 && H > 0 && W > 0) ? cdn::ceil_div(H * W, 64) * N : 0;
}

extern "C" int cdn_codenet_scale_forward_range(const float *x, const float *w_scale, const float *b_scale, float *s,
                                               int64_t N, int64_t C, int64_t H, int64_t W, float lo, float hi,
                                               float *partials, void *stream) {
  CDN_REQUIRE(partials, CDN_ERR_ARG, "null partials pointer");
  return scale_forward_impl(x, w_scale, b_scale, s, N, C, H, W, lo, hi, partials, stream);
}

static int dw_channels_per_wg(int64_t C, int64_t H, int64_t W) {
  const int pstride = (int)((H + 2) * (W + 2));
  int budget = 64 * 1024 / 4;  // floats of LDS per workgroup (2 workgroups per CU)
  int CC = (budget - 64) / (pstride + 9);
  if (CC < 4 && (C & 3) == 0) {                          // 64 x 64 planes: 76 KB hold a channel quad, still two per CU
    budget = 76 * 1024 / 4;
    CC = (budget - 64) / (pstride + 9);
    if (CC < 4) CC = (64 * 1024 / 4 - 64) / (pstride + 9);
  }
  if (CC < 1) return -4;                                 // planes too large: global gather, 4 channels per workgroup
  if (CC > 32) CC = 32;
  if (CC > C) CC = (int)C;
  if (CC >= 4 && (C & 3) == 0) CC &= ~3;                 // whole channel quads per workgroup (dw4_kernel)
  return CC;
}

// channels per workgroup of the up-sampled form (planes in LDS at stored resolution): enough workgroups to fill the
// chip twice, whole channel quads, at most 32 KB of planes (4+ workgroups per CU)
static int dw_up2_channels_per_wg(int64_t N, int64_t C, int64_t H, int64_t W) {
  if ((C & 3) || (H & 1) || (W & 1)) return 0;
  const int pstride = (int)((H / 2 + 2) * (W / 2 + 2));
  int CC = (32 * 1024 / 4 - 64) / (pstride + 9) & ~3;
  if (CC < 4) CC = (76 * 1024 / 4 - 64) / (pstride + 9) >= 4 ? 4 : 0;
  if (CC > 16) CC = 16;
  while (CC > 4 && cdn::ceil_div(C, CC) * N < 2L * cdn::kCUs) CC -= 4;
  if (CC > C) CC = (int)C;
  return CC;
}

static int dw_up2_forward_impl(const float *x, const float *s, const float *w_dw, float *d, int64_t N, int64_t C,
                               int64_t H, int64_t W, float *partials, void *stream, const cdn::QUpdate *qu = nullptr,
                               unsigned *qu_copy = nullptr) {
  CDN_REQUIRE(x && s && w_dw && d, CDN_ERR_ARG, "null tensor pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N <= 65535 && N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  const int CC = dw_up2_channels_per_wg(N, C, H, W);
  CDN_REQUIRE(CC >= 4, CDN_ERR_UNSUPPORTED, "up-sampled gather needs C %% 4 == 0, even H, W and a stored plane that fits LDS");
  const int pstride = (int)((H / 2 + 2) * (W / 2 + 2));
  const size_t lds = (size_t)(((CC * 9 + 3) & ~3) + CC * pstride) * sizeof(float);
  hipStream_t st = cdn::as_stream(stream);
  dim3 grid((unsigned)cdn::ceil_div(C, CC), (unsigned)N);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void *)dw4_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  dw4_kernel<true><<<grid, kDwThreads, lds, st>>>(x, s, w_dw, d, (int)C, (int)H, (int)W, CC,
                                                  reinterpret_cast<float2 *>(partials), qu ? *qu : kNoUpdate, qu_copy);
  return cdn::check_launch("codenet dw forward (up-sampled input)");
}

extern "C" int cdn_codenet_dw_up2_supported(int64_t N, int64_t C, int64_t H, int64_t W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return 0;
  if (dw_up2_channels_per_wg(N, C, H, W) < 4) return 0;
  const size_t cells = (size_t)(H / 2 + 1) * (W / 2 + 1);
  return cells * 2 * 12 + 2 * 9 * 4 + 256 <= (size_t)160 * 1024 - 512;
}

extern "C" int64_t cdn_codenet_dw_up2_range_partials(int64_t N, int64_t C, int64_t H, int64_t W) {
  const int CC = (N > 0 && C > 0 && H > 0 && W > 0) ? dw_up2_channels_per_wg(N, C, H, W) : 0;
  return CC >= 4 ? cdn::ceil_div(C, CC) * N : 0;
}

extern "C" int cdn_codenet_dw_up2_forward(const float *x_stored, const float *s_stored, const float *w_dw, float *d,
                                          int64_t N, int64_t C, int64_t H, int64_t W, float *partials, void *stream) {
  return dw_up2_forward_impl(x_stored, s_stored, w_dw, d, N, C, H, W, partials, stream);
}

// fixed-order sums of the reproducible backward's partials: grad_s[n][p] over the channel chunks, grad_w[c][k] over the
// images (four sums in flight, combined in one order)
__global__ void __launch_bounds__(256)
dw_bwd_reduce_kernel(const float *__restrict__ gs_part, float *__restrict__ gs, long ns, int chunks,
                     const float *__restrict__ gw_part, float *__restrict__ gw, long nw, int N) {
  const long sblocks = gs ? (ns + 255) / 256 : 0;
  const bool second = (long)blockIdx.x >= sblocks;
  const float *src = second ? gw_part : gs_part;
  float *dst = second ? gw : gs;
  const long len = second ? nw : ns;
  const int terms = second ? N : chunks;
  const long i = ((long)blockIdx.x - (second ? sblocks : 0)) * 256 + threadIdx.x;
  if (i >= len) return;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int z = 0;
  for (; z + 3 < terms; z += 4) {
    s0 += src[(long)z * len + i];
    s1 += src[(long)(z + 1) * len + i];
    s2 += src[(long)(z + 2) * len + i];
    s3 += src[(long)(z + 3) * len + i];
  }
  for (; z < terms; ++z) s0 += src[(long)z * len + i];
  dst[i] = (s0 + s1) + (s2 + s3);
}

// channel chunk of the lanes <-> channels backward kernels (shared by the launchers and the workspace query)
// (det: the reproducible form's per-wave weight-gradient sums, at most 16 waves x c x 9 floats more)
static int bwd2u_cch(int64_t N, int64_t C, int64_t Hs, int64_t Ws, bool det) {
  const size_t cells = (size_t)(Hs + 1) * (Ws + 1);
  const size_t lds_max = 160 * 1024 - 512;
  auto bwd_lds = [&](int c) { return cells * c * 12 + (size_t)c * 9 * 4 + 256 + (det ? (size_t)c * 16 * 36 : 0); };
  int cch = 0;
  for (int c : {32, 16, 8, 4, 2})
    if (bwd_lds(c) <= lds_max) {
      cch = c;
      break;
    }
  if (cch == 0) return 0;
#if defined(CDN_BWDU_CCH)
  cch = CDN_BWDU_CCH;
#else
  if (cch >= 16 && bwd_lds(cch / 2) * 2 <= lds_max) cch /= 2;
  while (cch > 4 && cdn::ceil_div(C, cch) * N < (long)cdn::kCUs) cch /= 2;
#endif
  return cch;
}
static int bwd2_cch(int64_t H, int64_t W, bool det) {
  const size_t cells = (size_t)(H + 1) * (W + 1);
  const size_t lds_max = 160 * 1024 - 512;
  auto bwd_lds = [&](int c) { return cells * c * 12 + (size_t)c * 9 * 4 + 128 + (det ? (size_t)c * 16 * 36 : 0); };
  int cch = 0;
  for (int c : {32, 16, 8, 4, 2})
    if (bwd_lds(c) <= lds_max) {
      cch = c;
      break;
    }
  if (cch >= 16 && bwd_lds(cch / 2) * 2 <= lds_max) cch /= 2;
  return cch;
}
// workspace of the reproducible form: grad_s partials [chunks][N][plane] + grad_w partials [N][C][9]
static size_t bwd_r_bytes(int64_t N, int64_t C, int64_t plane, int cch) {
  return ((size_t)cdn::ceil_div(C, cch) * N * plane + (size_t)N * C * 9) * sizeof(float);
}

static int dw_up2_backward_impl(const float *x_stored, const float *s_stored, const float *w_dw,
                                const float *grad_d, float *grad_x, float *grad_s, float *grad_w, int64_t N,
                                int64_t C, int64_t H, int64_t W, void *stream, float *part) {
  CDN_REQUIRE(x_stored && s_stored && w_dw && grad_d, CDN_ERR_ARG, "null tensor pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && (H & 1) == 0 && (W & 1) == 0, CDN_ERR_ARG, "bad size (even H, W)");
  CDN_REQUIRE(N <= 65535 && N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  CDN_REQUIRE((reinterpret_cast<uintptr_t>(grad_d) & 7) == 0 && (reinterpret_cast<uintptr_t>(grad_x) & 15) == 0,
              CDN_ERR_ARG, "grad_d must be 8-byte, grad_x 16-byte aligned");
  hipStream_t st = cdn::as_stream(stream);
  const int64_t Hs = H / 2, Ws = W / 2;
  if (grad_s && !part) {
    // (grad_w directly behind grad_s: one fill for both -- a QAT step is made of launches this small)
    const size_t ns = (size_t)(N * Hs * Ws), extra = (grad_w == grad_s + ns) ? (size_t)C * 9 : 0;
    hipError_t e = hipMemsetAsync(grad_s, 0, sizeof(float) * (ns + extra), st);
    if (e != hipSuccess) return cdn::fail(CDN_ERR_HIP, "memset grad_s: %s", hipGetErrorString(e));
  }
  const size_t cells = (size_t)(Hs + 1) * (Ws + 1);
  const size_t lds_max = 160 * 1024 - 512;
  auto bwd_lds = [&](int c) { return cells * c * 12 + (size_t)c * 9 * 4 + 256; };
  // two workgroups per CU when the halved chunk allows it (more waves hide the LDS atomics' latency), and enough
  // workgroups to fill the chip (bwd2u_cch)
  const int cch = bwd2u_cch(N, C, Hs, Ws, part != nullptr);
  CDN_REQUIRE(cch != 0, CDN_ERR_UNSUPPORTED, "stored plane too large for the LDS-resident backward");
  size_t lds = bwd_lds(cch);
  dim3 grid((unsigned)cdn::ceil_div(C, cch), (unsigned)N);
  // The kernel wants ~170 VGPRs: three waves per SIMD = 12 waves per CU (capped at 128 VGPRs for 1024-thread workgroups
  // it spills 40+ of them: 131 / 220 us against 99 / 165 us at the two stage shapes, batch 32).  768 threads when only
  // one workgroup fits a CU (64 x 64 stage), 256 when several do (32 x 32 stage: two of 55 KB)
  // (measured at the 32 x 32 / 64 x 64 stage: 256 threads 95 / 281 us, 384 (uneven over the four SIMDs) 122 / -,
  // 512: 105 / 184, 768: 99 / 165, 1024: 131 / 220).
#if !defined(CDN_BWDU_MAXT)
#define CDN_BWDU_MAXT 768
#endif
#if defined(CDN_BWDU_THREADS)
  const int threads = CDN_BWDU_THREADS;
#else
  const int threads = lds_max / (lds + (part ? (size_t)cch * 16 * 36 : 0)) <= 1 ? 768 : 256;
#endif
  // reproducible form: partials into the workspace, LDS for the per-wave weight-gradient sums
  const long plane = (long)(Hs * Ws), stride = part ? (long)N * plane : 0;
  float *gs_part = part, *gw_part = part ? part + (size_t)cdn::ceil_div(C, cch) * N * plane : nullptr;
  if (part) lds += (size_t)(threads / 64) * cch * 9 * 4;
#define CDN_BWDU(CCH_)                                                                                      \
  {                                                                                                         \
    auto kern = dw_bwd2u_kernel<CCH_, CDN_BWDU_MAXT>;                                                                    \
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);    \
    kern<<<grid, threads, lds, st>>>(x_stored, s_stored, w_dw, grad_d, grad_x, part ? gs_part : grad_s,       \
                                     part ? gw_part : grad_w, (int)C, (int)H, (int)W, stride);                \
  }
  switch (cch) {
    case 32: CDN_BWDU(32) break;
    case 16: CDN_BWDU(16) break;
    case 8: CDN_BWDU(8) break;
    case 4: CDN_BWDU(4) break;
    default: CDN_BWDU(2) break;
  }
#undef CDN_BWDU
  int rc = cdn::check_launch("codenet dw backward (up-sampled input)");
  if (rc || !part) return rc;
  const long ns = grad_s ? (long)N * plane : 0, nw = grad_w ? (long)C * 9 : 0;
  if (ns + nw == 0) return 0;
  dw_bwd_reduce_kernel<<<(unsigned)(cdn::ceil_div(ns, 256) + cdn::ceil_div(nw, 256)), 256, 0, st>>>(
      gs_part, grad_s, ns, (int)cdn::ceil_div(C, cch), gw_part, grad_w, nw, (int)N);
  return cdn::check_launch("codenet dw backward reduce");
}

extern "C" int cdn_codenet_dw_up2_backward(const float *x_stored, const float *s_stored, const float *w_dw,
                                           const float *grad_d, float *grad_x, float *grad_s, float *grad_w, int64_t N,
                                           int64_t C, int64_t H, int64_t W, void *stream) {
  return dw_up2_backward_impl(x_stored, s_stored, w_dw, grad_d, grad_x, grad_s, grad_w, N, C, H, W, stream, nullptr);
}

static int dw_forward_impl(const float *x, const float *s, const float *w_dw, float *d, int64_t N, int64_t C,
                           int64_t H, int64_t W, float *partials, void *stream, const cdn::QUpdate *qu = nullptr,
                               unsigned *qu_copy = nullptr) {
  CDN_REQUIRE(x && s && w_dw && d, CDN_ERR_ARG, "null tensor pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N <= 65535 && N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  const int pstride = (int)((H + 2) * (W + 2));
  int CC = dw_channels_per_wg(C, H, W);
  hipStream_t st = cdn::as_stream(stream);
  float2 *mm = reinterpret_cast<float2 *>(partials);
  if (CC >= 1) {
    const size_t lds = (size_t)(((CC * 9 + 3) & ~3) + CC * pstride) * sizeof(float);
    dim3 grid((unsigned)cdn::ceil_div(C, CC), (unsigned)N);
    if ((CC & 3) == 0 && (C & 3) == 0) {    // channel quads in LDS: one 16-byte read per cell and quad
      if (lds > 64 * 1024)
        (void)hipFuncSetAttribute((const void *)dw4_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      dw4_kernel<false><<<grid, kDwThreads, lds, st>>>(x, s, w_dw, d, (int)C, (int)H, (int)W, CC, mm,
                                                       qu ? *qu : kNoUpdate, qu_copy);
    }
    else {
      CDN_REQUIRE(!qu, CDN_ERR_UNSUPPORTED, "the in-kernel range update needs the channel-quad gather (C %% 4 == 0)");
      dw_kernel<true><<<grid, kDwThreads, lds, st>>>(x, s, w_dw, d, (int)C, (int)H, (int)W, CC, mm);
    }
  } else {
    CDN_REQUIRE(!qu, CDN_ERR_UNSUPPORTED, "the in-kernel range update needs an LDS-resident plane");
    CC = 4;
    const size_t lds = (size_t)((CC * 9 + 3) & ~3) * sizeof(float);
    dim3 grid((unsigned)cdn::ceil_div(C, CC), (unsigned)N);
    dw_kernel<false><<<grid, kDwThreads, lds, st>>>(x, s, w_dw, d, (int)C, (int)H, (int)W, CC, mm);
  }
  return cdn::check_launch("codenet dw forward");
}

extern "C" int cdn_codenet_dw_forward(const float *x, const float *s, const float *w_dw, float *d,
                                      int64_t N, int64_t C, int64_t H, int64_t W, void *stream) {
  return dw_forward_impl(x, s, w_dw, d, N, C, H, W, nullptr, stream);
}

extern "C" int64_t cdn_codenet_dw_range_partials(int64_t N, int64_t C, int64_t H, int64_t W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const int CC = dw_channels_per_wg(C, H, W);
  return cdn::ceil_div(C, CC >= 1 ? CC : 4) * N;
}

extern "C" int cdn_codenet_dw_forward_range(const float *x, const float *s, const float *w_dw, float *d, int64_t N,
                                            int64_t C, int64_t H, int64_t W, float *partials, void *stream) {
  CDN_REQUIRE(partials, CDN_ERR_ARG, "null partials pointer");
  return dw_forward_impl(x, s, w_dw, d, N, C, H, W, partials, stream);
}

// ---- round 6: the QAT step's producers update the QuantAct behind them in their LAST workgroup (cdn::block_minmax_finish,
// the fused inference schedule's protocol) -- no cdn_quantact_forward_partials update launch, no state-copy launch.
// counters: cdn_quantact_arrive_words() zero-initialised 32-bit words per QuantAct (left zero by every call);
// state_copy (8 words, may be NULL): the state after the update, for the backward pass.
extern "C" int cdn_quantact_arrive_words(void) { return cdn::kArriveWords; }

extern "C" int cdn_codenet_scale_forward_update(const float *x, const float *w_scale, const float *b_scale, float *s,
                                                int64_t N, int64_t C, int64_t H, int64_t W, float lo, float hi,
                                                float *x_min, float *x_max, void *state, void *counters, int bits,
                                                double momentum, void *state_copy, void *stream) {
  cdn::QUpdate qu;
  if (int rc = cdn::tracked_qupdate(&qu, x_min, x_max, state, counters, bits, momentum)) return rc;
  return scale_forward_impl(x, w_scale, b_scale, s, N, C, H, W, lo, hi, nullptr, stream, &qu,
                            static_cast<unsigned *>(state_copy));
}

extern "C" int cdn_codenet_dw_forward_update_supported(int64_t N, int64_t C, int64_t H, int64_t W, int up2) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || (C & 3)) return 0;
  if (up2) return dw_up2_channels_per_wg(N, C, H, W) >= 4 ? 1 : 0;
  const int CC = dw_channels_per_wg(C, H, W);
  return (CC >= 4 && (CC & 3) == 0) ? 1 : 0;
}

extern "C" int cdn_codenet_dw_forward_update(const float *x, const float *s, const float *w_dw, float *d, int64_t N,
                                             int64_t C, int64_t H, int64_t W, int up2, float *x_min, float *x_max,
                                             void *state, void *counters, int bits, double momentum, void *state_copy,
                                             void *stream) {
  cdn::QUpdate qu;
  if (int rc = cdn::tracked_qupdate(&qu, x_min, x_max, state, counters, bits, momentum)) return rc;
  unsigned *copy = static_cast<unsigned *>(state_copy);
  // (up2: x, s are the STORED tensors, H x W the up-sampled resolution -- cdn_codenet_dw_up2_forward's convention)
  if (up2) return dw_up2_forward_impl(x, s, w_dw, d, N, C, H, W, nullptr, stream, &qu, copy);
  return dw_forward_impl(x, s, w_dw, d, N, C, H, W, nullptr, stream, &qu, copy);
}

static int pointwise_forward_impl(const float *d, const float *w_pw, const float *bias, const float *ep_scale,
                                  const float *ep_shift, float *y, int64_t N, int64_t C, int64_t Co, int64_t HW,
                                  int relu, float *partials, void *stream, const void *d_state = nullptr,
                                  int64_t d_pitch = 0, int64_t y_pitch = 0) {
  CDN_REQUIRE(d && w_pw && y, CDN_ERR_ARG, "null tensor pointer");
  if (d_pitch == 0) d_pitch = C * HW;      // (0: a whole tensor)
  if (y_pitch == 0) y_pitch = Co * HW;
  CDN_REQUIRE((ep_scale == nullptr) == (ep_shift == nullptr), CDN_ERR_ARG,
              "ep_scale and ep_shift must both be set or both be NULL");
  CDN_REQUIRE(N > 0 && C > 0 && Co > 0 && HW > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N <= 65535 && C * HW < (1ll << 31) && Co * HW < (1ll << 31) && Co * C < (1ll << 31),
              CDN_ERR_UNSUPPORTED, "shape too large");
  dim3 grid((unsigned)cdn::ceil_div(HW, kPwBN), (unsigned)cdn::ceil_div(Co, kPwBM), (unsigned)N);
  pointwise_kernel<<<grid, 256, 0, cdn::as_stream(stream)>>>(d, w_pw, bias, ep_scale, ep_shift, y,
                                                             (int)C, (int)Co, (int)HW, relu,
                                                             reinterpret_cast<float2 *>(partials),
                                                             static_cast<const unsigned *>(d_state), (long)d_pitch,
                                                             (long)y_pitch);
  return cdn::check_launch("codenet pointwise forward");
}

extern "C" int cdn_codenet_pointwise_forward(const float *d, const float *w_pw, const float *bias,
                                             const float *ep_scale, const float *ep_shift,
                                             float *y, int64_t N, int64_t C, int64_t Co,
                                             int64_t HW, int relu, void *stream) {
  return pointwise_forward_impl(d, w_pw, bias, ep_scale, ep_shift, y, N, C, Co, HW, relu, nullptr, stream);
}

extern "C" int64_t cdn_codenet_pointwise_range_partials(int64_t N, int64_t Co, int64_t HW) {
  return (N > 0 && Co > 0 && HW > 0) ? cdn::ceil_div(HW, kPwBN) * cdn::ceil_div(Co, kPwBM) * N : 0;
}

extern "C" int cdn_codenet_pointwise_forward_range(const float *d, const void *d_state, const float *w_pw,
                                                   const float *bias, const float *ep_scale, const float *ep_shift,
                                                   float *y, int64_t N, int64_t C, int64_t Co, int64_t HW, int relu,
                                                   float *partials, void *stream) {
  CDN_REQUIRE(partials || d_state, CDN_ERR_ARG, "neither partials nor d_state: use cdn_codenet_pointwise_forward");
  return pointwise_forward_impl(d, w_pw, bias, ep_scale, ep_shift, y, N, C, Co, HW, relu, partials, stream, d_state);
}

// The same kernel with d and / or y a channel slice of a wider NCHW tensor, addressed in place through an image pitch
// (the QAT step of the ShuffleNetV2 units: x[:, h:] as input, grad_x[:, h:] as output).  d_state / partials may be NULL.
extern "C" int cdn_codenet_pointwise_forward_pitched(const float *d, int64_t d_image_pitch, const void *d_state,
                                                     const float *w_pw, const float *bias, float *y,
                                                     int64_t y_image_pitch, int64_t N, int64_t C, int64_t Co, int64_t HW,
                                                     int relu, float *partials, void *stream) {
  CDN_REQUIRE(N > 0 && C > 0 && Co > 0 && HW > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(d_image_pitch >= C * HW, CDN_ERR_ARG, "image pitch of d below C * HW");
  CDN_REQUIRE(y_image_pitch >= Co * HW, CDN_ERR_ARG, "image pitch of y below Co * HW");
  CDN_REQUIRE(N * d_image_pitch < (1ll << 31) && N * y_image_pitch < (1ll << 31), CDN_ERR_UNSUPPORTED,
              "shape too large");
  return pointwise_forward_impl(d, w_pw, bias, nullptr, nullptr, y, N, C, Co, HW, relu, partials, stream, d_state,
                                d_image_pitch, y_image_pitch);
}

extern "C" int cdn_codenet_dw_backward_supported(int64_t H, int64_t W) {
  if (H <= 0 || W <= 0 || H > 65535 || W > 65535) return 0;
  const size_t cells = (size_t)(H + 1) * (W + 1);
  if (cells * 2 * 12 + 2 * 9 * 4 + 128 <= (size_t)160 * 1024 - 512) return 1;      // lanes <-> channels kernel
  return (150 * 1024 / 4 - 64) / (2 * (H + 2) * (W + 2) + 18) >= 1;                 // bordered-plane kernel
}

static int dw_backward_impl(const float *x, const float *s, const float *w_dw, const float *grad_d, float *grad_x,
                            float *grad_s, float *grad_w, int64_t N, int64_t C, int64_t H, int64_t W, void *stream,
                            float *part) {
  CDN_REQUIRE(x && s && w_dw && grad_d, CDN_ERR_ARG, "null tensor pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N <= 65535 && N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  hipStream_t st = cdn::as_stream(stream);
  if (grad_s && !part) {
    // (grad_w directly behind grad_s: one fill for both -- a QAT step is made of launches this small)
    const size_t ns = (size_t)(N * H * W), extra = (grad_w == grad_s + ns) ? (size_t)C * 9 : 0;
    hipError_t e = hipMemsetAsync(grad_s, 0, sizeof(float) * (ns + extra), st);
    if (e != hipSuccess) return cdn::fail(CDN_ERR_HIP, "memset grad_s: %s", hipGetErrorString(e));
  }
  // lanes <-> channels kernel: the largest channel chunk whose two LDS images fit; half the chunk when that lets TWO
  // 512-thread workgroups share a CU (16 x 16 planes: 16 channels, 55 KB each): 16 instead of 8 waves per CU hide more
  // of the LDS-atomic latency (QAT step 2.397 -> 2.351 ms) (bwd2_cch)
  const size_t cells = (size_t)(H + 1) * (W + 1);
  const size_t lds_max = 160 * 1024 - 512;
  const int cch = bwd2_cch(H, W, part != nullptr);
  CDN_REQUIRE(cch != 0 || !part, CDN_ERR_UNSUPPORTED, "plane too large for the reproducible backward");
  if (cch != 0) {
    const size_t det_lds = part ? (size_t)cch * 16 * 36 : 0;
    const size_t lds0 = cells * cch * 12 + (size_t)cch * 9 * 4 + 128;
    dim3 grid((unsigned)cdn::ceil_div(C, cch), (unsigned)N);
    // one workgroup per CU (the images of a large plane fill LDS): 16 waves instead of 8 to hide the LDS atomics' latency
#if defined(CDN_BWD_THREADS)
    const int bwd_threads = CDN_BWD_THREADS;
#else
    const int bwd_threads = (lds0 + det_lds) * 2 <= lds_max ? 512 : 1024;
#endif
    const size_t lds = lds0 + (part ? (size_t)(bwd_threads / 64) * cch * 36 : 0);
    // reproducible form: partials into the workspace
    const long plane = (long)(H * W), stride = part ? (long)N * plane : 0;
    float *gs_part = part, *gw_part = part ? part + (size_t)cdn::ceil_div(C, cch) * N * plane : nullptr;
#define CDN_BWD(CCH_)                                                                          \
  {                                                                                            \
    auto kern = dw_bwd2_kernel<CCH_>;                                                          \
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,  \
                              (int)lds);                                                       \
    kern<<<grid, bwd_threads, lds, st>>>(x, s, w_dw, grad_d, grad_x, part ? gs_part : grad_s,  \
                                         part ? gw_part : grad_w, (int)C, (int)H, (int)W, stride); \
  }
    switch (cch) {
      case 32: CDN_BWD(32) break;
      case 16: CDN_BWD(16) break;
      case 8: CDN_BWD(8) break;
      case 4: CDN_BWD(4) break;
      default: CDN_BWD(2) break;
    }
#undef CDN_BWD
    int rc = cdn::check_launch("codenet dw backward");
    if (rc || !part) return rc;
    const long ns = grad_s ? (long)N * plane : 0, nw = grad_w ? (long)C * 9 : 0;
    if (ns + nw == 0) return 0;
    dw_bwd_reduce_kernel<<<(unsigned)(cdn::ceil_div(ns, 256) + cdn::ceil_div(nw, 256)), 256, 0, st>>>(
        gs_part, grad_s, ns, (int)cdn::ceil_div(C, cch), gw_part, grad_w, nw, (int)N);
    return cdn::check_launch("codenet dw backward reduce");
  }
  // fallback for very large planes: lanes <-> pixels kernel with bordered planes
  const int pstride = (int)((H + 2) * (W + 2));
  const int budget = 150 * 1024 / 4;  // floats of LDS per workgroup
  int CC = (budget - 64) / (2 * pstride + 18);
  CDN_REQUIRE(CC >= 1, CDN_ERR_UNSUPPORTED,
              "plane %lldx%lld too large for the LDS-resident backward (use the generic path)",
              (long long)H, (long long)W);
  if (CC > 16) CC = 16;
  if (CC > C) CC = (int)C;
  const size_t lds = (size_t)(2 * ((CC * 9 + 3) & ~3) + 2 * CC * pstride) * sizeof(float);
  dim3 grid((unsigned)cdn::ceil_div(C, CC), (unsigned)N);
  (void)hipFuncSetAttribute((const void *)dw_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)lds);
  dw_bwd_kernel<<<grid, kDwThreads, lds, st>>>(x, s, w_dw, grad_d, grad_x, grad_s, grad_w, (int)C,
                                               (int)H, (int)W, CC);
  return cdn::check_launch("codenet dw backward");
}

extern "C" int cdn_codenet_dw_backward(const float *x, const float *s, const float *w_dw,
                                       const float *grad_d, float *grad_x, float *grad_s,
                                       float *grad_w, int64_t N, int64_t C, int64_t H, int64_t W,
                                       void *stream) {
  return dw_backward_impl(x, s, w_dw, grad_d, grad_x, grad_s, grad_w, N, C, H, W, stream, nullptr);
}

// ---- the REPRODUCIBLE gather backward (round 5) ----------------------------------------------------------------------
// grad_s and grad_w_dw of the two entry points above are float atomics over the channel chunks / the images: equal inputs
// give sums that differ in the last bits from run to run, and with them every parameter of a QAT run after a few steps.
// The _r forms write per-workgroup partials into a caller workspace (every element exactly once, nothing to pre-zero)
// and reduce them in a fixed order: bit-identical results for identical inputs.  grad_x is the 64-bit fixed-point LDS
// sum in both forms (always reproducible).
extern "C" size_t cdn_codenet_dw_backward_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int up2) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535) return 0;
  if (up2) {
    if ((H & 1) || (W & 1)) return 0;
    const int cch = bwd2u_cch(N, C, H / 2, W / 2, true);
    return cch ? bwd_r_bytes(N, C, (H / 2) * (W / 2), cch) : 0;
  }
  const int cch = bwd2_cch(H, W, true);
  return cch ? bwd_r_bytes(N, C, H * W, cch) : 0;
}

extern "C" int cdn_codenet_dw_backward_r(const float *x, const float *s, const float *w_dw, const float *grad_d,
                                         float *grad_x, float *grad_s, float *grad_w, int64_t N, int64_t C, int64_t H,
                                         int64_t W, float *workspace, void *stream) {
  CDN_REQUIRE(workspace, CDN_ERR_ARG, "null workspace (cdn_codenet_dw_backward_workspace_bytes)");
  return dw_backward_impl(x, s, w_dw, grad_d, grad_x, grad_s, grad_w, N, C, H, W, stream, workspace);
}

extern "C" int cdn_codenet_dw_up2_backward_r(const float *x_stored, const float *s_stored, const float *w_dw,
                                             const float *grad_d, float *grad_x, float *grad_s, float *grad_w,
                                             int64_t N, int64_t C, int64_t H, int64_t W, float *workspace,
                                             void *stream) {
  CDN_REQUIRE(workspace, CDN_ERR_ARG, "null workspace (cdn_codenet_dw_backward_workspace_bytes)");
  return dw_up2_backward_impl(x_stored, s_stored, w_dw, grad_d, grad_x, grad_s, grad_w, N, C, H, W, stream, workspace);
}
