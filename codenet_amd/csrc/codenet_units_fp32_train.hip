// codenet_units_fp32_train.hip -- forward and backward of the fp32 ShuffleNetV2 units in training (main.py;
// lib/models/networks/shufflenetv2_dcn.py:57-114), per unit:
//   stride 1:  x1 = x[:, :h] (unchanged)                    x2 = x[:, h:]
//   stride 2:  y4 = dw3x3_s2(x, W4)   z4 = bn4(y4)          y5 = pw(z4, W5)   x1 = relu(bn5(y5))     x2 = x
//   both:      y1 = pw(x2, W1)        a1 = relu(bn1(y1))    y2 = dw3x3_s(a1, W2)   z2 = bn2(y2)
//              y3 = pw(z2, W3)        out[:, 2j] = x1[:, j],  out[:, 2j+1] = relu(bn3(y3))[:, j]
// The dense 1x1 convolutions and their gradients run on the pointwise kernels (the *_pitched entries where an operand is a
// channel slice), the BatchNorm statistics and the pitched second backward pass on the kernels of cdn_bn.h /
// codenet_heads_fp32_train.hip.  Here: the depthwise 3x3 at both strides with BatchNorm1 + ReLU folded into its loads
// (branch 2) or on the raw input (branch 1), BatchNorm without ReLU (z2 / z4, stored: the pointwise kernels read a plain
// tensor), the join (BatchNorm3 / 5 + ReLU + cat + channel_shuffle) and their backward.  Never stored: a1, the unmasked
// grad_a1, grad_y2 / grad_y4 and the outputs of BatchNorm3 / 5 outside `out`.
//
// ---- arithmetic (DESIGN.md section 4.3g is the contract; tests/units_fp32_ref.py restates it in numpy) ------------------
// Whole file under `#pragma clang fp contract(off)`, built with -fno-slp-vectorize, as codenet_heads_fp32_train.hip: every
// float32 operator written here is rounded on its own.
//   a1[q]     = relu_keep_nan(bn_z(y1[q])) inside the plane, 0.0f outside (the convolution's padding -- NOT relu(bn_z(0)))
//   y2[p]     = ((0 + w[0] a[0]) + w[1] a[1]) + .. + w[8] a[8], taps row-major, a[dy][dx] = a1[S p + (dy, dx) - 1]
//   z2        = bn_z(y2)                                     out[:, 2j + slot] = relu_keep_nan(bn_z(y3))[:, j]
//   g_z3      = z3 > 0 ? grad_out[:, 2j + slot] : 0          grad_y3 = head32_bn_bwd2_kernel's expression
//   grad_y2   = ((g_z2 - mb2) - xh2 mg2) (gamma2 invstd2) (training) or g_z2 (gamma2 invstd2) (eval), 0 outside the plane;
//               g_z2 is the pointwise data gradient itself (no ReLU behind a depthwise)
//   grad_a1[q] = sum over the taps t = (dy, dx), row-major from zero, with q + 1 - t = S p for an integer p, of
//               W2[c][t] grad_y2[p] (a tap whose p lies outside the half-resolution plane is a product with 0.0f; a tap of the
//               wrong parity is no term at all)
//   g_z1      = z1 > 0 ? grad_a1 : 0 (branch 2);  grad_x = grad_x + grad_a (branch 1: no mask, added by the pixel's thread)
// ---- the sums ---------------------------------------------------------------------------------------------------------------
// All in float64 (a product of two float32 is exact there), none with atomics, every order a function of the shape alone.
// unit32_bwd1_kernel follows the (channel, slab) protocol of cdn_bn.h: T1 = sum g_z, T2 = sum g_z xh.  unit32_dw_bwd_kernel:
// a workgroup works on a chunk of ONE (n, c) plane of the depthwise INPUT, a thread adds the terms of its own pixels q in
// row-major order -- grad_W[c][t] takes grad_y[p] a[q] from the pixel q = S p + t - 1 --, lanes by the xor tree, waves in
// wave order; the eleven partials [N][C][chunks][11] -- nine taps, T1 = sum g_z1, T2 = sum g_z1 xh1 -- are added in index
// order (images, then chunks) by the finish launch.
#include "cdn_bn.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ BnCh unit32_ch(bool bn, const float *__restrict__ mean, const float *__restrict__ invstd,
                                          const float *__restrict__ gamma, const float *__restrict__ beta, int c) {
  if (bn) return load_ch(mean, invstd, gamma, beta, c);
  BnCh p;
  p.mean = p.invstd = p.gamma = p.beta = 0.0f;
  return p;
}

// ------------------------------------------------------------------------------------------------------
// unit32_dw_fwd_kernel: out [N][C][Ho][Wo] = dw3x3(a, w, stride S, zero padding 1), no bias; the strip layout of
// head32_dw_fwd_kernel on the OUTPUT plane.  The window is 3 rows x 6 (S = 1) or 9 (S = 2) input columns.
// ------------------------------------------------------------------------------------------------------
template <int S, bool BN, bool VIN, bool VOUT>
__global__ void __launch_bounds__(256)
unit32_dw_fwd_kernel(const float *__restrict__ in, long in_pitch, const float *__restrict__ mean,
                     const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
                     const float *__restrict__ w9, float *__restrict__ out, int C, int H, int W, int Ho, int Wo, int wq,
                     int strips, long items) {
  constexpr int NC = S == 1 ? 6 : 9;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= items) return;
  const int q = (int)(idx % wq);
  const long t = idx / wq;
  const int strip = (int)(t % strips);
  const long plane = t / strips;
  const int c = (int)(plane % C);
  const long n = plane / C;
  const int x0 = q * 4, ya = strip * kStripRows, yb = min(Ho, ya + kStripRows);
  const float *src = in + n * in_pitch + (long)c * H * W;
  float *dst = out + plane * Ho * Wo;
  const BnCh p = unit32_ch(BN, mean, invstd, gamma, beta, c);
  float w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = w9[c * 9 + k];
  float a[3][NC];
  load_win<NC, BN, VIN>(src, ya * S - 1, H, W, x0 * S, p, a[0]);
  if (S == 1) load_win<NC, BN, VIN>(src, ya, H, W, x0, p, a[1]);
  for (int y = ya; y < yb; ++y) {
    if (S == 1) {
      load_win<NC, BN, VIN>(src, y + 1, H, W, x0, p, a[2]);
    } else {
      load_win<NC, BN, VIN>(src, 2 * y, H, W, 2 * x0, p, a[1]);
      load_win<NC, BN, VIN>(src, 2 * y + 1, H, W, 2 * x0, p, a[2]);
    }
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float acc = 0.0f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const float pr = w[dy * 3 + dx] * a[dy][i * S + dx];
          acc = acc + pr;
        }
      o[i] = acc;
    }
    cdn::store4<VOUT>(dst + (long)y * Wo, Wo, x0, o);
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      if (S == 1) {
        a[0][j] = a[1][j];
        a[1][j] = a[2][j];
      } else {
        a[0][j] = a[2][j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// unit32_apply_kernel: BatchNorm on a quad of one plane, grid-stride over planes * ceil(HW / 4) quads.
//   JOIN false: z [planes][HW] = bn_z(y)                                                         (z2 / z4)
//   JOIN true:  out [N][2 C][HW]: out[:, 2 c + slot] = relu(bn_z(y [N][C][HW])); x1 != NULL: out[:, 2 c] = x1[:, c] read
//               through x1's image pitch
// ------------------------------------------------------------------------------------------------------
template <bool JOIN, bool VEC>
__global__ void __launch_bounds__(256)
unit32_apply_kernel(const float *__restrict__ y, const float *__restrict__ mean, const float *__restrict__ invstd,
                    const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ out, int slot,
                    const float *__restrict__ x1, long x1_pitch, long planes, int C, int HW) {
  const int hq = (HW + 3) >> 2;
  const long total = planes * hq;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const unsigned plane = (unsigned)i / (unsigned)hq;
    const int p0 = (int)((unsigned)i - plane * (unsigned)hq) * 4;
    const unsigned img = plane / (unsigned)C;
    const int c = (int)(plane - img * (unsigned)C);
    const BnCh p = load_ch(mean, invstd, gamma, beta, c);
    const float *src = y + (long)plane * HW + p0;
    const int cnt = (VEC || HW - p0 > 4) ? 4 : HW - p0;
    float v[4], o[4], pass[4];
    const float *xs = (JOIN && x1) ? x1 + (long)img * x1_pitch + (long)c * HW + p0 : nullptr;
    if (VEC) {
      const float4 t = *reinterpret_cast<const float4 *>(src);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      if (xs) {
        const float4 u = *reinterpret_cast<const float4 *>(xs);
        pass[0] = u.x; pass[1] = u.y; pass[2] = u.z; pass[3] = u.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = e < cnt ? src[e] : 0.0f;
        pass[e] = (xs && e < cnt) ? xs[e] : 0.0f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xh;
      const float z = bn_z(v[e], p, xh);
      o[e] = JOIN ? cdn::relu_keep_nan(z) : z;
    }
    float *dst = JOIN ? out + ((long)img * 2 * C + 2 * c + slot) * HW + p0 : out + (long)plane * HW + p0;
    float *dst0 = JOIN ? out + ((long)img * 2 * C + 2 * c) * HW + p0 : nullptr;
    if (VEC) {
      *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
      if (xs) *reinterpret_cast<float4 *>(dst0) = make_float4(pass[0], pass[1], pass[2], pass[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) {
          dst[e] = o[e];
          if (xs) dst0[e] = pass[e];
        }
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// unit32_bwd1_kernel: the first BatchNorm backward pass of one (channel, slab) (bn_bwd1_kernel's walk).  part [C][slabs][2].
//   JOIN true:  g = grad_out [N][2 C][HW], read at channel 2 c + slot; g_z = z > 0 ? g : 0 is stored ([N][C][HW]); gx1 != NULL:
//               grad_out[:, 2 c] is copied to gx1 + n * gx1_pitch + c * HW (the pass-through half of grad_x)
//   JOIN false: g = grad_z [N][C][HW] is g_z already (BatchNorm without ReLU): only the sums
// ------------------------------------------------------------------------------------------------------
template <bool JOIN, bool VEC>
__global__ void __launch_bounds__(kBnThreads)
unit32_bwd1_kernel(const float *__restrict__ g, const float *__restrict__ y, const float *__restrict__ mean,
                   const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
                   float *__restrict__ gz, int slot, float *__restrict__ gx1, long gx1_pitch, double *__restrict__ part,
                   int C, int HW, long n, int slabs) {
  __shared__ double red[2 * kBnThreads / 64];
  const int c = (int)(blockIdx.x / slabs);
  const long start = (long)(blockIdx.x % slabs) * kBnSlab;
  BnCh p;
  p.mean = mean[c];
  p.invstd = invstd[c];
  p.gamma = JOIN ? gamma[c] : 0.0f;
  p.beta = JOIN ? beta[c] : 0.0f;
  double t1 = 0.0, t2 = 0.0;
#pragma unroll
  for (int it = 0; it < kBnQuads; ++it) {
    const long j0 = start + ((long)it * kBnThreads + threadIdx.x) * 4;
    if (j0 >= n) continue;
    if (VEC) {      // the quad lies in one plane
      const unsigned img = (unsigned)j0 / (unsigned)HW;
      const int pix = (int)((unsigned)j0 - img * (unsigned)HW);
      const long off = ((long)img * C + c) * HW + pix;
      const long goff = JOIN ? ((long)img * 2 * C + 2 * c + slot) * HW + pix : off;
      const float4 t = *reinterpret_cast<const float4 *>(y + off);
      const float4 a = *reinterpret_cast<const float4 *>(g + goff);
      const float v[4] = {t.x, t.y, t.z, t.w}, G[4] = {a.x, a.y, a.z, a.w};
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float xh;
        const float z = bn_z(v[e], p, xh);
        o[e] = JOIN ? (z > 0.0f ? G[e] : 0.0f) : G[e];
        t1 = t1 + (double)o[e];
        t2 = t2 + (double)o[e] * (double)xh;
      }
      if (JOIN) {
        *reinterpret_cast<float4 *>(gz + off) = make_float4(o[0], o[1], o[2], o[3]);
        if (gx1)
          *reinterpret_cast<float4 *>(gx1 + (long)img * gx1_pitch + (long)c * HW + pix) =
              *reinterpret_cast<const float4 *>(g + ((long)img * 2 * C + 2 * c) * HW + pix);
      }
    } else {
      const int cnt = n - j0 < 4 ? (int)(n - j0) : 4;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) {
          const unsigned img = (unsigned)(j0 + e) / (unsigned)HW;
          const int pix = (int)((unsigned)(j0 + e) - img * (unsigned)HW);
          const long off = ((long)img * C + c) * HW + pix;
          const float Ge = g[JOIN ? ((long)img * 2 * C + 2 * c + slot) * HW + pix : off];
          float xh;
          const float z = bn_z(y[off], p, xh);
          const float o = JOIN ? (z > 0.0f ? Ge : 0.0f) : Ge;
          t1 = t1 + (double)o;
          t2 = t2 + (double)o * (double)xh;
          if (JOIN) {
            gz[off] = o;
            if (gx1) gx1[(long)img * gx1_pitch + (long)c * HW + pix] = g[((long)img * 2 * C + 2 * c) * HW + pix];
          }
        }
    }
  }
  cdn::block_sums_store({t1, t2}, red, part);
}

// The terms of one row of a thread's strip: the four pixels x0 .. x0 + 3 of an input row.  gK: the window row of grad_y
// that tap row dy = K reads, DK: whether that tap row lands on an output row (stride 2: by the parity of the input row).
// Window column of tap (i, dx): i + 2 - dx (S = 1, the window starts at column x0 - 1) or (i + 1 - dx) / 2 where that is an
// integer (S = 2, the window starts at column x0 / 2).
template <int S, bool D0, bool D1, bool D2, int NG>
__device__ __forceinline__ void unit32_bwd_row(const float (&g0)[NG], const float (&g1)[NG], const float (&g2)[NG],
                                               const float (&w)[9], const float (&a)[4], int x0, int W,
                                               double (&sums)[kDwSums], float (&ga)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float acc = 0.0f;
    const bool live = x0 + i < W;
    const double ad = (double)a[i];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      if (!(dy == 0 ? D0 : dy == 1 ? D1 : D2)) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        if ((i + 1 - dx) % S != 0) continue;
        const int j = S == 1 ? i + 2 - dx : (i + 1 - dx) / 2;
        const float gv = dy == 0 ? g0[j] : dy == 1 ? g1[j] : g2[j];
        const float pr = w[dy * 3 + dx] * gv;
        acc = acc + pr;
        if (live) sums[dy * 3 + dx] = sums[dy * 3 + dx] + (double)gv * ad;
      }
    }
    ga[i] = acc;
  }
}

// ------------------------------------------------------------------------------------------------------
// unit32_dw_bwd_kernel: the backward of the depthwise 3x3 (a workgroup works on chunk blockIdx.x % chunks of the strips of
// ONE (n, c) plane of the depthwise INPUT, H x W; gz / y are the [N][C][Ho][Wo] tensors behind it).
//   grad_y formed while loading gz and y (SUB: batch statistics of the BatchNorm behind; !SUB: eval mode), 0 outside
//   BN:  in = y1, a = relu(bn_z(in)); gin [N][C][H][W] (pitched) = g_z1 = z1 > 0 ? grad_a : 0; T1, T2 of BatchNorm1
//   !BN: in = x as it is; gin (may be NULL) = gin + grad_a (acc) or grad_a
//   part [N][C][chunks][11]
// ------------------------------------------------------------------------------------------------------
template <int S, bool BN, bool SUB, bool VI, bool VO>
__global__ void __launch_bounds__(256)
unit32_dw_bwd_kernel(const float *__restrict__ gz, const float *__restrict__ y, const float *__restrict__ mean2,
                     const float *__restrict__ invstd2, const float *__restrict__ gamma2, const float *__restrict__ mb2,
                     const float *__restrict__ mg2, const float *__restrict__ in, long in_pitch,
                     const float *__restrict__ mean1, const float *__restrict__ invstd1, const float *__restrict__ gamma1,
                     const float *__restrict__ beta1, const float *__restrict__ w9, float *gin, long gin_pitch, int acc,
                     double *__restrict__ part, int C, int H, int W, int Ho, int Wo, int wq, int strips, int chunks) {
  constexpr int NG = S == 1 ? 6 : 3;
  __shared__ double red[4 * kDwSums];
  const int chunk = (int)(blockIdx.x % chunks);
  const long plane = blockIdx.x / chunks;
  const int c = (int)(plane % C);
  const long n = plane / C;
  const int item = chunk * (int)blockDim.x + (int)threadIdx.x;
  double sums[kDwSums];
#pragma unroll
  for (int k = 0; k < kDwSums; ++k) sums[k] = 0.0;
  if (item < wq * strips) {
    const int x0 = (item % wq) * 4, ya = (item / wq) * kStripRows, yb = min(H, ya + kStripRows);
    const float *gsrc = gz + plane * Ho * Wo, *ysrc = y + plane * Ho * Wo;
    const float *isrc = in + n * in_pitch + (long)c * H * W;
    float *dst = gin ? gin + n * gin_pitch + (long)c * H * W : nullptr;
    const BnCh p1 = unit32_ch(BN, mean1, invstd1, gamma1, beta1, c);
    const BnBwd2 q2 = load_bwd2<SUB>(mean2, invstd2, gamma2, mb2, mg2, c);
    float w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = w9[c * 9 + k];
    // one window row of grad_y (bn_grad_y), zeros outside the plane
    auto load_g = [&](int yo, float (&gr)[NG]) {
      float gv[NG], yv[NG];
      unsigned ok = 0u;
      if (S == 1) {
        ok = cdn::load_cols<NG, 1, VO>(gsrc, yo, Ho, Wo, x0, gv);
        if (SUB) cdn::load_cols<NG, 1, VO>(ysrc, yo, Ho, Wo, x0, yv);
      } else {
#pragma unroll
        for (int j = 0; j < NG; ++j) {
          const int xo = x0 / 2 + j;
          const bool inside = yo >= 0 && yo < Ho && xo < Wo;
          gv[j] = inside ? gsrc[(long)yo * Wo + xo] : 0.0f;
          yv[j] = (SUB && inside) ? ysrc[(long)yo * Wo + xo] : 0.0f;
          ok |= inside ? (1u << j) : 0u;
        }
      }
#pragma unroll
      for (int j = 0; j < NG; ++j) gr[j] = ((ok >> j) & 1u) ? bn_grad_y<SUB>(gv[j], SUB ? yv[j] : 0.0f, q2) : 0.0f;
    };
    // the thread's own four pixels of input row Y: a, the mask z > 0 and xh (BN) or the stored values
    float a[4], xh[4], ga[4];
    unsigned pos = 0u;
    auto load_own = [&](int Y) {
      float v[4];
      const float *row = isrc + (long)Y * W + x0;
      if (VI) {
        const float4 t = *reinterpret_cast<const float4 *>(row);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = x0 + i < W ? row[i] : 0.0f;
      }
      pos = 0u;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (BN) {
          const float z = bn_z(v[i], p1, xh[i]);
          a[i] = cdn::relu_keep_nan(z);
          pos |= z > 0.0f ? (1u << i) : 0u;
        } else {
          a[i] = v[i];
          xh[i] = 0.0f;
        }
      }
    };
    auto store_own = [&](int Y) {
      float o[4];
      if (BN) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          o[i] = ((pos >> i) & 1u) ? ga[i] : 0.0f;
          if (x0 + i < W) {
            sums[9] = sums[9] + (double)o[i];
            sums[10] = sums[10] + (double)o[i] * (double)xh[i];
          }
        }
      } else {
        if (!dst) return;
        float old[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (acc) {
          const float *row = dst + (long)Y * W + x0;
          if (VI) {
            const float4 t = *reinterpret_cast<const float4 *>(row);
            old[0] = t.x; old[1] = t.y; old[2] = t.z; old[3] = t.w;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) old[i] = x0 + i < W ? row[i] : 0.0f;
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = acc ? old[i] + ga[i] : ga[i];
      }
      cdn::store4<VI>(dst + (long)Y * W, W, x0, o);
    };
    if (S == 1) {
      float gw[3][NG];
      load_g(ya - 1, gw[0]);
      load_g(ya, gw[1]);
      for (int Y = ya; Y < yb; ++Y) {
        load_g(Y + 1, gw[2]);
        load_own(Y);
        unit32_bwd_row<S, true, true, true, NG>(gw[2], gw[1], gw[0], w, a, x0, W, sums, ga);
        store_own(Y);
#pragma unroll
        for (int j = 0; j < NG; ++j) {
          gw[0][j] = gw[1][j];
          gw[1][j] = gw[2][j];
        }
      }
    } else {
      // input rows in (even, odd) pairs: the even row 2 ye reads output row ye (tap row 1), the odd row 2 ye + 1 reads
      // output rows ye + 1 (tap row 0) and ye (tap row 2)
      float G0[NG], G1[NG];
      load_g(ya / 2, G0);
      for (int Y = ya; Y < yb; Y += 2) {
        load_own(Y);
        unit32_bwd_row<S, false, true, false, NG>(G0, G0, G0, w, a, x0, W, sums, ga);
        store_own(Y);
        load_g(Y / 2 + 1, G1);
        if (Y + 1 < yb) {
          load_own(Y + 1);
          unit32_bwd_row<S, true, false, true, NG>(G1, G0, G0, w, a, x0, W, sums, ga);
          store_own(Y + 1);
        }
#pragma unroll
        for (int j = 0; j < NG; ++j) G0[j] = G1[j];
      }
    }
  }
  cdn::block_sums_store(sums, red, part);
}

// a channel slice [N][C][H][W] of a wider tensor behind an image pitch
int unit32_check_pitch(int64_t pitch, int64_t N, int64_t C, int64_t H, int64_t W, const char *what) {
  CDN_REQUIRE(pitch >= C * H * W, CDN_ERR_ARG, "image pitch of %s below C * H * W", what);
  CDN_REQUIRE(N * pitch < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  return CDN_OK;
}

size_t unit32_ws_bytes(int64_t N, int64_t C, int64_t H, int64_t W) {
  const size_t slabs = (size_t)cdn::ceil_div(N * H * W, kBnSlab);
  const size_t bn = (size_t)C * slabs * 2 * sizeof(double);
  return cdn::round256(std::max(bn, dw_part_bytes(N, C, H, W)));
}

bool unit32_stride_ok(int stride) { return stride == 1 || stride == 2; }

}  // namespace

extern "C" size_t cdn_codenet_unit_fp32_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return unit32_ws_bytes(N, C, H, W);
}

extern "C" int cdn_codenet_unit_fp32_dw_forward(const float *in, int64_t in_image_pitch, const float *mean,
                                                const float *invstd, const float *gamma, const float *beta, const float *w,
                                                float *out, int64_t N, int64_t C, int64_t H, int64_t W, int stride,
                                                void *stream) {
  CDN_REQUIRE(in && w && out, CDN_ERR_ARG, "null pointer");
  const bool bn = mean != nullptr;
  CDN_REQUIRE(bn ? (invstd && gamma && beta) : (!invstd && !gamma && !beta), CDN_ERR_ARG,
              "mean, invstd, gamma, beta: all four or none");
  CDN_REQUIRE(unit32_stride_ok(stride), CDN_ERR_ARG, "stride must be 1 or 2, got %d", stride);
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  if (int rc = unit32_check_pitch(in_image_pitch, N, C, H, W, "in")) return rc;
  const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const StripPlan p = strip_plan(Ho, Wo);
  const long items = (long)(N * C) * p.strips * p.wq;
  const unsigned grid = (unsigned)cdn::ceil_div(items, 256);
  const bool vin = (W & 3) == 0 && (in_image_pitch & 3) == 0 && cdn::aligned16(in);
  const bool vout = (Wo & 3) == 0 && cdn::aligned16(out);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_U32FWD(S, BN, VI, VO)                                                                                             \
  unit32_dw_fwd_kernel<S, BN, VI, VO><<<grid, 256, 0, st>>>(in, (long)in_image_pitch, mean, invstd, gamma, beta, w, out,     \
                                                            (int)C, (int)H, (int)W, (int)Ho, (int)Wo, p.wq, p.strips, items)
#define CDN_U32FWD_V(S, BN)                                                                                                   \
  if (vin && vout) CDN_U32FWD(S, BN, true, true);                                                                             \
  else if (vin) CDN_U32FWD(S, BN, true, false);                                                                               \
  else if (vout) CDN_U32FWD(S, BN, false, true);                                                                              \
  else CDN_U32FWD(S, BN, false, false)
  if (stride == 1) {
    if (bn) { CDN_U32FWD_V(1, true); } else { CDN_U32FWD_V(1, false); }
  } else {
    if (bn) { CDN_U32FWD_V(2, true); } else { CDN_U32FWD_V(2, false); }
  }
#undef CDN_U32FWD_V
#undef CDN_U32FWD
  return cdn::check_launch("codenet unit fp32 depthwise forward");
}

extern "C" int cdn_codenet_unit_fp32_bn_forward(const float *y, const float *mean, const float *invstd, const float *gamma,
                                                const float *beta, float *z, int64_t N, int64_t C, int64_t H, int64_t W,
                                                void *stream) {
  CDN_REQUIRE(y && mean && invstd && gamma && beta && z, CDN_ERR_ARG, "null pointer");
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  const int64_t HW = H * W;
  const unsigned grid = rows_grid((long)(N * C), HW);
  hipStream_t st = cdn::as_stream(stream);
  if ((HW & 3) == 0 && cdn::aligned16(y) && cdn::aligned16(z))
    unit32_apply_kernel<false, true><<<grid, 256, 0, st>>>(y, mean, invstd, gamma, beta, z, 0, nullptr, 0, (long)(N * C), (int)C,
                                                           (int)HW);
  else
    unit32_apply_kernel<false, false><<<grid, 256, 0, st>>>(y, mean, invstd, gamma, beta, z, 0, nullptr, 0, (long)(N * C),
                                                            (int)C, (int)HW);
  return cdn::check_launch("codenet unit fp32 BatchNorm forward");
}

extern "C" int cdn_codenet_unit_fp32_join_forward(const float *y, const float *mean, const float *invstd, const float *gamma,
                                                  const float *beta, float *out, int slot, const float *x1,
                                                  int64_t x1_image_pitch, int64_t N, int64_t h, int64_t H, int64_t W,
                                                  void *stream) {
  CDN_REQUIRE(y && mean && invstd && gamma && beta && out, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(slot == 0 || slot == 1, CDN_ERR_ARG, "slot must be 0 or 1, got %d", slot);
  CDN_REQUIRE(!x1 || slot == 1, CDN_ERR_ARG, "the pass-through half goes with slot 1");
  if (int rc = train32_check_shape(N, 2 * h, H, W)) return rc;
  if (x1)
    if (int rc = unit32_check_pitch(x1_image_pitch, N, h, H, W, "x1")) return rc;
  const int64_t HW = H * W;
  const unsigned grid = rows_grid((long)(N * h), HW);
  const bool vec = (HW & 3) == 0 && cdn::aligned16(y) && cdn::aligned16(out) &&
                   (!x1 || (cdn::aligned16(x1) && (x1_image_pitch & 3) == 0));
  hipStream_t st = cdn::as_stream(stream);
  if (vec)
    unit32_apply_kernel<true, true><<<grid, 256, 0, st>>>(y, mean, invstd, gamma, beta, out, slot, x1, (long)x1_image_pitch,
                                                          (long)(N * h), (int)h, (int)HW);
  else
    unit32_apply_kernel<true, false><<<grid, 256, 0, st>>>(y, mean, invstd, gamma, beta, out, slot, x1, (long)x1_image_pitch,
                                                           (long)(N * h), (int)h, (int)HW);
  return cdn::check_launch("codenet unit fp32 join forward");
}

extern "C" int cdn_codenet_unit_fp32_join_backward(const float *grad_out, const float *y, const float *mean,
                                                   const float *invstd, const float *gamma, const float *beta, float *g_z,
                                                   float *grad_gamma, float *grad_beta, float *mb, float *mg, int slot,
                                                   float *grad_x1, int64_t grad_x1_image_pitch, int64_t N, int64_t h,
                                                   int64_t H, int64_t W, void *workspace, size_t workspace_bytes,
                                                   void *stream) {
  CDN_REQUIRE(grad_out && y && mean && invstd && gamma && beta && g_z && grad_gamma && grad_beta && mb && mg && workspace,
              CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(slot == 0 || slot == 1, CDN_ERR_ARG, "slot must be 0 or 1, got %d", slot);
  CDN_REQUIRE(!grad_x1 || slot == 1, CDN_ERR_ARG, "the pass-through half goes with slot 1");
  if (int rc = train32_check_shape(N, 2 * h, H, W)) return rc;
  if (grad_x1)
    if (int rc = unit32_check_pitch(grad_x1_image_pitch, N, h, H, W, "grad_x1")) return rc;
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, unit32_ws_bytes(N, h, H, W))) return rc;
  const BnPlan p = bn_plan(N, h, H, W);
  double *part = static_cast<double *>(workspace);
  const unsigned grid = (unsigned)(h * p.slabs);
  const int64_t HW = H * W;
  const bool vec = (HW & 3) == 0 && cdn::aligned16(grad_out) && cdn::aligned16(y) && cdn::aligned16(g_z) &&
                   (!grad_x1 || (cdn::aligned16(grad_x1) && (grad_x1_image_pitch & 3) == 0));
  hipStream_t st = cdn::as_stream(stream);
  if (vec)
    unit32_bwd1_kernel<true, true><<<grid, kBnThreads, 0, st>>>(grad_out, y, mean, invstd, gamma, beta, g_z, slot, grad_x1,
                                                                (long)grad_x1_image_pitch, part, (int)h, (int)HW, p.n, p.slabs);
  else
    unit32_bwd1_kernel<true, false><<<grid, kBnThreads, 0, st>>>(grad_out, y, mean, invstd, gamma, beta, g_z, slot, grad_x1,
                                                                 (long)grad_x1_image_pitch, part, (int)h, (int)HW, p.n, p.slabs);
  launch_bn_bwd_finish(part, grad_gamma, grad_beta, mb, mg, h, p, st);
  return cdn::check_launch("codenet unit fp32 join backward");
}

extern "C" int cdn_codenet_unit_fp32_bn_backward_sums(const float *grad_z, const float *y, const float *mean,
                                                      const float *invstd, float *grad_gamma, float *grad_beta, float *mb,
                                                      float *mg, int64_t N, int64_t C, int64_t H, int64_t W, void *workspace,
                                                      size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(grad_z && y && mean && invstd && grad_gamma && grad_beta && mb && mg && workspace, CDN_ERR_ARG, "null pointer");
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, unit32_ws_bytes(N, C, H, W))) return rc;
  const BnPlan p = bn_plan(N, C, H, W);
  double *part = static_cast<double *>(workspace);
  const unsigned grid = (unsigned)(C * p.slabs);
  const int64_t HW = H * W;
  hipStream_t st = cdn::as_stream(stream);
  if ((HW & 3) == 0 && cdn::aligned16(grad_z) && cdn::aligned16(y))
    unit32_bwd1_kernel<false, true><<<grid, kBnThreads, 0, st>>>(grad_z, y, mean, invstd, nullptr, nullptr, nullptr, 0, nullptr,
                                                                 0, part, (int)C, (int)HW, p.n, p.slabs);
  else
    unit32_bwd1_kernel<false, false><<<grid, kBnThreads, 0, st>>>(grad_z, y, mean, invstd, nullptr, nullptr, nullptr, 0, nullptr,
                                                                  0, part, (int)C, (int)HW, p.n, p.slabs);
  launch_bn_bwd_finish(part, grad_gamma, grad_beta, mb, mg, C, p, st);
  return cdn::check_launch("codenet unit fp32 BatchNorm backward sums");
}

extern "C" int cdn_codenet_unit_fp32_dw_backward(const float *grad_z, const float *y, const float *mean2, const float *invstd2,
                                                 const float *gamma2, const float *mb2, const float *mg2, int training2,
                                                 const float *in, int64_t in_image_pitch, const float *mean1,
                                                 const float *invstd1, const float *gamma1, const float *beta1, const float *w,
                                                 float *grad_in, int64_t grad_in_image_pitch, int accumulate, float *grad_w,
                                                 float *grad_gamma1, float *grad_beta1, float *mb1, float *mg1, int64_t N,
                                                 int64_t C, int64_t H, int64_t W, int stride, void *workspace,
                                                 size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(grad_z && y && mean2 && invstd2 && gamma2 && (!training2 || (mb2 && mg2)) && in && w && grad_w && workspace,
              CDN_ERR_ARG, "null pointer");
  const bool bn = mean1 != nullptr;
  if (bn)
    CDN_REQUIRE(invstd1 && gamma1 && beta1 && grad_in && grad_gamma1 && grad_beta1 && mb1 && mg1 && !accumulate, CDN_ERR_ARG,
                "BatchNorm1 given: invstd1, gamma1, beta1, grad_in and its four results are needed, accumulate must be 0");
  else
    CDN_REQUIRE(!invstd1 && !gamma1 && !beta1 && !grad_gamma1 && !grad_beta1 && !mb1 && !mg1, CDN_ERR_ARG,
                "no BatchNorm1: its operands and results must all be NULL");
  CDN_REQUIRE(unit32_stride_ok(stride), CDN_ERR_ARG, "stride must be 1 or 2, got %d", stride);
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  if (int rc = unit32_check_pitch(in_image_pitch, N, C, H, W, "in")) return rc;
  if (grad_in)
    if (int rc = unit32_check_pitch(grad_in_image_pitch, N, C, H, W, "grad_in")) return rc;
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, unit32_ws_bytes(N, C, H, W))) return rc;
  const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const StripPlan p = strip_plan(H, W);
  const bool vi = (W & 3) == 0 && (in_image_pitch & 3) == 0 && cdn::aligned16(in) &&
                  (!grad_in || ((grad_in_image_pitch & 3) == 0 && cdn::aligned16(grad_in)));
  const bool vo = stride == 1 && (Wo & 3) == 0 && cdn::aligned16(grad_z) && cdn::aligned16(y);
  const unsigned grid = (unsigned)(N * C * p.chunks);
  double *part = static_cast<double *>(workspace);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_U32BWD(S, BN, SUB, VI, VO)                                                                                        \
  unit32_dw_bwd_kernel<S, BN, SUB, VI, VO><<<grid, p.threads, 0, st>>>(                                                       \
      grad_z, y, mean2, invstd2, gamma2, mb2, mg2, in, (long)in_image_pitch, mean1, invstd1, gamma1, beta1, w, grad_in,       \
      (long)grad_in_image_pitch, accumulate, part, (int)C, (int)H, (int)W, (int)Ho, (int)Wo, p.wq, p.strips, p.chunks)
#define CDN_U32BWD_V(S, BN, SUB)                                                                                              \
  if (S == 1) {                                                                                                               \
    if (vi && vo) CDN_U32BWD(S, BN, SUB, true, true);                                                                         \
    else if (vi) CDN_U32BWD(S, BN, SUB, true, false);                                                                         \
    else if (vo) CDN_U32BWD(S, BN, SUB, false, true);                                                                         \
    else CDN_U32BWD(S, BN, SUB, false, false);                                                                                \
  } else {                                                                                                                    \
    if (vi) CDN_U32BWD(S, BN, SUB, true, false);                                                                              \
    else CDN_U32BWD(S, BN, SUB, false, false);                                                                                \
  }
#define CDN_U32BWD_M(S)                                                                                                       \
  if (bn) {                                                                                                                   \
    if (training2) { CDN_U32BWD_V(S, true, true) } else { CDN_U32BWD_V(S, true, false) }                                      \
  } else {                                                                                                                    \
    if (training2) { CDN_U32BWD_V(S, false, true) } else { CDN_U32BWD_V(S, false, false) }                                    \
  }
  if (stride == 1) { CDN_U32BWD_M(1) } else { CDN_U32BWD_M(2) }
#undef CDN_U32BWD_M
#undef CDN_U32BWD_V
#undef CDN_U32BWD
  dw_bwd_finish_kernel<<<(unsigned)cdn::ceil_div(C * kDwSums, 256), 256, 0, st>>>(
      part, grad_w, grad_gamma1, grad_beta1, mb1, mg1, (int)N, (int)C, p.chunks, (long)(N * H * W));
  return cdn::check_launch("codenet unit fp32 depthwise backward");
}
