// codenet_heads_fp32_train.hip -- forward and backward of the fp32 detection heads in training (main.py;
// lib/models/networks/shufflenetv2_dcn.py:246-258):
//   y1 = conv1x1(x, W1)            a1 = relu(bn1(y1))
//   y2 = dw3x3(a1, W2), pad 1      a2 = relu(bn2(y2))
//   y3 = conv1x1(a2, W3) + b3
// The dense 1x1 convolutions and their gradients run on the pointwise kernels of codenet_stage.hip / codenet_train.hip, the
// BatchNorm statistics, the stored a2 of a wide head (hm) and the first backward pass behind it on the kernels of cdn_bn.h.
// Here: the depthwise 3x3 with BatchNorm1 + ReLU folded into its loads, the last conv of a head with at most four output
// channels (wh, reg) with BatchNorm2 + ReLU folded into its loads, and their backward.  Never stored: a1, grad_y2, the
// unmasked grad_a1 and, for the narrow heads, a2 and grad_a2.
//
// ---- arithmetic (DESIGN.md section 4.3f is the contract; tests/heads_fp32_ref.py restates it in numpy) -----------------
// Whole file under `#pragma clang fp contract(off)`, built with -fno-slp-vectorize, as codenet_bn_train.hip: every float32
// operator written here is rounded on its own.
//   a1[q]     = relu_keep_nan(bn_z(y1[q])) inside the plane, 0.0f outside (the convolution's padding -- NOT relu(bn_z(0)))
//   y2        = ((0 + w[0] a[0]) + w[1] a[1]) + .. + w[8] a[8], taps row-major
//   y3[o]     = (sum_c W3[o][c] a2[c]) + b3[o], c ascending from zero, a2 = relu_keep_nan(bn_z(y2))          (Co <= 4)
//   grad_a2   = W3[0][c] g[0] (+ W3[o][c] g[o], o ascending);  g_z2 = z2 > 0 ? grad_a2 : 0                   (Co <= 4)
//   grad_y2   = ((g_z2 - mb2) - xh2 mg2) (gamma2 invstd2) (training) or g_z2 (gamma2 invstd2) (eval), 0 outside the plane
//   grad_a1[q] = sum_t W2[c][t] grad_y2[q - t] from zero in the loop order of head_dw_bwd_kernel; g_z1 = z1 > 0 ? grad_a1 : 0
//   grad_y1   = bn_bwd2_kernel's expression, written through an image pitch
// ---- the sums ---------------------------------------------------------------------------------------------------------------
// All in float64 (a product of two float32 is exact there), none with atomics, every order a function of the shape alone.
// head32_tail_bwd_kernel follows the (channel, slab) protocol of cdn_bn.h with 2 + 2 Co sums per workgroup: T1 = sum g_z2,
// T2 = sum g_z2 xh2, grad_W3[o][c] = sum g[o] a2 and sum g[o] (grad_b3: every channel's workgroups form it, channel 0's is
// stored).  head32_dw_bwd_kernel: a workgroup works on a chunk of ONE (n, c) plane, a thread adds its own pixels in row-major
// order, lanes by the xor tree, waves in wave order; the eleven partials [N][C][chunks][11] -- nine taps of grad_W2, T1 =
// sum g_z1, T2 = sum g_z1 xh1 -- are added in index order (images, then chunks) by the finish launch.
#include "cdn_bn.h"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------------
// head32_dw_fwd_kernel: y2 = dw3x3(relu(bn1(y1)), w2), zero padding 1, no bias; the strip layout of head_dw_fwd_kernel.
// ------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256)
head32_dw_fwd_kernel(const float *__restrict__ y1, const float *__restrict__ mean, const float *__restrict__ invstd,
                     const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ w2,
                     float *__restrict__ y2, int C, int H, int W, int wq, int strips, long items) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= items) return;
  const int q = (int)(idx % wq);
  const long t = idx / wq;
  const int strip = (int)(t % strips);
  const long plane = t / strips;
  const int c = (int)(plane % C);
  const int x0 = q * 4, ya = strip * kStripRows, yb = min(H, ya + kStripRows);
  const float *src = y1 + plane * H * W;
  float *dst = y2 + plane * H * W;
  const BnCh p = load_ch(mean, invstd, gamma, beta, c);
  float w[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) w[k] = w2[c * 9 + k];
  float a[3][6];
  load_win<6, true, VEC>(src, ya - 1, H, W, x0, p, a[0]);
  load_win<6, true, VEC>(src, ya, H, W, x0, p, a[1]);
  for (int y = ya; y < yb; ++y) {
    load_win<6, true, VEC>(src, y + 1, H, W, x0, p, a[2]);
    float out[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float acc = 0.0f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const float pr = w[dy * 3 + dx] * a[dy][i + dx];
          acc = acc + pr;
        }
      out[i] = acc;
    }
    cdn::store4<VEC>(dst + (long)y * W, W, x0, out);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      a[0][j] = a[1][j];
      a[1][j] = a[2][j];
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// head32_tail_fwd_kernel: y3 = W3 . relu(bn2(y2)) + b3 for CO <= 4 output channels on the VALU, y2 read once, a2 never
// stored.  A thread owns four consecutive pixels of one image and walks the input channels in ascending order.
// ------------------------------------------------------------------------------------------------------
template <int CO, bool VEC>
__global__ void __launch_bounds__(256)
head32_tail_fwd_kernel(const float *__restrict__ y2, const float *__restrict__ mean, const float *__restrict__ invstd,
                       const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ w3,
                       const float *__restrict__ b3, float *__restrict__ y3, int C, int HW, int hq, long items) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= items) return;
  const long n = idx / hq;
  const int p0 = (int)(idx % hq) * 4;
  const float *src = y2 + n * C * HW + p0;
  float acc[CO][4];
#pragma unroll
  for (int o = 0; o < CO; ++o)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[o][e] = 0.0f;
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    const BnCh p = load_ch(mean, invstd, gamma, beta, c);
    float v[4];
    if (VEC) {
      const float4 u = *reinterpret_cast<const float4 *>(src + (long)c * HW);
      v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (p0 + e < HW) ? src[(long)c * HW + e] : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xh;
      const float a = cdn::relu_keep_nan(bn_z(v[e], p, xh));
#pragma unroll
      for (int o = 0; o < CO; ++o) {
        const float pr = w3[o * C + c] * a;
        acc[o][e] = acc[o][e] + pr;
      }
    }
  }
#pragma unroll
  for (int o = 0; o < CO; ++o) {
    const float b = b3 ? b3[o] : 0.0f;
    float *dst = y3 + (n * CO + o) * HW + p0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (b3) acc[o][e] = acc[o][e] + b;      // (no bias: the sum as it is, a -0.0 kept)
    if (VEC) {
      *reinterpret_cast<float4 *>(dst) = make_float4(acc[o][0], acc[o][1], acc[o][2], acc[o][3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < HW) dst[e] = acc[o][e];
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// head32_tail_bwd_kernel: the backward of the narrow tail and the first BatchNorm2 pass, one (channel, slab) per workgroup
// (bn_bwd1_kernel's walk).  g: grad_y3 [N][CO][H][W].  Stores g_z2; part [C][slabs][2 + 2 CO]: T1, T2, grad_W3[o][c] (o
// ascending), sum g[o] (o ascending).
// ------------------------------------------------------------------------------------------------------
template <int CO, bool VEC>
__global__ void __launch_bounds__(kBnThreads)
head32_tail_bwd_kernel(const float *__restrict__ g, const float *__restrict__ y2, const float *__restrict__ mean,
                       const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
                       const float *__restrict__ w3, float *__restrict__ gz, double *__restrict__ part, int C, int HW, long n,
                       int slabs) {
  constexpr int K = 2 + 2 * CO;
  __shared__ double red[K * kBnThreads / 64];
  const int c = (int)(blockIdx.x / slabs);
  const long start = (long)(blockIdx.x % slabs) * kBnSlab;
  const BnCh p = load_ch(mean, invstd, gamma, beta, c);
  float w3c[CO];
#pragma unroll
  for (int o = 0; o < CO; ++o) w3c[o] = w3[o * C + c];
  double sums[K];
#pragma unroll
  for (int k = 0; k < K; ++k) sums[k] = 0.0;
#pragma unroll
  for (int it = 0; it < kBnQuads; ++it) {
    const long j0 = start + ((long)it * kBnThreads + threadIdx.x) * 4;
    if (j0 >= n) continue;
    float v[4], G[CO][4], o4[4];
    int cnt = 4;
    if (VEC) {      // the quad lies in one row
      const float4 t = *reinterpret_cast<const float4 *>(y2 + ch_offset(j0, c, C, HW));
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
#pragma unroll
      for (int o = 0; o < CO; ++o) {
        const float4 a = *reinterpret_cast<const float4 *>(g + ch_offset(j0, o, CO, HW));
        G[o][0] = a.x; G[o][1] = a.y; G[o][2] = a.z; G[o][3] = a.w;
      }
    } else {
      cnt = n - j0 < 4 ? (int)(n - j0) : 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = e < cnt ? y2[ch_offset(j0 + e, c, C, HW)] : 0.0f;
#pragma unroll
        for (int o = 0; o < CO; ++o) G[o][e] = e < cnt ? g[ch_offset(j0 + e, o, CO, HW)] : 0.0f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xh;
      const float z = bn_z(v[e], p, xh);
      float ga = w3c[0] * G[0][e];
#pragma unroll
      for (int o = 1; o < CO; ++o) {
        const float pr = w3c[o] * G[o][e];
        ga = ga + pr;
      }
      o4[e] = z > 0.0f ? ga : 0.0f;
      if (e < cnt) {
        const double a2 = (double)cdn::relu_keep_nan(z);
        sums[0] = sums[0] + (double)o4[e];
        sums[1] = sums[1] + (double)o4[e] * (double)xh;
#pragma unroll
        for (int o = 0; o < CO; ++o) {
          sums[2 + o] = sums[2 + o] + (double)G[o][e] * a2;
          sums[2 + CO + o] = sums[2 + CO + o] + (double)G[o][e];
        }
      }
    }
    if (VEC) {
      *reinterpret_cast<float4 *>(gz + ch_offset(j0, c, C, HW)) = make_float4(o4[0], o4[1], o4[2], o4[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) gz[ch_offset(j0 + e, c, C, HW)] = o4[e];
    }
  }
  cdn::block_sums_store(sums, red, part);
}

// one thread per channel: adds the slabs' partials in slab order; grad_gamma2, grad_beta2, the two means of the second
// pass, the channel's column of grad_W3 and, channel 0, grad_b3 (grad_w3 / grad_b3 may be NULL)
__global__ void __launch_bounds__(64)
head32_tail_bwd_finish_kernel(const double *__restrict__ part, float *__restrict__ grad_gamma, float *__restrict__ grad_beta,
                              float *__restrict__ mb, float *__restrict__ mg, float *__restrict__ grad_w3,
                              float *__restrict__ grad_b3, int C, int CO, int slabs, long n) {
  const int c = (int)(blockIdx.x * 64 + threadIdx.x);
  if (c >= C) return;
  const int K = 2 + 2 * CO;
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (int sl = 0; sl < slabs; ++sl) s = s + part[((long)c * slabs + sl) * K + k];
    if (k == 0) {
      grad_beta[c] = (float)s;
      mb[c] = (float)(s / (double)n);
    } else if (k == 1) {
      grad_gamma[c] = (float)s;
      mg[c] = (float)(s / (double)n);
    } else if (k < 2 + CO) {
      if (grad_w3) grad_w3[(k - 2) * C + c] = (float)s;
    } else if (c == 0 && grad_b3) {
      grad_b3[k - 2 - CO] = (float)s;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// head32_dw_bwd_kernel: the backward of the depthwise 3x3 between the two BatchNorm + ReLU pairs (head_dw_bwd_kernel's
// layout: a workgroup works on chunk blockIdx.x % chunks of the strips of ONE (n, c) plane).
//   grad_y2 formed while loading g_z2 and y2 (SUB: batch statistics of BatchNorm2; !SUB: eval mode), 0 outside the plane
//   grad_a1[q] = sum_t w2[c][t] grad_y2[q - t]       a GATHER over the nine neighbours with mirrored taps
//   g_z1 = z1 > 0 ? grad_a1 : 0                       stored; z1, xh1 from load_win's bn_z
//   part [N][C][chunks][11]: grad_W2[c][t] = sum_p grad_y2[p] a1[p + t], T1 = sum g_z1, T2 = sum g_z1 xh1 (float64)
// ------------------------------------------------------------------------------------------------------
template <bool SUB, bool VEC>
__global__ void __launch_bounds__(256, 4)      // four waves per SIMD: 128 VGPRs
head32_dw_bwd_kernel(const float *__restrict__ gz2, const float *__restrict__ y2, const float *__restrict__ mean2,
                     const float *__restrict__ invstd2, const float *__restrict__ gamma2, const float *__restrict__ mb2,
                     const float *__restrict__ mg2, const float *__restrict__ y1, const float *__restrict__ mean1,
                     const float *__restrict__ invstd1, const float *__restrict__ gamma1, const float *__restrict__ beta1,
                     const float *__restrict__ w2, float *__restrict__ gz1, double *__restrict__ part, int C, int H, int W,
                     int wq, int strips, int chunks) {
  __shared__ double red[4 * kDwSums];
  const int chunk = (int)(blockIdx.x % chunks);
  const long plane = blockIdx.x / chunks;
  const int c = (int)(plane % C);
  const int item = chunk * (int)blockDim.x + (int)threadIdx.x;
  double sums[kDwSums];
#pragma unroll
  for (int k = 0; k < kDwSums; ++k) sums[k] = 0.0;
  if (item < wq * strips) {
    const int x0 = (item % wq) * 4, ya = (item / wq) * kStripRows, yb = min(H, ya + kStripRows);
    const long HW = (long)H * W;
    const float *gsrc = gz2 + plane * HW, *y2src = y2 + plane * HW, *y1src = y1 + plane * HW;
    float *dst = gz1 + plane * HW;
    const BnCh p1 = load_ch(mean1, invstd1, gamma1, beta1, c);
    const BnBwd2 q2 = load_bwd2<SUB>(mean2, invstd2, gamma2, mb2, mg2, c);
    float w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = w2[c * 9 + k];
    float gw[3][6], aw[3][6], xm[4], xn[4];      // xh1 of the middle and of the newest row
    unsigned pos[3];
    // one window row: grad_y2 (bn_grad_y), a1 with its mask z1 > 0 and xh1
    auto load_row = [&](int y, float (&gr)[6], float (&ar)[6], float (&xr)[4], unsigned &pm) {
      float gv[6], yv[6];
      const unsigned ok = cdn::load_cols<6, 1, VEC>(gsrc, y, H, W, x0, gv);
      if (SUB) cdn::load_cols<6, 1, VEC>(y2src, y, H, W, x0, yv);
#pragma unroll
      for (int j = 0; j < 6; ++j) gr[j] = ((ok >> j) & 1u) ? bn_grad_y<SUB>(gv[j], SUB ? yv[j] : 0.0f, q2) : 0.0f;
      pm = load_win<6, true, VEC>(y1src, y, H, W, x0, p1, ar, xr);
    };
    load_row(ya - 1, gw[0], aw[0], xn, pos[0]);
    load_row(ya, gw[1], aw[1], xm, pos[1]);
    for (int y = ya; y < yb; ++y) {
      load_row(y + 1, gw[2], aw[2], xn, pos[2]);
      float out[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float ga = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const float pr = w[dy * 3 + dx] * gw[2 - dy][i + 2 - dx];
            ga = ga + pr;
          }
        out[i] = ((pos[1] >> (i + 1)) & 1u) ? ga : 0.0f;
        if (x0 + i < W) {
          const double gc = (double)gw[1][i + 1];
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) sums[dy * 3 + dx] = sums[dy * 3 + dx] + gc * (double)aw[dy][i + dx];
          sums[9] = sums[9] + (double)out[i];
          sums[10] = sums[10] + (double)out[i] * (double)xm[i];
        }
      }
      cdn::store4<VEC>(dst + (long)y * W, W, x0, out);
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        gw[0][j] = gw[1][j]; gw[1][j] = gw[2][j];
        aw[0][j] = aw[1][j]; aw[1][j] = aw[2][j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) xm[j] = xn[j];
      pos[0] = pos[1];
      pos[1] = pos[2];
    }
  }
  cdn::block_sums_store(sums, red, part);
}

// ------------------------------------------------------------------------------------------------------
// head32_bn_bwd2_kernel: bn_bwd2_kernel with grad_y written through an image pitch (a channel slice of a wider
// [N][heads * C][H][W] buffer); the same expression.  Rows and quads as in bn_apply_kernel.
// ------------------------------------------------------------------------------------------------------
template <bool SUB, bool VEC>
__global__ void __launch_bounds__(256)
head32_bn_bwd2_kernel(const float *__restrict__ gz, const float *__restrict__ y, const float *__restrict__ mean,
                      const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ mb,
                      const float *__restrict__ mg, float *__restrict__ gy, long pitch, long rows, int C, int H, int W) {
  const int Wq = (W + 3) >> 2;
  const long total = rows * Wq;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = (unsigned)i / (unsigned)Wq;
    const int w0 = (int)((unsigned)i - (unsigned)r * (unsigned)Wq) * 4;
    const unsigned plane = (unsigned)r / (unsigned)H;
    const int h = (int)((unsigned)r - plane * (unsigned)H);
    const unsigned img = plane / (unsigned)C;
    const int c = (int)(plane - img * (unsigned)C);
    const BnBwd2 q = load_bwd2<SUB>(mean, invstd, gamma, mb, mg, c);
    const long off = r * W + w0;
    float *dst = gy + (long)img * pitch + ((long)c * H + h) * W + w0;
    const int cnt = (VEC || W - w0 > 4) ? 4 : W - w0;
    float v[4], z[4], o[4];
    if (VEC) {
      const float4 t = *reinterpret_cast<const float4 *>(gz + off);
      z[0] = t.x; z[1] = t.y; z[2] = t.z; z[3] = t.w;
      if (SUB) {
        const float4 u = *reinterpret_cast<const float4 *>(y + off);
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        z[e] = e < cnt ? gz[off + e] : 0.0f;
        v[e] = (SUB && e < cnt) ? y[off + e] : 0.0f;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = bn_grad_y<SUB>(z[e], SUB ? v[e] : 0.0f, q);
    if (VEC) {
      *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) dst[e] = o[e];
    }
  }
}

size_t head32_ws_bytes(int64_t N, int64_t C, int64_t H, int64_t W) {
  const size_t slabs = (size_t)cdn::ceil_div(N * H * W, kBnSlab);
  const size_t tail = (size_t)C * slabs * 10 * sizeof(double);      // 2 + 2 Co sums, Co <= 4 (the statistics: 2)
  return cdn::round256(std::max(tail, dw_part_bytes(N, C, H, W)));
}

}  // namespace

extern "C" size_t cdn_codenet_head_fp32_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return head32_ws_bytes(N, C, H, W);
}

extern "C" int cdn_codenet_head_fp32_bn_stats(const float *y, float *running_mean, float *running_var,
                                              int64_t *num_batches_tracked, float *mean, float *var, float *invstd, int64_t N,
                                              int64_t C, int64_t H, int64_t W, int training, double eps, double momentum,
                                              void *workspace, size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(y && mean && var && invstd, CDN_ERR_ARG, "null pointer");
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  if (int rc = launch_bn_stats(y, running_mean, running_var, num_batches_tracked, mean, var, invstd, N, C, H, W, training, eps,
                               momentum, workspace, workspace_bytes, head32_ws_bytes(N, C, H, W), cdn::as_stream(stream)))
    return rc;
  return cdn::check_launch("codenet head fp32 statistics");
}

extern "C" int cdn_codenet_head_fp32_dw_forward(const float *y1, const float *mean1, const float *invstd1,
                                                const float *gamma1, const float *beta1, const float *w2, float *y2,
                                                int64_t N, int64_t C, int64_t H, int64_t W, void *stream) {
  CDN_REQUIRE(y1 && mean1 && invstd1 && gamma1 && beta1 && w2 && y2, CDN_ERR_ARG, "null pointer");
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  const StripPlan p = strip_plan(H, W);
  const long items = (long)(N * C) * p.strips * p.wq;
  const unsigned grid = (unsigned)cdn::ceil_div(items, 256);
  const bool vec = (W & 3) == 0 && cdn::aligned16(y1) && cdn::aligned16(y2);
  hipStream_t st = cdn::as_stream(stream);
  if (vec)
    head32_dw_fwd_kernel<true><<<grid, 256, 0, st>>>(y1, mean1, invstd1, gamma1, beta1, w2, y2, (int)C, (int)H, (int)W, p.wq,
                                                     p.strips, items);
  else
    head32_dw_fwd_kernel<false><<<grid, 256, 0, st>>>(y1, mean1, invstd1, gamma1, beta1, w2, y2, (int)C, (int)H, (int)W, p.wq,
                                                      p.strips, items);
  return cdn::check_launch("codenet head fp32 depthwise forward");
}

extern "C" int cdn_codenet_head_fp32_tail_forward(const float *y2, const float *mean2, const float *invstd2,
                                                  const float *gamma2, const float *beta2, const float *w3, const float *b3,
                                                  float *y3, int64_t N, int64_t C, int64_t Co, int64_t H, int64_t W,
                                                  void *stream) {
  CDN_REQUIRE(y2 && mean2 && invstd2 && gamma2 && beta2 && w3 && y3, CDN_ERR_ARG, "null pointer");
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  CDN_REQUIRE(Co > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(Co <= 4, CDN_ERR_UNSUPPORTED, "1 <= Co <= 4, got %lld", (long long)Co);
  const int64_t HW = H * W;
  const int hq = (int)cdn::ceil_div(HW, 4);
  const long items = (long)N * hq;
  const unsigned grid = (unsigned)cdn::ceil_div(items, 256);
  const bool vec = (HW & 3) == 0 && cdn::aligned16(y2) && cdn::aligned16(y3);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_TAIL32(CO)                                                                                                       \
  if (vec)                                                                                                                   \
    head32_tail_fwd_kernel<CO, true><<<grid, 256, 0, st>>>(y2, mean2, invstd2, gamma2, beta2, w3, b3, y3, (int)C, (int)HW, hq, \
                                                           items);                                                           \
  else                                                                                                                       \
    head32_tail_fwd_kernel<CO, false><<<grid, 256, 0, st>>>(y2, mean2, invstd2, gamma2, beta2, w3, b3, y3, (int)C, (int)HW,    \
                                                            hq, items)
  switch ((int)Co) {
    case 1: CDN_TAIL32(1); break;
    case 2: CDN_TAIL32(2); break;
    case 3: CDN_TAIL32(3); break;
    default: CDN_TAIL32(4); break;
  }
#undef CDN_TAIL32
  return cdn::check_launch("codenet head fp32 tail forward");
}

extern "C" int cdn_codenet_head_fp32_tail_backward(const float *grad_y3, const float *y2, const float *mean2,
                                                   const float *invstd2, const float *gamma2, const float *beta2,
                                                   const float *w3, float *g_z2, float *grad_gamma2, float *grad_beta2,
                                                   float *mb2, float *mg2, float *grad_w3, float *grad_b3, int64_t N,
                                                   int64_t C, int64_t Co, int64_t H, int64_t W, void *workspace,
                                                   size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(grad_y3 && y2 && mean2 && invstd2 && gamma2 && beta2 && w3 && g_z2 && grad_gamma2 && grad_beta2 && mb2 && mg2 &&
                  workspace,
              CDN_ERR_ARG, "null pointer");
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  CDN_REQUIRE(Co > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(Co <= 4, CDN_ERR_UNSUPPORTED, "1 <= Co <= 4, got %lld", (long long)Co);
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, head32_ws_bytes(N, C, H, W))) return rc;
  const BnPlan p = bn_plan(N, C, H, W);
  double *part = static_cast<double *>(workspace);
  const unsigned grid = (unsigned)(C * p.slabs);
  const bool vec = (W & 3) == 0 && cdn::aligned16(grad_y3) && cdn::aligned16(y2) && cdn::aligned16(g_z2);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_TBWD32(CO)                                                                                                        \
  if (vec)                                                                                                                    \
    head32_tail_bwd_kernel<CO, true><<<grid, kBnThreads, 0, st>>>(grad_y3, y2, mean2, invstd2, gamma2, beta2, w3, g_z2, part,   \
                                                                  (int)C, (int)(H * W), p.n, p.slabs);                        \
  else                                                                                                                        \
    head32_tail_bwd_kernel<CO, false><<<grid, kBnThreads, 0, st>>>(grad_y3, y2, mean2, invstd2, gamma2, beta2, w3, g_z2, part,  \
                                                                   (int)C, (int)(H * W), p.n, p.slabs)
  switch ((int)Co) {
    case 1: CDN_TBWD32(1); break;
    case 2: CDN_TBWD32(2); break;
    case 3: CDN_TBWD32(3); break;
    default: CDN_TBWD32(4); break;
  }
#undef CDN_TBWD32
  head32_tail_bwd_finish_kernel<<<(unsigned)cdn::ceil_div(C, 64), 64, 0, st>>>(part, grad_gamma2, grad_beta2, mb2, mg2, grad_w3,
                                                                               grad_b3, (int)C, (int)Co, p.slabs, p.n);
  return cdn::check_launch("codenet head fp32 tail backward");
}

extern "C" int cdn_codenet_head_fp32_bn_backward1(const float *grad_a, const float *y, const float *mean, const float *invstd,
                                                  const float *gamma, const float *beta, float *g_z, float *grad_gamma,
                                                  float *grad_beta, float *mb, float *mg, int64_t N, int64_t C, int64_t H,
                                                  int64_t W, void *workspace, size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(grad_a && y && mean && invstd && gamma && beta && g_z && grad_gamma && grad_beta && mb && mg && workspace,
              CDN_ERR_ARG, "null pointer");
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  CDN_REQUIRE(grad_a != g_z, CDN_ERR_ARG, "g_z must not be grad_a");
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, head32_ws_bytes(N, C, H, W))) return rc;
  const BnPlan p = bn_plan(N, C, H, W);
  double *part = static_cast<double *>(workspace);
  const unsigned grid = (unsigned)(C * p.slabs);
  hipStream_t st = cdn::as_stream(stream);
  if ((W & 3) == 0 && cdn::aligned16(grad_a) && cdn::aligned16(y) && cdn::aligned16(g_z))
    bn_bwd1_kernel<1, true><<<grid, kBnThreads, 0, st>>>(grad_a, y, mean, invstd, gamma, beta, g_z, part, (int)C, (int)H, (int)W,
                                                         p.n, p.slabs);
  else
    bn_bwd1_kernel<1, false><<<grid, kBnThreads, 0, st>>>(grad_a, y, mean, invstd, gamma, beta, g_z, part, (int)C, (int)H,
                                                          (int)W, p.n, p.slabs);
  launch_bn_bwd_finish(part, grad_gamma, grad_beta, mb, mg, C, p, st);
  return cdn::check_launch("codenet head fp32 BatchNorm backward, first pass");
}

extern "C" int cdn_codenet_head_fp32_dw_backward(const float *g_z2, const float *y2, const float *mean2, const float *invstd2,
                                                 const float *gamma2, const float *mb2, const float *mg2, int training2,
                                                 const float *y1, const float *mean1, const float *invstd1,
                                                 const float *gamma1, const float *beta1, const float *w2, float *g_z1,
                                                 float *grad_w2, float *grad_gamma1, float *grad_beta1, float *mb1, float *mg1,
                                                 int64_t N, int64_t C, int64_t H, int64_t W, void *workspace,
                                                 size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(g_z2 && y2 && mean2 && invstd2 && gamma2 && (!training2 || (mb2 && mg2)) && y1 && mean1 && invstd1 && gamma1 &&
                  beta1 && w2 && g_z1 && grad_w2 && grad_gamma1 && grad_beta1 && mb1 && mg1 && workspace,
              CDN_ERR_ARG, "null pointer");
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, head32_ws_bytes(N, C, H, W))) return rc;
  const StripPlan p = strip_plan(H, W);
  const bool vec = (W & 3) == 0 && cdn::aligned16(g_z2) && cdn::aligned16(y2) && cdn::aligned16(y1) && cdn::aligned16(g_z1);
  const unsigned grid = (unsigned)(N * C * p.chunks);
  double *part = static_cast<double *>(workspace);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_HBWD32(SUB, VEC)                                                                                                  \
  head32_dw_bwd_kernel<SUB, VEC><<<grid, p.threads, 0, st>>>(g_z2, y2, mean2, invstd2, gamma2, mb2, mg2, y1, mean1, invstd1,    \
                                                             gamma1, beta1, w2, g_z1, part, (int)C, (int)H, (int)W, p.wq,      \
                                                             p.strips, p.chunks)
  if (training2) {
    if (vec) CDN_HBWD32(true, true); else CDN_HBWD32(true, false);
  } else {
    if (vec) CDN_HBWD32(false, true); else CDN_HBWD32(false, false);
  }
#undef CDN_HBWD32
  dw_bwd_finish_kernel<<<(unsigned)cdn::ceil_div(C * kDwSums, 256), 256, 0, st>>>(
      part, grad_w2, grad_gamma1, grad_beta1, mb1, mg1, (int)N, (int)C, p.chunks, (long)(N * H * W));
  return cdn::check_launch("codenet head fp32 depthwise backward");
}

extern "C" int cdn_codenet_head_fp32_bn_backward2(const float *g_z, const float *y, const float *mean, const float *invstd,
                                                  const float *gamma, const float *mb, const float *mg, float *grad_y,
                                                  int64_t grad_y_image_pitch, int64_t N, int64_t C, int64_t H, int64_t W,
                                                  int training, void *stream) {
  CDN_REQUIRE(g_z && y && mean && invstd && gamma && (!training || (mb && mg)) && grad_y, CDN_ERR_ARG, "null pointer");
  if (int rc = train32_check_shape(N, C, H, W)) return rc;
  CDN_REQUIRE(grad_y_image_pitch >= C * H * W, CDN_ERR_ARG, "image pitch of grad_y below C * H * W");
  CDN_REQUIRE(N * grad_y_image_pitch < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  const long rows = (long)(N * C * H);
  const unsigned grid = rows_grid(rows, W);
  const bool vec = (W & 3) == 0 && (grad_y_image_pitch & 3) == 0 && cdn::aligned16(g_z) && cdn::aligned16(y) &&
                   cdn::aligned16(grad_y);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_BWD2P(SUB, VEC)                                                                                                 \
  head32_bn_bwd2_kernel<SUB, VEC><<<grid, 256, 0, st>>>(g_z, y, mean, invstd, gamma, mb, mg, grad_y, (long)grad_y_image_pitch, \
                                                        rows, (int)C, (int)H, (int)W)
  if (training) {
    if (vec) CDN_BWD2P(true, true); else CDN_BWD2P(true, false);
  } else {
    if (vec) CDN_BWD2P(false, true); else CDN_BWD2P(false, false);
  }
#undef CDN_BWD2P
  return cdn::check_launch("codenet head fp32 BatchNorm backward, second pass");
}
