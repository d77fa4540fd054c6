// cdn_bn.h -- the BatchNorm2d kernels of the fp32 training path (DESIGN.md sections 4.3e to 4.3h), shared by
// codenet_bn_train.hip (the block behind a deform stage), codenet_heads_fp32_train.hip (the detection heads),
// codenet_units_fp32_train.hip (the ShuffleNetV2 units) and codenet_stem_fp32_train.hip (the stem): bn_z, the per-channel
// operands, the second backward pass's expression (bn_grad_y), the float64 (channel, slab) sums and the statistics / apply /
// first- and second-pass backward kernels with their launch plan and the two launch sequences every file repeats (statistics,
// finish); and what the depthwise kernels of the heads and the units share: the window-row loader, the strip plan, the shape
// check and the finish kernel of the depthwise backward.  The head of codenet_bn_train.hip states the arithmetic and the order
// of the sums.  Everything is in an unnamed namespace: a file that includes this header holds its own copy, compiled with that
// file's flags.  The including file is built with -fno-slp-vectorize; `#pragma clang fp contract(off)` below holds to the end
// of the translation unit.
#pragma once
#include "cdn_train.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr int kBnThreads = 256;
constexpr int kBnQuads = 4;                                // quads per thread and slab
constexpr long kBnSlab = 4L * kBnThreads * kBnQuads;       // values per slab

// per-channel operands of the apply / backward kernels
struct BnCh {
  float mean, invstd, gamma, beta;
};
__device__ __forceinline__ BnCh load_ch(const float *__restrict__ mean, const float *__restrict__ invstd,
                                        const float *__restrict__ gamma, const float *__restrict__ beta, int c) {
  BnCh p;
  p.mean = mean[c];
  p.invstd = invstd[c];
  p.gamma = gamma[c];
  p.beta = beta[c];
  return p;
}
// z = gamma * xh + beta with xh = (y - mean) * invstd: four roundings.  The forward's and the backward's z are this function.
__device__ __forceinline__ float bn_z(float y, const BnCh &p, float &xh) {
  const float d = y - p.mean;
  xh = d * p.invstd;
  const float s = p.gamma * xh;
  return s + p.beta;
}

// The second backward pass: its per-channel operands and grad_y = ((g_z - mb) - xh * mg) * (gamma * invstd) (SUB: batch
// statistics) or g_z * (gamma * invstd) (!SUB: eval mode; mb, mg and y are not read).  Every kernel that forms grad_y -- the
// two second-pass kernels, the depthwise backward kernels on load, the stem's weight gradient -- forms it here.
struct BnBwd2 {
  float mean, invstd, k, mb, mg;
};
template <bool SUB>
__device__ __forceinline__ BnBwd2 load_bwd2(const float *__restrict__ mean, const float *__restrict__ invstd,
                                            const float *__restrict__ gamma, const float *__restrict__ mb,
                                            const float *__restrict__ mg, int c) {
  BnBwd2 q;
  q.mean = mean[c];
  q.invstd = invstd[c];
  q.k = gamma[c] * q.invstd;
  q.mb = SUB ? mb[c] : 0.0f;
  q.mg = SUB ? mg[c] : 0.0f;
  return q;
}
template <bool SUB>
__device__ __forceinline__ float bn_grad_y(float gz, float y, const BnBwd2 &q) {
  if (!SUB) return gz * q.k;
  const float d = y - q.mean;
  const float xh = d * q.invstd;
  const float t1 = gz - q.mb;
  const float t2 = xh * q.mg;
  const float t3 = t1 - t2;
  return t3 * q.k;
}

// One window row (NC columns from xa - 1) of a depthwise input.  BN: a = relu(bn_z(v)) inside the plane, literal zeros
// outside (the convolution's padding -- NOT relu(bn_z(0))); returns the mask of z > 0 (the ReLU mask of the backward); xh4
// (may be NULL): xh of the columns xa .. xa + 3.  !BN: the stored values as they are (zeros outside); returns the mask of
// the columns inside.
template <int NC, bool BN, bool VEC>
__device__ __forceinline__ unsigned load_win(const float *__restrict__ plane, int y, int H, int W, int xa, const BnCh &p,
                                             float (&a)[NC], float *xh4 = nullptr) {
  float v[NC];
  const unsigned ok = cdn::load_cols<NC, 1, VEC>(plane, y, H, W, xa, v);
  if (!BN) {
#pragma unroll
    for (int j = 0; j < NC; ++j) a[j] = v[j];
    return ok;
  }
  unsigned pos = 0u;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const bool in = (ok >> j) & 1u;
    float xh;
    const float z = bn_z(v[j], p, xh);
    a[j] = in ? cdn::relu_keep_nan(z) : 0.0f;
    pos |= (in && z > 0.0f) ? (1u << j) : 0u;
    if (xh4 && j >= 1 && j <= 4) xh4[j - 1] = xh;
  }
  return pos;
}

// offset of value j of channel c in an [N][C][HW] tensor.  (Every index of these kernels lies below 2^31, bn_check_shape:
// the divisions are 32-bit unsigned ones, a fraction of the 64-bit expansion.)
__device__ __forceinline__ long ch_offset(long j, int c, int C, int HW) {
  const unsigned img = (unsigned)j / (unsigned)HW;
  return ((long)img * C + c) * (long)HW + ((unsigned)j - img * (unsigned)HW);
}

// ------------------------------------------------------------------------------------------------------
// bn_stats_kernel: the partial S1, S2 of one (channel, slab).  part [C][slabs][2].
// ------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(kBnThreads)
bn_stats_kernel(const float *__restrict__ y, double *__restrict__ part, int C, int HW, long n, int slabs) {
  __shared__ double red[2 * kBnThreads / 64];
  const int c = (int)(blockIdx.x / slabs);
  const long start = (long)(blockIdx.x % slabs) * kBnSlab;
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int it = 0; it < kBnQuads; ++it) {
    const long j0 = start + ((long)it * kBnThreads + threadIdx.x) * 4;
    if (j0 >= n) continue;
    float v[4];
    int cnt = 4;
    if (VEC) {
      const float4 t = *reinterpret_cast<const float4 *>(y + ch_offset(j0, c, C, HW));
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
      cnt = n - j0 < 4 ? (int)(n - j0) : 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = e < cnt ? y[ch_offset(j0 + e, c, C, HW)] : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) {
        const double dv = (double)v[e];
        s1 = s1 + dv;
        s2 = s2 + dv * dv;
      }
  }
  cdn::block_sums_store({s1, s2}, red, part);
}

// f32 of 1 / sqrt(v), both correctly rounded in float32 (see the head of the file)
__device__ __forceinline__ float inv_sqrt_rn(float v) {
  const float s = (float)sqrt((double)v);
  return (float)(1.0 / (double)s);
}

// ------------------------------------------------------------------------------------------------------
// bn_stats_finish_kernel: one thread per channel adds the slabs' partials in slab order and leaves mean, var (biased),
// invstd; updates the running buffers (NULL: none) and, thread 0, the batch counter.
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
bn_stats_finish_kernel(const double *__restrict__ part, float *__restrict__ mean, float *__restrict__ var,
                       float *__restrict__ invstd, float *running_mean, float *running_var, long long *batches, int C,
                       int slabs, long n, float eps, float m, float one_minus_m) {
  const int c = (int)(blockIdx.x * 64 + threadIdx.x);
  if (c == 0 && batches) *batches = *batches + 1;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
  for (int s = 0; s < slabs; ++s) {
    s1 = s1 + part[((long)c * slabs + s) * 2];
    s2 = s2 + part[((long)c * slabs + s) * 2 + 1];
  }
  const double dn = (double)n;
  const double mean_d = s1 / dn;
  const double sq = mean_d * mean_d;
  double var_d = s2 / dn - sq;
  if (var_d < 0.0) var_d = 0.0;      // (a NaN stays)
  const float mu = (float)mean_d, vb = (float)var_d;
  mean[c] = mu;
  var[c] = vb;
  invstd[c] = inv_sqrt_rn(vb + eps);
  if (running_mean) {
    const float a = one_minus_m * running_mean[c], b = m * mu;
    running_mean[c] = a + b;
  }
  if (running_var) {
    const double ratio = dn / (dn - 1.0);
    const float vu = (float)(var_d * ratio);
    const float a = one_minus_m * running_var[c], b = m * vu;
    running_var[c] = a + b;
  }
}

// eval mode: the operands from the running statistics
__global__ void __launch_bounds__(64)
bn_eval_stats_kernel(const float *__restrict__ running_mean, const float *__restrict__ running_var,
                     float *__restrict__ mean, float *__restrict__ var, float *__restrict__ invstd, int C, float eps) {
  const int c = (int)(blockIdx.x * 64 + threadIdx.x);
  if (c >= C) return;
  mean[c] = running_mean[c];
  var[c] = running_var[c];
  invstd[c] = inv_sqrt_rn(running_var[c] + eps);
}

// ------------------------------------------------------------------------------------------------------
// bn_apply_kernel: out = relu(bn_z(y)), written once (UP == 1, [rows][W]) or to the 2 x 2 replicas (UP == 2, [2 rows][2 W]).
// rows = N * C * H; a thread takes one quad of a row (Wq = ceil(W / 4) quads per row), grid-stride.
// ------------------------------------------------------------------------------------------------------
template <int UP, bool VEC>
__global__ void __launch_bounds__(256)
bn_apply_kernel(const float *__restrict__ y, const float *__restrict__ mean, const float *__restrict__ invstd,
                const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ out, long rows, int C,
                int H, int W) {
  const int Wq = (W + 3) >> 2;
  const long total = rows * Wq;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = (unsigned)i / (unsigned)Wq;
    const int w0 = (int)((unsigned)i - (unsigned)r * (unsigned)Wq) * 4;
    const BnCh p = load_ch(mean, invstd, gamma, beta, (int)(((unsigned)r / (unsigned)H) % (unsigned)C));
    const float *src = y + r * W + w0;
    float v[4], o[4];
    const int cnt = (VEC || W - w0 > 4) ? 4 : W - w0;
    if (VEC) {
      const float4 t = *reinterpret_cast<const float4 *>(src);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = e < cnt ? src[e] : 0.0f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float xh;
      o[e] = cdn::relu_keep_nan(bn_z(v[e], p, xh));
    }
    if (UP == 1) {
      float *dst = out + r * W + w0;
      if (VEC) {
        *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) dst[e] = o[e];
      }
    } else {
      float *dst = out + (r * 2) * (2L * W) + 2 * w0;
      if (VEC) {
        const float4 a = make_float4(o[0], o[0], o[1], o[1]), b = make_float4(o[2], o[2], o[3], o[3]);
        *reinterpret_cast<float4 *>(dst) = a;
        *reinterpret_cast<float4 *>(dst + 4) = b;
        *reinterpret_cast<float4 *>(dst + 2L * W) = a;
        *reinterpret_cast<float4 *>(dst + 2L * W + 4) = b;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) {
            dst[2 * e] = o[e]; dst[2 * e + 1] = o[e];
            dst[2L * W + 2 * e] = o[e]; dst[2L * W + 2 * e + 1] = o[e];
          }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// bn_bwd1_kernel: g_z of one (channel, slab) at stored resolution and the partial T1 = sum g_z, T2 = sum g_z * xh.
// g: [N][C][H][W] (UP == 1) or [N][C][2H][2W] (UP == 2).  part [C][slabs][2].  !STORE: only the sums, gz is not written (the
// un-pooled fp32 stem, whose weight gradient forms the mask on load).
// ------------------------------------------------------------------------------------------------------
template <int UP, bool VEC, bool STORE = true>
__global__ void __launch_bounds__(kBnThreads)
bn_bwd1_kernel(const float *__restrict__ g, const float *__restrict__ y, const float *__restrict__ mean,
               const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
               float *__restrict__ gz, double *__restrict__ part, int C, int H, int W, long n, int slabs) {
  __shared__ double red[2 * kBnThreads / 64];
  const int c = (int)(blockIdx.x / slabs);
  const long start = (long)(blockIdx.x % slabs) * kBnSlab;
  const int HW = H * W;
  const BnCh p = load_ch(mean, invstd, gamma, beta, c);
  double t1 = 0.0, t2 = 0.0;
#pragma unroll
  for (int it = 0; it < kBnQuads; ++it) {
    const long j0 = start + ((long)it * kBnThreads + threadIdx.x) * 4;
    if (j0 >= n) continue;
    float v[4], G[4];
    int cnt = 4;
    if (VEC) {      // the quad lies in one row
      const long off = ch_offset(j0, c, C, HW);
      const float4 t = *reinterpret_cast<const float4 *>(y + off);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
      if (UP == 1) {
        const float4 a = *reinterpret_cast<const float4 *>(g + off);
        G[0] = a.x; G[1] = a.y; G[2] = a.z; G[3] = a.w;
      } else {
        const long plane = (unsigned)off / (unsigned)HW;
        const int pix = (int)((unsigned)off - (unsigned)plane * (unsigned)HW);
        const int h = (int)((unsigned)pix / (unsigned)W), w = pix - h * W;
        const float *q = g + (plane * 2 * H + 2 * h) * (2L * W) + 2 * w;
        const float4 a0 = *reinterpret_cast<const float4 *>(q), a1 = *reinterpret_cast<const float4 *>(q + 4);
        const float4 b0 = *reinterpret_cast<const float4 *>(q + 2L * W), b1 = *reinterpret_cast<const float4 *>(q + 2L * W + 4);
        G[0] = ((a0.x + a0.y) + b0.x) + b0.y;
        G[1] = ((a0.z + a0.w) + b0.z) + b0.w;
        G[2] = ((a1.x + a1.y) + b1.x) + b1.y;
        G[3] = ((a1.z + a1.w) + b1.z) + b1.w;
      }
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float xh;
        const float z = bn_z(v[e], p, xh);
        o[e] = z > 0.0f ? G[e] : 0.0f;
        t1 = t1 + (double)o[e];
        t2 = t2 + (double)o[e] * (double)xh;
      }
      if (STORE) *reinterpret_cast<float4 *>(gz + off) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      cnt = n - j0 < 4 ? (int)(n - j0) : 4;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) {
          const long off = ch_offset(j0 + e, c, C, HW);
          float Ge;
          if (UP == 1) {
            Ge = g[off];
          } else {
            const long plane = (unsigned)off / (unsigned)HW;
            const int pix = (int)((unsigned)off - (unsigned)plane * (unsigned)HW);
            const int h = (int)((unsigned)pix / (unsigned)W), w = pix - h * W;
            const float *q = g + (plane * 2 * H + 2 * h) * (2L * W) + 2 * w;
            Ge = ((q[0] + q[1]) + q[2L * W]) + q[2L * W + 1];
          }
          float xh;
          const float z = bn_z(y[off], p, xh);
          const float o = z > 0.0f ? Ge : 0.0f;
          if (STORE) gz[off] = o;
          t1 = t1 + (double)o;
          t2 = t2 + (double)o * (double)xh;
        }
    }
  }
  cdn::block_sums_store({t1, t2}, red, part);
}

// one thread per channel: grad_beta, grad_gamma (either may be NULL) and the two means of the second pass
__global__ void __launch_bounds__(64)
bn_bwd_finish_kernel(const double *__restrict__ part, float *__restrict__ grad_gamma, float *__restrict__ grad_beta,
                     float *__restrict__ mb, float *__restrict__ mg, int C, int slabs, long n) {
  const int c = (int)(blockIdx.x * 64 + threadIdx.x);
  if (c >= C) return;
  double t1 = 0.0, t2 = 0.0;
  for (int s = 0; s < slabs; ++s) {
    t1 = t1 + part[((long)c * slabs + s) * 2];
    t2 = t2 + part[((long)c * slabs + s) * 2 + 1];
  }
  if (grad_beta) grad_beta[c] = (float)t1;
  if (grad_gamma) grad_gamma[c] = (float)t2;
  const double dn = (double)n;
  mb[c] = (float)(t1 / dn);
  mg[c] = (float)(t2 / dn);
}

// ------------------------------------------------------------------------------------------------------
// bn_bwd2_kernel: grad_y from g_z (may be the same buffer: element i is read before it is written, by the same thread).
// SUB: batch statistics (the two subtracted terms); !SUB: eval mode.  Rows and quads as in bn_apply_kernel.
// ------------------------------------------------------------------------------------------------------
template <bool SUB, bool VEC>
__global__ void __launch_bounds__(256)
bn_bwd2_kernel(const float *gz, const float *__restrict__ y, const float *__restrict__ mean,
               const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ mb,
               const float *__restrict__ mg, float *gy, long rows, int C, int H, int W) {
  const int Wq = (W + 3) >> 2;
  const long total = rows * Wq;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long r = (unsigned)i / (unsigned)Wq;
    const int w0 = (int)((unsigned)i - (unsigned)r * (unsigned)Wq) * 4;
    const int c = (int)(((unsigned)r / (unsigned)H) % (unsigned)C);
    const BnBwd2 q = load_bwd2<SUB>(mean, invstd, gamma, mb, mg, c);
    const long off = r * W + w0;
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
      *reinterpret_cast<float4 *>(gy + off) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) gy[off + e] = o[e];
    }
  }
}

struct BnPlan {
  long n;
  int slabs;
  size_t part_bytes;
};
BnPlan bn_plan(int64_t N, int64_t C, int64_t H, int64_t W) {
  BnPlan p;
  p.n = (long)(N * H * W);
  p.slabs = (int)cdn::ceil_div(p.n, kBnSlab);
  p.part_bytes = cdn::round256((size_t)C * (size_t)p.slabs * 2 * sizeof(double));
  return p;
}

int bn_check_shape(int64_t N, int64_t C, int64_t H, int64_t W, int up) {
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(up == 1 || up == 2, CDN_ERR_ARG, "up must be 1 or 2, got %d", up);
  CDN_REQUIRE(N * C * H * W * up * up < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  CDN_REQUIRE(C * cdn::ceil_div(N * H * W, kBnSlab) < (1ll << 31), CDN_ERR_UNSUPPORTED, "too many workgroups");
  return CDN_OK;
}

unsigned rows_grid(long rows, int64_t W) {
  return (unsigned)std::max<long>(1, std::min<long>(cdn::ceil_div(rows * cdn::ceil_div(W, 4), 256), (long)cdn::kCUs * 16));
}

// The statistics of y [N][C][H][W] behind the caller's pointer and shape checks: mean, var, invstd from the batch (training:
// part = workspace, of at least `need` bytes; the running buffers and the counter updated) or from the running statistics.
// The caller checks the launches.
int launch_bn_stats(const float *y, float *running_mean, float *running_var, int64_t *num_batches_tracked, float *mean,
                    float *var, float *invstd, int64_t N, int64_t C, int64_t H, int64_t W, int training, double eps,
                    double momentum, void *workspace, size_t workspace_bytes, size_t need, hipStream_t st) {
  CDN_REQUIRE(eps >= 0.0, CDN_ERR_ARG, "eps must not be negative");
  const unsigned cgrid = (unsigned)cdn::ceil_div(C, 64);
  if (!training) {
    CDN_REQUIRE(running_mean && running_var, CDN_ERR_ARG, "eval mode needs the running statistics");
    bn_eval_stats_kernel<<<cgrid, 64, 0, st>>>(running_mean, running_var, mean, var, invstd, (int)C, (float)eps);
    return CDN_OK;
  }
  CDN_REQUIRE(N * H * W > 1, CDN_ERR_ARG, "batch statistics need more than one value per channel");
  CDN_REQUIRE((running_mean == nullptr) == (running_var == nullptr), CDN_ERR_ARG, "one running buffer without the other");
  CDN_REQUIRE(momentum >= 0.0 && momentum <= 1.0, CDN_ERR_ARG, "momentum must lie in [0, 1]");
  CDN_REQUIRE(workspace, CDN_ERR_ARG, "null workspace");
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, need)) return rc;
  const BnPlan p = bn_plan(N, C, H, W);
  double *part = static_cast<double *>(workspace);
  const unsigned grid = (unsigned)(C * p.slabs);
  if (W % 4 == 0 && cdn::aligned16(y))
    bn_stats_kernel<true><<<grid, kBnThreads, 0, st>>>(y, part, (int)C, (int)(H * W), p.n, p.slabs);
  else
    bn_stats_kernel<false><<<grid, kBnThreads, 0, st>>>(y, part, (int)C, (int)(H * W), p.n, p.slabs);
  bn_stats_finish_kernel<<<cgrid, 64, 0, st>>>(part, mean, var, invstd, running_mean, running_var,
                                               reinterpret_cast<long long *>(num_batches_tracked), (int)C, p.slabs, p.n,
                                               (float)eps, (float)momentum, (float)(1.0 - momentum));
  return CDN_OK;
}

// behind a first-pass kernel that left part [C][slabs][2]
void launch_bn_bwd_finish(const double *part, float *grad_gamma, float *grad_beta, float *mb, float *mg, int64_t C,
                          const BnPlan &p, hipStream_t st) {
  bn_bwd_finish_kernel<<<(unsigned)cdn::ceil_div(C, 64), 64, 0, st>>>(part, grad_gamma, grad_beta, mb, mg, (int)C, p.slabs, p.n);
}

// ---- what the depthwise kernels of the heads and the units share ----------------------------------------------------------
constexpr int kStripRows = 8;      // rows of a thread's strip
constexpr int kDwSums = 11;        // per-plane sums of a depthwise backward: nine taps of grad_w, T1, T2

// a thread owns a strip of kStripRows rows x 4 columns of an H x W plane; a workgroup a chunk of `threads` strips of one plane
struct StripPlan {
  int wq, strips, threads, chunks;
};
StripPlan strip_plan(int64_t H, int64_t W) {
  StripPlan p;
  p.wq = (int)cdn::ceil_div(W, 4);
  p.strips = (int)cdn::ceil_div(H, kStripRows);
  const long items = (long)p.wq * p.strips;
  p.threads = (int)std::min<long>(256, cdn::ceil_div(items, 64) * 64);
  p.chunks = (int)cdn::ceil_div(items, p.threads);
  return p;
}

// [N][C][H][W] tensors of the heads and the units: positive sizes, 32-bit indexing, grids below 2^31
int train32_check_shape(int64_t N, int64_t C, int64_t H, int64_t W) {
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  CDN_REQUIRE(C * cdn::ceil_div(N * H * W, kBnSlab) < (1ll << 31), CDN_ERR_UNSUPPORTED, "too many workgroups");
  CDN_REQUIRE(N * C * strip_plan(H, W).chunks < (1ll << 31), CDN_ERR_UNSUPPORTED, "too many workgroups");
  return CDN_OK;
}

// bytes of the partials [N][C][chunks][kDwSums] of a depthwise backward
size_t dw_part_bytes(int64_t N, int64_t C, int64_t H, int64_t W) {
  return (size_t)N * (size_t)C * (size_t)strip_plan(H, W).chunks * kDwSums * sizeof(double);
}

// one thread per (channel, sum): the partials [N][C][chunks][11] added in index order (images, then chunks); leaves
// grad_w [C][9] and (grad_gamma != NULL) grad_gamma, grad_beta and the two means of BatchNorm1's second pass
__global__ void __launch_bounds__(256)
dw_bwd_finish_kernel(const double *__restrict__ part, float *__restrict__ grad_w, float *__restrict__ grad_gamma,
                     float *__restrict__ grad_beta, float *__restrict__ mb, float *__restrict__ mg, int N, int C, int chunks,
                     long n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * kDwSums) return;
  const int c = i / kDwSums, k = i % kDwSums;
  if (k >= 9 && !grad_gamma) return;
  double s = 0.0;
  for (int img = 0; img < N; ++img)
    for (int h = 0; h < chunks; ++h) s = s + part[(((long)img * C + c) * chunks + h) * kDwSums + k];
  if (k < 9) {
    grad_w[c * 9 + k] = (float)s;
  } else if (k == 9) {
    grad_beta[c] = (float)s;
    mb[c] = (float)(s / (double)n);
  } else {
    grad_gamma[c] = (float)s;
    mg[c] = (float)(s / (double)n);
  }
}

}  // namespace
