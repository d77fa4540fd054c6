// codenet_heads_train.hip -- forward and backward of the quantised detection heads in the QAT step
// (QuantDepthwiseNode, reference quant_modules.py:1013-1071):
//   y1 = conv1x1(x, W1q) + b1      a1 = fq1(relu(y1))
//   y2 = dw3x3(a1, W2q, pad 0) + b2      r2 = relu(y2)      a2 = fq3(r2)
//   y3 = conv1x1(a2, W3q) + b3
// The two dense 1x1 convolutions and their gradients run on the pointwise kernels of codenet_stage.hip /
// codenet_train.hip; here: the depthwise 3x3 (forward with the range update of the QuantAct behind it, backward with
// fixed-order weight / bias gradients) and the last conv of the heads with at most four output channels (wh, reg), whose
// 64-channel input gradient is formed inside the depthwise backward instead of being stored.  NCHW fp32, as on the whole
// training path; straight-through quantisers, ReLU masks y > 0.
//
// Work decomposition of the depthwise kernels: a thread owns a strip of kHdRows rows x 4 columns of one (n, c) plane and
// slides a 3-row x 6-column register window down it, so every input row is read 1 + 2 / kHdRows times.  Consecutive
// threads own consecutive column quads of a row (one 16-byte load each where the rows are 16-byte aligned, scalar loads
// for ragged widths and misaligned pointers), then consecutive strips.  No LDS tiles, no scratch: occupancy hides the
// latency of these bandwidth-bound kernels.
#include "cdn_train.h"

#include <algorithm>

namespace {

constexpr int kHdRows = 8;      // rows of a thread's strip
constexpr int kHdSums = 10;     // per-channel sums of the backward: nine taps of grad_w2 and grad_b2

using cdn::Fq;
using cdn::load_fq;

// ------------------------------------------------------------------------------------------------------
// head_dw_fwd_kernel: r2 = relu(dw3x3(fq1(relu(y1)), w2) + b2), stored BEFORE quantisation (its consumers fake-quantise
// while loading).  qu.counters != NULL: the launch's last workgroup updates the QuantAct behind r2 from the extremes of
// what was stored and leaves the state snapshot (cdn::block_minmax_finish, the protocol of scale_kernel / dw4_kernel).
// Sum order of an output: taps in row-major order by fma from zero, then + b2.
// ------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256)
head_dw_fwd_kernel(const float *__restrict__ y1, const unsigned *__restrict__ a1_state, const float *__restrict__ w2,
                   const float *__restrict__ b2, float *__restrict__ r2, int C, int H, int W, int wq, int strips, long items,
                   cdn::QUpdate qu, unsigned *state_copy) {
  __shared__ float red[16];
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;
  if (idx < items) {
    const int q = (int)(idx % wq);
    const long t = idx / wq;
    const int strip = (int)(t % strips);
    const long plane = t / strips;
    const int c = (int)(plane % C);
    const int x0 = q * 4, ya = strip * kHdRows, yb = min(H, ya + kHdRows);
    const float *src = y1 + plane * H * W;
    float *dst = r2 + plane * H * W;
    const Fq f = load_fq(a1_state);
    float w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = w2[c * 9 + k];
    const float bias = b2 ? b2[c] : 0.0f;
    float a[3][6];
    cdn::load_act<6, true, VEC>(src, ya - 1, H, W, x0, f, a[0]);
    cdn::load_act<6, true, VEC>(src, ya, H, W, x0, f, a[1]);
    for (int y = ya; y < yb; ++y) {
      cdn::load_act<6, true, VEC>(src, y + 1, H, W, x0, f, a[2]);
      float out[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float acc = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) acc = fmaf(w[dy * 3 + dx], a[dy][i + dx], acc);
        const float v = cdn::relu_keep_nan(acc + bias);
        out[i] = v;
        if (x0 + i < W) {
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          has_nan |= (v != v);
        }
      }
      cdn::store4<VEC>(dst + (long)y * W, W, x0, out);
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        a[0][j] = a[1][j];
        a[1][j] = a[2][j];
      }
    }
  }
  if (qu.counters) {
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), (int)blockIdx.x, (int)gridDim.x, qu,
                             red);
    cdn::last_block_state_copy(qu, state_copy, red);
  }
}

// ------------------------------------------------------------------------------------------------------
// head_tail_fwd_kernel: y3 = W3q . fq3(r2) + b3 for CO <= 4 output channels on the VALU, r2 read once.  A thread owns four
// consecutive pixels of one image and walks the input channels in ascending order (fma from zero, then + b3).
// ------------------------------------------------------------------------------------------------------
template <int CO, bool VEC>
__global__ void __launch_bounds__(256)
head_tail_fwd_kernel(const float *__restrict__ r2, const unsigned *__restrict__ a2_state, const float *__restrict__ w3,
                     const float *__restrict__ b3, float *__restrict__ y3, int C, int HW, int hq, long items) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= items) return;
  const long n = idx / hq;
  const int p0 = (int)(idx % hq) * 4;
  const Fq f = load_fq(a2_state);
  const float *src = r2 + n * C * HW + p0;
  float acc[CO][4];
#pragma unroll
  for (int o = 0; o < CO; ++o)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[o][e] = 0.0f;
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
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
      const float a = cdn::fake_quant_r(v[e], f.s, f.z, f.r);
#pragma unroll
      for (int o = 0; o < CO; ++o) acc[o][e] = fmaf(w3[o * C + c], a, acc[o][e]);
    }
  }
#pragma unroll
  for (int o = 0; o < CO; ++o) {
    const float b = b3 ? b3[o] : 0.0f;
    float *dst = y3 + (n * CO + o) * HW + p0;
    if (VEC) {
      *reinterpret_cast<float4 *>(dst) = make_float4(acc[o][0] + b, acc[o][1] + b, acc[o][2] + b, acc[o][3] + b);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < HW) dst[e] = acc[o][e] + b;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// head_dw_bwd_kernel: the backward of the depthwise 3x3 between the two ReLU / QuantAct pairs.
//   g_y2 = g_a2 . [r2 > 0]                      CO == 0: g is g_a2 [N][C][H][W]
//   g_y2 = [r2 > 0] . sum_o W3q[o][c] g_y3[o]   CO >= 1: g is g_y3 [N][CO][H][W] (o ascending; g_a2 is never stored)
//   g_y1[q] = [y1[q] > 0] . sum_t W2q[c][t] g_y2[q - t]        a GATHER over the nine neighbours with mirrored taps
//   g_W2q[c][t] = sum_{n,p} g_y2[p] a1[p + t],  g_b2[c] = sum_{n,p} g_y2[p],  a1 = fq1(relu(y1)) recomputed on load
// A workgroup works on ONE (n, c) plane (chunk blockIdx.x % chunks of its strips), so its ten sums belong to one channel:
// a thread sums its own pixels in row-major order, then cdn::block_sums_store; the partials [N][C][chunks][10] of a
// channel are added in index order (images, then chunks) by cdn::launch_sums_reduce (cdn_train.h).
// g_y1 goes to gy1 + n * gy1_pitch + c * H * W: a channel slice of a wider [N][heads * C][H][W] buffer.
// ------------------------------------------------------------------------------------------------------
template <int CO, bool VEC>
__global__ void __launch_bounds__(256)
head_dw_bwd_kernel(const float *__restrict__ g, const float *__restrict__ w3, const float *__restrict__ r2,
                   const float *__restrict__ y1, const unsigned *__restrict__ a1_state, const float *__restrict__ w2,
                   float *__restrict__ gy1, long gy1_pitch, float *__restrict__ part, int C, int H, int W, int wq,
                   int strips, int chunks) {
  __shared__ float red[4 * kHdSums];
  const int chunk = (int)(blockIdx.x % chunks);
  const long plane = blockIdx.x / chunks;
  const int n = (int)(plane / C), c = (int)(plane % C);
  const int item = chunk * (int)blockDim.x + (int)threadIdx.x;
  float sums[kHdSums];
#pragma unroll
  for (int k = 0; k < kHdSums; ++k) sums[k] = 0.0f;
  if (item < wq * strips) {
    const int x0 = (item % wq) * 4, ya = (item / wq) * kHdRows, yb = min(H, ya + kHdRows);
    const long HW = (long)H * W;
    const float *gsrc = CO ? g + (long)n * (CO ? CO : 1) * HW : g + plane * HW;
    const float *rsrc = r2 + plane * HW, *ysrc = y1 + plane * HW;
    float *dst = gy1 + (long)n * gy1_pitch + (long)c * HW;
    const Fq f = load_fq(a1_state);
    float w[9], w3c[CO ? CO : 1];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = w2[c * 9 + k];
#pragma unroll
    for (int o = 0; o < CO; ++o) w3c[o] = w3[o * C + c];
    float gw[3][6], aw[3][6];
    unsigned pos[3];
    // one window row: g_y2 (masked by r2 > 0), a1 and the mask y1 > 0
    auto load_row = [&](int y, float (&gr)[6], float (&ar)[6], unsigned &pm) {
      float rr[6], gv[6];
      const unsigned ok = cdn::load_cols<6, 1, VEC>(rsrc, y, H, W, x0, rr);
      if (CO == 0) {
        cdn::load_cols<6, 1, VEC>(gsrc, y, H, W, x0, gv);
      } else {
#pragma unroll
        for (int o = 0; o < CO; ++o) {
          float t[6];
          cdn::load_cols<6, 1, VEC>(gsrc + (long)o * HW, y, H, W, x0, t);
#pragma unroll
          for (int j = 0; j < 6; ++j) gv[j] = o == 0 ? w3c[0] * t[j] : fmaf(w3c[o], t[j], gv[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) gr[j] = (((ok >> j) & 1u) && rr[j] > 0.0f) ? gv[j] : 0.0f;
      pm = cdn::load_act<6, true, VEC>(ysrc, y, H, W, x0, f, ar);
    };
    load_row(ya - 1, gw[0], aw[0], pos[0]);
    load_row(ya, gw[1], aw[1], pos[1]);
    for (int y = ya; y < yb; ++y) {
      load_row(y + 1, gw[2], aw[2], pos[2]);
      float out[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float ga = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) ga = fmaf(w[dy * 3 + dx], gw[2 - dy][i + 2 - dx], ga);
        out[i] = ((pos[1] >> (i + 1)) & 1u) ? ga : 0.0f;
        if (x0 + i < W) {
          const float gc = gw[1][i + 1];
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) sums[dy * 3 + dx] = fmaf(gc, aw[dy][i + dx], sums[dy * 3 + dx]);
          sums[9] += gc;
        }
      }
      cdn::store4<VEC>(dst + (long)y * W, W, x0, out);
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        gw[0][j] = gw[1][j]; gw[1][j] = gw[2][j];
        aw[0][j] = aw[1][j]; aw[1][j] = aw[2][j];
      }
      pos[0] = pos[1];
      pos[1] = pos[2];
    }
  }
  cdn::block_sums_store(sums, red, part);
}

// grad_w [C][K - 1] and grad_b [C] of the training kernels from their workgroups' partials (cdn_train.h): one thread per
// (channel, k), the partials of its sum added in index order
__global__ void __launch_bounds__(256)
train_sums_reduce_kernel(const float *__restrict__ part, float *__restrict__ gw, float *__restrict__ gb, int C, int G, int K,
                         int outer, long outer_stride, int chunks, long chunk_stride) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * K) return;
  const int c = i / K, k = i % K;
  const float *src = part + (long)(c / G) * chunks * chunk_stride + (c % G) * K + k;
  float s = 0.0f;
  for (int o = 0; o < outer; ++o)
    for (int h = 0; h < chunks; ++h) s += src[o * outer_stride + h * chunk_stride];
  if (k < K - 1) {
    if (gw) gw[c * (K - 1) + k] = s;
  } else if (gb) {
    gb[c] = s;
  }
}

struct HdPlan {
  int wq, strips, threads, chunks;
};
HdPlan head_plan(int64_t H, int64_t W) {
  HdPlan p;
  p.wq = (int)cdn::ceil_div(W, 4);
  p.strips = (int)cdn::ceil_div(H, kHdRows);
  const long items = (long)p.wq * p.strips;
  p.threads = (int)std::min<long>(256, cdn::ceil_div(items, 64) * 64);
  p.chunks = (int)cdn::ceil_div(items, p.threads);
  return p;
}

}  // namespace

int cdn::launch_sums_reduce(const float *part, float *grad_w, float *grad_b, int C, int G, int K, int outer, int chunks,
                            hipStream_t st, const char *what) {
  const long chunk_stride = (long)G * K, outer_stride = (long)(C / G) * chunks * chunk_stride;
  train_sums_reduce_kernel<<<(unsigned)cdn::ceil_div((int64_t)C * K, 256), 256, 0, st>>>(part, grad_w, grad_b, C, G, K, outer,
                                                                                         outer_stride, chunks, chunk_stride);
  return cdn::check_launch(what);
}

extern "C" int cdn_codenet_head_act_update(float *x_min, float *x_max, void *state, const float *partials,
                                           int64_t n_partials, int bits, double momentum, int running, int relu,
                                           void *state_copy, void *stream) {
  CDN_REQUIRE(x_min && x_max && state, CDN_ERR_ARG, "null QuantAct pointer");
  CDN_REQUIRE(bits >= 2 && bits <= 16, CDN_ERR_ARG, "bits must be in [2,16], got %d", bits);
  CDN_REQUIRE(!running || (partials && n_partials > 0 && n_partials < (1ll << 31)), CDN_ERR_ARG,
              "a running range needs the producer's partials");
  CDN_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7) == 0, CDN_ERR_ARG, "partials must be 8-byte aligned");
  cdn::launch_quantact_update(x_min, x_max, static_cast<unsigned *>(state), nullptr, nullptr,
                              running ? reinterpret_cast<const float2 *>(partials) : nullptr, running ? (int)n_partials : 0,
                              bits, momentum, running, cdn::as_stream(stream), relu, static_cast<unsigned *>(state_copy));
  return cdn::check_launch("codenet head activation range update");
}

extern "C" int cdn_codenet_head_dw_forward(const float *y1, const void *a1_state, const float *w2, const float *b2,
                                           float *r2, int64_t N, int64_t C, int64_t H, int64_t W, float *x_min,
                                           float *x_max, void *state, void *counters, int bits, double momentum,
                                           int running, void *state_copy, void *stream) {
  CDN_REQUIRE(y1 && a1_state && w2 && r2, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  cdn::QUpdate qu;
  if (int rc = cdn::tracked_qupdate(&qu, x_min, x_max, state, counters, bits, momentum, running)) return rc;
  const HdPlan p = head_plan(H, W);
  const long items = (long)(N * C) * p.strips * p.wq;
  const unsigned grid = (unsigned)cdn::ceil_div(items, 256);
  const bool vec = (W & 3) == 0 && cdn::aligned16(y1) && cdn::aligned16(r2);
  const unsigned *a1s = static_cast<const unsigned *>(a1_state);
  unsigned *copy = running ? static_cast<unsigned *>(state_copy) : nullptr;
  hipStream_t st = cdn::as_stream(stream);
  if (vec)
    head_dw_fwd_kernel<true><<<grid, 256, 0, st>>>(y1, a1s, w2, b2, r2, (int)C, (int)H, (int)W, p.wq, p.strips, items, qu,
                                                   copy);
  else
    head_dw_fwd_kernel<false><<<grid, 256, 0, st>>>(y1, a1s, w2, b2, r2, (int)C, (int)H, (int)W, p.wq, p.strips, items, qu,
                                                    copy);
  return cdn::check_launch("codenet head depthwise forward");
}

extern "C" int cdn_codenet_head_tail_train_forward(const float *r2, const void *a2_state, const float *w3, const float *b3,
                                                   float *y3, int64_t N, int64_t C, int64_t Co, int64_t HW, void *stream) {
  CDN_REQUIRE(r2 && a2_state && w3 && y3, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && HW > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(Co >= 1 && Co <= 4, CDN_ERR_UNSUPPORTED, "1 <= Co <= 4, got %lld", (long long)Co);
  CDN_REQUIRE(N * C * HW < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  const int hq = (int)cdn::ceil_div(HW, 4);
  const long items = (long)N * hq;
  const unsigned grid = (unsigned)cdn::ceil_div(items, 256);
  const bool vec = (HW & 3) == 0 && cdn::aligned16(r2) && cdn::aligned16(y3);
  const unsigned *a2s = static_cast<const unsigned *>(a2_state);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_TAIL(CO)                                                                                              \
  if (vec) head_tail_fwd_kernel<CO, true><<<grid, 256, 0, st>>>(r2, a2s, w3, b3, y3, (int)C, (int)HW, hq, items); \
  else head_tail_fwd_kernel<CO, false><<<grid, 256, 0, st>>>(r2, a2s, w3, b3, y3, (int)C, (int)HW, hq, items)
  switch ((int)Co) {
    case 1: CDN_TAIL(1); break;
    case 2: CDN_TAIL(2); break;
    case 3: CDN_TAIL(3); break;
    default: CDN_TAIL(4); break;
  }
#undef CDN_TAIL
  return cdn::check_launch("codenet head tail forward");
}

extern "C" size_t cdn_codenet_head_dw_backward_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const HdPlan p = head_plan(H, W);
  return cdn::round256((size_t)N * (size_t)C * (size_t)p.chunks * kHdSums * sizeof(float));
}

extern "C" int cdn_codenet_head_dw_backward(const float *g, const float *w3, int64_t Co, const float *r2, const float *y1,
                                            const void *a1_state, const float *w2, float *grad_y1,
                                            int64_t grad_y1_image_pitch, float *grad_w2, float *grad_b2, int64_t N,
                                            int64_t C, int64_t H, int64_t W, void *workspace, size_t workspace_bytes,
                                            void *stream) {
  CDN_REQUIRE(g && r2 && y1 && a1_state && w2 && grad_y1 && workspace, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(Co >= 0 && Co <= 4 && (Co == 0 || w3), CDN_ERR_ARG,
              "Co must be 0 (g is grad_a2) or 1..4 with the last conv's weights (g is grad_y3)");
  CDN_REQUIRE(grad_y1_image_pitch >= C * H * W, CDN_ERR_ARG, "image pitch of grad_y1 below C * H * W");
  CDN_REQUIRE(N * grad_y1_image_pitch < (1ll << 31) && N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED,
              "shape too large");
  const HdPlan p = head_plan(H, W);
  CDN_REQUIRE(N * C * p.chunks < (1ll << 31), CDN_ERR_UNSUPPORTED, "too many workgroups");
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, cdn_codenet_head_dw_backward_workspace_bytes(N, C, H, W)))
    return rc;
  const bool vec = (W & 3) == 0 && (grad_y1_image_pitch & 3) == 0 && cdn::aligned16(g) && cdn::aligned16(r2) && cdn::aligned16(y1) &&
                   cdn::aligned16(grad_y1);
  const unsigned grid = (unsigned)(N * C * p.chunks);
  const unsigned *a1s = static_cast<const unsigned *>(a1_state);
  float *part = static_cast<float *>(workspace);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_HBWD(CO)                                                                                                   \
  if (vec)                                                                                                             \
    head_dw_bwd_kernel<CO, true><<<grid, p.threads, 0, st>>>(g, w3, r2, y1, a1s, w2, grad_y1, (long)grad_y1_image_pitch, \
                                                             part, (int)C, (int)H, (int)W, p.wq, p.strips, p.chunks);   \
  else                                                                                                                 \
    head_dw_bwd_kernel<CO, false><<<grid, p.threads, 0, st>>>(g, w3, r2, y1, a1s, w2, grad_y1,                          \
                                                              (long)grad_y1_image_pitch, part, (int)C, (int)H, (int)W, \
                                                              p.wq, p.strips, p.chunks)
  switch ((int)Co) {
    case 0: CDN_HBWD(0); break;
    case 1: CDN_HBWD(1); break;
    case 2: CDN_HBWD(2); break;
    case 3: CDN_HBWD(3); break;
    default: CDN_HBWD(4); break;
  }
#undef CDN_HBWD
  int rc = cdn::check_launch("codenet head depthwise backward");
  if (rc || !(grad_w2 || grad_b2)) return rc;
  return cdn::launch_sums_reduce(part, grad_w2, grad_b2, (int)C, 1, kHdSums, (int)N, p.chunks, st,
                                 "codenet head depthwise backward reduce");
}
