// codenet_units_train.hip -- forward and backward of the quantised ShuffleNetV2 units in the QAT step (QuantBaseNode,
// reference quant_modules.py:809-907; layers 1-3 of the backbone):
//   stride 1:  x1 = x[:, :h] (passes through unchanged)      x2 = x[:, h:]
//   stride 2:  x1 = act(relu(pw5(act4(dw4_s2(x)))))           x2 = x
//   both:      y1 = pw1(x2)   y2 = dw2_s(fq1(relu(y1)))   y3 = pw3(fq2(y2))   x2' = act(relu(y3))
//              out[:, 2j] = x1[:, j],  out[:, 2j + 1] = x2'[:, j]      (cat + channel_shuffle(., 2))
// The dense 1x1 convolutions and their gradients run on the pointwise kernels of codenet_stage.hip / codenet_train.hip
// (the *_pitched entries read a channel slice in place); here: the depthwise 3x3 at stride 1 and 2 (NO ReLU behind it:
// the QuantAct behind it tracks the signed range of the raw output) with its backward, and the join that fake-quantises
// a branch with the layer's shared QuantAct while it interleaves the channels.  NCHW fp32, straight-through quantisers,
// ReLU masks y > 0.
//
// Work decomposition of the depthwise kernels.  An item is a strip of `rows` OUTPUT rows x 4 OUTPUT columns of one
// (n, c) plane (rows = 8 where Ho >= 32, else 4): the thread slides a 3-row x (3 S + 3)-column register window of the
// input down it, S the stride.  The items of ONE channel -- column quads fastest, then strips, then images -- are cut
// into chunks of one 256-thread workgroup each: grid = C * chunks, chunks = ceil(N * strips * wq / 256).
// A workgroup therefore covers several images' planes of one channel where the planes are small (16 x 16 at batch 32:
// 512 items, two workgroups per channel, 464 workgroups at 232 channels) and its ten partial sums of the backward still
// belong to one channel.  The grid is a function of the shape alone, so every order is fixed.  No LDS tiles, no scratch:
// the neighbours' rows come from L2 and occupancy hides the latency of these bandwidth-bound kernels.
#include "cdn_train.h"

#include <algorithm>

namespace {

constexpr int kUnSums = 10;     // per-channel sums of the backward: nine taps of grad_w and grad_b

using cdn::Fq;
using cdn::load_fq;

// the item of a thread: channel, image, first output row, first output column
struct Item {
  int c, n, ya, x0;
  bool live;
};
__device__ __forceinline__ Item unit_item(int chunks, int wq, int strips, int rows, long per_channel) {
  Item it;
  it.c = (int)(blockIdx.x / chunks);
  const long idx = (long)(blockIdx.x % chunks) * blockDim.x + threadIdx.x;
  it.live = idx < per_channel;
  it.x0 = (int)(idx % wq) * 4;
  const long t = idx / wq;
  it.ya = (int)(t % strips) * rows;
  it.n = (int)(t / strips);
  return it;
}

// ------------------------------------------------------------------------------------------------------
// unit_dw_fwd_kernel<S, RQ, VEC>: y = dw3x3(a, w, stride S, zero padding 1) + b, the RAW output (no ReLU), stored before
// quantisation (its consumers fake-quantise while loading).  The input is read in place through an image pitch:
// in + n * in_pitch + c * H * W.  qu.counters != NULL: the launch's last workgroup updates the QuantAct behind y from
// the extremes of what was stored and leaves the state snapshot (cdn::block_minmax_finish).
// Sum order of an output: taps in row-major order by fma from zero, then + b.
// ------------------------------------------------------------------------------------------------------
template <int S, bool RQ, bool VEC>
__global__ void __launch_bounds__(256)
unit_dw_fwd_kernel(const float *__restrict__ in, long in_pitch, const unsigned *__restrict__ in_state,
                   const float *__restrict__ w, const float *__restrict__ b, float *__restrict__ out, int C, int H, int W,
                   int Ho, int Wo, int wq, int strips, int rows, int chunks, long per_channel, cdn::QUpdate qu,
                   unsigned *state_copy) {
  constexpr int NC = 3 * S + 3;
  __shared__ float red[16];
  const Item it = unit_item(chunks, wq, strips, rows, per_channel);
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;
  if (it.live) {
    const int c = it.c, x0 = it.x0, ya = it.ya, yb = min(Ho, ya + rows);
    const float *src = in + (long)it.n * in_pitch + (long)c * H * W;
    float *dst = out + ((long)it.n * C + c) * Ho * Wo;
    Fq f = {1.0f, 0.0f, 1.0f};
    if (RQ) f = load_fq(in_state);
    float wt[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k] = w[c * 9 + k];
    const float bias = b ? b[c] : 0.0f;
    float a[3][NC];
    cdn::load_act<NC, RQ, VEC>(src, S * ya - 1, H, W, S * x0, f, a[0]);
    if (S == 1) cdn::load_act<NC, RQ, VEC>(src, ya, H, W, x0, f, a[1]);
    for (int y = ya; y < yb; ++y) {
      if (S == 1) {
        cdn::load_act<NC, RQ, VEC>(src, y + 1, H, W, x0, f, a[2]);
      } else {
        cdn::load_act<NC, RQ, VEC>(src, S * y, H, W, S * x0, f, a[1]);
        cdn::load_act<NC, RQ, VEC>(src, S * y + 1, H, W, S * x0, f, a[2]);
      }
      float o[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float acc = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) acc = fmaf(wt[dy * 3 + dx], a[dy][S * i + dx], acc);
        const float v = acc + bias;
        o[i] = v;
        if (x0 + i < Wo) {
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
          has_nan |= (v != v);
        }
      }
      cdn::store4<VEC>(dst + (long)y * Wo, Wo, x0, o);
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
  if (qu.counters) {
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), (int)blockIdx.x, (int)gridDim.x, qu,
                             red);
    cdn::last_block_state_copy(qu, state_copy, red);
  }
}

// ------------------------------------------------------------------------------------------------------
// unit_dw_bwd_kernel<S, RQ, VEC>: the backward of that convolution; g [N][C][Ho][Wo] is the gradient of its raw output.
//   g_in[Y][X] = sum over the taps (dy, dx) with Y + 1 - dy = S yo and X + 1 - dx = S xo of w[dy][dx] g[yo][xo]
//                -- a GATHER; taps in row-major order by fma from zero.  At stride 2 the taps that reach a pixel depend
//                on its parity: (even, even) one, (even, odd) / (odd, even) two, (odd, odd) four.  RQ: masked by in > 0.
//   g_w[c][t] = sum_{n, yo, xo} g[yo][xo] a[S yo - 1 + dy][S xo - 1 + dx],   g_b[c] = sum g,   a as the forward formed it
// The thread of an output strip owns the input pixels S yo .. S yo + S - 1 x S x0 .. S x0 + 4 S - 1 of its rows, so every
// input pixel is written exactly once (odd planes: the row / column past the edge is skipped).  g_in goes to
// gin + n * gin_pitch + c * H * W (a channel slice of a wider buffer); ACC: added to what is stored there (the second of
// the two contributions to a stride-2 unit's grad_x).  gin == NULL: only the weight / bias gradient.
// Sums: a thread adds its own outputs in row-major order, then cdn::block_sums_store; the partials [C][chunks][10] of a
// channel are added in chunk order by cdn::launch_sums_reduce (cdn_train.h).
// ------------------------------------------------------------------------------------------------------
template <int S, bool RQ, bool VEC>
__global__ void __launch_bounds__(256)
unit_dw_bwd_kernel(const float *__restrict__ g, const float *__restrict__ in, long in_pitch,
                   const unsigned *__restrict__ in_state, const float *__restrict__ w, float *__restrict__ gin,
                   long gin_pitch, int acc_in, float *__restrict__ part, int C, int H, int W, int Ho, int Wo, int wq,
                   int strips, int rows, int chunks, long per_channel) {
  constexpr int NC = 3 * S + 3;
  constexpr int GR = S == 1 ? 3 : 2, GC = S == 1 ? 6 : 5, GLEAD = S == 1 ? 1 : 0;      // window of g: rows yo - GLEAD ..
  __shared__ float red[4 * kUnSums];
  const Item it = unit_item(chunks, wq, strips, rows, per_channel);
  float sums[kUnSums];
#pragma unroll
  for (int k = 0; k < kUnSums; ++k) sums[k] = 0.0f;
  if (it.live) {
    const int c = it.c, x0 = it.x0, ya = it.ya, yb = min(Ho, ya + rows);
    const float *gsrc = g + ((long)it.n * C + c) * Ho * Wo;
    const float *src = in + (long)it.n * in_pitch + (long)c * H * W;
    float *dst = gin ? gin + (long)it.n * gin_pitch + (long)c * H * W : nullptr;
    Fq f = {1.0f, 0.0f, 1.0f};
    if (RQ) f = load_fq(in_state);
    float wt[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wt[k] = w[c * 9 + k];
    float a[3][NC], gw[GR][GC];
    unsigned pos[3];
    pos[0] = cdn::load_act<NC, RQ, VEC>(src, S * ya - 1, H, W, S * x0, f, a[0]);
    if (S == 1) pos[1] = cdn::load_act<NC, RQ, VEC>(src, ya, H, W, x0, f, a[1]);
#pragma unroll
    for (int r = 0; r + 1 < GR; ++r) cdn::load_cols<GC, GLEAD, VEC>(gsrc, ya - GLEAD + r, Ho, Wo, x0, gw[r]);
    for (int y = ya; y < yb; ++y) {
      if (S == 1) {
        pos[2] = cdn::load_act<NC, RQ, VEC>(src, y + 1, H, W, x0, f, a[2]);
      } else {
        pos[1] = cdn::load_act<NC, RQ, VEC>(src, S * y, H, W, S * x0, f, a[1]);
        pos[2] = cdn::load_act<NC, RQ, VEC>(src, S * y + 1, H, W, S * x0, f, a[2]);
      }
      cdn::load_cols<GC, GLEAD, VEC>(gsrc, y - GLEAD + GR - 1, Ho, Wo, x0, gw[GR - 1]);
      // grad_in of the input rows S y + r this output row owns
#pragma unroll
      for (int r = 0; r < S; ++r) {
        const int Y = S * y + r;
        if (dst != nullptr && Y < H) {
          float *drow = dst + (long)Y * W;
#pragma unroll
          for (int qd = 0; qd < S; ++qd) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int ii = 4 * qd + e;      // input column S x0 + ii
              float ga = 0.0f;
#pragma unroll
              for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                  const int ny = r + 1 - dy, nx = ii + 1 - dx;      // S (yo - y), S (xo - x0)
                  if (((ny % S) + S) % S == 0 && ((nx % S) + S) % S == 0) {
                    const int gy = (ny + S * GLEAD) / S, gx = (nx + S * GLEAD) / S;      // window indices
                    ga = fmaf(wt[dy * 3 + dx], gw[gy][gx], ga);
                  }
                }
              if (RQ) ga = ((pos[r + 1] >> (ii + 1)) & 1u) ? ga : 0.0f;
              o[e] = ga;
            }
            const int xs = S * x0 + 4 * qd;
            if (acc_in) {
              float old[4] = {0.0f, 0.0f, 0.0f, 0.0f};
              if (VEC) {
                if (xs < W) {
                  const float4 u = *reinterpret_cast<const float4 *>(drow + xs);
                  old[0] = u.x; old[1] = u.y; old[2] = u.z; old[3] = u.w;
                }
              } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (xs + e < W) old[e] = drow[xs + e];
              }
#pragma unroll
              for (int e = 0; e < 4; ++e) o[e] = old[e] + o[e];
            }
            cdn::store4<VEC>(drow, W, xs, o);
          }
        }
      }
      // weight / bias gradient of this output row
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (x0 + i < Wo) {
          const float gc = gw[GLEAD][i + GLEAD];
#pragma unroll
          for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) sums[dy * 3 + dx] = fmaf(gc, a[dy][S * i + dx], sums[dy * 3 + dx]);
          sums[9] += gc;
        }
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        if (S == 1) {
          a[0][j] = a[1][j];
          a[1][j] = a[2][j];
        } else {
          a[0][j] = a[2][j];
        }
      }
      if (S == 1) {
        pos[0] = pos[1];
        pos[1] = pos[2];
      } else {
        pos[0] = pos[2];
      }
#pragma unroll
      for (int r = 0; r + 1 < GR; ++r)
#pragma unroll
        for (int j = 0; j < GC; ++j) gw[r][j] = gw[r + 1][j];
    }
  }
  cdn::block_sums_store(sums, red, part);
}

// ------------------------------------------------------------------------------------------------------
// unit_join_fwd_kernel: out[n][2 j + slot] = fq_act(relu(y3[n][j])) with the shared QuantAct's state snapshot, and -- the
// stride-1 unit, x1 != NULL -- out[n][2 j] = x1[n][j] copied in the same launch (x1 + n * x1_pitch + j * HW: the first
// half of the unit's input, read in place; the only time the pass-through half moves).  A thread owns four consecutive
// pixels of one (n, j) plane.
// ------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256)
unit_join_fwd_kernel(const float *__restrict__ y3, const unsigned *__restrict__ act_state, float *__restrict__ out,
                     int slot, const float *__restrict__ x1, long x1_pitch, int h, int HW, int hq, long items) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= items) return;
  const int p0 = (int)(idx % hq) * 4;
  const long plane = idx / hq;
  const int j = (int)(plane % h);
  const long n = plane / h;
  const Fq f = load_fq(act_state);
  const float *src = y3 + plane * HW + p0;
  float *dst = out + (n * 2 * h + 2 * j + slot) * HW + p0;
  if (VEC) {
    const float4 u = *reinterpret_cast<const float4 *>(src);
    *reinterpret_cast<float4 *>(dst) = make_float4(cdn::fake_quant_r(cdn::relu_keep_nan(u.x), f.s, f.z, f.r),
                                                   cdn::fake_quant_r(cdn::relu_keep_nan(u.y), f.s, f.z, f.r),
                                                   cdn::fake_quant_r(cdn::relu_keep_nan(u.z), f.s, f.z, f.r),
                                                   cdn::fake_quant_r(cdn::relu_keep_nan(u.w), f.s, f.z, f.r));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p0 + e < HW) dst[e] = cdn::fake_quant_r(cdn::relu_keep_nan(src[e]), f.s, f.z, f.r);
  }
  if (x1) {
    const float *ps = x1 + n * x1_pitch + (long)j * HW + p0;
    float *pd = out + (n * 2 * h + 2 * j) * HW + p0;
    if (VEC) {
      *reinterpret_cast<float4 *>(pd) = *reinterpret_cast<const float4 *>(ps);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < HW) pd[e] = ps[e];
    }
  }
}

// unit_join_bwd_kernel: grad_y3[n][j] = [y3 > 0] . grad_out[n][2 j + slot] (straight-through QuantAct) and -- gx1 != NULL --
// grad_x[n][j] = grad_out[n][2 j] for the pass-through half, written at gx1 + n * gx1_pitch + j * HW
template <bool VEC>
__global__ void __launch_bounds__(256)
unit_join_bwd_kernel(const float *__restrict__ gout, const float *__restrict__ y3, float *__restrict__ gy3, int slot,
                     float *__restrict__ gx1, long gx1_pitch, int h, int HW, int hq, long items) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= items) return;
  const int p0 = (int)(idx % hq) * 4;
  const long plane = idx / hq;
  const int j = (int)(plane % h);
  const long n = plane / h;
  const float *gs = gout + (n * 2 * h + 2 * j + slot) * HW + p0;
  const float *ys = y3 + plane * HW + p0;
  float *gd = gy3 + plane * HW + p0;
  if (VEC) {
    const float4 u = *reinterpret_cast<const float4 *>(ys), v = *reinterpret_cast<const float4 *>(gs);
    *reinterpret_cast<float4 *>(gd) = make_float4(u.x > 0.0f ? v.x : 0.0f, u.y > 0.0f ? v.y : 0.0f,
                                                  u.z > 0.0f ? v.z : 0.0f, u.w > 0.0f ? v.w : 0.0f);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (p0 + e < HW) gd[e] = ys[e] > 0.0f ? gs[e] : 0.0f;
  }
  if (gx1) {
    const float *ps = gout + (n * 2 * h + 2 * j) * HW + p0;
    float *pd = gx1 + n * gx1_pitch + (long)j * HW + p0;
    if (VEC) {
      *reinterpret_cast<float4 *>(pd) = *reinterpret_cast<const float4 *>(ps);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (p0 + e < HW) pd[e] = ps[e];
    }
  }
}

struct UnPlan {
  int Ho, Wo, wq, strips, rows, threads, chunks;
  long per_channel;
};
UnPlan unit_plan(int64_t N, int64_t H, int64_t W, int stride) {
  UnPlan p;
  p.Ho = (int)((H - 1) / stride + 1);
  p.Wo = (int)((W - 1) / stride + 1);
  p.rows = p.Ho >= 32 ? 8 : 4;
  p.wq = (int)cdn::ceil_div(p.Wo, 4);
  p.strips = (int)cdn::ceil_div(p.Ho, p.rows);
  p.per_channel = (long)N * p.strips * p.wq;
  p.threads = 256;      // (always: cdn::block_minmax_finish resets its top counter from thread 64, a second wave must exist)
  p.chunks = (int)cdn::ceil_div(p.per_channel, p.threads);
  return p;
}

}  // namespace

extern "C" int cdn_codenet_unit_dw_forward(const float *in, int64_t in_image_pitch, const void *in_state, const float *w,
                                           const float *b, float *out, int64_t N, int64_t C, int64_t H, int64_t W,
                                           int stride, float *x_min, float *x_max, void *state, void *counters, int bits,
                                           double momentum, int running, void *state_copy, void *stream) {
  CDN_REQUIRE(in && w && out, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(stride == 1 || stride == 2, CDN_ERR_ARG, "stride must be 1 or 2, got %d", stride);
  CDN_REQUIRE(in_image_pitch >= C * H * W, CDN_ERR_ARG, "image pitch of the input below C * H * W");
  CDN_REQUIRE(N * in_image_pitch < (1ll << 31) && N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  cdn::QUpdate qu;
  if (int rc = cdn::tracked_qupdate(&qu, x_min, x_max, state, counters, bits, momentum, running)) return rc;
  const UnPlan p = unit_plan(N, H, W, stride);
  CDN_REQUIRE(C * (int64_t)p.chunks < (1ll << 31), CDN_ERR_UNSUPPORTED, "too many workgroups");
  const bool vec = (W & 3) == 0 && (p.Wo & 3) == 0 && (in_image_pitch & 3) == 0 && cdn::aligned16(in) && cdn::aligned16(out);
  const unsigned grid = (unsigned)(C * p.chunks);
  const unsigned *ins = static_cast<const unsigned *>(in_state);
  unsigned *copy = running ? static_cast<unsigned *>(state_copy) : nullptr;
  hipStream_t st = cdn::as_stream(stream);
#define CDN_UFWD(S, RQ, VEC)                                                                                          \
  unit_dw_fwd_kernel<S, RQ, VEC><<<grid, p.threads, 0, st>>>(in, (long)in_image_pitch, ins, w, b, out, (int)C, (int)H, \
                                                            (int)W, p.Ho, p.Wo, p.wq, p.strips, p.rows, p.chunks,     \
                                                            p.per_channel, qu, copy)
#define CDN_UFWD_V(S, RQ) \
  if (vec) CDN_UFWD(S, RQ, true); else CDN_UFWD(S, RQ, false)
  if (stride == 1) {
    if (ins) { CDN_UFWD_V(1, true); } else { CDN_UFWD_V(1, false); }
  } else {
    if (ins) { CDN_UFWD_V(2, true); } else { CDN_UFWD_V(2, false); }
  }
#undef CDN_UFWD_V
#undef CDN_UFWD
  return cdn::check_launch("codenet unit depthwise forward");
}

extern "C" size_t cdn_codenet_unit_dw_backward_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int stride) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2)) return 0;
  const UnPlan p = unit_plan(N, H, W, stride);
  return cdn::round256((size_t)C * (size_t)p.chunks * kUnSums * sizeof(float));
}

extern "C" int cdn_codenet_unit_dw_backward(const float *g, const float *in, int64_t in_image_pitch, const void *in_state,
                                            const float *w, float *grad_in, int64_t grad_in_image_pitch, int accumulate,
                                            float *grad_w, float *grad_b, int64_t N, int64_t C, int64_t H, int64_t W,
                                            int stride, void *workspace, size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(g && in && w && workspace, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(stride == 1 || stride == 2, CDN_ERR_ARG, "stride must be 1 or 2, got %d", stride);
  CDN_REQUIRE(in_image_pitch >= C * H * W, CDN_ERR_ARG, "image pitch of the input below C * H * W");
  CDN_REQUIRE(!grad_in || grad_in_image_pitch >= C * H * W, CDN_ERR_ARG, "image pitch of grad_in below C * H * W");
  CDN_REQUIRE(N * in_image_pitch < (1ll << 31) && N * C * H * W < (1ll << 31) &&
                  (!grad_in || N * grad_in_image_pitch < (1ll << 31)),
              CDN_ERR_UNSUPPORTED, "shape too large");
  const UnPlan p = unit_plan(N, H, W, stride);
  CDN_REQUIRE(C * (int64_t)p.chunks < (1ll << 31), CDN_ERR_UNSUPPORTED, "too many workgroups");
  if (int rc = cdn::check_workspace(workspace, workspace_bytes,
                                    cdn_codenet_unit_dw_backward_workspace_bytes(N, C, H, W, stride)))
    return rc;
  const bool vec = (W & 3) == 0 && (p.Wo & 3) == 0 && (in_image_pitch & 3) == 0 && cdn::aligned16(in) && cdn::aligned16(g) &&
                   (!grad_in || ((grad_in_image_pitch & 3) == 0 && cdn::aligned16(grad_in)));
  const unsigned grid = (unsigned)(C * p.chunks);
  const unsigned *ins = static_cast<const unsigned *>(in_state);
  float *part = static_cast<float *>(workspace);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_UBWD(S, RQ, VEC)                                                                                            \
  unit_dw_bwd_kernel<S, RQ, VEC><<<grid, p.threads, 0, st>>>(g, in, (long)in_image_pitch, ins, w, grad_in,               \
                                                            (long)grad_in_image_pitch, accumulate ? 1 : 0, part, (int)C, \
                                                            (int)H, (int)W, p.Ho, p.Wo, p.wq, p.strips, p.rows,         \
                                                            p.chunks, p.per_channel)
#define CDN_UBWD_V(S, RQ) \
  if (vec) CDN_UBWD(S, RQ, true); else CDN_UBWD(S, RQ, false)
  if (stride == 1) {
    if (ins) { CDN_UBWD_V(1, true); } else { CDN_UBWD_V(1, false); }
  } else {
    if (ins) { CDN_UBWD_V(2, true); } else { CDN_UBWD_V(2, false); }
  }
#undef CDN_UBWD_V
#undef CDN_UBWD
  int rc = cdn::check_launch("codenet unit depthwise backward");
  if (rc || !(grad_w || grad_b)) return rc;
  return cdn::launch_sums_reduce(part, grad_w, grad_b, (int)C, 1, kUnSums, 1, p.chunks, st,
                                 "codenet unit depthwise backward reduce");
}

extern "C" int cdn_codenet_unit_join_forward(const float *y3, const void *act_state, float *out, int slot, const float *x1,
                                             int64_t x1_image_pitch, int64_t N, int64_t h, int64_t HW, void *stream) {
  CDN_REQUIRE(y3 && act_state && out, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && h > 0 && HW > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(slot == 0 || slot == 1, CDN_ERR_ARG, "slot must be 0 or 1, got %d", slot);
  CDN_REQUIRE(!x1 || (slot == 1 && x1_image_pitch >= h * HW), CDN_ERR_ARG,
              "the pass-through half needs slot 1 and an image pitch of at least h * HW");
  CDN_REQUIRE(N * 2 * h * HW < (1ll << 31) && (!x1 || N * x1_image_pitch < (1ll << 31)), CDN_ERR_UNSUPPORTED,
              "shape too large");
  const int hq = (int)cdn::ceil_div(HW, 4);
  const long items = (long)N * h * hq;
  const unsigned grid = (unsigned)cdn::ceil_div(items, 256);
  const bool vec = (HW & 3) == 0 && cdn::aligned16(y3) && cdn::aligned16(out) && (!x1 || (cdn::aligned16(x1) && (x1_image_pitch & 3) == 0));
  const unsigned *as = static_cast<const unsigned *>(act_state);
  hipStream_t st = cdn::as_stream(stream);
  if (vec)
    unit_join_fwd_kernel<true><<<grid, 256, 0, st>>>(y3, as, out, slot, x1, (long)x1_image_pitch, (int)h, (int)HW, hq, items);
  else
    unit_join_fwd_kernel<false><<<grid, 256, 0, st>>>(y3, as, out, slot, x1, (long)x1_image_pitch, (int)h, (int)HW, hq, items);
  return cdn::check_launch("codenet unit join forward");
}

extern "C" int cdn_codenet_unit_join_backward(const float *grad_out, const float *y3, float *grad_y3, int slot,
                                              float *grad_x1, int64_t grad_x1_image_pitch, int64_t N, int64_t h, int64_t HW,
                                              void *stream) {
  CDN_REQUIRE(grad_out && y3 && grad_y3, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && h > 0 && HW > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(slot == 0 || slot == 1, CDN_ERR_ARG, "slot must be 0 or 1, got %d", slot);
  CDN_REQUIRE(!grad_x1 || (slot == 1 && grad_x1_image_pitch >= h * HW), CDN_ERR_ARG,
              "the pass-through half needs slot 1 and an image pitch of at least h * HW");
  CDN_REQUIRE(N * 2 * h * HW < (1ll << 31) && (!grad_x1 || N * grad_x1_image_pitch < (1ll << 31)), CDN_ERR_UNSUPPORTED,
              "shape too large");
  const int hq = (int)cdn::ceil_div(HW, 4);
  const long items = (long)N * h * hq;
  const unsigned grid = (unsigned)cdn::ceil_div(items, 256);
  const bool vec = (HW & 3) == 0 && cdn::aligned16(grad_out) && cdn::aligned16(y3) && cdn::aligned16(grad_y3) &&
                   (!grad_x1 || (cdn::aligned16(grad_x1) && (grad_x1_image_pitch & 3) == 0));
  hipStream_t st = cdn::as_stream(stream);
  if (vec)
    unit_join_bwd_kernel<true><<<grid, 256, 0, st>>>(grad_out, y3, grad_y3, slot, grad_x1, (long)grad_x1_image_pitch,
                                                     (int)h, (int)HW, hq, items);
  else
    unit_join_bwd_kernel<false><<<grid, 256, 0, st>>>(grad_out, y3, grad_y3, slot, grad_x1, (long)grad_x1_image_pitch,
                                                      (int)h, (int)HW, hq, items);
  return cdn::check_launch("codenet unit join backward");
}
