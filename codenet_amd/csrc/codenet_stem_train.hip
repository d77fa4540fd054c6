// codenet_stem_train.hip -- forward and backward of the quantised stem in the QAT step (layer0 after quantize_model.py:26-34):
//   Wq, b = fold + 8-bit fake-quantisation of the conv weights          (cdn_codenet_weight_prep_ranked, not here)
//   y0    = conv3x3(img, Wq, stride 4 or 2, zero padding 1) + b          raw, stored: float32 NCHW [N][24][Ho][Wo]
//   act:    range updated on the extremes of max(y0, 0), then q = fq(relu(y0)) with the state AFTER that update
//   out   = q                            (stride 4)
//   out   = maxpool3x3_s2_p1(q)          (the "S2 + MaxPool" stems; windows clipped at the borders)
// Backward: the pool sends a window's gradient to the FIRST maximum of the window in row-major scan order (the framework's
// rule, val > max || isnan(val)), compared on q; the QuantAct is straight-through; ReLU masks y0 > 0; then grad_b and
// grad_Wq.  The image takes no gradient, so nothing here reads the weights in the backward.
//
// Work decomposition of the parameter gradients (the only sums over more than 27 terms).  grad_Wq is 24 x 27 sums over the
// N * Ho * Wo output positions, grad_b 24 more: 28 per output channel.  A workgroup covers a GROUP of kStGroup = 4 output
// channels x a CHUNK of 256 * P consecutive output positions (n, oy, ox flattened; P = clamp(positions / 1024, 1, 8)):
// grid = 6 groups x chunks.  A thread takes the positions chunk_start + t + 256 k, k < P, in that order: it loads the 27
// image taps of the position once (guarded, zero outside the image) and the four gradients, and adds 4 x 28 products into
// registers.  Then cdn::block_sums_store with the workgroup's 112 sums, and cdn::launch_sums_reduce adds a channel's partials
// in chunk order (cdn_train.h).  No float atomics; the grid is a function of the shape alone.  The image patch is read once
// per channel group, six times in all, through L2.
#include "cdn_train.h"

namespace {

constexpr int kStCo = 24;                         // output channels of the stem
constexpr int kStTaps = cdn::kStemTaps;           // 3 input channels x 3 x 3
constexpr int kStGroup = 4;                       // output channels per workgroup of the weight gradient
constexpr int kStSums = kStTaps + 1;              // per channel: 27 taps of grad_w and grad_b
constexpr int kStPart = kStGroup * kStSums;       // partial sums a workgroup stores

using cdn::Fq;
using cdn::fq_relu;
using cdn::load_fq;

// ------------------------------------------------------------------------------------------------------
// stem_train_fwd_kernel: y0 = conv3x3(img, w [24][27], stride, zero padding 1) + b, the RAW output, NCHW.  One lane per
// output pixel with its 27 inputs in registers; the 24 x 27 weights are wave-uniform (scalar loads).  A workgroup is 256
// consecutive pixels of one image: grid = N * chunks, chunks = ceil(Ho * Wo / 256).  qu.counters != NULL: the launch's last
// workgroup updates the QuantAct behind the stem from the extremes of max(y0, 0) and leaves the state snapshot.
// Sum order of an output: the 27 taps in (ci, dy, dx) order by fma from zero, then + b.
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
stem_train_fwd_kernel(const float *__restrict__ img, const float *__restrict__ w, const float *__restrict__ b,
                      float *__restrict__ y0, int H, int W, int Ho, int Wo, int stride, int chunks, cdn::QUpdate qu,
                      unsigned *state_copy) {
  __shared__ float red[16];
  const int n = (int)(blockIdx.x / chunks);
  const int p = (int)(blockIdx.x % chunks) * 256 + (int)threadIdx.x;
  const int HW = Ho * Wo;
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;
  if (p < HW) {
    const int oy = p / Wo, ox = p - oy * Wo;
    float v[kStTaps];
    cdn::load_stem_patch(img, n, oy, ox, H, W, stride, v);
    float *dst = y0 + (long)n * kStCo * HW + p;
#pragma unroll
    for (int co = 0; co < kStCo; ++co) {
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < kStTaps; ++k) acc = fmaf(w[co * kStTaps + k], v[k], acc);
      acc = acc + (b ? b[co] : 0.0f);
      dst[(long)co * HW] = acc;
      const float r = cdn::relu_keep_nan(acc);
      mn = fminf(mn, r);
      mx = fmaxf(mx, r);
      has_nan |= (acc != acc);
    }
  }
  if (qu.counters) {
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), (int)blockIdx.x, (int)gridDim.x, qu, red);
    cdn::last_block_state_copy(qu, state_copy, red);
  }
}

// ------------------------------------------------------------------------------------------------------
// stem_pool_fwd_kernel: out [planes][Hp][Wp] = fq(relu(max of the 3 x 3 window of y0 [planes][H][W], stride 2, padding 1,
// clipped at the borders)).  relu and the fake-quantisation are monotone (non-decreasing), so quantising the window maximum
// of y0 once equals the maximum of the quantised values, which is what the module path pools (max fq(relu(x)) =
// fq(relu(max x))).  A NaN in the window wins, as in the framework.  One thread per output pixel.
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
stem_pool_fwd_kernel(const float *__restrict__ y0, const unsigned *__restrict__ state, float *__restrict__ out, int H,
                     int W, int Hp, int Wp, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int px = (int)(i % Wp);
  const long t = i / Wp;
  const int py = (int)(t % Hp);
  const float *src = y0 + (t / Hp) * (long)H * W;
  const Fq f = load_fq(state);
  float m = -INFINITY;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int y = 2 * py + dy - 1, x = 2 * px + dx - 1;
      if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
        const float v = src[(long)y * W + x];
        m = (v > m || v != v) ? v : m;
      }
    }
  out[i] = fq_relu(m, f);
}

// ------------------------------------------------------------------------------------------------------
// stem_pool_bwd_kernel: gy0 [planes][H][W] from g [planes][Hp][Wp], a GATHER.  A window's gradient belongs to the first
// maximum of the window in row-major scan order -- the tap that wins `val > max || isnan(val)` from -inf -- compared on
// q = fq(relu(y0)), formed from the forward's state snapshot by the forward's expression: after quantisation ties are
// common and the choice must be the framework's.  A thread owns the 2 x 2 block of y0 pixels (2 by, 2 bx) .. (2 by + 1,
// 2 bx + 1); the windows that contain one of them are exactly (by, bx), (by, bx + 1), (by + 1, bx), (by + 1, bx + 1) -- one,
// two, two and four of them by the parity of the pixel's row and column -- and lie in the 5 x 5 patch of q around the block,
// which the thread quantises once.  A pixel adds the gradients of the windows it won in row-major window order, is masked by
// y0 > 0 (ReLU; the QuantAct is straight-through) and stored once.  No atomics.
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
stem_pool_bwd_kernel(const float *__restrict__ g, const float *__restrict__ y0, const unsigned *__restrict__ state,
                     float *__restrict__ gy0, int H, int W, int Hp, int Wp, int Hb, int Wb, long total) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int bx = (int)(i % Wb);
  const long t = i / Wb;
  const int by = (int)(t % Hb);
  const long plane = t / Hb;
  const float *src = y0 + plane * (long)H * W;
  const float *gs = g + plane * (long)Hp * Wp;
  float *dst = gy0 + plane * (long)H * W;
  const Fq f = load_fq(state);
  const int ya = 2 * by - 1, xa = 2 * bx - 1;      // patch origin
  float q[5][5];
  unsigned pos = 0u, in = 0u;
#pragma unroll
  for (int r = 0; r < 5; ++r)
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      const int y = ya + r, x = xa + c;
      q[r][c] = 0.0f;
      if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
        const float v = src[(long)y * W + x];
        q[r][c] = fq_relu(v, f);
        in |= 1u << (r * 5 + c);
        pos |= v > 0.0f ? (1u << (r * 5 + c)) : 0u;
      }
    }
  float acc[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
#pragma unroll
  for (int wy = 0; wy < 2; ++wy)
#pragma unroll
    for (int wx = 0; wx < 2; ++wx) {      // row-major window order
      const int py = by + wy, px = bx + wx;
      if (py < Hp && px < Wp) {
        float m = -INFINITY;
        int arg = -1;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int r = 2 * wy + dy, c = 2 * wx + dx;
            if ((in >> (r * 5 + c)) & 1u) {
              const float v = q[r][c];
              if (v > m || v != v) {
                m = v;
                arg = r * 5 + c;
              }
            }
          }
        const float gv = gs[(long)py * Wp + px];
#pragma unroll
        for (int oy = 0; oy < 2; ++oy)
#pragma unroll
          for (int ox = 0; ox < 2; ++ox)
            if (arg == (oy + 1) * 5 + ox + 1) acc[oy][ox] += gv;
      }
    }
#pragma unroll
  for (int oy = 0; oy < 2; ++oy)
#pragma unroll
    for (int ox = 0; ox < 2; ++ox) {
      const int y = 2 * by + oy, x = 2 * bx + ox;
      if (y < H && x < W) dst[(long)y * W + x] = ((pos >> ((oy + 1) * 5 + ox + 1)) & 1u) ? acc[oy][ox] : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------------
// stem_wgrad_kernel: the partial sums of grad_w / grad_b of one channel group over one chunk of output positions (see the
// head of the file).  g [N][24][Ho][Wo]; y0 != NULL: g is the gradient behind the ReLU and is masked by y0 > 0 on load;
// NULL: g is already masked (the pool backward's output).  part [groups][chunks][4][28].
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
stem_wgrad_kernel(const float *__restrict__ g, const float *__restrict__ y0, const float *__restrict__ img,
                  float *__restrict__ part, int H, int W, int Ho, int Wo, int stride, int chunks, int per_thread,
                  long positions) {
  __shared__ float red[4 * kStPart];
  const int grp = (int)(blockIdx.x / chunks);
  const long start = (long)(blockIdx.x % chunks) * 256 * per_thread;
  const int HW = Ho * Wo;
  float sums[kStPart];      // [kStGroup][kStSums]
#pragma unroll
  for (int k = 0; k < kStPart; ++k) sums[k] = 0.0f;
  for (int it = 0; it < per_thread; ++it) {
    const long pidx = start + (long)it * 256 + threadIdx.x;
    if (pidx < positions) {
      const int n = (int)(pidx / HW), p = (int)(pidx - (long)n * HW);
      const int oy = p / Wo, ox = p - oy * Wo;
      float v[kStTaps];
      cdn::load_stem_patch(img, n, oy, ox, H, W, stride, v);
      const long o = ((long)n * kStCo + grp * kStGroup) * HW + p;
#pragma unroll
      for (int e = 0; e < kStGroup; ++e) {
        float gv = g[o + (long)e * HW];
        if (y0) gv = y0[o + (long)e * HW] > 0.0f ? gv : 0.0f;
#pragma unroll
        for (int k = 0; k < kStTaps; ++k) sums[e * kStSums + k] = fmaf(gv, v[k], sums[e * kStSums + k]);
        sums[e * kStSums + kStTaps] += gv;
      }
    }
  }
  cdn::block_sums_store(sums, red, part);
}

using StPlan = cdn::StemPlan;
using cdn::stem_plan;

}  // namespace

extern "C" int cdn_codenet_stem_train_forward(const float *img, const float *w, const float *b, float *y0, int64_t N,
                                              int64_t H, int64_t W, int64_t Co, int stride, float *x_min, float *x_max,
                                              void *state, void *counters, int bits, double momentum, int running,
                                              void *state_copy, void *stream) {
  CDN_REQUIRE(img && w && y0, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(Co == kStCo, CDN_ERR_ARG, "the stem has 24 output channels, got %lld", (long long)Co);
  CDN_REQUIRE(stride == 2 || stride == 4, CDN_ERR_ARG, "stride must be 2 or 4, got %d", stride);
  const StPlan p = stem_plan(N, H, W, stride);
  CDN_REQUIRE(N * 3 * H * W < (1ll << 31) && N * kStCo * p.Ho * p.Wo < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  cdn::QUpdate qu;
  if (int rc = cdn::tracked_qupdate(&qu, x_min, x_max, state, counters, bits, momentum, running)) return rc;
  const int chunks = (int)cdn::ceil_div((int64_t)p.Ho * p.Wo, 256);
  CDN_REQUIRE(N * (int64_t)chunks < (1ll << 31), CDN_ERR_UNSUPPORTED, "too many workgroups");
  unsigned *copy = running ? static_cast<unsigned *>(state_copy) : nullptr;
  // (always 256 threads: cdn::block_minmax_finish resets its top counter from thread 64, a second wave must exist)
  stem_train_fwd_kernel<<<(unsigned)(N * chunks), 256, 0, cdn::as_stream(stream)>>>(img, w, b, y0, (int)H, (int)W, p.Ho,
                                                                                      p.Wo, stride, chunks, qu, copy);
  return cdn::check_launch("codenet stem training forward");
}

extern "C" int cdn_codenet_stem_pool_forward(const float *y0, const void *act_state, float *out, int64_t N, int64_t C,
                                             int64_t H, int64_t W, void *stream) {
  CDN_REQUIRE(y0 && act_state && out, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  const int Hp = (int)((H - 1) / 2 + 1), Wp = (int)((W - 1) / 2 + 1);
  const long total = (long)(N * C) * Hp * Wp;
  stem_pool_fwd_kernel<<<(unsigned)cdn::ceil_div(total, 256), 256, 0, cdn::as_stream(stream)>>>(
      y0, static_cast<const unsigned *>(act_state), out, (int)H, (int)W, Hp, Wp, total);
  return cdn::check_launch("codenet stem pool forward");
}

extern "C" int cdn_codenet_stem_pool_backward(const float *g, const float *y0, const void *act_state, float *grad_y0,
                                              int64_t N, int64_t C, int64_t H, int64_t W, void *stream) {
  CDN_REQUIRE(g && y0 && act_state && grad_y0, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N * C * H * W < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  const int Hp = (int)((H - 1) / 2 + 1), Wp = (int)((W - 1) / 2 + 1);
  const int Hb = (int)((H + 1) / 2), Wb = (int)((W + 1) / 2);      // 2 x 2 blocks of y0
  const long total = (long)(N * C) * Hb * Wb;
  stem_pool_bwd_kernel<<<(unsigned)cdn::ceil_div(total, 256), 256, 0, cdn::as_stream(stream)>>>(
      g, y0, static_cast<const unsigned *>(act_state), grad_y0, (int)H, (int)W, Hp, Wp, Hb, Wb, total);
  return cdn::check_launch("codenet stem pool backward");
}

extern "C" size_t cdn_codenet_stem_backward_workspace_bytes(int64_t N, int64_t H, int64_t W, int stride) {
  if (N <= 0 || H <= 0 || W <= 0 || (stride != 2 && stride != 4)) return 0;
  const StPlan p = stem_plan(N, H, W, stride);
  return cdn::round256((size_t)(kStCo / kStGroup) * (size_t)p.chunks * kStPart * sizeof(float));
}

extern "C" int cdn_codenet_stem_backward(const float *g, const float *y0, const float *img, float *grad_w, float *grad_b,
                                         int64_t N, int64_t H, int64_t W, int64_t Co, int stride, void *workspace,
                                         size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(g && img && workspace, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(Co == kStCo, CDN_ERR_ARG, "the stem has 24 output channels, got %lld", (long long)Co);
  CDN_REQUIRE(stride == 2 || stride == 4, CDN_ERR_ARG, "stride must be 2 or 4, got %d", stride);
  const StPlan p = stem_plan(N, H, W, stride);
  CDN_REQUIRE(N * 3 * H * W < (1ll << 31) && N * kStCo * p.Ho * p.Wo < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, cdn_codenet_stem_backward_workspace_bytes(N, H, W, stride)))
    return rc;
  float *part = static_cast<float *>(workspace);
  hipStream_t st = cdn::as_stream(stream);
  stem_wgrad_kernel<<<(unsigned)((kStCo / kStGroup) * p.chunks), 256, 0, st>>>(g, y0, img, part, (int)H, (int)W, p.Ho, p.Wo,
                                                                              stride, p.chunks, p.per_thread, p.positions);
  int rc = cdn::check_launch("codenet stem backward");
  if (rc || !(grad_w || grad_b)) return rc;
  return cdn::launch_sums_reduce(part, grad_w, grad_b, kStCo, kStGroup, kStSums, 1, p.chunks, st,
                                 "codenet stem backward reduce");
}
