// codenet_stem_fp32_train.hip -- forward and backward of the fp32 stem in training (main.py; layer0 of
// lib/models/networks/shufflenetv2_dcn.py: Conv2d(3, 24, 3, stride 4 | 2, padding 1, bias=False) -> BatchNorm2d -> ReLU
// [-> MaxPool2d(3, 2, 1)]):
//   y0   = conv3x3(img, W, stride, zero padding 1)      raw, stored: cdn_codenet_stem_train_forward with b = NULL, running = 0
//   st   = (mean, var, invstd) of y0                    cdn_codenet_head_fp32_bn_stats (the kernels of cdn_bn.h)
//   a0   = relu(bn_z(y0))                               a NaN kept
//   out  = a0                       (stride 4)          cdn_codenet_bn_relu_up_forward with up = 1
//   out  = maxpool3x3_s2_p1(a0)     (stride 2 + pool)   here; windows clipped at the borders; a0 is NEVER stored
// Here: the pool forward on a0 formed on load, the first BatchNorm backward pass of both stems (the pool's gather and the
// ReLU mask inside it) and the weight gradient with BatchNorm's second pass folded into its loads.  Never stored: a0, the
// ReLU mask, grad_y0 and, for the un-pooled stem, g_z.  The image takes no gradient, so nothing here reads the weights.
//
// ---- arithmetic (DESIGN.md section 4.3h is the contract; tests/stem_fp32_ref.py restates it in numpy) -------------------
// Whole file under `#pragma clang fp contract(off)`, built with -fno-slp-vectorize, as codenet_heads_fp32_train.hip: every
// float32 operator written here is rounded on its own.
//   pool      out[py][px] = the winner of `val > max || isnan(val)` from -inf over the taps of the window inside the plane in
//             row-major scan order, val = a0.  gamma may be negative, so the window is compared on a0, not on y0.
//   g_z       pooled: a window's gradient goes to that first maximum; a pixel adds the gradients of the windows it won in
//             row-major window order from 0.0f (a gather: every element written once), then g_z = z > 0 ? sum : 0.
//             un-pooled: g_z = z > 0 ? grad_out : 0, formed on load, not stored.
//   grad_y0   = ((g_z - mb) - xh mg) (gamma invstd) (training) or g_z (gamma invstd) (eval): bn_grad_y, as bn_bwd2_kernel's,
//             expression, formed on load in the weight-gradient kernel.
//   grad_W    [24][27] = sum grad_y0[n][c][oy][ox] img[n][ci][oy S + dy - 1][ox S + dx - 1] (zero outside the image)
// ---- the sums ---------------------------------------------------------------------------------------------------------------
// T1 = sum g_z, T2 = sum g_z xh: float64, the (channel, slab) protocol of cdn_bn.h -- the un-pooled stem runs bn_bwd1_kernel
// itself without its store, stem32_pool_bwd_kernel walks a slab exactly as it does, so the partials, bn_bwd_finish_kernel and
// the restatement of tests/bn_block_ref.py are shared.
// grad_W keeps the decomposition of codenet_stem_train.hip's stem_wgrad_kernel: 4-channel groups x chunks of 256 * T
// positions, float32 fma in position order, cdn::block_sums_store, cdn::launch_sums_reduce in chunk order.  No float atomics;
// every grid is a function of the shape alone.
#include "cdn_bn.h"

#pragma clang fp contract(off)

namespace {

constexpr int kS32Co = 24;                         // output channels of the stem
constexpr int kS32Taps = cdn::kStemTaps;           // 3 input channels x 3 x 3
constexpr int kS32Group = 4;                       // output channels per workgroup of the weight gradient
constexpr int kS32Sums = kS32Taps + 1;             // cdn::launch_sums_reduce's layout: 27 taps and the bias slot (no bias
                                                   // here: the slot stays 0.0f and is not read)
constexpr int kS32Part = kS32Group * kS32Sums;     // partial sums a workgroup stores

// ------------------------------------------------------------------------------------------------------
// stem32_pool_fwd_kernel: out [planes][Hp][Wp] from y0 [planes][H][W].  A workgroup works on chunk blockIdx.x % chunks of ONE
// plane (the channel operands are workgroup-uniform); a thread takes four consecutive output pixels of a row: 3 rows x 9
// columns of y0 from column 8 q - 1.
// ------------------------------------------------------------------------------------------------------
template <bool VIN, bool VOUT>
__global__ void __launch_bounds__(256)
stem32_pool_fwd_kernel(const float *__restrict__ y0, const float *__restrict__ mean, const float *__restrict__ invstd,
                       const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ out, int C,
                       int H, int W, int Hp, int Wp, int wq, int chunks) {
  const long plane = blockIdx.x / chunks;
  const int item = (int)(blockIdx.x % chunks) * 256 + (int)threadIdx.x;
  if (item >= wq * Hp) return;
  const int py = item / wq, px0 = (item - py * wq) * 4;
  const BnCh p = load_ch(mean, invstd, gamma, beta, (int)(plane % C));
  const float *src = y0 + plane * H * W;
  float a[3][9];
  unsigned in[3];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    float v[9];
    in[dy] = cdn::load_cols<9, 1, VIN>(src, 2 * py + dy - 1, H, W, 2 * px0, v);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      float xh;
      a[dy][j] = cdn::relu_keep_nan(bn_z(v[j], p, xh));
    }
  }
  float o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float m = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx)
        if ((in[dy] >> (2 * i + dx)) & 1u) {
          const float v = a[dy][2 * i + dx];
          m = (v > m || v != v) ? v : m;
        }
    o[i] = m;
  }
  cdn::store4<VOUT>(out + (plane * Hp + py) * Wp, Wp, px0, o);
}

// The gradient pixel (y, x) of a y0 plane gathers from g [Hp][Wp]: the windows that contain it are py in {y / 2, (y + 1) /
// 2}, px in {x / 2, (x + 1) / 2} (one or two each, by parity); each is scanned as the forward scans it.
__device__ __forceinline__ float pool_route_pixel(const float *__restrict__ src, const float *__restrict__ gs, int H, int W,
                                                  int Hp, int Wp, int y, int x, const BnCh &p) {
  float acc = 0.0f;
  for (int py = y >> 1; py <= ((y + 1) >> 1); ++py) {
    if (py >= Hp) continue;
    for (int px = x >> 1; px <= ((x + 1) >> 1); ++px) {
      if (px >= Wp) continue;
      float m = -INFINITY;
      int ay = -1, ax = -1;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int yy = 2 * py + dy - 1, xx = 2 * px + dx - 1;
          if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
            float xh;
            const float v = cdn::relu_keep_nan(bn_z(src[(long)yy * W + xx], p, xh));
            if (v > m || v != v) {
              m = v;
              ay = yy;
              ax = xx;
            }
          }
        }
      if (ay == y && ax == x) acc = acc + gs[(long)py * Wp + px];
    }
  }
  return acc;
}

// The same for the quad (y, x0 .. x0 + 3), x0 % 4 == 0, of a plane with W % 4 == 0: the windows of the quad lie in the patch
// of rows y - 1 .. y + 1 (y even: one window row) or y - 2 .. y + 2 (ODD: two) x columns x0 - 1 .. x0 + 5, formed once.
// G: the gathered gradients, own: the quad's stored y0.
template <bool ODD>
__device__ __forceinline__ void pool_route_quad(const float *__restrict__ src, const float *__restrict__ gs, int H, int W,
                                                int Hp, int Wp, int y, int x0, const BnCh &p, float (&G)[4],
                                                float (&own)[4]) {
  constexpr int NR = ODD ? 5 : 3, OR = ODD ? 2 : 1;      // patch rows; the quad's own row
  float a[NR][7];
  unsigned in[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    float v[7];
    in[r] = cdn::load_cols<7, 1, true>(src, y - OR + r, H, W, x0, v);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      float xh;
      a[r][j] = cdn::relu_keep_nan(bn_z(v[j], p, xh));
    }
    if (r == OR) {
#pragma unroll
      for (int i = 0; i < 4; ++i) own[i] = v[1 + i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) G[i] = 0.0f;
#pragma unroll
  for (int wy = 0; wy < (ODD ? 2 : 1); ++wy) {      // row-major window order
    const int py = (y >> 1) + wy;
    if (py >= Hp) continue;
#pragma unroll
    for (int wx = 0; wx < 3; ++wx) {
      const int px = (x0 >> 1) + wx;
      if (px >= Wp) continue;
      float m = -INFINITY;
      int arg = -1;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int r = 2 * wy + dy, c = 2 * wx + dx;
          if ((in[r] >> c) & 1u) {
            const float v = a[r][c];
            if (v > m || v != v) {
              m = v;
              arg = r * 7 + c;
            }
          }
        }
      const float gv = gs[(long)py * Wp + px];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (arg == OR * 7 + 1 + i) G[i] = G[i] + gv;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// stem32_pool_bwd_kernel: the first BatchNorm backward pass of one (channel, slab) of y0 [N][C][H][W] behind the pool --
// bn_bwd1_kernel's walk, the same terms in the same order, with G = the pool's gather from g [N][C][Hp][Wp] in place of a
// load; g_z = z > 0 ? G : 0 is stored.  part [C][slabs][2].  (The un-pooled stem is bn_bwd1_kernel<1, VEC, false> itself.)
// ------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(kBnThreads)
stem32_pool_bwd_kernel(const float *__restrict__ g, const float *__restrict__ y0, const float *__restrict__ mean,
                       const float *__restrict__ invstd, const float *__restrict__ gamma, const float *__restrict__ beta,
                       float *__restrict__ gz, double *__restrict__ part, int C, int H, int W, int Hp, int Wp, long n,
                       int slabs) {
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
    if (VEC) {      // the quad lies in one row
      const long off = ch_offset(j0, c, C, HW);
      const long plane = (unsigned)off / (unsigned)HW;
      const int pix = (int)((unsigned)off - (unsigned)plane * (unsigned)HW);
      const int y = (int)((unsigned)pix / (unsigned)W), x0 = pix - y * W;
      const float *src = y0 + plane * HW, *gs = g + plane * Hp * Wp;
      float v[4], G[4], o[4];
      if (y & 1)
        pool_route_quad<true>(src, gs, H, W, Hp, Wp, y, x0, p, G, v);
      else
        pool_route_quad<false>(src, gs, H, W, Hp, Wp, y, x0, p, G, v);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float xh;
        const float z = bn_z(v[e], p, xh);
        o[e] = z > 0.0f ? G[e] : 0.0f;
        t1 = t1 + (double)o[e];
        t2 = t2 + (double)o[e] * (double)xh;
      }
      *reinterpret_cast<float4 *>(gz + off) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      const int cnt = n - j0 < 4 ? (int)(n - j0) : 4;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) {
          const long off = ch_offset(j0 + e, c, C, HW);
          const long plane = (unsigned)off / (unsigned)HW;
          const int pix = (int)((unsigned)off - (unsigned)plane * (unsigned)HW);
          const int y = (int)((unsigned)pix / (unsigned)W), x = pix - y * W;
          const float Ge = pool_route_pixel(y0 + plane * HW, g + plane * Hp * Wp, H, W, Hp, Wp, y, x, p);
          float xh;
          const float z = bn_z(y0[off], p, xh);
          const float o = z > 0.0f ? Ge : 0.0f;
          gz[off] = o;
          t1 = t1 + (double)o;
          t2 = t2 + (double)o * (double)xh;
        }
    }
  }
  cdn::block_sums_store({t1, t2}, red, part);
}

// ------------------------------------------------------------------------------------------------------
// stem32_wgrad_kernel: the partial sums of grad_W of one channel group over one chunk of output positions (stem_wgrad_kernel's
// decomposition: a thread takes the positions chunk_start + t + 256 k, k < per_thread, in that order).  grad_y0 is formed on
// load: MASKED: g is g_z (the pool backward's output); !MASKED: g is grad_out and g_z = z > 0 ? g : 0.  SUB: batch statistics
// (the two subtracted terms); !SUB: eval mode.  part [groups][chunks][4][28].
// ------------------------------------------------------------------------------------------------------
template <bool MASKED, bool SUB>
__global__ void __launch_bounds__(256)
stem32_wgrad_kernel(const float *__restrict__ g, const float *__restrict__ y0, const float *__restrict__ img,
                    const float *__restrict__ mean, const float *__restrict__ invstd, const float *__restrict__ gamma,
                    const float *__restrict__ beta, const float *__restrict__ mb, const float *__restrict__ mg,
                    float *__restrict__ part, int H, int W, int Ho, int Wo, int stride, int chunks, int per_thread,
                    long positions) {
  __shared__ float red[4 * kS32Part];
  const int grp = (int)(blockIdx.x / chunks);
  const long start = (long)(blockIdx.x % chunks) * 256 * per_thread;
  const int HW = Ho * Wo;
  BnCh p[kS32Group];
  BnBwd2 q[kS32Group];
#pragma unroll
  for (int e = 0; e < kS32Group; ++e) {
    p[e] = load_ch(mean, invstd, gamma, beta, grp * kS32Group + e);
    q[e] = load_bwd2<SUB>(mean, invstd, gamma, mb, mg, grp * kS32Group + e);
  }
  float sums[kS32Part];      // [kS32Group][kS32Sums]
#pragma unroll
  for (int i = 0; i < kS32Part; ++i) sums[i] = 0.0f;
  for (int it = 0; it < per_thread; ++it) {
    const long pidx = start + (long)it * 256 + threadIdx.x;
    if (pidx < positions) {
      const int n = (int)(pidx / HW), pos = (int)(pidx - (long)n * HW);
      const int oy = pos / Wo, ox = pos - oy * Wo;
      float v[kS32Taps];
      cdn::load_stem_patch(img, n, oy, ox, H, W, stride, v);
      const long o = ((long)n * kS32Co + grp * kS32Group) * HW + pos;
#pragma unroll
      for (int e = 0; e < kS32Group; ++e) {
        const float gv = g[o + (long)e * HW], yv = y0[o + (long)e * HW];
        float xh;
        const float z = bn_z(yv, p[e], xh);
        const float gy = bn_grad_y<SUB>(MASKED ? gv : (z > 0.0f ? gv : 0.0f), yv, q[e]);
#pragma unroll
        for (int t = 0; t < kS32Taps; ++t) sums[e * kS32Sums + t] = fmaf(gy, v[t], sums[e * kS32Sums + t]);
      }
    }
  }
  cdn::block_sums_store(sums, red, part);
}

int stem32_pool_hw(int64_t v) { return (int)((v - 1) / 2 + 1); }

}  // namespace

extern "C" size_t cdn_codenet_stem_fp32_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || N * C * H * W >= (1ll << 31) ||
      C * cdn::ceil_div(N * H * W, kBnSlab) >= (1ll << 31))
    return 0;      // what bn_check_shape refuses
  return bn_plan(N, C, H, W).part_bytes;
}

extern "C" int cdn_codenet_stem_fp32_pool_forward(const float *y0, const float *mean, const float *invstd,
                                                  const float *gamma, const float *beta, float *out, int64_t N, int64_t C,
                                                  int64_t H, int64_t W, void *stream) {
  CDN_REQUIRE(y0 && mean && invstd && gamma && beta && out, CDN_ERR_ARG, "null pointer");
  if (int rc = bn_check_shape(N, C, H, W, 1)) return rc;
  const int Hp = stem32_pool_hw(H), Wp = stem32_pool_hw(W);
  const int wq = (int)cdn::ceil_div(Wp, 4);
  const int64_t chunks = cdn::ceil_div((int64_t)wq * Hp, 256);
  CDN_REQUIRE(N * C * chunks < (1ll << 31), CDN_ERR_UNSUPPORTED, "too many workgroups");
  const bool vin = (W & 3) == 0 && cdn::aligned16(y0), vout = (Wp & 3) == 0 && cdn::aligned16(out);
  const unsigned grid = (unsigned)(N * C * chunks);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_S32POOL(VI, VO)                                                                                                   \
  stem32_pool_fwd_kernel<VI, VO><<<grid, 256, 0, st>>>(y0, mean, invstd, gamma, beta, out, (int)C, (int)H, (int)W, Hp, Wp, wq, \
                                                       (int)chunks)
  if (vin && vout) CDN_S32POOL(true, true);
  else if (vin) CDN_S32POOL(true, false);
  else if (vout) CDN_S32POOL(false, true);
  else CDN_S32POOL(false, false);
#undef CDN_S32POOL
  return cdn::check_launch("codenet stem fp32 pool forward");
}

extern "C" int cdn_codenet_stem_fp32_pool_backward(const float *g, const float *y0, const float *mean, const float *invstd,
                                                   const float *gamma, const float *beta, float *g_z, float *grad_gamma,
                                                   float *grad_beta, float *mb, float *mg, int64_t N, int64_t C, int64_t H,
                                                   int64_t W, void *workspace, size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(g && y0 && mean && invstd && gamma && beta && g_z && grad_gamma && grad_beta && mb && mg && workspace,
              CDN_ERR_ARG, "null pointer");
  if (int rc = bn_check_shape(N, C, H, W, 1)) return rc;
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, cdn_codenet_stem_fp32_workspace_bytes(N, C, H, W))) return rc;
  const BnPlan p = bn_plan(N, C, H, W);
  const int Hp = stem32_pool_hw(H), Wp = stem32_pool_hw(W);
  double *part = static_cast<double *>(workspace);
  const unsigned grid = (unsigned)(C * p.slabs);
  hipStream_t st = cdn::as_stream(stream);
  if ((W & 3) == 0 && cdn::aligned16(y0) && cdn::aligned16(g_z))
    stem32_pool_bwd_kernel<true><<<grid, kBnThreads, 0, st>>>(g, y0, mean, invstd, gamma, beta, g_z, part, (int)C, (int)H,
                                                              (int)W, Hp, Wp, p.n, p.slabs);
  else
    stem32_pool_bwd_kernel<false><<<grid, kBnThreads, 0, st>>>(g, y0, mean, invstd, gamma, beta, g_z, part, (int)C, (int)H,
                                                               (int)W, Hp, Wp, p.n, p.slabs);
  launch_bn_bwd_finish(part, grad_gamma, grad_beta, mb, mg, C, p, st);
  return cdn::check_launch("codenet stem fp32 pool backward");
}

extern "C" int cdn_codenet_stem_fp32_bn_relu_backward_sums(const float *g, const float *y0, const float *mean,
                                                           const float *invstd, const float *gamma, const float *beta,
                                                           float *grad_gamma, float *grad_beta, float *mb, float *mg,
                                                           int64_t N, int64_t C, int64_t H, int64_t W, void *workspace,
                                                           size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(g && y0 && mean && invstd && gamma && beta && grad_gamma && grad_beta && mb && mg && workspace, CDN_ERR_ARG,
              "null pointer");
  if (int rc = bn_check_shape(N, C, H, W, 1)) return rc;
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, cdn_codenet_stem_fp32_workspace_bytes(N, C, H, W))) return rc;
  const BnPlan p = bn_plan(N, C, H, W);
  double *part = static_cast<double *>(workspace);
  const unsigned grid = (unsigned)(C * p.slabs);
  hipStream_t st = cdn::as_stream(stream);
  if ((W & 3) == 0 && cdn::aligned16(y0) && cdn::aligned16(g))
    bn_bwd1_kernel<1, true, false><<<grid, kBnThreads, 0, st>>>(g, y0, mean, invstd, gamma, beta, nullptr, part, (int)C,
                                                                (int)H, (int)W, p.n, p.slabs);
  else
    bn_bwd1_kernel<1, false, false><<<grid, kBnThreads, 0, st>>>(g, y0, mean, invstd, gamma, beta, nullptr, part, (int)C,
                                                                 (int)H, (int)W, p.n, p.slabs);
  launch_bn_bwd_finish(part, grad_gamma, grad_beta, mb, mg, C, p, st);
  return cdn::check_launch("codenet stem fp32 BatchNorm + ReLU backward sums");
}

extern "C" size_t cdn_codenet_stem_fp32_wgrad_workspace_bytes(int64_t N, int64_t H, int64_t W, int stride) {
  if (N <= 0 || H <= 0 || W <= 0 || (stride != 2 && stride != 4)) return 0;
  const cdn::StemPlan p = cdn::stem_plan(N, H, W, stride);
  if (N * 3 * H * W >= (1ll << 31) || N * kS32Co * p.Ho * p.Wo >= (1ll << 31)) return 0;
  return cdn::round256((size_t)(kS32Co / kS32Group) * (size_t)p.chunks * kS32Part * sizeof(float));
}

extern "C" int cdn_codenet_stem_fp32_wgrad(const float *g, int masked, const float *y0, const float *img, const float *mean,
                                           const float *invstd, const float *gamma, const float *beta, const float *mb,
                                           const float *mg, float *grad_w, int64_t N, int64_t H, int64_t W, int64_t Co,
                                           int stride, int training, void *workspace, size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(g && y0 && img && mean && invstd && gamma && beta && (!training || (mb && mg)) && grad_w && workspace,
              CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && H > 0 && W > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(Co == kS32Co, CDN_ERR_ARG, "the stem has 24 output channels, got %lld", (long long)Co);
  CDN_REQUIRE(stride == 2 || stride == 4, CDN_ERR_ARG, "stride must be 2 or 4, got %d", stride);
  const cdn::StemPlan p = cdn::stem_plan(N, H, W, stride);
  CDN_REQUIRE(N * 3 * H * W < (1ll << 31) && N * kS32Co * p.Ho * p.Wo < (1ll << 31), CDN_ERR_UNSUPPORTED, "shape too large");
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, cdn_codenet_stem_fp32_wgrad_workspace_bytes(N, H, W, stride)))
    return rc;
  float *part = static_cast<float *>(workspace);
  const unsigned grid = (unsigned)((kS32Co / kS32Group) * p.chunks);
  hipStream_t st = cdn::as_stream(stream);
#define CDN_S32WGRAD(MASKED, SUB)                                                                                            \
  stem32_wgrad_kernel<MASKED, SUB><<<grid, 256, 0, st>>>(g, y0, img, mean, invstd, gamma, beta, mb, mg, part, (int)H, (int)W, \
                                                         p.Ho, p.Wo, stride, p.chunks, p.per_thread, p.positions)
  if (masked) {
    if (training) CDN_S32WGRAD(true, true); else CDN_S32WGRAD(true, false);
  } else {
    if (training) CDN_S32WGRAD(false, true); else CDN_S32WGRAD(false, false);
  }
#undef CDN_S32WGRAD
  if (int rc = cdn::check_launch("codenet stem fp32 weight gradient")) return rc;
  return cdn::launch_sums_reduce(part, grad_w, nullptr, kS32Co, kS32Group, kS32Sums, 1, p.chunks, st,
                                 "codenet stem fp32 weight gradient reduce");
}
