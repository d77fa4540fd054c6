// codenet_layers.hip -- the layers AROUND the deform stages on the same kernel conventions (channels-last
// fp32 activations, fake-quantisation applied by the consumer while loading, QuantAct range tracking in the
// producer's epilogue by the last-arriving workgroup; cdn_common.h):
//   dw3_kernel         plain depthwise 3x3, stride 1 / 2, optional nearest x2 up-sampling by addressing
//                      (detection heads: SURVEY.md section 8f row 1; ShuffleNetV2 units: row 3)
//   interleave_kernel  concat + channel_shuffle(2) + the shared block-output QuantAct of a unit
//   stem_kernel        layer0: dense 3x3 conv 3 -> 24 on the NCHW image
// The pointwise convolutions of these layers are the stage's pointwise kernels (codenet_pointwise.hip,
// cdn_codenet_pointwise_nhwc_forward).
#include "cdn_common.h"

#include <algorithm>
#include <type_traits>

namespace {

using cdn::fake_quant;
using cdn::kMaxGrid;
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using v2f = __attribute__((ext_vector_type(2))) float;
#define CDN_STAMPR(R, I) do { } while (0)

// ------------------------------------------------------------------------------------------
// dw3: plain depthwise 3x3 (pad 1, stride 1 or 2) on a channels-last activation, optionally nearest x2
// up-sampled on the fly -- the detection heads' second layer applied to the hot path's
// half-resolution output (shufflenetv2_dcn.py:247-262, quant_modules.py:1059-1066) and the depthwise
// convs of the ShuffleNetV2 units (shufflenetv2_dcn.py:57-114; stride 2 in the down-sampling units).
//   a   [n][Hs*Ws][ld_in]   stored resolution, fake-quantised while staged when aq != NULL
//   out [n][Ho*Wo][ld_out]  v = sum_{dy,dx} w[c][dy][dx] * U[s*oy+dy-1][s*ox+dx-1] (+ bias) (* es + eh) (ReLU)
//        UP: U = nearest x2 of a (Ho = 2 Hs);  STRIDE 2: Ho = (Hs - 1) / 2 + 1
// ld_in / ld_out >= C are the row strides; channels [C, ld) of a are read (must be finite) and ignored.
// Workgroup = (image, band of 4 (stride 2: 2) output-side rows, 32 channels): the input rows of the band plus
// halo sit in LDS as [row][col][32] with zero halos; a lane owns (pixel, channel quad), reads its 3x3
// neighbourhood (9 ds_read_b128) and produces the 2x2 (UP) or 1 output pixels -- each as the nine
// products of the reference's conv in (dy, dx) order; up-sampling only decides which cell a tap reads.
// ------------------------------------------------------------------------------------------
constexpr int dw3_band(int stride) { return stride == 2 ? 2 : 4; }   // output-side rows per workgroup
template <bool XQ, int UP, int STRIDE, int CCH>
__global__ void __launch_bounds__(256)
dw3_kernel(const float *__restrict__ a, const unsigned *__restrict__ aq, const float *__restrict__ w,
           const float *__restrict__ bias, const float *__restrict__ ep_scale,
           const float *__restrict__ ep_shift, float *__restrict__ out, cdn::QUpdate qu,
           int C, int ld_in, int ld_out, int Hs, int Ws, int relu, int nbands,
           const unsigned char *__restrict__ agen) {
  extern __shared__ float4 band4[];         // [rows][Ws + 2][CCH / 4 quads]
  constexpr int LPP = CCH / 4;
  constexpr int BAND = dw3_band(STRIDE);
  constexpr int ROWS = STRIDE == 2 ? 2 * BAND + 1 : BAND + 2;
  const int band = blockIdx.x % nbands, c0 = (blockIdx.x / nbands) * CCH, n = blockIdx.y;
  const int y0 = band * BAND;                                  // first row of the band (pixel-item space)
  const int iy0 = STRIDE == 2 ? 2 * y0 - 1 : y0 - 1;           // first staged input row
  const int Wc = Ws + 2;
  const int tid = threadIdx.x;
  // a thread stages ONE channel quad (256 % LPP == 0), so its four quantiser parameters are loaded once;
  // agen != NULL: channel c uses the QuantAct state aq + 8 * agen[c] (mixed generations)
  float qs[4] = {1.f, 1.f, 1.f, 1.f}, qz[4] = {0.f, 0.f, 0.f, 0.f};
  if (XQ) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float *sp = reinterpret_cast<const float *>(aq);
      if (agen) sp += cdn::kQStateWords * agen[min(c0 + (tid % LPP) * 4 + e, C - 1)];
      qs[e] = sp[2];
      qz[e] = sp[3];
    }
  }
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int items = ROWS * Wc * LPP;
  for (int base = 0; base < items; base += 256 * 4) {
    float4 v[4];
    bool in[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = base + u * 256 + tid;
      const int cq = q % LPP, cell = q / LPP;
      const int r = cell / Wc, col = cell - r * Wc;
      const int y = iy0 + r, x = col - 1;
      v[u] = z4;
      in[u] = q < items && (unsigned)y < (unsigned)Hs && (unsigned)x < (unsigned)Ws &&
              c0 + cq * 4 + 3 < ld_in;
      if (in[u])
        v[u] = *reinterpret_cast<const float4 *>(a + ((long)n * Hs * Ws + (long)y * Ws + x) * ld_in + c0 + cq * 4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = base + u * 256 + tid;
      if (q < items) {
        float4 t = v[u];
        if (XQ && in[u]) {       // (the zero halo is a zero of the conv padding, not a quantised value)
          t.x = fake_quant(t.x, qs[0], qz[0]);
          t.y = fake_quant(t.y, qs[1], qz[1]);
          t.z = fake_quant(t.z, qs[2], qz[2]);
          t.w = fake_quant(t.w, qs[3], qz[3]);
        }
        band4[q] = t;
      }
    }
  }
  __syncthreads();
  // pixel items: stored pixels (UP / stride 1) or output pixels (stride 2)
  const int Hi = STRIDE == 2 ? (Hs - 1) / 2 + 1 : Hs, Wi = STRIDE == 2 ? (Ws - 1) / 2 + 1 : Ws;
  const int Ho = Hi << UP, Wo = Wi << UP;
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  const int work = BAND * Wi * LPP;
  // 256 threads = 256 / LPP pixels x LPP channel quads per pass: a thread keeps ONE channel quad, so its weights
  // are loaded once (not per item: 45 global loads per 9 LDS reads otherwise)
  const int cq = tid % LPP;
  const int cb = c0 + cq * 4;
  float wk[9][4], bs[4], es[4], eh[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const bool live = cb + e < C;
    const int c = min(cb + e, C - 1);
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k][e] = live ? w[(long)c * 9 + k] : 0.0f;
    bs[e] = (bias && live) ? bias[c] : 0.0f;
    es[e] = (ep_scale && live) ? ep_scale[c] : 1.0f;
    eh[e] = (ep_scale && live) ? ep_shift[c] : 0.0f;
  }
  for (int q = tid; q < work; q += 256) {
    const int pix = q / LPP;
    const int ry = pix / Wi, X = pix - ry * Wi;
    const int Y = y0 + ry;
    if (Y >= Hi || cb >= C) continue;
    float4 V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        V[i][j] = band4[((STRIDE * ry + i) * Wc + (STRIDE * X + j)) * LPP + cq];
#pragma unroll
    for (int py = 0; py < (1 << UP); ++py)
#pragma unroll
      for (int px = 0; px < (1 << UP); ++px) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            // full-resolution neighbour (2Y+py+dy-1, 2X+px+dx-1) -> stored cell relative to (Y-1, X-1)
            const int i = UP ? ((py + dy + 1) >> 1) : dy;
            const int j = UP ? ((px + dx + 1) >> 1) : dx;
            const float4 t = V[i][j];
            acc[0] = fmaf(wk[dy * 3 + dx][0], t.x, acc[0]);
            acc[1] = fmaf(wk[dy * 3 + dx][1], t.y, acc[1]);
            acc[2] = fmaf(wk[dy * 3 + dx][2], t.z, acc[2]);
            acc[3] = fmaf(wk[dy * 3 + dx][3], t.w, acc[3]);
          }
        float *op = out + ((long)n * Ho * Wo + (long)((Y << UP) + py) * Wo + (X << UP) + px) * ld_out + cb;
        float r4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = acc[e] + bs[e];
          if (ep_scale) v = fmaf(v, es[e], eh[e]);
          if (relu) v = cdn::relu_keep_nan(v);
          r4[e] = v;
        }
        if (out == nullptr) {
          // range-only pass (the fused head tail recomputes the values once the range is known)
        } else if (cb + 3 < ld_out && (ld_out & 3) == 0) {
          *reinterpret_cast<float4 *>(op) = make_float4(r4[0], r4[1], r4[2], r4[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (cb + e < C) op[e] = r4[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (cb + e < C) {          // padding channels do not take part in the range
            mn = fminf(mn, r4[e]);
            mx = fmaxf(mx, r4[e]);
            has_nan |= (r4[e] != r4[e]);
          }
      }
  }
  if (qu.tracks()) {
    __syncthreads();
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, qu,
                             reinterpret_cast<float *>(band4));
  }
}

// ------------------------------------------------------------------------------------------
// dws: the same depthwise 3x3 (stride 1 / 2, no up-sampling) as a ROW-STREAMING kernel for the backbone.
// dw3_kernel stages a band of 4 output rows + halo (6 input rows: 1.5x read amplification, 50 KiB of LDS at
// 64 px, three workgroups per CU) and runs load -> barrier -> compute -> store once per workgroup, so the
// memory pipe idles while it computes (measured 2.5 TB/s).  Here a workgroup = (image, CCH channels, strip
// of output rows) walks DOWN its strip: the input rows it needs next are in flight in registers while it
// computes the current output row from a ring of 3 + STRIDE rows in LDS -- every input row is read once
// (plus 2 halo rows per strip), one barrier per output row, 17-42 KiB of LDS.
// A thread owns one channel quad (weights and quantiser parameters in registers) and the pixels
// x = x_l + u * (256 / LPP) of a row, for loading and for computing alike.
// ------------------------------------------------------------------------------------------
template <bool XQ, int STRIDE, int CCH, int MAXL>
__global__ void __launch_bounds__(256)
dws_kernel(const float *__restrict__ a, const unsigned *__restrict__ aq, const unsigned char *__restrict__ agen,
           const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ ep_scale,
           const float *__restrict__ ep_shift, float *__restrict__ out, cdn::QUpdate qu,
           int C, int ld_in, int ld_out, int Hs, int Ws, int relu, int nstrips, int rps) {
  extern __shared__ float4 ring4[];         // [RING][Ws + 2][LPP]
  constexpr int LPP = CCH / 4, RING = 3 + STRIDE, XPT = 256 / LPP;
  constexpr int DEPTH = 3;                  // output rows whose input rows are in flight in registers
  const int strip = blockIdx.x % nstrips, c0 = (blockIdx.x / nstrips) * CCH, n = blockIdx.y;
  const int Ho = STRIDE == 2 ? (Hs - 1) / 2 + 1 : Hs, Wo = STRIDE == 2 ? (Ws - 1) / 2 + 1 : Ws;
  const int oy0 = strip * rps, oy1 = min(oy0 + rps, Ho);
  const int Wc = Ws + 2;
  const int tid = threadIdx.x, cq = tid % LPP, cb = c0 + cq * 4, x_l = tid / LPP;
  const bool quad_in = cb + 3 < ld_in;       // the quad can be loaded (channels >= C are finite padding)
  float qs[4] = {1.f, 1.f, 1.f, 1.f}, qz[4] = {0.f, 0.f, 0.f, 0.f}, qr[4] = {1.f, 1.f, 1.f, 1.f};
  // Prologue loads are branch-free and batched (clamped indices, values selected afterwards): a load in one arm of
  // a conditional is a branch and a wait of its own in the ISA -- 10-13 serialised round trips here before.
  if (XQ) {
    int gen[4] = {0, 0, 0, 0};
    if (agen) {
#pragma unroll
      for (int e = 0; e < 4; ++e) gen[e] = agen[min(cb + e, C - 1)];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float2 sz = *reinterpret_cast<const float2 *>(reinterpret_cast<const float *>(aq) +
                                                          cdn::kQStateWords * gen[e] + 2);
      qs[e] = sz.x;
      qz[e] = sz.y;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) qr[e] = __fdiv_rn(1.0f, qs[e]);
  }
  float wk[9][4], bs[4], es[4], eh[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = min(cb + e, C - 1);
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k][e] = w[(long)c * 9 + k];
    bs[e] = 0.0f;
    es[e] = 1.0f;
    eh[e] = 0.0f;
  }
  if (bias) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bs[e] = bias[min(cb + e, C - 1)];
  }
  if (ep_scale) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      es[e] = ep_scale[min(cb + e, C - 1)];
      eh[e] = ep_shift[min(cb + e, C - 1)];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (!(cb + e < C)) {                       // channels beyond C: zero weights, identity epilogue
#pragma unroll
      for (int k = 0; k < 9; ++k) wk[k][e] = 0.0f;
      bs[e] = 0.0f;
      es[e] = 1.0f;
      eh[e] = 0.0f;
    }
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = tid; i < RING * 2 * LPP; i += 256) {          // the zero halo columns of every ring slot
    const int slot = i / (2 * LPP), side = (i / LPP) & 1, q = i % LPP;
    ring4[(slot * Wc + (side ? Ws + 1 : 0)) * LPP + q] = z4;
  }
  const int r_first = STRIDE * oy0 - 1;                       // first input row of the strip (may be -1)
  const float *abase = a + (long)n * Hs * Ws * ld_in + (quad_in ? cb : 0);
  auto load_row = [&](int r, float4 (&d)[MAXL]) {
    const bool row_in = (unsigned)r < (unsigned)Hs && quad_in;
    const long rc = min(max(r, 0), Hs - 1);
#pragma unroll
    for (int u = 0; u < MAXL; ++u) {
      const int x = x_l + u * XPT;
      const float4 t = *reinterpret_cast<const float4 *>(abase + (rc * Ws + min(x, Ws - 1)) * ld_in);
      d[u] = (row_in && x < Ws) ? t : z4;
    }
  };
  auto write_row = [&](int r, int slot, const float4 (&d)[MAXL]) {
    const bool row_in = (unsigned)r < (unsigned)Hs && quad_in;   // rows outside are the conv's zero padding
#pragma unroll
    for (int u = 0; u < MAXL; ++u) {
      const int x = x_l + u * XPT;
      if (x < Ws) {
        float4 t = d[u];
        if (XQ && row_in) {
          t.x = cdn::fake_quant_r(t.x, qs[0], qz[0], qr[0]);
          t.y = cdn::fake_quant_r(t.y, qs[1], qz[1], qr[1]);
          t.z = cdn::fake_quant_r(t.z, qs[2], qz[2], qr[2]);
          t.w = cdn::fake_quant_r(t.w, qs[3], qz[3], qr[3]);
        }
        ring4[(slot * Wc + x + 1) * LPP + cq] = t;
      }
    }
  };
  float4 pre[DEPTH][STRIDE][MAXL];
  int wslot = 0;                                              // ring slot of the next row to write
  // step k (output row oy0 + k) consumes input rows r_first + (3 - STRIDE) + STRIDE * k + s, s < STRIDE
  const int r_step0 = r_first + (3 - STRIDE);
  if (oy0 < oy1) {
    // every load of the prologue goes out before the first row is consumed: load -> write -> load -> write cost the
    // workgroup 3 - STRIDE + 1 dependent memory round trips before its first output row (all workgroups of these
    // one-round launches start together, so the launch was that much longer)
    float4 pro[3 - STRIDE][MAXL];
#pragma unroll
    for (int p_ = 0; p_ < 3 - STRIDE; ++p_) load_row(r_first + p_, pro[p_]);
#pragma unroll
    for (int d_ = 0; d_ < DEPTH; ++d_)
      if (oy0 + d_ < oy1) {
#pragma unroll
        for (int s_ = 0; s_ < STRIDE; ++s_) load_row(r_step0 + STRIDE * d_ + s_, pre[d_][s_]);
      }
#pragma unroll
    for (int p_ = 0; p_ < 3 - STRIDE; ++p_) {
      write_row(r_first + p_, wslot, pro[p_]);
      wslot = wslot + 1 == RING ? 0 : wslot + 1;
    }
  }
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  int cslot = 0;                                              // ring slot of the first row of the 3x3 window
  for (int oyb = oy0; oyb < oy1; oyb += DEPTH) {
#pragma unroll
    for (int d_ = 0; d_ < DEPTH; ++d_) {
      const int oy = oyb + d_;
      if (oy < oy1) {                                         // workgroup-uniform
        const int base_r = r_step0 + STRIDE * (oy - oy0);
#pragma unroll
        for (int s_ = 0; s_ < STRIDE; ++s_) {
          write_row(base_r + s_, wslot, pre[d_][s_]);
          wslot = wslot + 1 == RING ? 0 : wslot + 1;
        }
        __syncthreads();
        if (oy + DEPTH < oy1) {
#pragma unroll
          for (int s_ = 0; s_ < STRIDE; ++s_) load_row(base_r + STRIDE * DEPTH + s_, pre[d_][s_]);
        }
        int rs[3];
        rs[0] = cslot;
        rs[1] = cslot + 1 >= RING ? cslot + 1 - RING : cslot + 1;
        rs[2] = cslot + 2 >= RING ? cslot + 2 - RING : cslot + 2;
        cslot = cslot + STRIDE >= RING ? cslot + STRIDE - RING : cslot + STRIDE;
#pragma unroll
        for (int u = 0; u < MAXL; ++u) {
          const int ox = x_l + u * XPT;
          if (ox < Wo && cb < C) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
              for (int dx = 0; dx < 3; ++dx) {
                const float4 t = ring4[(rs[dy] * Wc + STRIDE * ox + dx) * LPP + cq];
                acc[0] = fmaf(wk[dy * 3 + dx][0], t.x, acc[0]);
                acc[1] = fmaf(wk[dy * 3 + dx][1], t.y, acc[1]);
                acc[2] = fmaf(wk[dy * 3 + dx][2], t.z, acc[2]);
                acc[3] = fmaf(wk[dy * 3 + dx][3], t.w, acc[3]);
              }
            float r4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = acc[e] + bs[e];
              if (ep_scale) v = fmaf(v, es[e], eh[e]);
              if (relu) v = cdn::relu_keep_nan(v);
              r4[e] = v;
            }
            float *op = out + ((long)n * Ho * Wo + (long)oy * Wo + ox) * ld_out + cb;
            if (cb + 3 < ld_out && (ld_out & 3) == 0) {
              *reinterpret_cast<float4 *>(op) = make_float4(r4[0], r4[1], r4[2], r4[3]);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (cb + e < C) op[e] = r4[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (cb + e < C) {
                mn = fminf(mn, r4[e]);
                mx = fmaxf(mx, r4[e]);
                has_nan |= (r4[e] != r4[e]);
              }
          }
        }
      }
    }
  }
  if (qu.tracks()) {
    __syncthreads();
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, qu,
                             reinterpret_cast<float *>(ring4));
  }
}

// ------------------------------------------------------------------------------------------
// dwx: the row-streaming depthwise with the workgroup cut along x instead of along the channels.  With few
// channels per pixel (58 + 2 padding = 240 B, 116 = 464 B) a 16- or 32-channel chunk is a 64- or 128-byte
// piece of every pixel: the chunks of one pixel belong to different workgroups -- on different XCDs, i.e.
// different L2s -- so every cache line is fetched from HBM several times (measured 2.4 TB/s of algorithmic
// bytes at C = 58, 128 x 128, stride 2).  Here a workgroup = (image, strip of output columns, strip of output
// rows) takes ALL channels of its pixels: its loads are whole contiguous pixels, the only shared lines are
// the one halo column on each side.  LPP = ceil(C / 4) quads per pixel and XPT = 256 / LPP pixels per pass
// are run-time values (blockDim = XPT * LPP); a thread still owns one channel quad.  C <= 128 (used up to 64).
// ------------------------------------------------------------------------------------------
template <bool XQ, int STRIDE, int MAXL>
__global__ void __launch_bounds__(256)
dwx_kernel(const float *__restrict__ a, const unsigned *__restrict__ aq, const unsigned char *__restrict__ agen,
           const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ ep_scale,
           const float *__restrict__ ep_shift, float *__restrict__ out, cdn::QUpdate qu,
           int C, int ld_in, int ld_out, int Hs, int Ws, int relu, int nxs, int XSo, int nstrips, int rps,
           int LPP, int XPT) {
  extern __shared__ float4 ring4[];         // [RING][Wc][LPP]
  constexpr int RING = 3 + STRIDE, DEPTH = 3;
  const int xs = blockIdx.x % nxs, strip = blockIdx.x / nxs, n = blockIdx.y;
  const int Ho = STRIDE == 2 ? (Hs - 1) / 2 + 1 : Hs, Wo = STRIDE == 2 ? (Ws - 1) / 2 + 1 : Ws;
  const int oy0 = strip * rps, oy1 = min(oy0 + rps, Ho);
  const int ox0 = xs * XSo, nxo = min(XSo, Wo - ox0);          // output columns of this workgroup
  const int Wc = STRIDE * (XSo - 1) + 3;                       // staged input columns (ring row width)
  const int ix0 = STRIDE * ox0 - 1;                            // first staged input column (may be -1)
  const int tid = threadIdx.x, cq = tid % LPP, cb = cq * 4, x_l = tid / LPP;
  const bool quad_in = cb + 3 < ld_in;
  float qs[4] = {1.f, 1.f, 1.f, 1.f}, qz[4] = {0.f, 0.f, 0.f, 0.f}, qr[4] = {1.f, 1.f, 1.f, 1.f};
  // Prologue loads are branch-free and batched (clamped indices, values selected afterwards): a load in one arm of
  // a conditional is a branch and a wait of its own in the ISA -- 10-13 serialised round trips here before.
  if (XQ) {
    int gen[4] = {0, 0, 0, 0};
    if (agen) {
#pragma unroll
      for (int e = 0; e < 4; ++e) gen[e] = agen[min(cb + e, C - 1)];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float2 sz = *reinterpret_cast<const float2 *>(reinterpret_cast<const float *>(aq) +
                                                          cdn::kQStateWords * gen[e] + 2);
      qs[e] = sz.x;
      qz[e] = sz.y;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) qr[e] = __fdiv_rn(1.0f, qs[e]);
  }
  float wk[9][4], bs[4], es[4], eh[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = min(cb + e, C - 1);
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k][e] = w[(long)c * 9 + k];
    bs[e] = 0.0f;
    es[e] = 1.0f;
    eh[e] = 0.0f;
  }
  if (bias) {
#pragma unroll
    for (int e = 0; e < 4; ++e) bs[e] = bias[min(cb + e, C - 1)];
  }
  if (ep_scale) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      es[e] = ep_scale[min(cb + e, C - 1)];
      eh[e] = ep_shift[min(cb + e, C - 1)];
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (!(cb + e < C)) {                       // channels beyond C: zero weights, identity epilogue
#pragma unroll
      for (int k = 0; k < 9; ++k) wk[k][e] = 0.0f;
      bs[e] = 0.0f;
      es[e] = 1.0f;
      eh[e] = 0.0f;
    }
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int r_first = STRIDE * oy0 - 1;
  const float *abase = a + (long)n * Hs * Ws * ld_in + (quad_in ? cb : 0);
  auto load_row = [&](int r, float4 (&d)[MAXL]) {
    const bool row_in = (unsigned)r < (unsigned)Hs && quad_in;
    const long rc = min(max(r, 0), Hs - 1);
#pragma unroll
    for (int u = 0; u < MAXL; ++u) {
      const int col = x_l + u * XPT, x = ix0 + col;
      const float4 t = *reinterpret_cast<const float4 *>(abase + (rc * Ws + min(max(x, 0), Ws - 1)) * ld_in);
      d[u] = (row_in && col < Wc && (unsigned)x < (unsigned)Ws) ? t : z4;
    }
  };
  auto write_row = [&](int r, int slot, const float4 (&d)[MAXL]) {
    const bool row_in = (unsigned)r < (unsigned)Hs && quad_in;   // rows / columns outside: the conv's zero padding
#pragma unroll
    for (int u = 0; u < MAXL; ++u) {
      const int col = x_l + u * XPT, x = ix0 + col;
      if (col < Wc) {
        float4 t = d[u];
        if (XQ && row_in && (unsigned)x < (unsigned)Ws) {
          t.x = cdn::fake_quant_r(t.x, qs[0], qz[0], qr[0]);
          t.y = cdn::fake_quant_r(t.y, qs[1], qz[1], qr[1]);
          t.z = cdn::fake_quant_r(t.z, qs[2], qz[2], qr[2]);
          t.w = cdn::fake_quant_r(t.w, qs[3], qz[3], qr[3]);
        }
        ring4[(slot * Wc + col) * LPP + cq] = t;
      }
    }
  };
  float4 pre[DEPTH][STRIDE][MAXL];
  int wslot = 0;
  const int r_step0 = r_first + (3 - STRIDE);
  if (oy0 < oy1) {
    // every load of the prologue goes out before the first row is consumed: load -> write -> load -> write cost the
    // workgroup 3 - STRIDE + 1 dependent memory round trips before its first output row (all workgroups of these
    // one-round launches start together, so the launch was that much longer)
    float4 pro[3 - STRIDE][MAXL];
#pragma unroll
    for (int p_ = 0; p_ < 3 - STRIDE; ++p_) load_row(r_first + p_, pro[p_]);
#pragma unroll
    for (int d_ = 0; d_ < DEPTH; ++d_)
      if (oy0 + d_ < oy1) {
#pragma unroll
        for (int s_ = 0; s_ < STRIDE; ++s_) load_row(r_step0 + STRIDE * d_ + s_, pre[d_][s_]);
      }
#pragma unroll
    for (int p_ = 0; p_ < 3 - STRIDE; ++p_) {
      write_row(r_first + p_, wslot, pro[p_]);
      wslot = wslot + 1 == RING ? 0 : wslot + 1;
    }
  }
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  int cslot = 0;
  for (int oyb = oy0; oyb < oy1; oyb += DEPTH) {
#pragma unroll
    for (int d_ = 0; d_ < DEPTH; ++d_) {
      const int oy = oyb + d_;
      if (oy < oy1) {                                         // workgroup-uniform
        const int base_r = r_step0 + STRIDE * (oy - oy0);
#pragma unroll
        for (int s_ = 0; s_ < STRIDE; ++s_) {
          write_row(base_r + s_, wslot, pre[d_][s_]);
          wslot = wslot + 1 == RING ? 0 : wslot + 1;
        }
        __syncthreads();
        if (oy + DEPTH < oy1) {
#pragma unroll
          for (int s_ = 0; s_ < STRIDE; ++s_) load_row(base_r + STRIDE * DEPTH + s_, pre[d_][s_]);
        }
        int rs[3];
        rs[0] = cslot;
        rs[1] = cslot + 1 >= RING ? cslot + 1 - RING : cslot + 1;
        rs[2] = cslot + 2 >= RING ? cslot + 2 - RING : cslot + 2;
        cslot = cslot + STRIDE >= RING ? cslot + STRIDE - RING : cslot + STRIDE;
#pragma unroll
        for (int u = 0; u < MAXL; ++u) {
          const int oxl = x_l + u * XPT;
          if (oxl < nxo && cb < C) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
              for (int dx = 0; dx < 3; ++dx) {
                const float4 t = ring4[(rs[dy] * Wc + STRIDE * oxl + dx) * LPP + cq];
                acc[0] = fmaf(wk[dy * 3 + dx][0], t.x, acc[0]);
                acc[1] = fmaf(wk[dy * 3 + dx][1], t.y, acc[1]);
                acc[2] = fmaf(wk[dy * 3 + dx][2], t.z, acc[2]);
                acc[3] = fmaf(wk[dy * 3 + dx][3], t.w, acc[3]);
              }
            float r4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = acc[e] + bs[e];
              if (ep_scale) v = fmaf(v, es[e], eh[e]);
              if (relu) v = cdn::relu_keep_nan(v);
              r4[e] = v;
            }
            float *op = out + ((long)n * Ho * Wo + (long)oy * Wo + ox0 + oxl) * ld_out + cb;
            if (cb + 3 < ld_out && (ld_out & 3) == 0) {
              *reinterpret_cast<float4 *>(op) = make_float4(r4[0], r4[1], r4[2], r4[3]);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (cb + e < C) op[e] = r4[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (cb + e < C) {
                mn = fminf(mn, r4[e]);
                mx = fmaxf(mx, r4[e]);
                has_nan |= (r4[e] != r4[e]);
              }
          }
        }
      }
    }
  }
  if (qu.tracks()) {
    __syncthreads();
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, qu,
                             reinterpret_cast<float *>(ring4));
  }
}

// ------------------------------------------------------------------------------------------
// pwdwx (round 4; VERDICT r3 "next" #1b): the first 1x1 conv of a stride-2 ShuffleNetV2 unit RECOMPUTED inside its
// depthwise 3x3 (stride 2) instead of stored.  In layer 1 that tensor -- 58 channels at 128 x 128, fp32 because the
// range of the QuantAct behind it is only known once the whole batch has been computed -- is 243 MB at batch 64,
// written once and read once (pwi8_kernel 108 us + dwx_kernel 108 us).  The conv itself is tiny (K = 24): a range-only
// pass of the int8 pointwise kernel (no store) fixes the QuantAct, then this kernel -- dwx_kernel's structure: workgroup =
// (image, strip of output columns, strip of output rows), a ring of 3 + 2 input rows in LDS, all channels of a pixel in
// one workgroup -- PRODUCES its ring rows from the 24-channel input:
//   input row -> levels L = rint(s x - z) + z of the input QuantAct, a = L - 128 split into nibbles a = 16 a1 + a0
//   (both int8; pwi8_kernel's split), four channels packed per dword in LDS;
//   ring[col][quad] = fake_quant_a1( relu( fma( float(16 dot(a1, qw) + dot(a0, qw) + 128 colsum), 1 / (s sw), bias) ) )
//   with v_dot4c_i32_i8 -- the same exact integer sum and the same epilogue expression as pwi8_kernel, so the values in
//   the ring are bit for bit those dwx_kernel would load and fake-quantise from the stored tensor;
//   then dwx_kernel's nine-tap loop, epilogue and range tracking, unchanged.
// A batch whose input codes are too wide for the nibble split (state word [6]; a range that lags the batch by more than
// 8x) takes an fp32 branch: sum_c fq(x_c) * w'_c accumulated in channel order -- another valid evaluation of the
// reference's fp32 conv, not the integer one (pwi8_kernel's own wide branch is an f32-MFMA evaluation, also not).
// Cin <= 32 (a multiple of 4), C <= 128, stride 2.
// ------------------------------------------------------------------------------------------
template <int MAXL, int Q4T>      // Q4T: input channel quads per pixel the dot products run over (6: Cin <= 24, else 8)
__global__ void __launch_bounds__(256)
pwdwx_kernel(const float *__restrict__ x, const unsigned *__restrict__ xq, const signed char *__restrict__ Wq,
             const float *__restrict__ wscale, const int *__restrict__ wsum, const float *__restrict__ Wf,
             const float *__restrict__ pbias, const unsigned *__restrict__ mq, const float *__restrict__ w,
             const float *__restrict__ bias, float *__restrict__ out, cdn::QUpdate qu, int Cin, int Cpad,
             int C, int ld_x, int ld_out, int Hs, int Ws, int nxs, int XSo, int nstrips, int rps, int LPP, int XPT) {
  extern __shared__ float4 ring4[];         // [RING][Wc][LPP], then the code rows [2][Wc][24] dwords
  __shared__ unsigned s_wide_row[2];        // some code of the rows in flight does not fit int8 (-> nibble-split sums)
  constexpr int STRIDE = 2, RING = 3 + STRIDE, DEPTH = 3;
  const int xs = blockIdx.x % nxs, strip = blockIdx.x / nxs, n = blockIdx.y;
  const int Ho = (Hs - 1) / 2 + 1, Wo = (Ws - 1) / 2 + 1;
  const int oy0 = strip * rps, oy1 = min(oy0 + rps, Ho);
  const int ox0 = xs * XSo, nxo = min(XSo, Wo - ox0);
  const int Wc = STRIDE * (XSo - 1) + 3;
  const int ix0 = STRIDE * ox0 - 1;
  const int tid = threadIdx.x, cq = tid % LPP, cb = cq * 4, x_l = tid / LPP;
  const int nthreads = blockDim.x;
  // [2][Wc][24] dwords: nibble planes a0 (0..7) and a1 (8..15) of a = L - 128 = 16 a1 + a0, and the whole code a as a
  // byte (16..23) -- valid when every code of the two rows fits int8 (the usual case: levels inside the tracked range),
  // then ONE v_dot4c chain per channel instead of two
  unsigned *codes = reinterpret_cast<unsigned *>(ring4 + (size_t)RING * Wc * LPP);
  constexpr int CS = 24;
  const int Q4 = Cin >> 2;                                    // input channel quads per pixel (<= 8)
  // ---- constants: input quantiser, the mid QuantAct (known: the range pass ran before), weights of this quad ----
  const float xs_ = reinterpret_cast<const float *>(xq)[2], xz_ = reinterpret_cast<const float *>(xq)[3];
  const bool wide = xq[6] != 0u;
  const float ms_ = reinterpret_cast<const float *>(mq)[2], mz_ = reinterpret_cast<const float *>(mq)[3];
  const float mr_ = __fdiv_rn(1.0f, ms_);
  int wq[4][Q4T];
  float rinv[4], pb[4], wk[9][4], bs[4];
  int t128[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = min(cb + e, C - 1);
    const bool on = cb + e < C;
    // the channel's code row as two vector loads (rows are zero-padded to Cpad >= 64 bytes, so the quads past Cin
    // read zeros): one dword load per quad, each behind its own branch and `s_waitcnt vmcnt(0)` -- what the compiler
    // made of `(on && q < Q4) ? load : 0` -- cost the workgroup 24 dependent L2 round trips before its first row
    {
      const i32x4 lo = *reinterpret_cast<const i32x4 *>(Wq + (long)c * Cpad);
      const i32x4 hi = *reinterpret_cast<const i32x4 *>(Wq + (long)c * Cpad + 16);
      const int msk = on ? -1 : 0;
#pragma unroll
      for (int q = 0; q < Q4T; ++q) wq[e][q] = (q < 4 ? lo[q] : hi[q - 4]) & msk;
    }
    rinv[e] = __fdiv_rn(1.0f, __fmul_rn(xs_, wscale[c]));
    t128[e] = 128 * wsum[c];
    pb[e] = pbias ? pbias[c] : 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float t = w[(long)c * 9 + k];
      wk[k][e] = on ? t : 0.0f;
    }
    bs[e] = bias ? bias[c] : 0.0f;
    if (!on) bs[e] = 0.0f;
  }
  const int ioff = (int)xz_ + (2048 - 128) - 0x4B400000;
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int r_first = STRIDE * oy0 - 1;
  const int nitems = Wc * Q4;                                  // float4 items of one input row of this strip
  // ---- stage A: this thread's items of an input row (raw fp32, prefetched into registers) --------------------
  constexpr int MAXI = 2;                                      // items per thread and row (Wc * Q4 <= 512)
  auto load_row = [&](int r, float4 (&d)[MAXI]) {
    const long rc = min(max(r, 0), Hs - 1);
#pragma unroll
    for (int u = 0; u < MAXI; ++u) {
      const int it = min(tid + u * nthreads, nitems - 1);
      const int col = it / Q4, q4 = it - col * Q4;
      const int xg = min(max(ix0 + col, 0), Ws - 1);
      d[u] = *reinterpret_cast<const float4 *>(x + ((long)n * Hs * Ws + rc * Ws + xg) * ld_x + 4 * q4);
    }
  };
  // ---- stage B: levels -> nibble-split codes of the row, four channels per dword, into code buffer `cbuf` ------
  auto write_codes = [&](int cbuf, const float4 (&d)[MAXI], int par) {
#pragma unroll
    for (int u = 0; u < MAXI; ++u) {
      const int it = tid + u * nthreads;
      if (it < nitems) {
        const int col = it / Q4, q4 = it - col * Q4;
        const float v[4] = {d[u].x, d[u].y, d[u].z, d[u].w};
        unsigned lo = 0u, hi = 0u, full = 0u;
        bool fit = true;
        if (!wide) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)
            const float y_p = xs_ * v[e];
            const float y = (y_p - xz_) + 12582912.0f;           // rint by the 1.5 * 2^23 trick (pwi8_kernel's ucode)
            int uu = (int)__float_as_uint(y) + ioff;
            uu = min(max(uu, 8), 4087);
            lo |= (unsigned)(uu & 15) << (8 * e);
            hi |= (unsigned)(((uu >> 4) - 128) & 255) << (8 * e);
            full |= (unsigned)((uu - 2048) & 255) << (8 * e);
            fit = fit && (unsigned)(uu - (2048 - 128)) < 256u;
          }
          codes[(cbuf * Wc + col) * CS + q4] = lo;
          codes[(cbuf * Wc + col) * CS + 8 + q4] = hi;
          codes[(cbuf * Wc + col) * CS + 16 + q4] = full;
          if (!fit) atomicOr(&s_wide_row[par], 1u);
        } else {            // wide batch: the fake-quantised fp32 values themselves (two dwords hold two floats each way)
          float *cf = reinterpret_cast<float *>(codes + (size_t)2 * Wc * CS) + ((size_t)cbuf * Wc + col) * 32 + 4 * q4;
#pragma unroll
          for (int e = 0; e < 4; ++e) cf[e] = cdn::fake_quant_r(v[e], xs_, xz_, __fdiv_rn(1.0f, xs_));
        }
      }
    }
  };
  // ---- stage C: the 1x1 conv + ReLU + fake-quantisation of this thread's (column, quad) items -> ring row `slot` ----
  auto produce_row = [&](int r, int slot, int cbuf, int par) {
    const bool row_in = (unsigned)r < (unsigned)Hs;
    const bool fits8 = s_wide_row[par] == 0u;             // workgroup-uniform
#pragma unroll
    for (int u = 0; u < MAXL; ++u) {
      const int col = x_l + u * XPT, xg = ix0 + col;
      if (col < Wc) {
        float4 t = z4;                                           // outside the image: the depthwise conv's zero padding
        if (row_in && (unsigned)xg < (unsigned)Ws && cb < C) {
          float y[4];
          if (!wide && fits8) {
            const uint4 *cp = reinterpret_cast<const uint4 *>(codes + (cbuf * Wc + col) * CS + 16);
            const uint4 f0 = cp[0], f1 = cp[1];
            const int af[8] = {(int)f0.x, (int)f0.y, (int)f0.z, (int)f0.w, (int)f1.x, (int)f1.y, (int)f1.z, (int)f1.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              int sa = 0;
#pragma unroll
              for (int q = 0; q < Q4T; ++q) sa = __builtin_amdgcn_sdot4(af[q], wq[e][q], sa, false);
              y[e] = fmaf((float)(sa + t128[e]), rinv[e], pb[e]);      // the same integer: sum_c a_c qw_c
            }
          } else if (!wide) {
            const uint4 *cp = reinterpret_cast<const uint4 *>(codes + (cbuf * Wc + col) * CS);
            const uint4 l0 = cp[0], l1 = cp[1], h0 = cp[2], h1 = cp[3];
            const int a0[8] = {(int)l0.x, (int)l0.y, (int)l0.z, (int)l0.w, (int)l1.x, (int)l1.y, (int)l1.z, (int)l1.w};
            const int a1[8] = {(int)h0.x, (int)h0.y, (int)h0.z, (int)h0.w, (int)h1.x, (int)h1.y, (int)h1.z, (int)h1.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              int s0 = 0, s1 = 0;
#pragma unroll
              for (int q = 0; q < Q4T; ++q) {
                s0 = __builtin_amdgcn_sdot4(a0[q], wq[e][q], s0, false);
                s1 = __builtin_amdgcn_sdot4(a1[q], wq[e][q], s1, false);
              }
              y[e] = fmaf((float)(16 * s1 + s0 + t128[e]), rinv[e], pb[e]);
            }
          } else {
            const float *cf = reinterpret_cast<const float *>(codes + (size_t)2 * Wc * CS) + ((size_t)cbuf * Wc + col) * 32;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int c = min(cb + e, C - 1);
              float acc = 0.0f;
              for (int k = 0; k < Cin; ++k) acc = fmaf(cf[k], Wf[(long)c * Cin + k], acc);
              y[e] = acc + pb[e];
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = cdn::fake_quant_r(fmaxf(y[e], 0.0f), ms_, mz_, mr_);
          t = make_float4(y[0], y[1], y[2], y[3]);
        }
        ring4[(slot * Wc + col) * LPP + cq] = t;
      }
    }
  };
  float4 pre[DEPTH][STRIDE][MAXI];
  int wslot = 0;
  const int r_step0 = r_first + (3 - STRIDE);
  if (oy0 < oy1) {
    if (tid < 2) s_wide_row[tid] = 0u;
    __syncthreads();
    float4 pro[MAXI];
    load_row(r_first, pro);                                       // the one row in front of the first output row
#pragma unroll
    for (int d_ = 0; d_ < DEPTH; ++d_)                            // (and every prefetch row: one round trip, not two)
      if (oy0 + d_ < oy1) {
#pragma unroll
        for (int s_ = 0; s_ < STRIDE; ++s_) load_row(r_step0 + STRIDE * d_ + s_, pre[d_][s_]);
      }
    write_codes(0, pro, 0);
    __syncthreads();
    produce_row(r_first, wslot, 0, 0);
    wslot = 1;
    __syncthreads();                                              // code row 0 is read: the loop may overwrite it
  }
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  int cslot = 0, par = 1;                        // flag word of the rows in flight (the prologue row used word 0)
  for (int oyb = oy0; oyb < oy1; oyb += DEPTH) {
#pragma unroll
    for (int d_ = 0; d_ < DEPTH; ++d_) {
      const int oy = oyb + d_;
      if (oy < oy1) {                                         // workgroup-uniform
        const int base_r = r_step0 + STRIDE * (oy - oy0);
        // (no barrier needed here: the code rows were last read before the previous row's barrier, and the two ring
        // slots produced below are not among the three the previous row's taps read)
        write_codes(0, pre[d_][0], par);
        write_codes(1, pre[d_][1], par);
        __syncthreads();
        if (tid == 0) s_wide_row[par ^ 1] = 0u;           // last read before the previous row's barrier, next written
                                                          // after this row's
        if (oy + DEPTH < oy1) {
#pragma unroll
          for (int s_ = 0; s_ < STRIDE; ++s_) load_row(base_r + STRIDE * DEPTH + s_, pre[d_][s_]);
        }
#pragma unroll
        for (int s_ = 0; s_ < STRIDE; ++s_) {
          produce_row(base_r + s_, wslot, s_, par);
          wslot = wslot + 1 == RING ? 0 : wslot + 1;
        }
        par ^= 1;
        __syncthreads();
        int rs[3];
        rs[0] = cslot;
        rs[1] = cslot + 1 >= RING ? cslot + 1 - RING : cslot + 1;
        rs[2] = cslot + 2 >= RING ? cslot + 2 - RING : cslot + 2;
        cslot = cslot + STRIDE >= RING ? cslot + STRIDE - RING : cslot + STRIDE;
#pragma unroll
        for (int u = 0; u < MAXL; ++u) {
          const int oxl = x_l + u * XPT;
          if (oxl < nxo && cb < C) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
              for (int dx = 0; dx < 3; ++dx) {
                const float4 t = ring4[(rs[dy] * Wc + STRIDE * oxl + dx) * LPP + cq];
                acc[0] = fmaf(wk[dy * 3 + dx][0], t.x, acc[0]);
                acc[1] = fmaf(wk[dy * 3 + dx][1], t.y, acc[1]);
                acc[2] = fmaf(wk[dy * 3 + dx][2], t.z, acc[2]);
                acc[3] = fmaf(wk[dy * 3 + dx][3], t.w, acc[3]);
              }
            float r4[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) r4[e] = acc[e] + bs[e];
            float *op = out + ((long)n * Ho * Wo + (long)oy * Wo + ox0 + oxl) * ld_out + cb;
            if (cb + 3 < ld_out && (ld_out & 3) == 0) {
              *reinterpret_cast<float4 *>(op) = make_float4(r4[0], r4[1], r4[2], r4[3]);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (cb + e < C) op[e] = r4[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (cb + e < C) {
                mn = fminf(mn, r4[e]);
                mx = fmaxf(mx, r4[e]);
                has_nan |= (r4[e] != r4[e]);
              }
          }
        }
      }
    }
  }
  if (qu.tracks()) {
    __syncthreads();
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, qu,
                             reinterpret_cast<float *>(ring4));
  }
}

// ------------------------------------------------------------------------------------------
// interleave: the concat + channel_shuffle(groups = 2) that ends a ShuffleNetV2 unit
// (shufflenetv2_dcn.py:43-49; quant_modules.py:905-907), with the block-output QuantAct applied:
//     dst[m][2 i + 0] = fq_A(srcA[m][i])      dst[m][2 i + 1] = fq_B(srcB[m][i])        i < h
// Either source may be NULL (its slots are left untouched: the two branches of a stride-2 unit are
// quantised with DIFFERENT states of the shared QuantAct, so each is written right after its own range
// update); a NULL state copies the values (the pass-through half of a stride-1 unit is already
// quantised).  Elementwise, 8 bytes per lane, rows of any stride.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
interleave_kernel(const float *__restrict__ srcA, int ldA, const unsigned *__restrict__ qA,
                  const float *__restrict__ srcB, int ldB, const unsigned *__restrict__ qB,
                  float *__restrict__ dst, int ld_dst, long M, int h) {
  float as = 1.f, az = 0.f, bs = 1.f, bz = 0.f;
  if (qA) {
    as = reinterpret_cast<const float *>(qA)[2];
    az = reinterpret_cast<const float *>(qA)[3];
  }
  if (qB) {
    bs = reinterpret_cast<const float *>(qB)[2];
    bz = reinterpret_cast<const float *>(qB)[3];
  }
  // both sources present, even h, 8 / 16-byte aligned rows: two channel pairs per lane (float2 in, float4 out)
  const bool vec = srcA && srcB && (h & 1) == 0 && (ldA & 1) == 0 && (ldB & 1) == 0 && (ld_dst & 3) == 0 &&
                   ((reinterpret_cast<uintptr_t>(srcA) | reinterpret_cast<uintptr_t>(srcB)) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  if (vec) {
    const int h2 = h >> 1;
    const long total = M * h2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
      const long m = q / h2;
      const int i = (int)(q - m * h2) * 2;
      float2 va = *reinterpret_cast<const float2 *>(srcA + m * ldA + i);
      float2 vb = *reinterpret_cast<const float2 *>(srcB + m * ldB + i);
      if (qA) {
        va.x = fake_quant(va.x, as, az);
        va.y = fake_quant(va.y, as, az);
      }
      if (qB) {
        vb.x = fake_quant(vb.x, bs, bz);
        vb.y = fake_quant(vb.y, bs, bz);
      }
      *reinterpret_cast<float4 *>(dst + m * ld_dst + 2 * i) = make_float4(va.x, vb.x, va.y, vb.y);
    }
    return;
  }
  const long total = M * h;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
    const long m = q / h;
    const int i = (int)(q - m * h);
    float *d = dst + m * ld_dst + 2 * i;
    if (srcA) {
      const float v = srcA[m * ldA + i];
      d[0] = qA ? fake_quant(v, as, az) : v;
    }
    if (srcB) {
      const float v = srcB[m * ldB + i];
      d[1] = qB ? fake_quant(v, bs, bz) : v;
    }
  }
}

// ------------------------------------------------------------------------------------------
// stem: the network's first layer, a dense 3x3 conv 3 -> Co (stride 4 or 2, pad 1) + folded BN + ReLU on
// the NCHW image (shufflenetv2_dcn.py:205-214; W4A8: QuantBnConv2d(8) quantize_model.py:26-34), output
// channels-last.  One lane per output pixel: 27 inputs in registers, the Co x 27 weights read as
// wave-uniform (scalar) loads, Co accumulators; min/max of the output in the epilogue.
// ------------------------------------------------------------------------------------------
template <int CO>
__global__ void __launch_bounds__(256)
stem_kernel(const float *__restrict__ img, const float *__restrict__ w, const float *__restrict__ bias,
            float *__restrict__ out, cdn::QUpdate qu, int H, int W, int Ho, int Wo, int stride,
            int relu) {
  __shared__ float red[16];
  const int n = blockIdx.y;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  if (p < (long)Ho * Wo) {
    const int oy = (int)(p / Wo), ox = (int)(p - (long)oy * Wo);
    float v[27];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          // (round 4, measured and reverted: unconditional loads from clamped addresses, masked afterwards -- the remedy that
          // took dwq8_kernel's guarded loads from 80 to 14-23 us -- make THIS kernel slower: 78-90 us against 61-62 us
          // alone on the GPU, three interleaved pairs; the guarded form stays)
          const int y = oy * stride + dy - 1, x = ox * stride + dx - 1;
          v[(c * 3 + dy) * 3 + dx] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
                                         ? img[(((long)n * 3 + c) * H + y) * W + x] : 0.0f;
        }
    float *op = out + ((long)n * Ho * Wo + p) * CO;
    static_assert(CO % 4 == 0, "16-byte stores");
#pragma unroll
    for (int c4 = 0; c4 < CO; c4 += 4) {
      float r4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = c4 + e;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 27; ++k) acc = fmaf(w[co * 27 + k], v[k], acc);
        acc += bias ? bias[co] : 0.0f;
        if (relu) acc = cdn::relu_keep_nan(acc);
        r4[e] = acc;
        mn = fminf(mn, acc);
        mx = fmaxf(mx, acc);
        has_nan |= (acc != acc);
      }
      *reinterpret_cast<float4 *>(op + c4) = make_float4(r4[0], r4[1], r4[2], r4[3]);   // 96-byte pixel rows
    }
  }
  if (qu.tracks()) cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, qu, red);
}

constexpr int kHtLD = 48;      // bytes per A / B row of one 32-channel int8 k-step (32 + 16 pad): head_small_kernel
// most output channels of the fused head tail: four class groups of 32 on the matrix cores (54 KB of LDS per workgroup;
// a fifth group would pass the 64 KB a workgroup may hold together with the ring and the A planes)
constexpr int kHeadTailMaxClasses = 128;

// ------------------------------------------------------------------------------------------
// maxpool: MaxPool2d(3, stride 2, padding 1) of the "S2 + MaxPool" stems (shufflenetv2_dcn.py:209-214;
// W4A8: after ReLU + QuantAct, quantize_model.py:30-33), channels-last, one float4 of channels per lane.
// Fake-quantisation is monotone, so it is applied once to the window maximum (max fq(x) = fq(max x)).
// ------------------------------------------------------------------------------------------
template <bool XQ>
__global__ void __launch_bounds__(256)
maxpool_kernel(const float *__restrict__ a, const unsigned *__restrict__ aq, float *__restrict__ out, int C,
               int H, int W, int Ho, int Wo, long total) {
  float qs = 1.f, qz = 0.f;
  if (XQ) {
    qs = reinterpret_cast<const float *>(aq)[2];
    qz = reinterpret_cast<const float *>(aq)[3];
  }
  const int CQ = C >> 2;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
    const int cq = (int)(q % CQ);
    long pix = q / CQ;
    const int ox = (int)(pix % Wo);
    pix /= Wo;
    const int oy = (int)(pix % Ho), n = (int)(pix / Ho);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const int y = 2 * oy + dy - 1, x = 2 * ox + dx - 1;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
          const float4 v = *reinterpret_cast<const float4 *>(a + (((long)n * H + y) * W + x) * C + cq * 4);
          m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
        }
      }
    if (XQ) {
      m.x = fake_quant(m.x, qs, qz); m.y = fake_quant(m.y, qs, qz);
      m.z = fake_quant(m.z, qs, qz); m.w = fake_quant(m.w, qs, qz);
    }
    *reinterpret_cast<float4 *>(out + (((long)n * Ho + oy) * Wo + ox) * C + cq * 4) = m;
  }
}

// ------------------------------------------------------------------------------------------
// head_small: the tail of a W4A8 detection head with FEW output channels (wh, reg: 2) as a row-streaming
// VALU kernel, and the range pass in front of it (quant_modules.py:1062-1069):
//   MODE 0  range of ReLU(depthwise 3x3 on the nearest x2 up-sampled fq(y1) + b)      (the QuantAct's batch extremes)
//   MODE 1  the same values -> integer levels L = round(s*v - z) + z -> out[cls] = (sum_c L_c * qw[cls][c]) /
//           (s * sw[cls]) + b[cls], NCHW
// The 64-channel full-resolution tensor (268 MB per head at batch 64, written by dw3_kernel and re-read by
// the pointwise kernel in the unfused schedule) never exists.  head_tail_kernel does this on the int8 matrix
// cores for up to 32 classes, one stored row per workgroup with 3x re-staging (150 us); for <= 4 outputs the
// dot products are 4 FMAs per pixel and class on the VALU: exact (|L * qw| sums stay below 2^24, so the fp32
// sum IS the integer sum of pwi8_kernel and the result is bit-identical to the unfused path), reduced over
// the 16 lanes of a pixel with a 15-shuffle transpose-reduce.  Workgroup = (image, strip of 32 stored
// columns, strip of stored rows), ring of 4 stored rows in LDS (fake-quantised once), two rows in flight.
// C == 64: lane = (pixel x_l = tid / 16, channel quad cq = tid % 16).
//   MODE 2  MODE 1's result for up to kHeadTailMaxClasses classes on the int8 matrix cores, in G = ceil(classes / 32)
//           class groups (Pascal VOC's 20 classes: G = 1; COCO's 80: G = 3): the codes of a stored row's 2 x 32 output
//           pixels are parked as nibble planes A0 | A1, the weight codes of all groups as B0 | B1 (rows of kHtLD bytes,
//           rows cls >= classes zero), and the 2 G tiles (output row, class group) are spread over the four waves.
//           G is a template parameter so that G = 1 stays the code it was before there were groups.
// WB (MODE 2): width of the weight codes the caller vouches for.  4: |q| <= 8, the B1 plane holds 16 q in a byte.  8: any
// int8 code (W8A8) -- 16 q does not fit a byte, so there is no B1 plane: the a1 products get an accumulator of their own
// and the epilogue forms acc_lo + 16 acc_hi (int32, exact: K = 64, |acc_lo| <= 15 * 128 * 64, 16 |acc_hi| <= 2^25), the
// split of pwi8_kernel at that width.  (MODE 1 reads the codes as fp32 values at any width: its fp32 sums are the integer
// sums while sum |L q| < 2^24, which K = 64 and |q| <= 128 guarantee for |L| <= 2047.)
// Y8 (frozen serving mode): y1 holds the BYTE CODES of its QuantAct ([N][Hs*Ws][64] int8, written by the int8 pointwise
// kernel on codes) instead of fp32 pre-quantisation values: a lane loads one 4-byte code quad and the ring receives
// (q + zp) / scale -- the value fake_quant_r gives the fp32 element that produced the code, bit for bit.
// ------------------------------------------------------------------------------------------
template <int MODE, int NCLS, bool Y8 = false, int G = 1, int WB = 4>
__global__ void __launch_bounds__(256)
head_small_kernel(const float *__restrict__ y1, const unsigned *__restrict__ q1, const float *__restrict__ wdw,
                  const float *__restrict__ bdw, const unsigned *__restrict__ q2,
                  const signed char *__restrict__ Wq, const float *__restrict__ wscale,
                  const int *__restrict__ wsum, const float *__restrict__ bias, float *__restrict__ out,
                  cdn::QUpdate qu, int Hs, int Ws, int classes, int Cpad, int nxs, int XS,
                  int nstrips, int rps, int only_if_wide, unsigned *oflow = nullptr) {
  // MODE 2 (G groups of 32 classes on the int8 matrix cores) handles codes that fit the nibble split; a batch with
  // wider codes (state[6], the first calls of a fresh running range) is left to the MODE 1 launch behind it
  // (Y8, the serving schedule: frozen ranges have no wide batches -- state[6] is 0 by construction -- and the test would
  // be a memory round trip in front of everything else in a launch that is one resident set of workgroups)
  if (!Y8 && MODE == 2 && q2[6]) return;
  if (MODE == 1 && only_if_wide && !q2[6]) return;
  extern __shared__ float4 ring4[];          // [4][XS + 2][16]  (MODE 2: + A0 | A1 | B0 | B1 byte planes)
  constexpr int LPP = 16, XPT = 16, MAXL = 3, DEPTH = 2, NV = 4 * NCLS, C = 64;   // ring of 4 rows
  const int xs = blockIdx.x % nxs, strip = blockIdx.x / nxs, n = blockIdx.y;
  const int Y0 = strip * rps, Y1 = min(Y0 + rps, Hs);
  const int x0 = xs * XS, nx = min(XS, Ws - x0), Wc = XS + 2, ix0 = x0 - 1;
  const int tid = threadIdx.x, cq = tid & 15, x_l = tid >> 4, cb = cq * 4;
  const int lane = tid & 63, wave = tid >> 6;
  const float s1 = reinterpret_cast<const float *>(q1)[2], z1 = reinterpret_cast<const float *>(q1)[3];
  const float r1 = __fdiv_rn(1.0f, s1);
  float s2 = 1.f, z2 = 0.f;
  if (MODE != 0) {
    s2 = reinterpret_cast<const float *>(q2)[2];
    z2 = reinterpret_cast<const float *>(q2)[3];
  }
  v2f wlo[9], whi[9], blo, bhi;               // depthwise weights / bias of channels (0,1) and (2,3)
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    wlo[k] = (v2f){wdw[(long)(cb + 0) * 9 + k], wdw[(long)(cb + 1) * 9 + k]};
    whi[k] = (v2f){wdw[(long)(cb + 2) * 9 + k], wdw[(long)(cb + 3) * 9 + k]};
  }
  blo = (v2f){bdw ? bdw[cb + 0] : 0.0f, bdw ? bdw[cb + 1] : 0.0f};
  bhi = (v2f){bdw ? bdw[cb + 2] : 0.0f, bdw ? bdw[cb + 3] : 0.0f};
  // MODE 1: this lane's 4 channels of NCLS classes' weight codes, classes paired {qw[2p][e], qw[2p+1][e]};
  // lane cq stores value (cq & (NV-1)) = class (..>>2), pixel (py, px) of the class group being reduced
  v2f wq2[NCLS / 2][4];
  const int my_idx = cq & (NV - 1), my_cls = my_idx >> 2;
  const int ngroups = MODE == 1 ? (classes + NCLS - 1) / NCLS : 0;
  auto load_group = [&](int g0) {
    float wq[NCLS][4];
#pragma unroll
    for (int c_ = 0; c_ < NCLS; ++c_) {
      const int word = g0 + c_ < classes ? *reinterpret_cast<const int *>(Wq + (long)(g0 + c_) * Cpad + cb) : 0;
      wq[c_][0] = (float)((word << 24) >> 24);
      wq[c_][1] = (float)((word << 16) >> 24);
      wq[c_][2] = (float)((word << 8) >> 24);
      wq[c_][3] = (float)(word >> 24);
    }
#pragma unroll
    for (int cp = 0; cp < NCLS / 2; ++cp)
#pragma unroll
      for (int e = 0; e < 4; ++e) wq2[cp][e] = (v2f){wq[2 * cp][e], wq[2 * cp + 1][e]};
  };
  if (MODE == 1) load_group(0);
  float my_rinv = 0.f, my_bias = 0.f;                           // single class group: this lane's class
  if (MODE == 1 && ngroups == 1 && my_cls < classes) {
    my_rinv = __fdiv_rn(1.0f, __fmul_rn(s2, wscale[my_cls]));
    my_bias = bias ? bias[my_cls] : 0.0f;
  }
  // MODE 2: byte planes behind the ring; rows of one 32-channel k-step are kHtLD = 48 bytes (pwi8's layout)
  const int nrows = 4 * XS;                                     // output pixels of a stored row: 2 x 2 XS
  unsigned char *A0 = reinterpret_cast<unsigned char *>(ring4 + 4 * Wc * LPP);
  unsigned char *A1 = A0 + (size_t)2 * nrows * kHtLD;
  unsigned char *B0 = A1 + (size_t)2 * nrows * kHtLD;
  unsigned char *B1 = B0 + (size_t)G * 2 * 32 * kHtLD;          // per plane: G class groups of [k-step][32 classes]
  const int ioff = (int)z2 + (2048 - 128) - 0x4B400000;
  // MODE 2 matrix phase: a stored row has 2 G tiles (output row py, class group g) of 32 pixels x 32 classes; wave w
  // owns py = w & 1 and the groups (w >> 1) + 2 j, j < NJ -- all four waves from G = 2 on, and one read of the A
  // fragments serves every group of a wave (G = 1: waves 0 and 1 with group 0, as before there were groups)
  constexpr int NJ = (G + 1) / 2;
  const int mpy = G == 1 ? wave : (wave & 1);
  auto wave_group = [&](int j) { return G == 1 ? 0 : (wave >> 1) + 2 * j; };
  auto wave_has = [&](int j) { return G == 1 ? wave < 2 : ((G & 1) == 0 || j < NJ - 1 || wave < 2); };
  float e_rinv[NJ], e_bias[NJ];                                 // MODE 2 epilogue: this lane's class of group j
  int e_t128[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    e_rinv[j] = 0.f;
    e_bias[j] = 0.f;
    e_t128[j] = 0;
  }
  if (MODE == 2) {
    for (int q = tid; q < G * 2 * 32 * 2; q += 256) {           // group x k-step x class row x 16-byte piece
      const int g = q >> 7, ks = (q >> 6) & 1, row = (q >> 1) & 31, cls = 32 * g + row, part = (q & 1) * 16;
      i32x4 bq = (i32x4){0, 0, 0, 0};
      if (cls < classes) bq = *reinterpret_cast<const i32x4 *>(Wq + (long)cls * Cpad + ks * 32 + part);
      if constexpr (WB == 4) {
        i32x4 s16;
#pragma unroll
        for (int e = 0; e < 4; ++e) s16[e] = (int)(((unsigned)bq[e] << 4) & 0xF0F0F0F0u);
        *reinterpret_cast<i32x4 *>(B0 + ((g * 2 + ks) * 32 + row) * kHtLD + part) = bq;
        *reinterpret_cast<i32x4 *>(B1 + ((g * 2 + ks) * 32 + row) * kHtLD + part) = s16;
      } else {
        *reinterpret_cast<i32x4 *>(B0 + ((g * 2 + ks) * 32 + row) * kHtLD + part) = bq;
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int cls = 32 * wave_group(j) + (lane & 31);
      if ((G == 1 || wave_has(j)) && cls < classes) {
        e_rinv[j] = __fdiv_rn(1.0f, __fmul_rn(s2, wscale[cls]));
        e_bias[j] = bias ? bias[cls] : 0.0f;
        e_t128[j] = 128 * wsum[cls];
      }
    }
  }
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float *abase = y1 + (long)n * Hs * Ws * C + cb;
  const signed char *abase8 = reinterpret_cast<const signed char *>(y1) + (long)n * Hs * Ws * C + cb;
  auto load_row = [&](int r, float4 (&d)[MAXL]) {
    const bool row_in = (unsigned)r < (unsigned)Hs;
    (void)row_in;                              // (only the CDN_HS_GUARDED form reads it)
#pragma unroll
    for (int u = 0; u < MAXL; ++u) {
      const int col = x_l + u * XPT, x = ix0 + col;
      if (Y8) {      // (clamped address: an unconditional load; the mask is applied in write_row)
        const long pix = (long)min(max(r, 0), Hs - 1) * Ws + min(max(x, 0), Ws - 1);
        d[u].x = __uint_as_float(*reinterpret_cast<const unsigned *>(abase8 + pix * C));
      } else {
#ifdef CDN_HS_GUARDED
        d[u] = (row_in && col < Wc && (unsigned)x < (unsigned)Ws)
                   ? *reinterpret_cast<const float4 *>(abase + ((long)r * Ws + x) * C) : z4;
#else
        // (clamped address, masked in write_row: `cond ? *p : zero` compiles to a FLAT load whose address is selected
        // between global memory and a zero constant parked in scratch memory)
        const long pix = (long)min(max(r, 0), Hs - 1) * Ws + min(max(x, 0), Ws - 1);
        d[u] = *reinterpret_cast<const float4 *>(abase + pix * C);
#endif
      }
    }
  };
  auto write_row = [&](int r, int slot, const float4 (&d)[MAXL]) {
    const bool row_in = (unsigned)r < (unsigned)Hs;
#pragma unroll
    for (int u = 0; u < MAXL; ++u) {
      const int col = x_l + u * XPT, x = ix0 + col;
      if (col < Wc) {
        float4 t = d[u];
        const bool in = row_in && (unsigned)x < (unsigned)Ws;
        if (Y8) {
          const unsigned wd = __float_as_uint(d[u].x), mk = in ? 0xffffffffu : 0u;
          float e4[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float l = __fadd_rn((float)(int)(signed char)((wd >> (8 * e)) & 0xff), z1);
            const float q0 = __fmul_rn(l, r1);
            e4[e] = __uint_as_float(__float_as_uint(fmaf(fmaf(-q0, s1, l), r1, q0)) & mk);
          }
          t = make_float4(e4[0], e4[1], e4[2], e4[3]);
        } else if (in) {
          t.x = cdn::fake_quant_r(t.x, s1, z1, r1);
          t.y = cdn::fake_quant_r(t.y, s1, z1, r1);
          t.z = cdn::fake_quant_r(t.z, s1, z1, r1);
          t.w = cdn::fake_quant_r(t.w, s1, z1, r1);
        } else {
          t = z4;                              // the depthwise conv's zero padding
        }
        ring4[(slot * Wc + col) * LPP + cq] = t;
      }
    }
  };
  float4 pre[DEPTH][MAXL];
  int wslot = 0;
  if (Y0 < Y1) {
    float4 pro[2][MAXL];                      // stored rows Y0 - 1, Y0: all prologue loads in flight together
#pragma unroll
    for (int p_ = 0; p_ < 2; ++p_) load_row(Y0 - 1 + p_, pro[p_]);
#pragma unroll
    for (int d_ = 0; d_ < DEPTH; ++d_)
      if (Y0 + d_ < Y1) load_row(Y0 + 1 + d_, pre[d_]);
#pragma unroll
    for (int p_ = 0; p_ < 2; ++p_) {
      write_row(Y0 - 1 + p_, wslot, pro[p_]);
      wslot = (wslot + 1) & 3;
    }
  }
  float mn = INFINITY, mx = -INFINITY;
  bool has_nan = false;      // a NaN among the tracked values: fminf / fmaxf drop it, the reference's min() / max() do not
  int cslot = 0;
  unsigned clamped = 0;
  const int Ho = 2 * Hs, Wo = 2 * Ws;
  constexpr int NPASS = MODE == 2 ? 1 : 2;                      // MODE 2 runs on 16-column strips
  for (int Yb = Y0; Yb < Y1; Yb += DEPTH) {
#pragma unroll
    for (int d_ = 0; d_ < DEPTH; ++d_) {
      const int Y = Yb + d_;
      if (Y < Y1) {                                           // workgroup-uniform
        write_row(Y + 1, wslot, pre[d_]);
        wslot = (wslot + 1) & 3;
        __syncthreads();
        if (Y + DEPTH < Y1) load_row(Y + 1 + DEPTH, pre[d_]);
        const int rs0 = cslot, rs1 = (cslot + 1) & 3, rs2 = (cslot + 2) & 3;
        cslot = (cslot + 1) & 3;
#pragma unroll
        for (int u = 0; u < NPASS; ++u) {
          const int X = x_l + u * XPT;
          if (X < nx) {                                       // uniform over the 16 lanes of a pixel
            float4 V[3][3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              V[0][j] = ring4[(rs0 * Wc + X + j) * LPP + cq];
              V[1][j] = ring4[(rs1 * Wc + X + j) * LPP + cq];
              V[2][j] = ring4[(rs2 * Wc + X + j) * LPP + cq];
            }
            // packed fp32 math (v_pk_fma_f32: two FMAs per lane and instruction): channel pairs (0,1), (2,3)
            float Lv[4][4];                    // MODE 1: integer levels [py * 2 + px][channel]
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
              for (int px = 0; px < 2; ++px) {
                v2f alo = (v2f){0.f, 0.f}, ahi = (v2f){0.f, 0.f};
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                  for (int dx = 0; dx < 3; ++dx) {
                    const float4 t = V[(py + dy + 1) >> 1][(px + dx + 1) >> 1];
                    alo = __builtin_elementwise_fma(wlo[dy * 3 + dx], (v2f){t.x, t.y}, alo);
                    ahi = __builtin_elementwise_fma(whi[dy * 3 + dx], (v2f){t.z, t.w}, ahi);
                  }
                const v2f zero2 = (v2f){0.f, 0.f};
                const v2f vlo = __builtin_elementwise_max(alo + blo, zero2);
                const v2f vhi = __builtin_elementwise_max(ahi + bhi, zero2);
                const float v4[4] = {vlo.x, vlo.y, vhi.x, vhi.y};
                if (MODE == 0) {
                  mn = fminf(mn, fminf(fminf(v4[0], v4[1]), fminf(v4[2], v4[3])));
                  mx = fmaxf(mx, fmaxf(fmaxf(v4[0], v4[1]), fmaxf(v4[2], v4[3])));
                  has_nan |= __builtin_isunordered(v4[0], v4[1]) | __builtin_isunordered(v4[2], v4[3]);
                } else if (MODE == 1) {
#pragma unroll
                  for (int e = 0; e < 4; ++e) Lv[py * 2 + px][e] = __fadd_rn(cdn::quant_code(v4[e], s2, z2), z2);
                } else {
                  // codes as in pwi8_kernel: u = rint(s*v - z) + z - 128 + 2048, nibble split, k = channel
                  unsigned uc[4];
#pragma unroll
                  for (int e = 0; e < 4; ++e) {
#pragma clang fp contract(off)
                    const float yv_p = s2 * v4[e];      // (plain operators under fp contract(off): two roundings, cdn_common.h)
  const float yv = (yv_p - z2) + 12582912.0f;
                    int uu = (int)__float_as_uint(yv) + ioff;
                    if (Y8 && (uu < 8 || uu > 4087)) clamped = 1;   // (frozen: nobody measured this batch's extremes)
                    uc[e] = (unsigned)min(max(uu, 8), 4087);
                  }
                  const unsigned p01 = uc[0] | (uc[1] << 16), p23 = uc[2] | (uc[3] << 16);
                  const unsigned lo = __builtin_amdgcn_perm(p23, p01, 0x06040200u) & 0x0F0F0F0Fu;
                  const unsigned hi = __builtin_amdgcn_perm(p23 >> 4, p01 >> 4, 0x06040200u) ^ 0x80808080u;
                  const int row = py * 2 * XS + 2 * X + px;
                  const int off = ((cq >> 3) * nrows + row) * kHtLD + (cq & 7) * 4;
                  *reinterpret_cast<unsigned *>(A0 + off) = lo;
                  *reinterpret_cast<unsigned *>(A1 + off) = hi;
                }
              }
            if (MODE == 1) {
              for (int g = 0; g < ngroups; ++g) {
                if (ngroups > 1) load_group(g * NCLS);
                v2f part2[NV / 2];             // [(cls pair) * 4 + py * 2 + px] -> {cls 2p, cls 2p + 1}
#pragma unroll
                for (int i = 0; i < NV / 2; ++i) part2[i] = (v2f){0.f, 0.f};
#pragma unroll
                for (int pp = 0; pp < 4; ++pp)
#pragma unroll
                  for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int cp = 0; cp < NCLS / 2; ++cp)
                      part2[cp * 4 + pp] = __builtin_elementwise_fma((v2f){Lv[pp][e], Lv[pp][e]}, wq2[cp][e],
                                                                     part2[cp * 4 + pp]);
                // transpose-reduce over the pixel's 16 lanes: after the step with mask m a lane keeps the half
                // of its values selected by (cq & m); lane cq ends with the total of value cq & (NV - 1)
                float cur[NV];
#pragma unroll
                for (int cp = 0; cp < NCLS / 2; ++cp)
#pragma unroll
                  for (int i = 0; i < 4; ++i) {
                    cur[(2 * cp) * 4 + i] = part2[cp * 4 + i].x;
                    cur[(2 * cp + 1) * 4 + i] = part2[cp * 4 + i].y;
                  }
                if (NV == 8) {                                // 8 values on 16 lanes: fold the two halves first
#pragma unroll
                  for (int i = 0; i < NV; ++i) cur[i] += __shfl_xor(cur[i], 8, 64);
                }
#pragma unroll
                for (int hb = NV / 2; hb >= 1; hb >>= 1) {
                  const bool up = (cq & hb) != 0;
#pragma unroll
                  for (int i = 0; i < hb; ++i) {
                    const float send = up ? cur[i] : cur[i + hb];
                    const float keep = up ? cur[i + hb] : cur[i];
                    cur[i] = keep + __shfl_xor(send, hb, 64);
                  }
                }
                const int cls = g * NCLS + my_cls, py = (my_idx >> 1) & 1, px = my_idx & 1;
                if (cls < classes && cq < NV) {
                  float rinv = my_rinv, bv = my_bias;
                  if (ngroups > 1) {
                    rinv = __fdiv_rn(1.0f, __fmul_rn(s2, wscale[cls]));
                    bv = bias ? bias[cls] : 0.0f;
                  }
                  out[(((long)n * classes + cls) * Ho + 2 * Y + py) * Wo + 2 * (x0 + X) + px] =
                      fmaf(cur[0], rinv, bv);
                }
              }
            }
          }
        }
        if (MODE == 2) {
          __syncthreads();                                    // the codes of this stored row are parked
          if (G > 1 || wave < 2) {                            // row block = output row mpy, class groups wave_group(j)
            const int fo = (lane & 31) * kHtLD + (lane >> 5) * 16;
            i32x16 acc[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = (i32x16){0};
            i32x16 acch[WB == 8 ? NJ : 1];                    // WB = 8: the sums of the a1 plane
            if constexpr (WB == 8) {
#pragma unroll
              for (int j = 0; j < NJ; ++j) acch[j] = (i32x16){0};
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              const i32x4 a0 = *reinterpret_cast<const i32x4 *>(A0 + (ks * nrows + mpy * 2 * XS) * kHtLD + fo);
              const i32x4 a1 = *reinterpret_cast<const i32x4 *>(A1 + (ks * nrows + mpy * 2 * XS) * kHtLD + fo);
#pragma unroll
              for (int j = 0; j < NJ; ++j) {
                if (wave_has(j)) {                            // (wave-uniform; false only for the odd group of G = 3)
                  const int bo = ((wave_group(j) * 2 + ks) * 32) * kHtLD + fo;
                  const i32x4 b0 = *reinterpret_cast<const i32x4 *>(B0 + bo);
                  if constexpr (WB == 4) {
                    const i32x4 b1 = *reinterpret_cast<const i32x4 *>(B1 + bo);
                    acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[j], 0, 0, 0);
                  } else {
                    acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[j], 0, 0, 0);
                    acch[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acch[j], 0, 0, 0);
                  }
                }
              }
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
              const int cls = 32 * wave_group(j) + (lane & 31);
              if constexpr (WB == 8) acc[j] += 16 * acch[j];
              if (wave_has(j) && cls < classes) {
                float *orow = out + (((long)n * classes + cls) * Ho + 2 * Y + mpy) * Wo + 2 * x0;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                  const int px0 = 8 * g + 4 * (lane >> 5);
                  if (px0 < 2 * nx) {
                    float4 o;
                    o.x = fmaf((float)(acc[j][4 * g + 0] + e_t128[j]), e_rinv[j], e_bias[j]);
                    o.y = fmaf((float)(acc[j][4 * g + 1] + e_t128[j]), e_rinv[j], e_bias[j]);
                    o.z = fmaf((float)(acc[j][4 * g + 2] + e_t128[j]), e_rinv[j], e_bias[j]);
                    o.w = fmaf((float)(acc[j][4 * g + 3] + e_t128[j]), e_rinv[j], e_bias[j]);
                    *reinterpret_cast<float4 *>(orow + px0) = o;
                  }
                }
              }
            }
          }
        }
      }
    }
  }
  if (Y8 && MODE == 2 && clamped && oflow) atomicOr(oflow, 1u);
  if (MODE == 0 && qu.tracks()) {
    __syncthreads();
    cdn::block_minmax_finish(cdn::nan_lo(mn, has_nan), cdn::nan_hi(mx, has_nan), blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, qu,
                             reinterpret_cast<float *>(ring4));
  }
}

}  // namespace

extern "C" int cdn_codenet_dw3x3_nhwc_forward(
    const float *a, const void *a_qstate, int64_t N, int64_t C, int64_t H, int64_t W, int up, int stride,
    int64_t ld_in, int64_t ld_out, const float *w, const float *bias, const float *ep_scale,
    const float *ep_shift, int relu, float *r_min, float *r_max, void *r_state, int bits,
    double momentum, int running, void *workspace, size_t workspace_bytes, float *out, void *stream) {
  return cdn_codenet_dw3x3_mixed_forward(a, a_qstate, nullptr, N, C, H, W, up, stride, ld_in, ld_out, w, bias,
                                         ep_scale, ep_shift, relu, r_min, r_max, r_state, bits, momentum,
                                         running, workspace, workspace_bytes, out, stream);
}

extern "C" int cdn_codenet_dw3x3_mixed_forward(
    const float *a, const void *a_qstate, const unsigned char *a_gen, int64_t N, int64_t C, int64_t H,
    int64_t W, int up, int stride, int64_t ld_in, int64_t ld_out, const float *w, const float *bias,
    const float *ep_scale, const float *ep_shift, int relu, float *r_min, float *r_max, void *r_state,
    int bits, double momentum, int running, void *workspace, size_t workspace_bytes, float *out,
    void *stream) {
  CDN_REQUIRE(a && w && (out || r_state), CDN_ERR_ARG, "null pointer (out may be NULL only for a range-only pass)");
  CDN_REQUIRE(a_gen == nullptr || a_qstate != nullptr, CDN_ERR_ARG, "a_gen needs the states in a_qstate");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && (up == 0 || up == 1) && (stride == 1 || stride == 2),
              CDN_ERR_ARG, "bad size");
  CDN_REQUIRE(!(up && stride == 2), CDN_ERR_UNSUPPORTED, "up-sampling with stride 2");
  if (ld_in == 0) ld_in = C;
  if (ld_out == 0) ld_out = C;
  CDN_REQUIRE(ld_in >= C && ld_out >= C && (ld_in & 3) == 0, CDN_ERR_UNSUPPORTED,
              "channels-last depthwise needs row strides >= C and ld_in %% 4 == 0 (got %lld, %lld)",
              (long long)ld_in, (long long)ld_out);
  CDN_REQUIRE((reinterpret_cast<uintptr_t>(a) & 15) == 0, CDN_ERR_ARG, "a must be 16-byte aligned");
  CDN_REQUIRE((ep_scale == nullptr) == (ep_shift == nullptr), CDN_ERR_ARG,
              "ep_scale / ep_shift must both be set or both be NULL");
  CDN_REQUIRE((r_state == nullptr) == (r_min == nullptr) && (r_state == nullptr) == (r_max == nullptr),
              CDN_ERR_ARG, "the output QuantAct needs x_min, x_max and state together");
  // H, W: INPUT (stored) resolution; output = 2H x 2W (up), (H-1)/2+1 x (W-1)/2+1 (stride 2) or H x W
  const int Hs = (int)H, Ws = (int)W;
  const int Hi = stride == 2 ? (Hs - 1) / 2 + 1 : Hs;
  CDN_REQUIRE(N <= 65535 && N * std::max(ld_in, ld_out) * H * W * (up ? 4 : 1) < (1ll << 31),
              CDN_ERR_UNSUPPORTED, "shape too large");
  // ---- backbone form: row-streaming kernel (no up-sampling, values are written) ----------------------
  constexpr bool no_dws = false;
  if (!up && out && !no_dws && (out == nullptr || (reinterpret_cast<uintptr_t>(out) & 15) == 0 || (ld_out & 3))) {
    const int Ho_ = Hi;
    constexpr bool no_dwx = false;
    // measured (fake-quantising input): x strips win at 24 and 58 channels (76 vs 124 us at 58 ch, 128 x 128,
    // stride 2), channel chunks at 116 (128-byte pieces of 464-byte pixels: 27 vs 29 us, 53 vs 60 us)
    constexpr int dwx_max_c = 64;      // measured crossover between the x-strip and the channel-chunk kernel
    if (!no_dwx && C <= dwx_max_c && C <= 128) {
      // x-strip form: all channels of a pixel in one workgroup
      const int LPP = (int)cdn::ceil_div(C, 4), XPT = 256 / LPP;
      const int Wo_ = stride == 2 ? (Ws - 1) / 2 + 1 : Ws;
      const int ring = 3 + stride;
      // widest strip whose staged columns fit MAXL passes and ~40 KiB of LDS
      int best_maxl = 0, best_xso = 0;
      for (int maxl = 4; maxl >= 1; --maxl) {
        int xso = stride == 2 ? (maxl * XPT - 1) / 2 : maxl * XPT - 2;
        if (xso < 1) continue;
        xso = std::min(xso, Wo_);
        const int nxs_ = (int)cdn::ceil_div(Wo_, xso);
        xso = (int)cdn::ceil_div(Wo_, nxs_);                    // balanced strips
        const int wc = stride * (xso - 1) + 3;
        if ((size_t)ring * wc * LPP * 16 <= 40 * 1024 && cdn::ceil_div(wc, XPT) <= maxl) {
          best_maxl = (int)cdn::ceil_div(wc, XPT);
          best_xso = xso;
          break;
        }
      }
      if (best_maxl) {
        const int XSo = best_xso, nxs = (int)cdn::ceil_div(Wo_, XSo), wc = stride * (XSo - 1) + 3;
        const size_t lds = (size_t)ring * wc * LPP * 16;
#if !defined(CDN_DWX_WGPCU)
#define CDN_DWX_WGPCU 2
#endif
        constexpr int wg_per_cu = CDN_DWX_WGPCU;
        long want = cdn::ceil_div((long)wg_per_cu * cdn::kCUs, (long)N * nxs);
        int nstrips = (int)std::max<long>(1, std::min<long>(want, std::max(1, Ho_ / 8)));
        const int rps = (int)cdn::ceil_div(Ho_, nstrips);
        nstrips = (int)cdn::ceil_div(Ho_, rps);
        if ((long)nstrips * nxs * N <= kMaxGrid) {
          unsigned *arrive = r_state ? cdn::aux_workspace(workspace, workspace_bytes) : nullptr;
          CDN_REQUIRE(!r_state || arrive, CDN_ERR_WORKSPACE, "workspace missing, too small or not 256-byte aligned");
          hipStream_t st = cdn::as_stream(stream);
          const cdn::QUpdate qu = cdn::make_qupdate(r_min, r_max, r_state, arrive, bits, momentum, running);
          const unsigned *aq = static_cast<const unsigned *>(a_qstate);
          dim3 grid((unsigned)(nstrips * nxs), (unsigned)N);
          cdn::ProfScope ps(cdn::kProfDw, (int)(H > 0xffff ? 0xffff : H), st);
#define CDN_GOX(XQ_, ST_, ML_)                                                                          \
  dwx_kernel<XQ_, ST_, ML_><<<grid, XPT * LPP, lds, st>>>(a, aq, a_gen, w, bias, ep_scale, ep_shift, out, \
      qu, (int)C, (int)ld_in, (int)ld_out, Hs, Ws, relu, nxs, XSo, nstrips, rps, LPP, XPT)
#define CDN_GOX2(XQ_, ST_)                                                                              \
  do {                                                                                                  \
    if (best_maxl == 1) CDN_GOX(XQ_, ST_, 1);                                                           \
    else if (best_maxl == 2) CDN_GOX(XQ_, ST_, 2);                                                      \
    else if (best_maxl == 3) CDN_GOX(XQ_, ST_, 3);                                                      \
    else CDN_GOX(XQ_, ST_, 4);                                                                          \
  } while (0)
          if (aq && stride == 2) CDN_GOX2(true, 2);
          else if (aq) CDN_GOX2(true, 1);
          else if (stride == 2) CDN_GOX2(false, 2);
          else CDN_GOX2(false, 1);
#undef CDN_GOX2
#undef CDN_GOX
          return cdn::check_launch("codenet dw3x3 (x strips)");
        }
      }
    }
    // channels per workgroup: a thread covers pixels x_l + u * (256 / LPP), u < 4
    int cch = Ws <= 16 ? 64 : (Ws <= 128 ? 32 : 16);
    if (cch == 32 && Ws > 64) cch = 16;                           // keep the ring under ~42 KiB
    if (cch == 64 && C <= 32) cch = 32;
    const int xpt = 256 / (cch / 4);
    if (Ws <= 4 * xpt) {
      const int ring = 3 + stride;
      const size_t lds = (size_t)ring * (Ws + 2) * cch * sizeof(float);
      const int nchunks = (int)cdn::ceil_div(C, cch);
      // strips: enough workgroups to fill the chip twice, at least 8 output rows each
#if !defined(CDN_DWS_WGPCU)
#define CDN_DWS_WGPCU 2
#endif
      constexpr int wg_per_cu = CDN_DWS_WGPCU;
      long want = cdn::ceil_div((long)wg_per_cu * cdn::kCUs, (long)N * nchunks);
      int nstrips = (int)std::max<long>(1, std::min<long>(want, std::max(1, Ho_ / 8)));
      const int rps = (int)cdn::ceil_div(Ho_, nstrips);
      nstrips = (int)cdn::ceil_div(Ho_, rps);
      if ((long)nstrips * nchunks * N <= kMaxGrid && lds <= 64 * 1024) {
        unsigned *arrive = r_state ? cdn::aux_workspace(workspace, workspace_bytes) : nullptr;
        CDN_REQUIRE(!r_state || arrive, CDN_ERR_WORKSPACE, "workspace missing, too small or not 256-byte aligned");
        hipStream_t st = cdn::as_stream(stream);
        const cdn::QUpdate qu = cdn::make_qupdate(r_min, r_max, r_state, arrive, bits, momentum, running);
        const unsigned *aq = static_cast<const unsigned *>(a_qstate);
        dim3 grid((unsigned)(nstrips * nchunks), (unsigned)N);
        cdn::ProfScope ps(cdn::kProfDw, (int)(H > 0xffff ? 0xffff : H), st);
        const int maxl = (int)cdn::ceil_div(Ws, xpt);       // pixels of a row per thread: 1, 2 or 4
#define CDN_GOS(XQ_, ST_, CCH_)                                                                       \
  do {                                                                                                \
    if (maxl <= 1)                                                                                    \
      dws_kernel<XQ_, ST_, CCH_, 1><<<grid, 256, lds, st>>>(a, aq, a_gen, w, bias, ep_scale, ep_shift, out, \
          qu, (int)C, (int)ld_in, (int)ld_out, Hs, Ws, relu, nstrips, rps);                           \
    else if (maxl == 2)                                                                               \
      dws_kernel<XQ_, ST_, CCH_, 2><<<grid, 256, lds, st>>>(a, aq, a_gen, w, bias, ep_scale, ep_shift, out, \
          qu, (int)C, (int)ld_in, (int)ld_out, Hs, Ws, relu, nstrips, rps);                           \
    else                                                                                              \
      dws_kernel<XQ_, ST_, CCH_, 4><<<grid, 256, lds, st>>>(a, aq, a_gen, w, bias, ep_scale, ep_shift, out, \
          qu, (int)C, (int)ld_in, (int)ld_out, Hs, Ws, relu, nstrips, rps);                           \
  } while (0)
#define CDN_GOS2(XQ_, ST_)                                                                            \
  do {                                                                                                \
    if (cch == 64) CDN_GOS(XQ_, ST_, 64);                                                             \
    else if (cch == 32) CDN_GOS(XQ_, ST_, 32);                                                        \
    else CDN_GOS(XQ_, ST_, 16);                                                                       \
  } while (0)
        if (aq && stride == 2) CDN_GOS2(true, 2);
        else if (aq) CDN_GOS2(true, 1);
        else if (stride == 2) CDN_GOS2(false, 2);
        else CDN_GOS2(false, 1);
#undef CDN_GOS2
#undef CDN_GOS
        return cdn::check_launch("codenet dw3x3 (row streaming)");
      }
    }
  }
  const int bandr = dw3_band(stride);
  const int rows = stride == 2 ? 2 * bandr + 1 : bandr + 2;
  // 32 channels per workgroup; 16 when the band of a wide plane would leave one workgroup per CU
  // (layer1's stride-2 depthwise at 128 px per row: 83 KiB -> 220 us for 315 MB)
  const int cch = (size_t)rows * (Ws + 2) * 32 * sizeof(float) > 52 * 1024 ? 16 : 32;
  const size_t lds = (size_t)rows * (Ws + 2) * cch * sizeof(float);
  CDN_REQUIRE(lds <= 128 * 1024, CDN_ERR_UNSUPPORTED, "stored row of %d pixels too wide", Ws);
  const int nbands = (int)cdn::ceil_div(Hi, bandr), nchunks = (int)cdn::ceil_div(C, cch);
  CDN_REQUIRE((long)nbands * nchunks * N <= kMaxGrid, CDN_ERR_UNSUPPORTED, "too many workgroups");
  unsigned *arrive = r_state ? cdn::aux_workspace(workspace, workspace_bytes) : nullptr;
  CDN_REQUIRE(!r_state || arrive, CDN_ERR_WORKSPACE, "workspace missing, too small or not 256-byte aligned");
  hipStream_t st = cdn::as_stream(stream);
  const cdn::QUpdate qu = cdn::make_qupdate(r_min, r_max, r_state, arrive, bits, momentum, running);
  const unsigned *aq = static_cast<const unsigned *>(a_qstate);
  dim3 grid((unsigned)(nbands * nchunks), (unsigned)N);
  cdn::ProfScope ps(cdn::kProfDw, (int)(H > 0xffff ? 0xffff : H), st);
#define CDN_GO(XQ_, UP_, ST_)                                                                      \
  {                                                                                                \
    auto kern = cch == 32 ? dw3_kernel<XQ_, UP_, ST_, 32> : dw3_kernel<XQ_, UP_, ST_, 16>;         \
    (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,      \
                              (int)lds);                                                           \
    kern<<<grid, 256, lds, st>>>(a, aq, w, bias, ep_scale, ep_shift, out, qu, (int)C, (int)ld_in, \
                                 (int)ld_out, Hs, Ws, relu, nbands, a_gen);                        \
  }
  if (aq && up) CDN_GO(true, 1, 1)
  else if (aq && stride == 2) CDN_GO(true, 0, 2)
  else if (aq) CDN_GO(true, 0, 1)
  else if (up) CDN_GO(false, 1, 1)
  else if (stride == 2) CDN_GO(false, 0, 2)
  else CDN_GO(false, 0, 1)
#undef CDN_GO
  return cdn::check_launch("codenet dw3x3");
}

// dst[m][2i] = fq_A(srcA[m][i]), dst[m][2i+1] = fq_B(srcB[m][i]): see interleave_kernel.
extern "C" int cdn_codenet_interleave_forward(const float *srcA, int64_t ldA, const void *qA,
                                              const float *srcB, int64_t ldB, const void *qB,
                                              int64_t M, int64_t h, float *dst, int64_t ld_dst,
                                              void *stream) {
  CDN_REQUIRE(dst && (srcA || srcB), CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(M > 0 && h > 0 && ld_dst >= 2 * h && (!srcA || ldA >= h) && (!srcB || ldB >= h),
              CDN_ERR_ARG, "bad size");
  CDN_REQUIRE(M * ld_dst < (1ll << 40), CDN_ERR_UNSUPPORTED, "shape too large");
  hipStream_t st = cdn::as_stream(stream);
  const long total = (long)(M * h);
  const unsigned blocks = (unsigned)std::min<long>(cdn::ceil_div(total, 256), (long)cdn::kCUs * 32);
  interleave_kernel<<<blocks, 256, 0, st>>>(srcA, (int)ldA, static_cast<const unsigned *>(qA), srcB,
                                            (int)ldB, static_cast<const unsigned *>(qB), dst,
                                            (int)ld_dst, (long)M, (int)h);
  return cdn::check_launch("codenet interleave");
}

// Dense 3x3 conv 3 -> Co on the NCHW image, channels-last output: see stem_kernel.
extern "C" int cdn_codenet_stem_forward(const float *img, int64_t N, int64_t H, int64_t W, int64_t Co,
                                        int stride, const float *w, const float *bias, int relu,
                                        float *r_min, float *r_max, void *r_state, int bits,
                                        double momentum, int running, void *workspace,
                                        size_t workspace_bytes, float *out, void *stream) {
  CDN_REQUIRE(img && w && out, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && H > 0 && W > 0 && stride >= 1, CDN_ERR_ARG, "bad size");
  CDN_REQUIRE(Co == 24, CDN_ERR_UNSUPPORTED, "stem kernel is instantiated for 24 output channels (got %lld)",
              (long long)Co);
  CDN_REQUIRE((r_state == nullptr) == (r_min == nullptr) && (r_state == nullptr) == (r_max == nullptr),
              CDN_ERR_ARG, "the output QuantAct needs x_min, x_max and state together");
  const int Ho = (int)((H + 2 - 3) / stride + 1), Wo = (int)((W + 2 - 3) / stride + 1);
  dim3 grid((unsigned)cdn::ceil_div((long)Ho * Wo, 256), (unsigned)N);
  CDN_REQUIRE(N <= 65535 && (long)grid.x * grid.y <= kMaxGrid, CDN_ERR_UNSUPPORTED, "too many workgroups");
  unsigned *arrive = r_state ? cdn::aux_workspace(workspace, workspace_bytes) : nullptr;
  CDN_REQUIRE(!r_state || arrive, CDN_ERR_WORKSPACE, "workspace missing, too small or not 256-byte aligned");
  hipStream_t st = cdn::as_stream(stream);
  const cdn::QUpdate qu = cdn::make_qupdate(r_min, r_max, r_state, arrive, bits, momentum, running);
  stem_kernel<24><<<grid, 256, 0, st>>>(img, w, bias, out, qu, (int)H,
                                        (int)W, Ho, Wo, stride, relu);
  return cdn::check_launch("codenet stem");
}

// Range pass and tail of a W4A8 detection head: see head_small_kernel.
static int launch_head_small(int mode, const float *y1, const void *y1_qstate, int64_t N, int64_t C, int64_t Hs,
                             int64_t Ws, const float *w_dw, const float *b_dw, const void *y2_qstate,
                             const signed char *w_codes, const float *w_scale, const int *w_colsum,
                             const float *bias, int64_t classes, float *out_nchw, float *r_min, float *r_max,
                             void *r_state, int bits, double momentum, int running, void *workspace,
                             size_t workspace_bytes, void *stream, bool y8 = false,
                             unsigned *overflow = nullptr, int w_bits = 4) {
  CDN_REQUIRE(w_bits == 4 || w_bits == 8, CDN_ERR_ARG, "w_bits must be 4 or 8 (got %d)", w_bits);
  CDN_REQUIRE(y1 && y1_qstate && w_dw, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && Hs > 0 && Ws > 0 && N <= 65535, CDN_ERR_ARG, "bad size");
  CDN_REQUIRE(C == 64, CDN_ERR_UNSUPPORTED, "head_small is instantiated for 64 channels (got %lld)", (long long)C);
  CDN_REQUIRE((reinterpret_cast<uintptr_t>(y1) & 15) == 0, CDN_ERR_ARG, "y1 must be 16-byte aligned");
#ifndef CDN_HS_WGS_RANGE
#define CDN_HS_WGS_RANGE 4      /* 120 VGPRs, 35 KB of LDS: four workgroups per CU */
#endif
#ifndef CDN_HS_WGS_TAIL
#define CDN_HS_WGS_TAIL 3       /* 144-152 VGPRs: three (three heads, one box: 0.359-0.369 ms at 2 / 2, 0.352-0.355 at 4 / 3) */
#endif
  const int hs_wgs_mode = mode == 0 ? CDN_HS_WGS_RANGE : CDN_HS_WGS_TAIL;      // row strips: workgroups per CU
  constexpr int hs_minrows = 8;
  hipStream_t st = cdn::as_stream(stream);
  const unsigned *q1 = static_cast<const unsigned *>(y1_qstate);
  // geometry for strips of XS stored columns, hs_wgs resident workgroups per CU
  auto geom = [&](int XS, int hs_wgs, int *nxs, int *nstrips, int *rps, size_t *lds, dim3 *grid) {
    *nxs = (int)cdn::ceil_div(Ws, XS);
    long want = cdn::ceil_div((long)hs_wgs * cdn::kCUs, (long)N * *nxs);
    *nstrips = (int)std::max<long>(1, std::min<long>(want, std::max<long>(1, Hs / hs_minrows)));
    *rps = (int)cdn::ceil_div(Hs, *nstrips);
    *nstrips = (int)cdn::ceil_div(Hs, *rps);
    *lds = (size_t)4 * (XS + 2) * 16 * 16;
    *grid = dim3((unsigned)(*nstrips * *nxs), (unsigned)N);
    return (long)*nstrips * *nxs * N <= kMaxGrid;
  };
  int nxs, nstrips, rps;
  size_t lds;
  dim3 grid;
  const int XS = (int)std::min<int64_t>(32, Ws);
  CDN_REQUIRE(geom(XS, hs_wgs_mode, &nxs, &nstrips, &rps, &lds, &grid), CDN_ERR_UNSUPPORTED, "too many workgroups");
  cdn::ProfScope ps(cdn::kProfDw, (int)Hs, st);
  if (mode == 0) {
    CDN_REQUIRE(r_min && r_max && r_state, CDN_ERR_ARG, "the range pass needs x_min, x_max and state");
    unsigned *arrive = cdn::aux_workspace(workspace, workspace_bytes);
    CDN_REQUIRE(arrive, CDN_ERR_WORKSPACE, "workspace missing, too small or not 256-byte aligned");
    const cdn::QUpdate qu = cdn::make_qupdate(r_min, r_max, r_state, arrive, bits, momentum, running);
    head_small_kernel<0, 2><<<grid, 256, lds, st>>>(y1, q1, w_dw, b_dw, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                    nullptr, qu, (int)Hs, (int)Ws, 0, 0, nxs, XS, nstrips,
                                                    rps, 0);
    return cdn::check_launch("codenet head range");
  }
  CDN_REQUIRE(y2_qstate && w_codes && w_scale && out_nchw, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(classes >= 1 && classes <= kHeadTailMaxClasses, CDN_ERR_UNSUPPORTED,
              "head tail handles 1..%d output channels (got %lld)", kHeadTailMaxClasses, (long long)classes);
  CDN_REQUIRE((reinterpret_cast<uintptr_t>(w_codes) & 15) == 0, CDN_ERR_ARG, "w_codes must be 16-byte aligned");
  const int Cpad = (int)((C + 63) / 64 * 64);
  const cdn::QUpdate none = cdn::no_qupdate();
  const unsigned *q2 = static_cast<const unsigned *>(y2_qstate);
  // matrix cores whenever the shape allows (measured at 2 classes: 64 us vs 74 us for the VALU form, which
  // remains for other widths and as the wide-code fallback)
  constexpr bool hs_no_mfma = false;
  const bool mfma_ok = !hs_no_mfma && w_colsum && (Ws & 15) == 0 &&
                       (reinterpret_cast<uintptr_t>(out_nchw) & 15) == 0;
  auto tail = [&](auto y8c) -> int {
    constexpr bool Y8 = decltype(y8c)::value;
    if (mfma_ok) {
    } else if (classes <= 2) {
      head_small_kernel<1, 2, Y8><<<grid, 256, lds, st>>>(y1, q1, w_dw, b_dw, q2, w_codes, w_scale, nullptr, bias,
                                                          out_nchw, none, (int)Hs, (int)Ws, (int)classes, Cpad,
                                                          nxs, XS, nstrips, rps, 0);
      return cdn::check_launch("codenet head tail (small)");
    }
    if (classes <= 4 && !mfma_ok) {
      head_small_kernel<1, 4, Y8><<<grid, 256, lds, st>>>(y1, q1, w_dw, b_dw, q2, w_codes, w_scale, nullptr, bias,
                                                          out_nchw, none, (int)Hs, (int)Ws, (int)classes, Cpad,
                                                          nxs, XS, nstrips, rps, 0);
      return cdn::check_launch("codenet head tail (small)");
    }
    // int8 matrix cores on 16-column strips; a batch whose codes are too wide for the nibble
    // split (state[6]) is computed by the VALU kernel launched behind it (4 classes at a time)
    CDN_REQUIRE(mfma_ok, CDN_ERR_UNSUPPORTED,
                "more than 4 classes need w_colsum, Ws %% 16 == 0 and a 16-byte aligned output");
    auto matrix = [&](auto gc) -> int {
      constexpr int G = decltype(gc)::value;                  // class groups of 32
      // ring (18 KB) + A planes (12 KB) + 6 KB of B planes per class group: 36 / 42 / 48 / 54 KB.  The grid is sized
      // for the workgroups a CU really holds -- by the registers three up to two groups (144-156 VGPRs) and two from
      // three groups on (172-192: a second accumulator tile per wave), by the 160 KB of LDS 4 / 3 / 3 / 2
      // (8-bit weight codes: a second accumulator tile per group -- 160-164 VGPRs on byte-code input, still three;
      // 172-176 on fp32 input, two; 204-252 from three groups on, two)
      const int by_regs = (G <= 2 && !(w_bits == 8 && !Y8)) ? CDN_HS_WGS_TAIL : 2;
      // (8-bit codes: no B1 plane, half the bytes per class group -- B1 lies behind B0, so the kernel's pointers hold)
      const size_t planes = (size_t)2 * 2 * (4 * 16) * kHtLD + (size_t)G * (w_bits == 8 ? 1 : 2) * 2 * 32 * kHtLD;
      const size_t ring = (size_t)4 * (16 + 2) * 16 * 16;
      const int fit = (int)std::min<size_t>(by_regs, ((size_t)160 * 1024) / (ring + planes + 512));
      int nxs2, nstrips2, rps2;
      size_t lds2;
      dim3 grid2;
      CDN_REQUIRE(geom(16, fit, &nxs2, &nstrips2, &rps2, &lds2, &grid2), CDN_ERR_UNSUPPORTED, "too many workgroups");
      lds2 += planes;
      auto kern = w_bits == 8 ? head_small_kernel<2, 2, Y8, G, 8> : head_small_kernel<2, 2, Y8, G, 4>;
      if (G > 1)
        (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
      kern<<<grid2, 256, lds2, st>>>(y1, q1, w_dw, b_dw, q2, w_codes, w_scale, w_colsum, bias, out_nchw, none, (int)Hs,
                                     (int)Ws, (int)classes, Cpad, nxs2, 16, nstrips2, rps2, 0, overflow);
      return CDN_OK;
    };
    static_assert(kHeadTailMaxClasses == 4 * 32, "one instantiation per number of class groups");
    int rc_m;
    switch ((int)((classes + 31) / 32)) {
      case 1: rc_m = matrix(std::integral_constant<int, 1>{}); break;
      case 2: rc_m = matrix(std::integral_constant<int, 2>{}); break;
      case 3: rc_m = matrix(std::integral_constant<int, 3>{}); break;
      default: rc_m = matrix(std::integral_constant<int, 4>{}); break;
    }
    if (rc_m != CDN_OK) return rc_m;
    // the wide-code fallback behind it -- never on byte-code input: frozen ranges have no wide batches (state[6] is 0 by
    // construction, a saturating code raises the overflow flag instead), and the early-exit launch still cost 14 us per
    // head in the serving network's kernel trace
    if (!Y8)
      head_small_kernel<1, 4, Y8><<<grid, 256, lds, st>>>(y1, q1, w_dw, b_dw, q2, w_codes, w_scale, nullptr, bias,
                                                          out_nchw, none, (int)Hs, (int)Ws, (int)classes, Cpad,
                                                          nxs, XS, nstrips, rps, 1);
    return cdn::check_launch("codenet head tail (matrix cores)");
  };
  return y8 ? tail(std::true_type{}) : tail(std::false_type{});
}

extern "C" int cdn_codenet_head_range_forward(const float *y1, const void *y1_qstate, int64_t N, int64_t C,
                                              int64_t Hs, int64_t Ws, const float *w_dw, const float *b_dw,
                                              float *r_min, float *r_max, void *r_state, int bits, double momentum,
                                              int running, void *workspace, size_t workspace_bytes, void *stream) {
  return launch_head_small(0, y1, y1_qstate, N, C, Hs, Ws, w_dw, b_dw, nullptr, nullptr, nullptr, nullptr, nullptr,
                           0, nullptr, r_min, r_max, r_state, bits, momentum, running, workspace, workspace_bytes,
                           stream);
}

extern "C" int cdn_codenet_head_tail_max_classes(void) { return kHeadTailMaxClasses; }

extern "C" int cdn_codenet_head_tail_small_forward(const float *y1, const void *y1_qstate, int64_t N, int64_t C,
                                                   int64_t Hs, int64_t Ws, const float *w_dw, const float *b_dw,
                                                   const void *y2_qstate, const signed char *w_codes,
                                                   const float *w_scale, const int *w_colsum, const float *bias,
                                                   int64_t classes, float *out_nchw, void *stream) {
  return launch_head_small(1, y1, y1_qstate, N, C, Hs, Ws, w_dw, b_dw, y2_qstate, w_codes, w_scale, w_colsum, bias,
                           classes, out_nchw, nullptr, nullptr, nullptr, 8, 0.99, 0, nullptr, 0, stream);
}

extern "C" int cdn_codenet_head_tail_small_q8_forward(const signed char *y1_codes, const void *y1_qstate, int64_t N,
                                                      int64_t C, int64_t Hs, int64_t Ws, const float *w_dw,
                                                      const float *b_dw, const void *y2_qstate,
                                                      const signed char *w_codes, const float *w_scale,
                                                      const int *w_colsum, const float *bias, int64_t classes,
                                                      float *out_nchw, unsigned *overflow, void *stream) {
  CDN_REQUIRE(overflow, CDN_ERR_ARG, "null pointer");
  return launch_head_small(1, reinterpret_cast<const float *>(y1_codes), y1_qstate, N, C, Hs, Ws, w_dw, b_dw, y2_qstate,
                           w_codes, w_scale, w_colsum, bias, classes, out_nchw, nullptr, nullptr, nullptr, 8, 0.99, 0,
                           nullptr, 0, stream, true, overflow);
}

extern "C" int cdn_codenet_head_tail_small_w_forward(const float *y1, const void *y1_qstate, int64_t N, int64_t C,
                                                     int64_t Hs, int64_t Ws, const float *w_dw, const float *b_dw,
                                                     const void *y2_qstate, const signed char *w_codes,
                                                     const float *w_scale, const int *w_colsum, const float *bias,
                                                     int64_t classes, float *out_nchw, int w_bits, void *stream) {
  return launch_head_small(1, y1, y1_qstate, N, C, Hs, Ws, w_dw, b_dw, y2_qstate, w_codes, w_scale, w_colsum, bias,
                           classes, out_nchw, nullptr, nullptr, nullptr, 8, 0.99, 0, nullptr, 0, stream, false, nullptr,
                           w_bits);
}

extern "C" int cdn_codenet_head_tail_small_q8_w_forward(const signed char *y1_codes, const void *y1_qstate, int64_t N,
                                                        int64_t C, int64_t Hs, int64_t Ws, const float *w_dw,
                                                        const float *b_dw, const void *y2_qstate,
                                                        const signed char *w_codes, const float *w_scale,
                                                        const int *w_colsum, const float *bias, int64_t classes,
                                                        float *out_nchw, unsigned *overflow, int w_bits, void *stream) {
  CDN_REQUIRE(overflow, CDN_ERR_ARG, "null pointer");
  return launch_head_small(1, reinterpret_cast<const float *>(y1_codes), y1_qstate, N, C, Hs, Ws, w_dw, b_dw, y2_qstate,
                           w_codes, w_scale, w_colsum, bias, classes, out_nchw, nullptr, nullptr, nullptr, 8, 0.99, 0,
                           nullptr, 0, stream, true, overflow, w_bits);
}

// out[n][oy*Wo+ox][c] = max_{3x3, stride 2, pad 1} fq(a[n][..][c]): see maxpool_kernel.
extern "C" int cdn_codenet_maxpool3x3s2_nhwc_forward(const float *a, const void *a_qstate, int64_t N, int64_t C,
                                                     int64_t H, int64_t W, float *out, void *stream) {
  CDN_REQUIRE(a && out, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && (C & 3) == 0, CDN_ERR_ARG, "bad size (C %% 4 == 0)");
  CDN_REQUIRE((reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
              CDN_ERR_ARG, "a / out must be 16-byte aligned");
  const int Ho = (int)((H - 1) / 2 + 1), Wo = (int)((W - 1) / 2 + 1);
  const long total = (long)N * Ho * Wo * (C / 4);
  hipStream_t st = cdn::as_stream(stream);
  const unsigned blocks = (unsigned)std::min<long>(cdn::ceil_div(total, 256), (long)cdn::kCUs * 32);
  if (a_qstate)
    maxpool_kernel<true><<<blocks, 256, 0, st>>>(a, static_cast<const unsigned *>(a_qstate), out, (int)C, (int)H,
                                                 (int)W, Ho, Wo, total);
  else
    maxpool_kernel<false><<<blocks, 256, 0, st>>>(a, nullptr, out, (int)C, (int)H, (int)W, Ho, Wo, total);
  return cdn::check_launch("codenet maxpool");
}

// First 1x1 conv (+ ReLU + QuantAct) of a stride-2 unit recomputed inside its depthwise 3x3 (pwdwx_kernel): a range-only
// pass of the int8 pointwise kernel updates the mid QuantAct, then the fused kernel writes the depthwise output and
// tracks the range of the QuantAct behind it.  See include/codenet_dcn.h.
extern "C" int cdn_codenet_pwdw_s2_supported(int64_t N, int64_t Cin, int64_t C, int64_t H, int64_t W) {
  if (N <= 0 || N > 65535 || Cin < 4 || Cin > 32 || (Cin & 3) || C < 4 || C > 128 || H < 2 || W < 2) return 0;
  const int LPP = (int)cdn::ceil_div(C, 4), XPT = 256 / LPP;
  const int Wo = (int)((W - 1) / 2 + 1);
  for (int maxl = 4; maxl >= 1; --maxl) {
    int xso = (maxl * XPT - 1) / 2;
    if (xso < 1) continue;
    xso = std::min(xso, Wo);
    xso = (int)cdn::ceil_div(Wo, cdn::ceil_div(Wo, xso));
    const int wc = 2 * (xso - 1) + 3;
    if ((size_t)5 * wc * LPP * 16 + (size_t)wc * 448 <= 56 * 1024 && cdn::ceil_div(wc, XPT) <= maxl &&
        wc * (Cin / 4) <= 2 * XPT * LPP)
      return 1;
  }
  return 0;
}

static int pwdw_s2_impl(
    bool range_pass, const float *x, const void *x_qstate, int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t ld_x,
    const float *w_pw, const signed char *w_pw_codes, const float *w_pw_scale, const int *w_pw_colsum,
    const float *bias_pw, float *m_min, float *m_max, void *m_state, int64_t C, const float *w_dw, const float *bias_dw,
    int64_t ld_out, float *r_min, float *r_max, void *r_state, int bits, double momentum, int running, void *workspace,
    size_t workspace_bytes, float *out, void *stream) {
  CDN_REQUIRE(x && x_qstate && w_pw && w_pw_codes && w_pw_scale && w_pw_colsum && m_min && m_max && m_state && w_dw && out,
              CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE((r_state == nullptr) == (r_min == nullptr) && (r_state == nullptr) == (r_max == nullptr), CDN_ERR_ARG,
              "the output QuantAct needs x_min, x_max and state together");
  CDN_REQUIRE(cdn_codenet_pwdw_s2_supported(N, Cin, C, H, W), CDN_ERR_UNSUPPORTED, "shape outside the fused pw -> dw kernel");
  CDN_REQUIRE(ld_x >= Cin && (ld_x & 3) == 0 && ld_out >= C && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(w_pw_codes) & 15) == 0, CDN_ERR_ARG, "bad row stride / alignment");
  // running | CDN_W_CODES_8BIT: the width of w_pw_codes, for the range-only pass (the recomputing kernel applies the 16
  // to the sum of the high plane and needs no flag)
  const int wflag = running & CDN_W_CODES_8BIT;
  running &= ~CDN_W_CODES_8BIT;
  // 1. the 1x1 conv as a RANGE-ONLY pass (out = NULL): batch extremes of relu(conv) -> the mid QuantAct
  const int64_t M = N * H * W;
  int rc = 0;
  if (range_pass)
    rc = cdn_codenet_pointwise_mixed_forward(x, x_qstate, nullptr, M, Cin, C, ld_x, 0, w_pw, w_pw_codes, w_pw_scale,
                                             w_pw_colsum, bias_pw, nullptr, nullptr, 1 | wflag, nullptr, m_min, m_max, m_state,
                                             bits, momentum, running, workspace, workspace_bytes, nullptr, stream);
  if (rc) return rc;
  // 2. conv recomputed into the ring rows of the stride-2 depthwise
  const int Hs = (int)H, Ws = (int)W, Ho = (Hs - 1) / 2 + 1, Wo = (Ws - 1) / 2 + 1;
  const int LPP = (int)cdn::ceil_div(C, 4), XPT = 256 / LPP;
  int best_maxl = 0, XSo = 0;
  for (int maxl = 4; maxl >= 1; --maxl) {
    int xso = (maxl * XPT - 1) / 2;
    if (xso < 1) continue;
    xso = std::min(xso, Wo);
    xso = (int)cdn::ceil_div(Wo, cdn::ceil_div(Wo, xso));
    const int wc = 2 * (xso - 1) + 3;
    if ((size_t)5 * wc * LPP * 16 + (size_t)wc * 448 <= 56 * 1024 && cdn::ceil_div(wc, XPT) <= maxl &&
        wc * (Cin / 4) <= 2 * XPT * LPP) {
      best_maxl = (int)cdn::ceil_div(wc, XPT);
      XSo = xso;
      break;
    }
  }
  const int nxs = (int)cdn::ceil_div(Wo, XSo), wc = 2 * (XSo - 1) + 3;
  const size_t lds = (size_t)5 * wc * LPP * 16 + (size_t)wc * 448;
#ifndef CDN_PWDWX_WGPCU
#define CDN_PWDWX_WGPCU 2     /* 223-250 VGPRs: two workgroups per CU, so whole rounds of 2 x 256 (3 x 256 workgroups ran as
                                 one and a half rounds: 173 -> 160 us for the range pass + this kernel, same box) */
#endif
  long want = cdn::ceil_div((long)CDN_PWDWX_WGPCU * cdn::kCUs, (long)N * nxs);
  int nstrips = (int)std::max<long>(1, std::min<long>(want, std::max(1, Ho / 8)));
  const int rps = (int)cdn::ceil_div(Ho, nstrips);
  nstrips = (int)cdn::ceil_div(Ho, rps);
  CDN_REQUIRE((long)nstrips * nxs * N <= kMaxGrid, CDN_ERR_UNSUPPORTED, "too many workgroups");
  unsigned *arrive = r_state ? cdn::aux_workspace(workspace, workspace_bytes) : nullptr;
  CDN_REQUIRE(!r_state || arrive, CDN_ERR_WORKSPACE, "workspace missing, too small or not 256-byte aligned");
  hipStream_t st = cdn::as_stream(stream);
  const cdn::QUpdate qu = cdn::make_qupdate(r_min, r_max, r_state, arrive, bits, momentum, running);
  const int Cpad = (int)((Cin + 63) / 64 * 64);
  dim3 grid((unsigned)(nstrips * nxs), (unsigned)N);
#define CDN_GOPD1(ML_, Q_)                                                                                     \
  pwdwx_kernel<ML_, Q_><<<grid, XPT * LPP, lds, st>>>(x, static_cast<const unsigned *>(x_qstate), w_pw_codes, w_pw_scale, \
      w_pw_colsum, w_pw, bias_pw, static_cast<const unsigned *>(m_state), w_dw, bias_dw, out, qu, (int)Cin, Cpad, \
      (int)C, (int)ld_x, (int)ld_out, Hs, Ws, nxs, XSo, nstrips, rps, LPP, XPT)
#define CDN_GOPD(ML_)                  \
  do {                                 \
    if (Cin <= 24) CDN_GOPD1(ML_, 6);  \
    else CDN_GOPD1(ML_, 8);            \
  } while (0)
  if (best_maxl == 1) CDN_GOPD(1);
  else if (best_maxl == 2) CDN_GOPD(2);
  else if (best_maxl == 3) CDN_GOPD(3);
  else CDN_GOPD(4);
#undef CDN_GOPD
#undef CDN_GOPD1
  return cdn::check_launch("codenet pw -> dw (stride 2, conv recomputed)");
}

extern "C" int cdn_codenet_pwdw_s2_forward(
    const float *x, const void *x_qstate, int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t ld_x,
    const float *w_pw, const signed char *w_pw_codes, const float *w_pw_scale, const int *w_pw_colsum,
    const float *bias_pw, float *m_min, float *m_max, void *m_state, int64_t C, const float *w_dw, const float *bias_dw,
    int64_t ld_out, float *r_min, float *r_max, void *r_state, int bits, double momentum, int running, void *workspace,
    size_t workspace_bytes, float *out, void *stream) {
  return pwdw_s2_impl(true, x, x_qstate, N, Cin, H, W, ld_x, w_pw, w_pw_codes, w_pw_scale, w_pw_colsum, bias_pw, m_min, m_max,
                      m_state, C, w_dw, bias_dw, ld_out, r_min, r_max, r_state, bits, momentum, running, workspace,
                      workspace_bytes, out, stream);
}

// The second half alone: the caller has run the range-only pass itself (cdn_codenet_pointwise_mixed_forward with
// out = NULL on the same arguments), e.g. to start other work between the two.
extern "C" int cdn_codenet_pwdw_s2_apply(
    const float *x, const void *x_qstate, int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t ld_x,
    const float *w_pw, const signed char *w_pw_codes, const float *w_pw_scale, const int *w_pw_colsum,
    const float *bias_pw, float *m_min, float *m_max, void *m_state, int64_t C, const float *w_dw, const float *bias_dw,
    int64_t ld_out, float *r_min, float *r_max, void *r_state, int bits, double momentum, int running, void *workspace,
    size_t workspace_bytes, float *out, void *stream) {
  return pwdw_s2_impl(false, x, x_qstate, N, Cin, H, W, ld_x, w_pw, w_pw_codes, w_pw_scale, w_pw_colsum, bias_pw, m_min,
                      m_max, m_state, C, w_dw, bias_dw, ld_out, r_min, r_max, r_state, bits, momentum, running, workspace,
                      workspace_bytes, out, stream);
}
