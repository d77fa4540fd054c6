// codenet_loss.hip -- the ctdet training criterion and its target maps (gfx950 only).
//
// cdn_ctdet_loss_forward / _backward: CtdetLoss (lib/trains/ctdet.py:17-74) for the options the trainer's defaults use --
// focal loss on hm (lib/models/losses.py:42-67 behind models/utils.py:9-11 _sigmoid), RegL1Loss / RegLoss on wh and reg
// (losses.py:100-155) -- as ONE pass over the logits and the target per direction.  cdn_ctdet_targets: the target maps of
// lib/datasets/sample/ctdet.py:87-122 from per-image object lists.
//
// Arithmetic.  Every per-element value is formed in float32 in the reference's operation order with contraction off
// (no fma where the reference has a product and a sum).  The SUMS are where this file leaves the reference: each thread
// adds its terms in double, waves and workgroups are reduced in double in a fixed order, every workgroup stores one slab
// of partials and a one-workgroup finish adds the slabs in index order ("store-and-sum").  No floating-point atomics, no
// dependence on which workgroup runs first: a call is a pure function of its inputs, bit for bit.  The double sums are
// rounded to float32 once, in front of the reference's float32 scalar arithmetic (num_pos branch, denominators, weights).
#include "cdn_common.h"

#include <cmath>

namespace {
using namespace cdn;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxHmBlocks = 2048;       // eight workgroups per CU; the grid is a function of the shape alone
constexpr int kSlab = 8;                 // doubles per workgroup: pos, neg, num_pos, wh, off, mask, -, -
// (the result block is 8 floats: loss, hm_loss, wh_loss, off_loss, hm denominator, reg denominator, num_pos, mask sum)
constexpr int kMaxObjs = 2048;           // target kernel: one 24-byte LDS record per object row

inline int hm_blocks(int64_t total) {
  const int64_t quads = (total + 3) / 4;
  const int64_t nb = ceil_div(quads, kThreads);
  return (int)(nb < kMaxHmBlocks ? nb : kMaxHmBlocks);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);      // the same tree in every wave of every call
  return v;
}

// NQ per-thread doubles -> one value per quantity in out[0 .. NQ): wave tree, then the waves in index order
template <int NQ>
__device__ __forceinline__ void block_sums(double (&v)[NQ], double *out, double *red) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) v[q] = wave_sum(v[q]);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) red[wave * NQ + q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < NQ) {
    double s = red[threadIdx.x];
    for (int w = 1; w < kWaves; ++w) s += red[w * NQ + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

__device__ __forceinline__ float sigmoid_f(float x) {
#pragma clang fp contract(off)
  return 1.0f / (1.0f + expf(-x));
}
#define CDN_P_LO 1e-4f
#define CDN_P_HI ((float)(1.0 - 1e-4))

// the regression term of one (object row, channel): |pred*m - t*m| or its smooth form; *dsign = d term / d pred
template <bool GRAD>
__device__ __forceinline__ float reg_term(float pred, float t, float m, int sl1, float *dterm) {
#pragma clang fp contract(off)
  const float d = pred * m - t * m;
  const float z = fabsf(d);
  if (GRAD) {
    const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : d);      // sign(0) = 0; a NaN stays one
    *dterm = ((sl1 && z < 1.0f) ? d : sg) * m;
  }
  return (sl1 && z < 1.0f) ? 0.5f * z * z : (sl1 ? z - 0.5f : z);
}

struct LossArgs {
  const float *hm, *hm_gt;
  int64_t total;                 // N * C * H * W
  int hm_nblk, vec;
  const float *wh, *reg, *wh_gt, *reg_gt;      // wh / reg: nullptr = that term is off
  const int64_t *ind;
  const unsigned char *mask;
  int N, M;
  int64_t HW;
  int sl1;
};

// ---- forward: workgroups [0, hm_nblk) walk the heat map in quads of four floats, workgroup hm_nblk + b owns the object
// rows of image b.  Every workgroup stores its kSlab partials (zeros where it has none).
__global__ __launch_bounds__(kThreads) void ctdet_loss_fwd_kernel(LossArgs a, float *p_out, double *slab) {
#pragma clang fp contract(off)
  __shared__ double red[kWaves * 3];
  double v[3] = {0.0, 0.0, 0.0};
  double *out = slab + (size_t)blockIdx.x * kSlab;
  if ((int)blockIdx.x < a.hm_nblk) {
    const int64_t quads = (a.total + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += (int64_t)a.hm_nblk * kThreads) {
      float x[4], g[4], p[4];
      const int64_t e0 = q * 4;
      const int n = a.total - e0 >= 4 ? 4 : (int)(a.total - e0);
      if (a.vec && n == 4) {
        const float4 xv = reinterpret_cast<const float4 *>(a.hm)[q], gv = reinterpret_cast<const float4 *>(a.hm_gt)[q];
        x[0] = xv.x, x[1] = xv.y, x[2] = xv.z, x[3] = xv.w;
        g[0] = gv.x, g[1] = gv.y, g[2] = gv.z, g[3] = gv.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          x[j] = j < n ? a.hm[e0 + j] : 0.0f;
          g[j] = j < n ? a.hm_gt[e0 + j] : 2.0f;      // (a target above 1 is in neither term)
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        p[j] = clamp_keep_nan(sigmoid_f(x[j]), CDN_P_LO, CDN_P_HI);
        const float omp = 1.0f - p[j];
        if (g[j] == 1.0f) {
          v[0] += (double)(logf(p[j]) * (omp * omp));
          v[2] += 1.0;
        } else if (g[j] < 1.0f) {
          const float omg = 1.0f - g[j], w2 = omg * omg;
          v[1] += (double)(logf(omp) * (p[j] * p[j]) * (w2 * w2));
        }
      }
      if (p_out) {
        if (a.vec && n == 4) {
          reinterpret_cast<float4 *>(p_out)[q] = make_float4(p[0], p[1], p[2], p[3]);
        } else {
          for (int j = 0; j < n; ++j) p_out[e0 + j] = p[j];
        }
      }
    }
    block_sums<3>(v, out, red);
    if (threadIdx.x >= 3 && threadIdx.x < kSlab) out[threadIdx.x] = 0.0;
    return;
  }
  const int b = (int)blockIdx.x - a.hm_nblk;
  for (int k = threadIdx.x; k < a.M; k += kThreads) {
    const int64_t row = (int64_t)b * a.M + k, cell = a.ind[row];
    const float m = (float)a.mask[row];
    const bool ok = cell >= 0 && cell < a.HW;       // a cell outside the map is not read: the loss turns NaN instead
    v[2] += (double)m;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (a.wh) {
        const float pred = ok ? a.wh[((int64_t)b * 2 + c) * a.HW + cell] : NAN;
        v[0] += (double)reg_term<false>(pred, a.wh_gt[row * 2 + c], m, a.sl1, nullptr);
      }
      if (a.reg) {
        const float pred = ok ? a.reg[((int64_t)b * 2 + c) * a.HW + cell] : NAN;
        v[1] += (double)reg_term<false>(pred, a.reg_gt[row * 2 + c], m, a.sl1, nullptr);
      }
    }
  }
  block_sums<3>(v, out + 3, red);
  if (threadIdx.x < 3) out[threadIdx.x] = 0.0;
  if (threadIdx.x >= 6 && threadIdx.x < kSlab) out[threadIdx.x] = 0.0;
}

// ---- finish: one workgroup adds the slabs of every stack in index order and runs the reference's scalar arithmetic
__global__ __launch_bounds__(kThreads) void ctdet_loss_finish_kernel(const double *slab, int nblk, int num_stacks, int sl1,
                                                                     int use_wh, int use_off, float hm_w, float wh_w,
                                                                     float off_w, float *result) {
#pragma clang fp contract(off)
  __shared__ double red[kWaves * 6];
  __shared__ double sums[6];
  float hm_loss = 0.0f, wh_loss = 0.0f, off_loss = 0.0f, hm_den = 1.0f, reg_den = 1.0f, npos = 0.0f, msum = 0.0f;
  for (int s = 0; s < num_stacks; ++s) {
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double *sl = slab + (size_t)s * nblk * kSlab;
    for (int i = threadIdx.x; i < nblk; i += kThreads) {
#pragma unroll
      for (int q = 0; q < 6; ++q) v[q] += sl[(size_t)i * kSlab + q];
    }
    __syncthreads();      // (`red` and `sums` of the previous stack have been read)
    block_sums<6>(v, sums, red);
    __syncthreads();
    if (threadIdx.x == 0) {
      const float pos = (float)sums[0], neg = (float)sums[1];
      npos = (float)sums[2];
      msum = (float)sums[5];
      // losses.py:63-66: `loss - neg_loss` without a positive, else `loss - (pos_loss + neg_loss) / num_pos`
      hm_den = npos == 0.0f ? 1.0f : npos;
      const float hm_s = npos == 0.0f ? 0.0f - neg : 0.0f - (pos + neg) / npos;
      hm_loss += hm_s / (float)num_stacks;
      // RegL1Loss divides by the sum of the EXPANDED mask (two channels), RegLoss by the plain count (losses.py:107,154)
      reg_den = (sl1 ? msum : (float)(2.0 * sums[5])) + 1e-4f;
      if (use_wh) wh_loss += ((float)sums[3] / reg_den) / (float)num_stacks;
      if (use_off) off_loss += ((float)sums[4] / reg_den) / (float)num_stacks;
    }
  }
  if (threadIdx.x == 0) {
    result[0] = hm_w * hm_loss + wh_w * wh_loss + off_w * off_loss;
    result[1] = hm_loss;
    result[2] = wh_loss;
    result[3] = off_loss;
    result[4] = hm_den;
    result[5] = reg_den;
    result[6] = npos;
    result[7] = msum;
  }
}

// ---- backward: the heat-map workgroups recompute p from the logits (two maps read, one written); workgroup
// hm_nblk + h * N + b clears the two planes of image b of head h (0 wh, 1 reg), then writes the object cells: the FIRST
// row of a cell adds every row of that cell in row order, so rows that share a cell need neither atomics nor a sort.
__global__ __launch_bounds__(kThreads) void ctdet_loss_bwd_kernel(LossArgs a, const float *result, const float *go,
                                                                  int num_stacks, float hm_w, float wh_w, float off_w,
                                                                  float *g_hm, float *g_wh, float *g_reg) {
#pragma clang fp contract(off)
  const float S = (float)num_stacks;
  if ((int)blockIdx.x < a.hm_nblk) {
    // d loss / d hm_loss of this stack, through `/ num_stacks`, the minus and `/ num_pos`
    const float coef = -(((go[0] * hm_w + go[1]) / S) / result[4]);
    const int64_t quads = (a.total + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += (int64_t)a.hm_nblk * kThreads) {
      float x[4], g[4], r[4];
      const int64_t e0 = q * 4;
      const int n = a.total - e0 >= 4 ? 4 : (int)(a.total - e0);
      if (a.vec && n == 4) {
        const float4 xv = reinterpret_cast<const float4 *>(a.hm)[q], gv = reinterpret_cast<const float4 *>(a.hm_gt)[q];
        x[0] = xv.x, x[1] = xv.y, x[2] = xv.z, x[3] = xv.w;
        g[0] = gv.x, g[1] = gv.y, g[2] = gv.z, g[3] = gv.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          x[j] = j < n ? a.hm[e0 + j] : 0.0f;
          g[j] = j < n ? a.hm_gt[e0 + j] : 2.0f;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = sigmoid_f(x[j]), omp = 1.0f - p;
        float d = 0.0f;
        if (g[j] == 1.0f) {
          d = (omp * omp) / p - 2.0f * logf(p) * omp;                       // d/dp of log(p) (1-p)^2
        } else if (g[j] < 1.0f) {
          const float omg = 1.0f - g[j], w2 = omg * omg;
          d = (2.0f * p * logf(omp) - (p * p) / omp) * (w2 * w2);           // d/dp of log(1-p) p^2 (1-gt)^4
        }
        // the clamp passes a gradient inside [1e-4, 1 - 1e-4] only (a NaN sigmoid is outside); sigmoid' = p (1 - p)
        r[j] = (p >= CDN_P_LO && p <= CDN_P_HI) ? coef * d * (p * omp) : 0.0f;
      }
      if (a.vec && n == 4) {
        reinterpret_cast<float4 *>(g_hm)[q] = make_float4(r[0], r[1], r[2], r[3]);
      } else {
        for (int j = 0; j < n; ++j) g_hm[e0 + j] = r[j];
      }
    }
    return;
  }
  const int t = (int)blockIdx.x - a.hm_nblk, head = t / a.N, b = t % a.N;
  const float *src = head ? a.reg : a.wh, *tgt = head ? a.reg_gt : a.wh_gt;
  float *dst = head ? g_reg : g_wh;
  if (!src || !dst) return;
  float *plane = dst + (int64_t)b * 2 * a.HW;
  const int64_t cells = 2 * a.HW;
  if ((cells & 3) == 0 && ((uintptr_t)plane & 15) == 0) {
    for (int64_t i = threadIdx.x; i < cells / 4; i += kThreads)
      reinterpret_cast<float4 *>(plane)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int64_t i = threadIdx.x; i < cells; i += kThreads) plane[i] = 0.0f;
  }
  __syncthreads();      // (waits for the stores of the whole workgroup: the object cells are written behind them)
  const float coef = ((go[0] * (head ? off_w : wh_w) + go[head ? 3 : 2]) / S) / result[5];
  const int64_t *ind = a.ind + (int64_t)b * a.M;
  for (int item = threadIdx.x; item < 2 * a.M; item += kThreads) {
    const int c = item / a.M, k = item % a.M;
    const int64_t cell = ind[k];
    if (cell < 0 || cell >= a.HW) continue;
    bool first = true;
    for (int j = 0; j < k; ++j) first &= ind[j] != cell;
    if (!first) continue;
    float acc = 0.0f;
    for (int j = k; j < a.M; ++j) {
      if (ind[j] != cell) continue;
      const int64_t row = (int64_t)b * a.M + j;
      float dterm;
      (void)reg_term<true>(src[((int64_t)b * 2 + c) * a.HW + cell], tgt[row * 2 + c], (float)a.mask[row], a.sl1, &dterm);
      acc += dterm * coef;
    }
    plane[(int64_t)c * a.HW + cell] = acc;
  }
}

// ---- target maps.  One workgroup per (image, class) plane: the object rows of the image become LDS records
// {centre, radius, 2 sigma^2} (radius -1: not of this class, or gated out), then every pixel takes the maximum over the
// records whose window holds it and is stored once.  The class-0 workgroup also writes the image's per-row outputs.
struct ObjRec {
  int x, y, r, pad;
  double den;
};

__device__ __forceinline__ int gaussian_radius_dev(double height, double width) {
#pragma clang fp contract(off)
  // lib/utils/image.py:90-110 with min_overlap = 0.7, double throughout, Python's operation order
  const double ov = 0.7;
  const double b1 = height + width;
  const double c1 = width * height * (1 - ov) / (1 + ov);
  const double r1 = (b1 + sqrt(b1 * b1 - 4 * c1)) / 2;
  const double b2 = 2 * (height + width);
  const double c2 = (1 - ov) * width * height;
  const double r2 = (b2 + sqrt(b2 * b2 - 16 * c2)) / 2;
  const double a3 = 4 * ov;
  const double b3 = -2 * ov * (height + width);
  const double c3 = (ov - 1) * width * height;
  const double r3 = (b3 + sqrt(b3 * b3 - 4 * a3 * c3)) / 2;
  const double r = fmin(r1, fmin(r2, r3));
  const int ri = (int)r;                     // int(): truncation
  return ri > 0 ? ri : 0;
}

__global__ __launch_bounds__(kThreads) void ctdet_targets_kernel(const float *boxes, const int *classes, const int *counts,
                                                                 int M, int C, int H, int W, float *hm, float *wh,
                                                                 float *reg, int64_t *ind, unsigned char *mask) {
#pragma clang fp contract(off)
  extern __shared__ double lds_raw[];
  ObjRec *rec = reinterpret_cast<ObjRec *>(lds_raw);
  const int b = blockIdx.x / C, cls = blockIdx.x % C;
  int cnt = counts[b];
  cnt = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  for (int k = threadIdx.x; k < M; k += kThreads) {
    const int64_t row = (int64_t)b * M + k;
    float w = 0.f, h = 0.f, rx = 0.f, ry = 0.f;
    int64_t cell = 0;
    unsigned char live = 0;
    ObjRec o = {0, 0, -1, 0, 1.0};
    if (k < cnt) {
      const float x1 = boxes[row * 4], y1 = boxes[row * 4 + 1], x2 = boxes[row * 4 + 2], y2 = boxes[row * 4 + 3];
      const float bh = y2 - y1, bw = x2 - x1;
      const int kc = classes[row];
      if (bh > 0.0f && bw > 0.0f && kc >= 0 && kc < C) {
        const float cx = (x1 + x2) / 2.0f, cy = (y1 + y2) / 2.0f;
        const int ix = (int)cx, iy = (int)cy;               // astype(int32): truncation
        w = bw, h = bh, rx = cx - (float)ix, ry = cy - (float)iy, live = 1;
        cell = (int64_t)iy * W + ix;
        if (kc == cls) {
          const int r = gaussian_radius_dev(ceil((double)bh), ceil((double)bw));
          const double sigma = (double)(2 * r + 1) / 6.0;
          o.x = ix, o.y = iy, o.r = r, o.den = 2 * sigma * sigma;
        }
      }
    }
    rec[k] = o;
    if (cls == 0) {
      wh[row * 2] = w, wh[row * 2 + 1] = h;
      reg[row * 2] = rx, reg[row * 2 + 1] = ry;
      ind[row] = cell;
      mask[row] = live;
    }
  }
  __syncthreads();
  float *plane = hm + (int64_t)blockIdx.x * H * W;
  const int HW = H * W;
  const bool vec = (HW & 3) == 0 && ((uintptr_t)plane & 15) == 0;
  for (int q = threadIdx.x; q < (HW + 3) / 4; q += kThreads) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    int px[4], py[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) py[j] = (q * 4 + j) / W, px[j] = (q * 4 + j) % W;
    for (int k = 0; k < cnt; ++k) {
      const ObjRec o = rec[k];
      if (o.r < 0) continue;
      // the quad's rows and columns against the window [x - r, x + r] x [y - r, y + r] (image.py:130-134; the map's
      // borders cut it because only pixels of the map are visited)
      if (py[0] > o.y + o.r || py[3] < o.y - o.r) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int dx = px[j] - o.x, dy = py[j] - o.y;
        if (dx < -o.r || dx > o.r || dy < -o.r || dy > o.r) continue;
        const double ddx = (double)dx, ddy = (double)dy;
        double gv = exp(-(ddx * ddx + ddy * ddy) / o.den);          // gaussian2D: double, image.py:113-119
        if (gv < 2.220446049250313e-16) gv = 0.0;                    // h[h < eps * h.max()] = 0, h.max() = 1
        v[j] = fmaxf(v[j], (float)gv);                               // np.maximum into the float32 map
      }
    }
    if (vec) {
      reinterpret_cast<float4 *>(plane)[q] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int j = 0; j < 4 && q * 4 + j < HW; ++j) plane[q * 4 + j] = v[j];
    }
  }
}

int check_shape(int64_t N, int64_t C, int64_t H, int64_t W, int64_t M) {
  CDN_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && M > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(N <= 65535 && M <= (1 << 20) && H * W <= (1 << 28), CDN_ERR_UNSUPPORTED, "shape too large");
  return CDN_OK;
}

LossArgs loss_args(const float *hm, const float *wh, const float *reg, const float *hm_gt, const float *wh_gt,
                   const float *reg_gt, const int64_t *ind, const uint8_t *mask, int64_t N, int64_t C, int64_t H,
                   int64_t W, int64_t M, int reg_loss, const void *other) {
  LossArgs a;
  a.hm = hm, a.hm_gt = hm_gt, a.total = N * C * H * W, a.hm_nblk = hm_blocks(a.total);
  a.vec = (((uintptr_t)hm | (uintptr_t)hm_gt | (uintptr_t)other) & 15) == 0;
  a.wh = wh, a.reg = reg, a.wh_gt = wh_gt, a.reg_gt = reg_gt, a.ind = ind, a.mask = mask;
  a.N = (int)N, a.M = (int)M, a.HW = H * W, a.sl1 = reg_loss == 1;
  return a;
}

}  // namespace

extern "C" size_t cdn_ctdet_loss_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t M, int num_stacks) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || M <= 0 || num_stacks <= 0) return 0;
  return round256((size_t)num_stacks * (size_t)(hm_blocks(N * C * H * W) + N) * kSlab * sizeof(double));
}

extern "C" int cdn_ctdet_loss_forward(const float *hm, const float *wh, const float *reg, const float *hm_gt,
                                      const float *wh_gt, const float *reg_gt, const int64_t *ind,
                                      const uint8_t *reg_mask, int64_t N, int64_t C, int64_t H, int64_t W, int64_t M,
                                      int stack, int num_stacks, int reg_loss, float hm_weight, float wh_weight,
                                      float off_weight, float *hm_sigmoid, float *result, void *workspace,
                                      size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(hm && hm_gt && ind && reg_mask && result && workspace, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE((!wh || wh_gt) && (!reg || reg_gt), CDN_ERR_ARG, "a regression head without its target");
  const int rc = check_shape(N, C, H, W, M);
  if (rc) return rc;
  CDN_REQUIRE(num_stacks > 0 && stack >= 0 && stack < num_stacks, CDN_ERR_ARG, "stack %d of %d", stack, num_stacks);
  CDN_REQUIRE(reg_loss == 0 || reg_loss == 1, CDN_ERR_ARG, "reg_loss must be 0 (l1) or 1 (sl1)");
  CDN_REQUIRE(((uintptr_t)workspace & 255) == 0 &&
                  workspace_bytes >= cdn_ctdet_loss_workspace_bytes(N, C, H, W, M, num_stacks),
              CDN_ERR_ARG, "workspace misaligned or too small");
  const LossArgs a = loss_args(hm, wh, reg, hm_gt, wh_gt, reg_gt, ind, reg_mask, N, C, H, W, M, reg_loss, hm_sigmoid);
  const int nblk = a.hm_nblk + (int)N;
  double *slab = static_cast<double *>(workspace);
  hipStream_t st = cdn::as_stream(stream);
  ctdet_loss_fwd_kernel<<<nblk, kThreads, 0, st>>>(a, hm_sigmoid, slab + (size_t)stack * nblk * kSlab);
  int rcl = cdn::check_launch("ctdet loss forward");
  if (rcl || stack != num_stacks - 1) return rcl;
  ctdet_loss_finish_kernel<<<1, kThreads, 0, st>>>(slab, nblk, num_stacks, a.sl1, wh != nullptr, reg != nullptr,
                                                   hm_weight, wh_weight, off_weight, result);
  return cdn::check_launch("ctdet loss finish");
}

extern "C" int cdn_ctdet_loss_backward(const float *hm, const float *wh, const float *reg, const float *hm_gt,
                                       const float *wh_gt, const float *reg_gt, const int64_t *ind,
                                       const uint8_t *reg_mask, int64_t N, int64_t C, int64_t H, int64_t W, int64_t M,
                                       int num_stacks, int reg_loss, float hm_weight, float wh_weight, float off_weight,
                                       const float *result, const float *grad_result, float *grad_hm, float *grad_wh,
                                       float *grad_reg, void *stream) {
  CDN_REQUIRE(hm && hm_gt && ind && reg_mask && result && grad_result && grad_hm, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE((!grad_wh || (wh && wh_gt)) && (!grad_reg || (reg && reg_gt)), CDN_ERR_ARG,
              "a regression gradient without its head or target");
  const int rc = check_shape(N, C, H, W, M);
  if (rc) return rc;
  CDN_REQUIRE(num_stacks > 0 && (reg_loss == 0 || reg_loss == 1), CDN_ERR_ARG, "bad num_stacks or reg_loss");
  const LossArgs a = loss_args(hm, wh, reg, hm_gt, wh_gt, reg_gt, ind, reg_mask, N, C, H, W, M, reg_loss, grad_hm);
  ctdet_loss_bwd_kernel<<<a.hm_nblk + 2 * (int)N, kThreads, 0, cdn::as_stream(stream)>>>(
      a, result, grad_result, num_stacks, hm_weight, wh_weight, off_weight, grad_hm, grad_wh, grad_reg);
  return cdn::check_launch("ctdet loss backward");
}

extern "C" int cdn_ctdet_targets(const float *boxes, const int32_t *classes, const int32_t *counts, int64_t N, int64_t M,
                                 int64_t C, int64_t H, int64_t W, float *hm, float *wh, float *reg, int64_t *ind,
                                 uint8_t *reg_mask, void *stream) {
  CDN_REQUIRE(boxes && classes && counts && hm && wh && reg && ind && reg_mask, CDN_ERR_ARG, "null pointer");
  const int rc = check_shape(N, C, H, W, M);
  if (rc) return rc;
  CDN_REQUIRE(M <= kMaxObjs, CDN_ERR_UNSUPPORTED, "more than %d object rows per image", kMaxObjs);
  CDN_REQUIRE(N * C <= 0x7fffffff && H * W <= (1 << 24), CDN_ERR_UNSUPPORTED, "shape too large");
  ctdet_targets_kernel<<<(unsigned)(N * C), kThreads, (size_t)M * sizeof(ObjRec), cdn::as_stream(stream)>>>(
      boxes, classes, counts, (int)M, (int)C, (int)H, (int)W, hm, wh, reg, ind, reg_mask);
  return cdn::check_launch("ctdet targets");
}
