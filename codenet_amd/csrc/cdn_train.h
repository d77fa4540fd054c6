// cdn_train.h -- what the kernels of the QAT step share (codenet_heads_train.hip, codenet_units_train.hip,
// codenet_stem_train.hip): the fake-quantiser of a state snapshot, the register-window row loaders
// of the depthwise kernels and the one protocol of the per-channel weight / bias gradient sums; and what the two stems share
// (codenet_stem_train.hip, codenet_stem_fp32_train.hip): the 27-tap patch loader and the plan of the weight gradient.
//
// The sums.  A workgroup's K sums belong to one channel (group): a thread adds its own terms in its own fixed order, the 64
// lanes of a wave by an xor shuffle tree (32, 16, .. 1), the waves in wave order through LDS, and the workgroup stores its K
// partials with plain stores, each word exactly once (block_sums_store).  launch_sums_reduce then adds a channel's partials
// in index order.  No float atomics, and the grids are functions of the shape alone: every sum has one order.
#pragma once
#include "cdn_common.h"

#include <algorithm>

namespace cdn {

// The 3 -> 24 stem (codenet_stem_train.hip, codenet_stem_fp32_train.hip): 3 input channels x 3 x 3 taps per output position,
// and the plan of its weight gradient -- chunks of 256 * per_thread consecutive output positions (n, oy, ox flattened),
// per_thread = clamp(positions / 1024, 1, 8).  The chunk order is part of grad_W's contract in both files.
constexpr int kStemTaps = 27;
struct StemPlan {
  int Ho, Wo, per_thread, chunks;
  long positions;
};
inline StemPlan stem_plan(int64_t N, int64_t H, int64_t W, int stride) {
  StemPlan p;
  p.Ho = (int)((H - 1) / stride + 1);
  p.Wo = (int)((W - 1) / stride + 1);
  p.positions = (long)N * p.Ho * p.Wo;
  p.per_thread = (int)std::min<long>(8, std::max<long>(1, p.positions / 1024));
  p.chunks = (int)ceil_div(p.positions, 256L * p.per_thread);
  return p;
}

// grad_w [C][K - 1] and grad_b [C] (either may be NULL) from the workgroups' partials
// [outer][C / G][chunks][G][K] -- K sums per channel: K - 1 taps and the bias, G channels per workgroup -- summed outer
// index first, then chunks, both ascending.  Defined in codenet_heads_train.hip.
int launch_sums_reduce(const float *part, float *grad_w, float *grad_b, int C, int G, int K, int outer, int chunks,
                       hipStream_t st, const char *what);

#ifdef __HIPCC__
// the 27 taps of the stem's output position (oy, ox) of image n in (ci, dy, dx) order, zero outside the image
__device__ __forceinline__ void load_stem_patch(const float *__restrict__ img, int n, int oy, int ox, int H, int W,
                                                int stride, float (&v)[kStemTaps]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        // (guarded loads, not clamped addresses masked afterwards: the inference stem_kernel of codenet_layers.hip measured
        // the clamped form slower, 78-90 us against 61-62 us)
        const int y = oy * stride + dy - 1, x = ox * stride + dx - 1;
        v[(c * 3 + dy) * 3 + dx] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
                                       ? img[(((long)n * 3 + c) * H + y) * W + x] : 0.0f;
      }
}

// scale, zero point and RN(1 / scale) of a QuantAct state (snapshot): the operands of fake_quant_r
struct Fq {
  float s, z, r;
};
__device__ __forceinline__ Fq load_fq(const unsigned *__restrict__ state) {
  Fq f;
  f.s = reinterpret_cast<const float *>(state)[2];
  f.z = reinterpret_cast<const float *>(state)[3];
  f.r = __fdiv_rn(1.0f, f.s);
  return f;
}
__device__ __forceinline__ float fq_relu(float v, const Fq &f) { return fake_quant_r(relu_keep_nan(v), f.s, f.z, f.r); }

// NC columns xa - LEAD .. xa - LEAD + NC - 1 of row y of an H x W plane: v[j], 0.0f where the column (or the whole row)
// lies outside the plane; returns the mask of the columns inside.  xa is a multiple of 4 inside the row: 0 <= xa < W (a
// live item's first quad; only the quads behind it are tested).  VEC: W % 4 == 0 and 16-byte aligned rows, so a quad that
// starts inside the plane ends inside it.
template <int NC, int LEAD, bool VEC>
__device__ __forceinline__ unsigned load_cols(const float *__restrict__ plane, int y, int H, int W, int xa,
                                              float (&v)[NC]) {
#pragma unroll
  for (int j = 0; j < NC; ++j) v[j] = 0.0f;
  if (y < 0 || y >= H) return 0u;
  const float *row = plane + (long)y * W;
  unsigned ok = 0u;
  if (VEC) {
    constexpr int NV = (NC - LEAD) / 4;
    if (LEAD && xa > 0) { v[0] = row[xa - 1]; ok |= 1u; }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if (k == 0 || xa + 4 * k < W) {
        const float4 c = *reinterpret_cast<const float4 *>(row + xa + 4 * k);
        v[LEAD + 4 * k] = c.x; v[LEAD + 4 * k + 1] = c.y; v[LEAD + 4 * k + 2] = c.z; v[LEAD + 4 * k + 3] = c.w;
        ok |= 0xfu << (LEAD + 4 * k);
      }
    }
#pragma unroll
    for (int j = LEAD + 4 * NV; j < NC; ++j) {
      const int x = xa - LEAD + j;
      if (x < W) { v[j] = row[x]; ok |= 1u << j; }
    }
  } else {
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int x = xa - LEAD + j;
      if (x >= 0 && x < W) { v[j] = row[x]; ok |= 1u << j; }
    }
  }
  return ok;
}

// columns x0 .. x0 + 3 of a row of width W; VEC: one 16-byte store where the quad starts inside the row
template <bool VEC>
__device__ __forceinline__ void store4(float *__restrict__ row, int W, int x0, const float (&v)[4]) {
  if (VEC) {
    if (x0 < W) *reinterpret_cast<float4 *>(row + x0) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x0 + i < W) row[x0 + i] = v[i];
  }
}

// One window row of a depthwise input (columns xa - 1 ..).  RQ: the stored values are pre-activation, a = fq(relu(v)) is
// formed here and the returned mask is v > 0 (the ReLU mask of the backward); !RQ: final values, read as they are.  Taps
// outside the plane are literal zeros (the convolution's padding).
template <int NC, bool RQ, bool VEC>
__device__ __forceinline__ unsigned load_act(const float *__restrict__ plane, int y, int H, int W, int xa, const Fq &f,
                                             float (&a)[NC]) {
  float v[NC];
  const unsigned ok = load_cols<NC, 1, VEC>(plane, y, H, W, xa, v);
  unsigned pos = 0u;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const bool in = (ok >> j) & 1u;
    if (RQ) {
      a[j] = in ? fake_quant_r(relu_keep_nan(v[j]), f.s, f.z, f.r) : 0.0f;
      pos |= (in && v[j] > 0.0f) ? (1u << j) : 0u;
    } else {
      a[j] = v[j];
    }
  }
  return RQ ? pos : ok;
}

// The end of a weight-gradient kernel (see the head of the file); every thread of the workgroup calls it.  red: K words
// of LDS per wave; part [workgroups][K]: workgroup blockIdx.x stores its K words.  T: float here, double in the fp32
// training path (cdn_bn.h).
template <int K, typename T>
__device__ __forceinline__ void block_sums_store(const T (&sums)[K], T *red, T *__restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    T v = sums[k];
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) red[wave * K + k] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    T s = red[threadIdx.x];
    for (int i = 1; i < nw; ++i) s += red[i * K + threadIdx.x];
    part[(long)blockIdx.x * K + threadIdx.x] = s;
  }
}
#endif

}  // namespace cdn
