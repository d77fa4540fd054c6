// codenet_preproc.hip -- what CtdetDetector.pre_process (lib/detectors/base_detector.py:47-77) and the input half of the
// training sample (lib/datasets/sample/ctdet.py:84-97) do to an image before the network sees it (SURVEY.md section 2
// rows 10 and 15): resize to the test scale, affine crop to the network input with a zero border, optional source flip,
// (v / 255 - mean) / std, HWC -> planes, and the W-mirrors of --flip_test.  One launch for all test scales (or all crops
// of a training batch), uint8 source in, float32 planes out.
//
// ---- arithmetic (DESIGN.md section 7.4b is the contract; tests/preproc_ref.py restates it in numpy) ---------------------
// An INTEGER specification of the project's own, in the form of the reference's cv2.resize + cv2.warpAffine(INTER_LINEAR)
// on uint8 (resize first, then crop: two resamplings, each rounded to uint8), NOT a copy of cv2's bits.
//   resize, per axis:  f = float32((d + 0.5) * ratio - 0.5)  (product and sum in double, each rounded once);
//                      i = floor(f), t = f - i; i < 0 -> (0, 0); i >= n - 1 -> (n - 1, 0); second tap min(i + 1, n - 1);
//                      w1 = rint(t * 2048), w0 = 2048 - w1;   pixel = (sum_y b_y (sum_x a_x v) + 2^21) >> 22
//   crop:              adelta = rint((M0 x) 1024), bdelta = rint((M3 x) 1024), X0 = rint((M1 y + M2) 1024) + 16,
//                      Y0 = rint((M4 y + M5) 1024) + 16 -- double, every operation rounded on its own (no fma);
//                      X = (X0 + adelta) >> 5 in 1/32 pixel, sx = X >> 5, fx = X & 31 (arithmetic shifts), Y likewise;
//                      each of the four taps is tested against the resized image on its own, a tap outside adds 0;
//                      weights (32-fy)(32-fx)32 ... fy fx 32 (sum 32768);  pixel = (sum w v + 2^14) >> 15
//   flip_src:          a tap at column xx that passed the test reads column new_w - 1 - xx
//   normalise:         out[c] = lut[v][c], the table built by the host in double from the float32 mean and std
// A resized image with new_h == 0 or new_w == 0 (a tiny image at a small test scale) has no pixel: every tap is outside.
//
// ---- the kernel ------------------------------------------------------------------------------------------------------
// A thread owns one output pixel (flat index over the plane, x fastest: the stores of a wave are 256 contiguous bytes
// per plane whatever out_w is; the mirrored stores are the same bytes of the row in descending order).  Everything that
// changes from image to image is read from the DEVICE item table; the launch geometry follows from P, out_h, out_w and
// mirror alone, so a captured graph replays for an image of any size.  For an item with a resize the resized pixel is
// RECOMPUTED at each of the four crop taps (16 source pixels): the same integer function, hence the same result as a
// resized uint8 image in memory, without the scratch image and the second launch.  The 3 KB table sits in LDS.
#include "cdn_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItem = 16;          // doubles per item

struct Axis {
  int i0, i1, w1;
};

// The two source taps and the 11-bit weight of index d of a resized axis (n_src source samples).
__device__ __forceinline__ Axis resize_axis(int d, int n_src, double ratio) {
#pragma clang fp contract(off)
  const double p = ((double)d + 0.5) * ratio;
  const float f = (float)(p - 0.5);
  const float fl = floorf(f);
  int i = (int)fl;
  float t = f - fl;
  if (i < 0) {
    i = 0;
    t = 0.0f;
  }
  if (i >= n_src - 1) {
    i = n_src - 1;
    t = 0.0f;
  }
  Axis a;
  a.i0 = i;
  a.i1 = i + 1 < n_src ? i + 1 : n_src - 1;
  a.w1 = __float2int_rn(t * 2048.0f);
  return a;
}

__device__ __forceinline__ long long fix10(double v) { return __double2ll_rn(v * 1024.0); }   // (x 2^10: exact)

// The crop of one output pixel (x, y) of an item (`it`: its 16 doubles of the table): the three uint8 values of the resized,
// cropped and optionally source-flipped image, 0 for the border.  Shared by pre_process_kernel and crop_sum_kernel.
__device__ __forceinline__ void crop_pixel(const unsigned char *__restrict__ arena, const double *__restrict__ it, int x,
                                           int y, int (&v)[3]) {
#pragma clang fp contract(off)
  const unsigned char *src = arena + (long long)it[0];
  const int h = (int)it[1], w = (int)it[2];
  const long long pitch = (long long)it[3];
  const int nh = (int)it[4], nw = (int)it[5];
  const bool resized = nh != h || nw != w;
  const bool flip = it[8] != 0.0;
  // ---- geometry, once for the three channels ---------------------------------------------------------------------------
  // (hipcc contracts by default, and __dmul_rn / __dadd_rn are plain operators of a header compiled WITH contraction:
  // the pragma on the operators written here is what keeps M1 y + M2 two roundings)
  const double dx = (double)x, dy = (double)y;
  const double px = it[10] * dy, py = it[13] * dy;
  const long long adelta = fix10(it[9] * dx);
  const long long bdelta = fix10(it[12] * dx);
  const long long X0 = fix10(px + it[11]) + 16;
  const long long Y0 = fix10(py + it[14]) + 16;
  const long long X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
  const long long sx = X >> 5, sy = Y >> 5;
  const int fx = (int)(X & 31), fy = (int)(Y & 31);
  const int wx[2] = {32 - fx, fx}, wy[2] = {32 - fy, fy};
  int acc[3] = {0, 0, 0};
#pragma unroll
  for (int ty = 0; ty < 2; ++ty) {
    const long long yy = sy + ty;
    if (yy < 0 || yy >= nh) continue;
#pragma unroll
    for (int tx = 0; tx < 2; ++tx) {
      const long long xx = sx + tx;
      if (xx < 0 || xx >= nw) continue;
      const int wgt = wy[ty] * wx[tx] * 32;
      const int col = flip ? nw - 1 - (int)xx : (int)xx;
      if (!resized) {
        const unsigned char *p = src + yy * pitch + (long long)col * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += wgt * (int)p[c];
      } else {
        const Axis ay = resize_axis((int)yy, h, it[6]), ax = resize_axis(col, w, it[7]);
        const unsigned char *r0 = src + (long long)ay.i0 * pitch, *r1 = src + (long long)ay.i1 * pitch;
        const int a0 = 2048 - ax.w1, a1 = ax.w1, b0 = 2048 - ay.w1, b1 = ay.w1;
        const int o0 = ax.i0 * 3, o1 = ax.i1 * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int top = a0 * (int)r0[o0 + c] + a1 * (int)r0[o1 + c];
          const int bot = a0 * (int)r1[o0 + c] + a1 * (int)r1[o1 + c];
          acc[c] += wgt * ((b0 * top + b1 * bot + (1 << 21)) >> 22);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = (acc[c] + (1 << 14)) >> 15;
}

__global__ void __launch_bounds__(kThreads)
pre_process_kernel(const unsigned char *__restrict__ arena, const double *__restrict__ items,
                   const float *__restrict__ lut, float *__restrict__ out, int out_h, int out_w, int P, int mirror) {
  __shared__ float s_lut[256 * 3];
  for (int k = threadIdx.x; k < 256 * 3; k += kThreads) s_lut[k] = lut[k];
  __syncthreads();
  const int item = blockIdx.y;
  const int hw = out_h * out_w;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  if (pix >= hw) return;
  const int y = pix / out_w, x = pix - y * out_w;
  int v[3];
  crop_pixel(arena, items + (size_t)item * kItem, x, y, v);
  const size_t plane = (size_t)hw;
  float *o = out + (size_t)item * 3 * plane + pix;
  float *m = out + ((size_t)P + item) * 3 * plane + (size_t)y * out_w + (out_w - 1 - x);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float f = s_lut[v[c] * 3 + c];
    o[c * plane] = f;
    if (mirror) m[c * plane] = f;
  }
}

// ---- colour augmentation of the training sample (tests/color_aug_ref.py restates it) --------------
// lib/datasets/sample/ctdet.py:76-79 with lib/utils/image.py:196-234: v / 255, brightness / contrast / saturation in the
// item's order, lighting, (x - mean) / std -- float32, every operation rounded once.  The contrast step blends with the
// mean grey value of the WHOLE crop, so the work is two launches: crop_sum_kernel leaves the crop's bytes (planar:
// crop_u8[item][c][pixel]) and the three channel sums of every item, color_aug_kernel reads both.
// The sums are INTEGERS (every pixel of the crop is a byte): one 64-bit integer atomic add per channel and workgroup.
// Integer addition gives the same bits in any order, so the result does not depend on the order the workgroups arrive
// in -- this is why an atomic is allowed here while every floating-point reduction of the library has a fixed order.
constexpr int kAug = 16;           // 4-byte words per aug row: int32 {on, order[3]}, float32 {a[3], om[3], d[3]}, 3 unused

__global__ void __launch_bounds__(kThreads) zero_sums_kernel(unsigned long long *__restrict__ sums, int n) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) sums[i] = 0ull;
}

__global__ void __launch_bounds__(kThreads)
crop_sum_kernel(const unsigned char *__restrict__ arena, const double *__restrict__ items,
                unsigned char *__restrict__ crop_u8, unsigned long long *__restrict__ sums, int out_h, int out_w) {
  __shared__ unsigned s_part[kThreads / 64][3];
  const int item = blockIdx.y;
  const int hw = out_h * out_w;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  int v[3] = {0, 0, 0};                       // a lane past the plane adds 0
  if (pix < hw) {
    const int y = pix / out_w, x = pix - y * out_w;
    crop_pixel(arena, items + (size_t)item * kItem, x, y, v);
    unsigned char *o = crop_u8 + (size_t)item * 3 * hw + pix;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[(size_t)c * hw] = (unsigned char)v[c];
  }
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] += __shfl_xor(v[c], m, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) s_part[threadIdx.x >> 6][c] = (unsigned)v[c];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned t = 0;                           // <= 256 * 255
#pragma unroll
    for (int wv = 0; wv < kThreads / 64; ++wv) t += s_part[wv][threadIdx.x];
    atomicAdd(sums + (size_t)item * 3 + threadIdx.x, (unsigned long long)t);
  }
}

__global__ void __launch_bounds__(kThreads)
color_aug_kernel(const unsigned char *__restrict__ crop_u8, const unsigned long long *__restrict__ sums,
                 const float *__restrict__ aug, const float *__restrict__ mean_std, float *__restrict__ out, int out_h,
                 int out_w) {
#pragma clang fp contract(off)
  __shared__ float s_gs_mean;
  const int item = blockIdx.y;
  const int hw = out_h * out_w;
  const float *__restrict__ row = aug + (size_t)item * kAug;      // uniform over the workgroup: scalar loads
  const int *__restrict__ rowi = reinterpret_cast<const int *>(row);
  const bool on = rowi[0] != 0;
  if (on && threadIdx.x == 0) {
    // float64, float64 literals, every operation rounded on its own; the sums are exact in a double (< 2^39)
    const double s0 = (double)sums[(size_t)item * 3], s1 = (double)sums[(size_t)item * 3 + 1],
                 s2 = (double)sums[(size_t)item * 3 + 2];
    const double p0 = 0.114 * s0, p1 = 0.587 * s1, p2 = 0.299 * s2;
    const double num = (p0 + p1) + p2;
    const double den = 255.0 * (double)hw;
    s_gs_mean = (float)(num / den);
  }
  __syncthreads();
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  if (pix >= hw) return;
  const unsigned char *p = crop_u8 + (size_t)item * 3 * hw + pix;
  float x[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) x[c] = (float)p[(size_t)c * hw] / 255.0f;
  if (on) {
    const float gs_mean = s_gs_mean;
    const float g0 = x[0] * 0.114f, g1 = x[1] * 0.587f, g2 = x[2] * 0.299f;
    const float gs = (g0 + g1) + g2;          // of the un-augmented pixel, once (image.py:230)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int f = rowi[1 + k] & 3;      // (the host admits 0, 1, 2 only; the mask keeps any word inside the row)
      const float a = row[4 + f], om = row[7 + f];
      if (f == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = x[c] * a;
      } else {
        const float q = (f == 1 ? gs_mean : gs) * om;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float t = x[c] * a;
          x[c] = t + q;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = x[c] + row[10 + c];
  }
  float *o = out + (size_t)item * 3 * hw + pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = x[c] - mean_std[c];
    o[(size_t)c * hw] = t / mean_std[3 + c];
  }
}

}  // namespace

extern "C" int cdn_ctdet_pre_process(const unsigned char *src_arena, const double *items, int64_t P, const float *lut,
                                     float *out, int64_t out_h, int64_t out_w, int mirror, void *stream) {
  CDN_REQUIRE(src_arena && items && lut && out, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(P > 0 && out_h > 0 && out_w > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(P <= 65535, CDN_ERR_UNSUPPORTED, "more than 65535 items in one call");
  CDN_REQUIRE(out_h <= (1 << 20) && out_w <= (1 << 20) && out_h * out_w < (int64_t(1) << 31) - kThreads,
              CDN_ERR_UNSUPPORTED, "output plane %lld x %lld too large", (long long)out_h, (long long)out_w);
  const dim3 grid((unsigned)cdn::ceil_div(out_h * out_w, kThreads), (unsigned)P);
  pre_process_kernel<<<grid, kThreads, 0, cdn::as_stream(stream)>>>(src_arena, items, lut, out, (int)out_h, (int)out_w,
                                                                    (int)P, mirror ? 1 : 0);
  return cdn::check_launch("ctdet pre_process");
}

extern "C" int cdn_ctdet_pre_process_aug(const unsigned char *src_arena, const double *items, int64_t P, const float *aug,
                                         const float *mean_std, unsigned char *crop_u8, unsigned long long *sums,
                                         float *out, int64_t out_h, int64_t out_w, void *stream) {
  CDN_REQUIRE(src_arena && items && aug && mean_std && crop_u8 && sums && out, CDN_ERR_ARG, "null pointer");
  CDN_REQUIRE(P > 0 && out_h > 0 && out_w > 0, CDN_ERR_ARG, "non-positive size");
  CDN_REQUIRE(P <= 65535, CDN_ERR_UNSUPPORTED, "more than 65535 items in one call");
  CDN_REQUIRE(out_h <= (1 << 20) && out_w <= (1 << 20) && out_h * out_w < (int64_t(1) << 31) - kThreads,
              CDN_ERR_UNSUPPORTED, "output plane %lld x %lld too large", (long long)out_h, (long long)out_w);
  hipStream_t st = cdn::as_stream(stream);
  // the sums start from zero in every call: a launch of our own in front of the kernel that adds, hence a node of a
  // captured graph.  NOT hipMemsetAsync: the runtime's memset node filled the sums with a stale 16-byte pattern on the
  // second replay of a captured run
  zero_sums_kernel<<<(unsigned)cdn::ceil_div(P * 3, kThreads), kThreads, 0, st>>>(sums, (int)(P * 3));
  const int rz = cdn::check_launch("ctdet zero_sums");
  if (rz != CDN_OK) return rz;
  const dim3 grid((unsigned)cdn::ceil_div(out_h * out_w, kThreads), (unsigned)P);
  crop_sum_kernel<<<grid, kThreads, 0, st>>>(src_arena, items, crop_u8, sums, (int)out_h, (int)out_w);
  const int rc = cdn::check_launch("ctdet crop_sum");
  if (rc != CDN_OK) return rc;
  color_aug_kernel<<<grid, kThreads, 0, st>>>(crop_u8, sums, aug, mean_std, out, (int)out_h, (int)out_w);
  return cdn::check_launch("ctdet color_aug");
}
