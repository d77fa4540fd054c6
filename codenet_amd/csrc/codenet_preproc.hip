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

__global__ void __launch_bounds__(kThreads)
pre_process_kernel(const unsigned char *__restrict__ arena, const double *__restrict__ items,
                   const float *__restrict__ lut, float *__restrict__ out, int out_h, int out_w, int P, int mirror) {
#pragma clang fp contract(off)
  __shared__ float s_lut[256 * 3];
  for (int k = threadIdx.x; k < 256 * 3; k += kThreads) s_lut[k] = lut[k];
  __syncthreads();
  const int item = blockIdx.y;
  const int hw = out_h * out_w;
  const int pix = blockIdx.x * kThreads + threadIdx.x;
  if (pix >= hw) return;
  const int y = pix / out_w, x = pix - y * out_w;
  const double *it = items + (size_t)item * kItem;
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
  const size_t plane = (size_t)hw;
  float *o = out + (size_t)item * 3 * plane + pix;
  float *m = out + ((size_t)P + item) * 3 * plane + (size_t)y * out_w + (out_w - 1 - x);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = (acc[c] + (1 << 14)) >> 15;
    const float f = s_lut[v * 3 + c];
    o[c * plane] = f;
    if (mirror) m[c * plane] = f;
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
