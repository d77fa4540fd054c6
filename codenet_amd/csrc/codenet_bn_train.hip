// codenet_bn_train.hip -- the block behind every deform stage of the fp32 model in training (main.py):
//   BatchNorm2d -> ReLU -> Upsample(x2, nearest)                         (lib/models/networks/shufflenetv2_dcn.py:303-308)
// forward and backward, with batch statistics (bn.training) or on the running statistics (eval mode under autograd).
// y [N][C][H][W] float32 NCHW is the stage's output; n = N * H * W values per channel.
//
// ---- arithmetic (DESIGN.md section 4.3e is the contract; tests/bn_block_ref.py restates it in numpy) -------------------
// Whole file under `#pragma clang fp contract(off)`: every operator written here is rounded on its own (hipcc contracts by
// default, and the _rn intrinsics of its headers are plain operators that contract with their neighbours, cdn_common.h).
//   statistics   S1 = sum y, S2 = sum y * y in float64 (the square of a float32 is exact in float64, so S2 / n - mean^2 has
//                no cancellation problem).  mean_d = S1 / n, var_d = max(S2 / n - mean_d * mean_d, 0) in float64, then ONE
//                rounding each: mean = f32(mean_d), var = f32(var_d) (biased).  invstd = 1 / sqrt(var + eps) in float32 with
//                correctly rounded sqrt and divide (formed through float64: 53 >= 2 * 24 + 2 bits make the second rounding
//                innocuous for both).  running_mean = (1 - m) * running_mean + m * mean and running_var = (1 - m) *
//                running_var + m * f32(var_d * (n / (n - 1))) in float32, (1 - m) = f32(1.0 - momentum); the int64
//                num_batches_tracked += 1.
//   apply        xh = (y - mean) * invstd, z = gamma * xh + beta (bn_z: the ONE device function forward and backward form z
//                with), out = relu(z) (NaN kept), written once (up = 1) or to its 2 x 2 replicas (up = 2).
//   backward 1   G = grad_out (up = 1) or ((g00 + g01) + g10) + g11 of the 2 x 2 block (up = 2); g_z = z > 0 ? G : 0 with z
//                recomputed by bn_z (no mask is stored); T1 = sum g_z and T2 = sum g_z * xh in float64 (the product of two
//                float32 is exact there); grad_beta = f32(T1), grad_gamma = f32(T2), mb = f32(T1 / n), mg = f32(T2 / n).
//   backward 2   grad_y = ((g_z - mb) - xh * mg) * (gamma * invstd); eval mode: grad_y = g_z * (gamma * invstd).
//
// ---- the sums ---------------------------------------------------------------------------------------------------------------
// cdn_train.h's protocol in float64.  A channel's n values, numbered j = image * H * W + pixel, are cut into slabs of
// kSlab = 4096 consecutive j; a workgroup (256 threads) owns one (channel, slab): grid = C * ceil(n / 4096), a function of
// the shape alone.  Thread t takes the quads q = t, t + 256, t + 512, t + 768 of the slab (values 4 q .. 4 q + 3) and adds its
// terms in that order from zero; the 64 lanes of a wave by an xor shuffle tree (32, 16, .. 1), the four waves in wave order
// through LDS, and the workgroup stores its two partial sums with plain stores, each word once.  A second small launch (one
// thread per channel) adds a channel's partials in slab order and finishes the per-channel numbers.  No float atomics.
// W % 4 == 0 (VEC): a quad lies in one row and moves as 16-byte words; otherwise element by element -- the same terms in the
// same order either way.
// The kernels live in cdn_bn.h (the fp32 heads, units and stem run the same ones, codenet_*_fp32_train.hip).
#include "cdn_bn.h"

#pragma clang fp contract(off)

extern "C" size_t cdn_codenet_bn_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return bn_plan(N, C, H, W).part_bytes + cdn::round256((size_t)C * 2 * sizeof(float));
}

extern "C" int cdn_codenet_bn_relu_up_forward(const float *y, const float *gamma, const float *beta, float *running_mean,
                                              float *running_var, int64_t *num_batches_tracked, float *mean, float *var,
                                              float *invstd, float *out, int64_t N, int64_t C, int64_t H, int64_t W, int up,
                                              int training, double eps, double momentum, void *workspace,
                                              size_t workspace_bytes, void *stream) {
  CDN_REQUIRE(y && gamma && beta && mean && var && invstd && out, CDN_ERR_ARG, "null pointer");
  if (int rc = bn_check_shape(N, C, H, W, up)) return rc;
  CDN_REQUIRE(cdn::aligned16(y) && cdn::aligned16(out), CDN_ERR_ARG, "tensors must be 16-byte aligned");
  hipStream_t st = cdn::as_stream(stream);
  if (int rc = launch_bn_stats(y, running_mean, running_var, num_batches_tracked, mean, var, invstd, N, C, H, W, training, eps,
                               momentum, workspace, workspace_bytes, cdn_codenet_bn_workspace_bytes(N, C, H, W), st))
    return rc;
  const long rows = (long)(N * C * H);
  const unsigned grid = rows_grid(rows, W);
  const bool vec = W % 4 == 0;
#define CDN_BN_APPLY(UP, VEC) \
  bn_apply_kernel<UP, VEC><<<grid, 256, 0, st>>>(y, mean, invstd, gamma, beta, out, rows, (int)C, (int)H, (int)W)
  if (up == 1) {
    if (vec) CDN_BN_APPLY(1, true); else CDN_BN_APPLY(1, false);
  } else {
    if (vec) CDN_BN_APPLY(2, true); else CDN_BN_APPLY(2, false);
  }
#undef CDN_BN_APPLY
  return cdn::check_launch("codenet bn relu up forward");
}

extern "C" int cdn_codenet_bn_relu_up_backward(const float *grad_out, const float *y, const float *gamma, const float *beta,
                                               const float *mean, const float *invstd, float *g_z, float *grad_y,
                                               float *grad_gamma, float *grad_beta, int64_t N, int64_t C, int64_t H,
                                               int64_t W, int up, int training, void *workspace, size_t workspace_bytes,
                                               void *stream) {
  CDN_REQUIRE(grad_out && y && gamma && beta && mean && invstd && g_z && grad_y && workspace, CDN_ERR_ARG, "null pointer");
  if (int rc = bn_check_shape(N, C, H, W, up)) return rc;
  CDN_REQUIRE(cdn::aligned16(grad_out) && cdn::aligned16(y) && cdn::aligned16(g_z) && cdn::aligned16(grad_y), CDN_ERR_ARG,
              "tensors must be 16-byte aligned");
  if (int rc = cdn::check_workspace(workspace, workspace_bytes, cdn_codenet_bn_workspace_bytes(N, C, H, W))) return rc;
  hipStream_t st = cdn::as_stream(stream);
  const BnPlan p = bn_plan(N, C, H, W);
  double *part = static_cast<double *>(workspace);
  float *mb = reinterpret_cast<float *>(static_cast<char *>(workspace) + p.part_bytes), *mg = mb + C;
  const unsigned grid1 = (unsigned)(C * p.slabs);
  const bool vec = W % 4 == 0;
#define CDN_BN_BWD1(UP, VEC)                                                                                            \
  bn_bwd1_kernel<UP, VEC><<<grid1, kBnThreads, 0, st>>>(grad_out, y, mean, invstd, gamma, beta, g_z, part, (int)C, (int)H, \
                                                        (int)W, p.n, p.slabs)
  if (up == 1) {
    if (vec) CDN_BN_BWD1(1, true); else CDN_BN_BWD1(1, false);
  } else {
    if (vec) CDN_BN_BWD1(2, true); else CDN_BN_BWD1(2, false);
  }
#undef CDN_BN_BWD1
  launch_bn_bwd_finish(part, grad_gamma, grad_beta, mb, mg, C, p, st);
  const long rows = (long)(N * C * H);
  const unsigned grid2 = rows_grid(rows, W);
#define CDN_BN_BWD2(SUB, VEC) \
  bn_bwd2_kernel<SUB, VEC><<<grid2, 256, 0, st>>>(g_z, y, mean, invstd, gamma, mb, mg, grad_y, rows, (int)C, (int)H, (int)W)
  if (training) {
    if (vec) CDN_BN_BWD2(true, true); else CDN_BN_BWD2(true, false);
  } else {
    if (vec) CDN_BN_BWD2(false, true); else CDN_BN_BWD2(false, false);
  }
#undef CDN_BN_BWD2
  return cdn::check_launch("codenet bn relu up backward");
}
