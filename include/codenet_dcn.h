/*
 * codenet_dcn.h -- C ABI of libcodenet_dcn.so, the MI355X (gfx950) implementation of
 * CoDeNet's deformable-convolution hot path.
 *
 * This is the drop-in boundary: every entry point replaces one function of the reference's
 * pybind11 module `dcn_deform_conv_cuda`
 * (lib/models/external/src/dcn_deform_conv_cuda.cpp:681-695) or one fused step of the
 * Python composition above it (lib/models/external/modules/dcn_deform_conv.py:285-330,
 * portable_quantizer/quant_modules.py:163-225,621-671).  Citations are relative to the
 * reference checkout.
 *
 * Conventions
 *   - All tensor arguments are DEVICE pointers to contiguous NCHW buffers owned by the
 *     caller; the library never allocates, frees or retains tensor memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work is
 *     enqueued asynchronously on it; no entry point synchronises the device or the host.
 *   - Every function returns 0 (CDN_OK) or a negative cdn_status; cdn_last_error() gives a
 *     thread-local human-readable message for the last failure on the calling thread.
 *   - dtype: CDN_F32, CDN_F64 or CDN_F16 (round 6: IEEE half in memory, fp32 arithmetic, one rounding per stored
 *     element; the reference dispatches half too, dcn_deform_conv_cuda_kernel.cu:258,352,450) for the generic entry
 *     points; the CoDeNet fast paths are f32 (activations) with int8 code paths where stated.
 *   - Re-entrant, no global mutable state (the only per-thread state: the cdn_last_error() message and the
 *     optional cdn_profile_* event list, both thread-local); safe to call concurrently from several host
 *     threads on different streams / devices (the current HIP device must be the one that
 *     owns the pointers).  tests/test_gpu_parity.py::test_stage_entry_points_from_two_threads drives two
 *     streams from two threads concurrently against the serial result.
 */
#ifndef CODENET_DCN_H_
#define CODENET_DCN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDN_ABI_VERSION 1

enum cdn_dtype { CDN_F32 = 0, CDN_F64 = 1, CDN_F16 = 2 };

enum cdn_status {
  CDN_OK = 0,
  CDN_ERR_ARG = -1,         /* null pointer / bad enum / non-positive size            */
  CDN_ERR_SHAPE = -2,       /* inconsistent shapes (reference: AT_CHECK in shape_check) */
  CDN_ERR_DTYPE = -3,
  CDN_ERR_HIP = -4,         /* a HIP runtime call or kernel launch failed             */
  CDN_ERR_UNSUPPORTED = -5, /* valid request outside what a fast path implements      */
  CDN_ERR_WORKSPACE = -6    /* workspace too small                                    */
};

int cdn_abi_version(void);
const char *cdn_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Generic deformable convolution -- the five roles of the reference extension.
 * Argument ORDER follows the reference (W before H in the three deform_conv_* functions,
 * H before W in the modulated ones; functions/dcn_deform_conv.py:51-56 vs :143-147).
 * Shapes: input [N,C,H,W]; offset [N, dg*2*kH*kW, Ho, Wo]; mask [N, dg*kH*kW, Ho, Wo];
 *         weight [Co, C/group, kH, kW]; output/gradOutput [N, Co, Ho, Wo],
 *         Ho = (H + 2*padH - (dilH*(kH-1)+1))/dH + 1  (cpp:187-190).
 * The reference's vestigial `columns` / `ones` buffer arguments and `im2col_step` are gone:
 * no column buffer is ever materialised.
 * ---------------------------------------------------------------------------------------- */

/* Replaces deform_conv_forward_cuda (dcn_deform_conv_cuda.cpp:151-258).
 * `output` is fully overwritten. */
int cdn_deform_conv_forward(const void *input, const void *weight, const void *offset,
                            void *output, int dtype, int64_t N, int64_t C, int64_t H, int64_t W,
                            int64_t Co, int kW, int kH, int dW, int dH, int padW, int padH,
                            int dilationW, int dilationH, int group, int deformable_group,
                            void *stream);

/* The same call with the reference's scratch argument put to use (round 6): `columns` of deform_conv_forward_cuda
 * (cpp:151-156, resized there, cpp:196-200) -> `scratch`.  For the CoDeNet call geometry (f32, depthwise 3x3, stride 1,
 * pad 1, dilation 1, deformable_group 1, C % 4 == 0, plane in LDS: ..._scratch_bytes != 0) one pass over the offsets
 * tests every pixel for the structure the reference's model always produces -- offset = anchor * t, exactly
 * (modules/dcn_deform_conv.py:319-325) -- and leaves t (or NaN) in scratch[N][H][W]; structured pixels then run the
 * module kernel's geometry (four axes, 25 cells per channel quad), any other pixel the generic nine taps: same sampling
 * positions bit for bit, fp32 re-association against cdn_deform_conv_forward only.  scratch == NULL or any other
 * geometry / dtype: exactly cdn_deform_conv_forward (which performs the same per-pixel test inside every workgroup). */
size_t cdn_deform_conv_forward_scratch_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int kW, int kH,
                                             int dW, int dH, int padW, int padH, int dilationW, int dilationH,
                                             int group, int deformable_group);
int cdn_deform_conv_forward_scratch(const void *input, const void *weight, const void *offset,
                                    void *output, int dtype, int64_t N, int64_t C, int64_t H, int64_t W,
                                    int64_t Co, int kW, int kH, int dW, int dH, int padW, int padH,
                                    int dilationW, int dilationH, int group, int deformable_group,
                                    void *scratch, size_t scratch_bytes, void *stream);

/* Replaces deform_conv_backward_input_cuda (cpp:260-371).
 * gradInput is ACCUMULATED into (caller zero-fills, as functions/dcn_deform_conv.py:73 does);
 * gradOffset is fully overwritten. */
int cdn_deform_conv_backward_input(const void *input, const void *offset, const void *gradOutput,
                                   void *gradInput, void *gradOffset, const void *weight,
                                   int dtype, int64_t N, int64_t C, int64_t H, int64_t W,
                                   int64_t Co, int kW, int kH, int dW, int dH, int padW, int padH,
                                   int dilationW, int dilationH, int group, int deformable_group,
                                   void *stream);

/* The same call with the reference's scratch argument put to use (round 6): `columns` of
 * deform_conv_backward_input_cuda (cpp:260-265) -> `scratch`.  For the CoDeNet call geometry (f32, depthwise 3x3,
 * stride 1, pad 1, dilation 1, deformable_group 1, plane images in LDS: ..._scratch_bytes != 0) the offsets are tested
 * for the anchor * t structure (as in cdn_deform_conv_forward_scratch; scratch = the [N][H][W] plane + a count of
 * pixels without it).  Every pixel structured: the module backward's geometry (four axes per pixel; 25 fixed-point
 * atomics per pixel and channel instead of 36; gradInput BIT-IDENTICAL to cdn_deform_conv_backward_input's, gradOffset
 * equal up to fp32 summation order over the channels).  Any pixel not: exactly cdn_deform_conv_backward_input.  The
 * choice is made on the device (both kernels are launched, one returns at once): no sync, capturable.
 * scratch == NULL or any other geometry / dtype: cdn_deform_conv_backward_input.
 * Two sizes: ..._scratch_min_bytes = the plane and the count ((N H W + 4) floats; less is CDN_ERR_WORKSPACE);
 * ..._scratch_bytes = what the call can USE: behind them one [N][18][H][W] plane of grad_offset terms per channel chunk
 * where grad_offset has a pass of its own (planes whose two LDS images leave room for fewer than eight channels: 64 x 64;
 * 302 MB for the 128 x 64 x 64 stage at batch 64 -- a quarter of what the reference's own `columns` takes there,
 * cpp:196-200) -- the chunks then STORE their terms and one pass sums the planes, instead of float atomics at the memory
 * side (~1.4 TB/s on MI355X).
 * Anything between the two sizes is valid and uses the atomics. */
size_t cdn_deform_conv_backward_input_scratch_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int kW,
                                                    int kH, int dW, int dH, int padW, int padH, int dilationW,
                                                    int dilationH, int group, int deformable_group);
size_t cdn_deform_conv_backward_input_scratch_min_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co, int kW,
                                                        int kH, int dW, int dH, int padW, int padH, int dilationW,
                                                        int dilationH, int group, int deformable_group);
int cdn_deform_conv_backward_input_scratch(const void *input, const void *offset, const void *gradOutput,
                                           void *gradInput, void *gradOffset, const void *weight,
                                           int dtype, int64_t N, int64_t C, int64_t H, int64_t W,
                                           int64_t Co, int kW, int kH, int dW, int dH, int padW, int padH,
                                           int dilationW, int dilationH, int group, int deformable_group,
                                           void *scratch, size_t scratch_bytes, void *stream);

/* Replaces deform_conv_backward_parameters_cuda (cpp:373-484).
 * gradWeight += scale * dL/dW  (accumulated, cpp:456-462; caller zero-fills). */
int cdn_deform_conv_backward_parameters(const void *input, const void *offset,
                                        const void *gradOutput, void *gradWeight, int dtype,
                                        int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                        int kW, int kH, int dW, int dH, int padW, int padH,
                                        int dilationW, int dilationH, int group,
                                        int deformable_group, float scale, void *stream);

/* Replaces modulated_deform_conv_cuda_forward (cpp:486-564).  bias may be NULL iff
 * with_bias == 0.  `output` is fully overwritten. */
int cdn_modulated_deform_conv_forward(const void *input, const void *weight, const void *bias,
                                      const void *offset, const void *mask, void *output,
                                      int dtype, int64_t N, int64_t C, int64_t H, int64_t W,
                                      int64_t Co, int kernel_h, int kernel_w, int stride_h,
                                      int stride_w, int pad_h, int pad_w, int dilation_h,
                                      int dilation_w, int group, int deformable_group,
                                      int with_bias, void *stream);

/* Replaces modulated_deform_conv_cuda_backward (cpp:566-679).
 * grad_input, grad_weight, grad_bias are ACCUMULATED into (caller zero-fills,
 * functions/dcn_deform_conv.py:157-161); grad_offset and grad_mask are overwritten.
 * Unlike the reference launcher (_kernel.cu:821, pad_h passed twice) pad_w is honoured. */
int cdn_modulated_deform_conv_backward(const void *input, const void *weight, const void *bias,
                                       const void *offset, const void *mask, void *grad_input,
                                       void *grad_weight, void *grad_bias, void *grad_offset,
                                       void *grad_mask, const void *grad_output, int dtype,
                                       int64_t N, int64_t C, int64_t H, int64_t W, int64_t Co,
                                       int kernel_h, int kernel_w, int stride_h, int stride_w,
                                       int pad_h, int pad_w, int dilation_h, int dilation_w,
                                       int group, int deformable_group, int with_bias,
                                       void *stream);

/* ------------------------------------------------------------------------------------------
 * CoDeNet fast paths (f32): the three steps of DeformConvWithOffsetScaleBoundPositive.forward
 * (modules/dcn_deform_conv.py:323-330) with the 18-channel offset tensor never materialised:
 *   s = Hardtanh(lo, hi)(conv1x1(x; C->1) + bias)                      :295,304-305,324
 *   d = depthwise 3x3 deformable conv sampling tap (i,j) at
 *       (h + (i-1) + (i-1)*(s-1),  w + (j-1) + (j-1)*(s-1))            :319-321,325 + :56-58
 *   y = conv1x1(d; C->Co)                                              :311-312,328
 * Tap positions are computed with exactly the reference's fp32 operation order
 * (t = s - 1; off = a*t; pos = float(h-1+i) + off), so they are bit-identical to the
 * positions the reference's im2col kernel derives from `anchor_offset * (s - 1)`.
 * ---------------------------------------------------------------------------------------- */

/* s[N,1,H,W] = clamp(sum_c w_scale[c]*x[n,c,h,w] + b_scale[0], lo, hi).
 * w_scale: [C] device floats, b_scale: device pointer to 1 float (may be NULL = 0). */
int cdn_codenet_scale_forward(const float *x, const float *w_scale, const float *b_scale,
                              float *s, int64_t N, int64_t C, int64_t H, int64_t W, float lo,
                              float hi, void *stream);

/* d[N,C,H,W] = depthwise deformable 3x3 of x with per-pixel scale s[N,1,H,W],
 * w_dw: [C,1,3,3].  stride 1, pad 1, dilation 1, groups = C, deformable_groups = 1. */
int cdn_codenet_dw_forward(const float *x, const float *s, const float *w_dw, float *d,
                           int64_t N, int64_t C, int64_t H, int64_t W, void *stream);

/* Backward of cdn_codenet_dw_forward.  grad_x [N,C,H,W] and grad_s [N,1,H,W] are fully
 * overwritten (grad_x is summed in LDS and stored once -- no global atomics; grad_s is
 * zeroed on `stream` and summed with one global float atomic per pixel and channel chunk);
 * grad_w [C,1,3,3] is ACCUMULATED into (caller zero-fills -- except when it lies directly behind grad_s in memory,
 * grad_w == grad_s + N*H*W (stored resolution for the _up2 form): the fill of grad_s then covers it).  Any of grad_x / grad_s / grad_w
 * may be NULL.  Requires the (H+2)x(W+2) plane to fit LDS twice (H*W up to ~17k pixels).
 * grad_s is dL/ds = sum_k (i-1)*dL/doff_y,k + (j-1)*dL/doff_x,k. */
/* ------------------------------------------------------------------------------------------
 * Backward of the two 1x1 convolutions around the gather (config e: the QAT step of quant_main.py; the
 * reference runs them as cuDNN calls under autograd: conv_scale modules/dcn_deform_conv.py:295,324 /
 * Quant_Conv2d quant_modules.py:314-321, conv_channel :311-312,328 / QuantBnConv2d :412-419).  NCHW fp32.
 *
 * cdn_codenet_pointwise_wgrad: grad_w [Co][C] = sum_{n,p} grad_y[n][co][p] * d[n][c][p] on f32 MFMA and,
 *   when grad_b != NULL, grad_b [Co] = sum_{n,p} grad_y[n][co][p]; both OVERWRITTEN, split-K partial tiles
 *   reduced in a fixed order (bitwise reproducible).  workspace: ..._wgrad_workspace_bytes(N,C,Co,HW) bytes,
 *   16-byte aligned, contents irrelevant.  (The data gradient grad_d = W^T grad_y is
 *   cdn_codenet_pointwise_forward with the transposed weights.)
 * cdn_codenet_scale_backward: backward of s_raw = conv1x1(x; C -> 1) + b given grad_s = dL/ds_raw [N][H*W]
 *   (the caller has applied the Hardtanh mask lo < s_raw < hi and the straight-through QuantAct):
 *   grad_x [N][C][H*W] += w_scale[c] * grad_s  (ACCUMULATED into, normally the gather's grad_x; may be NULL),
 *   grad_w_partial [N][C] = sum_p x * grad_s per image (overwritten; the caller sums over n; may be NULL).
 * ---------------------------------------------------------------------------------------- */
/* cdn_codenet_weight_prep: the per-forward WEIGHT transformation of Quant_Conv2d / QuantDeformConv2d / QuantBnConv2d
 *   (quant_modules.py:278-300 / 473-495 / 364-372 + SymmetricQuantFunction, quant_utils.py:207-225) in one launch:
 *   optional BN fold (scale_factor != NULL: [Co] = gamma / sqrt(running_var + eps), computed by the caller;
 *   w * scale_factor per output channel, bias_out = (conv_bias - mean) * scale_factor + beta, conv_bias may be NULL
 *   = 0), then per-output-channel symmetric fake-quantisation to `bits` bits (plain min / max ranges:
 *   per_channel=True, no --wt-percentile).  w [Co][K] -> w_q [Co][K].  Every operation is rounded like the
 *   reference's separate framework kernels: bit-identical to that composition. */
int cdn_codenet_weight_prep(const float *w, int64_t Co, int64_t K, const float *scale_factor, const float *bn_bias,
                            const float *bn_mean, const float *conv_bias, int bits, float *w_q, float *bias_out,
                            void *stream);
/* Training path without separate range passes: the three forward kernels of the stage can leave one {min, max} pair
 * per workgroup of the tensor they wrote (`partials`: 2 floats per pair, 8-byte aligned, *_range_partials(...) pairs),
 * and the QuantAct behind them reduces those pairs instead of re-reading the tensor:
 *   cdn_codenet_{scale,dw,pointwise}_forward_range  = the plain entry points + partials (same outputs);
 *   cdn_quantact_forward_partials                   = cdn_quantact_forward with the batch extremes from the pairs;
 *   cdn_quantact_relu_up2_forward_partials          = cdn_quantact_relu_up2_forward with the pairs of the PRE-ReLU tensor
 *                                                     (clamped at zero: the extremes of max(y, 0)).
 * Same range updates and values as the entry points with a range pass (min / max are exact). */
int64_t cdn_codenet_scale_range_partials(int64_t N, int64_t H, int64_t W);
int cdn_codenet_scale_forward_range(const float *x, const float *w_scale, const float *b_scale, float *s, int64_t N,
                                    int64_t C, int64_t H, int64_t W, float lo, float hi, float *partials, void *stream);
int64_t cdn_codenet_dw_range_partials(int64_t N, int64_t C, int64_t H, int64_t W);
int cdn_codenet_dw_forward_range(const float *x, const float *s, const float *w_dw, float *d, int64_t N, int64_t C,
                                 int64_t H, int64_t W, float *partials, void *stream);
int64_t cdn_codenet_pointwise_range_partials(int64_t N, int64_t Co, int64_t HW);
int cdn_codenet_pointwise_forward_range(const float *d, const void *d_state, const float *w_pw, const float *bias,
                                        const float *ep_scale, const float *ep_shift, float *y, int64_t N, int64_t C,
                                        int64_t Co, int64_t HW, int relu, float *partials, void *stream);
/* (d_state != NULL: d holds PRE-quantisation values and is fake-quantised with that QuantAct state while the kernel loads
 * it -- the values a separate cdn_quantact_forward pass would have stored; partials may then be NULL.)
 * cdn_quantact_forward_partials: out may be NULL (range update + parameters only: the consumer quantises on load);
 * state_copy (8 words, may be NULL) receives a snapshot of the state for consumers that outlive the QuantAct's next
 * call -- cdn_codenet_pointwise_wgrad_q in the backward pass. */
int cdn_quantact_forward_partials(const float *x, float *out, int64_t numel, float *x_min, float *x_max, void *state,
                                  const float *partials, int64_t n_partials, int bits, double momentum, int running,
                                  void *state_copy, void *stream);
/* The forward conv_channel of the QAT step on the int8 matrix cores (round 5; pwi8n_kernel, codenet_train.hip): same
 * arguments as cdn_codenet_pointwise_forward_range with d_state != NULL, for weights that are per-channel symmetric
 * <= 4-bit fake-quantised (w_q [Co][C] = q / ws, |q| <= 8: what cdn_codenet_weight_prep produces at bits <= 4) -- the
 * integer codes of both operands are summed exactly, y = (sum_c (L_c + zp) q_c) / (scale ws) + bias, as the inference
 * schedule does, instead of multiplying their fp32 forms on f32 MFMA (one rounding instead of C; agrees with
 * cdn_codenet_pointwise_forward_range to fp32 summation noise, equal on exact-arithmetic inputs).  A batch whose codes are
 * too wide for the kernel's nibble split (state word 6) runs on f32 MFMA inside the same launch.  The per-channel weight
 * scale is recovered from each row as m / max|w_q| with the smallest m in 1 ... 8 that puts the whole row on integers (any
 * weight_bit <= 4, --wt-percentile clamping included); a row that is on no such grid yields NaN outputs for its channel.
 *   ..._supported: C % 32 == 0, C <= 4096, HW % 32 == 0, Co <= 512;  workspace: ..._workspace_bytes, 256-byte aligned, contents
 *   irrelevant (the k-blocked weight codes are rebuilt by every call: the weights change every step);
 *   partials: ..._range_partials pairs, or NULL.
 * Reference: conv_channel under autograd, quant_modules.py:412-419 (F.conv2d on the fake-quantised operands). */
int cdn_codenet_pointwise_i8_supported(int64_t N, int64_t C, int64_t Co, int64_t HW);
/* Round 6: the QAT step's three producers -- scale prediction, gather, int8 pointwise -- with the QuantAct BEHIND them
 * updated by the launch's last workgroup (the fused inference schedule's arrival protocol, cdn::block_minmax_finish)
 * instead of per-workgroup {min, max} partials + a cdn_quantact_forward_partials update launch: same update arithmetic
 * (quant_modules.py:203-219: `+=` initialisation / two-rounding EMA), same extremes, nine launches fewer per step.
 *   counters: cdn_quantact_arrive_words() 32-bit words per QuantAct, zero before the first call, left zero by every call;
 *   state_copy (8 words, may be NULL): the state after the update -- what cdn_quantact_forward_partials' state_copy gave;
 *   ..._dw_forward_update: up2 != 0 = cdn_codenet_dw_up2_forward's convention (x, s stored, H x W up-sampled);
 *   ..._pointwise_i8_forward_update: relu_range != 0 = the QuantAct sits behind a ReLU (tracks max(y, 0));
 *   cdn_quantact_apply / cdn_quantact_relu_apply: the fake-quantisation [ReLU first; up != 0: + nearest x2] with the state
 *   as the producer left it -- the second half of cdn_quantact_forward_partials / cdn_quantact_relu[_up2]_forward_partials.
 * Reference: QuantAct.forward, quant_modules.py:203-225. */
int cdn_quantact_arrive_words(void);
int cdn_codenet_scale_forward_update(const float *x, const float *w_scale, const float *b_scale, float *s, int64_t N,
                                     int64_t C, int64_t H, int64_t W, float lo, float hi, float *x_min, float *x_max,
                                     void *state, void *counters, int bits, double momentum, void *state_copy,
                                     void *stream);
int cdn_codenet_dw_forward_update_supported(int64_t N, int64_t C, int64_t H, int64_t W, int up2);
int cdn_codenet_dw_forward_update(const float *x, const float *s, const float *w_dw, float *d, int64_t N, int64_t C,
                                  int64_t H, int64_t W, int up2, float *x_min, float *x_max, void *state, void *counters,
                                  int bits, double momentum, void *state_copy, void *stream);
int cdn_codenet_pointwise_i8_forward_update(const float *d, const void *d_state, const float *w_q, const float *bias,
                                            float *y, int64_t N, int64_t C, int64_t Co, int64_t HW, void *workspace,
                                            size_t workspace_bytes, int relu_range, float *x_min, float *x_max,
                                            void *state, void *counters, int bits, double momentum, void *stream);
int cdn_quantact_apply(const float *x, float *out, int64_t numel, const void *state, void *stream);
int cdn_quantact_relu_apply(const float *y, float *out, int64_t planes, int64_t H, int64_t W, int up, const void *state,
                            void *stream);
size_t cdn_codenet_pointwise_i8_workspace_bytes(int64_t N, int64_t C, int64_t Co, int64_t HW);
int64_t cdn_codenet_pointwise_i8_range_partials(int64_t N, int64_t C, int64_t Co, int64_t HW);
int cdn_codenet_pointwise_i8_forward_range(const float *d, const void *d_state, const float *w_q, const float *bias,
                                           float *y, int64_t N, int64_t C, int64_t Co, int64_t HW, float *partials,
                                           void *workspace, size_t workspace_bytes, void *stream);
/* The data gradient of the same conv, grad_d[n][c][p] = sum_co w_q[co][c] grad_y[n][co][p], with exact products on the bf16
 * matrix cores (round 5; pwb3n_kernel): grad_y / ws[co] split into three bf16 terms (exact), the 4-bit codes exact in
 * bf16, fp32 accumulation -- 3 bf16 MFMAs per 16 k instead of 8 f32 MFMAs.  fwd_workspace: the workspace the forward
 * call (cdn_codenet_pointwise_i8_forward_range, same N, C, Co, HW and weights) left behind: it holds the transposed bf16
 * codes and the reciprocal weight scales.  Agrees with cdn_codenet_pointwise_forward on the transposed weights to fp32
 * rounding noise.  Reference: autograd of conv_channel, quant_modules.py:412-419. */
int cdn_codenet_pointwise_dgrad_q4_supported(int64_t N, int64_t C, int64_t Co, int64_t HW);
int cdn_codenet_pointwise_dgrad_q4(const float *grad_y, const void *fwd_workspace, float *grad_d, int64_t N, int64_t C,
                                   int64_t Co, int64_t HW, void *stream);
/* cdn_codenet_pointwise_wgrad with d given as pre-quantisation values + the state that quantised them in the forward:
 * round 5: with whole 64 x 128 tiles (Co % 64 == 0, C % 128 == 0, HW % 64 == 0) the products are formed EXACTLY on the bf16
 * matrix cores -- d as the integer q' = round(scale d - zp) + zp - 128 in two bf16 terms, grad_y in three -- and
 * grad_w = (sum grad_y q' + 128 grad_b) / scale (pw_wgrad_q3_kernel; rounding noise against the f32-MFMA form, bitwise
 * reproducible like it); cdn_codenet_pointwise_wgrad_q_f32 keeps the f32-MFMA kernel (A/B, tests). */
int cdn_codenet_pointwise_wgrad_q(const float *grad_y, const float *d, const void *d_state, float *grad_w, float *grad_b,
                                  int64_t N, int64_t C, int64_t Co, int64_t HW, void *workspace, size_t workspace_bytes,
                                  void *stream);
int cdn_codenet_pointwise_wgrad_q_f32(const float *grad_y, const float *d, const void *d_state, float *grad_w, float *grad_b,
                                      int64_t N, int64_t C, int64_t Co, int64_t HW, void *workspace,
                                      size_t workspace_bytes, void *stream);
int cdn_quantact_relu_up2_forward_partials(const float *y, float *out, int64_t planes, int64_t H, int64_t W,
                                           float *x_min, float *x_max, void *state, const float *partials,
                                           int64_t n_partials, int bits, double momentum, int running, void *stream);
/* The same with the reference's --wt-percentile ranges (quant_modules.py:287-300): per output channel the range is
 * [k_low-th smallest, k_high-th largest] * shrink instead of [min, max] -- the caller passes
 *   K < 10 (every depthwise 3x3):  k_low = k_high = 1, shrink = 0.95f
 *   else:  k_low = ceil(K * 0.1 * 0.01), k_high = K - ceil(K * 99.9 * 0.01) + 1, shrink = 1   (torch.kthvalue ranks)
 * (k_low = k_high = 1, shrink = 1: exactly cdn_codenet_weight_prep).  Ranks up to 4 (channels of up to 4000 weights);
 * CDN_ERR_UNSUPPORTED beyond. */
int cdn_codenet_weight_prep_ranked(const float *w, int64_t Co, int64_t K, const float *scale_factor, const float *bn_bias,
                                   const float *bn_mean, const float *conv_bias, int bits, int k_low, int k_high,
                                   float shrink, float *w_q, float *bias_out, void *stream);
/* cdn_codenet_weight_prep_ranked for up to 8 tensors in ONE launch (round 5: the conv_scale and depthwise weights of the
 * three stages of a QAT step, and their three BN-folded pointwise weights -- launches at their launch floor): host
 * arrays of n entries; scale_factor / bn_bias / bn_mean / conv_bias / bias_out are arrays of pointers (or NULL arrays),
 * entry t of scale_factor NULL = no BN fold for tensor t.  Every row is prepared exactly as by the single-tensor call
 * (bit-identical). */
int cdn_codenet_weight_prep_multi(int n, const float *const *w, const int64_t *Co, const int64_t *K,
                                  const float *const *scale_factor, const float *const *bn_bias,
                                  const float *const *bn_mean, const float *const *conv_bias, const int *bits,
                                  const int *k_low, const int *k_high, const float *shrink, float *const *w_q,
                                  float *const *bias_out, void *stream);
/* Backward of the BN fold of cdn_codenet_weight_prep under the straight-through weight quantiser
 * (SymmetricQuantFunction.backward, quant_utils.py:227-229; autograd of quant_modules.py:365-372) in one launch:
 *   grad_w = grad_wq * scale_factor,  grad_gamma = (sum_k grad_wq * w + grad_bias * (conv_bias - mean)) / bn_std,
 *   grad_beta = grad_bias,  grad_conv_bias = grad_bias * scale_factor;  bn_std = sqrt(running_var + eps) as the caller
 *   computed it for the forward.  grad_bias / conv_bias may be NULL (= 0); every output may be NULL (not wanted). */
int cdn_codenet_weight_prep_backward(const float *grad_wq, const float *grad_bias, const float *w,
                                     const float *scale_factor, const float *bn_std, const float *bn_mean,
                                     const float *conv_bias, int64_t Co, int64_t K, float *grad_w, float *grad_gamma,
                                     float *grad_beta, float *grad_conv_bias, void *stream);
size_t cdn_codenet_pointwise_wgrad_workspace_bytes(int64_t N, int64_t C, int64_t Co, int64_t HW);
int cdn_codenet_pointwise_wgrad(const float *grad_y, const float *d, float *grad_w, float *grad_b, int64_t N,
                                int64_t C, int64_t Co, int64_t HW, void *workspace, size_t workspace_bytes,
                                void *stream);
int cdn_codenet_scale_backward(const float *x, const float *grad_s, const float *w_scale, float *grad_x,
                               float *grad_w_partial, int64_t N, int64_t C, int64_t H, int64_t W, void *stream);
/* The same with the Hardtanh backward folded in (F.hardtanh_backward of dcn_v2.py's scale clamp): grad_s is the gradient
 * with respect to the CLAMPED scale, s_clamped [N][H*W] the clamped value saved by the forward; the gradient passes
 * where lo < s_clamped < hi.  grad_wb_partial [N][C + 1] (may be NULL): columns 0..C-1 as above, column C =
 * sum_p of the masked gradient (the bias gradient's share of image n). */
int cdn_codenet_scale_backward_masked(const float *x, const float *grad_s, const float *s_clamped, float lo, float hi,
                                      const float *w_scale, float *grad_x, float *grad_wb_partial, int64_t N,
                                      int64_t C, int64_t H, int64_t W, void *stream);

/* The gather for a stage whose input is the nearest x2 up-sampling of a STORED tensor (stages 1-2 of the network:
 * shufflenetv2_dcn.py:303-308 puts an Upsample in front of them): x_stored [N][C][H/2][W/2], s_stored [N][H/2][W/2]
 * (the scale of a replicated tensor is constant over each 2x2 block), H, W = the stage's (output) resolution.
 * forward: d [N][C][H][W], bit-identical to cdn_codenet_dw_forward on the materialised up-sampled tensors; partials
 * (may be NULL): cdn_codenet_dw_up2_range_partials(N,C,H,W) {min,max} pairs of d.  backward (VERDICT r3 "next" #3;
 * replaces _kernel.cu:278-435 + the Upsample backward for these stages): grad_x [N][C][H/2][W/2] and grad_s
 * [N][H/2][W/2] with respect to the STORED tensors (the 2x2 sums of the up-sampling backward included), grad_w [C][9]
 * accumulated (+=); the four pixels of a block share their bilinear cells, so 25 instead of 100 LDS atomics per block
 * and channel.  grad_x / grad_s / grad_w may be NULL.  _supported: C % 4 == 0, even H, W, stored plane within LDS. */
int cdn_codenet_dw_up2_supported(int64_t N, int64_t C, int64_t H, int64_t W);
int64_t cdn_codenet_dw_up2_range_partials(int64_t N, int64_t C, int64_t H, int64_t W);
int cdn_codenet_dw_up2_forward(const float *x_stored, const float *s_stored, const float *w_dw, float *d, int64_t N,
                               int64_t C, int64_t H, int64_t W, float *partials, void *stream);
int cdn_codenet_dw_up2_backward(const float *x_stored, const float *s_stored, const float *w_dw, const float *grad_d,
                                float *grad_x, float *grad_s, float *grad_w, int64_t N, int64_t C, int64_t H, int64_t W,
                                void *stream);
int cdn_codenet_dw_backward_supported(int64_t H, int64_t W);   /* 1: the plane fits; 0: use the generic path */
int cdn_codenet_dw_backward(const float *x, const float *s, const float *w_dw,
                            const float *grad_d, float *grad_x, float *grad_s, float *grad_w,
                            int64_t N, int64_t C, int64_t H, int64_t W, void *stream);
/* The REPRODUCIBLE forms of the two gather backwards (round 5).  grad_s and grad_w of the entry points above are float
 * atomics over the channel chunks / the images -- as in the reference, whose _kernel.cu:278-435 accumulates with
 * atomicAdd -- so identical inputs give sums that differ in the last bits between runs.  These write per-workgroup
 * partials into a caller workspace and reduce them in a fixed order: bit-identical outputs for identical inputs; grad_s
 * and grad_w are OVERWRITTEN (not accumulated), grad_x as above.  _workspace_bytes: up2 != 0 for the up-sampled form
 * (H, W the stage's resolution there too); 0 = this form does not exist for the shape (plane beyond LDS). */
size_t cdn_codenet_dw_backward_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int up2);
int cdn_codenet_dw_backward_r(const float *x, const float *s, const float *w_dw, const float *grad_d, float *grad_x,
                              float *grad_s, float *grad_w, int64_t N, int64_t C, int64_t H, int64_t W,
                              float *workspace, void *stream);
int cdn_codenet_dw_up2_backward_r(const float *x_stored, const float *s_stored, const float *w_dw, const float *grad_d,
                                  float *grad_x, float *grad_s, float *grad_w, int64_t N, int64_t C, int64_t H,
                                  int64_t W, float *workspace, void *stream);

/* y[N,Co,HW] = sum_c w_pw[co,c] * d[n,c,p] (+ bias[co]) on f32 MFMA (exact f32 products,
 * f32 accumulate).  Optional epilogue: per-channel affine y*ep_scale[co] + ep_shift[co]
 * (a folded BatchNorm; either both NULL or both set), then ReLU if relu != 0. */
int cdn_codenet_pointwise_forward(const float *d, const float *w_pw, const float *bias,
                                  const float *ep_scale, const float *ep_shift, float *y,
                                  int64_t N, int64_t C, int64_t Co, int64_t HW, int relu,
                                  void *stream);

/* ------------------------------------------------------------------------------------------
 * QuantAct on device (portable_quantizer/quant_modules.py:163-225, asymmetric per-tensor branch
 * of AsymmetricQuantFunction, quantization_utils/quant_utils.py:172-200).  One call does, with
 * no host synchronisation:
 *   running != 0: batch min/max of x (or the caller's batch_min/batch_max device scalars, e.g.
 *                 the 0.1 / 99.9 percentiles of --act-percentile), then the reference's range
 *                 tracking on the x_min / x_max buffers IN PLACE ("+=" initialisation while
 *                 x_min == x_max, else EMA with `momentum`);
 *   always:       scale = (2^bits-1)/clamp(x_max-x_min,1e-10), zp = round(scale*x_min)+2^(bits-1),
 *                 q = round(scale*x - zp) (round-half-even, NOT clamped),
 *                 out = (q + zp)/scale (fp32, may alias x) and/or codes = q as int16.
 * `state` is a caller-owned device buffer of cdn_quantact_state_bytes() bytes, ZERO-INITIALISED before its first use
 * (words 0, 1 and 7 carry the range pass's atomics and arrival ticket and are left zero by every call); after the
 * call it holds {.., .., scale, zp, batch_min, batch_max} as fp32 words 2..5.
 * x, out must be 16-byte aligned, codes 8-byte aligned.  out and codes may be NULL.
 * ---------------------------------------------------------------------------------------- */
size_t cdn_quantact_state_bytes(void);

/* The k_lo-th and k_hi-th smallest elements (1-based, torch.kthvalue's k) of x[numel]: the order statistics that
 * --act-percentile / --wt-percentile use as the quantisation range (portable_quantizer/quantization_utils/
 * quant_utils.py:18-30, called per QuantAct forward at quant_modules.py:203-210).  Exact (the results are elements of
 * x); three histogram passes over x.  workspace: cdn_kth_values_workspace_bytes() bytes, 256-byte aligned, no
 * initialisation required.  numel < 2^32. */
size_t cdn_kth_values_workspace_bytes(void);
int cdn_kth_values(const float *x, int64_t numel, int64_t k_lo, int64_t k_hi, float *out_lo, float *out_hi,
                   void *workspace, size_t workspace_bytes, void *stream);
int cdn_quantact_forward(const float *x, float *out, int16_t *codes, int64_t numel, float *x_min,
                         float *x_max, void *state, const float *batch_min,
                         const float *batch_max, int bits, double momentum, int running,
                         void *stream);
/* Training-path block `ReLU(inplace) -> QuantAct -> Upsample(x2, nearest)` that follows every deform stage
 * (lib/models/networks/shufflenetv2_dcn.py:303-308 after quantize_model.py:79-81) as ONE QuantAct call that reads the
 * pre-ReLU tensor y [planes][H][W] once: range tracking on max(y, 0) exactly as cdn_quantact_forward would on the
 * ReLU output (x_min / x_max updated in place when running), out [planes][2H][2W] = the fake-quantised values
 * replicated 2x2.  cdn_up2_relu_backward: grad_y = 0 where y <= 0, else ((a + b) + c) + d over the four replicas of
 * grad_out in row-major order (straight-through QuantAct, quant_utils.py:202-204; torch's threshold backward: the
 * gradient passes where y is NaN).  Only grad_out must be 16-byte aligned. */
int cdn_quantact_relu_up2_forward(const float *y, float *out, int64_t planes, int64_t H, int64_t W, float *x_min,
                                  float *x_max, void *state, int bits, double momentum, int running, void *stream);
int cdn_up2_relu_backward(const float *grad_out, const float *y, float *grad_y, int64_t planes, int64_t H, int64_t W,
                          void *stream);
/* The same block WITHOUT materialising the Upsample (round 4): out [numel] = fake_quant(max(y, 0)) at stored
 * resolution for a consumer that reads its input through the up-sampling (cdn_codenet_dw_up2_*); partials (may be
 * NULL: a range pass over y) as in cdn_quantact_relu_up2_forward_partials.  cdn_relu_backward: grad_y = 0 where
 * y <= 0, else grad_out -- a NaN in y passes the gradient, as torch's ReLU backward does (the 2x2 sum of the
 * up-sampling backward has already happened in cdn_codenet_dw_up2_backward). */
int cdn_quantact_relu_forward(const float *y, float *out, int64_t numel, float *x_min, float *x_max, void *state,
                              const float *partials, int64_t n_partials, int bits, double momentum, int running,
                              void *stream);
int cdn_relu_backward(const float *grad_out, const float *y, float *grad_y, int64_t numel, void *stream);

/* ------------------------------------------------------------------------------------------
 * One whole up-sampling stage of the head as a fused kernel schedule (codenet_fused.hip):
 *   fp32 : DeformConvWithOffsetScaleBoundPositive -> BatchNorm2d -> ReLU            [-> Upsample]
 *          (modules/dcn_deform_conv.py:323-330, shufflenetv2_dcn.py:303-308)
 *   W4A8 : QuantDeformConvWithOffsetScaleBoundPositive -> ReLU -> QuantAct          [-> Upsample]
 *          (quant_modules.py:668-671, quantize_model.py:79-81)
 * The nearest x2 Upsample that FOLLOWS a stage is not executed: the next stage (x_up = 1) reads
 * its input at half resolution, and cdn_codenet_unpack_nchw materialises it for consumers outside
 * the fused path.  QuantAct min/max reductions run in the producing kernels' epilogues, the
 * fake-quantisation (same fp32 expression as cdn_quantact_forward) is applied by the consumer while
 * loading, so results equal the module-by-module composition.
 *
 *   x         stage input at STORED resolution (H>>x_up) x (W>>x_up); x_nhwc ? [N][pix][C] : [N][C][pix];
 *             x_up = 1 needs a channels-last input (CDN_ERR_UNSUPPORTED otherwise)
 *   x_qstate  NULL, or the QuantAct state of the producer: x then holds PRE-quantisation values
 *             (channels-last only) and is fake-quantised on load
 *   H, W      stage (output) resolution;  C -> Co channels
 *   w_scale [C], b_scale [1] (device, may be NULL), lo/hi: Hardtanh bounds
 *   w_dw [C,1,3,3], w_pw [Co,C], bias_pw [Co] or NULL; ep_scale/ep_shift [Co] or both NULL
 *             (W4A8: the already fake-quantised weights and the folded BN bias; fp32: BN as affine)
 *   w_pw_codes / w_pw_scale / w_pw_colsum: optional INTEGER form of the pointwise weights for the
 *             int8-MFMA path (used when the d quantiser is enabled): codes qw in [-8,7] as int8
 *             [Co][round_up(C,64)] zero padded and 16-byte aligned, per-channel scale sw[Co]
 *             (w' = qw / sw), column sums sum_c qw [Co] as int32.  NULL -> f32 MFMA on w_pw.
 *             The integer path computes sum_c (q_d + zp) * qw exactly and scales once; activation
 *             codes are NOT clamped to int8 (the reference does not clamp them).
 *   {s,d,r}_{min,max,state}: the three QuantAct of the stage (x_min/x_max buffers updated in place
 *             when running != 0; state as in cdn_quantact_forward); pass all three of a group NULL to
 *             disable that quantiser (fp32 path: all NULL)
 *   workspace cdn_codenet_stage_workspace_bytes(N,C,H,W,x_up) bytes (or more), 256-byte aligned.
 *             Its LAST 16 KiB hold workgroup arrival counters: zero them ONCE before the first call;
 *             every completed call leaves them zero again (QuantAct ranges are updated by the last
 *             workgroup of each producing kernel, no separate update launch).
 *   r_out     [N][H*W][Co] channels-last: act(pointwise(...)) BEFORE the output QuantAct (its
 *             parameters are left in r_state for the consumer)
 * ---------------------------------------------------------------------------------------- */
size_t cdn_codenet_stage_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int x_up);
/* 1 when cdn_codenet_stage_fused_forward implements this geometry (the stored plane must fit the
 * LDS-resident gather: 64- / 32-channel chunks up to ~1250 stored pixels = inputs up to ~544 px, thinner 16- / 8-
 * channel chunks up to ~4800 stored pixels = inputs up to ~1100 px), 0 otherwise: callers then keep the
 * module path (cdn_codenet_{scale,dw,pointwise}_forward, any plane size). */
int cdn_codenet_stage_supported(int64_t N, int64_t C, int64_t H, int64_t W, int x_nhwc, int x_up);
/* Diagnostics / parity tests: where cdn_codenet_stage_fused_forward leaves its intermediates in the workspace after a
 * call with these arguments (x_nhwc as passed, flags included): the clamped scale plane s BEFORE its QuantAct
 * ([N][stored pixels] floats) at byte offset 0, the gather output d BEFORE its QuantAct at *d_offset_bytes as
 * channels-last rows of *d_row_floats floats (the first C are the channels; CoDeNet2x stage 0 pads its rows).
 * int8_pointwise: the call passes w_pw_codes / scale / colsum and a d quantiser.  These are the tensors the
 * reference materialises between conv_scale / deform_conv / conv_channel (quant_modules.py:668-671). */
int cdn_codenet_stage_fused_intermediates(int64_t N, int64_t C, int64_t H, int64_t W, int x_nhwc, int x_up,
                                          int int8_pointwise, int64_t *d_offset_bytes, int64_t *d_row_floats);
/* What cdn_codenet_stage_fused_forward itself accepts: the above, or a stored plane too large for LDS, which it gathers
 * straight from global memory / L2 (round 4: inputs above ~1100 px; a size fallback with the module path's per-channel
 * expressions).  The byte-code entry points (cdn_codenet_stage_frozen*) keep the LDS-resident limit above. */
int cdn_codenet_stage_fused_supported(int64_t N, int64_t C, int64_t H, int64_t W, int x_nhwc, int x_up);
/* Schedule of the gather for an NCHW input at output resolution (stage 0) -- a PER-CALL choice OR-ed into the layout
 * argument of the stage entry points (`x_nhwc` of cdn_codenet_stage_fused_forward, `x_kind` of
 * cdn_codenet_stage_frozen[_chained]_forward); the library keeps no setting of its own (round 4: this replaces the
 * process-wide cdn_codenet_set_gather_mode, which contradicted "no global mutable state" above).  Nothing OR-ed in =
 * automatic (the persistent LDS-DMA kernel when every CU gets >= 2 items, the per-item kernel otherwise);
 * CDN_X_GATHER_PER_ITEM = always the per-item kernel; CDN_X_GATHER_PERSISTENT = persistent wherever its shape
 * conditions hold.  All compute bit-identical results (tests compare them).  No reference counterpart. */
#define CDN_X_GATHER_PER_ITEM 0x100
#define CDN_X_GATHER_PERSISTENT 0x200
#define CDN_X_GATHER_MASK 0x300
/* | CDN_X_ACT_PERCENTILE (--act-percentile, quant_modules.py:203-210): while the ranges are tracked (running != 0) the three
 * QuantActs of the stage follow the 0.1 % / 99.9 % order statistics of their inputs (cdn_kth_values) instead of the
 * batch extremes; needs the three QuantActs. */
#define CDN_X_ACT_PERCENTILE 0x400
/* | CDN_X_WCODES_KB (round 5): w_pw_codes holds, behind the row-major codes [Co][Cpad] (Cpad = round_up(C, 64)), at byte
 * offset cdn_codenet_wcodes_kb_offset(C, Co) = round_up(Co * Cpad, 256), a K-BLOCKED copy of the same codes
 *   kb[window][column][32]   window < Cpad / 32, column < cdn_codenet_wcodes_kb_columns(C, Co), 32 consecutive channels;
 *                            zero rows for column >= Co
 * which lets the int8 pointwise kernel of a long-K stage (C >= 512: stage 0) stream the weights with one coalesced
 * kilobyte per 32-column tile and window (pwi8s_kernel).  cdn_codenet_wcodes_kb_columns returns 0
 * where the library has no use for the copy (the flag is then an argument error).  Host-side weight preparation only; no
 * reference counterpart (the reference's conv_channel is a cuDNN 1x1 convolution on fake-quantised fp32 weights,
 * quant_modules.py:441-447).  Results are bit-identical with and without the copy. */
#define CDN_X_WCODES_KB 0x800
int64_t cdn_codenet_wcodes_kb_columns(int64_t C, int64_t Co);
int64_t cdn_codenet_wcodes_kb_offset(int64_t C, int64_t Co);
/* Diagnostics: the workgroups of the streaming int8 pointwise kernel (the instantiation taken for Co output columns, at
 * the launch's LDS size) that the runtime keeps resident per CU.  0: no such kernel for this Co; negative: the runtime's
 * error code. */
int cdn_codenet_pwi8s_resident_workgroups(int64_t Co);
/* Diagnostics / tests: the tile of the tiled int8 pointwise kernel for a dense [M][C] -> [M][Co] launch, as
 * rows * 1000 + columns (32128, 64128, 64064, 128064; 0: bad size).  The choice does not depend on the width of the
 * codes; launches that take the streaming kernel (4-bit codes with CDN_X_WCODES_KB) are not described by it. */
int cdn_codenet_pointwise_i8_tile(int64_t M, int64_t C, int64_t Co);
/* | CDN_X_DEFER_RANGE and the phase bits (round 5; SURVEY.md section 8e, collective 3 -- the multi-process parity mode in
 * which R ranks x B images track the ranges of ONE R*B-image run; the reference's only multi-GPU mechanism,
 * lib/models/data_parallel.py:64-84, scatters one batch and so has batch-global ranges by construction): the stage call
 * is split at its three QuantActs so that the caller can all-reduce the batch extremes between the kernels.
 *   CDN_X_PHASE_SCALE / _GATHER / _POINTWISE  run only the named steps (none named = all three); the intermediates stay
 *                       in the workspace, so the calls of one stage must pass the same workspace and arguments;
 *   CDN_X_DEFER_RANGE   the producers only MEASURE (needs running != 0 and the three QuantActs; not with
 *                       CDN_X_ACT_PERCENTILE): each leaves its batch {min, max} in state words [4], [5] (as floats) and
 *                       does not touch the range; the caller reduces them over the ranks and commits with
 *                       cdn_quantact_commit_range before the next phase reads the state.
 * cdn_quantact_commit_range: the QuantAct update (quant_modules.py:203-219: initialisation or momentum step, then scale /
 * zero point) from `range` = {min, max} on the device; the code-width flag (state word [6]) follows THIS rank's extremes
 * in words [4], [5]. */
#define CDN_X_DEFER_RANGE 0x1000
#define CDN_X_PHASE_SCALE 0x2000
#define CDN_X_PHASE_GATHER 0x4000
#define CDN_X_PHASE_POINTWISE 0x8000
#define CDN_X_PHASE_MASK 0xE000
/* | CDN_W_CODES_8BIT (W8A8): the int8 weight codes handed to the call (`w_pw_codes` / `w_codes`) may hold ANY int8 value
 * (per-channel symmetric weights of up to 8 bits, q in [-128, 127]).  A launcher cannot see the width of device bytes, so
 * the caller states it, per call (no library state); the flag is OR-ed into
 *   `x_nhwc` of cdn_codenet_stage_fused_forward,
 *   `relu`   of cdn_codenet_pointwise_nhwc_forward / _mixed_forward / _mixed_forward_n and
 *            cdn_codenet_heads_pointwise_forward (the epilogue sees relu without the flag),
 *   `running` of cdn_codenet_pwdw_s2_forward / _apply (for the range-only pass of the 1x1 conv inside _forward);
 * the head tail, which has no int argument, has sibling entries with a `w_bits` argument
 * (cdn_codenet_head_tail_small_w_forward / cdn_codenet_head_tail_small_q8_w_forward).
 * WITHOUT the flag these entries assume |q| <= 8 (<= 4-bit codes), as before the flag existed: the kernels that split the
 * activation code into two nibble planes multiply the high plane with 16 * q held in a byte, and an 8-bit code wraps
 * silently.  With it the same kernels keep the high plane's sums in an accumulator of their own and form
 * acc_lo + 16 * acc_hi in int32 (exact for C <= 4096, which is checked); long-K stages take the tiled
 * kernel instead of the streaming one (CDN_X_WCODES_KB is accepted and its copy not read).  Results with the flag on
 * <= 4-bit codes are those without it, bit for bit.
 * Entries that NEVER needed the flag, because their arithmetic does not depend on the width of the weight byte -- "4-bit"
 * in their descriptions named the network they were written for, not a limit: the byte-code entries of the serving mode
 * (cdn_codenet_pointwise_q8[_strided]_forward, cdn_codenet_dwpw_q8_forward, cdn_codenet_stage_frozen[_chained]_forward: int8
 * activation codes x int8 weight codes, one product plane), the recomputing kernel of cdn_codenet_pwdw_s2_forward / _apply
 * (the 16 multiplies the SUM of the high plane) and the bf16 x 3 kernels behind a_gen / final-valued inputs of the pointwise entries (|q| <= 128
 * is exact in bf16).  The training entries (cdn_codenet_pointwise_i8_*, cdn_codenet_weight_prep*) stay at <= 4 bits: their
 * scale recovery knows the grids m = 1 ... 8 only.  (0x10000 stays an invalid value of x_nhwc.) */
#define CDN_W_CODES_8BIT 0x20000
int cdn_quantact_commit_range(float *x_min, float *x_max, void *state, const float *range, int bits, double momentum,
                              int running, void *stream);
int cdn_codenet_stage_fused_forward(
    const float *x, int x_nhwc, int x_up, const void *x_qstate, int64_t N, int64_t C, int64_t Co,
    int64_t H, int64_t W, const float *w_scale, const float *b_scale, float lo, float hi,
    const float *w_dw, const float *w_pw, const signed char *w_pw_codes, const float *w_pw_scale,
    const int *w_pw_colsum, const float *bias_pw, const float *ep_scale, const float *ep_shift,
    int relu, float *s_min, float *s_max, void *s_state, float *d_min,
    float *d_max, void *d_state, float *r_min, float *r_max, void *r_state, int bits,
    double momentum, int running, void *workspace, size_t workspace_bytes, float *r_out,
    void *stream);

/* ------------------------------------------------------------------------------------------
 * FROZEN-RANGE schedule with byte codes in HBM (serving mode; not the reference's default behaviour).
 * `running_stat` is a plain attribute of the reference's QuantAct (portable_quantizer/quant_modules.py:172,181);
 * with running_stat = False the range update (:203-219) is skipped, every QuantAct is a fixed affine grid
 * (quant_utils.py:60-75,193-200) and stops being a batch-global dependency.  Activations then cross HBM as
 * one byte per element: the code q = round(scale*x - zp), in [-128,127] inside the range; value = (q + zp) / scale.
 * The reference does not clamp codes; a byte must: a code outside [-128,127] is saturated and *overflow
 * (a device word the caller zeroes) is set to 1 -- recompute that batch with cdn_codenet_stage_fused_forward
 * (running = 0), to which the results are otherwise bit-identical.
 *
 * cdn_quantact_frozen_params   state[i] words [2],[3] = (scale, zero-point) of x_min[i] / x_max[i] for up to 64
 *            QuantActs in ONE launch (host arrays of device pointers); word [6] (the running-range epilogues'
 *            wide-code flag) is cleared.  Call it once per step before the frozen kernels (or whenever a range
 *            buffer changed).
 * cdn_codenet_stage_frozen_forward   one stage: scale 1x1 -> QuantAct -> gather / depthwise -> QuantAct (bytes)
 *            -> int8-MFMA pointwise + bias -> ReLU -> QuantAct (bytes).  3 launches.
 *   x / x_kind   0: [N][C][H][W] fp32 final values (a PyTorch backbone), x_state NULL
 *                1: [N][Hs*Ws][C] fp32 pre-quantisation values + their quantiser x_state
 *                2: [N][Hs*Ws][C] byte codes of the quantiser x_state (the previous stage's r8_out)
 *                (Hs, Ws) = (H >> x_up, W >> x_up): x_up = 1 folds the nearest x2 Upsample; C % 4 == 0
 *   weights      as cdn_codenet_stage_fused_forward (the integer form of the pointwise weights is required)
 *   {s,d,r}_state  QuantAct device states with current (scale, zero-point) -- see cdn_quantact_frozen_params
 *   workspace    cdn_codenet_stage_frozen_workspace_bytes(N,C,H,W,x_up) bytes, 256-byte aligned
 *   r8_out       [N][H*W][Co] byte codes of the r quantiser (at stage resolution, not up-sampled)
 * cdn_codenet_pointwise_q8_forward   the pointwise step alone (detection heads): a [M][C] byte codes of a_state;
 *            output either r8_out (byte codes of r_state) or r_out (fp32 pre-quantisation values).
 * cdn_codenet_expand_codes     byte codes -> the fp32 values level / scale (for consumers that take fp32 + the
 *            quantiser state; fake-quantising level / scale again returns the same value).
 * ---------------------------------------------------------------------------------------- */
int cdn_quantact_frozen_params(int n, float *const *x_min, float *const *x_max, void *const *state, int bits,
                               void *stream);
/* The same launch also clears `clear_bytes` bytes at `clear` (16-byte aligned, multiple of 16): the integer scale sums
 * of the chained frozen schedule, cdn_codenet_stage_frozen_chained_forward. */
int cdn_quantact_frozen_params_clear(int n, float *const *x_min, float *const *x_max, void *const *state, int bits,
                                     void *clear, size_t clear_bytes, void *stream);
size_t cdn_codenet_stage_frozen_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int x_up);
int cdn_codenet_stage_frozen_forward(
    const void *x, int x_kind, int x_up, const void *x_state, int64_t N, int64_t C, int64_t Co, int64_t H, int64_t W,
    const float *w_scale, const float *b_scale, float lo, float hi, const float *w_dw,
    const signed char *w_pw_codes, const float *w_pw_scale, const int *w_pw_colsum, const float *bias_pw, int relu,
    const void *s_state, const void *d_state, const void *r_state, void *workspace, size_t workspace_bytes,
    signed char *r8_out, unsigned *overflow, void *stream);
/* The same stage, CHAINED with its neighbours (frozen serving schedule only): the scale prediction of stage k+1 --
 * s_raw = b + sum_co (qw_s[co] / sw) * ((q_r + zp_r) / sc_r), a sum of integer products over one denominator -- is
 * accumulated by stage k's pointwise epilogue as exact int32 sums and finished by stage k+1's gather with ONE rounding,
 * s_raw = clamp(b + sums / (sw * sc_r), lo, hi), instead of a scale launch that re-reads r (quant_modules.py:668-669
 * evaluate the same sum as an fp32 convolution: this is a DECLARED non-bit-identical variant -- the exact sum rounded
 * once -- checked against the oracle within its code-flip tolerance, tests/test_gpu_frozen.py).
 *   s_sums_in         [N][(H/2)*(W/2)] int32 from the previous stage (needs x_kind 2, x_up 1) or NULL (scale launch);
 *   w_scale_sw        device scalar: scale of this stage's conv_scale weight codes (w = codes / sw), with s_sums_in
 *   next_scale_codes  [Co] int8 codes of the NEXT stage's conv_scale weights, s_sums_out [N][H*W] int32 that must be
 *                     ZERO on entry (cdn_quantact_frozen_params_clear clears it in the step's first launch; a separate
 *                     memset node costs 4.7 us) and holds the sums afterwards, or both NULL. */
int cdn_codenet_stage_frozen_chained_forward(
    const void *x, int x_kind, int x_up, const void *x_state, int64_t N, int64_t C, int64_t Co, int64_t H, int64_t W,
    const float *w_scale, const float *b_scale, float lo, float hi, const float *w_dw,
    const signed char *w_pw_codes, const float *w_pw_scale, const int *w_pw_colsum, const float *bias_pw, int relu,
    const void *s_state, const void *d_state, const void *r_state, void *workspace, size_t workspace_bytes,
    signed char *r8_out, unsigned *overflow, const int *s_sums_in, const float *w_scale_sw,
    const signed char *next_scale_codes, int *s_sums_out, void *stream);
int cdn_codenet_pointwise_q8_forward(const signed char *a, const void *a_state, int64_t M, int64_t C, int64_t Co,
                                     const signed char *w_codes, const float *w_scale, const int *w_colsum,
                                     const float *bias, int relu, const void *r_state, signed char *r8_out,
                                     float *r_out, unsigned *overflow, void *stream);
/* Byte-code counterparts of the layers around the hot path (frozen serving mode: every QuantAct at running_stat
 * False; same arithmetic as cdn_codenet_{pointwise,dw3x3}_nhwc_forward / cdn_codenet_stem_forward on
 * the values (q + zp) / scale, one byte per element in HBM; a saturated output code sets *overflow):
 *   cdn_codenet_pointwise_q8_strided_forward  cdn_codenet_pointwise_q8_forward with row strides lda / ldo (bytes / elements
 *       per row, 0 = dense, lda % 4 == 0) and an optional output channel map (out_map[co] = slot of channel co:
 *       the shuffle-free unit layout of pipeline.FusedBackbone);
 *   cdn_codenet_stem_q8_forward   layer0: dense 3x3 conv 3 -> 24 (stride 2 / 4, pad 1) + folded BN + ReLU on the NCHW
 *       fp32 image -> codes of its QuantAct, channels-last rows of ld_out bytes (shufflenetv2_dcn.py:205-214);
 *   cdn_codenet_dw3x3_q8_forward  depthwise 3x3 (stride 1 / 2, pad 1) + folded-BN bias [+ ReLU] on codes, rows of
 *       ld_in / ld_out bytes holding round_up(C, 4) channels. */
int cdn_codenet_pointwise_q8_strided_forward(
    const signed char *a, const void *a_state, int64_t M, int64_t C, int64_t Co, int64_t lda, int64_t ldo,
    const signed char *w_codes, const float *w_scale, const int *w_colsum, const float *bias, int relu,
    const int *out_map, const void *r_state, signed char *r8_out, float *r_out, unsigned *overflow, void *stream);
int cdn_codenet_stem_q8_forward(const float *img, int64_t N, int64_t H, int64_t W, int64_t Co, int stride,
                                const float *w, const float *bias, int relu, const void *r_state,
                                signed char *out8, int64_t ld_out, unsigned *overflow, void *stream);
/* MaxPool2d(3, stride 2, padding 1) on byte codes (the "S2 + MaxPool" stems; the maximum of the codes is the code of
 * the maximum: the pool follows the QuantAct): a8 [N][H*W] rows of ld_in bytes -> out8 [N][Ho*Wo] rows of ld_out bytes. */
int cdn_codenet_maxpool3x3s2_q8_forward(const signed char *a8, int64_t N, int64_t C, int64_t H, int64_t W, int64_t ld_in,
                                        int64_t ld_out, signed char *out8, void *stream);
int cdn_codenet_dw3x3_q8_forward(const signed char *a8, const void *a_state, int64_t N, int64_t C, int64_t H,
                                 int64_t W, int stride, int64_t ld_in, int64_t ld_out, const float *w,
                                 const float *bias, int relu, const void *r_state, signed char *out8,
                                 unsigned *overflow, void *stream);
/* cdn_codenet_dw3x3_q8_forward followed by cdn_codenet_pointwise_q8_strided_forward in ONE launch: the depthwise output
 * (codes of d_state) is computed into the LDS operand tile of the 1x1 conv and never stored.  Bit-identical to the two
 * calls.  Geometry: cdn_codenet_dwpw_q8_supported (output width 8 / 16 / 32 or a multiple of 64, Ho * Wo % 64 == 0,
 * C <= 512, Co <= 256); a8 rows of ld_in bytes, outputs rows of ldo bytes (0 = Co) through the optional out_map. */
int cdn_codenet_dwpw_q8_supported(int64_t C, int64_t H, int64_t W, int stride, int64_t Co);
int cdn_codenet_dwpw_q8_forward(const signed char *a8, const void *a_state, int64_t N, int64_t C, int64_t H, int64_t W,
                                int stride, int64_t ld_in, const float *w_dw, const float *b_dw, int dw_relu,
                                const void *d_state, int64_t Co, const signed char *w_codes, const float *w_scale,
                                const int *w_colsum, const float *bias, int relu, int64_t ldo, const int *out_map,
                                const void *r_state, signed char *r8_out, unsigned *overflow, void *stream);
int cdn_codenet_expand_codes(const signed char *a, const void *a_state, float *out, int64_t numel, void *stream);

/* The FIRST 1x1 convolutions of the detection heads as ONE launch (round 6): n_heads (2-4) problems of 64 output columns
 * on one channels-last input a [M][C] (pre-quantisation values + its QuantAct state) -- the three heads of the reference
 * (shufflenetv2_dcn.py:244-271; W4A8: QuantDepthwiseNode's quant_convbn1, quant_modules.py:1013-1071) all read the last
 * stage's output.  w / w_codes / w_scale / w_colsum / bias: the heads' int8 forms CONCATENATED along the output rows
 * (row h * 64 + co; w = the f32 fake-quantised weights for wide-code batches); head h writes out + h * head_stride as a
 * dense [M][64] buffer (out_map: device int[64 * n_heads] = column % 64) and updates ITS QuantAct (r_min[h], r_max[h],
 * r_state[h]; workspaces[h]: cdn_codenet_aux_workspace_bytes(), zero-initialised, one per head) in the launch's last
 * workgroup of its column group.  Same sums as n_heads calls of cdn_codenet_pointwise_nhwc_forward: bit-identical. */
int cdn_codenet_heads_pointwise_supported(int64_t M, int64_t C, int n_heads);
int cdn_codenet_heads_pointwise_forward(
    const float *a, const void *a_qstate, int64_t M, int64_t C, int n_heads, const float *w,
    const signed char *w_codes, const float *w_scale, const int *w_colsum, const float *bias, int relu,
    float *const *r_min, float *const *r_max, void *const *r_state, int bits, double momentum, int running,
    void *const *workspaces, size_t workspace_bytes, const int *out_map, float *out, int64_t head_stride, void *stream);

/* Chained fp32 stages (round 6; VERDICT r5 weak #2: cfg2 is ten launches of 6-20 us).  Without QuantActs (the fp32 model)
 * the next stage's scale prediction s' = Hardtanh(conv1x1(relu(bn(y)); Co -> 1) + b) (modules/dcn_deform_conv.py:295-305,
 * 323-330 applied to the next module's input) is linear in this stage's output rows: the streaming f32 pointwise kernel
 * leaves, per column tile, the dot product of its output columns with next_w_scale [Co] in parts_out[part][N * H * W],
 * and the next stage -- called with parts_in / n_parts_in -- sums the planes in order, adds its bias and clamps while its
 * gather stages the scale plane: its scale launch is gone (fp32 re-association against the scale kernel's order; the fp32
 * schedule's parity bound is 1e-3 against the oracle).  ..._chain_parts: planes the pointwise of (N, C -> Co, H x W)
 * leaves, 0 = no chained form (then call cdn_codenet_stage_fused_forward).  Arguments as cdn_codenet_stage_fused_forward
 * without the QuantAct and int8 ones; parts_in == NULL: the scale kernel runs; next_w_scale == parts_out == NULL: nothing
 * is left for a next stage. */
int cdn_codenet_stage_chain_parts(int64_t N, int64_t C, int64_t Co, int64_t H, int64_t W);
int cdn_codenet_stage_fused_forward_chain(
    const float *x, int x_nhwc, int x_up, const void *x_qstate, int64_t N, int64_t C, int64_t Co,
    int64_t H, int64_t W, const float *w_scale, const float *b_scale, float lo, float hi,
    const float *w_dw, const float *w_pw, const float *bias_pw, const float *ep_scale, const float *ep_shift,
    int relu, void *workspace, size_t workspace_bytes, float *r_out, const float *parts_in, int n_parts_in,
    const float *next_w_scale, float *parts_out, void *stream);

/* out_nchw[n][c][(h<<up)+dy][(w<<up)+dx] = fq(r_nhwc[n][h*W+w][c]): channels-last -> NCHW with the
 * nearest x2 up-sampling (up = 1) and, if r_qstate != NULL, the fake-quantisation applied. */
int cdn_codenet_unpack_nchw(const float *r_nhwc, const void *r_qstate, float *out_nchw, int64_t N,
                            int64_t C, int64_t H, int64_t W, int up, void *stream);

/* ------------------------------------------------------------------------------------------
 * The layers that consume the hot path's output: the detection heads
 *   fp32 : Conv2d 1x1 -> BN -> ReLU -> Conv2d 3x3 depthwise -> BN -> ReLU -> Conv2d 1x1 (+bias)
 *          (lib/models/networks/shufflenetv2_dcn.py:244-271)
 *   W4A8 : QuantDepthwiseNode = QuantBnConv2d -> ReLU -> QuantAct -> QuantBnConv2d (depthwise) ->
 *          ReLU -> QuantAct -> Quant_Conv2d            (portable_quantizer/quant_modules.py:1013-1071)
 * run on the same kernels as the stages, on channels-last activations, so the heads read the last
 * stage's output at HALF resolution (the 1x1 conv of a nearest-up-sampled tensor is the up-sampled
 * 1x1 conv; the depthwise kernel up-samples by addressing) and cdn_codenet_unpack_nchw is not needed.
 * Range tracking of the output QuantAct (r_min / r_max / r_state, all three or none) runs in the
 * kernel's epilogue as in the stage schedule; a_qstate != NULL fake-quantises the input while loading.
 * workspace: cdn_codenet_aux_workspace_bytes() bytes, 256-byte aligned, required when r_state != NULL;
 * its LAST 16 KiB are arrival counters: zero them once, every call leaves them zero.
 * ---------------------------------------------------------------------------------------- */
size_t cdn_codenet_aux_workspace_bytes(void);

/* out[m][co] = act( sum_c fq(a[m][c]) * w[co][c] + bias[co] ) (* ep_scale + ep_shift before act),
 * a [M][C] with row stride lda floats, out [M][Co] with row stride ldo (0 = dense; strides let a and
 * out be channel ranges of wider channels-last tensors: the split halves of a ShuffleNetV2 unit),
 * w [Co][C] fp32 (fake-quantised already for W4A8).  w_codes / w_scale / w_colsum: optional integer
 * form as in cdn_codenet_stage_fused_forward: int8 MFMA on integer codes when a_qstate is given too;
 * with a_qstate NULL (final-valued input, e.g. a ShuffleNetV2 unit's first 1x1 whose channels carry
 * different generations of the running QuantAct) the exact-product bf16 x 3 split kernel: a = hi + mid + lo
 * in bf16 (exact), weight codes exact in bf16, fp32 accumulation, scaled by 1 / w_scale[co]. */
int cdn_codenet_pointwise_nhwc_forward(
    const float *a, const void *a_qstate, int64_t M, int64_t C, int64_t Co, int64_t lda, int64_t ldo,
    const float *w,
    const signed char *w_codes, const float *w_scale, const int *w_colsum, const float *bias,
    const float *ep_scale, const float *ep_shift, int relu, float *r_min, float *r_max, void *r_state,
    int bits, double momentum, int running, void *workspace, size_t workspace_bytes, float *out,
    void *stream);

/* The first 1x1 conv (+ folded BN + ReLU + QuantAct) of a stride-2 ShuffleNetV2 unit RECOMPUTED inside its depthwise
 * 3x3, stride 2 (QuantBaseNode branch 2, portable_quantizer/quant_modules.py:809-907: quant_convbn1 -> ReLU -> quant_act1
 * -> quant_convbn2 -> quant_act2), round 4: in layer 1 the conv's output at input resolution (58 channels, fp32 because
 * the batch-global range of quant_act1 must be known before it can be quantised) is 243 MB at batch 64, 512 x 512.  Two
 * launches: a RANGE-ONLY pass of the int8 pointwise kernel (computes the conv, stores nothing, updates m_min / m_max /
 * m_state exactly as cdn_codenet_pointwise_mixed_forward would), then the depthwise kernel producing its input rows from
 * x with the same exact integer sums and epilogue expression -- bit-identical to the two stored-tensor calls.
 *   x [N][H*W][ld_x] pre-quantisation values of the input QuantAct x_qstate (one state), Cin <= 32 channels (% 4);
 *   w_pw / codes / scale / colsum / bias_pw as in cdn_codenet_pointwise_mixed_forward (C outputs, C <= 128);
 *   w_dw [C][9], bias_dw [C] or NULL; out [N][Ho*Wo][ld_out] pre-quantisation values of the output QuantAct
 *   (r_min / r_max / r_state, may be NULL), Ho = (H - 1) / 2 + 1; workspace as the other layer entry points. */
int cdn_codenet_pwdw_s2_supported(int64_t N, int64_t Cin, int64_t C, int64_t H, int64_t W);
int cdn_codenet_pwdw_s2_forward(
    const float *x, const void *x_qstate, int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t ld_x,
    const float *w_pw, const signed char *w_pw_codes, const float *w_pw_scale, const int *w_pw_colsum,
    const float *bias_pw, float *m_min, float *m_max, void *m_state, int64_t C, const float *w_dw, const float *bias_dw,
    int64_t ld_out, float *r_min, float *r_max, void *r_state, int bits, double momentum, int running, void *workspace,
    size_t workspace_bytes, float *out, void *stream);
/* The second half of cdn_codenet_pwdw_s2_forward alone (same arguments): the caller has already run the range-only pass
 * of the 1x1 conv itself -- cdn_codenet_pointwise_mixed_forward(x, x_qstate, NULL, N*H*W, Cin, C, ld_x, 0, w_pw, ...,
 * relu = 1, NULL, m_min, m_max, m_state, ..., out = NULL) -- e.g. to fork other work between the two. */
int cdn_codenet_pwdw_s2_apply(
    const float *x, const void *x_qstate, int64_t N, int64_t Cin, int64_t H, int64_t W, int64_t ld_x,
    const float *w_pw, const signed char *w_pw_codes, const float *w_pw_scale, const int *w_pw_colsum,
    const float *bias_pw, float *m_min, float *m_max, void *m_state, int64_t C, const float *w_dw, const float *bias_dw,
    int64_t ld_out, float *r_min, float *r_max, void *r_state, int bits, double momentum, int running, void *workspace,
    size_t workspace_bytes, float *out, void *stream);
/* Mixed-generation variants (ShuffleNetV2 layers WITHOUT a physical channel shuffle):
 * the activation tensor of a layer keeps every channel in a fixed physical slot, pre-quantisation values,
 * and channel c was produced under generation a_gen[c] of the layer's running block-output QuantAct
 * (quant_modules.py:809-907 calls that one QuantAct once per branch, so its range moves between calls).
 * a_qstate then points at an ARRAY of QuantAct states, cdn_quantact_state_bytes() apart; a consumer
 * fake-quantises channel c with state a_gen[c] while loading.  concat + channel_shuffle become index
 * bookkeeping on the host: weight columns are permuted to the physical order (zero columns for the
 * pass-through half of a unit) and out_map[co] names the slot output channel co is written to (NULL:
 * slot co).  a_gen == NULL: exactly cdn_codenet_pointwise_nhwc_forward / cdn_codenet_dw3x3_nhwc_forward.
 * Pointwise only (round 4): a_gen[c] == 255 marks a column whose weight codes are all zero (the pass-through half of a
 * shuffle-free unit row); the kernel may skip whole 32-channel windows of such columns (x * 0 adds an exact zero).
 * The pointwise form needs the 4-bit weight codes (bf16 split kernel) and C <= 512. */
int cdn_codenet_pointwise_mixed_forward(
    const float *a, const void *a_qstate, const unsigned char *a_gen, int64_t M, int64_t C, int64_t Co,
    int64_t lda, int64_t ldo, const float *w, const signed char *w_codes, const float *w_scale,
    const int *w_colsum, const float *bias, const float *ep_scale, const float *ep_shift, int relu,
    const int *out_map, float *r_min, float *r_max, void *r_state, int bits, double momentum, int running,
    void *workspace, size_t workspace_bytes, float *out, void *stream);
/* The same call with the NUMBER of states a_qstate holds (round 6; 0: unknown = the call above): with 1 <= n_gens <= 16
 * the streaming kernel loads all of them together with the generation bytes -- one memory round trip of the prologue
 * instead of two dependent ones (a state's address otherwise waits for its generation byte).  Every a_gen[c] other than
 * 255 must be < n_gens. */
int cdn_codenet_pointwise_mixed_forward_n(
    const float *a, const void *a_qstate, const unsigned char *a_gen, int n_gens, int64_t M, int64_t C, int64_t Co,
    int64_t lda, int64_t ldo, const float *w, const signed char *w_codes, const float *w_scale,
    const int *w_colsum, const float *bias, const float *ep_scale, const float *ep_shift, int relu,
    const int *out_map, float *r_min, float *r_max, void *r_state, int bits, double momentum, int running,
    void *workspace, size_t workspace_bytes, float *out, void *stream);
int cdn_codenet_dw3x3_mixed_forward(
    const float *a, const void *a_qstate, const unsigned char *a_gen, int64_t N, int64_t C, int64_t H,
    int64_t W, int up, int stride, int64_t ld_in, int64_t ld_out, const float *w, const float *bias,
    const float *ep_scale, const float *ep_shift, int relu, float *r_min, float *r_max, void *r_state,
    int bits, double momentum, int running, void *workspace, size_t workspace_bytes, float *out,
    void *stream);

/* Depthwise 3x3, pad 1, stride 1 or 2, channels-last: a [N][H*W][ld_in] at its STORED resolution H x W,
 * w [C][9], bias / ep_scale / ep_shift [C] or NULL, out [N][Ho*Wo][ld_out] with
 *   up = 1 (stride 1 only): the input is nearest x2 up-sampled on the fly, Ho x Wo = 2H x 2W
 *   stride = 2:             Ho x Wo = ((H-1)/2+1) x ((W-1)/2+1);      otherwise Ho x Wo = H x W.
 * ld_in / ld_out: row strides in floats (0 = C), >= C, ld_in % 4 == 0; channels [C, ld_in) of a are read
 * and ignored (padding of an internal buffer: must be finite); they take no part in the range.
 * out = NULL (with r_state set): range-only pass, nothing is stored. */
int cdn_codenet_dw3x3_nhwc_forward(
    const float *a, const void *a_qstate, int64_t N, int64_t C, int64_t H, int64_t W, int up, int stride,
    int64_t ld_in, int64_t ld_out, const float *w, const float *bias, const float *ep_scale,
    const float *ep_shift, int relu, float *r_min, float *r_max, void *r_state, int bits,
    double momentum, int running, void *workspace, size_t workspace_bytes, float *out, void *stream);

/* The tail of a W4A8 detection head (quant_modules.py:1062-1069): depthwise 3x3 on the nearest x2 up-sampled y1
 * (+ folded-BN bias) -> ReLU -> QuantAct -> 1x1 conv C -> classes (+ bias), NCHW output, as ROW-STREAMING kernels
 * (every stored row staged and fake-quantised once), and its range pass; C == 64 (head_conv of every reference
 * configuration):
 *   y1 [N][Hs*Ws][C] pre-quantisation values + y1_qstate;  w_dw [C][9], b_dw [C] or NULL
 *   w_codes / w_scale / w_colsum: integer form of the 1x1 weights ([classes][round_up(C,64)] int8, ...)
 *   out_nchw [N][classes][2Hs][2Ws]
 *   cdn_codenet_head_range_forward       tracks the QuantAct after the depthwise conv (r_min / r_max / r_state)
 *                                        from ReLU(dw3x3(up2(fq(y1))) + b_dw) without storing it;
 *   cdn_codenet_head_tail_small_forward  recomputes those values, quantises them with y2_qstate and applies the
 *                                        1x1 conv on the int8 matrix cores (class groups of 32, up to
 *                                        cdn_codenet_head_tail_max_classes() classes -- 128, which covers COCO's 80;
 *                                        more: CDN_ERR_UNSUPPORTED before any launch; needs w_colsum,
 *                                        Ws % 16 == 0 and a 16-byte aligned output), with a VALU launch behind it
 *                                        for batches whose codes are too wide for int8; other shapes with
 *                                        classes <= 4 run on the VALU form (exact integer dot products).
 *                                        Bit-identical to cdn_codenet_dw3x3_nhwc_forward (up = 1) + the int8
 *                                        pointwise + unpack whenever that path runs on integer codes.
 *   w_codes [classes][64] int8 (16-byte aligned), w_scale / w_colsum / bias [classes] (w_colsum may be NULL for
 *   classes <= 4, bias may be NULL), out_nchw [N][classes][2Hs][2Ws]. */
int cdn_codenet_head_range_forward(const float *y1, const void *y1_qstate, int64_t N, int64_t C, int64_t Hs,
                                   int64_t Ws, const float *w_dw, const float *b_dw, float *r_min, float *r_max,
                                   void *r_state, int bits, double momentum, int running, void *workspace,
                                   size_t workspace_bytes, void *stream);
int cdn_codenet_head_tail_max_classes(void);
int cdn_codenet_head_tail_small_forward(const float *y1, const void *y1_qstate, int64_t N, int64_t C, int64_t Hs,
                                        int64_t Ws, const float *w_dw, const float *b_dw, const void *y2_qstate,
                                        const signed char *w_codes, const float *w_scale, const int *w_colsum,
                                        const float *bias, int64_t classes, float *out_nchw, void *stream);
/* The same tail in the frozen serving mode: y1 holds the BYTE CODES of its QuantAct ([N][Hs*Ws][64] int8, 16-byte
 * aligned; written by cdn_codenet_pointwise_q8_forward) -- a code is decoded to (q + zp) / scale, the value the fp32
 * form's fake-quantisation gives the element that produced the code, so the outputs are those of
 * cdn_codenet_head_tail_small_forward on the pre-quantisation tensor, bit for bit, at a quarter of the read traffic.
 * No range pass has measured this batch (y2_qstate word [6] is 0 after cdn_quantact_frozen_params): a y2 level outside
 * the int8 kernels' nibble split (|level - 128| > 2040, a value 8 ranges outside the frozen range) sets *overflow. */
int cdn_codenet_head_tail_small_q8_forward(const signed char *y1_codes, const void *y1_qstate, int64_t N, int64_t C,
                                           int64_t Hs, int64_t Ws, const float *w_dw, const float *b_dw,
                                           const void *y2_qstate, const signed char *w_codes, const float *w_scale,
                                           const int *w_colsum, const float *bias, int64_t classes, float *out_nchw,
                                           unsigned *overflow, void *stream);
/* The two tails with the width of w_codes stated by the caller (see CDN_W_CODES_8BIT): w_bits = 4 is exactly the entry
 * without the argument (|q| <= 8), w_bits = 8 admits any int8 code; other values: CDN_ERR_ARG.  Same results as the
 * unfused schedule on the same codes, bit for bit. */
int cdn_codenet_head_tail_small_w_forward(const float *y1, const void *y1_qstate, int64_t N, int64_t C, int64_t Hs,
                                          int64_t Ws, const float *w_dw, const float *b_dw, const void *y2_qstate,
                                          const signed char *w_codes, const float *w_scale, const int *w_colsum,
                                          const float *bias, int64_t classes, float *out_nchw, int w_bits,
                                          void *stream);
int cdn_codenet_head_tail_small_q8_w_forward(const signed char *y1_codes, const void *y1_qstate, int64_t N, int64_t C,
                                             int64_t Hs, int64_t Ws, const float *w_dw, const float *b_dw,
                                             const void *y2_qstate, const signed char *w_codes, const float *w_scale,
                                             const int *w_colsum, const float *bias, int64_t classes, float *out_nchw,
                                             unsigned *overflow, int w_bits, void *stream);

/* ------------------------------------------------------------------------------------------
 * The backbone's remaining layer types (lib/models/networks/
 * shufflenetv2_dcn.py:57-114,205-240; W4A8: QuantBaseNode quant_modules.py:809-907, layer0 / layer4
 * quantize_model.py:26-34,56-60).  A ShuffleNetV2 unit is pointwise -> depthwise 3x3 -> pointwise on
 * one half of the channels (cdn_codenet_pointwise_nhwc_forward with row strides,
 * cdn_codenet_dw3x3_nhwc_forward) followed by concat + channel_shuffle(2), which is
 *   dst[m][2i] = fq_A(srcA[m][i]),  dst[m][2i+1] = fq_B(srcB[m][i]),  i < h
 * with the block-output QuantAct applied (qA / qB: QuantAct state, NULL = copy).  Either source may be
 * NULL: its slots stay untouched (the two branches of a stride-2 unit are quantised with different
 * states of the layer's shared QuantAct, so each is written right after its own range update).
 * ---------------------------------------------------------------------------------------- */
int cdn_codenet_interleave_forward(const float *srcA, int64_t ldA, const void *qA, const float *srcB,
                                   int64_t ldB, const void *qB, int64_t M, int64_t h, float *dst,
                                   int64_t ld_dst, void *stream);

/* layer0: dense 3x3 conv 3 -> Co (Co = 24), pad 1, on the NCHW image img [N][3][H][W]; w [Co][27]
 * (BN folded, fake-quantised for W4A8), bias [Co] or NULL; out [N][Ho*Wo][Co] channels-last,
 * Ho = (H + 2 - 3) / stride + 1.  Range tracking of the following QuantAct as above. */
int cdn_codenet_stem_forward(const float *img, int64_t N, int64_t H, int64_t W, int64_t Co, int stride,
                             const float *w, const float *bias, int relu, float *r_min, float *r_max,
                             void *r_state, int bits, double momentum, int running, void *workspace,
                             size_t workspace_bytes, float *out, void *stream);

/* MaxPool2d(3, stride 2, padding 1) of the "S2 + MaxPool" stems (shufflenetv2_dcn.py:209-214; configs b / e),
 * channels-last: out[n][oy*Wo+ox][c] = max over the window of fq(a[n][y*W+x][c]) (a_qstate NULL: no
 * quantiser); Ho = (H-1)/2+1.  C % 4 == 0. */
int cdn_codenet_maxpool3x3s2_nhwc_forward(const float *a, const void *a_qstate, int64_t N, int64_t C,
                                          int64_t H, int64_t W, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * ctdet_decode (lib/models/decode.py:474-505 with _nms :10-16 and _topk :110-127; SURVEY.md section
 * 8f row 2): 3x3 peak filter, top-K over all classes, reg / wh gather, boxes.
 *   heat [B][cat][H][W]  scores (after sigmoid), or logits with apply_sigmoid != 0
 *   wh   [B][2][H][W]    (cat_spec_wh != 0: [B][2*cat][H][W]);  reg [B][2][H][W] or NULL (-> +0.5)
 *   heat_out  NULL, or [B][cat][H][W] receiving the (sigmoid of the) input.  heat_out == heat is
 *             allowed (the in-place sigmoid_ of lib/detectors/ctdet.py:32; with a sigmoid on planes that
 *             are cut into row bands it is stored by a second kernel behind the key pass, because a
 *             band's halo rows belong to its neighbours); a partial overlap is CDN_ERR_ARG
 *   dets [B][K][6] = x1, y1, x2, y2, score, class;  K <= 1024
 * Equal scores are ordered by ascending index class*H*W + y*W + x (torch.topk leaves it unspecified).
 * workspace: cdn_ctdet_decode_workspace_bytes(B,cat,H,W) bytes, 256-byte aligned; its LAST
 * round_up(B*8256, 256) bytes are per-image histograms and list counters: zero them once, every call leaves them zero.
 * ---------------------------------------------------------------------------------------- */
size_t cdn_ctdet_decode_workspace_bytes(int64_t B, int64_t cat, int64_t H, int64_t W);
int cdn_ctdet_decode(const float *heat, const float *wh, const float *reg, int64_t B, int64_t cat,
                     int64_t H, int64_t W, int cat_spec_wh, int K, int apply_sigmoid, float *heat_out,
                     float *dets, void *workspace, size_t workspace_bytes, void *stream);
/* Test-time flip augmentation in front of cdn_ctdet_decode (lib/detectors/ctdet.py:32-38, opt.flip_test: every test
 * command of the reference's README): hm [2P][cat][H][W] logits and wh [2P][wh_ch][H][W] of P images (0 .. P-1) and
 * their W-mirrors (P .. 2P-1; P = 1 is the reference's layout) ->
 *   hm <- sigmoid(hm) IN PLACE (the reference's hm.sigmoid_() on the whole batch),
 *   hm_out [P][cat][H][W] = (hm[p] + flip_W(hm[P + p])) / 2,   wh_out = (wh[p] + flip_W(wh[P + p])) / 2
 * (decode then takes hm_out without a sigmoid and reg[0 .. P-1]).  hm_out / wh_out must not overlap the inputs nor each
 * other (CDN_ERR_ARG). */
int cdn_ctdet_flip_merge(float *hm, const float *wh, int64_t P, int64_t cat, int64_t wh_ch, int64_t H, int64_t W,
                         float *hm_out, float *wh_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-scale test / --nms (test.py --test_scales a,b,c / --nms): what CtdetDetector.run does behind ctdet_decode --
 * post_process (lib/detectors/ctdet.py:48-57, lib/utils/post_process.py:86-103), the per-class merge across scales,
 * soft_nms (lib/models/external/nms.pyx:77-170) and the max_per_image cut (ctdet.py:59-74).
 *
 * soft_nms, all three methods (0 hard, 1 linear, 2 gaussian), with the arithmetic widths of the C code Cython makes
 * of nms.pyx (every `+ 1` is a DOUBLE addition, products of box sides are double, the gaussian calls the double exp;
 * the table is in codenet_merge.hip and DESIGN.md).  Argmax with strict <: the lowest index wins among equal scores.
 * REFERENCE-FAITHFUL TAIL: the reference discards a row by overwriting it with row N-1 and decrementing N; the slot
 * beyond the new N is not cleared, and merge_outputs ignores the returned `keep`, so the stale rows [N, n) stay in
 * the per-class arrays and take part in the max_per_image cut.  Both entry points reproduce the whole array the
 * reference leaves: a row that was pulled leaves its old slot with its pre-decay score, a row discarded in place
 * (position == N-1) keeps its decayed score.
 *
 * cdn_soft_nms_host: on the CPU, no HIP call; boxes [n][5] = x1, y1, x2, y2, score, HOST memory, in place;
 *   *n_keep (may be NULL) = the final N = len(keep).  method outside 0..2, sigma == 0 with method 2: CDN_ERR_ARG.
 *
 * cdn_ctdet_merge_scales: one launch, one workgroup per image, capturable.
 *   dets [B][S][K][6]   as cdn_ctdet_decode writes them for the S test scales of B images (output-map pixels)
 *   meta [B][S][6]      DEVICE doubles {c_x, c_y, s, out_w, out_h, scale}: the crop of pre_process and the test scale
 *   per image:  1. x = float32((p - out_w/2) * (s/out_w) + c_x) / float32(scale)   (y with out_h/2 and c_y; double
 *                  inside, then a float32 division: evalio.transform_preds / post_process)
 *               2. STABLE partition by class: inside a class rows are ordered by scale, then decode rank (the order
 *                  np.concatenate gives the reference; it decides ties and the tail layout).  Rows whose class is
 *                  not an integer in [0, num_classes) are dropped, as on the host.
 *               3. do_nms != 0: soft_nms(sigma, Nt, threshold, method) per class
 *               4. more than max_per_image rows (tails included): thresh = the max_per_image-th largest score of
 *                  all rows, rows with score >= thresh survive in order (ties may keep more, as np.partition does)
 *   boxes    [B][num_classes][S*K][5]  the surviving rows of every class, compacted to the front (the rest of a
 *                                      class's S*K slots is not written)
 *   rows_out, rows_in, live  int32 [B][num_classes]: surviving rows, rows of the class before soft-NMS, the
 *                                      soft-NMS N (= rows_in without do_nms)
 *   thresh   [B]                       the cut's threshold, -inf when the image had at most max_per_image rows
 * Capacity: S*K <= 4096 rows per image, K <= 1024, num_classes <= 256 (CDN_ERR_UNSUPPORTED beyond).  LDS per
 * workgroup: 20 B per row (the class lists: every row is in at most one) + 4 B per row (pre-decay scores) + 16 waves x
 * 64 ballot words of 8 B = 24 * S*K + 8192 bytes, 106496 of the 160 KiB at capacity.
 * The kernel needs no global scratch.  cdn_ctdet_merge_scales_workspace_bytes is the size of ONE block that holds
 * the five results back to back, each section rounded up to 256 bytes, in the order boxes, rows_out, rows_in, live,
 * thresh: a caller that carves the result pointers out of such a block fetches everything with one copy.
 * Argument errors are returned before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int cdn_soft_nms_host(float *boxes, int64_t n, float sigma, float Nt, float threshold, int method, int64_t *n_keep);
size_t cdn_ctdet_merge_scales_workspace_bytes(int64_t B, int64_t S, int64_t K, int64_t num_classes);
int cdn_ctdet_merge_scales(const float *dets, const double *meta, int64_t B, int64_t S, int64_t K, int64_t num_classes,
                           int max_per_image, int do_nms, float sigma, float Nt, float threshold, int method,
                           float *boxes, int32_t *rows_out, int32_t *rows_in, int32_t *live, float *thresh,
                           void *stream);

/* ------------------------------------------------------------------------------------------
 * Image pre-processing: CtdetDetector.pre_process for every test scale of an image
 * (lib/detectors/base_detector.py:47-77, fix_res) and the input crop of the training sample
 * (lib/datasets/sample/ctdet.py:84-97) -- resize, affine crop with a zero border, optional source flip,
 * (v / 255 - mean) / std, HWC uint8 -> float32 planes, the W-mirrors of --flip_test.  codenet_preproc.hip; Python:
 * codenet_amd/preproc.py.  The arithmetic is an INTEGER specification of this project (DESIGN.md section 7.4b;
 * tests/preproc_ref.py restates it in numpy and the kernel equals it bit for bit); it has the form of cv2.resize +
 * cv2.warpAffine(INTER_LINEAR) on uint8 but makes no claim about cv2's own bits.
 *
 * cdn_ctdet_pre_process: one launch, capturable; the launch geometry depends on P, out_h, out_w and mirror only.
 *   src_arena  DEVICE bytes that hold the source images: uint8, HWC, 3 channels, row pitch >= 3 w
 *   items      DEVICE doubles [P][16] (integers are exact in a double, as in the meta of cdn_ctdet_merge_scales):
 *                {src_off, h, w, pitch, new_h, new_w, ratio_y, ratio_x, flip_src, M0, M1, M2, M3, M4, M5, 0}
 *              src_off / pitch in bytes; new_h x new_w the size after the resize (equal to h x w: no resize), ratio =
 *              n_src / n_dst per axis, computed in double by the host; M maps output (x, y) to a position in the RESIZED
 *              image: (M0 x + M1 y + M2, M3 x + M4 y + M5); flip_src != 0 reads the resized image W-mirrored.
 *              The kernel trusts the table: the caller keeps every item inside the arena and |M . corner| < 2^20.
 *   lut        DEVICE float32 [256][3]: lut[v][c] = float32((v / 255.0 - mean[c]) / std[c]) evaluated in double
 *   out        float32 [P][3][out_h][out_w]; mirror != 0: [2P][3][out_h][out_w] and plane set P + i is the exact
 *              W-mirror of plane set i (the reference's images[:, :, :, ::-1])
 * A resized image with new_h == 0 or new_w == 0 has no pixel: the whole crop is border, lut[0].
 * P <= 65535, out_h * out_w < 2^31 (CDN_ERR_UNSUPPORTED beyond).  Argument errors are returned before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int cdn_ctdet_pre_process(const unsigned char *src_arena, const double *items, int64_t P, const float *lut, float *out,
                          int64_t out_h, int64_t out_w, int mirror, void *stream);

/* ------------------------------------------------------------------------------------------
 * The default training sample's input: the crop above followed by color_aug (lib/datasets/sample/ctdet.py:76-79 with
 * lib/utils/image.py:196-234): v / 255, brightness / contrast / saturation in a shuffled order, lighting,
 * (x - mean) / std.  The arithmetic is DESIGN.md section 7.4c (tests/color_aug_ref.py restates it; the kernels equal it
 * bit for bit): float32, every operation rounded once, no contraction; the contrast step's whole-crop grey mean comes
 * from EXACT integer channel sums, gs_mean = float32(((0.114 S0 + 0.587 S1) + 0.299 S2) / (255.0 N)) in double.
 *
 * cdn_ctdet_pre_process_aug: three launches on `stream` -- zero_sums_kernel clears `sums`, then crop_sum_kernel and
 * color_aug_kernel; capturable (the clearing is a kernel node of the graph: the runtime's memset node is avoided,
 * DESIGN.md section 7.4c); the launch geometry depends on P, out_h and out_w only.
 *   src_arena, items   as cdn_ctdet_pre_process
 *   aug        DEVICE [P][16] 4-byte words per item: int32 on, int32 order[3] (a permutation of 0 brightness, 1 contrast,
 *              2 saturation), float32 a[3] = float32(alpha_k), float32 om[3] = float32(1 - alpha_k), float32 d[3] (the
 *              lighting term per channel position), 3 unused.  on == 0 (validation split, --no_color_aug): the item is
 *              ((float32(v) / 255f) - mean) / std, the float32 chain of the reference's sample.  The host checks the rows.
 *   mean_std   DEVICE float32 [6]: mean[3], std[3], by channel position
 *   crop_u8    DEVICE scratch, P * 3 * out_h * out_w bytes: the crops as planes, crop_u8[item][c][y][x]
 *   sums       DEVICE uint64 [P][3]: on return (in stream order) S_c = the sum of channel c over all out_h * out_w
 *              pixels of the item's crop, border included.  Integer atomic adds: any order gives the same bits.
 *   out        float32 [P][3][out_h][out_w]
 * P <= 65535, out_h * out_w < 2^31 (CDN_ERR_UNSUPPORTED beyond); null pointers: CDN_ERR_ARG, before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int cdn_ctdet_pre_process_aug(const unsigned char *src_arena, const double *items, int64_t P, const float *aug,
                              const float *mean_std, unsigned char *crop_u8, unsigned long long *sums, float *out,
                              int64_t out_h, int64_t out_w, void *stream);

/* ------------------------------------------------------------------------------------------
 * Baseline JPEG decoding in front of the pre-processing: file bytes -> interleaved uint8 pixels with the bits of
 * libjpeg-turbo's default decode (ISLOW IDCT, fancy up-sampling, 16-bit fixed-point YCbCr -> RGB: what cv2.imread and PIL
 * give; EXIF orientation is ignored, as PIL does).  codenet_jpeg.hip + cdn_jpeg.h; Python: codenet_amd/jpeg.py.  The
 * arithmetic is DESIGN.md section 7.4d (tests/jpeg_ref.py restates it in numpy; both equal PIL bit for bit).
 * Supported: SOF0, 8-bit samples and quantisation tables, one interleaved scan, 1 or 3 components, every component 1x1
 * or Y 2x1 / 2x2 with 1x1 chroma, restart intervals.  Everything else (progressive, arithmetic, 12-bit, 16-bit tables,
 * CMYK, 4:4:0, 4:1:1, several scans, DNL, RGB-coded) is CDN_ERR_UNSUPPORTED from the two host functions.
 *
 * Records (int32, little-endian, written by cdn_jpeg_pack):
 *   item [16]    {w, h, components, mode (0 all 1x1, 1 Y 2x1, 2 Y 2x2), mcus_x, mcus_y, table selectors, Y pitch, Y rows,
 *                 C pitch, C rows, restart interval, output offset low / high word, output pitch, 0}
 *   segment [8]  {item, first MCU, MCU count, byte offset into the stream buffer, byte length, 0, 0, 0}; record 0 of the
 *                segment buffer is the header {segments used, items used, 0...}, the segments follow it
 *   tables       6144 bytes per item: 3 x 64 quantisation bytes per COMPONENT in natural order, then the decode form of
 *                the Huffman tables DC 0, DC 1, AC 0, AC 1 (struct cdn_jpeg::Tables)
 *
 * cdn_jpeg_parse (host, no HIP call): info[16] = {w, h, components, mode, mcus_x, mcus_y, restart interval, segments,
 *   offset of the entropy-coded data, 0...}.  Malformed data: CDN_ERR_ARG.
 * cdn_jpeg_pack (host, no HIP call): parses `data` again and, in one pass over its entropy-coded bytes, removes the
 *   stuffed 00 after every FF and cuts the bytes at RSTn / EOI into segments; writes the bytes at stream + stream_used,
 *   the records behind the segs_used segments already there, the item record and the table blob of item `item` (the
 *   caller passes the addresses of that item's slots) and the header record; used[0] / used[1] = the new byte / segment
 *   counts.  A missing EOI ends the last segment at the end of the data.  CDN_ERR_WORKSPACE when a capacity (stream
 *   bytes, segments, plane_stride for the image's padded planes) is too small: detected before anything is written.
 * cdn_jpeg_workspace_bytes: the planes of max_items images of at most max_h x max_w; per item
 *   plane_stride = cdn_jpeg_workspace_bytes(1, max_h, max_w) bytes.  0: a size outside 1..65535.
 * cdn_jpeg_decode: two launches on `stream`, capturable -- jpeg_entropy_idct_kernel (segments -> uint8 component planes,
 *   padded to whole MCUs) and jpeg_color_kernel (planes -> out + offset + y pitch + 3 x, B G R, or R G B with rgb != 0).
 *   Every pointer is DEVICE memory.  The launch geometry follows from seg_cap, item_cap and plane_stride alone and the
 *   counts are read from the header record, so a captured call replays for any batch inside the capacities.  The kernels
 *   check every record against stream_cap / seg_cap / item_cap / plane_stride / out_cap before they store.
 *   status [item_cap] int32, zeroed by the caller: per item the maximum of 0 ok, 1 bits were consumed beyond the end of a
 *   segment, 2 a code with no entry in its Huffman table, 3 a record outside the capacities (integer atomicMax: the order
 *   cannot change the bits).  The pixels of an item with a non-zero status are unspecified.
 *   Concurrency: a segment is decoded by ONE lane; the entropy kernel scales with batch size x restart intervals.
 * cdn_jpeg_decode_host: the same call with HOST pointers; runs the same decoder text on the calling thread, no HIP call.
 * Argument errors are returned before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int cdn_jpeg_parse(const unsigned char *data, int64_t n, int32_t *info);
int cdn_jpeg_pack(const unsigned char *data, int64_t n, int32_t item, int64_t out_off, int64_t out_pitch,
                  unsigned char *stream_bytes, int64_t stream_used, int64_t stream_cap, int32_t *segs, int64_t segs_used,
                  int64_t seg_cap, int32_t *item_rec, unsigned char *tables, int64_t plane_stride, int64_t *used);
size_t cdn_jpeg_workspace_bytes(int64_t max_items, int64_t max_h, int64_t max_w);
int cdn_jpeg_decode(const unsigned char *stream_bytes, int64_t stream_cap, const int32_t *segs, int64_t seg_cap,
                    const int32_t *items, int64_t item_cap, const unsigned char *tables, unsigned char *planes,
                    int64_t plane_stride, int32_t *status, unsigned char *out, int64_t out_cap, int rgb, void *stream);
int cdn_jpeg_decode_host(const unsigned char *stream_bytes, int64_t stream_cap, const int32_t *segs, int64_t seg_cap,
                         const int32_t *items, int64_t item_cap, const unsigned char *tables, unsigned char *planes,
                         int64_t plane_stride, int32_t *status, unsigned char *out, int64_t out_cap, int rgb);

/* The parallel entropy path (opt-in; the five functions above are untouched by it).  The same buffers and records, the
 * same pixels and the same zero / non-zero status as cdn_jpeg_decode, but a segment is decoded by the 256 lanes of a
 * workgroup: its bits (the host removed the stuffing) are cut into sub-sequences of subseq_bits, every lane decodes one
 * from a guessed state, and counted rounds hand the exact state from lane to lane.  Files
 * without restart markers no longer decode as one chain per image.
 * cdn_jpeg_parallel_workspace_bytes: the raw coefficients (int16 x 64 per 8 x 8 block) and DC words (int32 per block) of
 *   max_items images: 2.0625 x the plane bytes -- 6.19 MiB per item for the 1024 x 1024 default, 1.16 MiB for 375 x 500.
 *   0: a size outside 1..65535.
 * cdn_jpeg_decode_parallel: three launches on `stream`, capturable -- jpeg_entropy_parallel_kernel (segments -> workspace),
 *   jpeg_idct_kernel (workspace -> planes) and jpeg_color_kernel.  workspace: DEVICE memory, 16-byte aligned, at least
 *   cdn_jpeg_parallel_workspace_bytes(item_cap, ...) for the plane_stride given; subseq_bits: a multiple of 32 in
 *   64..8192; anything else is CDN_ERR_ARG.
 *   status: 0 exactly when cdn_jpeg_decode gives 0; otherwise 2 when the exact chain met a code with no table entry
 *   inside the segment's real bits, 1 when the real bits ran out before the segment's blocks were complete, 3 as above
 *   (and for a segment of more than 2^28 - 2^19 bytes: bit positions are 32-bit).
 * cdn_jpeg_decode_parallel_host: the same call with HOST pointers, the same text on the calling thread. */
size_t cdn_jpeg_parallel_workspace_bytes(int64_t max_items, int64_t max_h, int64_t max_w);
int cdn_jpeg_decode_parallel(const unsigned char *stream_bytes, int64_t stream_cap, const int32_t *segs, int64_t seg_cap,
                             const int32_t *items, int64_t item_cap, const unsigned char *tables, unsigned char *planes,
                             int64_t plane_stride, int32_t *status, unsigned char *out, int64_t out_cap, int rgb,
                             unsigned char *workspace, size_t workspace_bytes, int subseq_bits, void *stream);
int cdn_jpeg_decode_parallel_host(const unsigned char *stream_bytes, int64_t stream_cap, const int32_t *segs, int64_t seg_cap,
                                  const int32_t *items, int64_t item_cap, const unsigned char *tables, unsigned char *planes,
                                  int64_t plane_stride, int32_t *status, unsigned char *out, int64_t out_cap, int rgb,
                                  unsigned char *workspace, size_t workspace_bytes, int subseq_bits);

/* ------------------------------------------------------------------------------------------
 * The ctdet training criterion (main.py / quant_main.py: ModelWithLoss -> CtdetLoss, lib/trains/ctdet.py:17-74) and
 * the target maps it is fed (lib/datasets/sample/ctdet.py:87-122).  codenet_loss.hip; Python: codenet_amd/losses.py.
 *
 * Covered: FocalLoss on hm behind _sigmoid (lib/models/losses.py:42-67, models/utils.py:9-11), RegL1Loss
 * (reg_loss 0, --reg_loss l1) or RegLoss (reg_loss 1, sl1) on wh and reg (losses.py:100-155), num_stacks >= 1.
 * wh == NULL / reg == NULL switch that term off (opt.wh_weight == 0; not opt.reg_offset or opt.off_weight == 0).
 * Not covered (the Python mirror composes them from PyTorch): mse_loss, dense_wh, norm_wh, cat_spec_wh, eval_oracle_*.
 *
 *   hm [N][C][H][W] logits, hm_gt the same shape;  wh, reg [N][2][H][W];  wh_gt, reg_gt [N][M][2];
 *   ind [N][M] int64 cells y * W + x;  reg_mask [N][M] uint8.   All contiguous float32 unless said otherwise.
 * Per element, float32 in the reference's operation order: p = clamp(sigmoid(x), 1e-4, 1 - 1e-4);
 *   gt == 1: log(p) (1-p)^2 and num_pos += 1;   gt < 1: log(1-p) p^2 (1-gt)^4;
 *   per (row, channel): |pred m - target m| (l1) or its smooth-L1 form, pred = head[b][c][ind[b][k]], m = reg_mask.
 * SUMS: per thread in double, a fixed tree per wave and workgroup, one slab of partials per workgroup, added in index
 * order by a one-workgroup finish: no floating-point atomics, so a call is a pure function of its inputs bit for bit.
 * The finish rounds the sums to float32 and applies the reference's scalar arithmetic: `- neg` when num_pos == 0, else
 * `- (pos + neg) / num_pos`; RegL1Loss divides by the sum of the EXPANDED mask + 1e-4 (2 x the row sum), RegLoss by
 * the row sum + 1e-4; every term `/ num_stacks`; loss = hm_weight hm + wh_weight wh + off_weight off.
 * A cell outside [0, H*W) is never dereferenced: forward turns the term NaN, backward skips the row.
 *
 * cdn_ctdet_loss_forward: call once per stack (stack = 0 .. num_stacks-1, the same targets and workspace); the call
 *   with stack == num_stacks-1 also runs the finish.  Two launches at most, no host synchronisation, capturable.
 *   hm_sigmoid  NULL, or [N][C][H][W]: receives p (what the reference leaves in output['hm'])
 *   result      8 floats: loss, hm_loss, wh_loss, off_loss, then what backward reads -- the hm denominator (num_pos,
 *               or 1), the regression denominator, num_pos, the mask's row sum
 *   workspace   cdn_ctdet_loss_workspace_bytes(...) bytes, 256-byte aligned, every word written before it is read
 * cdn_ctdet_loss_backward: one launch per stack.  grad_result: 4 device floats, the gradient of (loss, hm_loss,
 *   wh_loss, off_loss).  grad_hm is RECOMPUTED from logits and target (zero where the sigmoid is outside the clamp):
 *   2 maps read + 1 written, the same traffic as reading a stored unscaled gradient and without its buffer.
 *   grad_wh / grad_reg (NULL: not wanted) are dense [N][2][H][W]: the kernel clears them and writes the object cells;
 *   rows that share a cell are added in row order by the first of them.
 *
 * cdn_ctdet_targets: one launch, one workgroup per (image, class) plane, no memset, no atomics.
 *   boxes [N][M][4] x1, y1, x2, y2 in OUTPUT-map pixels after the affine map and the clip to [0, W-1] x [0, H-1];
 *   classes [N][M] int32; counts [N] int32 rows in use (clamped to [0, M]).
 *   A row takes part when h = y2 - y1 > 0 and w = x2 - x1 > 0 (float32) and 0 <= class < C:
 *     radius = max(0, int(gaussian_radius(ceil(h), ceil(w)))) in double (lib/utils/image.py:90-110), sigma =
 *     (2 r + 1) / 6, ct = ((x1 + x2) / 2, (y1 + y2) / 2) in float32, ct_int by truncation;
 *     hm[b][class] = max(hm, float32(exp(-(dx^2 + dy^2) / (2 sigma^2)))) over the window |dx|, |dy| <= r, double exp;
 *     wh = (w, h), reg = ct - ct_int, ind = ct_int.y * W + ct_int.x, reg_mask = 1.
 *   Every other row, and every row at or beyond counts[b], is zero in wh, reg, ind and reg_mask.  M <= 2048.
 * Argument errors are returned before any HIP call.
 * ---------------------------------------------------------------------------------------- */
size_t cdn_ctdet_loss_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int64_t M, int num_stacks);
int cdn_ctdet_loss_forward(const float *hm, const float *wh, const float *reg, const float *hm_gt, const float *wh_gt,
                           const float *reg_gt, const int64_t *ind, const uint8_t *reg_mask, int64_t N, int64_t C,
                           int64_t H, int64_t W, int64_t M, int stack, int num_stacks, int reg_loss, float hm_weight,
                           float wh_weight, float off_weight, float *hm_sigmoid, float *result, void *workspace,
                           size_t workspace_bytes, void *stream);
int cdn_ctdet_loss_backward(const float *hm, const float *wh, const float *reg, const float *hm_gt, const float *wh_gt,
                            const float *reg_gt, const int64_t *ind, const uint8_t *reg_mask, int64_t N, int64_t C,
                            int64_t H, int64_t W, int64_t M, int num_stacks, int reg_loss, float hm_weight,
                            float wh_weight, float off_weight, const float *result, const float *grad_result,
                            float *grad_hm, float *grad_wh, float *grad_reg, void *stream);
int cdn_ctdet_targets(const float *boxes, const int32_t *classes, const int32_t *counts, int64_t N, int64_t M, int64_t C,
                      int64_t H, int64_t W, float *hm, float *wh, float *reg, int64_t *ind, uint8_t *reg_mask,
                      void *stream);

/* ------------------------------------------------------------------------------------------
 * The quantised detection heads in the QAT step (QuantDepthwiseNode, quant_modules.py:1013-1071), per head:
 *   y1 = conv1x1(x, W1q) + b1,  a1 = fq1(relu(y1)),  r2 = relu(dw3x3(a1, W2q, zero padding) + b2),  y3 = conv1x1(fq3(r2), W3q) + b3
 * NCHW fp32.  The dense 1x1 convolutions and their gradients are cdn_codenet_pointwise_forward[_range] /
 * cdn_codenet_pointwise_wgrad[_q]; these are the pieces in between.  Every call takes a stream, allocates nothing, launches
 * no memset node and is capturable; every floating-point sum has one order (no float atomics).
 *
 * cdn_codenet_head_act_update: the QuantAct update (range tracking when running != 0, then scale / zero point) from the
 *   {min, max} pairs a producer left (`partials`, float2 [n_partials]; ignored with running == 0); relu != 0: the extremes
 *   are those of max(x, 0).  state_copy (8 words, may be NULL) receives the snapshot a backward pass reads.  One launch.
 * cdn_codenet_head_dw_forward: r2 [N][C][H][W] from y1, with a1 formed while loading (a1_state: the 8-word state or
 *   snapshot of the QuantAct behind y1); taps outside the plane are 0.0f.  r2 is stored BEFORE quantisation.  running != 0:
 *   the launch's last workgroup updates the QuantAct behind r2 (x_min, x_max, state, counters =
 *   cdn_quantact_arrive_words() zero words, left zero) from the extremes of r2 and writes state_copy (may be NULL);
 *   running == 0: the QuantAct arguments are not read.
 * cdn_codenet_head_tail_train_forward: y3 [N][Co][HW] = W3q [Co][C] . fq(r2) + b3 (may be NULL) for 1 <= Co <= 4
 *   (CDN_ERR_UNSUPPORTED beyond), a2_state: the state of the QuantAct behind r2.
 * cdn_codenet_head_dw_backward:
 *   Co == 0: g = grad_a2 [N][C][H][W];   1 <= Co <= 4: g = grad_y3 [N][Co][H][W] and w3 = W3q [Co][C] -- the kernel
 *            forms grad_a2[c] = sum_o W3q[o][c] grad_y3[o] itself (o ascending) and never stores it
 *   grad_y2 = grad_a2 where r2 > 0;  grad_y1 = (sum_t W2q[c][t] grad_y2[q - t]) where y1 > 0 -- a gather;
 *   grad_y1 is written at grad_y1 + n * grad_y1_image_pitch + c * H * W (elements): a channel slice of a wider buffer
 *   grad_w2 [C][9], grad_b2 [C] (either may be NULL): OVERWRITTEN; per-workgroup partials in `workspace`
 *   (cdn_codenet_head_dw_backward_workspace_bytes, 16-byte aligned, every word written before it is read) summed in index
 *   order by a second launch.
 * 16-byte loads where W % 4 == 0 and the pointers (and the pitch) are 16-byte aligned, scalar loads otherwise.
 * N * C * H * W < 2^31 (CDN_ERR_UNSUPPORTED beyond).  Argument errors are returned before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int cdn_codenet_head_act_update(float *x_min, float *x_max, void *state, const float *partials, int64_t n_partials,
                                int bits, double momentum, int running, int relu, void *state_copy, void *stream);
int cdn_codenet_head_dw_forward(const float *y1, const void *a1_state, const float *w2, const float *b2, float *r2,
                                int64_t N, int64_t C, int64_t H, int64_t W, float *x_min, float *x_max, void *state,
                                void *counters, int bits, double momentum, int running, void *state_copy, void *stream);
int cdn_codenet_head_tail_train_forward(const float *r2, const void *a2_state, const float *w3, const float *b3, float *y3,
                                        int64_t N, int64_t C, int64_t Co, int64_t HW, void *stream);
size_t cdn_codenet_head_dw_backward_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W);
int cdn_codenet_head_dw_backward(const float *g, const float *w3, int64_t Co, const float *r2, const float *y1,
                                 const void *a1_state, const float *w2, float *grad_y1, int64_t grad_y1_image_pitch,
                                 float *grad_w2, float *grad_b2, int64_t N, int64_t C, int64_t H, int64_t W,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * The quantised ShuffleNetV2 units in the QAT step (QuantBaseNode, quant_modules.py:809-907; layers 1-3), per unit:
 *   stride 1:  x1 = x[:, :h] (unchanged)                      x2 = x[:, h:]
 *   stride 2:  x1 = act(relu(pw5(act4(dw4_s2(x)))))           x2 = x
 *   both:      x2' = act(relu(pw3(act2(dw2_s(act1(relu(pw1(x2))))))))     out[:, 2j] = x1[:, j],  out[:, 2j+1] = x2'[:, j]
 * NCHW fp32.  `act` is the ONE QuantAct a layer's units share.  The dense 1x1 convolutions and their gradients are the
 * pointwise entries (the *_pitched ones where an operand is a channel slice); these are the pieces in between.  Every
 * call takes a stream, allocates nothing, launches no memset node and is capturable; every floating-point sum has one
 * order (no float atomics).  An "image pitch" is the distance in elements between two images of a tensor: a channel slice
 * x[:, a:b] of [N][Cx][H][W] is (x + a * H * W, pitch Cx * H * W) and is read / written in place.
 *
 * cdn_codenet_pointwise_forward_pitched (replaces :602-604 / :599-600 on a slice, and the data gradient of pw1):
 *   cdn_codenet_pointwise_forward_range (no affine epilogue) with image pitches for d and y; d_state and partials may be
 *   NULL; partials holds cdn_codenet_pointwise_range_partials(N, Co, HW) pairs.  f32 MFMA, the bits of the unpitched call.
 * cdn_codenet_pointwise_wgrad_pitched: cdn_codenet_pointwise_wgrad with an image pitch for d; the same workspace.
 * cdn_codenet_unit_dw_forward (replaces quant_convbn2 / quant_convbn4 + the QuantAct behind them, :599, :603):
 *   out [N][C][Ho][Wo] = dw3x3(a, w [C][9], stride 1 or 2, zero padding 1) + b (may be NULL), Ho = (H - 1) / stride + 1,
 *   the RAW output (no ReLU), stored BEFORE quantisation.  in_state != NULL: a = fq(relu(in)) formed while loading with
 *   that 8-word QuantAct state (snapshot); NULL: in holds final values, read as they are.  running != 0: the launch's last
 *   workgroup updates the QuantAct behind out (x_min, x_max, state, counters = cdn_quantact_arrive_words() zero words,
 *   left zero) from the signed extremes of out and writes state_copy (may be NULL); running == 0: not read.
 *   Sum order of an output: taps in row-major order by fma from zero, then + b.
 * cdn_codenet_unit_dw_backward: g [N][C][Ho][Wo] is the gradient of that raw output (straight-through QuantAct).
 *   grad_in[Y][X] = sum of w[dy][dx] g[yo][xo] over the taps with Y + 1 - dy = stride * yo, X + 1 - dx = stride * xo
 *   (row-major tap order by fma from zero; a gather), masked by in > 0 when in_state != NULL; written at
 *   grad_in + n * grad_in_image_pitch + c * H * W, accumulate != 0: ADDED to what is stored there (by the one thread that
 *   owns the pixel).  grad_in may be NULL.  grad_w [C][9], grad_b [C] (either may be NULL): OVERWRITTEN; per-workgroup
 *   partials in `workspace` (cdn_codenet_unit_dw_backward_workspace_bytes, 16-byte aligned, every word written before it
 *   is read) summed in index order by a second launch.
 *   cdn_codenet_unit_dw_backward_workspace_bytes = round_up_256(C * chunks * 10 * 4), chunks = ceil(items / 256),
 *   items = N * ceil(Ho / rows) * ceil(Wo / 4), rows = 8 where Ho >= 32 else 4.
 * cdn_codenet_unit_join_forward (replaces the shared QuantAct's fake-quantisation + cat + channel_shuffle, :600 / :604-605):
 *   out [N][2h][HW]: out[:, 2j + slot] = fq(relu(y3 [N][h][HW])) with act_state (the shared QuantAct's state AFTER the
 *   update for this branch); x1 != NULL (slot 1 only): out[:, 2j] = x1[:, j] read at x1 + n * x1_image_pitch + j * HW.
 * cdn_codenet_unit_join_backward: grad_y3 = grad_out[:, 2j + slot] where y3 > 0; grad_x1 != NULL (slot 1 only):
 *   grad_x1 + n * pitch + j * HW = grad_out[:, 2j].
 * 16-byte accesses where the widths are multiples of 4 and pointers / pitches 16-byte aligned, scalar ones otherwise.
 * Sizes below 2^31 elements per tensor (CDN_ERR_UNSUPPORTED beyond).  Argument errors are returned before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int cdn_codenet_pointwise_forward_pitched(const float *d, int64_t d_image_pitch, const void *d_state, const float *w_pw,
                                          const float *bias, float *y, int64_t y_image_pitch, int64_t N, int64_t C,
                                          int64_t Co, int64_t HW, int relu, float *partials, void *stream);
int cdn_codenet_pointwise_wgrad_pitched(const float *grad_y, const float *d, int64_t d_image_pitch, float *grad_w,
                                        float *grad_b, int64_t N, int64_t C, int64_t Co, int64_t HW, void *workspace,
                                        size_t workspace_bytes, void *stream);
int cdn_codenet_unit_dw_forward(const float *in, int64_t in_image_pitch, const void *in_state, const float *w,
                                const float *b, float *out, int64_t N, int64_t C, int64_t H, int64_t W, int stride,
                                float *x_min, float *x_max, void *state, void *counters, int bits, double momentum,
                                int running, void *state_copy, void *stream);
size_t cdn_codenet_unit_dw_backward_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W, int stride);
int cdn_codenet_unit_dw_backward(const float *g, const float *in, int64_t in_image_pitch, const void *in_state,
                                 const float *w, float *grad_in, int64_t grad_in_image_pitch, int accumulate,
                                 float *grad_w, float *grad_b, int64_t N, int64_t C, int64_t H, int64_t W, int stride,
                                 void *workspace, size_t workspace_bytes, void *stream);
int cdn_codenet_unit_join_forward(const float *y3, const void *act_state, float *out, int slot, const float *x1,
                                  int64_t x1_image_pitch, int64_t N, int64_t h, int64_t HW, void *stream);
int cdn_codenet_unit_join_backward(const float *grad_out, const float *y3, float *grad_y3, int slot, float *grad_x1,
                                   int64_t grad_x1_image_pitch, int64_t N, int64_t h, int64_t HW, void *stream);

/* ------------------------------------------------------------------------------------------
 * The quantised stem in the QAT step (layer0 after quantisation: QuantBnConv2d(8) 3 -> 24, 3x3, stride 4 or 2, padding 1,
 * then ReLU -> QuantAct [-> MaxPool2d(3, 2, 1)]).  NCHW fp32; the weights come folded and fake-quantised from
 * cdn_codenet_weight_prep_ranked.  Every call takes a stream, allocates nothing, launches no memset node and is capturable;
 * every floating-point sum has one order (no float atomics).  The image takes no gradient.
 *
 * cdn_codenet_stem_train_forward: y0 [N][24][Ho][Wo] = conv3x3(img [N][3][H][W], w [24][27], stride, zero padding 1) + b
 *   (may be NULL), Ho = (H - 1) / stride + 1, the RAW output, stored BEFORE ReLU and quantisation.  Co must be 24, stride 2
 *   or 4.  running != 0: the launch's last workgroup updates the QuantAct behind the stem (x_min, x_max, state, counters =
 *   cdn_quantact_arrive_words() zero words, left zero) from the extremes of max(y0, 0) and writes state_copy (may be NULL);
 *   running == 0: not read.  Sum order of an output: the 27 taps in (ci, dy, dx) order by fma from zero, then + b.
 *   The un-pooled stem's output is cdn_quantact_relu_apply(y0, ..., state_copy).
 * cdn_codenet_stem_pool_forward: out [N][C][Hp][Wp] = fq(relu(max over the 3x3 window, stride 2, padding 1, of
 *   y0 [N][C][H][W])) with act_state, Hp = (H - 1) / 2 + 1: the pool of the quantised values (both maps are monotone).
 * cdn_codenet_stem_pool_backward: grad_y0 [N][C][H][W] from g [N][C][Hp][Wp]: a window's gradient goes to its first maximum
 *   in row-major scan order (val > max || isnan(val)), compared on fq(relu(y0)) with act_state; a pixel adds the windows it
 *   won in row-major window order (a gather, every element written exactly once), masked by y0 > 0.
 * cdn_codenet_stem_backward: grad_b [24] = sum g', grad_w [24][27] = sum g'[n][c][oy][ox] img[n][ci][oy S + dy - 1][ox S +
 *   dx - 1] (zero outside the image), g' = g where y0 > 0 else 0 when y0 != NULL, g' = g when y0 == NULL (g already masked:
 *   the pool backward's output).  Either result may be NULL; both are OVERWRITTEN.  Per-workgroup partials in `workspace`
 *   (16-byte aligned, every word written before it is read) summed in chunk order by a second launch.
 *   cdn_codenet_stem_backward_workspace_bytes = round_up_256(6 * chunks * 112 * 4), chunks = ceil(P / (256 * T)),
 *   P = N * Ho * Wo, T = min(8, max(1, P / 1024)); 0 for arguments the call refuses.
 * Sizes below 2^31 elements per tensor (CDN_ERR_UNSUPPORTED beyond); a workspace that is too small is CDN_ERR_WORKSPACE.
 * Argument errors are returned before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int cdn_codenet_stem_train_forward(const float *img, const float *w, const float *b, float *y0, int64_t N, int64_t H,
                                   int64_t W, int64_t Co, int stride, float *x_min, float *x_max, void *state,
                                   void *counters, int bits, double momentum, int running, void *state_copy, void *stream);
int cdn_codenet_stem_pool_forward(const float *y0, const void *act_state, float *out, int64_t N, int64_t C, int64_t H,
                                  int64_t W, void *stream);
int cdn_codenet_stem_pool_backward(const float *g, const float *y0, const void *act_state, float *grad_y0, int64_t N,
                                   int64_t C, int64_t H, int64_t W, void *stream);
size_t cdn_codenet_stem_backward_workspace_bytes(int64_t N, int64_t H, int64_t W, int stride);
int cdn_codenet_stem_backward(const float *g, const float *y0, const float *img, float *grad_w, float *grad_b, int64_t N,
                              int64_t H, int64_t W, int64_t Co, int stride, void *workspace, size_t workspace_bytes,
                              void *stream);

/* ------------------------------------------------------------------------------------------
 * The block behind every deform stage of the fp32 model under autograd -- BatchNorm2d -> ReLU -> Upsample(x2, nearest)
 * (lib/models/networks/shufflenetv2_dcn.py:303-308) -- forward and backward (codenet_bn_train.hip; DESIGN.md section 4.3e
 * states the arithmetic, every operation rounded on its own, every sum in float64 in one order, no float atomics).
 * y [N][C][H][W] float32 NCHW, 16-byte aligned, n = N H W values per channel; up = 1: out / grad_out are [N][C][H][W], up = 2:
 * [N][C][2H][2W].  mean, var (biased), invstd [C] are outputs of the forward and inputs of the backward.
 * cdn_codenet_bn_workspace_bytes: the workspace of either call (shufflenetv2_dcn.py:303-308): round_up_256(C * slabs * 16)
 *   + round_up_256(C * 8), slabs = ceil(n / 4096); 0 for arguments the calls refuse.
 * cdn_codenet_bn_relu_up_forward (shufflenetv2_dcn.py:303-308): training != 0: mean = f32(S1 / n), var = f32(max(S2 / n -
 *   (S1 / n)^2, 0)) from the float64 sums S1 = sum y, S2 = sum y^2, invstd = 1 / sqrt(var + eps) (float32, correctly
 *   rounded); running_mean = (1 - m) running_mean + m mean, running_var = (1 - m) running_var + m f32(var_d n / (n - 1)) and
 *   *num_batches_tracked += 1 on the device (each may be NULL: not updated; the two running buffers together); n == 1 is
 *   CDN_ERR_ARG.  training == 0: mean = running_mean, var = running_var, nothing is updated, no workspace is needed.
 *   Then out = relu(gamma * ((y - mean) * invstd) + beta), a NaN kept.
 * cdn_codenet_bn_relu_up_backward (shufflenetv2_dcn.py:303-308): g_z [N][C][H][W] = G where z > 0 else 0, z recomputed from
 *   y as in the forward, G = grad_out (up = 1) or ((g00 + g01) + g10) + g11 of its 2x2 block (up = 2); grad_beta = f32(sum
 *   g_z), grad_gamma = f32(sum g_z xh), xh = (y - mean) * invstd (either may be NULL); grad_y = ((g_z - mb) - xh mg) *
 *   (gamma * invstd) with mb = f32(sum g_z / n), mg = f32(sum g_z xh / n) (training != 0) or g_z * (gamma * invstd)
 *   (training == 0).  grad_y may be g_z itself.  Everything is OVERWRITTEN.
 * The workspace is the caller's, 16-byte aligned, every word written before it is read (CDN_ERR_WORKSPACE when too small).
 * Sizes below 2^31 elements per tensor (CDN_ERR_UNSUPPORTED beyond).  Argument errors are returned before any HIP call.
 * ---------------------------------------------------------------------------------------- */
size_t cdn_codenet_bn_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W);
int cdn_codenet_bn_relu_up_forward(const float *y, const float *gamma, const float *beta, float *running_mean,
                                   float *running_var, int64_t *num_batches_tracked, float *mean, float *var, float *invstd,
                                   float *out, int64_t N, int64_t C, int64_t H, int64_t W, int up, int training, double eps,
                                   double momentum, void *workspace, size_t workspace_bytes, void *stream);
int cdn_codenet_bn_relu_up_backward(const float *grad_out, const float *y, const float *gamma, const float *beta,
                                    const float *mean, const float *invstd, float *g_z, float *grad_y, float *grad_gamma,
                                    float *grad_beta, int64_t N, int64_t C, int64_t H, int64_t W, int up, int training,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * The fp32 detection heads under autograd (lib/models/networks/shufflenetv2_dcn.py:246-258): Conv2d 1x1 -> BatchNorm2d ->
 * ReLU -> depthwise Conv2d 3x3 (zero padding 1) -> BatchNorm2d -> ReLU -> Conv2d 1x1 + bias; codenet_heads_fp32_train.hip;
 * DESIGN.md section 4.3f states the arithmetic: every float32 operation rounded on its own, every sum in float64 in one
 * order, no float atomics.  The two dense convolutions of a head and their gradients are cdn_codenet_pointwise_forward /
 * cdn_codenet_pointwise_wgrad, a wide head's stored a2 is cdn_codenet_bn_relu_up_forward with up = 1.  All tensors float32
 * NCHW [N][C][H][W] unless stated, n = N H W values per channel; mean, var (biased), invstd, mb, mg, gamma, beta are [C].
 * Never stored: a1 = relu(bn1(y1)), grad_y2, the unmasked grad_a1 and, for Co <= 4, a2 = relu(bn2(y2)) and grad_a2.
 * cdn_codenet_head_fp32_workspace_bytes: the workspace of every call below: round_up_256(8 * max(C * slabs * 10,
 *   N * C * chunks * 11)), slabs = ceil(n / 4096), chunks = ceil(ceil(W / 4) * ceil(H / 8) / 256); 0 for arguments the calls
 *   refuse.
 * cdn_codenet_head_fp32_bn_stats: the statistics pass of cdn_codenet_bn_relu_up_forward alone (the same kernels): mean, var,
 *   invstd of y and, training != 0, the update of running_mean / running_var / *num_batches_tracked (each may be NULL; n == 1
 *   is CDN_ERR_ARG); training == 0: mean = running_mean, var = running_var, nothing is updated, no workspace is needed.
 * cdn_codenet_head_fp32_dw_forward: y2 = dw3x3(a1, w2 [C][9]) with a1 = relu(gamma1 * ((y1 - mean1) * invstd1) + beta1)
 *   formed on load, 0 outside the plane; y2 = ((0 + w[0] a[0]) + w[1] a[1]) + .. + w[8] a[8], taps row-major.
 * cdn_codenet_head_fp32_tail_forward: y3 [N][Co][H][W] = (sum_c w3[o][c] a2[c]) + b3[o] (b3 may be NULL), c ascending from
 *   zero, a2 = relu(bn2(y2)) formed on load; 1 <= Co <= 4 (Co > 4: CDN_ERR_UNSUPPORTED; Co < 1: CDN_ERR_ARG).
 * cdn_codenet_head_fp32_tail_backward (1 <= Co <= 4): from grad_y3 [N][Co][H][W] and y2: grad_a2 = w3[0][c] g[0] (+ w3[o][c]
 *   g[o], o ascending), g_z2 = grad_a2 where z2 > 0 else 0 (stored); grad_beta2 = f32(T1), grad_gamma2 = f32(T2), mb2 =
 *   f32(T1 / n), mg2 = f32(T2 / n) with T1 = sum g_z2, T2 = sum g_z2 xh2; grad_w3 [Co][C] = f32(sum g[o] a2) and grad_b3 [Co] =
 *   f32(sum g[o]) (either may be NULL).
 * cdn_codenet_head_fp32_bn_backward1: the first backward pass of cdn_codenet_bn_relu_up_backward (up = 1) alone: g_z = grad_a
 *   where z > 0 else 0 (g_z must not be grad_a), grad_gamma, grad_beta, mb, mg as above.
 * cdn_codenet_head_fp32_dw_backward: grad_y2 = ((g_z2 - mb2) - xh2 mg2) * (gamma2 * invstd2) (training2 != 0) or g_z2 * (gamma2
 *   * invstd2) (training2 == 0: mb2 / mg2 not read) formed on load, 0 outside the plane; grad_a1[q] = sum_t w2[c][t] grad_y2[q -
 *   t]; g_z1 = grad_a1 where z1 > 0 else 0 (stored); grad_w2 [C][9] = f32(sum_p grad_y2[p] a1[p + t]); grad_beta1, grad_gamma1,
 *   mb1, mg1 from T1 = sum g_z1, T2 = sum g_z1 xh1.
 * cdn_codenet_head_fp32_bn_backward2: grad_y = ((g_z - mb) - xh mg) * (gamma * invstd) (training != 0) or g_z * (gamma *
 *   invstd), written to grad_y + n * grad_y_image_pitch + c * H * W: a channel slice of a wider [N][heads * C][H][W] buffer.
 * Every call takes a stream, allocates nothing, launches no memset node and is capturable.  The workspace is the caller's,
 * 16-byte aligned, every word written before it is read (CDN_ERR_WORKSPACE when too small).  16-byte loads where W % 4 == 0
 * and the pointers (and the pitch) are 16-byte aligned, scalar loads otherwise: the same terms in the same order.  Sizes below
 * 2^31 elements per tensor (CDN_ERR_UNSUPPORTED beyond).  Argument errors are returned before any HIP call.  Everything
 * written is OVERWRITTEN.
 * ---------------------------------------------------------------------------------------- */
size_t cdn_codenet_head_fp32_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W);
int cdn_codenet_head_fp32_bn_stats(const float *y, float *running_mean, float *running_var, int64_t *num_batches_tracked,
                                   float *mean, float *var, float *invstd, int64_t N, int64_t C, int64_t H, int64_t W,
                                   int training, double eps, double momentum, void *workspace, size_t workspace_bytes,
                                   void *stream);
int cdn_codenet_head_fp32_dw_forward(const float *y1, const float *mean1, const float *invstd1, const float *gamma1,
                                     const float *beta1, const float *w2, float *y2, int64_t N, int64_t C, int64_t H,
                                     int64_t W, void *stream);
int cdn_codenet_head_fp32_tail_forward(const float *y2, const float *mean2, const float *invstd2, const float *gamma2,
                                       const float *beta2, const float *w3, const float *b3, float *y3, int64_t N, int64_t C,
                                       int64_t Co, int64_t H, int64_t W, void *stream);
int cdn_codenet_head_fp32_tail_backward(const float *grad_y3, const float *y2, const float *mean2, const float *invstd2,
                                        const float *gamma2, const float *beta2, const float *w3, float *g_z2,
                                        float *grad_gamma2, float *grad_beta2, float *mb2, float *mg2, float *grad_w3,
                                        float *grad_b3, int64_t N, int64_t C, int64_t Co, int64_t H, int64_t W,
                                        void *workspace, size_t workspace_bytes, void *stream);
int cdn_codenet_head_fp32_bn_backward1(const float *grad_a, const float *y, const float *mean, const float *invstd,
                                       const float *gamma, const float *beta, float *g_z, float *grad_gamma, float *grad_beta,
                                       float *mb, float *mg, int64_t N, int64_t C, int64_t H, int64_t W, void *workspace,
                                       size_t workspace_bytes, void *stream);
int cdn_codenet_head_fp32_dw_backward(const float *g_z2, const float *y2, const float *mean2, const float *invstd2,
                                      const float *gamma2, const float *mb2, const float *mg2, int training2, const float *y1,
                                      const float *mean1, const float *invstd1, const float *gamma1, const float *beta1,
                                      const float *w2, float *g_z1, float *grad_w2, float *grad_gamma1, float *grad_beta1,
                                      float *mb1, float *mg1, int64_t N, int64_t C, int64_t H, int64_t W, void *workspace,
                                      size_t workspace_bytes, void *stream);
int cdn_codenet_head_fp32_bn_backward2(const float *g_z, const float *y, const float *mean, const float *invstd,
                                       const float *gamma, const float *mb, const float *mg, float *grad_y,
                                       int64_t grad_y_image_pitch, int64_t N, int64_t C, int64_t H, int64_t W, int training,
                                       void *stream);

/* ------------------------------------------------------------------------------------------
 * The fp32 ShuffleNetV2 units under autograd (lib/models/networks/shufflenetv2_dcn.py:57-114; layers 1-3 of main.py's
 * model); codenet_units_fp32_train.hip; DESIGN.md section 4.3g states the arithmetic: every float32 operation rounded on its
 * own, every sum in float64 in one order, no float atomics.  Per unit:
 *   stride 1:  x1 = x[:, :h] (unchanged)                  x2 = x[:, h:]
 *   stride 2:  y4 = dw3x3_s2(x, W4)   z4 = bn4(y4)        y5 = pw(z4, W5)   x1 = relu(bn5(y5))     x2 = x
 *   both:      y1 = pw(x2, W1)        a1 = relu(bn1(y1))  y2 = dw3x3_s(a1, W2)   z2 = bn2(y2)
 *              y3 = pw(z2, W3)        out[:, 2j] = x1[:, j],  out[:, 2j+1] = relu(bn3(y3))[:, j]
 * The dense 1x1 convolutions and their gradients are cdn_codenet_pointwise_forward(_pitched) / cdn_codenet_pointwise_wgrad
 * (_pitched), the statistics of every BatchNorm cdn_codenet_head_fp32_bn_stats, the second backward pass of BatchNorm1 / 3 /
 * 5 cdn_codenet_head_fp32_bn_backward2; these are the pieces in between.  All tensors float32 NCHW, n = N H W values per
 * channel; mean, invstd, mb, mg, gamma, beta are [C]; an "image pitch" is the distance in elements between two images of a
 * tensor (a channel slice x[:, a:b] of [N][Cx][H][W] is (x + a * H * W, pitch Cx * H * W)).  Ho = (H - 1) / stride + 1.
 * Never stored: a1 = relu(bn1(y1)), the unmasked grad_a1, grad_y2 / grad_y4 and the outputs of BatchNorm3 / 5 outside out.
 * cdn_codenet_unit_fp32_workspace_bytes: the workspace of a call below on an [N][C][H][W] tensor (the depthwise backward: its
 *   INPUT shape; the join backward: [N][h][H][W]): round_up_256(8 * max(C * slabs * 2, N * C * chunks * 11)), slabs =
 *   ceil(n / 4096), chunks = ceil(items / min(256, round_up_64(items))), items = ceil(W / 4) * ceil(H / 8); 0 for arguments
 *   the calls refuse.
 * cdn_codenet_unit_fp32_dw_forward: out [N][C][Ho][Wo] = dw3x3(a, w [C][9], stride 1 or 2, zero padding 1), out = ((0 + w[0]
 *   a[0]) + w[1] a[1]) + .. + w[8] a[8], taps row-major.  mean != NULL (with invstd, gamma, beta): a = relu(gamma * ((in - mean)
 *   * invstd) + beta) formed on load, 0 outside the plane; all four NULL: a = in as it is.  in is read through its image pitch.
 * cdn_codenet_unit_fp32_bn_forward: z = gamma * ((y - mean) * invstd) + beta, no ReLU (behind a depthwise), stored.
 * cdn_codenet_unit_fp32_join_forward (replaces BatchNorm apply + ReLU + cat + channel_shuffle): out [N][2h][H][W]: out[:, 2j +
 *   slot] = relu(bn(y [N][h][H][W]))[:, j]; x1 != NULL (slot 1 only): out[:, 2j] = x1[:, j] read at x1 + n * x1_image_pitch +
 *   j * H * W.
 * cdn_codenet_unit_fp32_join_backward: g_z [N][h][H][W] = grad_out[:, 2j + slot] where z > 0 else 0, z recomputed from y as in
 *   the forward; grad_beta = f32(T1), grad_gamma = f32(T2), mb = f32(T1 / n), mg = f32(T2 / n) with T1 = sum g_z, T2 = sum g_z
 *   xh; grad_x1 != NULL (slot 1 only): grad_x1 + n * pitch + j * H * W = grad_out[:, 2j].
 * cdn_codenet_unit_fp32_bn_backward_sums: the same four per-channel results for a BatchNorm without ReLU: g_z is grad_z itself.
 * cdn_codenet_unit_fp32_dw_backward: grad_y = ((grad_z - mb2) - xh2 mg2) * (gamma2 * invstd2) (training2 != 0) or grad_z *
 *   (gamma2 * invstd2) formed on load from grad_z, y [N][C][Ho][Wo], 0 outside the plane.  grad_a[Y][X] = the sum, from zero
 *   in row-major tap order, of w[dy][dx] grad_y[yo][xo] over the taps with Y + 1 - dy = stride * yo, X + 1 - dx = stride * xo
 *   (a gather).  mean1 != NULL (branch 2; in = y1): grad_in = grad_a where z1 > 0 else 0 (= g_z1, required), grad_beta1,
 *   grad_gamma1, mb1, mg1 from T1 = sum g_z1, T2 = sum g_z1 xh1.  mean1 == NULL (branch 1; in = x as it is; the other
 *   BatchNorm1 arguments NULL): grad_in (may be NULL) = grad_a, accumulate != 0: ADDED to what is stored there, by the one
 *   thread that owns the pixel.  grad_w [C][9] = f32(sum grad_y[p] a[stride p + t - 1]).
 * Every call takes a stream, allocates nothing, launches no memset node and is capturable.  The workspace is the caller's,
 * 16-byte aligned, every word written before it is read (CDN_ERR_WORKSPACE when too small).  16-byte accesses where the width
 * of a tensor is a multiple of 4 and its pointer and pitch are 16-byte aligned, scalar ones otherwise: the same terms in the
 * same order.  Sizes below 2^31 elements per tensor, pitches included (CDN_ERR_UNSUPPORTED beyond).  Argument errors are
 * returned before any HIP call.  Everything written is OVERWRITTEN (but grad_in with accumulate).
 * ---------------------------------------------------------------------------------------- */
size_t cdn_codenet_unit_fp32_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W);
int cdn_codenet_unit_fp32_dw_forward(const float *in, int64_t in_image_pitch, const float *mean, const float *invstd,
                                     const float *gamma, const float *beta, const float *w, float *out, int64_t N, int64_t C,
                                     int64_t H, int64_t W, int stride, void *stream);
int cdn_codenet_unit_fp32_bn_forward(const float *y, const float *mean, const float *invstd, const float *gamma,
                                     const float *beta, float *z, int64_t N, int64_t C, int64_t H, int64_t W, void *stream);
int cdn_codenet_unit_fp32_join_forward(const float *y, const float *mean, const float *invstd, const float *gamma,
                                       const float *beta, float *out, int slot, const float *x1, int64_t x1_image_pitch,
                                       int64_t N, int64_t h, int64_t H, int64_t W, void *stream);
int cdn_codenet_unit_fp32_join_backward(const float *grad_out, const float *y, const float *mean, const float *invstd,
                                        const float *gamma, const float *beta, float *g_z, float *grad_gamma, float *grad_beta,
                                        float *mb, float *mg, int slot, float *grad_x1, int64_t grad_x1_image_pitch, int64_t N,
                                        int64_t h, int64_t H, int64_t W, void *workspace, size_t workspace_bytes,
                                        void *stream);
int cdn_codenet_unit_fp32_bn_backward_sums(const float *grad_z, const float *y, const float *mean, const float *invstd,
                                           float *grad_gamma, float *grad_beta, float *mb, float *mg, int64_t N, int64_t C,
                                           int64_t H, int64_t W, void *workspace, size_t workspace_bytes, void *stream);
int cdn_codenet_unit_fp32_dw_backward(const float *grad_z, const float *y, const float *mean2, const float *invstd2,
                                      const float *gamma2, const float *mb2, const float *mg2, int training2, const float *in,
                                      int64_t in_image_pitch, const float *mean1, const float *invstd1, const float *gamma1,
                                      const float *beta1, const float *w, float *grad_in, int64_t grad_in_image_pitch,
                                      int accumulate, float *grad_w, float *grad_gamma1, float *grad_beta1, float *mb1,
                                      float *mg1, int64_t N, int64_t C, int64_t H, int64_t W, int stride, void *workspace,
                                      size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * The fp32 stem under autograd (layer0 of main.py's model: Conv2d(3, 24, 3, stride 4 | 2, padding 1, bias=False) ->
 * BatchNorm2d -> ReLU [-> MaxPool2d(3, 2, 1)]); codenet_stem_fp32_train.hip; DESIGN.md section 4.3h states the arithmetic:
 * every float32 operation rounded on its own, T1 / T2 in float64 in one order, no float atomics.  The raw convolution y0 is
 * cdn_codenet_stem_train_forward with b = NULL and running = 0, its statistics cdn_codenet_head_fp32_bn_stats, the un-pooled
 * stem's output cdn_codenet_bn_relu_up_forward with up = 1; these are the pieces in between.  All tensors float32 NCHW; y0 is
 * [N][C][H][W] (H, W: ITS size, not the image's), n = N H W values per channel; mean, invstd, mb, mg, gamma, beta are [C];
 * Hp = (H - 1) / 2 + 1.  Never stored: a0 = relu(bn(y0)), the ReLU mask, grad_y0 and, without the pool, g_z.
 * cdn_codenet_stem_fp32_workspace_bytes: the workspace of the two backward calls on y0: round_up_256(C * slabs * 16), slabs =
 *   ceil(n / 4096); 0 for arguments the calls refuse, shapes of 2^31 elements or more included.
 * cdn_codenet_stem_fp32_pool_forward: out [N][C][Hp][Wp] = max over the 3x3 window, stride 2, padding 1, clipped at the
 *   borders, of a0 = relu(gamma * ((y0 - mean) * invstd) + beta) formed on load: the winner of `val > max || isnan(val)` from
 *   -inf in row-major scan order (a NaN in the window wins).
 * cdn_codenet_stem_fp32_pool_backward: from g [N][C][Hp][Wp]: a window's gradient goes to its first maximum in that scan
 *   order, compared on a0 formed on load; a pixel adds the windows it won in row-major window order from 0.0f (a gather, every
 *   element written exactly once); g_z [N][C][H][W] = that sum where z > 0 else 0 (stored); grad_beta = f32(T1), grad_gamma =
 *   f32(T2), mb = f32(T1 / n), mg = f32(T2 / n) with T1 = sum g_z, T2 = sum g_z xh, the (channel, slab) sums of
 *   cdn_codenet_bn_relu_up_backward.
 * cdn_codenet_stem_fp32_bn_relu_backward_sums: the same four per-channel results for the un-pooled stem: g [N][C][H][W] is
 *   grad_out, g_z = g where z > 0 else 0 is formed on load; nothing of tensor size is written.
 * cdn_codenet_stem_fp32_wgrad (N, H, W: the IMAGE's size; Co must be 24, stride 2 or 4; Ho = (H - 1) / stride + 1): grad_w
 *   [24][27] = sum grad_y0[n][c][oy][ox] img[n][ci][oy S + dy - 1][ox S + dx - 1] (zero outside the image) with grad_y0 =
 *   ((g_z - mb) - xh mg) * (gamma * invstd) (training != 0) or g_z * (gamma * invstd) (training == 0: mb / mg not read) formed
 *   on load from g, y0 [N][24][Ho][Wo]; masked != 0: g is g_z (the pool backward's); masked == 0: g is grad_out and g_z = g
 *   where z > 0 else 0.  float32 fma in the decomposition and chunk order of cdn_codenet_stem_backward; OVERWRITTEN.
 *   cdn_codenet_stem_fp32_wgrad_workspace_bytes: the size cdn_codenet_stem_backward_workspace_bytes gives; 0 for arguments the
 *   call refuses, an image or a y0 of 2^31 elements or more included.
 * Every call takes a stream, allocates nothing, launches no memset node and is capturable.  The workspace is the caller's,
 * 16-byte aligned, every word written before it is read (CDN_ERR_WORKSPACE when too small).  16-byte accesses where the width
 * of a tensor is a multiple of 4 and its pointer is 16-byte aligned, scalar ones otherwise: the same terms in the same order.
 * Sizes below 2^31 elements per tensor (CDN_ERR_UNSUPPORTED beyond).  Argument errors are returned before any HIP call.
 * ---------------------------------------------------------------------------------------- */
size_t cdn_codenet_stem_fp32_workspace_bytes(int64_t N, int64_t C, int64_t H, int64_t W);
int cdn_codenet_stem_fp32_pool_forward(const float *y0, const float *mean, const float *invstd, const float *gamma,
                                       const float *beta, float *out, int64_t N, int64_t C, int64_t H, int64_t W,
                                       void *stream);
int cdn_codenet_stem_fp32_pool_backward(const float *g, const float *y0, const float *mean, const float *invstd,
                                        const float *gamma, const float *beta, float *g_z, float *grad_gamma, float *grad_beta,
                                        float *mb, float *mg, int64_t N, int64_t C, int64_t H, int64_t W, void *workspace,
                                        size_t workspace_bytes, void *stream);
int cdn_codenet_stem_fp32_bn_relu_backward_sums(const float *g, const float *y0, const float *mean, const float *invstd,
                                                const float *gamma, const float *beta, float *grad_gamma, float *grad_beta,
                                                float *mb, float *mg, int64_t N, int64_t C, int64_t H, int64_t W,
                                                void *workspace, size_t workspace_bytes, void *stream);
size_t cdn_codenet_stem_fp32_wgrad_workspace_bytes(int64_t N, int64_t H, int64_t W, int stride);
int cdn_codenet_stem_fp32_wgrad(const float *g, int masked, const float *y0, const float *img, const float *mean,
                                const float *invstd, const float *gamma, const float *beta, const float *mb, const float *mg,
                                float *grad_w, int64_t N, int64_t H, int64_t W, int64_t Co, int stride, int training,
                                void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Detection scoring: VOC07 AP per class and COCO's bbox precision / recall arrays from a detection table that stays on
 * the device.  codenet_eval.hip + cdn_eval.h; Python: codenet_amd/evalio.py (DeviceResults, GroundTruth, voc_eval_device,
 * coco_eval).  DESIGN.md section 7.4e is the contract; tests/coco_eval_ref.py restates the COCO half in numpy.
 * All box arithmetic is float64, every operation rounded on its own; what crosses lanes is an integer count or a
 * maximum, so every entry is a pure function of its inputs bit for bit.  Every entry has a `_host` twin without the
 * stream argument that runs the same text (cdn_eval.h) on HOST memory with no HIP call.  One launch per entry, no host
 * synchronisation.  Argument errors are returned before any HIP call.
 *
 *   det    [n_images][cap][6] float64: x1 y1 x2 y2 score class (VOC) or x y w h score class (COCO), class 0-based
 *   count  [n_images] int32 rows in use, zeroed by the caller before the first append
 *   flag   [1] int32, zeroed by the caller: bit 0 an append met more than cap rows (the rows beyond are NOT stored and
 *          the accumulate entries hand the word back: the caller must treat it as an error), bit 1 a score that the
 *          sort key cannot order (NaN, or |score| >= 2^31 / 100 in COCO mode)
 *   gt_box [total_gt][4] float64 (x1 y1 x2 y2 / x y w h), gt_area [total_gt], gt_flag [total_gt] int32 (bit 0: difficult
 *          / iscrowd), gt_off [n_images * classes + 1] int32: the rows of (image, class) are gt_off[i * classes + c] ..
 * cap <= 1024, classes <= 256, n_images * cap < 2^25 (CDN_ERR_UNSUPPORTED beyond).
 *
 * cdn_eval_append: the result block of cdn_ctdet_merge_scales (boxes [B][classes][R][5] float32, rows_out [B][classes])
 *   behind the rows already in slots image_slot .. image_slot + B - 1, class-major.  coco != 0: w = x2 - x1 and
 *   h = y2 - y1 in float32, then every number v becomes rint((double)v * 100.0) / 100.0 = float("%.2f" % v).
 * cdn_eval_sort_keys: keys [n_images * cap] int64 = (class << 32) | inverted orderable score; rows behind count sort
 *   last.  An ascending STABLE sort of the keys (the caller's: torch.sort) orders every class by descending score with
 *   ties in (image, row) order; keys_sorted / perm below are its two results.
 * cdn_eval_match_voc: voc_eval.py:95-207 per (image, class), one wave each: tp / fp [n_images * cap] uint8 per table row.
 *   seen [total_gt] uint8 scratch.
 * cdn_eval_accumulate_voc: per class rec / prec [n_images * cap] at the sorted positions, env (the envelope) and terms
 *   [n_images * cap + classes] scratch; thresholds [n_thr] the recall points (np.arange(0, 1.1, 0.1)).
 *   out [4 * classes + 2] float64: ap_07 [classes], ap_area [classes] (numpy's pairwise summation order), npos [classes],
 *   the first sorted position of every class [classes + 1], the flag word.
 * cdn_eval_match_coco: COCOeval.evaluateImg for bbox per (image, category), one wave each, lanes = 10 IoU thresholds x 4
 *   area ranges (area_rng [4][2]).  dtm / dtig [40][n_images * cap] uint8 (lane = threshold * 4 + area range) per table
 *   row, rank [n_images * cap] int32 within (image, category), gt_nonign [n_images * classes][4] int32; gtm [40][total_gt]
 *   uint8 scratch.  The first 100 ranked detections take part.  The D x G IoU matrix lives in LDS when D * G <= 4096 and
 *   is formed on the fly otherwise: the same bits.  No cap on G.
 * cdn_eval_accumulate_coco: COCOeval.accumulate: precision [10][101][classes][4][3], recall [10][classes][4][3]
 *   (maxDets 1, 10, 100; -1 where no ground truth counts), rec_thrs [101]; flag_out [1] float64 = the flag word.
 * ---------------------------------------------------------------------------------------- */
int cdn_eval_append(const float *boxes, const int32_t *rows_out, int64_t B, int64_t classes, int64_t R, int64_t image_slot,
                    double *det, int32_t *count, int64_t n_images, int64_t cap, int coco, int32_t *flag, void *stream);
int cdn_eval_append_host(const float *boxes, const int32_t *rows_out, int64_t B, int64_t classes, int64_t R,
                         int64_t image_slot, double *det, int32_t *count, int64_t n_images, int64_t cap, int coco,
                         int32_t *flag);
int cdn_eval_sort_keys(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes, int coco,
                       int64_t *keys, int32_t *flag, void *stream);
int cdn_eval_sort_keys_host(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes, int coco,
                            int64_t *keys, int32_t *flag);
int cdn_eval_match_voc(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                       const double *gt_box, const int32_t *gt_flag, const int32_t *gt_off, double ovthresh,
                       unsigned char *seen, unsigned char *tp, unsigned char *fp, void *stream);
int cdn_eval_match_voc_host(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                            const double *gt_box, const int32_t *gt_flag, const int32_t *gt_off, double ovthresh,
                            unsigned char *seen, unsigned char *tp, unsigned char *fp);
int cdn_eval_accumulate_voc(const int64_t *keys_sorted, const int64_t *perm, int64_t n_images, int64_t cap, int64_t classes,
                            const unsigned char *tp, const unsigned char *fp, const int32_t *gt_flag, const int32_t *gt_off,
                            const double *thresholds, int64_t n_thr, const int32_t *flag, double *rec, double *prec,
                            double *env, double *terms, double *out, void *stream);
int cdn_eval_accumulate_voc_host(const int64_t *keys_sorted, const int64_t *perm, int64_t n_images, int64_t cap,
                                 int64_t classes, const unsigned char *tp, const unsigned char *fp, const int32_t *gt_flag,
                                 const int32_t *gt_off, const double *thresholds, int64_t n_thr, const int32_t *flag,
                                 double *rec, double *prec, double *env, double *terms, double *out);
int cdn_eval_match_coco(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                        const double *gt_box, const double *gt_area, const int32_t *gt_flag, const int32_t *gt_off,
                        int64_t total_gt, const double *iou_thrs, const double *area_rng, unsigned char *gtm,
                        unsigned char *dtm, unsigned char *dtig, int32_t *rank, int32_t *gt_nonign, void *stream);
int cdn_eval_match_coco_host(const double *det, const int32_t *count, int64_t n_images, int64_t cap, int64_t classes,
                             const double *gt_box, const double *gt_area, const int32_t *gt_flag, const int32_t *gt_off,
                             int64_t total_gt, const double *iou_thrs, const double *area_rng, unsigned char *gtm,
                             unsigned char *dtm, unsigned char *dtig, int32_t *rank, int32_t *gt_nonign);
int cdn_eval_accumulate_coco(const int64_t *keys_sorted, const int64_t *perm, int64_t n_images, int64_t cap, int64_t classes,
                             const unsigned char *dtm, const unsigned char *dtig, const int32_t *rank,
                             const int32_t *gt_nonign, const double *rec_thrs, const int32_t *flag, double *precision,
                             double *recall, double *flag_out, void *stream);
int cdn_eval_accumulate_coco_host(const int64_t *keys_sorted, const int64_t *perm, int64_t n_images, int64_t cap,
                                  int64_t classes, const unsigned char *dtm, const unsigned char *dtig, const int32_t *rank,
                                  const int32_t *gt_nonign, const double *rec_thrs, const int32_t *flag, double *precision,
                                  double *recall, double *flag_out);

/* ------------------------------------------------------------------------------------------
 * Optional per-kernel timing with HIP events on the launch stream (thread-local; off by default).
 * While enabled, each kernel of cdn_codenet_stage_fused_forward / cdn_codenet_unpack_nchw records
 * an event pair.  cdn_profile_read synchronises the recorded events and returns up to max_records
 * {kernel id (0 scale, 1 gather/depthwise, 2 pointwise, 3 unpack), tag (stage height), ms}, then
 * clears the list.  Not to be enabled while the stream is being captured into a HIP graph.
 * ---------------------------------------------------------------------------------------- */
int cdn_profile_enable(int on);
int cdn_profile_read(int max_records, int *kernel_ids, int *tags, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* CODENET_DCN_H_ */
