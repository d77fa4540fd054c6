"""The fp32 stem (layer0) in training as ONE autograd function on the HIP kernels of csrc/codenet_stem_fp32_train.hip
(DESIGN.md section 4.3h).

The reference's main.py trains the fp32 model; its stem is (shufflenetv2_dcn.py)

    layer0 = Sequential(Conv2d(3, 24, 3, stride 4 | 2, padding 1, bias=False), BatchNorm2d(24), ReLU[, MaxPool2d(3, 2, 1)])

three or four framework modules under autograd, the "S2 + MaxPool" form passing about ten times over a tensor four times
the size of its output.  Here one ``CodenetStemFp32Function`` between the image and layer1:

    forward   cdn_codenet_stem_train_forward with b = NULL, running = 0 (y0, raw, stored), then un-pooled
              cdn_codenet_bn_relu_up_forward with up = 1 (the statistics and out = relu(bn(y0))), pooled
              cdn_codenet_head_fp32_bn_stats and cdn_codenet_stem_fp32_pool_forward (a0 = relu(bn(y0)) formed on load,
              never written)
    backward  pooled cdn_codenet_stem_fp32_pool_backward (the window's gradient to its first maximum, masked by z > 0,
              stored as g_z; BatchNorm's sums in the same launch), un-pooled cdn_codenet_stem_fp32_bn_relu_backward_sums
              (the mask formed on load, only the sums); then cdn_codenet_stem_fp32_wgrad (grad_y0 formed on load, never
              stored; grad W in the fixed order of the quantised stem's weight gradient)

The BatchNorm follows its own ``training`` flag: batch statistics (running buffers and num_batches_tracked advance in
place, on the device) or the running statistics (nothing is written).  The image takes no gradient: an input that requires
one keeps the module path.  Every floating-point sum has one order, nothing allocates outside the caching allocator, the
step is capturable.
"""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N_
from .. import ops
from . import codenet_stage as CS
from ._fp32_common import (_bn_reason, _hook_reason, _input_reason, _one_value_error, _out_hw, _placement_reason, bn_relu_up,
                           bn_stats)

# A/B switch (tools/stem_fp32_bench.py): the fp32 stem of a training step on the kernels above (True) or module by module
# through the framework's autograd (False)
NATIVE_FP32_STEM = True

_p = CS._p


def _conv_forward(x, w, stride):
    """The raw stem output y0 = conv3x3(x, w, stride, zero padding 1): the QAT stem's forward without bias and QuantAct."""
    Nb, _, H, W = x.shape
    Co = w.shape[0]
    y0 = x.new_empty(Nb, Co, *_out_hw(H, W, stride))
    rc = N_.lib().cdn_codenet_stem_train_forward(_p(x), _p(w), None, _p(y0), Nb, H, W, Co, stride, None, None, None, None,
                                                 8, 0.0, 0, None, ops._stream(x))
    N_.check(rc, "cdn_codenet_stem_train_forward")
    return y0


def _pool_forward(y0, st, gamma, beta):
    """out = maxpool3x3_s2_p1(relu(bn(y0))); st = (mean, var, invstd) of y0."""
    Nb, C, H, W = y0.shape
    out = y0.new_empty(Nb, C, *_out_hw(H, W, 2))
    rc = N_.lib().cdn_codenet_stem_fp32_pool_forward(_p(y0), _p(st[0]), _p(st[2]), _p(gamma), _p(beta), _p(out), Nb, C, H, W,
                                                     ops._stream(y0))
    N_.check(rc, "cdn_codenet_stem_fp32_pool_forward")
    return out


def _bn_backward1(g, y0, st, gamma, beta, pooled):
    """(g_z or None, grad_gamma, grad_beta, means [2, C] = (mb, mg)) of the BatchNorm + ReLU [+ pool] behind y0.  pooled: g
    is the pooled output's gradient and g_z is stored; else g is grad_out and g_z is only summed."""
    lib = N_.lib()
    Nb, C, H, W = y0.shape
    gg, gb, means = y0.new_empty(C), y0.new_empty(C), y0.new_empty(2, C)
    ws = CS._workspace(lib.cdn_codenet_stem_fp32_workspace_bytes(Nb, C, H, W), y0.device)
    head = (_p(g), _p(y0), _p(st[0]), _p(st[2]), _p(gamma), _p(beta))
    tail = (_p(gg), _p(gb), _p(means[0]), _p(means[1]), Nb, C, H, W, _p(ws), ws.numel() * 4, ops._stream(y0))
    if pooled:
        gz = torch.empty_like(y0)
        rc = lib.cdn_codenet_stem_fp32_pool_backward(*head, _p(gz), *tail)
        N_.check(rc, "cdn_codenet_stem_fp32_pool_backward")
    else:
        gz = None
        rc = lib.cdn_codenet_stem_fp32_bn_relu_backward_sums(*head, *tail)
        N_.check(rc, "cdn_codenet_stem_fp32_bn_relu_backward_sums")
    return gz, gg, gb, means


def _wgrad(g, masked, y0, x, st, gamma, beta, means, stride, training):
    """grad_W [24, 3, 3, 3]; masked: g is g_z at y0's resolution, else grad_out (the mask z > 0 is formed on load)."""
    lib = N_.lib()
    Nb, _, H, W = x.shape
    Co = y0.shape[1]
    gw = x.new_empty(Co, 3, 3, 3)
    ws = CS._workspace(lib.cdn_codenet_stem_fp32_wgrad_workspace_bytes(Nb, H, W, stride), x.device)
    rc = lib.cdn_codenet_stem_fp32_wgrad(_p(g), int(bool(masked)), _p(y0), _p(x), _p(st[0]), _p(st[2]), _p(gamma), _p(beta),
                                         _p(means[0]), _p(means[1]), _p(gw), Nb, H, W, Co, stride, int(bool(training)), _p(ws),
                                         ws.numel() * 4, ops._stream(x))
    N_.check(rc, "cdn_codenet_stem_fp32_wgrad")
    return gw


class CodenetStemFp32Function(Function):
    """out = layer0(img).  meta = (stride, bn, pooled), bn the nn.BatchNorm2d; w, gamma, beta: the convolution's weight and
    the BatchNorm's affine parameters.  The BatchNorm buffers are updated in place by the forward, as the module path does.
    keep (a dict or None) receives x, w, y0, "bn" = (mean, var, invstd), pooled and out from the forward and, from the
    backward, grad_out, g_z (pooled stem; None otherwise: it is never formed in memory), "means" = (mb, mg), grad_gamma,
    grad_beta and grad_w.  No gradient for the image."""

    @staticmethod
    def forward(ctx, x, meta, keep, w, gamma, beta):
        ops._gpu_f32(x, w, gamma, beta)
        ctx.set_materialize_grads(False)
        stride, bn, pooled = meta
        w, gamma, beta = w.contiguous(), gamma.contiguous(), beta.contiguous()
        training = bool(bn.training)
        y0 = _conv_forward(x, w, stride)
        if pooled:
            st = bn_stats(y0, bn)
            out = _pool_forward(y0, st, gamma, beta)
        else:
            out, *st = bn_relu_up(y0, gamma, beta, bn)
        if keep is not None:
            keep.update(x=x, w=w, y0=y0, bn=tuple(st), pooled=pooled, out=out)
        ctx.stride, ctx.pooled, ctx.training, ctx.keep = stride, pooled, training, keep
        ctx.save_for_backward(x, y0, st[0], st[2], gamma, beta)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        if gout is None:
            return (None,) * 6
        x, y0, mean, invstd, gamma, beta = ctx.saved_tensors
        st = (mean, None, invstd)
        gout = gout.contiguous()
        gz, gg, gb, means = _bn_backward1(gout, y0, st, gamma, beta, ctx.pooled)
        gw = _wgrad(gz if ctx.pooled else gout, ctx.pooled, y0, x, st, gamma, beta, means, ctx.stride, ctx.training)
        if ctx.keep is not None:
            ctx.keep.update(grad_out=gout, g_z=gz, means=means, grad_gamma=gg, grad_beta=gb, grad_w=gw)
        need = ctx.needs_input_grad
        return None, None, None, gw if need[3] else None, gg if need[4] else None, gb if need[5] else None


def _split(layer0):
    """(Conv2d, BatchNorm2d, MaxPool2d or None) of an fp32 stem, or the reason -- a string -- why it is none."""
    if not (isinstance(layer0, nn.Sequential) and len(layer0) in (3, 4) and type(layer0[0]) is nn.Conv2d
            and type(layer0[1]) is nn.BatchNorm2d and isinstance(layer0[2], nn.ReLU)):
        return ("layer0 is not exactly Sequential(Conv2d, BatchNorm2d, ReLU[, MaxPool2d(3, 2, 1)]) (the quantised stem has "
                "functions/codenet_stem.CodenetStemFunction)")
    pool = layer0[3] if len(layer0) == 4 else None
    if pool is not None:
        pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)      # noqa: E731
        if not (isinstance(pool, nn.MaxPool2d) and pair(pool.kernel_size) == (3, 3) and pair(pool.stride) == (2, 2)
                and pair(pool.padding) == (1, 1) and pair(pool.dilation) == (1, 1) and not pool.ceil_mode
                and not pool.return_indices):
            return "layer0: its pool is not MaxPool2d(3, 2, 1) with ceil_mode=False, dilation 1 and no indices"
    return layer0[0], layer0[1], pool


def native_reason(layer0, x):
    """None when forward_stem runs the fp32 `layer0` on the kernels for the image x, else the reason -- a string -- why it
    takes the module path.  x None: the modules alone are judged (structure and settings, not where the model lives):
    pipeline.GraphedTrainStep.is_fp32_net."""
    if not NATIVE_FP32_STEM:
        return "NATIVE_FP32_STEM is off"
    if not torch.is_grad_enabled():
        return "grad mode is off (inference has pipeline.FusedBackbone)"
    parts = _split(layer0)
    if isinstance(parts, str):
        return parts
    conv, bn, pool = parts
    stride = (2, 2) if pool is not None else (4, 4)
    if not (conv.in_channels == 3 and conv.out_channels == 24 and tuple(conv.kernel_size) == (3, 3)
            and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and getattr(conv, "padding_mode", "zeros") == "zeros" and tuple(conv.stride) == stride):
        return ("layer0: not the stem's own geometry (3 -> 24, 3x3, stride 2 in front of the pool or stride 4 without one, "
                "zero padding 1, groups 1)")
    if conv.bias is not None:
        return "layer0: its convolution has a bias (the reference's has none)"
    why = _bn_reason(bn, conv.out_channels, "layer0: its BatchNorm2d") or _hook_reason(layer0, "layer0")
    if why is not None:
        return why
    if x is None:
        return None
    s = stride[0]
    why = _input_reason(x, lambda H, W: max(3 * H * W, 24 * ((H - 1) // s + 1) * ((W - 1) // s + 1)), channels=3,
                        aligned=True, takes_grad=False)
    if why is not None:
        return why
    return _placement_reason(x, layer0.parameters(), layer0.buffers(), "layer0: ")      # (x takes no grad: refused above)


def forward_fp32_stem(layer0, x, keep=None):
    """``layer0(x)`` for an fp32 stem that native_reason(layer0, x) accepts, as one CodenetStemFp32Function.  keep (tests): a
    dict that receives the function's own intermediates."""
    conv, bn, pool = _split(layer0)
    stride = int(conv.stride[0])
    Nb, _, H, W = x.shape
    Ho, Wo = _out_hw(H, W, stride)
    if bn.training and Nb * Ho * Wo == 1:      # the framework's error for one value per channel, before any launch
        raise _one_value_error((Nb, conv.out_channels, Ho, Wo))
    return CodenetStemFp32Function.apply(x, (stride, bn, pool is not None), keep, conv.weight, bn.weight, bn.bias)
