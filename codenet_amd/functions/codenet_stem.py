"""The quantised stem (layer0) as an autograd function on the HIP kernels (training path).

After ``quantize_shufflenetv2_dcn`` the stem is

    layer0 = Sequential(QuantBnConv2d(8),                                  # Conv2d(3, 24, 3, stride 4 | 2, padding 1) + BN fold
                        Sequential(ReLU, QuantAct[, MaxPool2d(3, 2, 1)]))

and the reference runs it module by module under autograd, its backward being the framework's convolution weight gradient.
Here one ``CodenetStemFunction`` between the image and layer1:

    forward   cdn_codenet_stem_train_forward (y0 = conv + b, stored raw; the QuantAct updated by the launch's last workgroup
              on the extremes of max(y0, 0)), then cdn_quantact_relu_apply (out = fq(relu(y0)) with the state snapshot) or,
              for the "S2 + MaxPool" stems, cdn_codenet_stem_pool_forward (out = fq(relu(window maximum of y0)))
    backward  [cdn_codenet_stem_pool_backward (the window's gradient to its first maximum, masked by y0 > 0)]
              cdn_codenet_stem_backward (grad Wq, grad b in a fixed order; the ReLU mask formed on load without the pool)

Straight-through quantiser, ReLU masks y0 > 0.  The weight transformation (BN fold, 8-bit fake-quantisation) stays the native
autograd function of codenet_stage.py (``QuantBnConv2d.folded``).  The image takes no gradient: an input that requires one
keeps the module path.  Every floating-point sum has one order, nothing allocates outside the caching allocator, the step is
capturable.
"""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N_
from .. import ops
from . import codenet_stage as CS
from ._qat_common import (_act_reason, _hook_reason, _input_reason, _placement_reason, _tracked_act,
                          _weight_prep_structural)

# A/B switch (tools/stem_train_bench.py): the stem of a QAT step on the kernels above (True) or module by module through the
# framework's autograd (False)
NATIVE_STEM = True

_p = CS._p


def _conv_forward(x, w, b, stride, act):
    """The raw stem output y0 (stored before ReLU and quantisation) and the snapshot of the state of the QuantAct behind it."""
    Nb, _, H, W = x.shape
    Co = w.shape[0]
    y0 = x.new_empty(Nb, Co, (H - 1) // stride + 1, (W - 1) // stride + 1)
    snap, upd = _tracked_act(act, x.device)
    rc = N_.lib().cdn_codenet_stem_train_forward(_p(x), _p(w), _p(b), _p(y0), Nb, H, W, Co, stride, *upd, ops._stream(x))
    N_.check(rc, "cdn_codenet_stem_train_forward")
    return y0, snap


def _quantise(y0, snap, pooled):
    """out = fq(relu(y0)) with the state snapshot; pooled: of the 3x3 / stride 2 / padding 1 window maximum."""
    Nb, C, H, W = y0.shape
    if pooled:
        out = y0.new_empty(Nb, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
        rc = N_.lib().cdn_codenet_stem_pool_forward(_p(y0), _p(snap), _p(out), Nb, C, H, W, ops._stream(y0))
        N_.check(rc, "cdn_codenet_stem_pool_forward")
    else:
        out = torch.empty_like(y0)
        rc = N_.lib().cdn_quantact_relu_apply(_p(y0), _p(out), Nb * C, H, W, 0, _p(snap), ops._stream(y0))
        N_.check(rc, "cdn_quantact_relu_apply")
    return out


def _pool_backward(g, y0, snap):
    """gy0 = dL/dy0 from the pooled output's gradient, already masked by y0 > 0."""
    Nb, C, H, W = y0.shape
    gy0 = torch.empty_like(y0)
    rc = N_.lib().cdn_codenet_stem_pool_backward(_p(g), _p(y0), _p(snap), _p(gy0), Nb, C, H, W, ops._stream(y0))
    N_.check(rc, "cdn_codenet_stem_pool_backward")
    return gy0


def _param_grads(g, y0, x, stride):
    """(grad_Wq [24, 3, 3, 3], grad_b [24]); y0 given: g is masked by y0 > 0 on load, None: g is masked already."""
    lib = N_.lib()
    Nb, _, H, W = x.shape
    Co = g.shape[1]
    gw, gb = x.new_empty(Co, 3, 3, 3), x.new_empty(Co)
    ws = CS._workspace(lib.cdn_codenet_stem_backward_workspace_bytes(Nb, H, W, stride), x.device)
    rc = lib.cdn_codenet_stem_backward(_p(g), _p(y0), _p(x), _p(gw), _p(gb), Nb, H, W, Co, stride, _p(ws), ws.numel() * 4,
                                       ops._stream(x))
    N_.check(rc, "cdn_codenet_stem_backward")
    return gw, gb


class CodenetStemFunction(Function):
    """out = layer0(img).  meta = (stride, act, pooled); wq, b: the folded, fake-quantised weights and the folded bias.  The
    QuantAct's buffers are updated in place by the forward, as the module path does.  keep (a dict or None) receives the
    saved tensors themselves.  No gradient for the image."""

    @staticmethod
    def forward(ctx, x, meta, keep, wq, b):
        ops._gpu_f32(x, wq, b)
        ctx.set_materialize_grads(False)
        stride, act, pooled = meta
        wq, b = wq.contiguous(), b.contiguous()
        y0, snap = _conv_forward(x, wq, b, stride, act)
        out = _quantise(y0, snap, pooled)
        if keep is not None:
            keep.update(x=x, y0=y0, snap=snap, pooled=pooled, wq=wq, b=b, out=out)
        ctx.stride, ctx.pooled, ctx.keep = stride, pooled, keep
        ctx.save_for_backward(x, y0, snap)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        if gout is None:
            return None, None, None, None, None
        x, y0, snap = ctx.saved_tensors
        gout = gout.contiguous()
        if ctx.pooled:
            gy0 = _pool_backward(gout, y0, snap)
            if ctx.keep is not None:
                ctx.keep["gy0"] = gy0
            gw, gb = _param_grads(gy0, None, x, ctx.stride)
        else:
            gw, gb = _param_grads(gout, y0, x, ctx.stride)
        return None, None, None, gw, gb


def _split(layer0):
    """(QuantBnConv2d, QuantAct, MaxPool2d or None) of a quantised stem, or the reason -- a string -- why it is none."""
    from ..portable_quantizer.quant_modules import QuantAct, QuantBnConv2d
    if not (isinstance(layer0, nn.Sequential) and len(layer0) == 2 and isinstance(layer0[0], QuantBnConv2d)):
        return "layer0 is not Sequential(QuantBnConv2d, ...) (the fp32 stem keeps the module path)"
    post = layer0[1]
    if not (isinstance(post, nn.Sequential) and len(post) in (2, 3) and isinstance(post[0], nn.ReLU)
            and isinstance(post[1], QuantAct)):
        return "layer0: its second module is not Sequential(ReLU, QuantAct[, MaxPool2d])"
    pool = post[2] if len(post) == 3 else None
    if pool is not None:
        pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)      # noqa: E731
        if not (isinstance(pool, nn.MaxPool2d) and pair(pool.kernel_size) == (3, 3) and pair(pool.stride) == (2, 2)
                and pair(pool.padding) == (1, 1) and pair(pool.dilation) == (1, 1) and not pool.ceil_mode
                and not pool.return_indices):
            return "layer0: its pool is not MaxPool2d(3, 2, 1) with ceil_mode=False, dilation 1 and no indices"
    return layer0[0], post[1], pool


def native_reason(layer0, x):
    """None when forward_stem runs `layer0` on the kernels for the image x, else the reason -- a string -- why it takes the
    module path.  x None: the modules alone are judged (structure and settings, not where the model lives):
    GraphedTrainStep.is_native_net."""
    if not NATIVE_STEM:
        return "NATIVE_STEM is off"
    if not torch.is_grad_enabled():
        return "grad mode is off (inference has pipeline.FusedBackbone)"
    parts = _split(layer0)
    if isinstance(parts, str):
        return parts
    cb, act, pool = parts
    why = _hook_reason(layer0, "layer0")
    if why is not None:
        return why
    conv = cb.conv
    if not (conv.in_channels == 3 and conv.out_channels == 24 and tuple(conv.kernel_size) == (3, 3)
            and tuple(conv.padding) == (1, 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1
            and getattr(conv, "padding_mode", "zeros") == "zeros" and tuple(conv.stride) in ((2, 2), (4, 4))):
        return "layer0: not the stem's own geometry (3 -> 24, 3x3, stride 2 or 4, zero padding 1)"
    if not _weight_prep_structural(conv.weight, cb) or cb.weight_bit > 8:
        return ("layer0: its weight quantiser is not on the device weight-prep path (per-channel symmetric, <= 8 bits, "
                "quantising, no bias quantisation)")
    why = _act_reason(act, "layer0: its QuantAct")
    if why is not None:
        return why
    if x is None:
        return None
    s = conv.stride[0]
    why = _input_reason(x, lambda H, W: max(3 * H * W, 24 * ((H - 1) // s + 1) * ((W - 1) // s + 1)), channels=3,
                        aligned=True, takes_grad=False)
    return why or _placement_reason(x, [(conv.weight, cb)], [act])


def forward_stem(layer0, x, keep=None):
    """``layer0(x)`` for the stem.  In the QAT step on the GPU (native_reason(layer0, x) is None) it runs as one
    CodenetStemFunction; an fp32 stem that codenet_stem_fp32.native_reason accepts runs as one CodenetStemFp32Function;
    otherwise exactly ``layer0(x)``.  keep (tests): a dict that receives the native path's own y0, the state snapshot, the
    pooled flag and -- after the backward of a pooled stem -- gy0 (the fp32 function: see its docstring)."""
    from . import codenet_stem_fp32 as S32
    if S32.native_reason(layer0, x) is None:
        return S32.forward_fp32_stem(layer0, x, keep)
    if native_reason(layer0, x) is not None:
        return layer0(x)
    cb, act, pool = _split(layer0)
    wq, b = cb.folded()
    return CodenetStemFunction.apply(x, (int(cb.conv.stride[0]), act, pool is not None), keep, wq, b)
