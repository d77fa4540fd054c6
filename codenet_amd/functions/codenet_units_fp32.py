"""The fp32 ShuffleNetV2 units (layers 1-3) and layer4 in training on the HIP kernels of csrc/codenet_units_fp32_train.hip
(DESIGN.md section 4.3g).

The reference's main.py trains the fp32 model; every unit is a ``BaseNode`` (shufflenetv2_dcn.py:57-114)

    stride 1:  x1 = x[:, :h] (unchanged)                    x2 = x[:, h:]
    stride 2:  y4 = dw3x3_s2(x, W4)   z4 = bn4(y4)          y5 = pw(z4, W5)   x1 = relu(bn5(y5))     x2 = x
    both:      y1 = pw(x2, W1)        a1 = relu(bn1(y1))    y2 = dw3x3_s(a1, W2)   z2 = bn2(y2)
               y3 = pw(z2, W3)        out[:, 2j] = x1[:, j],  out[:, 2j+1] = relu(bn3(y3))[:, j]

8 (stride 1) or 13 (stride 2) framework modules plus ``cat`` and ``channel_shuffle`` under autograd.  Here one
``CodenetUnitFp32Function`` per unit:

    forward   [stride 2: cdn_codenet_unit_fp32_dw_forward (dw4 on x as it is), cdn_codenet_head_fp32_bn_stats,
              cdn_codenet_unit_fp32_bn_forward (z4), cdn_codenet_pointwise_forward (y5), cdn_codenet_head_fp32_bn_stats,
              cdn_codenet_unit_fp32_join_forward (slot 0)]
              cdn_codenet_pointwise_forward_pitched (y1 from the channel slice in place), cdn_codenet_head_fp32_bn_stats,
              cdn_codenet_unit_fp32_dw_forward (y2, a1 formed on load, never written), cdn_codenet_head_fp32_bn_stats,
              cdn_codenet_unit_fp32_bn_forward (z2), cdn_codenet_pointwise_forward (y3), cdn_codenet_head_fp32_bn_stats,
              cdn_codenet_unit_fp32_join_forward (slot 1 + the pass-through half)
    backward  per branch: cdn_codenet_unit_fp32_join_backward (g_z3 / 5, BatchNorm3 / 5's sums, the pass-through half of
              grad_x), cdn_codenet_head_fp32_bn_backward2 (grad y3 / y5), cdn_codenet_pointwise_wgrad (grad W3 / W5),
              cdn_codenet_pointwise_forward on the transposed weights (grad z2 / z4), cdn_codenet_unit_fp32_bn_backward_sums
              (BatchNorm2 / 4's sums), cdn_codenet_unit_fp32_dw_backward (grad y2 / y4 formed on load; branch 2: g_z1, grad W2,
              BatchNorm1's sums; branch 1: grad W4, its grad_x ADDED to branch 2's), and for branch 2
              cdn_codenet_head_fp32_bn_backward2 (grad y1), cdn_codenet_pointwise_wgrad_pitched (grad W1),
              cdn_codenet_pointwise_forward_pitched on W1^T into grad_x's slice

layer4 (Conv2d 1x1 -> BatchNorm2d -> ReLU) is the pointwise kernel under ``PointwiseRangeFunction`` and
``codenet_bn.BnReluUpsample`` with up = 1.  Each BatchNorm follows its own ``training`` flag.  Every floating-point sum has
one order, nothing allocates outside the caching allocator, the step is capturable.
"""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N_
from .. import ops
from . import codenet_stage as CS
from ._fp32_common import (_bn_reason, _hook_reason, _input_reason, _is_1x1, _is_dw, _one_value_error, _out_hw,
                           _placement_reason, bn_backward2, bn_stats)
from .codenet_bn import BnReluUpsample
from .codenet_units import PointwiseRangeFunction, _pointwise, _transposed

# A/B switch (tools/units_fp32_bench.py): the fp32 units and layer4 of a training step on the kernels above (True) or module
# by module through the framework's autograd (False)
NATIVE_FP32_UNITS = True

_p = CS._p


def _ws(Nb, C, H, W, device):
    return CS._workspace(N_.lib().cdn_codenet_unit_fp32_workspace_bytes(Nb, C, H, W), device)


def _dw_forward(in_ptr, in_pitch, st, gamma, beta, w, Nb, C, H, W, stride, like):
    """dw3x3 at `stride` of relu(bn(in)) (st = (mean, var, invstd) of the BatchNorm in front) or of `in` as it is (st None)."""
    Ho, Wo = _out_hw(H, W, stride)
    y = like.new_empty(Nb, C, Ho, Wo)
    bn = (_p(st[0]), _p(st[2]), _p(gamma), _p(beta)) if st is not None else (None,) * 4
    rc = N_.lib().cdn_codenet_unit_fp32_dw_forward(in_ptr, in_pitch, *bn, _p(w), _p(y), Nb, C, H, W, stride, ops._stream(like))
    N_.check(rc, "cdn_codenet_unit_fp32_dw_forward")
    return y


def _bn_forward(y, st, gamma, beta):
    z = torch.empty_like(y)
    rc = N_.lib().cdn_codenet_unit_fp32_bn_forward(_p(y), _p(st[0]), _p(st[2]), _p(gamma), _p(beta), _p(z), *y.shape,
                                                   ops._stream(y))
    N_.check(rc, "cdn_codenet_unit_fp32_bn_forward")
    return z


def _join(y, st, gamma, beta, out, slot, x1=None):
    Nb, h, Ho, Wo = y.shape
    rc = N_.lib().cdn_codenet_unit_fp32_join_forward(_p(y), _p(st[0]), _p(st[2]), _p(gamma), _p(beta), _p(out), slot,
                                                     x1[0] if x1 else None, x1[1] if x1 else 0, Nb, h, Ho, Wo, ops._stream(y))
    N_.check(rc, "cdn_codenet_unit_fp32_join_forward")


def _join_backward(gout, y, st, gamma, beta, slot, gx1=None):
    """(g_z, grad_gamma, grad_beta, means [2, h] = (mb, mg)) of the BatchNorm + ReLU in front of `out`'s slot."""
    Nb, h, Ho, Wo = y.shape
    gz = torch.empty_like(y)
    gg, gb, means = y.new_empty(h), y.new_empty(h), y.new_empty(2, h)
    ws = _ws(Nb, h, Ho, Wo, y.device)
    rc = N_.lib().cdn_codenet_unit_fp32_join_backward(
        _p(gout), _p(y), _p(st[0]), _p(st[2]), _p(gamma), _p(beta), _p(gz), _p(gg), _p(gb), _p(means[0]), _p(means[1]), slot,
        gx1[0] if gx1 else None, gx1[1] if gx1 else 0, Nb, h, Ho, Wo, _p(ws), ws.numel() * 4, ops._stream(y))
    N_.check(rc, "cdn_codenet_unit_fp32_join_backward")
    return gz, gg, gb, means


def _bn_backward_sums(gz, y, st):
    """(grad_gamma, grad_beta, means [2, C]) of a BatchNorm without ReLU: g_z is the incoming gradient itself."""
    Nb, C, H, W = y.shape
    gg, gb, means = y.new_empty(C), y.new_empty(C), y.new_empty(2, C)
    ws = _ws(Nb, C, H, W, y.device)
    rc = N_.lib().cdn_codenet_unit_fp32_bn_backward_sums(_p(gz), _p(y), _p(st[0]), _p(st[2]), _p(gg), _p(gb), _p(means[0]),
                                                         _p(means[1]), Nb, C, H, W, _p(ws), ws.numel() * 4, ops._stream(y))
    N_.check(rc, "cdn_codenet_unit_fp32_bn_backward_sums")
    return gg, gb, means


def _dw_backward(gz, y, st2, gamma2, means2, training2, in_ptr, in_pitch, st1, gamma1, beta1, w, gin, accumulate, Nb, C, H, W,
                 stride):
    """Branch 2 (st1 given): (grad_w, grad_gamma1, grad_beta1, means1), g_z1 through gin = (pointer, image pitch).
    Branch 1 (st1 None): (grad_w, None, None, None), grad_in through gin (or None), added where `accumulate`."""
    gw = torch.empty_like(w)
    gg = gb = means = None
    bn1 = (None,) * 4
    res = (None,) * 4
    if st1 is not None:
        gg, gb, means = y.new_empty(C), y.new_empty(C), y.new_empty(2, C)
        bn1 = (_p(st1[0]), _p(st1[2]), _p(gamma1), _p(beta1))
        res = (_p(gg), _p(gb), _p(means[0]), _p(means[1]))
    ws = _ws(Nb, C, H, W, y.device)
    rc = N_.lib().cdn_codenet_unit_fp32_dw_backward(
        _p(gz), _p(y), _p(st2[0]), _p(st2[2]), _p(gamma2), _p(means2[0]), _p(means2[1]), int(bool(training2)), in_ptr,
        in_pitch, *bn1, _p(w), gin[0] if gin else None, gin[1] if gin else 0, int(bool(accumulate)), _p(gw), *res, Nb, C, H,
        W, stride, _p(ws), ws.numel() * 4, ops._stream(y))
    N_.check(rc, "cdn_codenet_unit_fp32_dw_backward")
    return gw, gg, gb, means


class CodenetUnitFp32Function(Function):
    """out = unit(x).  meta = (stride, (bn1, bn2, bn3[, bn4, bn5])), the nn.BatchNorm2d modules; flat: W, gamma, beta of
    conv / BatchNorm 1, 2, 3 (stride 2: + 4, 5).  The BatchNorm buffers are updated in place by the forward, as the module
    path does.  keep (a dict or None) receives x, y1, y2, z2, y3 (+ y4, z4, y5), out and "bn1" .. "bn5" = (mean, var,
    invstd) from the forward and, from the backward, g_z3, grad_y3, grad_z2, g_z1, grad_y1 (+ g_z5, grad_y5, grad_z4),
    "means1" .. "means5" = (mb, mg), grad_x and, stride 2, grad_x_b2: a copy of grad_x before branch 1 added to it."""

    @staticmethod
    def forward(ctx, x, meta, keep, *flat):
        ops._gpu_f32(x, *flat)
        ctx.set_materialize_grads(False)
        stride, bns = meta
        Nb, Cx, H, W = x.shape
        flat = [t.contiguous() for t in flat]
        w1, g1, b1, w2, g2, b2, w3, g3, b3 = flat[:9]
        h = w1.shape[0]
        Ho, Wo = _out_hw(H, W, stride)
        out = x.new_empty(Nb, 2 * h, Ho, Wo)
        pitch = Cx * H * W
        branch1 = ()
        if stride == 2:
            w4, g4, b4, w5, g5, b5 = flat[9:15]
            y4 = _dw_forward(x.data_ptr(), pitch, None, None, None, w4, Nb, Cx, H, W, 2, x)
            st4 = bn_stats(y4, bns[3])
            z4 = _bn_forward(y4, st4, g4, b4)
            y5 = ops.codenet_pointwise(z4, w5)
            st5 = bn_stats(y5, bns[4])
            _join(y5, st5, g5, b5, out, 0)
            branch1 = (y4, z4, y5, st4, st5, w4, g4, w5, g5, b5)
            x2_ptr, C2 = x.data_ptr(), Cx
        else:
            x2_ptr, C2 = x.data_ptr() + 4 * h * H * W, Cx - h
        y1, _ = _pointwise(x2_ptr, pitch, None, w1, None, Nb, C2, H, W, False, x)
        st1 = bn_stats(y1, bns[0])
        y2 = _dw_forward(y1.data_ptr(), h * H * W, st1, g1, b1, w2, Nb, h, H, W, stride, x)
        st2 = bn_stats(y2, bns[1])
        z2 = _bn_forward(y2, st2, g2, b2)
        y3 = ops.codenet_pointwise(z2, w3)
        st3 = bn_stats(y3, bns[2])
        _join(y3, st3, g3, b3, out, 1, (x.data_ptr(), pitch) if stride == 1 else None)
        if keep is not None:
            keep.update(x=x, y1=y1, y2=y2, z2=z2, y3=y3, out=out, bn1=tuple(st1), bn2=tuple(st2), bn3=tuple(st3))
            if stride == 2:
                keep.update(y4=y4, z4=z4, y5=y5, bn4=tuple(st4), bn5=tuple(st5))
        ctx.stride, ctx.keep = stride, keep
        ctx.modes = tuple(bool(bn.training) for bn in bns)
        ctx.save_for_backward(x, y1, y2, z2, y3, st1, st2, st3, w1, g1, b1, w2, g2, w3, g3, b3, *branch1)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        saved = ctx.saved_tensors
        x, y1, y2, z2, y3, st1, st2, st3, w1, g1, b1, w2, g2, w3, g3, b3 = saved[:16]
        stride, keep, modes = ctx.stride, ctx.keep, ctx.modes
        need = ctx.needs_input_grad
        grads = [None] * (3 + (15 if stride == 2 else 9))
        if gout is None:
            return tuple(grads)
        gout = gout.contiguous()
        Nb, Cx, H, W = x.shape
        h = w1.shape[0]
        Ho, Wo = y3.shape[2], y3.shape[3]
        pitch = Cx * H * W
        gx = torch.empty_like(x) if need[0] else None
        # ---- branch 2 (and the pass-through half of a stride-1 unit)
        gz3, gg3, gb3, means3 = _join_backward(gout, y3, st3, g3, b3, 1,
                                               (gx.data_ptr(), pitch) if (stride == 1 and gx is not None) else None)
        gy3 = torch.empty_like(y3)
        bn_backward2(gz3, y3, st3, g3, means3, modes[2], gy3, 0, h * Ho * Wo)
        gw3, _ = CS.pointwise_wgrad(gy3, z2, False)
        gz2 = ops.codenet_pointwise(gy3, _transposed(w3))
        gg2, gb2, means2 = _bn_backward_sums(gz2, y2, st2)
        gz1 = torch.empty_like(y1)
        gw2, gg1, gb1, means1 = _dw_backward(gz2, y2, st2, g2, means2, modes[1], y1.data_ptr(), h * H * W, st1, g1, b1, w2,
                                             (gz1.data_ptr(), h * H * W), False, Nb, h, H, W, stride)
        gy1 = torch.empty_like(y1)
        bn_backward2(gz1, y1, st1, g1, means1, modes[0], gy1, 0, h * H * W)
        off, C2 = (0, Cx) if stride == 2 else (h, Cx - h)
        lib = N_.lib()
        ws = CS._workspace(lib.cdn_codenet_pointwise_wgrad_workspace_bytes(Nb, C2, h, H * W), x.device)
        gw1 = x.new_empty(h, C2)
        rc = lib.cdn_codenet_pointwise_wgrad_pitched(_p(gy1), x.data_ptr() + 4 * off * H * W, pitch, _p(gw1), None, Nb, C2, h,
                                                     H * W, _p(ws), ws.numel() * 4, ops._stream(x))
        N_.check(rc, "cdn_codenet_pointwise_wgrad_pitched")
        if gx is not None:
            _pointwise(gy1.data_ptr(), h * H * W, None, _transposed(w1), None, Nb, h, H, W, False, x,
                       out=(gx.data_ptr() + 4 * off * H * W, pitch))
        grads[3:12] = [gw1.view_as(w1), gg1, gb1, gw2, gg2, gb2, gw3.view_as(w3), gg3, gb3]
        if keep is not None:
            keep.update(g_z3=gz3, grad_y3=gy3, grad_z2=gz2, g_z1=gz1, grad_y1=gy1, means1=means1, means2=means2,
                        means3=means3)
        # ---- branch 1 of a stride-2 unit: its grad_x is ADDED to branch 2's by the thread that owns the pixel
        if stride == 2:
            y4, z4, y5, st4, st5, w4, g4, w5, g5, b5 = saved[16:26]
            if keep is not None and gx is not None:
                keep["grad_x_b2"] = gx.clone()
            gz5, gg5, gb5, means5 = _join_backward(gout, y5, st5, g5, b5, 0)
            gy5 = torch.empty_like(y5)
            bn_backward2(gz5, y5, st5, g5, means5, modes[4], gy5, 0, h * Ho * Wo)
            gw5, _ = CS.pointwise_wgrad(gy5, z4, False)
            gz4 = ops.codenet_pointwise(gy5, _transposed(w5))
            gg4, gb4, means4 = _bn_backward_sums(gz4, y4, st4)
            gw4, _, _, _ = _dw_backward(gz4, y4, st4, g4, means4, modes[3], x.data_ptr(), pitch, None, None, None, w4,
                                        (gx.data_ptr(), pitch) if gx is not None else None, True, Nb, Cx, H, W, 2)
            grads[12:18] = [gw4, gg4, gb4, gw5.view_as(w5), gg5, gb5]
            if keep is not None:
                keep.update(g_z5=gz5, grad_y5=gy5, grad_z4=gz4, means4=means4, means5=means5)
        if keep is not None:
            keep["grad_x"] = gx
        grads[0] = gx
        return tuple(g if n else None for g, n in zip(grads, need))


def _unit_modules(node):
    """((conv, bn) pairs 1, 2, 3[, 4, 5]) of a BaseNode whose branches have the reference's layout, else None."""
    b2 = getattr(node, "b2", None)
    if not isinstance(b2, nn.Sequential) or len(b2) != 8 or not (isinstance(b2[2], nn.ReLU) and isinstance(b2[7], nn.ReLU)):
        return None
    pairs = [(b2[0], b2[1]), (b2[3], b2[4]), (b2[5], b2[6])]
    if node.stride == 2:
        b1 = getattr(node, "b1", None)
        if not isinstance(b1, nn.Sequential) or len(b1) != 5 or not isinstance(b1[4], nn.ReLU):
            return None
        pairs += [(b1[0], b1[1]), (b1[2], b1[3])]
    return pairs


def _node_reason(node, what):
    from ..harness import BaseNode
    if type(node) is not BaseNode:
        return "%s is a %s, not a BaseNode" % (what, type(node).__name__)
    why = _hook_reason(node, what)
    if why is not None:
        return why
    if node.stride not in (1, 2):
        return "%s: stride %s, the units have stride 1 or 2" % (what, node.stride)
    pairs = _unit_modules(node)
    if pairs is None:
        return "%s: not the units' own layout (Conv2d 1x1, BatchNorm2d, ReLU, depthwise Conv2d 3x3, BatchNorm2d, Conv2d " \
               "1x1, BatchNorm2d, ReLU)" % what
    for conv, _ in pairs:
        if type(conv) is not nn.Conv2d:
            return "%s: a convolution is a %s, not a Conv2d (the deform=True units keep the module path)" % (
                what, type(conv).__name__)
    c1, c2, c3 = pairs[0][0], pairs[1][0], pairs[2][0]
    h = c1.out_channels
    ok = (_is_1x1(c1) and _is_1x1(c3) and _is_dw(c2, node.stride) and c2.in_channels == h and c3.in_channels == h
          and c3.out_channels == h and (node.stride == 2 or c1.in_channels == h)
          and all(getattr(c, "padding_mode", "zeros") == "zeros" for c in (c1, c3)))
    if ok and node.stride == 2:
        c4, c5 = pairs[3][0], pairs[4][0]
        ok = (_is_dw(c4, 2) and c4.in_channels == c1.in_channels and _is_1x1(c5) and c5.in_channels == c4.out_channels
              and c5.out_channels == h and getattr(c5, "padding_mode", "zeros") == "zeros")
    if not ok:
        return "%s: not the units' own geometry (1x1 -> depthwise 3x3, zero padding 1 -> 1x1)" % what
    for i, (conv, bn) in enumerate(pairs):
        if conv.bias is not None:
            return "%s: convolution %d has a bias (the reference's have none)" % (what, i + 1)
        why = _bn_reason(bn, conv.out_channels, "%s: BatchNorm2d %d" % (what, i + 1))
        if why is not None:
            return why
    return None


def _is_fp32_layer4(mod):
    return (isinstance(mod, nn.Sequential) and len(mod) == 3 and type(mod[0]) is nn.Conv2d
            and isinstance(mod[2], nn.ReLU))


def _layer4_reason(layer4):
    why = _hook_reason(layer4, "layer4")
    if why is not None:
        return why
    conv, bn = layer4[0], layer4[1]
    if not _is_1x1(conv) or getattr(conv, "padding_mode", "zeros") != "zeros":
        return "layer4: not a 1x1 convolution"
    if conv.bias is not None:
        return "layer4: its convolution has a bias (the reference's has none)"
    return _bn_reason(bn, conv.out_channels, "layer4: its BatchNorm2d")


def _nodes_of(node_or_layer):
    from ..harness import BaseNode
    if isinstance(node_or_layer, BaseNode):
        return [node_or_layer]
    if isinstance(node_or_layer, nn.Sequential) and len(node_or_layer) and not _is_fp32_layer4(node_or_layer):
        return list(node_or_layer)
    return None


def native_reason(node_or_layer, x):
    """None when forward_fp32_units / forward_fp32_layer4 run `node_or_layer` (a harness.BaseNode, a Sequential of them, or
    the fp32 layer4) on the kernels for the input x, else the reason -- a string -- why it takes the module path.  x None:
    the modules alone are judged (their structure and settings, not where the model lives):
    pipeline.GraphedTrainStep.is_fp32_trunk."""
    if not NATIVE_FP32_UNITS:
        return "NATIVE_FP32_UNITS is off"
    if not torch.is_grad_enabled():
        return "grad mode is off (inference has pipeline.FusedBackbone)"
    layer4 = _is_fp32_layer4(node_or_layer)
    if layer4:
        why = _layer4_reason(node_or_layer)
        if why is not None:
            return why
        cin, widest = node_or_layer[0].in_channels, node_or_layer[0].out_channels
    else:
        nodes = _nodes_of(node_or_layer)
        if nodes is None:
            return "a %s is neither a BaseNode, a Sequential of them nor the fp32 layer4" % type(node_or_layer).__name__
        if len(nodes) > 1 or nodes[0] is not node_or_layer:
            why = _hook_reason(node_or_layer, "the layer")
            if why is not None:
                return why
        for i, node in enumerate(nodes):
            why = _node_reason(node, "unit %d" % i)
            if why is not None:
                return why
        c1 = nodes[0].b2[0]
        cin = c1.in_channels if nodes[0].stride == 2 else 2 * c1.out_channels
        widest = max(2 * n.b2[0].out_channels for n in nodes)
    if x is None:
        return None
    why = _input_reason(x, widest, channels=cin, aligned=True)
    if why is not None:
        return why
    return _placement_reason(x, node_or_layer.parameters(), node_or_layer.buffers())


def forward_fp32_units(layer, x, keep=None):
    """``layer(x)`` for an fp32 layer of the backbone (a Sequential of BaseNode, or one node) that native_reason(layer, x)
    accepts: every unit one CodenetUnitFp32Function.  keep (tests): a dict that receives {unit index: the unit's own
    intermediates}."""
    nodes = _nodes_of(layer)
    Nb, _, H, W = x.shape
    for node in nodes:      # the framework's error for one value per channel, before any launch
        pairs = _unit_modules(node)
        Ho, Wo = _out_hw(H, W, node.stride)
        for i, (conv, bn) in enumerate(pairs):
            n = Nb * H * W if i == 0 else Nb * Ho * Wo
            if bn.training and n == 1:
                raise _one_value_error((Nb, conv.out_channels) + ((H, W) if i == 0 else (Ho, Wo)))
        H, W = Ho, Wo
    for i, node in enumerate(nodes):
        k = None
        if keep is not None:
            k = keep[i] = {}
        pairs = _unit_modules(node)
        flat = []
        for conv, bn in pairs:
            flat += [conv.weight, bn.weight, bn.bias]
        x = CodenetUnitFp32Function.apply(x, (int(node.stride), tuple(bn for _, bn in pairs)), k, *flat)
    return x


def forward_fp32_layer4(layer4, x):
    """``layer4(x)`` for the fp32 layer4 (Conv2d 1x1 -> BatchNorm2d -> ReLU) that native_reason(layer4, x) accepts: the
    pointwise kernel and cdn_codenet_bn_relu_up_forward / backward with up = 1."""
    conv, bn = layer4[0], layer4[1]
    Nb, _, H, W = x.shape
    if bn.training and Nb * H * W == 1:
        raise _one_value_error((Nb, conv.out_channels, H, W))
    y, _ = PointwiseRangeFunction.apply(x, conv.weight, None, False)
    return BnReluUpsample.apply(y, bn.weight, bn.bias, bn, 1)[0]
