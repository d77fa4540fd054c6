"""The quantised ShuffleNetV2 units (layers 1-3) and layer4 as autograd functions on the HIP kernels (training path).

The reference runs every unit (``QuantBaseNode``, quant_modules.py:809-907) module by module under autograd:

    stride 1:  x1 = x[:, :h]  (passes through unchanged)      x2 = x[:, h:]
    stride 2:  x1 = act( relu( pw5( act4( dw4_s2(x) ) ) ) )   x2 = x
    both:      x2 = act( relu( pw3( act2( dw2_s( act1( relu( pw1(x2) ) ) ) ) ) ) )
               y[:, 2j] = x1[:, j],  y[:, 2j+1] = x2[:, j]      (cat + channel_shuffle(., 2))

``act`` is ONE QuantAct shared by every unit of a layer, updated once per application in program order: a stride-2 unit
updates it twice (branch 1, then branch 2) and each branch is quantised with the state after ITS OWN update.  Here one
``CodenetUnitFunction`` per unit:

    forward   [stride 2: cdn_codenet_unit_dw_forward (dw4 on x as it is, act4 updated by the launch's last workgroup),
              cdn_codenet_pointwise_forward_range (pw5, y4 fake-quantised on load), cdn_codenet_head_act_update (act, on
              max(y5, 0)), cdn_codenet_unit_join_forward (slot 0)]
              cdn_codenet_pointwise_forward_pitched (pw1 on the channel slice in place), cdn_codenet_head_act_update (act1),
              cdn_codenet_unit_dw_forward (dw2 with fq1(relu(.)) on load, act2 updated), cdn_codenet_pointwise_forward_range
              (pw3), cdn_codenet_head_act_update (act), cdn_codenet_unit_join_forward (slot 1 + the pass-through half)
    backward  cdn_codenet_unit_join_backward, cdn_codenet_pointwise_wgrad_q (pw3 / pw5), cdn_codenet_pointwise_forward on the
              transposed weights (data gradient), cdn_codenet_unit_dw_backward (grad y1 / grad x, grad W, b in fixed order),
              cdn_codenet_pointwise_wgrad_pitched (pw1), cdn_codenet_pointwise_forward_pitched on W1q^T into grad_x's slice

The dense 1x1 convolutions run on the f32-MFMA forms (pointwise_kernel, pw_wgrad_kernel; the exact-product bf16 weight
gradient where y2 / y4 come with a QuantAct state and the tiles are whole): the int8 / bf16-split forms take no image pitch.
Straight-through quantisers, ReLU masks y > 0.  The weight transformations (BN fold, fake-quantisation) stay the native
autograd functions of codenet_stage.py.  Every floating-point sum has one order, nothing allocates outside the caching
allocator, the step is capturable.
"""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N_
from .. import ops
from . import codenet_stage as CS
from ._qat_common import (_act_reason, _act_update, _fold_all, _hook_reason, _input_reason, _is_1x1, _is_dw,
                          _placement_reason, _relu_act_reason, _tracked_act, _weight_prep_structural)

# A/B switch (tools/units_train_bench.py): the units of a QAT step on the kernels above (True) or module by module through
# the framework's autograd (False)
NATIVE_UNITS = True

_p = CS._p


def _pointwise(d_ptr, d_pitch, d_state, w, b, Nb, C, H, W, want_range, like, out=None):
    """y = conv1x1(d; C -> Co) + b with d (and, out = (pointer, image pitch), y) addressed through an image pitch:
    (y or None, {min, max} pairs or None)."""
    lib = N_.lib()
    w2 = w.view(w.shape[0], -1)
    Co = w2.shape[0]
    y = None
    if out is None:
        y = like.new_empty(Nb, Co, H, W)
        out = (y.data_ptr(), Co * H * W)
    part = ops._partials(lib.cdn_codenet_pointwise_range_partials(Nb, Co, H * W), like) if want_range else None
    rc = lib.cdn_codenet_pointwise_forward_pitched(d_ptr, d_pitch, _p(d_state), _p(w2), _p(b), out[0], out[1], Nb, C, Co,
                                                   H * W, 0, _p(part), ops._stream(like))
    N_.check(rc, "cdn_codenet_pointwise_forward_pitched")
    return y, part


def _dw_forward(in_ptr, in_pitch, in_state, w, b, Nb, C, H, W, stride, act, like):
    """The raw depthwise output (stored before quantisation) and the snapshot of the state of the QuantAct behind it."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = like.new_empty(Nb, C, Ho, Wo)
    snap, upd = _tracked_act(act, like.device)
    rc = N_.lib().cdn_codenet_unit_dw_forward(in_ptr, in_pitch, _p(in_state), _p(w), _p(b), _p(y), Nb, C, H, W, stride, *upd,
                                              ops._stream(like))
    N_.check(rc, "cdn_codenet_unit_dw_forward")
    return y, snap


def _dw_backward(g, in_ptr, in_pitch, in_state, w, gin, accumulate, Nb, C, H, W, stride):
    """grad_in through gin = (pointer, image pitch) or None; returns (grad_w, grad_b)."""
    lib = N_.lib()
    gw, gb = torch.empty_like(w), g.new_empty(C)
    ws = CS._workspace(lib.cdn_codenet_unit_dw_backward_workspace_bytes(Nb, C, H, W, stride), g.device)
    rc = lib.cdn_codenet_unit_dw_backward(_p(g), in_ptr, in_pitch, _p(in_state), _p(w), gin[0] if gin else None,
                                          gin[1] if gin else 0, int(bool(accumulate)), _p(gw), _p(gb), Nb, C, H, W, stride,
                                          _p(ws), ws.numel() * 4, ops._stream(g))
    N_.check(rc, "cdn_codenet_unit_dw_backward")
    return gw, gb


def _join(y3, snap, out, slot, x1=None):
    Nb, h, Ho, Wo = y3.shape
    rc = N_.lib().cdn_codenet_unit_join_forward(_p(y3), _p(snap), _p(out), slot, x1[0] if x1 else None, x1[1] if x1 else 0,
                                                Nb, h, Ho * Wo, ops._stream(y3))
    N_.check(rc, "cdn_codenet_unit_join_forward")


def _join_backward(gout, y3, slot, gx1=None):
    Nb, h, Ho, Wo = y3.shape
    gy3 = torch.empty_like(y3)
    rc = N_.lib().cdn_codenet_unit_join_backward(_p(gout), _p(y3), _p(gy3), slot, gx1[0] if gx1 else None,
                                                 gx1[1] if gx1 else 0, Nb, h, Ho * Wo, ops._stream(y3))
    N_.check(rc, "cdn_codenet_unit_join_backward")
    return gy3


def _transposed(w):
    co = w.shape[0]
    w2 = w.reshape(co, -1)
    return w2.t().contiguous().view(w2.shape[1], co, 1, 1)


class CodenetUnitFunction(Function):
    """y = unit(x).  meta = (stride, act1, act2, act, act4 or None); flat: W1q, b1, W2q, b2, W3q, b3 (stride 2: + W4q, b4,
    W5q, b5), already folded / fake-quantised.  The QuantAct buffers are updated in place by the forward, in the
    reference's order, as the module path does.  keep (a dict or None) receives the saved tensors themselves."""

    @staticmethod
    def forward(ctx, x, meta, keep, *flat):
        ops._gpu_f32(x, *flat)
        ctx.set_materialize_grads(False)
        stride, act1, act2, act, act4 = meta
        Nb, Cx, H, W = x.shape
        flat = [t.contiguous() for t in flat]
        w1, b1, w2, b2, w3, b3 = flat[:6]
        h = w1.shape[0]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        out = x.new_empty(Nb, 2 * h, Ho, Wo)
        pitch = Cx * H * W
        y4 = y5 = snap4 = snap_a = None
        if stride == 2:
            w4, b4, w5, b5 = flat[6:10]
            y4, snap4 = _dw_forward(x.data_ptr(), pitch, None, w4, b4, Nb, Cx, H, W, 2, act4, x)
            y5, part = _pointwise(y4.data_ptr(), Cx * Ho * Wo, snap4, w5, b5, Nb, Cx, Ho, Wo, bool(act.running_stat), x)
            snap_a = _act_update(act, part, True)      # the shared act's FIRST update of this unit: branch 1
            _join(y5, snap_a, out, 0)
            x2_ptr, C2 = x.data_ptr(), Cx
        else:
            x2_ptr, C2 = x.data_ptr() + 4 * h * H * W, Cx - h
        y1, part = _pointwise(x2_ptr, pitch, None, w1, b1, Nb, C2, H, W, bool(act1.running_stat), x)
        snap1 = _act_update(act1, part, True)
        y2, snap2 = _dw_forward(y1.data_ptr(), h * H * W, snap1, w2, b2, Nb, h, H, W, stride, act2, x)
        y3, part = _pointwise(y2.data_ptr(), h * Ho * Wo, snap2, w3, b3, Nb, h, Ho, Wo, bool(act.running_stat), x)
        snap_b = _act_update(act, part, True)
        _join(y3, snap_b, out, 1, (x.data_ptr(), pitch) if stride == 1 else None)
        if keep is not None:
            keep.update(x=x, y1=y1, y2=y2, y3=y3, y4=y4, y5=y5, snap1=snap1, snap2=snap2, snap4=snap4, snap_a=snap_a,
                        snap_b=snap_b, out=out)
        ctx.stride = stride
        ctx.save_for_backward(x, y1, y2, y3, snap1, snap2, w1, w2, w3,
                              *((y4, y5, snap4, flat[6], flat[8]) if stride == 2 else ()))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        saved = ctx.saved_tensors
        x, y1, y2, y3, snap1, snap2, w1, w2, w3 = saved[:9]
        stride = ctx.stride
        need = ctx.needs_input_grad
        grads = [None] * (3 + (10 if stride == 2 else 6))
        if gout is None:
            return tuple(grads)
        gout = gout.contiguous()
        Nb, Cx, H, W = x.shape
        h = w1.shape[0]
        Ho, Wo = y3.shape[2], y3.shape[3]
        pitch = Cx * H * W
        gx = torch.empty_like(x) if need[0] else None
        # ---- branch 2 (and the pass-through half of a stride-1 unit)
        gy3 = _join_backward(gout, y3, 1, (gx.data_ptr(), pitch) if (stride == 1 and gx is not None) else None)
        gw3, gb3 = CS.pointwise_wgrad(gy3, y2, True, d_state=snap2)
        g2 = ops.codenet_pointwise(gy3, _transposed(w3))
        gy1 = torch.empty_like(y1)
        gw2, gb2 = _dw_backward(g2, y1.data_ptr(), h * H * W, snap1, w2, (gy1.data_ptr(), h * H * W), False, Nb, h, H, W,
                                stride)
        off, C2 = (0, Cx) if stride == 2 else (h, Cx - h)
        lib = N_.lib()
        ws = CS._workspace(lib.cdn_codenet_pointwise_wgrad_workspace_bytes(Nb, C2, h, H * W), x.device)
        gw1, gb1 = x.new_empty(h, C2), x.new_empty(h)
        rc = lib.cdn_codenet_pointwise_wgrad_pitched(_p(gy1), x.data_ptr() + 4 * off * H * W, pitch, _p(gw1), _p(gb1), Nb, C2,
                                                     h, H * W, _p(ws), ws.numel() * 4, ops._stream(x))
        N_.check(rc, "cdn_codenet_pointwise_wgrad_pitched")
        if gx is not None:
            _pointwise(gy1.data_ptr(), h * H * W, None, _transposed(w1), None, Nb, h, H, W, False, x,
                       out=(gx.data_ptr() + 4 * off * H * W, pitch))
        grads[3:9] = [gw1.view_as(w1), gb1, gw2, gb2, gw3.view_as(w3), gb3]
        # ---- branch 1 of a stride-2 unit: its grad_x is ADDED to branch 2's by the thread that owns the pixel
        if stride == 2:
            y4, y5, snap4, w4, w5 = saved[9:14]
            gy5 = _join_backward(gout, y5, 0)
            gw5, gb5 = CS.pointwise_wgrad(gy5, y4, True, d_state=snap4)
            g4 = ops.codenet_pointwise(gy5, _transposed(w5))
            gw4, gb4 = _dw_backward(g4, x.data_ptr(), pitch, None, w4, (gx.data_ptr(), pitch) if gx is not None else None,
                                    True, Nb, Cx, H, W, 2)
            grads[9:13] = [gw4, gb4, gw5.view_as(w5), gb5]
        grads[0] = gx
        return tuple(grads)


class PointwiseRangeFunction(Function):
    """(y, {min, max} pairs of y) = conv1x1(x, Wq) + b on the f32-MFMA pointwise kernel -- layer4's convolution; backward:
    cdn_codenet_pointwise_wgrad and the same kernel on the transposed weights."""

    @staticmethod
    def forward(ctx, x, w, b, want_range):
        ops._gpu_f32(x, w, b)
        ctx.set_materialize_grads(False)
        x, w = x.contiguous(), w.contiguous()
        if want_range:
            y, part = ops.codenet_pointwise(x, w, b, want_range=True)
        else:
            y, part = ops.codenet_pointwise(x, w, b), x.new_zeros(0, 2)
        ctx.has_b = b is not None
        ctx.save_for_backward(x, w)
        ctx.mark_non_differentiable(part)
        return y, part

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, *unused):
        x, w = ctx.saved_tensors
        need = ctx.needs_input_grad
        if gy is None:
            return None, None, None, None
        gy = gy.contiguous()
        gw = gb = gx = None
        if need[1] or (need[2] and ctx.has_b):
            gw, gb = CS.pointwise_wgrad(gy, x, need[2] and ctx.has_b)
            gw = gw.view_as(w) if need[1] else None
        if need[0]:
            gx = ops.codenet_pointwise(gy, _transposed(w))
        return gx, gw, gb, None


def _node_convbns(node):
    cbs = [node.quant_convbn1, node.quant_convbn2, node.quant_convbn3]
    if node.stride == 2:
        cbs += [node.quant_convbn4, node.quant_convbn5]
    return cbs


def _node_reason(node, what):
    from ..portable_quantizer.quant_modules import QuantBaseNode
    if type(node) is not QuantBaseNode:
        return "%s is a %s, not a QuantBaseNode (the fp32 and the deformable units keep the module path)" % (
            what, type(node).__name__)
    why = _hook_reason(node, what)
    if why is not None:
        return why
    if node.stride not in (1, 2) or getattr(node, "quant_act", None) is None:
        return "%s: not the units' own geometry (stride 1 or 2 with a shared QuantAct)" % what
    acts = [("quant_act1", node.quant_act1), ("quant_act2", node.quant_act2), ("quant_act", node.quant_act)]
    if node.stride == 2:
        acts.append(("quant_act4", node.quant_act4))
    for name, act in acts:
        why = _act_reason(act, "%s: %s" % (what, name))
        if why is not None:
            return why
    c1, c2, c3 = node.quant_convbn1.conv, node.quant_convbn2.conv, node.quant_convbn3.conv
    h = c1.out_channels
    ok = (_is_1x1(c1) and _is_1x1(c3) and _is_dw(c2, node.stride) and c2.in_channels == h and c3.in_channels == h
          and c3.out_channels == h)
    if ok and node.stride == 2:
        c4, c5 = node.quant_convbn4.conv, node.quant_convbn5.conv
        ok = (_is_dw(c4, 2) and c4.in_channels == c1.in_channels and _is_1x1(c5) and c5.in_channels == c4.out_channels
              and c5.out_channels == h)
    if not ok:
        return "%s: not the units' own geometry (1x1 -> depthwise 3x3, zero padding 1 -> 1x1)" % what
    for cb in _node_convbns(node):
        if not _weight_prep_structural(cb.conv.weight, cb):
            return ("%s: a weight quantiser is not on the device weight-prep path (per-channel symmetric <= 4-bit ranks, "
                    "quantising, no bias quantisation)" % what)
        if cb.weight_bit > 4:
            return "%s: a weight quantiser has more than 4 bits" % what
    return None


def _is_layer4(mod):
    from ..portable_quantizer.quant_modules import QuantBnConv2d
    return isinstance(mod, nn.Sequential) and len(mod) == 2 and isinstance(mod[0], QuantBnConv2d)


def _layer4_reason(layer4):
    why = _hook_reason(layer4, "layer4") or _relu_act_reason(layer4[1], "layer4: its second module")
    if why is not None:
        return why
    cb = layer4[0]
    if not _is_1x1(cb.conv):
        return "layer4: not a 1x1 convolution"
    if not _weight_prep_structural(cb.conv.weight, cb) or cb.weight_bit > 4:
        return "layer4: its weight quantiser is not on the device weight-prep path (per-channel symmetric, <= 4 bits)"
    return None


def native_reason(node_or_layer, x):
    """None when forward_units / forward_layer4 run `node_or_layer` (a QuantBaseNode, a Sequential of them, or the quantised
    layer4) on the kernels for the input x, else the reason -- a string -- why it takes the module path.  x None: the
    modules alone are judged (structure and settings, not where the model lives): GraphedTrainStep.is_native_trunk."""
    from ..portable_quantizer.quant_modules import QuantBaseNode
    if not NATIVE_UNITS:
        return "NATIVE_UNITS is off"
    if not torch.is_grad_enabled():
        return "grad mode is off (inference has pipeline.FusedBackbone)"
    layer4 = _is_layer4(node_or_layer)
    if layer4:
        nodes = []
        why = _layer4_reason(node_or_layer)
        if why is not None:
            return why
        cin = node_or_layer[0].conv.in_channels
    else:
        if isinstance(node_or_layer, QuantBaseNode):
            nodes = [node_or_layer]
        elif isinstance(node_or_layer, nn.Sequential) and len(node_or_layer):
            nodes = list(node_or_layer)
            why = _hook_reason(node_or_layer, "the layer")
            if why is not None:
                return why
        else:
            return "a %s is neither a QuantBaseNode nor a Sequential of them" % type(node_or_layer).__name__
        for i, node in enumerate(nodes):
            why = _node_reason(node, "unit %d" % i)
            if why is not None:
                return why
        c = nodes[0].quant_convbn1.conv
        cin = c.in_channels if nodes[0].stride == 2 else 2 * c.out_channels
    if x is None:
        return None
    widest = max([node_or_layer[0].conv.out_channels] if layer4 else [2 * n.quant_convbn1.conv.out_channels for n in nodes])
    why = _input_reason(x, widest, channels=cin, aligned=True)
    if why is not None:
        return why
    cbs = [node_or_layer[0]] if layer4 else [cb for n in nodes for cb in _node_convbns(n)]
    acts = [node_or_layer[1][1]] if layer4 else [a for n in nodes for a in (
        [n.quant_act1, n.quant_act2, n.quant_act] + ([n.quant_act4] if n.stride == 2 else []))]
    return _placement_reason(x, [(cb.conv.weight, cb) for cb in cbs], acts)


def _prepared_weights(node):
    """(W1q, b1, W2q, b2, W3q, b3[, W4q, b4, W5q, b5]): the folds of the unit in one launch where the multi-tensor weight
    prep takes them, else every module's own (native) preparation."""
    return _fold_all(_node_convbns(node))


def _unit_meta(node):
    return (int(node.stride), node.quant_act1, node.quant_act2, node.quant_act,
            node.quant_act4 if node.stride == 2 else None)


def forward_units(layer, x, keep=None):
    """``layer(x)`` for a layer of the backbone (a Sequential of QuantBaseNode, or one node).  In the QAT step on the GPU
    (native_reason(layer, x) is None) every unit runs as one CodenetUnitFunction; an fp32 layer of BaseNode units that
    codenet_units_fp32.native_reason accepts runs as one CodenetUnitFp32Function per unit; otherwise exactly ``layer(x)``.
    keep (tests): a dict that receives {unit index: the native path's own intermediates}."""
    if native_reason(layer, x) is not None:
        from . import codenet_units_fp32 as U32
        if U32.native_reason(layer, x) is None:
            return U32.forward_fp32_units(layer, x, keep)
        return layer(x)
    nodes = list(layer) if isinstance(layer, nn.Sequential) else [layer]
    for i, node in enumerate(nodes):
        k = None
        if keep is not None:
            k = keep[i] = {}
        x = CodenetUnitFunction.apply(x, _unit_meta(node), k, *_prepared_weights(node))
    return x


def forward_layer4(layer4, x):
    """``layer4(x)`` for the quantised layer4 (QuantBnConv2d 1x1 -> ReLU -> QuantAct): in the QAT step on the GPU the
    pointwise kernel (with the {min, max} pairs of its output) and CS.ReluQuant; the fp32 layer4 that
    codenet_units_fp32.native_reason accepts on the pointwise kernel and the fused BatchNorm + ReLU; otherwise exactly
    ``layer4(x)``."""
    if not _is_layer4(layer4) or native_reason(layer4, x) is not None:
        from . import codenet_units_fp32 as U32
        if U32.native_reason(layer4, x) is None:
            return U32.forward_fp32_layer4(layer4, x)
        return layer4(x)
    cb, act = layer4[0], layer4[1][1]
    w, b = cb.folded()
    y, part = PointwiseRangeFunction.apply(x, w, b, bool(act.running_stat))
    return CS.ReluQuant.apply(y, act, part, False)
