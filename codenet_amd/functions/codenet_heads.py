"""The quantised detection heads as ONE autograd function on the HIP kernels (training path).

The reference runs every head (``QuantDepthwiseNode``, quant_modules.py:1013-1071) module by module under autograd:

    y1 = conv1x1(x, W1q) + b1        a1 = fq1(relu(y1))       (act1 tracks the extremes of relu(y1))
    y2 = dw3x3(a1, W2q) + b2         a2 = fq3(relu(y2))       (act3 tracks the extremes of relu(y2))
    y3 = conv1x1(a2, W3q) + b3

Here forward and backward of all heads are one ``CodenetHeadsFunction`` between the deform stages
(functions/codenet_stage.py) and the criterion (losses.CtdetLoss):

    forward   cdn_codenet_pointwise_forward_range (y1 + its {min, max} pairs), cdn_codenet_head_act_update (act1),
              cdn_codenet_head_dw_forward (r2 = relu(y2), act3 updated by the launch's last workgroup),
              cdn_codenet_pointwise_forward_range (hm: y3 with r2 fake-quantised on load) or
              cdn_codenet_head_tail_train_forward (wh / reg: at most four output channels on the VALU)
    backward  per head cdn_codenet_pointwise_wgrad_q (grad W3q, b3), for hm cdn_codenet_pointwise_forward on W3q^T (grad a2),
              cdn_codenet_head_dw_backward (grad y1 into its slice of one [N, heads * 64, H, W] buffer, grad W2q, b2; for
              wh / reg it forms grad a2 from the two-channel grad y3 itself); then ONE cdn_codenet_pointwise_wgrad
              (grad W1q, b1 of all heads) and ONE cdn_codenet_pointwise_forward on the concatenated W1q^T (grad x)

Straight-through quantisers, ReLU masks y > 0.  The weight transformations (BN fold, fake-quantisation) stay the native
autograd functions of codenet_stage.py; this function takes their outputs and returns gradients for them.  Every
floating-point sum has one order, nothing allocates outside the caching allocator, the step is capturable.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N_
from .. import ops
from . import codenet_stage as CS
from ._qat_common import (_act_update, _fold_all, _hook_reason, _input_reason, _is_1x1, _is_dw, _placement_reason,
                          _relu_act_reason, _tracked_act, _weight_prep_structural)

# A/B switch (tools/heads_train_bench.py): the heads of a QAT step on the kernels above (True) or module by module
# through the framework's autograd (False)
NATIVE_HEADS = True

_p = CS._p


def _dw_forward(y1, snap1, w2, b2, act3):
    """r2 = relu(dw3x3(fq1(relu(y1)), w2) + b2) (stored before quantisation) and the snapshot of act3's state."""
    Nb, C, H, W = y1.shape
    r2 = torch.empty_like(y1)
    snap3, upd = _tracked_act(act3, y1.device)
    rc = N_.lib().cdn_codenet_head_dw_forward(_p(y1), _p(snap1), _p(w2), _p(b2), _p(r2), Nb, C, H, W, *upd, ops._stream(y1))
    N_.check(rc, "cdn_codenet_head_dw_forward")
    return r2, snap3


class CodenetHeadsFunction(Function):
    """(y3 of every head) = heads(x).  meta: one (name, act1, act3) per head; flat: W1q, b1, W2q, b2, W3q, b3 (or None)
    per head, already folded / fake-quantised.  The QuantAct buffers are updated in place by the forward, as the module
    path does.  keep (a dict or None) receives {name: {"y1": ..., "r2": ...}} -- the saved tensors themselves."""

    @staticmethod
    def forward(ctx, x, meta, keep, *flat):
        ops._gpu_f32(x, *flat)
        ctx.set_materialize_grads(False)      # (a head that took no part in the loss gets no zero tensor)
        Nb, Cin, H, W = x.shape
        outs, saved = [], [x]
        for h, (name, act1, act3) in enumerate(meta):
            w1, b1, w2, b2, w3, b3 = [t.contiguous() if t is not None else None for t in flat[6 * h: 6 * h + 6]]
            if act1.running_stat:
                y1, part = ops.codenet_pointwise(x, w1, b1, want_range=True)
            else:
                y1, part = ops.codenet_pointwise(x, w1, b1), None
            snap1 = _act_update(act1, part, True)
            r2, snap3 = _dw_forward(y1, snap1, w2, b2, act3)
            Co, C = w3.shape[0], w3.shape[1]
            if Co <= 4:
                y3 = x.new_empty(Nb, Co, H, W)
                rc = N_.lib().cdn_codenet_head_tail_train_forward(_p(r2), _p(snap3), _p(w3), _p(b3), _p(y3), Nb, C, Co,
                                                                  H * W, ops._stream(x))
                N_.check(rc, "cdn_codenet_head_tail_train_forward")
            else:
                y3 = ops.codenet_pointwise(r2, w3, b3, d_state=snap3)
            if keep is not None:
                keep[name] = {"y1": y1, "r2": r2}
            outs.append(y3)
            saved += [y1, r2, snap1, snap3, w1, w2, w3]
        ctx.n_heads = len(meta)
        ctx.has_b3 = [flat[6 * h + 5] is not None for h in range(len(meta))]
        ctx.save_for_backward(*saved)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gys):
        saved = ctx.saved_tensors
        x = saved[0]
        n = ctx.n_heads
        need = ctx.needs_input_grad
        grads = [None] * (3 + 6 * n)
        live = [h for h in range(n) if gys[h] is not None]
        if not live:
            return tuple(grads)
        lib = N_.lib()
        Nb, Cin, H, W = x.shape
        C = saved[1].shape[1]
        # the heads' grad_y1 in slices of one buffer: grad_x and grad_W1q of all heads are one launch each
        gy1 = x.new_empty(Nb, len(live) * C, H, W)
        pitch = len(live) * C * H * W
        nws = lib.cdn_codenet_head_dw_backward_workspace_bytes(Nb, C, H, W)
        for j, h in enumerate(live):
            y1, r2, snap1, snap3, w1, w2, w3 = saved[1 + 7 * h: 8 + 7 * h]
            gy = gys[h].contiguous()
            Co = w3.shape[0]
            want_b3 = ctx.has_b3[h] and need[3 + 6 * h + 5]
            if need[3 + 6 * h + 4] or want_b3:
                gw3, gb3 = CS.pointwise_wgrad(gy, r2, want_b3, d_state=snap3)
                grads[3 + 6 * h + 4] = gw3.view_as(w3) if need[3 + 6 * h + 4] else None
                grads[3 + 6 * h + 5] = gb3
            if Co <= 4:      # grad_a2 is formed inside the depthwise backward, never stored
                g, w3p, co = gy, w3, Co
            else:
                g = ops.codenet_pointwise(gy, w3.reshape(Co, C).t().contiguous().view(C, Co, 1, 1))
                w3p, co = None, 0
            gw2, gb2 = torch.empty_like(w2), x.new_empty(C)
            ws = CS._workspace(nws, x.device)
            rc = lib.cdn_codenet_head_dw_backward(_p(g), _p(w3p), co, _p(r2), _p(y1), _p(snap1), _p(w2),
                                                  gy1.data_ptr() + 4 * j * C * H * W, pitch, _p(gw2), _p(gb2), Nb, C, H, W,
                                                  _p(ws), ws.numel() * 4, ops._stream(x))
            N_.check(rc, "cdn_codenet_head_dw_backward")
            grads[3 + 6 * h + 2], grads[3 + 6 * h + 3] = gw2, gb2
        w1s = [saved[1 + 7 * h + 4].reshape(C, Cin) for h in live]
        gw1, gb1 = CS.pointwise_wgrad(gy1, x, True)
        for j, h in enumerate(live):
            grads[3 + 6 * h] = gw1[j * C:(j + 1) * C].view_as(saved[1 + 7 * h + 4])
            grads[3 + 6 * h + 1] = gb1[j * C:(j + 1) * C]
        if need[0]:
            w1t = (w1s[0] if len(w1s) == 1 else torch.cat(w1s, 0)).t().contiguous()
            grads[0] = ops.codenet_pointwise(gy1, w1t.view(Cin, len(live) * C, 1, 1))
        return tuple(grads)


def _head_reason(name, mod):
    from ..portable_quantizer.quant_modules import QuantDepthwiseNode
    if not isinstance(mod, QuantDepthwiseNode):
        return "head '%s' is a %s, not a QuantDepthwiseNode (the fp32 nn.Sequential heads keep the module path)" % (
            name, type(mod).__name__)
    why = _hook_reason(mod, "head '%s'" % name)
    if why is not None:
        return why
    for attr in ("quant_act1", "quant_act3"):
        why = _relu_act_reason(getattr(mod, attr), "head '%s': %s" % (name, attr))
        if why is not None:
            return why
    c1, c2, c3 = mod.quant_convbn1.conv, mod.quant_convbn2.conv, mod.quant_conv
    C = c1.out_channels
    if not (_is_1x1(c1) and _is_1x1(c3) and _is_dw(c2, 1) and c2.in_channels == C and c3.in_channels == C):
        return "head '%s': not the heads' own geometry (1x1 -> depthwise 3x3, stride 1, zero padding 1 -> 1x1)" % name
    return None


def native_reason(heads, x):
    """None when forward_heads runs `heads` (an ordered mapping name -> module) on the kernels for the input x, else
    the reason -- a string -- why it takes the module path.  x None: the heads alone are judged (their structure and
    settings, not where the model lives): pipeline.GraphedTrainStep.is_native_tail."""
    if not NATIVE_HEADS:
        return "NATIVE_HEADS is off"
    if not torch.is_grad_enabled():
        return "grad mode is off (inference has pipeline.FusedHeads)"
    if not heads:
        return "no heads"
    for name, mod in heads.items():
        why = _head_reason(name, mod)
        if why is not None:
            return why
    if len({m.quant_convbn1.conv.out_channels for m in heads.values()}) != 1:
        return "the heads do not share one hidden width"
    for name, mod in heads.items():
        for q, w in ((mod.quant_convbn1, mod.quant_convbn1.conv.weight), (mod.quant_convbn2, mod.quant_convbn2.conv.weight),
                     (mod.quant_conv, mod.quant_conv.weight)):
            if not _weight_prep_structural(w, q):
                return ("head '%s': a weight quantiser is not on the device weight-prep path (per-channel symmetric, "
                        "quantising, no bias quantisation)" % name)
    if x is None:
        return None
    hidden = next(iter(heads.values())).quant_convbn1.conv.out_channels
    why = _input_reason(x, len(heads) * hidden)
    if why is not None:
        return why
    Cin = x.shape[1]
    for name, mod in heads.items():
        if mod.quant_convbn1.conv.in_channels != Cin:
            return "head '%s' expects %d input channels, x has %d" % (name, mod.quant_convbn1.conv.in_channels, Cin)
        why = _placement_reason(x, ((mod.quant_convbn1.conv.weight, mod.quant_convbn1),
                                    (mod.quant_convbn2.conv.weight, mod.quant_convbn2), (mod.quant_conv.weight, mod.quant_conv)),
                                (mod.quant_act1[1], mod.quant_act3[1]), "head '%s': " % name)
        if why is not None:
            return why
    return None


def _prepared_weights(mods):
    """[(W1q, b1, W2q, b2, W3q, b3)] per head: the folds of all heads in one launch and the last convs' quantisers in
    another where the multi-tensor weight prep takes them, else every module's own (native) preparation."""
    cbs = [cb for m in mods for cb in (m.quant_convbn1, m.quant_convbn2)]
    f = _fold_all(cbs)
    if CS.MULTI_WEIGHT_PREP and len(cbs) <= 8:
        q = CS.MultiFakeQuantWeight.apply(tuple((m.quant_conv.weight_bit, m.quant_conv.weight_percentile) for m in mods),
                                          *[m.quant_conv.weight for m in mods])
    else:
        q = [m.quant_conv.quantized_weight() for m in mods]
    return [tuple(f[4 * i:4 * i + 4]) + (q[i], m.quant_conv.bias) for i, m in enumerate(mods)]


def forward_heads(heads, x, keep=None):
    """{name: head(x)} for an ordered mapping name -> head module.  In the QAT step on the GPU (native_reason(heads, x)
    is None) all heads run as one CodenetHeadsFunction; the fp32 heads of main.py under autograd on the GPU
    (codenet_heads_fp32.native_reason(heads, x) is None) as one CodenetHeadsFp32Function; otherwise exactly
    ``{h: mod(x)}``.  keep (tests): a dict that receives per head the native path's y1 and r2 (fp32: y1, y2 and both
    BatchNorms' numbers)."""
    if native_reason(heads, x) is not None:
        from . import codenet_heads_fp32
        if codenet_heads_fp32.native_reason(heads, x) is None:
            return codenet_heads_fp32.forward_fp32_heads(heads, x, keep)
        return {h: mod(x) for h, mod in heads.items()}
    names = list(heads)
    mods = [heads[h] for h in names]
    meta = tuple((h, m.quant_act1[1], m.quant_act3[1]) for h, m in zip(names, mods))
    flat = [t for trio in _prepared_weights(mods) for t in trio]
    outs = CodenetHeadsFunction.apply(x, meta, keep, *flat)
    return dict(zip(names, outs))
