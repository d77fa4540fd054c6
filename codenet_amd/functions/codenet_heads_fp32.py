"""The fp32 detection heads in training as ONE autograd function on the HIP kernels of csrc/codenet_heads_fp32_train.hip
(DESIGN.md section 4.3f).

The reference's main.py trains the fp32 model; every head is the ``nn.Sequential`` of shufflenetv2_dcn.py:246-258

    y1 = conv1x1(x, W1)                  a1 = relu(bn1(y1))
    y2 = dw3x3(a1, W2), zero padding 1   a2 = relu(bn2(y2))
    y3 = conv1x1(a2, W3) + b3

seven framework modules under autograd, each reading and writing a head-sized tensor.  Here forward and backward of all
heads are one ``CodenetHeadsFp32Function``:

    forward   cdn_codenet_pointwise_forward (y1), cdn_codenet_head_fp32_bn_stats (BatchNorm1's numbers; a1 is never
              written), cdn_codenet_head_fp32_dw_forward (y2, a1 formed on load), then for hm
              cdn_codenet_bn_relu_up_forward with up = 1 (BatchNorm2's numbers and the stored a2) and
              cdn_codenet_pointwise_forward (y3), for wh / reg cdn_codenet_head_fp32_bn_stats and
              cdn_codenet_head_fp32_tail_forward (a2 formed on load, never stored)
    backward  per head: hm cdn_codenet_pointwise_wgrad (grad W3, b3), cdn_codenet_pointwise_forward on W3^T (grad a2) and
              cdn_codenet_head_fp32_bn_backward1 (g_z2 and BatchNorm2's sums); wh / reg
              cdn_codenet_head_fp32_tail_backward (all of that from the two-channel grad y3); then
              cdn_codenet_head_fp32_dw_backward (g_z1, grad W2, BatchNorm1's sums; grad y2 formed on load) and
              cdn_codenet_head_fp32_bn_backward2 (grad y1 into the head's slice of one [N, heads * 64, H, W] buffer); then ONE
              cdn_codenet_pointwise_wgrad (grad W1 of all heads) and ONE cdn_codenet_pointwise_forward on the concatenated
              W1^T (grad x)

Each BatchNorm follows its own ``training`` flag: batch statistics (running buffers and num_batches_tracked advance in
place, on the device) or the running statistics (nothing is written).  Every floating-point sum has one order, nothing
allocates outside the caching allocator, the step is capturable.
"""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N_
from .. import ops
from . import codenet_stage as CS
from ._fp32_common import (_bn_reason, _hook_reason, _input_reason, _is_1x1, _is_dw, _one_value_error, _placement_reason,
                           bn_backward2, bn_relu_up, bn_stats)

# A/B switch (tools/heads_fp32_bench.py): the fp32 heads of a training step on the kernels above (True) or module by module
# through the framework's autograd (False)
NATIVE_FP32_HEADS = True

_p = CS._p


def _ws(shape, device):
    return CS._workspace(N_.lib().cdn_codenet_head_fp32_workspace_bytes(*shape), device)


def dw_forward(y1, st1, gamma1, beta1, w2):
    """y2 = dw3x3(relu(bn1(y1)), w2) with zero padding 1; st1 = (mean, var, invstd) of y1."""
    Nb, C, H, W = y1.shape
    y2 = torch.empty_like(y1)
    rc = N_.lib().cdn_codenet_head_fp32_dw_forward(_p(y1), _p(st1[0]), _p(st1[2]), _p(gamma1), _p(beta1), _p(w2), _p(y2), Nb, C,
                                                   H, W, ops._stream(y1))
    N_.check(rc, "cdn_codenet_head_fp32_dw_forward")
    return y2


def tail_forward(y2, st2, gamma2, beta2, w3, b3):
    """y3 = conv1x1(relu(bn2(y2)), w3) + b3 for at most four output channels."""
    Nb, C, H, W = y2.shape
    Co = w3.shape[0]
    y3 = y2.new_empty(Nb, Co, H, W)
    rc = N_.lib().cdn_codenet_head_fp32_tail_forward(_p(y2), _p(st2[0]), _p(st2[2]), _p(gamma2), _p(beta2), _p(w3), _p(b3),
                                                     _p(y3), Nb, C, Co, H, W, ops._stream(y2))
    N_.check(rc, "cdn_codenet_head_fp32_tail_forward")
    return y3


def tail_backward(gy3, y2, st2, gamma2, beta2, w3):
    """(g_z2, grad_gamma2, grad_beta2, means [2, C] = (mb2, mg2), grad_w3 [Co, C], grad_b3 [Co]) of the narrow tail."""
    Nb, C, H, W = y2.shape
    Co = w3.shape[0]
    gz2 = torch.empty_like(y2)
    gg, gb, means = y2.new_empty(C), y2.new_empty(C), y2.new_empty(2, C)
    gw3, gb3 = y2.new_empty(Co, C), y2.new_empty(Co)
    ws = _ws(y2.shape, y2.device)
    rc = N_.lib().cdn_codenet_head_fp32_tail_backward(
        _p(gy3), _p(y2), _p(st2[0]), _p(st2[2]), _p(gamma2), _p(beta2), _p(w3), _p(gz2), _p(gg), _p(gb), _p(means[0]),
        _p(means[1]), _p(gw3), _p(gb3), Nb, C, Co, H, W, _p(ws), ws.numel() * 4, ops._stream(y2))
    N_.check(rc, "cdn_codenet_head_fp32_tail_backward")
    return gz2, gg, gb, means, gw3, gb3


def bn_backward1(ga, y, st, gamma, beta):
    """(g_z, grad_gamma, grad_beta, means [2, C] = (mb, mg)): the first BatchNorm backward pass on a stored grad_a."""
    Nb, C, H, W = y.shape
    gz = torch.empty_like(y)
    gg, gb, means = y.new_empty(C), y.new_empty(C), y.new_empty(2, C)
    ws = _ws(y.shape, y.device)
    rc = N_.lib().cdn_codenet_head_fp32_bn_backward1(_p(ga), _p(y), _p(st[0]), _p(st[2]), _p(gamma), _p(beta), _p(gz), _p(gg),
                                                     _p(gb), _p(means[0]), _p(means[1]), Nb, C, H, W, _p(ws), ws.numel() * 4,
                                                     ops._stream(y))
    N_.check(rc, "cdn_codenet_head_fp32_bn_backward1")
    return gz, gg, gb, means


def dw_backward(gz2, y2, st2, gamma2, means2, training2, y1, st1, gamma1, beta1, w2):
    """(g_z1, grad_w2, grad_gamma1, grad_beta1, means [2, C] = (mb1, mg1)) of the depthwise 3x3 between the BatchNorms."""
    Nb, C, H, W = y1.shape
    gz1, gw2 = torch.empty_like(y1), torch.empty_like(w2)
    gg, gb, means = y1.new_empty(C), y1.new_empty(C), y1.new_empty(2, C)
    ws = _ws(y1.shape, y1.device)
    rc = N_.lib().cdn_codenet_head_fp32_dw_backward(
        _p(gz2), _p(y2), _p(st2[0]), _p(st2[2]), _p(gamma2), _p(means2[0]), _p(means2[1]), int(bool(training2)), _p(y1),
        _p(st1[0]), _p(st1[2]), _p(gamma1), _p(beta1), _p(w2), _p(gz1), _p(gw2), _p(gg), _p(gb), _p(means[0]), _p(means[1]),
        Nb, C, H, W, _p(ws), ws.numel() * 4, ops._stream(y1))
    N_.check(rc, "cdn_codenet_head_fp32_dw_backward")
    return gz1, gw2, gg, gb, means


class CodenetHeadsFp32Function(Function):
    """(y3 of every head) = heads(x).  meta: one (name, bn1, bn2) per head; flat: W1, gamma1, beta1, W2, gamma2, beta2, W3,
    b3 per head.  The BatchNorm buffers are updated in place by the forward, as the module path does.  keep (a dict or
    None) receives {name: {"y1", "y2", "bn1": (mean, var, invstd), "bn2": ...}} from the forward and, from the backward,
    "g_z2", "g_z1", "means2", "means1" and "grad_y1" (the head's slice)."""

    @staticmethod
    def forward(ctx, x, meta, keep, *flat):
        ops._gpu_f32(x, *flat)
        ctx.set_materialize_grads(False)      # (a head that took no part in the loss gets no zero tensor)
        saved = [x]
        outs, modes = [], []
        for h, (name, bn1, bn2) in enumerate(meta):
            w1, g1, b1, w2, g2, b2, w3, b3 = [t.contiguous() for t in flat[8 * h: 8 * h + 8]]
            y1 = ops.codenet_pointwise(x, w1)
            st1 = bn_stats(y1, bn1)
            y2 = dw_forward(y1, st1, g1, b1, w2)
            Co = w3.shape[0]
            if Co <= 4:
                st2 = bn_stats(y2, bn2)
                a2 = y2             # (a placeholder: a2 is never stored)
                y3 = tail_forward(y2, st2, g2, b2, w3, b3)
            else:
                a2, *st2 = bn_relu_up(y2, g2, b2, bn2)
                y3 = ops.codenet_pointwise(a2, w3, b3)
            if keep is not None:
                keep[name] = {"y1": y1, "y2": y2, "bn1": tuple(st1), "bn2": tuple(st2)}
            outs.append(y3)
            modes.append((bool(bn1.training), bool(bn2.training)))
            saved += [y1, y2, a2, *st1, *st2, w1, g1, b1, w2, g2, b2, w3]
        ctx.names = [m[0] for m in meta]
        ctx.modes, ctx.keep = modes, keep
        ctx.save_for_backward(*saved)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gys):
        saved = ctx.saved_tensors
        x = saved[0]
        n = len(ctx.names)
        need = ctx.needs_input_grad
        grads = [None] * (3 + 8 * n)
        live = [h for h in range(n) if gys[h] is not None]
        if not live:
            return tuple(grads)
        Nb, Cin, H, W = x.shape
        C = saved[1].shape[1]
        # the heads' grad_y1 in slices of one buffer: grad_x and grad_W1 of all heads are one launch each
        gy1 = x.new_empty(Nb, len(live) * C, H, W)
        pitch = len(live) * C * H * W
        for j, h in enumerate(live):
            y1, y2, a2, m1, v1, i1, m2, v2, i2, w1, g1, b1, w2, g2, b2, w3 = saved[1 + 16 * h: 17 + 16 * h]
            st1, st2 = (m1, v1, i1), (m2, v2, i2)
            train1, train2 = ctx.modes[h]
            gy = gys[h].contiguous()
            Co = w3.shape[0]
            base = 3 + 8 * h
            if Co <= 4:      # grad_a2 is formed inside the kernel, never stored
                gz2, gg2, gb2, means2, gw3, gb3 = tail_backward(gy, y2, st2, g2, b2, w3)
            else:
                gw3, gb3 = CS.pointwise_wgrad(gy, a2, True)
                ga2 = ops.codenet_pointwise(gy, w3.reshape(Co, C).t().contiguous().view(C, Co, 1, 1))
                gz2, gg2, gb2, means2 = bn_backward1(ga2, y2, st2, g2, b2)
            gz1, gw2, gg1, gb1, means1 = dw_backward(gz2, y2, st2, g2, means2, train2, y1, st1, g1, b1, w2)
            bn_backward2(gz1, y1, st1, g1, means1, train1, gy1, j, pitch)
            if ctx.keep is not None and ctx.names[h] in ctx.keep:
                ctx.keep[ctx.names[h]].update(g_z2=gz2, g_z1=gz1, means2=means2, means1=means1,
                                              grad_y1=gy1[:, j * C:(j + 1) * C])
            for k, g in ((1, gg1), (2, gb1), (3, gw2), (4, gg2), (5, gb2), (6, gw3.view_as(w3)), (7, gb3)):
                grads[base + k] = g if need[base + k] else None
        if any(need[3 + 8 * h] for h in live):
            gw1, _ = CS.pointwise_wgrad(gy1, x, False)
            for j, h in enumerate(live):
                if need[3 + 8 * h]:
                    grads[3 + 8 * h] = gw1[j * C:(j + 1) * C].view_as(saved[1 + 16 * h + 9])
        if need[0]:
            w1s = [saved[1 + 16 * h + 9].reshape(C, Cin) for h in live]
            w1t = (w1s[0] if len(w1s) == 1 else torch.cat(w1s, 0)).t().contiguous()
            grads[0] = ops.codenet_pointwise(gy1, w1t.view(Cin, len(live) * C, 1, 1))
        return tuple(grads)


def _head_reason(name, mod):
    what = "head '%s'" % name
    if not isinstance(mod, nn.Sequential) or len(mod) != 7:
        return ("%s is a %s, not the seven-module Sequential Conv2d 1x1 -> BatchNorm2d -> ReLU -> depthwise Conv2d 3x3 -> "
                "BatchNorm2d -> ReLU -> Conv2d 1x1 (head_conv = 0 and other forms keep the module path)"
                % (what, type(mod).__name__))
    c1, bn1, r1, c2, bn2, r2, c3 = list(mod)
    if not (type(c1) is nn.Conv2d and type(c2) is nn.Conv2d and type(c3) is nn.Conv2d and isinstance(r1, nn.ReLU)
            and isinstance(r2, nn.ReLU)):
        return "%s: not Conv2d, BatchNorm2d, ReLU, Conv2d, BatchNorm2d, ReLU, Conv2d" % what
    C = c1.out_channels
    if not (_is_1x1(c1) and _is_1x1(c3) and _is_dw(c2, 1) and c2.in_channels == C and c3.in_channels == C
            and all(getattr(c, "padding_mode", "zeros") == "zeros" for c in (c1, c3))):
        return "%s: not the heads' own geometry (1x1 -> depthwise 3x3, stride 1, zero padding 1 -> 1x1)" % what
    if c1.bias is not None or c2.bias is not None:
        return "%s: a convolution in front of a BatchNorm2d has a bias (the reference's have none)" % what
    if c3.bias is None:
        return "%s: the last convolution has no bias (the reference's has one)" % what
    for bn, which in ((bn1, "the first BatchNorm2d"), (bn2, "the second BatchNorm2d")):
        why = _bn_reason(bn, C, "%s: %s" % (what, which))
        if why is not None:
            return why
    return _hook_reason(mod, what)


def native_reason(heads, x):
    """None when forward_fp32_heads runs `heads` (an ordered mapping name -> module) on the kernels for the input x, else
    the reason -- a string -- why they take the module path.  x None: the heads alone are judged (their structure and
    settings, not where the model lives): pipeline.GraphedTrainStep.is_fp32_tail."""
    if not NATIVE_FP32_HEADS:
        return "NATIVE_FP32_HEADS is off"
    if not torch.is_grad_enabled():
        return "grad mode is off (inference has pipeline.FusedHeads)"
    if not heads:
        return "no heads"
    for name, mod in heads.items():
        why = _head_reason(name, mod)
        if why is not None:
            return why
    if len({m[0].out_channels for m in heads.values()}) != 1:
        return "the heads do not share one hidden width"
    if x is None:
        return None
    hidden = next(iter(heads.values()))[0].out_channels
    widest = max([len(heads) * hidden] + [m[6].out_channels for m in heads.values()])
    why = _input_reason(x, widest)
    if why is not None:
        return why
    for name, mod in heads.items():
        if mod[0].in_channels != x.shape[1]:
            return "head '%s' expects %d input channels, x has %d" % (name, mod[0].in_channels, x.shape[1])
        why = _placement_reason(x, mod.parameters(), mod.buffers(), "head '%s': " % name, nothing=None)
        if why is not None:
            return why
    return _placement_reason(x, [p for m in heads.values() for p in m.parameters()], ())      # (placed: it asks for grad)


def forward_fp32_heads(heads, x, keep=None):
    """{name: head(x)} for fp32 heads that native_reason(heads, x) accepts, as one CodenetHeadsFp32Function.  keep (tests):
    a dict that receives per head y1, y2 and (mean, var, invstd) of both BatchNorms."""
    names = list(heads)
    mods = [heads[h] for h in names]
    Nb, _, H, W = x.shape
    if Nb * H * W == 1 and any(m[i].training for m in mods for i in (1, 4)):
        raise _one_value_error((Nb, mods[0][0].out_channels, H, W))
    meta = tuple((h, m[1], m[4]) for h, m in zip(names, mods))
    flat = []
    for m in mods:
        flat += [m[0].weight, m[1].weight, m[1].bias, m[3].weight, m[4].weight, m[4].bias, m[6].weight, m[6].bias]
    outs = CodenetHeadsFp32Function.apply(x, meta, keep, *flat)
    return dict(zip(names, outs))
