"""What the native functions of the fp32 training step share (codenet_heads_fp32.py, codenet_units_fp32.py,
codenet_stem_fp32.py, codenet_bn.py): the BatchNorm launches more than one of them makes and the pieces of the gates that
decide between the kernels and the module path.  A gate returns None or the reason -- a string -- why the module path is
taken.  The structural predicates are those of the QAT step (_qat_common.py)."""
import torch
import torch.nn as nn

from .. import _native as N_
from .. import ops
from . import codenet_stage as CS
from ._qat_common import _hook_reason, _input_reason, _is_1x1, _is_dw      # noqa: F401 (handed on to the fp32 modules)

_p = CS._p


def _out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def bn_stats(y, bn):
    """(mean, var, invstd), the rows of one [3, C] tensor, of y for the BatchNorm2d `bn`: batch statistics with the buffers
    advanced in place (bn.training) or the running statistics (nothing written).  cdn_codenet_head_fp32_bn_stats."""
    Nb, C, H, W = y.shape
    training = bool(bn.training)
    stats = y.new_empty(3, C)
    ws = CS._workspace(N_.lib().cdn_codenet_head_fp32_workspace_bytes(*y.shape), y.device) if training else None
    rc = N_.lib().cdn_codenet_head_fp32_bn_stats(
        _p(y), _p(bn.running_mean), _p(bn.running_var), _p(bn.num_batches_tracked) if training else None, _p(stats[0]),
        _p(stats[1]), _p(stats[2]), Nb, C, H, W, int(training), float(bn.eps), float(bn.momentum), _p(ws),
        ws.numel() * 4 if ws is not None else 0, ops._stream(y))
    N_.check(rc, "cdn_codenet_head_fp32_bn_stats")
    return stats


def bn_relu_up(y, gamma, beta, bn, up=1, ws=None):
    """(out, mean, var, invstd) = ops.bn_relu_up_forward for the BatchNorm2d `bn` in its own mode: the running buffers and
    the batch counter advance only where it trains."""
    training = bool(bn.training)
    return ops.bn_relu_up_forward(y, gamma, beta, bn.running_mean, bn.running_var,
                                  bn.num_batches_tracked if training else None, bn.eps, bn.momentum, up, training, ws=ws)


def bn_backward2(gz, y, st, gamma, means, training, out, slot, pitch):
    """grad_y of BatchNorm's second pass into channels [slot * C, (slot + 1) * C) of `out` [N, pitch / (H W), H, W]."""
    Nb, C, H, W = y.shape
    rc = N_.lib().cdn_codenet_head_fp32_bn_backward2(_p(gz), _p(y), _p(st[0]), _p(st[2]), _p(gamma), _p(means[0]),
                                                     _p(means[1]), out.data_ptr() + 4 * slot * C * H * W, pitch, Nb, C, H, W,
                                                     int(bool(training)), ops._stream(y))
    N_.check(rc, "cdn_codenet_head_fp32_bn_backward2")


def _one_value_error(shape):
    """The framework's error for one value per channel, raised before any launch."""
    return ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(shape),))


def _bn_settings_reason(bn, what):
    if not bn.affine:
        return "%s: BatchNorm2d(affine=False)" % what
    if not bn.track_running_stats or bn.running_mean is None:
        return "%s: BatchNorm2d(track_running_stats=False)" % what
    if bn.momentum is None:
        return "%s: BatchNorm2d(momentum=None), the cumulative average" % what
    return None


def _bn_reason(bn, C, what):
    if type(bn) is not nn.BatchNorm2d:
        return "%s is a %s, not a BatchNorm2d" % (what, type(bn).__name__)
    why = _bn_settings_reason(bn, what)
    if why is not None:
        return why
    if bn.num_features != C:
        return "%s has %d features, the convolution in front of it %d channels" % (what, bn.num_features, C)
    return None


def _placement_reason(x, params, buffers, prefix="", nothing="nothing to differentiate"):
    """After _input_reason: the parameters and buffers are float32 tensors where x lives, and x or a parameter requires
    grad.  nothing None: the second question is not asked (a caller with several groups of tensors asks it once, last)."""
    params = list(params)
    for t in params + list(buffers):
        if t.device != x.device or (t.is_floating_point() and t.dtype != torch.float32):
            return prefix + "a parameter or buffer is not a float32 tensor on x's device"
    if nothing is not None and not (x.requires_grad or any(p.requires_grad for p in params)):
        return nothing
    return None
