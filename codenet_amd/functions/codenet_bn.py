"""The fp32 training block behind every deform stage -- BatchNorm2d -> ReLU -> Upsample(x2, nearest)
(lib/models/networks/shufflenetv2_dcn.py:303-308) -- as ONE autograd function on the HIP kernels of
csrc/codenet_bn_train.hip, and the walk of an fp32 ``deconv_layers`` on it.

The reference's main.py trains the fp32 model with BatchNorm in training mode: batch statistics, running buffers updated
every step.  Here the statistics are float64 sums in one order (no atomics), the apply pass writes the ReLU'd values once
(the stored hand-over to a next stage that reads through the up-sampling, codenet_stage x_up) or to their 2x2 replicas, and
the backward recomputes z from the saved stage output: no mask, no normalised tensor and no up-sampled tensor is stored.
"""
import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _native as N_
from .. import ops
from . import codenet_stage as CS
from ._fp32_common import _bn_settings_reason, _hook_reason, _one_value_error, _placement_reason, bn_relu_up

# A/B switch (tools/fp32_block_bench.py): False restores the module path (``seq(x)``) for the fp32 blocks
NATIVE_FP32_BLOCKS = True


class BnReluUpsample(Function):
    """(out, mean, var, invstd) = the block on y [N,C,H,W]: out = relu(bn(y)) at stored resolution (up = 1) or up-sampled
    x2 (up = 2).  bn: the nn.BatchNorm2d -- its mode decides between batch statistics (running buffers and
    num_batches_tracked advance in place, on the device) and the running statistics (nothing is written).  mean / var
    (biased) / invstd [C] are the per-channel numbers the call used; they take no gradient."""

    @staticmethod
    def forward(ctx, y, gamma, beta, bn, up):
        ops._gpu_f32(y, gamma, beta)
        y = y.contiguous()
        training = bool(bn.training)
        ws = CS._workspace(N_.lib().cdn_codenet_bn_workspace_bytes(*y.shape), y.device) if training else None
        out, mean, var, invstd = bn_relu_up(y, gamma, beta, bn, up, ws=ws)
        ctx.up, ctx.training = int(up), training
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y, gamma, beta, mean, invstd)
        ctx.mark_non_differentiable(mean, var, invstd)
        return out, mean, var, invstd

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *unused):
        if g is None:
            return (None,) * 5
        y, gamma, beta, mean, invstd = ctx.saved_tensors
        ws = CS._workspace(N_.lib().cdn_codenet_bn_workspace_bytes(*y.shape), y.device)
        gy, _, gg, gb = ops.bn_relu_up_backward(g, y, gamma, beta, mean, invstd, ctx.up, ctx.training, ws=ws)
        need = ctx.needs_input_grad
        return gy if need[0] else None, gg if need[1] else None, gb if need[2] else None, None, None


def _is_up2(up):
    return (isinstance(up, nn.Upsample) and up.mode == "nearest" and up.size is None
            and up.scale_factor in (2, 2.0, (2, 2), (2.0, 2.0)))


def native_reason(seq, x):
    """None when forward_stage_blocks runs the fp32 ``deconv_layers`` `seq` -- blocks of
    [DeformConvWithOffsetScaleBoundPositive, BatchNorm2d, ReLU, Upsample(x2, nearest)] -- on the fused kernels for the input
    x, else the reason -- a string -- why it takes ``seq(x)``.  x None: the modules alone are judged (structure and
    settings, not where the model lives): GraphedTrainStep.is_fp32_stage_stack."""
    from ..modules.dcn_deform_conv import DeformConvWithOffsetScaleBoundPositive
    if not NATIVE_FP32_BLOCKS:
        return "NATIVE_FP32_BLOCKS is off"
    if not torch.is_grad_enabled():
        return "grad mode is off (inference has pipeline.FusedHotPath)"
    mods = list(seq) if isinstance(seq, nn.Sequential) else None
    if not mods or len(mods) % 4:
        return "not a Sequential of four-module blocks"
    for i in range(0, len(mods), 4):
        st, bn, relu, up = mods[i:i + 4]
        what = "block %d" % (i // 4)
        if type(st) is not DeformConvWithOffsetScaleBoundPositive:
            return "%s: a mixed sequence (%s where the fp32 deform stage is expected)" % (what, type(st).__name__)
        if not (st.conv.is_codenet_depthwise() and st.conv_scale.out_channels == 1 and st.conv_scale.stride == (1, 1)):
            return "%s: the stage is not the co-designed depthwise form" % what
        if type(bn) is not nn.BatchNorm2d or not isinstance(relu, nn.ReLU) or not _is_up2(up):
            return "%s: a mixed sequence (not BatchNorm2d, ReLU, Upsample(x2, nearest))" % what
        why = _bn_settings_reason(bn, what)
        if why is not None:
            return why
        if bn.num_features != st.out_channels:
            return "%s: the BatchNorm2d has %d features, the stage %d channels" % (what, bn.num_features, st.out_channels)
        for m, name in ((st, "stage"), (bn, "BatchNorm2d"), (relu, "ReLU"), (up, "Upsample")):
            why = _hook_reason(m, "%s %s" % (what, name))
            if why is not None:
                return why
    if x is None:
        return None
    if not torch.is_tensor(x) or not x.is_cuda:
        return "x is a %s tensor, the kernels run on the GPU" % (x.device.type if torch.is_tensor(x) else type(x).__name__)
    if x.dtype != torch.float32 or x.dim() != 4 or x.numel() == 0:
        return "x must be a float32 [N, C, H, W] tensor (got %s %s)" % (x.dtype, tuple(x.shape))
    if x.shape[1] != mods[0].in_channels:
        return "the first stage expects %d input channels, x has %d" % (mods[0].in_channels, x.shape[1])
    Nb, _, H, W = x.shape
    for i in range(0, len(mods), 4):      # (every tensor of the walk within 32-bit indexing: what the entry points accept)
        st = mods[i]
        if Nb * max(st.in_channels, 4 * st.out_channels) * H * W >= 2 ** 31:
            return "block %d: a tensor of the walk reaches 2^31 elements (x %s)" % (i // 4, tuple(x.shape))
        H, W = 2 * H, 2 * W
    for i in range(0, len(mods), 4):
        st, bn = mods[i], mods[i + 1]
        why = _placement_reason(x, list(st.parameters()) + list(bn.parameters()), bn.buffers(), "block %d: " % (i // 4),
                                nothing=None)
        if why is not None:
            return why
    return _placement_reason(x, [p for m in mods for p in m.parameters()], (),
                             nothing="nothing to differentiate (the stages take their inference kernels)")


def forward_fp32_blocks(seq, x, keep=None):
    """The walk of an fp32 ``deconv_layers`` that native_reason(seq, x) accepts.  Every stage is one CodenetStageFunction,
    every block behind it one BnReluUpsample; where the next stage's gather reads through the up-sampling (the conditions
    of the quantised walk: STORED_RES_STAGES and cdn_codenet_dw_up2_supported) the block hands over the stored tensor and
    the up-sampled one is never written.  keep (tests): a list that receives (mean, var, invstd) of every block."""
    mods = list(seq)
    lib = N_.lib()
    x_up = False
    for i in range(0, len(mods), 4):
        st, bn = mods[i], mods[i + 1]
        pw = st.conv_channel if st.in_channels != st.out_channels else None
        Nb, H, W = x.shape[0], x.shape[2] * (2 if x_up else 1), x.shape[3] * (2 if x_up else 1)      # the stage's plane
        if bn.training and Nb * H * W == 1:
            raise _one_value_error((Nb, st.out_channels, H, W))
        y = CS.codenet_stage(x, st.conv_scale.weight, st.conv_scale.bias, st.conv.weight,
                             pw.weight if pw is not None else None, pw.bias if pw is not None else None,
                             st.conv_bound.min_val, st.conv_bound.max_val, x_up=x_up)
        C = y.shape[1]
        x_up = bool(CS.STORED_RES_STAGES and i + 4 < len(mods) and lib.cdn_codenet_dw_up2_supported(Nb, C, 2 * H, 2 * W))
        x, mean, var, invstd = BnReluUpsample.apply(y, bn.weight, bn.bias, bn, 1 if x_up else 2)
        if keep is not None:
            keep.append((mean, var, invstd))
    return x
