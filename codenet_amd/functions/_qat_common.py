"""What the native functions of the QAT step share (codenet_heads.py, codenet_units.py, codenet_stem.py): the QuantAct
update around a launch, the multi-tensor weight fold, and the gates that decide between the kernels and the module path.
A gate returns None or the reason -- a string -- why the module path is taken.  The fp32 training step (_fp32_common.py)
takes the structural predicates and the input gate from here."""
import torch
import torch.nn as nn

from .. import _native as N_
from .. import ops
from . import codenet_stage as CS

_p = CS._p


def _act_update(act, partials, relu):
    """The QuantAct update from a producer's {min, max} pairs (or, with a frozen range, only scale / zero point):
    returns the state snapshot the consumers and the backward pass read."""
    dev = act.x_min.device
    snap = torch.empty(8, dtype=torch.int32, device=dev)
    running = bool(act.running_stat)
    rc = N_.lib().cdn_codenet_head_act_update(
        _p(act.x_min), _p(act.x_max), _p(act._device_state(dev)), _p(partials) if running else None,
        partials.shape[0] if running else 0, int(act.activation_bit), float(act.momentum), int(running), int(bool(relu)),
        _p(snap), torch.cuda.current_stream(dev).cuda_stream)
    N_.check(rc, "cdn_codenet_head_act_update")
    return snap


def _tracked_act(act, device):
    """(snap, args) for a launch whose last workgroup updates `act`: the tensor that receives (running range) or already
    holds (frozen range) the state snapshot, and the entry point's arguments from x_min to state_copy."""
    if act.running_stat:
        snap = torch.empty(8, dtype=torch.int32, device=device)
        upd = ops._update_args(act, device, False)
    else:
        snap = _act_update(act, None, False)
        upd = (None, None, None, None, int(act.activation_bit), float(act.momentum))
    return snap, (*upd, int(bool(act.running_stat)), _p(snap))


def _fold_all(cbs):
    """(Wq, b) of every QuantBnConv2d of `cbs`, flat: one launch where the multi-tensor weight prep takes them, else
    every module's own (native) preparation."""
    if CS.MULTI_WEIGHT_PREP and len(cbs) <= 8:
        flat = []
        for cb in cbs:
            flat += [cb.conv.weight, cb.conv.bias, cb.bn.weight, cb.bn.bias, cb.bn.running_mean, cb.bn.running_var]
        return tuple(CS.MultiFoldFakeQuantWeight.apply(
            tuple((cb.weight_bit, cb.weight_percentile, cb.bn.eps) for cb in cbs), *flat))
    out = ()
    for cb in cbs:
        out += tuple(cb.folded())
    return out


def _is_1x1(conv):
    return (tuple(conv.kernel_size) == (1, 1) and tuple(conv.stride) == (1, 1) and tuple(conv.padding) == (0, 0)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1)


def _is_dw(conv, stride):
    C = conv.in_channels
    return (tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (stride, stride) and tuple(conv.padding) == (1, 1)
            and tuple(conv.dilation) == (1, 1) and conv.groups == C and conv.out_channels == C
            and getattr(conv, "padding_mode", "zeros") == "zeros")


def _weight_prep_structural(w, q):
    """CS.native_weight_prep_ok without the placement of `w`: what the quantiser is, not where the model lives."""
    k_lo, k_hi, _ = CS.weight_range_ranks(w.numel() // w.shape[0], q.weight_percentile)
    return (q.per_channel and q.quant_mode == "symmetric" and not q.full_precision_flag and not q.quantize_bias
            and k_lo <= 4 and k_hi <= 4)


def _hook_reason(root, what):
    for sub_name, m in root.named_modules():
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None):
            return "%s: a hook on sub-module '%s' must fire, the native path bypasses its __call__" % (
                what, sub_name or "<the module>")
    return None


def _act_reason(act, what):
    from ..portable_quantizer.quant_modules import QuantAct
    if not isinstance(act, QuantAct):
        return "%s is not a QuantAct" % what
    if act.percentile:
        return "%s uses percentile statistics (--act-percentile keeps the module path)" % what
    if not CS.native_act_ok(act):
        return "%s is not an asymmetric quantising QuantAct (quant_mode %s, full precision %s)" % (
            what, act.quant_mode, act.full_precision_flag)
    if getattr(act, "global_range", False):
        return "%s is in global_range mode" % what
    return None


def _relu_act_reason(seq, what):
    from ..portable_quantizer.quant_modules import QuantAct
    if not (isinstance(seq, nn.Sequential) and len(seq) == 2 and isinstance(seq[0], nn.ReLU)
            and isinstance(seq[1], QuantAct)):
        return "%s is not Sequential(ReLU, QuantAct)" % what
    return _act_reason(seq[1], what)


def _input_reason(x, widest, channels=None, aligned=False, takes_grad=True):
    """The gate on the input itself: a contiguous float32 [N, C, H, W] GPU tensor within 32-bit indexing.  widest: the
    largest per-pixel channel count of a tensor the kernels index with 32 bits -- a number or a function of (H, W);
    channels: what the first module expects; aligned: the kernels need 16-byte aligned rows; takes_grad False: the
    native path builds no gradient with respect to x (reported first)."""
    if not takes_grad and torch.is_tensor(x) and x.requires_grad:
        return "x requires grad: the native stem builds no gradient with respect to the image"
    if not torch.is_tensor(x) or not x.is_cuda:
        return "x is a %s tensor, the kernels run on the GPU" % (x.device.type if torch.is_tensor(x) else type(x).__name__)
    shape = "[N, %s, H, W]" % ("C" if channels is None else channels)
    if (x.dtype != torch.float32 or x.dim() != 4 or x.numel() == 0 or not x.is_contiguous()
            or (aligned and x.data_ptr() % 16)):
        return "x must be a contiguous%s float32 %s tensor (got %s %s)" % (
            ", 16-byte aligned" if aligned else "", shape, x.dtype, tuple(x.shape))
    Nb, Cx, H, W = x.shape
    if channels is not None and Cx != channels:
        return "the first module expects %d input channels, x has %d: it is no %s tensor" % (channels, Cx, shape)
    per_image = widest(H, W) if callable(widest) else max(Cx, widest) * H * W
    if Nb > 65535 or Nb * per_image >= 2 ** 31:
        return "x is too large for 32-bit indexing (%s)" % (tuple(x.shape),)
    return None


def _placement_reason(x, convs, acts, what=""):
    """After _input_reason: the parameters and the range buffers live where x does.  convs: (weight, quantiser) pairs."""
    for w, q in convs:
        if not CS.native_weight_prep_ok(w, q):
            return what + "a weight is not a float32 GPU tensor"
    for act in acts:
        if act.x_min.device != x.device:
            return what + "a QuantAct's range buffers are not on x's device"
    return None
