"""The caller side of the hot path: a ``PoseShuffleNetV2`` with the
reference's module tree / state-dict keys (lib/models/networks/shufflenetv2_dcn.py:57-114,189-330) whose
``deconv_layers`` are this package's deform modules, ``ctdet_decode`` (lib/models/decode.py:10-16,110-127,474-505; a torch
restatement for CPU tensors and ``ctdet_decode_native`` on the HIP kernels) and the body of ``CtdetDetector.process``
(lib/detectors/ctdet.py:29-46).  Module by module every operator of the three deform stages runs on the hand-written
kernels; ``enable_fused()`` runs the WHOLE network on them -- backbone (pipeline.FusedBackbone), stages
(pipeline.FusedHotPath), heads (pipeline.FusedHeads) -- and ``enable_fused(frozen_codes=True)`` the byte-code serving
schedule (pipeline.FrozenBackbone / FrozenHotPath / FusedHeads.forward_codes); ``capture_process`` records network +
decode as one HIP graph; ``process_scales`` / ``capture_process_scales`` run the S test scales of a multi-scale test as one
batch and merge them on the GPU (``merge_scales_native``: post_process + soft-NMS + the max_per_image cut).
"""
import hashlib

import torch
import torch.nn as nn
import torch.nn.functional as F

from .modules import dcn_deform_conv
from .portable_quantizer.quant_modules import channel_shuffle

BN_MOMENTUM = 0.1


class BaseNode(nn.Module):
    """ShuffleNetV2 unit: stride 1 = split / transform one half / concat / shuffle; stride 2 = two
    transformed branches (reference :57-114)."""

    def __init__(self, inp, oup, stride, batch_norm=nn.BatchNorm2d, conv_kernel=nn.Conv2d):
        super().__init__()
        self.stride = stride
        half = oup // 2

        def pw(i, o):
            return [nn.Conv2d(i, o, 1, 1, 0, bias=False), batch_norm(o, momentum=BN_MOMENTUM)]

        def dw(c, s):
            return [conv_kernel(c, c, 3, s, 1, groups=c, bias=False), batch_norm(c, momentum=BN_MOMENTUM)]

        if stride == 1:
            self.b2 = nn.Sequential(*pw(half, half), nn.ReLU(inplace=True), *dw(half, 1),
                                    *pw(half, half), nn.ReLU(inplace=True))
        elif stride == 2:
            self.b1 = nn.Sequential(*dw(inp, 2), *pw(inp, half), nn.ReLU(inplace=True))
            self.b2 = nn.Sequential(*pw(inp, half), nn.ReLU(inplace=True), *dw(half, 2),
                                    *pw(half, half), nn.ReLU(inplace=True))

    def forward(self, x):
        if self.stride == 1:
            half = x.shape[1] // 2
            x1, x2 = x[:, :half], self.b2(x[:, half:])
        else:
            x1, x2 = self.b1(x), self.b2(x)
        return channel_shuffle(torch.cat((x1, x2), 1), 2)


class PoseShuffleNetV2(nn.Module):
    """Backbone (stride 32) -> three deform up-sampling stages -> heads (reference :189-330).
    forward returns ``[ {head: tensor} ]`` like the reference."""

    def __init__(self, heads, head_conv, w2=None, deform=False, maxpool=False):
        super().__init__()
        self.w2 = w2
        self.deform_backbone = deform
        self.heads = heads
        self.deconv_with_bias = False
        self.channels = [24, 244, 488, 976, 2153] if w2 else [24, 116, 232, 464, 1024]
        c = self.channels
        stem = [nn.Conv2d(3, c[0], 3, 2 if maxpool else 4, 1, bias=False),
                nn.BatchNorm2d(c[0], momentum=BN_MOMENTUM), nn.ReLU(inplace=True)]
        if maxpool:
            stem.append(nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
        self.layer0 = nn.Sequential(*stem)
        # deform=True (reference :216-230; its factory never passes it): the units' 3x3 convs are CoDeNet operators
        kern = dcn_deform_conv.DeformConvWithOffsetScaleBoundPositive if deform else nn.Conv2d
        for idx, reps in enumerate([3, 7, 3]):
            nodes = [BaseNode(c[idx], c[idx + 1], 2, nn.BatchNorm2d, kern)]
            nodes += [BaseNode(c[idx], c[idx + 1], 1, nn.BatchNorm2d, kern) for _ in range(reps)]
            setattr(self, "layer%d" % (idx + 1), nn.Sequential(*nodes))
        self.layer4 = nn.Sequential(nn.Conv2d(c[3], c[4], 1, 1, 0, bias=False),
                                    nn.BatchNorm2d(c[4], momentum=BN_MOMENTUM), nn.ReLU(inplace=True))
        layers = []
        planes_in = [c[4], 256, 128]
        for cin, cout in zip(planes_in, [256, 128, 64]):
            layers += [dcn_deform_conv.DeformConvWithOffsetScaleBoundPositive(
                           cin, cout, 3, 1, 1, groups=cout, bias=False, hidden_state=128,
                           BN_MOMENTUM=BN_MOMENTUM),
                       nn.BatchNorm2d(cout, momentum=BN_MOMENTUM), nn.ReLU(inplace=True),
                       nn.Upsample(scale_factor=2, mode="nearest")]
        self.deconv_layers = nn.Sequential(*layers)
        for head, classes in heads.items():
            if head_conv > 0:
                fc = nn.Sequential(
                    nn.Conv2d(64, head_conv, 1, 1, 0, bias=False),
                    nn.BatchNorm2d(head_conv, momentum=BN_MOMENTUM), nn.ReLU(inplace=True),
                    nn.Conv2d(head_conv, head_conv, 3, 1, 1, groups=head_conv, bias=False),
                    nn.BatchNorm2d(head_conv, momentum=BN_MOMENTUM), nn.ReLU(inplace=True),
                    nn.Conv2d(head_conv, classes, kernel_size=1, stride=1, padding=0, bias=True))
            else:
                fc = nn.Conv2d(64, classes, kernel_size=1, stride=1, padding=0, bias=True)
            setattr(self, head, fc)

    def enable_fused(self, flag=True, backbone=True, frozen_codes=False, frozen_backbone=True):
        """Inference on GPU tensors: run deconv_layers AND the heads on the fused HIP schedules
        (pipeline.FusedHotPath.forward_nhwc -> pipeline.FusedHeads; nothing is materialised between
        them) and, for a W4A8 model (backbone=True), layer0..layer4 on pipeline.FusedBackbone.  The
        returned tensors are static buffers, overwritten by the next call.

        frozen_codes (serving mode; needs every QuantAct of deconv_layers at running_stat False, e.g. after
        pipeline.set_running_stat(model, False)): the three deform stages run on the byte-code schedule
        (pipeline.FrozenHotPath, chained scale sums), and -- frozen_backbone, when the QuantActs of layer0..layer4
        are frozen too and pipeline.FrozenBackbone.supported(model) -- the backbone on byte codes as well, so that
        every activation between the image and the heads crosses HBM as one byte.  The reference does not clamp
        activation codes, a byte must: check ``frozen_overflowed()`` after a batch and recompute it with frozen_codes
        off if it says True (pipeline.cover_frozen_ranges widens EMA ranges over calibration batches beforehand)."""
        from .portable_quantizer.quant_modules import QuantAct
        self._fused = bool(flag)
        self._fused_backbone = bool(backbone)
        self._frozen_codes = bool(frozen_codes)
        self._frozen_backbone = bool(frozen_backbone)
        self._fpath = self._fheads = self._fbackbone = self._ffrozen = self._fzbackbone = self._fzheads = None
        # the QuantActs whose settings key _plan(): collected once (the module tree is fixed after
        # quantize_shufflenetv2_dcn), so a forward reads 6 attributes of ~70 modules instead of walking the tree
        self.__dict__["_fused_acts"] = [a for a in self.modules() if isinstance(a, QuantAct)]
        self.__dict__["_plans"] = {}
        return self

    def byte_backbone(self):
        """The byte-code backbone (pipeline.FrozenBackbone) once a call on the serving schedule has built it, else None."""
        return getattr(self, "_fzbackbone", None)

    def overflowed_acts(self):
        """The QuantActs whose byte codes saturated since the last call (synchronises; resets the flags): every launch of
        the byte-code stages, heads and backbone names the QuantAct(s) it writes codes of (pipeline.OverflowFlags)."""
        out = []
        for f in (getattr(self, "_ffrozen", None), getattr(self, "_fzbackbone", None)):
            if f is not None and f._bufs is not None:
                out += [a for a in f._bufs["overflow"].acts() if all(a is not b for b in out)]
        return out

    def frozen_overflowed(self):
        """True when a code of the byte-code schedule saturated since the last call (synchronises, resets)."""
        return bool(self.overflowed_acts())

    def _plan(self, x):
        """The schedule of a call without autograd on the GPU tensor `x`: (schedule, byte_backbone, byte_heads) with
        schedule "fused" (the whole network on the fp32 fused schedules), "bytes" (the deform stages on byte codes; the
        backbone and the heads on them too where byte_backbone / byte_heads), "stages" (the deform stages alone on the
        fused schedule, the rest module by module) or "module".  The fused schedules implement the reference's default
        QuantAct settings (stored planes beyond the LDS-resident gather -- inputs above ~1100 px -- are gathered from
        global memory); anything else (--act-percentile in backbone / heads, symmetric activations) keeps the module
        path around the deform stages.  Decided BEFORE any kernel runs, so no QuantAct state is half-updated, and per
        (input shape, QuantAct configuration), not once: a backbone frozen after the stages is picked up.  Builds the
        schedule objects it picks on first use."""
        from . import pipeline
        from .portable_quantizer.quant_modules import QuantAct
        cfg = tuple((a.percentile, a.quant_mode, a.full_precision_flag, a.activation_bit, a.running_stat,
                     getattr(a, "global_range", False)) for a in self.__dict__["_fused_acts"])
        key = (tuple(x.shape), cfg)
        plans = self.__dict__["_plans"]
        if key in plans:
            return plans[key]
        Nb, _, R, R2 = x.shape
        stem = self.layer0[0].conv if hasattr(self.layer0[0], "conv") else self.layer0[0]
        down = stem.stride[0] * (2 if any(isinstance(m, nn.MaxPool2d) for m in self.layer0.modules()) else 1) * 8
        feat = (Nb, self.channels[4], -(-R // down), -(-R2 // down))        # layer4's output shape
        plan = ("module", False, False)
        if (R % down == 0 and R2 % down == 0 and feat[2] > 0 and feat[3] > 0
                and pipeline.FusedHotPath.supported(self.deconv_layers, feat)
                and pipeline.FusedHeads.supported({hd: getattr(self, hd) for hd in self.heads})):
            if self._fpath is None:
                self._fpath = pipeline.FusedHotPath(self.deconv_layers)
            if self._fheads is None:
                self._fheads = pipeline.FusedHeads({h: getattr(self, h) for h in self.heads})
                self._fbackbone = (pipeline.FusedBackbone(self)
                                   if self._fused_backbone and pipeline.FusedBackbone.supported(self) else None)
            plan = ("fused", False, False)
            stage_acts = [a for a in self.deconv_layers.modules() if isinstance(a, QuantAct)]
            last = (self._frozen_codes and stage_acts and not any(a.running_stat for a in stage_acts)
                    and pipeline.FrozenHotPath.planes_fit(self.deconv_layers, feat))
            if last:
                if self._ffrozen is None:
                    self._ffrozen = pipeline.FrozenHotPath(self.deconv_layers, chain_scale=True)
                byte_backbone = bool(self._fbackbone is not None and self._frozen_backbone
                                     and pipeline.FrozenBackbone.supported(self))
                if byte_backbone and self._fzbackbone is None:
                    self._fzbackbone = pipeline.FrozenBackbone(self)
                byte_heads = byte_backbone and last["codes"]
                if byte_heads and self._fzheads is None:
                    self._fzheads = pipeline.FusedHeads({h: getattr(self, h) for h in self.heads})
                plan = ("bytes", byte_backbone, bool(byte_heads and self._fzheads.codes_supported(last)))
        else:
            import warnings
            warnings.warn("codenet_amd: enable_fused() does not cover this model configuration / input "
                          "shape %s; running the module-by-module path (the deform stages alone stay on the "
                          "fused schedule where it implements them, e.g. --act-percentile)" % (tuple(x.shape),))
            if pipeline.FusedHotPath.supported(self.deconv_layers, feat):
                if self._fpath is None:
                    self._fpath = pipeline.FusedHotPath(self.deconv_layers)
                plan = ("stages", False, False)
        plans[key] = plan
        return plan

    def forward(self, x):
        fused = getattr(self, "_fused", False) and x.is_cuda and not torch.is_grad_enabled()
        schedule, byte_backbone, byte_heads = self._plan(x) if fused else ("module", False, False)
        if byte_backbone:            # byte codes from the image to the heads
            stages, fz = self._ffrozen, self._fzbackbone
            # the QuantAct parameters of the stages and the heads in the backbone's first launch (once their buffers
            # exist: from the second call on) -- two launches fewer in the chain
            also, sb = None, stages._bufs
            hb = self._fzheads._bufs if self._fzheads is not None else None
            if (sb is not None and hb is not None and hb.get("acts") is not None and sb.get("acts") is not None
                    and getattr(self, "merge_frozen_params", True)):      # (A/B switch: tools/e2e_frozen_bench.py)
                also = (list(sb["acts"]) + list(hb["acts"]), sb.get("sums_all"))
            feat8, fq, hw = fz(x, also=also)
            r8, rq, last = stages.forward_codes(feat8, fq, hw, covered=fz.covered)
            if byte_heads:
                return [self._fzheads.forward_codes(r8, rq, last, stages.head_flags(), covered=fz.covered)]
            return [self._fheads(*stages.expand(r8, rq, last))]
        if schedule in ("fused", "bytes"):
            if self._fbackbone is not None:       # W4A8: the whole network on the HIP kernels
                stages = self._ffrozen if schedule == "bytes" else self._fpath
                feat, fq, hw = self._fbackbone(x)       # hw None: an NCHW tensor (odd channel count)
                return [self._fheads(*stages.forward_nhwc(feat, fq, hw))]
            x = self.layer4(self.layer3(self.layer2(self.layer1(self.layer0(x)))))
            return [self._fheads(*self._fpath.forward_nhwc(x))]
        # == self.layer4(self.layer3(self.layer2(self.layer1(self.layer0(x))))); the quantised stem, units and layer4 of a
        # QAT step as native autograd functions (functions/codenet_stem.py, functions/codenet_units.py)
        from .functions.codenet_stem import forward_stem
        from .functions.codenet_units import forward_layer4, forward_units
        x = forward_stem(self.layer0, x)
        for layer in (self.layer1, self.layer2, self.layer3):
            x = forward_units(layer, x)
        x = forward_layer4(self.layer4, x)
        if schedule == "stages":      # one C call per stage + unpack, the rest module by module
            x = self._fpath(x)
        else:
            from .functions.codenet_stage import forward_stage_blocks
            x = forward_stage_blocks(self.deconv_layers, x)      # == self.deconv_layers(x); fused blocks in the QAT step
        from .functions.codenet_heads import forward_heads
        # == {head: getattr(self, head)(x)}; the quantised heads of a QAT step as one native autograd function
        return [forward_heads({head: getattr(self, head) for head in self.heads}, x)]


def fill_state_dict_(model, seed=317):
    """Deterministic, construction-order independent synthetic weights: every tensor is drawn from a
    generator seeded by (seed, state-dict key), so two models with the same keys (this package's
    and the reference's) get identical values.  Scales keep activations O(1) through the net and
    make conv_scale non-degenerate."""
    sd = model.state_dict()
    with torch.no_grad():
        for key in sorted(sd):
            t = sd[key]
            if not t.dtype.is_floating_point:
                continue
            h = int(hashlib.sha256(("%d:%s" % (seed, key)).encode()).hexdigest()[:12], 16)
            g = torch.Generator().manual_seed(h)
            shape = tuple(t.shape)
            if key.endswith("running_var"):
                v = torch.rand(shape, generator=g) + 0.5
            elif key.endswith("running_mean"):
                v = torch.randn(shape, generator=g) * 0.1
            elif key.endswith(("x_min", "x_max")):
                v = torch.zeros(shape)
            elif "conv_scale" in key and key.endswith("weight"):
                v = torch.randn(shape, generator=g) * (3.0 / max(1, t[0].numel()) ** 0.5)
            elif "conv_scale" in key and key.endswith("bias"):
                v = torch.ones(shape)
            elif t.dim() == 4:                       # conv weight: variance preserving
                fan_in = t.shape[1] * t.shape[2] * t.shape[3]
                v = torch.randn(shape, generator=g) * (1.2 / fan_in) ** 0.5
            elif key.endswith("weight"):             # BN gamma
                v = torch.rand(shape, generator=g) + 0.5
            elif key in ("hm.6.bias", "hm.quant_conv.bias", "hm.bias"):   # CenterNet focal-loss prior
                v = torch.full(shape, -2.19)
            else:                                    # BN beta / conv bias
                v = torch.randn(shape, generator=g) * 0.1
            t.copy_(v.to(t.device))
    return model


# ---- decode (lib/models/decode.py, lib/models/utils.py) ---------------------------------------

def _nms(heat, kernel=3):
    hmax = F.max_pool2d(heat, (kernel, kernel), stride=1, padding=(kernel - 1) // 2)
    return heat * (hmax == heat).float()


def _gather_feat(feat, ind):
    return feat.gather(1, ind.unsqueeze(2).expand(ind.size(0), ind.size(1), feat.size(2)))


def _transpose_and_gather_feat(feat, ind):
    feat = feat.permute(0, 2, 3, 1).contiguous()
    return _gather_feat(feat.view(feat.size(0), -1, feat.size(3)), ind)


def _topk(scores, K=40):
    batch, cat, height, width = scores.size()
    topk_scores, topk_inds = torch.topk(scores.view(batch, cat, -1), K)
    topk_inds = topk_inds % (height * width)
    topk_ys = torch.div(topk_inds, width, rounding_mode="floor").float()
    topk_xs = (topk_inds % width).float()
    topk_score, topk_ind = torch.topk(topk_scores.view(batch, -1), K)
    topk_clses = torch.div(topk_ind, K, rounding_mode="floor").int()
    topk_inds = _gather_feat(topk_inds.view(batch, -1, 1), topk_ind).view(batch, K)
    topk_ys = _gather_feat(topk_ys.view(batch, -1, 1), topk_ind).view(batch, K)
    topk_xs = _gather_feat(topk_xs.view(batch, -1, 1), topk_ind).view(batch, K)
    return topk_score, topk_inds, topk_clses, topk_ys, topk_xs


def ctdet_decode(heat, wh, reg=None, cat_spec_wh=False, K=100):
    """3x3 max-pool peak filter -> two-level top-K -> boxes [x1,y1,x2,y2,score,class]."""
    batch, cat, height, width = heat.size()
    heat = _nms(heat)
    scores, inds, clses, ys, xs = _topk(heat, K=K)
    if reg is not None:
        reg = _transpose_and_gather_feat(reg, inds).view(batch, K, 2)
        xs = xs.view(batch, K, 1) + reg[:, :, 0:1]
        ys = ys.view(batch, K, 1) + reg[:, :, 1:2]
    else:
        xs = xs.view(batch, K, 1) + 0.5
        ys = ys.view(batch, K, 1) + 0.5
    wh = _transpose_and_gather_feat(wh, inds)
    if cat_spec_wh:
        wh = wh.view(batch, K, cat, 2)
        wh = wh.gather(2, clses.view(batch, K, 1, 1).expand(batch, K, 1, 2).long()).view(batch, K, 2)
    else:
        wh = wh.view(batch, K, 2)
    clses = clses.view(batch, K, 1).float()
    scores = scores.view(batch, K, 1)
    bboxes = torch.cat([xs - wh[..., 0:1] / 2, ys - wh[..., 1:2] / 2,
                        xs + wh[..., 0:1] / 2, ys + wh[..., 1:2] / 2], dim=2)
    return torch.cat([bboxes, scores, clses], dim=2)


class ProcessBuffers:
    """Static buffers of the native post-processing -- the sigmoid copy of `hm` and the decode workspace -- keyed by
    (device, shape / size, stream).  OWNED: one instance lives on the model (`process`) or in the replay closure of a
    captured graph (`capture_process`, which runs on its own side stream), so the buffers die with their owner and
    two models / graphs of the same shape never share an `hm` a caller still holds."""

    def __init__(self):
        self.sigmoid = {}
        self.decode_ws = {}
        self.merge_ws = {}

    def sigmoid_buffer(self, hm, tag="hm"):
        # `tag` keeps the merged hm and wh of a flip test apart: a 2-class model gives both the shape [1,2,H,W]
        key = (tag, hm.device, tuple(hm.shape), torch.cuda.current_stream(hm.device).cuda_stream)
        if key not in self.sigmoid:
            self.sigmoid[key] = torch.empty_like(hm)
        return self.sigmoid[key]

    def workspace(self, device, need, stream):
        # its histograms must be zero at entry and are left zero by every call, so concurrent calls on
        # different streams must not share one
        key = (device, need, stream.cuda_stream)
        if key not in self.decode_ws:
            self.decode_ws[key] = torch.zeros(need // 4 + 64, dtype=torch.int32, device=device)
        return self.decode_ws[key]


    def merge_block(self, device, need, stream, tag="results"):
        # the result block of cdn_ctdet_merge_scales (boxes, row counts, thresholds back to back: one copy fetches all)
        # and, tag "meta", the device copy of the crop parameters
        key = (tag, device, need, stream.cuda_stream)
        if key not in self.merge_ws:
            self.merge_ws[key] = torch.zeros(need // 8 + 1, dtype=torch.float64, device=device)
        return self.merge_ws[key]


class _BoundedBuffers(ProcessBuffers):
    """Owner-less calls of ctdet_decode_native: at most `cap` workspaces are kept (oldest dropped first).  A captured
    graph keeps the raw workspace pointer, so an owner-less call under stream capture is refused: capture with an
    owner (`bufs=ProcessBuffers()` kept alive next to the graph; capture_process does that)."""
    cap = 4

    def workspace(self, device, need, stream):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ctdet_decode_native under graph capture needs bufs=ProcessBuffers() owned by the "
                               "capture (the graph keeps the workspace pointer; the shared default cache evicts)")
        ws = super().workspace(device, need, stream)
        while len(self.decode_ws) > self.cap:
            self.decode_ws.pop(next(iter(self.decode_ws)))
        return ws

    def merge_block(self, device, need, stream, tag="results"):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("merge_scales_native under graph capture needs bufs=ProcessBuffers() owned by the capture")
        blk = super().merge_block(device, need, stream, tag)
        while len(self.merge_ws) > 2 * self.cap:
            self.merge_ws.pop(next(iter(self.merge_ws)))
        return blk


_default_bufs = _BoundedBuffers()


def ctdet_decode_native(heat, wh, reg=None, cat_spec_wh=False, K=100, apply_sigmoid=False,
                        heat_out=None, bufs=None):
    """ctdet_decode on the HIP kernels (codenet_decode.hip, cdn_ctdet_decode): same arguments and result
    as ``ctdet_decode``; apply_sigmoid=True takes logits (heat_out, if given, receives the sigmoid).
    Equal scores are ordered by ascending flat index.  GPU float32 tensors only."""
    from . import _native as N_
    if not (heat.is_cuda and heat.dtype == torch.float32):
        raise NotImplementedError("ctdet_decode_native needs float32 GPU tensors")
    heat, wh = heat.contiguous(), wh.contiguous()
    reg = reg.contiguous() if reg is not None else None
    B, cat, H, W = heat.shape
    lib = N_.lib()
    need = lib.cdn_ctdet_decode_workspace_bytes(B, cat, H, W)
    # one workspace per (owner, device, size, stream); `bufs` = the owner's ProcessBuffers (a captured graph keeps
    # the raw pointer, so its owner must outlive the graph: capture_process keeps it in the replay closure)
    stream = torch.cuda.current_stream(heat.device)
    ws = (bufs if bufs is not None else _default_bufs).workspace(heat.device, need, stream)
    ws_ptr = N_.aligned_workspace(ws)[0]
    dets = torch.empty(B, K, 6, device=heat.device)
    rc = lib.cdn_ctdet_decode(heat.data_ptr(), wh.data_ptr(), reg.data_ptr() if reg is not None else None,
                              B, cat, H, W, int(bool(cat_spec_wh)), K, int(bool(apply_sigmoid)),
                              heat_out.data_ptr() if heat_out is not None else None, dets.data_ptr(),
                              ws_ptr, need, stream.cuda_stream)
    N_.check(rc, "cdn_ctdet_decode")
    return dets


def process(model, images, flip_test=True, reg_offset=True, cat_spec_wh=False, K=100, native_decode=None,
            bufs=None):
    """CtdetDetector.process (lib/detectors/ctdet.py:29-46): images [2,3,R,R] = image + its W-flip
    when flip_test.  Returns (output dict, dets [B,K,6]).  native_decode (default: on GPU tensors) runs
    the peak filter / top-K / box assembly on the HIP kernels, without flip_test fused with the sigmoid."""
    if bufs is None and isinstance(model, nn.Module):
        bufs = model.__dict__.setdefault("_process_bufs", ProcessBuffers())      # owned by (and freed with) the model
    with torch.no_grad():
        output = model(images)[-1]
        if native_decode is None:
            native_decode = output["hm"].is_cuda
        reg = output["reg"] if reg_offset else None
        if native_decode and not flip_test:
            hm = output["hm"]
            # the reference's in-place hm.sigmoid_() (ctdet.py:32): the sigmoid goes to a second static buffer
            # that replaces output["hm"] (in place it would cost a second kernel, see cdn_ctdet_decode)
            # (a model on the fused path returns static buffers anyway; the module-by-module path returns fresh
            # tensors per call, so its sigmoid is a fresh tensor too)
            static = bufs is not None and getattr(model, "_fused", False)
            sig = bufs.sigmoid_buffer(hm) if static else torch.empty_like(hm)
            dets = ctdet_decode_native(hm, output["wh"], reg=reg, cat_spec_wh=cat_spec_wh, K=K,
                                       apply_sigmoid=True, heat_out=sig, bufs=bufs)
            output = dict(output)
            output["hm"] = sig
            return output, dets
        if native_decode and flip_test and output["hm"].shape[0] == 2 and not cat_spec_wh:
            # the README's test commands (--flip_test): sigmoid + mirror merge in one launch into static buffers, then
            # the native decode (capturable as a graph: capture_process(flip_test=True))
            from . import _native as N_
            hm2, wh2 = output["hm"].contiguous(), output["wh"].contiguous()
            static = bufs is not None and getattr(model, "_fused", False)
            hm = bufs.sigmoid_buffer(hm2[0:1], "hm") if static else torch.empty_like(hm2[0:1])
            wh = bufs.sigmoid_buffer(wh2[0:1], "wh") if static else torch.empty_like(wh2[0:1])
            rc = N_.lib().cdn_ctdet_flip_merge(hm2.data_ptr(), wh2.data_ptr(), 1, hm2.shape[1], wh2.shape[1], hm2.shape[2],
                                               hm2.shape[3], hm.data_ptr(), wh.data_ptr(),
                                               torch.cuda.current_stream(hm2.device).cuda_stream)
            N_.check(rc, "cdn_ctdet_flip_merge")
            dets = ctdet_decode_native(hm, wh, reg=reg[0:1] if reg is not None else None, cat_spec_wh=False, K=K,
                                       bufs=bufs)
            if hm2.data_ptr() != output["hm"].data_ptr():      # (contiguous() copied: hand the sigmoid back)
                output = dict(output)
                output["hm"] = hm2
            return output, dets         # output["hm"] holds the sigmoid of both images, as after the reference's sigmoid_()
        hm = output["hm"].sigmoid_()
        wh = output["wh"]
        if flip_test:
            hm = (hm[0:1] + torch.flip(hm[1:2], [3])) / 2
            wh = (wh[0:1] + torch.flip(wh[1:2], [3])) / 2
            reg = reg[0:1] if reg is not None else None
        if native_decode:
            dets = ctdet_decode_native(hm, wh, reg=reg, cat_spec_wh=cat_spec_wh, K=K, bufs=bufs)
        else:
            dets = ctdet_decode(hm, wh, reg=reg, cat_spec_wh=cat_spec_wh, K=K)
    return output, dets


def capture_process(model, images, reg_offset=True, cat_spec_wh=False, K=100, flip_test=False, pre=None):
    """Capture ``process(model, images, flip_test)`` -- the whole fused network + native decode (flip_test: images =
    [image, its W-mirror] and the native sigmoid + mirror merge in between, the README's test procedure) -- over the
    static `images` buffer into one HIP graph (about 110 kernel launches; at small batches the Python /
    launch overhead of issuing them one by one dominates).  Returns replay() -> (output dict, dets); copy
    new images into `images` before each replay.  Needs model.enable_fused() and a GPU tensor.
    pre (a preproc.PreProcess that has an image loaded): ``pre.run(images)`` becomes the first node of the graph, so a
    replay needs only ``pre.load(next image)`` -- the image bytes and the crop table, not the float planes."""
    assert getattr(model, "_fused", False) and images.is_cuda
    bufs = ProcessBuffers()          # owned by this capture: kept alive by replay(), released with it
    kw = dict(flip_test=bool(flip_test), reg_offset=reg_offset, cat_spec_wh=cat_spec_wh, K=K, bufs=bufs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                 # warm-up: buffers, cached weights, kernel attributes
        for _ in range(3):
            if pre is not None:
                pre.run(images)
            process(model, images, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    # capture ON the warm-up stream: the static buffers are keyed by stream, so a capture stream of its own allocated
    # them again INSIDE the capture -- and the zero fill of the 84-MB decode workspace became a graph node, replayed
    # with every batch (12 us + a boundary in the kernel trace of round 4)
    with torch.cuda.graph(graph, stream=side):
        if pre is not None:
            pre.run(images)
        result = process(model, images, **kw)

    def replay():
        graph.replay()
        return result
    replay.buffers = bufs
    return replay


# ---- multi-scale test / --nms (test.py --test_scales / --nms; lib/detectors/base_detector.py:84-130, ctdet.py:48-74) ----

def scale_metas(metas, scales):
    """[B][S] meta dicts of pre_process ({'c', 's', 'out_height', 'out_width'}; a flat list of S dicts = one image) and
    the S test scales -> float64 tensor [B, S, 6] = {c_x, c_y, s, out_w, out_h, scale}, the layout cdn_ctdet_merge_scales
    reads."""
    if metas and isinstance(metas[0], dict):
        metas = [metas]
    rows = [[[float(m["c"][0]), float(m["c"][1]), float(m["s"]), float(m["out_width"]), float(m["out_height"]),
              float(sc)] for m, sc in zip(per_image, scales)] for per_image in metas]
    t = torch.tensor(rows, dtype=torch.float64)
    assert t.dim() == 3 and t.shape[1] == len(scales), "one meta per (image, scale)"
    return t


def unpack_merged(block, B, num_classes, R):
    """The result block of cdn_ctdet_merge_scales as a HOST tensor -> per image {class 1 .. num_classes: float32 [n, 5]}
    (what evalio.merge_outputs returns), plus the raw counters."""
    import numpy as np
    raw = block.numpy().view(np.uint8)
    r256 = lambda n: (n + 255) // 256 * 256
    nb, nc = r256(B * num_classes * R * 20), r256(B * num_classes * 4)
    boxes = raw[:B * num_classes * R * 20].view(np.float32).reshape(B, num_classes, R, 5)
    rows_out, rows_in, live = (raw[nb + i * nc: nb + i * nc + B * num_classes * 4].view(np.int32).reshape(B, num_classes)
                               for i in range(3))
    thresh = raw[nb + 3 * nc: nb + 3 * nc + B * 4].view(np.float32)
    results = [{j + 1: boxes[b, j, :rows_out[b, j]].copy() for j in range(num_classes)} for b in range(B)]
    return results, {"rows_out": rows_out, "rows_in": rows_in, "live": live, "thresh": thresh}


def merge_scales_native(dets, metas, scales, num_classes, max_per_image=100, nms=None, bufs=None, raw=False,
                        sigma=0.5, Nt=0.5, threshold=0.001, method=2):
    """CtdetDetector.post_process of every test scale + merge_outputs on the GPU (codenet_merge.hip,
    cdn_ctdet_merge_scales): dets [B, S, K, 6] (or [S, K, 6]: one image) float32 GPU detections as ctdet_decode_native
    writes them, metas [B][S] dicts of pre_process (or the float64 [B, S, 6] tensor of scale_metas, on the GPU for a
    captured graph), scales the S test scales.  nms None = the reference's rule `len(scales) > 1 or opt.nms` with
    opt.nms False.  Returns a list with one {class: float32 [n, 5]} dict per image after ONE device-to-host copy;
    raw=True returns the device tensors (block, boxes, rows_out, rows_in, live, thresh) and copies nothing.  The
    defaults of sigma / Nt / threshold / method are merge_outputs' call soft_nms(results[j], Nt=0.5, method=2)."""
    from . import _native as N_
    if not (dets.is_cuda and dets.dtype == torch.float32):
        raise NotImplementedError("merge_scales_native needs float32 GPU detections")
    if dets.dim() == 3:
        dets = dets.unsqueeze(0)
    dets = dets.contiguous()
    B, S, K, six = dets.shape
    assert six == 6 and S == len(scales), "dets [B, S, K, 6] with one entry per test scale"
    if nms is None:
        nms = S > 1
    lib = N_.lib()
    owner = bufs if bufs is not None else _default_bufs
    stream = torch.cuda.current_stream(dets.device)
    if isinstance(metas, torch.Tensor):
        meta = metas
        if not meta.is_cuda:
            dev_meta = owner.merge_block(dets.device, B * S * 48, stream, "meta")
            dev_meta[:B * S * 6].copy_(meta.reshape(-1))
            meta = dev_meta
    else:
        dev_meta = owner.merge_block(dets.device, B * S * 48, stream, "meta")
        dev_meta[:B * S * 6].copy_(scale_metas(metas, scales).reshape(-1))
        meta = dev_meta
    assert meta.dtype == torch.float64 and meta.numel() >= B * S * 6 and meta.is_contiguous()
    R = S * K
    need = lib.cdn_ctdet_merge_scales_workspace_bytes(B, S, K, num_classes)
    block = owner.merge_block(dets.device, need, stream)
    r256 = lambda n: (n + 255) // 256 * 256
    nb, nc = r256(B * num_classes * R * 20), r256(B * num_classes * 4)
    p0 = block.data_ptr()
    rc = lib.cdn_ctdet_merge_scales(dets.data_ptr(), meta.data_ptr(), B, S, K, num_classes, int(max_per_image),
                                    int(bool(nms)), sigma, Nt, threshold, int(method), p0, p0 + nb, p0 + nb + nc,
                                    p0 + nb + 2 * nc, p0 + nb + 3 * nc, stream.cuda_stream)
    N_.check(rc, "cdn_ctdet_merge_scales")
    if raw:
        u8 = block.view(torch.uint8)
        ints = [u8[nb + i * nc: nb + i * nc + B * num_classes * 4].view(torch.int32).view(B, num_classes) for i in range(3)]
        return (block, u8[:B * num_classes * R * 20].view(torch.float32).view(B, num_classes, R, 5), ints[0], ints[1],
                ints[2], u8[nb + 3 * nc: nb + 3 * nc + B * 4].view(torch.float32))
    return unpack_merged(block.cpu(), B, num_classes, R)[0]


def process_scales(model, images, n_scales, flip_test, metas, scales, num_classes=20, reg_offset=True, K=100,
                   max_per_image=100, nms=None, bufs=None, raw=False, batched=False):
    """One image at n_scales test scales (fix_res, the ctdet / pascal default, warps every scale onto the same
    input_h x input_w crop): images [S, 3, R, R], with flip_test [2S, 3, R, R] = the S images followed by their S
    W-mirrors.  Network -> (flip_test: sigmoid + mirror merge of the S pairs, cdn_ctdet_flip_merge with P = S) -> native
    decode of the S maps -> merge_scales_native.  Returns (output dict, dets [S, K, 6], results) with results = the
    {class: [n, 5]} dict of CtdetDetector.run (raw=True: the device tensors of merge_scales_native).  GPU tensors only.

    batched=False (default, reference-faithful): the NETWORK runs once per scale, on [image] or [image, mirror] -- the
    batches the reference's loop over the scales gives it -- and everything behind it on all scales at once.  Bit for
    bit what S ``process`` calls + evalio.post_process + evalio.merge_outputs give, for every model: a QuantAct with
    running ranges takes its statistics from the batch it sees and updates them once per call, and even an fp32 model is
    not bitwise batch-invariant (measured: MIOpen's convolutions and the fused pointwise kernels, whose channel chunk
    follows the batch size, sum in another order at batch 2S than at batch 2: logits move by ~1e-6).
    batched=True: the S (2S) images as ONE network batch -- one pass instead of S; equal to the above up to those
    last-bit / batch-statistics differences, and exactly equal to a batched network run merged on the host."""
    from . import _native as N_
    S = int(n_scales)
    assert images.is_cuda and images.shape[0] == (2 * S if flip_test else S) and len(scales) == S
    if bufs is None and isinstance(model, nn.Module):
        bufs = model.__dict__.setdefault("_process_bufs", ProcessBuffers())
    with torch.no_grad():
        if batched:
            output = model(images)[-1]
        else:
            outs = []
            for s in range(S):
                one = torch.cat([images[s:s + 1], images[S + s:S + s + 1]], 0) if flip_test else images[s:s + 1]
                outs.append({k: v.clone() for k, v in model(one.contiguous())[-1].items()})     # (static buffers)
            output = {k: torch.cat([o[k][0:1] for o in outs] + ([o[k][1:2] for o in outs] if flip_test else []), 0)
                      for k in outs[0]}
        reg = output["reg"] if reg_offset else None
        static = bufs is not None and getattr(model, "_fused", False)
        if flip_test:
            hm2, wh2 = output["hm"].contiguous(), output["wh"].contiguous()
            hm = bufs.sigmoid_buffer(hm2[0:S], "hm") if static else torch.empty_like(hm2[0:S])
            wh = bufs.sigmoid_buffer(wh2[0:S], "wh") if static else torch.empty_like(wh2[0:S])
            rc = N_.lib().cdn_ctdet_flip_merge(hm2.data_ptr(), wh2.data_ptr(), S, hm2.shape[1], wh2.shape[1], hm2.shape[2],
                                               hm2.shape[3], hm.data_ptr(), wh.data_ptr(),
                                               torch.cuda.current_stream(hm2.device).cuda_stream)
            N_.check(rc, "cdn_ctdet_flip_merge")
            dets = ctdet_decode_native(hm, wh, reg=reg[0:S] if reg is not None else None, K=K, bufs=bufs)
            if hm2.data_ptr() != output["hm"].data_ptr():
                output = dict(output)
                output["hm"] = hm2
        else:
            hm = output["hm"]
            sig = bufs.sigmoid_buffer(hm) if static else torch.empty_like(hm)
            dets = ctdet_decode_native(hm, output["wh"], reg=reg, K=K, apply_sigmoid=True, heat_out=sig, bufs=bufs)
            output = dict(output)
            output["hm"] = sig
        results = merge_scales_native(dets.view(1, S, K, 6), metas, scales, num_classes, max_per_image=max_per_image,
                                      nms=nms, bufs=bufs, raw=raw)
    return output, dets, (results if raw else results[0])


def capture_process_scales(model, images, n_scales, flip_test, metas, scales, num_classes=20, reg_offset=True, K=100,
                           max_per_image=100, nms=None, batched=False, pre=None):
    """``process_scales`` over the static `images` buffer as ONE HIP graph.  Returns replay() -> (output dict, dets,
    results) where results is read back from the graph's result block by one copy per replay; replay.meta is the
    float64 [1, S, 6] device tensor of crop parameters the graph reads (scale_metas layout): copy the next image's
    values into it, and its S (2S) pre-processed scales into `images`, before each replay.  pre (a preproc.PreProcess
    with an image loaded): ``pre.run(images)`` is the first node of the graph and fills `images` itself."""
    assert getattr(model, "_fused", False) and images.is_cuda
    S = int(n_scales)
    bufs = ProcessBuffers()
    meta = scale_metas(metas, scales).to(images.device)
    kw = dict(num_classes=num_classes, reg_offset=reg_offset, K=K, max_per_image=max_per_image, nms=nms, bufs=bufs,
              raw=True, batched=batched)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            if pre is not None:
                pre.run(images)
            process_scales(model, images, S, flip_test, meta, scales, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        if pre is not None:
            pre.run(images)
        output, dets, rawres = process_scales(model, images, S, flip_test, meta, scales, **kw)

    def replay():
        graph.replay()
        return output, dets, unpack_merged(rawres[0].cpu(), 1, num_classes, S * K)[0][0]
    replay.buffers = bufs
    replay.meta = meta
    replay.raw = rawres
    replay.graph = graph      # graph.replay() alone leaves the results in replay.raw with no host copy (evalio.DeviceResults)
    return replay


def create_model(heads=None, head_conv=64, w2=False, maxpool=False, quantize=False, seed=317,
                 w_bit=4, a_bit=8, wt_percentile=False, act_percentile=False):
    """PoseShuffleNetV2 with synthetic weights, optionally rewritten to W4A8 like
    lib/detectors/base_detector.py:28-34 does."""
    from .portable_quantizer import quantize_shufflenetv2_dcn
    heads = heads or {"hm": 20, "wh": 2, "reg": 2}
    model = PoseShuffleNetV2(heads, head_conv, w2=w2, maxpool=maxpool)
    fill_state_dict_(model, seed)
    if quantize:
        quantize_shufflenetv2_dcn(model, w_bit, None, a_bit, "symmetric", "asymmetric", True,
                                  wt_percentile, act_percentile, False, w2=w2, maxpool=maxpool)
    return model.eval()
