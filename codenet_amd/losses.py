"""The ctdet training criterion behind the reference's names (lib/models/losses.py, lib/models/utils.py::_sigmoid,
lib/trains/ctdet.py::CtdetLoss, lib/trains/base_trainer.py::ModelWithLoss) and the target maps of
lib/datasets/sample/ctdet.py:87-122 built from object lists.

Two paths, chosen per call by CtdetLoss.native_reason():

* NATIVE (codenet_loss.hip: cdn_ctdet_loss_forward / _backward, cdn_ctdet_targets) for contiguous float32 GPU heads and
  the trainer's default options -- focal hm loss, reg_loss l1 / sl1, reg_offset on / off, wh_weight == 0,
  off_weight == 0, num_stacks >= 1.  One autograd.Function over all heads; sums in a fixed order without floating-point
  atomics (two runs are bit-identical); loss and loss_stats are views of one 8-float device block, nothing synchronises.
* COMPOSED: the reference's arithmetic as plain PyTorch operations, for CPU tensors, other dtypes and every option the
  kernels do not implement (mse_loss, dense_wh, norm_wh, cat_spec_wh, eval_oracle_*).  tests/test_ctdet_loss.py pins it to
  the reference's own results; it is the yardstick the native path is tested against.

output['hm']: the reference replaces it by the clamped sigmoid in every call; its only readers are the validation and
debug paths.  The native path does so when grad mode is off or keep_hm=True is passed, and otherwise leaves the logits
in place.  On the native path a term that is switched off is a zero TENSOR in loss_stats (the reference
leaves the Python int 0).
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

__all__ = ["_sigmoid", "FocalLoss", "RegL1Loss", "RegLoss", "NormRegL1Loss", "RegWeightedL1Loss", "CtdetLoss",
           "ModelWithLoss", "ctdet_targets", "ctdet_loss_native"]


def _sigmoid(x):
    return torch.clamp(x.sigmoid_(), min=1e-4, max=1 - 1e-4)


def _transpose_and_gather_feat(feat, ind):
    feat = feat.permute(0, 2, 3, 1).contiguous()
    feat = feat.view(feat.size(0), -1, feat.size(3))
    return feat.gather(1, ind.unsqueeze(2).expand(ind.size(0), ind.size(1), feat.size(2)))


def _neg_loss(pred, gt):
    """The modified focal loss of CornerNet (losses.py:42-67)."""
    pos_inds = gt.eq(1).float()
    neg_inds = gt.lt(1).float()
    neg_weights = torch.pow(1 - gt, 4)
    loss = 0
    pos_loss = torch.log(pred) * torch.pow(1 - pred, 2) * pos_inds
    neg_loss = torch.log(1 - pred) * torch.pow(pred, 2) * neg_weights * neg_inds
    num_pos = pos_inds.float().sum()
    pos_loss = pos_loss.sum()
    neg_loss = neg_loss.sum()
    if num_pos == 0:
        loss = loss - neg_loss
    else:
        loss = loss - (pos_loss + neg_loss) / num_pos
    return loss


def _reg_loss(regr, gt_regr, mask):
    num = mask.float().sum()
    mask = mask.unsqueeze(2).expand_as(gt_regr).float()
    regr = regr * mask
    gt_regr = gt_regr * mask
    regr_loss = F.smooth_l1_loss(regr, gt_regr, reduction="sum")
    return regr_loss / (num + 1e-4)


class FocalLoss(nn.Module):
    def __init__(self):
        super().__init__()
        self.neg_loss = _neg_loss

    def forward(self, out, target):
        return self.neg_loss(out, target)


class RegLoss(nn.Module):
    """Smooth-L1 regression (--reg_loss sl1): divides by the number of live rows + 1e-4."""

    def forward(self, output, mask, ind, target):
        return _reg_loss(_transpose_and_gather_feat(output, ind), target, mask)


class RegL1Loss(nn.Module):
    """L1 regression (--reg_loss l1): divides by the sum of the EXPANDED mask + 1e-4."""

    def forward(self, output, mask, ind, target):
        pred = _transpose_and_gather_feat(output, ind)
        mask = mask.unsqueeze(2).expand_as(pred).float()
        loss = F.l1_loss(pred * mask, target * mask, reduction="sum")
        return loss / (mask.sum() + 1e-4)


class NormRegL1Loss(nn.Module):
    def forward(self, output, mask, ind, target):
        pred = _transpose_and_gather_feat(output, ind)
        mask = mask.unsqueeze(2).expand_as(pred).float()
        pred = pred / (target + 1e-4)
        target = target * 0 + 1
        loss = F.l1_loss(pred * mask, target * mask, reduction="sum")
        return loss / (mask.sum() + 1e-4)


class RegWeightedL1Loss(nn.Module):
    def forward(self, output, mask, ind, target):
        pred = _transpose_and_gather_feat(output, ind)
        mask = mask.float()
        loss = F.l1_loss(pred * mask, target * mask, reduction="sum")
        return loss / (mask.sum() + 1e-4)


def gen_oracle_map(feat, ind, w, h):
    """lib/utils/oracle_utils.py: every object's feature flooded breadth-first from its cell (eval_oracle_* only)."""
    B, M, D = feat.shape
    out = np.zeros((B, D, h, w), dtype=np.float32)
    for i in range(B):
        vis = np.zeros((h, w), dtype=bool)
        queue = []
        for j in range(M):
            if ind[i][j] > 0:
                x, y = int(ind[i][j] % w), int(ind[i][j] // w)
                out[i, :, y, x] = feat[i][j]
                vis[y, x] = True
                queue.append((x, y, feat[i][j]))
        head = 0
        while head < len(queue):
            x, y, f = queue[head]
            head += 1
            for dx, dy in ((0, 1), (0, -1), (1, 0), (-1, 0)):
                xx, yy = x + dx, y + dy
                if 0 <= xx < w and 0 <= yy < h and not vis[yy, xx]:
                    out[i, :, yy, xx] = f
                    vis[yy, xx] = True
                    queue.append((xx, yy, f))
    return out


# ---- native path ---------------------------------------------------------------------------------------------------

class _CtdetLossFn(torch.autograd.Function):
    """(cfg, hm_gt, wh_gt, reg_gt, ind, reg_mask, keep, hm_0, wh_0, reg_0, hm_1, ...) -> the 8-float result block
    (loss, hm_loss, wh_loss, off_loss, then the denominators backward reads).  wh_s / reg_s None: that term is off."""

    @staticmethod
    def forward(ctx, cfg, hm_gt, wh_gt, reg_gt, ind, reg_mask, keep, *heads):
        from . import _native as N_
        lib = N_.lib()
        S = len(heads) // 3
        hm0 = heads[0]
        N, C, H, W = hm0.shape
        M = ind.shape[1]
        stream = torch.cuda.current_stream(hm0.device).cuda_stream
        need = lib.cdn_ctdet_loss_workspace_bytes(N, C, H, W, M, S)
        ws = torch.empty(need + 256, dtype=torch.uint8, device=hm0.device)
        ws_ptr, ws_bytes = N_.aligned_workspace(ws)
        result = torch.empty(8, dtype=torch.float32, device=hm0.device)
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        for s in range(S):
            hm, wh, reg = heads[3 * s: 3 * s + 3]
            rc = lib.cdn_ctdet_loss_forward(
                hm.data_ptr(), ptr(wh), ptr(reg), hm_gt.data_ptr(), ptr(wh_gt), ptr(reg_gt), ind.data_ptr(),
                reg_mask.data_ptr(), N, C, H, W, M, s, S, cfg["reg_loss"], cfg["hm_weight"], cfg["wh_weight"],
                cfg["off_weight"], ptr(keep[s]) if keep is not None else None, result.data_ptr(), ws_ptr, ws_bytes, stream)
            N_.check(rc, "cdn_ctdet_loss_forward")
        ctx.cfg, ctx.S, ctx.shape = cfg, S, (N, C, H, W, M)
        ctx.save_for_backward(result, hm_gt, wh_gt, reg_gt, ind, reg_mask, *[h for h in heads if h is not None])
        ctx.present = [h is not None for h in heads]
        return result

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_result):
        from . import _native as N_
        lib = N_.lib()
        result, hm_gt, wh_gt, reg_gt, ind, reg_mask, *saved = ctx.saved_tensors
        it = iter(saved)
        heads = [next(it) if p else None for p in ctx.present]
        N, C, H, W, M = ctx.shape
        cfg = ctx.cfg
        go = grad_result.contiguous().float()
        stream = torch.cuda.current_stream(result.device).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731
        grads = []
        for s in range(ctx.S):
            hm, wh, reg = heads[3 * s: 3 * s + 3]
            g = [torch.empty_like(t) if t is not None else None for t in (hm, wh, reg)]
            rc = lib.cdn_ctdet_loss_backward(
                hm.data_ptr(), ptr(wh), ptr(reg), hm_gt.data_ptr(), ptr(wh_gt), ptr(reg_gt), ind.data_ptr(),
                reg_mask.data_ptr(), N, C, H, W, M, ctx.S, cfg["reg_loss"], cfg["hm_weight"], cfg["wh_weight"],
                cfg["off_weight"], result.data_ptr(), go.data_ptr(), g[0].data_ptr(), ptr(g[1]), ptr(g[2]), stream)
            N_.check(rc, "cdn_ctdet_loss_backward")
            grads += g
        return (None,) * 7 + tuple(grads)


def _as(t, dtype):
    return t.to(dtype).contiguous()


def ctdet_loss_native(heads, batch, reg_loss="l1", hm_weight=1.0, wh_weight=0.1, off_weight=1.0, keep=None):
    """heads: one (hm, wh or None, reg or None) triple of contiguous float32 GPU tensors per stack; batch: the target
    entries 'hm', 'ind', 'reg_mask' and, where the term is on, 'wh' / 'reg'.  keep: None or one tensor per stack (or
    None) that receives the clamped sigmoid.  Returns the 8-float result block (see _CtdetLossFn)."""
    for hm, wh, reg in heads:
        for t in (hm, wh, reg):
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise RuntimeError("ctdet_loss_native: heads must be contiguous float32 GPU tensors")
    use_wh, use_reg = heads[0][1] is not None, heads[0][2] is not None
    # the kernels index by these shapes: check them here, where a mistake is an exception and not a stray address
    N, C, H, W = heads[0][0].shape
    M = batch["ind"].shape[1]
    want = {"hm": (N, C, H, W), "ind": (N, M), "reg_mask": (N, M)}
    want.update({"wh": (N, M, 2)} if use_wh else {})
    want.update({"reg": (N, M, 2)} if use_reg else {})
    for k, shape in want.items():
        if tuple(batch[k].shape) != shape or batch[k].device != heads[0][0].device:
            raise RuntimeError("ctdet_loss_native: batch[%r] must be %s on %s" % (k, shape, heads[0][0].device))
    for hm, wh, reg in heads:
        if tuple(hm.shape) != (N, C, H, W) or any((t is not None) != use or (use and tuple(t.shape) != (N, 2, H, W))
                                                  for t, use in ((wh, use_wh), (reg, use_reg))):
            raise RuntimeError("ctdet_loss_native: every stack needs hm %s and wh / reg (N, 2, H, W)" % ((N, C, H, W),))
    cfg ={"reg_loss": {"l1": 0, "sl1": 1}[reg_loss], "hm_weight": float(hm_weight), "wh_weight": float(wh_weight),
           "off_weight": float(off_weight)}
    flat = [t for triple in heads for t in triple]
    return _CtdetLossFn.apply(cfg, _as(batch["hm"], torch.float32), _as(batch["wh"], torch.float32) if use_wh else None,
                              _as(batch["reg"], torch.float32) if use_reg else None, _as(batch["ind"], torch.int64),
                              _as(batch["reg_mask"], torch.uint8), keep, *flat)


_COMPOSED_ONLY = ("mse_loss", "dense_wh", "norm_wh", "cat_spec_wh", "eval_oracle_hm", "eval_oracle_wh",
                  "eval_oracle_offset")


class CtdetLoss(nn.Module):
    """CtdetLoss(opt).forward(outputs, batch) -> (loss, loss_stats), lib/trains/ctdet.py:17-74.  opt needs mse_loss,
    reg_loss, dense_wh, norm_wh, cat_spec_wh, num_stacks, hm_weight, wh_weight, off_weight, reg_offset and the
    eval_oracle_* switches (missing switches read as False)."""

    def __init__(self, opt):
        super().__init__()
        g = lambda k: getattr(opt, k, False)     # noqa: E731
        self.crit = nn.MSELoss() if g("mse_loss") else FocalLoss()
        self.crit_reg = RegL1Loss() if opt.reg_loss == "l1" else RegLoss() if opt.reg_loss == "sl1" else None
        self.crit_wh = nn.L1Loss(reduction="sum") if g("dense_wh") else NormRegL1Loss() if g("norm_wh") else \
            RegWeightedL1Loss() if g("cat_spec_wh") else self.crit_reg
        self.opt = opt

    def native_reason(self, outputs, batch):
        """None when the kernels take this call, else why the composed path does."""
        opt = self.opt
        for k in _COMPOSED_ONLY:
            if getattr(opt, k, False):
                return "option %s" % k
        if opt.reg_loss not in ("l1", "sl1"):
            return "reg_loss %r" % (opt.reg_loss,)
        use_wh, use_reg = opt.wh_weight > 0, bool(opt.reg_offset) and opt.off_weight > 0
        shape = None
        for s in range(opt.num_stacks):
            for k in ["hm"] + ["wh"] * use_wh + ["reg"] * use_reg:
                t = outputs[s][k]
                if not t.is_cuda:
                    return "CPU tensor"
                if t.dtype != torch.float32:
                    return "dtype %s" % t.dtype
                if not t.is_contiguous():
                    return "non-contiguous head"
                if k != "hm" and t.shape[1] != 2:
                    return "%s with %d channels" % (k, t.shape[1])
            if shape not in (None, tuple(outputs[s]["hm"].shape)):
                return "stacks of different shapes"
            shape = tuple(outputs[s]["hm"].shape)
        for k in ["hm", "ind", "reg_mask"] + ["wh"] * use_wh + ["reg"] * use_reg:
            if batch[k].device != outputs[0]["hm"].device:
                return "targets on another device"
        if tuple(batch["hm"].shape) != shape:
            return "target shape"
        return None

    def forward(self, outputs, batch, keep_hm=False):
        if self.native_reason(outputs, batch) is None:
            return self._forward_native(outputs, batch, keep_hm)
        return self._forward_composed(outputs, batch)

    def _forward_native(self, outputs, batch, keep_hm):
        opt = self.opt
        use_wh, use_reg = opt.wh_weight > 0, bool(opt.reg_offset) and opt.off_weight > 0
        heads = [(outputs[s]["hm"], outputs[s]["wh"] if use_wh else None, outputs[s]["reg"] if use_reg else None)
                 for s in range(opt.num_stacks)]
        keep = None
        if keep_hm or not torch.is_grad_enabled():
            keep = [torch.empty_like(h[0]) for h in heads]
        block = ctdet_loss_native(heads, batch, opt.reg_loss, opt.hm_weight, opt.wh_weight, opt.off_weight, keep)
        if keep is not None:
            for s in range(opt.num_stacks):
                outputs[s]["hm"] = keep[s]
        loss_stats = {"loss": block[0], "hm_loss": block[1], "wh_loss": block[2], "off_loss": block[3]}
        return block[0], loss_stats

    def _forward_composed(self, outputs, batch):
        opt = self.opt
        g = lambda k: getattr(opt, k, False)     # noqa: E731
        hm_loss, wh_loss, off_loss = 0, 0, 0
        for s in range(opt.num_stacks):
            output = outputs[s]
            if not g("mse_loss"):
                output["hm"] = _sigmoid(output["hm"])
            if g("eval_oracle_hm"):
                output["hm"] = batch["hm"]
            if g("eval_oracle_wh"):
                output["wh"] = torch.from_numpy(gen_oracle_map(
                    batch["wh"].detach().cpu().numpy(), batch["ind"].detach().cpu().numpy(),
                    output["wh"].shape[3], output["wh"].shape[2])).to(output["wh"].device)
            if g("eval_oracle_offset"):
                output["reg"] = torch.from_numpy(gen_oracle_map(
                    batch["reg"].detach().cpu().numpy(), batch["ind"].detach().cpu().numpy(),
                    output["reg"].shape[3], output["reg"].shape[2])).to(output["reg"].device)
            hm_loss += self.crit(output["hm"], batch["hm"]) / opt.num_stacks
            if opt.wh_weight > 0:
                if g("dense_wh"):
                    mask_weight = batch["dense_wh_mask"].sum() + 1e-4
                    wh_loss += (self.crit_wh(output["wh"] * batch["dense_wh_mask"],
                                             batch["dense_wh"] * batch["dense_wh_mask"]) / mask_weight) / opt.num_stacks
                elif g("cat_spec_wh"):
                    wh_loss += self.crit_wh(output["wh"], batch["cat_spec_mask"], batch["ind"],
                                            batch["cat_spec_wh"]) / opt.num_stacks
                else:
                    wh_loss += self.crit_reg(output["wh"], batch["reg_mask"], batch["ind"], batch["wh"]) / opt.num_stacks
            if opt.reg_offset and opt.off_weight > 0:
                off_loss += self.crit_reg(output["reg"], batch["reg_mask"], batch["ind"], batch["reg"]) / opt.num_stacks
        loss = opt.hm_weight * hm_loss + opt.wh_weight * wh_loss + opt.off_weight * off_loss
        loss_stats = {"loss": loss, "hm_loss": hm_loss, "wh_loss": wh_loss, "off_loss": off_loss}
        return loss, loss_stats


class ModelWithLoss(nn.Module):
    """lib/trains/base_trainer.py:12-21."""

    def __init__(self, model, loss):
        super().__init__()
        self.model = model
        self.loss = loss

    def forward(self, batch):
        outputs = self.model(batch["input"])
        loss, loss_stats = self.loss(outputs, batch)
        return outputs[-1], loss, loss_stats


# ---- target maps ---------------------------------------------------------------------------------------------------

def _gaussian_radius(height, width, min_overlap=0.7):
    b1 = height + width
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 + math.sqrt(b1 ** 2 - 4 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    r2 = (b2 + math.sqrt(b2 ** 2 - 16 * c2)) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    r3 = (b3 + math.sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def _targets_host(boxes, classes, counts, num_classes, out_h, out_w, max_objs):
    """The host composition of cdn_ctdet_targets (numpy; the widths are those of the data loader's code)."""
    N = boxes.shape[0]
    f32 = np.float32
    hm = np.zeros((N, num_classes, out_h, out_w), dtype=f32)
    wh = np.zeros((N, max_objs, 2), dtype=f32)
    reg = np.zeros((N, max_objs, 2), dtype=f32)
    ind = np.zeros((N, max_objs), dtype=np.int64)
    reg_mask = np.zeros((N, max_objs), dtype=np.uint8)
    for b in range(N):
        for k in range(max(0, min(int(counts[b]), max_objs))):
            x1, y1, x2, y2 = (f32(v) for v in boxes[b, k])
            h, w, cls = f32(y2 - y1), f32(x2 - x1), int(classes[b, k])
            if not (h > 0 and w > 0 and 0 <= cls < num_classes):
                continue
            r = max(0, int(_gaussian_radius(math.ceil(h), math.ceil(w))))
            ct = np.array([f32(x1 + x2) / f32(2), f32(y1 + y2) / f32(2)], dtype=f32)
            ct_int = ct.astype(np.int32)
            x, y = int(ct_int[0]), int(ct_int[1])
            sigma = (2 * r + 1) / 6
            gy, gx = np.ogrid[-r:r + 1, -r:r + 1]
            gauss = np.exp(-(gx * gx + gy * gy).astype(np.float64) / (2 * sigma * sigma))
            gauss[gauss < np.finfo(np.float64).eps * gauss.max()] = 0
            left, right = min(x, r), min(out_w - x, r + 1)
            top, bottom = min(y, r), min(out_h - y, r + 1)
            dst = hm[b, cls, y - top:y + bottom, x - left:x + right]
            src = gauss[r - top:r + bottom, r - left:r + right]
            if min(src.shape) > 0 and min(dst.shape) > 0:
                np.maximum(dst, src.astype(f32), out=dst)
            wh[b, k] = w, h
            ind[b, k] = y * out_w + x
            reg[b, k] = ct - ct_int.astype(f32)
            reg_mask[b, k] = 1
    return hm, wh, reg, ind, reg_mask


def ctdet_targets(boxes, classes, counts, num_classes, out_h, out_w, max_objs=None):
    """The target entries of the data loader's batch (lib/datasets/sample/ctdet.py:87-122) from object lists.

    boxes [N, M, 4] float32: x1, y1, x2, y2 in output-map pixels, after the affine map and the clip to the map;
    classes [N, M] integer class ids; counts [N] rows in use per image; max_objs = M when given.
    -> {'hm' [N, num_classes, out_h, out_w], 'wh' [N, M, 2], 'reg' [N, M, 2], 'ind' [N, M] int64, 'reg_mask' [N, M]
    uint8}.  GPU tensors: one launch of cdn_ctdet_targets on the current stream; CPU tensors: the host composition."""
    N, M = boxes.shape[:2]
    if max_objs is not None and max_objs != M:
        raise ValueError("ctdet_targets: boxes hold %d rows per image, max_objs is %d" % (M, max_objs))
    if not boxes.is_cuda:
        out = _targets_host(boxes.detach().float().numpy(), classes.numpy(), counts.numpy(), num_classes, out_h, out_w, M)
        return dict(zip(("hm", "wh", "reg", "ind", "reg_mask"), (torch.from_numpy(a) for a in out)))
    from . import _native as N_
    dev = boxes.device
    boxes, classes, counts = _as(boxes, torch.float32), _as(classes, torch.int32), _as(counts.to(dev), torch.int32)
    hm = torch.empty(N, num_classes, out_h, out_w, device=dev)
    wh, reg = torch.empty(N, M, 2, device=dev), torch.empty(N, M, 2, device=dev)
    ind = torch.empty(N, M, dtype=torch.int64, device=dev)
    reg_mask = torch.empty(N, M, dtype=torch.uint8, device=dev)
    rc = N_.lib().cdn_ctdet_targets(boxes.data_ptr(), classes.data_ptr(), counts.data_ptr(), N, M, num_classes, out_h,
                                    out_w, hm.data_ptr(), wh.data_ptr(), reg.data_ptr(), ind.data_ptr(),
                                    reg_mask.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    N_.check(rc, "cdn_ctdet_targets")
    return {"hm": hm, "wh": wh, "reg": reg, "ind": ind, "reg_mask": reg_mask}
