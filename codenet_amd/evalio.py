"""Checkpoint and evaluation I/O around the detector, host-side mirrors of the
reference's helpers with the same names and argument meaning:

    load_model / save_model          lib/models/model.py:35-100   (checkpoint dict {'epoch', 'state_dict'[, 'optimizer']})
    transform_preds                  lib/utils/image.py:14-19,22-55 (rot = 0: closed form, no cv2)
    ctdet_post_process               lib/utils/post_process.py:86-103
    post_process / merge_outputs     lib/detectors/ctdet.py:48-72
    soft_nms                         lib/models/external/nms.pyx:77-170 (multi-scale test / --nms)
    convert_eval_format / save_results   lib/datasets/dataset/pascal.py:58-79   (results.json for tools/reval.py)
    convert_eval_format_coco / save_results_coco   lib/datasets/dataset/coco.py:87-119 (results.json for COCOeval)
    DeviceResults / GroundTruth / voc_eval_device / coco_eval
                                     detections kept in a device table and scored there (codenet_eval.hip): VOC07 AP
                                     (tools/voc_eval_lib/datasets/voc_eval.py:31-207) and COCOeval's bbox statistics
                                     (evaluateImg / accumulate / summarize), DESIGN.md section 7.4e
    export_w4                        packed 4-bit weight codes + per-channel scales + QuantAct ranges of a
                                     quantised model (what an integer-only deployment of the W4A8 model loads)
"""
import json
import os

import numpy as np
import torch


# ---- checkpoints ---------------------------------------------------------------------------------

def load_model(model, model_path, optimizer=None, resume=False, lr=None, lr_step=None, verbose=True):
    """Reference semantics: strips a DataParallel 'module.' prefix, keeps the model's own tensor where a
    shape differs or a key is missing, loads non-strictly; with resume=True restores the optimizer and
    decays lr by 0.1 for every passed lr_step."""
    say = print if verbose else (lambda *a, **k: None)
    start_epoch = 0
    checkpoint = torch.load(model_path, map_location=lambda storage, loc: storage)
    say("loaded {}, epoch {}".format(model_path, checkpoint["epoch"]))
    state_dict = {}
    for k, v in checkpoint["state_dict"].items():
        state_dict[k[7:] if k.startswith("module") and not k.startswith("module_list") else k] = v
    own = model.state_dict()
    for k in list(state_dict):
        if k in own:
            if state_dict[k].shape != own[k].shape:
                say("Skip loading parameter {}, required shape{}, loaded shape{}.".format(
                    k, own[k].shape, state_dict[k].shape))
                state_dict[k] = own[k]
        else:
            say("Drop parameter {}.".format(k))
    for k in own:
        if k not in state_dict:
            say("No param {}.".format(k))
            state_dict[k] = own[k]
    model.load_state_dict(state_dict, strict=False)
    if optimizer is not None and resume:
        if "optimizer" in checkpoint:
            optimizer.load_state_dict(checkpoint["optimizer"])
            start_epoch = checkpoint["epoch"]
            start_lr = lr
            for step in lr_step:
                if start_epoch >= step:
                    start_lr *= 0.1
            for group in optimizer.param_groups:
                group["lr"] = start_lr
            say("Resumed optimizer with start lr", start_lr)
        else:
            say("No optimizer parameters in checkpoint.")
    return (model, optimizer, start_epoch) if optimizer is not None else model


def save_model(path, epoch, model, optimizer=None):
    sd = model.module.state_dict() if isinstance(model, torch.nn.DataParallel) else model.state_dict()
    data = {"epoch": epoch, "state_dict": sd}
    if optimizer is not None:
        data["optimizer"] = optimizer.state_dict()
    torch.save(data, path)


# ---- detections -> image coordinates -> results.json ---------------------------------------------

def transform_preds(coords, center, scale, output_size):
    """Inverse of the un-rotated crop transform: the reference builds it from three point pairs with
    cv2.getAffineTransform; for rot = 0 that affine map is
        p_img = center + (p_out - output_size / 2) * (scale_w / output_w)      (isotropic)."""
    coords = np.asarray(coords, dtype=np.float64)
    if not isinstance(scale, (np.ndarray, list, tuple)):
        scale = [scale, scale]
    k = float(scale[0]) / float(output_size[0])
    out = np.zeros(coords.shape)
    out[:, 0] = (coords[:, 0] - output_size[0] * 0.5) * k + center[0]
    out[:, 1] = (coords[:, 1] - output_size[1] * 0.5) * k + center[1]
    return out


def ctdet_post_process(dets, c, s, h, w, num_classes):
    """dets [B, K, 6] (x1, y1, x2, y2, score, class) in output-map pixels -> per image a 1-based class
    dict of [x1, y1, x2, y2, score] lists in image pixels."""
    ret = []
    for i in range(dets.shape[0]):
        top_preds = {}
        dets[i, :, :2] = transform_preds(dets[i, :, 0:2], c[i], s[i], (w, h))
        dets[i, :, 2:4] = transform_preds(dets[i, :, 2:4], c[i], s[i], (w, h))
        classes = dets[i, :, -1]
        for j in range(num_classes):
            inds = classes == j
            top_preds[j + 1] = np.concatenate([dets[i, inds, :4].astype(np.float32),
                                               dets[i, inds, 4:5].astype(np.float32)], axis=1).tolist()
        ret.append(top_preds)
    return ret


def post_process(dets, meta, num_classes, scale=1):
    """CtdetDetector.post_process: dets tensor [1, K, 6] of ONE image (or a flip pair merged by process)."""
    dets = dets.detach().cpu().numpy()
    dets = dets.reshape(1, -1, dets.shape[2])
    dets = ctdet_post_process(dets.copy(), [meta["c"]], [meta["s"]], meta["out_height"], meta["out_width"],
                              num_classes)
    for j in range(1, num_classes + 1):
        dets[0][j] = np.array(dets[0][j], dtype=np.float32).reshape(-1, 5)
        dets[0][j][:, :4] /= scale
    return dets[0]


def soft_nms(boxes, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """lib/models/external/nms.pyx:77-170 with the reference's signature: IN PLACE on a float32 [N, 5] array
    (x1, y1, x2, y2, score), returns keep = list(range(N_final)).  method 0 hard, 1 linear, 2 gaussian.  Runs on the
    library's host routine (cdn_soft_nms_host: the arithmetic the GPU merge kernel uses, no GPU involved) and leaves the
    whole array as the reference leaves it, INCLUDING the stale rows behind N_final that merge_outputs keeps."""
    import ctypes
    from . import _native as N_
    if not (isinstance(boxes, np.ndarray) and boxes.dtype == np.float32 and boxes.ndim == 2 and boxes.shape[1] == 5):
        raise ValueError("soft_nms needs a float32 [N, 5] array")           # (the reference: Cython buffer type error)
    work = boxes if boxes.flags["C_CONTIGUOUS"] else np.ascontiguousarray(boxes)
    n_keep = ctypes.c_int64(0)
    rc = N_.lib().cdn_soft_nms_host(work.ctypes.data, work.shape[0], sigma, Nt, threshold, int(method),
                                    ctypes.addressof(n_keep))
    N_.check(rc, "cdn_soft_nms_host")
    if work is not boxes:
        boxes[...] = work
    return list(range(n_keep.value))


def merge_outputs(detections, num_classes, max_per_image=100, nms=False):
    """CtdetDetector.merge_outputs (ctdet.py:59-74): per class the detections of every test scale concatenated, with more
    than one scale or --nms soft_nms(Nt=0.5, method=2) on them -- whose `keep` the reference ignores: the rows soft_nms
    left behind its final N stay and take part in the cut -- then the max_per_image cut over all classes."""
    results = {}
    for j in range(1, num_classes + 1):
        results[j] = np.concatenate([d[j] for d in detections], axis=0).astype(np.float32)
        if len(detections) > 1 or nms:
            soft_nms(results[j], Nt=0.5, method=2)
    scores = np.hstack([results[j][:, 4] for j in range(1, num_classes + 1)])
    if len(scores) > max_per_image:
        kth = len(scores) - max_per_image
        thresh = np.partition(scores, kth)[kth]
        for j in range(1, num_classes + 1):
            results[j] = results[j][results[j][:, 4] >= thresh]
    return results


def convert_eval_format(all_bboxes, images, num_classes):
    """pascal.py:58-68: detections[class][image index] = list of [x1, y1, x2, y2, score]."""
    detections = [[[] for __ in range(len(images))] for _ in range(num_classes + 1)]
    for i, img_id in enumerate(images):
        for j in range(1, num_classes + 1):
            v = all_bboxes[img_id][j]
            detections[j][i] = v.tolist() if isinstance(v, np.ndarray) else v
    return detections


def save_results(results, images, num_classes, save_dir):
    path = os.path.join(save_dir, "results.json")
    with open(path, "w") as f:
        json.dump(convert_eval_format(results, images, num_classes), f)
    return path


def _to_float(x):
    return float("{:.2f}".format(x))


def convert_eval_format_coco(all_bboxes, valid_ids):
    """coco.py:87-112: all_bboxes[image_id][class (1-based)] = rows of [x1, y1, x2, y2, score] (merge_outputs' arrays, or
    lists) -> the flat detection list COCO's evaluation loads,
        {"image_id", "category_id": valid_ids[class - 1], "bbox": [x, y, w, h], "score"},
    every number cut to two decimals through its decimal text.  valid_ids: the dataset's table of the 80 category ids
    (COCO._valid_ids; the caller has the dataset object, this library carries no copy).  Width and height are formed in
    the rows' own number type, as the reference forms them (float32 for merge_outputs' arrays).  The reference subtracts
    in place and leaves [x1, y1, w, h, score] behind in the caller's rows; this function does NOT touch its input, so
    converting the same results twice gives the same list."""
    detections = []
    for image_id in all_bboxes:
        for cls_ind in all_bboxes[image_id]:
            category_id = int(valid_ids[cls_ind - 1])
            for bbox in all_bboxes[image_id][cls_ind]:
                b = np.array(bbox)                       # (a copy in the row's own dtype)
                b[2] -= b[0]
                b[3] -= b[1]
                detections.append({"image_id": int(image_id), "category_id": category_id,
                                   "bbox": [_to_float(v) for v in b[0:4]], "score": _to_float(b[4])})
    return detections


def save_results_coco(results, valid_ids, save_dir):
    """coco.py:117-119: results.json in COCO's detection layout (pycocotools' loadRes reads it)."""
    path = os.path.join(save_dir, "results.json")
    with open(path, "w") as f:
        json.dump(convert_eval_format_coco(results, valid_ids), f)
    return path


# ---- scoring on the device (codenet_eval.hip) ----------------------------------------------

COCO_IOU_THRS = np.linspace(.5, .95, 10)                  # Params.iouThrs / recThrs / areaRng as pycocotools sets them
COCO_REC_THRS = np.linspace(.0, 1.00, 101)
COCO_AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
COCO_MAX_DETS = (1, 10, 100)
VOC07_POINTS = np.arange(0.0, 1.1, 0.1)


def _eval_device(device):
    """torch.device with the index filled in ("cuda" -> the current GPU), so that tables and blocks compare equal."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _eval_call(device, name, *args):
    """One entry of the scorer: the kernel on the current stream of a GPU `device`, the `_host` twin (the same header on
    CPU memory) otherwise."""
    from . import _native as N_
    lib = N_.lib()
    if device.type == "cuda":
        with torch.cuda.device(device):          # the launch goes to the table's GPU, whichever one is current
            rc = getattr(lib, name)(*args, torch.cuda.current_stream(device).cuda_stream)
    else:
        name += "_host"
        rc = getattr(lib, name)(*args)
    N_.check(rc, name)


class DeviceResults:
    """The detections of a whole evaluation run as ONE float64 table on `device`: [n_images, cap, 6] rows
    (x1, y1, x2, y2, score, class) -- coco=True: (x, y, w, h, score, class) with COCO's two-decimal cut
    (convert_eval_format_coco) -- plus a per-image count.  ``append`` is one launch and never synchronises; rows beyond
    `cap` raise a device flag that voc_eval_device / coco_eval read with their results and turn into an error."""

    def __init__(self, n_images, num_classes, cap=100, coco=False, device="cuda"):
        self.device = _eval_device(device)
        self.n_images, self.num_classes, self.cap, self.coco = int(n_images), int(num_classes), int(cap), bool(coco)
        self.det = torch.zeros(self.n_images, self.cap, 6, dtype=torch.float64, device=self.device)
        self.count = torch.zeros(self.n_images, dtype=torch.int32, device=self.device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.device)

    def append(self, raw, image_slot):
        """raw: what merge_scales_native(raw=True) / replay.raw give -- (block, boxes [B, classes, R, 5] float32,
        rows_out [B, classes] int32, ...) or just (boxes, rows_out) -- whose B images go to the slots image_slot ..
        image_slot + B - 1 with no host copy; or a host {class (1-based): [n, 5]} dict (a list of them: consecutive
        slots), as merge_outputs returns it."""
        if isinstance(raw, dict):
            raw = [raw]
        if isinstance(raw, list):
            n = max([1] + [len(d.get(j, ())) for d in raw for j in range(1, self.num_classes + 1)])
            boxes = np.zeros((len(raw), self.num_classes, n, 5), dtype=np.float32)
            rows = np.zeros((len(raw), self.num_classes), dtype=np.int32)
            for b, d in enumerate(raw):
                for j in range(1, self.num_classes + 1):
                    v = np.asarray(d.get(j, ()), dtype=np.float32).reshape(-1, 5)
                    boxes[b, j - 1, :len(v)] = v
                    rows[b, j - 1] = len(v)
            boxes, rows_out = torch.from_numpy(boxes).to(self.device), torch.from_numpy(rows).to(self.device)
        else:
            boxes, rows_out = (raw[1], raw[2]) if len(raw) > 2 else raw
        if boxes.device != self.device or rows_out.device != self.device:
            raise ValueError("DeviceResults.append: the block lives on %s, the table on %s" % (boxes.device, self.device))
        if not (boxes.dtype == torch.float32 and boxes.dim() == 4 and boxes.shape[1] == self.num_classes and boxes.shape[3] == 5
                and rows_out.dtype == torch.int32 and tuple(rows_out.shape) == tuple(boxes.shape[:2])
                and boxes.is_contiguous() and rows_out.is_contiguous()):
            raise ValueError("DeviceResults.append needs boxes [B, %d, R, 5] float32 and rows_out [B, %d] int32, contiguous"
                             % (self.num_classes, self.num_classes))
        _eval_call(self.device, "cdn_eval_append", boxes.data_ptr(), rows_out.data_ptr(), boxes.shape[0], self.num_classes,
                   boxes.shape[2], int(image_slot), self.det.data_ptr(), self.count.data_ptr(), self.n_images, self.cap,
                   int(self.coco), self.flag.data_ptr())
        return self

    def _sorted(self):
        """(sorted keys, permutation): per class descending score, stable over (image, row).  The one torch.sort."""
        keys = torch.empty(self.n_images * self.cap, dtype=torch.int64, device=self.device)
        _eval_call(self.device, "cdn_eval_sort_keys", self.det.data_ptr(), self.count.data_ptr(), self.n_images, self.cap,
                   self.num_classes, int(self.coco), keys.data_ptr(), self.flag.data_ptr())
        return torch.sort(keys, stable=True)


def _raise_on_flag(flag, results):
    if flag & 1:
        raise RuntimeError("DeviceResults: an image has more than cap = %d detections; the table was built too small "
                           "(rows beyond cap were not stored)" % results.cap)
    if flag:
        raise RuntimeError("DeviceResults: a score that cannot be ordered (NaN or out of range)")


class GroundTruth:
    """Ground truth in CSR form per (image slot, class): boxes [G, 4] float64 (voc=True: x1 y1 x2 y2, else x y w h), areas
    [G], flags [G] int32 (bit 0: difficult / iscrowd), offsets [n_images * classes + 1] int32; image_ids: slot -> image
    id, valid_ids: class -> category id."""

    def __init__(self, image_ids, valid_ids, boxes, areas, flags, offsets, voc, device="cpu"):
        self.image_ids, self.valid_ids, self.voc = list(image_ids), list(valid_ids), bool(voc)
        self.n_images, self.num_classes = len(self.image_ids), len(self.valid_ids)
        self.device = _eval_device(device)
        to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(self.device)   # noqa: E731
        self.boxes = to(np.asarray(boxes, dtype=np.float64).reshape(-1, 4), torch.float64)
        self.areas, self.flags, self.offsets = to(areas, torch.float64), to(flags, torch.int32), to(offsets, torch.int32)
        self.slot = {v: i for i, v in enumerate(self.image_ids)}
        assert self.offsets.numel() == self.n_images * self.num_classes + 1

    @classmethod
    def from_coco_dict(cls, ann, image_ids=None, valid_ids=None, voc=False, device="cpu"):
        """ann: a COCO-layout annotation dict ({"images", "annotations", "categories"}).  image_ids: the slot order
        (default: the sorted ids of ann["images"], COCOeval's order), valid_ids: the class order (default: the sorted
        category ids).  voc=True: boxes become x1 y1 x2 y2 and the flag is `ignore` or `difficult` (tools/eval_voc.py);
        otherwise x y w h, the annotated `area` (w * h where absent) and `iscrowd`."""
        if image_ids is None:
            image_ids = sorted(im["id"] for im in ann["images"])
        if valid_ids is None:
            valid_ids = sorted(c["id"] for c in ann["categories"])
        slot, klass = {v: i for i, v in enumerate(image_ids)}, {v: i for i, v in enumerate(valid_ids)}
        K = len(valid_ids)
        cells = {}
        for a in ann["annotations"]:
            if a["image_id"] not in slot or a["category_id"] not in klass:
                continue
            x, y, w, h = (float(v) for v in a["bbox"])
            if voc:
                row = ([x, y, x + w, y + h], 0.0, int(bool(a.get("ignore", 0) or a.get("difficult", 0))))
            else:
                row = ([x, y, w, h], float(a["area"]) if "area" in a else w * h, int(bool(a.get("iscrowd", 0))))
            cells.setdefault(slot[a["image_id"]] * K + klass[a["category_id"]], []).append(row)
        boxes, areas, flags, offsets = [], [], [], [0]
        for cell in range(len(image_ids) * K):
            for b, ar, f in cells.get(cell, ()):
                boxes.append(b)
                areas.append(ar)
                flags.append(f)
            offsets.append(len(boxes))
        return cls(image_ids, valid_ids, boxes, areas, flags, offsets, voc, device)

    def to(self, device):
        return GroundTruth(self.image_ids, self.valid_ids, self.boxes.cpu().numpy(), self.areas.cpu().numpy(),
                           self.flags.cpu().numpy(), self.offsets.cpu().numpy(), self.voc, device)


def _check_pair(results, gt, coco):
    if results.coco != coco or gt.voc == coco:
        raise ValueError("results and ground truth must both be in %s form" % ("COCO" if coco else "VOC"))
    if (results.n_images, results.num_classes) != (gt.n_images, gt.num_classes) or results.device != gt.device:
        raise ValueError("results (%d images, %d classes, %s) and ground truth (%d, %d, %s) do not match" % (
            results.n_images, results.num_classes, results.device, gt.n_images, gt.num_classes, gt.device))


def voc_eval_device(results, gt, ovthresh=0.5, curves=False):
    """VOC07 scoring of a DeviceResults table against a GroundTruth (voc=True), all classes at once: match
    (voc_eval.py:95-207, one wave per image and class), one stable sort, accumulate.  Returns {"ap_07": [classes]
    (the 11-point metric), "ap_area": [classes] (area under the envelope), "npos": [classes]} as float64 arrays after
    ONE device-to-host copy; curves=True adds "rec" / "prec": per class the arrays over its detections in descending
    score order (two more copies).  tools/eval_voc.py::voc_eval_curve / voc_ap07 / voc_ap_area give the same bits."""
    _check_pair(results, gt, False)
    dev, n, C = results.device, results.n_images * results.cap, results.num_classes
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)      # noqa: E731
    f64 = lambda k: torch.zeros(k, dtype=torch.float64, device=dev)   # noqa: E731
    seen, tp, fp = u8(max(1, gt.boxes.shape[0])), u8(n), u8(n)
    _eval_call(dev, "cdn_eval_match_voc", results.det.data_ptr(), results.count.data_ptr(), results.n_images, results.cap, C,
               gt.boxes.data_ptr() if gt.boxes.numel() else seen.data_ptr(),
               gt.flags.data_ptr() if gt.flags.numel() else seen.data_ptr(), gt.offsets.data_ptr(), float(ovthresh),
               seen.data_ptr(), tp.data_ptr(), fp.data_ptr())
    keys, perm = results._sorted()
    rec, prec, env, terms, out = f64(n), f64(n), f64(n), f64(n + C), f64(4 * C + 2)
    thr = torch.from_numpy(VOC07_POINTS.copy()).to(dev)
    _eval_call(dev, "cdn_eval_accumulate_voc", keys.data_ptr(), perm.data_ptr(), results.n_images, results.cap, C,
               tp.data_ptr(), fp.data_ptr(), gt.flags.data_ptr() if gt.flags.numel() else seen.data_ptr(),
               gt.offsets.data_ptr(), thr.data_ptr(), thr.numel(), results.flag.data_ptr(), rec.data_ptr(), prec.data_ptr(),
               env.data_ptr(), terms.data_ptr(), out.data_ptr())
    host = out.cpu().numpy()
    _raise_on_flag(int(host[4 * C + 1]), results)
    res = {"ap_07": host[:C].copy(), "ap_area": host[C:2 * C].copy(), "npos": host[2 * C:3 * C].copy()}
    if curves:
        off = host[3 * C:4 * C + 1].astype(np.int64)
        rec_h, prec_h = rec.cpu().numpy(), prec.cpu().numpy()
        res["rec"] = [rec_h[off[c]:off[c + 1]].copy() for c in range(C)]
        res["prec"] = [prec_h[off[c]:off[c + 1]].copy() for c in range(C)]
    return res


def coco_summarize(precision, recall):
    """COCOeval.summarize for bbox: the twelve statistics, each the mean of the entries > -1 (-1 if there are none)."""
    def stat(ap, iou=None, area=0, md=2):
        s = precision[:, :, :, area, md] if ap else recall[:, :, area, md]
        if iou is not None:
            s = s[np.where(iou == COCO_IOU_THRS)[0]]
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    return np.array([stat(1), stat(1, iou=.5), stat(1, iou=.75), stat(1, area=1), stat(1, area=2), stat(1, area=3),
                     stat(0, md=0), stat(0, md=1), stat(0, md=2), stat(0, area=1), stat(0, area=2), stat(0, area=3)],
                    dtype=np.float64)


def coco_eval(results, gt, details=False):
    """COCO bbox scoring of a DeviceResults table (coco=True) against a GroundTruth: COCOeval.evaluateImg (one wave per
    image and category, lanes = 10 IoU thresholds x 4 area ranges), one stable sort, COCOeval.accumulate.  Returns
    {"stats": float64 [12] (summarize's rule, formed here on the host), "precision": [10, 101, K, 4, 3], "recall":
    [10, K, 4, 3]} after ONE device-to-host copy.  details=True adds the per-detection arrays "dtm" / "dtig"
    [10, 4, n_images, cap] and "rank" [n_images, cap].  The algorithm is the one DESIGN.md section 7.4e writes down;
    it is not pinned to pycocotools' own bits (no fixture recorded from it exists)."""
    _check_pair(results, gt, True)
    dev, n, K = results.device, results.n_images * results.cap, results.num_classes
    G = int(gt.boxes.shape[0])
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device=dev)      # noqa: E731
    gtm, dtm, dtig = u8(max(1, 40 * G)), u8(40 * n), u8(40 * n)
    rank = torch.full((n,), 1 << 30, dtype=torch.int32, device=dev)
    nonign = torch.zeros(results.n_images * K * 4, dtype=torch.int32, device=dev)
    consts = torch.from_numpy(np.concatenate([COCO_IOU_THRS, COCO_AREA_RNG.reshape(-1), COCO_REC_THRS])).to(dev)
    p0 = consts.data_ptr()
    spare = gtm.data_ptr()
    _eval_call(dev, "cdn_eval_match_coco", results.det.data_ptr(), results.count.data_ptr(), results.n_images, results.cap, K,
               gt.boxes.data_ptr() if G else spare, gt.areas.data_ptr() if G else spare, gt.flags.data_ptr() if G else spare,
               gt.offsets.data_ptr(), G, p0, p0 + 80, gtm.data_ptr(), dtm.data_ptr(), dtig.data_ptr(), rank.data_ptr(),
               nonign.data_ptr())
    keys, perm = results._sorted()
    nP, nR = 10 * 101 * K * 4 * 3, 10 * K * 4 * 3
    out = torch.zeros(nP + nR + 1, dtype=torch.float64, device=dev)
    o0 = out.data_ptr()
    _eval_call(dev, "cdn_eval_accumulate_coco", keys.data_ptr(), perm.data_ptr(), results.n_images, results.cap, K,
               dtm.data_ptr(), dtig.data_ptr(), rank.data_ptr(), nonign.data_ptr(), p0 + 144, results.flag.data_ptr(), o0,
               o0 + 8 * nP, o0 + 8 * (nP + nR))
    host = out.cpu().numpy()
    _raise_on_flag(int(host[-1]), results)
    precision, recall = host[:nP].reshape(10, 101, K, 4, 3).copy(), host[nP:nP + nR].reshape(10, K, 4, 3).copy()
    res = {"stats": coco_summarize(precision, recall), "precision": precision, "recall": recall}
    if details:
        res["dtm"] = dtm.cpu().numpy().reshape(10, 4, results.n_images, results.cap)
        res["dtig"] = dtig.cpu().numpy().reshape(10, 4, results.n_images, results.cap)
        res["rank"] = rank.cpu().numpy().reshape(results.n_images, results.cap)
    return res


# ---- integer export --------------------------------------------------------------------------------

def pack_int4(codes):
    """int8 codes in [-8, 7], last dim even -> uint8 with two two's-complement nibbles per byte (low first)."""
    c = codes.to(torch.int16) & 0xF
    return (c[..., 0::2] | (c[..., 1::2] << 4)).to(torch.uint8)


def unpack_int4(packed):
    p = packed.to(torch.int16)
    lo, hi = p & 0xF, (p >> 4) & 0xF
    out = torch.stack([lo, hi], dim=-1).reshape(*packed.shape[:-1], packed.shape[-1] * 2)
    return torch.where(out > 7, out - 16, out).to(torch.int8)


def export_w4(model, path=None):
    """Every per-channel symmetric <= 4-bit conv of a quantised model as packed codes + scales (the
    fake-quantised weight is codes / scale, bit-exactly), plus the folded biases and every QuantAct range.
    Returns the dict; written with numpy.savez when `path` is given."""
    from .portable_quantizer.quant_modules import QuantAct, QuantBnConv2d, Quant_Conv2d, QuantDeformConv2d
    out = {}
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, QuantAct):
                out[name + ".x_min"] = m.x_min.cpu().numpy()
                out[name + ".x_max"] = m.x_max.cpu().numpy()
                continue
            if isinstance(m, QuantBnConv2d):
                sf = m.bn.weight / torch.sqrt(m.bn.running_var + m.bn.eps)
                w = m.conv.weight * sf.reshape(-1, 1, 1, 1)
                bias = m.folded()[1]
            elif isinstance(m, (Quant_Conv2d, QuantDeformConv2d)):
                w, bias = m.weight, m.bias
            else:
                continue
            if m.full_precision_flag or not m.per_channel or m.quant_mode != "symmetric" or m.weight_bit > 4:
                continue
            co = w.shape[0]
            flat = w.reshape(co, -1)
            codes, scale, _ = m._int8_codes(flat.reshape(co, -1, 1, 1))
            codes = codes[:, :flat.shape[1]]
            if codes.shape[1] % 2:
                codes = torch.cat([codes, torch.zeros(co, 1, dtype=torch.int8, device=codes.device)], 1)
            out[name + ".codes_packed"] = pack_int4(codes).cpu().numpy()
            out[name + ".scale"] = scale.cpu().numpy()
            out[name + ".shape"] = np.array(w.shape)
            if bias is not None:
                out[name + ".bias"] = bias.detach().cpu().numpy()
    if path is not None:
        np.savez_compressed(path, **out)
    return out
