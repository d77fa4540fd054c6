"""Writes tests/golden/ctdet_loss_ref.npz and tests/golden/ctdet_targets_ref.npz.  Runs in the build container only, like
make_golden.py: it needs the reference checkout.

    python tests/golden/make_loss_golden.py /path/to/reference

The reference's own modules are imported (nothing is copied) with empty stand-ins for the third-party imports this
container lacks (cv2, numba, progress, pycocotools): lib/trains/ctdet.py::CtdetLoss for the criterion, and
lib/utils/image.py::gaussian_radius / draw_umich_gaussian for the target maps, driven through the steps of
lib/datasets/sample/ctdet.py:87-122.  The fixtures hold arrays only.

ctdet_loss_ref.npz -- per case k (names[k]): inputs `c{k}_hm{s}`, `c{k}_wh{s}`, `c{k}_reg{s}` per stack s and the targets
`c{k}_gt_hm / gt_wh / gt_reg / ind / reg_mask`; the reference's results in float64, `c{k}_scalars` (loss, hm_loss,
wh_loss, off_loss) and `c{k}_g_hm{s} / g_wh{s} / g_reg{s}`; and the reference's OWN float32-vs-float64 error,
`c{k}_err_scalars` (absolute) and `c{k}_err_grads{s}` (largest element error over the largest float64 gradient, per
head).  Options per case: reg_loss (0 l1, 1 sl1), reg_offset, num_stacks, weights [hm, wh, off].  The generator asserts
that the float32 and float64 runs clamp the same elements.

ctdet_targets_ref.npz -- per shape t: `t{t}_boxes [N, M, 4]`, `t{t}_classes`, `t{t}_counts`, `t{t}_shape` (classes, H, W)
and the outputs `t{t}_hm / wh / reg / ind / reg_mask`.
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32


def import_reference(ref_root):
    for name in ["cv2", "numba", "progress", "progress.bar", "pycocotools", "pycocotools.coco", "pycocotools.cocoeval"]:
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["numba"].jit = lambda *a, **k: (lambda fn: fn)
    sys.modules["progress.bar"].Bar = type("Bar", (), {})
    sys.path.insert(0, os.path.join(ref_root, "lib"))
    from trains.ctdet import CtdetLoss
    from utils import image
    return CtdetLoss, image


def reference_targets(image, boxes, classes, counts, C, H, W):
    """lib/datasets/sample/ctdet.py:87-122 from the clipped output-space boxes on, with the reference's functions."""
    N, M = boxes.shape[:2]
    hm = np.zeros((N, C, H, W), dtype=f32)
    wh = np.zeros((N, M, 2), dtype=f32)
    reg = np.zeros((N, M, 2), dtype=f32)
    ind = np.zeros((N, M), dtype=np.int64)
    reg_mask = np.zeros((N, M), dtype=np.uint8)
    for b in range(N):
        for k in range(int(counts[b])):
            bbox = boxes[b, k].astype(f32)
            cls_id = int(classes[b, k])
            h, w = bbox[3] - bbox[1], bbox[2] - bbox[0]
            if h > 0 and w > 0:
                radius = image.gaussian_radius((math.ceil(h), math.ceil(w)))
                radius = max(0, int(radius))
                ct = np.array([(bbox[0] + bbox[2]) / 2, (bbox[1] + bbox[3]) / 2], dtype=f32)
                ct_int = ct.astype(np.int32)
                image.draw_umich_gaussian(hm[b, cls_id], ct_int, radius)
                wh[b, k] = 1. * w, 1. * h
                ind[b, k] = ct_int[1] * W + ct_int[0]
                reg[b, k] = ct - ct_int
                reg_mask[b, k] = 1
    return hm, wh, reg, ind, reg_mask


def clip_boxes(b, H, W):
    b = np.array(b, dtype=f32).reshape(-1, 4)
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], 0, W - 1)
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], 0, H - 1)
    return b


# ---- target fixture -------------------------------------------------------------------------------------------------

def target_images(rng, H, W, M):
    """-> per image (boxes, classes, count): one situation each."""
    imgs = []
    # 0: large boxes whose gaussians are cut by the left, right, top, bottom border and by a corner
    imgs.append(([[-5, 6, 9.5, 15.25], [W - 9.5, 4, W + 6, 13.5], [7, -4, 16.5, 6.75], [5.25, H - 8, 15, H + 3],
                  [W - 7.5, H - 6.5, W + 9, H + 9]], [0, 1, 2, 0, 1], 5))
    # 1: radius 0 (boxes of at most one pixel), inside and on the border
    imgs.append(([[4.25, 5.5, 5.0, 6.25], [0, 0, 0.75, 0.5], [W - 1.5, H - 1.75, W - 1, H - 1], [9.5, 3.25, 10.5, 4.25]],
                 [0, 1, 2, 2], 4))
    # 2: degenerate boxes (h == 0, w == 0, a box beyond the map that the clip collapses) between two live ones
    imgs.append(([[3, 4, 9, 4], [6, 2, 6, 9], [W + 3, 5, W + 9, 12], [2.5, 3.5, 8.25, 9.75], [5, H + 2, 11, H + 8],
                  [10.5, 8.25, 17.75, 14.5]], [0, 1, 2, 1, 0, 2], 6))
    # 3: overlapping gaussians of one class (the per-class maximum decides), two of them concentric
    imgs.append(([[3, 3, 13, 12], [6.5, 4.25, 17, 14.5], [5, 5, 11, 10], [4, 4, 12, 11]], [1, 1, 1, 1], 4))
    # 4: the same centre cell in two classes, and twice in one class
    imgs.append(([[4, 4, 12.5, 13], [5, 3, 11.5, 14], [4.5, 4.5, 12, 12.5]], [0, 2, 0], 3))
    # 5: a full max_objs image
    c = rng.uniform([2, 2], [W - 3, H - 3], (M, 2))
    s = rng.uniform(0.6, 9.0, (M, 2))
    imgs.append((np.concatenate([c - s / 2, c + s / 2], 1), rng.integers(0, 3, M), M))
    # 6: an empty image whose unused rows hold boxes that must be ignored
    imgs.append(([[3, 3, 9, 9], [5, 5, 12, 12]], [0, 1], 0))
    # 7: count below the rows given
    c = rng.uniform([0, 0], [W - 1, H - 1], (M, 2))
    s = rng.uniform(0.2, 14.0, (M, 2))
    imgs.append((np.concatenate([c - s / 2, c + s / 2], 1), rng.integers(0, 3, M), M - 2))
    return imgs


def make_targets_fixture(image):
    out = {}
    M, C = 7, 3
    for t, (H, W) in enumerate([(20, 24), (21, 23)]):         # H * W a multiple of four, and not
        rng = np.random.default_rng(77 + t)
        imgs = target_images(rng, H, W, M)
        boxes = np.zeros((len(imgs), M, 4), dtype=f32)
        classes = np.zeros((len(imgs), M), dtype=np.int32)
        counts = np.zeros(len(imgs), dtype=np.int32)
        for i, (b, c, n) in enumerate(imgs):
            b = clip_boxes(b, H, W)
            boxes[i, :len(b)], classes[i, :len(b)], counts[i] = b, np.asarray(c), n
        hm, wh, reg, ind, reg_mask = reference_targets(image, boxes, classes, counts, C, H, W)
        assert (hm == 1).sum() > 10 and (wh[2, :3] == 0).all() and reg_mask[2].sum() == 2 and reg_mask[6].sum() == 0
        assert reg_mask[5].all() and (hm[6] == 0).all() and ind[4, 0] == ind[4, 2]
        out.update({"t%d_boxes" % t: boxes, "t%d_classes" % t: classes, "t%d_counts" % t: counts,
                    "t%d_shape" % t: np.array([C, H, W]), "t%d_hm" % t: hm, "t%d_wh" % t: wh, "t%d_reg" % t: reg,
                    "t%d_ind" % t: ind, "t%d_reg_mask" % t: reg_mask})
    np.savez_compressed(os.path.join(HERE, "ctdet_targets_ref.npz"), **out)
    print("targets: %d shapes, %d bytes" % (2, os.path.getsize(os.path.join(HERE, "ctdet_targets_ref.npz"))))


# ---- loss fixture ---------------------------------------------------------------------------------------------------

def run_reference(CtdetLoss, case, dtype):
    opt = types.SimpleNamespace(
        mse_loss=False, reg_loss=case["reg_loss"], dense_wh=False, norm_wh=False, cat_spec_wh=False,
        num_stacks=len(case["heads"]), eval_oracle_hm=False, eval_oracle_wh=False, eval_oracle_offset=False,
        hm_weight=case["weights"][0], wh_weight=case["weights"][1], off_weight=case["weights"][2],
        reg_offset=case["reg_offset"], device=torch.device("cpu"))
    leaves, outputs = [], []
    for hm, wh, reg in case["heads"]:
        ls = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in (hm, wh, reg)]
        leaves.append(ls)
        outputs.append({"hm": ls[0].clone(), "wh": ls[1].clone(), "reg": ls[2].clone()})
    batch = {"hm": torch.from_numpy(case["gt_hm"]).to(dtype), "wh": torch.from_numpy(case["gt_wh"]).to(dtype),
             "reg": torch.from_numpy(case["gt_reg"]).to(dtype), "ind": torch.from_numpy(case["ind"]),
             "reg_mask": torch.from_numpy(case["reg_mask"])}
    loss, stats = CtdetLoss(opt)(outputs, batch)
    loss.backward()
    scalars = np.array([float(stats[k]) for k in ("loss", "hm_loss", "wh_loss", "off_loss")], dtype=np.float64)
    grads = [[(l.grad if l.grad is not None else torch.zeros_like(l)).double().numpy() for l in ls] for ls in leaves]
    return scalars, grads


def loss_cases(image):
    rng = np.random.default_rng(4242)
    N, C, H, W, M = 2, 3, 13, 15, 6          # N*C*H*W = 1170: not a multiple of four
    cases = []

    def objects(counts):
        boxes = np.zeros((N, M, 4), dtype=f32)
        for b in range(N):
            c = rng.uniform([1, 1], [W - 2, H - 2], (M, 2))
            s = rng.uniform(0.8, 7.0, (M, 2))
            boxes[b] = clip_boxes(np.concatenate([c - s / 2, c + s / 2], 1), H, W)
        return boxes, rng.integers(0, C, (N, M)).astype(np.int32), np.array(counts, dtype=np.int32)

    def heads(n=1, scale=1.5):
        return [((rng.normal(-1.5, scale, (N, C, H, W))).astype(f32), rng.uniform(0, 8, (N, 2, H, W)).astype(f32),
                 rng.uniform(-0.5, 1.5, (N, 2, H, W)).astype(f32)) for _ in range(n)]

    def add(name, objs, hd, reg_loss="l1", reg_offset=True, weights=(1.0, 0.1, 1.0), edit=None):
        gt = reference_targets(image, objs[0], objs[1], objs[2], C, H, W)
        case = dict(name=name, heads=hd, gt_hm=gt[0], gt_wh=gt[1], gt_reg=gt[2], ind=gt[3], reg_mask=gt[4],
                    reg_loss=reg_loss, reg_offset=reg_offset, weights=weights)
        if edit:
            edit(case)
        cases.append(case)
        return case

    base = objects([M, 4])
    add("l1", base, heads())
    # sl1 with differences on both sides of 1: wh predictions up to 8 against sizes below 7, offsets within 1
    add("sl1", base, heads(), reg_loss="sl1")
    add("reg_offset_off", base, heads(), reg_offset=False)
    add("wh_weight_zero", base, heads(), weights=(1.0, 0.0, 1.0))
    add("image_without_object", objects([5, 0]), heads())
    add("batch_without_object", objects([0, 0]), heads())

    def share_cells(case):                     # rows 0, 1 of image 0 on one cell; rows 1, 2, 4 of image 1 on another
        case["ind"][0, 1] = case["ind"][0, 0]
        case["ind"][1, 2] = case["ind"][1, 4] = case["ind"][1, 1]
    add("shared_cells", objects([M, M]), heads(), edit=share_cells)
    add("shared_cells_sl1", objects([M, M]), heads(), reg_loss="sl1", edit=share_cells)

    def beyond_clamp(case):                    # logits beyond both clamp bounds, on positives and negatives
        hm = case["heads"][0][0].reshape(-1)
        pos = np.flatnonzero(case["gt_hm"].reshape(-1) == 1)
        neg = np.flatnonzero(case["gt_hm"].reshape(-1) < 1)
        hm[pos[0]], hm[pos[1]], hm[pos[2]] = 14.0, -13.0, 12.0
        hm[neg[::7]] = rng.choice([-20.0, -12.0, 12.5, 16.0, 30.0, -40.0], len(neg[::7])).astype(f32)
    add("beyond_clamp", base, heads(), edit=beyond_clamp)

    def zero_difference(case):                 # predictions that equal their targets: sign(0) = 0 in the L1 gradient
        hm, wh, reg = case["heads"][0]
        for b, k in ((0, 0), (0, 2), (1, 1)):
            y, x = divmod(int(case["ind"][b, k]), W)
            wh[b, :, y, x] = case["gt_wh"][b, k]
            reg[b, 0, y, x] = case["gt_reg"][b, k, 0]
    add("zero_difference", base, heads(), edit=zero_difference)
    add("two_stacks", base, heads(2))
    add("two_stacks_sl1_weights", base, heads(2), reg_loss="sl1", weights=(0.7, 0.25, 1.5))
    return cases


def make_loss_fixture(CtdetLoss, image):
    out, names = {}, []
    cases = loss_cases(image)
    for k, case in enumerate(cases):
        s64, g64 = run_reference(CtdetLoss, case, torch.float64)
        s32, g32 = run_reference(CtdetLoss, case, torch.float32)
        names.append(case["name"])
        for key in ("gt_hm", "gt_wh", "gt_reg", "ind", "reg_mask"):
            out["c%d_%s" % (k, key)] = case[key]
        out["c%d_scalars" % k] = s64
        out["c%d_err_scalars" % k] = np.abs(s32 - s64)
        for s, (hm, wh, reg) in enumerate(case["heads"]):
            out["c%d_hm%d" % (k, s)], out["c%d_wh%d" % (k, s)], out["c%d_reg%d" % (k, s)] = hm, wh, reg
            errs = []
            for name, a64, a32 in zip(("g_hm", "g_wh", "g_reg"), g64[s], g32[s]):
                out["c%d_%s%d" % (k, name, s)] = a64
                top = np.abs(a64).max()
                errs.append(np.abs(a32 - a64).max() / top if top > 0 else 0.0)
                assert np.array_equal(a32 == 0, a64 == 0), "float32 and float64 clamp different elements (%s)" % case["name"]
            out["c%d_err_grads%d" % (k, s)] = np.array(errs)
    out["names"] = np.array(names)
    out["reg_loss"] = np.array([{"l1": 0, "sl1": 1}[c["reg_loss"]] for c in cases])
    out["reg_offset"] = np.array([int(c["reg_offset"]) for c in cases])
    out["num_stacks"] = np.array([len(c["heads"]) for c in cases])
    out["weights"] = np.array([c["weights"] for c in cases], dtype=np.float64)
    by = dict(zip(names, range(len(names))))
    assert out["c%d_scalars" % by["batch_without_object"]][2] == 0 and (out["c%d_gt_hm" % by["batch_without_object"]] == 0).all()
    assert (out["c%d_g_hm0" % by["beyond_clamp"]] == 0).sum() > 20
    path = os.path.join(HERE, "ctdet_loss_ref.npz")
    np.savez_compressed(path, **out)
    print("loss: %d cases, %d bytes" % (len(cases), os.path.getsize(path)))
    for k, n in enumerate(names):
        print("  %-24s scalars %s  err %s  grad err %s" % (n, out["c%d_scalars" % k].round(5), out["c%d_err_scalars" % k],
                                                          out["c%d_err_grads0" % k]))


def main():
    CtdetLoss, image = import_reference(sys.argv[1])
    make_targets_fixture(image)
    make_loss_fixture(CtdetLoss, image)


if __name__ == "__main__":
    main()
