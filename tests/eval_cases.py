"""Cases shared by tests/test_eval_device_host.py (the `_host` entries against tests/coco_eval_ref.py, the VOC fixture and
hand-derived answers) and tests/test_gpu_eval_device.py (the kernels against the `_host` entries on the same cases).

A case: {"image_ids", "cat_ids", "rows": {image_id: {class (1-based): float32 [n, 5] x1 y1 x2 y2 score}}, "gts": COCO-layout
annotations}.  Boxes in "rows" are what merge_outputs returns; COCO mode cuts them on the way into the table."""
import os

import numpy as np
import torch

from codenet_amd import evalio
from tests import coco_eval_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gt(image_id, cat, x, y, w, h, crowd=0, area=None):
    return {"image_id": image_id, "category_id": cat, "bbox": [float(x), float(y), float(w), float(h)],
            "area": float(w * h if area is None else area), "iscrowd": crowd}


def case(image_ids, cat_ids, rows, gts):
    rows = {i: {c + 1: np.asarray(rows.get(i, {}).get(c + 1, []), dtype=np.float32).reshape(-1, 5)
                for c in range(len(cat_ids))} for i in image_ids}
    return {"image_ids": list(image_ids), "cat_ids": list(cat_ids), "rows": rows, "gts": gts}


def ann_dict(c):
    return {"images": [{"id": i} for i in c["image_ids"]], "categories": [{"id": k} for k in c["cat_ids"]],
            "annotations": c["gts"]}


def ref_dets(c):
    """The case's detections as the flat COCO list, cut to two decimals by the Python text formatting, in table order."""
    out = []
    for i in c["image_ids"]:
        for k, cat in enumerate(c["cat_ids"]):
            for b in R.cut_rows(c["rows"][i][k + 1]):
                out.append({"image_id": i, "category_id": cat, "bbox": b[:4], "score": b[4]})
    return out


def run_coco(c, device, cap=100, via_block=False):
    g = evalio.GroundTruth.from_coco_dict(ann_dict(c), image_ids=c["image_ids"], valid_ids=c["cat_ids"], device=device)
    res = evalio.DeviceResults(len(c["image_ids"]), len(c["cat_ids"]), cap=cap, coco=True, device=device)
    if via_block:
        res.append([c["rows"][i] for i in c["image_ids"]], 0)
    else:
        for s, i in enumerate(c["image_ids"]):
            res.append(c["rows"][i], s)
    return evalio.coco_eval(res, g, details=True), res


def run_voc(c, device, cap=100, ovthresh=0.5):
    g = evalio.GroundTruth.from_coco_dict(ann_dict(c), image_ids=c["image_ids"], valid_ids=c["cat_ids"], voc=True,
                                          device=device)
    res = evalio.DeviceResults(len(c["image_ids"]), len(c["cat_ids"]), cap=cap, coco=False, device=device)
    res.append([c["rows"][i] for i in c["image_ids"]], 0)
    return evalio.voc_eval_device(res, g, ovthresh=ovthresh, curves=True), res


def flags_of(c, out, ev):
    """The native per-detection flags laid out like the restatement's: for every (k, a, image) with detections or ground
    truth, (dtm [T, D], dtig [T, D]) over the kept detections in rank order.  Rows of a class are contiguous in the table,
    in input order."""
    got = {}
    for (k, a, i), e in ev.items():
        if e is None:
            continue
        img = c["image_ids"][i]
        base = sum(len(c["rows"][img][j + 1]) for j in range(k))
        rows = base + e["order"]
        assert np.array_equal(out["rank"][i, rows], np.arange(len(rows)))
        got[k, a, i] = (out["dtm"][:, a, i, rows].astype(bool), out["dtig"][:, a, i, rows].astype(bool))
    return got


def box(x, y, w, h, s):
    return [x, y, x + w, y + h, s]


def hand_cases():
    """name -> case; the answers are derived in tests/test_eval_device_host.py."""
    cs = {}
    # (a) two ground truths, one detection exactly on the first, one far away
    cs["a"] = case([1], [1], {1: {1: [box(10, 10, 40, 40, .9), box(300, 300, 40, 40, .8)]}},
                   [gt(1, 1, 10, 10, 40, 40), gt(1, 1, 100, 100, 40, 40)])
    # (b) a crowd box absorbs three detections (scored above the true positive); a fourth overlaps it by half of ITS area
    cs["b"] = case([1], [1], {1: {1: [box(10, 10, 30, 30, .9), box(20, 20, 30, 30, .8), box(50, 50, 40, 40, .7),
                                     box(200, 200, 50, 50, .6), box(90, 0, 20, 20, .5)]}},
                   [gt(1, 1, 0, 0, 100, 100, crowd=1), gt(1, 1, 200, 200, 50, 50)])
    # (c) a ground truth of area 900 (small); an unmatched detection of area 10000 scored above the hit
    cs["c"] = case([1], [1], {1: {1: [box(10, 10, 30, 30, .9), box(200, 200, 100, 100, .95)]}}, [gt(1, 1, 10, 10, 30, 30)])
    # (d) two ground truths, both found: maxDets = 1 sees only the better detection
    cs["d"] = case([1], [1], {1: {1: [box(10, 10, 40, 40, .9), box(100, 100, 40, 40, .8)]}},
                   [gt(1, 1, 10, 10, 40, 40), gt(1, 1, 100, 100, 40, 40)])
    # (e) 0.799 (a miss, image 1) and 0.801 (the hit, image 2) are both 0.80 after the cut: (image, rank) order decides
    cs["e"] = case([1, 2], [1], {1: {1: [box(300, 300, 40, 40, .799)]}, 2: {1: [box(10, 10, 40, 40, .801)]}},
                   [gt(2, 1, 10, 10, 40, 40)])
    # (f) category 2 has a detection and no ground truth; category 1 has ground truth and no detection
    cs["f"] = case([1], [1, 2], {1: {2: [box(10, 10, 40, 40, .9)]}}, [gt(1, 1, 10, 10, 40, 40)])
    # (g) integer boxes with IoU exactly 0.5 in COCO's convention: 100 / (100 + 200 - 100)
    cs["g"] = case([1], [1], {1: {1: [box(0, 0, 10, 10, .9)]}}, [gt(1, 1, 0, 0, 10, 20)])
    # ... and in VOC's + 1 convention: x2 = 9 is a width of 10
    cs["g_voc"] = case([1], [1], {1: {1: [[0, 0, 9, 9, .9]]}}, [gt(1, 1, 0, 0, 9, 19)])
    return cs


def random_case(seed=5, n_images=40, n_cats=5, max_boxes=12):
    """Boxes on an integer grid (many exactly equal overlaps), float32 scores that tie after the cut, some crowd flags,
    areas on both sides of 32^2 and 96^2, detections that copy / shift ground truths."""
    rng = np.random.default_rng(seed)
    image_ids, cat_ids = list(range(101, 101 + n_images)), [3, 7, 8, 20, 41][:n_cats]
    rows, gts = {}, []
    for i in image_ids:
        rows[i] = {}
        for k, cat in enumerate(cat_ids):
            ng = int(rng.integers(0, max_boxes + 1)) if rng.random() < 0.7 else 0
            mine = []
            for _ in range(ng):
                x, y = rng.integers(0, 200, 2)
                w, h = rng.integers(4, 130, 2)
                mine.append((x, y, w, h))
                gts.append(gt(i, cat, x, y, w, h, crowd=int(rng.random() < 0.15),
                              area=float(w * h) * (1.0 if rng.random() < 0.5 else 0.6)))
            dets = []
            for _ in range(int(rng.integers(0, max_boxes + 1))):
                if mine and rng.random() < 0.7:
                    x, y, w, h = mine[int(rng.integers(len(mine)))]
                    x, y = x + int(rng.integers(-4, 5)), y + int(rng.integers(-4, 5))
                    w, h = max(1, w + int(rng.integers(-6, 7))), max(1, h + int(rng.integers(-6, 7)))
                else:
                    x, y = rng.integers(0, 200, 2)
                    w, h = rng.integers(4, 130, 2)
                dets.append(box(x, y, w, h, float(rng.random())))
            rows[i][k + 1] = dets
    return case(image_ids, cat_ids, rows, gts)


def big_case():
    """One (image, category) with D = 130 detections, cut to 100, and G = 300 ground truths -- D x G beyond the LDS matrix --
    and a second category with G = 3, inside it."""
    rng = np.random.default_rng(9)
    gts, dets = [], []
    for j in range(300):
        x, y = 12 * (j % 25), 12 * (j // 25)
        gts.append(gt(1, 1, x, y, 10, 10, crowd=int(j % 37 == 0), area=100.0 if j % 3 else 2000.0))
    for j in range(130):
        g = int(rng.integers(300))
        x, y = 12 * (g % 25) + int(rng.integers(-2, 3)), 12 * (g // 25) + int(rng.integers(-2, 3))
        dets.append(box(x, y, 10, 10, float(rng.random())))
    small = [box(400, 400, 40, 40, .9), box(402, 400, 40, 40, .85), box(500, 500, 20, 20, .3), box(0, 0, 5, 5, .2)]
    gts += [gt(1, 2, 400, 400, 40, 40), gt(1, 2, 500, 500, 20, 20), gt(1, 2, 600, 600, 50, 50, crowd=1)]
    return case([1], [1, 2], {1: {1: dets, 2: small}}, gts)


def voc_fixture_case():
    """tests/golden/voc_eval_ref.npz (recorded from the reference's own evaluator) as a case.  The table takes float32
    rows, as the merge block delivers them: the fixture's decimal coordinates move by < 1e-5 pixels, its scores stay
    distinct, and its overlaps nearest to the threshold are 0.495 / 0.515."""
    z = np.load(os.path.join(GOLDEN, "voc_eval_ref.npz"))
    n, classes = int(z["n_images"]), [str(c) for c in z["classes"]]
    rows = {i: {c + 1: [[r[3], r[4], r[5], r[6], r[2]] for r in z["dets"] if int(r[0]) == i and int(r[1]) == c]
                for c in range(len(classes))} for i in range(n)}
    gts = [dict(gt(int(g[0]), int(g[1]), g[2], g[3], g[4] - g[2], g[5] - g[3]), difficult=int(g[6])) for g in z["gt"]]
    return case(list(range(n)), list(range(len(classes))), rows, gts), z, classes


def as_block(c, device):
    """The case's rows as a merge-style block (boxes [B, classes, R, 5] float32, rows_out [B, classes] int32)."""
    B, K = len(c["image_ids"]), len(c["cat_ids"])
    Rm = max([1] + [len(c["rows"][i][k + 1]) for i in c["image_ids"] for k in range(K)])
    boxes, rows = np.zeros((B, K, Rm, 5), dtype=np.float32), np.zeros((B, K), dtype=np.int32)
    for b, i in enumerate(c["image_ids"]):
        for k in range(K):
            v = c["rows"][i][k + 1]
            boxes[b, k, :len(v)] = v
            rows[b, k] = len(v)
    return torch.from_numpy(boxes).to(device), torch.from_numpy(rows).to(device)
