"""A plain numpy restatement of COCO's bbox evaluation -- evaluateImg, accumulate and summarize as DESIGN.md section 7.4e
writes them down -- for tests/test_eval_device_host.py and tests/test_gpu_eval_device.py.  It imports no COCO library and is
not a copy of one: the yardstick for the native scorer is this text plus the hand-derived cases of the tests.

    dts   list of {"image_id", "category_id", "bbox": [x, y, w, h], "score"}   (in results.json order)
    gts   list of {"image_id", "category_id", "bbox": [x, y, w, h], "area", "iscrowd"}
"""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(.0, 1.00, 101)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
MAX_DETS = [1, 10, 100]


def to_float(v):
    """The reference's two-decimal cut (coco.py:87-112)."""
    return float("{:.2f}".format(v))


def cut_rows(rows):
    """float32 rows [n, 5] (x1, y1, x2, y2, score) -> [[x, y, w, h, score]] with the cut; w, h formed in float32."""
    out = []
    for r in np.asarray(rows, dtype=np.float32).reshape(-1, 5):
        b = np.array(r)
        b[2] -= b[0]
        b[3] -= b[1]
        out.append([to_float(v) for v in b])
    return out


def bb_iou(d, g, crowd):
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return i / u


def evaluate_img(dt, gt, a_rng, max_det=100):
    """dt, gt: the detections / ground truths of ONE (image, category), in input order.  Returns None when both are
    empty, else {"dtm" [T, D] bool, "dtig" [T, D] bool, "scores" [D], "order" [D] (input index of every kept
    detection), "npig"}."""
    if not dt and not gt:
        return None
    ig = np.array([bool(g["iscrowd"]) or g["area"] < a_rng[0] or g["area"] > a_rng[1] for g in gt], dtype=bool)
    gorder = np.argsort(ig, kind="mergesort")                    # non-ignored first, stable
    dorder = np.argsort([-d["score"] for d in dt], kind="mergesort")[:max_det]
    T, D, G = len(IOU_THRS), len(dorder), len(gt)
    dtm, dtig, gtm = np.zeros((T, D), dtype=bool), np.zeros((T, D), dtype=bool), np.zeros((T, G), dtype=bool)
    for ti, t in enumerate(IOU_THRS):
        for di, dind in enumerate(dorder):
            d = dt[dind]
            best, m = min(t, 1 - 1e-10), -1
            for gi in gorder:
                g = gt[gi]
                if gtm[ti, gi] and not g["iscrowd"]:
                    continue
                if m > -1 and not ig[m] and ig[gi]:
                    break
                o = bb_iou(d["bbox"], g["bbox"], bool(g["iscrowd"]))
                if o < best:
                    continue
                best, m = o, gi
            if m == -1:
                area = d["bbox"][2] * d["bbox"][3]
                dtig[ti, di] = area < a_rng[0] or area > a_rng[1]
                continue
            dtm[ti, di] = True
            dtig[ti, di] = ig[m]
            gtm[ti, m] = True
    return {"dtm": dtm, "dtig": dtig, "scores": np.array([dt[i]["score"] for i in dorder], dtype=np.float64),
            "order": np.asarray(dorder, dtype=np.int64), "npig": int((~ig).sum())}


def evaluate(dts, gts, image_ids, cat_ids):
    """-> {(k, a, image index): evaluate_img result}"""
    cell_d, cell_g = {}, {}
    for d in dts:
        cell_d.setdefault((d["image_id"], d["category_id"]), []).append(d)
    for g in gts:
        cell_g.setdefault((g["image_id"], g["category_id"]), []).append(g)
    out = {}
    for k, cat in enumerate(cat_ids):
        for a, rng in enumerate(AREA_RNG):
            for i, img in enumerate(image_ids):
                out[k, a, i] = evaluate_img(cell_d.get((img, cat), []), cell_g.get((img, cat), []), rng)
    return out


def accumulate(ev, n_images, K):
    T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
    precision, recall = -np.ones((T, R, K, A, M)), -np.ones((T, K, A, M))
    for k in range(K):
        for a in range(A):
            E = [ev[k, a, i] for i in range(n_images) if ev[k, a, i] is not None]
            if not E:
                continue
            npig = sum(e["npig"] for e in E)
            if npig == 0:
                continue
            for m, md in enumerate(MAX_DETS):
                scores = np.concatenate([e["scores"][:md] for e in E])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["dtm"][:, :md] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e["dtig"][:, :md] for e in E], axis=1)[:, inds]
                tps, fps = np.logical_and(dtm, ~dtig), np.logical_and(~dtm, ~dtig)
                tp_sum, fp_sum = np.cumsum(tps, axis=1).astype(np.float64), np.cumsum(fps, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + 2.220446049250313e-16)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    q = np.zeros(R)
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side="left")):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return precision, recall


def summarize(precision, recall):
    def stat(ap, iou=None, area=0, md=2):
        s = precision[:, :, :, area, md] if ap else recall[:, :, area, md]
        if iou is not None:
            s = s[np.where(iou == IOU_THRS)[0]]
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    return np.array([stat(1), stat(1, iou=.5), stat(1, iou=.75), stat(1, area=1), stat(1, area=2), stat(1, area=3),
                     stat(0, md=0), stat(0, md=1), stat(0, md=2), stat(0, area=1), stat(0, area=2), stat(0, area=3)])


def coco_eval(dts, gts, image_ids, cat_ids):
    ev = evaluate(dts, gts, image_ids, cat_ids)
    precision, recall = accumulate(ev, len(image_ids), len(cat_ids))
    return {"stats": summarize(precision, recall), "precision": precision, "recall": recall, "ev": ev}
