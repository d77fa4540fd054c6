"""How long does scoring take?  The Python scorer of tools/eval_voc.py (voc_eval over every class, as run_voc calls it)
against the device scorer (evalio.voc_eval_device) on the same synthetic VOC-sized results -- 4952 images x 100
detections, 20 classes -- and the numpy restatement tests/coco_eval_ref.py against evalio.coco_eval on 5000 images x 100
detections, 80 classes.  Regions are interleaved (Python, device, Python, device, ...) and medians reported; the results
of the two sides are compared exactly (VOC) / to the last bit of the twelve statistics (COCO) on the way.

    python tools/eval_bench.py [--reps 3] [--coco_reps 1] [--voc_images 4952] [--coco_images 5000] [--device cuda]

Prints one JSON line.  The device figures include everything voc_eval_device / coco_eval do: the match launch, the key
launch, torch.sort, the accumulate launch and the one copy of the results to the host.  `fill_ms` is the time to put the
detections into the table from HOST blocks (upload + append, 64 images per call); in tools/eval_voc.py --gpu_eval the blocks
are already on the device."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np      # noqa: E402
import torch            # noqa: E402

from codenet_amd import evalio      # noqa: E402


def synthetic(n_images, n_classes, per_image, seed):
    """-> (rows {image: {class (1-based): float32 [n, 5]}}, COCO-layout annotations).  1-5 ground truths per image; 60 %
    of the detections are jittered copies of one of them, the rest random."""
    rng = np.random.default_rng(seed)
    rows, anns = {}, []
    for i in range(n_images):
        ng = int(rng.integers(1, 6))
        gc = rng.integers(0, n_classes, ng)
        gb = np.concatenate([rng.integers(0, 400, (ng, 2)), rng.integers(20, 200, (ng, 2))], 1).astype(np.float64)
        for c, b in zip(gc, gb):
            anns.append({"image_id": i, "category_id": int(c) + 1, "bbox": [float(v) for v in b], "area": float(b[2] * b[3]),
                         "iscrowd": int(rng.random() < 0.05), "difficult": int(rng.random() < 0.1)})
        src = rng.integers(0, ng, per_image)
        copy = rng.random(per_image) < 0.6
        cls = np.where(copy, gc[src], rng.integers(0, n_classes, per_image))
        xywh = np.where(copy[:, None], gb[src] + rng.normal(0, 6, (per_image, 4)),
                        np.concatenate([rng.integers(0, 400, (per_image, 2)), rng.integers(20, 200, (per_image, 2))], 1))
        xywh[:, 2:] = np.maximum(xywh[:, 2:], 2.0)
        det = np.concatenate([xywh[:, :2], xywh[:, :2] + xywh[:, 2:], rng.random((per_image, 1))], 1).astype(np.float32)
        rows[i] = {c + 1: det[cls == c] for c in range(n_classes)}
    return rows, anns


def fill(rows, n_classes, coco, device, chunk=64):
    n = len(rows)
    table = evalio.DeviceResults(n, n_classes, cap=100, coco=coco, device=device)
    for lo in range(0, n, chunk):
        table.append([rows[i] for i in range(lo, min(n, lo + chunk))], lo)
    return table


def sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def timed(fn, device):
    sync(device)
    t0 = time.perf_counter()
    out = fn()
    sync(device)
    return (time.perf_counter() - t0) * 1e3, out


def bench_voc(args, device):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import eval_voc as ev
    rows, anns = synthetic(args.voc_images, 20, 100, seed=1)
    ann = {"images": [{"id": i} for i in range(args.voc_images)], "categories": [{"id": c} for c in range(1, 21)],
           "annotations": anns}
    gts = {c: {} for c in range(1, 21)}                       # as run_voc builds them
    for a in anns:
        x, y, w, h = a["bbox"]
        g = gts[a["category_id"]].setdefault(a["image_id"], ([], []))
        g[0].append([x, y, x + w, y + h])
        g[1].append(bool(a.get("ignore", 0) or a.get("difficult", 0)))
    gts = {c: {k: (np.array(b, dtype=np.float64), np.array(d, dtype=bool)) for k, (b, d) in v.items()} for c, v in gts.items()}
    ids = list(range(args.voc_images))

    def python_scorer():
        aps = []
        for c in range(1, 21):
            rws = [(i, float(r[4]), *map(float, r[:4])) for i in ids for r in rows[i][c]]
            aps.append(ev.voc_eval(rws, gts[c]))
        return np.array(aps)

    gt = evalio.GroundTruth.from_coco_dict(ann, image_ids=ids, valid_ids=list(range(1, 21)), voc=True, device=device)
    fill_ms, table = timed(lambda: fill(rows, 20, False, device), device)
    evalio.voc_eval_device(table, gt)                          # warm-up: code objects, allocator
    t_py, t_dev, same = [], [], True
    for _ in range(args.reps):
        ms, want = timed(python_scorer, device)
        t_py.append(ms)
        ms, got = timed(lambda: evalio.voc_eval_device(table, gt), device)
        t_dev.append(ms)
        same = same and bool(np.array_equal(got["ap_07"], want))
    return {"images": args.voc_images, "detections": args.voc_images * 100, "classes": 20, "reps": args.reps,
            "python_ms": statistics.median(t_py), "device_ms": statistics.median(t_dev), "python_all_ms": t_py,
            "device_all_ms": t_dev, "fill_ms": fill_ms, "ap_07_equal": same, "mean_ap_07": float(np.mean(got["ap_07"]))}


def bench_coco(args, device):
    from tests import coco_eval_ref as R
    K = 80
    rows, anns = synthetic(args.coco_images, K, 100, seed=2)
    ids, cats = list(range(args.coco_images)), list(range(1, K + 1))
    ann = {"images": [{"id": i} for i in ids], "categories": [{"id": c} for c in cats], "annotations": anns}
    dts = [{"image_id": i, "category_id": c, "bbox": b[:4], "score": b[4]} for i in ids for c in cats
           for b in R.cut_rows(rows[i][c])]
    gt = evalio.GroundTruth.from_coco_dict(ann, image_ids=ids, valid_ids=cats, device=device)
    fill_ms, table = timed(lambda: fill(rows, K, True, device), device)
    evalio.coco_eval(table, gt)
    t_np, t_dev, same = [], [], True
    reps = max(args.reps, args.coco_reps)
    for r in range(reps):
        want = None
        if r < args.coco_reps:
            ms, want = timed(lambda: R.coco_eval(dts, anns, ids, cats), device)
            t_np.append(ms)
        ms, got = timed(lambda: evalio.coco_eval(table, gt), device)
        t_dev.append(ms)
        if want is not None:
            same = same and bool(np.array_equal(got["stats"], want["stats"]) and np.array_equal(got["precision"], want["precision"]))
    return {"images": args.coco_images, "detections": args.coco_images * 100, "classes": K, "numpy_reps": args.coco_reps,
            "device_reps": reps, "numpy_ms": statistics.median(t_np) if t_np else None, "device_ms": statistics.median(t_dev),
            "numpy_all_ms": t_np, "device_all_ms": t_dev, "fill_ms": fill_ms, "equal": same, "stats": [float(v) for v in got["stats"]]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--coco_reps", type=int, default=1, help="runs of the numpy restatement (minutes each at full size)")
    ap.add_argument("--voc_images", type=int, default=4952)
    ap.add_argument("--coco_images", type=int, default=5000)
    ap.add_argument("--device", default="cuda", help="cpu: the `_host` entries (one thread) instead of the kernels")
    ap.add_argument("--skip_coco", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    device = torch.device(args.device)
    out = {"device": str(device), "voc": bench_voc(args, device)}
    if not args.skip_coco:
        out["coco"] = bench_coco(args, device)
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
