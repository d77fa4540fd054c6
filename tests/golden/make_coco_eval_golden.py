"""Writes tests/golden/coco_eval_format.npz.  Runs in the build container only, like make_loss_golden.py: it needs the
reference checkout.

    python tests/golden/make_coco_eval_golden.py /path/to/reference

The reference's own dataset class is imported (nothing is copied) with stand-ins for the third-party imports this
container lacks: lib/datasets/dataset/coco.py::COCO is constructed against a pycocotools stub without images, which
leaves its table of category ids and its convert_eval_format (coco.py:87-112) as they are.  The fixture holds data only:

    valid_ids [80]            the dataset's category ids, as the caller of evalio.convert_eval_format_coco passes them
    image_ids [R], classes [R] (1-based), boxes [R, 5] float32 (x1, y1, x2, y2, score): one row per detection, in the
                              order of the results dict (images in order of first appearance, classes ascending; every
                              image has an entry for each of the 80 classes, most of them empty)
    expected_json             json.dumps of the reference's list for the float32 arrays (what merge_outputs hands over)
    expected_json_lists       the same for the rows as lists of Python floats (float64 arithmetic)
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def import_reference(ref_root):
    for name in ["pycocotools", "pycocotools.coco", "pycocotools.cocoeval"]:
        sys.modules.setdefault(name, types.ModuleType(name))

    class NoImages:
        def __init__(self, annot_path):
            pass

        def getImgIds(self):
            return []
    sys.modules["pycocotools.coco"].COCO = NoImages
    sys.modules["pycocotools.cocoeval"].COCOeval = type("COCOeval", (), {})
    sys.modules["pycocotools"].coco = sys.modules["pycocotools.coco"]
    # (by file: the reference's lib/datasets has no __init__.py, and an installed `datasets` package would shadow it)
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "reference_coco", os.path.join(ref_root, "lib", "datasets", "dataset", "coco.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.COCO(types.SimpleNamespace(data_dir="", task="ctdet"), "val")


def results_dict(image_ids, classes, boxes, as_lists):
    """The rows as the results dict of CtdetDetector.run over a dataset: {image id: {class: rows}}."""
    res = {}
    for img in image_ids:
        if int(img) not in res:
            res[int(img)] = {j: [] for j in range(1, 81)}
    for img, j, b in zip(image_ids, classes, boxes):
        res[int(img)][int(j)].append(b)
    for img in res:
        for j in res[img]:
            rows = np.array(res[img][j], dtype=np.float32).reshape(-1, 5)
            res[img][j] = rows.astype(np.float64).tolist() if as_lists else rows
    return res


def rows():
    rng = np.random.default_rng(808)
    out = []
    # image 397133: awkward roundings -- x.005 / x.015 / x.125 ends, a negative corner that rounds to -0.0, a score that
    # rounds up to 1.0 and one that rounds down to 0.0, sizes whose float32 difference is not the decimal difference
    out += [(397133, 1, [10.005, 20.015, 110.125, 220.375, 0.995]),
            (397133, 1, [-0.004, -0.005, 33.335, 44.445, 0.004999]),
            (397133, 1, [0.125, 0.375, 0.25, 0.625, 0.125]),
            (397133, 80, [1234.565, 2.675, 1300.0, 480.005, 0.5051]),
            (397133, 12, [100.1, 100.2, 100.3, 100.4, 0.015]),
            (397133, 12, [0.005, 0.015, 1300.0, 480.0, 0.5]),          # float32 width 1299.99, float64 width 1300.0
            (397133, 12, [639.995, 479.995, 640.0, 480.0, 1.0])]
    # image 37777: random boxes over many classes, ids beyond the gaps of the table (12 -> 13, 80 -> 90)
    for _ in range(40):
        x1, y1 = rng.uniform(-5, 600), rng.uniform(-5, 440)
        w, h = rng.uniform(0.3, 200), rng.uniform(0.3, 200)
        out.append((37777, int(rng.integers(1, 81)), [x1, y1, x1 + w, y1 + h, rng.uniform(0, 1)]))
    # image 252219: one class only; image 87038: no detections at all
    for _ in range(5):
        x1, y1 = np.round(rng.uniform(0, 500, 2) * 200) / 200        # multiples of 0.005
        out.append((252219, 45, [x1, y1, x1 + 17.005, y1 + 9.995, np.round(rng.uniform(0, 1) * 200) / 200]))
    order = {397133: 0, 37777: 1, 252219: 2}
    out.sort(key=lambda r: (order[r[0]], r[1]))                       # the order of the results dict; stable
    image_ids = np.array([r[0] for r in out] , dtype=np.int64)
    classes = np.array([r[1] for r in out], dtype=np.int32)
    boxes = np.array([r[2] for r in out], dtype=np.float32)
    return image_ids, classes, boxes


def main():
    ds = import_reference(sys.argv[1])
    image_ids, classes, boxes = rows()
    empty = 87038
    out = {"valid_ids": np.array(ds._valid_ids, dtype=np.int32), "image_ids": image_ids, "classes": classes,
           "boxes": boxes, "empty_image_id": np.array(empty, dtype=np.int64)}
    for key, as_lists in (("expected_json", False), ("expected_json_lists", True)):
        res = results_dict(image_ids, classes, boxes, as_lists)
        res[empty] = {j: ([] if as_lists else np.zeros((0, 5), dtype=np.float32)) for j in range(1, 81)}
        dets = ds.convert_eval_format(res)                            # (subtracts in place: res is rebuilt per form)
        assert len(dets) == len(boxes) and all(set(d) == {"image_id", "category_id", "bbox", "score"} for d in dets)
        out[key] = np.array(json.dumps(dets))
    assert len(out["valid_ids"]) == 80 and "-0.0" in str(out["expected_json"])
    assert str(out["expected_json"]) != str(out["expected_json_lists"])
    path = os.path.join(HERE, "coco_eval_format.npz")
    np.savez_compressed(path, **out)
    print("coco eval format: %d detections, %d bytes" % (len(boxes), os.path.getsize(path)))


if __name__ == "__main__":
    main()
