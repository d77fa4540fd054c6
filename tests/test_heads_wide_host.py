"""Host side of the COCO heads (no GPU): the cap of the fused head tail as the library exports it, and COCO's
results.json layout (evalio.convert_eval_format_coco / save_results_coco) against a fixture recorded from the
reference's own method (tests/golden/make_coco_eval_golden.py)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def test_head_tail_cap_covers_coco():
    from codenet_amd import _native as N_
    assert N_.lib().cdn_codenet_head_tail_max_classes() >= 128
    header = open(os.path.join(HERE, "..", "include", "codenet_dcn.h")).read()
    assert "int cdn_codenet_head_tail_max_classes(void);" in header and N_.lib().cdn_abi_version() == 1


def _results(fx, as_lists):
    """The fixture's rows as the results dict {image id: {class: rows}}: every image has all 80 classes."""
    res = {}
    for img in list(fx["image_ids"]) + [fx["empty_image_id"]]:
        res.setdefault(int(img), {j: [] for j in range(1, 81)})
    for img, j, b in zip(fx["image_ids"], fx["classes"], fx["boxes"]):
        res[int(img)][int(j)].append(b)
    for img in res:
        for j in res[img]:
            rows = np.array(res[img][j], dtype=np.float32).reshape(-1, 5)
            res[img][j] = rows.astype(np.float64).tolist() if as_lists else rows
    return res


def test_coco_eval_format_equals_the_reference(tmp_path):
    from codenet_amd import evalio
    fx = np.load(os.path.join(HERE, "golden", "coco_eval_format.npz"))
    valid_ids = [int(v) for v in fx["valid_ids"]]
    assert len(valid_ids) == 80 and fx["boxes"].dtype == np.float32
    for key, as_lists in (("expected_json", False), ("expected_json_lists", True)):
        res = _results(fx, as_lists)
        before = json.dumps({i: {j: np.asarray(v).tolist() for j, v in d.items()} for i, d in res.items()})
        got = evalio.convert_eval_format_coco(res, valid_ids)
        assert json.dumps(got) == str(fx[key]), key
        # the input is left as it was (the reference turns its rows into [x, y, w, h, score])
        assert before == json.dumps({i: {j: np.asarray(v).tolist() for j, v in d.items()} for i, d in res.items()})
        assert json.dumps(evalio.convert_eval_format_coco(res, valid_ids)) == str(fx[key])
    assert len(got) == len(fx["boxes"]) and all(isinstance(d["image_id"], int) and isinstance(d["category_id"], int)
                                                and all(isinstance(v, float) for v in d["bbox"] + [d["score"]]) for d in got)
    assert {d["category_id"] for d in got} <= set(valid_ids) and any(d["category_id"] == 90 for d in got)
    path = evalio.save_results_coco(_results(fx, False), valid_ids, str(tmp_path))
    assert os.path.basename(path) == "results.json" and open(path).read() == str(fx["expected_json"])
