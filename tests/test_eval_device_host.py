"""The detection scorer of codenet_eval.hip on its `_host` entries (the same cdn_eval.h the kernels run, on CPU memory; no
GPU): VOC07 AP pinned to the fixture recorded from the reference's own evaluator, the two-decimal cut against Python's
text formatting, COCO bbox scoring against hand-derived answers and against the numpy restatement
tests/coco_eval_ref.py.  COCO mode follows the algorithm as DESIGN.md section 7.4e writes it down; it is not pinned to
pycocotools' own bits (no fixture recorded from it exists)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from codenet_amd import _native, evalio
from tests import coco_eval_ref as R
from tests import eval_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
# a precision "of 1" is tp / (tp + 2.22e-16): below 1 by one ulp; the hand answers are met to far less than this
TOL = 1e-12


def _eval_voc():
    spec = importlib.util.spec_from_file_location("eval_voc", os.path.join(ROOT, "tools", "eval_voc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_voc_mode_reproduces_the_reference_evaluator_fixture():
    """rec, prec, ap_07 and ap_area of every class, np.array_equal against tests/golden/voc_eval_ref.npz."""
    c, z, classes = C.voc_fixture_case()
    out, _ = C.run_voc(c, CPU)
    nontrivial = 0
    for k, name in enumerate(classes):
        assert out["rec"][k].shape == z[name + "_rec"].shape
        assert np.array_equal(out["rec"][k], z[name + "_rec"]), name
        assert np.array_equal(out["prec"][k], z[name + "_prec"]), name
        assert np.array_equal(out["ap_07"][k], z[name + "_ap_07"]), name
        assert np.array_equal(out["ap_area"][k], z[name + "_ap_area"]), name
        nontrivial += 0.05 < float(z[name + "_ap_07"]) < 0.95
    assert nontrivial >= 3


def test_voc_mode_equals_the_python_scorer_on_ties_difficult_boxes_and_long_curves():
    """A larger VOC case than the fixture (curves of several hundred points: the pairwise area sum takes its block and
    remainder paths; tied scores; difficult boxes) against tools/eval_voc.py's functions, exactly."""
    ev = _eval_voc()
    c = C.random_case(seed=11, n_images=60, n_cats=3, max_boxes=12)
    for g in c["gts"]:
        g["difficult"] = g["iscrowd"]
    for i in c["image_ids"]:                       # scores on a coarse grid: ties within and across images
        for k in c["rows"][i]:
            c["rows"][i][k][:, 4] = np.round(c["rows"][i][k][:, 4] * 20) / 20
    out, _ = C.run_voc(c, CPU, cap=64)
    for k, cat in enumerate(c["cat_ids"]):
        gts = {}
        for i in c["image_ids"]:
            mine = [g for g in c["gts"] if g["image_id"] == i and g["category_id"] == cat]
            gts[i] = (np.array([[g["bbox"][0], g["bbox"][1], g["bbox"][0] + g["bbox"][2], g["bbox"][1] + g["bbox"][3]]
                                for g in mine], dtype=np.float64).reshape(-1, 4),
                      np.array([bool(g["difficult"]) for g in mine], dtype=bool))
        rows = [(i, float(r[4]), *map(float, r[:4])) for i in c["image_ids"] for r in c["rows"][i][k + 1]]
        rec, prec = ev.voc_eval_curve(rows, gts)
        assert len(rec) > 130
        assert np.array_equal(out["rec"][k], rec) and np.array_equal(out["prec"][k], prec)
        assert out["ap_07"][k] == ev.voc_ap07(rec, prec) and out["ap_area"][k] == ev.voc_ap_area(rec, prec)


def _cut_inputs():
    k = np.arange(0, 4001, dtype=np.float64)
    rng = np.random.default_rng(2)
    return np.concatenate([(k / 8).astype(np.float32), (k / 200).astype(np.float32), (k / 1000).astype(np.float32),
                           rng.uniform(-10, 2000, 10000).astype(np.float32), np.array([0.0, -0.0], dtype=np.float32)])


def test_two_decimal_cut_equals_the_python_text_formatting():
    """rint((double) v * 100.0) / 100.0 against float("{:.2f}".format(v)): k / 8 (exact ties such as 0.125 and 0.375),
    k / 200, k / 1000 for k <= 4000, 10^4 random float32 in [-10, 2000], and +-0 -- through the append entry, in x1 and
    in the score column; w = x2 - x1 is formed in float32."""
    v = _cut_inputs()
    n = len(v)
    boxes = np.zeros((1, 1, n, 5), dtype=np.float32)
    boxes[0, 0, :, 0] = v
    boxes[0, 0, :, 2] = v[::-1]
    boxes[0, 0, :, 4] = v
    cap = 1024
    want = np.array([R.to_float(x) for x in v])
    want_w = np.array([R.to_float(x) for x in (v[::-1] - v)])
    assert (v[::-1] - v).dtype == np.float32
    for lo in range(0, n, cap):
        hi = min(n, lo + cap)
        res = evalio.DeviceResults(1, 1, cap=cap, coco=True, device=CPU)
        res.append((torch.from_numpy(boxes[:, :, lo:hi].copy()), torch.tensor([[hi - lo]], dtype=torch.int32)), 0)
        tab = res.det[0, :hi - lo].numpy()
        assert int(res.count[0]) == hi - lo and int(res.flag[0]) == 0
        for col, w in ((0, want[lo:hi]), (4, want[lo:hi]), (2, want_w[lo:hi])):
            assert np.array_equal(tab[:, col], w)
            assert np.array_equal(np.signbit(tab[:, col]), np.signbit(w))
    assert R.to_float(np.float32(0.125)) == 0.12 and R.to_float(np.float32(0.375)) == 0.38      # ties to even


def _coco(name):
    c = C.hand_cases()[name]
    out, _ = C.run_coco(c, CPU)
    ref = R.coco_eval(C.ref_dets(c), c["gts"], c["image_ids"], c["cat_ids"])
    assert np.array_equal(out["precision"], ref["precision"]) and np.array_equal(out["recall"], ref["recall"])
    assert np.array_equal(out["stats"], ref["stats"])
    return c, out


def test_coco_a_one_of_two_ground_truths_found():
    """tp = [1, 1], fp = [0, 1], npig = 2: rc = [.5, .5], pr = [1, .5] -> every threshold's row is 1 for the 51 recall
    points <= 0.5 and 0 after.  AP = 51 / 101, AR@100 = 0.5."""
    _, out = _coco("a")
    row = np.concatenate([np.ones(51), np.zeros(50)])
    for t in range(10):
        assert np.allclose(out["precision"][t, :, 0, 0, 2], row, rtol=0, atol=TOL)
    assert abs(out["stats"][0] - 51 / 101) < TOL and abs(out["stats"][8] - 0.5) < TOL
    assert out["stats"][3] == -1.0 and out["stats"][5] == -1.0            # both ground truths are medium (area 1600)
    assert abs(out["stats"][4] - 51 / 101) < TOL


def test_coco_b_a_crowd_box_absorbs_detections_and_uses_their_own_area():
    """Three detections inside the crowd box have IoU = inter / own area = 1: matched, ignored, not FP, although they
    are scored above the true positive -> AP = 1 at the thresholds where the fifth detection is absorbed too.  That one
    overlaps the crowd box by 200 of its own 400: IoU 0.5 exactly (with the union it would be 200 / 10200), matched at
    t = 0.5 only, an ordinary FP behind the hit above it."""
    _, out = _coco("b")
    assert out["dtm"][:, 0, 0, :3].all() and out["dtig"][:, 0, 0, :3].all()
    assert out["dtm"][:, 0, 0, 3].all() and not out["dtig"][:, 0, 0, 3].any()
    assert out["dtm"][0, 0, 0, 4] == 1 and out["dtig"][0, 0, 0, 4] == 1
    assert not out["dtm"][1:, 0, 0, 4].any() and not out["dtig"][1:, 0, 0, 4].any()
    assert np.allclose(out["precision"][:, :, 0, 0, 2], 1.0, rtol=0, atol=TOL)   # the FP comes after recall 1 is reached
    assert abs(out["stats"][0] - 1.0) < TOL and abs(out["stats"][8] - 1.0) < TOL


def test_coco_c_area_ranges_ignore_ground_truths_and_unmatched_detections():
    """The ground truth (area 900) counts for `all` and `small`; for medium / large nothing counts: -1.  The unmatched
    detection of area 10000, scored above the hit, is a FP for `all` (pr = [0, .5]: AP 0.5) and ignored for `small`
    (AP 1)."""
    _, out = _coco("c")
    assert abs(out["stats"][0] - 0.5) < TOL and abs(out["stats"][3] - 1.0) < TOL
    assert out["stats"][4] == -1.0 and out["stats"][5] == -1.0 and out["stats"][10] == -1.0 and out["stats"][11] == -1.0
    assert out["dtig"][:, 1, 0, 1].all() and not out["dtig"][:, 0, 0, 1].any() and not out["dtm"][:, :, 0, 1].any()


def test_coco_d_maxdets_1_sees_only_the_best_detection_of_an_image():
    _, out = _coco("d")
    assert abs(out["stats"][6] - 0.5) < TOL and abs(out["stats"][7] - 1.0) < TOL and abs(out["stats"][8] - 1.0) < TOL


def test_coco_e_scores_that_tie_after_the_cut_keep_image_order():
    """0.799 (image 1, a miss) and 0.801 (image 2, the hit) are both 0.80: the miss comes first, pr = [0, .5], AP = 0.5.
    Ordered by the uncut scores it would be 1."""
    c, out = _coco("e")
    assert R.to_float(np.float32(.799)) == R.to_float(np.float32(.801)) == 0.8
    assert abs(out["stats"][0] - 0.5) < TOL and abs(out["stats"][8] - 1.0) < TOL


def test_coco_f_no_ground_truth_gives_minus_one_and_no_detection_gives_zero():
    _, out = _coco("f")
    assert (out["precision"][:, :, 1] == -1).all() and (out["recall"][:, 1] == -1).all()       # category 2
    assert (out["precision"][:, :, 0, 0] == 0).all() and (out["recall"][:, 0, 0] == 0).all()   # category 1, area all
    assert out["stats"][0] == 0.0 and out["stats"][8] == 0.0


def test_g_iou_exactly_one_half_matches_in_coco_mode_and_not_in_voc_mode():
    """COCO skips a ground truth when iou < t: 0.5 matches at t = 0.5.  VOC needs ovmax > 0.5: a false positive."""
    _, out = _coco("g")
    assert out["dtm"][0, 0, 0, 0] == 1 and not out["dtm"][1:, 0, 0, 0].any()
    v, _ = C.run_voc(C.hand_cases()["g_voc"], CPU)
    assert np.array_equal(v["rec"][0], [0.0]) and np.array_equal(v["prec"][0], [0.0]) and v["ap_07"][0] == 0.0
    v, _ = C.run_voc(C.hand_cases()["g_voc"], CPU, ovthresh=0.49)
    eleven = 0.0
    for _ in range(11):
        eleven += 1.0 / 11.0             # (voc_ap07's own sum: 1.0000000000000002)
    assert np.array_equal(v["rec"][0], [1.0]) and v["ap_07"][0] == eleven and v["ap_area"][0] == 1.0


def test_coco_random_case_equals_the_restatement():
    """40 images, 5 categories, <= 12 boxes each on an integer grid, some crowd flags: precision, recall, the
    per-detection flags and stats, np.array_equal."""
    c = C.random_case()
    out, res = C.run_coco(c, CPU)
    ref = R.coco_eval(C.ref_dets(c), c["gts"], c["image_ids"], c["cat_ids"])
    assert np.array_equal(out["precision"], ref["precision"])
    assert np.array_equal(out["recall"], ref["recall"])
    assert np.array_equal(out["stats"], ref["stats"])
    got = C.flags_of(c, out, ref["ev"])
    n = 0
    for key, (dtm, dtig) in got.items():
        assert np.array_equal(dtm, ref["ev"][key]["dtm"]) and np.array_equal(dtig, ref["ev"][key]["dtig"]), key
        n += dtm.shape[1]
    assert n > 2000 and (ref["stats"] > 0.01).all() and (ref["stats"] < 0.99).all()     # a non-degenerate case
    # the table itself: the cut rows in (image, class, row) order
    want = np.array([d["bbox"] + [d["score"]] for d in C.ref_dets(c)])
    tab = np.concatenate([res.det[s, :int(res.count[s]), :5].numpy() for s in range(res.n_images)])
    assert np.array_equal(tab, want)


def test_coco_big_cell_equals_the_restatement():
    """D = 130 detections cut to 100 against G = 300 ground truths, and a G = 3 category beside it."""
    c = C.big_case()
    out, _ = C.run_coco(c, CPU, cap=160)
    ref = R.coco_eval(C.ref_dets(c), c["gts"], c["image_ids"], c["cat_ids"])
    assert np.array_equal(out["precision"], ref["precision"]) and np.array_equal(out["recall"], ref["recall"])
    for key, (dtm, dtig) in C.flags_of(c, out, ref["ev"]).items():
        assert np.array_equal(dtm, ref["ev"][key]["dtm"]) and np.array_equal(dtig, ref["ev"][key]["dtig"]), key
    assert int((out["rank"][0] < 100).sum()) == 104 and int((out["rank"][0] < (1 << 30)).sum()) == 134


def test_overflow_is_reported_and_never_silent():
    """cap = 4 with five detections in an image: the flag fires, the scorer raises, the stored rows are the first four."""
    c = C.hand_cases()["b"]
    g = evalio.GroundTruth.from_coco_dict(C.ann_dict(c), image_ids=c["image_ids"], valid_ids=c["cat_ids"])
    res = evalio.DeviceResults(1, 1, cap=4, coco=True, device=CPU)
    res.append(c["rows"][1], 0)
    assert int(res.flag[0]) == 1 and int(res.count[0]) == 4
    with pytest.raises(RuntimeError, match="more than cap = 4"):
        evalio.coco_eval(res, g)
    ok = evalio.DeviceResults(1, 1, cap=5, coco=True, device=CPU)
    ok.append(c["rows"][1], 0)
    assert int(ok.flag[0]) == 0 and np.array_equal(ok.det[0, :4].numpy(), res.det[0].numpy())
    evalio.coco_eval(ok, g)


@pytest.mark.parametrize("coco", [False, True])
def test_a_nan_score_is_ranked_last_and_reported(coco):
    """Scores 0.9, NaN, 0.5 in one class (and a NaN alone in another): the rank stays a permutation -- the NaN row last --
    so the matchers touch rows of the table only, and the final call raises 'cannot be ordered'."""
    rows = {1: {1: [C.box(10, 10, 40, 40, .9), C.box(10, 10, 40, 40, float("nan")), C.box(100, 100, 40, 40, .5)],
                2: [C.box(0, 0, 5, 5, float("nan"))]}}
    c = C.case([1], [1, 2], rows, [C.gt(1, 1, 10, 10, 40, 40), C.gt(1, 1, 100, 100, 40, 40)])
    g = evalio.GroundTruth.from_coco_dict(C.ann_dict(c), image_ids=[1], valid_ids=[1, 2], voc=not coco)
    res = evalio.DeviceResults(1, 2, cap=8, coco=coco, device=CPU)
    res.append(c["rows"][1], 0)
    with pytest.raises(RuntimeError, match="cannot be ordered"):
        (evalio.coco_eval if coco else evalio.voc_eval_device)(res, g)
    if coco:      # the ranks the matcher used, through a table without the flag's error: a permutation, NaN last
        import ctypes
        lib = _native.lib()
        rank = np.full(8, -1, dtype=np.int32)
        n = 8
        gtm, dtm, dtig = np.zeros(40 * 2, np.uint8), np.zeros(40 * n, np.uint8), np.zeros(40 * n, np.uint8)
        nonign = np.zeros(2 * 4, np.int32)
        consts = np.concatenate([evalio.COCO_IOU_THRS, evalio.COCO_AREA_RNG.reshape(-1)])
        rc = lib.cdn_eval_match_coco_host(res.det.data_ptr(), res.count.data_ptr(), 1, 8, 2, g.boxes.data_ptr(),
                                          g.areas.data_ptr(), g.flags.data_ptr(), g.offsets.data_ptr(), 2,
                                          consts.ctypes.data, consts.ctypes.data + 80, gtm.ctypes.data, dtm.ctypes.data,
                                          dtig.ctypes.data, rank.ctypes.data, nonign.ctypes.data)
        assert rc == 0 and rank[:4].tolist() == [0, 2, 1, 0]
        assert dtm[:n].tolist() == [1, 0, 1, 0, 0, 0, 0, 0]           # lane 0: the NaN row matches nothing


def test_argument_validation_without_gpu():
    lib = _native.lib()
    one = 4096
    assert lib.cdn_eval_append(one, one, 1, 20, 100, 5, one, one, 5, 100, 0, one, None) == -1
    assert b"slots" in lib.cdn_last_error()
    assert lib.cdn_eval_append(one, one, 1, 20, 100, 0, one, one, 5, 2000, 0, one, None) == _native.CDN_ERR_UNSUPPORTED
    assert lib.cdn_eval_match_voc(one, one, 5, 100, 20, None, one, one, 0.5, one, one, one, None) == -1
    assert lib.cdn_eval_accumulate_coco(one, one, 5, 100, 300, one, one, one, one, one, one, one, one, one, None) \
        == _native.CDN_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        evalio.coco_eval(evalio.DeviceResults(1, 1, device=CPU),
                         evalio.GroundTruth.from_coco_dict({"images": [{"id": 1}], "categories": [{"id": 1}],
                                                            "annotations": []}))
