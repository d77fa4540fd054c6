"""The detection scorer's kernels (codenet_eval.hip) against its `_host` entries, which tests/test_eval_device_host.py pins
to the VOC fixture, the Python text formatting, hand-derived answers and tests/coco_eval_ref.py.  Both sides run the same
cdn_eval.h; everything is np.array_equal."""
import numpy as np
import pytest
import torch

from codenet_amd import evalio, harness
from tests import eval_cases as C
from tests.test_eval_device_host import _cut_inputs

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


def _gpu():
    return torch.device("cuda", torch.cuda.current_device())


def _same_coco(a, b):
    for k in ("precision", "recall", "stats", "dtm", "dtig", "rank"):
        assert np.array_equal(a[k], b[k]), k


def _same_voc(a, b):
    for k in ("ap_07", "ap_area", "npos"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("rec", "prec"):
        assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k


def _same_table(a, b):
    assert np.array_equal(a.count.cpu().numpy(), b.count.cpu().numpy()) and int(a.flag.cpu()[0]) == int(b.flag.cpu()[0])
    for s in range(a.n_images):
        n = int(b.count[s])
        assert np.array_equal(a.det[s, :n].cpu().numpy(), b.det[s, :n].cpu().numpy())


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f", "g"])
def test_coco_hand_cases_equal_the_host_entries(name):
    c = C.hand_cases()[name]
    got, tab = C.run_coco(c, _gpu())
    want, tab_h = C.run_coco(c, CPU)
    _same_table(tab, tab_h)
    _same_coco(got, want)


def test_coco_random_case_equals_the_host_entries():
    c = C.random_case()
    got, tab = C.run_coco(c, _gpu(), via_block=True)
    want, tab_h = C.run_coco(c, CPU)          # (one append per image there, one block of 40 here)
    _same_table(tab, tab_h)
    _same_coco(got, want)
    assert (want["stats"] > 0.01).all()


def test_coco_big_cell_beside_the_lds_matrix_equals_the_host_entries():
    """D = 130 detections, cut to 100, against G = 300 ground truths: 30000 overlaps, formed on the fly; the second
    category (D = 4, G = 3) takes the LDS matrix."""
    c = C.big_case()
    got, _ = C.run_coco(c, _gpu(), cap=160)
    want, _ = C.run_coco(c, CPU, cap=160)
    _same_coco(got, want)
    assert int((want["rank"][0] < 100).sum()) == 104 and want["dtm"][:, 0, 0].any()


def test_voc_fixture_random_case_and_threshold_case_equal_the_host_entries():
    cases = [C.voc_fixture_case()[0], C.hand_cases()["g_voc"], C.random_case(seed=11, n_images=60, n_cats=3)]
    for g in cases[2]["gts"]:
        g["difficult"] = g["iscrowd"]
    for c in cases:
        got, tab = C.run_voc(c, _gpu(), cap=64)
        want, tab_h = C.run_voc(c, CPU, cap=64)
        _same_table(tab, tab_h)
        _same_voc(got, want)
    assert max(len(r) for r in want["rec"]) > 256        # more than one pass of the workgroup scans


def test_two_decimal_cut_equals_the_host_entries():
    v = _cut_inputs()
    v = np.concatenate([v, np.zeros(23000 - len(v), dtype=np.float32)]).reshape(23, 1, 1000)
    boxes = np.zeros((23, 1, 1000, 5), dtype=np.float32)
    boxes[..., 0], boxes[..., 2], boxes[..., 4] = v, v[:, :, ::-1], v
    rows = torch.full((23, 1), 1000, dtype=torch.int32)
    tabs = []
    for dev in (_gpu(), CPU):
        t = evalio.DeviceResults(23, 1, cap=1000, coco=True, device=dev)
        t.append((torch.from_numpy(boxes).to(dev), rows.to(dev)), 0)
        tabs.append(t)
    _same_table(*tabs)
    a, b = tabs[0].det.cpu().numpy(), tabs[1].det.numpy()
    assert np.array_equal(np.signbit(a), np.signbit(b))


def test_append_from_a_real_merge_block_equals_unpack_merged_through_the_host_path():
    """process_scales(raw=True) of a small model, 2 x 3 x 128^2 (two test scales): the device block appended with no host
    copy against harness.unpack_merged of the same block fed to the host table as dicts -- both modes."""
    model = harness.create_model(quantize=False, seed=3).cuda().enable_fused()
    g = torch.Generator().manual_seed(5)
    images = torch.randn(2, 3, 128, 128, generator=g).cuda()
    scales = [1.0, 1.5]
    metas = [{"c": np.array([int(120 * sc) / 2.0, int(90 * sc) / 2.0], dtype=np.float32), "s": 120.0, "out_height": 32,
              "out_width": 32} for sc in scales]
    _, _, raw = harness.process_scales(model, images, 2, False, metas, scales, raw=True)
    dicts, counters = harness.unpack_merged(raw[0].cpu(), 1, 20, 2 * 100)
    assert int(counters["rows_out"].sum()) >= 50
    for coco in (False, True):
        dev_t = evalio.DeviceResults(3, 20, cap=100, coco=coco, device=_gpu())
        host_t = evalio.DeviceResults(3, 20, cap=100, coco=coco, device=CPU)
        dev_t.append(raw, 1)
        host_t.append(dicts[0], 1)
        _same_table(dev_t, host_t)
        assert int(host_t.count[1]) == int(counters["rows_out"].sum()) and int(host_t.count[0]) == 0


def test_overflow_flag_fires_for_cap_4_and_nothing_is_dropped_silently():
    c = C.hand_cases()["b"]                    # five detections in one image
    dev = _gpu()
    g = evalio.GroundTruth.from_coco_dict(C.ann_dict(c), image_ids=c["image_ids"], valid_ids=c["cat_ids"], device=dev)
    res = evalio.DeviceResults(1, 1, cap=4, coco=True, device=dev)
    res.append(C.as_block(c, dev), 0)
    with pytest.raises(RuntimeError, match="more than cap = 4"):
        evalio.coco_eval(res, g)
    assert int(res.flag.cpu()[0]) == 1 and int(res.count.cpu()[0]) == 4
    ok = evalio.DeviceResults(1, 1, cap=5, coco=True, device=dev)
    ok.append(C.as_block(c, dev), 0)
    assert np.array_equal(ok.det[0, :4].cpu().numpy(), res.det[0].cpu().numpy())
    assert abs(evalio.coco_eval(ok, g)["stats"][0] - 1.0) < 1e-12


@pytest.mark.parametrize("test_scales", ["1", "1,1.5"])
def test_eval_voc_gpu_eval_agrees_with_the_python_scorer(tmp_path, capsys, test_scales):
    """tools/eval_voc.py --gpu_eval --check_eval over a synthetic VOC tree (single scale: the merge kernel's block with one
    scale; two scales: the captured graph's own block): pass 1 without ground truth leaves results.json from the device
    table; pass 2 scores the run's own detections as ground truth -- AP 1 for every class present -- and --check_eval
    raises on any difference between the two scorers."""
    import json
    from tests.test_gpu_eval_voc import _args, _eval_voc, _records, _tree, _write_ann
    ev = _eval_voc()
    root, images = _tree(tmp_path, [(200, 150), (128, 128)])
    ckpt = str(tmp_path / "model_last.pth")
    model = harness.create_model(quantize=True, seed=11)
    last_w, last_b = [p for n, p in model.named_parameters() if n.startswith("wh.") and p.shape[0] == 2]
    with torch.no_grad():
        last_w.mul_(0.02)
        last_b.fill_(6.0)
    evalio.save_model(ckpt, 1, model)

    def args(out, **kw):
        a = _args(tmp_path, ckpt, True, out)
        a.test_scales, a.gpu_eval = test_scales, True
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    _write_ann(root, images, [])
    ev.run_voc(args("o1"))
    out1 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out1["AP50"] == 0.0 and out1["scorer"].startswith("device")
    res = _records(str(tmp_path / "o1" / "results.json"), images)
    assert len(res) > 20
    ann = [{"image_id": r["image_id"], "category_id": r["category_id"], "bbox": r["bbox"], "ignore": 0} for r in res]
    _write_ann(root, images, ann)
    ev.run_voc(args("o2", check_eval=True))
    out2 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "equal to the Python scorer" in out2["scorer"]
    assert _records(str(tmp_path / "o2" / "results.json"), images) == res
    present = {r["category_id"] for r in res}
    for c, name in enumerate(ev.CLASSES, 1):
        ap = out2["per_class"][name]
        assert (1.0 - 1e-9 <= ap <= 1.0 + 1e-9) if c in present else ap == 0.0, (name, ap)
