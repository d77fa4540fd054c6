"""The pre-processing kernel (codenet_preproc.hip: cdn_ctdet_pre_process, codenet_amd/preproc.py) against the numpy
restatement of DESIGN.md section 7.4b (tests/preproc_ref.py).  The arithmetic is integer and every float64 operation is
rounded on its own on both sides, so every comparison is torch.equal over the whole tensor."""
import argparse
import functools
import json
import math

import numpy as np
import pytest
import torch

from tests import preproc_ref as R

pytestmark = pytest.mark.gpu

SCALES = (0.5, 0.75, 1.0, 1.25, 1.5)
# smallest shapes that reach: a crop larger than the image on all four sides (negative fixed-point coordinates), odd byte
# pitches (53 * 3 = 159), the clamps of up- and down-scaling, an image that vanishes at a small scale ((1, 1): int(0.5)
# = 0), a partial last wave and more than one workgroup per plane (48 x 80 = 15 x 256: the 64 x 64 plane is 16 x 256)
IMAGES = ((37, 53), (53, 37), (64, 64), (5, 300), (1, 1))
INPUTS = ((64, 64), (48, 80))


@functools.lru_cache(maxsize=None)
def _image(hw, seed=0):
    img = np.random.default_rng(1000 * hw[0] + hw[1] + seed).integers(0, 256, hw + (3,), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _reference(hw, inp, seed=0):
    """float32 [S, 3, in_h, in_w] of the five test scales, computed once per (image, input) and shared."""
    out = []
    for sc in SCALES:
        new_h, new_w, M = R.scale_matrix(hw[0], hw[1], inp[0], inp[1], sc)
        out.append(R.pre_process(_image(hw, seed), new_h, new_w, M, inp[0], inp[1]))
    ref = torch.from_numpy(np.stack(out, 0))
    return ref


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("inp", INPUTS)
def test_equals_restatement_every_element(inp, mirror):
    from codenet_amd import preproc
    pre = preproc.PreProcess(inp[0], inp[1], scales=SCALES, flip_test=mirror, max_h=64, max_w=300)
    for k, hw in enumerate(IMAGES):
        # the three accepted kinds of image: numpy, torch on the CPU, torch on the GPU
        img = _image(hw) if k % 3 == 0 else torch.from_numpy(_image(hw).copy())
        got, metas = pre(img.cuda() if k % 3 == 2 else img)
        ref = _reference(hw, inp)
        assert got.shape == ((10 if mirror else 5), 3, inp[0], inp[1]) and got.dtype == torch.float32
        assert torch.equal(got[:5].cpu(), ref), "image %s input %s" % (hw, inp)
        if mirror:
            assert torch.equal(got[5:], torch.flip(got[:5], [3]))
        assert len(metas) == 5
        for sc, m in zip(SCALES, metas):
            assert np.array_equal(m["c"], np.array([int(hw[1] * sc) / 2.0, int(hw[0] * sc) / 2.0], dtype=np.float32))
            assert m["s"] == float(max(hw)) and m["out_height"] == inp[0] // 4 and m["out_width"] == inp[1] // 4
    # the crop is larger than the image on all four sides somewhere in this set: border pixels on every edge
    border = torch.from_numpy(R.lut()[0])
    r = _reference((37, 53), inp)[0]
    for edge in (r[:, 0, :], r[:, -1, :], r[:, :, 0], r[:, :, -1]):
        assert torch.equal(edge, border[:, None].expand_as(edge))


def test_batched_items_offset_pitch_flip_rotation():
    """Two images in one arena at a non-zero offset with pitch > 3 w; flip_src; a train_matrix crop that reaches past the
    top-left corner; a rotated matrix (M1, M3 != 0); a resized + flipped item."""
    from codenet_amd import preproc
    a, b = _image((37, 53), 1), _image((20, 31), 2)
    in_h, in_w = 48, 80
    pa, pb = 53 * 3 + 5, 31 * 3 + 1
    off_a = 7
    off_b = off_a + 37 * pa + 3
    arena = np.random.default_rng(5).integers(0, 256, off_b + 20 * pb + 11, dtype=np.uint8)
    for img, off, pitch in ((a, off_a, pa), (b, off_b, pb)):
        for y in range(img.shape[0]):
            arena[off + y * pitch: off + y * pitch + img.shape[1] * 3] = img[y].reshape(-1)
    m_corner = preproc.train_matrix(np.array([5.0, 4.0], dtype=np.float32), 60.0, in_w, in_h)     # reaches to (-25, -14)
    m_flip = preproc.train_matrix(np.array([15.5, 10.0], dtype=np.float32), 31.0 * 0.9, in_w, in_h)
    k, th = 53.0 / in_w, math.radians(17.0)
    m_rot = [k * math.cos(th), -k * math.sin(th), 9.25, k * math.sin(th), k * math.cos(th), -6.5]
    m_rs = preproc.train_matrix(np.array([23.0, 15.0], dtype=np.float32), 50.0, in_w, in_h)
    table = [preproc.item_row(off_a, 37, 53, pa, m_corner),
             preproc.item_row(off_b, 20, 31, pb, m_flip, flip_src=True),
             preproc.item_row(off_a, 37, 53, pa, m_rot),
             preproc.item_row(off_b, 20, 31, pb, m_rs, new_h=30, new_w=46, flip_src=True)]
    want = [R.pre_process(a, 37, 53, m_corner, in_h, in_w), R.pre_process(b, 20, 31, m_flip, in_h, in_w, flip_src=True),
            R.pre_process(a, 37, 53, m_rot, in_h, in_w), R.pre_process(b, 30, 46, m_rs, in_h, in_w, flip_src=True)]
    pre = preproc.PreProcess(in_h, in_w, max_h=64, max_w=64, max_items=4)
    pre.load_items(arena, table)
    out = torch.empty(4, 3, in_h, in_w, device="cuda")
    pre.run(out)
    for i in range(4):
        assert torch.equal(out[i].cpu(), torch.from_numpy(want[i])), "item %d" % i
    assert not torch.equal(out[0], out[2]) and float((out[0, :, 0, 0].cpu() - torch.from_numpy(R.lut()[0])).abs().max()) == 0
    # an item that does not lie inside the bytes given, and a matrix beyond the guard: refused before any copy
    with pytest.raises(ValueError):
        pre.load_items(arena, [preproc.item_row(off_b, 21, 31, pb, m_flip)])
    with pytest.raises(ValueError):
        pre.load_items(arena, [preproc.item_row(off_a, 37, 53, pa, [1.0, 0.0, 2.0 ** 20, 0.0, 1.0, 0.0])])
    pre.run(out)
    assert torch.equal(out[3].cpu(), torch.from_numpy(want[3]))


def test_captured_run_replays_for_an_image_of_any_size():
    from codenet_amd import preproc
    pre = preproc.PreProcess(64, 64, scales=SCALES, flip_test=True, max_h=64, max_w=64)
    out = torch.zeros(10, 3, 64, 64, device="cuda")
    pre.load(_image((64, 64)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pre.run(out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pre.run(out)
    for hw in ((37, 53), (60, 41)):
        pre.load(_image(hw))
        out.zero_()
        graph.replay()
        assert torch.equal(out[:5].cpu(), _reference(hw, (64, 64))), hw
        assert torch.equal(out[5:], torch.flip(out[:5], [3]))


def test_errors_leave_the_stream_usable():
    from codenet_amd import preproc
    pre = preproc.PreProcess(64, 64, scales=SCALES, max_h=40, max_w=60)
    with pytest.raises(ValueError):
        pre.load(_image((64, 64)))                        # 12288 bytes into an arena of 7200
    with pytest.raises(ValueError):
        pre.run(torch.empty(5, 3, 64, 64, device="cuda"))  # nothing loaded
    pre.load(_image((37, 53)))
    with pytest.raises(NotImplementedError):
        pre.run(torch.empty(5, 3, 64, 64))
    with pytest.raises(ValueError):
        pre.run(torch.empty(10, 3, 64, 64, device="cuda"))
    with pytest.raises(ValueError):
        pre.load(np.zeros((8, 8), dtype=np.uint8))
    out = pre.run(torch.empty(5, 3, 64, 64, device="cuda"))
    assert torch.equal(out.cpu(), _reference((37, 53), (64, 64)))


def _args(tmp_path, ckpt, out, **kw):
    return argparse.Namespace(data=str(tmp_path / "data"), load_model=ckpt, res=128, quantize=False, w2=False,
                              maxpool=False, flip_test=True, limit=0, out=str(tmp_path / out), reference_ap50=None,
                              gpu_pre=True, **kw)


def test_eval_voc_with_gpu_pre_end_to_end(tmp_path, capsys):
    from PIL import Image
    from codenet_amd import evalio, harness, preproc
    from tests.test_gpu_eval_voc import _eval_voc, _records, _tree, _write_ann
    ev = _eval_voc()
    root, images = _tree(tmp_path, [(150, 113), (100, 140), (128, 128)])
    ckpt = str(tmp_path / "model_last.pth")
    model = harness.create_model(quantize=False, seed=11)
    last_w, last_b = [p for n, p in model.named_parameters() if n.startswith("wh.") and p.shape[0] == 2]
    with torch.no_grad():                 # well-formed boxes from a random `wh` head, as tests/test_gpu_eval_voc.py does
        last_w.mul_(0.02)
        last_b.fill_(6.0)
    evalio.save_model(ckpt, 1, model)

    _write_ann(root, images, [])
    ev.run_voc(_args(tmp_path, ckpt, "o1"))
    out1 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out1["AP50"] == 0.0 and out1["images"] == 3 and "codenet_preproc.hip" in out1["note"]
    res = _records(str(tmp_path / "o1" / "results.json"), images)       # (asserts the reference's shape)
    assert {r["image_id"] for r in res} == {1, 2, 3}
    ann = [{"image_id": r["image_id"], "category_id": r["category_id"], "bbox": r["bbox"], "ignore": 0} for r in res]
    _write_ann(root, images, ann)
    ev.run_voc(_args(tmp_path, ckpt, "o2"))
    out2 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    present = {r["category_id"] for r in res}
    assert present
    for c, name in enumerate(ev.CLASSES, 1):
        ap = out2["per_class"][name]
        print("AP %s = %r" % (name, ap))
        assert (abs(ap - 1.0) <= 1e-9) if c in present else ap == 0.0, (name, ap)

    # three test scales through capture_process_scales(..., pre=pre): image 1 against the eager composition
    scales = [0.5, 1.0, 1.5]
    ev.run_voc(_args(tmp_path, ckpt, "o3", test_scales="0.5,1,1.5"))
    capsys.readouterr()
    det = json.load(open(str(tmp_path / "o3" / "results.json")))
    m2 = harness.create_model(quantize=False)
    evalio.load_model(m2, ckpt)
    m2 = m2.cuda().eval().enable_fused()
    img = np.asarray(Image.open(str(root / "images" / images[0]["file_name"])).convert("RGB"))
    pre = preproc.PreProcess(128, 128, scales=scales, flip_test=True, max_h=150, max_w=150)
    inp, metas = pre(img)
    _, _, want = harness.process_scales(m2, inp, 3, True, metas, scales, nms=True)
    rows = 0
    for c in range(1, 21):
        got = np.array(det[c][0], dtype=np.float32).reshape(-1, 5)
        assert got.shape == want[c].shape and np.array_equal(got, want[c]), "class %d" % c
        rows += len(got)
    assert rows > 0
