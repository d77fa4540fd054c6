"""Host side of the GPU pre-processing (codenet_amd/preproc.py) and its numpy restatement (tests/preproc_ref.py): the crop
matrices and metas against tools/eval_voc.pre_process, the restatement against that float path within the bound derived
from the fixed point, and the 2^20 guard.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest

from codenet_amd import preproc
from tests import preproc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5)


def _eval_voc():
    spec = importlib.util.spec_from_file_location("eval_voc", os.path.join(ROOT, "tools", "eval_voc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_identity_matrix_and_lut():
    new_h, new_w, M, meta = preproc.crop_matrix(64, 64, 64, 64)
    assert (new_h, new_w) == (64, 64) and M == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert meta["s"] == 64.0 and meta["out_height"] == 16 and meta["out_width"] == 16
    img = np.random.default_rng(0).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    table = R.lut()
    assert np.array_equal(table, preproc.lut()) and table.dtype == np.float32 and table.shape == (256, 3)
    got = R.pre_process(img, 64, 64, M, 64, 64)
    want = np.stack([table[img[..., c], c] for c in range(3)], 0)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    # the table is the reference's numpy expression (base_detector.py:67) on uint8-valued pixels, bit for bit
    expr = ((img / 255.0 - R.MEAN) / R.STD).astype(np.float32).transpose(2, 0, 1)
    assert np.array_equal(got, expr)


@pytest.mark.parametrize("hw", [(37, 53), (53, 37), (375, 500)])
def test_meta_equals_eval_voc(hw):
    ev = _eval_voc()
    img = np.zeros(hw + (3,), dtype=np.uint8)
    for res in (64, 256):
        for sc in SCALES:
            _, want = ev.pre_process(img, res, sc)
            new_h, new_w, M, meta = preproc.crop_matrix(hw[0], hw[1], res, res, sc)
            assert (new_h, new_w) == (int(hw[0] * sc), int(hw[1] * sc))
            assert set(meta) == set(want) and meta["c"].dtype == np.float32 and np.array_equal(meta["c"], want["c"])
            assert meta["s"] == want["s"] and isinstance(meta["s"], float)
            assert meta["out_height"] == want["out_height"] and meta["out_width"] == want["out_width"]
            assert (new_h, new_w, M) == R.scale_matrix(hw[0], hw[1], res, res, sc)


def test_train_matrix_is_the_same_closed_form():
    c = np.array([26.5, 18.5], dtype=np.float32)
    assert preproc.train_matrix(c, 53.0, 64, 64) == preproc.crop_matrix(37, 53, 64, 64)[2]
    M = preproc.train_matrix([10.0, 20.0], 96.0, 48, 32)
    assert M == [2.0, 0.0, 10.0 - 24 * 2.0, 0.0, 2.0, 20.0 - 16 * 2.0]


@pytest.mark.parametrize("hw", [(37, 53), (375, 500)])
@pytest.mark.parametrize("res", [64, 256])
def test_restatement_within_bound_of_float_path(hw, res):
    """Against the float path of tools/eval_voc.pre_process on a seeded noise image, after undoing mean and std.  The
    bound: the crop's coordinates are rounded to 1/32 pixel (error <= 1/64 per axis, + 1/2048 from the 1/1024 grid of
    the row and column terms), an adjacent-pixel step is at most 255, two axes: 2 * 255 * (1/64 + 1/2048), + 0.5 from
    the uint8 rounding of the crop, + 0.62 from the resize's 11-bit weights and its uint8 rounding = 9.3 < 10."""
    ev = _eval_voc()
    img = np.random.default_rng(7).integers(0, 256, hw + (3,), dtype=np.uint8)
    table = R.lut()
    back = {c: {table[v, c].item(): v for v in range(256)} for c in range(3)}
    worst = 0.0
    for sc in SCALES:
        want, _ = ev.pre_process(img, res, sc)
        want = (want[0].numpy().astype(np.float64) * R.STD.astype(np.float64)[:, None, None]
                + R.MEAN.astype(np.float64)[:, None, None]) * 255.0
        new_h, new_w, M = R.scale_matrix(hw[0], hw[1], res, res, sc)
        got = R.pre_process(img, new_h, new_w, M, res, res, table=table)
        grey = np.stack([np.vectorize(back[c].__getitem__)(got[c]) for c in range(3)], 0).astype(np.float64)
        d = np.abs(grey - want)
        print("%s res %d scale %.2f: max %.3f mean %.3f grey levels" % (hw, res, sc, d.max(), d.mean()))
        worst = max(worst, d.max())
    assert worst <= 10.0


def test_guard_rejects_coordinates_beyond_2_20():
    preproc.check_matrix([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 512, 512)
    preproc.check_matrix([2000.0, 0.0, 0.0, 0.0, 2000.0, 0.0], 512, 512)          # 511 * 2000 < 2^20
    with pytest.raises(ValueError):
        preproc.check_matrix([2100.0, 0.0, 0.0, 0.0, 1.0, 0.0], 512, 512)         # 511 * 2100 > 2^20
    with pytest.raises(ValueError):
        preproc.check_matrix([1.0, 0.0, 0.0, 0.0, 1.0, -float(1 << 20)], 512, 512)
    with pytest.raises(ValueError):
        preproc.check_matrix([1.0, 0.0, float("nan"), 0.0, 1.0, 0.0], 512, 512)
    with pytest.raises(ValueError):
        preproc.check_matrix(preproc.train_matrix([0.0, 0.0], float(1 << 30), 512, 512), 512, 512)


def test_keep_res_and_cpu_device_are_not_built():
    with pytest.raises(NotImplementedError):
        preproc.PreProcess(64, 64, keep_res=True)
    with pytest.raises(NotImplementedError):
        preproc.PreProcess(64, 64, device="cpu")
