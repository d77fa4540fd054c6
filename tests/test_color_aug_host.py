"""Host side of the colour augmentation (codenet_amd/preproc.py: color_aug_params, aug_row, check_aug) and its numpy
restatement (tests/color_aug_ref.py) against the reference's own color_aug, recorded in
tests/golden/color_aug.npz by tests/golden/make_color_aug_golden.py.  No GPU."""
import functools
import os
import random

import numpy as np
import pytest

from codenet_amd import preproc
from tests import color_aug_ref as C
from tests import preproc_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24          # unit roundoff of float32
# DESIGN.md section 7.4c, "distance to the reference": every intermediate |x| < 4 (ulp 4 U), |out| < 16 (ulp 16 U).
#   gs_mean: exact here (error U), numpy's float32 pairwise mean of rounded gs values there (<= 32 U): 33 U, times |om| <= 0.4
#   contrast first:            0.4 * 33 U + 0.5 U (the product) + 4 U (the sum)           = 17.7 U
#   then a blend (x 1.4, two roundings), then brightness (x 1.4, one rounding)            -> 32.8 U -> 49.9 U
#   lighting (float32 d, <= 0.1 U; float32 sum against a float64 sum rounded once, 4 U)   -> 54 U
#   minus mean (4 U), / std >= 0.224, the quotient's rounding (16 U)                      -> 275 U = 1.64e-5
TOL = 275 * U


@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(HERE, "golden", "color_aug.npz"))


def test_restatement_against_the_reference_output():
    """Measured when written (numpy 2.2.6): worst |difference| 1.43e-6 over the 20 cases (bound 1.64e-5), 0 - 48 % of the
    elements of a case differ, by last bits."""
    g = _golden()
    assert np.array_equal(g["eig_val"], preproc.EIG_VAL) and np.array_equal(g["eig_vec"], preproc.EIG_VEC)
    assert np.array_equal(g["eig_val"], C.EIG_VAL) and np.array_equal(g["eig_vec"], C.EIG_VEC)
    assert np.array_equal(g["mean"], preproc.MEAN) and np.array_equal(g["std"], preproc.STD)
    worst, orders = 0.0, set()
    for k in range(int(g["cases"])):
        u8, seeds = g["c%d_u8" % k], g["c%d_seeds" % k]
        random.seed(int(seeds[0]))
        data_rng = np.random.RandomState(int(seeds[1]))
        row = preproc.color_aug_params(data_rng)
        # both streams stand where the reference left them
        assert random.random() == float(g["c%d_next" % k][0]) and data_rng.uniform() == float(g["c%d_next" % k][1])
        assert len(row) == preproc.AUG and row[0] == 1
        preproc.check_aug([row], 1)
        orders.add(tuple(row[1:4]))
        got, want = C.color_aug(u8, C.from_list(row)), g["c%d_out" % k]
        assert got.shape == want.shape and got.dtype == want.dtype == np.float32
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        print("case %2d %3d x %3d order %s: max %.3e, %.1f %% of the elements differ"
              % (k, u8.shape[0], u8.shape[1], row[1:4], d.max(), 100.0 * (d > 0).mean()))
        worst = max(worst, d.max())
    print("worst %.3e (bound %.3e, recorded with numpy %s, here %s)" % (worst, TOL, g["numpy_version"], np.__version__))
    assert len(orders) >= 4
    assert worst <= TOL


def test_params_equal_the_restatement_row():
    """aug_row's float32 values are those of the restatement's row(): a = float32(alpha), om = float32(1 - alpha) with the
    subtraction in float64, d rounded once; and the draws are the reference's (image.py:226-234) written out."""
    random.seed(5)
    rng = np.random.RandomState(6)
    row = preproc.color_aug_params(rng)
    random.seed(5)
    rng = np.random.RandomState(6)
    order = [0, 1, 2]
    random.shuffle(order)
    alphas = [None] * 3
    for k in order:
        alphas[k] = 1. + rng.uniform(low=-0.4, high=0.4)
    d = np.dot(C.EIG_VEC, C.EIG_VAL * rng.normal(scale=0.1, size=(3,)))
    want, got = C.row(order, alphas, d), C.from_list(row)
    assert got["order"] == want["order"] and got["on"]
    for key in ("a", "om", "d"):
        assert np.array_equal(got[key], want[key]), key
    ident, off = C.from_list(preproc.AUG_IDENTITY), C.from_list(preproc.AUG_OFF)
    assert ident["on"] and not off["on"] and np.array_equal(ident["a"], [1, 1, 1]) and not ident["om"].any()
    u8 = np.random.default_rng(3).integers(0, 256, (9, 7, 3), dtype=np.uint8)
    assert np.array_equal(C.color_aug(u8, ident), C.color_aug(u8, off))


def test_off_item_is_the_float32_chain():
    """All 256 bytes x 3 channels: an off item is ((float32(v) / float32(255)) - mean32) / std32, the reference sample's
    bits (sample/ctdet.py:76-79 without color_aug); the detector's table (float64, rounded once) differs in some entries."""
    u8 = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, axis=2)         # [256, 1, 3]
    got = C.color_aug(u8, C.from_list(preproc.AUG_OFF))[:, :, 0].T                    # [256, 3]
    want = np.empty((256, 3), dtype=np.float32)
    for v in range(256):
        for c in range(3):
            want[v, c] = (np.float32(v) / np.float32(255) - R.MEAN[c]) / R.STD[c]
    assert got.dtype == np.float32 and np.array_equal(got, want)
    ref = ((u8.astype(np.float32) / 255. - R.MEAN.reshape(1, 1, 3)) / R.STD.reshape(1, 1, 3))[:, 0]     # the sample's expression
    assert ref.dtype == np.float32 and np.array_equal(got, ref)
    differ = int((got != R.lut()).sum())
    print("%d of the 768 entries differ from the detector's table" % differ)
    assert 0 < differ < 768
    # last bits only: v / 255 (U) and the difference (U) over std >= 0.224, + the quotient's and the table's rounding
    # (|out| < 4: 4 U each) = 17 U
    assert np.abs(got.astype(np.float64) - R.lut().astype(np.float64)).max() <= 17 * U


def test_host_refusals():
    good = preproc.aug_row((2, 0, 1), (1.1, 0.9, 1.3), (0.01, -0.02, 0.03))
    assert preproc.check_aug([good, preproc.AUG_OFF], 2).shape == (2, preproc.AUG)
    for order in ((0, 0, 1), (0, 1, 3), (1, 2, 2), (0.5, 1, 2), (-1, 0, 1)):
        bad = list(good)
        bad[1:4] = order
        with pytest.raises(ValueError):
            preproc.check_aug([bad], 1)
    for k, v in ((4, float("nan")), (8, float("inf")), (12, -float("inf")), (5, 1e39)):     # 1e39: infinite as a float32
        bad = list(good)
        bad[k] = v
        with pytest.raises(ValueError):
            preproc.check_aug([good, bad], 2)
    bad = list(good)
    bad[0] = 2
    with pytest.raises(ValueError):
        preproc.check_aug([bad], 1)
    with pytest.raises(ValueError):
        preproc.check_aug([good], 2)                    # one row for two items
    with pytest.raises(ValueError):
        preproc.check_aug([good, good, good], 2)
    with pytest.raises(ValueError):
        preproc.check_aug([good[:12]], 1)
    with pytest.raises(ValueError):
        preproc.check_aug([], 1)
    # a training mode: refused before the device is looked at
    with pytest.raises(ValueError):
        preproc.PreProcess(64, 64, flip_test=True, color_aug=True)
    with pytest.raises(ValueError):
        preproc.PreProcess(64, 64, scales=(0.5, 1.0), color_aug=True)
