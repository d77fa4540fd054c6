"""Writes tests/golden/color_aug.npz.  Runs in the build container only, like make_loss_golden.py: it needs the reference
checkout.

    python tests/golden/make_color_aug_golden.py /path/to/reference

The reference's own lib/utils/image.py::color_aug is imported (nothing is copied) and driven as
lib/datasets/sample/ctdet.py:76-79 drives it: inp.astype(float32) / 255., color_aug(data_rng, inp, eig_val, eig_vec),
(inp - mean) / std, HWC -> CHW.  cv2 is not in this container: the stand-in module has the one function color_aug reaches,
cvtColor(img, COLOR_BGR2GRAY), by its definition on float32: (b 0.114 + g 0.587) + r 0.299.

Per case k: `c{k}_u8` the byte crop [h, w, 3] (some half black: the zero border of a crop larger than its image),
`c{k}_seeds` = (seed of the `random` module, seed of the numpy RandomState), `c{k}_out` the reference's float32
[3, h, w], `c{k}_next` = the next random.random() and the next data_rng.uniform() after the call (where the two streams
stand).  `numpy_version`, `eig_val`, `eig_vec`, `mean`, `std`: what the run used (pascal.py:15-18, 38-44).
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32

MEAN = np.array([0.485, 0.456, 0.406], dtype=f32).reshape(1, 1, 3)
STD = np.array([0.229, 0.224, 0.225], dtype=f32).reshape(1, 1, 3)
EIG_VAL = np.array([0.2141788, 0.01817699, 0.00341571], dtype=f32)
EIG_VEC = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408],
                    [-0.56089297, 0.71832671, 0.41158938]], dtype=f32)
# (h, w, half black)
CASES = ([(8, 8, k == 3) for k in range(7)] + [(37, 53, k in (2, 5)) for k in range(7)]
         + [(64, 64, k in (1, 3)) for k in range(4)] + [(128, 96, k == 1) for k in range(2)])


def import_reference(ref_root):
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_BGR2GRAY = 6

    def cvtColor(img, code):
        assert code == cv2.COLOR_BGR2GRAY and img.dtype == f32 and img.ndim == 3 and img.shape[2] == 3
        return (img[..., 0] * f32(0.114) + img[..., 1] * f32(0.587)) + img[..., 2] * f32(0.299)
    cv2.cvtColor = cvtColor
    sys.modules["cv2"] = cv2
    sys.path.insert(0, os.path.join(ref_root, "lib"))
    from utils import image
    return image


def main():
    image = import_reference(sys.argv[1])
    out = {"numpy_version": np.array(np.__version__), "eig_val": EIG_VAL, "eig_vec": EIG_VEC, "mean": MEAN.reshape(3),
           "std": STD.reshape(3), "cases": np.array(len(CASES))}
    for k, (h, w, half) in enumerate(CASES):
        u8 = np.random.default_rng(9000 + k).integers(0, 256, (h, w, 3), dtype=np.uint8)
        if half:
            u8[:, : w // 2] = 0
        seeds = (100 + k, 500 + 7 * k)
        random.seed(seeds[0])
        data_rng = np.random.RandomState(seeds[1])
        inp = u8.astype(f32) / 255.
        image.color_aug(data_rng, inp, EIG_VAL, EIG_VEC)
        inp = (inp - MEAN) / STD
        assert inp.dtype == f32
        out["c%d_u8" % k] = u8
        out["c%d_seeds" % k] = np.array(seeds, dtype=np.int64)
        out["c%d_out" % k] = np.ascontiguousarray(inp.transpose(2, 0, 1))
        out["c%d_next" % k] = np.array([random.random(), data_rng.uniform()], dtype=np.float64)
    path = os.path.join(HERE, "color_aug.npz")
    np.savez_compressed(path, **out)
    print("color_aug: %d cases, %d bytes, numpy %s" % (len(CASES), os.path.getsize(path), np.__version__))


if __name__ == "__main__":
    main()
