"""The colour augmentation of the training sample, DESIGN.md section 7.4c, restated in numpy, independent of the package:
the crop of tests/preproc_ref.py -> exact integer channel sums -> v / 255, brightness / contrast / saturation in the item's
order, lighting, (x - mean) / std.  Every operation is on explicit np.float32 / np.float64 values, each rounded once, so the
result does not depend on the numpy version.  The kernels (codenet_preproc.hip: crop_sum_kernel, color_aug_kernel) must
equal it bit for bit."""
import numpy as np

from tests import preproc_ref as R

f32, f64 = np.float32, np.float64
MEAN, STD = R.MEAN, R.STD
EIG_VAL = np.array([0.2141788, 0.01817699, 0.00341571], dtype=f32)
EIG_VEC = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408],
                    [-0.56089297, 0.71832671, 0.41158938]], dtype=f32)


def row(order=(0, 1, 2), alphas=(1.0, 1.0, 1.0), d=(0.0, 0.0, 0.0), on=True):
    """{on, order, a, om, d} from float64 alphas (index = step: 0 brightness, 1 contrast, 2 saturation) and a float64 d."""
    alphas = np.asarray(alphas, dtype=f64)
    return {"on": bool(on), "order": [int(k) for k in order], "a": alphas.astype(f32),
            "om": (f64(1.0) - alphas).astype(f32), "d": np.asarray(d, dtype=f64).astype(f32)}


def from_list(r):
    """The 13-value row of codenet_amd.preproc.aug_row() -> the dict form used here (the values are float32 already)."""
    r = [float(v) for v in r]
    return {"on": r[0] != 0.0, "order": [int(v) for v in r[1:4]], "a": np.array(r[4:7], dtype=f32),
            "om": np.array(r[7:10], dtype=f32), "d": np.array(r[10:13], dtype=f32)}


def sums(u8):
    """uint8 [h, w, 3] -> the three exact channel sums as Python integers."""
    return [int(u8[..., c].astype(np.int64).sum()) for c in range(3)]


def gs_mean(S, n):
    """float32(((0.114 S0 + 0.587 S1) + 0.299 S2) / (255.0 n)) in float64, every operation rounded on its own."""
    p0, p1, p2 = f64(0.114) * f64(S[0]), f64(0.587) * f64(S[1]), f64(0.299) * f64(S[2])
    return f32(((p0 + p1) + p2) / (f64(255.0) * f64(n)))


def color_aug(u8, r, mean=MEAN, std=STD):
    """uint8 [h, w, 3] (border pixels 0 included) and a row -> float32 [3, h, w]."""
    x = u8.astype(f32) / f32(255)                                     # float32 / float32
    assert x.dtype == f32
    if r["on"]:
        gm = gs_mean(sums(u8), u8.shape[0] * u8.shape[1])
        gs = (x[..., 0] * f32(0.114) + x[..., 1] * f32(0.587)) + x[..., 2] * f32(0.299)    # of the un-augmented pixel
        for k in r["order"]:
            a, om = f32(r["a"][k]), f32(r["om"][k])
            if k == 0:
                x = x * a
            elif k == 1:
                x = x * a + gm * om
            else:
                x = x * a + (gs * om)[..., None]
            assert x.dtype == f32
        x = x + r["d"].astype(f32)[None, None, :]
    out = (x - np.asarray(mean, dtype=f32).reshape(1, 1, 3)) / np.asarray(std, dtype=f32).reshape(1, 1, 3)
    assert out.dtype == f32
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def crop_u8(img, new_h, new_w, M, out_h, out_w, flip_src=False):
    """The bytes of section 7.4b's resize + crop + flip_src: uint8 [out_h, out_w, 3]."""
    if (new_h, new_w) != img.shape[:2]:
        img = R.resize(img, new_h, new_w)
    return R.crop(img, M, out_h, out_w, flip_src)


def pre_process_aug(img, new_h, new_w, M, out_h, out_w, r, flip_src=False):
    """-> (float32 [3, out_h, out_w], [S0, S1, S2])."""
    u8 = crop_u8(img, new_h, new_w, M, out_h, out_w, flip_src)
    return color_aug(u8, r), sums(u8)
