"""The pre-processing arithmetic of DESIGN.md section 7.4b restated in numpy (int64 / float64), independent of the package:
resize -> affine crop with a zero border (optional source flip) -> LUT normalisation -> planes.  The kernel
(codenet_preproc.hip) must equal it bit for bit."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def lut(mean=MEAN, std=STD):
    v = np.arange(256, dtype=np.float64)[:, None]
    return ((v / 255.0 - mean.astype(np.float64)) / std.astype(np.float64)).astype(np.float32)      # [256, 3]


def _axis(n_src, n_dst):
    ratio = np.float64(n_src) / np.float64(n_dst)
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * ratio - 0.5).astype(np.float32)
    i = np.floor(f)
    t = f - i                                          # float32
    i = i.astype(np.int64)
    t[i < 0] = 0
    i[i < 0] = 0
    t[i >= n_src - 1] = 0
    i[i >= n_src - 1] = n_src - 1
    w1 = np.rint(t * np.float32(2048)).astype(np.int64)
    return i, np.minimum(i + 1, n_src - 1), 2048 - w1, w1


def resize(img, new_h, new_w):
    """uint8 [h, w, 3] -> uint8 [new_h, new_w, 3]; an empty result when a side is 0."""
    if new_h == 0 or new_w == 0:
        return np.zeros((new_h, new_w, 3), dtype=np.uint8)
    v = img.astype(np.int64)
    y0, y1, b0, b1 = _axis(img.shape[0], new_h)
    x0, x1, a0, a1 = _axis(img.shape[1], new_w)
    rows = v[:, x0] * a0[None, :, None] + v[:, x1] * a1[None, :, None]
    out = (rows[y0] * b0[:, None, None] + rows[y1] * b1[:, None, None] + (1 << 21)) >> 22
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def crop(img, M, out_h, out_w, flip_src=False):
    """uint8 [nh, nw, 3], M = six float64 mapping output (x, y) to a source position -> uint8 [out_h, out_w, 3]."""
    M = [np.float64(m) for m in M]
    nh, nw = img.shape[:2]
    src = (img[:, ::-1] if flip_src else img).astype(np.int64)
    x, y = np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64)
    adelta, bdelta = np.rint((M[0] * x) * 1024).astype(np.int64), np.rint((M[3] * x) * 1024).astype(np.int64)
    X0 = np.rint((M[1] * y + M[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((M[4] * y + M[5]) * 1024).astype(np.int64) + 16
    X, Y = (X0[:, None] + adelta[None, :]) >> 5, (Y0[:, None] + bdelta[None, :]) >> 5
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    acc = np.zeros((out_h, out_w, 3), dtype=np.int64)
    for ty, tx, wgt in ((0, 0, (32 - fy) * (32 - fx)), (0, 1, (32 - fy) * fx), (1, 0, fy * (32 - fx)), (1, 1, fy * fx)):
        yy, xx = sy + ty, sx + tx
        ok = (yy >= 0) & (yy < nh) & (xx >= 0) & (xx < nw)
        if nh and nw:
            acc += np.where(ok[..., None], src[np.clip(yy, 0, nh - 1), np.clip(xx, 0, nw - 1)], 0) * (wgt * 32)[..., None]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def pre_process(img, new_h, new_w, M, out_h, out_w, flip_src=False, table=None):
    """-> float32 [3, out_h, out_w].  The resize is skipped when the size does not change (with equal sizes it is the
    identity: ratio 1 gives t = 0 everywhere)."""
    if (new_h, new_w) != img.shape[:2]:
        img = resize(img, new_h, new_w)
    table = lut() if table is None else table
    px = crop(img, M, out_h, out_w, flip_src)
    return np.ascontiguousarray(np.stack([table[px[..., c], c] for c in range(3)], 0))


def scale_matrix(h, w, in_h, in_w, scale=1.0):
    """(new_h, new_w, M) of a test scale, fix_res: the closed form of the inverse of get_affine_transform(c, s, 0,
    [in_w, in_h]), written out here independently of codenet_amd.preproc."""
    nh, nw = int(h * scale), int(w * scale)
    c = np.array([nw / 2.0, nh / 2.0], dtype=np.float32)
    k = float(max(h, w)) / in_w
    return nh, nw, [k, 0.0, float(c[0]) - (in_w / 2.0) * k, 0.0, k, float(c[1]) - (in_h / 2.0) * k]

