"""Numpy restatement of the fp32 stem in training as codenet_amd/csrc/codenet_stem_fp32_train.hip computes it (DESIGN.md
section 4.3h), on top of tests/bn_block_ref.py (bn_z, the running update, the second pass) and the (channel, slab) sum order
of tests/heads_fp32_ref.py (`slab_sums`, `batch_stats`, `_finish`): every float32 operation rounded on its own, T1 / T2 in
float64 in the kernels' own order -- so on equal y0 every number but grad_W is the kernels' bit for bit.  The convolution's
fma chain and grad_W's float32 chunk sums are not restated: `stem(..., given={"y0": ...})` takes the GPU's own y0 (absent: the
float64 value rounded once), and grad_W comes as its float64 sum over the restatement's float32 grad_y0 with the sum of its
|terms| (the bound of tests/qat_support.within)."""
import numpy as np

from tests import bn_block_ref as R
from tests import heads_fp32_ref as H

F = np.float32


def out_hw(Hh, W, S):
    return (Hh - 1) // S + 1, (W - 1) // S + 1


def patches(x, S):
    """[N, 27, Ho, Wo] float32: the taps of every output position in (ci, dy, dx) order, zero outside the image."""
    x = np.asarray(x, F)
    Nb, C, Hh, W = x.shape
    Ho, Wo = out_hw(Hh, W, S)
    xp = np.zeros((Nb, C, S * (Ho - 1) + 3, S * (Wo - 1) + 3), F)
    xp[:, :, 1:Hh + 1, 1:W + 1] = x[:, :, :xp.shape[2] - 1, :xp.shape[3] - 1]
    cols = [xp[:, c, dy:dy + S * (Ho - 1) + 1:S, dx:dx + S * (Wo - 1) + 1:S]
            for c in range(C) for dy in range(3) for dx in range(3)]
    return np.stack(cols, axis=1)


def conv64(x, w, S):
    """The convolution in float64 (its 27 products are exact there), [N, Co, Ho, Wo]."""
    w = np.asarray(w, F).reshape(len(w), -1).astype(np.float64)
    return np.einsum("ok,nkhw->nohw", w, patches(x, S).astype(np.float64))


def _windows(Hh, W):
    Hp, Wp = out_hw(Hh, W, 2)
    return Hp, Wp, [(dy, dx, slice(dy, dy + 2 * Hp - 1, 2), slice(dx, dx + 2 * Wp - 1, 2)) for dy in range(3) for dx in range(3)]


def pool_scan(a0):
    """(out, arg) of maxpool3x3_s2_p1 on a0: the winner of `val > max || isnan(val)` from -inf over the window's taps inside
    the plane in row-major scan order, and its tap index dy * 3 + dx.  (A tap outside is -inf here: it never wins.)"""
    a0 = np.asarray(a0, F)
    Nb, C, Hh, W = a0.shape
    Hp, Wp, taps = _windows(Hh, W)
    ap = np.full((Nb, C, 2 * Hp + 1, 2 * Wp + 1), -np.inf, F)
    ap[:, :, 1:Hh + 1, 1:W + 1] = a0
    m = np.full((Nb, C, Hp, Wp), -np.inf, F)
    arg = np.full((Nb, C, Hp, Wp), -1, np.int64)
    with np.errstate(invalid="ignore"):
        for dy, dx, ys, xs in taps:
            v = ap[:, :, ys, xs]
            take = (v > m) | np.isnan(v)
            m = np.where(take, v, m)
            arg = np.where(take, dy * 3 + dx, arg)
    return m.astype(F), arg


def pool_gather(g, arg, Hh, W, last_wins=False):
    """G [N, C, H, W]: every pixel adds, from 0.0f in float32, the gradients of the windows it won in row-major window order.
    Window (py, px) holds pixel (y, x) at tap (y - 2 py + 1, x - 2 px + 1): an earlier window is a LATER tap, so the taps
    run backwards; within one tap the map window -> pixel is one to one.  last_wins (a wrong variant): the taps forwards."""
    g = np.asarray(g, F)
    Nb, C, Hp, Wp = g.shape
    _, _, taps = _windows(Hh, W)
    Gp = np.zeros((Nb, C, 2 * Hp + 1, 2 * Wp + 1), F)
    for dy, dx, ys, xs in (taps if last_wins else taps[::-1]):
        view = Gp[:, :, ys, xs]
        Gp[:, :, ys, xs] = np.where(arg == dy * 3 + dx, view + g, view)
    return Gp[:, :, 1:Hh + 1, 1:W + 1].copy()


def stem(x, p, gout, given=None, mutate=()):
    """The stem, forward and backward.  p: stride (2: with the pool, 4: without), float32 w [24, 27], gamma, beta, rm, rv,
    eps, momentum and the flag train.  given: {"y0": the GPU's own}.  mutate (deliberately wrong variants): "y0max" (the pool
    compared on y0 instead of a0), "order" (a pixel adds its windows in reverse order)."""
    given = given or {}
    x, gout = np.asarray(x, F), np.asarray(gout, F)
    S, eps, training = p["stride"], p["eps"], p["train"]
    pooled = S == 2
    y0 = np.asarray(given["y0"], F) if "y0" in given else conv64(x, p["w"], S).astype(F)
    Nb, C, Hh, W = y0.shape
    n = Nb * Hh * W
    o = dict(y0=y0)
    if training:
        st = H.batch_stats(y0, eps)
        o["rm"], o["rv"] = R.running_update(p["rm"], p["rv"], st, p["momentum"])
    else:
        st = H.eval_stats(p["rm"], p["rv"], eps)
        o["rm"], o["rv"] = np.asarray(p["rm"], F), np.asarray(p["rv"], F)
    z, xh = R.bn_z(y0, st["mean"], st["invstd"], p["gamma"], p["beta"])
    a0 = np.where(z < 0, F(0.0), z).astype(F)      # (a NaN stays)
    if pooled:
        m, arg = pool_scan(y0 if "y0max" in mutate else a0)
        if "y0max" in mutate:
            m = np.take_along_axis(np.pad(a0, ((0, 0), (0, 0), (1, 2), (1, 2))).reshape(Nb, C, -1),
                                   _flat_index(arg, W).reshape(Nb, C, -1), axis=2).reshape(arg.shape)
        o["out"] = m
        G = pool_gather(gout, arg, Hh, W, last_wins="order" in mutate)
        o["arg"] = arg
    else:
        o["out"] = a0
        G = gout
    gz = np.where(z > 0, G, F(0.0)).astype(F)
    gz64 = gz.astype(np.float64)
    sums = H._finish(H.slab_sums(gz64), H.slab_sums(gz64 * xh.astype(np.float64)), n)
    gy = R.backward_gy(gz, y0, st["mean"], st["invstd"], p["gamma"], sums["mb"], sums["mg"], training)
    pt = patches(x, S).astype(np.float64)
    gy64 = gy.astype(np.float64)
    o.update(st=st, z=z, xh=xh, a0=a0, G=G, g_z=gz, grad_y0=gy, **sums)
    o["grad_w_64"] = np.einsum("nohw,nkhw->ok", gy64, pt)
    o["grad_w_abs"] = np.einsum("nohw,nkhw->ok", np.abs(gy64), np.abs(pt))
    return o


def _flat_index(arg, W):
    """The flat index, in the plane padded by (1, 2), of every window's winning tap."""
    Nb, C, Hp, Wp = arg.shape
    py, px = np.arange(Hp).reshape(1, 1, -1, 1), np.arange(Wp).reshape(1, 1, 1, -1)
    return (2 * py + arg // 3) * (W + 3) + 2 * px + arg % 3
