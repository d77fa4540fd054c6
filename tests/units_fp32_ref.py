"""Numpy restatement of the fp32 ShuffleNetV2 units in training as codenet_amd/csrc/codenet_units_fp32_train.hip computes
them, on top of tests/bn_block_ref.py and tests/heads_fp32_ref.py: every float32 operation rounded
on its own, every sum in float64 in the kernels' OWN order -- the (channel, slab) protocol (`H.slab_sums`) for the BatchNorm
sums and the (plane, chunk) protocol on the depthwise INPUT plane (`H.plane_sums`) for the depthwise backward -- so on equal
inputs every number is the kernels' bit for bit.  The dense 1x1 convolutions run on MFMA kernels whose order is not restated:
`H.conv1x1_64` gives their float64 value, exact whenever the terms are; `unit(..., given=...)` takes the GPU's own instead.

The deliberately wrong variants (`mutate`): "pad" (a padded tap is relu(bn_z(0)), not 0), "col" (the stride-2 window one
column to the right), "taps" (the backward gather with the tap order reversed), "slot" (slots 0 and 1 swapped in the join),
"mb" (mb dropped where grad_y is formed), "overwrite" (branch 1's grad_x overwriting branch 2's instead of adding)."""
import numpy as np

from tests import bn_block_ref as R
from tests import heads_fp32_ref as H

F = np.float32


def out_hw(Hh, W, S):
    return (Hh - 1) // S + 1, (W - 1) // S + 1


def stats(y, rm, rv, eps, training):
    return H.batch_stats(y, eps) if training else H.eval_stats(rm, rv, eps)


def dw_forward(inp, w, S, st=None, gamma=None, beta=None, pad_value=None, col_shift=0):
    """out[p] = ((0 + w[0] a[0]) + w[1] a[1]) + .. + w[8] a[8], a[dy][dx] = a[S p + (dy, dx) - 1], taps row-major; a =
    relu(bn_z(inp)) inside the plane (st given) or inp itself, 0.0f outside."""
    inp = np.asarray(inp, F)
    a = R.forward(inp, st["mean"], st["invstd"], gamma, beta, 1) if st is not None else inp
    Nb, C, Hh, W = a.shape
    Ho, Wo = out_hw(Hh, W, S)
    ap = np.zeros((Nb, C, Hh + 2, W + 2 + col_shift), F)
    if pad_value is not None and st is not None:
        ap[:] = R.forward(np.full((1, C, 1, 1), pad_value, F), st["mean"], st["invstd"], gamma, beta, 1)
    ap[:, :, 1:Hh + 1, 1:W + 1] = a
    w = np.asarray(w, F).reshape(1, C, 3, 3)
    acc = np.zeros((Nb, C, Ho, Wo), F)
    for dy in range(3):
        for dx in range(3):
            x0 = dx + col_shift
            pr = w[:, :, dy, dx].reshape(1, C, 1, 1) * ap[:, :, dy:dy + S * (Ho - 1) + 1:S, x0:x0 + S * (Wo - 1) + 1:S]
            acc = acc + pr
    return acc.astype(F)


def bn_forward(y, st, gamma, beta):
    return R.bn_z(y, st["mean"], st["invstd"], gamma, beta)[0]


def join_backward(gout, y, st, gamma, beta, slot):
    """g_z = z > 0 ? grad_out[:, 2j + slot] : 0 and the four per-channel results, T1 / T2 in slab order."""
    return H.bn_backward1(np.asarray(gout, F)[:, slot::2], y, st, gamma, beta)


def bn_backward_sums(gz, y, st):
    """T1 = sum g_z, T2 = sum g_z xh in slab order for a BatchNorm without ReLU (g_z is the incoming gradient)."""
    gz, y = np.asarray(gz, F), np.asarray(y, F)
    d = y - R._ch(st["mean"])
    xh = (d * R._ch(st["invstd"])).astype(F)
    gz64 = gz.astype(np.float64)
    n = y.shape[0] * y.shape[2] * y.shape[3]
    return H._finish(H.slab_sums(gz64), H.slab_sums(gz64 * xh.astype(np.float64)), n)


def _landing(gy, Hh, W, S, dy, dx):
    """(G, land): G[Y][X] = grad_y[(Y + 1 - dy) / S][(X + 1 - dx) / S] where both are integers (0.0f outside the plane),
    land: where they are."""
    Nb, C, Ho, Wo = gy.shape
    gp = np.zeros((Nb, C, Ho + 2, Wo + 2), F)
    gp[:, :, 1:Ho + 1, 1:Wo + 1] = gy
    Ys = [Y for Y in range(Hh) if (Y + 1 - dy) % S == 0]
    Xs = [X for X in range(W) if (X + 1 - dx) % S == 0]
    G = np.zeros((Nb, C, Hh, W), F)
    land = np.zeros((1, 1, Hh, W), bool)
    if Ys and Xs:
        yo = [(Y + 1 - dy) // S + 1 for Y in Ys]
        xo = [(X + 1 - dx) // S + 1 for X in Xs]
        G[:, :, np.array(Ys)[:, None], np.array(Xs)[None, :]] = gp[:, :, np.array(yo)[:, None], np.array(xo)[None, :]]
        land[:, :, np.array(Ys)[:, None], np.array(Xs)[None, :]] = True
    return G, land


def dw_backward(gz, y, st2, gamma2, mb2, mg2, training2, inp, w, S, st1=None, gamma1=None, beta1=None, reverse_taps=False,
                drop_mb=False):
    """grad_y formed on load; grad_a[q] = the sum from zero, taps row-major, of w[t] grad_y[p] over the taps with q + 1 - t =
    S p; branch 2 (st1 given): g_z1 = z1 > 0 ? grad_a : 0 with T1, T2; grad_w[t] = sum over the input pixels q of grad_y[p]
    a[q], all sums in (plane, chunk) order on the input plane."""
    if drop_mb and training2:
        mb2 = np.zeros_like(np.asarray(mb2, F))
    gy = R.backward_gy(gz, y, st2["mean"], st2["invstd"], gamma2, mb2, mg2, training2)
    inp = np.asarray(inp, F)
    Nb, C, Hh, W = inp.shape
    if st1 is not None:
        z1, xh1 = R.bn_z(inp, st1["mean"], st1["invstd"], gamma1, beta1)
        a = np.where(z1 < 0, F(0.0), z1).astype(F)
    else:
        a = inp
    w = np.asarray(w, F).reshape(C, 9)
    ga = np.zeros_like(a)
    a64 = a.astype(np.float64)
    gw = []
    for t in range(9):
        G, land = _landing(gy, Hh, W, S, t // 3, t % 3)
        wt = w[:, 8 - t] if reverse_taps else w[:, t]
        pr = wt.reshape(1, C, 1, 1) * G
        ga = np.where(land, ga + pr, ga).astype(F)
        gw.append(H.plane_sums(np.where(land, G.astype(np.float64) * a64, 0.0)))
    out = dict(grad_y=gy, grad_a=ga, grad_w=np.stack(gw, axis=1).astype(F).reshape(np.asarray(w).shape))
    if st1 is not None:
        gz1 = np.where(z1 > 0, ga, F(0.0)).astype(F)
        gz64 = gz1.astype(np.float64)
        out.update(g_z=gz1, **H._finish(H.plane_sums(gz64), H.plane_sums(gz64 * xh1.astype(np.float64)), Nb * Hh * W))
    return out


def _t(w):
    w = np.asarray(w)
    return w.reshape(len(w), -1).T


def unit(x, p, gout, given=None, mutate=()):
    """One unit, forward and backward.  p: stride, float32 arrays w1 .. w5 (w2 / w4 [C, 9]), g1 .. g5, b1 .. b5, the running
    buffers rm1 .. rv5, eps, momentum and the flags train1 .. train5.  given (a dict or None): the GPU's own pointwise
    results y1, y3, y5, grad_z2, grad_z4 and grad_x2 (W1^T grad_y1); what is absent is the float64 value rounded once."""
    given = given or {}
    x, gout = np.asarray(x, F), np.asarray(gout, F)
    S, eps = p["stride"], p["eps"]
    Nb, Cx, Hh, W = x.shape
    h = len(p["w1"])
    o = {}
    st = {}

    def take(name, fn):
        return np.asarray(given[name], F) if name in given else fn().astype(F)

    def stat(k, y):
        st[k] = stats(y, p["rm%d" % k], p["rv%d" % k], eps, p["train%d" % k])
        if p["train%d" % k]:
            o["rm%d" % k], o["rv%d" % k] = R.running_update(p["rm%d" % k], p["rv%d" % k], st[k], p["momentum"])
        else:
            o["rm%d" % k], o["rv%d" % k] = np.asarray(p["rm%d" % k], F), np.asarray(p["rv%d" % k], F)
        return st[k]

    x2 = x if S == 2 else x[:, h:]
    y1 = take("y1", lambda: H.conv1x1_64(x2, p["w1"]))
    stat(1, y1)
    y2 = dw_forward(y1, p["w2"], S, st[1], p["g1"], p["b1"], pad_value=0.0 if "pad" in mutate else None,
                    col_shift=1 if ("col" in mutate and S == 2) else 0)
    stat(2, y2)
    z2 = bn_forward(y2, st[2], p["g2"], p["b2"])
    y3 = take("y3", lambda: H.conv1x1_64(z2, p["w3"]))
    stat(3, y3)
    Ho, Wo = y3.shape[2:]
    out = np.zeros((Nb, 2 * h, Ho, Wo), F)
    s2, s1 = (0, 1) if "slot" in mutate else (1, 0)
    out[:, s2::2] = R.forward(y3, st[3]["mean"], st[3]["invstd"], p["g3"], p["b3"], 1)
    if S == 2:
        y4 = dw_forward(x, p["w4"], 2, col_shift=1 if "col" in mutate else 0)
        stat(4, y4)
        z4 = bn_forward(y4, st[4], p["g4"], p["b4"])
        y5 = take("y5", lambda: H.conv1x1_64(z4, p["w5"]))
        stat(5, y5)
        out[:, s1::2] = R.forward(y5, st[5]["mean"], st[5]["invstd"], p["g5"], p["b5"], 1)
        o.update(y4=y4, z4=z4, y5=y5)
    else:
        out[:, s1::2] = x[:, :h]
    o.update(y1=y1, y2=y2, z2=z2, y3=y3, out=out, st=st)
    # ---- backward
    gx = np.zeros_like(x)
    j3 = join_backward(gout, y3, st[3], p["g3"], p["b3"], s2)
    gy3 = R.backward_gy(j3["g_z"], y3, st[3]["mean"], st[3]["invstd"], p["g3"], j3["mb"], j3["mg"], p["train3"])
    gz2 = take("grad_z2", lambda: H.conv1x1_64(gy3, _t(p["w3"])))
    s2b = bn_backward_sums(gz2, y2, st[2])
    d2 = dw_backward(gz2, y2, st[2], p["g2"], s2b["mb"], s2b["mg"], p["train2"], y1, p["w2"], S, st[1], p["g1"], p["b1"],
                     reverse_taps="taps" in mutate, drop_mb="mb" in mutate)
    gy1 = R.backward_gy(d2["g_z"], y1, st[1]["mean"], st[1]["invstd"], p["g1"], d2["mb"], d2["mg"], p["train1"])
    gx2 = take("grad_x2", lambda: H.conv1x1_64(gy1, _t(p["w1"])))
    if S == 2:
        gx[:] = gx2
    else:
        gx[:, :h] = gout[:, s1::2]
        gx[:, h:] = gx2
    o.update(join3=j3, grad_y3=gy3, grad_z2=gz2, bn2=s2b, dw2=d2, grad_y1=gy1, grad_x_b2=gx.copy())
    o["grad_w3_64"] = np.einsum("nohw,nchw->oc", gy3.astype(np.float64), z2.astype(np.float64))
    o["grad_w1_64"] = np.einsum("nohw,nchw->oc", gy1.astype(np.float64), x2.astype(np.float64))
    if S == 2:
        j5 = join_backward(gout, y5, st[5], p["g5"], p["b5"], s1)
        gy5 = R.backward_gy(j5["g_z"], y5, st[5]["mean"], st[5]["invstd"], p["g5"], j5["mb"], j5["mg"], p["train5"])
        gz4 = take("grad_z4", lambda: H.conv1x1_64(gy5, _t(p["w5"])))
        s4b = bn_backward_sums(gz4, y4, st[4])
        d4 = dw_backward(gz4, y4, st[4], p["g4"], s4b["mb"], s4b["mg"], p["train4"], x, p["w4"], 2,
                         reverse_taps="taps" in mutate, drop_mb="mb" in mutate)
        gx = d4["grad_a"].copy() if "overwrite" in mutate else (gx + d4["grad_a"]).astype(F)
        o.update(join5=j5, grad_y5=gy5, grad_z4=gz4, bn4=s4b, dw4=d4)
        o["grad_w5_64"] = np.einsum("nohw,nchw->oc", gy5.astype(np.float64), z4.astype(np.float64))
    o["grad_x"] = gx
    return o
