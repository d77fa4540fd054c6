"""Numpy restatement of the fp32 detection heads in training as codenet_amd/csrc/codenet_heads_fp32_train.hip computes them
(DESIGN.md section 4.3f), on top of tests/bn_block_ref.py: every float32 operation rounded on its own, every sum in float64.
Unlike bn_block_ref, the float64 sums here follow the kernels' OWN order -- the (channel, slab) protocol of cdn_bn.h
(`slab_sums`) and the (plane, chunk) protocol of the depthwise backward (`plane_sums`) -- so on equal inputs every number
is the kernels' bit for bit, whatever the inputs are.  The dense 1x1 convolutions run on MFMA kernels whose order is not
restated: `conv1x1_64` gives their float64 value, exact whenever the terms are."""
import numpy as np

from tests import bn_block_ref as R

F = np.float32
SLAB, THREADS, ROWS = 4096, 256, 8


def _tree(v):
    """v [..., waves, 64] float64 -> [...]: the xor shuffle tree (32, 16, .. 1), then the waves in wave order."""
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ m]
    w = v[..., 0]
    s = w[..., 0]
    for i in range(1, w.shape[-1]):
        s = s + w[..., i]
    return s


def slab_sums(terms):
    """terms float64 [N,C,H,W] -> [C]: the (channel, slab) protocol.  Value j = image * H * W + pixel; slabs of 4096;
    thread t adds the quads t, t + 256, t + 512, t + 768 of the slab in that order from zero; lanes by the xor tree, waves
    in order, slabs in order.  (Padding with +0.0 stands for the terms a thread skips: s + 0.0 == s.)"""
    Nb, C, H, W = terms.shape
    n = Nb * H * W
    slabs = -(-n // SLAB)
    v = np.zeros((C, slabs * SLAB))
    v[:, :n] = terms.transpose(1, 0, 2, 3).reshape(C, n)
    v = v.reshape(C, slabs, 4, THREADS, 4)
    s = np.zeros((C, slabs, THREADS))
    for it in range(4):
        for e in range(4):
            s = s + v[:, :, it, :, e]
    part = _tree(s.reshape(C, slabs, THREADS // 64, 64))
    out = np.zeros(C)
    for sl in range(slabs):
        out = out + part[:, sl]
    return out


def plan(H, W):
    """(wq, strips, threads, chunks) of the strip kernels: a thread owns 8 rows x 4 columns of one plane."""
    wq, strips = -(-W // 4), -(-H // ROWS)
    items = wq * strips
    threads = min(256, -(-items // 64) * 64)
    return wq, strips, threads, -(-items // threads)


def plane_sums(terms):
    """terms float64 [N,C,H,W] -> [C]: the protocol of head32_dw_bwd_kernel.  A thread adds the pixels of its strip in
    row-major order from zero; items (strip * wq + quad) in chunks of `threads`; lanes by the xor tree, waves in order; the
    partials [N][C][chunks] in index order (images, then chunks)."""
    Nb, C, H, W = terms.shape
    wq, strips, threads, chunks = plan(H, W)
    v = np.zeros((Nb, C, strips * ROWS, wq * 4))
    v[:, :, :H, :W] = terms
    v = v.reshape(Nb, C, strips, ROWS, wq, 4)
    s = np.zeros((Nb, C, strips, wq))
    for r in range(ROWS):
        for i in range(4):
            s = s + v[:, :, :, r, :, i]
    items = np.zeros((Nb, C, chunks * threads))
    items[:, :, :strips * wq] = s.reshape(Nb, C, strips * wq)
    part = _tree(items.reshape(Nb, C, chunks, threads // 64, 64))
    out = np.zeros(C)
    for img in range(Nb):
        for h in range(chunks):
            out = out + part[img, :, h]
    return out


def batch_stats(y, eps):
    """R.batch_stats with S1, S2 in the kernels' order: mean, var, invstd are the kernels' bit for bit."""
    y = np.asarray(y, F)
    n = y.shape[0] * y.shape[2] * y.shape[3]
    y64 = y.astype(np.float64)
    s1, s2 = slab_sums(y64), slab_sums(y64 * y64)
    mean_d = s1 / float(n)
    var_d = np.maximum(s2 / float(n) - mean_d * mean_d, 0.0)
    mean, var = mean_d.astype(F), var_d.astype(F)
    return dict(n=n, s1=s1, s2=s2, mean_d=mean_d, var_d=var_d, mean=mean, var=var, invstd=R.invstd_of(var, eps))


def eval_stats(running_mean, running_var, eps):
    rm, rv = np.asarray(running_mean, F), np.asarray(running_var, F)
    return dict(mean=rm, var=rv, invstd=R.invstd_of(rv, eps))


def _pad(a):
    return np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)))


def dw_forward(y1, st1, gamma1, beta1, w2, pad_value=None):
    """y2 = ((0 + w[0] a[0]) + w[1] a[1]) + .. + w[8] a[8], a = relu(bn_z(y1)) inside the plane and 0.0f outside.
    pad_value (the mutation "padded tap not zero"): relu(bn_z(pad_value)) outside instead."""
    a1 = R.forward(y1, st1["mean"], st1["invstd"], gamma1, beta1, 1)
    ap = _pad(a1)
    if pad_value is not None:
        edge = R.forward(np.full((1, a1.shape[1], 1, 1), pad_value, F), st1["mean"], st1["invstd"], gamma1, beta1, 1)
        ap = np.broadcast_to(edge, ap.shape).copy()
        ap[:, :, 1:-1, 1:-1] = a1
    H, W = a1.shape[2:]
    w = np.asarray(w2, F).reshape(1, -1, 3, 3)
    acc = np.zeros_like(a1)
    for dy in range(3):
        for dx in range(3):
            pr = w[:, :, dy, dx].reshape(1, -1, 1, 1) * ap[:, :, dy:dy + H, dx:dx + W]
            acc = acc + pr
    return acc.astype(F)


def tail_forward(y2, st2, gamma2, beta2, w3, b3):
    """y3[o] = (sum_c W3[o][c] a2[c]) + b3[o], c ascending from zero, a2 = relu(bn_z(y2)); Co <= 4."""
    a2 = R.forward(y2, st2["mean"], st2["invstd"], gamma2, beta2, 1)
    w = np.asarray(w3, F).reshape(len(w3), -1)
    Nb, C, H, W = a2.shape
    acc = np.zeros((Nb, w.shape[0], H, W), F)
    for c in range(C):
        pr = w[:, c].reshape(1, -1, 1, 1) * a2[:, c:c + 1]
        acc = acc + pr
    return (acc + np.asarray(b3, F).reshape(1, -1, 1, 1)).astype(F)


def _finish(t1, t2, n):
    return dict(t1=t1, t2=t2, grad_beta=t1.astype(F), grad_gamma=t2.astype(F), mb=(t1 / float(n)).astype(F),
                mg=(t2 / float(n)).astype(F))


def bn_backward1(ga, y, st, gamma, beta):
    """The first BatchNorm backward pass on a stored grad_a (bn_bwd1_kernel, up = 1) with its sums in slab order."""
    gz, xh, _, _ = R.backward_gz(ga, y, st["mean"], st["invstd"], gamma, beta, 1)
    gz64 = gz.astype(np.float64)
    n = y.shape[0] * y.shape[2] * y.shape[3]
    return dict(g_z=gz, **_finish(slab_sums(gz64), slab_sums(gz64 * xh.astype(np.float64)), n))


def tail_backward(gy3, y2, st2, gamma2, beta2, w3, drop_gb3=False):
    """The narrow tail's backward and the first BatchNorm2 pass: grad_a2 = W3[0][c] g[0] (+ W3[o][c] g[o], o ascending),
    g_z2 = z2 > 0 ? grad_a2 : 0; T1, T2, grad_W3[o][c] = sum g[o] a2, grad_b3[o] = sum g[o] in float64, slab order."""
    g = np.asarray(gy3, F)
    w = np.asarray(w3, F).reshape(len(w3), -1)
    z, xh = R.bn_z(y2, st2["mean"], st2["invstd"], gamma2, beta2)
    a2 = np.where(z < 0, F(0.0), z).astype(F)
    ga = w[0].reshape(1, -1, 1, 1) * g[:, 0:1]
    for o in range(1, w.shape[0]):
        pr = w[o].reshape(1, -1, 1, 1) * g[:, o:o + 1]
        ga = ga + pr
    gz = np.where(z > 0, ga, F(0.0)).astype(F)
    gz64, a64, g64 = gz.astype(np.float64), a2.astype(np.float64), g.astype(np.float64)
    n = g.shape[0] * g.shape[2] * g.shape[3]
    out = dict(g_z=gz, **_finish(slab_sums(gz64), slab_sums(gz64 * xh.astype(np.float64)), n))
    out["grad_w3"] = np.stack([slab_sums(g64[:, o:o + 1] * a64) for o in range(w.shape[0])]).astype(F)
    # (every channel's workgroups form sum g[o]; channel 0's is stored)
    out["grad_b3"] = (np.zeros(w.shape[0], F) if drop_gb3 else
                      np.stack([slab_sums(g64[:, o:o + 1])[0] for o in range(w.shape[0])]).astype(F))
    return out


def dw_backward(gz2, y2, st2, gamma2, mb2, mg2, training2, y1, st1, gamma1, beta1, w2, reverse_taps=False, drop_mb2=False):
    """grad_y2 formed on load (0 outside the plane), grad_a1[q] = sum_t W2[c][t] grad_y2[q - t] from zero in the loop order
    of head_dw_bwd_kernel, g_z1 = z1 > 0 ? grad_a1 : 0, grad_W2[c][t] = sum_p grad_y2[p] a1[p + t], T1 = sum g_z1, T2 =
    sum g_z1 xh1, the sums in (plane, chunk) order.  reverse_taps / drop_mb2: the mutations of the same names."""
    if drop_mb2 and training2:
        mb2 = np.zeros_like(np.asarray(mb2, F))
    gy2 = R.backward_gy(gz2, y2, st2["mean"], st2["invstd"], gamma2, mb2, mg2, training2)
    z1, xh1 = R.bn_z(y1, st1["mean"], st1["invstd"], gamma1, beta1)
    a1 = np.where(z1 < 0, F(0.0), z1).astype(F)
    H, W = a1.shape[2:]
    gp, ap = _pad(gy2), _pad(a1)
    w = np.asarray(w2, F).reshape(1, -1, 3, 3)
    ga = np.zeros_like(a1)
    for dy in range(3):
        for dx in range(3):
            ry, rx = (dy, dx) if reverse_taps else (2 - dy, 2 - dx)
            pr = w[:, :, dy, dx].reshape(1, -1, 1, 1) * gp[:, :, ry:ry + H, rx:rx + W]
            ga = ga + pr
    gz1 = np.where(z1 > 0, ga, F(0.0)).astype(F)
    g64, gz64 = gy2.astype(np.float64), gz1.astype(np.float64)
    gw2 = np.stack([plane_sums(g64 * ap[:, :, dy:dy + H, dx:dx + W].astype(np.float64))
                    for dy in range(3) for dx in range(3)], axis=1).astype(F)
    n = y1.shape[0] * H * W
    return dict(g_z=gz1, grad_y2=gy2, grad_w2=gw2.reshape(np.asarray(w2).shape),
                **_finish(plane_sums(gz64), plane_sums(gz64 * xh1.astype(np.float64)), n))


def conv1x1_64(d, w, b=None):
    """conv1x1 in float64: d [N,C,H,W], w [Co,C(,1,1)]."""
    w = np.asarray(w, np.float64).reshape(len(w), -1)
    y = np.einsum("oc,nchw->nohw", w, np.asarray(d, np.float64))
    return y if b is None else y + np.asarray(b, np.float64).reshape(1, -1, 1, 1)


def head(x, p, gy3, y1=None, mutate=()):
    """One head, forward and backward.  p: dict of float32 arrays w1 [C,Cin], g1, b1, w2 [C,9], g2, b2, w3 [Co,C], b3, the
    running buffers rm1, rv1, rm2, rv2, eps, momentum and the flags train1, train2.  y1 None: y1 = f32(conv1x1 in float64)
    (exact inputs); else the given y1 (the GPU's own).  For Co > 4, y3, grad_a2 and grad_W3 / grad_b3 are the float64
    values rounded once (exact inputs; their MFMA order is not restated).  mutate: names of deliberately wrong variants."""
    out = {}
    y1 = conv1x1_64(x, p["w1"]).astype(F) if y1 is None else np.asarray(y1, F)
    st = {}
    for k, y in ((1, y1),):
        st[k] = batch_stats(y, p["eps"]) if p["train%d" % k] else eval_stats(p["rm%d" % k], p["rv%d" % k], p["eps"])
    y2 = dw_forward(y1, st[1], p["g1"], p["b1"], p["w2"], pad_value=0.0 if "pad" in mutate else None)
    st[2] = batch_stats(y2, p["eps"]) if p["train2"] else eval_stats(p["rm2"], p["rv2"], p["eps"])
    for k in (1, 2):
        if p["train%d" % k]:
            out["rm%d" % k], out["rv%d" % k] = R.running_update(p["rm%d" % k], p["rv%d" % k], st[k], p["momentum"])
        else:
            out["rm%d" % k], out["rv%d" % k] = np.asarray(p["rm%d" % k], F), np.asarray(p["rv%d" % k], F)
    Co = len(p["w3"])
    if Co <= 4:
        y3 = tail_forward(y2, st[2], p["g2"], p["b2"], p["w3"], p["b3"])
        tb = tail_backward(gy3, y2, st[2], p["g2"], p["b2"], p["w3"], drop_gb3="gb3" in mutate)
    else:
        a2 = R.forward(y2, st[2]["mean"], st[2]["invstd"], p["g2"], p["b2"], 1)
        y3 = conv1x1_64(a2, p["w3"], p["b3"]).astype(F)
        ga2 = conv1x1_64(gy3, np.asarray(p["w3"]).reshape(Co, -1).T).astype(F)
        tb = bn_backward1(ga2, y2, st[2], p["g2"], p["b2"])
        g64 = np.asarray(gy3, np.float64)
        tb["grad_w3_64"] = np.einsum("nohw,nchw->oc", g64, a2.astype(np.float64))
        tb["grad_w3_abs"] = np.einsum("nohw,nchw->oc", np.abs(g64), np.abs(a2.astype(np.float64)))
        tb["grad_b3"] = g64.sum(axis=(0, 2, 3)).astype(F)
    db = dw_backward(tb["g_z"], y2, st[2], p["g2"], tb["mb"], tb["mg"], p["train2"], y1, st[1], p["g1"], p["b1"], p["w2"],
                     reverse_taps="taps" in mutate, drop_mb2="mb2" in mutate)
    gy1 = R.backward_gy(db["g_z"], y1, st[1]["mean"], st[1]["invstd"], p["g1"], db["mb"], db["mg"], p["train1"])
    out.update(y1=y1, y2=y2, y3=y3, st1=st[1], st2=st[2], tail=tb, dw=db, grad_y1=gy1)
    return out
