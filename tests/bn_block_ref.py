"""Numpy restatement of the fp32 training block BatchNorm2d -> ReLU -> Upsample(x2, nearest) as
codenet_amd/csrc/codenet_bn_train.hip computes it: float64 sums, every float32 operation rounded
on its own.  numpy rounds each elementwise float32 operation once and its float32 sqrt / divide are correctly rounded, so
on equal per-channel numbers the elementwise results are the kernels' bit for bit; only the ORDER of the float64 sums is
numpy's own (exact whenever the terms are small integers or binary fractions)."""
import numpy as np

F = np.float32
U32 = 2.0 ** -24          # unit round-off of float32
U64 = 2.0 ** -53


def _ch(v):
    return np.asarray(v, F).reshape(1, -1, 1, 1)


def batch_stats(y, eps):
    """y float32 [N,C,H,W] -> dict of the per-channel numbers of the statistics pass."""
    y = np.asarray(y, F)
    n = y.shape[0] * y.shape[2] * y.shape[3]
    y64 = y.astype(np.float64)
    s1 = y64.sum(axis=(0, 2, 3))
    s2 = (y64 * y64).sum(axis=(0, 2, 3))
    mean_d = s1 / float(n)
    var_d = np.maximum(s2 / float(n) - mean_d * mean_d, 0.0)
    mean, var = mean_d.astype(F), var_d.astype(F)
    return dict(n=n, s1=s1, s2=s2, mean_d=mean_d, var_d=var_d, mean=mean, var=var, invstd=invstd_of(var, eps),
                abs1=np.abs(y64).sum(axis=(0, 2, 3)))


def invstd_of(var, eps):
    var = np.asarray(var, F)
    return (F(1.0) / np.sqrt(var + F(eps))).astype(F)


def running_update(running_mean, running_var, st, momentum):
    """The running buffers after the call whose statistics are `st` (batch_stats)."""
    m, omm = F(momentum), F(1.0 - float(momentum))
    n = float(st["n"])
    var_u = (st["var_d"] * (n / (n - 1.0))).astype(F)
    rm = omm * np.asarray(running_mean, F) + m * st["mean"]
    rv = omm * np.asarray(running_var, F) + m * var_u
    return rm.astype(F), rv.astype(F)


def bn_z(y, mean, invstd, gamma, beta):
    """(z, xh): four float32 roundings."""
    y = np.asarray(y, F)
    d = y - _ch(mean)
    xh = d * _ch(invstd)
    s = _ch(gamma) * xh
    return (s + _ch(beta)).astype(F), xh.astype(F)


def up2(a):
    return np.repeat(np.repeat(a, 2, axis=2), 2, axis=3)


def forward(y, mean, invstd, gamma, beta, up):
    z, _ = bn_z(y, mean, invstd, gamma, beta)
    out = np.where(z < 0, F(0.0), z).astype(F)      # (a NaN stays)
    return up2(out) if up == 2 else out


def block_sum(g, up):
    """G at stored resolution: g itself (up 1) or ((g00 + g01) + g10) + g11 of every 2x2 block (up 2), in float32."""
    g = np.asarray(g, F)
    if up == 1:
        return g
    return ((g[:, :, 0::2, 0::2] + g[:, :, 0::2, 1::2]) + g[:, :, 1::2, 0::2]) + g[:, :, 1::2, 1::2]


def backward_gz(g, y, mean, invstd, gamma, beta, up):
    """(g_z, xh, T1, T2): the first pass; T1 = sum g_z, T2 = sum g_z * xh in float64."""
    z, xh = bn_z(y, mean, invstd, gamma, beta)
    gz = np.where(z > 0, block_sum(g, up), F(0.0)).astype(F)
    gz64, xh64 = gz.astype(np.float64), xh.astype(np.float64)
    return gz, xh, gz64.sum(axis=(0, 2, 3)), (gz64 * xh64).sum(axis=(0, 2, 3))


def backward_gy(gz, y, mean, invstd, gamma, mb, mg, training):
    """The second pass on given per-channel means mb, mg (float32)."""
    gz, y = np.asarray(gz, F), np.asarray(y, F)
    k = _ch(gamma) * _ch(invstd)
    if not training:
        return (gz * k).astype(F)
    d = y - _ch(mean)
    xh = d * _ch(invstd)
    t1 = gz - _ch(mb)
    t2 = xh * _ch(mg)
    t3 = t1 - t2
    return (t3 * k).astype(F)


def backward(g, y, mean, invstd, gamma, beta, up, training=True):
    """Everything the backward leaves, from the restatement's own sums."""
    gz, xh, t1, t2 = backward_gz(g, y, mean, invstd, gamma, beta, up)
    n = float(y.shape[0] * y.shape[2] * y.shape[3])
    mb, mg = (t1 / n).astype(F), (t2 / n).astype(F)
    return dict(g_z=gz, t1=t1, t2=t2, grad_beta=t1.astype(F), grad_gamma=t2.astype(F), mb=mb, mg=mg,
                grad_y=backward_gy(gz, y, mean, invstd, gamma, mb, mg, training),
                abs1=np.abs(gz.astype(np.float64)).sum(axis=(0, 2, 3)),
                abs2=np.abs(gz.astype(np.float64) * xh.astype(np.float64)).sum(axis=(0, 2, 3)))


def channel_bound(ref, n, abs_terms):
    """|got - ref| allowed for a per-channel number that is ONE float32 rounding of a float64 sum of n terms:
    2^-24 |ref| + n 2^-52 sum |terms|."""
    return U32 * np.abs(ref) + n * 2.0 ** -52 * abs_terms


# k of |z - z64| <= k 2^-24 S, S = |gamma| invstd (|y| + |mean|) + |beta| (one rounding of the mean,
# three in invstd, and the four operations of bn_z)
K_Z = 8.0
# k of |grad_y - grad_y64| <= k 2^-24 |gamma| invstd (G + B1 + A B2) (section 4.3e)
K_GY = 23.0
