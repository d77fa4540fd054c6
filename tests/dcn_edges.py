"""Shared inputs, references and yardsticks of the edge tests of the generic (modulated) deformable convolution
(codenet_amd/csrc/dcn_generic.hip): tests/test_dcn_edges_host.py (CPU) and tests/test_gpu_dcn_edges.py (GPU).  No tests here.

REFERENCES.  The float64 reference is the C oracle (oracle/dcn.py) on .double() copies of the float32 (or half-rounded)
inputs; the float32 yardstick is the same oracle in float32.  Beside it `restate` is a plain vectorised torch restatement
of the forward and the three backward roles, written from the formulas the kernels cite (the bilinear sample with
per-corner zeroing, _kernel.cu:83-114; the gradient and coordinate weights, :116-187; position and strict gate, :221-228).
It takes a `mutant=` switch (MUTANTS) -- the mistakes this kind of kernel makes -- with which the host test shows that
the inputs discriminate.  The oracle forms every contraction in double whatever the tensor type, where the kernels add
float32 chains (Cg * K taps per output, 256 private sums and a tree per weight, float atomics in arrival order per
grad_input cell): `restate` therefore adds in the kernels' orders, and its float32 evaluation is a second float32 yardstick
beside the oracle's (the larger figure counts, as R.bound takes a list).

OFFSETS.  Every offset is built from a target POSITION, off = target - base, and kept only if base + off == target holds in
float32 and in float64 (and after rounding off to half, for the half runs): no position of these tests is rounded, so
every tap lands in the same cell, on the same side of every gate, in the kernel's and in the reference's precision.  The
background targets are uniform on a grid of 2^-12 (2^-2 for half, whose offsets have 11 bits); a family's targets are
mixed in on about half of the (pixel, tap) entries, cycled along the diagonals so that every row, column and tap meets
every value; where a value does not survive at an entry's base (a float32 neighbour of -1 survives only next to it) the
next value of the family is tried.  `far` entries are not positions to land on: they only have to be gated out in both
precisions."""
import types

import numpy as np
import torch

from oracle import dcn as O
from tests import gather_ref as R

# grid_for (dcn_generic.hip): a launch is capped at kCUs * 16 workgroups of 256 threads; elements beyond take the
# grid-stride loop's second trip
GRID_CAP = 256 * 16 * 256
MARGIN = 4.0
U16 = 2.0 ** -11
F64_OVER_F32 = 2.0 ** -29          # ratio of the unit roundoffs 2^-53 / 2^-24

MUTANTS = ("gate", "corner", "left_derivative", "swap_hw", "dg_local")
FAMILIES = ("integers", "halves", "gates", "far")


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


class Geom:
    """One call geometry; members named as cdn::Geom."""

    def __init__(self, N, C, H, W, Co, k, s, p, d, G, DG, only=None):
        self.N, self.C, self.H, self.W, self.Co, self.G, self.DG = N, C, H, W, Co, G, DG
        (self.kH, self.kW), (self.sH, self.sW), (self.pH, self.pW), (self.dH, self.dW) = _pair(k), _pair(s), _pair(p), _pair(d)
        self.Ho, self.Wo = O.out_size(H, W, self.kH, self.kW, (self.sH, self.sW), (self.pH, self.pW), (self.dH, self.dW))
        self.K, self.P, self.Cg, self.Cog, self.cpdg = self.kH * self.kW, self.Ho * self.Wo, C // G, Co // G, C // DG
        self.only = only                                  # a dtype tag the row is restricted to

    @property
    def square(self):
        return self.kH == self.kW and self.sH == self.sW and self.pH == self.pW and self.dH == self.dW

    def cfg(self):
        """stride, padding, dilation, groups, deformable_groups of the oracle / of deform_conv."""
        return (self.sH, self.sW), (self.pH, self.pW), (self.dH, self.dW), self.G, self.DG

    def abi_plain(self):
        """cdn_deform_conv_*: (N, C, H, W, Co, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, dg) -- W first."""
        return (self.N, self.C, self.H, self.W, self.Co, self.kW, self.kH, self.sW, self.sH, self.pW, self.pH, self.dW,
                self.dH, self.G, self.DG)

    def abi_modulated(self):
        """cdn_modulated_deform_conv_*: (..., kernel_h, kernel_w, stride_h, stride_w, ...) -- H first."""
        return (self.N, self.C, self.H, self.W, self.Co, self.kH, self.kW, self.sH, self.sW, self.pH, self.pW, self.dH,
                self.dW, self.G, self.DG)

    def totals(self):
        """Threads of work of fwd_kernel, bwd_input_kernel, bwd_offset_kernel."""
        return {"fwd": self.N * self.Co * self.P, "bwd_input": self.N * self.C * self.K * self.P,
                "bwd_offset": self.N * self.DG * self.K * self.P}

    def tag(self):
        return "%dx%dx%dx%d_co%d_k%dx%d_s%d%d_p%d%d_d%d%d_g%d_dg%d" % (
            self.N, self.C, self.H, self.W, self.Co, self.kH, self.kW, self.sH, self.sW, self.pH, self.pW, self.dH, self.dW,
            self.G, self.DG)


# N, C, H, W, Co, k, stride, pad, dilation, G, DG: the smallest shapes that reach each decision of the generic kernels
GEOMS = [
    Geom(2, 4, 7, 9, 6, 3, 1, 1, 1, 1, 1),
    Geom(2, 4, 6, 5, 4, 1, 1, 0, 1, 2, 2),                        # K = 1
    Geom(1, 4, 6, 6, 8, (1, 3), (1, 2), (0, 1), (1, 2), 1, 1),
    Geom(1, 4, 9, 6, 8, (3, 1), (2, 1), (1, 0), (2, 1), 1, 1),    # the transpose of the row above
    Geom(2, 3, 8, 8, 3, 2, 3, 0, 1, 1, 1),                        # an even kernel, stride 3
    Geom(1, 2, 3, 3, 2, 3, 1, 0, 1, 1, 1),                        # one output pixel: N Ho Wo = 1
    Geom(2, 6, 7, 7, 6, 5, 1, 2, 1, 6, 6),                        # depthwise, but 5x5: the generic kernels
    Geom(2, 6, 5, 7, 2, 3, 1, 1, 1, 2, 3),                        # Cg = 3, cpdg = 2: deformable group 1 straddles both
                                                                  # convolution groups; Co / G = 1
    Geom(3, 16, 12, 12, 16, 3, 1, 1, 1, 16, 1, only="f64"),       # the fast-path geometry in the type without a fast path
]
STRADDLE, ROW13 = GEOMS[7], GEOMS[2]
STRIDE_CASE = Geom(2, 8, 176, 176, 24, 3, 1, 1, 1, 2, 2)
# the CoDeNet call geometry (groups = C = Co, 3x3, stride 1, pad 1), float32, unstructured 18-channel offsets
FAST_CASES = [(2, 37, 9, 11),       # a partial chunk, no quad kernel
              (1, 36, 16, 16),      # dwo4_kernel, dwo_wgrad_kernel
              (1, 4, 3, 3),
              (1, 6, 80, 72)]       # two-channel chunks, dwo_bwd_kernel<2, false>
STRUCTURED_CASES = [(2, 64, 16, 16), (2, 24, 32, 32), (1, 20, 64, 64)]
STRUCTURED_FAMILIES = ("integers_halves", "neighbours", "gates")


def fast_geom(N, C, H, W):
    return Geom(N, C, H, W, C, 3, 1, 1, 1, C, 1)


# ---- inputs ------------------------------------------------------------------------------------------------------------

def tap_bases(g, mutant=None):
    """Integer tap positions before the offset: base_h [K, Ho], base_w [K, Wo] (int64)."""
    kW, sH, sW, pH, pW, dH, dW = g.kW, g.sH, g.sW, g.pH, g.pW, g.dH, g.dW
    if mutant == "swap_hw":
        kW, sH, sW, pH, pW, dH, dW = g.kH, sW, sH, pW, pH, dW, dH
    k = torch.arange(g.K)
    i, j = k // kW, k % kW
    base_h = torch.arange(g.Ho).view(1, -1) * sH - pH + (i * dH).view(-1, 1)
    base_w = torch.arange(g.Wo).view(1, -1) * sW - pW + (j * dW).view(-1, 1)
    return base_h, base_w


def family_targets(name, size):
    """float32 target positions of a family on an axis of `size` cells."""
    f = np.float32
    if name == "integers":
        v = np.arange(0, size, dtype=f)
    elif name == "halves":
        v = np.arange(-0.5, size, 1.0, dtype=f)
    elif name == "gates":
        e = np.array([-1, 0, size - 1, size], dtype=f)
        v = np.concatenate([np.array([-1, size], dtype=f), np.nextafter(e, f(-np.inf)), np.nextafter(e, f(np.inf))])
    else:
        raise KeyError(name)
    return torch.from_numpy(v.astype(f))


FAR_OFFSETS = torch.tensor([1e4, -1e4, 3e9, -3e9, float("inf"), float("-inf"), float("nan")], dtype=torch.float32)


def _exact(base, off, target):
    """base + off == target in float32 and in float64."""
    return ((base + off) == target) & ((base.double() + off.double()) == target.double())


def make_offsets(g, family, seed, half=False, share=0.5):
    """-> off [N, DG * 2K, Ho, Wo] float32 (half-representable with half=True), info dict: 'family' [N, DG, K, Ho, Wo] bool,
    the (pixel, tap) entries that carry a surviving family value on at least one axis, 'placed', the entries it was tried
    on, and 'inexact', the number of finite positions that are rounded in float32 (asserted zero by the host test)."""
    gen = torch.Generator().manual_seed(seed)
    N, DG, K, Ho, Wo = g.N, g.DG, g.K, g.Ho, g.Wo
    shape = (N, DG, K, Ho, Wo)
    q = 4.0 if half else 4096.0
    base_h, base_w = tap_bases(g)
    bases = (base_h.float().view(1, 1, K, Ho, 1).expand(shape), base_w.float().view(1, 1, K, 1, Wo).expand(shape))
    nn_, dd, kk = torch.arange(N).view(N, 1, 1, 1, 1), torch.arange(DG).view(1, DG, 1, 1, 1), torch.arange(K).view(1, 1, K, 1, 1)
    hh, ww = torch.arange(Ho).view(1, 1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, 1, Wo)
    diag = ((hh + ww + kk + dd) % 2 == 0).expand(shape)
    use = ((torch.rand(shape, generator=gen) < share * 0.5) | (diag & (torch.rand(shape, generator=gen) < share))).clone()
    if use.numel() < 64:                                  # a handful of entries: most of them carry the family
        use = torch.rand(shape, generator=gen) < 0.8
    offs, fam_any, far_any = [], torch.zeros(shape, dtype=torch.bool), torch.zeros(shape, dtype=torch.bool)
    far_axis = torch.randint(0, 2, shape, generator=gen)
    for axis, (size, base) in enumerate(zip((g.H, g.W), bases)):
        target = torch.floor(torch.empty(shape).uniform_(-2.0, size + 1.0, generator=gen) * q) / q
        off = target - base
        assert bool(_exact(base, off, target).all())
        if family == "far" or family == "all":
            pick = (hh + 2 * ww + 3 * kk + 5 * nn_ + dd + axis).expand(shape) % len(FAR_OFFSETS)
            far = FAR_OFFSETS[pick]
            if half:
                far = far.half().float()
            pos32, pos64 = base + far, base.double() + far.double()
            out = ~((pos32 > -1) & (pos32 < size)) & ~((pos64 > -1) & (pos64 < size))
            sel = use & out & (far_axis == axis)
            if family == "all":
                sel = sel & ((hh + ww + kk) % 5 == 0)
            off = torch.where(sel, far, off)
            fam_any |= sel
            far_any |= sel
        if family != "far":
            names = ("integers", "halves", "gates") if family == "all" else (family,)
            vals = torch.cat([family_targets(n, size) for n in names])
            L = len(vals)
            pick = torch.randint(0, L, shape, generator=gen)
            pick = torch.where(diag, (hh + 2 * ww + 3 * kk + 5 * nn_ + dd).expand(shape) % L, pick)
            if family != "all":
                # both axes of an entry at the family's first / last value (-0.5 and size - 0.5: the taps with one live corner)
                both = (hh * Wo + ww + kk + nn_ + dd).expand(shape) % 7
                pick = torch.where(both == 0, torch.zeros_like(pick), torch.where(both == 1, torch.full_like(pick, L - 1), pick))
            todo = use & ~far_any & ~((hh + ww + kk) % 5 == 0) if family == "all" else use.clone()
            for step in range(L):
                t = vals[(pick + step) % L]
                o = t - base
                if half:
                    o = o.half().float()
                ok = todo & _exact(base, o, t)
                off = torch.where(ok, o, off)
                fam_any |= ok
                todo &= ~ok
        if half:
            assert torch.equal(off.half().float()[torch.isfinite(off)], off[torch.isfinite(off)])
        offs.append(off)
    # (far offsets, +-1e4 and beyond, are exempt: they only have to be gated out)
    inexact = sum(int(((o.abs() < 1e3) & ((b + o).double() != b.double() + o.double())).sum()) for b, o in zip(bases, offs))
    off = torch.stack(offs, 3).reshape(N, DG * 2 * K, Ho, Wo).contiguous()
    return off, {"family": fam_any, "placed": use, "inexact": inexact}


def make_inputs(g, family, seed=0, modulated=False, with_bias=False, half=False):
    """Seeded x, w, grad_out (randn), mask (uniform), bias, the family's offsets; all float32 (half-representable with
    half=True).  The random tensors do not depend on the family, the mask or the bias."""
    gen = torch.Generator().manual_seed(1000 + seed)
    rd = (lambda t: t.half().float()) if half else (lambda t: t)
    x = rd(torch.randn(g.N, g.C, g.H, g.W, generator=gen))
    w = rd(torch.randn(g.Co, g.Cg, g.kH, g.kW, generator=gen))
    gout = rd(torch.randn(g.N, g.Co, g.Ho, g.Wo, generator=gen))
    mask = rd(torch.rand(g.N, g.DG * g.K, g.Ho, g.Wo, generator=gen))
    bias = rd(torch.randn(g.Co, generator=gen))
    off, info = make_offsets(g, family, seed, half)
    return types.SimpleNamespace(g=g, x=x, off=off, w=w, gout=gout, mask=mask if modulated else None,
                                 bias=bias if (modulated and with_bias) else None, info=info, family=family, half=half)


def positions32(g, off):
    """float32 positions [N, DG, K, Ho, Wo] per axis, as every kernel forms them: float(base) + offset."""
    base_h, base_w = tap_bases(g)
    o = off.view(g.N, g.DG, g.K, 2, g.Ho, g.Wo)
    return base_h.float().view(1, 1, g.K, g.Ho, 1) + o[:, :, :, 0], base_w.float().view(1, 1, g.K, 1, g.Wo) + o[:, :, :, 1]


def edge_counts(g, off):
    """What the offsets hit, counted from the float32 geometry."""
    ph, pw = positions32(g, off)
    gate = (ph > -1) & (pw > -1) & (ph < g.H) & (pw < g.W)
    o = off.view(g.N, g.DG, g.K, 2, g.Ho, g.Wo)
    nonfin = ~torch.isfinite(o[:, :, :, 0]) | ~torch.isfinite(o[:, :, :, 1])
    return {
        "on_minus1": int((ph == -1).sum() + (pw == -1).sum()),
        "on_size": int((ph == g.H).sum() + (pw == g.W).sum()),
        "integer_rows": int((gate & (ph == torch.floor(ph))).sum()),
        "integer_cols": int((gate & (pw == torch.floor(pw))).sum()),
        "only_lower_right": int((gate & (ph < 0) & (pw < 0)).sum()),
        "only_upper_left": int((gate & (ph >= g.H - 1) & (pw >= g.W - 1)).sum()),
        "nonfinite_gated": int(nonfin.sum()),
        "gated": int((~gate).sum()),
    }


def gated_entries(g, off):
    """[N, DG, K, Ho, Wo] bool: the (pixel, tap) entries the strict gate removes (float32 positions; NaN compares false)."""
    ph, pw = positions32(g, off)
    return ~((ph > -1) & (pw > -1) & (ph < g.H) & (pw < g.W))


# ---- the restatement ---------------------------------------------------------------------------------------------------

def _block_sum(t, lanes=256):
    """Sum over the last axis as bwd_weight_kernel / bwd_bias_kernel do: thread q of 256 adds elements q, q + 256, ... in
    order, then the 256 private sums go through a halving tree.  (lanes: another power of two of private sums.)"""
    n = t.shape[-1]
    rows = -(-n // lanes)
    t = torch.cat([t, t.new_zeros(t.shape[:-1] + (rows * lanes - n,))], -1).view(t.shape[:-1] + (rows, lanes))
    acc = t[..., 0, :].clone()
    for r in range(1, rows):
        acc = acc + t[..., r, :]
    s = lanes // 2
    while s > 0:
        acc = acc[..., :s] + acc[..., s:2 * s]
        s >>= 1
    return acc[..., 0]


def restate(x, off, w, g, mask=None, bias=None, gout=None, mutant=None, order_seed=None, absolute=False, counts=False,
            pos_dtype=None, lanes=256):
    """The operator in the dtype of its arguments (float32 or float64; positions in that dtype too).  -> dict with 'out'
    and, with gout, 'grad_input', 'grad_offset', 'grad_mask' (with mask), 'grad_weight' (the un-scaled sum) and
    'grad_bias'.  Sums are formed in the kernels' orders; the scatter into grad_input in natural order, or in the order of
    a seeded permutation (order_seed).  absolute: every difference of the coordinate weights becomes a sum -- on |inputs|
    the outputs are then the sums of the absolute terms.  counts: also 'n_input' [N, C, H, W], the number of non-zero
    corner contributions into each cell of grad_input.  pos_dtype: the type the positions are formed in (float32 for
    offsets whose positions ARE rounded in float32 -- the structured family's neighbours of integers: what is discrete
    then follows the float32 position, as in tests/gather_ref.py; the fraction is exact in that type)."""
    dt = x.dtype
    pdt = pos_dtype or dt
    N, C, H, W, Co, K, P, Cg, Cog, DG = g.N, g.C, g.H, g.W, g.Co, g.K, g.P, g.Cg, g.Cog, g.DG
    base_h, base_w = tap_bases(g, mutant)
    o = off.view(N, DG, K, 2, g.Ho, g.Wo)
    o = o.to(pdt)
    ph = (base_h.to(pdt).view(1, 1, K, g.Ho, 1) + o[:, :, :, 0]).reshape(N, DG, K, P)
    pw = (base_w.to(pdt).view(1, 1, K, 1, g.Wo) + o[:, :, :, 1]).reshape(N, DG, K, P)
    if mutant == "gate":
        gate = (ph >= -1) & (pw >= -1) & (ph <= H) & (pw <= W)
    else:
        gate = (ph > -1) & (pw > -1) & (ph < H) & (pw < W)
    zero = torch.zeros((), dtype=dt)
    ph, pw = torch.where(gate, ph, torch.zeros((), dtype=pdt)), torch.where(gate, pw, torch.zeros((), dtype=pdt))
    c_all = torch.arange(C)
    dg_of_c = (c_all % Cg) // g.cpdg if mutant == "dg_local" else c_all // g.cpdg
    dg_of_c = dg_of_c.clamp(max=DG - 1)

    def per_c(t):
        return t.index_select(1, dg_of_c)                                     # [N, C, K, P]

    xf = x.reshape(-1)
    plane = ((torch.arange(N).view(N, 1) * C + c_all.view(1, C)) * (H * W)).view(N, C, 1, 1)

    def cell(ph, pw):
        """Floor cell (int64) and fractions (exact in the positions' type) of a position."""
        hl, wl = torch.floor(ph), torch.floor(pw)
        lh, lw = (ph - hl).to(dt), (pw - wl).to(dt)
        return hl.long(), wl.long(), lh, lw

    def corners(hl, wl, lh, lw):
        """Per channel [N, C, K, P], for the four corners of a cell: (validity, flat address, bilinear weight, value)."""
        hl, wl, lh, lw, gt = per_c(hl), per_c(wl), per_c(lh), per_c(lw), per_c(gate)
        uh, uw = 1 - lh, 1 - lw
        top, lef = hl >= 0, wl >= 0
        bot, rig = ((hl + 1 < H - 1), (wl + 1 < W - 1)) if mutant == "corner" else ((hl + 1 <= H - 1), (wl + 1 <= W - 1))
        out = []
        for ok, dh_, dw_, wt in ((top & lef, 0, 0, uh * uw), (top & rig, 0, 1, uh * lw), (bot & lef, 1, 0, lh * uw),
                                 (bot & rig, 1, 1, lh * lw)):
            idx = plane + (hl + dh_) * W + (wl + dw_)                         # the address a kernel forms
            ok = ok & gt & (idx >= 0) & (idx < xf.numel())
            idx = idx.clamp(0, xf.numel() - 1)
            out.append((ok, idx, wt, torch.where(ok, xf[idx], zero)))
        return out, (uh, uw, lh, lw)

    hl, wl, lh, lw = cell(ph, pw)
    cs, (uh, uw, lhc, lwc) = corners(hl, wl, lh, lw)
    (_, _, w1, v1), (_, _, w2, v2), (_, _, w3, v3), (_, _, w4, v4) = cs
    val = ((w1 * v1 + w2 * v2) + w3 * v3) + w4 * v4                            # [N, C, K, P]; zero where gated
    m_c = per_c(mask.reshape(N, DG, K, P)) if mask is not None else None
    mval = val * m_c if mask is not None else val
    wv = w.reshape(Co, Cg, K)
    co_all = torch.arange(Co)
    res = {}
    acc = torch.zeros(N, Co, P, dtype=dt)
    for cl in range(Cg):
        cidx = (co_all // Cog) * Cg + cl
        for k in range(K):
            acc = acc + wv[:, cl, k].view(1, Co, 1) * mval[:, cidx, k, :]
    if bias is not None:
        acc = acc + bias.view(1, Co, 1)
    res["out"] = acc.view(N, Co, g.Ho, g.Wo)
    if gout is None:
        return res
    go = gout.reshape(N, Co, P)
    gcol = torch.zeros(N, C, K, P, dtype=dt)
    for m in range(Cog):
        coi = (c_all // Cg) * Cog + m
        gcol = gcol + wv[coi, c_all % Cg, :].view(1, C, K, 1) * go[:, coi, :].view(N, C, 1, P)
    gcm = gcol * m_c if mask is not None else gcol
    # grad_input: every corner's share scattered to the address the kernel forms
    idxs = torch.cat([c[1][c[0]] for c in cs])
    terms = torch.cat([(c[2] * gcm)[c[0]] for c in cs])
    if order_seed is not None:
        perm = torch.randperm(idxs.numel(), generator=torch.Generator().manual_seed(order_seed))
        idxs, terms = idxs[perm], terms[perm]
    res["grad_input"] = torch.zeros(xf.numel(), dtype=dt).index_add_(0, idxs, terms).view(N, C, H, W)
    if counts:
        nz = torch.cat([(c[2] != 0)[c[0]] for c in cs])
        res["n_input"] = torch.zeros(xf.numel(), dtype=torch.int64).index_add_(
            0, torch.cat([c[1][c[0]] for c in cs]), nz.long()).view(N, C, H, W)
    # grad_offset / grad_mask: the derivative of the sample on the floor cell (one-sided at an integer position)
    if mutant == "left_derivative":
        onh, onw = gate & (lh == 0), gate & (lw == 0)
        hl2, wl2 = torch.where(onh, hl - 1, hl), torch.where(onw, wl - 1, wl)
        one = torch.ones((), dtype=dt)
        ds, (uh, uw, lhc, lwc) = corners(hl2, wl2, torch.where(onh, one, lh), torch.where(onw, one, lw))
        d1, d2, d3, d4 = (c[3] for c in ds)
    else:
        d1, d2, d3, d4 = v1, v2, v3, v4
    sg = 1.0 if absolute else -1.0
    dh = uw * (d3 + sg * d1) + lwc * (d4 + sg * d2)
    dw = uh * (d2 + sg * d1) + lhc * (d4 + sg * d3)
    th, tw = dh * gcol, dw * gcol
    if mask is not None:
        th, tw = th * m_c, tw * m_c
    gh, gw_, gm = (torch.zeros(N, DG, K, P, dtype=dt) for _ in range(3))
    tm = gcol * val
    for c in range(C):
        d = int(dg_of_c[c])
        gh[:, d] = gh[:, d] + th[:, c]
        gw_[:, d] = gw_[:, d] + tw[:, c]
        gm[:, d] = gm[:, d] + tm[:, c]
    res["grad_offset"] = torch.stack([gh, gw_], 3).reshape(N, DG * 2 * K, g.Ho, g.Wo)
    if mask is not None:
        res["grad_mask"] = gm.reshape(N, DG * K, g.Ho, g.Wo)
    gwt = torch.zeros(Co, Cg, K, dtype=dt)
    for cl in range(Cg):
        cidx = (co_all // Cog) * Cg + cl
        for k in range(K):
            gwt[:, cl, k] = _block_sum((mval[:, cidx, k, :] * go).permute(1, 0, 2).reshape(Co, N * P), lanes)
    res["grad_weight"] = gwt.view(Co, Cg, g.kH, g.kW)
    res["grad_bias"] = _block_sum(go.permute(1, 0, 2).reshape(Co, N * P))
    return res


def restate_inputs(inp, dtype, **kw):
    cv = lambda t: None if t is None else t.to(dtype)      # noqa: E731
    return restate(cv(inp.x), cv(inp.off), cv(inp.w), inp.g, cv(inp.mask), cv(inp.bias), cv(inp.gout), **kw)


def oracle_outputs(inp, dtype):
    """The C oracle on `dtype` copies of the inputs: the same dict as restate (grad_weight for scale 1 on zeros)."""
    g = inp.g
    cv = lambda t: None if t is None else t.to(dtype)      # noqa: E731
    x, off, w, gout, mask, bias = (cv(t) for t in (inp.x, inp.off, inp.w, inp.gout, inp.mask, inp.bias))
    res = {"out": O.deform_conv_forward(x, off, w, *g.cfg(), mask=mask, bias=bias)}
    r = O.deform_conv_backward_input(x, off, w, gout, *g.cfg(), mask=mask)
    res["grad_input"], res["grad_offset"] = r[0], r[1]
    if mask is not None:
        res["grad_mask"] = r[2]
    res["grad_weight"], res["grad_bias"] = O.deform_conv_backward_params(x, off, tuple(w.shape), gout, *g.cfg(), mask=mask,
                                                                         with_bias=True)
    return res


def term_bound(inp, name):
    """(terms + 2) 2^-53 sum |terms| per element, for the float64 restatement against the float64 oracle: the sums of
    absolute terms are the restatement on |inputs| with sums in place of differences; `terms` counts the leaves of the
    longest sum of the output and the products along each."""
    g = inp.g
    ab = types.SimpleNamespace(**vars(inp))
    for k in ("x", "w", "gout", "mask", "bias"):
        if getattr(inp, k) is not None:
            setattr(ab, k, getattr(inp, k).abs())
    S = restate_inputs(ab, torch.float64, absolute=True, counts=True)
    n = {"out": 4 * g.Cg * g.K + 1, "grad_offset": 8 * g.cpdg * g.Cog, "grad_mask": 4 * g.cpdg * g.Cog,
         "grad_weight": 4 * g.N * g.P, "grad_bias": g.N * g.P}
    if name == "grad_input":
        # the oracle's corner weight is the reference's (h + 1) - pos, not pos - floor(pos): an absolute error of
        # 2^-53 (size + 2) per weight, which the sum of the terms does not see where the exact weight is tiny
        terms = S["n_input"].double() * g.Cog
        gmax = (ab.w.abs().max() * ab.gout.abs().max() * g.Cog).item()
        return 1.01 * 2.0 ** -53 * ((terms + 8) * S[name] + (S["n_input"].max().item() + 4 * g.K) * (max(g.H, g.W) + 2) * gmax)
    terms = float(n[name])
    return 1.01 * (terms + 8) * 2.0 ** -53 * S[name]


class References:
    """Everything a comparison needs for one set of inputs, computed once: ref64 (oracle, float64), the float32 yardsticks
    (oracle in float32; the restatement in float32 with the kernels' summation orders, grad_input in `orders` seeded
    scatter orders) and, for half, the contribution counts and absolute sums of grad_input."""

    def __init__(self, inp, orders=4):
        self.inp, self._alt64 = inp, None
        self.ref64 = oracle_outputs(inp, torch.float64)
        o32 = oracle_outputs(inp, torch.float32)
        chains = [restate_inputs(inp, torch.float32, order_seed=s) for s in range(orders)]
        self.ref32 = {k: [o32[k]] + ([c[k] for c in chains] if k == "grad_input" else [chains[0][k]]) for k in o32}

    def own_error(self, name):
        """The float64 reference's own error, for the comparisons of the float64 kernels: the oracle is itself a float64
        evaluation (its contractions are sequential double sums: N Ho Wo additions per weight), so a float64 kernel cannot
        be held to it more closely than two float64 evaluations of the reference agree -- the figure of the float64
        restatement (the same sums in another order) against it.  No kernel output enters."""
        if self._alt64 is None:
            self._alt64 = restate_inputs(self.inp, torch.float64)
        return R.rel_err(self._alt64[name], self.ref64[name])

    def half_input_allowance(self):
        """Per cell of grad_input: (n + 1) 2^-11 S -- n half-rounded atomic adds of float32 terms into the cell, S the sum
        of the absolute terms (bilinear weights are non-negative: the operator on |w|, |grad_out|, |mask|)."""
        inp = self.inp
        ab = types.SimpleNamespace(**vars(inp))
        for k in ("w", "gout", "mask"):
            if getattr(inp, k) is not None:
                setattr(ab, k, getattr(inp, k).abs())
        r = restate_inputs(ab, torch.float64, counts=True)
        return (r["n_input"].double() + 1) * U16 * r["grad_input"]


def yardstick(name, refs, scale=1.0):
    return scale * R.yardstick(refs.ref32[name], refs.ref64[name])


def bound(name, refs, scale=1.0, add=0.0):
    """The bound of one output: MARGIN x the float32 figure (x `scale`: 2^-29 for float64 kernels), at least 8 ulps of
    the tensor's maximum in the kernel's type, plus `add` (2^-11 for half outputs stored once)."""
    ref64 = refs.ref64[name]
    m = ref64.abs().max().item()
    if m == 0:
        return 0.0
    floor = 8.0 * float(np.spacing(np.float32(m))) / m * scale
    return max(MARGIN * yardstick(name, refs, scale), floor) + add


# ---- the fast paths of the CoDeNet geometry: which chunk a shape takes ----------------------------------------------------
# A second copy of the launchers' rules in dcn_generic.hip (dwo_bwd_chunk, dwo_wgrad_chunk, dwos_bwd_chunk / dwos_bwd_split),
# to be changed together with them: the chained yardsticks below need the chain lengths.
LDS_MAX = 160 * 1024 - 512


def dwo_bwd_input_chunk(H, W):
    """Channel chunk of dwo_bwd_kernel<., true> (at most 4 channels; 0: the plane is beyond it)."""
    cells = (H + 1) * (W + 1)
    return next((c for c in (4, 2) if cells * c * 12 + c * 36 + 256 <= LDS_MAX), 0)


def dwo_wgrad_lanes(N, C, H, W):
    """Private sums per weight of the _parameters call: threads / chunk of dwo_wgrad_kernel, or of dwo_bwd_kernel<., false>."""
    cells = (H + 2) * (W + 2)
    need = lambda c, waves: cells * c * 4 + c * 36 + waves * c * 36      # noqa: E731
    c = 16 if need(16, 16) <= LDS_MAX else 8 if need(8, 16) <= LDS_MAX else 0
    if c:
        if c == 16 and need(8, 8) * 2 <= LDS_MAX and -(-C // 16) * N < 2 * 256:
            c = 8
        return (512 if need(c, 8) * 2 <= LDS_MAX else 1024) // c
    cells = (H + 1) * (W + 1)
    for c in (32, 16, 8, 4, 2):
        lds = cells * c * 4 + c * 36 + 256
        if lds + c * 16 * 36 <= LDS_MAX:
            if c >= 16 and (cells * (c // 2) * 4 + (c // 2) * 36 + 256 + c * 8 * 36) * 2 <= LDS_MAX:
                c //= 2
            lds = cells * c * 4 + c * 36 + 256
            return (512 if lds * 2 <= LDS_MAX else 1024) // c
    return 256


def dwos_goff_chunk(N, C, H, W):
    """(chunk, chunks per workgroup) of the pass of dwos_bwd_kernel that forms grad_offset: MODE 0, or MODE 2 where MODE 0
    has no chunk of 8 (the split form)."""
    cells = (H + 1) * (W + 1)

    def pick(per, group_ok):
        for c in (16, 8, 4, 2):
            need = cells * c * per + 256
            if need <= LDS_MAX:
                part, G = 18 * H * W * 4, 1
                two = need * 2 <= LDS_MAX
                if group_ok and need + part <= LDS_MAX and (not two or (need + part) * 2 <= LDS_MAX):
                    for t in (4, 2):
                        if -(-(-(-C // c)) // t) * N >= 2 * 256:
                            G = t
                            break
                return c, G
        return 0, 1
    c0, G0 = pick(12, True)
    return (c0, G0) if c0 >= 8 else pick(4, True)


def chained_channel_sums(per_channel, chunk, group=1, orders=8, seed=0, natural=False):
    """per_channel [C][...] float32 terms of a sum over channels that ends in float atomics (or, natural=True, in a pass that
    adds the chunks' planes in order): channels of a chunk summed first, `group` chunks added in order, then the groups
    one after the other in `orders` seeded random orders -> list of float32 tensors."""
    C = per_channel.shape[0]
    nch = -(-C // chunk)
    parts = [per_channel[i * chunk:(i + 1) * chunk].sum(0) for i in range(nch)]
    groups = []
    for i in range(0, nch, group):
        acc = parts[i]
        for q in parts[i + 1:i + group]:
            acc = acc + q
        groups.append(acc)
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(1 if natural else orders):
        acc = torch.zeros_like(groups[0])
        for i in (range(len(groups)) if natural else torch.randperm(len(groups), generator=gen).tolist()):
            acc = acc + groups[i]
        out.append(acc)
    return out


def per_channel_grad_offset32(inp):
    """[C][N, 18, H, W]: each channel's share of grad_offset, from the float32 oracle on channel slices (groups = C makes the
    channels independent)."""
    g = inp.g
    out = []
    for c in range(g.C):
        r = O.deform_conv_backward_input(inp.x[:, c:c + 1], inp.off, inp.w[c:c + 1], inp.gout[:, c:c + 1], 1, 1, 1, 1, 1)
        out.append(r[1])
    return torch.stack(out)


# ---- structured offsets of the CoDeNet geometry -----------------------------------------------------------------------

ANCHOR = torch.tensor([-1, -1, -1, 0, -1, 1, 0, -1, 0, 0, 0, 1, 1, -1, 1, 0, 1, 1], dtype=torch.float32).view(1, 18, 1, 1)


def structured_t(name, N, H, W, seed, share=0.6):
    """t [N, 1, H, W] (offsets = ANCHOR * t): a uniform background on a 2^-12 grid in [-8, 7] with the family's values on
    `share` of the pixels and on the diagonals.  integers_halves: k and k + 0.5; neighbours: both float32 neighbours of
    every integer in [-8, 7]; gates: per pixel the t that puts a tap exactly on -1 or on `size` (h + 1 + t = H, h - 1 - t
    = -1, and the same along the row)."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.floor(torch.empty(N, 1, H, W).uniform_(-8, 7, generator=gen) * 4096) / 4096
    hh = torch.arange(H).view(1, 1, H, 1).expand(N, 1, H, W)
    ww = torch.arange(W).view(1, 1, 1, W).expand(N, 1, H, W)
    nn_ = torch.arange(N).view(N, 1, 1, 1)
    diag = (hh == ww) | (hh == ww + 1)
    use = (torch.rand(N, 1, H, W, generator=gen) < share) | diag
    if name == "gates":
        # h + 1 + t = H, h - 1 - t = -1, w + 1 + t = W, w - 1 - t = -1, and their mirror images through the other tap
        cands = torch.stack([(H - 1 - hh), hh, (W - 1 - ww), ww, -(hh + 2), -(H + 1 - hh), -(ww + 2), -(W + 1 - ww)]).float()
        pick = torch.randint(0, 8, (N, 1, H, W), generator=gen)
        pick = torch.where(diag, (hh + 3 * nn_) % 8, pick)
        v = cands.gather(0, pick.unsqueeze(0))[0]
    else:
        ints = np.arange(-8, 8, dtype=np.float32)
        if name == "integers_halves":
            vals = np.concatenate([ints, ints[:-1] + np.float32(0.5)])
        elif name == "neighbours":
            vals = np.concatenate([np.nextafter(ints, np.float32(-np.inf)), np.nextafter(ints, np.float32(np.inf))])
        else:
            raise KeyError(name)
        vals = torch.from_numpy(vals.astype(np.float32))
        pick = torch.randint(0, len(vals), (N, 1, H, W), generator=gen)
        pick = torch.where(diag, (hh + 5 * nn_) % len(vals), pick)
        v = vals[pick]
    return torch.where(use, v, t).contiguous()
