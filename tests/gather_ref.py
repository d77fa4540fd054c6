"""A plain reference of the scale-dilated gather (depthwise 3x3 deformable convolution whose nine taps are dilated by
one scalar s per pixel) and of its backward, in PyTorch on the CPU.

    d[n,c,h,w] = sum_{i,j} w[c,i,j] * V(x[n,c]; pos_y, pos_x),   pos_y = (h - 1 + i) + (i - 1) (s - 1),  pos_x likewise

What is DISCRETE is decided from float32 positions, because that is the rule the kernels (and the reference
implementation the project was modelled on) follow: t = s - 1 and pos = float32(h - 1 + i) + (i - 1) * t are float32
operations, a tap takes part only if -1 < pos_y < H and -1 < pos_x < W, and the bilinear cell is floor(pos).  What is
CONTINUOUS -- the bilinear weights from the (exact) fraction pos - floor(pos), every product and every sum -- is done in
`dtype`: float64 for the reference proper, float32 for the yardstick that says how far a float32 evaluation of the same
formulas lies from it.  Corners outside the image read zero.  At a position on a grid line the derivative with respect to
the position is the one-sided one on the floor cell [floor(pos), floor(pos) + 1].

positions64=True takes t and the positions in float64 instead: a "continuous" evaluation that rounds no position.  It
exists only to prove that a test's inputs discriminate (its grad_s differs wherever the float32 rounding of a position
moves a floor cell or a gate)."""
import numpy as np
import torch


def tap_positions(s, size, axis, positions64=False):
    """Positions [3][N,1,H,W] of the taps i = 0, 1, 2 along `axis` (2: rows, 3: columns) for the scale plane s
    [N,1,H,W]: float32 arithmetic (float64 with positions64)."""
    pdt = torch.float64 if positions64 else torch.float32
    t = s.to(pdt) - 1
    n = s.shape[axis]
    assert n == size
    shape = [1, 1, 1, 1]
    shape[axis] = n
    out = []
    for i in range(3):
        base = (torch.arange(n, dtype=torch.int64) - 1 + i).to(pdt).view(shape)
        out.append(base + (i - 1) * t)
    return out


def gather_ref(x, s, w, grad_d=None, dtype=torch.float64, positions64=False, terms=None):
    """x [N,C,H,W], s [N,1,H,W], w [C,1,3,3], grad_d [N,C,H,W] or None -> d, grad_x, grad_s, grad_w (the gradients None
    without grad_d), all in `dtype`.  terms (a dict): also receives the summands of the two reductions, before they are
    summed -- "grad_s" [N,C,H,W], each channel's share of grad_s, and "grad_w" [9][N,C,H,W], grad_d x the tap's value."""
    N, C, H, W = x.shape
    assert s.shape == (N, 1, H, W) and w.shape == (C, 1, 3, 3)
    xd, wd = x.to(dtype), w.to(dtype).view(C, 3, 3)
    gd = grad_d.to(dtype) if grad_d is not None else None
    # x with a border of zeros: cell (y, x) of the image is cell (y + 1, x + 1) here, rows / columns -1 and size are zero
    Hp, Wp = H + 2, W + 2
    xp = torch.zeros(N, C, Hp, Wp, dtype=dtype)
    xp[:, :, 1:-1, 1:-1] = xd
    xp = xp.view(N, C, Hp * Wp)
    pys = tap_positions(s, H, 2, positions64)
    pxs = tap_positions(s, W, 3, positions64)

    def axis_terms(pos, size):
        inside = (pos > -1) & (pos < size)
        fl = torch.floor(pos)
        frac = (pos - fl).to(dtype)                      # exact in the positions' own format
        cell = fl.to(torch.int64).clamp(-1, size - 1)    # (a gated-out tap reads somewhere harmless; it is masked below)
        return inside, cell, 1 - frac, frac

    d = torch.zeros(N, C, H, W, dtype=dtype)
    grad_x = grad_s = grad_w = None
    if gd is not None:
        gxp = torch.zeros(N, C, Hp * Wp, dtype=dtype)
        grad_s = torch.zeros(N, 1, H, W, dtype=dtype)
        grad_w = torch.zeros(C, 3, 3, dtype=dtype)
    for i in range(3):
        in_y, cy, hy, ly = axis_terms(pys[i].expand(N, 1, H, W), H)
        for j in range(3):
            in_x, cx, hx, lx = axis_terms(pxs[j].expand(N, 1, H, W), W)
            on = (in_y & in_x).to(dtype)
            i00 = ((cy + 1) * Wp + cx + 1).view(N, 1, H * W).expand(N, C, H * W)
            idx = (i00, i00 + 1, i00 + Wp, i00 + Wp + 1)
            v00, v01, v10, v11 = (xp.gather(2, k).view(N, C, H, W) for k in idx)
            wts = (hy * hx * on, hy * lx * on, ly * hx * on, ly * lx * on)
            val = wts[0] * v00 + wts[1] * v01 + wts[2] * v10 + wts[3] * v11
            wk = wd[:, i, j].view(1, C, 1, 1)
            d += wk * val
            if gd is None:
                continue
            gk = gd * wk
            for k, wt in zip(idx, wts):
                gxp.scatter_add_(2, k, (wt * gk).reshape(N, C, H * W))
            dv_dy = hx * (v10 - v00) + lx * (v11 - v01)
            dv_dx = hy * (v01 - v00) + ly * (v11 - v10)
            share = on * gk * ((i - 1) * dv_dy + (j - 1) * dv_dx)
            grad_s += share.sum(1, keepdim=True)
            grad_w[:, i, j] = (gd * val).sum((0, 2, 3))
            if terms is not None:
                terms["grad_s"] = terms["grad_s"] + share if "grad_s" in terms else share
                terms.setdefault("grad_w", []).append(gd * val)
    if gd is not None:
        grad_x = gxp.view(N, C, Hp, Wp)[:, :, 1:-1, 1:-1].contiguous()
        grad_w = grad_w.view(C, 1, 3, 3)
    return d, grad_x, grad_s, grad_w


def contribution_counts(s):
    """[N,1,H,W] int64: how many (pixel, tap, corner) terms with a non-zero bilinear weight the backward adds into each
    cell of grad_x (the same for every channel) -- the number of roundings of a fixed-point accumulation of that cell."""
    N, _, H, W = s.shape
    Hp, Wp = H + 2, W + 2
    cnt = torch.zeros(N, 1, Hp * Wp, dtype=torch.int64)
    pys, pxs = tap_positions(s, H, 2), tap_positions(s, W, 3)
    for i in range(3):
        py = pys[i].expand(N, 1, H, W)
        fy = torch.floor(py)
        for j in range(3):
            px = pxs[j].expand(N, 1, H, W)
            fx = torch.floor(px)
            on = (py > -1) & (py < H) & (px > -1) & (px < W)
            i00 = ((fy.to(torch.int64).clamp(-1, H - 1) + 1) * Wp + fx.to(torch.int64).clamp(-1, W - 1) + 1).view(N, 1, -1)
            ly, lx = py - fy, px - fx
            for k, nz in ((i00, (ly < 1) & (lx < 1)), (i00 + 1, (ly < 1) & (lx > 0)), (i00 + Wp, (ly > 0) & (lx < 1)),
                          (i00 + Wp + 1, (ly > 0) & (lx > 0))):
                cnt.scatter_add_(2, k, (on & nz).to(torch.int64).view(N, 1, -1))
    return cnt.view(N, 1, Hp, Wp)[:, :, 1:-1, 1:-1].contiguous()


def replicate2(t):
    """Nearest x2 up-sampling [N,C,H,W] -> [N,C,2H,2W]."""
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3).contiguous()


def fold2(t):
    """Backward of replicate2: the sums over the 2x2 blocks."""
    N, C, H, W = t.shape
    return t.view(N, C, H // 2, 2, W // 2, 2).sum((3, 5))


def gather_up2_ref(x_stored, s_stored, w, grad_d=None, dtype=torch.float64, positions64=False):
    """The gather on the nearest x2 replication of the stored x [N,C,H/2,W/2] and s [N,1,H/2,W/2]: d at H x W, the
    gradients with respect to the STORED tensors (the 2x2 sums of the up-sampling backward)."""
    d, gx, gs, gw = gather_ref(replicate2(x_stored), replicate2(s_stored), w, grad_d, dtype, positions64)
    if grad_d is None:
        return d, None, None, None
    return d, fold2(gx), fold2(gs), gw


def chained_float32_sums(x, s, w, grad_d, up2, chunk, lanes, orders=8, seed=0):
    """The float32 yardstick for the ATOMIC forms' grad_s and grad_w.  Those two outputs end in float atomics: a chain of
    float32 additions, one per channel chunk (grad_s of a pixel) or per lane of the workgroup and then per image (grad_w
    of a weight), in the order in which the atomics arrive -- where torch.sum of the plain float32 reference adds
    pairwise.  This evaluates the float32 reference's own summands (gather_ref(..., terms=)) with chains of the same
    lengths: channels of a chunk summed first, then the chunks one after the other; the pixels (2x2 blocks for the
    up-sampled form) dealt out to `lanes` private sums (lanes > 0: lane l owns pixels l, l + lanes, ...; lanes < 0: a
    private sum is the tree sum of -lanes consecutive pixels), then the private sums one after the other, then the
    images.  The arrival order is not defined, so `orders` seeded random orders are evaluated: a list of
    (grad_s, grad_w) float32 pairs, whose largest error is the yardstick (bound)."""
    terms = {}
    if up2:
        gather_ref(replicate2(x), replicate2(s), w, grad_d, torch.float32, terms=terms)
        share, prods = fold2(terms["grad_s"]), [fold2(p) for p in terms["grad_w"]]
    else:
        gather_ref(x, s, w, grad_d, torch.float32, terms=terms)
        share, prods = terms["grad_s"], terms["grad_w"]
    N, C, H, W = share.shape
    nch = -(-C // chunk)
    pad = torch.zeros(N, nch * chunk - C, H, W)
    parts = torch.cat([share, pad], 1).view(N, nch, chunk, H, W).sum(2)                   # [N, chunks, H, W]
    P = H * W
    if lanes > 0:
        L = min(lanes, P)
        K = -(-P // L)
        private = []
        for p in prods:
            q = torch.cat([p.reshape(N, C, P), torch.zeros(N, C, K * L - P)], 2).view(N, C, K, L)
            acc = q[:, :, 0].clone()
            for k in range(1, K):
                acc = acc + q[:, :, k]
            private.append(acc)                                                           # [N, C, L]
    else:
        G = -lanes
        L = -(-P // G)
        private = [torch.cat([p.reshape(N, C, P), torch.zeros(N, C, L * G - P)], 2).view(N, C, L, G).sum(3) for p in prods]
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(orders):
        gs = torch.zeros(N, H, W)
        for k in torch.randperm(nch, generator=g).tolist():
            gs = gs + parts[:, k]
        gw = torch.zeros(9, C)
        perm_l, perm_n = torch.randperm(L, generator=g).tolist(), torch.randperm(N, generator=g).tolist()
        for tap, pr in enumerate(private):
            acc = torch.zeros(N, C)
            for l in perm_l:
                acc = acc + pr[:, :, l]
            tot = torch.zeros(C)
            for n in perm_n:
                tot = tot + acc[n]
            gw[tap] = tot
        out.append((gs.view(N, 1, H, W), gw.t().reshape(C, 1, 3, 3).contiguous()))
    return out


# ---- what the inputs of a test hit (counted on the CPU from the float32 geometry) ------------------------------------

def edge_counts(s):
    """For a full-resolution scale plane s [N,1,H,W]: how many taps sit exactly on -1 / on `size` (per axis occurrences,
    off-centre taps), and how many pixels have every off-centre tap gated out."""
    N, _, H, W = s.shape
    on_minus1 = on_size = 0
    per_axis = []
    for size, axis in ((H, 2), (W, 3)):
        pos = tap_positions(s, size, axis)
        oks = []
        for i in (0, 2):
            p = pos[i].expand(N, 1, H, W)
            on_minus1 += int((p == -1).sum())
            on_size += int((p == size).sum())
            oks.append((p > -1) & (p < size))
        per_axis.append(oks)
    # an off-centre tap (i, j) lives if its off-centre axes are in range
    (ya, yb), (xa, xb) = per_axis
    alive = ya | yb | xa | xb
    return {"on_minus1": on_minus1, "on_size": on_size, "centre_only": int((~alive).sum())}


def unfoldable_pairs(s_stored):
    """For a stored scale plane [N,1,Hs,Ws] of the up-sampled form: boolean maps [N,1,Hs,Ws] per axis name ('ya', 'yb',
    'xa', 'xb') of the 2x2 blocks whose two pixels along that axis are both in range with floor cells that differ by 2,
    the first one odd -- the pair whose corners do not fall onto two consecutive stored cells."""
    N, _, Hs, Ws = s_stored.shape
    s = replicate2(s_stored)
    out = {}
    for size, axis, names in ((2 * Hs, 2, ("ya", "yb")), (2 * Ws, 3, ("xa", "xb"))):
        pos = tap_positions(s, size, axis)
        for i, name in zip((0, 2), names):
            p = pos[i].expand(N, 1, 2 * Hs, 2 * Ws)
            p0, p1 = (p[:, :, 0::2, 0::2], p[:, :, 1::2, 0::2]) if axis == 2 else (p[:, :, 0::2, 0::2], p[:, :, 0::2, 1::2])
            ok = (p0 > -1) & (p0 < size) & (p1 > -1) & (p1 < size)
            f0, f1 = torch.floor(p0).to(torch.int64), torch.floor(p1).to(torch.int64)
            out[name] = ok & (f1 - f0 == 2) & (f0 % 2 != 0)
    return out


# ---- input families ---------------------------------------------------------------------------------------------------

def family_values(name):
    """The float32 values of s a family mixes into a random background."""
    ints = np.arange(-7, 9, dtype=np.float32)
    if name == "integers":
        v = ints
    elif name == "halves":
        v = np.arange(-6.5, 8.0, 1.0, dtype=np.float32)
    elif name == "neighbours":
        v = np.concatenate([np.nextafter(ints, np.float32(-np.inf)), np.nextafter(ints, np.float32(np.inf))])
    elif name == "clamps":
        v = np.array([-7.0, 8.0], dtype=np.float32)
    elif name == "one_zero":
        v = np.array([1.0, 0.0], dtype=np.float32)
    else:
        raise KeyError(name)
    return torch.from_numpy(v.astype(np.float32))


FAMILIES = ("integers", "halves", "neighbours", "clamps", "one_zero")


def family_scale_plane(name, N, H, W, seed, share=0.6):
    """s [N,1,H,W]: a uniform background in [-7, 8] with the family's values on `share` of the pixels (seeded, so every
    workgroup sees ordinary pixels as well).  The family's values cycle along the diagonals too, so that each value meets
    every row and column (and equal row and column indices: both axes of a pixel at the same distance from the border)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.empty(N, 1, H, W).uniform_(-7, 8, generator=g)
    vals = family_values(name)
    pick = torch.randint(0, len(vals), (N, 1, H, W), generator=g)
    hh = torch.arange(H).view(1, 1, H, 1)
    ww = torch.arange(W).view(1, 1, 1, W)
    nn = torch.arange(N).view(N, 1, 1, 1)
    diag = (hh == ww) | (hh == ww + 1)
    pick = torch.where(diag, (hh + 5 * nn) % len(vals), pick)
    use = (torch.rand(N, 1, H, W, generator=g) < share) | diag
    return torch.where(use, vals[pick], s).contiguous()


def unfoldable_table(size_stored):
    """(value, 'a' / 'b', stored index) of every neighbour-of-integer value and stored row (= column) index at which the
    pixel pair of an axis does not fold (unfoldable_pairs), on an axis of 2 * size_stored pixels: found by scanning the
    float32 geometry, one entry per hit."""
    tab = []
    for v in family_values("neighbours"):
        u = unfoldable_pairs(torch.full((1, 1, size_stored, 1), float(v)))
        for ab in "ab":
            for idx in torch.nonzero(u["y" + ab][0, 0, :, 0]).flatten().tolist():
                tab.append((float(v), ab, idx))
    return tab


def stored_scale_plane(name, N, Hs, Ws, seed, share=0.6):
    """family_scale_plane for the STORED scale plane of the up-sampled form.  For 'neighbours' the values of
    unfoldable_table are also put on the rows and the columns where the fold of the 2x2 block breaks -- every entry on
    three columns (rows) per image, so all four axes ya / yb / xa / xb meet it at every block-row / block-column the
    geometry allows -- and on the crossings of such a row and column, where two axes break in one block."""
    s = family_scale_plane(name, N, Hs, Ws, seed, share)
    if name != "neighbours":
        return s
    ytab, xtab = unfoldable_table(Hs), unfoldable_table(Ws)
    for n in range(N):
        for k, (v, _, iy) in enumerate(ytab):
            for m in range(3):
                s[n, 0, iy, (5 * k + 7 * m + n) % Ws] = v
        for k, (v, _, ix) in enumerate(xtab):
            for m in range(3):
                s[n, 0, (3 * k + 5 * m + n + 1) % Hs, ix] = v
        for v, _, iy in ytab:
            for v2, _, ix in xtab:
                if v2 == v:
                    s[n, 0, iy, ix] = v
    return s


def gather_inputs(N, C, H, W, seed, up2=False):
    """Seeded randn x, w and grad_d (x at the stored resolution for the up-sampled form)."""
    g = torch.Generator().manual_seed(seed)
    Hs, Ws = (H // 2, W // 2) if up2 else (H, W)
    x = torch.randn(N, C, Hs, Ws, generator=g)
    w = torch.randn(C, 1, 3, 3, generator=g)
    gd = torch.randn(N, C, H, W, generator=g)
    return x, w, gd


# ---- which kernel and which channel chunk a shape takes ---------------------------------------------------------------
# A SECOND COPY of the launchers' rules in codenet_amd/csrc/codenet_stage.hip, so that the shapes below can be checked
# against them without a GPU.  Mirrored, and to be changed together with them:
#   bwd2_chunk          static bwd2_cch(H, W, det)
#   bwd2u_chunk         static bwd2u_cch(N, C, Hs, Ws, det), with cdn::kCUs (cdn_common.h) as CUS
#   bwd_fallback_chunk  the "fallback for very large planes" branch of dw_backward_impl (150 KB budget, CC <= 16)
#   forward_kernel      static dw_channels_per_wg(C, H, W) + the kernel choice in dw_forward_impl
#   atomic_plan         the thread counts in dw_backward_impl (bwd_threads) and dw_up2_backward_impl (threads)
#   LDS_MAX             `lds_max = 160 * 1024 - 512` in those functions
# Only the reproducible forms' chunk can be asked of the library (cdn_codenet_dw_backward_workspace_bytes; the GPU tests
# assert it).  The atomic forms' chunk and the forward kernel rest on this copy: if a launcher threshold changes, the
# statements "which shape runs which path" go stale without a failing test -- test_the_shapes_take_the_paths_they_are_listed_for
# pins the thresholds as they were read from the code.

LDS_MAX = 160 * 1024 - 512
CUS = 256


def bwd2_chunk(H, W, det):
    """Channel chunk of dw_bwd2_kernel (0: the plane is beyond it -- dw_bwd_kernel, atomic form only)."""
    cells = (H + 1) * (W + 1)
    lds = lambda c: cells * c * 12 + c * 36 + 128 + (c * 16 * 36 if det else 0)
    cch = next((c for c in (32, 16, 8, 4, 2) if lds(c) <= LDS_MAX), 0)
    if cch >= 16 and lds(cch // 2) * 2 <= LDS_MAX:
        cch //= 2
    return cch


def bwd2u_chunk(N, C, H, W, det):
    """Channel chunk of dw_bwd2u_kernel for the up-sampled resolution H x W."""
    cells = (H // 2 + 1) * (W // 2 + 1)
    lds = lambda c: cells * c * 12 + c * 36 + 256 + (c * 16 * 36 if det else 0)
    cch = next((c for c in (32, 16, 8, 4, 2) if lds(c) <= LDS_MAX), 0)
    if cch == 0:
        return 0
    if cch >= 16 and lds(cch // 2) * 2 <= LDS_MAX:
        cch //= 2
    while cch > 4 and -(-C // cch) * N < CUS:
        cch //= 2
    return cch


def bwd_fallback_chunk(C, H, W):
    """Channels per workgroup of dw_bwd_kernel (0: not even one bordered plane pair fits)."""
    cc = (150 * 1024 // 4 - 64) // (2 * (H + 2) * (W + 2) + 18)
    return min(cc, 16, C)


def atomic_plan(up2, N, C, H, W):
    """(channel chunk, lanes) of the atomic backward of a shape, for chained_float32_sums: the number of private grad_w
    sums a workgroup adds into one LDS word -- (64 / chunk) pixels per wave x the waves of the workgroup -- or, for
    dw_bwd_kernel, -64 (one wave sum of 64 pixels per atomic)."""
    if up2:
        chunk = bwd2u_chunk(N, C, H, W, False)
        lds = (H // 2 + 1) * (W // 2 + 1) * chunk * 12 + chunk * 36 + 256
        threads = 768 if LDS_MAX // lds <= 1 else 256
        return chunk, (64 // chunk) * (threads // 64)
    chunk = bwd2_chunk(H, W, False)
    if chunk == 0:
        return bwd_fallback_chunk(C, H, W), -64
    lds = (H + 1) * (W + 1) * chunk * 12 + chunk * 36 + 128
    threads = 512 if lds * 2 <= LDS_MAX else 1024
    return chunk, (64 // chunk) * (threads // 64)


def forward_kernel(C, H, W):
    """Which forward kernel cdn_codenet_dw_forward launches."""
    pstride = (H + 2) * (W + 2)
    cc = (64 * 1024 // 4 - 64) // (pstride + 9)
    if cc < 4 and C % 4 == 0:
        cc = (76 * 1024 // 4 - 64) // (pstride + 9)
        if cc < 4:
            cc = (64 * 1024 // 4 - 64) // (pstride + 9)
    if cc < 1:
        return "dw_kernel<false>"
    cc = min(cc, 32, C)
    if cc >= 4 and C % 4 == 0:
        cc &= ~3
    return "dw4_kernel<false>" if (cc % 4 == 0 and C % 4 == 0) else "dw_kernel<true>"


# (N, C, H, W, path of the backward): the smallest shapes that reach each path; H * W is no multiple of 4 anywhere, C is
# ragged against the chunk (below it, chunk + 1) and C % 4 != 0 selects dw_kernel<true> in the forward
FULL_CASES = [
    (2, 17, 7, 9, "bwd2<16>"),       # 80 cells: chunk 16 (DPP records of 16 lanes), C = chunk + 1; forward dw_kernel<true>
    (1, 12, 5, 7, "bwd2<16>"),       # C below the chunk, planes under 8 pixels (the clamp values gate whole pixels);
                                      # forward dw4_kernel<false>
    (2, 9, 21, 21, "bwd2<8>"),       # 484 cells: chunk 8 (DPP records of 8 lanes), C = chunk + 1
    (1, 4, 19, 23, "bwd2<8>"),       # C below the chunk; forward dw4_kernel<false>
    (1, 5, 41, 43, "bwd2<4>"),       # 1848 cells: chunk 4 (plain path: geometry per lane), C = chunk + 1
    (1, 3, 59, 59, "bwd2<2>"),       # 3600 cells: chunk 2 (plain path), C = chunk + 1
    (1, 33, 1, 210, "bwd2<32>"),     # 422 cells exactly: the one plane size whose chunk stays 32 in the atomic form (32
                                      # channels fit, two workgroups of 16 do not); the reproducible form takes 8
    (1, 3, 82, 83, "bwd<2>"),        # 6972 cells, beyond dw_bwd2_kernel: dw_bwd_kernel, two bordered planes per workgroup + 1
    (1, 2, 127, 125, "bwd<1>"),      # dw_bwd_kernel with one plane per workgroup; forward dw_kernel<false> (global gather)
]
# (N, C, H, W at the up-sampled resolution, chunk of dw_bwd2u_kernel).  The chunk falls to 4 unless ceil(C / chunk) * N
# fills the 256 CUs: chunks above 4 need many channels, on tiny planes to stay cheap
UP2_CASES = [
    (4, 1032, 8, 8, 16),      # 65 chunks x 4 images = 260 workgroups: chunk 16, the last chunk holds 8 channels
    (2, 1028, 10, 6, 8),      # 129 x 2 = 258: chunk 8, the last chunk holds 4 channels; 15 stored pixels
    (2, 8, 32, 32, 4),        # the 16-row stored plane on which every entry of unfoldable_table occurs
    (3, 6, 20, 26, 4),        # C % 4 != 0 (backward only: the up-sampled forward needs channel quads), last chunk 2 channels
    (1, 4, 118, 122, 2),      # 60 x 62 = 3720 stored cells, above the 3394 that chunk 4 holds: chunk 2, 768 threads
]


def rel_err(got, ref64):
    """max |got - ref64| / max |ref64| (the figure every comparison here reports)."""
    m = ref64.abs().max().item()
    e = (got.double() - ref64).abs().max().item()
    return e / m if m > 0 else e


def bound(ref32, ref64, margin=4.0):
    """The bound granted to a kernel: `margin` times the same figure of the float32 evaluation of the reference, at least
    8 float32 ulps of the tensor's maximum.  ref32 may be a list of float32 evaluations (chained_float32_sums: one per
    order of the chain); the largest figure counts."""
    m = ref64.abs().max().item()
    if m == 0:
        return 0.0
    floor = 8.0 * float(np.spacing(np.float32(m))) / m
    return max(margin * yardstick(ref32, ref64), floor)


def yardstick(ref32, ref64):
    """The float32 figure: rel_err of the float32 evaluation (the largest of a list of them)."""
    return max(rel_err(r, ref64) for r in (ref32 if isinstance(ref32, (list, tuple)) else [ref32]))
