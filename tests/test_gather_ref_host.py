"""The plain gather reference (tests/gather_ref.py) on the CPU: it equals the float64 oracle wherever the two can be
compared (scales on a dyadic grid, where float32 and float64 positions coincide), the shapes of the GPU tests take the
kernel paths they are meant to take, and the input families of tests/test_gpu_gather_edges.py really sit on the edges --
counted from the float32 geometry, with stated minima -- and move grad_s there by far more than the bound a kernel gets."""
import numpy as np
import pytest
import torch

from oracle import dcn as O
from oracle import quant as Q
from tests import gather_ref as R

# how far above the bound of grad_s (R.bound with the plain float32 reference: 4 x its figure, at least 8 float32 ulps of
# the maximum -- the bound of the reproducible forms and of single-chunk atomic calls) the float64-position evaluation must
# lie at EVERY pixel where a rounded position decides: a kernel with a continuous but wrong rule misses the bound by at
# least this factor there.  (The atomic forms' grad_s over several chunks is bounded by 4 x the chained float32 figure,
# R.chained_float32_sums, up to 3 x the plain one at the 1028-channel shape: a factor of 300 at least.)
EDGE_FACTOR = 1000.0


def _oracle(x, s, w, gd):
    xd, sd, wd, gdd = x.double(), s.double(), w.double(), gd.double()
    anchor = Q.ANCHOR.double()
    off = anchor * (sd - 1)
    C = x.shape[1]
    d = O.deform_conv_forward(xd, off, wd, 1, 1, 1, C, 1)
    gx, goff = O.deform_conv_backward_input(xd, off, wd, gdd, 1, 1, 1, C, 1)
    gw = O.deform_conv_backward_params(xd, off, tuple(w.shape), gdd, 1, 1, 1, C, 1)
    return d, gx, (goff * anchor).sum(1, keepdim=True), gw


def _dyadic_scale(N, H, W, seed):
    """Multiples of 1/8 in [-7, 8]; the first pixels of image 0 get scales that put taps exactly on -1 and on `size`."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randint(-56, 65, (N, 1, H, W), generator=g).float() / 8
    s[0, 0, 0, 0] = 1.0                       # tap i = 0 of row 0: position -1 exactly (and the column's)
    s[0, 0, H - 1, W - 1] = 1.0               # tap i = 2 of the last row / column: position `size` exactly
    if W > 2:
        s[0, 0, 0, 1] = 2.0                   # column tap j = 0 of column 1: 0 - 1 = -1
        s[0, 0, 0, W - 2] = 2.0               # column tap j = 2 of column W - 2: W - 1 + 1 = W (and row tap i = 0: -2, out)
    return s


@pytest.mark.parametrize("N,C,H,W", [(1, 1, 1, 1), (2, 3, 5, 7), (1, 5, 9, 4), (3, 2, 8, 8), (1, 4, 13, 3)])
def test_float64_reference_equals_the_float64_oracle_on_dyadic_scales(N, C, H, W):
    x, w, gd = R.gather_inputs(N, C, H, W, seed=H * 10 + W)
    s = _dyadic_scale(N, H, W, seed=N)
    hit = R.edge_counts(s)
    assert hit["on_minus1"] >= 2 and hit["on_size"] >= 2, hit
    # float32 and float64 positions are the same numbers here: the flag changes nothing
    ref = R.gather_ref(x, s, w, gd)
    for a, b in zip(ref, R.gather_ref(x, s, w, gd, positions64=True)):
        assert torch.equal(a, b)
    for name, a, b in zip(("d", "grad_x", "grad_s", "grad_w"), ref, _oracle(x, s, w, gd)):
        assert a.dtype == torch.float64 and a.shape == b.shape
        # float64 rounding: sums of at most 36 (d), 9 * 4 * few (grad_x), 36 C (grad_s), 36 N H W (grad_w) terms
        assert (a - b).abs().max().item() <= 64 * np.finfo(np.float64).eps * max(1.0, b.abs().max().item()), name


@pytest.mark.parametrize("N,C,Hs,Ws", [(2, 3, 3, 4), (1, 2, 5, 2)])
def test_upsampled_reference_is_the_oracle_on_the_replicated_tensors(N, C, Hs, Ws):
    x, w, gd = R.gather_inputs(N, C, 2 * Hs, 2 * Ws, seed=7, up2=True)
    s = _dyadic_scale(N, Hs, Ws, seed=3)
    d, gx, gs, gw = R.gather_up2_ref(x, s, w, gd)
    od, ogx, ogs, ogw = _oracle(R.replicate2(x), R.replicate2(s), w, gd)
    tol = 64 * np.finfo(np.float64).eps
    assert (d - od).abs().max().item() <= tol * od.abs().max().item()
    assert (gx - R.fold2(ogx)).abs().max().item() <= tol * ogx.abs().max().item() * 4
    assert (gs - R.fold2(ogs)).abs().max().item() <= tol * ogs.abs().max().item() * 4
    assert (gw - ogw).abs().max().item() <= tol * ogw.abs().max().item()
    assert gx.shape == x.shape and gs.shape == s.shape


def test_float32_yardstick_is_close_and_not_identical():
    x, w, gd = R.gather_inputs(2, 5, 9, 11, seed=1)
    s = R.family_scale_plane("halves", 2, 9, 11, seed=2)
    r64, r32 = R.gather_ref(x, s, w, gd), R.gather_ref(x, s, w, gd, dtype=torch.float32)
    for a, b in zip(r32, r64):
        assert a.dtype == torch.float32
        assert 0 < R.rel_err(a, b) < 1e-6


def test_the_shapes_take_the_paths_they_are_listed_for():
    for N, C, H, W, path in R.FULL_CASES:
        assert (H * W) % 4 != 0
        kind, chunk = path.rstrip(">").split("<")
        if kind == "bwd2":
            assert R.bwd2_chunk(H, W, False) == int(chunk)
            assert R.bwd2_chunk(H, W, True) == (8 if chunk == "32" else int(chunk))
            assert C < int(chunk) or C == int(chunk) + 1
        else:
            assert R.bwd2_chunk(H, W, False) == 0 and R.bwd_fallback_chunk(C, H, W) == int(chunk)
    assert {p for *_, p in R.FULL_CASES} == {"bwd2<32>", "bwd2<16>", "bwd2<8>", "bwd2<4>", "bwd2<2>", "bwd<2>", "bwd<1>"}
    assert {R.forward_kernel(C, H, W) for _, C, H, W, _ in R.FULL_CASES} == {"dw_kernel<true>", "dw_kernel<false>",
                                                                             "dw4_kernel<false>"}
    for N, C, H, W, chunk in R.UP2_CASES:
        assert R.bwd2u_chunk(N, C, H, W, False) == R.bwd2u_chunk(N, C, H, W, True) == chunk
        assert C % chunk != 0 or C == 2 * chunk or chunk == 2
    assert {c for *_, c in R.UP2_CASES} == {16, 8, 4, 2}
    # the thresholds themselves: the largest plane of each chunk and the first one beyond it (atomic form)
    for cells, chunk in ((421, 16), (422, 32), (423, 8), (1697, 8), (1698, 4), (3397, 4), (3398, 2), (6797, 2), (6798, 0)):
        assert R.bwd2_chunk(cells - 1, 0, False) == chunk, cells


# ---- the families sit on the edges --------------------------------------------------------------------------------------

def test_integer_and_clamp_scales_put_taps_exactly_on_minus_one_and_on_size():
    """An integer scale lands a tap exactly on -1 or on `size` only within |s - 1| + 1 pixels of a border, so the count
    grows with the perimeter: at least N (H + W) / 16 taps on each of the two gates per plane (2 at least, 10 suffice)."""
    for N, C, H, W, _ in R.FULL_CASES:
        for fam in ("integers", "clamps", "one_zero"):
            if fam == "clamps" and max(H, W) < 9:      # (-7 and 8 throw every tap of so small a plane far outside)
                continue
            hit = R.edge_counts(R.family_scale_plane(fam, N, H, W, seed=H))
            need = max(2, min(10, N * (H + W) // 16))
            if fam == "clamps" and min(H, W) < 9:      # only two columns of the one long axis land on each gate
                need = 1
            assert hit["on_minus1"] >= need and hit["on_size"] >= need, (fam, H, W, hit)
    for N, C, H, W, _ in R.UP2_CASES:
        for fam in ("integers", "clamps"):
            hit = R.edge_counts(R.replicate2(R.stored_scale_plane(fam, N, H // 2, W // 2, seed=H)))
            assert hit["on_minus1"] >= 4 and hit["on_size"] >= 4, (fam, H, W, hit)


def test_clamp_scales_on_small_planes_gate_whole_pixels_down_to_the_centre_tap():
    """|s - 1| >= 7 moves every off-centre tap at least 8 pixels: on a 5 x 7 plane all eight are outside, on the 4 x 4
    stored plane (8 x 8 pixels) those of the pixels away from the far border."""
    N, C, H, W, _ = R.FULL_CASES[1]
    assert H < 8 and W < 8
    hit = R.edge_counts(R.family_scale_plane("clamps", N, H, W, seed=H))
    assert hit["centre_only"] >= N * H * W // 2, hit
    N, C, H, W, _ = R.UP2_CASES[0]
    hit = R.edge_counts(R.replicate2(R.stored_scale_plane("clamps", N, H // 2, W // 2, seed=H)))
    assert hit["centre_only"] >= N * H * W // 4, hit


def test_half_integers_never_touch_a_gate_exactly():
    for N, C, H, W, _ in R.FULL_CASES[:4]:
        hit = R.edge_counts(R.family_scale_plane("halves", N, H, W, seed=H))
        assert hit["on_minus1"] == 0 and hit["on_size"] == 0


def test_neighbour_scales_break_the_fold_on_every_axis_and_on_two_axes_at_once():
    """unfoldable_table finds twelve (value, row) pairs on a 16-row stored plane: seven values just below an integer for
    the b axes, five just above for the a axes -- among the 32 neighbours of -7 .. 8.  stored_scale_plane puts each on three
    columns (rows) and on the crossings, per image."""
    tab = R.unfoldable_table(16)
    assert len(tab) == 12 and {ab for _, ab, _ in tab} == {"a", "b"}
    assert sum(ab == "a" for _, ab, _ in tab) == 5
    for v, _, _ in tab:      # all of them neighbours of even integers
        assert float(v) != round(float(v)) and round(float(v)) % 2 == 0 and abs(float(v) - round(float(v))) < 1e-6
    # per case of R.UP2_CASES: the least number of blocks on (ya, yb, xa, xb) and with two axes at once.  Rows 0 .. 12
    # carry the table's entries, so planes with fewer stored rows / columns meet fewer of them; on the 5 x 3 stored
    # plane of the chunk-8 case no xa pair is in range at all (its only entry within 3 columns, nextafter(-6, 0) at
    # column 1, puts the tap at column 7 of 6): dw_bwd2u_kernel<8> meets the four-pass path on three axes
    least = [((8, 8, 8, 8), 4), ((6, 4, 0, 4), 2), ((16, 16, 16, 16), 8), ((24, 24, 24, 24), 12), ((8, 8, 8, 8), 4)]
    for (N, C, H, W, chunk), (per_axis, two) in zip(R.UP2_CASES, least):
        u = R.unfoldable_pairs(R.stored_scale_plane("neighbours", N, H // 2, W // 2, seed=H))
        n = {k: int(v.sum()) for k, v in u.items()}
        n["two"] = int(((u["ya"] | u["yb"]) & (u["xa"] | u["xb"])).sum())
        print(N, C, H, W, n)
        for k, need in zip(("ya", "yb", "xa", "xb"), per_axis):
            assert n[k] >= need, (H, W, k, n)
        assert n["two"] >= two, (H, W, n)
    assert int(R.unfoldable_pairs(R.stored_scale_plane("neighbours", 2, 5, 3, seed=10))["xa"].sum()) == 0
    # the other families never reach it
    for fam in ("integers", "halves", "clamps", "one_zero"):
        u = R.unfoldable_pairs(R.stored_scale_plane(fam, 2, 16, 16, seed=1))
        assert sum(int(v.sum()) for v in u.values()) == 0


# ---- and the edges move the answer ----------------------------------------------------------------------------------------

def _moved(fn, x, s, w, gd, where):
    """grad_s of the float32-position and the float64-position reference at the pixels `where` [N,1,h,w], as
    |difference| / max |grad_s|, with the bound a kernel is granted."""
    r64 = fn(x, s, w, gd)
    r32 = fn(x, s, w, gd, dtype=torch.float32)
    cont = fn(x, s, w, gd, positions64=True)
    bound = R.bound(r32[2], r64[2])
    diff = (cont[2] - r64[2]).abs() / r64[2].abs().max()
    return diff[where], bound


def test_a_continuous_rule_misses_grad_s_at_the_unfoldable_blocks_by_a_large_factor():
    N, C, H, W, _ = R.UP2_CASES[2]
    x, w, gd = R.gather_inputs(N, C, H, W, seed=11, up2=True)
    s = R.stored_scale_plane("neighbours", N, H // 2, W // 2, seed=H)
    u = R.unfoldable_pairs(s)
    where = u["ya"] | u["yb"] | u["xa"] | u["xb"]
    diff, bound = _moved(R.gather_up2_ref, x, s, w, gd, where)
    print("blocks", int(where.sum()), "bound", bound, "median moved", diff.median().item(), "min", diff.min().item())
    assert bound < 2e-6
    assert diff.min().item() > EDGE_FACTOR * bound           # at EVERY such pixel


@pytest.mark.parametrize("case", [0, 2])
def test_a_continuous_rule_misses_grad_s_where_float32_rounding_moves_a_floor_or_a_gate(case):
    """Full resolution, neighbours of integers: the pixels where a float32 position is an integer (or -1, or `size`)
    that the float64 position is not."""
    N, C, H, W, _ = R.FULL_CASES[case]
    x, w, gd = R.gather_inputs(N, C, H, W, seed=12)
    s = R.family_scale_plane("neighbours", N, H, W, seed=H)
    where = torch.zeros(N, 1, H, W, dtype=torch.bool)
    for size, axis in ((H, 2), (W, 3)):
        p32, p64 = R.tap_positions(s, size, axis), R.tap_positions(s, size, axis, positions64=True)
        for i in (0, 2):
            a, b = p32[i].expand(N, 1, H, W).double(), p64[i].expand(N, 1, H, W)
            inside = lambda p: (p > -1) & (p < size)
            where |= (inside(a) != inside(b)) | (inside(a) & inside(b) & (torch.floor(a) != torch.floor(b)))
    assert int(where.sum()) >= 20
    diff, bound = _moved(R.gather_ref, x, s, w, gd, where)
    print("pixels", int(where.sum()), "bound", bound, "median moved", diff.median().item(), "min", diff.min().item())
    assert bound < 2e-6
    assert diff.min().item() > EDGE_FACTOR * bound           # at EVERY such pixel


def test_contribution_counts_count_the_terms_of_grad_x():
    """s = 1: nine taps on grid points, one non-zero corner each -- every interior cell receives nine terms."""
    cnt = R.contribution_counts(torch.ones(1, 1, 5, 6))
    assert cnt.shape == (1, 1, 5, 6) and int(cnt[0, 0, 2, 2]) == 9 and int(cnt[0, 0, 0, 0]) == 4
    s = R.family_scale_plane("halves", 1, 6, 6, seed=0)
    x, w, gd = R.gather_inputs(1, 1, 6, 6, seed=0)
    _, gx, _, _ = R.gather_ref(x, s, torch.ones_like(w), torch.ones_like(gd))
    assert torch.equal(R.contribution_counts(s) > 0, gx != 0)


def test_chained_float32_sums_are_float32_evaluations_with_longer_chains():
    """The atomic forms' yardstick: the same summands as the plain float32 reference, added in chains -- close to the
    float64 reference, different between orders, and no better than the pairwise sum on a long chain."""
    N, C, H, W, _ = R.FULL_CASES[5]
    assert R.atomic_plan(False, N, C, H, W) == (2, 512)                     # 32 pixels per wave x 16 waves
    assert R.atomic_plan(False, *R.FULL_CASES[0][:4]) == (16, 32) and R.atomic_plan(False, *R.FULL_CASES[7][:4]) == (2, -64)
    assert R.atomic_plan(True, *R.UP2_CASES[4][:4]) == (2, 384) and R.atomic_plan(True, *R.UP2_CASES[0][:4]) == (16, 16)
    x, w, gd = R.gather_inputs(N, C, H, W, seed=105)
    s = R.family_scale_plane("halves", N, H, W, seed=H)
    r64, r32 = R.gather_ref(x, s, w, gd), R.gather_ref(x, s, w, gd, dtype=torch.float32)
    ch = R.chained_float32_sums(x, s, w, gd, False, 2, 512, orders=4)
    assert len(ch) == 4 and ch[0][0].dtype == torch.float32 and ch[0][1].shape == w.shape
    assert not torch.equal(ch[0][1], ch[1][1])
    figure = R.yardstick([c[1] for c in ch], r64[3])
    assert R.rel_err(r32[3], r64[3]) < figure < 1e-5
    assert R.yardstick([c[0] for c in ch], r64[2]) < 1e-6
    assert R.bound([c[1] for c in ch], r64[3]) == 4 * figure
