"""CPU proof that the inputs of tests/test_gpu_dcn_edges.py can tell a right kernel from a subtly wrong one (tests/dcn_edges.py):
the plain float64 restatement equals the C oracle to rounding on every case and family; every family reaches what it is
for; every mutant of the restatement moves an output by more than 100 x the bound the GPU test grants that output; and
what the strict gate removes is an exact zero, with no NaN of a non-finite offset in any output."""
import pytest
import torch

from tests import dcn_edges as E

ALL_ROWS = [(i, f) for i in range(len(E.GEOMS)) for f in E.FAMILIES] + [("stride", "all")]


def _geom(i):
    return E.STRIDE_CASE if i == "stride" else E.GEOMS[i]


@pytest.mark.parametrize("row,family", ALL_ROWS)
def test_the_restatement_equals_the_oracle_in_float64(row, family):
    """|restatement - oracle| <= (terms + 2) 2^-53 sum |terms| per element (E.term_bound), plain and modulated with bias."""
    g = _geom(row)
    for modulated in (False, True):
        inp = E.make_inputs(g, family, 0, modulated, modulated)
        want, got = E.oracle_outputs(inp, torch.float64), E.restate_inputs(inp, torch.float64)
        assert set(want) == set(got)
        for name in want:
            assert torch.isfinite(want[name]).all() and torch.isfinite(got[name]).all(), name
            slack = (E.term_bound(inp, name) - (got[name] - want[name]).abs()).min().item()
            print("DCN-HOST %s %s %s %s: smallest slack %.3e" % (g.tag(), family, "mod" if modulated else "plain", name, slack))
            assert slack >= 0, (name, slack)


@pytest.mark.parametrize("row,family", ALL_ROWS)
@pytest.mark.parametrize("half", [False, True])
def test_every_family_reaches_what_it_is_for(row, family, half):
    g = _geom(row)
    inp = E.make_inputs(g, family, 0, half=half)
    info, c = inp.info, E.edge_counts(g, inp.off)
    entries = g.N * g.DG * g.K * g.P
    print("DCN-HOST %s %s half=%d: %d entries, %d placed, %d survive, %s" % (
        g.tag(), family, half, entries, int(info["placed"].sum()), int(info["family"].sum()), c))
    # no position is rounded: every tap lands in the same cell in float32 and in float64
    assert info["inexact"] == 0
    survive, placed = int(info["family"].sum()), int(info["placed"].sum())
    assert survive >= min(20, placed) and placed >= 1
    big = entries >= 64
    if family in ("integers", "all"):
        assert c["integer_rows"] >= (20 if big else 1) and c["integer_cols"] >= (20 if big else 1)
    if family in ("halves", "all") and big:
        # taps whose only live corner is the lower-right one (both axes in (-1, 0)) / the upper-left one
        assert c["only_lower_right"] >= 1 and c["only_upper_left"] >= 1
    if family in ("gates", "all"):
        assert c["on_minus1"] + c["on_size"] >= (8 if big else 1)
        if big:
            assert c["on_minus1"] >= 2 and c["on_size"] >= 2
    if family in ("far", "all") and (big or family == "far"):
        assert c["nonfinite_gated"] >= 1
        o = inp.off
        if big and not half:
            assert (o.abs() == 3e9).any() and torch.isinf(o).any() and torch.isnan(o).any() and (o.abs() == 1e4).any()


def test_the_grid_stride_case_exceeds_the_launch_cap():
    for name, total in E.STRIDE_CASE.totals().items():
        assert total > E.GRID_CAP, name
    assert E.STRIDE_CASE.totals() == {"fwd": 1486848, "bwd_input": 4460544, "bwd_offset": 1115136}
    assert max(max(g.totals().values()) for g in E.GEOMS) < E.GRID_CAP


# mutant -> (rows, family) meant to catch it
CATCHERS = {
    "gate": ([0, 7], "gates"),
    "corner": ([0, 6], "halves"),
    "left_derivative": ([0, 4], "integers"),
    "swap_hw": ([2, 3], "halves"),
    "dg_local": ([1, 7, "stride"], "integers"),
}


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_every_mutant_moves_an_output_by_100_bounds(mutant):
    rows, family = CATCHERS[mutant]
    for row in rows:
        g = _geom(row)
        family_ = "all" if row == "stride" else family
        for modulated in (False, True):
            inp = E.make_inputs(g, family_, 0, modulated, modulated)
            refs = E.References(inp, orders=1 if row == "stride" else 4)
            mut = E.restate_inputs(inp, torch.float64, mutant=mutant)
            worst = {}
            for name, ref in refs.ref64.items():
                lim = E.bound(name, refs) * ref.abs().max().item()      # the GPU test's bound, in absolute terms
                d = (mut[name] - ref).abs().max().item()
                worst[name] = d / lim if lim > 0 else (float("inf") if d > 0 else 0.0)
            print("DCN-HOST mutant %s on %s %s %s: moves / bound %s" % (
                mutant, g.tag(), family_, "mod" if modulated else "plain", {k: "%.3g" % v for k, v in worst.items()}))
            assert max(worst.values()) > 100, (mutant, g.tag(), worst)
            if mutant in ("gate", "left_derivative"):
                # the mistakes a forward comparison cannot see: the sample is continuous there, its derivative is not
                assert worst["grad_offset"] > 100


@pytest.mark.parametrize("row,family", [(r, f) for r, f in ALL_ROWS if f in ("gates", "far", "all")])
def test_gated_entries_are_exact_zeros_and_no_nan_escapes(row, family):
    """grad_offset of both axes and grad_mask at a gated (pixel, tap) entry are exact zeros in the reference, and the
    entry's share of `out` is: zeroing the weights of the gated taps leaves `out` bit for bit."""
    g = _geom(row)
    inp = E.make_inputs(g, family, 0, True, True)
    gated = E.gated_entries(g, inp.off)                                     # [N, DG, K, Ho, Wo]
    assert gated.any()
    for dtype in (torch.float64, torch.float32):
        for res in (E.oracle_outputs(inp, dtype), E.restate_inputs(inp, dtype)):
            for name, t in res.items():
                assert torch.isfinite(t).all(), name
            go = res["grad_offset"].view(g.N, g.DG, g.K, 2, g.Ho, g.Wo)
            assert (go[:, :, :, 0][gated] == 0).all() and (go[:, :, :, 1][gated] == 0).all()
            assert (res["grad_mask"].view(g.N, g.DG, g.K, g.Ho, g.Wo)[gated] == 0).all()
    if g.DG == 1 and row != "stride":
        # the share of `out`: an output pixel all of whose taps are gated is the bias alone
        dead = gated.all(2)[:, 0]                                            # [N, Ho, Wo]
        out = E.oracle_outputs(inp, torch.float64)["out"]
        want = inp.bias.double().view(1, -1, 1, 1).expand_as(out)
        assert torch.equal(out.permute(0, 2, 3, 1)[dead], want.permute(0, 2, 3, 1)[dead])
    # a mask of any size at a gated entry does not reach `out`
    big = types_copy(inp)
    m = big.mask.view(g.N, g.DG, g.K, g.Ho, g.Wo).clone()
    m[gated] = 1e30
    big.mask = m.view_as(inp.mask)
    assert torch.equal(E.restate_inputs(big, torch.float64)["out"], E.restate_inputs(inp, torch.float64)["out"])
    assert torch.equal(E.oracle_outputs(big, torch.float64)["out"], E.oracle_outputs(inp, torch.float64)["out"])


def types_copy(inp):
    import types
    return types.SimpleNamespace(**vars(inp))


def test_structured_families_put_taps_on_the_gates_and_on_integers():
    for N, C, H, W in E.STRUCTURED_CASES:
        for fam in E.STRUCTURED_FAMILIES:
            t = E.structured_t(fam, N, H, W, 0)
            off = (E.ANCHOR * t).contiguous()
            c = E.edge_counts(E.fast_geom(N, 1, H, W), off)
            print("DCN-HOST structured %dx%dx%d %s: %s" % (N, H, W, fam, c))
            assert torch.equal(off[:, 16:17], t)
            if fam == "gates":
                assert c["on_minus1"] >= 20 and c["on_size"] >= 20
            if fam == "integers_halves":
                assert c["integer_rows"] >= 9 * N * H * W // 4
