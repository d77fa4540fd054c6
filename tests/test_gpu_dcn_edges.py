"""The generic (modulated) deformable convolution (codenet_amd/csrc/dcn_generic.hip: fwd_kernel, bwd_input_kernel,
bwd_offset_kernel, bwd_weight_kernel, bwd_bias_kernel in float32, float64 and half; the depthwise fast paths dwo_kernel,
dwo4_kernel, dwo_bwd_kernel, dwo_wgrad_kernel and the structured dwos_bwd_kernel) against the float64 C oracle, through the
C ABI, on offsets that sit ON the edges: integer and half-integer positions, positions exactly on -1 and on `size` and both
float32 neighbours of the gates, offsets of +-1e4, +-3e9, +-inf and NaN -- each mixed into a random background
(tests/dcn_edges.py; tests/test_dcn_edges_host.py proves on the CPU that these inputs reach the edges and catch the
mutants).  The grid-stride case takes the second trip of the three grid-stride loops in all three types.

Every output is compared as  max |got - ref64| / max |ref64|  per tensor, no element left out, against MARGIN x the same
figure of the float32 evaluation on the same inputs (at least 8 float32 ulps of the tensor's maximum); x 2^-29 for the
float64 kernels, plus the float64 reference's own error (References.own_error: the oracle is a float64 evaluation too); + 2^-11 for half outputs stored once; grad_input in half per cell, (n + 1) 2^-11 S.  grad_weight and
grad_bias are `got - initial` on buffers of random values: the store of initial + sum adds one unit roundoff of the storage
type at the size of that value (_accumulation_allowance).

The float32 evaluation is the C oracle in float32 AND the restatement in float32 summed as the kernels sum (the larger
figure counts): the oracle forms its contractions in double whatever the tensor type, so its float32 figure is one or two
roundings per element and says nothing about a chain of Cg * K float32 additions (fwd_kernel), of N Ho Wo / 256 additions
per thread and a tree (bwd_weight_kernel) or of float atomics in arrival order (bwd_input_kernel: 4 seeded orders).
grad_offset of dwo_bwd_kernel and of dwos_bwd_kernel ends in float atomics over channel chunks: its yardstick sums the
per-channel terms of the float32 oracle (run on channel slices) in chains of the kernel's lengths in 8 seeded orders.
Every comparison prints its figures (pytest -s)."""
import functools
import types

import pytest
import torch

from tests import dcn_edges as E
from tests import gather_ref as R

pytestmark = pytest.mark.gpu

TYPES = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16}


def _lib():
    from codenet_amd import _native as N_
    return N_, N_.lib()


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, dtype):
    return None if t is None else t.to(dtype).cuda().contiguous()


@functools.lru_cache(maxsize=8)
def _refs(row, family, modulated, with_bias, half, orders=4):
    g = E.STRIDE_CASE if row == "stride" else E.GEOMS[row]
    return E.References(E.make_inputs(g, family, 0, modulated, with_bias, half), orders)


class _Report:
    """Collects the figures of one test, prints them, and fails at the end if any exceeds its bound."""
    worst = {}      # kernel family -> [largest err / float32 figure of the outputs stored once in float32 / float64 with
                    # nothing granted beyond MARGIN x that figure, largest err / bound of every comparison]

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def check(self, fam, name, got, ref64, ref32, scale=1.0, add=0.0):
        got = got.detach().cpu()
        assert got.shape == ref64.shape and torch.isfinite(got).all(), (self.tag, name)
        err, e32 = R.rel_err(got, ref64), scale * R.yardstick(ref32, ref64)
        m = ref64.abs().max().item()
        lim = (scale * R.bound(ref32, ref64, E.MARGIN) + add) if m > 0 else 0.0
        ratio = err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))
        print("DCN %s | %s %s: err %.3e  float32 figure %.3e  ratio %.2f  bound %.3e" % (self.tag, fam, name, err, e32, ratio, lim))
        w = _Report.worst.setdefault(fam, [0.0, 0.0])
        if add == 0.0 and ratio != float("inf"):
            w[0] = max(w[0], ratio)
        if lim > 0:
            w[1] = max(w[1], err / lim)
        if not err <= lim:
            self.bad.append((fam, name, err, lim))

    def done(self):
        assert not self.bad, (self.tag, self.bad)


def _call(inp, tag, scale=1.0, gw0=None, gb0=None, gx=None, fill=float("nan")):
    """One forward, one backward_input and one backward_parameters call (one backward call for the modulated op) through
    the C ABI on dirty buffers: out, grad_offset and grad_mask start NaN-filled, grad_input on zeros (or the caller's
    view), grad_weight / grad_bias on the caller's values."""
    N_, lib = _lib()
    g, dt = inp.g, TYPES[tag]
    code = {"f32": N_.CDN_F32, "f64": N_.CDN_F64, "f16": N_.CDN_F16}[tag]
    x, off, w, gout, mask, bias = (_dev(t, dt) for t in (inp.x, inp.off, inp.w, inp.gout, inp.mask, inp.bias))
    out = torch.full((g.N, g.Co, g.Ho, g.Wo), fill, dtype=dt, device="cuda")
    goff = torch.full_like(off, fill)
    gx = torch.zeros_like(x) if gx is None else gx
    gw = torch.zeros_like(w) if gw0 is None else _dev(gw0, dt)
    res = {"out": out, "grad_input": gx, "grad_offset": goff, "grad_weight": gw}
    if mask is None:
        N_.check(lib.cdn_deform_conv_forward(_p(x), _p(w), _p(off), _p(out), code, *g.abi_plain(), _stream()), "forward")
        N_.check(lib.cdn_deform_conv_backward_input(_p(x), _p(off), _p(gout), _p(gx), _p(goff), _p(w), code, *g.abi_plain(),
                                                    _stream()), "backward_input")
        N_.check(lib.cdn_deform_conv_backward_parameters(_p(x), _p(off), _p(gout), _p(gw), code, *g.abi_plain(), scale,
                                                         _stream()), "backward_parameters")
    else:
        assert scale == 1.0
        wb = int(bias is not None)
        gm = torch.full_like(mask, fill)
        gb = (torch.zeros(g.Co, dtype=dt, device="cuda") if gb0 is None else _dev(gb0, dt)) if wb else None
        N_.check(lib.cdn_modulated_deform_conv_forward(_p(x), _p(w), _p(bias), _p(off), _p(mask), _p(out), code,
                                                       *g.abi_modulated(), wb, _stream()), "modulated forward")
        N_.check(lib.cdn_modulated_deform_conv_backward(_p(x), _p(w), _p(bias), _p(off), _p(mask), _p(gx), _p(gw), _p(gb),
                                                        _p(goff), _p(gm), _p(gout), code, *g.abi_modulated(), wb, _stream()),
                 "modulated backward")
        res["grad_mask"] = gm
        if wb:
            res["grad_bias"] = gb
    torch.cuda.synchronize()
    return res


def _accumulation_allowance(ref64, init, tag):
    """The store of `initial + scale x sum` rounds to the size of that value, not of the sum: one unit roundoff of the
    kernel's storage type on max |initial + reference|, in units of max |reference| (the figure's denominator)."""
    u = {"f32": 2.0 ** -24, "f64": 2.0 ** -53, "f16": E.U16}[tag]
    m = ref64.abs().max().item()
    return u * (init.double() + ref64).abs().max().item() / m if m > 0 else 0.0


def _check_zeros_at_gated(inp, got):
    g = inp.g
    gated = E.gated_entries(g, inp.off)
    go = got["grad_offset"].cpu().view(g.N, g.DG, g.K, 2, g.Ho, g.Wo)
    assert (go[:, :, :, 0][gated] == 0).all() and (go[:, :, :, 1][gated] == 0).all()
    if "grad_mask" in got:
        assert (got["grad_mask"].cpu().view(g.N, g.DG, g.K, g.Ho, g.Wo)[gated] == 0).all()
    if g.DG == 1 and "out" in got:
        # the gated taps' share of `out`: a pixel all of whose taps are gated is the bias alone (zero without one), exactly
        dead = gated.all(2)[:, 0]                                              # [N, Ho, Wo]
        out = got["out"].cpu().double().permute(0, 2, 3, 1)[dead]              # [pixels, Co]
        want = inp.bias.double() if inp.bias is not None else torch.zeros(g.Co, dtype=torch.float64)
        assert torch.equal(out, want.view(1, -1).expand_as(out))


def _compare(rep, fam, refs, got, tag, scale=1.0, gw0=None, gb0=None):
    sc = E.F64_OVER_F32 if tag == "f64" else 1.0
    add = E.U16 if tag == "f16" else 0.0
    own = (lambda n: refs.own_error(n)) if tag == "f64" else (lambda n: 0.0)      # (the float64 reference's own error)
    for name in ("out", "grad_offset", "grad_mask"):
        if name in got:
            rep.check(fam, name, got[name], refs.ref64[name], refs.ref32[name], sc, add + own(name))
    if tag != "f16":
        rep.check(fam, "grad_input", got["grad_input"], refs.ref64["grad_input"], refs.ref32["grad_input"], sc, own("grad_input"))
    for name, init in (("grad_weight", gw0), ("grad_bias", gb0)):
        if name in got:
            init = torch.zeros_like(refs.ref64[name], dtype=torch.float32) if init is None else init
            k = scale if name == "grad_weight" else 1.0
            ref64 = k * refs.ref64[name]
            rep.check(fam, name, got[name].cpu().double() - init.double(), ref64, [k * r for r in refs.ref32[name]], sc,
                      _accumulation_allowance(ref64, init, tag) + own(name))
    _check_zeros_at_gated(refs.inp, got)


def _inits(g, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(g.Co, g.Cg, g.kH, g.kW, generator=gen), torch.randn(g.Co, generator=gen)


ROWS = [(i, f, t) for i, g in enumerate(E.GEOMS) for f in E.FAMILIES for t in ("f32", "f64") if g.only in (None, t)]


@pytest.mark.parametrize("row,family,tag", ROWS)
def test_generic_kernels_on_the_edge_families(row, family, tag):
    """Every row of GEOMS, plain (grad_weight scaled by 0.5 and by 1) and modulated without and with bias (the non-square
    rows too: the raw ABI takes (h, w) pairs); grad_weight and grad_bias accumulate onto random values."""
    g = E.GEOMS[row]
    rep = _Report("%s %s %s" % (g.tag(), family, tag))
    gw0, gb0 = _inits(g)
    for modulated, with_bias in ((False, False), (True, False), (True, True)):
        refs = _refs(row, family, modulated, with_bias, False)
        fam = "generic %s %s" % ("modulated" if modulated else "plain", tag)
        for scale in ((0.5, 1.0) if not modulated else (1.0,)):
            got = _call(refs.inp, tag, scale, gw0, gb0)
            _compare(rep, fam, refs, got, tag, scale, gw0, gb0)
    rep.done()


def _second_trip(g, name, t):
    """The elements of an output that threads with idx >= GRID_CAP produce."""
    cap = E.GRID_CAP
    if name == "out":
        return t.reshape(-1)[cap:]
    if name == "grad_offset":      # thread (n, dg, k, p) writes both axes of its tap
        return t.view(g.N * g.DG * g.K, 2, g.P).permute(0, 2, 1).reshape(-1, 2)[cap:].reshape(-1)
    if name == "grad_mask":
        return t.reshape(-1)[cap:]
    if name == "grad_input":       # thread (n, c, k, p): the planes all of whose threads are beyond the cap
        return t.view(g.N * g.C, -1)[-(-cap // (g.K * g.P)):].reshape(-1)
    raise KeyError(name)


@pytest.mark.parametrize("tag", ["f32", "f64", "f16"])
def test_grid_stride_loops_take_a_second_trip(tag):
    """STRIDE_CASE: 1 486 848, 4 460 544 and 1 115 136 threads of work in fwd_kernel, bwd_input_kernel and
    bwd_offset_kernel against a launch of 1 048 576.  Modulated with bias; the error of the elements produced beyond the
    cap is reported on its own (in units of the whole tensor's maximum)."""
    g = E.STRIDE_CASE
    assert all(v > E.GRID_CAP for v in g.totals().values())
    half = tag == "f16"
    refs = _refs("stride", "all", True, True, half, 2)
    rep = _Report("stride %s" % tag)
    got = _call(refs.inp, tag)
    fam = "generic modulated %s" % tag
    _compare(rep, fam, refs, got, tag)
    if half:
        _check_half_grad_input(rep, refs, got["grad_input"])
    for name in ("out", "grad_offset", "grad_mask", "grad_input"):
        ref = refs.ref64[name]
        a, b = _second_trip(g, name, got[name].cpu().double()), _second_trip(g, name, ref)
        assert a.numel() > 0 and b.abs().max() > 0
        m = ref.abs().max().item()
        print("DCN stride %s | %s beyond the cap: %d elements, err %.3e (whole tensor %.3e)" % (
            tag, name, a.numel(), (a - b).abs().max().item() / m, R.rel_err(got[name].cpu(), ref)))
    rep.done()


def _check_half_grad_input(rep, refs, gx):
    """grad_input in half is a chain of half-rounded atomic adds: per cell |got - ref64| <= (n + 1) 2^-11 S plus the float32
    allowance (MARGIN x the float32 figure, in absolute terms)."""
    ref = refs.ref64["grad_input"]
    gx = gx.cpu().double()
    assert torch.isfinite(gx).all()
    allow = refs.half_input_allowance() + E.bound("grad_input", refs) * ref.abs().max().item()
    excess = ((gx - ref).abs() - allow).max().item()
    print("DCN %s | half grad_input: err %.3e, largest allowance %.3e, smallest slack %.3e" % (
        rep.tag, (gx - ref).abs().max().item(), allow.max().item(), -excess))
    if excess > 0:
        rep.bad.append(("half", "grad_input", excess, 0.0))


@pytest.mark.parametrize("row,family,modulated", [(7, "halves", False), (7, "gates", True), (2, "integers", True),
                                                  (2, "far", True)])
def test_half_on_the_straddling_and_the_non_square_row(row, family, modulated):
    """Half with a mask, with deformable_groups > 1 and on non-square geometry; the reference is the float64 oracle on the
    half-rounded inputs.  (grad_weight and grad_bias start from zeros here: a half store of `initial + sum` rounds to the
    initial value's size, which the accumulation tests of float32 and float64 cover without that rounding.)"""
    g = E.GEOMS[row]
    refs = _refs(row, family, modulated, modulated, True)
    rep = _Report("%s %s f16" % (g.tag(), family))
    got = _call(refs.inp, "f16")
    for t in got.values():
        assert t.dtype == torch.float16
    _compare(rep, "generic %s f16" % ("modulated" if modulated else "plain"), refs, got, "f16")
    _check_half_grad_input(rep, refs, got["grad_input"])
    rep.done()


def test_half_grad_input_on_the_high_half_of_a_word():
    """grad_input as an odd-offset contiguous view (data_ptr % 4 == 2) into a larger half buffer: every atomic add is a
    compare-and-swap on the 32-bit word that holds the element, the first and the last element share their words with a
    sentinel each.  The sentinels stay bitwise unchanged."""
    g = E.STRADDLE
    refs = _refs(7, "integers", True, True, True)
    n = g.N * g.C * g.H * g.W
    buf = torch.zeros(n + 4, dtype=torch.float16, device="cuda")
    assert buf.data_ptr() % 4 == 0
    sentinel = torch.tensor([1.2345, -77.5, 3.0e-5, 6.0e4], dtype=torch.float16)
    buf[0], buf[n + 1], buf[n + 2], buf[n + 3] = sentinel[0], sentinel[1], sentinel[2], sentinel[3]
    gx = buf[1:n + 1].view(g.N, g.C, g.H, g.W)
    assert gx.data_ptr() % 4 == 2 and gx.is_contiguous()
    rep = _Report("%s odd view f16" % g.tag())
    got = _call(refs.inp, "f16", gx=gx)
    _check_half_grad_input(rep, refs, got["grad_input"])
    after = buf.cpu()
    assert torch.equal(after[[0, n + 1, n + 2, n + 3]].view(torch.int16), sentinel.view(torch.int16))
    # and the aligned call gives the same cells to the same allowance
    _check_half_grad_input(rep, refs, _call(refs.inp, "f16")["grad_input"])
    rep.done()


def test_the_python_api_gives_the_bits_of_the_abi_call():
    """deform_conv on the non-square row and modulated_deform_conv on the straddling row: the outputs that do not end in
    float atomics are bit for bit those of the raw ABI call on zeroed accumulators; grad_input (float atomics in arrival
    order) to its bound."""
    from codenet_amd.functions.dcn_deform_conv import deform_conv, modulated_deform_conv
    for row, family, modulated in ((2, "gates", False), (7, "gates", True)):
        g = E.GEOMS[row]
        refs = _refs(row, family, modulated, modulated, False)
        inp = refs.inp
        raw = _call(inp, "f32")
        x, off, w, gout = (t.cuda().requires_grad_(True) for t in (inp.x, inp.off, inp.w, inp.gout))
        if modulated:
            m, b = inp.mask.cuda().requires_grad_(True), inp.bias.cuda().requires_grad_(True)
            out = modulated_deform_conv(x, off, m, w, b, g.sH, g.pH, g.dH, g.G, g.DG)
        else:
            out = deform_conv(x, off, w, *g.cfg())
        out.backward(gout.detach())
        api = {"out": out.detach(), "grad_offset": off.grad, "grad_weight": w.grad}
        if modulated:
            api.update(grad_mask=m.grad, grad_bias=b.grad)
        for name, t in api.items():
            assert torch.equal(t, raw[name]), (g.tag(), name)
        rep = _Report("%s api" % g.tag())
        rep.check("generic %s f32" % ("modulated" if modulated else "plain"), "grad_input", x.grad, refs.ref64["grad_input"],
                  refs.ref32["grad_input"])
        rep.done()


# ---- the depthwise fast paths ------------------------------------------------------------------------------------------

def _fast_call(inp, scratch_bytes=None, gw0=None, scale=1.0):
    """forward, backward_input (through the scratch entry point when scratch_bytes is given) and backward_parameters of the
    CoDeNet call geometry in float32."""
    N_, lib = _lib()
    g = inp.g
    x, off, w, gout = (_dev(t, torch.float32) for t in (inp.x, inp.off, inp.w, inp.gout))
    nan = float("nan")
    out, goff, gx = torch.full_like(x, nan), torch.full_like(off, nan), torch.zeros_like(x)
    gw = torch.zeros_like(w) if gw0 is None else gw0.cuda()
    N_.check(lib.cdn_deform_conv_forward(_p(x), _p(w), _p(off), _p(out), N_.CDN_F32, *g.abi_plain(), _stream()), "forward")
    scratch = None
    if scratch_bytes is None:
        N_.check(lib.cdn_deform_conv_backward_input(_p(x), _p(off), _p(gout), _p(gx), _p(goff), _p(w), N_.CDN_F32,
                                                    *g.abi_plain(), _stream()), "backward_input")
    else:
        scratch = torch.full((scratch_bytes // 4,), nan, device="cuda")
        N_.check(lib.cdn_deform_conv_backward_input_scratch(_p(x), _p(off), _p(gout), _p(gx), _p(goff), _p(w), N_.CDN_F32,
                                                            *g.abi_plain(), _p(scratch), scratch_bytes, _stream()),
                 "backward_input_scratch")
    N_.check(lib.cdn_deform_conv_backward_parameters(_p(x), _p(off), _p(gout), _p(gw), N_.CDN_F32, *g.abi_plain(), scale,
                                                     _stream()), "backward_parameters")
    torch.cuda.synchronize()
    return {"out": out, "grad_input": gx, "grad_offset": goff, "grad_weight": gw}, scratch


@pytest.mark.parametrize("shape", E.FAST_CASES)
@pytest.mark.parametrize("family", E.FAMILIES)
def test_depthwise_fast_paths_on_unstructured_edge_offsets(shape, family):
    """dwo_kernel / dwo4_kernel, dwo_bwd_kernel<., true>, dwo_wgrad_kernel / dwo_bwd_kernel<., false> on 18-channel offsets of
    every family.  grad_offset: one float atomic per (pixel, tap, axis, channel chunk) -- the chained yardstick; grad_weight:
    threads / chunk private sums per weight and image, then one float atomic per image onto the caller's values."""
    N, C, H, W = shape
    g = E.fast_geom(*shape)
    inp = E.make_inputs(g, family, 0)
    refs = E.References(inp, orders=1)
    lanes = E.dwo_wgrad_lanes(N, C, H, W)
    refs.ref32["grad_weight"].append(E.restate_inputs(inp, torch.float32, lanes=lanes)["grad_weight"])
    chunk = E.dwo_bwd_input_chunk(H, W)
    assert chunk in (2, 4)
    if -(-C // chunk) > 1:
        refs.ref32["grad_offset"] = E.chained_channel_sums(E.per_channel_grad_offset32(inp), chunk)
    gw0 = torch.randn(C, 1, 3, 3, generator=torch.Generator().manual_seed(3))
    rep = _Report("fast %dx%dx%dx%d %s" % (N, C, H, W, family))
    for scale in (0.5, 1.0):
        got, _ = _fast_call(inp, None, gw0, scale)
        got2, _ = _fast_call(inp, None, gw0, scale)
        assert torch.equal(got["grad_input"], got2["grad_input"]) and torch.equal(got["out"], got2["out"])
        _compare(rep, "fast unstructured f32", refs, got, "f32", scale, gw0)
    if family == "gates":
        # the shim's route (structure plane in `columns`, the count sends the call to dwo_bwd_kernel) gives the same bits
        from codenet_amd.functions.dcn_deform_conv import deform_conv
        x, off, w = (v.cuda().requires_grad_(True) for v in (inp.x, inp.off, inp.w))
        out = deform_conv(x, off, w, 1, 1, 1, C, 1)
        out.backward(inp.gout.cuda())
        assert torch.equal(out.detach(), got["out"]) and torch.equal(x.grad, got["grad_input"])
    rep.done()


@pytest.mark.parametrize("shape", E.STRUCTURED_CASES)
@pytest.mark.parametrize("family", E.STRUCTURED_FAMILIES)
def test_structured_backward_input_on_edge_scales(shape, family):
    """dwos_bwd_kernel (MODE 0 at 16 x 16 and 32 x 32, the split MODE 1 + 2 at 64 x 64) on offsets anchor * t with t on
    integers and halves, on both float32 neighbours of every integer, and on the values that put a tap exactly on -1 and
    on `size`: weights (1, 0) on an integer axis, the neighbour cell read for the derivative.  Positions ARE rounded in
    float32 here (h - 1 - t next to an integer), so the reference is the restatement in float64 on the float32 positions
    (as tests/gather_ref.py does).  Full scratch and minimum scratch (the latter ends in float atomics) give grad_input
    bit for bit; the structured and the generic route keep the relations of test_gpu_parity.py."""
    N_, lib = _lib()
    N, C, H, W = shape
    g = E.fast_geom(*shape)
    inp = E.make_inputs(g, "integers", 0)
    t = E.structured_t(family, N, H, W, 1)
    inp.off = (E.ANCHOR * t).contiguous()
    r64 = E.restate_inputs(inp, torch.float64, pos_dtype=torch.float32)
    r32 = E.restate_inputs(inp, torch.float32)
    refs = types.SimpleNamespace(inp=inp, ref64=r64, ref32={k: [v] for k, v in r32.items()})
    full = lib.cdn_deform_conv_backward_input_scratch_bytes(*g.abi_plain())
    least = lib.cdn_deform_conv_backward_input_scratch_min_bytes(*g.abi_plain())
    assert least == (N * H * W + 4) * 4 and full >= least
    chunk, group = E.dwos_goff_chunk(N, C, H, W)
    per_c = E.per_channel_grad_offset32(inp)
    atomic = E.chained_channel_sums(per_c, chunk, group)
    ordered = E.chained_channel_sums(per_c, chunk, group, natural=True)
    rep = _Report("structured %dx%dx%dx%d %s" % (N, C, H, W, family))
    outs = {}
    for what, nbytes in (("full", full), ("min", least), ("generic", None)):
        got, scratch = _fast_call(inp, nbytes)
        outs[what] = got
        if scratch is not None:
            assert scratch[N * H * W:N * H * W + 1].view(torch.int32).item() == 0          # every pixel has the structure
            assert torch.equal(scratch[:N * H * W].view(N, 1, H, W).cpu(), t)
        fam = "structured f32" if nbytes else "fast unstructured f32"
        stores = what == "full" and full > least + 16                                      # the chunks' planes, summed in order
        refs.ref32["grad_offset"] = ordered if stores else (
            atomic if what != "generic" else E.chained_channel_sums(per_c, E.dwo_bwd_input_chunk(H, W)))
        for name in ("out", "grad_input", "grad_offset"):
            rep.check(fam, name, got[name], refs.ref64[name], refs.ref32[name])
        _check_zeros_at_gated(inp, got)
    assert torch.equal(outs["full"]["grad_input"], outs["min"]["grad_input"])
    gx_s, gx_g = outs["full"]["grad_input"], outs["generic"]["grad_input"]
    assert (gx_s - gx_g).abs().max().item() <= 1e-6 * max(1.0, gx_g.abs().max().item())
    for a in ("full", "min"):
        d = (outs[a]["grad_offset"] - outs["generic"]["grad_offset"]).abs().max().item()
        assert d <= 2e-5 * max(1.0, outs["generic"]["grad_offset"].abs().max().item())
    # the shim (deform_conv) takes the full-scratch route: grad_input bit for bit
    from codenet_amd.functions.dcn_deform_conv import deform_conv
    x, off, w = (v.cuda().requires_grad_(True) for v in (inp.x, inp.off, inp.w))
    out = deform_conv(x, off, w, 1, 1, 1, C, 1)
    out.backward(inp.gout.cuda())
    assert torch.equal(x.grad, gx_s) and torch.equal(out.detach(), outs["full"]["out"])
    rep.done()


def test_print_the_largest_ratios():
    """Not a check: the largest figures seen per kernel family by the tests above (DESIGN.md section 4.4a records them)."""
    for fam, (ratio, used) in sorted(_Report.worst.items()):
        print("DCN largest | %s: err / float32 figure %.2f (comparisons with no allowance), err / bound %.2f (all)" % (fam, ratio, used))
