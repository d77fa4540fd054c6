"""The training kernels of the scale-dilated gather (codenet_stage.hip: dw_kernel, dw4_kernel, dw_bwd2_kernel,
dw_bwd2u_kernel, dw_bwd_kernel, atomic and reproducible forms) and cdn_codenet_scale_backward_masked against the plain
float64 reference of tests/gather_ref.py, through the C ABI, on scales that sit ON the edges: integers and half-integers,
both float32 neighbours of every integer, the Hardtanh bounds, s = 1 and s = 0 -- each mixed into a random background.
tests/test_gather_ref_host.py proves on the CPU that these inputs reach the edges (taps exactly on -1 and on `size`,
pixels gated down to the centre tap, 2x2 blocks whose fold breaks: the four-pass path of dw_bwd2u_kernel) and that a
continuous rule would move grad_s at every such pixel by more than 1000 x the bound of the plain float32 yardstick (300 x
that of the atomic forms' chained one).

Every output is compared as  max |got - ref64| / max |ref64|  per tensor, no element left out, against
MARGIN x the same figure of the reference evaluated in float32 on the same inputs (at least 8 float32 ulps of the
tensor's maximum): the convention of test_gpu_ctdet_loss.py.  For the sums of the atomic forms that end in float atomics
the float32 evaluation adds in chains as they do (see MARGIN).  Every comparison prints its figures (pytest -s).

Which shape runs which kernel and path: the tables FULL_CASES / UP2_CASES of tests/gather_ref.py."""
import math

import numpy as np
import pytest
import torch

from tests import gather_ref as R

pytestmark = pytest.mark.gpu

# One margin for every comparison.  What differs is the float32 evaluation it multiplies.  grad_s and grad_w of the ATOMIC
# forms end in float atomics -- a chain of float32 additions in arrival order: up to 32 lanes x 16 waves = 512 private sums
# into one LDS word and then one per image (grad_w; dw_bwd_kernel: one wave sum per 64 pixels), one per channel chunk
# (grad_s, 65 / 129 chunks at the 1032- / 1028-channel shapes) -- so their error moves from call to call.  Against
# torch.sum's PAIRWISE float32 sum they were measured at up to 12.0 x (grad_w) and 4.2 x (grad_s) over 40 calls, which
# no margin within the allowed 16 bounds safely.  Their yardstick is therefore the float32 reference summed the way they
# sum: R.chained_float32_sums, chains of the kernel's lengths in 8 seeded orders, the largest error of the 8.  Everything
# else -- d, grad_x, the reproducible forms, grad_s where one chunk holds all channels -- keeps the plain float32 reference.
MARGIN = 4.0
NAMES = ("d", "grad_x", "grad_s", "grad_w")


def _lib():
    from codenet_amd import _native as N_
    return N_, N_.lib()


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _forward(x, s, w, up2=False):
    """x, s on the device (the stored tensors for up2) -> d at full resolution."""
    N_, lib = _lib()
    N, C, H, W = x.shape
    if up2:
        H, W = 2 * H, 2 * W
    d = torch.full((N, C, H, W), float("nan"), device="cuda")
    if up2:
        N_.check(lib.cdn_codenet_dw_up2_forward(_p(x), _p(s), _p(w), _p(d), N, C, H, W, None, _stream()), "up2 forward")
    else:
        N_.check(lib.cdn_codenet_dw_forward(_p(x), _p(s), _p(w), _p(d), N, C, H, W, _stream()), "forward")
    return d


def _backward(x, s, w, gd, up2=False, fixed=False, want=(True, True, True), fill=float("nan"), joined=False):
    """One call of cdn_codenet_dw[_up2]_backward[_r]; outputs not wanted are passed as NULL.  The outputs (and the
    workspace) start dirty -- except the atomic form's grad_w, which accumulates."""
    N_, lib = _lib()
    N, C = x.shape[:2]
    H, W = gd.shape[2:]
    gx = torch.full_like(x, fill) if want[0] else None
    gs = torch.full_like(s, fill) if want[1] else None
    gw = (torch.full_like(w, fill) if fixed else torch.zeros_like(w)) if want[2] else None
    if joined:      # grad_w directly behind grad_s in one dirty buffer
        buf = torch.full((s.numel() + w.numel(),), fill, device="cuda")
        gs, gw = buf[:s.numel()].view_as(s), buf[s.numel():].view_as(w)
    args = (_p(x), _p(s), _p(w), _p(gd), _p(gx), _p(gs), _p(gw), N, C, H, W)
    if fixed:
        need = lib.cdn_codenet_dw_backward_workspace_bytes(N, C, H, W, int(up2))
        assert need > 0
        ws = torch.full((need // 4,), fill, device="cuda")
        fn = lib.cdn_codenet_dw_up2_backward_r if up2 else lib.cdn_codenet_dw_backward_r
        N_.check(fn(*args, _p(ws), _stream()), "reproducible backward")
    else:
        fn = lib.cdn_codenet_dw_up2_backward if up2 else lib.cdn_codenet_dw_backward
        N_.check(fn(*args, _stream()), "atomic backward")
    torch.cuda.synchronize()
    return gx, gs, gw


def _fixed_chunks(N, C, H, W, up2):
    """Channel chunks of the reproducible form, from its workspace: bytes / 4 = chunks * N * plane + N * C * 9."""
    _, lib = _lib()
    need = lib.cdn_codenet_dw_backward_workspace_bytes(N, C, H, W, int(up2))
    if need == 0:
        return 0
    plane = (H // 2) * (W // 2) if up2 else H * W
    chunks, rest = divmod(need // 4 - N * C * 9, N * plane)
    assert rest == 0
    return chunks


class _Report:
    """Collects the figures of one test, prints them, and fails at the end if any exceeds its bound."""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def check(self, what, name, got, ref64, ref32, margin=MARGIN):
        got = got.cpu()
        assert got.shape == ref64.shape and torch.isfinite(got).all(), (self.tag, what, name)
        err, lim = R.rel_err(got, ref64), R.bound(ref32, ref64, margin)
        e32 = R.yardstick(ref32, ref64)
        print("GATHER %s | %s %s: err %.3e  float32 reference %.3e  ratio %.2f  bound %.3e" %
              (self.tag, what, name, err, e32, err / e32 if e32 > 0 else float("inf"), lim))
        if not err <= lim:
            self.bad.append((what, name, err, lim))

    def done(self):
        assert not self.bad, (self.tag, self.bad)


def _atomic_yardsticks(x, s, w, gd, up2, r32):
    """The float32 references of the atomic forms' (grad_x, grad_s, grad_w): the plain one for grad_x, and for grad_s
    where one chunk holds every channel (one atomic into a zeroed word: nothing to order); chains of the kernel's
    lengths in 8 orders (R.chained_float32_sums) for grad_w and for grad_s over several chunks."""
    N, C = x.shape[:2]
    H, W = gd.shape[2:]
    chunk, lanes = R.atomic_plan(up2, N, C, H, W)
    chained = R.chained_float32_sums(x, s, w, gd, up2, chunk, lanes)
    several = -(-C // chunk) > 1
    return (r32[1], [c[0] for c in chained] if several else r32[2], [c[1] for c in chained]), chunk, lanes


def _run_case(tag, x, s, w, gd, up2, has_forward=True):
    """Everything the issue asks of one (shape, family): forward, atomic and reproducible backward against the reference,
    reproducibility, grad_x bit-identical between the two forms where they take one chunk, NULL-output combinations."""
    N, C = x.shape[:2]
    H, W = gd.shape[2:]
    ref_fn = R.gather_up2_ref if up2 else R.gather_ref
    r64 = ref_fn(x, s, w, gd)
    r32 = ref_fn(x, s, w, gd, dtype=torch.float32)
    a32, atomic_chunk, lanes = _atomic_yardsticks(x, s, w, gd, up2, r32)
    fixed_point = lanes > 0          # dw_bwd2_kernel / dw_bwd2u_kernel: grad_x is the order-free fixed-point sum
    xc, sc, wc, gc = (t.cuda() for t in (x, s, w, gd))
    rep = _Report(tag)
    if has_forward:
        d = _forward(xc, sc, wc, up2)
        rep.check("forward", "d", d, r64[0], r32[0])
        if up2:     # the header's promise: bit-identical to the full-resolution forward on the materialised replication
            assert torch.equal(d, _forward(R.replicate2(x).cuda(), R.replicate2(s).cuda(), wc))
    a = _backward(xc, sc, wc, gc, up2)
    for name, got, r6, r3 in zip(NAMES[1:], a, r64[1:], a32):
        rep.check("atomic", name, got, r6, r3)
    # NULL-output combinations of the atomic form: each output alone, and grad_s + grad_w in ONE buffer (grad_w right
    # behind grad_s: the library's fill of grad_s covers both, the way CodenetStageFunction calls it) -- grad_x to the bit
    # where it is the fixed-point sum, the float atomics against the reference
    for k, name in enumerate(NAMES[1:]):
        got = _backward(xc, sc, wc, gc, up2, want=tuple(i == k for i in range(3)))[k]
        if k == 0 and fixed_point:
            assert torch.equal(got, a[0])
        else:
            rep.check("atomic, alone", name, got, r64[k + 1], a32[k])
    j = _backward(xc, sc, wc, gc, up2, joined=True)
    if fixed_point:
        assert torch.equal(j[0], a[0])
    for name, got, r6, r3 in zip(NAMES[2:], j[1:], r64[2:], a32[1:]):
        rep.check("atomic, one buffer", name, got, r6, r3)
    chunks = _fixed_chunks(N, C, H, W, up2)
    if chunks:
        f1 = _backward(xc, sc, wc, gc, up2, fixed=True)
        f2 = _backward(xc, sc, wc, gc, up2, fixed=True, fill=7.0)
        for u, v in zip(f1, f2):
            assert torch.equal(u, v)
        for name, got, r6, r3 in zip(NAMES[1:], f1, r64[1:], r32[1:]):
            rep.check("fixed-order", name, got, r6, r3)
        fixed_chunk = (R.bwd2u_chunk(N, C, H, W, True) if up2 else R.bwd2_chunk(H, W, True))
        assert chunks == -(-C // fixed_chunk), (chunks, fixed_chunk)       # the chunk the shape is listed for was taken
        if fixed_chunk == atomic_chunk:
            assert torch.equal(a[0], f1[0])
        for k, name in enumerate(NAMES[1:]):                                # each output alone: the full call's to the bit
            got = _backward(xc, sc, wc, gc, up2, fixed=True, want=tuple(i == k for i in range(3)))[k]
            assert torch.equal(got, f1[k]), name
    if not up2:
        # the Python route (autograd function of ops.codenet_dw): the reproducible form where it exists
        from codenet_amd import ops
        xg, sg, wg = (t.clone().requires_grad_(True) for t in (xc, sc, wc))
        dd = ops.codenet_dw(xg, sg, wg)
        dd.backward(gc)
        rep.check("ops.codenet_dw", "d", dd.detach(), r64[0], r32[0])
        for name, t_, r6, r3 in zip(NAMES[1:], (xg, sg, wg), r64[1:], r32[1:] if chunks else a32):
            rep.check("ops.codenet_dw", name, t_.grad, r6, r3)
    rep.done()


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("case", range(len(R.FULL_CASES)), ids=["%dx%dx%dx%d-%s" % c for c in R.FULL_CASES])
def test_full_resolution_gather_on_the_edges(case, fam):
    N, C, H, W, path = R.FULL_CASES[case]
    x, w, gd = R.gather_inputs(N, C, H, W, seed=100 + case)
    s = R.family_scale_plane(fam, N, H, W, seed=H)
    _run_case("%s %s %s" % (path, (N, C, H, W), fam), x, s, w, gd, False)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("case", range(len(R.UP2_CASES)), ids=["%dx%dx%dx%d-chunk%d" % c for c in R.UP2_CASES])
def test_upsampled_gather_on_the_edges(case, fam):
    """dw_bwd2u_kernel and dw4_kernel<true>.  With fam = neighbours the blocks whose fold breaks (the four-pass path) are
    on all four axes, two at once included, in every case but the 5 x 3 stored plane of chunk 8, where no xa pair is in
    range (three axes) -- counted per case, with minima, in
    test_gather_ref_host.py::test_neighbour_scales_break_the_fold_on_every_axis_and_on_two_axes_at_once."""
    _, lib = _lib()
    N, C, H, W, chunk = R.UP2_CASES[case]
    x, w, gd = R.gather_inputs(N, C, H, W, seed=200 + case, up2=True)
    s = R.stored_scale_plane(fam, N, H // 2, W // 2, seed=H)
    has_forward = C % 4 == 0
    assert bool(lib.cdn_codenet_dw_up2_supported(N, C, H, W)) == has_forward
    assert R.atomic_plan(True, N, C, H, W)[0] == chunk
    _run_case("bwd2u<%d> %s %s" % (chunk, (N, C, H, W), fam), x, s, w, gd, True, has_forward)


@pytest.mark.parametrize("fam", R.FAMILIES)
def test_upsampled_stage_route_on_the_edges(fam):
    """The Python route of the up-sampled form: ops.codenet_dw_up2 gives the forward; its backward is reached through the
    stage function only, so the full-resolution autograd function on the materialised replication pins the pair."""
    from codenet_amd import ops
    N, C, H, W, _ = R.UP2_CASES[2]
    x, w, gd = R.gather_inputs(N, C, H, W, seed=202, up2=True)
    s = R.stored_scale_plane(fam, N, H // 2, W // 2, seed=H)
    out = ops.codenet_dw_up2(x.cuda(), s.cuda(), w.cuda(), want_range=False)
    d = out[0] if isinstance(out, tuple) else out
    xg, sg = R.replicate2(x).cuda().requires_grad_(True), R.replicate2(s).cuda().requires_grad_(True)
    dd = ops.codenet_dw(xg, sg, w.cuda())
    assert torch.equal(d, dd.detach())
    dd.backward(gd.cuda())
    r64, r32 = R.gather_up2_ref(x, s, w, gd), R.gather_up2_ref(x, s, w, gd, dtype=torch.float32)
    rep = _Report("ops route of %s %s" % ((N, C, H, W), fam))
    rep.check("ops.codenet_dw on the replication", "grad_x", R.fold2(xg.grad.cpu()), r64[1], r32[1])
    rep.check("ops.codenet_dw on the replication", "grad_s", R.fold2(sg.grad.cpu()), r64[2], r32[2])
    rep.done()


# ---- the fixed-point scale of grad_x ------------------------------------------------------------------------------------

SCALE_CASES = [(False, 0), (False, 4), (True, 2)]       # (up2, index into the case table): chunks 16, 4 and bwd2u<4>


def _scale_case(up2, idx):
    N, C, H, W, _ = (R.UP2_CASES if up2 else R.FULL_CASES)[idx]
    x, w, gd = R.gather_inputs(N, C, H, W, seed=300 + idx, up2=up2)
    s = (R.stored_scale_plane("halves", N, H // 2, W // 2, seed=3) if up2 else R.family_scale_plane("halves", N, H, W, seed=3))
    return x, s, w, gd


@pytest.mark.parametrize("up2,idx", SCALE_CASES + [(False, 7)])
def test_zero_grad_d_gives_exact_zeros(up2, idx):
    """gmax == 0: the scale falls back to 2^40 and every sum is a sum of zeros."""
    x, s, w, gd = _scale_case(up2, idx)
    xc, sc, wc, gc = x.cuda(), s.cuda(), w.cuda(), torch.zeros_like(gd).cuda()
    forms = [False] + ([True] if _fixed_chunks(x.shape[0], x.shape[1], gd.shape[2], gd.shape[3], up2) else [])
    for fixed in forms:
        for t in _backward(xc, sc, wc, gc, up2, fixed=fixed):
            assert (t == 0).all()


@pytest.mark.parametrize("up2,idx", SCALE_CASES)
def test_tiny_gradients_keep_their_precision_under_the_exponent_clamp(up2, idx):
    """grad_d * 2^-100: gmax ~ 2^-96, below the 2^-86 at which the exponent of the scale is clamped (2^126 must stay a
    finite float).  The largest contributions still carry ~30 bits, so grad_x = 2^-100 x the unscaled gradient to the
    usual bound -- not NaN (0 x inf), not flushed to zero."""
    x, s, w, gd = _scale_case(up2, idx)
    tiny = 2.0 ** -100
    ref_fn = R.gather_up2_ref if up2 else R.gather_ref
    r64 = ref_fn(x, s, w, gd)
    r32 = ref_fn(x, s, w, gd * tiny, dtype=torch.float32)
    a32 = _atomic_yardsticks(x, s, w, gd * tiny, up2, r32)[0]
    xc, sc, wc, gc = x.cuda(), s.cuda(), w.cuda(), (gd * tiny).cuda()
    rep = _Report("2^-100 %s" % ((up2, idx),))
    for fixed in (False, True):
        got = _backward(xc, sc, wc, gc, up2, fixed=fixed)
        assert got[0].abs().max().item() > 0
        for name, t, r6, r3 in zip(NAMES[1:], got, r64[1:], r32[1:] if fixed else a32):
            rep.check("fixed-order" if fixed else "atomic", name, t, r6 * tiny, r3)
    rep.done()


@pytest.mark.parametrize("power", [40, 20])
@pytest.mark.parametrize("up2,idx", SCALE_CASES)
def test_small_channels_beside_a_large_one_keep_the_documented_resolution(up2, idx, power):
    """Channel 1 of chunk 0 gets grad_d x 2^power.  The workgroup's scale follows its largest |grad_d| x |w|: a value
    v < 2^e is scattered as round(v x 2^(40 - e)), so every term of a small channel's cell is rounded to q = 2^(e - 40),
    half of it at most per term (round to nearest).  Bound of a cell of a small channel: (number of non-zero terms it
    receives, R.contribution_counts) x q / 2, plus the float32 rounding the usual bound grants.  For the up-sampled form
    (four pixels added in float32 before the conversion, gmax 4 x larger) the 2x2 sum of the counts bounds the terms.
    The large channel itself, and the chunks beside it, keep the usual bound."""
    x, s, w, gd = _scale_case(up2, idx)
    N, C = x.shape[:2]
    chunk = (R.bwd2u_chunk(N, C, gd.shape[2], gd.shape[3], False) if up2 else R.bwd2_chunk(gd.shape[2], gd.shape[3], False))
    big = 1
    gd = gd.clone()
    gd[:, big] *= 2.0 ** power
    cc = min(chunk, C)
    small = [c for c in range(cc) if c != big]
    ref_fn = R.gather_up2_ref if up2 else R.gather_ref
    r64 = ref_fn(x, s, w, gd)
    r32 = ref_fn(x, s, w, gd, dtype=torch.float32)
    cnt = R.contribution_counts(R.replicate2(s) if up2 else s)
    if up2:
        cnt = R.fold2(cnt)
    # q per image: the kernel's gmax is the float32 product of the chunk's largest |grad_d| and |w| (x 4 when folding)
    q = torch.empty(N, 1, 1, 1, dtype=torch.float64)
    for n in range(N):
        gmax = np.float32(gd[n, :cc].abs().max().item()) * (np.float32(4.0 if up2 else 1.0) * np.float32(w[:cc].abs().max().item()))
        q[n] = 2.0 ** (math.frexp(float(gmax))[1] - 40)
    usual = R.bound(r32[1][:, small], r64[1][:, small]) * r64[1][:, small].abs().max().item()
    limit = cnt.double() * q / 2 + usual                                         # [N,1,h,w], the same for every small channel
    xc, sc, wc, gc = x.cuda(), s.cuda(), w.cuda(), gd.cuda()
    rep = _Report("2^%d beside %s" % (power, (up2, idx)))
    for fixed in (False, True):
        gx = _backward(xc, sc, wc, gc, up2, fixed=fixed, want=(True, False, False))[0].cpu()
        err = (gx[:, small].double() - r64[1][:, small]).abs()
        print("GATHER 2^%d %s %s: small channels' worst error / cell bound %.3f (q/2 = %.3e, at most %d terms)" %
              (power, (up2, idx), "fixed-order" if fixed else "atomic", (err / limit).max().item(), q.max().item() / 2,
               int(cnt.max())))
        assert (err <= limit).all()
        rep.check("fixed-order" if fixed else "atomic", "grad_x of the large channel", gx[:, big], r64[1][:, big], r32[1][:, big])
        if C > cc:
            rep.check("fixed-order" if fixed else "atomic", "grad_x of the other chunks", gx[:, cc:], r64[1][:, cc:], r32[1][:, cc:])
    rep.done()


# ---- cdn_codenet_scale_backward_masked ----------------------------------------------------------------------------------

def _nextafter(v, to):
    return float(np.nextafter(np.float32(v), np.float32(to)))


@pytest.mark.parametrize("with_partials", [True, False])
@pytest.mark.parametrize("N,C,H,W", [(2, 5, 7, 9), (1, 6, 8, 8), (2, 3, 10, 10), (1, 9, 16, 20)])
def test_scale_backward_masked(N, C, H, W, with_partials):
    """grad_x += w_scale[c] * m * grad_s and the partial sums [N][C + 1] (column C: sum_p m * grad_s, the bias share) with
    m = (lo < s_clamped < hi): s_clamped exactly on lo and on hi (mask 0), one float32 step inside each (mask 1), and in
    between.  H * W = 63 (scalar path), 64, 100 and 320 (vector path: a multiple of 4, of 64, of neither 64 ...); C ragged
    against the four channels of a workgroup.  The mask must match exactly: with a zero grad_x going in, the output is
    zero precisely where the mask is."""
    N_, lib = _lib()
    lo, hi = -7.0, 8.0
    g = torch.Generator().manual_seed(N * 10 + C)
    x = torch.randn(N, C, H, W, generator=g)
    gs = torch.randn(N, 1, H, W, generator=g)
    gs[gs == 0] = 1.0
    ws = torch.randn(C, generator=g)
    ws[ws == 0] = 1.0
    gx_in = torch.randn(N, C, H, W, generator=g)
    special = torch.tensor([lo, hi, _nextafter(lo, 9), _nextafter(hi, -9), 0.5, -6.5, 7.75, lo, hi])
    sc = torch.empty(N, 1, H, W).uniform_(lo, hi, generator=g)
    pick = torch.randint(0, len(special), (N, 1, H, W), generator=g)
    sc = torch.where(torch.rand(N, 1, H, W, generator=g) < 0.7, special[pick], sc).contiguous()
    mask = (sc > lo) & (sc < hi)
    assert int((sc == lo).sum()) >= 4 and int((sc == hi).sum()) >= 4 and int(mask.sum()) >= 8
    assert int((sc == _nextafter(lo, 9)).sum()) >= 2 and int((sc == _nextafter(hi, -9)).sum()) >= 2

    def ref(dt):
        gm = gs.to(dt) * mask.to(dt)
        gxo = gx_in.to(dt) + ws.to(dt).view(1, C, 1, 1) * gm
        part = torch.cat([(x.to(dt) * gm).sum((2, 3)), gm.sum((2, 3))], 1)
        return gxo, part

    r64, r32 = ref(torch.float64), ref(torch.float32)

    xc, gsc, scc, wsc = x.cuda(), gs.cuda(), sc.cuda(), ws.cuda()

    def run(gx0):
        gx = gx0.clone().cuda()
        part = torch.full((N, C + 1), float("nan"), device="cuda") if with_partials else None
        rc = lib.cdn_codenet_scale_backward_masked(_p(xc), _p(gsc), _p(scc), lo, hi, _p(wsc), _p(gx), _p(part), N, C, H, W,
                                                   _stream())
        N_.check(rc, "cdn_codenet_scale_backward_masked")
        torch.cuda.synchronize()
        return gx, part

    rep = _Report("scale_backward_masked %s" % ((N, C, H, W),))
    gx, part = run(gx_in)
    rep.check("masked", "grad_x", gx, r64[0], r32[0])
    if with_partials:
        rep.check("masked", "partials", part, r64[1], r32[1])
    gz, _ = run(torch.zeros_like(gx_in))
    assert torch.equal(gz.cpu() != 0, mask.expand(N, C, H, W))
    rep.done()
