"""The QuantAct element kernels of codenet_amd/csrc/codenet_quant.hip and the one-thread update they share
(cdn::quantact_update_device, cdn_common.h), called directly at tails, rounding ties, stale-state sequences and
degenerate ranges.  Every comparison is an equality: forward quantities against oracle/quant.py (CPU, float32, the
reference's expression order), gradients against the CPU module path (nn.ReLU, nn.Upsample(2, "nearest")).  Where NaNs
are expected, equality is the same NaN mask plus torch.equal on the rest; state words [2..6] are compared as raw words.

Sizes, from the launch arithmetic of codenet_quant.hip (kCUs = 256, 256 threads per workgroup, one float4 per thread):

  minmax_grid(n) = min(ceil(max(n >> 2, 1) / 1024), 512) workgroups, stride = 256 * grid threads.  A thread runs the
      4-way unrolled loop while i + 3 * stride < (n >> 2), then the remainder loop, then the scalar tail of n & 3.
        n = 1, 2, 3       no float4 at all: only the tail loop
        n = 5, 7          one float4 (remainder loop) + tail 1 / 3
        n = 1023, 1025    255 / 256 float4 in the remainder loop (256 + 768 > n >> 2) + tail 3 / 1
        n = 4099          1024 float4 = exactly one pass of the unrolled loop of one workgroup + tail 3
        n_big = 2^21 + 2^19 + 3 = 2 621 443: 640 > 512 workgroups wanted, so the cap holds: stride 131 072, n >> 2 =
            655 360 = 5 strides = one unrolled pass over floats [0, 2 097 152), one remainder pass over floats
            [2 097 152, 2 621 440), tail of 3 (test_constructions re-derives this).
  stream_grid(n) = min(ceil(max(n >> 2, 1) / 256), 2048) workgroups = 524 288 threads: n_big has 655 360 float4, so the
      grid-stride loops of fake_quant_kernel, relu_fq_kernel and relu_bwd_kernel wrap once.
  relu_fq_up2_kernel / up2_relu_bwd_kernel: one thread per pair of columns, min(ceil(planes * H * ceil(W / 2) / 256),
      4096) workgroups = 1 048 576 threads.  Odd W: the scalar path with a lone last column (W = 1, 3, 9); even W: the
      16-byte path (W = 2, 6, 10 and W = 4, 16); H = 1 included; 8 x 512 x 514 has 4096 * 257 = 1 052 672 pairs, so the
      grid-stride loop wraps (8.4 MB in, 34 MB out).  The range passes also see n_big as 1 x 1 x n_big (42 MB out).
  quantact_update_kernel: 256 threads reduce the pairs with stride 256, so 1, 63, 255, 256, 257 and 1000 pairs put the
      extremes in a lone thread, the last thread of the first pass, the first thread of the second pass and a thread
      in its fourth pass.

Aliasing: include/codenet_dcn.h allows out to alias x for cdn_quantact_forward; cdn_quantact_forward_partials is
declared there as that call with the extremes taken from the pairs.  Both are run in place.
"""
import pytest
import torch

from oracle import quant as Q

SMALL = [1, 2, 3, 5, 7, 1023, 1025, 4099]
N_BIG = 2 ** 21 + 2 ** 19 + 3
UP_SHAPES = [(3, 1, 1), (2, 3, 3), (5, 2, 9), (3, 1, 2), (2, 5, 6), (1, 3, 10), (7, 2, 4), (2, 3, 16)]
UP_BIG = (8, 512, 514)
TIE_RANGE = (0.0, 31.875)
PAIR_COUNTS = [1, 63, 255, 256, 257, 1000]
K_CUS, WG = 256, 256


# ---- launch arithmetic of codenet_quant.hip, restated (test_constructions checks the sizes against it) ------------

def minmax_grid(n):
    return min(-(-max(n >> 2, 1) // (WG * 4)), 2 * K_CUS)


def stream_grid(n):
    return min(-(-max(n >> 2, 1) // WG), 8 * K_CUS)


def up2_grid(planes, H, W):
    return min(-(-planes * H * ((W + 1) // 2) // WG), 16 * K_CUS)


def minmax_regions(n):
    """Floats covered by the unrolled loop, by the remainder loop and by the tail of minmax_kernel (whole strides at
    the sizes used here, so every thread of the grid makes the same passes)."""
    n4, stride = n >> 2, minmax_grid(n) * WG
    i = 0
    while i + 3 * stride < n4:
        i += 4 * stride
    return 4 * min(i, n4), 4 * (n4 - min(i, n4)), n - 4 * n4


def sweep_positions(n):
    """Where a lone extreme (or NaN) goes: index 0, the .w lane, the last element of the last float4, the first tail
    element, the last element and, for n_big, one index inside each of the three regions."""
    n4 = n >> 2
    pos = [0, 3, 4 * n4 - 1, 4 * n4, n - 1]
    if n == N_BIG:
        pos += [1_000_003, 2 ** 21 + 100_001, n - 2]
    out = []
    for p in pos:
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


# ---- references ---------------------------------------------------------------------------------------------------

class Given(Q.QuantActState):
    """The oracle with the batch extremes handed in (the partials / external-extremes / commit paths)."""
    def batch_stats(self, x, percentile=False):
        return self.given


def f32(v):
    return torch.tensor([v], dtype=torch.float32)


def wide_flag(bits, scale, zp, extremes):
    """State word [6] as cdn_common.h documents it: 1 when the codes of this batch cannot be carried by the int8
    kernels or nobody knows the batch extremes."""
    if bits != 8 or extremes is None:
        return 1
    for b in extremes:
        level = torch.round(scale * b - zp) + (zp - 128.0)
        if bool(torch.isnan(level).any()) or bool((level.abs() > 2039.0).any()):
            return 1
    return 0 if bool((zp.abs() < 4.0e6).all()) else 1


def same(a, b):
    """Equality where NaNs may stand: the same NaN mask and torch.equal on the rest."""
    a, b = a.reshape(-1), b.reshape(-1)
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def same_words(a, b):
    """Raw 32-bit equality of float words; a NaN (whose payload is nobody's contract) matches any NaN."""
    a, b = a.reshape(-1), b.reshape(-1)
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def relu_ref(y):
    return torch.relu(y)


def special_y(n, g):
    """Pre-ReLU values with every case of the threshold: positive, negative, 0.0, -0.0, a positive denormal, +inf, NaN --
    counted from the END, so that the last element (the scalar tail, the lone last column) is the NaN at every n."""
    y = torch.randn(n, generator=g)
    idx = (n - 1 - torch.arange(n)) % 11
    for k, v in enumerate([float("nan"), -0.0, 0.0, 1e-42, -1.0, float("inf")]):
        y[idx == k] = v
    return y


def wide_g(shape, g):
    return torch.randn(shape, generator=g) * torch.exp(3.0 * torch.randn(shape, generator=g))


# ---- the device side ----------------------------------------------------------------------------------------------

def _p(t):
    return t.data_ptr() if t is not None else None


class Dev:
    """One QuantAct on the device: its range, its 8-word state, and the entry points that touch them."""

    def __init__(self, bits=8, momentum=0.99, x_min=0.0, x_max=0.0):
        from codenet_amd import _native, ops
        self.N_, self.ops, self.lib = _native, ops, _native.lib()
        self.activation_bit, self.momentum = bits, momentum
        self.x_min = torch.full((1,), x_min, device="cuda")
        self.x_max = torch.full((1,), x_max, device="cuda")
        self.state = ops.quantact_state("cuda")

    def _device_state(self, device):             # (what ops.quantact_apply / quantact_forward_partials ask of an act)
        return self.state

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def _tail(self, running):
        return (int(self.activation_bit), float(self.momentum), int(bool(running)))

    def reset_range(self):
        self.x_min.zero_()
        self.x_max.zero_()

    def forward(self, x, running=True, want_out=True, want_codes=False, bmin=None, bmax=None):
        return self.ops.quantact_forward(x, self.x_min, self.x_max, self.state, bits=self.activation_bit,
                                         momentum=self.momentum, running=running, batch_min=bmin, batch_max=bmax,
                                         want_codes=want_codes, want_out=want_out)

    def forward_inplace(self, x, running=True):
        rc = self.lib.cdn_quantact_forward(_p(x), _p(x), None, x.numel(), _p(self.x_min), _p(self.x_max), _p(self.state),
                                           None, None, *self._tail(running), self._stream())
        self.N_.check(rc, "cdn_quantact_forward")
        return x

    def forward_partials(self, x, partials, out=None, running=True, snap=None):
        rc = self.lib.cdn_quantact_forward_partials(_p(x), _p(out), x.numel() if x is not None else 0, _p(self.x_min),
                                                    _p(self.x_max), _p(self.state), _p(partials), partials.shape[0],
                                                    *self._tail(running), _p(snap), self._stream())
        self.N_.check(rc, "cdn_quantact_forward_partials")
        return out

    def head_update(self, partials, running=True, relu=False, snap=None):
        rc = self.lib.cdn_codenet_head_act_update(_p(self.x_min), _p(self.x_max), _p(self.state), _p(partials),
                                                  partials.shape[0] if partials is not None else 0, *self._tail(running),
                                                  int(bool(relu)), _p(snap), self._stream())
        self.N_.check(rc, "cdn_codenet_head_act_update")

    def relu_forward(self, y, partials=None, running=True):
        out = torch.empty_like(y)
        rc = self.lib.cdn_quantact_relu_forward(_p(y), _p(out), y.numel(), _p(self.x_min), _p(self.x_max), _p(self.state),
                                                _p(partials), partials.shape[0] if partials is not None else 0,
                                                *self._tail(running), self._stream())
        self.N_.check(rc, "cdn_quantact_relu_forward")
        return out

    def relu_up2_forward(self, y, partials=None, running=True):
        P, H, W = y.shape
        out = torch.empty(P, 2 * H, 2 * W, device=y.device)
        if partials is None:
            rc = self.lib.cdn_quantact_relu_up2_forward(_p(y), _p(out), P, H, W, _p(self.x_min), _p(self.x_max),
                                                        _p(self.state), *self._tail(running), self._stream())
        else:
            rc = self.lib.cdn_quantact_relu_up2_forward_partials(_p(y), _p(out), P, H, W, _p(self.x_min), _p(self.x_max),
                                                                 _p(self.state), _p(partials), partials.shape[0],
                                                                 *self._tail(running), self._stream())
        self.N_.check(rc, "cdn_quantact_relu_up2_forward[_partials]")
        return out

    def commit(self, rng, running=True):
        rc = self.lib.cdn_quantact_commit_range(_p(self.x_min), _p(self.x_max), _p(self.state), _p(rng),
                                                *self._tail(running), self._stream())
        self.N_.check(rc, "cdn_quantact_commit_range")

    def apply(self, x):
        return self.ops.quantact_apply(x, self)

    def relu_apply(self, y, up):
        P, H, W = y.shape
        out = torch.empty((P, 2 * H, 2 * W) if up else (P, H, W), device=y.device)
        rc = self.lib.cdn_quantact_relu_apply(_p(y), _p(out), P, H, W, int(up), _p(self.state), self._stream())
        self.N_.check(rc, "cdn_quantact_relu_apply")
        return out

    # -- checks ---------------------------------------------------------------------------------------------------
    def words(self):
        return self.state.cpu()

    def check(self, st, extremes, what="", raw_extremes=True, snap=None):
        """Range, words [2..6] and the zero words against the oracle state `st`; extremes: this batch's (min, max)
        as the call knew them, None when it knew none (then words [4], [5] are not looked at)."""
        w = self.words()
        f = w.view(torch.float32)
        assert w[0].item() == 0 and w[1].item() == 0 and w[7].item() == 0, (what, w.tolist())
        assert same(self.x_min.cpu(), st.x_min) and same(self.x_max.cpu(), st.x_max), \
            (what, self.x_min.item(), self.x_max.item(), st.x_min.item(), st.x_max.item())
        scale, zp = Q.act_params(st.x_min, st.x_max, st.bits)
        assert same_words(f[2:3], scale) and same_words(f[3:4], zp), (what, f[2].item(), f[3].item(), scale.item(), zp.item())
        if extremes is not None:
            ext = torch.stack([e.reshape(()) for e in extremes]).float()
            assert (same_words if raw_extremes else same)(f[4:6], ext), (what, f[4:6].tolist(), ext.tolist())
        assert w[6].item() == wide_flag(st.bits, scale, zp, extremes), (what, w[6].item())
        if snap is not None:
            s = snap.cpu()
            assert torch.equal(s[2:7], w[2:7]) and s[0].item() == 0 and s[1].item() == 0 and s[7].item() == 0, (what, s.tolist())


def replicas(out, P, H, W):
    """The four replicas of a 2 x nearest up-sampled [P, 2H, 2W] tensor, each [P, H, W]."""
    o = out.view(P, H, 2, W, 2)
    return [o[:, :, i, :, j] for i in (0, 1) for j in (0, 1)]


RANGE_KINDS = ["forward", "relu", "relu_up2"]


def range_call(dev, kind, x):
    """One running call with a range pass over x (flat, on the device); returns the output (flat; for the
    up-sampling form its four replicas, each flat)."""
    if kind == "forward":
        return [dev.forward(x)[0]]
    if kind == "relu":
        return [dev.relu_forward(x)]
    out = dev.relu_up2_forward(x.view(1, 1, -1))
    return [r.reshape(-1) for r in replicas(out, 1, 1, x.numel())]


def range_input(kind, x):
    """What the oracle's QuantAct sees: the tensor itself or its ReLU."""
    return x if kind == "forward" else relu_ref(x)


# ---- 0. the constructions, on the CPU -------------------------------------------------------------------------------

def test_constructions():
    """The properties the GPU cases rely on, so that none passes by being dead."""
    # ties: scale 8, zero point 128, every scale * x - zp an exact tie, every code even
    st = Q.QuantActState(x_min=TIE_RANGE[0], x_max=TIE_RANGE[1])
    scale, zp = Q.act_params(st.x_min, st.x_max, 8)
    assert scale.item() == 8.0 and zp.item() == 128.0
    x = tie_input()
    t = scale * x - zp
    assert torch.equal(t - torch.floor(t), torch.full_like(t, 0.5))
    q = Q.act_codes(x, scale, zp)
    assert torch.equal(torch.remainder(q, 2.0), torch.zeros_like(q))
    assert q.min().item() < -128 and q.max().item() > 127            # most codes are outside the int8 range
    assert not torch.equal(q, torch.floor(t + 0.5))                    # round-half-up differs on them
    # sizes: every small n has a tail, both vector loops of the range pass occur, n_big is the three regions stated
    assert all(n & 3 for n in SMALL) and N_BIG & 3 == 3
    assert minmax_regions(4099) == (4096, 0, 3) and minmax_regions(1025) == (0, 1024, 1)
    assert minmax_regions(1023) == (0, 1020, 3) and minmax_regions(3) == (0, 0, 3)
    assert -(-(N_BIG >> 2) // (WG * 4)) > 2 * K_CUS and minmax_grid(N_BIG) == 2 * K_CUS          # the cap holds
    stride = minmax_grid(N_BIG) * WG
    assert stride == 131072 and (N_BIG >> 2) == 5 * stride
    assert minmax_regions(N_BIG) == (2097152, 524288, 3)
    for p, lo, hi in zip(sweep_positions(N_BIG)[-3:], (0, 2097152, 2621440), (2097152, 2621440, N_BIG)):
        assert lo <= p < hi
    # the streaming kernels wrap their capped grid at n_big and at no small n
    assert stream_grid(N_BIG) == 8 * K_CUS and (N_BIG >> 2) > stream_grid(N_BIG) * WG
    assert all((n >> 2) <= stream_grid(n) * WG for n in SMALL)
    # the up-sampling kernels: both paths, and the big shape wraps the grid
    assert {W & 1 for _, _, W in UP_SHAPES} == {0, 1} and any(H == 1 for _, H, _ in UP_SHAPES)
    P, H, W = UP_BIG
    assert up2_grid(P, H, W) == 16 * K_CUS and P * H * ((W + 1) // 2) > 16 * K_CUS * WG == 1048576
    assert all(p * h * ((w + 1) // 2) <= up2_grid(p, h, w) * WG for p, h, w in UP_SHAPES)
    # the pair counts straddle the 256 threads of the update kernel
    assert {1, 255, 256, 257} <= set(PAIR_COUNTS) and max(PAIR_COUNTS) > 3 * WG
    # a constant tensor restarts from the "+=" branch: (2.5, 2.5), then (5, 5), output 2.5, codes beyond int16
    st = Q.QuantActState()
    c = torch.full((7,), 2.5)
    out, q = st(c, return_codes=True)
    assert (st.x_min.item(), st.x_max.item()) == (2.5, 2.5) and torch.equal(out, c)
    out, q = st(c, return_codes=True)
    assert (st.x_min.item(), st.x_max.item()) == (5.0, 5.0) and torch.equal(out, c)
    assert torch.equal(q, torch.full((7,), -6.375e12))
    # an all-negative tensor behind a ReLU stays at (0, 0); +inf gives x_max = inf, then NaN
    st = Q.QuantActState()
    st(torch.relu(-torch.rand(5) - 1))
    assert (st.x_min.item(), st.x_max.item()) == (0.0, 0.0)
    st = Q.QuantActState()
    xi = torch.tensor([-1.0, float("inf"), 2.0])
    assert torch.isnan(st(xi)).all() and st.x_max.item() == float("inf")
    assert torch.isnan(st(xi)).all() and torch.isnan(st.x_max).all()
    # ReLU backward of torch: y <= 0 ? 0 : g, so the gradient passes at a NaN
    y = torch.tensor([float("nan"), -0.0, 0.0, 1e-42, -1.0, float("inf")], requires_grad=True)
    torch.relu(y).backward(torch.full((6,), 3.0))
    assert y.grad.tolist() == [3.0, 0.0, 0.0, 3.0, 0.0, 3.0]
    # torch's CPU nearest up-sampling backward sums the replicas as ((a + b) + c) + d in row-major order
    g = torch.Generator().manual_seed(5)
    told_apart = False
    for P, H, W in UP_SHAPES[:5]:
        go = wide_g((1, P, 2 * H, 2 * W), g)
        yy = torch.randn(1, P, H, W, generator=g).requires_grad_(True)
        torch.nn.Upsample(scale_factor=2, mode="nearest")(yy).backward(go)
        a, b, c, d = replicas(go.view(P, 2 * H, 2 * W), P, H, W)
        assert torch.equal(yy.grad.view(P, H, W), ((a + b) + c) + d)
        told_apart |= not torch.equal(((a + b) + c) + d, ((c + d) + a) + b)
    assert told_apart                                                  # (another order gives other sums on this data)


def tie_input():
    k = torch.arange(-300, 601, dtype=torch.float32)            # 901 values: a tail of one
    return (k + 0.5) / 8.0


# ---- 1. range pass --------------------------------------------------------------------------------------------------

def _sweep_base(n, kind, g):
    x = torch.rand(n, generator=g) * 2.0 - 1.0
    # behind a ReLU the minimum of the same data would always be 0: shift it so that both extremes stay informative
    return x if kind == "forward" else x + 6.0


def _sweep(kind, sizes):
    g = torch.Generator().manual_seed(11)
    dev = Dev()
    for n in sizes:
        base = _sweep_base(n, kind, g)
        lo, hi = (-5.0, 7.0) if kind == "forward" else (1.0, 13.0)
        pos = sweep_positions(n)
        cases = [(pos[i], pos[(i + 1) % len(pos)]) for i in range(len(pos))] if n > 1 else [(0, 0)]
        for pmin, pmax in cases:
            x = base.clone()
            x[pmin] = lo
            x[pmax] = hi                        # (n = 1: the one element is both extremes)
            st = Q.QuantActState()
            xin = range_input(kind, x)
            ref = st(xin)
            dev.reset_range()
            outs = range_call(dev, kind, x.cuda())
            dev.check(st, (xin.min(), xin.max()), (kind, n, pmin, pmax), raw_extremes=False)
            for o in outs:
                assert torch.equal(o.cpu(), ref), (kind, n, pmin, pmax)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", RANGE_KINDS)
def test_range_pass_finds_a_lone_extreme_everywhere_small(kind):
    """One unique minimum and one unique maximum moved over the lanes, the last float4, the tail; ONE state tensor for
    the whole sweep (only x_min / x_max are reset), so a word [0], [1] or [7] left behind by one case spoils the next."""
    _sweep(kind, SMALL)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", RANGE_KINDS)
def test_range_pass_finds_a_lone_extreme_everywhere_big(kind):
    """The same at n_big: unrolled pass, remainder pass, tail, with the grid at its cap."""
    _sweep(kind, [N_BIG])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", RANGE_KINDS)
@pytest.mark.parametrize("n", [7, 4099])
def test_range_pass_narrower_second_batch(kind, n):
    """wide, narrow, wide on one QuantAct: a batch extreme that survived a call would widen the narrow step."""
    g = torch.Generator().manual_seed(12 + n)
    dev, st = Dev(), Q.QuantActState()
    for it, amp in enumerate((4.0, 0.5, 3.0)):
        x = (torch.rand(n, generator=g) * 2.0 - 1.0) * amp + (0.0 if kind == "forward" else 0.25 * amp)
        xin = range_input(kind, x)
        ref = st(xin)
        outs = range_call(dev, kind, x.cuda())
        dev.check(st, (xin.min(), xin.max()), (kind, n, it), raw_extremes=False)
        for o in outs:
            assert torch.equal(o.cpu(), ref), (kind, n, it)


def _nans():
    return torch.tensor([0x7fc00000, -0x400000, 0x7f800001], dtype=torch.int32).view(torch.float32)     # +qNaN, -qNaN, sNaN


def _nan_sweep(kind, n):
    g = torch.Generator().manual_seed(13)
    dev = Dev()
    base = _sweep_base(n, kind, g)
    pos = sweep_positions(n)
    for p in (1, 2, 4 * (n >> 2) - 2):          # both lanes of a compared pair: .x and .y, .z and .w
        if 0 <= p < n and p not in pos:
            pos.append(p)
    nans = _nans()
    for i, p in enumerate(pos):
        x = base.clone()
        x[p] = nans[i % 3]
        st = Q.QuantActState()
        xin = range_input(kind, x)
        assert torch.isnan(st(xin)).all() and torch.isnan(st.x_min).all() and torch.isnan(st.x_max).all()
        dev.reset_range()
        outs = range_call(dev, kind, x.cuda())
        dev.check(st, (xin.min(), xin.max()), (kind, n, p), raw_extremes=False)
        for o in outs:
            assert bool(torch.isnan(o).all().item()), (kind, n, p)
    # and the poisoned range stays poisoned through a clean batch
    st(range_input(kind, base))
    outs = range_call(dev, kind, base.cuda())
    dev.check(st, (range_input(kind, base).min(), range_input(kind, base).max()), (kind, n, "after"), raw_extremes=False)
    assert all(bool(torch.isnan(o).all().item()) for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", RANGE_KINDS)
@pytest.mark.parametrize("n", [3, 7, 1025, 4099, N_BIG])
def test_range_pass_keeps_a_lone_nan(kind, n):
    """One NaN (either sign, quiet or signalling) anywhere: both ranges NaN as the oracle's, the output NaN throughout;
    with the ReLU in front the NaN stays."""
    _nan_sweep(kind, n)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["relu", "relu_up2"])
@pytest.mark.parametrize("n", [5, 1025])
def test_relu_range_of_all_negative_batches_stays_zero(kind, n):
    """All-negative twice, then mixed: (0, 0), (0, 0), then the "+=" initialisation from the third batch; then a tensor
    of mixed -0.0 and 0.0 on a fresh QuantAct."""
    g = torch.Generator().manual_seed(14 + n)
    dev, st = Dev(), Q.QuantActState()
    for it in range(3):
        x = -torch.rand(n, generator=g) - 0.5 if it < 2 else torch.randn(n, generator=g) * 2.0
        xin = relu_ref(x)
        ref = st(xin)
        outs = range_call(dev, kind, x.cuda())
        if it < 2:
            assert (st.x_min.item(), st.x_max.item()) == (0.0, 0.0)
        dev.check(st, (xin.min(), xin.max()), (kind, n, it), raw_extremes=False)
        for o in outs:
            assert torch.equal(o.cpu(), ref), (kind, n, it)
    dev, st = Dev(), Q.QuantActState()
    x = torch.zeros(n)
    x[::2] = -0.0
    for it in range(2):
        ref = st(relu_ref(x))
        outs = range_call(dev, kind, x.cuda())
        dev.check(st, (f32(0.0), f32(0.0)), (kind, n, "zeros", it), raw_extremes=False)
        for o in outs:
            assert torch.equal(o.cpu(), ref)


# ---- 2. fake-quantisation -------------------------------------------------------------------------------------------

def _int16(q):
    return torch.clamp(q, -32768.0, 32767.0)


def _frozen_dev_and_oracle(lo, hi, bits=8):
    """A QuantAct with a given range whose device state holds the parameters (a running = 0 call derives them)."""
    dev, st = Dev(bits=bits, x_min=lo, x_max=hi), Q.QuantActState(bits=bits, x_min=lo, x_max=hi)
    dev.forward(torch.zeros(4, device="cuda"), running=False, want_out=False)
    dev.check(st, None, "frozen")
    return dev, st


@pytest.mark.gpu
def test_fake_quant_rounds_ties_to_even():
    """Range (0, 31.875): scale 8, zero point 128, x = (k + 0.5) / 8 -- every code is an exact tie, most of them outside
    [-128, 127] (not clamped).  roundf, or scale * x - zp contracted into one fma, gives other codes."""
    x = tie_input()
    dev, st = _frozen_dev_and_oracle(*TIE_RANGE)
    ref, q = st(x, running=False, return_codes=True)
    assert torch.equal(torch.remainder(q, 2.0), torch.zeros_like(q))
    xd = x.cuda()
    out, codes = dev.forward(xd, running=False, want_codes=True)
    assert torch.equal(codes.cpu().float(), q) and torch.equal(out.cpu(), ref)
    assert torch.equal(dev.apply(xd).cpu(), ref)
    # behind the ReLU: negative x become 0 (code -128, no tie), positive x keep their ties
    rref = st(relu_ref(x), running=False)
    assert torch.equal(dev.relu_forward(xd, running=False).cpu(), rref)
    assert torch.equal(dev.relu_apply(xd.view(1, 1, -1), 0).cpu().view(-1), rref)
    for P, H, W in ((1, 17, 53), (1, 30, 30)):               # the scalar and the 16-byte path of the up-sampling kernel
        y = xd[:P * H * W].view(P, H, W).contiguous()
        for out in (dev.relu_up2_forward(y, running=False), dev.relu_apply(y, 1)):
            for r in replicas(out, P, H, W):
                assert torch.equal(r.cpu().reshape(-1), rref[:P * H * W])


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL + [N_BIG])
def test_fake_quant_tails_wrap_and_aliasing(n):
    """Outputs and int16 codes of every element -- the scalar tail, the wrapped grid at n_big -- through every entry
    point of fake_quant_kernel and relu_fq_kernel; out aliasing x where the header allows it."""
    g = torch.Generator().manual_seed(21 + n % 97)
    x = torch.randn(n, generator=g) * 3.0
    xd = x.cuda()
    dev, st = Dev(), Q.QuantActState()
    ref, q = st(x, return_codes=True)
    out, codes = dev.forward(xd, want_codes=True)
    dev.check(st, (x.min(), x.max()), ("forward", n), raw_extremes=False)
    assert torch.equal(out.cpu(), ref) and torch.equal(codes.cpu().float(), _int16(q))
    _, codes = dev.forward(xd, running=False, want_out=False, want_codes=True)           # codes alone
    assert torch.equal(codes.cpu().float(), _int16(q))
    assert torch.equal(dev.apply(xd).cpu(), ref)
    # in place: cdn_quantact_forward (second running call of this act) and cdn_quantact_forward_partials
    x2 = torch.randn(n, generator=g)
    ref2 = st(x2)
    assert torch.equal(dev.forward_inplace(x2.cuda()).cpu(), ref2)
    dev.check(st, (x2.min(), x2.max()), ("in place", n), raw_extremes=False)
    x3 = torch.randn(n, generator=g) * 2.0
    part = torch.stack([x3.min(), x3.max()]).view(1, 2).cuda()
    ref3 = st(x3)
    x3d = x3.cuda()
    assert torch.equal(dev.forward_partials(x3d, part, out=x3d).cpu(), ref3)
    dev.check(st, (x3.min(), x3.max()), ("in place, partials", n))
    # behind the ReLU, on the state the calls above left
    rref = st(relu_ref(x), running=False)
    assert torch.equal(dev.relu_apply(xd.view(1, 1, -1), 0).cpu().view(-1), rref)
    assert torch.equal(dev.relu_forward(xd, running=False).cpu(), rref)
    rref = st(relu_ref(x))
    assert torch.equal(dev.relu_forward(xd).cpu(), rref)
    dev.check(st, (relu_ref(x).min(), relu_ref(x).max()), ("relu", n), raw_extremes=False)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [2, 3, 4, 8, 16])
def test_fake_quant_bit_widths(bits):
    """Three running calls per width, the second narrower than the first: ranges, outputs and int16 codes (saturated
    where the unclamped code leaves int16, as at 16 bits outside the tracked range)."""
    g = torch.Generator().manual_seed(30 + bits)
    dev, st = Dev(bits=bits), Q.QuantActState(bits=bits)
    for it, amp in enumerate((3.0, 0.7, 5.0)):
        x = torch.randn(1027, generator=g) * amp + 0.3 * it
        ref, q = st(x, return_codes=True)
        out, codes = dev.forward(x.cuda(), want_codes=True)
        dev.check(st, (x.min(), x.max()), (bits, it), raw_extremes=False)
        assert torch.equal(out.cpu(), ref) and torch.equal(codes.cpu().float(), _int16(q)), (bits, it)
        rref = st(relu_ref(x), running=False)
        assert torch.equal(dev.relu_apply(x.cuda().view(1, 1, -1), 0).cpu().view(-1), rref), (bits, it)


@pytest.mark.gpu
def test_constant_tensor_restarts_the_range_and_saturates_int16():
    """2.5 everywhere: x_min == x_max after the first call, so the second takes the "+=" branch again: (2.5, 2.5), then
    (5, 5); the output stays 2.5 and the second call's codes, -6.375e12, saturate the int16 output."""
    x = torch.full((1025,), 2.5)
    dev, st = Dev(), Q.QuantActState()
    for it, rng in enumerate(((2.5, 2.5), (5.0, 5.0))):
        ref, q = st(x, return_codes=True)
        assert (st.x_min.item(), st.x_max.item()) == rng and torch.equal(ref, x)
        out, codes = dev.forward(x.cuda(), want_codes=True)
        dev.check(st, (x.min(), x.max()), ("constant", it))
        assert torch.equal(out.cpu(), ref) and torch.equal(codes.cpu().float(), _int16(q))
    assert q[0].item() == f32(-6.375e12).item() and codes[0].item() == -32768


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["zeros", "signed zeros", "inf"])
def test_degenerate_and_non_finite_inputs(case):
    """Two calls each: zeros and mixed +-0.0 keep the range (0, 0); one +inf gives x_max = inf, then NaN, all outputs
    NaN both times."""
    n = 1027
    if case == "inf":
        x = torch.randn(n, generator=torch.Generator().manual_seed(41))
        x[n - 2] = float("inf")
    else:
        x = torch.zeros(n)
        if case == "signed zeros":
            x[1::3] = -0.0
    dev, st = Dev(), Q.QuantActState()
    for it in range(2):
        ref, q = st(x, return_codes=True)
        out, codes = dev.forward(x.cuda(), want_codes=True)
        dev.check(st, (x.min(), x.max()), (case, it), raw_extremes=False)
        assert same(out.cpu(), ref), (case, it)
        ok = ~torch.isnan(q)                         # (a NaN code has no int16 image)
        assert torch.equal(codes.cpu().float()[ok], _int16(q)[ok]), (case, it)
        if case == "inf":
            assert torch.isnan(ref).all() and (it == 0) == (st.x_max.item() == float("inf"))
        else:
            assert (st.x_min.item(), st.x_max.item()) == (0.0, 0.0) and torch.equal(ref, torch.zeros(n))


def _up_case(P, H, W, on_device):
    g = torch.Generator().manual_seed(50 + W + 16 * H)
    dev, st = Dev(), Q.QuantActState()
    eq = (lambda a, b: torch.equal(a, b)) if on_device else (lambda a, b: torch.equal(a.cpu(), b))
    for it, amp in enumerate((2.0, 0.6)):
        y = torch.randn(P, H, W, generator=g) * amp
        ref = st(relu_ref(y))
        yd = y.cuda()
        out = dev.relu_up2_forward(yd)
        dev.check(st, (relu_ref(y).min(), relu_ref(y).max()), ("up2", P, H, W, it), raw_extremes=False)
        ref = ref.cuda() if on_device else ref               # (the 34 MB output is compared where it lies)
        for r in replicas(out, P, H, W):
            assert eq(r, ref), ("up2", P, H, W, it)
        for r in replicas(dev.relu_apply(yd, 1), P, H, W):         # the apply form on the state that call left
            assert eq(r, ref), ("apply", P, H, W, it)
    # a NaN and a -0.0 in y, through the apply form: what ReLU -> QuantAct (frozen) -> Upsample gives them
    y = y.clone().view(-1)
    y[0], y[-1] = -0.0, float("nan")
    if y.numel() > 2:
        y[y.numel() // 2] = float("nan")
    y = y.view(P, H, W)
    ref = st(relu_ref(y), running=False)
    assert torch.isnan(ref.view(-1)[-1]) and int(torch.isnan(ref).sum()) <= 2
    for r in replicas(dev.relu_apply(y.cuda(), 1), P, H, W):
        assert same(r.cpu(), ref), ("apply, NaN", P, H, W)


@pytest.mark.gpu
@pytest.mark.parametrize("P,H,W", UP_SHAPES)
def test_relu_fake_quant_upsample_replicas(P, H, W):
    """The four replicas are identical and equal the oracle on relu(y): odd widths (scalar path, lone last column),
    even widths (16-byte path), H = 1."""
    _up_case(P, H, W, False)


@pytest.mark.gpu
def test_relu_fake_quant_upsample_replicas_wrapped_grid():
    """8 x 512 x 514: more column pairs than the capped grid has threads."""
    _up_case(*UP_BIG, True)


# ---- 3. update from given extremes ----------------------------------------------------------------------------------

def _pairs(n, pmin, pmax, lo, hi, g):
    p = torch.stack([-torch.rand(n, generator=g), torch.rand(n, generator=g)], dim=1)
    p[pmin, 0] = lo
    p[pmax, 1] = hi
    return p


UPDATE_KINDS = ["partials", "head", "head relu", "relu", "relu_up2"]


def _update_from_pairs(dev, st, kind, pairs, extremes, running=True, what=""):
    """One update of `dev` from the pairs through entry point `kind`, the oracle step from `extremes`, and the check."""
    relu = kind in ("head relu", "relu", "relu_up2")
    given = tuple(torch.clamp(e, min=0.0) for e in extremes) if relu else tuple(extremes)
    st.given = given
    y = torch.tensor([0.5, -1.0, 3.0, 0.0, 2.0, -0.25, 1.0])
    yin = relu_ref(y) if relu else y
    ref = st(yin, running=running)
    pd, yd = pairs.cuda(), y.cuda()
    snap, known = None, given
    if kind == "partials":
        snap = torch.full((8,), -1, dtype=torch.int32, device="cuda")
        if running:                                        # (the wrapper is the running form)
            out, snap = dev.ops.quantact_forward_partials(yd, dev, pd, want_out=True, want_state_copy=True)
        else:
            out = dev.forward_partials(yd, pd, out=torch.empty_like(yd), running=False, snap=snap)
    elif kind in ("head", "head relu"):
        snap = torch.full((8,), -1, dtype=torch.int32, device="cuda")
        dev.head_update(pd, running=running, relu=relu, snap=snap)
        out = dev.relu_apply(yd.view(1, 1, -1), 0).view(-1) if relu else dev.apply(yd)
        known = given if running else None                 # (running == 0: the pairs are not read)
    elif kind == "relu":
        out = dev.relu_forward(yd, partials=pd, running=running)
        known = given if running else None
    else:
        out = replicas(dev.relu_up2_forward(yd.view(1, 1, -1), partials=pd, running=running), 1, 1, y.numel())[0].reshape(-1)
        known = given if running else None
    dev.check(st, known, (kind, what), snap=snap)
    assert same(out.cpu(), ref), (kind, what)


@pytest.mark.gpu
@pytest.mark.parametrize("n", PAIR_COUNTS)
def test_update_from_pairs_finds_the_extremes_at_every_index(n):
    """The global extremes at pair 0, 255, 256 and n - 1, empty pairs (+inf, -inf) mixed in, through the five entry
    points that reduce pairs; the snapshot equals the state in words [2..6] and is zero in [0], [1], [7]."""
    g = torch.Generator().manual_seed(60 + n)
    pos = sorted({p for p in (0, 255, 256, n - 1) if p < n})
    for pmin in pos:
        for pmax in pos:
            for lo, hi in ((-5.0, 7.0), (2.0, 7.0)) if pmin == pos[0] else ((-5.0, 7.0),):
                pairs = _pairs(n, pmin, pmax, lo, hi, g)
                if lo > 0:
                    pairs[:, 0] += 4.0                     # every minimum positive: the ReLU clamp must leave 2.0 alone
                    pairs[pmin, 0] = lo
                if n > 2:                                  # empty pairs change nothing
                    for e in {1 % n, n // 2, n - 2} - {pmin, pmax}:
                        pairs[e, 0], pairs[e, 1] = float("inf"), float("-inf")
                for kind in UPDATE_KINDS:
                    _update_from_pairs(Dev(), Given(), kind, pairs, (f32(lo)[0], f32(hi)[0]), what=(n, pmin, pmax, lo))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257])
def test_update_from_pairs_nan_and_empty(n):
    """All pairs empty: both ranges NaN (an all-NaN producer tensor).  A NaN in either slot of the LAST pair: both
    ranges NaN -- with relu = 1 the NaN is kept, not clamped to 0."""
    g = torch.Generator().manual_seed(70 + n)
    nan = f32(float("nan"))[0]
    empty = torch.tensor([[float("inf"), float("-inf")]]).repeat(n, 1)
    cases = [("empty", empty)]
    for slot in (0, 1):
        p = _pairs(n, 0, 0, -5.0, 7.0, g)
        p[n - 1, slot] = _nans()[slot]
        cases.append(("nan in slot %d" % slot, p))
    for what, pairs in cases:
        for kind in UPDATE_KINDS:
            dev, st = Dev(), Given()
            _update_from_pairs(dev, st, kind, pairs, (nan, nan), what=(n, what))
            assert torch.isnan(dev.x_min).item() and torch.isnan(dev.x_max).item()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", UPDATE_KINDS)
def test_update_sequence_from_pairs(kind):
    """Initialisation, a wide EMA step, a narrower one; then running = 0 on a range changed behind the kernel's back:
    the range is untouched, scale and zero point are re-derived from it."""
    g = torch.Generator().manual_seed(80)
    dev, st = Dev(), Given()
    for it, (lo, hi) in enumerate(((-2.0, 3.0), (-6.0, 9.0), (-0.5, 0.75))):
        pairs = _pairs(300, 299, 256, lo, hi, g) * torch.tensor([min(1.0, -lo), min(1.0, hi)])
        pairs[299, 0], pairs[256, 1] = lo, hi
        _update_from_pairs(dev, st, kind, pairs, (f32(lo)[0], f32(hi)[0]), what=it)
    dev.x_max.mul_(1.5)
    st.x_max.mul_(1.5)
    lo_hi = (dev.x_min.clone(), dev.x_max.clone())
    _update_from_pairs(dev, st, kind, _pairs(300, 0, 1, -1.0, 2.0, g), (f32(-1.0)[0], f32(2.0)[0]), running=False, what="frozen")
    assert torch.equal(dev.x_min, lo_hi[0]) and torch.equal(dev.x_max, lo_hi[1])


@pytest.mark.gpu
def test_relu_update_of_negative_extremes_stays_in_the_initialisation_branch():
    """relu = 1 on all-negative extremes: (0, 0), and the next call initialises again."""
    g = torch.Generator().manual_seed(81)
    for kind in ("head relu", "relu", "relu_up2"):
        dev, st = Dev(), Given()
        pairs = torch.stack([-torch.rand(257, generator=g) - 2.0, -torch.rand(257, generator=g) - 1.0], dim=1)
        _update_from_pairs(dev, st, kind, pairs, (pairs[:, 0].min(), pairs[:, 1].max()), what="negative")
        assert (dev.x_min.item(), dev.x_max.item()) == (0.0, 0.0)
        _update_from_pairs(dev, st, kind, _pairs(257, 256, 255, -1.0, 4.0, g), (f32(-1.0)[0], f32(4.0)[0]), what="then mixed")
        assert (dev.x_min.item(), dev.x_max.item()) == (0.0, 4.0)


@pytest.mark.gpu
def test_update_from_external_extremes_and_commit_range():
    """cdn_quantact_forward with batch_min / batch_max, and cdn_quantact_commit_range with running = 1, against the
    oracle EMA over three steps (the second narrower)."""
    g = torch.Generator().manual_seed(82)
    x = torch.randn(1027, generator=g)
    xd = x.cuda()
    dev, st = Dev(), Given()
    cdev, cst = Dev(), Given()
    for it, (lo, hi) in enumerate(((-2.0, 3.0), (-0.25, 0.5), (-6.0, 9.0))):
        st.given = cst.given = (f32(lo)[0], f32(hi)[0])
        ref, q = st(x, return_codes=True)
        bmin, bmax = f32(lo).cuda(), f32(hi).cuda()
        out, codes = dev.forward(xd, bmin=bmin, bmax=bmax, want_codes=True)
        dev.check(st, st.given, ("external", it))
        assert torch.equal(out.cpu(), ref) and torch.equal(codes.cpu().float(), _int16(q))
        # the commit: the range follows `range`, the code-width flag this rank's extremes in words [4], [5]
        cst.update(None)
        mine = (f32(0.5 * lo)[0], f32(0.5 * hi)[0])
        cdev.state.view(torch.float32)[4:6] = torch.stack(mine).cuda()
        cdev.commit(torch.tensor([lo, hi]).cuda())
        cdev.check(cst, mine, ("commit", it))
    ref = st(x, running=False)                             # running = 0 with extremes: frozen range, words [4], [5] theirs
    out, _ = dev.forward(xd, running=False, bmin=f32(-1.0).cuda(), bmax=f32(1.0).cuda())
    dev.check(st, (f32(-1.0)[0], f32(1.0)[0]), "external, frozen")
    assert torch.equal(out.cpu(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("b,level,flag", [(270.875, 2039.0, 0), (271.0, 2040.0, 1), (-238.875, -2039.0, 0), (-239.0, -2040.0, 1)])
def test_code_width_flag_at_its_threshold(b, level, flag):
    """Word [6] sends consumers to the int8 or the f32 kernels; its threshold is a level magnitude of 2039.  Frozen range
    (0, 31.875) (scale 8, zero point 128), this rank's extremes (0, b) / (b, 0) in words [4], [5], running = 0 commit."""
    scale, zp = Q.act_params(f32(TIE_RANGE[0]), f32(TIE_RANGE[1]), 8)
    assert (torch.round(scale * f32(b) - zp) + (zp - 128.0)).item() == level
    dev, st = Dev(x_min=TIE_RANGE[0], x_max=TIE_RANGE[1]), Given(x_min=TIE_RANGE[0], x_max=TIE_RANGE[1])
    mine = (f32(min(b, 0.0))[0], f32(max(b, 0.0))[0])
    dev.state.view(torch.float32)[4:6] = torch.stack(mine).cuda()
    dev.commit(torch.tensor([-100.0, 100.0]).cuda(), running=False)
    assert wide_flag(8, scale, zp, mine) == flag
    dev.check(st, mine, ("threshold", b))
    assert dev.words()[6].item() == flag
    # no batch extremes known, or another width: always 1
    dev.forward(torch.zeros(4, device="cuda"), running=False, want_out=False)
    assert dev.words()[6].item() == 1
    d4 = Dev(bits=4)
    d4.forward(torch.rand(5, device="cuda"), want_out=False)
    assert d4.words()[6].item() == 1


# ---- 4. backward ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL + [N_BIG])
def test_relu_backward_equals_the_module(n):
    """cdn_relu_backward against the CPU nn.ReLU backward (y <= 0 ? 0 : g) on positive, negative, +-0.0, denormal, +inf
    and NaN y: the gradient passes at a NaN."""
    from codenet_amd import _native as N_
    g = torch.Generator().manual_seed(90 + n % 89)
    y = special_y(n, g).requires_grad_(True)
    go = wide_g((n,), g)
    torch.nn.ReLU()(y).backward(go)
    yd, gd = y.detach().cuda(), go.cuda()
    gy = torch.full_like(yd, 123.0)
    N_.check(N_.lib().cdn_relu_backward(_p(gd), _p(yd), _p(gy), n, torch.cuda.current_stream().cuda_stream), "cdn_relu_backward")
    assert torch.equal(gy.cpu(), y.grad), n
    nan = torch.isnan(y.detach())
    assert nan[n - 1] and torch.equal(y.grad[nan], go[nan])


def _up2_backward_case(P, H, W, on_device):
    from codenet_amd import _native as N_
    g = torch.Generator().manual_seed(100 + W + 16 * H)
    n = P * H * W
    y = special_y(n, g).view(1, P, H, W).requires_grad_(True)
    go = wide_g((1, P, 2 * H, 2 * W), g)
    torch.nn.Upsample(scale_factor=2, mode="nearest")(torch.nn.ReLU()(y)).backward(go)
    ref = y.grad.view(-1)
    gd = go.cuda()
    st = torch.cuda.current_stream().cuda_stream
    yd = y.detach().view(-1).cuda()
    gy = torch.full_like(yd, 123.0)
    N_.check(N_.lib().cdn_up2_relu_backward(_p(gd), _p(yd), _p(gy), P, H, W, st), "cdn_up2_relu_backward")
    assert torch.equal(gy, ref.cuda()) if on_device else torch.equal(gy.cpu(), ref), (P, H, W)
    # y and grad_y as views that start 4 bytes into their allocation: only grad_out must be aligned
    ybuf, gbuf = torch.empty(n + 1, device="cuda"), torch.full((n + 1,), 123.0, device="cuda")
    yv, gv = ybuf[1:], gbuf[1:]
    yv.copy_(yd)
    assert yv.data_ptr() % 16 == 4 and gv.data_ptr() % 16 == 4
    N_.check(N_.lib().cdn_up2_relu_backward(_p(gd), _p(yv), _p(gv), P, H, W, st), "cdn_up2_relu_backward")
    assert torch.equal(gv, ref.cuda()) if on_device else torch.equal(gv.cpu(), ref), (P, H, W, "offset")
    assert gbuf[0].item() == 123.0


@pytest.mark.gpu
@pytest.mark.parametrize("P,H,W", UP_SHAPES)
def test_up2_relu_backward_equals_the_module_bit_for_bit(P, H, W):
    """cdn_up2_relu_backward against the CPU backward of Upsample(ReLU(y)): the replica sum in the order
    ((a + b) + c) + d, the threshold mask of torch, on both paths of the kernel."""
    _up2_backward_case(P, H, W, False)


@pytest.mark.gpu
def test_up2_relu_backward_wrapped_grid():
    _up2_backward_case(*UP_BIG, True)
