"""The quantised stem (layer0) of the QAT step on the native path (functions/codenet_stem.py, csrc/codenet_stem_train.hip):
forward and backward against the module path, both stems (stride 4, and stride 2 + MaxPool2d(3, 2, 1)).

1. `test_exact_arithmetic_*`: the construction of tests/test_gpu_units_train.py -- inputs on which every summation order
   gives the same float32 -- so the native path must be torch.equal to the CPU module path on the output and on the gradients
   of conv.weight, bn.weight and bn.bias, eagerly and replayed twice from a HIP graph.  The pooled cases also assert that
   enough pool windows have a tied maximum, so the first-maximum rule of the pool backward is exercised.
2. `test_own_intermediates_*`: the model's own weights, running ranges, three forwards.  The oracle's QuantAct on relu of the
   native path's own y0 must track the device range bit for bit; y0, grad_Wq and grad_b must agree with a float64 evaluation
   from those intermediates within |got - ref| <= 1.01 (n + 2) 2^-24 S (n terms, S the float64 sum of their magnitudes); the
   quantised output, the pool and the pool's gradient are selections and roundings the CPU repeats bit for bit.
3. `test_detection_net_*`: image -> stem -> layers 1-4 -> stages -> heads -> CtdetLoss -> Adam as one captured step,
   bit-identical to the eager step, accepted by GraphedTrainStep without `unvalidated`; two runs from one seed end
   bit-identical.
4. `test_gating_*`: what takes the native path and what keeps the module path.

Smallest shapes at which the kernels can go wrong, N = 2: images 36 x 44 (ragged planes, no multiple of 4), 17 x 22 (the last
row's taps run off the image; pooled: an odd 9 x 11 conv plane, windows clipped right and bottom), 64 x 64 (aligned; two to
eight chunks of the weight gradient, two positions per thread in the pooled case); 256 x 256 in the float64 comparison alone
(8192 and 32768 positions: the weight gradient's full eight positions per thread, as at the QAT shape).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import quant as Q
from tests import qat_support

pytestmark = pytest.mark.gpu

# (maxpool, H, W)
CASES = [(False, 36, 44), (False, 17, 22), (False, 64, 64), (True, 36, 44), (True, 17, 22), (True, 64, 64)]

_model, _fq32, _within, _SLACK = qat_support.model, qat_support.fq32, qat_support.within, qat_support.SLACK


def _parts(layer0):
    return layer0[0], layer0[1][1]      # QuantBnConv2d, QuantAct


# ---- 1. exact arithmetic -------------------------------------------------------------------------------------------------

def exact_stem(maxpool, seed=5):
    """The stem of a quantised model with weights / BatchNorm / range on which every float32 sum is exact: integer codes in
    [-127, 127] over 128, all 27 taps non-zero, one of them +-127 per channel, so the 8-bit scale is exactly 128 and the
    fake-quantisation of the weights is the identity."""
    g = torch.Generator().manual_seed(seed)
    layer0 = copy.deepcopy(_model(maxpool=maxpool).layer0)
    cb, act = _parts(layer0)
    co = cb.conv.out_channels
    assert cb.conv.bias is None and cb.weight_bit == 8 and tuple(cb.conv.weight.shape) == (24, 3, 3, 3)
    codes = torch.randint(1, 128, (co, 27), generator=g).float() * (torch.randint(0, 2, (co, 27), generator=g) * 2 - 1).float()
    codes[torch.arange(co), torch.randint(0, 27, (co,), generator=g)] = 127.0
    codes[::2] = -codes[::2]      # the +-127 tap: both signs occur
    assert bool((codes != 0).all()) and bool((codes.abs().max(1).values == 127).all())
    with torch.no_grad():
        cb.conv.weight.copy_((codes / 128).view(co, 3, 3, 3))
        cb.bn.eps = 0.0
        cb.bn.running_var.fill_(1.0)
        cb.bn.running_mean.zero_()
        cb.bn.weight.fill_(1.0)
        cb.bn.bias.copy_(torch.randint(-8, 9, (co,), generator=g).float() / 8)
        act.running_stat = False
        act.x_min.zero_()
        act.x_max.fill_(255.0 / 8)
    return layer0


def run_stem(layer0, x, gy, dtype=None, fn=None):
    """forward + backward of the stem on a fresh copy -> (output, {parameter name: grad})."""
    layer0 = copy.deepcopy(layer0)
    if dtype is not None:
        layer0, x, gy = layer0.to(dtype), x.to(dtype), gy.to(dtype)
    layer0.train()
    out = fn(layer0, x) if fn is not None else layer0(x)
    (out * gy).sum().backward()
    grads = {n: p.grad for n, p in layer0.named_parameters()}
    assert sorted(grads) == ["0.bn.bias", "0.bn.weight", "0.conv.weight"] and all(v is not None for v in grads.values())
    return out.detach(), grads


def _tied_share(q):
    """Share of the 3 x 3 / stride 2 / padding 1 windows of q whose maximum is attained more than once."""
    Nb, C, H, W = q.shape
    cols = F.unfold(F.pad(q, (1, 1, 1, 1), value=float("-inf")).view(Nb * C, 1, H + 2, W + 2), 3, stride=2)
    return float(((cols == cols.max(1, keepdim=True).values).sum(1) > 1).float().mean())


_EXACT = {}


def exact_case(maxpool, H, W):
    """The CPU module-path reference of one exact case (computed once), with the construction asserts."""
    key = (maxpool, H, W)
    if key not in _EXACT:
        layer0 = exact_stem(maxpool)
        g = torch.Generator().manual_seed(6)
        x = torch.randint(0, 32, (2, 3, H, W), generator=g).float() / 8 - 2
        with torch.no_grad():
            shape = copy.deepcopy(layer0)(x).shape
        gy = torch.randint(-2, 3, tuple(shape), generator=g).float()
        o32, g32 = run_stem(layer0, x, gy)
        o64, g64 = run_stem(layer0, x, gy, dtype=torch.float64)
        # the construction: float32 equals float64 bit for bit, so no summation order can change a float32
        assert torch.equal(o32.double(), o64)
        for n in g32:
            assert torch.equal(g32[n].double(), g64[n]), n
        # no case passes by being dead
        live = lambda t: float((t != 0).float().mean())      # noqa: E731
        assert live(o32) >= 0.40 and float(o32.max()) < 255.0 / 8, (live(o32), float(o32.max()))
        assert live(g32["0.conv.weight"]) >= 0.60, live(g32["0.conv.weight"])
        if maxpool:
            with torch.no_grad():
                pre = copy.deepcopy(layer0)
                q = pre[1][1](pre[1][0](pre[0](x)))
            assert _tied_share(q) >= 0.02, _tied_share(q)      # the tie rule of the pool backward is exercised
        _EXACT[key] = (layer0, x, gy, o32, g32)
    return _EXACT[key]


@pytest.mark.parametrize("maxpool,H,W", CASES)
def test_exact_arithmetic_forward_and_backward_equal_the_cpu_module_path(maxpool, H, W):
    from codenet_amd.functions import codenet_stem as ST
    layer0, x, gy, o_ref, g_ref = exact_case(maxpool, H, W)
    dev = copy.deepcopy(layer0).cuda().train()
    xs, gys = x.cuda(), gy.cuda()
    assert ST.native_reason(dev, xs) is None
    params = dict(dev.named_parameters())

    def step():
        keep = {}
        out = ST.forward_stem(dev, xs, keep=keep)
        assert "y0" in keep and keep["pooled"] == maxpool      # the native path ran
        (out * gys).sum().backward()
        return out

    def check(out, what):
        assert torch.equal(out.detach().cpu(), o_ref), what
        for n, p in params.items():
            assert torch.equal(p.grad.cpu(), g_ref[n]), (what, n)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    check(out, "eager")
    for p in params.values():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for replay in (1, 2):
        with torch.no_grad():
            for p in params.values():
                p.grad.fill_(float("nan"))
            out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        check(out, "graph replay %d" % replay)


# ---- 2. running ranges, real arithmetic on the kernels' own intermediates ------------------------------------------------

def _conv_ref(x, w, b, g, stride):
    """float64 forward / parameter gradients of the stem's convolution from float32 operands, and the sums of magnitudes."""
    res = []
    for mag in (False, True):
        xd = (x.abs() if mag else x).double()
        wd = (w.abs() if mag else w).double().requires_grad_(True)
        bd = (b.abs() if mag else b).double().requires_grad_(True)
        y = F.conv2d(xd, wd, bd, stride, 1)
        y.backward((g.abs() if mag else g).double())
        res.append((y.detach(), wd.grad, bd.grad))
    return res[0], res[1]


@pytest.mark.parametrize("maxpool", [False, True])
@pytest.mark.parametrize("H,W", [(17, 22), (64, 64), (256, 256)])      # (256 x 256: eight positions per thread in grad_Wq)
def test_own_intermediates_ranges_through_the_oracle_and_every_kernel_against_float64(maxpool, H, W):
    from codenet_amd.functions import codenet_stem as ST
    layer0 = copy.deepcopy(_model(maxpool=maxpool).layer0).cuda().train()
    cb, act = _parts(layer0)
    stride = cb.conv.stride[0]
    assert act.running_stat and stride == (2 if maxpool else 4)
    act.x_min.zero_()
    act.x_max.zero_()
    mirror = Q.QuantActState()
    g = torch.Generator().manual_seed(11 + H + int(maxpool))
    N = 2
    for fwd in (1, 2, 3):      # the "+=" initialisation, then two EMA steps
        x = (torch.rand(N, 3, H, W, generator=g) * 5 - 2.5).cuda()
        keep = {}
        if fwd < 3:
            assert ST.native_reason(layer0, x) is None
            out = ST.forward_stem(layer0, x, keep=keep)
        else:      # as forward_stem calls it, with the prepared weights in reach for their gradients
            wq, b = cb.folded()
            wq.retain_grad()
            b.retain_grad()
            out = ST.CodenetStemFunction.apply(x, (stride, act, maxpool), keep, wq, b)
        what = "%s %dx%d forward %d" % ("pooled" if maxpool else "plain", H, W, fwd)
        y0 = keep["y0"].cpu()
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        assert y0.shape == (N, 24, Ho, Wo) and keep["pooled"] == maxpool and keep["out"].data_ptr() == out.data_ptr()
        # the device range: the oracle's QuantAct on relu of the native path's own y0
        mirror.update(torch.relu(y0))
        assert torch.equal(mirror.x_min, act.x_min.cpu()) and torch.equal(mirror.x_max, act.x_max.cpu()), \
            "%s: oracle (%r, %r) vs device (%r, %r)" % (what, mirror.x_min, mirror.x_max, act.x_min, act.x_max)
        assert float(act.x_min) == 0.0 and float(act.x_max) > 0
        # y0 from the image and the native path's own Wq, b
        (ref, _, _), (S, _, _) = _conv_ref(x.cpu(), keep["wq"].detach().cpu(), keep["b"].detach().cpu(), torch.zeros_like(y0),
                                           stride)
        _within(keep["y0"], ref, 28, S, what + " y0")
        # the quantised values (a rounding the CPU repeats bit for bit) and the pool (a selection)
        q = _fq32(torch.relu(y0), mirror.x_min, mirror.x_max)
        assert torch.equal(out.detach().cpu(), F.max_pool2d(q, 3, 2, 1) if maxpool else q), what
    # backward of forward 3
    gy = torch.randn(out.shape, generator=g).cuda()
    out.backward(gy)
    torch.cuda.synchronize()
    if maxpool:
        qd = q.clone().requires_grad_(True)
        F.max_pool2d(qd, 3, 2, 1).backward(gy.cpu())
        gy0 = qd.grad * (y0 > 0)
        assert torch.equal(keep["gy0"].cpu(), gy0), what + ": the pool's gradient"      # selection rounds nothing
        assert _tied_share(q) > 0
    else:
        gy0 = gy.cpu() * (y0 > 0)
    (_, ref_gw, ref_gb), (_, S_gw, S_gb) = _conv_ref(x.cpu(), wq.detach().cpu(), b.detach().cpu(), gy0, stride)
    _within(wq.grad, ref_gw, N * Ho * Wo, S_gw, what + " grad_Wq")
    _within(b.grad, ref_gb, N * Ho * Wo, S_gb, what + " grad_b")
    for p in layer0.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().sum()) > 0
    print("worst slack: %.3e (%s)" % min(_SLACK))


# ---- 3. reproducibility and capture -------------------------------------------------------------------------------------

def _net(maxpool=False):
    from codenet_amd import pipeline
    return qat_support.train_net(pipeline.DetectionNet, maxpool=maxpool)


def _net_setup():
    return qat_support.step_setup(lambda g, N, R: torch.randint(0, 256, (N, 3, 4 * R, 4 * R), generator=g).float() / 64 - 2, 4)


@pytest.mark.parametrize("maxpool", [False, True])
def test_detection_net_captured_step_replays_the_eager_step_bit_for_bit(maxpool):
    from codenet_amd import pipeline
    from codenet_amd.functions import codenet_stem as ST
    loss_fn, imgs = _net_setup()
    eager, (net_g, opt_g) = [qat_support.with_capturable_adam(_net(maxpool)) for _ in range(2)]
    G = pipeline.GraphedTrainStep
    assert G.is_native_net(net_g) and not G.is_native_trunk(net_g) and not G.is_native_tail(net_g) and not G.is_stage_stack(net_g)
    assert ST.native_reason(net_g.layer0, imgs[0]) is None
    # three steps; the stem took part in the loss
    qat_support.check_captured_step(eager, (net_g, opt_g), loss_fn, imgs, lambda n: n == "layer0.0.conv.weight")
    if maxpool:
        return
    # the bare model stays outside the validated scope; so does the net with the stem's switch off
    whole = _model().cuda().train()
    assert not G.is_native_net(whole)
    with pytest.raises(NotImplementedError):
        G(whole, opt_g, loss_fn, (imgs[0],))
    ST.NATIVE_STEM = False
    try:
        assert not G.is_native_net(net_g)
        with pytest.raises(NotImplementedError):
            G(net_g, opt_g, loss_fn, (imgs[0],))
    finally:
        ST.NATIVE_STEM = True


def test_detection_net_two_identical_runs_end_bit_identical():
    loss_fn, imgs = _net_setup()
    qat_support.check_two_identical_runs(_net, loss_fn, imgs[:3])


def test_detection_net_is_the_bare_model_in_train_mode_head_by_head():
    from codenet_amd import pipeline
    _, imgs = _net_setup()
    m1 = _model().cuda().train()
    m2 = copy.deepcopy(m1)
    o1 = m1(imgs[0])[0]
    o2 = pipeline.DetectionNet(m2)(imgs[0])[0]
    assert sorted(o1) == sorted(o2) == ["hm", "reg", "wh"]
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    assert "CodenetHeads" in type(o1["hm"].grad_fn).__name__
    for (n1, b1), (_, b2) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(b1, b2), n1


# ---- 4. gating ---------------------------------------------------------------------------------------------------------------

def test_gating_on_the_gpu():
    from codenet_amd.functions import codenet_stem as ST
    model = _model().cuda().train()
    layer0 = model.layer0
    x = (torch.rand(2, 3, 32, 36, generator=torch.Generator().manual_seed(4)) * 4 - 2).cuda()
    assert ST.native_reason(layer0, x) is None
    assert "contiguous" in ST.native_reason(layer0, x.transpose(2, 3))
    assert "[N, 3, H, W]" in ST.native_reason(layer0, x[:, :2].contiguous())
    assert "aligned" in ST.native_reason(layer0, torch.empty(2 * 3 * 32 * 36 + 1, device="cuda")[1:].view(2, 3, 32, 36))
    # with the switch off: exactly the module path, and nothing kept
    a, b = copy.deepcopy(layer0), copy.deepcopy(layer0)
    ST.NATIVE_STEM = False
    try:
        keep = {}
        got = ST.forward_stem(a, x, keep=keep)
        assert "NATIVE_STEM" in ST.native_reason(a, x) and not keep
    finally:
        ST.NATIVE_STEM = True
    assert torch.equal(got, b(x))
    for (n1, b1), (_, b2) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(b1, b2), n1
    # a percentile QuantAct keeps the module path, with the module path's result
    a, b = copy.deepcopy(layer0), copy.deepcopy(layer0)
    for m in (a, b):
        m[1][1].percentile = True
    assert "percentile" in ST.native_reason(a, x)
    keep = {}
    assert torch.equal(ST.forward_stem(a, x, keep=keep), b(x)) and not keep
    # a forward hook on a sub-module fires: the module path
    c = copy.deepcopy(layer0)
    fired = []
    c[0].register_forward_hook(lambda mod, inp, out: fired.append(1))
    assert "hook" in ST.native_reason(c, x)
    ST.forward_stem(c, x, keep=keep)
    assert fired and not keep
    # an image that requires grad takes the module path and receives its gradient
    d = copy.deepcopy(layer0)
    xg = x.clone().requires_grad_(True)
    assert "requires grad" in ST.native_reason(d, xg)
    ST.forward_stem(d, xg, keep=keep).sum().backward()
    assert not keep and xg.grad is not None and float(xg.grad.abs().sum()) > 0
    # without any of these the same stem runs natively (keep is filled) and its QuantAct's range moves in place
    e = copy.deepcopy(layer0)
    y = ST.forward_stem(e, x, keep=keep)
    assert "y0" in keep and y.shape == (2, 24, 8, 9) and "CodenetStem" in type(y.grad_fn).__name__
    assert float(e[1][1].x_max) > 0 and float(layer0[1][1].x_max) == 0
    with torch.no_grad():      # grad mode off: forward is unchanged -- the module path, whatever the switch says
        m1, m2 = copy.deepcopy(model), copy.deepcopy(model)
        img = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(6)).cuda()
        assert "grad" in ST.native_reason(m1.layer0, img)
        o1 = m1(img)[0]
        ST.NATIVE_STEM = False
        try:
            o2 = m2(img)[0]
        finally:
            ST.NATIVE_STEM = True
        assert all(torch.equal(o1[k], o2[k]) for k in o1)
