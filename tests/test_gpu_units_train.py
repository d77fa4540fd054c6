"""The quantised ShuffleNetV2 units and layer4 of the QAT step on the native path (functions/codenet_units.py,
csrc/codenet_units_train.hip): forward and backward against the module path.

1. `test_exact_arithmetic_*`: the construction of tests/test_gpu_heads_train.py -- inputs on which every summation order
   gives the same float32 -- so the native path must be torch.equal to the CPU module path on the output, grad_x and every
   parameter gradient, eagerly and replayed twice from a HIP graph.  One unit per case: a chain of two units is not exact in
   the first unit's gradients with this construction (the fractional bits accumulate).
2. `test_own_intermediates_*`: stride 2 followed by two stride-1 units with one shared QuantAct, random weights, running
   ranges, three forwards.  The oracle's QuantAct on the native path's own intermediates, applied in the reference's order
   (four applications of the shared act per forward), must track every device range bit for bit; every new kernel's output
   must agree with a float64 evaluation from those intermediates within |got - ref| <= 1.01 (n + 2) 2^-24 S (n terms, S the
   float64 sum of their magnitudes); the pass-through half and its gradient are copies.
3. `test_detection_trunk_*`: layers 1-4 -> stages -> heads -> CtdetLoss as one captured step, bit-identical to the eager
   step, accepted by GraphedTrainStep without `unvalidated`; two runs from one seed end bit-identical.
4. `test_gating_*`: what takes the native path and what keeps the module path.

Smallest shapes at which the kernels can go wrong: N = 2; planes 12 x 20 (output width 10: the scalar path, rows no multiple
of the strip), 9 x 10 (odd: output 5 x 5, ragged widths), 16 x 16 (the 16-byte path at both strides), 64 x 24 (output 32 rows:
the 8-row strips); channels 24 -> 58 (no multiple of 4), 116 / 232 for the wider units.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import quant as Q
from tests import qat_support

pytestmark = pytest.mark.gpu

# (stride, C_in, h, H, W)
CASES = [(2, 24, 58, 12, 20), (2, 24, 58, 9, 10), (1, 116, 58, 12, 20), (1, 116, 58, 9, 10), (1, 232, 116, 16, 16),
         (2, 116, 116, 16, 16)]
_UNIT_OF = {(2, 24, 58): ("layer1", 0), (1, 116, 58): ("layer1", 1), (1, 232, 116): ("layer2", 1), (2, 116, 116): ("layer2", 0)}


_model, _codes, _fq32, _within, _SLACK = (qat_support.model, qat_support.codes, qat_support.fq32, qat_support.within,
                                          qat_support.SLACK)


# ---- 1. exact arithmetic -------------------------------------------------------------------------------------------------

def _convbns(node):
    cbs = [node.quant_convbn1, node.quant_convbn2, node.quant_convbn3]
    return cbs + ([node.quant_convbn4, node.quant_convbn5] if node.stride == 2 else [])


def exact_unit(stride, cin, h, seed=5):
    """One unit of a quantised model with weights / BatchNorms / ranges on which every float32 sum is exact."""
    g = torch.Generator().manual_seed(seed)
    layer, idx = _UNIT_OF[(stride, cin, h)]
    node = copy.deepcopy(getattr(_model(), layer)[idx])
    assert node.stride == stride and node.quant_convbn1.conv.out_channels == h
    with torch.no_grad():
        for cb in _convbns(node):
            co, ci, kh, kw = cb.conv.weight.shape
            assert cb.conv.bias is None
            if kh == 1:
                cb.conv.weight.copy_((_codes(g, co, ci, 3) / 8).view(co, ci, 1, 1))
            else:
                cb.conv.weight.copy_((_codes(g, co, 9, 9) / 16).view(co, 1, 3, 3))
            cb.bn.eps = 0.0
            cb.bn.running_var.fill_(1.0)
            cb.bn.running_mean.zero_()
            cb.bn.weight.fill_(1.0)
            cb.bn.bias.copy_(torch.randint(-8, 9, (co,), generator=g).float() / 8)
        acts = [(node.quant_act1, 0.0, 255.0 / 16), (node.quant_act2, -16.0, 127.0 / 8), (node.quant_act, 0.0, 255.0 / 8)]
        if stride == 2:
            acts.append((node.quant_act4, -16.0, 127.0 / 8))
        for act, lo, hi in acts:
            act.running_stat = False
            act.x_min.fill_(lo)
            act.x_max.fill_(hi)
    return node


def run_unit(node, x, gy, dtype=None, fn=None):
    """forward + backward of the unit on a fresh copy -> (output, x.grad, {parameter name: grad})."""
    node = copy.deepcopy(node)
    if dtype is not None:
        node, x, gy = node.to(dtype), x.to(dtype), gy.to(dtype)
    x = x.detach().clone().requires_grad_(True)
    node.train()
    out = fn(node, x) if fn is not None else node(x)
    (out * gy).sum().backward()
    grads = {n: p.grad for n, p in node.named_parameters()}
    assert all(v is not None for v in grads.values())
    return out.detach(), x.grad, grads


_EXACT = {}


def exact_case(stride, cin, h, H, W):
    """The CPU module-path reference of one exact case (computed once), with the construction asserts."""
    key = (stride, cin, h, H, W)
    if key not in _EXACT:
        node = exact_unit(stride, cin, h)
        g = torch.Generator().manual_seed(6)
        x = torch.randint(0, 32, (2, cin, H, W), generator=g).float() / 8
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        gy = torch.randint(-2, 3, (2, 2 * h, Ho, Wo), generator=g).float()
        o32, gx32, g32 = run_unit(node, x, gy)
        o64, gx64, g64 = run_unit(node, x, gy, dtype=torch.float64)
        # the construction: float32 equals float64 bit for bit, so no summation order can change a float32
        assert torch.equal(o32.double(), o64) and torch.equal(gx32.double(), gx64)
        for n in g32:
            assert torch.equal(g32[n].double(), g64[n]), n
        # no case passes by being dead
        live = lambda t: float((t != 0).float().mean())      # noqa: E731
        assert live(o32) >= 0.40 and float(o32.max()) < 255.0 / 8, (live(o32), float(o32.max()))
        assert live(gx32) >= 0.60, live(gx32)
        for n, v in g32.items():
            if n.endswith("conv.weight"):
                assert live(v) >= 0.60, (n, live(v))
        _EXACT[key] = (node, x, gy, o32, gx32, g32)
    return _EXACT[key]


@pytest.mark.parametrize("stride,cin,h,H,W", CASES)
def test_exact_arithmetic_forward_and_backward_equal_the_cpu_module_path(stride, cin, h, H, W):
    from codenet_amd.functions import codenet_units as CU
    node, x, gy, o_ref, gx_ref, g_ref = exact_case(stride, cin, h, H, W)
    dev = copy.deepcopy(node).cuda().train()
    xs = x.cuda().requires_grad_(True)
    gys = gy.cuda()
    assert CU.native_reason(dev, xs) is None
    params = dict(dev.named_parameters())

    def step():
        keep = {}
        out = CU.forward_units(dev, xs, keep=keep)
        assert 0 in keep      # the native path ran
        (out * gys).sum().backward()
        return out

    def check(out, what):
        assert torch.equal(out.detach().cpu(), o_ref), what
        assert torch.equal(xs.grad.cpu(), gx_ref), what
        for n, p in params.items():
            assert torch.equal(p.grad.cpu(), g_ref[n]), (what, n)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    check(out, "eager")
    xs.grad = None
    for p in params.values():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for replay in (1, 2):
        with torch.no_grad():
            xs.grad.fill_(float("nan"))
            for p in params.values():
                p.grad.fill_(float("nan"))
            out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        check(out, "graph replay %d" % replay)


def test_exact_arithmetic_layer4_equals_the_cpu_module_path():
    from codenet_amd.functions import codenet_units as CU
    g = torch.Generator().manual_seed(9)
    l4 = copy.deepcopy(_model().layer4)
    cb, act = l4[0], l4[1][1]
    co, ci = cb.conv.weight.shape[:2]
    with torch.no_grad():
        cb.conv.weight.copy_((_codes(g, co, ci, 3) / 8).view(co, ci, 1, 1))
        cb.bn.eps = 0.0
        cb.bn.running_var.fill_(1.0)
        cb.bn.running_mean.zero_()
        cb.bn.weight.fill_(1.0)
        cb.bn.bias.copy_(torch.randint(-8, 9, (co,), generator=g).float() / 8)
        act.running_stat = False
        act.x_min.zero_()
        act.x_max.fill_(255.0 / 8)
    x = torch.randint(0, 32, (2, ci, 5, 4), generator=g).float() / 8
    gy = torch.randint(-2, 3, (2, co, 5, 4), generator=g).float()
    o32, gx32, g32 = run_unit(l4, x, gy)
    o64, gx64, g64 = run_unit(l4, x, gy, dtype=torch.float64)
    assert torch.equal(o32.double(), o64) and torch.equal(gx32.double(), gx64)
    assert all(torch.equal(g32[n].double(), g64[n]) for n in g32)
    assert float((o32 != 0).float().mean()) >= 0.40 and float((gx32 != 0).float().mean()) >= 0.60
    o, gx, gr = run_unit(l4.cuda(), x.cuda(), gy.cuda(), fn=CU.forward_layer4)
    assert torch.equal(o.cpu(), o32) and torch.equal(gx.cpu(), gx32)
    for n in g32:
        assert torch.equal(gr[n].cpu(), g32[n]), n


# ---- 2. running ranges, real arithmetic on the kernels' own intermediates ------------------------------------------------

def _chain():
    layer1 = _model().layer1
    chain = nn.Sequential(layer1[0], layer1[1], layer1[2]).cuda().train()
    assert [n.stride for n in chain] == [2, 1, 1] and all(n.quant_act is chain[0].quant_act for n in chain)
    return chain


def _node_acts(node):
    return [node.quant_act1, node.quant_act2] + ([node.quant_act4] if node.stride == 2 else [])


@pytest.mark.parametrize("H,W", [(64, 24), (9, 10)])
def test_own_intermediates_ranges_through_the_oracle_and_the_pass_through_half(H, W):
    from codenet_amd.functions import codenet_units as CU
    chain = _chain()
    shared = chain[0].quant_act
    for a in [shared] + [a for n in chain for a in _node_acts(n)]:
        assert a.running_stat
        a.x_min.zero_()
        a.x_max.zero_()
    m_shared = Q.QuantActState()
    mirrors = [{"act1": Q.QuantActState(), "act2": Q.QuantActState(), "act4": Q.QuantActState()} for _ in chain]
    g = torch.Generator().manual_seed(11 + H)
    N = 2

    def same(m, a, what):
        assert torch.equal(m.x_min, a.x_min.cpu()) and torch.equal(m.x_max, a.x_max.cpu()), \
            "%s: oracle (%r, %r) vs device (%r, %r)" % (what, m.x_min, m.x_max, a.x_min, a.x_max)

    def check_ranges(keep, what):
        """The oracle's QuantAct on the native path's own intermediates, in the reference's order; also the join: every
        branch is quantised with the shared act's state after ITS OWN update."""
        for i, node in enumerate(chain):
            k, m = keep[i], mirrors[i]
            h = k["y3"].shape[1]
            if node.stride == 2:
                m["act4"].update(k["y4"].cpu())
                same(m["act4"], node.quant_act4, "%s unit %d act4" % (what, i))
                r5 = torch.relu(k["y5"].cpu())
                m_shared.update(r5)
                ref = _fq32(r5, m_shared.x_min, m_shared.x_max).double()
                _within(k["out"][:, 0::2], ref, 1, ref.abs(), "%s unit %d join slot 0" % (what, i))
            else:
                assert torch.equal(k["out"][:, 0::2], k["x"][:, :h]), "pass-through half"
            m["act1"].update(torch.relu(k["y1"].cpu()))
            same(m["act1"], node.quant_act1, "%s unit %d act1" % (what, i))
            m["act2"].update(k["y2"].cpu())
            same(m["act2"], node.quant_act2, "%s unit %d act2" % (what, i))
            r3 = torch.relu(k["y3"].cpu())
            m_shared.update(r3)
            ref = _fq32(r3, m_shared.x_min, m_shared.x_max).double()
            _within(k["out"][:, 1::2], ref, 1, ref.abs(), "%s unit %d join slot 1" % (what, i))
            if i + 1 < len(chain):
                assert keep[i + 1]["x"].data_ptr() == k["out"].data_ptr()
        same(m_shared, shared, "%s shared act" % what)

    def grid_input():
        return (torch.randint(0, 256, (N, 24, H, W), generator=g).float() / 32).cuda().requires_grad_(True)

    for fwd in (1, 2):      # the "+=" initialisation, then one EMA step, through the public entry
        keep = {}
        x = grid_input()
        assert CU.native_reason(chain, x) is None
        out = CU.forward_units(chain, x, keep=keep)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        assert out.shape == (N, 116, Ho, Wo) and sorted(keep) == [0, 1, 2]
        check_ranges(keep, "forward %d" % fwd)
    # forward 3 unit by unit, as forward_units chains them, so that every unit's input gradient can be read
    x = grid_input()
    keep, xs = {}, [x]
    for i, node in enumerate(chain):
        keep[i] = {}
        xs.append(CU.CodenetUnitFunction.apply(xs[-1], CU._unit_meta(node), keep[i], *CU._prepared_weights(node)))
        xs[-1].retain_grad()
    check_ranges(keep, "forward 3")
    gy = torch.randn(xs[-1].shape, generator=g).cuda()
    xs[-1].backward(gy)
    torch.cuda.synchronize()
    h = 58
    # the pass-through half's gradient is the de-interleaved grad_out, bit for bit
    assert torch.equal(xs[2].grad[:, :h], xs[3].grad[:, 0::2]) and torch.equal(xs[1].grad[:, :h], xs[2].grad[:, 0::2])
    assert torch.equal(xs[3].grad, gy) and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().sum()) > 0
    for p in chain.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    print("worst slack: %.3e (%s)" % min(_SLACK))


def _dw_ref(inp, w, b, g, stride, rq, lo, hi):
    """float64 forward / backward of the depthwise 3x3 from float32 operands, and the sums of magnitudes of every result."""
    C = inp.shape[1]
    a32 = _fq32(torch.relu(inp), lo, hi) if rq else inp
    res = []
    for mag in (False, True):
        a = (a32.abs() if mag else a32).double().requires_grad_(True)
        wd = (w.abs() if mag else w).double().view(C, 1, 3, 3).requires_grad_(True)
        bd = (b.abs() if mag else b).double().requires_grad_(True)
        y = F.conv2d(a, wd, bd, stride, 1, 1, C)
        y.backward((g.abs() if mag else g).double())
        res.append((y.detach(), a.grad, wd.grad.view(C, 9), bd.grad))
    return res[0], res[1]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("rq", [True, False])
@pytest.mark.parametrize("H,W", [(64, 24), (9, 10), (16, 16)])
def test_own_intermediates_depthwise_kernels_against_float64(stride, rq, H, W):
    """Both strides, both input modes, through image pitches: the input is a channel slice of the native path's own y1
    (pre-activation values of a stride-2 unit), grad_in a channel slice of a wider buffer."""
    from codenet_amd.functions import codenet_units as CU
    chain = _chain()
    g = torch.Generator().manual_seed(3 + H)
    N, Cw, c0 = 2, 58, 8
    C = Cw - c0
    keep = {}
    x = (torch.randint(0, 256, (N, 24, H, W), generator=g).float() / 32).cuda().requires_grad_(True)
    CU.forward_units(chain[0], x, keep=keep)
    y1, act1 = keep[0]["y1"], chain[0].quant_act1
    assert y1.shape == (N, Cw, H, W)
    lo, hi = act1.x_min.cpu(), act1.x_max.cpu()
    snap = keep[0]["snap1"] if rq else None
    w = (torch.randn(C, 9, generator=g) / 3).cuda()
    b = torch.randn(C, generator=g).cuda()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    gout = torch.randn(N, C, Ho, Wo, generator=g).cuda()
    in_ptr, pitch = y1.data_ptr() + 4 * c0 * H * W, Cw * H * W
    # forward, with the running update of a fresh QuantAct behind it
    act = copy.deepcopy(chain[0].quant_act2)
    act.x_min.zero_()
    act.x_max.zero_()
    out, snap_o = CU._dw_forward(in_ptr, pitch, snap, w, b, N, C, H, W, stride, act, y1)
    (ref, ref_gin, ref_gw, ref_gb), (S, S_gin, S_gw, S_gb) = _dw_ref(y1[:, c0:].cpu(), w.cpu(), b.cpu(), gout.cpu(), stride, rq,
                                                                      lo, hi)
    tag = "stride %d %s %dx%d" % (stride, "fq(relu) on load" if rq else "as is", H, W)
    _within(out, ref, 10, S, "dw forward " + tag)
    mirror = Q.QuantActState()
    mirror.update(out.cpu())
    assert torch.equal(mirror.x_min, act.x_min.cpu()) and torch.equal(mirror.x_max, act.x_max.cpu())
    assert float(act.x_min) < 0      # the signed range of the raw output: no ReLU behind the depthwise conv
    # backward into a slice of a wider buffer
    wide = torch.full((N, Cw + 3, H, W), float("nan"), device="cuda")
    gin = (wide.data_ptr() + 4 * 3 * H * W, (Cw + 3) * H * W)
    wide[:, 3:3 + c0] = 7.0
    gw, gb = CU._dw_backward(gout, in_ptr, pitch, snap, w, (gin[0] + 4 * c0 * H * W, gin[1]), False, N, C, H, W, stride)
    torch.cuda.synchronize()
    assert torch.isnan(wide[:, :3]).all() and bool((wide[:, 3:3 + c0] == 7.0).all())      # the neighbours are untouched
    got_gin = wide[:, 3 + c0:].clone()
    mask = (y1[:, c0:].cpu() > 0).double() if rq else 1.0
    _within(got_gin, ref_gin * mask, 9 if stride == 1 else 4, S_gin, "dw grad_in " + tag)
    _within(gw, ref_gw, N * Ho * Wo, S_gw, "dw grad_w " + tag)
    _within(gb, ref_gb, N * Ho * Wo, S_gb, "dw grad_b " + tag)
    # accumulate: the same values added to what is stored, by the thread that owns the pixel
    base = torch.randn(N, C, H, W, generator=g).cuda()
    wide[:, 3 + c0:] = base
    gw2, gb2 = CU._dw_backward(gout, in_ptr, pitch, snap, w, (gin[0] + 4 * c0 * H * W, gin[1]), True, N, C, H, W, stride)
    torch.cuda.synchronize()
    assert torch.equal(wide[:, 3 + c0:], base + got_gin) and torch.equal(gw2, gw) and torch.equal(gb2, gb)


@pytest.mark.parametrize("H,W", [(16, 16), (9, 10)])
def test_own_intermediates_join_and_pitched_pointwise_against_float64(H, W):
    from codenet_amd import _native as N_
    from codenet_amd.functions import codenet_stage as CS
    from codenet_amd.functions import codenet_units as CU
    chain = _chain()
    g = torch.Generator().manual_seed(5 + H)
    N, h, Cx = 2, 58, 116
    keep = {}
    x0 = (torch.randint(0, 256, (N, 24, 2 * H, 2 * W), generator=g).float() / 32).cuda().requires_grad_(True)
    CU.forward_units(chain, x0, keep=keep)
    k = keep[1]      # a stride-1 unit: x [N, 116, H, W], the pointwise conv reads x[:, 58:] in place
    x, y3 = k["x"], k["y3"]
    assert x.shape == (N, Cx, H, W)
    lib, st = N_.lib(), torch.cuda.current_stream().cuda_stream
    # -- the join backward on the unit's own y3
    gout = torch.randn(N, 2 * h, H, W, generator=g).cuda()
    gx = torch.full((N, Cx, H, W), float("nan"), device="cuda")
    gy3 = CU._join_backward(gout, y3, 1, (gx.data_ptr(), Cx * H * W))
    assert torch.equal(gy3, gout[:, 1::2] * (y3 > 0)) and torch.equal(gx[:, :h], gout[:, 0::2]) and torch.isnan(gx[:, h:]).all()
    assert torch.equal(CU._join_backward(gout, y3, 0), gout[:, 0::2] * (y3 > 0))
    # -- the pitched pointwise: the slice in place, the output into a slice
    w = (torch.randn(h, h, generator=g) / 4).cuda()
    b = torch.randn(h, generator=g).cuda()
    xd, wd = x[:, h:].detach().double().cpu(), w.double().cpu()
    ref = torch.einsum("oc,nchw->nohw", wd, xd) + b.double().cpu().view(1, h, 1, 1)
    S = torch.einsum("oc,nchw->nohw", wd.abs(), xd.abs()) + b.double().cpu().abs().view(1, h, 1, 1)
    y, part = CU._pointwise(x.data_ptr() + 4 * h * H * W, Cx * H * W, None, w, b, N, h, H, W, True, x)
    _within(y, ref, h + 1, S, "pitched pointwise %dx%d" % (H, W))
    assert float(part[:, 0].min()) == float(y.min()) and float(part[:, 1].max()) == float(y.max())
    CU._pointwise(x.data_ptr() + 4 * h * H * W, Cx * H * W, None, w, b, N, h, H, W, False, x,
                  out=(gx.data_ptr() + 4 * h * H * W, Cx * H * W))
    assert torch.equal(gx[:, h:], y) and torch.equal(gx[:, :h], gout[:, 0::2])
    # -- the pitched weight gradient
    gyy = torch.randn(N, h, H, W, generator=g).cuda()
    ws = CS._workspace(lib.cdn_codenet_pointwise_wgrad_workspace_bytes(N, h, h, H * W), x.device)
    gw, gb = torch.full((h, h), float("nan"), device="cuda"), torch.full((h,), float("nan"), device="cuda")
    rc = lib.cdn_codenet_pointwise_wgrad_pitched(gyy.data_ptr(), x.data_ptr() + 4 * h * H * W, Cx * H * W, gw.data_ptr(),
                                                 gb.data_ptr(), N, h, h, H * W, ws.data_ptr(), ws.numel() * 4, st)
    N_.check(rc, "cdn_codenet_pointwise_wgrad_pitched")
    gd = gyy.double().cpu()
    _within(gw, torch.einsum("nohw,nchw->oc", gd, xd), N * H * W, torch.einsum("nohw,nchw->oc", gd.abs(), xd.abs()),
            "pitched weight gradient %dx%d" % (H, W))
    _within(gb, gd.sum((0, 2, 3)), N * H * W, gd.abs().sum((0, 2, 3)), "pitched bias gradient %dx%d" % (H, W))


# ---- 3. reproducibility and capture -------------------------------------------------------------------------------------

def _trunk():
    from codenet_amd import pipeline
    return qat_support.train_net(pipeline.DetectionTrunk)


def _trunk_setup():
    return qat_support.step_setup(lambda g, N, R: torch.randint(0, 256, (N, 24, R, R), generator=g).float() / 64, 4)


def test_detection_trunk_captured_step_replays_the_eager_step_bit_for_bit():
    from codenet_amd import pipeline
    from codenet_amd.functions import codenet_units as CU
    loss_fn, feats = _trunk_setup()
    eager, (net_g, opt_g) = [qat_support.with_capturable_adam(_trunk()) for _ in range(2)]
    G = pipeline.GraphedTrainStep
    assert G.is_native_trunk(net_g) and not G.is_native_tail(net_g) and not G.is_stage_stack(net_g)
    probe = torch.empty(2, 24, 32, 32, device="cuda")
    assert CU.native_reason(net_g.layer1, probe) is None
    assert CU.native_reason(net_g.layer4, torch.empty(2, 464, 4, 4, device="cuda")) is None
    # three steps; every unit took part in the loss
    qat_support.check_captured_step(eager, (net_g, opt_g), loss_fn, feats,
                                    lambda n: n.split(".")[0] in ("layer1", "layer2", "layer3", "layer4"))
    # the whole model holds the stem, which runs the framework's backward: not accepted as validated
    whole = _model().cuda().train()
    assert not G.is_native_trunk(whole)
    with pytest.raises(NotImplementedError):
        G(whole, opt_g, loss_fn, (torch.zeros(2, 3, 128, 128, device="cuda"),))
    CU.NATIVE_UNITS = False
    try:
        assert not G.is_native_trunk(net_g)
        with pytest.raises(NotImplementedError):
            G(net_g, opt_g, loss_fn, (feats[0],))
    finally:
        CU.NATIVE_UNITS = True


def test_detection_trunk_two_identical_runs_end_bit_identical():
    loss_fn, feats = _trunk_setup()
    qat_support.check_two_identical_runs(_trunk, loss_fn, feats[:3])


# ---- 4. gating ---------------------------------------------------------------------------------------------------------------

def test_gating_on_the_gpu():
    from codenet_amd.functions import codenet_units as CU
    model = _model().cuda().train()
    layer = model.layer2
    x = (torch.randint(0, 256, (2, 116, 8, 8), generator=torch.Generator().manual_seed(4)).float() / 32).cuda().requires_grad_(True)
    assert CU.native_reason(layer, x) is None
    assert "contiguous" in CU.native_reason(layer, x.detach().transpose(2, 3))
    assert "input channels" in CU.native_reason(layer, x.detach()[:, :100].contiguous())
    # with the switch off: exactly the module path
    a, b = copy.deepcopy(layer), copy.deepcopy(layer)
    CU.NATIVE_UNITS = False
    try:
        keep = {}
        got = CU.forward_units(a, x, keep=keep)
        assert "NATIVE_UNITS" in CU.native_reason(a, x) and not keep
    finally:
        CU.NATIVE_UNITS = True
    assert torch.equal(got, b(x))
    for (n1, b1), (_, b2) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(b1, b2), n1
    # a percentile QuantAct keeps the module path, with the module path's result
    a, b = copy.deepcopy(layer), copy.deepcopy(layer)
    for m in (a, b):
        m[1].quant_act2.percentile = True
    assert "percentile" in CU.native_reason(a, x) and "quant_act2" in CU.native_reason(a, x)
    assert torch.equal(CU.forward_units(a, x), b(x))
    # a forward hook on a sub-module fires: the module path
    c = copy.deepcopy(layer)
    fired = []
    c[0].quant_convbn4.register_forward_hook(lambda mod, inp, out: fired.append(1))
    assert "hook" in CU.native_reason(c, x)
    keep = {}
    CU.forward_units(c, x, keep=keep)
    assert fired and not keep
    # without the hook the same layer runs natively (keep is filled), and so does layer4
    CU.forward_units(copy.deepcopy(layer), x, keep=keep)
    assert sorted(keep) == list(range(len(layer)))
    l4a, l4b = copy.deepcopy(model.layer4), copy.deepcopy(model.layer4)
    x4 = (torch.randint(0, 256, (2, 464, 4, 4), generator=torch.Generator().manual_seed(5)).float() / 32).cuda().requires_grad_(True)
    assert CU.native_reason(l4a, x4) is None
    y4 = CU.forward_layer4(l4a, x4)
    assert y4.shape == (2, 1024, 4, 4) and y4.grad_fn is not None and "ReluQuant" in type(y4.grad_fn).__name__
    assert float(l4a[1][1].x_max) > 0 and float(l4b[1][1].x_max) == 0      # the QuantAct's range moved in place
    with torch.no_grad():      # grad mode off: forward is unchanged -- the module path, whatever the switch says
        m1, m2 = copy.deepcopy(model), copy.deepcopy(model)
        img = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(6)).cuda()
        assert "grad" in CU.native_reason(m1.layer1, m1.layer0(img))
        o1 = m1(img)[0]
        CU.NATIVE_UNITS = False
        try:
            o2 = m2(img)[0]
        finally:
            CU.NATIVE_UNITS = True
        assert all(torch.equal(o1[k], o2[k]) for k in o1)
