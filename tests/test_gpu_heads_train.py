"""The quantised detection heads of the QAT step on the native path (functions/codenet_heads.py,
csrc/codenet_heads_train.hip): forward and backward against the module path.

1. `test_exact_arithmetic_*`: the construction of tests/test_gpu_exact_codes.py -- inputs on which every summation order
   gives the same float32 (dyadic weights, power-of-two quantiser scales, small integers) -- so the native path must be
   torch.equal to the CPU module path on every output and every gradient, eagerly and replayed from a HIP graph.
2. `test_own_intermediates_*`: random weights, running ranges.  The oracle's QuantAct on the native path's own
   relu(y1) / r2 must track the device's ranges bit for bit, and every new kernel's output must agree with a float64
   evaluation from the native path's own intermediates within the order-independent bound
   |got - ref| <= 1.01 (n + 2) 2^-24 S  (n terms, S the float64 sum of their magnitudes).
3. `test_detection_tail_*`: stages -> heads -> CtdetLoss as one captured step, bit-identical to the eager step, accepted
   by GraphedTrainStep without `unvalidated`; two runs from one seed end bit-identical.
4. `test_gating_*`: what takes the native path and what keeps the module path.

Smallest shapes at which the kernels can go wrong: N = 2, C = 64, planes 12 x 20 (rows no multiple of the 8-row strip),
16 x 16 and 9 x 10 (width no multiple of 4: the scalar-load path), heads 20 / 2 / 2 and one case with 80 classes.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from oracle import quant as Q
from tests import qat_support

pytestmark = pytest.mark.gpu

HEADS = ("hm", "wh", "reg")
CASES = [(12, 20, 20), (16, 16, 20), (9, 10, 20), (16, 16, 80)]      # (H, W, classes of hm)


_model, _codes, _fq32, _bound, _within = (qat_support.model, qat_support.codes, qat_support.fq32, qat_support.bound,
                                          qat_support.within)


def _heads_of(model):
    return {h: getattr(model, h) for h in model.heads}


# ---- 1. exact arithmetic -------------------------------------------------------------------------------------------------

def exact_heads(classes, seed=5):
    """The heads of a quantised model with weights / BatchNorms / ranges on which every float32 sum is exact."""
    g = torch.Generator().manual_seed(seed)
    heads = copy.deepcopy(_heads_of(_model(classes)))
    ints = lambda n, lo, hi: torch.randint(lo, hi + 1, (n,), generator=g).float()      # noqa: E731
    with torch.no_grad():
        for name, m in heads.items():
            co = m.quant_conv.weight.shape[0]
            m.quant_convbn1.conv.weight.copy_((_codes(g, 64, 64, 3) / 8).view(64, 64, 1, 1))
            m.quant_convbn2.conv.weight.copy_((_codes(g, 64, 9, 9) / 16).view(64, 1, 3, 3))
            m.quant_conv.weight.copy_((_codes(g, co, 64, 4 if name == "hm" else 32) / 8).view(co, 64, 1, 1))
            m.quant_conv.bias.copy_(ints(co, -8, 8) / 8)
            for cb in (m.quant_convbn1, m.quant_convbn2):
                assert cb.conv.bias is None
                cb.bn.eps = 0.0
                cb.bn.running_var.fill_(1.0)
                cb.bn.running_mean.zero_()
                cb.bn.weight.fill_(1.0)
                cb.bn.bias.copy_(ints(64, -8, 8) / 8)
            for seq, hi in ((m.quant_act1, 255.0 / 16), (m.quant_act3, 255.0 / 8)):
                seq[1].running_stat = False
                seq[1].x_min.zero_()
                seq[1].x_max.fill_(hi)
    return heads


def exact_inputs(heads, H, W, seed=6):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 32, (2, 64, H, W), generator=g).float() / 16
    gy = {h: torch.randint(-2, 3, (2, m.quant_conv.weight.shape[0], H, W), generator=g).float() for h, m in heads.items()}
    return x, gy


def run_heads(heads, x, gy, dtype=None, fn=None):
    """forward + backward of the heads on fresh copies -> (outputs, x.grad, {parameter name: grad})."""
    heads = copy.deepcopy(heads)
    if dtype is not None:
        heads = {h: m.to(dtype) for h, m in heads.items()}
        x, gy = x.to(dtype), {h: v.to(dtype) for h, v in gy.items()}
    x = x.detach().clone().requires_grad_(True)
    for m in heads.values():
        m.train()
    out = fn(heads, x) if fn is not None else {h: m(x) for h, m in heads.items()}
    sum((out[h] * gy[h]).sum() for h in heads).backward()
    grads = {"%s.%s" % (h, n): p.grad for h, m in heads.items() for n, p in m.named_parameters()}
    assert all(v is not None for v in grads.values())
    return {h: v.detach() for h, v in out.items()}, x.grad, grads


_EXACT = {}


def exact_case(H, W, classes):
    """The CPU module-path reference of one exact case (computed once), with the construction asserts."""
    key = (H, W, classes)
    if key not in _EXACT:
        heads = exact_heads(classes)
        x, gy = exact_inputs(heads, H, W)
        o32, gx32, g32 = run_heads(heads, x, gy)
        o64, gx64, g64 = run_heads(heads, x, gy, dtype=torch.float64)
        # the construction: float32 equals float64 bit for bit, so no summation order can change a float32
        for h in heads:
            assert torch.equal(o32[h].double(), o64[h]), h
        assert torch.equal(gx32.double(), gx64)
        for n in g32:
            assert torch.equal(g32[n].double(), g64[n]), n
        for h in heads:      # enough of the backward is exercised
            live = int((g32["%s.quant_convbn2.conv.weight" % h].abs().sum((1, 2, 3)) > 0).sum())
            assert live >= 24, (h, live)
        assert float((gx32 != 0).float().mean()) >= 0.40
        _EXACT[key] = (heads, x, gy, o32, gx32, g32)
    return _EXACT[key]


def _to_cuda(heads):
    return {h: copy.deepcopy(m).cuda() for h, m in heads.items()}


@pytest.mark.parametrize("H,W,classes", CASES)
def test_exact_arithmetic_forward_and_backward_equal_the_cpu_module_path(H, W, classes):
    from codenet_amd.functions import codenet_heads as CH
    heads, x, gy, o_ref, gx_ref, g_ref = exact_case(H, W, classes)
    dev = _to_cuda(heads)
    for m in dev.values():
        m.train()
    xs = x.cuda().requires_grad_(True)
    gys = {h: v.cuda() for h, v in gy.items()}
    assert CH.native_reason(dev, xs) is None
    params = {"%s.%s" % (h, n): p for h, m in dev.items() for n, p in m.named_parameters()}

    def step():
        out = CH.forward_heads(dev, xs)
        sum((out[h] * gys[h]).sum() for h in dev).backward()
        return out

    def check(out, what):
        for h in dev:
            assert torch.equal(out[h].detach().cpu(), o_ref[h]), (what, h)
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
    # the same step replayed from a graph
    xs.grad = None
    for p in params.values():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    with torch.no_grad():
        xs.grad.fill_(float("nan"))
        for p in params.values():
            p.grad.fill_(float("nan"))
        for h in dev:
            out[h].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    check(out, "graph replay")


# ---- 2. running ranges, real arithmetic on the kernels' own intermediates ------------------------------------------------

def _project(got, ref, what, rel=3e-6):
    """The project's bound for the existing pointwise / weight-gradient kernels (tests/test_train_step.py)."""
    err = float((got.double().cpu() - ref).abs().max())
    print("%-28s max err %.3e of max |ref| %.3e" % (what, err, float(ref.abs().max())))
    assert err <= rel * float(ref.abs().max()), what


@pytest.mark.parametrize("H,W,classes", CASES)
def test_own_intermediates_through_the_oracle_quantiser_and_float64(H, W, classes):
    from codenet_amd import _native as N_
    from codenet_amd import ops
    from codenet_amd.functions import codenet_heads as CH
    from codenet_amd.functions import codenet_stage as CS
    model = _model(classes)
    heads = {h: m.cuda().train() for h, m in _heads_of(model).items()}
    acts = {h: (m.quant_act1[1], m.quant_act3[1]) for h, m in heads.items()}
    for pair in acts.values():
        for a in pair:
            assert a.running_stat
            a.x_min.zero_()
            a.x_max.zero_()
    mirrors = {h: (Q.QuantActState(), Q.QuantActState()) for h in heads}
    g = torch.Generator().manual_seed(11 + H)
    N, C = 2, 64

    def grid_input():
        return (torch.randint(0, 256, (N, C, H, W), generator=g).float() / 32).cuda()

    def check_ranges(keep, what):
        for h in heads:
            y1, r2 = keep[h]["y1"].cpu(), keep[h]["r2"].cpu()
            for m, t, a in ((mirrors[h][0], torch.relu(y1), acts[h][0]), (mirrors[h][1], r2, acts[h][1])):
                m.update(t)
                assert torch.equal(m.x_min, a.x_min.cpu()) and torch.equal(m.x_max, a.x_max.cpu()), \
                    "%s %s: oracle (%r, %r) vs device (%r, %r)" % (what, h, m.x_min, m.x_max, a.x_min, a.x_max)

    # forward 1: the "+=" initialisation, through the public entry
    keep = {}
    x0 = grid_input()
    assert CH.native_reason(heads, x0) is None
    out0 = CH.forward_heads(heads, x0, keep=keep)
    assert all(out0[h].shape == (N, heads[h].quant_conv.weight.shape[0], H, W) for h in heads)
    check_ranges(keep, "forward 1")
    module_copy = copy.deepcopy(heads)      # the module path from the same state, for the code-flip share
    # forward 2: one EMA step, on leaf copies of the prepared weights so that their gradients can be read
    x = grid_input().requires_grad_(True)
    names = list(heads)
    mods = [heads[h] for h in names]
    with torch.enable_grad():
        flat = [t.detach().clone().requires_grad_(True) if t is not None else None
                for six in CH._prepared_weights(mods) for t in six]
    meta = tuple((h, m.quant_act1[1], m.quant_act3[1]) for h, m in zip(names, mods))
    keep = {}
    outs = CH.CodenetHeadsFunction.apply(x, meta, keep, *flat)
    check_ranges(keep, "forward 2")
    gy = [torch.randn(o.shape, generator=g).cuda() for o in outs]
    torch.autograd.backward(outs, gy)
    torch.cuda.synchronize()

    lib, st = N_.lib(), torch.cuda.current_stream().cuda_stream
    xd = x.detach().double().cpu()
    gy1_all, w1_all = [], []
    for i, h in enumerate(names):
        w1, b1, w2, b2, w3, b3 = flat[6 * i: 6 * i + 6]
        y1, r2 = keep[h]["y1"], keep[h]["r2"]
        a1m, a3m = mirrors[h]
        Co = w3.shape[0]
        a1 = _fq32(torch.relu(y1.cpu()), a1m.x_min, a1m.x_max).double()
        a2 = _fq32(r2.cpu(), a3m.x_min, a3m.x_max).double()
        W2, W3 = w2.detach().double().cpu(), w3.detach().double().cpu().view(Co, C)
        # -- the depthwise forward: r2
        ref = F.conv2d(a1, W2, b2.detach().double().cpu(), 1, 1, 1, C)
        S = F.conv2d(a1.abs(), W2.abs(), b2.detach().double().cpu().abs(), 1, 1, 1, C)
        _within(r2, torch.relu(ref), 10, S, "%s r2" % h)
        # -- y3
        ref3 = torch.einsum("oc,nchw->nohw", W3, a2) + b3.detach().double().cpu().view(1, Co, 1, 1)
        S3 = torch.einsum("oc,nchw->nohw", W3.abs(), a2.abs()) + b3.detach().double().cpu().abs().view(1, Co, 1, 1)
        if Co <= 4:
            _within(outs[i].detach(), ref3, C + 1, S3, "%s y3 (small tail)" % h)
        else:
            _project(outs[i].detach(), ref3, "%s y3 (pointwise)" % h)
        # the code-flip share against the module path on the GPU: explained by the two checks above, not a criterion
        with torch.no_grad():
            y_mod = module_copy[h](x.detach())
        flips = ((y_mod.double().cpu() - outs[i].detach().double().cpu()).abs() > _bound(C + 1, S3)).double().mean()
        print("%s: share of y3 elements beyond the re-association bound of the module path: %.4f" % (h, float(flips)))
        # -- the depthwise backward, called as the function calls it: its own grad_y1 (a slice of a wider buffer)
        gyh = gy[i].contiguous()
        if Co <= 4:
            gsrc, w3p, co = gyh, w3.detach(), Co
            ga2 = torch.einsum("oc,nohw->nchw", W3, gyh.double().cpu())
            Sa2 = torch.einsum("oc,nohw->nchw", W3.abs(), gyh.double().cpu().abs())
            terms = Co
        else:
            gsrc = ops.codenet_pointwise(gyh, w3.detach().reshape(Co, C).t().contiguous().view(C, Co, 1, 1))
            _project(gsrc, torch.einsum("oc,nohw->nchw", W3, gyh.double().cpu()), "%s grad_a2 (pointwise)" % h)
            w3p, co = None, 0
            ga2 = gsrc.double().cpu()
            Sa2, terms = ga2.abs(), 1
        wide = torch.full((N, 2 * C, H, W), float("nan"), device="cuda")
        gw2, gb2 = torch.full((C, 9), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        need = lib.cdn_codenet_head_dw_backward_workspace_bytes(N, C, H, W)
        ws = torch.full((need // 4 + 64,), float("nan"), device="cuda")
        snap1 = acts[h][0]._device_state(x.device)
        rc = lib.cdn_codenet_head_dw_backward(gsrc.data_ptr(), w3p.data_ptr() if w3p is not None else None, co,
                                              r2.data_ptr(), y1.data_ptr(), snap1.data_ptr(), w2.data_ptr(),
                                              wide.data_ptr() + 4 * C * H * W, 2 * C * H * W, gw2.data_ptr(), gb2.data_ptr(),
                                              N, C, H, W, ws.data_ptr(), ws.numel() * 4, st)
        N_.check(rc, "cdn_codenet_head_dw_backward")
        torch.cuda.synchronize()
        assert torch.isnan(wide[:, :C]).all()      # the other head's slice is untouched
        gy1 = wide[:, C:]
        mask2 = (r2.cpu() > 0).double()
        gy2, Sy2 = ga2 * mask2, Sa2 * mask2
        Wm = W2.flip(2, 3)      # grad_a1[q] = sum_t W[t] grad_y2[q - t]: the correlation with the mirrored taps
        ref = F.conv2d(gy2, Wm, None, 1, 1, 1, C) * (y1.cpu() > 0).double()
        S = F.conv2d(Sy2, Wm.abs(), None, 1, 1, 1, C)
        _within(gy1, ref, 9 * terms, S, "%s grad_y1" % h)
        # grad_W2q[c, t] = sum_{n, p} grad_y2[p] a1[p + t], grad_b2[c] = sum grad_y2
        a1p, n_sum = F.pad(a1, (1, 1, 1, 1)), N * H * W * terms
        ref_w = torch.stack([(gy2 * a1p[:, :, dy:dy + H, dx:dx + W]).sum((0, 2, 3)) for dy in range(3) for dx in range(3)], 1)
        S_w = torch.stack([(Sy2 * a1p[:, :, dy:dy + H, dx:dx + W].abs()).sum((0, 2, 3)) for dy in range(3) for dx in range(3)], 1)
        _within(gw2, ref_w, n_sum, S_w, "%s grad_W2q" % h)
        _within(gb2, gy2.sum((0, 2, 3)), n_sum, Sy2.sum((0, 2, 3)), "%s grad_b2" % h)
        # what the autograd function returned for the same inputs is the same launch: bit-identical
        assert torch.equal(w2.grad.view(C, 9), gw2) and torch.equal(b2.grad, gb2), h
        # -- grad_W3q / grad_b3
        ref_w3 = torch.einsum("nohw,nchw->oc", gyh.double().cpu(), a2)
        ref_b3 = gyh.double().cpu().sum((0, 2, 3))
        if Co <= 4:
            S_w3 = torch.einsum("nohw,nchw->oc", gyh.double().cpu().abs(), a2.abs())
            _within(w3.grad.view(Co, C), ref_w3, N * H * W, S_w3, "%s grad_W3q (small tail)" % h)
            _within(b3.grad, ref_b3, N * H * W, gyh.double().cpu().abs().sum((0, 2, 3)), "%s grad_b3 (small tail)" % h)
        else:
            _project(w3.grad.view(Co, C), ref_w3, "%s grad_W3q" % h)
            _project(b3.grad, ref_b3, "%s grad_b3" % h)
        gy1_all.append(gy1.double().cpu())
        w1_all.append(w1.detach().double().cpu().view(C, C))
        _project(w1.grad.view(C, C), torch.einsum("nohw,nchw->oc", gy1_all[-1], xd), "%s grad_W1q" % h)
        _project(b1.grad, gy1_all[-1].sum((0, 2, 3)), "%s grad_b1" % h)
    ref_gx = sum(torch.einsum("oc,nohw->nchw", w, g1) for w, g1 in zip(w1_all, gy1_all))
    _project(x.grad, ref_gx, "grad_x")


# ---- 3. reproducibility and capture -------------------------------------------------------------------------------------

def _tail():
    from codenet_amd import pipeline
    return qat_support.train_net(pipeline.DetectionTail)


def _tail_setup():
    return qat_support.step_setup(lambda g, N, R: torch.randn(N, 1024, 4, 4, generator=g).abs_() * 1.66, 5)


def test_detection_tail_captured_step_replays_the_eager_step_bit_for_bit():
    from codenet_amd import pipeline
    from codenet_amd.functions import codenet_heads as CH
    loss_fn, feats = _tail_setup()
    eager, (net_g, opt_g) = [qat_support.with_capturable_adam(_tail()) for _ in range(2)]
    assert pipeline.GraphedTrainStep.is_native_tail(net_g) and not pipeline.GraphedTrainStep.is_stage_stack(net_g)
    assert CH.native_reason(net_g.head_modules(), torch.empty(2, 64, 32, 32, device="cuda")) is None
    # four steps; every head took part in the loss
    qat_support.check_captured_step(eager, (net_g, opt_g), loss_fn, feats, lambda n: n.split(".")[0] in HEADS)
    # with the switch off the same net runs the framework's backward: not accepted as validated
    CH.NATIVE_HEADS = False
    try:
        assert not pipeline.GraphedTrainStep.is_native_tail(net_g)
        with pytest.raises(NotImplementedError):
            pipeline.GraphedTrainStep(net_g, opt_g, loss_fn, (feats[0],))
    finally:
        CH.NATIVE_HEADS = True


def test_detection_tail_two_identical_runs_end_bit_identical():
    loss_fn, feats = _tail_setup()
    qat_support.check_two_identical_runs(_tail, loss_fn, feats[:4])


# ---- 4. gating ---------------------------------------------------------------------------------------------------------------

def test_gating_on_the_gpu():
    from codenet_amd.functions import codenet_heads as CH
    model = _model().cuda().train()
    x = (torch.rand(2, 64, 16, 16, generator=torch.Generator().manual_seed(4)) * 4).cuda().requires_grad_(True)
    assert CH.native_reason(_heads_of(model), x) is None
    assert "contiguous" in CH.native_reason(_heads_of(model), x.detach().transpose(2, 3))
    # a percentile QuantAct keeps the module path, with the module path's result
    a, b = copy.deepcopy(_heads_of(model)), copy.deepcopy(_heads_of(model))
    for hs in (a, b):
        hs["wh"].quant_act3[1].percentile = True
    assert "percentile" in CH.native_reason(a, x)
    # (both sides are the module path, whose 1x1 convolutions are the framework's: on some machines its default
    # algorithm gives one of two results, 1 ulp apart, from call to call -- so the two evaluations ask for its
    # deterministic algorithms; the comparison stays an equality)
    with torch.backends.cudnn.flags(deterministic=True):
        got, want = CH.forward_heads(a, x), {h: m(x) for h, m in b.items()}
    assert all(torch.equal(got[h], want[h]) for h in a)
    # a forward hook on a sub-module fires: the module path
    c = copy.deepcopy(_heads_of(model))
    fired = []
    c["hm"].quant_act1.register_forward_hook(lambda mod, inp, out: fired.append(1))
    assert "hook" in CH.native_reason(c, x)
    keep = {}
    CH.forward_heads(c, x, keep=keep)
    assert fired and not keep
    # without the hook the same heads run natively (keep is filled)
    CH.forward_heads(copy.deepcopy(_heads_of(model)), x, keep=keep)
    assert set(keep) == set(HEADS)
