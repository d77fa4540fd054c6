"""The native fp32 ShuffleNetV2 units and layer4 on the GPU (csrc/codenet_units_fp32_train.hip,
functions/codenet_units_fp32.py) against their numpy restatement (tests/units_fp32_ref.py), against
float64 on the GPU's own operands, against the float32 module path, behind the gate and as a captured training step.

What is compared how.  Everything the library's own fixed-order kernels leave -- y2, y4, z2, z4, out, every BatchNorm's
numbers, buffers and counter, g_z3 / 5, grad_y3 / 5, g_z1, grad_y1, the gradients of W2 / W4 and of every gamma / beta, the
pass-through half of grad_x and the sum of both branches' grad_x -- is `torch.equal` to the restatement, which follows the
kernels' sum orders, evaluated on the GPU's own pointwise results (y1, y3, y5 and the pointwise data gradients), on ANY
input.  The dense 1x1 convolutions run on MFMA kernels whose order is not restated: their outputs and gradients are held to
float64 on the GPU's own operands within (n + 2) 2^-24 sum |terms| and must be bit-identical across the eager run and the
replays."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import bn_block_ref as R
from tests import qat_support
from tests.test_units_fp32_host import (CAP, EXTRA_CASES, IDS, LAYER4_SHAPES, UNIT_CASES, cancelling_magnitudes, close,
                                        convs_bns, make_case, params_of, restate, stage_fractions)

pytestmark = pytest.mark.gpu

CASES = UNIT_CASES + EXTRA_CASES
GB_NAMES = {1: ("b2.1.weight", "b2.1.bias"), 2: ("b2.4.weight", "b2.4.bias"), 3: ("b2.6.weight", "b2.6.bias"),
            4: ("b1.1.weight", "b1.1.bias"), 5: ("b1.3.weight", "b1.3.bias")}


def _np(t):
    return t.detach().cpu().numpy()


def _eq(got, want):
    return torch.equal(got.detach().cpu().reshape(-1), torch.from_numpy(np.ascontiguousarray(want)).reshape(-1))


def _forward_backward(node, xd, gd, keep, native=True):
    from codenet_amd.functions import codenet_units as CU, codenet_units_fp32 as U32
    U32.NATIVE_FP32_UNITS = native
    try:
        with torch.backends.cudnn.flags(deterministic=True):
            out = CU.forward_units(node, xd, keep)
            out.backward(gd)
    finally:
        U32.NATIVE_FP32_UNITS = True
    return out


def _run(node, x, gout, native=True):
    """One forward + backward of forward_units on the GPU on a copy of `node`: (keep of the unit, out, grad_x, the copy)."""
    node = copy.deepcopy(node).cuda()
    xd = x.cuda().requires_grad_(True)
    keep = {}
    out = _forward_backward(node, xd, gout.cuda(), keep, native)
    return keep.get(0, {}), out, xd.grad, node


def _given(k, stride, h):
    g = dict(y1=_np(k["y1"]), y3=_np(k["y3"]), grad_z2=_np(k["grad_z2"]))
    if stride == 2:
        g.update(y5=_np(k["y5"]), grad_z4=_np(k["grad_z4"]), grad_x2=_np(k["grad_x_b2"]))
    else:
        g["grad_x2"] = _np(k["grad_x"][:, h:])
    return g


def _check(k, out, gx, node, ref, step):
    """torch.equal to the restatement `ref` (of the unit's state before the first step) after `step` steps on one batch."""
    stride = int(node.stride)
    for name in ("y2", "z2", "out") + (("y4", "z4") if stride == 2 else ()):
        assert _eq(k[name], ref[name]), name
    assert _eq(out, ref["out"])
    for i, (_, bn) in enumerate(convs_bns(node), 1):
        st = ref["st"][i]
        assert all(_eq(a, st[key]) for a, key in zip(k["bn%d" % i], ("mean", "var", "invstd"))), i
        rm, rv = ref["rm%d" % i], ref["rv%d" % i]
        for _ in range(step - 1):
            rm, rv = R.running_update(rm, rv, st, bn.momentum)
        assert _eq(bn.running_mean, rm) and _eq(bn.running_var, rv), i
        assert int(bn.num_batches_tracked) == step, i
    g = {n: p.grad for n, p in node.named_parameters()}
    pairs = [("g_z3", ref["join3"]["g_z"]), ("grad_y3", ref["grad_y3"]), ("g_z1", ref["dw2"]["g_z"]), ("grad_y1", ref["grad_y1"])]
    sums = {1: ref["dw2"], 2: ref["bn2"], 3: ref["join3"]}
    if stride == 2:
        pairs += [("g_z5", ref["join5"]["g_z"]), ("grad_y5", ref["grad_y5"])]
        sums.update({4: ref["bn4"], 5: ref["join5"]})
    for name, want in pairs:
        assert _eq(k[name], want), name
    for i, s in sums.items():
        assert _eq(k["means%d" % i][0], s["mb"]) and _eq(k["means%d" % i][1], s["mg"]), i
        assert _eq(g[GB_NAMES[i][0]], s["grad_gamma"]) and _eq(g[GB_NAMES[i][1]], s["grad_beta"]), i
    assert _eq(g["b2.3.weight"], ref["dw2"]["grad_w"])
    if stride == 2:
        assert _eq(g["b1.0.weight"], ref["dw4"]["grad_w"])
    assert _eq(gx, ref["grad_x"]) and _eq(k["grad_x"], ref["grad_x"])


def _pointwise_results(k, gx, node, x):
    """Every result of an MFMA kernel, in a fixed order: for the float64 bounds and the bit comparison between runs."""
    g = {n: p.grad for n, p in node.named_parameters()}
    stride, h = int(node.stride), k["y1"].shape[1]
    res = [k["y1"], k["y3"], k["grad_z2"], g["b2.0.weight"], g["b2.5.weight"],
           k["grad_x_b2"] if stride == 2 else gx[:, h:]]
    if stride == 2:
        res += [k["y5"], k["grad_z4"], g["b1.2.weight"]]
    return [t.detach().clone() for t in res]


def _pointwise_within_float64(k, gx, node, x, what):
    """(n + 2) 2^-24 sum |terms| of float64 on the GPU's own operands (qat_support.within) for every MFMA result."""
    stride, h = int(node.stride), k["y1"].shape[1]
    d = lambda t: t.detach().double().cpu()      # noqa: E731
    g = {n: d(p.grad) for n, p in node.named_parameters()}
    w = {n: d(p).reshape(p.shape[0], -1) for n, p in node.named_parameters() if p.dim() == 4 and p.shape[1] > 1}
    x2 = d(x) if stride == 2 else d(x)[:, h:]

    def fwd(got, wt, src, name):
        qat_support.within(got, torch.einsum("oc,nchw->nohw", wt, src), wt.shape[1],
                           torch.einsum("oc,nchw->nohw", wt.abs(), src.abs()), "%s %s" % (what, name))

    def wgrad(got, gy, src, name):
        n = gy.shape[0] * gy.shape[2] * gy.shape[3]
        qat_support.within(got.reshape(gy.shape[1], -1), torch.einsum("nohw,nchw->oc", gy, src), n,
                           torch.einsum("nohw,nchw->oc", gy.abs(), src.abs()), "%s %s" % (what, name))

    fwd(k["y1"], w["b2.0.weight"], x2, "y1")
    fwd(k["y3"], w["b2.5.weight"], d(k["z2"]), "y3")
    fwd(k["grad_z2"], w["b2.5.weight"].t(), d(k["grad_y3"]), "grad_z2")
    fwd(k["grad_x_b2"] if stride == 2 else gx[:, h:], w["b2.0.weight"].t(), d(k["grad_y1"]), "grad_x2")
    wgrad(g["b2.0.weight"], d(k["grad_y1"]), x2, "grad_W1")
    wgrad(g["b2.5.weight"], d(k["grad_y3"]), d(k["z2"]), "grad_W3")
    if stride == 2:
        fwd(k["y5"], w["b1.2.weight"], d(k["z4"]), "y5")
        fwd(k["grad_z4"], w["b1.2.weight"].t(), d(k["grad_y5"]), "grad_z4")
        wgrad(g["b1.2.weight"], d(k["grad_y5"]), d(k["z4"]), "grad_W5")


@pytest.mark.parametrize("shape,h,stride", CASES, ids=IDS)
def test_intermediates_eager_and_on_two_graph_replays(shape, h, stride):
    """Coarse-grid inputs (integers, halves and quarters; the 5 x 7 case with beta1 > 0, where a padded tap computed as
    relu(bn_z(0)) shows): every intermediate the new kernels write, every BatchNorm number, buffer and counter and every
    gradient they sum are the restatement's bit for bit -- eagerly, and after each of two replays of a HIP graph of the same
    calls (the buffers advance three times); the MFMA results within (n + 2) 2^-24 sum |terms| of float64 on the GPU's own
    operands, and bit-identical across the three."""
    node, x, gout = make_case(shape, h, stride, 11, exact=True, beta1_positive=(shape[2:] == (5, 7)))
    side = torch.cuda.Stream()      # (eager run and capture on one stream: the parameters' autograd nodes live there)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        k, out, gx, nd = _run(node, x, gout)
    torch.cuda.synchronize()
    assert k, "the native path did not run"
    ref = restate(node, x, gout, given=_given(k, stride, h))
    _check(k, out, gx, nd, ref, 1)
    _pointwise_within_float64(k, gx, nd, x, "eager")
    first = _pointwise_results(k, gx, nd, x)
    xd, gd = x.cuda().requires_grad_(True), gout.cuda()
    nd.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keep = {}
    with torch.cuda.graph(graph, stream=side):
        out = _forward_backward(nd, xd, gd, keep)
    for step in (2, 3):
        for t in [xd.grad, out] + [p.grad for p in nd.parameters()]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _check(keep[0], out, xd.grad, nd, ref, step)
        assert all(torch.equal(a, b) for a, b in zip(_pointwise_results(keep[0], xd.grad, nd, x), first))


@functools.lru_cache(maxsize=None)
def _random(i):
    """The random inputs of case i, the GPU's native result and the restatement on the GPU's own pointwise results, computed
    once."""
    shape, h, stride = CASES[i]
    node, x, gout = make_case(shape, h, stride, 1000 + i, exact=False)
    k, out, gx, nd = _run(node, x, gout)
    assert k, "the native path did not run"
    return node, x, gout, k, out, gx, nd, restate(node, x, gout, given=_given(k, stride, h))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_own_intermediates_on_random_inputs(i):
    """Random inputs: the same equalities to the restatement on the GPU's own pointwise results, the MFMA results within
    (n + 2) 2^-24 sum |terms| of float64 on the GPU's own operands, and every stage within the derived bounds of float64
    (tests/test_units_fp32_host.stage_fractions)."""
    shape, h, stride = CASES[i]
    node, x, gout, k, out, gx, nd, ref = _random(i)
    _check(k, out, gx, nd, ref, 1)
    _pointwise_within_float64(k, gx, nd, x, "random")
    # `ref` is the GPU's own result (just compared): every stage within the derived bounds of float64 on the GPU's operands
    worst, left_out = stage_fractions(params_of(node), ref, x, gout, stride)
    print("largest seen fraction of each bound:", worst, "left out:", left_out)
    assert left_out <= CAP and all(v <= 1.0 for v in worst.values()), (worst, left_out)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_native_against_the_module_path(i):
    """Native against NATIVE_FP32_UNITS = False on the GPU: out, grad_x, every parameter gradient and every buffer within
    2e-4 of the tensor's magnitude -- for the tensors tests/test_units_fp32_host.cancelling_magnitudes names (grad_beta2 / 4,
    zero in exact arithmetic, in every case; every gradient in front of a training-mode BatchNorm where a channel has two
    values), of their sum of |terms|; `keep` is filled only when native."""
    shape, h, stride = CASES[i]
    node, x, gout, k, out, gx, nd, ref = _random(i)
    k0, out0, gx0, nd0 = _run(node, x, gout, native=False)
    assert not k0
    assert type(out0.grad_fn).__name__ != "CodenetUnitFp32FunctionBackward"
    assert type(out.grad_fn).__name__ == "CodenetUnitFp32FunctionBackward"
    mags = cancelling_magnitudes(params_of(node), ref, x, stride)
    seen = {"out": close(_np(out), _np(out0), "out"), "grad_x": close(_np(gx), _np(gx0), "grad_x", mag=mags.get("grad_x"))}
    for (n1, p1), (_, p0) in zip(nd.named_parameters(), nd0.named_parameters()):
        seen[n1] = close(_np(p1.grad), _np(p0.grad), n1, mag=mags.get(n1))
    for (n1, b1), (_, b0) in zip(nd.named_buffers(), nd0.named_buffers()):
        seen[n1] = close(_np(b1), _np(b0), n1)
    print("largest share of a magnitude:", max(seen.items(), key=lambda kv: kv[1]))


@pytest.mark.parametrize("shape", LAYER4_SHAPES, ids=["%dx%dx%dx%d" % s for s in LAYER4_SHAPES])
def test_layer4_native_against_restatement_and_module_path(shape):
    """layer4 = relu(bn(pw(x, W))): the pointwise kernel and the fused BatchNorm + ReLU (section 4.3e's kernels, up = 1).  out
    is the restatement's R.forward on the GPU's own pointwise output with the kernels' own statistics within float64's
    channel bound, and out, grad_x, the parameter gradients and the buffers are within 2e-4 of the module path's."""
    from codenet_amd import harness
    from codenet_amd.functions import codenet_units as CU, codenet_units_fp32 as U32
    g = torch.Generator().manual_seed(5)
    layer4 = harness.PoseShuffleNetV2({"hm": 20}, 64).layer4.train()
    x, gout = torch.randn(shape, generator=g), torch.randn(shape[0], 1024, *shape[2:], generator=g)
    res = []
    for native in (True, False):
        l4 = copy.deepcopy(layer4).cuda()
        xd = x.cuda().requires_grad_(True)
        U32.NATIVE_FP32_UNITS = native
        try:
            assert (U32.native_reason(l4, xd) is None) == native
            out = CU.forward_layer4(l4, xd)
            out.backward(gout.cuda())
        finally:
            U32.NATIVE_FP32_UNITS = True
        res.append((out, xd.grad, l4))
    (o1, gx1, m1), (o0, gx0, m0) = res
    assert type(o1.grad_fn).__name__ == "BnReluUpsampleBackward" and type(o0.grad_fn).__name__ != "BnReluUpsampleBackward"
    close(_np(o1), _np(o0), "out")
    close(_np(gx1), _np(gx0), "grad_x")
    for (n1, p1), (_, p0) in zip(m1.named_parameters(), m0.named_parameters()):
        close(_np(p1.grad), _np(p0.grad), n1)
    for (n1, b1), (_, b0) in zip(m1.named_buffers(), m0.named_buffers()):
        close(_np(b1), _np(b0), n1)
    assert int(m1[1].num_batches_tracked) == 1


def test_each_batchnorm_in_eval_mode_writes_no_buffer():
    """Each BatchNorm of a stride-2 unit in turn in eval mode under grad: its buffers and counter stay, the others advance,
    and everything is still the restatement's bit for bit."""
    shape, h, stride = (2, 24, 9, 10), 58, 2
    for which in range(5):
        node, x, gout = make_case(shape, h, stride, 40 + which, exact=False)
        convs_bns(node)[which][1].eval()
        k, out, gx, nd = _run(node, x, gout)
        assert k
        ref = restate(node, x, gout, given=_given(k, stride, h))
        for i, ((_, bn), (_, bn0)) in enumerate(zip(convs_bns(nd), convs_bns(node))):
            if i == which:
                assert torch.equal(bn.running_mean.cpu(), bn0.running_mean) and torch.equal(bn.running_var.cpu(), bn0.running_var)
                assert int(bn.num_batches_tracked) == 0
            else:
                assert int(bn.num_batches_tracked) == 1
            assert _eq(bn.running_mean, ref["rm%d" % (i + 1)]) and _eq(bn.running_var, ref["rv%d" % (i + 1)])
        assert _eq(out, ref["out"]) and _eq(gx, ref["grad_x"])
        assert _eq(k["g_z1"], ref["dw2"]["g_z"]) and _eq(k["grad_y1"], ref["grad_y1"]) and _eq(k["grad_y5"], ref["grad_y5"])
        g = {n: p.grad for n, p in nd.named_parameters()}
        assert _eq(g["b2.3.weight"], ref["dw2"]["grad_w"]) and _eq(g["b1.0.weight"], ref["dw4"]["grad_w"])


def test_gating_on_the_gpu():
    """One value per channel raises the framework's error before any launch; a hooked inner module takes the module path and
    its hook fires; a quantised layer still takes the QAT path; no_grad takes the module path."""
    from codenet_amd import harness
    from codenet_amd.functions import codenet_units as CU, codenet_units_fp32 as U32
    node, x, gout = make_case((1, 116, 1, 1), 58, 1, 3, exact=True)
    nd = node.cuda()
    before = [b.clone() for b in nd.buffers()]
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        CU.forward_units(nd, x.cuda().requires_grad_(True))
    assert all(torch.equal(a, b) for a, b in zip(before, nd.buffers()))
    node, x, gout = make_case((2, 116, 9, 10), 58, 1, 3, exact=False)
    nd = copy.deepcopy(node).cuda()
    fired = []
    nd.b2[3].register_forward_hook(lambda *a: fired.append(1))
    xd = x.cuda().requires_grad_(True)
    assert "a hook on sub-module 'b2.3'" in U32.native_reason(nd, xd)
    keep = {}
    out = CU.forward_units(nd, xd, keep)
    assert fired and not keep and type(out.grad_fn).__name__ != "CodenetUnitFp32FunctionBackward"
    nd = copy.deepcopy(node).cuda()
    with torch.no_grad():
        a = CU.forward_units(nd, x.cuda())
    b = copy.deepcopy(node).cuda()(x.cuda())
    assert torch.equal(a, b)
    for reason, t in (("16-byte aligned float32", torch.zeros(2 * 116 * 90 + 1, device="cuda")[1:].view(2, 116, 9, 10)),
                      ("expects 116 input channels, x has 24", torch.zeros(2, 24, 9, 10, device="cuda")),
                      ("x must be a contiguous", torch.zeros(2, 116, 10, 9, device="cuda").transpose(2, 3)),
                      ("got torch.float16", torch.zeros(2, 116, 9, 10, device="cuda", dtype=torch.float16)),
                      ("too large for 32-bit indexing", torch.zeros(65536, 116, 1, 1, device="cuda"))):
        assert reason in U32.native_reason(nd, t.requires_grad_(True)), reason
    assert "not a float32 tensor on x's device" in U32.native_reason(copy.deepcopy(node), x.cuda().requires_grad_(True))
    assert "nothing to differentiate" in U32.native_reason(copy.deepcopy(nd).requires_grad_(False), x.cuda())
    q = harness.create_model(heads={"hm": 20, "wh": 2, "reg": 2}, quantize=True).cuda().train()
    x0 = torch.rand(2, 24, 8, 8, device="cuda", requires_grad=True)
    assert CU.native_reason(q.layer1, x0) is None
    assert type(CU.forward_units(q.layer1, x0).grad_fn).__name__ == "CodenetUnitFunctionBackward"


# ---- the captured step --------------------------------------------------------------------------------------------------

def _trunk():
    from codenet_amd import harness, pipeline
    return pipeline.DetectionTrunk(harness.create_model(heads={"hm": 20, "wh": 2, "reg": 2})).cuda().train()


def _trunk_setup(count=5):
    """CtdetLoss on the native criterion over fixed targets at N = 2 on 16 x 16 maps -- layer0's features of a 64 x 64
    image -- and `count` feature tensors drawn in turn from one generator."""
    from codenet_amd.losses import CtdetLoss, ctdet_targets
    N, M, R_ = 2, 8, 16
    crit = CtdetLoss(qat_support.default_opt())
    batch = ctdet_targets(*qat_support.objects(N, M, R_, R_, 3), 20, R_, R_, M)

    def loss_fn(net, x):
        out = net(x)
        assert crit.native_reason(out, batch) is None
        return crit(out, batch)[0]

    g = torch.Generator().manual_seed(2)
    return loss_fn, [(torch.randn(N, 24, 16, 16, generator=g).abs_() * 0.7).cuda() for _ in range(count)]


def test_fp32_trunk_captured_step_replays_the_eager_step_bit_for_bit():
    """GraphedTrainStep(DetectionTrunk(fp32 model).train(), capturable Adam, CtdetLoss) WITHOUT unvalidated=True (on the
    parent commit: NotImplementedError): replays bit-identical to eager steps in loss, parameters, BatchNorm buffers and
    Adam state; every parameter of layers 1-4 took part."""
    from codenet_amd import pipeline
    from codenet_amd.functions import codenet_units_fp32 as U32
    loss_fn, feats = _trunk_setup()
    eager, (net_g, opt_g) = [qat_support.with_capturable_adam(_trunk()) for _ in range(2)]
    G = pipeline.GraphedTrainStep
    assert G.is_fp32_trunk(net_g) and not G.is_native_trunk(net_g) and not G.is_fp32_tail(net_g)
    assert U32.native_reason(net_g.layer1, feats[0].clone().requires_grad_(True)) is None
    qat_support.check_captured_step(eager, (net_g, opt_g), loss_fn, feats, lambda n: n.split(".")[0].startswith("layer"))
    assert int(net_g.layer1[0].b1[1].num_batches_tracked) == 7 and int(net_g.layer4[1].num_batches_tracked) == 7
    U32.NATIVE_FP32_UNITS = False      # with the switch off the same net runs the framework's backward: not validated
    try:
        assert not G.is_fp32_trunk(net_g)
        with pytest.raises(NotImplementedError, match="NATIVE_FP32_UNITS is off"):
            G(net_g, opt_g, loss_fn, (feats[0],))
    finally:
        U32.NATIVE_FP32_UNITS = True


def test_fp32_trunk_two_identical_runs_end_bit_identical():
    loss_fn, feats = _trunk_setup(4)
    qat_support.check_two_identical_runs(_trunk, loss_fn, feats)
