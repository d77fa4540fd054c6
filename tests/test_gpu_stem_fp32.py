"""The native fp32 stem on the GPU (csrc/codenet_stem_fp32_train.hip, functions/codenet_stem_fp32.py) against its numpy
restatement (tests/stem_fp32_ref.py), against float64 on the GPU's own operands, against the float32
module path, behind the gate and as a captured training step from the image.

What is compared how.  Everything the new kernels and the BatchNorm kernels leave -- out, the BatchNorm's numbers, buffers
and counter, g_z (the pooled stem), mb / mg, grad_gamma, grad_beta -- is `torch.equal` to the restatement, which follows the
kernels' sum orders, evaluated on the GPU's own y0, on ANY input.  grad_W is a float32 fma chain per thread whose order is not
restated: it is held to float64 on the restatement's grad_y0 (bit for bit the operands the kernel forms) within (n + 2) 2^-24
sum |terms| and must be bit-identical across the eager run and the replays; where every term is exact it is the float64 sum.

Image shapes (tests/test_stem_fp32_host.CASES).  Stride 4: [2,3,20,28] -> y0 5x7, the scalar tails; [1,3,17,23] -> 5x6, an odd
image with every right / bottom tap partly outside; [2,3,64,256] -> 16x64, the 16-byte path, one slab; [3,3,152,200] -> 38x50,
n = 5700: two slabs, the second partial, scalar with W % 4 != 0.  Stride 2 + pool: [2,3,18,26] -> 9x13 -> 5x7, clipped at all
four borders; [1,3,16,24] -> 8x12 -> 4x6; [2,3,96,128] -> 48x64, n = 6144: two slabs, the 16-byte path, four weight-gradient
chunks; [1,3,2,2] -> 1x1, one window."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import bn_block_ref as R
from tests import qat_support
from tests import stem_fp32_ref as SR
from tests.test_stem_fp32_host import CAP, CASES, IDS, SEEDS, close, left_out_share, make_stem, params_of, restate

pytestmark = pytest.mark.gpu

NATIVE = "CodenetStemFp32FunctionBackward"


def _np(t):
    return t.detach().cpu().numpy()


def _eq(got, want):
    a = got.detach().cpu().reshape(-1)
    b = torch.from_numpy(np.ascontiguousarray(want)).reshape(-1)
    return torch.equal(a, b) or (a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all()))


def _forward_backward(layer0, xd, gd, keep, native=True):
    from codenet_amd.functions import codenet_stem, codenet_stem_fp32 as S32
    S32.NATIVE_FP32_STEM = native
    try:
        with torch.backends.cudnn.flags(deterministic=True):
            out = codenet_stem.forward_stem(layer0, xd, keep)
            out.backward(gd)
    finally:
        S32.NATIVE_FP32_STEM = True
    return out


def _run(layer0, x, gout, native=True):
    """One forward + backward of forward_stem on the GPU on a copy of `layer0`: (keep, out, the copy)."""
    l0 = copy.deepcopy(layer0).cuda()
    keep = {}
    out = _forward_backward(l0, x.cuda(), gout.cuda(), keep, native)
    return keep, out, l0


def _check(k, out, l0, ref, step, start=0):
    """torch.equal to the restatement `ref` (of the stem's state before the first step) after `step` steps on one batch."""
    bn, st = l0[1], ref["st"]
    assert _eq(out, ref["out"]) and _eq(k["out"], ref["out"])
    assert all(_eq(a, st[key]) for a, key in zip(k["bn"], ("mean", "var", "invstd")))
    rm, rv = ref["rm"], ref["rv"]
    if bn.training:
        for _ in range(step - 1):
            rm, rv = R.running_update(rm, rv, st, bn.momentum)
        assert int(bn.num_batches_tracked) == start + step
    else:
        assert int(bn.num_batches_tracked) == start
    assert _eq(bn.running_mean, rm) and _eq(bn.running_var, rv)
    if k["pooled"]:
        assert _eq(k["g_z"], ref["g_z"])
    else:
        assert k["g_z"] is None
    assert _eq(k["means"][0], ref["mb"]) and _eq(k["means"][1], ref["mg"])
    assert _eq(bn.weight.grad, ref["grad_gamma"]) and _eq(bn.bias.grad, ref["grad_beta"])
    assert _eq(k["grad_gamma"], ref["grad_gamma"]) and _eq(k["grad_beta"], ref["grad_beta"])


def _grad_w_within_float64(l0, ref, what):
    """grad_W within (n + 2) 2^-24 sum |terms| of float64 on the kernel's own grad_y0 operands (the restatement's, equal bit
    for bit: every number they are formed from has just been compared)."""
    n = ref["y0"].shape[0] * ref["y0"].shape[2] * ref["y0"].shape[3]
    qat_support.within(l0[0].weight.grad.reshape(24, 27), torch.from_numpy(ref["grad_w_64"]), n,
                       torch.from_numpy(ref["grad_w_abs"]), "%s grad_W" % what)


@pytest.mark.parametrize("shape,stride", CASES, ids=IDS)
def test_intermediates_eager_and_on_two_graph_replays(shape, stride):
    """Coarse-grid inputs (integers, halves, quarters; gamma and beta of both signs; channel 1 with every window <= 0; channel
    2 with equal positive values inside its windows): everything the kernels write is the restatement's bit for bit --
    eagerly, and after each of two replays of a HIP graph of the same calls with the outputs NaN-filled in between (the
    buffers advance three times); grad_W within (n + 2) 2^-24 sum |terms| of float64 and bit-identical across the three."""
    layer0, x, gout = make_stem(shape, stride, 11, exact=True)
    side = torch.cuda.Stream()      # (eager run and capture on one stream: the parameters' autograd nodes live there)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        k, out, l0 = _run(layer0, x, gout)
    torch.cuda.synchronize()
    assert k, "the native path did not run"
    ref = restate(layer0, x, gout, given={"y0": _np(k["y0"])})
    assert _eq(k["y0"], restate(layer0, x, gout)["y0"])      # (the convolution is exact on the coarse grid)
    _check(k, out, l0, ref, 1)
    _grad_w_within_float64(l0, ref, "eager")
    first = l0[0].weight.grad.detach().clone()
    xd, gd = x.cuda(), gout.cuda()
    l0.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keep = {}
    with torch.cuda.graph(graph, stream=side):
        out = _forward_backward(l0, xd, gd, keep)
    for step in (2, 3):
        for t in [out, keep["y0"], keep["means"]] + ([keep["g_z"]] if stride == 2 else []) + [p.grad for p in l0.parameters()]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _check(keep, out, l0, ref, step)
        assert torch.equal(l0[0].weight.grad, first)


@pytest.mark.parametrize("shape,stride", [CASES[1], CASES[2], CASES[4], CASES[6]], ids=[IDS[1], IDS[2], IDS[4], IDS[6]])
def test_exact_terms_give_the_float64_weight_gradient(shape, stride):
    """Weights, image and gradient from the coarse grid, BatchNorm in eval mode with eps = 0, running_var = 1 / 4 and gamma a
    signed power of two: gamma invstd is a power of two, every term of grad_W is exact and so is every partial sum --
    grad_W is the float64 sum bit for bit, and nothing is written to the buffers."""
    layer0, x, gout = make_stem(shape, stride, 13, exact=True, train=False)
    bn = layer0[1]
    bn.eps = 0.0
    with torch.no_grad():
        bn.running_var.fill_(0.25)
        bn.weight.copy_(torch.tensor([1.0, -2.0, 0.5, 2.0] * 6))
        bn.bias[1] = 0.5
    k, out, l0 = _run(layer0, x, gout)
    assert k, "the native path did not run"
    ref = restate(layer0, x, gout, given={"y0": _np(k["y0"])})
    assert _eq(k["bn"][2], np.full(24, 2.0, np.float32))
    _check(k, out, l0, ref, 1)
    assert _eq(l0[0].weight.grad, ref["grad_w_64"].astype(np.float32))
    assert np.array_equal(ref["grad_w_64"].astype(np.float32).astype(np.float64), ref["grad_w_64"])


@functools.lru_cache(maxsize=None)
def _random(i):
    """The random inputs of case i, the GPU's native result and the restatement on the GPU's own y0, computed once."""
    shape, stride = CASES[i]
    layer0, x, gout = make_stem(shape, stride, SEEDS[IDS[i]], exact=False)
    k, out, l0 = _run(layer0, x, gout)
    assert k, "the native path did not run"
    return layer0, x, gout, k, out, l0, restate(layer0, x, gout, given={"y0": _np(k["y0"])})


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_own_intermediates_on_random_inputs(i):
    """Random inputs: the same equalities to the restatement on the GPU's own y0; y0 and grad_W within (n + 2) 2^-24 sum
    |terms| of float64 on the GPU's own operands."""
    layer0, x, gout, k, out, l0, ref = _random(i)
    _check(k, out, l0, ref, 1)
    _grad_w_within_float64(l0, ref, "random")
    p = params_of(layer0)
    pt = torch.from_numpy(SR.patches(x.numpy(), p["stride"])).double()
    w = torch.from_numpy(p["w"]).double()
    qat_support.within(k["y0"], torch.einsum("ok,nkhw->nohw", w, pt), 27,
                       torch.einsum("ok,nkhw->nohw", w.abs(), pt.abs()), "random y0")


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_native_against_the_module_path(i):
    """Native against NATIVE_FP32_STEM = False on the GPU: out, grad_W, grad_gamma, grad_beta and the buffers within 2e-4 of
    the tensor's magnitude; at most CAP of the GPU's own y0 lies where the two may part (the host test's rule: a float64 z
    within 8u S of zero, a window's runner-up within that distance of its winner; with the chosen seeds: none); `keep` is
    filled only when native and the grad_fn tells the paths apart."""
    layer0, x, gout, k, out, l0, ref = _random(i)
    k0, out0, l00 = _run(layer0, x, gout, native=False)
    assert not k0
    assert type(out0.grad_fn).__name__ != NATIVE and type(out.grad_fn).__name__ == NATIVE
    assert left_out_share(params_of(layer0), ref["y0"]) <= CAP
    seen = {"out": close(_np(out), _np(out0), "out")}
    for (n1, p1), (_, p0) in zip(l0.named_parameters(), l00.named_parameters()):
        seen[n1] = close(_np(p1.grad), _np(p0.grad), n1)
    for (n1, b1), (_, b0) in zip(l0.named_buffers(), l00.named_buffers()):
        seen[n1] = close(_np(b1), _np(b0), n1)
    print("largest share of a magnitude:", max(seen.items(), key=lambda kv: kv[1]))


@pytest.mark.parametrize("shape,stride", [((2, 3, 20, 28), 4), ((2, 3, 18, 26), 2), ((1, 3, 2, 2), 2)],
                         ids=["s4", "s2", "s2-1x1"])
def test_eval_mode_batchnorm_writes_no_buffer_and_keeps_a_nan(shape, stride):
    """BatchNorm in eval mode under grad: no buffer or counter is written and everything is the restatement's bit for bit (the
    1 x 1 plane too: one window).  With one NaN image pixel, out is NaN at exactly the module path's positions, and the pooled
    backward routes a window's gradient to a NaN element: no other element of a window that holds a NaN receives it."""
    layer0, x, gout = make_stem(shape, stride, 21, exact=False, train=False)
    k, out, l0 = _run(layer0, x, gout)
    assert k, "the native path did not run"
    ref = restate(layer0, x, gout, given={"y0": _np(k["y0"])})
    _check(k, out, l0, ref, 1)
    _grad_w_within_float64(l0, ref, "eval")
    for b, b0 in zip(l0.buffers(), layer0.buffers()):
        assert torch.equal(b.cpu(), b0)
    xn = x.clone()
    xn[0, 1, min(8, shape[2] - 1), min(12, shape[3] - 1)] = float("nan")      # (a pixel the stride-4 taps reach)
    k, out, l0 = _run(layer0, xn, gout)
    _, out0, _ = _run(layer0, xn, gout, native=False)
    assert bool(out.isnan().any()) and torch.equal(out.isnan(), out0.isnan())
    ref = restate(layer0, xn, gout, given={"y0": _np(k["y0"])})
    assert _eq(out, ref["out"])
    if stride == 2:
        assert _eq(k["g_z"], ref["g_z"])
        # every window that holds a NaN was won by a NaN element, so its gradient reaches no other element (and g_z, equal
        # to the restatement's, is 0 at the NaN itself: z > 0 is false there)
        a0, arg = ref["a0"], ref["arg"]
        flat = np.pad(a0, ((0, 0), (0, 0), (1, 2), (1, 2))).reshape(a0.shape[0], 24, -1)
        winner = np.take_along_axis(flat, SR._flat_index(arg, a0.shape[3]).reshape(a0.shape[0], 24, -1), axis=2)
        held = _np(torch.nn.functional.max_pool2d(torch.from_numpy(a0).isnan().float(), 3, 2, 1) > 0)
        assert held.any() and np.isnan(winner.reshape(arg.shape)[held]).all()
        assert not np.isnan(ref["g_z"]).any()


def test_gating_on_the_gpu():
    """The switch, no_grad, an image that requires grad and a non-contiguous image each take the module path with results
    equal to layer0(x); one value per channel in training mode raises the framework's error before any launch."""
    from codenet_amd.functions import codenet_stem, codenet_stem_fp32 as S32
    layer0, x, gout = make_stem((2, 3, 20, 28), 4, 3, exact=False)
    xd = x.cuda()

    def both(inp, **ctx):
        a, b = copy.deepcopy(layer0).cuda(), copy.deepcopy(layer0).cuda()
        keep = {}
        with torch.backends.cudnn.flags(deterministic=True):
            ya, yb = codenet_stem.forward_stem(a, inp, keep), b(inp)
        assert not keep and type(ya.grad_fn).__name__ != NATIVE
        assert torch.equal(ya, yb) and all(torch.equal(u, v) for u, v in zip(a.buffers(), b.buffers()))

    assert S32.native_reason(copy.deepcopy(layer0).cuda(), xd) is None
    S32.NATIVE_FP32_STEM = False
    try:
        both(xd)
    finally:
        S32.NATIVE_FP32_STEM = True
    with torch.no_grad():
        both(xd)
    both(xd.clone().requires_grad_(True))
    nc = torch.zeros(2, 3, 28, 20, device="cuda").transpose(2, 3).copy_(xd)
    assert "x must be a contiguous" in S32.native_reason(copy.deepcopy(layer0).cuda(), nc)
    both(nc)
    assert "not a float32 tensor on x's device" in S32.native_reason(copy.deepcopy(layer0), xd)
    assert "nothing to differentiate" in S32.native_reason(copy.deepcopy(layer0).cuda().requires_grad_(False), xd)
    tiny, x1, _ = make_stem((1, 3, 2, 2), 2, 3, exact=False)
    tiny = tiny.cuda()
    before = [b.clone() for b in tiny.buffers()]
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        codenet_stem.forward_stem(tiny, x1.cuda())
    assert all(torch.equal(a, b) for a, b in zip(before, tiny.buffers()))


# ---- the captured step --------------------------------------------------------------------------------------------------

def _net(maxpool):
    from codenet_amd import harness, pipeline
    return pipeline.DetectionNet(harness.create_model(heads={"hm": 20, "wh": 2, "reg": 2}, maxpool=maxpool)).cuda().train()


def _fused_adam(net):
    return net, torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device="cuda"), capturable=True, fused=True)


def _setup(count):
    """CtdetLoss on the native criterion over fixed targets at N = 2 on 32 x 32 maps and `count` 128 x 128 images."""
    return qat_support.step_setup(lambda g, N, R_: torch.rand(N, 3, 4 * R_, 4 * R_, generator=g), count)


@pytest.mark.parametrize("maxpool", [False, True], ids=["s4", "s2-pool"])
def test_fp32_net_captured_step_replays_the_eager_step_bit_for_bit(maxpool):
    """GraphedTrainStep(DetectionNet(fp32 model).train(), fused capturable Adam, CtdetLoss) WITHOUT unvalidated=True (on the
    parent commit: NotImplementedError): replays bit-identical to eager steps in loss, parameters, BatchNorm buffers and
    Adam state; every parameter of the stem and of layers 1-4 took part.  With the switch off the constructor refuses."""
    from codenet_amd import pipeline
    from codenet_amd.functions import codenet_stem_fp32 as S32
    loss_fn, imgs = _setup(5)
    eager, (net_g, opt_g) = [_fused_adam(_net(maxpool)) for _ in range(2)]
    G = pipeline.GraphedTrainStep
    assert G.is_fp32_net(net_g) and not G.is_native_net(net_g) and not G.is_fp32_trunk(net_g)
    assert S32.native_reason(net_g.layer0, imgs[0]) is None
    qat_support.check_captured_step(eager, (net_g, opt_g), loss_fn, imgs, lambda n: n.split(".")[0].startswith("layer"))
    assert int(net_g.layer0[1].num_batches_tracked) == 7 and int(net_g.layer4[1].num_batches_tracked) == 7
    S32.NATIVE_FP32_STEM = False      # with the switch off the same net runs the framework's backward: not validated
    try:
        assert not G.is_fp32_net(net_g)
        with pytest.raises(NotImplementedError, match="NATIVE_FP32_STEM is off"):
            G(net_g, opt_g, loss_fn, (imgs[0],))
    finally:
        S32.NATIVE_FP32_STEM = True


@pytest.mark.parametrize("maxpool", [False, True], ids=["s4", "s2-pool"])
def test_fp32_net_two_identical_runs_end_bit_identical(maxpool):
    loss_fn, imgs = _setup(4)
    qat_support.check_two_identical_runs(lambda: _net(maxpool), loss_fn, imgs)
