"""The restatement of the fp32 stem (tests/stem_fp32_ref.py) against the framework's float64
operators, the gate of functions/codenet_stem_fp32.py, the module path on CPU tensors, the GraphedTrainStep predicates and
the argument errors of the new entry points -- everything that needs no GPU.  The cases built here are the GPU tests' too
(tests/test_gpu_stem_fp32.py)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from tests import bn_block_ref as R
from tests import stem_fp32_ref as SR
from tests.test_bn_block_host import gy_bound
from tests.test_units_fp32_host import CAP, REL, _z64, close

F = np.float32
U = R.U32

# the image shapes of the GPU test (DESIGN.md section 4.3h says which path each one reaches)
S4_SHAPES = [(2, 3, 20, 28), (1, 3, 17, 23), (2, 3, 64, 256), (3, 3, 152, 200)]
S2_SHAPES = [(2, 3, 18, 26), (1, 3, 16, 24), (2, 3, 96, 128)]
CASES = [(s, 4) for s in S4_SHAPES] + [(s, 2) for s in S2_SHAPES]
IDS = ["s%d-%dx%dx%dx%d" % (st, *s) for s, st in CASES]
# The seed of every case's random inputs, chosen on the CPU: 1000, the first tried, for every case -- with it no element of the
# float64 reference lies within 8u S of the ReLU's kink and no window's runner-up within that distance of its winner (a share
# of at most CAP = 1e-4 may; test_seeds_of_the_gpu_cases_stay_under_the_cap_of_elements_left_out)
SEEDS = {i: 1000 for i in IDS}


def _grid(g, shape, lo, hi, den):
    return torch.randint(lo * den, hi * den + 1, shape, generator=g).float() / den


def make_stem(shape, stride, seed, exact, train=True):
    """(layer0, x, gout): the fp32 stem (stride 2: with the pool) with non-trivial BatchNorm parameters and buffers, an image
    and the gradient of its output.  exact: integers, halves and quarters (the convolution exact in float32), gamma of both
    signs, beta of both signs, channel 1 negative everywhere behind the BatchNorm (every window of it is <= 0) and channel 2
    a copy of one image tap (17 levels: equal positive values inside most windows)."""
    g = torch.Generator().manual_seed(seed)
    mods = [nn.Conv2d(3, 24, 3, stride, 1, bias=False), nn.BatchNorm2d(24, momentum=0.1), nn.ReLU(inplace=True)]
    if stride == 2:
        mods.append(nn.MaxPool2d(kernel_size=3, stride=2, padding=1))
    layer0 = nn.Sequential(*mods).train(train)
    conv, bn = layer0[0], layer0[1]
    sign = 1 - 2 * (torch.arange(24) % 3 == 0).float()
    with torch.no_grad():
        if exact:
            conv.weight.copy_(_grid(g, conv.weight.shape, -1, 1, 2))
            conv.weight[2].zero_()
            conv.weight[2, 1, 1, 1] = 1.0
            bn.weight.copy_(_grid(g, (24,), 1, 2, 4) * sign)
            bn.bias.copy_(_grid(g, (24,), -1, 1, 4))
            bn.weight[1], bn.bias[1] = 1.0, -64.0
            bn.weight[2], bn.bias[2] = 1.0, 0.25
        else:
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * 0.2)
            bn.weight.copy_((torch.randn(24, generator=g) * 0.25 + 1.0) * sign)
            bn.bias.copy_(torch.randn(24, generator=g) * 0.3)
        bn.running_mean.copy_(_grid(g, (24,), -1, 1, 4))
        bn.running_var.copy_(_grid(g, (24,), 1, 3, 4))
    Nb, _, Hh, W = shape
    Ho, Wo = SR.out_hw(Hh, W, stride)
    if stride == 2:
        Ho, Wo = SR.out_hw(Ho, Wo, 2)
    if exact:
        x, gout = _grid(g, shape, -2, 2, 4), _grid(g, (Nb, 24, Ho, Wo), -2, 2, 4)
    else:
        x, gout = torch.randn(shape, generator=g), torch.randn(Nb, 24, Ho, Wo, generator=g)
    return layer0, x, gout


def params_of(layer0):
    conv, bn = layer0[0], layer0[1]
    return dict(stride=int(conv.stride[0]), eps=bn.eps, momentum=bn.momentum, train=bool(bn.training),
                w=conv.weight.detach().cpu().numpy().reshape(24, 27), gamma=bn.weight.detach().cpu().numpy(),
                beta=bn.bias.detach().cpu().numpy(), rm=bn.running_mean.cpu().numpy().copy(),
                rv=bn.running_var.cpu().numpy().copy())


def restate(layer0, x, gout, given=None, mutate=()):
    return SR.stem(x.cpu().numpy(), params_of(layer0), gout.cpu().numpy(), given=given, mutate=mutate)


def module_path_64(layer0, x, gout):
    """The stem in float64 under the framework's autograd: (out, {name: grad}, the double copy)."""
    l64 = copy.deepcopy(layer0).double()
    out = l64(x.double())
    out.backward(gout.double())
    return out.detach(), {k: v.grad for k, v in l64.named_parameters()}, l64


def left_out_share(p, y0):
    """The share of y0's elements the float32 path may treat differently from float64: |z64| <= 8u S (the ReLU's kink) or,
    with the pool, a window whose winner is positive and whose runner-up lies within 8u S (the larger S of the window) of
    it.  z64, S: F.batch_norm in float64 on the float32 y0, batch statistics (tests/test_units_fp32_host._z64)."""
    z64, S = _z64(y0, p["gamma"], p["beta"], p["eps"])
    share = float((z64.abs() <= R.K_Z * U * S).double().mean())
    if p["stride"] == 2:
        a = z64.clamp_min(0.0)
        top, idx = Fn.max_pool2d(a, 3, 2, 1, return_indices=True)
        rest = a.flatten(2).scatter(2, idx.flatten(2), -1.0).view_as(a)
        second = Fn.max_pool2d(rest, 3, 2, 1)
        tie = (top > 0) & (top - second <= R.K_Z * U * Fn.max_pool2d(S, 3, 2, 1))
        share = max(share, float(tie.double().mean()))
    return share


@pytest.mark.parametrize("shape,stride", CASES[:2] + CASES[4:6], ids=IDS[:2] + IDS[4:6])
def test_whole_stem_against_layer0_double(shape, stride):
    """The restatement on the float32 module path's own y0 against layer0.double() under autograd: out, grad_W, grad_gamma,
    grad_beta and the running buffers within 2e-4 of the tensor's magnitude; z within 8u S and grad_y0 within 23u B of the
    float64 BatchNorm on that y0 (sections 4.3e / f).  Nothing is left out with the chosen seeds.  (The larger planes are
    left to the GPU test: the comparison is the same.)"""
    layer0, x, gout = make_stem(shape, stride, SEEDS["s%d-%dx%dx%dx%d" % (stride, *shape)], exact=False)
    p = params_of(layer0)
    with torch.no_grad():
        y0 = layer0[0](x)
    ref = restate(layer0, x, gout, given={"y0": y0.numpy()})
    assert left_out_share(p, ref["y0"]) <= CAP
    out, grads, l64 = module_path_64(layer0, x, gout)
    close(ref["out"], out.numpy(), "out")
    close(ref["grad_w_64"], grads["0.weight"].numpy().reshape(24, 27), "grad_W")
    close(ref["grad_gamma"], grads["1.weight"].numpy(), "grad_gamma")
    close(ref["grad_beta"], grads["1.bias"].numpy(), "grad_beta")
    close(ref["rm"], l64[1].running_mean.numpy(), "running_mean")
    close(ref["rv"], l64[1].running_var.numpy(), "running_var")
    # the stages on the float32 y0
    t = lambda v: torch.from_numpy(np.asarray(v, F)).double()      # noqa: E731
    z64, S = _z64(ref["y0"], p["gamma"], p["beta"], p["eps"])
    assert bool(((t(ref["z"]) - z64).abs() <= 1.01 * R.K_Z * U * S).all())
    y = t(ref["y0"]).requires_grad_(True)
    Fn.relu(Fn.batch_norm(y, None, None, t(p["gamma"]), t(p["beta"]), True, 0.0, p["eps"])).backward(t(ref["G"]))
    yd = y.detach()
    mean, invstd = yd.mean((0, 2, 3)), 1.0 / torch.sqrt(yd.var((0, 2, 3), unbiased=False) + p["eps"])
    B = gy_bound(yd, t(p["gamma"]), mean, invstd, t(ref["g_z"]), 1)
    assert bool(((t(ref["grad_y0"]) - y.grad).abs() <= 1.01 * R.K_GY * U * B).all())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_seeds_of_the_gpu_cases_stay_under_the_cap_of_elements_left_out(i):
    shape, stride = CASES[i]
    layer0, x, gout = make_stem(shape, stride, SEEDS[IDS[i]], exact=False)
    assert left_out_share(params_of(layer0), restate(layer0, x, gout)["y0"]) <= CAP


def test_pool_restatement_is_the_frameworks_on_exact_inputs_and_tells_its_wrong_variants_apart():
    """On the coarse grid (ties everywhere) the restated pool and its gather are F.max_pool2d's, forward and backward; the
    two wrong variants differ from the restatement where they should."""
    layer0, x, gout = make_stem((2, 3, 18, 26), 2, 11, exact=True)
    ref = restate(layer0, x, gout)
    a0 = torch.from_numpy(ref["a0"]).requires_grad_(True)
    out = Fn.max_pool2d(a0, 3, 2, 1)
    out.backward(gout)
    assert np.array_equal(ref["out"], out.detach().numpy()) and np.array_equal(ref["G"], a0.grad.numpy())
    assert not ref["a0"][:, 1].any() and not ref["g_z"][:, 1].any()      # the channel whose every window is <= 0
    assert not np.array_equal(restate(layer0, x, gout, mutate=("y0max",))["out"], ref["out"])
    # (the order of a pixel's additions shows in the rounding alone: a random gradient on the same ties)
    grand = torch.randn(gout.shape, generator=torch.Generator().manual_seed(12))
    assert not np.array_equal(restate(layer0, x, grand, mutate=("order",))["g_z"], restate(layer0, x, grand)["g_z"])


# ---- the gate ------------------------------------------------------------------------------------------------------------

def _model(**kw):
    from codenet_amd import harness
    return harness.PoseShuffleNetV2({"hm": 20, "wh": 2, "reg": 2}, 64, **kw)


def test_gate_refuses_with_a_reason_that_names_the_cause():
    from codenet_amd import harness
    from codenet_amd.functions import codenet_stem, codenet_stem_fp32 as S32
    for maxpool in (False, True):
        assert S32.native_reason(_model(maxpool=maxpool).layer0, None) is None
    layer0 = _model().layer0
    assert "cpu tensor" in S32.native_reason(layer0, torch.zeros(2, 3, 16, 16))
    assert "requires grad" in S32.native_reason(layer0, torch.zeros(2, 3, 16, 16, requires_grad=True))
    S32.NATIVE_FP32_STEM = False
    try:
        assert S32.native_reason(layer0, None) == "NATIVE_FP32_STEM is off"
    finally:
        S32.NATIVE_FP32_STEM = True
    with torch.no_grad():
        assert "grad mode is off" in S32.native_reason(layer0, None)

    def broken(change, maxpool=False):
        mm = _model(maxpool=maxpool)
        change(mm.layer0)
        return S32.native_reason(mm.layer0, None)

    def bias(l0):
        l0[0] = nn.Conv2d(3, 24, 3, 4, 1, bias=True)
    assert "has a bias" in broken(bias)

    def stride3(l0):
        l0[0] = nn.Conv2d(3, 24, 3, 3, 1, bias=False)
    assert "geometry" in broken(stride3)
    assert "geometry" in broken(lambda l0: l0.__setitem__(0, nn.Conv2d(3, 24, 3, 4, 1, bias=False)), maxpool=True)

    def ceil(l0):
        l0[3] = nn.MaxPool2d(3, 2, 1, ceil_mode=True)
    assert "ceil_mode" in broken(ceil, maxpool=True)

    def momentum(l0):
        l0[1].momentum = None
    assert "momentum=None" in broken(momentum)

    def affine(l0):
        l0[1] = nn.BatchNorm2d(24, affine=False)
    assert "affine=False" in broken(affine)

    def hook(l0):
        l0[1].register_forward_hook(lambda *a: None)
    assert "a hook on sub-module '1'" in broken(hook)
    q = harness.create_model(heads={"hm": 20, "wh": 2, "reg": 2}, quantize=True)
    assert "not exactly Sequential(Conv2d, BatchNorm2d, ReLU" in S32.native_reason(q.layer0, None)
    # the quantised stem's gate and its messages stay as they are
    assert codenet_stem.native_reason(q.layer0, None) is None
    assert "the fp32 stem keeps the module path" in codenet_stem.native_reason(layer0, None)


@pytest.mark.parametrize("maxpool", [False, True])
@pytest.mark.parametrize("grad", [True, False])
def test_forward_stem_on_cpu_tensors_is_the_module_path_bit_for_bit(grad, maxpool):
    from codenet_amd.functions.codenet_stem import forward_stem
    m = _model(maxpool=maxpool).train()
    a, b = copy.deepcopy(m), copy.deepcopy(m)
    x = torch.randn(2, 3, 32, 32)
    with torch.set_grad_enabled(grad):
        y1, y2 = forward_stem(a.layer0, x), b.layer0(x)
    assert torch.equal(y1, y2)
    for u, v in zip(a.buffers(), b.buffers()):
        assert torch.equal(u, v)


def test_is_fp32_net_and_the_older_predicates():
    from codenet_amd import harness, pipeline
    from codenet_amd.functions import codenet_stem_fp32 as S32
    G = pipeline.GraphedTrainStep
    for maxpool in (False, True):
        m = _model(maxpool=maxpool)
        net, trunk, tail = pipeline.DetectionNet(m), pipeline.DetectionTrunk(m), pipeline.DetectionTail(m)
        assert G.is_fp32_net(net)
        with torch.no_grad():
            assert G.is_fp32_net(net)      # a property of the modules
        assert not G.is_fp32_net(trunk) and not G.is_fp32_net(tail) and not G.is_fp32_net(m)
        assert not G.is_native_net(net) and not G.is_native_trunk(net) and not G.is_native_tail(net)
        assert not G.is_fp32_trunk(net) and not G.is_fp32_tail(net) and not G.is_stage_stack(net)
        assert not G.is_fp32_stage_stack(net)
        assert G.is_fp32_trunk(trunk) and G.is_fp32_tail(tail)
    q = harness.create_model(heads={"hm": 20, "wh": 2, "reg": 2}, quantize=True)
    assert not G.is_fp32_net(pipeline.DetectionNet(q)) and G.is_native_net(pipeline.DetectionNet(q))
    hooked = _model()
    hooked.layer0[0].register_forward_hook(lambda *a: None)
    assert not G.is_fp32_net(pipeline.DetectionNet(hooked))
    hooked_units = _model()
    hooked_units.layer2[3].b2[0].register_forward_hook(lambda *a: None)
    assert not G.is_fp32_net(pipeline.DetectionNet(hooked_units))
    S32.NATIVE_FP32_STEM = False
    try:
        assert not G.is_fp32_net(net)
    finally:
        S32.NATIVE_FP32_STEM = True


def test_constructor_judges_the_example_image():
    from codenet_amd import pipeline
    from codenet_amd.functions import codenet_stem_fp32 as S32
    G = pipeline.GraphedTrainStep
    net = pipeline.DetectionNet(_model())
    with pytest.raises(NotImplementedError, match="layer0: the fp32 stem: no example image to judge"):
        G(net, None, None, [])
    with pytest.raises(NotImplementedError, match="layer0: the fp32 stem: x requires grad"):
        G(net, None, None, [torch.zeros(2, 3, 64, 64, requires_grad=True)])
    with pytest.raises(NotImplementedError, match="layer0: the fp32 stem: x is a cpu tensor"):
        G(net, None, None, [torch.zeros(2, 3, 64, 64)])
    S32.NATIVE_FP32_STEM = False
    try:
        with pytest.raises(NotImplementedError, match="layer0: the fp32 stem: NATIVE_FP32_STEM is off"):
            G(net, None, None, [torch.zeros(2, 3, 64, 64)])
    finally:
        S32.NATIVE_FP32_STEM = True
    # a stem and an image the gate accepts in front of a trunk it refuses: the trunk's reason is shown, not "None"
    hooked = _model()
    hooked.layer2[3].b2[0].register_forward_hook(lambda *a: None)
    ok = S32.native_reason
    S32.native_reason = lambda layer0, x: ok(layer0, None)      # (stands for a GPU image: this test has no GPU)
    try:
        with pytest.raises(NotImplementedError, match=r"the fp32 network \([^\[\]]*\) "      # (the scope's own words)
                                                      r"\[layer2: the layer: a hook on sub-module .3.b2.0."):
            G(pipeline.DetectionNet(hooked), None, None, [torch.zeros(2, 3, 64, 64)])
    finally:
        S32.native_reason = ok


# ---- the entry points ----------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("cdn_codenet_stem_fp32_workspace_bytes", "cdn_codenet_stem_fp32_pool_forward",
               "cdn_codenet_stem_fp32_pool_backward", "cdn_codenet_stem_fp32_bn_relu_backward_sums",
               "cdn_codenet_stem_fp32_wgrad_workspace_bytes", "cdn_codenet_stem_fp32_wgrad")


def test_the_library_exports_the_new_entry_points():
    import os
    from codenet_amd import _native
    lib = _native.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "codenet_dcn.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _native._SIGNATURES and s in header, s


def test_argument_errors_come_back_before_any_launch():
    from codenet_amd import _native
    lib = _native.lib()
    one, big = 4096, 1 << 24
    ARG, UNSUPPORTED, WORKSPACE = -1, -5, -6

    def pool_fwd(y0=one, mean=one, out=one, N=2, C=24, H=9, W=13):
        return lib.cdn_codenet_stem_fp32_pool_forward(y0, mean, one, one, one, out, N, C, H, W, None)

    assert pool_fwd(y0=None) == ARG and pool_fwd(mean=None) == ARG and pool_fwd(out=None) == ARG
    assert pool_fwd(N=0) == ARG and pool_fwd(C=0) == ARG and pool_fwd(H=-1) == ARG and pool_fwd(W=0) == ARG
    assert pool_fwd(N=64, C=24, H=2048, W=2048) == UNSUPPORTED

    need = lib.cdn_codenet_stem_fp32_workspace_bytes(2, 24, 48, 64)
    assert need == (24 * 2 * 16 + 255) // 256 * 256                # two slabs of 4096 per channel
    assert lib.cdn_codenet_stem_fp32_workspace_bytes(0, 24, 8, 8) == 0
    assert lib.cdn_codenet_stem_fp32_workspace_bytes(2, 24, 8, -8) == 0
    assert lib.cdn_codenet_stem_fp32_workspace_bytes(64, 24, 2048, 2048) == 0      # (what the calls refuse as UNSUPPORTED)

    def pool_bwd(g=one, y0=one, gz=one, mb=one, N=2, C=24, H=48, W=64, ws=one, nbytes=big):
        return lib.cdn_codenet_stem_fp32_pool_backward(g, y0, one, one, one, one, gz, one, one, mb, one, N, C, H, W, ws, nbytes,
                                                       None)

    def sums(g=one, y0=one, mb=one, N=2, C=24, H=48, W=64, ws=one, nbytes=big):
        return lib.cdn_codenet_stem_fp32_bn_relu_backward_sums(g, y0, one, one, one, one, one, one, mb, one, N, C, H, W, ws,
                                                               nbytes, None)

    for call in (pool_bwd, sums):
        assert call(g=None) == ARG and call(y0=None) == ARG and call(mb=None) == ARG and call(ws=None) == ARG
        assert call(N=0) == ARG and call(W=0) == ARG
        assert call(N=64, C=24, H=2048, W=2048) == UNSUPPORTED
        assert call(nbytes=need - 1) == WORKSPACE and call(ws=one + 4) == WORKSPACE
    assert pool_bwd(gz=None) == ARG

    wneed = lib.cdn_codenet_stem_fp32_wgrad_workspace_bytes(2, 96, 128, 2)
    assert wneed == lib.cdn_codenet_stem_backward_workspace_bytes(2, 96, 128, 2) == (6 * 4 * 112 * 4 + 255) // 256 * 256
    assert lib.cdn_codenet_stem_fp32_wgrad_workspace_bytes(2, 96, 128, 3) == 0
    assert lib.cdn_codenet_stem_fp32_wgrad_workspace_bytes(0, 96, 128, 2) == 0
    assert lib.cdn_codenet_stem_fp32_wgrad_workspace_bytes(4096, 1024, 1024, 2) == 0

    def wgrad(g=one, y0=one, img=one, mb=one, gw=one, N=2, H=96, W=128, Co=24, stride=2, training=1, ws=one, nbytes=big):
        return lib.cdn_codenet_stem_fp32_wgrad(g, 1, y0, img, one, one, one, one, mb, one, gw, N, H, W, Co, stride, training, ws,
                                               nbytes, None)

    assert wgrad(g=None) == ARG and wgrad(y0=None) == ARG and wgrad(img=None) == ARG and wgrad(gw=None) == ARG
    assert wgrad(mb=None) == ARG and wgrad(ws=None) == ARG
    assert wgrad(Co=16) == ARG and wgrad(stride=3) == ARG and wgrad(stride=1) == ARG and wgrad(N=0) == ARG
    assert wgrad(N=4096, H=1024, W=1024) == UNSUPPORTED
    assert wgrad(nbytes=wneed - 1) == WORKSPACE and wgrad(ws=one + 4) == WORKSPACE
