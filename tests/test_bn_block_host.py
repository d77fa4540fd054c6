"""Host side of the fp32 training block BatchNorm2d -> ReLU -> Upsample (functions/codenet_bn.py): the numpy restatement
of its arithmetic against the framework in float64, the gate's reasons, the GraphedTrainStep scope test and the library's
new entry points.  No GPU."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import bn_block_ref as R

NEW_SYMBOLS = ("cdn_codenet_bn_workspace_bytes", "cdn_codenet_bn_relu_up_forward", "cdn_codenet_bn_relu_up_backward")
SHAPES = [(2, 3, 5, 7), (3, 5, 9, 11), (1, 4, 16, 16), (2, 64, 8, 8), (2, 4, 96, 100), (2, 256, 16, 16)]
EPS, MOM = 1e-5, 0.1


def make_case(shape, up, seed):
    """The random inputs of the issue: y = 1.5 randn + 0.3, gamma in [0.5, 1.5), beta = 0.1 randn, a random gradient."""
    g = torch.Generator().manual_seed(seed)
    Nb, C, H, W = shape
    y = torch.randn(shape, generator=g) * 1.5 + 0.3
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    grad = torch.randn(Nb, C, up * H, up * W, generator=g)
    rm, rv = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    return y, gamma, beta, grad, rm, rv


def framework64(y, gamma, beta, grad, rm, rv, up, training=True):
    """F.batch_norm -> relu -> interpolate in float64 under autograd."""
    y64 = y.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    z = F.batch_norm(y64, rm64, rv64, g64, b64, training, MOM, EPS)
    z.retain_grad()
    out = F.relu(z)
    if up == 2:
        out = F.interpolate(out, scale_factor=2, mode="nearest")
    out.backward(grad.double())
    return dict(z=z.detach(), out=out.detach(), g_z=z.grad, grad_y=y64.grad, grad_gamma=g64.grad, grad_beta=b64.grad,
                running_mean=rm64, running_var=rv64)


def z_bound(y, gamma, beta, mean, invstd):
    """S of |z - z64| <= k 2^-24 S, from float64 per-channel numbers."""
    c = lambda v: v.reshape(1, -1, 1, 1)      # noqa: E731
    return c(gamma.abs()) * c(invstd) * (y.abs() + c(mean.abs())) + c(beta.abs())


def gy_bound(y, gamma, mean, invstd, grad, up):
    """|gamma| invstd (G + B1 + A B2) of the grad_y bound: G the sum of |grad| over an element's
    block, A = invstd (|y| + |mean|), B1 / B2 the channel means of G and G A."""
    c = lambda v: v.reshape(1, -1, 1, 1)      # noqa: E731
    G = grad.abs()
    if up == 2:
        G = G[:, :, 0::2, 0::2] + G[:, :, 0::2, 1::2] + G[:, :, 1::2, 0::2] + G[:, :, 1::2, 1::2]
    A = c(invstd) * (y.abs() + c(mean.abs()))
    B1, B2 = G.mean(dim=(0, 2, 3)), (G * A).mean(dim=(0, 2, 3))
    return c(gamma.abs()) * c(invstd) * (G + c(B1) + A * c(B2))


@pytest.mark.parametrize("up", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_restatement_agrees_with_the_framework_in_float64(shape, up):
    """The float32 restatement against F.batch_norm -> relu -> interpolate in float64: |z - z64| <= 8 * 2^-24 * S and
    |grad_y - grad_y64| <= 23 * 2^-24 * |gamma| invstd (G + B1 + A B2), the bounds DESIGN.md section 4.3e derives from the
    operation counts; the per-channel numbers within one float32 rounding plus the float64 accumulation.  Elements with
    |z64| <= 8 * 2^-24 * S (the ReLU could fall either way) would be left out of the ReLU-dependent comparisons: with this
    generator there are none.  (Measured: z reaches 3.8 of its 8, grad_y 2.4 of its 23.)"""
    y, gamma, beta, grad, rm, rv = make_case(shape, up, 1000 + up)
    ref = framework64(y, gamma, beta, grad, rm, rv, up)
    st = R.batch_stats(y.numpy(), EPS)
    n = st["n"]
    mean64 = y.double().mean(dim=(0, 2, 3))
    var64 = y.double().var(dim=(0, 2, 3), unbiased=False)
    assert np.all(np.abs(st["mean"] - mean64.numpy()) <= R.channel_bound(mean64.numpy(), n, st["abs1"] / n))
    assert np.all(np.abs(st["var"] - var64.numpy())
                  <= R.channel_bound(var64.numpy(), n, (st["s2"] / n + mean64.numpy() ** 2)))
    rm1, rv1 = R.running_update(rm.numpy(), rv.numpy(), st, MOM)
    # (three float32 operations on operands that carry one rounding each)
    assert np.all(np.abs(rm1 - ref["running_mean"].numpy()) <= 4 * R.U32 * (np.abs(rm.numpy()) + np.abs(mean64.numpy())))
    assert np.all(np.abs(rv1 - ref["running_var"].numpy()) <= 4 * R.U32 * (np.abs(rv.numpy()) + 2 * var64.numpy()))
    invstd64 = 1.0 / torch.sqrt(var64 + EPS)
    z, _ = R.bn_z(y.numpy(), st["mean"], st["invstd"], gamma.numpy(), beta.numpy())
    S = z_bound(y.double(), gamma.double(), beta.double(), mean64, invstd64)
    ratio = ((torch.from_numpy(z).double() - ref["z"]).abs() / (R.U32 * S)).max().item()
    assert ratio <= R.K_Z, ratio
    unsure = ref["z"].abs() <= R.K_Z * R.U32 * S
    assert unsure.sum().item() == 0
    out = R.forward(y.numpy(), st["mean"], st["invstd"], gamma.numpy(), beta.numpy(), up)
    S_up = torch.from_numpy(R.up2(S.numpy())) if up == 2 else S
    assert ((torch.from_numpy(out).double() - ref["out"]).abs() <= R.K_Z * R.U32 * S_up).all()
    bw = R.backward(grad.numpy(), y.numpy(), st["mean"], st["invstd"], gamma.numpy(), beta.numpy(), up)
    B = gy_bound(y.double(), gamma.double(), mean64, invstd64, grad.double(), up)
    gratio = ((torch.from_numpy(bw["grad_y"]).double() - ref["grad_y"]).abs() / (R.U32 * B)).max().item()
    assert gratio <= R.K_GY, gratio
    # the per-channel gradients: one rounding of a float64 sum whose terms carry the error of g_z (up 2: three float32
    # additions, 3 * 2^-24 * G) and of xh (6 * 2^-24 * A)
    G = grad.double().abs()
    if up == 2:
        G = G[:, :, 0::2, 0::2] + G[:, :, 0::2, 1::2] + G[:, :, 1::2, 0::2] + G[:, :, 1::2, 1::2]
    A = (invstd64.reshape(1, -1, 1, 1) * (y.double().abs() + mean64.abs().reshape(1, -1, 1, 1)))
    gb, gg = ref["grad_beta"].numpy(), ref["grad_gamma"].numpy()
    assert np.all(np.abs(bw["grad_beta"] - gb) <= R.U32 * (np.abs(gb) + 3 * G.sum(dim=(0, 2, 3)).numpy()))
    assert np.all(np.abs(bw["grad_gamma"] - gg) <= R.U32 * (np.abs(gg) + 9 * (G * A).sum(dim=(0, 2, 3)).numpy()))


def test_eval_mode_restatement_agrees_with_the_framework_in_float64():
    shape, up = (3, 5, 9, 11), 2
    y, gamma, beta, grad, rm, rv = make_case(shape, up, 7)
    ref = framework64(y, gamma, beta, grad, rm, rv, up, training=False)
    invstd = R.invstd_of(rv.numpy(), EPS)
    out = R.forward(y.numpy(), rm.numpy(), invstd, gamma.numpy(), beta.numpy(), up)
    assert np.allclose(out, ref["out"].numpy(), rtol=0, atol=1e-5)
    bw = R.backward(grad.numpy(), y.numpy(), rm.numpy(), invstd, gamma.numpy(), beta.numpy(), up, training=False)
    assert np.allclose(bw["grad_y"], ref["grad_y"].numpy(), rtol=1e-5, atol=1e-6)
    assert np.allclose(bw["grad_gamma"], ref["grad_gamma"].numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(ref["running_mean"], rm.double())      # (eval mode: the framework leaves the buffers alone too)


def test_the_library_exports_the_new_entry_points():
    from codenet_amd import _native
    lib = _native.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _native._SIGNATURES, s
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "codenet_dcn.h")).read()
    for s in NEW_SYMBOLS:
        assert s in header and "shufflenetv2_dcn.py:303-308" in header[header.index(s) - 200:header.index(s) + 200], s


def test_argument_errors_come_back_before_any_launch():
    from codenet_amd import _native
    lib = _native.lib()
    one, big = 4096, 1 << 24
    ARG, UNSUPPORTED, WORKSPACE = -1, -5, -6

    def fwd(y=one, gamma=one, out=one, rm=one, rv=one, N=2, C=4, H=8, W=8, up=2, training=1, ws=one, nbytes=big, mom=0.1):
        return lib.cdn_codenet_bn_relu_up_forward(y, gamma, one, rm, rv, one, one, one, one, out, N, C, H, W, up, training,
                                                  1e-5, mom, ws, nbytes, None)

    assert fwd(y=None) == ARG and fwd(gamma=None) == ARG and fwd(out=None) == ARG
    assert fwd(N=0) == ARG and fwd(C=-1) == ARG and fwd(H=0) == ARG and fwd(W=0) == ARG
    assert fwd(up=0) == ARG and fwd(up=3) == ARG
    assert fwd(y=one + 4) == ARG                                  # not 16-byte aligned
    assert fwd(N=1, H=1, W=1) == ARG                              # batch statistics of one value per channel
    assert fwd(rm=None) == ARG and fwd(mom=1.5) == ARG
    assert fwd(training=0, rm=None, rv=None) == ARG               # eval mode without running statistics
    assert fwd(N=64, C=256, H=512, W=512) == UNSUPPORTED
    need = lib.cdn_codenet_bn_workspace_bytes(2, 4, 96, 100)
    assert need == (4 * 5 * 16 + 255) // 256 * 256 + 256          # five slabs of 4096 per channel
    assert fwd(H=96, W=100, nbytes=need - 1) == WORKSPACE and fwd(ws=one + 4) == WORKSPACE and fwd(ws=None) == ARG
    assert lib.cdn_codenet_bn_workspace_bytes(0, 4, 8, 8) == 0

    def bwd(g=one, y=one, gz=one, N=2, C=4, H=8, W=8, up=2, ws=one, nbytes=big):
        return lib.cdn_codenet_bn_relu_up_backward(g, y, one, one, one, one, gz, one, one, one, N, C, H, W, up, 1, ws,
                                                   nbytes, None)

    assert bwd(g=None) == ARG and bwd(y=None) == ARG and bwd(gz=None) == ARG
    assert bwd(N=0) == ARG and bwd(up=4) == ARG and bwd(g=one + 8) == ARG
    assert bwd(N=64, C=256, H=512, W=512) == UNSUPPORTED
    assert bwd(H=96, W=100, nbytes=need - 1) == WORKSPACE and bwd(ws=one + 4) == WORKSPACE


def _fp32_net(**kw):
    from codenet_amd import pipeline
    return pipeline.build_hot_path(quantized=False, planes=kw.pop("planes", [24, 16, 8, 4]), **kw)


def test_the_gate_names_its_reason():
    from codenet_amd import pipeline
    from codenet_amd.functions import codenet_bn as BN
    net = _fp32_net().train()
    seq = net.deconv_layers
    x = torch.randn(2, 24, 4, 4)
    assert BN.native_reason(seq, None) is None
    assert "GPU" in BN.native_reason(seq, x)                                       # a CPU input
    with torch.no_grad():
        assert "grad mode" in BN.native_reason(seq, None)
    BN.NATIVE_FP32_BLOCKS = False
    try:
        assert "NATIVE_FP32_BLOCKS" in BN.native_reason(seq, None)
    finally:
        BN.NATIVE_FP32_BLOCKS = True
    for attr, value, word in (("momentum", None, "momentum=None"), ("affine", False, "affine=False"),
                              ("track_running_stats", False, "track_running_stats=False")):
        other = copy.deepcopy(seq)
        setattr(other[5], attr, value)
        assert word in BN.native_reason(other, None), attr
        assert BN.native_reason(other, None).startswith("block 1")
    for pick in (lambda s: s[1], lambda s: s[2], lambda s: s[7], lambda s: s[4].conv_channel, lambda s: s[0]):
        hooked = copy.deepcopy(seq)
        pick(hooked).register_forward_hook(lambda m, i, o: None)
        assert "hook" in BN.native_reason(hooked, None)
    mixed = nn.Sequential(*(list(copy.deepcopy(seq))[:4] + list(pipeline.build_hot_path(planes=[16, 8]).deconv_layers) + [nn.ReLU()]))
    assert "mixed sequence" in BN.native_reason(mixed, None)
    assert "four-module" in BN.native_reason(nn.Sequential(*list(copy.deepcopy(seq))[:3]), None)
    wrong = copy.deepcopy(seq)
    wrong[1] = nn.BatchNorm2d(17)
    assert "features" in BN.native_reason(wrong, None)
    # everything the gate refuses is exactly seq(x): a CPU input takes the module path
    from codenet_amd.functions.codenet_stage import forward_stage_blocks
    seq.forward = lambda t: "the module path"
    assert forward_stage_blocks(seq, x) == "the module path"


def test_is_fp32_stage_stack_accepts_the_fp32_stack_and_rejects_everything_else():
    from codenet_amd import pipeline
    G = pipeline.GraphedTrainStep
    net = pipeline.build_hot_path(quantized=False)
    assert G.is_fp32_stage_stack(net) and not G.is_stage_stack(net)
    # a bare Sequential, or a container whose forward is not forward_stage_blocks, runs the framework's BatchNorm: refused
    assert not G.is_fp32_stage_stack(net.deconv_layers)

    class Plain(nn.Module):
        def __init__(self, seq):
            super().__init__()
            self.deconv_layers = seq

        def forward(self, t):
            return self.deconv_layers(t)

    class Overridden(pipeline.DeconvLayers):
        def forward(self, t):
            return self.deconv_layers(t)

    assert not G.is_fp32_stage_stack(Plain(net.deconv_layers))
    other = Overridden(planes=[24, 16])
    assert not G.is_fp32_stage_stack(other) and G.is_fp32_stage_stack(pipeline.DeconvLayers(planes=[24, 16]))
    assert G.is_fp32_stage_stack(net.train())                                      # BatchNorm in training mode too
    with torch.no_grad():
        assert G.is_fp32_stage_stack(net)                                          # a property of the modules
    quant = pipeline.build_hot_path(quantized=True, planes=[24, 16, 8, 4])
    assert G.is_stage_stack(quant) and not G.is_fp32_stage_stack(quant)            # `is_stage_stack` keeps its meaning
    hooked = _fp32_net()
    hooked.deconv_layers[1].register_forward_hook(lambda m, i, o: None)
    assert not G.is_fp32_stage_stack(hooked)
    cumulative = _fp32_net()
    cumulative.deconv_layers[5].momentum = None
    assert not G.is_fp32_stage_stack(cumulative)
    two = nn.Sequential(_fp32_net().deconv_layers, nn.ReLU())                      # more than the one Sequential
    two.deconv_layers = two[0]
    assert not G.is_fp32_stage_stack(two)
    assert "is_fp32_stage_stack" in G.__doc__ and "fp32 stack" in G.__doc__
    with pytest.raises(NotImplementedError, match="fp32 stack"):
        G(nn.Linear(2, 2), None, None, ())
