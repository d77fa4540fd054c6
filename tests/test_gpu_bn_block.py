"""The fp32 training block BatchNorm2d -> ReLU -> Upsample(x2, nearest) on the GPU (csrc/codenet_bn_train.hip,
functions/codenet_bn.py) against its numpy restatement (tests/bn_block_ref.py), against the
framework in float64 on the CPU, through the walk of an fp32 ``deconv_layers`` and as a captured training step."""
import functools

import numpy as np
import pytest
import torch

from tests import bn_block_ref as R
from tests.test_bn_block_host import EPS, MOM, SHAPES, framework64, gy_bound, make_case, z_bound

pytestmark = pytest.mark.gpu

CASES = [(s, up) for s in SHAPES for up in (1, 2)]


def _np(t):
    return t.detach().cpu().numpy()


def _eq(got, want):
    """Bit-for-bit: torch.equal on the values (a NaN nowhere in these tests)."""
    return torch.equal(got.detach().cpu(), torch.from_numpy(np.ascontiguousarray(want)))


def _run(y, gamma, beta, grad, rm, rv, up, training=True):
    """One forward + backward of the operators on the GPU: a dict of everything they leave."""
    from codenet_amd import ops
    d = "cuda"
    y, gamma, beta, grad = y.to(d), gamma.to(d), beta.to(d), grad.to(d)
    rm, rv = rm.clone().to(d), rv.clone().to(d)
    nbt = torch.zeros((), dtype=torch.int64, device=d)
    out, mean, var, invstd = ops.bn_relu_up_forward(y, gamma, beta, rm, rv, nbt if training else None, EPS, MOM, up,
                                                    training)
    keep = {}
    gy, gz, gg, gb = ops.bn_relu_up_backward(grad, y, gamma, beta, mean, invstd, up, training, keep_gz=True, keep=keep)
    gy2, none, _, _ = ops.bn_relu_up_backward(grad, y, gamma, beta, mean, invstd, up, training)      # g_z in grad_y's buffer
    assert none is None and torch.equal(gy, gy2)
    return dict(out=out, mean=mean, var=var, invstd=invstd, rm=rm, rv=rv, nbt=nbt, grad_y=gy, g_z=gz, grad_gamma=gg,
                grad_beta=gb, mb=keep["mb"], mg=keep["mg"])


def _exact_case(shape, up, seed):
    """y integers in [-8, 8], gamma half-integers, beta quarter-integers, integer gradients: every float64 sum of the
    statistics and of g_z is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    Nb, C, H, W = shape
    y = torch.randint(-8, 9, shape, generator=g).float()
    gamma = torch.randint(-4, 5, (C,), generator=g).float() / 2
    beta = torch.randint(-8, 9, (C,), generator=g).float() / 4
    grad = torch.randint(-8, 9, (Nb, C, up * H, up * W), generator=g).float()
    rm = torch.randint(-8, 9, (C,), generator=g).float() / 8
    rv = torch.randint(1, 9, (C,), generator=g).float() / 4
    return y, gamma, beta, grad, rm, rv


@pytest.mark.parametrize("shape,up", CASES)
def test_exact_arithmetic_eager_and_on_two_graph_replays(shape, up):
    """Inputs on which every float64 sum is exact: mean, var, both running buffers, the batch counter, out, grad_beta and
    g_z are the restatement's bit for bit -- eagerly, and again after each of two replays of a HIP graph of the same calls
    (the buffers advance three times)."""
    from codenet_amd import ops
    y, gamma, beta, grad, rm, rv = _exact_case(shape, up, 50 + up)
    st = R.batch_stats(_np(y), EPS)
    bw = R.backward(_np(grad), _np(y), st["mean"], st["invstd"], _np(gamma), _np(beta), up)
    want_out = R.forward(_np(y), st["mean"], st["invstd"], _np(gamma), _np(beta), up)
    rms, rvs = [_np(rm)], [_np(rv)]
    for _ in range(3):
        a, b = R.running_update(rms[-1], rvs[-1], st, MOM)
        rms.append(a)
        rvs.append(b)

    def check(r, step):
        assert _eq(r["mean"], st["mean"]) and _eq(r["var"], st["var"]) and _eq(r["invstd"], st["invstd"])
        assert _eq(r["rm"], rms[step]) and _eq(r["rv"], rvs[step]) and int(r["nbt"]) == step
        assert _eq(r["out"], want_out)
        assert _eq(r["g_z"], bw["g_z"]) and _eq(r["grad_beta"], bw["grad_beta"])
        assert _eq(r["mb"], bw["mb"])

    got = _run(y, gamma, beta, grad, rm, rv, up)
    check(got, 1)
    # the same calls captured: the buffers of `got` advance in place on every replay
    d = "cuda"
    yd, gd, bd, grd = y.to(d), gamma.to(d), beta.to(d), grad.to(d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out, mean, var, invstd = ops.bn_relu_up_forward(yd, gd, bd, got["rm"], got["rv"], got["nbt"], EPS, MOM, up, True)
        gy, gz, gg, gb = ops.bn_relu_up_backward(grd, yd, gd, bd, mean, invstd, up, True, keep_gz=True)
    for step in (2, 3):
        for t in (out, mean, var, invstd, gy, gz, gb):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        rep = dict(got, out=out, mean=mean, var=var, invstd=invstd, g_z=gz, grad_beta=gb)
        check(rep, step)


@functools.lru_cache(maxsize=None)
def _random_case(shape, up):
    """The random inputs, the GPU's results and the float64 framework reference of one case, computed once."""
    case = make_case(shape, up, 1000 + up)
    return case, _run(*case, up), framework64(*case, up)


@pytest.mark.parametrize("shape,up", CASES)
def test_own_intermediates_on_random_inputs(shape, up):
    """Per-channel numbers against float64 within one float32 rounding plus the float64 accumulation, |got - ref| <=
    2^-24 |ref| + n 2^-52 sum |terms|; everything elementwise (out, g_z, grad_y) bit for bit the restatement evaluated on
    the GPU's own per-channel numbers, and invstd the correctly rounded 1 / sqrt(var + eps) of the GPU's own var."""
    (y, gamma, beta, grad, rm, rv), r, _ = _random_case(shape, up)
    st = R.batch_stats(_np(y), EPS)
    n = st["n"]
    mean, var, invstd = _np(r["mean"]), _np(r["var"]), _np(r["invstd"])
    assert np.all(np.abs(mean - st["mean_d"]) <= R.channel_bound(st["mean_d"], n, st["abs1"] / n))
    assert np.all(np.abs(var - st["var_d"]) <= R.channel_bound(st["var_d"], n, st["s2"] / n + st["mean_d"] ** 2))
    assert _eq(r["invstd"], R.invstd_of(var, EPS))
    assert _eq(r["out"], R.forward(_np(y), mean, invstd, _np(gamma), _np(beta), up))
    gz, xh, t1, t2 = R.backward_gz(_np(grad), _np(y), mean, invstd, _np(gamma), _np(beta), up)
    assert _eq(r["g_z"], gz)
    a1 = np.abs(gz.astype(np.float64)).sum(axis=(0, 2, 3))
    a2 = np.abs(gz.astype(np.float64) * xh.astype(np.float64)).sum(axis=(0, 2, 3))
    assert np.all(np.abs(_np(r["grad_beta"]) - t1) <= R.channel_bound(t1, n, a1))
    assert np.all(np.abs(_np(r["grad_gamma"]) - t2) <= R.channel_bound(t2, n, a2))
    assert np.all(np.abs(_np(r["mb"]) - t1 / n) <= R.channel_bound(t1 / n, n, a1 / n))
    assert np.all(np.abs(_np(r["mg"]) - t2 / n) <= R.channel_bound(t2 / n, n, a2 / n))
    assert _eq(r["grad_y"], R.backward_gy(gz, _np(y), mean, invstd, _np(gamma), _np(r["mb"]), _np(r["mg"]), True))
    # the running buffers from the GPU's own mean (and var_d within the same bound as var)
    m, omm = R.F(MOM), R.F(1.0 - MOM)
    assert _eq(r["rm"], omm * _np(rm) + m * mean) and int(r["nbt"]) == 1
    rv_ref = R.running_update(_np(rm), _np(rv), st, MOM)[1]
    # (one ulp of the result, <= 2 * 2^-24 |rv|, plus the ulp var_u may move by under a different float64 sum order)
    assert np.all(np.abs(_np(r["rv"]) - rv_ref) <= 4 * R.U32 * np.abs(rv_ref))


@pytest.mark.parametrize("shape,up", CASES)
def test_against_the_framework_in_float64(shape, up):
    """|z - z64| <= 8 * 2^-24 * S with S = |gamma| invstd (|y| + |mean|) + |beta| (on out: the ReLU and the replication
    change nothing), |grad_y - grad_y64| <= 23 * 2^-24 * |gamma| invstd (G + B1 + A B2): the bounds DESIGN.md section 4.3e
    derives from the operation counts.  Elements with |z64| <= 8 * 2^-24 * S are left out of the ReLU-dependent comparisons
    (at most 1e-4 of all; with this generator none)."""
    (y, gamma, beta, grad, rm, rv), r, ref = _random_case(shape, up)
    mean64 = y.double().mean(dim=(0, 2, 3))
    var64 = y.double().var(dim=(0, 2, 3), unbiased=False)
    invstd64 = 1.0 / torch.sqrt(var64 + EPS)
    S = z_bound(y.double(), gamma.double(), beta.double(), mean64, invstd64)
    unsure = ref["z"].abs() <= R.K_Z * R.U32 * S
    assert unsure.double().mean().item() <= 1e-4
    sure_up = ~(torch.from_numpy(R.up2(_np(unsure))) if up == 2 else unsure)
    S_up = torch.from_numpy(R.up2(_np(S))) if up == 2 else S
    ratio = ((r["out"].cpu().double() - ref["out"]).abs() / (R.U32 * S_up))[sure_up].max().item()
    print("out: %.2f of %.0f" % (ratio, R.K_Z))
    assert ratio <= R.K_Z
    B = gy_bound(y.double(), gamma.double(), mean64, invstd64, grad.double(), up)
    gratio = ((r["grad_y"].cpu().double() - ref["grad_y"]).abs() / (R.U32 * B)).max().item()
    print("grad_y: %.2f of %.0f" % (gratio, R.K_GY))
    assert unsure.sum().item() == 0      # (this generator: no ReLU decision in doubt, so every comparison below is whole)
    assert gratio <= R.K_GY
    G = grad.double().abs()
    if up == 2:
        G = G[:, :, 0::2, 0::2] + G[:, :, 0::2, 1::2] + G[:, :, 1::2, 0::2] + G[:, :, 1::2, 1::2]
    assert ((r["g_z"].cpu().double() - ref["g_z"]).abs() <= 3 * R.U32 * G)[~unsure].all()
    rm64, rv64 = _np(ref["running_mean"]), _np(ref["running_var"])
    assert np.all(np.abs(_np(r["rm"]) - rm64) <= 4 * R.U32 * (np.abs(_np(rm)) + np.abs(_np(mean64))))
    assert np.all(np.abs(_np(r["rv"]) - rv64) <= 4 * R.U32 * (np.abs(_np(rv)) + 2 * _np(var64)))


def test_eval_mode_batchnorm_under_grad():
    """bn.training == False: the same apply kernel on the running statistics, the backward without the two subtracted
    terms -- bit for bit the restatement; the buffers are untouched."""
    for shape, up in (((3, 5, 9, 11), 2), ((2, 64, 8, 8), 1), ((2, 4, 96, 100), 2)):
        y, gamma, beta, grad, rm, rv = make_case(shape, up, 77)
        r = _run(y, gamma, beta, grad, rm, rv, up, training=False)
        invstd = R.invstd_of(_np(rv), EPS)
        assert _eq(r["mean"], _np(rm)) and _eq(r["var"], _np(rv)) and _eq(r["invstd"], invstd)
        assert _eq(r["rm"], _np(rm)) and _eq(r["rv"], _np(rv)) and int(r["nbt"]) == 0
        assert _eq(r["out"], R.forward(_np(y), _np(rm), invstd, _np(gamma), _np(beta), up))
        gz, xh, t1, t2 = R.backward_gz(_np(grad), _np(y), _np(rm), invstd, _np(gamma), _np(beta), up)
        n = shape[0] * shape[2] * shape[3]
        assert _eq(r["g_z"], gz)
        assert _eq(r["grad_y"], R.backward_gy(gz, _np(y), _np(rm), invstd, _np(gamma), None, None, False))
        a2 = np.abs(gz.astype(np.float64) * xh.astype(np.float64)).sum(axis=(0, 2, 3))
        assert np.all(np.abs(_np(r["grad_gamma"]) - t2) <= R.channel_bound(t2, n, a2))
        assert np.all(np.abs(_np(r["grad_beta"]) - t1) <= R.channel_bound(t1, n, np.abs(gz.astype(np.float64)).sum(axis=(0, 2, 3))))


# ---- the walk ---------------------------------------------------------------------------------------------------------------
# Two float32 evaluations of the whole stack (three stages, three blocks, forward and backward) are held to REL of the
# largest magnitude of the compared tensor.  Where it comes from: what differs between the two runs is sharp-checked block by
# block below -- at most 2 * 8 * 2^-24 ~ 1e-6 relative to S in a block's forward, 2 * 23 * 2^-24 ~ 3e-6 in its backward (three
# blocks, both directions: ~ 1.2e-5 if nothing amplified them) -- or a re-association of four-term sums in the stage's
# stored-resolution gather backward; the stages in between are the same kernels on both sides.  What their condition
# numbers make of it has no useful worst-case bound (the Lipschitz product of one stage is 1e3 .. 1e4), so the stack is held
# to the figure this project already holds re-association-level differences of this very stack to, the quantised twin
# test_train_step.py::test_stored_resolution_stages_equal_the_upsampled_path: 2e-4 of the magnitude, an amplification of
# ~ 16 over the sum of the per-block bounds.  A dropped, swapped or sign-flipped gradient is wrong by O(1) of the magnitude.
REL = 2e-4


def _loss(out):
    return out.square().reshape(-1, 64).sum(1).sum() / out.numel()      # (a two-level reduction: one order)


def _walk(planes, x, native=True, stored=True, hook=None, mode="train"):
    """One forward + backward of the fp32 stack from seed 5: (out, {parameter: grad}, {buffer: value}, seen, net, tape).
    hook: forward hooks on the stages (the walk then takes seq(x)) record every stage's (input, output) in `seen` and, in
    `tape`, the framework's gradient of every stage output ("gy", b) and of every block output ("gin", b)."""
    from codenet_amd import pipeline
    from codenet_amd.functions import codenet_bn as BN, codenet_stage as CS
    net = pipeline.build_hot_path(quantized=False, planes=planes, seed=5).cuda()
    net = net.train() if mode == "train" else net.eval()
    seen, tape = [], {}

    def on_stage(m, i_, o):
        b = len(seen)
        seen.append((i_[0].detach(), o.detach()))
        o.register_hook(lambda g: tape.__setitem__(("gy", b), g.detach().clone()))
        if b > 0:
            i_[0].register_hook(lambda g: tape.__setitem__(("gin", b - 1), g.detach().clone()))

    if hook is not None:
        for i in range(0, len(net.deconv_layers), 4):
            net.deconv_layers[i].register_forward_hook(on_stage)
    BN.NATIVE_FP32_BLOCKS, CS.STORED_RES_STAGES = native, stored
    try:
        out = net(x)
        if hook is not None:
            out.register_hook(lambda g: tape.__setitem__(("gin", len(seen) - 1), g.detach().clone()))
        _loss(out).backward()
    finally:
        BN.NATIVE_FP32_BLOCKS, CS.STORED_RES_STAGES = True, True
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    grads["x"] = x.grad.detach().clone()
    x.grad = None
    return out.detach(), grads, {k: b.detach().clone() for k, b in net.named_buffers()}, seen, net, tape


def _close(a, b, what):
    """|a - b| <= REL max|b| (see REL)."""
    d, m = (a - b).abs().max().item(), b.abs().max().item()
    print("%s: %.3g of %.3g (%.2g of the magnitude)" % (what, d, m, d / (m + 1e-30)))
    assert d <= REL * m, what


@pytest.mark.parametrize("planes", [[24, 16, 8, 4], [64, 32, 16, 8]])
def test_the_walk_against_the_module_path(planes):
    """build_hot_path(quantized=False) in .train(), BatchNorm in training mode, input [2, C, 8, 8]: the fused walk against
    the same net with NATIVE_FP32_BLOCKS = False (the framework's BatchNorm2d, ReLU and Upsample under autograd).

    Sharp, per block, on the module path's own tensors (captured with hooks: the stage output y, the gradient arriving at
    the block's output, the framework's gradient of y and of gamma / beta):
      * forward: the native block on that y within 2 * 8 * 2^-24 * S of the module path's block output (both sides within
        8 * 2^-24 * S of exact);
      * backward, THROUGH THE AUTOGRAD FUNCTION (BnReluUpsample.apply(...).backward(incoming gradient)): grad_y within
        23 * 2^-24 * |gamma| invstd (G + B1 + A B2) of F.batch_norm -> relu -> interpolate in float64 on the CPU and within
        twice that of the module path's float32 grad_y; grad_gamma / grad_beta within one rounding of a float64 sum whose
        terms carry 9 * 2^-24 * G A / 3 * 2^-24 * G (as the host test holds the restatement);
      * block 0's running buffers (the same y in both runs, bit for bit) within 2 * 8 * 2^-24 (|running| + |batch value|) /
        (1 - momentum) of each other.
    No element of these tensors has |z64| <= 8 * 2^-24 * S (asserted), so no ReLU decision is in doubt.
    Whole stack: output, every parameter gradient, grad_x and every running buffer of the native walk within REL = 2e-4 of
    the magnitude of the module path's (see REL above for where that figure comes from).

    Bit for bit: the forward -- output and BatchNorm buffers -- with the stored-resolution hand-over on and off (the same
    values through the same expressions); a hook on an inner module takes seq(x), which is the NATIVE_FP32_BLOCKS = False
    run.  The GRADIENTS with the hand-over on and off are not bit-identical and cannot be: the stage's stored-resolution
    gather backward (cdn_codenet_dw_up2_backward) folds the four pixels of a 2x2 block onto their shared cells in another
    order than gather backward + 2x2 sum, exactly as in the quantised walk; they are held to that test's 2e-4 of the
    magnitude."""
    import copy
    from codenet_amd import ops
    from codenet_amd.functions import codenet_bn as BN
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(2, planes[0], 8, 8, generator=g).abs_() * 1.66).cuda().requires_grad_(True)
    out_n, gr_n, bf_n, _, net_n, _ = _walk(planes, x)
    assert BN.native_reason(net_n.deconv_layers, x) is None
    out_s, gr_s, bf_s, _, _, _ = _walk(planes, x, stored=False)
    assert torch.equal(out_n, out_s) and all(torch.equal(bf_n[k], bf_s[k]) for k in bf_n)
    out_m, gr_m, bf_m, _, _, _ = _walk(planes, x, native=False)
    out_h, gr_h, bf_h, seen, net_h, tape = _walk(planes, x, hook=True)      # hooked: seq(x)
    assert "hook" in BN.native_reason(net_h.deconv_layers, x)
    assert torch.equal(out_h, out_m) and all(torch.equal(gr_h[k], gr_m[k]) for k in gr_m)
    assert all(torch.equal(bf_h[k], bf_m[k]) for k in bf_m)
    # block 0's buffers, sharp; |initial| + |batch| <= (|after| + |batch|) / (1 - momentum)
    y0 = seen[0][1].double()
    mean0, var0 = y0.mean(dim=(0, 2, 3)), y0.var(dim=(0, 2, 3), unbiased=False)
    for name, batch in (("running_mean", mean0.abs()), ("running_var", 2 * var0)):
        k = "deconv_layers.1." + name
        assert ((bf_n[k] - bf_m[k]).abs().double() <= 2 * R.K_Z * R.U32 * (bf_m[k].abs().double() + batch) / 0.9).all(), k
    assert all(int(bf_n["deconv_layers.%d.num_batches_tracked" % i]) == 1 for i in (1, 5, 9))
    # every block, sharp, on the module path's own tensors
    mods_h = list(net_h.deconv_layers)
    for b in range(3):
        y, bn = seen[b][1], mods_h[4 * b + 1]
        gam, bet, gin = bn.weight.detach(), bn.bias.detach(), tape[("gin", b)]
        want = seen[b + 1][0] if b < 2 else out_h
        ref = framework64(y.cpu(), gam.cpu(), bet.cpu(), gin.cpu(), torch.zeros(len(gam)), torch.ones(len(gam)), 2)
        y64 = y.double().cpu()
        mean = y64.mean(dim=(0, 2, 3))
        invstd = 1.0 / torch.sqrt(y64.var(dim=(0, 2, 3), unbiased=False) + bn.eps)
        S = z_bound(y64, gam.double().cpu(), bet.double().cpu(), mean, invstd)
        assert (ref["z"].abs() <= R.K_Z * R.U32 * S).sum().item() == 0
        # forward
        o = ops.bn_relu_up_forward(y, gam, bet, None, None, None, bn.eps, bn.momentum, 2, True)[0]
        S2 = S.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        ratio = ((o - want).abs().double().cpu() / (R.U32 * S2)).max().item()
        print("block %d forward on the same y: %.2f of %.0f" % (b, ratio, 2 * R.K_Z))
        assert ratio <= 2 * R.K_Z, b
        # backward through the autograd function
        yl, gl, bl = (t.clone().requires_grad_(True) for t in (y, gam, bet))
        on, mean_n, var_n, invstd_n = BN.BnReluUpsample.apply(yl, gl, bl, copy.deepcopy(bn), 2)
        assert torch.equal(on, o) and not mean_n.requires_grad and not invstd_n.requires_grad
        on.backward(gin)
        B = gy_bound(y64, gam.double().cpu(), mean, invstd, gin.double().cpu(), 2)
        r64 = ((yl.grad.double().cpu() - ref["grad_y"]).abs() / (R.U32 * B)).max().item()
        r32 = ((yl.grad - tape[("gy", b)]).abs().double().cpu() / (R.U32 * B)).max().item()
        print("block %d grad_y: %.2f of %.0f against float64, %.2f of %.0f against the module path"
              % (b, r64, R.K_GY, r32, 2 * R.K_GY))
        assert r64 <= R.K_GY and r32 <= 2 * R.K_GY, b
        G = gin.double().cpu().abs()
        G = G[:, :, 0::2, 0::2] + G[:, :, 0::2, 1::2] + G[:, :, 1::2, 0::2] + G[:, :, 1::2, 1::2]
        A = invstd.reshape(1, -1, 1, 1) * (y64.abs() + mean.abs().reshape(1, -1, 1, 1))
        gb64, gg64 = ref["grad_beta"], ref["grad_gamma"]
        assert ((bl.grad.double().cpu() - gb64).abs() <= R.U32 * (gb64.abs() + 3 * G.sum(dim=(0, 2, 3)))).all(), b
        assert ((gl.grad.double().cpu() - gg64).abs() <= R.U32 * (gg64.abs() + 9 * (G * A).sum(dim=(0, 2, 3)))).all(), b
    # the whole stack against the module path
    _close(out_n, out_m, "out")
    assert set(gr_n) == set(gr_m) and len(gr_m) == 19
    for k in gr_m:
        _close(gr_n[k], gr_m[k], "grad " + k)
    for k in bf_m:
        if bf_m[k].is_floating_point():
            _close(bf_n[k], bf_m[k], k)
    # hand-over on / off: the gradients, re-associated
    for k in gr_s:
        _close(gr_n[k], gr_s[k], "stored on / off, grad " + k)


def test_the_walk_with_batchnorm_in_eval_mode():
    """The same stack in .eval() under grad (running statistics; what tools/train_step_bench.py --fp32 runs): the fused walk
    -- BnReluUpsample without a statistics pass, workspace or buffer update -- against NATIVE_FP32_BLOCKS = False within
    REL of the magnitude (output, every parameter gradient, grad_x); the buffers are untouched, bit for bit."""
    planes = [24, 16, 8, 4]
    g = torch.Generator().manual_seed(10)
    x = (torch.randn(2, planes[0], 8, 8, generator=g).abs_() * 1.66).cuda().requires_grad_(True)
    out_n, gr_n, bf_n, _, net_n, _ = _walk(planes, x, mode="eval")
    out_m, gr_m, bf_m, _, _, _ = _walk(planes, x, native=False, mode="eval")
    from codenet_amd import pipeline
    fresh = dict(pipeline.build_hot_path(quantized=False, planes=planes, seed=5).named_buffers())
    assert all(torch.equal(bf_n[k].cpu(), fresh[k]) for k in fresh) and len(fresh) == 9
    _close(out_n, out_m, "out")
    for k in gr_m:
        _close(gr_n[k], gr_m[k], "grad " + k)


def test_one_value_per_channel_in_training_mode_raises():
    from codenet_amd import pipeline
    net = pipeline.build_hot_path(quantized=False, planes=[24, 16], seed=5).cuda().train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):      # (before any launch)
        net(torch.rand(1, 24, 1, 1, device="cuda").requires_grad_(True))


# ---- the captured step ------------------------------------------------------------------------------------------------------
def _build_step():
    from codenet_amd import pipeline
    net = pipeline.build_hot_path(quantized=False, planes=[24, 16, 8, 4], seed=6).cuda().train()
    return net, torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device="cuda"), capturable=True)


def _state(net, opt):
    ts = [p.detach() for p in net.parameters()] + list(net.buffers())
    for st in opt.state.values():
        ts += [v for v in st.values() if torch.is_tensor(v)]
    return ts


def test_graphed_train_step_of_the_fp32_stack_replays_the_eager_step_bit_for_bit():
    """GraphedTrainStep on the fp32 stack, BatchNorm in training mode, Adam, WITHOUT unvalidated=True (on the parent commit:
    NotImplementedError).  Replays are bit-identical to eager steps on the same batches in loss, parameters, BatchNorm
    buffers and Adam state; two runs from one seed end bit-identical."""
    from codenet_amd import pipeline

    def loss_fn(net, x):
        return _loss(net(x))

    g = torch.Generator().manual_seed(3)
    batches = [(torch.randn(2, 24, 8, 8, generator=g).abs_() * 1.66).cuda() for _ in range(4)]

    def run_graphed():
        net, opt = _build_step()
        assert pipeline.GraphedTrainStep.is_fp32_stage_stack(net)
        step = pipeline.GraphedTrainStep(net, opt, loss_fn, (batches[0],), warmup=2)
        losses = [step(x).detach().clone() for x in batches[1:]]
        torch.cuda.synchronize()
        return net, opt, losses

    net_g, opt_g, losses_g = run_graphed()
    net_e, opt_e = _build_step()
    losses_e = []
    for i, x in enumerate([batches[0]] * 2 + batches[1:]):
        opt_e.zero_grad(set_to_none=True)
        le = loss_fn(net_e, x)
        le.backward()
        opt_e.step()
        if i >= 2:
            losses_e.append(le.detach().clone())
    assert all(torch.equal(a, b) for a, b in zip(losses_e, losses_g)) and len(losses_g) == 3
    for a, b in zip(_state(net_e, opt_e), _state(net_g, opt_g)):
        assert torch.equal(a, b)
    assert int(net_g.deconv_layers[1].num_batches_tracked) == 5
    net_2, opt_2, losses_2 = run_graphed()
    assert all(torch.equal(a, b) for a, b in zip(losses_g, losses_2))
    for a, b in zip(_state(net_g, opt_g), _state(net_2, opt_2)):
        assert torch.equal(a, b)
