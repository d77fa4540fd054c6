"""Host side of the native fp32 detection heads (functions/codenet_heads_fp32.py, csrc/codenet_heads_fp32_train.hip): the
numpy restatement (tests/heads_fp32_ref.py) against the framework in float64, the gate's reasons, the GraphedTrainStep
scope, the library's new entry points and the launch arithmetic of the GPU test's shapes.  No GPU.  The generators and the
stage-wise float64 bounds are shared with tests/test_gpu_heads_fp32.py."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import bn_block_ref as R
from tests import heads_fp32_ref as HR
from tests.test_bn_block_host import gy_bound, z_bound

NEW_SYMBOLS = ("cdn_codenet_head_fp32_workspace_bytes", "cdn_codenet_head_fp32_bn_stats", "cdn_codenet_head_fp32_dw_forward",
               "cdn_codenet_head_fp32_tail_forward", "cdn_codenet_head_fp32_tail_backward",
               "cdn_codenet_head_fp32_bn_backward1", "cdn_codenet_head_fp32_dw_backward",
               "cdn_codenet_head_fp32_bn_backward2")
# x = [N, 64, H, W], the hm width K, and what the shape exercises (strips, chunks per plane, slabs per channel)
SHAPES = [((2, 64, 1, 1), 5), ((3, 64, 5, 7), 5), ((2, 64, 9, 10), 20), ((2, 64, 16, 16), 5), ((2, 64, 33, 50), 5),
          ((1, 64, 72, 116), 20)]
PLANS = {(2, 64, 1, 1): (1, 1, 1, 1), (3, 64, 5, 7): (2, 1, 1, 1), (2, 64, 9, 10): (3, 2, 1, 1), (2, 64, 16, 16): (4, 2, 1, 1),
         (2, 64, 33, 50): (13, 5, 1, 1), (1, 64, 72, 116): (29, 9, 2, 3)}      # (wq, strips, chunks, slabs)
EPS, MOM, C = 1e-5, 0.1, 64
U = R.U32
# the constants of DESIGN.md section 4.3f (operation counts): z within K_Z u S of exact (section 4.3e); a depthwise output
# passes one product and nine additions; a 1x1 output over 64 channels 64 products, 64 additions and the bias;
# grad_y within K_GY u B (section 4.3e); xh within K_XH u A
K_Z, K_GY, K_DW, K_XH = R.K_Z, R.K_GY, 10.0, 6.0
SECOND_ORDER = 1.01


def make_heads(widths):
    """{name: the seven-module Sequential of shufflenetv2_dcn.py:246-258}; the generators below set every parameter."""
    heads = {}
    for name, co in widths.items():
        heads[name] = nn.Sequential(
            nn.Conv2d(C, C, 1, 1, 0, bias=False), nn.BatchNorm2d(C, momentum=MOM), nn.ReLU(inplace=True),
            nn.Conv2d(C, C, 3, 1, 1, groups=C, bias=False), nn.BatchNorm2d(C, momentum=MOM), nn.ReLU(inplace=True),
            nn.Conv2d(C, co, kernel_size=1, stride=1, padding=0, bias=True))
    return heads


def head_params(mod):
    """The float32 numpy operands of tests/heads_fp32_ref.head from a head module (before a forward)."""
    n = lambda t: t.detach().cpu().numpy().copy()      # noqa: E731
    return dict(w1=n(mod[0].weight).reshape(C, -1), g1=n(mod[1].weight), b1=n(mod[1].bias), w2=n(mod[3].weight).reshape(C, 9),
                g2=n(mod[4].weight), b2=n(mod[4].bias), w3=n(mod[6].weight).reshape(mod[6].out_channels, C),
                b3=n(mod[6].bias), rm1=n(mod[1].running_mean), rv1=n(mod[1].running_var), rm2=n(mod[4].running_mean),
                rv2=n(mod[4].running_var), eps=mod[1].eps, momentum=mod[1].momentum, train1=mod[1].training,
                train2=mod[4].training)


def random_case(shape, widths, seed):
    """The generator of test_gpu_bn_block.py carried to the heads: y1 ~ 1.5 randn + 0.3 per channel comes from x ~ randn
    through a weight of row norm 1.5 (the 0.3 through gamma / beta), gamma in [0.5, 1.5), beta = 0.1 randn, random gradients."""
    g = torch.Generator().manual_seed(seed)
    heads = make_heads(widths)
    with torch.no_grad():
        for mod in heads.values():
            w = torch.randn(C, C, generator=g)
            mod[0].weight.copy_((1.5 * w / w.norm(dim=1, keepdim=True)).view(C, C, 1, 1))
            mod[3].weight.copy_(torch.randn(C, 1, 3, 3, generator=g) / 3)
            co = mod[6].out_channels
            mod[6].weight.copy_(torch.randn(co, C, 1, 1, generator=g) / 8)
            mod[6].bias.copy_(torch.randn(co, generator=g) * 0.1)
            for bn in (mod[1], mod[4]):
                bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
                bn.bias.copy_(torch.randn(C, generator=g) * 0.1)
                bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
                bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    x = torch.randn(shape, generator=g) + 0.2
    gys = {h: torch.randn(shape[0], co, shape[2], shape[3], generator=g) for h, co in widths.items()}
    return heads, x, gys


def exact_case(shape, widths, seed, beta1_positive=False):
    """Integers and quarter-integers on a coarse grid: x integers in [-4, 4], three non-zero halves / ones per row of W1 (y1
    a multiple of 1/2 below 16: every order of its sums is exact, in float32 and in the float64 statistics), W2 quarter-
    integers, BatchNorm weights half-, biases quarter-integers, integer gradients.  A narrow head's W3 holds quarter-
    integers (its sums have the kernels' own order, which the restatement follows); a wide head's W3 has ONE power of two
    per row, in a column of its own, so y3 and grad_a2 on the MFMA kernels are one product each: exact in any order."""
    g = torch.Generator().manual_seed(seed)
    heads = make_heads(widths)
    ri = lambda lo, hi, size: torch.randint(lo, hi + 1, size, generator=g).float()      # noqa: E731
    with torch.no_grad():
        for mod in heads.values():
            w1 = torch.zeros(C, C)
            for r in range(C):
                idx = torch.randperm(C, generator=g)[:3]
                w1[r, idx] = (ri(1, 2, (3,)) / 2) * (ri(0, 1, (3,)) * 2 - 1)
            mod[0].weight.copy_(w1.view(C, C, 1, 1))
            mod[3].weight.copy_(ri(-8, 8, (C, 1, 3, 3)) / 4)
            co = mod[6].out_channels
            if co <= 4:
                mod[6].weight.copy_(ri(-8, 8, (co, C, 1, 1)) / 4)
            else:
                w3 = torch.zeros(co, C)
                cols = torch.randperm(C, generator=g)[:co]
                w3[torch.arange(co), cols] = (2.0 ** ri(-1, 1, (co,))) * (ri(0, 1, (co,)) * 2 - 1)
                mod[6].weight.copy_(w3.view(co, C, 1, 1))
            mod[6].bias.copy_(ri(-8, 8, (co,)) / 4)
            for bn in (mod[1], mod[4]):
                bn.weight.copy_(ri(1, 4, (C,)) / 2 * (ri(0, 1, (C,)) * 2 - 1))
                bn.bias.copy_(ri(-8, 8, (C,)) / 4)
                bn.running_mean.copy_(ri(-8, 8, (C,)) / 8)
                bn.running_var.copy_(ri(1, 8, (C,)) / 4)
            if beta1_positive:
                mod[1].bias.copy_(ri(1, 8, (C,)) / 4)
    x = ri(-4, 4, shape)
    gys = {h: ri(-4, 4, (shape[0], co, shape[2], shape[3])) for h, co in widths.items()}
    return heads, x, gys


def restate(heads, x, gys, y1=None, mutate=()):
    """tests/heads_fp32_ref.head for every head: {name: result}, from the modules' state BEFORE a forward."""
    return {h: HR.head(x.numpy(), head_params(m), gys[h].numpy(), None if y1 is None else y1[h], mutate)
            for h, m in heads.items()}


def module_path64(heads, x, gys):
    """The heads as float64 framework modules on the CPU under autograd: ({name: y3}, {name: {parameter: grad}}, grad_x,
    {name: module after the step})."""
    mods = {h: copy.deepcopy(m).double() for h, m in heads.items()}
    x64 = x.double().requires_grad_(True)
    outs = {h: m(x64) for h, m in mods.items()}
    torch.autograd.backward([outs[h] for h in mods], [gys[h].double() for h in mods])
    grads = {h: {k: p.grad for k, p in m.named_parameters()} for h, m in mods.items()}
    return {h: o.detach() for h, o in outs.items()}, grads, x64.grad, mods


# ---- the stage-wise float64 bounds of DESIGN.md section 4.3f -----------------------------------------------------------------

def _c(v):
    return v.reshape(1, -1, 1, 1)


def _bn_fw64(y, p, k, grad_z=None):
    """BatchNorm k of the FRAMEWORK in float64 (F.batch_norm under autograd) on the float32 tensor y: z, and with grad_z
    (the float32 gradient arriving at z) the framework's grad_y, grad_gamma, grad_beta.  Beside them the per-channel numbers
    and the magnitudes S, A, B of the bounds (z_bound / gy_bound of tests/test_bn_block_host.py), which are no references."""
    t = lambda a: torch.from_numpy(np.asarray(a)).double()      # noqa: E731
    y = t(y).requires_grad_(True)
    gamma, beta = t(p["g%d" % k]).requires_grad_(True), t(p["b%d" % k]).requires_grad_(True)
    training = bool(p["train%d" % k])
    rm, rv = t(p["rm%d" % k]).clone(), t(p["rv%d" % k]).clone()
    if training:
        mean, var = y.detach().mean(dim=(0, 2, 3)), y.detach().var(dim=(0, 2, 3), unbiased=False)
    else:
        mean, var = rm.clone(), rv.clone()
    z = F.batch_norm(y, rm, rv, gamma, beta, training, p["momentum"], p["eps"])
    invstd = 1.0 / torch.sqrt(var + p["eps"])
    yd, gd, bd = y.detach(), gamma.detach(), beta.detach()
    out = dict(z=z.detach(), S=z_bound(yd, gd, bd, mean, invstd), A=_c(invstd) * (yd.abs() + _c(mean.abs())))
    if grad_z is not None:
        gz = t(grad_z)
        z.backward(gz)
        k_ = _c((gd * invstd).abs())
        out.update(grad_y=y.grad, grad_gamma=gamma.grad, grad_beta=beta.grad, gz=gz,
                   B=gy_bound(yd, gd, mean, invstd, gz, 1) if training else gz.abs() * k_)
    return out


def stage_ratios(x, p, r, gy3, n_w3):
    """Every stage of one head AS THE FRAMEWORK COMPUTES IT IN FLOAT64 -- F.conv2d, F.batch_norm, F.relu under autograd on
    the CPU, the operators of the module path -- ON THE FLOAT32 INPUTS OF THAT STAGE (x, r["y1"], r["y2"], r["g_z2"],
    r["g_z1"]: the GPU's or the restatement's own), against what the stage left, as fractions of the bounds DESIGN.md
    section 4.3f derives by operation count.  No reference here is a formula of the test's own: forward values are module
    outputs, gradients are autograd's.  n_w3: roundings a term of grad_W3 passes in its sum (1: a float64 sum rounded once;
    n + 1: a float32 accumulation over n pixels).  Returns ({what: max |err| / bound}, fraction of elements left out of the
    ReLU-dependent comparisons)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).double()      # noqa: E731
    x, gy3 = t(x), t(gy3)
    w1, w2, w3, b3 = t(p["w1"]).view(C, C, 1, 1), t(p["w2"]).view(C, 1, 3, 3), t(p["w3"]), t(p["b3"])
    Co = w3.shape[0]
    w3 = w3.view(Co, C, 1, 1)
    out = {}

    def ratio(what, got, ref, bound, keep=None):
        err, bound = (t(got).reshape(ref.shape) - ref).abs(), SECOND_ORDER * bound + 1e-300
        q = err / bound
        out[what] = float((q if keep is None else q[keep]).max())

    conv = lambda a, w: F.conv2d(a, w, padding=1, groups=C)      # noqa: E731
    # y1: 64 products and 64 additions in any order
    ratio("y1", r["y1"], F.conv2d(x, w1), (C + 1) * U * F.conv2d(x.abs(), w1.abs()))
    # BatchNorm 1 / 2 of the framework on the stage's own y, with the stage's own g_z arriving: grad_y, grad_gamma, grad_beta
    b1, b2 = _bn_fw64(r["y1"], p, 1, r["g_z1"]), _bn_fw64(r["y2"], p, 2, r["g_z2"])
    unsure1, unsure2 = b1["z"].abs() <= K_Z * U * b1["S"], b2["z"].abs() <= K_Z * U * b2["S"]
    left_out = max(unsure1.double().mean().item(), unsure2.double().mean().item())
    # the depthwise stage: y2 = conv(relu(z1)); autograd gives its gradient at z1 and at W2 for the framework's grad_y2
    z1, w2l = b1["z"].clone().requires_grad_(True), w2.clone().requires_grad_(True)
    a1 = F.relu(z1)
    y2 = conv(a1, w2l)
    ratio("y2", r["y2"], y2.detach(), U * (K_Z * conv(b1["S"], w2.abs()) + K_DW * conv(a1.detach(), w2.abs())))
    gy2, B2 = b2["grad_y"], b2["B"]
    y2.backward(gy2)
    wf = w2.flip(2, 3).abs()
    ratio("g_z1", r["g_z1"], z1.grad, U * (K_GY * conv(B2, wf) + K_DW * conv(gy2.abs(), wf)), ~unsure1)
    ap, Sp = F.pad(a1.detach(), (1, 1, 1, 1)), F.pad(b1["S"], (1, 1, 1, 1))
    H, W = a1.shape[2:]
    s = lambda v: v.sum(dim=(0, 2, 3))      # noqa: E731
    gw2_b = torch.stack([s(K_GY * B2 * ap[:, :, dy:dy + H, dx:dx + W] + K_Z * gy2.abs() * Sp[:, :, dy:dy + H, dx:dx + W])
                         for dy in range(3) for dx in range(3)], 1)
    gw2 = w2l.grad.view(C, 9)
    ratio("grad_w2", r["grad_w2"], gw2, U * (gw2.abs() + gw2_b))
    # the last conv: y3 = conv1x1(relu(z2)) + b3; autograd gives its gradient at z2 (g_z2), at W3 and at b3
    z2, w3l, b3l = b2["z"].clone().requires_grad_(True), w3.clone().requires_grad_(True), b3.clone().requires_grad_(True)
    a2 = F.relu(z2)
    y3 = F.conv2d(a2, w3l, b3l)
    a2d = a2.detach()
    ratio("y3", r["y3"], y3.detach(), U * (K_Z * F.conv2d(b2["S"], w3.abs())
                                            + (C + 2) * (F.conv2d(a2d, w3.abs()) + _c(b3.abs()))))
    y3.backward(gy3)
    ratio("g_z2", r["g_z2"], z2.grad, (Co + 1) * U * torch.einsum("oc,nohw->nchw", w3.abs().view(Co, C), gy3.abs()), ~unsure2)
    gw3 = w3l.grad.view(Co, C)
    ratio("grad_w3", r["grad_w3"], gw3, U * (n_w3 * torch.einsum("nohw,nchw->oc", gy3.abs(), a2d)
                                             + K_Z * torch.einsum("nohw,nchw->oc", gy3.abs(), b2["S"])))
    ratio("grad_b3", r["grad_b3"], b3l.grad, (n_w3 if n_w3 > 1 else 1) * U * gy3.abs().sum(dim=(0, 2, 3)))
    # the second pass of BatchNorm 1 and the per-channel gradients of both: ONE rounding of a float64 sum whose terms carry
    # the errors of their factors
    ratio("grad_y1", r["grad_y1"], b1["grad_y"], K_GY * U * b1["B"])
    n = x.shape[0] * x.shape[2] * x.shape[3]
    for k, b in ((1, b1), (2, b2)):
        ratio("grad_beta%d" % k, r["grad_b%d" % k], b["grad_beta"], U * b["grad_beta"].abs() + n * 2.0 ** -52 * s(b["gz"].abs()))
        ratio("grad_gamma%d" % k, r["grad_g%d" % k], b["grad_gamma"],
              U * (b["grad_gamma"].abs() + K_XH * s(b["gz"].abs() * b["A"])))
    return out, left_out


def flat_result(res):
    """The result dict of tests/heads_fp32_ref.head in the flat names stage_ratios reads."""
    tb, db = res["tail"], res["dw"]
    gw3 = tb["grad_w3"] if "grad_w3" in tb else tb["grad_w3_64"].astype(np.float32)
    return dict(y1=res["y1"], y2=res["y2"], y3=res["y3"], g_z2=tb["g_z"], g_z1=db["g_z"], grad_y1=res["grad_y1"],
                grad_g1=db["grad_gamma"], grad_b1=db["grad_beta"], grad_g2=tb["grad_gamma"], grad_b2=tb["grad_beta"],
                grad_w2=db["grad_w2"], grad_w3=gw3, grad_b3=tb["grad_b3"])


WIDTHS = {"hm": 5, "wh": 2, "reg": 2}


@pytest.mark.parametrize("shape,K", SHAPES[1:5])
def test_the_restatement_agrees_with_the_framework_in_float64(shape, K):
    """Stage by stage against the framework's own operators in float64 under autograd (stage_ratios: F.conv2d, F.batch_norm,
    F.relu on the float32 inputs the restatement gave each stage), within the bounds of DESIGN.md section 4.3f (no ReLU
    decision in doubt with this generator); and the whole chain against nn.Sequential.double() under autograd: every output,
    running buffer and parameter gradient the restatement forms within 2e-4 of the tensor's magnitude."""
    widths = dict(WIDTHS, hm=K)
    heads, x, gys = random_case(shape, widths, 100 + K)
    res = restate(heads, x, gys)
    seen = {}
    for h, m in heads.items():
        ratios, left_out = stage_ratios(x.numpy(), head_params(m), flat_result(res[h]), gys[h].numpy(), 1)
        assert left_out == 0.0, (h, left_out)
        for k, v in ratios.items():
            seen[k] = max(seen.get(k, 0.0), v)
            assert v <= 1.0, (h, k, v)
    print("fractions of the derived bounds:", {k: round(v, 3) for k, v in seen.items()})
    o64, g64, gx64, mods64 = module_path64(heads, x, gys)
    for h in heads:
        f = flat_result(res[h])
        pairs = [("y3", res[h]["y3"], o64[h])]
        pairs += [(k, f[name], g64[h][k]) for k, name in (("1.weight", "grad_g1"), ("1.bias", "grad_b1"), ("3.weight", "grad_w2"),
                                                          ("4.weight", "grad_g2"), ("4.bias", "grad_b2"), ("6.weight", "grad_w3"),
                                                          ("6.bias", "grad_b3"))]
        pairs += [("rm%d" % k, res[h]["rm%d" % k], mods64[h][3 * k - 2].running_mean) for k in (1, 2)]
        pairs += [("rv%d" % k, res[h]["rv%d" % k], mods64[h][3 * k - 2].running_var) for k in (1, 2)]
        for what, got, want in pairs:
            want = want.detach().numpy().reshape(-1)
            assert np.abs(np.asarray(got, np.float64).reshape(-1) - want).max() <= 2e-4 * np.abs(want).max(), (h, what)


def test_eval_mode_restatement_agrees_with_the_framework_in_float64():
    heads, x, gys = random_case((3, 64, 5, 7), WIDTHS, 7)
    for m in heads.values():
        m[1].eval()
    res = restate(heads, x, gys)
    o64, g64, _, mods64 = module_path64(heads, x, gys)
    for h, m in heads.items():
        ratios, left_out = stage_ratios(x.numpy(), head_params(m), flat_result(res[h]), gys[h].numpy(), 1)
        assert left_out == 0.0 and all(v <= 1.0 for v in ratios.values()), (h, ratios)
        assert np.array_equal(res[h]["rm1"], m[1].running_mean.numpy())       # eval mode: no buffer moves
        assert torch.equal(mods64[h][1].running_mean, m[1].running_mean.double())
        assert np.abs(res[h]["y3"] - o64[h].numpy()).max() <= 2e-4 * o64[h].abs().max().item()


def test_the_sum_orders_of_the_restatement():
    """slab_sums / plane_sums add every term exactly once (integers: any order is exact) and in the stated order: a
    sequence whose float64 sum depends on the order separates them from numpy's pairwise sum."""
    g = np.random.default_rng(0)
    ints = g.integers(-8, 9, (2, 3, 33, 50)).astype(np.float64)
    assert np.array_equal(HR.slab_sums(ints), ints.sum(axis=(0, 2, 3)))
    assert np.array_equal(HR.plane_sums(ints), ints.sum(axis=(0, 2, 3)))
    big = np.zeros((1, 1, 72, 116))
    big[0, 0, 0, 0], big[0, 0, 0, 1], big[0, 0, 71, 115] = 1.0, 2.0 ** -60, -1.0
    # thread 0 of slab 0 adds 1 + 2^-60 first (lost), the -1 arrives in slab 2: 0; the plane protocol alike (chunk 0 / 1)
    assert HR.slab_sums(big)[0] == 0.0 and HR.plane_sums(big)[0] == 0.0
    assert HR.plan(72, 116) == (29, 9, 256, 2) and HR.plan(1, 1) == (1, 1, 64, 1)


@pytest.mark.parametrize("name,where", [("pad", "y2"), ("taps", "g_z1"), ("mb2", "g_z1"), ("gb3", "grad_b3")])
def test_the_exact_cases_tell_the_mutations_apart(name, where):
    """The deliberately wrong variants of the restatement -- a padded tap that is relu(bn_z(0)), the tap order reversed in the
    gather, mb2 dropped on load, grad_b3 dropped -- differ from the contract on the inputs of the exact-arithmetic GPU test
    (beta1 > 0 on a 5 x 7 plane), in the tensor that test compares bit for bit."""
    heads, x, gys = exact_case((3, 64, 5, 7), WIDTHS, 11, beta1_positive=True)
    good, bad = restate(heads, x, gys), restate(heads, x, gys, mutate=(name,))
    pick = {"y2": lambda r: r["y2"], "g_z1": lambda r: r["dw"]["g_z"], "grad_b3": lambda r: r["tail"]["grad_b3"]}[where]
    assert not np.array_equal(pick(good["wh"]), pick(bad["wh"]))


def test_forward_heads_on_the_cpu_is_the_module_path():
    from codenet_amd.functions import codenet_heads as CH
    heads, x, _ = random_case((2, 64, 5, 7), WIDTHS, 3)
    want = {h: copy.deepcopy(m)(x) for h, m in heads.items()}
    keep = {}
    got = CH.forward_heads(heads, x, keep)
    assert keep == {} and all(torch.equal(got[h], want[h]) for h in heads)
    assert "QuantDepthwiseNode" in CH.native_reason(heads, None)      # the quantised gate keeps its answer for fp32 heads


def test_the_gate_names_its_reason():
    from codenet_amd.functions import codenet_heads_fp32 as HF
    heads, x, _ = random_case((2, 64, 5, 7), WIDTHS, 3)
    assert HF.native_reason(heads, None) is None
    assert "GPU" in HF.native_reason(heads, x)                                    # a CPU input
    with torch.no_grad():
        assert "grad mode" in HF.native_reason(heads, None)
    HF.NATIVE_FP32_HEADS = False
    try:
        assert "NATIVE_FP32_HEADS" in HF.native_reason(heads, None)
    finally:
        HF.NATIVE_FP32_HEADS = True
    assert HF.native_reason({}, None) == "no heads"
    assert "seven-module" in HF.native_reason({"hm": nn.Conv2d(64, 5, 1)}, None)  # head_conv = 0
    for attr, value, word in (("momentum", None, "momentum=None"), ("affine", False, "affine=False"),
                              ("track_running_stats", False, "track_running_stats=False")):
        for i in (1, 4):
            other = copy.deepcopy(heads)
            setattr(other["wh"][i], attr, value)
            assert word in HF.native_reason(other, None) and "head 'wh'" in HF.native_reason(other, None), (attr, i)

    def swapped(i, mod):
        other = copy.deepcopy(heads)
        other["reg"][i] = mod
        return HF.native_reason(other, None)

    assert "geometry" in swapped(3, nn.Conv2d(C, C, 3, 1, 0, groups=C, bias=False))       # no padding
    assert "geometry" in swapped(3, nn.Conv2d(C, C, 3, 2, 1, groups=C, bias=False))       # stride 2
    assert "geometry" in swapped(3, nn.Conv2d(C, C, 3, 1, 1, bias=False))                 # dense 3x3
    assert "geometry" in swapped(0, nn.Conv2d(C, C, 3, 1, 1, bias=False))
    assert "has a bias" in swapped(0, nn.Conv2d(C, C, 1, bias=True))
    assert "has a bias" in swapped(3, nn.Conv2d(C, C, 3, 1, 1, groups=C, bias=True))
    assert "no bias" in swapped(6, nn.Conv2d(C, 2, 1, bias=False))
    assert "not a BatchNorm2d" in swapped(1, nn.GroupNorm(1, C))
    assert "features" in swapped(4, nn.BatchNorm2d(32))
    assert "not Conv2d" in swapped(2, nn.Sigmoid())
    narrow = copy.deepcopy(heads)
    narrow["reg"] = nn.Sequential(nn.Conv2d(C, 32, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(),
                                  nn.Conv2d(32, 32, 3, 1, 1, groups=32, bias=False), nn.BatchNorm2d(32), nn.ReLU(),
                                  nn.Conv2d(32, 2, 1))
    assert "hidden width" in HF.native_reason(narrow, None)
    for i in range(7):
        hooked = copy.deepcopy(heads)
        hooked["hm"][i].register_forward_hook(lambda m, i_, o: None)
        assert "hook" in HF.native_reason(hooked, None), i
    hooked = copy.deepcopy(heads)
    hooked["hm"].register_forward_pre_hook(lambda m, i_: None)
    assert "hook" in HF.native_reason(hooked, None)


def test_is_fp32_tail_and_the_other_predicates():
    from codenet_amd import harness, pipeline
    G = pipeline.GraphedTrainStep
    hd = {"hm": 20, "wh": 2, "reg": 2}
    model = harness.create_model(heads=hd)
    tail = pipeline.DetectionTail(model)
    others = (G.is_native_tail, G.is_stage_stack, G.is_fp32_stage_stack, G.is_native_trunk, G.is_native_net)
    assert G.is_fp32_tail(tail) and G.is_fp32_tail(tail.train()) and not any(f(tail) for f in others)
    with torch.no_grad():
        assert G.is_fp32_tail(tail)                                                # a property of the modules
    assert not G.is_fp32_tail(model)                                               # the bare model
    assert not G.is_fp32_tail(pipeline.DetectionTrunk(model)) and not G.is_fp32_tail(tail.deconv_layers)
    qtail = pipeline.DetectionTail(harness.create_model(heads=hd, quantize=True))
    assert not G.is_fp32_tail(qtail) and G.is_native_tail(qtail) and not G.is_stage_stack(qtail)
    stack, qstack = pipeline.build_hot_path(quantized=False), pipeline.build_hot_path(quantized=True)
    assert G.is_fp32_stage_stack(stack) and not G.is_fp32_tail(stack)
    assert G.is_stage_stack(qstack) and not G.is_fp32_tail(qstack) and not G.is_fp32_stage_stack(qstack)
    hooked = pipeline.DetectionTail(harness.create_model(heads=hd))
    hooked.wh[3].register_forward_hook(lambda m, i, o: None)
    assert not G.is_fp32_tail(hooked)
    cumulative = pipeline.DetectionTail(harness.create_model(heads=hd))
    cumulative.hm[4].momentum = None
    assert not G.is_fp32_tail(cumulative)
    stage_bn = pipeline.DetectionTail(harness.create_model(heads=hd))
    stage_bn.deconv_layers[1].momentum = None
    assert not G.is_fp32_tail(stage_bn)
    assert not G.is_fp32_tail(pipeline.DetectionTail(harness.create_model(heads=hd, head_conv=0)))
    assert "is_fp32_tail" in G.__doc__ and "fp32 tail" in G.__doc__
    with pytest.raises(NotImplementedError, match="fp32 stack") as e:              # the message keeps its words and gains the case
        G(cumulative, None, None, ())
    assert "fp32 tail" in str(e.value) and "momentum=None" in str(e.value)


def test_the_library_exports_the_new_entry_points():
    from codenet_amd import _native
    lib = _native.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "codenet_dcn.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _native._SIGNATURES, s
        fn = getattr(lib, s)
        assert fn.argtypes == _native._SIGNATURES[s][1] and fn.restype is _native._SIGNATURES[s][0], s
        # the declaration carries as many parameters as the ctypes signature
        decl = header[header.rindex(s + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == len(_native._SIGNATURES[s][1]), s
    assert "shufflenetv2_dcn.py:246-258" in header


def test_the_launch_arithmetic_of_the_test_shapes():
    """Strips, chunks and slabs of every shape of the GPU test, re-derived: what the table of the GPU test says each shape
    exercises, and the workspace size the library answers."""
    from codenet_amd import _native
    lib = _native.lib()
    for (Nb, Cc, H, W), _ in SHAPES:
        wq, strips, threads, chunks = HR.plan(H, W)
        slabs = -(-Nb * H * W // 4096)
        assert (wq, strips, chunks, slabs) == PLANS[(Nb, Cc, H, W)]
        need = (8 * max(Cc * slabs * 10, Nb * Cc * chunks * 11) + 255) // 256 * 256
        assert lib.cdn_codenet_head_fp32_workspace_bytes(Nb, Cc, H, W) == need
    assert [s for s, _ in SHAPES if s[3] % 4 == 0] == [(2, 64, 16, 16), (1, 64, 72, 116)]      # the 16-byte route
    assert lib.cdn_codenet_head_fp32_workspace_bytes(0, 64, 8, 8) == 0


def test_argument_errors_come_back_before_any_launch():
    from codenet_amd import _native
    lib = _native.lib()
    one, big = 4096, 1 << 26
    ARG, UNSUPPORTED, WORKSPACE = -1, -5, -6
    huge = dict(N=64, C=256, H=512, W=512)

    def stats(y=one, mean=one, rm=one, rv=one, N=2, C=64, H=8, W=8, training=1, ws=one, nbytes=big, mom=0.1, eps=1e-5):
        return lib.cdn_codenet_head_fp32_bn_stats(y, rm, rv, one, mean, one, one, N, C, H, W, training, eps, mom, ws, nbytes,
                                                  None)

    assert stats(y=None) == ARG and stats(mean=None) == ARG and stats(N=0) == ARG and stats(W=-1) == ARG
    assert stats(N=1, H=1, W=1) == ARG                              # batch statistics of one value per channel
    assert stats(rm=None) == ARG and stats(mom=1.5) == ARG and stats(eps=-1.0) == ARG and stats(ws=None) == ARG
    assert stats(training=0, rm=None, rv=None) == ARG               # eval mode without running statistics
    assert stats(**huge) == UNSUPPORTED
    need = lib.cdn_codenet_head_fp32_workspace_bytes(1, 64, 72, 116)
    assert stats(N=1, H=72, W=116, nbytes=need - 1) == WORKSPACE and stats(ws=one + 4) == WORKSPACE

    def dwf(y1=one, w2=one, y2=one, N=2, C=64, H=8, W=8):
        return lib.cdn_codenet_head_fp32_dw_forward(y1, one, one, one, one, w2, y2, N, C, H, W, None)

    assert dwf(y1=None) == ARG and dwf(w2=None) == ARG and dwf(y2=None) == ARG and dwf(H=0) == ARG
    assert dwf(**huge) == UNSUPPORTED

    def tailf(y2=one, y3=one, Co=2, N=2, C=64, H=8, W=8):
        return lib.cdn_codenet_head_fp32_tail_forward(y2, one, one, one, one, one, one, y3, N, C, Co, H, W, None)

    assert tailf(y2=None) == ARG and tailf(y3=None) == ARG and tailf(C=0) == ARG
    assert tailf(Co=5) == UNSUPPORTED and tailf(Co=0) == ARG and tailf(Co=-1) == ARG and tailf(**huge) == UNSUPPORTED

    def tailb(g=one, gz=one, Co=2, N=2, C=64, H=8, W=8, ws=one, nbytes=big):
        return lib.cdn_codenet_head_fp32_tail_backward(g, one, one, one, one, one, one, gz, one, one, one, one, one, one, N, C,
                                                       Co, H, W, ws, nbytes, None)

    assert tailb(g=None) == ARG and tailb(gz=None) == ARG and tailb(ws=None) == ARG and tailb(N=0) == ARG
    assert tailb(Co=5) == UNSUPPORTED and tailb(Co=0) == ARG and tailb(**huge) == UNSUPPORTED
    assert tailb(N=1, H=72, W=116, nbytes=need - 1) == WORKSPACE and tailb(ws=one + 8) == WORKSPACE

    def bwd1(g=one, gz=one + 64, N=2, C=64, H=8, W=8, ws=one, nbytes=big):
        return lib.cdn_codenet_head_fp32_bn_backward1(g, one, one, one, one, one, gz, one, one, one, one, N, C, H, W, ws, nbytes,
                                                      None)

    assert bwd1(g=None) == ARG and bwd1(gz=None) == ARG and bwd1(gz=one) == ARG and bwd1(W=0) == ARG
    assert bwd1(**huge) == UNSUPPORTED and bwd1(N=1, H=72, W=116, nbytes=need - 1) == WORKSPACE

    def dwb(gz2=one, mb2=one, gz1=one, training2=1, N=2, C=64, H=8, W=8, ws=one, nbytes=big):
        return lib.cdn_codenet_head_fp32_dw_backward(gz2, one, one, one, one, mb2, one, training2, one, one, one, one, one, one,
                                                     gz1, one, one, one, one, one, N, C, H, W, ws, nbytes, None)

    assert dwb(gz2=None) == ARG and dwb(gz1=None) == ARG and dwb(mb2=None) == ARG and dwb(ws=None) == ARG and dwb(C=0) == ARG
    assert dwb(**huge) == UNSUPPORTED
    assert dwb(N=1, H=72, W=116, nbytes=need - 1) == WORKSPACE and dwb(ws=one + 4) == WORKSPACE

    def bwd2(gz=one, gy=one, pitch=3 * 64 * 64, N=2, C=64, H=8, W=8, training=1, mb=one):
        return lib.cdn_codenet_head_fp32_bn_backward2(gz, one, one, one, one, mb, one, gy, pitch, N, C, H, W, training, None)

    assert bwd2(gz=None) == ARG and bwd2(gy=None) == ARG and bwd2(mb=None) == ARG and bwd2(N=0) == ARG
    assert bwd2(pitch=64 * 64 - 1) == ARG                           # an image pitch below C * H * W
    assert bwd2(**dict(huge, pitch=256 * 512 * 512)) == UNSUPPORTED and bwd2(N=64, pitch=1 << 26) == UNSUPPORTED
