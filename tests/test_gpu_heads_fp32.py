"""The native fp32 detection heads on the GPU (csrc/codenet_heads_fp32_train.hip, functions/codenet_heads_fp32.py) against
their numpy restatement (tests/heads_fp32_ref.py), against the framework's operators in float64
under autograd stage by stage, against the float32 module path, in eval mode, behind the gate and as a captured training step.

What is compared how.  Everything the library's own fixed-order kernels leave -- y2, y3 of a narrow head, both
BatchNorms' numbers and buffers, g_z2, g_z1, grad_y1, the gradients of gamma, beta, W2 and a narrow head's W3 / b3 -- is
`torch.equal` to the restatement, which follows the kernels' sum orders, on ANY input.  The dense 1x1 convolutions run on
MFMA kernels whose order is not restated: y1, a wide head's y3, grad_a2 and grad_b3 are bit for bit where the inputs make
every order exact (the exact cases), while a wide head's grad_W3, grad_W1 and grad_x -- sums of products of BatchNorm
outputs, exact in no arithmetic -- are held to float64 on the GPU's own operands within (n + 2) 2^-24 sum |terms|.  On
random inputs a wide head's grad_a2 is an MFMA sum of Co inexact products too: its g_z2 is held to (Co + 2) 2^-24 sum |terms|
of float64 and to an exact zero where z2 <= 0, and g_z1, grad_y1 and the sums behind it are bit for bit the restatement
evaluated on that g_z2 (in the eval-mode test the wide head is held to the stage bounds alone)."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import bn_block_ref as R
from tests import heads_fp32_ref as HR
from tests import qat_support
from tests.test_gpu_bn_block import REL
from tests.test_heads_fp32_host import (C, SHAPES, WIDTHS, exact_case, head_params, random_case, restate,
                                        stage_ratios)

pytestmark = pytest.mark.gpu

CASES = [(s, dict(WIDTHS, hm=K)) for s, K in SHAPES] + [((2, 64, 9, 10), {"hm": 5, "wh": 2, "reg": 3})]
IDS = ["%dx%dx%d-%s" % (s[0], s[2], s[3], "-".join(str(v) for v in w.values())) for s, w in CASES]
PARAMS = ("0.weight", "1.weight", "1.bias", "3.weight", "4.weight", "4.bias", "6.weight", "6.bias")


def _np(t):
    return t.detach().cpu().numpy()


def _eq(got, want):
    return torch.equal(got.detach().cpu().reshape(-1), torch.from_numpy(np.ascontiguousarray(want)).reshape(-1))


def _collect(heads, xd, out, keep):
    """Everything one forward + backward left, by head."""
    res = {"grad_x": xd.grad}
    for h, m in heads.items():
        k = keep.get(h, {})
        res[h] = dict(k, y3=out[h], grads={n: p.grad for n, p in m.named_parameters()},
                      buffers={n: b for n, b in m.named_buffers()})
    return res


def _run(heads, x, gys, native=True):
    """One forward + backward of forward_heads on the GPU on a copy of `heads`: (result, the copy)."""
    from codenet_amd.functions import codenet_heads as CH, codenet_heads_fp32 as HF
    heads = {h: copy.deepcopy(m).cuda() for h, m in heads.items()}
    xd = x.cuda().requires_grad_(True)
    keep = {}
    HF.NATIVE_FP32_HEADS = native
    try:
        with torch.backends.cudnn.flags(deterministic=True):
            out = CH.forward_heads(heads, xd, keep)
            torch.autograd.backward([out[h] for h in heads], [gys[h].cuda() for h in heads])
    finally:
        HF.NATIVE_FP32_HEADS = True
    return _collect(heads, xd, out, keep), heads


def _flat(r):
    g = r["grads"]
    return dict(y1=_np(r["y1"]), y2=_np(r["y2"]), y3=_np(r["y3"]), g_z2=_np(r["g_z2"]), g_z1=_np(r["g_z1"]),
                grad_y1=_np(r["grad_y1"]), grad_g1=_np(g["1.weight"]), grad_b1=_np(g["1.bias"]), grad_g2=_np(g["4.weight"]),
                grad_b2=_np(g["4.bias"]), grad_w2=_np(g["3.weight"]), grad_w3=_np(g["6.weight"]), grad_b3=_np(g["6.bias"]))


def _mfma_sums(res, heads, x, what):
    """grad_W1 of every head, grad_x and a wide head's grad_W3 against float64 on the GPU's own operands (grad_y1, x, a2
    from the GPU's y2 and numbers) within (n + 2) 2^-24 sum |terms| (qat_support.bound)."""
    x64 = x.double()
    n = x.shape[0] * x.shape[2] * x.shape[3]
    gx, gx_abs = torch.zeros_like(x64), torch.zeros_like(x64)
    for h, m in heads.items():
        gy1 = res[h]["grad_y1"].double().cpu()
        w1 = m[0].weight.detach().double().cpu().view(C, C)
        qat_support.within(res[h]["grads"]["0.weight"].view(C, C), torch.einsum("nohw,nchw->oc", gy1, x64), n,
                           torch.einsum("nohw,nchw->oc", gy1.abs(), x64.abs()), "%s %s grad_W1" % (what, h))
        gx += torch.einsum("oc,nohw->nchw", w1, gy1)
        gx_abs += torch.einsum("oc,nohw->nchw", w1.abs(), gy1.abs())
        Co = m[6].out_channels
        if Co > 4:
            st = [_np(t) for t in res[h]["bn2"]]
            a2 = torch.from_numpy(R.forward(_np(res[h]["y2"]), st[0], st[2], _np(m[4].weight), _np(m[4].bias), 1)).double()
            g = res[h]["gy3"].double()
            qat_support.within(res[h]["grads"]["6.weight"].view(Co, C), torch.einsum("nohw,nchw->oc", g, a2), n,
                               torch.einsum("nohw,nchw->oc", g.abs(), a2.abs()), "%s %s grad_W3" % (what, h))
    qat_support.within(res["grad_x"], gx, len(heads) * C, gx_abs, "%s grad_x" % what)


def _check_against_restatement(res, ref, heads, step, exact):
    """torch.equal to the restatement `ref` (of the heads' state before the first step) after `step` steps on one batch."""
    for h, m in heads.items():
        r, want = res[h], ref[h]
        Co = m[6].out_channels
        assert _eq(r["y1"], want["y1"]) and _eq(r["y2"], want["y2"]), h
        if Co <= 4 or exact:
            assert _eq(r["y3"], want["y3"]), h
        for k in (1, 2):
            st, bn = want["st%d" % k], m[3 * k - 2]
            assert all(_eq(a, st[key]) for a, key in zip(r["bn%d" % k], ("mean", "var", "invstd"))), (h, k)
            rm, rv = want["rm%d" % k], want["rv%d" % k]
            if bn.training:
                for _ in range(step - 1):
                    rm, rv = R.running_update(rm, rv, st, bn.momentum)
            assert _eq(bn.running_mean, rm) and _eq(bn.running_var, rv), (h, k)
            assert int(bn.num_batches_tracked) == (step if bn.training else 0), (h, k)
        tb, db, g = want["tail"], want["dw"], r["grads"]
        assert _eq(r["g_z2"], tb["g_z"]) and _eq(r["means2"][0], tb["mb"]) and _eq(r["means2"][1], tb["mg"]), h
        assert _eq(g["4.weight"], tb["grad_gamma"]) and _eq(g["4.bias"], tb["grad_beta"]), h
        assert _eq(r["g_z1"], db["g_z"]) and _eq(r["means1"][0], db["mb"]) and _eq(r["means1"][1], db["mg"]), h
        assert _eq(g["3.weight"], db["grad_w2"]) and _eq(g["1.weight"], db["grad_gamma"]), h
        assert _eq(g["1.bias"], db["grad_beta"]) and _eq(r["grad_y1"], want["grad_y1"]), h
        if Co <= 4:
            assert _eq(g["6.weight"], tb["grad_w3"]) and _eq(g["6.bias"], tb["grad_b3"]), h
        elif exact:
            assert _eq(g["6.bias"], tb["grad_b3"]), h


@pytest.mark.parametrize("shape,widths", CASES, ids=IDS)
def test_exact_arithmetic_eager_and_on_two_graph_replays(shape, widths):
    """Coarse-grid inputs (tests/test_heads_fp32_host.exact_case; the 5 x 7 case with beta1 > 0, where a padded tap computed
    as relu(bn_z(0)) shows): y1, y2, y3, both BatchNorms' mean / var / invstd, running buffers and counters, every parameter
    gradient the library's own kernels sum and every intermediate are the restatement's bit for bit -- eagerly, and after
    each of two replays of a HIP graph of the same calls (the buffers advance three times); grad_W1, grad_x and a wide
    head's grad_W3 within (n + 2) 2^-24 sum |terms| of float64 on the GPU's own operands, and bit-identical across the three."""
    from codenet_amd.functions import codenet_heads as CH
    heads, x, gys = exact_case(shape, widths, 11, beta1_positive=(shape[2:] == (5, 7)))
    ref = restate(heads, x, gys)
    side = torch.cuda.Stream()      # (eager run and capture on one stream: the parameters' autograd nodes live there)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res, hd = _run(heads, x, gys)
    torch.cuda.synchronize()
    for h in hd:
        res[h]["gy3"] = gys[h]
    _check_against_restatement(res, ref, hd, 1, True)
    _mfma_sums(res, hd, x, "eager")
    first = {(h, n): g.clone() for h in hd for n, g in res[h]["grads"].items()}
    first["x"] = res["grad_x"].clone()
    # the same calls captured on the same modules: their buffers advance in place on every replay
    xd = x.cuda().requires_grad_(True)
    gyd = [gys[h].cuda() for h in hd]
    for m in hd.values():
        m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    keep = {}
    with torch.cuda.graph(graph, stream=side):
        out = CH.forward_heads(hd, xd, keep)
        torch.autograd.backward([out[h] for h in hd], gyd)
    for step in (2, 3):
        for t in [xd.grad] + [p.grad for m in hd.values() for p in m.parameters()] + [out[h] for h in hd]:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        rep = _collect(hd, xd, out, keep)
        _check_against_restatement(rep, ref, hd, step, True)
        assert torch.equal(rep["grad_x"], first["x"])
        assert all(torch.equal(rep[h]["grads"][n], first[(h, n)]) for h in hd for n in PARAMS)


@functools.lru_cache(maxsize=None)
def _random(i):
    """The random inputs of case i, the GPU's native result and the modules after it, computed once."""
    shape, widths = CASES[i]
    heads, x, gys = random_case(shape, widths, 1000 + i)
    res, hd = _run(heads, x, gys)
    for h in hd:
        res[h]["gy3"] = gys[h]
    return heads, x, gys, res, hd


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_own_intermediates_on_random_inputs(i):
    """Random inputs: the per-channel numbers within 2^-24 |ref| + n 2^-52 sum |terms| of float64 (bn_block_ref.channel_bound);
    y2, y3 of the narrow heads, g_z2, g_z1, grad_y1, the per-channel numbers themselves and the float64-summed gradients
    torch.equal to the restatement evaluated on the GPU's own y1 (it follows the kernels' sum orders); y1 within 65 u sum
    |w x| of float64 (stage_ratios)."""
    heads, x, gys, res, hd = _random(i)
    ref = restate(heads, x, gys, y1={h: _np(res[h]["y1"]) for h in hd})
    if any(m[6].out_channels > 4 for m in heads.values()):      # a wide head's grad_a2 is the GPU's own: read back from g_z2
        for h, m in heads.items():
            if m[6].out_channels > 4:
                p = head_params(m)
                y2, st2 = ref[h]["y2"], ref[h]["st2"]
                z2, _ = R.bn_z(y2, st2["mean"], st2["invstd"], p["g2"], p["b2"])
                ga2 = HR.conv1x1_64(gys[h].numpy(), p["w3"].T)
                gz2 = _np(res[h]["g_z2"])
                assert np.all(gz2[~(z2 > 0)] == 0), h
                bound = qat_support.bound(p["w3"].shape[0], HR.conv1x1_64(np.abs(gys[h].numpy()), np.abs(p["w3"]).T))
                assert np.all(np.abs(gz2 - ga2)[z2 > 0] <= bound[z2 > 0]), h
                tb = HR.bn_backward1(np.where(z2 > 0, gz2, np.float32(0)), y2, st2, p["g2"], p["b2"])
                db = HR.dw_backward(tb["g_z"], y2, st2, p["g2"], tb["mb"], tb["mg"], p["train2"], ref[h]["y1"], ref[h]["st1"],
                                    p["g1"], p["b1"], p["w2"])
                ref[h]["tail"].update(tb)
                ref[h].update(dw=db, grad_y1=R.backward_gy(db["g_z"], ref[h]["y1"], ref[h]["st1"]["mean"],
                                                           ref[h]["st1"]["invstd"], p["g1"], db["mb"], db["mg"], p["train1"]))
    _check_against_restatement(res, ref, hd, 1, False)
    for h in hd:
        for k, y in ((1, res[h]["y1"]), (2, res[h]["y2"])):
            st = R.batch_stats(_np(y), hd[h][1].eps)
            n = st["n"]
            mean, var = _np(res[h]["bn%d" % k][0]), _np(res[h]["bn%d" % k][1])
            assert np.all(np.abs(mean - st["mean_d"]) <= R.channel_bound(st["mean_d"], n, st["abs1"] / n)), (h, k)
            assert np.all(np.abs(var - st["var_d"]) <= R.channel_bound(st["var_d"], n, st["s2"] / n + st["mean_d"] ** 2)), (h, k)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_float64_stage_by_stage_and_against_the_module_path(i):
    """Against the module path's operators in float64 on the CPU: every stage as F.conv2d / F.batch_norm / F.relu compute it
    under float64 autograd (stage_ratios; no reference is a formula of the test's own) on the float32 inputs the GPU gave
    that stage, within the bounds DESIGN.md section 4.3f derives by operation count (the constants of tests/test_heads_fp32_host.py: 8 u S for z, 10 roundings for a
    depthwise term, 66 for a 1x1 term, 23 u B for grad_y, 6 u A for xh); elements whose float64 z lies within 8 u S of zero
    are left out of the ReLU-dependent comparisons (at most 1e-4 of a tensor; seen: at most 1.9e-6).  Seen fractions of the
    bounds on an MI355X, largest over the cases: y1 0.09, y2 0.24, y3 0.06, g_z2 0.63, g_z1 0.10, grad_y1 0.15, grad_beta
    0.98 (one rounding: its bound IS one rounding), grad_gamma 0.44, grad_w2 0.04, grad_w3 0.14, grad_b3 0.43 (the prints
    below show them).
    The whole heads against the float32 module path on the GPU (NATIVE_FP32_HEADS off): outputs, every parameter gradient,
    grad_x and every running buffer within REL = 2e-4 of the tensor's magnitude (seen: at most 4.9e-6); `keep` is filled
    only with the switch on."""
    heads, x, gys, res, hd = _random(i)
    n = x.shape[0] * x.shape[2] * x.shape[3]
    for h, m in heads.items():
        ratios, left_out = stage_ratios(x.numpy(), head_params(m), _flat(res[h]), gys[h].numpy(),
                                        1 if m[6].out_channels <= 4 else n + 1)
        print(h, "left out %.2g;" % left_out, {k: round(v, 3) for k, v in ratios.items()})
        assert left_out <= 1e-4 and all(v <= 1.0 for v in ratios.values()), (h, ratios)
    _mfma_sums(res, hd, x, "random")
    off, hd_off = _run(heads, x, gys, native=False)
    assert all("y1" not in off[h] for h in heads) and all("y1" in res[h] for h in heads)      # keep: only when on
    worst = 0.0

    def close(a, b, what):
        nonlocal worst
        d, mag = (a - b).abs().max().item(), b.abs().max().item()
        worst = max(worst, d / (mag + 1e-30))
        assert d <= REL * mag, (what, d, mag)

    # Two values per channel (the 1 x 1 planes at N = 2): xh = +-1 / sqrt(1 + eps / var) whatever y is, so BatchNorm's output
    # does not depend on its input and grad_y is the derivative of a constant up to eps -- (g_z - mb) - xh mg cancels to
    # rounding noise in BOTH float32 evaluations (seen: |grad_W1| ~ 3e-5 against terms of ~ 1).  Noise has no magnitude to
    # be relative to, so everything behind a BatchNorm's second pass is left to the stage-wise bounds above (which are
    # relative to the terms) and to the bit-for-bit tests; outputs, buffers and what is in front of it are compared.
    behind_bn2 = PARAMS if n > 2 else ("4.weight", "4.bias", "6.weight", "6.bias")
    if n > 2:
        close(res["grad_x"], off["grad_x"], "grad_x")
    for h in heads:
        close(res[h]["y3"], off[h]["y3"], h + " y3")
        for k in behind_bn2:
            close(res[h]["grads"][k], off[h]["grads"][k], "%s grad %s" % (h, k))
        for k, b in off[h]["buffers"].items():
            if b.is_floating_point():
                close(res[h]["buffers"][k], b, "%s %s" % (h, k))
            else:
                assert int(b) == int(res[h]["buffers"][k]) == 1
    print("native against the module path: %.2g of the magnitude at worst (REL %.0e)" % (worst, REL))


@pytest.mark.parametrize("modes", [(False, False), (True, False), (False, True)])
def test_eval_mode_batchnorm_under_grad(modes):
    """Each BatchNorm follows its own training flag: in eval mode the running statistics are the operands, the backward
    drops the two subtracted terms, and no buffer is written -- bit for bit the restatement, and within the stage bounds."""
    shape, widths = CASES[6]
    heads, x, gys = random_case(shape, widths, 77)
    for m in heads.values():
        m[1].train(modes[0])
        m[4].train(modes[1])
    res, hd = _run(heads, x, gys)
    ref = restate(heads, x, gys, y1={h: _np(res[h]["y1"]) for h in hd})
    for h, m in heads.items():
        if m[6].out_channels > 4:
            continue                       # (the wide head's grad_a2 is the MFMA kernel's: covered by the stage bounds)
        _check_against_restatement({h: res[h]}, {h: ref[h]}, {h: hd[h]}, 1, False)
    for h, m in heads.items():
        for i, train in ((1, modes[0]), (4, modes[1])):
            if not train:
                assert torch.equal(hd[h][i].running_mean.cpu(), m[i].running_mean), (h, i)
                assert torch.equal(hd[h][i].running_var.cpu(), m[i].running_var) and int(hd[h][i].num_batches_tracked) == 0
                assert _eq(res[h]["bn%d" % (1 if i == 1 else 2)][0], _np(m[i].running_mean))
        ratios, left_out = stage_ratios(x.numpy(), head_params(m), _flat(res[h]), gys[h].numpy(),
                                        1 if m[6].out_channels <= 4 else x.shape[0] * x.shape[2] * x.shape[3] + 1)
        assert left_out <= 1e-4 and all(v <= 1.0 for v in ratios.values()), (h, ratios)


def test_one_value_per_channel_in_training_mode_raises():
    from codenet_amd.functions import codenet_heads as CH
    heads, _, _ = random_case((1, 64, 1, 1), WIDTHS, 5)
    heads = {h: m.cuda() for h, m in heads.items()}
    with pytest.raises(ValueError, match="more than 1 value per channel"):      # (before any launch)
        CH.forward_heads(heads, torch.rand(1, 64, 1, 1, device="cuda").requires_grad_(True))
    assert all(int(m[1].num_batches_tracked) == 0 for m in heads.values())


def test_a_hooked_inner_module_takes_the_module_path():
    from codenet_amd.functions import codenet_heads as CH, codenet_heads_fp32 as HF
    heads, x, gys = random_case((2, 64, 9, 10), WIDTHS, 6)
    off, _ = _run(heads, x, gys, native=False)
    fired = []
    heads["wh"][3].register_forward_hook(lambda m, i, o: fired.append(1))
    got, hd = _run(heads, x, gys)
    xd = x.cuda().requires_grad_(True)
    assert "hook" in HF.native_reason(hd, xd)
    assert fired and all("y1" not in got[h] for h in heads)
    assert torch.equal(got["grad_x"], off["grad_x"]) and all(torch.equal(got[h]["y3"], off[h]["y3"]) for h in heads)
    clean = {h: copy.deepcopy(m).cuda() for h, m in random_case((2, 64, 9, 10), WIDTHS, 6)[0].items()}
    assert HF.native_reason(clean, xd) is None
    with torch.no_grad():      # inference is untouched: the gate refuses
        assert "grad mode" in HF.native_reason(clean, xd)
    assert "contiguous" in HF.native_reason(clean, xd.detach().transpose(2, 3).requires_grad_(True))
    assert "nothing to differentiate" in HF.native_reason({h: m.requires_grad_(False) for h, m in clean.items()}, xd.detach())


# ---- the captured step ------------------------------------------------------------------------------------------------------

def _tail():
    from codenet_amd import harness, pipeline
    return pipeline.DetectionTail(harness.create_model(heads={"hm": 20, "wh": 2, "reg": 2})).cuda().train()


def _tail_setup():
    return qat_support.step_setup(lambda g, N, R_: torch.randn(N, 1024, 4, 4, generator=g).abs_() * 1.66, 5)


def test_fp32_tail_captured_step_replays_the_eager_step_bit_for_bit():
    """GraphedTrainStep(DetectionTail(fp32 model).train(), capturable Adam, CtdetLoss) WITHOUT unvalidated=True (on the
    parent commit: NotImplementedError): replays bit-identical to eager steps in loss, parameters, BatchNorm buffers and
    Adam state; every head parameter took part."""
    from codenet_amd import pipeline
    from codenet_amd.functions import codenet_heads_fp32 as HF
    loss_fn, feats = _tail_setup()
    eager, (net_g, opt_g) = [qat_support.with_capturable_adam(_tail()) for _ in range(2)]
    G = pipeline.GraphedTrainStep
    assert G.is_fp32_tail(net_g) and not G.is_native_tail(net_g) and not G.is_stage_stack(net_g)
    assert HF.native_reason(net_g.head_modules(), torch.empty(2, 64, 32, 32, device="cuda")) is None
    qat_support.check_captured_step(eager, (net_g, opt_g), loss_fn, feats, lambda n: n.split(".")[0] in ("hm", "wh", "reg"))
    assert int(net_g.hm[1].num_batches_tracked) == 7 and int(net_g.deconv_layers[1].num_batches_tracked) == 7
    HF.NATIVE_FP32_HEADS = False      # with the switch off the same net runs the framework's backward: not validated
    try:
        assert not G.is_fp32_tail(net_g)
        with pytest.raises(NotImplementedError, match="NATIVE_FP32_HEADS is off"):
            G(net_g, opt_g, loss_fn, (feats[0],))
    finally:
        HF.NATIVE_FP32_HEADS = True


def test_fp32_tail_two_identical_runs_end_bit_identical():
    loss_fn, feats = _tail_setup()
    qat_support.check_two_identical_runs(_tail, loss_fn, feats[:4])
