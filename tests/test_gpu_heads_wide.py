"""Heads with more than 32 outputs (COCO: an 80-class heat map) on the fused head tail: class groups of 32 on the int8
matrix cores (head_small_kernel MODE 2, cdn_codenet_head_tail_small_forward / _q8_forward), the gates of
pipeline.FusedHeads that send such a head there, and the serving plan of an 80-class model.  Equalities only: the tail
is bit-identical to the unfused schedule and to itself called once per slice of 32 classes."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _cap():
    from codenet_amd import _native as N_
    return N_.lib().cdn_codenet_head_tail_max_classes()


def _tail_inputs(N, Hs, Ws, classes, dev):
    """As test_head_tail_on_byte_codes_equals_the_fp32_form: y1 inside its QuantAct's range, so that the byte codes of
    y1 exist; 4-bit weight codes with their scales, column sums and bias."""
    from codenet_amd import ops
    g = torch.Generator().manual_seed(Hs * Ws + classes)
    y1 = (torch.rand(N, Hs * Ws, 64, generator=g) * 4.0).to(dev)
    q1 = ops.quantact_state(dev)
    q2 = ops.quantact_state(dev)
    q1.view(torch.float32)[2], q1.view(torch.float32)[3] = 255.0 / 4.2, 128.0 - 3.0
    q2.view(torch.float32)[2], q2.view(torch.float32)[3] = 11.0, 128.0
    s1, z1 = q1.view(torch.float32)[2], q1.view(torch.float32)[3]
    codes = torch.round(s1 * y1 - z1)
    assert codes.min().item() >= -128 and codes.max().item() <= 127
    wq = torch.randint(-8, 8, (classes, 64), generator=g, dtype=torch.int32)
    return dict(
        y1=y1, y8=codes.to(torch.int8).contiguous(), q1=q1, q2=q2,
        w_dw=(torch.randn(64, 9, generator=g) * 0.3).to(dev), b_dw=(torch.randn(64, generator=g) * 0.1).to(dev),
        w_codes=wq.to(torch.int8).to(dev), w_scale=(torch.rand(classes, generator=g) * 10 + 3).to(dev),
        w_colsum=wq.sum(1).to(torch.int32).to(dev), bias=(torch.randn(classes, generator=g) * 0.1).to(dev))


def _tail(t, N, Hs, Ws, lo, hi, q8, out, flag=None):
    """One call of the tail on classes [lo, hi) -> the entry's return code."""
    from codenet_amd import _native as N_
    lib = N_.lib()
    st = torch.cuda.current_stream().cuda_stream
    args = [t["q1"].data_ptr(), N, 64, Hs, Ws, t["w_dw"].data_ptr(), t["b_dw"].data_ptr(), t["q2"].data_ptr(),
            t["w_codes"].data_ptr() + lo * 64, t["w_scale"].data_ptr() + lo * 4, t["w_colsum"].data_ptr() + lo * 4,
            t["bias"].data_ptr() + lo * 4, hi - lo, out.data_ptr()]
    if q8:
        return lib.cdn_codenet_head_tail_small_q8_forward(t["y8"].data_ptr(), *args, flag.data_ptr(), st)
    return lib.cdn_codenet_head_tail_small_forward(t["y1"].data_ptr(), *args, st)


def _in_slices(t, N, Hs, Ws, K, q8, flag=None):
    """The tail on consecutive slices of at most 32 classes (one class group each), concatenated on dim 1."""
    from codenet_amd import _native as N_
    parts = []
    for lo in range(0, K, 32):
        hi = min(K, lo + 32)
        o = torch.zeros(N, hi - lo, 2 * Hs, 2 * Ws, device=t["y1"].device)
        N_.check(_tail(t, N, Hs, Ws, lo, hi, q8, o, flag), "tail on classes [%d, %d)" % (lo, hi))
        parts.append(o)
    return torch.cat(parts, 1)


@pytest.mark.parametrize("N,Hs,Ws", [(2, 16, 16), (1, 12, 48), (3, 8, 32)])
@pytest.mark.parametrize("K", [33, 64, 65, 80, "cap"])
def test_wide_tail_equals_itself_in_slices_of_32_classes(N, Hs, Ws, K):
    """cdn_codenet_head_tail_small_forward with K > 32 classes against the same entry on slices of at most 32 classes
    (weight codes, scales, column sums and bias offset, outputs concatenated): torch.equal, for the fp32 form and for
    the byte-code form; the byte-code form equals the fp32 form on the tensor that produced the codes, reports no
    overflow, and reports one once the y2 scale pushes levels outside the nibble split."""
    from codenet_amd import _native as N_
    dev = torch.device("cuda", 0)
    K = _cap() if K == "cap" else K
    t = _tail_inputs(N, Hs, Ws, K, dev)
    a = torch.zeros(N, K, 2 * Hs, 2 * Ws, device=dev)
    N_.check(_tail(t, N, Hs, Ws, 0, K, False, a), "fp32 tail")
    want = _in_slices(t, N, Hs, Ws, K, False)
    assert want.abs().max().item() > 0 and torch.equal(a, want), (a - want).abs().max().item()
    of, of_s = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    b = torch.zeros_like(a)
    N_.check(_tail(t, N, Hs, Ws, 0, K, True, b, of), "byte tail")
    want8 = _in_slices(t, N, Hs, Ws, K, True, of_s)
    assert torch.equal(b, want8) and torch.equal(b, a)
    assert of.item() == 0 and of_s.item() == 0
    t["q2"].view(torch.float32)[2] = 4000.0
    N_.check(_tail(t, N, Hs, Ws, 0, K, True, b, of), "byte tail")
    assert of.item() == 1


def test_wide_tail_refuses_more_than_its_cap_before_any_launch():
    """classes = cap + 1: both entries return an error and the output buffer keeps its sentinel."""
    dev = torch.device("cuda", 0)
    N, Hs, Ws, K = 1, 8, 16, _cap() + 1
    assert K - 1 >= 128
    t = _tail_inputs(N, Hs, Ws, K, dev)
    of = torch.zeros(1, dtype=torch.int32, device=dev)
    for q8 in (False, True):
        out = torch.full((N, K, 2 * Hs, 2 * Ws), -7.5, device=dev)
        assert _tail(t, N, Hs, Ws, 0, K, q8, out, of) != 0
        torch.cuda.synchronize()
        assert bool((out == -7.5).all()) and of.item() == 0


def _head_modules(C, classes, g, quantized, pct=False):
    """name -> head module (fp32 nn.Sequential or QuantDepthwiseNode) with seeded weights (tests/test_gpu_parity.py)."""
    import torch.nn as nn
    from codenet_amd.portable_quantizer import quant_modules as qm
    heads = {}
    for name, ncls in classes.items():
        def bn(c):
            b = nn.BatchNorm2d(c)
            b.weight.data = torch.rand(c, generator=g) + 0.5
            b.bias.data = torch.randn(c, generator=g) * 0.1
            b.running_mean = torch.randn(c, generator=g) * 0.1
            b.running_var = torch.rand(c, generator=g) + 0.5
            return b
        seq = nn.Sequential(nn.Conv2d(C, C, 1, bias=False), bn(C), nn.ReLU(inplace=True),
                            nn.Conv2d(C, C, 3, 1, 1, groups=C, bias=False), bn(C), nn.ReLU(inplace=True),
                            nn.Conv2d(C, ncls, 1, bias=True)).eval()
        seq[0].weight.data = torch.randn(C, C, 1, 1, generator=g) * (1.5 / C) ** 0.5
        seq[3].weight.data = torch.randn(C, 1, 3, 3, generator=g) / 3
        seq[6].weight.data = torch.randn(ncls, C, 1, 1, generator=g) * (1.0 / C) ** 0.5
        seq[6].bias.data = torch.randn(ncls, generator=g) * 0.1
        if quantized:
            q = qm.QuantDepthwiseNode(4, 8, act_percentile=False, wt_quant_mode="symmetric",
                                      act_quant_mode="asymmetric", per_channel=True,
                                      weight_percentile=pct)
            q.set_param(seq)
            heads[name] = q.eval()
        else:
            heads[name] = seq
    return heads


WIDE_HEADS = {"hm80": 80, "c33": 33, "c64": 64, "c128": 128, "wh": 2}


@pytest.mark.parametrize("res,batch,fused", [(4, 2, True), (12, 1, True), (6, 2, False)])
def test_wide_heads_on_the_fused_tail_are_bit_identical_to_the_unfused_schedule(res, batch, fused):
    """FusedHeads(small_tail=True) against small_tail=False for heads of 33..128 outputs over four forwards from fresh
    running ranges (the first ones run with codes too wide for int8: the VALU launch behind the matrix launch): identical
    outputs and QuantAct buffers, as test_head_small_tail_is_bit_identical_to_unfused_schedule asserts them.  The fused
    side never allocates the unfused schedule's full-resolution scratch -- except at Ws = 24 (res 6), where the gate
    (Ws % 16) sends the wide heads to the unfused schedule on both sides."""
    from codenet_amd import pipeline
    planes = [64, 32, 16, 64]
    net = pipeline.build_hot_path(quantized=True, planes=planes, seed=5).cuda()
    g = torch.Generator().manual_seed(res)
    heads = _head_modules(64, WIDE_HEADS, g, True)
    ha = {k: copy.deepcopy(v).cuda() for k, v in heads.items()}
    hb = {k: copy.deepcopy(v).cuda() for k, v in heads.items()}
    path = pipeline.FusedHotPath(net.deconv_layers)
    fa = pipeline.FusedHeads(ha, small_tail=True)
    fb = pipeline.FusedHeads(hb, small_tail=False)
    exact = 0
    for it in range(4):
        x = (torch.randn(batch, planes[0], res, res, generator=g).abs() * (1.0 + 0.2 * it)).cuda()
        r, rq, shape = path.forward_nhwc(x)
        assert shape["W"] == 4 * res
        oa = {k: v.clone() for k, v in fa(r, rq, shape).items()}
        ob = fb(r, rq, shape)
        for k in oa:
            wide = hb[k].quant_act3[1]._device_state(x.device)[6].item() != 0
            if wide:       # f32-MFMA branch of the pointwise kernel on one side: fp32 rounding of the same sums
                assert (oa[k] - ob[k]).abs().max().item() < 1e-4 * (1 + ob[k].abs().max().item()), \
                    (k, it, "wide", (oa[k] - ob[k]).abs().max().item(), ob[k].abs().max().item())
            else:
                assert torch.equal(oa[k], ob[k]), (k, it, (oa[k] - ob[k]).abs().max().item())
                exact += 1
    assert exact >= 3 * len(ha) - 6, exact
    for k in ha:
        for aa, bb in ((ha[k].quant_act1[1], hb[k].quant_act1[1]), (ha[k].quant_act3[1], hb[k].quant_act3[1])):
            assert torch.equal(aa.x_min, bb.x_min) and torch.equal(aa.x_max, bb.x_max), \
                (k, aa.x_min.item(), bb.x_min.item(), aa.x_max.item(), bb.x_max.item())
    for k in ("hm80", "c33", "c64", "c128"):
        assert (k in fa._bufs["y2"]) == (not fused), k      # the unfused schedule's scratch tensor
        assert k in fb._bufs["y2"]
    assert "wh" not in fa._bufs["y2"]


def test_coco_model_serves_with_the_heads_on_byte_codes():
    """An 80-class W4A8 model in serving mode: the plan keeps the heads on the byte codes of the last stage (third
    member), and their outputs equal those of the same calibrated model with the heads on the expanded codes (FusedHeads
    with small_tail=False: codes_supported is False, the tails run unfused on fp32); no overflow on the calibration
    batch; harness.process returns finite detections of classes 0..79."""
    from codenet_amd import harness, pipeline
    heads = {"hm": 80, "wh": 2, "reg": 2}
    model = harness.create_model(heads=heads, quantize=True).cuda()
    other = copy.deepcopy(model)
    images = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(3)).cuda()
    rep = pipeline.prepare_serving(model, images, settle=20, margin=0.02)
    assert rep["clean"] and rep["byte_backbone"], rep
    assert model._plan(images) == ("bytes", True, True)
    other.load_state_dict(model.state_dict())
    pipeline.set_running_stat(other, False)
    other.enable_fused(frozen_codes=True)
    assert other._plan(images) == ("bytes", True, True)         # (builds the schedule objects)
    mods = {h: getattr(other, h) for h in other.heads}
    other._fheads = pipeline.FusedHeads(mods, small_tail=False)
    other._fzheads = pipeline.FusedHeads(mods, small_tail=False)
    other.__dict__["_plans"].clear()
    assert other._plan(images) == ("bytes", True, False)
    with torch.no_grad():
        model(images)
        other(images)
    assert not model.frozen_overflowed() and not other.frozen_overflowed()
    fresh = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        a = {k: v.clone() for k, v in model(fresh)[-1].items()}
        b = other(fresh)[-1]
    assert a["hm"].shape == (2, 80, 32, 32)
    for k in heads:
        assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())
    assert "hm" in other._fheads._bufs["y2"] and model._fzheads._bufs.get("y2") is None
    dets = harness.process(model, fresh, flip_test=False)[1]
    assert dets.shape[0] == 2 and torch.isfinite(dets).all()
    cls = dets[..., 5]
    assert bool((cls >= 0).all()) and bool((cls < 80).all()) and bool((cls == cls.round()).all())
