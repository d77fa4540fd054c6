"""W8A8 on the GPU: 8-bit weight codes on the int8 matrix cores (CDN_W_CODES_8BIT, include/codenet_dcn.h).

Arithmetic is checked with torch.equal against a numpy restatement of what the kernels compute: the activation level
L = rint(fl(fl(s x) - z)) + z formed in float32 operation by operation, the int64 sum of L q, the epilogue
fma(float(sum), 1 / fl(s ws), bias) with ONE rounding (float64 product -- exact, 24 x 24 bits -- plus bias, rounded to
odd, then to float32), ReLU.  The same codes WITHOUT the flag run the kernels that hold 16 q in a byte and give other
sums -- that call is made and only required to differ nowhere it must not: nothing is asserted about wrong values.

Schedules (heads, stages, whole network, serving mode) are compared with the unfused schedule / the module path as their
W4A8 twins are: tests/test_gpu_heads_wide.py, tests/test_gpu_real_shapes.py, tests/test_harness.py."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from codenet_amd.pipeline import W_CODES_8BIT as W8      # CDN_W_CODES_8BIT  # noqa: E402


# ---- the restatement ------------------------------------------------------------------------------------------------

def _fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the float64 product is exact, the float64 sum is rounded to odd (TwoSum error
    term), so the final rounding to float32 is the single rounding of the fused operation."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def _levels(a, s, z):
    """QuantAct levels as the int8 kernels form them: two float32 roundings, rint (half to even), + z."""
    t = (np.float32(s) * a.astype(np.float32)).astype(np.float32) - np.float32(z)
    return np.rint(t.astype(np.float32)).astype(np.int64) + int(z)


def _expected(a, s, z, q, ws, bias, relu):
    """-> (float32 [M, Co], int64 sums).  a [M, C] float32, q [Co, C] integer codes, ws / bias [Co] float32."""
    L = _levels(a, s, z)
    assert np.abs(L - 128).max() <= 2040, "test construction: levels outside the nibble split"
    isum = L @ q.astype(np.int64).T
    assert np.abs(isum).max() < 2 ** 31 and np.abs(L - 128).max() * 128 * a.shape[1] < 2 ** 31
    rinv = (np.float32(1.0) / (np.float32(s) * ws.astype(np.float32)).astype(np.float32)).astype(np.float32)
    v = _fma32(isum.astype(np.int32).astype(np.float32), np.broadcast_to(rinv, isum.shape),
               np.broadcast_to(bias.astype(np.float32), isum.shape))
    return (np.maximum(v, np.float32(0)) if relu else v), isum


def _state(dev, s, z, wide=0):
    from codenet_amd import ops
    st = ops.quantact_state(dev)
    st.view(torch.float32)[2], st.view(torch.float32)[3] = float(s), float(z)
    st.view(torch.int32)[6] = int(wide)
    return st


def _codes8(Co, C, g, extremes=True):
    """int codes in [-128, 127] [Co, C]; rows 0 / 1 all 127 / all -128 when `extremes`."""
    q = torch.randint(-128, 128, (Co, C), generator=g, dtype=torch.int32)
    if extremes and Co >= 2:
        q[0] = 127
        q[1] = -128
    return q


def _pw_call(a, st, q, ws, bias, relu, flag, lda=0, w=None):
    """cdn_codenet_pointwise_nhwc_forward on codes q (padded to 64 columns) -> out [M, Co] (cpu numpy), rc."""
    from codenet_amd import _native as N_
    lib, dev = N_.lib(), a.device
    M, (Co, C) = a.shape[0], q.shape
    cp = torch.zeros(Co, (C + 63) // 64 * 64, dtype=torch.int8)
    cp[:, :C] = q.to(torch.int8)
    cp = cp.to(dev)
    wsd, bd = torch.from_numpy(ws).to(dev), torch.from_numpy(bias).to(dev)
    colsum = q.sum(1).to(torch.int32).to(dev)
    if w is None:
        w = (q.float() / torch.from_numpy(ws).view(-1, 1)).contiguous()
    w = w.to(dev)
    out = torch.full((M, Co), -7.5, device=dev)
    rc = lib.cdn_codenet_pointwise_nhwc_forward(
        a.data_ptr(), st.data_ptr(), M, C, Co, lda, 0, w.data_ptr(), cp.data_ptr(), wsd.data_ptr(), colsum.data_ptr(),
        bd.data_ptr(), None, None, int(relu) | flag, None, None, None, 8, 0.99, 0, None, 0, out.data_ptr(),
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rc


# ---- pointwise ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [24, 116, 232, 1024])
def test_pointwise_eight_bit_codes_equal_the_integer_restatement(C):
    """M in {1, 33, 257} (tails of the 32 / 64 / 128-row tiles) x Co in {20, 58, 80, 256} at K = C: a k tail below 32,
    non-multiples of 64, the long-K shape (tiled kernel: the streaming one is a 4-bit kernel).  Instantiations taken:
    Co > 64: 32 x 128 tiles (K < 256, and K >= 1024 with few tiles); Co <= 64: 128 x 64; whole-tile (K % 32 == 0) and
    ragged forms.  (The 64 x 128 and 64 x 64 tiles: test_every_tile_of_the_eight_bit_pointwise_is_exact_and_named.)
    Rows of 127s and of -128s in every case."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(C)
    for M in (1, 33, 257):
        for Co in (20, 58, 80, 256):
            s, z = 255.0 / 6.1, float(int(torch.randint(100, 140, (1,), generator=g)))
            a = (torch.rand(M, C, generator=g) * 7.0 - 0.6)            # levels from a few below 0 to a few above 255
            q = _codes8(Co, C, g)
            ws = (torch.rand(Co, generator=g) * 40 + 3).numpy().astype(np.float32)
            bias = (torch.randn(Co, generator=g) * 0.5).numpy().astype(np.float32)
            relu = (M + Co) % 2
            want, isum = _expected(a.numpy(), s, z, q.numpy(), ws, bias, relu)
            got, rc = _pw_call(a.to(dev), _state(dev, s, z), q, ws, bias, relu, W8)
            assert rc == 0
            assert np.array_equal(got, want), (M, C, Co, np.abs(got - want).max(), np.abs(isum).max())


def test_pointwise_large_m_small_co_takes_the_64x64_tiles():
    """M >= 65536 with Co <= 64: the 64 x 64 instantiation (stage 2, layer 1 and the heads at real batch sizes)."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(64)
    M, C, Co = 65537, 32, 20
    a = torch.rand(M, C, generator=g) * 7.0 - 0.6
    q = _codes8(Co, C, g)
    ws = (torch.rand(Co, generator=g) * 40 + 3).numpy().astype(np.float32)
    bias = (torch.randn(Co, generator=g) * 0.5).numpy().astype(np.float32)
    want, _ = _expected(a.numpy(), 41.0, 117.0, q.numpy(), ws, bias, 1)
    got, rc = _pw_call(a.to(dev), _state(dev, 41.0, 117.0), q, ws, bias, 1, W8)
    assert rc == 0 and np.array_equal(got, want), np.abs(got - want).max()


def test_pointwise_extremes_and_the_int32_bound():
    """(a) rows of 127s and of -128s against activations ON level 255 and level 0; (b) C = 4096 with levels over the
    whole range of the split, L - 128 in [-2040, 2039] (u = L - 128 + 2048 in [8, 4087]: codes wider than a byte; a batch
    beyond it sets state word 6): the case of the int32 bound, 2040 * 128 * 4096 plus 128 * colsum; (c) C above 4096 is
    refused with the flag."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    # (a) s = 1, z = 0: L = rint(a)
    M, C, Co = 33, 116, 20
    a = torch.where(torch.rand(M, C, generator=g) < 0.5, torch.tensor(255.0), torch.tensor(0.0))
    a[0], a[1] = 255.0, 0.0
    q = _codes8(Co, C, g)
    ws, bias = np.full(Co, 2.0, np.float32), np.zeros(Co, np.float32)
    want, isum = _expected(a.numpy(), 1.0, 0.0, q.numpy(), ws, bias, 0)
    assert isum[0, 0] == 255 * 127 * C and isum[0, 1] == -255 * 128 * C and isum[1, 0] == 0
    got, rc = _pw_call(a.to(dev), _state(dev, 1.0, 0.0), q, ws, bias, 0, W8)
    assert rc == 0 and np.array_equal(got, want)
    # (b) the bound: every level at 128 + 2039 / 128 - 2040 in rows 0 / 1, random wide levels elsewhere
    M, C, Co = 33, 4096, 20
    a = torch.randint(128 - 2040, 128 + 2040, (M, C), generator=g).float()
    a[0], a[1] = 128.0 + 2039.0, 128.0 - 2040.0
    q = _codes8(Co, C, g)
    ws, bias = np.full(Co, 64.0, np.float32), (torch.randn(Co, generator=g)).numpy().astype(np.float32)
    want, isum = _expected(a.numpy(), 1.0, 0.0, q.numpy(), ws, bias, 0)
    assert isum[0, 1] == -(128 + 2039) * 128 * C and abs(int(isum[0, 1])) > 2 ** 30       # 1 136 132 096
    assert isum[1, 1] == (2040 - 128) * 128 * C
    got, rc = _pw_call(a.to(dev), _state(dev, 1.0, 0.0), q, ws, bias, 0, W8)
    assert rc == 0 and np.array_equal(got, want), np.abs(got - want).max()
    # (c)
    a = torch.zeros(8, 4160)
    q = _codes8(4, 4160, g)
    _, rc = _pw_call(a.to(dev), _state(dev, 1.0, 0.0), q, np.ones(4, np.float32), np.zeros(4, np.float32), 0, W8)
    assert rc != 0


def test_pointwise_wide_code_batch_takes_the_f32_branch_at_eight_bits():
    """State word 6 set (codes too wide for the split): the batch runs on f32 MFMA with the fake-quantised weights, as
    for 4-bit codes.  An fp32 evaluation of the same sum: within K * 2^-24 * sum |terms| of the int64 value."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(6)
    M, C, Co = 33, 232, 80
    s, z = 3.0, 100.0
    a = torch.randn(M, C, generator=g) * 3000.0                     # levels to +-30 000
    q = _codes8(Co, C, g)
    ws = (torch.rand(Co, generator=g) * 40 + 3).numpy().astype(np.float32)
    bias = (torch.randn(Co, generator=g) * 0.5).numpy().astype(np.float32)
    L = _levels(a.numpy(), s, z)
    assert np.abs(L - 128).max() > 2040
    exact = (L @ q.numpy().astype(np.int64).T).astype(np.float64) / (np.float64(s) * ws.astype(np.float64)) + bias
    bound = C * 2.0 ** -24 * (np.abs(L) @ np.abs(q.numpy().astype(np.int64)).T) / (s * ws.astype(np.float64)) + 1e-3
    got, rc = _pw_call(a.to(dev), _state(dev, s, z, wide=1), q, ws, bias, 0, W8)
    assert rc == 0 and bool((np.abs(got - exact) <= bound).all()), (np.abs(got - exact) / bound).max()


def test_the_same_codes_without_the_flag_are_another_call():
    """Without CDN_W_CODES_8BIT the entry assumes |q| <= 8, as before the flag existed: 4-bit codes give the same output
    with and without the flag, bit for bit (and with the flag they equal the restatement); 8-bit codes are handed over
    WITH the flag only -- the call without it is made once here to show that it is accepted (its sums are undefined)."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(4)
    for (M, C, Co) in ((257, 232, 80), (33, 1024, 256), (257, 116, 58)):
        a = torch.rand(M, C, generator=g) * 7.0 - 0.6
        q4 = torch.randint(-8, 8, (Co, C), generator=g, dtype=torch.int32)
        ws = (torch.rand(Co, generator=g) * 4 + 1).numpy().astype(np.float32)
        bias = (torch.randn(Co, generator=g) * 0.5).numpy().astype(np.float32)
        st = _state(dev, 40.0, 120.0)
        want, _ = _expected(a.numpy(), 40.0, 120.0, q4.numpy(), ws, bias, 1)
        plain, rc0 = _pw_call(a.to(dev), st, q4, ws, bias, 1, 0)
        flagged, rc1 = _pw_call(a.to(dev), st, q4, ws, bias, 1, W8)
        assert rc0 == 0 and rc1 == 0
        assert np.array_equal(plain, want) and np.array_equal(flagged, want)
    q8 = _codes8(Co, C, g)
    want8, _ = _expected(a.numpy(), 40.0, 120.0, q8.numpy(), ws, bias, 1)
    flagged8, rc1 = _pw_call(a.to(dev), st, q8, ws, bias, 1, W8)
    unflagged8, rc0 = _pw_call(a.to(dev), st, q8, ws, bias, 1, 0)
    assert rc0 == 0 and rc1 == 0
    assert np.array_equal(flagged8, want8) and not np.array_equal(unflagged8, want8)      # why the flag exists


# ---- byte-code kernels (no flag: one product plane) -------------------------------------------------------------------

def test_byte_code_pointwise_on_eight_bit_codes():
    """pwq8_kernel, M = 65, C = 116, Co = 58: activation byte codes x 8-bit weight codes, fp32 output against the
    restatement (levels = code + zp), and no overflow flag."""
    from codenet_amd import _native as N_
    lib, dev = N_.lib(), torch.device("cuda", 0)
    g = torch.Generator().manual_seed(65)
    M, C, Co = 65, 116, 58
    s, z = 37.0, 121.0
    a8 = torch.randint(-128, 128, (M, C), generator=g, dtype=torch.int32)
    a8[0], a8[1] = 127, -128
    q = _codes8(Co, C, g)
    ws = (torch.rand(Co, generator=g) * 40 + 3).numpy().astype(np.float32)
    bias = (torch.randn(Co, generator=g) * 0.5).numpy().astype(np.float32)
    isum = (a8.numpy().astype(np.int64) + int(z)) @ q.numpy().astype(np.int64).T
    rinv = (np.float32(1.0) / (np.float32(s) * ws).astype(np.float32)).astype(np.float32)
    want = np.maximum(_fma32(isum.astype(np.int32).astype(np.float32), np.broadcast_to(rinv, isum.shape),
                             np.broadcast_to(bias, isum.shape)), np.float32(0))
    cp = torch.zeros(Co, 128, dtype=torch.int8)
    cp[:, :C] = q.to(torch.int8)
    ad = torch.zeros(M, 128, dtype=torch.int8)
    ad[:, :C] = a8.to(torch.int8)
    ad, cp = ad.to(dev), cp.to(dev)
    out = torch.full((M, Co), -7.5, device=dev)
    of = torch.zeros(1, dtype=torch.int32, device=dev)
    st, wsd, bd = _state(dev, s, z), torch.from_numpy(ws).to(dev), torch.from_numpy(bias).to(dev)
    colsum = q.sum(1).to(torch.int32).to(dev)
    rc = lib.cdn_codenet_pointwise_q8_strided_forward(
        ad.data_ptr(), st.data_ptr(), M, C, Co, 128, 0, cp.data_ptr(), wsd.data_ptr(), colsum.data_ptr(), bd.data_ptr(), 1,
        None, None, None, out.data_ptr(), of.data_ptr(), torch.cuda.current_stream().cuda_stream)
    N_.check(rc, "cdn_codenet_pointwise_q8_strided_forward")
    torch.cuda.synchronize()
    assert of.item() == 0 and np.array_equal(out.cpu().numpy(), want), np.abs(out.cpu().numpy() - want).max()


def test_fused_byte_code_depthwise_pointwise_on_eight_bit_codes():
    """dwpwq8_kernel at its smallest geometry (output 8 x 8): 8-bit pointwise codes, equal to the two separate launches
    (cdn_codenet_dw3x3_q8_forward + cdn_codenet_pointwise_q8_strided_forward), whose pointwise is the kernel of the test
    above."""
    from codenet_amd import _native as N_
    lib, dev = N_.lib(), torch.device("cuda", 0)
    g = torch.Generator().manual_seed(88)
    N, C, H, W, Co = 2, 116, 8, 8, 58
    assert lib.cdn_codenet_dwpw_q8_supported(C, H, W, 1, Co)
    ld = 128
    a8 = torch.zeros(N * H * W, ld, dtype=torch.int8)
    a8[:, :C] = torch.randint(-128, 128, (N * H * W, C), generator=g, dtype=torch.int32).to(torch.int8)
    a8 = a8.to(dev)
    w_dw = (torch.randn(C, 9, generator=g) * 0.3).to(dev)
    b_dw = (torch.randn(C, generator=g) * 0.1).to(dev)
    q = _codes8(Co, C, g)
    cp = torch.zeros(Co, 128, dtype=torch.int8)
    cp[:, :C] = q.to(torch.int8)
    cp = cp.to(dev)
    ws = (torch.rand(Co, generator=g) * 40 + 3).to(dev)
    bias = (torch.randn(Co, generator=g) * 0.5).to(dev)
    colsum = q.sum(1).to(torch.int32).to(dev)
    qa, qd, qr = _state(dev, 30.0, 125.0), _state(dev, 20.0, 128.0), _state(dev, 0.5, 3.0)
    st = torch.cuda.current_stream().cuda_stream
    of = torch.zeros(2, dtype=torch.int32, device=dev)
    fused = torch.zeros(N * H * W, Co, dtype=torch.int8, device=dev)
    N_.check(lib.cdn_codenet_dwpw_q8_forward(
        a8.data_ptr(), qa.data_ptr(), N, C, H, W, 1, ld, w_dw.data_ptr(), b_dw.data_ptr(), 0, qd.data_ptr(), Co,
        cp.data_ptr(), ws.data_ptr(), colsum.data_ptr(), bias.data_ptr(), 1, 0, None, qr.data_ptr(), fused.data_ptr(),
        of.data_ptr(), st), "cdn_codenet_dwpw_q8_forward")
    d8 = torch.zeros(N * H * W, ld, dtype=torch.int8, device=dev)
    N_.check(lib.cdn_codenet_dw3x3_q8_forward(a8.data_ptr(), qa.data_ptr(), N, C, H, W, 1, ld, ld, w_dw.data_ptr(),
                                              b_dw.data_ptr(), 0, qd.data_ptr(), d8.data_ptr(), of.data_ptr() + 4, st),
             "cdn_codenet_dw3x3_q8_forward")
    two = torch.zeros_like(fused)
    N_.check(lib.cdn_codenet_pointwise_q8_strided_forward(
        d8.data_ptr(), qd.data_ptr(), N * H * W, C, Co, ld, 0, cp.data_ptr(), ws.data_ptr(), colsum.data_ptr(),
        bias.data_ptr(), 1, None, qr.data_ptr(), two.data_ptr(), None, of.data_ptr() + 4, st),
        "cdn_codenet_pointwise_q8_strided_forward")
    torch.cuda.synchronize()
    assert torch.equal(fused, two) and fused.float().std().item() > 1.0


# ---- head tail --------------------------------------------------------------------------------------------------------

def _head_modules(C, classes, g, w_bit):
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
        q = qm.QuantDepthwiseNode(w_bit, 8, act_percentile=False, wt_quant_mode="symmetric",
                                  act_quant_mode="asymmetric", per_channel=True, weight_percentile=False)
        q.set_param(seq)
        heads[name] = q.eval()
    return heads


def test_eight_bit_heads_on_the_fused_tail_are_bit_identical_to_the_unfused_schedule():
    """FusedHeads(small_tail=True) against small_tail=False on 8-bit heads of 20 and 80 classes (matrix cores, one and
    three class groups) and 2 classes, Ws = 16, four forwards from fresh running ranges -- the acceptance of
    tests/test_gpu_heads_wide.py; the first 1x1 convs run as the one launch of all heads (pwi8h at 8 bits)."""
    from codenet_amd import pipeline
    planes = [64, 32, 16, 64]
    res, batch = 4, 2
    net = pipeline.build_hot_path(quantized=True, planes=planes, seed=5).cuda()
    g = torch.Generator().manual_seed(res)
    heads = _head_modules(64, {"hm20": 20, "hm80": 80, "wh": 2}, g, 8)
    assert all(h.quant_conv.int8_form()[0].abs().max().item() > 100 for h in heads.values())
    ha = {k: copy.deepcopy(v).cuda() for k, v in heads.items()}
    hb = {k: copy.deepcopy(v).cuda() for k, v in heads.items()}
    path = pipeline.FusedHotPath(net.deconv_layers)
    fa = pipeline.FusedHeads(ha, small_tail=True, fuse_first=True)
    fb = pipeline.FusedHeads(hb, small_tail=False)
    exact = 0
    for it in range(4):
        x = (torch.randn(batch, planes[0], res, res, generator=g).abs() * (1.0 + 0.2 * it)).cuda()
        r, rq, shape = path.forward_nhwc(x)
        assert shape["W"] == 16
        oa = {k: v.clone() for k, v in fa(r, rq, shape).items()}
        ob = fb(r, rq, shape)
        for k in oa:
            wide = hb[k].quant_act3[1]._device_state(x.device)[6].item() != 0
            if wide:       # f32-MFMA branch of the pointwise kernel on one side: fp32 rounding of the same sums
                assert (oa[k] - ob[k]).abs().max().item() < 1e-4 * (1 + ob[k].abs().max().item()), (k, it, "wide")
            else:
                assert torch.equal(oa[k], ob[k]), (k, it, (oa[k] - ob[k]).abs().max().item())
                exact += 1
    assert exact >= 3 * len(ha) - 3, exact
    for k in ha:
        for aa, bb in ((ha[k].quant_act1[1], hb[k].quant_act1[1]), (ha[k].quant_act3[1], hb[k].quant_act3[1])):
            assert torch.equal(aa.x_min, bb.x_min) and torch.equal(aa.x_max, bb.x_max), k
    assert not fa._bufs["y2"] and set(fb._bufs["y2"]) == set(ha)
    assert fa._bufs.get("y1_all") is not None          # the heads' first convs ran as one launch


@pytest.mark.parametrize("classes", [2, 20, 80])
def test_eight_bit_tail_on_byte_codes_equals_the_fp32_form(classes):
    """cdn_codenet_head_tail_small_q8_w_forward against cdn_codenet_head_tail_small_w_forward (w_bits = 8) on the tensor
    that produced the codes, and the fp32 form against the restatement of its matrix phase through the unfused pair
    (depthwise launch + flagged pointwise): identical outputs; w_bits = 4 on 4-bit codes equals the entry without the
    argument; other widths are refused."""
    from codenet_amd import _native as N_, ops
    lib, dev = N_.lib(), torch.device("cuda", 0)
    g = torch.Generator().manual_seed(classes)
    N, Hs, Ws = 2, 8, 16
    y1 = (torch.rand(N, Hs * Ws, 64, generator=g) * 4.0).to(dev)
    q1, q2 = _state(dev, 255.0 / 4.2, 125.0), _state(dev, 11.0, 128.0)
    y8 = torch.round(q1.view(torch.float32)[2] * y1 - q1.view(torch.float32)[3])
    assert y8.min().item() >= -128 and y8.max().item() <= 127
    y8 = y8.to(torch.int8).contiguous()
    w_dw, b_dw = (torch.randn(64, 9, generator=g) * 0.3).to(dev), (torch.randn(64, generator=g) * 0.1).to(dev)
    st = torch.cuda.current_stream().cuda_stream

    def run(q, w_bits, q8, sibling=True):
        codes, scale = q.to(torch.int8).to(dev), (torch.rand(classes, generator=torch.Generator().manual_seed(7)) * 10 + 3).to(dev)
        colsum = q.sum(1).to(torch.int32).to(dev)
        bias = (torch.randn(classes, generator=torch.Generator().manual_seed(8)) * 0.1).to(dev)
        out = torch.zeros(N, classes, 2 * Hs, 2 * Ws, device=dev)
        of = torch.zeros(1, dtype=torch.int32, device=dev)
        args = [q1.data_ptr(), N, 64, Hs, Ws, w_dw.data_ptr(), b_dw.data_ptr(), q2.data_ptr(), codes.data_ptr(),
                scale.data_ptr(), colsum.data_ptr(), bias.data_ptr(), classes, out.data_ptr()]
        if q8:
            rc = (lib.cdn_codenet_head_tail_small_q8_w_forward(y8.data_ptr(), *args, of.data_ptr(), w_bits, st) if sibling
                  else lib.cdn_codenet_head_tail_small_q8_forward(y8.data_ptr(), *args, of.data_ptr(), st))
        else:
            rc = (lib.cdn_codenet_head_tail_small_w_forward(y1.data_ptr(), *args, w_bits, st) if sibling
                  else lib.cdn_codenet_head_tail_small_forward(y1.data_ptr(), *args, st))
        torch.cuda.synchronize()
        return rc, out, of.item(), (codes, scale, colsum, bias)

    q = _codes8(classes, 64, g)
    rc, a, _, (codes, scale, colsum, bias) = run(q, 8, False)
    assert rc == 0
    rc, b, of, _ = run(q, 8, True)
    assert rc == 0 and of == 0 and torch.equal(a, b) and a.abs().max().item() > 0
    # the unfused pair: depthwise on the up-sampled fq(y1) -> y2 (fp32), then the flagged int8 pointwise, NHWC -> NCHW
    aux = lib.cdn_codenet_aux_workspace_bytes()
    wsb = torch.zeros(aux // 4 + 64, device=dev)
    wp, wb = N_.aligned_workspace(wsb)
    M4 = N * 4 * Hs * Ws
    y2 = torch.empty(M4, 64, device=dev)
    N_.check(lib.cdn_codenet_dw3x3_nhwc_forward(y1.data_ptr(), q1.data_ptr(), N, 64, Hs, Ws, 1, 1, 0, 0, w_dw.data_ptr(),
                                                b_dw.data_ptr(), None, None, 1, None, None, None, 8, 0.99, 0, wp, wb,
                                                y2.data_ptr(), st), "cdn_codenet_dw3x3_nhwc_forward")
    o = torch.empty(M4, classes, device=dev)
    wf = (q.float().to(dev) / scale.view(-1, 1)).contiguous()
    N_.check(lib.cdn_codenet_pointwise_nhwc_forward(
        y2.data_ptr(), q2.data_ptr(), M4, 64, classes, 0, 0, wf.data_ptr(), codes.data_ptr(), scale.data_ptr(),
        colsum.data_ptr(), bias.data_ptr(), None, None, 0 | W8, None, None, None, 8, 0.99, 0, None, 0, o.data_ptr(), st),
        "cdn_codenet_pointwise_nhwc_forward")
    torch.cuda.synchronize()
    want = o.view(N, 2 * Hs, 2 * Ws, classes).permute(0, 3, 1, 2)
    assert torch.equal(a, want), (a - want).abs().max().item()
    # 4-bit codes: w_bits = 4 is the entry without the argument; w_bits = 8 gives the same values
    q4 = torch.randint(-8, 8, (classes, 64), generator=g, dtype=torch.int32)
    for q8 in (False, True):
        _, old, _, _ = run(q4, 4, q8, sibling=False)
        _, new4, _, _ = run(q4, 4, q8)
        _, new8, _, _ = run(q4, 8, q8)
        assert torch.equal(old, new4) and torch.equal(old, new8)
    rc, _, _, _ = run(q4, 6, False)
    assert rc != 0


# ---- stage and network, random inputs ---------------------------------------------------------------------------------

def _w8_hot_path(planes, seed):
    from codenet_amd import pipeline
    from codenet_amd.pipeline.common import quantize_deform_stages
    net = pipeline.build_hot_path(quantized=False, planes=planes, seed=seed)
    quantize_deform_stages(net, 8, 8, "symmetric", "asymmetric", True, False, False)
    return net.eval()


@pytest.mark.parametrize("C,kblocked", [(256, True), (1024, True), (1024, False)])
def test_one_w8a8_stage_fused_against_the_module_path(C, kblocked):
    """(N, C, Co, H, W) = (2, 256, 128, 16, 16), and the long-K shape C = 1024 with and without the k-blocked codes asked
    for (8-bit codes take the tiled kernel either way; the two outputs are compared with each other in
    test_long_k_stage_is_the_same_with_and_without_the_kblocked_request): the acceptance of
    test_cfg3_modules_w4a8_batch64_matches_fused -- no element off by more than one LSB, fewer than 0.2 % off at all."""
    from codenet_amd import pipeline
    net = _w8_hot_path([C, 128], seed=37)
    a, b = copy.deepcopy(net).cuda(), copy.deepcopy(net).cuda()
    fused = pipeline.FusedHotPath(b.deconv_layers, kblocked_codes=kblocked)
    p = fused._stage_params(fused.stages[0])
    assert p["i8"] is not None and p["kb_flag"] == W8 and p["i8"][0].abs().max().item() > 100
    g = torch.Generator().manual_seed(137)
    for it in range(2):
        x = (torch.randn(2, C, 16, 16, generator=g).abs() * (1.66 * (1.0 + 0.15 * it))).cuda()
        with torch.no_grad():
            ya = a(x)
        yb = fused(x)
        last = list(b.deconv_layers)[-2][1]
        lsb = (last.x_max - last.x_min).item() / 255.0
        diff = (ya - yb).abs()
        share = (diff > 1e-3).float().mean().item()
        print("W8A8 stage C=%d fwd %d: max |diff| %.3g (LSB %.3g), share off %.3g" % (C, it, diff.max().item(), lsb, share))
        assert diff.max().item() <= 1.05 * lsb + 1e-3
        assert share < 2e-3


def _ranges_agree_in_lsb(ma, mb):
    from codenet_amd.portable_quantizer.quant_modules import QuantAct
    worst = 0.0
    for (na, a), (nb, b) in zip(ma.named_modules(), mb.named_modules()):
        if isinstance(a, QuantAct):
            lsb = max((a.x_max - a.x_min).item(), 1e-6) / 255.0
            worst = max(worst, (a.x_min - b.x_min).abs().item() / lsb, (a.x_max - b.x_max).abs().item() / lsb)
    return worst


def test_w8a8_network_fused_plan_and_agreement_with_the_module_path():
    """create_model(quantize=True, w_bit=8) at 2 x 3 x 128 x 128: enable_fused() plans ("fused", False, False) -- on the
    parent every 1x1 conv left the int8 matrix cores -- and agrees with the module path as
    test_other_reference_configs_fused_match_module_path accepts its W4A8 twins (median over three inputs of mean / max
    |d| over the output's std below 0.12 / 2.5, no input above 0.5 in the mean; QuantAct ranges within 20 LSB)."""
    from codenet_amd import harness
    for heads in (None, {"hm": 80, "wh": 2, "reg": 2}):
        model = harness.create_model(heads=heads, quantize=True, w_bit=8).cuda()
        m2 = copy.deepcopy(model).enable_fused()
        stats = {}
        seeds = (2, 12, 22) if heads is None else (2,)
        for seed in seeds:
            ma, mb = (model, m2) if seed == seeds[-1] else (copy.deepcopy(model), copy.deepcopy(m2))
            x = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(seed)).cuda()
            assert mb._plan(x) == ("fused", False, False)
            with torch.no_grad():
                a = ma(x)[-1]
                b = mb(x)[-1]
            for k in a:
                std = a[k].std().item() + 1e-6
                diff = (a[k] - b[k]).abs()
                stats.setdefault(k, []).append((diff.mean().item() / std, diff.max().item() / std))
        for k, v in stats.items():
            means, maxes = sorted(m for m, _ in v), sorted(m for _, m in v)
            print("   W8A8 %s: mean |d| / std %s, max |d| / std %s" % (k, ["%.3f" % m for m in means], ["%.3f" % m for m in maxes]))
            assert means[len(means) // 2] < 0.12 and maxes[len(maxes) // 2] < 2.5, (k, v)
            assert means[-1] < 0.5, (k, v)
        worst = _ranges_agree_in_lsb(model, m2)
        print("   W8A8 worst QuantAct bound difference: %.2f LSB" % worst)
        assert worst < 20.0
        # every int8 layer of the schedule announces its width
        assert m2._fpath._stage_params(m2._fpath.stages[0])["kb_flag"] == W8


# ---- serving ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("heads", [None, {"hm": 80, "wh": 2, "reg": 2}])
def test_w8a8_model_serves_on_byte_codes(heads):
    """After calibrate_serving (through prepare_serving) enable_fused(frozen_codes=True) on the w_bit=8 model plans
    ("bytes", True, True) (NotImplementedError on the parent) and serves the calibration batch without overflow; a batch
    far outside the ranges raises the overflow flag."""
    from codenet_amd import harness, pipeline
    model = harness.create_model(heads=heads, quantize=True, w_bit=8).cuda()
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
    assert other._plan(images) == ("bytes", True, False)        # heads unfused, on the expanded codes
    with torch.no_grad():
        out = {k: v.clone() for k, v in model(images)[-1].items()}
        ref = other(images)[-1]
    assert not model.frozen_overflowed() and not other.frozen_overflowed()
    for k in out:
        assert torch.isfinite(out[k]).all() and torch.equal(out[k], ref[k]), (k, (out[k] - ref[k]).abs().max().item())
    big = images * 50.0
    with torch.no_grad():
        model(big)
    assert model.frozen_overflowed()


@pytest.mark.parametrize("planes,res,n", [([64, 32, 16, 8], 8, 3), ([1024, 256, 128, 64], 16, 4)])
def test_w8a8_byte_code_stages_are_bit_identical_to_the_fp32_frozen_schedule(planes, res, n):
    """FrozenHotPath on an 8-bit stage chain against FusedHotPath with running_stat False (the acceptance of
    test_frozen_codes_bit_identical_to_fp32_frozen_schedule): outputs torch.equal, the byte codes are the codes of the
    fp32 schedule's pre-quantisation output, eager and replayed; a batch outside the ranges raises the overflow flag."""
    from codenet_amd import pipeline
    from codenet_amd.portable_quantizer.quant_modules import QuantAct
    net = _w8_hot_path(planes, seed=41).cuda()
    g = torch.Generator().manual_seed(141)
    xs = [torch.randn(n, planes[0], res, res, generator=g).abs_() * (1.66 * (1.0 - 0.04 * i)) for i in range(3)]
    pipeline.set_running_stat(net, True)
    warm = pipeline.FusedHotPath(net.deconv_layers)
    for _ in range(2):
        for x in xs:
            warm(x.cuda())
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, QuantAct):
                w = (m.x_max - m.x_min) * 0.5
                m.x_min.sub_(w)
                m.x_max.add_(w)
    pipeline.set_running_stat(net, False)
    ref = pipeline.FusedHotPath(net.deconv_layers)
    frz = pipeline.FrozenHotPath(net.deconv_layers)
    for x in xs:
        xg = x.cuda()
        a = ref(xg).clone()
        b = frz(xg).clone()
        assert not frz.overflowed()
        assert torch.equal(a, b)
        r, rq, shape = ref.forward_nhwc(xg)
        r8, rq8, shape8 = frz.forward_codes(xg)
        assert rq == rq8 and r8.dtype == torch.int8 and tuple(r8.shape) == tuple(r.shape)
        st = list(net.deconv_layers)[-2][1]._device_state(xg.device).view(torch.float32)
        assert torch.equal(r8.float(), torch.round(st[2] * r - st[3]))
    xbuf = xs[0].cuda()
    replay = frz.capture(xbuf)
    for x in xs:
        xbuf.copy_(x.cuda())
        got = replay().clone()
        assert torch.equal(got, frz.forward_codes(xbuf)[0])
    frz(xs[0].cuda() * 4.0)
    assert frz.overflowed()


# ---- a 4-bit model is what it was ---------------------------------------------------------------------------------------

def test_four_bit_stage_is_bit_identical_with_and_without_the_flag():
    """A W4A8 stage chain (cfg3 shapes at batch 4): the planned flags carry no width bit, and forcing
    CDN_W_CODES_8BIT onto the same 4-bit codes (the 8-bit kernels: second accumulator, tiled long-K form) leaves every
    output and every QuantAct range bit-identical over two forwards from fresh running ranges."""
    from codenet_amd import pipeline
    net = pipeline.build_hot_path(quantized=True, planes=[1024, 256, 128, 64], seed=11)
    a, b = copy.deepcopy(net).cuda(), copy.deepcopy(net).cuda()
    fa, fb = pipeline.FusedHotPath(a.deconv_layers), pipeline.FusedHotPath(b.deconv_layers)
    flags = [fa._stage_params(st)["kb_flag"] for st in fa.stages]
    assert flags == [pipeline.WCODES_KB, 0, 0]
    orig = fb._stage_params

    def forced(st):
        p = dict(orig(st))
        p["kb_flag"] |= W8
        return p
    fb._stage_params = forced
    g = torch.Generator().manual_seed(12)
    for it in range(2):
        x = (torch.randn(4, 1024, 16, 16, generator=g).abs() * 1.66).cuda()
        ya, yb = fa(x).clone(), fb(x)
        assert torch.equal(ya, yb), (it, (ya - yb).abs().max().item())
    from codenet_amd.portable_quantizer.quant_modules import QuantAct
    for (_, ma), (_, mb) in zip(a.named_modules(), b.named_modules()):
        if isinstance(ma, QuantAct):
            assert torch.equal(ma.x_min, mb.x_min) and torch.equal(ma.x_max, mb.x_max)


def test_four_bit_exact_codes_case_and_network_plan_are_what_they_were():
    """The exact-arithmetic three-stage case of tests/test_gpu_exact_codes.py (cfg3 shapes, frozen dyadic ranges): the
    output equals the CPU oracle with the width flag absent (the planned call) and with the 8-bit kernels forced onto
    the 4-bit codes.  A W4A8 network plans the schedule it planned before, and none of its stages carries the flag."""
    from codenet_amd import harness, pipeline
    from oracle import dcn as O
    from tests.test_gpu_exact_codes import CFG3, _exact_chain, _oracle_chain
    net, x = _exact_chain(CFG3, 4, seed=23)
    O.lib()
    want, _ = _oracle_chain(copy.deepcopy(net), x)
    net = net.cuda()
    plain = pipeline.FusedHotPath(net.deconv_layers)
    assert [plain._stage_params(st)["kb_flag"] for st in plain.stages] == [pipeline.WCODES_KB, 0, 0]
    assert torch.equal(plain(x.cuda()).cpu(), want)
    forcedp = pipeline.FusedHotPath(net.deconv_layers)
    orig = forcedp._stage_params
    forcedp._stage_params = lambda st: dict(orig(st), kb_flag=orig(st)["kb_flag"] | W8)
    assert torch.equal(forcedp(x.cuda()).cpu(), want)
    model = harness.create_model(quantize=True).cuda().enable_fused()
    img = torch.randn(2, 3, 128, 128, generator=torch.Generator().manual_seed(2)).cuda()
    assert model._plan(img) == ("fused", False, False)
    assert [model._fpath._stage_params(st)["kb_flag"] & W8 for st in model._fpath.stages] == [0, 0, 0]
    for h in model.heads:
        node = getattr(model, h)
        assert node.quant_conv.int8_width() == 4 and node.quant_convbn1.int8_width_flag() == 0


# ---- whole stage chain on exact-arithmetic inputs -------------------------------------------------------------------------

EXACT_PLANES = [64, 32, 16, 8]      # C <= 64 everywhere: 255 * 127 * 64 < 2^24


def _exact_net8(planes, seed):
    """The construction of tests/test_gpu_exact_codes.py::_exact_net with 7 -> 127: every weight row has magnitude
    127 * 2^-k, so the per-channel 8-bit scales 127 / mag are powers of two and the fake-quantised weights dyadic; exact
    BN folds (gamma = 1, var + eps == 1, mean = 0, dyadic beta)."""
    from codenet_amd import pipeline
    from codenet_amd.pipeline.common import quantize_deform_stages
    net = pipeline.build_hot_path(quantized=False, planes=planes, seed=seed)
    quantize_deform_stages(net, 8, 8, "symmetric", "asymmetric", True, False, False)
    net = net.eval()
    g = torch.Generator().manual_seed(seed)
    stages = [m for m in net.deconv_layers if hasattr(m, "quant_deform_conv")]
    with torch.no_grad():
        for k, q in enumerate(stages):
            C = q.quant_deform_conv.in_channels
            Co = q.quant_conv_channel_bn.conv.out_channels
            ks = (8, 10, 11)[k]
            ws = torch.zeros(1, C, 1, 1)
            ws[0, :8, 0, 0] = torch.tensor([127., -127., 5., -5., 3., -3., 1., -1.]) * 2.0 ** -ks
            q.quant_conv_scale.weight.copy_(ws)
            q.quant_conv_scale.bias.fill_(1.0)
            wd = torch.randint(-127, 128, (C, 1, 3, 3), generator=g).float()
            flat = wd.view(C, -1)
            flat[torch.arange(C), torch.randint(0, 9, (C,), generator=g)] = \
                127.0 * (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1)
            q.quant_deform_conv.weight.copy_(wd * 2.0 ** -8)
            # pointwise 1x1: DENSE rows of 8-bit codes over the channels >= 10 (one of them +-127), * 2^-7
            wp = torch.zeros(Co, C, 1, 1)
            wp[:, 10:, 0, 0] = torch.randint(-127, 128, (Co, C - 10), generator=g).float()
            wp[torch.arange(Co), 10 + torch.randint(0, C - 10, (Co,), generator=g), 0, 0] = \
                127.0 * (torch.randint(0, 2, (Co,), generator=g).float() * 2 - 1)
            q.quant_conv_channel_bn.conv.weight.copy_(wp * 2.0 ** -7)
            bn = q.quant_conv_channel_bn.bn
            bn.weight.fill_(1.0)
            bn.running_mean.zero_()
            var = torch.tensor(1.0 - bn.eps, dtype=torch.float32)
            if (var + bn.eps).item() != 1.0:
                var = torch.nextafter(var, torch.tensor(2.0))
            assert (var + bn.eps).item() == 1.0 and torch.sqrt(var + bn.eps).item() == 1.0
            bn.running_var.fill_(var.item())
            bn.bias.copy_(torch.randint(-8, 9, (Co,), generator=g).float() / 8.0)
    return net


def _oracle_stage8(cur, w, mirrors):
    """One stage through the CPU oracle at 8 weight bits, frozen ranges; asserts the 24-bit bound of the pointwise
    sum on the way (sum of |level * code| in units of the product grid)."""
    import torch.nn.functional as F
    from oracle import quant as Q
    r = Q.stage_w4a8(cur, w["w_scale"], w["b_scale"], w["w_dw"], w["w_pw"], w["bn"], mirrors[0], mirrors[1], w_bits=8,
                     running=False, lo=w["lo"], hi=w["hi"])
    s_raw = torch.clamp(F.conv2d(cur, Q.weight_fake_quant(w["w_scale"], 8), w["b_scale"]), w["lo"], w["hi"])
    wf, _ = Q.fold_bn(w["w_pw"], None, *w["bn"])
    _, codes, _ = Q.weight_fake_quant(wf, 8, return_codes=True)
    levels = r["d_codes"].double().abs() + abs(float(Q.act_params(mirrors[1].x_min, mirrors[1].x_max)[1]))
    worst = F.conv2d(levels, codes.double().abs().view(codes.shape[0], -1, 1, 1)).max().item()
    assert worst < 2 ** 24 and codes.abs().max().item() == 127, worst
    for c in (r["s_codes"], r["d_codes"]):      # (the byte-code schedule stores them)
        assert c.min().item() >= -128 and c.max().item() <= 127
    rr = torch.relu(r["y"])
    r_q, r_codes = mirrors[2](rr, False, return_codes=True)
    return dict(s=s_raw, d=r["d"], r=rr, r_q=r_q, r_codes=r_codes)


def _exact_chain8(n, seed):
    from codenet_amd import pipeline
    from tests.test_gpu_exact_codes import _set_range
    net = _exact_net8(EXACT_PLANES, seed)
    stages = [m for m in net.deconv_layers if hasattr(m, "quant_deform_conv")]
    posts = [m for m in net.deconv_layers if isinstance(m, torch.nn.Sequential)]
    for q, post, (rs, rd, rr) in zip(stages, posts, EXACT_RANGES):
        _set_range(q.quant_act[1], *rs)
        _set_range(q.quant_identity_deform, *rd)
        _set_range(post[1], *rr)
    pipeline.set_running_stat(net, False)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randint(0, 4, (n, EXACT_PLANES[0], 16, 16), generator=g).float()
    return net, x


def _oracle_chain8(cpu, x):
    import torch.nn.functional as F
    from oracle import quant as Q
    from tests.test_gpu_exact_codes import _is_pow2, _mirror_like, _stage_weights
    stages = [m for m in cpu.deconv_layers if hasattr(m, "quant_deform_conv")]
    posts = [m for m in cpu.deconv_layers if isinstance(m, torch.nn.Sequential)]
    cur, recs = x, []
    for q, post in zip(stages, posts):
        mirrors = [_mirror_like(q.quant_act[1]), _mirror_like(q.quant_identity_deform), _mirror_like(post[1])]
        assert all(_is_pow2(Q.act_params(m.x_min, m.x_max)[0].item()) for m in mirrors)
        rec = _oracle_stage8(cur, _stage_weights(q), mirrors)
        recs.append(rec)
        cur = F.interpolate(rec["r_q"], scale_factor=2, mode="nearest")
    return cur, recs


#                 s range               d range                r range
EXACT_RANGES = [((-3.0, 4.96875),     (-15.9375, 15.9375),   (0.0, 63.75)),         # scales 32, 8, 4
                ((-31.875, 31.875),   (-127.5, 127.5),       (0.0, 127.5)),         # scales 4, 1, 2
                ((-31.875, 31.875),   (-255.0, 255.0),       (0.0, 255.0))]         # scales 4, 1/2, 1


@pytest.mark.parametrize("n", [4, 33])
def test_exact_arithmetic_w8a8_three_stage_chain_frozen_ranges(n):
    """Three W8A8 stages (64 -> 32 -> 16 -> 8 channels at 16^2 / 32^2 / 64^2) on inputs where every summation order gives
    the same fp32 value: integer x, weight rows of magnitude 127 * 2^-k (power-of-two 8-bit scales), frozen dyadic
    QuantAct ranges, dense 8-bit pointwise rows with sum |level * code| < 2^24 (asserted on the CPU first).  The fused
    schedule eager and as a replayed graph -- s, d, relu(y) of every stage and the output torch.equal to the CPU
    oracle of the module path -- and the byte-code serving schedule: its output codes equal the oracle's, eager and
    replayed, no overflow.  (Running ranges are not covered: the planted extremes of the 4-bit construction do not
    carry over to 127-magnitude rows, and an EMA step from non-planted extremes leaves the dyadic grid.)"""
    from codenet_amd import pipeline
    from oracle import dcn as O
    from tests.test_gpu_exact_codes import _Tap
    net, x = _exact_chain8(n, seed=23)
    O.lib()
    want, recs = _oracle_chain8(copy.deepcopy(net), x)
    assert all(r["r_codes"].min().item() >= -128 and r["r_codes"].max().item() <= 127 for r in recs)
    assert all(r["r_codes"].unique().numel() > 64 for r in recs)
    net = net.cuda()
    xg = x.cuda()
    fused = pipeline.FusedHotPath(net.deconv_layers)
    assert all(fused._stage_params(st)["kb_flag"] == W8 for st in fused.stages)
    tap = _Tap(fused, n)
    out = fused(xg).cpu()
    for k, (rec, ref) in enumerate(zip(tap.records, recs)):
        s_ref = ref["s"] if not rec["up"] else ref["s"][:, :, ::2, ::2]
        assert torch.equal(rec["s"], s_ref), "stage %d: s" % k
        assert torch.equal(rec["d"], ref["d"]), "stage %d: d (%g)" % (k, (rec["d"] - ref["d"]).abs().max().item())
        assert torch.equal(rec["r"], ref["r"]), "stage %d: relu(y) (%g)" % (k, (rec["r"] - ref["r"]).abs().max().item())
    assert torch.equal(out, want), "fused schedule, frozen ranges: output"
    fused.stage_hook = None
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out_g = fused(xg)
    for _ in range(2):
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_g.cpu(), want), "graph replay: output"
    frz = pipeline.FrozenHotPath(net.deconv_layers)
    codes = frz.forward_codes(xg)[0]
    Co, H = EXACT_PLANES[-1], 64
    got = codes.view(n, H, H, -1)[..., :Co].permute(0, 3, 1, 2).cpu().float()
    assert not frz.overflowed()
    assert torch.equal(got, recs[-1]["r_codes"]), "byte-code schedule: output codes"
    step = frz.capture(xg)
    got_g = step().view(n, H, H, -1)[..., :Co].permute(0, 3, 1, 2).cpu().float()
    assert torch.equal(got_g, recs[-1]["r_codes"]), "byte-code schedule, graph replay"


# ---- every tile of the launcher, and the stage entry, against the restatement ---------------------------------------------

@pytest.mark.parametrize("M,C,Co,tile", [(257, 256, 80, 64128), (257, 512, 256, 64128), (33, 232, 80, 32128),
                                         (257, 1024, 256, 32128), (257, 116, 58, 128064), (65537, 32, 20, 64064)])
def test_every_tile_of_the_eight_bit_pointwise_is_exact_and_named(M, C, Co, tile):
    """The four tiles the launcher can pick for 8-bit codes, each named by the launcher's own query
    (cdn_codenet_pointwise_i8_tile) and compared with the int64 restatement: 64 x 128 (stage 1: the second accumulator
    set of two column tiles, 160 registers) at K = 256 and 512, 32 x 128 at K < 256 and at long K with few tiles,
    128 x 64 and 64 x 64 for Co <= 64."""
    from codenet_amd import _native as N_
    assert N_.lib().cdn_codenet_pointwise_i8_tile(M, C, Co) == tile
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(M + C + Co)
    a = torch.rand(M, C, generator=g) * 7.0 - 0.6
    q = _codes8(Co, C, g)
    ws = (torch.rand(Co, generator=g) * 40 + 3).numpy().astype(np.float32)
    bias = (torch.randn(Co, generator=g) * 0.5).numpy().astype(np.float32)
    want, _ = _expected(a.numpy(), 39.0, 119.0, q.numpy(), ws, bias, 1)
    got, rc = _pw_call(a.to(dev), _state(dev, 39.0, 119.0), q, ws, bias, 1, W8)
    assert rc == 0 and np.array_equal(got, want), np.abs(got - want).max()


@pytest.mark.parametrize("C,Co,kblocked", [(256, 128, True), (1024, 256, True), (1024, 256, False)])
def test_stage_entry_pointwise_equals_the_restatement_of_its_own_d(C, Co, kblocked):
    """cdn_codenet_stage_fused_forward on a W8A8 stage: the pointwise output relu(y) the call leaves against the
    restatement fed with the call's OWN gather output d and the d quantiser's state (scale, zero point) -- torch.equal;
    stage 1's shape (64 x 128 tiles) and the long-K shape with and without the k-blocked codes asked for, whose outputs
    are also compared with each other by the caller below."""
    from codenet_amd import pipeline
    from tests.test_gpu_exact_codes import _Tap
    net = _w8_hot_path([C, Co], seed=37).cuda()
    fused = pipeline.FusedHotPath(net.deconv_layers, kblocked_codes=kblocked)
    n = 2
    tap = _Tap(fused, n)
    x = (torch.randn(n, C, 16, 16, generator=torch.Generator().manual_seed(5)).abs() * 1.66).cuda()
    fused(x)
    rec = tap.records[0]
    q = fused.stages[0][0]
    st = q.quant_identity_deform._device_state(x.device)
    assert st.view(torch.int32)[6].item() == 0
    s, z = st.view(torch.float32)[2].item(), st.view(torch.float32)[3].item()
    codes, scale, _ = q.quant_conv_channel_bn.folded_int8()
    _, b = q.quant_conv_channel_bn.folded()
    d = rec["d"].permute(0, 2, 3, 1).reshape(-1, C).numpy()
    want, _ = _expected(d, s, z, codes[:, :C].cpu().to(torch.int32).numpy(), scale.cpu().numpy(), b.detach().cpu().numpy(), 1)
    got = rec["r"].permute(0, 2, 3, 1).reshape(-1, Co).numpy()
    assert np.array_equal(got, want), np.abs(got - want).max()


def test_long_k_stage_is_the_same_with_and_without_the_kblocked_request():
    from codenet_amd import pipeline
    net = _w8_hot_path([1024, 256], seed=37).cuda()
    pipeline.set_running_stat(net, False)
    x = (torch.randn(2, 1024, 16, 16, generator=torch.Generator().manual_seed(5)).abs() * 1.66).cuda()
    warm = pipeline.FusedHotPath(net.deconv_layers)
    pipeline.set_running_stat(net, True)
    warm(x)
    pipeline.set_running_stat(net, False)
    a = pipeline.FusedHotPath(net.deconv_layers, kblocked_codes=True)(x).clone()
    b = pipeline.FusedHotPath(net.deconv_layers, kblocked_codes=False)(x).clone()
    assert torch.equal(a, b) and a.abs().max().item() > 0


# ---- head tail off the matrix path (VALU form, MODE 1) ----------------------------------------------------------------------

@pytest.mark.parametrize("classes", [2, 4])
def test_eight_bit_tail_on_the_valu_form_equals_the_unfused_pair(classes):
    """Ws = 24 (not a multiple of 16): the tail takes the VALU form (fp32 sums of integer products, exact while
    sum |L q| < 2^24 -- asserted) for 2 and 4 classes, fp32 and byte-code input, on a batch whose codes fit the split
    (state word 6 clear): equal to the depthwise launch + flagged int8 pointwise."""
    from codenet_amd import _native as N_
    lib, dev = N_.lib(), torch.device("cuda", 0)
    g = torch.Generator().manual_seed(24 + classes)
    N, Hs, Ws = 2, 8, 24
    y1 = (torch.rand(N, Hs * Ws, 64, generator=g) * 4.0).to(dev)
    q1, q2 = _state(dev, 255.0 / 4.2, 125.0), _state(dev, 11.0, 128.0)
    y8 = torch.round(q1.view(torch.float32)[2] * y1 - q1.view(torch.float32)[3])
    assert y8.min().item() >= -128 and y8.max().item() <= 127
    y8 = y8.to(torch.int8).contiguous()
    w_dw, b_dw = (torch.randn(64, 9, generator=g) * 0.3).to(dev), (torch.randn(64, generator=g) * 0.1).to(dev)
    q = _codes8(classes, 64, g)
    codes, scale = q.to(torch.int8).to(dev), (torch.rand(classes, generator=g) * 10 + 3).to(dev)
    colsum, bias = q.sum(1).to(torch.int32).to(dev), (torch.randn(classes, generator=g) * 0.1).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    args = [q1.data_ptr(), N, 64, Hs, Ws, w_dw.data_ptr(), b_dw.data_ptr(), q2.data_ptr(), codes.data_ptr(),
            scale.data_ptr(), colsum.data_ptr(), bias.data_ptr(), classes]
    a, b = (torch.zeros(N, classes, 2 * Hs, 2 * Ws, device=dev) for _ in range(2))
    of = torch.zeros(1, dtype=torch.int32, device=dev)
    N_.check(lib.cdn_codenet_head_tail_small_w_forward(y1.data_ptr(), *args, a.data_ptr(), 8, st), "fp32 tail")
    N_.check(lib.cdn_codenet_head_tail_small_q8_w_forward(y8.data_ptr(), *args, b.data_ptr(), of.data_ptr(), 8, st), "q8 tail")
    wsb = torch.zeros(lib.cdn_codenet_aux_workspace_bytes() // 4 + 64, device=dev)
    wp, wb = N_.aligned_workspace(wsb)
    M4 = N * 4 * Hs * Ws
    y2 = torch.empty(M4, 64, device=dev)
    N_.check(lib.cdn_codenet_dw3x3_nhwc_forward(y1.data_ptr(), q1.data_ptr(), N, 64, Hs, Ws, 1, 1, 0, 0, w_dw.data_ptr(),
                                                b_dw.data_ptr(), None, None, 1, None, None, None, 8, 0.99, 0, wp, wb,
                                                y2.data_ptr(), st), "cdn_codenet_dw3x3_nhwc_forward")
    o = torch.empty(M4, classes, device=dev)
    wf = (q.float().to(dev) / scale.view(-1, 1)).contiguous()
    N_.check(lib.cdn_codenet_pointwise_nhwc_forward(
        y2.data_ptr(), q2.data_ptr(), M4, 64, classes, 0, 0, wf.data_ptr(), codes.data_ptr(), scale.data_ptr(),
        colsum.data_ptr(), bias.data_ptr(), None, None, 0 | W8, None, None, None, 8, 0.99, 0, None, 0, o.data_ptr(), st),
        "cdn_codenet_pointwise_nhwc_forward")
    torch.cuda.synchronize()
    L = _levels(y2.cpu().numpy(), 11.0, 128.0)
    assert np.abs(L - 128).max() <= 2039 and (np.abs(L) @ np.abs(q.numpy().astype(np.int64)).T).max() < 2 ** 24
    want = o.view(N, 2 * Hs, 2 * Ws, classes).permute(0, 3, 1, 2)
    assert torch.equal(a, want), (a - want).abs().max().item()
    assert torch.equal(b, want) and of.item() == 0


# ---- the byte-code kernels' int32 guard ---------------------------------------------------------------------------------------

def test_byte_code_pointwise_flags_a_sum_that_would_leave_int32():
    """|zp * colsum| + 128 * 128 * Cpad >= 2^31 for a column (8-bit codes: colsum near 128 * C, a frozen range far from
    zero): the kernel raises the overflow flag; the guard written for |q| <= 8, (|zp| + 128) * 8 * Cpad, stays below
    2^31 for the same call.  The same call with a small zero point raises nothing."""
    from codenet_amd import _native as N_
    lib, dev = N_.lib(), torch.device("cuda", 0)
    M, C, Co = 65, 1024, 20
    zp_big, zp_small = 20000.0, 100.0
    q = torch.full((Co, C), -128, dtype=torch.int32)
    colsum_abs = 128 * C
    assert zp_big * colsum_abs + 128 * 128 * C >= 2 ** 31 and (zp_big + 128) * 8 * C < 2 ** 31
    assert zp_small * colsum_abs + 128 * 128 * C < 2 ** 31
    a8 = torch.zeros(M, C, dtype=torch.int8, device=dev)
    cp = q.to(torch.int8).to(dev)
    ws, bias = torch.ones(Co, device=dev), torch.zeros(Co, device=dev)
    colsum = q.sum(1).to(torch.int32).to(dev)
    out = torch.zeros(M, Co, device=dev)
    flags = []
    for zp in (zp_big, zp_small):
        of = torch.zeros(1, dtype=torch.int32, device=dev)
        st = _state(dev, 1.0, zp)
        N_.check(lib.cdn_codenet_pointwise_q8_strided_forward(
            a8.data_ptr(), st.data_ptr(), M, C, Co, C, 0, cp.data_ptr(), ws.data_ptr(), colsum.data_ptr(), bias.data_ptr(),
            0, None, None, None, out.data_ptr(), of.data_ptr(), torch.cuda.current_stream().cuda_stream), "pwq8")
        torch.cuda.synchronize()
        flags.append(of.item())
    assert flags == [1, 0], flags


# ---- one stage on exact-arithmetic inputs, RUNNING ranges with planted extremes ---------------------------------------------

RUN_C, RUN_CO = 64, 32


def _exact_stage8_running(seed):
    """One W8A8 stage (64 -> 32 channels) for the running-range case: rows of magnitude 127 * 2^-k (power-of-two 8-bit
    scales) and extremes planted so that the three tracked widths are 255 / 32, 510 / 64 and 255 / 16 -- activation
    scales 32, 32 and 16 after the "+=" initialisation, unchanged by EMA steps on batches with the same extremes.
      s   = 1 + tot / 32, tot = 127 (x0 - x1) + 5 (x2 - x3) + 3 (x4 - x5) + (x6 - x7) kept in [-128, 127], both planted
      d   channels 8 / 9 are the constant 4 under taps (127, 127, 1) * 2^-8 / their negatives: +-255 / 64 in the interior;
          every other row has magnitude 127 * 2^-9 on inputs in {0, 1}: |d| <= 9 * 127 / 512 < 255 / 64
      r   output 0 sees channel 8 alone through 127 * 2^-5: fq(255 / 64) = 4 (code 128), 4 * 127 / 32 + 1 / 16 = 255 / 16;
          output 1 is relu-ed to 0 everywhere; the others carry three codes * 2^-7 on channels >= 10: |y| < 8"""
    from codenet_amd import pipeline
    from codenet_amd.pipeline.common import quantize_deform_stages
    net = pipeline.build_hot_path(quantized=False, planes=[RUN_C, RUN_CO], seed=seed)
    quantize_deform_stages(net, 8, 8, "symmetric", "asymmetric", True, False, False)
    net = net.eval()
    g = torch.Generator().manual_seed(seed)
    q = [m for m in net.deconv_layers if hasattr(m, "quant_deform_conv")][0]
    C, Co = RUN_C, RUN_CO
    with torch.no_grad():
        ws = torch.zeros(1, C, 1, 1)
        ws[0, :8, 0, 0] = torch.tensor([127., -127., 5., -5., 3., -3., 1., -1.]) * 2.0 ** -5
        q.quant_conv_scale.weight.copy_(ws)
        q.quant_conv_scale.bias.fill_(1.0)
        wd = torch.randint(-127, 128, (C, 1, 3, 3), generator=g).float()
        wd.view(C, -1)[torch.arange(C), torch.randint(0, 9, (C,), generator=g)] = \
            127.0 * (torch.randint(0, 2, (C,), generator=g).float() * 2 - 1)
        wd = wd * 2.0 ** -9
        wd[:8] = 0.0
        wd[:8, 0, 1, 1] = 127.0 * 2.0 ** -9
        pat = torch.zeros(3, 3)
        pat[0, 0], pat[1, 1], pat[2, 2] = 127.0, 127.0, 1.0
        wd[8, 0] = pat * 2.0 ** -8
        wd[9, 0] = -pat * 2.0 ** -8
        q.quant_deform_conv.weight.copy_(wd)
        wp = torch.zeros(Co, C, 1, 1)
        for co in range(Co):
            idx = torch.randperm(C - 10, generator=g)[:3] + 10
            codes = torch.randint(-127, 128, (3,), generator=g).float()
            codes[0] = 127.0 if torch.rand(1, generator=g).item() < 0.5 else -127.0
            wp[co, idx, 0, 0] = codes * 2.0 ** -7
        beta = torch.randint(-8, 9, (Co,), generator=g).float() / 8.0
        wp[0] = 0.0
        wp[0, 8, 0, 0] = 127.0 * 2.0 ** -5
        beta[0], beta[1] = 0.0625, -64.0
        q.quant_conv_channel_bn.conv.weight.copy_(wp)
        bn = q.quant_conv_channel_bn.bn
        bn.weight.fill_(1.0)
        bn.running_mean.zero_()
        var = torch.tensor(1.0 - bn.eps, dtype=torch.float32)
        if (var + bn.eps).item() != 1.0:
            var = torch.nextafter(var, torch.tensor(2.0))
        assert (var + bn.eps).item() == 1.0 and torch.sqrt(var + bn.eps).item() == 1.0
        bn.running_var.fill_(var.item())
        bn.bias.copy_(beta)
    return net


def _exact_input_running8(n, res, g):
    x = torch.randint(0, 2, (n, RUN_C, res, res), generator=g).float()
    xs = torch.randint(0, 2, (n, 8, res, res), generator=g).float()
    qv = torch.tensor([127., -127., 5., -5., 3., -3., 1., -1.]).view(1, 8, 1, 1)
    tot = (xs * qv).sum(1, keepdim=True)
    xs = xs * ((tot >= -128) & (tot <= 127)).float()               # offending pixels: s = 1
    xs[0, :, 2, 3] = torch.tensor([0., 1., 0., 0., 0., 0., 0., 1.])          # -127 - 1 = -128
    xs[n - 1, :, res - 3, 4] = torch.tensor([1., 0., 0., 0., 0., 0., 0., 0.])   # 127
    x[:, :8] = xs
    x[:, 8:10] = 4.0
    return x


def _oracle_stage8_running(x, w, mirrors):
    import torch.nn.functional as F
    from oracle import quant as Q
    r = Q.stage_w4a8(x, w["w_scale"], w["b_scale"], w["w_dw"], w["w_pw"], w["bn"], mirrors[0], mirrors[1], w_bits=8,
                     running=True, lo=w["lo"], hi=w["hi"])
    s_raw = torch.clamp(F.conv2d(x, Q.weight_fake_quant(w["w_scale"], 8), w["b_scale"]), w["lo"], w["hi"])
    rr = torch.relu(r["y"])
    r_q, r_codes = mirrors[2](rr, True, return_codes=True)
    return dict(s=s_raw, d=r["d"], r=rr, r_q=r_q, r_codes=r_codes)


@pytest.mark.parametrize("n,graph", [(4, False), (33, False), (4, True)])
def test_exact_arithmetic_w8a8_stage_running_ranges(n, graph):
    """A W8A8 stage with RUNNING ranges over three forwards on different inputs with planted extremes ("+="
    initialisation, then two EMA steps): s, d, relu(y), all three ranges (x_min / x_max) and the output torch.equal to
    the CPU oracle of the module path after every forward; from the second forward on also as a replayed graph."""
    import torch.nn.functional as F
    from codenet_amd import pipeline
    from oracle import dcn as O
    from oracle import quant as Q
    from tests.test_gpu_exact_codes import _Tap, _stage_weights
    net = _exact_stage8_running(seed=5)
    cpu = copy.deepcopy(net)
    net = net.cuda()
    pipeline.set_running_stat(net, True)
    fused = pipeline.FusedHotPath(net.deconv_layers)
    assert fused._stage_params(fused.stages[0])["kb_flag"] == W8
    tap = _Tap(fused, n)
    w = _stage_weights(list(cpu.deconv_layers)[0])
    mirrors = [Q.QuantActState(), Q.QuantActState(), Q.QuantActState()]
    g = torch.Generator().manual_seed(17)
    O.lib()
    xs = [_exact_input_running8(n, 16, g) for _ in range(3)]
    xbuf = xs[0].cuda()
    replay = None
    for it, x in enumerate(xs):
        ref = _oracle_stage8_running(x, w, mirrors)
        sc = [Q.act_params(m.x_min, m.x_max)[0].item() for m in mirrors]
        assert sc == [32.0, 32.0, 16.0], "test construction: activation scales %r" % sc
        tap.records.clear()
        if graph and it > 0:
            if replay is None:
                fused.stage_hook = None
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    out_static = fused(xbuf)
                replay = gr
            xbuf.copy_(x.cuda())
            replay.replay()
            torch.cuda.synchronize()
            out = out_static.cpu()
            acts = fused._stage_params(fused.stages[0])["acts"]
            ranges = [(a.x_min.cpu(), a.x_max.cpu()) for a in acts]
        else:
            xbuf.copy_(x.cuda())
            out = fused(xbuf).cpu()
            rec = tap.records[0]
            assert torch.equal(rec["s"], ref["s"]), "forward %d: s" % it
            assert torch.equal(rec["d"], ref["d"]), "forward %d: d (%g)" % (it, (rec["d"] - ref["d"]).abs().max().item())
            assert torch.equal(rec["r"], ref["r"]), "forward %d: relu(y)" % it
            ranges = rec["ranges"]
        for k, m in enumerate(mirrors):
            assert torch.equal(m.x_min, ranges[k][0]) and torch.equal(m.x_max, ranges[k][1]), \
                "forward %d: range %d (%r, %r) vs oracle (%r, %r)" % (it, k, ranges[k][0], ranges[k][1], m.x_min, m.x_max)
        want = F.interpolate(ref["r_q"], scale_factor=2, mode="nearest")
        assert torch.equal(out, want), "forward %d: output codes" % it
    q = fused.stages[0][0]
    assert q.quant_act[1].x_min.item() == -3.0 and q.quant_act[1].x_max.item() == 4.96875
    assert q.quant_identity_deform.x_max.item() == 3.984375 and list(net.deconv_layers)[-2][1].x_max.item() == 15.9375


# ---- the whole network on exact-arithmetic inputs ---------------------------------------------------------------------------

def _exact_model8(heads, seed):
    """create_model(quantize=True, w_bit=8) with every quantised weight row rewritten to a few integer codes in
    [-127, 127] (one of them +-127) times 2^-k -- power-of-two per-channel 8-bit scales, dyadic fake-quantised weights --
    exact BN folds (gamma = 1, mean = 0, var + eps == 1, dyadic beta) and dyadic biases.  At most 9 non-zero codes per
    row, so a sum of |level * code| stays below 9 * 510 * 127 * 16 (the 16: bilinear weights on the 1/4 grid of s) < 2^24
    once every level is within 510 of zero, which _freeze_dyadic asserts."""
    from codenet_amd import harness
    from codenet_amd.portable_quantizer import quant_modules as QM
    model = harness.create_model(heads=heads, quantize=True, w_bit=8)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, mod in model.named_modules():
            if not isinstance(mod, QM._WeightQuantizer):
                continue
            conv = mod.conv if hasattr(mod, "conv") else mod
            w = conv.weight
            Co, K = w.shape[0], w[0].numel()
            scale_conv = name.endswith("quant_conv_scale")
            nnz = min(K, 8 if scale_conv else 3)
            new = torch.zeros(Co, K)
            for row in range(Co):
                idx = torch.randperm(K, generator=g)[:nnz]
                codes = torch.randint(-127, 128, (nnz,), generator=g).float()
                codes[0] = 127.0 if torch.rand(1, generator=g).item() < 0.5 else -127.0
                new[row, idx] = codes
            w.copy_(new.view_as(w) * 2.0 ** (-11 if scale_conv else -7))
            if getattr(conv, "bias", None) is not None:
                conv.bias.copy_(torch.ones(Co) if scale_conv else torch.randint(-8, 9, (Co,), generator=g).float() / 8.0)
            if hasattr(mod, "bn"):
                bn = mod.bn
                bn.weight.fill_(1.0)
                bn.running_mean.zero_()
                var = torch.tensor(1.0 - bn.eps, dtype=torch.float32)
                if (var + bn.eps).item() != 1.0:
                    var = torch.nextafter(var, torch.tensor(2.0))
                assert (var + bn.eps).item() == 1.0 and torch.sqrt(var + bn.eps).item() == 1.0
                bn.running_var.fill_(var.item())
                bn.bias.copy_(torch.randint(-2, 7, (Co,), generator=g).float() / 8.0)
    return model


def _freeze_dyadic(model, x):
    """Frozen ranges of width 255 * 2^j (activation scales are powers of two, zero points integers) that cover what the
    CPU module path feeds every QuantAct on `x`: one running pass for the extremes, then frozen passes that widen a range
    until nothing leaves its byte grid.  The scale planes of the deform stages get (-31.875, 31.875): s on a 1/4 grid."""
    import math
    from codenet_amd import pipeline
    from codenet_amd.portable_quantizer.quant_modules import QuantAct
    acts = [(n, m) for n, m in model.named_modules() if isinstance(m, QuantAct)]
    pipeline.set_running_stat(model, True)
    with torch.no_grad():
        model(x)
    pipeline.set_running_stat(model, False)
    seen = {}
    hooks = [m.register_forward_pre_hook(lambda mod, inp: seen.__setitem__(
        id(mod), (min(seen.get(id(mod), (1e30, -1e30))[0], inp[0].min().item()),
                  max(seen.get(id(mod), (1e30, -1e30))[1], inp[0].max().item())))) for _, m in acts]

    def fit(m, lo, hi, name):
        if name.endswith("quant_act.1") and "deconv_layers" in name:      # the scale plane s of a deform stage
            lo, hi, j = -31.875, 31.875, -2
        else:
            j = math.ceil(math.log2(max(hi - lo, 1e-3) * 1.25 / 255.0))
            lo = 0.0 if lo >= 0 else math.floor(lo * 1.125 / 2.0 ** j) * 2.0 ** j
            while lo + 255 * 2.0 ** j < hi:
                j += 1
                lo = 0.0 if lo >= 0 else math.floor(lo / 2.0 ** j) * 2.0 ** j
            hi = lo + 255 * 2.0 ** j
        with torch.no_grad():
            m.x_min.fill_(lo)
            m.x_max.fill_(hi)
    for n, m in acts:
        fit(m, m.x_min.item(), m.x_max.item(), n)
    for _ in range(8):
        seen.clear()
        with torch.no_grad():
            model(x)
        bad = [(n, m) for n, m in acts if seen[id(m)][0] < m.x_min.item() or seen[id(m)][1] > m.x_max.item()]
        if not bad:
            break
        for n, m in bad:
            fit(m, min(seen[id(m)][0], m.x_min.item()), max(seen[id(m)][1], m.x_max.item()), n)
    assert not bad, [n for n, _ in bad]
    for h in hooks:
        h.remove()
    for n, m in acts:
        scale = 255.0 / (m.x_max.item() - m.x_min.item())
        assert math.frexp(scale)[0] == 0.5, (n, scale)
        assert abs(m.x_min.item() * scale) <= 255 and abs(m.x_max.item() * scale) <= 510, n       # every level within 510
    return model


@pytest.mark.parametrize("heads", [None, {"hm": 80, "wh": 2, "reg": 2}])
def test_exact_arithmetic_w8a8_whole_network(heads, monkeypatch):
    """create_model(quantize=True, w_bit=8) on inputs where every summation order gives the same fp32 value (integer
    image, sparse rows of magnitude 127 * 2^-k, frozen dyadic ranges; the 24-bit bound asserted on the CPU): the head
    outputs of the fused schedule and of the byte-code serving schedule are torch.equal to the CPU module path."""
    from codenet_amd import pipeline
    from codenet_amd.modules import dcn_deform_conv as M
    from codenet_amd.portable_quantizer import quant_modules as QM
    from oracle import dcn as O
    monkeypatch.setattr(M, "deform_conv", O.deform_conv)
    monkeypatch.setattr(QM, "deform_conv", O.deform_conv)
    O.lib()
    x = torch.randint(0, 4, (2, 3, 128, 128), generator=torch.Generator().manual_seed(7)).float()
    model = _freeze_dyadic(_exact_model8(heads, seed=29), x)
    with torch.no_grad():
        want = {k: v.clone() for k, v in model(x)[-1].items()}
    assert all(v.unique().numel() > 16 for v in want.values())
    monkeypatch.undo()
    a = copy.deepcopy(model).cuda().enable_fused()
    b = copy.deepcopy(model).cuda().enable_fused(frozen_codes=True)
    xg = x.cuda()
    assert a._plan(xg) == ("fused", False, False) and b._plan(xg) == ("bytes", True, True)
    with torch.no_grad():
        ga = {k: v.cpu() for k, v in a(xg)[-1].items()}
        gb = {k: v.cpu() for k, v in b(xg)[-1].items()}
    assert not b.frozen_overflowed()
    for k in want:
        assert torch.equal(ga[k], want[k]), ("fused", k, (ga[k] - want[k]).abs().max().item())
        assert torch.equal(gb[k], want[k]), ("bytes", k, (gb[k] - want[k]).abs().max().item())
