"""Host side of the native QAT units (functions/codenet_units.py): the gate that decides between the kernels and the module
path, the DetectionTrunk / GraphedTrainStep scope test and the library's new entry points.  No GPU."""
import copy

import torch

NEW_SYMBOLS = ("cdn_codenet_pointwise_forward_pitched", "cdn_codenet_pointwise_wgrad_pitched", "cdn_codenet_unit_dw_forward",
               "cdn_codenet_unit_dw_backward_workspace_bytes", "cdn_codenet_unit_dw_backward",
               "cdn_codenet_unit_join_forward", "cdn_codenet_unit_join_backward")


def _model(**kw):
    from codenet_amd import harness
    return harness.create_model(quantize=kw.pop("quantize", True), **kw)


def test_the_library_exports_the_new_entry_points():
    from codenet_amd import _native
    lib = _native.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s) and s in _native._SIGNATURES, s


def test_argument_errors_come_back_before_any_launch():
    from codenet_amd import _native
    lib = _native.lib()
    one, big = 4096, 1 << 20
    ARG, UNSUPPORTED, WORKSPACE = -1, -5, -6
    # a workspace that is too small, a tensor beyond 32-bit indexing: their own codes
    assert lib.cdn_codenet_unit_dw_backward(one, one, 24 * 64, None, one, one, 24 * 64, 0, None, None, 1, 24, 8, 8, 2, one, 16,
                                            None) == WORKSPACE
    assert lib.cdn_codenet_unit_dw_forward(one, 24 * 4096 * 4096, None, one, one, one, 8, 24, 4096, 4096, 1, None, None, None,
                                           None, 8, 0.99, 0, None, None) == UNSUPPORTED

    def fwd(inp=one, pitch=24 * 64, N=1, C=24, H=8, W=8, stride=2, running=0):
        return lib.cdn_codenet_unit_dw_forward(inp, pitch, None, one, one, one, N, C, H, W, stride, None, None, None, None, 8,
                                               0.99, running, None, None)

    assert fwd(inp=None) == ARG                      # a null pointer
    assert fwd(stride=3) == ARG and fwd(stride=0) == ARG
    assert fwd(pitch=24 * 64 - 1) == ARG             # a pitch smaller than C * H * W
    assert fwd(H=0) == ARG and fwd(N=-1) == ARG      # a non-positive size
    assert fwd(running=1) == ARG                     # a running range without the QuantAct's buffers

    def bwd(g=one, pitch=24 * 64, gpitch=24 * 64, stride=1, W=8):
        return lib.cdn_codenet_unit_dw_backward(g, one, pitch, one, one, one, gpitch, 0, None, None, 1, 24, 8, W, stride, one,
                                                big, None)

    assert bwd(g=None) == ARG and bwd(stride=4) == ARG and bwd(pitch=5) == ARG and bwd(gpitch=24 * 64 - 1) == ARG
    assert bwd(W=0) == ARG
    assert lib.cdn_codenet_unit_join_forward(one, None, one, 1, None, 0, 1, 58, 64, None) == ARG
    assert lib.cdn_codenet_unit_join_forward(one, one, one, 2, None, 0, 1, 58, 64, None) == ARG
    assert lib.cdn_codenet_unit_join_forward(one, one, one, 1, one, 58 * 64 - 1, 1, 58, 64, None) == ARG
    assert lib.cdn_codenet_unit_join_forward(one, one, one, 1, None, 0, 1, 58, 0, None) == ARG
    assert lib.cdn_codenet_unit_join_backward(one, one, None, 1, None, 0, 1, 58, 64, None) == ARG
    assert lib.cdn_codenet_unit_join_backward(one, one, one, 0, one, 58 * 64, 1, 58, 64, None) == ARG      # slot 0 + pass-through
    assert lib.cdn_codenet_unit_join_backward(one, one, one, 1, one, 58 * 64 - 1, 1, 58, 64, None) == ARG
    assert lib.cdn_codenet_pointwise_forward_pitched(one, 58 * 64 - 1, None, one, None, one, 58 * 64, 1, 58, 58, 64, 0, None,
                                                     None) == ARG
    assert lib.cdn_codenet_pointwise_forward_pitched(one, 58 * 64, None, one, None, one, 58 * 64 - 1, 1, 58, 58, 64, 0, None,
                                                     None) == ARG
    assert lib.cdn_codenet_pointwise_forward_pitched(None, 58 * 64, None, one, None, one, 58 * 64, 1, 58, 58, 64, 0, None,
                                                     None) == ARG
    assert lib.cdn_codenet_pointwise_forward_pitched(one, 58 * 64, None, one, None, one, 58 * 64, 0, 58, 58, 64, 0, None,
                                                     None) == ARG
    assert lib.cdn_codenet_pointwise_wgrad_pitched(one, one, 58 * 64 - 1, one, None, 1, 58, 58, 64, one, big, None) == ARG
    assert lib.cdn_codenet_pointwise_wgrad_pitched(one, None, 58 * 64, one, None, 1, 58, 58, 64, one, big, None) == ARG


def _ws_formula(N, C, H, W, stride):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    rows = 8 if Ho >= 32 else 4
    items = N * -(-Ho // rows) * -(-Wo // 4)
    chunks = -(-items // 256)
    return -(-(C * chunks * 10 * 4) // 256) * 256


def test_workspace_size_is_the_documented_formula():
    from codenet_amd import _native
    lib = _native.lib()
    for shape in ((32, 232, 16, 16, 1), (32, 24, 128, 128, 2), (32, 58, 64, 64, 1), (2, 58, 9, 10, 2), (2, 116, 12, 20, 1),
                  (1, 1, 1, 1, 1), (3, 7, 65, 33, 2)):
        assert lib.cdn_codenet_unit_dw_backward_workspace_bytes(*shape) == _ws_formula(*shape), shape
    assert lib.cdn_codenet_unit_dw_backward_workspace_bytes(32, 232, 16, 16, 1) == 18688      # 232 channels x 2 chunks
    assert lib.cdn_codenet_unit_dw_backward_workspace_bytes(2, 58, 9, 10, 3) == 0
    assert lib.cdn_codenet_unit_dw_backward_workspace_bytes(0, 58, 9, 10, 1) == 0


def test_native_reason_names_the_cause_of_every_gate():
    from codenet_amd.functions import codenet_units as CU
    model = _model()
    layer = model.layer2
    x = torch.rand(1, 116, 8, 8)
    assert CU.native_reason(layer, None) is None and CU.native_reason(layer[0], None) is None
    assert CU.native_reason(model.layer4, None) is None
    assert "cpu" in CU.native_reason(layer, x) and "cpu" in CU.native_reason(model.layer4, torch.rand(1, 464, 4, 4))
    with torch.no_grad():
        assert "grad" in CU.native_reason(layer, x)
    assert "percentile" in CU.native_reason(_model(act_percentile=True).layer2, x)
    assert "percentile" in CU.native_reason(_model(act_percentile=True).layer4, x)
    hooked = copy.deepcopy(layer)
    hooked[1].quant_convbn2.register_forward_hook(lambda m, i, o: None)
    why = CU.native_reason(hooked, x)
    assert "hook" in why and "quant_convbn2" in why
    l4 = copy.deepcopy(model.layer4)
    l4[1].register_forward_pre_hook(lambda m, i: None)
    assert "hook" in CU.native_reason(l4, None)
    why = CU.native_reason(_model(quantize=False).layer2, x)
    assert "QuantBaseNode" in why
    sym = copy.deepcopy(layer)
    sym[0].quant_act4.quant_mode = "symmetric"
    assert "asymmetric" in CU.native_reason(sym, x) and "quant_act4" in CU.native_reason(sym, x)
    glob = copy.deepcopy(layer)
    glob[2].quant_act.global_range = True      # the shared act: every unit sees it
    assert "global_range" in CU.native_reason(glob, x)
    geo = copy.deepcopy(layer)
    geo[0].quant_convbn2.conv.padding = (0, 0)
    assert "geometry" in CU.native_reason(geo, x)
    for attr, val in (("per_channel", False), ("quant_mode", "asymmetric"), ("quantize_bias", True), ("weight_bit", 8)):
        wq = copy.deepcopy(layer)
        setattr(wq[1].quant_convbn3, attr, val)
        assert "weight quantiser" in CU.native_reason(wq, x), attr
    assert "neither" in CU.native_reason(torch.nn.ReLU(), x)
    CU.NATIVE_UNITS = False
    try:
        assert "NATIVE_UNITS" in CU.native_reason(layer, x)
    finally:
        CU.NATIVE_UNITS = True


def test_forward_units_and_layer4_are_the_module_path_on_cpu_tensors():
    from codenet_amd.functions import codenet_units as CU
    model = _model()
    g = torch.Generator().manual_seed(0)
    for name, shape in (("layer1", (2, 24, 9, 10)), ("layer2", (2, 116, 8, 8)), ("layer4", (2, 464, 4, 4))):
        x = torch.rand(*shape, generator=g) * 4
        for grad in (True, False):
            a, b = copy.deepcopy(getattr(model, name)), copy.deepcopy(getattr(model, name))
            with torch.set_grad_enabled(grad):
                keep = {}
                got = CU.forward_layer4(a, x) if name == "layer4" else CU.forward_units(a, x, keep=keep)
                want = b(x)
            assert torch.equal(got, want) and not keep, (name, grad)
            for (n1, b1), (_, b2) in zip(a.named_buffers(), b.named_buffers()):
                assert torch.equal(b1, b2), n1


def test_is_native_trunk_accepts_the_trunk_and_rejects_everything_else():
    from codenet_amd import pipeline
    model = _model()
    trunk = pipeline.DetectionTrunk(model)
    assert trunk.layer1 is model.layer1 and trunk.layer4 is model.layer4 and trunk.hm is model.hm      # shared, not copied
    assert trunk.deconv_layers is model.deconv_layers and list(trunk.head_modules()) == list(model.heads)
    assert not hasattr(trunk, "layer0")
    G = pipeline.GraphedTrainStep
    assert G.is_native_trunk(trunk) and not G.is_native_tail(trunk) and not G.is_stage_stack(trunk)
    tail = pipeline.DetectionTail(model)
    assert G.is_native_tail(tail) and not G.is_native_trunk(tail)
    assert not G.is_native_trunk(model) and not G.is_native_tail(model) and not G.is_stage_stack(model)
    assert not G.is_native_trunk(pipeline.DetectionTrunk(_model(quantize=False)))
    assert not G.is_native_trunk(pipeline.DetectionTrunk(_model(act_percentile=True)))
    one_pct = _model()
    one_pct.layer3[0].quant_act2.percentile = True
    assert not G.is_native_trunk(pipeline.DetectionTrunk(one_pct))
    hooked = _model()
    hooked.layer2[3].quant_convbn1.register_forward_hook(lambda m, i, o: None)
    assert not G.is_native_trunk(pipeline.DetectionTrunk(hooked))
    from codenet_amd.functions import codenet_units as CU
    CU.NATIVE_UNITS = False
    try:
        assert not G.is_native_trunk(trunk)
    finally:
        CU.NATIVE_UNITS = True
    assert "DetectionTrunk" in G.__doc__ and "is_native_trunk" in G.__doc__
