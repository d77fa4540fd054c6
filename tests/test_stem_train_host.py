"""Host side of the native QAT stem (functions/codenet_stem.py): the gate that decides between the kernels and the module
path, the DetectionNet / GraphedTrainStep scope test and the library's new entry points.  No GPU."""
import copy

import torch

NEW_SYMBOLS = ("cdn_codenet_stem_train_forward", "cdn_codenet_stem_pool_forward", "cdn_codenet_stem_pool_backward",
               "cdn_codenet_stem_backward_workspace_bytes", "cdn_codenet_stem_backward")


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

    def fwd(img=one, w=one, y0=one, N=1, H=8, W=8, Co=24, stride=4, running=0):
        return lib.cdn_codenet_stem_train_forward(img, w, one, y0, N, H, W, Co, stride, None, None, None, None, 8, 0.99,
                                                  running, None, None)

    assert fwd(img=None) == ARG and fwd(w=None) == ARG and fwd(y0=None) == ARG      # a null pointer
    assert fwd(stride=3) == ARG and fwd(stride=1) == ARG and fwd(stride=0) == ARG
    assert fwd(H=0) == ARG and fwd(N=-1) == ARG and fwd(W=0) == ARG                   # a non-positive size
    assert fwd(Co=23) == ARG and fwd(Co=32) == ARG
    assert fwd(running=1) == ARG                     # a running range without the QuantAct's buffers
    assert fwd(N=64, H=4096, W=4096) == UNSUPPORTED  # an image batch beyond 32-bit indexing

    def bwd(g=one, img=one, ws=one, nbytes=big, N=1, H=8, W=8, Co=24, stride=4):
        return lib.cdn_codenet_stem_backward(g, one, img, one, one, N, H, W, Co, stride, ws, nbytes, None)

    assert bwd(g=None) == ARG and bwd(img=None) == ARG and bwd(ws=None) == ARG
    assert bwd(stride=3) == ARG and bwd(H=0) == ARG and bwd(N=0) == ARG and bwd(Co=3) == ARG
    assert bwd(N=64, H=4096, W=4096) == UNSUPPORTED
    need = lib.cdn_codenet_stem_backward_workspace_bytes(2, 64, 64, 2)
    assert need > 0 and bwd(N=2, H=64, W=64, stride=2, nbytes=need - 1) == WORKSPACE      # one byte short: its own code
    assert bwd(N=2, H=64, W=64, stride=2, ws=one + 4) == WORKSPACE                        # not 16-byte aligned
    pf = lib.cdn_codenet_stem_pool_forward
    assert pf(None, one, one, 1, 24, 8, 8, None) == ARG and pf(one, None, one, 1, 24, 8, 8, None) == ARG
    assert pf(one, one, None, 1, 24, 8, 8, None) == ARG and pf(one, one, one, 1, 24, 0, 8, None) == ARG
    assert pf(one, one, one, 0, 24, 8, 8, None) == ARG
    assert pf(one, one, one, 64, 24, 2048, 2048, None) == UNSUPPORTED
    pb = lib.cdn_codenet_stem_pool_backward
    assert pb(None, one, one, one, 1, 24, 8, 8, None) == ARG and pb(one, None, one, one, 1, 24, 8, 8, None) == ARG
    assert pb(one, one, None, one, 1, 24, 8, 8, None) == ARG and pb(one, one, one, None, 1, 24, 8, 8, None) == ARG
    assert pb(one, one, one, one, 1, 24, 8, -1, None) == ARG
    assert pb(one, one, one, one, 64, 24, 2048, 2048, None) == UNSUPPORTED


def _ws_formula(N, H, W, stride):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    P = N * Ho * Wo
    T = min(8, max(1, P // 1024))
    chunks = -(-P // (256 * T))
    return -(-(6 * chunks * 112 * 4) // 256) * 256


def test_workspace_size_is_the_documented_formula():
    from codenet_amd import _native
    lib = _native.lib()
    for shape in ((32, 512, 512, 4), (32, 512, 512, 2), (2, 36, 44, 4), (2, 17, 22, 2), (2, 64, 64, 2), (2, 128, 128, 4),
                  (1, 1, 1, 4), (3, 65, 33, 2)):
        assert lib.cdn_codenet_stem_backward_workspace_bytes(*shape) == _ws_formula(*shape), shape
    assert lib.cdn_codenet_stem_backward_workspace_bytes(32, 512, 512, 4) == 6 * 256 * 112 * 4      # 256 chunks of 2048
    assert lib.cdn_codenet_stem_backward_workspace_bytes(2, 64, 64, 3) == 0
    assert lib.cdn_codenet_stem_backward_workspace_bytes(0, 64, 64, 4) == 0


def test_native_reason_names_the_cause_of_every_gate():
    from codenet_amd.functions import codenet_stem as ST
    x = torch.rand(1, 3, 16, 16)
    for maxpool in (False, True):
        layer0 = _model(maxpool=maxpool).layer0
        assert ST.native_reason(layer0, None) is None
        assert len(layer0[1]) == (3 if maxpool else 2) and layer0[0].conv.stride == ((2, 2) if maxpool else (4, 4))
        assert "cpu" in ST.native_reason(layer0, x)
        with torch.no_grad():
            assert "grad" in ST.native_reason(layer0, x)
    layer0 = _model().layer0
    assert "QuantBnConv2d" in ST.native_reason(_model(quantize=False).layer0, x)
    assert "percentile" in ST.native_reason(_model(act_percentile=True).layer0, x)
    hooked = copy.deepcopy(layer0)
    hooked[1][1].register_forward_hook(lambda m, i, o: None)
    assert "hook" in ST.native_reason(hooked, x) and "hook" in ST.native_reason(hooked, None)
    sym = copy.deepcopy(layer0)
    sym[1][1].quant_mode = "symmetric"
    assert "asymmetric" in ST.native_reason(sym, None)
    glob = copy.deepcopy(layer0)
    glob[1][1].global_range = True
    assert "global_range" in ST.native_reason(glob, None)
    for attr, val in (("stride", (1, 1)), ("padding", (0, 0)), ("dilation", (2, 2)), ("padding_mode", "reflect")):
        geo = copy.deepcopy(layer0)
        setattr(geo[0].conv, attr, val)
        assert "geometry" in ST.native_reason(geo, None), attr
    pooled = _model(maxpool=True).layer0
    for attr, val in (("kernel_size", 2), ("ceil_mode", True), ("return_indices", True), ("dilation", 2), ("stride", 1)):
        p = copy.deepcopy(pooled)
        setattr(p[1][2], attr, val)
        assert "pool" in ST.native_reason(p, None), attr
    for attr, val in (("per_channel", False), ("quant_mode", "asymmetric"), ("quantize_bias", True), ("weight_bit", 16)):
        wq = copy.deepcopy(layer0)
        setattr(wq[0], attr, val)
        assert "weight quantiser" in ST.native_reason(wq, None), attr
    narrow = copy.deepcopy(layer0)
    narrow[0].weight_bit = 4      # any width up to 8 bits is accepted
    assert ST.native_reason(narrow, None) is None
    assert "Sequential" in ST.native_reason(torch.nn.ReLU(), None)
    ST.NATIVE_STEM = False
    try:
        assert "NATIVE_STEM" in ST.native_reason(layer0, x) and "NATIVE_STEM" in ST.native_reason(layer0, None)
    finally:
        ST.NATIVE_STEM = True
    # an image that requires grad: no input gradient is built, whatever the device
    why = ST.native_reason(layer0, x.clone().requires_grad_())
    assert "requires grad" in why and "cpu" not in why


def test_forward_stem_is_the_module_path_on_cpu_tensors():
    from codenet_amd.functions import codenet_stem as ST
    g = torch.Generator().manual_seed(0)
    for maxpool in (False, True):
        layer0 = _model(maxpool=maxpool).layer0
        for shape in ((2, 3, 17, 22), (2, 3, 32, 32)):
            x = torch.rand(*shape, generator=g) * 4 - 2
            for grad in (True, False):
                a, b = copy.deepcopy(layer0), copy.deepcopy(layer0)
                with torch.set_grad_enabled(grad):
                    keep = {}
                    got = ST.forward_stem(a, x, keep=keep)
                    want = b(x)
                assert torch.equal(got, want) and not keep, (maxpool, shape, grad)
                for (n1, b1), (_, b2) in zip(a.named_buffers(), b.named_buffers()):
                    assert torch.equal(b1, b2), n1
                assert float(a[1][1].x_max) > 0      # the QuantAct's range moved in place


def test_the_three_wrappers_share_the_models_modules_in_one_registration_order():
    from codenet_amd import pipeline
    model = _model()
    heads = list(model.heads)
    assert heads == ["hm", "wh", "reg"]
    layers = ["layer0", "layer1", "layer2", "layer3", "layer4"]
    classes = {pipeline.DetectionTail: [], pipeline.DetectionTrunk: layers[1:], pipeline.DetectionNet: layers}
    for cls, front in classes.items():
        w = cls(model)
        names = front + ["deconv_layers"] + heads      # layers ascending, the stages, the heads in model.heads order
        assert [n for n, _ in w.named_children()] == names, cls.__name__
        assert all(getattr(w, n) is getattr(model, n) for n in names)
        own = dict(model.named_parameters())
        params = list(w.named_parameters())
        assert params and all(p is own[n] for n, p in params), cls.__name__      # the model's own objects, under its names
        assert [n for n, _ in params] == [n for n in own if n.split(".")[0] in names]      # (and so an optimizer's order)
        assert list(w.state_dict()) == [k for k in model.state_dict() if k.split(".")[0] in names]
        assert type(w.heads) is dict and w.heads == dict(model.heads) and list(w.head_modules()) == heads
        assert not any(issubclass(cls, other) for other in classes if other is not cls)


def test_is_native_net_accepts_the_whole_net_and_rejects_everything_else():
    from codenet_amd import pipeline
    model = _model()
    net = pipeline.DetectionNet(model)
    assert net.layer0 is model.layer0 and net.layer1 is model.layer1 and net.layer4 is model.layer4      # shared, not copied
    assert net.hm is model.hm and net.deconv_layers is model.deconv_layers
    assert list(net.head_modules()) == list(model.heads)
    G = pipeline.GraphedTrainStep
    assert G.is_native_net(net)
    assert not G.is_native_trunk(net) and not G.is_native_tail(net) and not G.is_stage_stack(net)
    assert G.is_native_net(pipeline.DetectionNet(_model(maxpool=True)))
    assert not G.is_native_net(model)      # the bare model: its forward dispatches on inference schedules
    trunk = pipeline.DetectionTrunk(model)
    assert G.is_native_trunk(trunk) and not G.is_native_net(trunk) and not G.is_native_net(pipeline.DetectionTail(model))
    assert not G.is_native_net(pipeline.DetectionNet(_model(quantize=False)))
    assert not G.is_native_net(pipeline.DetectionNet(_model(act_percentile=True)))
    hooked = _model()
    hooked.layer0[0].register_forward_hook(lambda m, i, o: None)
    assert not G.is_native_net(pipeline.DetectionNet(hooked))
    assert G.is_native_trunk(pipeline.DetectionTrunk(hooked))      # the hook sits in the stem alone
    one_pct = _model()
    one_pct.layer3[0].quant_act2.percentile = True      # a unit off the native path takes the whole net with it
    assert not G.is_native_net(pipeline.DetectionNet(one_pct))
    from codenet_amd.functions import codenet_stem as ST
    ST.NATIVE_STEM = False
    try:
        assert not G.is_native_net(net) and G.is_native_trunk(trunk)
    finally:
        ST.NATIVE_STEM = True
    assert "DetectionNet" in G.__doc__ and "is_native_net" in G.__doc__
