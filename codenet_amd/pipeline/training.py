"""GraphedTrainStep: the QAT step of the deform-stage stack -- or of the detection tail, stages + heads, or of the trunk,
layers 1-4 in front of that tail, or of the whole network from the image -- as one HIP graph.

Part of codenet_amd.pipeline (split by concern in round 6; `from codenet_amd import pipeline` exposes every name as
before)."""
import collections
import importlib

import torch
import torch.nn as nn


class _DetectionChain(nn.Module):
    """The back of a CoDeNet from one of its layers on as one module for the QAT step.  PARTS names what a subclass takes
    from `model` (a harness.PoseShuffleNetV2) in front of the heads, in registration order; the modules are SHARED, not
    copied.  forward(x) -> [{head: tensor}], as the model's own forward returns it, always through the training chain
    functions/codenet_stem.forward_stem -> codenet_units.forward_units x 3 -> forward_layer4 ->
    codenet_stage.forward_stage_blocks -> codenet_heads.forward_heads, entered at the first part present."""
    PARTS = ()

    def __init__(self, model):
        super().__init__()
        self.heads = dict(model.heads)
        for name in self.PARTS + tuple(self.heads):
            setattr(self, name, getattr(model, name))

    def head_modules(self):
        return {h: getattr(self, h) for h in self.heads}

    def forward(self, x):
        from ..functions.codenet_heads import forward_heads
        from ..functions.codenet_stage import forward_stage_blocks
        from ..functions.codenet_stem import forward_stem
        from ..functions.codenet_units import forward_layer4, forward_units
        if "layer0" in self.PARTS:
            x = forward_stem(self.layer0, x)
        if "layer1" in self.PARTS:
            for layer in (self.layer1, self.layer2, self.layer3):
                x = forward_units(layer, x)
        if "layer4" in self.PARTS:
            x = forward_layer4(self.layer4, x)
        return [forward_heads(self.head_modules(), forward_stage_blocks(self.deconv_layers, x))]


class DetectionTail(_DetectionChain):
    """Everything of the CoDeNet behind the backbone as one module: the deform stages and the detection heads of `model`
    (a harness.PoseShuffleNetV2; the modules are SHARED, not copied).  forward(feat) -> [{head: tensor}] from a layer-4
    feature map, as the model's own forward returns it.  After quantisation every kernel of its training step is this
    library's (functions/codenet_stage.forward_stage_blocks, functions/codenet_heads.forward_heads)."""
    PARTS = ("deconv_layers",)


class DetectionTrunk(_DetectionChain):
    """Everything of the CoDeNet behind the stem as one module: layers 1-4 of the backbone, the deform stages and the
    detection heads of `model` (modules SHARED, not copied).  forward(feat0) -> [{head: tensor}] from layer0's output.
    After quantisation every kernel of its training step is this library's (functions/codenet_units.forward_units /
    forward_layer4 in front of DetectionTail's chain); the stem stays outside (DetectionNet takes it in)."""
    PARTS = ("layer1", "layer2", "layer3", "layer4", "deconv_layers")


class DetectionNet(_DetectionChain):
    """The whole CoDeNet as one module for the QAT step: the stem, layers 1-4 of the backbone, the deform stages and the
    detection heads of `model` (modules SHARED, not copied).  forward(img) -> [{head: tensor}] from the image, always through
    the training chain functions/codenet_stem.forward_stem -> codenet_units.forward_units x 3 -> forward_layer4 ->
    codenet_stage.forward_stage_blocks -> codenet_heads.forward_heads -- never through the inference schedules the model's
    own forward dispatches on.  After quantisation every kernel of its training step is this library's."""
    PARTS = ("layer0",) + DetectionTrunk.PARTS


def _stage_blocks_ok(seq):
    """A Sequential of [quantised deform stage, Sequential(ReLU, QuantAct), Upsample] blocks."""
    from ..portable_quantizer.quant_modules import QuantAct, QuantDeformConvWithOffsetScaleBoundPositive
    if not isinstance(seq, nn.Sequential) or len(seq) == 0 or len(seq) % 3:
        return False
    mods = list(seq)
    for i in range(0, len(mods), 3):
        q, post, up = mods[i:i + 3]
        if not (isinstance(q, QuantDeformConvWithOffsetScaleBoundPositive) and isinstance(post, nn.Sequential)
                and len(post) == 2 and isinstance(post[0], nn.ReLU) and isinstance(post[1], QuantAct)
                and isinstance(up, nn.Upsample)):
            return False
    return True


_Scope = collections.namedtuple("_Scope", "name predicate chain precision words shown_by")

# What GraphedTrainStep accepts without `unvalidated=True`, one row per scope: its name (`GraphedTrainStep.scope_of`), its
# public predicate, the chain class whose parts are judged (`_chain_reason`) or None for a stage stack (`_is_stack`), the
# precision that picks the gates and their order below, the words of the constructor's error, and the test file that shows
# its replays bit-identical to the eager steps.
SCOPES = (
    # The quantised stages -- this row and the `deconv_layers` part of the three QAT chains -- are judged by their classes
    # alone (`_stage_blocks_ok`).  That is weaker than `block_ok` inside functions/codenet_stage.forward_stage_blocks, which
    # also asks native_act_ok, global_range, the Upsample's mode and factor and hooks: a stack whose post-stage QuantAct has
    # percentile=True is accepted here although forward_stage_blocks then takes seq(x).  Merging the two changes answers: left as it is (DESIGN.md
    # section 4.3, "The scope table").
    _Scope("stage stack", "is_stage_stack", None, "qat",
           "a stack of quantised deform stages (pipeline.build_hot_path, a quantised deconv_layers)",
           "tests/test_train_step.py"),
    _Scope("fp32 stack", "is_fp32_stage_stack", None, "fp32",
           "the fp32 stack (a pipeline.DeconvLayers of [deform stage, BatchNorm2d, ReLU, Upsample] blocks)",
           "tests/test_gpu_bn_block.py"),
    _Scope("QAT tail", "is_native_tail", DetectionTail, "qat",
           "a pipeline.DetectionTail of a quantised model whose heads run natively", "tests/test_gpu_heads_train.py"),
    _Scope("QAT trunk", "is_native_trunk", DetectionTrunk, "qat",
           "a pipeline.DetectionTrunk of a quantised model whose units also run natively", "tests/test_gpu_units_train.py"),
    _Scope("QAT net", "is_native_net", DetectionNet, "qat",
           "a pipeline.DetectionNet of a quantised model whose stem also runs natively", "tests/test_gpu_stem_train.py"),
    _Scope("fp32 tail", "is_fp32_tail", DetectionTail, "fp32",
           "the fp32 tail (a pipeline.DetectionTail of an fp32 model: those blocks and the fp32 heads)",
           "tests/test_gpu_heads_fp32.py"),
    _Scope("fp32 trunk", "is_fp32_trunk", DetectionTrunk, "fp32",
           "the fp32 trunk (a pipeline.DetectionTrunk of an fp32 model: layers 1-4 in front of that tail)",
           "tests/test_gpu_units_fp32.py"),
    _Scope("fp32 net", "is_fp32_net", DetectionNet, "fp32",
           "the fp32 network (a pipeline.DetectionNet of an fp32 model: the fp32 stem, judged with the example image, in "
           "front of that trunk)", "tests/test_gpu_stem_fp32.py"),
)
_ROW = {s.predicate: s for s in SCOPES}

# Per precision: the functions/ module whose native_reason(part, x) gates each part (None: `_stage_blocks_ok` alone), the
# order in which the parts of a chain are asked -- it decides which reason is reported first -- and the text for a
# `deconv_layers` that is no sequence of that precision's blocks at all.
_LAYERS = ("layer1", "layer2", "layer3", "layer4")
_GATES = {"qat": dict(dict.fromkeys(_LAYERS, "codenet_units"), layer0="codenet_stem", deconv_layers=None,
                      heads="codenet_heads"),
          "fp32": dict(dict.fromkeys(_LAYERS, "codenet_units_fp32"), layer0="codenet_stem_fp32", deconv_layers="codenet_bn",
                       heads="codenet_heads_fp32")}
_ORDER = {"qat": ("deconv_layers", "heads") + _LAYERS + ("layer0",),
          "fp32": ("layer0",) + _LAYERS + ("deconv_layers", "heads")}
_NOT_STAGES = {"qat": "not a Sequential of [quantised deform stage, Sequential(ReLU, QuantAct), Upsample] blocks",
               "fp32": "not a Sequential of [deform stage, BatchNorm2d, ReLU, Upsample] blocks"}


def _part_reason(precision, name, part, x=None):
    """None, or the reason -- the gate's own words -- why `part`, the part `name` of a net, is outside the scopes of
    `precision`.  x None: the modules alone are judged.  The QAT gates see the caller's grad mode (under no_grad every one
    refuses); the fp32 gates are asked with grad mode on: their answer is a property of the modules.  The gate is looked up
    at every call, so a NATIVE_* switch of its module counts from the moment it is flipped."""
    if name == "deconv_layers" and not (_stage_blocks_ok(part) if precision == "qat"
                                        else isinstance(part, nn.Sequential) and len(part) > 0):
        return _NOT_STAGES[precision]
    gate = _GATES[precision][name]
    if gate is None:
        return None
    with torch.set_grad_enabled(precision == "fp32" or torch.is_grad_enabled()):
        return importlib.import_module("..functions." + gate, __package__).native_reason(part, x)


def _chain_reason(net, precision, example_inputs=None):
    """None, or "<part>: <reason>" for the first part of `net`, a DetectionTail / DetectionTrunk / DetectionNet, that
    `_part_reason` refuses, asked in `_ORDER[precision]`.  example_inputs None: the modules alone are judged; else the fp32
    stem is also judged on the image the capture will see (example_inputs[0]) -- one that requires grad, lives on the CPU or
    is not float32 contiguous would silently put the stem back on the framework's backward."""
    for name in _ORDER[precision]:
        if name != "heads" and name not in net.PARTS:
            continue
        part = net.head_modules() if name == "heads" else getattr(net, name)
        why = _part_reason(precision, name, part)
        if (precision, name) == ("fp32", "layer0"):
            if why is None and example_inputs is not None:
                why = _part_reason(precision, name, part, example_inputs[0]) if example_inputs else "no example image to judge"
            if why is not None and isinstance(part, nn.Sequential) and len(part) and type(part[0]) is nn.Conv2d:
                why = "the fp32 stem: " + why      # (a quantised stem keeps the gate's words alone)
        if why is not None:
            return "%s: %s" % (name, why)
    return None


def _is_stack(net, precision):
    """True for a stage stack of `precision`: a sequence that `_part_reason` accepts as `deconv_layers`, in a container whose
    forward runs it through functions/codenet_stage.forward_stage_blocks.  QAT: the Sequential itself, or a module whose
    only child it is.  fp32: a pipeline.DeconvLayers with its own forward whose only child it is -- a bare Sequential, or
    another container, runs ``Sequential.forward``: the framework's BatchNorm under autograd."""
    from .common import DeconvLayers
    seq = getattr(net, "deconv_layers", net)
    if _part_reason(precision, "deconv_layers", seq) is not None:
        return False
    only_child = [m for m in net.children()] == [seq]
    if precision == "qat":
        return seq is net or only_child
    return isinstance(net, DeconvLayers) and type(net).forward is DeconvLayers.forward and only_child


def _accepts(scope, net, example_inputs=None):
    """Whether `net` is in `scope`, a row of SCOPES."""
    if scope.chain is None:
        return _is_stack(net, scope.precision)
    return isinstance(net, scope.chain) and _chain_reason(net, scope.precision, example_inputs) is None


def _refusal(net, example_inputs):
    """The constructor's error for a `net` outside every scope: the scopes, each chain scope of the class of `net` with the
    reason why `net` is outside it."""
    scopes = ["%s [%s]" % (s.words, _chain_reason(net, s.precision, example_inputs))
              if s.chain is not None and isinstance(net, s.chain) else s.words for s in SCOPES]
    return ("GraphedTrainStep is validated (bit-identical replays) only for: %s. `net` holds other modules, whose "
            "PyTorch-ROCm kernels under autograd are not run-to-run deterministic. Pass unvalidated=True to capture it "
            "anyway (see the class docstring for what was measured)." % "; ".join(scopes))


class GraphedTrainStep:
    """One training step -- forward, loss, backward, optimizer -- over static input buffers as ONE HIP graph.

    The reference's training loop (quant_main.py -> lib/trains/base_trainer.py:51-80) launches eagerly; the QAT step of
    the three deform stages is 61 kernels of 4-130 us, so eager launches are host-bound (1.4-1.9 ms per step against
    1.05 ms of GPU work).  Captured once, the step replays without the host in the loop.  Every
    sum of the step has a fixed order (section 4.3), so a replayed step is bit-identical to the eager one.

        opt = torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device=dev), capturable=True)
        step = GraphedTrainStep(net, opt, loss_fn, example_inputs)                  # loss_fn(net, *inputs) -> scalar
        for batch in loader:
            loss = step(*batch)           # copies the batch into the static buffers, replays; loss: a static tensor
            step.set_lr(schedule(it))     # (a learning rate held as a Python float is a constant of the graph)

    Shapes are fixed at capture; QuantAct running ranges, BatchNorm buffers and the optimizer state advance in place
    exactly as in the eager loop.  `warmup` eager steps run first on a side stream (they DO train: allocator and lazily
    derived tensors settle before capture); the capture records on that same stream.

    SCOPE.  Validated -- and accepted without `unvalidated=True` -- are the rows of `SCOPES` in this module: in each, every
    kernel of the step is this library's and every sum has one order, and the test file named shows the replays (of a chain:
    with the native criterion) bit-identical to the eager steps.  `scope_of` names the row of a net; `step.scope` keeps it.
      `is_stage_stack`: the quantised deform stages, ``pipeline.build_hot_path()`` / a quantised ``deconv_layers``; tests/test_train_step.py
      `is_fp32_stage_stack`: the fp32 stack of main.py, ``pipeline.build_hot_path(quantized=False)`` (section 4.3e); tests/test_gpu_bn_block.py
      `is_native_tail`: ``pipeline.DetectionTail(model)``, quantised: those stages and the heads (4.3b); tests/test_gpu_heads_train.py
      `is_native_trunk`: ``pipeline.DetectionTrunk(model)``, quantised: layers 1-4 in front of that tail (4.3c); tests/test_gpu_units_train.py
      `is_native_net`: ``pipeline.DetectionNet(model)``, quantised: the stem in front of that trunk (4.3d); tests/test_gpu_stem_train.py
      `is_fp32_tail`: the fp32 tail, ``pipeline.DetectionTail(model)`` of an fp32 model (4.3f); tests/test_gpu_heads_fp32.py
      `is_fp32_trunk`: the fp32 trunk, ``pipeline.DetectionTrunk(model)`` of an fp32 model (4.3g); tests/test_gpu_units_fp32.py
      `is_fp32_net`: the fp32 network, ``pipeline.DetectionNet(model)`` of an fp32 model and an example image its stem accepts (4.3h); tests/test_gpu_stem_fp32.py
    What each part must be is the `native_reason` of the functions/ module that runs it (`_GATES`); BatchNorms may be in
    training or eval mode.  test_graphed_train_step_* also show replays of the first row bit-identical from a restored state
    whatever else the process does in between (a second model built before the capture taking its first eager steps, another
    framework model training, the allocator's free memory filled with NaN).
    A network that also runs PyTorch-ROCm operators under autograd (a bare harness.PoseShuffleNetV2, whose forward
    dispatches on inference schedules the capture was never validated for -- wrap it in DetectionNet --, an fp32 or
    percentile stem, heads or units, NATIVE_STEM / NATIVE_HEADS / NATIVE_UNITS off) needs `unvalidated=True`; what was measured for it (tools/experiments/gts_probe*.py):
      * parameters and gradients of a replay agree with any other replay FROM THE SAME STATE to ~1e-6 of their magnitude --
        with or without other work in between.  That residue is the framework's own backward (atomics), present in two
        eager runs too; after a quantiser amplifies it the loss trajectories of two runs part ways in the fifth digit by
        the second step.  This -- not memory corruption -- is what round 5 recorded as "wrong losses after a second model's
        first steps": poisoning every free byte of the allocator with NaN between replays changes nothing;
      * the scalar LOSS a replay returns can be stale in one situation: loss_fn reduces a large tensor with one
        ``mean()`` / ``sum()`` (ATen's multi-block reduction: a semaphore word zeroed by a memset node), and another model
        takes its FIRST eager step between two replays -- that replay's reduction leaves its output unwritten while the
        gradients and parameters of the same replay are right (the backward of a mean does not read its value).  A
        two-level reduction (``v.square().reshape(-1, 64).sum(1).sum() / v.numel()``: no semaphore) does not show it, and neither does the native criterion
        (``codenet_amd.losses.CtdetLoss``: its sums are fixed-order slabs of this library's own kernels)."""

    def __init__(self, net, optimizer, loss_fn, example_inputs, warmup=3, unvalidated=False):
        self.scope = self.scope_of(net, example_inputs or ())      # (None: only `unvalidated=True` lets it through)
        if self.scope is None and not unvalidated:
            raise NotImplementedError(_refusal(net, example_inputs or ()))
        self.static = [t.detach().clone() for t in example_inputs]
        for t, src in zip(self.static, example_inputs):
            t.requires_grad_(src.requires_grad)
        self._net, self._opt, self._loss_fn = net, optimizer, loss_fn
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(int(warmup), 1)):
                self.eager_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        # capture ON the warm-up stream: the autograd nodes of the parameters were created there, and a capture stream of
        # its own makes every gradient accumulation a cross-stream branch of the graph (the framework warns about it)
        with torch.cuda.graph(self.graph, stream=side):
            self.loss = loss_fn(net, *self.static)
            self.loss.backward()
            optimizer.step()

    @staticmethod
    def scope_of(net, example_inputs=None):
        """The name of the row of `SCOPES` that accepts `net`, or None.  example_inputs None: the modules alone are judged;
        else, as the constructor does, the fp32 stem also judges example_inputs[0], the image the capture will see."""
        return next((s.name for s in SCOPES if _accepts(s, net, example_inputs)), None)

    # The public predicates: one view each of a row of SCOPES, the modules alone.

    @staticmethod
    def is_stage_stack(net):
        """SCOPES row "stage stack": classes and container only, whatever the grad mode."""
        return _accepts(_ROW["is_stage_stack"], net)

    @staticmethod
    def is_fp32_stage_stack(net):
        """SCOPES row "fp32 stack": a property of the modules, whatever the caller's grad mode."""
        return _accepts(_ROW["is_fp32_stage_stack"], net)

    @staticmethod
    def is_native_tail(net):
        """SCOPES row "QAT tail": False under no_grad, as its gates are."""
        return _accepts(_ROW["is_native_tail"], net)

    @staticmethod
    def is_native_trunk(net):
        """SCOPES row "QAT trunk": False under no_grad, as its gates are."""
        return _accepts(_ROW["is_native_trunk"], net)

    @staticmethod
    def is_native_net(net):
        """SCOPES row "QAT net": False under no_grad, as its gates are."""
        return _accepts(_ROW["is_native_net"], net)

    @staticmethod
    def is_fp32_tail(net):
        """SCOPES row "fp32 tail": a property of the modules, whatever the caller's grad mode."""
        return _accepts(_ROW["is_fp32_tail"], net)

    @staticmethod
    def is_fp32_trunk(net):
        """SCOPES row "fp32 trunk": a property of the modules, whatever the caller's grad mode."""
        return _accepts(_ROW["is_fp32_trunk"], net)

    @staticmethod
    def is_fp32_net(net):
        """SCOPES row "fp32 net", the modules alone: the constructor and `scope_of` also judge the example image."""
        return _accepts(_ROW["is_fp32_net"], net)

    def set_lr(self, value, group=None):
        """Write a new learning rate where the captured step reads it: the param group's lr must be a device TENSOR
        (torch.optim with capturable=True accepts one).  A Python float was baked into the graph at capture -- a scheduler
        that assigns ``group['lr'] = float`` changes nothing on replay -- so that case raises instead of silently ignoring."""
        groups = self._opt.param_groups if group is None else [self._opt.param_groups[group]]
        for g in groups:
            if not torch.is_tensor(g["lr"]):
                raise RuntimeError("GraphedTrainStep.set_lr: this optimizer holds its learning rate as a Python float, which "
                                   "the captured graph holds as a constant; construct the optimizer with "
                                   "lr=torch.tensor(value, device=...) (capturable=True) before the capture")
            with torch.no_grad():
                g["lr"].fill_(float(value))

    def eager_step(self):
        """The same step with eager launches (what the capture records), on the static buffers."""
        self._opt.zero_grad(set_to_none=True)
        loss = self._loss_fn(self._net, *self.static)
        loss.backward()
        self._opt.step()
        return loss

    def __call__(self, *inputs):
        if len(inputs) != len(self.static):
            raise ValueError("GraphedTrainStep: %d inputs, captured with %d" % (len(inputs), len(self.static)))
        with torch.no_grad():
            for dst, src in zip(self.static, inputs):
                if dst.shape != src.shape:
                    raise ValueError("GraphedTrainStep: input shape %s, captured with %s" % (tuple(src.shape), tuple(dst.shape)))
                dst.copy_(src, non_blocking=True)
        self.graph.replay()
        return self.loss
