"""GraphedTrainStep: the QAT step of the deform-stage stack -- or of the detection tail, stages + heads, or of the trunk,
layers 1-4 in front of that tail, or of the whole network from the image -- as one HIP graph.

Part of codenet_amd.pipeline (split by concern in round 6; `from codenet_amd import pipeline` exposes every name as
before)."""
import os

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


def _outside_scope(net):
    """None, or the reason why `net`, a DetectionTail / DetectionTrunk / DetectionNet, is outside the validated scope: its
    stages are not the blocks above, or a part it holds is refused by the gate of the functions/ module that runs it.  (The
    gates see the caller's grad mode: under no_grad every one refuses, so the predicates built on this are False there.)"""
    from ..functions import codenet_heads, codenet_stem, codenet_units
    if not _stage_blocks_ok(net.deconv_layers):
        return "deconv_layers: not a Sequential of [quantised deform stage, Sequential(ReLU, QuantAct), Upsample] blocks"
    gated = [("heads", codenet_heads, net.head_modules())]
    gated += [(name, codenet_units, getattr(net, name)) for name in net.PARTS if name in ("layer1", "layer2", "layer3", "layer4")]
    gated += [(name, codenet_stem, getattr(net, name)) for name in net.PARTS if name == "layer0"]
    for name, gate, part in gated:
        why = gate.native_reason(part, None)
        if why is not None:
            return "%s: %s" % (name, why)
    return None


def _fp32_tail_outside_scope(net):
    """None, or the reason why `net`, a DetectionTail, is not the fp32 tail GraphedTrainStep.is_fp32_tail accepts."""
    from ..functions import codenet_bn, codenet_heads_fp32
    seq = net.deconv_layers
    if not isinstance(seq, nn.Sequential) or len(seq) == 0:
        return "deconv_layers: not a Sequential of [deform stage, BatchNorm2d, ReLU, Upsample] blocks"
    with torch.enable_grad():      # (a property of the modules, as is_fp32_stage_stack)
        why = codenet_bn.native_reason(seq, None)
        if why is not None:
            return "deconv_layers: %s" % why
        why = codenet_heads_fp32.native_reason(net.head_modules(), None)
    return "heads: %s" % why if why is not None else None


def _fp32_trunk_outside_scope(net):
    """None, or the reason why `net`, a DetectionTrunk, is not the fp32 trunk GraphedTrainStep.is_fp32_trunk accepts: layers
    1-4 that functions/codenet_units_fp32 refuses, or a tail that `_fp32_tail_outside_scope` refuses."""
    from ..functions import codenet_units_fp32
    with torch.enable_grad():      # (a property of the modules, as is_fp32_tail)
        for name in ("layer1", "layer2", "layer3", "layer4"):
            why = codenet_units_fp32.native_reason(getattr(net, name), None)
            if why is not None:
                return "%s: %s" % (name, why)
    return _fp32_tail_outside_scope(net)


def _fp32_stem_reason(net, example_inputs):
    """None, or the reason why the fp32 stem of `net`, a DetectionNet, would not run natively on the example image: the gate
    of functions/codenet_stem_fp32 on the modules AND on the image the capture will see -- an image that requires grad,
    lives on the CPU or is not float32 contiguous would silently put the stem back on the framework's backward."""
    from ..functions import codenet_stem_fp32
    with torch.enable_grad():
        why = codenet_stem_fp32.native_reason(net.layer0, None)
        if why is not None:
            return why
        if not example_inputs:
            return "no example image to judge"
        return codenet_stem_fp32.native_reason(net.layer0, example_inputs[0])


def _fp32_net_outside_scope(net):
    """None, or the reason why `net`, a DetectionNet, is not the fp32 network GraphedTrainStep.is_fp32_net accepts: a stem
    that functions/codenet_stem_fp32 refuses, or a trunk that `_fp32_trunk_outside_scope` refuses."""
    from ..functions import codenet_stem_fp32
    with torch.enable_grad():      # (a property of the modules, as is_fp32_trunk)
        why = codenet_stem_fp32.native_reason(net.layer0, None)
    return "layer0: %s" % why if why is not None else _fp32_trunk_outside_scope(net)


def _fp32_net_reason(net, example_inputs):
    """The bracket of the constructor's error for `net`, a DetectionNet: for an fp32 stem (its first module is a Conv2d) what
    the stem's gate says about the modules and the example image, behind "layer0: the fp32 stem: "; where the stem is
    accepted, or is no fp32 stem at all, the reason of `_fp32_net_outside_scope` (the trunk's, or the stem's structure)."""
    l0 = net.layer0
    if isinstance(l0, nn.Sequential) and len(l0) and type(l0[0]) is nn.Conv2d:
        why = _fp32_stem_reason(net, example_inputs)
        if why is not None:
            return "layer0: the fp32 stem: %s" % why
    return _fp32_net_outside_scope(net)


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

    SCOPE.  Validated -- and accepted without `unvalidated=True` -- are (1) the stack of deform stages
    (``pipeline.build_hot_path`` / a quantised ``deconv_layers``, `is_stage_stack`) and (2) the detection tail,
    ``pipeline.DetectionTail(model)`` of a quantised model whose heads run on functions/codenet_heads.py
    (`is_native_tail`), and (3) the trunk, ``pipeline.DetectionTrunk(model)`` -- layers 1-4 of the backbone in front of
    that tail, from layer0's output -- of a quantised model whose units run on functions/codenet_units.py
    (`is_native_trunk`), and (4) the whole network, ``pipeline.DetectionNet(model)`` -- the stem in front of that trunk,
    from the image -- of a quantised model whose stem runs on functions/codenet_stem.py (`is_native_net`): every kernel of
    those steps is this library's, every sum has one order; and (5) the fp32 stack of the reference's main.py --
    ``pipeline.build_hot_path(quantized=False)``: a ``pipeline.DeconvLayers`` (its forward is forward_stage_blocks) of
    [deform stage, BatchNorm2d, ReLU, Upsample] blocks, BatchNorm in training or eval mode (`is_fp32_stage_stack`; functions/codenet_bn.py, DESIGN.md section 4.3e;
    tests/test_gpu_bn_block.py shows its replays bit-identical to the eager step); and (6) the fp32 tail,
    ``pipeline.DetectionTail(model)`` of an fp32 model: those blocks in front of the fp32 detection heads [Conv2d 1x1,
    BatchNorm2d, ReLU, depthwise Conv2d 3x3, BatchNorm2d, ReLU, Conv2d 1x1] on functions/codenet_heads_fp32.py, every
    BatchNorm in training or eval mode (`is_fp32_tail`; tests/test_gpu_heads_fp32.py shows its
    replays with the native criterion bit-identical to the eager steps); and (7) the fp32 trunk,
    ``pipeline.DetectionTrunk(model)`` of an fp32 model: layers 1-3 of ``harness.BaseNode`` units and layer4 [Conv2d 1x1,
    BatchNorm2d, ReLU] on functions/codenet_units_fp32.py in front of that tail, from layer0's output, every BatchNorm in
    training or eval mode (`is_fp32_trunk`; tests/test_gpu_units_fp32.py shows its replays with the
    native criterion bit-identical to the eager steps); and (8) the fp32 network, ``pipeline.DetectionNet(model)`` of an fp32
    model: the stem [Conv2d 3 -> 24, BatchNorm2d, ReLU(, MaxPool2d(3, 2, 1))] on functions/codenet_stem_fp32.py in front of
    that trunk, from the image, every BatchNorm in training or eval mode (`is_fp32_net`; DESIGN.md section 4.3h;
    tests/test_gpu_stem_fp32.py shows its replays with the native criterion bit-identical to the eager steps) -- accepted
    when the gate also accepts the example image (a float32, contiguous GPU image that does not require grad): main.py's
    whole step, image -> loss -> optimizer, is then one chain of this library's kernels.
    tests/test_train_step.py::test_graphed_train_step_* show replays of (1) bit-identical to the eager step and
    bit-identical from a restored state whatever else the process does in between (a second model built before the capture
    taking its first eager steps, another framework model training, the allocator's free memory filled with NaN);
    tests/test_gpu_heads_train.py shows replays of (2) with the native criterion bit-identical to the eager steps,
    tests/test_gpu_units_train.py those of (3), tests/test_gpu_stem_train.py those of (4).
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
        if not unvalidated and not self.is_stage_stack(net) and not self.is_fp32_stage_stack(net) \
                and not self.is_native_tail(net) and not self.is_native_trunk(net) and not self.is_native_net(net) \
                and not self.is_fp32_tail(net) and not self.is_fp32_trunk(net) \
                and not (self.is_fp32_net(net) and _fp32_stem_reason(net, example_inputs) is None):
            raise NotImplementedError(
                "GraphedTrainStep is validated (bit-identical replays) for a stack of quantised deform stages, for the "
                "fp32 stack (a pipeline.DeconvLayers of [deform stage, BatchNorm2d, ReLU, Upsample] blocks on functions/codenet_bn), for a "
                "pipeline.DetectionTail whose heads run natively, for a pipeline.DetectionTrunk whose units run "
                "natively and for a pipeline.DetectionNet whose stem runs natively only; `net` "
                "holds other modules, whose PyTorch-ROCm kernels under autograd are not run-to-run deterministic. Pass "
                "unvalidated=True to capture it anyway (see the class docstring for what was measured)."
                + (" [%s]" % _outside_scope(net) if isinstance(net, _DetectionChain) else "")
                + " Also validated: the fp32 tail, a pipeline.DetectionTail of an fp32 model whose [deform stage, BatchNorm2d, "
                "ReLU, Upsample] blocks run on functions/codenet_bn and whose heads run on functions/codenet_heads_fp32"
                + (" [%s]" % _fp32_tail_outside_scope(net) if isinstance(net, DetectionTail) else "")
                + ", and the fp32 trunk, a pipeline.DetectionTrunk of an fp32 model whose layers 1-4 also run on "
                "functions/codenet_units_fp32"
                + (" [%s]" % _fp32_trunk_outside_scope(net) if isinstance(net, DetectionTrunk) else "")
                + ", and the fp32 network, a pipeline.DetectionNet of an fp32 model whose stem also runs on "
                "functions/codenet_stem_fp32 for the example image"
                + (" [%s]" % _fp32_net_reason(net, example_inputs) if isinstance(net, DetectionNet) else "") + ".")
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
    def is_stage_stack(net):
        """True for a (container of one) Sequential of [quantised deform stage, Sequential(ReLU, QuantAct), Upsample]
        blocks -- what functions/codenet_stage.forward_stage_blocks runs natively and the bit-level tests cover."""
        seq = getattr(net, "deconv_layers", net)
        return _stage_blocks_ok(seq) and (seq is net or [m for m in net.children()] == [seq])

    @staticmethod
    def is_fp32_stage_stack(net):
        """True for a pipeline.DeconvLayers -- the container whose forward IS functions/codenet_stage.forward_stage_blocks --
        of fp32 blocks [DeformConvWithOffsetScaleBoundPositive, BatchNorm2d, ReLU, Upsample(x2, nearest)] that
        functions/codenet_bn runs natively (native_reason(seq, None) is None: affine BatchNorms that track running statistics
        with a float momentum, no hooks, NATIVE_FP32_BLOCKS on), BatchNorm in training or eval mode: the stage stack of the
        reference's main.py.  A bare ``nn.Sequential`` of such blocks, or another container around it, is refused: calling it
        runs ``Sequential.forward``, the framework's BatchNorm under autograd, which this scope does not cover."""
        from ..functions.codenet_bn import native_reason
        from .common import DeconvLayers
        if not isinstance(net, DeconvLayers) or type(net).forward is not DeconvLayers.forward:
            return False
        seq = net.deconv_layers
        if not isinstance(seq, nn.Sequential) or len(seq) == 0 or [m for m in net.children()] != [seq]:
            return False
        with torch.enable_grad():
            return native_reason(seq, None) is None

    @staticmethod
    def is_fp32_tail(net):
        """True for a pipeline.DetectionTail of an fp32 model: ``deconv_layers`` a Sequential of the blocks
        `is_fp32_stage_stack` describes (functions/codenet_bn.native_reason(seq, None) is None) and heads that
        functions/codenet_heads_fp32 runs natively (native_reason(heads, None) is None: the seven-module Sequential of
        shufflenetv2_dcn.py:246-258 with affine BatchNorms that track running statistics with a float momentum, one hidden
        width, no hooks, NATIVE_FP32_HEADS on), every BatchNorm in training or eval mode.  A property of the modules: the
        caller's grad mode does not change the answer.  `is_native_tail` stays False for it."""
        return isinstance(net, DetectionTail) and _fp32_tail_outside_scope(net) is None

    @staticmethod
    def is_fp32_trunk(net):
        """True for a pipeline.DetectionTrunk of an fp32 model: a tail that `is_fp32_tail` would accept (the same stages and
        heads) behind layers 1-3 and layer4 that functions/codenet_units_fp32 runs natively (native_reason(layer, None) is
        None: exactly ``harness.BaseNode`` units of nn.Conv2d / nn.BatchNorm2d in the reference's geometry and layer4 =
        [Conv2d 1x1, BatchNorm2d, ReLU], no conv bias, affine BatchNorms that track running statistics with a float
        momentum, no hooks, NATIVE_FP32_UNITS on), every BatchNorm in training or eval mode.  A property of the modules: the
        caller's grad mode does not change the answer.  `is_native_trunk` stays False for it."""
        return isinstance(net, DetectionTrunk) and _fp32_trunk_outside_scope(net) is None

    @staticmethod
    def is_fp32_net(net):
        """True for a pipeline.DetectionNet of an fp32 model: a trunk that `is_fp32_trunk` would accept (the same layers 1-4,
        stages and heads) behind a stem that functions/codenet_stem_fp32 runs natively (native_reason(layer0, None) is None:
        exactly Sequential(Conv2d 3 -> 24 3x3 without bias, BatchNorm2d, ReLU[, MaxPool2d(3, 2, 1)]) at stride 2 with the pool
        or 4 without, an affine BatchNorm that tracks running statistics with a float momentum, no hooks, NATIVE_FP32_STEM
        on).  A property of the modules: the caller's grad mode does not change the answer.  The constructor also judges the
        example image (`_fp32_stem_reason`).  `is_native_net` stays False for it."""
        return isinstance(net, DetectionNet) and _fp32_net_outside_scope(net) is None

    @staticmethod
    def is_native_tail(net):
        """True for a pipeline.DetectionTail whose stages are the blocks `is_stage_stack` accepts and whose heads
        functions/codenet_heads.forward_heads runs natively (native_reason(heads, None) is None: quantised heads with
        the default QuantAct settings, no hooks, NATIVE_HEADS on) -- stages, heads and, with losses.CtdetLoss, the
        criterion are then one chain of this library's kernels."""
        return isinstance(net, DetectionTail) and _outside_scope(net) is None

    @staticmethod
    def is_native_trunk(net):
        """True for a pipeline.DetectionTrunk whose stages and heads are what `is_native_tail` accepts and whose layers 1-3
        and layer4 functions/codenet_units runs natively (native_reason(layer, None) is None: QuantBaseNode units with the
        default QuantAct settings, no hooks, NATIVE_UNITS on)."""
        return isinstance(net, DetectionTrunk) and _outside_scope(net) is None

    @staticmethod
    def is_native_net(net):
        """True for a pipeline.DetectionNet whose layers 1-4, stages and heads are what `is_native_trunk` accepts and whose
        stem functions/codenet_stem runs natively (native_reason(layer0, None) is None: the quantised 3 -> 24 stem with the
        default QuantAct settings, no hooks, NATIVE_STEM on) -- image -> loss -> optimizer is then one chain of this
        library's kernels."""
        return isinstance(net, DetectionNet) and _outside_scope(net) is None

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
