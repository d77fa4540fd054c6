"""Timing of the quantised detection heads in the QAT step (codenet_heads_train.hip through
codenet_amd.functions.codenet_heads): forward + backward of the three heads (hm 20, wh 2, reg 2) at the QAT shape,
x = [32, 64, 128, 128].  HIP events, one process, after warm-up:

  (a) native: CodenetHeadsFunction (NATIVE_HEADS = True)      (b) the module path under the framework's autograd
      timed in INTERLEAVED regions (a, b, a, b, ...) so that clock and temperature drift hit both alike.

Both include the weight preparation (fold + fake-quantisation, native either way) and the gradients of x and of every
parameter.  Prints one JSON line: the medians, min / max, the ratio, whether (a) < (b) held in every pair, and the native path's
algorithmic HBM bytes -- every pass over a [N, 64, H, W] tensor it has to make, plus the thin y3 / grad_y3 -- divided by
its time.  --step: the captured step of the whole detection tail instead (see tail_step).  GPU only."""
import json
import sys

import torch

import qat_bench
from codenet_amd import harness
from codenet_amd.functions import codenet_heads as CH


def algorithmic_bytes(N, C, HW, couts):
    """Bytes the native path has to move: T = one pass over a [N, C, HW] float32 tensor.
    forward, per head:  x -> y1 (2 T), y1 -> r2 (2 T), r2 -> y3 (T + y3)
    backward, per head: grad_W3q reads r2 and grad_y3 (T + g); Co > 4: grad_a2 written (T + g); the depthwise backward
                        reads grad_a2 (T; Co <= 4: grad_y3 instead), r2, y1 and writes grad_y1 (3 T)
    backward, once:     grad_W1q reads grad_y1 of all heads and x ((heads + 1) T); grad_x reads grad_y1 again and is
                        written ((heads + 1) T)"""
    T = N * C * HW * 4
    total = 0
    for co in couts:
        thin = N * co * HW * 4
        total += 5 * T + thin                       # forward
        total += T + thin                           # grad_W3q / grad_b3
        total += (2 * T + thin) if co > 4 else thin      # grad_a2 written and read back / grad_y3 read in its place
        total += 3 * T                              # r2, y1 read, grad_y1 written
    total += 2 * (len(couts) + 1) * T
    return total


def main(regions=40, warm=3, N=32, R=128):
    model = harness.create_model(quantize=True).cuda().train()
    heads = {h: getattr(model, h) for h in model.heads}
    params = [p for m in heads.values() for p in m.parameters()]
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(N, 64, R, R, generator=g) * 4).cuda().requires_grad_(True)
    gys = [torch.randn(N, c, R, R, generator=g).cuda() for c in model.heads.values()]
    assert CH.native_reason(heads, x) is None, CH.native_reason(heads, x)

    def step(native):
        CH.NATIVE_HEADS = native
        x.grad = None
        for p in params:
            p.grad = None
        out = CH.forward_heads(heads, x)
        torch.autograd.backward([out[h] for h in heads], gys)

    ms = qat_bench.interleaved_ab(step, lambda: setattr(CH, "NATIVE_HEADS", True), regions, warm)
    res = {"shape": "x=[%d,64,%d,%d] heads=%s" % (N, R, R, dict(model.heads)),
           **qat_bench.report(*ms, algorithmic_bytes(N, 64, R * R, list(model.heads.values())))}
    print(json.dumps(res))
    return res


def tail_step(batch=32, res=512, steps=20):
    """--step: the captured QAT step of the detection tail -- deform stages, heads, losses.CtdetLoss, fused Adam -- as
    pipeline.GraphedTrainStep accepts it without `unvalidated`, timed over `steps` replays (wall clock around the
    replays, as tools/train_step_bench.py times cfg5's step over the stages alone)."""
    from codenet_amd import pipeline
    net = qat_bench.bn_eval(pipeline.DetectionTail(harness.create_model(quantize=True)).cuda().train())
    feat = pipeline.make_input(batch, res, device="cuda").requires_grad_(True)      # (as cfg5: the backbone would need it)
    return qat_bench.captured_step(net, feat, "CoDeNet1x %dx%d W4A8 QAT step over deconv_layers + heads + CtdetLoss, batch %d, "
                                   "one HIP graph" % (res, res, batch), res, steps)


if __name__ == "__main__":
    if "--step" in sys.argv[1:]:
        tail_step()
    else:
        main()
