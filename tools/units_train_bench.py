"""Timing of the quantised ShuffleNetV2 units and layer4 in the QAT step (codenet_units_train.hip through
codenet_amd.functions.codenet_units): forward + backward of layers 1-4 (16 units + the 1x1 layer4) from layer0's output at
the QAT shape, x = [32, 24, 128, 128].  HIP events, one process, after warm-up:

  (a) native: CodenetUnitFunction per unit (NATIVE_UNITS = True)      (b) the module path under the framework's autograd
      timed in INTERLEAVED regions (a, b, a, b, ...) so that clock and temperature drift hit both alike.

Both include the weight preparation (fold + fake-quantisation, native either way) and the gradients of x and of every
parameter.  Prints one JSON line: the medians, min / max, the ratio, whether (a) < (b) held in every pair, and the native path's
algorithmic HBM bytes divided by its time.  The byte count, pass by pass (float32; weights, biases and partials are left
out: kilobytes).  With P = N h HW 4 bytes (one pass over half a unit's tensor at its INPUT plane), Po the same at its output
plane, X / Xo one pass over the whole input x [N, Cx] at the input / output plane:

  stride-1 unit (input and output plane are the same, Po = P):
    forward    pw1 reads x[:, h:], writes y1                               2 P
               dw2 reads y1, writes y2                                     2 P
               pw3 reads y2, writes y3                                     2 P
               join reads y3 and x[:, :h], writes out                      4 P
    backward   join reads grad_out and y3, writes grad_y3 and grad_x[:, :h] 5 P
               grad_W3q reads grad_y3 and y2                               2 P
               grad_y2 = W3q^T grad_y3: read, written                      2 P
               dw2 backward reads grad_y2 and y1, writes grad_y1           3 P
               grad_W1q reads grad_y1 and x[:, h:]                         2 P
               grad_x[:, h:] = W1q^T grad_y1: read, written                2 P        = 26 P
  stride-2 unit:
    forward    dw4 reads x, writes y4                                      X + Xo
               pw5 reads y4, writes y5                                     Xo + Po
               join (slot 0) reads y5, writes half of out                  2 Po
               pw1 reads x, writes y1                                      X + P
               dw2 reads y1, writes y2                                     P + Po
               pw3 reads y2, writes y3; join (slot 1)                      2 Po + 2 Po
    backward   the two joins read half of grad_out and y3 / y5, write grad_y3 / grad_y5       6 Po
               grad_W3q, grad_y2 (as above)                                4 Po
               dw2 backward reads grad_y2 and y1, writes grad_y1           Po + 2 P
               grad_W1q reads grad_y1 and x; grad_x written from grad_y1   2 P + 2 X
               grad_W5q reads grad_y5 and y4; grad_y4 written from grad_y5 2 Po + 2 Xo
               dw4 backward reads grad_y4 and x, adds into grad_x          Xo + 3 X
  layer4 (A = N 464 HW 4, B = N 1024 HW 4):
    forward    pointwise reads x, writes y; ReLU + QuantAct reads y, writes out               A + 3 B
    backward   ReLU backward 3 B; grad_W reads grad_y and x (A + B); grad_x read / written (A + B)

--step: the captured step of pipeline.DetectionTrunk (layers 1-4, stages, heads, CtdetLoss, fused Adam) instead.  GPU only."""
import json
import sys

import torch

import qat_bench
from codenet_amd import harness
from codenet_amd.functions import codenet_units as CU


def algorithmic_bytes(model, N, H, W):
    """Bytes the native path has to move through layers 1-4 for layer0's output [N, C, H, W] (see the module docstring)."""
    total = 0
    for name in ("layer1", "layer2", "layer3"):
        for node in getattr(model, name):
            h = node.quant_convbn1.conv.out_channels
            if node.stride == 1:
                total += 26 * N * h * H * W * 4
                continue
            Cx = node.quant_convbn1.conv.in_channels
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            P, Po, X, Xo = (4 * N * c * p for c, p in ((h, H * W), (h, Ho * Wo), (Cx, H * W), (Cx, Ho * Wo)))
            total += (X + Xo) + (Xo + Po) + 2 * Po + (X + P) + (P + Po) + 4 * Po                    # forward
            total += 6 * Po + 4 * Po + (Po + 2 * P) + (2 * P + 2 * X) + (2 * Po + 2 * Xo) + (Xo + 3 * X)      # backward
            H, W = Ho, Wo
    conv = model.layer4[0].conv
    A, B = 4 * N * conv.in_channels * H * W, 4 * N * conv.out_channels * H * W
    return total + (A + 3 * B) + (3 * B + 2 * (A + B))


def _layers(model, x):
    for layer in (model.layer1, model.layer2, model.layer3):
        x = CU.forward_units(layer, x)
    return CU.forward_layer4(model.layer4, x)


def main(regions=30, warm=3, N=32, R=128):
    model = qat_bench.bn_eval(harness.create_model(quantize=True).cuda().train())
    layers = [model.layer1, model.layer2, model.layer3, model.layer4]
    params = [p for m in layers for p in m.parameters()]
    g = torch.Generator().manual_seed(1)
    x = (torch.randint(0, 256, (N, 24, R, R), generator=g).float() / 64).cuda().requires_grad_(True)
    gy = torch.randn(N, model.layer4[0].conv.out_channels, R // 8, R // 8, generator=g).cuda()
    assert CU.native_reason(model.layer1, x) is None, CU.native_reason(model.layer1, x)

    def step(native):
        CU.NATIVE_UNITS = native
        x.grad = None
        for p in params:
            p.grad = None
        _layers(model, x).backward(gy)

    ms = qat_bench.interleaved_ab(step, lambda: setattr(CU, "NATIVE_UNITS", True), regions, warm)
    res = {"shape": "x=[%d,24,%d,%d] layers 1-4" % (N, R, R), **qat_bench.report(*ms, algorithmic_bytes(model, N, R, R))}
    print(json.dumps(res))
    return res


def trunk_step(batch=32, res=512, steps=20):
    """--step: the captured QAT step of the trunk -- layers 1-4, deform stages, heads, losses.CtdetLoss, fused Adam -- as
    pipeline.GraphedTrainStep accepts it without `unvalidated`, timed over `steps` replays (wall clock around the replays,
    as tools/heads_train_bench.py --step times the tail's)."""
    from codenet_amd import pipeline
    net = qat_bench.bn_eval(pipeline.DetectionTrunk(harness.create_model(quantize=True)).cuda().train())
    g = torch.Generator().manual_seed(1)
    R = res // 4
    feat0 = (torch.randint(0, 256, (batch, 24, R, R), generator=g).float() / 64).cuda().requires_grad_(True)      # (the stem would need it)
    return qat_bench.captured_step(net, feat0, "CoDeNet1x %dx%d W4A8 QAT step over layers 1-4 + deconv_layers + heads + "
                                   "CtdetLoss, batch %d, one HIP graph" % (res, res, batch), res, steps)


if __name__ == "__main__":
    if "--step" in sys.argv[1:]:
        trunk_step()
    else:
        main()
