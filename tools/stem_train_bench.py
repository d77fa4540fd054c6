"""Timing of the quantised stem in the QAT step (codenet_stem_train.hip through codenet_amd.functions.codenet_stem):
forward + backward of layer0 including its weight preparation at the QAT shape, x = [32, 3, 512, 512].  HIP events, one
process, after warm-up:

  (a) native: CodenetStemFunction (NATIVE_STEM = True)      (b) the module path under the framework's autograd
      timed in INTERLEAVED regions (a, b, a, b, ...) so that clock and temperature drift hit both alike.

Both include the weight preparation (fold + 8-bit fake-quantisation, native either way) and the gradients of every parameter;
neither builds a gradient for the image.  Prints one JSON line: the medians, min / max, the ratio, whether (a) < (b) held in
every pair, and the native path's algorithmic HBM bytes divided by its time.  The byte count, pass by pass (float32; weights,
biases, partials and the 8-word state are left out: kilobytes).  I = N 3 H W 4 bytes (the image), Y = N 24 Ho Wo 4 (y0),
O = N 24 Hp Wp 4 (the pooled output, Y / 4):

  stride 4:            forward   conv reads the image, writes y0                       I + Y
                                 quantise reads y0, writes out                         2 Y
                       backward  reads grad_out, y0 and the image                      2 Y + I              = 2 I + 5 Y
  stride 2 + MaxPool:  forward   conv                                                  I + Y
                                 pool reads y0, writes out                             Y + O
                       backward  pool backward reads grad_out and y0, writes gy0       O + 2 Y
                                 reads gy0 and the image                               Y + I                = 2 I + 5 Y + 2 O

--maxpool: the "S2 + MaxPool" stem.  --step: the captured step of pipeline.DetectionNet (stem, layers 1-4, stages, heads,
CtdetLoss, fused Adam) instead.  GPU only."""
import json
import sys

import torch

import qat_bench
from codenet_amd import harness
from codenet_amd.functions import codenet_stem as ST


def algorithmic_bytes(layer0, N, H, W):
    """Bytes the native path has to move through the stem for the image [N, 3, H, W] (see the module docstring)."""
    s = layer0[0].conv.stride[0]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    I, Y = 4 * N * 3 * H * W, 4 * N * 24 * Ho * Wo
    if len(layer0[1]) == 2:
        return 2 * I + 5 * Y
    return 2 * I + 5 * Y + 2 * (4 * N * 24 * ((Ho - 1) // 2 + 1) * ((Wo - 1) // 2 + 1))


def main(maxpool=False, regions=30, warm=3, N=32, R=512):
    model = qat_bench.bn_eval(harness.create_model(quantize=True, maxpool=maxpool).cuda().train())
    layer0 = model.layer0
    params = list(layer0.parameters())
    g = torch.Generator().manual_seed(1)
    x = (torch.randint(0, 256, (N, 3, R, R), generator=g).float() / 64 - 2).cuda()
    assert ST.native_reason(layer0, x) is None, ST.native_reason(layer0, x)
    with torch.no_grad():
        shape = layer0(x).shape
    gy = torch.randn(tuple(shape), generator=g).cuda()

    def step(native):
        ST.NATIVE_STEM = native
        for p in params:
            p.grad = None
        ST.forward_stem(layer0, x).backward(gy)

    ms = qat_bench.interleaved_ab(step, lambda: setattr(ST, "NATIVE_STEM", True), regions, warm)
    res = {"shape": "x=[%d,3,%d,%d] layer0%s" % (N, R, R, " (stride 2 + MaxPool)" if maxpool else " (stride 4)"),
           **qat_bench.report(*ms, algorithmic_bytes(layer0, N, R, R))}
    print(json.dumps(res))
    return res


def net_step(maxpool=False, batch=32, res=512, steps=20):
    """--step: the captured QAT step of the whole network -- stem, layers 1-4, deform stages, heads, losses.CtdetLoss, fused
    Adam -- as pipeline.GraphedTrainStep accepts it without `unvalidated`, timed over `steps` replays (wall clock around the
    replays, as tools/units_train_bench.py --step times the trunk's)."""
    from codenet_amd import pipeline
    net = qat_bench.bn_eval(pipeline.DetectionNet(harness.create_model(quantize=True, maxpool=maxpool)).cuda().train())
    g = torch.Generator().manual_seed(1)
    img = (torch.randint(0, 256, (batch, 3, res, res), generator=g).float() / 64 - 2).cuda()
    return qat_bench.captured_step(net, img, "CoDeNet1x %dx%d W4A8 QAT step over the whole network%s (layer0-4 + deconv_layers + "
                                   "heads + CtdetLoss), batch %d, one HIP graph" % (
                                       res, res, " (S2 + MaxPool stem)" if maxpool else "", batch), res, steps)


if __name__ == "__main__":
    pool = "--maxpool" in sys.argv[1:]
    if "--step" in sys.argv[1:]:
        net_step(pool)
    else:
        main(pool)
