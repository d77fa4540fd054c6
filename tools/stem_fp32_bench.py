"""Timing of the fp32 stem in training (the reference's main.py): forward + backward of layer0 of the fp32 model, BatchNorm
in TRAINING mode, at batch 32, 512^2 (x = [32, 3, 512, 512]), for both stems -- stride 4, and "S2 + MaxPool".  HIP events,
one process, after warm-up:

  (a) native: one codenet_stem_fp32.CodenetStemFp32Function (NATIVE_FP32_STEM = True)
  (b) the module path: Conv2d, BatchNorm2d, ReLU[, MaxPool2d] of PyTorch-ROCm under autograd (NATIVE_FP32_STEM = False)
      timed in INTERLEAVED regions (a, b, a, b, ...) so that clock and temperature drift hit both alike.

Prints one JSON line per stem: medians, min and max of both, in how many pairs (a) < (b) held, and the algorithmic bytes of
both paths.

Algorithmic bytes by this tool's own count (`stem_bytes`; float32 tensors; per-channel numbers, weights and partials left
out): every tensor a kernel (native) or a framework operator (module path) reads or writes, once per read or write.  With I
the bytes of the image, Y those of y0 [N, 24, Ho, Wo] and P those of the pooled output:
  native   stride 4   forward: convolution (I + Y), statistics (Y), apply (2Y); backward: sums (grad_out and y0: 2Y), weight
                      gradient (grad_out, y0 and the image: 2Y + I)                                          = 2I + 8Y
           S2 + pool  forward: convolution (I + Y), statistics (Y), pool (Y + P); backward: gather (P + Y, writes g_z: Y),
                      weight gradient (g_z, y0 and the image: 2Y + I)                                        = 2I + 7Y + 2P
  module   per operator: the convolution 2 tensors forward (I + Y) and its weight gradient (I + Y); BatchNorm 3Y forward
           (statistics, apply) and 5Y backward; ReLU in place 2Y forward and 3Y backward; the pool Y + P forward and P + Y
           backward                                      stride 4 = 2I + 15Y;  S2 + pool = 2I + 17Y + 2P
At batch 32, 512^2: I = 100.7 MB; stride 4: Y = 50.3 MB; S2 + pool: Y = 201.3 MB, P = 50.3 MB.

--step: the captured training step (pipeline.GraphedTrainStep, losses.CtdetLoss, fused capturable Adam) of
pipeline.DetectionNet(fp32 model) on x = [32, 3, 512, 512], native and module path (the latter needs unvalidated=True).
GPU only."""
import json
import sys

import numpy as np
import torch

import qat_bench
from codenet_amd import harness, pipeline
from codenet_amd.functions import codenet_stem as CST
from codenet_amd.functions import codenet_stem_fp32 as S32


def _model(maxpool):
    return harness.create_model(heads={"hm": 20, "wh": 2, "reg": 2}, maxpool=maxpool).cuda().train()


def stem_bytes(Nb, H, W, maxpool, native):
    """Algorithmic bytes of the stem's forward + backward (see the head of the file)."""
    s = 2 if maxpool else 4
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    I, Y = 4 * Nb * 3 * H * W, 4 * Nb * 24 * Ho * Wo
    P = 4 * Nb * 24 * ((Ho - 1) // 2 + 1) * ((Wo - 1) // 2 + 1)
    if native:
        return 2 * I + 7 * Y + 2 * P if maxpool else 2 * I + 8 * Y
    return 2 * I + 17 * Y + 2 * P if maxpool else 2 * I + 15 * Y


def main(regions=16, warm=3, batch=32, res=512):
    out = []
    for maxpool in (False, True):
        layer0 = _model(maxpool).layer0
        g = torch.Generator().manual_seed(1)
        x = torch.rand(batch, 3, res, res, generator=g).cuda()
        gy = torch.randn(batch, 24, res // 4, res // 4, generator=g).cuda()
        assert S32.native_reason(layer0, x) is None, S32.native_reason(layer0, x)

        def step(native):
            S32.NATIVE_FP32_STEM = native
            for p in layer0.parameters():
                p.grad = None
            CST.forward_stem(layer0, x).backward(gy)

        nat_ms, mod_ms = qat_bench.interleaved_ab(step, lambda: setattr(S32, "NATIVE_FP32_STEM", True), regions, warm)
        res_ = {"shape": "x=[%d,3,%d,%d], layer0 of the fp32 model (%s), BatchNorm in training mode"
                         % (batch, res, res, "stride 2 + MaxPool" if maxpool else "stride 4"),
                **qat_bench.report(nat_ms, mod_ms, moved=stem_bytes(batch, res, res, maxpool, True), ratio_digits=3),
                "pairs_native_below_module": int(np.sum(nat_ms < mod_ms)),
                "module_bytes_moved_mb": round(stem_bytes(batch, res, res, maxpool, False) / 1e6, 1)}
        print(json.dumps(res_))
        out.append(res_)
    return out


def captured_step(batch=32, res=512, steps=10):
    """--step: the captured training step of the whole fp32 network from the image, native stem and module-path stem, wall
    clock over replays."""
    crit, targets = qat_bench.ctdet_setup(batch, res)
    img = torch.rand(batch, 3, res, res, generator=torch.Generator().manual_seed(3)).cuda()
    out = {}
    try:
        for maxpool in (False, True):
            for native in (True, False):
                S32.NATIVE_FP32_STEM = native
                net = pipeline.DetectionNet(_model(maxpool))
                opt = torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device="cuda"), capturable=True, fused=True)
                step = pipeline.GraphedTrainStep(net, opt, lambda n, f: crit(n(f), targets)[0], (img,), warmup=3,
                                                 unvalidated=not native)
                key = "%s_%s_ms_per_step" % ("s2_pool" if maxpool else "s4", "native" if native else "module")
                out[key] = round(qat_bench.replay_s(step, steps) * 1e3, 3)
                del step, opt, net
    finally:
        S32.NATIVE_FP32_STEM = True
    out["config"] = ("DetectionNet(fp32 model) %dx%d, batch %d, BatchNorm in training mode, CtdetLoss, fused Adam, one HIP "
                     "graph" % (res, res, batch))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    if "--step" in sys.argv[1:]:
        captured_step()
    else:
        main()
