"""Timing of the fp32 detection heads in training (the reference's main.py): forward + backward of the three heads hm 20 /
wh 2 / reg 2 -- each Conv2d 1x1 -> BatchNorm2d -> ReLU -> depthwise Conv2d 3x3 -> BatchNorm2d -> ReLU -> Conv2d 1x1, BatchNorm
in TRAINING mode -- at batch 32, 512^2 (x = [32, 64, 128, 128]).  HIP events, one process, after warm-up:

  (a) native: all heads as one codenet_heads_fp32.CodenetHeadsFp32Function (NATIVE_FP32_HEADS = True)
  (b) the module path: seven PyTorch-ROCm modules per head under autograd (NATIVE_FP32_HEADS = False)
      timed in INTERLEAVED regions (a, b, a, b, ...) so that clock and temperature drift hit both alike.

Prints one JSON line: medians, min and max of both, in how many pairs (a) < (b) held, the algorithmic bytes, and the time
and rate of each new kernel next to bn_apply_kernel (cdn_codenet_bn_relu_up_forward, eval mode, up = 1) on the same tensor.

Algorithmic bytes, S = the bytes of one 64-channel head tensor (float32; x, the narrow y3 / grad_y3, per-channel numbers and
partials are left out):
  native   forward   hm: y1 written, read by the statistics and by the depthwise kernel, y2 written, read twice by
                     BatchNorm2 (statistics, apply), a2 written and read by the last conv                        = 8 S
                     wh / reg: the same up to y2, which the statistics and the tail kernel read once each       = 6 S
           backward  hm: a2 read (grad W3), grad_a2 written, first pass reads it and y2, writes g_z2; the depthwise
                     backward reads g_z2, y2, y1, writes g_z1; the second pass reads g_z1, y1, writes grad_y1, which
                     grad W1 and grad x read once each                                                           = 14 S
                     wh / reg: the tail backward reads y2 and writes g_z2 instead of the first three           = 11 S
           one step of the three heads                                                                          = 56 S
  module   forward   conv (1), BatchNorm (3), ReLU in place (2), depthwise (2), BatchNorm (3), ReLU (2), conv (1) = 14 S
           backward  conv (2), ReLU (3), BatchNorm (5), depthwise (4), ReLU (3), BatchNorm (5), conv (2)          = 24 S
           one step of the three heads                                                                          = 114 S

--step: the captured training step (pipeline.GraphedTrainStep, losses.CtdetLoss, fused capturable Adam) of
pipeline.DetectionTail(fp32 model) on x = [32, 1024, 16, 16], native and module path (the latter needs unvalidated=True).
GPU only."""
import json
import sys
import types

import numpy as np
import torch

import qat_bench
from fp32_block_bench import _median_ms
from codenet_amd import harness, ops, pipeline
from codenet_amd.functions import codenet_heads as CH
from codenet_amd.functions import _fp32_common as F32
from codenet_amd.functions import codenet_heads_fp32 as HF

WIDTHS = {"hm": 20, "wh": 2, "reg": 2}


def _model():
    return harness.create_model(heads=dict(WIDTHS)).cuda().train()


def kernel_rates(Nb=32, C=64, H=128, W=128):
    """Microseconds and GB/s (algorithmic bytes) of the new kernels on one head tensor, next to bn_apply_kernel on the same
    tensor.  The tensor is 134 MB and the calls repeat back to back, so part of it is served by the 256-MB Infinity Cache
    -- for every kernel alike: the rates compare the kernels with each other, they are not HBM rates."""
    g = torch.Generator().manual_seed(2)
    y1 = (torch.randn(Nb, C, H, W, generator=g) * 1.5 + 0.3).cuda()
    gy3 = torch.randn(Nb, 2, H, W, generator=g).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.1).cuda()
    w2 = (torch.randn(C, 1, 3, 3, generator=g) / 3).cuda()
    w3, b3 = (torch.randn(2, C, 1, 1, generator=g) / 8).cuda(), torch.zeros(2, device="cuda")
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    S = y1.numel() * 4
    st1 = F32.bn_stats(y1, bn)
    y2 = HF.dw_forward(y1, st1, gamma, beta, w2)
    st2 = F32.bn_stats(y2, bn)
    gz2, _, _, means2, _, _ = HF.tail_backward(gy3, y2, st2, gamma, beta, w3)
    gz1, _, _, _, means1 = HF.dw_backward(gz2, y2, st2, gamma, means2, True, y1, st1, gamma, beta, w2)
    gy1 = torch.empty_like(y1)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    calls = {
        "bn_apply_kernel": (2, lambda: ops.bn_relu_up_forward(y1, gamma, beta, rm, rv, None, 1e-5, 0.1, 1, False)),
        "bn_stats_kernel": (1, lambda: F32.bn_stats(y1, bn)),
        "head32_dw_fwd_kernel": (2, lambda: HF.dw_forward(y1, st1, gamma, beta, w2)),
        "head32_tail_fwd_kernel": (1, lambda: HF.tail_forward(y2, st2, gamma, beta, w3, b3)),
        "head32_tail_bwd_kernel": (2, lambda: HF.tail_backward(gy3, y2, st2, gamma, beta, w3)),
        "head32_dw_bwd_kernel": (4, lambda: HF.dw_backward(gz2, y2, st2, gamma, means2, True, y1, st1, gamma, beta, w2)),
        "head32_bn_bwd2_kernel": (3, lambda: F32.bn_backward2(gz1, y1, st1, gamma, means1, True, gy1, 0, C * H * W)),
    }
    out = {}
    for name, (tensors, fn) in calls.items():
        ms = _median_ms(fn, reps=10, warm=2, calls=4)
        out[name] = {"us": round(ms * 1e3, 1), "tensors": tensors, "gb_per_s": round(tensors * S / ms / 1e6, 1)}
    return out


def main(regions=16, warm=3, batch=32, res=512):
    model = _model()
    heads = {h: getattr(model, h) for h in WIDTHS}
    params = [p for m in heads.values() for p in m.parameters()]
    g = torch.Generator().manual_seed(1)
    R = res // 4
    x = (torch.randn(batch, 64, R, R, generator=g).abs_() * 1.66).cuda().requires_grad_(True)
    gys = [torch.randn(batch, co, R, R, generator=g).cuda() for co in WIDTHS.values()]
    assert HF.native_reason(heads, x) is None, HF.native_reason(heads, x)

    def step(native):
        HF.NATIVE_FP32_HEADS = native
        x.grad = None
        for p in params:
            p.grad = None
        out = CH.forward_heads(heads, x)
        torch.autograd.backward([out[h] for h in WIDTHS], gys)

    nat_ms, mod_ms = qat_bench.interleaved_ab(step, lambda: setattr(HF, "NATIVE_FP32_HEADS", True), regions, warm)
    S = 4 * batch * 64 * R * R
    res_ = {"shape": "x=[%d,64,%d,%d], heads hm 20 / wh 2 / reg 2, BatchNorm in training mode" % (batch, R, R),
            **qat_bench.report(nat_ms, mod_ms, moved=56 * S, ratio_digits=3),
            "pairs_native_below_module": int(np.sum(nat_ms < mod_ms)), "module_bytes_moved_mb": round(114 * S / 1e6, 1),
            "kernels_head_tensor": kernel_rates(batch, 64, R, R)}
    print(json.dumps(res_))
    return res_


def captured_step(batch=32, res=512, steps=10):
    """--step: the captured training step of the fp32 tail, native and module path, wall clock over replays."""
    from codenet_amd.losses import CtdetLoss, ctdet_targets
    R, M = res // 4, 50
    rng = np.random.default_rng(1)
    c = rng.uniform([1, 1], [R - 2, R - 2], (batch, M, 2))
    s = rng.uniform(0.8, 40.0, (batch, M, 2))
    boxes = torch.from_numpy(np.clip(np.concatenate([c - s / 2, c + s / 2], 2), 0, R - 1).astype(np.float32)).cuda()
    targets = ctdet_targets(boxes, torch.from_numpy(rng.integers(0, 20, (batch, M))).cuda(),
                            torch.from_numpy(rng.integers(M // 2, M + 1, batch)).cuda(), 20, R, R, M)
    crit = CtdetLoss(types.SimpleNamespace(mse_loss=False, reg_loss="l1", dense_wh=False, norm_wh=False, cat_spec_wh=False,
                                           num_stacks=1, hm_weight=1.0, wh_weight=0.1, off_weight=1.0, reg_offset=True))
    feat = (torch.randn(batch, 1024, res // 32, res // 32, generator=torch.Generator().manual_seed(3)).abs_() * 1.66).cuda()
    out = {}
    try:
        for native in (True, False):
            HF.NATIVE_FP32_HEADS = native
            net = pipeline.DetectionTail(_model())
            opt = torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device="cuda"), capturable=True, fused=True)
            step = pipeline.GraphedTrainStep(net, opt, lambda n, f: crit(n(f), targets)[0], (feat,), warmup=3,
                                             unvalidated=not native)
            out["native_ms_per_step" if native else "module_ms_per_step"] = round(qat_bench.replay_s(step, steps) * 1e3, 3)
            del step, opt, net
    finally:
        HF.NATIVE_FP32_HEADS = True
    out["config"] = ("DetectionTail(fp32 model) %dx%d, batch %d, BatchNorm in training mode, CtdetLoss, fused Adam, one HIP "
                     "graph" % (res, res, batch))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    if "--step" in sys.argv[1:]:
        captured_step()
    else:
        main()
