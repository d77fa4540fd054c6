"""Timing of the fp32 ShuffleNetV2 units and layer4 in training (the reference's main.py): forward + backward of layers 1-4
of the fp32 model, BatchNorm in TRAINING mode, at batch 32, 512^2 (x = [32, 24, 128, 128], layer0's output).  HIP events,
one process, after warm-up:

  (a) native: every unit one codenet_units_fp32.CodenetUnitFp32Function, layer4 the pointwise kernel + the fused BatchNorm +
      ReLU (NATIVE_FP32_UNITS = True)
  (b) the module path: 8 / 13 PyTorch-ROCm modules per unit plus cat and channel_shuffle under autograd
      (NATIVE_FP32_UNITS = False)
      timed in INTERLEAVED regions (a, b, a, b, ...) so that clock and temperature drift hit both alike.

Prints one JSON line: medians, min and max of both, in how many pairs (a) < (b) held, the algorithmic bytes of both paths,
and the time and rate of each new kernel next to bn_apply_kernel (cdn_codenet_bn_relu_up_forward, eval mode, up = 1) on one
tensor.

Algorithmic bytes by this tool's own count (`unit_bytes`; float32 tensors, per-channel numbers, weights and partials left
out): every tensor a kernel (native) or a framework operator (module path) reads or writes, once per read or write.  With A
the bytes of [N, h, H, W], B those of [N, h, Ho, Wo], X those of x and D those of [N, Cin, Ho, Wo]:
  native   branch 2 forward   pw1 (2A), statistics (A), depthwise (A + B), statistics (B), BatchNorm (2B), pw3 (2B), statistics
                              (B), join (B + its slot of out B [+ the pass-through half, read and written: 2B at stride 1])
           branch 2 backward  join backward (reads B of grad_out and y3, writes g_z3: 3B [+ 2B pass-through]), second pass
                              (3B), grad W3 (2B), grad z2 (2B), sums (2B), depthwise backward (2B + 2A), second pass (3A), grad
                              W1 (2A), grad x2 (2A)
           branch 1 (stride 2) depthwise (X + D), statistics (D), BatchNorm (2D), pw5 (D + B), statistics (B), join (2B);
                              join backward (3B), second pass (3B), grad W5 (B + D), grad z4 (B + D), sums (2D), depthwise
                              backward (2D + X + 2X: grad_x read and written)
  module   per operator: a convolution 2 tensors forward and 4 backward (data and weight gradient), BatchNorm 3 forward
           (statistics, apply) and 5 backward, ReLU in place 2 forward and 3 backward, cat and channel_shuffle 2 each way of
           `out`, the stride-1 split's gradient 2X.

--step: the captured training step (pipeline.GraphedTrainStep, losses.CtdetLoss, fused capturable Adam) of
pipeline.DetectionTrunk(fp32 model) on x = [32, 24, 128, 128], native and module path (the latter needs unvalidated=True).
GPU only."""
import json
import sys
import types

import numpy as np
import torch

import qat_bench
from fp32_block_bench import _median_ms
from codenet_amd import harness, ops, pipeline
from codenet_amd.functions import _fp32_common as F32
from codenet_amd.functions import codenet_units as CU
from codenet_amd.functions import codenet_units_fp32 as U32


def _model():
    return harness.create_model(heads={"hm": 20, "wh": 2, "reg": 2}).cuda().train()


def unit_bytes(Nb, Cin, h, H, W, stride, native):
    """Algorithmic bytes of one unit's forward + backward (see the head of the file)."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    A, B, X, D = (4 * Nb * c * a * b for c, a, b in ((h, H, W), (h, Ho, Wo), (Cin, H, W), (Cin, Ho, Wo)))
    if native:
        fwd = 2 * A + A + (A + B) + B + 2 * B + 2 * B + B + 2 * B + (2 * B if stride == 1 else 0)
        bwd = 3 * B + (2 * B if stride == 1 else 0) + 3 * B + 2 * B + 2 * B + 2 * B + (2 * B + 2 * A) + 3 * A + 2 * A + 2 * A
        if stride == 2:
            fwd += (X + D) + D + 2 * D + (D + B) + B + 2 * B
            bwd += 3 * B + 3 * B + (B + D) + (B + D) + 2 * D + (2 * D + 3 * X)
        return fwd + bwd
    Cx2 = X if stride == 2 else A      # the input of pw1
    fwd = (Cx2 + A) + 3 * A + 2 * A + (A + B) + 3 * B + 2 * B + 3 * B + 2 * B + 4 * (2 * B)
    bwd = 2 * (Cx2 + A) + 5 * A + 3 * A + 2 * (A + B) + 5 * B + 4 * B + 5 * B + 3 * B + 4 * (2 * B) + (2 * X if stride == 1 else 0)
    if stride == 2:
        fwd += (X + D) + 3 * D + (D + B) + 3 * B + 2 * B
        bwd += 2 * (X + D) + 5 * D + 2 * (D + B) + 5 * B + 3 * B + 3 * X      # (+ the sum of both branches' grad_x)
    return fwd + bwd


def trunk_bytes(model, Nb, H, W, native):
    total = 0
    for layer in (model.layer1, model.layer2, model.layer3):
        for node in layer:
            c1 = node.b2[0]
            h = c1.out_channels
            Cin = c1.in_channels if node.stride == 2 else 2 * h
            total += unit_bytes(Nb, Cin, h, H, W, node.stride, native)
            H, W = (H - 1) // node.stride + 1, (W - 1) // node.stride + 1
    Y = 4 * Nb * H * W
    c4 = model.layer4[0]
    # layer4: the convolution (2 / 4), BatchNorm + ReLU fused (statistics 1, apply 2; backward 3 + 3) or 3 + 2 / 5 + 3
    total += Y * ((c4.in_channels + c4.out_channels) * 3 + c4.out_channels * ((3 + 6) if native else (5 + 8)))
    return total


def kernel_rates(Nb=32, C=58, H=128, W=128):
    """Microseconds and GB/s (algorithmic bytes) of the new kernels on y1 of layer1's first unit, next to bn_apply_kernel on
    the same tensor.  The tensor is 122 MB and the calls repeat back to back, so part of it is served by the 256-MB Infinity
    Cache -- for every kernel alike: the rates compare the kernels with each other, they are not HBM rates."""
    g = torch.Generator().manual_seed(2)
    y1 = (torch.randn(Nb, C, H, W, generator=g) * 1.5 + 0.3).cuda()
    x = torch.randn(Nb, 2 * C, H, W, generator=g).cuda()
    gout = torch.randn(Nb, 2 * C, H, W, generator=g).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.1).cuda()
    w = (torch.randn(C, 1, 3, 3, generator=g) / 3).cuda()
    bn = torch.nn.BatchNorm2d(C).cuda().train()
    S, pitch = y1.numel() * 4, C * H * W
    st1 = F32.bn_stats(y1, bn)
    y2 = {s: U32._dw_forward(y1.data_ptr(), pitch, st1, gamma, beta, w, Nb, C, H, W, s, y1) for s in (1, 2)}
    st2 = {s: F32.bn_stats(y2[s], bn) for s in (1, 2)}
    gz2 = {s: torch.randn_like(y2[s]) for s in (1, 2)}
    means2 = {s: U32._bn_backward_sums(gz2[s], y2[s], st2[s])[2] for s in (1, 2)}
    out, gx, gz1 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(y1)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")

    def dw_bwd(s):
        return U32._dw_backward(gz2[s], y2[s], st2[s], gamma, means2[s], True, y1.data_ptr(), pitch, st1, gamma, beta, w,
                                (gz1.data_ptr(), pitch), False, Nb, C, H, W, s)

    calls = {
        "bn_apply_kernel": (2, lambda: ops.bn_relu_up_forward(y1, gamma, beta, rm, rv, None, 1e-5, 0.1, 1, False)),
        "unit32_dw_fwd_kernel stride 1": (2, lambda: U32._dw_forward(y1.data_ptr(), pitch, st1, gamma, beta, w, Nb, C, H, W, 1, y1)),
        "unit32_dw_fwd_kernel stride 2": (1.25, lambda: U32._dw_forward(y1.data_ptr(), pitch, st1, gamma, beta, w, Nb, C, H, W, 2, y1)),
        "unit32_apply_kernel (BatchNorm)": (2, lambda: U32._bn_forward(y1, st1, gamma, beta)),
        "unit32_apply_kernel (join, stride 1)": (4, lambda: U32._join(y1, st1, gamma, beta, out, 1, (x.data_ptr(), 2 * pitch))),
        "unit32_bwd1_kernel (join, stride 1)": (5, lambda: U32._join_backward(gout, y1, st1, gamma, beta, 1, (gx.data_ptr(), 2 * pitch))),
        "unit32_bwd1_kernel (sums)": (2, lambda: U32._bn_backward_sums(gz2[1], y1, st1)),
        "unit32_dw_bwd_kernel stride 1": (4, lambda: dw_bwd(1)),
        "unit32_dw_bwd_kernel stride 2": (2.5, lambda: dw_bwd(2)),
    }
    res = {}
    for name, (tensors, fn) in calls.items():
        ms = _median_ms(fn, reps=10, warm=2, calls=4)
        res[name] = {"us": round(ms * 1e3, 1), "tensors": tensors, "gb_per_s": round(tensors * S / ms / 1e6, 1)}
    return res


def main(regions=16, warm=3, batch=32, res=512):
    model = _model()
    layers = [model.layer1, model.layer2, model.layer3]
    params = [p for m in layers + [model.layer4] for p in m.parameters()]
    g = torch.Generator().manual_seed(1)
    R = res // 4
    x = (torch.randn(batch, 24, R, R, generator=g).abs_() * 0.7).cuda().requires_grad_(True)
    gy = torch.randn(batch, 1024, R // 8, R // 8, generator=g).cuda()
    assert U32.native_reason(model.layer1, x) is None, U32.native_reason(model.layer1, x)

    def step(native):
        U32.NATIVE_FP32_UNITS = native
        x.grad = None
        for p in params:
            p.grad = None
        t = x
        for layer in layers:
            t = CU.forward_units(layer, t)
        CU.forward_layer4(model.layer4, t).backward(gy)

    nat_ms, mod_ms = qat_bench.interleaved_ab(step, lambda: setattr(U32, "NATIVE_FP32_UNITS", True), regions, warm)
    res_ = {"shape": "x=[%d,24,%d,%d], layers 1-4 of the fp32 model, BatchNorm in training mode" % (batch, R, R),
            **qat_bench.report(nat_ms, mod_ms, moved=trunk_bytes(model, batch, R, R, True), ratio_digits=3),
            "pairs_native_below_module": int(np.sum(nat_ms < mod_ms)),
            "module_bytes_moved_mb": round(trunk_bytes(model, batch, R, R, False) / 1e6, 1),
            "kernels_y1_tensor": kernel_rates(batch, 58, R, R)}
    print(json.dumps(res_))
    return res_


def captured_step(batch=32, res=512, steps=10):
    """--step: the captured training step of the fp32 trunk, native and module path, wall clock over replays."""
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
    feat = (torch.randn(batch, 24, R, R, generator=torch.Generator().manual_seed(3)).abs_() * 0.7).cuda()
    out = {}
    try:
        for native in (True, False):
            U32.NATIVE_FP32_UNITS = native
            net = pipeline.DetectionTrunk(_model())
            opt = torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device="cuda"), capturable=True, fused=True)
            step = pipeline.GraphedTrainStep(net, opt, lambda n, f: crit(n(f), targets)[0], (feat,), warmup=3,
                                             unvalidated=not native)
            out["native_ms_per_step" if native else "module_ms_per_step"] = round(qat_bench.replay_s(step, steps) * 1e3, 3)
            del step, opt, net
    finally:
        U32.NATIVE_FP32_UNITS = True
    out["config"] = ("DetectionTrunk(fp32 model) %dx%d, batch %d, BatchNorm in training mode, CtdetLoss, fused Adam, one HIP "
                     "graph" % (res, res, batch))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    if "--step" in sys.argv[1:]:
        captured_step()
    else:
        main()
