"""Timing of the quantised detection heads in the QAT step (codenet_heads_train.hip through
codenet_amd.functions.codenet_heads): forward + backward of the three heads (hm 20, wh 2, reg 2) at the QAT shape,
x = [32, 64, 128, 128].  HIP events, one process, after warm-up:

  (a) native: CodenetHeadsFunction (NATIVE_HEADS = True)      (b) the module path under the framework's autograd
      timed in INTERLEAVED regions (a, b, a, b, ...) so that clock and temperature drift hit both alike.

Both include the weight preparation (fold + fake-quantisation, native either way) and the gradients of x and of every
parameter.  Prints one JSON line: the medians, the ratio, whether (a) < (b) held in every pair, and the native path's
algorithmic HBM bytes -- every pass over a [N, 64, H, W] tensor it has to make, plus the thin y3 / grad_y3 -- divided by
its time.  --step: the captured step of the whole detection tail instead (see tail_step).  GPU only."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

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

    def timed(native):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(native)
        b.record()
        return a, b

    try:
        for _ in range(warm):
            step(True), step(False)
        torch.cuda.synchronize()
        ev = {True: [], False: []}
        for _ in range(regions):
            ev[True].append(timed(True))
            ev[False].append(timed(False))
        torch.cuda.synchronize()
    finally:
        CH.NATIVE_HEADS = True
    ms = {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
    nat, mod = float(np.median(ms[True])), float(np.median(ms[False]))
    moved = algorithmic_bytes(N, 64, R * R, list(model.heads.values()))
    res = {"shape": "x=[%d,64,%d,%d] heads=%s" % (N, R, R, dict(model.heads)), "regions": regions,
           "native_fwd_bwd_ms": round(nat, 4), "module_fwd_bwd_ms": round(mod, 4), "module_over_native": round(mod / nat, 2),
           "native_below_module_in_every_pair": bool(np.all(ms[True] < ms[False])),
           "native_max_ms": round(float(ms[True].max()), 4), "module_min_ms": round(float(ms[False].min()), 4),
           "native_bytes_moved_mb": round(moved / 1e6, 1), "native_gb_per_s": round(moved / nat / 1e6, 1)}
    print(json.dumps(res))
    return res


def tail_step(batch=32, res=512, steps=20):
    """--step: the captured QAT step of the detection tail -- deform stages, heads, losses.CtdetLoss, fused Adam -- as
    pipeline.GraphedTrainStep accepts it without `unvalidated`, timed over `steps` replays (wall clock around the
    replays, as tools/train_step_bench.py times cfg5's step over the stages alone)."""
    import time
    import types
    from codenet_amd import pipeline
    from codenet_amd.losses import CtdetLoss, ctdet_targets
    net = pipeline.DetectionTail(harness.create_model(quantize=True)).cuda().train()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    R, M = res // 4, 50
    rng = np.random.default_rng(1)
    c = rng.uniform([1, 1], [R - 2, R - 2], (batch, M, 2))
    s = rng.uniform(0.8, 40.0, (batch, M, 2))
    boxes = torch.from_numpy(np.clip(np.concatenate([c - s / 2, c + s / 2], 2), 0, R - 1).astype(np.float32)).cuda()
    targets = ctdet_targets(boxes, torch.from_numpy(rng.integers(0, 20, (batch, M))).cuda(),
                            torch.from_numpy(rng.integers(M // 2, M + 1, batch)).cuda(), 20, R, R, M)
    crit = CtdetLoss(types.SimpleNamespace(mse_loss=False, reg_loss="l1", dense_wh=False, norm_wh=False, cat_spec_wh=False,
                                           num_stacks=1, hm_weight=1.0, wh_weight=0.1, off_weight=1.0, reg_offset=True))
    feat = pipeline.make_input(batch, res, device="cuda").requires_grad_(True)      # (as cfg5: the backbone would need it)
    opt = torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device="cuda"), capturable=True, fused=True)
    step = pipeline.GraphedTrainStep(net, opt, lambda n, f: crit(n(f), targets)[0], (feat,), warmup=3)
    for _ in range(3):
        step.graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.graph.replay()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    res_ = {"config": "CoDeNet1x %dx%d W4A8 QAT step over deconv_layers + heads + CtdetLoss, batch %d, one HIP graph" % (
        res, res, batch), "ms_per_step": round(dt * 1e3, 3), "images_per_s": round(batch / dt, 1),
        "loss": float(step.loss.detach())}
    print(json.dumps(res_))
    return res_


if __name__ == "__main__":
    if "--step" in sys.argv[1:]:
        tail_step()
    else:
        main()
