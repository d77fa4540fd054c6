"""Timing of the fp32 stage stack in training (the reference's main.py): forward + backward of ``deconv_layers`` --
three blocks of [deform stage, BatchNorm2d, ReLU, Upsample(x2, nearest)], BatchNorm in TRAINING mode -- at batch 32, 512^2
(x = [32, 1024, 16, 16]).  HIP events, one process, after warm-up:

  (a) native: the block behind every stage as codenet_bn.BnReluUpsample, stages 1-2 on the stored hand-over
      (NATIVE_FP32_BLOCKS = True)
  (b) the module path: BatchNorm2d, ReLU and Upsample as PyTorch-ROCm operators (NATIVE_FP32_BLOCKS = False)
      timed in INTERLEAVED regions (a, b, a, b, ...) so that clock and temperature drift hit both alike.

The stages themselves are this library's kernels either way.  Prints one JSON line: medians, min and max of both, in how many
pairs (a) < (b) held, the algorithmic bytes of the blocks, and the rate of each new entry point next to relu_fq_up2_kernel
(cdn_quantact_relu_apply) on the same tensor, stage 2's output.

Algorithmic bytes of one block, S = the bytes of its stage output y (float32; per-channel numbers and partials are left
out: kilobytes):
  module path   forward   BatchNorm reads y twice (statistics, apply), writes z 3 S; ReLU (in place) 2 S; Upsample reads S,
                          writes 4 S                                                                          = 10 S
                backward  Upsample reads 4 S, writes S; ReLU reads two, writes one 3 S; BatchNorm reads grad and y twice,
                          writes grad_y 5 S                                                                   = 13 S
  native        forward   statistics read S; apply reads S, writes S (stored hand-over) or 4 S (up-sampled)   = 3 S / 6 S
                backward  pass 1 reads the gradient S (stored) or 4 S, reads y, writes g_z; pass 2 reads g_z and y,
                          writes grad_y                                                                       = 6 S / 9 S

--step: the captured training step (pipeline.GraphedTrainStep, fused Adam) of the same stack, native and module path (the
latter needs unvalidated=True).  GPU only."""
import json
import sys

import numpy as np
import torch

import qat_bench
from codenet_amd import _native as N_
from codenet_amd import ops, pipeline
from codenet_amd.functions import codenet_bn as BN


def algorithmic_bytes(net, x):
    """(native, module path) bytes of the three blocks for the input x (see the module docstring)."""
    lib = N_.lib()
    mods = list(net.deconv_layers)
    Nb, _, H, W = x.shape
    native = module = 0
    for i in range(0, len(mods), 4):
        C = mods[i].out_channels
        S = 4 * Nb * C * H * W
        stored = bool(i + 4 < len(mods) and lib.cdn_codenet_dw_up2_supported(Nb, C, 2 * H, 2 * W))
        native += (3 + 6) * S if stored else (6 + 9) * S
        module += (10 + 13) * S
        H, W = 2 * H, 2 * W
    return native, module


def _net():
    return pipeline.build_hot_path(quantized=False).cuda().train()


def _median_ms(fn, reps=20, warm=3, calls=10):
    """Median time of ONE call of fn: `calls` calls captured as a HIP graph (launched eagerly these launches of 5-50 us
    are bound by the host), the replay timed by HIP events over `reps` regions."""
    for _ in range(warm):
        fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(calls):
            fn()
    graph.replay()
    ev = [qat_bench.timed(graph.replay) for _ in range(reps)]
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) / calls


def kernel_rates(Nb=32, C=64, H=64, W=64):
    """GB/s of the new entry points on stage 2's output, next to relu_fq_up2_kernel on the same tensor.  The statistics
    pass is the training forward minus the eval-mode forward (which is the apply kernel alone).  The tensor is 33.5 MB and
    the calls repeat back to back, so part of it is served by the 256-MB Infinity Cache -- for every kernel alike: the rates
    compare the kernels with each other, they are not HBM rates."""
    g = torch.Generator().manual_seed(2)
    y = (torch.randn(Nb, C, H, W, generator=g) * 1.5 + 0.3).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.1).cuda()
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    S = y.numel() * 4
    out = {}
    for up in (1, 2):
        go = torch.randn(Nb, C, up * H, up * W, generator=g).cuda()
        t_train = _median_ms(lambda: ops.bn_relu_up_forward(y, gamma, beta, rm, rv, nbt, 1e-5, 0.1, up, True))
        t_apply = _median_ms(lambda: ops.bn_relu_up_forward(y, gamma, beta, rm, rv, None, 1e-5, 0.1, up, False))
        _, mean, _, invstd = ops.bn_relu_up_forward(y, gamma, beta, rm, rv, nbt, 1e-5, 0.1, up, True)
        t_bwd = _median_ms(lambda: ops.bn_relu_up_backward(go, y, gamma, beta, mean, invstd, up, True))
        u = up * up
        out["up%d" % up] = {
            "apply_us": round(t_apply * 1e3, 1), "apply_gb_per_s": round((1 + u) * S / t_apply / 1e6, 1),
            "stats_us": round((t_train - t_apply) * 1e3, 1),
            "stats_gb_per_s": round(S / max(t_train - t_apply, 1e-6) / 1e6, 1),
            "backward_us": round(t_bwd * 1e3, 1), "backward_gb_per_s": round((u + 5) * S / t_bwd / 1e6, 1)}
    state = torch.zeros(8, dtype=torch.int32, device="cuda")
    state.view(torch.float32)[2] = 16.0      # scale; zero point 0
    o2 = torch.empty(Nb, C, 2 * H, 2 * W, device="cuda")
    lib = N_.lib()
    t_ref = _median_ms(lambda: N_.check(
        lib.cdn_quantact_relu_apply(y.data_ptr(), o2.data_ptr(), Nb * C, H, W, 1, state.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream), "cdn_quantact_relu_apply"))
    out["relu_fq_up2_us"] = round(t_ref * 1e3, 1)
    out["relu_fq_up2_gb_per_s"] = round(5 * S / t_ref / 1e6, 1)
    return out


def main(regions=24, warm=3, batch=32, res=512):
    net = _net()
    params = list(net.parameters())
    x = pipeline.make_input(batch, res, device="cuda").requires_grad_(True)
    g = torch.Generator().manual_seed(1)
    gy = torch.randn(batch, 64, res // 4, res // 4, generator=g).cuda()
    assert BN.native_reason(net.deconv_layers, x) is None, BN.native_reason(net.deconv_layers, x)

    def step(native):
        BN.NATIVE_FP32_BLOCKS = native
        x.grad = None
        for p in params:
            p.grad = None
        net(x).backward(gy)

    nat_ms, mod_ms = qat_bench.interleaved_ab(step, lambda: setattr(BN, "NATIVE_FP32_BLOCKS", True), regions, warm)
    b_nat, b_mod = algorithmic_bytes(net, x)
    res_ = {"shape": "x=[%d,1024,%d,%d] fp32 deconv_layers, BatchNorm in training mode" % (batch, res // 32, res // 32),
            **qat_bench.report(nat_ms, mod_ms, ratio_digits=3), "pairs_native_below_module": int(np.sum(nat_ms < mod_ms)),
            "block_bytes_native_mb": round(b_nat / 1e6, 1), "block_bytes_module_mb": round(b_mod / 1e6, 1),
            "kernels_stage2_tensor": kernel_rates(batch, 64, res // 8, res // 8)}
    print(json.dumps(res_))
    return res_


def captured_step(batch=32, res=512, steps=20):
    """--step: the captured training step of the stack with fused Adam, native and module path, wall clock over replays."""
    x = pipeline.make_input(batch, res, device="cuda")
    out = {}
    try:
        for native in (True, False):
            BN.NATIVE_FP32_BLOCKS = native
            net = _net()
            opt = torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device="cuda"), capturable=True, fused=True)

            def loss_fn(n, t):
                y = n(t)
                return y.square().reshape(-1, 64).sum(1).sum() / y.numel()

            step = pipeline.GraphedTrainStep(net, opt, loss_fn, (x,), warmup=3, unvalidated=not native)
            out["native_ms_per_step" if native else "module_ms_per_step"] = round(qat_bench.replay_s(step, steps) * 1e3, 3)
    finally:
        BN.NATIVE_FP32_BLOCKS = True
    out["config"] = "fp32 deconv_layers %dx%d, batch %d, BatchNorm in training mode, fused Adam, one HIP graph" % (res, res, batch)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    if "--step" in sys.argv[1:]:
        captured_step()
    else:
        main()
