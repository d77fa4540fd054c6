"""Per-image cost of pre-processing for the AP50 procedure: the HOST path (tools/eval_voc.pre_process for the S test
scales: F.interpolate + F.grid_sample on the CPU, the mirrors, and the upload of [S or 2S, 3, res, res] floats) against
the GPU path (codenet_amd.preproc: upload of the image bytes + the item table, one launch of cdn_ctdet_pre_process), and
the kernel alone by HIP events beside a device-to-device copy and a fill of the same output tensor (the bandwidth
yardsticks).  A 375 x 500 image at res 512, S in {1, 5}, with and without the mirrors; host and GPU path alternate and
the figures are medians.  One JSON line per image.  GPU only.

--color_aug: the training sample's input instead (sample/ctdet.py:76-79) for a batch of res x res byte crops: the HOST path
(numpy float32: v / 255, the three blends and the lighting term per item, (x - mean) / std, HWC -> CHW, the upload of
[B, 3, res, res] floats) against the GPU path (upload of the bytes, the item and the aug table, cdn_ctdet_pre_process_aug =
zero_sums_kernel + crop_sum_kernel + color_aug_kernel), and the three launches alone by HIP events beside the same yardsticks."""
import argparse
import importlib.util
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from codenet_amd import preproc

SCALES = [0.5, 0.75, 1.0, 1.25, 1.5]


def _eval_voc():
    spec = importlib.util.spec_from_file_location("eval_voc", os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                                           "eval_voc.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, steps, warm=10, inner=10):
    """Median over `steps` event pairs of the time of ONE call; a pair spans `inner` back-to-back calls, so the events'
    own cost does not sit in a figure of a few microseconds."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        for _ in range(inner):
            fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) / inner for a, b in ev)
    return ms[len(ms) // 2]


def median(v):
    return sorted(v)[len(v) // 2]


def one_config(ev, img, res, scales, flip, reps, steps):
    S = len(scales)
    pre = preproc.PreProcess(res, res, scales=scales, flip_test=flip, max_h=img.shape[0], max_w=img.shape[1])
    out = torch.empty((2 if flip else 1) * S, 3, res, res, dtype=torch.float32, device="cuda")
    static = torch.empty_like(out)

    def host():
        inp = torch.cat([ev.pre_process(img, res, sc)[0] for sc in scales], 0)
        if flip:
            inp = torch.cat([inp, torch.flip(inp, [3])], 0)
        static.copy_(inp, non_blocking=True)

    def gpu():
        pre.load(img)
        pre.run(out)

    host(), gpu()                                   # warm-up of both
    t_host, t_gpu = [], []
    for _ in range(reps):                           # interleaved
        t_host.append(wall_ms(host))
        t_gpu.append(wall_ms(gpu))
    # how far the two inputs are apart (the integer specification against the float path), in normalised units
    diff = (out - static).abs()
    k_ms = event_ms(lambda: pre.run(out), steps)
    copy_ms = event_ms(lambda: static.copy_(out), steps)
    fill_ms = event_ms(lambda: static.fill_(1.0), steps)
    ob = out.numel() * 4
    sb = img.size
    return {"S": S, "flip": bool(flip), "host_ms": round(median(t_host), 3), "gpu_ms": round(median(t_gpu), 3),
            "kernel_us": round(k_ms * 1e3, 2), "copy_us": round(copy_ms * 1e3, 2), "fill_us": round(fill_ms * 1e3, 2),
            "out_bytes": ob, "src_bytes": sb,
            "kernel_GBps": round((ob + sb) / k_ms * 1e-6, 1),           # output written + source read once
            "copy_GBps": round(2 * ob / copy_ms * 1e-6, 1),             # read + written
            "fill_GBps": round(ob / fill_ms * 1e-6, 1),
            "kernel_share_of_copy_bandwidth": round(((ob + sb) / k_ms) / (2 * ob / copy_ms), 3),
            "kernel_time_over_fill_time": round(k_ms / fill_ms, 3),
            "max_abs_diff_vs_host_path": round(float(diff.max()), 4), "mean_abs_diff_vs_host_path": round(float(diff.mean()), 5)}


def host_color_aug(u8, row, mean, std):
    """The float32 chain of DESIGN.md section 7.4c in numpy, except that gs_mean is numpy's own float32 mean (what a host
    loader would do): the cost yardstick, not the contract."""
    x = u8.astype(np.float32) / np.float32(255)
    if row[0]:
        gs = (x[..., 0] * np.float32(0.114) + x[..., 1] * np.float32(0.587)) + x[..., 2] * np.float32(0.299)
        gm = gs.mean()
        for k in row[1:4]:
            x *= np.float32(row[4 + k])
            if k == 1:
                x += gm * np.float32(row[7 + k])
            elif k == 2:
                x += (gs * np.float32(row[7 + k]))[..., None]
        x += np.array(row[10:13], dtype=np.float32)
    return np.ascontiguousarray(((x - mean) / std).transpose(2, 0, 1))


def color_aug_config(res, batch, reps, steps):
    rng = np.random.RandomState(123)
    imgs = np.random.default_rng(0).integers(0, 256, (batch, res, res, 3), dtype=np.uint8)
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    table = [preproc.item_row(i * res * res * 3, res, res, 3 * res, ident) for i in range(batch)]
    rows = [preproc.color_aug_params(rng) for _ in range(batch)]
    pre = preproc.PreProcess(res, res, max_h=res * batch, max_w=res, max_items=batch, color_aug=True)
    out = torch.empty(batch, 3, res, res, dtype=torch.float32, device="cuda")
    static = torch.empty_like(out)
    pinned = torch.empty(out.shape, dtype=torch.float32).pin_memory()
    mean, std = preproc.MEAN.reshape(1, 1, 3), preproc.STD.reshape(1, 1, 3)

    def host():
        for i in range(batch):
            pinned[i] = torch.from_numpy(host_color_aug(imgs[i], rows[i], mean, std))
        static.copy_(pinned, non_blocking=True)

    def gpu():
        pre.load_items(imgs, table, aug=rows)
        pre.run(out)

    host(), gpu()
    t_host, t_gpu = [], []
    for _ in range(reps):
        t_host.append(wall_ms(host))
        t_gpu.append(wall_ms(gpu))
    diff = (out - static).abs()
    k_ms = event_ms(lambda: pre.run(out), steps)
    copy_ms = event_ms(lambda: static.copy_(out), steps)
    fill_ms = event_ms(lambda: static.fill_(1.0), steps)
    ob, sb = out.numel() * 4, imgs.size
    moved = ob + 3 * sb                 # source read, crop bytes written and read back, planes written
    return {"color_aug": True, "batch": batch, "res": res, "host_ms": round(median(t_host), 3),
            "gpu_ms": round(median(t_gpu), 3), "launches_us": round(k_ms * 1e3, 2),
            "copy_us": round(copy_ms * 1e3, 2), "fill_us": round(fill_ms * 1e3, 2), "out_bytes": ob, "src_bytes": sb,
            "launches_GBps": round(moved / k_ms * 1e-6, 1), "copy_GBps": round(2 * ob / copy_ms * 1e-6, 1),
            "fill_GBps": round(ob / fill_ms * 1e-6, 1), "launches_time_over_fill_time": round(k_ms / fill_ms, 3),
            "max_abs_diff_vs_host_path": float(diff.max()), "host_threads": torch.get_num_threads()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=9, help="interleaved host / GPU repetitions per configuration")
    ap.add_argument("--steps", type=int, default=30, help="event pairs (of 10 launches each) per HIP-event median")
    ap.add_argument("--color_aug", action="store_true", help="the training sample's colour augmentation leg")
    ap.add_argument("--batch", type=int, default=32, help="--color_aug: items per batch")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "preproc_bench needs the GPU"
    if args.color_aug:
        print(json.dumps(color_aug_config(args.res, args.batch, args.reps, args.steps)), flush=True)
        return
    ev = _eval_voc()
    for n in range(args.images):
        img = np.random.default_rng(n).integers(0, 256, (args.height, args.width, 3), dtype=np.uint8)
        rows = [one_config(ev, img, args.res, scales, flip, args.reps, args.steps)
                for scales in ([1.0], SCALES) for flip in (False, True)]
        print(json.dumps({"image": "%dx%d noise, seed %d" % (args.height, args.width, n), "res": args.res,
                          "host_threads": torch.get_num_threads(), "configs": rows}), flush=True)


if __name__ == "__main__":
    main()
