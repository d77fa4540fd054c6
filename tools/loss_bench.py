"""Timing of the ctdet criterion (codenet_loss.hip through codenet_amd.losses.CtdetLoss) at the training shape of cfg5:
N = 32 images, 20 classes, 128 x 128 maps, 50 object rows per image.  HIP events, one process, after warm-up:

  (a) native forward + backward            (b) the composed PyTorch path, forward + backward
      timed in INTERLEAVED pairs (a, b, a, b, ...) so that clock and temperature drift hit both alike;
  (c) cdn_ctdet_targets (one launch from the object lists) against the host-to-device copy of the same hm map from
      pinned memory -- what a data loader that builds the map on the host has to ship every step.

Prints one JSON line: medians, the ratio, whether (a) < (b) held in every pair, and the GB/s (a) achieves against the
bytes it has to move (hm logits and target read forward and backward, the hm gradient written: 5 maps; plus the two
dense regression gradients).  GPU only."""
import json
import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from codenet_amd.losses import CtdetLoss, ctdet_targets


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main(pairs=200, warm=10):
    N, C, H, W, M = 32, 20, 128, 128, 50
    g = torch.Generator().manual_seed(1)
    hm = (torch.randn(N, C, H, W, generator=g) * 1.5 - 2.0).cuda().requires_grad_(True)
    wh = (torch.rand(N, 2, H, W, generator=g) * 30).cuda().requires_grad_(True)
    reg = torch.rand(N, 2, H, W, generator=g).cuda().requires_grad_(True)
    rng = np.random.default_rng(1)
    c = rng.uniform([1, 1], [W - 2, H - 2], (N, M, 2))
    s = rng.uniform(0.8, 40.0, (N, M, 2))
    boxes = torch.from_numpy(np.clip(np.concatenate([c - s / 2, c + s / 2], 2), 0, [W - 1, H - 1, W - 1, H - 1])
                             .astype(np.float32)).cuda()
    classes = torch.from_numpy(rng.integers(0, C, (N, M))).cuda()
    counts = torch.from_numpy(rng.integers(M // 2, M + 1, N)).cuda()
    batch = ctdet_targets(boxes, classes, counts, C, H, W, M)
    crit = CtdetLoss(types.SimpleNamespace(mse_loss=False, reg_loss="l1", dense_wh=False, norm_wh=False, cat_spec_wh=False,
                                           num_stacks=1, hm_weight=1.0, wh_weight=0.1, off_weight=1.0, reg_offset=True))

    def native():
        for t in (hm, wh, reg):
            t.grad = None
        crit([{"hm": hm, "wh": wh, "reg": reg}], batch)[0].backward()

    def composed():
        for t in (hm, wh, reg):
            t.grad = None
        crit._forward_composed([{"hm": hm.clone(), "wh": wh, "reg": reg}], batch)[0].backward()

    def clone_only():          # the copy that keeps the composed path's in-place sigmoid off the leaf: subtracted from (b)
        hm.clone()

    host_hm = batch["hm"].cpu().pin_memory()
    dev_hm = torch.empty_like(batch["hm"])
    for _ in range(warm):
        native(), composed(), clone_only(), ctdet_targets(boxes, classes, counts, C, H, W, M), dev_hm.copy_(host_hm, non_blocking=True)
    torch.cuda.synchronize()
    ev = {k: [] for k in ("native", "composed", "clone", "targets", "h2d")}
    for _ in range(pairs):
        ev["native"].append(event_ms(native))
        ev["composed"].append(event_ms(composed))
        ev["clone"].append(event_ms(clone_only))
        ev["targets"].append(event_ms(lambda: ctdet_targets(boxes, classes, counts, C, H, W, M)))
        ev["h2d"].append(event_ms(lambda: dev_hm.copy_(host_hm, non_blocking=True)))
    torch.cuda.synchronize()
    ms = {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    composed_net = ms["composed"] - med["clone"]
    moved = 5 * hm.numel() * 4 + 2 * wh.numel() * 4
    res = {"shape": "N=%d C=%d %dx%d M=%d" % (N, C, H, W, M), "pairs": pairs,
           "native_fwd_bwd_ms": round(med["native"], 4), "composed_fwd_bwd_ms": round(float(np.median(composed_net)), 4),
           "composed_over_native": round(float(np.median(composed_net)) / med["native"], 2),
           "native_below_composed_in_every_pair": bool(np.all(ms["native"] < composed_net)),
           "native_max_ms": round(float(ms["native"].max()), 4), "composed_min_ms": round(float(composed_net.min()), 4),
           "native_bytes_moved_mb": round(moved / 1e6, 1), "native_gb_per_s": round(moved / med["native"] / 1e6, 1),
           "targets_launch_ms": round(med["targets"], 4), "hm_host_to_device_ms": round(med["h2d"], 4)}
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
