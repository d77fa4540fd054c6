"""Timing of the multi-scale merge (codenet_merge.hip, cdn_ctdet_merge_scales: post_process + per-class soft-NMS + the
max_per_image cut, one workgroup per image) for B = 64 images x S = 5 scales x K = 100 detections, 20 classes, on
CLUSTERED boxes (five objects per image: long soft-NMS chains, many discards) and on SPREAD boxes (little overlap), with
HIP events; beside it, in the same process, cdn_ctdet_decode for the 320-image batch that feeds it.  GPU only."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from codenet_amd import harness

SCALES = [0.5, 0.75, 1.0, 1.25, 1.5]


def timed(fn, steps=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[0]


def detections(B, S, K, clustered, seed, nclass=None):
    rng = np.random.default_rng(seed)
    d = np.zeros((B, S, K, 6), dtype=np.float32)
    for b in range(B):
        centres = rng.uniform(16, 112, (5, 2))
        for s in range(S):
            c = centres[rng.integers(0, 5, K)] + rng.normal(0, 1.5, (K, 2)) if clustered else rng.uniform(4, 124, (K, 2))
            wh = (24 if clustered else 6) * np.exp(rng.normal(0, 0.1, (K, 2)))
            sc = np.sort(np.exp(rng.uniform(np.log(1e-3), 0, K)))[::-1]
            cls = rng.integers(0, nclass or (5 if clustered else 20), K)
            d[b, s] = np.concatenate([c - wh / 2, c + wh / 2, sc[:, None], cls[:, None]], 1)
    return torch.from_numpy(d).cuda()


def main():
    B, S, K = 64, 5, 100
    metas = [[{"c": np.array([250.0 * sc, 187.5 * sc], dtype=np.float32), "s": 500.0, "out_height": 128,
               "out_width": 128} for sc in SCALES] for _ in range(B)]
    meta = harness.scale_metas(metas, SCALES).cuda()
    bufs = harness.ProcessBuffers()
    res = {"shape": "B=%d S=%d K=%d classes=20" % (B, S, K)}
    for name, clustered, nclass in (("clustered", True, None), ("clustered_one_class", True, 1), ("spread", False, None)):
        dets = detections(B, S, K, clustered, 1, nclass)
        for nms in (True, False):
            med, best = timed(lambda: harness.merge_scales_native(dets, meta, SCALES, 20, nms=nms, bufs=bufs, raw=True))
            res["merge_%s_%s_ms" % (name, "nms" if nms else "no_nms")] = round(med, 4)
        raw = harness.merge_scales_native(dets, meta, SCALES, 20, nms=True, bufs=bufs, raw=True)
        torch.cuda.synchronize()
        res["%s_rows_discarded_per_image" % name] = round(float((raw[3] - raw[4]).sum().item()) / B, 1)
        res["%s_largest_class_rows" % name] = int(raw[3].max().item())
    g = torch.Generator().manual_seed(1)
    logits = (torch.randn(B * S, 20, 128, 128, generator=g) * 0.05 - 1.75).cuda()
    wh = (torch.rand(B * S, 2, 128, 128, generator=g) * 9).cuda()
    reg = torch.rand(B * S, 2, 128, 128, generator=g).cuda()
    sig = torch.empty_like(logits)
    med, best = timed(lambda: harness.ctdet_decode_native(logits, wh, reg=reg, K=K, apply_sigmoid=True, heat_out=sig,
                                                          bufs=bufs))
    res["decode_320_images_ms"] = round(med, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
