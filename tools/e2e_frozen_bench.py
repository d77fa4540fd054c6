"""Serving mode of the whole W4A8 network (every QuantAct frozen, byte codes from the stem to the heads) as one HIP
graph, batch 64 at 512x512: ms per batch.  The calibration is short (settle 30): an A/B timing tool, the judged
number comes from bench.py's `e2e.frozen` leg (settle 300).  GPU only.
    python tools/e2e_frozen_bench.py [--steps 20] [--stages-only] [--classes 80] [--ab-heads 10]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from codenet_amd import harness, pipeline


def heads_ab(a, model, twin, images, replay):
    """The serving graph with the heads on byte codes against the same calibrated network with the heads on the expanded
    codes: a.ab_heads interleaved pairs of a.steps replays each."""
    twin.load_state_dict(model.state_dict())
    pipeline.set_running_stat(twin, False)
    twin.enable_fused(frozen_codes=True)
    twin._plan(images)                                     # (builds the schedule objects)
    mods = {h: getattr(twin, h) for h in twin.heads}
    twin._fheads = pipeline.FusedHeads(mods, small_tail=False)
    twin._fzheads = pipeline.FusedHeads(mods, small_tail=False)
    twin.__dict__["_plans"].clear()
    plans = {"byte_heads": model._plan(images), "expanded": twin._plan(images)}
    legs = {"byte_heads": replay, "expanded": harness.capture_process(twin, images)}
    for _ in range(5):
        legs["expanded"]()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(a.ab_heads):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
    out = {"classes": a.classes, "batch": a.batch, "pairs": a.ab_heads, "plans": plans,
           "pairs_won_by_byte_heads": sum(f < u for f, u in zip(ms["byte_heads"], ms["expanded"])),
           "overflow": bool(model.frozen_overflowed())}
    for k, v in ms.items():
        out[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--no-merge-params", action="store_true", help="A/B: the stages' and the heads' QuantAct parameters in "
                    "launches of their own instead of in the backbone's first launch")
    ap.add_argument("--stages-only", action="store_true", help="backbone on the fp32 kernels, stages on byte codes")
    ap.add_argument("--w2", action="store_true", help="CoDeNet2x (BASELINE cfg4's model; batch 32 per GPU there): stage 0 on "
                    "the fp32 frozen schedule, everything else on byte codes")
    ap.add_argument("--classes", type=int, default=20, help="outputs of the hm head (Pascal VOC 20, COCO 80)")
    ap.add_argument("--ab-heads", type=int, default=0, metavar="PAIRS",
                    help="A/B: the heads on the byte codes of the last stage (the plan's third member) against the heads on "
                         "the expanded codes (FusedHeads(small_tail=False)), PAIRS interleaved pairs of the captured graphs")
    ap.add_argument("--w-bit", type=int, default=4, help="weight width of the quantised model (8: W8A8)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model = harness.create_model(heads={"hm": a.classes, "wh": 2, "reg": 2}, quantize=True, w2=a.w2, w_bit=a.w_bit).to(dev)
    twin = copy.deepcopy(model) if a.ab_heads else None
    model.merge_frozen_params = not a.no_merge_params
    model.enable_fused()
    images = torch.randn(a.batch, 3, 512, 512, generator=torch.Generator().manual_seed(0)).to(dev)
    report = pipeline.prepare_serving(model, images, settle=30, margin=0.02)
    with torch.no_grad():
        model.enable_fused(frozen_codes=True, frozen_backbone=not a.stages_only)
        replay = harness.capture_process(model, images)
        for _ in range(5):
            replay()
        torch.cuda.synchronize()
        model.frozen_overflowed()
        if a.ab_heads:
            return heads_ab(a, model, twin, images, replay)
        res = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(a.steps):
                replay()
            torch.cuda.synchronize()
            res.append((time.perf_counter() - t0) / a.steps * 1e3)
    print(json.dumps({"ms_per_batch": [round(r, 4) for r in res], "overflow": bool(model.frozen_overflowed()),
                      "byte_backbone": model._fzbackbone is not None, "calibration_clean": report.get("clean"),
                      "model": "CoDeNet2x" if a.w2 else "CoDeNet1x", "batch": a.batch}))


if __name__ == "__main__":
    main()
