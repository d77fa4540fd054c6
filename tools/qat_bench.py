"""What the component benches of the training step share (heads_train_bench.py, units_train_bench.py, stem_train_bench.py,
fp32_block_bench.py): the interleaved A/B regions of a native path against its module path, their common report, and the
timer of a captured QAT step.  Imported as ``import qat_bench`` by a tool run as ``python tools/X.py`` or with tools/ on
sys.path.  GPU only."""
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def bn_eval(net):
    """BatchNorm on its running statistics, as in the QAT step; the rest of `net` stays as it is."""
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    return net


def timed(fn):
    """One call of fn between two HIP events -> the pair (read it with a.elapsed_time(b) after a synchronize)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def interleaved_ab(step, restore, regions, warm=3):
    """step(native) is one region, native path (True) or module path (False); `warm` of each, then `regions` pairs timed in
    the order a, b, a, b, ... so that clock and temperature drift hit both alike; restore() puts the switch back whatever
    happens.  -> (native, module): two arrays of milliseconds."""
    try:
        for _ in range(warm):
            step(True), step(False)
        torch.cuda.synchronize()
        ev = {True: [], False: []}
        for _ in range(regions):
            ev[True].append(timed(lambda: step(True)))
            ev[False].append(timed(lambda: step(False)))
        torch.cuda.synchronize()
    finally:
        restore()
    return tuple(np.array([a.elapsed_time(b) for a, b in ev[k]]) for k in (True, False))


def report(nat_ms, mod_ms, moved=None, ratio_digits=2):
    """The keys every A/B bench prints: medians, their ratio, whether native < module held in every pair, min and max of
    both and, for `moved` algorithmic bytes of the native path, megabytes and GB/s at its median."""
    nat, mod = float(np.median(nat_ms)), float(np.median(mod_ms))
    res = {"regions": len(nat_ms), "native_fwd_bwd_ms": round(nat, 4), "module_fwd_bwd_ms": round(mod, 4),
           "module_over_native": round(mod / nat, ratio_digits),
           "native_below_module_in_every_pair": bool(np.all(nat_ms < mod_ms)),
           "native_min_ms": round(float(nat_ms.min()), 4), "native_max_ms": round(float(nat_ms.max()), 4),
           "module_min_ms": round(float(mod_ms.min()), 4), "module_max_ms": round(float(mod_ms.max()), 4)}
    if moved is not None:
        res.update(native_bytes_moved_mb=round(moved / 1e6, 1), native_gb_per_s=round(moved / nat / 1e6, 1))
    return res


def replay_s(step, steps):
    """Seconds per replay of a pipeline.GraphedTrainStep: 3 replays, then wall clock around `steps` of them."""
    for _ in range(3):
        step.graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step.graph.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def ctdet_setup(batch, res):
    """(crit, targets): losses.CtdetLoss with the default options and fixed targets of 25-50 objects per image on the
    res / 4 maps -- what every captured-step timing of these tools trains against."""
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
    return crit, targets


def captured_step(net, example, config, res=512, steps=20):
    """The captured QAT step of `net` (a pipeline.Detection* wrapper) on the input `example` -- losses.CtdetLoss on fixed
    targets at res / 4, fused capturable Adam -- as pipeline.GraphedTrainStep accepts it without `unvalidated`, timed over
    `steps` replays.  Prints and returns one JSON line under `config`."""
    from codenet_amd import pipeline
    batch = example.shape[0]
    crit, targets = ctdet_setup(batch, res)
    opt = torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device="cuda"), capturable=True, fused=True)
    step = pipeline.GraphedTrainStep(net, opt, lambda n, f: crit(n(f), targets)[0], (example,), warmup=3)
    dt = replay_s(step, steps)
    out = {"config": config, "ms_per_step": round(dt * 1e3, 3), "images_per_s": round(batch / dt, 1),
           "loss": float(step.loss.detach())}
    print(json.dumps(out))
    return out
