#!/usr/bin/env python
"""bench.py -- images/sec of CoDeNet's deform hot path (the three up-sampling stages,
``deconv_layers``) on MI355X, plus the whole-network figure it is a part of.

    python bench.py --gpus N --steps K --warmup W

N > 1: either launched by ``python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`` (the
driver's way: RANK / LOCAL_RANK / WORLD_SIZE in the environment), or run directly -- then this process starts
the N ranks itself as CHILD processes before it has touched the GPU, waits for them and exits with their
code.  The run fails (non-zero exit) unless exactly N ranks joined the RCCL process group.

A "step" is one pass of the hot path over one batch of synthetic images whose stage-0 input is already
resident in HBM: scale 1x1 -> QuantAct -> bilinear-gather depthwise 3x3 -> QuantAct -> pointwise 1x1 + folded
BN -> ReLU -> (range of the) QuantAct, three times, handing the channels-last half-resolution tensor + its
QuantAct state to the consumer (the native detection heads).  The NCHW / up-sampled copy a PyTorch consumer
would need (``unpack``) is timed and reported separately (`with_unpack`), not part of the step.

Default workload = BASELINE.json configs[2] ("cfg3"): CoDeNet1x config-c, 512x512, W4A8, batch 64 per GPU
(weak scaling: every rank processes its own images; start-up RCCL broadcast of weights / BN statistics /
QuantAct ranges; in the `e2e` leg a per-batch all_gather of the detections [B,100,6]).  --config cfg4 =
configs[3] (CoDeNet2x, 32 images per GPU, global 256 at 8 GPUs), --config cfg2 = configs[1] (256x256 fp32,
batch 32).

A plain run sets up, warms up (--warmup steps, then min(--steps, SETTLE_STEPS) untimed steps), times exactly --steps
steps (one region), writes the last step's outputs when --dump-outputs DIR is given and prints ONE JSON line on rank 0
with the headline (metric, value, unit, ms_per_step, ...).  --full adds everything else the benchmark measures, as extra
keys of the same line (and 15 regions by default):
  roofline          dominant kernel family (the gather), live HIP-event timing on its launch stream
  with_unpack, frozen_int8, configs   the hand-over copy, the frozen byte-code schedule, the other BASELINE configs
  cpu_baseline      the CPU oracle timed on a bounded sample of the same hot-path workload (N = 1 only)
  e2e               whole network (native backbone + stages + heads) + native ctdet_decode as one HIP graph
  cpu_baseline_e2e  whole model + decode on the CPU oracle path, batch 1 and 8, all cores and 1 thread
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)
F32_MFMA_PEAK_TF = 157.3

PRESETS = {
    "cfg2": dict(res=256, batch=32, w2=False, fp32=True),     # BASELINE configs[1]
    "cfg3": dict(res=512, batch=64, w2=False, fp32=False),    # BASELINE configs[2] (the metric's config)
    "cfg4": dict(res=512, batch=32, w2=True, fp32=False),     # BASELINE configs[3]: 256 images over 8 GPUs
}

# --dump-outputs: an output of more elements is written as this many of them (16 MB of float32 per array; the
# default step's output has 16.8 M elements)
DUMP_SAMPLE = 1 << 22

# plain run: at most this many untimed steps between the warm-up and the one timed region (50 ms of the default step)
SETTLE_STEPS = 200


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--full", action="store_true",
                    help="also measure and report everything beyond the headline: roofline and per-kernel times, "
                         "with_unpack, frozen_int8, e2e, configs, the CPU baselines (each --no-* option below skips "
                         "one of them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed step returned in its last step as DIR/<name>.npy "
                         "(float32; a fixed seeded sample of an output larger than %d elements)" % DUMP_SAMPLE)
    ap.add_argument("--regions", type=int, default=None,
                    help="the timed K-step region (barrier + synchronize on both sides) is run this many times "
                         "back to back; the headline ms_per_step is the MEDIAN region, min / max are reported "
                         "(default 1, so that --steps is the number of timed steps; 15 with --full)")
    ap.add_argument("--config", choices=sorted(PRESETS), default=None,
                    help="preset of --res/--batch/--w2/--fp32 (default: cfg3 values)")
    ap.add_argument("--batch", type=int, default=None, help="images per GPU per step")
    ap.add_argument("--res", type=int, default=None)
    ap.add_argument("--w2", action="store_true", default=None, help="CoDeNet2x (stage-0 C = 2153)")
    ap.add_argument("--fp32", action="store_true", default=None, help="fp32 hot path instead of W4A8")
    ap.add_argument("--frozen", action="store_true",
                    help="freeze QuantAct ranges (default: reference-faithful running ranges)")
    ap.add_argument("--path", choices=["fused", "modules"], default="fused",
                    help="fused: per-stage fused kernel schedule (codenet_fused.hip); modules: the "
                         "reference-shaped nn.Module chain, one op at a time")
    ap.add_argument("--no-graph", action="store_true", help="fused path: launch eagerly instead of "
                    "replaying a captured HIP graph")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="skip the whole-network leg")
    ap.add_argument("--no-config-legs", action="store_true",
                    help="skip the `configs` block (the other BASELINE configs -- cfg2, cfg4 per rank, the cfg5 QAT step -- "
                         "timed in the default single-GPU run)")
    ap.add_argument("--no-live-pmc", action="store_true",
                    help="do not measure roofline.traffic in this run (two short rocprofv3 --pmc child runs of the same "
                         "workload, N = 1 only); the committed profiles/ numbers are used instead")
    ap.add_argument("--cpu-images", type=int, default=2)
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="nccl == RCCL on ROCm; gloo only with --plumbing-only")
    ap.add_argument("--plumbing-only", action="store_true",
                    help="no kernels are launched and no rate is reported: exercises the launcher, the rendezvous, "
                         "the start-up broadcast, the image sharding and the detections gather on CPU tensors "
                         "(tests/test_distributed_cpu.py)")
    a = ap.parse_args(argv)
    base = dict(PRESETS[a.config or "cfg3"])
    for k in ("batch", "res", "w2", "fp32"):
        if getattr(a, k) is None:
            setattr(a, k, base[k])
    if a.regions is None:
        a.regions = 15 if a.full else 1
    if a.backend == "gloo" and not a.plumbing_only:
        ap.error("--backend gloo runs no kernels: use it with --plumbing-only")
    return a


# ---- launcher --------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _visible_gpus():
    """GPU count from the KFD topology in sysfs (nodes with SIMDs), narrowed by HIP_/ROCR_VISIBLE_DEVICES;
    None when sysfs does not say -- the ranks then fail by themselves (main() exits 3 unless N ranks joined)."""
    import glob
    n = 0
    props = glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")
    if not props:
        return None
    for f in props:
        try:
            for line in open(f):
                k, _, v = line.partition(" ")
                if k == "simd_count" and int(v) > 0:
                    n += 1
        except (OSError, ValueError):
            return None
    for var in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([t for t in v.split(",") if t.strip()]))
    return n


def launch_ranks(args):
    """Start N ranks as child processes (torch.distributed.run, one rank per GPU) BEFORE this process touches
    the GPU, and return their exit code.  Never exec: a child is spawned and waited for."""
    if not args.plumbing_only:
        have = _visible_gpus()                  # sysfs only: the launcher parent never calls into HIP / torch.cuda
        if have is not None and have < args.gpus:
            print("bench.py: --gpus %d but only %d GPU(s) visible" % (args.gpus, have), file=sys.stderr)
            return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC (RCCL needs it on this host driver)
    return subprocess.call(cmd, env=env)



# ---- live HBM traffic of the step (roofline.traffic measured IN THIS RUN) -------------------------

FAMILY_OF = (("dw0p_kernel", "dw"), ("dw2u_kernel", "dw"), ("dw2_kernel", "dw"), ("pwi8_kernel", "pointwise"), ("pwi8s_kernel", "pointwise"),
             ("pw3_kernel", "pointwise"), ("pws_kernel", "pointwise"), ("pwq8_kernel", "pointwise"), ("pwb3_kernel", "pointwise"),
             ("pwd3_kernel", "pointwise"), ("scale_n", "scale"), ("unpack_kernel", "unpack"), ("expand8", "unpack"))


def _family_bytes(per_kernel_bytes):
    fam = {}
    for name, b in per_kernel_bytes.items():
        for tag, f in FAMILY_OF:
            if tag in name:
                fam[f] = fam.get(f, 0) + int(b)
                break
    return fam


def live_pmc_traffic(args):
    """HBM bytes per step by kernel family, measured now: this process (which has NOT touched the GPU yet) starts two
    short child runs of the same workload under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` / `--pmc WRITE_SIZE`
    (separate passes, no trace domain beyond the kernel trace; eager launches, 3 steps) and reads the steady-state
    iterations with tools/pmc_steady.py's rules (read bytes = 2 x FETCH_SIZE on gfx950, MI355X_MICROARCH.md).  Returns
    None -- and the committed profiles/ numbers are used -- when rocprofv3 is missing, this process is itself being
    profiled, or anything fails; never raises."""
    import shutil
    import tempfile
    try:
        exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
        if exe is None or args.path != "fused" or not os.path.exists("/dev/kfd"):
            return None
        if any("rocprof" in os.environ.get(v, "").lower() for v in ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "HSA_TOOLS_LIB")):
            return None                              # already under a profiler: no nested profiling
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import pmc_steady
        base = [sys.executable, os.path.abspath(__file__), "--full", "--steps", "3", "--warmup", "2", "--no-graph",
                "--no-cpu-baseline", "--no-e2e", "--no-config-legs", "--no-live-pmc", "--regions", "1", "--batch", str(args.batch),
                "--res", str(args.res)] + (["--w2"] if args.w2 else []) + (["--fp32"] if args.fp32 else []) + \
               (["--frozen"] if args.frozen else [])
        per = {}
        t_start = time.perf_counter()
        with tempfile.TemporaryDirectory(prefix="cdn_pmc_", dir="/tmp") as tmp:
            env = dict(os.environ, TMPDIR="/tmp")
            for key, counter, mul in (("read", "FETCH_SIZE", 2048.0), ("write", "WRITE_SIZE", 1024.0)):
                # bounded: the two passes together get ~4 minutes (the first python start on a fresh box pages the
                # framework in for 1-2 minutes); a slow first pass cancels the second -> committed numbers instead
                left = 240.0 - (time.perf_counter() - t_start)
                if left < 60.0:
                    return None
                d = os.path.join(tmp, key)
                # own process group: on a timeout the profiler AND the bench under it are ended (a survivor would run
                # beside the timed region) -- by exact group id, never by pattern
                proc = subprocess.Popen([exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", d, "--"]
                                        + base, cwd="/tmp", env=env, stdout=subprocess.DEVNULL,
                                        stderr=subprocess.DEVNULL, start_new_session=True)
                try:
                    rc = proc.wait(timeout=min(left, 170.0))
                except subprocess.TimeoutExpired:
                    import signal
                    try:
                        os.killpg(proc.pid, signal.SIGKILL)
                    except OSError:
                        pass
                    proc.wait()
                    return None
                if rc != 0:
                    return None
                rows, spans = pmc_steady.iterations(pmc_steady.load(d, counter),
                                                    "frozen_params_kernel" if args.frozen and not args.fp32 else "scale_n",
                                                    1 if (args.frozen and not args.fp32) else 3, 2,
                                                    ["__amd_rocclr", "at::native"])
                for lo, hi in spans:
                    for name, v in rows[lo:hi]:
                        k = pmc_steady.short(name)
                        per[k] = per.get(k, 0.0) + v * mul / len(spans)
        fam = _family_bytes(per)
        return fam if fam.get("dw") and fam.get("pointwise") else None
    except (Exception, SystemExit):      # noqa: BLE001 -- a measurement aid must never take the benchmark down
        return None



def fused_algorithmic_bytes(shapes, batch, frozen=False, chain_parts=None):
    """ALGORITHMIC bytes per step of the fused schedule by kernel family: stages >= 1 read
    their input at stored (half) resolution, the up-sampling is folded into addressing; the frozen schedule moves byte
    codes everywhere except the stage-0 input and the scale planes.  chain_parts (fp32 model, round 6): per stage the
    number of partial-sum planes its pointwise epilogue leaves for the next stage's scale prediction -- that stage then has
    no scale launch: its pointwise writes, and the next gather reads, parts x pixels x 4 bytes instead."""
    alg = {"scale": 0, "dw": 0, "pointwise": 0, "unpack": 0}
    for i, (C, Co, H, W) in enumerate(shapes):
        HWs = H * W // (1 if i == 0 else 4)
        if chain_parts and i > 0 and chain_parts[i - 1]:
            alg["dw"] += (C * HWs + chain_parts[i - 1] * HWs + C * H * W) * 4 * batch
            alg["pointwise"] += ((C + Co) * H * W + (chain_parts[i] if i < len(chain_parts) else 0) * H * W) * 4 * batch
            continue
        if chain_parts and chain_parts[i]:
            alg["pointwise"] += chain_parts[i] * H * W * 4 * batch
        if frozen:
            xb = 4 if i == 0 else 1
            alg["scale"] += (C * xb + 4) * HWs * batch
            alg["dw"] += (C * HWs * xb + HWs * 4 + C * H * W) * batch
            alg["pointwise"] += (C + Co) * H * W * batch
            continue
        alg["scale"] += (C + 1) * HWs * 4 * batch
        alg["dw"] += (C * HWs + HWs + C * H * W) * 4 * batch
        alg["pointwise"] += (C + Co) * H * W * 4 * batch
    C, Co, H, W = shapes[-1]
    alg["unpack"] = (Co * H * W + 4 * Co * H * W) * 4 * batch
    return alg


def kernel_event_durations(step_fn, steps, keep, durs):
    """`steps` eager steps with the library's HIP-event pairs around every kernel (recorded on the launch stream);
    fills durs[(family, (tag,))] -> [ms per launch]."""
    import ctypes
    import torch
    from codenet_amd import _native
    lib = _native.lib()
    kname = {0: "scale", 1: "dw", 2: "pointwise", 3: "unpack"}
    lib.cdn_profile_enable(1)
    for _ in range(steps):
        step_fn()
    torch.cuda.synchronize()
    cap = steps * 16
    ids = (ctypes.c_int * cap)()
    tags = (ctypes.c_int * cap)()
    ms = (ctypes.c_float * cap)()
    n = lib.cdn_profile_read(cap, ids, tags, ms)
    lib.cdn_profile_enable(0)
    for i in range(n):
        name = kname.get(ids[i], "other")
        if keep(name):
            durs.setdefault((name, (tags[i],)), []).append(ms[i])


def committed_step_traffic(preset):
    """HBM bytes per step of a preset's fused running-range step from the newest committed PMC collection
    (profiles/rNN/pmc_steady_<preset>.json: steady-state iterations of `bench.py --config <preset> --no-graph` under
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, FETCH_SIZE doubled; the hand-over kernels unpack / expand8 excluded)."""
    for rnd in ("r06", "r05", "r04"):
        try:
            pm = json.load(open(os.path.join(ROOT, "profiles", rnd, "pmc_steady_%s.json" % preset)))
        except (OSError, ValueError):
            continue
        mb = sum(v["read"] + v["write"] for k, v in pm["per_kernel_MB"].items()
                 if "unpack" not in k and "expand8" not in k)
        return int(mb * 2 ** 20), "committed: profiles/%s/pmc_steady_%s.json" % (rnd, preset)
    return None, None


def hot_path_config_leg(preset, dev, steps, warmup, regions=5):
    """One more BASELINE config through the SAME measurement as the headline (VERDICT r4 "next" #1a): the preset's
    fused running-range step as a replayed HIP graph, `regions` regions of `steps` steps between synchronisations
    (median), per-kernel HIP events on the launch stream, algorithmic bytes of the fused definition and the
    committed PMC traffic of the same command."""
    import torch
    from codenet_amd import pipeline
    p = PRESETS[preset]
    quantized = not p["fp32"]
    net = pipeline.build_hot_path(w2=p["w2"], quantized=quantized, seed=317).to(dev)
    if quantized:
        pipeline.set_running_stat(net, True)
    x = pipeline.make_input(p["batch"], p["res"], p["w2"], seed=0, device=dev)
    fused = pipeline.FusedHotPath(net.deconv_layers)
    for _ in range(max(1, warmup // 2)):
        fused.forward_nhwc(x)
    step = fused.capture(x, unpack=False)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    region_s = []
    for _ in range(regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step()
        torch.cuda.synchronize()
        region_s.append(time.perf_counter() - t0)
    region_s.sort()
    ms = region_s[len(region_s) // 2] / steps * 1e3
    assert torch.isfinite(out).all()
    durs = {}
    kernel_event_durations(lambda: fused.forward_nhwc(x), steps, lambda nm: nm != "unpack", durs)
    per_kernel = {}
    for (name, _tag), v in durs.items():
        per_kernel[name] = per_kernel.get(name, 0.0) + sum(v) / steps
    shapes = pipeline.stage_shapes(p["res"], p["w2"])
    parts = [sb["parts"] for sb in fused._bufs["stages"]]
    alg = fused_algorithmic_bytes(shapes, p["batch"], chain_parts=parts if any(parts) else None)
    alg_step = alg["scale"] + alg["dw"] + alg["pointwise"]
    dominant = max(per_kernel, key=per_kernel.get)
    traffic, source = committed_step_traffic(preset)
    fam = {k: {"algorithmic_bytes_per_step": alg[k], "ms_per_step_in_kernel": per_kernel[k],
               "achieved": alg[k] / (per_kernel[k] * 1e-3) / 1e9,
               "frac": alg[k] / (per_kernel[k] * 1e-3) / 1e9 / HBM_PEAK_GBS}
           for k in ("dw", "pointwise", "scale") if per_kernel.get(k)}
    roof = {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBS, "kernel_family": dominant,
            "achieved": fam[dominant]["achieved"], "frac": fam[dominant]["frac"],
            "algorithmic_bytes_per_step": alg[dominant], "ms_per_step_in_kernel": per_kernel[dominant],
            "families": fam,
            "step": {"algorithmic_bytes": alg_step, "achieved": alg_step / ms / 1e6,
                     "frac": alg_step / ms / 1e6 / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": source,
                     "traffic_frac": (traffic / ms / 1e6 / HBM_PEAK_GBS) if traffic else None}}
    if p["fp32"]:
        # the fp32 stage-0 pointwise (K = 1024) sits on the f32-MFMA roofline, not on HBM
        C, Co, H, W = shapes[0]
        pw0 = [sum(v) / len(v) for (nm, tag), v in durs.items() if nm == "pointwise" and tag == (H,)]
        if pw0:
            tf = 2.0 * C * Co * H * W * p["batch"] / (pw0[0] * 1e-3) / 1e12
            roof["stage0_pointwise_mfma"] = {"bound": "mfma", "unit": "TFLOP/s", "peak": F32_MFMA_PEAK_TF,
                                             "achieved": tf, "frac": tf / F32_MFMA_PEAK_TF, "us_per_launch": pw0[0] * 1e3}
    del step, fused, net, x
    torch.cuda.empty_cache()
    return {"workload": "CoDeNet%s %dx%d %s, batch %d per GPU, the three deform stages (the headline's step), fused "
                        "schedule, HIP-graph replay" % ("2x" if p["w2"] else "1x", p["res"], p["res"],
                                                        "fp32" if p["fp32"] else "W4A8 (running QuantAct ranges)",
                                                        p["batch"]),
            "ms_per_step": ms, "images_per_s": p["batch"] / ms * 1e3, "chained_scale_planes": parts,
            "regions": {"n": regions, "steps_each": steps, "ms_per_step_min": region_s[0] / steps * 1e3,
                        "ms_per_step_max": region_s[-1] / steps * 1e3},
            "roofline": roof,
            "kernel_ms_per_launch": {"%s@%d" % (nm, tag[0]): round(sum(v) / len(v), 5)
                                     for (nm, tag), v in sorted(durs.items())}}


def qat_step_leg(dev, steps=20):
    """BASELINE configs[4] ("cfg5"): the W4A8 quant-aware training step of quant_main.py restricted to the hot path --
    forward + backward + Adam over the three deform stages, batch 32 (lib/opts.py:91), 512x512, one HIP graph
    (tools/train_step_bench.py's step) -- with its algorithmic bytes and the gather backward against the LDS-atomic
    rate that bounds it."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train_step_bench as T
    return T.measure(batch=32, res=512, steps=steps, graph=True)


# ---- CPU baselines (the only place bench.py touches oracle/) ------------------------------------------------

def cpu_baseline(args, net_cpu):
    """The CPU oracle (oracle/ -- the reference has no CPU deform conv) timed
    on a bounded sample: `cpu_images` images of the same workload through the same three stages
    in the reference's algorithmic form (im2col gather + per-group contraction in C/OpenMP,
    torch-CPU conv2d / fake-quant around it).  kind = "port"."""
    import torch
    import torch.nn.functional as F
    from codenet_amd import pipeline
    from oracle import dcn as O
    from oracle import quant as Q
    n = args.cpu_images
    x = pipeline.make_input(n, args.res, args.w2, seed=1)
    mods = list(net_cpu.deconv_layers)
    cores = torch.get_num_threads()
    O.lib()

    def run(x):
        if args.fp32:
            for i in range(0, len(mods), 4):
                op, bn = mods[i], mods[i + 1]
                r = Q.stage_fp32(x, op.conv_scale.weight, op.conv_scale.bias, op.conv.weight,
                                 op.conv_channel.weight)
                x = F.interpolate(torch.relu(bn(r["y"])), scale_factor=2, mode="nearest")
            return x
        for i in range(0, len(mods), 3):
            q = mods[i]
            bnm = q.quant_conv_channel_bn.bn
            bn = (bnm.weight, bnm.bias, bnm.running_mean, bnm.running_var, bnm.eps)
            r = Q.stage_w4a8(x, q.quant_conv_scale.weight, q.quant_conv_scale.bias,
                             q.quant_deform_conv.weight, q.quant_conv_channel_bn.conv.weight, bn,
                             Q.QuantActState(), Q.QuantActState())
            y = Q.QuantActState()(torch.relu(r["y"]))
            x = F.interpolate(y, scale_factor=2, mode="nearest")
        return x

    # on many-core hosts a 16-thread pool (torch-CPU's small ops are slower on 128 threads than on 16);
    # `cores` is the thread count the reported leg used
    legs = {}
    with torch.no_grad():
        # (round 5: the all-cores leg on a >= 64-core host is oversubscribed noise -- 12 against 102 images/s on 128
        # threads in the driver's round-4 run -- and is no longer run; `cores` is what was used)
        for threads in ((16,) if cores > 32 else (cores,)):
            torch.set_num_threads(threads)
            O.set_threads(threads)
            run(x[:1])                       # warm caches / thread pools
            t0 = time.perf_counter()
            reps = 0
            while True:
                run(x)
                reps += 1
                if time.perf_counter() - t0 > 10.0 or reps >= 400:
                    break
            dt = time.perf_counter() - t0
            legs[threads] = (n * reps / dt, reps)
        # the scalar port's one-thread figure (SURVEY 8(d) asks for both ends): ONE image, bounded to ~5 s
        one = None
        if cores > 1:
            torch.set_num_threads(1)
            O.set_threads(1)
            run(x[:1])
            t0 = time.perf_counter()
            reps1 = 0
            while True:
                run(x[:1])
                reps1 += 1
                if time.perf_counter() - t0 > 5.0 or reps1 >= 100:
                    break
            one = reps1 / (time.perf_counter() - t0)
        torch.set_num_threads(cores)
        O.set_threads(cores)
    best = max(legs, key=lambda t: legs[t][0])
    return {"value": legs[best][0], "unit": "images/sec", "cores": best, "kind": "port",
            "legs": {"threads%d" % t: round(v[0], 3) for t, v in legs.items()},
            "one_thread": ({"value": round(one, 3), "unit": "images/sec", "cores": 1,
                            "sample": "single images for ~5 s on one thread"} if one else None),
            "sample": "%d x %d images, %s hot path, %dx%d, oracle C (OpenMP) + torch CPU"
                      % (legs[best][1], n, "fp32" if args.fp32 else "W4A8", args.res, args.res)}


def gpu_clock_state(index=0):
    """Shader / memory clock levels as sysfs shows them (read-only; None where not readable).  The in-kernel
    clock under load can sit below pp_dpm_sclk (MI355X_MICROARCH.md, DVFS give-back) -- context, not a correction."""
    import glob
    out = {}
    cards = sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))
    if not cards:
        return None
    base = os.path.dirname(cards[min(index, len(cards) - 1)])
    for key, fn in (("sclk", "pp_dpm_sclk"), ("mclk", "pp_dpm_mclk")):
        try:
            lines = [l.strip() for l in open(os.path.join(base, fn)) if l.strip()]
            cur = [l for l in lines if l.endswith("*")]
            out[key] = (cur[0] if cur else lines[-1]).rstrip("*").strip()
        except OSError:
            out[key] = None
    try:
        out["power_cap_w"] = int(open(glob.glob(os.path.join(base, "hwmon/hwmon*/power1_cap"))[0]).read()) / 1e6
    except (OSError, IndexError, ValueError):
        pass
    return out


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline_e2e(args, budget_s=4.0):
    """SURVEY.md section 8(d) CPU protocol: WHOLE-model forward + ctdet_decode (the body of
    CtdetDetector.process, lib/detectors/ctdet.py:29-46, timed like BaseDetector.run,
    lib/detectors/base_detector.py:93-155) on the host cores: the harness model on torch-CPU with the
    module-level ``deform_conv`` bound to the CPU oracle (the reference has no CPU deform conv), batch 1 and 8,
    all cores and 1 thread.  Bounded: every leg runs one warm-up forward at batch 1 and then whole batches until
    `budget_s` seconds have passed (at least one)."""
    import torch
    from codenet_amd import harness
    from codenet_amd.modules import dcn_deform_conv as M
    from codenet_amd.portable_quantizer import quant_modules as QM
    from oracle import dcn as O
    O.lib()
    saved = (M.deform_conv, QM.deform_conv)
    M.deform_conv = QM.deform_conv = O.deform_conv
    all_threads = torch.get_num_threads()
    legs = {}
    try:
        model = harness.create_model(w2=args.w2, quantize=not args.fp32)
        g = torch.Generator().manual_seed(0)
        # (>= 64 host cores: a 16-thread pool stands in for "all cores" -- torch-CPU's small ops are slower on 128
        # threads than on one; the driver's round-4 run: 7.9 against 31.9 images/s)
        for threads in ((16, 1) if all_threads > 32 else (all_threads, 1)):
            torch.set_num_threads(threads)
            O.set_threads(threads)                   # the oracle's OpenMP loops follow the same count
            for n in (1, 8):
                x = torch.randn(n, 3, args.res, args.res, generator=g)
                harness.process(model, x[:1], flip_test=False, native_decode=False)
                t0 = time.perf_counter()
                reps = 0
                while True:
                    harness.process(model, x, flip_test=False, native_decode=False)
                    reps += 1
                    if time.perf_counter() - t0 > budget_s:
                        break
                dt = time.perf_counter() - t0
                legs["batch%d_threads%d" % (n, threads)] = {
                    "images_per_s": round(n * reps / dt, 3), "ms_per_batch": round(dt / reps * 1e3, 1),
                    "batches": reps}
    finally:
        torch.set_num_threads(all_threads)
        O.set_threads(all_threads)
        M.deform_conv, QM.deform_conv = saved
    best = max(v["images_per_s"] for v in legs.values())
    return {"value": best, "unit": "images/sec", "kind": "port", "cores": (16 if all_threads > 32 else all_threads),
            "nproc": os.cpu_count(),
            "cpu_model": cpu_model_name(), "legs": legs,
            "sample": "CoDeNet%s %dx%d %s whole model + ctdet_decode on torch-CPU + the C/OpenMP oracle for the "
                      "deform conv; per leg one warm-up image, then whole batches for >= %.0f s"
                      % ("2x" if args.w2 else "1x", args.res, args.res, "fp32" if args.fp32 else "W4A8", budget_s)}


# ---- plumbing-only mode (CPU, gloo): launcher + collectives, no kernels ---------------------------------------

class _count_host_syncs:
    """Counts Tensor.item() / .tolist() / .cpu() calls (the host reads of a tensor) inside the block: the per-batch
    detections gather must make none when the shard sizes are known."""
    def __call__(self):
        return self

    def __enter__(self):
        import torch
        self.n = 0
        self._saved = {}
        for name in ("item", "tolist", "cpu"):
            orig = getattr(torch.Tensor, name)
            self._saved[name] = orig

            def wrap(t, *a, _o=orig, **k):
                self.n += 1
                return _o(t, *a, **k)
            setattr(torch.Tensor, name, wrap)
        return self

    def __exit__(self, *exc):
        import torch
        for name, orig in self._saved.items():
            setattr(torch.Tensor, name, orig)
        return False


def plumbing_only(args, world, rank):
    import torch
    import torch.distributed as dist
    from codenet_amd import pipeline
    if world > 1:
        dist.init_process_group(args.backend, rank=rank, world_size=world)
    joined = dist.get_world_size() if world > 1 else 1
    if joined != args.gpus:
        print("bench.py: --gpus %d but %d rank(s) joined" % (args.gpus, joined), file=sys.stderr)
        return 3
    net = pipeline.build_hot_path(w2=args.w2, quantized=not args.fp32, seed=317 if rank == 0 else 1000 + rank)
    nbytes = pipeline.broadcast_parameters(net, src=0)
    digest = torch.stack([v.double().sum() for v in net.state_dict().values() if v.dtype.is_floating_point])
    same = True
    if world > 1:
        parts = [torch.zeros_like(digest) for _ in range(world)]
        dist.all_gather(parts, digest)
        same = all(torch.equal(parts[0], p) for p in parts)
    lo, hi = pipeline.shard_range(world * args.batch + 1, rank, world)      # uneven on purpose
    dets = torch.full((hi - lo, 100, 6), float(rank))
    dets[:, 0, 0] = torch.arange(lo, hi, dtype=torch.float32)               # global image index
    counts = pipeline.exchange_shard_sizes(hi - lo)                          # once, at start-up
    syncs = _count_host_syncs()
    with syncs:
        allv = pipeline.gather_detections(dets, counts=counts)               # per batch: one collective, no host read
        even = pipeline.gather_detections(dets[:args.batch], counts=[args.batch] * world)
    ok_even = (even.shape[0] == world * args.batch)
    ok = (allv.shape[0] == world * args.batch + 1
          and torch.equal(allv[:, 0, 0], torch.arange(world * args.batch + 1, dtype=torch.float32)))
    if rank == 0:
        print(json.dumps({"plumbing_only": True, "n_gpus": joined, "backend": args.backend,
                          "broadcast_bytes": nbytes, "replicas_identical": bool(same),
                          "detections_gathered": list(allv.shape), "detections_in_rank_order": bool(ok),
                          "equal_shards_gathered": bool(ok_even), "shard_sizes": counts,
                          "host_syncs_in_gather": syncs.n, "value": None}))
    if world > 1:
        dist.destroy_process_group()
    return 0 if (same and ok and ok_even and syncs.n == 0) else 4


# ---- the measured run ----------------------------------------------------------------------------------------

def dump_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy in float32 (float64 kept).  An array of more than DUMP_SAMPLE
    elements is written flattened as DUMP_SAMPLE of its elements in index order, picked by a fixed seed: the same
    positions for the same shape in every run, so that two builds compare output for output."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > DUMP_SAMPLE:
            idx = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:DUMP_SAMPLE].sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        a = t.cpu().numpy()
        np.save(os.path.join(path, name + ".npy"), a if a.dtype == np.float64 else a.astype(np.float32))


def main():
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and env_world is None:
        sys.exit(launch_ranks(args))            # children do the work; nothing here has touched the GPU
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print("bench.py: --gpus %d but WORLD_SIZE %d" % (args.gpus, world), file=sys.stderr)
        sys.exit(2)
    if args.plumbing_only:
        sys.exit(plumbing_only(args, world, rank))
    # roofline.traffic measured in THIS run (N = 1): two short profiled child runs, started before this process
    # touches the GPU
    live_traffic = None
    if args.full and world == 1 and rank == 0 and not args.no_live_pmc and not args.no_graph:
        live_traffic = live_pmc_traffic(args)

    import torch
    import torch.distributed as dist
    torch.cuda.set_device(local_rank)          # before the process group: RCCL binds to the current device
    dev = torch.device("cuda", local_rank)
    if world > 1:
        dist.init_process_group("nccl", rank=rank, world_size=world)   # nccl == RCCL on ROCm
    # ranks seen by the collective itself (not the launcher's claim)
    seen = torch.ones(1, device=dev)
    if world > 1:
        dist.all_reduce(seen)
    n_seen = int(round(seen.item()))
    if n_seen != args.gpus:
        if rank == 0:
            print("bench.py: --gpus %d but %d rank(s) joined RCCL" % (args.gpus, n_seen), file=sys.stderr)
        sys.exit(3)

    from codenet_amd import ops, pipeline

    quantized = not args.fp32
    # rank 0 owns the weights; the other ranks start from different values and receive them
    net = pipeline.build_hot_path(w2=args.w2, quantized=quantized, seed=317 if rank == 0 else 1000 + rank)
    net_cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        import copy
        net_cpu = copy.deepcopy(net)
    net = net.to(dev)
    bcast_bytes = pipeline.broadcast_parameters(net, src=0)
    if quantized:
        pipeline.set_running_stat(net, not args.frozen)
    x = pipeline.make_input(args.batch, args.res, args.w2, seed=rank, device=dev)

    import ctypes
    from codenet_amd import _native
    fused = pipeline.FusedHotPath(net.deconv_layers) if args.path == "fused" else None
    # --frozen: the serving schedule (QuantAct.running_stat = False, byte codes in HBM) is the timed step
    frozen_main = bool(args.frozen and quantized and fused is not None)
    frz = pipeline.FrozenHotPath(net.deconv_layers) if (quantized and fused is not None) else None

    def eager_step():
        if frozen_main:
            return frz.forward_codes(x)[0]
        if fused is not None:
            return fused.forward_nhwc(x)[0]
        with torch.no_grad():
            return net(x)

    def eager_step_unpack():
        return frz(x) if frozen_main else fused(x)

    def barrier():
        if world > 1:
            dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize()

    if quantized and args.frozen:          # ranges must exist before they can be frozen
        pipeline.set_running_stat(net, True)
        for _ in range(3):
            (fused.forward_nhwc(x) if fused is not None else net(x))
        pipeline.set_running_stat(net, False)
    for _ in range(max(1, args.warmup // 2)):
        eager_step()
    use_graph = fused is not None and not args.no_graph
    if use_graph:
        step = frz.capture(x) if frozen_main else fused.capture(x, unpack=False)
    else:
        step = eager_step
    for _ in range(args.warmup):
        step()
    if not args.full:
        # the one timed region of a plain run must not start while the clocks still ramp up: right after a few ms of
        # warm-up a region reads ~0.4 % slower than the steady state the median of --full's regions gives.  One untimed
        # region of the same length first (at most SETTLE_STEPS); a fixed count, so that the last step's outputs are the
        # same in every run
        for _ in range(min(args.steps, SETTLE_STEPS)):
            step()
    barrier()
    # ---- timed regions: each is exactly K steps between barrier + synchronize; R of them back to back,
    #      MAX over ranks per region, headline = the median region (one region = ms_per_step * steps) ------
    names = {"scale", "dw", "pointwise", "quantact"}
    region_s = []
    with ops.KernelTimer(names if (fused is None and args.full) else set()) as kt:
        for _ in range(max(1, args.regions)):
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                out = step()
            barrier()
            region_s.append(time.perf_counter() - t0)
    tmax = torch.tensor(region_s, dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    region_s = sorted(tmax.tolist())
    dt = region_s[len(region_s) // 2] if len(region_s) % 2 else 0.5 * (region_s[len(region_s) // 2 - 1]
                                                                       + region_s[len(region_s) // 2])
    assert out.dtype == torch.int8 or torch.isfinite(out).all()
    if frozen_main:
        assert not frz.overflowed(), "a code left its frozen 8-bit grid: this batch needs the fp32 schedule"
    if args.dump_outputs and rank == 0:
        # what the timed step hands its caller, before any later leg overwrites it: the last stage's output and, on the
        # fused W4A8 schedules, the range of the QuantAct whose state travels with it (the heads quantise with it)
        arrays = {"output": out}
        if quantized and fused is not None:
            from codenet_amd.portable_quantizer.quant_modules import QuantAct
            act = [m for m in net.deconv_layers.modules() if isinstance(m, QuantAct)][-1]
            arrays["output_range"] = torch.cat([act.x_min.reshape(-1), act.x_max.reshape(-1)])
        dump_outputs(args.dump_outputs, arrays)

    # ---- the same step + the NCHW / up-sampled copy for a PyTorch consumer (reported separately) ---
    with_unpack_ms = None
    if args.full and fused is not None:
        if use_graph:
            step_u = frz.capture(x, codes_only=False) if frozen_main else fused.capture(x, unpack=True)
        else:
            step_u = eager_step_unpack
        for _ in range(5):
            step_u()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step_u()
        barrier()
        with_unpack_ms = (time.perf_counter() - t0) / args.steps * 1e3

    # ---- per-kernel durations: HIP events on the launch stream (fused path: the library's own
    #      event pairs around every kernel, K eager steps right after the timed region) ------------
    durs = {}
    if args.full and fused is not None and rank == 0:
        # `eager_step` is the TIMED step: until round 3 these steps also ran unpack_kernel (320 MB through the caches
        # between two steps), which made the kernels behind it 10-40 % slower than inside the timed region
        kernel_event_durations(eager_step, args.steps, lambda nm: nm != "unpack", durs)
        kernel_event_durations(eager_step_unpack, args.steps, lambda nm: nm == "unpack", durs)   # (`with_unpack`)
    elif args.full and rank == 0:
        durs = kt.durations_ms()

    # ---- "reported both running (reference-faithful) and frozen": the frozen byte-code schedule on the
    #      ranges the timed running steps left behind (same weights, same input), K graph replays ---------------
    frozen_leg = None
    if args.full and frz is not None and not frozen_main and use_graph:
        stepf = frz.capture(x)
        for _ in range(5):
            stepf()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            stepf()
        barrier()
        msf = (time.perf_counter() - t0) / args.steps * 1e3
        frozen_leg = {"ms_per_step": msf, "images_per_s": world * args.batch / msf * 1e3,
                      "overflow": bool(frz.overflowed()),
                      "what": "same three stages with QuantAct.running_stat = False (serving mode, not the reference's "
                              "default): byte codes in HBM, 3 launches per stage, bit-identical to the fp32 frozen schedule"}
        # the same schedule fed with BYTE CODES at stage 0 (what a frozen byte-code backbone hands over: layer4's
        # QuantAct codes, channels-last) instead of the fp32 NCHW tensor read twice
        if not args.w2:
            from codenet_amd.portable_quantizer.quant_modules import QuantAct
            act_in = QuantAct(8, quant_mode="asymmetric").to(dev)
            with torch.no_grad():
                xq = act_in(x)
                # (the running ranges are an EMA: let them settle on this input before they are frozen, or the
                # extreme elements of the batch land half an LSB outside the byte grid)
                pipeline.set_running_stat(net, True)
                for _ in range(300):
                    fused.forward_nhwc(xq)
                pipeline.set_running_stat(net, False)
            act_in.running_stat = False
            stq = act_in._device_state(dev).view(torch.float32)
            Nb, C0, H0, W0 = x.shape
            x8 = torch.round(stq[2] * xq - stq[3]).clamp_(-128, 127).to(torch.int8) \
                .permute(0, 2, 3, 1).reshape(Nb, H0 * W0, C0).contiguous()
            qptr = act_in._device_state(dev).data_ptr()
            stepc = frz.capture(x8, x_qstate=qptr, hw=(H0, W0))
            for _ in range(5):
                stepc()
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                stepc()
            barrier()
            msc = (time.perf_counter() - t0) / args.steps * 1e3
            frzc = pipeline.FrozenHotPath(net.deconv_layers, chain_scale=True)
            stepcc = frzc.capture(x8, x_qstate=qptr, hw=(H0, W0))
            for _ in range(5):
                stepcc()
            barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                stepcc()
            barrier()
            mscc = (time.perf_counter() - t0) / args.steps * 1e3
            frozen_leg["codes_in_chained_scale"] = {
                "ms_per_step": mscc, "images_per_s": world * args.batch / mscc * 1e3, "overflow": bool(frzc.overflowed()),
                "what": "as codes_in, with the scale prediction of stages 1-2 accumulated as exact integer sums in the "
                        "previous stage's pointwise epilogue (7 launches instead of 9; declared non-bit-identical "
                        "variant: the exact sum rounded once)"}
            frozen_leg["codes_in"] = {
                "ms_per_step": msc, "images_per_s": world * args.batch / msc * 1e3, "overflow": bool(frz.overflowed()),
                "what": "stage-0 input as int8 codes [N, H*W, C] of the backbone's last QuantAct + its state "
                        "(x_kind 2) instead of fp32 NCHW"}
            pipeline.set_running_stat(net, not args.frozen)

    # ---- whole network + native decode as one HIP graph (every rank; per-batch detections all_gather) ---
    e2e = None
    if args.full and not args.no_e2e and args.path == "fused":
        e2e = e2e_leg(args, dev, rank, world, local_rank, dt / args.steps * 1e3)

    # ---- the other BASELINE configs, timed by the same run (N = 1, default workload only): VERDICT r4 "next" #1a ----
    configs = None
    if args.full and rank == 0 and world == 1 and args.config is None and not args.no_config_legs \
            and args.path == "fused" \
            and (args.res, args.batch, args.w2, args.fp32, args.frozen) == (512, 64, False, False, False):
        configs = {}
        for key, fn in (("cfg2", lambda: hot_path_config_leg("cfg2", dev, args.steps, args.warmup)),
                        ("cfg4_rank", lambda: hot_path_config_leg("cfg4", dev, args.steps, args.warmup)),
                        ("cfg5_qat", lambda: qat_step_leg(dev))):
            try:
                configs[key] = fn()
            except Exception as exc:          # noqa: BLE001 -- reported in the JSON line, the headline stands
                configs[key] = {"error": "%s: %s" % (type(exc).__name__, exc)}
            torch.cuda.empty_cache()

    if args.full and rank == 0:
        per_kernel = {}
        for (name, tag), v in durs.items():
            per_kernel.setdefault(name, 0.0)
            per_kernel[name] += sum(v) / args.steps          # ms per step in this kernel
        per_launch = {"%s@%s" % (name, "x".join(str(t) for t in tag)): round(sum(v) / len(v), 5)
                      for (name, tag), v in sorted(durs.items())}
        in_step = {k: v for k, v in per_kernel.items() if k != "unpack"}
        dominant = max(in_step, key=in_step.get)
        _, per_stage = pipeline.algorithmic_bytes(args.batch, args.res, args.w2)
        alg = {"scale": 0, "dw": 0, "pointwise": 0}
        for v in per_stage.values():
            for k in alg:
                alg[k] += v[k]
        shapes = pipeline.stage_shapes(args.res, args.w2)
        if fused is not None:
            parts = [sb.get("parts", 0) for sb in getattr(fused, "_bufs", None)["stages"]] if getattr(fused, "_bufs", None) else []
            alg = fused_algorithmic_bytes(shapes, args.batch, frozen_main, chain_parts=parts if any(parts) else None)
        flops_pw = sum(2.0 * C * Co * H * W * args.batch
                       for (C, Co, H, W) in pipeline.stage_shapes(args.res, args.w2))
        # The fused schedules' pointwise kernels (int8 MFMA on codes / the bf16 split) keep the matrix cores 6-12 % busy
        # (profiles/r03/pmc_summary.txt): they stream their operand once and are HBM kernels like the gather -- priced
        # against HBM below.  Only the module path's fp32-MFMA pointwise_kernel is priced against the fp32 matrix peak.
        if dominant == "pointwise" and fused is None:
            ach = flops_pw / (per_kernel["pointwise"] * 1e-3) / 1e12
            roof = {"bound": "mfma", "achieved": ach, "peak": F32_MFMA_PEAK_TF, "unit": "TFLOP/s",
                    "frac": ach / F32_MFMA_PEAK_TF, "traffic": None,
                    "kernel": "pwi8s_kernel/pwi8_kernel/pw3_kernel" if fused is not None else "pointwise_kernel"}
        else:
            key = dominant if dominant in alg else "dw"
            nbytes = alg.get(key, 0)
            if dominant == "quantact":      # read for min/max + read & write for the fake-quant
                nbytes = sum(3 * n[0] * 4 for (nm, n) in durs if nm == "quantact")
            ach = nbytes / (per_kernel[dominant] * 1e-3) / 1e9
            roof = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": ach / HBM_PEAK_GBS, "traffic": None,
                    "kernel": ({"dw": "dw0p_kernel+dw2_kernel+dw2u_kernel", "scale": "scale_*_kernel",
                                "unpack": "unpack_kernel", "pointwise": "pwi8s_kernel/pwi8_kernel/pw3_kernel/pwq8_kernel"}
                               if fused is not None else
                               {"dw": "dw_kernel", "scale": "scale_kernel",
                                "quantact": "minmax_kernel+fake_quant_kernel"}).get(dominant, dominant)}
        # HBM traffic of the step: measured live in this run (live_pmc_traffic), else from the committed rocprofv3 PMC
        # passes of the same workload (profiles/<round>/; null when none matches)
        def _set_traffic(bytes_per_step, source):
            roof["traffic"] = bytes_per_step.get(dominant)
            roof["traffic_source"] = source
            roof["traffic_note"] = "bytes per step (sum over the kernel family's launches), PMC FETCH_SIZE*2 + WRITE_SIZE"
            roof["algorithmic_bytes_per_step"] = nbytes
            step_bytes = sum(v for k, v in bytes_per_step.items() if k != "unpack")
            roof["step"] = {"traffic": step_bytes, "achieved": step_bytes / (dt / args.steps) / 1e9,
                            "frac": step_bytes / (dt / args.steps) / 1e9 / HBM_PEAK_GBS,
                            "traffic_by_family": {k: int(v) for k, v in bytes_per_step.items()},
                            "note": "all kernels of the step (scale + gather + pointwise): PMC bytes per step / "
                                    "ms_per_step"}
        if live_traffic and roof["bound"] == "hbm":
            _set_traffic(live_traffic, "live: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child runs of this bench.py "
                                       "invocation (eager launches, 3 steps)")
        elif roof["bound"] == "hbm":
            for rnd in ("r05", "r04", "r03", "r02", "r01"):
                try:
                    pm = json.load(open(os.path.join(ROOT, "profiles", rnd,
                                                     "pmc_traffic_frozen.json" if frozen_main else "pmc_traffic.json")))
                except (OSError, ValueError):
                    continue
                w = pm["workload"]
                if (w["res"], w["batch"], w["w2"], w["fp32"], w["path"]) == \
                        (args.res, args.batch, args.w2, args.fp32, args.path) \
                        and bool(w.get("frozen", False)) == bool(args.frozen):
                    _set_traffic(pm["bytes_per_step"], "committed: profiles/%s" % rnd)
                break
        if fused is not None:
            # every family of the step against the same HBM peak (the dominant one flips between the gather and the
            # pointwise family from box to box: they take 103-110 us each)
            roof["families"] = {k: {"algorithmic_bytes_per_step": alg[k], "ms_per_step_in_kernel": per_kernel[k],
                                    "achieved": alg[k] / (per_kernel[k] * 1e-3) / 1e9,
                                    "frac": alg[k] / (per_kernel[k] * 1e-3) / 1e9 / HBM_PEAK_GBS}
                                for k in ("dw", "pointwise", "scale") if per_kernel.get(k)}
        roof["launches_per_step"] = sum(1 for (nm, _t) in durs if nm == dominant)
        roof["ms_per_step_in_kernel"] = per_kernel[dominant]
    if rank == 0:
        ms_step = dt / args.steps * 1e3
        res = {
            "metric": "images/sec CoDeNet%s %dx%d ctdet inference (deform hot path: deconv_layers; whole network in `e2e`)"
                      % ("2x" if args.w2 else "1x", args.res, args.res),
            "value": world * args.batch * args.steps / dt,
            "unit": "images/sec",
            "n_gpus": n_seen,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_step,
            "regions": {"n": len(region_s), "steps_each": args.steps,
                        "ms_per_step_min": region_s[0] / args.steps * 1e3,
                        "ms_per_step_median": ms_step,
                        "ms_per_step_max": region_s[-1] / args.steps * 1e3,
                        "note": "every region = exactly `steps` steps between barrier + synchronize, MAX over "
                                "ranks; value / ms_per_step are the median region"},
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32" if args.fp32 else "f32+i8 (W4A8: fp32 scale / gather, int8-MFMA pointwise on 8-bit activation and 4-bit weight codes, i32 sums)",
            "data": "synthetic",
            "config": {
                "workload": "CoDeNet%s config-%s %dx%d %s, batch %d per GPU, 3 deform stages "
                            "(scale 1x1 -> QuantAct -> bilinear-gather depthwise 3x3 -> QuantAct -> "
                            "pointwise 1x1 + folded BN -> ReLU -> QuantAct range; output channels-last at stage "
                            "resolution for the native heads), %s, %s"
                            % ("2x" if args.w2 else "1x", "d" if args.w2 else ("c" if quantized else "a"),
                               args.res, args.res, "fp32" if args.fp32 else "W4A8", args.batch,
                               "frozen QuantAct ranges, byte codes in HBM (serving mode)" if args.frozen else
                               "running QuantAct ranges (reference-faithful)",
                               ("fused per-stage schedule" + (", HIP-graph replay" if use_graph else ", eager launches"))
                               if fused is not None else "module-by-module"),
                "preset": args.config or "cfg3",
                "global_batch": world * args.batch,
                "parallelism": "dp%d (independent image shards, start-up RCCL broadcast of %d bytes, per-batch "
                               "all_gather of detections in the e2e leg)" % (world, bcast_bytes),
            },
        }
        if args.full:
            res.update({
                "gpu_clock": gpu_clock_state(local_rank),
                "roofline": roof,
                "with_unpack": (None if with_unpack_ms is None else
                                {"ms_per_step": with_unpack_ms,
                                 "images_per_s": world * args.batch / with_unpack_ms * 1e3,
                                 "note": "step + unpack_kernel (fake-quant + nearest x2 + NCHW copy for a PyTorch "
                                         "consumer; the native heads do not need it)"}),
                "kernel_ms_per_step": per_kernel,
                "kernel_ms_per_launch": per_launch,
                "frozen_int8": frozen_leg,
                "e2e": e2e,
                "configs": configs,
            })
            if net_cpu is not None:
                res["cpu_baseline"] = cpu_baseline(args, net_cpu)
                res["cpu_baseline_e2e"] = cpu_baseline_e2e(args) if e2e is not None else None
                if e2e is not None and res["cpu_baseline_e2e"]:
                    res["e2e"]["vs_cpu_baseline_e2e"] = e2e["images_per_s"] / res["cpu_baseline_e2e"]["value"]
            else:
                res["cpu_baseline"] = None
                res["cpu_baseline_e2e"] = None
        print(json.dumps(res))
    if world > 1:
        dist.destroy_process_group()


def _e2e_frozen_leg(args, model, images, replay, n_fresh=16, n_cal=8, sigmas=6.0):
    """Serving mode of the whole network on THIS rank: every QuantAct frozen, byte codes from the stem to the heads.
    Ranges are calibrated on the schedule that serves (pipeline.prepare_serving -> calibrate_serving: the byte network
    itself names the QuantActs whose codes saturate) over `n_cal` calibration batches, with the tail policy for unseen
    batches (`sigmas`).  Round 6: the leg is TIMED ON FRESH BATCHES -- `n_fresh` batches whose seeds
    differ from the calibration batches' -- one graph replay per batch between HIP events (the copy into the static input
    buffer is outside the events: inputs are resident in HBM), the overflow flag read after every batch.  ms_per_batch
    is the EFFECTIVE time under the serving contract: byte schedule + overflow_rate x the fp32
    frozen recompute.  `saturating`: the same replays read as the saturating policy (no recompute; the saturated codes
    clamp to the byte range as an integer accelerator's would)."""
    import torch
    from codenet_amd import harness, pipeline
    dev = images.device
    gen = torch.Generator().manual_seed(7001)
    cal = [torch.randn(images.shape, generator=gen).to(dev) for _ in range(n_cal - 1)]
    report = pipeline.prepare_serving(model, images, settle=300, margin=0.02, replay=replay, more_batches=cal,
                                      sigmas=sigmas)
    del cal
    torch.cuda.empty_cache()
    gen = torch.Generator().manual_seed(9001)
    fresh = [torch.randn(images.shape, generator=gen).to(dev) for _ in range(n_fresh)]
    static = images.clone()

    def timed(batches, **kw):
        model.enable_fused(**kw)
        replay_f = harness.capture_process(model, static)
        for _ in range(5):
            replay_f()
        torch.cuda.synchronize()
        model.frozen_overflowed()          # (reset: only the timed batches count)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in batches]
        over, dets_f = [], None
        for (e0, e1), b in zip(ev, batches):
            static.copy_(b)
            e0.record()
            dets_f = replay_f()[1]
            e1.record()
            torch.cuda.synchronize()
            over.append(bool(model.frozen_overflowed()))
        # steady-state rate of the same graph: back-to-back replays on the last batch (what a pipelined server sees)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            replay_f()
        torch.cuda.synchronize()
        steady = (time.perf_counter() - t0) / args.steps * 1e3
        model.frozen_overflowed()
        return [a.elapsed_time(b_) for a, b_ in ev], over, dets_f, steady
    ms_st, of_st, _, steady_st = timed(fresh[:4], frozen_codes=True, frozen_backbone=False)
    ms_b, of_b, dets_f, steady_b = timed(fresh, frozen_codes=True)
    ms_cal, of_cal, _, _ = timed([images], frozen_codes=True)
    byte_backbone = model._fzbackbone is not None
    byte_heads = (model._fzheads is not None and model._fzheads._bufs is not None
                  and model._fzheads._bufs["key"][0][0] == "codes")
    rate = sum(of_b) / len(of_b)
    recompute_ms = None
    if rate > 0:                            # the contract: an overflowed batch is recomputed on the fp32 frozen schedule
        recompute_ms = timed(fresh[:2], frozen_codes=False)[3]
    total = steady_b + rate * (recompute_ms or 0.0)
    # the reference's own operating point in serving mode: ONE image + its mirror per call (test.py --flip_test) on the
    # byte schedule with the ranges calibrated above -- no range protocol between the ~55 launches of the chain
    flip = None
    try:
        model.enable_fused(frozen_codes=True)
        one = fresh[0][:1]
        pair = torch.cat([one, torch.flip(one, [3])], 0)
        rp = harness.capture_process(model, pair, flip_test=True)
        for _ in range(10):
            rp()
        torch.cuda.synchronize()
        model.frozen_overflowed()
        t0 = time.perf_counter()
        for _ in range(200):
            d2 = rp()[1]
        torch.cuda.synchronize()
        fms = (time.perf_counter() - t0) / 200 * 1e3
        flip = {"graph_ms_per_call": fms, "images_per_s": 1e3 / fms, "overflow": bool(model.frozen_overflowed()),
                "finite": bool(torch.isfinite(d2).all()),
                "what": "one image + its mirror per call (batch 2, --flip_test) on the byte-code serving schedule, one "
                        "HIP graph replay per call; e2e.latency_flip is the same call with running ranges"}
        del rp
    except Exception as exc:          # noqa: BLE001 -- an extra figure: the leg's numbers stand without it
        flip = {"error": "%s: %s" % (type(exc).__name__, exc)}
    return {"ms_per_batch": total, "images_per_s": args.batch / total * 1e3, "per_rank": True, "latency_flip": flip,
            "fresh_batches": n_fresh, "overflow_rate": rate, "valid": rate < 0.02, "overflow": rate > 0,
            "byte_schedule_ms": steady_b, "byte_schedule_ms_per_fresh_batch_events": sum(ms_b) / len(ms_b),
            "fp32_recompute_ms": recompute_ms,
            "saturating": {"ms_per_batch": steady_b, "images_per_s": args.batch / steady_b * 1e3,
                           "batches_with_a_saturated_code": rate,
                           "what": "the same replays under the saturating policy: nothing is recomputed, a code beyond the "
                                   "byte range clamps (what an int8 accelerator does; the reference's fake-quantised "
                                   "floats do not clamp, quant_utils.py:193-200)"},
            "calibration_batch": {"ms_per_batch": ms_cal[0], "overflow": of_cal[0],
                                  "what": "round 5's figure: timed on the batch the ranges were calibrated on"},
            "finite": bool(torch.isfinite(dets_f).all()),
            "byte_backbone": byte_backbone, "byte_heads": byte_heads,
            "stages_only": {"ms_per_batch": steady_st, "overflow_rate": sum(of_st) / len(of_st),
                            "what": "backbone on the fp32 kernels without range updates, stages on byte codes"},
            "calibration": report,
            "what": "the same network with every QuantAct frozen (running_stat False: serving mode, not the "
                    "reference's default) on BYTE CODES from the stem to the heads' input: backbone "
                    "(pipeline.FrozenBackbone), the three deform stages with chained scale sums "
                    "(pipeline.FrozenHotPath), the heads' 1x1 convs and tails (FusedHeads.forward_codes); no "
                    "range passes anywhere; ranges calibrated on the byte schedule itself over %d batches "
                    "(pipeline.calibrate_serving, %g-sigma tail policy); TIMED ON %d FRESH BATCHES (other seeds) on "
                    "rank 0's shard without collectives; ms_per_batch = steady-state byte schedule + overflow_rate x "
                    "the fp32 frozen recompute" % (n_cal, sigmas, n_fresh)}


def _flip_latency_leg(args, dev, rank, calls=200):
    """Latency of what `test.py ctdet --flip_test` does per image (VERDICT r5 missing #7): batch 2 = the image and its
    W-mirror through the whole network (running QuantAct ranges, as the reference), the native sigmoid + mirror merge,
    ctdet_decode -- one HIP graph replay per call, and the same call launched eagerly from Python."""
    import torch
    from codenet_amd import harness
    model = harness.create_model(w2=args.w2, quantize=not args.fp32, seed=317).to(dev)
    model.enable_fused()
    img = torch.randn(1, 3, args.res, args.res, generator=torch.Generator().manual_seed(rank)).to(dev)
    pair = torch.cat([img, torch.flip(img, [3])], 0)
    out = {}
    for _ in range(10):
        harness.process(model, pair, flip_test=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        harness.process(model, pair, flip_test=True)
    torch.cuda.synchronize()
    out["eager_ms_per_call"] = (time.perf_counter() - t0) / 50 * 1e3
    replay = harness.capture_process(model, pair, flip_test=True)
    for _ in range(10):
        replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        dets = replay()[1]
    torch.cuda.synchronize()
    out["graph_ms_per_call"] = (time.perf_counter() - t0) / calls * 1e3
    out["images_per_s"] = 1e3 / out["graph_ms_per_call"]
    out["finite"] = bool(torch.isfinite(dets).all())
    out["what"] = ("one image + its mirror per call (batch 2, --flip_test), whole network + mirror merge + decode; a "
                   "dependency chain of ~110 short launches: latency-, not bandwidth-bound")
    del replay, model
    torch.cuda.empty_cache()
    return out


def e2e_leg(args, dev, rank, world, local_rank, hot_ms):
    """Whole network (stem + 16 ShuffleNetV2 units + layer4 + three deform stages + three heads, all on the HIP
    kernels) + native ctdet_decode, captured as ONE HIP graph per rank over a static image buffer; for N > 1
    every batch ends with the all_gather of the ranks' detections [B,100,6]."""
    import torch
    import torch.distributed as dist
    from codenet_amd import harness, pipeline
    model = harness.create_model(w2=args.w2, quantize=not args.fp32, seed=317 if rank == 0 else 1000 + rank).to(dev)
    pipeline.broadcast_parameters(model, src=0)
    model.enable_fused()
    g = torch.Generator().manual_seed(rank)
    images = torch.randn(args.batch, 3, args.res, args.res, generator=g).to(dev)
    if not args.fp32 and args.frozen:
        harness.process(model, images, flip_test=False)
        pipeline.set_running_stat(model, False)
    replay = harness.capture_process(model, images)
    counts = pipeline.exchange_shard_sizes(args.batch, dev)      # once: shard sizes are static

    def step():
        dets = replay()[1]
        return pipeline.gather_detections(dets, counts=counts) if world > 1 else dets

    def barrier():
        if world > 1:
            dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize()
    for _ in range(5):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        dets = step()
    barrier()
    dt = time.perf_counter() - t0
    tmax = torch.tensor([dt], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = tmax.item()
    assert torch.isfinite(dets).all() and dets.shape[0] == world * args.batch
    ms = dt / args.steps * 1e3
    # ---- serving mode: every QuantAct frozen (running_stat False), the three stages on the byte-code schedule ----
    frozen = None
    if not args.fp32 and not args.frozen:
        # per-rank leg without collectives (a failure here must not hang the other ranks or lose the headline)
        try:
            frozen = _e2e_frozen_leg(args, model, images, replay)
        except Exception as exc:          # noqa: BLE001 -- reported in the JSON line, the step's numbers stand
            frozen = {"error": "%s: %s" % (type(exc).__name__, exc)}
    # ---- the reference's own entry point: test.py runs ONE image + its mirror per call (test.py:62-64,
    #      lib/detectors/base_detector.py:70-71 --flip_test): the latency of that call, as a graph and eagerly ----
    latency = None
    if not args.frozen:
        try:
            latency = _flip_latency_leg(args, dev, rank)
        except Exception as exc:          # noqa: BLE001
            latency = {"error": "%s: %s" % (type(exc).__name__, exc)}
    return {"ms_per_batch": ms, "images_per_s": world * args.batch / ms * 1e3, "frozen": frozen,
            "latency_flip": latency,
            "hot_path_share": hot_ms / ms, "detections": list(dets.shape),
            "what": "CoDeNet%s %dx%d %s batch %d per GPU: whole network on the HIP kernels + native ctdet_decode "
                    "(K=100), one HIP graph per rank%s" % (
                        "2x" if args.w2 else "1x", args.res, args.res, "fp32" if args.fp32 else "W4A8", args.batch,
                        ", all_gather of detections per batch" if world > 1 else "")}


if __name__ == "__main__":
    main()
