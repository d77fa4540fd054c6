"""Cost of JPEG decoding for a batch of 64 streams of 375 x 500, 4:2:0, quality 75 (a Pascal VOC image): the HOST path
against the GPU path (codenet_amd.jpeg), and the two kernels alone.  GPU only; one JSON line per image set.

(a) host: PIL (libjpeg-turbo) on a 16-thread pool into a pinned buffer + the upload of the decoded bytes.  Where PIL does
    not import this leg is left out.
(b) gpu:  JpegDecoder.load (host parse + pack, upload of the entropy-coded bytes and the tables) + JpegDecoder.run (the
    two launches).
(c) kernels: jpeg_entropy_idct_kernel + jpeg_color_kernel by HIP events, beside a device copy of the output bytes.

(a) and (b) alternate; the figures are medians with min / max.  Two image sets: the streams as a VOC file has them (no
restart markers: ONE segment per image, so the entropy kernel runs 64 lane-serial chains, one per image) and the same images
encoded with a restart interval of one MCU row (24 segments per image) -- how the entropy kernel scales with the segment
count.  The streams come from PIL when it imports (64 different images); otherwise the fixture's stream is replicated and
the restart set is left out.

--entropy parallel adds the parallel entropy path (JpegDecoder(entropy="parallel", subseq_bits=--subseq_bits)) to every
image set: (d) the launches of the serial and of the parallel decoder by HIP events, INTERLEAVED pair by pair on the same
streams, at the batch given and at batch 1 (the first stream alone: what test.py replays per image), with the number of
pairs in which the parallel launches were the shorter ones, and a small sweep of subseq_bits.  The two outputs must be
torch.equal.  The yardstick is the serial path of the same run."""
import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from codenet_amd import jpeg

try:
    from PIL import Image
except ImportError:
    Image = None

H, W = 375, 500


def streams(batch, restart_rows):
    """[bytes] x batch: smooth structure + mild noise, the statistics of a photograph at quality 75 (about 45 KB)."""
    out = []
    for k in range(batch):
        rng = np.random.RandomState(k)
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        img = np.stack([128 + 100 * np.sin(x / (7.0 + k % 5) + y / 11.0), 128 + 90 * np.cos(x / 5.0 - y / (9.0 + k % 3)),
                        40 + 0.3 * x + 0.2 * y], axis=2) + rng.randint(-12, 13, size=(H, W, 3))
        buf = io.BytesIO()
        kw = {"restart_marker_rows": restart_rows} if restart_rows else {}
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, "JPEG", quality=75, subsampling=2, **kw)
        out.append(buf.getvalue())
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, steps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def stats(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3)}


def pair_ms(serial, parallel, out_s, out_p, pairs, warm=3):
    """HIP-event times of serial.run and parallel.run, alternating -> (stats serial, stats parallel, pairs won)."""
    for _ in range(warm):
        serial.run(out_s)
        parallel.run(out_p)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(pairs)]
    for a, b, c, d in ev:
        a.record()
        serial.run(out_s)
        b.record()
        c.record()
        parallel.run(out_p)
        d.record()
    torch.cuda.synchronize()
    ts, tp = [a.elapsed_time(b) for a, b, _, _ in ev], [c.elapsed_time(d) for _, _, c, d in ev]
    return stats(ts), stats(tp), sum(int(p < s) for s, p in zip(ts, tp))


def parallel_rows(row, datas, serial, out, steps, subseq_bits, sweep):
    """(d): the serial and the parallel launches interleaved, at the whole batch and at batch 1, and the sweep."""
    batch = len(datas)
    kw = dict(max_items=batch, max_h=H, max_w=W, max_stream_bytes=serial.max_stream_bytes, max_segments=serial.max_segments)
    out_p = torch.zeros_like(out)
    row["subseq_bits"], row["pairs"] = subseq_bits, steps
    for S in [subseq_bits] + [s for s in sweep if s != subseq_bits]:
        par = jpeg.JpegDecoder(entropy="parallel", subseq_bits=S, **kw)
        for label, sub in (("batch_%d" % batch, datas), ("batch_1", datas[:1])):
            serial.load(sub)
            par.load(sub)
            out.zero_()
            out_p.zero_()
            serial.run(out)
            par.run(out_p)
            serial.check()
            par.check()
            assert torch.equal(out, out_p), "parallel and serial outputs differ (%s, subseq_bits %d)" % (label, S)
            ts, tp, won = pair_ms(serial, par, out, out_p, steps)
            if S == subseq_bits:
                row["kernels_serial_ms_" + label], row["kernels_parallel_ms_" + label] = ts, tp
                row["parallel_below_serial_pairs_" + label] = won
            else:
                row.setdefault("sweep_parallel_ms_" + label, {})[str(S)] = tp
        del par
    serial.load(datas)


def one_set(name, datas, reps, steps, threads, entropy="serial", subseq_bits=1024, sweep=()):
    batch = len(datas)
    infos = [jpeg.parse(d) for d in datas]
    dec = jpeg.JpegDecoder(max_items=batch, max_h=H, max_w=W, max_stream_bytes=sum(len(d) for d in datas) + 64,
                           max_segments=sum(i.segments for i in infos))
    out = torch.zeros(batch * H * W * 3, dtype=torch.uint8, device="cuda")
    static = torch.zeros_like(out)
    pinned = torch.zeros(batch, H, W, 3, dtype=torch.uint8).pin_memory()
    pinned_np = pinned.numpy()
    pool = ThreadPoolExecutor(threads)

    def host_one(k):
        pinned_np[k] = np.asarray(Image.open(io.BytesIO(datas[k])).convert("RGB"))[:, :, ::-1]

    def host():
        list(pool.map(host_one, range(batch)))
        static.copy_(pinned.view(-1), non_blocking=True)

    def gpu():
        dec.load(datas)
        dec.run(out)

    row = {"set": name, "batch": batch, "segments": sum(i.segments for i in infos),
           "stream_bytes": sum(len(d) for d in datas), "out_bytes": out.numel(), "host_threads": threads}
    gpu()
    dec.check()
    t_host, t_gpu = [], []
    if Image is not None:
        host()
        row["equal_to_pil"] = bool(torch.equal(out, static))
    for _ in range(reps):                           # interleaved
        if Image is not None:
            t_host.append(wall_ms(host))
        t_gpu.append(wall_ms(gpu))
    t_pack = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dec.load(datas)
        t_pack.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
    if t_host:
        row["host_ms"] = stats(t_host)
    row["gpu_ms"] = stats(t_gpu)
    row["gpu_load_host_side_ms"] = stats(t_pack)            # parse + pack + issuing the copies, before the device is waited for
    row["kernels_ms"] = event_ms(lambda: dec.run(out), steps)
    row["copy_ms"] = event_ms(lambda: static.copy_(out), steps)
    row["images_per_s_gpu_path"] = round(batch / row["gpu_ms"]["median"] * 1e3, 1)
    if entropy == "parallel":
        parallel_rows(row, datas, dec, out, steps, subseq_bits, sweep)
    if t_host:
        row["images_per_s_host_path"] = round(batch / row["host_ms"]["median"] * 1e3, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=9, help="interleaved host / GPU repetitions")
    ap.add_argument("--steps", type=int, default=15, help="HIP-event pairs per kernel median")
    ap.add_argument("--threads", type=int, default=16, help="threads of the host decode")
    ap.add_argument("--entropy", choices=("serial", "parallel"), default="serial",
                    help="parallel: also time the parallel entropy path against the serial one, interleaved")
    ap.add_argument("--subseq_bits", type=int, default=1024, help="sub-sequence size of the parallel path")
    ap.add_argument("--sweep", type=int, nargs="*", default=[256, 512, 1024, 2048, 4096],
                    help="further sub-sequence sizes timed with --entropy parallel")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpeg_bench needs the GPU"
    if Image is not None:
        sets = [("voc-like, no restart markers", streams(args.batch, 0)),
                ("restart interval of one MCU row", streams(args.batch, 1))]
    else:
        fixture = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg_cases.npz")
        sets = [("fixture stream replicated, no restart markers", [bytes(np.load(fixture)["big_jpg"])] * args.batch)]
    for name, datas in sets:
        print(json.dumps(one_set(name, datas, args.reps, args.steps, args.threads, args.entropy, args.subseq_bits,
                                 args.sweep)), flush=True)


if __name__ == "__main__":
    main()
