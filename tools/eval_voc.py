"""AP50 on PASCAL VOC2007 test through the native network, end to end -- the reference's procedure
(README.md:87-108: ``test.py ctdet --arch shufflenetv2 ... --resume-quantize`` then ``tools/reval.py``):

    image -> pre_process (lib/detectors/base_detector.py:47-77: keep-ratio affine crop to input_res, mean / std)
          -> PoseShuffleNetV2 on the HIP kernels (harness.enable_fused) [+ W-flip averaging, ctdet.py:32-39]
          -> ctdet_decode (K = 100) -> post_process / merge_outputs (lib/utils/post_process.py:86-103, ctdet.py:48-72)
          -> results.json (lib/datasets/dataset/pascal.py:58-79)
          -> VOC07 11-point AP at IoU 0.5 per class, mean = AP50
             (tools/voc_eval_lib/datasets/voc_eval.py:31-48,95-200, pascal_voc.py:237-247)

Needs what the reference needs and this container does not have: ``<data>/voc/images/*.jpg`` +
``<data>/voc/annotations/pascal_test2007.json`` (tools/get_pascal_voc.sh) and a checkpoint
(``exp/ctdet/pascal_shufflenetv2_config_*/model_last.pth``).  When they are absent it prints the PROXY of SURVEY 8(d)
instead -- the whole network against tests/golden/model_io.npz (outputs of the reference's own model) -- and says so.
cv2 is not available here: images are read with PIL and the affine crop is done by torch's bilinear grid_sample
(cv2.INTER_LINEAR's arithmetic differs in the last bits; this is stated in the output).

    python tools/eval_voc.py --data /data --load_model exp/ctdet/pascal_shufflenetv2_config_c/model_last.pth \
        --res 512 --quantize [--w2] [--maxpool] [--flip_test] [--test_scales 0.5,0.75,1,1.25,1.5] [--nms] [--gpu_pre]

--gpu_eval: the merged detections of every image stay on the device (evalio.DeviceResults.append on the merge block, no
per-image copy to the host) and one call at the end scores all 20 classes there (evalio.voc_eval_device,
codenet_eval.hip).  --check_eval: the Python scorer below runs beside it on host copies of the
same blocks, and any difference in a curve or an AP is an error.

--gpu_pre: the image BYTES go to the device and codenet_amd.preproc (codenet_preproc.hip) builds every test scale and
mirror there, as the first node of the captured graph -- an integer resize + crop of this project's own (DESIGN.md
section 7.4b), within 10 grey levels of the float path above on noise, not a copy of cv2's bits either.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from codenet_amd import evalio, harness, preproc

CLASSES = ["aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog",
           "horse", "motorbike", "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor"]   # pascal.py:32-36
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)                                           # pascal.py:15-18
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def pre_process(img, res, scale=1.0):
    """BaseDetector.pre_process with fix_res (ctdet on pascal: opts.py keep_res False): c = image centre,
    s = max(h, w); the un-rotated affine map of get_affine_transform (lib/utils/image.py:30-55) sends the square of
    side s around c onto the res x res input.  img: uint8 [H, W, 3] RGB -> ([1,3,res,res] float32, meta).
    scale (--test_scales, base_detector.py:47-55): the image is first resized to int(h * scale) x int(w * scale), c is
    the centre of the RESIZED image and s stays max(h, w) of the unscaled one, so every scale lands on the same
    res x res crop (post_process divides the boxes by scale again)."""
    h, w = img.shape[:2]
    t = torch.from_numpy(np.ascontiguousarray(img).copy()).permute(2, 0, 1).float().unsqueeze(0)
    s = float(max(h, w))
    if scale != 1.0:
        h, w = int(h * scale), int(w * scale)
        t = torch.nn.functional.interpolate(t, size=(h, w), mode="bilinear", align_corners=False)   # (cv2.resize)
    c = np.array([w / 2.0, h / 2.0], dtype=np.float32)
    # output pixel (u, v) <- source (c + ((u, v) - res/2) * s/res); grid_sample wants normalised source coordinates
    u = (torch.arange(res, dtype=torch.float32) - res / 2.0) * (s / res)
    xs, ys = c[0] + u, c[1] + u
    gx = (2 * xs + 1) / w - 1           # align_corners=False: pixel centres at (i + 0.5) / size
    gy = (2 * ys + 1) / h - 1
    grid = torch.stack(torch.meshgrid(gy, gx, indexing="ij")[::-1], dim=-1).unsqueeze(0)
    inp = torch.nn.functional.grid_sample(t, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    inp = (inp / 255.0 - torch.from_numpy(MEAN).view(1, 3, 1, 1)) / torch.from_numpy(STD).view(1, 3, 1, 1)
    return inp, {"c": c, "s": s, "out_height": res // 4, "out_width": res // 4}


def voc_ap07(rec, prec):
    """11-point interpolated AP (voc_eval.py:36-48)."""
    ap = 0.0
    for t in np.arange(0.0, 1.1, 0.1):
        ap += (np.max(prec[rec >= t]) if np.sum(rec >= t) else 0.0) / 11.0
    return ap


def voc_ap_area(rec, prec):
    """Area under the monotone precision envelope (voc_eval.py:49-62, use_07_metric=False)."""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


def voc_eval_curve(dets, gts, ovthresh=0.5):
    """dets: list of (image_id, score, x1, y1, x2, y2) of one class; gts: image_id -> (boxes [n,4], difficult [n]).
    -> (rec, prec) over the detections in descending score order.  voc_eval.py:95-207 (+1 pixel conventions kept;
    a detection on a difficult box is neither TP nor FP; a second detection of a found box is a FP; equal scores
    keep their input order -- the reference's argsort leaves ties unspecified).  One divergence: with no
    non-difficult ground truth the reference divides by npos = 0; here rec is all zeros."""
    npos = sum(int((~d).sum()) for _, d in gts.values())
    seen = {k: np.zeros(len(b), dtype=bool) for k, (b, _) in gts.items()}
    dets = sorted(dets, key=lambda r: -r[1])
    tp, fp = np.zeros(len(dets)), np.zeros(len(dets))
    for i, (img, _score, *bb) in enumerate(dets):
        boxes, diff = gts.get(img, (np.zeros((0, 4)), np.zeros(0, dtype=bool)))
        ovmax, jmax = -np.inf, -1
        if len(boxes):
            ixmin, iymin = np.maximum(boxes[:, 0], bb[0]), np.maximum(boxes[:, 1], bb[1])
            ixmax, iymax = np.minimum(boxes[:, 2], bb[2]), np.minimum(boxes[:, 3], bb[3])
            inter = np.maximum(ixmax - ixmin + 1.0, 0.0) * np.maximum(iymax - iymin + 1.0, 0.0)
            uni = (bb[2] - bb[0] + 1.0) * (bb[3] - bb[1] + 1.0) + \
                (boxes[:, 2] - boxes[:, 0] + 1.0) * (boxes[:, 3] - boxes[:, 1] + 1.0) - inter
            ov = inter / uni
            jmax = int(np.argmax(ov))
            ovmax = ov[jmax]
        if ovmax > ovthresh:
            if not diff[jmax]:
                if not seen[img][jmax]:
                    tp[i] = 1.0
                    seen[img][jmax] = True
                else:
                    fp[i] = 1.0
        else:
            fp[i] = 1.0
    tp, fp = np.cumsum(tp), np.cumsum(fp)
    rec = tp / max(npos, 1)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec


def voc_eval(dets, gts, ovthresh=0.5):
    """VOC07 11-point AP of one class (what pascal_voc.py:237-247 asks voc_eval for)."""
    return voc_ap07(*voc_eval_curve(dets, gts, ovthresh))


def run_voc(args):
    from PIL import Image
    root = os.path.join(args.data, "voc")
    ann = json.load(open(os.path.join(root, "annotations", "pascal_test2007.json")))
    images = {im["id"]: im for im in ann["images"]}
    gts = {c: {} for c in range(1, 21)}
    for a in ann["annotations"]:
        x, y, w, h = a["bbox"]
        g = gts[a["category_id"]].setdefault(a["image_id"], ([], []))
        g[0].append([x, y, x + w, y + h])
        g[1].append(bool(a.get("ignore", 0) or a.get("difficult", 0)))
    gts = {c: {k: (np.array(b, dtype=np.float64), np.array(d, dtype=bool)) for k, (b, d) in v.items()}
           for c, v in gts.items()}
    model = harness.create_model(w2=args.w2, maxpool=args.maxpool, quantize=args.quantize)
    evalio.load_model(model, args.load_model)
    model = model.cuda().eval().enable_fused()
    results = {}
    ids = sorted(images)[: args.limit or None]
    gpu_eval, check_eval = bool(getattr(args, "gpu_eval", False)), bool(getattr(args, "check_eval", False))
    if check_eval and not gpu_eval:
        raise SystemExit("--check_eval checks the device scorer: it needs --gpu_eval")
    dev_results = evalio.DeviceResults(len(ids), 20, cap=100, device="cuda") if gpu_eval else None
    host_too = check_eval or not gpu_eval          # the per-image host copy: only without --gpu_eval, or to check it

    def keep_single(n, img_id, dets, meta):
        """one scale, no --nms: post_process + the max_per_image cut -- on the host, or (--gpu_eval) by the merge kernel
        with one scale and without soft-NMS, whose block goes straight into the device table"""
        if gpu_eval:
            dev_results.append(harness.merge_scales_native(dets.view(1, 1, -1, 6), [meta], [1.0], 20, nms=False, raw=True), n)
        if host_too:
            results[img_id] = evalio.merge_outputs([evalio.post_process(dets.clone(), meta, 20)], 20)

    def keep_multi(n, img_id, replay):
        if host_too:
            results[img_id] = replay()[2]
        else:
            replay.graph.replay()
        if gpu_eval:
            dev_results.append(replay.raw, n)
    static, replay = None, None        # the network + [flip merge +] decode as ONE HIP graph over a static input buffer
    scales = [float(v) for v in str(getattr(args, "test_scales", "1")).split(",")]
    multi = len(scales) > 1 or bool(getattr(args, "nms", False))   # all scales of an image in one graph, merged on the GPU
    pre = None
    if getattr(args, "gpu_pre", False):
        # resize + crop + normalise + mirrors on the GPU, inside the graph: per image only the bytes and the crop table go
        # up.  The arena holds the largest image of the annotation file (1024 x 1024 when it does not give the sizes)
        pre = preproc.PreProcess(args.res, args.res, scales=scales if multi else (1.0,), flip_test=args.flip_test,
                                 max_h=max(im.get("height", 0) for im in images.values()) or 1024,
                                 max_w=max(im.get("width", 0) for im in images.values()) or 1024)
    for n, img_id in enumerate(ids):
        img = np.asarray(Image.open(os.path.join(root, "images", images[img_id]["file_name"])).convert("RGB"))
        if pre is not None:
            metas = pre.load(img)
            if static is None:
                static = torch.empty(pre.out_shape(), dtype=torch.float32, device="cuda")
                ranges = [(b, b.clone()) for nme, b in model.named_buffers() if nme.endswith(("x_min", "x_max"))]
                if multi:
                    replay = harness.capture_process_scales(model, static, len(scales), args.flip_test, metas, scales, nms=True,
                                                            batched=bool(getattr(args, "batch_scales", False)), pre=pre)
                else:
                    replay = harness.capture_process(model, static, flip_test=args.flip_test, pre=pre)
                with torch.no_grad():
                    for b, saved in ranges:
                        b.copy_(saved)
            if multi:
                replay.meta.copy_(harness.scale_metas(metas, scales), non_blocking=True)
                keep_multi(n, img_id, replay)
            else:
                keep_single(n, img_id, replay()[1], metas[0])
            if n % 500 == 0:
                print("%d / %d images" % (n, len(ids)), file=sys.stderr)
            continue
        if multi:
            per_scale = [pre_process(img, args.res, sc) for sc in scales]
            inp = torch.cat([p[0] for p in per_scale], 0)
            metas = [p[1] for p in per_scale]
            if args.flip_test:
                inp = torch.cat([inp, torch.flip(inp, [3])], 0)
            if static is None:
                static = inp.cuda()
                ranges = [(b, b.clone()) for nme, b in model.named_buffers() if nme.endswith(("x_min", "x_max"))]
                replay = harness.capture_process_scales(model, static, len(scales), args.flip_test, metas, scales,
                                                        nms=True, batched=bool(getattr(args, "batch_scales", False)))
                with torch.no_grad():
                    for b, saved in ranges:
                        b.copy_(saved)
            static.copy_(inp, non_blocking=True)
            replay.meta.copy_(harness.scale_metas(metas, scales), non_blocking=True)
            keep_multi(n, img_id, replay)
            if n % 500 == 0:
                print("%d / %d images" % (n, len(ids)), file=sys.stderr)
            continue
        inp, meta = pre_process(img, args.res)
        if args.flip_test:
            inp = torch.cat([inp, torch.flip(inp, [3])], 0)
        if static is None:
            static = inp.cuda()
            # capturing runs the network a few times on this first image; the QuantAct ranges keep tracking during
            # test as in the reference (running_stat stays True), so they are put back: every image counts once
            ranges = [(b, b.clone()) for nme, b in model.named_buffers() if nme.endswith(("x_min", "x_max"))]
            replay = harness.capture_process(model, static, flip_test=args.flip_test)
            with torch.no_grad():
                for b, saved in ranges:
                    b.copy_(saved)
        static.copy_(inp, non_blocking=True)
        keep_single(n, img_id, replay()[1], meta)
        if n % 500 == 0:
            print("%d / %d images" % (n, len(ids)), file=sys.stderr)
    os.makedirs(args.out, exist_ok=True)
    scored = None
    if gpu_eval:
        gt_dev = evalio.GroundTruth.from_coco_dict(ann, image_ids=ids, valid_ids=list(range(1, 21)), voc=True, device="cuda")
        scored = evalio.voc_eval_device(dev_results, gt_dev, curves=check_eval)
        if not host_too:                           # results.json from ONE copy of the table
            table, count = dev_results.det.cpu().numpy(), dev_results.count.cpu().numpy()
            for n, img_id in enumerate(ids):
                rows = table[n, :count[n]]
                results[img_id] = {c: rows[rows[:, 5] == c - 1, :5].astype(np.float32) for c in range(1, 21)}
    evalio.save_results(results, ids, 20, args.out)
    aps = []
    for c in range(1, 21):
        if gpu_eval and not check_eval:
            aps.append(float(scored["ap_07"][c - 1]))
        else:
            rows = [(img_id, float(r[4]), *map(float, r[:4])) for img_id in ids for r in results[img_id][c]]
            rec, prec = voc_eval_curve(rows, gts[c])
            aps.append(voc_ap07(rec, prec))
            if gpu_eval:
                same = (np.array_equal(rec, scored["rec"][c - 1]) and np.array_equal(prec, scored["prec"][c - 1])
                        and aps[-1] == scored["ap_07"][c - 1] and voc_ap_area(rec, prec) == scored["ap_area"][c - 1])
                if not same:
                    raise SystemExit("--check_eval: the device scorer and the Python scorer differ for %s (AP %r vs %r)"
                                     % (CLASSES[c - 1], float(scored["ap_07"][c - 1]), aps[-1]))
        print("AP for %s = %.4f" % (CLASSES[c - 1], aps[-1]))
    out = {"AP50": float(np.mean(aps)), "per_class": dict(zip(CLASSES, map(float, aps))), "images": len(ids),
           "note": "VOC07 11-point, IoU 0.5; pre-processing by PIL + " + (
               "the integer resize / crop of codenet_preproc.hip on the GPU (--gpu_pre; cv2 absent)" if pre is not None
               else "torch bilinear grid_sample (cv2 absent)")}
    if gpu_eval:
        out["scorer"] = "device (evalio.voc_eval_device)" + (", equal to the Python scorer in every curve and AP"
                                                             if check_eval else "")
    if args.reference_ap50 is not None:
        out["delta_vs_reference"] = out["AP50"] - args.reference_ap50
    print(json.dumps(out))


def run_proxy(args):
    """No data / checkpoint here: the SURVEY 8(d) proxy on the reference model's golden outputs."""
    g = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
    z = {k: torch.from_numpy(np.asarray(v)) for k, v in np.load(os.path.join(g, "model_io.npz")).items()}
    nz = {k: float(v) for k, v in np.load(os.path.join(g, "model_noise.npz")).items()}
    gen = torch.Generator().manual_seed(int(z["image_seed"]))
    img = torch.randn(1, 3, 256, 256, generator=gen)
    images = torch.cat([img, torch.flip(img, [3])], 0).cuda()
    out = {"measured": "PROXY (no VOC data / checkpoint on this box): whole network vs the reference model's golden "
                       "outputs on a synthetic image + its flip, synthetic weights"}
    for tag in ("fp32", "w4a8"):
        model = harness.create_model(quantize=(tag == "w4a8")).cuda().enable_fused()
        for _ in range(int(z[tag + "_nfwd"]) - 1):
            with torch.no_grad():
                model(images)
        o, dets = harness.process(model, images)
        worst, means = 0.0, {}
        for k in ("hm", "wh", "reg"):
            raw = o[k].cpu() if k != "hm" else torch.logit(o[k].cpu())
            d = (raw[:, :, ::4, ::4] - z["%s_%s_sub" % (tag, k)]).abs()
            worst = max(worst, d.max().item())
            means[k] = d.mean().item()
        ref = z[tag + "_dets"][0]
        ours = dets.cpu()[0]
        oc = torch.stack([(ours[:, 0] + ours[:, 2]) / 2, (ours[:, 1] + ours[:, 3]) / 2], 1)
        rc = torch.stack([(ref[:, 0] + ref[:, 2]) / 2, (ref[:, 1] + ref[:, 3]) / 2], 1)
        tol = (0.05, 2e-3) if tag == "fp32" else (0.5, 2e-2)
        hit = sum(int(((ours[:, 5] == ref[i, 5]) & ((oc - rc[i]).abs().max(dim=1).values <= tol[0])
                       & ((ours[:, 4] - ref[i, 4]).abs() <= tol[1])).any()) for i in range(ref.shape[0]))
        out[tag] = {"max_abs_diff": worst, "mean_abs_diff": means, "top100_agreement": hit / ref.shape[0]}
    out["reference_vs_itself_w4a8"] = {"mean_abs_diff": {k: nz["noise_mean_" + k] for k in ("hm", "wh", "reg")},
                                       "top100_agreement": nz["self_agreement"]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default="data")
    ap.add_argument("--load_model", default="")
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--quantize", action="store_true")
    ap.add_argument("--w2", action="store_true")
    ap.add_argument("--maxpool", action="store_true")
    ap.add_argument("--flip_test", action="store_true")
    ap.add_argument("--test_scales", default="1", help="comma list of test scales (test.py --test_scales), e.g. "
                    "0.5,0.75,1,1.25,1.5: the scales of an image run as one batch and are merged by soft-NMS on the GPU")
    ap.add_argument("--nms", action="store_true", help="soft-NMS also with a single test scale (test.py --nms)")
    ap.add_argument("--batch_scales", action="store_true", help="run the scales of an image as ONE network batch instead "
                    "of one pass per scale (faster; QuantAct ranges then update once per image, not once per scale)")
    ap.add_argument("--gpu_pre", action="store_true", help="pre-process on the GPU inside the captured graph "
                    "(codenet_amd.preproc: integer resize + crop, DESIGN.md section 7.4b) instead of on the host")
    ap.add_argument("--gpu_eval", action="store_true", help="keep the merged detections on the device and score them "
                    "there (evalio.DeviceResults / voc_eval_device, DESIGN.md section 7.4e): no per-image copy to the host")
    ap.add_argument("--check_eval", action="store_true", help="with --gpu_eval: also run the Python scorer on host copies "
                    "and fail on any difference")
    ap.add_argument("--limit", type=int, default=0)
    ap.add_argument("--out", default="gpurun_out/voc_eval")
    ap.add_argument("--proxy-images", type=int, default=0, help="without data / checkpoint: also run the detection-"
                    "agreement proxy on this many synthetic images (tests/proxy_agreement.py; SURVEY 8(d) asks for >= 256)")
    ap.add_argument("--proxy-out", default="", help="JSON file for the at-size proxy")
    ap.add_argument("--proxy-ap", type=int, default=0, help="without data / checkpoint: the AP50-DELTA proxy on this many "
                    "synthetic images -- pseudo ground truth from the fp32 CPU-oracle path, CPU-W4A8 and GPU-W4A8 detections "
                    "(running / frozen / byte serving) scored by this file's voc_eval (tests/proxy_ap.py)")
    ap.add_argument("--proxy-ap-out", default="", help="JSON file for the AP50-delta proxy")
    ap.add_argument("--reference-ap50", type=float, default=None, help="the reference's AP50 for this config "
                    "(README.md:14-18) to print the delta")
    args = ap.parse_args()
    have = (os.path.isfile(os.path.join(args.data, "voc", "annotations", "pascal_test2007.json"))
            and os.path.isfile(args.load_model))
    if have:
        run_voc(args)
    else:
        run_proxy(args)
        if args.proxy_images > 0:
            # the proxy at size (>= 256 images): the GPU build against the CPU oracle path.  The comparison
            # uses oracle/, which only tests/ may import: it lives in tests/proxy_agreement.py and runs as a child process
            import subprocess
            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            cmd = [sys.executable, os.path.join(root, "tests", "proxy_agreement.py"), "--images", str(args.proxy_images),
                   "--res", str(args.res)] + (["--out", args.proxy_out] if args.proxy_out else [])
            rc = subprocess.call(cmd)
            if rc:
                sys.exit(rc)
        if args.proxy_ap > 0:
            # the AP50-delta proxy through voc_eval (VERDICT r5 missing #1); uses oracle/ too: a child process of tests/
            import subprocess
            root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
            cmd = [sys.executable, os.path.join(root, "tests", "proxy_ap.py"), "--images", str(args.proxy_ap),
                   "--res", str(args.res)] + (["--out", args.proxy_ap_out] if args.proxy_ap_out else [])
            sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
