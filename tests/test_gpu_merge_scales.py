"""The multi-scale merge on the GPU (codenet_merge.hip: cdn_ctdet_merge_scales, harness.merge_scales_native /
process_scales / capture_process_scales) against the host path -- evalio.post_process + soft_nms + the max_per_image cut,
whose soft_nms tests/test_soft_nms.py pins bitwise to the compiled reference.  Everything is np.array_equal: both sides
run the same float32 / double operations in the same order.  (The one operation the two sides take from different
libraries is the double exp of the gaussian method: the device's and glibc's can differ in the last bit of the DOUBLE,
which changes the float32 weight only when that double lies within an ulp of a float32 rounding midpoint, ~2^-29 per
weight.)"""
import copy
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "soft_nms_ref.npz")
SCALES = [0.5, 0.75, 1.0, 1.25, 1.5]


def _host_merge(per_scale, num_classes, max_per_image, do_nms, sigma=0.5, Nt=0.5, threshold=0.001, method=2):
    """merge_outputs (ctdet.py:59-74) with soft_nms' settings open; -> (results, full arrays, N per class, thresh)."""
    from codenet_amd import evalio
    full, live = {}, {}
    for j in range(1, num_classes + 1):
        full[j] = np.concatenate([d[j] for d in per_scale], axis=0).astype(np.float32)
        live[j] = len(evalio.soft_nms(full[j], sigma=sigma, Nt=Nt, threshold=threshold, method=method)) if do_nms \
            else len(full[j])
    scores = np.hstack([full[j][:, 4] for j in range(1, num_classes + 1)])
    results, thresh = dict(full), -np.inf
    if len(scores) > max_per_image:
        kth = len(scores) - max_per_image
        thresh = np.partition(scores, kth)[kth]
        results = {j: full[j][full[j][:, 4] >= thresh] for j in full}
    return results, full, live, thresh


def _same(a, b, what=""):
    assert set(a) == set(b)
    for j in a:
        assert a[j].dtype == np.float32 and a[j].shape == b[j].shape and np.array_equal(a[j], b[j]), \
            "%s class %d: %s vs %s rows" % (what, j, a[j].shape, b[j].shape)


@pytest.mark.gpu
def test_fixture_cases_through_the_kernel():
    """(a) every fixture case as the decoded detections of one image (identity crop: (p - 64) * 1 + 64 is exact), all
    rows in one class, no cut: the kernel's class list must equal the compiled reference's array bitwise, tail rows
    included, and its N must be len(keep)."""
    from codenet_amd import harness
    z = np.load(GOLD)
    off = np.concatenate([[0], np.cumsum(z["n"])])
    ident = [{"c": np.array([64.0, 64.0], dtype=np.float32), "s": 128.0, "out_height": 128, "out_width": 128}]
    ran = 0
    for k in range(len(z["n"])):
        n = int(z["n"][k])
        if n == 0:
            continue
        cls = k % 20
        dets = np.concatenate([z["inputs"][off[k]:off[k + 1]], np.full((n, 1), cls, dtype=np.float32)], 1)
        kw = dict(sigma=float(z["sigma"][k]), Nt=float(z["Nt"][k]), threshold=float(z["threshold"][k]),
                  method=int(z["method"][k]))
        _, boxes, rows_out, rows_in, live, thresh = harness.merge_scales_native(
            torch.from_numpy(dets).cuda().view(1, 1, n, 6), ident, [1.0], 20, max_per_image=4096, nms=True, raw=True, **kw)
        want = z["outputs"][off[k]:off[k + 1]]
        got = boxes[0, cls, :n].cpu().numpy()
        assert np.array_equal(got, want) and got.tobytes() == want.tobytes(), "case %d (n = %d, method %d)" % (k, n, kw["method"])
        assert int(live[0, cls]) == int(z["n_keep"][k]) and int(rows_in[0, cls]) == n and int(rows_out[0, cls]) == n
        assert int(rows_out.sum()) == n and float(thresh[0]) == -np.inf
        ran += 1
    assert ran >= 30


def _synthetic(B, S, K, seed):
    """Heavily overlapping detections in output-map pixels, [B, S, K, 6], every (image, scale) in descending score
    order like a decode; scores log-uniform down to the soft-NMS threshold, some exact ties; most rows in 5 classes."""
    rng = np.random.default_rng(seed)
    dets = np.zeros((B, S, K, 6), dtype=np.float32)
    for b in range(B):
        centres = rng.uniform(20, 108, (5, 2))
        for s in range(S):
            c = centres[rng.integers(0, 5, K)] + rng.normal(0, 1.5, (K, 2))
            wh = 24 * np.exp(rng.normal(0, 0.1, (K, 2)))
            sc = np.sort(np.exp(rng.uniform(np.log(1.2e-3), 0, K)))[::-1].copy()
            sc[10:20] = sc[10]                                             # ties inside a scale ...
            if s:
                sc[40:45] = dets[b, 0, 40:45, 4]                            # ... and across scales
            cls = np.where(rng.uniform(size=K) < 0.85, rng.integers(0, 5, K), rng.integers(0, 20, K))
            dets[b, s] = np.concatenate([c - wh / 2, c + wh / 2, sc[:, None], cls[:, None]], 1)
    metas = [[{"c": np.array([250.0 * sc + b, 187.5 * sc], dtype=np.float32), "s": 500.0 + 3 * b,
               "out_height": 128, "out_width": 128} for sc in SCALES[:S]] for b in range(B)]
    return dets, metas


@pytest.mark.gpu
@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("do_nms", [True, False])
@pytest.mark.parametrize("max_per_image", [100, 7])
def test_merge_scales_matches_host_path(method, do_nms, max_per_image):
    """(b) B = 3 images x S = 5 scales x K = 100, 20 classes."""
    from codenet_amd import evalio, harness
    B, S, K = 3, 5, 100
    dets, metas = _synthetic(B, S, K, seed=100 + method)
    gd = torch.from_numpy(dets).cuda()
    got = harness.merge_scales_native(gd, metas, SCALES, 20, max_per_image=max_per_image, nms=do_nms, method=method)
    _, boxes, rows_out, rows_in, live, thresh = harness.merge_scales_native(
        gd, metas, SCALES, 20, max_per_image=max_per_image, nms=do_nms, method=method, raw=True)
    rows_in, live, thresh = rows_in.cpu().numpy(), live.cpu().numpy(), thresh.cpu().numpy()
    assert len(got) == B
    shrunk = 0
    for b in range(B):
        per_scale = [evalio.post_process(torch.from_numpy(dets[b, s:s + 1]), metas[b][s], 20, SCALES[s]) for s in range(S)]
        want, full, n_live, th = _host_merge(per_scale, 20, max_per_image, do_nms, method=method)
        _same(got[b], want, "image %d" % b)
        assert [int(v) for v in rows_in[b]] == [len(full[j]) for j in range(1, 21)]
        assert [int(v) for v in live[b]] == [n_live[j] for j in range(1, 21)]
        assert np.float32(thresh[b]) == np.float32(th)
        shrunk += sum(n_live[j] < len(full[j]) for j in full)
        if do_nms and method == 2:            # the public host entry, as CtdetDetector.run calls it
            _same(got[b], evalio.merge_outputs(per_scale, 20, max_per_image=max_per_image), "merge_outputs %d" % b)
    assert (shrunk > 0) == do_nms, "the synthetic detections must exercise the discard path"


@pytest.mark.gpu
def test_merge_scales_single_scale_and_capacity():
    """One scale without nms is the single-scale merge_outputs; the largest supported shape (4 x 1024 rows) runs."""
    from codenet_amd import evalio, harness
    dets, metas = _synthetic(2, 1, 100, seed=9)
    got = harness.merge_scales_native(torch.from_numpy(dets).cuda(), metas, [1.0], 20, max_per_image=30)
    for b in range(2):
        pc = evalio.post_process(torch.from_numpy(dets[b, 0:1]), metas[b][0], 20, 1.0)
        _same(got[b], evalio.merge_outputs([pc], 20, max_per_image=30))
    dets, metas = _synthetic(1, 4, 1024, seed=10)
    got = harness.merge_scales_native(torch.from_numpy(dets).cuda(), metas, SCALES[:4], 20)
    per_scale = [evalio.post_process(torch.from_numpy(dets[0, s:s + 1]), metas[0][s], 20, SCALES[s]) for s in range(4)]
    _same(got[0], evalio.merge_outputs(per_scale, 20))


def _scale_batch(seed, S=5, res=512):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randn(S, 3, res, res, generator=g)
    images = torch.cat([imgs, torch.flip(imgs, [3])], 0).cuda()
    metas = [{"c": np.array([int(500 * sc) / 2.0, int(375 * sc) / 2.0], dtype=np.float32), "s": 500.0,
              "out_height": res // 4, "out_width": res // 4} for sc in SCALES[:S]]
    return images, metas


def _per_scale_reference(model, images, metas, S):
    from codenet_amd import evalio, harness
    per_scale, dets = [], []
    for s in range(S):
        _, d = harness.process(model, torch.cat([images[s:s + 1], images[S + s:S + s + 1]], 0).contiguous(), flip_test=True)
        dets.append(d.clone())
        per_scale.append(evalio.post_process(dets[-1], metas[s], 20, SCALES[s]))
    return evalio.merge_outputs(per_scale, 20), torch.cat(dets, 0)


@pytest.mark.gpu
def test_process_scales_fp32_equals_per_scale_process():
    """fp32 model (no running-range state): the 5 flip pairs at 512^2 through process_scales against 5 harness.process
    calls, one per pair, followed by the host post_process + merge_outputs -- exactly.

    This holds because process_scales gives the network the reference's batches (one flip pair per call) unless asked
    otherwise.  With the pairs as ONE batch of 10 images (batched=True) it does NOT hold, and not because of the merge:
    measured on the MI355X, on identical inputs layer1 (MIOpen convolutions) already differs between batch 10 and
    batch 2 (whole backbone: max |diff| 1.8e-6), and the fused stages + heads fed IDENTICAL features differ by up to
    1.4e-6 (hm logits), 1.1e-6 (wh), 1.1e-6 (reg) -- their pointwise kernels pick the channel chunk by batch size, which
    changes the summation order; decoded boxes then move by up to 7.6e-6, scores by 4.5e-8.  The figures of both
    modes are printed before the assertion."""
    from codenet_amd import harness
    model = harness.create_model(quantize=False).cuda().enable_fused()
    images, metas = _scale_batch(21)
    S = 5
    want, want_dets = _per_scale_reference(model, images, metas, S)
    _, dets, got = harness.process_scales(model, images, S, True, metas, SCALES)
    assert dets.shape == (S, 100, 6)
    _, bdets, _ = harness.process_scales(model, images, S, True, metas, SCALES, batched=True)
    for name, d in (("per-pair batches", dets), ("one batch of 10", bdets)):
        print("fp32 %s vs per-scale process: dets equal %s, max |diff| boxes %.3g scores %.3g" % (
            name, torch.equal(d, want_dets), (d[..., :4] - want_dets[..., :4]).abs().max().item(),
            (d[..., 4] - want_dets[..., 4]).abs().max().item()))
    assert torch.equal(dets, want_dets)
    _same(got, want, "fp32")
    assert sum(len(v) for v in got.values()) >= 100


@pytest.mark.gpu
@pytest.mark.parametrize("quantize", [False, True])
def test_process_scales_per_pair_batches_equal_per_scale_process(quantize):
    """Per-pair batches (the default): the network sees the reference's batches (one flip pair per call), everything behind it runs on
    all scales at once.  Equal to 5 harness.process calls on a fresh copy of the same model state + the host merge --
    exactly, also for the W4A8 model whose running ranges move with every call."""
    from codenet_amd import harness
    model = harness.create_model(quantize=quantize).cuda()
    m2 = copy.deepcopy(model)
    model.enable_fused()
    m2.enable_fused()
    images, metas = _scale_batch(24)
    S = 5
    want, want_dets = _per_scale_reference(m2, images, metas, S)
    _, dets, got = harness.process_scales(model, images, S, True, metas, SCALES)
    assert torch.equal(dets, want_dets)
    _same(got, want, "per-pair batches")
    assert sum(len(v) for v in got.values()) >= 100
    if not quantize:          # (stateless: the same five passes + merge as one HIP graph)
        replay = harness.capture_process_scales(model, images, S, True, metas, SCALES)
        _, dg, res = replay()
        assert torch.equal(dg, want_dets)
        _same(res, want, "per-pair batches, replay")


@pytest.mark.gpu
def test_process_scales_w4a8_and_graph_replay():
    """Random-weight W4A8 model, S = 5 scales with flip at 512^2.  Its running-range QuantActs see the batch they are
    given, so per-scale calls (batches of 2) and the batched call (10 images) quantise differently BY DESIGN: the
    comparison is against a BATCHED run of an identical model copy -- network on the 10 images, the sigmoid + mirror
    merge and the decode called directly -- merged on the HOST (evalio.post_process + merge_outputs), with
    process_scales(batched=True).  Then the same batch through capture_process_scales(batched=True) on frozen ranges:
    the replay equals the eager call."""
    from codenet_amd import evalio, harness, pipeline, _native as N_
    model = harness.create_model(quantize=True).cuda()
    m2 = copy.deepcopy(model)
    model.enable_fused()
    m2.enable_fused()
    images, metas = _scale_batch(22)
    S = 5
    _, dets, got = harness.process_scales(model, images, S, True, metas, SCALES, batched=True)
    with torch.no_grad():
        out = m2(images)[-1]
        hm2, wh2 = out["hm"].contiguous(), out["wh"].contiguous()
        hm, wh = torch.empty_like(hm2[:S]), torch.empty_like(wh2[:S])
        N_.check(N_.lib().cdn_ctdet_flip_merge(hm2.data_ptr(), wh2.data_ptr(), S, hm2.shape[1], wh2.shape[1], hm2.shape[2],
                                               hm2.shape[3], hm.data_ptr(), wh.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "flip merge")
        d2 = harness.ctdet_decode_native(hm, wh, reg=out["reg"][:S].contiguous(), K=100)
    assert torch.equal(dets, d2)
    per_scale = [evalio.post_process(d2[s:s + 1].clone(), metas[s], 20, SCALES[s]) for s in range(S)]
    _same(got, evalio.merge_outputs(per_scale, 20), "w4a8")
    # ---- graph: frozen ranges make every pass the same function of the image batch
    pipeline.set_running_stat(model, False)
    _, de, eager = harness.process_scales(model, images, S, True, metas, SCALES, batched=True)
    de = de.clone()
    replay = harness.capture_process_scales(model, images, S, True, metas, SCALES, batched=True)
    for _ in range(2):
        _, dg, res = replay()
        assert torch.equal(dg, de)
        _same(res, eager, "replay")
    # a new image batch and new crop parameters through the static buffers
    images2, metas2 = _scale_batch(23)
    for m in metas2:
        m["c"] = m["c"] + np.float32(3.0)
    _, de2, eager2 = harness.process_scales(model, images2, S, True, metas2, SCALES, batched=True)
    de2 = de2.clone()
    images.copy_(images2)
    replay.meta.copy_(harness.scale_metas(metas2, SCALES))
    _, dg2, res2 = replay()
    assert torch.equal(dg2, de2)
    _same(res2, eager2, "replay, second batch")
