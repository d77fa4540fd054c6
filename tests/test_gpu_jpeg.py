"""The JPEG kernels (codenet_jpeg.hip: jpeg_entropy_idct_kernel, jpeg_color_kernel; codenet_amd/jpeg.py) against PIL's
pixels in tests/golden/jpeg_cases.npz.  The arithmetic is integer: every comparison is
torch.equal over the whole image.  The fixture is read from the file; PIL is not needed here."""
import functools

import numpy as np
import pytest
import torch

from tests.jpeg_cases import FUZZ_CASE, cases, extra, midpoint_truncation

pytestmark = pytest.mark.gpu


def _bgr(pix):
    return torch.from_numpy(np.ascontiguousarray(pix[:, :, ::-1]))


@functools.lru_cache(maxsize=None)
def _decoder(max_items):
    from codenet_amd import jpeg
    return jpeg.JpegDecoder(max_items=max_items, max_h=64, max_w=64, max_segments=16 * max_items)    # 3-MCU restarts


def _check_batch(dec, out, batch, what=""):
    for (name, _, pix), img in zip(batch, dec.images(out)):
        assert torch.equal(img.cpu(), _bgr(pix)), "%s %s" % (what, name)
    assert not dec.status.any()


def test_every_case_one_item_at_a_time():
    dec = _decoder(1)
    out = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    for case in cases():
        infos = dec.load([case[1]])
        assert (infos[0].h, infos[0].w) == case[2].shape[:2] and dec.layout == [(0, infos[0].h, infos[0].w, 3 * infos[0].w)]
        dec.run(out)
        dec.check()
        _check_batch(dec, out, [case])


def test_all_cases_in_one_batch_and_rgb_order():
    from codenet_amd import jpeg
    n = len(cases())
    dec = _decoder(n)
    dec.load([bytes(c[1]) if k % 2 else c[1] for k, c in enumerate(cases())])       # bytes and uint8 arrays
    off = 0
    for (o, h, w, pitch), c in zip(dec.layout, cases()):
        assert (o, h, w, pitch) == (off, c[2].shape[0], c[2].shape[1], 3 * c[2].shape[1])
        off += h * w * 3
    assert dec.out_bytes == off
    out = torch.full((off + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dec.run(out)
    dec.check()
    _check_batch(dec, out, cases())
    assert (out[off:] == 0xA5).all()
    rgb = jpeg.JpegDecoder(max_items=3, max_h=64, max_w=64, max_segments=48, order="rgb")
    picks = [cases()[3], cases()[14], cases()[21]]
    rgb.load([c[1] for c in picks])
    rgb.run(out)
    rgb.check()
    for c, img in zip(picks, rgb.images(out)):
        assert torch.equal(img.cpu(), torch.from_numpy(c[2].copy())), c[0]


def test_a_voc_sized_stream_equals_the_host_decode():
    from codenet_amd import jpeg
    big = extra("big_jpg")
    want = torch.from_numpy(jpeg.decode_host([big])[0])
    dec = jpeg.JpegDecoder(max_items=2, max_h=375, max_w=500)
    out = torch.zeros(2 * 375 * 500 * 3, dtype=torch.uint8, device="cuda")
    dec.load([big, big])
    dec.run(out)
    dec.check()
    for img in dec.images(out):
        assert img.shape == (375, 500, 3) and torch.equal(img.cpu(), want)


def test_captured_run_replays_for_batches_of_other_sizes_and_samplings():
    dec = _decoder(4)
    first = [cases()[k] for k in (4, 9, 15, 21)]            # 4:4:4 40x64, 4:2:2 33x50, 4:2:0 33x50, grey 33x50 (restarts)
    second = [cases()[k] for k in (13, 20, 3)]              # 4:2:0 8x9 (restarts), grey 17x31, 4:4:4 33x50 (restarts)
    out = torch.zeros(4 * 64 * 64 * 3, dtype=torch.uint8, device="cuda")
    dec.load([c[1] for c in first])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dec.run(out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dec.run(out)
    for batch in (second, first):
        dec.load([c[1] for c in batch])
        out.zero_()
        graph.replay()
        dec.check()
        _check_batch(dec, out, batch, "replay")


def test_jpeg_pre_process_equals_pre_process_of_the_decoded_pixels():
    from codenet_amd import jpeg, preproc
    name, jpg, pix = cases()[15]
    img = np.ascontiguousarray(pix[:, :, ::-1])
    # test mode: two scales with flip_test
    pre = preproc.PreProcess(64, 64, scales=(1.0, 0.5), flip_test=True, max_h=64, max_w=64)
    want_metas = pre.load(img)
    want = pre.run(torch.zeros(4, 3, 64, 64, device="cuda")).clone()
    pre.arena.zero_()
    jp = jpeg.JpegPreProcess(_decoder(1), pre)
    metas = jp.load(jpg)
    got = jp.run(torch.zeros(4, 3, 64, 64, device="cuda"))
    assert torch.equal(got, want)
    assert len(metas) == 2 and all(np.array_equal(a["c"], b["c"]) and a["s"] == b["s"] for a, b in zip(metas, want_metas))
    # training mode: a table of three items over two images, colour augmentation on
    batch = [cases()[15], cases()[9]]
    pre = preproc.PreProcess(48, 80, max_h=64, max_w=64, max_items=3, color_aug=True)
    rng = np.random.RandomState(3)
    aug = [preproc.color_aug_params(rng, shuffle=lambda o: rng.shuffle(o)) for _ in range(2)] + [preproc.AUG_OFF]

    def table(layout):
        (o0, h0, w0, p0), (o1, h1, w1, p1) = layout
        return [preproc.item_row(o0, h0, w0, p0, preproc.train_matrix([w0 / 2.0, h0 / 2.0], 40.0, 80, 48)),
                preproc.item_row(o1, h1, w1, p1, preproc.train_matrix([10.0, 30.0], 70.0, 80, 48), flip_src=True),
                preproc.item_row(o0, h0, w0, p0, preproc.train_matrix([20.0, 20.0], 25.0, 80, 48))]

    arena = np.concatenate([np.ascontiguousarray(c[2][:, :, ::-1]).reshape(-1) for c in batch])
    layout = [(0, 50, 33, 99), (50 * 33 * 3, 50, 33, 99)]
    pre.load_items(arena, table(layout), aug=aug)
    want = pre.run(torch.zeros(3, 3, 48, 80, device="cuda")).clone()
    pre.arena.zero_()
    jp = jpeg.JpegPreProcess(_decoder(4), pre)
    rows = jp.load([c[1] for c in batch], table=table, aug=aug)
    assert len(rows) == 3
    got = jp.run(torch.zeros(3, 3, 48, 80, device="cuda"))
    assert torch.equal(got, want)
    # a row outside the decoded bytes is refused before anything is copied
    with pytest.raises(ValueError):
        jp.load([c[1] for c in batch], table=lambda lay: [preproc.item_row(lay[1][0], 51, 33, 99, [1, 0, 0, 0, 1, 0])], aug=None)
    assert torch.equal(jp.run(torch.zeros(3, 3, 48, 80, device="cuda")), want)


def test_errors_leave_the_stream_usable():
    from codenet_amd import jpeg
    dec = _decoder(4)
    out = torch.zeros(4 * 64 * 64 * 3, dtype=torch.uint8, device="cuda")
    good = [cases()[k] for k in (16, 2)]
    dec.load([c[1] for c in good])
    with pytest.raises(NotImplementedError):
        dec.load([good[0][1], extra("unsupported_progressive")])
    with pytest.raises(ValueError):
        dec.load([good[0][1], bytes(good[1][1])[:40]])
    with pytest.raises(ValueError):
        dec.load([c[1] for c in cases()[:5]])                       # five streams, four items
    with pytest.raises(ValueError):
        dec.load([extra("big_jpg")])                                # 375 x 500 into planes of 64 x 64
    with pytest.raises(ValueError):
        dec.run(out[:100])
    with pytest.raises(NotImplementedError):
        dec.run(out.cpu())
    dec.run(out)                                                    # the batch loaded before the refusals
    dec.check()
    _check_batch(dec, out, good)
    with pytest.raises(NotImplementedError):
        jpeg.JpegDecoder(device="cpu")


def test_a_truncated_stream_raises_in_check_and_leaves_the_other_items_alone():
    """The one malformed stream decoded on the GPU: the midpoint truncation of the host test's 4:2:0 stream (the host
    decode of the same bytes and the sanitizer run of tools/probes/jpeg_host_fuzz.cpp are clean)."""
    dec = _decoder(4)
    out = torch.zeros(4 * 64 * 64 * 3, dtype=torch.uint8, device="cuda")
    victim = [c for c in cases() if c[0] == FUZZ_CASE][0]
    batch = [cases()[5], victim, cases()[22]]
    dec.load([batch[0][1], midpoint_truncation(victim[1]), batch[2][1]])
    dec.run(out)
    with pytest.raises(RuntimeError, match="item 1"):
        dec.check()
    assert dec.status.tolist() == [0, 1, 0]
    imgs = dec.images(out)
    assert torch.equal(imgs[0].cpu(), _bgr(batch[0][2])) and torch.equal(imgs[2].cpu(), _bgr(batch[2][2]))
