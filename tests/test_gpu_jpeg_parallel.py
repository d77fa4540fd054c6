"""The parallel entropy path on the GPU (codenet_jpeg.hip: jpeg_entropy_parallel_kernel, jpeg_idct_kernel;
JpegDecoder(entropy="parallel")) against PIL's pixels in tests/golden/jpeg_cases.npz and jpeg_parallel_cases.npz.  The
arithmetic is integer: every comparison is torch.equal over the whole image."""
import functools

import numpy as np
import pytest
import torch

from tests.jpeg_cases import FUZZ_CASE, cases, extra, midpoint_truncation
from tests.test_jpeg_parallel_host import all_cases, parallel_cases

pytestmark = pytest.mark.gpu


def _bgr(pix):
    return torch.from_numpy(np.ascontiguousarray(pix[:, :, ::-1]))


@functools.lru_cache(maxsize=None)
def _decoder(max_items, S, side=64):
    from codenet_amd import jpeg
    # (the noise stream of jpeg_parallel_cases.npz has 13 KB: more than the default of one byte per pixel)
    return jpeg.JpegDecoder(max_items=max_items, max_h=side, max_w=side, max_stream_bytes=16384 * max_items,
                            max_segments=16 * max_items, entropy="parallel", subseq_bits=S)


def _check_batch(dec, out, batch, what=""):
    for (name, _, pix), img in zip(batch, dec.images(out)):
        assert torch.equal(img.cpu(), _bgr(pix)), "%s %s" % (what, name)
    assert not dec.status.any()


@pytest.mark.parametrize("S", [64, 128, 1024])
def test_every_case_one_item_at_a_time(S):
    out = torch.zeros(256 * 256 * 3, dtype=torch.uint8, device="cuda")
    for case in all_cases():
        dec = _decoder(1, S, 256 if max(case[2].shape) > 64 else 64)
        dec.load([case[1]])
        dec.run(out)
        dec.check()
        _check_batch(dec, out, [case], "S %d" % S)


def test_all_cases_in_one_batch_leave_the_tail_alone():
    n = len(cases())
    dec = _decoder(n, 64)
    dec.load([c[1] for c in cases()])
    out = torch.full((dec.out_bytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dec.run(out)
    dec.check()
    _check_batch(dec, out, cases())
    assert (out[dec.out_bytes:] == 0xA5).all()


@pytest.mark.parametrize("S", [64, 1024])
def test_a_voc_sized_stream_equals_the_serial_host_decode(S):
    from codenet_amd import jpeg
    big = extra("big_jpg")
    want = torch.from_numpy(jpeg.decode_host([big])[0])
    dec = jpeg.JpegDecoder(max_items=2, max_h=375, max_w=500, entropy="parallel", subseq_bits=S)
    out = torch.zeros(2 * 375 * 500 * 3, dtype=torch.uint8, device="cuda")
    dec.load([big, big])
    dec.run(out)
    dec.check()
    for img in dec.images(out):
        assert img.shape == (375, 500, 3) and torch.equal(img.cpu(), want)


def test_the_flat_image_whose_rounds_run_to_the_induction_bound():
    case = [c for c in parallel_cases() if c[0] == "flat_opt"][0]
    dec = _decoder(1, 64, 256)
    out = torch.zeros(256 * 256 * 3, dtype=torch.uint8, device="cuda")
    dec.load([case[1]])
    dec.run(out)
    dec.check()
    _check_batch(dec, out, [case])


def test_captured_run_replays_for_batches_of_other_sizes_and_samplings():
    dec = _decoder(4, 64)
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


def test_a_truncated_stream_raises_in_check_and_leaves_the_other_items_alone():
    """The one malformed stream decoded on the GPU: the midpoint truncation of the host test's 4:2:0 stream, whose host
    decode through the same text is clean (tests/test_jpeg_parallel_host.py, tools/probes/jpeg_host_fuzz.cpp)."""
    from codenet_amd import jpeg
    dec = _decoder(4, 64)
    out = torch.zeros(4 * 64 * 64 * 3, dtype=torch.uint8, device="cuda")
    victim = [c for c in cases() if c[0] == FUZZ_CASE][0]
    batch = [cases()[5], victim, cases()[22]]
    datas = [batch[0][1], midpoint_truncation(victim[1]), batch[2][1]]
    host = jpeg.decode_host_raw(datas, entropy="parallel", subseq_bits=64)
    dec.load(datas)
    dec.run(out)
    with pytest.raises(RuntimeError, match="item 1"):
        dec.check()
    assert dec.status.tolist() == host["status"].tolist() and host["status"][1] != 0
    imgs = dec.images(out)
    assert torch.equal(imgs[0].cpu(), _bgr(batch[0][2])) and torch.equal(imgs[2].cpu(), _bgr(batch[2][2]))


def test_jpeg_pre_process_over_a_parallel_decoder_equals_pre_process_of_the_decoded_pixels():
    from codenet_amd import jpeg, preproc
    name, jpg, pix = cases()[15]
    pre = preproc.PreProcess(64, 64, scales=(1.0, 0.5), flip_test=True, max_h=64, max_w=64)
    pre.load(np.ascontiguousarray(pix[:, :, ::-1]))
    want = pre.run(torch.zeros(4, 3, 64, 64, device="cuda")).clone()
    pre.arena.zero_()
    jp = jpeg.JpegPreProcess(_decoder(1, 1024), pre)
    jp.load(jpg)
    assert torch.equal(jp.run(torch.zeros(4, 3, 64, 64, device="cuda")), want)
