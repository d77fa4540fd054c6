"""The parallel entropy path of the JPEG decoder without a GPU (-m "not gpu"): the Python restatement of its tile algorithm
(tests/jpeg_parallel_ref.py) against the serial restatement, and the library's host routine
(cdn_jpeg_decode_parallel_host: the text jpeg_entropy_parallel_kernel and jpeg_idct_kernel run) against PIL's pixels in
tests/golden/jpeg_cases.npz and tests/golden/jpeg_parallel_cases.npz, bit for bit; corrupt streams and argument
validation."""
import functools
import os

import numpy as np
import pytest

from tests import jpeg_parallel_ref as P
from tests.jpeg_cases import FUZZ_CASE, cases, entropy_offset, extra, midpoint_truncation, truncated

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_parallel_cases.npz")


@functools.lru_cache(maxsize=None)
def parallel_cases():
    """[(name, JPEG bytes, PIL's RGB pixels)] of jpeg_parallel_cases.npz, read once and shared (read-only)."""
    z = np.load(G)
    out = []
    for k, name in enumerate(z["names"]):
        jpg, pix = z["jpg_%d" % k], z["pix_%d" % k]
        jpg.setflags(write=False)
        pix.setflags(write=False)
        out.append((str(name), jpg, pix))
    return out


def all_cases():
    return cases() + parallel_cases()


@functools.lru_cache(maxsize=None)
def _serial_blocks(k):
    return P.serial_blocks(all_cases()[k][1])


@pytest.mark.parametrize("S", [64, 96, 1024])
def test_restatement_equals_the_serial_restatement(S):
    assert len(all_cases()) == 28
    for k, (name, jpg, _) in enumerate(all_cases()):
        want, got = _serial_blocks(k), P.parallel_blocks(jpg, S)
        assert len(want) == len(got), name
        for (cw, sw), (cg, sg) in zip(want, got):
            assert sw == 0 and sg == 0 and np.array_equal(cw, cg), name


def test_restatement_with_small_tiles_and_the_induction_bound():
    """W = 4 gives many tiles on every stream; on the flat image with optimised tables a cold lane starts on the wrong block
    of the MCU and never falls into step, so the rounds run until the exact state has walked through the tile."""
    for k, (name, jpg, _) in enumerate(all_cases()):
        for (cw, _), (cg, sg) in zip(_serial_blocks(k), P.parallel_blocks(jpg, 64, W=4)):
            assert sg == 0 and np.array_equal(cw, cg), name
    k = [c[0] for c in all_cases()].index("flat_opt")
    seen = []
    got = P.parallel_blocks(all_cases()[k][1], 64, W=256, rounds_seen=seen)
    assert np.array_equal(got[0][0], _serial_blocks(k)[0][0])
    assert max(seen) >= 40                              # 48 sub-sequences of 64 bits: the state is handed on lane by lane


@pytest.mark.parametrize("S", [64, 96, 128, 1024, 8192])
def test_decode_host_parallel_equals_pil(S):
    from codenet_amd import jpeg
    for name, jpg, pix in all_cases():
        got = jpeg.decode_host([jpg], "rgb", entropy="parallel", subseq_bits=S)[0]
        assert got.dtype == np.uint8 and np.array_equal(got, pix), name
    batch = jpeg.JpegDecoder.decode_host([c[1] for c in all_cases()], entropy="parallel", subseq_bits=S)
    assert all(np.array_equal(got, c[2][:, :, ::-1]) for got, c in zip(batch, all_cases()))


@pytest.mark.parametrize("S", [64, 1024])
def test_decode_host_parallel_of_a_voc_sized_stream_equals_the_serial_decode(S):
    from codenet_amd import jpeg
    big = extra("big_jpg")                              # at S = 64 about 4900 sub-sequences: more tiles than any W
    r = jpeg.decode_host_raw([big], entropy="parallel", subseq_bits=S)
    assert r["status"][0] == 0
    assert np.array_equal(r["out"].reshape(375, 500, 3), jpeg.decode_host([big])[0])
    assert np.array_equal(r["planes"], jpeg.decode_host_raw([big])["planes"])


def _assert_guards(r, what):
    g = r["guard"]
    assert g >= 64
    for buf in (r["out_buf"], r["planes_buf"], r["work_buf"]):
        assert (buf[:g] == 0xA5).all() and (buf[len(buf) - g:] == 0xA5).all(), what


def test_corrupt_streams_stay_inside_their_buffers_and_are_flagged_as_the_serial_decode_flags_them():
    from codenet_amd import jpeg
    name, jpg, pix = [c for c in cases() if c[0] == FUZZ_CASE][0]
    off, n = entropy_offset(jpg), len(jpg)
    r = jpeg.decode_host_raw([jpg], "rgb", guard=64, entropy="parallel", subseq_bits=64)
    assert r["status"][0] == 0 and np.array_equal(r["out"].reshape(pix.shape), pix)
    _assert_guards(r, "intact")
    flagged = 0
    for data in [truncated(jpg, cut) for cut in range(off, n, 7)] + [midpoint_truncation(jpg)]:
        serial = jpeg.decode_host_raw([data], guard=64)
        r = jpeg.decode_host_raw([data], guard=64, entropy="parallel", subseq_bits=64)
        _assert_guards(r, "cut %d" % len(data))
        assert r["status"][0] in (0, 1, 2) and (r["status"][0] != 0) == (serial["status"][0] != 0), len(data)
        flagged += int(r["status"][0] != 0)
    assert flagged >= len(range(off, n, 7))
    with pytest.raises(RuntimeError, match="item 0"):
        jpeg.decode_host([midpoint_truncation(jpg)], entropy="parallel", subseq_bits=64)


def test_argument_validation_of_the_parallel_entry_points_without_gpu():
    """The new entry points validate before they dereference a pointer or make a HIP call (fake pointers)."""
    from codenet_amd import _native, jpeg
    lib = _native.lib()
    one = 4096
    assert lib.cdn_jpeg_parallel_workspace_bytes(1, 16, 16) == 768 * 33 // 16
    assert lib.cdn_jpeg_parallel_workspace_bytes(64, 1024, 1024) == 64 * 3 * 1024 * 1024 * 33 // 16
    assert lib.cdn_jpeg_parallel_workspace_bytes(1, 375, 500) == 384 * 512 * 3 * 33 // 16
    for bad in ((0, 16, 16), (1, 0, 16), (1, 16, 65536)):
        assert lib.cdn_jpeg_parallel_workspace_bytes(*bad) == 0
    need = 768 * 33 // 16
    dec = [one, 100, one, 4, one, 1, one, one, 768, one, one, 3, 0, one, need, 64]
    for fn, tail in ((lib.cdn_jpeg_decode_parallel, [None]), (lib.cdn_jpeg_decode_parallel_host, [])):
        for k in (0, 2, 4, 6, 7, 9, 10, 13):                            # every pointer
            assert fn(*(dec[:k] + [None] + dec[k + 1:] + tail)) == -1, k
        for bits in (0, 32, 63, 65, 80, 8192 + 32, 16384, -64):
            assert fn(*(dec[:15] + [bits] + tail)) == -1, bits
        assert b"subseq_bits" in lib.cdn_last_error()
        for k, v, rc in ((14, need - 1, -1), (14, 0, -1), (13, one + 8, -1), (13, one + 2, -1), (8, 0, -1), (8, 770, -1),
                         (1, 0, -1), (1, 2 ** 31, -5), (5, 65536, -5)):
            assert fn(*(dec[:k] + [v] + dec[k + 1:] + tail)) == rc, (k, v)
        assert fn(*(dec[:5] + [2] + dec[6:] + tail)) == -1 and b"workspace" in lib.cdn_last_error()       # two items, room for one
    for kw in ({"entropy": "fast"}, {"entropy": "parallel", "subseq_bits": 100}, {"entropy": "parallel", "subseq_bits": 32}):
        with pytest.raises(ValueError):
            jpeg.decode_host([cases()[0][1]], **kw)
        with pytest.raises(ValueError):
            jpeg.decode_host_raw([cases()[0][1]], **kw)
        with pytest.raises(ValueError):
            jpeg.JpegDecoder(device="cpu", **kw)        # refused before the device is looked at
