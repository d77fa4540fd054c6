"""Baseline JPEG decoding without a GPU (-m "not gpu"): the numpy restatement of DESIGN.md section 7.4d
(tests/jpeg_ref.py) and the library's host decode (cdn_jpeg_decode_host: the text the kernels run) against PIL's pixels
in tests/golden/jpeg_cases.npz, bit for bit; the header parse, the refusals, argument validation and corrupt streams."""
import io

import numpy as np
import pytest

from tests import jpeg_ref as R
from tests.jpeg_cases import FUZZ_CASE, cases, entropy_offset, extra, midpoint_truncation, truncated


def test_restatement_equals_fixture():
    assert len(cases()) == 24
    for name, jpg, pix in cases():
        assert np.array_equal(R.decode(jpg, "rgb"), pix), name
    name, jpg, pix = cases()[2]
    assert np.array_equal(R.decode(jpg, "bgr"), pix[:, :, ::-1])


def test_restatement_equals_a_fresh_pil_decode():
    Image = pytest.importorskip("PIL.Image")
    for name, jpg, pix in cases() + [("big", extra("big_jpg"), None)]:
        fresh = np.asarray(Image.open(io.BytesIO(bytes(jpg))).convert("RGB"))
        assert np.array_equal(R.decode(jpg, "rgb"), fresh), name
    assert fresh.shape == (375, 500, 3)


def test_decode_host_equals_fixture_in_both_orders():
    from codenet_amd import jpeg
    for name, jpg, pix in cases():
        rgb, bgr = jpeg.decode_host([jpg], "rgb")[0], jpeg.JpegDecoder.decode_host([jpg])[0]
        assert rgb.dtype == np.uint8 and np.array_equal(rgb, pix), name
        assert np.array_equal(bgr, pix[:, :, ::-1]), name
    # all of them as one batch, and the large stream against the restatement
    batch = jpeg.decode_host([c[1] for c in cases()], "rgb")
    assert all(np.array_equal(got, c[2]) for got, c in zip(batch, cases()))
    big = extra("big_jpg")
    assert np.array_equal(jpeg.decode_host([bytes(big)])[0], R.decode(big, "bgr"))


def test_parse_returns_the_header_fields():
    from codenet_amd import jpeg
    want = {"444": "4:4:4", "422": "4:2:2", "420": "4:2:0", "grey": "grey"}
    mcu = {"444": (8, 8), "422": (16, 8), "420": (16, 16), "grey": (8, 8)}
    for name, jpg, pix in cases():
        samp, size, _, _, restart = name.split("_")
        info = jpeg.parse(jpg)
        assert (info.h, info.w) == pix.shape[:2] and "%dx%d" % (info.w, info.h) == size
        assert info.sampling == want[samp] and info.components == (1 if samp == "grey" else 3)
        assert info.restart_interval == int(restart[1:])
        mcus = -(-info.w // mcu[samp][0]) * -(-info.h // mcu[samp][1])
        assert info.segments == (-(-mcus // 3) if info.restart_interval else 1), name
    assert jpeg.parse(bytes(extra("big_jpg")))[:4] == (375, 500, 3, "4:2:0")
    assert any(jpeg.parse(c[1]).segments > 3 for c in cases())


def test_unsupported_and_malformed_streams_are_refused_on_the_host():
    from codenet_amd import jpeg
    for kind in ("progressive", "411", "440", "cmyk"):
        data = extra("unsupported_" + kind)
        with pytest.raises(NotImplementedError):
            jpeg.parse(data)
        with pytest.raises(NotImplementedError):
            jpeg.decode_host([cases()[0][1], data])
    good = bytes(cases()[9][1])
    sof = good.index(b"\xff\xc0")
    twelve_bit = good[:sof + 4] + b"\x0c" + good[sof + 5:]
    dqt = good.index(b"\xff\xdb")
    wide_table = good[:dqt + 4] + b"\x10" + good[dqt + 5:]
    for data in (twelve_bit, wide_table):
        with pytest.raises(NotImplementedError):
            jpeg.parse(data)
    for data in (b"", b"\xff\xd8", good[2:], good[:sof + 6], good[:entropy_offset(good) - 3],
                 good[:sof + 2] + b"\xff\xff" + good[sof + 4:], b"\x89PNG\r\n\x1a\n" + bytes(32)):
        with pytest.raises(ValueError):
            jpeg.parse(data)
    with pytest.raises(ValueError):
        jpeg.parse(np.zeros(16, dtype=np.float32))
    with pytest.raises(ValueError):
        jpeg.decode_host([good], order="gbr")


def test_argument_validation_of_the_jpeg_entry_points_without_gpu():
    """Every new entry point validates before it dereferences a pointer or makes a HIP call (fake pointers)."""
    from codenet_amd import _native
    lib = _native.lib()
    one = 4096
    assert lib.cdn_jpeg_parse(None, 10, one) == -1 and lib.cdn_jpeg_parse(one, 10, None) == -1
    assert lib.cdn_jpeg_parse(one, 0, one) == -1
    pack = [one, 10, 0, 0, 3, one, 0, 100, one, 0, 4, one, one, 1024, one]
    for k in (0, 5, 8, 11, 12, 14):                                     # every pointer
        assert lib.cdn_jpeg_pack(*(pack[:k] + [None] + pack[k + 1:])) == -1, k
    for k, v in ((1, 0), (2, -1), (2, 65535), (6, 101), (6, -1), (9, 5), (13, 0), (12, one + 4)):
        assert lib.cdn_jpeg_pack(*(pack[:k] + [v] + pack[k + 1:])) == -1, (k, v)
    assert lib.cdn_jpeg_workspace_bytes(1, 16, 16) == 768 and lib.cdn_jpeg_workspace_bytes(2, 17, 1) == 2 * 1536
    assert lib.cdn_jpeg_workspace_bytes(64, 1024, 1024) == 64 * 3 * 1024 * 1024
    for bad in ((0, 16, 16), (1, 0, 16), (1, 16, 65536)):
        assert lib.cdn_jpeg_workspace_bytes(*bad) == 0
    dec = [one, 100, one, 4, one, 1, one, one, 768, one, one, 3, 0]
    for fn, tail in ((lib.cdn_jpeg_decode, [None]), (lib.cdn_jpeg_decode_host, [])):
        for k in (0, 2, 4, 6, 7, 9, 10):
            assert fn(*(dec[:k] + [None] + dec[k + 1:] + tail)) == -1, k
        for k, v, rc in ((1, 0, -1), (3, 0, -1), (5, 0, -1), (8, 0, -1), (11, 0, -1), (8, 770, -1), (7, one + 4, -1),
                         (6, one + 8, -1), (2, one + 2, -1), (1, 2 ** 31, -5), (5, 65536, -5)):
            assert fn(*(dec[:k] + [v] + dec[k + 1:] + tail)) == rc, (k, v)
        assert fn(*(dec[:8] + [770] + dec[9:] + tail)) == -1 and b"8 bytes" in lib.cdn_last_error()


def test_pack_reports_capacity_overruns_before_writing():
    from codenet_amd import _native, jpeg
    lib = _native.lib()
    name, jpg, pix = [c for c in cases() if c[0] == "grey_33x50_q92o_noise_r3"][0]
    info = jpeg.parse(jpg)
    stride = lib.cdn_jpeg_workspace_bytes(1, info.h, info.w)

    def call(stream_cap, seg_cap, plane_stride):
        bufs = {"stream": np.full(stream_cap + 64, 0xA5, np.uint8), "segs": np.full((1 + seg_cap) * 8 + 16, -1, np.int32),
                "item": np.full(16 + 16, -1, np.int32), "tables": jpeg._aligned(6144 + 64), "used": np.zeros(2, np.int64)}
        bufs["tables"][:] = 0xA5
        rc = lib.cdn_jpeg_pack(jpg.ctypes.data, jpg.size, 0, 0, 3 * info.w, bufs["stream"].ctypes.data, 0, stream_cap,
                               bufs["segs"].ctypes.data, 0, seg_cap, bufs["item"].ctypes.data, bufs["tables"].ctypes.data,
                               plane_stride, bufs["used"].ctypes.data)
        return rc, bufs

    rc, b = call(jpg.size, info.segments, stride)
    assert rc == 0 and tuple(b["used"]) == (b["used"][0], info.segments) and 0 < b["used"][0] < jpg.size
    assert (b["stream"][jpg.size:] == 0xA5).all() and (b["segs"][(1 + info.segments) * 8:] == -1).all()
    assert (b["item"][16:] == -1).all() and (b["tables"][6144:] == 0xA5).all()
    segs = b["segs"][8:(1 + info.segments) * 8].reshape(-1, 8)
    assert list(segs[:, 1]) == list(range(0, 35, 3)) and list(segs[:, 2]) == [3] * 11 + [2]
    assert segs[:, 4].sum() == b["used"][0] and (np.cumsum(segs[:, 4])[:-1] == segs[1:, 3]).all()
    for args in ((16, info.segments, stride), (jpg.size, info.segments - 1, stride), (jpg.size, info.segments, 40 * 56 - 8)):      # the padded plane is 40 x 56
        rc, b = call(*args)
        assert rc == -6, args
        assert (b["stream"] == 0xA5).all() and (b["segs"] == -1).all() and (b["item"] == -1).all()
        assert (b["tables"] == 0xA5).all() and not b["used"].any()


def _fake_pre(capacity=64 * 64 * 3, max_items=4, color_aug=False):
    """A PreProcess without its device buffers: what check_table / load_table look at before they copy."""
    from codenet_amd import preproc
    pre = object.__new__(preproc.PreProcess)
    pre.in_h = pre.in_w = 64
    pre.capacity, pre.max_items, pre.color_aug = capacity, max_items, color_aug
    return pre


def test_load_table_refuses_rows_outside_the_bytes():
    from codenet_amd import preproc
    pre = _fake_pre()
    M = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    good = preproc.item_row(30, 20, 31, 100, M)
    rows, aug = pre.check_table(30 + 19 * 100 + 93, [good])
    assert len(rows) == 1 and rows[0][:6] == [30.0, 20.0, 31.0, 100.0, 20.0, 31.0] and aug is None
    for nbytes, table in ((30 + 19 * 100 + 92, [good]),                                  # the last row ends one byte outside
                          (4000, [preproc.item_row(-1, 20, 31, 100, M)]), (4000, [preproc.item_row(0, 20, 31, 92, M)]),
                          (4000, [preproc.item_row(0, 0, 31, 100, M)]), (4000, [good] * 5),          # 5 items of 4
                          (64 * 64 * 3 + 1, [good]), (4000, [preproc.item_row(0, 20.5, 31, 100, M)]),
                          (4000, [preproc.item_row(0, 20, 31, 100, [1.0, 0.0, 2.0 ** 20, 0.0, 1.0, 0.0])]), (4000, [])):
        with pytest.raises(ValueError):
            pre.load_table(nbytes, table)               # refused before anything touches the device
    with pytest.raises(ValueError):
        pre.load_table(4000, [good], aug=[preproc.AUG_OFF])             # aug rows need color_aug=True
    with pytest.raises(ValueError):
        _fake_pre(color_aug=True).load_table(4000, [good], aug=[preproc.AUG_OFF] * 2)


def _assert_guards(r, what):
    g = r["guard"]
    assert g >= 64
    for buf in (r["out_buf"], r["planes_buf"]):
        assert (buf[:g] == 0xA5).all() and (buf[len(buf) - g:] == 0xA5).all(), what


def test_corrupt_streams_end_and_stay_inside_their_buffers():
    from codenet_amd import jpeg
    name, jpg, pix = [c for c in cases() if c[0] == FUZZ_CASE][0]
    off, n = entropy_offset(jpg), len(jpg)
    r = jpeg.decode_host_raw([jpg], "rgb", guard=64)
    assert r["status"][0] == 0 and np.array_equal(r["out"].reshape(pix.shape), pix)
    _assert_guards(r, "intact")
    flagged = 0
    for cut in range(off, n, 7):                        # a truncation at every 7th byte of the entropy-coded data
        r = jpeg.decode_host_raw([truncated(jpg, cut)], guard=64)
        _assert_guards(r, "cut %d" % cut)
        flagged += int(r["status"][0] != 0)
    assert flagged >= len(range(off, n, 7)) - 1         # every cut loses data, but for one that removes little more than EOI
    with pytest.raises(RuntimeError):
        jpeg.decode_host([midpoint_truncation(jpg)])
    rng = np.random.RandomState(7)
    for k in range(200):                                # seeded single-bit flips in the entropy-coded data
        d = np.array(jpg)
        d[off + rng.randint(n - off - 2)] ^= 1 << rng.randint(8)
        try:
            r = jpeg.decode_host_raw([d], guard=64)
        except (ValueError, NotImplementedError):       # the flip made a marker: refused by the host parse
            continue
        _assert_guards(r, "flip %d" % k)
        assert r["status"][0] in (0, 1, 2)
