"""Writes tests/golden/jpeg_cases.npz with PIL (libjpeg-turbo): JPEG byte streams and PIL's decoded pixels, arrays only.

    python tests/golden/make_jpeg_golden.py

Cases: the sizes 1x1, 8x9, 17x31 (a partial MCU on both axes, an odd chroma width), 33x50, 40x64 (whole MCUs), 48x40
crossed with 4:4:4 / 4:2:2 / 4:2:0 / grey; over that grid the qualities 20, 50 (optimize), 92 (optimize), 100, smooth
content and noise of amplitude 120, and restart interval 0 or 3 MCUs (where the MCU count is no multiple of 3) rotate so
that every sampling meets every quality, both contents and both restart settings.  One 375x500 4:2:0 quality-75 stream is
stored as bytes only.  Streams outside the decoder's supported set (progressive, 4:1:1, 4:4:0, CMYK) are stored as bytes
for the NotImplementedError tests.  Three of the cases are also written as files, jpeg_fuzz_420.jpg,
jpeg_fuzz_444_r3.jpg and jpeg_fuzz_420_q100.jpg: the input of tools/probes/jpeg_host_fuzz.cpp, which reads no numpy
archive.  The tests read the .npz file, never PIL (the GPU tests run where PIL may be missing)."""
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import jpeg_ref  # noqa: E402

SIZES = [(1, 1), (8, 9), (17, 31), (33, 50), (40, 64), (48, 40)]            # (w, h)
SAMPLINGS = ["444", "422", "420", "grey"]
QUALITIES = [(20, False), (50, True), (92, True), (100, False)]             # (quality, optimize)
MCU = {"444": (8, 8), "422": (16, 8), "420": (16, 16), "grey": (8, 8)}
SUB = {"444": 0, "422": 1, "420": 2}


def content(w, h, kind, rng):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 7.0 + y / 11.0), 128 + 90 * np.cos(x / 5.0 - y / 9.0),
                     40 + 3.0 * x + 2.0 * y], axis=2)
    if kind == "noise":
        base = base + rng.uniform(-120, 120, size=base.shape)
    return np.clip(np.rint(base), 0, 255).astype(np.uint8)


def encode(pix, sampling, quality, optimize, restart, **extra):
    img = Image.fromarray(pix[:, :, 1] if sampling == "grey" else pix, "L" if sampling == "grey" else "RGB")
    buf = io.BytesIO()
    kw = dict(quality=quality, optimize=optimize)
    if sampling != "grey":
        kw["subsampling"] = SUB.get(sampling, sampling)
    if restart:
        kw["restart_marker_blocks"] = restart
    kw.update(extra)
    img.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    rng = np.random.RandomState(20240607)
    out, names, stats, seen = {}, [], {}, set()
    for si, sampling in enumerate(SAMPLINGS):
        for zi, (w, h) in enumerate(SIZES):
            quality, optimize = QUALITIES[(zi + si) % 4]
            kind = "noise" if (zi + si // 2) % 2 == 0 else "smooth"
            mw, mh = MCU[sampling]
            mcus = -(-w // mw) * -(-h // mh)
            restart = 3 if (zi % 2 == 1 and mcus % 3 != 0) else 0
            data = encode(content(w, h, kind, rng), sampling, quality, optimize, restart)
            pix = pil_pixels(data)
            assert pix.shape == (h, w, 3)
            assert np.array_equal(jpeg_ref.decode(data, "rgb", stats), pix), (sampling, w, h)
            k = len(names)
            names.append("%s_%dx%d_q%d%s_%s_r%d" % (sampling, w, h, quality, "o" if optimize else "", kind, restart))
            out["jpg_%d" % k], out["pix_%d" % k] = np.frombuffer(data, dtype=np.uint8), pix
            seen |= {(sampling, "q", quality), (sampling, kind), (sampling, "r", restart)}
    for sampling in SAMPLINGS:
        for q, _ in QUALITIES:
            assert (sampling, "q", q) in seen, (sampling, q)
        assert (sampling, "noise") in seen and (sampling, "smooth") in seen
        assert (sampling, "r", 0) in seen and (sampling, "r", 3) in seen, sampling
    assert stats.get("zrl", 0) > 0 and stats.get("code16", 0) > 0 and stats.get("clamped", 0) > 0, stats
    out["names"] = np.array(names)
    big = content(500, 375, "smooth", rng).astype(np.int64) + rng.randint(-12, 13, size=(375, 500, 3))
    big = encode(np.clip(big, 0, 255).astype(np.uint8), "420", 75, False, 0)
    assert np.array_equal(jpeg_ref.decode(big, "rgb"), pil_pixels(big))
    out["big_jpg"] = np.frombuffer(big, dtype=np.uint8)
    # outside the supported set
    small = content(33, 50, "smooth", rng)
    unsupported = {"progressive": encode(small, "420", 75, False, 0, progressive=True)}
    # PIL writes neither 4:1:1 (its "4:1:1" is a legacy name of 4:2:0) nor 4:4:0: a 4:2:2 stream whose frame header declares
    # Y as 4x1 / 1x2 (the decoder refuses on the header; the entropy-coded data is never read)
    for name, hv in (("411", 0x41), ("440", 0x12)):
        d = bytearray(encode(small, "422", 75, False, 0))
        sof = d.index(b"\xff\xc0")
        assert d[sof + 11] == 0x21
        d[sof + 11] = hv
        unsupported[name] = bytes(d)
    buf = io.BytesIO()
    Image.fromarray(np.concatenate([small, small[:, :, :1]], axis=2), "CMYK").save(buf, "JPEG", quality=75)
    unsupported["cmyk"] = buf.getvalue()
    for name, data in unsupported.items():
        out["unsupported_" + name] = np.frombuffer(data, dtype=np.uint8)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    for case, fname in (("420_33x50_q50o_noise_r0", "jpeg_fuzz_420.jpg"), ("444_33x50_q100_smooth_r3", "jpeg_fuzz_444_r3.jpg"),
                        ("420_48x40_q100_noise_r0", "jpeg_fuzz_420_q100.jpg")):       # one segment longer than the stream window
        with open(os.path.join(os.path.dirname(path), fname), "wb") as f:
            f.write(out["jpg_%d" % names.index(case)].tobytes())
    print("%d cases, %s, unsupported: %s, %d bytes" % (len(names), stats, sorted(unsupported), os.path.getsize(path)))


if __name__ == "__main__":
    main()
