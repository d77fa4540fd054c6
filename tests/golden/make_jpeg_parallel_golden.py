"""Writes tests/golden/jpeg_parallel_cases.npz with PIL (libjpeg-turbo): streams that stress the state machine of the
parallel entropy path, each with PIL's decoded pixels, arrays only, as make_jpeg_golden.py does.

    python tests/golden/make_jpeg_parallel_golden.py

flat_opt   a flat 256 x 256 image of grey level 128, 4:2:0, quality 75, optimize=True: about 2 bits per block, 1536
           blocks, dozens of them in every 64-bit sub-sequence.  A lane that starts cold starts on the wrong block of the
           MCU and cannot fall into step, so the synchronisation rounds run to the induction bound.
flat_std   the same image with the standard tables: one MCU is exactly 32 bits, so block boundaries fall on sub-sequence
           boundaries.
noise      a 64 x 48 noise image at quality 100, 4:4:4: blocks far longer than 64 bits, so many sub-sequences complete no
           block.
tiny       a 1 x 1 image: one segment that is one sub-sequence."""
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import jpeg_ref  # noqa: E402


def encode(pix, **kw):
    buf = io.BytesIO()
    Image.fromarray(pix, "RGB").save(buf, "JPEG", **kw)
    return buf.getvalue()


def main():
    rng = np.random.RandomState(20240901)
    flat = np.full((256, 256, 3), 128, dtype=np.uint8)
    noise = rng.randint(0, 256, size=(48, 64, 3)).astype(np.uint8)
    streams = [("flat_opt", encode(flat, quality=75, subsampling=2, optimize=True)),
               ("flat_std", encode(flat, quality=75, subsampling=2, optimize=False)),
               ("noise", encode(noise, quality=100, subsampling=0)),
               ("tiny", encode(np.full((1, 1, 3), 90, dtype=np.uint8), quality=75, subsampling=2))]
    out = {"names": np.array([n for n, _ in streams])}
    for k, (name, data) in enumerate(streams):
        pix = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert np.array_equal(jpeg_ref.decode(data, "rgb"), pix), name
        out["jpg_%d" % k], out["pix_%d" % k] = np.frombuffer(data, dtype=np.uint8), pix
        hd = jpeg_ref.parse(data)
        bits = 8 * len(jpeg_ref._segments(hd["entropy"])[0])
        print("%s: %d bytes, %d entropy-coded bits, %s" % (name, len(data), bits, pix.shape))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_parallel_cases.npz")
    np.savez_compressed(path, **out)
    print("%d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
