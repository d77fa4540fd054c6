"""tests/golden/jpeg_cases.npz (written by tests/golden/make_jpeg_golden.py with PIL) as the JPEG tests read it: byte
streams and PIL's decoded pixels, loaded once and shared read-only, and the corrupt variants both test files use."""
import functools
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")
FUZZ_CASE = "420_33x50_q50o_noise_r0"           # the 4:2:0 stream of the corruption tests (tests/golden/jpeg_fuzz_420.jpg)


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, JPEG bytes, PIL's RGB pixels)], read once and shared (read-only)."""
    z = np.load(G)
    out = []
    for k, name in enumerate(z["names"]):
        jpg, pix = z["jpg_%d" % k], z["pix_%d" % k]
        jpg.setflags(write=False)
        pix.setflags(write=False)
        out.append((str(name), jpg, pix))
    return out


@functools.lru_cache(maxsize=None)
def extra(name):
    a = np.load(G)[name]
    a.setflags(write=False)
    return a


def entropy_offset(data):
    """First byte of the entropy-coded data: behind the SOS header."""
    d = bytes(data)
    sos = d.index(b"\xff\xda")
    return sos + 2 + ((d[sos + 2] << 8) | d[sos + 3])


def truncated(data, cut):
    return np.frombuffer(bytes(data)[:cut], dtype=np.uint8)


def midpoint_truncation(data):
    """The one malformed stream the GPU test decodes: cut in the middle of the entropy-coded data."""
    off = entropy_offset(data)
    return truncated(data, off + (len(data) - off) // 2)
