"""Writes tests/golden/soft_nms_ref.npz: inputs and the FULL in-place outputs (tail rows included) plus len(keep) of the
reference's compiled soft_nms (lib/models/external/nms.pyx:77-170) on ~40 small cases.  Runs in the build container only,
like make_golden.py: it needs the reference checkout, Cython and a C compiler.

    python tests/golden/make_soft_nms_golden.py /path/to/reference

The reference file is copied to a temporary directory without its unrelated hard `nms` function (np.int_t / np.int /
np.float no longer exist in this numpy, the file does not compile with it), cythonized with language_level=2 and numpy's
include directory, and its soft_nms is run.  The fixture holds arrays only.

Layout: cases are concatenated; case k owns rows off[k] : off[k] + n[k] of `inputs` / `outputs`.
    n, n_keep, method [cases]; sigma, Nt, threshold [cases] float32; tags [cases] uint16 bit set (TAGS below), found by a
    Python trace of the same loop (which is also checked against the compiled result, bit for bit).
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TAGS = {"shrinks": 1, "pulled_row_discarded": 2, "tie_at_max": 4, "identical_boxes": 8, "disjoint_boxes": 16,
        "discarded_in_place": 32}


def build_reference(ref_root):
    src = open(os.path.join(ref_root, "lib", "models", "external", "nms.pyx")).read()
    a, b, c = src.index("def nms("), src.index("def soft_nms("), src.index("def soft_nms_39(")
    tmp = tempfile.mkdtemp(prefix="softnms_ref_")
    with open(os.path.join(tmp, "refnms.pyx"), "w") as f:
        f.write(src[:a] + src[b:c])
    with open(os.path.join(tmp, "setup.py"), "w") as f:
        f.write("import numpy\nfrom setuptools import setup, Extension\nfrom Cython.Build import cythonize\n"
                "setup(ext_modules=cythonize([Extension('refnms', ['refnms.pyx'], include_dirs=[numpy.get_include()])],"
                " language_level=2))\n")
    subprocess.check_call([sys.executable, "setup.py", "-q", "build_ext", "--inplace"], cwd=tmp)
    sys.path.insert(0, tmp)
    import refnms
    return refnms, tmp


f32 = np.float32


def trace(boxes, sigma, Nt, threshold, method):
    """The loop of nms.pyx with the widths of Cython's C (f32(): float32 rounding, the rest double) -> (array, N, tags)."""
    b = boxes.copy()
    N, tags = b.shape[0], 0
    sigma, Nt, threshold = f32(sigma), f32(Nt), f32(threshold)
    for i in range(b.shape[0]):
        if i >= N:
            break
        maxpos = i + int(np.argmax(b[i:N, 4]))          # first maximum == strict < scan
        if np.sum(b[i:N, 4] == b[maxpos, 4]) > 1:
            tags |= TAGS["tie_at_max"]
        b[[i, maxpos]] = b[[maxpos, i]]
        tx1, ty1, tx2, ty2 = b[i, :4]
        pos, pulled = i + 1, False
        while pos < N:
            x1, y1, x2, y2, s = b[pos]
            area = f32((float(f32(x2 - x1)) + 1.0) * (float(f32(y2 - y1)) + 1.0))
            iw = f32(float(f32(min(tx2, x2) - max(tx1, x1))) + 1.0)
            ih = f32(float(f32(min(ty2, y2) - max(ty1, y1))) + 1.0)
            discarded = False
            if not (iw > 0 and ih > 0):
                tags |= TAGS["disjoint_boxes"]
            else:
                inter = f32(iw * ih)
                ua = f32((float(f32(tx2 - tx1)) + 1.0) * (float(f32(ty2 - ty1)) + 1.0) + float(area) - float(inter))
                ov = f32(inter / ua)
                if ov == 1 and (x1, y1, x2, y2) == (tx1, ty1, tx2, ty2):
                    tags |= TAGS["identical_boxes"]
                if method == 1:
                    w = f32(1.0 - float(ov)) if ov > Nt else f32(1)
                elif method == 2:
                    w = f32(np.exp(float(f32(f32(-(ov * ov)) / sigma))))
                else:
                    w = f32(0) if ov > Nt else f32(1)
                b[pos, 4] = f32(w * s)
                if b[pos, 4] < threshold:
                    tags |= TAGS["shrinks"]
                    if pulled:
                        tags |= TAGS["pulled_row_discarded"]
                    if pos == N - 1:
                        tags |= TAGS["discarded_in_place"]
                    b[pos] = b[N - 1]
                    N -= 1
                    discarded = True
            pulled = discarded
            if not discarded:
                pos += 1
    return b, N, tags


def boxes_around(rng, centres, n, size, jitter, scores):
    c = centres[rng.integers(0, len(centres), n)] + rng.normal(0, jitter, (n, 2))
    wh = size * np.exp(rng.normal(0, 0.15, (n, 2)))
    return np.concatenate([c - wh / 2, c + wh / 2, scores.reshape(-1, 1)], 1).astype(np.float32)


def make_cases():
    rng = np.random.default_rng(20240607)
    cases = []

    def add(b, method, sigma=0.5, Nt=0.5, threshold=0.001):
        cases.append((np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 5), method, sigma, Nt, threshold))

    add(np.zeros((0, 5)), 2)                                             # n = 0
    add([[10.5, 20.25, 50.75, 80.5, 0.9]], 2)                            # n = 1
    big = [10.0, 10.0, 60.0, 60.0]
    # hand-made: row 1 is discarded, pulls row 3 (identical to the maximum: discarded too), then pulls row 2 (disjoint)
    for m in (0, 1, 2):
        add([big + [0.9], big + [0.5], [200.0, 200.0, 240.0, 250.0, 0.4], big + [0.3]], m, Nt=0.3, threshold=0.35)
    # exact tie at the maximum, apart and overlapping
    add([[0, 0, 30, 30, 0.7], [100, 100, 140, 130, 0.8], [15, 15, 45, 45, 0.8], [102, 98, 139, 133, 0.8]], 2)
    add([[5.5, 5.5, 40.25, 40.75, 0.6]] * 4 + [[300, 300, 320, 330, 0.6]], 1, Nt=0.3, threshold=0.01)
    # disjoint boxes only
    add([[i * 50.0, 0.0, i * 50.0 + 20.0, 20.0, 0.1 * (i + 1)] for i in range(6)], 0)
    for m in (0, 1, 2):
        for kind in range(9):
            n = int(rng.integers(2, 120))
            clustered = kind % 3 != 2
            centres = rng.uniform(40, 460, (3 if clustered else n, 2))
            low = kind % 2 == 1                                            # scores near the threshold: N shrinks
            scores = np.exp(rng.uniform(np.log(2e-3), np.log(0.05), n)) if low else rng.uniform(0.01, 1.0, n)
            b = boxes_around(rng, centres, n, rng.uniform(20, 120), 4.0 if clustered else 30.0, scores)
            if kind == 4:                                                  # duplicates of the top rows (5 scales agree)
                b = np.concatenate([b, b[: n // 2]], 0)
            add(b, m, threshold=0.001 if not low else float(rng.choice([0.001, 0.004, 0.01])),
                Nt=float(rng.choice([0.3, 0.5])))
    # 5 scales x 100 detections of one crowded image, merge_outputs' own settings
    centres = rng.uniform(60, 440, (6, 2))
    parts = [boxes_around(rng, centres, 100, 70.0, 5.0, np.sort(np.exp(rng.uniform(np.log(1e-3), 0, 100)))[::-1])
             for _ in range(5)]
    add(np.concatenate(parts, 0), 2)
    return cases


def main():
    refnms, tmp = build_reference(sys.argv[1])
    try:
        cases = make_cases()
        ins, outs, meta, tags_all = [], [], [], 0
        for b, method, sigma, Nt, threshold in cases:
            out = b.copy()
            keep = refnms.soft_nms(out, sigma=sigma, Nt=Nt, threshold=threshold, method=method)
            tb, tn, tags = trace(b, sigma, Nt, threshold, method)
            assert tn == len(keep) and tb.tobytes() == out.tobytes(), "the Python trace disagrees with the compiled reference"
            ins.append(b)
            outs.append(out)
            meta.append((b.shape[0], len(keep), method, sigma, Nt, threshold, tags))
            tags_all |= tags
        assert tags_all == sum(TAGS.values()), "a required situation is missing: %d" % tags_all
        m = np.array(meta, dtype=np.float64)
        np.savez_compressed(os.path.join(HERE, "soft_nms_ref.npz"), inputs=np.concatenate(ins, 0),
                            outputs=np.concatenate(outs, 0), n=m[:, 0].astype(np.int64), n_keep=m[:, 1].astype(np.int64),
                            method=m[:, 2].astype(np.int64), sigma=m[:, 3].astype(np.float32),
                            Nt=m[:, 4].astype(np.float32), threshold=m[:, 5].astype(np.float32),
                            tags=m[:, 6].astype(np.uint16), tag_bits=np.array(list(TAGS.values()), dtype=np.uint16),
                            tag_names=np.array(list(TAGS.keys())))
        print("%d cases, %d rows, tags %s" % (len(cases), sum(x.shape[0] for x in ins), [int(t[6]) for t in meta]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
