"""numpy restatement of DESIGN.md section 7.4d: baseline JPEG -> uint8 [h, w, 3] with the bits of libjpeg-turbo's default
decode (ISLOW IDCT, fancy up-sampling, 16-bit fixed-point colour).  Written from the specification, not from the library's
code: it shares nothing with codenet_amd/csrc/cdn_jpeg.h.  decode(data, order='bgr')."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7,
                   14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39,
                   46, 53, 60, 61, 54, 47, 55, 62, 63])


def parse(data):
    """-> dict(w, h, comps [(id, hs, vs, tq)], quant {id: natural-order int array}, huff {(cls, id): (counts, values)},
    restart, scan [(td, ta)], entropy bytes)."""
    d = bytes(data)
    assert d[:2] == b"\xff\xd8"
    pos, out = 2, {"quant": {}, "huff": {}, "restart": 0}
    while True:
        assert d[pos] == 0xFF
        while d[pos] == 0xFF:
            pos += 1
        m = d[pos]
        pos += 1
        n = (d[pos] << 8) | d[pos + 1]
        body = d[pos + 2:pos + n]
        pos += n
        if m == 0xC0:
            assert body[0] == 8
            out["h"], out["w"] = (body[1] << 8) | body[2], (body[3] << 8) | body[4]
            out["comps"] = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c])
                            for c in range(body[5])]
        elif m == 0xDB:
            o = 0
            while o < len(body):
                assert body[o] >> 4 == 0
                q = np.zeros(64, dtype=np.int64)
                q[ZIGZAG] = np.frombuffer(body[o + 1:o + 65], dtype=np.uint8)
                out["quant"][body[o] & 15] = q
                o += 65
        elif m == 0xC4:
            o = 0
            while o < len(body):
                counts = list(body[o + 1:o + 17])
                out["huff"][(body[o] >> 4, body[o] & 15)] = (counts, list(body[o + 17:o + 17 + sum(counts)]))
                o += 17 + sum(counts)
        elif m == 0xDD:
            out["restart"] = (body[0] << 8) | body[1]
        elif m == 0xDA:
            ns = body[0]
            out["scan"] = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(ns)]
            out["entropy"] = d[pos:]
            return out
        else:
            assert m not in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF), "not baseline"


def _codes(counts, values):
    """{(length, code): symbol} of a canonical Huffman table."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = values[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _segments(entropy):
    """The entropy-coded bytes without stuffing, cut at RSTn, ended by EOI or the end of the data."""
    segs, cur, i, n = [], bytearray(), 0, len(entropy)
    while i < n:
        b = entropy[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        j = i + 1
        while j < n and entropy[j] == 0xFF:
            j += 1
        if j >= n:
            break
        m = entropy[j]
        i = j + 1
        if m == 0:
            cur.append(0xFF)
        elif 0xD0 <= m <= 0xD7:
            segs.append(bytes(cur))
            cur = bytearray()
        else:
            break
    segs.append(bytes(cur))
    return segs


class _Bits:
    def __init__(self, data):
        self.v = int.from_bytes(data, "big") if data else 0
        self.n = 8 * len(data)
        self.pos = 0
        self.stats = None

    def take(self, k):
        """The next k bits, zeros beyond the end."""
        end = self.pos + k
        if end <= self.n:
            r = (self.v >> (self.n - end)) & ((1 << k) - 1)
        else:
            have = max(self.n - self.pos, 0)
            r = ((self.v & ((1 << have) - 1)) << (k - have)) if have else 0
        self.pos = end
        return r


def _symbol(bits, table, stats):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | bits.take(1)
        if (length, code) in table:
            if length == 16:
                stats["code16"] = stats.get("code16", 0) + 1
            return table[(length, code)]
    raise ValueError("no Huffman code in 16 bits")


def _extend(v, t):
    return v if v >= (1 << (t - 1)) else v - (1 << t) + 1


def idct(blocks):
    """[..., 8, 8] dequantised coefficients (natural order) -> [..., 8, 8] samples 0..255: jidctint.c with CONST_BITS 13,
    PASS1_BITS 2."""
    def one_d(x, shift):        # along the LAST axis but one -> rows of 8 inputs in x[..., k, :]
        i = [x[..., k, :] for k in range(8)]
        z1 = (i[2] + i[6]) * 4433
        e2, e3 = z1 - i[6] * 15137, z1 + i[2] * 6270
        e0, e1 = (i[0] + i[4]) * 8192, (i[0] - i[4]) * 8192
        t10, t13, t11, t12 = e0 + e3, e0 - e3, e1 + e2, e1 - e2
        t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * 9633
        t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
        z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, z5 - z3 * 16069, z5 - z4 * 3196
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        half = 1 << (shift - 1)
        outs = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
        return np.stack([(o + half) >> shift for o in outs], axis=-2)
    x = np.asarray(blocks, dtype=np.int64)
    ws = one_d(x, 11)                                        # pass 1: columns (inputs are the 8 rows of a column)
    y = one_d(np.swapaxes(ws, -1, -2), 18)                   # pass 2: rows
    return np.clip(np.swapaxes(y, -1, -2) + 128, 0, 255)


def upsample_h2v1(p):
    """[r, n] -> [r, 2n]."""
    p = p.astype(np.int64)
    n = p.shape[1]
    out = np.zeros((p.shape[0], 2 * n), dtype=np.int64)
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, 2 * n - 1] = p[:, 0], p[:, n - 1]
    return out


def upsample_h2v2(p):
    """[r, n] -> [2r, 2n]."""
    p = p.astype(np.int64)
    r, n = p.shape
    out = np.zeros((2 * r, 2 * n), dtype=np.int64)
    up, down = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    for v, nb in ((0, up), (1, down)):
        s = 3 * p + nb
        left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        even, odd = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
        even[:, 0], odd[:, n - 1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, n - 1] + 7) >> 4
        out[v::2, 0::2], out[v::2, 1::2] = even, odd
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def color(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    return [np.clip(v, 0, 255) for v in (r, g, b)]


def decode(data, order="bgr", stats=None):
    """-> uint8 [h, w, 3].  stats (a dict) counts ZRL symbols, 16-bit codes and samples the final clamp changed."""
    stats = {} if stats is None else stats
    hd = parse(data)
    w, h, comps = hd["w"], hd["h"], hd["comps"]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if len(comps) == 1:
        comps, hmax, vmax = [(comps[0][0], 1, 1, comps[0][3])], 1, 1
    mcus_x, mcus_y = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    coef = [np.zeros((mcus_y * c[2], mcus_x * c[1], 64), dtype=np.int64) for c in comps]
    tables = {k: _codes(*v) for k, v in hd["huff"].items()}
    total, ri = mcus_x * mcus_y, hd["restart"]
    per = ri if ri else total
    for s, seg in enumerate(_segments(hd["entropy"])):
        bits, pred = _Bits(seg), [0] * len(comps)
        for mi in range(s * per, min((s + 1) * per, total)):
            my, mx = divmod(mi, mcus_x)
            for c, (_, hs, vs, tq) in enumerate(comps):
                dc, ac = tables[(0, hd["scan"][c][0])], tables[(1, hd["scan"][c][1])]
                for by in range(vs):
                    for bx in range(hs):
                        blk = coef[c][my * vs + by, mx * hs + bx]
                        t = _symbol(bits, dc, stats)
                        pred[c] += _extend(bits.take(t), t) if t else 0
                        blk[0] = pred[c]
                        k = 1
                        while k < 64:
                            rs = _symbol(bits, ac, stats)
                            r, t = rs >> 4, rs & 15
                            if t:
                                k += r
                                blk[ZIGZAG[k]] = _extend(bits.take(t), t)
                                k += 1
                            elif r == 15:
                                stats["zrl"] = stats.get("zrl", 0) + 1
                                k += 16
                            else:
                                break
    planes = []
    for c, (_, hs, vs, tq) in enumerate(comps):
        blocks = (coef[c] * hd["quant"][tq]).reshape(coef[c].shape[0], coef[c].shape[1], 8, 8)
        pix = idct(blocks)
        plane = pix.transpose(0, 2, 1, 3).reshape(blocks.shape[0] * 8, blocks.shape[1] * 8)
        planes.append(plane[:-(-h * vs // vmax), :-(-w * hs // hmax)])          # the component's TRUE size
    if len(planes) == 1:
        return np.repeat(planes[0][:, :, None], 3, axis=2).astype(np.uint8)
    up = {(1, 1): lambda p: p, (2, 1): upsample_h2v1, (2, 2): upsample_h2v2}[(hmax, vmax)]
    y, cb, cr = planes[0], up(planes[1])[:h, :w], up(planes[2])[:h, :w]
    yy, cbb, crr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    raw = [yy + ((_fix(1.402) * crr + 32768) >> 16), yy + ((-_fix(0.34414) * cbb + 32768 - _fix(0.71414) * crr) >> 16),
           yy + ((_fix(1.772) * cbb + 32768) >> 16)]
    stats["clamped"] = stats.get("clamped", 0) + int(sum(((v < 0) | (v > 255)).sum() for v in raw))
    rgb = color(y, cb, cr)
    return np.stack(rgb if order == "rgb" else rgb[::-1], axis=2).astype(np.uint8)
