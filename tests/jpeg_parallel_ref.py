"""Python restatement of the parallel entropy path of DESIGN.md section 7.4d on top of tests/jpeg_ref.py's Huffman decode:
states (p, b, z), the dry pass, the counted synchronisation rounds, the exclusive prefix sum of completed blocks, the
guarded write pass and the DC scan.  It shares nothing with codenet_amd/csrc/cdn_jpeg.h.

    serial_blocks(data)              -> [(coefficients [count * nblk, 64] in natural order, DC predicted), status] per segment
    parallel_blocks(data, S, W=256)  -> the same through tiles of W sub-sequences of S bits
"""
import numpy as np

from tests import jpeg_ref as R

DEAD_OVERREAD, DEAD_BAD_CODE = 1, 2


class _BitList:
    """take(k) as jpeg_ref._Bits has it (zeros beyond the end), over a list of bits and from any position."""

    def __init__(self, bits, pos):
        self.bits, self.pos = bits, pos

    def take(self, k):
        r = 0
        for _ in range(k):
            r = (r << 1) | (self.bits[self.pos] if self.pos < len(self.bits) else 0)
            self.pos += 1
        return r


def _layout(hd):
    """-> (component of each block of an MCU, MCUs in all, {component: (dc table, ac table)})."""
    comps = hd["comps"]
    if len(comps) == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcus = -(-hd["w"] // (8 * hmax)) * -(-hd["h"] // (8 * vmax))
    order = [c for c, (_, hs, vs, _) in enumerate(comps) for _ in range(hs * vs)]
    codes = {k: R._codes(*v) for k, v in hd["huff"].items()}
    tables = {c: (codes[(0, hd["scan"][c][0])], codes[(1, hd["scan"][c][1])]) for c in range(len(comps))}
    return order, mcus, tables


def _segment_list(data):
    hd = R.parse(data)
    order, mcus, tables = _layout(hd)
    per = hd["restart"] or mcus
    out = []
    for s, seg in enumerate(R._segments(hd["entropy"])):
        count = max(0, min((s + 1) * per, mcus) - s * per)
        out.append((list(np.unpackbits(np.frombuffer(seg, dtype=np.uint8)).tolist()), count))
    return order, tables, out


def subseq(bits, order, tables, entry, end, store=None, blk=0):
    """The symbols that start in [p of entry, end) -> (exit state, blocks completed).  A state is (p, b, z) or
    ('dead', why).  store = (coef, dc, limit): coefficients and DC differences of blocks below the limit are written."""
    if entry[0] == "dead" or entry[0] >= end:
        return entry, 0
    p, b, z = entry
    total, done = len(bits), 0
    while p < end:
        if store is not None and blk >= store[2]:
            break
        br = _BitList(bits, p)
        table = tables[order[b]][0 if z == 0 else 1]
        try:
            sym = R._symbol(br, table, {})
        except ValueError:
            return ("dead", DEAD_OVERREAD if p + 16 > total else DEAD_BAD_CODE), done
        t = sym & 15
        v = R._extend(br.take(t), t) if t else 0
        if br.pos > total:
            return ("dead", DEAD_OVERREAD), done
        p = br.pos
        if z == 0:
            if store is not None:
                store[1][blk] = v
            z = 1
        elif t:
            z += sym >> 4
            if store is not None and z < 64:
                store[0][blk, R.ZIGZAG[z]] = v
            z += 1
        elif sym >> 4 == 15:
            z += 16
        else:
            z = 64
        if z >= 64:
            done, blk, b, z = done + 1, blk + 1, (b + 1) % len(order), 0
    return (p, b, z), done


def _dc_scan(coef, dc, order, limit):
    pred = {}
    for i in range(limit):
        c = order[i % len(order)]
        pred[c] = (pred.get(c, 0) + int(dc[i]) + 2 ** 31) % 2 ** 32 - 2 ** 31          # uint32 wrap-around
        coef[i, 0] = pred[c]


def serial_blocks(data):
    order, tables, segs = _segment_list(data)
    out = []
    for bits, count in segs:
        limit = count * len(order)
        coef, dc = np.zeros((limit, 64), dtype=np.int64), np.zeros(limit, dtype=np.int64)
        state, done = subseq(bits, order, tables, (0, 0, 0), len(bits) + 64, (coef, dc, limit), 0)
        _dc_scan(coef, dc, order, limit)
        out.append((coef, 0 if done >= limit else (state[1] if state[0] == "dead" else DEAD_OVERREAD)))
    return out


def parallel_blocks(data, S, W=256, rounds_seen=None):
    order, tables, segs = _segment_list(data)
    out = []
    for bits, count in segs:
        limit = count * len(order)
        coef, dc = np.zeros((limit, 64), dtype=np.int64), np.zeros(limit, dtype=np.int64)
        nsub = -(-len(bits) // S)
        carry, carry_blk = (0, 0, 0), 0
        for sub0 in range(0, nsub, W):
            na = min(W, nsub - sub0)                    # sub-sequences of this tile: the lanes that take part
            ends = [(sub0 + j + 1) * S for j in range(na)]
            entry = [carry] + [((sub0 + j) * S, 0, 0) for j in range(1, na)]
            res = [subseq(bits, order, tables, entry[j], ends[j]) for j in range(na)]           # dry pass
            exits, cnt = [r[0] for r in res], [r[1] for r in res]
            for r in range(1, na):                                                              # counted rounds
                prev, changed = list(exits), False
                for j in range(1, na):
                    if prev[j - 1] != entry[j]:
                        entry[j] = prev[j - 1]
                        x, cnt[j] = subseq(bits, order, tables, entry[j], ends[j])
                        changed |= x != exits[j]
                        exits[j] = x
                if rounds_seen is not None:
                    rounds_seen.append(r)
                if not changed:
                    break
            first = [carry_blk + sum(cnt[:j]) for j in range(na)]                               # exclusive prefix sum
            for j in range(na):                                                                 # write pass
                subseq(bits, order, tables, entry[j], ends[j], (coef, dc, limit), first[j])
            carry, carry_blk = exits[na - 1], carry_blk + sum(cnt)
        _dc_scan(coef, dc, order, limit)
        out.append((coef, 0 if carry_blk >= limit else (carry[1] if carry[0] == "dead" else DEAD_OVERREAD)))
    return out
