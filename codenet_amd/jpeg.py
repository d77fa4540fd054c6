"""Baseline JPEG decoding on the GPU (codenet_jpeg.hip, cdn_jpeg.h): file bytes -> interleaved uint8 pixels in front of
preproc.PreProcess, so that test.py / main.py start at the .jpg file and not at a host cv2.imread.

The result equals libjpeg-turbo's default decode bit for bit (ISLOW IDCT, fancy up-sampling, 16-bit fixed-point
YCbCr -> RGB): what cv2.imread and PIL produce.  The arithmetic is DESIGN.md section 7.4d; tests/jpeg_ref.py restates it in
numpy.  EXIF orientation is IGNORED, as PIL's Image.open does; cv2.imread applies it -- rotate such files on the host.

Supported: SOF0 (baseline), 8-bit samples and quantisation tables, one interleaved scan, grey or three components with
4:4:4, 4:2:2 (Y 2x1) or 4:2:0 (Y 2x2) sampling, restart intervals.  Everything else -- progressive, arithmetic coding,
12-bit, 16-bit tables, four components / CMYK, 4:4:0, 4:1:1, several scans, DNL -- raises NotImplementedError on the host
before anything is copied, so a caller can fall back to a decoder of its own.

The host parses the header and, in one pass, removes the byte stuffing and cuts the entropy-coded bytes at the restart
markers into segments; the GPU does the rest.  Two entropy paths write the same pixels:

entropy="serial" (the default, two launches): a segment is a dependent chain that ONE lane decodes, so the entropy
kernel's concurrency is batch size x restart intervals.  Files without restart markers (Pascal VOC) give one segment per
image, and the batch is the only parallelism of that kernel.

entropy="parallel" (three launches): a segment is decoded by the 256 lanes of a workgroup.  Without its stuffing a segment
is a plain bit string; it is cut into sub-sequences of subseq_bits bits, every lane decodes one from a guessed state, and
counted rounds hand the exact state from lane to lane until nothing changes (255 rounds always suffice; Huffman streams
self-synchronise, so far fewer can -- but the block position within the MCU does not).  It needs a
coefficient workspace of 2.0625 x the plane bytes (6.19 MiB per item at the 1024 x 1024 default, 1.16 MiB at 375 x 500).
DESIGN.md section 7.4d has the algorithm and the measurements.
"""
import collections

import numpy as np
import torch

from . import _native as N_
from . import preproc

ITEM, SEG, TABLE_BYTES = 16, 8, 6144
SAMPLING = {(1, 0): "grey", (3, 0): "4:4:4", (3, 1): "4:2:2", (3, 2): "4:2:0"}
STATUS = {1: "bits consumed beyond the end of a segment", 2: "a code with no entry in its Huffman table",
          3: "a record outside the decoder's capacities"}

JpegInfo = collections.namedtuple("JpegInfo", "h w components sampling restart_interval segments")


def _as_bytes(data):
    """bytes / bytearray / memoryview / uint8 array -> a contiguous uint8 numpy array (no copy where possible)."""
    if isinstance(data, np.ndarray):
        if data.dtype != np.uint8:
            raise ValueError("JPEG data must be bytes or a uint8 array")
        return np.ascontiguousarray(data).reshape(-1)
    if isinstance(data, torch.Tensor):
        return _as_bytes(data.cpu().numpy())
    return np.frombuffer(data, dtype=np.uint8)


def _raise(rc, what):
    """cdn_status of the two host functions -> NotImplementedError (outside the supported set) or ValueError."""
    msg = "%s: %s" % (what, N_.last_error())
    if rc == N_.CDN_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise ValueError(msg)


def parse(data):
    """The header of one JPEG stream -> JpegInfo(h, w, components, sampling, restart_interval, segments).  ValueError for
    malformed data, NotImplementedError for a stream outside the supported set."""
    d = _as_bytes(data)
    info = np.zeros(16, dtype=np.int32)
    rc = N_.lib().cdn_jpeg_parse(d.ctypes.data, d.size, info.ctypes.data)
    if rc != 0:
        _raise(rc, "cdn_jpeg_parse")
    return JpegInfo(int(info[1]), int(info[0]), int(info[2]), SAMPLING[(int(info[2]), int(info[3]))], int(info[6]),
                    int(info[7]))


def default_layout(infos):
    """The default packing of the decoded images: [(offset, h, w, pitch = 3 w)] back to back, and the bytes in all."""
    layout, off = [], 0
    for i in infos:
        layout.append((off, i.h, i.w, 3 * i.w))
        off += i.h * i.w * 3
    return layout, off


def _aligned(nbytes, align=64):
    raw = np.zeros(nbytes + align, dtype=np.uint8)
    o = (-raw.ctypes.data) % align
    return raw[o:o + nbytes]


def _pack(datas, layout, stream, segs, items, tables, plane_stride):
    """cdn_jpeg_pack for every stream into the host buffers given (numpy views) -> (stream bytes, segments) used."""
    lib = N_.lib()
    used = np.zeros(2, dtype=np.int64)
    seg_cap = segs.size // SEG - 1
    for k, (d, (off, _, _, pitch)) in enumerate(zip(datas, layout)):
        rc = lib.cdn_jpeg_pack(d.ctypes.data, d.size, k, off, pitch, stream.ctypes.data, int(used[0]), stream.size,
                               segs.ctypes.data, int(used[1]), seg_cap, items.ctypes.data + k * ITEM * 4,
                               tables.ctypes.data + k * TABLE_BYTES, plane_stride, used.ctypes.data)
        if rc != 0:
            _raise(rc, "cdn_jpeg_pack (item %d)" % k)
    return int(used[0]), int(used[1])


ENTROPY = ("serial", "parallel")


def _check_entropy(entropy, subseq_bits):
    if entropy not in ENTROPY:
        raise ValueError("entropy must be 'serial' or 'parallel'")
    if entropy == "parallel" and not (64 <= int(subseq_bits) <= 8192 and int(subseq_bits) % 32 == 0):
        raise ValueError("subseq_bits must be a multiple of 32 in 64..8192")


def decode_host_raw(datas, order="bgr", guard=0, entropy="serial", subseq_bits=1024):
    """The whole decode on the calling thread through cdn_jpeg_decode_host (or, with entropy='parallel',
    cdn_jpeg_decode_parallel_host) -- the text the kernels run -- without a GPU.
    -> dict(infos, layout, out, planes, status, out_buf, planes_buf): out / planes are the views the library was given,
    *_buf the allocations around them with `guard` bytes of 0xA5 on either side; the parallel path adds work / work_buf,
    its coefficient workspace."""
    if order not in ("bgr", "rgb"):
        raise ValueError("order must be 'bgr' or 'rgb'")
    _check_entropy(entropy, subseq_bits)
    datas = [_as_bytes(d) for d in datas]
    infos = [parse(d) for d in datas]
    layout, total = default_layout(infos)
    lib = N_.lib()
    stride = max(int(lib.cdn_jpeg_workspace_bytes(1, i.h, i.w)) for i in infos)
    n, nseg = len(datas), sum(i.segments for i in infos)
    stream = _aligned(max(1, sum(d.size for d in datas)))
    segs = _aligned((1 + nseg) * SEG * 4).view(np.int32)
    items = _aligned(n * ITEM * 4).view(np.int32)
    tables = _aligned(n * TABLE_BYTES)
    _pack(datas, layout, stream, segs, items, tables, stride)
    guard = (int(guard) + 63) // 64 * 64
    out_buf, planes_buf = _aligned(total + 2 * guard), _aligned(n * stride + 2 * guard)
    out_buf[:], planes_buf[:] = 0xA5, 0xA5
    out, planes = out_buf[guard:guard + total], planes_buf[guard:guard + n * stride]
    status = np.zeros(n, dtype=np.int32)
    r = {"infos": infos, "layout": layout, "out": out, "planes": planes, "status": status, "out_buf": out_buf,
         "planes_buf": planes_buf, "guard": guard}
    args = [stream.ctypes.data, stream.size, segs.ctypes.data, nseg, items.ctypes.data, n, tables.ctypes.data,
            planes.ctypes.data, stride, status.ctypes.data, out.ctypes.data, total, int(order == "rgb")]
    if entropy == "parallel":
        nwork = n * max(int(lib.cdn_jpeg_parallel_workspace_bytes(1, i.h, i.w)) for i in infos)       # (of the largest planes)
        r["work_buf"] = _aligned(nwork + 2 * guard)
        r["work_buf"][:] = 0xA5
        r["work"] = r["work_buf"][guard:guard + nwork]
        rc = lib.cdn_jpeg_decode_parallel_host(*(args + [r["work"].ctypes.data, nwork, int(subseq_bits)]))
        N_.check(rc, "cdn_jpeg_decode_parallel_host")
    else:
        N_.check(lib.cdn_jpeg_decode_host(*args), "cdn_jpeg_decode_host")
    return r


def _raise_status(status):
    bad = [(k, int(s)) for k, s in enumerate(status) if s != 0]
    if bad:
        raise RuntimeError("JPEG decode failed: " + "; ".join("item %d: %s" % (k, STATUS.get(s, "status %d" % s))
                                                              for k, s in bad))


def decode_host(datas, order="bgr", entropy="serial", subseq_bits=1024):
    """[JPEG streams] -> [uint8 h x w x 3 numpy arrays], decoded on the host by the library (no GPU needed); entropy and
    subseq_bits as JpegDecoder takes them.  RuntimeError when an item's entropy-coded data is corrupt."""
    r = decode_host_raw(datas, order, entropy=entropy, subseq_bits=subseq_bits)
    _raise_status(r["status"])
    return [r["out"][off:off + h * w * 3].reshape(h, w, 3).copy() for off, h, w, _ in r["layout"]]


class JpegDecoder:
    """Owns the pinned staging, the device stream / segment / table buffers, the component planes and the status words
    for batches of up to max_items images of up to max_h x max_w.  load(datas) -> run(out_bytes); run is two launches and
    capturable, and because every per-batch value lives in device memory a captured run replays for any batch inside
    the capacities.  entropy='parallel' decodes a segment on the 256 lanes of a workgroup in sub-sequences of subseq_bits
    bits (a multiple of 32 in 64..8192): three launches, the same pixels, and a coefficient workspace of 2.0625 x the
    plane bytes beside the planes."""

    decode_host = staticmethod(decode_host)

    def __init__(self, max_items=1, max_h=1024, max_w=1024, max_stream_bytes=None, max_segments=None, device="cuda",
                 order="bgr", entropy="serial", subseq_bits=1024):
        if order not in ("bgr", "rgb"):
            raise ValueError("order must be 'bgr' or 'rgb'")
        _check_entropy(entropy, subseq_bits)
        self.entropy, self.subseq_bits = entropy, int(subseq_bits)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("JpegDecoder needs a GPU device (decode_host() runs without one)")
        self.max_items, self.max_h, self.max_w = int(max_items), int(max_h), int(max_w)
        self.plane_stride = int(N_.lib().cdn_jpeg_workspace_bytes(1, self.max_h, self.max_w))
        if self.max_items < 1 or self.max_items > 65535 or self.plane_stride == 0:
            raise ValueError("JpegDecoder capacities: 1..65535 items of 1..65535 x 1..65535 pixels")
        # defaults: one byte of entropy-coded data per pixel, one restart interval per row of 8 x 8 blocks
        self.max_stream_bytes = int(max_stream_bytes or self.max_items * self.max_h * self.max_w)
        self.max_segments = int(max_segments or self.max_items * ((self.max_h + 7) // 8))
        if not 0 < self.max_stream_bytes < 2 ** 31 or not 0 < self.max_segments < 2 ** 27:
            raise ValueError("JpegDecoder capacities: stream bytes below 2^31, segments below 2^27")
        self.rgb = order == "rgb"
        sizes = {"stream": (self.max_stream_bytes, torch.uint8), "segs": ((1 + self.max_segments) * SEG, torch.int32),
                 "items": (self.max_items * ITEM, torch.int32), "tables": (self.max_items * TABLE_BYTES, torch.uint8)}
        self._host = {k: torch.zeros(n, dtype=t).pin_memory() for k, (n, t) in sizes.items()}
        self._host_np = {k: v.numpy() for k, v in self._host.items()}
        self._dev = {k: torch.zeros(n, dtype=t, device=self.device) for k, (n, t) in sizes.items()}
        self.planes = torch.zeros(self.max_items * self.plane_stride, dtype=torch.uint8, device=self.device)
        self._status = torch.zeros(self.max_items, dtype=torch.int32, device=self.device)
        self.work = None
        if entropy == "parallel":
            nwork = int(N_.lib().cdn_jpeg_parallel_workspace_bytes(self.max_items, self.max_h, self.max_w))
            self.work = torch.zeros(nwork, dtype=torch.uint8, device=self.device)
        self.P, self.infos, self.layout, self.out_bytes = 0, [], [], 0
        self._copied = None

    def load(self, datas, out_capacity=None):
        """datas: the bytes of up to max_items JPEG files.  Parses and packs them on the host into the pinned buffers and
        issues the asynchronous copies on the current stream; -> [JpegInfo].  ValueError (malformed data, a batch beyond a
        capacity or beyond out_capacity bytes of output) and NotImplementedError (a stream outside the supported set) are
        raised before any copy: the batch loaded before stays loaded."""
        datas = [_as_bytes(d) for d in datas]
        if not 0 < len(datas) <= self.max_items:
            raise ValueError("%d streams for a decoder of %d items" % (len(datas), self.max_items))
        infos = [parse(d) for d in datas]
        layout, total = default_layout(infos)
        if out_capacity is not None and total > out_capacity:
            raise ValueError("the decoded batch has %d bytes: beyond the %d of the output buffer" % (total, out_capacity))
        with torch.cuda.device(self.device):
            if self._copied is not None:
                self._copied.synchronize()      # the previous batch may still be on its way out of the pinned buffers
            h = self._host_np
            nbytes, nseg = _pack(datas, layout, h["stream"], h["segs"], h["items"], h["tables"], self.plane_stride)
            used = {"stream": max(nbytes, 1), "segs": (1 + nseg) * SEG, "items": len(datas) * ITEM,
                    "tables": len(datas) * TABLE_BYTES}
            for k, n in used.items():
                self._dev[k][:n].copy_(self._host[k][:n], non_blocking=True)
            self._status.zero_()
            self._copied = torch.cuda.Event()
            self._copied.record(torch.cuda.current_stream(self.device))
        self.P, self.infos, self.layout, self.out_bytes = len(datas), infos, layout, total
        return infos

    def run(self, out_bytes):
        """The two launches (three with entropy='parallel') on the current stream: item k's pixels go to out_bytes[offset_k + y pitch_k + 3 x] (layout),
        B G R (or R G B with order='rgb').  out_bytes: a contiguous uint8 GPU tensor of at least self.out_bytes bytes; a
        captured run checks every later batch against its size on the device (status 3)."""
        if not isinstance(out_bytes, torch.Tensor) or not out_bytes.is_cuda:
            raise NotImplementedError("JpegDecoder.run needs a GPU tensor")
        if self.P == 0:
            raise ValueError("JpegDecoder.run before load()")
        if out_bytes.dtype != torch.uint8 or not out_bytes.is_contiguous() or out_bytes.device != self.planes.device \
                or out_bytes.numel() < self.out_bytes:
            raise ValueError("out_bytes must be a contiguous uint8 tensor of at least %d bytes on %s"
                             % (self.out_bytes, self.planes.device))
        d = self._dev
        args = [d["stream"].data_ptr(), self.max_stream_bytes, d["segs"].data_ptr(), self.max_segments,
                d["items"].data_ptr(), self.max_items, d["tables"].data_ptr(), self.planes.data_ptr(), self.plane_stride,
                self._status.data_ptr(), out_bytes.data_ptr(), out_bytes.numel(), int(self.rgb)]
        stream = torch.cuda.current_stream(self.planes.device).cuda_stream
        if self.work is not None:
            rc = N_.lib().cdn_jpeg_decode_parallel(*(args + [self.work.data_ptr(), self.work.numel(), self.subseq_bits,
                                                             stream]))
            N_.check(rc, "cdn_jpeg_decode_parallel")
        else:
            N_.check(N_.lib().cdn_jpeg_decode(*(args + [stream])), "cdn_jpeg_decode")
        return out_bytes

    @property
    def status(self):
        """int32 per loaded item (device): 0, or why its pixels are not to be trusted (STATUS)."""
        return self._status[:self.P]

    def check(self):
        """Waits for the work on the current stream and raises RuntimeError when an item's status is not zero."""
        torch.cuda.current_stream(self.planes.device).synchronize()
        _raise_status(self.status.cpu().numpy())

    def images(self, out_bytes):
        """Views of the decoded items in out_bytes: [uint8 h x w x 3] (default layout: rows are contiguous)."""
        return [out_bytes[off:off + h * w * 3].view(h, w, 3) for off, h, w, _ in self.layout]


class JpegPreProcess:
    """JPEG files -> network input planes: decoder.run(pre.arena) followed by pre.run(images).  It has the run() that
    harness.capture_process / capture_process_scales call on their pre= argument, so file bytes -> detections is one graph:
    a replay needs load(next file) only."""

    def __init__(self, decoder, pre):
        if decoder.rgb:
            raise ValueError("PreProcess reads B G R, as cv2.imread gives it: the decoder must have order='bgr'")
        if decoder.planes.device != pre.arena.device:
            raise ValueError("decoder and pre-processing live on different devices")
        self.decoder, self.pre = decoder, pre

    def load(self, data, table=None, aug=None):
        """One stream (test mode): the S items of pre's test scales for the decoded size, as PreProcess.load -> the S meta
        dicts.  A list of streams (training mode): table(layout) -> the [n][16] item rows for the decoded images, whose
        (offset, h, w, pitch) are `layout`, or the rows themselves; committed as PreProcess.load_items does -> the rows.
        Nothing is copied when a stream or a row is refused."""
        pre, dec = self.pre, self.decoder
        if not isinstance(data, (list, tuple)):
            info = parse(data)
            rows, metas = [], []
            for sc in pre.scales:
                new_h, new_w, M, meta = preproc.crop_matrix(info.h, info.w, pre.in_h, pre.in_w, sc)
                rows.append(preproc.item_row(0, info.h, info.w, 3 * info.w, M, new_h, new_w))
                metas.append(meta)
            nbytes = info.h * info.w * 3
            pre.check_table(nbytes, rows, None)
            dec.load([data], out_capacity=pre.capacity)
            pre.load_table(nbytes, rows)
            return metas
        layout, nbytes = default_layout([parse(d) for d in data])
        rows = table(layout) if callable(table) else table
        if rows is None:
            raise ValueError("a list of streams needs table=: the item rows, or a function of the layout that builds them")
        pre.check_table(nbytes, rows, aug)
        dec.load(data, out_capacity=pre.capacity)
        pre.load_table(nbytes, rows, aug)
        return rows

    def run(self, images):
        self.decoder.run(self.pre.arena)
        return self.pre.run(images)
