"""Image pre-processing on the GPU (codenet_preproc.hip, cdn_ctdet_pre_process): what CtdetDetector.pre_process does for
every test scale of an image (lib/detectors/base_detector.py:47-77, fix_res: ctdet on pascal) and what the training
sample does to its input (lib/datasets/sample/ctdet.py:84-97) -- resize, affine crop with a zero border, optional source
flip, (v / 255 - mean) / std, HWC uint8 -> float32 planes, the W-mirrors of --flip_test -- as ONE launch that reads the
image bytes and a per-item table from device memory.

The arithmetic is an integer specification of this project, in the form of cv2.resize +
cv2.warpAffine(INTER_LINEAR) on uint8; it is exact and tested bit for bit against a numpy restatement
(tests/preproc_ref.py).  It makes no claim about cv2's own bits.  Not here: keep_res.  The image bytes may come from the
GPU JPEG decoder (codenet_amd/jpeg.py: JpegPreProcess decodes into the arena and load_table() commits the rows).

PreProcess(..., color_aug=True) is the training mode with the reference's default colour augmentation
(sample/ctdet.py:76-79, lib/utils/image.py:196-234; cdn_ctdet_pre_process_aug): the crop's bytes and their exact integer
channel sums in one launch, then v / 255, brightness / contrast / saturation in the item's order, lighting and
(x - mean) / std in float32 in a second (restated in tests/color_aug_ref.py, bit for bit).  The
host draws the parameters of an item with color_aug_params(), which consumes the two random streams as the reference does.
"""
import random

import numpy as np
import torch

from . import _native as N_

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)        # pascal.py:15-18
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
ITEM = 16                                                       # doubles per item of the device table
EIG_VAL = np.array([0.2141788, 0.01817699, 0.00341571], dtype=np.float32)       # pascal.py:38-44
EIG_VEC = np.array([[-0.58752847, -0.69563484, 0.41340352], [-0.5832747, 0.00994535, -0.81221408],
                    [-0.56089297, 0.71832671, 0.41158938]], dtype=np.float32)
AUG = 13                                                        # values of an aug row; 16 4-byte words on the device
COORD_LIMIT = float(1 << 20)


def _closed_form(c, s, out_w, out_h):
    k = float(s) / out_w
    return [k, 0.0, float(c[0]) - (out_w / 2.0) * k, 0.0, k, float(c[1]) - (out_h / 2.0) * k]


def crop_matrix(h, w, in_h, in_w, scale=1.0):
    """The crop of one test scale, fix_res: -> (new_h, new_w, M, meta).  The image is resized to new_h x new_w =
    int(h * scale) x int(w * scale); c = float32 centre of the RESIZED image, s = max(h, w) of the unscaled one; M = six
    float64 that send output pixel (x, y) to (M0 x + M1 y + M2, M3 x + M4 y + M5) in the resized image: the inverse of
    get_affine_transform(c, s, 0, [in_w, in_h]) (lib/utils/image.py:30-55) in closed form (the reference solves
    cv2.getAffineTransform on float32 points and inverts numerically).  meta is what pre_process hands post_process."""
    new_h, new_w = int(h * scale), int(w * scale)
    c = np.array([new_w / 2.0, new_h / 2.0], dtype=np.float32)
    s = float(max(h, w))
    return new_h, new_w, _closed_form(c, s, in_w, in_h), {"c": c, "s": s, "out_height": in_h // 4, "out_width": in_w // 4}


def train_matrix(c, s, out_w, out_h):
    """The training sample's input crop (sample/ctdet.py:84-92): centre c (x, y), side s, onto out_w x out_h."""
    return _closed_form(c, s, out_w, out_h)


def check_matrix(M, out_h, out_w):
    """The kernel's fixed point is int32-safe while every output corner maps to |coordinate| < 2^20: ValueError beyond."""
    M = [float(m) for m in M]
    if len(M) != 6 or not all(np.isfinite(M)):
        raise ValueError("crop matrix needs six finite values, got %r" % (M,))
    for x in (0.0, out_w - 1.0):
        for y in (0.0, out_h - 1.0):
            px, py = M[0] * x + M[1] * y + M[2], M[3] * x + M[4] * y + M[5]
            if not (abs(px) < COORD_LIMIT and abs(py) < COORD_LIMIT):
                raise ValueError("crop matrix sends output corner (%d, %d) to (%g, %g): beyond 2^20" % (x, y, px, py))


def item_row(src_off, h, w, pitch, M, new_h=None, new_w=None, flip_src=False):
    """One row of the item table: {src_off, h, w, pitch, new_h, new_w, ratio_y, ratio_x, flip_src, M0..M5, 0}."""
    new_h, new_w = h if new_h is None else new_h, w if new_w is None else new_w
    return [float(src_off), float(h), float(w), float(pitch), float(new_h), float(new_w),
            float(np.float64(h) / np.float64(new_h)) if new_h else 0.0,
            float(np.float64(w) / np.float64(new_w)) if new_w else 0.0,
            1.0 if flip_src else 0.0] + [float(m) for m in M] + [0.0]


def lut(mean=MEAN, std=STD):
    """float32 [256, 3]: (v / 255.0 - mean) / std in float64 from the float32 mean and std -- the value numpy gives
    base_detector.py:67 for a uint8-valued pixel."""
    v = np.arange(256, dtype=np.float64)[:, None]
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    return ((v / 255.0 - mean.astype(np.float64)) / std.astype(np.float64)).astype(np.float32)


def aug_row(order=(0, 1, 2), alphas=(1.0, 1.0, 1.0), d=(0.0, 0.0, 0.0), on=True):
    """One aug row {on, order[3], a[3], om[3], d[3]}: `order` the sequence of the steps 0 brightness, 1 contrast,
    2 saturation; alphas[k] the float64 factor of step k (a = float32(alpha), om = float32(1 - alpha), the subtraction in
    float64); d the lighting term per channel position, rounded to float32 once."""
    alphas = [np.float64(v) for v in alphas]
    return ([1 if on else 0] + [int(k) for k in order] + [float(np.float32(v)) for v in alphas]
            + [float(np.float32(np.float64(1.0) - v)) for v in alphas] + [float(np.float32(np.float64(v))) for v in d])


AUG_OFF = aug_row(on=False)             # the validation split / --no_color_aug: ((float32(v) / 255) - mean) / std
AUG_IDENTITY = aug_row()                # alphas 1, d 0: the same bits as an off item


def color_aug_params(data_rng, eig_val=EIG_VAL, eig_vec=EIG_VEC, var=0.4, alphastd=0.1, shuffle=random.shuffle):
    """The draws of one color_aug call (lib/utils/image.py:226-234) -> aug row.  Consumes `shuffle` (the `random`
    module's stream) and data_rng (a numpy RandomState) exactly as the reference does: the shuffle of a 3-list, one
    uniform(-var, var) per step in shuffled order, normal(scale=alphastd, size=(3,))."""
    order = [0, 1, 2]
    shuffle(order)
    alphas = [None] * 3
    for k in order:
        alphas[k] = 1. + data_rng.uniform(low=-var, high=var)
    alpha3 = data_rng.normal(scale=alphastd, size=(3,))
    return aug_row(order, alphas, np.dot(eig_vec, eig_val * alpha3))


def check_aug(rows, n):
    """rows -> float64 [n, 13], or ValueError: one row per item, on 0 / 1, order a permutation of 0, 1, 2, every value
    finite as a float32."""
    try:
        rows = np.asarray(rows, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("aug rows must be %d numbers each (aug_row())" % AUG)
    if rows.ndim != 2 or rows.shape[1] != AUG or rows.shape[0] != n:
        raise ValueError("aug needs one row of %d values per item (%d items), got shape %s" % (AUG, n, rows.shape))
    with np.errstate(over="ignore"):
        if not np.isfinite(rows).all() or not np.isfinite(rows[:, 4:].astype(np.float32)).all():
            raise ValueError("aug rows must be finite")
    for r in rows:
        if r[0] not in (0.0, 1.0) or sorted(r[1:4].tolist()) != [0.0, 1.0, 2.0]:
            raise ValueError("aug row: on must be 0 or 1 and order a permutation of 0, 1, 2, got %r" % (r[:4].tolist(),))
    return rows


class PreProcess:
    """Owns a pinned staging buffer, a device byte arena for one max_h x max_w image (or a training batch of that many
    bytes), the device item table and the LUT.  load(img) -> run(out); run is capturable, and because every per-image
    value lives in device memory a captured run replays for an image of any size up to the capacity."""

    def __init__(self, in_h, in_w, scales=(1.0,), flip_test=False, max_h=1024, max_w=1024, mean=MEAN, std=STD,
                 device="cuda", max_items=None, keep_res=False, color_aug=False):
        if keep_res:
            raise NotImplementedError("keep_res pre-processing is not built (fix_res only: ctdet on pascal)")
        if color_aug and (flip_test or len(scales) != 1):
            raise ValueError("color_aug is a training mode: no flip_test, one scale")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise NotImplementedError("PreProcess needs a GPU device")
        self.in_h, self.in_w = int(in_h), int(in_w)
        self.scales = [float(s) for s in scales]
        self.flip_test = bool(flip_test)
        self.capacity = int(max_h) * int(max_w) * 3
        self.max_items = max(len(self.scales), int(max_items or 0))
        assert self.in_h > 0 and self.in_w > 0 and self.capacity > 0 and self.scales
        self._stage = torch.empty(self.capacity, dtype=torch.uint8).pin_memory()
        self._stage_np = self._stage.numpy()
        self._items_host = torch.zeros(self.max_items, ITEM, dtype=torch.float64).pin_memory()
        self.arena = torch.zeros(self.capacity, dtype=torch.uint8, device=self.device)
        self.items = torch.zeros(self.max_items, ITEM, dtype=torch.float64, device=self.device)
        self.lut = torch.from_numpy(lut(mean, std)).to(self.device)
        self.color_aug = bool(color_aug)
        if self.color_aug:      # the aug table, the crops' bytes as planes, the integer channel sums (uint64 bits)
            self._aug_host = torch.zeros(self.max_items, 16, dtype=torch.float32).pin_memory()
            self._aug_np = self._aug_host.numpy()
            self.aug = torch.zeros(self.max_items, 16, dtype=torch.float32, device=self.device)
            self.crop_u8 = torch.zeros(self.max_items * self.in_h * self.in_w * 3, dtype=torch.uint8, device=self.device)
            self.sums = torch.zeros(self.max_items, 3, dtype=torch.int64, device=self.device)
            self.mean_std = torch.from_numpy(np.concatenate([np.asarray(mean, dtype=np.float32).reshape(3),
                                                             np.asarray(std, dtype=np.float32).reshape(3)])).to(self.device)
        self.P = 0
        self._copied = None             # event behind the last copies out of the pinned buffers

    # ---- host -> device --------------------------------------------------------------------------------------------------
    def _bytes(self, data, n):
        """n bytes of `data` (numpy / torch, any device) into the arena, asynchronously on the current stream."""
        if isinstance(data, torch.Tensor) and data.is_cuda:
            self.arena[:n].copy_(data.contiguous().view(-1), non_blocking=True)
            return
        if isinstance(data, torch.Tensor):
            data = data.numpy()
        self._stage_np[:n] = np.asarray(data).reshape(-1)
        self.arena[:n].copy_(self._stage[:n], non_blocking=True)

    def _commit(self, rows, aug=None):
        self._items_host[:len(rows)] = torch.tensor(rows, dtype=torch.float64)
        self.items[:len(rows)].copy_(self._items_host[:len(rows)], non_blocking=True)
        if self.color_aug:
            aug = np.tile(np.asarray(AUG_OFF, dtype=np.float64), (len(rows), 1)) if aug is None else aug
            self._aug_np[:len(rows)] = 0
            self._aug_np[:len(rows), 4:AUG] = aug[:, 4:]
            self._aug_np.view(np.int32)[:len(rows), :4] = aug[:, :4].astype(np.int32)
            self.aug[:len(rows)].copy_(self._aug_host[:len(rows)], non_blocking=True)
        self.P = len(rows)
        self._copied = torch.cuda.Event()
        self._copied.record(torch.cuda.current_stream(self.device))

    def _reuse_pinned(self):
        if self._copied is not None:
            self._copied.synchronize()      # the previous image may still be on its way out of the pinned buffers

    def load(self, img):
        """img: uint8 [h, w, 3] (numpy, or a torch tensor on the CPU or the GPU).  Copies the bytes and the S items of
        the test scales; -> the S meta dicts of pre_process.  ValueError before any copy when the image is beyond the
        capacity."""
        if tuple(img.shape[2:]) != (3,) or len(img.shape) != 3 or str(img.dtype).split(".")[-1] != "uint8":
            raise ValueError("load() takes a uint8 [h, w, 3] image")
        h, w = int(img.shape[0]), int(img.shape[1])
        if h < 1 or w < 1 or h * w * 3 > self.capacity:
            raise ValueError("image %d x %d is beyond the arena's %d bytes" % (h, w, self.capacity))
        rows, metas = [], []
        for sc in self.scales:
            new_h, new_w, M, meta = crop_matrix(h, w, self.in_h, self.in_w, sc)
            check_matrix(M, self.in_h, self.in_w)
            rows.append(item_row(0, h, w, 3 * w, M, new_h, new_w))
            metas.append(meta)
        with torch.cuda.device(self.device):
            self._reuse_pinned()
            self._bytes(img, h * w * 3)
            self._commit(rows)
        return metas

    def check_table(self, nbytes, table, aug=None):
        """What load_items and load_table check before anything is copied: -> (rows, aug rows) or ValueError."""
        if aug is not None and not self.color_aug:
            raise ValueError("aug= needs PreProcess(..., color_aug=True)")
        table = np.asarray(table, dtype=np.float64).reshape(-1, ITEM)
        if nbytes > self.capacity or not 0 < len(table) <= self.max_items:
            raise ValueError("%d bytes / %d items are beyond the capacity (%d bytes, %d items)"
                             % (nbytes, len(table), self.capacity, self.max_items))
        rows = []
        for r in table:
            off, h, w, pitch, new_h, new_w = (int(v) for v in r[:6])
            if not np.array_equal(r[:6], [off, h, w, pitch, new_h, new_w]):
                raise ValueError("item sizes must be integers")
            if h < 1 or w < 1 or pitch < 3 * w or off < 0 or off + (h - 1) * pitch + 3 * w > nbytes:
                raise ValueError("item (offset %d, %d x %d, pitch %d) does not lie inside the %d bytes given"
                                 % (off, h, w, pitch, nbytes))
            if not (0 <= new_h < COORD_LIMIT and 0 <= new_w < COORD_LIMIT):
                raise ValueError("resized size %d x %d" % (new_h, new_w))
            check_matrix(r[9:15], self.in_h, self.in_w)
            rows.append(item_row(off, h, w, pitch, r[9:15], new_h, new_w, r[8] != 0.0))
        if aug is not None:
            aug = check_aug(aug, len(rows))
        return rows, aug

    def load_items(self, arena_bytes, table, aug=None):
        """The batched (training) form: arena_bytes = uint8 bytes that hold several images, table = [n][16] rows as
        item_row() builds them (any offset, pitch, matrix and flip_src; ratio_y / ratio_x are recomputed here).  Every
        row is checked against the bytes given before anything is copied.  aug (color_aug=True only): one aug row per
        item (aug_row(), color_aug_params(), AUG_OFF); None = every item off."""
        nbytes = int(np.prod(arena_bytes.shape))
        rows, aug = self.check_table(nbytes, table, aug)
        with torch.cuda.device(self.device):
            self._reuse_pinned()
            self._bytes(arena_bytes, nbytes)
            self._commit(rows, aug)

    def load_table(self, nbytes, table, aug=None):
        """load_items without the bytes: commits the item rows (and aug rows) for `nbytes` bytes that are ALREADY in
        self.arena, or that work queued on the current stream writes there before run() -- jpeg.JpegDecoder.run(pre.arena).
        The rows are checked against nbytes exactly as load_items checks them; nothing is copied when one is refused."""
        rows, aug = self.check_table(int(nbytes), table, aug)
        with torch.cuda.device(self.device):
            self._reuse_pinned()
            self._commit(rows, aug)

    # ---- launch ----------------------------------------------------------------------------------------------------------
    def out_shape(self):
        return ((2 if self.flip_test else 1) * self.P, 3, self.in_h, self.in_w)

    def run(self, out):
        """One launch on the current stream into the float32 GPU tensor [S or 2S, 3, in_h, in_w] (color_aug=True: the
        clearing of the sums and two launches into [P, 3, in_h, in_w]; self.sums[:P] then holds the crops' integer channel sums)."""
        if not out.is_cuda:
            raise NotImplementedError("PreProcess.run needs a GPU tensor")
        if self.P == 0:
            raise ValueError("PreProcess.run before load()")
        if out.dtype != torch.float32 or tuple(out.shape) != self.out_shape() or not out.is_contiguous() \
                or out.device != self.arena.device:
            raise ValueError("out must be a contiguous float32 %s tensor on %s" % (self.out_shape(), self.arena.device))
        stream = torch.cuda.current_stream(out.device).cuda_stream
        if self.color_aug:
            rc = N_.lib().cdn_ctdet_pre_process_aug(self.arena.data_ptr(), self.items.data_ptr(), self.P, self.aug.data_ptr(),
                                                    self.mean_std.data_ptr(), self.crop_u8.data_ptr(), self.sums.data_ptr(),
                                                    out.data_ptr(), self.in_h, self.in_w, stream)
            N_.check(rc, "cdn_ctdet_pre_process_aug")
            return out
        rc = N_.lib().cdn_ctdet_pre_process(self.arena.data_ptr(), self.items.data_ptr(), self.P, self.lut.data_ptr(),
                                            out.data_ptr(), self.in_h, self.in_w, int(self.flip_test), stream)
        N_.check(rc, "cdn_ctdet_pre_process")
        return out

    def __call__(self, img):
        metas = self.load(img)
        return self.run(torch.empty(self.out_shape(), dtype=torch.float32, device=self.device)), metas
