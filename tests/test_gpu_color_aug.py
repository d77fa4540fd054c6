"""The colour augmentation kernels (codenet_preproc.hip: cdn_ctdet_pre_process_aug = zero_sums_kernel + crop_sum_kernel +
color_aug_kernel; codenet_amd/preproc.py: PreProcess(color_aug=True)) against the numpy restatement of DESIGN.md section
7.4c (tests/color_aug_ref.py).  The crop and the channel sums are integer, every float operation is rounded on its own on
both sides, so every comparison is torch.equal over the whole tensor."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from tests import color_aug_ref as C

pytestmark = pytest.mark.gpu

# (64, 64): 16 full workgroups per item; (48, 80): 15; (7, 9): 63 pixels -- one partial wave and three waves without a
# pixel, so the reduction must ignore dead lanes
SHAPES = ((64, 64), (48, 80), (7, 9))
ORDERS = list(itertools.permutations((0, 1, 2)))


def _image(hw, seed):
    return np.random.default_rng(1000 * hw[0] + hw[1] + seed).integers(0, 256, hw + (3,), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _load(shape, variant=0):
    """One load_items of eight items drawn from a 37 x 53 and a 20 x 31 image that lie in one arena at an offset, with
    pitch > 3 w: the six orders, one off item, one more drawn by color_aug_params; two crops larger than their image on
    all four sides (the border counts in N and in the sums), two flip_src items, one resized item, a rotated matrix.
    -> (arena, table, rows, float32 [8, 3, h, w] of the restatement, int64 [8, 3] sums); computed once per shape."""
    from codenet_amd import preproc
    in_h, in_w = shape
    a, b = _image((37, 53), 1 + 10 * variant), _image((20, 31), 2 + 10 * variant)
    pa, pb = 53 * 3 + 5, 31 * 3 + 1
    off_a = 7
    off_b = off_a + 37 * pa + 3
    arena = np.random.default_rng(5 + variant).integers(0, 256, off_b + 20 * pb + 11, dtype=np.uint8)
    for img, off, pitch in ((a, off_a, pa), (b, off_b, pb)):
        for y in range(img.shape[0]):
            arena[off + y * pitch: off + y * pitch + img.shape[1] * 3] = img[y].reshape(-1)
    f32 = np.float32
    m_corner = preproc.train_matrix(np.array([5.0, 4.0], dtype=f32), 60.0, in_w, in_h)
    m_flip = preproc.train_matrix(np.array([15.5, 10.0], dtype=f32), 31.0 * 0.9, in_w, in_h)
    k, th = 53.0 / in_w, math.radians(17.0)
    m_rot = [k * math.cos(th), -k * math.sin(th), 9.25, k * math.sin(th), k * math.cos(th), -6.5]
    m_rs = preproc.train_matrix(np.array([23.0, 15.0], dtype=f32), 50.0, in_w, in_h)
    m_wide_a = preproc.train_matrix(np.array([26.5, 18.5], dtype=f32), 53.0 * 1.6 * max(1.0, in_w / in_h), in_w, in_h)
    m_wide_b = preproc.train_matrix(np.array([15.5, 10.0], dtype=f32), 31.0 * 1.7 * max(1.0, in_w / in_h), in_w, in_h)
    # (image, offset, pitch, matrix, new_h, new_w, flip_src)
    geo = [(a, off_a, pa, m_corner, 37, 53, False), (b, off_b, pb, m_flip, 20, 31, True),
           (a, off_a, pa, m_rot, 37, 53, False), (b, off_b, pb, m_rs, 30, 46, True),
           (a, off_a, pa, m_wide_a, 37, 53, False), (b, off_b, pb, m_flip, 20, 31, False),
           (a, off_a, pa, m_corner, 37, 53, False), (b, off_b, pb, m_wide_b, 20, 31, False)]
    rng = np.random.RandomState(77 + variant)
    rows = []
    for order in (ORDERS if variant == 0 else ORDERS[::-1]):
        d = np.dot(C.EIG_VEC, C.EIG_VAL * rng.normal(scale=0.1, size=(3,)))
        rows.append(preproc.aug_row(order, 1.0 + rng.uniform(-0.4, 0.4, 3), d))
    rows.append(preproc.AUG_OFF)
    rows.append(preproc.color_aug_params(rng, shuffle=np.random.RandomState(3 + variant).shuffle))
    table = [preproc.item_row(off, img.shape[0], img.shape[1], pitch, M, new_h=nh, new_w=nw, flip_src=fl)
             for img, off, pitch, M, nh, nw, fl in geo]
    want, sums = [], []
    for (img, off, pitch, M, nh, nw, fl), row in zip(geo, rows):
        w, s = C.pre_process_aug(img, nh, nw, M, in_h, in_w, C.from_list(row), flip_src=fl)
        want.append(w)
        sums.append(s)
    for i in (4, 7):        # larger than the image on all four sides: a black frame, inside the sums' N
        u8 = C.crop_u8(geo[i][0], geo[i][4], geo[i][5], geo[i][3], in_h, in_w)
        assert not u8[0].any() and not u8[-1].any() and not u8[:, 0].any() and not u8[:, -1].any() and u8.any()
    arena.setflags(write=False)
    return arena, table, rows, torch.from_numpy(np.stack(want, 0)), torch.tensor(sums, dtype=torch.int64)


def _pre(shape):
    from codenet_amd import preproc
    return preproc.PreProcess(shape[0], shape[1], max_h=64, max_w=64, max_items=8, color_aug=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_equals_restatement_every_element(shape):
    arena, table, rows, want, sums = _load(shape)
    pre = _pre(shape)
    pre.load_items(arena, table, aug=rows)
    out = torch.empty(8, 3, shape[0], shape[1], device="cuda")
    assert pre.out_shape() == tuple(out.shape)
    pre.run(out)
    assert torch.equal(pre.sums[:8].cpu(), sums), "channel sums %s" % (shape,)
    for i in range(8):
        assert torch.equal(out[i].cpu(), want[i]), "item %d of %s" % (i, shape)
    # the augmentation did something: item 0 and the off item 6 share their geometry
    assert torch.equal(pre.sums[0], pre.sums[6]) and not torch.equal(out[0], out[6])


def test_second_run_is_bit_identical():
    """... and the sums are those of ONE run: they are zeroed in front of every run."""
    arena, table, rows, want, sums = _load((48, 80))
    pre = _pre((48, 80))
    pre.load_items(arena, table, aug=rows)
    first = pre.run(torch.empty(8, 3, 48, 80, device="cuda")).clone()
    second = pre.run(torch.zeros(8, 3, 48, 80, device="cuda"))
    assert torch.equal(first, second) and torch.equal(second.cpu(), want)
    assert torch.equal(pre.sums[:8].cpu(), sums)


def test_captured_run_replays_for_other_images_and_rows():
    """Capture after one load, replay twice after a different load.  The second replay equals the restatement only if the
    clearing of the sums is a node of the graph and clears on every replay (otherwise the sums are not those of one run
    and every contrast step moves).  The runtime's memset node did not: DESIGN.md section 7.4c."""
    shape = (48, 80)
    pre = _pre(shape)
    out = torch.zeros(8, 3, 48, 80, device="cuda")
    arena, table, rows, want0, _ = _load(shape)
    pre.load_items(arena, table, aug=rows)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pre.run(out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pre.run(out)
    arena, table, rows, want1, sums1 = _load(shape, 1)
    assert not torch.equal(want0, want1)
    pre.load_items(arena, table, aug=rows)
    for replay in range(2):
        out.zero_()
        graph.replay()
        assert torch.equal(pre.sums[:8].cpu(), sums1), "replay %d" % replay
        assert torch.equal(out.cpu(), want1), "replay %d" % replay


def test_identity_row_equals_an_off_item():
    from codenet_amd import preproc
    arena, table, _, want, _ = _load((48, 80))
    pre = _pre((48, 80))
    pre.load_items(arena, table, aug=[preproc.AUG_IDENTITY] * 4 + [preproc.AUG_OFF] * 4)
    ident = pre.run(torch.empty(8, 3, 48, 80, device="cuda")).clone()
    pre.load_items(arena, table)                                    # aug=None: every item off
    off = pre.run(torch.empty(8, 3, 48, 80, device="cuda"))
    assert torch.equal(ident, off)
    assert torch.equal(off[6].cpu(), want[6])                       # item 6 is off in the shared load too


def test_errors_leave_the_stream_usable():
    from codenet_amd import preproc
    shape = (48, 80)
    arena, table, rows, want, sums = _load(shape)
    pre = _pre(shape)
    pre.load_items(arena, table, aug=rows)
    out = torch.empty(8, 3, 48, 80, device="cuda")
    pre.run(out)
    other = _load(shape, 1)[0]
    bad_order, bad_value = [list(r) for r in rows], [list(r) for r in rows]
    bad_order[3][1:4] = [0, 0, 2]
    bad_value[5][8] = float("nan")
    for aug in (bad_order, bad_value, rows[:7]):                    # refused before anything is copied
        with pytest.raises(ValueError):
            pre.load_items(other, table, aug=aug)
    with pytest.raises(ValueError):                                 # an item outside the bytes given, with good rows
        pre.load_items(other, [table[0], preproc.item_row(int(table[1][0]), 21, 31, 31 * 3 + 1, table[1][9:15])] + table[2:],
                       aug=rows)
    plain = preproc.PreProcess(48, 80, max_h=64, max_w=64, max_items=8)
    with pytest.raises(ValueError):
        plain.load_items(arena, table, aug=rows)
    with pytest.raises(ValueError):
        plain.run(torch.empty(8, 3, 48, 80, device="cuda"))         # nothing was loaded
    with pytest.raises(ValueError):
        preproc.PreProcess(48, 80, flip_test=True, color_aug=True)
    out.zero_()
    pre.run(out)
    assert torch.equal(out.cpu(), want) and torch.equal(pre.sums[:8].cpu(), sums)
