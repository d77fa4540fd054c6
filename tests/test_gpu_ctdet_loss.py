"""The native criterion and target maps (codenet_loss.hip through codenet_amd.losses) on the GPU.

Yardsticks: the reference's float64 results of tests/golden/ctdet_loss_ref.npz, and at the real shape the PyTorch
composition of losses.py in float64 (pinned to the reference by tests/test_ctdet_loss.py).  Criteria:

  scalars    |native - ref64| <= max(4 x the reference's own float32 error, 8 float32 ulps of the value): the block is
             float32 and a handful of roundings combine the partial sums.
  gradients  max |native - ref64| / max |ref64| <= 4 x the reference's own float32 figure: device exp / log are allowed
             one more ulp than libm and two of them chain.  Elements whose float64 sigmoid lies within 1e-6 relative of a
             clamp bound may be left out, at most 1e-4 of all elements.
  targets    ind, reg_mask, wh, reg bitwise; hm bitwise except that at most 1e-5 of its non-zero elements may differ by
             one float32 ulp (last bit of the double exp), never an element that is 1.0 in the fixture.

Measured on an MI355X (the figures are printed by every run): see DESIGN.md section 4.3a.
"""
import os
import types

import numpy as np
import pytest
import torch

from tests.test_ctdet_loss import GOLD, KEYS, grads_of, load_case

LO, HI = 1e-4, 1 - 1e-4


def scalar_ok(got, want, err32):
    tol = np.maximum(4 * np.asarray(err32), 8 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64))
    return np.abs(got - want), tol


def near_clamp(logits):
    s = torch.sigmoid(logits.double())
    return ((s - LO).abs() <= 1e-6 * LO) | ((s - HI).abs() <= 1e-6 * HI)


def grad_error(got, ref, skip=None):
    """largest |got - ref| over the largest |ref| (elements in `skip` left out of the numerator)."""
    d = (got.double() - ref.double()).abs()
    if skip is not None:
        assert float(skip.double().mean()) <= 1e-4
        d = d.masked_fill(skip, 0.0)
    top = float(ref.abs().max())
    return float(d.max()) / top if top > 0 else float(d.max())


def default_opt(**kw):
    o = dict(mse_loss=False, reg_loss="l1", dense_wh=False, norm_wh=False, cat_spec_wh=False, num_stacks=1, hm_weight=1.0,
             wh_weight=0.1, off_weight=1.0, reg_offset=True)
    o.update(kw)
    return types.SimpleNamespace(**o)


def random_objects(N, M, H, W, seed, full=False):
    rng = np.random.default_rng(seed)
    c = rng.uniform([1, 1], [W - 2, H - 2], (N, M, 2))
    s = rng.uniform(0.8, 40.0, (N, M, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], 2)
    boxes[..., [0, 2]] = np.clip(boxes[..., [0, 2]], 0, W - 1)
    boxes[..., [1, 3]] = np.clip(boxes[..., [1, 3]], 0, H - 1)
    counts = np.full(N, M) if full else rng.integers(0, M + 1, N)
    return (torch.from_numpy(boxes.astype(np.float32)).cuda(), torch.from_numpy(rng.integers(0, 20, (N, M))).cuda(),
            torch.from_numpy(counts).cuda())


def run(crit, heads, batch, composed=False, dtype=None, keep_hm=False):
    """forward + backward on fresh leaves -> (4 scalars as a float64 array, loss_stats, [grads per stack])."""
    leaves = [[t.detach().to(dtype or t.dtype).clone().requires_grad_(True) for t in trio] for trio in heads]
    b = {k: (v.to(dtype) if dtype is not None and v.is_floating_point() else v) for k, v in batch.items()}
    outputs = [{"hm": l[0].clone() if composed else l[0], "wh": l[1], "reg": l[2]} for l in leaves]
    if composed:
        loss, stats = crit._forward_composed(outputs, b)
    else:
        assert crit.native_reason(outputs, b) is None
        loss, stats = crit(outputs, b, keep_hm=keep_hm)
    loss.backward()
    grads = [[l.grad if l.grad is not None else torch.zeros_like(l) for l in ls] for ls in leaves]
    scal = np.array([float(stats[k].detach()) if torch.is_tensor(stats[k]) else float(stats[k]) for k in KEYS])
    return scal, stats, grads, outputs


@pytest.mark.gpu
def test_loss_fixture_native_against_the_reference_float64():
    from codenet_amd.losses import CtdetLoss
    z = np.load(os.path.join(GOLD, "ctdet_loss_ref.npz"))
    worst_s, worst_g = 0.0, 0.0
    for k in range(len(z["names"])):
        opt, outputs, leaves, batch = load_case(z, k, torch.float32, "cuda")
        outputs = [{"hm": l[0], "wh": l[1], "reg": l[2]} for l in leaves]          # the native path keeps the logits
        crit = CtdetLoss(opt)
        assert crit.native_reason(outputs, batch) is None
        loss, stats = crit(outputs, batch)
        assert all(torch.is_tensor(stats[n]) and stats[n]._base is loss._base for n in KEYS)      # views of one block
        assert outputs[0]["hm"] is leaves[0][0]
        loss.backward()
        got = np.array([float(stats[n].detach()) for n in KEYS])
        err, tol = scalar_ok(got, z["c%d_scalars" % k], z["c%d_err_scalars" % k])
        print("case %-24s scalar error %s (bound %s)" % (z["names"][k], err, tol))
        assert np.all(err <= tol), (z["names"][k], got, z["c%d_scalars" % k])
        worst_s = max(worst_s, float((err / tol).max()))
        for s, gs in enumerate(grads_of(leaves)):
            skip = near_clamp(leaves[s][0].detach())
            for j, (n, g) in enumerate(zip(("g_hm", "g_wh", "g_reg"), gs)):
                ref = torch.from_numpy(z["c%d_%s%d" % (k, n, s)])
                e = grad_error(torch.from_numpy(g), ref, skip.cpu() if j == 0 else None)
                bound = 4 * float(z["c%d_err_grads%d" % (k, s)][j])
                print("     stack %d %-5s gradient error %.3g (bound %.3g)" % (s, n, e, bound))
                assert e <= bound, (z["names"][k], n, s, e, bound)
                if j == 0:
                    assert np.array_equal((g == 0)[~skip.cpu().numpy()], (ref.numpy() == 0)[~skip.cpu().numpy()])
                    worst_g = max(worst_g, e / bound)
    print("worst scalar error / bound %.3f, worst hm gradient error / bound %.3f" % (worst_s, worst_g))


@pytest.fixture(scope="module")
def real_shape():
    """N = 32, C = 20, 128 x 128, M = 50, seeded: heads, device-built targets, and the composition's float64 / float32
    results (computed once, shared, never modified)."""
    from codenet_amd.losses import CtdetLoss, ctdet_targets
    N, C, H, W, M = 32, 20, 128, 128, 50
    g = torch.Generator().manual_seed(2024)
    heads = [((torch.randn(N, C, H, W, generator=g) * 1.5 - 2.0).cuda(), (torch.rand(N, 2, H, W, generator=g) * 30).cuda(),
              (torch.rand(N, 2, H, W, generator=g) * 2 - 0.5).cuda())]
    boxes, classes, counts = random_objects(N, M, H, W, 5)
    batch = ctdet_targets(boxes, classes, counts, C, H, W, M)
    crit = CtdetLoss(default_opt())
    s64, _, g64, _ = run(crit, heads, batch, composed=True, dtype=torch.float64)
    s32, _, g32, _ = run(crit, heads, batch, composed=True)
    return dict(heads=heads, batch=batch, crit=crit, s64=s64, g64=g64, s32=s32, g32=g32)


@pytest.mark.gpu
def test_real_shape_against_the_float64_composition(real_shape):
    r = real_shape
    got, stats, grads, _ = run(r["crit"], r["heads"], r["batch"])
    err, tol = scalar_ok(got, r["s64"], np.abs(r["s32"] - r["s64"]))
    print("real shape: scalars %s, error %s, bound %s" % (got, err, tol))
    assert np.all(err <= tol)
    skip = near_clamp(r["heads"][0][0])
    for j, n in enumerate(("hm", "wh", "reg")):
        bound = 4 * grad_error(r["g32"][0][j], r["g64"][0][j])
        e = grad_error(grads[0][j], r["g64"][0][j], skip if j == 0 else None)
        print("real shape: %s gradient error %.3g (bound %.3g)" % (n, e, bound))
        assert e <= bound, n
    keep = ~skip
    assert torch.equal((grads[0][0] == 0)[keep], (r["g64"][0][0] == 0)[keep])


@pytest.mark.gpu
def test_keep_hm_and_no_grad_materialise_the_clamped_sigmoid(real_shape):
    r = real_shape
    heads = [tuple(t[:2] for t in r["heads"][0])]
    batch = {k: v[:2] for k, v in r["batch"].items()}
    _, _, _, outputs = run(r["crit"], heads, batch, keep_hm=True)
    want = torch.clamp(torch.sigmoid(heads[0][0].double()), LO, HI)
    assert outputs[0]["hm"].data_ptr() != heads[0][0].data_ptr()
    # p < 1, so a float32 ulp is at most 6e-8: expf (up to two ulps), the add and the division round once each
    assert float((outputs[0]["hm"].double() - want).abs().max()) <= 2.5e-7
    assert float(outputs[0]["hm"].min()) >= np.float32(LO) and float(outputs[0]["hm"].max()) <= np.float32(HI)
    with torch.no_grad():
        outs = [{"hm": heads[0][0].clone(), "wh": heads[0][1], "reg": heads[0][2]}]
        logits = outs[0]["hm"]
        loss, _ = r["crit"](outs, batch)
    assert torch.equal(outs[0]["hm"], outputs[0]["hm"]) and outs[0]["hm"] is not logits and not loss.requires_grad


@pytest.mark.gpu
def test_reproducible_and_independent_of_row_order():
    """Two runs are bit-identical; permuting the object rows while rows of one cell keep their order changes nothing
    (the regression sums are double sums of float32 terms above 2^-20: exact, so order-free); rows that share a cell
    give the in-order float32 sum of their single gradients."""
    from codenet_amd.losses import CtdetLoss
    N, C, H, W, M = 3, 4, 24, 20, 12
    g = torch.Generator().manual_seed(9)
    heads = [((torch.randn(N, C, H, W, generator=g) - 1.5).cuda(), (torch.rand(N, 2, H, W, generator=g) * 9).cuda(),
              torch.rand(N, 2, H, W, generator=g).cuda())]
    ind = torch.stack([torch.randperm(H * W, generator=g)[:M] for _ in range(N)])
    ind[0, 5] = ind[0, 2]                                   # two rows on one cell
    ind[1, 3] = ind[1, 9] = ind[1, 10] = ind[1, 0]          # four rows on one cell
    mask = torch.ones(N, M, dtype=torch.uint8)
    mask[2, 7:] = 0
    hm = torch.zeros(N, C, H, W)
    hm.view(N, C, -1)[:, 1].scatter_(1, ind, 1.0)
    hm[:, 2] = torch.rand(N, H, W, generator=g) * 0.9
    batch = {"hm": hm.cuda(), "wh": (torch.rand(N, M, 2, generator=g) * 9).cuda(), "reg": torch.rand(N, M, 2, generator=g).cuda(),
             "ind": ind.cuda(), "reg_mask": mask.cuda()}
    for reg_loss in ("l1", "sl1"):
        crit = CtdetLoss(default_opt(reg_loss=reg_loss, wh_weight=0.37))
        a = run(crit, heads, batch)
        b = run(crit, heads, batch)
        assert np.array_equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2][0], b[2][0]))
        # a permutation that keeps the rows of a shared cell in their order: sort a random key, then restore the order
        # inside every group of equal cells
        pb = {k: v.clone() for k, v in batch.items()}
        for n in range(N):
            perm = torch.randperm(M, generator=g).tolist()
            cells = ind[n].tolist()
            for cell in set(cells):
                slots = [i for i, p in enumerate(perm) if cells[p] == cell]
                for slot, p in zip(slots, sorted(perm[i] for i in slots)):
                    perm[slot] = p
            assert sorted(perm) == list(range(M)) and perm != list(range(M))
            for k in ("wh", "reg", "ind", "reg_mask"):
                pb[k][n] = batch[k][n][torch.tensor(perm).cuda()]
        c = run(crit, heads, pb)
        assert np.array_equal(a[0], c[0]) and all(torch.equal(x, y) for x, y in zip(a[2][0], c[2][0]))
        # shared cells: the dense gradient is the in-order sum of the gradients each row gives alone
        for head, key in ((1, "wh"), (2, "reg")):
            for n, rows in ((0, [2, 5]), (1, [0, 3, 9, 10])):
                acc = torch.zeros(2, device="cuda")
                free = [q for q in range(H * W) if q not in ind[n].tolist()]
                for row in rows:
                    sb = {k: v.clone() for k, v in batch.items()}
                    others = [q for q in rows if q != row]
                    sb["ind"][n, others] = torch.tensor(free[:len(others)]).cuda()     # the others move to unused cells
                    alone = run(crit, heads, sb)
                    cell = int(ind[n, row])
                    acc = acc + alone[2][0][head][n, :, cell // W, cell % W]
                cell = int(ind[n, rows[0]])
                assert torch.equal(a[2][0][head][n, :, cell // W, cell % W], acc), (reg_loss, key, n)


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_graph():
    from codenet_amd.losses import CtdetLoss, ctdet_targets
    N, C, H, W, M = 2, 20, 64, 64, 16
    g = torch.Generator().manual_seed(31)
    mk = lambda: [(torch.randn(N, C, H, W, generator=g) - 2).cuda(), (torch.rand(N, 2, H, W, generator=g) * 20).cuda(),   # noqa: E731
                  torch.rand(N, 2, H, W, generator=g).cuda()]
    crit = CtdetLoss(default_opt())
    static = [t.requires_grad_(True) for t in mk()]
    batch = ctdet_targets(*random_objects(N, M, H, W, 1), C, H, W, M)
    outputs = [{"hm": static[0], "wh": static[1], "reg": static[2]}]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            crit(outputs, batch)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in static:
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, stats = crit(outputs, batch)
        loss.backward()
    new_heads, new_batch = mk(), ctdet_targets(*random_objects(N, M, H, W, 2), C, H, W, M)
    with torch.no_grad():
        for t, v in zip(static, new_heads):
            t.copy_(v)
        for k in batch:
            batch[k].copy_(new_batch[k])
    graph.replay()
    torch.cuda.synchronize()
    eager = run(crit, [tuple(new_heads)], new_batch)
    assert np.array_equal(np.array([float(stats[k].detach()) for k in KEYS]), eager[0])
    for t, e in zip(static, eager[2][0]):
        assert torch.equal(t.grad, e)


@pytest.mark.gpu
def test_target_fixture_on_the_device():
    from codenet_amd.losses import ctdet_targets
    z = np.load(os.path.join(GOLD, "ctdet_targets_ref.npz"))
    for t in range(2):
        C, H, W = (int(v) for v in z["t%d_shape" % t])
        boxes = torch.from_numpy(z["t%d_boxes" % t]).cuda()
        out = ctdet_targets(boxes, torch.from_numpy(z["t%d_classes" % t]).cuda(), torch.from_numpy(z["t%d_counts" % t]).cuda(),
                            C, H, W, boxes.shape[1])
        for n in ("wh", "reg", "ind", "reg_mask"):
            want = z["t%d_%s" % (t, n)]
            got = out[n].cpu().numpy()
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (t, n)
        got, want = out["hm"].cpu().numpy(), z["t%d_hm" % t]
        diff = got != want
        print("targets shape %d: %d of %d non-zero hm elements differ" % (t, diff.sum(), (want != 0).sum()))
        assert not diff[want == 1].any() and not diff[want == 0].any()
        assert diff.sum() <= 1e-5 * (want != 0).sum()
        assert np.all(np.abs(got[diff].view(np.int32) - want[diff].view(np.int32)) <= 1)


@pytest.mark.gpu
def test_targets_at_the_real_shape_match_the_host_composition(real_shape):
    """M = 50 rows, 128 x 128: the device maps against losses.py's host composition (bitwise pinned to the reference by
    the CPU test), same allowance for the double exp."""
    from codenet_amd.losses import ctdet_targets
    boxes, classes, counts = random_objects(4, 50, 128, 128, 5)
    dev = ctdet_targets(boxes, classes, counts, 20, 128, 128, 50)
    host = ctdet_targets(boxes.cpu(), classes.cpu(), counts.cpu(), 20, 128, 128, 50)
    for n in ("wh", "reg", "ind", "reg_mask"):
        assert torch.equal(dev[n].cpu(), host[n]), n
    got, want = dev["hm"].cpu().numpy(), host["hm"].numpy()
    diff = got != want
    print("targets 128 x 128: %d of %d non-zero hm elements differ" % (diff.sum(), (want != 0).sum()))
    assert not diff[want == 1].any() and not diff[want == 0].any() and diff.sum() <= 1e-5 * (want != 0).sum()
    assert np.all(np.abs(got[diff].view(np.int32) - want[diff].view(np.int32)) <= 1)


@pytest.mark.gpu
def test_end_to_end_device_targets_native_loss_on_the_quantised_model():
    from codenet_amd import harness
    from codenet_amd.losses import CtdetLoss, ModelWithLoss, ctdet_targets
    model = harness.create_model(quantize=True).cuda().train()
    N, M = 2, 50
    x = torch.randn(N, 3, 256, 256, generator=torch.Generator().manual_seed(5)).cuda()
    batch = ctdet_targets(*random_objects(N, M, 64, 64, 3), 20, 64, 64, M)
    batch["input"] = x
    crit = CtdetLoss(default_opt())
    seen = {}
    crit.register_forward_pre_hook(lambda m, args: seen.update(reason=m.native_reason(*args[:2]), heads=args[0][-1]))
    last, loss, stats = ModelWithLoss(model, crit)(batch)
    assert seen["reason"] is None and tuple(last["hm"].shape) == (N, 20, 64, 64)
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) > 50 and all(torch.isfinite(gr).all() for gr in grads)
    heads = [tuple(seen["heads"][k].detach() for k in ("hm", "wh", "reg"))]
    s64 = run(crit, heads, batch, composed=True, dtype=torch.float64)[0]
    s32 = run(crit, heads, batch, composed=True)[0]
    got = np.array([float(stats[k].detach()) for k in KEYS])
    err, tol = scalar_ok(got, s64, np.abs(s32 - s64))
    print("end to end: scalars %s, error %s, bound %s" % (got, err, tol))
    assert np.all(err <= tol)
