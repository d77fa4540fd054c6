"""What tests/test_gpu_heads_train.py, test_gpu_units_train.py and test_gpu_stem_train.py share: the quantised model, the
exact-arithmetic weight codes, the float32 fake-quantisation and the order-independent bound of the float64 comparisons,
and the captured-step / two-identical-runs checks of the QAT step with their criterion, targets and state collector.
A plain module (``from tests import qat_support``): no fixtures, nothing runs at import."""
import types

import numpy as np
import torch

from oracle import quant as Q

U = 2.0 ** -24


def model(classes=20, **kw):
    from codenet_amd import harness
    return harness.create_model(heads={"hm": classes, "wh": 2, "reg": 2}, quantize=True, **kw)


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------

def codes(g, rows, cols, nonzero):
    """Integer codes in [-7, 7], `nonzero` non-zero entries per row, one of them +-7."""
    w = torch.zeros(rows, cols)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:nonzero]
        v = torch.randint(1, 8, (nonzero,), generator=g).float() * (torch.randint(0, 2, (nonzero,), generator=g) * 2 - 1).float()
        v[0] = 7.0 if v[0] > 0 else -7.0
        w[r, idx] = v
    return w


# ---- running ranges, real arithmetic on the kernels' own intermediates ------------------------------------------------------

def fq32(v, x_min, x_max):
    """Fake-quantisation in float32, the reference's expression order (every operation rounds the same on both sides)."""
    scale, zp = Q.act_params(x_min, x_max)
    return Q.act_dequant(Q.act_codes(v, scale, zp), scale, zp)


def bound(n, S):
    return 1.01 * (n + 2) * U * S


SLACK = []      # (smallest slack, what) of every `within` of the process: a test may print its minimum


def within(got, ref, n, S, what):
    err = (got.detach().double().cpu() - ref).abs()
    tol = bound(n, S)
    worst = float((err - tol).max())
    SLACK.append((-worst, what))
    print("%-44s max err %.3e, smallest slack %.3e (bound up to %.3e)" % (what, float(err.max()), -worst, float(tol.max())))
    assert worst <= 0, what


# ---- reproducibility and capture of the QAT step ----------------------------------------------------------------------------

def default_opt():
    return types.SimpleNamespace(mse_loss=False, reg_loss="l1", dense_wh=False, norm_wh=False, cat_spec_wh=False,
                                 num_stacks=1, hm_weight=1.0, wh_weight=0.1, off_weight=1.0, reg_offset=True)


def objects(N, M, H, W, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform([1, 1], [W - 2, H - 2], (N, M, 2))
    s = rng.uniform(0.8, 12.0, (N, M, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], 2)
    boxes[..., [0, 2]] = np.clip(boxes[..., [0, 2]], 0, W - 1)
    boxes[..., [1, 3]] = np.clip(boxes[..., [1, 3]], 0, H - 1)
    return (torch.from_numpy(boxes.astype(np.float32)).cuda(), torch.from_numpy(rng.integers(0, 20, (N, M))).cuda(),
            torch.from_numpy(rng.integers(1, M + 1, N)).cuda())


def train_net(wrapper, **kw):
    """`wrapper` (a pipeline.Detection* class) over a fresh quantised model, on the GPU in train mode, BatchNorm in eval."""
    net = wrapper(model(**kw)).cuda().train()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    return net


def state(net, opt):
    """Parameters, buffers (QuantAct ranges), the optimizer's state and the QuantActs' device words."""
    ts = list(net.parameters()) + list(net.buffers())
    for st in opt.state.values():
        ts += [v for v in st.values() if torch.is_tensor(v)]
    ts += [m._state for m in net.modules() if torch.is_tensor(getattr(m, "_state", None))]
    return ts


def step_setup(make_input, count):
    """(loss_fn, inputs): CtdetLoss on the native criterion over fixed targets at N = 2, 32 x 32 maps, and `count` inputs
    ``make_input(g, N, R)`` drawn in turn from one generator."""
    from codenet_amd.losses import CtdetLoss, ctdet_targets
    N, M, R = 2, 8, 32
    crit = CtdetLoss(default_opt())
    batch = ctdet_targets(*objects(N, M, R, R, 3), 20, R, R, M)

    def loss_fn(net, x):
        out = net(x)
        assert crit.native_reason(out, batch) is None
        return crit(out, batch)[0]

    g = torch.Generator().manual_seed(2)
    return loss_fn, [make_input(g, N, R).cuda() for _ in range(count)]


def with_capturable_adam(net):
    return net, torch.optim.Adam(net.parameters(), lr=torch.tensor(1.25e-4, device="cuda"), capturable=True)


def check_captured_step(eager, graphed, loss_fn, inputs, took_part):
    """`eager` and `graphed` are two (net, capturable Adam) built alike.  The second is captured on inputs[0] (no
    `unvalidated`: the caller has asserted its scope) with three warm-up steps, which the first repeats eagerly; then
    every further input is one step of both: the losses, and at the end every parameter, range, Adam state and device
    word, must be bit-identical, and every parameter whose name `took_part` accepts must have a non-zero gradient."""
    from codenet_amd import pipeline
    (net_e, opt_e), (net_g, opt_g) = eager, graphed
    step = pipeline.GraphedTrainStep(net_g, opt_g, loss_fn, (inputs[0],), warmup=3)
    for _ in range(3):
        opt_e.zero_grad(set_to_none=True)
        loss_fn(net_e, inputs[0]).backward()
        opt_e.step()
    for x in inputs[1:]:
        opt_e.zero_grad(set_to_none=True)
        le = loss_fn(net_e, x)
        le.backward()
        opt_e.step()
        lg = step(x)
        assert torch.equal(le.detach(), lg.detach())
    torch.cuda.synchronize()
    assert le.detach().item() == le.detach().item() and le.detach().item() > 0
    took = 0
    for (n1, p1), (n2, p2) in zip(net_e.named_parameters(), net_g.named_parameters()):
        assert torch.equal(p1, p2), n1
        if took_part(n1):
            assert p1.grad is not None and float(p1.grad.abs().sum()) > 0, n1
            took += 1
    assert took
    for u, v in zip(state(net_e, opt_e), state(net_g, opt_g)):      # ranges, Adam state, device words
        assert torch.equal(u, v)


def check_two_identical_runs(build_net, loss_fn, inputs):
    """Two eager runs over `inputs` from freshly built nets end with the same losses and bit-identical state."""
    def run():
        net = build_net()
        opt = torch.optim.Adam(net.parameters(), lr=1.25e-4)
        losses = []
        for x in inputs:
            opt.zero_grad(set_to_none=True)
            loss = loss_fn(net, x)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        return losses, [t.detach().clone() for t in state(net, opt)]

    l1, s1 = run()
    l2, s2 = run()
    assert l1 == l2
    assert len(s1) == len(s2) and all(torch.equal(u, v) for u, v in zip(s1, s2))
