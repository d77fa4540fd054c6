"""Frozen-range (serving) schedules on byte codes: calibration (cover_frozen_ranges / calibrate_serving /
prepare_serving), overflow flags, FrozenHotPath, FrozenBackbone.

Part of codenet_amd.pipeline (split by concern in round 6; `from codenet_amd import pipeline` exposes every name as
before)."""
import os

import torch
import torch.nn as nn

from ..ops import _p as ptr
from .common import (OverflowFlags, act_fusable, set_running_stat, uniform_act_settings)
from .hotpath import (FusedHotPath, act_pointers, capture_graph, deform_stages, stage_acts, stage_fused_forward,
                      stage_params, unpack_nchw)
from .backbone import (FusedBackbone)


def cover_frozen_ranges(net, batches, forward=None, margin=0.02, passes=2, spread=None):
    """Deployment step for the byte-code serving mode.  With ``running_stat = False`` the reference keeps the EMA
    ranges it trained with (quant_modules.py:203-219 skipped) and a value outside such a range simply becomes a code
    beyond the 8-bit grid (the fake-quantised float has no clamp, quant_utils.py:132-171).  A byte cannot hold that code
    -- the frozen kernels flag it (``overflowed()``) and the caller goes back to the fp32 schedule -- and an EMA range
    is routinely exceeded: a QuantAct shared by the units of a ShuffleNetV2 layer averages the extremes of four
    different tensors.  This helper runs ``forward(batch)`` (default: ``net``) on calibration batches with every
    QuantAct frozen, records what each one is fed, and WIDENS x_min / x_max (never narrows) to cover it with `margin` of
    the span to spare; two passes, since moving a grid moves what the layers behind it see.  It changes the model's
    quantisation grids -- the same widened model is what the fp32 frozen schedule is compared on.  Returns the number of
    QuantActs whose range moved.  spread (a dict, round 6): receives id(act) -> (sigma_lo, sigma_hi), the standard
    deviations of the per-BATCH extremes over the calibration batches of the last pass (what calibrate_serving's
    `sigmas` policy prices the tail of unseen batches with); needs >= 2 batches."""
    from ..portable_quantizer.quant_modules import QuantAct
    acts = [m for m in net.modules() if isinstance(m, QuantAct)]
    was = [a.running_stat for a in acts]
    forward = forward if forward is not None else net
    moved = set()
    try:
        for a in acts:
            a.running_stat = False
        for _ in range(passes):
            seen, per_batch, cur = {}, {}, [0]

            def hook(mod, args):
                x = args[0].detach()
                lo, hi = x.min().float(), x.max().float()
                if id(mod) in seen:
                    seen[id(mod)] = (torch.minimum(seen[id(mod)][0], lo), torch.maximum(seen[id(mod)][1], hi))
                else:
                    seen[id(mod)] = (lo, hi)
                pb = per_batch.setdefault(id(mod), {})      # (a QuantAct shared by several call sites: one pair per batch)
                if cur[0] in pb:
                    pb[cur[0]] = (torch.minimum(pb[cur[0]][0], lo), torch.maximum(pb[cur[0]][1], hi))
                else:
                    pb[cur[0]] = (lo, hi)
            handles = [a.register_forward_pre_hook(hook) for a in acts]
            try:
                with torch.no_grad():
                    for bi, b in enumerate(batches):
                        cur[0] = bi
                        forward(b)
            finally:
                for h_ in handles:
                    h_.remove()
            if acts and not seen:
                raise RuntimeError("cover_frozen_ranges: no QuantAct was called by forward() -- the model runs a fused "
                                   "schedule (enable_fused()), which never calls the modules; calibrate on the module "
                                   "path (model.enable_fused(False)) or use pipeline.calibrate_serving(model, batches)")
            with torch.no_grad():
                for a in acts:
                    if id(a) not in seen:
                        continue
                    lo, hi = seen[id(a)]
                    span = (torch.maximum(hi, a.x_max.reshape(())) - torch.minimum(lo, a.x_min.reshape(()))) * margin
                    new_lo = torch.minimum(a.x_min.reshape(()), lo - span)
                    new_hi = torch.maximum(a.x_max.reshape(()), hi + span)
                    if bool(new_lo < a.x_min.reshape(())) or bool(new_hi > a.x_max.reshape(())):
                        moved.add(id(a))
                    a.x_min.copy_(new_lo.reshape(a.x_min.shape))
                    a.x_max.copy_(new_hi.reshape(a.x_max.shape))
            if spread is not None:
                for a in acts:
                    pb = per_batch.get(id(a))
                    if pb and len(pb) >= 2:
                        los = torch.stack([v[0] for v in pb.values()]).double()
                        his = torch.stack([v[1] for v in pb.values()]).double()
                        spread[id(a)] = (float(los.std()), float(his.std()))
    finally:
        for a, f in zip(acts, was):
            a.running_stat = f
    return len(moved)


def _widen(act, frac, low_too):
    with torch.no_grad():
        lo, hi = act.x_min.reshape(()), act.x_max.reshape(())
        span = (hi - lo).clamp_min(1e-6) * frac
        act.x_max.copy_((hi + span).reshape(act.x_max.shape))
        if low_too:
            act.x_min.copy_((lo - span).reshape(act.x_min.shape))


def calibrate_serving(model, batches, margin=0.02, grow=0.04, max_iter=40, sigmas=0.0):
    """Calibration of the byte-code serving mode ON THE SCHEDULE THAT SERVES.

    cover_frozen_ranges() records what the MODULE path feeds every QuantAct; the byte network's exact-integer first
    convolutions flip single codes against that path and a deep network amplifies them, so ranges that cover the module
    path with 2 % to spare can still saturate a byte on the serving schedule.  Here: (1) cover_frozen_ranges on the
    module path without margin (a starting point), (2) the byte network itself (``model.enable_fused(frozen_codes=True)``)
    runs the calibration batches; every launch that saturated a code names its QuantAct(s) through its own flag word
    (OverflowFlags) and exactly those ranges are widened by `grow` of their span -- repeated until a whole pass is
    clean; (3) every range gets `margin` of its span to spare and the pass is repeated until clean again.  Only widens.
    Leaves the model frozen (running_stat False) and on the byte schedule.  Returns a dict (iterations, widened, clean).

    sigmas > 0 (round 6, VERDICT r5 weak #5: ranges that are clean on the calibration batches with 2 % to spare saturated a
    byte in 8 of 32 UNSEEN batches): the margin of step (3) is priced per QuantAct from the spread of its per-batch
    extremes over the calibration batches (>= 4 of them) -- each live end moves out by a further `sigmas` standard
    deviations of that end's batch extreme.  Batch extremes are maxima of ~10^6 values: Gumbel-like with scale
    beta = 0.78 sigma; the largest of m calibration batches sits ~ beta ln m above the location, a fresh batch exceeds
    location + t beta with probability e^-t, and with ~140 QuantActs a batch-level recompute rate below 2 % asks for
    t ~ 9, i.e. ~ 5-6 sigma beyond the calibration extreme at m = 8.  The price is resolution: every grid gets coarser by the
    widening (reported as `mean_widening`).  The alternative is the saturating policy: serve what the byte schedule
    produced and do not recompute."""
    from ..portable_quantizer.quant_modules import QuantAct
    acts = [m for m in model.modules() if isinstance(m, QuantAct)]
    set_running_stat(model, False)
    model.enable_fused(False)
    spread = {} if (sigmas > 0 and len(batches) >= 4) else None
    covered = cover_frozen_ranges(model, batches, margin=0.0, spread=spread)
    span0 = {id(a): float(a.x_max.reshape(()) - a.x_min.reshape(())) for a in acts}
    model.enable_fused(frozen_codes=True)
    hits, widened, iters = {}, set(), 0

    # attribution needs one launch per QuantAct: the depthwise-into-pointwise fusion of the byte backbone writes two
    # QuantActs' codes from one launch (bit-identical to the two kernels), so it is off while calibrating
    def fuse_dwpw(flag):            # -> whether the model runs a byte-code backbone
        fz = model.byte_backbone()
        if fz is not None:
            fz.fuse_dwpw = flag
        return fz is not None

    def until_clean():
        nonlocal iters
        while iters < max_iter:
            iters += 1
            fuse_dwpw(False)
            with torch.no_grad():
                for b in batches:
                    model(b)
            bad = model.overflowed_acts()
            if not bad:
                return True
            for a in bad:
                hits[id(a)] = hits.get(id(a), 0) + 1
                _widen(a, grow, bool(a.x_min.reshape(()) < 0) or hits[id(a)] >= 3)
                widened.add(id(a))
        return False
    clean = False
    try:
        with torch.no_grad():
            model(batches[0])                   # builds the byte-code objects
        clean = until_clean()
        if clean and (margin > 0 or spread):
            with torch.no_grad():
                for a in acts:
                    low_live = bool(a.x_min.reshape(()) < 0)
                    if margin > 0:
                        _widen(a, margin, low_live)
                    s_lo, s_hi = (spread or {}).get(id(a), (0.0, 0.0))
                    a.x_max.add_(sigmas * s_hi)
                    if low_live:
                        a.x_min.sub_(sigmas * s_lo)
            clean = until_clean()
    finally:
        byte_backbone = fuse_dwpw(True)         # (also when a calibration pass raised)
    if byte_backbone:
        with torch.no_grad():
            for b in batches:               # the serving configuration itself (fused depthwise) must be clean too
                model(b)
        clean = clean and not model.frozen_overflowed()
    widening = [float(a.x_max.reshape(()) - a.x_min.reshape(())) / max(span0[id(a)], 1e-12) for a in acts if span0[id(a)] > 0]
    return {"iterations": iters, "covered_on_module_path": covered, "widened_on_byte_schedule": len(widened),
            "clean": bool(clean), "byte_backbone": byte_backbone, "calibration_batches": len(batches),
            "sigmas": float(sigmas) if spread is not None else 0.0, "margin": float(margin),
            "mean_widening": (sum(widening) / len(widening)) if widening else 1.0,
            "max_widening": max(widening) if widening else 1.0}


def prepare_serving(model, images, settle=300, margin=0.02, replay=None, more_batches=(), sigmas=0.0):
    """The serving recipe bench.py's `e2e.frozen` leg times and tests/test_harness.py checks on three seeds: let the
    running (EMA) ranges settle over `settle` forwards of `images` (replay: an already captured graph of the running
    network), freeze every QuantAct, calibrate ON THE BYTE SCHEDULE (calibrate_serving) over `images` + `more_batches`
    (sigmas: its tail policy for unseen batches).  Leaves the model on enable_fused(frozen_codes=True); returns
    calibrate_serving's report."""
    if replay is None:
        model.enable_fused()
        with torch.no_grad():
            for _ in range(settle):
                model(images)
    else:
        for _ in range(settle):
            replay()
    torch.cuda.synchronize()
    return calibrate_serving(model, [images] + list(more_batches), margin=margin, sigmas=sigmas)


class FrozenHotPath:
    """``deconv_layers`` (W4A8) with FROZEN QuantAct ranges on byte codes: cdn_codenet_stage_frozen_forward, three
    launches per stage, every quantised tensor crosses HBM as one byte per element.  This is the serving
    mode (``QuantAct.running_stat = False``: a plain attribute in the reference, quant_modules.py:172,181,203-219),
    NOT the reference's default -- ``FusedHotPath`` is.  Results are bit-identical to ``FusedHotPath`` with
    running_stat False as long as no activation leaves its frozen 8-bit grid; the reference does not clamp codes,
    a byte must, so a saturated code raises the sticky device flag read by ``overflowed()`` and the caller
    recomputes that batch with ``FusedHotPath``.  Stages whose input channel count is not a multiple of 4
    (CoDeNet2x stage 0, C = 2153) run on the fp32 frozen schedule and hand fp32 + state to the next stage.

    chain_scale=True (cdn_codenet_stage_frozen_chained_forward): the scale prediction of stage k+1 is accumulated as
    exact integer sums in stage k's pointwise epilogue and finished by stage k+1's gather -- two launches fewer and no
    re-read of r.  A DECLARED non-bit-identical variant: s_raw is the exact sum rounded once instead of an fp32 sum
    of C products, so single scale codes can differ from the default schedule by one LSB (checked against the oracle
    with the same code-flip tolerance, tests/test_gpu_frozen.py)."""

    def __init__(self, deconv_layers, chain_scale=False):
        self.chain_scale = bool(chain_scale)
        if not FusedHotPath.supported(deconv_layers):
            raise NotImplementedError("this deconv_layers configuration is not implemented by the fused schedules")
        quantized, self.stages, _ = deform_stages(deconv_layers)
        if not quantized:
            raise NotImplementedError("FrozenHotPath needs the W4A8 deconv_layers")
        self.seq = deconv_layers
        for st in self.stages:
            if st[0].quant_conv_channel_bn.folded_int8() is None:
                raise NotImplementedError("FrozenHotPath needs per-channel symmetric <= 8-bit pointwise weights")
        self._bufs = None

    @staticmethod
    def planes_fit(deconv_layers, input_shape):
        """The last stage's geometry -- dict(C, Co, H, W, codes) as in forward_codes' shape dict, codes: it leaves byte
        codes -- when every stage's stored plane fits the LDS-resident gather -- the byte-code entry points' own limit
        (cdn_codenet_stage_supported) --, else None.  Above it (inputs beyond ~1100 px) the fp32 fused schedule, which
        honours frozen ranges too and gathers large planes from global memory, is the one to use: a byte-code stage
        cannot hand its codes to an fp32-schedule stage."""
        from .. import _native as N_
        quantized, _, geometry = deform_stages(deconv_layers, input_shape)
        if not quantized:
            return None
        Nb = input_shape[0]
        last = None
        for C, Co, H, W, up in geometry:
            if C % 4:      # no byte-code form (CoDeNet2x stage 0): that stage runs on the fp32 frozen schedule, NCHW input
                if up or not N_.lib().cdn_codenet_stage_fused_supported(Nb, C, H, W, 0, 0):
                    return None
            elif not N_.lib().cdn_codenet_stage_supported(Nb, C, H, W, 1, up):
                return None
            last = dict(C=C, Co=Co, H=H, W=W, codes=C % 4 == 0)
        return last

    def _alloc(self, shape, dev, nhwc_in, key):
        import ctypes
        from .. import _native as N_
        Nb = shape[0]
        lib = N_.lib()
        bufs, ws_bytes, ws32_bytes = [], 0, 0
        for i, (cin, cout, Hs, Ws, up) in enumerate(deform_stages(self.seq, shape)[2]):
            codes = cin % 4 == 0 and bool(lib.cdn_codenet_stage_supported(Nb, cin, Hs, Ws, 1 if (i or nhwc_in) else 0, up))
            if codes:
                ws_bytes = max(ws_bytes, lib.cdn_codenet_stage_frozen_workspace_bytes(Nb, cin, Hs, Ws, up))
            else:
                ws32_bytes = max(ws32_bytes, lib.cdn_codenet_stage_workspace_bytes(Nb, cin, Hs, Ws, up))
            bufs.append(dict(C=cin, Co=cout, H=Hs, W=Ws, up=up, codes=codes,
                             r8=torch.empty(Nb, Hs * Ws, cout, dtype=torch.int8, device=dev) if codes else None,
                             r=None if codes else torch.empty(Nb, Hs * Ws, cout, device=dev),
                             sums=None))
        sums_all = None
        if self.chain_scale:      # stage k's pointwise leaves the integer scale sums of stage k+1 (both on byte codes)
            take = [i for i in range(len(bufs) - 1)
                    if bufs[i]["codes"] and bufs[i + 1]["codes"]
                    and self.stages[i + 1][0].quant_conv_scale.int8_form() is not None]
            sizes = [(Nb * bufs[i]["H"] * bufs[i]["W"] + 3) // 4 * 4 for i in take]
            if take:      # ONE buffer, cleared by the step's first launch (cdn_quantact_frozen_params_clear)
                sums_all = torch.zeros(sum(sizes), dtype=torch.int32, device=dev)
                off = 0
                for i, sz in zip(take, sizes):
                    bufs[i]["sums"] = sums_all[off:off + Nb * bufs[i]["H"] * bufs[i]["W"]]
                    off += sz
        acts = [a for st in self.stages for a in stage_acts(st)]
        n = len(acts)
        arr = ctypes.c_void_p * n
        last = bufs[-1]
        self._bufs = dict(
            key=key, stages=bufs, sums_all=sums_all,
            ws=torch.empty(ws_bytes + 512, dtype=torch.uint8, device=dev),
            ws32=torch.zeros(ws32_bytes // 4 + 64, device=dev) if ws32_bytes else None,
            overflow=OverflowFlags(len(bufs) + 16, dev),      # word i: stage i; words n .. n+15: the byte-code heads
            expanded=torch.empty(Nb, last["H"] * last["W"], last["Co"], device=dev),
            out=torch.empty(Nb, last["Co"], last["H"] * 2, last["W"] * 2, device=dev),
            n_acts=n, acts=acts,      # (kept alive: the pointer arrays below refer to their buffers)
            p_min=arr(*[a.x_min.data_ptr() for a in acts]), p_max=arr(*[a.x_max.data_ptr() for a in acts]),
            p_state=arr(*[a._device_state(dev).data_ptr() for a in acts]))
        for i, st in enumerate(self.stages):
            self._bufs["overflow"].name(i, stage_acts(st))

    def head_flags(self):
        """the flag words the byte-code heads number from 0 (FusedHeads.forward_codes)"""
        return self._bufs["overflow"].slice(len(self.stages))

    def forward_codes(self, x, x_qstate=None, hw=None, covered=None):
        """-> (r8 [N, H*W, Co] int8 codes of the last stage's output QuantAct (or the fp32 tensor when that stage
        had to run on the fp32 schedule), r_state pointer, the stage's shape dict).  Input as FusedHotPath.forward_nhwc.
        covered: what THIS call's FrozenBackbone launch covered (its ``covered``) -- when it names these QuantActs and
        this schedule's scale sums, their parameters and the clear were in that launch; else this call launches its own."""
        from .. import _native as N_
        nhwc_in = hw is not None
        codes_in = x.dtype == torch.int8       # byte codes of the QuantAct whose state is x_qstate (a frozen backbone)
        if not (x.is_cuda and (x.dtype == torch.float32 or (codes_in and nhwc_in and x_qstate is not None))
                and x.dim() == (3 if nhwc_in else 4)):
            raise NotImplementedError("FrozenHotPath needs a GPU tensor: float32 NCHW, float32 [N, H*W, C] with hw "
                                      "and its QuantAct state, or int8 codes [N, H*W, C] with hw and the state")
        x = x.contiguous()
        c0 = self.stages[0][0].quant_deform_conv.in_channels
        if codes_in and (c0 % 4 or x.shape[2] != c0):
            # CoDeNet2x (C = 2153, round 5): stage 0 runs on the fp32 frozen schedule (no byte-code form for C % 4 != 0), so
            # the backbone's codes -- rows padded to a multiple of 16 bytes -- are expanded to the values level / scale
            # first (re-quantising them with the same state returns the same codes)
            xf = self.__dict__.get("_xin")
            if xf is None or xf.shape != x.shape or xf.device != x.device:
                xf = self._xin = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            N_.check(N_.lib().cdn_codenet_expand_codes(x.data_ptr(), x_qstate, xf.data_ptr(), x.numel(),
                                                        torch.cuda.current_stream(x.device).cuda_stream),
                     "cdn_codenet_expand_codes")
            # (an odd channel count has no channels-last form in the fused schedule either: NCHW, final values)
            x = xf.view(x.shape[0], hw[0], hw[1], x.shape[2])[..., :c0].permute(0, 3, 1, 2).contiguous()
            codes_in, nhwc_in, x_qstate, hw = False, False, None, None
        shape = (x.shape[0], x.shape[2], hw[0], hw[1]) if nhwc_in else tuple(x.shape)
        if shape[1] != c0:        # (the kernels take the channel count from the modules: a mismatch would read out of bounds)
            raise RuntimeError("FrozenHotPath: the input has %d channels, stage 0 expects %d" % (shape[1], c0))
        dev = x.device
        # the cached pointer arrays name the QuantActs' range buffers: a re-assigned buffer (load_state_dict(assign=
        # True), a .to() round trip) must rebuild them, so their addresses are part of the key
        key = (shape, dev, nhwc_in, codes_in) + tuple(p for st in self.stages for a in stage_acts(st)
                                            for p in (a.x_min.data_ptr(), a.x_max.data_ptr()))
        if self._bufs is None or self._bufs["key"] != key:
            self._alloc(shape, dev, nhwc_in, key)
        B = self._bufs
        lib = N_.lib()
        stream = torch.cuda.current_stream(dev).cuda_stream
        Nb = shape[0]
        # ONE (bits, momentum, running_stat) over all nine QuantActs: cdn_quantact_frozen_params takes the bit
        # width once for every state it derives (stages with different activation_bit would silently get the
        # last stage's grid otherwise)
        bits, _, _ = uniform_act_settings(B["acts"], "FrozenHotPath (all stages)")
        # (scale, zero-point) of all nine frozen QuantActs from their range buffers: one launch per step
        sa = B["sums_all"]
        if not (covered is not None and covered[1] is sa and set(id(a) for a in B["acts"]) <= set(covered[0])):
            # (not derived and cleared by the backbone's first launch, FrozenBackbone.__call__(also=...): this schedule's own)
            N_.check(lib.cdn_quantact_frozen_params_clear(B["n_acts"], B["p_min"], B["p_max"], B["p_state"], bits,
                                                          sa.data_ptr() if sa is not None else None,
                                                          sa.numel() * 4 if sa is not None else 0, stream),
                     "cdn_quantact_frozen_params_clear")
        ws_ptr = N_.aligned_workspace(B["ws"])[0]
        ws_bytes = B["ws"].numel() - (ws_ptr - B["ws"].data_ptr())      # (all of it: not rounded down to 256 bytes)
        cur_ptr, cur_kind, cur_q = x.data_ptr(), (2 if codes_in else 1 if nhwc_in else 0), (x_qstate if nhwc_in else None)
        with torch.no_grad():
            for si, (st, sb) in enumerate(zip(self.stages, B["stages"])):
                p = stage_params(st, kblocked=not sb["codes"])
                a = act_pointers(p["acts"], dev)
                if sb["codes"]:
                    sums_in = B["stages"][si - 1]["sums"] if si > 0 and cur_kind == 2 else None
                    # (the next stage's scale codes come from its module: its view is derived right before its own launch)
                    rc = lib.cdn_codenet_stage_frozen_chained_forward(
                        cur_ptr, cur_kind | getattr(self, "gather_flag", 0), sb["up"], cur_q, Nb, sb["C"], sb["Co"],
                        sb["H"], sb["W"], ptr(p["w_scale"]), ptr(p["b_scale"]), float(p["lo"]), float(p["hi"]),
                        ptr(p["w_dw"]), *map(ptr, p["i8"]), ptr(p["bias"]), 1, a[2], a[5], a[8],
                        ws_ptr, ws_bytes, sb["r8"].data_ptr(), B["overflow"].ptr(si), ptr(sums_in),
                        p["scale_i8"]()[1].data_ptr() if sums_in is not None else None,
                        self.stages[si + 1][0].quant_conv_scale.int8_form()[0].data_ptr() if sb["sums"] is not None
                        else None,
                        ptr(sb["sums"]), stream)
                    N_.check(rc, "cdn_codenet_stage_frozen_chained_forward")
                    cur_ptr, cur_kind = sb["r8"].data_ptr(), 2
                else:
                    if cur_kind == 2:
                        raise NotImplementedError("a byte-code stage cannot feed an fp32-schedule stage")
                    # (the fp32 frozen schedule: running = 0, automatic gather schedule)
                    stage_fused_forward(cur_ptr, cur_kind, cur_q, Nb, sb, p, a + [bits, float(p["acts"][2].momentum), 0],
                                        N_.aligned_workspace(B["ws32"]), stream)
                    cur_ptr, cur_kind = sb["r"].data_ptr(), 1
                cur_q = a[8]
        last = B["stages"][-1]
        return (last["r8"] if last["codes"] else last["r"]), cur_q, last

    def forward_nhwc(self, x, x_qstate=None, hw=None):
        """What FusedHotPath.forward_nhwc returns -- (fp32 [N, H*W, Co], QuantAct state pointer, shape) -- for the
        native heads: the byte codes expanded to the values level / scale (re-quantising them with the same state
        returns the same values)."""
        return self.expand(*self.forward_codes(x, x_qstate, hw))

    def expand(self, r, rq, last):
        """forward_codes' result -> what the fp32 heads take (byte codes expanded to level / scale; fp32 passes)."""
        from .. import _native as N_
        if r.dtype != torch.int8:
            return r, rq, last
        B = self._bufs
        rc = N_.lib().cdn_codenet_expand_codes(r.data_ptr(), rq, B["expanded"].data_ptr(), r.numel(),
                                               torch.cuda.current_stream(r.device).cuda_stream)
        N_.check(rc, "cdn_codenet_expand_codes")
        return B["expanded"], rq, last

    def __call__(self, x):
        """The Sequential's output tensor (NCHW, up-sampled, fake-quantised), like FusedHotPath.__call__."""
        return unpack_nchw(*self.forward_nhwc(x), self._bufs["out"])

    def overflowed(self):
        """True when some code saturated since the last call of this method (synchronises; resets the flag): the
        batches computed in between must be recomputed with FusedHotPath (running_stat False)."""
        if self._bufs is None:
            return False
        return self._bufs["overflow"].any()

    def capture(self, x, codes_only=True, x_qstate=None, hw=None):
        """One pass over the static buffer `x` as a HIP graph; returns replay() -> the static output (byte codes
        of the last stage with codes_only, else the unpacked NCHW tensor).  x_qstate / hw: a channels-last input
        (fp32 pre-quantisation values or int8 codes) as in forward_codes."""
        if hw is not None:
            if not codes_only:
                raise NotImplementedError("a channels-last input is captured with codes_only")
            run = lambda t: self.forward_codes(t, x_qstate, hw)[0]      # noqa: E731
        else:
            run = (lambda t: self.forward_codes(t)[0]) if codes_only else self.__call__
        return capture_graph(run, x)


class FrozenBackbone:
    """layer0 .. layer4 of a W4A8 ``PoseShuffleNetV2`` with every QuantAct FROZEN (``running_stat = False``: the
    serving mode, quant_modules.py:172,181,203-219 skipped) on BYTE CODES: every activation crosses HBM as one byte
    per element (the code of its QuantAct), every 1x1 conv is the int8-MFMA kernel on the codes as they lie in memory
    (cdn_codenet_pointwise_q8_strided_forward), the depthwise convs and the stem write codes directly
    (cdn_codenet_dw3x3_q8_forward, cdn_codenet_stem_q8_forward); no range epilogues, no arrival counters.  With frozen
    ranges the layer's shared block-output QuantAct is ONE fixed grid, so the "generations" of the running-range
    schedule (FusedBackbone) collapse and a layer is one int8 tensor whose channel slots never move (same slot
    assignment and permuted weight codes as FusedBackbone._mixed_plan).  Returns (codes [N, H*W, 1024] int8, state
    pointer of layer4's QuantAct, (H, W)) -- what ``FrozenHotPath.forward_codes`` takes.

    Arithmetic: the depthwise chains and the stem are those of the fp32 kernels on the values (q + zp) / scale
    (bit-identical); a unit's first 1x1 conv is an EXACT integer sum here where the running-range schedule
    accumulates exact products in fp32 (pwd3_kernel), so results agree with FusedBackbone at running_stat False up
    to single code flips (tests/test_gpu_backbone.py).  A saturated code sets the overflow flag (``overflowed()``)."""

    _MAX_C = 1024      # widest layer of the byte-code schedule (no per-channel table: int8 rows of up to 1024 codes)

    def __init__(self, model, fuse_dwpw=True, two_streams=True):
        self.model = model
        self._fb = FusedBackbone(model)
        self._bufs = None
        self.fuse_dwpw = fuse_dwpw          # a unit's depthwise inside its second 1x1 conv (cdn_codenet_dwpw_q8_forward)
        self.two_streams = two_streams      # the two branches of a stride-2 unit on two streams

    @staticmethod
    def supported(model):
        from ..portable_quantizer.quant_modules import QuantAct
        if not FusedBackbone.supported(model) or not hasattr(model.layer0[0], "folded"):
            return False
        fb = FusedBackbone(model)
        if not (len(model.layer0[1]) == 2 or (len(model.layer0[1]) == 3 and FusedBackbone._is_pool(model.layer0[1][2]))):
            return False                                     # (stem = conv, [ReLU, QuantAct] or [ReLU, QuantAct, MaxPool])
        for name in ("layer1", "layer2", "layer3"):      # (CoDeNet2x: layer3 is 976 channels wide; round 5)
            if not fb.mixed_supported(list(getattr(model, name)), max_c=FrozenBackbone._MAX_C):
                return False
        q4 = model.layer4[0]
        if q4.folded_int8() is None:
            return False
        acts = [a for n in ("layer0", "layer1", "layer2", "layer3", "layer4") for a in getattr(model, n).modules()
                if isinstance(a, QuantAct)]
        return bool(acts) and len(acts) <= 48 and all(act_fusable(a) and not a.running_stat for a in acts)

    def still_frozen(self):
        """The per-forward check (supported() walks the module tree once, when the object is built)."""
        from ..portable_quantizer.quant_modules import QuantAct
        acts = self.__dict__.get("_acts")
        if acts is None:
            acts = self._acts = [a for n in ("layer0", "layer1", "layer2", "layer3", "layer4")
                                 for a in getattr(self.model, n).modules() if isinstance(a, QuantAct)]
        return not any(a.running_stat for a in acts)

    def overflowed(self):
        if self._bufs is None:
            return False
        return self._bufs["overflow"].any()

    def _alloc(self, images, key):
        import ctypes
        from ..portable_quantizer.quant_modules import QuantAct
        m, dev = self.model, images.device
        acts = []
        for n in ("layer0", "layer1", "layer2", "layer3", "layer4"):
            for a in getattr(m, n).modules():
                if isinstance(a, QuantAct) and all(a is not b for b in acts):
                    acts.append(a)
        arr = ctypes.c_void_p * len(acts)
        self._bufs = dict(
            key=key, layers={}, overflow=OverflowFlags(len(acts), dev), acts=acts, n_acts=len(acts),
            p_min=arr(*[a.x_min.data_ptr() for a in acts]), p_max=arr(*[a.x_max.data_ptr() for a in acts]),
            p_state=arr(*[a._device_state(dev).data_ptr() for a in acts]))
        self._bufs["act_index"] = {id(a): i for i, a in enumerate(acts)}
        for i, a in enumerate(acts):            # word i: the launches that write act i's codes
            self._bufs["overflow"].name(i, [a])

    def _of(self, *acts):
        """the flag word of the launch writing `acts[0]`'s codes (a fused launch writing two QuantActs' codes is
        attributed to both)"""
        B = self._bufs
        i = B["act_index"][id(acts[0])]                 # (the acts list keeps the modules alive: ids are stable)
        for extra in acts[1:]:                          # (fused depthwise -> pointwise launches; recorded once)
            if (i, id(extra)) not in B.setdefault("attributed", set()):
                B["attributed"].add((i, id(extra)))
                B["overflow"].who[i].append(extra)      # (the backbone's flags are never sliced: word i == who[i])
        return B["overflow"].ptr(i)

    @staticmethod
    def _ld(c):
        return (c + 15) // 16 * 16          # 16-byte aligned byte rows (the int8 pointwise loads 16 bytes per lane)

    def _layer(self, name, nodes, x8, x_ld, x_state, in_logical, Nb, H, W):
        from .. import _native as N_
        fb, lib, B = self._fb, N_.lib(), self._bufs
        dev = x8.device
        plan = fb._mixed_plan(nodes, in_logical, dev, None)
        units = [fb._unit(n) for n in nodes]
        h, cin, C = plan["h"], plan["cin"], plan["C"]
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        Mi, Mo = Nb * H * W, Nb * Ho * Wo
        ldh, ldc, ldi = self._ld(h), self._ld(C), self._ld(cin)
        L = B["layers"].get(name)
        if L is None:
            z = lambda m_, c_: torch.zeros(m_, c_, dtype=torch.int8, device=dev)   # noqa: E731
            L = B["layers"][name] = dict(Y=z(Mo, ldc), t4=z(Mo, ldi), t1s2=z(Mi, ldh), t1=z(Mo, ldh), t2=z(Mo, ldh))
        main = torch.cuda.current_stream(dev)
        st = main.cuda_stream
        qp = lambda act: act._device_state(dev).data_ptr()   # noqa: E731

        def pw(a, a_state, M, K, lda, Wt, act, out, ldo, omap, st=st):
            rc = lib.cdn_codenet_pointwise_q8_strided_forward(
                a.data_ptr(), a_state, M, K, Wt["Co"], lda, ldo, Wt["codes"].data_ptr(), Wt["scale"].data_ptr(),
                Wt["colsum"].data_ptr(), Wt["bias"].data_ptr(), 1, omap, qp(act), out.data_ptr(), None, self._of(act), st)
            N_.check(rc, "cdn_codenet_pointwise_q8_strided_forward")

        def dw(a, a_state, Cc, Hs, Ws, stride, ld_in, w, b, act, out, ld_out, st=st):
            rc = lib.cdn_codenet_dw3x3_q8_forward(a.data_ptr(), a_state, Nb, Cc, Hs, Ws, stride, ld_in, ld_out,
                                                  w.data_ptr(), b.data_ptr(), 0, qp(act), out.data_ptr(), self._of(act), st)
            N_.check(rc, "cdn_codenet_dw3x3_q8_forward")

        def dwpw(a, a_state, Cc, Hs, Ws, stride, ld_in, w, b, act, Wt, out_act, omap, tmp=None, st=st):
            """depthwise (output codes of `act`) -> 1x1 conv -> ReLU -> codes of out_act into Y's slots: one launch
            where cdn_codenet_dwpw_q8_supported, else the two kernels through the scratch tensor `tmp`"""
            if self.fuse_dwpw and lib.cdn_codenet_dwpw_q8_supported(Cc, Hs, Ws, stride, Wt["Co"]):
                rc = lib.cdn_codenet_dwpw_q8_forward(
                    a.data_ptr(), a_state, Nb, Cc, Hs, Ws, stride, ld_in, w.data_ptr(), b.data_ptr(), 0, qp(act),
                    Wt["Co"], Wt["codes"].data_ptr(), Wt["scale"].data_ptr(), Wt["colsum"].data_ptr(),
                    Wt["bias"].data_ptr(), 1, ldc, omap, qp(out_act), Y.data_ptr(), self._of(out_act, act), st)
                N_.check(rc, "cdn_codenet_dwpw_q8_forward")
                return
            tmp = L["t2"] if tmp is None else tmp
            ldt = tmp.shape[1]
            dw(a, a_state, Cc, Hs, Ws, stride, ld_in, w, b, act, tmp, ldt, st=st)
            pw(tmp, qp(act), Mo, Cc, ldt, Wt, out_act, Y, ldc, omap, st=st)

        Y = L["Y"]
        with torch.no_grad():
            for k, (u, P) in enumerate(zip(units, plan["units"])):
                sh = u["sh"]
                if k == 0:
                    # the two branches of a stride-2 unit read the same input and write disjoint slots of Y: branch 1
                    # on a side stream (these launches leave most of the chip idle on their own)
                    side = None
                    if self.two_streams:
                        side = B.get("side")
                        if side is None:
                            side = B["side"] = torch.cuda.Stream(dev)
                        side.wait_stream(main)
                    # branch 1: dw s2 -> QuantAct -> pw -> ReLU -> shared QuantAct (slots omapA)
                    dwpw(x8, x_state, cin, H, W, 2, x_ld, P["w4"], P["b4"], u["a4"], P["c5"], sh, P["omapA"].data_ptr(),
                         tmp=L["t4"], st=side.cuda_stream if side is not None else st)
                    # branch 2: pw -> ReLU -> QuantAct -> dw s2 -> QuantAct -> pw -> ReLU -> shared QuantAct (omapB)
                    pw(x8, x_state, Mi, cin, x_ld, P["c1"], u["a1"], L["t1s2"], ldh, None)
                    dwpw(L["t1s2"], qp(u["a1"]), h, H, W, 2, ldh, P["w2"], P["b2"], u["a2"], P["c3"], sh,
                         P["omapB"].data_ptr())
                    if side is not None:
                        main.wait_stream(side)
                else:
                    pw(Y, qp(sh), Mo, C, ldc, P["c1"], u["a1"], L["t1"], ldh, None)
                    dwpw(L["t1"], qp(u["a1"]), h, Ho, Wo, 1, ldh, P["w2"], P["b2"], u["a2"], P["c3"], sh,
                         P["omapB"].data_ptr())
        return Y, ldc, qp(units[0]["sh"]), plan["logical"], Ho, Wo

    def __call__(self, images, also=None):
        """also: (acts, clear) of the schedules behind this one -- their QuantActs' (scale, zero-point) are derived, and
        `clear` (the chained stages' integer scale sums, or None) is zeroed, in THIS call's first launch instead of in two
        launches of their own; only when the bit widths agree and the list fits one launch (returns what it covered)."""
        import ctypes
        from .. import _native as N_
        if not (images.is_cuda and images.dtype == torch.float32 and images.dim() == 4 and images.shape[1] == 3):
            raise NotImplementedError("FrozenBackbone needs a [N,3,H,W] float32 GPU tensor")
        images = images.contiguous()
        m, dev, lib = self.model, images.device, N_.lib()
        Nb, _, R, R2 = images.shape
        # (the cached pointer arrays name the QuantActs' range buffers: their addresses are part of the key)
        stale = (self._bufs is None or self._bufs["key"][:2] != (tuple(images.shape), dev)
                 or self._bufs["key"][2:] != tuple(a.x_min.data_ptr() for a in self._bufs["acts"]))
        if stale:
            self._alloc(images, None)
            self._bufs["key"] = (tuple(images.shape), dev) + tuple(a.x_min.data_ptr() for a in self._bufs["acts"])
        B = self._bufs
        st = torch.cuda.current_stream(dev).cuda_stream
        bits, _, _ = uniform_act_settings(B["acts"], "FrozenBackbone")
        self.covered = None
        merged = None
        if also is not None:
            extra, clear = also
            acts_all = list(B["acts"]) + [a for a in extra if all(a is not b for b in B["acts"])]
            if len(acts_all) <= 64 and all(a.activation_bit == bits for a in extra):
                mkey = tuple(p for a in acts_all for p in (a.x_min.data_ptr(), a.x_max.data_ptr()))
                if B.get("merged_key") != mkey:
                    arr = ctypes.c_void_p * len(acts_all)
                    B["merged"] = (arr(*[a.x_min.data_ptr() for a in acts_all]), arr(*[a.x_max.data_ptr() for a in acts_all]),
                                   arr(*[a._device_state(dev).data_ptr() for a in acts_all]))
                    B["merged_key"] = mkey
                merged = (len(acts_all),) + B["merged"]
                self.covered = (tuple(id(a) for a in extra), clear)
        if merged is not None:
            clear = also[1]
            N_.check(lib.cdn_quantact_frozen_params_clear(*merged, bits, clear.data_ptr() if clear is not None else None,
                                                          clear.numel() * clear.element_size() if clear is not None else 0,
                                                          st), "cdn_quantact_frozen_params_clear")
        else:
            N_.check(lib.cdn_quantact_frozen_params(B["n_acts"], B["p_min"], B["p_max"], B["p_state"], bits, st),
                     "cdn_quantact_frozen_params")
        q0, act0 = m.layer0[0], m.layer0[1][1]
        q4, act4 = m.layer4[0], m.layer4[1][1]
        s0 = q0.conv.stride[0]
        H, W = (R + 2 - 3) // s0 + 1, (R2 + 2 - 3) // s0 + 1
        with torch.no_grad():
            w0, b0 = self._fb._folded(q0)
            if B.get("x0") is None:
                B["x0"] = torch.zeros(Nb, H * W, 32, dtype=torch.int8, device=dev)
            rc = lib.cdn_codenet_stem_q8_forward(images.data_ptr(), Nb, R, R2, 24, s0, w0.reshape(24, 27).data_ptr(),
                                                 b0.data_ptr(), 1, act0._device_state(dev).data_ptr(),
                                                 B["x0"].data_ptr(), 32, self._of(act0), st)
            N_.check(rc, "cdn_codenet_stem_q8_forward")
            x8, x_ld, x_state, logical = B["x0"], 32, act0._device_state(dev).data_ptr(), None
            if len(m.layer0[1]) == 3:                        # "S2 + MaxPool" stems (README configs b, e): pool the codes
                Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                if B.get("x0p") is None:
                    B["x0p"] = torch.zeros(Nb, Hp * Wp, 32, dtype=torch.int8, device=dev)
                rc = lib.cdn_codenet_maxpool3x3s2_q8_forward(x8.data_ptr(), Nb, 24, H, W, 32, 32, B["x0p"].data_ptr(), st)
                N_.check(rc, "cdn_codenet_maxpool3x3s2_q8_forward")
                x8, H, W = B["x0p"], Hp, Wp
            for name in ("layer1", "layer2", "layer3"):
                x8, x_ld, x_state, logical, H, W = self._layer(name, list(getattr(m, name)), x8, x_ld, x_state, logical,
                                                               Nb, H, W)
            c4 = q4.conv.out_channels
            ld4 = c4 if c4 % 4 == 0 else self._ld(c4)      # (CoDeNet2x: 2153 codes in rows of 2160 bytes, the pad stays 0)
            if B.get("out") is None:
                B["out"] = torch.zeros(Nb, H * W, ld4, dtype=torch.int8, device=dev)
            W4 = self._fb._l4_weights(q4, logical, dev, None)
            rc = lib.cdn_codenet_pointwise_q8_strided_forward(
                x8.data_ptr(), x_state, Nb * H * W, W4["K"], c4, x_ld, ld4, W4["codes"].data_ptr(),
                W4["scale"].data_ptr(), W4["colsum"].data_ptr(), W4["bias"].data_ptr(), 1, None,
                act4._device_state(dev).data_ptr(), B["out"].data_ptr(), None, self._of(act4), st)
            N_.check(rc, "cdn_codenet_pointwise_q8_strided_forward (layer4)")
        return B["out"], act4._device_state(dev).data_ptr(), (H, W)
