"""The streaming int8 pointwise kernel (pwi8s_kernel) on its ring of two windows per wave: results against the tile
kernel at the shapes where the ring, its prologue and its peeled last step can go wrong, the register / scratch budget that
makes four workgroups per CU possible, and the residency the runtime reports for it."""
import copy
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "build", "asm", "codenet_pointwise-hip-amdgcn-amd-amdhsa-gfx950.s")

# K at stage 0: 512 -- two windows per wave: the prologue runs straight into the last two steps, the loop is empty;
# 576, 640 -- 9 / 10 window pairs on four waves: uneven; 1024 -- CoDeNet1x; 2153 -- padded to 2176, 17 pairs.
# Co at stage 0: 32, 64 -- the two-tile instantiation; 100 -- ragged columns (zero rows of the k-blocked copy);
# 256 -- two column groups.  Planes 4 x 4 and 6 x 6 with 3 images: M = 48 and 108, one partial 32-row block each.
# Every K meets Co = 256 and Co = 100, the shortest and the longest K meet every Co, and every K and Co meet both planes.
CASES = [(512, 32, 4), (512, 64, 6), (512, 100, 4), (512, 256, 6),
         (576, 100, 6), (576, 256, 4),
         (640, 64, 4), (640, 100, 4), (640, 256, 6),
         (1024, 32, 6), (1024, 100, 6), (1024, 256, 4),
         (2153, 32, 4), (2153, 64, 6), (2153, 100, 4), (2153, 256, 6)]


def _same(a, b):
    """bitwise-equal values, NaN at the same places"""
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("K,Co,hw", CASES)
def test_small_ring_matches_the_tile_kernel(K, Co, hw):
    """FusedHotPath with and without the k-blocked weight codes (pwi8s_kernel against pwi8_kernel at stage 0): every
    stage's r, the final tensor and all x_min / x_max are EQUAL over 4 batches with running ranges (the first take the
    wide-code f32 branch, later ones the int8 path), and equal with NaN at the same places for a fifth batch that has a
    NaN in its input."""
    from codenet_amd import pipeline
    planes = [K, Co, 16 if Co == 32 else 32]
    net_a = pipeline.build_hot_path(quantized=True, planes=planes, seed=K + Co + hw).cuda()
    net_b = copy.deepcopy(net_a)
    for n in (net_a, net_b):
        pipeline.set_running_stat(n, True)
    fa = pipeline.FusedHotPath(net_a.deconv_layers, kblocked_codes=True)
    fb = pipeline.FusedHotPath(net_b.deconv_layers, kblocked_codes=False)
    used = []
    fa.stage_hook = lambda sb: used.append(fa._stage_params(fa.stages[0])["kb_flag"])
    g = torch.Generator().manual_seed(K + hw)
    for it in range(5):
        x = torch.randn(3, K, hw, hw, generator=g) * (1.0 + 0.3 * it)
        if it == 4:
            x[1, 3, 2, 2] = float("nan")
        x = x.cuda()
        ya, yb = fa(x).clone(), fb(x).clone()
        assert _same(ya, yb), "batch %d: outputs differ" % it
        for ba, bb in zip(fa._bufs["stages"], fb._bufs["stages"]):
            assert _same(ba["r"], bb["r"]), "batch %d: stage output %dx%d differs" % (it, ba["H"], ba["W"])
        rb = net_b.state_dict()
        nrng = 0
        for k, v in net_a.state_dict().items():
            if k.endswith(("x_min", "x_max")):
                assert _same(v, rb[k]), "batch %d: range %s differs" % (it, k)
                nrng += 1
        assert nrng >= 2
        if it < 4:
            assert not torch.isnan(ya).any()
        else:
            assert torch.isnan(ya).any()      # the NaN reached the output through both kernels
    assert used and used[0] == pipeline.WCODES_KB       # the k-blocked form was in use for stage 0


def _kernel_metadata(text, needle):
    """{kernel name: {key: int}} from the .amdgpu_metadata of a device assembly file, for names that contain needle"""
    out = {}
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target|\Z)", text, re.S | re.M):
        blk = m.group(0)
        name = re.search(r"^\s+\.name:\s+(\S+)", blk, re.M)
        if not name or needle not in name.group(1):
            continue
        out[name.group(1)] = {k: int(v) for k, v in re.findall(r"^\s+-?\s*\.(\w+):\s+(\d+)\s*$", blk, re.M)}
    return out


@pytest.mark.skipif(not os.path.exists(ASM), reason="the device assembly of codenet_pointwise.hip has not been kept")
def test_both_instantiations_fit_four_workgroups_per_cu():
    """Four 256-thread workgroups per CU are four waves per SIMD: at most 128 registers (VGPR + AGPR), and nothing in
    scratch -- a spill store inside the k loop would also be one more count behind every s_waitcnt vmcnt."""
    meta = _kernel_metadata(open(ASM).read(), "pwi8s_kernel")
    assert len(meta) == 2 and any("pwi8s_kernelILi2E" in n for n in meta) \
        and any("pwi8s_kernelILi4E" in n for n in meta), sorted(meta)
    for name, md in meta.items():
        assert md["vgpr_count"] <= 128, (name, md["vgpr_count"])
        assert md["vgpr_spill_count"] == 0, (name, md["vgpr_spill_count"])
        assert md["private_segment_fixed_size"] == 0, (name, md["private_segment_fixed_size"])


@pytest.mark.gpu
@pytest.mark.parametrize("Co", [64, 128, 256])
def test_runtime_keeps_four_workgroups_per_cu_resident(Co):
    from codenet_amd import _native
    assert _native.lib().cdn_codenet_pwi8s_resident_workgroups(Co) >= 4
