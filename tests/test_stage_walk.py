"""Host-side pieces shared by the fused stage schedules: the stage walk over a deconv_layers Sequential and the aligned
workspace of a library call -- no GPU."""
import pytest
import torch
import torch.nn as nn

from codenet_amd import _native, pipeline


@pytest.mark.parametrize("quantized", [True, False])
def test_stage_walk_splits_and_doubles_the_plane(quantized):
    net = pipeline.build_hot_path(w2=True, quantized=quantized)
    q, stages, geometry = pipeline.hotpath.deform_stages(net.deconv_layers, (2, 2153, 16, 16))
    assert q == quantized and [len(st) for st in stages] == [3 if quantized else 4] * 3
    assert geometry == [(2153, 256, 16, 16, 0), (256, 128, 32, 32, 1), (128, 64, 64, 64, 1)]
    assert pipeline.hotpath.deform_stages(net.deconv_layers)[2] is None


def test_stage_walk_rejects_what_the_fused_schedules_do_not_implement():
    mods = list(pipeline.build_hot_path(quantized=True).deconv_layers)
    up3 = mods[:-1] + [nn.Upsample(scale_factor=3)]
    for seq in (nn.Sequential(), nn.Sequential(*mods[:-1]), nn.Sequential(*up3)):
        with pytest.raises(NotImplementedError):
            pipeline.hotpath.deform_stages(seq)
        assert not pipeline.FusedHotPath.supported(seq)
        with pytest.raises(NotImplementedError):
            pipeline.FusedHotPath(seq)


def test_frozen_planes_fit_runs_a_c2153_stage0_on_the_fp32_schedule():
    net = pipeline.build_hot_path(w2=True, quantized=True)
    assert pipeline.FrozenHotPath.planes_fit(net.deconv_layers, (2, 2153, 16, 16)) == dict(
        C=128, Co=64, H=64, W=64, codes=True)
    assert pipeline.FrozenHotPath.planes_fit(pipeline.build_hot_path(quantized=False).deconv_layers,
                                             (2, 1024, 16, 16)) is None


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_aligned_workspace_stays_inside_the_tensor(dtype):
    for n in (1000, 1023, 4099):
        t = torch.empty(n, dtype=dtype)
        p, nbytes = _native.aligned_workspace(t)
        end = t.data_ptr() + t.numel() * t.element_size()
        assert p % 256 == 0 and t.data_ptr() <= p < t.data_ptr() + 256 and nbytes % 256 == 0
        assert 0 <= end - p - nbytes < 256
