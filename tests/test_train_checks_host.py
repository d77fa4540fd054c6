"""The entry points of the QAT step that take a tracked QuantAct or a workspace validate them alike (cdn_common.h:
tracked_qupdate, check_workspace), before any launch: no GPU needed."""
import pytest

P = 4096      # a non-null, 16-byte aligned address that nothing dereferences: every call below fails its validation
ACT = dict(x_min=P, x_max=P, state=P, counters=P, bits=8, momentum=0.99, running=1, state_copy=P)


def _act(a):
    return (a["x_min"], a["x_max"], a["state"], a["counters"], a["bits"], a["momentum"], a["running"], a["state_copy"])


# name -> (call(lib, act or (workspace, bytes)), workspace size or None); shapes as small as the entry points allow
FORWARDS = {
    "cdn_codenet_head_dw_forward": lambda lib, a: lib.cdn_codenet_head_dw_forward(P, P, P, P, P, 1, 4, 8, 8, *_act(a), None),
    "cdn_codenet_unit_dw_forward": lambda lib, a: lib.cdn_codenet_unit_dw_forward(P, 4 * 64, P, P, P, P, 1, 4, 8, 8, 1,
                                                                                 *_act(a), None),
    "cdn_codenet_stem_train_forward": lambda lib, a: lib.cdn_codenet_stem_train_forward(P, P, P, P, 1, 8, 8, 24, 4,
                                                                                       *_act(a), None),
}
BACKWARDS = {
    "cdn_codenet_head_dw_backward": (
        lambda lib, ws, n: lib.cdn_codenet_head_dw_backward(P, None, 0, P, P, P, P, P, 4 * 64, P, P, 1, 4, 8, 8, ws, n, None),
        lambda lib: lib.cdn_codenet_head_dw_backward_workspace_bytes(1, 4, 8, 8)),
    "cdn_codenet_unit_dw_backward": (
        lambda lib, ws, n: lib.cdn_codenet_unit_dw_backward(P, P, 4 * 64, P, P, P, 4 * 64, 0, P, P, 1, 4, 8, 8, 1, ws, n, None),
        lambda lib: lib.cdn_codenet_unit_dw_backward_workspace_bytes(1, 4, 8, 8, 1)),
    "cdn_codenet_stem_backward": (
        lambda lib, ws, n: lib.cdn_codenet_stem_backward(P, P, P, P, P, 1, 8, 8, 24, 4, ws, n, None),
        lambda lib: lib.cdn_codenet_stem_backward_workspace_bytes(1, 8, 8, 4)),
    "cdn_codenet_pointwise_wgrad": (
        lambda lib, ws, n: lib.cdn_codenet_pointwise_wgrad(P, P, P, P, 1, 4, 4, 64, ws, n, None),
        lambda lib: lib.cdn_codenet_pointwise_wgrad_workspace_bytes(1, 4, 4, 64)),
}
ARG, WORKSPACE = -1, -6      # CDN_ERR_ARG, CDN_ERR_WORKSPACE


@pytest.mark.parametrize("entry", sorted(FORWARDS) + sorted(BACKWARDS))
def test_tracked_quantact_and_workspace_are_validated_alike(entry):
    from codenet_amd import _native
    lib = _native.lib()
    if entry in FORWARDS:
        call = FORWARDS[entry]
        for missing in ("counters", "x_min", "x_max", "state"):
            assert call(lib, dict(ACT, **{missing: None})) == ARG, missing
            assert "null QuantAct pointer" in _native.last_error()
        for bits in (1, 17):
            assert call(lib, dict(ACT, bits=bits)) == ARG, bits
            assert "bits must be in [2,16], got %d" % bits in _native.last_error()
    else:
        call, size = BACKWARDS[entry]
        need = size(lib)
        assert need > 0 and need % 256 == 0
        assert call(lib, P, need - 1) == WORKSPACE                 # one byte short
        assert "workspace too small or not 16-byte aligned" in _native.last_error()
        assert call(lib, P + 4, need) == WORKSPACE                 # an address that is 4 mod 16
        assert "workspace too small or not 16-byte aligned" in _native.last_error()
        assert call(lib, P + 4, need + 16) == WORKSPACE
        assert call(lib, None, need) == ARG                        # (a missing workspace is a null pointer, not a size)
