"""Argument checks of the depth entry points (``ec_stem_conv1_depth``, ``ec_rn50_forward_depth``): they come before any HIP
call, so they are checked here without a GPU."""
from embodied_clip_amd import _lib

EC_ERR_ARG, EC_ERR_SHAPE = -1, -2
P = 0x1000          # a non-NULL pointer that is never dereferenced: every call below is refused first


def test_stem_conv1_depth_refuses_null_pointers():
    lib = _lib.load()
    for args in ((0, P, P, P), (P, 0, P, P), (P, P, 0, P), (P, P, P, 0)):
        depth, w9, bias, out = args
        assert lib.ec_stem_conv1_depth(depth, 1.0, 0.0, w9, bias, out, 2, 34, 34, 32, 0) == EC_ERR_ARG


def test_stem_conv1_depth_refuses_other_channel_counts_and_degenerate_frames():
    lib = _lib.load()
    assert lib.ec_stem_conv1_depth(P, 1.0, 0.0, P, P, P, 2, 34, 34, 40, 0) == EC_ERR_SHAPE
    assert lib.ec_stem_conv1_depth(P, 1.0, 0.0, P, P, P, 2, 1, 34, 32, 0) == EC_ERR_SHAPE
    assert lib.ec_stem_conv1_depth(P, 1.0, 0.0, P, P, P, 2, 34, 1, 32, 0) == EC_ERR_SHAPE
    assert lib.ec_stem_conv1_depth(P, 1.0, 0.0, P, P, P, 0, 34, 34, 32, 0) == EC_ERR_SHAPE


def test_rn50_forward_depth_refuses_null_pointers():
    lib = _lib.load()
    # (handle, depth, stem_w9, workspace, feat)
    for args in ((0, P, P, P, P), (P, 0, P, P, P), (P, P, 0, P, P), (P, P, P, 0, P), (P, P, P, P, 0)):
        h, depth, w9, ws, feat = args
        assert lib.ec_rn50_forward_depth(h, depth, 1.0, 0.0, w9, 2, ws, 1 << 20, feat, 0, 0) == EC_ERR_ARG


def test_version_counts_the_depth_entry_points():
    assert _lib.load().ec_version() >= 620
