"""GPU parity of the one-channel depth stem (``ec_stem_conv1_depth``) and of the depth tower (``ec_rn50_forward_depth`` /
``RN50Trunk.forward_depth``) against torch-CPU references and the oracle.

Bounds: rel-L2 < 4e-3 against the fp32 conv (the bound ``test_stem_pool_layout_kernels`` uses for the RGB kernel: one bf16
rounding of inputs, weights and output); against a reference that rounds where the kernel's route rounds every element
within ``2^-7 max|ref|`` (one bf16 ulp at the top of the range) and fewer than 1 % of the elements different at all (the
rule of ``test_uint8_input_path_matches_normalised_fp32_path``); tower: the project's encoder tolerance (rel-L2 < 2e-2,
cosine > 0.999 against the fp32 oracle), < 1e-2 against the RGB tower on the three-channel expansion (same math, other
rounding points in the stem) and <= 7e-3 across launch shapes (``test_rn50_trunk_matches_oracle``).
"""
import pytest
import torch
import torch.nn.functional as F

from embodied_clip_amd import synthetic as syn
from oracle import clip_resnet as ocr

pytestmark = pytest.mark.gpu

SENTINEL = -7.0          # exactly representable in bf16; a ReLU output is never negative
GUARD = 2                # guard rows (of Wo * Cout elements) in front of and behind `out`


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _bfr(x):
    return x.to(torch.bfloat16).float()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _case(B, H, W, Cout, seed):
    from embodied_clip_amd.encoder import fold_stem_depth
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, generator=g)
    w = torch.randn(Cout, 3, 3, 3, generator=g) * 0.2          # [co, ci, ky, kx]: the three-channel stem conv
    b = torch.randn(Cout, generator=g) * 0.1
    w9 = fold_stem_depth(w.permute(2, 3, 1, 0).reshape(27, Cout).contiguous())      # [(ky,kx), co]
    return x, w, b, w9


def _run(dev, x, w9, b, Cout, scale=1.0, shift=0.0):
    """-> (out bf16 [B,Ho,Wo,Cout] on the host, the whole guarded buffer)."""
    from embodied_clip_amd import _lib
    lib = _lib.load()
    B, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    row = Wo * Cout
    buf = torch.full((GUARD * row + B * Ho * row + GUARD * row,), SENTINEL, dtype=torch.bfloat16, device=dev)
    out = buf[GUARD * row: GUARD * row + B * Ho * row]
    xd, wd, bd = x.to(dev).contiguous(), w9.to(dev).contiguous(), b.to(dev).contiguous()
    _lib.check(lib.ec_stem_conv1_depth(xd.data_ptr(), scale, shift, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, W, Cout,
                                       _lib.stream_ptr()), "ec_stem_conv1_depth")
    torch.cuda.synchronize()
    return out.cpu().view(B, Ho, Wo, Cout), buf.cpu()


def _conv1(x_b1hw, w9, b):
    Cout = w9.shape[1]
    return F.relu(F.conv2d(x_b1hw, w9.t().reshape(Cout, 1, 3, 3), b, stride=2, padding=1)).permute(0, 2, 3, 1)


# (2,34,34,32): two tiles per axis, ragged last tile, vector staging, MFMA; (2,30,38,64): W % 4 != 0 -> scalar staging,
# non-square, two channel blocks; (3,33,31,48): odd sizes, the fp32 route
@pytest.mark.parametrize("B,H,W,Cout", [(2, 34, 34, 32), (2, 30, 38, 64), (3, 33, 31, 48)])
def test_depth_stem_matches_the_three_channel_conv(dev, B, H, W, Cout):
    x, w, b, w9 = _case(B, H, W, Cout, 3)
    got, buf = _run(dev, x, w9, b, Cout)
    # (a) upstream's arithmetic in fp32: the frame repeated to three channels through the three-channel conv
    ref = F.relu(F.conv2d(x[:, None].repeat(1, 3, 1, 1), w, b, stride=2, padding=1)).permute(0, 2, 3, 1)
    r = _rel(got, ref)
    print(f"depth stem {(B, H, W, Cout)}: rel-L2 vs fp32 three-channel conv = {r:.3e}")
    assert got.shape == ref.shape
    assert r < 4e-3, r
    # (b) a reference that rounds where the route rounds: bf16 window values and weights on the MFMA route, fp32 on the
    # other; fp32 accumulation, bf16 output
    mfma = Cout % 32 == 0
    ref_r = _bfr(_conv1(_bfr(x[:, None]) if mfma else x[:, None], _bfr(w9) if mfma else w9, b))
    d = (got.float() - ref_r).abs()
    frac = (d > 0).float().mean().item()
    print(f"  vs same-rounding reference: max|d| = {d.max().item():.3e} (bound {2 ** -7 * ref_r.abs().max().item():.3e}), differing {frac:.4%}")
    assert d.max().item() <= 2 ** -7 * ref_r.abs().max().item()
    assert frac < 0.01, frac
    # (c) canary: the guard rows in front of and behind `out` are untouched
    row = ((W - 1) // 2 + 1) * Cout
    assert torch.all(buf[:GUARD * row] == SENTINEL) and torch.all(buf[-GUARD * row:] == SENTINEL)
    assert torch.all(got >= 0)


def test_depth_stem_pads_after_the_affine(dev):
    """value = depth * scale + shift inside the frame, exactly zero in the padding: the conv of the NORMALISED frame padded
    with zeros.  (Padding the raw frame and normalising afterwards puts `shift` into the border windows.)"""
    B, H, W, Cout = 2, 34, 34, 32
    x, w, b, w9 = _case(B, H, W, Cout, 5)
    scale, shift = 4.0, -2.0
    got, _ = _run(dev, x, w9, b, Cout, scale, shift)
    ref = _conv1((x * scale + shift)[:, None], w9, b)
    wrong = F.relu(F.conv2d(F.pad(x[:, None], (1, 1, 1, 1)) * scale + shift, w9.t().reshape(Cout, 1, 3, 3), b, stride=2)).permute(0, 2, 3, 1)
    r = _rel(got, ref)
    print(f"fused affine: rel-L2 vs fp32 conv of the normalised frame = {r:.3e}; a pad-then-normalise kernel would be at {_rel(wrong, ref):.3e}")
    assert r < 4e-3, r


# ---- tower ---------------------------------------------------------------------------------------------------------------
_TOWERS = {}


def _tower(dev, key):
    """(state dict, trunk, depth frames [B,R,R,1] normalised, depth features on the host, oracle features) -- built once."""
    if key not in _TOWERS:
        from embodied_clip_amd.encoder import RN50Trunk
        (width, layers, res, B) = key
        sd = (syn.rn50_visual_state_dict(11, width=width, layers=layers, output_dim=64, heads=4, input_resolution=res)
              if res != 224 else syn.rn50_visual_state_dict(0))
        trunk = RN50Trunk(sd, device=dev, input_resolution=res)
        depth = syn.normalize_depth(syn.synthetic_depth(1005, B, res))
        feat = trunk.forward_depth(depth.to(dev))
        got = trunk.to_nchw_f32(feat).cpu()
        ref = ocr.clip_resnet_preprocessor(depth, sd)
        _TOWERS[key] = (sd, trunk, depth, feat, got, ref)
    return _TOWERS[key]


TOWER_KEYS = [(64, (1, 1, 1, 1), 64, 3), (64, (3, 4, 6, 3), 224, 2)]


@pytest.mark.parametrize("key", TOWER_KEYS)
def test_depth_tower_matches_oracle(dev, key):
    sd, trunk, depth, feat, got, ref = _tower(dev, key)
    assert got.shape == ref.shape
    r = _rel(got, ref)
    cos = F.cosine_similarity(got.flatten(1), ref.flatten(1)).min().item()
    print(f"depth tower {key}: rel-L2 vs fp32 oracle = {r:.3e}, cosine = {cos:.6f}")
    assert r < 2e-2, r
    assert cos > 0.999, cos


@pytest.mark.parametrize("key", TOWER_KEYS)
def test_depth_tower_matches_the_rgb_tower_on_the_expanded_frame(dev, key):
    sd, trunk, depth, feat, got, ref = _tower(dev, key)
    rgb3 = depth.to(dev).expand(-1, -1, -1, 3).contiguous()
    feat3 = trunk.forward(rgb3)
    r = _rel(feat.cpu(), feat3.cpu())
    print(f"depth tower {key}: rel-L2 vs RGB tower on the three-channel expansion = {r:.3e}")
    assert r < 1e-2, r
    # [B,R,R] is the same input as [B,R,R,1]; `out=` is written in place
    out = torch.empty_like(feat)
    assert trunk.forward_depth(depth.to(dev).squeeze(-1).contiguous(), out=out) is out
    assert torch.equal(out.cpu(), feat.cpu())


@pytest.mark.parametrize("key,chunk", [(TOWER_KEYS[0], 2), (TOWER_KEYS[1], 1)])
def test_depth_tower_chunked_matches_unchunked(dev, key, chunk):
    """Sub-batches read their frames at the ONE-channel stride (a three-channel stride reads the wrong frame in the second
    chunk): the same features up to the fp32-accumulation differences between launch shapes."""
    sd, trunk, depth, feat, got, ref = _tower(dev, key)
    trunk.chunk = chunk
    try:
        featc = trunk.forward_depth(depth.to(dev))
    finally:
        trunk.chunk = 0
    r = _rel(featc.cpu(), feat.cpu())
    print(f"depth tower {key}: chunk {chunk} vs unchunked rel-L2 = {r:.3e}")
    assert r <= 7e-3, r


def test_depth_tower_fused_normalisation(dev):
    """``forward_depth(raw, scale, shift)`` == ``forward_depth(normalize_depth(raw))`` up to the fp32 rounding of the affine."""
    key = TOWER_KEYS[0]
    sd, trunk, depth, feat, got, ref = _tower(dev, key)
    raw = syn.synthetic_depth(1005, key[3], key[2]).to(dev)
    f2 = trunk.forward_depth(raw, scale=1.0 / syn.DEPTH_STD, shift=-syn.DEPTH_MEAN / syn.DEPTH_STD)
    assert _rel(f2.cpu(), feat.cpu()) < 1e-2


def test_torchvision_stem_handle_is_unsupported(dev):
    from embodied_clip_amd import _lib
    from embodied_clip_amd.encoder import ImageNetRN50Trunk
    sd = syn.tv_resnet_state_dict(5, layers=(1, 1, 1, 1))
    trunk = ImageNetRN50Trunk(sd, device=dev, input_resolution=64)
    assert trunk.stem_w9 is None
    depth = torch.zeros(1, 64, 64, device=dev)
    w9 = torch.zeros(9, 64, device=dev)
    ws = trunk._workspace(1)
    out = torch.empty(1, trunk.out_spatial, trunk.out_spatial, trunk.out_channels, dtype=torch.bfloat16, device=dev)
    rc = trunk.lib.ec_rn50_forward_depth(trunk.h, depth.data_ptr(), 1.0, 0.0, w9.data_ptr(), 1, ws.data_ptr(), ws.numel(),
                                         out.data_ptr(), 0, _lib.stream_ptr())
    assert rc == -6, rc          # EC_ERR_UNSUPPORTED
    with pytest.raises(_lib.EcError):
        trunk.forward_depth(depth)
