"""GPU checks of the pooled net's RGB-D encoder: ``ec_spatial_mean_pair_bf16`` against float64 of its bf16 inputs, and the joint
pass ``ec_rn50_embed_rgbd`` / ``RN50Trunk.embed_rgbd`` against the entry points it replaces and against the fp32 oracle.

Bounds.  Pair kernel: ``|got - ref| <= (2 HW + 2) 2^-24 (sum_hw |a| + |b|) / HW`` per element -- the recursive-summation bound
for ``2 HW`` fp32 terms plus the division; it holds for any summation order, so it carries no measured margin.  Joint pass:
rel-L2 <= 7e-3 against the same maps from other launch shapes (the project's bound across launch shapes,
``test_depth_tower_chunked_matches_unchunked``), the encoder tolerance (rel-L2 < 2e-2, cosine > 0.999) against the fp32 oracle,
< 1e-2 for uint8 against host-normalised fp32 frames (``test_uint8_input_path_matches_normalised_fp32_path``), and no tolerance
at all for the pairing: a changed frame changes its own row and no other."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from _child import GPU
from embodied_clip_amd import synthetic as syn
from oracle import clip_resnet as ocr

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 2                # guard rows (of C floats) in front of and behind `out`
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


# ---- the pair kernel ------------------------------------------------------------------------------------------------------------
def _pair(dev, a, b):
    """a, b: device bf16 [B, HW, C] views -> (out f32 [B, C] on the host, the guarded buffer on the host)"""
    from embodied_clip_amd import _lib
    lib = _lib.load()
    B, HW, Cc = a.shape
    buf = torch.full(((B + 2 * GUARD) * Cc,), SENTINEL, dtype=torch.float32, device=dev)
    out = buf[GUARD * Cc:(GUARD + B) * Cc]
    _lib.check(lib.ec_spatial_mean_pair_bf16(a.data_ptr(), b.data_ptr(), out.data_ptr(), B, HW, Cc, _lib.stream_ptr()), "ec_spatial_mean_pair_bf16")
    torch.cuda.synchronize()
    return out.cpu().view(B, Cc), buf.cpu()


# (3,49,64): one slab, 8 of its 32 column groups; (2,7,40): vector loads, C no multiple of 64, fewer pixels than row parts;
# (1,1,3), (2,5,13): the scalar route; (4,49,2048): the real row, 8 slabs per pair; offset: C % 8 == 0 but `a` starts one element
# off the 16-byte grid, so the aligned route must not be taken
@pytest.mark.parametrize("B,HW,Cc,offset", [(3, 49, 64, 0), (2, 7, 40, 0), (1, 1, 3, 0), (2, 5, 13, 0), (4, 49, 2048, 0), (3, 49, 64, 1)])
def test_pair_kernel_against_float64(dev, B, HW, Cc, offset):
    g = torch.Generator().manual_seed(7 * B + HW + Cc)
    n = B * HW * Cc
    sa = (torch.randn(n + 8, generator=g) * 2).to(torch.bfloat16).to(dev)
    sb = (torch.rand(n + 8, generator=g) * 3 - 1).to(torch.bfloat16).to(dev)
    a, b = sa[offset:offset + n].view(B, HW, Cc), sb[:n].view(B, HW, Cc)
    assert a.data_ptr() % 16 == (2 * offset) % 16 and b.data_ptr() % 16 == 0
    a64, b64 = a.cpu().double(), b.cpu().double()
    ref = (a64 + b64).sum(1) / HW
    bound = (2 * HW + 2) * 2.0 ** -24 * (a64.abs() + b64.abs()).sum(1) / HW
    got, buf = _pair(dev, a, b)
    err = (got.double() - ref).abs()
    print(f"pair kernel {(B, HW, Cc, offset)}: max |err| / bound = {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert torch.all(err <= bound)
    assert torch.all(buf[:GUARD * Cc] == SENTINEL) and torch.all(buf[-GUARD * Cc:] == SENTINEL)      # guard rows untouched
    again, _ = _pair(dev, a, b)
    assert torch.equal(again, got)                                                                   # two calls: equal bits
    if offset == 0:
        swapped, _ = _pair(dev, b, a)
        assert torch.all((swapped.double() - ref).abs() <= bound)


# ---- the joint pass -------------------------------------------------------------------------------------------------------------
_CASES = {}


def _case(dev, key):
    """(sd, trunk, rgb, depth on the host, embedding at chunk 0 on the host, float64 composed reference, oracle reference): built once"""
    if key not in _CASES:
        from embodied_clip_amd.encoder import RN50Trunk
        res, B = key
        sd = (syn.rn50_visual_state_dict(11, width=64, layers=(1, 1, 1, 1), output_dim=64, heads=4, input_resolution=res)
              if res != 224 else syn.rn50_visual_state_dict(0))
        trunk = RN50Trunk(sd, device=dev, input_resolution=res)
        rgb = syn.synthetic_rgb(1000, B, res)
        depth = syn.normalize_depth(syn.synthetic_depth(1005, B, res))
        got = trunk.embed_rgbd(rgb.to(dev), depth.to(dev)).cpu()
        # the composed reference, from entry points this encoder replaces: the two maps, pooled in float64
        fa, fb = trunk.forward(rgb.to(dev)).cpu().double(), trunk.forward_depth(depth.to(dev)).cpu().double()
        composed = (fa + fb).flatten(1, 2).mean(1)
        oracle = (ocr.clip_resnet_preprocessor(rgb, sd) + ocr.clip_resnet_preprocessor(depth, sd)).double().flatten(2).mean(2)
        _CASES[key] = (sd, trunk, rgb, depth, got, composed, oracle)
    return _CASES[key]


SMALL, REAL = (64, 5), (224, 2)


@pytest.mark.parametrize("key", [SMALL, REAL])
def test_joint_pass_matches_the_composed_entry_points_and_the_oracle(dev, key):
    sd, trunk, rgb, depth, got, composed, oracle = _case(dev, key)
    assert got.shape == composed.shape == oracle.shape == (key[1], trunk.out_channels) and got.dtype == torch.float32
    r = _rel(got, composed)
    ro = _rel(got, oracle)
    cos = F.cosine_similarity(got.double(), oracle).min().item()
    print(f"embed_rgbd {key}: rel-L2 vs forward + forward_depth pooled in float64 = {r:.3e}; vs fp32 oracle = {ro:.3e}, cosine = {cos:.6f}")
    assert r <= 7e-3, r
    assert ro < 2e-2, ro
    assert cos > 0.999, cos


@pytest.mark.parametrize("chunk", [0, 2])
def test_pairing(dev, chunk):
    """embedding row j is a function of RGB frame j and depth frame j alone: no tolerance.  chunk 2: chunks of 2, 2, 1 pairs --
    j = 3 sits in the second chunk, j = 4 in the ragged one"""
    sd, trunk, rgb, depth, got0, _, _ = _case(dev, SMALL)
    rgb_d, dep_d = rgb.to(dev), depth.to(dev)
    trunk.chunk = chunk
    try:
        base = trunk.embed_rgbd(rgb_d, dep_d).cpu()
        for j in (0, 3, 4):
            others = [i for i in range(SMALL[1]) if i != j]
            d2 = dep_d.clone()
            d2[j] = dep_d[(j + 1) % SMALL[1]]
            e = trunk.embed_rgbd(rgb_d, d2).cpu()
            assert not torch.equal(e[j], base[j]) and torch.equal(e[others], base[others]), ("depth", j)
            r2 = rgb_d.clone()
            r2[j] = rgb_d[(j + 2) % SMALL[1]]
            e = trunk.embed_rgbd(r2, dep_d).cpu()
            assert not torch.equal(e[j], base[j]) and torch.equal(e[others], base[others]), ("rgb", j)
    finally:
        trunk.chunk = 0
    r = _rel(base, got0)
    print(f"embed_rgbd chunk {chunk} vs chunk 0: rel-L2 = {r:.3e}")
    assert r <= 7e-3, r                                              # (d): across launch shapes
    if chunk == 0:
        assert torch.equal(base, got0)
    # [B,R,R] is the same input as [B,R,R,1]; `out=` is written in place
    out = torch.empty_like(got0, device=dev)
    assert trunk.embed_rgbd(rgb_d, dep_d.squeeze(-1).contiguous(), out=out) is out and torch.equal(out.cpu(), got0)


def test_uint8_rgb_matches_host_normalised_fp32(dev):
    sd, trunk, _, depth, _, _, _ = _case(dev, SMALL)
    u8 = syn.synthetic_rgb_u8(1000, SMALL[1], SMALL[0])
    e8 = trunk.embed_rgbd(u8.to(dev), depth.to(dev)).cpu()
    e32 = trunk.embed_rgbd(syn.normalize_rgb(u8).to(dev), depth.to(dev)).cpu()
    r = _rel(e8, e32)
    print(f"embed_rgbd uint8 vs host-normalised fp32 frames: rel-L2 = {r:.3e}")
    assert r < 1e-2, r


_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from embodied_clip_amd import synthetic as syn
from embodied_clip_amd.encoder import RN50Trunk
dev = torch.device("cuda:0")
sd = syn.rn50_visual_state_dict(11, width=64, layers=(1, 1, 1, 1), output_dim=64, heads=4, input_resolution=64)
trunk = RN50Trunk(sd, device=dev, input_resolution=64)
rgb = syn.synthetic_rgb(1000, 5, 64).to(dev)
depth = syn.normalize_depth(syn.synthetic_depth(1005, 5, 64)).to(dev)
torch.save(trunk.embed_rgbd(rgb, depth).cpu(), sys.argv[2])
"""


def test_composed_route_in_a_child_process(dev, tmp_path):
    """EC_RGBD_JOINT=0 is read once per process: a child runs the composed route (the plan on the RGB chunk, again on the depth
    chunk, the pair kernel) on the same frames"""
    _, _, _, _, got, _, _ = _case(dev, SMALL)
    path = str(tmp_path / "composed.pt")
    r = GPU.run([sys.executable, "-c", _CHILD, ROOT, path], env={"EC_RGBD_JOINT": "0"}, limit=300)
    assert r.returncode == 0, r.stderr[-2000:]
    composed = torch.load(path)
    rel = _rel(composed, got)
    print(f"embed_rgbd EC_RGBD_JOINT=0 vs default: rel-L2 = {rel:.3e}")
    assert rel <= 7e-3, rel


def test_torchvision_stem_handle_is_unsupported(dev):
    from embodied_clip_amd import _lib
    from embodied_clip_amd.encoder import ImageNetRN50Trunk
    sd = syn.tv_resnet_state_dict(5, layers=(1, 1, 1, 1))
    trunk = ImageNetRN50Trunk(sd, device=dev, input_resolution=64)
    assert trunk.stem_w9 is None
    rgb, depth = torch.zeros(1, 64, 64, 3, device=dev), torch.zeros(1, 64, 64, device=dev)
    w9 = torch.zeros(9, 64, device=dev)
    need = trunk.lib.ec_rn50_rgbd_workspace_bytes(trunk.h, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(1, trunk.out_channels, device=dev)
    rc = trunk.lib.ec_rn50_embed_rgbd(trunk.h, rgb.data_ptr(), 0, None, None, depth.data_ptr(), 1.0, 0.0, w9.data_ptr(), 1, ws.data_ptr(),
                                      ws.numel(), out.data_ptr(), 0, _lib.stream_ptr())
    assert rc == -6, rc          # EC_ERR_UNSUPPORTED
    with pytest.raises(_lib.EcError):
        trunk.embed_rgbd(rgb, depth)
