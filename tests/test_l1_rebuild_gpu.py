"""Layer 1's rebuilt identity on the GPU.  The boundary kernel that rebuilds block 0's output (conv_pair_rebuild.hip) against the two
launches it stands for, and the trunk with ``ec_rn50_set_l1_rebuild`` on against off: bit for bit.  The existing kernels are held to
float64 element bounds elsewhere (tests/test_trunk_fused_ref.py), so bit-identity to them is the whole numeric claim."""
import pytest
import torch

from embodied_clip_amd import synthetic as syn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _operands(dev, M, seed):
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(torch.bfloat16).to(dev)  # noqa: E731
    act = lambda: bf(torch.randn(M, 64, generator=g).relu())  # noqa: E731
    w = lambda n, k, s: bf(torch.randn(n, k, generator=g) * s)  # noqa: E731
    b = lambda n: torch.randn(n, generator=g).mul(0.3).to(dev)  # noqa: E731
    return dict(a=act(), i0=act(), i1=act(), w3=w(256, 64, 0.15), wi0=w(256, 64, 0.15), wi1=w(256, 64, 0.15), b3=b(256), bi0=b(256),
                bi1=b(256), w2a=w(64, 256, 0.08), b2a=b(64), w2=w(64, 256, 0.08), b2=b(64))


# one tile; more tiles than one sweep of the 256 x 4 wave slots, with a ragged rest of 3
@pytest.mark.parametrize("M", [32, 32 * 1027])
def test_rebuild_kernel_is_the_two_launches_bit_for_bit(dev, M):
    from embodied_clip_amd.encoder import conv1x1_pair_bf16, conv1x1_pair_rebuild_bf16
    o = _operands(dev, M, seed=M)
    # block 0's boundary (conv3 + folded downsample conv -> y0, block 1's conv1 -> z0), then block 1's with y0 as its identity
    y0, z0 = conv1x1_pair_bf16(o["i0"], o["wi0"], o["bi0"], o["w2a"], o["b2a"], a1=o["i1"], w1=o["wi1"], b1=o["bi1"])
    y1, z1 = conv1x1_pair_bf16(o["a"], o["w3"], o["b3"], o["w2"], o["b2"], res=y0)
    gy, gz = conv1x1_pair_rebuild_bf16(o["a"], o["w3"], o["b3"], o["i0"], o["wi0"], o["bi0"], o["i1"], o["wi1"], o["bi1"], o["w2"], o["b2"])
    torch.cuda.synchronize()
    assert y0.count_nonzero().item() > y0.numel() // 4 and y1.count_nonzero().item() > y1.numel() // 4      # (the ReLUs cut, not kill)
    assert torch.equal(gy, y1) and torch.equal(gz, z1)

    # the block-0 boundary without its y store: z the same bits, and the buffer a storing launch has just filled stays as it was
    sentinel = torch.full_like(y0, -7.0)
    y0.copy_(sentinel)
    none, zn = conv1x1_pair_bf16(o["i0"], o["wi0"], o["bi0"], o["w2a"], o["b2a"], a1=o["i1"], w1=o["wi1"], b1=o["bi1"], store_y=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(zn, z0) and torch.equal(y0, sentinel)
    # ... for the residual instance too
    _, zr = conv1x1_pair_bf16(o["a"], o["w3"], o["b3"], o["w2"], o["b2"], res=gy, store_y=False)
    _, zw = conv1x1_pair_bf16(o["a"], o["w3"], o["b3"], o["w2"], o["b2"], res=gy)
    assert torch.equal(zr, zw)


@pytest.fixture(scope="module")
def trunk(dev):
    from embodied_clip_amd.encoder import RN50Trunk
    return RN50Trunk(syn.rn50_visual_state_dict(0), device=dev)


# 1 and 3 frames: every op on its small-launch route; 128: the engine's shape, the fused bottlenecks on
@pytest.mark.parametrize("frames", [1, 3, 128])
def test_trunk_features_are_bit_identical_with_the_option_on(dev, trunk, frames):
    if frames <= 3:
        x = syn.synthetic_rgb(40 + frames, frames).to(dev)
    else:
        x = torch.randn((frames, 224, 224, 3), generator=torch.Generator(device=dev).manual_seed(frames), device=dev)
    base_hash, ws = trunk.plan_hash(), trunk.lib.ec_rn50_workspace_bytes(trunk.h, frames)
    off = trunk.forward(x).clone()
    assert trunk.set_l1_rebuild(True)
    try:
        assert trunk.plan_hash() != base_hash and trunk.lib.ec_rn50_workspace_bytes(trunk.h, frames) == ws
        on = trunk.forward(x).clone()
    finally:
        assert trunk.set_l1_rebuild(False)
    torch.cuda.synchronize()
    assert trunk.plan_hash() == base_hash
    assert torch.isfinite(off.float()).all() and off.float().abs().max().item() > 0
    assert torch.equal(on, off)
    assert torch.equal(trunk.forward(x), off)


def test_a_tower_without_the_plan_keeps_its_own(dev):
    from embodied_clip_amd.encoder import RN50Trunk
    t = RN50Trunk(syn.rn50_visual_state_dict(0, layers=(1, 1, 1, 1)), device=dev)
    h = t.plan_hash()
    assert t.set_l1_rebuild(True) is False and t.plan_hash() == h
