"""Host side of the RGB-D path: synthetic depth frames, the folded one-channel stem weights, the env's depth pool."""
import torch
import torch.nn.functional as F

from embodied_clip_amd import synthetic as syn


def test_synthetic_depth_is_deterministic_and_in_range():
    a, b, c = syn.synthetic_depth(3, 2, 32), syn.synthetic_depth(3, 2, 32), syn.synthetic_depth(4, 2, 32)
    assert a.shape == (2, 32, 32, 1) and a.dtype == torch.float32
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    assert 0.4 < float(a.mean()) < 0.6                      # uniform, not a constant
    n = syn.normalize_depth(a)
    assert torch.allclose(n, (a - 0.5) / 0.25)


def test_fold_stem_depth_equals_the_three_channel_conv_on_the_repeated_frame():
    from embodied_clip_amd.encoder import fold_stem_depth, pack_rn50
    sd = syn.rn50_visual_state_dict(11, width=64, layers=(1, 1, 1, 1), output_dim=64, heads=4, input_resolution=64)
    _, stem_w, _, bias = pack_rn50(sd)
    sc = stem_w.shape[1]
    w9 = fold_stem_depth(stem_w)
    assert w9.shape == (9, sc) and w9.dtype == torch.float32
    d = syn.normalize_depth(syn.synthetic_depth(5, 2, 64)).permute(0, 3, 1, 2)              # [2,1,64,64]
    w3 = stem_w.t().reshape(sc, 3, 3, 3).permute(0, 3, 1, 2).contiguous()                   # [sc, ci, ky, kx]
    w1 = w9.t().reshape(sc, 1, 3, 3).contiguous()
    ref = F.conv2d(d.repeat(1, 3, 1, 1), w3, bias[:sc], stride=2, padding=1)
    got = F.conv2d(d, w1, bias[:sc], stride=2, padding=1)
    rel = ((got - ref).norm() / ref.norm()).item()
    assert rel < 1e-6, rel


def test_depth_env_keeps_every_other_attribute_bit_equal():
    from embodied_clip_amd.engine import NavSyntheticEnv, SyntheticEnv
    a = SyntheticEnv(4, 3, "cpu", 7, res=32)
    b = SyntheticEnv(4, 3, "cpu", 7, res=32, depth=True)
    assert not hasattr(a, "depth")
    for k in ("frames", "masks", "goals", "rewards", "success"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert b.depth.shape == (b.pool_steps, 4, 32, 32, 1) and b.depth.dtype == torch.float32
    for i in range(b.pool_steps):
        for j in range(i + 1, b.pool_steps):
            assert not torch.equal(b.depth[i], b.depth[j])
    # normalised: ~ U[-2, 2)
    assert float(b.depth.min()) >= -2.0 and float(b.depth.max()) <= 2.0 and float(b.depth.min()) < -1.5
    # the depth batch follows the RGB batch in both ways of asking
    for k in range(6):
        f = b.observe()
        assert torch.equal(f, b.observe_at(k))
        assert torch.equal(b.observe_depth(), b.observe_depth_at(k)) and torch.equal(b.observe_depth(), b.depth[k % b.pool_steps])
    n = NavSyntheticEnv(4, 3, "cpu", 7, res=32, depth=True)
    assert torch.equal(n.depth, b.depth) and torch.equal(n.frames, a.frames)


def test_default_size_env_matches_the_issue_call():
    from embodied_clip_amd.engine import SyntheticEnv
    a, b = SyntheticEnv(4, 3, "cpu", 7), SyntheticEnv(4, 3, "cpu", 7, depth=True)
    for k in ("frames", "masks", "goals", "rewards", "success"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert b.depth.shape == (4, 4, 224, 224, 1)
    assert not torch.equal(b.depth[0], b.depth[1])
