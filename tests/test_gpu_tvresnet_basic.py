"""GPU parity of the ImageNet ResNet-18 / 34 agents: the BasicBlock transition-tail kernel (ec_basic_tail_s2_bf16), the
generic 3x3 + residual epilogue the stride-1 conv2 launches take, whole ec_tvresnet_basic_create trunks against the
restatement in tests/_tv_basic_ref.py (itself pinned to HuggingFace ResNetModel), the drop-in ResNetPreprocessor, the
policy on 512-channel features and engine.Worker(encoder="imagenet_rn18").

Tolerances as for the torchvision ResNet-50 trunk (tests/test_gpu_tvresnet.py): vs the bf16 emulation rel-L2 <= 4e-3 *
sqrt(1 + #blocks); vs fp32 rel-L2 <= 2e-2 and cosine >= 0.999."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from embodied_clip_amd import synthetic as syn
from oracle import policy as opol
from oracle import ppo as oppo

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tv_basic_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

L18, L34 = (2, 2, 2, 2), (3, 4, 6, 3)


def _rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)).item()


def _bf(x):
    return x.to(torch.bfloat16)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


_SD = {}


def _sd(layers):
    if layers not in _SD:
        _SD[layers] = syn.tv_resnet_state_dict(7, layers=layers, block="basic")
    return _SD[layers]


@pytest.mark.parametrize("Ho,planes,inplanes", [(28, 128, 64), (14, 256, 128), (7, 512, 256)])
@pytest.mark.parametrize("B", [1, 5, 32])
def test_basic_tail_matches_torch(dev, B, Ho, planes, inplanes):
    """relu(conv3x3(c1) + conv1x1_s2(x) + b) in one launch vs F.conv2d on the same bf16-rounded operands."""
    from embodied_clip_amd.encoder import basic_tail_s2_bf16
    g = torch.Generator().manual_seed(B * 100 + planes)
    c1 = _bf(torch.randn(B, Ho, Ho, planes, generator=g).relu())
    x = _bf(torch.randn(B, 2 * Ho, 2 * Ho, inplanes, generator=g).relu())
    w2 = _bf(torch.randn(planes, 3, 3, planes, generator=g) * (9 * planes) ** -0.5)
    wd = _bf(torch.randn(planes, inplanes, generator=g) * inplanes ** -0.5)
    b = torch.randn(planes, generator=g) * 0.1
    y = F.conv2d(c1.float().permute(0, 3, 1, 2), w2.float().permute(0, 3, 1, 2), None, padding=1)
    y = y + F.conv2d(x.float().permute(0, 3, 1, 2), wd.float()[:, :, None, None], None, stride=2)
    y = F.relu(y + b.view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    w_cat = torch.cat([w2.reshape(planes, -1), wd], dim=1).contiguous()
    got = basic_tail_s2_bf16(c1.to(dev), x.to(dev), w_cat.to(dev), b.to(dev))
    torch.cuda.synchronize()
    got = got.cpu().float()
    assert got.shape == y.shape == (B, Ho, Ho, planes)
    assert _rel(got, y) < 4e-3, _rel(got, y)


@pytest.mark.parametrize("B,H,C", [(2, 28, 128), (3, 14, 256), (5, 7, 512)])
def test_generic_3x3_residual_epilogue(dev, B, H, C):
    """The stride-1 conv2 of layers 2-4: ec_conv_bf16 3x3 with a residual (no Bottleneck ever had one)."""
    from embodied_clip_amd import encoder as enc
    g = torch.Generator().manual_seed(B + C)
    x = _bf(torch.randn(B, H, H, C, generator=g).relu())
    w = _bf(torch.randn(C, 3, 3, C, generator=g) * (9 * C) ** -0.5)
    b = torch.randn(C, generator=g) * 0.1
    r = _bf(torch.randn(B, H, H, C, generator=g).relu())
    y = F.conv2d(x.float().permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), b, padding=1) + r.float().permute(0, 3, 1, 2)
    y = F.relu(y).permute(0, 2, 3, 1)
    got = enc.conv_bf16(x.to(dev), w.reshape(C, -1).to(dev), b.to(dev), res=r.to(dev), ksize=3, act=1)
    torch.cuda.synchronize()
    assert _rel(got.cpu().float(), y) < 4e-3


@pytest.mark.parametrize("layers", [L18, L34])
@pytest.mark.parametrize("B", [1, 3, 32, 128])
def test_basic_trunk_matches_restatement(dev, layers, B):
    from embodied_clip_amd.encoder import ImageNetBasicTrunk
    sd = _sd(layers)
    x = syn.normalize_rgb_imagenet(syn.synthetic_rgb_u8(17 + B, B, 224))
    trunk = ImageNetBasicTrunk(sd, device=dev)
    assert trunk.out_channels == 512 and trunk.out_spatial == 7
    feat = trunk.forward(x.contiguous().to(dev))
    nchw = trunk.to_nchw_f32(feat).cpu()
    avg = trunk.spatial_mean(feat).cpu()
    assert nchw.shape == (B, 512, 7, 7)
    assert torch.allclose(avg, nchw.mean(dim=(2, 3)), rtol=1e-5, atol=1e-6)
    idx = sorted({0, B // 2, B - 1})      # the CPU restatement on a few frames of the launch
    xs = x[idx].permute(0, 3, 1, 2)
    r32 = ref.basic_trunk(xs, sd)
    emu = ref.basic_trunk(xs, sd, emulate_bf16=True)
    got = nchw[idx]
    nb = sum(layers)
    assert _rel(got, emu) < 4e-3 * math.sqrt(1 + nb), _rel(got, emu)
    assert _rel(got, r32) < 2e-2, _rel(got, r32)
    assert F.cosine_similarity(got.flatten(1), r32.flatten(1)).min() > 0.999


def test_chunked_256_launch_agrees_with_single_frames(dev):
    from embodied_clip_amd.encoder import ImageNetBasicTrunk
    sd = _sd(L18)
    trunk = ImageNetBasicTrunk(sd, device=dev, chunk=100)             # chunks of 100, 100, 56
    frames = syn.normalize_rgb_imagenet(syn.synthetic_rgb_u8(5, 8, 224)).to(dev)
    big = frames.repeat(32, 1, 1, 1).contiguous()
    fb = trunk.forward(big).float().cpu()
    assert torch.equal(fb[:8], fb[8:16])                                # same frame, same launch geometry -> bit-identical
    single = ImageNetBasicTrunk(None, device=dev, weights_from=trunk)
    for i in (0, 99, 100, 255):
        f1 = single.forward(big[i:i + 1].contiguous()).float().cpu()
        assert _rel(fb[i:i + 1], f1) < 7e-3, (i, _rel(fb[i:i + 1], f1))


def test_u8_path_matches_f32_path(dev):
    from embodied_clip_amd.encoder import ImageNetBasicTrunk
    trunk = ImageNetBasicTrunk(_sd(L34), device=dev)
    raw = syn.synthetic_rgb_u8(3, 4, 224).to(dev)
    f_u8 = trunk.forward_u8(raw).float().cpu()
    f_f32 = trunk.forward(syn.normalize_rgb_imagenet(raw).contiguous()).float().cpu()
    assert _rel(f_u8, f_f32) < 7e-3, _rel(f_u8, f_f32)


@pytest.mark.parametrize("N", [1, 64])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("host", [False, True])
def test_resnet_preprocessor_process(dev, N, pool, host):
    from embodied_clip_amd.encoder import ImageNetBasicTrunk
    from embodied_clip_amd.imagenet_preprocessors import ResNetPreprocessor
    sd = _sd(L18)
    p = ResNetPreprocessor(224, 224, 7, 7, 512, pool, torchvision_resnet_model="resnet18", device=dev, state_dict=sd,
                           input_uuids=["rgb_lowres"], output_uuid="rgb_resnet")
    x = syn.normalize_rgb_imagenet(syn.synthetic_rgb_u8(40 + N, N, 224)).contiguous()
    out = p.process({"rgb_lowres": x if host else x.to(dev)})
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == ((N, 512) if pool else (N, 512, 7, 7))
    trunk = ImageNetBasicTrunk(sd, device=dev)
    feat = trunk.forward(x.to(dev))
    want = trunk.spatial_mean(feat) if pool else trunk.to_nchw_f32(feat)
    assert torch.equal(out, want)
    d = p.process({"rgb_lowres": x[..., :1].contiguous().to(dev)})     # depth: one channel repeated x 3
    assert tuple(d.shape) == tuple(out.shape)


def test_policy_on_512_channel_features(dev):
    from embodied_clip_amd import ppo
    from embodied_clip_amd.policy import PolicyHandle
    T, N, C, S, H = 3, 8, 512, 7, 512
    cfg = dict(in_channels=C, spatial=S, hidden=H)
    sd = syn.policy_state_dict(5, **cfg)
    g = torch.Generator().manual_seed(6)
    feat = torch.randn(T, N, C, S, S, generator=g).abs().to(torch.bfloat16).float()
    goal = syn.synthetic_goals(7, (T, N))
    h0 = torch.randn(1, N, H, generator=g) * 0.5
    masks = syn.synthetic_masks(8, T, N, p_reset=0.2)
    actions = torch.randint(0, 6, (T, N), generator=g)
    with torch.no_grad():
        lg, vv, _ = opol.actor_critic_forward(feat, goal, h0, masks, sd)
    old_lp = opol.categorical_log_prob(lg, actions).unsqueeze(-1) + 0.2 * torch.randn(T, N, 1, generator=g)
    old_v = vv + 0.2 * torch.randn(T, N, 1, generator=g)
    returns, nadv = torch.randn(T, N, 1, generator=g), torch.randn(T, N, 1, generator=g)
    batch = dict(feat=feat, goal=goal, h0=h0, masks=masks, actions=actions, old_log_probs=old_lp, old_values=old_v,
                 returns=returns, norm_adv=nadv)
    info, ref_grads = oppo.ppo_update_step({k: v.clone() for k, v in sd.items()}, batch, {}, lr=3e-4, max_grad_norm=0.5)
    h = PolicyHandle(**cfg)
    flat = h.flatten(sd, dev)
    rows = feat.permute(0, 1, 3, 4, 2).reshape(T * N, S * S, C).contiguous().to(torch.bfloat16).to(dev)
    m = masks.reshape(-1).to(dev)
    ws = torch.empty(h.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
    hv, _ = h.forward(flat, rows, goal.reshape(-1).to(dev), h0[0].contiguous().to(dev), m, T, N, ws)
    torch.cuda.synchronize()
    hvv = hv.view(T, N, -1).cpu()
    assert _rel(hvv[..., :6], lg) < 2e-5 and _rel(hvv[..., 6:], vv) < 2e-5
    f = lambda t: t.reshape(-1).contiguous().to(dev)
    dhv, sums = ppo.ppo_loss_raw(hv, f(actions), f(old_lp), f(old_v), f(returns), f(nadv), 6)
    grads = torch.zeros_like(flat)
    h.backward(flat, rows, m, T, N, ws, dhv, None, grads)
    torch.cuda.synchronize()
    total = ((sums[0] + 0.5 * sums[1] + 0.01 * sums[2]) / (T * N)).item()
    assert abs(total - info["ppo_total"]) < 1e-5 * max(1.0, abs(info["ppo_total"]))
    gv = h.views(grads)
    for name, gref in ref_grads.items():
        assert _rel(gv[name].cpu(), gref) < 2e-4, (name, _rel(gv[name].cpu(), gref))


def test_worker_imagenet_rn18(dev):
    from embodied_clip_amd.encoder import ImageNetBasicTrunk
    from embodied_clip_amd.engine import Worker
    T, N = 4, 8
    enc_sd = _sd(L18)
    runs = []
    for _ in range(2):
        w = Worker(N, T=T, device="cuda:0", seed=3, update_repeats=1, encoder="imagenet_rn18", encoder_sd=enc_sd)
        assert (w.S, w.C) == (7, 512)
        w.collect_rollout()
        torch.cuda.synchronize()
        feats = w.feat.clone()
        w.compute_returns()
        w.update()
        w.after_update()
        torch.cuda.synchronize()
        runs.append((w, feats, w.loss_info()))
    w, feats, info = runs[0]
    trunk = ImageNetBasicTrunk(enc_sd, device=dev)
    frames = w.env.frames
    for t in range(T + 1):
        fr = frames[t % frames.shape[0]].contiguous()
        want = trunk.forward_u8(fr) if fr.dtype == torch.uint8 else trunk.forward(fr)
        got = feats[t].view(N, 7, 7, 512)
        assert _rel(got.float(), want.float()) < 7e-3, (t, _rel(got.float(), want.float()))
    assert all(math.isfinite(v) for v in info.values()), info
    assert torch.isfinite(w.params).all()
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0].params, runs[1][0].params)


def test_plan_hashes_are_distinct(dev):
    from embodied_clip_amd.encoder import ImageNetBasicTrunk, ImageNetRN50Trunk, RN50Trunk
    h18 = ImageNetBasicTrunk(_sd(L18), device=dev).plan_hash()
    h34 = ImageNetBasicTrunk(_sd(L34), device=dev).plan_hash()
    h50 = ImageNetRN50Trunk(syn.tv_resnet_state_dict(0), device=dev).plan_hash()
    clip = RN50Trunk(syn.rn50_visual_state_dict(0), device=dev).plan_hash()
    assert len({h18, h34, h50, clip}) == 4
