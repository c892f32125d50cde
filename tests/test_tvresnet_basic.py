"""CPU side of the ImageNet ResNet-18 / 34 agents: the BasicBlock restatement (tests/_tv_basic_ref.py) pinned to
HuggingFace ``ResNetModel``, the packer's sizes and BN fold, the drop-in ``ResNetPreprocessor``'s surface (no GPU, no
download) and its rebinding into an allenact tree."""
import os
import subprocess
import sys
import textwrap

import pytest
import torch

from embodied_clip_amd import synthetic as syn
from oracle import tv_resnet as otv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tv_basic_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _randomise(model, g):
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.1)
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.2)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
            elif isinstance(mod, torch.nn.Conv2d):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (mod.weight[0].numel() ** -0.5))


@pytest.mark.parametrize("depths,res", [((2, 2, 2, 2), 64), ((3, 4, 6, 3), 64)])
def test_basic_restatement_matches_hf_resnet_model(depths, res):
    tr = pytest.importorskip("transformers")
    cfg = tr.ResNetConfig(num_channels=3, embedding_size=64, hidden_sizes=[64, 128, 256, 512], depths=list(depths),
                          layer_type="basic", hidden_act="relu", downsample_in_first_stage=False)
    model = tr.ResNetModel(cfg).eval()
    g = torch.Generator().manual_seed(23)
    _randomise(model, g)
    sd = otv.hf_resnet_to_torchvision_keys(model.state_dict())
    assert "layer2.0.downsample.0.weight" in sd and "layer1.0.downsample.0.weight" not in sd
    assert not any(".conv3." in k for k in sd)
    x = torch.randn(2, 3, res, res, generator=g)
    with torch.no_grad():
        out = model(x.clone()).last_hidden_state
    for fold in (True, False):
        got = ref.basic_trunk(x, sd, fold=fold)
        assert got.shape == out.shape == (2, 512, res // 32, res // 32)
        assert (got - out).abs().max() < 5e-5 * max(1.0, float(out.abs().max()))
    emu = ref.basic_trunk(x, sd, emulate_bf16=True)
    assert torch.nn.functional.cosine_similarity(emu.flatten(1), out.flatten(1)).min() > 0.999


@pytest.mark.parametrize("layers,n_w,n_b,n_layers", [((2, 2, 2, 2), 11_166_912, 4_800, 20), ((3, 4, 6, 3), 21_267_648, 8_512, 36)])
def test_pack_sizes(layers, n_w, n_b, n_layers):
    from embodied_clip_amd.encoder import pack_tv_basic
    sd = syn.tv_resnet_state_dict(0, layers=layers, block="basic", with_fc=True)
    (width, got_layers), stem_w, w, b = pack_tv_basic(sd)
    assert width == 64 and list(got_layers) == list(layers)
    assert w.numel() + 64 * 3 * 7 * 7 == n_w and b.numel() == n_b
    assert stem_w.shape == (64, 176) and w.dtype == torch.bfloat16 and b.dtype == torch.float32
    # conv layers: stem + 2 per block + 3 downsample convs (ResNet-18: 1 + 16 + 3 = 20; ResNet-34: 1 + 32 + 3 = 36)
    assert 1 + sum(1 for k in sd if k.endswith(".weight") and ".conv" in k or "downsample.0.weight" in k) == n_layers


def test_pack_rejects_bottleneck():
    from embodied_clip_amd.encoder import pack_tv_basic
    with pytest.raises(ValueError):
        pack_tv_basic(syn.tv_resnet_state_dict(0, layers=(1, 1, 1, 1)))


def test_bn_fold_equals_eval_bn():
    from embodied_clip_amd.encoder import pack_tv_basic
    sd = syn.tv_resnet_state_dict(4, layers=(2, 2, 2, 2), block="basic")
    (_wd, _l), _s, w, b = pack_tv_basic(sd)
    # layer2.0: conv1 [128,3,3,64], conv2 [128,3,3,128], downsample [128,1,1,64]; offsets in the packed order
    off = 0
    for li, n in enumerate((2, 2, 2, 2), start=1):
        for blk in range(n):
            for conv in ("conv1", "conv2", "downsample.0"):
                key = f"layer{li}.{blk}.{conv}.weight"
                if key not in sd:
                    continue
                wt = sd[key]
                if (li, blk) == (2, 0):
                    bn = f"layer{li}.{blk}." + ("downsample.1" if conv == "downsample.0" else "bn" + conv[-1])
                    x = torch.randn(1, wt.shape[1], 6, 6)
                    y = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, wt, padding=wt.shape[-1] // 2),
                                                       sd[bn + ".running_mean"], sd[bn + ".running_var"], sd[bn + ".weight"],
                                                       sd[bn + ".bias"], False, 0.0, 1e-5)
                    wf = w[off:off + wt.numel()].float().view(wt.shape[0], wt.shape[2], wt.shape[3], wt.shape[1]).permute(0, 3, 1, 2)
                    bi = [i for i, k in enumerate(_bias_keys(sd)) if k == bn][0]
                    bf = b[bi:bi + wt.shape[0]]
                    yf = torch.nn.functional.conv2d(x, wf, bf, padding=wt.shape[-1] // 2)
                    assert ((yf - y).norm() / y.norm()).item() < 1e-2          # (bf16 weights)
                off += wt.numel()
    assert off == w.numel()


def _bias_keys(sd):
    """bias-vector start offsets, keyed by BN prefix, in the packed order (stem first) -> list expanded per channel."""
    out = ["bn1"] * 64
    for k in sd:
        if k.endswith(".running_mean") and k != "bn1.running_mean":
            bn = k[: -len(".running_mean")]
            out += [bn] * sd[k].numel()
    return out


def test_resnet_preprocessor_surface_without_gpu(monkeypatch, tmp_path):
    from embodied_clip_amd.imagenet_preprocessors import ResNetPreprocessor, resnet_name
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url",
                        lambda *a, **k: (_ for _ in ()).throw(AssertionError("ResNetPreprocessor tried to download")))
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "hub"))
    monkeypatch.delenv("EC_TORCHVISION_WEIGHTS_DIR", raising=False)
    for name, C in (("resnet18", 512), ("resnet34", 512), ("resnet50", 2048)):
        fn = _named(name)   # what torchvision.models.<name> is to the preprocessor: a callable with that __name__
        assert resnet_name(fn) == name == resnet_name(name)
        for pool in (False, True):
            p = ResNetPreprocessor(224, 224, 7, 7, C, pool, torchvision_resnet_model=fn, device=torch.device("cpu"),
                                   input_uuids=["rgb_lowres"], output_uuid="rgb_resnet")
            assert p.observation_space.shape == ((C,) if pool else (C, 7, 7))
            assert p.input_uuids == ["rgb_lowres"] and p.uuid == "rgb_resnet"
    with pytest.raises(ValueError):
        resnet_name("resnet19")
    with pytest.raises(ValueError):
        ResNetPreprocessor(224, 224, 7, 7, 2048, False, torchvision_resnet_model="resnet18", input_uuids=["rgb"], output_uuid="o")
    with pytest.raises(ValueError):
        ResNetPreprocessor(224, 224, 8, 8, 512, False, torchvision_resnet_model="resnet18", input_uuids=["rgb"], output_uuid="o")
    p = ResNetPreprocessor(224, 224, 7, 7, 512, False, input_uuids=["rgb"], output_uuid="o", device=torch.device("cpu"))
    with pytest.raises(FileNotFoundError) as ei:
        p.resnet
    msg = str(ei.value)
    assert "state_dict=" in msg and "EC_TORCHVISION_WEIGHTS_DIR" in msg and "hub" in msg


def _named(name):
    def f(*a, **k):
        raise AssertionError("the model constructor must not be called")
    f.__name__ = name
    return f


def test_resnet_preprocessor_finds_weights_in_order(monkeypatch, tmp_path):
    from embodied_clip_amd.imagenet_preprocessors import find_weights
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url",
                        lambda *a, **k: (_ for _ in ()).throw(AssertionError("download attempted")))
    hub = tmp_path / "hub"
    (hub / "checkpoints").mkdir(parents=True)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(hub))
    torch.save({"w": torch.ones(1)}, hub / "checkpoints" / "resnet18-f37072fd.pth")
    assert torch.equal(find_weights("resnet18")["w"], torch.ones(1))
    envd = tmp_path / "env"
    envd.mkdir()
    torch.save({"w": torch.zeros(1)}, envd / "resnet18.pth")
    monkeypatch.setenv("EC_TORCHVISION_WEIGHTS_DIR", str(envd))
    assert torch.equal(find_weights("resnet18")["w"], torch.zeros(1))
    assert torch.equal(find_weights("resnet18", state_dict={"w": torch.full((1,), 2.0)})["w"], torch.full((1,), 2.0))
    with pytest.raises(FileNotFoundError):
        find_weights("resnet34")


FAKE = {
    "allenact/__init__.py": "",
    "allenact/embodiedai/__init__.py": "",
    "allenact/embodiedai/preprocessors/__init__.py": "",
    "allenact/embodiedai/preprocessors/resnet.py": """
        class ResNetPreprocessor: ORIGINAL = True
        """,
    "experiment_config.py": """
        from allenact.embodiedai.preprocessors.resnet import ResNetPreprocessor
        """,
}


def test_install_into_allenact_rebinds_resnet_preprocessor(tmp_path):
    for rel, src in FAKE.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(textwrap.dedent(src))
    prog = textwrap.dedent("""
        from embodied_clip_amd import allenact_compat as ac
        from embodied_clip_amd.imagenet_preprocessors import ResNetPreprocessor
        done = ac.install_into_allenact()
        assert 'allenact.embodiedai.preprocessors.resnet.ResNetPreprocessor' in done, done
        import experiment_config as cfg
        assert cfg.ResNetPreprocessor is ResNetPreprocessor and not hasattr(cfg.ResNetPreprocessor, 'ORIGINAL')
        print('OK')
    """)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", prog], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
