"""Child process of tests/test_gpu_vit_cls.py: the class embedding of every tower of `_vit_cls_towers.TOWERS` and of the golden
ViT-B/32 preprocessor on the route the environment selects (EC_VIT_CLS_TAIL is read once per process).  Saves {name: fp32 [B, D]}
to argv[1]."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from _vit_cls_towers import TOWERS, golden_case, tower_case  # noqa: E402


def main(out_path):
    from embodied_clip_amd.clip_preprocessors import ClipViTPreprocessor
    from embodied_clip_amd.encoder import ViTEmbedder
    dev = torch.device("cuda:0")
    got = {}
    for t in TOWERS:
        sd, rgb = tower_case(t)
        vit = ViTEmbedder(sd, device=dev, heads=t["heads"], input_resolution=t["res"])
        e = vit.embed_cls(rgb.to(dev))
        assert e.dtype == torch.float32 and tuple(e.shape) == (t["B"], t["width"])
        # into a caller's buffer (a rollout slice): the same values
        buf = torch.zeros((2, t["B"], t["width"]), dtype=torch.float32, device=dev)
        vit.embed_cls(rgb.to(dev), buf[1])
        torch.cuda.synchronize()
        assert torch.equal(buf[1], e) and not buf[0].any()
        got[t["name"]] = e.cpu()
    sd, rgb = golden_case()
    pre = ClipViTPreprocessor("rgb_lowres", "ViT-B/32", class_emb_only=True, cls_shortcut=True, state_dict=sd, device=dev)
    assert pre.observation_space.shape == (768,)
    o = pre.process({"rgb_lowres": rgb})
    assert o.is_cuda and o.dtype == torch.float32
    got["golden_b32"] = o.cpu()
    torch.save(got, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
