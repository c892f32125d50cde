"""The seeded towers of the class-embedding tests (tests/test_gpu_vit_cls.py and its child process), and their inputs."""
import os

import torch

from embodied_clip_amd import synthetic as syn

# width, layers, heads, patch, resolution, B
TOWERS = (
    dict(name="L50_fold", width=128, layers=3, heads=2, patch=32, res=224, B=3),        # 50 tokens, LayerNorm fold on
    dict(name="L82_general", width=192, layers=3, heads=3, patch=16, res=144, B=3),     # 82 tokens: general core; 192 % 128 != 0: fold off
    dict(name="L37_one_block", width=128, layers=2, heads=2, patch=16, res=96, B=5),    # layers_run = 1: the CLS block follows ln_pre
    dict(name="L37_three_blocks", width=128, layers=4, heads=2, patch=16, res=96, B=2),
)


def tower_case(t, seed=7):
    sd = syn.vit_visual_state_dict(seed, width=t["width"], layers=t["layers"], heads=t["heads"], patch_size=t["patch"],
                                   input_resolution=t["res"], output_dim=64)
    return sd, syn.synthetic_rgb(70 + seed, t["B"], t["res"])


def golden_case():
    G = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_golden.pt"))
    return syn.vit_visual_state_dict(G["vit"]["seed_weights"]), syn.synthetic_rgb(G["vit"]["seed_rgb"], 2)
