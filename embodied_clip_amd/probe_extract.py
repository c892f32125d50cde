"""From simulator scene files to the probe's feature cache -- the three data scripts of ``primitive_probing/generate_data``
after the renderer, with the reference's flag names:

    python -m embodied_clip_amd.probe_extract thor --data_dir data/ithor_scenes --output_dir data \
        --target-objects tests/golden/probe_target_objects.json          # thor_image_features.py  -> thor_{split}.pt
    python -m embodied_clip_amd.probe_extract reachable --data_dir data/CSR/edge_full --output_dir data
                                                                         # reachable_image_features.py -> reachable_image_features.pt
    python -m embodied_clip_amd.probe_extract reachable-metadata --data_dir data/CSR/edge_full --output_dir data
                                                                         # reachable_metadata.py   -> reachable_{split}.pkl

then ``python -m embodied_clip_amd.probe_train --data-dir data ...``.  Rendering (thor_frames.py: the Unity simulator)
is the one step that stays outside.

Weights: ``--clip-weights PATH`` or ``$EC_CLIP_WEIGHTS_DIR/RN50.pt``; ``--imagenet-weights PATH``,
``$EC_TORCHVISION_WEIGHTS_DIR/resnet50*.pth`` or torch's hub cache; ``--synthetic-weights`` uses the seeded stand-ins
of ``probe_train --synthetic-frames``.  Nothing is ever downloaded.  Without ImageNet weights the cache holds the three
``clip_*`` keys only and a notice says so.  ``thor`` and ``reachable`` need the GPU (no CPU fallback);
``reachable-metadata`` is host-only.  Each sub-command prints one JSON line.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch

from . import synthetic as syn
from .probe_data import (CLIP_KEYS, IMAGENET_KEYS, ClipFeatureExtractor, build_reachable_features, build_thor_features,
                         write_reachable_cache, write_thor_cache)
from .probe_labels import SPLITS, build_reachable_metadata, label_points, read_scene_file, read_target_objects


def _need_gpu():
    if not torch.cuda.is_available():
        raise SystemExit("embodied_clip_amd.probe_extract needs an MI355X (no CPU fallback)")


def make_extractor(a, device="cuda:0") -> ClipFeatureExtractor:
    """Both frozen towers of the feature scripts (thor_image_features.py:46-67) from the weights the flags name."""
    if a.synthetic_weights:
        return ClipFeatureExtractor(syn.rn50_visual_state_dict(0), device=device, imagenet_state_dict=syn.tv_resnet_state_dict(0))
    from .clip_preprocessors import _load_visual_state_dict
    from .imagenet_preprocessors import find_weights
    path = a.clip_weights
    if path is None and os.environ.get("EC_CLIP_WEIGHTS_DIR"):
        path = os.path.join(os.environ["EC_CLIP_WEIGHTS_DIR"], "RN50.pt")
    if path is None or not os.path.exists(path):
        raise SystemExit(f"probe_extract: no CLIP RN50 checkpoint at {path!r}: pass --clip-weights PATH, set EC_CLIP_WEIGHTS_DIR, "
                         "or use --synthetic-weights (nothing is downloaded)")
    clip_sd = _load_visual_state_dict("RN50", None, path)
    try:
        imagenet_sd = find_weights("resnet50", weights_path=a.imagenet_weights)
    except FileNotFoundError as e:
        if a.imagenet_weights is not None:
            raise
        imagenet_sd = None
        print(f"probe_extract: the cache will hold {', '.join(CLIP_KEYS)} only; {', '.join(IMAGENET_KEYS)} are missing "
              f"because no torchvision ResNet-50 weights were found ({e})", file=sys.stderr)
    return ClipFeatureExtractor(clip_sd, device=device, imagenet_state_dict=imagenet_sd)


class _Timed:
    """Seconds between two device synchronisations, summed per name."""

    def __init__(self):
        self.seconds = {}

    def __call__(self, name, fn, *args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*args, **kw)
        torch.cuda.synchronize()
        self.seconds[name] = self.seconds.get(name, 0.0) + time.perf_counter() - t0
        return out


def extract_thor(a) -> dict:
    """thor_image_features.py:91-140: every ``*.npy`` of every split -> ``thor_{split}.pt``."""
    _need_gpu()
    targets = read_target_objects(a.target_objects)
    ex = make_extractor(a)
    timed = _Timed()
    frames = scenes = 0
    t0 = time.perf_counter()
    for split in SPLITS:
        features = {}
        for path in sorted(glob.glob(os.path.join(a.data_dir, split, "*.npy"))):
            scene_name = os.path.splitext(os.path.basename(path))[0]
            points = timed("labels", label_points, read_scene_file(path), targets, ex.device, ex.batch)
            features.update(timed("encoders", build_thor_features, ex, {scene_name: points}))
            frames += len(points)
            scenes += 1
        write_thor_cache(a.output_dir, split, features)
    dt = time.perf_counter() - t0
    return {"command": "thor", "frames": frames, "scenes": scenes, "frames_per_s": round(frames / max(dt, 1e-9), 1),
            "labels_s": round(timed.seconds.get("labels", 0.0), 4), "encoders_s": round(timed.seconds.get("encoders", 0.0), 4),
            "embedding_keys": list(ex.keys)}


def extract_reachable(a) -> dict:
    """reachable_image_features.py:24,77-100: every ``*.png`` of ``--data_dir`` -> ``reachable_image_features.pt``."""
    _need_gpu()
    from PIL import Image   # only this sub-command decodes image files
    ex = make_extractor(a)
    timed = _Timed()
    paths = sorted(glob.glob(os.path.join(a.data_dir, "*.png")))
    by_size = {}
    for p in paths:
        with Image.open(p) as im:
            arr = torch.from_numpy(np.asarray(im.convert("RGB")).copy())
        by_size.setdefault(tuple(arr.shape), {})[os.path.splitext(os.path.basename(p))[0]] = arr
    t0 = time.perf_counter()
    feats = {}
    for images in by_size.values():
        feats.update(timed("encoders", build_reachable_features, ex, images))
    dt = time.perf_counter() - t0
    write_reachable_cache(a.output_dir, feats, {})
    return {"command": "reachable", "frames": len(feats), "scenes": 0, "frames_per_s": round(len(feats) / max(dt, 1e-9), 1),
            "labels_s": 0.0, "encoders_s": round(timed.seconds.get("encoders", 0.0), 4), "embedding_keys": list(ex.keys)}


def extract_reachable_metadata(a) -> dict:
    """reachable_metadata.py -> ``reachable_{split}.pkl``."""
    t0 = time.perf_counter()
    superset, triples = build_reachable_metadata(a.data_dir, a.seed)
    write_reachable_cache(a.output_dir, None, triples)
    return {"command": "reachable-metadata", "classes": len(superset), "triples": {s: len(r) for s, r in triples.items()},
            "seconds": round(time.perf_counter() - t0, 4)}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m embodied_clip_amd.probe_extract", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)

    def weights(p):
        p.add_argument("--clip-weights", dest="clip_weights", default=None, help="CLIP RN50 checkpoint (else $EC_CLIP_WEIGHTS_DIR/RN50.pt)")
        p.add_argument("--imagenet-weights", dest="imagenet_weights", default=None,
                       help="torchvision resnet50 state dict (else $EC_TORCHVISION_WEIGHTS_DIR, then torch's hub cache)")
        p.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                       help="seeded stand-in weights for both towers (exercises the tool where no checkpoint exists)")

    p = sub.add_parser("thor", help="ithor_scenes/{train,val,test}/*.npy -> thor_{split}.pt (thor_image_features.py)")
    p.add_argument("--data_dir", type=str, default="data/ithor_scenes", help="Path to ithor_scenes directory, generated by thor_frames.py")
    p.add_argument("--output_dir", type=str, default="data", help="Path output directory")
    p.add_argument("--target-objects", dest="target_objects", required=True,
                   help="file with the target object names of the labels (a JSON list, or one name per line)")
    weights(p)
    p.set_defaults(fn=extract_thor)

    p = sub.add_parser("reachable", help="CSR edge_full/*.png -> reachable_image_features.pt (reachable_image_features.py); "
                       "every image goes through .convert('RGB') after Image.open -- the identity for RGB files and the "
                       "one deviation from the reference, which hands the opened image to the transforms as it is")
    p.add_argument("--data_dir", type=str, default="data/CSR/edge_full", help="Path to CSR edge_full directory")
    p.add_argument("--output_dir", type=str, default="data", help="Path output directory")
    weights(p)
    p.set_defaults(fn=extract_reachable)

    p = sub.add_parser("reachable-metadata", help="CSR edge_full/{split}_boxes*.json -> reachable_{split}.pkl (reachable_metadata.py)")
    p.add_argument("--data_dir", type=str, default="data/CSR/edge_full", help="Path to CSR edge_full directory")
    p.add_argument("--output_dir", type=str, default="data", help="Path output directory")
    p.add_argument("--seed", type=int, default=1, help="seed of the shuffle (the reference shuffles unseeded)")
    p.set_defaults(fn=extract_reachable_metadata)

    a = ap.parse_args(argv)
    print(json.dumps(a.fn(a)))


if __name__ == "__main__":
    main()
