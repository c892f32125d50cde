"""Measurements behind profiles/probe_extract_labels.txt: the label kernel of ``probe_extract thor`` next to the encoders.

    python tools/bench_probe_extract.py write DIR [--points 640]      scene files of seeded 300 x 300 points
                                                                      (DIR/ithor_scenes/train/FloorPlan*.npy, 64 points each)
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o p -- \
        python -m embodied_clip_amd.probe_extract thor --data_dir DIR/ithor_scenes --output_dir DIR/data \
            --target-objects tests/golden/probe_target_objects.json --synthetic-weights
    python tools/bench_probe_extract.py stats OUT                     semantic_labels_kernel next to resize_crop_kernel:
                                                                      us per 64-frame launch, bytes/s against 6.29 TB/s
    python tools/bench_probe_extract.py ab DIR [--reps 3]             one process, the same points, alternating: labels
                                                                      supplied (``build_thor_features`` alone) and labels
                                                                      computed from the semantic frames; medians, spreads

The semantic frames are those of the label tests (tests/_probe_label_frames.py: flat regions, as a simulator's are)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
TARGETS = os.path.join(ROOT, "tests", "golden", "probe_target_objects.json")
HBM_ACHIEVABLE = 6.29e12   # bytes/s: the project's figure for achievable HBM bandwidth
RES, PER_SCENE = 300, 64


def write(a):
    import _probe_label_frames as plf
    from embodied_clip_amd import synthetic as syn
    targets = json.load(open(TARGETS))
    d = os.path.join(a.dir, "ithor_scenes", "train")
    os.makedirs(d, exist_ok=True)
    for s in ("val", "test"):
        os.makedirs(os.path.join(a.dir, "ithor_scenes", s), exist_ok=True)
    for s in range(a.points // PER_SCENE):
        rgb = syn.synthetic_rgb_u8(500 + s, PER_SCENE, RES).numpy()
        pts = []
        for k in range(PER_SCENE):
            seed = 9000 + s * PER_SCENE + k
            pts.append({"frame": rgb[k], "semantic_frame": plf.semantic_frame(seed, RES, RES),
                        "object_id_to_color": plf.dictionary(k, seed, targets)[0], "valid_moves_forward": k % 11})
        np.save(os.path.join(d, f"FloorPlan{s + 1}.npy"), pts)
    print("wrote", a.points // PER_SCENE, "scenes of", PER_SCENE, "points under", d)


def stats(a):
    path = sorted(glob.glob(os.path.join(a.dir, "**", "*kernel_stats.csv"), recursive=True))[0]
    rows = {}
    for r in csv.DictReader(open(path)):
        for key in ("semantic_labels_kernel", "resize_crop_kernel"):
            if key in r["Name"]:
                rows[key] = r
    frame_bytes = RES * RES * 3
    for key, r in rows.items():
        calls, avg, mn = int(r["Calls"]), float(r["AverageNs"]), float(r["MinNs"])
        print(f"{key:24s} {calls:4d} launches of {PER_SCENE} frames  avg {avg / 1e3:7.1f} us  min {mn / 1e3:7.1f} us  max {float(r['MaxNs']) / 1e3:7.1f} us"
              f"  input {PER_SCENE * frame_bytes / avg / 1e3:6.2f} TB/s avg = {PER_SCENE * frame_bytes / avg * 1e9 / HBM_ACHIEVABLE:5.1%} of 6.29 TB/s")
    if len(rows) == 2:
        print(f"labels / resize (avg per launch): {float(rows['semantic_labels_kernel']['AverageNs']) / float(rows['resize_crop_kernel']['AverageNs']):.3f}")


def ab(a):
    import torch
    from embodied_clip_amd import synthetic as syn
    from embodied_clip_amd.probe_data import ClipFeatureExtractor, build_thor_features
    from embodied_clip_amd.probe_labels import label_points, read_scene_file
    assert torch.cuda.is_available(), "needs the GPU"
    targets = json.load(open(TARGETS))
    scenes = {os.path.basename(p)[:-4]: read_scene_file(p) for p in sorted(glob.glob(os.path.join(a.dir, "ithor_scenes", "train", "*.npy")))}
    n = sum(len(v) for v in scenes.values())
    ex = ClipFeatureExtractor(syn.rn50_visual_state_dict(0), device="cuda:0", imagenet_state_dict=syn.tv_resnet_state_dict(0))
    labelled = {k: label_points(v, targets, ex.device, ex.batch) for k, v in scenes.items()}     # also the warm-up of the label path
    build_thor_features(ex, {k: v[:PER_SCENE] for k, v in list(labelled.items())[:1]})             # warm-up of the encoders

    def supplied():
        return build_thor_features(ex, labelled)

    def computed():
        return build_thor_features(ex, {k: label_points(v, targets, ex.device, ex.batch) for k, v in scenes.items()})

    def labels_only():
        return {k: label_points(v, targets, ex.device, ex.batch) for k, v in scenes.items()}

    t = {"supplied": [], "computed": [], "labels_only": []}
    for _ in range(a.reps):
        for name, fn in (("supplied", supplied), ("computed", computed), ("labels_only", labels_only)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            t[name].append(time.perf_counter() - t0)
            del out
    print("device:", torch.cuda.get_device_name(0))
    print(f"{n} points of {RES} x {RES}, {a.reps} alternating repetitions, seconds per pass over all points (host clock around synchronised work)")
    for name, v in t.items():
        v = sorted(v)
        print(f"{name:12s} median {v[len(v) // 2]:.4f} s  min {v[0]:.4f}  max {v[-1]:.4f}  = {n / v[len(v) // 2]:8.1f} points/s   all: "
              + " ".join(f"{x:.4f}" for x in t[name]))
    ms, mc = sorted(t["supplied"])[a.reps // 2], sorted(t["computed"])[a.reps // 2]
    print(f"computed / supplied = {mc / ms:.3f}  (+{(mc - ms) / n * 1e6:.1f} us per point)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["write", "stats", "ab"])
    ap.add_argument("dir")
    ap.add_argument("--points", type=int, default=640)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    {"write": write, "stats": stats, "ab": ab}[a.mode](a)
