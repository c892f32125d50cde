"""Throughput of the ImageNet-feature agents (engine.Worker with encoder="imagenet_rn18" | "imagenet_rn34" |
"imagenet_rn50"), timed as bench.py times the CLIP agents: warm-up iterations, then `steps` timed iterations between two
device synchronisations; env-frames/s = steps * rollout * actors / wall clock.  One JSON line per (encoder, actors).

    python tools/bench_imagenet_agent.py --encoder imagenet_rn18 imagenet_rn50 --actors 256 32 --steps 3 --warmup 1
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from embodied_clip_amd.engine import IMAGENET_ENCODERS, Worker  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder", nargs="+", choices=sorted(IMAGENET_ENCODERS), default=["imagenet_rn18"])
    ap.add_argument("--actors", type=int, nargs="+", default=[256])
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--update-repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    for enc in a.encoder:
        for n in a.actors:
            w = Worker(n, T=a.rollout, device="cuda:0", seed=0, update_repeats=a.update_repeats, encoder=enc)
            for _ in range(a.warmup):
                w.iteration()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                w.iteration()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"encoder": enc, "actors": n, "rollout": a.rollout, "update_repeats": a.update_repeats,
                              "steps": a.steps, "slices": w.ns, "feat_channels": w.C, "plan_hash": w.slices[0].enc.plan_hash(),
                              "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                              "env_frames_per_s": round(a.steps * a.rollout * n / dt, 1)}), flush=True)
            del w
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
