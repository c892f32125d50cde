"""The pooled net's RGB-D encoder (RN50Trunk.embed_rgbd: ec_rn50_embed_rgbd + ec_spatial_mean_pair_bf16) beside what it replaces.

  * one slice's encode step at `--pairs` pairs (224 x 224 frames, CLIP RN50, the conv8 threshold the engine gives a slice of that
    size): `--reps` back-to-back steps between two HIP events, and the kernel launches of ONE step (torch.profiler), for
      joint     embed_rgbd with EC_RGBD_JOINT=1: the plan once at 2 n frames
      composed  embed_rgbd with EC_RGBD_JOINT=0: the plan at n frames on the RGB chunk, again on the depth chunk, the pair kernel
      parent    the way to the same vector without this entry point: forward + forward_depth + two ec_spatial_mean_bf16 + one add
    The switch is read once per process, so every (round, setting) is a child process; each child also measures `parent`, which
    runs the same code under both settings and shows what one process differs from the next by;
  * the pair kernel alone at 32 / 128 pairs of 2048 x 7 x 7 maps against two ec_spatial_mean_bf16 + the add, with the achieved
    bytes/s (bytes = both maps read + the vectors written);
  * whole workers, timed as bench.py times the flagship: warm-up iterations, then `steps` timed iterations between two device
    synchronisations -- the pooled RGB-D worker, the pooled RGB avgpool worker and the two-tower Worker(depth=True), at
    `--actors` x `--rollout`: env-frames/s, the update phase (HIP events around Worker.update) and the rollout feature storage.

One JSON line per measurement.

    python tools/bench_rgbd_pooled.py --rounds 2
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_lstm import kernel_events, kernel_name  # noqa: E402  (tools/ is sys.path[0] when run as a program)

WORKERS = {"pooled-rgbd": dict(net="pooled", pooling="avgpool", depth=True, sensors=(2, 2)),
           "pooled-rgb-avgpool": dict(net="pooled", pooling="avgpool", sensors=(2, 2)),
           "two-tower-rgbd": dict(depth=True)}


def timed(fn, reps: int) -> float:
    """ms per call: `reps` back-to-back calls between two HIP events, after three warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launches(fn):
    ev = kernel_events(fn)
    return None if ev is None else [kernel_name(n) for n, _ in ev]


def encode_child(a) -> None:
    from embodied_clip_amd import _lib, synthetic as syn
    from embodied_clip_amd.encoder import RN50Trunk
    dev = torch.device("cuda:0")
    lib = _lib.load()
    joint = os.environ.get("EC_RGBD_JOINT", "1") != "0"
    trunk = RN50Trunk(syn.rn50_visual_state_dict(0), device=dev)
    S, Cc = trunk.out_spatial, trunk.out_channels
    for n in a.pairs:
        min_tiles = 50 if n >= 128 else (75 if n >= 64 else 0)        # engine._build_slices for a slice of n frames, two slices
        trunk.set_conv8_min_tiles(min_tiles)
        rgb = syn.synthetic_rgb(1000, 4).repeat((n + 3) // 4, 1, 1, 1)[:n].contiguous().to(dev)
        dep = syn.normalize_depth(syn.synthetic_depth(1005, 4)).repeat((n + 3) // 4, 1, 1, 1)[:n].contiguous().to(dev)
        out = torch.empty(n, Cc, device=dev)
        ma, mb = (torch.empty(n, S, S, Cc, dtype=torch.bfloat16, device=dev) for _ in range(2))
        va, vb = torch.empty(n, Cc, device=dev), torch.empty(n, Cc, device=dev)

        def new():
            trunk.embed_rgbd(rgb, dep, out)

        def parent():
            trunk.forward(rgb, ma)
            trunk.forward_depth(dep, mb)
            _lib.check(lib.ec_spatial_mean_bf16(ma.data_ptr(), va.data_ptr(), n, S * S, Cc, _lib.stream_ptr()), "ec_spatial_mean_bf16")
            _lib.check(lib.ec_spatial_mean_bf16(mb.data_ptr(), vb.data_ptr(), n, S * S, Cc, _lib.stream_ptr()), "ec_spatial_mean_bf16")
            torch.add(va, vb, out=va)
        for route, fn in (("joint" if joint else "composed", new), ("parent", parent)):
            line = {"measure": "encode_step", "round": a.encode_child, "rgbd_joint": int(joint), "route": route, "pairs": n,
                    "conv8_min_tiles": min_tiles, "reps": a.reps, "ms_per_step": round(timed(fn, a.reps), 4)}
            if a.encode_child == 0:
                names = launches(fn)
                if names is not None:
                    line.update(launches=len(names))
            print(json.dumps(line), flush=True)
        if a.encode_child == 0:     # the two ways agree on the vector
            new()
            e = out.clone()
            parent()
            print(json.dumps({"measure": "encode_step_agreement", "pairs": n, "rgbd_joint": int(joint),
                              "rel_l2_new_vs_parent": float((e - va).norm() / va.norm())}), flush=True)
    if joint:       # the pair kernel alone (the switch does not reach it)
        for n in a.pool_pairs:
            g = torch.Generator().manual_seed(n)
            ma, mb = (torch.randn(n, S * S, Cc, generator=g).to(torch.bfloat16).to(dev) for _ in range(2))
            va, vb, out = (torch.empty(n, Cc, device=dev) for _ in range(3))

            def pair():
                _lib.check(lib.ec_spatial_mean_pair_bf16(ma.data_ptr(), mb.data_ptr(), out.data_ptr(), n, S * S, Cc, _lib.stream_ptr()),
                           "ec_spatial_mean_pair_bf16")

            def two_and_add():
                _lib.check(lib.ec_spatial_mean_bf16(ma.data_ptr(), va.data_ptr(), n, S * S, Cc, _lib.stream_ptr()), "ec_spatial_mean_bf16")
                _lib.check(lib.ec_spatial_mean_bf16(mb.data_ptr(), vb.data_ptr(), n, S * S, Cc, _lib.stream_ptr()), "ec_spatial_mean_bf16")
                torch.add(va, vb, out=va)
            nbytes = 2 * ma.numel() * 2 + out.numel() * 4
            for name, fn in (("ec_spatial_mean_pair_bf16", pair), ("2 x ec_spatial_mean_bf16 + add", two_and_add)):
                ms = timed(fn, 4 * a.reps)
                print(json.dumps({"measure": "pair_pool", "round": a.encode_child, "route": name, "pairs": n, "us_per_call": round(1e3 * ms, 2),
                                  "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)}), flush=True)


def iteration(a, rnd: int) -> None:
    from embodied_clip_amd.engine import Worker
    for actors in a.actors:
        for kind, kw in WORKERS.items():
            core = dict(rnn_type="LSTM", rnn_layers=2, prev_actions=32) if kind.startswith("pooled") else {}
            w = Worker(actors, T=a.rollout, device="cuda:0", seed=0, update_repeats=a.update_repeats, **core, **kw)
            for _ in range(a.warmup):
                w.iteration()
            torch.cuda.synchronize()
            w.time_trunk, w.update_events, w.trunk_events = True, [], []      # (as bench.py: HIP events around the update phase)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                w.iteration()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            w.time_trunk = False
            upd = [e0.elapsed_time(e1) for e0, e1 in w.update_events]
            feat_bytes = sum(sl.feat.numel() * sl.feat.element_size() * (2 if sl.feat2 is not None else 1) for sl in w.slices)
            print(json.dumps({"measure": "iteration", "round": rnd, "agent": kind, "actors": actors, "rollout": a.rollout,
                              "update_repeats": a.update_repeats, "steps": a.steps, "slices": w.ns,
                              "rollout_feature_MB": round(feat_bytes / 2 ** 20, 1), "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                              "env_frames_per_s": round(a.steps * a.rollout * actors / dt, 1),
                              "update_ms": round(sum(upd) / len(upd), 3) if upd else None}), flush=True)
            del w
            torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", nargs="+", type=int, default=[32, 64, 128], help="pairs of one slice's encode step")
    ap.add_argument("--pool-pairs", nargs="+", type=int, default=[32, 128], help="pairs of the pair kernel's own measurement")
    ap.add_argument("--actors", nargs="+", type=int, default=[256, 64], help="actors of the whole-worker measurements")
    ap.add_argument("--update-repeats", type=int, default=4)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2, help="repeat the whole list")
    ap.add_argument("--encode-child", type=int, default=None, help="(child mode) only the encode-step measurements; the value is the round")
    ap.add_argument("--skip", nargs="*", default=[], choices=("encode", "iteration"))
    a = ap.parse_args()
    if a.encode_child is not None:
        encode_child(a)
        return
    if "encode" not in a.skip:        # fresh child processes, before this one opens the GPU
        for rnd in range(a.rounds):
            for setting in ("1", "0"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--encode-child", str(rnd), "--reps", str(a.reps), "--pairs",
                                    *map(str, a.pairs), "--pool-pairs", *map(str, a.pool_pairs)], env={**os.environ, "EC_RGBD_JOINT": setting},
                                   timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"encode-step measurement with EC_RGBD_JOINT={setting} failed with status {r.returncode}")
    if "iteration" not in a.skip:
        for rnd in range(a.rounds):
            iteration(a, rnd)


if __name__ == "__main__":
    main()
