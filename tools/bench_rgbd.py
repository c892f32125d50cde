"""The RGB-D agent (engine.Worker(depth=True): a depth tower through the one-channel stem beside the RGB tower, dual goal
encoder) beside the RGB agent of the same build at the same actor count.  Both workers live in one process and their timed
iterations ALTERNATE (rgb, rgbd, rgb, rgbd, ...), each between two device synchronisations, after `--warmup` iterations of
each.  One JSON line per agent: env-frames/s, the update phase (HIP events around Worker.update, mean over the timed
iterations) and one slice's policy act step (HIP events around `--act-reps` back-to-back act steps with reused tables).

`--stem FRAMES...`: the one-channel stem kernel (ec_stem_conv1_depth) beside what it replaces -- the three-channel expansion
pass plus ec_stem_conv1 -- on FRAMES 224 x 224 frames, HIP events around `--stem-reps` launches of each route, alternating
blocks; one JSON line per frame count with the bytes each route moves and the achieved TB/s.  (Kernel times proper come from
a kernel-trace run of this mode: profiles/rgbd_stem_kernel.txt.)

    python tools/bench_rgbd.py --actors 256 --rollout 128 --steps 3 --warmup 1
    python tools/bench_rgbd.py --stem 128 256
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from embodied_clip_amd import _lib, synthetic as syn  # noqa: E402
from embodied_clip_amd.engine import Worker  # noqa: E402

AGENTS = {"rgb": dict(), "rgbd": dict(depth=True)}


def act_step_us(w: Worker, reps: int) -> float:
    sl = w.slices[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with w._on(sl):
        w._act_slice(sl, 0)                       # tables built
        s = torch.cuda.current_stream()
        e0.record(s)
        for _ in range(reps):
            w._act_slice(sl, 0)
        e1.record(s)
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def bench_agents(a) -> None:
    ws = {name: Worker(a.actors, T=a.rollout, device="cuda:0", seed=0, update_repeats=a.update_repeats, **AGENTS[name])
          for name in a.agents}
    for w in ws.values():
        for _ in range(a.warmup):
            w.iteration()
        w.time_trunk, w.update_events, w.trunk_events = True, [], []
    torch.cuda.synchronize()
    dt = {name: 0.0 for name in ws}
    for _ in range(a.steps):
        for name, w in ws.items():
            t0 = time.perf_counter()
            w.iteration()
            torch.cuda.synchronize()
            dt[name] += time.perf_counter() - t0
    for name, w in ws.items():
        w.time_trunk = False
        upd = [e0.elapsed_time(e1) for e0, e1 in w.update_events]
        enc = [e0.elapsed_time(e1) for e0, e1 in w.trunk_events]
        print(json.dumps({"agent": name, "depth": bool(w.depth), "actors": a.actors, "rollout": a.rollout,
                          "update_repeats": a.update_repeats, "steps": a.steps, "slices": w.ns,
                          "policy_params": int(sum(n for _, n in w.policy.offsets.values())),
                          "feature_storage_gb": round(sum(sl.feat.numel() * sl.feat.element_size() * (2 if w.depth else 1)
                                                          for sl in w.slices) / 1e9, 2),
                          "ms_per_iteration": round(1e3 * dt[name] / a.steps, 2),
                          "env_frames_per_s": round(a.steps * a.rollout * a.actors / dt[name], 1),
                          "encode_ms_per_slice_step": round(sum(enc) / len(enc), 3),
                          "update_ms": round(sum(upd) / len(upd), 3),
                          "act_step_us": round(act_step_us(w, a.act_reps), 2), "act_step_actors": w.slices[0].n}), flush=True)


def bench_stem(a) -> None:
    from embodied_clip_amd.encoder import RN50Trunk
    lib = _lib.load()
    dev = torch.device("cuda:0")
    trunk = RN50Trunk(syn.rn50_visual_state_dict(0), device=dev)
    sc = trunk.stem_w.shape[1]
    R = trunk.input_resolution
    sp = _lib.stream_ptr()
    for B in a.stem:
        depth = syn.normalize_depth(syn.synthetic_depth(1005, B, R)).to(dev).contiguous()          # [B,R,R,1]
        rgb3 = torch.empty((B, R, R, 3), dtype=torch.float32, device=dev)
        o1 = torch.empty((B, R // 2, R // 2, sc), dtype=torch.bfloat16, device=dev)
        o3 = torch.empty_like(o1)

        def one():
            _lib.check(lib.ec_stem_conv1_depth(depth.data_ptr(), 1.0, 0.0, trunk.stem_w9.data_ptr(), trunk.bias.data_ptr(),
                                               o1.data_ptr(), B, R, R, sc, sp), "ec_stem_conv1_depth")

        def three():
            rgb3.copy_(depth.expand(-1, -1, -1, 3))                                              # the expansion pass
            _lib.check(lib.ec_stem_conv1(rgb3.data_ptr(), trunk.stem_w.data_ptr(), trunk.bias.data_ptr(), o3.data_ptr(),
                                         B, R, R, sc, sp), "ec_stem_conv1")

        for _ in range(5):
            one(); three()
        torch.cuda.synchronize()
        tot = {"one": 0.0, "three": 0.0}
        for _ in range(a.stem_blocks):
            for tag, fn in (("one", one), ("three", three)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.stem_reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                tot[tag] += e0.elapsed_time(e1)
        n = a.stem_blocks * a.stem_reps
        us1, us3 = 1e3 * tot["one"] / n, 1e3 * tot["three"] / n
        px = B * R * R
        bytes1 = px * 4 + px // 4 * sc * 2                           # frame in, bf16 output out
        bytes3 = px * 4 + 2 * px * 12 + px // 4 * sc * 2             # expansion (read 1, write 3) + RGB kernel (read 3, write out)
        rel = ((o1.float() - o3.float()).norm() / o3.float().norm()).item()
        print(json.dumps({"stem_frames": B, "res": R, "channels": sc,
                          "depth_stem_us": round(us1, 2), "expand_plus_rgb_stem_us": round(us3, 2),
                          "depth_stem_bytes": bytes1, "expand_plus_rgb_stem_bytes": bytes3,
                          "depth_stem_tb_s": round(bytes1 / us1 / 1e6, 3), "achievable_tb_s": 6.29,
                          "speedup": round(us3 / us1, 2), "rel_l2_between_routes": float(f"{rel:.3e}")}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", nargs="+", choices=sorted(AGENTS), default=["rgb", "rgbd"])
    ap.add_argument("--actors", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--update-repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--act-reps", type=int, default=200)
    ap.add_argument("--stem", type=int, nargs="+", default=None, metavar="FRAMES", help="time the stem kernels instead of the agents")
    ap.add_argument("--stem-reps", type=int, default=50)
    ap.add_argument("--stem-blocks", type=int, default=4)
    a = ap.parse_args()
    if a.stem:
        bench_stem(a)
    else:
        bench_agents(a)


if __name__ == "__main__":
    main()
