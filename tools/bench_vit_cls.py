"""The ViT's class embedding (ViTEmbedder.embed_cls: ec_vit_embed_cls) on its two routes, and the agent built on it.

  * one slice's encode step at `--frames` frames (ViT-B/32, 50 tokens) and `--frames16` frames (a ViT-B/16-geometry tower, 197
    tokens), both 12 blocks of width 768 (11 run): `--reps` back-to-back calls between two HIP events, and the kernel launches of
    ONE call (torch.profiler), for
      embed_cls        under the child's EC_VIT_CLS_TAIL: 1 the CLS-only last block, 0 the general route
      forward+row0     forward + to_f32(class_emb_only=True): the general route spelled out -- the parent commit's only way
    The switch is read once per process, so every (round, setting) is a child process; inside a child the two alternate (a, b, a,
    b), and `forward+row0` runs the same code under both settings: what it differs by between children is the spread;
  * the rel-L2 between the two routes' embeddings at each size (child with the tail on: embed_cls against forward+row0);
  * rows_gemm (ec_gemm_rows_bf16) alone beside ec_gemm_bf16 on the CLS chain's four shapes (q, out_proj + residual, c_fc +
    QuickGELU, c_proj + residual; D = 768) at 32 and 128 rows;
  * whole workers, timed as bench.py times the flagship: warm-up iterations, then `steps` timed iterations between two device
    synchronisations -- Worker(net="pooled", encoder="vit", pooling="cls", sensors=(2, 2)) under both settings of the switch,
    Worker(encoder="vit") (the token-map agent of BASELINE config 3) and the pooled RN50 avgpool worker, at `--actors` x
    `--rollout`: env-frames/s, the update phase (HIP events around Worker.update) and the rollout feature storage.

One JSON line per measurement.

    python tools/bench_vit_cls.py --rounds 2
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

CLS_WORKER = dict(net="pooled", encoder="vit", pooling="cls", sensors=(2, 2))
OTHER_WORKERS = {"vit-token-map": dict(encoder="vit"), "pooled-rn50-avgpool": dict(net="pooled", pooling="avgpool", sensors=(2, 2))}
NONE, QUICKGELU = 0, 2


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


def switch() -> str:
    return os.environ.get("EC_VIT_CLS_TAIL", "unset")


def encode_child(a) -> None:
    from embodied_clip_amd import _lib, synthetic as syn
    from embodied_clip_amd.encoder import ViTEmbedder
    dev = torch.device("cuda:0")
    lib = _lib.load()
    rnd = a.encode_child
    for tower, patch, sizes in (("ViT-B/32", 32, a.frames), ("ViT-B/16-geometry", 16, a.frames16)):
        vit = ViTEmbedder(syn.vit_visual_state_dict(0, patch_size=patch), device=dev)
        for n in sizes:
            rgb = syn.synthetic_rgb(1000, 4).repeat((n + 3) // 4, 1, 1, 1)[:n].contiguous().to(dev)
            out = torch.empty(n, vit.D, device=dev)
            tok = torch.empty(n, vit.L, vit.D, dtype=torch.bfloat16, device=dev)

            def new():
                vit.embed_cls(rgb, out)

            def spelled():
                vit.to_f32(vit.forward(rgb, tok), class_emb_only=True)
            for half in range(2):          # a, b, a, b
                for route, fn in (("embed_cls", new), ("forward+row0", spelled)):
                    line = {"measure": "encode_step", "round": rnd, "pass": half, "EC_VIT_CLS_TAIL": switch(), "route": route, "tower": tower,
                            "tokens": vit.L, "frames": n, "reps": a.reps, "ms_per_step": round(timed(fn, a.reps), 4)}
                    if rnd == 0 and half == 0:
                        names = launches(fn)
                        if names is not None:
                            line.update(launches=len(names))
                    print(json.dumps(line), flush=True)
            if rnd == 0:
                new()
                e = out.clone()
                ref = vit.to_f32(vit.forward(rgb, tok), class_emb_only=True)
                print(json.dumps({"measure": "route_agreement", "EC_VIT_CLS_TAIL": switch(), "tower": tower, "frames": n,
                                  "rel_l2_embed_cls_vs_forward_row0": float((e - ref).norm() / ref.norm())}), flush=True)
        del vit
        torch.cuda.empty_cache()
    if switch() != "1":
        return
    # rows_gemm alone beside the tile GEMM on the chain's shapes (the switch does not reach either)
    D = 768
    g = torch.Generator().manual_seed(1)
    for M in a.gemm_rows:
        for name, N, K, act, res in (("q", D, D, NONE, False), ("out_proj+res", D, D, NONE, True), ("c_fc+gelu", 4 * D, D, QUICKGELU, False),
                                     ("c_proj+res", D, 4 * D, NONE, True)):
            A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
            W = (torch.randn(N, K, generator=g) * K ** -0.5).to(torch.bfloat16).to(dev)
            b = torch.randn(N, generator=g).to(dev)
            r = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev) if res else None
            o1, o2 = (torch.empty(M, N, dtype=torch.bfloat16, device=dev) for _ in range(2))

            def rows():
                _lib.check(lib.ec_gemm_rows_bf16(A.data_ptr(), K, W.data_ptr(), b.data_ptr(), _lib.ptr(r), N, o1.data_ptr(), N, M, N, K, act, 0,
                                                 _lib.stream_ptr()), "ec_gemm_rows_bf16")

            def tiles():
                _lib.check(lib.ec_gemm_bf16(A.data_ptr(), W.data_ptr(), b.data_ptr(), _lib.ptr(r), o2.data_ptr(), M, N, K, act, _lib.stream_ptr()),
                           "ec_gemm_bf16")
            for half in range(2):
                for route, fn in (("ec_gemm_rows_bf16", rows), ("ec_gemm_bf16", tiles)):
                    print(json.dumps({"measure": "cls_gemm", "round": rnd, "pass": half, "shape": name, "M": M, "N": N, "K": K, "route": route,
                                      "us_per_call": round(1e3 * timed(fn, 4 * a.reps), 2)}), flush=True)


def one_worker(a, rnd: int, kind: str, kw: dict, actors: int) -> None:
    from embodied_clip_amd.engine import Worker
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
    feat_bytes = sum(sl.feat.numel() * sl.feat.element_size() for sl in w.slices)
    print(json.dumps({"measure": "iteration", "round": rnd, "agent": kind, "EC_VIT_CLS_TAIL": switch(), "actors": actors, "rollout": a.rollout,
                      "update_repeats": a.update_repeats, "steps": a.steps, "slices": w.ns,
                      "rollout_feature_MB": round(feat_bytes / 2 ** 20, 1), "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                      "env_frames_per_s": round(a.steps * a.rollout * actors / dt, 1),
                      "update_ms": round(sum(upd) / len(upd), 3) if upd else None}), flush=True)
    del w
    torch.cuda.empty_cache()


def worker_child(a) -> None:
    rnd = a.worker_child
    for actors in a.actors:
        one_worker(a, rnd, "pooled-vit-cls", CLS_WORKER, actors)
        if switch() == "1":        # the agents the switch does not reach: once per round
            for kind, kw in OTHER_WORKERS.items():
                one_worker(a, rnd, kind, kw, actors)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", nargs="+", type=int, default=[32, 64, 128], help="frames of one slice's encode step, ViT-B/32")
    ap.add_argument("--frames16", nargs="+", type=int, default=[32, 128], help="... of the ViT-B/16-geometry tower")
    ap.add_argument("--gemm-rows", nargs="+", type=int, default=[32, 128], help="rows of the GEMM-alone measurement")
    ap.add_argument("--actors", nargs="+", type=int, default=[256, 64], help="actors of the whole-worker measurements")
    ap.add_argument("--update-repeats", type=int, default=4)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=2, help="repeat the whole list")
    ap.add_argument("--encode-child", type=int, default=None, help="(child mode) only the encode-step measurements; the value is the round")
    ap.add_argument("--worker-child", type=int, default=None, help="(child mode) only the whole-worker measurements; the value is the round")
    ap.add_argument("--skip", nargs="*", default=[], choices=("encode", "iteration"))
    a = ap.parse_args()
    if a.encode_child is not None:
        encode_child(a)
        return
    if a.worker_child is not None:
        worker_child(a)
        return
    me = [sys.executable, os.path.abspath(__file__)]
    common = ["--reps", str(a.reps), "--frames", *map(str, a.frames), "--frames16", *map(str, a.frames16), "--gemm-rows", *map(str, a.gemm_rows),
              "--actors", *map(str, a.actors), "--update-repeats", str(a.update_repeats), "--rollout", str(a.rollout), "--steps", str(a.steps),
              "--warmup", str(a.warmup)]
    for what, flag in (("encode", "--encode-child"), ("iteration", "--worker-child")):
        if what in a.skip:
            continue
        for rnd in range(a.rounds):
            for setting in ("1", "0"):
                r = subprocess.run(me + [flag, str(rnd)] + common, env={**os.environ, "EC_VIT_CLS_TAIL": setting}, timeout=900)
                if r.returncode != 0:
                    raise SystemExit(f"{what} measurement with EC_VIT_CLS_TAIL={setting} failed with status {r.returncode}")


if __name__ == "__main__":
    main()
