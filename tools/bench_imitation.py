"""Imitation learning beside PPO in the engine of the same build, in ONE process, alternating.

  1. engine.Worker(loss="imitation", teacher_forcing=p 0.5) beside the default PPO worker at `--actors` (256 and 64), rollout 128:
     warm-up iterations, then `--rounds` rounds in which each worker runs `--steps` timed iterations between two device
     synchronisations (the two take turns, so a drift of the box hits both).  One JSON line per worker and round:
     env-frames/s and the update phase (HIP events around Worker.update, mean over the timed iterations; the GAE launch is
     outside them for both).
  2. one slice's act step at 128 and 32 actors per slice with teacher forcing on (p = 0.5: ec_policy_act, then
     ec_teacher_force) and off: HIP events around `--act-reps` back-to-back act steps with reused tables.
  3. the loss kernels alone at B = 16384: ec_imitation_loss for A = 6 (one thread per row) and A = 84 (one wave per row),
     with ec_ppo_loss_ex at A = 6 beside them: HIP events around `--loss-reps` launches, and the rows' bytes over that time.

    python tools/bench_imitation.py
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from embodied_clip_amd import imitation as il  # noqa: E402
from embodied_clip_amd import ppo  # noqa: E402
from embodied_clip_amd.engine import Worker  # noqa: E402

MODES = {"ppo": dict(), "imitation": dict(loss="imitation", teacher_forcing=lambda s: 0.5)}


def timed(w: Worker, steps: int):
    w.time_trunk, w.update_events, w.trunk_events = True, [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        w.iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    w.time_trunk = False
    upd = [e0.elapsed_time(e1) for e0, e1 in w.update_events]
    return dt, sum(upd) / len(upd)


def act_step_us(w: Worker, reps: int, p: float) -> float:
    sl = w.slices[0]
    w._tf_p = p
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


def loss_kernel_us(B: int, A: int, reps: int, which: str) -> float:
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(A)
    hv = torch.randn(B, A + 1, generator=g).to(dev)
    ids = torch.randint(0, A, (B,), generator=g).to(dev)
    mask = (torch.rand(B, generator=g) > 0.05).float().to(dev)
    dhv = torch.empty_like(hv)
    if which == "imitation":
        sums, scratch = torch.zeros(3, dtype=torch.float64, device=dev), il.imitation_scratch(dev)
        denom = il.expert_count(mask.view(1, B), 0, B)
        run = lambda: il.imitation_loss_raw(hv, ids, mask, A, denom=denom, dhv=dhv, sums=sums, scratch=scratch)   # noqa: E731
    else:
        sums = torch.zeros(4, dtype=torch.float64, device=dev)
        f = torch.randn(4, B, generator=g).to(dev)
        run = lambda: ppo.ppo_loss_raw(hv, ids, f[0], f[1], f[2], f[3], A, dhv=dhv, sums=sums)                     # noqa: E731
    for _ in range(10):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", type=int, nargs="+", default=[256, 64])
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--act-reps", type=int, default=200)
    ap.add_argument("--loss-reps", type=int, default=200)
    ap.add_argument("--loss-rows", type=int, default=16384)
    a = ap.parse_args()
    for n in a.actors:
        ws = {name: Worker(n, T=a.rollout, device="cuda:0", seed=0, **kw) for name, kw in MODES.items()}
        for w in ws.values():
            for _ in range(a.warmup):
                w.iteration()
        torch.cuda.synchronize()
        for r in range(a.rounds):
            for name, w in ws.items():
                dt, upd = timed(w, a.steps)
                print(json.dumps({"bench": "worker", "loss": name, "teacher_forcing_p": w._tf_p, "actors": n, "rollout": a.rollout,
                                  "round": r, "steps": a.steps, "slices": w.ns, "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                                  "env_frames_per_s": round(a.steps * a.rollout * n / dt, 1), "update_ms": round(upd, 3),
                                  "loss_info": {k: round(v, 5) for k, v in w.loss_info().items()}}), flush=True)
        del ws
        torch.cuda.empty_cache()
    for per_slice in (128, 32):
        w = Worker(2 * per_slice, T=2, device="cuda:0", seed=0, update_repeats=1, loss="imitation", teacher_forcing=lambda s: 0.5)
        assert w.slices[0].n == per_slice
        for r in range(2):
            for p in (0.5, 0.0):
                print(json.dumps({"bench": "act_step", "actors_per_slice": per_slice, "teacher_forcing_p": p, "round": r,
                                  "reps": a.act_reps, "act_step_us": round(act_step_us(w, a.act_reps, p), 2)}), flush=True)
        del w
        torch.cuda.empty_cache()
    B = a.loss_rows
    for r in range(2):
        for which, A in (("imitation", 6), ("imitation", 84), ("ppo", 6)):
            us = loss_kernel_us(B, A, a.loss_reps, which)
            mb = 2 * B * (A + 1) * 4 / 1e6          # the rows read and the gradient rows written
            print(json.dumps({"bench": "loss_kernel", "kernel": which, "B": B, "A": A, "round": r, "reps": a.loss_reps,
                              "us_per_call": round(us, 2), "hv_plus_dhv_MB": round(mb, 3),
                              "GB_per_s": round(mb / us * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
