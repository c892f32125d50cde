"""An 84-action agent (the width of the reference's rearrangement experiment) through the one-call act step and the wide loss
kernel, beside the multi-call route of the same build, in ONE process, alternating.

  1. one slice's act step at 84 actions, 32 and 128 actors per slice, teacher forcing p = 0.5 and off: ec_policy_act_ex (the
     wide heads launch computes the logits, samples and forces) against the forward with the GEMM heads, ec_sample_actions
     and ec_teacher_force -- the route a worker built under EC_ACT_FUSED_SAMPLE=0 takes, and the only one before the wide
     kernels.  HIP events around `--act-reps` back-to-back act steps with reused tables; the two routes take turns.
  2. the wide PPO loss alone at B = 16384 for A = 17 and 84, with ec_imitation_loss on the same rows beside it.
  3. Worker(num_actions=84, loss="imitation", teacher_forcing=p 0.5) at `--actors`, rollout 128: the same worker object with
     the one-call act step on and off, rounds alternating -- env-frames/s and the update phase (HIP events).

    python tools/bench_wide_actions.py
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

A = 84


def act_step_us(w: Worker, reps: int, p: float, wide: bool) -> float:
    sl = w.slices[0]
    w._tf_p, w._act_wide = p, wide
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


def loss_kernel_us(B: int, A_: int, reps: int, which: str) -> float:
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(A_)
    hv = torch.randn(B, A_ + 1, generator=g).to(dev)
    ids = torch.randint(0, A_, (B,), generator=g).to(dev)
    mask = (torch.rand(B, generator=g) > 0.05).float().to(dev)
    dhv = torch.empty_like(hv)
    if which == "imitation":
        sums, scratch = torch.zeros(3, dtype=torch.float64, device=dev), il.imitation_scratch(dev)
        denom = il.expert_count(mask.view(1, B), 0, B)
        run = lambda: il.imitation_loss_raw(hv, ids, mask, A_, denom=denom, dhv=dhv, sums=sums, scratch=scratch)   # noqa: E731
    else:
        sums, scratch = torch.zeros(4, dtype=torch.float64, device=dev), ppo.ppo_wide_scratch(dev)
        f = torch.randn(4, B, generator=g).to(dev)
        run = lambda: ppo.ppo_loss_raw(hv, ids, f[0], f[1], f[2], f[3], A_, dhv=dhv, sums=sums, scratch=scratch)   # noqa: E731
    for _ in range(10):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def timed(w: Worker, steps: int):
    w.update_events = []
    w.time_trunk = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        w.iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    w.time_trunk = False
    upd = [e0.elapsed_time(e1) for e0, e1 in w.update_events]
    return dt, sum(upd) / len(upd)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--actors", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--act-reps", type=int, default=200)
    ap.add_argument("--loss-reps", type=int, default=200)
    ap.add_argument("--loss-rows", type=int, default=16384)
    ap.add_argument("--skip-worker", action="store_true")
    a = ap.parse_args()
    for per_slice in (32, 128):
        w = Worker(2 * per_slice, T=2, device="cuda:0", seed=0, update_repeats=1, num_actions=A, loss="imitation",
                   teacher_forcing=lambda s: 0.5)
        assert w.slices[0].n == per_slice and w._act_wide
        for r in range(a.rounds):
            for p in (0.5, 0.0):
                for wide in (True, False):
                    print(json.dumps({"bench": "act_step", "num_actions": A, "actors_per_slice": per_slice, "teacher_forcing_p": p,
                                      "route": "act_ex" if wide else "forward+sample+force", "round": r, "reps": a.act_reps,
                                      "act_step_us": round(act_step_us(w, a.act_reps, p, wide), 2)}), flush=True)
        del w
        torch.cuda.empty_cache()
    B = a.loss_rows
    for r in range(2):
        for which, A_ in (("ppo_wide", 17), ("ppo_wide", A), ("imitation", 17), ("imitation", A)):
            us = loss_kernel_us(B, A_, a.loss_reps, which)
            mb = 2 * B * (A_ + 1) * 4 / 1e6          # the rows read and the gradient rows written
            print(json.dumps({"bench": "loss_kernel", "kernel": which, "B": B, "A": A_, "round": r, "reps": a.loss_reps,
                              "us_per_call": round(us, 2), "hv_plus_dhv_MB": round(mb, 3), "GB_per_s": round(mb / us * 1e3, 1)}),
                  flush=True)
    if a.skip_worker:
        return
    w = Worker(a.actors, T=a.rollout, device="cuda:0", seed=0, num_actions=A, loss="imitation", teacher_forcing=lambda s: 0.5)
    w.iteration()
    for r in range(a.rounds):
        for wide in (True, False):
            w._act_wide = wide
            dt, upd = timed(w, a.steps)
            print(json.dumps({"bench": "worker", "num_actions": A, "loss": "imitation", "teacher_forcing_p": w._tf_p,
                              "route": "act_ex" if wide else "forward+sample+force", "actors": a.actors, "rollout": a.rollout,
                              "round": r, "steps": a.steps, "slices": w.ns, "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                              "env_frames_per_s": round(a.steps * a.rollout * a.actors / dt, 1), "update_ms": round(upd, 3)}),
                  flush=True)


if __name__ == "__main__":
    main()
