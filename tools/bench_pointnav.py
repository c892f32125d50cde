"""The PointNav agent (engine.Worker(goal_in=2, num_actions=4): coordinate goals through embed_goal and the per-frame bias
rows) beside the ObjectNav agent of the same build, timed as bench.py times the flagship: warm-up iterations, then `steps`
timed iterations between two device synchronisations.  One JSON line per agent: env-frames/s, the update phase (HIP events
around Worker.update, mean over the timed iterations) and one slice's policy act step (HIP events around `--act-reps`
back-to-back act steps with reused tables, after the timed iterations).

    python tools/bench_pointnav.py --actors 256 --rollout 128 --steps 3 --warmup 1
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from embodied_clip_amd.engine import Worker  # noqa: E402

AGENTS = {"objectnav": dict(), "pointnav": dict(goal_in=2, num_actions=4)}


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--agents", nargs="+", choices=sorted(AGENTS), default=["objectnav", "pointnav"])
    ap.add_argument("--actors", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--update-repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--act-reps", type=int, default=200)
    a = ap.parse_args()
    for name in a.agents:
        w = Worker(a.actors, T=a.rollout, device="cuda:0", seed=0, update_repeats=a.update_repeats, **AGENTS[name])
        for _ in range(a.warmup):
            w.iteration()
        torch.cuda.synchronize()
        w.time_trunk, w.update_events, w.trunk_events = True, [], []
        t0 = time.perf_counter()
        for _ in range(a.steps):
            w.iteration()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        w.time_trunk = False
        upd = [e0.elapsed_time(e1) for e0, e1 in w.update_events]
        print(json.dumps({"agent": name, "goal_in": w.goal_in, "num_actions": w.A, "actors": a.actors, "rollout": a.rollout,
                          "update_repeats": a.update_repeats, "steps": a.steps, "slices": w.ns,
                          "policy_params": int(sum(n for _, n in w.policy.offsets.values())),
                          "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                          "env_frames_per_s": round(a.steps * a.rollout * a.actors / dt, 1),
                          "update_ms": round(sum(upd) / len(upd), 3),
                          "act_step_us": round(act_step_us(w, a.act_reps), 2), "act_step_actors": w.slices[0].n}), flush=True)
        del w
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
