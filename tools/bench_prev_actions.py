"""The agent with a previous-action embedding (engine.Worker(prev_actions=E): the table row added in the input projection's fold,
the binned ordered gradient in the backward) beside the agent without it, of the same build.

  * the act step: one slice's policy act step at 32 and 128 actors (HIP events around `--act-reps` back-to-back act steps with
    reused tables -- the later steps of a rollout), and one act step that rebuilds the tables (the first after a parameter update);
  * the learn side, timed as bench.py times the flagship: warm-up iterations, then `steps` timed iterations between two device
    synchronisations -- env-frames/s and the update phase (HIP events around Worker.update, mean over the timed iterations).

One JSON line per measurement.

    python tools/bench_prev_actions.py --actors 256 --rollout 128 --steps 3 --warmup 1
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


def act_step_us(w: Worker, reps: int):
    """-> (us per act step with reused tables, us of one act step that rebuilds them)"""
    sl = w.slices[0]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with w._on(sl):
        w._act_slice(sl, 0)                       # tables built
        s = torch.cuda.current_stream()
        ev[0].record(s)
        for _ in range(reps):
            w._act_slice(sl, 0)
        ev[1].record(s)
        w.invalidate_act_tables()
        ev[2].record(s)
        w._act_slice(sl, 0)
        ev[3].record(s)
    torch.cuda.synchronize()
    return 1e3 * ev[0].elapsed_time(ev[1]) / reps, 1e3 * ev[2].elapsed_time(ev[3])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", nargs="+", type=int, default=[0, 6, 32], help="embedding widths (0: the agent without)")
    ap.add_argument("--act-actors", nargs="+", type=int, default=[32, 128])
    ap.add_argument("--actors", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--update-repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--act-reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=1, help="repeat the whole list (alternating the widths)")
    a = ap.parse_args()
    for _round in range(a.rounds):
        for n in a.act_actors:
            for E in a.widths:
                w = Worker(n, T=2, device="cuda:0", seed=0, encoder_streams=1, prev_actions=E)
                reuse, rebuild = act_step_us(w, a.act_reps)
                print(json.dumps({"measure": "act_step", "prev_actions": E, "actors": w.slices[0].n, "act_step_us": round(reuse, 2),
                                  "act_step_rebuild_us": round(rebuild, 2)}), flush=True)
                del w
                torch.cuda.empty_cache()
        for E in a.widths:
            w = Worker(a.actors, T=a.rollout, device="cuda:0", seed=0, update_repeats=a.update_repeats, prev_actions=E)
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
            print(json.dumps({"measure": "iteration", "prev_actions": E, "actors": a.actors, "rollout": a.rollout,
                              "update_repeats": a.update_repeats, "steps": a.steps, "slices": w.ns,
                              "policy_params": int(sum(k for _, k in w.policy.offsets.values())),
                              "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                              "env_frames_per_s": round(a.steps * a.rollout * a.actors / dt, 1),
                              "update_ms": round(sum(upd) / len(upd), 3)}), flush=True)
            del w
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
