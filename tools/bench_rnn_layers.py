"""Agents with a two-layer recurrent core (engine.Worker(rnn_layers=2): csrc/rnn_stack.hip on the act step) beside the one-layer
agents of the same build, both cells, alternating within each round.

  * the act step: one slice's policy act step at 32 and 128 actors (HIP events around `--act-reps` back-to-back act steps with
    reused tables -- the later steps of a rollout) and the number of kernel launches of ONE such act step (torch.profiler), with
    EC_RNN_STACK 1 (one launch per upper layer) and 0 (the general route: a GEMM and a step launch per upper layer).  The switch
    is read once per process, so every (round, setting) is a child process that measures L = 1 and L = 2 of both cells,
    alternating; the L = 1 lines of the two settings run the same code and show what one process differs from the next by;
  * the learn side, timed as bench.py times the flagship: warm-up iterations, then `steps` timed iterations between two device
    synchronisations -- env-frames/s and the update phase (HIP events around Worker.update, mean over the timed iterations).

One JSON line per measurement.

    python tools/bench_rnn_layers.py --actors 256 --rollout 128 --steps 3 --warmup 1 --rounds 2
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

from bench_lstm import act_launches, act_step_us  # noqa: E402  (tools/ is sys.path[0] when run as a program)

CONFIGS = [(cell, layers) for layers in (1, 2) for cell in ("GRU", "LSTM")]


def act_child(a) -> None:
    from embodied_clip_amd.engine import Worker
    for n in a.act_actors:
        for cell, layers in CONFIGS:
            w = Worker(n, T=2, device="cuda:0", seed=0, encoder_streams=1, rnn_type=cell, rnn_layers=layers)
            us = act_step_us(w, a.act_reps)
            line = {"measure": "act_step", "round": a.act_child, "rnn_stack": os.environ.get("EC_RNN_STACK", "1"), "cell": cell,
                    "layers": layers, "actors": w.slices[0].n, "act_step_us": round(us, 2)}
            if a.act_child == 0:
                names = act_launches(w)
                if names is not None:
                    line.update(launches=len(names), kernels=names)
            print(json.dumps(line), flush=True)
            del w
            torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--act-actors", nargs="+", type=int, default=[32, 128])
    ap.add_argument("--actors", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--update-repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--act-reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2, help="repeat the whole list (alternating the configurations)")
    ap.add_argument("--act-child", type=int, default=None, help="(child mode) only the act-step measurements; the value is the round")
    ap.add_argument("--skip", nargs="*", default=[], choices=("act", "iteration"))
    a = ap.parse_args()
    if a.act_child is not None:
        act_child(a)
        return
    if "act" not in a.skip:         # fresh child processes, before this one opens the GPU
        for rnd in range(a.rounds):
            for stack in ("1", "0"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--act-child", str(rnd), "--act-reps", str(a.act_reps),
                                    "--act-actors", *map(str, a.act_actors)], env={**os.environ, "EC_RNN_STACK": stack}, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"act-step measurement with EC_RNN_STACK={stack} failed with status {r.returncode}")
    if "iteration" in a.skip:
        return
    from embodied_clip_amd.engine import Worker
    for rnd in range(a.rounds):
        for cell, layers in CONFIGS:
            w = Worker(a.actors, T=a.rollout, device="cuda:0", seed=0, update_repeats=a.update_repeats, rnn_type=cell, rnn_layers=layers)
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
            print(json.dumps({"measure": "iteration", "round": rnd, "cell": cell, "layers": layers, "actors": a.actors, "rollout": a.rollout,
                              "update_repeats": a.update_repeats, "steps": a.steps, "slices": w.ns,
                              "policy_params": int(sum(k for _, k in w.policy.offsets.values())),
                              "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                              "env_frames_per_s": round(a.steps * a.rollout * a.actors / dt, 1),
                              "update_ms": round(sum(upd) / len(upd), 3)}), flush=True)
            del w
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
