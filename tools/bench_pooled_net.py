"""The pooled-embedding net (PolicyHandle.pooled: csrc/pooled_net.hip on the act step) beside the goal-encoder agent with the same
core -- LSTM x 2, previous-action embedding 32.

  * the act step: `--act-reps` back-to-back act steps with reused tables between two HIP events, at 32 and 128 actors, and the
    number of kernel launches of ONE such act step (torch.profiler), with EC_POOLED_ACT 1 (pooled_fc_act_kernel +
    pooled_step0_kernel) and 0 (the general route).  The switch is read once per process, so every (round, setting) is a child
    process that measures both agents, alternating; the goal-encoder lines of the two settings run the same code and show what one
    process differs from the next by;
  * one slice's learn pass (forward with EC_POLICY_LEARN, then the backward) at `--rollout` x `--slice-actors` rows, HIP events
    around `--steps` passes after `--warmup`;
  * the whole worker, timed as bench.py times the flagship (engine.Worker(net="pooled", ...) beside the goal-encoder Worker):
    warm-up iterations, then `steps` timed iterations between two device synchronisations -- env-frames/s and the update phase
    (HIP events around Worker.update, mean over the timed iterations) at `--actors` x `--rollout`.

One JSON line per measurement.

    python tools/bench_pooled_net.py --rounds 2
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_lstm import kernel_events, kernel_name  # noqa: E402  (tools/ is sys.path[0] when run as a program)

CORE = dict(rnn_type="LSTM", rnn_layers=2)
AGENTS = ("pooled-attnpool", "pooled-avgpool", "goal-encoder")


class Agent:
    """A handle, its parameters and one batch of synthetic inputs for `rows` = T * N frames."""

    def __init__(self, kind: str, T: int, N: int, dev):
        from embodied_clip_amd import synthetic as syn
        from embodied_clip_amd.policy import PolicyHandle
        self.kind, self.T, self.N = kind, T, N
        g = torch.Generator().manual_seed(3)
        rows = T * N
        if kind.startswith("pooled"):
            D = 1024 if kind.endswith("attnpool") else 2048
            self.h = PolicyHandle.pooled(D, hidden=512, num_goals=12, sensors=(2, 2), num_actions=6, prev_action_dims=32, **CORE)
            sd = syn.policy_state_dict(0, pooled=self.h.pooled_cfg)
            self.feat = torch.randn(rows, D, generator=g).to(dev)
            self.kw = dict(sensors=torch.randn(rows, 4, generator=g).to(dev))
        else:
            self.h = PolicyHandle(prev_action_dims=32, prev_action_null=1, **CORE)
            sd = syn.policy_state_dict(0, **self.h.cfg, **CORE)
            self.feat = (torch.randn(rows, 49, 2048, generator=g).abs() * 0.5).to(torch.bfloat16).to(dev)
            self.kw = {}
        self.flat = self.h.flatten(sd, dev)
        self.goal = torch.randint(0, 12, (rows,), generator=g).to(dev)
        self.prev = torch.randint(0, 6, (rows,), generator=g).to(dev)
        self.m = (torch.rand(rows, generator=g) > 0.01).float().to(dev)
        self.state = [torch.zeros(N, self.h.state_width, device=dev) for _ in range(2)]
        self.hv = torch.empty(rows, 7, device=dev)
        self.out = [torch.empty(N, dtype=dt, device=dev) for dt in (torch.int64, torch.float32, torch.float32)]

    def act(self, ws, step: int, reuse: bool):
        a, b = self.state[step & 1], self.state[1 - (step & 1)]
        fn = self.h.act if self.kind.startswith("pooled") else self.h.act_ex
        fn(self.flat, self.feat, self.goal, a, self.m, self.N, ws, self.hv, b, *self.out, 1, step, 0, reuse_tables=reuse,
           prev_actions=self.prev, **self.kw)


def act_step_us(ag: Agent, reps: int) -> float:
    ws = torch.empty(ag.h.workspace_bytes(1, ag.N, False), dtype=torch.uint8, device=ag.flat.device)
    for s in range(4):
        ag.act(ws, s, s > 0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for s in range(reps):
        ag.act(ws, s, True)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def act_launches(ag: Agent):
    ws = torch.empty(ag.h.workspace_bytes(1, ag.N, False), dtype=torch.uint8, device=ag.flat.device)
    ag.act(ws, 0, False)
    ev = kernel_events(lambda: ag.act(ws, 1, True))
    return None if ev is None else [kernel_name(n) for n, _ in ev]


def act_child(a) -> None:
    dev = torch.device("cuda:0")
    for n in a.act_actors:
        for kind in AGENTS:
            ag = Agent(kind, 1, n, dev)
            line = {"measure": "act_step", "round": a.act_child, "pooled_act": os.environ.get("EC_POOLED_ACT", "1"), "agent": kind,
                    "actors": n, "act_step_us": round(act_step_us(ag, a.act_reps), 2)}
            if a.act_child == 0:
                names = act_launches(ag)
                if names is not None:
                    line.update(launches=len(names), kernels=names)
            print(json.dumps(line), flush=True)
            del ag
            torch.cuda.empty_cache()


def learn_pass(a, rnd: int) -> None:
    dev = torch.device("cuda:0")
    T, N = a.rollout, a.slice_actors
    for kind in AGENTS:
        ag = Agent(kind, T, N, dev)
        ws = torch.empty(ag.h.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
        dhv = torch.randn(T * N, 7, device=dev) / (T * N)
        grads = torch.zeros_like(ag.flat)

        def one():
            ag.h.forward(ag.flat, ag.feat, ag.goal, ag.state[0], ag.m, T, N, ws, hv=ag.hv, h_final=ag.state[1], prev_actions=ag.prev, **ag.kw)
            ag.h.backward(ag.flat, ag.feat, ag.m, T, N, ws, dhv, None, grads)
        for _ in range(a.warmup):
            one()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            one()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps({"measure": "learn_pass", "round": rnd, "agent": kind, "rollout": T, "actors": N, "steps": a.steps,
                          "policy_params": int(sum(k for _, k in ag.h.offsets.values())),
                          "rollout_feature_MB": round(ag.feat.numel() * ag.feat.element_size() / 2 ** 20, 1),
                          "forward_backward_ms": round(e0.elapsed_time(e1) / a.steps, 3)}), flush=True)
        del ag, ws
        torch.cuda.empty_cache()


def iteration(a, rnd: int) -> None:
    import time
    from embodied_clip_amd.engine import Worker
    for kind in AGENTS:
        kw = dict(net="pooled", pooling=kind.split("-")[1], sensors=(2, 2)) if kind.startswith("pooled") else {}
        w = Worker(a.actors, T=a.rollout, device="cuda:0", seed=0, update_repeats=a.update_repeats, prev_actions=32, **CORE, **kw)
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
        print(json.dumps({"measure": "iteration", "round": rnd, "agent": kind, "actors": a.actors, "rollout": a.rollout,
                          "update_repeats": a.update_repeats, "steps": a.steps, "slices": w.ns,
                          "rollout_feature_MB": round(sum(sl.feat.numel() * sl.feat.element_size() for sl in w.slices) / 2 ** 20, 1),
                          "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                          "env_frames_per_s": round(a.steps * a.rollout * a.actors / dt, 1),
                          "update_ms": round(sum(upd) / len(upd), 3)}), flush=True)
        del w
        torch.cuda.empty_cache()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--act-actors", nargs="+", type=int, default=[32, 128])
    ap.add_argument("--slice-actors", type=int, default=128, help="actors of one slice's learn pass (a 256-actor worker has two)")
    ap.add_argument("--actors", type=int, default=256, help="actors of the whole-worker measurement")
    ap.add_argument("--update-repeats", type=int, default=4)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--act-reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2, help="repeat the whole list (alternating the agents)")
    ap.add_argument("--act-child", type=int, default=None, help="(child mode) only the act-step measurements; the value is the round")
    ap.add_argument("--skip", nargs="*", default=[], choices=("act", "learn", "iteration"))
    a = ap.parse_args()
    if a.act_child is not None:
        act_child(a)
        return
    if "act" not in a.skip:         # fresh child processes, before this one opens the GPU
        for rnd in range(a.rounds):
            for setting in ("1", "0"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--act-child", str(rnd), "--act-reps", str(a.act_reps),
                                    "--act-actors", *map(str, a.act_actors)], env={**os.environ, "EC_POOLED_ACT": setting}, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"act-step measurement with EC_POOLED_ACT={setting} failed with status {r.returncode}")
    if "learn" not in a.skip:
        for rnd in range(a.rounds):
            learn_pass(a, rnd)
    if "iteration" not in a.skip:
        for rnd in range(a.rounds):
            iteration(a, rnd)


if __name__ == "__main__":
    main()
