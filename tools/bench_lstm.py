"""The agent with an LSTM core (engine.Worker(rnn_type="LSTM"): csrc/lstm.hip's step kernels) beside the GRU agent of the same
build, in one process, the two cells alternating within each round.

  * the act step: one slice's policy act step at 32 and 128 actors (HIP events around `--act-reps` back-to-back act steps with
    reused tables -- the later steps of a rollout), and the number of kernel launches of ONE such act step (torch.profiler);
  * the recurrences alone at T = 128, N = 128, H = 512: a learn-pass forward and backward of the policy handle under
    torch.profiler, the device time of the step kernels summed by name (forward: *_step_fwd*; backward: *_step_bwd*,
    *_gates_bwd* and, on the gate-plus-GEMM route, the per-step GEMM), beside the HIP-event time of the whole pass.  The
    gate-plus-GEMM backward is the same handle in a child process with EC_GRU_FUSED=0 (the configuration is read once per
    process; on an LSTM handle the switch selects the backward route only);
  * the learn side, timed as bench.py times the flagship: warm-up iterations, then `steps` timed iterations between two device
    synchronisations -- env-frames/s and the update phase (HIP events around Worker.update, mean over the timed iterations).

One JSON line per measurement.

    python tools/bench_lstm.py --actors 256 --rollout 128 --steps 3 --warmup 1 --rounds 2
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

CELLS = ("GRU", "LSTM")


def act_step_us(w, reps: int) -> float:
    """us per act step of slice 0 with reused tables"""
    sl = w.slices[0]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with w._on(sl):
        w._act_slice(sl, 0)                       # tables built
        s = torch.cuda.current_stream()
        ev[0].record(s)
        for _ in range(reps):
            w._act_slice(sl, 0)
        ev[1].record(s)
    torch.cuda.synchronize()
    return 1e3 * ev[0].elapsed_time(ev[1]) / reps


def kernel_events(fn):
    """[(kernel name, device us)] of the launches `fn` makes (torch.profiler), or None where the profiler is not usable"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = []
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                out.append((e.name, float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))))
        return out
    except Exception as ex:     # (a measurement that is missing is reported as missing, never guessed)
        print(json.dumps({"measure": "profiler_unavailable", "error": repr(ex)[:200]}), flush=True)
        return None


def kernel_name(n: str) -> str:
    n = re.sub(r"^void\s+", "", n.replace("(anonymous namespace)::", ""))
    return re.split(r"[<(]", n)[0].strip()[:60]


def act_launches(w):
    sl = w.slices[0]

    def one():
        with w._on(sl):
            w._act_slice(sl, 0)
    one()
    ev = kernel_events(one)
    # (a kernel's name without its return type, template arguments and parameter list)
    return None if ev is None else [kernel_name(n) for n, _ in ev]


def recurrence(cell: str, T: int, N: int, H: int, reps: int) -> None:
    """One JSON line: the learn-pass forward and backward of a handle with a small front end (64 channels), HIP-event time of each
    pass and the step kernels' device time by name."""
    from embodied_clip_amd import synthetic as syn
    from embodied_clip_amd.policy import PolicyHandle
    dev = torch.device("cuda:0")
    kw = dict(in_channels=64, hidden=H)
    h = PolicyHandle(rnn_type=cell, **kw)
    flat = h.flatten(syn.policy_state_dict(0, **kw, rnn_type=cell), dev)
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(T * N, 49, 64, generator=g).abs().to(torch.bfloat16).to(dev)
    goal = syn.synthetic_goals(1, (T * N,)).to(dev)
    h0 = torch.zeros(N, h.state_width, device=dev)
    m = syn.synthetic_masks(2, T, N, p_reset=0.02).reshape(-1).to(dev)
    ws = torch.empty(h.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
    dhv = torch.randn(T * N, h.A + 1, generator=g).to(dev) * 1e-3
    grads = torch.zeros_like(flat)
    fwd = lambda: h.forward(flat, rows, goal, h0, m, T, N, ws)
    bwd = lambda: h.backward(flat, rows, m, T, N, ws, dhv, None, grads)
    fwd(); bwd()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    tf = tb = 0.0
    for _ in range(reps):
        ev[0].record(); fwd(); ev[1].record(); bwd(); ev[2].record()
        torch.cuda.synchronize()
        tf += ev[0].elapsed_time(ev[1]); tb += ev[1].elapsed_time(ev[2])
    out = {"measure": "recurrence", "cell": cell, "T": T, "N": N, "H": H, "gru_fused_env": os.environ.get("EC_GRU_FUSED", "default"),
           "forward_pass_ms": round(tf / reps, 3), "backward_pass_ms": round(tb / reps, 3)}
    kf, kb = kernel_events(fwd), kernel_events(bwd)
    if kf is not None and kb is not None:
        step = lambda n: ("step_fwd" in n or "gates_fwd" in n)
        out["forward_recurrence_ms"] = round(sum(t for n, t in kf if step(n)) / 1e3, 3)
        out["forward_step_launches"] = sum(1 for n, _ in kf if step(n))
        stepb = [(n, t) for n, t in kb if "step_bwd" in n or "gates_bwd" in n]
        out["backward_step_kernels_ms"] = round(sum(t for _, t in stepb) / 1e3, 3)
        out["backward_step_launches"] = len(stepb)
        # the gate-plus-GEMM route: its per-step GEMMs are the [N, H] <- [N, G] x [G, H] launches between the gate kernels
        idx = [i for i, (n, _) in enumerate(kb) if "gates_bwd" in n]
        if len(idx) > 1:
            out["backward_step_gemms_ms"] = round(sum(t for i, (n, t) in enumerate(kb) if idx[0] < i < idx[-1] + 2 and "gemm" in n.lower()) / 1e3, 3)
    print(json.dumps(out), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--act-actors", nargs="+", type=int, default=[32, 128])
    ap.add_argument("--actors", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--update-repeats", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--act-reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=1, help="repeat the whole list (alternating the cells)")
    ap.add_argument("--recurrence", default=None, choices=CELLS, help="(child mode) only the recurrence measurement of this cell")
    ap.add_argument("--rec-shape", nargs=3, type=int, default=[128, 128, 512], metavar=("T", "N", "H"))
    ap.add_argument("--rec-reps", type=int, default=3)
    ap.add_argument("--skip", nargs="*", default=[], choices=("act", "recurrence", "iteration"))
    a = ap.parse_args()
    if a.recurrence:
        recurrence(a.recurrence, *a.rec_shape, a.rec_reps)
        return
    from embodied_clip_amd.engine import Worker
    if "recurrence" not in a.skip:      # fresh child processes (EC_GRU_FUSED is read once per process), before this one opens the GPU
        for _round in range(a.rounds):
            for cell, env in (("GRU", {}), ("LSTM", {}), ("GRU", {"EC_GRU_FUSED": "0"}), ("LSTM", {"EC_GRU_FUSED": "0"})):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--recurrence", cell, "--rec-shape", *map(str, a.rec_shape),
                                    "--rec-reps", str(a.rec_reps)], env={**os.environ, **env}, timeout=300)
                if r.returncode != 0:
                    raise SystemExit(f"recurrence measurement of {cell} {env} failed with status {r.returncode}")
    for _round in range(a.rounds):
        if "act" not in a.skip:
            for n in a.act_actors:
                for cell in CELLS:
                    w = Worker(n, T=2, device="cuda:0", seed=0, encoder_streams=1, rnn_type=cell)
                    us = act_step_us(w, a.act_reps)
                    line = {"measure": "act_step", "cell": cell, "actors": w.slices[0].n, "act_step_us": round(us, 2)}
                    if _round == 0:
                        names = act_launches(w)
                        if names is not None:
                            line.update(launches=len(names), kernels=names)
                    print(json.dumps(line), flush=True)
                    del w
                    torch.cuda.empty_cache()
        if "iteration" not in a.skip:
            for cell in CELLS:
                w = Worker(a.actors, T=a.rollout, device="cuda:0", seed=0, update_repeats=a.update_repeats, rnn_type=cell)
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
                print(json.dumps({"measure": "iteration", "cell": cell, "actors": a.actors, "rollout": a.rollout,
                                  "update_repeats": a.update_repeats, "steps": a.steps, "slices": w.ns,
                                  "policy_params": int(sum(k for _, k in w.policy.offsets.values())),
                                  "ms_per_iteration": round(1e3 * dt / a.steps, 2),
                                  "env_frames_per_s": round(a.steps * a.rollout * a.actors / dt, 1),
                                  "update_ms": round(sum(upd) / len(upd), 3)}), flush=True)
                del w
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
