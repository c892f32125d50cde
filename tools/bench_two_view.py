"""Timings of the two-view rearrangement net's front (csrc/two_view.hip) and of its handle's act step on one MI355X:

    python tools/bench_two_view.py --rounds 2 > profiles/two_view_bench.txt

  * ec_two_view_fwd / ec_two_view_bwd alone at C = 2048, S2 = 49, H = 512, A1 = 32 and B = 32 / 128 frames (an act step's) and at
    the frames of a learn pass (--learn-frames, default 256 actors x rollout 128 = 32768);
  * the yardstick of the forward kernel: torch.matmul (the vendor bf16 GEMM) on a MATERIALISED [B * 49, 6144] x [6144, 544]
    operand -- ONE bf16 product over K = 3C where the kernel walks eleven C-wide plane products (three weight planes against u and
    against w, five against the two planes of u * w: 3.67 x the MFMA work), and with the 3C-wide operand already in memory,
    which the kernel never writes.  A yardstick, not a pass mark;
  * the act step of PolicyHandle.two_view(2048, 512, 84, prev_action_dims=512, rnn_type="LSTM") at 32 / 128 actors with reused
    tables;
  * whole workers at --actors x --rollout (256 x 128), timed as bench.py times the flagship (one warm-up, three timed iterations):
    Worker(net="two_view", num_actions=84, loss="imitation", rnn_type="LSTM") beside the two-tower Worker(depth=True), which
    carries the same feature bytes.

Every figure is the median over --rounds x --iters timed calls between two stream events, after a warm-up; inputs are seeded.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from embodied_clip_amd import _lib, synthetic as syn  # noqa: E402
from embodied_clip_amd.policy import PolicyHandle  # noqa: E402

C, S2, H, A1 = 2048, 49, 512, 32


def timed(fn, rounds, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds * iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def front(B, dev, rounds, iters, params):
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(B)
    u = torch.relu(torch.randn(B, S2, C, generator=g, device=dev)).to(torch.bfloat16)
    w = torch.relu(torch.randn(B, S2, C, generator=g, device=dev)).to(torch.bfloat16)
    dv = torch.randn(B, H, generator=g, device=dev)
    v = torch.empty(B, H, device=dev)
    n1, n0 = lib.ec_two_view_workspace_bytes(B, S2, C, H, A1, 1), lib.ec_two_view_workspace_bytes(B, S2, C, H, A1, 0)
    ws = torch.empty(n1, dtype=torch.uint8, device=dev)
    We, be, Wa, ba, w2, b2 = params
    grads = [torch.zeros_like(t) for t in params]
    s = _lib.stream_ptr()

    def fwd(save):
        _lib.check(lib.ec_two_view_fwd(u.data_ptr(), w.data_ptr(), We.data_ptr(), be.data_ptr(), Wa.data_ptr(), ba.data_ptr(), w2.data_ptr(),
                                       b2.data_ptr(), v.data_ptr(), B, S2, C, H, A1, ws.data_ptr(), n1 if save else n0, save, s))

    def bwd():
        _lib.check(lib.ec_two_view_bwd(u.data_ptr(), w.data_ptr(), w2.data_ptr(), dv.data_ptr(), grads[0].data_ptr(), grads[1].data_ptr(),
                                       grads[2].data_ptr(), grads[3].data_ptr(), grads[4].data_ptr(), grads[5].data_ptr(), B, S2, C, H, A1,
                                       ws.data_ptr(), n1, s))
    t_inf = timed(lambda: fwd(0), rounds, iters)
    t_save = timed(lambda: fwd(1), rounds, iters)
    t_bwd = timed(bwd, rounds, iters)
    return t_inf, t_save, t_bwd, n1


def yardstick(B, dev, rounds, iters):
    g = torch.Generator(device=dev).manual_seed(B + 1)
    a = torch.randn(B * S2, 3 * C, generator=g, device=dev).to(torch.bfloat16)
    b = torch.randn(3 * C, H + A1, generator=g, device=dev).to(torch.bfloat16)
    out = torch.empty(B * S2, H + A1, dtype=torch.bfloat16, device=dev)
    return timed(lambda: torch.matmul(a, b, out=out), rounds, iters)


def act_step(N, dev, rounds, iters):
    h = PolicyHandle.two_view(C, H, 84, prev_action_dims=H, rnn_type="LSTM")
    flat = h.flatten(syn.policy_state_dict(0, two_view=h.two_view_cfg), dev)
    g = torch.Generator(device=dev).manual_seed(N)
    u = torch.relu(torch.randn(N, S2, C, generator=g, device=dev)).to(torch.bfloat16)
    w = torch.relu(torch.randn(N, S2, C, generator=g, device=dev)).to(torch.bfloat16)
    prev = torch.randint(0, 84, (N,), generator=g, device=dev)
    h0, hf = torch.zeros(N, h.state_width, device=dev), torch.empty(N, h.state_width, device=dev)
    m = torch.ones(N, device=dev)
    ws = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    hv = torch.empty(N, 85, device=dev)
    a, lp, vv = torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    h.act(flat, u, None, h0, m, N, ws, hv, hf, a, lp, vv, seed=1, step=0, feat2=w, prev_actions=prev)       # builds the tables
    return timed(lambda: h.act(flat, u, None, h0, m, N, ws, hv, hf, a, lp, vv, seed=1, step=1, feat2=w, prev_actions=prev, reuse_tables=True),
                 rounds, iters)


def worker_line(kind, kw, actors, rollout, steps, warmup):
    """One whole worker, timed as bench.py times the flagship: env-frames/s over `steps` iterations and HIP events around update()."""
    import time
    from embodied_clip_amd.engine import Worker
    w = Worker(actors, T=rollout, device="cuda:0", seed=0, **kw)
    for _ in range(warmup):
        w.iteration()
    torch.cuda.synchronize()
    w.time_trunk, w.update_events, w.trunk_events = True, [], []
    t0 = time.perf_counter()
    for _ in range(steps):
        w.iteration()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    upd = [e0.elapsed_time(e1) for e0, e1 in w.update_events]
    feat_gb = sum(sl.feat.numel() * sl.feat.element_size() * (2 if sl.feat2 is not None else 1) for sl in w.slices) / 2 ** 30
    print(f"worker {kind:34s} {actors} actors x rollout {rollout}: {steps * rollout * actors / dt:9.0f} env-frames/s  "
          f"update_ms {sum(upd) / len(upd):8.2f}  rollout features {feat_gb:5.1f} GiB  ({w.ns} slices)", flush=True)
    del w
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--learn-frames", type=int, default=256 * 128)
    ap.add_argument("--actors", type=int, default=256)
    ap.add_argument("--rollout", type=int, default=128)
    ap.add_argument("--no-workers", action="store_true")
    ap.add_argument("--yardstick-frames", type=int, default=8192, help="largest B whose [B * 49, 6144] operand is materialised")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"# two-view front, C={C} S2={S2} H={H} A1={A1}; library {_lib.load().ec_version()}; {torch.cuda.get_device_name(0)}; "
          f"median of {args.rounds} x {args.iters} calls")
    sd = syn.policy_state_dict(0, two_view=dict(in_channels=C, hidden=H, num_actions=84))
    names = ("visual_encoder.0.weight", "visual_encoder.0.bias", "visual_attention.0.weight", "visual_attention.0.bias",
             "visual_attention.2.weight", "visual_attention.2.bias")
    params = [sd[n].reshape(-1).float().contiguous().to(dev) for n in names]
    mmac = S2 * 3 * C * (H + A1) / 1e6
    print(f"# {mmac:.0f} MMAC per frame as ONE bf16 product over K = 3C; the kernel walks 11 C-wide plane products (3 + 3 + 5) where that "
          f"product has 3: 3.67 x the MFMA work")
    yard = {}
    for B in sorted({32, 128, args.yardstick_frames, args.learn_frames}):
        t_inf, t_save, t_bwd, nbytes = front(B, dev, args.rounds, args.iters, params)
        line = (f"front B={B:6d}: fwd {t_inf:9.3f} ms  fwd+save {t_save:9.3f} ms  bwd {t_bwd:9.3f} ms  "
                f"({t_inf * 1e3 / B:8.2f} us/frame fwd; {2 * mmac * B / t_inf / 1e3:7.1f} TFLOP/s of the ONE-product count; workspace {nbytes / 2**20:.0f} MiB)")
        if B <= args.yardstick_frames:
            yard[B] = yardstick(B, dev, args.rounds, args.iters)
            line += f"  | torch.matmul bf16 on the materialised operand {yard[B]:9.3f} ms: kernel / yardstick = {t_inf / yard[B]:.2f}x"
        print(line, flush=True)
    for N in (32, 128):
        t = act_step(N, dev, args.rounds, max(args.iters, 20))
        print(f"act step N={N:4d} (84 actions, E=512, LSTM, reused tables): {t * 1e3:8.1f} us; launches: front, step 0, heads = 3", flush=True)
    if not args.no_workers:     # the same feature bytes per env step: two 2048 x 7 x 7 maps per actor
        for rnd in range(args.rounds):
            worker_line("net=two_view imitation LSTM A=84", dict(net="two_view", num_actions=84, loss="imitation", rnn_type="LSTM"),
                        args.actors, args.rollout, 3, 1)
            worker_line("depth=True (two-tower, PPO, GRU)", dict(depth=True), args.actors, args.rollout, 3, 1)


if __name__ == "__main__":
    main()
