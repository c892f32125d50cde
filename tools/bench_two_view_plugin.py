"""Timings of the two-view model's AllenAct drop-in (policy.ResNetRearrangeActorCriticRNN) on one MI355X:

    python tools/bench_two_view_plugin.py > profiles/two_view_plugin_bench.txt

  * conversion: ec_nchw_f32_pair_to_nhwc_bf16 (both views, one launch) beside two calls of ec_nchw_f32_to_nhwc_bf16 (one per view)
    at B = 128 and B = 4096 frames per view, C = 2048, HW = 49: microseconds and GB/s (fp32 read + bf16 written, both views).
    CONDITION: the pair kernel's median is not above the two-call route's at either size, beyond the spread the two-call route
    itself shows between the rounds of this run (largest minus smallest per-round median); the verdict is printed;
  * act step: the class under no_grad plus distributions.sample() at N = 32 / 128 beside handle.act on ready bf16 rows with reused
    tables -- the difference is the conversion, the host bridge, and the weight-derived tables, which the class's call rebuilds
    (handle.act with reuse_tables=False is timed beside them to size that part);
  * learn pass at T = 32, N = 64: the class's forward, Imitation().loss and backward() beside the handle's forward +
    imitation_loss_raw + backward3 on cached rows (the class caches its rows too: the conversion is paid once per rollout).

The net is the full-size one: C = 2048, 7 x 7, H = 512, 84 actions, LSTM, previous-action embedding 512 wide.  Every figure is a
median of timed calls between two stream events after a warm-up; the two routes of a comparison ALTERNATE round by round, and
their per-round medians are printed; inputs are seeded.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from embodied_clip_amd import _lib, imitation, spaces, synthetic as syn  # noqa: E402
from embodied_clip_amd.policy import Memory, PolicyHandle, ResNetRearrangeActorCriticRNN  # noqa: E402

C, S, H, A, E = 2048, 7, 512, 84, 512
HW = S * S


def span(fn, iters):
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def alternate(routes, rounds, iters, warm=3):
    """routes: {name: fn}.  -> {name: (median over all calls, [per-round medians])}, the routes taking turns within every round"""
    for fn in routes.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    calls = {k: [] for k in routes}
    per_round = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t = span(fn, iters)
            calls[k] += t
            per_round[k].append(statistics.median(t))
    return {k: (statistics.median(calls[k]), per_round[k]) for k in routes}


def fmt_rounds(xs, scale=1e3):
    return "[" + " ".join(f"{x * scale:.1f}" for x in xs) + "]"


def conversion(B, dev, rounds, iters):
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(B)
    a = torch.relu(torch.randn(B, C, HW, generator=g, device=dev)).to(torch.bfloat16).float()
    b = torch.relu(torch.randn(B, C, HW, generator=g, device=dev)).to(torch.bfloat16).float()
    out = torch.empty(2, B, HW, C, dtype=torch.bfloat16, device=dev)
    flag = torch.zeros(4, dtype=torch.int32, device=dev)
    s = _lib.stream_ptr()

    def pair():
        _lib.check(lib.ec_nchw_f32_pair_to_nhwc_bf16(a.data_ptr(), b.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), B, HW, C,
                                                     flag.data_ptr(), s))

    def two_calls():
        _lib.check(lib.ec_nchw_f32_to_nhwc_bf16(a.data_ptr(), out[0].data_ptr(), B, HW, C, flag.data_ptr(), s))
        _lib.check(lib.ec_nchw_f32_to_nhwc_bf16(b.data_ptr(), out[1].data_ptr(), B, HW, C, flag.data_ptr(), s))
    r = alternate({"pair": pair, "two": two_calls}, rounds, iters)
    gb = 2 * B * C * HW * 6 / 1e9
    (tp, rp), (tt, rt) = r["pair"], r["two"]
    spread = max(rt) - min(rt)
    ok = tp <= tt + spread
    print(f"conversion B={B:5d} per view: pair kernel {tp * 1e3:9.1f} us {gb / tp * 1e3:7.0f} GB/s  rounds {fmt_rounds(rp)} | "
          f"two calls {tt * 1e3:9.1f} us {gb / tt * 1e3:7.0f} GB/s  rounds {fmt_rounds(rt)} (spread {spread * 1e3:.1f} us) | "
          f"pair / two = {tp / tt:.3f}: condition {'MET' if ok else 'NOT MET'}", flush=True)
    return ok


def make_model(dev):
    obs = spaces.Dict({"rgb": spaces.Box(-1e9, 1e9, (C, S, S)), "unshuffled_rgb": spaces.Box(-1e9, 1e9, (C, S, S))})
    return ResNetRearrangeActorCriticRNN(spaces.Discrete(A), obs, "rgb", "unshuffled_rgb", hidden_size=H, rnn_type="LSTM",
                                         prev_action_embedding_dim=E, device=dev)


def features(T, N, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    mk = lambda: torch.relu(torch.randn(T, N, C, S, S, generator=g, device=dev)).to(torch.bfloat16).float()
    return mk(), mk()


def rows_of(x):
    T, N = x.shape[:2]
    return x.view(T * N, C, HW).transpose(1, 2).to(torch.bfloat16).contiguous()


def act_step(model, N, dev, rounds, iters):
    h = model.handle
    flat = model.flat_params
    u, w = features(1, N, dev, N)
    ru, rw = rows_of(u), rows_of(w)
    g = torch.Generator(device=dev).manual_seed(N + 1)
    prev = torch.randint(0, A, (1, N), generator=g, device=dev)
    masks = torch.ones(1, N, 1, device=dev)
    mem0 = torch.zeros(model.num_recurrent_layers, N, H, device=dev)
    obs = {"rgb": u, "unshuffled_rgb": w}

    def plugin():
        with torch.no_grad():
            out, _ = model(obs, Memory().check_append("rnn", mem0, 1), prev, masks)
            out.distributions.sample()

    h0, hf = torch.zeros(N, h.state_width, device=dev), torch.empty(N, h.state_width, device=dev)
    m, p = masks.reshape(N), prev.reshape(N)
    ws = torch.empty(h.workspace_bytes(1, N, False), dtype=torch.uint8, device=dev)
    hv = torch.empty(N, A + 1, device=dev)
    a, lp, vv = torch.empty(N, dtype=torch.int64, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    h.act(flat, ru, None, h0, m, N, ws, hv, hf, a, lp, vv, seed=1, step=0, feat2=rw, prev_actions=p)       # builds the tables

    def handle():
        h.act(flat, ru, None, h0, m, N, ws, hv, hf, a, lp, vv, seed=1, step=1, feat2=rw, prev_actions=p, reuse_tables=True)
    def handle_rebuild():      # what the class's call does behind the conversion: the weight-derived tables are built again
        h.act(flat, ru, None, h0, m, N, ws, hv, hf, a, lp, vv, seed=1, step=1, feat2=rw, prev_actions=p, reuse_tables=False)
    r = alternate({"plugin": plugin, "handle": handle, "rebuild": handle_rebuild}, rounds, iters)
    (tp, rp), (th, rh), (tr, rr) = r["plugin"], r["handle"], r["rebuild"]
    print(f"act step N={N:4d}: class under no_grad + sample() {tp * 1e3:8.1f} us  rounds {fmt_rounds(rp)} | handle.act on ready rows, reused "
          f"tables {th * 1e3:8.1f} us  rounds {fmt_rounds(rh)} | difference {1e3 * (tp - th):8.1f} us, of which the tables rebuilt per call "
          f"{1e3 * (tr - th):8.1f} us (handle.act, reuse_tables=False: {tr * 1e3:8.1f} us  rounds {fmt_rounds(rr)})", flush=True)


def learn_pass(model, T, N, dev, rounds, iters):
    h = model.handle
    flat = model.flat_params
    u, w = features(T, N, dev, 7)
    ru, rw = rows_of(u), rows_of(w)
    g = torch.Generator(device=dev).manual_seed(8)
    prev = torch.randint(0, A, (T, N), generator=g, device=dev)
    expert = torch.randint(0, A, (T, N), generator=g, device=dev)
    emask = (torch.rand(T, N, generator=g, device=dev) < 0.7).float()
    masks = torch.ones(T, N, 1, device=dev)
    mem0 = torch.zeros(model.num_recurrent_layers, N, H, device=dev)
    obs = {"rgb": u, "unshuffled_rgb": w}
    batch = dict(observations=dict(expert_action=torch.stack([expert.float(), emask], -1)))
    loss = imitation.Imitation()

    def plugin():
        out, _ = model(obs, Memory().check_append("rnn", mem0, 1), prev, masks)
        total, _ = loss.loss(0, batch, out)
        total.backward()

    h0 = torch.zeros(N, h.state_width, device=dev)
    m, p, ex, em = masks.reshape(-1), prev.reshape(-1), expert.reshape(-1), emask.reshape(-1).contiguous()
    ws = torch.empty(h.workspace_bytes(T, N, True), dtype=torch.uint8, device=dev)
    grads = torch.zeros_like(flat)

    def handle():
        hv, _ = h.forward(flat, ru, None, h0, m, T, N, ws, feat2=rw, prev_actions=p)
        dhv, _ = imitation.imitation_loss_raw(hv, ex, em, A)
        h.backward(flat, ru, m, T, N, ws, dhv, None, grads.zero_(), feat2=rw)
    r = alternate({"plugin": plugin, "handle": handle}, rounds, iters)
    (tp, rp), (th, rh) = r["plugin"], r["handle"]
    print(f"learn pass T={T} N={N}: class forward + Imitation().loss + backward() {tp:8.3f} ms  rounds {fmt_rounds(rp, 1.0)} | handle forward + "
          f"imitation_loss_raw + backward3 on cached rows {th:8.3f} ms  rounds {fmt_rounds(rh, 1.0)} | difference {tp - th:7.3f} ms", flush=True)
    conv = alternate({"pair": lambda: model._pair_rows(u, w, T * N)}, rounds, iters)["pair"][0]
    print(f"           (the first pass of a rollout also converts both views once: {conv * 1e3:.1f} us, and reads the flag)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"# two-view plugin class, C={C} {S}x{S} H={H} A={A} E={E} LSTM; library {_lib.load().ec_version()}; {torch.cuda.get_device_name(0)}; "
          f"medians of {args.rounds} alternating rounds x {args.iters} calls")
    ok = [conversion(B, dev, args.rounds, args.iters) for B in (128, 4096)]
    print(f"# conversion condition (pair <= two calls + the two-call route's round-to-round spread) at both sizes: {'MET' if all(ok) else 'NOT MET'}")
    torch.cuda.empty_cache()
    model = make_model(dev)
    for N in (32, 128):
        act_step(model, N, dev, args.rounds, max(args.iters, 30))
    learn_pass(model, 32, 64, dev, args.rounds, max(args.iters // 4, 3))


if __name__ == "__main__":
    main()
