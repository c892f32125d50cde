"""Evaluation throughput beside the training rollout, on one GPU.

Prints env-frames/s of ``Evaluator.run`` (sampled and greedy actions) and of ``Worker.collect_rollout`` -- the same launches per
env step -- at 256 actors, ``--repeats`` timings each (their spread is the run-to-run noise the comparison has to clear), and
the time of ``ec_episode_stats`` beside ``ec_gae`` at T = 128, N = 256.  On a checkout without ``embodied_clip_amd.evaluate``
(the parent commit) it prints the rollout rate and the ``ec_gae`` time only.  Where the tree has the navigation metrics it also
times ``ec_nav_episode_stats`` (12 categories) at the same shape, with and without records, and ``Evaluator.run`` with
``nav_metrics`` on beside the runs with it off."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from embodied_clip_amd import _lib  # noqa: E402
from embodied_clip_amd.engine import Worker  # noqa: E402

try:
    from embodied_clip_amd.evaluate import Evaluator
except ImportError:
    Evaluator = None

ap = argparse.ArgumentParser()
ap.add_argument("--actors", type=int, default=256)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
N, T = a.actors, a.steps


def rates(fn):
    fn()                                   # warm-up: tables, allocator, clocks
    torch.cuda.synchronize()
    out = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(N * T / (time.perf_counter() - t0))
    return out


def show(name, r):
    print(f"{name:34s} {N} actors x {T} steps: " + "  ".join(f"{x / 1e3:7.2f}" for x in r) + "  k env-frames/s"
          f"   (median {sorted(r)[len(r) // 2] / 1e3:.2f}, spread {(max(r) - min(r)) / max(r) * 100:.1f} %)")


def kernel_us(fn, iters=200):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


w = Worker(N, T=T, device="cuda:0")
show("Worker.collect_rollout", rates(w.collect_rollout))
w.compute_returns()
print(f"ec_gae (+ advantage normalisation)   T={T} N={N}: {kernel_us(w.compute_returns):6.1f} us per call")
env = w.env
del w
torch.cuda.empty_cache()
if Evaluator is None:
    sys.exit(0)
from embodied_clip_amd.episodes import EpisodeTracker  # noqa: E402

tr = EpisodeTracker(N, "cuda:0")
print(f"ec_episode_stats                     T={T} N={N}: {kernel_us(lambda: tr.update(env.rewards, env.masks, env.success)):6.1f} us per call")
tr = EpisodeTracker(N, "cuda:0", capacity=4096)
print(f"ec_episode_stats, records kept       T={T} N={N}: {kernel_us(lambda: (tr.reset(), tr.update(env.rewards, env.masks, env.success))):6.1f} us per call (with the reset)")
try:
    from embodied_clip_amd.engine import NavSyntheticEnv
    from embodied_clip_amd.episodes import NavEpisodeTracker
except ImportError:
    NavSyntheticEnv = None
if NavSyntheticEnv is not None:
    nav = NavSyntheticEnv(N, T, "cuda:0", seed=1000)
    nav_args = (nav.rewards, nav.masks, nav.success, nav.step_dist, nav.start_dist, nav.goal_dist, nav.goals)
    assert torch.equal(nav.rewards, env.rewards) and torch.equal(nav.masks, env.masks)      # the same episodes as the legs above
    ntr = NavEpisodeTracker(N, "cuda:0", num_categories=12)
    print(f"ec_nav_episode_stats, C=12           T={T} N={N}: {kernel_us(lambda: ntr.update(*nav_args)):6.1f} us per call")
    ntr = NavEpisodeTracker(N, "cuda:0", num_categories=12, capacity=4096)
    print(f"ec_nav_episode_stats, records kept   T={T} N={N}: {kernel_us(lambda: (ntr.reset(), ntr.update(*nav_args))):6.1f} us per call (with the reset)")
    ntr = NavEpisodeTracker(N, "cuda:0", num_categories=0)
    print(f"ec_nav_episode_stats, C=0            T={T} N={N}: {kernel_us(lambda: ntr.update(*nav_args[:6])):6.1f} us per call")
    del nav, nav_args, ntr
del env
for det in (False, True):
    ev = Evaluator(N, T=T, device="cuda:0", deterministic=det)
    show(f"Evaluator.run, {'greedy' if det else 'sampled'} actions", rates(lambda: ev.run(1)))
    print("    ", ev.info())
    del ev
    torch.cuda.empty_cache()
if NavSyntheticEnv is not None:
    ev = Evaluator(N, T=T, device="cuda:0", nav_metrics=True)
    show("Evaluator.run, sampled, nav_metrics", rates(lambda: ev.run(1)))
    print("    ", ev.info())
    del ev
    torch.cuda.empty_cache()
print("library:", _lib.LIB_PATH)
