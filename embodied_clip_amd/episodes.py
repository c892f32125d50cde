"""Episode metrics of a rollout, kept on the device.

[U] AllenAct's tasks add up their rewards and steps on the host and ``ScalarMeanTracker`` averages the finished episodes
into the ``reward`` / ``ep_length`` / ``success`` scalars of every log line -- the numbers an evaluation run exists to report
(the reference's ``--eval``: readme_files/baselines_robothor_objectnav.md:66-68, baselines_habitat.md:89-97,
zeroshot_objectnav.md:20-27).  Here the rollout's ``rewards`` / ``masks`` already sit in HBM, so one ``ec_episode_stats``
launch per rollout does the bookkeeping there (csrc/episode.hip) and nothing is read back until ``info()`` is asked for.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib


class EpisodeTracker:
    """Carries (running return / length of every actor), totals over the completed episodes and, with ``capacity > 0``, one
    record ``(actor, t, length, return, success)`` per completed episode, in the order actor-ascending then step-ascending
    within each ``update``."""

    def __init__(self, N: int, device, capacity: int = 0):
        self.lib = _lib.load()
        self.N, self.capacity = N, capacity
        self.device = d = torch.device(device)
        self.carry_ret = torch.zeros(N, dtype=torch.float32, device=d)
        self.carry_len = torch.zeros(N, dtype=torch.int32, device=d)
        self.totals = torch.zeros(5, dtype=torch.float64, device=d)    # episodes, sum return, sum return^2, sum length, sum success
        self.n_records = torch.zeros(1, dtype=torch.int32, device=d)
        self.rec_f = torch.zeros((capacity, 2), dtype=torch.float32, device=d) if capacity else None
        self.rec_i = torch.zeros((capacity, 3), dtype=torch.int32, device=d) if capacity else None

    @_lib.on_device
    def update(self, rewards: torch.Tensor, masks: torch.Tensor, success: Optional[torch.Tensor] = None) -> None:
        """One rollout: ``rewards`` f32 [T, N], ``masks`` f32 [T+1, N] (``masks[t+1, n] == 0``: step t ended an episode;
        ``masks[0]`` is not read), ``success`` f32 [T, N] or None (read where an episode ends).  One launch on the current stream."""
        T, N = rewards.shape
        assert N == self.N and tuple(masks.shape) == (T + 1, N), (tuple(rewards.shape), tuple(masks.shape), self.N)
        for x in (rewards, masks, success):
            assert x is None or (x.dtype == torch.float32 and x.is_contiguous() and x.device == self.carry_ret.device)
        assert success is None or tuple(success.shape) == (T, N)
        _lib.check(self.lib.ec_episode_stats(rewards.data_ptr(), masks.data_ptr(), _lib.ptr(success), self.carry_ret.data_ptr(),
                                             self.carry_len.data_ptr(), self.totals.data_ptr(), _lib.ptr(self.rec_f),
                                             _lib.ptr(self.rec_i), self.capacity, self.n_records.data_ptr(), T, N,
                                             _lib.stream_ptr()), "ec_episode_stats")

    def info(self) -> Dict[str, float]:
        """Means over the completed episodes (NaN when there are none); ``reward_std`` is the population deviation."""
        return info_from_totals(self.totals.tolist())

    def records(self) -> Dict[str, torch.Tensor]:
        """The stored records (at most ``capacity``; ``"dropped"`` says how many more completed)."""
        n = int(self.n_records.item())
        k = min(n, self.capacity)
        if not self.capacity:
            e = torch.zeros(0, device=self.device)
            return {"actor": e.int(), "t": e.int(), "length": e.int(), "return": e, "success": e, "dropped": n}
        return {"actor": self.rec_i[:k, 0], "t": self.rec_i[:k, 1], "length": self.rec_i[:k, 2],
                "return": self.rec_f[:k, 0], "success": self.rec_f[:k, 1], "dropped": n - k}

    def reset(self) -> None:
        """Clear totals and records; running episodes stay in the carries."""
        self.totals.zero_()
        self.n_records.zero_()


def info_from_totals(totals5) -> Dict[str, float]:
    n, s, s2, ln, sc = (float(x) for x in totals5)
    if n <= 0:
        nan = float("nan")
        return {"episodes": 0, "reward": nan, "reward_std": nan, "ep_length": nan, "success": nan}
    mean = s / n
    return {"episodes": int(n), "reward": mean, "reward_std": math.sqrt(max(s2 / n - mean * mean, 0.0)), "ep_length": ln / n,
            "success": sc / n}
