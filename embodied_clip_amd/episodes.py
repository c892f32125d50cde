"""Episode metrics of a rollout, kept on the device.

[U] AllenAct's tasks add up their rewards and steps on the host and ``ScalarMeanTracker`` averages the finished episodes
into the ``reward`` / ``ep_length`` / ``success`` scalars of every log line -- the numbers an evaluation run exists to report
(the reference's ``--eval``: readme_files/baselines_robothor_objectnav.md:66-68, baselines_habitat.md:89-97,
zeroshot_objectnav.md:20-27).  Here the rollout's ``rewards`` / ``masks`` already sit in HBM, so one ``ec_episode_stats``
launch per rollout does the bookkeeping there (csrc/episode.hip) and nothing is read back until ``info()`` is asked for.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib
from .dist import allreduce_totals


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


# ---- navigation metrics -------------------------------------------------------------------------------------------------------
# The scores the reference's result tables give beside the success rate: SPL (RoboTHOR ObjectNav, PointNav), SoftSPL and the
# distance to the goal (Habitat), success and SPL per object type averaged over seen and unseen types
# (readme_files/zeroshot_objectnav.md:20-48).  [U] AllenAct's ``spl_metric`` and Habitat's ``SPL`` / ``SoftSPL`` measures are
# restated from their published descriptions (include/ec_amd.h: ec_nav_episode_stats), not pinned.

NAV_COLS = 10       # episodes, sum return, sum return^2, sum length, sum success, sum spl, sum soft_spl, sum goal_dist, sum path, no_path
NAV_MAX_CATEGORIES = 64


class NavEpisodeTracker:
    """``EpisodeTracker`` with the navigation metrics: one ``ec_nav_episode_stats`` launch per ``update`` keeps, beside the
    return / length / success, every episode's path length (the fp32 sum of ``step_dist``, carried across updates), its SPL,
    SoftSPL and final distance to the goal, and totals per goal category (``num_categories`` rows behind the all-episodes row).
    Records, with ``capacity > 0``: ``(actor, t, length, category, return, success, spl, soft_spl, path, goal_dist,
    start_dist)`` in the order of ``EpisodeTracker``."""

    def __init__(self, N: int, device, num_categories: int = 0, capacity: int = 0):
        if not 0 <= num_categories <= NAV_MAX_CATEGORIES:
            raise ValueError(f"NavEpisodeTracker: num_categories is 0..{NAV_MAX_CATEGORIES}, got {num_categories}")
        self.lib = _lib.load()
        self.N, self.C, self.capacity = N, num_categories, capacity
        self.device = d = torch.device(device)
        self.carry_ret = torch.zeros(N, dtype=torch.float32, device=d)
        self.carry_len = torch.zeros(N, dtype=torch.int32, device=d)
        self.carry_path = torch.zeros(N, dtype=torch.float32, device=d)
        self.totals = torch.zeros((1 + num_categories, NAV_COLS), dtype=torch.float64, device=d)
        self.n_records = torch.zeros(1, dtype=torch.int32, device=d)
        self.rec_f = torch.zeros((capacity, 7), dtype=torch.float32, device=d) if capacity else None
        self.rec_i = torch.zeros((capacity, 4), dtype=torch.int32, device=d) if capacity else None
        self.has_goal_dist: Optional[bool] = None      # fixed by the first update: the sums of a mixed run would mean nothing

    @_lib.on_device
    def update(self, rewards: torch.Tensor, masks: torch.Tensor, success: Optional[torch.Tensor], step_dist: torch.Tensor,
               start_dist: torch.Tensor, goal_dist: Optional[torch.Tensor] = None,
               category: Optional[torch.Tensor] = None) -> None:
        """One rollout.  ``rewards`` / ``masks`` / ``success`` as for ``EpisodeTracker.update``; ``step_dist`` f32 [T, N]
        (metres moved by step t), ``start_dist`` f32 [T, N] (the episode's shortest-path length, read where it ends; < 0: no
        path), ``goal_dist`` f32 [T, N] or None (distance to the goal after step t, read where an episode ends), ``category``
        int64 [>= T, N] or None (the goal id, read where an episode ends; required iff ``num_categories > 0``).  One launch."""
        T, N = rewards.shape
        assert N == self.N and tuple(masks.shape) == (T + 1, N), (tuple(rewards.shape), tuple(masks.shape), self.N)
        for x in (rewards, masks, success, step_dist, start_dist, goal_dist):
            assert x is None or (x.dtype == torch.float32 and x.is_contiguous() and x.device == self.carry_ret.device)
        for x in (success, step_dist, start_dist, goal_dist):
            assert x is None or tuple(x.shape) == (T, N)
        if (category is not None) != (self.C > 0):
            raise ValueError("NavEpisodeTracker.update: category goes with num_categories > 0")
        if category is not None:
            assert category.dtype == torch.int64 and category.is_contiguous() and category.device == self.carry_ret.device
            assert category.dim() == 2 and category.shape[0] >= T and category.shape[1] == N, tuple(category.shape)
        if self.has_goal_dist is None:
            self.has_goal_dist = goal_dist is not None
        elif self.has_goal_dist != (goal_dist is not None):
            raise ValueError("NavEpisodeTracker.update: goal_dist is given on every update or on none")
        _lib.check(self.lib.ec_nav_episode_stats(
            rewards.data_ptr(), masks.data_ptr(), _lib.ptr(success), step_dist.data_ptr(), start_dist.data_ptr(),
            _lib.ptr(goal_dist), _lib.ptr(category), self.C, self.carry_ret.data_ptr(), self.carry_len.data_ptr(),
            self.carry_path.data_ptr(), self.totals.data_ptr(), _lib.ptr(self.rec_f), _lib.ptr(self.rec_i), self.capacity,
            self.n_records.data_ptr(), T, N, _lib.stream_ptr()), "ec_nav_episode_stats")

    def _table(self, group=None) -> List[List[float]]:
        return allreduce_totals(self.totals, group=group, device=self.device).tolist()

    def info(self, group=None) -> Dict[str, float]:
        """The five keys of ``EpisodeTracker.info()`` plus ``spl``, ``soft_spl``, ``dist_to_goal``, ``path_length`` (means)
        and ``no_path`` (a count); NaN where nothing was accumulated.  ``group``: summed over the ranks of that process group
        first (``dist.allreduce_totals``; every rank must call)."""
        return info_from_nav_totals(self._table(group)[0], self.has_goal_dist is not False)

    def info_by_category(self, names: Optional[Sequence[str]] = None, group=None) -> Dict[str, Dict[str, float]]:
        """``{name: info}`` per goal category; ``names[c]`` names id ``c`` (default ``"0"``, ``"1"``, ...)."""
        return info_by_category_from_totals(self._table(group), names, self.has_goal_dist is not False)

    def info_groups(self, groups: Dict[str, Sequence[str]], names: Optional[Sequence[str]] = None,
                    group=None) -> Dict[str, Dict[str, float]]:
        """``{group name: info}`` over the episodes of the group's categories: ratios of the summed totals (every episode
        weighs the same), not means of the categories' means."""
        return info_groups_from_totals(self._table(group), groups, names, self.has_goal_dist is not False)

    def records(self) -> Dict[str, torch.Tensor]:
        """The stored records (at most ``capacity``; ``"dropped"`` says how many more completed)."""
        n = int(self.n_records.item())
        k = min(n, self.capacity)
        if not self.capacity:
            e = torch.zeros(0, device=self.device)
            out = {key: e.int() for key in NAV_REC_I}
            out.update({key: e for key in NAV_REC_F})
            out["dropped"] = n
            return out
        out = {key: self.rec_i[:k, i] for i, key in enumerate(NAV_REC_I)}
        out.update({key: self.rec_f[:k, i] for i, key in enumerate(NAV_REC_F)})
        out["dropped"] = n - k
        return out

    def reset(self) -> None:
        """Clear totals and records; running episodes stay in the carries."""
        self.totals.zero_()
        self.n_records.zero_()


NAV_REC_I = ("actor", "t", "length", "category")
NAV_REC_F = ("return", "success", "spl", "soft_spl", "path", "goal_dist", "start_dist")


def info_from_nav_totals(row10, goal_dist: bool = True) -> Dict[str, float]:
    """One row of a navigation totals table -> the info dict.  ``goal_dist=False``: no distance to the goal was ever given, so
    ``soft_spl`` and ``dist_to_goal`` are NaN and not the 0 their sums hold."""
    row = [float(x) for x in row10]
    assert len(row) == NAV_COLS, len(row)
    info = info_from_totals(row[:5])
    n = row[0]
    nan = float("nan")
    if n <= 0:
        info.update(spl=nan, soft_spl=nan, dist_to_goal=nan, path_length=nan, no_path=0)
        return info
    info.update(spl=row[5] / n, soft_spl=row[6] / n if goal_dist else nan, dist_to_goal=row[7] / n if goal_dist else nan,
                path_length=row[8] / n, no_path=int(row[9]))
    return info


def category_names(C: int, names: Optional[Sequence[str]] = None) -> List[str]:
    if names is None:
        return [str(c) for c in range(C)]
    names = list(names)
    if len(names) != C or len(set(names)) != C:
        raise ValueError(f"{C} distinct category names are needed, got {names}")
    return names


def info_by_category_from_totals(totals, names: Optional[Sequence[str]] = None,
                                 goal_dist: bool = True) -> Dict[str, Dict[str, float]]:
    rows = totals.tolist() if hasattr(totals, "tolist") else [list(r) for r in totals]
    names = category_names(len(rows) - 1, names)
    return {name: info_from_nav_totals(rows[1 + c], goal_dist) for c, name in enumerate(names)}


def info_groups_from_totals(totals, groups: Dict[str, Sequence[str]], names: Optional[Sequence[str]] = None,
                            goal_dist: bool = True) -> Dict[str, Dict[str, float]]:
    rows = totals.tolist() if hasattr(totals, "tolist") else [list(r) for r in totals]
    index = {name: c for c, name in enumerate(category_names(len(rows) - 1, names))}
    out = {}
    for gname, members in groups.items():
        unknown = [m for m in members if m not in index]
        if unknown:
            raise ValueError(f"group {gname!r} names unknown categories {unknown}")
        summed = [math.fsum(rows[1 + index[m]][i] for m in members) for i in range(NAV_COLS)]
        out[gname] = info_from_nav_totals(summed, goal_dist)
    return out


def nav_env_tensors(env, with_goal_ids: bool):
    """``(step_dist, start_dist, goal_dist | None, category | None)`` of an env for ``NavEpisodeTracker.update``; an env
    without ``step_dist`` or ``start_dist`` cannot be scored (``ValueError``), one without ``goal_dist`` only lacks SoftSPL."""
    for attr in ("step_dist", "start_dist"):
        if getattr(env, attr, None) is None:
            raise ValueError(f"nav_metrics=True needs the env's `{attr}` (f32 [T, N]); {type(env).__name__} has none")
    return env.step_dist, env.start_dist, getattr(env, "goal_dist", None), env.goals if with_goal_ids else None
