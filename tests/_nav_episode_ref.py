"""Sequential reference of ``ec_nav_episode_stats`` (csrc/episode.hip) and the hand-made case the navigation-metric tests share.

As in ``_episode_ref``: the carries (return, path) are fp32 sums formed one step at a time with ``numpy.float32`` additions,
every per-episode value (spl, soft_spl) is computed in ``numpy.float32`` in the operation order include/ec_amd.h states, and
the totals are ``math.fsum`` over the completed episodes -- the correctly rounded sums the kernel's doubles are compared to."""
import math

import numpy as np

import _episode_ref as er

F = np.float32
COLS = ("episodes", "return", "return2", "length", "success", "spl", "soft_spl", "goal_dist", "path", "no_path")


def scores(d0, d1, p, s):
    """(spl, soft_spl) of one episode in fp32; ``d1`` None: no distance to the goal (soft_spl 0)."""
    d0, p, s = F(d0), F(p), F(s)
    if d0 < 0:
        return F(0), F(0)
    if d0 == 0:
        one = F(1) if (s > 0 and p == 0) else F(0)
        return one, (one if d1 is not None else F(0))
    ratio = F(d0 / max(d0, p))
    spl = ratio if s > 0 else F(0)
    if d1 is None:
        return spl, F(0)
    soft = F(max(F(0), F(F(1) - F(F(d1) / d0))) * ratio)
    return spl, soft


class NavEpisodeRef:
    """Records are dicts with the keys of ``NavEpisodeTracker.records()`` (floats kept as ``numpy.float32``)."""

    def __init__(self, N, C=0):
        self.N, self.C = N, C
        self.carry_ret = np.zeros(N, dtype=np.float32)
        self.carry_len = np.zeros(N, dtype=np.int32)
        self.carry_path = np.zeros(N, dtype=np.float32)
        self.records = []
        self.calls = []
        self.goal_dist = None

    def update(self, rewards, masks, success, step_dist, start_dist, goal_dist=None, category=None):
        """numpy float32 [T, N] (masks [T+1, N]); category int64 [>= T, N] or None."""
        T, N = rewards.shape
        assert N == self.N and masks.shape == (T + 1, N) and (category is not None) == (self.C > 0)
        self.goal_dist = goal_dist is not None
        out = []
        for n in range(N):                       # actor ascending, then t ascending
            ret, path, ln = F(self.carry_ret[n]), F(self.carry_path[n]), int(self.carry_len[n])
            for t in range(T):
                ret = F(ret + F(rewards[t, n]))
                path = F(path + F(step_dist[t, n]))
                ln += 1
                if masks[t + 1, n] == 0:
                    s = F(success[t, n]) if success is not None else F(0)
                    d0 = F(start_dist[t, n])
                    d1 = F(goal_dist[t, n]) if goal_dist is not None else None
                    spl, soft = scores(d0, d1, path, s)
                    out.append({"actor": n, "t": t, "length": ln, "category": int(category[t, n]) if category is not None else -1,
                                "return": ret, "success": s, "spl": spl, "soft_spl": soft, "path": path,
                                "goal_dist": d1 if d1 is not None else F(0), "start_dist": d0})
                    ret, path, ln = F(0), F(0), 0
            self.carry_ret[n], self.carry_path[n], self.carry_len[n] = ret, path, ln
        self.calls.append(out)
        self.records += out
        return out

    def rows(self):
        """The records of each totals row: row 0 all of them, row 1 + c those of category c (ids outside [0, C): row 0 only)."""
        return [self.records] + [[r for r in self.records if r["category"] == c] for c in range(self.C)]

    @staticmethod
    def _terms(recs):
        return [[1.0] * len(recs), [float(r["return"]) for r in recs], [float(r["return"]) ** 2 for r in recs],
                [float(r["length"]) for r in recs], [float(r["success"]) for r in recs], [float(r["spl"]) for r in recs],
                [float(r["soft_spl"]) for r in recs], [float(r["goal_dist"]) for r in recs], [float(r["path"]) for r in recs],
                [1.0 if r["start_dist"] < 0 else 0.0 for r in recs]]

    def totals(self):
        """[(1 + C)][10], each sum correctly rounded."""
        return [[math.fsum(col) for col in self._terms(recs)] for recs in self.rows()]

    def abs_sums(self):
        """[(1 + C)][10] sums of |x|: the scales of the n-term summation bound."""
        return [[math.fsum(abs(x) for x in col) for col in self._terms(recs)] for recs in self.rows()]

    @staticmethod
    def info_of(row, goal_dist=True):
        nan = float("nan")
        n = row[0]
        if n == 0:
            return {"episodes": 0, "reward": nan, "reward_std": nan, "ep_length": nan, "success": nan, "spl": nan,
                    "soft_spl": nan, "dist_to_goal": nan, "path_length": nan, "no_path": 0}
        mean = row[1] / n
        return {"episodes": int(n), "reward": mean, "reward_std": math.sqrt(max(row[2] / n - mean * mean, 0.0)),
                "ep_length": row[3] / n, "success": row[4] / n, "spl": row[5] / n,
                "soft_spl": row[6] / n if goal_dist else nan, "dist_to_goal": row[7] / n if goal_dist else nan,
                "path_length": row[8] / n, "no_path": int(row[9])}

    def info(self):
        return self.info_of(self.totals()[0], self.goal_dist is not False)


# ---- the hand-made case: _episode_ref.hand_case() (T = 4, N = 5, two calls, 7 ends) with geometry ------------------------------
# Ends in record order (call, t, n):  (1,1,0) (1,0,1) (1,1,1) (1,3,2) | (2,3,1) (2,0,2) (2,2,3); successes: the first, the third
# and the last.  step_dist is 0.25 on the steps listed in HAND_MOVES and 0 elsewhere, so every path is a small dyadic number.
HAND_C = 3
HAND_MOVES = [[(0, 0), (0, 2), (1, 2), (2, 2), (3, 3), (2, 0), (3, 4)],            # (t, n) of call 1
              [(0, 1), (1, 1), (3, 1), (0, 2), (0, 3), (1, 3), (1, 0)]]            # call 2
#                      d0     d1    category        the episode
HAND_END_GEOM = [[((1, 0), 1.0, 0.5, 0),          # success, path 0.25 < d0: the clamp gives spl 1; soft = 0.5
                  ((0, 1), 0.0, 0.25, 1),         # d0 == 0, path 0, no success: 0 / 0
                  ((1, 1), 0.0, 0.0, 2),          # d0 == 0, path 0, success: 1 / 1
                  ((3, 2), 2.0, 3.0, 0)],         # failure, path 0.75, d1 > d0: spl 0, soft 0
                 [((3, 1), -1.0, 4.0, 1),         # no path (length 6, path 0.75 over both calls)
                  ((0, 2), 0.0, 1.0, 2),          # d0 == 0 with path 0.25 > 0 (a length-1 episode that moved): 0 / 0
                  ((2, 3), 0.5, 0.125, 1)]]       # success, path 0.25 (call 1) + 0.5 (call 2) = 0.75 > d0: spl 0.5 / 0.75; crosses the call
# expected, in record order
HAND_PATH = [0.25, 0.0, 0.0, 0.75, 0.75, 0.25, 0.75]
HAND_SPL = [1.0, 0.0, 1.0, 0.0, 0.0, 0.0, float(F(0.5) / F(0.75))]
HAND_SOFT_SPL = [0.5, 0.0, 1.0, 0.0, 0.0, 0.0, float(F(F(1) - F(F(0.125) / F(0.5))) * F(F(0.5) / F(0.75)))]
HAND_CATEGORY = [0, 1, 2, 0, 1, 2, 1]
HAND_CARRY_PATH = [0.5, 0.0, 0.0, 0.0, 0.25]


def hand_case():
    """[(rewards, masks, success, step_dist, start_dist, goal_dist, category [T+1, N] int64)] for the two calls.  Off the ending
    steps start_dist / goal_dist / category hold values that would spoil every score if they were read (-7, 99, 77)."""
    calls = []
    for c, (rewards, masks, success) in enumerate(er.hand_case()):
        step_dist = np.zeros((er.HAND_T, er.HAND_N), dtype=np.float32)
        for t, n in HAND_MOVES[c]:
            step_dist[t, n] = 0.25
        start_dist = np.full((er.HAND_T, er.HAND_N), -7.0, dtype=np.float32)
        goal_dist = np.full((er.HAND_T, er.HAND_N), 99.0, dtype=np.float32)
        category = np.full((er.HAND_T + 1, er.HAND_N), 77, dtype=np.int64)
        for (t, n), d0, d1, cat in HAND_END_GEOM[c]:
            start_dist[t, n], goal_dist[t, n], category[t, n] = d0, d1, cat
        calls.append((rewards, masks, success, step_dist, start_dist, goal_dist, category))
    return calls
