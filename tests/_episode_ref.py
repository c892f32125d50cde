"""Sequential reference of ``ec_episode_stats`` (csrc/episode.hip) and the hand-made case the episode tests share.

The carries are fp32 sums formed one step at a time in a Python loop (``numpy.float32`` additions: the order and the rounding the
kernel's per-actor loop has), the totals are ``math.fsum`` over the completed episodes -- the correctly rounded sums the kernel's
double accumulation is compared against."""
import math

import numpy as np


class EpisodeRef:
    def __init__(self, N):
        self.N = N
        self.carry_ret = np.zeros(N, dtype=np.float32)
        self.carry_len = np.zeros(N, dtype=np.int32)
        self.records = []            # (actor, t, length, return, success) in the kernel's order, over all calls
        self.calls = []              # the records of each call

    def update(self, rewards, masks, success=None):
        """rewards [T, N], masks [T+1, N], success [T, N] or None: numpy float32."""
        T, N = rewards.shape
        assert N == self.N and masks.shape == (T + 1, N)
        out = []
        for n in range(N):                       # actor ascending, then t ascending
            ret, ln = np.float32(self.carry_ret[n]), int(self.carry_len[n])
            for t in range(T):
                ret = np.float32(ret + np.float32(rewards[t, n]))
                ln += 1
                if masks[t + 1, n] == 0:
                    out.append((n, t, ln, float(ret), float(success[t, n]) if success is not None else 0.0))
                    ret, ln = np.float32(0), 0
            self.carry_ret[n], self.carry_len[n] = ret, ln
        self.calls.append(out)
        self.records += out
        return out

    def totals(self):
        """(episodes, sum return, sum return^2, sum length, sum success), each correctly rounded."""
        r = self.records
        return (len(r), math.fsum(x[3] for x in r), math.fsum(x[3] * x[3] for x in r), sum(x[2] for x in r),
                math.fsum(x[4] for x in r))

    def abs_sums(self):
        """(sum |return|, sum return^2): the scales of the n-term summation bound."""
        return math.fsum(abs(x[3]) for x in self.records), math.fsum(x[3] * x[3] for x in self.records)

    def info(self):
        n, s, s2, ln, sc = self.totals()
        if n == 0:
            nan = float("nan")
            return {"episodes": 0, "reward": nan, "reward_std": nan, "ep_length": nan, "success": nan}
        mean = s / n
        return {"episodes": n, "reward": mean, "reward_std": math.sqrt(max(s2 / n - mean * mean, 0.0)), "ep_length": ln / n,
                "success": sc / n}


# ---- the hand-made case: T = 4, N = 5, two calls ---------------------------------------------------------------------------
HAND_T, HAND_N = 4, 5
HAND_ENDS = [[(1, 0), (0, 1), (1, 1), (3, 2)],      # (t, n) with masks[t+1, n] = 0, call 1
             [(3, 1), (0, 2), (2, 3)]]              # call 2
HAND_LENGTHS = [[2, 1, 1, 4], [6, 1, 7]]            # in record order
HAND_CARRY_LEN = [6, 0, 3, 1, 8]
HAND_SUCCESS = [[(1, 0), (1, 1)], [(2, 3)]]         # three of the seven ends succeed


def hand_case():
    """[(rewards [T,N], masks [T+1,N], success [T,N])] for the two calls, float32; rewards are small non-dyadic numbers plus a
    +10 on the successful ends, so the fp32 sums round."""
    calls = []
    for c in range(2):
        k = np.arange(HAND_T * HAND_N, dtype=np.float64).reshape(HAND_T, HAND_N)
        rewards = (-0.01 - 0.003 * np.sin(1.7 * k + c)).astype(np.float32)
        masks = np.ones((HAND_T + 1, HAND_N), dtype=np.float32)
        success = np.zeros((HAND_T, HAND_N), dtype=np.float32)
        for t, n in HAND_ENDS[c]:
            masks[t + 1, n] = 0
        for t, n in HAND_SUCCESS[c]:
            success[t, n] = 1
            rewards[t, n] += np.float32(10)
        calls.append((rewards, masks, success))
    return calls
