"""The sequential reference of the episode bookkeeping (tests/_episode_ref.py) on the hand-made case: an episode that ends on
a call's last step, a length-1 episode right after an end, two ends on consecutive steps, an episode that spans the call
boundary, and an actor that never finishes."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _episode_ref as er  # noqa: E402


def test_hand_made_case():
    ref = er.EpisodeRef(er.HAND_N)
    for c, (rewards, masks, success) in enumerate(er.hand_case()):
        out = ref.update(rewards, masks, success)
        assert [(r[1], r[0]) for r in out] == sorted(er.HAND_ENDS[c], key=lambda e: (e[1], e[0]))   # actor, then t
        assert [r[2] for r in out] == er.HAND_LENGTHS[c]
    assert len(ref.records) == 7
    assert ref.carry_len.tolist() == er.HAND_CARRY_LEN
    n, s, s2, ln, sc = ref.totals()
    assert (n, ln, sc) == (7, 2 + 1 + 1 + 4 + 6 + 1 + 7, 3.0)
    # the returns are the step-ordered fp32 sums, carried over the call boundary (actor 1: steps 2, 3 of call 1, then all of call 2)
    (r1, _, _), (r2, _, _) = er.hand_case()
    want = np.float32(0)
    for x in list(r1[2:, 1]) + list(r2[:, 1]):
        want = np.float32(want + x)
    assert ref.calls[1][0][:3] == (1, 3, 6) and ref.calls[1][0][3] == float(want)
    # the running episodes are in the carries and nowhere else
    run4 = np.float32(0)
    for x in list(r1[:, 4]) + list(r2[:, 4]):
        run4 = np.float32(run4 + x)
    assert ref.carry_ret[4] == run4 and ref.carry_ret[1] == 0
    info = ref.info()
    assert info["episodes"] == 7 and info["ep_length"] == 22 / 7 and info["success"] == 3 / 7
    assert math.isclose(info["reward"], s / 7) and info["reward_std"] > 0


def test_no_episode_gives_nan():
    ref = er.EpisodeRef(3)
    ref.update(np.ones((2, 3), np.float32), np.ones((3, 3), np.float32))
    assert ref.info()["episodes"] == 0 and math.isnan(ref.info()["reward"])
    assert ref.carry_len.tolist() == [2, 2, 2]
