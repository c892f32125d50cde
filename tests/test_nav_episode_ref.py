"""The sequential reference of the navigation metrics (tests/_nav_episode_ref.py) against values worked out by hand."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _episode_ref as er  # noqa: E402
import _nav_episode_ref as nr  # noqa: E402

F = np.float32


def _run():
    ref = nr.NavEpisodeRef(er.HAND_N, nr.HAND_C)
    for c in nr.hand_case():
        ref.update(*c)
    return ref


def test_scores_of_single_episodes():
    # (d0, d1, path, success) -> (spl, soft_spl)
    assert nr.scores(1.0, 0.5, 0.25, 1) == (1.0, 0.5)                      # shorter than the shortest path: clamped to 1
    assert nr.scores(0.5, 0.125, 0.75, 1) == (F(0.5) / F(0.75), F(0.75) * (F(0.5) / F(0.75)))
    assert float(nr.scores(0.5, 0.125, 0.75, 1)[0]) == 0.6666666865348816   # 2/3 rounded to fp32
    assert float(nr.scores(0.5, 0.125, 0.75, 1)[1]) == 0.5                  # 0.75 * fp32(2/3) rounds to 0.5
    assert nr.scores(2.0, 3.0, 0.75, 0) == (0.0, 0.0)                      # failure that ends farther away than it began
    assert nr.scores(2.0, 1.0, 4.0, 0) == (0.0, 0.25)                      # failure that got halfway on twice the path
    assert nr.scores(0.0, 0.0, 0.0, 1) == (1.0, 1.0)
    assert nr.scores(0.0, 0.0, 0.25, 1) == (0.0, 0.0)                      # started on the goal and walked away
    assert nr.scores(0.0, 0.0, 0.0, 0) == (0.0, 0.0)
    assert nr.scores(-1.0, 0.5, 0.75, 1) == (0.0, 0.0)                     # no path
    assert nr.scores(1.0, None, 2.0, 1) == (0.5, 0.0)                      # no distance to the goal: no soft_spl


def test_hand_made_case_records():
    ref = _run()
    rec = ref.records
    assert len(rec) == 7 and [len(c) for c in ref.calls] == [4, 3]
    assert [(r["actor"], r["t"]) for r in rec] == [(0, 1), (1, 0), (1, 1), (2, 3), (1, 3), (2, 0), (3, 2)]
    assert [r["length"] for r in rec] == er.HAND_LENGTHS[0] + er.HAND_LENGTHS[1]
    assert [r["category"] for r in rec] == [0, 1, 2, 0, 1, 2, 1] == nr.HAND_CATEGORY
    assert [float(r["path"]) for r in rec] == [0.25, 0.0, 0.0, 0.75, 0.75, 0.25, 0.75] == nr.HAND_PATH
    assert [float(r["spl"]) for r in rec] == [1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.6666666865348816] == nr.HAND_SPL
    assert [float(r["soft_spl"]) for r in rec] == [0.5, 0.0, 1.0, 0.0, 0.0, 0.0, 0.5] == nr.HAND_SOFT_SPL
    assert [float(r["success"]) for r in rec] == [1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    assert [float(r["start_dist"]) for r in rec] == [1.0, 0.0, 0.0, 2.0, -1.0, 0.0, 0.5]
    assert [float(r["goal_dist"]) for r in rec] == [0.5, 0.25, 0.0, 3.0, 4.0, 1.0, 0.125]
    assert all(isinstance(r[k], np.float32) for r in rec for k in ("return", "spl", "soft_spl", "path"))
    # the returns are those of the plain reference
    plain = er.EpisodeRef(er.HAND_N)
    for c in er.hand_case():
        plain.update(*c)
    assert [float(r["return"]) for r in rec] == [r[3] for r in plain.records]
    assert ref.carry_path.tolist() == [0.5, 0.0, 0.0, 0.0, 0.25] == nr.HAND_CARRY_PATH
    assert ref.carry_len.tolist() == er.HAND_CARRY_LEN
    # the last episode's path crosses the call boundary: 0.25 of it was walked in call 1
    assert float(ref.calls[1][2]["path"]) == 0.75 and ref.calls[1][2]["length"] == 7


def test_hand_made_case_totals_and_info():
    ref = _run()
    tot = ref.totals()
    assert len(tot) == 1 + nr.HAND_C and all(len(r) == 10 for r in tot)
    spl7 = 0.6666666865348816
    assert tot[0][0] == 7 and tot[0][3] == 22 and tot[0][4] == 3 and tot[0][9] == 1
    assert tot[0][5] == math.fsum([1.0, 1.0, spl7]) and tot[0][6] == 2.0 and tot[0][7] == 8.875 and tot[0][8] == 2.75
    assert [r[0] for r in tot[1:]] == [2, 3, 2]                            # episodes per category
    assert [r[9] for r in tot[1:]] == [0, 1, 0]
    assert [r[5] for r in tot[1:]] == [1.0, spl7, 1.0]
    assert [r[8] for r in tot[1:]] == [1.0, 1.5, 0.25]
    for i in range(10):                                                     # every id is in range: the rows add up
        assert abs(sum(r[i] for r in tot[1:]) - tot[0][i]) <= 1e-12 * max(1.0, abs(tot[0][i]))
    info = ref.info()
    assert info["episodes"] == 7 and info["no_path"] == 1 and info["success"] == 3 / 7
    assert info["spl"] == tot[0][5] / 7 and info["soft_spl"] == 2.0 / 7 and info["dist_to_goal"] == 8.875 / 7
    assert info["path_length"] == 2.75 / 7 and info["ep_length"] == 22 / 7
    plain = er.EpisodeRef(er.HAND_N)
    for c in er.hand_case():
        plain.update(*c)
    assert {k: info[k] for k in plain.info()} == plain.info()


def test_absent_inputs():
    calls = nr.hand_case()
    ref = nr.NavEpisodeRef(er.HAND_N, 0)
    for r, m, s, sd, d0, d1, cat in calls:
        ref.update(r, m, None, sd, d0, None, None)
    assert all(float(x["spl"]) == 0 and float(x["soft_spl"]) == 0 and x["category"] == -1 for x in ref.records)
    assert len(ref.totals()) == 1 and ref.totals()[0][8] == 2.75 and ref.totals()[0][9] == 1
    info = ref.info()
    assert info["spl"] == 0 and np.isnan(info["soft_spl"]) and np.isnan(info["dist_to_goal"])
    empty = nr.NavEpisodeRef(3, 2)
    assert empty.info()["episodes"] == 0 and np.isnan(empty.info()["spl"])
    # ids outside [0, C) count in row 0 only
    out = nr.NavEpisodeRef(er.HAND_N, 2)
    for c in calls:
        out.update(*c)
    assert [r[0] for r in out.totals()] == [7, 2, 3]
