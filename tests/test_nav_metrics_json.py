"""The host side of the navigation metrics on hand-built totals and records (CPU tensors): the info dicts, the per-category and
group scores, the metrics file and this project's reader of it."""
import json
import math
import os

import numpy as np
import pytest
import torch

from embodied_clip_amd import episodes as ep
from embodied_clip_amd.evaluate import metrics_from_records, scores_by_object_type, write_metrics_json

FIXTURE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robothor_object_types.json")))
NAMES = FIXTURE["object_types"]


def test_fixture_shape():
    assert len(NAMES) == 12 and NAMES == sorted(NAMES)
    assert len(FIXTURE["seen"]) == 8 and len(FIXTURE["unseen"]) == 4
    assert sorted(FIXTURE["seen"] + FIXTURE["unseen"]) == NAMES


#        episodes  ret   ret^2  length  success  spl   soft  goal_d  path  no_path
ROWS = {"AlarmClock": [4, 8.0, 40.0, 100, 3, 2.5, 2.0, 3.0, 20.0, 0],        # seen
        "Apple":      [1, -1.0, 1.0, 50, 0, 0.0, 0.25, 4.0, 2.0, 1],         # unseen
        "Mug":        [5, 10.0, 30.0, 60, 1, 0.5, 1.0, 10.0, 15.0, 2],       # seen
        "Television": [3, 3.0, 9.0, 30, 3, 3.0, 3.0, 0.75, 6.0, 0]}          # unseen


def _table():
    t = torch.zeros((13, 10), dtype=torch.float64)
    for name, row in ROWS.items():
        t[1 + NAMES.index(name)] = torch.tensor(row, dtype=torch.float64)
    t[0] = t[1:].sum(0)
    t[0, 0] += 2                      # two episodes with ids outside the table: row 0 only
    return t


def test_info_from_totals():
    t = _table()
    info = ep.info_from_nav_totals(t[0])
    assert list(info)[:5] == ["episodes", "reward", "reward_std", "ep_length", "success"]
    assert {k: info[k] for k in list(info)[:5]} == ep.info_from_totals(t[0, :5].tolist())
    assert info["episodes"] == 15 and info["spl"] == 6.0 / 15 and info["soft_spl"] == 6.25 / 15
    assert info["dist_to_goal"] == 17.75 / 15 and info["path_length"] == 43.0 / 15 and info["no_path"] == 3
    nogoal = ep.info_from_nav_totals(t[0], goal_dist=False)
    assert np.isnan(nogoal["soft_spl"]) and np.isnan(nogoal["dist_to_goal"]) and nogoal["spl"] == info["spl"]
    empty = ep.info_from_nav_totals([0.0] * 10)
    assert empty["episodes"] == 0 and empty["no_path"] == 0
    assert all(np.isnan(empty[k]) for k in ("reward", "success", "spl", "soft_spl", "dist_to_goal", "path_length"))


def test_info_by_category_and_groups():
    t = _table()
    by = ep.info_by_category_from_totals(t, NAMES)
    assert list(by) == NAMES
    assert by["AlarmClock"]["success"] == 0.75 and by["AlarmClock"]["spl"] == 0.625 and by["Television"]["spl"] == 1.0
    assert by["Bowl"]["episodes"] == 0 and np.isnan(by["Bowl"]["spl"]) and np.isnan(by["Bowl"]["success"])   # NaN, no division error
    assert list(ep.info_by_category_from_totals(t)) == [str(c) for c in range(12)]
    groups = ep.info_groups_from_totals(t, {"seen": FIXTURE["seen"], "unseen": FIXTURE["unseen"]}, NAMES)
    # ratios of the summed totals ...
    assert groups["seen"]["episodes"] == 9 and groups["seen"]["success"] == 4 / 9 and groups["seen"]["spl"] == 3.0 / 9
    assert groups["unseen"]["episodes"] == 4 and groups["unseen"]["success"] == 3 / 4 and groups["unseen"]["spl"] == 3.0 / 4
    assert groups["seen"]["no_path"] == 2 and groups["unseen"]["dist_to_goal"] == 4.75 / 4
    # ... not the mean of the types' means
    assert groups["seen"]["spl"] != pytest.approx((0.625 + 0.1) / 2)
    assert groups["unseen"]["success"] != pytest.approx((0.0 + 1.0) / 2)
    none = ep.info_groups_from_totals(t, {"empty": ["Bowl", "Vase"]}, NAMES)["empty"]
    assert none["episodes"] == 0 and np.isnan(none["spl"])
    with pytest.raises(ValueError, match="Sofa"):
        ep.info_groups_from_totals(t, {"bad": ["Sofa"]}, NAMES)
    with pytest.raises(ValueError):
        ep.info_by_category_from_totals(t, NAMES[:5])


def _records(dropped=0):
    cat = [NAMES.index("Apple"), NAMES.index("Mug"), NAMES.index("Apple"), NAMES.index("Vase"), 13]
    return {"actor": torch.tensor([0, 0, 2, 3, 3], dtype=torch.int32), "t": torch.tensor([1, 2, 0, 1, 2], dtype=torch.int32),
            "length": torch.tensor([2, 1, 9, 5, 1], dtype=torch.int32), "category": torch.tensor(cat, dtype=torch.int32),
            "return": torch.tensor([9.5, -0.25, 9.75, -0.5, -0.125]), "success": torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0]),
            "spl": torch.tensor([1.0, 0.0, 0.5, 0.0, 0.0]), "soft_spl": torch.tensor([0.75, 0.25, 0.5, 0.0, 0.0]),
            "path": torch.tensor([0.5, 0.25, 2.0, 1.25, 0.0]), "goal_dist": torch.tensor([0.25, 3.0, 0.5, 7.0, 2.0]),
            "start_dist": torch.tensor([1.0, 2.0, 1.0, -1.0, 0.0]), "dropped": dropped}


def test_metrics_file_and_its_reader(tmp_path, capsys):
    path = str(tmp_path / "metrics.json")
    written = write_metrics_json(path, _records(), NAMES)
    metrics = json.load(open(path))
    assert metrics == written and isinstance(metrics, list) and len(metrics) == 1 and "dropped" not in metrics[0]
    tasks = metrics[0]["tasks"]
    assert len(tasks) == 5
    assert tasks[0] == {"task_info": {"object_type": "Apple", "actor": 0}, "success": 1.0, "spl": 1.0, "soft_spl": 0.75,
                        "ep_length": 2, "reward": 9.5, "dist_to_target": 0.25, "path_length": 0.5}
    assert [t["task_info"]["object_type"] for t in tasks] == ["Apple", "Mug", "Apple", "Vase", "13"]     # an id without a name
    # what a per-object-type reader does with the file
    apples = [t for t in metrics[0]["tasks"] if t["task_info"]["object_type"] == "Apple"]
    assert sum(t["success"] for t in apples) / len(apples) == 1.0 and sum(t["spl"] for t in apples) / len(apples) == 0.75
    scores = scores_by_object_type(path, NAMES)
    assert list(scores) == NAMES
    assert scores["Apple"] == (1.0, 0.75) and scores["Mug"] == (0.0, 0.0) and scores["Vase"] == (0.0, 0.0)
    assert all(math.isnan(x) for x in scores["Bowl"])                       # no episodes: NaN, not a division error
    assert scores_by_object_type(metrics, NAMES)["Apple"] == scores["Apple"]
    assert capsys.readouterr().err == ""
    # default names
    assert metrics_from_records(_records())[0]["tasks"][1]["task_info"]["object_type"] == str(NAMES.index("Mug"))


def test_dropped_episodes_are_reported(tmp_path, capsys):
    path = str(tmp_path / "metrics.json")
    write_metrics_json(path, _records(dropped=3), NAMES)
    metrics = json.load(open(path))
    assert metrics[0]["dropped"] == 3 and len(metrics[0]["tasks"]) == 5
    assert "3 episodes" in capsys.readouterr().err


def test_records_dropped_comes_from_the_count():
    """``dropped`` is n_records - capacity: the tracker's own arithmetic on CPU stand-ins of its buffers."""
    tr = ep.NavEpisodeTracker.__new__(ep.NavEpisodeTracker)
    tr.capacity, tr.device = 4, torch.device("cpu")
    tr.n_records = torch.tensor([7], dtype=torch.int32)
    tr.rec_f = torch.arange(28, dtype=torch.float32).reshape(4, 7)
    tr.rec_i = torch.arange(16, dtype=torch.int32).reshape(4, 4)
    rec = tr.records()
    assert rec["dropped"] == 3 and rec["category"].tolist() == [3, 7, 11, 15] and rec["start_dist"].tolist() == [6.0, 13.0, 20.0, 27.0]
    assert metrics_from_records(rec, NAMES)[0]["dropped"] == 3
