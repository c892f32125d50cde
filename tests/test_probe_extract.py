"""CPU side of the probe-cache builder (probe_labels.py / probe_extract.py): the fixtures made by the reference's own code
(tests/golden/make_probe_labels_golden.py) are what they must be, the C-ABI argument checks, the colour table, the scene
file reader, and the reachability metadata against reachable_metadata.py's recorded output."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _probe_label_frames as plf  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _targets():
    return json.load(open(os.path.join(GOLDEN, "probe_target_objects.json")))


def _labels():
    return np.load(os.path.join(GOLDEN, "probe_labels_golden.npz"))


def _reachable():
    return json.load(open(os.path.join(GOLDEN, "probe_reachable_golden.json")))


def _write_csr(dirname, files):
    os.makedirs(dirname, exist_ok=True)
    for name, obj in files.items():
        with open(os.path.join(dirname, name), "w") as f:
            json.dump(obj, f)


def test_label_fixture_cannot_be_met_by_a_lazy_kernel():
    g, targets = _labels(), _targets()
    pres, loc = g["object_presence"], g["object_localization"]
    assert len(targets) == 52 and pres.shape == (8, 52) and loc.shape == (8, 9, 52) and g["tables"].shape == (8, 52, 4)
    assert pres.dtype == np.int64 and loc.dtype == np.int64 and set(np.unique(pres)) == {0, 1} and set(np.unique(loc)) == {0, 1}
    assert [tuple(s) for s in g["sizes"]] == plf.SIZES and list(g["seeds"]) == plf.SEEDS
    assert 0.15 <= pres.mean() <= 0.70, pres.mean()
    assert 0.03 <= loc.mean() <= 0.50, loc.mean()
    assert (pres.max(axis=0) == 1).sum() >= 40, "at least 40 of the 52 classes are positive in some frame"
    assert (pres.min(axis=0) == 0).all(), "every class is negative in some frame"
    for cell in range(9):
        assert loc[:, cell].min() == 0 and loc[:, cell].max() == 1, cell
    assert np.array_equal(loc.max(axis=1), pres)


def test_reachable_fixture_has_truncated_negatives_and_enough_triples():
    g = _reachable()
    superset = g["object_superset"]
    assert superset == sorted(set(superset)) and any("_" not in o for s in ("train", "val", "test")
                                                    for objs in g["files"][f"{s}_boxes.json"].values() for o in objs)
    cls = lambda o: o.split("_", 1)[0]  # noqa: E731
    for s in ("train", "val", "test"):
        rows = g["triples"][s]
        assert len(rows) >= 60 and rows == sorted(rows)
        neg_in, neg_out = {}, {}
        for im, objs in g["files"][f"{s}_boxes.json"].items():
            reach = {cls(o) for o in g["files"][f"{s}_boxes_pickupable.json"][im]}
            for c in {cls(o) for o in objs}:
                if c not in reach:
                    neg_in[c] = neg_in.get(c, 0) + 1
        for _im, o, r in rows:
            if not r:
                neg_out[superset[o]] = neg_out.get(superset[o], 0) + 1
        assert any(neg_in[c] > neg_out.get(c, 0) for c in neg_in), s


def test_semantic_labels_argument_checks_need_no_gpu():
    from embodied_clip_amd import _lib
    lib = _lib.load()
    assert lib.ec_version() >= 610
    f = lib.ec_semantic_labels_u8
    assert f(None, None, None, None, 1, 300, 300, 52, None) == -1
    assert f(1, 1, 1, None, 1, 300, 300, 52, None) == -1
    assert f(1, 1, None, 1, 1, 300, 300, 52, None) == -1
    assert f(1, None, 1, 1, 1, 300, 300, 52, None) == -1
    assert f(None, 1, 1, 1, 1, 300, 300, 52, None) == -1
    assert f(1, 1, 1, 1, 1, 300, 300, 65, None) == -2
    assert f(1, 1, 1, 1, 1, 300, 300, 0, None) == -2
    assert f(1, 1, 1, 1, 1, 2, 300, 52, None) == -2
    assert f(1, 1, 1, 1, 1, 300, 2, 52, None) == -2
    assert f(1, 1, 1, 1, 0, 300, 300, 52, None) == -2


def test_color_table_on_the_fixture_dictionaries():
    from embodied_clip_amd.probe_labels import color_table
    g, targets = _labels(), _targets()
    for i, (_sem, d, tab) in enumerate(plf.all_frames(targets)):
        got = color_table(d, targets)
        assert got.dtype == np.uint8 and got.shape == (52, 4)
        assert np.array_equal(got, g["tables"][i]) and np.array_equal(got, tab), i
        absent = [c for c in range(52) if c % 7 == i % 7]
        assert (got[absent] == 0).all()                                     # missing name: valid = 0
    foreign = color_table(plf.dictionary(plf.FOREIGN_FRAME, plf.SEEDS[plf.FOREIGN_FRAME], targets)[0], targets)
    assert foreign[plf.OUT_OF_RANGE_CLASS, 3] == 0                          # 300 is no uint8 value
    assert foreign[25, 3] == 1 and foreign[0, 3] == 1                       # 'Mug|1|2|3' did not replace 'Mug'
    dup = color_table(plf.dictionary(plf.DUPLICATE_FRAME, plf.SEEDS[plf.DUPLICATE_FRAME], targets)[0], targets)
    a, b = plf.DUPLICATE_CLASSES
    assert dup[a, 3] == 1 and np.array_equal(dup[a], dup[b])
    # shapes a uint8 pixel can never equal
    assert color_table({"Mug": (1, 2)}, ["Mug"])[0, 3] == 0 and color_table({"Mug": (1, 2, 3, 255)}, ["Mug"])[0, 3] == 0
    assert color_table({"Mug": (-1, 2, 3)}, ["Mug"])[0, 3] == 0 and color_table({"Mug": (1.5, 2, 3)}, ["Mug"])[0, 3] == 0
    assert color_table({"Mug": np.array([1, 2, 255], dtype=np.uint8)}, ["Mug", "Cup"]).tolist() == [[1, 2, 255, 1], [0, 0, 0, 0]]


def test_read_scene_file_round_trip(tmp_path):
    from embodied_clip_amd.probe_labels import read_scene_file
    targets = _targets()
    frames = plf.all_frames(targets)
    data = []
    for i in range(3):                                                      # thor_frames.py:88-104's dictionary
        sem, d, _ = frames[i]
        data.append({"agent_metadata": {"position": {"x": 0.25 * i, "y": 0.9, "z": 1.0}, "rotation": dict(x=0, y=90 * i, z=0),
                                        "horizon": 0, "standing": True},
                     "object_metadata": [{"objectId": "Mug|1|2|3", "visible": True}],
                     "frame": np.full(sem.shape, i, dtype=np.uint8), "depth_frame": np.zeros(sem.shape[:2], dtype=np.float32),
                     "semantic_frame": sem, "instance_frame": sem[::-1].copy(), "object_id_to_color": d,
                     "valid_moves_forward": 3 * i})
    path = str(tmp_path / "FloorPlan1.npy")
    np.save(path, data)
    got = read_scene_file(path)
    assert isinstance(got, list) and len(got) == 3
    for a, b in zip(got, data):
        assert set(a) == set(b) and a["valid_moves_forward"] == b["valid_moves_forward"]
        assert a["object_id_to_color"] == b["object_id_to_color"]
        assert a["semantic_frame"].dtype == np.uint8 and np.array_equal(a["semantic_frame"], b["semantic_frame"])
        assert np.array_equal(a["frame"], b["frame"])


def test_build_reachable_metadata_equals_the_reference_output(tmp_path):
    from embodied_clip_amd.probe_labels import build_reachable_metadata
    g = _reachable()
    d = str(tmp_path / "edge_full")
    _write_csr(d, g["files"])
    superset, triples = build_reachable_metadata(d, seed=1)
    assert superset == g["object_superset"]
    again = build_reachable_metadata(d, seed=1)[1]
    other = build_reachable_metadata(d, seed=2)[1]
    for s in ("train", "val", "test"):
        assert all(isinstance(im, str) and type(o) is int and type(r) is bool for im, o, r in triples[s])
        assert sorted([im, o, r] for im, o, r in triples[s]) == g["triples"][s], s     # the same multiset of triples
        assert triples[s] == again[s]
        assert triples[s] != other[s] and sorted(triples[s]) == sorted(other[s])
        assert triples[s] != sorted(triples[s])                                         # shuffled


def test_probe_extract_reachable_metadata_cli(tmp_path, capsys):
    from embodied_clip_amd import probe_extract
    g = _reachable()
    d, out = str(tmp_path / "edge_full"), str(tmp_path / "data")
    _write_csr(d, g["files"])
    probe_extract.main(["reachable-metadata", "--data_dir", d, "--output_dir", out, "--seed", "3"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["command"] == "reachable-metadata" and line["classes"] == len(g["object_superset"])
    for s in ("train", "val", "test"):
        with open(os.path.join(out, f"reachable_{s}.pkl"), "rb") as fh:      # what THOREmbeddingsDataset does (data.py:36-37)
            triples = pickle.load(fh)
        assert line["triples"][s] == len(triples) == len(g["triples"][s])
        assert sorted([im, o, r] for im, o, r in triples) == g["triples"][s]
        image, obj, r = triples[0]
        assert torch.tensor(r, dtype=torch.int64).item() in (0, 1) and 0 <= obj < len(g["object_superset"])
    assert not os.path.exists(os.path.join(out, "reachable_image_features.pt"))


def test_probe_extract_gpu_commands_refuse_to_run_without_a_gpu(tmp_path, monkeypatch):
    from embodied_clip_amd import probe_extract
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no CPU fallback"):
        probe_extract.main(["thor", "--data_dir", str(tmp_path), "--output_dir", str(tmp_path), "--synthetic-weights",
                            "--target-objects", os.path.join(GOLDEN, "probe_target_objects.json")])
    with pytest.raises(SystemExit, match="no CPU fallback"):
        probe_extract.main(["reachable", "--data_dir", str(tmp_path), "--output_dir", str(tmp_path), "--synthetic-weights"])
