"""GPU side of the probe-cache builder: ``ec_semantic_labels_u8`` against the labels the reference's own functions gave
(tests/golden/probe_labels_golden.npz, made by tests/golden/make_probe_labels_golden.py), and the ``probe_extract`` CLI from
raw scene files / PNGs to a cache that ``probe_train`` trains on.  The labels are integer equality: tolerance zero."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _probe_label_frames as plf  # noqa: E402
from embodied_clip_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TARGETS_FILE = os.path.join(GOLDEN, "probe_target_objects.json")


def _targets():
    return json.load(open(TARGETS_FILE))


def _golden():
    g = np.load(os.path.join(GOLDEN, "probe_labels_golden.npz"))
    return torch.from_numpy(g["object_presence"]), torch.from_numpy(g["object_localization"]), g["tables"]


def test_kernel_equals_the_reference_labels_on_all_fixture_frames():
    from embodied_clip_amd.probe_labels import color_table, semantic_labels
    targets = _targets()
    frames = plf.all_frames(targets)
    pres_ref, loc_ref, tables = _golden()
    cols = np.stack([color_table(d, targets) for _, d, _ in frames])
    assert np.array_equal(cols, tables)
    pres, loc = semantic_labels([sem for sem, _, _ in frames], cols, "cuda:0")        # mixed sizes: grouped by size
    print("ones: presence", float(pres.double().mean()), "localization", float(loc.double().mean()),
          "| mismatches:", int((pres != pres_ref).sum()), int((loc != loc_ref).sum()))
    assert pres.dtype == torch.int64 and loc.dtype == torch.int64
    assert pres.shape == (8, 52) and loc.shape == (8, 9, 52)
    assert torch.equal(pres, pres_ref)
    assert torch.equal(loc, loc_ref)


def test_labels_do_not_depend_on_the_batch():
    from embodied_clip_amd.probe_labels import semantic_labels
    targets = _targets()
    frames = plf.all_frames(targets)
    pres_ref, loc_ref, tables = _golden()
    for i, (sem, _, _) in enumerate(frames):                                           # alone
        p, l = semantic_labels(sem[None], tables[i:i + 1], "cuda:0")
        assert torch.equal(p[0], pres_ref[i]) and torch.equal(l[0], loc_ref[i]), i
    four = np.stack([frames[i][0] for i in range(4)])                                   # a batch of 4
    p, l = semantic_labels(four, tables[:4], "cuda:0")
    assert torch.equal(p, pres_ref[:4]) and torch.equal(l, loc_ref[:4])
    for i in (1, 6):                                                                    # 65 repeats: crosses the batch of 64
        sem = np.repeat(frames[i][0][None], 65, axis=0)
        p, l = semantic_labels(sem, np.repeat(tables[i:i + 1], 65, axis=0), "cuda:0", batch=64)
        assert torch.equal(p, pres_ref[i].expand(65, -1)) and torch.equal(l, loc_ref[i].expand(65, -1, -1)), i


def _numpy_labels(sem, table):
    """Equality of all three channels per class, any() per cell -- written out once more for shapes the fixture has not
    (the fixture's expected values come from the reference; these cases have no reference run behind them)."""
    H, W, _ = sem.shape
    C = table.shape[0]
    loc = np.zeros((9, C), dtype=np.int64)
    for c in range(C):
        if not table[c, 3]:
            continue
        m = (sem == table[c, :3]).all(-1)
        for i in range(3):
            for j in range(3):
                loc[i * 3 + j, c] = m[i * H // 3:(i + 1) * H // 3, j * W // 3:(j + 1) * W // 3].any()
    return loc.max(0), loc


@pytest.mark.parametrize("H,W,C,n_colours", [(3, 3, 64, 5), (5, 7, 1, 2), (33, 1030, 64, 90), (300, 300, 52, 200), (97, 64, 13, 3)])
def test_noise_frames_edge_sizes_and_class_counts(H, W, C, n_colours):
    """Every pixel its own colour draw (no wave sees one colour), frames smaller than one pass and wider than one,
    C = 1 and C = 64."""
    from embodied_clip_amd.probe_labels import semantic_labels
    n = 3
    u = syn.hash_u64(H * 1000 + W, n * H * W + n_colours * 3 + n * C * 2, stream=51)
    pal = (u[:n_colours * 3] % np.uint64(256)).astype(np.uint8).reshape(n_colours, 3)
    sem = pal[(u[n_colours * 3:n_colours * 3 + n * H * W] % np.uint64(n_colours)).astype(np.int64)].reshape(n, H, W, 3)
    sem[:, H // 2:, :W // 2] = pal[0]                                   # one flat region as well
    k = u[n_colours * 3 + n * H * W:].reshape(n, C, 2)
    table = np.zeros((n, C, 4), dtype=np.uint8)
    table[:, :, :3] = pal[(k[:, :, 0] % np.uint64(n_colours)).astype(np.int64)]
    table[:, :, 3] = (k[:, :, 1] % np.uint64(4) != 0)
    pres, loc = semantic_labels(sem, table, "cuda:0")
    for b in range(n):
        p_ref, l_ref = _numpy_labels(sem[b], table[b])
        assert np.array_equal(pres[b].numpy(), p_ref) and np.array_equal(loc[b].numpy(), l_ref), b


# ------------------------------------------------------------------------------------------------
# the CLI: raw scene files -> thor_{split}.pt -> probe_train
# ------------------------------------------------------------------------------------------------
# scene -> (split, fixture frame indices, number of points); a scene holds frames of one size
SCENES = {"FloorPlan1": ("train", (0, 1, 2, 3), 66), "FloorPlan201": ("train", (4, 5), 6),
          "FloorPlan2": ("val", (0, 1, 2, 3), 4), "FloorPlan202": ("val", (4, 5), 2),
          "FloorPlan3": ("test", (3, 2, 1, 0), 4), "FloorPlan203": ("test", (5, 4), 2)}


def _scene_points(name, targets, frames):
    _split, idx, n = SCENES[name]
    res = frames[idx[0]][0].shape[0]
    rgb = syn.synthetic_rgb_u8(int(name[len("FloorPlan"):]), n, res).numpy()
    pts = []
    for k in range(n):
        sem, d, _ = frames[idx[k % len(idx)]]
        pts.append({"frame": rgb[k], "semantic_frame": sem, "object_id_to_color": d, "valid_moves_forward": (5 * k + 3) % 15,
                    "agent_metadata": {"horizon": 0, "standing": True}})
    return pts, [idx[k % len(idx)] for k in range(n)]


@pytest.fixture(scope="module")
def thor_cache(tmp_path_factory):
    from embodied_clip_amd import probe_extract
    root = tmp_path_factory.mktemp("probe_extract")
    targets = _targets()
    frames = plf.all_frames(targets)
    for name, (split, _idx, _n) in SCENES.items():
        os.makedirs(str(root / "ithor_scenes" / split), exist_ok=True)
        np.save(str(root / "ithor_scenes" / split / f"{name}.npy"), _scene_points(name, targets, frames)[0])
    out = str(root / "data")
    probe_extract.main(["thor", "--data_dir", str(root / "ithor_scenes"), "--output_dir", out, "--target-objects", TARGETS_FILE,
                        "--synthetic-weights"])
    return out


def test_probe_extract_thor_from_scene_files(thor_cache, capsys):
    from embodied_clip_amd import probe_data as pd
    targets = _targets()
    frames = plf.all_frames(targets)
    pres_ref, loc_ref, _ = _golden()
    ex = pd.ClipFeatureExtractor(syn.rn50_visual_state_dict(0), device="cuda:0", imagenet_state_dict=syn.tv_resnet_state_dict(0))
    for split in ("train", "val", "test"):
        cache = torch.load(os.path.join(thor_cache, f"thor_{split}.pt"))
        assert sorted(cache) == sorted(n for n, (s, _, _) in SCENES.items() if s == split)
        for name, rows in cache.items():
            pts, which = _scene_points(name, targets, frames)
            assert len(rows) == len(pts)
            direct = ex(torch.stack([torch.from_numpy(p["frame"]) for p in pts]))          # the same frames in the same batches
            assert set(rows[0]) == set(direct) | {"object_presence", "object_localization", "free_space"}
            assert set(direct) == set(pd.CLIP_KEYS) | set(pd.IMAGENET_KEYS)
            for k, row in enumerate(rows):
                assert row["object_presence"].dtype == torch.int64 and torch.equal(row["object_presence"], pres_ref[which[k]])
                assert row["object_localization"].dtype == torch.int64 and torch.equal(row["object_localization"], loc_ref[which[k]])
                assert row["free_space"] == pts[k]["valid_moves_forward"] and isinstance(row["free_space"], int)
                for key, v in direct.items():
                    assert torch.equal(row[key], v[k]), (name, k, key)
        n = sum(c for s, _, c in SCENES.values() if s == split)
        for task in ("object_presence", "object_localization", "free_space"):
            ds = pd.THOREmbeddingsDataset(thor_cache, split, "clip_avgpool", task)
            assert len(ds) == n
            x, y = ds[0]
            assert x.shape == ((2048, 7, 7) if task == "object_localization" else (2048,))
        assert len(pd.THOREmbeddingsDataset(thor_cache, split, "imagenet_avgpool", "object_presence")) == n


def test_probe_train_runs_on_the_cache_made_from_scene_files(thor_cache, tmp_path, capsys):
    """The user's whole route: raw scene files -> probe_extract thor -> probe_train -> a probe number."""
    from embodied_clip_amd import probe_train
    capsys.readouterr()
    probe_train.main(["--data-dir", thor_cache, "--log-dir", str(tmp_path / "logs"), "--embedding-type", "clip_avgpool",
                      "--prediction-type", "object_localization", "--epochs", "2", "--batch-size", "8"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    print(line)
    assert line["train_frames"] == 72 and line["epochs"] == 2 and line["train_steps"] == 18
    for k in ("train_loss", "val_loss", "test_loss", "val_acc", "test_acc"):
        assert np.isfinite(line[k]), (k, line[k])
    assert line["train_loss"] > 0 and line["val_loss"] > 0


def test_probe_extract_reachable_from_png_files(tmp_path, capsys):
    Image = pytest.importorskip("PIL.Image")       # the one test of this feature that may skip: no Pillow, no PNGs
    from embodied_clip_amd import probe_data as pd
    from embodied_clip_amd import probe_extract
    src, out = tmp_path / "edge_full", str(tmp_path / "data")
    os.makedirs(str(src))
    rgb = syn.synthetic_rgb_u8(77, 3, 300).numpy()
    small = syn.synthetic_rgb_u8(78, 1, 224).numpy()[0]
    alpha = (syn.hash_u64(79, 300 * 300, stream=52) % np.uint64(256)).astype(np.uint8).reshape(300, 300, 1)
    Image.fromarray(rgb[0]).save(str(src / "kitchen_0001.png"))
    Image.fromarray(rgb[1]).save(str(src / "kitchen_0002.png"))
    Image.fromarray(np.concatenate([rgb[2], alpha], axis=2)).save(str(src / "bedroom.0003.png"))
    Image.fromarray(small).save(str(src / "small.png"))
    (src / "train_boxes.json").write_text("{}")                                           # not an image: left alone
    capsys.readouterr()
    probe_extract.main(["reachable", "--data_dir", str(src), "--output_dir", out, "--synthetic-weights"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["command"] == "reachable" and line["frames"] == 4
    table = torch.load(os.path.join(out, "reachable_image_features.pt"))
    assert sorted(table) == ["bedroom.0003", "kitchen_0001", "kitchen_0002", "small"]
    ex = pd.ClipFeatureExtractor(syn.rn50_visual_state_dict(0), device="cuda:0", imagenet_state_dict=syn.tv_resnet_state_dict(0))
    decoded = {n: torch.from_numpy(np.asarray(Image.open(str(src / f"{n}.png")).convert("RGB")).copy()) for n in table}
    assert torch.equal(decoded["bedroom.0003"], torch.from_numpy(rgb[2])) and torch.equal(decoded["kitchen_0001"], torch.from_numpy(rgb[0]))
    for group in (["bedroom.0003", "kitchen_0001", "kitchen_0002"], ["small"]):           # sorted names, one size per call
        direct = ex(torch.stack([decoded[n] for n in group]))
        for k, n in enumerate(group):
            assert set(table[n]) == {"imagenet_avgpool", "clip_avgpool", "clip_attnpool"}
            assert table[n]["imagenet_avgpool"].shape == (2048,) and table[n]["clip_avgpool"].shape == (2048,)
            assert table[n]["clip_attnpool"].shape == (1024,)
            for key in table[n]:
                assert torch.equal(table[n][key], direct[key][k]), (n, key)
