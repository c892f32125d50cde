"""Generates the probe-label fixtures with the REFERENCE'S OWN CODE, read from a checkout of it at run time:

    python tests/golden/make_probe_labels_golden.py /path/to/embodied-clip        (from the repository root; CPU only)

  tests/golden/probe_target_objects.json    ``target_objects`` of primitive_probing/constants.py
  tests/golden/probe_labels_golden.npz      seeds, sizes, colour tables and the labels that ``class_mask``,
                                            ``obj_presence`` and ``grid_bboxes`` of generate_data/thor_image_features.py
                                            give for the frames of tests/_probe_label_frames.py
  tests/golden/probe_reachable_golden.json  input JSONs of a small CSR-shaped directory and what
                                            generate_data/reachable_metadata.py, run as a child process, wrote for it
                                            (sorted per split: the reference shuffles unseeded)

The three label functions are cut out of the script with ``ast`` and executed in a namespace that holds only numpy (the
script itself imports CUDA-only packages at module level); the label expressions are those of its lines 115-127.  This
file holds none of the reference's text."""
import ast
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _probe_label_frames as plf  # noqa: E402
from embodied_clip_amd import synthetic as syn  # noqa: E402


def reference_functions(ref_root):
    path = os.path.join(ref_root, "primitive_probing", "generate_data", "thor_image_features.py")
    tree = ast.parse(open(path).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("class_mask", "obj_presence", "grid_bboxes")]
    assert len(keep) == 3
    ns = {"np": np}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["class_mask"], ns["obj_presence"], ns["grid_bboxes"]


def reference_targets(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, "primitive_probing", "constants.py")).read())
    for n in tree.body:
        if isinstance(n, ast.Assign) and n.targets[0].id == "target_objects":
            return list(ast.literal_eval(n.value))
    raise AssertionError("constants.py: no target_objects")


def check_label_fixture(presence, localization):
    """What keeps a lazy kernel from passing (tests/test_probe_extract.py re-asserts it on the committed file)."""
    assert 0.15 <= presence.mean() <= 0.70, presence.mean()
    assert 0.03 <= localization.mean() <= 0.50, localization.mean()
    assert (presence.max(axis=0) == 1).sum() >= 40 and (presence.min(axis=0) == 0).all()
    for cell in range(9):
        assert localization[:, cell].min() == 0 and localization[:, cell].max() == 1, cell
    assert np.array_equal(localization.max(axis=1), presence)


def make_labels(ref_root, targets):
    class_mask, obj_presence, grid_bboxes = reference_functions(ref_root)
    frames = plf.all_frames(targets)
    pres, loc, seconds = [], [], []
    for sem, d, _tab in frames:
        t0 = time.perf_counter()
        class_masks = np.array([class_mask(sem, d.get(o, None)) for o in targets])
        p = obj_presence(class_masks)
        g = [obj_presence(class_masks[:, y1:y2, x1:x2]) for (y1, y2, x1, x2) in grid_bboxes(class_masks.shape[1:3], (3, 3))]
        seconds.append(time.perf_counter() - t0)
        pres.append(np.asarray(p).astype(np.int64))
        loc.append(np.asarray(g).astype(np.int64))
    pres, loc = np.stack(pres), np.stack(loc)
    check_label_fixture(pres, loc)
    # the special dictionary entries do something in their frames
    a, b = plf.DUPLICATE_CLASSES
    assert pres[plf.DUPLICATE_FRAME, a] == 1 and pres[plf.DUPLICATE_FRAME, b] == 1
    assert pres[plf.BACKGROUND_FRAME, plf.BACKGROUND_CLASS] == 1 and pres[plf.FOREIGN_FRAME, plf.OUT_OF_RANGE_CLASS] == 0
    assert all(loc[i, 8, 3] == 1 for i in range(len(frames)) if 3 % 7 != i % 7)         # the pixel at (H-1, W-1)
    path = os.path.join(HERE, "probe_labels_golden.npz")
    np.savez_compressed(path, seeds=np.array(plf.SEEDS), sizes=np.array(plf.SIZES), tables=np.stack([t for _, _, t in frames]),
                        object_presence=pres, object_localization=loc, reference_cpu_seconds=np.array(seconds))
    print("wrote", path, os.path.getsize(path), "bytes; ones:", round(float(pres.mean()), 3), round(float(loc.mean()), 3),
          "classes seen:", int((pres.max(axis=0) == 1).sum()), "reference seconds per 300x300 frame:", round(min(seconds[:4]), 4))


def csr_directory(seed=7):
    """{file name: JSON object} of a CSR-shaped directory: three splits of about 60 images; ids such as Mug_12, some
    without '_'; about 40 % of the boxes pickupable."""
    classes = ["Mug", "Apple", "Bowl", "Book", "Laptop", "Vase", "Pen", "Cup", "Plate", "Knife", "Sofa", "Fridge", "Television"]
    files = {}
    for k, split in enumerate(("train", "val", "test")):
        n = 58 + 3 * k
        h = syn.hash_u64(seed + k, n * 8 * 3, stream=41).reshape(n, 8, 3)
        boxes, pick = {}, {}
        for i in range(n):
            name = f"{split}_{i:04d}"
            objs, reach = {}, []
            for j in range(2 + int(h[i, 0, 2] % np.uint64(5))):
                cls = classes[int(h[i, j, 0] % np.uint64(len(classes if k == 0 else classes[:-1 - k])))]
                oid = cls if int(h[i, j, 1] % np.uint64(5)) == 0 else f"{cls}_{int(h[i, j, 1] % np.uint64(40))}"
                objs[oid] = [int(v) for v in (h[i, j] % np.uint64(200))] + [223]
                if int(h[i, j, 2] >> np.uint64(8)) % 100 < 40:
                    reach.append(oid)
            boxes[name], pick[name] = objs, reach
        files[f"{split}_boxes.json"], files[f"{split}_boxes_pickupable.json"] = boxes, pick
    return files


def make_reachable(ref_root):
    files = csr_directory()
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "edge_full"), os.path.join(tmp, "out")
        os.makedirs(src), os.makedirs(dst)
        for name, obj in files.items():
            json.dump(obj, open(os.path.join(src, name), "w"))
        script = os.path.join(ref_root, "primitive_probing", "generate_data", "reachable_metadata.py")
        subprocess.run([sys.executable, script, "--data_dir", src, "--output_dir", dst], check=True)
        triples = {s: sorted((im, int(o), bool(r)) for im, o, r in pickle.load(open(os.path.join(dst, f"reachable_{s}.pkl"), "rb")))
                   for s in ("train", "val", "test")}
    cls = lambda o: o.split("_", 1)[0]  # noqa: E731
    superset = sorted({cls(o) for s in ("train", "val", "test") for objs in files[f"{s}_boxes.json"].values() for o in objs})
    for s, rows in triples.items():
        assert len(rows) >= 60, (s, len(rows))
        # the reference keeps its superset to itself; its obj_ids pin ours: every triple's class is in its image
        assert all(superset[o] in {cls(k) for k in files[f"{s}_boxes.json"][im]} for im, o, _r in rows)
        # some class has more negatives in the input than the reference kept
        neg_in = {}
        for im, objs in files[f"{s}_boxes.json"].items():
            reach = {cls(o) for o in files[f"{s}_boxes_pickupable.json"][im]}
            for c in {cls(o) for o in objs}:
                if c not in reach:
                    neg_in[c] = neg_in.get(c, 0) + 1
        neg_out = {}
        for _im, o, r in rows:
            if not r:
                neg_out[superset[o]] = neg_out.get(superset[o], 0) + 1
        assert any(neg_in[c] > neg_out.get(c, 0) for c in neg_in), s
    path = os.path.join(HERE, "probe_reachable_golden.json")
    json.dump({"files": files, "object_superset": superset, "triples": {s: [list(t) for t in r] for s, r in triples.items()}},
              open(path, "w"), separators=(",", ":"))
    print("wrote", path, os.path.getsize(path), "bytes; triples:", {s: len(r) for s, r in triples.items()})


if __name__ == "__main__":
    ref = sys.argv[1]
    targets = reference_targets(ref)
    json.dump(targets, open(os.path.join(HERE, "probe_target_objects.json"), "w"))
    make_labels(ref, targets)
    make_reachable(ref)
