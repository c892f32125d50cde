"""Probe labels from simulator scene files (``thor_image_features.py:70-127,137``) and the reachability metadata
(``reachable_metadata.py``): what lies between ``thor_frames.py``'s ``ithor_scenes/{split}/<scene>.npy`` / the CSR
``edge_full`` directory and ``probe_data``'s cache writer.

    read_scene_file      np.load(scene, allow_pickle=True)                                     (:98)
    color_table          object_id_to_color.get(o) per target object -> uint8 [C, 4]           (:118)
    semantic_labels      class_mask / obj_presence / grid_bboxes on the GPU (ec_semantic_labels_u8, labels.hip):
                         object_presence int64 [n, C], object_localization int64 [n, 9, C]     (:71-88,115-127)
    label_points         scene points -> the points ``probe_data.build_thor_features`` takes
    build_reachable_metadata   reachable_metadata.py:18-66 (host only: a few JSON files)

The target object names are the reference's data (constants.py) and are not kept in the package: every function takes
them as an argument.  There is no host implementation of the labels; without the HIP library / a GPU they raise.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import synthetic as syn

MAX_CLASSES = 64
SPLITS = ("train", "val", "test")


def read_target_objects(path: str) -> List[str]:
    """A JSON list of names, or one name per line."""
    with open(path) as f:
        txt = f.read()
    if txt.lstrip().startswith("["):
        names = json.loads(txt)
    else:
        names = [ln.strip() for ln in txt.splitlines() if ln.strip()]
    if not names or not all(isinstance(n, str) for n in names) or len(names) > MAX_CLASSES:
        raise ValueError(f"{path}: expected 1..{MAX_CLASSES} object names")
    return list(names)


def read_scene_file(path: str) -> List[dict]:
    """``np.load(scene, allow_pickle=True)`` (thor_image_features.py:98): the pickled list of points thor_frames.py:88-104
    writes (the file is a pickle: load only files you made)."""
    return list(np.load(path, allow_pickle=True))


def color_table(object_id_to_color, target_objects: Sequence[str]) -> np.ndarray:
    """uint8 [C, 4] = r, g, b, valid of ``object_id_to_color.get(name)`` per target name (thor_image_features.py:118).
    valid = 0 where the name is missing (``class_mask`` returns an empty mask, :72-73) and where the colour cannot equal
    a uint8 pixel (not three components, or a component outside 0..255: ``np.all(frame == colour, -1)`` is all False).
    Keys that are not target names (instance ids such as ``Mug|1|2|3``) are never looked up."""
    none = (0, 0, 0, 0)
    rows = []
    for name in target_objects:
        row = none
        col = object_id_to_color.get(name, None)
        if col is not None:
            try:
                r, g, b = col
                if 0 <= r <= 255 and 0 <= g <= 255 and 0 <= b <= 255 and r == int(r) and g == int(g) and b == int(b):
                    row = (int(r), int(g), int(b), 1)
            except (TypeError, ValueError):       # not three numbers
                pass
        rows.append(row)
    return np.array(rows, dtype=np.uint8).reshape(len(rows), 4)


def _as_u8(a, what: str) -> torch.Tensor:
    t = torch.as_tensor(np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a)
    if t.dtype != torch.uint8:
        raise TypeError(f"{what} must be uint8, got {t.dtype}")
    return t


def _labels_batch(lib, sem: torch.Tensor, col: torch.Tensor, device) -> Tuple[torch.Tensor, torch.Tensor]:
    n, H, W, _ = sem.shape
    C = col.shape[1]
    with torch.cuda.device(device):
        s = sem.pin_memory().to(device, non_blocking=True)           # one upload per batch
        c = col.contiguous().to(device)
        pres = torch.empty(n, C, dtype=torch.int64, device=device)
        loc = torch.empty(n, 9, C, dtype=torch.int64, device=device)
        _lib.check(lib.ec_semantic_labels_u8(_lib.ptr(s), _lib.ptr(c), _lib.ptr(pres), _lib.ptr(loc), n, H, W, C,
                                             _lib.stream_ptr(device)), "ec_semantic_labels_u8")
        return pres.cpu(), loc.cpu()


def semantic_labels(sem_u8, colors, device="cuda:0", batch: int = 64) -> Tuple[torch.Tensor, torch.Tensor]:
    """``sem_u8``: uint8 [n, H, W, 3], or a sequence of n uint8 [H_i, W_i, 3] frames of mixed sizes (grouped by size);
    ``colors``: uint8 [n, C, 4] (``color_table`` per frame).  Returns (object_presence int64 [n, C],
    object_localization int64 [n, 9, C]) on the host.  Batched like ``ClipFeatureExtractor`` (``batch`` frames per
    upload and launch); a frame's labels do not depend on the batch it is in."""
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise RuntimeError("embodied_clip_amd.probe_labels.semantic_labels needs an MI355X (no CPU fallback)")
    device = torch.device(device)
    col = _as_u8(colors, "colors")
    frames = [_as_u8(f, "semantic frame") for f in sem_u8]
    n = len(frames)
    if col.dim() != 3 or col.shape[0] != n or col.shape[2] != 4 or not 1 <= col.shape[1] <= MAX_CLASSES:
        raise ValueError(f"colors must be uint8 [n={n}, C<={MAX_CLASSES}, 4], got {tuple(col.shape)}")
    C = col.shape[1]
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, f in enumerate(frames):
        if f.dim() != 3 or f.shape[2] != 3 or f.shape[0] < 3 or f.shape[1] < 3:
            raise ValueError(f"semantic frame {i}: expected [H>=3, W>=3, 3], got {tuple(f.shape)}")
        groups.setdefault((f.shape[0], f.shape[1]), []).append(i)
    pres = torch.zeros(n, C, dtype=torch.int64)
    loc = torch.zeros(n, 9, C, dtype=torch.int64)
    for idx in groups.values():
        for j in range(0, len(idx), batch):
            sel = idx[j:j + batch]
            p, l = _labels_batch(lib, torch.stack([frames[i] for i in sel]).contiguous(), col[sel], device)
            pres[sel], loc[sel] = p, l
    return pres, loc


def label_points(points: Sequence[dict], target_objects: Sequence[str], device="cuda:0", batch: int = 64) -> List[dict]:
    """Scene points (``frame``, ``semantic_frame``, ``object_id_to_color``, ``valid_moves_forward``) -> the points
    ``build_thor_features`` takes: ``frame``, ``object_presence`` int64 [C], ``object_localization`` int64 [9, C]
    (thor_image_features.py:115-127) and ``free_space`` = ``valid_moves_forward`` (:137)."""
    if not len(points):
        return []
    cols = np.stack([color_table(p["object_id_to_color"], target_objects) for p in points])
    pres, loc = semantic_labels([p["semantic_frame"] for p in points], cols, device, batch)
    return [{"frame": p["frame"], "object_presence": pres[i], "object_localization": loc[i],
             "free_space": int(p["valid_moves_forward"])} for i, p in enumerate(points)]


# ------------------------------------------------------------------------------------------------
# reachability metadata (reachable_metadata.py; host only)
# ------------------------------------------------------------------------------------------------
def thor_id_to_class(thor_id: str) -> str:
    """Text before the first ``_`` (reachable_metadata.py:18-21)."""
    return thor_id.split("_", 1)[0]


def build_reachable_metadata(data_dir: str, seed: int = 1):
    """(object_superset, {split: [(image, obj_id, reachable), ...]}) from ``{split}_boxes.json`` and
    ``{split}_boxes_pickupable.json`` of the CSR ``edge_full`` directory.  Superset: sorted classes over the three
    splits (:24-36).  Per image one triple per distinct class (:49-54); per class all positives and the FIRST
    ``len(positives)`` negatives in insertion order (:56-60).  The reference then shuffles with the unseeded global
    ``random`` (:66); here the order is the portable hash permutation of ``probe_data._Loader`` from ``seed``, so the
    content of each split equals the reference's and the order is reproducible."""
    def load(name):
        with open(os.path.join(data_dir, name)) as f:
            return json.load(f)

    boxes = {s: load(f"{s}_boxes.json") for s in SPLITS}
    superset = sorted({thor_id_to_class(o) for s in SPLITS for objs in boxes[s].values() for o in objs.keys()})
    index = {name: i for i, name in enumerate(superset)}
    out = {}
    for k, split in enumerate(SPLITS):
        labels = load(f"{split}_boxes_pickupable.json")
        per_class: List[list] = [[] for _ in superset]
        for image, objs in boxes[split].items():
            reachable = {thor_id_to_class(o) for o in labels[image]}
            for obj in sorted({thor_id_to_class(o) for o in objs.keys()}):
                per_class[index[obj]].append((image, index[obj], obj in reachable))
        rows = []
        for data in per_class:
            positives = [d for d in data if d[2]]
            rows += [d for d in data if not d[2]][:len(positives)] + positives
        order = np.argsort(syn.hash_u64(seed + k, len(rows), stream=22), kind="stable")
        out[split] = [rows[int(j)] for j in order]
    return superset, out
