"""Seeded semantic frames and colour dictionaries for the probe-label tests: ONE recipe, imported by
tests/golden/make_probe_labels_golden.py (which labels them with the reference's own functions) and by the tests (which
rebuild the same frames from the seeds the fixture stores).  Built on the portable hash generator, so the frames are
the same on every machine."""
import numpy as np

from embodied_clip_amd import synthetic as syn

SIZES = [(300, 300)] * 4 + [(224, 224)] * 2 + [(301, 299), (64, 97)]
SEEDS = [4100 + i for i in range(len(SIZES))]
N_PALETTE, N_RECTS = 70, 40
# frames with something special in their dictionary
FOREIGN_FRAME, DUPLICATE_FRAME, BACKGROUND_FRAME = 1, 2, 3
OUT_OF_RANGE_CLASS, DUPLICATE_CLASSES, BACKGROUND_CLASS = 10, (20, 21), 30


def palette_of(seed):
    """70 distinct colours; entries 0 and 1 differ by one bit of the last channel."""
    h = syn.hash_u64(seed, N_PALETTE, stream=31)
    pal = np.zeros((N_PALETTE, 3), dtype=np.uint8)
    pal[:, 0] = (h & np.uint64(255)).astype(np.uint8)
    pal[:, 1] = ((h >> np.uint64(8)) & np.uint64(255)).astype(np.uint8)
    pal[:, 2] = (np.arange(N_PALETTE) * 3).astype(np.uint8)          # distinct last channel: 0, 3, 6, ...
    pal[1] = pal[0]
    pal[1, 2] = pal[0, 2] ^ 1
    return pal


def background_index(seed):
    return int(syn.hash_u64(seed, 1, stream=32)[0] % np.uint64(N_PALETTE))


def semantic_frame(seed, h, w):
    """uint8 [h, w, 3]: a background of one palette colour, 40 filled rectangles of palette colours, a 4 x 6 patch of
    palette colour 21 in the middle, one pixel of palette colour 2 at (h/3 - 1, w/3 - 1) and one of palette colour 3 at (h - 1, w - 1)."""
    pal = palette_of(seed)
    img = np.empty((h, w, 3), dtype=np.uint8)
    img[:] = pal[background_index(seed)]
    r = syn.hash_u64(seed, N_RECTS * 5, stream=33).reshape(N_RECTS, 5)
    for k in range(N_RECTS):
        y0, x0 = int(r[k, 0] % np.uint64(h)), int(r[k, 1] % np.uint64(w))
        rh, rw = 1 + int(r[k, 2] % np.uint64(max(1, h // 3))), 1 + int(r[k, 3] % np.uint64(max(1, w // 3)))
        img[y0:y0 + rh, x0:x0 + rw] = pal[int(r[k, 4] % np.uint64(N_PALETTE))]
    img[h // 2:h // 2 + 4, w // 2:w // 2 + 6] = pal[DUPLICATE_CLASSES[1]]   # the shared colour of DUPLICATE_FRAME is on screen
    img[h // 3 - 1, w // 3 - 1] = pal[2]
    img[h - 1, w - 1] = pal[3]
    return img


def dictionary(index, seed, target_objects):
    """(object_id_to_color of frame ``index``, the uint8 [C, 4] table that dictionary MEANS, written down by
    construction).  Class c has palette colour c; palette colours >= C belong to objects that are no targets.  Every
    seventh class (offset by the frame index) is absent."""
    pal = palette_of(seed)
    C = len(target_objects)
    assert C <= N_PALETTE
    d, tab = {}, np.zeros((C, 4), dtype=np.uint8)
    for c, name in enumerate(target_objects):
        if c % 7 == index % 7:
            continue
        d[name] = tuple(int(v) for v in pal[c])
        tab[c] = [*pal[c], 1]
    for k in range(C, N_PALETTE):
        d[f"Structure{k}"] = tuple(int(v) for v in pal[k])
    if index == FOREIGN_FRAME:
        # instance ids are keys of the simulator's dictionary too, and are never looked up; one colour out of range
        d[f"{target_objects[25]}|1|2|3"] = tuple(int(v) for v in pal[60])
        d[f"{target_objects[0]}|-01.20|+00.90|+02.10"] = tuple(int(v) for v in pal[61])
        d[target_objects[OUT_OF_RANGE_CLASS]] = (300, int(pal[OUT_OF_RANGE_CLASS, 1]), int(pal[OUT_OF_RANGE_CLASS, 2]))
        tab[OUT_OF_RANGE_CLASS] = 0
    if index == DUPLICATE_FRAME:
        a, b = DUPLICATE_CLASSES
        d[target_objects[a]] = d[target_objects[b]]
        tab[a] = tab[b]
    if index == BACKGROUND_FRAME:
        bg = pal[background_index(seed)]
        d[target_objects[BACKGROUND_CLASS]] = tuple(int(v) for v in bg)
        tab[BACKGROUND_CLASS] = [*bg, 1]
    return d, tab


def all_frames(target_objects):
    """[(semantic frame, object_id_to_color, table), ...] of the eight fixture frames."""
    out = []
    for i, ((h, w), seed) in enumerate(zip(SIZES, SEEDS)):
        d, tab = dictionary(i, seed, target_objects)
        out.append((semantic_frame(seed, h, w), d, tab))
    return out
