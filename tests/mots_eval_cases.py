"""The inputs of tests/test_gpu_mots_eval.py, built on the host.  tests/test_mots_eval_host.py checks on the oracle alone that each case
holds the situation it is named after, before anything goes to the device."""
import functools
import json

import numpy as np

from tests import data_oracle as do
from tests import mots_eval_oracle as oracle

LABEL_SHAPES = [(7, 5), (1, 40), (40, 1), (37, 53), (130, 200)]
STATUS_CASES = ("empty", "bad_char_high", "open_group", "negative_count", "short_sum")          # one string per status 1, 2, 4, 8, 16


# ------------------------------------------------------------------------------------------------ rle_decode_labels
def bands(h, w, n):
    """n disjoint masks that tile the plane: bands of the row-major pixel index, so that a band's edges cut rows (several runs per
    column in the column-major strings).  With n above h * w some masks are empty."""
    idx = np.arange(h * w).reshape(h, w) * n // (h * w)
    return [idx == k for k in range(n)]


def blob(h, w, rng):
    """A rectangle of at least one pixel."""
    y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
    m = np.zeros((h, w), bool)
    m[y0:y0 + 1 + int(rng.integers(0, max(1, h // 2))), x0:x0 + 1 + int(rng.integers(0, max(1, w // 2)))] = True
    return m


PLANES = ("nobody-first", "disjoint", "two-overlap", "three-overlap", "ones-and-zeros", "refused-among-accepted", "seventy", "nobody-last")


@functools.lru_cache(maxsize=None)
def label_case(h, w):
    """One call with a plane per data case -> dict(strings, planes, labels, P, h, w, masks (dense, None for a refused string),
    want = the oracle's (maps, overlap, status))."""
    rng = np.random.default_rng(1000 * h + w)
    strings, planes, labels, masks = [], [], [], []

    def add(q, mask, label):
        strings.append(do.mask_string(mask.astype(np.uint8)))
        planes.append(q)
        labels.append(label)
        masks.append(mask)
    for mask, label in zip(bands(h, w, 5), (9, 1, 65535, 300, 2)):                 # disjoint; labels 1 and 65535 among them
        add(1, mask, label)
    a = np.zeros((h, w), bool)
    a.reshape(-1)[:(h * w * 2) // 3] = True
    b = np.zeros((h, w), bool)
    b.reshape(-1)[(h * w) // 3:] = True
    add(2, a, 40)
    add(2, b, 7)                                                                   # the later string has the SMALLER label: 40 wins
    c = np.zeros((w, h), bool)
    c.reshape(-1)[(h * w) // 4:(3 * h * w) // 4] = True                            # the middle half in COLUMN-major order
    c = np.ascontiguousarray(c.T)
    add(3, a, 5)
    add(3, c, 600)
    add(3, b, 70)
    add(4, np.ones((h, w), bool), 7)
    add(4, np.zeros((h, w), bool), 9)
    bad = {name: s for name, s, _ in do.malformed_cases(h, w)}
    good = bands(h, w, len(STATUS_CASES) + 1)
    for k, name in enumerate(STATUS_CASES):
        add(5, good[k], 10 + k)
        strings.append(bad[name])
        planes.append(5)
        labels.append(65535)                                                       # would win everywhere if it were decoded
        masks.append(None)
    add(5, good[-1], 3)
    seventy = bands(h, w, 70) if h * w >= 700 else [blob(h, w, rng) for _ in range(70)]
    for k, mask in enumerate(seventy):
        add(6, mask, int(rng.integers(1, 65536)))
    P = len(PLANES)
    want = oracle.decode_labels(strings, planes, labels, P, h, w)
    for arr in want:
        arr.setflags(write=False)
    return dict(strings=strings, planes=planes, labels=labels, P=P, h=h, w=w, masks=masks, want=want)


# ------------------------------------------------------------------------------------------------ label_pair_counts
def _noise(rng, T, H, W, K, above=0):
    """Blocks of 1 .. 9 equal labels along the rows, labels 0 .. K + above, about half of them 0."""
    n = T * H * W
    vals = rng.integers(0, K + above + 1, n) * (rng.random(n) < 0.5)
    return np.repeat(vals, rng.integers(1, 10, n))[:n].reshape(T, H, W).astype(np.uint16)


def _pair_small():
    rng = np.random.default_rng(1)
    return _noise(rng, 1, 5, 7, 3), _noise(rng, 1, 5, 7, 3), 3, 3


def _pair_medium():
    rng = np.random.default_rng(2)
    a, b = _noise(rng, 3, 37, 53, 5, above=3), _noise(rng, 3, 37, 53, 9, above=3)
    b[0, 3, 10:30], b[2, 30:, 50] = 65535, 40000                                    # far above K, on top of whatever a holds there
    return a, b, 5, 9


def _pair_large():
    """130 x 200, T = 3: noise; a frame that is entirely (0, 0); a frame that is entirely the pair (2, 3)."""
    rng = np.random.default_rng(3)
    a, b = _noise(rng, 3, 130, 200, 6), _noise(rng, 3, 130, 200, 4)
    a[1], b[1] = 0, 0
    a[2], b[2] = 2, 3
    return a, b, 6, 4


def _pair_all_cells():
    """70 x 70, Ka = Kb = 63: pixel n < 4096 holds the pair (n % 64, n // 64); the others are noise."""
    rng = np.random.default_rng(4)
    a, b = _noise(rng, 1, 70, 70, 63), _noise(rng, 1, 70, 70, 63)
    n = np.arange(4096)
    a.reshape(-1)[:4096], b.reshape(-1)[:4096] = n % 64, n // 64
    return a, b, 63, 63


def _pair_many_frames():
    rng = np.random.default_rng(5)
    return _noise(rng, 70, 5, 7, 3, above=2), _noise(rng, 70, 5, 7, 2), 3, 2


def _pair_narrow():
    rng = np.random.default_rng(6)
    return _noise(rng, 3, 37, 53, 1, above=2), _noise(rng, 3, 37, 53, 63, above=5), 1, 63


def _pair_narrow_t():
    a, b, Ka, Kb = _pair_narrow()
    return b, a, Kb, Ka


def _pair_two_frames():
    """Frame 0 is the pair (3, 1) throughout, frame 1 the pair (1, 2)."""
    a, b = np.zeros((2, 37, 53), np.uint16), np.zeros((2, 37, 53), np.uint16)
    a[0], b[0], a[1], b[1] = 3, 1, 1, 2
    return a, b, 3, 2


PAIR_CASES = {"5x7 T1": _pair_small, "37x53 T3 labels above K": _pair_medium, "130x200 T3 uniform frames": _pair_large,
              "70x70 K63 every cell": _pair_all_cells, "5x7 T70": _pair_many_frames, "Ka1 Kb63": _pair_narrow, "Ka63 Kb1": _pair_narrow_t,
              "two uniform frames": _pair_two_frames}


@functools.lru_cache(maxsize=None)
def pair_case(name):
    a, b, Ka, Kb = PAIR_CASES[name]()
    want = oracle.pair_counts(a, b, Ka, Kb)
    for arr in (a, b, want):
        arr.setflags(write=False)
    return a, b, Ka, Kb, want


# ------------------------------------------------------------------------------------------------ sequences for the evaluator
def rect_mask(h, w, box):
    m = np.zeros((h, w), np.uint8)
    if box is not None:
        y0, y1, x0, x1 = box                                                       # (ends exclusive)
        m[y0:y1, x0:x1] = 1
    return m


def records(spec, h, w):
    """spec: [(frame, track, class, box or None)] -> MOTS records; None is a zero-area mask."""
    return [(t, track, c, h, w, do.mask_string(rect_mask(h, w, box))) for t, track, c, box in spec]


IGN = (10000, 10)


def seq_a():
    """40 x 60, 6 frames; every count of both classes occurs.
    cars: gt 1001 drifts right, matched by result 1 (shifted one column: IoU < 1) in frames 0-2 and by result 2 in frames 3-5 (an ID
      switch); gt 1002 is matched exactly by result 3 in frame 0 and missed afterwards (FN); result 4 lies on nothing in frame 1 (FP);
      result 5 lies inside the ignore region in frame 2 (ignored).
    pedestrians: gt 2001 is matched by result 6 in frames 0-1, by nobody in frame 2, by result 7 from frame 3 (an ID switch across a
      gap); gt 2002 is never found (FN); result 8 lies on nothing in frame 0 (FP); result 9 lies inside the ignore region in frame 4.
    Also: a result of class 3 on top of gt 1001 (left out), a zero-area result and a zero-area ground-truth mask (dropped)."""
    h, w, T = 40, 60, 6
    gt, res = [], []
    for t in range(T):
        gt += [(t, 1001, 1, (2, 12, 2 + t, 14 + t)), (t, 1002, 1, (2, 10, 30, 41)), (t, 2001, 2, (20, 34, 5, 11)), (t, 2002, 2, (20, 31, 20, 25)),
               (t,) + IGN + ((30, 40, 40, 60),)]
        res.append((t, 1 if t < 3 else 2, 1, (2, 12, 3 + t, 15 + t)))
        if t != 2:
            res.append((t, 6 if t < 2 else 7, 2, (21, 34, 5, 11)))
    res += [(0, 3, 1, (2, 10, 30, 41)), (1, 4, 1, (14, 19, 45, 56)), (2, 5, 1, (31, 39, 42, 56)), (0, 8, 2, (14, 19, 30, 37)),
            (4, 9, 2, (32, 38, 45, 50)), (3, 10, 3, (2, 12, 5, 17)), (5, 11, 1, None)]
    gt.append((1, 1003, 1, None))
    return "0002", records(res, h, w), records(gt, h, w), T, h, w


def seq_b():
    """37 x 53, 5 frames: a car re-matched by the SAME result id after a gap (no switch); a result that covers its object by less than
    half (FP and FN); an ignore region that holds five sixths of an unmatched result."""
    h, w, T = 37, 53, 5
    gt, res = [], []
    for t in range(T):
        gt += [(t, 1001, 1, (5, 15, 5, 20)), (t, 2001, 2, (20, 30, 30, 36)), (t,) + IGN + ((0, 10, 40, 53),)]
        if t != 2:
            res.append((t, 1, 1, (5, 15, 6, 20)))
    res += [(1, 2, 2, (20, 30, 34, 44)), (3, 3, 2, (20, 30, 30, 36)), (4, 4, 1, (0, 6, 38, 50))]
    return "0006", records(res, h, w), records(gt, h, w), T, h, w


def seq_c():
    """24 x 31, 3 frames, pedestrians only (the cars' M is 0 here), no ignore region; frame 1 holds no result."""
    h, w, T = 24, 31, 3
    gt = [(t, 2001, 2, (3, 15, 4 + t, 9 + t)) for t in range(T)] + [(0, 2002, 2, (16, 23, 20, 30))]
    res = [(0, 1, 2, (3, 15, 4, 9)), (2, 1, 2, (3, 14, 6, 11)), (0, 2, 2, (17, 23, 20, 30))]
    return "0013", records(res, h, w), records(gt, h, w), T, h, w


def seq_long():
    """40 x 60, 11 frames, to be run with CHUNK_FRAMES = 4: both tracks are matched in frame 1 (first chunk), by nobody in frames 2-8
    (the whole second chunk), and by another result id in frames 9-10 (third chunk): the switches show only if the last-matched state
    crosses two chunk seams."""
    h, w, T = 40, 60, 11
    gt, res = [], []
    for t in range(T):
        gt += [(t, 1001, 1, (2, 12, 2, 14)), (t, 2001, 2, (20, 34, 5, 11)), (t,) + IGN + ((30, 40, 40, 60),)]
    res += [(1, 1, 1, (2, 12, 2, 13)), (1, 2, 2, (20, 34, 5, 11))]
    for t in (9, 10):
        res += [(t, 3, 1, (2, 12, 3, 14)), (t, 4, 2, (21, 34, 5, 11))]
    return "0007", records(res, h, w), records(gt, h, w), T, h, w


SEQUENCES = (seq_a, seq_b, seq_c)


@functools.lru_cache(maxsize=None)
def sequence(fn):
    """(name, result records, gt records, T, h, w, the oracle's counts, its notes)."""
    name, res, gt, T, h, w = fn()
    notes = []
    return name, res, gt, T, h, w, oracle.sequence_counts(res, gt, T, notes), notes


# ------------------------------------------------------------------------------------------------ files
def write_txt(path, recs):
    with open(path, "w") as fh:
        fh.writelines("%d %d %d %d %d %s\n" % r for r in recs)


def json_record(name, gt_records, T, h, w, image_paths=None):
    """The ground truth of one sequence as a video-dataset json record: instance id = track id, category = class, 10 -> 3."""
    cats = {}
    segs = [dict() for _ in range(T)]
    for t, track, c, _, _, s in gt_records:
        cats[str(track)] = 3 if c == 10 else c
        segs[t][str(track)] = s
    return {"id": name, "height": h, "width": w, "image_paths": image_paths or ["%s/%06d.png" % (name, t) for t in range(T)], "categories": cats,
            "segmentations": segs}


def write_json(path, recs):
    with open(path, "w") as fh:
        json.dump({"meta": {"category_labels": {"1": "car", "2": "pedestrian", "3": "ignore"}}, "sequences": recs}, fh)
    return path
