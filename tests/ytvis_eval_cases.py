"""The inputs of tests/test_gpu_ytvis_eval.py, built on the host.  tests/test_ytvis_eval_host.py checks on the oracle alone that each
case holds the situation it is named after, before anything goes to the device."""
import functools
import json
from collections import OrderedDict

import numpy as np

from tests import data_oracle as do
from tests import writer_oracle as wo
from tests import ytvis_eval_oracle as oracle

PAIR_SHAPES = [(7, 5), (37, 53), (130, 200)]
STATUS_CASES = ("empty", "bad_char_high", "open_group", "negative_count", "short_sum")          # one string per status 1, 2, 4, 8, 16


# ------------------------------------------------------------------------------------------------ rle_pair_inter
def column_major(h, w, lo, hi):
    """The pixels lo <= p < hi of the column-major order p = x * h + y."""
    flat = np.zeros(h * w, bool)
    flat[lo:hi] = True
    return np.ascontiguousarray(flat.reshape(w, h).T)


def checkerboard(h, w, bh, bw, y0=0, x0=0, phase=0):
    m = np.zeros((h, w), bool)
    yy, xx = np.mgrid[0:bh, 0:bw]
    m[y0:y0 + bh, x0:x0 + bw] = (yy + xx + phase) % 2 == 0
    return m


def blob(h, w, rng):
    y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
    m = np.zeros((h, w), bool)
    m[y0:y0 + 1 + int(rng.integers(0, max(1, h // 2))), x0:x0 + 1 + int(rng.integers(0, max(1, w // 2)))] = True
    m &= rng.random((h, w)) < 0.8                                                   # holes: many runs per column
    m[y0, x0] = True
    return m


@functools.lru_cache(maxsize=None)
def pair_case(h, w):
    """One call with every kind of string and pair -> dict(strings, pairs, index {name: string}, group {name: [pair indices]}, h, w,
    want = the oracle's (area, inter, status))."""
    rng = np.random.default_rng(100 * h + w)
    hw = h * w
    strings, index, pairs, group = [], OrderedDict(), [], OrderedDict()

    def add(name, mask=None, counts=None, string=None):
        index[name] = len(strings)
        strings.append(string if string is not None else wo.counts_to_string(counts if counts is not None else wo.encode(mask)))

    def pair(name, a, b):
        group.setdefault(name, []).append(len(pairs))
        pairs.append((index[a], index[b]))
    add("zeros", np.zeros((h, w), bool))
    add("ones", np.ones((h, w), bool))
    first0 = column_major(h, w, 0, 3) | column_major(h, w, hw // 2, hw // 2 + 4)
    add("first-count-0", first0)
    add("zero-length-zero-run", counts=[3, 2, 0, 4, hw - 9])                       # 1-runs [3, 5) and [5, 9): adjacent through a 0
    add("zero-length-one-run", counts=[3, 0, 2, 4, 0, 5, hw - 14])                 # 1-runs [3, 3), [5, 9) and, through a 0, [9, 14)
    for name, (y, x) in (("corner-tl", (0, 0)), ("corner-tr", (0, w - 1)), ("corner-bl", (h - 1, 0)), ("corner-br", (h - 1, w - 1))):
        m = np.zeros((h, w), bool)
        m[y, x] = True
        add(name, m)
    same = blob(h, w, rng)
    add("same-a", same)
    add("same-b", same.copy())
    cut = (w // 2) * h                                                              # a column boundary
    add("left", column_major(h, w, h // 2, cut - 1))
    add("right", column_major(h, w, cut + 1, hw - h // 2))
    add("touch-a", column_major(h, w, 2, cut + 1))                                  # ends with pixel `cut`
    add("touch-b", column_major(h, w, cut, hw - 1))                                 # begins with pixel `cut`
    bh, bw = min(64, h), min(64, w)
    add("board", checkerboard(h, w, bh, bw))
    add("board-shifted", checkerboard(h, w, bh, bw, phase=1))
    add("long-run", column_major(h, w, 1, bw * h - 1))                              # one run over every column the board touches
    # the long run AND a larger checkerboard to its right: more characters than "board", so whichever string a kernel strides over, one
    # thread owns a run that spans every run of the board
    rest = w - bw - 1
    heavy = column_major(h, w, 0, bw * h)
    if rest > 0:
        heavy |= checkerboard(h, w, h, rest, 0, bw + 1)
    add("long-run-and-more", heavy)
    cols = np.zeros((h, w), bool)
    cols[:, ::2] = True
    rows = np.zeros((h, w), bool)
    rows[::3] = True
    add("column-stripes", cols)
    add("row-stripes", rows)
    for k in range(3):
        add("blob-%d" % k, blob(h, w, rng))
    bad = {name: s for name, s, _ in do.malformed_cases(h, w)}
    for name in STATUS_CASES:
        add("refused-" + name, string=bad[name])

    good = [n for n in index if not n.startswith("refused-")]
    for n in good:
        pair("self", n, n)                                                          # a pair naming one string twice: inter = area
    for a, b in (("zeros", "ones"), ("ones", "ones"), ("ones", "blob-0"), ("zeros", "blob-0"), ("first-count-0", "ones"),
                 ("first-count-0", "blob-1"), ("zero-length-zero-run", "zero-length-one-run"), ("zero-length-one-run", "zero-length-zero-run"),
                 ("zero-length-zero-run", "ones"), ("zero-length-one-run", "first-count-0"), ("zero-length-one-run", "board")):
        pair("degenerate", a, b)
    for c in ("corner-tl", "corner-tr", "corner-bl", "corner-br"):
        for other in ("ones", "board", "long-run", "first-count-0", "corner-tl", "corner-br"):
            pair("corners", c, other)
            pair("corners", other, c)
    pair("identical", "same-a", "same-b")
    pair("identical", "same-b", "same-a")
    pair("disjoint-extents", "left", "right")
    pair("disjoint-extents", "right", "left")
    pair("touching-extents", "touch-a", "touch-b")
    pair("touching-extents", "touch-b", "touch-a")
    pair("long-vs-board", "long-run", "board")
    pair("long-vs-board", "board", "long-run")
    pair("long-vs-board", "long-run-and-more", "board")
    pair("long-vs-board", "board", "long-run-and-more")
    pair("long-vs-board", "long-run-and-more", "board-shifted")
    pair("board-vs-shifted", "board", "board-shifted")
    pair("board-vs-shifted", "board-shifted", "board")
    pair("stripes", "column-stripes", "row-stripes")
    pair("stripes", "row-stripes", "column-stripes")
    pair("stripes", "column-stripes", "board")
    for a in ("blob-0", "blob-1", "blob-2"):
        for b in ("blob-0", "blob-1", "blob-2", "same-a", "board", "column-stripes", "row-stripes", "long-run", "touch-a"):
            pair("blobs", a, b)
    for name in STATUS_CASES:
        r = "refused-" + name
        pair("refused", r, "ones")
        pair("refused", "blob-0", r)
        pair("refused", r, r)
    pair("refused", "refused-empty", "refused-short_sum")
    for _ in range(3):
        pair("repeated", "blob-0", "blob-1")
        pair("repeated", "same-a", "same-b")
    want = oracle.pair_tables(strings, pairs, h, w)
    for arr in want:
        arr.setflags(write=False)
    return dict(strings=strings, pairs=pairs, index=index, group=group, h=h, w=w, want=want)


@functools.lru_cache(maxsize=None)
def many_pairs_case():
    """70 000 pairs over six short strings of 7 x 5, one of them refused: more pairs than one grid dimension holds."""
    h, w = 7, 5
    rng = np.random.default_rng(7)
    strings = [oracle.mask_string(blob(h, w, rng)) for _ in range(4)] + [oracle.mask_string(np.ones((h, w), bool)), ""]
    every = [(a, b) for a in range(6) for b in range(6)]
    area, table, status = oracle.pair_tables(strings, every, h, w)
    pairs = rng.integers(0, 6, (70000, 2))
    inter = table.reshape(6, 6)[pairs[:, 0], pairs[:, 1]]
    return dict(strings=strings, pairs=[tuple(p) for p in pairs.tolist()], h=h, w=w, want=(area, inter, status))


@functools.lru_cache(maxsize=None)
def many_strings_case():
    """4097 strings of 8 x 8 and 8193 pairs: one string more than the area kernel has workgroups and one pair more than the pair kernel
    has, so both take a second trip through their workgroup loops; (0, 4096) and (4096, 4096) name the string of that second trip.
    Blobs, all ones, a refused string now and then; pairs repeat."""
    h, w, M, K = 8, 8, 4097, 8193
    rng = np.random.default_rng(11)
    strings = ["5" if m % 97 == 50 else oracle.mask_string(np.ones((h, w), bool) if m % 41 == 7 else blob(h, w, rng))
               for m in range(M)]                                          # "5": one count of 5, not 64 -- refused for its sum
    for m, box in ((0, (0, 6, 0, 8)), (3, (4, 8, 0, 8)), (M - 1, (0, 8, 2, 7))):          # areas 48, 32, 40; they meet in 30 (0, last), 20 (last, 3)
        strings[m] = oracle.mask_string(rect(h, w, box))
    pairs = rng.integers(0, M, (K, 2))
    pairs[0], pairs[1], pairs[K - 1] = (0, M - 1), (M - 1, M - 1), (M - 1, 3)
    pairs = [tuple(p) for p in pairs.tolist()]
    return dict(strings=strings, pairs=pairs, h=h, w=w, want=oracle.pair_tables(strings, pairs, h, w))


# ------------------------------------------------------------------------------------------------ videos for the evaluator
def rect(h, w, box):
    m = np.zeros((h, w), bool)
    y0, y1, x0, x1 = box                                                            # (ends exclusive)
    m[y0:y1, x0:x1] = True
    return m


def track(h, w, category, boxes, score=None, iscrowd=None, video=None):
    """boxes: per frame a box, a list of boxes (their union) or None (no mask in that frame)."""
    segs = []
    for b in boxes:
        if b is None:
            segs.append(None)
            continue
        m = np.zeros((h, w), bool)
        for box in (b if isinstance(b, list) else [b]):
            m |= rect(h, w, box)
        segs.append({"size": [h, w], "counts": oracle.mask_string(m)})
    out = {"category_id": category, "segmentations": segs}
    if score is not None:
        out["score"], out["video_id"] = score, video
    if iscrowd is not None:
        out["iscrowd"] = iscrowd
    return out


def shifted(box, t, dy=0, dx=1):
    return (box[0] + dy * t, box[1] + dy * t, box[2] + dx * t, box[3] + dx * t)


def video_main():
    """24 x 40, 4 frames, categories 1, 2 and (results only) 3.
    ground truth: g0 and g1 of category 1 overlap each other; g2 of category 2 has no mask in frame 1; g3 is a crowd of category 1;
      g4 of category 1 is small and is found only by the LAST of the twelve results of category 1.
    results of category 1, by score: r0 on g0 (a column off: IoU 9 / 11), r1 and r2 with EQUAL scores, r1 on g1 and r2 a second, looser hit on
      g0 (an FP at every threshold: g0 is taken), r3 inside the crowd (ignored), r4 .. r10 on nothing or on too little (FPs), two of
      them with equal scores, r11 on g4 exactly.  So one true positive at maxDet 1, two at 10, three at 100.
    results of category 2: r12 on g2 with no mask in frame 2; r13 overlapping r12 and g2 loosely.  Category 3: r14, no ground truth."""
    h, w, T = 24, 40, 4
    v = "main"
    g0, g1, g2, g4 = (2, 10, 2, 12), (6, 14, 8, 18), (14, 22, 20, 28), (17, 23, 2, 7)
    crowd = (0, 12, 30, 40)
    gt = [track(h, w, 1, [shifted(g0, t) for t in range(T)]),
          track(h, w, 1, [shifted(g1, t) for t in range(T)], iscrowd=0),
          track(h, w, 2, [g2, None, g2, shifted(g2, 1)]),
          track(h, w, 1, [crowd] * T, iscrowd=1),
          track(h, w, 1, [g4] * T)]
    res = [track(h, w, 1, [shifted(g0, t + 1) for t in range(T)], 0.95, video=v),                                   # r0: 8 x 9 of 8 x 11
           track(h, w, 1, [shifted((7, 14, 8, 18), t) for t in range(T)], 0.90, video=v),                           # r1: 7 of g1's 8 rows
           track(h, w, 1, [shifted((3, 10, 2, 12), t) for t in range(T)], 0.90, video=v),                           # r2: 7 of g0's 8 rows
           track(h, w, 1, [(2, 8, 32, 38)] * T, 0.85, video=v),                                                     # r3: inside the crowd
           track(h, w, 1, [(15, 20, 12, 18)] * T, 0.80, video=v),                                                   # r4: on nothing
           track(h, w, 1, [shifted((2, 5, 2, 5), t) for t in range(T)], 0.70, video=v),                             # r5: a corner of g0
           track(h, w, 1, [(20, 24, 30, 36), None, None, (20, 24, 30, 36)], 0.70, video=v),                         # r6: on nothing, two frames
           track(h, w, 1, [(12, 16, 20, 24)] * T, 0.60, video=v),
           track(h, w, 1, [(0, 2, 14, 28)] * T, 0.50, video=v),
           track(h, w, 1, [[(17, 19, 2, 4), (21, 23, 10, 14)]] * T, 0.40, video=v),                                 # r9: 4 pixels of g4 and more
           track(h, w, 1, [(14, 16, 30, 40)] * T, 0.30, video=v),
           track(h, w, 1, [g4] * T, 0.20, video=v),                                                                 # r11: g4 itself
           track(h, w, 2, [g2, None, None, shifted(g2, 1)], 0.75, video=v),                                         # r12
           track(h, w, 2, [shifted(g2, 3, 1, 1)] * T, 0.65, video=v),                                               # r13
           track(h, w, 3, [(0, 5, 0, 5)] * T, 0.99, video=v)]                                                       # r14
    return v, res, gt, (h, w)


def video_results_only():
    h, w = 24, 40
    return "results-only", [track(h, w, 1, [(3, 9, 3, 9)] * 4, 0.97, video="results-only")], [], (h, w)


def video_gt_only():
    h, w = 24, 40
    return "gt-only", [], [track(h, w, 2, [(3, 9, 3, 9)] * 4), track(h, w, 1, [(10, 20, 10, 20)] * 4)], (h, w)


def video_other_size():
    """37 x 53, 3 frames: both categories, a perfect track, one that loses its object half way, and a score equal to one of ``main``."""
    h, w, T = 37, 53, 3
    v = "other-size"
    a, b = (5, 20, 5, 25), (20, 33, 30, 50)
    gt = [track(h, w, 1, [shifted(a, t, 1, 2) for t in range(T)]), track(h, w, 2, [b] * T)]
    res = [track(h, w, 1, [shifted(a, t, 1, 2) for t in range(T)], 0.90, video=v),
           track(h, w, 2, [b, b, None], 0.75, video=v),
           track(h, w, 2, [(0, 4, 0, 50)] * T, 0.10, video=v)]
    return v, res, gt, (h, w)


VIDEOS = (video_main, video_results_only, video_gt_only, video_other_size)


@functools.lru_cache(maxsize=None)
def video(fn):
    """(id, results, ground truth, size, the oracle's records, its notes)."""
    vid, res, gt, size = fn()
    notes = []
    return vid, res, gt, size, oracle.video_records(res, gt, size, notes), notes


def oracle_summary(fns=VIDEOS):
    return oracle.summary(OrderedDict((video(fn)[0], video(fn)[4]) for fn in fns))


# ------------------------------------------------------------------------------------------------ files
def json_record(name, gt_tracks, size, ids=None, image_paths=None):
    """Ground-truth tracks as one sequence of a video-dataset json: instance ids ``ids`` (default 1 ..), in ascending order of which the
    reader returns the tracks."""
    T = len(gt_tracks[0]["segmentations"])
    ids = ids or list(range(1, len(gt_tracks) + 1))
    segs = [dict() for _ in range(T)]
    for iid, tr in zip(ids, gt_tracks):
        for t, seg in enumerate(tr["segmentations"]):
            if seg is not None:
                segs[t][str(iid)] = seg["counts"]
    return {"id": name, "height": size[0], "width": size[1], "image_paths": image_paths or ["%s/%05d.jpg" % (name, t) for t in range(T)],
            "categories": {str(iid): tr["category_id"] for iid, tr in zip(ids, gt_tracks)}, "segmentations": segs}


def write_json(path, recs):
    with open(path, "w") as fh:
        json.dump({"meta": {"category_labels": {"1": "person", "2": "dog", "3": "cat"}}, "sequences": recs}, fh)
    return path
