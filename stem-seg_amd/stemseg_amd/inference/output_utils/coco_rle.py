"""Host-side reading of COCO RLE strings for the KITTI-MOTS filters (kitti_mots_postprocessing.py:38-52 reads area and bbox
through pycocotools; pycocotools is not a dependency here).  numpy only; the strings themselves are produced on the device
(``hip.rle_encode``).  Semantics of pycocotools 2.0 ``maskApi.c``: rleFrString, rleArea, rleToBbox."""
import numpy as np


def string_to_counts(s):
    """rleFrString: characters - 48 in 5-bit groups, LSB first, 0x20 = more, sign from bit 0x10 of the last group; counts
    from index 3 on are deltas against the count two places earlier."""
    counts = []
    p, n = 0, len(s)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return np.asarray(counts, dtype=np.int64)


def area(counts):
    """rleArea: the sum of the odd-indexed (foreground) runs."""
    return int(np.asarray(counts)[1::2].sum())


def to_bbox(counts, h):
    """rleToBbox: [x, y, w, h]; an even number of counts is used, an empty list gives zeros, and a foreground run that crosses
    a column boundary makes the box span the full height."""
    c = np.asarray(counts, dtype=np.int64)
    m = (len(c) // 2) * 2
    if m == 0:
        return [0, 0, 0, 0]
    ends = np.cumsum(c[:m])
    starts, lasts = ends[0::2], ends[1::2] - 1                # first / last pixel of every foreground run
    xs0, ys0, xs1, ys1 = starts // h, starts % h, lasts // h, lasts % h
    x_min, x_max = int(min(xs0.min(), xs1.min())), int(max(xs0.max(), xs1.max()))
    if (xs0 < xs1).any():
        y_min, y_max = 0, h - 1
    else:
        y_min, y_max = int(min(ys0.min(), ys1.min())), int(max(ys0.max(), ys1.max()))
    return [x_min, y_min, x_max - x_min + 1, y_max - y_min + 1]
