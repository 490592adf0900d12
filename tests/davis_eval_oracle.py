"""The DAVIS J and F measures of include/stemseg_hip.h (csrc/davis_eval.hip, stemseg_amd/evaluation/davis.py) restated in plain numpy and
Python loops: boundary maps by the clamped 2 x 2 rule, a brute-force dilation with an explicit disk array, integer counts, then J, F and
the sequence statistics in fp64.  It follows the published DAVIS 2017 "unsupervised" protocol; agreement with the official toolkit's
numbers is unverified.  Counts are compared with integer equality; J, F and the statistics with ``==``: both sides divide the same
integers in the same order and average with ``numpy.mean`` over one contiguous fp64 vector."""
import itertools
import math

import numpy as np

TABLES = ("inter", "m_p", "m_g", "area_p", "n_p", "area_g", "n_g")
STATS = ("J-Mean", "J-Recall", "J-Decay", "F-Mean", "F-Recall", "F-Decay")


def radius(H, W):
    return int(math.ceil(0.008 * math.sqrt(float(H) * float(H) + float(W) * float(W))))


def disk(r):
    """bool [2r + 1, 2r + 1]: entry (dy + r, dx + r) is dx^2 + dy^2 <= r^2."""
    d = np.zeros((2 * r + 1, 2 * r + 1), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            d[dy + r, dx + r] = dx * dx + dy * dy <= r * r
    return d


def boundary(m):
    """bool [H, W]: m[y, x] differs from m at (y, x + 1), (y + 1, x) or (y + 1, x + 1), neighbour coordinates clamped to the image."""
    m = np.asarray(m) != 0
    H, W = m.shape
    ys, xs = np.minimum(np.arange(H) + 1, H - 1), np.minimum(np.arange(W) + 1, W - 1)
    e, s, se = m[:, xs], m[ys, :], m[ys][:, xs]
    return (m != e) | (m != s) | (m != se)


def dilate(b, r):
    """The OR of the disk stamped on every set pixel of ``b``; what leaves the image is dropped."""
    H, W = b.shape
    d = disk(r)
    out = np.zeros((H, W), bool)
    for y, x in zip(*np.nonzero(b)):
        ya, yb, xa, xb = max(0, y - r), min(H, y + r + 1), max(0, x - r), min(W, x + r + 1)
        out[ya:yb, xa:xb] |= d[ya - y + r:yb - y + r, xa - x + r:xb - x + r]
    return out


def counts(pred, gt, Kp, r):
    """pred: integer index map [T, H, W] (labels 1 .. Kp are the proposals), gt [Kg, T, H, W] (non-zero = member) -> the seven int64
    tables of ``TABLES`` as a dict."""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt) != 0
    Kg, T = gt.shape[0], gt.shape[1]
    out = {"inter": np.zeros((T, Kp, Kg), np.int64), "m_p": np.zeros((T, Kp, Kg), np.int64), "m_g": np.zeros((T, Kp, Kg), np.int64),
           "area_p": np.zeros((T, Kp), np.int64), "n_p": np.zeros((T, Kp), np.int64), "area_g": np.zeros((T, Kg), np.int64),
           "n_g": np.zeros((T, Kg), np.int64)}
    for t in range(T):
        bg = [boundary(gt[g, t]) for g in range(Kg)]
        near_g = [dilate(b, r) for b in bg]
        for g in range(Kg):
            out["area_g"][t, g], out["n_g"][t, g] = gt[g, t].sum(), bg[g].sum()
        for p in range(Kp):
            m = pred[t] == p + 1
            out["area_p"][t, p] = m.sum()
            if not m.any():
                continue          # (an empty mask has no boundary: every pair count of the proposal stays 0)
            bp = boundary(m)
            near_p = dilate(bp, r)
            out["n_p"][t, p] = bp.sum()
            for g in range(Kg):
                out["inter"][t, p, g] = (m & gt[g, t]).sum()
                out["m_p"][t, p, g] = (bp & near_g[g]).sum()
                out["m_g"][t, p, g] = (bg[g] & near_p).sum()
    return out


def jaccard(inter, area_p, area_g):
    union = int(area_p) + int(area_g) - int(inter)
    return 1.0 if union == 0 else float(int(inter)) / float(union)


def precision_recall(n_p, n_g, m_p, m_g):
    n_p, n_g = int(n_p), int(n_g)
    if n_p > 0 and n_g > 0:
        return float(int(m_p)) / float(n_p), float(int(m_g)) / float(n_g)
    if n_p == 0 and n_g > 0:
        return 1.0, 0.0
    if n_g == 0 and n_p > 0:
        return 0.0, 1.0
    return 1.0, 1.0


def f_from_pr(P, R):
    return 0.0 if P + R == 0 else 2.0 * P * R / (P + R)


def f_measure(n_p, n_g, m_p, m_g):
    return f_from_pr(*precision_recall(n_p, n_g, m_p, m_g))


def mean(values):
    return float(np.mean(np.ascontiguousarray(values, dtype=np.float64)))


def decay_bins(n):
    """The four [first, last] index ranges (inclusive) over n counted frames."""
    ids = np.round(np.linspace(1, n, 5) + 1e-10) - 1
    ids = [int(v) for v in ids]
    return [(ids[i], ids[i + 1]) for i in range(4)]


def frame_stats(values):
    """(mean, recall, decay) of the per-frame values of one object over the counted frames."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    bins = decay_bins(len(v))
    first, last = v[bins[0][0]:bins[0][1] + 1], v[bins[3][0]:bins[3][1] + 1]
    return mean(v), mean([1.0 if x > 0.5 else 0.0 for x in v]), mean(first) - mean(last)


def counted_frames(T):
    if T < 3:
        raise ValueError("a sequence of %d frames: the first and the last frame are left out, so at least 3 are needed" % T)
    return list(range(1, T - 1))


def assign(score, Kg):
    """perm[g] = the row (proposal, or a padded row) given to object g so that the sum of score[perm[g], g] is largest, no row used
    twice.  Brute force over every choice of Kg distinct rows -- the padded columns score 0 whatever they get -- for the small cases
    of the tests."""
    n = score.shape[0]
    assert score.shape == (n, n) and math.factorial(n) // math.factorial(n - Kg) <= 100000, "the oracle's brute-force assignment is for small cases"
    best, best_total = None, None
    for perm in itertools.permutations(range(n), Kg):
        total = sum(score[perm[g], g] for g in range(Kg))
        if best_total is None or total > best_total:
            best, best_total = perm, total
    return list(best)


def sequence_stats(tab, Kp, Kg):
    """From the tables of one sequence -> {"J": [Kg][frames], "F": ..., "assignment": [Kg] (proposal index or -1), and per object the six
    statistics}."""
    T = tab["area_g"].shape[0]
    frames = counted_frames(T)
    J = np.zeros((len(frames), Kp, Kg))
    F = np.zeros((len(frames), Kp, Kg))
    for k, t in enumerate(frames):
        for p in range(Kp):
            for g in range(Kg):
                J[k, p, g] = jaccard(tab["inter"][t, p, g], tab["area_p"][t, p], tab["area_g"][t, g])
                F[k, p, g] = f_measure(tab["n_p"][t, p], tab["n_g"][t, g], tab["m_p"][t, p, g], tab["m_g"][t, p, g])
    n = max(Kp, Kg)
    score = np.zeros((n, n))
    for p in range(Kp):
        for g in range(Kg):
            score[p, g] = mean([(J[k, p, g] + F[k, p, g]) / 2.0 for k in range(len(frames))])
    perm = assign(score, Kg)
    out = {"assignment": [], "J": [], "F": [], "objects": []}
    for g in range(Kg):
        p = perm[g] if perm[g] < Kp else -1
        j = [J[k, p, g] if p >= 0 else 0.0 for k in range(len(frames))]
        f = [F[k, p, g] if p >= 0 else 0.0 for k in range(len(frames))]
        out["assignment"].append(p)
        out["J"].append(j)
        out["F"].append(f)
        out["objects"].append(dict(zip(STATS, frame_stats(j) + frame_stats(f))))
    return out


def summary(per_sequence):
    """per_sequence: {name: sequence_stats(...)} -> the dataset figures: means over all objects of all sequences."""
    objs = [o for s in per_sequence.values() for o in s["objects"]]
    out = {k: mean([o[k] for o in objs]) for k in STATS}
    out["J&F-Mean"] = (out["J-Mean"] + out["F-Mean"]) / 2.0
    return out
