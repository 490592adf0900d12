"""The inputs of tests/test_gpu_davis_eval.py, generated from seeds on the host.  tests/test_davis_eval_host.py checks on the oracle
alone that each case holds the situation it is named after, before anything goes to the device."""
import functools

import numpy as np

from tests import davis_eval_oracle as oracle


def scene(T, H, W, Kp, Kg, seed, dtype=np.uint8):
    """Rectangles and ellipses drifting over T frames: an index map with labels 1 .. Kp (later shapes cover earlier ones) and Kg planes,
    the first min(Kp, Kg) of them shifted copies of proposals (so that boundaries match within a few pixels), the others free."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]

    def shape(cy, cx, ry, rx, ellipse):
        if ellipse:
            return ((yy - cy) / max(ry, 0.6)) ** 2 + ((xx - cx) / max(rx, 0.6)) ** 2 <= 1.0
        return (abs(yy - cy) <= ry) & (abs(xx - cx) <= rx)
    recipes = [(rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1, H / 5), rng.uniform(1, W / 5), bool(rng.integers(2)), rng.uniform(-2, 2, 2))
               for _ in range(max(Kp, Kg))]
    shift = rng.integers(-3, 4, (Kg, 2))
    pred, gt = np.zeros((T, H, W), dtype), np.zeros((Kg, T, H, W), np.uint8)
    for t in range(T):
        for k, (cy, cx, ry, rx, ell, v) in enumerate(recipes):
            if k < Kp:
                pred[t][shape(cy + v[0] * t, cx + v[1] * t, ry, rx, ell)] = k + 1
            if k < Kg:
                gt[k, t] = shape(cy + v[0] * t + shift[k, 0], cx + v[1] * t + shift[k, 1], ry + (k % 2), rx, ell)
    return pred, gt


# name -> (T, H, W, Kp, Kg, r, dtype, seed): both sizes, both T, every radius, every Kp and Kg of the list, both map types
GRID = {
    "37x53 T3 r1 Kp1 Kg1 u8": (3, 37, 53, 1, 1, 1, np.uint8, 1),
    "37x53 T5 r2 Kp20 Kg10 u16": (5, 37, 53, 20, 10, 2, np.uint16, 2),
    "45x70 T3 r8 Kp64 Kg32 u8": (3, 45, 70, 64, 32, 8, np.uint8, 3),
    "37x53 T3 r19 Kp64 Kg1 u16": (3, 37, 53, 64, 1, 19, np.uint16, 4),
    "45x70 T5 r8 Kp1 Kg32 u16": (5, 45, 70, 1, 32, 8, np.uint16, 5),
    "45x70 T3 r19 Kp20 Kg10 u8": (3, 45, 70, 20, 10, 19, np.uint8, 6),
    "45x70 T5 r1 Kp64 Kg10 u8": (5, 45, 70, 64, 10, 1, np.uint8, 7),
    "37x53 T5 r2 Kp20 Kg32 u8": (5, 37, 53, 20, 32, 2, np.uint8, 8),
}


def rect(a, y0, y1, x0, x1, v=1):
    a[y0:y1 + 1, x0:x1 + 1] = v          # (both ends inclusive)


def edges_case():
    """37 x 53, r = 2: proposals and objects on all four edges and in all four corners."""
    T, H, W = 3, 37, 53
    pred, gt = np.zeros((T, H, W), np.uint8), np.zeros((4, T, H, W), np.uint8)
    for t in range(T):
        rect(pred[t], 0, 3, 0, 4, 1); rect(pred[t], 0, 2, W - 6, W - 1, 2); rect(pred[t], H - 4, H - 1, 0, 5, 3); rect(pred[t], H - 3, H - 1, W - 4, W - 1, 4)
        rect(pred[t], 0, 1, 20, 30, 5); rect(pred[t], H - 2, H - 1, 18, 28, 6); rect(pred[t], 12, 22, 0, 1, 7); rect(pred[t], 14, 24, W - 2, W - 1, 8)
        rect(gt[0, t], 0, 4, 0, 3); rect(gt[0, t], H - 5, H - 1, W - 5, W - 1)          # two corners in one plane
        rect(gt[1, t], 0, 3, W - 5, W - 1); rect(gt[1, t], H - 3, H - 1, 0, 6)
        rect(gt[2, t], 0, 2, 19, 31); rect(gt[2, t], H - 1, H - 1, 17, 29)             # top and bottom edges
        rect(gt[3, t], 11, 23, 0, 0); rect(gt[3, t], 13, 25, W - 3, W - 1)             # left and right edges
    return pred, gt, 8, 2


def special_case():
    """45 x 70, T = 4, Kp = 4, Kg = 3, r = 2: label 3 never occurs; plane 2 is empty; frame 2 holds nothing at all; planes 0 and 1
    overlap; labels 5 and 200 (above Kp) are background."""
    T, H, W = 4, 45, 70
    pred, gt = np.zeros((T, H, W), np.uint8), np.zeros((3, T, H, W), np.uint8)
    for t in (0, 1, 3):
        rect(pred[t], 5 + t, 15 + t, 6, 20, 1); rect(pred[t], 20, 30, 30 + t, 44, 2); rect(pred[t], 32, 40, 50, 60, 4)
        rect(pred[t], 4, 9, 50, 60, 5); rect(pred[t], 36, 42, 5, 15, 200)
        rect(gt[0, t], 6 + t, 16 + t, 5, 21); rect(gt[1, t], 12 + t, 28, 15, 40)          # plane 1 overlaps plane 0
    return pred, gt, 4, 2


def exact_radius_case():
    """45 x 70, r = 8: the object's right boundary column is 20, the proposal's left boundary column 28 -- at the same rows the nearest
    boundary pixels are exactly 8 apart, and no pair is nearer."""
    T, H, W = 3, 45, 70
    pred, gt = np.zeros((T, H, W), np.uint8), np.zeros((1, T, H, W), np.uint8)
    for t in range(T):
        rect(gt[0, t], 10, 20, 10, 20); rect(pred[t], 10, 20, 29, 40, 1)
    return pred, gt, 1, 8


def seam_case():
    """130 x 200, r = 8 (tiles of 32: seams at 32, 64, ... in x and y): the proposal's boundary lies left of / above a seam, the
    object's within r on the other side, and the other way round at the next seam."""
    T, H, W = 3, 130, 200
    pred, gt = np.zeros((T, H, W), np.uint8), np.zeros((2, T, H, W), np.uint8)
    for t in range(T):
        rect(pred[t], 10, 29, 10, 29, 1); rect(gt[0, t], 12, 35, 12, 36)          # p's right / bottom boundary at 29 < 32, g's at 36 / 35 > 32
        rect(pred[t], 40, 69, 70, 100, 2); rect(gt[1, t], 38, 60, 60, 94)         # around x = 64 / 96 and y = 64
        rect(pred[t], 100, 129, 150, 199, 3)                                       # bottom-right corner, several tiles from the origin
    return pred, gt, 3, 8


def frame_leak_case():
    """37 x 53, r = 8: a proposal on the bottom rows of frame 0 and an object on the top rows of frame 1 (adjacent in memory), and the
    mirror image between frames 1 and 2: alone, no frame has a match."""
    T, H, W = 3, 37, 53
    pred, gt = np.zeros((T, H, W), np.uint8), np.zeros((1, T, H, W), np.uint8)
    rect(pred[0], H - 4, H - 1, 10, 30, 1); rect(gt[0, 1], 0, 3, 10, 30)
    rect(gt[0, 1], H - 3, H - 1, 5, 25); rect(pred[2], 0, 2, 5, 25, 1)
    return pred, gt, 1, 8


SPECIAL = {"edges and corners": edges_case, "special": special_case, "exactly r": exact_radius_case, "tile seams": seam_case,
           "frame leak": frame_leak_case}
CASE_NAMES = list(GRID) + list(SPECIAL)


@functools.lru_cache(maxsize=None)
def case(name):
    """(pred, gt, Kp, r, the oracle's tables): computed once, shared, never written to."""
    if name in GRID:
        T, H, W, Kp, Kg, r, dtype, seed = GRID[name]
        pred, gt = scene(T, H, W, Kp, Kg, seed, dtype)
    else:
        pred, gt, Kp, r = SPECIAL[name]()
    tab = oracle.counts(pred, gt, Kp, r)
    for a in (pred, gt) + tuple(tab.values()):
        a.setflags(write=False)
    return pred, gt, Kp, r, tab


def evaluator_sequences():
    """Two small sequences for the evaluator: (name, pred, gt, Kp); more proposals than objects in the first, fewer in the second."""
    a_pred, a_gt = scene(6, 37, 53, 4, 2, 21)
    b_pred, b_gt = scene(7, 45, 70, 2, 3, 22, np.uint16)
    return [("more-proposals", a_pred, a_gt, 4), ("fewer-proposals", b_pred, b_gt, 2)]
