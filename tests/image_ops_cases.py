"""The inputs of tests/test_image_ops_host.py and tests/test_gpu_image_ops.py, generated deterministically (numpy's legacy
RandomState streams do not change between versions).

Frames are uniform uint8 noise: adjacent pixels differ by ~85 on average, so a tap off by one, or a weight wrong in its third
digit, is a thousand times any bound the tests use (the smooth synthetic frames of the older tests hide both).  The shapes are the
smallest at which each path of csrc/image_ops.hip is taken: up- and down-scaling, the identity, in_size == 1 on either axis, pad equal
to and larger than the size, mask_scale 1, 2 and 4, a crop inside the up-sampled map, and one case per kernel whose element count
exceeds the launch cap, so that the grid-stride loop runs (the caps are stated in tests/test_image_ops_host.py and checked there against
the launch code)."""
import functools

import numpy as np

# ------------------------------------------------------------------------------------------------ pre-processing
# (name, (H0, W0), (new_h, new_w), (pad_h, pad_w), T)
PRE_CASES = (
    ("up", (50, 70), (64, 90), (64, 96), 2),
    ("odd", (37, 53), (45, 64), (64, 64), 3),
    ("down", (96, 64), (32, 32), (32, 32), 2),
    ("identity", (33, 47), (33, 47), (64, 64), 1),
    ("one_row", (1, 5), (7, 3), (32, 32), 2),
    ("one_column", (6, 1), (4, 9), (32, 32), 2),
    ("two_by_two", (2, 2), (63, 65), (64, 96), 1),
    ("stride", (30, 32), (480, 500), (480, 512), 9),          # 9 * 480 * 512 = 2,211,840 outputs
)
MASKED_CASES = PRE_CASES[:3]
CAFFE_MEAN, IMAGENET_MEAN, IMAGENET_STD = (102.9801, 115.9465, 122.7717), (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (name, mean, std, unit_scale, flip); in the third every slot is distinct, so a channel / flip mix-up shows
PARAM_SETS = (
    ("caffe", CAFFE_MEAN, (1.0, 1.0, 1.0), False, False),
    ("imagenet_flip", IMAGENET_MEAN, IMAGENET_STD, True, True),
    ("caffe_std_flip", CAFFE_MEAN, (57.375, 57.12, 58.395), False, True),
)
INVALID_PATTERNS = ("none", "all", "checkerboard", "one_pixel", "random30")


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def frames(name):
    i, (_, (H0, W0), _, _, T) = next((i, c) for i, c in enumerate(PRE_CASES) if c[0] == name)
    return _frozen(np.random.RandomState(1000 + i).randint(0, 256, (T, H0, W0, 3)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def invalid(name, pattern):
    """uint8 [T,H0,W0]; non-zero = invalid (any non-zero value counts: the patterns use 1, 255 and 7)."""
    T, H0, W0 = frames(name).shape[:3]
    yy, xx = np.mgrid[0:H0, 0:W0]
    inv = np.zeros((T, H0, W0), np.uint8)
    if pattern == "all":
        inv[:] = 255
    elif pattern == "checkerboard":
        inv[:] = ((yy + xx) % 2).astype(np.uint8)
        inv[1:] = 1 - inv[1:]
    elif pattern == "one_pixel":
        inv[T - 1, H0 // 3 - 1, W0 // 2] = 7           # (a pixel that every case taps with a non-zero weight)
    elif pattern == "random30":
        inv[:] = (np.random.RandomState(77).rand(T, H0, W0) < 0.3) * 255
    else:
        assert pattern == "none"
    return _frozen(inv)


# ------------------------------------------------------------------------------------------------ mask resampling
# (name, (h, w), mask_scale, (crop_h, crop_w), (out_h, out_w))
MASK_CASES = (
    ("same", (30, 54), 4.0, (120, 216), (120, 216)),
    ("crop_up", (30, 54), 4.0, (113, 200), (180, 320)),
    ("down", (24, 32), 4.0, (90, 120), (45, 61)),
    ("scale1", (24, 30), 1.0, (24, 30), (90, 120)),
    ("scale2", (12, 16), 2.0, (23, 30), (50, 70)),
    ("one_row", (1, 7), 4.0, (4, 28), (3, 50)),
    ("one_column", (9, 1), 4.0, (33, 4), (70, 5)),
    ("half", (16, 28), 0.5, (8, 14), (13, 23)),               # mask_scale < 1: the only way to 16 DISTINCT source pixels (see LAYOUTS)
    ("stride", (8, 8), 4.0, (32, 32), (1025, 1024)),          # 1,049,600 outputs
)
# "all_different": 1 + 7 (y w + x) mod 23, so no two of the 16 source slots under an output pixel need agree.  With mask_scale >= 1 the
# two up-sampled rows a pixel reads are neighbours and share a source row, so the 16 slots hold at most 3 x 3 = 9 distinct pixels (the
# dedup has 7 duplicates to skip); at mask_scale 0.5 all 16 differ.
LAYOUTS = ("rectangles", "all_different", "stripes")
WIDE_INDICES = (1, 255, 256, 32767, 32768, 65535)
NARROW_RECT = (1, 2, 3, 100, 127, 128, 254, 255)              # the 8 rectangles' indices at width 1
# every (case, layout, index width): all cases at width 1, the first three again at width 2.  "half" runs the all-different layout alone:
# averaging pixel pairs puts a plane of the other two layouts on exactly 0.5 at most pixels, where float64 itself decides nothing.
MASK_RUNS = tuple((c[0], l, 1) for c in MASK_CASES for l in LAYOUTS if c[0] != "half" or l == "all_different") + \
    tuple((c[0], l, 2) for c in MASK_CASES[:3] for l in LAYOUTS)


def mask_case(name):
    return next(c for c in MASK_CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def dense_map(name, layout, index_bytes):
    """The condensed map at mask resolution: uint8 (index_bytes 1) or uint16 (2) [h,w]."""
    i, (_, (h, w), _, _, _) = next((i, c) for i, c in enumerate(MASK_CASES) if c[0] == name)
    yy, xx = np.mgrid[0:h, 0:w]
    if layout == "rectangles":                      # 8 instances, later ones on top, background left
        lab, rng = np.zeros((h, w), np.int64), np.random.RandomState(2000 + i)
        for k in range(8):
            y0, x0 = rng.randint(0, h), rng.randint(0, w)
            lab[y0:y0 + 1 + rng.randint(0, max(h // 2, 1)), x0:x0 + 1 + rng.randint(0, max(w // 2, 1))] = k + 1
        vals = np.array((0,) + (NARROW_RECT if index_bytes == 1 else WIDE_INDICES + (32768, 255)))   # (two instances have two parts)
        out = vals[lab]
    elif layout == "all_different":                 # 23 indices, neighbours never equal: 16 distinct labels under most output pixels
        lab = 1 + (7 * (yy * w + xx)) % 23
        out = lab if index_bytes == 1 else np.array(WIDE_INDICES)[lab % 6]
    else:                                           # one-pixel stripes of two indices, the lower half shifted by one pixel
        assert layout == "stripes"
        a, b = (3, 200) if index_bytes == 1 else (32767, 32768)
        out = np.where((xx + (yy >= h // 2)) % 2 == 0, a, b)
    return _frozen(out.astype(np.uint8 if index_bytes == 1 else np.uint16))


# ------------------------------------------------------------------------------------------------ scatter
SCATTER_HW = (13, 17)
LUT = (0, 255, 256, 65535, 65536, 9, -4, 1)          # 256: zero at width 1, kept at width 2; 65536 and the negative entry: zero at both


def scatter_points():
    """(ys, xs, labels) int64: every refusal next to accepted points, no two accepted points on one pixel."""
    H, W = SCATTER_HW
    n = len(LUT)
    pts = [  # (y, x, label); the LUT slot read is label + 1
        (-1, 3, 0), (H, 3, 0), (3, -1, 0), (3, W, 0), (-(2 ** 40), 2, 0), (2, 2 ** 40, 0),       # outside on each side: nothing written
        (0, 0, -1), (0, 1, -2), (0, 2, -(2 ** 40)),                                              # slot 0 (background) and below the LUT
        (1, 0, n - 2), (1, 1, n - 1), (1, 2, n), (1, 3, 2 ** 40), (1, 4, 2 ** 31 - 1),            # last slot, one past it, beyond
        (2, 0, 0), (2, 1, 1), (2, 2, 2), (2, 3, 3), (2, 4, 4), (2, 5, 5),                         # 255, 256, 65535, 65536, 9, -4
        (0, W - 1, 0), (H - 1, 0, 4), (H - 1, W - 1, 1),                                          # the corners
    ]
    a = np.array(pts, dtype=np.int64)
    return _frozen(a[:, 0].copy()), _frozen(a[:, 1].copy()), _frozen(a[:, 2].copy())


SCATTER_BIG_HW = (725, 724)                          # 524,900 map pixels


@functools.lru_cache(maxsize=None)
def scatter_big():
    """524,600 points on distinct pixels of the big map (300 pixels stay background): both the zeroing and the scatter loop stride."""
    H, W = SCATTER_BIG_HW
    rng = np.random.RandomState(3000)
    flat = rng.permutation(H * W)[:H * W - 300].astype(np.int64)
    labels = rng.randint(-2, len(LUT) + 1, flat.size).astype(np.int64)
    return _frozen(flat // W), _frozen(flat % W), _frozen(labels)
