"""``ImageToSeqAugmenter`` under the reference's name (data/image_to_seq_augmenter.py): there imgaug warps an image, its condensed
instance map and an all-ones image into one more frame of a clip.  Here the class only SAMPLES the warp, on the host and without any
library -- ``hip.warp_clip`` and ``hip.motion_blur`` apply it on the device, and include/stemseg_hip.h defines what they compute.  The
distributions below are this library's contract (DESIGN.md section 9p lists where they depart from imgaug 0.4):

    jitter        n in {1, 2} uniform; n = 1: one of (add, hue / saturation) uniformly; applied in that order
    add, hs       integers uniform over ``brightness_range`` / ``hue_saturation_range``, ends included
    perspective   per corner (x, y) a jitter |N(0, magnitude)| mod 1 of the frame's extent, towards the inside; the homography takes that
                  quadrilateral to the whole frame
    affine        about the frame's centre ((W - 1) / 2, (H - 1) / 2): rotation uniform in degrees, translation one uniform draw per axis
                  as a fraction of the size, scale uniform over ``scale_range`` (the reference's 1.0: no draw)
    composition   perspective, then affine; inverted in fp64 and scaled to a denominator of 1 at the frame's centre
    motion blur   with probability ``motion_blur_prob`` one k of ``motion_blur_kernel_sizes``, a direction ~ U(-1, 1), an angle ~ U(0, 360)

``sample`` draws from the ``random.Random`` it is given, in the order above, so a seeded run is reproducible (the reference seeds imgaug
from the wall clock).  Everything returned is float / int / list: it travels in a recipe."""
import math
import random

import numpy as np

JITTER_ADD, JITTER_HUE_SAT = 1, 2


def perspective_matrix(jitters, width, height):
    """jitters: four (jx, jy) fractions for the corners top-left, top-right, bottom-right, bottom-left -> the 3 x 3 fp64 homography that
    takes the inset quadrilateral to the whole frame (pixel centres: corners (0, 0) .. (W - 1, H - 1))."""
    (a, b), (c, d), (e, f), (g, h) = jitters
    quad = np.array([[a, b], [1 - c, d], [1 - e, 1 - f], [g, 1 - h]], np.float64) * [width - 1, height - 1]
    full = np.array([[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1]], np.float64)
    rows, rhs = [], []
    for (x, y), (X, Y) in zip(quad, full):
        rows.append([x, y, 1, 0, 0, 0, -X * x, -X * y]); rhs.append(X)
        rows.append([0, 0, 0, x, y, 1, -Y * x, -Y * y]); rhs.append(Y)
    return np.append(np.linalg.solve(np.asarray(rows), np.asarray(rhs)), 1.0).reshape(3, 3)


def affine_matrix(rotation_deg, translate_px, scale, width, height):
    """Rotation and scale about the frame's centre, then the translation: 3 x 3 fp64."""
    a = math.radians(rotation_deg)
    c, s = math.cos(a) * scale, math.sin(a) * scale
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    return np.array([[c, -s, cx - c * cx + s * cy + translate_px[0]], [s, c, cy - s * cx - c * cy + translate_px[1]], [0, 0, 1]], np.float64)


def invert_homography(m, width, height):
    """The fp64 inverse, scaled so that its denominator is 1 at the frame's centre (``warp_clip`` takes a pixel whose denominator is not
    above 1e-12 as outside, which means something only at a fixed scale)."""
    inv = np.linalg.inv(np.asarray(m, np.float64))
    d = inv[2, 0] * (width - 1) / 2.0 + inv[2, 1] * (height - 1) / 2.0 + inv[2, 2]
    return inv / d if abs(d) > 1e-300 else inv


def _bilinear_zero(img, u, v):
    """img [k, k] read at (u, v) with a zero border, numpy fp64."""
    k = img.shape[0]
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = u - x0, v - y0
    out = np.zeros(u.shape)
    for yt, wy in ((y0, 1 - fy), (y0 + 1, fy)):
        for xt, wx in ((x0, 1 - fx), (x0 + 1, fx)):
            ok = (xt >= 0) & (xt < k) & (yt >= 0) & (yt < k)
            out += np.where(ok, wy * wx * img[np.clip(yt, 0, k - 1), np.clip(xt, 0, k - 1)], 0.0)
    return out


def blur_matrix(k, angle_deg, direction):
    """The k x k motion-blur correlation matrix (k odd): the middle column linspace(d, 1 - d, k), d = (direction + 1) / 2, rotated by
    ``angle_deg`` about the centre with a bilinear resample, normalised to sum 1 -> float32 [k, k]."""
    assert k % 2 == 1 and k >= 1
    d = (min(max(direction, -1.0), 1.0) + 1) / 2.0
    m = np.zeros((k, k), np.float64)
    m[:, k // 2] = np.linspace(d, 1 - d, k)
    quarter = int(round(angle_deg / 90.0))
    if abs(angle_deg - 90.0 * quarter) < 1e-12:
        rot = np.rot90(m, -quarter % 4)                       # exact at the multiples of 90 degrees
    else:
        a, c = math.radians(angle_deg), (k - 1) / 2.0
        y, x = np.mgrid[0:k, 0:k].astype(np.float64)
        rot = _bilinear_zero(m, math.cos(a) * (x - c) + math.sin(a) * (y - c) + c, -math.sin(a) * (x - c) + math.cos(a) * (y - c) + c)
    total = rot.sum()
    if total <= 0:                                            # (cannot happen for |direction| <= 1: the centre tap is 0.5)
        rot, total = m, m.sum()
    return (rot / total).astype(np.float32)


class ImageToSeqAugmenter(object):
    def __init__(self, perspective=True, affine=True, motion_blur=True, brightness_range=(-50, 50), hue_saturation_range=(-15, 15),
                 perspective_magnitude=0.12, scale_range=1.0, translate_range={"x": (-0.15, 0.15), "y": (-0.15, 0.15)},
                 rotation_range=(-20, 20), motion_blur_kernel_sizes=(7, 9), motion_blur_prob=0.5):
        self.perspective, self.affine, self.motion_blur = bool(perspective), bool(affine), bool(motion_blur)
        self.brightness_range = tuple(int(v) for v in brightness_range)
        self.hue_saturation_range = tuple(int(v) for v in hue_saturation_range)
        self.perspective_magnitude = float(perspective_magnitude)
        self.scale_range = scale_range
        if not isinstance(translate_range, dict):          # one range for both axes (the image loaders' (-0.1, 0.1)); still a draw per axis
            translate_range = {"x": translate_range, "y": translate_range}
        self.translate_range = {k: tuple(float(x) for x in v) for k, v in translate_range.items()}
        self.rotation_range = tuple(float(v) for v in rotation_range)
        self.motion_blur_kernel_sizes = tuple(int(k) for k in motion_blur_kernel_sizes)
        self.motion_blur_prob = float(motion_blur_prob)
        assert all(k % 2 == 1 and 1 <= k <= 11 for k in self.motion_blur_kernel_sizes), "motion blur kernels are odd and at most 11 x 11"

    def sample(self, width, height, rng):
        """One warp: {"hinv": nine floats (output pixel -> source coordinate), "matrix": nine floats (the forward map), "add", "hs",
        "flags", "blur": k x k lists or None, "params": what was drawn}."""
        n = rng.randint(1, 2)
        flags = JITTER_ADD | JITTER_HUE_SAT if n == 2 else (JITTER_ADD, JITTER_HUE_SAT)[rng.randint(0, 1)]
        add = rng.randint(*self.brightness_range) if flags & JITTER_ADD else 0
        hs = rng.randint(*self.hue_saturation_range) if flags & JITTER_HUE_SAT else 0
        drawn = {"corners": None, "rotation": 0.0, "translate": (0.0, 0.0), "scale": 1.0, "blur": None}
        m = np.eye(3)
        if self.perspective:
            drawn["corners"] = [(abs(rng.gauss(0.0, self.perspective_magnitude)) % 1.0, abs(rng.gauss(0.0, self.perspective_magnitude)) % 1.0)
                                for _ in range(4)]
            m = perspective_matrix(drawn["corners"], width, height)
        if self.affine:
            drawn["rotation"] = rng.uniform(*self.rotation_range)
            drawn["translate"] = (rng.uniform(*self.translate_range["x"]), rng.uniform(*self.translate_range["y"]))
            if not isinstance(self.scale_range, (int, float)):
                drawn["scale"] = rng.uniform(*self.scale_range)
            else:
                drawn["scale"] = float(self.scale_range)
            m = affine_matrix(drawn["rotation"], (drawn["translate"][0] * width, drawn["translate"][1] * height), drawn["scale"], width, height) @ m
        blur = None
        if self.motion_blur and rng.random() < self.motion_blur_prob:
            k = rng.choice(self.motion_blur_kernel_sizes)
            direction, angle = rng.uniform(-1.0, 1.0), rng.uniform(0.0, 360.0)
            drawn["blur"] = (k, direction, angle)
            blur = blur_matrix(k, angle, direction).tolist()
        return {"hinv": invert_homography(m, width, height).reshape(-1).tolist(), "matrix": m.reshape(-1).tolist(), "add": int(add), "hs": int(hs),
                "flags": int(flags), "blur": blur, "params": drawn}

    def sample_clip(self, width, height, num_warps):
        """``num_warps`` warps, each from a generator of its own seeded with ONE ``random.getrandbits(64)`` of the global generator."""
        return [self.sample(width, height, random.Random(random.getrandbits(64))) for _ in range(num_warps)]
