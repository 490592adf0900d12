"""numpy restatement of the augmentation transforms include/stemseg_hip.h defines (csrc/augment.hip): the source coordinates and every
nearest / inside decision in fp64 exactly as the kernels compute them, the resampled values in fp64 (the kernels sum in fp32: the band
rule below), the colour jitter in float32 operation for operation (bit for bit).  Also the inputs the tests share, all from fixed seeds,
and the band rule itself."""
import numpy as np

JITTER_ADD, JITTER_HUE_SAT = 1, 2
U8_BAND = 1e-3          # a uint8 may differ by 1 where the oracle's unrounded value is this close to k + 0.5 (fp32 taps err by ~1e-4)
COORD_BAND = 1e-9       # a plane bit may differ where a source coordinate is this close to a half-integer
WEIGHT_BAND = 1e-6      # an invalid / mask bit may differ where the weight sum is this close to 0.5
SHARE_CAP = 1e-3        # ... and fewer than this share of an output's elements may differ at all


# ------------------------------------------------------------------------------------------------ jitter (float32, bit for bit)
def _round_u8(v):
    """floor(v + 0.5) clamped, v float32."""
    f = np.floor(v + np.float32(0.5))
    return np.clip(f, 0, 255).astype(np.int32)


def jitter(bgr, add, hs, flags):
    """uint8 [..., 3] (b, g, r) -> uint8 [..., 3]: warp.h's jitter_pixel."""
    f32 = np.float32
    px = np.asarray(bgr).astype(np.int32)
    b, g, r = px[..., 0], px[..., 1], px[..., 2]
    add, hs = int(np.clip(add, -255, 255)), int(np.clip(hs, -255, 255))
    if flags & JITTER_ADD:
        b, g, r = [np.clip(c + add, 0, 255) for c in (b, g, r)]
    if flags & JITTER_HUE_SAT:
        V = np.maximum(b, np.maximum(g, r))
        diff = V - np.minimum(b, np.minimum(g, r))
        with np.errstate(divide="ignore", invalid="ignore"):
            S = np.where(V > 0, np.floor((f32(255) * diff.astype(f32)) / V.astype(f32) + f32(0.5)), 0).astype(np.int32)
            fd = diff.astype(f32)
            hr = (f32(60) * (g - b).astype(f32)) / fd
            hg = f32(120) + (f32(60) * (b - r).astype(f32)) / fd
            hb = f32(240) + (f32(60) * (r - g).astype(f32)) / fd
            h = np.where(V == r, hr, np.where(V == g, hg, hb)).astype(f32)
            h = np.where(h < 0, h + f32(360), h).astype(f32)
            Hh = np.where(diff > 0, np.floor(h * f32(0.5) + f32(0.5)), 0).astype(np.int32)
        Hh = np.where(Hh >= 180, Hh - 180, Hh)
        dh = abs(hs * 180) // 255 * (1 if hs >= 0 else -1)          # truncation towards zero
        Hh = (Hh + dh) % 180
        S = np.clip(S + hs, 0, 255)
        sector = Hh // 30
        f = (Hh - 30 * sector).astype(f32) / f32(30)
        s = S.astype(f32) / f32(255)
        v = V.astype(f32)
        one = f32(1)
        p = v * (one - s)
        q = v * (one - s * f)
        t = v * (one - s * (one - f))
        rr = np.choose(sector, [v, q, p, p, t, v])
        gg = np.choose(sector, [t, v, v, q, p, p])
        bb = np.choose(sector, [p, p, t, v, v, q])
        for a in (p, q, t, rr):
            assert a.dtype == np.float32
        b, g, r = _round_u8(bb), _round_u8(gg), _round_u8(rr)
    return np.stack([b, g, r], -1).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ warp_clip
def source_coords(hinv, H, W):
    """-> (u, v float64 [H, W], inside bool [H, W]): the kernel's unfused fp64 coordinates; inside: d > 1e-12 and (u, v) within reach of a tap."""
    h = np.asarray(hinv, np.float64).reshape(9)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        d = (h[6] * x + h[7] * y) + h[8]
        u = ((h[0] * x + h[1] * y) + h[2]) / d
        v = ((h[3] * x + h[4] * y) + h[5]) / d
        inside = (d > 1e-12) & (u > -1.0) & (u < W) & (v > -1.0) & (v < H)
    return np.where(inside, u, 0.0), np.where(inside, v, 0.0), inside


def bilinear(img, u, v, inside, column_map=None):
    """img [H, W, C] -> (value float64 [H, W, C], weight float64 [H, W]): zero-border bilinear read at (u, v), and the summed weights of
    the taps inside the frame.  column_map(xt, yt) -> xt: the duplicator's mirrored read."""
    H, W = img.shape[:2]
    img = np.asarray(img, np.float64)
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = u - x0, v - y0
    val, wsum = np.zeros(u.shape + (img.shape[2],)), np.zeros(u.shape)
    for a, wy in ((0, 1.0 - fy), (1, fy)):
        for b, wx in ((0, 1.0 - fx), (1, fx)):
            xt, yt = x0 + b, y0 + a
            ok = inside & (xt >= 0) & (xt < W) & (yt >= 0) & (yt < H)
            xs = xt if column_map is None else column_map(xt, yt)
            ok = ok & (xs >= 0) & (xs < W)
            w = np.where(ok, wy * wx, 0.0)
            val += w[..., None] * img[np.clip(yt, 0, H - 1), np.clip(xs, 0, W - 1)]
            wsum += w
    return val, wsum


def round_u8(val):
    return np.clip(np.floor(val + 0.5), 0, 255).astype(np.uint8)


def condense_expand(planes, yn, xn, ok):
    """The reference's condense_masks -> nearest read -> expand_masks: [N, H, W] planes read at (yn, xn) where ok."""
    N, H, W = planes.shape
    condensed = np.zeros((H, W), np.int32)
    for n in range(N):
        condensed = np.where(planes[n] != 0, n + 1, condensed)
    got = np.where(ok, condensed[np.clip(yn, 0, H - 1), np.clip(xn, 0, W - 1)], 0)
    return np.stack([(got == n + 1).astype(np.uint8) for n in range(N)], 0) if N else np.zeros((0,) + got.shape, np.uint8)


def warp_clip(src, planes, hinv, jit=None):
    """-> dict(frames [F,H,W,3], planes [N,F,H,W], invalid [F,H,W], and what the band rule reads: soft [F,H,W,3], weight [F,H,W],
    near_coord bool [F,H,W])."""
    H, W = src.shape[:2]
    hm = np.asarray(hinv, np.float64).reshape(-1, 9)
    F = hm.shape[0]
    jt = np.zeros((F, 3), np.int64) if jit is None else np.asarray(jit).reshape(F, 3)
    planes = np.zeros((0, H, W), np.uint8) if planes is None else np.asarray(planes)
    out = {k: [] for k in ("frames", "planes", "invalid", "soft", "weight", "near_coord")}
    for f in range(F):
        u, v, inside = source_coords(hm[f], H, W)
        soft, weight = bilinear(jitter(src, *[int(t) for t in jt[f]]), u, v, inside)
        xn, yn = np.floor(u + 0.5).astype(np.int64), np.floor(v + 0.5).astype(np.int64)
        ok = inside & (xn >= 0) & (xn < W) & (yn >= 0) & (yn < H)
        near = inside & ((np.abs(u + 0.5 - np.round(u + 0.5)) < COORD_BAND) | (np.abs(v + 0.5 - np.round(v + 0.5)) < COORD_BAND))
        for k, a in (("frames", round_u8(soft)), ("planes", condense_expand(planes, yn, xn, ok)), ("invalid", (weight < 0.5).astype(np.uint8)),
                     ("soft", soft), ("weight", weight), ("near_coord", near)):
            out[k].append(a)
    res = {k: np.stack(a, 0) for k, a in out.items()}
    res["planes"] = np.ascontiguousarray(res["planes"].transpose(1, 0, 2, 3))
    return res


# ------------------------------------------------------------------------------------------------ motion_blur
def motion_blur(frames, matrices):
    """-> (out uint8 [F,H,W,3], soft float64): correlation with the float32 matrix, reflect-101 border."""
    frames = np.asarray(frames)
    soft = frames.astype(np.float64)
    for f, m in enumerate(matrices):
        if m is None:
            continue
        m = np.asarray(m, np.float32).astype(np.float64)
        k = m.shape[0]
        R = k // 2
        H, W = frames.shape[1:3]
        pad = np.pad(frames[f].astype(np.float64), ((R, R), (R, R), (0, 0)), mode="reflect")
        acc = np.zeros((H, W, 3))
        for dy in range(k):
            for dx in range(k):
                acc += m[dy, dx] * pad[dy:dy + H, dx:dx + W]
        soft[f] = acc
    return round_u8(soft), soft


# ------------------------------------------------------------------------------------------------ duplicate_instance
def duplicate_instance(frames, mask, boxes, flip, shifts):
    """-> dict(frames [T,H,W,3], masks [2,T,H,W], soft [T,H,W,3], weight [T,H,W] (the bilinear mask value), pasted bool [T,H,W])."""
    frames, mask = np.asarray(frames), np.asarray(mask)
    T, H, W = mask.shape
    out_f, soft_all, w_all = frames.copy(), frames.astype(np.float64), np.zeros((T, H, W))
    orig, dup = mask.copy(), mask.copy()
    for t in range(T):
        if boxes[t] is None:
            w_all[t] = (mask[t] != 0)
            continue
        xmin, ymin, xmax, ymax = [int(b) for b in boxes[t]]
        sx, sy = [float(np.float32(s)) for s in shifts[t]]
        u = np.broadcast_to(np.arange(W, dtype=np.float64)[None, :] - sx, (H, W))
        v = np.broadcast_to(np.arange(H, dtype=np.float64)[:, None] - sy, (H, W))
        with np.errstate(invalid="ignore"):
            inside = (u > -1.0) & (u < W) & (v > -1.0) & (v < H)
        u, v = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
        cmap = None
        if flip:
            cmap = lambda xt, yt: np.where((xt >= xmin) & (xt < xmax) & (yt >= ymin) & (yt < ymax), xmin + xmax - 1 - xt, xt)
        soft, _ = bilinear(frames[t], u, v, inside, cmap)
        msoft, _ = bilinear((mask[t] != 0).astype(np.float64)[..., None], u, v, inside, cmap)
        m = msoft[..., 0] >= 0.5
        dup[t] = m
        orig[t] = np.where(m, 0, mask[t])
        out_f[t] = np.where(m[..., None], round_u8(soft), frames[t])
        soft_all[t], w_all[t] = np.where(m[..., None], soft, frames[t]), msoft[..., 0]
    return {"frames": out_f, "masks": np.stack([orig, dup], 0).astype(np.uint8), "soft": soft_all, "weight": w_all, "pasted": dup.astype(bool)}


# ------------------------------------------------------------------------------------------------ masked pre-processing
def preprocess_masked(frames, invalid, new_hw, pad_hw, mean, std, unit_scale=False, flip_channels=False):
    """normalise -> x (1 - invalid) -> bilinear resize -> pad (coco_data_loader.py), torch CPU float32: [T,3,pad_h,pad_w]."""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        x = torch.from_numpy(np.asarray(frames)).permute(0, 3, 1, 2).float()
        if unit_scale:
            x = x / 255.0
        x = (x - torch.tensor(mean, dtype=torch.float32)[None, :, None, None]) / torch.tensor(std, dtype=torch.float32)[None, :, None, None]
        x = x * (1 - torch.from_numpy(np.asarray(invalid)).float())[:, None]
        x = F.interpolate(x, tuple(int(v) for v in new_hw), mode="bilinear", align_corners=False)
        if flip_channels:
            x = x.flip(dims=[1])
        out = torch.zeros((x.shape[0], 3, int(pad_hw[0]), int(pad_hw[1])))
        out[:, :, :new_hw[0], :new_hw[1]] = x
    return out.numpy()


# ------------------------------------------------------------------------------------------------ the band rule
def u8_band(soft):
    """bool: the oracle's unrounded value lies within U8_BAND of k + 0.5."""
    return np.abs(soft - np.floor(soft) - 0.5) <= U8_BAND


def check_u8(got, ref, soft, what=""):
    """A uint8 output against the fp64 oracle: equal, or off by one inside the band, fewer than SHARE_CAP of the elements.  -> mismatches."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    diff = got != ref
    n = int(diff.sum())
    if n:
        assert (np.abs(got.astype(np.int32) - ref.astype(np.int32))[diff] == 1).all(), "%s: a value is off by more than one" % what
        assert u8_band(soft)[diff].all(), "%s: %d values differ away from the rounding band" % (what, int((diff & ~u8_band(soft)).sum()))
        assert n < SHARE_CAP * diff.size, "%s: %d of %d values differ" % (what, n, diff.size)
    return n


def check_bits(got, ref, band, what=""):
    """A 0 / 1 output: equal, or different only where ``band`` (bool, broadcastable) is set, fewer than SHARE_CAP of the elements."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert set(np.unique(got).tolist()) <= {0, 1}, what
    diff = got != ref
    n = int(diff.sum())
    if n:
        assert np.broadcast_to(band, diff.shape)[diff].all(), "%s: %d bits differ away from the band" % (what, n)
        assert n < SHARE_CAP * diff.size, "%s: %d of %d bits differ" % (what, n, diff.size)
    return n


def weight_band(weight):
    return np.abs(weight - 0.5) <= WEIGHT_BAND


def check_warp(got_frames, got_planes, got_invalid, ref, what=""):
    check_u8(got_frames, ref["frames"], ref["soft"], what + " frames")
    check_bits(got_invalid, ref["invalid"], weight_band(ref["weight"]), what + " invalid")
    if ref["planes"].shape[0]:
        check_bits(got_planes, ref["planes"], ref["near_coord"][None], what + " planes")


# ------------------------------------------------------------------------------------------------ inputs (fixed seeds)
def image(H, W, seed):
    """A uint8 [H, W, 3] frame with smooth regions, edges and noise."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([127 + 120 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)], -1)
    base[(x // 8 + y // 8) % 2 == 0] *= 0.5
    return np.clip(base + rng.randint(-20, 21, (H, W, 3)), 0, 255).astype(np.uint8)


def planes(N, H, W, seed):
    """N overlapping discs (uint8 [N, H, W]); with N == 127 most pixels are claimed by several planes."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros((N, H, W), np.uint8)
    for n in range(N):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(3, 0.35 * min(H, W))
        if 0 < n < 4:                      # the first planes overlap for certain: the centre lies inside the disc before
            cy, cx = np.clip(prev[0] + rng.uniform(-0.6, 0.6) * prev[2], 0, H - 1), np.clip(prev[1] + rng.uniform(-0.6, 0.6) * prev[2], 0, W - 1)
        prev = (cy, cx, r)
        out[n] = ((y - cy) ** 2 + (x - cx) ** 2 <= r * r) * (1 + n % 3)          # non-zero values other than 1 count as set
    return out


def identity():
    return np.eye(3).reshape(9)


def translation(tx, ty):
    """Inverse map of a shift of the content by (tx, ty): output (x, y) reads source (x - tx, y - ty)."""
    return np.array([1, 0, -tx, 0, 1, -ty, 0, 0, 1], np.float64)


def mirror(W):
    return np.array([-1, 0, W - 1, 0, 1, 0, 0, 0, 1], np.float64)


def rotation(deg, H, W):
    a = np.deg2rad(deg)
    c, s, cx, cy = np.cos(a), np.sin(a), (W - 1) / 2.0, (H - 1) / 2.0
    m = np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0, 0, 1]])
    return np.linalg.inv(m).reshape(9)


def perspective(magnitude, H, W, seed):
    """A random quadrilateral inset from the corners by |N(0, magnitude)| mod 1 of the size, taken to the whole frame; its inverse."""
    rng = np.random.RandomState(seed)
    j = np.mod(np.abs(rng.normal(0, magnitude, (4, 2))), 1)
    quad = np.array([[j[0, 0], j[0, 1]], [1 - j[1, 0], j[1, 1]], [1 - j[2, 0], 1 - j[2, 1]], [j[3, 0], 1 - j[3, 1]]]) * [W - 1, H - 1]
    full = np.array([[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]], np.float64)
    return homography(full, quad).reshape(9)          # output (whole frame) -> source (the quadrilateral)


def homography(src_pts, dst_pts):
    """The 3 x 3 matrix taking four points to four points (h8 = 1), fp64."""
    A, bvec = [], []
    for (x, y), (X, Y) in zip(src_pts, dst_pts):
        A.append([x, y, 1, 0, 0, 0, -X * x, -X * y]); bvec.append(X)
        A.append([0, 0, 0, x, y, 1, -Y * x, -Y * y]); bvec.append(Y)
    h = np.linalg.solve(np.asarray(A, np.float64), np.asarray(bvec, np.float64))
    return np.append(h, 1.0).reshape(3, 3)


def crossing_denominator(H, W):
    """d = 1 - 2 x / W - y / 1000: positive on the left, zero or negative from x = W / 2 on -- those pixels are outside by the rule."""
    return np.array([1, 0, 0.3137, 0, 1, 0.1771, -2.0 / W, -0.001, 1], np.float64)


WARP_SHAPES = ((37, 53), (45, 40), (64, 96))
JITTERS = ((40, 0, JITTER_ADD), (-40, 0, JITTER_ADD), (0, 5, JITTER_HUE_SAT), (0, -5, JITTER_HUE_SAT), (0, 15, JITTER_HUE_SAT),
           (0, -15, JITTER_HUE_SAT), (25, -12, JITTER_ADD | JITTER_HUE_SAT))


def general_warps(H, W):
    """The seven non-exact warps of one shape: rotations of +-12 degrees, perspectives at 0.08 and 0.12, a fractional shift."""
    return [rotation(12, H, W), rotation(-12, H, W), perspective(0.08, H, W, 1), perspective(0.12, H, W, 2), perspective(0.08, H, W, 3),
            perspective(0.12, H, W, 4), translation(2.3137, -1.1771)]


def warp_cases():
    """(name, src, planes | None, hinv [F, 9], jitter [F, 3] | None) for every band-rule warp case of tests/test_gpu_augment.py."""
    cases = []
    for s, (H, W) in enumerate(WARP_SHAPES):
        for N in (0, 1, 3, 127):
            hs = general_warps(H, W)
            cases.append(("%dx%d N=%d F=7" % (H, W, N), image(H, W, 10 + s), planes(N, H, W, 20 + s) if N else None, np.stack(hs), JITTERS))
        cases.append(("%dx%d N=3 F=1" % (H, W), image(H, W, 30 + s), planes(3, H, W, 40 + s), perspective(0.12, H, W, 5)[None], None))
    return cases


def box_matrix(k):
    return np.full((k, k), 1.0 / (k * k), np.float32)


def delta_matrix(k):
    m = np.zeros((k, k), np.float32)
    m[k // 2, k // 2] = 1
    return m


def line_matrix(k, seed):
    """A motion-blur line: the middle column linspace(d, 1 - d, k), rotated by a random angle about the centre (bilinear), sum 1."""
    rng = np.random.RandomState(seed)
    d = (rng.uniform(-1, 1) + 1) / 2
    m = np.zeros((k, k))
    m[:, k // 2] = np.linspace(d, 1 - d, k)
    a = np.deg2rad(rng.uniform(0, 360))
    c = (k - 1) / 2.0
    y, x = np.mgrid[0:k, 0:k].astype(np.float64)
    u = np.cos(a) * (x - c) + np.sin(a) * (y - c) + c
    v = -np.sin(a) * (x - c) + np.cos(a) * (y - c) + c
    inside = (u > -1) & (u < k) & (v > -1) & (v < k)
    rot, _ = bilinear(m[..., None], np.where(inside, u, 0), np.where(inside, v, 0), inside)
    rot = rot[..., 0]
    return (rot / rot.sum()).astype(np.float32)


BLUR_SHAPES = ((16, 23), (40, 45))


def blur_cases():
    """(name, frames [4, H, W, 3], matrices) per shape: k = 0, 7, 9, 11 in one call, box and sampled lines."""
    cases = []
    for s, (H, W) in enumerate(BLUR_SHAPES):
        frames = np.stack([image(H, W, 50 + 4 * s + f) for f in range(4)])
        cases.append(("%dx%d box" % (H, W), frames, [None, box_matrix(7), box_matrix(9), box_matrix(11)]))
        cases.append(("%dx%d lines" % (H, W), frames, [line_matrix(11, 1 + s), None, line_matrix(7, 3 + s), line_matrix(9, 5 + s)]))
    return cases


def disc_mask(T, H, W, cx, cy, rx, ry, drift=1.0):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(((x - cx - drift * t) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1).astype(np.uint8) for t in range(T)])


def bbox(mask):
    """instance_duplicator.py:25-38: (xmin, ymin, xmax, ymax) with exclusive maxima, or None."""
    cols, rows = np.flatnonzero(mask.any(0)), np.flatnonzero(mask.any(1))
    return None if cols.size == 0 else (int(cols[0]), int(rows[0]), int(cols[-1]) + 1, int(rows[-1]) + 1)


def duplicate_cases():
    """(name, frames, mask, boxes, flip, shifts): integer and fractional shifts, flip on and off, a box on each border, a frame
    without a box, and a shift at the 0.3 x size cap."""
    T, H, W = 3, 37, 53
    frames = np.stack([image(H, W, 70 + t) for t in range(T)])
    cases = []
    mid = disc_mask(T, H, W, 20, 18, 6, 5)
    mid[1] = 0                                                    # frame 1 has no box
    for name, mask, flip, shift in (("integer", mid, False, (9.0, -3.0)), ("integer flip", mid, True, (-8.0, 2.0)),
                                    ("fraction", mid, False, (10.3, 1.7)), ("fraction flip", mid, True, (-7.6, -2.2)),
                                    ("left border", disc_mask(T, H, W, 2, 18, 6, 5, 0), False, (6.7, 0.4)),
                                    ("right border", disc_mask(T, H, W, W - 3, 18, 6, 5, 0), False, (-6.7, -0.4)),
                                    ("top border", disc_mask(T, H, W, 25, 1, 6, 5), True, (8.4, 1.3)),
                                    ("bottom border", disc_mask(T, H, W, 25, H - 2, 6, 5), True, (8.4, -1.3)),
                                    ("cap", disc_mask(T, H, W, 14, 18, 12, 9, 0), False, (min(24 * 0.9, W * 0.3), min(18 * 0.2, H * 0.3)))):
        cases.append((name, frames, mask, [bbox(m) for m in mask], flip, [shift] * T))
    return cases


# ------------------------------------------------------------------------------------------------ the duplicator's decision, restated
def duplicator_decision(boxes, W, H, draws):
    """instance_duplicator.py:41-172 in other words, on boxes (exclusive maxima) and an iterator of the ``random.random()`` values in
    the order the reference draws them: -> (None | {"flip", "shifts"}, number of values drawn)."""
    it, used = iter(draws), [0]

    def draw():
        used[0] += 1
        return next(it)
    real = [b for b in boxes if b is not None]
    left, right = any(b[0] == 0 for b in real), any(b[2] == W for b in real)
    top, bottom = any(b[1] == 0 for b in real), any(b[3] == H for b in real)

    def axis(lo, hi, size):          # the LAST frame that says something decides, as in the loop of the reference
        mult = None
        for b in real:
            ext = b[hi] - b[lo]
            if ext > 0.4 * size:
                mult = -1.0 if b[lo] == 0 else (1.0 if b[hi] == size else mult)
            elif ext < 0.2 * size:
                c = (b[lo] + b[hi]) / 2.0
                mult = 1.0 if c < 0.25 * size else (-1.0 if c > 0.75 * size else mult)
        return mult
    hm, vm = axis(0, 2, W), axis(1, 3, H)
    if left and right:
        return None, 0
    if top and bottom:
        vm = 0.0
    if hm is None:
        hm = -1.0 if draw() < 0.5 else 1.0
    if vm is None:
        vm = -1.0 if draw() < 0.5 else 1.0
    flip = (draw() < 0.5) if not (left or right) else False
    shifts = []
    for b in boxes:
        if b is None:
            shifts.append(None)
            continue
        w, h = b[2] - b[0], b[3] - b[1]
        sx = hm * (w * 0.75 + draw() * 0.25 * w)
        sy = vm * (h * draw() * 0.25)
        shifts.append((float(np.float32(min(sx, W * 0.3))), float(np.float32(min(sy, H * 0.3)))))
    return {"flip": flip, "shifts": shifts}, used[0]


# ------------------------------------------------------------------------------------------------ a batch entry from a recipe, on the host
def image_dataset_json(entries):
    """entries: (image_path, masks [N, H, W], category ids, ignore mask | None) -> the generic image-dataset JSON as a dict."""
    from tests import writer_oracle as wo
    images = []
    for path, masks, cats, ignore in entries:
        item = {"height": int(masks.shape[1]), "width": int(masks.shape[2]), "image_path": path, "categories": [int(c) for c in cats],
                "segmentations": [wo.counts_to_string(wo.encode(m)) for m in masks]}
        if ignore is not None:
            item["ignore"] = wo.counts_to_string(wo.encode(ignore))
        images.append(item)
    return {"meta": {"category_labels": {str(c): "c%d" % c for c in range(1, 5)}}, "images": images}


def write_image_datasets(base):
    """coco.json and pascal_voc.json below ``base`` over the golden's 37 x 53 JPEG and 45 x 40 PNG (already written there): three
    overlapping instances each (categories 1, 2 and 4) and a fourth of 15 pixels, below Pascal VOC's area filter; Pascal VOC with an
    ignore region."""
    import json
    import os
    entries = []
    for path, (h, w), seed in (("a/00000.jpg", (37, 53), 2), ("b/00001.png", (45, 40), 4)):
        masks = (planes(4, h, w, seed) != 0).astype(np.uint8)
        masks[3] = 0
        masks[3, 1:4, 1:6] = 1
        ignore = np.zeros((h, w), np.uint8)
        ignore[h - 9:h - 2, 3:w // 2] = 1
        entries.append((path, masks, [1, 2, 4, 1], ignore))
    for name, with_ignore in (("coco.json", False), ("pascal_voc.json", True)):
        with open(os.path.join(base, name), "w") as fh:
            json.dump(image_dataset_json([(p, m, c, i if with_ignore else None) for p, m, c, i in entries]), fh)


def image_recipe_warp(recipe, decode_image):
    """An image recipe the reference's way: the image and its planes are MIRRORED first when the recipe says so, then warped by each
    frame's own (un-mirrored) matrix; slot k of the clip shows frame perm[k].  -> (the mirrored source, its planes [P, H, W], what
    ``warp_clip`` makes of them in the clip's order)."""
    from tests import writer_oracle as wo
    w, h = recipe["size"]
    src = decode_image(recipe["frames"][0])
    pl = np.ascontiguousarray(np.stack([wo.decode(wo.string_to_counts(s), h, w) for s in recipe["rle"]]), dtype=np.uint8)
    if recipe["flip"]:
        src, pl = np.ascontiguousarray(src[:, ::-1]), np.ascontiguousarray(pl[:, :, ::-1])
    hinvs, jit, blurs = [], [], []
    for k in recipe["perm"]:
        wp = recipe["warps"][k - 1] if k else None
        hinvs.append(np.asarray(wp["hinv"]) if k else identity())
        jit.append((wp["add"], wp["hs"], wp["flags"]) if k else (0, 0, 0))
        blurs.append(None if not k or wp["blur"] is None else np.asarray(wp["blur"], np.float32))
    return src, pl, warp_clip(src, pl, np.stack(hinvs), jit), blurs
