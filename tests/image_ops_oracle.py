"""Numpy restatements of the image-space kernels (csrc/image_ops.hip on csrc/bilinear.h), in two kinds.

TWINS: the arithmetic csrc/bilinear.h and image_ops.hip spell out, in float32 with one rounding per operation -- numpy evaluates every
ufunc on float32 arrays in float32 and never contracts a product into a sum -- and a fused multiply-add exactly where the kernels write
`fmaf` (``_fma``: the float64 product of two float32 is exact, the float64 sum is corrected where its own rounding would land on a
float32 tie, so the one rounding to float32 is the fma's; no other float64 enters a twin).  A kernel that computes what its source says
equals its twin bit for bit.  The scales are formed as the launchers form them: float(in) / float(out),
float32(1.0 / float64(mask_scale)), up = floor(float32(h) * mask_scale).
``masks_twin`` does NOT restate the kernel's condensed evaluation: it builds one whole one-hot plane per index, up-samples, crops,
resizes, thresholds and lets later indices overwrite earlier ones, the way the reference's writers do -- so its agreement with the
kernel checks the argument that the 16 source pixels under an output pixel decide it.

Where the fmas are is not free: the source index scale * (dst + 0.5) - 0.5 is one fma in torch's kernels, and the older tests hold the
device to torch's F.interpolate within 1e-4 (test_preprocess_frames_vs_golden_and_oracle, test_masked_preprocess, the writers' mask
tests).  A device build that rounded the product first failed all three on the MI355X (8e-4 and 2.9e-4 against the 1e-4; 0.5 % of
the mask pixels against 0.1 %), so the twins fuse there too; the kernels used to reach the same instructions only through the
compiler's default contraction of what was written as __fmul_rn / __fadd_rn / __fsub_rn.

EXACT FORMS: float64 throughout with the scales in / out and 1 / mask_scale, in the reference's order of operations as restated in
oracle/pipeline.py, oracle/masks.py and tests/augment_oracle.py:preprocess_masked -- normalise, mask, resize; flip; pad -- not the
kernel's (which resizes the raw pixels first wherever no tap is masked; the two orders agree in exact arithmetic because the
normalisation is affine and the bilinear weights sum to one).

The bounds that tie the two together are derived, not measured:
  * make_tap rounds the scale, the product and the subtraction (its fma spares one), each moving the source coordinate by at most
    in_size * 2^-24; the interpolant is continuous (the clamps included) with slope <= 255 per source pixel; the remaining
    roundings (two weights, four levels of the lerp, / 255, - mean, / std, and the float32 mean and std themselves) are each <= 2^-24 of a value <= 255.  Per
    channel: |twin - exact| <= (3 (H0 + W0) + 16) 2^-24 S_c with S_c = (unit_scale ? 1 : 255) / |std_c|   (``preprocess_bound``).
  * the same over the masks' two stages, planes in [0, 1]: band = (3 (h + w + crop_h + crop_w) + 8) 2^-24   (``mask_band``); a
    thresholded plane may differ from the exact one only where the exact value lies within the band of 0.5.
"""
import numpy as np

F32 = np.float32
EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ twins (float32)
def _fma(a, b, c):
    """fmaf on float32 operands: round(a * b + c) with ONE rounding.  p = a * b is exact in float64 (48 bits); s = p + c rounds to 53
    bits, and only if s sits exactly on a float32 tie while the discarded part (TwoSum's error term, exact) is not zero would the second
    rounding go wrong: there s is nudged one float64 ulp towards the true sum first."""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = np.atleast_1d(p + c)
    t = s - p
    err = (p - (s - t)) + (c - t)
    tie = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) & (err != 0)
    s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32).reshape(np.broadcast(p, c).shape)


def taps(scale, n_out, n_in):
    """bilinear.h make_tap for dst = 0 .. n_out - 1 -> (i0, i1 int64 [n_out], w0, w1 float32 [n_out])."""
    scale = F32(scale)
    dst = np.arange(n_out, dtype=F32)
    src = _fma(scale, dst + F32(0.5), F32(-0.5))
    src = np.where(src < F32(0), F32(0), src)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    l1 = src - i0.astype(F32)
    l1 = np.minimum(np.maximum(l1, F32(0)), F32(1))
    i1 = i0 + (i0 < n_in - 1)
    w0 = F32(1) - l1
    assert src.dtype == l1.dtype == w0.dtype == F32
    return i0, i1, w0, l1


def _lerp2(v00, v01, v10, v11, wy0, wy1, wx0, wx1):
    """bilinear.h lerp2: (v00 wx0 + v01 wx1) wy0 + (v10 wx0 + v11 wx1) wy1; in each sum the second product is rounded and the first
    is fused into the addition."""
    if v00.dtype != F32:            # the exact forms share the gather: plain float64 there
        return (v00 * wx0 + v01 * wx1) * wy0 + (v10 * wx0 + v11 * wx1) * wy1
    r0 = _fma(v00, wx0, v01 * wx1)
    r1 = _fma(v10, wx0, v11 * wx1)
    return _fma(r0, wy0, r1 * wy1)


def _resize(plane, ty, tx, lead=0):
    """``plane`` [..., H, W, (C)] sampled at the taps: ``lead`` leading axes, trailing channel axis if plane.ndim - lead == 3."""
    (y0, y1, wy0, wy1), (x0, x1, wx0, wx1) = ty, tx
    trail = plane.ndim - lead - 2
    ys = (slice(None),) * lead
    g = lambda yi, xi: plane[ys + (yi[:, None], xi[None, :])]
    shp_y = (len(y0), 1) + (1,) * trail
    shp_x = (1, len(x0)) + (1,) * trail
    return _lerp2(g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1), wy0.reshape(shp_y), wy1.reshape(shp_y), wx0.reshape(shp_x), wx1.reshape(shp_x))


def _normalise(a, mean, std, unit_scale):
    """image_ops.hip normalise: (/ 255) -> (a - mean) / std, unfused; mean, std float32 [3] on the trailing axis."""
    if unit_scale:
        a = a / F32(255)
    return (a - mean) / std


def preprocess_twin(frames, invalid, new_hw, pad_hw, mean, std, unit_scale, flip):
    """preprocess_kernel: uint8 [T,H0,W0,3] (+ invalid uint8 [T,H0,W0] | None) -> float32 [T,3,pad_h,pad_w].  A pixel takes the
    masked order (normalise -> x (1 - invalid) -> resize) only when one of its four taps is invalid; every other pixel resizes the raw
    values and normalises the result."""
    frames = np.asarray(frames)
    T, H0, W0, _ = frames.shape
    (nh, nw), (ph, pw) = new_hw, pad_hw
    mean, std = np.asarray(mean, dtype=F32), np.asarray(std, dtype=F32)       # (the binding hands the kernel C floats)
    ty, tx = taps(F32(H0) / F32(nh), nh, H0), taps(F32(W0) / F32(nw), nw, W0)
    f = frames.astype(F32)
    v = _normalise(_resize(f, ty, tx, lead=1), mean, std, unit_scale)
    if invalid is not None:
        keep = (np.asarray(invalid) == 0)
        k = keep.astype(F32)
        vm = _resize(_normalise(f, mean, std, unit_scale) * k[..., None], ty, tx, lead=1)
        g = lambda yi, xi: keep[:, yi[:, None], xi[None, :]]
        all_valid = g(ty[0], tx[0]) & g(ty[0], tx[1]) & g(ty[1], tx[0]) & g(ty[1], tx[1])
        v = np.where(all_valid[..., None], v, vm)
    assert v.dtype == F32
    out = np.zeros((T, 3, ph, pw), F32)
    for c in range(3):
        out[:, 2 - c if flip else c, :nh, :nw] = v[..., c]
    return out


def mask_geometry(h, w, mask_scale, crop_hw):
    """launch_resample's sizes and scale: (up_h, up_w, up_scale float32, accepted)."""
    ms = F32(mask_scale)
    up_h, up_w = int(np.floor(F32(h) * ms)), int(np.floor(F32(w) * ms))
    ok = 1 <= crop_hw[0] <= up_h and 1 <= crop_hw[1] <= up_w
    return up_h, up_w, F32(1.0 / np.float64(ms)), ok


def soft_masks_twin(dense, mask_scale, crop_hw, out_hw):
    """(indices ascending [K], float32 planes [K,out_h,out_w]): one-hot plane of each index present -> x mask_scale -> crop -> resize."""
    dense = np.asarray(dense)
    h, w = dense.shape
    up_h, up_w, up_scale, ok = mask_geometry(h, w, mask_scale, crop_hw)
    assert ok, "crop %s exceeds the up-sampled map (%d, %d)" % (crop_hw, up_h, up_w)
    (ch, cw), (oh, ow) = crop_hw, out_hw
    # rows / columns 0 .. crop - 1 of the up-sampled plane: the crop takes the top-left corner
    uy, ux = taps(up_scale, ch, h), taps(up_scale, cw, w)
    ty, tx = taps(F32(ch) / F32(oh), oh, ch), taps(F32(cw) / F32(ow), ow, cw)
    idx = np.unique(dense)
    idx = idx[idx != 0]
    planes = np.zeros((len(idx), oh, ow), F32)
    for n, v in enumerate(idx):
        planes[n] = _resize(_resize((dense == v).astype(F32), uy, ux), ty, tx)
    return idx, planes


def overwrite(idx, hard, dtype):
    """davis.py:104-107: planes in ascending index order, later ones overwrite earlier ones -> condensed map."""
    out = np.zeros(hard.shape[1:], dtype)
    for n, v in enumerate(idx):
        out[hard[n]] = v
    return out


def masks_twin(dense, mask_scale, crop_hw, out_hw):
    """mask_resample_kernel's result the reference's way: K whole planes, > 0.5, later indices overwrite earlier ones."""
    idx, planes = soft_masks_twin(dense, mask_scale, crop_hw, out_hw)
    return overwrite(idx, planes > F32(0.5), np.asarray(dense).dtype)


def scatter_twin(ys, xs, labels, lut, H, W, index_bytes):
    """mask_zero_kernel + mask_scatter_kernel: lut[label + 1] at (y, x) when the point is inside, the label is in the LUT and the
    entry fits the index type; 0 otherwise (a refused point still writes nothing, a refused VALUE writes 0).  No two points may share
    a pixel: the kernel's order is a race by design."""
    dtype, max_v = (np.uint8, 256) if index_bytes == 1 else (np.uint16, 65536)
    dense = np.zeros((H, W), dtype)
    ys, xs, labels, lut = (np.asarray(a, dtype=np.int64) for a in (ys, xs, labels, lut))
    inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    l = labels + 1
    in_lut = (l >= 0) & (l < len(lut))
    v = np.where(in_lut, lut[np.where(in_lut, l, 0)] if len(lut) else 0, 0)
    v = np.where((v > 0) & (v < max_v), v, 0)
    flat = ys[inside] * W + xs[inside]
    assert len(np.unique(flat)) == len(flat), "two points on one pixel"
    dense.reshape(-1)[flat] = v[inside].astype(dtype)
    return dense


# ------------------------------------------------------------------------------------------------ exact forms (float64)
def taps_exact(scale, n_out, n_in):
    """torch's align_corners=False rule in float64: (i0, i1, w0, w1)."""
    src = np.maximum(np.float64(scale) * (np.arange(n_out, dtype=np.float64) + 0.5) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    l1 = np.clip(src - i0, 0.0, 1.0)
    return i0, i0 + (i0 < n_in - 1), 1.0 - l1, l1


def preprocess_exact(frames, invalid, new_hw, pad_hw, mean, std, unit_scale, flip):
    """normalise -> x (1 - invalid) -> resize; flip; pad, float64 [T,3,pad_h,pad_w]."""
    frames = np.asarray(frames)
    T, H0, W0, _ = frames.shape
    (nh, nw), (ph, pw) = new_hw, pad_hw
    x = frames.astype(np.float64)
    if unit_scale:
        x = x / 255.0
    x = (x - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)
    if invalid is not None:
        x = x * (np.asarray(invalid) == 0)[..., None]
    x = _resize(x, taps_exact(np.float64(H0) / nh, nh, H0), taps_exact(np.float64(W0) / nw, nw, W0), lead=1)
    assert x.dtype == np.float64
    x = x.transpose(0, 3, 1, 2)
    if flip:
        x = x[:, ::-1]
    out = np.zeros((T, 3, ph, pw), np.float64)
    out[:, :, :nh, :nw] = x
    return out


def soft_masks_exact(dense, mask_scale, crop_hw, out_hw):
    """(indices ascending [K], float64 planes [K,out_h,out_w]) before the threshold: F.interpolate(scale_factor=s) has
    floor(in * s) outputs at coordinate scale 1 / s; crop; size-driven resize at crop / out."""
    dense = np.asarray(dense)
    h, w = dense.shape
    s = np.float64(mask_scale)
    up_h, up_w = int(np.floor(h * s)), int(np.floor(w * s))
    (ch, cw), (oh, ow) = crop_hw, out_hw
    assert ch <= up_h and cw <= up_w
    uy, ux = taps_exact(1.0 / s, ch, h), taps_exact(1.0 / s, cw, w)
    ty, tx = taps_exact(np.float64(ch) / oh, oh, ch), taps_exact(np.float64(cw) / ow, ow, cw)
    idx = np.unique(dense)
    idx = idx[idx != 0]
    planes = np.zeros((len(idx), oh, ow), np.float64)
    for n, v in enumerate(idx):
        planes[n] = _resize(_resize((dense == v).astype(np.float64), uy, ux), ty, tx)
    return idx, planes


# ------------------------------------------------------------------------------------------------ the derived bounds
BAND_SHARE_CAP = 0.03          # a condition on the inputs: at most this share of a case's pixels may lie in the band


def preprocess_bound(H0, W0, std, unit_scale, flip):
    """Per OUTPUT channel [3]: (3 (H0 + W0) + 16) 2^-24 S_c, S_c = (unit_scale ? 1 : 255) / |std_c| of the source channel stored there."""
    s = (1.0 if unit_scale else 255.0) / np.abs(np.asarray(std, np.float64))
    b = (3.0 * (H0 + W0) + 16.0) * EPS * s
    return b[::-1].copy() if flip else b


def check_preprocess(got, exact, new_hw, bound, what=""):
    """``got`` float32 against the exact form: within the channel's bound inside the image, exactly zero in the padding.  -> the
    largest error as a share of its bound."""
    nh, nw = new_hw
    got = np.asarray(got)
    assert got.shape == exact.shape and got.dtype == F32, what
    assert not got[:, :, nh:].any() and not got[:, :, :, nw:].any(), "%s: the padding is not zero" % what
    err = np.abs(got.astype(np.float64) - exact).max(axis=(0, 2, 3))
    assert (err <= bound).all(), "%s: max |got - exact| per channel %s exceeds the bound %s" % (what, err, bound)
    return float((err / bound).max())


def mask_band(h, w, crop_hw):
    return (3.0 * (h + w + crop_hw[0] + crop_hw[1]) + 8.0) * EPS


def check_masks(got, idx, exact_planes, band, what=""):
    """A condensed map against the exact planes: equal to ``overwrite(exact > 0.5)`` wherever no plane lies within ``band`` of 0.5, and
    at most BAND_SHARE_CAP of the pixels may lie in the band.  -> (share in the band, mismatches inside the band)."""
    got = np.asarray(got)
    in_band = (np.abs(exact_planes - 0.5) <= band).any(axis=0) if len(idx) else np.zeros(got.shape, bool)
    share = float(in_band.mean())
    assert share <= BAND_SHARE_CAP, "%s: %.4f of the pixels lie in the band" % (what, share)
    ref = overwrite(idx, exact_planes > 0.5, got.dtype)
    wrong = got != ref
    assert not (wrong & ~in_band).any(), "%s: %d pixels differ from the exact form outside the band" % (what, int((wrong & ~in_band).sum()))
    return share, int(wrong.sum())
