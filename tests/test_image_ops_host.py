"""CPU tests of the restatements that tests/test_gpu_image_ops.py holds csrc/image_ops.hip to (tests/image_ops_oracle.py) on the
inputs of tests/image_ops_cases.py: the float32 twins against the float64 exact forms under the derived bounds, the properties the
twins must have on their own, the launch caps the stride cases exceed, and every argument refusal of the six entry points (each
returns -1 before any HIP call, so they run here).

Why the older tests carry 1e-4: their reference is torch's CPU float32 F.interpolate, which evaluates the source index
scale * (dst + 0.5) - 0.5 as one fma.  On random uint8 frames at 720 x 1280 -> 480 x 853, in 0..255 units, a float32 restatement of
make_tap / lerp2 that rounds every operation differs from torch by up to 7.2e-3, one with only that expression fused agrees with
torch to 3e-5, and both are 1.78e-2 from an exact float64 evaluation (the bound below gives 9.1e-2 there).  The kernels were written
as if every operation rounded (__fmul_rn and friends), but those are plain operators to the HIP compiler, which contracted them: the
device has always computed the fused index, and must -- built without the contraction it fails the 1e-4 of those older tests on the
MI355X (8e-4 and 2.9e-4) and the writers' mask test (0.5 % of the pixels against 0.1 %).  csrc/bilinear.h now writes its fmas out and
switches the contraction off, and the twins restate exactly that, so they need no slack at all.

Measured on the host (numpy twins, this file's cases; printed by the tests with -s):
  * pre-processing, 8 shapes x 3 parameter sets: max |twin - exact| is at most 0.192 of the channel's bound (the "stride" case);
    masked, 3 shapes x 5 patterns x 3 sets: at most 0.120 of it.
  * masks, 34 runs: at most 1.64 % of a run's pixels lie in the band around 0.5 (cap 3 %; "down" with stripes, all of them on exactly
    0.5), and the twin differs from the exact form at no pixel outside the band; inside it, at 48 and 20 pixels of the two "scale1"
    runs whose exact planes hit 0.5, and nowhere else.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import image_ops_cases as ic
from tests import image_ops_oracle as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# outputs (map pixels, points) above which a kernel's grid-stride loop runs: grid cap x block, as launched in csrc/image_ops.hip
PREPROCESS_CAP = 8192 * 256
RESAMPLE_CAP = 4096 * 256
SCATTER_CAP = 2048 * 256


# ------------------------------------------------------------------------------------------------ the launch caps
def test_stride_cases_exceed_the_launch_caps():
    src = open(os.path.join(ROOT, "stem-seg_amd", "csrc", "image_ops.hip")).read()
    launches = re.findall(r"hipLaunchKernelGGL\((\w+)(?:<\w+>)?, dim3\(grid_for\([^;]*?, (\d+)\)\), dim3\((\d+)\)", src)
    caps = {}
    for kernel, cap, block in launches:
        caps.setdefault(kernel, set()).add(int(cap) * int(block))
    assert caps == {"preprocess_kernel": {PREPROCESS_CAP}, "mask_resample_kernel": {RESAMPLE_CAP}, "mask_zero_kernel": {SCATTER_CAP},
                    "mask_scatter_kernel": {SCATTER_CAP}}, caps
    _, _, _, (ph, pw), T = ic.PRE_CASES[-1]
    assert T * ph * pw > PREPROCESS_CAP and all(c[4] * c[3][0] * c[3][1] < PREPROCESS_CAP for c in ic.PRE_CASES[:-1])
    assert ic.MASK_CASES[-1][4][0] * ic.MASK_CASES[-1][4][1] > RESAMPLE_CAP
    assert ic.SCATTER_BIG_HW[0] * ic.SCATTER_BIG_HW[1] > SCATTER_CAP and ic.scatter_big()[0].size > SCATTER_CAP


# ------------------------------------------------------------------------------------------------ the taps
def test_taps_twin_edges():
    """Identity: weight 1 on the pixel itself.  in_size == 1: both taps are pixel 0.  Indices stay inside, weights inside [0, 1]."""
    i0, i1, w0, w1 = io.taps(np.float32(33) / np.float32(33), 33, 33)
    assert np.array_equal(i0, np.arange(33)) and (w0 == 1).all() and (w1 == 0).all()
    i0, i1, w0, w1 = io.taps(np.float32(1) / np.float32(7), 7, 1)
    assert not i0.any() and not i1.any()
    for n_in, n_out in ((50, 64), (96, 32), (2, 63), (120, 45), (5, 3)):
        i0, i1, w0, w1 = io.taps(np.float32(n_in) / np.float32(n_out), n_out, n_in)
        e0, e1, x0, x1 = io.taps_exact(np.float64(n_in) / n_out, n_out, n_in)
        assert i0.min() >= 0 and i1.max() <= n_in - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()
        assert w0.dtype == w1.dtype == np.float32 and w1.min() >= 0 and w1.max() <= 1
        # the coordinate i0 + w1 is within 3 in_size 2^-24 of the exact one (the same tap, or the neighbour across an integer)
        assert np.abs((i0 + w1.astype(np.float64)) - (e0 + x1)).max() <= 3 * n_in * io.EPS


# ------------------------------------------------------------------------------------------------ pre-processing
@pytest.mark.parametrize("params", ic.PARAM_SETS, ids=[p[0] for p in ic.PARAM_SETS])
@pytest.mark.parametrize("case", ic.PRE_CASES, ids=[c[0] for c in ic.PRE_CASES])
def test_preprocess_twin_vs_exact(case, params):
    name, (H0, W0), new_hw, pad_hw, T = case
    _, mean, std, unit, flip = params
    fr = ic.frames(name)
    assert fr.shape == (T, H0, W0, 3) and fr.dtype == np.uint8
    if H0 * W0 >= 100:              # noise: neighbours differ by ~85
        assert 75 < np.abs(np.diff(fr.astype(np.int64), axis=2)).mean() < 95
    twin = io.preprocess_twin(fr, None, new_hw, pad_hw, mean, std, unit, flip)
    exact = io.preprocess_exact(fr, None, new_hw, pad_hw, mean, std, unit, flip)
    share = io.check_preprocess(twin, exact, new_hw, io.preprocess_bound(H0, W0, std, unit, flip), name)
    print("%s / %s: max |twin - exact| = %.3f of the bound" % (name, params[0], share))
    if name == "identity":          # normalise(pixel), bit for bit
        px = fr.astype(np.float32)
        if unit:
            px = px / np.float32(255)
        px = ((px - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)).transpose(0, 3, 1, 2)
        assert np.array_equal(twin[:, :, :H0, :W0], px[:, ::-1] if flip else px)


def test_preprocess_exact_agrees_with_the_torch_oracles():
    """The exact form restates the order of oracle/pipeline.py and augment_oracle.preprocess_masked: within their float32 noise of both."""
    from tests import augment_oracle as ao
    name, (H0, W0), new_hw, pad_hw, T = ic.PRE_CASES[1]
    for _, mean, std, unit, flip in ic.PARAM_SETS:
        for pattern in ("none", "random30"):
            inv = ic.invalid(name, pattern)
            ref = ao.preprocess_masked(ic.frames(name).copy(), (inv != 0).astype(np.uint8), new_hw, pad_hw, mean, std, unit, flip)
            exact = io.preprocess_exact(ic.frames(name), inv, new_hw, pad_hw, mean, std, unit, flip)
            assert np.abs(ref - exact).max() <= 1e-4 * max(1.0, np.abs(exact).max())


@pytest.mark.parametrize("params", ic.PARAM_SETS, ids=[p[0] for p in ic.PARAM_SETS])
@pytest.mark.parametrize("pattern", ic.INVALID_PATTERNS)
@pytest.mark.parametrize("case", ic.MASKED_CASES, ids=[c[0] for c in ic.MASKED_CASES])
def test_masked_preprocess_twin_vs_exact(case, pattern, params):
    name, (H0, W0), new_hw, pad_hw, T = case
    _, mean, std, unit, flip = params
    fr, inv = ic.frames(name), ic.invalid(name, pattern)
    twin = io.preprocess_twin(fr, inv, new_hw, pad_hw, mean, std, unit, flip)
    exact = io.preprocess_exact(fr, inv, new_hw, pad_hw, mean, std, unit, flip)
    share = io.check_preprocess(twin, exact, new_hw, io.preprocess_bound(H0, W0, std, unit, flip), name + " " + pattern)
    print("%s / %s / %s: max |twin - exact| = %.3f of the bound" % (name, pattern, params[0], share))
    plain = io.preprocess_twin(fr, None, new_hw, pad_hw, mean, std, unit, flip)
    same = float((twin == plain)[:, :, :new_hw[0], :new_hw[1]].mean())
    if pattern == "none":
        assert np.array_equal(twin, plain)
    elif pattern == "all":
        assert not twin.any()
    elif pattern == "one_pixel":
        assert 0.9 < same < 1.0 and np.array_equal(twin[:T - 1], plain[:T - 1])
    else:
        assert same < 0.5


# ------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("run", ic.MASK_RUNS, ids=["%s-%s-%d" % r for r in ic.MASK_RUNS])
def test_masks_twin_vs_exact(run):
    name, layout, ib = run
    _, (h, w), scale, crop_hw, out_hw = ic.mask_case(name)
    dense = ic.dense_map(name, layout, ib)
    assert dense.shape == (h, w) and dense.dtype == (np.uint8 if ib == 1 else np.uint16)
    idx, planes = io.soft_masks_twin(dense, scale, crop_hw, out_hw)
    twin = io.masks_twin(dense, scale, crop_hw, out_hw)
    assert twin.dtype == dense.dtype and twin.shape == tuple(out_hw)
    assert ((planes > np.float32(0.5)).sum(0) <= 1).all(), "two twin planes exceed 0.5 at one pixel"
    eidx, exact = io.soft_masks_exact(dense, scale, crop_hw, out_hw)
    assert np.array_equal(idx, eidx)
    share, wrong = io.check_masks(twin, eidx, exact, io.mask_band(h, w, crop_hw), "%s %s %d" % run)
    on_half = float((exact == 0.5).any(0).mean())
    print("%s / %s / width %d: %.4f of the pixels in the band, %.4f on exactly 0.5, %d mismatches inside it" % (name, layout, ib, share, on_half, wrong))
    assert len(idx) == {"rectangles": len(idx), "all_different": min(23, h * w) if ib == 1 else 6, "stripes": 2 if w > 1 or h > 1 else 1}[layout]
    assert np.isin(twin, np.concatenate([[0], idx])).all() and (name == "half" or len(np.unique(twin)) >= min(len(idx), 2))
    if ib == 2:
        assert set(idx.tolist()) <= set(ic.WIDE_INDICES) and idx.max() >= 32768


def distinct_under(name):
    """[out_h,out_w]: how many distinct labels the 16 source slots of each output pixel hold under the all-different layout."""
    _, (h, w), scale, crop_hw, out_hw = ic.mask_case(name)
    dense = ic.dense_map(name, "all_different", 1)
    _, _, up_scale, _ = io.mask_geometry(h, w, scale, crop_hw)
    uy, ux = io.taps(up_scale, crop_hw[0], h), io.taps(up_scale, crop_hw[1], w)
    ty = io.taps(np.float32(crop_hw[0]) / np.float32(out_hw[0]), out_hw[0], crop_hw[0])
    tx = io.taps(np.float32(crop_hw[1]) / np.float32(out_hw[1]), out_hw[1], crop_hw[1])
    rows = np.stack([uy[a][ty[b]] for a in (0, 1) for b in (0, 1)], 0)          # [4, out_h] source rows
    cols = np.stack([ux[a][tx[b]] for a in (0, 1) for b in (0, 1)], 0)
    under = dense[rows[:, None, :, None], cols[None, :, None, :]].reshape(16, out_hw[0], out_hw[1])
    return (np.diff(np.sort(under, axis=0), axis=0) != 0).sum(0) + 1


def test_all_different_layout_fills_the_sixteen_slots():
    """The dedup of the kernel's 16 source slots is exercised only if they differ: 9 distinct labels (the most that mask_scale >= 1
    allows, see image_ops_cases.LAYOUTS) under some of the pixels of the up-scaling cases, all 16 at mask_scale 0.5."""
    for name in ("crop_up", "scale2"):
        d = distinct_under(name)
        assert d.max() == 9 and (d == 9).mean() > 0.02, (name, d.max(), (d == 9).mean())
    d = distinct_under("half")
    assert d.max() == 16 and (d == 16).mean() > 0.3, (d.max(), (d == 16).mean())


# ------------------------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize("ib", (1, 2))
def test_scatter_twin_on_the_edge_points(ib):
    H, W = ic.SCATTER_HW
    ys, xs, labels = ic.scatter_points()
    got = io.scatter_twin(ys, xs, labels, ic.LUT, H, W, ib)
    expect = np.zeros((H, W), np.int64)
    expect[1, 0] = 1                                                    # the last LUT slot
    expect[2, 0], expect[2, 1], expect[2, 2], expect[2, 4] = 255, (256 if ib == 2 else 0), (65535 if ib == 2 else 0), 9
    expect[0, W - 1], expect[H - 1, 0], expect[H - 1, W - 1] = 255, 9, (256 if ib == 2 else 0)
    assert np.array_equal(got.astype(np.int64), expect)
    assert not io.scatter_twin(ys[:0], xs[:0], labels[:0], ic.LUT, H, W, ib).any()
    with pytest.raises(AssertionError):
        io.scatter_twin([1, 1], [2, 2], [0, 1], ic.LUT, H, W, ib)


# ------------------------------------------------------------------------------------------------ refusals (before any HIP call)
def test_every_argument_refusal_returns_an_error():
    from stemseg_amd import hip
    l = hip.lib()
    p = C.c_void_p(0x1000)          # never dereferenced: every call below fails its argument check first
    err = lambda: l.stemseg_hip_last_error()
    for ex in (False, True):
        def scatter(ys=p, xs=p, lab=p, n=4, lut=p, lut_len=3, dense=p, H=4, W=4, ib=1):
            if ex:
                return l.stemseg_hip_scatter_instance_index_ex(ys, xs, lab, n, lut, lut_len, dense, ib, H, W, None)
            return l.stemseg_hip_scatter_instance_index(ys, xs, lab, n, lut, lut_len, dense, H, W, None)
        for kw in (dict(dense=None), dict(H=0), dict(W=0), dict(H=-1), dict(n=-1), dict(lut_len=-1)):
            assert scatter(**kw) == -1 and b"bad arguments" in err(), kw
        for kw in (dict(ys=None), dict(xs=None), dict(lab=None), dict(lut=None)):
            assert scatter(**kw) == -1 and b"null pointer" in err(), kw

        def resample(dense=p, h=4, w=4, scale=4.0, ch=8, cw=8, oh=8, ow=8, out=p, ib=1):
            if ex:
                return l.stemseg_hip_resample_instance_masks_ex(dense, ib, h, w, scale, ch, cw, oh, ow, out, None)
            return l.stemseg_hip_resample_instance_masks(dense, h, w, scale, ch, cw, oh, ow, out, None)
        for kw in (dict(dense=None), dict(out=None), dict(h=0), dict(w=0), dict(oh=0), dict(ow=0), dict(scale=0.0), dict(scale=-4.0)):
            assert resample(**kw) == -1 and b"bad arguments" in err(), kw
        for kw in (dict(ch=0), dict(cw=0), dict(ch=17), dict(cw=17), dict(scale=1.0, ch=5), dict(scale=2.0, cw=9), dict(scale=0.2)):
            assert resample(**kw) == -1 and b"padded dims" in err(), kw
    for ib in (0, 3, 4, -1):
        assert l.stemseg_hip_scatter_instance_index_ex(p, p, p, 4, p, 3, p, ib, 4, 4, None) == -1 and b"index_bytes" in err()
        assert l.stemseg_hip_resample_instance_masks_ex(p, ib, 4, 4, 4.0, 8, 8, 8, 8, p, None) == -1 and b"index_bytes" in err()

    f3 = lambda *v: (C.c_float * 3)(*v)
    for masked in (False, True):
        def pre(frames=p, inv=p, T=1, H0=4, W0=4, nh=6, nw=6, ph=8, pw=8, mean=f3(1, 2, 3), std=f3(1, 1, 1), out=p):
            if masked:
                return l.stemseg_hip_preprocess_frames_masked(frames, inv, T, H0, W0, nh, nw, ph, pw, mean, std, 0, 0, out, None)
            return l.stemseg_hip_preprocess_frames(frames, T, H0, W0, nh, nw, ph, pw, mean, std, 0, 0, out, None)
        for kw in (dict(frames=None), dict(out=None), dict(mean=None), dict(std=None)) + ((dict(inv=None),) if masked else ()):
            assert pre(**kw) == -1 and b"null pointer" in err(), kw
        for kw in (dict(T=0), dict(H0=0), dict(W0=0), dict(nh=0), dict(nw=0), dict(ph=5), dict(pw=5)):
            assert pre(**kw) == -1 and b"bad dims" in err(), kw
        for kw in (dict(std=f3(0, 1, 1)), dict(std=f3(1, 0, 1)), dict(std=f3(1, 1, -0.0))):
            assert pre(**kw) == -1 and b"zero std" in err(), kw
