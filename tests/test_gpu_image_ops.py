"""GPU tests of csrc/image_ops.hip (on csrc/bilinear.h): pre-processing, masked pre-processing, the instance-index scatter and the
mask resampling, on the inputs of tests/image_ops_cases.py -- uint8 noise frames, every edge of the resize (identity, in_size == 1,
up, down, pad equal to the size), mask_scale 0.5, 1, 2 and 4, crops inside the up-sampled map, both index widths up to 65535, and
one size per kernel above its launch cap, so that the grid-stride loops run.

Each result is held to two things.  The float32 TWIN of tests/image_ops_oracle.py (the arithmetic the sources spell out, one rounding
per operation and an fma where `fmaf` is written; for the masks the reference's K whole planes, not the kernel's 16 source pixels) with np.array_equal: no tolerance, no
threshold band.  And the float64 EXACT form in the reference's order of operations under the derived bounds of that module,
|got - exact| <= (3 (H0 + W0) + 16) 2^-24 S_c per channel and, for the masks, equality wherever no exact plane lies within
(3 (h + w + crop_h + crop_w) + 8) 2^-24 of 0.5 with at most 3 % of the pixels there -- so the kernels stay tied to float64 even
if a twin comparison ever has to go.  Outputs the tests can reach are pre-filled with 0xFF bytes (NaN as float32), so an element
a kernel does not write shows; one case of each kernel goes through the C ABI between canary blocks.

Why the older tests (test_preprocess_frames_vs_golden_and_oracle, test_masked_preprocess) carry 1e-4 and the mask tests a band of
1e-6: their reference is torch's CPU float32 F.interpolate, which evaluates the source index scale * (dst + 0.5) - 0.5 as one fma.
On random uint8 frames at 720 x 1280 -> 480 x 853, in 0..255 units, a float32 restatement that rounds every operation differs from
torch by up to 7.2e-3, one with only that expression fused agrees with torch to 3e-5, and both are 1.78e-2 from float64.  The kernels
fuse it as torch does (csrc/bilinear.h writes the fmas out; they used to arise from the compiler's contraction of __fmul_rn /
__fadd_rn): with every operation rounded the device passes this file against a twin that rounds likewise, but misses those older tests
(8e-4 and 2.9e-4 against 1e-4, 0.5 % of the mask pixels against 0.1 %), so the fused index is the arithmetic the suite pins.

Measured: on the host (tests/test_image_ops_host.py) the twins reach at most 0.192 of the pre-processing bound (0.120 masked), at most
1.64 % of a mask run's pixels lie in the band, and the twin differs from the exact form nowhere outside it.  On an MI355X the device
equals the twin in every element of all 114 tests and so reaches the same 0.192 of the bound.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import image_ops_cases as ic
from tests import image_ops_oracle as io
from tests.test_gpu_augment import Guarded, all_intact

pytestmark = pytest.mark.gpu
NP_INDEX = {1: np.uint8, 2: np.uint16}


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def dev(a):
    """A (read-only) numpy array on the device; a uint16 map travels as int16 bits."""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def poison(nbytes):
    """Best effort for outputs the binding allocates itself: leave a freed block of 0xFF bytes (NaN as float32) of the size about to be
    asked for, which the caching allocator hands out next.  (The C-ABI tests below pre-fill their outputs for certain.)"""
    torch.cuda.synchronize()
    t = torch.full((int(nbytes),), 0xFF, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    del t


def f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


# ------------------------------------------------------------------------------------------------ pre-processing
@pytest.mark.parametrize("params", ic.PARAM_SETS, ids=[p[0] for p in ic.PARAM_SETS])
@pytest.mark.parametrize("case", ic.PRE_CASES, ids=[c[0] for c in ic.PRE_CASES])
def test_preprocess_vs_twin_and_exact(hip, case, params):
    name, (H0, W0), new_hw, pad_hw, T = case
    _, mean, std, unit, flip = params
    fr = ic.frames(name)
    poison(T * 3 * pad_hw[0] * pad_hw[1] * 4)
    got = host(hip.preprocess_frames(dev(fr), new_hw, pad_hw, mean, std, unit, flip))
    assert not np.isnan(got).any(), "an output element was not written"
    share = io.check_preprocess(got, io.preprocess_exact(fr, None, new_hw, pad_hw, mean, std, unit, flip), new_hw,
                                io.preprocess_bound(H0, W0, std, unit, flip), name)
    twin = io.preprocess_twin(fr, None, new_hw, pad_hw, mean, std, unit, flip)
    print("%s / %s: max |device - exact| = %.3f of the bound, %d elements differ from the twin" % (name, params[0], share, int((got != twin).sum())))
    assert np.array_equal(got, twin)


@pytest.mark.parametrize("params", ic.PARAM_SETS, ids=[p[0] for p in ic.PARAM_SETS])
@pytest.mark.parametrize("pattern", ic.INVALID_PATTERNS)
@pytest.mark.parametrize("case", ic.MASKED_CASES, ids=[c[0] for c in ic.MASKED_CASES])
def test_masked_preprocess_vs_twin_and_exact(hip, case, pattern, params):
    """Also: nothing invalid gives the bits of the unmasked call, on noise frames."""
    name, (H0, W0), new_hw, pad_hw, T = case
    _, mean, std, unit, flip = params
    fr, inv = ic.frames(name), ic.invalid(name, pattern)
    poison(T * 3 * pad_hw[0] * pad_hw[1] * 4)
    out = hip.preprocess_frames(dev(fr), new_hw, pad_hw, mean, std, unit, flip, invalid=dev(inv))
    got = host(out)
    assert not np.isnan(got).any(), "an output element was not written"
    share = io.check_preprocess(got, io.preprocess_exact(fr, inv, new_hw, pad_hw, mean, std, unit, flip), new_hw,
                                io.preprocess_bound(H0, W0, std, unit, flip), name + " " + pattern)
    twin = io.preprocess_twin(fr, inv, new_hw, pad_hw, mean, std, unit, flip)
    print("%s / %s / %s: max |device - exact| = %.3f of the bound, %d elements differ from the twin"
          % (name, pattern, params[0], share, int((got != twin).sum())))
    assert np.array_equal(got, twin)
    if pattern == "none":
        assert torch.equal(out, hip.preprocess_frames(dev(fr), new_hw, pad_hw, mean, std, unit, flip))


@pytest.mark.parametrize("masked", (False, True))
def test_preprocess_c_abi_between_canaries(hip, masked):
    name, (H0, W0), (nh, nw), (ph, pw), T = ic.PRE_CASES[1]
    _, mean, std, unit, flip = ic.PARAM_SETS[2]
    fr, inv = ic.frames(name), ic.invalid(name, "random30")
    g_in, g_inv, g_out = Guarded.of(fr), Guarded.of(inv), Guarded(T * 3 * ph * pw * 4, fill=0xFF)
    l = hip.lib()
    if masked:
        rc = l.stemseg_hip_preprocess_frames_masked(g_in.ptr(), g_inv.ptr(), T, H0, W0, nh, nw, ph, pw, f3(mean), f3(std), int(unit), int(flip),
                                                    g_out.ptr(), hip.stream())
    else:
        rc = l.stemseg_hip_preprocess_frames(g_in.ptr(), T, H0, W0, nh, nw, ph, pw, f3(mean), f3(std), int(unit), int(flip), g_out.ptr(), hip.stream())
    assert rc == 0, l.stemseg_hip_last_error().decode()
    all_intact(frames=g_in, invalid=g_inv, out=g_out)
    got = g_out.numpy((T, 3, ph, pw), np.float32)
    assert not np.isnan(got).any(), "an output element was not written"
    assert np.array_equal(got, io.preprocess_twin(fr, inv if masked else None, (nh, nw), (ph, pw), mean, std, unit, flip))
    assert np.array_equal(g_in.numpy(fr.shape), fr) and np.array_equal(g_inv.numpy(inv.shape), inv)


# ------------------------------------------------------------------------------------------------ mask resampling
@pytest.mark.parametrize("run", ic.MASK_RUNS, ids=["%s-%s-%d" % r for r in ic.MASK_RUNS])
def test_resample_vs_twin_and_exact(hip, run):
    name, layout, ib = run
    _, (h, w), scale, crop_hw, out_hw = ic.mask_case(name)
    dense = ic.dense_map(name, layout, ib)
    poison(out_hw[0] * out_hw[1] * ib)
    got = host(hip.resample_instance_masks_ex(dev(dense), scale, crop_hw, out_hw, ib))
    assert got.dtype == NP_INDEX[ib] and got.shape == tuple(out_hw)
    idx, exact = io.soft_masks_exact(dense, scale, crop_hw, out_hw)
    share, wrong = io.check_masks(got, idx, exact, io.mask_band(h, w, crop_hw), "%s %s %d" % run)
    twin = io.masks_twin(dense, scale, crop_hw, out_hw)
    print("%s / %s / width %d: %.4f of the pixels in the band, %d differ from the exact form there, %d differ from the twin"
          % (name, layout, ib, share, wrong, int((got != twin).sum())))
    assert np.array_equal(got, twin)
    if ib == 1:             # the ABI <= 10 entry point is the same kernel
        poison(out_hw[0] * out_hw[1])
        assert np.array_equal(host(hip.resample_instance_masks(dev(dense), scale, crop_hw, out_hw)), twin)


def test_resample_c_abi_between_canaries(hip):
    name, layout, ib = "crop_up", "all_different", 2
    _, (h, w), scale, (ch, cw), (oh, ow) = ic.mask_case(name)
    dense = ic.dense_map(name, layout, ib)
    g_in, g_out = Guarded.of(dense), Guarded(oh * ow * ib, fill=0xFF)
    l = hip.lib()
    rc = l.stemseg_hip_resample_instance_masks_ex(g_in.ptr(), ib, h, w, scale, ch, cw, oh, ow, g_out.ptr(), hip.stream())
    assert rc == 0, l.stemseg_hip_last_error().decode()
    all_intact(dense=g_in, out=g_out)
    twin = io.masks_twin(dense, scale, (ch, cw), (oh, ow))
    assert 0 < (twin == 65535).sum() < twin.size, "0xFFFF is an index of this case: the pre-fill must not explain it"
    assert np.array_equal(g_out.numpy((oh, ow), np.uint16), twin) and np.array_equal(g_in.numpy((h, w), np.uint16), dense)


# ------------------------------------------------------------------------------------------------ scatter
def scatter_inputs(which):
    if which == "edges":
        return ic.SCATTER_HW, ic.scatter_points()
    if which == "empty":
        return ic.SCATTER_HW, tuple(a[:0] for a in ic.scatter_points())
    return ic.SCATTER_BIG_HW, ic.scatter_big()


@pytest.mark.parametrize("ib", (1, 2))
@pytest.mark.parametrize("which", ("edges", "empty", "stride"))
def test_scatter_vs_twin(hip, which, ib):
    """Through the binding and through the C ABI between canaries, the map pre-filled with 0xFF: the zeroing reaches every pixel."""
    (H, W), (ys, xs, labels) = scatter_inputs(which)
    lut = np.array(ic.LUT, np.int32)
    twin = io.scatter_twin(ys, xs, labels, lut, H, W, ib)
    assert which == "empty" or 0 < (twin != 0).mean() < 1
    poison(H * W * ib)
    got = host(hip.scatter_instance_index_ex(dev(ys), dev(xs), dev(labels), dev(lut), H, W, ib))
    assert got.dtype == NP_INDEX[ib] and np.array_equal(got, twin)
    if ib == 1:
        poison(H * W)
        assert np.array_equal(host(hip.scatter_instance_index(dev(ys), dev(xs), dev(labels), dev(lut), H, W)), twin)
    n = len(ys)
    g_y, g_x, g_l, g_lut, g_out = Guarded.of(ys), Guarded.of(xs), Guarded.of(labels), Guarded.of(lut), Guarded(H * W * ib, fill=0xFF)
    l = hip.lib()
    rc = l.stemseg_hip_scatter_instance_index_ex(g_y.ptr(), g_x.ptr(), g_l.ptr(), n, g_lut.ptr(), len(lut), g_out.ptr(), ib, H, W, hip.stream())
    assert rc == 0, l.stemseg_hip_last_error().decode()
    all_intact(ys=g_y, xs=g_x, labels=g_l, lut=g_lut, dense=g_out)
    assert np.array_equal(g_out.numpy((H, W), NP_INDEX[ib]), twin)


def test_scatter_then_resample_chain(hip):
    """The two kernels as the writers chain them: a 16-bit map scattered from points, resampled, against the twins of both."""
    name, (h, w), scale, crop_hw, out_hw = ic.MASK_CASES[1]
    want = ic.dense_map(name, "rectangles", 2)
    ys, xs = np.nonzero(want)
    vals = np.unique(want)
    lut = np.concatenate([[0], vals[vals != 0]]).astype(np.int32)               # label k -> slot k + 1 -> the k-th index
    labels = (np.searchsorted(lut[1:], want[ys, xs])).astype(np.int64)
    d = hip.scatter_instance_index_ex(dev(ys.astype(np.int64)), dev(xs.astype(np.int64)), dev(labels), dev(lut), h, w, 2)
    assert np.array_equal(host(d), want)
    assert np.array_equal(host(hip.resample_instance_masks_ex(d, scale, crop_hw, out_hw, 2)), io.masks_twin(want, scale, crop_hw, out_hw))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_an_error_and_write_nothing(hip):
    l = hip.lib()
    name, (H0, W0), (nh, nw), (ph, pw), T = ic.PRE_CASES[1]
    fr, inv = ic.frames(name), ic.invalid(name, "random30")
    g_in, g_inv, g_out = Guarded.of(fr), Guarded.of(inv), Guarded(T * 3 * ph * pw * 4, fill=0x5A)
    mean, one = f3(ic.CAFFE_MEAN), f3((1, 1, 1))
    for masked in (False, True):
        def pre(nh=nh, nw=nw, ph=ph, pw=pw, std=one):
            if masked:
                return l.stemseg_hip_preprocess_frames_masked(g_in.ptr(), g_inv.ptr(), T, H0, W0, nh, nw, ph, pw, mean, std, 0, 0, g_out.ptr(), hip.stream())
            return l.stemseg_hip_preprocess_frames(g_in.ptr(), T, H0, W0, nh, nw, ph, pw, mean, std, 0, 0, g_out.ptr(), hip.stream())
        for c in range(3):
            assert pre(std=f3([0.0 if k == c else 1.0 for k in range(3)])) == -1 and b"zero std" in l.stemseg_hip_last_error()
        assert pre(ph=nh - 1) == -1 and b"bad dims" in l.stemseg_hip_last_error()
        assert pre(pw=nw - 1) == -1 and b"bad dims" in l.stemseg_hip_last_error()
    all_intact(frames=g_in, invalid=g_inv, out=g_out)
    assert (g_out.view == 0x5A).all()

    _, (h, w), scale, (ch, cw), (oh, ow) = ic.MASK_CASES[0]
    dense = ic.dense_map("same", "rectangles", 1)
    g_d, g_o = Guarded.of(dense), Guarded(oh * ow * 2, fill=0x5A)
    assert l.stemseg_hip_resample_instance_masks(g_d.ptr(), h, w, scale, ch + 1, cw, oh, ow, g_o.ptr(), hip.stream()) == -1
    assert b"padded dims" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_resample_instance_masks_ex(g_d.ptr(), 1, h, w, scale, ch, cw + 1, oh, ow, g_o.ptr(), hip.stream()) == -1
    assert b"padded dims" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_resample_instance_masks_ex(g_d.ptr(), 2, h, w, 1.0, h + 1, w, oh, ow, g_o.ptr(), hip.stream()) == -1
    assert b"padded dims" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_resample_instance_masks_ex(g_d.ptr(), 3, h, w, scale, ch, cw, oh, ow, g_o.ptr(), hip.stream()) == -1
    assert b"index_bytes" in l.stemseg_hip_last_error()
    all_intact(dense=g_d, out=g_o)
    assert (g_o.view == 0x5A).all()

    (H, W), (ys, xs, labels) = ic.SCATTER_HW, ic.scatter_points()
    g_y, g_x, g_l, g_lut, g_m = Guarded.of(ys), Guarded.of(xs), Guarded.of(labels), Guarded.of(np.array(ic.LUT, np.int32)), Guarded(H * W * 4, fill=0x5A)
    n = len(ys)
    for ib in (0, 3, 4):
        assert l.stemseg_hip_scatter_instance_index_ex(g_y.ptr(), g_x.ptr(), g_l.ptr(), n, g_lut.ptr(), len(ic.LUT), g_m.ptr(), ib, H, W, hip.stream()) == -1
        assert b"index_bytes" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_scatter_instance_index_ex(g_y.ptr(), g_x.ptr(), None, n, g_lut.ptr(), len(ic.LUT), g_m.ptr(), 2, H, W, hip.stream()) == -1
    assert l.stemseg_hip_scatter_instance_index(g_y.ptr(), g_x.ptr(), g_l.ptr(), -1, g_lut.ptr(), len(ic.LUT), g_m.ptr(), H, W, hip.stream()) == -1
    assert l.stemseg_hip_scatter_instance_index(g_y.ptr(), g_x.ptr(), g_l.ptr(), n, g_lut.ptr(), len(ic.LUT), g_m.ptr(), 0, W, hip.stream()) == -1
    all_intact(ys=g_y, xs=g_x, labels=g_l, lut=g_lut, dense=g_m)
    assert (g_m.view == 0x5A).all()
