"""CPU tests around the augmentation kernels (csrc/augment.hip): the inputs tests/test_gpu_augment.py uses are pinned and shown, on the
numpy oracle alone, to hold so few elements in the bands of the band rule that the rule cannot hide a wrong kernel; the oracle's own
properties; and the argument errors of every entry point, which return -1 before any HIP call."""
import ctypes as C

import numpy as np
import pytest

from tests import augment_oracle as ao

def exact_ties(soft):
    """Values the oracle has ON k + 0.5 up to its own rounding noise: there fp64 itself goes either way, and so may fp32 -- a rational
    shift such as (2.3, -1.2) makes 2 % of a frame such values, which the cap on differing elements cannot bear."""
    return int((np.abs(soft - np.floor(soft) - 0.5) < 1e-7).sum())


U8_BAND_SHARE = 6e-3      # a band of +-1e-3 around k + 0.5 holds ~2e-3 of arbitrary values (and the zeros outside the frame hold none)


# ------------------------------------------------------------------------------------------------ the band rule on the chosen inputs
def test_warp_cases_hold_few_elements_in_the_bands():
    """Under every warp case the rounding band holds < 0.6 % of the values, and NO pixel has a nearest-pixel or weight-sum tie within the
    band: every plane bit and every invalid bit must be exact, and a kernel wrong on 1 % of the image values fails.  Every case warps
    something out of the frame (or is the single-frame case), sets planes, and leaves most of the frame valid."""
    names = set()
    for name, src, pl, hm, jt in ao.warp_cases():
        ref = ao.warp_clip(src, pl, hm, jt)
        share = float(ao.u8_band(ref["soft"]).mean())
        assert share < U8_BAND_SHARE, (name, share)
        assert exact_ties(ref["soft"]) == 0, name
        assert not ao.weight_band(ref["weight"]).any() and not ref["near_coord"].any(), name
        assert 0.0 <= ref["invalid"].mean() < 0.2, name
        assert (ref["invalid"].mean() > 0.01) == (hm.shape[0] == 7), name
        if pl is not None and pl.shape[0] > 1:
            assert ((pl != 0).sum(0) > 1).sum() >= 20, "%s: the planes must overlap" % name
        if pl is not None:
            assert ref["planes"].any(axis=(2, 3)).sum() >= min(pl.shape[0], 3) * hm.shape[0] // 2, name
            assert (ref["planes"].sum(0) <= 1).all()
        assert (ref["frames"] != src[None]).mean() > 0.5, name
        names.add(name)
    assert len(names) == 15
    assert {c[2].shape[0] if c[2] is not None else 0 for c in ao.warp_cases()} == {0, 1, 3, 127}
    assert {c[3].shape[0] for c in ao.warp_cases()} == {1, 7}


def test_exact_case_planes_overlap():
    for H, W in ao.WARP_SHAPES:
        for N, seed in ((3, 2), (127, 2), (3, 4)):
            assert ((ao.planes(N, H, W, seed) != 0).sum(0) > 1).sum() >= 20, (H, W, N, seed)


def test_pole_case_is_outside_by_the_rule_on_the_right_half():
    H, W = 45, 40
    u, v, inside = ao.source_coords(ao.crossing_denominator(H, W), H, W)
    assert not inside[:, W // 2:].any() and inside[:H // 2, 0].all()
    ref = ao.warp_clip(ao.image(H, W, 5), ao.planes(3, H, W, 6), ao.crossing_denominator(H, W)[None])
    assert not ao.weight_band(ref["weight"]).any() and not ref["near_coord"].any()


def test_blur_and_duplicate_cases_hold_few_elements_in_the_bands():
    for name, frames, matrices in ao.blur_cases():
        ref, soft = ao.motion_blur(frames, matrices)
        assert float(ao.u8_band(soft).mean()) < U8_BAND_SHARE and exact_ties(soft) == 0, name
        assert (ref != frames).mean() > 0.5, name
        for m in matrices:
            assert m is None or (abs(float(m.sum()) - 1) < 1e-6 and m.shape[0] in (7, 9, 11))
    kinds = set()
    for name, frames, mask, boxes, flip, shifts in ao.duplicate_cases():
        ref = ao.duplicate_instance(frames, mask, boxes, flip, shifts)
        assert float(ao.u8_band(ref["soft"]).mean()) < U8_BAND_SHARE and not ao.weight_band(ref["weight"]).any(), name
        assert exact_ties(ref["soft"]) <= 1, name
        assert ref["pasted"].sum() > 100 and ref["masks"][0].sum() > 100, name
        H, W = mask.shape[1:]
        b = [x for x in boxes if x is not None][0]
        kinds |= {k for k, hit in (("left", b[0] == 0), ("top", b[1] == 0), ("right", b[2] == W), ("bottom", b[3] == H), ("flip", flip),
                                   ("no flip", not flip), ("no box", None in boxes),
                                   ("fraction", shifts[0][0] != int(shifts[0][0])), ("integer", shifts[0][0] == int(shifts[0][0]))) if hit}
    assert kinds == {"left", "top", "right", "bottom", "flip", "no flip", "no box", "fraction", "integer"}


def test_band_checks_refuse_what_they_should():
    soft = np.array([[10.2, 10.4995, 20.7]])
    ref = ao.round_u8(soft)
    assert ao.check_u8(ref, ref, soft) == 0
    with pytest.raises(AssertionError):
        ao.check_u8(ref + np.array([[1, 0, 0]], np.uint8), ref, soft)              # away from the band
    with pytest.raises(AssertionError):
        ao.check_u8(ref + np.array([[0, 2, 0]], np.uint8), ref, soft)              # in the band, but by two
    with pytest.raises(AssertionError):
        ao.check_u8(ref + np.array([[0, 1, 0]], np.uint8), ref, soft)              # in the band, but a third of the elements
    big = np.full((1, 2000), 10.2)
    big[0, 0] = 10.4995
    got = ao.round_u8(big)
    got[0, 0] += 1
    assert ao.check_u8(got, ao.round_u8(big), big) == 1
    bits = np.zeros((1, 2000), np.uint8)
    flipped = bits.copy()
    flipped[0, 3] = 1
    band = np.zeros((1, 2000), bool)
    with pytest.raises(AssertionError):
        ao.check_bits(flipped, bits, band)
    band[0, 3] = True
    assert ao.check_bits(flipped, bits, band) == 1


# ------------------------------------------------------------------------------------------------ the oracle's own properties
def test_jitter_oracle_properties():
    rng = np.random.RandomState(0)
    px = rng.randint(0, 256, (5000, 3)).astype(np.uint8)
    assert np.array_equal(ao.jitter(px, 40, 7, 0), px)
    assert np.array_equal(ao.jitter(px, 40, 7, ao.JITTER_ADD), np.clip(px.astype(int) + 40, 0, 255))
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    assert np.array_equal(ao.jitter(grey, 0, -15, ao.JITTER_HUE_SAT), grey)         # no saturation to take away: grey stays grey
    back = ao.jitter(px, 0, 0, ao.JITTER_HUE_SAT).astype(int)                        # the 8-bit HSV round trip moves a channel by a few levels
    assert np.abs(back - px).max() <= 4
    red = np.array([[0, 0, 200]], np.uint8)
    assert ao.jitter(red, 0, 85, ao.JITTER_HUE_SAT)[0].argmax() == 1                 # + trunc(85 * 180 / 255) = 60 hue steps = 120 degrees: red -> green
    assert np.array_equal(ao.jitter(px, 10, 3, 3), ao.jitter(ao.jitter(px, 10, 3, ao.JITTER_ADD), 10, 3, ao.JITTER_HUE_SAT))


def test_warp_oracle_identity_and_homography():
    H, W = 21, 30
    src, pl = ao.image(H, W, 0), ao.planes(3, H, W, 1)
    ref = ao.warp_clip(src, pl, ao.identity()[None])
    assert np.array_equal(ref["frames"][0], src) and not ref["invalid"].any()
    assert np.array_equal(ref["planes"][2, 0], (pl[2] != 0)) and np.array_equal(ref["planes"][0, 0], (pl[0] != 0) & (pl[1] == 0) & (pl[2] == 0))
    pts, dst = [(0, 0), (W - 1, 0), (W - 1, H - 1), (0, H - 1)], [(2, 1), (W - 3, 2), (W - 2, H - 4), (1, H - 2)]
    m = ao.homography(pts, dst)
    for (x, y), (X, Y) in zip(pts, dst):
        q = m @ [x, y, 1]
        assert abs(q[0] / q[2] - X) < 1e-9 and abs(q[1] / q[2] - Y) < 1e-9


# ------------------------------------------------------------------------------------------------ argument errors: -1 before any HIP call
@pytest.fixture(scope="module")
def lib():
    from stemseg_amd import hip
    return hip.lib()


def _last(lib):
    return lib.stemseg_hip_last_error().decode()


FAKE = C.c_void_p(0x1000)


def test_warp_clip_argument_errors(lib):
    def call(src=FAKE, planes=FAKE, N=3, H=8, W=8, hinv=FAKE, jitter=FAKE, F=2, frames=FAKE, out_planes=FAKE, invalid=FAKE):
        return lib.stemseg_hip_warp_clip(src, planes, N, H, W, hinv, jitter, F, frames, out_planes, invalid, None)
    for kw, word in ((dict(src=None), "null"), (dict(planes=None), "null"), (dict(out_planes=None), "null"), (dict(hinv=None), "null"),
                     (dict(jitter=None), "null"), (dict(frames=None), "null"), (dict(invalid=None), "null"), (dict(N=-1), "bad dims"),
                     (dict(N=128), "bad dims"), (dict(H=0), "bad dims"), (dict(W=0), "bad dims"), (dict(F=0), "bad dims"),
                     (dict(H=65536, W=32768), "2^31"), (dict(hinv=C.c_void_p(0x1004)), "aligned"), (dict(jitter=C.c_void_p(0x1002)), "aligned")):
        assert call(**kw) == -1, kw
        assert word in _last(lib), (kw, _last(lib))


def test_motion_blur_argument_errors(lib):
    def ks(*v):
        return (C.c_int32 * len(v))(*v)

    def call(frames=FAKE, F=2, H=8, W=8, ksize_host=ks(7, 0), taps=FAKE, out=C.c_void_p(0x2000)):
        return lib.stemseg_hip_motion_blur(frames, F, H, W, ksize_host, taps, out, None)
    for kw, word in ((dict(frames=None), "null"), (dict(ksize_host=None), "null"), (dict(taps=None), "null"),
                     (dict(F=129, ksize_host=ks(*([0] * 129))), "at most 128"),
                     (dict(out=None), "null"), (dict(out=FAKE), "another buffer"), (dict(F=0), "bad dims"), (dict(H=0), "bad dims"),
                     (dict(H=65536, W=32768), "2^31"), (dict(ksize_host=ks(7, 8)), "kernel size 8"), (dict(ksize_host=ks(-1, 0)), "kernel size -1"),
                     (dict(ksize_host=ks(13, 0)), "kernel size 13"), (dict(ksize_host=ks(0, 11), W=5), "reflected"),
                     (dict(ksize_host=ks(9, 0), H=4), "reflected"), (dict(taps=C.c_void_p(0x1002)), "misaligned")):
        assert call(**kw) == -1, kw
        assert word in _last(lib), (kw, _last(lib))


def test_duplicate_instance_and_masked_preprocess_argument_errors(lib):
    out, out2 = C.c_void_p(0x2000), C.c_void_p(0x3000)

    def call(frames=FAKE, mask=FAKE, T=2, H=8, W=8, params=FAKE, frames_out=out, masks_out=out2):
        return lib.stemseg_hip_duplicate_instance(frames, mask, T, H, W, params, frames_out, masks_out, None)
    for kw, word in ((dict(frames=None), "null"), (dict(mask=None), "null"), (dict(params=None), "null"), (dict(frames_out=None), "null"),
                     (dict(masks_out=None), "null"), (dict(frames_out=FAKE), "other buffers"), (dict(masks_out=FAKE), "other buffers"),
                     (dict(T=0), "bad dims"), (dict(W=0), "bad dims"), (dict(H=65536, W=32768), "2^31"), (dict(params=C.c_void_p(0x1001)), "misaligned")):
        assert call(**kw) == -1, kw
        assert word in _last(lib), (kw, _last(lib))
    three = (C.c_float * 3)(1, 1, 1)

    def pre(frames=FAKE, invalid=FAKE, T=2, H0=8, W0=8, nh=4, nw=4, ph=32, pw=32, mean=three, std=three, o=out):
        return lib.stemseg_hip_preprocess_frames_masked(frames, invalid, T, H0, W0, nh, nw, ph, pw, mean, std, 0, 0, o, None)
    for kw, word in ((dict(frames=None), "null"), (dict(invalid=None), "null"), (dict(o=None), "null"), (dict(T=0), "bad dims"), (dict(ph=3), "bad dims"),
                     (dict(std=(C.c_float * 3)(1, 0, 1)), "zero std")):
        assert pre(**kw) == -1, kw
        assert word in _last(lib), (kw, _last(lib))
