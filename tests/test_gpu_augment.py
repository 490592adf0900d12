"""GPU tests of the augmentation kernels (csrc/augment.hip) and the masked pre-processing, through the C-ABI, against the numpy
restatement in tests/augment_oracle.py under its band rule (tests/test_augment_host.py shows how few elements the bands hold for these
very inputs).  Every kernel output sits between canary blocks, which are checked."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import augment_oracle as ao

pytestmark = pytest.mark.gpu
GUARD = 4096
CANARY = 0xA5


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


class Guarded(object):
    """``nbytes`` of device memory between two canary blocks (8-byte aligned payload); ``fill``: what the payload holds before the call."""

    def __init__(self, nbytes, fill=0x5A):
        self.nbytes = int(nbytes)
        self.buf = torch.full((max(self.nbytes, 1) + 2 * GUARD,), CANARY, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.nbytes]
        self.view.fill_(fill)

    @classmethod
    def of(cls, array):
        a = np.ascontiguousarray(array)
        g = cls(a.nbytes)
        if a.nbytes:
            g.view.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
        return g

    def ptr(self):
        return C.c_void_p(self.view.data_ptr()) if self.nbytes else None

    def numpy(self, shape, dtype=np.uint8):
        return self.view.cpu().numpy().view(dtype).reshape(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == CANARY).all()) and bool((self.buf[GUARD + max(self.nbytes, 1):] == CANARY).all())


def all_intact(**guards):
    torch.cuda.synchronize()
    for name, g in guards.items():
        assert g.intact(), "a canary around %s was overwritten" % name


def warp_guarded(hip, src, planes, hinv, jit=None):
    """``stemseg_hip_warp_clip`` with every buffer between canaries -> (frames, out_planes, invalid) numpy."""
    H, W = src.shape[:2]
    hm = np.ascontiguousarray(hinv, np.float64).reshape(-1, 9)
    F = hm.shape[0]
    jt = np.zeros((F, 3), np.int32) if jit is None else np.ascontiguousarray(jit, np.int32).reshape(F, 3)
    N = 0 if planes is None else planes.shape[0]
    g_src, g_pl, g_h, g_j = Guarded.of(src), Guarded.of(planes if N else np.zeros(0, np.uint8)), Guarded.of(hm), Guarded.of(jt)
    g_fr, g_op, g_inv = Guarded(F * H * W * 3), Guarded(N * F * H * W), Guarded(F * H * W)
    rc = hip.lib().stemseg_hip_warp_clip(g_src.ptr(), g_pl.ptr(), N, H, W, g_h.ptr(), g_j.ptr(), F, g_fr.ptr(), g_op.ptr(), g_inv.ptr(), hip.stream())
    assert rc == 0, hip.lib().stemseg_hip_last_error().decode()
    all_intact(src=g_src, planes=g_pl, hinv=g_h, jitter=g_j, frames=g_fr, out_planes=g_op, invalid=g_inv)
    return g_fr.numpy((F, H, W, 3)), g_op.numpy((N, F, H, W)), g_inv.numpy((F, H, W))


def blur_guarded(hip, frames, matrices):
    F, H, W = frames.shape[:3]
    ks = np.array([0 if m is None else m.shape[0] for m in matrices], np.int32)
    taps = np.zeros((F, hip.BLUR_MAX_K ** 2), np.float32)
    for f, m in enumerate(matrices):
        if m is not None:
            taps[f, :m.size] = np.asarray(m, np.float32).reshape(-1)
    g_in, g_t, g_out = Guarded.of(frames), Guarded.of(taps), Guarded(frames.nbytes)
    rc = hip.lib().stemseg_hip_motion_blur(g_in.ptr(), F, H, W, ks.ctypes.data_as(C.c_void_p), g_t.ptr(), g_out.ptr(), hip.stream())
    assert rc == 0, hip.lib().stemseg_hip_last_error().decode()
    all_intact(frames=g_in, taps=g_t, out=g_out)
    return g_out.numpy(frames.shape)


def duplicate_guarded(hip, frames, mask, boxes, flip, shifts):
    T, H, W = mask.shape
    g_in, g_m, g_p = Guarded.of(frames), Guarded.of(mask), Guarded.of(hip.duplicate_params(boxes, flip, shifts))
    g_fo, g_mo = Guarded(frames.nbytes), Guarded(2 * mask.nbytes)
    rc = hip.lib().stemseg_hip_duplicate_instance(g_in.ptr(), g_m.ptr(), T, H, W, g_p.ptr(), g_fo.ptr(), g_mo.ptr(), hip.stream())
    assert rc == 0, hip.lib().stemseg_hip_last_error().decode()
    all_intact(frames=g_in, mask=g_m, params=g_p, frames_out=g_fo, masks_out=g_mo)
    return g_fo.numpy(frames.shape), g_mo.numpy((2, T, H, W))


# ------------------------------------------------------------------------------------------------ warp_clip
@pytest.mark.parametrize("shape", ao.WARP_SHAPES)
@pytest.mark.parametrize("N", (0, 1, 3, 127))
def test_warp_identity_is_exact(hip, shape, N):
    """Frames equal to the source, nothing invalid, planes equal to the condensed expansion, bit for bit; F = 1."""
    H, W = shape
    src, pl = ao.image(H, W, 1), ao.planes(N, H, W, 2) if N else None
    frames, out_planes, invalid = warp_guarded(hip, src, pl, ao.identity()[None])
    assert np.array_equal(frames[0], src) and not invalid.any()
    if N:
        yy, xx = np.mgrid[0:H, 0:W]
        expect = ao.condense_expand(pl, yy, xx, np.ones((H, W), bool))
        assert np.array_equal(out_planes[:, 0], expect)
        assert N == 1 or (pl != 0).sum(0).max() > 1, "the planes must overlap"
        assert (out_planes[:, 0].sum(0) <= 1).all()


@pytest.mark.parametrize("shape", ao.WARP_SHAPES)
def test_warp_integer_translations_and_mirror_are_exact(hip, shape):
    """Shifts by whole pixels and a mirror, seven frames in one call: the content moves exactly, the uncovered strip is zero and invalid."""
    H, W = shape
    src, pl = ao.image(H, W, 3), ao.planes(3, H, W, 4)
    shifts = [(5, 0), (-4, 0), (0, 6), (0, -3), (7, -2), (-W, 0)]
    frames, out_planes, invalid = warp_guarded(hip, src, pl, np.stack([ao.translation(tx, ty) for tx, ty in shifts] + [ao.mirror(W)]))
    yy, xx = np.mgrid[0:H, 0:W]
    cond = ao.condense_expand(pl, yy, xx, np.ones((H, W), bool))
    for f, (tx, ty) in enumerate(shifts):
        exp_img, exp_inv, exp_pl = np.zeros_like(src), np.ones((H, W), np.uint8), np.zeros_like(cond)
        ys, xs = slice(max(ty, 0), min(H + ty, H)), slice(max(tx, 0), min(W + tx, W))
        ys0, xs0 = slice(max(-ty, 0), min(H - ty, H)), slice(max(-tx, 0), min(W - tx, W))
        exp_img[ys, xs], exp_inv[ys, xs], exp_pl[:, ys, xs] = src[ys0, xs0], 0, cond[:, ys0, xs0]
        assert np.array_equal(frames[f], exp_img) and np.array_equal(invalid[f], exp_inv) and np.array_equal(out_planes[:, f], exp_pl), (tx, ty)
    assert invalid[5].all() and not frames[5].any()
    assert np.array_equal(frames[6], src[:, ::-1]) and not invalid[6].any() and np.array_equal(out_planes[:, 6], cond[:, :, ::-1])


WARP_CASES = ao.warp_cases()


@pytest.mark.parametrize("case", WARP_CASES, ids=[c[0] for c in WARP_CASES])
def test_warp_rotations_perspectives_and_jitter_within_the_band(hip, case):
    """Rotations of +-12 degrees, random perspectives at magnitude 0.08 and 0.12 and a fractional shift, each frame under another jitter."""
    name, src, pl, hm, jt = case
    ref = ao.warp_clip(src, pl, hm, jt)
    ao.check_warp(*warp_guarded(hip, src, pl, hm, jt), ref, name)
    assert ref["invalid"].any() or hm.shape[0] == 1


def test_warp_denominator_crossing_zero(hip):
    """d = 1 - 2 x / W - y / 1000: from the middle column on the pixels are outside by the rule -- zero, invalid, no plane -- and nothing is
    written out of bounds for the huge coordinates next to the pole."""
    H, W = 45, 40
    src, pl = ao.image(H, W, 5), ao.planes(3, H, W, 6)
    hm = ao.crossing_denominator(H, W)[None]
    ref = ao.warp_clip(src, pl, hm)
    frames, out_planes, invalid = warp_guarded(hip, src, pl, hm)
    ao.check_warp(frames, out_planes, invalid, ref, "pole")
    assert invalid[0, :, W // 2:].all() and not frames[0, :, W // 2:].any() and not out_planes[:, 0, :, W // 2:].any()
    assert not invalid[0, :, :W // 4].all()


@pytest.mark.parametrize("N", (0, 3))
def test_warp_frames_do_not_leak_into_each_other(hip, N):
    """Seven frames with distinct parameters in one call equal seven single-frame calls."""
    H, W = 37, 53
    src, pl = ao.image(H, W, 7), ao.planes(N, H, W, 8) if N else None
    hm, jt = np.stack(ao.general_warps(H, W)), np.asarray(ao.JITTERS, np.int32)
    frames, out_planes, invalid = [torch.from_numpy(a.copy()) for a in warp_guarded(hip, src, pl, hm, jt)]
    for f in range(7):
        one = [torch.from_numpy(a.copy()) for a in warp_guarded(hip, src, pl, hm[f:f + 1], jt[f:f + 1])]
        assert torch.equal(one[0][0], frames[f]) and torch.equal(one[2][0], invalid[f]) and torch.equal(one[1][:, 0], out_planes[:, f]), f
    assert len({frames[f].numpy().tobytes() for f in range(7)}) == 7


def test_warp_wrapper_matches_the_guarded_call(hip):
    H, W = 45, 40
    src, pl = ao.image(H, W, 9), ao.planes(3, H, W, 10)
    hm, jt = np.stack(ao.general_warps(H, W)), np.asarray(ao.JITTERS, np.int32)
    got = hip.warp_clip(torch.from_numpy(src).cuda(), torch.from_numpy(pl).cuda(), hm.reshape(-1, 3, 3), jt)
    for a, b in zip(got, warp_guarded(hip, src, pl, hm, jt)):
        assert np.array_equal(a.cpu().numpy(), b)
    got = hip.warp_clip(torch.from_numpy(src).cuda(), None, hm)
    assert got[1].shape == (0, 7, H, W) and np.array_equal(got[0].cpu().numpy(), warp_guarded(hip, src, None, hm)[0])


# ------------------------------------------------------------------------------------------------ jitter
@pytest.fixture(scope="module")
def all_colours():
    c = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([c & 255, (c >> 8) & 255, c >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.parametrize("params", ((40, 5, ao.JITTER_ADD), (-40, -5, ao.JITTER_ADD), (40, 5, ao.JITTER_HUE_SAT), (40, -5, ao.JITTER_HUE_SAT),
                                    (-40, 15, ao.JITTER_HUE_SAT), (-40, -15, ao.JITTER_HUE_SAT), (40, -15, 3), (-40, 5, 3)),
                         ids=lambda p: "add%+d_hs%+d_flags%d" % p)
def test_jitter_of_every_colour_is_the_float32_restatement(hip, all_colours, params):
    """All 2^24 colours as a 4096 x 4096 source under the identity warp: add only at +-40, hue / saturation only at +-5 and +-15, both."""
    src = torch.from_numpy(all_colours).cuda()
    frames, _, invalid = hip.warp_clip(src, None, ao.identity()[None], [params])
    expect = torch.from_numpy(ao.jitter(all_colours, *params))
    assert torch.equal(frames[0].cpu(), expect)
    assert not bool(invalid.any())
    if params[2] == ao.JITTER_ADD:          # the unused parameter is ignored
        assert torch.equal(expect, torch.from_numpy(np.clip(all_colours.astype(np.int32) + params[0], 0, 255).astype(np.uint8)))


# ------------------------------------------------------------------------------------------------ motion_blur
@pytest.mark.parametrize("shape", ao.BLUR_SHAPES)
def test_blur_delta_matrix_and_k0_copy_exactly(hip, shape):
    H, W = shape
    frames = np.stack([ao.image(H, W, 60 + f) for f in range(4)])
    out = blur_guarded(hip, frames, [None, ao.delta_matrix(7), ao.delta_matrix(9), ao.delta_matrix(11)])
    assert np.array_equal(out, frames)


BLUR_CASES = ao.blur_cases()


@pytest.mark.parametrize("case", BLUR_CASES, ids=[c[0] for c in BLUR_CASES])
def test_blur_box_and_line_matrices_within_the_band(hip, case):
    name, frames, matrices = case
    ref, soft = ao.motion_blur(frames, matrices)
    out = blur_guarded(hip, frames, matrices)
    ao.check_u8(out, ref, soft, name)
    for f, m in enumerate(matrices):
        assert np.array_equal(out[f], frames[f]) == (m is None)
    got = hip.motion_blur(torch.from_numpy(frames).cuda(), matrices)
    assert np.array_equal(got.cpu().numpy(), out)


@pytest.mark.parametrize("k,H,W", ((7, 4, 23), (9, 16, 5), (11, 6, 6), (11, 6, 40)))
def test_blur_reflect_101_on_a_frame_barely_larger_than_the_halo(hip, k, H, W):
    """H or W = k / 2 + 1: every halo pixel is a reflection, up to the far edge.  A matrix with all its weight in one corner reads
    exactly the reflected pixel."""
    frames = ao.image(H, W, 80)[None]
    ref, soft = ao.motion_blur(frames, [ao.line_matrix(k, 9)])
    ao.check_u8(blur_guarded(hip, frames, [ao.line_matrix(k, 9)]), ref, soft, "k=%d on %dx%d" % (k, H, W))
    R = k // 2
    for dy, dx in ((0, 0), (k - 1, k - 1), (0, k - 1)):
        m = np.zeros((k, k), np.float32)
        m[dy, dx] = 1
        expect = np.pad(frames[0], ((R, R), (R, R), (0, 0)), mode="reflect")[dy:dy + H, dx:dx + W]
        assert np.array_equal(blur_guarded(hip, frames, [m])[0], expect), (dy, dx)


# ------------------------------------------------------------------------------------------------ duplicate_instance
DUP_CASES = ao.duplicate_cases()


@pytest.mark.parametrize("case", DUP_CASES, ids=[c[0] for c in DUP_CASES])
def test_duplicate_instance(hip, case):
    name, frames, mask, boxes, flip, shifts = case
    ref = ao.duplicate_instance(frames, mask, boxes, flip, shifts)
    got_f, got_m = duplicate_guarded(hip, frames, mask, boxes, flip, shifts)
    assert ref["pasted"].any() and ref["masks"][0].any(), "the case must paste something and keep something"
    if name.startswith("integer"):
        assert np.array_equal(got_f, ref["frames"]) and np.array_equal(got_m, ref["masks"])
    band = ao.weight_band(ref["weight"])
    ao.check_bits(got_m[1], ref["masks"][1], band, name + " copy")
    ao.check_bits(got_m[0], ref["masks"][0], band, name + " original")
    agree = (got_m[1] == ref["masks"][1])[..., None]
    ao.check_u8(np.where(agree, got_f, ref["frames"]), ref["frames"], ref["soft"], name + " frames")
    for t, b in enumerate(boxes):
        if b is None:
            assert np.array_equal(got_f[t], frames[t]) and np.array_equal(got_m[0, t], mask[t]) and np.array_equal(got_m[1, t], mask[t])
    out_f, out_m = hip.duplicate_instance(torch.from_numpy(frames).cuda(), torch.from_numpy(mask).cuda(), boxes, flip, shifts)
    assert np.array_equal(out_f.cpu().numpy(), got_f) and np.array_equal(out_m.cpu().numpy(), got_m)


def test_duplicate_integer_shift_moves_the_flipped_box(hip):
    """Independent of the oracle: an integer shift with flip pastes the mirrored box content, shifted, wherever the mirrored mask is set."""
    name, frames, mask, boxes, flip, shifts = DUP_CASES[1]
    got_f, got_m = duplicate_guarded(hip, frames, mask, boxes, flip, shifts)
    sx, sy = int(shifts[0][0]), int(shifts[0][1])
    xmin, ymin, xmax, ymax = boxes[0]
    fl_img, fl_mask = frames[0].copy(), mask[0].copy()
    fl_img[ymin:ymax, xmin:xmax], fl_mask[ymin:ymax, xmin:xmax] = fl_img[ymin:ymax, xmin:xmax][:, ::-1], fl_mask[ymin:ymax, xmin:xmax][:, ::-1]
    sh_img, sh_mask = np.zeros_like(fl_img), np.zeros_like(fl_mask)
    H, W = fl_mask.shape
    ys, xs = slice(max(sy, 0), min(H + sy, H)), slice(max(sx, 0), min(W + sx, W))
    ys0, xs0 = slice(max(-sy, 0), min(H - sy, H)), slice(max(-sx, 0), min(W - sx, W))
    sh_img[ys, xs], sh_mask[ys, xs] = fl_img[ys0, xs0], fl_mask[ys0, xs0]
    assert np.array_equal(got_m[1, 0], sh_mask) and np.array_equal(got_m[0, 0], np.where(sh_mask, 0, mask[0]))
    assert np.array_equal(got_f[0], np.where(sh_mask[..., None] > 0, sh_img, frames[0]))


# ------------------------------------------------------------------------------------------------ masked pre-processing
MEAN, STD = (102.9801, 115.9465, 122.7717), (1.0, 1.0, 1.0)


@pytest.mark.parametrize("unit_scale,flip", ((False, False), (True, True)))
def test_masked_preprocess(hip, unit_scale, flip):
    """Nothing invalid: the bits of ``preprocess_frames``.  Otherwise within that function's 1e-4 of normalise -> mask -> resize on the CPU,
    and still the unmasked bits wherever no tap is invalid."""
    T, H, W, new_hw, pad_hw = 3, 37, 53, (45, 64), (64, 64)
    frames = np.stack([ao.image(H, W, 90 + t) for t in range(T)])
    mean, std = (MEAN, STD) if not unit_scale else ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    dev = torch.from_numpy(frames).cuda()
    plain = hip.preprocess_frames(dev, new_hw, pad_hw, mean, std, unit_scale, flip)
    none = hip.preprocess_frames(dev, new_hw, pad_hw, mean, std, unit_scale, flip, invalid=torch.zeros((T, H, W), dtype=torch.uint8, device="cuda"))
    assert torch.equal(plain, none)
    invalid = ao.warp_clip(frames[0], None, np.stack(ao.general_warps(H, W)[:T]))["invalid"]
    assert 0.01 < invalid.mean() < 0.5
    g_out = Guarded(T * 3 * pad_hw[0] * pad_hw[1] * 4)
    g_in, g_inv = Guarded.of(frames), Guarded.of(invalid)
    m, s = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    rc = hip.lib().stemseg_hip_preprocess_frames_masked(g_in.ptr(), g_inv.ptr(), T, H, W, new_hw[0], new_hw[1], pad_hw[0], pad_hw[1], m, s,
                                                        int(unit_scale), int(flip), g_out.ptr(), hip.stream())
    assert rc == 0, hip.lib().stemseg_hip_last_error().decode()
    all_intact(frames=g_in, invalid=g_inv, out=g_out)
    got = g_out.numpy((T, 3, pad_hw[0], pad_hw[1]), np.float32)
    ref = ao.preprocess_masked(frames, invalid, new_hw, pad_hw, mean, std, unit_scale, flip)
    err = float(np.abs(got - ref).max())
    print("masked pre-process: max |got - oracle| = %.3g" % err)
    assert err <= 1e-4
    assert not got[:, :, new_hw[0]:].any() and not got[:, :, :, new_hw[1]:].any()
    same = got == plain.cpu().numpy()
    assert 0.3 < same[:, :, :new_hw[0], :new_hw[1]].mean() < 1.0
