"""The stage-end tail (csrc/bottleneck_fused.hip, the LAT variants of fused_tail_kernel -- stage 1 -- and fused_tail_r1_kernel -- stages 2-3;
StemsegEncoderDesc.fuse_tail bits 6-8 keep the stand-alone launches).  Reference: stemseg/modeling/backbone/resnet.py:262-282 (the last
Bottleneck of a stage) and fpn.py:47-69 (the level's lateral 1x1) of the reference implementation.

The last block of stages 1-3 ends in ONE launch: conv3 + identity + ReLU write the stage output, the same values -- split in registers -- feed
the K loop of the level's FPN lateral (1x1, 4 MID -> 256, + bias, no ReLU, a dense map), and the lanes at even (y, x) also store their value
into the next stage's 2x sub-sampled input.  Same operands, MFMA, product and chunk order and the same two rounded finishing steps as the three
stand-alone launches (conv3, lateral, sub-sample pass): everything a pass leaves must be BIT-IDENTICAL with the tails (fuse_tail 7), with bits
6-8 set (7 | 64 | 128 | 256: the launches of before) and with three launches per block (0) -- every pass here is planned on 4096 frames, where
no launch splits K.  A wrong counted wait of the variant reads stale LDS, it does not fault: this comparison is what catches it.

Shapes (R-50; V = positions at stages 1 / 2 / 3, a workgroup owns 128):
  1 x 64 x 128    V = 512 / 128 / 32      whole tiles at stage 1, one at stage 2, a partial one at stage 3
  3 x 96 x 192    V = 3456 / 864 / 216    partial last tiles at stages 2-3
  3 x 96 x 160    V = 2880 / 720 / 180    a partial last tile at stage 1; the 16x level is 10 wide, so stage 3 keeps its launches
  2 x (1 x 64 x 128) in one pass (n_clips = 2) against each clip alone.
Compared as int32 bit patterns, so that the non-finite case compares too."""
import numpy as np
import pytest
import torch

from tests import synth
from tests.fused_tail_util import FUSED_TAG, MEAN, backbone as _backbone

pytestmark = pytest.mark.gpu

PLAN_FRAMES = 4096                       # no convolution of a pass planned on this many frames splits K
ENDS, LAUNCHES, THREE = 7, 7 | 64 | 128 | 256, 0
END_TAG, SUBSAMPLE_TAG = 52, 49          # profile slots: the stage-end tail, the sub-sample pass
CONV1X1_TAGS = (18, 17, 14, 16, 12)      # hip.PROFILE_CONV_TAGS["conv1x1x1"] without the fused launches' own tags
NAMES = ("1/4", "1/8", "1/16", "1/32", "stage 1", "stage 2", "stage 3", "stage 4's sub-sampled input")


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


@pytest.fixture(scope="module")
def bb():
    b, _ = _backbone("R-50-FPN", 91)
    b.plan_frames = PLAN_FRAMES
    return b


def _frames(T, H, W, seed):
    return (torch.from_numpy(synth.synth_frames(T, H, W, seed=seed).astype(np.float32)).permute(0, 3, 1, 2) - MEAN).cuda()


def _left_behind(hip, bb, x):
    """Copies of what the last pass of x left in its workspace: the outputs of stages 1-3 and XS, the 2x sub-sampled output of stage 3."""
    T, _, H, W = x.shape
    key = (T, H, W, x.device.index, bb.lane, None, int(bb.plan_frames))
    offs = (hip.C.c_int64 * 25)()
    hip.check(hip.lib().stemseg_hip_encoder_plan_offsets(hip.C.byref(bb._ws_desc[key]), offs))
    ws = bb._ws[key].view(torch.float32)
    out = []
    for st in (0, 1, 2):
        C, h, w = 256 << st, H >> (2 + st), W >> (2 + st)
        out.append(ws[int(offs[4 + st]):int(offs[4 + st]) + C * T * h * w].view(C, T, h, w).clone())
    out.append(ws[int(offs[14]):int(offs[14]) + 1024 * T * (H // 32) * (W // 32)].view(1024, T, H // 32, W // 32).clone())
    return out


def _run(hip, bb, x, fuse, n_clips=1):
    """-> (4 n_clips FPN maps [+ the stage outputs and XS of a one-clip pass], launch counts of the pass)."""
    bb.fuse_tail, bb.precision = fuse, "f16x3"
    T, _, H, W = x.shape
    outs = [torch.full((256, T // n_clips, H // s, W // s), float("nan"), device="cuda") for _ in range(n_clips) for s in (4, 8, 16, 32)]
    hip.profile_enable(True)
    hip.profile_read()
    bb.run_backbone_into(x, [hip.dense_volume(o) for o in outs])
    prof = hip.profile_read()
    hip.profile_enable(False)
    if n_clips == 1:
        outs = outs + _left_behind(hip, bb, x)
    n = lambda t: prof.get(t, (0, 0, 0))[2]
    counts = dict(end=n(END_TAG), fused=n(FUSED_TAG), sub=n(SUBSAMPLE_TAG), conv1x1=sum(n(t) for t in CONV1X1_TAGS))
    assert bb.check_workspaces()[0] == 0
    return outs, counts


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _three_ways(hip, bb, x, engaged):
    got, c_got = _run(hip, bb, x, ENDS)
    own, c_own = _run(hip, bb, x, LAUNCHES)
    ref, c_ref = _run(hip, bb, x, THREE)
    print("[stage end] %s launches: default %s, bits 6-8 %s, fuse_tail 0 %s" % (tuple(x.shape), c_got, c_own, c_ref))
    # host side: `engaged` stage ends, none with bits 6-8 set; R-50's 2 + 3 + 5 block-to-block tails either way; no sub-sample pass in front of
    # a stage whose input the previous stage's end wrote; conv3 and the lateral of an engaged stage are no launches of their own
    assert c_got["end"] == engaged and c_own["end"] == 0 and c_ref["end"] == 0, (c_got, c_own, c_ref)
    assert c_got["fused"] == c_own["fused"] == 10 and c_ref["fused"] == 0, (c_got, c_own, c_ref)
    assert c_got["sub"] == 3 - engaged and c_own["sub"] == 3 and c_ref["sub"] == 3, (c_got, c_own, c_ref)
    assert c_got["conv1x1"] == c_own["conv1x1"] - 2 * engaged, (c_got, c_own)
    for g, o, r, s in zip(got, own, ref, NAMES):
        assert _same_bits(g, o), "%s: %d of %d values differ from the stand-alone stage ends" % (s, int((g != o).sum()), g.numel())
        assert _same_bits(g, r), "%s: %d of %d values differ from the three-launch blocks" % (s, int((g != r).sum()), g.numel())
    return got


@pytest.mark.parametrize("shape,engaged", [((1, 64, 128), 3), ((3, 96, 192), 3), ((3, 96, 160), 2)])
def test_stage_ends_are_bit_identical(hip, bb, shape, engaged):
    T, H, W = shape
    x = _frames(T, H, W, 95)
    mask = hip.C.c_int32(-1)
    bb.fuse_tail, bb.precision = ENDS, "f16x3"
    hip.check(hip.lib().stemseg_hip_encoder_stage_end_mask(hip.C.byref(bb._desc(T, H, W)), hip.C.byref(mask)))
    assert mask.value == (7 if engaged == 3 else 3)          # (a 16x level 10 wide has no dense-lateral add pass: stage 3 falls back)
    got = _three_ways(hip, bb, x, engaged)
    for g in got:
        assert torch.isfinite(g).all()
    # the comparison is not one of zeros: the last ReLU of every stage clips some of its outputs and passes others
    for st in (4, 5, 6):
        zeros = float((got[st] == 0).float().mean())
        print("[stage end] %s stage %d: %.1f %% of the output clipped by the ReLU" % (shape, st - 3, 100 * zeros))
        assert 0.0 < zeros < 1.0, (st, zeros)
    # the copy is the stride-2 sub-sample of stage 3's output
    assert _same_bits(got[7], got[6][:, :, ::2, ::2])


def test_two_clips_in_one_pass_against_each_alone(hip, bb):
    xa, xb = _frames(1, 64, 128, 96), _frames(1, 64, 128, 97)
    both, c_both = _run(hip, bb, torch.cat([xa, xb], 0), ENDS, n_clips=2)
    assert c_both["end"] == 3 and c_both["sub"] == 0
    for k, x in enumerate((xa, xb)):
        alone, _ = _run(hip, bb, x, ENDS)
        for a, b in zip(alone[:4], both[4 * k:4 * k + 4]):
            assert _same_bits(a, b)
    ref, _ = _run(hip, bb, torch.cat([xa, xb], 0), THREE, n_clips=2)
    for a, b in zip(both, ref):
        assert _same_bits(a, b)


def test_an_inf_in_the_input_arrives_as_in_the_stand_alone_launches(hip, bb):
    """One +inf pixel in one colour channel, the exact fp32 stem: every stem output under it is ONE inf term plus finite ones -- +-inf by the
    tap's sign, never inf - inf -- and the ReLU and the max-pool hand +inf on.  Its f16x3 split is (inf, NaN): the sums under it are NaN in
    every path, relu_keep_nan keeps them in the stage outputs, the lateral (no ReLU) and the copy carry them as the launches do, and the three
    paths must agree on every bit of every map."""
    x = _frames(1, 64, 128, 98)
    x[0, 1, 30, 44] = float("inf")
    s2d = bb.stem_s2d
    bb.stem_s2d = False
    try:
        got = _three_ways(hip, bb, x, 3)
    finally:
        bb.stem_s2d = s2d
    bad = ~torch.isfinite(got[4][:, 0]).all(0)                  # [16, 32]: positions of stage 1's output with a non-finite channel
    assert bad[5:10, 9:14].all() and not bad[:, :4].any() and not bad[:, -4:].any(), "the planted value reaches stage 1 around (7, 11), and only there"
    assert not torch.isfinite(got[0]).all() and not torch.isfinite(got[7]).all(), "the 4x lateral and the sub-sampled copy carry it"
