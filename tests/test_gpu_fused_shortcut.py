"""The projection shortcut inside the fused tail of a stage's first block (csrc/bottleneck_fused.hip, the DS variants of fused_tail_kernel --
stage 1, 64 -> 256 -- and fused_tail_r1_kernel -- stage 2, 256 -> 512; StemsegEncoderDesc.fuse_tail bit 5 keeps the stand-alone launch).
Reference: stemseg/modeling/backbone/resnet.py:262-282 of the reference implementation (Bottleneck.forward with a downsample branch).

The variant sums the shortcut with the operands (split_pair_f16 of the block's fp32 input, the packed down_w), the MFMA, the product order
and the k order of the stand-alone 1x1 launch, and finishes it with the same two rounded steps (x 1 / scale, + bias): the encoder's four FPN
maps must be BIT-IDENTICAL with the shortcut in the tail (fuse_tail 7), as its own launch in front of the tail (7 | 32) and with three
launches per block (0), wherever the separate launches run without split-K -- every pass here is planned on 4096 frames, where none splits.
A wrong counted wait of the variant reads stale LDS, it does not fault: this comparison is what catches it.

Shapes (R-50, V = positions at stage 1 / stage 2; a workgroup owns 128):
  1 x 64 x 96     V = 384 / 96     whole tiles at stage 1, less than one tile at stage 2
  3 x 96 x 160    V = 2880 / 720   a partial last tile at both stages (columns past V are computed from the last valid one and never stored)
  2 x (1 x 64 x 96) in one pass (n_clips = 2) against each clip alone.
Compared as int32 bit patterns, so that the non-finite case compares too."""
import numpy as np
import pytest
import torch

from tests import synth
from tests.fused_tail_util import FUSED_TAG, MEAN, backbone as _backbone

pytestmark = pytest.mark.gpu

PLAN_FRAMES = 4096                       # no convolution of a pass planned on this many frames splits K
IN_TAIL, OWN_LAUNCH, THREE = 7, 7 | 32, 0
CONV1X1_TAGS = (18, 17, 14, 16, 12)      # hip.PROFILE_CONV_TAGS["conv1x1x1"] without the fused tail's own tag


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


def _stage_outputs(hip, bb, x):
    """Copies of the outputs of stages 1 and 2 ([256, T, H/4, W/4], [512, T, H/8, W/8]) as the last pass of x left them in its workspace."""
    T, _, H, W = x.shape
    key = (T, H, W, x.device.index, bb.lane, None, int(bb.plan_frames))
    offs = (hip.C.c_int64 * 25)()
    hip.check(hip.lib().stemseg_hip_encoder_plan_offsets(hip.C.byref(bb._ws_desc[key]), offs))
    ws = bb._ws[key].view(torch.float32)
    out = []
    for st in (0, 1):
        C, h, w = 256 << st, H >> (2 + st), W >> (2 + st)
        out.append(ws[int(offs[4 + st]):int(offs[4 + st]) + C * T * h * w].view(C, T, h, w).clone())
    return out


def _run(hip, bb, x, fuse, n_clips=1):
    """-> (4 n_clips FPN maps [+ the outputs of stages 1-2 of a one-clip pass], stand-alone 1x1 launches of the pass, fused-tail launches)."""
    bb.fuse_tail, bb.precision = fuse, "f16x3"
    T, _, H, W = x.shape
    outs = [torch.full((256, T // n_clips, H // s, W // s), float("nan"), device="cuda") for _ in range(n_clips) for s in (4, 8, 16, 32)]
    hip.profile_enable(True)
    hip.profile_read()
    bb.run_backbone_into(x, [hip.dense_volume(o) for o in outs])
    prof = hip.profile_read()
    hip.profile_enable(False)
    if n_clips == 1:
        outs = outs + _stage_outputs(hip, bb, x)
    return outs, sum(prof.get(t, (0, 0, 0))[2] for t in CONV1X1_TAGS), prof.get(FUSED_TAG, (0, 0, 0))[2]


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _three_ways(hip, bb, x):
    got, n_got, f_got = _run(hip, bb, x, IN_TAIL)
    own, n_own, f_own = _run(hip, bb, x, OWN_LAUNCH)
    ref, n_ref, f_ref = _run(hip, bb, x, THREE)
    # host side: R-50 fuses 2 + 3 + 5 tails either way; the default pass has exactly the two shortcut launches of stages 1-2 fewer
    assert f_got == f_own == 10 and f_ref == 0, (f_got, f_own, f_ref)
    assert n_got == n_own - 2, "stand-alone 1x1 launches: %d with the shortcut in the tail, %d with bit 5 set" % (n_got, n_own)
    for g, o, r, s in zip(got, own, ref, ("1/4", "1/8", "1/16", "1/32", "stage 1", "stage 2")):
        assert _same_bits(g, o), "%s: %d of %d values differ from the stand-alone shortcut in front of the tail" % (s, int((g != o).sum()), g.numel())
        assert _same_bits(g, r), "%s: %d of %d values differ from the three-launch blocks" % (s, int((g != r).sum()), g.numel())
    return got


@pytest.mark.parametrize("shape", [(1, 64, 96), (3, 96, 160)])
def test_shortcut_in_the_tail_is_bit_identical(hip, bb, shape):
    T, H, W = shape
    got = _three_ways(hip, bb, _frames(T, H, W, 91))
    for g in got:
        assert torch.isfinite(g).all()
    # both signs in front of the blocks' last ReLU: a fair share of the stage outputs is clipped to zero, a fair share is not
    for st in (4, 5):
        zeros = float((got[st] == 0).float().mean())
        print("[shortcut] %s stage %d: %.1f %% of the output clipped by the ReLU" % (shape, st - 3, 100 * zeros))
        assert 0.05 <= zeros <= 0.95
    assert bb.check_workspaces()[0] == 0


def test_two_clips_in_one_pass_against_each_alone(hip, bb):
    xa, xb = _frames(1, 64, 96, 92), _frames(1, 64, 96, 93)
    both, _, _ = _run(hip, bb, torch.cat([xa, xb], 0), IN_TAIL, n_clips=2)
    for k, x in enumerate((xa, xb)):
        alone, _, _ = _run(hip, bb, x, IN_TAIL)
        for a, b in zip(alone[:4], both[4 * k:4 * k + 4]):
            assert _same_bits(a, b)
    ref, _, _ = _run(hip, bb, torch.cat([xa, xb], 0), THREE, n_clips=2)
    for a, b in zip(both, ref):
        assert _same_bits(a, b)
    assert bb.check_workspaces()[0] == 0


def test_an_inf_in_the_shortcut_input_arrives_as_in_the_three_launch_path(hip, bb):
    """One +inf pixel in one colour channel, the exact fp32 stem: every stem output under it is ONE inf term plus finite ones -- +-inf by the
    tap's sign, never inf - inf -- and the ReLU and the max-pool hand +inf on to xin.  Its f16x3 split is (inf, NaN): the shortcut's sums, and
    conv1's, are NaN at those positions in every path, relu_keep_nan keeps them, and the three paths must agree on every bit of every map."""
    x = _frames(1, 64, 96, 94)
    x[0, 1, 30, 44] = float("inf")
    s2d = bb.stem_s2d
    bb.stem_s2d = False
    try:
        got = _three_ways(hip, bb, x)
    finally:
        bb.stem_s2d = s2d
    bad = ~torch.isfinite(got[4][:, 0]).all(0)                  # [16, 24]: positions of stage 1's output with a non-finite channel
    assert bad[5:10, 9:14].all() and not bad[:, :4].any() and not bad[:, -4:].any(), "the planted value reaches stage 1 around (7, 11), and only there"
    assert bb.check_workspaces()[0] == 0
