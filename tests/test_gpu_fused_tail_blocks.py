"""The fused bottleneck tail (csrc/bottleneck_fused.hip) block by block: what the kernel ITSELF writes -- y, a block's output, and z, the next
block's conv1 output inside the stage's zero-haloed M1 buffer -- against an fp64 reference of the same folded weights (tests/bottleneck_ref.py),
per output channel, for all three kernel forms.

Networks (tests/fused_tail_util.py): ONE stage of three blocks, one block elsewhere -- (3,1,1,1), (1,3,1,1), (1,1,3,1): six bottlenecks.  The
three-block stage runs two tails (block 0 -> 1 behind the projection shortcut, block 1 -> 2 behind the plain identity); after the pass the
workspace still holds B = block 1's output (the second tail's y), M1[stage] = block 2's conv1 output (its z) and Cst[stage] = the stage output.

Forms: stage 1 always runs the 32-column form (MID 64); stage 2 the one-wave-per-SIMD form (MID 128) or, under fuse_tail's form bits = 1, the
32-column form (MID 128); stage 3 the one-wave-per-SIMD form (MID 256) or the 16-column form.

Shapes: 32 x 32 frames with T = 1, 32, 33 -- the stage-3 map is 2 x 2: V = 4 (far below one 128-position workgroup), 128 (exactly one), 132;
stage 1: V = 64, 2048, 2112 -- and 64 x 96 with T = 3 (V = 1152 / 288 / 72).  plan_frames = 4096 throughout: conv2 hands its output over as
operand planes only where its PLANNED launch is un-split (conv_igemm.h, plan_ksplit: >= 128 planned workgroups); a 2 x 2 map makes
ceil(plan_frames x 16 / 512) x 2 flat workgroups, i.e. needs plan_frames >= 2048, and at 4096 the separate 1x1 launches of the comparison
runs stay un-split as well (more than 320 planned workgroups, or the 256-channel tile that takes no scratch) -- except stage 3's conv1 on
2 x 2 maps (256 workgroups), so fused == three launches is asserted there on the 4 x 6 maps of the 64 x 96 frames only.
Observed: 2 fused launches (profile slot 19) in every fused f16x3 pass of every shape above, 0 in the f32 and fuse_tail = 0 passes.

Error bound: per channel max|got - ref64| / max|ref64[channel]|, worst channel <= max(3 x the fp32-input MFMA pass's worst channel, 2e-6) --
the rule of test_split_modes_keep_fp32_level_with_per_channel_dynamic_range with the encoder-depth floor of the checkpoint-like-BN test: the
buffers sit 7 (stage 1's B) to 16 (stage 3's Cst) convolutions deep, every one re-rounding its operands to 22 bits; independent roundings of
the single-conv floor 4e-7 compound to 4e-7 x sqrt(7 ... 16) = 1.1e-6 ... 1.6e-6."""
import functools

import pytest
import torch

from tests import fused_tail_util as U
from tests.fused_tail_util import R1, W16

pytestmark = pytest.mark.gpu
FLOOR = 2e-6
# (stage, fuse_tail, kernel form)
FORMS = [pytest.param(0, 7, id="s1-32col"), pytest.param(1, R1, id="s2-r1"), pytest.param(1, W16, id="s2-32col"), pytest.param(2, R1, id="s3-r1"),
         pytest.param(2, W16, id="s3-16col")]
SHAPES = [(1, 32, 32), (32, 32, 32), (33, 32, 32), (3, 64, 96)]
BUFFERS = ("B", "M1", "Cst")


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


@functools.lru_cache(maxsize=None)
def _net(stage, stress=False, g=1.0):
    """-> (backbone on the device, the folded weights its kernels are packed from, as the fp64 reference reads them)"""
    bb, sd = U.tiny_backbone(stage, stress)
    if g != 1.0:
        U.load(bb, U.scale_network(sd, g))
    bb = bb.cuda()
    return bb, {k: (w.cpu(), b.cpu()) for k, (w, b) in bb.folded_state().items()}


def _frames(shape, seed=U.SEED, g=1.0):
    return U.frames(*shape, seed=seed, scale=g)


def _pass(hip, bb, x, stage, fuse, precision="f16x3"):
    """One pass; asserts that the fused kernel ran exactly twice (the three-block stage's two tails) or, un-fused / f32, not at all."""
    outs, n = U.run(hip, bb, x, fuse, precision)
    want = 2 if (fuse and precision == "f16x3") else 0
    assert n == want, "%d fused launches, expected %d (T, H, W = %s, fuse_tail %s, %s)" % (n, want, (x.shape[0],) + tuple(x.shape[2:]), fuse, precision)
    buf = U.tail_buffers(hip, bb, x, stage)
    buf["outs"] = outs
    return buf


@functools.lru_cache(maxsize=None)
def _yardstick(hip, stage, shape, stress=False, g=1.0, seed=U.SEED):
    """-> (fp64 reference of the three buffers, {buffer: per-channel error of the fp32-input MFMA pass}, live channels per buffer); computed once per case"""
    bb, folded = _net(stage, stress, g)
    x = _frames(shape, seed, g)
    ref = U.reference(bb, x, stage, folded)
    got = _pass(hip, bb, x.cuda(), stage, False, "f32")
    live = {k: U.channel_scales(ref[k]) > 0 for k in BUFFERS}
    for k in BUFFERS:
        assert U.dead_share(ref[k]) <= 0.10
    return ref, {k: _channel_err(got[k], ref[k]) for k in BUFFERS}, live


def _channel_err(got, ref):
    """max|got - ref| / max|ref| per channel, over the channels the reference does not leave identically zero"""
    s = U.channel_scales(ref)
    e = (got.double().cpu() - ref).abs().reshape(ref.shape[0], -1).amax(1)
    return e[s > 0] / s[s > 0]


def _assert_fp32_level(tag, got, ref, e32):
    for k in BUFFERS:
        assert torch.isfinite(got[k]).all(), "%s %s: non-finite values" % (tag, k)
        e = _channel_err(got[k], ref[k])
        print("[fused blocks] %s %s: worst channel fp32-MFMA %.3e, fused f16x3 %.3e (median %.3e / %.3e)" % (tag, k, float(e32[k].max()), float(e.max()),
                                                                                                          float(e32[k].median()), float(e.median())))
        assert float(e.max()) <= max(3.0 * float(e32[k].max()), FLOOR), "%s %s: channel %d of the live ones" % (tag, k, int(e.argmax()))
        # the same rule on the median channel: one cancellation-heavy channel (a block output is conv3 + identity) sets both worst cases
        assert float(e.median()) <= max(3.0 * float(e32[k].median()), FLOOR), "%s %s: median channel" % (tag, k)


def _assert_halo_zero(hip, bb, buf, tag):
    bad = int((buf["M1_halo"] != 0).sum())
    assert bad == 0, "%s: %d halo words of M1 are not +0" % (tag, bad)
    assert bb.check_workspaces()[0] == 0, tag


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("stage,fuse", FORMS)
def test_every_channel_of_y_and_z_at_the_fp32_level(hip, stage, fuse, shape):
    """1. Per-channel accuracy of B, M1[stage] and Cst[stage] against fp64, yardstick: the same pass through the fp32-input MFMA."""
    ref, e32, _ = _yardstick(hip, stage, shape)
    bb, _ = _net(stage)
    got = _pass(hip, bb, _frames(shape).cuda(), stage, fuse)
    _assert_fp32_level("stage %d fuse %d %s" % (stage + 1, fuse, shape), got, ref, e32)


@pytest.mark.parametrize("g", [1e-4, 1.0, 5.0])
@pytest.mark.parametrize("stage,fuse", FORMS)
def test_every_channel_under_checkpoint_like_statistics_and_operand_magnitudes(hip, stage, fuse, g):
    """2. The same with FrozenBN-like per-output-channel ranges on the tails' own layers (bn3 of blocks 0-1, bn1 of blocks 1-2: running_var over
    1e-6 ... 1e2, gamma over 1e-4 ... 0.5 / 3) and every activation of the network scaled by g: the stage inputs are ~1e-2 (g = 1e-4; many
    values below the 2.5e-4 where the high fp16 term goes subnormal), ~2e2 (max 2e3) and ~1e3 (max 1e4)."""
    shape = (33, 32, 32)
    ref, e32, _ = _yardstick(hip, stage, shape, True, g)
    bb, _ = _net(stage, True, g)
    got = _pass(hip, bb, _frames(shape, g=g).cuda(), stage, fuse)
    _assert_fp32_level("stress g %g stage %d fuse %d" % (g, stage + 1, fuse), got, ref, e32)


@pytest.mark.parametrize("shape", [(1, 32, 32), (33, 32, 32), (3, 64, 96)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("stage,fuse", FORMS)
def test_ragged_columns_leave_the_halo_of_m1_zero(hip, stage, fuse, shape):
    """3. Position counts that are no multiple of the workgroup's: the columns past V are computed and dropped -- none may be decoded into a halo
    word of M1 (the next 3x3 would read it), nor anywhere outside the slices; also after a second pass of other frames through the same workspace."""
    bb, _ = _net(stage)
    for seed in (U.SEED, U.SEED + 1):
        buf = _pass(hip, bb, _frames(shape, seed).cuda(), stage, fuse)
        _assert_halo_zero(hip, bb, buf, "stage %d fuse %d %s seed %d" % (stage + 1, fuse, shape, seed))
    ref, e32, _ = _yardstick(hip, stage, shape, seed=U.SEED + 1)          # (and the second pass is a right one: nothing of the first left behind)
    _assert_fp32_level("second pass stage %d fuse %d %s" % (stage + 1, fuse, shape), buf, ref, e32)


@pytest.mark.parametrize("stage,fuse,shape", [(0, 7, (33, 32, 32)), (1, R1, (33, 32, 32)), (1, W16, (33, 32, 32)), (0, 7, (3, 64, 96)), (1, R1, (3, 64, 96)),
                                              (1, W16, (3, 64, 96)), (2, R1, (3, 64, 96))])
def test_fused_equals_the_three_launches_bit_for_bit(hip, stage, fuse, shape):
    """4. The 32-column and one-wave-per-SIMD forms against conv3 and conv1 as separate f16x3 launches, where those do not split K (module docstring:
    stage 3 on the 64 x 96 frames only)."""
    bb, _ = _net(stage)
    x = _frames(shape).cuda()
    sep = _pass(hip, bb, x, stage, False)
    got = _pass(hip, bb, x, stage, fuse)
    for k in BUFFERS:
        assert torch.equal(sep[k], got[k]), "%s: %d of %d values differ, max %g" % (k, int((sep[k] != got[k]).sum()), sep[k].numel(), float((sep[k] - got[k]).abs().max()))


@pytest.mark.parametrize("shape", [(33, 32, 32), (3, 64, 96)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("stage,fuse", FORMS)
def test_buffers_do_not_depend_on_the_batch(hip, stage, fuse, shape):
    """5. T frames alone and as the tail of a 2T pass (same plan_frames; the frames then start at another column of another workgroup)."""
    bb, _ = _net(stage)
    T = shape[0]
    x, other = _frames(shape).cuda(), _frames(shape, U.SEED + 2).cuda()
    alone = _pass(hip, bb, x, stage, fuse)
    both = _pass(hip, bb, torch.cat([other, x], 0).contiguous(), stage, fuse)
    for k in BUFFERS:
        assert torch.equal(alone[k], both[k][:, T:]), "%s: %d values differ" % (k, int((alone[k] != both[k][:, T:]).sum()))
    _assert_halo_zero(hip, bb, both, "2T pass")


@pytest.mark.parametrize("stage", [0, 1, 2])
def test_overflow_is_not_silent_through_the_tail(hip, stage):
    """6. One output channel of block 1's conv3 raised until B exceeds 4 x 65520 at some positions (8 x that at the largest: 2.1e6, ordinary finite
    fp32 values): B is stored in fp32 and stays finite and right, conv1 consumes the overflowed fp16 planes, and z must come back NON-FINITE in
    every channel at exactly those positions -- through the ReLU of all three forms and of the separate launches -- and the encoder's outputs flag it."""
    shape = (33, 32, 32)
    x = _frames(shape)
    bb, _, channel, factor, over, inside, _ = U.overflow_network(stage, x)
    assert int(over.sum()) > 0 and int(inside.sum()) > 0
    bb = bb.cuda()
    ref = U.reference(bb, x, stage, {k: (w.cpu(), b.cpu()) for k, (w, b) in bb.folded_state().items()})
    keep = torch.ones(ref["B"].shape[0], dtype=torch.bool)
    keep[channel] = False
    e32 = _channel_err(_pass(hip, bb, x.cuda(), stage, False, "f32")["B"][keep], ref["B"][keep])
    for fuse in {0: (7, False), 1: (R1, W16, False), 2: (R1, W16, False)}[stage]:
        got = _pass(hip, bb, x.cuda(), stage, fuse)
        tag = "overflow stage %d fuse %s (channel %d x %.4g: %d positions over, %d inside)" % (stage + 1, fuse, channel, factor, int(over.sum()), int(inside.sum()))
        assert torch.isfinite(got["B"]).all(), tag
        e = _channel_err(got["B"][keep], ref["B"][keep])
        print("[fused blocks] %s: B worst channel fp32-MFMA %.3e, f16x3 %.3e" % (tag, float(e32.max()), float(e.max())))
        assert float(e.max()) <= max(3.0 * float(e32.max()), FLOOR), tag
        finite = torch.isfinite(got["M1"]).cpu()
        assert not finite[:, over].any(), "%s: %d finite values of z at over-range positions" % (tag, int(finite[:, over].sum()))
        assert finite[:, inside].all(), "%s: %d non-finite values of z at in-range positions" % (tag, int((~finite[:, inside]).sum()))
        assert bool(hip.overflow_status(got["outs"]).any()), tag
        assert bb.check_workspaces()[0] == 0
