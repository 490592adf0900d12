"""Host side of the stage-end tail (csrc/encoder.hip, stage_end_mask; csrc/bottleneck_fused.hip): which stage ends engage, as far as the encoder
descriptor decides, and where their lateral maps live -- no GPU needed.  The shapes are those of tests/test_gpu_stage_end_tail.py and the
flagship workload's."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    return h


def _desc(hip, T, H, W, blocks=(3, 4, 6, 3), fuse_tail=7, precision="f16x3", plan_frames=4096, n_clips=1):
    e = hip.EncoderDesc()
    e.struct_bytes = ctypes.sizeof(hip.EncoderDesc)
    for i, n in enumerate(blocks):
        e.blocks[i] = n
    e.T, e.H, e.W, e.out_channels, e.precision, e.n_clips = T, H, W, 256, hip.PRECISIONS[precision], n_clips
    e.plan_frames, e.fuse_tail = plan_frames, fuse_tail
    e.conv2_groups, e.width_per_group, e.stride_in_3x3 = 1, 64, 0
    return e


def _mask(hip, e):
    m = ctypes.c_int32(-1)
    assert hip.lib().stemseg_hip_encoder_stage_end_mask(ctypes.byref(e), ctypes.byref(m)) == 0, hip.lib().stemseg_hip_last_error()
    return m.value


def _offsets(hip, e):
    offs = (ctypes.c_int64 * 25)()
    assert hip.lib().stemseg_hip_encoder_plan_offsets(ctypes.byref(e), offs) == 0
    return list(offs)


def test_which_stage_ends_engage(hip):
    # W / 16 a multiple of 4: all three; a 16x level 10 wide has no dense-lateral add pass, so stage 3 keeps its launches
    assert _mask(hip, _desc(hip, 1, 64, 128)) == 7
    assert _mask(hip, _desc(hip, 3, 96, 192)) == 7
    assert _mask(hip, _desc(hip, 3, 96, 160)) == 3
    # the flagship shape (32 frames of 480 x 864, planned on 32): 30 x 54 at 16x is no multiple of 4 either
    assert _mask(hip, _desc(hip, 32, 480, 864, blocks=(3, 4, 23, 3), plan_frames=32, n_clips=4)) == 3
    # the switches: bits 6-8 one by one; a stage whose fused tails are off keeps its end too; other precisions
    for k in range(3):
        assert _mask(hip, _desc(hip, 1, 64, 128, fuse_tail=7 | (64 << k))) == 7 & ~(1 << k)
        assert _mask(hip, _desc(hip, 1, 64, 128, fuse_tail=7 & ~(1 << k))) == 7 & ~(1 << k)
    assert _mask(hip, _desc(hip, 1, 64, 128, fuse_tail=455)) == 0 and _mask(hip, _desc(hip, 1, 64, 128, fuse_tail=0)) == 0
    assert _mask(hip, _desc(hip, 1, 64, 128, precision="f32")) == 0 and _mask(hip, _desc(hip, 1, 64, 128, precision="bf16x6")) == 0
    # a one-block stage's end is also its first block: it keeps its launches
    assert _mask(hip, _desc(hip, 1, 64, 128, blocks=(1, 3, 1, 1))) == 2
    # the stand-alone lateral of a small map may split K (fewer than 128 workgroups of 256 voxels on the planning shape): those levels keep their launches
    assert _mask(hip, _desc(hip, 1, 64, 128, plan_frames=32)) == 0           # 512 / 128 / 32 positions a frame: 64 / 16 / 4 workgroups
    assert _mask(hip, _desc(hip, 1, 64, 128, plan_frames=128)) == 1          # 256 / 64 / 16
    assert _mask(hip, _desc(hip, 1, 64, 128, plan_frames=256)) == 3          # 512 / 128 / 32
    e = _desc(hip, 1, 64, 128)
    e.conv2_groups, e.width_per_group = 32, 8
    assert _mask(hip, e) == 0                                                # ResNeXt blocks run their launches


def test_plan_offsets_keep_their_meaning(hip):
    """The 25 values are what they were -- the stage-end tails' lateral maps reuse S0 and X1 (dead by then) and add ONE slice behind the
    split-K scratch, so only the total grows, by that slice and its guard block."""
    for T, H, W in ((1, 64, 128), (3, 96, 192), (3, 96, 160)):
        e = _desc(hip, T, H, W)
        offs = _offsets(hip, e)
        V = [T * (H >> (2 + i)) * (W >> (2 + i)) for i in range(4)]
        present = [o for o in offs if o >= 0]
        assert len(set(present)) == len(present) == 21 and offs[0] == 0 and offs[24] == max(present)
        assert offs[24] * 4 == hip.lib().stemseg_hip_encoder_workspace_bytes(ctypes.byref(e))
        # S0 holds the 4x lateral map (the space-to-depth image lies between it and X1) and X1 exactly the 8x one (A starts a guard block later)
        up64 = lambda n: (n + 63) // 64 * 64
        assert offs[1] - offs[0] >= up64(256 * V[0]) + 64
        assert offs[2] - offs[1] == up64(64 * V[0]) + 64 and 64 * V[0] == 256 * V[1]
        # behind the split-K scratch (offs[23], 32 Mi floats at plan_frames >= T): the 16x lateral map and its guard block, then the end
        assert offs[24] - offs[23] == (32 << 20) + 64 + up64(256 * V[2]) + 64
        # the switches change launches, not the plan
        assert _offsets(hip, _desc(hip, T, H, W, fuse_tail=455)) == offs
