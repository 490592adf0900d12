"""The fused bottleneck tail (csrc/bottleneck_fused.hip; StemsegEncoderDesc.fuse_tail): conv3 (+ bias + identity + ReLU) of block b and
conv1 (+ bias + ReLU) of block b + 1 in ONE back-to-back kernel, conv2 handing its output over as fp16 operand planes.
Reference: /root/reference/stemseg/modeling/backbone/resnet.py:262-282 of two consecutive blocks.

Stages 1-2 run the 32-column form, stage 3 (MID = 256) the one-wave-per-SIMD form: both issue v_mfma_f32_32x32x16_f16 on the same operands,
with the same split arithmetic and the same k order per accumulator as the separate launches => the encoder's four FPN maps must be
BIT-IDENTICAL with the fusion on and off wherever the separate launches run without split-K (the bench shape at its planning frame count).
The earlier stage-3 kernel, the 16-column form (fuse_tail bit 3; one v_mfma_f32_16x16x32_f16 sums a 32-channel chunk where the others issue
two 16-deep groups), is fp32 round-off apart, ONE result whatever the batch.  Everything within 1e-4 of the CPU oracle."""
import numpy as np
import pytest
import torch

from tests import synth
from tests.fused_tail_util import MEAN, R1, W16, backbone as _backbone, run as _run
from oracle import encoder as oenc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def test_fused_tail_vs_the_three_launch_blocks_at_the_bench_shape(hip):
    """480 x 864, R-101, 8 frames under the 32-frame plan (what a bench step runs).  Stages 1-2 fused (mask 3): 2 + 3 launches; all three stages
    (mask 7, the default): 2 + 3 + 22 launches -- every FPN map torch.equal to the un-fused encoder's; the SAME bits whether the 8 frames pass
    alone or as the second clip of a 16-frame pass (batch invariance of the fused path).  The 16-column form of stage 3: fp32 round-off apart."""
    bb, _ = _backbone("R-101-FPN", 71)
    x = (torch.from_numpy(synth.synth_frames(8, 480, 864, seed=71).astype(np.float32)).permute(0, 3, 1, 2) - MEAN).cuda()
    ref, n0 = _run(hip, bb, x, False)
    got3, n3 = _run(hip, bb, x, 3)
    got, n1 = _run(hip, bb, x, True)
    got_r1, n2 = _run(hip, bb, x, R1)
    got16, n16 = _run(hip, bb, x, W16)
    assert n0 == 0 and n3 == 2 + 3 and n1 == n2 == n16 == 2 + 3 + 22, (n0, n3, n1, n2, n16)
    for r, g3, g, g1, g16, s in zip(ref, got3, got, got_r1, got16, (4, 8, 16, 32)):
        assert torch.isfinite(g).all()
        assert torch.equal(r, g3), "mask 3, 1/%d: %d of %d values differ, max %g" % (s, int((r != g3).sum()), r.numel(), float((r - g3).abs().max()))
        assert torch.equal(r, g), "mask 7, 1/%d: %d of %d values differ, max %g" % (s, int((r != g).sum()), r.numel(), float((r - g).abs().max()))
        assert torch.equal(g, g1)
        scale = max(1.0, float(r.abs().max()))
        err = float((r - g16).abs().max()) / scale
        print("[fused] 1/%d: stage-3 16-column form vs separate launches: max |diff| / scale = %.3g" % (s, err))
        assert err <= 1e-5
    # a second pass of other frames through the same workspaces (no state left behind in the operand planes), alone and behind another clip
    x2 = (torch.from_numpy(synth.synth_frames(8, 480, 864, seed=72).astype(np.float32)).permute(0, 3, 1, 2) - MEAN).cuda()
    for mask, first in ((True, got), (W16, got16)):
        alone, _ = _run(hip, bb, x2, mask)
        both, _ = _run(hip, bb, torch.cat([x, x2], 0), mask)
        for a, b, g in zip(alone, both, first):
            assert torch.equal(a, b[:, 8:]) and torch.equal(g, b[:, :8])
    assert bb.check_workspaces()[0] == 0


@pytest.mark.parametrize("shape", [(3, 96, 160), (5, 128, 224), (2, 480, 864)])
def test_fused_tail_vs_oracle_on_ragged_sizes(hip, shape):
    """Frame counts / map sizes whose position count is not a multiple of the 256-position tile, R-50, vs the CPU oracle (and vs the
    un-fused path to fp32 round-off: at these sizes the separate launches may split K, i.e. sum in another order).  Fused launches: R-50 has
    2 + 3 + 5 tails in stages 1-3; a tail is fused where conv2's launch, planned on 32 frames, is un-split (conv_igemm.h, plan_ksplit: from
    128 planned workgroups on) -- all 10, except 96 x 160: stage 2's 12 x 20 maps plan 96 workgroups of 4 rows x 32 columns and split, its
    three tails run as separate launches (stage 3's 6 x 10 maps: 96 tiles x 2 channel tiles = 192) => 2 + 0 + 5."""
    T, H, W = shape
    bb, sd = _backbone("R-50-FPN", 73)
    x = torch.from_numpy(synth.synth_frames(T, H, W, seed=73).astype(np.float32)).permute(0, 3, 1, 2) - MEAN
    ref = oenc.resnet_fpn(x, {"backbone." + k: v for k, v in sd.items()}, "R-50-FPN")
    got, n1 = _run(hip, bb, x.cuda(), True)
    unf, _ = _run(hip, bb, x.cuda(), False)
    print("[fused] %s: %d fused launches" % (shape, n1))
    assert n1 == {(3, 96, 160): 7, (5, 128, 224): 10, (2, 480, 864): 10}[shape]
    for g, u, s in zip(got, unf, (4, 8, 16, 32)):
        r = ref[s].permute(1, 0, 2, 3).numpy()
        scale = max(1.0, float(np.abs(r).max()))
        assert float(np.abs(g.cpu().numpy() - r).max()) / scale <= 1e-4
        assert float((g - u).abs().max()) / scale <= 2e-5
    assert bb.check_workspaces()[0] == 0


def test_fused_tail_only_in_f16x3(hip):
    bb, _ = _backbone("R-50-FPN", 74)
    x = (torch.from_numpy(synth.synth_frames(2, 96, 160, seed=74).astype(np.float32)).permute(0, 3, 1, 2) - MEAN).cuda()
    for prec in ("bf16x6", "f32"):
        _, n = _run(hip, bb, x, True, prec)
        assert n == 0


@pytest.mark.parametrize("shape", [(3, 96, 160), (5, 128, 224), (1, 480, 864)])
def test_one_wave_per_simd_form_on_ragged_sizes(hip, shape):
    """Position counts that are not a multiple of the 128-position workgroup (columns past V are computed and dropped by the buffer
    descriptors' range check): vs the CPU oracle, and no write outside the workspace slices."""
    T, H, W = shape
    bb, sd = _backbone("R-50-FPN", 73)
    x = torch.from_numpy(synth.synth_frames(T, H, W, seed=73).astype(np.float32)).permute(0, 3, 1, 2) - MEAN
    ref = oenc.resnet_fpn(x, {"backbone." + k: v for k, v in sd.items()}, "R-50-FPN")
    got, n1 = _run(hip, bb, x.cuda(), R1)
    w16, _ = _run(hip, bb, x.cuda(), W16)
    for g, u, s in zip(got, w16, (4, 8, 16, 32)):
        r = ref[s].permute(1, 0, 2, 3).numpy()
        scale = max(1.0, float(np.abs(r).max()))
        assert float(np.abs(g.cpu().numpy() - r).max()) / scale <= 1e-4
        assert float((g - u).abs().max()) / scale <= 2e-5
    assert bb.check_workspaces()[0] == 0
