"""Host side of tests/test_gpu_fused_tail_blocks.py (no GPU): the fp64 helper tests/bottleneck_ref.py is pinned to the CPU oracle, and the inputs
of every GPU case are valid on the fp64 reference alone -- few channels that the ReLU leaves identically zero (they cannot be scaled), and
positions of both kinds, over the f16x3 range and inside it, in the overflow case."""
import numpy as np
import pytest
import torch

from oracle import encoder as oenc
from tests import fused_tail_util as U
from tests.bottleneck_ref import bottleneck_stages_f64

SHAPES = [(1, 32, 32), (32, 32, 32), (33, 32, 32), (3, 64, 96)]


def test_bottleneck_ref_equals_the_oracle_block_by_block(monkeypatch):
    """R-50: every block output the oracle (fp32, FrozenBN un-folded) produces internally against the helper's (fp64, folded)."""
    bb, sd = U.backbone("R-50-FPN", 73, cuda=False)
    x = U.frames(2, 64, 96, 73)
    seen, inner = [], oenc._bottleneck

    def spy(*a, **k):
        seen.append(inner(*a, **k))
        return seen[-1]
    monkeypatch.setattr(oenc, "_bottleneck", spy)
    oenc.resnet_fpn(x, {"backbone." + k: v for k, v in sd.items()}, "R-50-FPN")
    r = bottleneck_stages_f64(bb, x)
    assert len(seen) == len(r["block_out"]) == len(r["conv1_out"]) == 16
    for i, (o, h) in enumerate(zip(seen, r["block_out"])):
        assert o.shape == h.shape
        assert float((o.double() - h).abs().max()) <= 1e-5 * float(h.abs().max()), "block %d" % i
    for st, i in enumerate((2, 6, 12, 15)):
        assert r["stage_out"][st] is r["block_out"][i]
    # conv1 outputs: the helper's own blocks recomputed from them (conv2, conv3, shortcut) give the block outputs the oracle confirmed
    f = {k: (w.double(), b.double()) for k, (w, b) in bb.folded_state().items()}
    xin = r["stem"]
    for i, blk in enumerate(bb.blocks()):
        z = r["conv1_out"][i]
        assert z.shape[1] == blk.conv1.out_channels and float(z.min()) >= 0
        m = torch.relu(torch.nn.functional.conv2d(z, *f["b%d.conv2" % i], padding=1))
        idt = torch.nn.functional.conv2d(xin, *f["b%d.down" % i], stride=blk.stride) if blk.downsample is not None else xin
        assert torch.equal(torch.relu(torch.nn.functional.conv2d(m, *f["b%d.conv3" % i]) + idt), r["block_out"][i])
        xin = r["block_out"][i]


@pytest.mark.parametrize("stress,g", [(False, 1.0), (True, 1e-4), (True, 1.0), (True, 5.0)])
@pytest.mark.parametrize("stage", [0, 1, 2])
def test_gpu_cases_leave_few_channels_identically_zero(stage, stress, g):
    bb, sd = U.tiny_backbone(stage, stress)
    if g != 1.0:
        U.load(bb, U.scale_network(sd, g))
    for shape in (SHAPES if not stress else [(33, 32, 32)]):
        for seed in ((U.SEED, U.SEED + 1) if not stress else (U.SEED,)):
            r = U.reference(bb, U.frames(*shape, seed=seed, scale=g), stage)
            for k in ("B", "M1", "Cst"):
                assert U.dead_share(r[k]) <= 0.10, (shape, seed, k, U.dead_share(r[k]))
            live = r["stage_in"][r["stage_in"] > 0]
            print("[fused cases] stage %d stress %s g %g %s: stage input median %.3g max %.3g" % (stage + 1, stress, g, shape, float(live.median()), float(live.max())))


@pytest.mark.parametrize("stage", [0, 1, 2])
def test_overflow_case_has_positions_over_the_range_and_inside_it(stage):
    x = U.frames(33, 32, 32, U.SEED)
    bb, sd, channel, factor, over, inside, ref = U.overflow_network(stage, x)
    B = ref["B"]
    assert int(over.sum()) > 0 and int(inside.sum()) > 0 and not bool((over & inside).any())
    assert float(B.max()) == pytest.approx(8 * U.F16X3_INF, rel=1e-3) and float(B.max()) < 1e-30 * float(np.finfo(np.float32).max)
    others = torch.ones(B.shape[0], dtype=torch.bool)
    others[channel] = False
    assert float(B[others].max()) < 0.1 * U.F16X3_MAX           # the raised channel alone leaves the range
    print("[fused cases] stage %d: channel %d x %.4g, %d positions over, %d inside, %d at the boundary" % (stage + 1, channel, factor, int(over.sum()), int(inside.sum()),
                                                                                                     over.numel() - int(over.sum()) - int(inside.sum())))
