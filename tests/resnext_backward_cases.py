"""The case lists of the ResNeXt backward tests (tests/test_resnext_backward_host.py, tests/test_gpu_resnext_backward.py): the grouped /
strided 3x3 convolution's (groups, channels per group, stride) and maps, the blocks, the composed bodies and the backbones."""
from tests import body_backward_oracle as BO

# (groups, channels per group): every per-group width small, many groups, one group
GROUPED = ((4, 4), (2, 8), (2, 16), (2, 32), (2, 64), (32, 8), (64, 4))
ONE_GROUP = ((1, 32), (1, 64), (1, 128))
# grouped cases at stride 1 and 2, one group at stride 2, plus (1, 32) at stride 1: the cross-check against conv2d_wgrad
CONV_CASES = tuple((g, cg, s) for g, cg in GROUPED for s in (1, 2)) + tuple((g, cg, 2) for g, cg in ONE_GROUP) + ((1, 32, 1),)
# (F, H, W) of the INPUT map: the smallest map with a stride-2 output of 1 x 2; odd and ragged; several tiles per row (32 columns), a ragged last
# tile, more than one K chunk
WGRAD_MAPS = ((1, 2, 4), (3, 13, 37), (2, 40, 70))
LARGEST = (2, 40, 70)


def dgrad_map(Fr, H, W, stride):
    """The data gradient at stride 2 composes ``scatter2``: even H and W (13 x 37 -> 12 x 38)."""
    return (Fr, H, W) if stride == 1 or (H % 2 == 0 and W % 2 == 0) else (Fr, H - 1, W + 1)


LEAK_WIDTHS = ((4, 4), (2, 8), (2, 16))                   # groups do not leak: 4, 8 and 16 channels per group

# one block: (kind, Cin, mid, Cout, stride, groups, stride_in_3x3)
BLOCKS = (("grouped projection", 64, 32, 128, 1, 4, False), ("grouped identity", 128, 32, 128, 1, 2, False),
          ("grouped stride-in-3x3", 128, 64, 256, 2, 16, True), ("one-group stride-in-3x3", 128, 64, 256, 2, 1, True))
BLOCK_F, BLOCK_HW = BO.BLOCK_F, BO.BLOCK_HW               # F 1 and 3; maps 1x2, 3x5, 8x16 after the stride

# the composed bodies: (name, groups, stride_in_3x3, stages (blocks, mid, Cout)); input 32 channels at 2 x 16 x 32
STAGES_A = ((2, 32, 64), (3, 64, 128), (2, 128, 256))     # groups 4: 8, 16 and 32 channels per group
BODIES = (("A", 4, True, STAGES_A), ("B", 4, False, STAGES_A), ("C", 1, True, BO.BODY_STAGES))
BODY_LEVELS = ((1, 2, 3), (3,))
BODY_FREEZE = (2, 4)

# the recompute against the pass: (tag, backbone type, groups, width per group, stride in the 1x1)
BACKBONES = (("X50_32x4d", "R-50-FPN", 32, 4, True), ("R50_s3", "R-50-FPN", 1, 64, False))
RECOMPUTE_FRAMES = (4, 64, 96)
