"""ResNeXt / stride-in-3x3 backbones on the host side (no GPU): MODEL.RESNETS.NUM_GROUPS, WIDTH_PER_GROUP and STRIDE_IN_1X1 build the
reference's network (state-dict keys and shapes of tests/golden/encoder_resnext.npz, made from the reference by tools/make_goldens.py),
the folded network restated in fp64 reproduces the reference's outputs, unsupported keys fail loudly, and the library takes both sizes
of StemsegEncoderDesc."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import synth
from tests.resnext_ref import folded_resnet_fpn_f64

CASES = ["X50_32x4d", "X101_32x8d_s3", "R50_s3"]
TYPES = {"X50_32x4d": "R-50-FPN", "X101_32x8d_s3": "R-101-FPN", "R50_s3": "R-50-FPN"}


def _backbone(g, tag):
    from stemseg_amd.modeling.backbone import ResNetFPN
    H, W, seed, stride, groups, width, s1x1 = g[tag + "__meta"].tolist()
    return ResNetFPN(TYPES[tag], 256, groups, width, bool(s1x1)).eval(), (H, W, seed, stride)


def _cfg(btype="R-101-FPN", **resnets):
    from stemseg_amd import config
    c = config.make_cfg()
    c.MODEL.BACKBONE.TYPE = btype
    for k, v in resnets.items():
        setattr(c.MODEL.RESNETS, k, v)
    return c


@pytest.mark.parametrize("tag", CASES)
def test_state_dict_keys_and_shapes_equal_the_reference(golden, tag):
    g = golden("encoder_resnext")
    bb, _ = _backbone(g, tag)
    got = ["%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in bb.state_dict().items()]
    assert got == g[tag + "__keys"].tolist()


@pytest.mark.parametrize("tag", CASES)
def test_build_model_reads_the_resnets_keys(golden, tag):
    from stemseg_amd.modeling.backbone import build_resnet_fpn_backbone
    g = golden("encoder_resnext")
    _, _, _, _, groups, width, s1x1 = g[tag + "__meta"].tolist()
    bb = build_resnet_fpn_backbone(_cfg(TYPES[tag], NUM_GROUPS=groups, WIDTH_PER_GROUP=width, STRIDE_IN_1X1=bool(s1x1)))
    got = ["%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in bb.state_dict().items()]
    assert got == g[tag + "__keys"].tolist()
    d = bb._desc(2, 64, 96)
    assert (d.conv2_groups, d.width_per_group, d.stride_in_3x3) == (groups, width, int(not s1x1))


@pytest.mark.parametrize("tag", CASES)
def test_folded_network_fp64_matches_the_reference(golden, tag):
    g = golden("encoder_resnext")
    bb, (H, W, seed, stride) = _backbone(g, tag)
    sd = {k: torch.from_numpy(np.asarray(synth.synth_param("backbone." + k, v.shape, seed))).reshape(v.shape) for k, v in bb.state_dict().items()}
    bb.load_state_dict(sd)
    x = synth.synth_frames(2, H, W, seed=seed).astype(np.float32)
    x = torch.from_numpy(x).permute(0, 3, 1, 2) - torch.tensor([102.9801, 115.9465, 122.7717])[None, :, None, None]
    outs = folded_resnet_fpn_f64(bb, x)
    for s in (4, 8, 16, 32):
        ref = g["%s_s%d" % (tag, s)]
        assert list(outs[s].shape) == g["%s_s%d__shape" % (tag, s)].tolist()
        got = outs[s].numpy().reshape(-1)[::stride]
        scale = max(1.0, float(np.abs(ref).max()))
        assert float(np.abs(got - ref).max()) / scale <= 1e-4, (tag, s)


def test_default_keys_build_the_default_network():
    from stemseg_amd.modeling.backbone import build_resnet_fpn_backbone, ResNetFPN
    c = _cfg("R-50-FPN")
    c.MODEL.RESNETS = NS(BACKBONE_OUT_CHANNELS=256)          # a cfg without the architecture keys: the reference's defaults
    bb = build_resnet_fpn_backbone(c)
    ref = ResNetFPN("R-50-FPN")
    assert [(k, v.shape) for k, v in bb.state_dict().items()] == [(k, v.shape) for k, v in ref.state_dict().items()]
    d = bb._desc(2, 64, 96)
    assert (d.conv2_groups, d.width_per_group, d.stride_in_3x3) == (1, 64, 0)


@pytest.mark.parametrize("key,value", [("STEM_OUT_CHANNELS", 32), ("RES2_OUT_CHANNELS", 128), ("WIDTH_PER_GROUP", 16),
                                       ("WIDTH_PER_GROUP", 2), ("WIDTH_PER_GROUP", 128)])
def test_unsupported_resnets_keys_raise(key, value):
    from stemseg_amd.modeling.backbone import build_resnet_fpn_backbone
    kw = {key: value}
    if key == "WIDTH_PER_GROUP" and value != 128:
        kw["NUM_GROUPS"] = 32
    with pytest.raises(NotImplementedError, match=key):
        build_resnet_fpn_backbone(_cfg("R-50-FPN", **kw))


@pytest.mark.parametrize("key", ["USE_GN", "USE_RELU"])
def test_fpn_gn_and_relu_raise(key):
    from stemseg_amd.modeling.backbone import build_resnet_fpn_backbone
    c = _cfg("R-50-FPN")
    c.MODEL.FPN = NS(USE_GN=False, USE_RELU=False)
    setattr(c.MODEL.FPN, key, True)
    with pytest.raises(NotImplementedError, match=key):
        build_resnet_fpn_backbone(c)


def test_x101_type_string_keeps_raising_keyerror():
    from stemseg_amd.modeling.backbone import build_resnet_fpn_backbone
    with pytest.raises(KeyError):
        build_resnet_fpn_backbone(_cfg("X-101-FPN", NUM_GROUPS=32, WIDTH_PER_GROUP=8, STRIDE_IN_1X1=False))


def _enc_desc(hip, nbytes):
    e = hip.EncoderDesc()
    e.struct_bytes = nbytes
    for i, n in enumerate((3, 4, 23, 3)):
        e.blocks[i] = n
    e.T, e.H, e.W, e.out_channels, e.precision, e.n_clips = 8, 480, 864, 256, 0, 1
    return e


def test_encoder_descriptor_sizes():
    from stemseg_amd import hip
    lib = hip.lib()
    new = ctypes.sizeof(hip.EncoderDesc)
    old = hip.EncoderDesc.conv2_groups.offset
    assert new == old + 12 and old == 60
    e_new, e_old = _enc_desc(hip, new), _enc_desc(hip, old)
    base = lib.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e_new))
    assert base > 0 and lib.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e_old)) == base     # old size = today's network
    e_new.conv2_groups, e_new.width_per_group = 1, 64
    assert lib.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e_new)) == base
    offs_a, offs_b = (ctypes.c_int64 * 25)(), (ctypes.c_int64 * 25)()
    assert lib.stemseg_hip_encoder_plan_offsets(ctypes.byref(e_old), offs_a) == 0
    assert lib.stemseg_hip_encoder_plan_offsets(ctypes.byref(e_new), offs_b) == 0
    assert list(offs_a) == list(offs_b)
    for bad in (old - 4, new + 4, new - 4):
        assert lib.stemseg_hip_encoder_workspace_bytes(ctypes.byref(_enc_desc(hip, bad))) == 0
        assert b"descriptor size" in lib.stemseg_hip_last_error()
    # ResNeXt-101 32x8d: M1 / M2 sized for 256 << s bottleneck channels; stride in the 3x3 adds the previous-resolution conv1 buffers
    e_new.conv2_groups, e_new.width_per_group = 32, 8
    x = lib.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e_new))
    assert x > base + (256 - 64) * 8 * 120 * 216 * 4
    e_new.stride_in_3x3 = 1
    assert lib.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e_new)) > x + 512 * 8 * 122 * 220 * 4
    for groups, width in ((32, 16), (32, 2), (1, 32), (3, 8)):
        e_new.conv2_groups, e_new.width_per_group = groups, width
        assert lib.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e_new)) == 0, (groups, width)
    e_new.conv2_groups, e_new.width_per_group, e_new.stride_in_3x3 = 32, 8, 2
    assert lib.stemseg_hip_encoder_workspace_bytes(ctypes.byref(e_new)) == 0


def test_grouped_packed_weight_bytes():
    from stemseg_amd import hip
    lib = hip.lib()
    P = hip.PRECISIONS
    # per 16 output channels and 16-channel chunk of the window (max(16, channels per group)): f32 9 taps x 16 x 16 floats; split modes
    # 5 k-steps x 3 planes x 64 lanes x 16 B (+ f16x3: 8 B per output channel)
    assert lib.stemseg_hip_packed_grouped_weight_bytes(256, 8, 32, P["f32"]) == 16 * 1 * 9 * 256 * 4
    assert lib.stemseg_hip_packed_grouped_weight_bytes(256, 8, 32, P["bf16x6"]) == 16 * 1 * 5 * 3 * 64 * 16
    assert lib.stemseg_hip_packed_grouped_weight_bytes(2048, 64, 32, P["f16x3"]) == 128 * 4 * 5 * 3 * 64 * 16 + 8 * 2048
    assert lib.stemseg_hip_packed_grouped_weight_bytes(512, 512, 1, P["f32"]) == 32 * 32 * 9 * 256 * 4
    for Cout, Cg, groups, prec in ((256, 16, 32, P["f32"]), (96, 3, 32, P["f32"]), (256, 128, 2, P["f32"]), (256, 8, 32, 1), (24, 24, 1, P["f32"])):
        assert lib.stemseg_hip_packed_grouped_weight_bytes(Cout, Cg, groups, prec) == 0, (Cout, Cg, groups, prec)
