"""Host tests of the ResNeXt body backward (csrc/conv_backward.hip conv2d_grouped_wgrad behind hip.conv2d_grouped_wgrad / conv2d_grouped_dgrad
and the ``groups`` / ``stride_in_3x3`` keys of encoder_backward.bottleneck_backward / body_stage_forward / body_backward; ResNetFPN.train_resnext;
TrainingModel.train_resnext; training.utils.configure_trainable): the C-ABI and its argument checks (every one is made before any GPU call),
the plan functions, the oracle of the GPU tests against the mathematics written out, and the switch.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import decoder_tail_oracle as TO
from tests import resnext_backward_cases as RC
from tests import resnext_backward_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stemseg_hip_conv2d_grouped_wgrad_workspace_bytes", "stemseg_hip_conv2d_grouped_wgrad_chunks", "stemseg_hip_conv2d_grouped_wgrad")


def test_symbols_exported_declared_and_bound():
    from stemseg_amd import hip
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    for n in NAMES:
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in header and hip.lib().stemseg_hip_version() == 11 and hip.ABI_VERSION == 11
    for f in ("conv2d_grouped_wgrad_chunks", "conv2d_grouped_wgrad", "conv2d_grouped_dgrad", "grouped_dgrad_weight"):
        assert callable(getattr(hip, f)), f


def test_calls_reject_bad_arguments_before_any_gpu_call():
    from stemseg_amd import hip
    l = hip.lib()
    err = l.stemseg_hip_last_error
    fake = ctypes.c_void_p(256)
    Cn, Fr, H, W = 32, 2, 4, 6
    pitch = 8
    ts = (H + 2) * pitch
    cs = Fr * ts

    def vol(ptr=256, C=Cn, dims=(Fr, H + 2, W + 2), strides=(cs, ts, pitch), limit=None):
        return hip.Volume(ptr, strides[0], strides[1], strides[2], C, dims[0], dims[1], dims[2], C * cs if limit is None else limit)

    def call(x="vol", dy=fake, C=Cn, groups=2, stride=1, dw=fake, ws=fake, ws_bytes=1 << 30):
        xv = vol() if isinstance(x, str) else x
        return l.stemseg_hip_conv2d_grouped_wgrad(ctypes.byref(xv) if xv is not None else None, dy, C, groups, stride, dw, ws, ws_bytes, None)

    assert call(x=None) == -1 and b"conv2d_grouped_wgrad: x_haloed is a null pointer" in err()
    assert call(x=vol(ptr=None)) == -1 and b"x_haloed is a null pointer" in err()
    assert call(dy=None) == -1 and b"conv2d_grouped_wgrad: dy is a null pointer" in err()
    assert call(dw=None) == -1 and b"conv2d_grouped_wgrad: dw is a null pointer" in err()
    assert call(ws=None) == -1 and b"conv2d_grouped_wgrad: workspace is a null pointer" in err()
    assert call(x=vol(dims=(Fr, 2, W + 2))) == -1 and b"x must be the y/x-haloed view" in err()
    assert call(C=48) == -1 and b"x has 32 channels, C = 48" in err()
    assert call(x=vol(C=24), C=24, groups=1) == -1 and b"C = 24 is no multiple of 16" in err()
    assert call(x=vol(C=48), C=48, groups=4) == -1 and b"12 channels per group unsupported (4, 8, 16, 32, 64; one group: a multiple of 16)" in err()
    assert call(groups=16) == -1 and b"2 channels per group unsupported" in err()
    assert call(groups=3) == -1 and b"32 channels in 3 groups" in err()
    assert call(stride=3) == -1 and b"conv2d_grouped_wgrad: stride 3 (1 or 2)" in err()
    assert call(x=vol(strides=(cs, ts, W))) == -1 and b"strides of x do not hold its extents" in err()
    assert call(x=vol(limit=Cn * cs - ts)) == -1 and b"x reaches past its limit" in err()
    assert call(ws=ctypes.c_void_p(264)) == -1 and b"workspace must be 256-byte aligned" in err()
    need = l.stemseg_hip_conv2d_grouped_wgrad_workspace_bytes(Cn, 2, 1, Fr, H, W)
    assert need == 9 * Cn * 16 * 8
    assert call(ws_bytes=need - 1) != 0 and b"conv2d_grouped_wgrad: workspace too small (%d < %d bytes)" % (need - 1, need) in err()
    # the plan functions refuse the same shapes
    assert l.stemseg_hip_conv2d_grouped_wgrad_workspace_bytes(24, 1, 1, Fr, H, W) == 0 and b"no multiple of 16" in err()
    assert l.stemseg_hip_conv2d_grouped_wgrad_chunks(32, 2, 3, Fr, H, W) < 0 and b"stride 3" in err()
    assert l.stemseg_hip_conv2d_grouped_wgrad_chunks(32, 2, 1, 0, H, W) < 0 and b"bad dims" in err()


def test_python_wrappers_name_the_bad_argument():
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward as EB
    xv = hip.Volume(256, 2 * 6 * 8, 6 * 8, 8, 32, 2, 6, 8, 32 * 96)               # the haloed view of [32][2][4][6]
    with pytest.raises(ValueError, match=r"conv2d_grouped_wgrad: dy \(32, 2, 4, 5\) does not fit the haloed input view \[32\]\(2, 6, 8\) at stride 1"):
        hip.conv2d_grouped_wgrad(xv, torch.zeros(32, 2, 4, 5), 2, 1)
    with pytest.raises(ValueError, match=r"does not fit the haloed input view .* at stride 2 \(expected \(32, 2, 2, 3\)\)"):
        hip.conv2d_grouped_wgrad(xv, torch.zeros(32, 2, 4, 6), 2, 2)
    with pytest.raises(ValueError, match=r"conv2d_grouped_wgrad: stride 3"):
        hip.conv2d_grouped_wgrad(xv, torch.zeros(32, 2, 4, 6), 2, 3)
    with pytest.raises(ValueError, match=r"conv2d_grouped_wgrad: 2 channels per group unsupported"):
        hip.conv2d_grouped_wgrad(xv, torch.zeros(32, 2, 4, 6), 16, 1)
    with pytest.raises(ValueError, match=r"conv2d_grouped_wgrad: 24 channels in 1 groups"):
        hip.conv2d_grouped_wgrad(hip.Volume(256, 96, 48, 8, 24, 2, 6, 8, 24 * 96), torch.zeros(24, 2, 4, 6), 1, 1)
    dy, w = torch.zeros(32, 2, 2, 3), torch.zeros(32, 16, 3, 3)
    with pytest.raises(ValueError, match=r"conv2d_grouped_dgrad: precision 'f16x3'"):
        hip.conv2d_grouped_dgrad(dy, w, 2, 2, "f16x3")
    with pytest.raises(ValueError, match=r"conv2d_grouped_dgrad: w .* against dy"):
        hip.conv2d_grouped_dgrad(dy, torch.zeros(16, 16, 3, 3), 2, 2)
    with pytest.raises(ValueError, match=r"conv2d_grouped_dgrad: w .* holds 16 channels per group, 4 groups of 32 channels need 8"):
        hip.conv2d_grouped_dgrad(dy, w, 4, 2)
    with pytest.raises(ValueError, match=r"conv2d_grouped_dgrad: stride 3"):
        hip.conv2d_grouped_dgrad(dy, w, 2, 3)
    # odd H or W at stride 2: the map of a1 is 3 x 6 / 4 x 5, its stride-2 output 2 x 3
    for Hm, Wm in ((3, 6), (4, 5)):
        with pytest.raises(ValueError, match=r"conv2d_grouped_dgrad: stride 2 needs even H and W, the mask is %d x %d" % (Hm, Wm)):
            hip.conv2d_grouped_dgrad(dy, w, 2, 2, "f32", mask=hip.Volume(256, 2 * Hm * Wm, Hm * Wm, Wm, 32, 2, Hm, Wm, 32 * 2 * Hm * Wm))
    with pytest.raises(ValueError, match=r"conv2d_grouped_dgrad: mask \[32\]\(2, 4, 7\)"):
        hip.conv2d_grouped_dgrad(dy, w, 2, 2, "f32", mask=hip.Volume(256, 56, 28, 7, 32, 2, 4, 7, 32 * 56))
    weights = dict(conv1=torch.zeros(32, 64, 1, 1), conv2=torch.zeros(32, 8, 3, 3), conv3=torch.zeros(128, 32, 1, 1), down=None, groups=4)
    xv = hip.Volume(256, 30, 15, 5, 64, 2, 3, 5, 64 * 30)
    G = torch.zeros(128, 2, 3, 5)
    with pytest.raises(ValueError, match="identity block needs Cin == Cout"):
        EB.bottleneck_backward(xv, {}, G, weights, "f32")
    with pytest.raises(ValueError, match=r"are no bottleneck of 2 groups"):
        EB.bottleneck_backward(xv, {}, G, dict(weights, groups=2, down=torch.zeros(128, 64, 1, 1)), "f32")
    with pytest.raises(ValueError, match=r"stride in the 3x3: twice its map"):
        EB.bottleneck_backward(xv, {}, G, dict(weights, stride_in_3x3=True, down=torch.zeros(128, 64, 1, 1)), "f32")
    with pytest.raises(ValueError, match=r"addend_x joins the gradient of a stride-in-3x3 block only"):
        EB.bottleneck_backward(xv, {}, G, dict(weights, down=torch.zeros(128, 64, 1, 1)), "f32", addend_x=torch.zeros(64, 2, 3, 5))
    with pytest.raises(ValueError, match=r"addend_x joins the gradient of a stride-in-3x3 block only"):
        EB.bottleneck_backward(xv, {}, G, dict(weights, groups=1, conv2=torch.zeros(32, 32, 3, 3)), "f32", addend_x=torch.zeros(64, 2, 3, 5))


def test_chunks_and_workspace_are_functions_of_the_shape():
    from stemseg_amd import hip
    l = hip.lib()
    seen = {}
    for g, cg, s in RC.CONV_CASES:
        for Fr, H, W in RC.WGRAD_MAPS:
            a = (g * cg, g, s, Fr, H, W)
            n, b = hip.conv2d_grouped_wgrad_chunks(*a), l.stemseg_hip_conv2d_grouped_wgrad_workspace_bytes(*a)
            assert n >= 1 and b == n * 9 * g * cg * cg * 8, a
            assert (n, b) == (hip.conv2d_grouped_wgrad_chunks(*a), l.stemseg_hip_conv2d_grouped_wgrad_workspace_bytes(*a))
            seen[a] = n
    for g, cg, s in RC.CONV_CASES:
        assert seen[(g * cg, g, s) + RC.LARGEST] > 1, (g, cg, s)
    assert seen[(16, 4, 1, 1, 2, 4)] == 1
    with pytest.raises(ValueError, match="conv2d_grouped_wgrad: stride 3"):
        hip.conv2d_grouped_wgrad_chunks(32, 2, 3, 1, 4, 4)


@pytest.mark.parametrize("g,cg,s", [(2, 8, 1), (2, 8, 2), (4, 4, 2), (1, 32, 2), (2, 16, 2)])
def test_oracle_convolution_is_the_mathematics_written_out(g, cg, s):
    """fp64 autograd against the dW formula of the header and against the flipped, per-group transposed (and zero-dilated) forward convolution
    for dx; 13 x 37 for dW (odd and ragged), 12 x 38 for dx at stride 2."""
    Fr, H, W = RC.WGRAD_MAPS[1]
    case = RO.conv_case(g, cg, s, Fr, H, W)
    r = RO.conv_oracle(case, torch.float64)
    assert np.abs(RO.dw_formula(case) - r["dw"]).max() <= 1e-13 * np.abs(r["dw"]).max()
    Fr, H, W = RC.dgrad_map(Fr, H, W, s)
    case = RO.conv_case(g, cg, s, Fr, H, W)
    r = RO.conv_oracle(case, torch.float64)
    assert r["dx"].shape == (g * cg, Fr, H, W)
    assert np.abs(RO.dx_formula(case, H, W) - r["dx"]).max() <= 1e-13 * np.abs(r["dx"]).max()


def test_dgrad_weight_of_the_binding_is_the_oracles():
    from stemseg_amd import hip
    rng = np.random.default_rng(3)
    for g, cg in ((4, 4), (2, 16), (1, 32)):
        w = rng.standard_normal((g * cg, cg, 3, 3)).astype(np.float32)
        assert np.array_equal(hip.grouped_dgrad_weight(torch.from_numpy(w), g).numpy(), RO.dgrad_weight(w, g))


@pytest.mark.parametrize("g,cg,s", RC.CONV_CASES)
def test_every_case_has_a_gradient_and_a_spread(g, cg, s):
    """Every case's reference gradients are non-zero and its fp32-vs-fp64 spread is positive: the rule bites."""
    for Fr, H, W in RC.WGRAD_MAPS:
        for what, dims in (("dw", (Fr, H, W)), ("dx", RC.dgrad_map(Fr, H, W, s))):
            case = RO.conv_case(g, cg, s, *dims)
            r32, r64 = RO.conv_oracle(case, torch.float32), RO.conv_oracle(case, torch.float64)
            spread = TO.max_norm_err(r32[what], r64[what])
            print("(%d, %d) s%d %s %s: spread %.2e bound %.2e" % (g, cg, s, dims, what, spread, TO.bound(spread, r64[what])))
            assert np.abs(r64[what]).max() > 0 and 0 < spread < 1e-4, (what, dims)


def test_oracle_block_with_the_stride_in_the_3x3_is_the_mathematics_written_out():
    """fp64: the chain of a stride-in-3x3 projection block against autograd -- grouped and one group -- and pinning the activations changes nothing."""
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    for kind, Cin, mid, Cout, stride, groups, s3 in RC.BLOCKS[2:]:
        case = RO.block_case(kind, Cin, mid, Cout, stride, groups, s3, 2, 3, 5)
        g, acts = RO.block_gradients(case, torch.float64)
        g2, _ = RO.block_gradients(case, torch.float64, {k: v.numpy() for k, v in acts.items()})
        assert all(np.abs(g[n] - g2[n]).max() <= 1e-13 * max(1.0, np.abs(g[n]).max()) for n in g), kind
        p = case["params"]
        Wf = {n: t(p[n]) * t(p[n + ".s"])[:, None, None, None] for n in RO.CONVS}
        x = t(case["x"])
        xs2 = x[:, :, ::2, ::2]
        a1, a2, out = (acts[k].double() for k in ("a1", "a2", "out"))
        assert a1.shape[2:] == x.shape[2:] and a2.shape[2:] == xs2.shape[2:]
        g3 = (out > 0) * t(case["g"])
        wgrad1 = lambda v, dy: torch.einsum("ofhw,ifhw->oi", dy, v)[:, :, None, None]
        dgrad1 = lambda dy, w: torch.einsum("ofhw,oi->ifhw", dy, w[:, :, 0, 0])
        g_a2 = (a2 > 0) * dgrad1(g3, Wf["conv3"])
        c2 = dict(x=a1.numpy(), w=Wf["conv2"].numpy(), g=g_a2.numpy(), groups=groups, stride=2)
        g_a1 = (a1 > 0) * torch.from_numpy(RO.dx_formula(c2, *a1.shape[2:]))
        side = torch.zeros_like(x)
        side[:, :, ::2, ::2] = dgrad1(g3, Wf["down"])                            # scatter2
        want = {"conv3": wgrad1(a2, g3), "conv2": torch.from_numpy(RO.dw_formula(c2)), "conv1": wgrad1(x, g_a1), "down": wgrad1(xs2, g3)}
        for n, v in want.items():
            v = v * t(p[n + ".s"])[:, None, None, None]
            assert np.abs(v.numpy() - g[n]).max() <= 1e-12 * np.abs(g[n]).max(), (kind, n)
        gx = dgrad1(g_a1, Wf["conv1"]) + side
        assert g["g_x"].shape == tuple(x.shape) and np.abs(gx.numpy() - g["g_x"]).max() <= 1e-12 * np.abs(g["g_x"]).max(), kind


OLD_GROUPS = "MODEL.RESNETS.NUM_GROUPS=32: the body's backward has no grouped-convolution backward (NUM_GROUPS=1 only)"
OLD_STRIDE = ("MODEL.RESNETS.STRIDE_IN_1X1=False: the body's backward has no backward of the stride-2 3x3 convolution "
              "(STRIDE_IN_1X1=True only)")


def test_the_switch_on_the_backbone():
    from stemseg_amd.modeling.backbone import ResNetFPN
    x32 = ResNetFPN("R-50-FPN", num_groups=32, width_per_group=8)
    s3 = ResNetFPN("R-50-FPN", stride_in_1x1=False)
    assert x32.train_resnext is False and s3.train_resnext is False
    for bb, msg in ((x32, OLD_GROUPS), (s3, OLD_STRIDE)):
        with pytest.raises(NotImplementedError) as e:
            bb.body_parameter_list(2)
        assert str(e.value) == msg
    for bb, groups in ((x32, 32), (s3, 1)):
        bb.train_resnext = True
        names = {id(p): n for n, p in bb.named_parameters()}
        got = [names[id(p)] for p in bb.body_parameter_list(2)]
        assert got == [n for n, _ in bb.named_parameters() if any(n.startswith("body.layer%d." % st) for st in (2, 3, 4))]
        assert got[:4] == ["body.layer2.0.downsample.0.weight", "body.layer2.0.conv1.weight", "body.layer2.0.conv2.weight", "body.layer2.0.conv3.weight"]
        for st in (2, 3, 4):
            for blk in getattr(bb.body, "layer%d" % st):
                mid = blk.conv2.weight.shape[0]
                assert tuple(blk.conv2.weight.shape) == (mid, mid // groups, 3, 3) and mid == groups * bb.width_per_group * 2 ** (st - 1)
        for fa in (1, 0, 5):
            with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE=%d" % fa):
                bb.body_parameter_list(fa)
        bb.train_resnext = False
        with pytest.raises(NotImplementedError):
            bb.body_parameter_list(2)
    plain = ResNetFPN("R-50-FPN")
    plain.train_resnext = True
    assert len(plain.body_parameter_list(2)) == 42


def _cfg_model(groups=1, width=64, s1x1=True, freeze_at=2):
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    config.load_preset("kittimots")
    config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
    r = config.cfg.MODEL.RESNETS
    r.NUM_GROUPS, r.WIDTH_PER_GROUP, r.STRIDE_IN_1X1 = groups, width, s1x1
    config.cfg.MODEL.BACKBONE.FREEZE_AT_STAGE = freeze_at
    return build_model(), config.cfg


def test_configure_trainable_sets_the_switch_for_a_resnext_cfg():
    from stemseg_amd import config
    from stemseg_amd.training.utils import configure_trainable
    try:
        m, cfg = _cfg_model(32, 4)
        assert m.train_resnext is False and m.backbone.train_resnext is False
        with pytest.raises(NotImplementedError) as e:
            m.body_parameters(2)
        assert str(e.value) == OLD_GROUPS.replace("=32", "=32")
        configure_trainable(m, cfg, freeze_backbone=False)
        assert m.train_resnext is True and m.backbone.train_resnext is True and m.train_body is True
        assert len(m.body_parameters(2)) == 42 and m.body_fpn_and_decoders_only_trainable(2)
        m.train_resnext = False                                  # mirrored onto the backbone, both ways
        assert m.backbone.train_resnext is False
        m, cfg = _cfg_model(1, 64, False)
        configure_trainable(m, cfg, freeze_backbone=False)
        assert m.train_resnext is True and m.backbone.train_resnext is True
        m, cfg = _cfg_model()
        configure_trainable(m, cfg, freeze_backbone=False)
        assert m.train_resnext is False and m.backbone.train_resnext is False and m.train_body is True
        # a bad FREEZE_AT_STAGE is refused before anything changes
        m, cfg = _cfg_model(32, 4, True, freeze_at=1)
        before = [p.requires_grad for p in m.parameters()]
        with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE=1"):
            configure_trainable(m, cfg, freeze_backbone=False)
        assert m.train_resnext is False and m.backbone.train_resnext is False and m.train_body is False
        assert [p.requires_grad for p in m.parameters()] == before
    finally:
        config.load_preset("defaults")
