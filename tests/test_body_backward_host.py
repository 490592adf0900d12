"""Host tests of the body backward (csrc/bottleneck_backward.hip behind hip.relu_backward / subsample2 / scatter2 / scale_rows / conv1x1_dgrad and
encoder_backward.bottleneck_backward / body_stage_forward / body_backward; modeling.ops.EncoderFunction; ResNetFPN.forward_trainable_body;
TrainingModel.train_body): the oracle of the GPU tests against the block's mathematics written out, the C-ABI and its argument checks (every
one is made before any GPU call), the refusals and the gating of TrainingModel.forward behind the three switches.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import body_backward_oracle as BO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stemseg_hip_relu_backward", "stemseg_hip_conv2d_col2img_relu", "stemseg_hip_subsample2", "stemseg_hip_scatter2", "stemseg_hip_scale_rows",
         "stemseg_hip_sum_partials")


def test_symbols_exported_declared_and_bound():
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward, ops
    from stemseg_amd.modeling.backbone import ResNetFPN
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    for n in NAMES:
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in header and hip.lib().stemseg_hip_version() == 11 and hip.ABI_VERSION == 11
    for f in ("relu_backward", "subsample2", "scatter2", "scale_rows", "conv1x1_dgrad"):
        assert callable(getattr(hip, f)), f
    for f in ("bottleneck_backward", "body_stage_forward", "body_backward"):
        assert callable(getattr(encoder_backward, f)), f
    assert issubclass(ops.EncoderFunction, torch.autograd.Function)
    assert callable(ResNetFPN.forward_trainable_body) and callable(ResNetFPN.body_parameter_list)


def test_calls_reject_bad_arguments_before_any_gpu_call():
    from stemseg_amd import hip
    l = hip.lib()
    err = l.stemseg_hip_last_error
    fake = ctypes.c_void_p(256)
    Cn, Fr, H, W = 32, 2, 4, 6
    pitch = 8
    ts = (H + 2) * pitch
    cs = Fr * ts

    def vol(ptr=256 + 4 * (pitch + 1), C=Cn, dims=(Fr, H, W), strides=(cs, ts, pitch), limit=Cn * cs):
        return hip.Volume(ptr, strides[0], strides[1], strides[2], C, dims[0], dims[1], dims[2], limit)

    rb = lambda y="vol", g=fake, a=None, out=fake: l.stemseg_hip_relu_backward(ctypes.byref(vol() if isinstance(y, str) else y) if y is not None else None, g, a, out, None)
    assert rb(y=None) == -1 and b"y is a null pointer" in err()
    assert rb(y=vol(ptr=None)) == -1 and b"y is a null pointer" in err()
    assert rb(g=None) == -1 and b"g is a null pointer" in err()
    assert rb(out=None) == -1 and b"out is a null pointer" in err()
    assert rb(y=vol(dims=(Fr, 0, W))) == -1 and b"y has bad extents" in err()
    assert rb(y=vol(strides=(cs, ts, W - 1))) == -1 and b"strides of y do not hold its extents" in err()
    assert rb(y=vol(strides=(cs, ts - 3 * pitch, pitch))) == -1 and b"strides of y do not hold its extents" in err()
    assert rb(y=vol(strides=(cs - ts, ts, pitch))) == -1 and b"strides of y do not hold its extents" in err()
    assert rb(y=vol(limit=Cn * cs - ts)) == -1 and b"y reaches past its limit" in err()

    c2i = lambda cols=fake, dims=(Cn, Fr, H, W), m="vol", dx=fake: l.stemseg_hip_conv2d_col2img_relu(
        cols, dims[0], dims[1], dims[2], dims[3], None, ctypes.byref(vol() if isinstance(m, str) else m) if m is not None else None, dx, None)
    assert c2i(cols=None) == -1 and b"cols is a null pointer" in err()
    assert c2i(dx=None) == -1 and b"dx is a null pointer" in err()
    assert c2i(m=None) == -1 and b"mask is a null pointer" in err()
    assert c2i(dims=(Cn, 0, H, W)) == -1 and b"bad dims" in err()
    assert c2i(m=vol(strides=(cs, ts, W - 2))) == -1 and b"strides of mask do not hold its extents" in err()
    assert c2i(m=vol(limit=7)) == -1 and b"mask reaches past its limit" in err()
    assert c2i(m=vol(dims=(Fr, H, W - 1))) == -1 and b"mask is [32][2][4][5], expected [32][2][4][6]" in err()
    assert c2i(m=vol(C=Cn + 4, limit=(Cn + 4) * cs)) == -1 and b"mask is [36]" in err()

    for name, fn in (("subsample2", lambda a=fake, d=(Cn, Fr, H, W), o=fake: l.stemseg_hip_subsample2(a, d[0], d[1], d[2], d[3], o, None)),
                     ("scatter2", lambda a=fake, d=(Cn, Fr, H, W), o=fake: l.stemseg_hip_scatter2(a, d[0], d[1], d[2], d[3], None, o, None))):
        first = b"in" if name == "subsample2" else b"g"
        assert fn(a=None) == -1 and name.encode() + b": " + first + b" is a null pointer" in err()
        assert fn(o=None) == -1 and name.encode() + b": out is a null pointer" in err()
        assert fn(d=(Cn, Fr, 5, W)) == -1 and name.encode() + b": H and W of the large map must be even, got H=5, W=6" in err()
        assert fn(d=(Cn, Fr, H, 7)) == -1 and b"must be even, got H=4, W=7" in err()
        assert fn(d=(0, Fr, H, W)) == -1 and name.encode() + b": bad dims" in err()
        assert fn(d=(Cn, Fr, H, -2)) == -1 and b"bad dims" in err()
    sr = lambda dw=fake, s=fake, rows=4, n=9: l.stemseg_hip_scale_rows(dw, s, rows, n, None)
    assert sr(dw=None) == -1 and b"dw is a null pointer" in err()
    assert sr(s=None) == -1 and b"scale is a null pointer" in err()
    assert sr(rows=0) == -1 and b"rows" in err()
    assert sr(n=0) == -1 and b"row_len" in err()
    sp = lambda parts=fake, n=3, N=8, out=fake: l.stemseg_hip_sum_partials(parts, n, N, None, out, None)
    assert sp(parts=None) == -1 and b"parts is a null pointer" in err()
    assert sp(out=None) == -1 and b"out is a null pointer" in err()
    assert sp(n=0) == -1 and b"sum_partials: n must be" in err()
    assert sp(N=0) == -1 and b"sum_partials: bad N" in err()


def test_python_wrappers_name_the_bad_argument():
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward as EB
    y = hip.Volume(256, 2 * 12, 12, 4, 32, 2, 3, 4, 32 * 24)
    with pytest.raises(ValueError, match=r"relu_backward: g \(32, 2, 3, 5\)"):
        hip.relu_backward(y, torch.zeros(32, 2, 3, 5))
    with pytest.raises(ValueError, match="relu_backward: addend"):
        hip.relu_backward(y, torch.zeros(32, 2, 3, 4), torch.zeros(32, 2, 3))
    with pytest.raises(ValueError, match="subsample2: x .* needs even H and W"):
        hip.subsample2(torch.zeros(4, 1, 3, 4))
    with pytest.raises(ValueError, match="scatter2: addend"):
        hip.scatter2(torch.zeros(4, 1, 3, 4), torch.zeros(4, 1, 6, 7))
    with pytest.raises(ValueError, match="scale_rows: scale"):
        hip.scale_rows(torch.zeros(4, 3), torch.zeros(5))
    dy, w = torch.zeros(64, 2, 3, 5), torch.zeros(64, 32, 1, 1)
    with pytest.raises(ValueError, match=r"conv1x1_dgrad: precision 'f16x3'"):
        hip.conv1x1_dgrad(dy, w, "f16x3")
    with pytest.raises(ValueError, match="Cin = 4 is no multiple of 32"):
        hip.conv1x1_dgrad(dy, torch.zeros(64, 4, 1, 1))
    with pytest.raises(ValueError, match="against dy"):
        hip.conv1x1_dgrad(dy, torch.zeros(32, 32, 1, 1))
    with pytest.raises(ValueError, match="conv1x1_dgrad: addend"):
        hip.conv1x1_dgrad(dy, w, "f32", addend=torch.zeros(32, 2, 3, 6))
    with pytest.raises(ValueError, match="conv2d_dgrad: mask"):
        hip.conv2d_dgrad(torch.zeros(32, 2, 3, 4), torch.zeros(32, 32, 3, 3), "f32", mask=hip.Volume(256, 24, 12, 4, 32, 2, 3, 3, 32 * 24))
    weights = dict(conv1=torch.zeros(32, 64, 1, 1), conv2=torch.zeros(32, 32, 3, 3), conv3=torch.zeros(128, 32, 1, 1), down=None)
    xv = hip.Volume(256, 30, 15, 5, 64, 2, 3, 5, 64 * 30)
    with pytest.raises(ValueError, match="bottleneck_backward: precision 'f16x3'"):
        EB.bottleneck_backward(xv, {}, torch.zeros(128, 2, 3, 5), weights, "f16x3")
    with pytest.raises(ValueError, match="identity block needs Cin == Cout"):
        EB.bottleneck_backward(xv, {}, torch.zeros(128, 2, 3, 5), weights, "f32")
    with pytest.raises(ValueError, match="mid = 48 is no multiple of 32"):
        EB.bottleneck_backward(xv, {}, torch.zeros(128, 2, 3, 5), dict(weights, conv1=torch.zeros(48, 64, 1, 1)), "f32")
    with pytest.raises(ValueError, match="fpn_backward: want_dC needs inner_weights"):
        EB.fpn_backward([xv] * 4, [xv] * 4, [torch.zeros(32, 2, 8, 16)] * 4, [torch.zeros(32, 32, 3, 3)] * 4, "f32", want_dC=True)


MOVED = ("fpn_backward", "bottleneck_backward", "body_stage_forward", "body_backward")


def test_the_binding_holds_no_encoder_backward():
    """``hip`` is the binding: what knows the network's structure lives in modeling.encoder_backward, once, and the two grouped doubles are gone."""
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward
    for f in MOVED + ("_bottleneck_backward_grouped", "_grouped_block_forward", "_body_scratch"):
        assert not hasattr(hip, f), f
    for f in MOVED:
        assert callable(getattr(encoder_backward, f)), f
    for f in ("_bottleneck_backward_grouped", "_grouped_block_forward"):
        assert not hasattr(encoder_backward, f), f


def test_bottleneck_backward_refuses_in_the_pinned_order():
    """An addend_x without the stride in the 3x3 is refused before any shape is looked at, dense or grouped; an identity block with the stride in
    the 3x3 is refused as an identity block, naming the stride."""
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward as EB
    xv = hip.Volume(256, 30, 15, 5, 64, 2, 3, 5, 64 * 30)
    G, addend = torch.zeros(128, 2, 3, 5), torch.zeros(64, 2, 3, 5)
    dense = dict(conv1=torch.zeros(32, 64, 1, 1), conv2=torch.zeros(32, 32, 3, 3), conv3=torch.zeros(128, 32, 1, 1), down=None, groups=1)
    with pytest.raises(ValueError, match="addend_x joins the gradient of a stride-in-3x3 block only"):
        EB.bottleneck_backward(xv, {}, G, dense, "f32", addend_x=addend)
    grouped = dict(dense, conv2=torch.zeros(32, 8, 3, 3), down=torch.zeros(128, 64, 1, 1), groups=4)
    with pytest.raises(ValueError, match="addend_x joins the gradient of a stride-in-3x3 block only"):
        EB.bottleneck_backward(xv, {}, G, grouped, "f32", addend_x=addend)
    identity = dict(dense, conv1=torch.zeros(32, 128, 1, 1), stride_in_3x3=True)
    with pytest.raises(ValueError, match=r"identity block needs Cin == Cout and no stride, got 128 and 128, stride in the 3x3"):
        EB.bottleneck_backward(hip.Volume(256, 120, 60, 10, 128, 2, 6, 10, 128 * 120), {}, G, identity, "f32")


def test_refusals_name_the_config_key():
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward as EB
    from stemseg_amd.modeling.backbone import ResNetFPN
    bb = ResNetFPN("R-50-FPN")
    for fa in (1, 0, 5):
        with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE=%d" % fa):
            bb.body_parameter_list(fa)
        with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE"):
            EB.body_backward({}, {}, {}, "f32", freeze_at=fa)
    with pytest.raises(NotImplementedError, match=r"MODEL\.RESNETS\.NUM_GROUPS=32"):
        ResNetFPN("R-50-FPN", num_groups=32, width_per_group=8).body_parameter_list(2)
    with pytest.raises(NotImplementedError, match=r"MODEL\.RESNETS\.STRIDE_IN_1X1=False"):
        ResNetFPN("R-50-FPN", stride_in_1x1=False).body_parameter_list(2)
    with pytest.raises(NotImplementedError, match=r"MODEL\.RESNETS\.NUM_GROUPS"):
        ResNetFPN("R-50-FPN", num_groups=32, width_per_group=8).forward_trainable_body(torch.zeros(1, 3, 32, 32), 2)
    # network order: per block the projection (where there is one), conv1, conv2, conv3
    names = {id(p): n for n, p in bb.named_parameters()}
    got = [names[id(p)] for p in bb.body_parameter_list(3)]
    assert got == [n for n, _ in bb.named_parameters() if n.startswith("body.layer3.") or n.startswith("body.layer4.")]
    assert got[:4] == ["body.layer3.0.downsample.0.weight", "body.layer3.0.conv1.weight", "body.layer3.0.conv2.weight", "body.layer3.0.conv3.weight"]
    assert len(ResNetFPN("R-101-FPN").body_parameter_list(2)) == 13 + 70 + 10


def test_oracle_block_is_the_mathematics_written_out():
    """fp64: the chain of the issue -- g3 = relu'(out) G, dW3 = wgrad1(a2, g3), ... -- against autograd, on a stride-2 projection block and on an
    identity block; and pinning the activations to their own values changes nothing."""
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    ff = BO.frames_first
    for kind, Cin, mid, Cout, stride in (BO.BLOCKS[2], BO.BLOCKS[1]):
        case = BO.block_case(kind, Cin, mid, Cout, stride, 2, 3, 5)
        g, acts = BO.block_gradients(case, torch.float64)
        g2, _ = BO.block_gradients(case, torch.float64, {k: v.numpy() for k, v in acts.items()})
        assert all(np.abs(g[n] - g2[n]).max() <= 1e-13 * max(1.0, np.abs(g[n]).max()) for n in g), kind
        p = case["params"]
        W = {n: t(p[n]) * t(p[n + ".s"])[:, None, None, None] for n in BO.CONVS if n in p}
        xs = t(case["x"])[:, :, ::stride, ::stride]
        a1, a2, out = (acts[k].double() for k in ("a1", "a2", "out"))
        g3 = (out > 0) * t(case["g"])
        wgrad1 = lambda x, dy: torch.einsum("ofhw,ifhw->oi", dy, x)[:, :, None, None]
        dgrad1 = lambda dy, w: torch.einsum("ofhw,oi->ifhw", dy, w[:, :, 0, 0])
        g_a2 = (a2 > 0) * dgrad1(g3, W["conv3"])
        g_a1 = (a1 > 0) * ff(F.conv_transpose2d(ff(g_a2), W["conv2"], padding=1))
        dW2 = torch.einsum("ofyx,ifyxab->oiab", g_a2, F.pad(a1, (1, 1, 1, 1)).unfold(2, 3, 1).unfold(3, 3, 1))
        want = {"conv3": wgrad1(a2, g3), "conv2": dW2, "conv1": wgrad1(xs, g_a1)}
        gx = dgrad1(g_a1, W["conv1"])
        if "down" in W:
            want["down"] = wgrad1(xs, g3)
            gx = gx + dgrad1(g3, W["down"])
        else:
            gx = gx + g3
        for n, v in want.items():
            v = v * t(p[n + ".s"])[:, None, None, None]          # dW[co] = s[co] dW_folded[co]
            assert np.abs(v.numpy() - g[n]).max() <= 1e-12 * np.abs(g[n]).max(), (kind, n)
        assert np.abs(gx.numpy() - g["g_x"]).max() <= 1e-12 * np.abs(g["g_x"]).max(), kind


def test_oracle_given_values_carry_the_device_mask():
    """A given activation decides the mask, whatever the oracle's own pre-activation says: with a1 given as all zeros no gradient reaches conv1."""
    kind, Cin, mid, Cout, stride = BO.BLOCKS[1]
    case = BO.block_case(kind, Cin, mid, Cout, stride, 1, 3, 5)
    _, acts = BO.block_gradients(case, torch.float64)
    given = {k: v.float().numpy() for k, v in acts.items()}
    given["a1"] = np.zeros_like(given["a1"])
    g, acts2 = BO.block_gradients(case, torch.float64, given)
    assert not g["conv1"].any() and not g["conv2"].any() and g["conv3"].any()
    assert np.array_equal(acts2["a2"].numpy(), given["a2"].astype(np.float64))
    vals = np.array([0.0, -0.0, np.nan, 1e-45, -1.0, np.inf, 2.0], np.float32).reshape(1, 1, 1, 7)      # threshold_backward: the gradient passes unless y <= 0
    lin = torch.zeros(1, 1, 1, 7, dtype=torch.float64, requires_grad=True)
    (grad,) = torch.autograd.grad(BO._given(lin, vals, torch.float64), lin, torch.ones(1, 1, 1, 7, dtype=torch.float64))
    assert grad.reshape(-1).tolist() == [0, 0, 1, 1, 0, 1, 1]
    want = torch.ops.aten.threshold_backward(torch.ones(7), torch.from_numpy(vals.reshape(-1)), 0)
    assert grad.reshape(-1).tolist() == want.tolist()


def test_body_parameters_of_an_r50_and_the_gating_of_forward():
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        m = build_model()
        sd = dict(m.named_parameters())
        body = m.body_parameters(2)
        assert m.train_body is False and m.train_fpn is False and m.train_decoders is False
        assert len(body) == 42 and all(body[k] is sd[k] for k in body)
        assert [sum(1 for k in body if k.startswith("backbone.body.layer%d." % st)) for st in (2, 3, 4)] == [13, 19, 10]
        assert len(m.body_parameters(3)) == 29 and len(m.body_parameters(4)) == 10
        assert [id(p) for p in m.backbone.body_parameter_list(2)] == [id(p) for p in body.values()]
        with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE=1"):
            m.body_parameters(1)
        frames = torch.zeros(1, 8, 3, 32, 32)
        # train_body off: the refusals of tests/test_fpn_backward_host.py, word for word, whatever the other switches say
        with pytest.raises(NotImplementedError) as e:
            m(frames, [])
        assert str(e.value) == ("TrainingModel.forward with gradients: the decoder and encoder backward passes are not implemented; call it under "
                                "torch.no_grad() (validation), or use compute_losses for the loss gradients with respect to the head outputs")
        m.train_decoders = True
        first = next(k for k in sd if k.startswith("backbone."))
        n_other = sum(1 for k in sd if k.startswith("backbone."))
        with pytest.raises(NotImplementedError) as e:
            m(frames, [])
        assert str(e.value) == ("TrainingModel.forward with train_decoders: the encoder backward pass is not implemented, and %d parameters outside the "
                                "decoders require a gradient (%s, ...); freeze the backbone (TRAINING.FREEZE_BACKBONE)" % (n_other, first))
        m.train_fpn = True
        n_body = sum(1 for k in sd if k.startswith("backbone.body."))
        first_body = next(k for k in sd if k.startswith("backbone.body."))
        with pytest.raises(NotImplementedError) as e:
            m(frames, [])
        assert str(e.value) == ("TrainingModel.forward with train_decoders and train_fpn: behind the FPN the encoder backward pass is not implemented, and "
                                "%d parameters outside the decoders and the FPN require a gradient (%s, ...); the backbone's body must be frozen "
                                "(requires_grad_(False) on backbone.body)" % (n_body, first_body))
        # train_body alone, or without train_fpn, counts for nothing
        m.train_decoders = m.train_fpn = False
        m.train_body = True
        with pytest.raises(NotImplementedError, match="decoder and encoder backward passes are not implemented"):
            m(frames, [])
        m.train_decoders = True
        with pytest.raises(NotImplementedError, match="TrainingModel.forward with train_decoders: the encoder backward pass is not implemented"):
            m(frames, [])
        # the three switches: a trainable stem or layer1 parameter is refused, naming it
        m.train_fpn = True
        assert first_body == "backbone.body.stem.conv1.weight" and not m.body_fpn_and_decoders_only_trainable(2)
        with pytest.raises(NotImplementedError, match=r"train_decoders, train_fpn and train_body.*FREEZE_AT_STAGE >= 2.* 11 parameters.*backbone\.body\.stem\.conv1\.weight"):
            m(frames, [])
        sd[first_body].requires_grad_(False)
        with pytest.raises(NotImplementedError, match=r" 10 parameters.*backbone\.body\.layer1\.0\.downsample\.0\.weight"):
            m(frames, [])
        for k, p in sd.items():
            p.requires_grad_(not (k.startswith("backbone.body.stem.") or k.startswith("backbone.body.layer1.")))
        assert m.body_fpn_and_decoders_only_trainable(2) and not m.body_fpn_and_decoders_only_trainable(3) and m.body_freeze_at() == 2
        assert not m.fpn_and_decoders_only_trainable()
        for k in body:
            sd[k].requires_grad_(k.startswith("backbone.body.layer4."))
        assert m.body_freeze_at() == 4 and m.body_fpn_and_decoders_only_trainable(4)
        # a body the backward does not cover is refused by its key
        m.backbone.stride_in_1x1 = False
        with pytest.raises(NotImplementedError, match=r"MODEL\.RESNETS\.STRIDE_IN_1X1=False"):
            m(frames, [])
        m.backbone.stride_in_1x1 = True
        m.train_body = False                                    # ... and without the switch a trainable layer4 is what it ever was
        with pytest.raises(NotImplementedError, match="behind the FPN the encoder backward pass is not implemented.*body must be frozen"):
            m(frames, [])
    finally:
        config.load_preset("defaults")
