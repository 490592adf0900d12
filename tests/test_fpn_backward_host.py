"""Host tests of the FPN backward (csrc/conv_backward.hip behind hip.conv2d_wgrad / conv2d_dgrad and encoder_backward.fpn_backward; modeling.ops.EncoderFunction;
ResNetFPN.forward_trainable_fpn; TrainingModel.train_fpn): the oracle of the GPU tests against the encoder oracle, the adjoint of its top-down
path, the C-ABI and its argument checks (every one is made before any GPU call), and the gating of TrainingModel.forward behind the two
switches.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encoder as oenc
from tests import fpn_backward_oracle as FO
from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stemseg_hip_conv2d_wgrad", "stemseg_hip_conv2d_wgrad_workspace_bytes", "stemseg_hip_conv2d_wgrad_chunks", "stemseg_hip_conv2d_col2img")


def test_oracle_fpn_equals_the_encoder_oracle(golden):
    """On the frames and weights of the encoder golden (R-50): the stage outputs from the encoder oracle's own blocks, then this oracle's FPN on
    them gives the four maps of ``oracle.encoder.resnet_fpn``."""
    g = golden("encoder")
    H, W, seed, _ = g["R50FPN__meta"].tolist()
    sd = synth.synth_state_dict(oenc.backbone_param_shapes("R-50-FPN"), seed)
    x = torch.from_numpy(synth.synth_frames(2, H, W, seed=seed).astype(np.float32)).permute(0, 3, 1, 2) - torch.tensor([102.9801, 115.9465, 122.7717])[None, :, None, None]
    want = oenc.resnet_fpn(x, sd, "R-50-FPN")
    with torch.no_grad():
        b = "backbone.body."
        y = F.max_pool2d(F.relu(oenc._frozen_bn(F.conv2d(x, oenc._t(sd[b + "stem.conv1.weight"]), stride=2, padding=3), sd, b + "stem.bn1")), 3, 2, 1)
        Cs = []
        for li, n in enumerate(oenc.STAGE_BLOCKS["R-50-FPN"], 1):
            for bi in range(n):
                y = oenc._bottleneck(y, sd, b + "layer%d.%d" % (li, bi), 2 if (bi == 0 and li > 1) else 1, bi == 0)
            Cs.append(y.permute(1, 0, 2, 3))
        params = {k[len("backbone.fpn."):]: np.asarray(v) for k, v in sd.items() if k.startswith("backbone.fpn.")}
        assert len(params) == 16
        _, Ps = FO.fpn_forward(Cs, params, torch.float32)
    for P, s in zip(Ps, (4, 8, 16, 32)):
        assert torch.equal(P.permute(1, 0, 2, 3), want[s]), s


def test_bilinear_adjoint_identity():
    """<up(a), b> == <a, up^T(b)> in fp64, on an odd and an even map."""
    gen = torch.Generator().manual_seed(3)
    for h, w in ((3, 5), (4, 8), (1, 2)):
        a = torch.randn(5, 2, h, w, generator=gen, dtype=torch.float64)
        b = torch.randn(5, 2, 2 * h, 2 * w, generator=gen, dtype=torch.float64)
        lhs, rhs = float((FO.up2(a) * b).sum()), float((a * FO.up2_adjoint(b)).sum())
        assert abs(lhs - rhs) <= 1e-12 * float((FO.up2(a.abs()) * b.abs()).sum()), (h, w, lhs, rhs)


def test_fpn_gradients_with_given_laterals_equal_plain_autograd():
    """Pinning the laterals to their own values changes nothing; and the chain written out -- wgrad of layer_k, G_k = dgrad + up^T(G_{k-1}),
    wgrad of inner_k -- is what autograd computes."""
    case = FO.fpn_case()
    g, Ls, Ps = FO.fpn_gradients(case["C"], case["params"], case["g"], torch.float64)
    g2, _, _ = FO.fpn_gradients(case["C"], case["params"], case["g"], torch.float64, Ls)
    assert all(np.abs(g[n] - g2[n]).max() <= 1e-13 * max(1.0, np.abs(g[n]).max()) for n in g)
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    G = None
    for k in range(4):
        dP, w = t(case["g"][k]), t(case["params"]["fpn_layer%d.weight" % (k + 1)])
        dx = FO.frames_first(F.conv_transpose2d(FO.frames_first(dP), w, padding=1))
        G = dx if G is None else dx + FO.up2_adjoint(G)
        dw = torch.einsum("ofhw,ifhw->oi", G, t(case["C"][k]))
        assert np.abs(dw.numpy() - g["fpn_inner%d.weight" % (k + 1)][:, :, 0, 0]).max() <= 1e-12 * np.abs(dw.numpy()).max(), k
        assert np.abs(G.sum((1, 2, 3)).numpy() - g["fpn_inner%d.bias" % (k + 1)]).max() <= 1e-12 * np.abs(G.sum((1, 2, 3)).numpy()).max(), k


def test_symbols_exported_declared_and_bound():
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward, ops
    from stemseg_amd.modeling.backbone import ResNetFPN
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    for n in NAMES:
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in header and hip.lib().stemseg_hip_version() == 11
    for f in ("conv2d_wgrad", "conv2d_wgrad_chunks", "conv2d_dgrad"):
        assert callable(getattr(hip, f))
    assert callable(encoder_backward.fpn_backward)
    assert issubclass(ops.EncoderFunction, torch.autograd.Function) and callable(ResNetFPN.forward_trainable_fpn)


def test_the_chunk_rule_is_a_function_of_the_shape():
    """9 taps: a chunk holds at least 8 tiles of 64 pixels; 1 tap: at least 16 tiles of 32 voxels; the partials stay within 256 MiB and the
    workspace is the chunks' fp64 slots, taps Cout Cin weights and Cout biases each."""
    from stemseg_amd import hip
    l = hip.lib()
    chunks, wsb = l.stemseg_hip_conv2d_wgrad_chunks, l.stemseg_hip_conv2d_wgrad_workspace_bytes
    assert chunks(32, 32, 9, 1, 1, 2) == 1 and chunks(*FO.WGRAD9_CHUNKED[:2], 9, *FO.WGRAD9_CHUNKED[2:]) == 3
    assert chunks(32, 32, 1, 1, 1, 2) == 1 and chunks(*FO.WGRAD1_CHUNKED[:2], 1, *FO.WGRAD1_CHUNKED[2:]) == 3
    for H in range(1, 200, 7):
        n, tiles = chunks(256, 256, 9, 8, H, 216), 8 * H * 4
        assert 1 <= n <= 64 and (n == 1 or (tiles - 1) // (n - 1) >= 8), (H, n)          # (every chunk but the last holds at least 8 tiles)
        assert wsb(256, 256, 9, 8, H, 216) == n * (9 * 256 * 256 + 256) * 8 <= (256 << 20)
        n, tiles = chunks(2048, 256, 1, 8, H, 216), -(-8 * H * 216 // 32)
        assert 1 <= n <= 64 and (n == 1 or (tiles - 1) // (n - 1) >= 16), (H, n)
        assert wsb(2048, 256, 1, 8, H, 216) == n * (2048 * 256 + 256) * 8 <= (256 << 20)
    assert chunks(256, 256, 9, 8, 120, 216) > 8 and chunks(256, 256, 1, 8, 120, 216) > 8          # the workload's 4x level is cut many times


def test_calls_reject_bad_arguments_before_any_gpu_call():
    from stemseg_amd import hip
    l = hip.lib()
    err = l.stemseg_hip_last_error
    fake = ctypes.c_void_p(256)
    chunks, wsb = l.stemseg_hip_conv2d_wgrad_chunks, l.stemseg_hip_conv2d_wgrad_workspace_bytes
    for args, word in (((32, 32, 3, 2, 3, 5), b"taps"), ((6, 32, 9, 2, 3, 5), b"Cin"), ((32, 48, 9, 2, 3, 5), b"Cout"), ((32, 48, 1, 2, 3, 5), b"Cout"),
                       ((0, 32, 1, 2, 3, 5), b"Cin"), ((32, 32, 9, 0, 3, 5), b"bad dims"), ((32, 32, 1, 2, 3, -1), b"bad dims"),
                       ((32, 32, 1, 1 << 12, 1 << 10, 1 << 10), b"bad dims")):
        assert wsb(*args) == 0 and word in err(), (args, err())
        assert chunks(*args) == -1, args
    Cin, Cout, Fr, H, W = 32, 64, 2, 3, 5
    pitch = 8
    ts = (H + 2) * pitch
    cs = Fr * ts

    def vol(ptr=256, C=Cin, dims=(Fr, H + 2, W + 2), strides=(cs, ts, pitch), limit=Cin * cs + 64):
        return hip.Volume(ptr, strides[0], strides[1], strides[2], C, dims[0], dims[1], dims[2], limit)

    for taps in (9, 1):
        halo = 2 if taps == 9 else 0
        Hm, Wm = H + 2 - halo, W + 2 - halo                   # the same view read as a 9-tap input (map H x W) or as a 1-tap input (map H + 2 x W + 2)
        need = wsb(Cin, Cout, taps, Fr, Hm, Wm)
        assert need == chunks(Cin, Cout, taps, Fr, Hm, Wm) * (taps * Cout * Cin + Cout) * 8

        def wgrad(x="vol", dy=fake, cout=Cout, t=taps, dw=fake, db=fake, ws=fake, nb=need):
            v = vol() if isinstance(x, str) else x
            return l.stemseg_hip_conv2d_wgrad(ctypes.byref(v) if v is not None else None, dy, cout, t, dw, db, ws, nb, None)
        for kw in (dict(x=None), dict(x=vol(ptr=None)), dict(dy=None), dict(dw=None), dict(ws=None)):
            assert wgrad(**kw) == -1 and b"null pointer" in err(), kw
        assert wgrad(t=3) == -1 and b"taps" in err()
        assert wgrad(x=vol(C=6)) == -1 and b"Cin" in err()
        assert wgrad(cout=48) == -1 and b"Cout" in err()
        assert wgrad(x=vol(strides=(cs, ts, W + 1))) == -1 and b"strides" in err()
        assert wgrad(x=vol(strides=(cs - pitch, ts, pitch))) == -1 and b"strides" in err()
        assert wgrad(x=vol(limit=Cin * cs - ts)) == -1 and b"limit" in err()
        assert wgrad(ws=ctypes.c_void_p(264)) == -1 and b"256-byte aligned" in err()
        assert wgrad(nb=need - 1) == -3 and b"workspace too small" in err()
    assert l.stemseg_hip_conv2d_wgrad(ctypes.byref(vol(dims=(Fr, 2, W + 2))), fake, Cout, 9, fake, fake, fake, 1 << 30, None) == -1 and b"haloed view" in err()
    c2i = lambda cols=fake, dims=(32, 2, 3, 5), dx=fake: l.stemseg_hip_conv2d_col2img(cols, dims[0], dims[1], dims[2], dims[3], None, dx, None)
    assert c2i(cols=None) == -1 and b"null pointer" in err()
    assert c2i(dx=None) == -1 and b"null pointer" in err()
    assert c2i(dims=(32, 0, 3, 5)) == -1 and b"bad dims" in err()
    with pytest.raises(ValueError, match="Cin"):
        hip.conv2d_wgrad_chunks(6, 32, 9, 2, 3, 5)
    with pytest.raises(ValueError, match="taps"):
        hip.conv2d_wgrad(vol(), torch.zeros(Cout, Fr, H, W), 3)
    with pytest.raises(ValueError, match="does not fit"):
        hip.conv2d_wgrad(vol(), torch.zeros(Cout, Fr, H, W + 1), 9)
    with pytest.raises(ValueError, match="does not fit"):
        hip.conv2d_wgrad(vol(), torch.zeros(Cout, Fr, H, W), 1)


def test_python_wrappers_name_the_bad_argument():
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward as EB
    dy, w = torch.zeros(32, 2, 3, 5), torch.zeros(32, 32, 3, 3)
    with pytest.raises(ValueError, match=r"conv2d_dgrad: precision 'f16x3'"):
        hip.conv2d_dgrad(dy, w, "f16x3")
    with pytest.raises(ValueError, match="precision"):
        hip.conv2d_dgrad(dy, w, "bf16x3")
    with pytest.raises(ValueError, match="Cin = 4 is no multiple of 32"):
        hip.conv2d_dgrad(dy, torch.zeros(32, 4, 3, 3))
    with pytest.raises(ValueError, match="against dy"):
        hip.conv2d_dgrad(torch.zeros(64, 2, 3, 5), w)
    with pytest.raises(ValueError, match="addend"):
        hip.conv2d_dgrad(dy, w, "f32", addend=torch.zeros(32, 2, 3, 6))
    maps = ((8, 16), (4, 8), (2, 4), (1, 2))
    d = [torch.zeros(32, 2, h, ww) for h, ww in maps]
    cv = [hip.Volume(256, 2 * h * ww, h * ww, ww, 32, 2, h, ww, 64 * h * ww) for h, ww in maps]
    lv = [hip.padded2d_halo_view(torch.zeros(1), hip.padded2d_geometry(32, 2, h, ww), 32, 2, h, ww) for h, ww in maps]
    lw = [w] * 4
    with pytest.raises(ValueError, match="fpn_backward: precision 'f16x3'"):
        EB.fpn_backward(cv, lv, d, lw, "f16x3")
    with pytest.raises(ValueError, match="C_views holds 3 levels"):
        EB.fpn_backward(cv[:3], lv, d, lw, "f32")
    with pytest.raises(ValueError, match=r"d_out\[1\].*is not half"):
        EB.fpn_backward(cv, lv, [d[0], d[0], d[2], d[3]], lw, "f32")
    with pytest.raises(ValueError, match=r"layer_weights\[2\]"):
        EB.fpn_backward(cv, lv, d, [w, w, torch.zeros(32, 32, 1, 1), w], "f32")
    with pytest.raises(ValueError, match=r"C_views\[3\]"):
        EB.fpn_backward(cv[:3] + [cv[2]], lv, d, lw, "f32")
    with pytest.raises(ValueError, match=r"L_halo_views\[0\]"):
        EB.fpn_backward(cv, [lv[1]] + lv[1:], d, lw, "f32")


def test_padded2d_geometry_is_the_encoders():
    """hip.padded2d_geometry against the encoder's plan: the distance between two merged-lateral slots is the layout's total rounded up to 64
    floats plus the 64-float guard block."""
    from stemseg_amd import hip
    from stemseg_amd.modeling.backbone import ResNetFPN
    bb = ResNetFPN("R-50-FPN")
    T, H, W = 3, 64, 96
    offs = (ctypes.c_int64 * 25)()
    assert hip.lib().stemseg_hip_encoder_plan_offsets(ctypes.byref(bb._desc(T, H, W)), offs) == 0
    for k in range(3):
        g = hip.padded2d_geometry(256, T, H >> (2 + k), W >> (2 + k))
        assert offs[16 + k] - offs[15 + k] == (g["total"] + 63) // 64 * 64 + 64, k
        assert g["cs"] == T * g["ts"] and g["ts"] == ((H >> (2 + k)) + 2) * g["pitch"] and g["pitch"] % 4 == 0 and g["pitch"] >= (W >> (2 + k)) + 2


def test_train_fpn_is_off_by_default_and_gates_forward():
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        m = build_model()
        sd = dict(m.named_parameters())
        fpn = m.fpn_parameters()
        assert m.train_fpn is False and m.train_decoders is False
        assert set(fpn) == {k for k in sd if k.startswith("backbone.fpn.")} and len(fpn) == 16 and all(fpn[k] is sd[k] for k in fpn)
        assert {k.rsplit(".", 1)[0] for k in fpn} == {"backbone.fpn.fpn_%s%d" % (kind, k) for kind in ("inner", "layer") for k in (1, 2, 3, 4)}
        assert [id(p) for p in m.backbone.fpn_parameter_list()] == [id(sd["backbone.fpn.fpn_%s%d.%s" % (kind, k, part)]) for kind in ("inner", "layer")
                                                                    for part in ("weight", "bias") for k in (1, 2, 3, 4)]
        frames = torch.zeros(1, 8, 3, 32, 32)
        old = "decoder and encoder backward passes are not implemented"
        # the switch off: the three refusals tests/test_conv3d_backward_host.py pins, word for word
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
        for k, p in sd.items():
            p.requires_grad_(not k.startswith("backbone."))
        m.train_decoders = False
        with pytest.raises(NotImplementedError, match=old):
            m(frames, [])
        # ... and train_fpn alone counts for nothing
        m.train_fpn = True
        with pytest.raises(NotImplementedError, match=old):
            m(frames, [])
        m.train_decoders = True
        for p in fpn.values():
            p.requires_grad_(True)
        assert m.fpn_and_decoders_only_trainable() and not m.decoders_only_trainable()
        m.train_fpn = False                                      # a trainable FPN parameter without the switch: refused as any backbone parameter
        with pytest.raises(NotImplementedError, match="encoder backward pass is not implemented.*" + next(iter(fpn)).replace(".", r"\.")):
            m(frames, [])
        m.train_fpn = True
        body = next(k for k in sd if k.startswith("backbone.body."))
        sd[body].requires_grad_(True)
        assert not m.fpn_and_decoders_only_trainable()
        with pytest.raises(NotImplementedError, match="encoder backward pass is not implemented.*" + body.replace(".", r"\.") + ".*body must be frozen"):
            m(frames, [])
        for p in m.parameters():
            p.requires_grad_(False)
        assert not m.fpn_and_decoders_only_trainable()           # nothing trainable: the validation path, switches or not
    finally:
        config.load_preset("defaults")
