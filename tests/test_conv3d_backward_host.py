"""Host tests of the 3x3x3 convolution backward and of decoder training (csrc/conv_backward.hip behind hip.conv3d_wgrad /
hip.conv3d_dgrad; modeling.ops.Conv3dFunction; SqueezeExpandTrunk.forward_trainable; TrainingModel.train_decoders): the C-ABI, the argument
checks (every one is made before any GPU call), the identity the data gradient rests on, the oracle-side condition of the composed GPU
test, and the gating of TrainingModel.forward behind the switch.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import conv3d_backward_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stemseg_hip_conv3d_wgrad", "stemseg_hip_conv3d_wgrad_workspace_bytes", "stemseg_hip_conv3d_wgrad_chunks",
         "stemseg_hip_conv3d_col2vol")


def test_symbols_exported_declared_and_bound():
    from stemseg_amd import hip
    from stemseg_amd.modeling import ops
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    for n in NAMES:
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in header and hip.lib().stemseg_hip_version() == 11
    for f in ("conv3d_wgrad", "conv3d_wgrad_chunks", "conv3d_dgrad"):
        assert callable(getattr(hip, f))
    assert issubclass(ops.Conv3dFunction, torch.autograd.Function)


def test_the_chunk_rule_is_a_function_of_the_shape():
    """One chunk holds at least 8 tiles of 64 voxels (1 row x 64 columns on a map wider than 32), the partials stay within 256 MiB, and the
    workspace is the chunks' fp64 slots: 27 Cout Cin weights and Cout biases each."""
    from stemseg_amd import hip
    l = hip.lib()
    chunks, wsb = l.stemseg_hip_conv3d_wgrad_chunks, l.stemseg_hip_conv3d_wgrad_workspace_bytes
    assert chunks(32, 32, 1, 1, 2) == 1 and chunks(32, 32, 5, 8, 16) == 2 and chunks(32, 32, 5, 12, 16) == 2
    assert chunks(*CO.CHUNKED_SHAPE) == 3
    for H in range(1, 200, 7):
        n, tiles = chunks(256, 128, 8, H, 216), 8 * H * 4
        assert 1 <= n <= 64 and (n == 1 or tiles // n >= 8), (H, n)
        assert wsb(256, 128, 8, H, 216) == n * (27 * 128 * 256 + 128) * 8 <= (256 << 20)
    assert chunks(256, 128, 8, 120, 216) > 8                      # the reference preset's 4x stage is cut many times


def test_calls_reject_bad_arguments_before_any_gpu_call():
    from stemseg_amd import hip
    l = hip.lib()
    err = l.stemseg_hip_last_error
    fake = ctypes.c_void_p(256)
    chunks, wsb = l.stemseg_hip_conv3d_wgrad_chunks, l.stemseg_hip_conv3d_wgrad_workspace_bytes
    for args, word in (((6, 32, 2, 3, 5), b"Cin"), ((32, 48, 2, 3, 5), b"Cout"), ((0, 32, 2, 3, 5), b"Cin"), ((32, 32, 0, 3, 5), b"bad dims"),
                       ((32, 32, 2, 3, -1), b"bad dims"), ((32, 32, 1 << 12, 1 << 10, 1 << 10), b"bad dims")):
        assert wsb(*args) == 0 and word in err(), (args, err())
        assert chunks(*args) == -1, args
    Cin, Cout, T, H, W = 32, 64, 2, 3, 5
    need = wsb(Cin, Cout, T, H, W)
    assert need == chunks(Cin, Cout, T, H, W) * (27 * Cout * Cin + Cout) * 8
    pitch = 8
    ts, cs = (H + 2) * pitch, (T + 2) * (H + 2) * pitch

    def vol(ptr=256, C=Cin, dims=(T + 2, H + 2, W + 2), strides=(cs, ts, pitch), limit=Cin * cs + 64):
        return hip.Volume(ptr, strides[0], strides[1], strides[2], C, dims[0], dims[1], dims[2], limit)

    def wgrad(x="vol", dy=fake, cout=Cout, dw=fake, db=fake, ws=fake, nb=need):
        v = vol() if isinstance(x, str) else x
        return l.stemseg_hip_conv3d_wgrad(ctypes.byref(v) if v is not None else None, dy, cout, dw, db, ws, nb, None)
    for kw in (dict(x=None), dict(x=vol(ptr=None)), dict(dy=None), dict(dw=None), dict(ws=None)):
        assert wgrad(**kw) == -1 and b"null pointer" in err(), kw
    assert wgrad(x=vol(dims=(2, H + 2, W + 2))) == -1 and b"haloed view" in err()
    assert wgrad(x=vol(dims=(T + 2, H + 2, 2))) == -1 and b"haloed view" in err()
    assert wgrad(x=vol(C=6)) == -1 and b"Cin" in err()
    assert wgrad(cout=48) == -1 and b"Cout" in err()
    assert wgrad(x=vol(strides=(cs, ts, W + 1))) == -1 and b"strides" in err()
    # (a channel ends at its last element, (T + 1) ts + (H + 1) pitch + W + 2 = cs - 1 here: the first channel stride that cuts into it)
    assert wgrad(x=vol(strides=(cs - 2, ts, pitch))) == -1 and b"strides" in err()
    assert wgrad(x=vol(strides=(cs, ts - pitch - 1, pitch))) == -1 and b"strides" in err()
    assert wgrad(x=vol(limit=Cin * cs - pitch)) == -1 and b"limit" in err()
    assert wgrad(ws=ctypes.c_void_p(264)) == -1 and b"256-byte aligned" in err()
    assert wgrad(nb=need - 1) == -3 and b"workspace too small" in err()
    c2v = lambda cols=fake, dims=(32, 2, 3, 5), dx=fake: l.stemseg_hip_conv3d_col2vol(cols, dims[0], dims[1], dims[2], dims[3], dx, None)
    assert c2v(cols=None) == -1 and b"null pointer" in err()
    assert c2v(dx=None) == -1 and b"null pointer" in err()
    assert c2v(dims=(32, 0, 3, 5)) == -1 and b"bad dims" in err()
    with pytest.raises(ValueError, match="Cin"):
        hip.conv3d_wgrad_chunks(6, 32, 2, 3, 5)
    with pytest.raises(ValueError, match="does not fit"):
        hip.conv3d_wgrad(vol(), torch.zeros(Cout, T, H, W + 1))


def test_dgrad_refuses_f16x3_and_narrow_input_channels():
    from stemseg_amd import hip
    dy, w = torch.zeros(32, 2, 3, 5), torch.zeros(32, 32, 3, 3, 3)
    with pytest.raises(ValueError, match=r"2\.5e-4 <= \|activation\| < 2\.6e5"):
        hip.conv3d_dgrad(dy, w, "f16x3")
    with pytest.raises(ValueError, match="precision"):
        hip.conv3d_dgrad(dy, w, "bf16x3")
    with pytest.raises(ValueError, match="Cin = 4 is no multiple of 32"):
        hip.conv3d_dgrad(dy, torch.zeros(32, 4, 3, 3, 3))
    with pytest.raises(ValueError, match="against dy"):
        hip.conv3d_dgrad(torch.zeros(64, 2, 3, 5), w)


@pytest.mark.parametrize("Cin,Cout,T,H,W", [(4, 32, 1, 1, 2), (32, 32, 3, 6, 10), (32, 96, 2, 3, 5)])
def test_the_data_gradient_is_the_convolution_with_flipped_transposed_weights(Cin, Cout, T, H, W):
    c = CO.conv_case(Cin, Cout, T, H, W)
    r64 = CO.conv_oracle(c, torch.float64)
    t = lambda a: torch.from_numpy(a).double()
    dx = F.conv3d(t(c["g"])[None], CO.flipped_transposed(t(c["w"])), padding=1)[0].numpy()
    assert np.abs(dx - r64["dx"]).max() <= 1e-13 * np.abs(r64["dx"]).max()
    # ... and tap by tap, as hip.conv3d_dgrad forms it: O_k = W_all[(k, ci)][co] dy (W_all[(k, ci)][co] = w[co][ci][k]), dx[u] = sum_k O_k[u - k + 1]
    w_all = t(c["w"]).permute(2, 3, 4, 1, 0).reshape(27, Cin, Cout)
    cols = torch.einsum("kic,cthw->kithw", w_all, t(c["g"]))
    pad = torch.zeros(Cin, T + 2, H + 2, W + 2, dtype=torch.float64)
    for k in range(27):
        kt, ky, kx = k // 9, (k // 3) % 3, k % 3
        pad[:, kt:kt + T, ky:ky + H, kx:kx + W] += cols[k]
    assert np.abs(pad[:, 1:T + 1, 1:H + 1, 1:W + 1].numpy() - r64["dx"]).max() <= 1e-13 * np.abs(r64["dx"]).max()
    for t0, y0, x0 in CO.CORNERS_AND_INTERIOR(T, H, W):          # the oracle of the one-hot cases is the neighbourhood of x
        g = np.zeros((Cout, T, H, W), np.float32)
        g[1, t0, y0, x0] = 1.0
        assert np.array_equal(CO.conv_oracle(dict(c, g=g), torch.float64)["dw"][1], CO.neighbourhood(c["x"], t0, y0, x0).astype(np.float64))


def test_round22_keeps_22_bits_and_passes_the_gradient():
    v = (torch.randn(4096, dtype=torch.float64) * torch.logspace(-3, 3, 4096, dtype=torch.float64)).requires_grad_(True)
    r = CO.round22(v)
    m = float(v.detach().abs().max())
    assert float((r - v).detach().abs().max()) <= 2.0 ** -22 * 2.0 ** np.ceil(np.log2(m))      # absolute, on the tensor's scale: one scale per tensor
    big = v.detach().abs() >= m / 8
    assert float(((r - v).abs() / v.abs()).detach()[big].max()) <= 2.0 ** -19
    r.sum().backward()
    assert torch.equal(v.grad, torch.ones_like(v))


@pytest.mark.parametrize("T", [4, 8])
@pytest.mark.parametrize("kind", ["embedding", "semseg"])
def test_a_seed_keeps_every_pre_relu_value_away_from_zero(kind, T):
    """The condition of tests/test_gpu_decoder_training.py, on the oracle alone: among seeds 0..15 there is one whose features keep every
    pre-ReLU value of all seven stages at least 2e-5 from 0 in fp64."""
    seed, margin, tried = CO.select_seed(kind, T)
    print("%s T %d: seed %d, min |pre-ReLU| %.2e (tried %s)" % (kind, T, seed, margin, ["%.1e" % v for v in tried]))
    assert seed in CO.SEEDS and margin >= CO.RELU_MARGIN == 2e-5


def test_trunk_refusals_keep_their_messages():
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder
    from stemseg_amd.modeling.semseg_decoder import SqueezeExpandDecoder
    norm = lambda c: nn.GroupNorm(8, c)
    feats = [torch.zeros(32, 4, h, w) for h, w in CO.MAP_SIZES]
    with pytest.raises(NotImplementedError, match="POOL_TYPE 'max': the max pool has no backward kernel"):
        SqueezingExpandDecoder(32, (32, 32, 32, 32), 4, tanh_activation=True, seediness_output=True, experimental_dims="xyff",
                               PoolType=nn.MaxPool3d, NormType=norm, num_frames=4).forward_trainable(feats)
    with pytest.raises(NotImplementedError, match="NUM_CLASSES"):
        SqueezeExpandDecoder(32, 40, (32, 32, 32, 32), (4, 8, 16, 32), foreground_channel=True, PoolType=nn.AvgPool3d, NormType=norm,
                             num_frames=4).forward_trainable(feats)


def test_train_decoders_is_off_by_default_and_gates_forward():
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        m = build_model()
        sd = dict(m.named_parameters())
        dec = m.decoder_parameters()
        assert m.train_decoders is False
        assert set(dec) == {k for k in sd if not k.startswith("backbone.")} and all(dec[k] is sd[k] for k in dec)
        assert set(m.tail_parameters()) < set(dec) and "embedding_head.block_32x.0.weight" in dec
        frames = torch.zeros(1, 8, 3, 32, 32)
        old = "decoder and encoder backward passes are not implemented"
        assert not m.decoders_only_trainable()                   # everything trainable
        with pytest.raises(NotImplementedError, match=old):
            m(frames, [])
        m.train_decoders = True
        with pytest.raises(NotImplementedError, match="encoder backward pass is not implemented"):
            m(frames, [])
        for k, p in sd.items():
            p.requires_grad_(not k.startswith("backbone."))
        assert m.decoders_only_trainable() and not m.tail_only_trainable()
        m.train_decoders = False                                 # off: a trainable decoder convolution is refused as ever
        with pytest.raises(NotImplementedError, match=old):
            m(frames, [])
        m.train_decoders = True
        first = next(k for k in sd if k.startswith("backbone."))
        sd[first].requires_grad_(True)
        assert not m.decoders_only_trainable()
        with pytest.raises(NotImplementedError, match="encoder backward pass is not implemented.*" + first.replace(".", r"\.")):
            m(frames, [])
        for p in m.parameters():
            p.requires_grad_(False)
        assert not m.decoders_only_trainable()                   # nothing trainable: the validation path, switch or not
    finally:
        config.load_preset("defaults")
