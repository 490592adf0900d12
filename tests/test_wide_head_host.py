"""Host tests of the wide linear heads (csrc/decoder_backward.hip behind hip.wide_level_head / hip.wide_heads_backward;
modeling.ops.HeadsFunction; SqueezeExpandTrunk.train_wide_head; TrainingModel.train_wide_head): the C-ABI, the argument checks (every one
is made before any launch), the chunk plan and its workspace, the switch, and the validity of the composed GPU case on the oracle alone.
No GPU."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from tests import conv3d_backward_oracle as CO
from tests import wide_head_cases as WC
from tests import wide_head_oracle as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stemseg_hip_wide_level_head", "stemseg_hip_wide_heads_backward_workspace_bytes", "stemseg_hip_wide_heads_backward_chunks",
         "stemseg_hip_wide_heads_backward")


def test_symbols_exported_declared_and_bound():
    from stemseg_amd import hip
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    for n in NAMES:
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in header and hip.lib().stemseg_hip_version() == 11
    assert hip.MAX_WIDE_HEAD_OUT == 64 and hip.MAX_HEAD_OUT == 10
    assert re.search(r"#define\s+STEMSEG_MAX_WIDE_HEAD_OUT\s+64\b", header)
    for f in ("wide_level_head", "wide_heads_backward", "wide_heads_backward_chunks"):
        assert callable(getattr(hip, f))


def test_calls_reject_bad_arguments_before_any_launch():
    from stemseg_amd import hip
    l = hip.lib()
    err = l.stemseg_hip_last_error
    fake = ctypes.c_void_p(256)
    wsb, chunks = l.stemseg_hip_wide_heads_backward_workspace_bytes, l.stemseg_hip_wide_heads_backward_chunks
    fwd = lambda Cin=32, V=30, n_out=42, x=fake, w=fake, out=fake: l.stemseg_hip_wide_level_head(x, Cin, V, w, n_out, None, out, None)
    need = wsb(32, 42, 30)
    assert need > 0

    def bwd(Cin=32, V=30, n_out=42, x=fake, w=fake, dz=fake, dw=fake, ws=fake, nb=need):
        return l.stemseg_hip_wide_heads_backward(x, Cin, V, w, n_out, dz, fake, dw, None, ws, nb, None)
    for kw, words in ((dict(n_out=10), (b"n_out=10",)), (dict(n_out=65), (b"n_out=65",)), (dict(Cin=6), (b"Cin", b"Cin=6")),
                      (dict(Cin=516), (b"Cin", b"Cin=516")), (dict(V=0), (b"voxel count", b"V=0")), (dict(V=1 << 40), (b"voxel count",))):
        args = (kw.get("Cin", 32), kw.get("n_out", 42), kw.get("V", 30))
        assert wsb(*args) == 0 and b"wide_heads_backward" in err() and all(w in err() for w in words), (kw, err())
        assert chunks(*args) == 0 and b"wide_heads_backward" in err(), kw
        assert fwd(**kw) == -1 and b"wide_level_head" in err() and all(w in err() for w in words), (kw, err())
        assert bwd(**kw) == -1 and b"wide_heads_backward" in err() and all(w in err() for w in words), (kw, err())
    for kw in (dict(x=None), dict(w=None), dict(out=None)):
        assert fwd(**kw) == -1 and b"wide_level_head: null pointer" in err(), kw
    for kw in (dict(x=None), dict(w=None), dict(dz=None), dict(dw=None), dict(ws=None)):
        assert bwd(**kw) == -1 and b"wide_heads_backward: null pointer" in err(), kw
    assert bwd(ws=ctypes.c_void_p(264)) == -1 and b"256-byte aligned" in err()
    assert bwd(nb=need - 1) == -3 and b"wide_heads_backward: workspace too small" in err()
    with pytest.raises(RuntimeError, match="n_out=65"):
        hip.wide_heads_backward_chunks(32, 65, 30)
    with pytest.raises(RuntimeError, match="Cin=6"):
        hip.wide_heads_backward(torch.zeros(6, 1, 1, 2), torch.zeros(42, 6), torch.zeros(42, 1, 1, 2))


def test_the_chunk_rule_is_a_function_of_the_shape_and_the_workspace_holds_its_slots():
    """At most 256 chunks of whole 32-voxel tiles; the workspace is the chunks' fp64 slots, n_out x (Cin weights + 1 bias) each."""
    from stemseg_amd import hip
    l = hip.lib()
    wsb, chunks = l.stemseg_hip_wide_heads_backward_workspace_bytes, l.stemseg_hip_wide_heads_backward_chunks
    for V in (1, 2, 30, 32, 33, 77, 512, 8192, 8193, 17751, 8 * 120 * 216, (1 << 40) - 1):
        for Cin, n_out in ((4, 11), (36, 42), (256, 42), (512, 64)):
            n = chunks(Cin, n_out, V)
            assert n == WC.expected_chunks(V) and 1 <= n <= WC.MAX_CHUNKS, (V, n)
            assert n == hip.wide_heads_backward_chunks(Cin, n_out, V)
            assert wsb(Cin, n_out, V) == n * n_out * (Cin + 1) * 8
    for dims in WC.CHUNKED_DIMS:                                  # the GPU test's chunked shapes: >= 3 chunks, a ragged last tile
        V = dims[0] * dims[1] * dims[2]
        assert chunks(256, 42, V) >= 3 and V % WC.TILE
    assert chunks(256, 42, 77) == 3 and chunks(256, 42, 17751) == 185 and -(-17751 // 32) == 555 == 184 * 3 + 3
    assert chunks(256, 42, 8 * 120 * 216) == 250                  # the YouTube-VIS head at T = 8, 120 x 216: 6480 tiles, 26 to a chunk


def _wide_trunk(classes, T=4):
    from stemseg_amd.modeling.semseg_decoder import SqueezeExpandDecoder
    return SqueezeExpandDecoder(32, classes, (32, 32, 32, 32), (4, 8, 16, 32), foreground_channel=True, PoolType=nn.AvgPool3d,
                                NormType=lambda c: nn.GroupNorm(8, c), num_frames=T)


def test_the_switch_is_off_by_default_and_the_refusals_name_the_head():
    feats = [torch.zeros(32, 4, h, w) for h, w in CO.MAP_SIZES]
    m = _wide_trunk(41)
    assert m.out_channels == 42 and m.train_wide_head is False
    for run in (m.forward_tail_trainable, m.forward_trainable):
        with pytest.raises(NotImplementedError, match=r"42 output channels \(INPUT\.NUM_CLASSES.*train_wide_head"):
            run(feats)
    big = _wide_trunk(64)
    big.train_wide_head = True
    for run in (big.forward_tail_trainable, big.forward_trainable):
        with pytest.raises(NotImplementedError, match=r"65 output channels \(INPUT\.NUM_CLASSES.*at most 64"):
            run(feats)
    m.train_wide_head = True
    m._check_tail_trainable()                                    # 42 channels with the switch on: accepted
    narrow = _wide_trunk(3)
    narrow._check_tail_trainable()                               # a narrow head does not need it


def test_heads_function_refuses_what_the_wide_kernels_do_not_serve():
    from stemseg_amd.modeling.ops import HeadsFunction
    x = torch.zeros(32, 1, 2, 4)
    with pytest.raises(NotImplementedError, match="65 output channels"):
        HeadsFunction.apply(x, torch.zeros(65, 32), None, None, None, None)
    with pytest.raises(NotImplementedError, match="wide head .42 output channels.* with an activation"):
        HeadsFunction.apply(x, torch.zeros(42, 32), None, [0] * 41 + [2], [0] * 42, None)
    with pytest.raises(NotImplementedError, match="wide head .42 output channels.* with an activation or a grid"):
        HeadsFunction.apply(x, torch.zeros(42, 32), None, [0] * 42, [0] * 41 + [1], None)
    with pytest.raises(NotImplementedError, match="with a bias"):
        HeadsFunction.apply(x, torch.zeros(42, 32), torch.zeros(42), None, None, None)


def test_training_model_switch_defaults_to_false_and_reaches_the_semseg_head():
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    try:
        config.load_preset("ytvis")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        m = build_model()
        assert m.semseg_head.out_channels == 42
        assert m.train_wide_head is False and m.semseg_head.train_wide_head is False
        assert (m.train_decoders, m.train_fpn, m.train_body) == (False, False, False)
        m.train_wide_head = True
        assert m.train_wide_head is True and m.semseg_head.train_wide_head is True
        assert (m.train_decoders, m.train_fpn, m.train_body) == (False, False, False)      # orthogonal to the other three
        assert m.embedding_head.train_wide_head is False                                   # it drives the semseg head alone
        m.train_wide_head = False
        assert m.semseg_head.train_wide_head is False
        assert "train_wide_head" not in m.state_dict() and "_train_wide_head" not in m.state_dict()
    finally:
        config.load_preset("defaults")


@pytest.mark.parametrize("T", [4, 8])
def test_the_wide_decoder_shares_the_trunk_and_the_seed_of_the_three_class_case(T):
    """The condition of the composed case of tests/test_gpu_wide_heads.py, on the oracle alone: among seeds 0..15 one keeps every pre-ReLU
    value of all seven stages 2e-5 from 0 in fp64.  The trunk is built before conv_out under the same seed, so every parameter but
    conv_out.weight, the selected seed and its margin are those of the existing 3-class case: asserted, not assumed."""
    wide, small = WO.init_wide_decoder(T), CO.init_decoder("semseg", T)
    sw, ss = wide.state_dict(), small.state_dict()
    assert set(sw) == set(ss) and sw["conv_out.weight"].shape == (42, 32, 1, 1, 1) and ss["conv_out.weight"].shape == (4, 32, 1, 1, 1)
    for k in sw:
        if k != "conv_out.weight":
            assert torch.equal(sw[k], ss[k]), k
    seed, margin, tried = WO.select_seed(T, wide)
    print("wide T %d: seed %d, min |pre-ReLU| %.2e (tried %s)" % (T, seed, margin, ["%.1e" % v for v in tried]))
    assert seed in CO.SEEDS and margin >= CO.RELU_MARGIN == 2e-5
    assert (seed, margin, tried) == CO.select_seed("semseg", T, small)
    # the oracle's gradients have the decoder's full key set, the head's 42 rows among them
    feats = CO.features(T, seed)
    H4, W4 = CO.MAP_SIZES[3]
    up = torch.randn((WO.N_OUT, T, H4, W4), generator=torch.Generator().manual_seed(7))
    g64, out = WO.decoder_gradients(wide, T, feats, up, torch.float64)
    assert set(g64) == {n for n, _ in wide.named_parameters()} and g64["conv_out.weight"].shape == (42, 32, 1, 1, 1)
    assert out.shape == (42, T, H4, W4)
