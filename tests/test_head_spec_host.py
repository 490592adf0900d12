"""CPU tests of the decoders' head specification: which output widths go through the fused heads kernel ("narrow") and which through
the 1x1x1 MFMA conv ("wide"), and the weight forms _head_spec hands to the library on each side.  SqueezeExpandTrunk._narrow_head is
the one rule; _head_spec, _fold, _packed, run_hip and the library's decoder plan must all agree with it.  No GPU: the wide side's
weight packing is replaced by the identity, and the library is asked only for workspace sizes (argument checks, no launch)."""
import ctypes

import pytest
import torch

C32, C16, C8, C4 = 32, 64, 32, 64          # four distinct widths, so a wrong level order or slice shows up as a wrong length


def _semseg(n_out, seed=0):
    from stemseg_amd.modeling.semseg_decoder import SqueezeExpandDecoder as Sem
    torch.manual_seed(seed)
    return Sem(32, n_out, [C32, C16, C8, C4], (4, 8, 16, 32), num_frames=8)


def _expected_tail(m, n):
    """The fold written out step by step in fp64: conv_out . conv_4 . (conv_8 | conv_16) per level."""
    wh = m.conv_out.weight.detach().reshape(n, C4).double()
    w4 = m.conv_4.weight.detach().reshape(C4, C8 + C4).double()
    w8 = m.conv_8.weight.detach().reshape(C8, C16 + C8).double()
    w16 = m.conv_16.weight.detach().reshape(C16, C32 + C16).double()
    m4, a = wh @ w4[:, C8:], wh @ w4[:, :C8]
    m8, b = a @ w8[:, C16:], a @ w8[:, :C16]
    m16, m32 = b @ w16[:, C32:], b @ w16[:, :C32]
    return m32, m16, m8, m4


@pytest.mark.parametrize("n", [1, 8, 9, 10])
def test_narrow_semseg_head_spec_in_every_fold_mode(n):
    """9 and 10 classes used to raise IndexError: _head_spec sent them to the wide branch while _fold already returned the flat
    narrow form."""
    from stemseg_amd import hip
    m = _semseg(n, seed=n)
    assert n <= hip.MAX_HEAD_OUT
    m32, m16, m8, m4 = _expected_tail(m, n)
    w4 = m.conv_4.weight.detach().reshape(C4, C8 + C4).double()
    wh = m.conv_out.weight.detach().reshape(n, C4).double()
    for lin, fold4, want in ((True, True, torch.cat([t.float().reshape(-1) for t in (m32, m16, m8, m4)])),
                             (False, True, (wh @ w4).float()),
                             (False, False, wh.float())):
        m.fold_linear_tail, m.fold_conv4 = lin, fold4
        w, b, act, axes = m._head_spec()
        assert tuple(w.shape) == tuple(want.shape), (lin, fold4, tuple(w.shape))
        assert torch.allclose(w, want, rtol=1e-6, atol=1e-7), (lin, fold4)
        assert tuple(b.shape) == (n,) and not b.any()
        assert act == [0] * n and axes == [0] * n
    m.fold_linear_tail, m.fold_conv4 = True, True
    assert m._head_spec()[0].numel() == n * (C32 + C16 + C8 + C4)
    assert m._narrow_head(n)


def test_every_width_lands_on_one_side_for_head_spec_fold_packed_and_the_library(monkeypatch):
    """n = 1..300: the predicate, the form _fold returns, the width _packed and run_hip see (len(act): the padded width on the wide
    side), and the output widths the library's decoder plan accepts all agree.  The library serves narrow heads up to
    STEMSEG_MAX_HEAD_OUT and wide heads padded to a multiple of 32 up to 256."""
    from stemseg_amd import hip
    from stemseg_amd.modeling.decoder_base import SqueezeExpandTrunk
    monkeypatch.setattr(hip, "pack_conv_weight_any", lambda w, precision="f32": w)
    l = hip.lib()
    d = hip.DecoderDesc()
    d.struct_bytes = ctypes.sizeof(hip.DecoderDesc)
    d.in_channels, d.T, d.H4, d.W4, d.gn_groups = 32, 8, 16, 24, 0
    for i, c in enumerate((C32, C16, C8, C4)):
        d.inter[i] = c
    for i, (p, s) in enumerate(zip((1, 1, 0), (1, 2, 2))):
        d.pool[i], d.t_scale[i] = p, s

    def plan_accepts(n_out):
        d.n_out = n_out
        return l.stemseg_hip_decoder_workspace_bytes(ctypes.byref(d)) > 0

    m = _semseg(1)
    narrow_seen = []
    for n in range(1, 301):
        narrow = SqueezeExpandTrunk._narrow_head(n)
        assert narrow == (n <= hip.MAX_HEAD_OUT)
        m.out_channels = n
        m.conv_out = torch.nn.Conv3d(C4, n, 1, bias=False)
        w_flat = m._fold(m.conv_out.weight.reshape(n, -1))
        assert (w_flat.dim() == 1) == narrow, n                       # _fold: the flat [M32|M16|M8|M4] vector exactly on the narrow side
        if not narrow and n > 256:
            continue                                                  # (wider than the MFMA head serves: the library refuses, below)
        w, b, act, axes = m._head_spec()
        width = len(act)
        assert m._narrow_head(width) == narrow, n                     # what _packed / run_hip decide from len(act)
        assert tuple(b.shape) == (width,) and len(axes) == width
        if narrow:
            assert width == n and tuple(w.shape) == (n * (C32 + C16 + C8 + C4),)
            narrow_seen.append(n)
        else:
            assert width == (n + 31) // 32 * 32 and tuple(w.shape) == (width, C8 + C4, 1, 1, 1)
            assert torch.equal(w[:n].reshape(n, -1), m._fold(m.conv_out.weight.reshape(n, -1))) and not w[n:].any()
        assert plan_accepts(width), (n, l.stemseg_hip_last_error())
    assert narrow_seen == list(range(1, hip.MAX_HEAD_OUT + 1))
    for n_out in range(1, 301):                                       # the library's own rule, for the record
        assert plan_accepts(n_out) == (n_out <= hip.MAX_HEAD_OUT or (n_out % 32 == 0 and n_out <= 256)), n_out


def test_embedding_head_wider_than_the_heads_kernel_is_refused():
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder as Emb
    Emb(32, [C32, C16, C8, C4], 5, True, True, "xytff", num_frames=8)          # 5 + 3 + 1 = 9 channels: served
    with pytest.raises(NotImplementedError):
        Emb(32, [C32, C16, C8, C4], 8, True, True, "xytff", num_frames=8)      # 5 + 6 + 1 = 12
