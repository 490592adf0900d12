"""Host tests of the decoder-tail backward (csrc/decoder_backward.hip behind hip.heads_backward, hip.upsample_trilinear_backward,
hip.gn_relu_pool_backward; modeling/ops.py; SqueezeExpandTrunk.forward_tail_trainable; TrainingModel.tail_parameters): the C-ABI, the
argument checks (every one is made before any GPU call), the differentiable twin of the weight fold, the gating of TrainingModel.forward,
the refusals, and the oracle-side condition of the GroupNorm cases.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import decoder_tail_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stemseg_hip_heads_backward", "stemseg_hip_heads_backward_workspace_bytes", "stemseg_hip_upsample_trilinear_backward",
         "stemseg_hip_gn_relu_pool_backward", "stemseg_hip_gn_relu_pool_backward_workspace_bytes", "stemseg_hip_level_head")


def test_symbols_exported_declared_and_bound():
    from stemseg_amd import hip
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    for n in NAMES:
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in header and hip.lib().stemseg_hip_version() == 11
    for f in ("heads_backward", "upsample_trilinear_backward", "gn_relu_pool_backward", "level_head"):
        assert callable(getattr(hip, f))


def test_calls_reject_bad_arguments_before_any_gpu_call():
    from stemseg_amd import hip
    l = hip.lib()
    err = l.stemseg_hip_last_error
    fake = ctypes.c_void_p(256)
    # heads
    hws = l.stemseg_hip_heads_backward_workspace_bytes
    ws = hws(64, 7, 4099)
    assert ws > 0 and hws(64, 7, 8198) > ws and hws(128, 7, 4099) > ws
    for args, word in (((64, 11, 70), b"n_out=11"), ((64, 0, 70), b"n_out"), ((6, 4, 70), b"Cin"), ((516, 4, 70), b"Cin"), ((64, 4, 0), b"voxel")):
        assert hws(*args) == 0 and word in err(), (args, err())
    act = (ctypes.c_int32 * 10)(*([1] * 10))
    ax = (ctypes.c_int32 * 10)(*([3] * 10))

    def heads(x=fake, Cin=64, n_out=7, a=act, g=ax, grids=fake, out=fake, d_out=fake, dx=fake, dw=fake, db=fake, w=fake, wsp=fake, nb=ws):
        return l.stemseg_hip_heads_backward(x, Cin, 1, 1, 4099, w, None, n_out, a, g, grids, grids, grids, out, d_out, dx, dw, db, wsp, nb, None)
    assert heads(n_out=11) == -1 and b"n_out=11" in err()
    for kw in (dict(x=None), dict(w=None), dict(d_out=None), dict(dw=None), dict(wsp=None), dict(out=None)):
        assert heads(**kw) == -1 and b"null pointer" in err(), kw
    assert heads(a=None) == -1 and b"go together" in err()
    assert heads(grids=None) == -1 and b"grid vectors" in err()
    assert heads(a=(ctypes.c_int32 * 10)(*([5] * 10))) == -1 and b"bad act/axis" in err()
    assert heads(nb=ws - 1) != 0 and b"workspace too small" in err()
    assert heads(wsp=ctypes.c_void_p(264)) == -1 and b"256-byte aligned" in err()
    # trilinear adjoint
    up = lambda d=fake, s=(1, 2, 2), o=fake, C=3: l.stemseg_hip_upsample_trilinear_backward(d, C, 2, 3, 5, s[0], s[1], s[2], o, None)
    for s in ((1, 3, 3), (3, 2, 2), (1, 2, 4), (1, 1, 1), (2, 8, 8), (0, 2, 2)):
        assert up(s=s) == -1 and b"unsupported" in err(), s
    assert up(d=None) == -1 and b"null pointer" in err()
    assert up(o=None) == -1 and b"null pointer" in err()
    assert up(C=0) == -1 and b"bad dims" in err()
    # GroupNorm + ReLU + pool
    gws = l.stemseg_hip_gn_relu_pool_backward_workspace_bytes
    assert gws(32, 4, 6, 10, 8) > 0 and gws(32, 4, 6, 10, 0) > 0
    assert gws(32, 4, 6, 10, 5) == 0 and b"not divisible" in err()
    assert gws(32, 0, 6, 10, 8) == 0 and b"bad dims" in err()

    def gn(x=fake, groups=8, pool=1, d_out=fake, dx=fake, dg=fake, st=fake, wsp=fake, nb=1 << 20):
        return l.stemseg_hip_gn_relu_pool_backward(x, 32, 4, 6, 10, groups, st, fake, fake, pool, d_out, dx, dg, fake, wsp, nb, None)
    assert gn(pool=2) == -1 and b"pool code 2" in err()
    assert gn(groups=5) == -1 and b"not divisible" in err()
    for kw in (dict(x=None), dict(d_out=None), dict(dx=None), dict(dg=None), dict(st=None), dict(wsp=None)):
        assert gn(**kw) == -1 and b"null pointer" in err(), kw
    assert gn(nb=8) != 0 and b"workspace too small" in err()
    assert l.stemseg_hip_level_head(None, 64, 70, fake, 7, None, fake, None) == -1


def _trunk(kind="embedding", pool=nn.AvgPool3d, num_classes=3, T=4):
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder
    from stemseg_amd.modeling.semseg_decoder import SqueezeExpandDecoder
    norm = lambda c: nn.GroupNorm(8, c)
    torch.manual_seed(3)
    if kind == "embedding":
        return SqueezingExpandDecoder(32, (32, 32, 32, 32), 4, tanh_activation=True, seediness_output=True, experimental_dims="xyff",
                                      PoolType=pool, NormType=norm, num_frames=T)
    return SqueezeExpandDecoder(32, num_classes, (32, 32, 32, 32), (4, 8, 16, 32), foreground_channel=True, PoolType=pool, NormType=norm, num_frames=T)


def test_fold_twin_equals_the_fold_bit_for_bit():
    for m in (_trunk("embedding"), _trunk("semseg")):
        w_head = torch.cat([c.weight.reshape(-1, 32) for c in m._head_convs()], 0)
        twin, fold = m._linear_tail_trainable(w_head), m._linear_tail(w_head)
        assert all(t.requires_grad and not f.requires_grad for t, f in zip(twin, fold))
        assert all(torch.equal(t.detach(), f) and t.dtype == torch.float32 for t, f in zip(twin, fold))


def test_fold_twin_gradients_equal_the_unfolded_chain_in_fp64():
    """Loss <g, out> on the folded form with the twin's matrices against the same loss on the unfolded chain (up-sample, concat,
    conv_16 / conv_8 / conv_4, head), everything in fp64 on the CPU.  The twin hands over fp32 matrices (as the kernels take them), so
    their gradient passes one rounding to fp32, 2^-24 relative; 4 x that is allowed on the max norm."""
    import torch.nn.functional as F
    m = _trunk("embedding").double()
    convs = m._head_convs()
    rng = np.random.default_rng(0)
    ys = [torch.from_numpy(rng.standard_normal(s)) for s in ((32, 2, 1, 2), (32, 2, 2, 4), (32, 2, 4, 8), (32, 4, 8, 16))]
    g = torch.from_numpy(rng.standard_normal((7, 4, 8, 16)))
    ts = m.t_scales
    up = lambda v, t: F.interpolate(v[None], scale_factor=(float(t), 2.0, 2.0), mode="trilinear", align_corners=False)[0]
    mix = lambda w, v: torch.einsum("oc,cthw->othw", w, v)
    params = [c.weight for c in convs] + [m.conv_16.weight, m.conv_8.weight, m.conv_4.weight]
    # folded
    mats = [a.double() for a in m._linear_tail_trainable(torch.cat([c.weight.reshape(-1, 32) for c in convs], 0))]
    z = mix(mats[0], ys[0])
    for lvl in range(1, 4):
        z = up(z, ts[lvl - 1]) + mix(mats[lvl], ys[lvl])
    folded = torch.autograd.grad((z * g).sum(), params)
    # unfolded
    x = ys[0]
    for lvl, conv in zip(range(1, 4), (m.conv_16, m.conv_8, m.conv_4)):
        x = mix(conv.weight.reshape(32, 64), torch.cat((up(x, ts[lvl - 1]), ys[lvl]), 0))
    z2 = torch.cat([mix(c.weight.reshape(-1, 32), x) for c in convs], 0)
    unfolded = torch.autograd.grad((z2 * g).sum(), params)
    assert TO.max_norm_err(z.detach().numpy(), z2.detach().numpy()) <= 4 * 2.0 ** -24
    for a, b, p in zip(folded, unfolded, params):
        e = TO.max_norm_err(a.numpy(), b.numpy())
        print(tuple(p.shape), "fold-twin gradient error / max|g| %.2e" % e)
        assert e <= 4 * 2.0 ** -24, (tuple(p.shape), e)


def _expected_tail_keys(m):
    from stemseg_amd.config import cfg
    trunk = ["conv_16.weight", "conv_8.weight", "conv_4.weight"]
    for blk in ("block_32x.9", "block_16x.5", "block_8x.1", "block_4x.1"):
        trunk += [blk + ".weight", blk + ".bias"]
    keys = ["embedding_head." + k for k in ["conv_embedding.weight", "conv_variance.weight", "conv_variance.bias"] + trunk]
    if cfg.MODEL.USE_SEEDINESS_HEAD:
        keys += ["seediness_head." + k for k in ["conv_out.weight"] + trunk]
    else:
        keys.append("embedding_head.conv_seediness.weight")
    if cfg.MODEL.USE_SEMSEG_HEAD:
        keys += ["semseg_head." + k for k in ["conv_out.weight"] + trunk]
    return set(keys)


@pytest.mark.parametrize("preset", ["davis", "ytvis", "kittimots"])
def test_tail_parameters_and_the_gating_predicate(preset):
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    try:
        config.load_preset(preset)
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        m = build_model()
        tail = m.tail_parameters()
        sd = dict(m.named_parameters())
        assert set(tail) == _expected_tail_keys(m)
        assert all(tail[k] is sd[k] for k in tail)
        assert not any(".0.weight" in k or k.startswith("backbone") for k in tail)
        frames = torch.zeros(1, 8, 3, 32, 32)
        assert not m.tail_only_trainable()                       # everything trainable: refused with the pinned message
        with pytest.raises(NotImplementedError, match="decoder and encoder backward passes are not implemented"):
            m(frames, [])
        for p in m.parameters():
            p.requires_grad_(False)
        assert not m.tail_only_trainable()                       # nothing trainable: the validation path
        for k in list(tail)[::3]:
            tail[k].requires_grad_(True)
        assert m.tail_only_trainable()
        for k in tail:
            tail[k].requires_grad_(True)
        assert m.tail_only_trainable()
        for other in ("embedding_head.block_4x.0.weight", next(k for k in sd if k.startswith("backbone"))):
            sd[other].requires_grad_(True)
            assert not m.tail_only_trainable(), other
            with pytest.raises(NotImplementedError, match="decoder and encoder backward passes are not implemented"):
                m(frames, [])
            sd[other].requires_grad_(False)
        config.cfg.TRAINING.LOSS_AT_FULL_RES = True
        full = build_model()
        with pytest.raises(NotImplementedError, match="LOSS_AT_FULL_RES"):
            full.forward_embeddings_and_semseg({}, 1, 8)
    finally:
        config.load_preset("defaults")


def test_max_pool_and_wide_heads_are_refused_by_name():
    from stemseg_amd.modeling.ops import GnReluPoolFunction
    feats = [torch.zeros(32, 4, 1, 2), torch.zeros(32, 4, 2, 4), torch.zeros(32, 4, 4, 8), torch.zeros(32, 4, 8, 16)]
    with pytest.raises(NotImplementedError, match="POOL_TYPE"):
        _trunk("embedding", pool=nn.MaxPool3d).forward_tail_trainable(feats)
    with pytest.raises(NotImplementedError, match="NUM_CLASSES"):
        _trunk("semseg", num_classes=40).forward_tail_trainable(feats)
    with pytest.raises(NotImplementedError, match="POOL_TYPE"):
        GnReluPoolFunction.apply(torch.zeros(8, 2, 3, 5, requires_grad=True), torch.zeros(4), torch.ones(8), torch.zeros(8), 2, 2)
    assert "conv_out.weight" in _trunk("semseg", num_classes=40).tail_parameter_names()


@pytest.mark.parametrize("C,groups", TO.GN_CG)
def test_no_groupnorm_case_has_a_pre_relu_value_near_zero(C, groups):
    """The sign of a pre-ReLU value decides a whole gradient term: every case the GPU test runs keeps |y| >= 1e-4 in fp64, and its
    upstream gradient has zeros and negatives."""
    for H, W in TO.GN_HW:
        for T in TO.GN_T:
            for pool in (0, 1):
                c = TO.gn_case(C, groups, T, H, W, pool)
                t = lambda a: torch.from_numpy(a).double()
                y, out = TO.gn_forward(t(c["x"]), t(c["gamma"]), t(c["beta"]), groups, pool)
                assert float(y.abs().min()) >= TO.RELU_MARGIN and c["min_abs_y"] >= TO.RELU_MARGIN
                assert tuple(out.shape) == c["g"].shape == (C, (T + 1) // 2 if pool else T, H, W)
                assert (c["g"] == 0).any() and (c["g"] < 0).any() and (y < 0).any() and (y > 0).any()
