"""The temporal-halo promise of the 3x3x3 convolutions (stemseg_hip_conv3d_zero_t_halo, ConvEpilogue::zero_t_halo).

The decoders' 3x3x3 stages read zero-haloed volumes, so the workgroups of the first / last output plane multiply one whole plane of
zeros.  With the promise the split-staged kernels leave out the k-groups whose taps all fall into that plane (2 of 7 per channel chunk),
their weights and the plane's staging.  Every surviving product is formed and summed in the same order, and the promised call takes the
same launch decisions as the plain one, so the claim under test is EQUALITY: torch.equal(promised, plain) on the same zero-haloed input,
for every split-staged mode, every 3x3x3 tile the launcher can pick (tile_cfg 1 / 2 / 3: 16 / 8 / 4 rows x 32 columns; f16x3 also 6: the
20 x 24 block tile, 7: the 4 x 56 block tile), T in {1, 2, 3, 4, 8}, with and without split-K scratch, on a ragged H x W.  The API
requires Cin % 4 == 0 and a 3x3x3 chunk is 4 channels, so "Cin that is not a multiple of the chunk" cannot be fed; Cin = 20 gives five
chunks, which no split-K factor divides evenly (splits of 2 + 2 + 1 chunks).  One fp64 comparison per mode and tile pins both calls to the
truth at the tolerance of tests/test_gpu_bf16x6.py, and the GroupNorm-statistics epilogue is compared with stemseg_hip_conv3d_gn for equality."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as cc      # the shape tuples live there: tests/test_conv_plan_host.py asks which tile every launch of this file plans

pytestmark = pytest.mark.gpu

TILES = cc.THS_TILES
CIN, COUT, H, W = cc.THS_SHAPE


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _rand(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def _haloed(hip, x):
    Cn, T, Hh, Ww = x.shape
    buf, g = hip.alloc_padded(Cn, T, Hh, Ww)
    hip.copy_to_volume(dev(x), 0, hip.padded_interior_view(buf, g, Cn, T, Hh, Ww))
    return buf, hip.padded_halo_view(buf, g, Cn, T, Hh, Ww)


def _case(T, seed):
    x = _rand((CIN, T, H, W), seed)
    w = _rand((COUT, CIN, 3, 3, 3), seed + 1, 1.0 / np.sqrt(CIN * 27))
    b = _rand((COUT,), seed + 2)
    return x, w, b


def _run(hip, vin, wp, b, T, cfg, prec, promised, splitk, gn_groups=0):
    out = torch.full((COUT, T, H, W), float("nan"), device="cuda")
    scratch = torch.full((16 * COUT * T * H * W,), float("nan"), device="cuda") if splitk else None
    stats = None
    if promised:
        stats = hip.conv3d_zero_t_halo(vin, wp, b, hip.dense_volume(out), 3, cfg, scratch, precision=prec, gn_groups=gn_groups)
    elif gn_groups:
        stats = hip.conv3d_gn(vin, wp, b, hip.dense_volume(out), 3, gn_groups, tile_cfg=cfg, splitk_scratch=scratch, precision=prec)
    else:
        hip.conv3d(vin, wp, b, hip.dense_volume(out), 3, cfg, scratch, dict(precision=prec))
    torch.cuda.synchronize()
    return out, stats


@pytest.mark.parametrize("splitk", [False, True], ids=["plain", "splitk"])
@pytest.mark.parametrize("T", cc.THS_T)
@pytest.mark.parametrize("prec,cfg", TILES)
def test_promised_equals_plain(hip, prec, cfg, T, splitk):
    x, w, b = _case(T, 100 + T)
    buf, vin = _haloed(hip, x)
    wp, bd = hip.pack_conv_weight_any(dev(w), prec), dev(b)
    plain, _ = _run(hip, vin, wp, bd, T, cfg, prec, False, splitk)
    prom, _ = _run(hip, vin, wp, bd, T, cfg, prec, True, splitk)
    assert torch.isfinite(plain).all()
    n_diff = int((prom != plain).sum())
    print("[%s cfg%d T%d %s] differing elements: %d of %d" % (prec, cfg, T, "split-K" if splitk else "plain", n_diff, plain.numel()))
    assert torch.equal(prom, plain)


@pytest.mark.parametrize("prec,cfg", TILES)
def test_promised_vs_fp64(hip, prec, cfg):
    """Both calls against an fp64 convolution, at the bound of tests/test_gpu_bf16x6.py::_check: the split mode's error is at most
    3 x the exact-fp32-MFMA kernel's own error (or 4e-7 of the largest output)."""
    T = cc.THS_FP64_T
    x, w, b = _case(T, 300)
    ref = F.conv3d(torch.from_numpy(x).double()[None], torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1)[0].numpy()
    buf, vin = _haloed(hip, x)
    bd = dev(b)
    o32, _ = _run(hip, vin, hip.pack_conv_weight_any(dev(w), "f32"), bd, T, cfg if cfg <= 3 else 0, "f32", False, False)
    wp = hip.pack_conv_weight_any(dev(w), prec)
    assert torch.isfinite(o32).all(), "the fp32-MFMA yardstick leg is not finite"      # (its own fp64 bound: tests/test_gpu_conv_f32.py)
    e32 = float(np.abs(o32.cpu().numpy().astype(np.float64) - ref).max())
    scale = float(np.abs(ref).max())
    for promised in (False, True):
        o, _ = _run(hip, vin, wp, bd, T, cfg, prec, promised, False)
        e = float(np.abs(o.cpu().numpy().astype(np.float64) - ref).max())
        print("[%s cfg%d %s] max|err| vs fp64: fp32-MFMA %.3e, split %.3e (max|ref| %.3g)" % (prec, cfg, "promised" if promised else "plain", e32, e, scale))
        assert e <= max(3.0 * e32, 4e-7 * scale)


@pytest.mark.parametrize("splitk", [False, True], ids=["plain", "splitk"])
@pytest.mark.parametrize("groups", cc.THS_GN["groups"])
@pytest.mark.parametrize("prec,cfg", cc.THS_GN["tiles"])
def test_promised_groupnorm_statistics_equal(hip, prec, cfg, groups, splitk):
    """The fused GroupNorm statistics (groups of 8 and of 4 channels) under the skip: output and (mean, rstd) equal stemseg_hip_conv3d_gn's."""
    T = cc.THS_GN["T"]
    x, w, b = _case(T, 500)
    buf, vin = _haloed(hip, x)
    wp, bd = hip.pack_conv_weight_any(dev(w), prec), dev(b)
    plain, s_plain = _run(hip, vin, wp, bd, T, cfg, prec, False, splitk, gn_groups=groups)
    prom, s_prom = _run(hip, vin, wp, bd, T, cfg, prec, True, splitk, gn_groups=groups)
    assert torch.isfinite(s_plain).all()
    assert torch.equal(prom, plain)
    assert torch.equal(s_prom, s_plain)


def test_promise_needs_kt3(hip):
    x = _rand((8, 2, 5, 9), 1)
    buf = torch.zeros(8, 2, 7, 12, device="cuda")
    vin = hip.Volume(buf.data_ptr(), 2 * 7 * 12, 7 * 12, 12, 8, 2, 7, 11, buf.numel())
    out = torch.zeros(32, 2, 5, 9, device="cuda")
    wp = hip.pack_conv_weight_any(dev(_rand((32, 8, 1, 3, 3), 2)), "f16x3")
    with pytest.raises(RuntimeError, match="kt == 3"):
        hip.conv3d_zero_t_halo(vin, wp, None, hip.dense_volume(out), (1, 3, 3), 0, None, precision="f16x3")
