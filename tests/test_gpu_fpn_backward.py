"""GPU tests of the FPN backward (csrc/conv_backward.hip, hip.conv2d_wgrad / conv2d_dgrad / fpn_backward, modeling.ops.EncoderFunction,
ResNetFPN.forward_trainable_fpn, TrainingModel.train_fpn) against torch-CPU autograd (tests/fpn_backward_oracle.py).

Bounds, per case (the rule of tests/test_gpu_decoder_tail.py): the oracle runs in fp32 and in fp64 on the case's own input; the device may be
FACTOR = 4 x that spread, floored at 2^-24, away from the fp64 result, on the max norm relative to max|g|.  One-hot upstream gradients are
checked bit for bit, and the three inner products <conv(x; W, 0), g>, <W, wgrad(x, g)>, <x, dgrad(g)> against each other.  Every case prints
its spread, bound and device error before the test asserts; the per-family table is in DESIGN.md section 9i.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from stemseg_amd.modeling import encoder_backward as EB
from tests import decoder_tail_oracle as TO
from tests import fpn_backward_oracle as FO

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def haloed(hip, x):
    """x [Cin, F, H, W] numpy or tensor -> (the y/x-zero-haloed device buffer, its haloed view); the view points into the buffer: keep both."""
    x = dev(x) if isinstance(x, np.ndarray) else x
    Cin, Fr, H, W = x.shape
    buf, g = hip.alloc_padded2d(Cin, Fr, H, W)
    hip.copy_to_volume(x.contiguous(), 0, hip.padded2d_interior_view(buf, g, Cin, Fr, H, W))
    return buf, hip.padded2d_halo_view(buf, g, Cin, Fr, H, W)


def shapes():
    return [(Fr, H, W) for Fr in FO.CONV_F for H, W in FO.CONV_HW]


def wgrad9_case(hip, name, c, bad):
    r32, r64 = FO.conv_oracle(c, torch.float32), FO.conv_oracle(c, torch.float64)
    buf, view = haloed(hip, c["x"])
    dw, db = hip.conv2d_wgrad(view, dev(c["g"]), 9)
    TO.check(name, "dw", host(dw), r32["dw"], r64["dw"], bad)
    TO.check(name, "db", host(db), r32["db"], r64["db"], bad)
    dw2, db2 = hip.conv2d_wgrad(view, dev(c["g"]), 9)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "reruns differ"
    dw3, none = hip.conv2d_wgrad(view, dev(c["g"]), 9, want_db=False)
    assert none is None and torch.equal(dw3, dw)
    return buf, view


def one_hot_last(hip, c, view):
    Cout, Fr, H, W = c["g"].shape
    Cin = c["x"].shape[0]
    g = np.zeros((Cout, Fr, H, W), np.float32)
    g[Cout - 1, Fr - 1, H - 1, W - 1] = 1.0
    dw, db = hip.conv2d_wgrad(view, dev(g), 9)
    want = np.zeros((Cout, Cin, 3, 3), np.float32)
    want[Cout - 1] = FO.neighbourhood(c["x"], Fr - 1, H - 1, W - 1)
    assert np.array_equal(dw.cpu().numpy(), want) and np.array_equal(db.cpu().numpy(), g.sum((1, 2, 3)))


@pytest.mark.parametrize("Cin,Cout", FO.WGRAD9_CHANNELS)
def test_wgrad9_vs_autograd(hip, Cin, Cout):
    """F 1, 3 x maps 1x2, 3x5, 6x10, 8x16: maps narrower than a tile, ragged rows and columns, an odd pixel count against the two-pixel MFMA
    step; channels 4 -> 32 (a mostly empty channel tile), 64 -> 96 (two ci tiles, three of four waves), 36 -> 160 (a second co workgroup with
    one wave at work).  dw and db by the rule, reruns equal, want_db=False the same dw; a one-hot in the last pixel of the last frame bit for bit."""
    bad = []
    for Fr, H, W in shapes():
        c = FO.conv_case(Cin, Cout, Fr, H, W)
        buf, view = wgrad9_case(hip, "wgrad9 %d->%d F %d %dx%d" % (Cin, Cout, Fr, H, W), c, bad)
        one_hot_last(hip, c, view)
    assert not bad, bad


@pytest.mark.parametrize("Cin,Cout,Fr,H,W", FO.WGRAD9_WIDE)
def test_wgrad9_on_wide_maps(hip, Cin, Cout, Fr, H, W):
    """The 2 x 32 and 1 x 64 tiles of maps wider than 16 and 32 columns, several tiles along x with a ragged last one."""
    bad = []
    c = FO.conv_case(Cin, Cout, Fr, H, W)
    buf, view = wgrad9_case(hip, "wgrad9 %d->%d F %d %dx%d" % (Cin, Cout, Fr, H, W), c, bad)
    one_hot_last(hip, c, view)
    assert not bad, bad


def test_wgrad9_frames_do_not_leak(hip):
    """F = 2, frame 0 of x filled with +-1e30, dy zero in frame 0 and one-hot in frame 1: dw is frame 1's neighbourhood bit for bit.  A kernel
    that read frame f + kt - 1, as the 3-D form does, would bring 1e30 (times 1.0) into the sum."""
    Cin, Cout, H, W = 32, 32, 6, 10
    c = FO.conv_case(Cin, Cout, 2, H, W)
    x = c["x"].copy()
    x[:, 0] = np.where(np.arange(H * W).reshape(H, W) % 2 == 0, 1e30, -1e30).astype(np.float32)
    buf, view = haloed(hip, x)
    for y, xx in FO.corners(H, W) + [(H // 2, W // 2)]:
        g = np.zeros((Cout, 2, H, W), np.float32)
        g[5, 1, y, xx] = 1.0
        dw, db = hip.conv2d_wgrad(view, dev(g), 9)
        want = np.zeros((Cout, Cin, 3, 3), np.float32)
        want[5] = FO.neighbourhood(x, 1, y, xx)
        assert np.array_equal(dw.cpu().numpy(), want), (y, xx)
        assert np.array_equal(db.cpu().numpy(), g.sum((1, 2, 3)))


def test_wgrad9_over_several_chunks_with_a_short_last_one(hip):
    """The chunk rule (csrc/conv_backward.hip wgrad_plan): tiles of 64 pixels -- 4 rows x 16 columns on a 16-wide map -- and at least 8
    tiles to a chunk.  F = 5, 13 x 16: 20 tiles in 3 chunks, and whatever uniform chunk length gives 3 chunks of 20 tiles leaves a shorter
    last one.  The number of chunks is a function of the shape only."""
    Cin, Cout, Fr, H, W = FO.WGRAD9_CHUNKED
    n = hip.conv2d_wgrad_chunks(Cin, Cout, 9, Fr, H, W)
    tiles = Fr * -(-H // 4) * -(-W // 16)
    lengths = [L for L in range(1, tiles + 1) if -(-tiles // L) == n]
    print("chunks %d, tiles %d, chunk lengths giving that many chunks %s" % (n, tiles, lengths))
    assert n >= 3 and lengths and all(tiles - (n - 1) * L < L for L in lengths)
    assert n == hip.conv2d_wgrad_chunks(Cin, Cout, 9, Fr, H, W)
    assert hip.conv2d_wgrad_chunks(Cin, Cout, 9, Fr, 12, W) == 2 and hip.conv2d_wgrad_chunks(Cin, Cout, 9, 1, 8, 16) == 1
    bad = []
    wgrad9_case(hip, "wgrad9 chunked", FO.conv_case(Cin, Cout, Fr, H, W), bad)
    assert not bad, bad


def wgrad1_case(hip, name, c, bad, view_of=None):
    r32, r64 = FO.conv_oracle(c, torch.float32), FO.conv_oracle(c, torch.float64)
    x = dev(c["x"])
    keep, view = (x, hip.dense_volume(x)) if view_of is None else view_of(x)
    dw, db = hip.conv2d_wgrad(view, dev(c["g"]), 1)
    assert tuple(dw.shape) == c["w"].shape
    TO.check(name, "dw", host(dw), r32["dw"], r64["dw"], bad)
    TO.check(name, "db", host(db), r32["db"], r64["db"], bad)
    dw2, db2 = hip.conv2d_wgrad(view, dev(c["g"]), 1)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "reruns differ"
    dw3, none = hip.conv2d_wgrad(view, dev(c["g"]), 1, want_db=False)
    assert none is None and torch.equal(dw3, dw)
    return keep, view


def one_hot_1(hip, c, view):
    """dy = 1.0 at the last voxel of one channel: dw[co] is x there, every other row zero."""
    Cout, Fr, H, W = c["g"].shape
    g = np.zeros((Cout, Fr, H, W), np.float32)
    g[Cout - 3, Fr - 1, H - 1, W - 1] = 1.0
    dw, db = hip.conv2d_wgrad(view, dev(g), 1)
    want = np.zeros(c["w"].shape, np.float32)
    want[Cout - 3, :, 0, 0] = c["x"][:, Fr - 1, H - 1, W - 1]
    assert np.array_equal(dw.cpu().numpy(), want) and np.array_equal(db.cpu().numpy(), g.sum((1, 2, 3)))


@pytest.mark.parametrize("Cin", FO.WGRAD1_CIN)
def test_wgrad1_vs_autograd(hip, Cin):
    """Cin 4, 68 (a 32-block of input channels with 4 filled, alone and behind two full ones) x Cout 32, 96, 160 (one, three and five 32-blocks:
    half a wave's rows, a second wave row, a second workgroup) x F h w = 15 (odd), 2, 384 (twelve tiles)."""
    bad = []
    for Cout in FO.WGRAD1_COUT:
        for Fr, H, W in FO.WGRAD1_FHW:
            c = FO.conv_case(Cin, Cout, Fr, H, W, taps=1)
            keep, view = wgrad1_case(hip, "wgrad1 %d->%d F %d %dx%d" % (Cin, Cout, Fr, H, W), c, bad)
            one_hot_1(hip, c, view)
    assert not bad, bad


def test_wgrad1_widest_lateral_strided_view_and_chunks(hip):
    """The real widest lateral (2048 -> 256: sixteen workgroups along ci) on a 1 x 2 map of two frames; a strided x view (the interior of a
    zero-haloed buffer); several chunks with a shorter last one."""
    bad = []
    Cin, Cout, Fr, H, W = FO.WGRAD1_WIDEST
    c = FO.conv_case(Cin, Cout, Fr, H, W, taps=1)
    keep, view = wgrad1_case(hip, "wgrad1 %d->%d F %d %dx%d" % (Cin, Cout, Fr, H, W), c, bad)
    one_hot_1(hip, c, view)

    def interior(x):
        Cn, Fn, Hn, Wn = x.shape
        buf, g = hip.alloc_padded2d(Cn, Fn, Hn, Wn)
        v = hip.padded2d_interior_view(buf, g, Cn, Fn, Hn, Wn)
        hip.copy_to_volume(x, 0, v)
        return buf, v
    c = FO.conv_case(68, 96, 3, 6, 10, taps=1)
    keep, view = wgrad1_case(hip, "wgrad1 strided 68->96 F 3 6x10", c, bad, view_of=interior)
    one_hot_1(hip, c, view)
    xd = dev(c["x"])
    dense, _ = hip.conv2d_wgrad(hip.dense_volume(xd), dev(c["g"]), 1)
    assert torch.equal(dense, hip.conv2d_wgrad(view, dev(c["g"]), 1)[0]), "a strided view of the same values gives other bits"

    Cin, Cout, Fr, H, W = FO.WGRAD1_CHUNKED
    n = hip.conv2d_wgrad_chunks(Cin, Cout, 1, Fr, H, W)
    tiles = -(-Fr * H * W // 32)
    lengths = [L for L in range(1, tiles + 1) if -(-tiles // L) == n]
    print("chunks %d, tiles %d, chunk lengths giving that many chunks %s" % (n, tiles, lengths))
    assert n >= 3 and lengths and all(tiles - (n - 1) * L < L for L in lengths)
    assert hip.conv2d_wgrad_chunks(Cin, Cout, 1, Fr, H, W) == n and hip.conv2d_wgrad_chunks(Cin, Cout, 1, 1, 16, 32) == 1
    c = FO.conv_case(Cin, Cout, Fr, H, W, taps=1)
    keep, view = wgrad1_case(hip, "wgrad1 chunked", c, bad)
    one_hot_1(hip, c, view)
    assert not bad, bad


@pytest.mark.parametrize("precision", ["bf16x6", "f32"])
@pytest.mark.parametrize("Cin,Cout", FO.DGRAD_CHANNELS)
def test_dgrad_vs_autograd(hip, Cin, Cout, precision):
    """The 3x3 data gradient -- one 1x1x1 convolution of dy with the 9 Cin x Cout matrix of per-tap weights, then the fp64 gather -- by the
    rule, with and without an addend (the oracle's dx plus the addend, added in the oracle's dtype)."""
    bad = []
    for Fr, H, W in shapes():
        c = FO.conv_case(Cin, Cout, Fr, H, W)
        name = "dgrad %s %d->%d F %d %dx%d" % (precision, Cin, Cout, Fr, H, W)
        r32, r64 = FO.conv_oracle(c, torch.float32), FO.conv_oracle(c, torch.float64)
        dx = hip.conv2d_dgrad(dev(c["g"]), dev(c["w"]), precision)
        TO.check(name, "dx", host(dx), r32["dx"], r64["dx"], bad)
        assert torch.equal(dx, hip.conv2d_dgrad(dev(c["g"]), dev(c["w"]), precision)), "reruns differ"
        a32 = (torch.from_numpy(r32["dx"]).float() + torch.from_numpy(c["a"])).double().numpy()
        dxa = hip.conv2d_dgrad(dev(c["g"]), dev(c["w"]), precision, addend=dev(c["a"]))
        TO.check(name, "dx+a", host(dxa), a32, r64["dx"] + c["a"].astype(np.float64), bad)
        assert torch.equal(dxa, hip.conv2d_dgrad(dev(c["g"]), dev(c["w"]), precision, addend=dev(c["a"]))), "reruns differ"
    assert not bad, bad


def test_dgrad_one_hot_corners_and_refusals(hip):
    """dy = 1.0 at each of the four corners of a frame: in 'f32' dx is w[co] placed around the pixel, bit for bit, in that frame only; with an
    addend, the addend everywhere else.  'f16x3' is refused."""
    Cin, Cout, Fr, H, W = 32, 96, 3, 6, 10
    c = FO.conv_case(Cin, Cout, Fr, H, W)
    for i, (y, x) in enumerate(FO.corners(H, W)):
        co, f = (7 * i + 3) % Cout, i % Fr
        g = np.zeros((Cout, Fr, H, W), np.float32)
        g[co, f, y, x] = 1.0
        want = np.zeros((Cin, Fr, H, W), np.float32)
        hit = np.zeros((Fr, H, W), bool)
        for ky in range(3):
            for kx in range(3):
                u = (y + ky - 1, x + kx - 1)             # out[v] reads x[v + k - 1]: pixel u = v + k - 1 receives w[k]
                if 0 <= u[0] < H and 0 <= u[1] < W:
                    want[:, f, u[0], u[1]] = c["w"][co, :, ky, kx]
                    hit[f, u[0], u[1]] = True
        assert np.array_equal(hip.conv2d_dgrad(dev(g), dev(c["w"]), "f32").cpu().numpy(), want), (y, x)
        dxa = hip.conv2d_dgrad(dev(g), dev(c["w"]), "f32", addend=dev(c["a"])).cpu().numpy()
        assert np.array_equal(dxa[:, ~hit], c["a"][:, ~hit]), (y, x)
        assert np.array_equal(dxa[:, hit], (want.astype(np.float64) + c["a"])[:, hit].astype(np.float32)), (y, x)
    with pytest.raises(ValueError, match="f16x3"):
        hip.conv2d_dgrad(dev(c["g"]), dev(c["w"]), "f16x3")


@pytest.mark.parametrize("precision", ["bf16x6", "f32"])
@pytest.mark.parametrize("Cin,Cout,Fr,H,W", [(32, 32, 3, 6, 10), (64, 96, 2, 8, 16)])
def test_adjoint_identities(hip, Cin, Cout, Fr, H, W, precision):
    """<conv2d(x; W, 0), g> = <W, wgrad9(x, g)> = <x, dgrad(g)>: the same triple sum of g w x, from the device outputs in fp64, and
    <conv1x1(x; W, 0), g> = <W, wgrad1(x, g)>.  A dot product of n terms accumulated in fp32 in any order is within n 2^-24 of the sum of its
    |terms|, so each side is within (its terms per element + 2) 2^-24 S of the exact value, S the triple sum of |g w x| (the bound of
    tests/test_gpu_conv3d_backward.py): taps Cin terms for the convolution, F H W for the weight gradient, 9 Cout for the data gradient."""
    u = 2.0 ** -24
    d = lambda a: np.asarray(a, np.float64)
    t64 = lambda v: torch.from_numpy(np.abs(v)).double()
    c = FO.conv_case(Cin, Cout, Fr, H, W, seed=1)
    buf, view = haloed(hip, c["x"])
    out = torch.empty(Cout, Fr, H, W, dtype=torch.float32, device="cuda")
    hip.conv3d(view, hip.pack_conv_weight_any(dev(c["w"]).reshape(Cout, Cin, 1, 3, 3), precision), None, hip.dense_volume(out), (1, 3, 3),
               epilogue=dict(precision=precision))
    dw, _ = hip.conv2d_wgrad(view, dev(c["g"]), 9)
    dx = hip.conv2d_dgrad(dev(c["g"]), dev(c["w"]), precision)
    a, b, e = float((host(out) * d(c["g"])).sum()), float((host(dw) * d(c["w"])).sum()), float((host(dx) * d(c["x"])).sum())
    S = float((FO.frames_first(F.conv2d(FO.frames_first(t64(c["x"])), t64(c["w"]), padding=1)) * t64(c["g"])).sum())
    n_conv, n_w, n_x = 9 * Cin + 2, Fr * H * W + 2, 9 * Cout + 2
    print("adjoint 3x3 %s %d->%d F %d %dx%d: <conv, g> %.9e <W, dw> %.9e <x, dx> %.9e, S %.3e; differences / (u S): %.3f (allowed %d), %.3f (allowed %d)"
          % (precision, Cin, Cout, Fr, H, W, a, b, e, S, abs(a - b) / (u * S), n_conv + n_w, abs(b - e) / (u * S), n_w + n_x))
    assert abs(a - b) <= (n_conv + n_w) * u * S
    assert abs(b - e) <= (n_w + n_x) * u * S
    assert abs(a - e) <= (n_conv + n_x) * u * S
    c = FO.conv_case(Cin, Cout, Fr, H, W, taps=1, seed=1)
    x = dev(c["x"])
    out = torch.empty(Cout, Fr * H * W, dtype=torch.float32, device="cuda")
    hip.conv3d(hip.flat_volume(x.view(Cin, -1)), hip.pack_conv_weight_any(dev(c["w"]).reshape(Cout, Cin, 1, 1, 1), precision), None, hip.flat_volume(out), 1,
               epilogue=dict(precision=precision))
    dw, _ = hip.conv2d_wgrad(hip.dense_volume(x), dev(c["g"]), 1)
    a, b = float((host(out).reshape(c["g"].shape) * d(c["g"])).sum()), float((host(dw) * d(c["w"])).sum())
    S = float((FO.frames_first(F.conv2d(FO.frames_first(t64(c["x"])), t64(c["w"]))) * t64(c["g"])).sum())
    print("adjoint 1x1 %s %d->%d: <conv, g> %.9e <W, dw> %.9e, S %.3e; difference / (u S): %.3f (allowed %d)"
          % (precision, Cin, Cout, a, b, S, abs(a - b) / (u * S), Cin + 2 + n_w))
    assert abs(a - b) <= (Cin + 2 + n_w) * u * S


# ------------------------------------------------------------------------------------------------ the composed FPN
def run_fpn_backward(hip, case, L_vals, precision):
    Cs = [dev(v) for v in case["C"]]
    keep = [haloed(hip, v.float().contiguous().cuda()) for v in L_vals]
    lw = [dev(case["params"]["fpn_layer%d.weight" % (k + 1)]) for k in range(4)]
    out = EB.fpn_backward([hip.dense_volume(v) for v in Cs], [v for _, v in keep], [dev(g) for g in case["g"]], lw, precision)
    torch.cuda.synchronize()
    return out


def check_fpn(name, got, r32, r64, bad):
    d_layer_w, d_layer_b, d_inner_w, d_inner_b = got
    for k in range(4):
        for what, t in (("fpn_layer%d.weight", d_layer_w), ("fpn_layer%d.bias", d_layer_b), ("fpn_inner%d.weight", d_inner_w), ("fpn_inner%d.bias", d_inner_b)):
            n = what % (k + 1)
            TO.check(name, n, host(t[k]), r32[n], r64[n], bad)


@pytest.mark.parametrize("precision", ["bf16x6", "f32"])
@pytest.mark.parametrize("levels", [(0, 1, 2, 3), (0,), (3,)])
def test_fpn_backward_composed(hip, levels, precision):
    """Four levels 8x16 .. 1x2, F = 2, 32 FPN channels, lateral widths 32 / 64 / 128 / 256: all sixteen gradients by the rule and the same bits
    on a second call.  The merged laterals the device reads are the fp64 oracle's, rounded to fp32, and both oracle runs see those values.
    Upstream on one level only: on level 0, the top-down adjoint carries it to every level (all inner gradients non-zero, the layer gradients
    of levels 1-3 exactly zero); on level 3, nothing reaches the finer levels (their sixteen gradients exactly zero)."""
    case = FO.fpn_case(levels=levels)
    L64, _ = FO.fpn_forward(case["C"], case["params"], torch.float64)
    L_vals = [v.float() for v in L64]
    r32, _, _ = FO.fpn_gradients(case["C"], case["params"], case["g"], torch.float32, L_vals)
    r64, _, _ = FO.fpn_gradients(case["C"], case["params"], case["g"], torch.float64, L_vals)
    got = run_fpn_backward(hip, case, L_vals, precision)
    bad = []
    check_fpn("fpn %s levels %s" % (precision, levels), got, r32, r64, bad)
    again = run_fpn_backward(hip, case, L_vals, precision)
    assert all(torch.equal(a, b) for ga, gb in zip(got, again) for a, b in zip(ga, gb)), "reruns differ"
    for k in range(4):
        reached = any(l <= k for l in levels)          # an upstream at level l reaches the levels at or above it (coarser)
        for t in got:
            assert bool(t[k].abs().max() > 0) == (reached and (k in levels or t is got[2] or t is got[3])), (k, levels)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the FPN into a decoder
class _OracleFpn(torch.autograd.Function):
    """A test stand-in for the encoder pass: the forward hands out given maps P_k (the fp64 oracle's), the backward is encoder_backward.fpn_backward on the
    given stage outputs and laterals -- what modeling.ops.EncoderFunction does with the workspace of a real pass."""

    @staticmethod
    def forward(ctx, hip, c_views, l_views, layer_w, maps, *params):
        ctx.args = (hip, c_views, l_views, layer_w)
        return tuple(m.clone() for m in maps)

    @staticmethod
    def backward(ctx, *d):
        hip, c_views, l_views, layer_w = ctx.args
        d_layer_w, d_layer_b, d_inner_w, d_inner_b = EB.fpn_backward(c_views, l_views, [g.contiguous() for g in d], layer_w, "bf16x6")
        return (None,) * 5 + tuple(d_inner_w) + tuple(d_inner_b) + tuple(d_layer_w) + tuple(d_layer_b)


def test_fpn_into_a_decoder(hip):
    """The small embedding decoder of tests/test_gpu_decoder_training.py (in = inter = 32, T = 4 = the FPN's frame batch) fed by the composed
    FPN through ``forward_trainable`` with attached maps: the first stage of every branch now computes its data gradient, and the sixteen FPN
    gradients meet the rule against the fp64 chain FPN -> decoder.  The decoder's own gradients are the bits of a run on detached maps."""
    from tests import conv3d_backward_oracle as CO
    T = 4
    m = CO.init_decoder("embedding", T).cuda()
    m.precision = "bf16x6"
    seed, case, L, P, margin = FO.select_fpn_seed(m, T)
    print("fpn into decoder: seed %d, min |pre-ReLU| %.2e" % (seed, margin))
    c = m._packed()
    acts = m._train_acts()
    act = list(c["act"]) if acts is None else list(acts)
    H4, W4 = FO.FPN_MAPS[0]
    grids = tuple(None if v is None else v.cpu() for v in m._grid(c, T, H4, W4, torch.device("cuda", torch.cuda.current_device())))
    up = torch.randn((len(act), T, H4, W4), generator=torch.Generator().manual_seed(7))
    g32, g64 = (FO.fpn_decoder_gradients(m, T, case, L, P, up, act, list(c["axes"]), grids, dt) for dt in (torch.float32, torch.float64))
    Cs = [dev(v) for v in case["C"]]
    keep = [haloed(hip, v.cuda().contiguous()) for v in L]
    names = [k % (i + 1) for k in ("fpn_inner%d.weight", "fpn_inner%d.bias", "fpn_layer%d.weight", "fpn_layer%d.bias") for i in range(4)]
    params = [dev(case["params"][n]).requires_grad_(True) for n in names]
    maps = _OracleFpn.apply(hip, [hip.dense_volume(v) for v in Cs], [v for _, v in keep], [p.detach() for p in params[8:12]], [v.cuda() for v in P], *params)
    assert all(v.requires_grad for v in maps)
    out = m.forward_trainable(list(maps[::-1]), acts)
    out.backward(up.cuda())
    bad = []
    for n, p in zip(names, params):
        TO.check("fpn into decoder", n, host(p.grad), g32[n], g64[n], bad)
    attached = {n: p.grad.clone() for n, p in m.named_parameters()}
    assert set("decoder." + n for n in attached) == {k for k in g64 if k.startswith("decoder.")}
    for p in m.parameters():
        p.grad = None
    out2 = m.forward_trainable([v.detach() for v in maps[::-1]], acts)
    out2.backward(up.cuda())
    assert torch.equal(out2, out)
    assert all(torch.equal(p.grad, attached[n]) for n, p in m.named_parameters()), "attaching the maps changed the decoder's own gradients"
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model(hip):
    """kittimots preset, R-50, synthetic weights; the body frozen, the FPN and the decoders trainable, both switches on."""
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    from tests import synth
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        m = build_model()
        sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], 11)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()})
        m = m.cuda().eval()
        for k, p in m.named_parameters():
            p.requires_grad_(not k.startswith("backbone.body."))
        m.train_decoders = m.train_fpn = True
        m.image_mean = torch.tensor(config.cfg.INPUT.IMAGE_MEAN)
        m.initial_state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        yield m
    finally:
        config.load_preset("defaults")


def _inputs(m, N, T, H, W):
    from tests import semseg_loss_oracle as SO
    from tests import synth
    frames = torch.stack([torch.from_numpy(synth.synth_frames(T, H, W, seed=3 + n).astype(np.float32)).permute(0, 3, 1, 2) - m.image_mean[None, :, None, None]
                          for n in range(N)]).cuda()
    samples = [SO.make_sample(np.random.default_rng(5 + n), 1, T, H, W, (1, 2, 2))[1:] for n in range(N)]
    raw = lambda: [{"masks": torch.from_numpy(a).cuda(), "ignore_masks": torch.from_numpy(b).cuda(), "category_ids": torch.from_numpy(c).cuda()} for a, b, c in samples]
    return frames, raw


def _set_precision(m, precision):
    """... and the weights the fixture loaded: one test's optimiser step is not another test's input, in whatever order or selection they run."""
    m.load_state_dict(m.initial_state)
    for mod in (m.backbone, m.embedding_head, m.seediness_head, m.semseg_head):
        if mod is not None:
            mod.precision = precision


def _train_pass(m, frames, raw):
    """forward with the graph + backward of the summed losses; the four FPN maps (with their retained gradients) are caught on the way."""
    bb = m.backbone
    caught = []
    inner = bb.forward_trainable_fpn

    def catching(x):
        outs = inner(x)
        for o in outs:
            o.retain_grad()
        caught.append(outs)
        return outs
    for p in m.parameters():
        p.grad = None
    bb.forward_trainable_fpn = catching
    try:
        out = m(frames, raw())
    finally:
        del bb.forward_trainable_fpn
    loss = sum(out["optimization_losses"].values())
    assert loss.requires_grad and bool(torch.isfinite(loss))
    loss.backward()
    assert len(caught) == 1
    return caught[0], loss.detach()


def _workspace_maps(hip, bb, frames):
    """Copies of the stage outputs and merged laterals the last pass over ``frames`` left in its workspace, dense [C, F, h, w]."""
    x = frames.reshape((-1,) + tuple(frames.shape[-3:]))
    key = bb.workspace_key(x)
    c_views, l_views, _ = bb.fpn_workspace_views(key)
    ws = bb._ws[key].view(torch.float32)
    off = lambda v: (v.ptr - ws.data_ptr()) // 4
    Cs = [ws[off(v):off(v) + v.C * v.T * v.H * v.W].view(v.C, v.T, v.H, v.W).clone() for v in c_views]
    Ls = [ws[off(v):off(v) + v.C * v.c_stride].view(v.C, v.T, v.H, v.y_stride)[:, :, 1:v.H - 1, 1:v.W - 1].clone() for v in l_views]
    return Cs, Ls


def _check_fpn_gradients(hip, m, name, frames, maps):
    """The sixteen FPN gradients by the rule.  The oracle's upstream is the maps' own gradient and its inputs are the stage outputs and laterals
    the device's pass left in the workspace, so it sees exactly what the device's backward saw: no forward-precision term enters the bound."""
    Cs, Ls = _workspace_maps(hip, m.backbone, frames)
    ups = [host(o.grad.permute(1, 0, 2, 3)) for o in maps]
    params = {n: p.detach().cpu().numpy() for n, p in m.backbone.fpn.named_parameters()}
    Cs, Ls = [v.cpu() for v in Cs], [v.cpu() for v in Ls]
    r32, _, _ = FO.fpn_gradients(Cs, params, ups, torch.float32, Ls)
    r64, _, _ = FO.fpn_gradients(Cs, params, ups, torch.float64, Ls)
    bad = []
    for n, p in m.backbone.fpn.named_parameters():
        TO.check(name, n, host(p.grad), r32[n], r64[n], bad)
    return bad


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"])
def test_training_model_end_to_end(hip, model, precision):
    """One clip of 8 x 96 x 128.  The four maps are the bits of the no-grad ``run_backbone``; the summed losses' backward fills finite gradients
    on exactly the FPN and decoder parameters; the FPN's sixteen meet the rule; a second pass gives the same bits; one SGD step (lr 1e-3)
    changes the no-grad output while the body's packed tensors stay the same objects."""
    from stemseg_amd.utils.constants import ModelOutput
    m, bb = model, model.backbone
    _set_precision(m, precision)
    frames, raw = _inputs(m, 1, 8, 96, 128)
    with torch.no_grad():
        ref = [v.clone() for v in m.run_backbone(frames).values()]
        before = m(frames, raw())[ModelOutput.INFERENCE][ModelOutput.EMBEDDINGS].clone()
    maps, loss = _train_pass(m, frames, raw)
    assert all(a.requires_grad and torch.equal(a, b) for a, b in zip(maps, ref))
    named = dict(m.named_parameters())
    want = set(m.fpn_parameters()) | set(m.decoder_parameters())
    filled = {k for k, p in named.items() if p.grad is not None}
    assert filled == want and len(m.fpn_parameters()) == 16, sorted(filled ^ want)
    assert not any(k.startswith("backbone.body.") for k in filled)
    assert all(bool(torch.isfinite(named[k].grad).all()) for k in filled)
    assert all(bool(named[k].grad.any()) for k in m.fpn_parameters())
    bad = _check_fpn_gradients(hip, m, "end to end %s" % precision, frames, maps)
    first = {k: named[k].grad.clone() for k in filled}
    maps2, loss2 = _train_pass(m, frames, raw)
    assert torch.equal(loss, loss2) and all(torch.equal(named[k].grad, first[k]) for k in filled), "reruns differ"
    (w, keep), n_body = bb._packed[precision][1], bb._packed[precision][2]
    body_ids, n_kept = [id(t) for t in keep[:n_body]], len(keep)
    torch.optim.SGD([named[k] for k in sorted(want)], lr=1e-3).step()
    with torch.no_grad():
        after = m(frames, raw())[ModelOutput.INFERENCE][ModelOutput.EMBEDDINGS]
    assert not torch.equal(after, before)
    (w2, keep2), n_body2 = bb._packed[precision][1], bb._packed[precision][2]
    assert w2 is w and n_body2 == n_body and [id(t) for t in keep2[:n_body]] == body_ids, "the step re-packed the body"
    assert len(keep2) == n_kept and bb._packed[precision][0][1] == bb._signature_of(bb.fpn)          # ... and the FPN's packing is the stepped weights'
    assert not bad, bad


def test_two_clips_in_one_pass(hip, model):
    """N = 2: two clips of 8 x 64 x 64 are 16 frames of one encoder pass and one FPN backward; the same gradient check."""
    m = model
    _set_precision(m, "f16x3")
    frames, raw = _inputs(m, 2, 8, 64, 64)
    maps, _ = _train_pass(m, frames, raw)
    assert maps[0].shape == (16, 256, 16, 16)
    bad = _check_fpn_gradients(hip, m, "two clips", frames, maps)
    assert not bad, bad


def test_backward_refuses_a_workspace_another_pass_has_used(hip, model):
    """Forward with a graph, a no-grad forward of the same shape on the same lane, then backward: the RuntimeError names the workspace and
    the remedy.  With the training pass on a lane of its own the same sequence goes through."""
    from stemseg_amd.utils.constants import ModelOutput
    m, bb = model, model.backbone
    _set_precision(m, "f16x3")
    frames, raw = _inputs(m, 1, 8, 64, 64)
    for p in m.parameters():
        p.grad = None
    loss = sum(m(frames, raw())["optimization_losses"].values())
    with torch.no_grad():
        m.run_backbone(frames)
    with pytest.raises(RuntimeError, match=r"1 more encoder passes have run on the workspace .*lane"):
        loss.backward()
    try:
        bb.lane = 1
        loss = sum(m(frames, raw())["optimization_losses"].values())
        bb.lane = 0
        with torch.no_grad():
            m.run_backbone(frames)
        loss.backward()
    finally:
        bb.lane = 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.fpn_parameters().values())


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_the_fpn_alone_is_the_body_pass_without_its_body(hip, model, precision):
    """One EncoderFunction behind both entry points: ``forward_trainable_fpn(x)`` against ``forward_trainable_body(x, 4)`` with layer4 trainable,
    two frames of 64 x 64 (the smallest map with a 2 x 2 level at 32x), one fixed upstream per map: the four maps and the sixteen FPN gradients
    are the same bits, and the FPN-only call leaves every body parameter without a gradient."""
    m, bb = model, model.backbone
    _set_precision(m, precision)
    x = _inputs(m, 1, 2, 64, 64)[0][0]
    assert tuple(x.shape) == (2, 3, 64, 64)
    g = torch.Generator().manual_seed(17)
    ups = [torch.randn(2, 256, 64 >> (2 + k), 64 >> (2 + k), generator=g).cuda() for k in range(4)]
    layer4 = list(bb.body.layer4.parameters())

    def run(call):
        for p in bb.parameters():
            p.grad = None
        maps = call()
        assert [tuple(o.shape) for o in maps] == [tuple(u.shape) for u in ups] and all(o.requires_grad for o in maps)
        torch.autograd.backward(maps, ups)
        return [o.detach().clone() for o in maps], [p.grad.clone() for p in bb.fpn_parameter_list()]

    maps_fpn, grads_fpn = run(lambda: bb.forward_trainable_fpn(x))
    assert all(p.grad is None for p in bb.body.parameters())
    try:
        for p in layer4:
            p.requires_grad_(True)
        maps_body, grads_body = run(lambda: bb.forward_trainable_body(x, 4))
        assert all(p.grad is not None and bool(p.grad.any()) for p in layer4)
    finally:
        for p in layer4:
            p.requires_grad_(False)
            p.grad = None
    assert len(grads_fpn) == len(grads_body) == 16
    assert all(torch.equal(a, b) for a, b in zip(maps_fpn, maps_body)), "the maps differ"
    assert [i for i, (a, b) in enumerate(zip(grads_fpn, grads_body)) if not torch.equal(a, b)] == [], "FPN gradients differ"
