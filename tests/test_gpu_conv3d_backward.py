"""GPU tests of the 3x3x3 convolution backward (csrc/conv_backward.hip, hip.conv3d_wgrad / conv3d_dgrad, modeling.ops.Conv3dFunction)
against torch-CPU autograd (tests/conv3d_backward_oracle.py).

Bounds, per case (the rule of tests/test_gpu_decoder_tail.py): the oracle runs in fp32 and in fp64 on the case's own input; the device
may be FACTOR = 4 x that spread, floored at 2^-24, away from the fp64 result, on the max norm relative to max|g|; dw, db and dx are
checked separately, the data gradient in 'bf16x6' and in 'f32'.  One-hot upstream gradients are checked bit for bit, and the three inner
products <conv(x; W, 0), g>, <W, wgrad(x, g)>, <x, dgrad(g)> -- one triple sum of g w x -- against each other.  Every case prints its
spread, bound and device error before the test asserts; the per-family table is in DESIGN.md section 9h.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv3d_backward_oracle as CO
from tests import decoder_tail_oracle as TO

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
    """x [Cin, T, H, W] numpy -> (the zero-haloed device buffer, its haloed view); the view points into the buffer: keep both."""
    Cin, T, H, W = x.shape
    buf, g = hip.alloc_padded(Cin, T, H, W)
    hip.copy_to_volume(dev(x), 0, hip.padded_interior_view(buf, g, Cin, T, H, W))
    return buf, hip.padded_halo_view(buf, g, Cin, T, H, W)


def shapes():
    return [(T, H, W) for T in CO.CONV_T for H, W in CO.CONV_HW]


@pytest.mark.parametrize("Cin,Cout", CO.WGRAD_CHANNELS)
def test_wgrad_vs_autograd(hip, Cin, Cout):
    """T 1, 2, 3, 5 x maps 1x2, 3x5, 6x10, 8x16: maps narrower than a tile, tiles with rows and columns beyond the map, an odd voxel count (the
    MFMA takes two voxels a step), Cin 4 (a 32-channel tile mostly empty) and 64 (two channel tiles), Cout 96 (three of a workgroup's four
    waves at work)."""
    bad = []
    for T, H, W in shapes():
        c = CO.conv_case(Cin, Cout, T, H, W)
        name = "wgrad %d->%d T %d %dx%d" % (Cin, Cout, T, H, W)
        r32, r64 = CO.conv_oracle(c, torch.float32), CO.conv_oracle(c, torch.float64)
        buf, view = haloed(hip, c["x"])
        dw, db = hip.conv3d_wgrad(view, dev(c["g"]))
        TO.check(name, "dw", host(dw), r32["dw"], r64["dw"], bad)
        TO.check(name, "db", host(db), r32["db"], r64["db"], bad)
        dw2, db2 = hip.conv3d_wgrad(view, dev(c["g"]))
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "reruns differ"
        dw3, none = hip.conv3d_wgrad(view, dev(c["g"]), want_db=False)
        assert none is None and torch.equal(dw3, dw)
    assert not bad, bad


def test_wgrad_over_several_chunks_with_a_short_last_one(hip):
    """The chunk rule (csrc/conv_backward.hip wgrad_plan): tiles of 64 voxels -- 4 rows x 16 columns on a 16-wide map -- and at least 8
    tiles to a chunk.  T = 5, 13 x 16: 5 x 4 x 1 = 20 tiles in 3 chunks, and whatever uniform chunk length gives 3 chunks of 20 tiles (7, 8,
    9) leaves a shorter last one.  The number of chunks is a function of the shape only."""
    Cin, Cout, T, H, W = CO.CHUNKED_SHAPE
    n = hip.conv3d_wgrad_chunks(Cin, Cout, T, H, W)
    tiles = T * -(-H // 4) * -(-W // 16)
    lengths = [L for L in range(1, tiles + 1) if -(-tiles // L) == n]
    print("chunks %d, tiles %d, chunk lengths giving that many chunks %s" % (n, tiles, lengths))
    assert n >= 3 and lengths and all(tiles - (n - 1) * L < L for L in lengths)
    assert n == hip.conv3d_wgrad_chunks(Cin, Cout, T, H, W)
    assert hip.conv3d_wgrad_chunks(Cin, Cout, T, 12, W) == 2 and hip.conv3d_wgrad_chunks(Cin, Cout, 1, 8, 16) == 1
    bad = []
    c = CO.conv_case(Cin, Cout, T, H, W)
    r32, r64 = CO.conv_oracle(c, torch.float32), CO.conv_oracle(c, torch.float64)
    buf, view = haloed(hip, c["x"])
    dw, db = hip.conv3d_wgrad(view, dev(c["g"]))
    TO.check("wgrad chunked", "dw", host(dw), r32["dw"], r64["dw"], bad)
    TO.check("wgrad chunked", "db", host(db), r32["db"], r64["db"], bad)
    assert all(torch.equal(a, b) for a, b in zip((dw, db), hip.conv3d_wgrad(view, dev(c["g"])))), "reruns differ"
    assert not bad, bad


@pytest.mark.parametrize("Cin,Cout,T,H,W", CO.WIDE_SHAPES)
def test_wgrad_on_wide_maps_and_further_channel_tiles(hip, Cin, Cout, T, H, W):
    """The paths the shapes above do not take: the 2 x 32 and 1 x 64 tiles of maps wider than 16 and 32 columns, several tiles along x with
    a ragged last one, a second tile of input channels (4 of its 32 filled) and a second workgroup of output channels (one of its four
    waves at work).  Against the oracle, and a one-hot in the last column of the last row bit for bit."""
    bad = []
    c = CO.conv_case(Cin, Cout, T, H, W)
    name = "wgrad %d->%d T %d %dx%d" % (Cin, Cout, T, H, W)
    r32, r64 = CO.conv_oracle(c, torch.float32), CO.conv_oracle(c, torch.float64)
    buf, view = haloed(hip, c["x"])
    dw, db = hip.conv3d_wgrad(view, dev(c["g"]))
    TO.check(name, "dw", host(dw), r32["dw"], r64["dw"], bad)
    TO.check(name, "db", host(db), r32["db"], r64["db"], bad)
    assert all(torch.equal(a, b) for a, b in zip((dw, db), hip.conv3d_wgrad(view, dev(c["g"])))), "reruns differ"
    g = np.zeros((Cout, T, H, W), np.float32)
    g[Cout - 1, T - 1, H - 1, W - 1] = 1.0
    dw, db = hip.conv3d_wgrad(view, dev(g))
    want = np.zeros((Cout, Cin, 3, 3, 3), np.float32)
    want[Cout - 1] = CO.neighbourhood(c["x"], T - 1, H - 1, W - 1)
    assert np.array_equal(dw.cpu().numpy(), want) and np.array_equal(db.cpu().numpy(), g.sum((1, 2, 3)))
    assert not bad, bad


@pytest.mark.parametrize("precision", ["bf16x6", "f32"])
@pytest.mark.parametrize("Cin,Cout", CO.DGRAD_CHANNELS)
def test_dgrad_vs_autograd(hip, Cin, Cout, precision):
    """The data gradient -- one 1x1x1 convolution of dy with the 27 Cin x Cout matrix of per-tap weights on the forward kernel, then the
    fp64 gather of every voxel's 27 taps -- by the rule above, on every shape of the weight gradient's test.  (Its first form, the 3x3x3
    forward kernel on flipped, transposed weights, kept all 27 Cout products in one fp32 accumulator and missed this bound by up to 2.6 x in
    both modes; torch's CPU data gradient is the GEMM-then-col2vol form, 1 - 2 ulp from fp64.)"""
    bad = []
    for T, H, W in shapes():
        c = CO.conv_case(Cin, Cout, T, H, W)
        name = "dgrad %s %d->%d T %d %dx%d" % (precision, Cin, Cout, T, H, W)
        r32, r64 = CO.conv_oracle(c, torch.float32), CO.conv_oracle(c, torch.float64)
        dx = hip.conv3d_dgrad(dev(c["g"]), dev(c["w"]), precision)
        TO.check(name, "dx", host(dx), r32["dx"], r64["dx"], bad)
        assert torch.equal(dx, hip.conv3d_dgrad(dev(c["g"]), dev(c["w"]), precision)), "reruns differ"
    assert not bad, bad


@pytest.mark.parametrize("Cin,Cout,T,H,W", [(32, 32, 3, 6, 10), (4, 32, 2, 3, 5), (32, 96, 5, 13, 16)])
def test_one_hot_upstream_is_exact(hip, Cin, Cout, T, H, W):
    """dy = 1.0 at one voxel of one channel, at the 8 corners and one interior voxel: dw[co] is the 3x3x3 neighbourhood of x there (zeros
    outside the volume), every other channel's dw is zero, db is the one-hot; in 'f32' mode dx is w[co] placed around the voxel.  Products
    with 1.0 and sums with zeros are exact on the fp32-input MFMA: bit for bit."""
    c = CO.conv_case(Cin, Cout, T, H, W)
    buf, view = haloed(hip, c["x"])
    for i, (t, y, x) in enumerate(CO.CORNERS_AND_INTERIOR(T, H, W)):
        co = (7 * i + 3) % Cout
        g = np.zeros((Cout, T, H, W), np.float32)
        g[co, t, y, x] = 1.0
        dw, db = hip.conv3d_wgrad(view, dev(g))
        want = np.zeros((Cout, Cin, 3, 3, 3), np.float32)
        want[co] = CO.neighbourhood(c["x"], t, y, x)
        assert np.array_equal(dw.cpu().numpy(), want), (t, y, x)
        assert np.array_equal(db.cpu().numpy(), g.sum((1, 2, 3))), (t, y, x)
        if Cin % 32 == 0:
            dx = hip.conv3d_dgrad(dev(g), dev(c["w"]), "f32").cpu().numpy()
            want = np.zeros((Cin, T, H, W), np.float32)
            for kt in range(3):
                for ky in range(3):
                    for kx in range(3):
                        u = (t + kt - 1, y + ky - 1, x + kx - 1)             # out[v] reads x[v + k - 1]: voxel u = v + k - 1 receives w[k]
                        if all(0 <= a < n for a, n in zip(u, (T, H, W))):
                            want[(slice(None),) + u] = c["w"][co, :, kt, ky, kx]
            assert np.array_equal(dx, want), (t, y, x)


@pytest.mark.parametrize("precision", ["bf16x6", "f32"])
@pytest.mark.parametrize("Cin,Cout,T,H,W", [(32, 32, 3, 6, 10), (64, 32, 5, 8, 16), (32, 96, 2, 3, 5)])
def test_adjoint_identities(hip, Cin, Cout, T, H, W, precision):
    """<conv(x; W, 0), g> = <W, wgrad(x, g)> = <x, dgrad(g)>: the same triple sum of g w x.  From the device outputs in fp64.  A dot
    product of n terms accumulated in fp32 in any order is within n 2^-24 of the sum of its |terms|, so each side is within (its terms
    per element + 2) 2^-24 S of the exact value, S the triple sum of |g w x| (+ 2: the final rounding, and the products the bf16x6 split
    drops, <= 2^-23 each): 27 Cin terms for the convolution, T H W for the weight gradient, 27 Cout for the data gradient."""
    c = CO.conv_case(Cin, Cout, T, H, W, seed=1)
    buf, view = haloed(hip, c["x"])
    out = torch.empty(Cout, T, H, W, dtype=torch.float32, device="cuda")
    hip.conv3d_zero_t_halo(view, hip.pack_conv_weight_any(dev(c["w"]), precision), None, hip.dense_volume(out), 3, precision=precision)
    dw, _ = hip.conv3d_wgrad(view, dev(c["g"]))
    dx = hip.conv3d_dgrad(dev(c["g"]), dev(c["w"]), precision)
    d = lambda a: np.asarray(a, np.float64)
    a = float((host(out) * d(c["g"])).sum())
    b = float((host(dw) * d(c["w"])).sum())
    e = float((host(dx) * d(c["x"])).sum())
    t64 = lambda v: torch.from_numpy(np.abs(v)).double()
    S = float((F.conv3d(t64(c["x"])[None], t64(c["w"]), padding=1)[0] * t64(c["g"])).sum())
    u = 2.0 ** -24
    n_conv, n_w, n_x = 27 * Cin + 2, T * H * W + 2, 27 * Cout + 2
    print("adjoint %s %d->%d T %d %dx%d: <conv, g> %.9e <W, dw> %.9e <x, dx> %.9e, S %.3e; differences / (u S): %.3f (allowed %d), %.3f (allowed %d)"
          % (precision, Cin, Cout, T, H, W, a, b, e, S, abs(a - b) / (u * S), n_conv + n_w, abs(b - e) / (u * S), n_w + n_x))
    assert abs(a - b) <= (n_conv + n_w) * u * S
    assert abs(b - e) <= (n_w + n_x) * u * S
    assert abs(a - e) <= (n_conv + n_x) * u * S


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6", "f32"])
def test_conv3d_function_forward_and_backward(hip, precision):
    """modeling.ops.Conv3dFunction end to end: the forward on the inference kernel in the caller's precision with the GroupNorm statistics
    riding along, the backward never in f16x3.  A convolution is linear, so its gradients do not depend on the forward's precision: dw and
    db against the oracle in every mode, dx the very bits of hip.conv3d_dgrad in the backward's mode (which test_dgrad_vs_autograd holds
    against the oracle).  Without a gradient wanted for x there is none."""
    from stemseg_amd.modeling.ops import Conv3dFunction
    Cin, Cout, T, H, W = 32, 64, 3, 6, 10
    c = CO.conv_case(Cin, Cout, T, H, W, seed=2)
    r32, r64 = CO.conv_oracle(c, torch.float32), CO.conv_oracle(c, torch.float64)
    x, w, b = dev(c["x"]).requires_grad_(True), dev(c["w"]).requires_grad_(True), dev(c["b"]).requires_grad_(True)
    packed = hip.pack_conv_weight_any(w.detach(), precision)
    D, stats = Conv3dFunction.apply(x, w, b, packed, precision, 8, 1e-5)
    assert D.requires_grad and not stats.requires_grad
    assert np.allclose(host(D), r64["out"], rtol=1e-5, atol=1e-5)          # (the forward kernels have their own tests: this is the wiring)
    assert np.allclose(host(stats), TO.gn_stats(r64["out"].astype(np.float32), 8, 1e-5).numpy(), rtol=1e-4, atol=1e-5)
    D.backward(dev(c["g"]))
    bad = []
    for what, p in (("dw", w), ("db", b)):
        TO.check("Conv3dFunction " + precision, what, host(p.grad), r32[what], r64[what], bad)
    assert torch.equal(x.grad, hip.conv3d_dgrad(dev(c["g"]), w.detach(), "f32" if precision == "f32" else "bf16x6"))
    assert np.allclose(host(x.grad), r64["dx"], rtol=1e-5, atol=1e-5)
    x2, w2 = dev(c["x"]), dev(c["w"]).requires_grad_(True)
    D2, none = Conv3dFunction.apply(x2, w2, None, packed, precision, 0, 0.0)
    assert none is None
    D2.backward(dev(c["g"]))
    assert x2.grad is None and torch.equal(w2.grad, w.grad)
    assert not bad, bad


@pytest.mark.parametrize("H,W", [(13, 16), (3, 5), (40, 64)])
def test_one_plane_wgrad_is_the_2d_wgrad(hip, H, W):
    """The 2-D 9-tap weight gradient is the 3-D kernel without its temporal taps.  With T = F = 1 the problems
    coincide: output plane 0 reads the frame at kt = 1 and the zero t-halo at kt = 0 and 2, and for 32 -> 32 channels both plans cut K alike
    (the cap of 64 chunks binds in both).  So dw3[:, :, 1] holds the very bits of the 2-D dw, the other two planes are zero, and db agrees.
    13 x 16: 4 tiles with ragged rows in one chunk; 3 x 5: narrower than a tile, an odd pixel count; 40 x 64: 40 tiles of 1 x 64 in 5 chunks."""
    Cin = Cout = 32
    n3, n2 = hip.conv3d_wgrad_chunks(Cin, Cout, 1, H, W), hip.conv2d_wgrad_chunks(Cin, Cout, 9, 1, H, W)
    print("one plane %dx%d: chunks %d (3-D), %d (2-D)" % (H, W, n3, n2))
    assert n3 == n2
    if (H, W) == (40, 64):
        assert hip.conv3d_wgrad_chunks(32, 32, 1, 40, 64) == hip.conv2d_wgrad_chunks(32, 32, 9, 1, 40, 64) == 5
    c = CO.conv_case(Cin, Cout, 1, H, W, seed=3)
    g = dev(c["g"])
    buf3, view3 = haloed(hip, c["x"])
    buf2, g2 = hip.alloc_padded2d(Cin, 1, H, W)
    hip.copy_to_volume(dev(c["x"]), 0, hip.padded2d_interior_view(buf2, g2, Cin, 1, H, W))
    dw3, db3 = hip.conv3d_wgrad(view3, g)
    dw2, db2 = hip.conv2d_wgrad(hip.padded2d_halo_view(buf2, g2, Cin, 1, H, W), g, 9)
    assert torch.equal(dw3[:, :, 1], dw2)
    assert int(torch.count_nonzero(dw3[:, :, 0])) == 0 and int(torch.count_nonzero(dw3[:, :, 2])) == 0
    assert torch.equal(db3, db2)
    assert float(dw2.abs().max()) > 0 and float(db2.abs().max()) > 0


@pytest.mark.parametrize("W", [10, 12])
def test_one_plane_col2vol_is_col2img(hip, W):
    """The same for the tap gather: with T = 1 only the nine kt = 1 taps of a voxel are in range, so col2vol of cols [27][32][1][6][W] is
    col2img of its slices 9 .. 17 with no addend, bit for bit.  W = 10 and 12: by element, and four elements of a row to a thread."""
    Cin, H = 32, 6
    cols = torch.from_numpy(np.random.default_rng(7 + W).standard_normal((27, Cin, 1, H, W)).astype(np.float32)).cuda()
    mid = cols[9:18].contiguous()
    dx3 = torch.empty(Cin, 1, H, W, dtype=torch.float32, device="cuda")
    dx2 = torch.empty_like(dx3)
    hip.check(hip.lib().stemseg_hip_conv3d_col2vol(hip.ptr(cols), Cin, 1, H, W, hip.ptr(dx3), hip.stream()))
    hip.check(hip.lib().stemseg_hip_conv2d_col2img(hip.ptr(mid), Cin, 1, H, W, None, hip.ptr(dx2), hip.stream()))
    torch.cuda.synchronize()
    assert torch.equal(dx3, dx2) and float(dx2.abs().max()) > 0
