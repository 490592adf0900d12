"""GPU tests of the body backward (csrc/bottleneck_backward.hip; hip.relu_backward / subsample2 / scatter2 / scale_rows / conv1x1_dgrad /
bottleneck_backward / body_stage_forward / body_backward; modeling.ops.EncoderFunction; ResNetFPN.forward_trainable_body;
TrainingModel.train_body) against torch-CPU autograd (tests/body_backward_oracle.py, tests/fpn_backward_oracle.py).

The streaming kernels are checked bit for bit against the same fp32 operation on the CPU.  Gradients, per case (the rule of
tests/test_gpu_decoder_tail.py): the oracle runs in fp32 and in fp64 on the case's own input, taking the device's recomputed activations as
given values (so the ReLU masks and the inputs of the weight gradients are the device's); the device may be FACTOR = 4 x that spread, floored
at 2^-24, away from the fp64 result, on the max norm relative to max|g|.  Every case prints its spread, bound and device error before the test
asserts; the per-family table is in DESIGN.md section 9j.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from stemseg_amd.modeling import encoder_backward as EB
from tests import body_backward_oracle as BO
from tests import decoder_tail_oracle as TO
from tests import fpn_backward_oracle as FO

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def haloed(hip, x):
    """x [C, F, H, W] -> (the y/x-zero-haloed device buffer, its geometry)."""
    x = dev(x) if isinstance(x, np.ndarray) else x
    Cn, Fr, H, W = x.shape
    buf, g = hip.alloc_padded2d(Cn, Fr, H, W)
    hip.copy_to_volume(x.contiguous(), 0, hip.padded2d_interior_view(buf, g, Cn, Fr, H, W))
    return buf, g


SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, -1.0, np.inf, -np.inf, np.nan, 1e-38, 3.0], np.float32)


def activation(rng, shape):
    """Normal values with +0.0, -0.0, denormals, infinities and NaN spread over them."""
    y = rng.standard_normal(shape).astype(np.float32)
    flat = y.reshape(-1)
    pos = rng.permutation(flat.size)[:min(flat.size // 2, 4 * SPECIALS.size)]
    flat[pos] = SPECIALS[np.arange(pos.size) % SPECIALS.size]
    return y


# ------------------------------------------------------------------------------------------------ the streaming kernels
@pytest.mark.parametrize("W", [2, 5, 16, 130])
def test_relu_backward_is_threshold_backward(hip, W):
    """Rows of 2, 5, 16 and 130 (no vector path, none, all of it, vector rows that are no multiple of a workgroup's); y dense and as the interior
    of the haloed layout; with and without the addend; out a new tensor and g itself.  y holds +0.0, -0.0, denormals of both signs, negatives,
    +-inf and NaN.  Bit-equal to torch-CPU threshold_backward of the fp32 sum g + addend."""
    rng = np.random.default_rng(W)
    shape = (3, 2, 3, W)
    y, g, a = activation(rng, shape), rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)
    for special in SPECIALS:
        assert bool((bits(torch.from_numpy(y)) == bits(torch.tensor([special]))).any()), special
    yd = dev(y)
    buf, geo = haloed(hip, y)
    for layout, view in (("dense", hip.dense_volume(yd)), ("haloed", hip.padded2d_interior_view(buf, geo, *shape))):
        for addend in (None, a):
            total = torch.from_numpy(g) if addend is None else torch.from_numpy(g) + torch.from_numpy(addend)          # (the same fp32 add)
            want = torch.ops.aten.threshold_backward(total, torch.from_numpy(y), 0)
            ad = None if addend is None else dev(addend)
            got = hip.relu_backward(view, dev(g), ad)
            assert torch.equal(bits(got), bits(want)), (layout, addend is not None)
            gd = dev(g)
            same = hip.relu_backward(view, gd, ad, out=gd)
            assert same is gd and torch.equal(bits(gd), bits(want)), (layout, "in place")


SUB_SHAPES = ((4, 1, 2, 4), (36, 3, 6, 10), (32, 2, 16, 32))


@pytest.mark.parametrize("shape", SUB_SHAPES)
def test_subsample2_and_scatter2(hip, shape):
    """[4][1][2][4] (one output row of 2), [36][3][6][10] (odd small rows: no vector path), [32][2][16][32] (the vector paths, several workgroups):
    bit-exact against slicing; <subsample2(x), g> == <x, scatter2(g)> exactly on integer-valued data; scatter2 with an addend leaves the
    addend's bits -- -0.0, NaN -- at the odd positions and adds at the even ones."""
    rng = np.random.default_rng(sum(shape))
    Cn, Fr, H, W = shape
    x = activation(rng, shape)
    sub = hip.subsample2(dev(x))
    assert torch.equal(bits(sub), bits(torch.from_numpy(x[:, :, ::2, ::2].copy())))
    g = rng.standard_normal((Cn, Fr, H // 2, W // 2)).astype(np.float32)
    g[0, 0, 0, 0] = -0.0
    want = np.zeros(shape, np.float32)
    want[:, :, ::2, ::2] = g
    assert torch.equal(bits(hip.scatter2(dev(g))), bits(torch.from_numpy(want)))
    xi, gi = rng.integers(-8, 9, shape).astype(np.float32), rng.integers(-8, 9, g.shape).astype(np.float32)
    lhs = float((hip.subsample2(dev(xi)).double() * dev(gi).double()).sum())
    rhs = float((dev(xi).double() * hip.scatter2(dev(gi)).double()).sum())
    assert lhs == rhs == float((xi[:, :, ::2, ::2].astype(np.float64) * gi).sum())
    a = activation(rng, shape)
    wanted = torch.from_numpy(a.copy())
    wanted[:, :, ::2, ::2] = torch.from_numpy(a[:, :, ::2, ::2].copy()) + torch.from_numpy(g)
    got = hip.scatter2(dev(g), dev(a))
    odd = np.ones(shape, bool)
    odd[:, :, ::2, ::2] = False
    assert torch.equal(bits(got)[torch.from_numpy(odd)], bits(torch.from_numpy(a))[torch.from_numpy(odd)])
    even = ~torch.from_numpy(odd)
    nan = torch.isnan(wanted)
    assert torch.equal(bits(got)[even & ~nan], bits(wanted)[even & ~nan]) and bool(torch.isnan(got.cpu())[nan].all())


@pytest.mark.parametrize("Cin,Cout", FO.DGRAD_CHANNELS)
def test_col2img_relu_is_relu_backward_of_col2img(hip, Cin, Cout):
    """On the dgrad shapes of the FPN tests (F 1, 3 x maps 1x2, 3x5, 6x10, 8x16): bit for bit relu_backward(mask, col2img(cols, addend)), with
    and without the addend, the mask read from the interior of a haloed buffer; and conv2d_dgrad(mask=) is conv2d_dgrad + relu_backward."""
    for Fr in FO.CONV_F:
        for H, W in FO.CONV_HW:
            rng = np.random.default_rng(Cin + 10 * Fr + H + W)
            cols = dev(rng.standard_normal((9 * Cin, Fr, H, W)).astype(np.float32))
            a = dev(rng.standard_normal((Cin, Fr, H, W)).astype(np.float32))
            buf, geo = haloed(hip, activation(rng, (Cin, Fr, H, W)))
            mask = hip.padded2d_interior_view(buf, geo, Cin, Fr, H, W)
            for addend in (None, a):
                plain = torch.empty(Cin, Fr, H, W, device="cuda")
                hip.check(hip.lib().stemseg_hip_conv2d_col2img(hip.ptr(cols), Cin, Fr, H, W, hip.ptr(addend), hip.ptr(plain), hip.stream()))
                fused = torch.full((Cin, Fr, H, W), float("nan"), device="cuda")
                hip.check(hip.lib().stemseg_hip_conv2d_col2img_relu(hip.ptr(cols), Cin, Fr, H, W, hip.ptr(addend), C.byref(mask), hip.ptr(fused), hip.stream()))
                assert torch.equal(bits(fused), bits(hip.relu_backward(mask, plain))), (Fr, H, W, addend is not None)
            c = FO.conv_case(Cin, Cout, Fr, H, W)
            dx = hip.conv2d_dgrad(dev(c["g"]), dev(c["w"]), "bf16x6", addend=dev(c["a"]))
            dxm = hip.conv2d_dgrad(dev(c["g"]), dev(c["w"]), "bf16x6", addend=dev(c["a"]), mask=mask)
            assert torch.equal(bits(dxm), bits(hip.relu_backward(mask, dx))), (Fr, H, W)


@pytest.mark.parametrize("rows,n", [(32, 288), (5, 7), (96, 64), (3, 1)])
def test_scale_rows(hip, rows, n):
    """Rows of 288 and 64 (vector path) and of 7 and 1 (by element): the same fp32 multiply as on the CPU, bit for bit."""
    rng = np.random.default_rng(rows + n)
    dw, s = rng.standard_normal((rows, n)).astype(np.float32), rng.uniform(0.5, 1.5, rows).astype(np.float32)
    d = dev(dw)
    assert hip.scale_rows(d, dev(s)) is d
    assert torch.equal(bits(d), bits(torch.from_numpy(dw) * torch.from_numpy(s)[:, None]))


@pytest.mark.parametrize("n,N", [(1, 5), (3, 7), (8, 4096 + 4), (2, 64)])
def test_sum_partials(hip, n, N):
    """The fp64 sum of n partials and the addend in order, rounded once: bit for bit the same sum on the CPU; rows by element (5, 7) and by
    four (4100, 64), with and without the addend."""
    rng = np.random.default_rng(n + N)
    parts, a = (rng.standard_normal((n, N)) * 10.0 ** rng.integers(-3, 4, (n, N))).astype(np.float32), rng.standard_normal(N).astype(np.float32)
    for addend in (None, a):
        acc = np.zeros(N, np.float64)
        for j in range(n):
            acc = acc + parts[j].astype(np.float64)
        if addend is not None:
            acc = acc + addend.astype(np.float64)
        out, pd, ad = torch.full((N,), float("nan"), device="cuda"), dev(parts), None if addend is None else dev(addend)
        hip.check(hip.lib().stemseg_hip_sum_partials(hip.ptr(pd), n, N, hip.ptr(ad), hip.ptr(out), hip.stream()))
        assert torch.equal(bits(out), bits(torch.from_numpy(acc.astype(np.float32)))), (n, N, addend is not None)


@pytest.mark.parametrize("Cout", [96, 256, 288, 544])
def test_conv1x1_dgrad_vs_autograd(hip, Cout):
    """w^T dy with and without the addend, 64 input channels on 3 x (3 x 5) voxels, by the rule, in both precisions: 96 and 256 output channels
    in one convolution, 288 and 544 in chunks of hip.DGRAD_K_CHUNK = 256 (256 + 32; 256 + 256 + 32) added in fp64."""
    assert hip.DGRAD_K_CHUNK == 256
    bad = []
    c = FO.conv_case(64, Cout, 3, 3, 5, taps=1)
    r32, r64 = FO.conv_oracle(c, torch.float32), FO.conv_oracle(c, torch.float64)
    for precision in ("bf16x6", "f32"):
        dx = hip.conv1x1_dgrad(dev(c["g"]), dev(c["w"]), precision)
        TO.check("dgrad1 %s" % precision, "dx", host(dx), r32["dx"], r64["dx"], bad)
        dxa = hip.conv1x1_dgrad(dev(c["g"]), dev(c["w"]), precision, addend=dev(c["a"]))
        TO.check("dgrad1 %s" % precision, "dx+a", host(dxa), r32["dx"] + c["a"].astype(np.float32).astype(np.float64), r64["dx"] + c["a"], bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ one block
def device_block(hip, p, stride, precision):
    """The dict ``encoder_backward.body_stage_forward`` / ``encoder_backward.body_backward`` take for one block with the oracle's parameters p."""
    d = dict(stride=stride)
    for n, key, wkey, skey in (("conv1", "conv1", "w1", "s1"), ("conv2", "conv2", "w2", "s2"), ("conv3", "conv3", "w3", "s3"), ("down", "down", "wd", "sd")):
        if n in p:
            w = dev(BO.folded(p, n))
            d[key] = (hip.pack_conv_weight_any(w.reshape(w.shape[0], w.shape[1], 1, w.shape[2], w.shape[3]), precision), dev(p[n + ".b"]))
            d[wkey], d[skey] = w, dev(p[n + ".s"])
    return d


def block_weights(blk):
    return dict(conv1=blk["w1"], conv2=blk["w2"], conv3=blk["w3"], down=blk.get("wd"), s1=blk["s1"], s2=blk["s2"], s3=blk["s3"], sd=blk.get("sd"))


def given_of(s):
    buf, g = s["a1"]
    mid, Fr, h, w = s["a2"].shape
    a1 = buf[:mid * g["cs"]].view(mid, Fr, h + 2, g["pitch"])[:, :, 1:h + 1, 1:w + 1]
    return dict(a1=a1.cpu().numpy(), a2=s["a2"].cpu().numpy(), out=s["out"].cpu().numpy())


@pytest.mark.parametrize("precision", ["bf16x6", "f32"])
@pytest.mark.parametrize("kind,Cin,mid,Cout,stride", BO.BLOCKS)
def test_one_block_vs_autograd(hip, kind, Cin, mid, Cout, stride, precision):
    """A stride-1 projection block 64 -> 32 -> 128, an identity block 128 -> 32 -> 128 and a stride-2 projection block 128 -> 64 -> 256, F 1
    and 3, maps 1x2, 3x5 and 8x16 after the stride: every dW and g_x by the rule, the oracle on the device's recomputed activations; with
    want_dx=False no g_x and the same dW bits; a second call gives the same bits."""
    bad = []
    for Fr in BO.BLOCK_F:
        for h, w in BO.BLOCK_HW:
            name = "%s %s F %d %dx%d" % (kind, precision, Fr, h, w)
            case = BO.block_case(kind, Cin, mid, Cout, stride, Fr, h, w)
            blk = device_block(hip, case["params"], stride, precision)
            s = EB.body_stage_forward(dev(case["x"]), [blk], precision)[0]
            given = given_of(s)
            r32, _ = BO.block_gradients(case, torch.float32, given)
            r64, _ = BO.block_gradients(case, torch.float64, given)
            got = EB.bottleneck_backward(hip.dense_volume(s["xs"]), s, dev(case["g"]), block_weights(blk), precision)
            for n in r64:
                TO.check(name, n, host(got[n]), r32[n], r64[n], bad)
            assert (got["down"] is None) == (kind == "identity")
            nodx = EB.bottleneck_backward(hip.dense_volume(s["xs"]), s, dev(case["g"]), block_weights(blk), precision, want_dx=False)
            again = EB.bottleneck_backward(hip.dense_volume(s["xs"]), s, dev(case["g"]), block_weights(blk), precision)
            assert nodx["g_x"] is None
            for n in BO.CONVS:
                if got[n] is not None:
                    assert torch.equal(nodx[n], got[n]) and torch.equal(again[n], got[n]), (name, n)
            assert torch.equal(again["g_x"], got["g_x"])
    assert not bad, bad


def test_a_groups_1_key_changes_nothing(hip):
    """The identity block at F = 1 on 3 x 5: weights that carry groups=1 and stride_in_3x3=False give every gradient and g_x bit for bit as
    weights without the keys -- the keys alone do not move a dense block off the dense kernels."""
    kind, Cin, mid, Cout, stride = BO.BLOCKS[1]
    case = BO.block_case(kind, Cin, mid, Cout, stride, 1, 3, 5)
    blk = device_block(hip, case["params"], stride, "bf16x6")
    s = EB.body_stage_forward(dev(case["x"]), [blk], "bf16x6")[0]
    run = lambda weights: EB.bottleneck_backward(hip.dense_volume(s["xs"]), s, dev(case["g"]), weights, "bf16x6")
    plain, keyed = run(block_weights(blk)), run(dict(block_weights(blk), groups=1, stride_in_3x3=False))
    assert plain["down"] is None and keyed["down"] is None
    for n in ("conv1", "conv2", "conv3", "g_x"):
        assert torch.equal(keyed[n], plain[n]), n


def test_identity_block_with_zero_weights_passes_the_masked_gradient(hip):
    """All conv weights zero, a one-hot G in the last pixel of the last frame: out = relu(b3 + x), and g_x is exactly relu'(out) G; every dW of a
    zero-weight chain but conv3's is exactly zero."""
    kind, Cin, mid, Cout, stride = BO.BLOCKS[1]
    Fr, h, w = 3, 3, 5
    case = BO.block_case(kind, Cin, mid, Cout, stride, Fr, h, w)
    for n in ("conv1", "conv2", "conv3"):
        case["params"][n] = np.zeros_like(case["params"][n])
    blk = device_block(hip, case["params"], stride, "bf16x6")
    s = EB.body_stage_forward(dev(case["x"]), [blk], "bf16x6")[0]
    out = s["out"].cpu()
    assert torch.equal(out, torch.relu(torch.from_numpy(case["x"]) + torch.from_numpy(case["params"]["conv3.b"])[:, None, None, None]))
    hits = 0
    for co in range(0, Cout, 8):
        G = np.zeros((Cout, Fr, h, w), np.float32)
        G[co, Fr - 1, h - 1, w - 1] = 1.5
        got = EB.bottleneck_backward(hip.dense_volume(s["xs"]), s, dev(G), block_weights(blk), "bf16x6")
        want = torch.ops.aten.threshold_backward(torch.from_numpy(G), out, 0)
        assert torch.equal(bits(got["g_x"]), bits(want)), co
        assert not bool(got["conv1"].any()) and not bool(got["conv2"].any())
        hits += int(bool(want.any()))
    assert 0 < hits < Cout // 8                             # both kinds of pixel: the gradient passed and was blocked


def test_frames_do_not_leak(hip):
    """F = 2 on 8 x 16: frame 0 of xs and of every activation filled with +-1e30, the upstream in frame 1 only: every dW and frame 1 of g_x equal
    those of the one-frame run on frame 1 alone, bit for bit (a kernel that read across frames would bring 1e30 into a sum)."""
    kind, Cin, mid, Cout, stride = BO.BLOCKS[0]
    h, w = 8, 16
    case = BO.block_case(kind, Cin, mid, Cout, 1, 1, h, w)
    blk = device_block(hip, case["params"], 1, "bf16x6")
    s1 = EB.body_stage_forward(dev(case["x"]), [blk], "bf16x6")[0]
    one = EB.bottleneck_backward(hip.dense_volume(s1["xs"]), s1, dev(case["g"]), block_weights(blk), "bf16x6")
    g1 = given_of(s1)
    big = np.where(np.arange(h * w).reshape(h, w) % 2 == 0, 1e30, -1e30).astype(np.float32)
    two = lambda a: np.stack([np.broadcast_to(big, a[:, 0].shape), a[:, 0]], 1).astype(np.float32)
    xs2, a2, out = dev(two(case["x"])), dev(two(g1["a2"])), dev(two(g1["out"]))
    acts = dict(a1=haloed(hip, two(g1["a1"])), a2=a2, out=out)
    G = np.concatenate([np.zeros_like(case["g"]), case["g"]], 1)
    both = EB.bottleneck_backward(hip.dense_volume(xs2), acts, dev(G), block_weights(blk), "bf16x6")
    for n in BO.CONVS:
        assert torch.equal(both[n], one[n]), n
    assert torch.equal(both["g_x"][:, 1:], one["g_x"]) and not bool(both["g_x"][:, 0].any())


# ------------------------------------------------------------------------------------------------ the composed body
def device_body(hip, case, precision):
    """-> ({stage: block dicts}, {stage: the stage's input}, per stage per block the device's activations) of the three-stage body of ``case``;
    the stages are numbered 2 .. 4 as in the network."""
    stages, inputs, given = {}, {}, []
    x = dev(case["x"])
    for k, blocks in enumerate(case["stages"]):
        st = k + 2
        stages[st] = [device_block(hip, p, 2 if b == 0 else 1, precision) for b, p in enumerate(blocks)]
        inputs[st] = x
        stash = EB.body_stage_forward(x, stages[st], precision)
        given.append([given_of(s) for s in stash])
        x = stash[-1]["out"]
    return stages, inputs, given


@pytest.mark.parametrize("freeze_at", [2, 3, 4])
@pytest.mark.parametrize("levels", [(1, 2, 3), (3,), (1,)])
def test_body_backward_composed(hip, levels, freeze_at):
    """Three stages of 2 / 3 / 2 blocks, outputs 64 / 128 / 256 channels on 8x16 / 4x8 / 2x4 from a 32-channel 16x32 input, F = 2.  Upstream on
    every stage output, on the last only, on the first only; freeze_at 2, 3, 4: every weight gradient of the stages from freeze_at on by the
    rule, none for the stages below; an upstream on the first stage alone leaves the gradients of the other two exactly zero."""
    precision = "bf16x6"
    case = BO.body_case(levels)
    stages, inputs, given = device_body(hip, case, precision)
    r32 = BO.body_gradients(case, torch.float32, given, freeze_at - 2)
    r64 = BO.body_gradients(case, torch.float64, given, freeze_at - 2)
    dC = {k + 2: (dev(case["g"][k]) if k + 1 in levels else None) for k in range(3)}
    got = EB.body_backward(inputs, stages, dC, precision, freeze_at)
    assert sorted(got) == list(range(freeze_at, 5))
    bad, seen = [], set()
    for st, blocks in got.items():
        for b, g in enumerate(blocks):
            for n in BO.CONVS:
                if g[n] is not None:
                    key = (st - 2, b, n)
                    seen.add(key)
                    TO.check("body levels %s freeze_at %d" % (levels, freeze_at), "s%d.b%d.%s" % (st, b, n), host(g[n]), r32[key], r64[key], bad)
                    if levels == (1,) and st > 2:
                        assert not bool(g[n].any()), key
                    if any(l >= st - 1 for l in levels):              # (an upstream on level l reaches the stages at and below it)
                        assert bool(g[n].any()), key
    assert seen == set(r64)
    again = EB.body_backward(inputs, stages, dC, precision, freeze_at)
    assert all(torch.equal(a[n], b[n]) for st in got for a, b in zip(got[st], again[st]) for n in BO.CONVS if a[n] is not None), "reruns differ"
    assert not bad, bad


@pytest.mark.parametrize("precision", ["bf16x6", "f32"])
def test_fpn_backward_with_dC(hip, precision):
    """want_dC returns the same sixteen gradients bit for bit, and dC_k = inner_k^T G_k by the rule against autograd on the stage outputs;
    the levels not asked for are None."""
    case = FO.fpn_case()
    L64, _ = FO.fpn_forward(case["C"], case["params"], torch.float64)
    L_vals = [v.float() for v in L64]
    Cs = [dev(v) for v in case["C"]]
    keep = [haloed(hip, v.cuda().contiguous()) for v in L_vals]
    l_views = [hip.padded2d_halo_view(buf, g, *v.shape) for (buf, g), v in zip(keep, L_vals)]
    args = ([hip.dense_volume(v) for v in Cs], l_views, [dev(v) for v in case["g"]], [dev(case["params"]["fpn_layer%d.weight" % (k + 1)]) for k in range(4)], precision)
    inner = [dev(case["params"]["fpn_inner%d.weight" % (k + 1)]) for k in range(4)]
    plain = EB.fpn_backward(*args)
    full = EB.fpn_backward(*args, want_dC=True, inner_weights=inner)
    some = EB.fpn_backward(*args, want_dC=(1, 3), inner_weights=inner)
    assert len(plain) == 4 and len(full) == 5
    for other in (full, some):
        assert all(torch.equal(a, b) for ga, gb in zip(plain, other[:4]) for a, b in zip(ga, gb))
    assert some[4][0] is None and some[4][2] is None and torch.equal(some[4][1], full[4][1]) and torch.equal(some[4][3], full[4][3])
    refs = []
    for dt in (torch.float32, torch.float64):
        live = [torch.from_numpy(v).to(dt).requires_grad_(True) for v in case["C"]]
        _, Ps = FO.fpn_forward(live, case["params"], dt, L_vals)
        sum((P * torch.from_numpy(u).to(dt)).sum() for P, u in zip(Ps, case["g"])).backward()
        refs.append([v.grad.double().numpy() for v in live])
    bad = []
    for k in range(4):
        TO.check("fpn dC %s" % precision, "dC%d" % k, host(full[4][k]), refs[0][k], refs[1][k], bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the recompute
def _frames(T, H, W, seed=3):
    from tests import synth
    mean = torch.tensor([102.9801, 115.9465, 122.7717])[None, :, None, None]
    return (torch.from_numpy(synth.synth_frames(T, H, W, seed=seed).astype(np.float32)).permute(0, 3, 1, 2) - mean).cuda()


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6", "f32"])
def test_recompute_against_the_stage_outputs_of_the_pass(hip, precision):
    """R-50 on 8 x 96 x 128: the last ``out`` of the recompute of stages 2-4 (three launches per block, the pass's packed weights, precision and
    plan_frames, from the stage output below) against the stage outputs Cst[k] the pass left in its workspace: at most 4e-6 of max|Cst[k]|,
    the project's figure for ``forward_trainable`` against ``run_hip``.  The observed differences are in DESIGN.md section 9j."""
    from tests.fused_tail_util import backbone
    bb, _ = backbone("R-50-FPN", 11)
    bb.precision = precision
    x = _frames(8, 96, 128)
    bb.forward_channel_major(x)
    key = bb.workspace_key(x)
    inputs = bb.body_stage_inputs(key, 2)
    specs = bb.body_stage_specs(2, bb._packed_names[precision])
    c_views, _, _ = bb.fpn_workspace_views(key)
    ws = bb._ws[key].view(torch.float32)
    worst = 0.0
    for st in (2, 3, 4):
        v = c_views[st - 1]
        off = (v.ptr - ws.data_ptr()) // 4
        cst = ws[off:off + v.C * v.T * v.H * v.W].view(v.C, v.T, v.H, v.W)
        out = EB.body_stage_forward(inputs[st], specs[st], precision, int(bb.plan_frames))[-1]["out"]
        assert out.shape == cst.shape and bool(torch.isfinite(cst).all()) and float(cst.max()) > 0
        d = float((out - cst).abs().max() / cst.abs().max())
        print("recompute %s stage %d: max |out - Cst| / max |Cst| = %.3e, equal %s" % (precision, st, d, torch.equal(out, cst)))
        worst = max(worst, d)
    assert worst <= 4e-6, worst


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model(hip):
    """kittimots preset, R-50, synthetic weights; the stem and layer1 frozen, everything else trainable, the three switches on."""
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
        m.train_decoders = m.train_fpn = m.train_body = True
        m.image_mean = torch.tensor(config.cfg.INPUT.IMAGE_MEAN)
        m.initial_state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        yield m
    finally:
        config.load_preset("defaults")


def _prepare(m, precision, freeze_at=2):
    m.load_state_dict(m.initial_state)
    for mod in (m.backbone, m.embedding_head, m.seediness_head, m.semseg_head):
        if mod is not None:
            mod.precision = precision
    for k, p in m.named_parameters():
        frozen = k.startswith("backbone.body.stem.") or any(k.startswith("backbone.body.layer%d." % st) for st in range(1, freeze_at))
        p.requires_grad_(not frozen)
        p.grad = None


def _inputs(m, T, H, W):
    from tests import semseg_loss_oracle as SO
    frames = _frames(T, H, W)[None]
    sample = SO.make_sample(np.random.default_rng(5), 1, T, H, W, (1, 2, 2))[1:]
    raw = lambda: [{"masks": torch.from_numpy(sample[0]).cuda(), "ignore_masks": torch.from_numpy(sample[1]).cuda(), "category_ids": torch.from_numpy(sample[2]).cuda()}]
    return frames, raw


def _train_pass(m, frames, raw):
    """forward with the graph + backward of the summed losses; the four maps (with their retained gradients) are caught on the way."""
    bb = m.backbone
    caught = []
    inner = bb.forward_trainable_body

    def catching(x, freeze_at):
        outs = inner(x, freeze_at)
        for o in outs:
            o.retain_grad()
        caught.append((outs, freeze_at))
        return outs
    for p in m.parameters():
        p.grad = None
    bb.forward_trainable_body = catching
    try:
        out = m(frames, raw())
    finally:
        del bb.forward_trainable_body
    loss = sum(out["optimization_losses"].values())
    assert loss.requires_grad and bool(torch.isfinite(loss))
    loss.backward()
    assert len(caught) == 1
    return caught[0][0], caught[0][1], loss.detach()


def _check_body_gradients(hip, m, name, frames, maps, freeze_at):
    """The body's gradients by the rule.  The oracle is the body linearised around the device's recomputed activations, fed into the FPN oracle
    on the stage outputs and merged laterals the pass left in its workspace; its upstream is the device's own dP_k."""
    bb = m.backbone
    x = frames.reshape((-1,) + tuple(frames.shape[-3:]))
    key = bb.workspace_key(x)
    c_views, l_views, _ = bb.fpn_workspace_views(key)
    ws = bb._ws[key].view(torch.float32)
    off = lambda v: (v.ptr - ws.data_ptr()) // 4
    Cs = [ws[off(v):off(v) + v.C * v.T * v.H * v.W].view(v.C, v.T, v.H, v.W).clone().cpu() for v in c_views]
    Ls = [ws[off(v):off(v) + v.C * v.c_stride].view(v.C, v.T, v.H, v.y_stride)[:, :, 1:v.H - 1, 1:v.W - 1].clone().cpu() for v in l_views]
    specs = bb.body_stage_specs(freeze_at, bb._packed_names[bb.precision])
    inputs = bb.body_stage_inputs(key, freeze_at)
    given = [[given_of(s) for s in EB.body_stage_forward(inputs[st], specs[st], bb.precision, int(bb.plan_frames))] for st in range(freeze_at, 5)]
    ups = [o.grad.permute(1, 0, 2, 3).detach().cpu() for o in maps]
    fpn = {n: p.detach().cpu().numpy() for n, p in bb.fpn.named_parameters()}
    refs = []
    for dt in (torch.float32, torch.float64):
        live = []
        for st in range(freeze_at, 5):
            live.append([])
            for blk in getattr(bb.body, "layer%d" % st):
                p = {}
                for n, conv, bn in (("conv1", blk.conv1, blk.bn1), ("conv2", blk.conv2, blk.bn2), ("conv3", blk.conv3, blk.bn3)) + (
                        (("down", blk.downsample[0], blk.downsample[1]),) if blk.downsample is not None else ()):
                    s, b = bn.scale_shift()
                    p[n], p[n + ".s"], p[n + ".b"] = conv.weight.detach().cpu().numpy(), s.detach().cpu().numpy(), b.detach().cpu().numpy()
                live[-1].append(BO.live_params(p, dt))
        outs = BO.body_forward(BO.frames_first(Cs[freeze_at - 2]).to(dt), live, dt, given, stage_in=[Cs[st - 2] for st in range(freeze_at, 5)])
        C_or = [c.to(dt) for c in Cs[:freeze_at - 1]]
        for st, o in zip(range(freeze_at, 5), outs):
            o = BO.frames_first(o)
            C_or.append(o + (Cs[st - 1].to(dt) - o).detach())               # the FPN reads the pass's stage output
        _, Ps = FO.fpn_forward(C_or, fpn, dt, Ls)
        sum((P * u.to(dt)).sum() for P, u in zip(Ps, ups)).backward()
        g = {}
        for st, blocks in zip(range(freeze_at, 5), live):
            for b, lp in enumerate(blocks):
                for n in BO.CONVS:
                    if n in lp:
                        g["backbone.body.layer%d.%d.%s.weight" % (st, b, "downsample.0" if n == "down" else n)] = lp[n].grad.double().numpy()
        refs.append(g)
    named = dict(m.named_parameters())
    bad = []
    assert set(refs[1]) == set(m.body_parameters(freeze_at))
    for n in refs[1]:
        TO.check(name, n[len("backbone.body."):], host(named[n].grad), refs[0][n], refs[1][n], bad)
    return bad


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"])
def test_training_model_end_to_end(hip, model, precision):
    """One clip of 8 x 96 x 128, the three switches on, the stem and layer1 frozen.  The four maps are the bits of the no-grad ``run_backbone``;
    the summed losses' backward fills finite gradients on exactly the 42 body, 16 FPN and 67 decoder parameters and none on the stem or
    layer1; the body's meet the rule; a second pass gives the same bits; a step on the FPN parameters alone leaves the body's packed tensors
    the same objects, one SGD step (lr 1e-3) on everything re-packs the body and moves the no-grad output."""
    from stemseg_amd.utils.constants import ModelOutput
    m, bb = model, model.backbone
    _prepare(m, precision)
    frames, raw = _inputs(m, 8, 96, 128)
    with torch.no_grad():
        ref = [v.clone() for v in m.run_backbone(frames).values()]
        before = m(frames, raw())[ModelOutput.INFERENCE][ModelOutput.EMBEDDINGS].clone()
    maps, freeze_at, loss = _train_pass(m, frames, raw)
    assert freeze_at == 2 and all(a.requires_grad and torch.equal(a, b) for a, b in zip(maps, ref))
    named = dict(m.named_parameters())
    body, fpn, dec = m.body_parameters(2), m.fpn_parameters(), m.decoder_parameters()
    assert (len(body), len(fpn), len(dec)) == (42, 16, 67)
    filled = {k for k, p in named.items() if p.grad is not None}
    assert filled == set(body) | set(fpn) | set(dec), sorted(filled ^ (set(body) | set(fpn) | set(dec)))
    assert not any(k.startswith("backbone.body.stem.") or k.startswith("backbone.body.layer1.") for k in filled)
    assert all(bool(torch.isfinite(named[k].grad).all()) for k in filled) and all(bool(named[k].grad.any()) for k in body)
    bad = _check_body_gradients(hip, m, "end to end %s" % precision, frames, maps, 2)
    first = {k: named[k].grad.clone() for k in filled}
    _, _, loss2 = _train_pass(m, frames, raw)
    assert torch.equal(loss, loss2) and all(torch.equal(named[k].grad, first[k]) for k in filled), "reruns differ"
    (w, keep), n_body = bb._packed[precision][1], bb._packed[precision][2]
    body_ids = [id(t) for t in keep[:n_body]]
    torch.optim.SGD(list(fpn.values()), lr=1e-3).step()
    with torch.no_grad():
        mid = m(frames, raw())[ModelOutput.INFERENCE][ModelOutput.EMBEDDINGS].clone()
    (w2, keep2), n_body2 = bb._packed[precision][1], bb._packed[precision][2]
    assert not torch.equal(mid, before)
    assert w2 is w and n_body2 == n_body and [id(t) for t in keep2[:n_body]] == body_ids, "a step on the FPN alone re-packed the body"
    names_before = bb._packed_names[precision]
    torch.optim.SGD([named[k] for k in sorted(filled)], lr=1e-3).step()
    with torch.no_grad():
        after = m(frames, raw())[ModelOutput.INFERENCE][ModelOutput.EMBEDDINGS]
    assert not torch.equal(after, mid)
    assert bb._packed[precision][1][0] is not w and bb._packed_names[precision] is not names_before, "the step did not re-pack the body"
    assert bb._packed[precision][0][0][0] == bb._signature_of(bb.body)
    assert not bad, bad


def test_freeze_at_4_trains_layer4_only(hip, model):
    """layer2 and layer3 frozen as well: the pass runs with freeze_at = 4, only layer4's 10 weights of the body get a gradient, and they meet
    the rule."""
    m = model
    _prepare(m, "f16x3", freeze_at=4)
    frames, raw = _inputs(m, 8, 96, 128)
    maps, freeze_at, _ = _train_pass(m, frames, raw)
    assert freeze_at == 4
    filled = {k for k, p in m.named_parameters() if p.grad is not None and k.startswith("backbone.body.")}
    assert filled == set(m.body_parameters(4)) and len(filled) == 10 and all(k.startswith("backbone.body.layer4.") for k in filled)
    bad = _check_body_gradients(hip, m, "freeze_at 4", frames, maps, 4)
    assert not bad, bad


def test_backward_refuses_a_workspace_another_pass_has_used(hip, model):
    """Forward with a graph, a no-grad forward of the same shape on the same lane, then backward: the RuntimeError names the workspace and the
    remedy.  With the training pass on a lane of its own the same sequence goes through."""
    m, bb = model, model.backbone
    _prepare(m, "f16x3")
    frames, raw = _inputs(m, 8, 64, 64)
    loss = sum(m(frames, raw())["optimization_losses"].values())
    with torch.no_grad():
        m.run_backbone(frames)
    with pytest.raises(RuntimeError, match=r"EncoderFunction\.backward: 1 more encoder passes have run on the workspace .*lane"):
        loss.backward()
    try:
        bb.lane = 1
        for p in m.parameters():
            p.grad = None
        loss = sum(m(frames, raw())["optimization_losses"].values())
        bb.lane = 0
        with torch.no_grad():
            m.run_backbone(frames)
        loss.backward()
    finally:
        bb.lane = 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.body_parameters(2).values())
