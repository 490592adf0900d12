"""GPU tests of the decoder-tail backward: the heads, the trilinear adjoint and GroupNorm -> ReLU -> pool against torch-CPU autograd
(tests/decoder_tail_oracle.py), the composed tail of a decoder against the fp64 restatement of the unfolded reference decoder, and
TrainingModel.forward with only tail parameters trainable.

Bounds, per case (the rule of tests/test_gpu_semseg_loss.py): the oracle runs in fp32 and in fp64 on the same input; the device may be
FACTOR = 4 x that case's own fp32-versus-fp64 spread away from the fp64 result, the spread floored at 2^-24 (rounding a result to fp32
alone); gradients on the max norm relative to max|g|; a term that is exactly zero in the oracle must be exactly zero on the device.
Every test prints spread, bound and device error before it asserts; the per-case table is in DESIGN.md section 9g.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

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


# ------------------------------------------------------------------------------------------------ heads
@pytest.mark.parametrize("n_out", [1, 4, 10])
@pytest.mark.parametrize("Cin", TO.HEAD_CIN)
def test_heads_backward_vs_autograd(hip, Cin, n_out):
    """Every activation code and grid axis (HEAD_TABLES), V = 70 and V = 4099, with and without dx, and the dz-direct form.  The forward
    output handed to the kernel is the fp64 oracle's, rounded to fp32: what a forward kernel leaves."""
    bad = []
    for dims in TO.HEAD_DIMS:
        c = TO.heads_case(Cin, n_out, dims)
        name = "heads Cin %d n_out %d V %d" % (Cin, n_out, int(np.prod(dims)))
        r32, r64 = TO.heads_oracle(c, torch.float32), TO.heads_oracle(c, torch.float64)
        args = (dev(c["x"]), dev(c["w"]), dev(c["g"]), dev(r64["out"].astype(np.float32)), c["act"], c["axis"], dev(c["gt"]), dev(c["gy"]), dev(c["gx"]))
        dx, dw, db = hip.heads_backward(*args)
        for what, got in (("dx", dx), ("dw", dw), ("db", db)):
            TO.check(name, what, host(got), r32[what], r64[what], bad)
        again = hip.heads_backward(*args)
        assert all(torch.equal(a, b) for a, b in zip((dx, dw, db), again)), "reruns differ"
        nodx = hip.heads_backward(*args, want_dx=False)
        assert nodx[0] is None and torch.equal(nodx[1], dw) and torch.equal(nodx[2], db)
        # the dz-direct form: a level matrix of the folded tail (no activation table, no bias; g is the gradient of w x)
        l32, l64 = TO.heads_oracle(c, torch.float32, False), TO.heads_oracle(c, torch.float64, False)
        dx, dw, db = hip.heads_backward(args[0], args[1], args[2])
        for what, got in (("dx", dx), ("dw", dw)):
            TO.check(name + " dz-direct", what, host(got), l32[what], l64[what], bad)
        TO.check(name + " dz-direct", "db", host(db), torch.from_numpy(c["g"]).sum((1, 2, 3)).double().numpy(), c["g"].astype(np.float64).sum((1, 2, 3)), bad)
        assert all(torch.equal(a, b) for a, b in zip((dx, dw, db), hip.heads_backward(args[0], args[1], args[2])))
    assert not bad, bad


def test_heads_backward_of_an_all_zero_upstream_is_exactly_zero(hip):
    c = TO.heads_case(64, 10, (2, 5, 7))
    out = TO.heads_oracle(c, torch.float64)["out"].astype(np.float32)
    z = np.zeros_like(c["g"])
    for got in hip.heads_backward(dev(c["x"]), dev(c["w"]), dev(z), dev(out), c["act"], c["axis"], dev(c["gt"]), dev(c["gy"]), dev(c["gx"])):
        assert not got.any()


@pytest.mark.parametrize("linear", [False, True], ids=["fused heads", "level matrix"])
def test_heads_function_forward_and_backward(hip, linear):
    """modeling.ops.HeadsFunction end to end (forward on the inference kernel): W % 4 == 0 as the fused heads need; the level matrix on
    an odd shape."""
    from stemseg_amd.modeling.ops import HeadsFunction
    dims = (3, 5, 7) if linear else (2, 4, 8)
    c = TO.heads_case(64, 10, dims, seed=5)
    r32, r64 = TO.heads_oracle(c, torch.float32, not linear), TO.heads_oracle(c, torch.float64, not linear)
    x, w, b = dev(c["x"]).requires_grad_(True), dev(c["w"]).requires_grad_(True), dev(c["b"]).requires_grad_(True)
    if linear:
        out = HeadsFunction.apply(x, w, None, None, None, None)
    else:
        out = HeadsFunction.apply(x, w, b, c["act"], c["axis"], (dev(c["gt"]), dev(c["gy"]), dev(c["gx"])))
    out.backward(dev(c["g"]))
    bad = []
    assert np.allclose(host(out), r64["out"], rtol=1e-5, atol=1e-5)      # (the forward kernels have their own tests: this is the wiring)
    for what, p in (("dx", x), ("dw", w)) + (() if linear else (("db", b),)):
        TO.check("HeadsFunction", what, host(p.grad), r32[what], r64[what], bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ trilinear adjoint
@pytest.mark.parametrize("scale", TO.UP_SCALES, ids=lambda s: "x".join(map(str, s)))
def test_trilinear_adjoint_vs_autograd_and_inner_products(hip, scale):
    """C = 3, T 1..3, H 1..5, W 1..9: every border clamp, single rows, columns and frames.  Against autograd, and <up(x), g> = <x, up^T(g)>
    in fp64 from the device outputs: the forward rounds 7 lerps per output and the adjoint once per input, so the two inner products may
    differ by (7 sum |up(x)| |g| + sum |x| |up^T(g)|) 2^-24."""
    bad, worst = [], {}
    for T in (1, 2, 3):
        for H in range(1, 6):
            for W in range(1, 10):
                x, g = TO.up_case(scale, T, H, W)
                (_, r32), (_, r64) = TO.up_oracle(x, g, scale, torch.float32), TO.up_oracle(x, g, scale, torch.float64)
                d_in = hip.upsample_trilinear_backward(dev(g), *scale)
                spread, err = TO.max_norm_err(r32, r64), TO.max_norm_err(host(d_in), r64)
                b = TO.bound(spread, r64)
                if T not in worst or err / b > worst[T][2] / worst[T][1]:
                    worst[T] = (spread, b, err, (T, H, W))
                if not err <= b:
                    bad.append((scale, T, H, W, err, b))
                up = host(hip.upsample_trilinear(dev(x), *scale))
                lhs, rhs = float((up * g).sum()), float((x.astype(np.float64) * host(d_in)).sum())
                tol = (7 * float((np.abs(up) * np.abs(g)).sum()) + float((np.abs(x) * np.abs(host(d_in))).sum())) * 2.0 ** -24
                if not abs(lhs - rhs) <= tol:
                    bad.append((scale, T, H, W, "inner products", lhs, rhs, tol))
                assert torch.equal(d_in, hip.upsample_trilinear_backward(dev(g), *scale)), "reruns differ"
    for T, (spread, b, err, shape) in sorted(worst.items()):
        print("trilinear adjoint %s T %d: worst case %s spread %.2e bound %.2e device %.2e" % (scale, T, shape, spread, b, err))
    assert not bad, bad


def test_upsample_module_carries_gradients(hip):
    from stemseg_amd.modeling.common import UpsampleTrilinear3D
    x, g = TO.up_case((2, 2, 2), 2, 3, 4)
    (o32, r32), (o64, r64) = TO.up_oracle(x, g, (2, 2, 2), torch.float32), TO.up_oracle(x, g, (2, 2, 2), torch.float64)
    up = UpsampleTrilinear3D(scale_factor=(2, 2, 2))
    xx = dev(x)[None].requires_grad_(True)
    out = up(xx)
    assert out.requires_grad and torch.equal(out.detach(), up(xx.detach())) and not up(xx.detach()).requires_grad
    out.backward(dev(g)[None])
    bad = []
    TO.check("UpsampleTrilinear3D", "dx", host(xx.grad[0]), r32, r64, bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ GroupNorm + ReLU + pool
@pytest.mark.parametrize("H,W", TO.GN_HW)
@pytest.mark.parametrize("C,groups", TO.GN_CG)
def test_gn_relu_pool_backward_vs_autograd(hip, C, groups, H, W):
    """T 1..5 (odd T: To = (T + 1) / 2), pool none and average, through modeling.ops.GnReluPoolFunction (forward on the inference kernel,
    statistics from the forward's statistics kernel); the upstream gradient has zeros and negatives."""
    from stemseg_amd.modeling.ops import GnReluPoolFunction
    bad = []
    for T in TO.GN_T:
        for pool in (0, 1):
            c = TO.gn_case(C, groups, T, H, W, pool)
            name = "gn C %d G %d T %d %dx%d pool %d" % (C, groups, T, H, W, pool)
            r32, r64 = TO.gn_oracle(c, torch.float32), TO.gn_oracle(c, torch.float64)
            x = dev(c["x"]).requires_grad_(True)
            gamma, beta = dev(c["gamma"]).requires_grad_(True), dev(c["beta"]).requires_grad_(True)
            stats = hip.groupnorm_stats(x.detach(), groups, TO.GN_EPS) if groups else None
            out = GnReluPoolFunction.apply(x, stats, gamma if groups else None, beta if groups else None, groups, pool)
            out.backward(dev(c["g"]))
            assert np.allclose(host(out), r64["out"], rtol=1e-5, atol=1e-5), name      # (the forward kernel has its own tests: the wiring)
            TO.check(name, "dx", host(x.grad), r32["dx"], r64["dx"], bad)
            if groups:
                TO.check(name, "dgamma", host(gamma.grad), r32["dgamma"], r64["dgamma"], bad)
                TO.check(name, "dbeta", host(beta.grad), r32["dbeta"], r64["dbeta"], bad)
            runs = [hip.gn_relu_pool_backward(x.detach(), groups, stats, gamma.detach(), beta.detach(), pool, dev(c["g"])) for _ in range(2)]
            assert torch.equal(runs[0][0], x.grad) and torch.equal(runs[0][0], runs[1][0]), "reruns differ"
            if groups:
                assert all(torch.equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:])) and torch.equal(runs[0][1], gamma.grad)
            else:
                assert runs[0][1] is None and runs[0][2] is None and gamma.grad is None
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the composed tail
def _decoder(kind, T):
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder
    from stemseg_amd.modeling.semseg_decoder import SqueezeExpandDecoder
    norm = lambda c: nn.GroupNorm(8, c)
    if kind == "embedding":        # 'xyff' with tanh and the seediness output: 4 + 2 + 1 channels
        m = SqueezingExpandDecoder(32, (32, 32, 32, 32), 4, tanh_activation=True, seediness_output=True, experimental_dims="xyff",
                                   PoolType=nn.AvgPool3d, NormType=norm, num_frames=T)
    else:                          # 3 classes + the foreground channel
        m = SqueezeExpandDecoder(32, 3, (32, 32, 32, 32), (4, 8, 16, 32), foreground_channel=True, PoolType=nn.AvgPool3d, NormType=norm, num_frames=T)
    return m


RELU_MARGIN_COMPOSED = 1e-5


@pytest.mark.parametrize("T", [4, 8])
@pytest.mark.parametrize("kind", ["embedding", "semseg"])
def test_composed_tail_vs_the_unfolded_reference_decoder(hip, kind, T):
    """in_channels 32, inter (32, 32, 32, 32), GroupNorm(8), H4 x W4 = 8 x 16.  forward_tail_trainable against run_hip (4e-6 of
    max(1, |x|): the README's figure for the fold against the step-by-step form), then the gradients of every tail parameter and of the
    four last conv outputs against the unfolded reference decoder restated in torch (fp32 and fp64) from those conv outputs on.
    The conv outputs come from the device, so their pre-ReLU values cannot be placed: the features are the first of a fixed sequence of
    seeds whose pre-ReLU values all keep |y| >= 1e-5 in fp64 -- ten times the 1e-6 the fp32 evaluation of fma(x, rstd gamma, beta -
    mean rstd gamma) can move a value of this size, so no sign is in doubt."""
    torch.manual_seed(11)
    m = _decoder(kind, T)
    with torch.no_grad():
        for blk, idx in m._LAST_STAGE:
            gn = getattr(m, blk)[idx + 1]
            gn.weight.copy_(1.0 + 0.3 * torch.randn(32))
            gn.bias.copy_(0.2 * torch.randn(32))
        if kind == "embedding":
            m.conv_variance.bias.copy_(0.1 * torch.randn(2))
    m = m.cuda()
    acts = m._train_acts()
    pools = [m.pool_flags[2], m.pool_flags[1], m.pool_flags[0], 0]
    cpu = {dt: _decoder(kind, T).to(dt) for dt in (torch.float32, torch.float64)}
    for t in cpu.values():
        t.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    for seed in range(20):
        g = torch.Generator().manual_seed(100 * T + seed)
        feats = [torch.randn(32, T, h, w, generator=g).cuda() for h, w in ((1, 2), (2, 4), (4, 8), (8, 16))]
        convouts = [o[0] for o in m._last_conv_outputs(m._packed(), feats)]
        c = m._packed()
        act = list(c["act"]) if acts is None else list(acts)
        grids = tuple(None if v is None else v.cpu() for v in m._grid(c, T, 8, 16, feats[0].device))
        leaves = [d.detach().cpu().double().requires_grad_(True) for d in convouts]
        out64, pre = TO.unfolded_tail(cpu[torch.float64], leaves, act, c["axes"], grids, m.t_scales, pools, torch.float64)
        margin = min(float(p.detach().abs().min()) for p in pre)
        print("seed %d: min |pre-ReLU| %.2e" % (seed, margin))
        if margin >= RELU_MARGIN_COMPOSED:
            break
    else:
        raise AssertionError("no seed keeps the pre-ReLU values away from 0")
    ref = m.run_hip(feats, 0, acts)
    out = m.forward_tail_trainable(feats, acts)
    diff = float(((out.detach() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    print("%s T %d: forward_tail_trainable vs run_hip, max |diff| / max(1, |x|) %.2e" % (kind, T, diff))
    assert out.shape == ref.shape and diff <= 4e-6
    up = torch.randn(out.shape, generator=torch.Generator().manual_seed(7))
    out.backward(up.cuda())
    names = m.tail_parameter_names()
    got = {n: host(p.grad) for n, p in m.named_parameters() if p.grad is not None}
    assert set(got) == set(names), (sorted(got), sorted(names))
    got.update({"conv output %dx" % s: host(d.grad) for s, d in zip((32, 16, 8, 4), m.tail_conv_outputs)})
    want = {}
    for dt, trunk in cpu.items():
        leaves = [d.detach().cpu().to(dt).requires_grad_(True) for d in convouts]
        o, _ = TO.unfolded_tail(trunk, leaves, act, c["axes"], grids, m.t_scales, pools, dt)
        o.backward(up.to(dt))
        want[dt] = {n: host(p.grad) for n, p in trunk.named_parameters() if p.grad is not None}
        want[dt].update({"conv output %dx" % s: host(d.grad) for s, d in zip((32, 16, 8, 4), leaves)})
    assert set(want[torch.float64]) == set(got)
    bad = []
    for n in sorted(got):
        TO.check("%s T %d" % (kind, T), n, got[n], want[torch.float32][n], want[torch.float64][n], bad)
    # a second pass gives the same bits
    for p in m.parameters():
        p.grad = None
    out2 = m.forward_tail_trainable(feats, acts)
    out2.backward(up.cuda())
    assert torch.equal(out2, out)
    assert all(np.array_equal(host(p.grad), got[n]) for n, p in m.named_parameters() if p.grad is not None)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the whole model
def test_training_model_forward_fills_exactly_the_tail_gradients(hip):
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    from tests import semseg_loss_oracle as SO
    from tests import synth
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        m = build_model()
        sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], 11)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()})
        m = m.cuda().eval()
        tail = m.tail_parameters()
        for p in m.parameters():
            p.requires_grad_(False)
        for p in tail.values():
            p.requires_grad_(True)
        frames = torch.from_numpy(synth.synth_frames(8, 96, 128, seed=3).astype(np.float32)).permute(0, 3, 1, 2) - \
            torch.tensor(config.cfg.INPUT.IMAGE_MEAN)[None, :, None, None]
        _, masks, ig, cat = SO.make_sample(np.random.default_rng(5), 1, 8, 96, 128, (1, 2, 2))
        raw = lambda: [{"masks": torch.from_numpy(masks).cuda(), "ignore_masks": torch.from_numpy(ig).cuda(), "category_ids": torch.from_numpy(cat).cuda()}]
        out = m(frames[None].cuda(), raw())
        loss = sum(out["optimization_losses"].values())
        assert loss.requires_grad and torch.isfinite(loss)
        loss.backward()
        named = dict(m.named_parameters())
        filled = {k for k, p in named.items() if p.grad is not None}
        assert filled == set(tail), (sorted(filled ^ set(tail)))
        assert all(torch.isfinite(named[k].grad).all() and named[k].grad.any() for k in tail), [k for k in tail if not named[k].grad.any()]
        grads = {k: named[k].grad.clone() for k in tail}
        # the same by hand: frozen backbone, the decoders' trainable tails, the losses
        for p in m.parameters():
            p.grad = None
        feats = m.run_backbone(frames[None].cuda())
        stack = lambda s: [feats[k].reshape((1, 8) + tuple(feats[k].shape[1:])).permute(0, 2, 1, 3, 4) for k in s]
        sem = torch.stack([m.semseg_head.forward_tail_trainable([f[0] for f in stack(m.semseg_feature_map_scale)[::-1]])], 0).permute(0, 2, 1, 3, 4)
        emb = torch.stack([m.embedding_head.forward_tail_trainable([f[0] for f in stack(m.embedding_head_feature_map_scale)], m.embedding_head._acts())], 0)
        if m.seediness_head is not None:
            emb = torch.cat((emb, torch.stack([m.seediness_head.forward_tail_trainable([f[0] for f in stack(m.seediness_head_feature_map_scale)])], 0)), 1)
        out2 = m.compute_losses(emb, sem, m.resize_masks(raw()))
        loss2 = sum(out2["optimization_losses"].values())
        loss2.backward()
        assert torch.equal(loss2, loss)
        assert all(torch.equal(named[k].grad, grads[k]) for k in tail)
        with torch.no_grad():                                   # the validation path is what it was
            out3 = m(frames[None].cuda(), raw())
        assert not sum(out3["optimization_losses"].values()).requires_grad
    finally:
        config.load_preset("defaults")
