"""GPU tests of the ResNeXt body backward (csrc/conv_backward.hip conv2d_grouped_wgrad; hip.conv2d_grouped_wgrad / conv2d_grouped_dgrad; the
``groups`` / ``stride_in_3x3`` keys of encoder_backward.bottleneck_backward / body_stage_forward / body_backward; ResNetFPN.train_resnext;
TrainingModel.train_resnext) against torch-CPU autograd (tests/resnext_backward_oracle.py).

The rule is that of tests/test_gpu_body_backward.py: the oracle runs in fp32 and in fp64 on the case's own input, linearised around the device's
recomputed activations where there are any; the device may be FACTOR = 4 x that spread, floored at 2^-24, away from the fp64 result, on the max
norm relative to max|reference|.  Every case prints its spread, bound and device error before the test asserts; the per-family table is in
DESIGN.md section 9m."""
import ctypes as C

import numpy as np
import pytest
import torch

from stemseg_amd.modeling import encoder_backward as EB
from tests import body_backward_oracle as BO
from tests import decoder_tail_oracle as TO
from tests import resnext_backward_cases as RC
from tests import resnext_backward_oracle as RO
from tests import test_gpu_body_backward as TB
from tests.test_gpu_body_backward import _check_body_gradients, _frames, _inputs, _prepare, _train_pass, bits, dev, haloed, host

pytestmark = pytest.mark.gpu

GUARD = 64
_oracles = {}


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def oracle(g, cg, s, dims):
    """The case and its fp32 and fp64 references: computed once, shared by the tests, never written to."""
    key = (g, cg, s) + tuple(dims)
    if key not in _oracles:
        case = RO.conv_case(g, cg, s, *dims)
        _oracles[key] = (case, RO.conv_oracle(case, torch.float32), RO.conv_oracle(case, torch.float64))
    return _oracles[key]


def wgrad_guarded(hip, x, dy, groups, stride):
    """conv2d_grouped_wgrad through the C call: dw inside a NaN-filled buffer with guards on both sides, the workspace filled with NaN.
    -> (dw, the guards are intact)"""
    Cn, Fr, H, W = x.shape
    buf, geo = haloed(hip, x)
    v = hip.padded2d_halo_view(buf, geo, Cn, Fr, H, W)
    n = Cn * (Cn // groups) * 9
    whole = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    nbytes = hip.lib().stemseg_hip_conv2d_grouped_wgrad_workspace_bytes(Cn, groups, stride, Fr, H, W)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    assert nbytes > 0 and ws.data_ptr() % 256 == 0
    d = dev(dy) if isinstance(dy, np.ndarray) else dy
    hip.check(hip.lib().stemseg_hip_conv2d_grouped_wgrad(C.byref(v), hip.ptr(d), Cn, groups, stride, whole.data_ptr() + 4 * GUARD, hip.ptr(ws), nbytes,
                                                          hip.stream()))
    intact = bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[GUARD + n:]).all())
    return whole[GUARD:GUARD + n].view(Cn, Cn // groups, 3, 3).clone(), intact


# ------------------------------------------------------------------------------------------------ the weight gradient
@pytest.mark.parametrize("g,cg,s", RC.CONV_CASES)
def test_wgrad_vs_autograd(hip, g, cg, s):
    """dW by the rule on 2 x 4 (F 1), 13 x 37 (F 3) and 40 x 70 (F 2): finite, inside intact guards, from a NaN-filled workspace, the same
    bits from a second call and from the binding; (1, 32) at stride 1 also against conv2d_wgrad by the rule."""
    bad = []
    for dims in RC.WGRAD_MAPS:
        case, r32, r64 = oracle(g, cg, s, dims)
        name = "wgrad (%d, %d) s%d %s" % (g, cg, s, dims)
        dw, intact = wgrad_guarded(hip, case["x"], case["g"], g, s)
        assert intact, name
        assert bool(torch.isfinite(dw).all()), name
        TO.check(name, "dw", host(dw), r32["dw"], r64["dw"], bad)
        again, _ = wgrad_guarded(hip, case["x"], case["g"], g, s)
        buf, geo = haloed(hip, case["x"])
        bound = hip.conv2d_grouped_wgrad(hip.padded2d_halo_view(buf, geo, *case["x"].shape), dev(case["g"]), g, s)
        assert torch.equal(bits(again), bits(dw)) and torch.equal(bits(bound), bits(dw)), name
        if (g, s) == (1, 1):
            plain = hip.conv2d_wgrad(hip.padded2d_halo_view(buf, geo, *case["x"].shape), dev(case["g"]), 9, want_db=False)[0]
            TO.check(name, "wgrad9", host(plain), r32["dw"], r64["dw"], bad)
    assert not bad, bad


@pytest.mark.parametrize("g,cg,s", RC.CONV_CASES)
def test_wgrad_one_hot_dy_copies_the_patch(hip, g, cg, s):
    """A one-hot dy at the first pixel of frame 0 and at the last pixel of the last frame: dW[co] is the 3 x 3 x Cg patch of x there, bit for
    bit, and every other row of dW is exactly zero."""
    for dims in RC.WGRAD_MAPS:
        case, _, _ = oracle(g, cg, s, dims)
        x = case["x"]
        Cn, Fr, H, W = x.shape
        _, _, Ho, Wo = case["g"].shape
        xh = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
        for co, f, y, xx in ((Cn - 1, 0, 0, 0), (cg % Cn, Fr - 1, Ho - 1, Wo - 1), (Cn // 2, Fr - 1, Ho - 1, Wo - 1)):
            dy = np.zeros_like(case["g"])
            dy[co, f, y, xx] = 1.0
            dw, intact = wgrad_guarded(hip, x, dy, g, s)
            grp = co // cg
            want = np.zeros((Cn, cg, 3, 3), np.float32)
            want[co] = xh[grp * cg:(grp + 1) * cg, f, s * y:s * y + 3, s * xx:s * xx + 3]
            assert intact and torch.equal(bits(dw), bits(torch.from_numpy(want))), (g, cg, s, dims, co, f, y, xx)


@pytest.mark.parametrize("g,cg,s", [(4, 4, 1), (2, 16, 2), (1, 32, 2)])
def test_wgrad_frames_do_not_leak(hip, g, cg, s):
    """x non-zero in frame 0 only, dy in frame 1 only: dW is exactly zero."""
    for dims in RC.WGRAD_MAPS[1:]:
        case, _, _ = oracle(g, cg, s, dims)
        x, dy = case["x"].copy() + 1.0, case["g"].copy()
        x[:, 1:] = 0.0
        dy[:, 0] = 0.0
        dy[:, 2:] = 0.0
        dw, intact = wgrad_guarded(hip, x, dy, g, s)
        assert intact and not bool(dw.any()), (g, cg, s, dims)


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("g,cg", RC.LEAK_WIDTHS)
def test_wgrad_groups_do_not_leak(hip, g, cg, s):
    """One group's input all NaN, and in another run all inf: the rows of dW of every other group are the clean run's, bit for bit (with 4 and 8
    channels per group the poisoned group shares a 16 x 16 block of the kernel with the others)."""
    for dims in RC.WGRAD_MAPS[1:]:
        case, _, _ = oracle(g, cg, s, dims)
        clean, _ = wgrad_guarded(hip, case["x"], case["g"], g, s)
        for poisoned in (0, g - 1):
            for value in (np.nan, np.inf):
                x = case["x"].copy()
                x[poisoned * cg:(poisoned + 1) * cg] = value
                dw, intact = wgrad_guarded(hip, x, case["g"], g, s)
                rows = np.ones(g * cg, bool)
                rows[poisoned * cg:(poisoned + 1) * cg] = False
                rows = torch.from_numpy(rows)
                assert intact and torch.equal(bits(dw)[rows], bits(clean)[rows]), (g, cg, s, dims, poisoned, value)
                assert not bool(torch.isfinite(dw[~rows]).all())


# ------------------------------------------------------------------------------------------------ the data gradient
@pytest.mark.parametrize("g,cg,s", RC.CONV_CASES)
def test_dgrad_vs_autograd(hip, g, cg, s):
    """dx by the rule, with and without the ReLU mask (read from the interior of a haloed buffer), and the same bits from a second call."""
    bad = []
    for dims in RC.WGRAD_MAPS:
        dims = RC.dgrad_map(*dims, s)
        case, r32, r64 = oracle(g, cg, s, dims)
        name = "dgrad (%d, %d) s%d %s" % (g, cg, s, dims)
        dy, w = dev(case["g"]), dev(case["w"])
        dx = hip.conv2d_grouped_dgrad(dy, w, g, s, "f32")
        assert tuple(dx.shape) == case["x"].shape
        TO.check(name, "dx", host(dx), r32["dx"], r64["dx"], bad)
        buf, geo = haloed(hip, case["m"])
        mask = hip.padded2d_interior_view(buf, geo, *case["m"].shape)
        dxm = hip.conv2d_grouped_dgrad(dy, w, g, s, "f32", mask=mask)
        keep = case["m"] > 0
        TO.check(name, "dx mask", host(dxm), r32["dx"] * keep, r64["dx"] * keep, bad)
        assert torch.equal(bits(dxm), bits(hip.relu_backward(mask, dx)))
        assert torch.equal(bits(hip.conv2d_grouped_dgrad(dy, w, g, s, "f32")), bits(dx)), name
    assert not bad, bad


@pytest.mark.parametrize("g,cg,s", RC.CONV_CASES)
def test_adjoint_identities(hip, g, cg, s):
    """<conv(x; w, 0), g> = <w, dW> = <x, dx> from device outputs summed in fp64, the forward ``conv2d_grouped`` in f32.  The bound of
    tests/test_gpu_fpn_backward.py::test_adjoint_identities: each side within (terms per element + 2) 2^-24 S of the exact value, S the sum of
    the absolute products behind it; 9 Cg terms per element for the convolution and the data gradient, F Ho Wo for the weight gradient."""
    for dims in RC.WGRAD_MAPS:
        dims = RC.dgrad_map(*dims, s)
        case, _, r64 = oracle(g, cg, s, dims)
        Cn, Fr, H, W = case["x"].shape
        _, _, Ho, Wo = case["g"].shape
        buf, geo = haloed(hip, case["x"])
        v = hip.padded2d_halo_view(buf, geo, Cn, Fr, H, W)
        y = torch.empty(Cn, Fr, Ho, Wo, device="cuda")
        hip.conv2d_grouped(v, hip.pack_grouped_conv_weight(dev(case["w"]), g, "f32"), None, hip.dense_volume(y), g, s, False, "f32")
        dw = hip.conv2d_grouped_wgrad(v, dev(case["g"]), g, s)
        dx = hip.conv2d_grouped_dgrad(dev(case["g"]), dev(case["w"]), g, s, "f32")
        d = lambda a: np.asarray(a, np.float64)
        lhs, mid, rhs = float((host(y) * d(case["g"])).sum()), float((d(case["w"]) * host(dw)).sum()), float((d(case["x"]) * host(dx)).sum())
        exact = float((r64["y"] * d(case["g"])).sum())
        ab = dict(x=np.abs(case["x"]), w=np.abs(case["w"]), g=np.abs(case["g"]), groups=g, stride=s)
        S = float((RO.conv_oracle(ab, torch.float64)["y"] * d(ab["g"])).sum())
        u = 2.0 ** -24
        for what, val, terms in (("conv", lhs, 9 * cg), ("wgrad", mid, Fr * Ho * Wo), ("dgrad", rhs, 9 * cg)):
            tol = (terms + 2) * u * S
            print("adjoint (%d, %d) s%d %s %-5s |side - exact| %.3e tol %.3e" % (g, cg, s, dims, what, abs(val - exact), tol))
            assert abs(val - exact) <= tol, (g, cg, s, dims, what)


# ------------------------------------------------------------------------------------------------ one block
def device_block(hip, p, stride, precision, groups, s3):
    """The dict ``encoder_backward.body_stage_forward`` / ``encoder_backward.body_backward`` take for one block with the oracle's parameters p."""
    d = dict(stride=stride, groups=groups, stride_in_3x3=bool(s3 and stride == 2))
    grouped = groups != 1 or d["stride_in_3x3"]
    for n, key, wkey, skey in (("conv1", "conv1", "w1", "s1"), ("conv2", "conv2", "w2", "s2"), ("conv3", "conv3", "w3", "s3"), ("down", "down", "wd", "sd")):
        if n in p:
            w = dev(BO.folded(p, n))
            if n == "conv2" and grouped:
                packed = hip.pack_grouped_conv_weight(w, groups, precision)
            else:
                packed = hip.pack_conv_weight_any(w.reshape(w.shape[0], w.shape[1], 1, w.shape[2], w.shape[3]), precision)
            d[key] = (packed, dev(p[n + ".b"]))
            d[wkey], d[skey] = w, dev(p[n + ".s"])
    return d


def block_weights(blk, s):
    return dict(conv1=blk["w1"], conv2=blk["w2"], conv3=blk["w3"], down=blk.get("wd"), s1=blk["s1"], s2=blk["s2"], s3=blk["s3"], sd=blk.get("sd"),
                groups=blk["groups"], stride_in_3x3="xs2" in s)


def given_of(s):
    buf, g = s["a1"]
    mid, Fr = s["a2"].shape[:2]
    H, W = s["xs"].shape[2:]
    a1 = buf[:mid * g["cs"]].view(mid, Fr, H + 2, g["pitch"])[:, :, 1:H + 1, 1:W + 1]
    return dict(a1=a1.cpu().numpy(), a2=s["a2"].cpu().numpy(), out=s["out"].cpu().numpy())


@pytest.mark.parametrize("precision", ["bf16x6", "f32"])
@pytest.mark.parametrize("kind,Cin,mid,Cout,stride,groups,s3", RC.BLOCKS)
def test_one_block_vs_autograd(hip, kind, Cin, mid, Cout, stride, groups, s3, precision):
    """A grouped stride-1 projection block, a grouped identity block, a grouped and a one-group stride-in-3x3 projection block; F 1 and 3, maps
    1x2, 3x5 and 8x16 after the stride: every dW and g_x by the rule, the oracle on the device's recomputed activations; with want_dx=False no
    g_x and the same dW bits; a second call gives the same bits."""
    bad = []
    for Fr in RC.BLOCK_F:
        for h, w in RC.BLOCK_HW:
            name = "%s %s F %d %dx%d" % (kind, precision, Fr, h, w)
            case = RO.block_case(kind, Cin, mid, Cout, stride, groups, s3, Fr, h, w)
            blk = device_block(hip, case["params"], stride, precision, groups, s3)
            s = EB.body_stage_forward(dev(case["x"]), [blk], precision)[0]
            assert ("xs2" in s) == bool(s3) and tuple(s["out"].shape) == (Cout, Fr, h, w)
            given = given_of(s)
            r32, _ = RO.block_gradients(case, torch.float32, given)
            r64, _ = RO.block_gradients(case, torch.float64, given)
            run = lambda **kw: EB.bottleneck_backward(hip.dense_volume(s["xs"]), s, dev(case["g"]), block_weights(blk, s), precision, **kw)
            got = run()
            assert tuple(got["g_x"].shape) == case["x"].shape if s3 else tuple(got["g_x"].shape) == (Cin, Fr, h, w)
            for n in r64:
                TO.check(name, n, host(got[n]), r32[n], r64[n], bad)
            assert (got["down"] is None) == ("identity" in kind)
            nodx, again = run(want_dx=False), run()
            assert nodx["g_x"] is None
            for n in BO.CONVS:
                if got[n] is not None:
                    assert torch.equal(nodx[n], got[n]) and torch.equal(again[n], got[n]), (name, n)
            assert torch.equal(again["g_x"], got["g_x"])
            if s3:                                            # the addend joins g_x: the same fp32 sum as scatter2's
                a = dev(np.random.default_rng(h + w).standard_normal(case["x"].shape).astype(np.float32))
                joined = run(addend_x=a)["g_x"]
                TO.check(name, "g_x + a", host(joined), r32["g_x"] + host(a), r64["g_x"] + host(a), bad)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the composed body
def device_body(hip, case, precision):
    stages, inputs, given = {}, {}, []
    x = dev(case["x"])
    for k, blocks in enumerate(case["stages"]):
        st = k + 2
        stages[st] = [device_block(hip, p, 2 if b == 0 else 1, precision, case["groups"], case["stride_in_3x3"]) for b, p in enumerate(blocks)]
        inputs[st] = x
        stash = EB.body_stage_forward(x, stages[st], precision)
        given.append([given_of(s) for s in stash])
        x = stash[-1]["out"]
    return stages, inputs, given


@pytest.mark.parametrize("freeze_at", RC.BODY_FREEZE)
@pytest.mark.parametrize("levels", RC.BODY_LEVELS)
@pytest.mark.parametrize("name,groups,s3,stage_spec", RC.BODIES)
def test_body_backward_composed(hip, name, groups, s3, stage_spec, levels, freeze_at):
    """A: groups 4 with the stride in the 3x3 (8, 16, 32 channels per group); B: the same with the stride in the 1x1; C: one group with the stride
    in the 3x3.  Upstream on all three stage outputs and on the last only, freeze_at 2 and 4: every weight gradient from freeze_at on by the rule
    (the FPN's dC of the level below joins inside the stride-in-3x3 block, nothing is scattered twice), a second call gives the same bits."""
    precision = "bf16x6"
    case = RO.body_case(groups, s3, stage_spec, levels)
    stages, inputs, given = device_body(hip, case, precision)
    r32 = RO.body_gradients(case, torch.float32, given, freeze_at - 2)
    r64 = RO.body_gradients(case, torch.float64, given, freeze_at - 2)
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
                    TO.check("body %s levels %s freeze_at %d" % (name, levels, freeze_at), "s%d.b%d.%s" % (st, b, n), host(g[n]), r32[key], r64[key], bad)
                    assert bool(g[n].any()), key
                    if n == "conv2":
                        assert tuple(g[n].shape) == (g[n].shape[0], g[n].shape[0] // groups, 3, 3)
    assert seen == set(r64)
    again = EB.body_backward(inputs, stages, dC, precision, freeze_at)
    assert all(torch.equal(a[n], b[n]) for st in got for a, b in zip(got[st], again[st]) for n in BO.CONVS if a[n] is not None), "reruns differ"
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the recompute
def _resnext_backbone(kind, groups, width, s1x1, seed=11):
    from stemseg_amd.modeling.backbone import ResNetFPN
    from tests import synth
    bb = ResNetFPN(kind, 256, groups, width, s1x1).eval()
    sd = synth.synth_state_dict([(k, v.shape) for k, v in bb.state_dict().items()], seed, prefix="backbone.")
    bb.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(bb.state_dict()[k].shape) for k, v in sd.items()})
    return bb.cuda()


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("tag,kind,groups,width,s1x1", RC.BACKBONES)
def test_recompute_against_the_stage_outputs_of_the_pass(hip, tag, kind, groups, width, s1x1, precision):
    """X50_32x4d and a one-group R-50 with the stride in the 3x3 on 4 x 64 x 96: the last ``out`` of the recompute of stages 2-4 (conv2 on
    ``conv2d_grouped`` with the pass's packing) against the stage outputs the pass left in its workspace: at most 4e-6 of max|Cst[k]|."""
    bb = _resnext_backbone(kind, groups, width, s1x1)
    bb.precision = precision
    bb.train_resnext = True
    x = _frames(*RC.RECOMPUTE_FRAMES)
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
        stash = EB.body_stage_forward(inputs[st], specs[st], precision, int(bb.plan_frames))
        out = stash[-1]["out"]
        assert ("xs2" in stash[0]) == (not s1x1)
        assert out.shape == cst.shape and bool(torch.isfinite(cst).all()) and float(cst.max()) > 0
        d = float((out - cst).abs().max() / cst.abs().max())
        print("recompute %s %s stage %d: max |out - Cst| / max |Cst| = %.3e, equal %s" % (tag, precision, st, d, torch.equal(out, cst)))
        worst = max(worst, d)
    assert worst <= 4e-6, worst


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model(hip):
    """kittimots preset with 4-frame clips, an R-50 of 32 groups x 4 with the stride in the 3x3, synthetic weights, ``configure_trainable``."""
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    from stemseg_amd.training.utils import configure_trainable
    from tests import synth
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        r = config.cfg.MODEL.RESNETS
        r.NUM_GROUPS, r.WIDTH_PER_GROUP, r.STRIDE_IN_1X1 = 32, 4, False
        config.cfg.INPUT.NUM_FRAMES = 4                          # (the decoders' temporal pooling is fixed at construction)
        m = build_model()
        sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], 11)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()})
        m = m.cuda().eval()
        configure_trainable(m, config.cfg, freeze_backbone=False)
        m.image_mean = torch.tensor(config.cfg.INPUT.IMAGE_MEAN)
        m.initial_state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        yield m
    finally:
        config.load_preset("defaults")


def test_training_model_end_to_end(hip, model):
    """One clip of 4 x 64 x 96 in bf16x6: finite gradients on exactly the body (layer2 .. layer4), FPN and decoder parameters and none on the stem
    or layer1; the body's meet the rule; a second pass gives the same bits; one DeviceSGD step re-packs the body and moves the no-grad output;
    with ``train_resnext`` off the same call raises the existing message."""
    from stemseg_amd.training.optim import DeviceSGD
    from stemseg_amd.utils.constants import ModelOutput
    m, bb = model, model.backbone
    precision = "bf16x6"
    assert m.train_resnext and bb.train_resnext and m.train_body and m.train_fpn and m.train_decoders
    _prepare(m, precision)
    frames, raw = _inputs(m, 4, 64, 96)
    with torch.no_grad():
        before = m(frames, raw())[ModelOutput.INFERENCE][ModelOutput.EMBEDDINGS].clone()
    maps, freeze_at, loss = _train_pass(m, frames, raw)
    assert freeze_at == 2
    named = dict(m.named_parameters())
    body, fpn, dec = m.body_parameters(2), m.fpn_parameters(), m.decoder_parameters()
    assert len(body) == 42 and len(fpn) == 16
    filled = {k for k, p in named.items() if p.grad is not None}
    assert filled == set(body) | set(fpn) | set(dec), sorted(filled ^ (set(body) | set(fpn) | set(dec)))
    assert not any(k.startswith("backbone.body.stem.") or k.startswith("backbone.body.layer1.") for k in filled)
    assert all(bool(torch.isfinite(named[k].grad).all()) for k in filled) and all(bool(named[k].grad.any()) for k in body)
    assert tuple(named["backbone.body.layer2.0.conv2.weight"].grad.shape) == (256, 8, 3, 3)
    # (the oracle of tests/test_gpu_body_backward.py builds its blocks with BO.body_forward: one group, the stride in the 1x1 -- here the
    # ResNeXt block forward stands in for it)
    saved = BO.block_forward, TB.given_of
    BO.block_forward = lambda x, live, stride, dtype, given=None: RO.block_forward(x, live, stride, dtype, given, 32, True)
    TB.given_of = given_of                                   # (a1 of a stride-in-3x3 block lies at the stage input's resolution)
    try:
        bad = _check_body_gradients(hip, m, "end to end resnext %s" % precision, frames, maps, 2)
    finally:
        BO.block_forward, TB.given_of = saved
    first = {k: named[k].grad.clone() for k in filled}
    _, _, loss2 = _train_pass(m, frames, raw)
    assert torch.equal(loss, loss2) and all(torch.equal(named[k].grad, first[k]) for k in filled), "reruns differ"
    w, names_before = bb._packed[precision][1][0], bb._packed_names[precision]
    opt = DeviceSGD([named[k] for k in sorted(filled)], lr=1e-3)
    opt.step()
    with torch.no_grad():
        after = m(frames, raw())[ModelOutput.INFERENCE][ModelOutput.EMBEDDINGS]
    assert not torch.equal(after, before)
    assert bb._packed[precision][1][0] is not w and bb._packed_names[precision] is not names_before, "the step did not re-pack the body"
    m.train_resnext = False
    try:
        with pytest.raises(NotImplementedError) as e:
            m(frames, raw())
        assert str(e.value) == "MODEL.RESNETS.NUM_GROUPS=32: the body's backward has no grouped-convolution backward (NUM_GROUPS=1 only)"
    finally:
        m.train_resnext = True
    assert not bad, bad
