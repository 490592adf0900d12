"""GPU tests of the stem backward (csrc/stem_backward.hip; hip.maxpool3x3s2_backward / stem_wgrad; ResNetFPN.stem_forward;
encoder_backward.stem_backward / body_backward at freeze_at 0 and 1; modeling.ops.EncoderFunction; TrainingModel.train_stem) against
torch-CPU autograd (tests/stem_backward_oracle.py).

The max-pool backward is checked bit for bit against torch's CPU backward.  Gradients, per case (the rule of tests/test_gpu_decoder_tail.py):
the oracle runs in fp32 and in fp64 on the case's own input, taking the device's recomputed activations as given values; the device may be
FACTOR = 4 x that spread, floored at 2^-24, away from the fp64 result, on the max norm relative to max|g|.  Every case prints its spread,
bound and device error before the test asserts; the table is in DESIGN.md section 9v."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from stemseg_amd.modeling import encoder_backward as EB
from tests import body_backward_oracle as BO
from tests import decoder_tail_oracle as TO
from tests import fpn_backward_oracle as FO
from tests import stem_backward_cases as SC
from tests import stem_backward_oracle as SO

pytestmark = pytest.mark.gpu
bits = SO.bits


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def guarded(n, lead=64):
    """-> (a NaN-filled buffer with ``lead`` floats before and after n, the view of the n floats; the view stays 16-byte aligned)."""
    buf = torch.full((n + 2 * lead,), float("nan"), dtype=torch.float32, device="cuda")
    return buf, buf[lead:lead + n]


def guards_intact(buf, n, lead=64):
    return bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + n:]).all())


# ------------------------------------------------------------------------------------------------ the max-pool backward
@pytest.mark.parametrize("planes,H,W", SC.POOL_CASES)
def test_maxpool_backward_is_torchs_cpu_backward(hip, planes, H, W):
    """2x2, 4x6, 6x10 (odd Ho), 34x70 and 64x128 with 1-5 planes, and 2x4, 6x8, 10x12 (the 16-byte form's edges): both forms where the 16-byte one applies, with and without the ReLU mask, on
    post-ReLU maps of halves with zero and positive ties, +-0.0, denormals, inf and NaN (two in one window), g with zeros; the output in a
    NaN-filled guarded buffer; bit-equal to torch's CPU backward; two runs the same bits; a forced 16-byte form where W % 4 != 0 is refused."""
    x, g = SC.pool_input(planes, H, W), SC.pool_upstream(planes, H, W)
    xd, gd = dev(x), dev(g)
    forms = [hip.STREAM_FORM_SCALAR] + ([hip.STREAM_FORM_VEC4] if W % 4 == 0 else [])
    for mask in (False, True):
        want = SO.pool_backward_torch(x, g, mask)
        for form in forms + [0]:
            buf, view = guarded(planes * H * W)
            out, used = hip.maxpool3x3s2_backward(xd, gd, mask, out=view.view(planes, H, W), form=form)
            assert used == (form or forms[-1])
            assert torch.equal(bits(out), bits(want)), (mask, form)
            assert guards_intact(buf, planes * H * W), (mask, form)
            again, _ = hip.maxpool3x3s2_backward(xd, gd, mask, form=form)
            assert torch.equal(bits(again), bits(out)), (mask, form, "reruns differ")
    if W % 4:
        with pytest.raises(RuntimeError, match="the 16-byte form needs W % 4 == 0"):
            hip.maxpool3x3s2_backward(xd, gd, form=hip.STREAM_FORM_VEC4)
    else:                                                    # an output that is only 4-byte aligned takes the scalar form
        buf, _ = guarded(planes * H * W, lead=65)
        out, used = hip.maxpool3x3s2_backward(xd, gd, True, out=buf[65:65 + planes * H * W].view(planes, H, W))
        assert used == hip.STREAM_FORM_SCALAR and torch.equal(bits(out), bits(SO.pool_backward_torch(x, g, True)))


# ------------------------------------------------------------------------------------------------ the stem's weight gradient
def _wgrad_guarded(hip, frames, g):
    """stem_wgrad with a NaN frame behind frame F - 1, NaN bands around g, and dw written into a NaN-filled guarded buffer -> dw."""
    Fr, _, H, W = frames.shape
    fb = torch.full((Fr + 1, 3, H, W), float("nan"), dtype=torch.float32, device="cuda")
    fb[:Fr] = dev(frames)
    gbuf, gview = guarded(g.size)
    gview.copy_(dev(g).reshape(-1))
    wbuf, wview = guarded(64 * 147)
    dw = hip.stem_wgrad(fb[:Fr], gview.view(g.shape), out=wview.view(64, 3, 7, 7))
    assert dw.data_ptr() == wview.data_ptr() and guards_intact(wbuf, 64 * 147)
    assert bool(torch.isnan(fb[Fr]).all()) and guards_intact(gbuf, g.size)
    return dw.clone()


@pytest.mark.parametrize("Fr,H,W", SC.WGRAD_CASES)
def test_stem_wgrad_vs_autograd(hip, Fr, H, W):
    """F = 1, 2, 3 on 8x8, 14x22 (Ho = 7, Wo = 11: ragged tiles), 64x96, and the several-chunk case with its ragged last chunk: dw by the rule
    against ``F.conv2d(stride=2, padding=3)`` autograd; nothing of a NaN frame behind the last one or of the NaN bands around g leaks; two
    runs give the same bits; the adjoint identity <g, conv(frames; w)> = <dw, w> within the rule."""
    frames, g = SC.wgrad_case(Fr, H, W)
    name = "stem_wgrad F %d %dx%d (%d chunks)" % (Fr, H, W, hip.stem_wgrad_chunks(Fr, H, W))
    r32, r64 = SO.wgrad_oracle(frames, g, torch.float32), SO.wgrad_oracle(frames, g, torch.float64)
    dw = _wgrad_guarded(hip, frames, g)
    assert dw.shape == (64, 3, 7, 7) and bool(torch.isfinite(dw).all())
    bad = []
    TO.check(name, "dw", host(dw), r32, r64, bad)
    assert torch.equal(bits(_wgrad_guarded(hip, frames, g)), bits(dw)), "reruns differ"
    # <g, conv(frames; w)> = <dw, w>: both sides in fp64 from the fp32 data, the left by the oracle's convolution
    w = np.random.default_rng(5).standard_normal((64, 3, 7, 7)).astype(np.float32)
    conv = torch.nn.functional.conv2d(torch.from_numpy(frames).double(), torch.from_numpy(w).double(), stride=2, padding=3).permute(1, 0, 2, 3)
    lhs = float((conv * torch.from_numpy(g).double()).sum())
    lhs32 = float((r32 * w.astype(np.float64)).sum())
    rhs = float((host(dw) * w.astype(np.float64)).sum())
    scale = float(np.abs(r64 * w).sum())
    spread = abs(lhs32 - lhs) / scale
    print("%s adjoint: lhs %.9e rhs %.9e spread %.2e device %.2e" % (name, lhs, rhs, spread, abs(rhs - lhs) / scale))
    assert abs(rhs - lhs) / scale <= TO.FACTOR * max(spread, TO.FP32_ROUNDING)
    assert not bad, bad


@pytest.mark.parametrize("Fr,H,W", [(1, 8, 8), (3, 14, 22), (2, 64, 96), SC.WGRAD_SEVERAL])
def test_stem_wgrad_one_hot_is_the_patch(hip, Fr, H, W):
    """A one-hot upstream (value 1) at the four corners, at the last pixel of the last frame and inside: dw[co] is the frames' 7x7 patch bit for
    bit -- zero padding on the sides that leave the frame -- and every other channel exactly zero."""
    frames, _ = SC.wgrad_case(Fr, H, W)
    Ho, Wo = H // 2, W // 2
    spots = [(0, 0, 0), (0, 0, Wo - 1), (Fr - 1, Ho - 1, 0), (Fr - 1, Ho - 1, Wo - 1), (Fr // 2, Ho // 2, Wo // 2)]
    fd = dev(frames)
    for i, (f, oy, ox) in enumerate(spots):
        co = (17 * i + 3) % 64
        g = np.zeros((64, Fr, Ho, Wo), np.float32)
        g[co, f, oy, ox] = 1.0
        dw = hip.stem_wgrad(fd, dev(g)).cpu()
        assert torch.equal(bits(dw[co]), bits(SO.stem_patch(frames, f, oy, ox))), (f, oy, ox)
        dw[co] = 0
        assert not bool(dw.any()), (f, oy, ox)


# ------------------------------------------------------------------------------------------------ the recompute
def _frames(T, H, W, seed=3):
    from tests import synth
    mean = torch.tensor([102.9801, 115.9465, 122.7717])[None, :, None, None]
    return (torch.from_numpy(synth.synth_frames(T, H, W, seed=seed).astype(np.float32)).permute(0, 3, 1, 2) - mean).cuda()


def _slice(ws, off, shape):
    return ws[off:off + int(np.prod(shape))].view(shape)


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6", "f32"])
def test_stem_forward_recomputes_the_pass(hip, precision):
    """R-50 on 8 x 96 x 128.  Where no stage-end tail re-uses the slices (``encoder_stage_end_mask``; never in bf16x6 and f32) the pass's own
    stem map S0 and pooled map X1 are still in its workspace: the recompute is bit-equal.  In every precision layer1 recomputed from the
    recomputed pooled map lies within 4e-6 of max|Cst[0]| of the pass's stage output, the figure of
    ``test_recompute_against_the_stage_outputs_of_the_pass``; a second recompute gives the same bits and the pass's maps are untouched."""
    from tests.fused_tail_util import backbone
    bb, _ = backbone("R-50-FPN", 11)
    bb.precision = precision
    x = _frames(8, 96, 128)
    maps = [o.clone() for o in bb.forward_channel_major(x)]
    key = bb.workspace_key(x)
    offs = (C.c_int64 * 25)()
    hip.check(hip.lib().stemseg_hip_encoder_plan_offsets(C.byref(bb._ws_desc[key]), offs))
    mask = C.c_int32(0)
    hip.check(hip.lib().stemseg_hip_encoder_stage_end_mask(C.byref(bb._ws_desc[key]), C.byref(mask)))
    ws = bb._ws[key].view(torch.float32)
    stem, pooled = bb.stem_forward(x)
    assert stem.shape == (64, 8, 48, 64) and pooled.shape == (64, 8, 24, 32)
    if precision != "f16x3":
        assert mask.value == 0
    if not mask.value & 1:
        assert torch.equal(bits(stem), bits(_slice(ws, offs[0], stem.shape))), "S0"
    if not mask.value & 2:
        assert torch.equal(bits(pooled), bits(_slice(ws, offs[1], pooled.shape))), "X1"
    assert torch.equal(bits(pooled), bits(hip.maxpool3x3s2(stem.view(64 * 8, 48, 64))[0].view(pooled.shape)))
    assert bool((stem >= 0).all()) and float(stem.max()) > 0
    specs = bb.body_stage_specs(1, bb._packed_names[precision])
    assert sorted(specs) == [1, 2, 3, 4] and len(specs[1]) == 3 and specs[1][0]["stride"] == 1 and "down" in specs[1][0]
    out = EB.body_stage_forward(pooled, specs[1], precision, int(bb.plan_frames))[-1]["out"]
    cst = _slice(ws, offs[4], out.shape)
    d = float((out - cst).abs().max() / cst.abs().max())
    print("stem recompute %s: stage-end mask %d, layer1 max |out - Cst| / max |Cst| = %.3e, equal %s" % (precision, mask.value, d, torch.equal(out, cst)))
    assert d <= 4e-6, d
    bb.train_stem = True
    inputs = bb.body_stage_inputs(key, 0, x)
    assert sorted(inputs) == [0, 1, 2, 3, 4] and torch.equal(bits(inputs[0]), bits(stem)) and torch.equal(bits(inputs[1]), bits(pooled))
    assert bb._ws_passes[key] == 1 and all(torch.equal(a, b) for a, b in zip(maps, bb.forward_channel_major(x)))


def test_stem_forward_follows_the_pass_of_a_backbone_that_changed_precision(hip):
    """ONE backbone, one shape, a pass in bf16x6 and then one in f16x3 on the same workspace (its key holds no precision).  The recompute
    after the second pass is the f16x3 pass's -- bit-equal to the S0 and X1 that pass left (no stage-end tail re-uses them at this size) and
    not the bf16x6 maps --, by the backbone's current precision and by the precision a backward hands in after the backbone has moved on;
    the workspace's descriptor is the last pass's."""
    from tests.fused_tail_util import backbone
    bb, _ = backbone("R-50-FPN", 11)
    x = _frames(8, 96, 128)
    key = bb.workspace_key(x)
    offs = (C.c_int64 * 25)()
    seen = {}
    for precision in ("bf16x6", "f16x3"):
        bb.precision = precision
        bb.forward_channel_major(x)
        assert bb._ws_desc[key].precision == hip.PRECISIONS[precision]
        mask = C.c_int32(-1)
        hip.check(hip.lib().stemseg_hip_encoder_stage_end_mask(C.byref(bb._ws_desc[key]), C.byref(mask)))
        assert mask.value == 0
        hip.check(hip.lib().stemseg_hip_encoder_plan_offsets(C.byref(bb._ws_desc[key]), offs))
        ws = bb._ws[key].view(torch.float32)
        stem, pooled = bb.stem_forward(x)
        assert torch.equal(bits(stem), bits(_slice(ws, offs[0], stem.shape))), (precision, "S0")
        assert torch.equal(bits(pooled), bits(_slice(ws, offs[1], pooled.shape))), (precision, "X1")
        seen[precision] = (stem, pooled)
    assert len(bb._ws) == 1 and not torch.equal(seen["bf16x6"][0], seen["f16x3"][0])          # (the two paths do differ: the test can see a mix-up)
    bb.precision = "bf16x6"                                  # the backbone moves on; a backward of the f16x3 pass hands in its own precision
    stem, pooled = bb.stem_forward(x, "f16x3")
    assert torch.equal(bits(stem), bits(seen["f16x3"][0])) and torch.equal(bits(pooled), bits(seen["f16x3"][1]))
    inputs = bb.body_stage_inputs(key, 0, x, "f16x3")
    assert torch.equal(bits(inputs[0]), bits(seen["f16x3"][0])) and torch.equal(bits(inputs[1]), bits(seen["f16x3"][1]))
    with pytest.raises(ValueError, match="stem_forward: precision 'fp8'"):
        bb.stem_forward(x, "fp8")


# ------------------------------------------------------------------------------------------------ the composed stem + body
def device_block(hip, p, stride, precision, groups=1):
    d = dict(stride=stride, groups=groups, stride_in_3x3=False)
    for n, key, wkey, skey in (("conv1", "conv1", "w1", "s1"), ("conv2", "conv2", "w2", "s2"), ("conv3", "conv3", "w3", "s3"), ("down", "down", "wd", "sd")):
        if n in p:
            w = dev(BO.folded(p, n))
            if n == "conv2" and groups != 1:
                packed = hip.pack_grouped_conv_weight(w, groups, precision)
            else:
                packed = hip.pack_conv_weight_any(w.reshape(w.shape[0], w.shape[1], 1, w.shape[2], w.shape[3]), precision)
            d[key] = (packed, dev(p[n + ".b"]))
            d[wkey], d[skey] = w, dev(p[n + ".s"])
    return d


def given_of(s):
    buf, g = s["a1"]
    mid, Fr, h, w = s["a2"].shape
    a1 = buf[:mid * g["cs"]].view(mid, Fr, h + 2, g["pitch"])[:, :, 1:h + 1, 1:w + 1]
    return dict(a1=a1.cpu().numpy(), a2=s["a2"].cpu().numpy(), out=s["out"].cpu().numpy())


def device_stem_body(hip, case, precision):
    """The device's stem (the exact fp32-MFMA stem on the folded weight), max-pool and stages of ``case`` -> (stages, stage inputs, the stem's
    map, per stage per block the device's activations)."""
    st = case["stem"]
    frames = dev(case["frames"])
    stem = hip.stem_conv(frames, dev(st["w"] * st["s"][:, None, None, None]), dev(st["b"]))
    Fr = frames.shape[0]
    pooled = hip.maxpool3x3s2(stem.view(64 * Fr, *stem.shape[2:]))[0].view(64, Fr, stem.shape[2] // 2, stem.shape[3] // 2)
    stages, inputs, given = {}, {}, []
    x = pooled
    for k, blocks in enumerate(case["stages"]):
        stages[k + 1] = [device_block(hip, p, 2 if (b == 0 and k > 0) else 1, precision, case["groups"]) for b, p in enumerate(blocks)]
        inputs[k + 1] = x
        stash = EB.body_stage_forward(x, stages[k + 1], precision)
        given.append([given_of(s) for s in stash])
        x = stash[-1]["out"]
    return stages, inputs, stem, given


@functools.lru_cache(maxsize=None)
def _composed(groups):
    """The case, the device's forward and both oracle runs at freeze_at 0 (freeze_at 1 is the same without the stem's entry): computed once."""
    from stemseg_amd import hip
    case = SC.stem_body_case(groups=groups, stages=SC.STEM_STAGES if groups == 1 else SC.RESNEXT_STAGES)
    stages, inputs, stem, given = device_stem_body(hip, case, "bf16x6")
    gs = stem.cpu().numpy()
    refs = [SO.stem_body_gradients(case, dt, gs, given, 0) for dt in (torch.float32, torch.float64)]
    return case, stages, inputs, stem, refs


def _check_composed(hip, name, case, stages, inputs, stem, refs, freeze_at):
    n_st = len(case["stages"])
    dC = {k + 1: dev(case["g"][k]) for k in range(n_st)}
    args = dict(frames=dev(case["frames"]), stem_map=stem, bn_scale=dev(case["stem"]["s"]))
    run = lambda: EB.body_backward(dict(inputs), stages, dC, "bf16x6", freeze_at, stem=args)
    got = run()
    bad, seen = [], set()
    assert sorted(got) == list(range(freeze_at, n_st + 1))
    if freeze_at == 0:
        TO.check(name, "stem", host(got[0]), refs[0]["stem"], refs[1]["stem"], bad)
        assert bool(got[0].any())
        seen.add("stem")
    for st in range(1, n_st + 1):
        for b, g in enumerate(got[st]):
            for n in BO.CONVS:
                if g[n] is not None:
                    key = (st - 1, b, n)
                    seen.add(key)
                    TO.check(name, "s%d.b%d.%s" % (st, b, n), host(g[n]), refs[0][key], refs[1][key], bad)
                    assert bool(g[n].any()), key
    assert seen == set(refs[1]) - (set() if freeze_at == 0 else {"stem"})
    again = run()
    assert all(torch.equal(a[n], b[n]) for st in range(1, n_st + 1) for a, b in zip(got[st], again[st]) for n in BO.CONVS if a[n] is not None), "reruns differ"
    assert freeze_at or torch.equal(got[0], again[0])
    return bad


@pytest.mark.parametrize("freeze_at", [0, 1])
def test_body_backward_composed_with_the_stem(hip, freeze_at):
    """An R-50's widths, two blocks a stage, F = 2, 32 x 64 frames: the stem's map 16 x 32, layer1 (a stride-1 projection block first) on 8 x 16,
    then 4 x 8, 2 x 4, 1 x 2; an upstream on every stage output.  freeze_at 0: the stem's dw and every weight gradient of layer1 .. layer4 by
    the rule, the oracle linearised around the device's activations (the ReLU masks and the pool's arg-max positions are the device's);
    freeze_at 1: the same without the stem's, and layer1's first block computes no data gradient.  Reruns give the same bits."""
    case, stages, inputs, stem, refs = _composed(1)
    bad = _check_composed(hip, "stem + body freeze_at %d" % freeze_at, case, stages, inputs, stem, refs, freeze_at)
    with pytest.raises(NotImplementedError, match="MODEL.BACKBONE.FREEZE_AT_STAGE"):
        EB.body_backward(dict(inputs), stages, {}, "bf16x6", freeze_at)
    if freeze_at == 0:
        with pytest.raises(ValueError, match=r"freeze_at 0 needs stem\['stem_map'\]"):
            EB.body_backward(dict(inputs), stages, {k + 1: dev(g) for k, g in enumerate(case["g"])}, "bf16x6", 0, stem=dict(frames=dev(case["frames"])))
    assert not bad, bad


@pytest.mark.parametrize("freeze_at", [0, 1])
def test_resnext_layer1_block_route_with_the_stem(hip, freeze_at):
    """A ResNeXt 32x4d's widths, two blocks a stage: layer1 is 64 -> 128 in 32 groups of 4 -> 256 at stride 1, and its grouped conv2 goes through
    ``conv2d_grouped_wgrad`` / ``conv2d_grouped_dgrad``; the gradient of the pooled map goes on through the max-pool into the stem's dw.  By
    the rule, as the plain case."""
    case, stages, inputs, stem, refs = _composed(32)
    assert case["stages"][0][0]["conv2"].shape == (128, 4, 3, 3) and stages[1][0]["groups"] == 32
    bad = _check_composed(hip, "resnext layer1 freeze_at %d" % freeze_at, case, stages, inputs, stem, refs, freeze_at)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def model(hip):
    """kittimots preset, R-50, synthetic weights, the four switches on."""
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
        m.train_decoders = m.train_fpn = m.train_body = m.train_stem = True
        m.initial_state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        yield m
    finally:
        config.load_preset("defaults")


def _prepare(m, precision, freeze_at):
    m.load_state_dict(m.initial_state)
    for mod in (m.backbone, m.embedding_head, m.seediness_head, m.semseg_head):
        if mod is not None:
            mod.precision = precision
    for k, p in m.named_parameters():
        frozen = (k.startswith("backbone.body.stem.") and freeze_at >= 1) or any(k.startswith("backbone.body.layer%d." % st) for st in range(1, freeze_at))
        p.requires_grad_(not frozen)
        p.grad = None


def _inputs(T, H, W):
    from tests import semseg_loss_oracle as SLO
    frames = _frames(T, H, W)[None]
    sample = SLO.make_sample(np.random.default_rng(5), 1, T, H, W, (1, 2, 2))[1:]
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


def _check_stem_and_layer1(hip, m, name, frames, maps, freeze_at):
    """The stem's and layer1's gradients by the rule.  The oracle is the stem and the body linearised around the device's recomputed activations
    (stages 2 .. 4 start from the stage outputs the pass left, as the device's recompute does), fed into the FPN oracle on the stage outputs
    and merged laterals of the pass; its upstream is the device's own dP_k."""
    bb = m.backbone
    x = frames.reshape((-1,) + tuple(frames.shape[-3:]))
    key = bb.workspace_key(x)
    c_views, l_views, _ = bb.fpn_workspace_views(key)
    ws = bb._ws[key].view(torch.float32)
    off = lambda v: (v.ptr - ws.data_ptr()) // 4
    Cs = [ws[off(v):off(v) + v.C * v.T * v.H * v.W].view(v.C, v.T, v.H, v.W).clone().cpu() for v in c_views]
    Ls = [ws[off(v):off(v) + v.C * v.c_stride].view(v.C, v.T, v.H, v.y_stride)[:, :, 1:v.H - 1, 1:v.W - 1].clone().cpu() for v in l_views]
    specs = bb.body_stage_specs(freeze_at, bb._packed_names[bb.precision])
    inputs = bb.body_stage_inputs(key, freeze_at, x)
    given = [[given_of(s) for s in EB.body_stage_forward(inputs[st], specs[st], bb.precision, int(bb.plan_frames))] for st in range(1, 5)]
    stem_dev = inputs[0].cpu().numpy()
    ups = [o.grad.permute(1, 0, 2, 3).detach().cpu() for o in maps]
    fpn = {n: p.detach().cpu().numpy() for n, p in bb.fpn.named_parameters()}
    s0, b0 = bb.body.stem.bn1.scale_shift()
    refs = []
    for dt in (torch.float32, torch.float64):
        live = []
        for st in range(1, 5):
            live.append([])
            for blk in getattr(bb.body, "layer%d" % st):
                p = {}
                for n, conv, bn in (("conv1", blk.conv1, blk.bn1), ("conv2", blk.conv2, blk.bn2), ("conv3", blk.conv3, blk.bn3)) + (
                        (("down", blk.downsample[0], blk.downsample[1]),) if blk.downsample is not None else ()):
                    s, b = bn.scale_shift()
                    p[n], p[n + ".s"], p[n + ".b"] = conv.weight.detach().cpu().numpy(), s.detach().cpu().numpy(), b.detach().cpu().numpy()
                live[-1].append(BO.live_params(p, dt))
        stem = dict(w=bb.body.stem.conv1.weight.detach().cpu().to(dt).requires_grad_(True), s=s0.detach().cpu().to(dt), b=b0.detach().cpu().to(dt))
        _, pooled = SO.stem_forward(x.cpu().to(dt), stem, dt, stem_dev)
        outs = SO.body_forward(pooled, live, dt, given, stage_in=[None] + [Cs[st - 2] for st in range(2, 5)])
        C_or = []
        for k, o in enumerate(outs):
            o = BO.frames_first(o)
            C_or.append(o + (Cs[k].to(dt) - o).detach())                    # the FPN reads the pass's stage output
        _, Ps = FO.fpn_forward(C_or, fpn, dt, Ls)
        sum((P * u.to(dt)).sum() for P, u in zip(Ps, ups)).backward()
        g = {"backbone.body.stem.conv1.weight": stem["w"].grad.double().numpy()} if freeze_at == 0 else {}
        for b, lp in enumerate(live[0]):
            for n in BO.CONVS:
                if n in lp:
                    g["backbone.body.layer1.%d.%s.weight" % (b, "downsample.0" if n == "down" else n)] = lp[n].grad.double().numpy()
        refs.append(g)
    named = dict(m.named_parameters())
    bad = []
    assert len(refs[1]) == 10 + (freeze_at == 0)
    for n in refs[1]:
        TO.check(name, n[len("backbone.body."):], host(named[n].grad), refs[0][n], refs[1][n], bad)
    return bad


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"])
def test_training_model_end_to_end_with_the_stem(hip, model, precision):
    """One clip of 8 x 96 x 128, the four switches on, everything trainable (FREEZE_AT_STAGE 0).  The four maps are the bits of the no-grad
    ``run_backbone``; the summed losses' backward fills finite, non-zero gradients on exactly the stem's weight, layer1's 10, the 42 of
    layer2 .. layer4, the 16 FPN and the 67 decoder parameters; the stem's and layer1's meet the rule; a second pass gives the same bits; one
    DeviceSGD step (lr 1e-3) re-packs the stem -- the space-to-depth packing of f16x3 included -- and layer1, and moves the no-grad output."""
    from stemseg_amd.training.optim import DeviceSGD
    from stemseg_amd.utils.constants import ModelOutput
    m, bb = model, model.backbone
    _prepare(m, precision, 0)
    frames, raw = _inputs(8, 96, 128)
    with torch.no_grad():
        ref = [v.clone() for v in m.run_backbone(frames).values()]
        before = m(frames, raw())[ModelOutput.INFERENCE][ModelOutput.EMBEDDINGS].clone()
    assert m.body_freeze_at() == 0
    maps, freeze_at, loss = _train_pass(m, frames, raw)
    assert freeze_at == 0 and all(a.requires_grad and torch.equal(a, b) for a, b in zip(maps, ref))
    named = dict(m.named_parameters())
    body, fpn, dec = m.body_parameters(0), m.fpn_parameters(), m.decoder_parameters()
    assert (len(body), len(fpn), len(dec)) == (1 + 10 + 42, 16, 67)
    filled = {k for k, p in named.items() if p.grad is not None}
    assert filled == set(body) | set(fpn) | set(dec), sorted(filled ^ (set(body) | set(fpn) | set(dec)))
    assert all(bool(torch.isfinite(named[k].grad).all()) for k in filled)
    assert not [k for k in sorted(filled) if not bool(named[k].grad.any())], "gradients that are all zero"
    bad = _check_stem_and_layer1(hip, m, "end to end %s" % precision, frames, maps, 0)
    first = {k: named[k].grad.clone() for k in filled}
    _, _, loss2 = _train_pass(m, frames, raw)
    assert torch.equal(loss, loss2) and all(torch.equal(named[k].grad, first[k]) for k in filled), "reruns differ"
    w_before, names_before = bb._packed[precision][1][0], bb._packed_names[precision]
    stem_ptrs = (w_before.stem_w, w_before.stem_w_s2d)
    assert bool(stem_ptrs[1]) == (precision == "f16x3")
    l1_before = names_before["b0.conv1"][2].clone()
    kept = lambda w_, address: next(t for t in bb._packed[precision][1][1] if t.data_ptr() == address)
    s2d_before = kept(w_before, w_before.stem_w_s2d).clone() if precision == "f16x3" else None
    DeviceSGD([named[k] for k in sorted(filled)], lr=1e-3).step()
    with torch.no_grad():
        after = m(frames, raw())[ModelOutput.INFERENCE][ModelOutput.EMBEDDINGS]
    w_after = bb._packed[precision][1][0]
    assert not torch.equal(after, before)
    assert w_after is not w_before and bb._packed_names[precision] is not names_before, "the step did not re-pack the body"
    assert bb._packed[precision][0][0][0] == bb._signature_of(bb.body)
    assert bool(w_after.stem_w) and bool(w_after.stem_w_s2d) == (precision == "f16x3")
    assert not torch.equal(bb._packed_names[precision]["b0.conv1"][2], l1_before), "layer1's folded weight did not move"
    stem_now = bb.folded_state()["stem"][0].cuda().reshape(64, 147).t().contiguous()
    assert torch.equal(kept(w_after, w_after.stem_w), stem_now), "the packed stem is not the stepped weight"
    if precision == "f16x3":                                 # ... and the space-to-depth packing the f16x3 pass reads (ResNetFPN._pack's formula)
        w8 = torch.zeros(64, 3, 8, 8, dtype=torch.float32, device="cuda")
        w8[:, :, 1:, 1:] = bb.folded_state()["stem"][0].cuda().reshape(64, 3, 7, 7)
        w2 = w8.reshape(64, 3, 4, 2, 4, 2).permute(0, 3, 5, 1, 2, 4).reshape(64, 12, 1, 4, 4).contiguous()
        s2d_now = kept(w_after, w_after.stem_w_s2d)
        assert torch.equal(s2d_now, hip.pack_conv_weight_any(w2, "f16x3")), "stem_w_s2d is not the packing of the stepped weight"
        assert s2d_now.shape == s2d_before.shape and not torch.equal(s2d_now, s2d_before), "stem_w_s2d did not move"
    assert not bad, bad


def test_freeze_at_1_leaves_the_stem_without_a_gradient(hip, model):
    """The stem frozen, layer1 trainable: the pass runs with freeze_at = 1, layer1's 10 weights and the 42 above get a gradient, the stem's
    none, and layer1's meet the rule."""
    m = model
    _prepare(m, "f16x3", 1)
    frames, raw = _inputs(8, 96, 128)
    maps, freeze_at, _ = _train_pass(m, frames, raw)
    assert freeze_at == 1
    filled = {k for k, p in m.named_parameters() if p.grad is not None and k.startswith("backbone.body.")}
    assert filled == set(m.body_parameters(1)) and len(filled) == 52 and m.backbone.body.stem.conv1.weight.grad is None
    bad = _check_stem_and_layer1(hip, m, "freeze_at 1", frames, maps, 1)
    assert not bad, bad


def test_switch_off_refuses_as_before(hip, model):
    """The same model with ``train_stem`` off: a trainable stem or layer1 raises the NotImplementedError it always raised."""
    m = model
    _prepare(m, "f16x3", 0)
    frames, raw = _inputs(8, 64, 64)
    m.train_stem = False
    try:
        with pytest.raises(NotImplementedError) as e:
            m(frames, raw())
        assert str(e.value) == ("TrainingModel.forward with train_decoders, train_fpn and train_body: the backward pass of the stem, the max-pool and "
                                "layer1 is not implemented (MODEL.BACKBONE.FREEZE_AT_STAGE >= 2), and 11 parameters there require a gradient "
                                "(backbone.body.stem.conv1.weight, ...); freeze them (requires_grad_(False) on backbone.body.stem and "
                                "backbone.body.layer1)")
        with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE=0"):
            m.backbone.forward_trainable_body(frames[0], 0)
    finally:
        m.train_stem = True


def test_resnext_backbone_trains_from_the_stem(hip):
    """A ResNeXt-50 32x4d with ``train_resnext`` and ``train_stem``: ``forward_trainable_body(x, 0)`` on 2 x 64 x 64 gives the bits of the plain
    pass, and the backward fills finite, non-zero gradients on the stem's weight, layer1's grouped blocks and everything above; a second pass
    gives the same bits."""
    from stemseg_amd.modeling.backbone import ResNetFPN
    from tests import synth
    bb = ResNetFPN("R-50-FPN", num_groups=32, width_per_group=4).eval()
    sd = synth.synth_state_dict([(k, v.shape) for k, v in bb.state_dict().items()], 11, prefix="backbone.")
    bb.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(bb.state_dict()[k].shape) for k, v in sd.items()})
    bb = bb.cuda()
    bb.train_resnext = bb.train_stem = True
    x = _frames(2, 64, 64)
    ref = bb.forward(x)
    ups = [torch.from_numpy(np.random.default_rng(k).standard_normal(tuple(r.shape)).astype(np.float32)).cuda() for k, r in enumerate(ref)]
    params = bb.body_parameter_list(0)
    assert len(params) == 53 and params[3].shape == (128, 4, 3, 3)
    grads = []
    for _ in range(2):
        for p in bb.parameters():
            p.grad = None
        outs = bb.forward_trainable_body(x, 0)
        assert all(torch.equal(a, b) for a, b in zip(outs, ref))
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        grads.append([p.grad.clone() for p in params])
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads[0])
    assert all(torch.equal(a, b) for a, b in zip(*grads)), "reruns differ"
