"""ResNeXt / stride-in-3x3 backbones on the MI355X: the grouped 3x3 convolution (csrc/grouped_conv.hip, stemseg_hip_conv2d_grouped) in
every precision against an fp64 convolution, the encoder with MODEL.RESNETS.NUM_GROUPS / WIDTH_PER_GROUP / STRIDE_IN_1X1 against the
reference's outputs (tests/golden/encoder_resnext.npz), batch invariance, the fused-tail gate, and a ResNeXt model end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import synth

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16x6", "f16x3"]
MEAN = torch.tensor([102.9801, 115.9465, 122.7717])[None, :, None, None]


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def _rand(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def _conv_ref(x, w, b, groups, stride, dtype):
    """x [C][T][H][W] -> [Cout][T][Ho][Wo] by F.conv2d over the frames in `dtype`."""
    xt = torch.from_numpy(x).permute(1, 0, 2, 3).to(dtype)
    o = F.conv2d(xt, torch.from_numpy(w).to(dtype), None if b is None else torch.from_numpy(b).to(dtype), stride=stride, padding=1, groups=groups)
    return o.permute(1, 0, 2, 3).contiguous().double().numpy()


def _run(hip, x, w, b, groups, stride, precision, relu=False):
    Cin, T, H, W = x.shape
    Cout = w.shape[0]
    xh = F.pad(torch.from_numpy(x), (1, 1, 1, 1)).contiguous().cuda()
    vin = hip.Volume(xh.data_ptr(), T * (H + 2) * (W + 2), (H + 2) * (W + 2), W + 2, Cin, T, H + 2, W + 2, xh.numel())
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.full((Cout, T, Ho, Wo), float("nan"), device="cuda")
    pw = hip.pack_grouped_conv_weight(torch.from_numpy(w).cuda(), groups, precision)
    hip.conv2d_grouped(vin, pw, None if b is None else torch.from_numpy(b).cuda(), hip.dense_volume(out), groups, stride, relu, precision)
    torch.cuda.synchronize()
    return out.cpu().double().numpy()


def _check(name, got, x, w, b, groups, stride):
    ref = _conv_ref(x, w, b, groups, stride, torch.float64)
    e32 = float(np.abs(_conv_ref(x, w, b, groups, stride, torch.float32) - ref).max())
    err = float(np.abs(got - ref).max())
    bound = max(3.0 * e32, 4e-7 * float(np.abs(ref).max()))
    print("[grouped] %-40s max|err| %.3e  fp32 CPU %.3e  bound %.3e" % (name, err, e32, bound))
    assert np.isfinite(got).all() and err <= bound, name


# (groups, channels per group, stride): every per-group width at stride 1 and 2, 32 and 64 groups, one group at stride 2
CASES = [(32, c, s) for c in (4, 8, 16, 32, 64) for s in (1, 2)] + [(64, 4, 1), (64, 8, 2), (64, 16, 1), (1, 64, 2), (1, 128, 2)]


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("groups,cg,stride", CASES)
def test_grouped_conv_vs_fp64_ragged(hip, precision, groups, cg, stride):
    C = groups * cg
    T, H, W = 2, 13, 37                                                  # odd rows, columns not a multiple of 32
    x = _rand((C, T, H, W), 1 + cg + stride)
    w = _rand((C, cg, 3, 3), 2 + cg, 1.0 / np.sqrt(cg * 9))
    b = _rand((C,), 3)
    got = _run(hip, x, w, b, groups, stride, precision)
    _check("%s g%d x %d s%d" % (precision, groups, cg, stride), got, x, w, b, groups, stride)


@pytest.mark.parametrize("precision", MODES)
def test_grouped_conv_stage1_frame_and_relu(hip, precision):
    """The 4x level of a 480 x 864 frame (ResNeXt-101 32x8d layer1 conv2: 256 channels, 32 groups of 8), + bias + ReLU."""
    C, cg, T, H, W = 256, 8, 1, 120, 216
    x = np.maximum(_rand((C, T, H, W), 7), 0)
    w, b = _rand((C, cg, 3, 3), 8, 1.0 / np.sqrt(cg * 9)), _rand((C,), 9)
    got = _run(hip, x, w, b, 32, 1, precision, relu=True)
    ref = np.maximum(_conv_ref(x, w, b, 32, 1, torch.float64), 0)
    e32 = float(np.abs(np.maximum(_conv_ref(x, w, b, 32, 1, torch.float32), 0) - ref).max())
    assert np.abs(got - ref).max() <= max(3.0 * e32, 4e-7 * np.abs(ref).max())


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("xscale", [1e-4, 1e-2, 1.0, 100.0, 2e4])
def test_grouped_conv_operand_magnitudes(hip, precision, xscale):
    """Activations of 1e-4 ... 2e4 times unit scale (the f16x3 operand scaling must keep fp32-level results over that range)."""
    groups, cg, T, H, W = 32, 8, 2, 11, 40
    C = groups * cg
    x = _rand((C, T, H, W), 31, xscale)
    w, b = _rand((C, cg, 3, 3), 32, 1.0 / np.sqrt(cg * 9)), _rand((C,), 33, xscale)
    for stride in (1, 2):
        _check("%s x*%g s%d" % (precision, xscale, stride), _run(hip, x, w, b, groups, stride, precision), x, w, b, groups, stride)


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("cg", [8, 64])
def test_grouped_conv_per_channel_weight_range(hip, precision, cg):
    """Per-output-channel weight magnitudes log-uniform over 2^-20 ... 1 (FrozenBN folded with eps = 0): every channel is held to the
    fp32 CPU error level relative to its own output scale."""
    rs = np.random.RandomState(41)
    groups, T, H, W = 32, 2, 9, 35
    C = groups * cg
    ch = (2.0 ** rs.uniform(-20, 0, size=(C, 1, 1, 1))).astype(np.float32)
    x = np.maximum(_rand((C, T, H, W), 42, 30.0), 0)
    w = _rand((C, cg, 3, 3), 43, 1.0 / np.sqrt(cg * 9)) * ch
    got = _run(hip, x, w, None, groups, 1, precision)
    ref = _conv_ref(x, w, None, groups, 1, torch.float64)
    r32 = _conv_ref(x, w, None, groups, 1, torch.float32)
    scale = np.abs(ref.reshape(C, -1)).max(1)
    e = np.abs(got - ref).reshape(C, -1).max(1) / scale
    e32 = np.abs(r32 - ref).reshape(C, -1).max(1) / scale
    print("[grouped] %s per-channel range 2^-20..1: worst relative error %.3e (fp32 CPU %.3e)" % (precision, e.max(), e32.max()))
    assert np.isfinite(got).all() and e.max() <= max(3.0 * e32.max(), 4e-7)


def test_grouped_conv_f16x3_overflow_is_not_silent(hip):
    """|activation| >= 2.6e5 is beyond the f16x3 operand range: the outputs it feeds must be non-finite (what the overflow guard of
    ClipPipeline.step_checked looks for); in bf16x6 the same input is fine."""
    groups, cg, T, H, W = 32, 8, 1, 12, 40
    C = groups * cg
    x = _rand((C, T, H, W), 51)
    x[19, 0, 5, 17] = 3.0e5                                             # channel 19: group 2 (channels 16..23)
    w = _rand((C, cg, 3, 3), 52, 1.0 / np.sqrt(cg * 9))
    o = _run(hip, x, w, None, groups, 1, "f16x3")
    assert not np.isfinite(o[16:24, 0, 5, 17]).any()
    assert np.isfinite(o[:, :, :3]).all() and np.isfinite(o[:, :, 8:]).all()
    _check("bf16x6 3e5", _run(hip, x, w, None, groups, 1, "bf16x6"), x, w, None, groups, 1)


def test_grouped_conv_is_frame_count_invariant(hip):
    """No split-K: a frame's output bits do not depend on the frames that share its launch."""
    groups, cg, H, W = 32, 16, 15, 27
    C = groups * cg
    x = _rand((C, 6, H, W), 61)
    w, b = _rand((C, cg, 3, 3), 62, 1.0 / np.sqrt(cg * 9)), _rand((C,), 63)
    for precision in MODES:
        for stride in (1, 2):
            whole = _run(hip, x, w, b, groups, stride, precision)
            one = _run(hip, np.ascontiguousarray(x[:, 4:5]), w, b, groups, stride, precision)
            assert np.array_equal(whole[:, 4:5], one), (precision, stride)


# ------------------------------------------------------------------------------------------------ encoder
RESNEXT = {"X50_32x4d": "R-50-FPN", "X101_32x8d_s3": "R-101-FPN", "R50_s3": "R-50-FPN"}


def _backbone(g, tag, precision):
    from stemseg_amd.modeling.backbone import ResNetFPN
    H, W, seed, stride, groups, width, s1x1 = g[tag + "__meta"].tolist()
    bb = ResNetFPN(RESNEXT[tag], 256, groups, width, bool(s1x1)).eval()
    sd = {k: torch.from_numpy(np.asarray(synth.synth_param("backbone." + k, v.shape, seed))).reshape(v.shape) for k, v in bb.state_dict().items()}
    bb.load_state_dict(sd)
    bb.precision = precision
    return bb.cuda(), (H, W, seed, stride)


def _frames(n, H, W, seed):
    x = synth.synth_frames(n, H, W, seed=seed).astype(np.float32)
    return torch.from_numpy(x).permute(0, 3, 1, 2) - MEAN


@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("tag", list(RESNEXT))
def test_resnext_encoder_vs_golden(hip, golden, tag, precision):
    g = golden("encoder_resnext")
    bb, (H, W, seed, stride) = _backbone(g, tag, precision)
    feats = bb.run_backbone(_frames(2, H, W, seed).cuda())
    for s in (4, 8, 16, 32):
        ref = g["%s_s%d" % (tag, s)]
        assert list(feats[s].shape) == g["%s_s%d__shape" % (tag, s)].tolist()
        got = feats[s].contiguous().cpu().numpy().reshape(-1)[::stride]
        scale = max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(got - ref).max()) / scale
        print("[resnext] %s %s 1/%d: max|err| / max %.3e" % (tag, precision, s, err))
        assert err <= 1e-4, (tag, precision, s)
    bad, where = bb.check_workspaces()
    assert bad == 0, where


def test_resnext101_frame_is_batch_invariant(hip, golden):
    """ResNeXt-101 32x8d (stride in the 3x3), f16x3: one frame's four maps alone, inside a 4-clip pass, and inside overlapping windows
    (the same plan_frames) are torch.equal."""
    g = golden("encoder_resnext")
    bb, _ = _backbone(g, "X101_32x8d_s3", "f16x3")
    H, W = 64, 96
    fr = _frames(12, H, W, 5).cuda().contiguous()

    def maps(T):
        return [torch.empty(256, T, H // s, W // s, device="cuda") for s in (4, 8, 16, 32)]
    alone = maps(1)
    bb.run_backbone_into(fr[6:7].contiguous(), [hip.dense_volume(o) for o in alone])
    clips = [maps(3) for _ in range(4)]                                  # frames 0..11 as four clips of three: frame 6 is clip 2, frame 0
    bb.run_backbone_into(fr, [hip.dense_volume(o) for c in clips for o in c])
    wins = [maps(4) for _ in range(5)]                                   # windows of 4 every 2 frames: frame 6 is window 2 frame 2, window 3 frame 0
    bb.run_backbone_into(fr, [hip.dense_volume(o) for c in wins for o in c], window=(4, 2))
    torch.cuda.synchronize()
    for k in range(4):
        a = alone[k][:, 0]
        assert torch.isfinite(a).all()
        assert torch.equal(a, clips[2][k][:, 0]) and torch.equal(a, wins[2][k][:, 2]) and torch.equal(a, wins[3][k][:, 0]), k
    assert bb.check_workspaces()[0] == 0


def test_fused_tail_is_inert_for_resnext(hip, golden):
    """The fused bottleneck tail exists for one group at today's widths only: on ResNeXt fuse_tail 0 and 7 give the same bits."""
    g = golden("encoder_resnext")
    for tag in ("X50_32x4d", "X101_32x8d_s3"):
        bb, (H, W, seed, _) = _backbone(g, tag, "f16x3")
        x = _frames(2, H, W, seed).cuda()
        bb.fuse_tail = 0
        a = [t.clone() for t in bb.forward_channel_major(x)]
        bb.fuse_tail = 7
        b = bb.forward_channel_major(x)
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(a, b)), tag


def test_resnext_model_end_to_end_graph_and_clustering(hip):
    """An InferenceModel built from a ResNeXt-101 32x8d cfg (STRIDE_IN_1X1 False): a clip through a captured ClipPipeline step has the
    eager step's bits, and the labels equal the oracle clusterer's on the same embeddings (ties at a threshold excepted)."""
    from oracle import pipeline as opipe
    from stemseg_amd import config
    from stemseg_amd.modeling.inference_model import InferenceModel
    from stemseg_amd.pipeline import ClipPipeline
    config.load_preset("davis")
    try:
        config.cfg.MODEL.BACKBONE.TYPE = "R-101-FPN"
        r = config.cfg.MODEL.RESNETS
        r.NUM_GROUPS, r.WIDTH_PER_GROUP, r.STRIDE_IN_1X1 = 32, 8, False
        model = InferenceModel()
        bb = model._model.backbone
        assert (bb.num_groups, bb.width_per_group, bb.stride_in_1x1) == (32, 8, False)
        assert tuple(model._model.state_dict()["backbone.body.layer1.0.conv2.weight"].shape) == (256, 8, 3, 3)
        names = [(k, v.shape) for k, v in model._model.state_dict().items()]
        sd = synth.synth_state_dict(names, 7)
        sd["seediness_head.conv_out.weight"] = sd["seediness_head.conv_out.weight"] * -30      # (this trunk's seediness logits are all negative at +30)
        model._model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(model._model.state_dict()[k].shape) for k, v in sd.items()})
        pipe = ClipPipeline(model, device="cuda:0")
        clip = (torch.from_numpy(synth.synth_frames(8, 96, 128, seed=7).astype(np.float32)).permute(0, 3, 1, 2) -
                torch.tensor(config.cfg.INPUT.IMAGE_MEAN)[None, :, None, None]).cuda().contiguous()
        eager = pipe.step(clip)
        keep = {k: eager[k].clone() for k in ("emb", "bw", "seed", "labels", "fg")}
        assert all(bool(torch.isfinite(keep[k]).all()) for k in ("emb", "bw", "seed"))
        gstep = pipe.capture(clip)
        for _ in range(2):
            o = gstep.run(clip)
            torch.cuda.synchronize()
            assert all(torch.equal(o[k], keep[k]) for k in keep)
        emb, bw, seed = keep["emb"].cpu(), keep["bw"].cpu(), keep["seed"].cpu()
        fg = opipe.fg_mask_from_seediness([(list(range(seed.shape[1])), seed)], 0.25)
        labels, meta, _ = opipe.cluster_clip(emb, bw, seed, fg, free_dim_stds=[0.3, 0.3], return_probs=True)
        o2 = pipe.cluster(keep["emb"].contiguous(), keep["bw"].contiguous(), keep["seed"].contiguous())
        n = int(o2["frame_offsets"].cpu()[-1])
        assert n == labels.shape[0] and n > 0
        assert hip.read_cluster_meta(o2["meta"]).K == len(meta["instance_labels"])
        bad = np.flatnonzero(o2["labels"][:n].cpu().numpy() != labels)
        if bad.size:
            P = np.stack(meta["instance_probs"])
            near = (np.abs(P - 0.5) < 2e-6).any(0) | (np.abs(P - 0.3) < 2e-6).any(0)
            assert near[bad].all(), "%d labels differ from the oracle clusterer away from the threshold band" % bad.size
    finally:
        config.load_preset("defaults")
