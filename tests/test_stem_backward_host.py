"""Host tests of the stem backward (csrc/stem_backward.hip behind hip.maxpool3x3s2_backward / stem_wgrad; stemseg_hip_encoder_stem_forward;
encoder_backward.stem_backward / body_backward at freeze_at 0 and 1; ResNetFPN.train_stem; TrainingModel.train_stem;
configure_trainable(train_stem=True); --train_stem): the window rule of the GPU tests against torch's CPU backward bit for bit, the C-ABI
and its argument checks (made before any GPU call), the chunk plan, the refusals with the switch off and the parameter lists with it on.
No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import stem_backward_cases as SC
from tests import stem_backward_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("stemseg_hip_maxpool3x3s2_backward", "stemseg_hip_stem_wgrad", "stemseg_hip_stem_wgrad_chunks", "stemseg_hip_stem_wgrad_workspace_bytes",
         "stemseg_hip_encoder_stem_forward")


@pytest.mark.parametrize("planes,H,W", SC.POOL_CASES + ((1, 10, 14),))
@pytest.mark.parametrize("mask_relu", [False, True])
def test_window_rule_is_torchs_cpu_backward(planes, H, W, mask_relu):
    """The numpy restatement of the kernel's rule -- first maximum wins, last NaN wins, windows added in ascending order in fp32 -- gives the
    bits of ``F.max_pool2d(x, 3, 2, 1).backward`` (and of ``threshold_backward`` behind it) on every pool case."""
    x, g = SC.pool_input(planes, H, W), SC.pool_upstream(planes, H, W)
    if H >= 4 and W >= 6:
        assert np.isnan(x).sum() >= 5 and np.isinf(x).any() and (x == 0).sum() > x.size // 8 and np.signbit(x[x == 0]).any()
        assert ((x > 0) & (x < 1e-38)).any() and (g == 0).any()
    want = SO.pool_backward_torch(x, g, mask_relu)
    got = SO.pool_backward_rule(x, g, mask_relu)
    assert torch.equal(SO.bits(got), SO.bits(want))


def test_symbols_exported_declared_and_bound():
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward
    from stemseg_amd.modeling.backbone import ResNetFPN
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    for n in NAMES:
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in header and hip.lib().stemseg_hip_version() == 11 and hip.ABI_VERSION == 11
    # the argument lists of the binding are the header's
    count = lambda n: header[header.index(n + "("):].split(";")[0].count(",") + 1
    for n in NAMES:
        assert len(hip.SIGNATURES[n][1]) == count(n), n
    for f in ("maxpool3x3s2_backward", "stem_wgrad", "stem_wgrad_chunks"):
        assert callable(getattr(hip, f)), f
    assert callable(encoder_backward.stem_backward) and callable(ResNetFPN.stem_forward)
    assert os.path.exists(os.path.join(ROOT, "stem-seg_amd", "csrc", "stem_backward.hip"))


def test_calls_reject_bad_arguments_before_any_gpu_call():
    from stemseg_amd import hip
    l = hip.lib()
    err = l.stemseg_hip_last_error
    fake = ctypes.c_void_p(256)
    used = ctypes.c_int32(-7)
    pb = lambda x=fake, g=fake, planes=3, H=4, W=8, mask=0, dx=fake, form=0: l.stemseg_hip_maxpool3x3s2_backward(x, g, planes, H, W, mask, dx, form, ctypes.byref(used), None)
    assert pb(x=None) == -1 and b"maxpool3x3s2_backward: null pointer" in err()
    assert pb(g=None) == -1 and b"null pointer" in err()
    assert pb(dx=None) == -1 and b"null pointer" in err()
    assert pb(H=5) == -1 and b"maxpool3x3s2_backward: planes=3 H=5 W=8 (H, W even)" in err()
    assert pb(W=7) == -1 and b"(H, W even)" in err()
    assert pb(planes=0) == -1 and b"planes=0" in err()
    assert pb(mask=2) == -1 and b"mask_relu=2" in err()
    assert pb(form=3) == -1 and b"form=3" in err()
    assert pb(W=6, form=hip.STREAM_FORM_VEC4) == -1 and b"the 16-byte form needs W % 4 == 0 (W=6)" in err()
    assert pb(dx=ctypes.c_void_p(260), form=hip.STREAM_FORM_VEC4) == -1 and b"16-byte aligned x and dx" in err()
    assert pb(x=ctypes.c_void_p(264), form=hip.STREAM_FORM_VEC4) == -1 and b"16-byte aligned x and dx" in err()
    assert used.value == -7                                  # nothing ran

    sw = lambda fr=fake, g=fake, F=2, H=8, W=12, dw=fake, ws=fake, n=1 << 30: l.stemseg_hip_stem_wgrad(fr, g, F, H, W, dw, ws, n, None)
    assert sw(fr=None) == -1 and b"stem_wgrad: frames is a null pointer" in err()
    assert sw(g=None) == -1 and b"stem_wgrad: g is a null pointer" in err()
    assert sw(dw=None) == -1 and b"stem_wgrad: dw is a null pointer" in err()
    assert sw(ws=None) == -1 and b"stem_wgrad: workspace is a null pointer" in err()
    assert sw(H=9) == -1 and b"stem_wgrad: F=2 H=9 W=12 (H, W even)" in err()
    assert sw(W=13) == -1 and b"(H, W even)" in err()
    assert sw(F=0) == -1 and b"F=0" in err()
    assert sw(ws=ctypes.c_void_p(264)) == -1 and b"workspace must be 256-byte aligned" in err()
    need = l.stemseg_hip_stem_wgrad_workspace_bytes(2, 8, 12)
    assert need == l.stemseg_hip_stem_wgrad_chunks(2, 8, 12) * 64 * 147 * 8
    assert sw(n=need - 1) == -3 and b"stem_wgrad: workspace too small (%d < %d bytes)" % (need - 1, need) in err()
    assert l.stemseg_hip_stem_wgrad_workspace_bytes(2, 7, 12) == 0 and b"(H, W even)" in err()
    assert l.stemseg_hip_stem_wgrad_chunks(2, 8, 11) == -1

    d = hip.EncoderDesc()
    d.struct_bytes = ctypes.sizeof(hip.EncoderDesc)
    assert l.stemseg_hip_encoder_stem_forward(ctypes.byref(d), None, fake, fake, fake, fake, 1 << 40, None) == -1      # (an empty descriptor: refused by the plan)
    assert l.stemseg_hip_encoder_stem_forward(None, None, fake, fake, fake, fake, 1 << 40, None) == -1 and b"null descriptor" in err()


def test_python_wrappers_name_the_bad_argument():
    from stemseg_amd import hip
    from stemseg_amd.modeling import encoder_backward as EB
    with pytest.raises(ValueError, match=r"maxpool3x3s2_backward: x \(2, 3, 4\) must be \[planes, H, W\] with even H and W"):
        hip.maxpool3x3s2_backward(torch.zeros(2, 3, 4), torch.zeros(2, 1, 2))
    with pytest.raises(ValueError, match=r"maxpool3x3s2_backward: g \(2, 2, 3\), expected \(2, 2, 2\)"):
        hip.maxpool3x3s2_backward(torch.zeros(2, 4, 4), torch.zeros(2, 2, 3))
    with pytest.raises(ValueError, match="maxpool3x3s2_backward: out"):
        hip.maxpool3x3s2_backward(torch.zeros(2, 4, 4), torch.zeros(2, 2, 2), out=torch.zeros(2, 4, 5))
    with pytest.raises(ValueError, match=r"stem_wgrad: frames \(2, 4, 8, 8\) must be \[F, 3, H, W\]"):
        hip.stem_wgrad(torch.zeros(2, 4, 8, 8), torch.zeros(64, 2, 4, 4))
    with pytest.raises(ValueError, match="stem_wgrad: g .* against frames"):
        hip.stem_wgrad(torch.zeros(2, 3, 8, 8), torch.zeros(64, 2, 4, 5))
    with pytest.raises(ValueError, match="stem_wgrad: "):
        hip.stem_wgrad_chunks(1, 8, 9)
    with pytest.raises(ValueError, match="stem_backward: G_pooled"):
        EB.stem_backward(torch.zeros(2, 3, 16, 16), torch.zeros(64, 2, 8, 8), torch.zeros(64, 2, 4, 5))
    with pytest.raises(ValueError, match="stem_backward: frames"):
        EB.stem_backward(torch.zeros(2, 3, 16, 18), torch.zeros(64, 2, 8, 8), torch.zeros(64, 2, 4, 4))
    with pytest.raises(ValueError, match="stem_backward: stem_map"):
        EB.stem_backward(torch.zeros(2, 3, 12, 16), torch.zeros(64, 2, 6, 9), torch.zeros(64, 2, 3, 4))


def test_chunk_counts_come_from_the_library():
    """Every case's chunk count is ``stem_wgrad_chunks``', which is the plan restated in tests/stem_backward_cases.py; the list holds a one-chunk
    case, one of at least three chunks and one whose last chunk is ragged; the benchmark's shape stays near a thousand workgroups."""
    from stemseg_amd import hip
    plans = {}
    for Fr, H, W in SC.WGRAD_CASES:
        tiles, per, chunks = SC.wgrad_plan(Fr, H, W)
        assert hip.stem_wgrad_chunks(Fr, H, W) == chunks, (Fr, H, W)
        assert hip.lib().stemseg_hip_stem_wgrad_workspace_bytes(Fr, H, W) == chunks * 64 * 147 * 8
        plans[(Fr, H, W)] = (tiles, per, chunks)
    assert any(c == 1 for _, _, c in plans.values())
    assert any(c >= 3 for _, _, c in plans.values())
    assert any(c >= 3 and t % p for t, p, c in plans.values())          # a ragged last chunk behind whole ones
    assert plans[SC.WGRAD_SEVERAL] == (30, 4, 8)
    assert hip.stem_wgrad_chunks(8, 480, 864) == SC.wgrad_plan(8, 480, 864)[2] == 960
    # no chunk is longer than 8 tiles, whatever the shape: beyond 8192 tiles the chunks grow in number, not in length
    assert SC.wgrad_plan(32, 480, 864) == (26880, 8, 3360) and hip.stem_wgrad_chunks(32, 480, 864) == 3360
    # a function of the shape only: the same answer again
    assert [hip.stem_wgrad_chunks(*c) for c in SC.WGRAD_CASES] == [plans[c][2] for c in SC.WGRAD_CASES]


def test_one_hot_patch_is_the_oracles_gradient():
    """The patch the GPU test expects for a one-hot upstream is what autograd gives, at the four corners (zero padding on two sides each)."""
    frames, _ = SC.wgrad_case(2, 14, 22)
    for f, oy, ox in ((0, 0, 0), (1, 0, 10), (0, 6, 0), (1, 6, 10), (1, 3, 5)):
        g = np.zeros((64, 2, 7, 11), np.float32)
        g[5, f, oy, ox] = 1.0
        dw = SO.wgrad_oracle(frames, g, torch.float64)
        assert np.array_equal(dw[5], SO.stem_patch(frames, f, oy, ox).astype(np.float64)) and not dw[:5].any() and not dw[6:].any()
    assert not SO.stem_patch(frames, 0, 0, 0)[:, :3].any() and not SO.stem_patch(frames, 1, 6, 10)[:, :, 5:].any()


def test_refusals_unchanged_with_the_switch_off_and_lists_with_it_on():
    from stemseg_amd.modeling import encoder_backward as EB
    from stemseg_amd.modeling.backbone import ResNetFPN
    bb = ResNetFPN("R-50-FPN")
    assert bb.train_stem is False
    for fa in (1, 0):
        with pytest.raises(NotImplementedError) as e:
            bb.check_body_trainable(fa)
        assert str(e.value) == ("MODEL.BACKBONE.FREEZE_AT_STAGE=%d: the body's backward covers layer2 .. layer4 (FREEZE_AT_STAGE 2, 3 or 4); below that it "
                                "would need the backward of the max-pool and the stem" % fa)
        with pytest.raises(NotImplementedError) as e:
            EB.body_backward({}, {}, {}, "f32", freeze_at=fa)
        assert str(e.value) == ("body_backward: freeze_at = %d; stages below 2 need the backward of the max-pool and the stem "
                                "(MODEL.BACKBONE.FREEZE_AT_STAGE >= 2)" % fa)
        with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE=%d" % fa):
            bb.forward_trainable_body(torch.zeros(1, 3, 32, 32), fa)
    bb.train_stem = True
    for fa in (0, 1, 2, 3, 4):
        bb.check_body_trainable(fa)
    for fa in (-1, 5):
        with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE"):
            bb.check_body_trainable(fa)
        with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE"):
            EB.body_backward({}, {}, {}, "f32", freeze_at=fa, stem={})
    names = {id(p): n for n, p in bb.named_parameters()}
    got = [names[id(p)] for p in bb.body_parameter_list(0)]
    assert got == [n for n, _ in bb.named_parameters() if n.startswith("body.")] and len(got) == 1 + 10 + 42
    assert got[:3] == ["body.stem.conv1.weight", "body.layer1.0.downsample.0.weight", "body.layer1.0.conv1.weight"]
    assert [names[id(p)] for p in bb.body_parameter_list(1)] == got[1:]
    assert [names[id(p)] for p in bb.body_parameter_list(2)] == got[11:]
    assert len(ResNetFPN("R-101-FPN").body_parameter_list(2)) == 93
    # the ResNeXt refusals stand beside the new switch
    x = ResNetFPN("R-50-FPN", num_groups=32, width_per_group=4)
    x.train_stem = True
    with pytest.raises(NotImplementedError, match=r"MODEL\.RESNETS\.NUM_GROUPS=32"):
        x.body_parameter_list(0)
    x.train_resnext = True
    assert len(x.body_parameter_list(0)) == 53


@pytest.fixture()
def model():
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        yield build_model()
    finally:
        config.load_preset("defaults")


def test_training_model_switch(model):
    m = model
    sd = dict(m.named_parameters())
    frames = torch.zeros(1, 8, 3, 32, 32)
    assert m.train_stem is False and m.backbone.train_stem is False
    with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE=0"):
        m.body_parameters(0)
    m.train_decoders = m.train_fpn = m.train_body = True
    assert m.body_freeze_at() == 2                           # (switch off: the stem's trainable parameters do not count)
    with pytest.raises(NotImplementedError) as e:
        m(frames, [])
    assert str(e.value) == ("TrainingModel.forward with train_decoders, train_fpn and train_body: the backward pass of the stem, the max-pool and layer1 "
                            "is not implemented (MODEL.BACKBONE.FREEZE_AT_STAGE >= 2), and 11 parameters there require a gradient "
                            "(backbone.body.stem.conv1.weight, ...); freeze them (requires_grad_(False) on backbone.body.stem and backbone.body.layer1)")
    m.train_stem = True
    assert m.backbone.train_stem is True
    body0, body1 = m.body_parameters(0), m.body_parameters(1)
    assert len(body0) == 1 + 10 + 42 and len(body1) == 10 + 42 and len(m.body_parameters(2)) == 42
    assert next(iter(body0)) == "backbone.body.stem.conv1.weight" and all(body0[k] is sd[k] for k in body0)
    assert list(body0)[1:] == list(body1)
    assert [id(p) for p in m.backbone.body_parameter_list(0)] == [id(p) for p in body0.values()]
    assert [id(p) for p in m.backbone.body_parameter_list(1)] == [id(p) for p in body1.values()]
    assert m.body_freeze_at() == 0 and m.body_fpn_and_decoders_only_trainable(0) and not m.body_fpn_and_decoders_only_trainable(1)
    sd["backbone.body.stem.conv1.weight"].requires_grad_(False)
    assert m.body_freeze_at() == 1 and m.body_fpn_and_decoders_only_trainable(1)
    m.backbone.body.layer1.requires_grad_(False)
    assert m.body_freeze_at() == 2
    m.train_stem = False
    assert m.backbone.train_stem is False


def test_configure_trainable_with_train_stem(model):
    from stemseg_amd import config
    from stemseg_amd.training.utils import configure_trainable
    m = model
    cfg = config.cfg
    old = cfg.MODEL.BACKBONE.FREEZE_AT_STAGE
    try:
        for fa in (0, 1):
            cfg.MODEL.BACKBONE.FREEZE_AT_STAGE = fa
            m.train_stem = False
            with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.FREEZE_AT_STAGE=%d" % fa):     # (refused before anything is changed)
                configure_trainable(m, cfg, freeze_backbone=False)
            assert m.train_stem is False and m.backbone.train_stem is False
            configure_trainable(m, cfg, freeze_backbone=False, train_stem=True)
            assert m.train_stem and m.backbone.train_stem and m.train_body and m.train_fpn and m.train_decoders
            assert m.body_freeze_at() == fa
            trainable = {k for k, p in m.named_parameters() if p.requires_grad and k.startswith("backbone.body.")}
            assert trainable == set(m.body_parameters(fa))
            assert m.backbone.body.stem.conv1.weight.requires_grad == (fa == 0)
            assert all(p.requires_grad for p in m.backbone.body.layer1.parameters())
        cfg.MODEL.BACKBONE.FREEZE_AT_STAGE = 2
        configure_trainable(m, cfg, freeze_backbone=False, train_stem=True)
        assert m.train_stem and m.body_freeze_at() == 2 and not m.backbone.body.stem.conv1.weight.requires_grad
        configure_trainable(m, cfg, freeze_backbone=False)
        assert m.train_stem is False and m.backbone.train_stem is False
        configure_trainable(m, cfg, freeze_backbone=True, train_stem=True)
        assert m.train_stem is False and not any(p.requires_grad for p in m.backbone.parameters())
    finally:
        cfg.MODEL.BACKBONE.FREEZE_AT_STAGE = old


def test_command_line_flag():
    from stemseg_amd.training.main import build_parser
    p = build_parser()
    assert p.parse_args(["--model_dir", "x", "--cfg", "davis"]).train_stem is False
    assert p.parse_args(["--model_dir", "x", "--cfg", "davis", "--train_stem"]).train_stem is True


@pytest.mark.parametrize("flag", [True, False])
def test_trainer_hands_the_flag_to_configure_trainable(monkeypatch, flag):
    """``Trainer`` passes ``args.train_stem`` on as ``configure_trainable(train_stem=True)``, and nothing new when the flag is off or absent."""
    import logging
    from types import SimpleNamespace
    from stemseg_amd.training import main as TM
    seen = {}

    class Stop(Exception):
        pass

    def fake(model, **kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(TM, "configure_trainable", fake)
    cfg = SimpleNamespace(MIXED_PRECISION=False, FREEZE_BACKBONE=False)
    args = SimpleNamespace(restore_session=None, initial_ckpt=None, **({"train_stem": True} if flag else {}))
    with pytest.raises(Stop):
        TM.Trainer(cfg, "unused", args, logging.getLogger("test"), model=torch.nn.Linear(1, 1))
    assert seen == (dict(freeze_backbone=False, train_stem=True) if flag else dict(freeze_backbone=False))
