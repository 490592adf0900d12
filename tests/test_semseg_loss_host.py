"""CPU tests of the training targets, the semseg cross-entropy and the foreground loss: the torch oracle (tests/semseg_loss_oracle.py)
against the golden values of the reference's own resize_masks / CrossEntropyLoss / compute_fg_loss (tests/golden/semseg_loss.npz, written
by tools/make_semseg_loss_goldens.py), the C-ABI of the four entry points (argument errors are reported before any GPU call) and the
public modules' interface.

Bounds: prepared targets are integers and must be identical.  For the losses both sides are fp32 restatements of one arithmetic in
different summation orders, so the yardstick is that arithmetic's own fp32-versus-fp64 spread on the fixtures (the oracle in both
precisions, and the golden values against the fp64 oracle), measured on the CPU: at most 2.5e-7 relative on a loss
(weight_semseg_2p5, the weighted cross-entropy; 2.1e-7 unweighted), 2.6e-7 of max|g| on an element of a gradient (k3_fg_n2_kitti,
the cross-entropy's).  Allowed: 4 x that.  The oracle's fp32 results sit at 0 to 1.1e-7 (losses) and 0 to 1.8e-7 (gradient) from the
goldens."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import semseg_loss_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = SO.load_fixtures(os.path.join(ROOT, "tests", "golden", "semseg_loss.npz"))
LOSS_REL = 4 * 2.5e-7
GRAD_REL = 4 * 2.6e-7


def test_fixture_list_covers_the_quirks():
    assert sorted(FIXTURES) == sorted(SO.FIXTURE_CASES)
    f = FIXTURES["k2_fg_n1"]
    assert (f["K"], f["has_fg"], f["x"].shape[0], f["x"].shape[1]) == (2, True, 1, 3)
    f = FIXTURES["k3_fg_n2_kitti"]
    assert (f["K"], f["has_fg"], f["x"].shape[0], f["x"].shape[1]) == (3, True, 2, 4)
    f = FIXTURES["k41_fg_ytvis_width"]
    assert (f["K"], f["x"].shape[1]) == (41, 42) and int(f["prepared"][0]["semseg_masks"].max()) == 40
    f = FIXTURES["k5_no_fg"]
    assert not f["has_fg"] and f["x"].shape[1] == f["K"] == 5 and f["losses"][2] == 0
    f = FIXTURES["no_instances"]                                      # all background: nothing set at either resolution
    assert not f["targets"][0]["masks"].any() and not f["prepared"][0]["semseg_masks"].any() and f["prepared"][1]["semseg_masks"].any()
    f = FIXTURES["overlap_max_rule"]                                  # a pixel of two instances with different categories takes the larger id
    m, cats, sem = f["prepared"][0]["masks"].bool(), f["targets"][0]["category_ids"], f["prepared"][0]["semseg_masks"]
    both = m[0] & m[1]
    assert cats.tolist() == [2, 5, 3, 4] and both.any() and (sem[both] >= 5).all()
    lower_on_top = m[1] & m[2] & m[3]                                 # ... also when the LATER instances have the smaller ids (5, then 3, 4)
    assert lower_on_top.any() and (sem[lower_on_top] == 5).all()
    only = m[2] & m[3] & ~m[1]
    assert only.any() and (sem[only] == 4).all()
    for name, hw in (("odd_18x23", (18, 23)), ("odd_30x41_n2", (30, 41))):
        f = FIXTURES[name]
        assert tuple(f["targets"][0]["masks"].shape[-2:]) == hw and hw[0] % 4 and hw[1] % 4
        assert tuple(f["prepared"][0]["masks"].shape[-2:]) == (hw[0] // 4, hw[1] // 4) == tuple(f["x"].shape[-2:])
    ig = FIXTURES["ignore_partly"]["prepared"][0]["ignore_masks"]
    assert ig.any() and not ig.all()
    f = FIXTURES["ignore_all_n2"]                                     # the NaN case: sample 0 fully ignored, sample 1 not
    assert f["prepared"][0]["ignore_masks"].all() and not f["prepared"][1]["ignore_masks"].all()
    assert np.isnan(f["losses"]).all() and np.isnan(f["grad"][0]).all() and np.isfinite(f["grad"][1]).all() and f["grad"][1].any()
    f = FIXTURES["weight_semseg_2p5"]
    assert f["weight"] == 2.5 and f["losses"][1] == np.float32(np.float32(f["losses"][0]) * np.float32(2.5))
    # the four taps of an output pixel disagree somewhere: the AND is not a plain subsampling
    t = FIXTURES["k2_fg_n1"]["targets"][0]["masks"]
    assert not torch.equal(t[..., 1::4, 1::4][..., :8, :12], FIXTURES["k2_fg_n1"]["prepared"][0]["masks"])


@pytest.mark.parametrize("name", sorted(SO.FIXTURE_CASES))
def test_oracle_prepares_the_reference_targets_bit_exact(name):
    f = FIXTURES[name]
    x, targets = SO.make_case(name)                                   # the generator that made the stored inputs
    assert torch.equal(x, f["x"])
    for a, b in zip(targets, f["targets"]):
        assert all(torch.equal(a[k], b[k]) for k in ("masks", "ignore_masks", "category_ids"))
    for got, want in zip(SO.prepared(f["targets"]), f["prepared"]):
        for k in ("masks", "ignore_masks", "semseg_masks"):
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (name, k)


@pytest.mark.parametrize("name", sorted(SO.FIXTURE_CASES))
def test_oracle_reproduces_reference_losses_and_gradient(name):
    f = FIXTURES[name]
    losses, grads = SO.losses_and_grads(f["x"], f["prepared"], f["K"], f["has_fg"], torch.float32)
    got = [losses[0], float(np.float32(losses[0]) * np.float32(f["weight"])), losses[1]]
    gtotal = grads[0] * f["weight"] + grads[1]
    for g, want, what in zip(got, f["losses"], ("semseg", "weighted semseg", "foreground")):
        print(name, what, g, want)
        if np.isnan(want):
            assert np.isnan(g), (what, g)
        else:
            assert abs(g - want) <= LOSS_REL * abs(want), (what, g, want)
    nan = np.isnan(f["grad"])
    assert np.array_equal(np.isnan(gtotal), nan)                      # NaN where the reference has NaN, and nowhere else
    if (~nan).any():
        gmax = np.abs(f["grad"][~nan]).max()
        err = np.abs(gtotal[~nan] - f["grad"][~nan]).max()
        print(name, "grad max-norm error / max|g|", err / gmax)
        assert err <= GRAD_REL * gmax


# ------------------------------------------------------------------------------------------------ C-ABI
NAMES = ("stemseg_hip_prepare_targets", "stemseg_hip_semseg_loss_workspace_bytes", "stemseg_hip_semseg_loss_forward",
         "stemseg_hip_semseg_loss_backward")


def _desc(hip, **over):
    d = hip.semseg_loss_desc(3, True, 2, 4, 6, (48, 24, 6, 1))
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _prep(hip, **over):
    d = hip.target_prep_desc(2, 2, 16, 24)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def test_symbols_exported_declared_and_bound():
    from stemseg_amd import hip
    raw = ctypes.CDLL(hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    for n in NAMES:
        assert hasattr(raw, n) and n in hip.SIGNATURES and n + "(" in header, n
    assert "StemsegSemsegLossDesc" in header and "StemsegTargetPrepDesc" in header
    assert hip.lib().stemseg_hip_version() == 11
    assert ctypes.sizeof(hip.SemsegLossDesc) == 64 and ctypes.sizeof(hip.TargetPrepDesc) == 24


def test_semseg_loss_calls_reject_bad_arguments_before_any_gpu_call():
    from stemseg_amd import hip
    l = hip.lib()
    wsb = l.stemseg_hip_semseg_loss_workspace_bytes
    ws = wsb(ctypes.byref(_desc(hip)))
    assert ws > 0 and wsb(ctypes.byref(_desc(hip, T=4))) > ws
    assert wsb(ctypes.byref(_desc(hip, n_classes=41))) == ws          # the width does not enter: lse and the partial sums only
    assert wsb(ctypes.byref(_desc(hip, n_classes=0))) == ws           # the foreground channel alone
    for over, word in ((dict(struct_bytes=8), b"ABI skew"), (dict(n_classes=1), b"n_classes"), (dict(n_classes=129), b"n_classes"),
                       (dict(n_classes=0, has_foreground_channel=0), b"n_classes"), (dict(has_foreground_channel=2), b"has_foreground_channel"),
                       (dict(T=0), b"bad dims"), (dict(W=-1), b"bad dims"), (dict(T=4096, H=4096, W=128), b"voxels"),
                       (dict(stride_c=0), b"strides"), (dict(stride_w=-1), b"strides"), (dict(reserved=1), b"reserved"),
                       (dict(reserved2=1), b"reserved")):
        assert wsb(ctypes.byref(_desc(hip, **over))) == 0
        assert word in l.stemseg_hip_last_error(), (over, l.stemseg_hip_last_error())
    d, fake = _desc(hip), ctypes.c_void_p(256)
    fwd = lambda x=fake, s=fake, ig=fake, w=fake, nb=ws, out=fake, flag=fake, dd=d: l.stemseg_hip_semseg_loss_forward(
        ctypes.byref(dd), x, s, ig, w, nb, out, flag, None)
    for kw in (dict(x=None), dict(s=None), dict(ig=None), dict(w=None), dict(out=None), dict(flag=None)):
        assert fwd(**kw) == -1 and b"null pointer" in l.stemseg_hip_last_error(), kw
    assert fwd(nb=ws - 1) == -1 and b"workspace too small" in l.stemseg_hip_last_error()
    assert fwd(w=ctypes.c_void_p(8)) == -1 and b"256-byte aligned" in l.stemseg_hip_last_error()
    for kw in (dict(x=ctypes.c_void_p(258)), dict(out=ctypes.c_void_p(260)), dict(flag=ctypes.c_void_p(257))):
        assert fwd(**kw) == -1 and b"aligned" in l.stemseg_hip_last_error(), kw
    assert fwd(dd=_desc(hip, struct_bytes=4)) == -1 and b"ABI skew" in l.stemseg_hip_last_error()
    assert fwd(dd=_desc(hip, n_classes=200)) == -1 and b"n_classes" in l.stemseg_hip_last_error()
    bwd = lambda x=fake, up=fake, batch=1, g=fake, nb=ws, w=fake, dd=d: l.stemseg_hip_semseg_loss_backward(
        ctypes.byref(dd), x, fake, fake, w, nb, up, batch, g, None)
    assert bwd(up=None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert bwd(g=None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert bwd(batch=0) == -1 and b"batch_size" in l.stemseg_hip_last_error()
    assert bwd(nb=0) == -1 and b"workspace too small" in l.stemseg_hip_last_error()
    assert bwd(w=ctypes.c_void_p(64)) == -1 and b"256-byte aligned" in l.stemseg_hip_last_error()
    assert bwd(g=ctypes.c_void_p(258)) == -1 and b"aligned" in l.stemseg_hip_last_error()
    assert bwd(dd=_desc(hip, stride_t=0)) == -1 and b"strides" in l.stemseg_hip_last_error()


def test_prepare_targets_rejects_bad_arguments_before_any_gpu_call():
    from stemseg_amd import hip
    l = hip.lib()
    fake = ctypes.c_void_p(256)
    call = lambda dd=None, m=fake, ig=fake, cat=fake, mo=fake, io=fake, so=fake, flag=fake: l.stemseg_hip_prepare_targets(
        ctypes.byref(dd or _prep(hip)), m, ig, cat, mo, io, so, flag, None)
    for over, word in ((dict(struct_bytes=8), b"ABI skew"), (dict(n_instances=-1), b"n_instances"), (dict(n_instances=1025), b"n_instances"),
                       (dict(T=0), b"bad dims"), (dict(H=3), b"bad dims"), (dict(W=2), b"bad dims"), (dict(T=4096, H=4096, W=128), b"voxels"),
                       (dict(reserved=1), b"reserved")):
        assert call(dd=_prep(hip, **over)) == -1 and word in l.stemseg_hip_last_error(), (over, l.stemseg_hip_last_error())
    for kw in (dict(m=None), dict(ig=None), dict(cat=None), dict(mo=None), dict(io=None), dict(so=None), dict(flag=None)):
        assert call(**kw) == -1 and b"null pointer" in l.stemseg_hip_last_error(), kw
    assert call(flag=ctypes.c_void_p(258)) == -1 and b"aligned" in l.stemseg_hip_last_error()
    assert call(cat=ctypes.c_void_p(257)) == -1 and b"aligned" in l.stemseg_hip_last_error()


def test_isa_report_covers_the_semseg_loss_kernels():
    import json
    from stemseg_amd import hip
    rep = json.load(open(os.path.splitext(hip.LIB_PATH)[0] + ".isa.json"))["sources"]["semseg_loss.hip"]
    assert rep["assembly_found"] and rep["kernels"] == 4 and rep["packed_fp32_valu_instructions"] == 0


# ------------------------------------------------------------------------------------------------ public modules
def test_registry_constants_and_overlay_import():
    from stemseg_amd import overlay
    from stemseg_amd.modeling import losses, model_builder
    from stemseg_amd.utils.constants import Loss
    assert (Loss.SEMSEG, Loss.FOREGROUND) == ("semantic_segmentation_loss", "foreground")
    assert model_builder.SEMSEG_LOSS_REGISTRY["CrossEntropy"] is losses.CrossEntropyLoss
    overlay.install()
    try:
        from stemseg.modeling.losses import CrossEntropyLoss, EmbeddingLoss
        from stemseg.modeling.model_builder import TrainingModel
        assert CrossEntropyLoss is losses.CrossEntropyLoss and EmbeddingLoss is losses.EmbeddingLoss and TrainingModel is model_builder.TrainingModel
    finally:
        overlay.uninstall()


def test_cross_entropy_module_output_keys_and_weight(monkeypatch):
    from stemseg_amd import config
    from stemseg_amd.modeling.losses import cross_entropy as mod
    seen = []

    def fake_apply(logits, sems, igs, K, has_fg):
        seen.append((tuple(logits.shape), K, has_fg))
        return torch.tensor(0.5), torch.tensor(0.25)
    monkeypatch.setattr(mod.SemsegLossFunction, "apply", staticmethod(fake_apply))
    monkeypatch.setattr(mod.hip, "require_gpu", lambda: 1)
    monkeypatch.setattr(config.cfg.TRAINING.LOSSES, "WEIGHT_SEMSEG", 2.5)
    t = [{"semseg_masks": torch.zeros(2, 4, 6, dtype=torch.uint8), "ignore_masks": torch.zeros(2, 4, 6, dtype=torch.uint8)}]
    od = {"optimization_losses": {"embedding_loss": 1.0}, "others": {}}
    mod.CrossEntropyLoss()(torch.zeros(1, 2, 3, 4, 6), t, od)          # [N, T, cls, H, W] -> the function sees [N, cls, T, H, W]
    assert seen[-1] == ((1, 3, 2, 4, 6), 3, False)
    assert set(od["optimization_losses"]) == {"embedding_loss", "semantic_segmentation_loss"} and set(od["others"]) == {"semantic_segmentation_loss"}
    assert float(od["others"]["semantic_segmentation_loss"]) == 0.5 and float(od["optimization_losses"]["semantic_segmentation_loss"]) == 1.25
    od = {"optimization_losses": {}, "others": {}}
    mod.CrossEntropyLoss().forward_with_foreground(torch.zeros(1, 2, 4, 4, 6), t, od)
    assert seen[-1] == ((1, 4, 2, 4, 6), 3, True)
    assert set(od["optimization_losses"]) == {"semantic_segmentation_loss", "foreground"} and float(od["optimization_losses"]["foreground"]) == 0.25
    od = {"optimization_losses": {}, "others": {}}
    mod.foreground_loss(torch.zeros(1, 2, 4, 6), t, od)
    assert seen[-1] == ((1, 1, 2, 4, 6), 0, True) and set(od["optimization_losses"]) == {"foreground"} and not od["others"]


@pytest.fixture
def kitti_cfg():
    from stemseg_amd import config
    config.load_preset("kittimots")
    config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
    yield config.cfg
    config.load_preset("defaults")


def test_training_model_interface(kitti_cfg, monkeypatch):
    from stemseg_amd.modeling import losses, model_builder
    from stemseg_amd.modeling.inference_model import InferenceModel
    m = model_builder.build_model()
    assert type(m).__name__ == "TrainingModel" and isinstance(m, model_builder.InferenceOnlyModel)
    assert isinstance(m.embedding_loss_criterion, losses.EmbeddingLoss) and isinstance(m.semseg_loss_criterion, losses.CrossEntropyLoss)
    assert m.semseg_head.has_foreground_channel and m.semseg_head.out_channels == 4 and m.multiclass_semseg_output
    assert (m.embedding_head_output_scale, m.semseg_output_scale, m.output_resize_scale) == (4, 4, 1.0)
    assert {k.split(".")[0] for k in m.state_dict()} == {"backbone", "embedding_head", "semseg_head"}
    for name in ("resize_masks", "compute_fg_loss", "compute_losses", "forward", "run_backbone", "forward_embeddings_and_semseg"):
        assert callable(getattr(m, name))
    # gradients through the decoders and the encoder do not exist: a training call is refused, not answered with a dead graph
    assert any(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError, match="decoder and encoder backward"):
        m(torch.zeros(1, 8, 3, 64, 64), [])
    # the tail of forward: the embedding criterion, then ONE pass for the foreground loss and the cross-entropy
    calls = []
    monkeypatch.setattr(m.embedding_loss_criterion, "forward", lambda e, t, od: (calls.append("embedding"), od.update(
        {"optimization_losses": {"embedding_loss": torch.tensor(1.)}, "others": {}})))
    monkeypatch.setattr(losses.CrossEntropyLoss, "forward_with_foreground", lambda self, x, t, od: calls.append(("combined", tuple(x.shape))))
    monkeypatch.setattr(losses.CrossEntropyLoss, "forward", lambda self, x, t, od: calls.append(("sliced", tuple(x.shape))))
    out = m.compute_losses(torch.zeros(1, 7, 8, 4, 6), torch.zeros(1, 8, 4, 4, 6), [])
    assert calls == ["embedding", ("combined", (1, 8, 4, 4, 6))]
    assert set(out) == {"inference", "optimization_losses", "others"}
    # InferenceModel builds on the same model and sees no difference
    im = InferenceModel()
    assert type(im._model) is model_builder.TrainingModel and im.mask_scale == 4 and im.has_semseg_head


def test_loss_at_full_res_is_refused(kitti_cfg):
    from stemseg_amd.modeling import model_builder
    kitti_cfg.TRAINING.LOSS_AT_FULL_RES = True
    m = model_builder.build_model()
    assert m.output_resize_scale == 4.0
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="LOSS_AT_FULL_RES"):
        m.resize_masks([])
    with pytest.raises(NotImplementedError, match="LOSS_AT_FULL_RES"):
        m(torch.zeros(1, 8, 3, 64, 64), [])


def test_model_without_semseg_head_has_no_semseg_criterion():
    from stemseg_amd import config
    from stemseg_amd.modeling import model_builder
    config.load_preset("davis")
    config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
    try:
        m = model_builder.build_model()
        assert m.semseg_head is None and m.semseg_loss_criterion is None and m.seediness_head is not None
        assert torch.equal(m.embedding_loss_criterion.free_dim_bandwidths, 1. / torch.tensor([[0.3, 0.3]]) ** 2)
        assert not any("criterion" in k for k in m.state_dict())      # weights only, as before (see TrainingModel's docstring)
    finally:
        config.load_preset("defaults")
