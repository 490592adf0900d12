"""GPU tests of the training targets, the semseg cross-entropy and the foreground loss (csrc/semseg_loss.hip behind hip.prepare_targets,
stemseg_amd.modeling.losses.CrossEntropyLoss and TrainingModel): prepared targets bit-exact against the goldens of the reference's own
resize_masks and against the oracle (tests/semseg_loss_oracle.py); loss values and gradients against the goldens and the fp64 oracle on
every fixture, at T = 8 on 120 x 216 maps with 3, 4 and 42 channels and at N = 2; each loss's gradient on its own and both together;
through the permuted [N, T, cls, H, W] view; the all-ignored sample (NaN); a target id outside the class channels; bit-identical runs;
TrainingModel.compute_losses and TrainingModel.forward under no_grad against the two loss oracles.

Bounds, per case (the rule of tests/test_gpu_embedding_loss.py).  The yardstick is the reference arithmetic's own fp32-versus-fp64
spread ON THE SAME INPUT: every test runs the oracle in fp32 and in fp64 on its input and allows the device FACTOR = 4 x that case's own
spread, no more; on the fixtures the reference's golden values against the fp64 oracle give the spread for the comparison with the
goldens.  Errors are relative for a loss and max-norm over every finite element, relative to max|g|, for a gradient.  One floor, from
the number format: the device returns fp32 losses and gradient elements, and rounding a value to fp32 alone moves it by up to
2^-24 = 6.0e-8 relative, so a smaller spread counts as 2^-24.  A term that is exactly zero in the oracle must be exactly zero on the
device.  Prepared targets are integers: identical or wrong.

The per-case table of measured spreads and device errors is in DESIGN.md section 9f.
"""
import os

import numpy as np
import pytest
import torch

from tests import loss_oracle as LO
from tests import semseg_loss_oracle as SO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = SO.load_fixtures(os.path.join(ROOT, "tests", "golden", "semseg_loss.npz"))
FACTOR = 4                     # the device may be this many times the case's own fp32-vs-fp64 spread away from the fp64 oracle
FP32_ROUNDING = 2.0 ** -24     # rounding a result to fp32: the least spread a case is credited with (see the header)
NAMES = ("cross-entropy", "foreground")


def _cuda(targets):
    return [{k: v.cuda() for k, v in t.items()} for t in targets]


def device_components(x, prepared, K, has_fg):
    """-> (losses float64 numpy [2], the two component gradients as float64 numpy) through the autograd function, on the [N, C, T, h, w]
    tensor as the decoder leaves it."""
    from stemseg_amd.modeling.losses.cross_entropy import SemsegLossFunction
    xx = x.cuda().requires_grad_(True)
    t = _cuda(prepared)
    comps = SemsegLossFunction.apply(xx, [a["semseg_masks"] for a in t], [a["ignore_masks"] for a in t], K, has_fg)
    grads = []
    for c in comps:
        g, = torch.autograd.grad(c, xx, retain_graph=True)
        grads.append(g.double().cpu().numpy())
    return np.array([float(c.detach()) for c in comps]), grads


def _rel(a, b):
    if np.isnan(b):
        return 0.0 if np.isnan(a) else float("inf")
    return abs(a - b) / abs(b) if b else abs(a)


def _grad_err(g, ref):
    """max-norm error over the finite elements of ``ref`` relative to their max; inf if the NaN patterns differ."""
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(g), nan):
        return float("inf")
    if nan.all():
        return 0.0
    g, ref = g[~nan], ref[~nan]
    gmax = np.abs(ref).max()
    return np.abs(g - ref).max() / gmax if gmax else np.abs(g).max()


def _bound(spread):
    return FACTOR * max(spread, FP32_ROUNDING) if spread else 0.0      # (a zero spread is an exactly-zero term: the device must give 0 too)


def check_against_oracle(name, x, prepared, K, has_fg):
    losses, grads = device_components(x, prepared, K, has_fg)
    l32, g32 = SO.losses_and_grads(x, prepared, K, has_fg, torch.float32)
    l64, g64 = SO.losses_and_grads(x, prepared, K, has_fg, torch.float64)
    bad = []
    for k in range(2):
        lb, gb = _bound(_rel(l32[k], l64[k])), _bound(_grad_err(g32[k], g64[k]))
        rel, gerr = _rel(losses[k], l64[k]), _grad_err(grads[k], g64[k])
        print("%s %-13s loss %.9g (fp64 %.9g) spread %.2e rel %.2e (bound %.2e) | grad spread %.2e err / max|g| %.2e (bound %.2e)"
              % (name, NAMES[k], losses[k], l64[k], _rel(l32[k], l64[k]), rel, lb, _grad_err(g32[k], g64[k]), gerr, gb))
        if not rel <= lb:
            bad.append((NAMES[k], "loss", rel, lb))
        if not gerr <= gb:
            bad.append((NAMES[k], "grad", gerr, gb))
    assert not bad, bad
    return losses, grads, (l64, g64)


# ------------------------------------------------------------------------------------------------ targets
@pytest.mark.parametrize("name", sorted(SO.FIXTURE_CASES))
def test_prepared_targets_bit_exact_vs_reference_and_oracle(name):
    from stemseg_amd import hip
    f = FIXTURES[name]
    for raw, want, mine in zip(f["targets"], f["prepared"], SO.prepared(f["targets"])):
        m, ig, sem, flag = hip.prepare_targets(raw["masks"].cuda(), raw["ignore_masks"].cuda(), raw["category_ids"].cuda())
        assert int(flag) == 0 and m.dtype == ig.dtype == sem.dtype == torch.uint8
        for got, key in ((m, "masks"), (ig, "ignore_masks"), (sem, "semseg_masks")):
            assert torch.equal(got.cpu().long(), want[key].long()), (name, key, "reference")
            assert torch.equal(got.cpu().long(), mine[key].long()), (name, key, "oracle")


def test_prepared_targets_at_full_size_with_20_instances():
    from stemseg_amd import hip
    rng = np.random.default_rng(20)
    cats = tuple(int(c) for c in rng.integers(1, 41, 20))
    _, masks, ig, cat = SO.make_sample(rng, 1, 8, 480, 864, cats)
    want = SO.prepare_targets(torch.from_numpy(masks), torch.from_numpy(ig), torch.from_numpy(cat))
    got = hip.prepare_targets(torch.from_numpy(masks).cuda(), torch.from_numpy(ig).cuda(), torch.from_numpy(cat).cuda())
    assert int(got[3]) == 0 and tuple(got[0].shape) == (20, 8, 120, 216)
    for g, w in zip(got[:3], want):
        assert torch.equal(g.cpu().long(), w.long())
    assert want[2].max() > 1 and want[0].any() and want[1].any()
    # bool inputs give the same bytes; a category id that does not fit the uint8 mask raises the flag
    again = hip.prepare_targets(torch.from_numpy(masks).cuda().bool(), torch.from_numpy(ig).cuda(), cat.tolist())
    assert all(torch.equal(a, b) for a, b in zip(again[:3], got[:3]))
    assert int(hip.prepare_targets(torch.from_numpy(masks[:2]).cuda(), torch.from_numpy(ig).cuda(), [3, 256])[3]) == 1
    assert int(hip.prepare_targets(torch.from_numpy(masks[:2]).cuda(), torch.from_numpy(ig).cuda(), [-1, 3])[3]) == 1
    none = hip.prepare_targets(torch.zeros((0, 8, 480, 864), dtype=torch.uint8).cuda(), torch.from_numpy(ig).cuda(), [])
    assert none[0].numel() == 0 and torch.equal(none[1], got[1]) and not none[2].any()


# ------------------------------------------------------------------------------------------------ losses
@pytest.mark.parametrize("name", sorted(SO.FIXTURE_CASES))
def test_fixture_vs_reference_and_fp64_oracle(name):
    f = FIXTURES[name]
    losses, grads, (l64, g64) = check_against_oracle(name, f["x"], f["prepared"], f["K"], f["has_fg"])
    w = f["weight"]
    got = [losses[0], float(np.float32(losses[0]) * np.float32(w)), losses[1]]
    exact = [l64[0], l64[0] * w, l64[1]]
    for g, want, ex, what in zip(got, f["losses"], exact, ("semseg", "weighted semseg", "foreground")):
        rel, bound = _rel(g, want), _bound(_rel(want, ex))             # the reference's own distance from fp64 on this case
        print("%s %-15s device %.9g reference %.9g rel %.2e (bound %.2e)" % (name, what, g, want, rel, bound))
        assert rel <= bound, (what, g, want)
    gtotal, gt64 = grads[0] * w + grads[1], g64[0] * w + g64[1]
    gerr, bound = _grad_err(gtotal, f["grad"]), _bound(_grad_err(f["grad"], gt64))
    print("%s total grad vs reference: err / max|g| %.2e (bound %.2e)" % (name, gerr, bound))
    assert gerr <= bound


@pytest.mark.parametrize("name", sorted(SO.LARGE_CASES))
def test_large_vs_fp64_oracle(name):
    K, has_fg, _, _ = SO.LARGE_CASES[name]
    x, targets = SO.make_case(name, SO.LARGE_CASES)
    assert tuple(x.shape[1:]) == (K + has_fg, 8, 120, 216) or name == "n2_c4"
    _, grads, _ = check_against_oracle(name, x, SO.prepared(targets), K, has_fg)
    # one upstream weight zero: the other loss's channels get exact zeros
    assert not grads[1][:, :K].any() and (not has_fg or (not grads[0][:, K].any() and grads[1][:, K].any()))


def test_all_ignored_sample_gives_nan_where_the_reference_does():
    f = FIXTURES["ignore_all_n2"]
    losses, grads = device_components(f["x"], f["prepared"], f["K"], f["has_fg"])
    assert np.isnan(losses).all()
    K = f["K"]                                                         # sample 0: NaN in every element of the differentiated loss's channels,
    assert np.isnan(grads[0][0, :K]).all() and not grads[0][0, K].any()    # exact zeros in the other's (it is not in the graph), as autograd gives
    assert np.isnan(grads[1][0, K]).all() and not grads[1][0, :K].any()
    assert all(np.isfinite(g[1]).all() for g in grads)
    # an upstream of zero is not "absent": 0 * NaN = NaN in the reference's arithmetic, and here
    from stemseg_amd.modeling.losses.cross_entropy import SemsegLossFunction
    xx, t = f["x"].cuda().requires_grad_(True), _cuda(f["prepared"])
    ce, fg = SemsegLossFunction.apply(xx, [a["semseg_masks"] for a in t], [a["ignore_masks"] for a in t], K, True)
    (ce * 0 + fg).backward()
    assert torch.isnan(xx.grad[0]).all() and torch.isfinite(xx.grad[1]).all() and not xx.grad[1, :K].any()
    total = grads[0] * f["weight"] + grads[1]
    assert np.array_equal(np.isnan(total), np.isnan(f["grad"]))
    l64, g64 = SO.losses_and_grads(f["x"], f["prepared"], f["K"], f["has_fg"], torch.float64)
    gerr, bound = _grad_err(total, f["grad"]), _bound(_grad_err(f["grad"], g64[0] * f["weight"] + g64[1]))
    print("ignore_all_n2 finite part of the gradient vs reference: %.2e (bound %.2e)" % (gerr, bound))
    assert gerr <= bound


@pytest.mark.parametrize("name", ["k3_fg_n2_kitti", "k41_fg_ytvis_width", "odd_30x41_n2"])
def test_gradient_through_the_permuted_view(name):
    """The reference's call site hands [N, T, cls, H, W], a permuted view of the decoder's [N, cls, T, H, W]: same bits as the dense
    path, gradient in the leaf's layout -- and the same again when the leaf itself is dense in [N, T, cls, H, W]."""
    from stemseg_amd.modeling.losses import CrossEntropyLoss
    f = FIXTURES[name]
    assert f["weight"] == 1.0
    K, has_fg, t = f["K"], f["has_fg"], _cuda(f["prepared"])
    _, grads = device_components(f["x"], f["prepared"], K, has_fg)
    want = torch.from_numpy(grads[0] * f["weight"] + grads[1]).float()
    crit = CrossEntropyLoss()
    call = crit.forward_with_foreground if has_fg else crit.forward
    for leaf_layout in ("NCTHW", "NTCHW"):
        leaf = (f["x"] if leaf_layout == "NCTHW" else f["x"].permute(0, 2, 1, 3, 4).contiguous()).cuda().requires_grad_(True)
        view = leaf.permute(0, 2, 1, 3, 4) if leaf_layout == "NCTHW" else leaf
        assert view.shape[2] == K + has_fg and (leaf_layout == "NTCHW" or not view.is_contiguous())
        od = {"optimization_losses": {}, "others": {}}
        call(view, t, od)
        sum(od["optimization_losses"].values()).backward()
        g = leaf.grad if leaf_layout == "NCTHW" else leaf.grad.permute(0, 2, 1, 3, 4)
        assert leaf.grad.stride() == leaf.stride()
        assert torch.equal(g.cpu(), want), leaf_layout                  # (WEIGHT_SEMSEG is 1 in these cases: the same products)
    # the sliced call of the reference's tail (class channels only) reads the same memory through its strides
    if has_fg:
        leaf = f["x"].cuda().requires_grad_(True)
        od = {"optimization_losses": {}, "others": {}}
        crit(leaf.permute(0, 2, 1, 3, 4)[:, :, :K], t, od)
        od["others"]["semantic_segmentation_loss"].backward()
        assert torch.equal(leaf.grad[:, :K].cpu(), torch.from_numpy(grads[0]).float()[:, :K]) and not leaf.grad[:, K].any()


def test_foreground_loss_alone():
    from stemseg_amd.modeling.losses.cross_entropy import foreground_loss
    f = FIXTURES["k3_fg_n2_kitti"]
    losses, grads = device_components(f["x"], f["prepared"], f["K"], True)
    leaf = f["x"].cuda().requires_grad_(True)
    od = {"optimization_losses": {}, "others": {}}
    foreground_loss(leaf.permute(0, 2, 1, 3, 4)[:, :, f["K"]], _cuda(f["prepared"]), od)
    fg = od["optimization_losses"]["foreground"]
    fg.backward()
    assert float(fg.detach()) == losses[1] and torch.equal(leaf.grad.cpu(), torch.from_numpy(grads[1]).float())


def test_target_outside_the_class_channels_raises_and_the_process_goes_on():
    f = FIXTURES["k3_fg_n2_kitti"]
    bad = [dict(t) for t in f["prepared"]]
    bad[1]["semseg_masks"] = bad[1]["semseg_masks"].clone()
    bad[1]["semseg_masks"][0, 0, 0] = f["K"]
    with pytest.raises(ValueError, match="class id outside"):
        device_components(f["x"], bad, f["K"], f["has_fg"])
    bad[1]["semseg_masks"][0, 0, 0] = -3                               # int64 ids that do not fit the uint8 mask
    with pytest.raises(ValueError, match="class id outside"):
        device_components(f["x"], bad, f["K"], f["has_fg"])
    check_against_oracle("after the refusals", f["x"], f["prepared"], f["K"], f["has_fg"])


@pytest.mark.parametrize("name", ["k3_fg_n2_kitti", "train_c42"])
def test_two_runs_give_identical_bits(name):
    if name in FIXTURES:
        f = FIXTURES[name]
        x, prep, K, has_fg = f["x"], f["prepared"], f["K"], f["has_fg"]
    else:
        K, has_fg, _, _ = SO.LARGE_CASES[name]
        x, targets = SO.make_case(name, SO.LARGE_CASES)
        prep = SO.prepared(targets)
    from stemseg_amd.modeling.losses import CrossEntropyLoss
    t, runs = _cuda(prep), []
    for _ in range(2):
        xx = x.cuda().requires_grad_(True)
        od = {"optimization_losses": {}, "others": {}}
        CrossEntropyLoss().forward_with_foreground(xx.permute(0, 2, 1, 3, 4), t, od)
        sum(od["optimization_losses"].values()).backward()
        runs.append([od["optimization_losses"][k].detach() for k in sorted(od["optimization_losses"])] + [xx.grad])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------------------------------------ the model
def _model(preset):
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    from tests import synth
    config.load_preset(preset)
    config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
    m = build_model()
    sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], 11)      # random weights under the reference's keys
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()})
    return m.cuda().eval()


def _check_dict(name, out, emb, logits_nctHW, prepared, K, E, stds, weight=1.0):
    """The output dict against the two loss oracles (fp32 and fp64) run on ``emb`` and ``logits_nctHW``."""
    o32, o64 = [], []
    for dt, o in ((torch.float32, o32), (torch.float64, o64)):
        comps = [float(c) for c in LO.embedding_loss(emb.cpu(), prepared, E, stds, dt)]
        total, _ = LO.total_of(comps, [0, 0, 0])
        sl, _ = SO.losses_and_grads(logits_nctHW.cpu(), prepared, K, True, dt)
        o.extend(comps + [total, sl[0], sl[0] * weight, sl[1]])
    opt, others = out["optimization_losses"], out["others"]
    assert set(opt) == {"embedding_loss", "semantic_segmentation_loss", "foreground"}
    assert set(others) == {"lovasz_loss", "variance_smoothness_loss", "seediness_loss", "semantic_segmentation_loss"}
    got = [others["lovasz_loss"], others["variance_smoothness_loss"], others["seediness_loss"], opt["embedding_loss"],
           others["semantic_segmentation_loss"], opt["semantic_segmentation_loss"], opt["foreground"]]
    what = ("lovasz", "smoothness", "seediness", "embedding total", "semseg", "weighted semseg", "foreground")
    for g, a, b, w in zip(got, o32, o64, what):
        rel, bound = _rel(float(g), b), _bound(_rel(a, b))
        print("%s %-16s device %.9g fp64 %.9g rel %.2e (bound %.2e)" % (name, w, float(g), b, rel, bound))
        assert rel <= bound, (w, float(g), b)


@pytest.mark.parametrize("preset,K,E,stds,cats", [("ytvis", 41, 4, (0.3, 0.3), (40, 7, 23)), ("kittimots", 3, 3, (), (1, 2, 2))])
def test_compute_losses_gives_the_oracles_dictionary(preset, K, E, stds, cats):
    from stemseg_amd import config
    try:
        m = _model(preset)
        assert m.semseg_head.out_channels == K + 1
        config.cfg.TRAINING.LOSSES.WEIGHT_SEMSEG = 1.5
        rng = np.random.default_rng(K)
        raw, emb, logits = [], [], []
        for n in range(2):
            x, masks, ig, cat = SO.make_sample(rng, K + 1, 4, 96, 160, cats, overlap=bool(n))
            raw.append({"masks": torch.from_numpy(masks), "ignore_masks": torch.from_numpy(ig), "category_ids": torch.from_numpy(cat)})
            logits.append(x)
            emb.append(LO.make_sample(rng, E, len(stds), 4, 24, 40, len(cats))[0])
        emb, logits = torch.from_numpy(np.stack(emb)), torch.from_numpy(np.stack(logits))
        prepared = SO.prepared(raw)
        targets = m.resize_masks(_cuda(raw))
        for a, b in zip(targets, prepared):
            assert all(torch.equal(a[k].cpu().long(), b[k].long()) for k in ("masks", "ignore_masks", "semseg_masks"))
        out = m.compute_losses(emb.cuda(), logits.cuda().permute(0, 2, 1, 3, 4), targets)
        _check_dict(preset, out, emb, logits, prepared, K, E, stds, 1.5)
    finally:
        config.load_preset("defaults")


def test_training_model_forward_under_no_grad():
    from stemseg_amd import config
    from tests import synth
    try:
        m = _model("kittimots")
        frames = torch.from_numpy(synth.synth_frames(8, 96, 128, seed=3).astype(np.float32)).permute(0, 3, 1, 2) - \
            torch.tensor(config.cfg.INPUT.IMAGE_MEAN)[None, :, None, None]
        rng = np.random.default_rng(5)
        _, masks, ig, cat = SO.make_sample(rng, 1, 8, 96, 128, (1, 2, 2))
        raw = [{"masks": torch.from_numpy(masks), "ignore_masks": torch.from_numpy(ig), "category_ids": torch.from_numpy(cat)}]
        with pytest.raises(NotImplementedError, match="backward"):
            m(frames[None].cuda(), _cuda(raw))
        with torch.no_grad():
            out = m(frames[None].cuda(), _cuda(raw))
        emb, logits = out["inference"][("embeddings",)], out["inference"][("semseg_masks",)]
        assert tuple(emb.shape) == (1, 7, 8, 24, 32) and tuple(logits.shape) == (1, 8, 4, 24, 32)
        assert torch.isfinite(emb).all() and torch.isfinite(logits).all()
        _check_dict("forward", out, emb, logits.permute(0, 2, 1, 3, 4), SO.prepared(raw), 3, 3, ())
    finally:
        config.load_preset("defaults")
