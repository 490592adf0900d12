"""stemseg_amd.training.main.Trainer on the small models of tests/test_gpu_body_backward.py (kittimots preset, R-50, one clip of
8 x 96 x 128) and tests/test_gpu_wide_heads.py (ytvis preset): the loop with gradient accumulation, the device step against torch.optim.SGD
fed the device's own accumulated gradients (so that only the step is compared), the packed-operand caches after a step, the scheduler,
checkpoint resume, the clip, and the wide head.  The first iteration is also run by a twin: a second model with the same weights, a
hand-written loop over the same two batches and torch.optim.SGD.  Each leg is run once, in a module fixture of its own."""
import contextlib
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests import decoder_tail_oracle as TO
from tests.test_gpu_body_backward import _inputs

pytestmark = pytest.mark.gpu

OPTS = NS(save_interval=10 ** 6, display_interval=1, summary_interval=1, ckpts_to_keep=2)
HYPER = dict(lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip
    hip.require_gpu()
    return hip


def _training_cfg(**over):
    """The reference's defaults (SGD 0.9, Nesterov, 1e-4, lr 1e-3, batch 2 at one sample per pass: interval 2), the rate dropping after
    the second step."""
    from stemseg_amd import config
    t = NS(**vars(config.make_cfg().TRAINING))
    t.LR_DECAY_TYPE, t.LR_DECAY_STEPS, t.LR_DECAY_FACTOR, t.MAX_ITERATIONS = "step", [2], 0.1, 1000
    for k, v in over.items():
        setattr(t, k, v)
    return t


class Batches(object):
    """An iterable of (image_seqs, targets, meta_info) with fresh target dicts every time (the model resizes the masks in place)."""

    def __init__(self, items):
        self.items = items

    def __iter__(self):
        for frames, raw in self.items:
            yield frames.cpu(), raw(), [{}]            # (host tensors: the loop moves them)


def _two_batches(frames, raw):
    def flipped():
        t = raw()[0]
        return [{"masks": t["masks"].flip(1), "ignore_masks": t["ignore_masks"].flip(0), "category_ids": t["category_ids"]}]
    return [(frames, raw), (frames.flip(1), flipped)]


def _build(initial_state=None, seed=11):
    from stemseg_amd.modeling.model_builder import build_model
    from tests import synth
    m = build_model()
    if initial_state is None:
        sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], seed)
        initial_state = {k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()}
    m.load_state_dict(initial_state)
    return m.cuda().eval()


class Snapshot(object):
    """A step pre-hook: the parameters and the accumulated gradients as the step finds them."""

    def __init__(self, trainer):
        self.taken, self.model = [], trainer.model
        trainer.optimizer.register_step_pre_hook(self)

    def __call__(self, optimizer, args, kwargs):
        self.taken.append({k: (p.detach().cpu().clone(), None if p.grad is None else p.grad.detach().cpu().clone())
                           for k, p in self.model.named_parameters()})


def _trainer(tmp, model, cfg, restore=None, **kw):
    from stemseg_amd.training.main import Trainer
    said = []
    log = NS(info=said.append, debug=said.append)
    t = Trainer(cfg, str(tmp), NS(restore_session=restore, initial_ckpt=None), log, model=model, **kw)
    t.said = said
    return t


def _run(trainer, items):
    trainer.data_loader = Batches(items)
    trainer.start(OPTS)
    torch.cuda.synchronize()


def _cpu_sgd(before, dtype, scale=None):
    """torch.optim.SGD on the CPU in ``dtype`` over {name: (p, g)} -> {name: p after one step}."""
    names = [k for k, (p, g) in before.items() if g is not None]
    params = [torch.nn.Parameter(before[k][0].to(dtype).clone()) for k in names]          # (a copy: the step writes in place)
    for p, k in zip(params, names):
        g = before[k][1].to(dtype)
        p.grad = g * torch.tensor(np.float32(scale)).to(dtype) if scale is not None else g
    torch.optim.SGD(params, **HYPER).step()
    return {k: p.detach().double().numpy() for k, p in zip(names, params)}


def _by_the_rule(name, after, before, scale=None):
    r32, r64 = _cpu_sgd(before, torch.float32, scale), _cpu_sgd(before, torch.float64, scale)
    bad = []
    for k in r64:
        TO.check(name, k, after[k].double().numpy(), r32[k], r64[k], bad)
    return bad, set(r64)


@contextlib.contextmanager
def _preset(name):
    from stemseg_amd import config
    try:
        config.load_preset(name)
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        yield config
    finally:
        config.load_preset("defaults")


def _named(model, grads=False):
    return {k: (p.grad if grads else p).detach().cpu().clone() for k, p in model.named_parameters() if not grads or p.grad is not None}


@pytest.fixture(scope="module")
def kitti(hip):
    """The start weights and the two batches every kittimots leg shares."""
    with _preset("kittimots"):
        m = _build()
        frames, raw = _inputs(m, 8, 96, 128)
        return NS(initial={k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, frames=frames, raw=raw, items=_two_batches(frames, raw))


@pytest.fixture(scope="module")
def twin(hip, kitti):
    """The loop written out by hand on a second model with the same weights: per batch forward, the summed optimisation losses over 2,
    backward; then ONE torch.optim.SGD step.  Leaves the accumulated gradients, and the weights before and after the stock step."""
    from stemseg_amd.training import configure_trainable
    with _preset("kittimots"):
        m = configure_trainable(_build(kitti.initial))
        opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], **HYPER)
        before = _named(m)
        for frames, raw in kitti.items:
            out = m(frames, raw())
            (sum(out["optimization_losses"].values()) / 2).backward()
        grads = _named(m, grads=True)
        opt.step()
        torch.cuda.synchronize()
        return NS(before=before, grads=grads, after=_named(m))


@pytest.fixture(scope="module")
def runs(hip, kitti, tmp_path_factory):
    """One Trainer: iteration 1, the packed caches, a checkpoint, iterations 2 and 3; then a second Trainer resumed from the checkpoint."""
    from stemseg_amd.utils.constants import ModelOutput
    E = ModelOutput.EMBEDDINGS
    r = {}
    frames, raw, items, initial = kitti.frames, kitti.raw, kitti.items, kitti.initial
    with _preset("kittimots"):
        m = _build(initial)
        tr = _trainer(tmp_path_factory.mktemp("session"), m, _training_cfg())
        r["optimizer_type"], r["switches"] = type(tr.optimizer).__name__, (m.train_decoders, m.train_fpn, m.train_body, m.train_wide_head)
        r["trainable"] = {k for k, p in m.named_parameters() if p.requires_grad}
        r["expected_trainable"] = set(m.decoder_parameters()) | set(m.fpn_parameters()) | set(m.body_parameters(2))
        snap = Snapshot(tr)
        _run(tr, items)
        r["iterations_after_first"], r["lr_after_first"] = tr.elapsed_iterations, tr.optimizer.param_groups[0]["lr"]
        r["before"], r["after"] = snap.taken[0], _named(m)
        r["grads_cleared"] = all(p.grad is None for p in m.parameters())
        r["first_point"] = dict(tr.logger.last_point)
        # the packed caches: the trained model's no-grad forward against a fresh model loaded from its state dict
        with torch.no_grad():
            out_trained = m(frames, raw())[ModelOutput.INFERENCE][E].clone()
            fresh = _build({k: v.detach().clone() for k, v in m.state_dict().items()})
            r["fresh_equal"] = torch.equal(out_trained, fresh(frames, raw())[ModelOutput.INFERENCE][E])
            r["moved"] = not torch.equal(out_trained, _build(initial)(frames, raw())[ModelOutput.INFERENCE][E])
            del fresh
        ckpt = tr.backup_session()
        r["ckpt_keys"] = sorted(torch.load(ckpt, map_location="cpu").keys())
        r["logger_keys"] = sorted(torch.load(ckpt, map_location="cpu")["logger"].keys())
        lrs, points = [], []
        for k in range(2):
            _run(tr, items)
            lrs.append(tr.optimizer.param_groups[0]["lr"])
            points.append(dict(tr.logger.last_point))
            if k == 0:
                r["straight_after_second"] = _named(m)                   # the uninterrupted run
        r["lrs"], r["points"], r["uploads"], r["straight_iterations"] = lrs, points, tr.optimizer.table_uploads, tr.elapsed_iterations
        # resume: a new Trainer on a new model from the checkpoint, iteration 2 on the same batches
        tr2 = _trainer(tmp_path_factory.mktemp("resumed"), _build(initial), _training_cfg(), restore=ckpt)
        r["resumed_iterations"], r["resumed_lr"] = tr2.elapsed_iterations, tr2.optimizer.param_groups[0]["lr"]
        _run(tr2, items)
        r["resumed_after_second"] = _named(tr2.model)
        for it in (5, 6, 7):
            tr2.elapsed_iterations = it
            tr2.backup_session()
        tr2.prune_checkpoints(2)
        r["kept"] = sorted(f for f in os.listdir(tr2.model_save_dir) if f.endswith(".pth"))
    return r


@pytest.fixture(scope="module")
def fpn_only(hip, kitti):
    """One forward and backward, every gradient but the FPN's dropped, one DeviceSGD step over all parameters."""
    from stemseg_amd.training import DeviceSGD, configure_trainable
    from stemseg_amd.utils.constants import ModelOutput
    E = ModelOutput.EMBEDDINGS
    frames, raw = kitti.frames, kitti.raw
    with _preset("kittimots"):
        m = configure_trainable(_build(kitti.initial))
        bb = m.backbone
        with torch.no_grad():
            out_before = m(frames, raw())[ModelOutput.INFERENCE][E].clone()
        (w, keep), n_body = bb._packed[bb.precision][1], bb._packed[bb.precision][2]
        body_ids = [id(t) for t in keep[:n_body]]
        sum(m(frames, raw())["optimization_losses"].values()).backward()
        for k, p in m.named_parameters():
            if not k.startswith("backbone.fpn."):
                p.grad = None
        DeviceSGD(m.parameters(), **HYPER).step()
        with torch.no_grad():
            out_after = m(frames, raw())[ModelOutput.INFERENCE][E]
        (w2, keep2), n_body2 = bb._packed[bb.precision][1], bb._packed[bb.precision][2]
        return NS(moved=not torch.equal(out_after, out_before),
                  body_kept=w2 is w and n_body2 == n_body and [id(t) for t in keep2[:n_body]] == body_ids)


@pytest.fixture(scope="module")
def clip(hip, kitti, tmp_path_factory):
    with _preset("kittimots"):
        m = _build(kitti.initial)
        tr = _trainer(tmp_path_factory.mktemp("clip"), m, _training_cfg(CLIP_GRADIENTS=True), max_norm=0.01)
        snap = Snapshot(tr)
        _run(tr, kitti.items)
        return NS(before=snap.taken[0], after=_named(m), norm=float(tr.last_grad_norm), logged=tr.logger.last_point.get("grad_norm"))


@pytest.fixture(scope="module")
def ytvis(hip, tmp_path_factory):
    """The ytvis-preset small model of tests/test_gpu_wide_heads.py through one Trainer iteration (batch size 1)."""
    from tests import semseg_loss_oracle as SO
    from tests import synth
    with _preset("ytvis") as config:
        m = _build()
        fr = (torch.from_numpy(synth.synth_frames(8, 96, 128, seed=3).astype(np.float32)).permute(0, 3, 1, 2) -
              torch.tensor(config.cfg.INPUT.IMAGE_MEAN)[None, :, None, None])[None]
        _, masks, ig, cat = SO.make_sample(np.random.default_rng(5), 1, 8, 96, 128, (1, 17, 40))
        raw = lambda: [{"masks": torch.from_numpy(masks), "ignore_masks": torch.from_numpy(ig), "category_ids": torch.from_numpy(cat)}]
        before = _named(m)
        tr = _trainer(tmp_path_factory.mktemp("ytvis"), m, _training_cfg(BATCH_SIZE=1))
        r = NS(wide=m.train_wide_head, n_out=m.semseg_head.out_channels)
        _run(tr, [(fr, raw)])
        r.iterations, r.point = tr.elapsed_iterations, dict(tr.logger.last_point)
        r.moved = {k for k, p in m.named_parameters() if not torch.equal(p.detach().cpu(), before[k])}
        r.trainable = {k for k, p in m.named_parameters() if p.requires_grad}
        r.finite = all(bool(torch.isfinite(p).all()) for p in m.parameters())
        return r


def test_one_iteration_at_interval_two_matches_the_twin(runs, twin):
    """Trainer picks DeviceSGD and the reference's trainable set; after two sub-iterations one step has run.  The twin -- same weights,
    the same two batches through a hand-written loop at loss / 2, torch.optim.SGD (0.9, Nesterov, 1e-4) -- must end where the Trainer
    ends: both are held to the rule against the CPU optimiser in fp64 fed the TWIN's accumulated gradients, the spread being the same in
    fp32.  A Trainer that dropped a batch, cleared the gradients between sub-iterations or divided wrongly would miss it by the size of
    the update."""
    assert runs["optimizer_type"] == "DeviceSGD" and runs["switches"] == (True, True, True, False)
    assert runs["trainable"] == runs["expected_trainable"] and len(runs["trainable"]) == 42 + 16 + 67
    assert runs["iterations_after_first"] == 1 and runs["grads_cleared"]
    assert set(twin.grads) == runs["trainable"]
    assert all(torch.equal(twin.before[k], runs["before"][k][0]) for k in twin.before), "the twin did not start from the same weights"
    oracle_in = {k: (twin.before[k], twin.grads.get(k)) for k in twin.before}
    bad, stepped = _by_the_rule("trainer vs twin's gradients", runs["after"], oracle_in)
    assert stepped == runs["trainable"] and not bad, bad
    bad, _ = _by_the_rule("twin (stock SGD)", twin.after, oracle_in)
    assert not bad, bad
    # the gradients themselves: what the Trainer accumulated is what the hand-written loop accumulated
    worst = max(TO.max_norm_err(runs["before"][k][1].double().numpy(), twin.grads[k].double().numpy()) for k in twin.grads)
    print("largest distance between the Trainer's and the twin's accumulated gradients: %.3e of max |g|" % worst)
    assert worst <= 4 * TO.FP32_ROUNDING, "the Trainer's accumulated gradients are not the hand-written loop's"
    # ... and half an update off is far outside the rule: the check above can tell
    after, before = runs["after"], runs["before"]
    moved = {k for k in after if not torch.equal(after[k], before[k][0])}
    assert moved == runs["trainable"], sorted(moved ^ runs["trainable"])[:5]
    pt = runs["first_point"]
    assert pt["iteration"] == 1 and all(np.isfinite(v) for v in pt.values()) and "embedding_loss" in pt


def test_packed_caches_follow_the_step(runs, fpn_only):
    """The kernel writes the parameters through raw pointers; without the version bump the packed operands would be stale and the trained
    model would still compute with the old weights."""
    assert runs["moved"] and runs["fresh_equal"]
    assert fpn_only.moved and fpn_only.body_kept, "a step on the FPN alone re-packed the body (or changed nothing)"


def test_two_further_iterations_follow_the_scheduler(runs):
    assert runs["lr_after_first"] == HYPER["lr"]
    assert np.allclose(runs["lrs"], [HYPER["lr"] * 0.1, HYPER["lr"] * 0.1], rtol=1e-12)          # MultiStepLR: down by 0.1 after step 2
    for k, pt in enumerate(runs["points"]):
        assert pt["iteration"] == k + 2 and all(np.isfinite(v) for v in pt.values()), pt
    # fresh momentum buffers, initialised ones, and (gradients re-allocated by zero_grad) at most one more table per step
    assert 2 <= runs["uploads"] <= 3


def test_checkpoint_resume_gives_the_uninterrupted_bits(runs):
    assert runs["ckpt_keys"] == ["iterations", "logger", "lr_scheduler", "model", "optimizer"]
    assert runs["logger_keys"] == ["_TrainingLogger__latest_iteration_num", "_TrainingLogger__latest_timestamp", "_TrainingLogger__pause_duration",
                                   "_TrainingLogger__train_start_time", "total_iterations"]
    assert runs["resumed_iterations"] == 1 and runs["resumed_lr"] == HYPER["lr"] and runs["straight_iterations"] == 3
    a, b = runs["resumed_after_second"], runs["straight_after_second"]
    differ = [k for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]
    assert not differ, differ[:5]
    assert any(not torch.equal(a[k], runs["after"][k]) for k in a)
    assert runs["kept"] == ["000006.pth", "000007.pth"]


def test_clip_scales_the_update_by_coef(clip):
    norm, max_norm = clip.norm, 0.01
    before, after = clip.before, clip.after
    exact = float(np.sqrt(sum(float((g.double() ** 2).sum()) for p, g in before.values() if g is not None)))
    print("gradient norm %.6g (fp64 on the host %.6g), max_norm %g" % (norm, exact, max_norm))
    assert norm > max_norm and abs(norm - exact) <= 1e-12 * exact and clip.logged == norm
    coef = np.float32(min(1.0, max_norm / (exact + 1e-6)))
    bad, _ = _by_the_rule("clip", after, before, scale=coef)
    assert not bad, bad
    # ... and the unclipped oracle is far off: the clip really acted
    r32, r64 = _cpu_sgd(before, torch.float32), _cpu_sgd(before, torch.float64)
    k = max(r64, key=lambda n: np.abs(r64[n] - before[n][0].double().numpy()).max())
    _, bound, err = TO.check("unclipped", k, after[k].double().numpy(), r32[k], r64[k], [])
    assert err > 10 * bound


def test_ytvis_preset_trains_through_the_wide_head(ytvis):
    assert ytvis.n_out == 42 and ytvis.wide is True
    assert ytvis.iterations == 1 and ytvis.finite and all(np.isfinite(v) for v in ytvis.point.values())
    assert ytvis.moved == ytvis.trainable and any(k.startswith("semseg_head.") for k in ytvis.moved)
