"""GPU tests of decoder training on a frozen backbone: SqueezeExpandTrunk.forward_trainable (Conv3dFunction -> GnReluPoolFunction per
stage, then the folded tail) against the fp64 restatement of the whole reference decoder (tests/conv3d_backward_oracle.py), and
TrainingModel.forward behind the switch ``train_decoders``.

Bound of a parameter's gradient: 4 x max(the oracle's own fp32-versus-fp64 spread, 2^-24) on the max norm relative to max|g|; with the
decoder in 'f16x3' the fp64 oracle's own change when every convolution operand is rounded to the 22-bit significand that mode keeps
enters the max as well (the forward's convolutions see their operands so; the backward never runs in f16x3).  The features are the
first of seeds 0..15 whose pre-ReLU values all keep 2e-5 from 0 in the fp64 oracle (tests/test_conv3d_backward_host.py checks that
there is one): no sign of a ReLU is in doubt.  Every gradient prints spread, bound and device error before the test asserts.
"""
import functools

import numpy as np
import pytest
import torch

from tests import conv3d_backward_oracle as CO
from tests import decoder_tail_oracle as TO

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


@functools.lru_cache(maxsize=None)
def _case(kind, T):
    """The decoder, its input and the oracle's gradients (fp32, fp64, fp64 on rounded operands): computed once, shared by the precisions."""
    m = CO.init_decoder(kind, T).cuda()
    seed, margin, tried = CO.select_seed(kind, T, m)
    print("%s T %d: seed %d, min |pre-ReLU| %.2e" % (kind, T, seed, margin))
    feats = CO.features(T, seed)
    c = m._packed()
    acts = m._train_acts()
    act = list(c["act"]) if acts is None else list(acts)
    H4, W4 = CO.MAP_SIZES[3]
    grids = tuple(None if v is None else v.cpu() for v in m._grid(c, T, H4, W4, torch.device("cuda", torch.cuda.current_device())))
    up = torch.randn((len(act), T, H4, W4), generator=torch.Generator().manual_seed(7))
    grad = lambda dt, rounded=False: CO.decoder_gradients(m, kind, T, feats, up, act, list(c["axes"]), grids, dt, rounded)[0]
    return dict(m=m, feats=feats, acts=acts, up=up, g32=grad(torch.float32), g64=grad(torch.float64), g22=grad(torch.float64, True))


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("T", [4, 8])
@pytest.mark.parametrize("kind", ["embedding", "semseg"])
def test_every_decoder_gradient_vs_the_reference_decoder(hip, kind, T, precision):
    """in = inter = 32 channels, GroupNorm(8), a 4x map of 8 x 16 (the 32x map is 1 x 2), T 4 and 8.  forward_trainable within 4e-6 of
    run_hip (the fold figure), then the gradient of every parameter of the decoder -- the seven convolutions' weights and biases, every
    GroupNorm's affine parameters, conv_16 / conv_8 / conv_4, the heads -- against the oracle, and the same bits on a second pass."""
    k = _case(kind, T)
    m = k["m"]
    m.precision = precision
    for p in m.parameters():
        p.grad = None
    feats = [f.cuda() for f in k["feats"]]
    ref = m.run_hip(feats, 0, k["acts"])
    out = m.forward_trainable(feats, k["acts"])
    diff = float(((out.detach() - ref).abs() / ref.abs().clamp(min=1.0)).max())
    print("%s T %d %s: forward_trainable vs run_hip, max |diff| / max(1, |x|) %.2e" % (kind, T, precision, diff))
    assert out.shape == ref.shape and diff <= 4e-6
    out.backward(k["up"].cuda())
    got = {n: host(p.grad) for n, p in m.named_parameters() if p.grad is not None}
    assert set(got) == set(k["g64"]) == {n for n, _ in m.named_parameters()}, sorted(set(got) ^ set(k["g64"]))
    bad = []
    for n in sorted(got):
        r64 = k["g64"][n]
        spread, err = TO.max_norm_err(k["g32"][n], r64), TO.max_norm_err(got[n], r64)
        change = TO.max_norm_err(k["g22"][n], r64) if precision == "f16x3" else 0.0
        b = TO.bound(max(spread, change), r64)
        print("%s T %d %s %-28s spread %.2e 22-bit change %.2e bound %.2e device %.2e" % (kind, T, precision, n, spread, change, b, err))
        if not err <= b:
            bad.append((n, err, b))
    for p in m.parameters():
        p.grad = None
    out2 = m.forward_trainable(feats, k["acts"])
    out2.backward(k["up"].cuda())
    assert torch.equal(out2, out)
    assert all(np.array_equal(host(p.grad), got[n]) for n, p in m.named_parameters()), "reruns differ"
    assert not bad, bad


@pytest.fixture(scope="module")
def trained(hip):
    """kittimots preset, R-50, one clip of 8 frames of 96 x 128; backbone frozen, ``train_decoders`` on; forward, the summed losses'
    backward, one step of the reference's optimiser (SGD, INITIAL_LR 1e-3: config/kitti_mots_*.yaml), the no-grad forward before and
    after, and ``forward_trainable`` of every head by hand on the stepped weights.  Computed once for the tests below."""
    from stemseg_amd import config
    from stemseg_amd.modeling.model_builder import build_model
    from stemseg_amd.utils.constants import ModelOutput
    from tests import semseg_loss_oracle as SO
    from tests import synth
    E, S = ModelOutput.EMBEDDINGS, ModelOutput.SEMSEG_MASKS
    r = {}
    try:
        config.load_preset("kittimots")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        m = build_model()
        sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], 11)
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()})
        m = m.cuda().eval()
        dec = m.decoder_parameters()
        for p in m.parameters():
            p.requires_grad_(False)
        for p in dec.values():
            p.requires_grad_(True)
        frames = (torch.from_numpy(synth.synth_frames(8, 96, 128, seed=3).astype(np.float32)).permute(0, 3, 1, 2) -
                  torch.tensor(config.cfg.INPUT.IMAGE_MEAN)[None, :, None, None])[None].cuda()
        _, masks, ig, cat = SO.make_sample(np.random.default_rng(5), 1, 8, 96, 128, (1, 2, 2))
        raw = lambda: [{"masks": torch.from_numpy(masks).cuda(), "ignore_masks": torch.from_numpy(ig).cuda(), "category_ids": torch.from_numpy(cat).cuda()}]
        try:
            m(frames, raw())                                     # the switch is off by default
        except NotImplementedError as e:
            r["refusal"] = str(e)
        m.train_decoders = True

        def by_hand(run):
            feats = m.run_backbone(frames)
            stack = lambda s: [feats[k].reshape((1, 8) + tuple(feats[k].shape[1:])).permute(0, 2, 1, 3, 4) for k in s]
            sem = run(m.semseg_head)([f[0] for f in stack(m.semseg_feature_map_scale)[::-1]]).detach()[None].permute(0, 2, 1, 3, 4)
            m.embedding_head.fuse_bandwidth_activation, fused = False, m.embedding_head.fuse_bandwidth_activation
            try:
                emb = run(m.embedding_head)([f[0] for f in stack(m.embedding_head_feature_map_scale)], m.embedding_head._acts()).detach()[None]
            finally:
                m.embedding_head.fuse_bandwidth_activation = fused
            if m.seediness_head is not None:
                emb = torch.cat((emb, run(m.seediness_head)([f[0] for f in stack(m.seediness_head_feature_map_scale)]).detach()[None]), 1)
            return {"embeddings": emb, "semseg": sem}

        rel = lambda a, b: float(((a - b).abs() / b.abs().clamp(min=1.0)).max()) if a.shape == b.shape else float("inf")
        with torch.no_grad():
            before = m(frames, raw())[ModelOutput.INFERENCE]
        hand = by_hand(lambda h: h.forward_trainable)
        r["diff_before"] = {"embeddings": rel(before[E], hand["embeddings"]), "semseg": rel(before[S], hand["semseg"])}
        tail = by_hand(lambda h: h.forward_tail_trainable)
        r["tail_path_vs_full_path"] = {k: rel(tail[k], hand[k]) for k in hand}
        out = m(frames, raw())
        loss = sum(out["optimization_losses"].values())
        r["loss_ok"] = bool(loss.requires_grad and torch.isfinite(loss))
        loss.backward()
        named = dict(m.named_parameters())
        r["decoder_keys"] = set(dec)
        r["filled"] = {k for k, p in named.items() if p.grad is not None}
        r["finite"] = all(bool(torch.isfinite(named[k].grad).all()) for k in r["filled"])
        r["all_zero"] = [k for k in r["filled"] if not named[k].grad.any()]
        torch.optim.SGD(list(dec.values()), lr=1e-3).step()
        with torch.no_grad():
            after = m(frames, raw())[ModelOutput.INFERENCE]
        r["moved"] = not torch.equal(after[E], before[E]) and not torch.equal(after[S], before[S])
        hand = by_hand(lambda h: h.forward_trainable)
        r["diff_after"] = {"embeddings": rel(after[E], hand["embeddings"]), "semseg": rel(after[S], hand["semseg"])}
        print("loss %.6f; %d decoder parameters, %d gradients, all-zero: %s" % (float(loss.detach()), len(dec), len(r["filled"]), r["all_zero"]))
        print("no-grad forward vs forward_trainable, max |diff| / max(1, |x|): before the step %s, after %s; forward_tail_trainable vs "
              "forward_trainable %s" % (r["diff_before"], r["diff_after"], r["tail_path_vs_full_path"]))
    finally:
        config.load_preset("defaults")
    return r


def test_training_model_fills_exactly_the_decoder_gradients(trained):
    """Off by default: the old refusal.  With ``train_decoders`` on and the backbone frozen, forward and the summed losses' backward fill
    .grad on exactly ``decoder_parameters()``, every gradient finite, none on the backbone."""
    assert "decoder and encoder backward passes are not implemented" in trained["refusal"]
    assert trained["loss_ok"]
    assert trained["filled"] == trained["decoder_keys"], sorted(trained["filled"] ^ trained["decoder_keys"])
    assert not any(k.startswith("backbone.") for k in trained["filled"]) and trained["finite"]


def test_after_an_optimiser_step_the_forward_follows_the_weights(trained):
    """After one SGD step the no-grad forward differs from before and equals ``forward_trainable`` on the stepped weights within 4e-6 of
    max(1, |x|), so the packed-weight cache followed the update.  (``forward_trainable`` hands its convolutions the inference decoder's
    split-K scratch and so takes its K partition: measured, the two agree bit for bit, before and after the step.  Without the scratch the
    distance at this model's 256 / 128-channel widths is 4e-6 ... 8e-6, which is what ``forward_tail_trainable`` shows against ``run_hip``.)"""
    assert trained["moved"]
    assert max(trained["diff_before"].values()) <= 4e-6, trained["diff_before"]
    assert max(trained["diff_after"].values()) <= 4e-6, trained["diff_after"]
