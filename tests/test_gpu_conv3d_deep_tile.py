"""The deep 3x3x3 tile (conv_split_family.h DeepTiles::Y3Deep, tile_cfg hip.TILE_CFG_DEEP): f16x3, under the zero-temporal-halo promise, T == 8.

One workgroup owns all eight output planes of an 8 x 8 patch (wave wn = plane wn) and stages every input plane once.  The k order of every
accumulator is the block tile's, so the claim under test is EQUALITY of the raw convolution output with today's tiles (tile_cfg 6: the 20 x 24
block tile, 1: the 16 x 32 tile) on the same promised call.  Shapes are the smallest at which the tile can go wrong: Cin 4 and 12 (one and
three channel chunks), Cout 128 and 40 -- the API wants Cout % 32 == 0, so the ragged channel tile is 64 of 128 (the issue's "40" cannot be
fed) --, maps of 8 x 8 (one patch, every halo a map edge) and 16 x 24 (2 x 3 patches, interior halos both ways), one and two clips per launch
(stemseg_hip_conv3d_zero_t_halo_batch).  GroupNorm statistics are one slot per workgroup, i.e. another summation order than today's: they are
held to the fp64 statistics of the output at the bound of tests/test_gpu_parity.py (mean 2e-6, rstd 2e-6 relative) and to run-to-run equality.
A request the tile cannot serve (T = 4, a 12 x 24 map, bf16x6, a plan that splits K) plans and computes what the un-flagged call does."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as cc
from tests import synth

pytestmark = pytest.mark.gpu

T = 8
CINS, COUTS, MAPS = (4, 12), (128, 64), ((8, 8), (16, 24))


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _rand(shape, seed, scale=1.0):
    return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def _case(Cin, Cout, Tn, H, W, seed):
    return (_rand((Cin, Tn, H, W), seed), _rand((Cout, Cin, 3, 3, 3), seed + 1, 1.0 / np.sqrt(Cin * 27)), _rand((Cout,), seed + 2))


def _haloed(hip, x):
    Cn, Tn, H, W = x.shape
    buf, g = hip.alloc_padded(Cn, Tn, H, W)
    hip.copy_to_volume(dev(x), 0, hip.padded_interior_view(buf, g, Cn, Tn, H, W))
    return buf, hip.padded_halo_view(buf, g, Cn, Tn, H, W)


def _run(hip, vin, wp, b, shape, cfg, prec="f16x3", gn_groups=0, scratch=None):
    out = torch.full(shape, float("nan"), device="cuda")
    stats = hip.conv3d_zero_t_halo(vin, wp, b, hip.dense_volume(out), 3, cfg, scratch, precision=prec, gn_groups=gn_groups)
    torch.cuda.synchronize()
    return out, stats


def _plan(hip, Cin, Cout, Tn, H, W, cfg, prec="f16x3", scratch=0, gn_groups=0, plan_clips=0):
    gi, go = cc.halo_geom("k3", Cin, Tn, H, W), cc.dense_geom(Cout, Tn, H, W)
    return hip.conv3d_plan(cc.volume(hip, gi, cc.BASE), cc.volume(hip, go, 2 * cc.BASE), 3, cfg, (4 * cc.BASE, scratch) if scratch else None,
                           dict(precision=prec), gn_groups=gn_groups, zero_t_halo=True, plan_clips=plan_clips)


def _is_deep(rec):
    return rec["deep"] == 8 and (rec["rows"], rec["tw"], rec["nt"], rec["blk"], rec["threads"], rec["ksplit"]) == (8, 8, 512, 2, 512, 1)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("Cout", COUTS)
@pytest.mark.parametrize("Cin", CINS)
def test_deep_tile_equals_todays_tiles(hip, Cin, Cout, H, W, bias):
    x, w, b = _case(Cin, Cout, T, H, W, 700 + Cin + Cout + H)
    buf, vin = _haloed(hip, x)
    wp, bd = hip.pack_conv_weight_any(dev(w), "f16x3"), (dev(b) if bias else None)
    recs = _plan(hip, Cin, Cout, T, H, W, hip.TILE_CFG_DEEP)
    assert len(recs) == 1 and _is_deep(recs[0]) and recs[0]["grid"] == ((H // 8) * (W // 8), 1, 1), recs
    deep, _ = _run(hip, vin, wp, bd, (Cout, T, H, W), hip.TILE_CFG_DEEP)
    assert torch.isfinite(deep).all()
    for cfg in (6, 1):
        today, _ = _run(hip, vin, wp, bd, (Cout, T, H, W), cfg)
        n_diff = int((deep != today).sum())
        print("[Cin %d Cout %d %dx%d %s] vs tile_cfg %d: %d of %d elements differ" % (Cin, Cout, H, W, "bias" if bias else "nobias", cfg, n_diff, deep.numel()))
        assert torch.equal(deep, today)


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("Cin,Cout", [(4, 64), (12, 128)])
def test_two_clips_per_launch_equal_single_clip_calls(hip, Cin, Cout, H, W):
    """The clip is blockIdx.y of the one launch: clip c of a batch of two is the single-clip call's output, for the deep tile and against today's."""
    bufs, g, stride = hip.alloc_padded_batch(2, Cin, T, H, W)
    w, b = _rand((Cout, Cin, 3, 3, 3), 31, 1.0 / np.sqrt(Cin * 27)), _rand((Cout,), 32)
    wp, bd = hip.pack_conv_weight_any(dev(w), "f16x3"), dev(b)
    for c in range(2):
        hip.copy_to_volume(dev(_rand((Cin, T, H, W), 40 + c)), 0, hip.padded_interior_view(bufs[c], g, Cin, T, H, W))
    out = torch.full((2, Cout, T, H, W), float("nan"), device="cuda")
    hip.conv3d_zero_t_halo_batch(hip.padded_halo_view(bufs[0], g, Cin, T, H, W), wp, bd, hip.dense_volume(out[0]), 2, stride, out[0].numel(),
                                 tile_cfg=hip.TILE_CFG_DEEP, precision="f16x3")
    torch.cuda.synchronize()
    assert not torch.equal(out[0], out[1])
    for c in range(2):
        vin = hip.padded_halo_view(bufs[c], g, Cin, T, H, W)
        for cfg in (hip.TILE_CFG_DEEP, 6):
            single, _ = _run(hip, vin, wp, bd, (Cout, T, H, W), cfg)
            assert torch.equal(out[c], single), "clip %d vs its single-clip call at tile_cfg %d" % (c, cfg)


def test_deep_tile_vs_fp64(hip):
    """At the bound of tests/test_gpu_t_halo_skip.py: error <= max(3 x the fp32-MFMA kernel's own error, 4e-7 max|ref|)."""
    Cin, Cout, H, W = 12, 128, 16, 24
    x, w, b = _case(Cin, Cout, T, H, W, 900)
    ref = F.conv3d(torch.from_numpy(x).double()[None], torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1)[0].numpy()
    buf, vin = _haloed(hip, x)
    o32, _ = _run(hip, vin, hip.pack_conv_weight_any(dev(w), "f32"), dev(b), (Cout, T, H, W), 0, prec="f32")
    assert torch.isfinite(o32).all()
    e32, scale = float(np.abs(o32.cpu().numpy().astype(np.float64) - ref).max()), float(np.abs(ref).max())
    o, _ = _run(hip, vin, hip.pack_conv_weight_any(dev(w), "f16x3"), dev(b), (Cout, T, H, W), hip.TILE_CFG_DEEP)
    e = float(np.abs(o.cpu().numpy().astype(np.float64) - ref).max())
    print("max|err| vs fp64: fp32-MFMA %.3e, deep f16x3 %.3e (max|ref| %.3g)" % (e32, e, scale))
    assert e <= max(3.0 * e32, 4e-7 * scale)


def test_nonfinite_voxels_spread_as_in_todays_tile(hip):
    Cin, Cout, H, W = 12, 128, 16, 24
    x, w, b = _case(Cin, Cout, T, H, W, 910)
    x[3, 0, 7, 8] = np.inf          # first plane, at the seam of four patches
    x[9, 5, 15, 23] = np.nan        # an interior plane, the map's last corner
    buf, vin = _haloed(hip, x)
    wp, bd = hip.pack_conv_weight_any(dev(w), "f16x3"), dev(b)
    deep, _ = _run(hip, vin, wp, bd, (Cout, T, H, W), hip.TILE_CFG_DEEP)
    today, _ = _run(hip, vin, wp, bd, (Cout, T, H, W), 6)
    bad = ~torch.isfinite(deep)
    assert int(bad.sum()) > 0 and torch.equal(bad, ~torch.isfinite(today))
    assert torch.equal(torch.isnan(deep), torch.isnan(today))
    assert torch.equal(deep[~bad], today[~bad])


@pytest.mark.parametrize("groups", [16, 32])
@pytest.mark.parametrize("H,W", MAPS)
def test_groupnorm_statistics(hip, H, W, groups):
    Cin, Cout = 12, 128
    x, w, b = _case(Cin, Cout, T, H, W, 920 + H)
    buf, vin = _haloed(hip, x)
    wp, bd = hip.pack_conv_weight_any(dev(w), "f16x3"), dev(b)
    recs = _plan(hip, Cin, Cout, T, H, W, hip.TILE_CFG_DEEP, gn_groups=groups)
    assert len(recs) == 1 and _is_deep(recs[0]) and recs[0]["gn"] == "tile epilogue", recs
    deep, st = _run(hip, vin, wp, bd, (Cout, T, H, W), hip.TILE_CFG_DEEP, gn_groups=groups)
    again, st2 = _run(hip, vin, wp, bd, (Cout, T, H, W), hip.TILE_CFG_DEEP, gn_groups=groups)
    today, st_today = _run(hip, vin, wp, bd, (Cout, T, H, W), 6, gn_groups=groups)
    assert torch.equal(deep, today) and torch.equal(deep, again) and torch.equal(st, st2)
    og = deep.cpu().numpy().astype(np.float64).reshape(groups, -1)
    got = st.cpu().numpy().astype(np.float64).reshape(groups, 2)
    mean, rstd = og.mean(1), 1.0 / np.sqrt(og.var(1) + 1e-5)
    e_mean, e_rstd = np.abs(got[:, 0] - mean).max(), np.abs(got[:, 1] / rstd - 1.0).max()
    print("[%dx%d, %d groups] mean err %.3e, rstd rel err %.3e; vs today's statistics: %d of %d floats differ" % (
        H, W, groups, e_mean, e_rstd, int((st != st_today).sum()), st.numel()))
    assert e_mean <= 2e-6 * max(1.0, np.abs(mean).max()) and e_rstd <= 2e-6


@pytest.mark.parametrize("why", ["T4", "map12x24", "bf16x6", "splitk"])
def test_request_falls_back_where_the_tile_does_not_exist(hip, why):
    Cin, Cout, Tn, H, W, prec, scratch = 12, 128, T, 16, 24, "f16x3", 0
    if why == "T4":
        Tn = 4
    elif why == "map12x24":
        H = 12
    elif why == "bf16x6":
        prec = "bf16x6"
    else:
        scratch = 16 * Cout * Tn * H * W
    asked, plain = _plan(hip, Cin, Cout, Tn, H, W, hip.TILE_CFG_DEEP, prec, scratch), _plan(hip, Cin, Cout, Tn, H, W, 0, prec, scratch)
    assert asked == plain and all(r["deep"] == 0 for r in asked), (asked, plain)
    assert cc.tile_name(asked[0]) in cc.split_tiles(prec)
    if why == "splitk":
        assert asked[0]["ksplit"] > 1
    x, w, b = _case(Cin, Cout, Tn, H, W, 930)
    buf, vin = _haloed(hip, x)
    wp, bd = hip.pack_conv_weight_any(dev(w), prec), dev(b)
    scr = torch.full((scratch,), float("nan"), device="cuda") if scratch else None
    a, _ = _run(hip, vin, wp, bd, (Cout, Tn, H, W), hip.TILE_CFG_DEEP, prec, scratch=scr)
    p, _ = _run(hip, vin, wp, bd, (Cout, Tn, H, W), 0, prec, scratch=scr)
    assert torch.isfinite(p).all() and torch.equal(a, p)


def test_decoder_switch_heads_agree_and_plan_is_the_deep_tile(hip):
    """One small decoder (T = 8, 4x level 16 x 24, two clips per call) with the model switch on and off: head outputs within the decoder
    goldens' 1e-3.  plan_clips is raised so that the 6-workgroup block_4x launch plans un-split, as the 405-workgroup one of a real step does."""
    from stemseg_amd.modeling.embedding_decoder import SqueezingExpandDecoder as Emb
    CIN, INTER, H4, W4, N = 32, [64, 64, 32, 32], 16, 24, 2
    m = Emb(CIN, INTER, 4, True, False, "xyff", NormType=lambda c: torch.nn.GroupNorm(8, c), num_frames=T)
    sd = synth.synth_state_dict([(k, v.shape) for k, v in m.state_dict().items()], 23, prefix="x.")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(m.state_dict()[k].shape) for k, v in sd.items()})
    m = m.cuda().eval()
    m.precision, m.plan_clips = "f16x3", 64
    recs = _plan(hip, CIN, INTER[3], T, H4, W4, hip.TILE_CFG_DEEP, scratch=2 * INTER[3] * T * H4 * W4, gn_groups=8, plan_clips=64)
    assert len(recs) == 1 and _is_deep(recs[0]), recs
    levels = [hip.alloc_padded_batch(N, CIN, T, (H4 // 8) * s, (W4 // 8) * s, "cuda") for s in (1, 2, 4, 8)]
    for c in range(N):
        feats = synth.synth_features(T, H4 // 8, W4 // 8, C=CIN, seed=80 + c)
        for (bufs, g, _), f, s in zip(levels, feats, (1, 2, 4, 8)):
            hip.copy_to_volume(dev(f), 0, hip.padded_interior_view(bufs[c], g, CIN, T, (H4 // 8) * s, (W4 // 8) * s))
    outs = {}
    for on in (True, False):
        m.deep_block4x = on
        outs[on] = m.forward_single(([lv[0][0] for lv in levels], (T, H4, W4)), 2, clip_batch=(N, [lv[2] for lv in levels])).clone()
        single = m.forward_single(([lv[0][1] for lv in levels], (T, H4, W4)), 2).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(outs[on]).all() and torch.equal(outs[on][1], single)
    err = float((outs[True] - outs[False]).abs().max())
    print("decoder heads, deep tile on vs off: max |diff| %.3e (max |out| %.3g)" % (err, float(outs[False].abs().max())))
    assert err <= 1e-3
    bad, where = m.check_workspaces()
    assert bad == 0, where


def test_pipeline_labels_identical_with_the_switch_on_and_off(hip):
    """A synthetic clip through the whole model (64 x 96 frames: 4x level 16 x 24) and the clustering: embeddings within 1e-3, labels identical."""
    from stemseg_amd import config
    from stemseg_amd.modeling.inference_model import InferenceModel
    from stemseg_amd.pipeline import ClipPipeline
    try:
        config.load_preset("davis")
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        model = InferenceModel()
        names = [(k, v.shape) for k, v in model._model.state_dict().items()]
        sd = synth.synth_state_dict(names, 7)
        sd["seediness_head.conv_out.weight"] = sd["seediness_head.conv_out.weight"] * 30
        model._model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(model._model.state_dict()[k].shape) for k, v in sd.items()})
        model.plan_clips = 64
        pipe = ClipPipeline(model, device="cuda:0")
        frames = (torch.from_numpy(synth.synth_frames(8, 64, 96, seed=7).astype(np.float32)).permute(0, 3, 1, 2) -
                  torch.tensor(config.cfg.INPUT.IMAGE_MEAN)[None, :, None, None]).cuda()
        res = {}
        for on in (True, False):
            model.deep_block4x = on
            out = pipe.step(frames)
            o2 = pipe.cluster(out["emb"].contiguous(), out["bw"].contiguous(), out["seed"].contiguous())
            torch.cuda.synchronize()
            n = int(o2["frame_offsets"].cpu()[-1])
            res[on] = (out["emb"].clone(), out["seed"].clone(), n, o2["labels"][:n].cpu().numpy().copy())
        assert float((res[True][0] - res[False][0]).abs().max()) <= 1e-3 and float((res[True][1] - res[False][1]).abs().max()) <= 1e-3
        print("fg points %d / %d, instances %d" % (res[True][2], res[False][2], len(np.unique(res[True][3]))))
        assert res[True][2] == res[False][2] > 0 and np.array_equal(res[True][3], res[False][3])
    finally:
        config.load_preset("defaults")
