"""GPU tests of the YouTube-VIS / KITTI-MOTS writers (ABI 11): the on-device COCO RLE encoder against the numpy restatement of
pycocotools 2.0 maskApi.c semantics (tests/writer_oracle.py), the 16-bit index maps, the per-instance class statistics, and
both writers end to end on synthetic sequences -- directly and through the reference's names (the overlay), ending in save()."""
import json
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest
import torch

from tests import writer_oracle as wo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _as_index_map(a, K):
    """numpy condensed map -> device tensor of the dtype the encoder reads (uint8, or int16 holding uint16 values)."""
    if K <= 255:
        return dev(a.astype(np.uint8))
    return dev(a.astype(np.uint16).view(np.int16))


def _blocks(rs, F, H, W, K, n_blocks):
    m = np.zeros((F, H, W), np.int32)
    for f in range(F):
        for _ in range(n_blocks):
            k = rs.randint(1, K + 1)
            y, x = rs.randint(0, H), rs.randint(0, W)
            m[f, y:y + rs.randint(1, max(2, H // 3)), x:x + rs.randint(1, max(2, W // 3))] = k
    return m


def _check_rle(hip, maps, K, **kw):
    F, H, W = maps.shape
    r = hip.rle_encode(_as_index_map(maps, K), K, **kw)
    for f in range(F):
        ref = wo.encode_map(maps[f], K)
        for n in range(1, K + 1):
            c, s, a, bb = ref[n - 1]
            q = r.plane(f, n)
            assert r.plane_counts(f, n).tolist() == c, (f, n)
            assert r.strings[q] == s, (f, n)
            assert int(r.area[q]) == a and r.bbox[q].tolist() == bb, (f, n, int(r.area[q]), r.bbox[q].tolist(), a, bb)
    return r


def test_rle_small_cases(hip):
    rs = np.random.RandomState(1)
    cases = [np.zeros((2, 5, 7), np.int32), np.ones((2, 5, 7), np.int32),
             rs.randint(0, 4, (3, 37, 29)).astype(np.int32),                  # random: a boundary at almost every pixel
             rs.randint(0, 3, (1, 1, 1)).astype(np.int32) + 1, rs.randint(0, 3, (2, 1, 17)).astype(np.int32),
             rs.randint(0, 3, (2, 23, 1)).astype(np.int32), _blocks(rs, 4, 31, 45, 5, 6)]
    single = np.zeros((2, 9, 11), np.int32)
    single[0, 0, 0] = 1                                                          # p = 0
    single[1, 8, 10] = 2                                                         # p = H*W - 1
    cases.append(single)
    for m in cases:
        K = max(int(m.max()), 1) + 1                                             # (one plane that is always empty)
        _check_rle(hip, m, K)


def test_rle_capacity_retry(hip):
    """A plan over capacity reports the need and the wrapper re-plans: same result as a roomy first plan."""
    m = np.random.RandomState(2).randint(0, 5, (2, 40, 50)).astype(np.int32)
    r = _check_rle(hip, m, 4, max_changes=16)
    r2 = hip.rle_encode(_as_index_map(m, 4), 4)
    assert r.strings == r2.strings


@pytest.mark.parametrize("H,W,F,K", [(720, 1280, 3, 10), (375, 1242, 3, 12)])
def test_rle_full_size_and_deterministic(hip, H, W, F, K):
    rs = np.random.RandomState(H)
    m = _blocks(rs, F, H, W, K, 14)
    m[0, :, W // 2] = 0                                                          # a cut through every column-crossing run
    m[-1] = 0                                                                    # an empty frame
    r = _check_rle(hip, m, K)
    r2 = hip.rle_encode(_as_index_map(m, K), K)
    assert r.strings == r2.strings and np.array_equal(r.counts, r2.counts) and np.array_equal(r.bbox, r2.bbox)
    assert np.array_equal(r.chars, r2.chars)


def test_rle_uint16_k1000(hip):
    rs = np.random.RandomState(7)
    m = _blocks(rs, 2, 120, 200, 1000, 400)
    m[1, :7, :9] = 1000
    r = _check_rle(hip, m, 1000)
    r2 = hip.rle_encode(_as_index_map(m, 1000), 1000)
    assert r.strings == r2.strings


# ------------------------------------------------------------------------------------------------ 16-bit index maps
def _points(maps):
    idx, lab = [], []
    for m in maps:
        ys, xs = np.nonzero(m)
        idx.append((dev(ys.astype(np.int64)), dev(xs.astype(np.int64))))
        lab.append(dev(m[ys, xs].astype(np.int64)))
    return idx, lab


def test_index16_equals_uint8_and_oracle(hip):
    from oracle import masks as omask
    from stemseg_amd import config
    from stemseg_amd.inference.output_utils import MaskMaterializer
    rs = np.random.RandomState(4)
    try:
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 96, 128
        ih, iw = 90, 120
        rw, rh, _ = omask.compute_resize_params_2((iw, ih), 96, 128)
        # K <= 255: the 16-bit path holds exactly the uint8 path's values
        maps = np.zeros((3, 24, 32), np.int64)
        for k in range(1, 30):
            y, x = rs.randint(0, 22), rs.randint(0, 30)
            maps[:, y:y + rs.randint(1, 8), x:x + rs.randint(1, 8)] = k
        maps[1] = np.roll(maps[1], 2, axis=1)
        lut = MaskMaterializer(-1)._lut(list(range(1, 30)), "cuda")
        for t in range(3):
            ys, xs = np.nonzero(maps[t])
            a = [dev(ys.astype(np.int64)), dev(xs.astype(np.int64)), dev(maps[t][ys, xs])]
            d8 = hip.scatter_instance_index(*a, lut, 24, 32)
            d16 = hip.scatter_instance_index_ex(*a, lut, 24, 32, 2)
            d8b = hip.scatter_instance_index_ex(*a, lut, 24, 32, 1)
            assert torch.equal(d8.to(torch.int32), d16.to(torch.int32)) and torch.equal(d8, d8b)
            o8 = hip.resample_instance_masks(d8, 4.0, (rh, rw), (ih, iw))
            o16 = hip.resample_instance_masks_ex(d16, 4.0, (rh, rw), (ih, iw), 2)
            assert torch.equal(o8.to(torch.int32), o16.to(torch.int32))
            assert torch.equal(o8, hip.resample_instance_masks_ex(d8, 4.0, (rh, rw), (ih, iw), 1))
        # K > 255: MaskMaterializer switches to 16 bits; equal to the oracle chain with a wide result (threshold ties allowed)
        big = np.zeros((2, 24, 32), np.int64)
        big[0] = np.arange(24 * 32).reshape(24, 32) // 2 % 300 + 1            # 300 instances, two pixels each
        big[1] = np.flipud(big[0])
        life = {k: 1000 - k for k in range(1, 301)}
        idx, lab = _points(big)
        keep, out = MaskMaterializer(-1).process_sequence((ih, iw), idx, lab, life, (24, 32), 4.0, 300)
        assert out.dtype == torch.int16 and len(keep) == 300 and keep == list(range(1, 301))
        got = out.cpu().numpy().view(np.uint16).astype(np.int32)
        ref = wo.condensed_masks_wide(big, keep, (ih, iw), (rh, rw))
        bad = got != ref
        for t in np.unique(np.nonzero(bad)[0]).tolist():
            soft = omask.soft_masks(big[t], keep, (ih, iw), 96, 128).numpy()
            assert (np.abs(soft - 0.5).min(0)[bad[t]] < 1e-6).all()
        assert bad.mean() < 1e-3 and got.max() > 255
    finally:
        config.load_preset("defaults")


# ------------------------------------------------------------------------------------------------ class statistics
def test_instance_class_stats(hip):
    from stemseg_amd.inference.output_utils import MaskMaterializer
    rs = np.random.RandomState(9)
    F, h, w, C, K = 5, 30, 41, 7, 6
    maps = rs.randint(0, K + 3, (F, h, w)).astype(np.int64)                  # ids K+1, K+2: not kept
    maps[2] = 0                                                               # a frame without points
    keep = list(range(1, K + 1))[::-1]                                        # instance n = keep[n-1]
    lut = MaskMaterializer(-1)._lut(keep, "cuda")
    logits = (rs.randn(F, C, h, w) * 3).astype(np.float32)
    am = rs.randint(0, 3, (F, h, w)).astype(np.int64)
    idx, lab = _points(maps)
    sizes = [int(l.numel()) for l in lab]
    cat = lambda ts: torch.cat(ts) if ts else torch.zeros(0, dtype=torch.int64, device="cuda")
    args = (cat([i[0] for i in idx]), cat([i[1] for i in idx]), cat(lab), sizes, lut, K, (h, w))
    pts, sums, votes = hip.instance_class_stats(*args, logits=dev(logits), argmax=dev(am), n_votes=3)
    pts2, sums2, votes2 = hip.instance_class_stats(*args, logits=dev(logits), argmax=dev(am), n_votes=3)
    assert torch.equal(sums, sums2) and torch.equal(pts, pts2) and torch.equal(votes, votes2)       # bitwise deterministic
    pts, sums, votes = pts.cpu().numpy(), sums.cpu().numpy(), votes.cpu().numpy()
    for n, k in enumerate(keep, 1):
        sel = maps == k
        assert pts[:, n - 1].tolist() == sel.reshape(F, -1).sum(1).tolist()
        assert votes[n - 1].tolist() == [int((am[sel] == c).sum()) for c in range(3)]
        ref = np.array([logits[:, c][sel].astype(np.float64).sum() for c in range(1, C)])
        assert np.all(np.abs(sums[n - 1] - ref) <= 1e-5 * np.maximum(np.abs(ref), 1.0)), (sums[n - 1], ref)


# ------------------------------------------------------------------------------------------------ writers end to end
def _sequence(rs, F, h, w, n_inst, C):
    """Label maps at mask resolution (moving boxes; ids 1..n_inst plus outlier points), multi-class logits with a clear top two
    per instance, an arg-max map with a clear majority per instance, and the chainer-style dicts."""
    maps = np.zeros((F, h, w), np.int64)
    cls = {}
    for k in range(1, n_inst + 1):
        y, x = rs.randint(0, h - 8), rs.randint(0, w - 10)
        hh, ww = rs.randint(4, 10), rs.randint(5, 14)
        first, last = rs.randint(0, F // 2), rs.randint(F // 2, F)
        for t in range(first, last + 1):
            yy, xx = min(h - hh, y + t // 2), min(w - ww, x + t)
            maps[t, yy:yy + hh, xx:xx + ww] = k
        cls[k] = 1 + rs.randint(0, C - 1)
    maps[:, :2, :3] = -1                                                      # outlier points
    logits = (rs.randn(F, C, h, w) * 0.1).astype(np.float32)
    am = np.zeros((F, h, w), np.int64)
    for k, c in cls.items():
        sel = maps == k
        logits[:, c][sel] += 4.0
        am[sel] = 1 + (c % 2)
        am[sel & (rs.rand(F, h, w) < 0.1)] = 2 - (c % 2)
    idx, lab = [], []
    for t in range(F):
        ys, xs = np.nonzero(maps[t] != 0)
        idx.append((dev(ys.astype(np.int64)), dev(xs.astype(np.int64))))
        lab.append(dev(maps[t][ys, xs]))
    ids = [k for k in range(1, n_inst + 1) if (maps == k).any()]
    counts = {k: int((maps == k).sum()) for k in ids}
    counts[-1] = int((maps == -1).sum())
    life = {k: int((maps == k).reshape(F, -1).any(1).sum()) for k in ids}
    life[-1] = F
    return maps, logits, am, idx, lab, counts, life


def _check_masks_vs_oracle(masks, maps, keep, image_hw):
    from oracle import masks as omask
    from stemseg_amd.config import cfg
    rw, rh, _ = omask.compute_resize_params_2((image_hw[1], image_hw[0]), cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM)
    ref = wo.condensed_masks_wide(np.where(maps > 0, maps, 0), keep, image_hw, (rh, rw))
    bad = masks != ref
    for t in np.unique(np.nonzero(bad)[0]).tolist():
        soft = omask.soft_masks(np.where(maps[t] > 0, maps[t], 0), keep, image_hw, cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM).numpy()
        assert (np.abs(soft - 0.5).min(0)[bad[t]] < 1e-6).all()
    assert bad.mean() < 1e-3


def test_ytvis_writer_end_to_end(hip, tmp_path):
    from stemseg_amd import config
    from stemseg_amd.inference.output_utils import YoutubeVISOutputGenerator
    rs = np.random.RandomState(21)
    F, h, w, C, ih, iw = 9, 24, 32, 6, 90, 120
    try:
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 96, 128
        maps, logits, _, idx, lab, counts, life = _sequence(rs, F, h, w, 7, C)
        seq = types.SimpleNamespace(id=3, image_dims=(ih, iw))
        texts = []
        for run in range(2):
            out = str(tmp_path / ("run%d" % run))
            gen = YoutubeVISOutputGenerator(out, -1, True, None, None)
            keep, extra = gen.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(logits), (h, w), 4.0, 5, device="cuda:0")
            assert extra == {} and keep == wo.ytvis_keep(life, -1, 5)
            gen.save()
            texts.append(open(os.path.join(out, "results.json"), "rb").read())
            import zipfile
            with zipfile.ZipFile(os.path.join(out, "results.zip")) as zf:
                assert zf.namelist() == ["results.json"] and zf.read("results.json") == texts[-1]
        assert texts[0] == texts[1]                                             # byte-identical across runs
        masks = gen.sequences[3]["masks"].cpu().numpy().astype(np.int32)
        _check_masks_vs_oracle(masks, maps, keep, (ih, iw))
        res = json.loads(texts[0])
        ref = wo.ytvis_instances(3, keep, counts, maps, logits, masks)
        assert [r["category_id"] for r in res] == [r["category_id"] for r in ref]
        assert [r["score"] for r in res] == [r["score"] for r in ref]
        assert res == ref
        for n, r in enumerate(res, 1):
            for t, s in enumerate(r["segmentations"]):
                assert s["size"] == [ih, iw]
                assert np.array_equal(wo.decode(wo.string_to_counts(s["counts"]), ih, iw), masks[t] == n)
        # nothing kept: None, and no entry
        gen2 = YoutubeVISOutputGenerator(str(tmp_path / "none"), -1, False, keep_masks=False)
        assert gen2.process_sequence(seq, idx, lab, counts, {-1: 3}, torch.from_numpy(logits), (h, w), 4.0, 5) is None
        assert gen2.instances == [] and gen2.sequences == {}
    finally:
        config.load_preset("defaults")


@pytest.mark.parametrize("n_inst,max_tracks", [(9, 6), (300, 1000)])
def test_kitti_writer_end_to_end(hip, tmp_path, n_inst, max_tracks):
    from stemseg_amd import config
    from stemseg_amd.inference.output_utils import KittiMOTSOutputGenerator
    rs = np.random.RandomState(31 + n_inst)
    F, h, w, ih, iw = 12, 24, 60, 60, 150
    try:
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 96, 320
        if n_inst > 255:
            h, w = 48, 120
            maps = np.zeros((F, h, w), np.int64)
            base = (np.arange(h * w).reshape(h, w) // 3) % n_inst + 1
            for t in range(F):
                maps[t] = np.roll(base, t, axis=1)
            maps[F // 2] = np.where(maps[F // 2] % 5 == 0, 0, maps[F // 2])     # instances absent in one frame
            am = rs.randint(0, 3, (F, h, w)).astype(np.int64)
            idx, lab = _points(maps)
            counts = {k: int((maps == k).sum()) for k in range(1, n_inst + 1)}
            life = {k: int((maps == k).reshape(F, -1).any(1).sum()) for k in counts}
            ih, iw = 120, 300
        else:
            maps, _, am, idx, lab, counts, life = _sequence(rs, F, h, w, n_inst, 3)
        seq = types.SimpleNamespace(id="5", image_dims=(ih, iw))
        gen = KittiMOTSOutputGenerator(str(tmp_path / "out"), -1, False)
        keep, mapping = gen.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(am), (h, w), 4.0, max_tracks, device="cuda:0")
        assert keep == wo.kitti_keep(counts, life, -1, max_tracks) and mapping == {n: k for n, k in enumerate(keep, 1)}
        masks = gen.sequences["5"]["masks"].cpu()
        masks = (masks.numpy().view(np.uint16) if masks.dtype == torch.int16 else masks.numpy()).astype(np.int32)
        assert (masks.max() > 255) == (len(keep) > 255)
        _check_masks_vs_oracle(masks, maps, keep, (ih, iw))
        got = open(str(tmp_path / "out" / "results" / "0005.txt")).read().splitlines()
        assert got == wo.kitti_lines(keep, maps, am, masks)
        gen.save()
        nms = open(str(tmp_path / "out" / "results_nms" / "0005.txt")).read().splitlines()
        assert nms == wo.kitti_filter_lines(got)
        with pytest.raises(ValueError):
            gen.process_sequence(seq, idx, lab, {-1: 4}, {-1: 4}, torch.from_numpy(am), (h, w), 4.0, max_tracks)
    finally:
        config.load_preset("defaults")


def test_writers_through_the_reference_names(tmp_path):
    """The reference driver's last steps through ``stemseg.*`` (overlay, skeleton mode): process_sequence then save() for both
    formats; the outputs equal the direct stemseg_amd writers'."""
    code = textwrap.dedent("""
        import json, os, sys, types
        import numpy as np, torch
        import stemseg_amd.overlay as ov
        ov.install()
        from stemseg.config import cfg
        from stemseg.inference.output_utils import YoutubeVISOutputGenerator, KittiMOTSOutputGenerator
        from stemseg.inference.online_chainer import OnlineChainer
        from stemseg_amd.inference.output_utils import generators as direct
        from tests import test_gpu_writers as T
        cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM = 96, 128
        rs = np.random.RandomState(5)
        maps, logits, am, idx, lab, counts, life = T._sequence(rs, 8, 24, 32, 6, 5)
        seq = types.SimpleNamespace(id=0, image_dims=(90, 120))
        out = r"%s"
        y = YoutubeVISOutputGenerator(out + "/y", OnlineChainer.OUTLIER_LABEL, False, None, None, upscaled_inputs=False)
        y.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(logits), (24, 32), 4.0, 10, device="cuda:0")
        y.save()
        k = KittiMOTSOutputGenerator(out + "/k", OnlineChainer.OUTLIER_LABEL, False, upscaled_inputs=False)
        k.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(am), (24, 32), 4.0, 1000, device="cuda:0")
        k.save()
        assert os.path.exists(out + "/y/results.json") and os.path.exists(out + "/y/results.zip")
        assert os.path.exists(out + "/k/results/0000.txt") and os.path.exists(out + "/k/results_nms/0000.txt")
        d = direct.YoutubeVISOutputGenerator(out + "/yd", -1, False)
        d.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(logits), (24, 32), 4.0, 10, device="cuda:0")
        d.save()
        assert open(out + "/y/results.json").read() == open(out + "/yd/results.json").read()
        print("WRITERS-OVERLAY-OK", len(json.load(open(out + "/y/results.json"))))
    """ % str(tmp_path))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "stem-seg_amd")]), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "WRITERS-OVERLAY-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
