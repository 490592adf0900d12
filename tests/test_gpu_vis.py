"""GPU tests of the save_vis visualisations: the overlay composite against the reference's numpy arithmetic for every (colour,
pixel) pair, the device JPEG encoder byte-identical to PIL / libjpeg-turbo (tests/jpeg_oracle.py restates it), and the three
writers end to end with ``save_visualization=True`` -- directly and through the reference's names (the overlay)."""
import json
import os
import subprocess
import sys
import textwrap
import types

import numpy as np
import pytest
import torch

from tests import jpeg_oracle as jo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [(480, 854), (375, 1242), (720, 1280), (1, 1), (9, 17), (33, 15)]          # (H, W)
QUALITIES = [1, 10, 50, 75, 95, 100]


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def contents(H, W, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    grad = np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), ((xx + yy) * 7) % 256], 2).astype(np.uint8)
    return [rs.randint(0, 256, (H, W, 3)).astype(np.uint8), np.full((H, W, 3), (30, 200, 90), np.uint8), grad,
            (rs.randint(0, 2, (H, W, 3)) * 255).astype(np.uint8)]


# ------------------------------------------------------------------------------------------------ composite
@pytest.mark.parametrize("index_bytes", [1, 2])
def test_composite_every_colour_pixel_pair(hip, index_bytes):
    """Row y of the frame holds instance y + 1 (uint8: 255 instances, colours n and n - 1 on two channels; uint16: 256
    instances), column x the pixel value x: all 65 536 (colour, pixel) pairs, plus rows of 0 and of ids beyond K."""
    table = jo.overlay_table()
    K = 255 if index_bytes == 1 else 256
    n = np.arange(K + 1)
    colors = np.stack([n % 256, np.maximum(n - 1, 0), (n * 37) % 256], 1).astype(np.uint8)
    if index_bytes == 2:
        colors[:, 0] = np.maximum(n - 1, 0)
    H, W = K + 2, 256
    img = np.empty((1, H, W, 3), np.uint8)
    img[..., 0] = np.arange(W)[None, None, :]
    img[..., 1] = (255 - np.arange(W))[None, None, :]
    img[..., 2] = ((np.arange(W) * 5) % 256)[None, None, :]
    m = np.zeros((1, H, W), np.int64)
    m[0, :K] = np.arange(1, K + 1)[:, None]
    m[0, K + 1] = K + 1 if index_bytes == 2 else 0                                   # beyond K: unchanged
    mt = dev(m.astype(np.uint8)) if index_bytes == 1 else dev(m.astype(np.uint16).view(np.int16))
    got = hip.vis_composite(dev(img), mt, dev(colors)).cpu().numpy()
    sel = (m[0] >= 1) & (m[0] <= K)
    ref = img.copy()
    ids = m[0][sel]
    for c in range(3):
        ref[0][..., c][sel] = table[colors[ids, c], img[0][..., c][sel]]
    assert np.array_equal(got, ref)
    pairs = set()
    for c in range(3):
        pairs |= set((colors[ids, c].astype(np.int64) * 256 + img[0][..., c][sel]).tolist())
    assert len(pairs) == 65536
    # the reference's per-instance loop on a random map of a few instances gives the same image
    rs = np.random.RandomState(3)
    rm = rs.randint(0, 6, (2, 40, 50))
    rimg = rs.randint(0, 256, (2, 40, 50, 3)).astype(np.uint8)
    cm = rs.randint(0, 256, (6, 3)).astype(np.uint8)
    got = hip.vis_composite(dev(rimg), dev(rm.astype(np.uint8)) if index_bytes == 1 else dev(rm.astype(np.uint16).view(np.int16)),
                            dev(cm)).cpu().numpy()
    for t in range(2):
        assert np.array_equal(got[t], jo.overlay(rimg[t], rm[t], cm))


# ------------------------------------------------------------------------------------------------ JPEG
@pytest.mark.parametrize("quality", QUALITIES)
def test_jpeg_encode_matches_pil(hip, quality):
    for H, W in SIZES:
        frames = np.stack(contents(H, W, H * 7 + W + quality))
        data, offs = hip.jpeg_encode(dev(frames), quality)
        assert offs.shape == (len(frames) + 1,) and offs[0] == 0 and offs[-1] == len(data)
        for f in range(len(frames)):
            got = data[offs[f]:offs[f + 1]].tobytes()
            assert got == jo.pil_encode(frames[f], quality), (H, W, quality, f)
        data2, offs2 = hip.jpeg_encode(dev(frames), quality)
        assert np.array_equal(offs, offs2) and np.array_equal(data, data2)                # deterministic


def test_jpeg_encode_single_frames_and_long_batches(hip):
    rs = np.random.RandomState(9)
    frames = rs.randint(0, 256, (21, 24, 40, 3)).astype(np.uint8)
    frames[::3] //= 16                                                                     # some smooth frames in between
    data, offs = hip.jpeg_encode(dev(frames), 95)
    for f in range(len(frames)):
        assert data[offs[f]:offs[f + 1]].tobytes() == jo.pil_encode(frames[f], 95)
        d1, o1 = hip.jpeg_encode(dev(frames[f:f + 1]), 95)
        assert d1.tobytes() == data[offs[f]:offs[f + 1]].tobytes()


# ------------------------------------------------------------------------------------------------ writers end to end
def _write_frames(tmp_path, T, ih, iw, seed):
    from PIL import Image
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:ih, 0:iw]
    paths, frames = [], []
    os.makedirs(str(tmp_path / "img"), exist_ok=True)
    for t in range(T):
        bgr = np.stack([(xx * 3 + t * 11) % 256, (yy * 5 + t * 3) % 256, rs.randint(0, 256, (ih, iw))], 2).astype(np.uint8)
        p = "img/%05d.png" % t
        Image.fromarray(bgr[..., ::-1]).save(str(tmp_path / p))
        paths.append(p)
        frames.append(bgr)
    return paths, frames


def _tree(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d)] = open(p, "rb").read()
    return out


def _check_vis(vis_dir, frames, masks, colors_of_frame):
    names = sorted(os.listdir(vis_dir))
    assert names == ["{:05d}.jpg".format(t) for t in range(len(frames))]
    for t, bgr in enumerate(frames):
        ref = jo.pil_encode(jo.overlay(bgr, masks[t], colors_of_frame(t)), 95)
        assert open(os.path.join(vis_dir, names[t]), "rb").read() == ref, t


@pytest.mark.parametrize("fmt", ["davis", "ytvis", "kitti"])
def test_writers_save_visualization(hip, tmp_path, fmt):
    from PIL import Image
    from stemseg_amd import config
    from stemseg_amd.inference.output_utils import DavisOutputGenerator, KittiMOTSOutputGenerator, YoutubeVISOutputGenerator
    from stemseg_amd.inference.output_utils.generators import pascal_color_map
    from stemseg_amd.utils.video_dataset import GenericVideoSequence
    from tests import test_gpu_writers as W
    rs = np.random.RandomState(41)
    T, h, w, ih, iw = 18, 24, 32, 90, 120                      # 18 frames: more than one chunk of the writers' vis loop
    cmap = pascal_color_map()
    try:
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 96, 128
        maps, logits, am, idx, lab, counts, life = W._sequence(rs, T, h, w, 7, 5)
        paths, frames = _write_frames(tmp_path, T, ih, iw, 5)
        seq_id = "0003" if fmt == "kitti" else "seq3"
        seq = GenericVideoSequence(dict(id=seq_id, height=ih, width=iw, image_paths=paths), str(tmp_path))
        trees = []
        for flag in (False, True):
            out = str(tmp_path / ("out%d" % flag))
            if fmt == "davis":
                gen = DavisOutputGenerator(out, -1, flag)
                gen.process_sequence(seq, idx, lab, counts, life, None, (h, w), 4.0, 5, device="cuda:0")
            elif fmt == "ytvis":
                gen = YoutubeVISOutputGenerator(out, -1, flag, None, None)
                gen.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(logits), (h, w), 4.0, 5, device="cuda:0")
                gen.save()
            else:
                gen = KittiMOTSOutputGenerator(out, -1, flag)
                gen.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(am), (h, w), 4.0, 1000, device="cuda:0")
                gen.save()
            tree = _tree(out)
            trees.append({k: v for k, v in tree.items() if not k.startswith("vis" + os.sep)})
            assert any(k.startswith("vis" + os.sep) for k in tree) == flag
        assert trees[0] == trees[1]                                                          # results identical, flag on or off
        out = str(tmp_path / "out1")
        if fmt == "davis":
            masks = [np.array(Image.open(os.path.join(out, "results", seq_id, "{:05d}.png".format(t)))) for t in range(T)]
            _check_vis(os.path.join(out, "vis", seq_id), frames, masks, lambda t: cmap)
        elif fmt == "ytvis":
            masks = gen.sequences[seq_id]["masks"].cpu().numpy()
            assert json.load(open(os.path.join(out, "results.json")))
            _check_vis(os.path.join(out, "vis", seq_id), frames, masks, lambda t: cmap)
        else:
            masks = gen.sequences[seq_id]["masks"].cpu().numpy()
            # kitti_mots.py:230 colours by the mapped id n (the txt lines carry cat * 1000 + n)
            ids = {int(line.split()[1]) for line in open(os.path.join(out, "results", seq_id + ".txt"))}
            assert ids and all(i // 1000 in (1, 2) for i in ids)
            _check_vis(os.path.join(out, "vis", seq_id), frames, masks, lambda t: cmap)
    finally:
        config.load_preset("defaults")


def test_writer_visualization_through_the_reference_names(tmp_path):
    """The reference driver's last steps through ``stemseg.*`` (overlay, skeleton mode) with save_vis on: the sequence comes from
    ``parse_generic_video_dataset`` and the vis/ files equal the direct writer's."""
    _write_frames(tmp_path, 6, 90, 120, 8)
    json.dump({"meta": {"category_labels": {"1": "a"}},
               "sequences": [{"id": "0001", "height": 90, "width": 120, "image_paths": ["img/%05d.png" % t for t in range(6)]}]},
              open(str(tmp_path / "ds.json"), "w"))
    code = textwrap.dedent("""
        import os, numpy as np, torch
        import stemseg_amd.overlay as ov
        ov.install()
        from stemseg.config import cfg
        from stemseg.data import parse_generic_video_dataset
        from stemseg.inference.output_utils import YoutubeVISOutputGenerator, KittiMOTSOutputGenerator
        from stemseg.inference.online_chainer import OnlineChainer
        from stemseg_amd.inference.output_utils import generators as direct
        from tests import test_gpu_writers as T
        cfg.INPUT.MIN_DIM, cfg.INPUT.MAX_DIM = 96, 128
        base = r"%s"
        seqs, _ = parse_generic_video_dataset(base, base + "/ds.json")
        seq = seqs[0]
        rs = np.random.RandomState(5)
        maps, logits, am, idx, lab, counts, life = T._sequence(rs, 6, 24, 32, 6, 5)
        y = YoutubeVISOutputGenerator(base + "/y", OnlineChainer.OUTLIER_LABEL, True, None, None, upscaled_inputs=False)
        y.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(logits), (24, 32), 4.0, 10, device="cuda:0")
        k = KittiMOTSOutputGenerator(base + "/k", OnlineChainer.OUTLIER_LABEL, True, upscaled_inputs=False)
        k.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(am), (24, 32), 4.0, 1000, device="cuda:0")
        yd = direct.YoutubeVISOutputGenerator(base + "/yd", -1, True)
        yd.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(logits), (24, 32), 4.0, 10, device="cuda:0")
        kd = direct.KittiMOTSOutputGenerator(base + "/kd", -1, True)
        kd.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(am), (24, 32), 4.0, 1000, device="cuda:0")
        for a, b in (("y/vis/0001", "yd/vis/0001"), ("k/vis/0001", "kd/vis/0001")):
            names = sorted(os.listdir(os.path.join(base, a)))
            assert names == ["%%05d.jpg" %% t for t in range(6)], names
            for n in names:
                assert open(os.path.join(base, a, n), "rb").read() == open(os.path.join(base, b, n), "rb").read()
        print("VIS-OVERLAY-OK")
    """ % str(tmp_path))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "stem-seg_amd")]), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0 and "VIS-OVERLAY-OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
