"""CPU tests of the save_vis visualisations: the numpy JPEG restatement (tests/jpeg_oracle.py) is byte-identical to PIL /
libjpeg-turbo over qualities, edge-case sizes and contents, the restated overlay equals its per-pixel table, the dataset
sequences load their frames, the C-ABI of the visualisation entry points rejects bad arguments before any GPU call, and a
writer whose sequence has no frames warns and writes no vis/."""
import ctypes
import io
import os
import types
import warnings

import numpy as np
import pytest

from tests import jpeg_oracle as jo

SIZES = [(480, 854), (375, 1242), (720, 1280), (1, 1), (9, 17), (33, 15)]          # (H, W)
QUALITIES = [1, 10, 50, 75, 95, 100]


def _content(kind, H, W, seed):
    rs = np.random.RandomState(seed)
    if kind == "random":
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "flat":
        return np.full((H, W, 3), (30, 200, 90), np.uint8)
    if kind == "gradient":
        yy, xx = np.mgrid[0:H, 0:W]
        return np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), ((xx + yy) * 7) % 256], 2).astype(np.uint8)
    return (rs.randint(0, 2, (H, W, 3)) * 255).astype(np.uint8)                          # 0 / 255 saturated


@pytest.mark.parametrize("kind", ["random", "flat", "gradient", "saturated"])
@pytest.mark.parametrize("H,W", SIZES)
def test_oracle_jpeg_matches_pil(H, W, kind):
    img = _content(kind, H, W, H + W)
    for q in QUALITIES:
        assert jo.encode(img, q) == jo.pil_encode(img, q), (H, W, kind, q)


def test_oracle_header_and_tables():
    from PIL import Image
    lq, cq = jo.quant_tables(50)
    assert lq == jo.STD_LUMA_Q and cq == jo.STD_CHROMA_Q                                # scale 100: the Annex K tables
    assert jo.quant_tables(100) == ([1] * 64, [1] * 64)
    assert max(jo.quant_tables(1)[0]) == 255                                             # baseline clamp
    h = jo.header(9, 17, 75)
    assert jo.pil_encode(np.zeros((9, 17, 3), np.uint8), 75).startswith(h)
    im = Image.open(io.BytesIO(jo.encode(_content("random", 33, 15, 1), 95)))
    assert im.size == (15, 33) and im.mode == "RGB"
    assert [tuple(l[1:3]) for l in im.layer] == [(2, 2), (1, 1), (1, 1)]                 # 4:2:0


def test_oracle_overlay_is_the_per_pixel_table():
    """The reference's per-instance loop (non-mask pixels pass through 0.6 s + 0.4 s once per instance) equals one table lookup
    per mask pixel, whatever the order of the instances."""
    t = jo.overlay_table()
    s = np.arange(256, dtype=np.float64)
    assert np.array_equal(((0.6 * s) + ((1. - 0.6) * s)).astype(np.uint8), np.arange(256))
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, (30, 40, 3)).astype(np.uint8)
    m = rs.randint(0, 9, (30, 40))
    colors = rs.randint(0, 256, (9, 3)).astype(np.uint8)
    ref = img.copy()
    sel = m > 0
    for c in range(3):
        ref[..., c][sel] = t[colors[m[sel], c], img[..., c][sel]]
    assert np.array_equal(jo.overlay(img, m, colors), ref)


def test_generic_sequence_load_images(tmp_path):
    from PIL import Image
    from stemseg_amd.modeling.inference_model import InferenceModel
    from stemseg_amd.utils.video_dataset import GenericVideoSequence
    rs = np.random.RandomState(2)
    os.makedirs(str(tmp_path / "a"))
    paths = []
    for t in range(3):
        Image.fromarray(rs.randint(0, 256, (7, 11, 3)).astype(np.uint8)).save(str(tmp_path / "a" / ("%d.png" % t)))
        paths.append("a/%d.png" % t)
    seq = GenericVideoSequence(dict(id="s", height=7, width=11, image_paths=paths), str(tmp_path))
    ref = InferenceModel.load_images([str(tmp_path / p) for p in paths])
    got = seq.load_images()
    assert len(got) == 3 and all(np.array_equal(a, b) and a.dtype == np.uint8 for a, b in zip(got, ref))
    sub = seq.load_images([2, 0])
    assert np.array_equal(sub[0], ref[2]) and np.array_equal(sub[1], ref[0])
    assert got[0].shape == seq.image_dims + (3,)
    seq.image_paths.append("a/missing.png")
    with pytest.raises(ValueError):
        seq.load_images([3])


def test_cabi_vis_argument_errors():
    from stemseg_amd import hip
    l = hip.lib()
    for n in ("stemseg_hip_vis_composite", "stemseg_hip_jpeg_workspace_bytes", "stemseg_hip_jpeg_plan", "stemseg_hip_jpeg_encode"):
        assert hasattr(ctypes.CDLL(hip.LIB_PATH), n) and n in hip.SIGNATURES, n
    assert l.stemseg_hip_version() == 11
    fake = ctypes.c_void_p(0x1000)                      # never dereferenced: every call below fails its argument check first
    assert l.stemseg_hip_vis_composite(fake, fake, 3, 1, 4, 4, fake, 2, fake, None) == -1
    assert b"index_bytes" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_vis_composite(fake, fake, 1, 1, 4, 4, fake, 256, fake, None) == -1
    assert b"does not fit" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_vis_composite(fake, fake, 1, 0, 4, 4, fake, 2, fake, None) == -1
    assert b"bad dims" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_vis_composite(fake, None, 2, 1, 4, 4, fake, 2, fake, None) == -1
    assert b"null pointer" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_jpeg_workspace_bytes(0, 4, 4) == 0
    assert l.stemseg_hip_jpeg_workspace_bytes(1, 65536, 4) == 0
    ws = l.stemseg_hip_jpeg_workspace_bytes(2, 9, 17)
    assert ws > 0 and l.stemseg_hip_jpeg_workspace_bytes(3, 9, 17) > ws
    out = (ctypes.c_int64 * 4)()
    plan = lambda F, H, W, q, nbytes, frames=fake: l.stemseg_hip_jpeg_plan(frames, F, H, W, q, fake, nbytes, fake, fake, None)
    assert plan(2, 9, 17, 0, ws) == -1 and b"quality" in l.stemseg_hip_last_error()
    assert plan(2, 9, 17, 101, ws) == -1 and b"quality" in l.stemseg_hip_last_error()
    assert plan(2, 9, 70000, 95, ws) == -1 and b"65535" in l.stemseg_hip_last_error()
    assert plan(0, 9, 17, 95, ws) == -1 and b"bad dims" in l.stemseg_hip_last_error()
    assert plan(2, 9, 17, 95, ws - 1) == -1 and b"workspace" in l.stemseg_hip_last_error()
    assert plan(2, 9, 17, 95, ws, None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_jpeg_encode(2, 9, 17, 95, fake, ws, None, 100, out, None) == -1
    assert b"null pointer" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_jpeg_encode(2, 9, 17, 95, fake, ws, fake, 0, out, None) == -1
    assert b"out_bytes" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_jpeg_encode(2, 9, 17, 95, fake, ws - 1, fake, 100, out, None) == -1
    assert b"workspace" in l.stemseg_hip_last_error()


def test_writer_visualization_without_frames_warns(tmp_path):
    """A sequence object without load_images (as the existing writer tests pass): one warning, no vis/, no device work."""
    from stemseg_amd.inference.output_utils import YoutubeVISOutputGenerator
    gen = YoutubeVISOutputGenerator(str(tmp_path / "y"), -1, True, None, None)
    seq = types.SimpleNamespace(id=3, image_dims=(9, 17))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        gen._save_visualizations(seq, None, np.zeros((2, 3), np.uint8), os.path.join(gen.vis_output_dir, "3"))
    assert len(w) == 1 and "load_images" in str(w[0].message)
    assert not os.path.exists(str(tmp_path / "y" / "vis"))
