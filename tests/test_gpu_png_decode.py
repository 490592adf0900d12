"""GPU tests of the device PNG decoder (hip.png_decode, csrc/png_decode.hip): pixel-identical to PIL on the device-supported
matrix, batches equal single frames, the backstop-only path, corrupt files handed to the host, JPEG and PNG mixed in one
decode_frames call, nothing written outside the workspace, and the two places that read frames (InferenceModel.forward, the
save_vis writers)."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_fixtures as J
from tests import png_fixtures as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def _check_all(hip, files, **kw):
    """Frames of one size per call (the decoder's contract); returns the statuses in order."""
    by_size = {}
    for label, data in files:
        by_size.setdefault(X.pil_bgr(data).shape[:2], []).append((label, data))
    sts = []
    for group in by_size.values():
        out, status = hip.png_decode([d for _, d in group], **kw)
        assert out.shape[0] == len(group)
        for i, (label, data) in enumerate(group):
            assert status[i] & (hip.PNG_STATUS_CORRUPT | hip.PNG_STATUS_HOST) == 0, (label, status[i])
            assert torch.equal(out[i].cpu(), torch.from_numpy(X.pil_bgr(data))), label
        sts.append(status)
    return np.concatenate(sts)


@pytest.mark.parametrize("size", X.SIZES)
def test_matrix_equals_pil(hip, size):
    """Every filter type, zlib level, strategy, memLevel, window size, flush, IDAT split and colour type, and PIL's own files:
    each frame torch.equal to PIL with neither the corrupt nor the host bit."""
    _check_all(hip, X.matrix([size]))


def test_batch_equals_single_frames(hip):
    files = [X.write(X.pixels(120, 200, ct, s), ct, None, s, level=lv) for s, (ct, lv) in enumerate([(2, 6), (6, 1), (0, 9), (4, 0), (2, 3)])]
    batch, _ = hip.png_decode(files[:1] + files[2:3])
    for i, f in enumerate(files[:1] + files[2:3]):
        one, st = hip.png_decode([f])
        assert st[0] & (hip.PNG_STATUS_CORRUPT | hip.PNG_STATUS_HOST) == 0, st
        assert torch.equal(batch[i], one[0]), i
    same = [X.write(X.pixels(120, 200, 2, s), 2, None, s, level=lv) for s, lv in enumerate([6, 1, 9, 0, 3, 6, 6, 2])]
    batch, _ = hip.png_decode(same)
    for i, f in enumerate(same):
        assert torch.equal(batch[i], hip.png_decode([f])[0][0]), i


def test_serial_backstop_only(hip):
    """flags = 1 turns the block finder off: every block goes through the serial backstop, with the same pixels."""
    files = [("%s" % lv, X.write(X.pixels(90, 150, 2, lv), 2, None, lv, level=lv, mem_level=1 + lv % 9)) for lv in range(10)]
    st = _check_all(hip, files, flags=1)
    assert (st & hip.PNG_STATUS_BACKSTOP).all(), st
    dyn = [X.write(X.pixels(90, 150, 2, 3), 2, None, 3, level=6)]
    _, st = hip.png_decode(dyn)
    assert not st[0] & hip.PNG_STATUS_BACKSTOP, st                  # dynamic blocks only: the finder found every one


def test_multi_round_subsequences(hip):
    """Tiny subsequences (64 bits) need more than one synchronisation round somewhere; long ones (4096 bits) and the default give
    the same pixels."""
    files = [("noise %d" % s, X.write(X.pixels(96, 160, 2, s, noise=s < 2), 2, None, s, level=[6, 9, 1, 6][s])) for s in range(4)]
    files.append(("pil", X.pil_png(X.pixels(96, 160, 2, 9))))
    st = _check_all(hip, files, sub_bits=64)
    assert (st & hip.PNG_STATUS_MULTI_ROUND).any(), st
    _check_all(hip, files, sub_bits=4096)
    _check_all(hip, files)


def _host_outcome(data):
    try:
        return X.pil_bgr(data), None
    except Exception as ex:                                     # noqa: BLE001 -- the host loader's own exception is the expectation
        return None, type(ex)


@pytest.mark.parametrize("label", [l for l, _ in X.corrupt_files()])
def test_corrupt_files_go_to_the_host(hip, label):
    from stemseg_amd.utils import png as P
    bad = dict(X.corrupt_files())[label]
    good = X.write(X.pixels(23, 31, 2, 9), 2, None, 9)
    assert P.parse(bad).device, label
    ref, exc = _host_outcome(bad)
    if exc is not None:
        with pytest.raises(exc):
            hip.png_decode([good, bad])
        return
    out, st = hip.png_decode([good, bad])
    assert st[1] & hip.PNG_STATUS_CORRUPT and not st[0] & hip.PNG_STATUS_CORRUPT, st
    assert torch.equal(out[1].cpu(), torch.from_numpy(ref)) and torch.equal(out[0].cpu(), torch.from_numpy(X.pil_bgr(good)))


def test_corrupt_frames_are_flagged(hip):
    """The device flags every corrupt fixture itself (pixels never come from the device for them)."""
    from stemseg_amd.utils import png as P
    files = [d for _, d in X.corrupt_files()]
    blob = [P.parse(f) for f in files]
    st = _direct(hip, files, blob)[1]
    assert list(st & 1) == [1] * len(files), [(l, s) for (l, _), s in zip(X.corrupt_files(), st)]


def test_small_png_calls_go_to_the_host(hip):
    """decode_frames sends PNG frames to the device from PNG_MIN_DEVICE_FRAMES per call; fewer are read by the host loader."""
    n = hip.PNG_MIN_DEVICE_FRAMES
    files = [X.write(X.pixels(30, 40, 2, s), 2, None, s) for s in range(n)]
    for k, host in ((n - 1, True), (n, False)):
        out, st = hip.decode_frames(files[:k])
        assert bool((st & hip.PNG_STATUS_HOST).all()) == host and not (st & hip.PNG_STATUS_CORRUPT).any(), st
        for i in range(k):
            assert torch.equal(out[i].cpu(), torch.from_numpy(X.pil_bgr(files[i]))), i


def test_host_classified_and_jpeg_frames_mix_in(hip, monkeypatch):
    monkeypatch.setattr(hip, "PNG_MIN_DEVICE_FRAMES", 1)
    from PIL import Image
    import io
    px = X.pixels(9, 13, 2, 3)
    files = [X.write(px, 2, None, 1)] + [d for _, d in X.host_files() if _host_outcome(d)[1] is None]
    out, st = hip.png_decode(files)
    assert st[0] & (hip.PNG_STATUS_CORRUPT | hip.PNG_STATUS_HOST) == 0 and all(s & hip.PNG_STATUS_HOST for s in st[1:]), st
    for i, f in enumerate(files):
        assert torch.equal(out[i].cpu(), torch.from_numpy(hip._host_png(f))), i
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "BMP")
    mixed = [J.encode(J.content(9, 13, 1), 2, 90), files[0], buf.getvalue(), J.encode(J.content(9, 13, 2), 0, 80), X.write(px, 2, 3)]
    out, st = hip.decode_frames(mixed)
    assert list(st & 0x80) == [0, 0, 0x80, 0, 0], st
    for i, f in enumerate(mixed):
        assert torch.equal(out[i].cpu(), torch.from_numpy(hip._host_jpeg(f))), i


def _direct(hip, files, infos, flags=0, sub_bits=0, G=4096):
    """A direct C-ABI call with canaries around the workspace, the output and the status: returns (frames, status)."""
    from stemseg_amd.utils import png as P
    segs = [P.stream(i, f) for f, i in zip(files, infos)]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)
    total = int(offs[-1])
    data = torch.from_numpy(np.frombuffer(b"".join(segs) + b"\0" * 8, np.uint8).copy()).cuda()
    hdr, recs = P.header_blob(infos)
    blob = torch.from_numpy(np.concatenate([hdr.reshape(-1).view(np.uint8), recs.reshape(-1).view(np.uint8)])).cuda()
    offs_d = torch.from_numpy(offs).cuda()
    F, H, W, C = len(files), infos[0].H, infos[0].W, infos[0].channels
    l = hip.lib()
    wsb = l.stemseg_hip_png_decode_workspace_bytes(F, H, W, C, total, sub_bits, flags)
    assert wsb > 0
    ws = torch.full((wsb + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((F * H * W * 3 + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((F + 2 * G,), 0x3C, dtype=torch.uint8, device="cuda")
    hip.check(l.stemseg_hip_png_decode(hip.ptr(data), hip.ptr(offs_d), hip.ptr(blob), F, H, W, C, total, sub_bits, flags, hip.ptr(ws[G:]), wsb,
                                       hip.ptr(out[G:]), hip.ptr(st[G:]), hip.stream()))
    torch.cuda.synchronize()
    for t, v, n in ((ws, 0xA5, wsb), (out, 0x5A, F * H * W * 3), (st, 0x3C, F)):
        assert bool((t[:G] == v).all()) and bool((t[G + n:] == v).all())
    return out[G:G + F * H * W * 3].view(F, H, W, 3), st[G:G + F].cpu().numpy()


def test_nothing_written_outside_the_workspace(hip):
    from stemseg_amd.utils import png as P
    files = [X.write(X.pixels(23, 31, 2, s, noise=s == 0), 2, None, s, level=s, idat_size=50) for s in range(3)]
    files += [d for _, d in X.corrupt_files()]
    infos = [P.parse(f) for f in files]
    for flags, sub_bits in ((0, 0), (0, 64), (1, 0)):
        img, s = _direct(hip, files, infos, flags, sub_bits)
        assert list(s[:3] & 1) == [0, 0, 0] and (s[3:] & 1).all(), s
        for i in range(3):
            assert torch.equal(img[i].cpu(), torch.from_numpy(X.pil_bgr(files[i])))


def _write_sequence(tmp_path, T, H, W):
    os.makedirs(str(tmp_path / "img"), exist_ok=True)
    paths = []
    for t in range(T):
        p = str(tmp_path / "img" / ("%06d.png" % t))
        with open(p, "wb") as fh:
            fh.write(X.pil_png(X.pixels(H, W, 2, 100 + t)))
        paths.append(p)
    return paths


def test_forward_from_png_paths_device_decode_equals_host(tmp_path):
    from stemseg_amd import config
    from stemseg_amd.modeling.inference_model import InferenceModel
    from tests import synth
    config.load_preset("kittimots")
    try:
        model = InferenceModel()
        names = [(k, v.shape) for k, v in model._model.state_dict().items()]
        sd = synth.synth_state_dict(names, 7)
        model._model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(model._model.state_dict()[k].shape) for k, v in sd.items()})
        model = model.cuda()
        paths = _write_sequence(tmp_path, 12, 120, 400)
        subseq = [list(range(0, 8)), list(range(4, 12))]
        assert torch.equal(InferenceModel.load_images(paths, "cuda").cpu(), torch.from_numpy(np.stack(InferenceModel.load_images(paths))))
        _, st = hip_mod().decode_frames(paths, "cuda")
        assert not (st & 0x81).any(), st                                 # the PNG frames took the device path
        outs = []
        for flag in (True, False):
            model.device_decode = flag
            o = model(paths, subseq)
            torch.cuda.synchronize()
            outs.append(o)
        a, b = outs
        assert len(a["embeddings"]) == len(b["embeddings"]) == 2
        for ea, eb in zip(a["embeddings"], b["embeddings"]):
            for k in ("embeddings", "bandwidths", "seediness"):
                assert torch.equal(getattr(ea, k), getattr(eb, k)), k
        for k in ("fg_masks", "multiclass_masks"):
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), k
    finally:
        config.load_preset("defaults")


def hip_mod():
    from stemseg_amd import hip as h
    return h


def test_kitti_writer_vis_identical_either_way(tmp_path):
    from stemseg_amd import config
    from stemseg_amd.inference.output_utils import KittiMOTSOutputGenerator
    from stemseg_amd.utils.video_dataset import GenericVideoSequence
    from tests import test_gpu_writers as Wr
    from tests.test_gpu_vis import _tree
    rs = np.random.RandomState(41)
    T, h, w, ih, iw = 18, 24, 32, 90, 120
    try:
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 96, 128
        maps, logits, am, idx, lab, counts, life = Wr._sequence(rs, T, h, w, 7, 5)
        paths = [os.path.relpath(p, str(tmp_path)) for p in _write_sequence(tmp_path, T, ih, iw)]
        _, st = hip_mod().decode_frames([os.path.join(str(tmp_path), p) for p in paths], "cuda")
        assert not (st & 0x81).any(), st                                 # the PNG frames took the device path
        seq = GenericVideoSequence(dict(id="0003", height=ih, width=iw, image_paths=paths), str(tmp_path))
        trees = []
        for flag in (True, False):
            out = str(tmp_path / ("out%d" % flag))
            gen = KittiMOTSOutputGenerator(out, -1, True)
            gen.device_decode = flag
            gen.process_sequence(seq, idx, lab, counts, life, torch.from_numpy(am), (h, w), 4.0, 1000, device="cuda:0")
            gen.save()
            trees.append(_tree(out))
        assert any(k.startswith("vis" + os.sep) for k in trees[0])
        assert trees[0] == trees[1]
    finally:
        config.load_preset("defaults")


def test_cv2_equals_device_decode(hip):
    cv2 = pytest.importorskip("cv2")
    files = X.matrix([(17, 33)])
    out, _ = hip.png_decode([d for _, d in files])
    for i, (label, data) in enumerate(files):
        ref = cv2.imdecode(np.frombuffer(data, np.uint8), cv2.IMREAD_COLOR)
        assert torch.equal(out[i].cpu(), torch.from_numpy(ref)), label
