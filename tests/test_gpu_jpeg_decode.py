"""GPU tests of the device JPEG decoder (hip.jpeg_decode, csrc/jpeg_decode.hip): pixel-identical to PIL (libjpeg-turbo) on the
device-supported matrix, batches equal single frames, the multi-round and serial-backstop paths, corrupt files handed to the host,
nothing written outside the workspace, and the two places that read frames (InferenceModel.forward, the save_vis writers)."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_fixtures as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from stemseg_amd import hip as h
    h.require_gpu()
    return h


def _check_all(hip, files, **kw):
    out, status = hip.jpeg_decode([d for _, d in files], **kw)
    assert out.shape[0] == len(files)
    for i, (label, data) in enumerate(files):
        assert status[i] & (hip.JPEG_STATUS_CORRUPT | hip.JPEG_STATUS_HOST) == 0, (label, status[i])
        assert torch.equal(out[i].cpu(), torch.from_numpy(X.pil_bgr(data))), label
    return status


@pytest.mark.parametrize("size", X.SIZES)
def test_matrix_equals_pil(hip, size):
    """Every quality x sampling (noise at q100), optimised tables, restart markers by blocks and by rows, 16-bit quant tables:
    one call per size (frames of several geometries and tables), each frame torch.equal to PIL."""
    _check_all(hip, X.matrix([size]))


def test_own_encoder_files(hip):
    frames = torch.from_numpy(np.stack([X.content(90, 120, s)[..., ::-1] for s in range(5)]).copy()).cuda()
    data, offsets = hip.jpeg_encode(frames, 95)
    files = [("enc %d" % i, data[offsets[i]:offsets[i + 1]].tobytes()) for i in range(5)]
    _check_all(hip, files)


def test_batch_equals_single_frames(hip):
    files = [X.encode(X.content(240, 432, s), 2, q, optimize=bool(s & 1)) for s, q in enumerate([20, 45, 75, 90, 95, 100, 60, 85])]
    batch, _ = hip.jpeg_decode(files)
    for i, f in enumerate(files):
        one, st = hip.jpeg_decode([f])
        assert st[0] & (hip.JPEG_STATUS_CORRUPT | hip.JPEG_STATUS_HOST) == 0, st
        assert torch.equal(batch[i], one[0]), i


def test_multi_round_and_serial_backstop(hip):
    """Tiny subsequences on noise at q100 need more than one synchronisation round; a bound of one round per launch leaves frames
    unconverged, and the serial backstop decodes them -- the same pixels either way."""
    files = [("noise %d" % s, X.encode(X.content(240, 432, s, noise=True), sub, 100)) for s, sub in enumerate([2, 0, "L"])]
    st = _check_all(hip, files, sub_bits=64)
    assert (st & hip.JPEG_STATUS_MULTI_ROUND).any(), st
    st = _check_all(hip, files, sub_bits=64, max_rounds=1)
    assert (st & hip.JPEG_STATUS_BACKSTOP).all(), st
    _check_all(hip, files, sub_bits=4096)


def _host_outcome(data):
    try:
        return X.pil_bgr(data), None
    except Exception as ex:                                     # noqa: BLE001 -- the host loader's own exception is the expectation
        return None, type(ex)


def test_corrupt_files_go_to_the_host(hip):
    good = X.encode(X.content(240, 432, 4), 2, 90)
    rst = X.encode(X.content(240, 432, 5), 0, 90, restart_marker_rows=1)
    i = rst.index(b"\xff\xd1")
    for bad in (X.truncated(good), X.bad_code(good), rst[:i] + b"\xff\xd3" + rst[i + 2:]):
        ref, exc = _host_outcome(bad)
        if exc is not None:
            with pytest.raises(exc):
                hip.jpeg_decode([good, bad])
            continue
        out, st = hip.jpeg_decode([good, bad])
        assert st[1] & hip.JPEG_STATUS_CORRUPT and not st[0] & hip.JPEG_STATUS_CORRUPT
        assert torch.equal(out[1].cpu(), torch.from_numpy(ref)) and torch.equal(out[0].cpu(), torch.from_numpy(X.pil_bgr(good)))


def test_host_classified_files_mix_in(hip):
    files = [X.encode(X.content(17, 33, 1), 2, 80), X.progressive(), X.exif_rotated(orientation=1), X.cmyk()]
    out, st = hip.jpeg_decode(files)
    assert list(st & hip.JPEG_STATUS_HOST) == [0, hip.JPEG_STATUS_HOST, 0, hip.JPEG_STATUS_HOST]
    for i, f in enumerate(files):
        assert torch.equal(out[i].cpu(), torch.from_numpy(hip._host_jpeg(f))), i


def test_nothing_written_outside_the_workspace(hip):
    """Canaries around the workspace, the output and the status: a direct C-ABI call on noise, restart and corrupt frames."""
    from stemseg_amd.utils import jpeg as J
    files = [X.encode(X.content(33, 47, s, noise=True), 2, 100, restart_marker_blocks=3) for s in range(3)]
    files.append(X.bad_code(X.encode(X.content(33, 47, 9), 2, 90)))
    infos = [J.parse(f) for f in files]
    segs = [f[i.ecs_begin:i.ecs_end] for f, i in zip(files, infos)]
    lens = np.array([len(s) for s in segs])
    ends = np.cumsum(lens)
    offs = torch.from_numpy(np.stack([ends - lens, ends], 1).astype(np.int64)).cuda()
    data = torch.from_numpy(np.frombuffer(b"".join(segs), np.uint8).copy()).cuda()
    tabs = torch.from_numpy(np.concatenate([J.table_blob(i) for i in infos])).cuda()
    n_int = sum(-(-J.mcu_count(i) // (i.restart or J.mcu_count(i))) for i in infos)
    F, H, W, G = len(files), 33, 47, 4096
    l = hip.lib()
    for sub_bits, rounds in ((0, 0), (64, 1)):
        wsb = l.stemseg_hip_jpeg_decode_workspace_bytes(F, H, W, 0x22, int(ends[-1]), n_int, sub_bits)
        ws = torch.full((wsb + 2 * G,), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.full((F * H * W * 3 + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
        st = torch.full((F + 2 * G,), 0x3C, dtype=torch.uint8, device="cuda")
        hip.check(l.stemseg_hip_jpeg_decode(hip.ptr(data), hip.ptr(offs), hip.ptr(tabs), F, H, W, 0x22, int(ends[-1]), n_int, sub_bits, rounds,
                                            hip.ptr(ws[G:]), wsb, hip.ptr(out[G:]), hip.ptr(st[G:]), hip.stream()))
        torch.cuda.synchronize()
        for t, v, n in ((ws, 0xA5, wsb), (out, 0x5A, F * H * W * 3), (st, 0x3C, F)):
            assert bool((t[:G] == v).all()) and bool((t[G + n:] == v).all())
        s = st[G:G + F].cpu().numpy()
        assert list(s & 1) == [0, 0, 0, 1]
        img = out[G:G + F * H * W * 3].view(F, H, W, 3)
        for i in range(3):
            assert torch.equal(img[i].cpu(), torch.from_numpy(X.pil_bgr(files[i])))


def _write_sequence(tmp_path, T, H, W):
    os.makedirs(str(tmp_path / "img"), exist_ok=True)
    paths = []
    for t in range(T):
        p = str(tmp_path / "img" / ("%05d.jpg" % t))
        with open(p, "wb") as fh:
            fh.write(X.encode(X.content(H, W, 100 + t), 2, 90))
        paths.append(p)
    return paths


def test_forward_from_paths_device_decode_equals_host(tmp_path):
    from stemseg_amd import config
    from stemseg_amd.modeling.inference_model import InferenceModel
    from tests import synth
    config.load_preset("davis")
    try:
        config.cfg.MODEL.BACKBONE.TYPE = "R-50-FPN"
        model = InferenceModel()
        names = [(k, v.shape) for k, v in model._model.state_dict().items()]
        sd = synth.synth_state_dict(names, 7)
        model._model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(model._model.state_dict()[k].shape) for k, v in sd.items()})
        model = model.cuda()
        paths = _write_sequence(tmp_path, 12, 240, 432)
        subseq = [list(range(0, 8)), list(range(4, 12))]
        assert torch.equal(InferenceModel.load_images(paths, "cuda").cpu(), torch.from_numpy(np.stack(InferenceModel.load_images(paths))))
        outs = []
        for flag in (True, False):
            model.device_decode = flag
            o = model(paths, subseq)
            torch.cuda.synchronize()
            outs.append(o)
        a, b = outs
        assert len(a["embeddings"]) == len(b["embeddings"]) == 2
        for ea, eb in zip(a["embeddings"], b["embeddings"]):
            assert ea.subseq_frames == eb.subseq_frames
            for k in ("embeddings", "bandwidths", "seediness"):
                assert torch.equal(getattr(ea, k), getattr(eb, k)), k
        for k in ("fg_masks", "multiclass_masks"):
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), k
    finally:
        config.load_preset("defaults")


def test_writer_vis_identical_either_way(tmp_path):
    from stemseg_amd import config
    from stemseg_amd.inference.output_utils import DavisOutputGenerator
    from stemseg_amd.utils.video_dataset import GenericVideoSequence
    from tests import test_gpu_writers as Wr
    from tests.test_gpu_vis import _tree
    rs = np.random.RandomState(41)
    T, h, w, ih, iw = 18, 24, 32, 90, 120
    try:
        config.cfg.INPUT.MIN_DIM, config.cfg.INPUT.MAX_DIM = 96, 128
        maps, logits, am, idx, lab, counts, life = Wr._sequence(rs, T, h, w, 7, 5)
        paths = [os.path.relpath(p, str(tmp_path)) for p in _write_sequence(tmp_path, T, ih, iw)]
        seq = GenericVideoSequence(dict(id="seq3", height=ih, width=iw, image_paths=paths), str(tmp_path))
        trees = []
        for flag in (True, False):
            out = str(tmp_path / ("out%d" % flag))
            gen = DavisOutputGenerator(out, -1, True)
            gen.device_decode = flag
            gen.process_sequence(seq, idx, lab, counts, life, None, (h, w), 4.0, 5, device="cuda:0")
            trees.append(_tree(out))
        assert any(k.startswith("vis" + os.sep) for k in trees[0])
        assert trees[0] == trees[1]
    finally:
        config.load_preset("defaults")


def test_cv2_equals_device_decode(hip):
    cv2 = pytest.importorskip("cv2")
    files = X.matrix([(17, 33), (240, 432)])
    out, _ = hip.jpeg_decode([d for _, d in files])
    for i, (label, data) in enumerate(files):
        ref = cv2.imdecode(np.frombuffer(data, np.uint8), cv2.IMREAD_COLOR)
        assert torch.equal(out[i].cpu(), torch.from_numpy(ref)), label
