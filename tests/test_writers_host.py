"""CPU tests of the YouTube-VIS / KITTI-MOTS writers' host side: the COCO RLE string codec, area and bbox (restated from
pycocotools 2.0 ``maskApi.c`` semantics in tests/writer_oracle.py), the KITTI-MOTS track filters of ``save()``, and the C-ABI
of the ABI-11 entry points (argument errors are reported before any GPU call)."""
import ctypes
import os

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from tests import writer_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _product_rle():
    from stemseg_amd.inference.output_utils import coco_rle
    return coco_rle


# ------------------------------------------------------------------------------------------------ string codec
@pytest.mark.parametrize("counts, s", [([4], "4"), ([1, 3], "13"), ([0, 100], "0T3"), ([0], "0"),
                                       # 16 = 0x10: one group would read as negative, so a second group follows
                                       ([16], "`0"), ([15], "?"), ([31], "o0"),
                                       # i > 2 sends deltas: count 3 -> 1 - 3 = -2 = group 0x1e, x == -1 after it: "N"
                                       ([2, 3, 4, 1, 5], "234N1"), ([0, 1, 0, 1, 0], "01000")])
def test_rle_string_hand_vectors(counts, s):
    assert wo.counts_to_string(counts) == s
    assert wo.string_to_counts(s) == counts
    assert _product_rle().string_to_counts(s).tolist() == counts


def test_rle_string_negative_deltas():
    # (count 3 minus count 1 when i = 3; i = 2 is sent whole: the quirk of "i > 2")
    counts = [0, 50, 3, 1, 7, 40]
    s = wo.counts_to_string(counts)
    assert wo.string_to_counts(s) == counts and _product_rle().string_to_counts(s).tolist() == counts
    assert wo.counts_to_string([0, 64, 1, 0]) != wo.counts_to_string([0, 64, 1, 64])


@settings(max_examples=150, deadline=None)
@given(st.integers(1, 9), st.integers(1, 9), st.integers(0, 2 ** 32 - 1))
def test_rle_encode_decode_round_trip(h, w, seed):
    rs = np.random.RandomState(seed)
    mask = rs.rand(h, w) < rs.rand()
    counts = wo.encode(mask)
    assert sum(counts) == h * w and all(c > 0 for c in counts[1:])
    assert np.array_equal(wo.decode(counts, h, w), mask)
    s = wo.counts_to_string(counts)
    assert wo.string_to_counts(s) == counts
    assert _product_rle().string_to_counts(s).tolist() == counts
    assert wo.area(counts) == int(mask.sum()) == _product_rle().area(counts)
    assert _product_rle().to_bbox(counts, h) == wo.to_bbox(counts, h)


@settings(max_examples=100, deadline=None)
@given(st.lists(st.integers(0, 3000), min_size=1, max_size=12))
def test_rle_string_round_trip_any_counts(counts):
    s = wo.counts_to_string(counts)
    assert wo.string_to_counts(s) == counts and _product_rle().string_to_counts(s).tolist() == counts


def test_bbox_quirks():
    h, w = 4, 3
    assert wo.to_bbox(wo.encode(np.zeros((h, w), bool)), h) == [0, 0, 0, 0]              # empty: counts [12], m = 0
    m = np.zeros((h, w), bool)
    m[1:3, 1] = True
    assert wo.to_bbox(wo.encode(m), h) == [1, 1, 1, 2]
    m = np.zeros((h, w), bool)
    m[3, 0] = m[0, 1] = True                          # one run crossing the column boundary: y spans the full height
    assert wo.to_bbox(wo.encode(m), h) == [0, 0, 2, 4]
    m = np.zeros((h, w), bool)
    m[3, 0] = m[1, 1] = True                          # two runs in two columns: the true box
    assert wo.to_bbox(wo.encode(m), h) == [0, 1, 2, 3]
    full = np.ones((h, w), bool)
    assert wo.encode(full) == [0, 12] and wo.to_bbox([0, 12], h) == [0, 0, 3, 4]
    assert wo.to_bbox([2, 3, 7], h) == wo.to_bbox([2, 3], h) == [0, 0, 2, 4]            # odd count list: the last run is dropped (pixels 2..4 cross a column)
    assert wo.to_bbox([1, 2, 9], h) == [0, 1, 1, 2]
    for c in ([12], [0, 12], [2, 3, 7], [5, 1, 6], [3, 2, 7]):
        assert _product_rle().to_bbox(c, h) == wo.to_bbox(c, h)


# ------------------------------------------------------------------------------------------------ KITTI-MOTS filters
def _line(frame, tid, cat, h, w, mask):
    return "%d %d %d %d %d %s" % (frame, tid, cat, h, w, wo.counts_to_string(wo.encode(mask)))


def test_kitti_save_filters_vs_restatement(tmp_path):
    from stemseg_amd.inference.output_utils.generators import KittiMOTSOutputGenerator
    rs = np.random.RandomState(5)
    h, w = 40, 60
    files = {}
    for seq in (0, 7):
        lines = []
        for n in range(1, 9):
            cat = 1 + (n % 2)
            big = n % 3 != 0
            for t in range(int(rs.randint(1, 16))):
                if rs.rand() < 0.25:
                    continue                                                        # time breaks
                m = np.zeros((h, w), bool)
                y, x = rs.randint(0, 20), rs.randint(0, 30)
                sz = (rs.randint(14, 20), rs.randint(14, 30)) if big else (rs.randint(2, 12), rs.randint(2, 12))
                m[y:y + sz[0], x:x + sz[1]] = True
                if rs.rand() < 0.3:
                    m &= rs.rand(h, w) < 0.5                                        # sparse: a low area / bbox ratio
                lines.append(_line(t, cat * 1000 + n, cat, h, w, m))
        files[seq] = lines
        os.makedirs(str(tmp_path / "out" / "results"), exist_ok=True)
        with open(str(tmp_path / "out" / "results" / ("%04d.txt" % seq)), "w") as fh:
            fh.writelines(l + "\n" for l in lines)
    with open(str(tmp_path / "out" / "results" / "notes.txt"), "w") as fh:        # not ????.txt: ignored
        fh.write("x")
    gen = KittiMOTSOutputGenerator(str(tmp_path / "out"), -1, False)
    gen.save()
    outs = sorted(os.listdir(str(tmp_path / "out" / "results_nms")))
    assert outs == ["0000.txt", "0007.txt"]
    n_kept = 0
    for seq, lines in files.items():
        got = open(str(tmp_path / "out" / "results_nms" / ("%04d.txt" % seq))).read().splitlines()
        ref = wo.kitti_filter_lines(lines)
        assert got == ref
        n_kept += len(got)
        assert len(got) < len(lines)
    assert n_kept > 0


# ------------------------------------------------------------------------------------------------ C-ABI (ABI 11)
def test_cabi_abi11_symbols_exported():
    from stemseg_amd import hip
    assert hip.ABI_VERSION == 11
    hdr = open(os.path.join(ROOT, "include", "stemseg_hip.h")).read()
    assert "#define STEMSEG_HIP_ABI_VERSION 11" in hdr
    lib = ctypes.CDLL(hip.LIB_PATH)
    for n in ("stemseg_hip_scatter_instance_index_ex", "stemseg_hip_resample_instance_masks_ex", "stemseg_hip_rle_workspace_bytes",
              "stemseg_hip_rle_plan", "stemseg_hip_rle_encode", "stemseg_hip_instance_class_stats"):
        assert hasattr(lib, n) and n in hip.SIGNATURES, n
    assert hip.lib().stemseg_hip_version() == 11


def test_cabi_abi11_argument_errors():
    from stemseg_amd import hip
    l = hip.lib()
    fake = ctypes.c_void_p(0x1000)                      # never dereferenced: every call below fails its argument check first
    assert l.stemseg_hip_scatter_instance_index_ex(None, None, None, 0, None, 0, fake, 3, 4, 4, None) == -1
    assert b"index_bytes" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_resample_instance_masks_ex(fake, 4, 4, 4, 4.0, 8, 8, 8, 8, fake, None) == -1
    assert b"index_bytes" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_resample_instance_masks_ex(fake, 2, 4, 4, 4.0, 20, 8, 8, 8, fake, None) == -1
    assert b"padded dims" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_rle_workspace_bytes(0, 4, 4, 1, 10) == 0
    assert l.stemseg_hip_rle_workspace_bytes(1, 4, 4, 1, 0) == 0
    ws = l.stemseg_hip_rle_workspace_bytes(2, 4, 4, 3, 64)
    assert ws > 0 and l.stemseg_hip_rle_workspace_bytes(2, 4, 4, 3, 4096) > ws
    args = lambda ib, K, cap, nbytes: (fake, ib, 2, 4, 4, K, cap, fake, nbytes, fake, fake, fake, None)
    assert l.stemseg_hip_rle_plan(*args(3, 3, 64, ws)) == -1 and b"index_bytes" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_rle_plan(*args(1, 256, 64, ws)) == -1 and b"does not fit" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_rle_plan(*args(1, 3, 64, ws - 1)) == -1 and b"workspace" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_rle_plan(*args(1, 3, 0, ws)) == -1 and b"max_changes" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_rle_encode(fake, 1, 2, 4, 4, 3, 64, fake, ws, None, fake, fake, fake, fake, fake, None) == -1
    assert b"null pointer" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_instance_class_stats(None, None, None, fake, 1, 0, None, 0, 0, 4, 4, None, 0, None, None, None, 0, fake, None,
                                              None) == -1
    assert b"bad dims" in l.stemseg_hip_last_error()
    assert l.stemseg_hip_instance_class_stats(None, None, None, fake, 1, 0, None, 0, 2, 4, 4, fake, 1, fake, fake, None, 0, fake, None,
                                              None) == -1
    assert b"C >= 2" in l.stemseg_hip_last_error()


def test_writers_accept_reference_constructor_arguments(tmp_path):
    from stemseg_amd.inference.output_utils import KittiMOTSOutputGenerator, YoutubeVISOutputGenerator
    y = YoutubeVISOutputGenerator(str(tmp_path / "y"), -1, True, {1: 1}, {1: "a"}, upscaled_inputs=False, keep_masks=False)
    assert not y.keep_masks and y.sequences == {} and os.path.isdir(str(tmp_path / "y"))
    y.save()                                            # no sequence yet: an empty result list, as the reference writes it
    assert open(str(tmp_path / "y" / "results.json")).read() == "[]"
    k = KittiMOTSOutputGenerator(str(tmp_path / "k"), -1, True)
    assert k.keep_masks
