"""Host tests of the argument checks of the four entry points that read COCO RLE strings (csrc/data_loader.hip): ``rle_decode``,
``rle_decode_union``, ``rle_decode_labels`` and ``rle_pair_inter``, on argument sets that break TWO OR MORE rules at once.  The checks
have an order -- the dimensions, ``rle_decode``'s one string per plane, the 2^31 plane, the characters, the null pointers, the
alignment, the ends of the offsets, then string by string the offsets and whatever the entry point asks of that string, the pairs, and
last the workspace -- and the first rule broken in that order is the one reported, so every case names the message it expects.  No
device call: the addresses are made up and every call is refused before any HIP call.

``CASES`` is also what a tool can run through two builds of the library to compare their answers line by line."""
import ctypes as C

import numpy as np
import pytest

from tests import data_oracle as do
from tests import writer_oracle as wo

FAKE, ODD = 0x1000, 0x1004          # never dereferenced; ODD is 4-byte but not 8-byte aligned
ENTRIES = ("rle_decode", "rle_decode_union", "rle_decode_labels", "rle_pair_inter")
PLANE_ENTRIES = ENTRIES[:3]
BIG = dict(H=65536, W=32768)        # 2^31 pixels
BAD_OFFS = (0, 4, 2, 9)             # decrease at string 1


def call(lib, entry, **kw):
    """One call of ``stemseg_hip_<entry>`` on three strings of 4, 2 and 3 characters for three 7 x 5 planes (or two pairs), every address
    made up; ``kw`` replaces arguments.  -> (rc, message)."""
    a = dict(chars=FAKE, n=9, offs=(0, 4, 6, 9), planes=(0, 1, 2), labels=(1, 2, 3), pairs=((0, 1), (2, 2)), offs_dev=FAKE, planes_dev=FAKE,
             labels_dev=FAKE, pairs_dev=FAKE, M=3, P=3, K=2, H=7, W=5, ws=FAKE, ws_bytes=1 << 30, out=FAKE, overlap=FAKE, area=FAKE, inter=FAKE,
             status=FAKE)
    assert set(kw) <= set(a), kw
    a.update(kw)
    i64 = lambda v: None if v is None else (C.c_int64 * len(v))(*v)
    i32 = lambda v: None if v is None else (C.c_int32 * max(len(v), 1))(*v)
    offs, planes, labels = i64(a["offs"]), i32(a["planes"]), i32(a["labels"])
    pairs = i32(None if a["pairs"] is None else [v for p in a["pairs"] for v in p])
    fn = getattr(lib, "stemseg_hip_" + entry)
    if entry == "rle_decode_labels":
        rc = fn(a["chars"], a["n"], offs, planes, labels, a["offs_dev"], a["planes_dev"], a["labels_dev"], a["M"], a["P"], a["H"], a["W"], a["ws"],
                a["ws_bytes"], a["out"], a["overlap"], a["status"], None)
    elif entry == "rle_pair_inter":
        rc = fn(a["chars"], a["n"], offs, pairs, a["offs_dev"], a["pairs_dev"], a["M"], a["K"], a["H"], a["W"], a["ws"], a["ws_bytes"], a["area"],
                a["inter"], a["status"], None)
    else:
        rc = fn(a["chars"], a["n"], offs, planes, a["offs_dev"], a["planes_dev"], a["M"], a["P"], a["H"], a["W"], a["ws"], a["ws_bytes"], a["out"],
                a["status"], None)
    return rc, lib.stemseg_hip_last_error().decode()


def _cases():
    """[(entry, arguments, a distinctive part of the message)]"""
    out = []
    for e in PLANE_ENTRIES:
        out += [(e, dict(planes=(7, 1, 2), offs=BAD_OFFS), "string 0 names plane 7 of 3"),          # string 0's plane before string 1's offsets
                (e, dict(planes=(0, 1, 7), offs=BAD_OFFS), "offsets decrease at string 1"),         # and the reverse
                (e, dict(planes=(0, 7, 2), offs=BAD_OFFS), "offsets decrease at string 1"),         # at one string: its offsets first
                (e, dict(planes=(0, 1, -1), offs=(0, -1, 6, 9)), "offsets decrease at string 0"),
                (e, dict(P=0, **BIG), "bad dims M=3 P=0"),
                (e, dict(n=1 << 30, **BIG), "65536 x 32768 exceeds 2^31"),
                (e, dict(n=-1, chars=None), "n_chars=-1 out of range"),
                (e, dict(out=None, offs_dev=ODD), "null pointer"),
                (e, dict(status=None, planes_dev=0x1002, offs=(1, 4, 6, 9)), "null pointer"),
                (e, dict(offs_dev=ODD, offs=(0, 4, 6, 8)), "8-byte aligned"),
                (e, dict(planes_dev=0x1002, offs=BAD_OFFS), "8-byte aligned"),
                (e, dict(offs=(0, 4, 6, 8), planes=(7, 1, 2)), "offsets must run from 0 to n_chars=9"),
                (e, dict(offs=(1, 4, 2, 9), planes=(7, 1, 2)), "offsets must run from 0 to n_chars=9")]
    e = "rle_decode"
    out += [(e, dict(P=2, **BIG), "3 strings for 2 planes"),                                        # M > P before the 2^31 plane
            (e, dict(P=2, H=0), "bad dims M=3 P=2 H=0"),
            (e, dict(P=2, n=-1), "3 strings for 2 planes"),
            (e, dict(planes=(1, 1, 2), offs=BAD_OFFS), "offsets decrease at string 1"),
            (e, dict(planes=(1, 1, 2), offs=(0, 4, 6, 5), n=5), "plane 1 is named by two strings"),
            (e, dict(planes=(1, 1, 9)), "plane 1 is named by two strings"),
            (e, dict(planes=(1, 9, 1)), "string 1 names plane 9 of 3"),
            (e, dict(planes=(2, 0, 2), offs=(0, 4, 6, 5), n=5), "offsets decrease at string 2")]            # at one string: its offsets first
    for e in ("rle_decode_union", "rle_decode_labels"):
        out += [(e, dict(planes=(1, 0, 7)), "plane indices decrease at string 1 (0 after 1)"),
                (e, dict(planes=(1, -1, 2)), "string 1 names plane -1 of 3"),                       # at one string: the range before the order
                (e, dict(planes=(2, 1, 0), offs=(0, 4, 6, 5), n=5), "plane indices decrease at string 1 (1 after 2)"),
                (e, dict(planes=(2, 1, 0), offs=(0, 4, 3, 9)), "offsets decrease at string 1")]
    e = "rle_decode_labels"
    out += [(e, dict(planes=(1, 0, 2), labels=(1, 0, 3)), "plane indices decrease at string 1 (0 after 1)"),      # at one string: the order before the label
            (e, dict(planes=(1, 0, 2), labels=(0, 2, 3)), "string 0 has label 0"),                                  # at different strings: the earlier string
            (e, dict(planes=(1, 0, 2), labels=(1, 2, 65536)), "plane indices decrease at string 1 (0 after 1)"),
            (e, dict(planes=(0, 1, 7), labels=(1, 70000, 3)), "string 1 has label 70000"),
            (e, dict(labels=(1, 2, 0), offs=BAD_OFFS), "offsets decrease at string 1"),
            (e, dict(labels=(0, 2, 3), offs=BAD_OFFS), "string 0 has label 0"),
            (e, dict(labels_dev=0x1002, out=0x1001), "plane indices and labels 4-byte aligned"),
            (e, dict(out=0x1001, offs=(0, 4, 6, 8)), "misaligned maps"),
            (e, dict(overlap=0x1002, labels=(0, 0, 0)), "misaligned maps"),
            (e, dict(overlap=None, out=0x1001), "null pointer"),
            (e, dict(labels=None, labels_dev=0x1002), "null pointer")]
    e = "rle_pair_inter"
    out += [(e, dict(offs=BAD_OFFS, pairs=((0, 3), (1, 1))), "offsets decrease at string 1"),       # every offset before any pair
            (e, dict(offs=(0, 4, 6, 5), n=5, pairs=((0, 3), (1, 1))), "offsets decrease at string 2"),
            (e, dict(pairs=((0, 3), (-1, 0))), "pair 0 names strings (0, 3) of 3"),
            (e, dict(pairs=((0, 2), (-1, 3))), "pair 1 names strings (-1, 3) of 3"),
            (e, dict(K=-1, **BIG), "bad dims M=3 n_pairs=-1"),
            (e, dict(n=1 << 30, **BIG), "65536 x 32768 exceeds 2^31"),
            (e, dict(n=-1, ws=None), "n_chars=-1 out of range"),
            (e, dict(inter=None, offs_dev=ODD), "null pointer"),
            (e, dict(area=None, pairs_dev=0x1002), "null pointer"),
            (e, dict(offs_dev=ODD, pairs_dev=0x1002), "offsets must be 8-byte aligned"),
            (e, dict(pairs_dev=0x1002, offs=(0, 4, 6, 8)), "misaligned pairs, area or inter"),
            (e, dict(area=0x1002, offs=BAD_OFFS), "misaligned pairs, area or inter"),
            (e, dict(offs=(0, 4, 6, 8), pairs=((0, 3), (1, 1))), "offsets must run from 0 to n_chars=9")]
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def lib():
    from stemseg_amd import hip
    return hip.lib()


def test_the_calls_pass_every_check_but_the_workspace(lib):
    """The arguments the cases start from break no rule: with a workspace too small they are refused for that alone -- the last check."""
    for entry in ENTRIES:
        rc, msg = call(lib, entry, ws_bytes=16)
        assert rc == -1 and msg.startswith(entry + ": workspace 16 bytes < "), (entry, msg)


@pytest.mark.parametrize("ws_bytes", [1 << 30, 16], ids=["workspace_ok", "workspace_short"])
@pytest.mark.parametrize("k", range(len(CASES)), ids=["%s-%d" % (c[0], k) for k, c in enumerate(CASES)])
def test_the_first_rule_broken_is_the_one_reported(lib, k, ws_bytes):
    entry, kw, word = CASES[k]
    rc, msg = call(lib, entry, ws_bytes=ws_bytes, **kw)
    assert rc == -1, (entry, kw)
    assert msg.startswith(entry + ": ") and word in msg, (entry, kw, msg)


def test_mask_string_is_the_plain_encoder():
    """``data_oracle.mask_string`` takes its run lengths from numpy; the plain loop of ``writer_oracle.encode`` must give the same strings."""
    rs = np.random.RandomState(3)
    masks = [np.zeros((7, 5), np.uint8), np.ones((7, 5), bool), np.ones((1, 1), np.uint8), np.zeros((1, 1), np.uint8), do.checkerboard(),
             do.blobs(33, 21, 3, 1), 2 * do.blobs(20, 30, 2, 2), (rs.rand(40, 1) < 0.5), (rs.rand(1, 40) < 0.5), (rs.rand(24, 25) < 0.3).astype(np.float32)]
    masks += [m for _, _, _, ms in do.rle_small_cases() for m in ms]
    for m in masks:
        assert do.mask_string(m) == wo.counts_to_string(wo.encode(m)), m.shape
