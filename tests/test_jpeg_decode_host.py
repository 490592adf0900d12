"""CPU half of the device JPEG decoder: the marker parser and its device / host classification, the table blob, the numpy
restatement of the decoder (tests/jpeg_decode_oracle.py) against PIL, and the C-ABI argument checks."""
import ctypes
import io

import numpy as np
import pytest

from stemseg_amd.utils import jpeg as J
from tests import jpeg_decode_oracle as O
from tests import jpeg_fixtures as X


@pytest.fixture(scope="module")
def small_matrix():
    return X.matrix(X.SMALL_SIZES)


def test_parser_classifies_the_matrix_for_the_device(small_matrix):
    want = {"L": J.SAMPLING_GRAY, 0: J.SAMPLING_444, 1: J.SAMPLING_422, 2: J.SAMPLING_420}
    for label, data in small_matrix + X.matrix([(240, 432), (1080, 1920)], qualities=[75], subs=["L", 2]):
        info = J.parse(data)
        assert info.device, (label, info)
        H, W = (int(v) for v in label.split()[0].split("x"))
        assert (info.H, info.W) == (H, W), label
        sub = label.split()[-1]
        if sub in ("L", "0", "1", "2"):
            assert info.sampling == want[sub if sub == "L" else int(sub)], label
        assert data[info.ecs_end:] == b"\xff\xd9" and b"\xff\xda" in data[:info.ecs_begin]
        if "rst" in label:
            assert info.restart > 0, label


def test_parser_sends_other_files_to_the_host():
    base = X.encode(X.content(17, 33, 0), 2, 80)
    cases = {
        "progressive": X.progressive(),
        "cmyk": X.cmyk(),
        "exif rotated": X.exif_rotated(),
        "no EOI": base[:-2],
        "truncated header": base[:40],
        "garbage": bytes(np.random.RandomState(0).randint(0, 256, 500).astype(np.uint8)),
        "empty": b"",
        "png": b"\x89PNG\r\n\x1a\n" + b"\x00" * 40,
        "trailing bytes": base + b"\x00\x00",
    }
    for name, data in cases.items():
        info = J.parse(data)
        assert not info.device, (name, info)
    assert J.parse(X.exif_rotated(orientation=1)).device


def test_table_blob_holds_the_dqt_and_dht_contents():
    data = X.encode(X.content(33, 15, 5), 2, 37, optimize=True)
    info = J.parse(data)
    b = J.table_blob(info)
    assert b.size == J.BLOB_BYTES == 7872
    hdr = b[:64].view(np.int32)
    assert hdr[0] == info.restart and hdr[1] == 3
    assert list(hdr[2:5]) == info.comp_dc and list(hdr[5:8]) == info.comp_ac and list(hdr[8:11]) == info.comp_q
    q = b[64:576].view(np.uint16).reshape(4, 64)
    from PIL import Image
    pq = Image.open(io.BytesIO(data)).quantization                  # natural order per table id
    for t, zz in pq.items():
        assert [int(v) for v in q[t]] == list(zz)
    for (tc, th), (bits, vals) in info.huff.items():
        o = 576 + (4 * tc + th) * J.HUFF_BYTES
        look = b[o:o + 512].view(np.uint16)
        maxcode = b[o + 512:o + 584].view(np.int32)
        valoff = b[o + 584:o + 656].view(np.int32)
        hv = b[o + 656:o + 912]
        code, k = 0, 0                                               # every code decodes to its symbol through the blob
        for l in range(1, 17):
            for _ in range(bits[l - 1]):
                if l <= 8:
                    for pad in range(1 << (8 - l)):
                        e = int(look[(code << (8 - l)) | pad])
                        assert e >> 8 == l and e & 255 == vals[k]
                else:
                    assert int(look[code >> (l - 8)]) == 0
                    assert code <= maxcode[l] and hv[code + valoff[l]] == vals[k]
                code += 1
                k += 1
            code <<= 1


def test_oracle_equals_pil_on_the_device_matrix(small_matrix):
    for label, data in small_matrix + X.matrix([(240, 432)], qualities=[1, 75, 100], subs=["L", 1, 2]):
        out, ok = O.decode(data)
        assert ok, label
        assert np.array_equal(out, X.pil_bgr(data)), label


def test_oracle_flags_corrupt_files():
    data = X.encode(X.content(64, 80, 9), 2, 90)
    for bad in (X.truncated(data), X.bad_code(data)):
        assert J.parse(bad).device
        out, ok = O.decode(bad)
        assert not ok and out is None
    rst = X.encode(X.content(64, 80, 9), 0, 90, restart_marker_blocks=2)
    i = rst.index(b"\xff\xd1")
    swapped = rst[:i] + b"\xff\xd2" + rst[i + 2:]                      # RST1 -> RST2: out of sequence
    assert not O.decode(swapped)[1]


def test_cabi_jpeg_decode_argument_errors():
    from stemseg_amd import hip
    l = hip.lib()
    for n in ("stemseg_hip_jpeg_decode_workspace_bytes", "stemseg_hip_jpeg_decode"):
        assert hasattr(ctypes.CDLL(hip.LIB_PATH), n) and n in hip.SIGNATURES, n
    wsb = l.stemseg_hip_jpeg_decode_workspace_bytes
    assert wsb(0, 8, 8, 0x22, 100, 1, 0) == 0
    assert wsb(1, 8, 8, 0x12, 100, 1, 0) == 0                        # h1v2: not supported
    assert wsb(1, 8, 8, 0x22, 100, 0, 0) == 0                        # fewer intervals than frames
    assert wsb(1, 8, 8, 0x22, 100, 1, 96) == 0                       # sub_bits not a multiple of 64
    assert wsb(1, 70000, 8, 0x22, 100, 1, 0) == 0
    ws = wsb(2, 9, 17, 0x22, 1000, 2, 0)
    assert ws > 0 and wsb(2, 9, 17, 0x22, 100000, 2, 0) > ws and wsb(2, 9, 17, 0x22, 100000, 2, 64) > wsb(2, 9, 17, 0x22, 100000, 2, 0)
    fake = ctypes.c_void_p(0x1000)                                    # never dereferenced: every call below fails its argument check
    dec = lambda F=2, H=9, W=17, s=0x22, nb=ws, data=fake, sub=0, rounds=0, out=fake: l.stemseg_hip_jpeg_decode(
        data, fake, fake, F, H, W, s, 1000, 2, sub, rounds, fake, nb, out, fake, None)
    assert dec(F=0) == -1 and b"bad dims" in l.stemseg_hip_last_error()
    assert dec(W=70000) == -1 and b"bad dims" in l.stemseg_hip_last_error()
    assert dec(s=0x12) == -1 and b"sampling" in l.stemseg_hip_last_error()
    assert dec(sub=100) == -1 and b"sub_bits" in l.stemseg_hip_last_error()
    assert dec(rounds=-1) == -1 and b"max_rounds" in l.stemseg_hip_last_error()
    assert dec(data=None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert dec(out=None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert dec(nb=ws - 1) == -1 and b"workspace" in l.stemseg_hip_last_error()
