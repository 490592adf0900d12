"""CPU half of the device PNG decoder: the chunk walker and its device / host classification, the header blob, the numpy
restatement of the decoder (tests/png_decode_oracle.py) against zlib and PIL, and the C-ABI argument checks."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

from stemseg_amd.utils import png as P
from tests import png_decode_oracle as O
from tests import png_fixtures as X


@pytest.fixture(scope="module")
def small_matrix():
    return X.matrix(X.SMALL_SIZES)


def test_parser_classifies_the_matrix_for_the_device(small_matrix):
    for label, data in small_matrix:
        info = P.parse(data)
        assert info.device, (label, info)
        assert zlib.decompress(P.stream(info, data)), label


def test_parser_sends_other_files_to_the_host():
    for label, data in X.host_files():
        info = P.parse(data)
        assert not info.device and info.reason, label
    for junk in (b"", b"\x89PNG", X.SIGNATURE + b"\0" * 30, b"\xff\xd8\xff\xe0", X.write(X.pixels(3, 4, 2, 0), 2)[:-5]):
        assert not P.parse(junk).device
    px = X.pixels(5, 6, 2, 0)
    s = X.compress(X.filter_rows(px, [0] * 5))
    unknown = X.assemble(5, 6, 2, s, extra_before=[(b"ABCD", b"x")])
    assert "critical" in P.parse(unknown).reason
    ancillary = X.assemble(5, 6, 2, s, extra_before=[(b"tEXt", b"k\x00v"), (b"gAMA", struct.pack(">I", 45455))])
    assert P.parse(ancillary).device
    assert not P.parse(X.assemble(5, 6, 2, s, extra_before=[(b"eXIf", b"MM\x00*")])).device
    assert not P.parse(X.assemble(5, 6, 0, s, extra_before=[(b"PLTE", b"\0" * 6)])).device


def test_header_blob_holds_what_the_parser_read():
    files = [X.write(X.pixels(7, 9, 2, s), 2, None, s, idat_size=[None, 5, 1][s]) for s in range(3)]
    infos = [P.parse(f) for f in files]
    hdr, recs = P.header_blob(infos)
    assert hdr.shape == (3, P.HDR_WORDS) and hdr.dtype == np.int64 and recs.dtype == np.uint32
    first = 0
    for f, (data, info) in enumerate(zip(files, infos)):
        s = P.stream(info, data)
        assert list(hdr[f, :6]) == [7, 9, 3, len(s), first, len(info.idat)]
        off = 0
        for k in range(len(info.idat)):
            o, n, crc, fr = (int(v) for v in recs[first + k])
            assert (o, fr) == (off, f) and crc == zlib.crc32(b"IDAT" + s[o:o + n])
            off += n
        assert off == len(s)
        first += len(info.idat)
    assert recs.shape == (first, 4)


def test_parser_never_raises_on_mangled_files():
    rs = np.random.RandomState(3)
    good = X.write(X.pixels(11, 13, 6, 1), 6, None, 1, idat_size=40)
    for _ in range(300):
        d = bytearray(good)
        for _ in range(rs.randint(1, 4)):
            d[rs.randint(len(d))] = rs.randint(256)
        P.parse(bytes(d[:rs.randint(1, len(d) + 1)]))


def _multi_block():
    """Small files of several blocks: 128-symbol blocks (memLevel 1), fixed blocks, sync / full flushes (empty stored blocks),
    stored blocks (level 0), Z_RLE runs (dist = 1 chains), every filter type and colour type."""
    out = []
    for ct in (0, 2, 4, 6):
        px = X.pixels(12, 19, ct, ct)
        out.append(("ct%d memLevel 1" % ct, X.write(px, ct, None, ct, mem_level=1)))
    px = X.pixels(12, 19, 2, 7)
    n = 12 * (1 + 19 * 3)
    out.append(("fixed", X.write(px, 2, None, 1, strategy=zlib.Z_FIXED)))
    out.append(("rle memLevel 1", X.write(px, 2, None, 2, strategy=zlib.Z_RLE, mem_level=1)))
    out.append(("flushes", X.write(px, 2, None, 3, mem_level=1, flush_at=[n // 4, n // 2], flush_mode=zlib.Z_FULL_FLUSH)))
    out.append(("stored", X.write(px, 2, None, 4, level=0, idat_size=7)))
    out.append(("wbits 9", X.write(px, 2, None, 5, wbits=9, mem_level=1)))
    out.append(("pil", X.pil_png(px)))
    return out


def test_oracle_equals_zlib_and_pil_on_multi_block_files():
    """Finder, speculative decode, chain, write pass and pointer jumping give zlib's bytes; the unfilter gives PIL's pixels.  The
    finder finds every dynamic block (the backstop takes only stored and fixed ones), and the backstop alone gives the same."""
    from stemseg_amd.utils import png as P
    multi = 0
    for label, data in _multi_block():
        info = P.parse(data)
        s = P.stream(info, data)
        raw, st = O.inflate(s, info.H * (1 + info.W * info.channels))
        assert raw == zlib.decompress(s), (label, st)
        multi += st["blocks"] > 1
        assert O.inflate(s, len(raw), use_finder=False)[0] == raw, label
        img, st = O.decode_png(data)
        assert img is not None and np.array_equal(img, X.pil_bgr(data)), (label, st)
    assert multi >= 6


def test_oracle_finder_finds_every_dynamic_block():
    from stemseg_amd.utils import png as P
    for H, W in ((24, 40), (20, 64)):
        data = X.write(X.pixels(H, W, 2, 3), 2, None, 3, mem_level=1)       # 128-symbol blocks, dynamic and fixed
        info = P.parse(data)
        s = P.stream(info, data)
        raw, st = O.inflate(s, info.H * (1 + info.W * 3))
        assert raw == zlib.decompress(s), st
        assert st["blocks"] > 20 and st["candidates"] >= 6 and st["missed_dynamic"] == 0 and st["jump_rounds"] >= 1, st


def test_oracle_flags_corrupt_files():
    for label, data in X.corrupt_files():
        img, why = O.decode_png(data)
        assert img is None, label


def test_cabi_png_decode_argument_errors():
    from stemseg_amd import hip
    l = hip.lib()
    for n in ("stemseg_hip_png_decode_workspace_bytes", "stemseg_hip_png_decode"):
        assert hasattr(ctypes.CDLL(hip.LIB_PATH), n) and n in hip.SIGNATURES, n
    wsb = l.stemseg_hip_png_decode_workspace_bytes
    assert wsb(0, 8, 8, 3, 100, 0, 0) == 0
    assert wsb(1, 8, 8, 5, 100, 0, 0) == 0                           # channels
    assert wsb(1, 8, 8, 3, -1, 0, 0) == 0
    assert wsb(1, 8, 8, 3, 100, 0, 2) == 0                           # unknown flag
    assert wsb(1, 8, 8, 3, 100, 96, 0) == 0                          # sub_bits not a multiple of 64
    assert wsb(1, 70000, 8, 3, 100, 0, 0) == 0
    assert wsb(1, 65535, 65535, 4, 100, 0, 0) == 0                   # a frame's inflated bytes beyond int32
    ws = wsb(2, 9, 17, 3, 1000, 0, 0)
    assert ws > 0 and wsb(2, 9, 17, 3, 100000, 0, 0) > ws and wsb(3, 9, 17, 3, 1000, 0, 0) > ws and wsb(2, 9, 17, 3, 1000, 64, 1) == ws
    fake = ctypes.c_void_p(0x1000)                                    # never dereferenced: every call below fails its argument check
    dec = lambda F=2, H=9, W=17, C=3, nb=ws, data=fake, sub=0, flags=0, out=fake: l.stemseg_hip_png_decode(
        data, fake, fake, F, H, W, C, 1000, sub, flags, fake, nb, out, fake, None)
    assert dec(F=0) == -1 and b"bad dims" in l.stemseg_hip_last_error()
    assert dec(W=70000) == -1 and b"bad dims" in l.stemseg_hip_last_error()
    assert dec(C=0) == -1 and b"channels" in l.stemseg_hip_last_error()
    assert dec(flags=4) == -1 and b"flags" in l.stemseg_hip_last_error()
    assert dec(sub=100) == -1 and b"sub_bits" in l.stemseg_hip_last_error()
    assert dec(data=None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert dec(out=None) == -1 and b"null pointer" in l.stemseg_hip_last_error()
    assert dec(nb=ws - 1) == -1 and b"workspace" in l.stemseg_hip_last_error()
