"""Host half of the device JPEG decoder (``hip.jpeg_decode``, csrc/jpeg_decode.hip): the marker parser, the device / host
classification and the per-frame table blob.

Only the markers are walked here; the entropy-coded segment is never read on the host.  A file goes to the device when it is a
single-scan baseline (SOF0) or extended-sequential (SOF1) Huffman JPEG with 8-bit samples, one component (grayscale) or three
YCbCr components with luma sampling 1x1, 2x1 or 2x2 and chroma 1x1, an orientation of 1, and a final EOI.  Everything else --
progressive, arithmetic, lossless, 12-bit, CMYK, RGB (Adobe transform 0 or component ids 'R' 'G' 'B'), other samplings, a
rotating EXIF orientation, a missing SOS or EOI, bytes after the EOI, or anything the parser does not know -- goes to the host
loader, which then decides as it always did.

The table blob (``BLOB_BYTES`` bytes per frame, little-endian; the layout csrc/jpeg_decode.hip reads):
    [0, 64)       int32 hdr[16]: restart interval in MCUs (0 = none), components, DC table of component c (hdr[2 + c]),
                  AC table (hdr[5 + c]), quant table (hdr[8 + c]); the rest 0
    [64, 576)     uint16 quant[4][64], natural (row-major) order
    [576, ...)    8 Huffman tables, DC 0..3 then AC 0..3, HUFF_BYTES each:
                    uint16 look[256]   8-bit lookahead: (code length << 8) | symbol, 0 = the code is longer than 8 bits
                    int32  maxcode[18] largest code of length l (l = 1..16), -1 if none; maxcode[17] = 0x7FFFFFFF
                    int32  valoff[18]  index into vals of the first code of length l, minus that code
                    uint8  vals[256]
"""
import struct

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63]

HDR_BYTES = 64
QUANT_BYTES = 4 * 64 * 2
HUFF_BYTES = 512 + 72 + 72 + 256
BLOB_BYTES = HDR_BYTES + QUANT_BYTES + 8 * HUFF_BYTES

# sampling codes of the C-ABI: 0 = one component; (luma h << 4) | luma v for three YCbCr components with chroma 1x1
SAMPLING_GRAY, SAMPLING_444, SAMPLING_422, SAMPLING_420 = 0, 0x11, 0x21, 0x22


class JpegInfo(object):
    """What the parser learnt about one file.  ``device`` says whether the device decoder takes it; ``reason`` says why not."""

    def __init__(self):
        self.device = False
        self.reason = ""
        self.H = self.W = 0
        self.ncomp = 0
        self.sampling = None
        self.restart = 0
        self.ecs_begin = self.ecs_end = 0
        self.qt = [None] * 4                  # natural order, int
        self.huff = {}                        # (class 0 DC / 1 AC, id) -> (bits[16], vals)
        self.comp_q = []                      # per component, from SOF
        self.comp_dc = []                     # per component, from SOS
        self.comp_ac = []

    @property
    def geometry(self):
        return (self.H, self.W, self.sampling)

    def __repr__(self):
        return "JpegInfo(%s, %dx%d, sampling=%r, restart=%d%s)" % ("device" if self.device else "host", self.W, self.H, self.sampling,
                                                                  self.restart, "" if self.device else ", " + self.reason)


def _exif_orientation(p):
    """Orientation tag (0x0112) of IFD0 of an APP1 Exif payload; 1 when absent.  Raises ValueError on a malformed payload."""
    t = p[6:]
    if len(t) < 8 or t[:2] not in (b"II", b"MM"):
        raise ValueError("bad TIFF header")
    e = "<" if t[:2] == b"II" else ">"
    off = struct.unpack(e + "I", t[4:8])[0]
    n = struct.unpack(e + "H", t[off:off + 2])[0]
    for i in range(n):
        ent = t[off + 2 + 12 * i: off + 14 + 12 * i]
        if len(ent) < 12:
            raise ValueError("truncated IFD0")
        tag, typ, cnt = struct.unpack(e + "HHI", ent[:8])
        if tag == 0x0112:
            return struct.unpack(e + "H", ent[8:10])[0] if typ == 3 else -1
    return 1


def _check_huffman(bits, vals):
    code = 0
    for l in range(16):
        code += bits[l]
        if code > (1 << (l + 1)):
            return False
        code <<= 1
    return sum(bits) == len(vals) <= 256


def parse(data):
    """Marker parse of one file's bytes -> JpegInfo.  Never raises on bad data: such a file is classified for the host."""
    info = JpegInfo()
    try:
        _parse(bytes(data), info)
    except (IndexError, ValueError, struct.error) as ex:
        info.device, info.reason = False, "unparsable: %s" % ex
    return info


def _host(info, reason):
    info.device, info.reason = False, reason
    return info


def _parse(d, info):
    if d[:2] != b"\xff\xd8":
        return _host(info, "no SOI")
    i, n = 2, len(d)
    sof = None
    jfif = adobe = False
    adobe_transform = None
    while True:
        if i >= n or d[i] != 0xFF:
            return _host(info, "marker expected at byte %d" % i)
        while i < n and d[i] == 0xFF:
            i += 1
        if i >= n:
            return _host(info, "truncated marker")
        m = d[i]
        i += 1
        if m == 0xD9:
            return _host(info, "EOI before SOS")
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            return _host(info, "standalone marker 0x%02X outside a scan" % m)
        if i + 2 > n:
            return _host(info, "truncated segment")
        L = (d[i] << 8) | d[i + 1]
        if L < 2 or i + L > n:
            return _host(info, "bad segment length")
        p = d[i + 2:i + L]
        i += L
        if m == 0xE0 and p[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xE1 and p[:6] == b"Exif\x00\x00":
            if _exif_orientation(p) != 1:
                return _host(info, "EXIF orientation is not 1")
        elif m == 0xEE and p[:5] == b"Adobe" and len(p) >= 12:
            adobe, adobe_transform = True, p[11]
        elif 0xE0 <= m <= 0xEF or m == 0xFE:
            pass
        elif m == 0xDB:
            k = 0
            while k < len(p):
                pq, tq = p[k] >> 4, p[k] & 15
                if pq > 1 or tq > 3:
                    return _host(info, "bad DQT")
                if pq == 0:
                    v = list(p[k + 1:k + 65])
                    k += 65
                else:
                    v = [(p[k + 1 + 2 * j] << 8) | p[k + 2 + 2 * j] for j in range(64)]
                    k += 129
                if len(v) != 64 or k > len(p):
                    return _host(info, "truncated DQT")
                q = [0] * 64
                for j in range(64):
                    q[ZIGZAG[j]] = v[j]
                if min(q) == 0:
                    return _host(info, "zero quantiser")
                info.qt[tq] = q
        elif m == 0xC4:
            k = 0
            while k < len(p):
                tc, th = p[k] >> 4, p[k] & 15
                if tc > 1 or th > 3:
                    return _host(info, "bad DHT")
                bits = list(p[k + 1:k + 17])
                nv = sum(bits)
                vals = list(p[k + 17:k + 17 + nv])
                k += 17 + nv
                if len(bits) != 16 or len(vals) != nv or not _check_huffman(bits, vals):
                    return _host(info, "bad Huffman table")
                info.huff[(tc, th)] = (bits, vals)
        elif m == 0xDD:
            info.restart = (p[0] << 8) | p[1]
        elif m in (0xC0, 0xC1):
            if sof is not None:
                return _host(info, "second SOF")
            sof = m
            if p[0] != 8:
                return _host(info, "%d-bit samples" % p[0])
            info.H, info.W, nc = (p[1] << 8) | p[2], (p[3] << 8) | p[4], p[5]
            if info.H == 0 or info.W == 0:
                return _host(info, "zero height (DNL) or width")
            comps = [tuple(p[6 + 3 * c:9 + 3 * c]) for c in range(nc)]
            if len(p) < 6 + 3 * nc or nc not in (1, 3):
                return _host(info, "%d components" % nc)
            info.ncomp = nc
            info.comp_ids = [c[0] for c in comps]
            samp = [(c[1] >> 4, c[1] & 15) for c in comps]
            info.comp_q = [c[2] for c in comps]
            if any(q > 3 for q in info.comp_q):
                return _host(info, "bad quant table id")
            if nc == 1:
                if samp[0] != (1, 1):
                    return _host(info, "grayscale sampling %r" % (samp[0],))
                info.sampling = SAMPLING_GRAY
            else:
                if samp[1] != (1, 1) or samp[2] != (1, 1) or samp[0] not in ((1, 1), (2, 1), (2, 2)):
                    return _host(info, "sampling %r" % (samp,))
                info.sampling = (samp[0][0] << 4) | samp[0][1]
        elif 0xC0 <= m <= 0xCF:
            return _host(info, "SOF%d / DAC (progressive, lossless, arithmetic or hierarchical)" % (m - 0xC0))
        elif m == 0xDA:
            if sof is None:
                return _host(info, "SOS before SOF")
            ns = p[0]
            if ns != info.ncomp:
                return _host(info, "scan of %d of %d components" % (ns, info.ncomp))
            sel = [(p[1 + 2 * c], p[2 + 2 * c]) for c in range(ns)]
            if [s[0] for s in sel] != info.comp_ids:
                return _host(info, "scan component order")
            ss, se, a = p[1 + 2 * ns], p[2 + 2 * ns], p[3 + 2 * ns]
            if (ss, se, a) != (0, 63, 0):
                return _host(info, "spectral selection %d..%d / approximation %d" % (ss, se, a))
            info.comp_dc = [s[1] >> 4 for s in sel]
            info.comp_ac = [s[1] & 15 for s in sel]
            for c in range(ns):
                if info.comp_dc[c] > 3 or info.comp_ac[c] > 3 or (0, info.comp_dc[c]) not in info.huff or (1, info.comp_ac[c]) not in info.huff:
                    return _host(info, "undefined Huffman table")
                if info.qt[info.comp_q[c]] is None:
                    return _host(info, "undefined quant table")
            if info.ncomp == 3:
                if not jfif and adobe and adobe_transform == 0:
                    return _host(info, "Adobe transform 0 (RGB)")
                if not jfif and not adobe and info.comp_ids == [82, 71, 66]:
                    return _host(info, "component ids R G B")
            if n - i < 2 or d[-2:] != b"\xff\xd9":
                return _host(info, "no EOI at the end of the file")
            info.ecs_begin, info.ecs_end = i, n - 2
            info.device = True
            return info
        else:
            return _host(info, "marker 0x%02X" % m)


def huffman_lookup(bits, vals):
    """(look[256] uint16, maxcode[18] int32, valoff[18] int32, vals[256] uint8) of one DHT table (libjpeg jdhuff's derived table)."""
    look = np.zeros(256, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    v = np.zeros(256, np.uint8)
    v[:len(vals)] = vals
    code, k = 0, 0
    for l in range(1, 17):
        nl = bits[l - 1]
        if nl:
            valoff[l] = k - code
            for j in range(nl):
                if l <= 8:
                    lo = (code + j) << (8 - l)
                    look[lo:lo + (1 << (8 - l))] = (l << 8) | vals[k + j]
            code += nl
            k += nl
            maxcode[l] = code - 1
        code <<= 1
    maxcode[17] = 0x7FFFFFFF
    return look, maxcode, valoff, v


def table_blob(info):
    """The BLOB_BYTES-byte table blob of a device-classified file (layout: module docstring)."""
    assert info.device
    b = np.zeros(BLOB_BYTES, np.uint8)
    hdr = np.zeros(16, np.int32)
    hdr[0], hdr[1] = info.restart, info.ncomp
    for c in range(info.ncomp):
        hdr[2 + c], hdr[5 + c], hdr[8 + c] = info.comp_dc[c], info.comp_ac[c], info.comp_q[c]
    b[:HDR_BYTES] = hdr.view(np.uint8)
    q = np.zeros((4, 64), np.uint16)
    for t in range(4):
        if info.qt[t] is not None:
            q[t] = info.qt[t]
    b[HDR_BYTES:HDR_BYTES + QUANT_BYTES] = q.reshape(-1).view(np.uint8)
    for tc in range(2):
        for th in range(4):
            if (tc, th) not in info.huff:
                continue
            look, maxcode, valoff, vals = huffman_lookup(*info.huff[(tc, th)])
            o = HDR_BYTES + QUANT_BYTES + (4 * tc + th) * HUFF_BYTES
            b[o:o + 512] = look.view(np.uint8)
            b[o + 512:o + 584] = maxcode.view(np.uint8)
            b[o + 584:o + 656] = valoff.view(np.uint8)
            b[o + 656:o + 912] = vals
    return b


def mcu_count(info):
    if info.sampling == SAMPLING_GRAY:
        return -(-info.H // 8) * -(-info.W // 8)
    h, v = info.sampling >> 4, info.sampling & 15
    return -(-info.H // (8 * v)) * -(-info.W // (8 * h))


def read_file(path):
    with open(path, "rb") as fh:
        return fh.read()
