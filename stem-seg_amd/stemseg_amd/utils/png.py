"""Host half of the device PNG decoder (``hip.png_decode``, csrc/png_decode.hip): the chunk walker, the device / host
classification and the per-call header blob.

Only the chunks are walked here; the zlib stream is never inflated on the host, and the IDAT CRCs are checked on the device.  A
file goes to the device when it has a valid signature, an IHDR with bit depth 8, colour type 0 / 2 / 4 / 6 (gray, RGB, gray+alpha,
RGBA) and no interlace, at least one IDAT with all of them consecutive, a final IEND with nothing after it, no tRNS, no eXIf (cv2
would rotate the image, PIL would not), no APNG chunk, no unknown critical chunk, and a correct CRC on every chunk but the IDATs.
Everything else -- palette, 16-bit, sub-8-bit, interlaced, animated, anything unparsable -- goes to the host loader, which then
decides as it always did.

The header blob of one call (little-endian, the layout csrc/png_decode.hip reads):
    int64 hdr[F][8]     H, W, channels, zlib stream length, first IDAT record, IDAT count, 0, 0
    uint32 idat[N][4]   per IDAT chunk, in frame order: offset of its payload in the frame's zlib stream, payload length, the
                        stored CRC (over the chunk type and the payload), frame index
The zlib stream of a frame is its IDAT payloads concatenated.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
HDR_WORDS = 8
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}
MAX_DIM = 65535
KNOWN_CRITICAL = (b"IHDR", b"PLTE", b"IDAT", b"IEND")


class PngInfo(object):
    """What the parser learnt about one file.  ``device`` says whether the device decoder takes it; ``reason`` says why not."""

    def __init__(self):
        self.device = False
        self.reason = ""
        self.H = self.W = 0
        self.color_type = -1
        self.channels = 0
        self.idat = []                        # (payload offset in the file, payload length, stored CRC)

    @property
    def geometry(self):
        return (self.H, self.W, self.channels)

    @property
    def stream_len(self):
        return sum(n for _, n, _ in self.idat)

    def __repr__(self):
        return "PngInfo(%s, %dx%d, channels=%d, %d IDAT%s)" % ("device" if self.device else "host", self.W, self.H, self.channels,
                                                              len(self.idat), "" if self.device else ", " + self.reason)


def is_png(data):
    return bytes(data[:8]) == SIGNATURE


def parse(data):
    """PngInfo of one file's bytes.  Never raises: anything the walker cannot follow is classified for the host."""
    info = PngInfo()
    try:
        reason = _parse(bytes(data), info)
    except Exception as e:  # noqa: BLE001 -- a malformed file is the host loader's business, never ours
        reason = "unparsable: %s" % e
    info.device = reason is None
    info.reason = reason or ""
    return info


def _parse(d, info):
    if d[:8] != SIGNATURE:
        return "no PNG signature"
    pos, n = 8, len(d)
    first = True
    idat_state = 0                            # 0 before any IDAT, 1 inside the IDAT run, 2 after it
    while True:
        if pos + 12 > n:
            return "truncated chunk header"
        length, ctype = struct.unpack(">I4s", d[pos:pos + 8])
        if length > 0x7FFFFFFF or pos + 12 + length > n:
            return "chunk %r overruns the file" % ctype
        payload = d[pos + 8:pos + 8 + length]
        crc = struct.unpack(">I", d[pos + 8 + length:pos + 12 + length])[0]
        if ctype != b"IDAT" and zlib.crc32(ctype + payload) != crc:
            return "bad CRC in %r" % ctype
        if first and ctype != b"IHDR":
            return "IHDR is not the first chunk"
        if ctype == b"IHDR":
            if not first or length != 13:
                return "bad IHDR"
            W, H, depth, ct, comp, filt, interlace = struct.unpack(">IIBBBBB", payload)
            if depth != 8 or ct not in CHANNELS:
                return "bit depth %d, colour type %d" % (depth, ct)
            if comp != 0 or filt != 0 or interlace != 0:
                return "compression %d, filter %d, interlace %d" % (comp, filt, interlace)
            if not (1 <= W <= MAX_DIM and 1 <= H <= MAX_DIM):
                return "size %dx%d" % (W, H)
            info.W, info.H, info.color_type, info.channels = W, H, ct, CHANNELS[ct]
        elif ctype == b"IDAT":
            if idat_state == 2:
                return "IDAT chunks are not consecutive"
            idat_state = 1
            info.idat.append((pos + 8, length, crc))
        else:
            if idat_state == 1:
                idat_state = 2
            if ctype == b"IEND":
                if length != 0 or pos + 12 != n:
                    return "data after IEND"
                break
            if ctype in (b"tRNS", b"eXIf", b"acTL", b"fcTL", b"fdAT"):
                return "%r chunk" % ctype
            if ctype == b"PLTE" and (info.color_type in (0, 4) or idat_state):
                return "PLTE in a gray image or after IDAT"
            if not (ctype[0] & 0x20) and ctype not in KNOWN_CRITICAL:
                return "unknown critical chunk %r" % ctype
        first = False
        pos += 12 + length
    if not info.idat:
        return "no IDAT"
    if len(info.idat) > max(1, info.stream_len):
        return "more IDAT chunks than stream bytes"
    return None


def stream(info, data):
    """The frame's zlib stream: its IDAT payloads back to back."""
    d = bytes(data)
    return b"".join(d[o:o + n] for o, n, _ in info.idat)


def header_blob(infos):
    """(int64 hdr [F][8], uint32 idat [N][4]) of the device-classified frames ``infos`` (see the module docstring)."""
    F = len(infos)
    hdr = np.zeros((F, HDR_WORDS), np.int64)
    recs = []
    for f, info in enumerate(infos):
        hdr[f, :6] = (info.H, info.W, info.channels, info.stream_len, len(recs), len(info.idat))
        off = 0
        for _, n, crc in info.idat:
            recs.append((off, n, crc, f))
            off += n
    return hdr, np.array(recs, np.uint32).reshape(-1, 4)


def read_file(path):
    with open(path, "rb") as fh:
        return fh.read()
