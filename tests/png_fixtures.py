"""PNG files for the decoder tests, written at test time: a small writer with explicit per-row filters, zlib settings and IDAT
splits (chunk CRCs by zlib.crc32), PIL-written files, files outside the device subset, and corrupt files."""
import io
import struct
import zlib

import numpy as np

from tests.jpeg_fixtures import content

SIGNATURE = b"\x89PNG\r\n\x1a\n"
SMALL_SIZES = [(1, 1), (1, 7), (7, 1), (17, 33), (40, 57)]
SIZES = SMALL_SIZES + [(375, 1242)]


def chunk(ctype, payload):
    return struct.pack(">I", len(payload)) + ctype + payload + struct.pack(">I", zlib.crc32(ctype + payload))


def pixels(H, W, color_type, seed, noise=False):
    """uint8 [H, W, channels]: the JPEG fixtures' textured (or noisy) content, with gray and alpha planes derived from it."""
    rgb = content(H, W, seed, noise)
    gray = ((rgb[..., 0].astype(np.int32) * 3 + rgb[..., 1] * 5 + rgb[..., 2]) // 9).astype(np.uint8)
    alpha = rgb[..., 2][..., None] ^ 0x5A
    return {0: gray[..., None], 2: rgb, 4: np.concatenate([gray[..., None], alpha], -1), 6: np.concatenate([rgb, alpha], -1)}[color_type]


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(px, filters):
    """The filtered scanlines (filter byte + bytes per row) of px [H, W, C] with filter type filters[r] on row r."""
    H, W, C = px.shape
    rows = px.reshape(H, W * C).astype(np.int32)
    out = []
    for r in range(H):
        x = rows[r]
        b = rows[r - 1] if r else np.zeros_like(x)
        a = np.concatenate([np.zeros(C, np.int32), x[:-C]])
        c = np.concatenate([np.zeros(C, np.int32), b[:-C]])
        f = int(filters[r])
        pred = [0, a, b, (a + b) >> 1, _paeth(a, b, c)][f] if f <= 4 else 0
        out.append(bytes([f]) + ((x - pred) & 255).astype(np.uint8).tobytes())
    return b"".join(out)


def compress(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, wbits=15, flush_at=(), flush_mode=zlib.Z_SYNC_FLUSH):
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem_level, strategy)
    parts, last = [], 0
    for cut in sorted(flush_at):
        parts.append(co.compress(raw[last:cut]) + co.flush(flush_mode))
        last = cut
    parts.append(co.compress(raw[last:]) + co.flush())
    return b"".join(parts)


def assemble(H, W, color_type, stream, idat_size=None, extra_before=(), depth=8, interlace=0, trailing=b""):
    ihdr = struct.pack(">IIBBBBB", W, H, depth, color_type, 0, 0, interlace)
    step = idat_size or max(1, len(stream))
    idats = [chunk(b"IDAT", stream[i:i + step]) for i in range(0, max(1, len(stream)), step)]
    return SIGNATURE + chunk(b"IHDR", ihdr) + b"".join(chunk(t, p) for t, p in extra_before) + b"".join(idats) + chunk(b"IEND", b"") + trailing


def write(px, color_type, filters=None, seed=0, idat_size=None, **zkw):
    """A PNG of px [H, W, C]: filters None (per-row random over 0..4), an int (every row), or a list."""
    H = px.shape[0]
    if filters is None:
        filters = np.random.RandomState(seed).randint(0, 5, H)
    elif np.isscalar(filters):
        filters = [filters] * H
    return assemble(H, px.shape[1], color_type, compress(filter_rows(px, filters), **zkw), idat_size)


def pil_png(px, **kw):
    from PIL import Image
    im = Image.fromarray(px[..., 0] if px.shape[2] == 1 else px, {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[px.shape[2]])
    buf = io.BytesIO()
    im.save(buf, "PNG", **kw)
    return buf.getvalue()


def pil_bgr(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


def matrix(sizes, seed=0):
    """[(label, bytes)] of device-supported files: every filter type and random mixes, levels 0-9, every strategy, memLevel 1 / 9,
    wbits 9-15, sync and full flushes, 1-byte and single IDATs, colour types 0 / 2 / 4 / 6, PIL at every level and optimize."""
    out = []
    for (H, W) in sizes:
        big = H * W > 100000
        for ct in (0, 2, 4, 6):
            px = pixels(H, W, ct, seed + ct)
            for f in range(5):
                out.append(("%dx%d ct%d filter %d" % (H, W, ct, f), write(px, ct, f)))
            out.append(("%dx%d ct%d mixed" % (H, W, ct), write(px, ct, None, seed)))
            out.append(("%dx%d ct%d pil" % (H, W, ct), pil_png(px)))
        px = pixels(H, W, 2, seed + 7)
        for lv in ([0, 1, 6, 9] if big else range(10)):
            out.append(("%dx%d level %d" % (H, W, lv), write(px, 2, None, seed, level=lv)))
            out.append(("%dx%d pil level %d" % (H, W, lv), pil_png(px, compress_level=lv)))
        out.append(("%dx%d pil optimize" % (H, W), pil_png(px, optimize=True)))
        for name, st in (("filtered", zlib.Z_FILTERED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE), ("fixed", zlib.Z_FIXED)):
            out.append(("%dx%d %s" % (H, W, name), write(px, 2, None, seed, strategy=st)))
        for ml in (1, 9):
            out.append(("%dx%d memLevel %d" % (H, W, ml), write(px, 2, None, seed, mem_level=ml)))
        for wb in ([9, 12, 15] if big else range(9, 16)):
            out.append(("%dx%d wbits %d" % (H, W, wb), write(px, 2, None, seed, wbits=wb)))
        n = H * (1 + W * 3)
        cuts = [n // 3, n // 2] if n > 2 else []
        out.append(("%dx%d sync flush" % (H, W), write(px, 2, None, seed, flush_at=cuts)))
        out.append(("%dx%d full flush" % (H, W), write(px, 2, None, seed, flush_at=cuts, flush_mode=zlib.Z_FULL_FLUSH)))
        if not big:
            out.append(("%dx%d 1-byte IDATs" % (H, W), write(px, 2, None, seed, idat_size=1)))
        out.append(("%dx%d 97-byte IDATs" % (H, W), write(px, 2, None, seed, idat_size=97)))
        out.append(("%dx%d noise" % (H, W), write(pixels(H, W, 2, seed, noise=True), 2, None, seed)))
    return out


# ------------------------------------------------------------------------------------------------ files outside the device subset
def host_files():
    """[(label, bytes)] the chunk walker sends to the host loader (all decodable by PIL)."""
    from PIL import Image
    px = pixels(9, 13, 2, 3)
    out = []
    buf = io.BytesIO()
    Image.fromarray(px).convert("P").save(buf, "PNG")
    out.append(("palette", buf.getvalue()))
    buf = io.BytesIO()
    Image.fromarray((px[..., 0].astype(np.uint16) * 257)).save(buf, "PNG")
    out.append(("16-bit", buf.getvalue()))
    out.append(("tRNS", assemble(9, 13, 2, compress(filter_rows(px, [0] * 9)), extra_before=[(b"tRNS", b"\x00\x01\x00\x02\x00\x03")])))
    good = write(px, 2, 0)
    out.append(("trailing data", good + b"junk"))
    bad_crc = bytearray(good)
    bad_crc[8 + 8 + 13] ^= 1                                                # IHDR CRC
    out.append(("bad IHDR CRC", bytes(bad_crc)))
    out.append(("interlaced", assemble(9, 13, 2, compress(filter_rows(px, [0] * 9)), interlace=1)))
    out.append(("split IDAT run", _split_idat_run(px)))
    return out


def _split_idat_run(px):
    s = compress(filter_rows(px, [0] * px.shape[0]))
    ihdr = struct.pack(">IIBBBBB", px.shape[1], px.shape[0], 8, 2, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", s[:5]) + chunk(b"tEXt", b"a\x00b") + chunk(b"IDAT", s[5:]) + chunk(b"IEND", b"")


# ------------------------------------------------------------------------------------------------ corrupt files
def corrupt_files(H=23, W=31):
    """[(label, bytes)] the chunk walker gives the device but that the device must flag as corrupt."""
    px = pixels(H, W, 2, 5)
    filt = np.random.RandomState(1).randint(0, 5, H)
    raw = filter_rows(px, filt)
    s = compress(raw)
    out = []
    good = assemble(H, W, 2, s)
    i = good.index(b"IDAT")
    bad_crc = bytearray(good)
    bad_crc[i + 4 + len(s)] ^= 0x40                                         # the IDAT CRC
    out.append(("bad IDAT CRC", bytes(bad_crc)))
    out.append(("bad Adler", assemble(H, W, 2, s[:-1] + bytes([s[-1] ^ 1]))))
    out.append(("truncated stream", assemble(H, W, 2, s[:len(s) // 2])))
    out.append(("no Adler", assemble(H, W, 2, s[:-4])))
    flip = bytearray(s)
    flip[len(s) // 2] ^= 0x10
    out.append(("flipped bit", assemble(H, W, 2, bytes(flip))))
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, zdict=raw[:200])
    body = co.compress(raw) + co.flush()                                    # matches into a dictionary the decoder never sees
    out.append(("distance too far back", assemble(H, W, 2, b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(raw)))))
    raw5 = bytearray(raw)
    raw5[(1 + W * 3) * (H // 2)] = 5
    out.append(("filter 5", assemble(H, W, 2, zlib.compress(bytes(raw5)))))
    out.append(("too much data", assemble(H, W, 2, zlib.compress(raw + b"\x00" * 7))))
    out.append(("too little data", assemble(H, W, 2, zlib.compress(raw[:-1]))))
    out.append(("BTYPE 11", assemble(H, W, 2, b"\x78\x9c\x07" + s[3:])))
    return out
