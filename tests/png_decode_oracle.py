"""A numpy / Python restatement of the device PNG decoder (csrc/png_decode.hip), stage by stage, for the CPU tests: the
dynamic-block finder at every bit position, the speculative block decode, the chain with its serial backstop, the write pass into
literals and source indices (dst - dist + (i mod dist)), pointer jumping, the Adler-32 and filter checks, and the unfilter."""
import struct
import zlib

import numpy as np

from stemseg_amd.utils import png as P

ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bad(Exception):
    pass


class Bits(object):
    def __init__(self, s):
        self.s, self.n = s, len(s)
        self.end = 8 * len(s)

    def get(self, pos, k):
        v = 0
        for i in range(k):
            b = pos + i
            if (b >> 3) < self.n:
                v |= ((self.s[b >> 3] >> (b & 7)) & 1) << i
        return v, pos + k


def build(lengths):
    """(count, symbols, Kraft remainder, longest length) of a canonical code."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    left, mx = 1, 0
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if count[l]:
            mx = l
        if left < 0:
            return None, None, left, mx
    syms = [i for l in range(1, 16) for i, x in enumerate(lengths) if x == l]
    return count, syms, left, mx


def decode(bs, pos, code_tab):
    count, syms = code_tab
    code = first = index = 0
    for l in range(1, 16):
        b, pos = bs.get(pos, 1)
        code |= b
        c = count[l]
        if code - c < first:
            return syms[index + code - first], pos
        index += c
        first = (first + c) << 1
        code <<= 1
    raise Bad("no code")


def code_ok(left, mx):
    return left == 0 or (left > 0 and mx == 1)


def dynamic_header(bs, pos):
    """(literal/length code, distance code, body start) of the dynamic header after BTYPE, or Bad if zlib would reject it."""
    v, pos = bs.get(pos, 5)
    nlen = v + 257
    v, pos = bs.get(pos, 5)
    ndist = v + 1
    v, pos = bs.get(pos, 4)
    ncode = v + 4
    if nlen > 286 or ndist > 30:
        raise Bad("HLIT / HDIST")
    cl = [0] * 19
    for i in range(ncode):
        cl[ORDER[i]], pos = bs.get(pos, 3)
    if pos > bs.end:
        raise Bad("overrun")
    count, syms, left, _ = build(cl)
    if left != 0:
        raise Bad("code-length code")
    lens = []
    while len(lens) < nlen + ndist:
        s, pos = decode(bs, pos, (count, syms))
        if pos > bs.end:
            raise Bad("overrun")
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Bad("leading repeat")
            val = lens[-1]
            r, pos = bs.get(pos, 2)
            rep = 3 + r
        elif s == 17:
            val = 0
            r, pos = bs.get(pos, 3)
            rep = 3 + r
        else:
            val = 0
            r, pos = bs.get(pos, 7)
            rep = 11 + r
        if len(lens) + rep > nlen + ndist or pos > bs.end:
            raise Bad("repeat overrun")
        lens += [val] * rep
    if lens[256] == 0:
        raise Bad("no EOB")
    lc, ls, ll, lm = build(lens[:nlen])
    if not code_ok(ll, lm):
        raise Bad("literal/length code")
    dc, ds, dl, dm = build(lens[nlen:])
    if not (dm == 0 or code_ok(dl, dm)):
        raise Bad("distance code")
    return (lc, ls), (dc, ds), pos


def fixed_codes():
    lc, ls, _, _ = build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
    dc, ds, _, _ = build([5] * 32)
    return (lc, ls), (dc, ds)


def finder(stream):
    """Every bit position (after the zlib header) holding a dynamic block header that zlib would accept."""
    bs = Bits(stream)
    out = []
    for pos in range(16, 8 * len(stream)):
        if bs.get(pos + 1, 2)[0] != 2:
            continue
        try:
            dynamic_header(bs, pos + 3)
            out.append(pos)
        except Bad:
            pass
    return out


def block(bs, pos, o0, cap, window, src):
    """One block from its header: (end bit, output bytes, BFINAL); appends literals (-1 - byte) and source indices to src when it
    is a list.  Bad if zlib would reject it."""
    final, pos = bs.get(pos, 1)
    typ, pos = bs.get(pos, 2)
    o = o0
    if typ == 0:
        pos = (pos + 7) & ~7
        ln, pos = bs.get(pos, 16)
        nl, pos = bs.get(pos, 16)
        if ln ^ 0xFFFF != nl or pos + 8 * ln > bs.end or o0 + ln > cap:
            raise Bad("stored length")
        if src is not None:
            src += [-1 - b for b in bs.s[pos >> 3:(pos >> 3) + ln]]
        return pos + 8 * ln, ln, final
    if typ == 3:
        raise Bad("BTYPE 11")
    if typ == 1:
        lit, dist = fixed_codes()
    else:
        lit, dist, pos = dynamic_header(bs, pos)
    while True:
        s, pos = decode(bs, pos, lit)
        if pos > bs.end:
            raise Bad("overrun")
        if s < 256:
            if o >= cap:
                raise Bad("too much output")
            if src is not None:
                src.append(-1 - s)
            o += 1
            continue
        if s == 256:
            return pos, o - o0, final
        if s > 285:
            raise Bad("length symbol")
        e, pos = bs.get(pos, LEN_EXTRA[s - 257])
        n = LEN_BASE[s - 257] + e
        ds, pos = decode(bs, pos, dist)
        if ds > 29:
            raise Bad("distance symbol")
        e, pos = bs.get(pos, DIST_EXTRA[ds])
        d = DIST_BASE[ds] + e
        if pos > bs.end or o + n > cap or d > window:
            raise Bad("distance / overrun")
        if src is not None:
            if o - d < 0:
                raise Bad("distance before the start")
            src += [o - d + (i % d) for i in range(n)]
        o += n


def inflate(stream, raw_len, use_finder=True):
    """(bytes, stats) of a frame's zlib stream as the device inflates it, or (None, reason)."""
    bs = Bits(stream)
    if len(stream) < 6:
        return None, "short"
    cmf, flg = stream[0], stream[1]
    if (cmf & 15) != 8 or (cmf >> 4) > 7 or ((cmf << 8) | flg) % 31 or flg & 0x20:
        return None, "zlib header"
    window = 1 << ((cmf >> 4) + 8)
    spec = {}
    if use_finder:
        for c in finder(stream):
            try:
                end, olen, _ = block(bs, c, 0, raw_len, window, None)
                spec[c] = (end, olen)
            except Bad:
                pass
    pos, out, fin, blocks, backstop, missed = 16, 0, 0, [], 0, 0
    try:
        while not fin:
            blocks.append((pos, out))
            if bs.get(pos + 1, 2)[0] == 2 and pos in spec:
                end, olen = spec[pos]
                fin = bs.get(pos, 1)[0]
            else:
                backstop += 1
                missed += bs.get(pos + 1, 2)[0] == 2                     # a dynamic block the finder did not give
                end, olen, fin = block(bs, pos, out, raw_len, window, None)
            pos, out = end, out + olen
            if out > raw_len:
                return None, "too much output"
        pos = (pos + 7) & ~7
        if pos // 8 + 4 != len(stream) or out != raw_len:
            return None, "length or trailing bytes"
        src = []
        for start, o0 in blocks:                                    # the write pass
            block(bs, start, o0, raw_len, window, src)
    except Bad as e:
        return None, str(e)
    src = np.array(src, np.int64)
    rounds = 0
    while (src >= 0).any():                                         # pointer jumping
        m = src >= 0
        src[m] = src[src[m]]
        rounds += 1
    data = (-1 - src).astype(np.uint8).tobytes()
    if zlib.adler32(data) != struct.unpack(">I", stream[-4:])[0]:
        return None, "Adler-32"
    return data, {"blocks": len(blocks), "backstop": backstop, "missed_dynamic": missed, "candidates": len(spec),
                  "jump_rounds": rounds}


def unfilter(data, H, W, C):
    """uint8 [H, W, C] of the inflated scanlines, or None on a filter type > 4."""
    S = 1 + W * C
    rows = np.frombuffer(data, np.uint8).reshape(H, S)
    if (rows[:, 0] > 4).any():
        return None
    out = np.zeros((H, W * C), np.int32)
    for r in range(H):
        f, x = rows[r, 0], rows[r, 1:].astype(np.int32)
        up = out[r - 1] if r else np.zeros(W * C, np.int32)
        if f in (0, 2):
            out[r] = (x + (up if f == 2 else 0)) & 255
            continue
        cur = out[r]
        for j in range(W * C):
            a = cur[j - C] if j >= C else 0
            b = up[j]
            c = up[j - C] if j >= C else 0
            if f == 1:
                pred = a
            elif f == 3:
                pred = (a + b) >> 1
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else b if pb <= pc else c
            cur[j] = (x[j] + pred) & 255
    return out.reshape(H, W, C).astype(np.uint8)


def decode_png(data, use_finder=True):
    """(BGR uint8 [H, W, 3] or None, stats or reason) as the device decodes a device-classified file; None = flagged corrupt."""
    info = P.parse(data)
    assert info.device, info
    s = P.stream(info, data)
    for off, n, crc in info.idat:
        if zlib.crc32(b"IDAT" + bytes(data[off:off + n])) != crc:
            return None, "IDAT CRC"
    raw, st = inflate(s, info.H * (1 + info.W * info.channels), use_finder)
    if raw is None:
        return None, st
    px = unfilter(raw, info.H, info.W, info.channels)
    if px is None:
        return None, "filter type"
    bgr = np.repeat(px[..., :1], 3, -1) if info.channels <= 2 else px[..., 2::-1]
    return np.ascontiguousarray(bgr), st
