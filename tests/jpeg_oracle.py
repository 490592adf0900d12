"""numpy restatement of the visualisation path: the reference's overlay (``utils/vis.py`` ``overlay_mask_on_image`` applied per
kept instance, ``output_utils/davis.py:140-161``) and a baseline 4:2:0 JPEG encoder that writes the bytes libjpeg-turbo writes
when PIL drives it (``Image.save(buf, "JPEG", quality=q)``; also cv2.imwrite's defaults).  Pure integer arithmetic, so the
restatement is exact: the CPU tests pin it against PIL, and the GPU tests pin ``hip.jpeg_encode`` / ``hip.vis_composite``
against it.

What it restates (libjpeg's jcparam / jccolor / jcsample / jcprepct / jccoefct / jfdctint / jcdctmgr / jchuff / jcmarker):
  quality -> table scaling with the baseline clamp; fixed-point RGB -> YCbCr (16 fraction bits, Cb / Cr with a 0.5 - eps
  fudge); h2v2 downsampling with the alternating 1 / 2 bias; edge replication to whole MCUs (right edge at full resolution,
  bottom edge by row pairs, then by downsampled rows); dummy blocks right of / below the image that carry the neighbouring
  block's quantised DC; the "islow" integer FDCT; the reciprocal quantiser of the 16-bit SIMD build; DC prediction per
  component across Y0 Y1 Y2 Y3 Cb Cr; the standard Huffman tables; 0xFF00 stuffing and 1-bit padding.
"""
import numpy as np

# ------------------------------------------------------------------------------------------------ tables (ITU T.81 Annex K)
STD_LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
              14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
STD_CHROMA_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63]                                                      # zigzag position k -> natural (row-major) index

DC_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
DC_BITS_C = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
AC_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]
AC_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_BITS_C = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]
AC_VALS_C = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]


def quant_tables(quality):
    """(luma, chroma) quantisation tables in natural order: jpeg_quality_scaling, then (basic * scale + 50) // 100 clamped to
    [1, 255] (force_baseline)."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((b * scale + 50) // 100, 1), 255) for b in basic] for basic in (STD_LUMA_Q, STD_CHROMA_Q))


def reciprocal(q):
    """jcdctmgr compute_reciprocal for divisor 8 * q (the islow FDCT output carries a factor 8), 16-bit DCTELEM:
    (reciprocal, correction, shift) with quantised |x| = ((|x| + correction) * reciprocal) >> (16 + shift)."""
    d = 8 * q
    b = d.bit_length() - 1
    r = 16 + b
    fq, fr = (1 << r) // d, (1 << r) % d
    c = d // 2
    if fr == 0:
        fq >>= 1
        r -= 1
    elif fr <= d // 2:
        c += 1
    else:
        fq += 1
    return fq, c, r - 16


def huff_codes(bits, vals):
    """jpeg_make_c_derived_tbl: symbol -> (code, length) of a canonical table."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


DC_CODES = (huff_codes(DC_BITS, DC_VALS), huff_codes(DC_BITS_C, DC_VALS))
AC_CODES = (huff_codes(AC_BITS, AC_VALS), huff_codes(AC_BITS_C, AC_VALS_C))


def header(height, width, quality):
    """SOI, JFIF 1.01 APP0 (density 1:1, unit 0), DQT x2, SOF0 (Y 2x2, Cb / Cr 1x1), DHT x4 (DC0 AC0 DC1 AC1), SOS."""
    def seg(marker, payload):
        return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)
    lq, cq = quant_tables(quality)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += seg(0xDB, [0] + [lq[z] for z in ZIGZAG]) + seg(0xDB, [1] + [cq[z] for z in ZIGZAG])
    out += seg(0xC0, [8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls_id, bits, vals in ((0x00, DC_BITS, DC_VALS), (0x10, AC_BITS, AC_VALS), (0x01, DC_BITS_C, DC_VALS),
                               (0x11, AC_BITS_C, AC_VALS_C)):
        out += seg(0xC4, [cls_id] + bits + vals)
    return out + seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


# ------------------------------------------------------------------------------------------------ sample pipeline
def rgb_to_ycc(rgb):
    """jccolor rgb_ycc_convert: int64 planes Y, Cb, Cr of an [H, W, 3] RGB uint8 image."""
    def fix(x):
        return int(x * 65536 + 0.5)
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    half = 1 << 15
    y = (fix(0.299) * r + fix(0.587) * g + fix(0.114) * b + half) >> 16
    cb = (-fix(0.16874) * r - fix(0.33126) * g + fix(0.5) * b + (128 << 16) + half - 1) >> 16
    cr = (fix(0.5) * r - fix(0.41869) * g - fix(0.08131) * b + (128 << 16) + half - 1) >> 16
    return y, cb, cr


def planes(rgb):
    """Y [16*mh, 16*mw] and Cb, Cr [8*mh, 8*mw] as the FDCT sees them (edge handling of jcprepct / jcsample)."""
    H, W = rgb.shape[:2]
    mh, mw = -(-H // 16), -(-W // 16)
    y, cb, cr = rgb_to_ycc(rgb)
    rows = np.minimum(np.arange(16 * mh), H - 1)
    cols = np.minimum(np.arange(16 * mw), W - 1)
    Y = y[rows][:, cols]
    # chroma: rows go in pairs (an odd last row pairs with itself), downsampled rows past the last pair repeat the last one;
    # columns replicate the right edge at full resolution first
    n_pairs = -(-H // 2)
    pr = np.minimum(np.arange(8 * mh), n_pairs - 1)
    r0, r1 = 2 * pr, np.minimum(2 * pr + 1, H - 1)
    bias = 1 + (np.arange(8 * mw) & 1)
    out = []
    for p in (cb, cr):
        pc = p[:, cols]
        s = pc[r0][:, 0::2] + pc[r0][:, 1::2] + pc[r1][:, 0::2] + pc[r1][:, 1::2]
        out.append((s + bias[None, :]) >> 2)
    return Y, out[0], out[1]


_C = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137, c1961=16069,
          c2053=16819, c2562=20995, c3072=25172)


def _fdct_1d(d, axis, pass1):
    """One pass of jfdctint.c over the given axis of int64 blocks [..., 8, 8]."""
    x = [np.take(d, i, axis=axis) for i in range(8)]
    C = _C
    tmp0, tmp7 = x[0] + x[7], x[0] - x[7]
    tmp1, tmp6 = x[1] + x[6], x[1] - x[6]
    tmp2, tmp5 = x[2] + x[5], x[2] - x[5]
    tmp3, tmp4 = x[3] + x[4], x[3] - x[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = 13 - 2 if pass1 else 13 + 2

    def desc(v, s):
        return (v + (1 << (s - 1))) >> s
    o = [None] * 8
    if pass1:
        o[0], o[4] = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
    else:
        o[0], o[4] = desc(tmp10 + tmp11, 2), desc(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * C["c0541"]
    o[2] = desc(z1 + tmp13 * C["c0765"], n)
    o[6] = desc(z1 - tmp12 * C["c1847"], n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * C["c1175"]
    tmp4, tmp5, tmp6, tmp7 = tmp4 * C["c0298"], tmp5 * C["c2053"], tmp6 * C["c3072"], tmp7 * C["c1501"]
    z1, z2, z3, z4 = -z1 * C["c0899"], -z2 * C["c2562"], -z3 * C["c1961"] + z5, -z4 * C["c0390"] + z5
    o[7] = desc(tmp4 + z1 + z3, n)
    o[5] = desc(tmp5 + z2 + z4, n)
    o[3] = desc(tmp6 + z2 + z3, n)
    o[1] = desc(tmp7 + z1 + z4, n)
    return np.stack(o, axis=axis)


def block_coefficients(plane, qtable):
    """Quantised coefficients [bh, bw, 64] (natural order) of every 8x8 block of a sample plane."""
    h, w = plane.shape
    blk = (plane.astype(np.int64) - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    d = _fdct_1d(_fdct_1d(blk, 3, True), 2, False).reshape(h // 8, w // 8, 64)
    rc = np.array([reciprocal(q) for q in qtable], np.int64)
    a = np.abs(d)
    qa = ((a + rc[:, 1]) * rc[:, 0]) >> (16 + rc[:, 2])
    return np.where(d < 0, -qa, qa)


def mcu_blocks(rgb, quality):
    """Coefficient blocks in coding order [mh * mw * 6, 64] (natural order), dummy blocks included."""
    H, W = rgb.shape[:2]
    mh, mw = -(-H // 16), -(-W // 16)
    hib, wib = -(-H // 8), -(-W // 8)
    lq, cq = quant_tables(quality)
    Y, Cb, Cr = planes(rgb)
    yc = block_coefficients(Y, lq)
    yc[:, wib:] = 0                                                  # right dummies: DC of the left neighbour
    if wib < 2 * mw:
        yc[:, wib, 0] = yc[:, wib - 1, 0]
    if hib < 2 * mh:                                                 # bottom dummy row: DC of the MCU's block Y1
        yc[hib] = 0
        yc[hib, :, 0] = yc[hib - 1, 1::2, 0].repeat(2)
    cbc, crc = block_coefficients(Cb, cq), block_coefficients(Cr, cq)
    y4 = yc.reshape(mh, 2, mw, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mh, mw, 4, 64)
    return np.concatenate([y4, cbc[:, :, None], crc[:, :, None]], axis=2).reshape(-1, 64)


class _Bits(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put(0x7F, 8 - self.n)
        return bytes(self.out)


def entropy_code(blocks):
    """Huffman-code blocks in coding order (6 per MCU), DC predicted per component."""
    bw = _Bits()
    last = [0, 0, 0]
    zz = blocks[:, ZIGZAG].tolist()
    for i, b in enumerate(zz):
        j = i % 6
        comp = 0 if j < 4 else j - 3
        t = 0 if comp == 0 else 1
        diff = b[0] - last[comp]
        last[comp] = b[0]
        nb = abs(diff).bit_length()
        bw.put(*DC_CODES[t][nb])
        if nb:
            bw.put(diff if diff > 0 else diff - 1, nb)
        ac, r = AC_CODES[t], 0
        for k in range(1, 64):
            v = b[k]
            if v == 0:
                r += 1
                continue
            while r > 15:
                bw.put(*ac[0xF0])
                r -= 16
            nb = abs(v).bit_length()
            bw.put(*ac[(r << 4) + nb])
            bw.put(v if v > 0 else v - 1, nb)
            r = 0
        if r:
            bw.put(*ac[0])
    return bw.flush()


def encode(bgr, quality=95):
    """The JFIF file of one BGR uint8 frame [H, W, 3]."""
    rgb = np.ascontiguousarray(bgr[..., ::-1])
    H, W = rgb.shape[:2]
    return header(H, W, quality) + entropy_code(mcu_blocks(rgb, quality)) + b"\xff\xd9"


def pil_encode(bgr, quality=95):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, "JPEG", quality=quality)
    return buf.getvalue()


# ------------------------------------------------------------------------------------------------ overlay
def overlay(bgr, index_map, colors):
    """The reference's overlay of every kept instance n > 0 of a condensed index map, in colour ``colors[n]`` (RGB order applied
    to the BGR image, as the reference does): ``overlay_mask_on_image`` evaluated per instance in numpy."""
    img = bgr.copy()
    for n in sorted(set(np.unique(index_map).tolist()) - {0}):
        m = np.stack([index_map == n] * 3, axis=2)
        masked = np.where(m > 0, list(colors[n]), img)
        img = ((0.6 * masked) + ((1. - 0.6) * img)).astype(np.uint8)
    return img


def overlay_table():
    """T[c, s] = trunc(0.6 * c + (1 - 0.6) * s) in fp64, for every uint8 colour c and pixel s."""
    c = np.arange(256, dtype=np.float64)[:, None]
    s = np.arange(256, dtype=np.float64)[None, :]
    return ((0.6 * c) + ((1. - 0.6) * s)).astype(np.uint8)
