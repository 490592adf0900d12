"""JPEG files for the decoder tests, written at test time by PIL (libjpeg-turbo): the device-supported matrix and files outside it."""
import io

import numpy as np

SIZES = [(1, 1), (7, 9), (17, 33), (33, 15), (240, 432), (481, 855), (720, 1280), (1080, 1920)]     # (H, W)
SMALL_SIZES = [(1, 1), (7, 9), (17, 33), (33, 15), (64, 80)]
QUALITIES = [1, 10, 50, 75, 90, 95, 100]
SUBSAMPLINGS = ["L", 0, 1, 2]                              # grayscale, 4:4:4, 4:2:2, 4:2:0


def content(H, W, seed, noise=False):
    """RGB uint8 [H, W, 3]: smooth gradients with texture, or uniform noise (long codes, many sync rounds)."""
    rs = np.random.RandomState(seed)
    if noise:
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    a = np.stack([xx * 255 // max(W - 1, 1), yy * 255 // max(H - 1, 1), (xx * 3 + yy * 5 + seed * 17) % 256], -1)
    return np.clip(a + rs.randint(-24, 25, a.shape), 0, 255).astype(np.uint8)


def encode(rgb, sub, quality=90, **kw):
    from PIL import Image
    im = Image.fromarray(rgb)
    buf = io.BytesIO()
    if sub == "L":
        im.convert("L").save(buf, "JPEG", quality=quality, **kw)
    else:
        im.save(buf, "JPEG", quality=quality, subsampling=sub, **kw)
    return buf.getvalue()


def matrix(sizes, qualities=QUALITIES, subs=SUBSAMPLINGS, seed=0):
    """[(label, bytes)] over sizes x qualities x subsamplings (noise content at q100), plus the option variants per size."""
    out = []
    for (H, W) in sizes:
        for q in qualities:
            for sub in subs:
                out.append(("%dx%d q%d %s" % (H, W, q, sub), encode(content(H, W, seed + q, noise=q == 100), sub, q)))
        for sub in subs:
            rgb = content(H, W, seed + 7)
            out.append(("%dx%d optimize %s" % (H, W, sub), encode(rgb, sub, 85, optimize=True)))
            out.append(("%dx%d rst-blocks %s" % (H, W, sub), encode(rgb, sub, 85, restart_marker_blocks=5)))
            out.append(("%dx%d rst-rows %s" % (H, W, sub), encode(rgb, sub, 85, restart_marker_rows=1)))
        qt = [[min(65535, 300 + 37 * i) for i in range(64)], [min(65535, 280 + 41 * i) for i in range(64)]]
        out.append(("%dx%d qtables16" % (H, W), encode(content(H, W, seed + 3), 2, qtables=qt)))
    return out


def pil_bgr(data):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[:, :, ::-1])


def progressive(H=17, W=33):
    return encode(content(H, W, 1), 2, 80, progressive=True)


def cmyk(H=17, W=33):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(content(H, W, 2)).convert("CMYK").save(buf, "JPEG", quality=80)
    return buf.getvalue()


def exif_rotated(H=17, W=33, orientation=6):
    from PIL import Image
    im = Image.fromarray(content(H, W, 3))
    ex = Image.Exif()
    ex[0x0112] = orientation
    buf = io.BytesIO()
    im.save(buf, "JPEG", quality=80, exif=ex.tobytes())
    return buf.getvalue()


def truncated(data, keep=0.5):
    """The file cut inside its entropy-coded segment, with an EOI appended (the parser sends it to the device, which flags it)."""
    from stemseg_amd.utils import jpeg as J
    info = J.parse(data)
    cut = info.ecs_begin + int((info.ecs_end - info.ecs_begin) * keep)
    if data[cut - 1] == 0xFF:
        cut -= 1
    return data[:cut] + b"\xff\xd9"


def bad_code(data):
    """A run of one bits (stuffed 0xFF 0x00 pairs) in the middle of the entropy-coded segment: an invalid Huffman code."""
    from stemseg_amd.utils import jpeg as J
    info = J.parse(data)
    mid = (info.ecs_begin + info.ecs_end) // 2
    while data[mid - 1] == 0xFF:
        mid += 1
    return data[:mid] + b"\xff\x00" * 8 + data[mid:]
