"""Upright output, restated in numpy (include/jpeg2png_amd.h, "Upright output"): the eight maps, the replication beyond the
upright image, the Orientation tag's reader, and builders for the APP1 segments the reader tests feed it.  No tolerance
anywhere: the library permutes, and so does this."""
import struct

import numpy as np

ORIENTATIONS = (1, 2, 3, 4, 5, 6, 7, 8)
# every pair of axis reversals, with and without transposition: what the heavier forms are run with
HEAVY = (1, 3, 6, 7)
TAG = 0x0112


def upright_size(o, w, h):
    """(w', h') of the upright image of a w x h source"""
    return (h, w) if o >= 5 else (w, h)


def source_index(o, w, h, x, y):
    """(sx, sy): U[y][x] = I[sy][sx]; x, y may be arrays"""
    return {1: (x, y), 2: (w - 1 - x, y), 3: (w - 1 - x, h - 1 - y), 4: (x, h - 1 - y),
            5: (y, x), 6: (y, h - 1 - x), 7: (w - 1 - y, h - 1 - x), 8: (w - 1 - y, x)}[o]


def upright(image, o, w=None, h=None, canvas=None):
    """U of the top-left w x h of `image` ([rows, columns] or [rows, columns, channels]) under orientation o.  canvas=(W, H): U on
    that many columns and rows, replicated beyond the upright image — U[y][x] = U[min(y, h' - 1)][min(x, w' - 1)]; default: the
    upright image itself."""
    image = np.asarray(image)
    h = image.shape[0] if h is None else h
    w = image.shape[1] if w is None else w
    uw, uh = upright_size(o, w, h)
    W, H = (uw, uh) if canvas is None else canvas
    x, y = np.meshgrid(np.minimum(np.arange(W), uw - 1), np.minimum(np.arange(H), uh - 1))
    sx, sy = source_index(o, w, h, x, y)
    return np.ascontiguousarray(image[sy, sx])


def upright_canvas(o, w, h):
    """(W, H) against which an oriented call's extents are checked: w' and h' rounded up to multiples of 16"""
    uw, uh = upright_size(o, w, h)
    return -(-uw // 16) * 16, -(-uh // 16) * 16


def upright_planes(planes, o, w, h):
    """what an output form of an oriented solver reads: every downloaded plane permuted onto the upright canvas"""
    return [upright(p, o, w, h, canvas=upright_canvas(o, w, h)) for p in planes]


# ---- the tag ----

def tiff_orientation(t):
    """the tag of one TIFF structure (the bytes behind b"Exif\\0\\0"), 1 where it has none that counts"""
    if len(t) < 8 or t[:2] not in (b"II", b"MM"):
        return 1
    e = "<" if t[:2] == b"II" else ">"
    if struct.unpack_from(e + "H", t, 2)[0] != 42:
        return 1
    ifd = struct.unpack_from(e + "I", t, 4)[0]
    if ifd + 2 > len(t):
        return 1
    n = struct.unpack_from(e + "H", t, ifd)[0]
    if ifd + 2 + 12 * n > len(t):
        return 1
    for k in range(n):
        tag, kind, count = struct.unpack_from(e + "HHI", t, ifd + 2 + 12 * k)
        if tag != TAG:
            continue
        if kind != 3 or count != 1:
            return 1
        v = struct.unpack_from(e + "H", t, ifd + 2 + 12 * k + 8)[0]
        return v if 1 <= v <= 8 else 1
    return 1


def orientation(file):
    """the Orientation of a JPEG file: IFD0 of the first APP1 segment that begins b"Exif\\0\\0", segments up to SOS"""
    f = bytes(file)
    if f[:2] != b"\xff\xd8":
        return 1
    pos = 2
    while pos + 4 <= len(f) and f[pos] == 0xff:
        marker = f[pos + 1]
        if marker == 0xff:
            pos += 1
            continue
        if marker == 0x01 or 0xd0 <= marker <= 0xd8:
            pos += 2
            continue
        if marker in (0xd9, 0xda):
            return 1
        n = struct.unpack_from(">H", f, pos + 2)[0]
        if n < 2 or pos + 2 + n > len(f):
            return 1
        body = f[pos + 4:pos + 2 + n]
        if marker == 0xe1 and body[:6] == b"Exif\0\0":
            return tiff_orientation(body[6:])
        pos += 2 + n
    return 1


# ---- builders ----

def tiff(order, entries, ifd_offset=8, count=None, pad=b""):
    """a TIFF structure in byte order "II" or "MM": the header, `pad` up to ifd_offset, IFD0 with `entries` — (tag, type, count,
    value) with the value left-justified in its field as a SHORT (type 3) or a LONG — and a zero next-IFD offset.  count: the entry
    count WRITTEN (default: the true one)."""
    e = "<" if order == "II" else ">"
    out = order.encode() + struct.pack(e + "HI", 42, ifd_offset) + pad
    out += struct.pack(e + "H", len(entries) if count is None else count)
    for tag, kind, n, value in entries:
        field = struct.pack(e + "HH", value, 0) if kind == 3 else struct.pack(e + "I", value)
        out += struct.pack(e + "HHI", tag, kind, n) + field
    return out + struct.pack(e + "I", 0)


def segment(marker, payload):
    return bytes([0xff, marker]) + struct.pack(">H", len(payload) + 2) + payload


def exif_segment(tiff_bytes):
    return segment(0xe1, b"Exif\0\0" + tiff_bytes)


def orientation_tiff(order, value, kind=3, n=1, **kw):
    """a TIFF structure with two harmless entries around the Orientation entry"""
    return tiff(order, [(0x010f, 3, 1, 7), (TAG, kind, n, value), (0x0128, 3, 1, 2)], **kw)


def insert_segments(jpeg, segments):
    """`segments` (bytes) put right behind the SOI marker of a JPEG file"""
    assert jpeg[:2] == b"\xff\xd8"
    return jpeg[:2] + segments + jpeg[2:]


def strip_app_segments(jpeg):
    """the file without its APPn and COM segments (what PIL wrote in front of the tables)"""
    out, pos = bytearray(jpeg[:2]), 2
    while jpeg[pos + 1] != 0xda:
        n = struct.unpack_from(">H", jpeg, pos + 2)[0]
        if not (0xe0 <= jpeg[pos + 1] <= 0xef or jpeg[pos + 1] == 0xfe):
            out += jpeg[pos:pos + 2 + n]
        pos += 2 + n
    return bytes(out) + jpeg[pos:]


def pil_jpeg(width, height, seed=1, orientation=None, subsampling="4:2:0", quality=85, progressive=False, grey=False):
    """a baseline (or progressive) JPEG file made by PIL from seeded smooth content, with the Orientation tag (MM, PIL's) or none"""
    import io

    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = np.stack([128 + 90 * np.sin(xx / 5.0 + k) * np.cos(yy / 7.0 - k) for k in range(3)], axis=2)
    pixels = np.clip(base + rng.normal(0, 6, base.shape), 0, 255).astype(np.uint8)
    im = Image.fromarray(pixels[:, :, 0] if grey else pixels)
    kw = {}
    if orientation is not None:
        exif = Image.Exif()
        exif[TAG] = orientation
        kw["exif"] = exif.tobytes()
    if not grey:
        kw["subsampling"] = subsampling
    out = io.BytesIO()
    im.save(out, "JPEG", quality=quality, progressive=progressive, **kw)
    return out.getvalue()
