"""LAS and LAST images with GPS times, for the time-range search tests (test_time_cli.py, test_gpu_time.py).

The oracle's synthesiser writes formats 0-3 in LAS 1.2 only; the time search also reads formats 6-10 (time at record + 22),
which need a LAS 1.4 header.  So the images are built here from the record layout of the LAS specification as the reference
reads it (query/src/las.rs:7-40, las.rs:305-330): positions {i32 x, y, z} at +0, the class byte at +15 (formats 1-5) or
+16 (6-10), the f64 GPS time at +20 or +22, the colour at +20 (format 2), +28 (3, 5) or +30 (7, 8).  A LAST image is the
same record transposed by attribute: the attribute at record offset o with size s occupies [otp + N*o, otp + N*(o+s))
(oracle/synth.c, readers/src/last_reader.rs:83-144).

Expected results come from numpy: sel = (t >= start) & (t < end) on float64, a match's record is x * scale + offset
(unfused) with class 0 and colour (0, 0, 0) (las.rs:345-355).
"""
import struct

import numpy as np

# format -> (record length, time offset or None, colour offset or None, class offset)
FORMATS = {
    0: (20, None, None, 15),
    1: (28, 20, None, 15),
    2: (26, None, 20, 15),
    3: (34, 20, 28, 15),
    4: (57, 20, None, 15),   # format 1 + a 29-byte wave packet
    5: (63, 20, 28, 15),     # format 3 + the wave packet
    6: (30, 22, None, 16),
    7: (36, 22, 30, 16),
    8: (38, 22, 30, 16),
    9: (59, 22, None, 16),   # format 6 + the wave packet
    10: (67, 22, 30, 16),    # format 8 + the wave packet
}

SCALE = (0.01, 0.02, 0.05)
OFFSET = (100.0, -200.0, 7.5)


def points(n, seed):
    """Positions (i32), class bytes, colours (u16) and ordinary GPS times of n points."""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.integers(-5000, 5000, n), rng.integers(-5000, 5000, n), rng.integers(-1000, 1000, n)], axis=1).astype(np.int32)
    cls = rng.choice(np.array([1, 2, 6], dtype=np.uint8), n)
    rgb = rng.integers(1, 65536, (n, 3)).astype(np.uint16)
    t = np.sort(rng.uniform(1000.0, 2000.0, n))
    return xyz, cls, rgb, t


def world(xyz, scale=SCALE, offset=OFFSET):
    """x * scale + offset, two roundings (numpy does not fuse)."""
    return np.stack([xyz[:, a].astype(np.float64) * scale[a] + offset[a] for a in range(3)], axis=1)


def records(fmt, xyz, cls, rgb, t):
    """The AoS records of a format, n x record length bytes."""
    rl, toff, coff, kof = FORMATS[fmt]
    n = len(xyz)
    rec = np.zeros((n, rl), dtype=np.uint8)
    rec[:, 0:12] = np.ascontiguousarray(xyz.astype("<i4")).view(np.uint8).reshape(n, 12)
    rec[:, 12:14] = 0x34  # intensity: any bytes that are not the attributes under test
    rec[:, kof] = cls
    if toff is not None:
        rec[:, toff:toff + 8] = np.ascontiguousarray(t.astype("<f8")).view(np.uint8).reshape(n, 8)
    if coff is not None:
        rec[:, coff:coff + 6] = np.ascontiguousarray(rgb.astype("<u2")).view(np.uint8).reshape(n, 6)
    return rec


def header(fmt, n, xyz, scale=SCALE, offset=OFFSET, fmt_byte=None, v14=None, legacy=None):
    """LAS 1.2 header (227 bytes) for formats up to 5, LAS 1.4 (375 bytes, 64-bit point count) for 6-10.  v14=True gives
    formats up to 5 the 1.4 header too; legacy=False leaves its legacy point count 0 (the 64-bit count then holds n)."""
    rl = FORMATS[fmt][0] if fmt in FORMATS else 34
    v14 = fmt >= 6 if v14 is None else v14
    legacy = not v14 if legacy is None else legacy
    size = 375 if v14 else 227
    h = bytearray(size)
    h[0:4] = b"LASF"
    h[24], h[25] = 1, (4 if v14 else 2)
    struct.pack_into("<HII", h, 94, size, size, 0)
    h[104] = fmt if fmt_byte is None else fmt_byte
    struct.pack_into("<HI", h, 105, rl, n if legacy else 0)
    struct.pack_into("<3d", h, 131, *scale)
    struct.pack_into("<3d", h, 155, *offset)
    w = world(xyz, scale, offset) if n else np.zeros((1, 3))
    for a in range(3):
        struct.pack_into("<2d", h, 179 + 16 * a, float(w[:, a].max()), float(w[:, a].min()))
    if v14:
        struct.pack_into("<Q", h, 247, n)
    return bytes(h)


def las_image(fmt, xyz, cls, rgb, t, fmt_byte=None, **hdr):
    rec = records(fmt, xyz, cls, rgb, t)
    return np.concatenate([np.frombuffer(header(fmt, len(xyz), xyz, fmt_byte=fmt_byte, **hdr), dtype=np.uint8), rec.reshape(-1)])


def last_image(fmt, xyz, cls, rgb, t, fmt_byte=None, **hdr):
    """The LAS record transposed by attribute: positions, time and colour as one block each, every other byte alone."""
    rl, toff, coff, _ = FORMATS[fmt]
    rec = records(fmt, xyz, cls, rgb, t)
    attrs, o = [], 0
    while o < rl:
        s = 12 if o == 0 else 8 if o == toff else 6 if o == coff else 1
        attrs.append((o, s))
        o += s
    body = np.concatenate([np.ascontiguousarray(rec[:, a:a + s]).reshape(-1) for a, s in attrs])
    return np.concatenate([np.frombuffer(header(fmt, len(xyz), xyz, fmt_byte=fmt_byte, **hdr), dtype=np.uint8), body])


def time_offset(fmt):
    return FORMATS[fmt][1]


def expect_records(xyz, sel, point_dtype):
    """The buffer collector's records of a time search, in file order: class 0, colour (0, 0, 0)."""
    idx = np.flatnonzero(sel)
    out = np.zeros(len(idx), dtype=point_dtype)
    w = world(xyz[idx])
    out["x"], out["y"], out["z"] = w[:, 0], w[:, 1], w[:, 2]
    return out


def select(t, start, end):
    """Range<f64>::contains on float64: NaN anywhere -> False."""
    with np.errstate(invalid="ignore"):
        return (t >= start) & (t < end)


def adversarial_times(n, start, end, seed):
    """Times on and around the bounds of [start, end), and the IEEE special values, shuffled among ordinary ones."""
    rng = np.random.default_rng(seed)
    special = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, 1e-310, -1e-310,
               1.0, -1.0, 1e300, -1e300]
    for b in (start, end):
        if np.isfinite(b):
            special += [b, np.nextafter(b, np.inf), np.nextafter(b, -np.inf)]
    t = rng.uniform(-2.0, 2.0, n)
    pick = rng.integers(0, 3, n) == 0
    t[pick] = rng.choice(np.array(special, dtype=np.float64), int(pick.sum()))
    return t


# [start, end) pairs the adversarial tests run: ordinary, at zero and in the denormals, whole line, empty, reversed, NaN
RANGES = [(-0.5, 0.5), (0.0, 1.0), (-0.0, 5e-324), (5e-324, 2.2250738585072009e-308), (-np.inf, np.inf), (-np.inf, 0.0),
          (1.0, np.inf), (1.0, 1.0), (1.0, -1.0), (np.nan, 1.0), (-1.0, np.nan)]
