"""trc_host_load_png (libtrc_host.so): synthetic PNGs written here with Python's zlib (levels 0 / 1 / 6 / 9, colour types 0 / 2 / 4 / 6,
random scanline filters), the reference's PNGs where present, a round trip through trc_host_write_png, and corrupt / unsupported
files.  CPU only."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from tracer_amd import abi, host

REF_PNGS = ["uv_test/uv_test.png", "coatball/tex_ao.png", "coatball/tex_metallic.png", "scuffed/gold-scuffed_base.png",
            "scuffed/gold-scuffed_normal.png", "scuffed/gold-scuffed_metallic.png", "scuffed/gold-scuffed_roughness.png"]
REF_ROOT = "/root/reference/RT_Metal"
CHANNELS = {0: 1, 2: 3, 4: 2, 6: 4}


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def _filter_rows(pixels, bpp, rng):
    """pixels: (h, stride) uint8 -> filtered scanlines with a random filter type per row (PNG specification section 9)."""
    h, stride = pixels.shape
    out = bytearray()
    prev = np.zeros(stride, dtype=np.int32)
    for y in range(h):
        cur = pixels[y].astype(np.int32)
        ft = int(rng.integers(0, 5))
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if stride > bpp else np.zeros(stride, np.int32)
        a = a[:stride]
        c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])[:stride] if stride > bpp else np.zeros(stride, np.int32)
        if ft == 0:
            f = cur
        elif ft == 1:
            f = cur - a
        elif ft == 2:
            f = cur - prev
        elif ft == 3:
            f = cur - ((a + prev) >> 1)
        else:
            f = cur - np.array([_paeth(int(x), int(y_), int(z)) for x, y_, z in zip(a, prev, c)], dtype=np.int32)
        out.append(ft)
        out += (f & 0xFF).astype(np.uint8).tobytes()
        prev = cur
    return bytes(out)


def make_png(pixels, ctype, level=6, rng=None, depth=8, interlace=0, raw=None):
    """pixels: (h, w, channels) uint8, rows top-down."""
    h, w = pixels.shape[:2]
    ch = CHANNELS.get(ctype, 1)
    rng = rng or np.random.default_rng(0)
    data = raw if raw is not None else _filter_rows(pixels.reshape(h, w * ch), ch, rng)
    ihdr = struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(data, level)) + _chunk(b"IEND", b"")


def expected_rgb(pixels, ctype):
    """what the reader must return: byte / 255 as float32, grey replicated, alpha dropped, rows bottom-up."""
    p = pixels.astype(np.float32) / np.float32(255.0)
    rgb = np.repeat(p[..., :1], 3, axis=2) if ctype in (0, 4) else p[..., :3]
    return np.ascontiguousarray(rgb[::-1]).astype(np.float32)


def load(path):
    w, h = C.c_uint32(), C.c_uint32()
    p = C.POINTER(C.c_float)()
    L = host.lib()
    st = L.trc_host_load_png(os.fsencode(str(path)), C.byref(w), C.byref(h), C.byref(p))
    if st != abi.OK:
        assert not p, "a failed load must not hand out a buffer"
        return st, None
    try:
        return st, np.ctypeslib.as_array(p, shape=(h.value, w.value, 3)).copy()
    finally:
        L.trc_host_free(p)


@pytest.mark.parametrize("level", [0, 1, 6, 9])
@pytest.mark.parametrize("ctype", [0, 2, 4, 6])
@pytest.mark.parametrize("width", [1, 3, 7, 64])
def test_synthetic_png_bit_exact(tmp_path, level, ctype, width):
    rng = np.random.default_rng(1000 * level + 10 * ctype + width)
    height = int(rng.integers(1, 20))
    px = rng.integers(0, 256, size=(height, width, CHANNELS[ctype]), dtype=np.uint8)
    if width == 64:     # some long runs so that the compressor emits back-references
        px[: height // 2] = px[0, 0]
    f = tmp_path / "t.png"
    f.write_bytes(make_png(px, ctype, level, rng))
    st, got = load(f)
    assert st == abi.OK
    exp = expected_rgb(px, ctype)
    assert got.shape == exp.shape
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(host.load_png(f), exp)


def test_large_dynamic_huffman(tmp_path):
    """a larger RGB image with structure: dynamic Huffman blocks and long matches across scanlines"""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:300, 0:257]
    px = np.stack([(x * 3) & 255, (y * 5) & 255, ((x ^ y) + rng.integers(0, 4, size=x.shape)) & 255], axis=2).astype(np.uint8)
    for level in (1, 9):
        f = tmp_path / f"big{level}.png"
        f.write_bytes(make_png(px, 2, level, rng))
        st, got = load(f)
        assert st == abi.OK and np.array_equal(got, expected_rgb(px, 2))


def _unfilter_numpy(raw, w, h, ch):
    stride = w * ch
    out = np.zeros((h, stride), dtype=np.int32)
    prev = np.zeros(stride, dtype=np.int32)
    for yy in range(h):
        row = raw[yy * (stride + 1):(yy + 1) * (stride + 1)]
        ft, f = row[0], np.frombuffer(row[1:], dtype=np.uint8).astype(np.int32)
        cur = np.zeros(stride, dtype=np.int32)
        for i in range(stride):
            a = cur[i - ch] if i >= ch else 0
            b = prev[i]
            c = prev[i - ch] if i >= ch else 0
            pred = [0, a, b, (a + b) >> 1, _paeth(a, b, c)][ft]
            cur[i] = (f[i] + pred) & 0xFF
        out[yy] = cur
        prev = cur
    return out.reshape(h, w, ch).astype(np.uint8)


def _independent_decode(path):
    d = open(path, "rb").read()
    pos, idat = 8, b""
    while pos < len(d):
        n = struct.unpack(">I", d[pos:pos + 4])[0]
        kind = d[pos + 4:pos + 8]
        body = d[pos + 8:pos + 8 + n]
        if kind == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
        elif kind == b"IDAT":
            idat += body
        pos += n + 12
    try:
        from PIL import Image
        im = Image.open(path)
        im.load()
        px = np.asarray(im)
        if px.ndim == 2:
            px = px[..., None]
    except ImportError:
        px = _unfilter_numpy(zlib.decompress(idat), w, h, CHANNELS[ctype])
    return px, ctype


@pytest.mark.parametrize("name", REF_PNGS)
def test_reference_pngs(name):
    path = os.path.join(REF_ROOT, name)
    if not os.path.exists(path):
        pytest.skip("the reference's PNGs are not on this machine")
    px, ctype = _independent_decode(path)
    st, got = load(path)
    assert st == abi.OK
    assert np.array_equal(got.view(np.uint32), expected_rgb(px, ctype).view(np.uint32))


def test_roundtrip_write_png(tmp_path):
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, size=(13, 29, 4), dtype=np.uint8)
    f = tmp_path / "w.png"
    host.write_png(str(f), rgba)
    st, got = load(f)
    assert st == abi.OK and np.array_equal(got, expected_rgb(rgba, 6))


def _good(rng):
    px = rng.integers(0, 256, size=(9, 11, 3), dtype=np.uint8)
    return make_png(px, 2, 6, rng)


def test_corrupt_files(tmp_path):
    rng = np.random.default_rng(11)
    good = bytearray(_good(rng))
    f = tmp_path / "c.png"

    def status(data):
        f.write_bytes(bytes(data))
        return load(f)[0]

    assert status(good) == abi.OK
    idat = good.find(b"IDAT")
    n = struct.unpack(">I", good[idat - 4:idat])[0]
    # a flipped CRC byte (of IHDR, of IDAT)
    for at in (8 + 4 + 4 + 13, idat + 4 + n):
        bad = bytearray(good); bad[at] ^= 0x01
        assert status(bad) == abi.ERR_INVALID_ARG
    # a bad Adler-32 (last 4 bytes of the zlib stream), CRC recomputed so that only the checksum is wrong
    z = bytearray(good[idat + 4:idat + 4 + n]); z[-1] ^= 0x40
    bad = good[:idat - 4] + _chunk(b"IDAT", bytes(z)) + _chunk(b"IEND", b"")
    assert status(bad) == abi.ERR_INVALID_ARG
    # a truncated IDAT (consistent chunk, stream cut short), and a file cut anywhere
    bad = good[:idat - 4] + _chunk(b"IDAT", bytes(good[idat + 4:idat + 4 + n // 2])) + _chunk(b"IEND", b"")
    assert status(bad) == abi.ERR_INVALID_ARG
    for cut in (0, 7, 20, idat + 10, len(good) - 13, len(good) - 1):
        assert status(good[:cut]) == abi.ERR_INVALID_ARG
    # a lying IHDR size (bigger and smaller than the data), CRC valid
    for w, h in ((12, 9), (11, 8), (11, 10), (1 << 20, 1 << 20)):
        ihdr = struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)
        bad = good[:8] + _chunk(b"IHDR", ihdr) + good[8 + 25:]
        assert status(bad) == abi.ERR_INVALID_ARG, (w, h)
    # a random filter byte out of range
    px = rng.integers(0, 256, size=(3, 4, 3), dtype=np.uint8)
    raw = b"".join(b"\x07" + px[y].tobytes() for y in range(3))
    assert status(make_png(px, 2, raw=raw)) == abi.ERR_INVALID_ARG
    # fuzz: random byte flips and truncations never crash and never succeed with a wrong size
    for k in range(300):
        bad = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            bad[int(rng.integers(8, len(bad)))] ^= int(rng.integers(1, 256))
        if k % 3 == 0:
            bad = bad[:int(rng.integers(8, len(bad)))]
        st, got = load_bytes(f, bad)
        assert st in (abi.OK, abi.ERR_INVALID_ARG, abi.ERR_UNSUPPORTED)
        if st == abi.OK:
            assert got.shape == (9, 11, 3)


def load_bytes(f, data):
    f.write_bytes(bytes(data))
    return load(f)


def test_unsupported_formats(tmp_path):
    rng = np.random.default_rng(5)
    f = tmp_path / "u.png"
    px = rng.integers(0, 4, size=(4, 5, 1), dtype=np.uint8)
    # palette (colour type 3, with a PLTE chunk)
    data = make_png(px, 3)
    plte = _chunk(b"PLTE", bytes(range(12)))
    data = data[:33] + plte + data[33:]
    f.write_bytes(data)
    assert load(f)[0] == abi.ERR_UNSUPPORTED
    # 16-bit RGB
    px16 = rng.integers(0, 256, size=(4, 5, 6), dtype=np.uint8)
    raw = b"".join(b"\x00" + px16[y].tobytes() for y in range(4))
    f.write_bytes(make_png(px16, 2, depth=16, raw=raw))
    assert load(f)[0] == abi.ERR_UNSUPPORTED
    # Adam7 interlaced
    px8 = rng.integers(0, 256, size=(4, 5, 3), dtype=np.uint8)
    f.write_bytes(make_png(px8, 2, interlace=1))
    assert load(f)[0] == abi.ERR_UNSUPPORTED
    # not a PNG at all / missing file
    f.write_bytes(b"GIF89a" + bytes(40))
    assert load(f)[0] == abi.ERR_INVALID_ARG
    assert load(tmp_path / "nope.png")[0] == abi.ERR_INVALID_ARG
