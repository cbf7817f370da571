"""The BGZF encoder of the BAM writer (ngsqc_bgzf_compress, csrc/deflate.hip) checked with Python's zlib / gzip: every member inflates to its 0xff00-byte slice,
CRC32, ISIZE and BSIZE are right, no member is larger than 65536 bytes, two runs give the same bytes, and the output is at most 1.35 x the size of zlib level 6
over the same pieces."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import bamgen_lib as G

ngsqc = __import__("importlib").import_module("ngs-bits_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GI = os.path.join(ROOT, "tests", "golden", "ref_in")
PIECE = 0xff00
RATIO_BAR = 1.35


def members(z):
    """(offset, length, payload, crc, isize) of every BGZF member of z"""
    out, o = [], 0
    while o < len(z):
        assert z[o:o + 4] == b"\x1f\x8b\x08\x04", o
        xlen = struct.unpack_from("<H", z, o + 10)[0]
        assert xlen == 6 and z[o + 12:o + 16] == b"BC\x02\x00", o
        bsize = struct.unpack_from("<H", z, o + 16)[0] + 1
        assert bsize <= 65536 and o + bsize <= len(z)
        crc, isize = struct.unpack_from("<II", z, o + bsize - 8)
        out.append((o, bsize, z[o + 18:o + bsize - 8], crc, isize))
        o += bsize
    return out


def check(data):
    z = ngsqc.bgzf_compress(data)
    ms = members(z)
    assert len(ms) == (len(data) + PIECE - 1) // PIECE
    for i, (_, _, payload, crc, isize) in enumerate(ms):
        piece = data[i * PIECE:(i + 1) * PIECE]
        d = zlib.decompressobj(-15)
        got = d.decompress(payload) + d.flush()
        assert d.eof and not d.unused_data, i
        assert got == piece, i
        assert crc == zlib.crc32(piece) and isize == len(piece), i
    if data:
        assert gzip.decompress(z) == data
    assert ngsqc.bgzf_compress(data) == z   # deterministic
    return z


def zlib6_size(data):
    """BGZF bytes htslib's level 6 gives for the same pieces (raw DEFLATE + 26 bytes of framing per member)"""
    n = 0
    for o in range(0, len(data), PIECE):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        n += len(c.compress(data[o:o + PIECE]) + c.flush()) + 26
    return n


def test_small_and_edge_sizes():
    assert ngsqc.bgzf_compress(b"") == b""
    check(b"A")
    rng = np.random.default_rng(7)
    base = bytes(rng.integers(0, 4, PIECE + 1, dtype=np.uint8) + 65)
    check(base[:PIECE])
    check(base[:PIECE + 1])
    check(b"ACGT" * 10)
    check(bytes(range(256)) * 3)


def test_random_takes_the_stored_fallback():
    data = bytes(np.random.default_rng(11).integers(0, 256, 8 << 20, dtype=np.uint8))
    z = check(data)
    ms = members(z)
    assert all(p[0] & 6 == 0 for _, _, p, _, _ in ms)   # BTYPE 00: stored
    assert max(b for _, b, _, _, _ in ms) <= 65536


def test_zeros():
    data = bytes(8 << 20)
    z = check(data)
    print(f"zeros: {len(data) / len(z):.1f} x")
    assert len(z) < len(data) // 50


@pytest.mark.parametrize("period", [32767, 32769])
def test_period_near_window(period):
    rng = np.random.default_rng(period)
    unit = bytes(rng.integers(0, 256, period, dtype=np.uint8))
    data = (unit * (3 * PIECE // period + 2))[:3 * PIECE + 17]
    check(data)


def _bam_stream(path):
    with open(path, "rb") as f:
        return gzip.decompress(f.read())


STREAMS = ["MappingQC_in2.bam", "MappingQC_in4.bam", "Statistics_mapqc_wgs.bam", "BamReader_rna.bam", "BamFilter/BamFilter_in1.bam", "BamFilter/BamFilter_in2.bam"]


def _ratio(name, data):
    z = check(data)
    r = len(z) / zlib6_size(data)
    print(f"{name}: {len(data)} bytes, ratio {len(data) / len(z):.2f} (zlib-6 {len(data) / zlib6_size(data):.2f}), size vs zlib-6 {r:.3f}")
    return r


@pytest.mark.parametrize("name", STREAMS)
def test_fixture_streams(name):
    r = _ratio(name, _bam_stream(os.path.join(GI, name)))
    if not name.startswith("BamFilter"):   # (2 KB streams: the fixed cost of a dynamic header is a large share)
        assert r <= RATIO_BAR


@pytest.mark.parametrize("flavor", [0, 3, 5])
def test_bamgen_streams(flavor):
    img = G.generate(200_000, flavor=flavor, level=1)
    data = gzip.decompress(img.tobytes())
    assert _ratio(f"bamgen flavor {flavor}", data) <= RATIO_BAR


def test_too_small_buffer_reports_the_whole_size():
    import ctypes as C
    data = bytes(np.random.default_rng(5).integers(0, 4, 3 * PIECE, dtype=np.uint8) + 65)
    full = ngsqc.bgzf_compress(data)
    out = (C.c_uint8 * 16)(); got = C.c_size_t(0)
    rc = ngsqc.lib().ngsqc_bgzf_compress(data, len(data), 0, C.cast(out, C.c_void_p), 16, C.byref(got))
    assert rc == -3 and got.value == len(full)
