"""tests/deflate_model.py, the specification of the BGZF encoder (csrc/deflate.hip), checked without a GPU: on every piece of tests/deflate_cases.py at every
level its members inflate with zlib to the piece (CRC32 and ISIZE right), its chain equals the kernel's round loop, every required path of the catalogue is
reached, and on the fixture streams it stays within the size bar of tests/test_gpu_bgzf_write.py."""
import gzip
import os
import struct
import time
import zlib

import numpy as np
import pytest

import deflate_cases as D
import deflate_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GI = os.path.join(ROOT, "tests", "golden", "ref_in")
LEVELS = (0, 1, 2, 3, None)
RATIO_BAR = 1.35
STREAMS = ["MappingQC_in2.bam", "MappingQC_in4.bam", "Statistics_mapqc_wgs.bam", "BamReader_rna.bam"]


def members(z):
    out, o = [], 0
    while o < len(z):
        assert z[o:o + 16] == M.HEADER, o
        bsize = struct.unpack_from("<H", z, o + 16)[0] + 1
        assert bsize <= 65536 and o + bsize <= len(z)
        crc, isize = struct.unpack_from("<II", z, o + bsize - 8)
        out.append((z[o + 18:o + bsize - 8], crc, isize))
        o += bsize
    return out


@pytest.fixture(scope="module")
def outputs():
    """{case name: (data, {level: (bytes, stats)})}"""
    out = {}
    for c in D.CASES:
        d = c.data()
        out[c.name] = (d, {lv: M.compress_stats(d, lv) for lv in LEVELS})
    return out


def test_every_case_inflates(outputs):
    for name, (d, by_level) in outputs.items():
        for lv, (z, _) in by_level.items():
            ms = members(z)
            assert len(ms) == (len(d) + M.PIECE - 1) // M.PIECE, (name, lv)
            for i, (payload, crc, isize) in enumerate(ms):
                piece = d[i * M.PIECE:(i + 1) * M.PIECE]
                dz = zlib.decompressobj(-15)
                got = dz.decompress(payload) + dz.flush()
                assert dz.eof and not dz.unused_data and got == piece, (name, lv, i)
                assert crc == zlib.crc32(piece) and isize == len(piece), (name, lv, i)
            assert (gzip.decompress(z) if z else b"") == d, (name, lv)


def test_high_levels_are_the_default_parse(outputs):
    for name, (d, by_level) in outputs.items():
        if len(d) <= 8192:
            for lv in range(4, 10):
                assert M.compress(d, lv) == by_level[None][0], (name, lv)


def test_required_paths(outputs):
    counts = {p: 0 for p in D.REQUIRED_PATHS}
    for c in D.CASES:
        sl = {lv: st for lv, (_, st) in outputs[c.name][1].items() if lv != 0}
        for p in D.REQUIRED_PATHS:
            counts[p] += sum(D.PATHS[p](s) for s in sl.values())
        assert c.path in D.UNREACHED or any(D.PATHS[c.path](s) for s in sl.values()), (c.name, c.path)
        if c.expect:
            assert c.expect(sl), c.name
    for p, k in counts.items():
        print(f"path {p}: {k} (case, level) pairs")
    assert all(counts.values()), [p for p, k in counts.items() if not k]
    depths = {name: outputs[name][1][None][1][0] for name in ("deep_litlen", "deep_dist", "deep_codelen")}
    print("depths without the limit:", {k: (s.depth_litlen, s.depth_dist, s.depth_codelen) for k, s in depths.items()})
    for name, (d, by_level) in outputs.items():
        if by_level[None][1]:
            s = by_level[None][1][0]
            print(f"  {name}: n={len(d)} stored={s.stored} margin={s.margin} hlit={s.hlit} hdist={s.hdist} hclen={s.hclen}")


def test_level0_stores(outputs):
    for name, (d, by_level) in outputs.items():
        assert all(s.stored for s in by_level[0][1]), name


def test_chain_equals_the_round_loop(outputs):
    rng = np.random.default_rng(3)
    pieces = [outputs[n][0][:M.PIECE] for n in ("hash_collisions", "lookback_32", "lookback_33", "chain_48_inside", "zeros", "size_65280", "period_32768")]
    pieces += [bytes(rng.integers(0, 3, 3000, dtype=np.uint8)), bytes(rng.integers(0, 256, 20000, dtype=np.uint8)), b"ab", b"abc"]
    for p in pieces:
        assert M.chain(p).tolist() == M.chain_rounds(p)


def _bam_stream(path):
    with open(path, "rb") as f:
        return gzip.decompress(f.read())


@pytest.mark.parametrize("name", STREAMS)
def test_fixture_streams_within_the_bar(name):
    data = _bam_stream(os.path.join(GI, name))[:10 * M.PIECE]
    t = time.time()
    z, stats = M.compress_stats(data)
    dt = time.time() - t
    assert gzip.decompress(z) == data
    zl = 0
    for o in range(0, len(data), M.PIECE):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        zl += len(c.compress(data[o:o + M.PIECE]) + c.flush()) + 26
    print(f"{name}: {len(stats)} pieces, {dt / len(stats):.2f} s per piece (default parse), size {len(z) / zl:.3f} x zlib-6")
    assert len(z) <= RATIO_BAR * zl
