"""The BGZF encoder (ngsqc_bgzf_compress / ngsqc_bgzf_compress_level, csrc/deflate.hip) gives the bytes of its specification, tests/deflate_model.py, byte for
byte: on every piece of tests/deflate_cases.py at levels 0, 1, 2, 3, 4, 6, 9 and the default, on the first pieces of fixture streams, across the grid stride
(one workgroup deflating a second member of another shape after its first) and across the windows of 16384 pieces of ngsqc_bgzf_compress. Every member also
inflates with zlib and two runs give the same bytes. A zlib round trip alone cannot see a parse that drifts from its design while staying valid DEFLATE."""
import ctypes as C
import gzip
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_cases as D
import deflate_model as M
from test_gpu_bgzf_write import members

ngsqc = __import__("importlib").import_module("ngs-bits_amd")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GI = os.path.join(ROOT, "tests", "golden", "ref_in")
PIECE = M.PIECE
LEVELS = (0, 1, 2, 3, 4, 6, 9, None)
WINDOW_PIECES = 16384

_model = {}


def model(data, level):
    """the model's bytes, computed once per session per distinct parse (levels 4-9 and None share one)"""
    key = (id(data), M.params(level))
    if key not in _model:
        _model[key] = (data, M.compress(data, level))
    return _model[key][1]


def inflate_all(z, data):
    ms = members(z)
    assert len(ms) == (len(data) + PIECE - 1) // PIECE
    for i, (_, _, payload, crc, isize) in enumerate(ms):
        piece = data[i * PIECE:(i + 1) * PIECE]
        d = zlib.decompressobj(-15)
        got = d.decompress(payload) + d.flush()
        assert d.eof and not d.unused_data and got == piece, i
        assert crc == zlib.crc32(piece) and isize == len(piece), i
    return ms


@pytest.fixture(scope="module")
def case_data():
    return {c.name: c.data() for c in D.CASES}


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_case_exact(case_data, name):
    data = case_data[name]
    for level in LEVELS:
        z = ngsqc.bgzf_compress(data, level=level)
        assert z == model(data, level), (name, level)
        if data:
            inflate_all(z, data)
        assert ngsqc.bgzf_compress(data, level=level) == z, (name, level)


def _bam_stream(name):
    with open(os.path.join(GI, name), "rb") as f:
        return gzip.decompress(f.read())


@pytest.mark.parametrize("name", ["MappingQC_in2.bam", "Statistics_mapqc_wgs.bam"])
def test_fixture_streams_exact(name):
    data = _bam_stream(name)[:3 * PIECE]
    for level in (1, None):
        assert ngsqc.bgzf_compress(data, level=level) == model(data, level), level


def _compute_units():
    code = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, check=True)
    return int(out.stdout.strip().splitlines()[-1])


def _acgt(seed, n):
    return (np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8) * 7 % 26 + 65).tobytes()


def test_grid_stride():
    """grid = min(members, 2 x CUs); 2 x grid + 3 pieces, so that workgroup m deflates pieces m, m + grid and (m < 3) m + 2 grid. For m < 16 the two pieces
    of a workgroup differ in shape: stored then dynamic, dynamic then stored, and a piece that repeats its partner's trigrams at other positions (a head
    entry left over from the partner would be found). The last piece is 7 bytes."""
    grid = 2 * _compute_units()
    n_pieces = 2 * grid + 3
    rnd = lambda m: np.random.default_rng(m).integers(0, 256, PIECE, dtype=np.uint8).tobytes()
    pieces = [_acgt(m, PIECE) for m in range(n_pieces)]
    for m in range(16):
        if m % 3 == 0:
            pieces[m] = rnd(m)
        elif m % 3 == 1:
            pieces[m + grid] = rnd(m + grid)
        else:
            text = _acgt(1000 + m, PIECE)
            pieces[m] = text
            pieces[m + grid] = text[PIECE // 3:] + text[:PIECE // 3]
    pieces[-1] = pieces[-1][:7]
    data = b"".join(pieces)
    z = ngsqc.bgzf_compress(data)
    ms = inflate_all(z, data)
    for m in list(range(16)) + [m + grid for m in range(16)] + [2 * grid, 2 * grid + 1, 2 * grid + 2]:
        o, bsize = ms[m][0], ms[m][1]
        assert z[o:o + bsize] == M.member(pieces[m]), m
    assert ngsqc.bgzf_compress(data) == z


def test_window_loop():
    """more than one window (16384 pieces, about 1.07 GB) of ngsqc_bgzf_compress at levels 0 and 1: needs about 3 GB of host memory. Every piece is the same
    ACGT text with its index stamped into it, so that no two pieces are equal."""
    n_pieces = WINDOW_PIECES + 2
    base = np.frombuffer(_acgt(5, PIECE), np.uint8)
    arr = np.tile(base, n_pieces + 1)[:n_pieces * PIECE + 1000].copy()
    idx = np.arange(n_pieces, dtype=np.uint32)
    stamp = idx.view(np.uint8).reshape(n_pieces, 4)
    for k in range(4):
        arr[np.arange(n_pieces) * PIECE + 1000 + k] = stamp[:, k]
    data = arr.tobytes()
    del arr
    n_all = (len(data) + PIECE - 1) // PIECE
    for level in (0, 1):
        z = ngsqc.bgzf_compress(data, level=level)
        zv, dv = memoryview(z), memoryview(data)
        ms, o = [], 0
        while o < len(z):                  # (offsets only: a list of every payload would hold another copy of the stream)
            assert z[o:o + 4] == b"\x1f\x8b\x08\x04", (level, o)
            bsize = int.from_bytes(z[o + 16:o + 18], "little") + 1
            ms.append((o, bsize))
            o += bsize
        assert o == len(z) and len(ms) == n_all
        for i, (o, bsize) in enumerate(ms):
            d = zlib.decompressobj(-15)
            got = d.decompress(zv[o + 18:o + bsize - 8]) + d.flush()
            assert d.eof and not d.unused_data and got == dv[i * PIECE:(i + 1) * PIECE], (level, i)
            assert int.from_bytes(z[o + bsize - 8:o + bsize - 4], "little") == zlib.crc32(got), (level, i)
        for i in (WINDOW_PIECES - 1, WINDOW_PIECES, WINDOW_PIECES + 1, n_all - 1):
            o, bsize = ms[i]
            assert z[o:o + bsize] == M.member(data[i * PIECE:(i + 1) * PIECE], level), (level, i)
        out = (C.c_uint8 * 16)()
        got = C.c_size_t(0)
        rc = ngsqc.lib().ngsqc_bgzf_compress_level(data, len(data), 0, level, C.cast(out, C.c_void_p), 16, C.byref(got))
        assert rc == -3 and got.value == len(z), level
        del z, zv, ms
