"""The device's FASTQ reader (ngs-bits_amd/csrc/fastq_visit.h - the text the GPU library compiles into the kernels of csrc/fastqin.hip) on the CPU, against the
Python model (tests/fastq_model.py): the line index, the entries, every counter and the first error - on the designed texts (tests/fastq_cases.py) and on the
reference's five ReadQC inputs. Integer code and the reference's double division: held here without a GPU."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import emul_build
import fastq_cases as K
import fastq_model as M
from conftest import ROOT

GI = os.path.join(ROOT, "tests", "golden", "ref_in", "ReadQC")
NO_ERROR = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(emul_build.library("fastqin_emul.cpp"))
    L.fastq_block.restype = C.c_int32
    L.fastq_emul.argtypes = [C.c_char_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint64] + [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 2
    return L


def prepared(text, last):
    """what the accumulator does on the host before a piece reaches the device: the last piece of a file gets its missing final newline, and the lines at the
    end that are empty ("" or "\\r") stay behind (in the carry; behind the last piece they are dropped)"""
    text = bytes(text)
    if last and text and not text.endswith(b"\n"):
        text += b"\n"
    while True:
        if text.endswith(b"\n") and (len(text) == 1 or text[-2:-1] == b"\n"):
            text = text[:-1]
        elif text.endswith(b"\r\n") and (len(text) == 2 or text[-3:-2] == b"\n"):
            text = text[:-2]
        else:
            return text


def emulate(L, text, reverse=False, long_read=False, last=True, entry_base=0):
    text = prepared(text, last)
    acc, out, cyc = np.zeros(328, np.uint64), np.zeros(6, np.uint64), np.zeros((320, 7), np.uint64)
    lens, lines = np.zeros(len(text) + 2, np.uint64), np.zeros(len(text) + 2, np.uint32)
    L.fastq_emul(text, len(text), int(last), int(reverse), int(long_read), entry_base, acc.ctypes.data, out.ctypes.data, lens.ctypes.data, len(text), cyc.ctypes.data, lines.ctypes.data)
    a = acc.astype(np.int64)
    n_lines, max_cycles = int(out[0]), int(out[5])
    got = {"c_forward": int(a[0]), "c_reverse": int(a[1]), "bases_sequenced": int(a[2]), "bases": a[3:8], "base_qualities": a[8:108], "read_qualities": a[108:208],
           "qscore_dist_r1": a[208:268], "qscore_dist_r2": a[268:328], "max_cycles": max_cycles, "n_unknown_base": 0, "n_quality_out_of_range": 0,
           "read_lengths": lens[:max_cycles + 1].astype(np.int64), "cycles": cyc.astype(np.int64)}
    err = None if int(out[3]) == NO_ERROR else (int(out[3]) >> 8, int(out[3]) & 255)
    return got, {"lines": lines[:n_lines + 1].tolist(), "entries": int(out[1]), "carry": int(out[2]), "headers": int(out[4])}, err


def same(got, exp):
    assert sorted(got) == sorted(exp)
    for k in exp:
        assert np.array_equal(np.asarray(got[k]), np.asarray(exp[k])), k


def check(L, text, reverse=False, long_read=False):
    st, index, err = M.run([(text, reverse)], long_read)
    got, info, gerr = emulate(L, text, reverse, long_read)
    assert gerr == (None if err is None else (err[1], err[2]))
    if err is None:
        same(got, st.fields())
        assert info["headers"] == index[0] and info["entries"] == len(M.entries_of(text)) and info["carry"] == len(prepared(text, True))
    return info


def test_block_is_the_designed_one(lib):
    assert lib.fastq_block() == K.B


@pytest.mark.parametrize("long_read", [False, True])
def test_designed_text(lib, long_read):
    text = K.designed(long_read)
    assert {0, K.B - 1} <= K.newline_offsets_hit(text)
    info = check(lib, text, False, long_read)
    check(lib, text, True, long_read)
    # the line index is the offsets behind the newlines
    a = np.frombuffer(text, np.uint8)
    assert info["lines"] == [0] + (np.nonzero(a == 10)[0] + 1).tolist()
    st, index, _ = M.run([(text, False)], long_read)
    assert set(K.LENGTHS) <= set(st.lengths) and index[0] == len(M.entries_of(text)) - 2      # (two entries have no header)
    assert st.base_qualities[0] > 300 and st.base_qualities[93 if long_read else 41] > 300
    if not long_read:                       # qualities above 41 are long-read only: the same text is an error without the flag
        assert M.run([(K.designed(True), False)], False)[2][2] == M.ERR_QUALITY


def test_sizes_and_file_ends(lib):
    for name, text in K.size_cases().items():
        check(lib, text)
    text = K.designed()
    exp = M.run([(text, False)])[0].fields()
    for name, v in K.variants(text).items():
        got, _, err = emulate(lib, v)
        assert err is None, name
        same(got, exp)
        same(M.run([(v, False)])[0].fields(), exp)


def test_a_piece_that_is_not_the_last_keeps_its_tail(lib):
    text = K.designed()
    cut = len(text) // 2
    got, info, err = emulate(lib, text[:cut], last=False)
    lines = M.lines_of(text[:cut] + (b"" if text[cut - 1:cut] == b"\n" else b"\n"))
    n_complete = text[:cut].count(b"\n")
    assert err is None and info["entries"] == n_complete // 4
    assert info["carry"] == len(b"".join(l + b"\n" for l in lines[:4 * (n_complete // 4)]))
    rest, _, err2 = emulate(lib, text[info["carry"]:], entry_base=info["entries"])
    assert err2 is None
    exp = M.run([(text, False)])[0].fields()
    for k in ("c_forward", "bases_sequenced"):
        assert got[k] + rest[k] == exp[k]
    for k in ("bases", "base_qualities", "read_qualities", "qscore_dist_r1", "cycles"):
        assert np.array_equal(got[k] + rest[k], exp[k]), k


@pytest.mark.parametrize("long_read", [False, True])
def test_error_cases(lib, long_read):
    cases = K.error_cases(long_read)
    assert {c[2][1] for c in cases} == {1, 2, 3, 4, 5, 6}
    for name, text, expect, _ in cases:
        _, _, err = M.run([(text, False)], long_read)
        assert (err[1], err[2]) == expect, name
        _, _, got = emulate(lib, text, long_read=long_read)
        assert got == expect, name
        _, _, got = emulate(lib, text, long_read=long_read, entry_base=1000)
        assert got == (expect[0] + 1000, expect[1]), name


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_reference_inputs(lib, k):
    text = gzip.open(os.path.join(GI, "ReadQC_in%d.fastq.gz" % k)).read()
    check(lib, text, reverse=k in (2, 4), long_read=k == 5)
