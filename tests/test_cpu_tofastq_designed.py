"""BamToFastq's per-entry text (ngs-bits_amd/csrc/tofastq_visit.h - what the GPU library compiles into fq_keys_kernel and fq_format_kernel) on the CPU over the
designed runs (tests/tofastq_cases.py), against the Python restatement (tests/bamtofastq_oracle.py): the entry's size with the NUL cut-off of gzputs, the
throw bit, bam_endpos and the region rule per record; every entry byte by byte; and every entry through the format kernel's range split - for each alignment
of its start and every cut of its range each launch must write exactly its part. The same text runs as a stand-alone program under AddressSanitizer and
UBSan, and four value-only mutations of a scratch copy of the header must each be caught by a named run."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bamtofastq_oracle as Q
import emul_build
import tofastq_cases as K
from bamfilter_oracle import Rec
from conftest import ROOT

CSRC = os.path.join(ROOT, "ngs-bits_amd", "csrc")
HEADERS = ("tofastq_visit.h", "join_visit.h", "rec.h")
DENSE = 40   # entries of up to 2 * DENSE bytes meet every cut; longer ones the cuts within DENSE bytes of either end and every 251st between


def load(so):
    L = C.CDLL(so)
    L.tofastq_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tofastq_entry.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_void_p]
    L.tofastq_splits.restype = C.c_int64; L.tofastq_splits.argtypes = [C.c_char_p, C.c_uint32, C.c_int32, C.c_char_p, C.c_int32]
    return L


@pytest.fixture(scope="module")
def lib():
    return load(emul_build.library("tofastq_emul.cpp", include=[CSRC]))


@pytest.fixture(scope="module")
def runs():
    return {r.name: r for r in K.small_runs()}


def info(L, recs, extend, region):
    blob = np.frombuffer(b"".join(recs) + bytes(8), np.uint8)
    off = np.cumsum([0] + [len(b) for b in recs]).astype(np.int64)
    n = len(recs)
    inf, inr, end = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint8), np.zeros(n + 1, np.int64)
    tid, a, b = region if region else (-1, 0, 0)
    L.tofastq_info(blob.ctypes.data, off.ctypes.data, n, extend, tid, a, b, inf.ctypes.data, inr.ctypes.data, end.ctypes.data)
    return inf[:n], inr[:n], end[:n]


def differences(L, run, splits=True):
    """every record of the run at which the CPU build and the restatement differ: (index, what, got, expected)"""
    out = []
    recs, extend, region = run.records, run.kw.get("extend", 0), run.kw.get("region")
    inf, inr, end = info(L, recs, extend, region)
    for i, b in enumerate(recs):
        r = Rec(b)
        try:
            exp, throws = Q.entry(r, extend), False
        except Q.ComplementError:
            throws = True
            fwd = Rec(b[:18] + bytes([b[18] & ~0x10]) + b[19:])   # the bytes a thrower would have are never written: its size is that of the other strand's entry
            exp = None; size_exp = len(fwd.name) + 2 * max(r.l_seq, extend) + 6
        size, got_throws = int(inf[i]) & 0x3fffffff, bool(int(inf[i]) & 0x40000000)
        if got_throws != throws: out.append((i, "throws", got_throws, throws))
        if int(end[i]) != Q.endpos(r): out.append((i, "endpos", int(end[i]), Q.endpos(r)))
        if region and bool(inr[i]) != Q.in_region(r, region): out.append((i, "region", bool(inr[i]), Q.in_region(r, region)))
        if exp is None:
            continue
        if size != len(exp):
            out.append((i, "size", size, len(exp))); continue
        got = C.create_string_buffer(size + 1)
        L.tofastq_entry(b, size, extend, got)
        if got.raw[:size] != exp:
            out.append((i, "entry", got.raw[:size], exp)); continue
        if splits:
            bad = L.tofastq_splits(b, size, extend, exp, DENSE)
            if bad != -1:
                out.append((i, "split", (bad >> 60, (bad >> 56) & 15, (bad >> 24) & 0xffffffff, bad & 0xffffff), -1))
    return out


ALL = [f.__name__ for f in (K.bases, K.qualities, K.throws, K.fix, K.region, K.max_cached)]


@pytest.mark.parametrize("group", ALL)
def test_designed_records(lib, group):
    for run in getattr(K, group)():
        assert differences(lib, run) == [], run.name


def test_format_cuts_lie_where_designed_and_format(lib):
    run = K.format_cuts()
    e1, e2, c = run.expected()
    K.format_cut_premises(run, e1, e2)
    assert c["paired"] == len(run.records) // 2 and c["unmatched"] == 0
    assert differences(lib, run) == []


def test_names_with_more_than_one_nul(lib):
    """the "@" line is the name in front of the first NUL, as gzputs writes it (join_cases.c_string_names)"""
    import join_cases as J
    run = K.Run("c_string_names", J.c_string_names().tiles)
    assert differences(lib, run) == []
    e1, e2, c = run.expected()
    assert e1.count(b"@ab\n") == 1 and e2.count(b"@ab\n") == 1 and b"\0" not in e1 + e2 and c["paired"] == 7 and c["unmatched"] == 0


def test_stand_alone_under_sanitizers(tmp_path, runs):
    """the same text as a program of its own under AddressSanitizer and UBSan: every record in a heap buffer of exactly its size, every entry in one of exactly
    the announced size"""
    exe = emul_build.program("tofastq_emul_main.cpp", tmp_path, include=[CSRC], sanitize=True)
    for name in ("bases", "qualities_extend0", "qualities_extend12", "throws_in_tile", "region", "fix"):
        run = runs[name]
        recs = run.records
        (tmp_path / "recs").write_bytes(b"".join(recs))
        (tmp_path / "offs").write_bytes(np.cumsum([0] + [len(b) for b in recs]).astype(np.int64).tobytes())
        r = subprocess.run([exe, str(tmp_path / "recs"), str(tmp_path / "offs"), str(run.kw.get("extend", 0)), str(DENSE)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (name, r.stdout[-500:], r.stderr[-2000:])
        lines = r.stdout.strip().split("\n")
        assert len(lines) == len(recs) and all(l.endswith("splits -1") for l in lines), name


# value-only mutations of the header's text (no address moves): (label, text, replacement, the runs that must notice)
MUTATIONS = [
    ("the reverse quality index is off by one", "e.qual[e.rev ? e.lseq - 1 - k : k]", "e.qual[e.rev ? e.lseq - 1 - (k ? k - 1 : 0) : k]", {"qualities_extend0", "bases"}),
    ("qcut is off by one (forward)", "if (qu[j] == 223) { qcut = j; break; } }\n", "if (qu[j] == 223) { qcut = j + 1; break; } }\n", {"qualities_extend0", "qualities_extend12"}),
    ("endpos > start - 1 becomes >=", "rec_endpos(r) > (int64_t)reg_start - 1", "rec_endpos(r) >= (int64_t)reg_start - 1", {"region"}),
    ("lane - 8 < b - d1 becomes <=", "lane - 8 < b - d1", "lane - 8 <= b - d1", {"bases", "qualities_extend0"}),
]


def test_mutations_are_caught(tmp_path, runs):
    text = open(os.path.join(CSRC, "tofastq_visit.h")).read()
    table = {}
    for k, (label, old, new, must) in enumerate(MUTATIONS):
        d = tmp_path / ("m%d" % k); d.mkdir()
        assert text.count(old) == 1, label
        (d / "tofastq_visit.h").write_text(text.replace(old, new))
        for h in HEADERS[1:]:
            shutil.copy(os.path.join(CSRC, h), d / h)
        L = load(emul_build.library("tofastq_emul.cpp", d / "libtofastq_mut.so", include=[d]))
        caught = {name for name, run in runs.items() if differences(L, run)}
        table[label] = sorted(caught)
        assert must <= caught, (label, sorted(caught))
    print(table)
