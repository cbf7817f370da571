"""The position table of the site pileup, its scan rider and the indel windows (ngs-bits_amd/csrc/postable.h) on the CPU: tests/emul/postable_emul.cpp compiles
the header's own text - the host builder every table goes through, and the two lookups that walk_scan_kernel, pileup_kernel, pileup_long_kernel and the window
kernels inline - and this file holds them to bisect_left over each reference's positions: every lookup must be first + bisect_left(positions of the reference, x).
The geometry sits on both sides of a 64 kb bucket edge, behind a reference's end and in references without items; the builder's first error must be the one
each of its three callers reported when they carried the loop themselves (reference id, the item's own checks, then order inside a run or contiguity). The same
cases run once more in a stand-alone program under AddressSanitizer and UBSan, every array in a heap buffer of exactly its size."""
import ctypes as C
import subprocess
from bisect import bisect_left

import numpy as np
import pytest

import emul_build
import pileup_model as PM

SHIFT = PM.PILEUP_BUCKET_SHIFT
BUCKET = 1 << SHIFT
SITES, WINDOWS, REGIONS = 0, 1, 2
NOUN = {SITES: "site", WINDOWS: "window", REGIONS: "region"}
MERGED = "Merged and sorted BED file required for coverage details statistics!"
UNSORTED = {SITES: "sites must be sorted by position within a reference", WINDOWS: "windows must be sorted by start within a reference", REGIONS: MERGED}
SPLIT = {SITES: "sites of one reference must be contiguous", WINDOWS: "windows of one reference must be contiguous", REGIONS: MERGED}
OWN = {SITES: "a site is a single 1-based position (start == end)", WINDOWS: "invalid window range", REGIONS: "invalid region range"}


class Item(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("tid", "start", "end", "kind", "len", "has_allele", "has_slice")]


def item(tid, start, end=None, kind=0, length=0, has_allele=0, has_slice=0):
    return (tid, start, start if end is None else end, kind, length, has_allele, has_slice)


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(emul_build.library("postable_emul.cpp"))
    L.postable_emul_build.restype = C.c_void_p
    L.postable_emul_build.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_char_p]
    L.postable_emul_free.argtypes = [C.c_void_p]
    L.postable_emul_array.restype = C.c_int64
    L.postable_emul_array.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    L.postable_emul_lower.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    return L


class Table:
    """the emulator's table of (rules, items, ref_lens): .error, or the five arrays and lower(form, tid, xs)"""

    def __init__(self, L, rules, items, ref_lens):
        self.L = L
        arr = (Item * max(len(items), 1))(*[Item(*i) for i in items])
        lens = np.array(list(ref_lens) + [0], np.int64)
        err = C.create_string_buffer(256)
        self.t = L.postable_emul_build(rules, arr, len(items), lens.ctypes.data, len(ref_lens), err)
        self.error = err.value.decode() if not self.t else None
        self.arrays = []
        for which in range(5) if self.t else ():
            n = L.postable_emul_array(self.t, which, None, -1)
            a = np.zeros(n, np.int64 if which == 4 else np.int32)
            assert L.postable_emul_array(self.t, which, a.ctypes.data, n) == n
            self.arrays.append(a.tolist())

    def lower(self, form, tid, xs):
        xs = np.array(xs, np.int64); out = np.full(len(xs), -7, np.int32)
        self.L.postable_emul_lower(self.t, form, tid, xs.ctypes.data, len(xs), out.ctypes.data)
        return out.tolist()

    def close(self):
        if self.t:
            self.L.postable_emul_free(self.t)
        self.t = None


# ---- the designed tables: (name, reference lengths, (tid, positions) runs in file order) ----
LONG = [1, 65535, 65536, 65537, 131072, 131072, 200000]   # both sides of the first edge, on the second, a repeated position, one behind the reference's end
TABLES = [
    ("all", [140000, 100000, 70000, 10], [(0, LONG), (2, [2, 65536, 65536, 69999, 70000]), (3, [3, 3, 10, 11])]),           # (reference 1 has no items)
    ("file order is not reference order", [140000, 100000, 70000, 10], [(3, [10]), (0, LONG), (2, [65535, 65537])]),
    ("edges only", [140000, 70000], [(0, [65536, 131072]), (1, [65536])]),
    ("first reference empty", [10, 140000], [(1, LONG)]),
    ("one item", [140000, 70000, 10], [(1, [65536])]),
    ("one item at 1", [10], [(0, [1])]),
    ("empty", [140000, 70000, 10], []),
    ("empty without references", [], []),
]


def rows(runs, rules):
    """the runs as items of a rule set: a site is one position; a window reaches ten bases further"""
    return [item(t, p, p if rules == SITES else p + 10) for t, ps in runs for p in ps]


def model(ref_lens, runs):
    """tid_first, tid_last, bucket, tid_bucket0 as the library lays them out, from bisect_left alone"""
    n_ref = len(ref_lens); tf, tl = [0] * max(n_ref, 1), [0] * max(n_ref, 1)
    i = 0; per = {}
    for t, ps in runs:
        tf[t], tl[t] = i, i + len(ps); per[t] = ps; i += len(ps)
    bucket, tb0 = [], []
    for t in range(n_ref):
        tb0.append(len(bucket))
        if t in per:
            nb = (max(ref_lens[t], per[t][-1]) >> SHIFT) + 2
            bucket += [tf[t] + bisect_left(per[t], b << SHIFT) for b in range(nb)]
    tb0.append(len(bucket))
    return tf, tl, bucket or [0], tb0, per


def queries(ref_len, ps):
    far = max([ref_len] + ps)
    xs = {-(1 << 31), -5, 0, 1, 2, ref_len - 1, ref_len, ref_len + 1, (1 << 31) - 1}
    xs |= {p + d for p in ps for d in (-1, 0, 1)}
    xs |= {k * BUCKET + d for k in range((far >> SHIFT) + 4) for d in (-1, 0, 1)}        # (the table's last bucket starts at ((far >> SHIFT) + 1) * BUCKET)
    return sorted(xs)


WIDE = [-(1 << 62), -(1 << 40), -(1 << 31) - 1, 1 << 31, (1 << 31) + 65536, 1 << 40, (1 << 62) + 1]   # the binary-search form takes a 64-bit x


def case_lookups(ref_lens, runs):
    """[(form, tid, x, expected)] of a table: the scan form is asked as its callers ask it, with x >= 0"""
    tf, _, _, _, per = model(ref_lens, runs)
    out = []
    for t, n in enumerate(ref_lens):
        ps = per.get(t, [])
        for x in queries(n, ps):
            if x >= 0:
                out.append((0, t, x, tf[t] + bisect_left(ps, x)))
            out.append((1, t, x, tf[t] + bisect_left(ps, x)))
        out += [(1, t, x, tf[t] + bisect_left(ps, x)) for x in WIDE]
    return out


@pytest.mark.parametrize("name,ref_lens,runs", TABLES, ids=[t[0] for t in TABLES])
@pytest.mark.parametrize("rules", [SITES, WINDOWS], ids=["sites", "windows"])
def test_builder_and_lookups_equal_bisect_left(lib, rules, name, ref_lens, runs):
    T = Table(lib, rules, rows(runs, rules), ref_lens)
    try:
        assert T.error is None, T.error
        tf, tl, bucket, tb0, _ = model(ref_lens, runs)
        assert T.arrays == [[p for _, ps in runs for p in ps], tf, tl, bucket, tb0]
        want = case_lookups(ref_lens, runs)
        for form in (0, 1):
            for t in range(len(ref_lens)):
                q = [(x, e) for f, tt, x, e in want if f == form and tt == t]
                got = T.lower(form, t, [x for x, _ in q])
                assert got == [e for _, e in q], (name, form, t, [(x, g, e) for (x, e), g in zip(q, got) if g != e][:5])
        assert len(want) >= 40 * len(ref_lens)
    finally:
        T.close()


def test_the_queries_reach_what_they_are_designed_for():
    ref_lens, runs = TABLES[0][1], TABLES[0][2]
    xs = queries(ref_lens[0], runs[0][1])
    for x in (65534, 65535, 65536, 65537, 65538, 131071, 131073, 139999, 140001, 199999, 200001, 4 * BUCKET - 1, 5 * BUCKET + 1, 6 * BUCKET):   # (buckets 0 .. 4 exist: 200 000 >> 16 = 3)
        assert x in xs
    assert model(ref_lens, runs)[3] == [0, 5, 5, 8, 10]     # tid_bucket0: 5 buckets, none for the empty reference, 3 and 2


# ---- the first error is the one each caller reported ----
def bad_item(rules, tid, start):
    return item(tid, start, start + 1) if rules == SITES else item(tid, start, start - 1)


def error_cases(rules):
    ok = lambda tid, start: item(tid, start, start if rules == SITES else start + 10)
    bad_tid = NOUN[rules] + " with invalid reference id"
    cases = [
        ("an invalid reference id behind an unsorted pair", [ok(0, 100), ok(0, 50), ok(9, 1)], UNSORTED[rules]),
        ("an unsorted pair behind an invalid reference id", [ok(0, 100), ok(-1, 1), ok(0, 50)], bad_tid),
        ("an unsorted pair behind an item that fails its own check", [ok(0, 100), bad_item(rules, 0, 200), ok(0, 300), ok(0, 250)], OWN[rules]),
        ("an item that is out of order and fails its own check", [ok(0, 100), bad_item(rules, 0, 50)], OWN[rules]),
        ("an item of an invalid reference that fails its own check", [ok(0, 100), bad_item(rules, 3, 50)], bad_tid),
        ("a reference that comes back after another", [ok(0, 10), ok(1, 10), ok(0, 200)], SPLIT[rules]),
        ("a reference that comes back out of order", [ok(0, 100), ok(1, 10), ok(0, 50)], SPLIT[rules]),
        ("an unsorted pair behind a reference that comes back", [ok(0, 10), ok(1, 10), ok(0, 200), ok(0, 150)], SPLIT[rules]),
        ("a position of zero", [item(0, 0, 0 if rules == SITES else 5)], OWN[rules]),
        ("any item of a file without references", [ok(0, 1)], bad_tid),
    ]
    if rules == WINDOWS:
        cases += [
            ("an allele without its bases, out of order", [ok(0, 100), item(0, 50, 60, 1, 3, 0, 0)], "invalid window allele"),
            ("a range and an allele that both fail", [item(0, 50, 40, 7, 3, 0, 0)], "invalid window range"),
            ("a deletion without its reference slice, out of order", [ok(0, 100), item(0, 50, 60, 2, 3, 1, 0)], "a deletion window needs its reference slice"),
            ("a deletion with everything, out of order", [ok(0, 100), item(0, 50, 60, 2, 3, 1, 1)], UNSORTED[rules]),
        ]
    if rules == REGIONS:
        cases += [("regions that touch", [item(0, 100, 200), item(0, 200, 300)], MERGED), ("a region inside the one in front", [item(0, 100, 200), item(0, 150, 160)], MERGED)]
    return cases


def accepted_cases(rules):
    """what the order rules let pass: equal positions for sites and windows (and windows that overlap), neighbours for regions"""
    if rules == REGIONS:
        return [[item(0, 100, 200), item(0, 201, 300), item(2, 1, 1)]]
    return [[item(0, 100, 100 if rules == SITES else 150), item(0, 100, 100 if rules == SITES else 120), item(2, 5, 5)]]


REFS3 = [140000, 70000, 10]


@pytest.mark.parametrize("rules", [SITES, WINDOWS, REGIONS], ids=["sites", "windows", "regions"])
def test_first_error_is_the_callers(lib, rules):
    for label, items, message in error_cases(rules):
        T = Table(lib, rules, items, [] if "without references" in label else REFS3)
        assert T.error == message, (NOUN[rules], label, T.error); T.close()
    for items in accepted_cases(rules):
        T = Table(lib, rules, items, REFS3)
        assert T.error is None and T.arrays[1] == [0, 0, 2] and T.arrays[2] == [2, 0, 3], (T.error, T.arrays); T.close()
    assert "Merged and sorted" in UNSORTED[REGIONS] and "Merged and sorted" in SPLIT[REGIONS]   # (what ngsqc_region_read_counts looks for)


# ---- the same cases in a program of their own under the sanitizers ----
def case_text(rules, items, ref_lens, lookups):
    nums = [rules, len(ref_lens), *ref_lens, len(items)] + [v for i in items for v in i] + [len(lookups)] + [v for f, t, x, _ in lookups for v in (f, t, x)]
    return " ".join(map(str, nums)) + "\n"


def test_stand_alone_under_sanitizers(tmp_path):
    exe = emul_build.program("postable_emul_main.cpp", tmp_path, sanitize=True)

    def run(rules, items, ref_lens, lookups):
        p = tmp_path / "case.txt"; p.write_text(case_text(rules, items, ref_lens, lookups))
        r = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.rstrip("\n").split("\n")

    for name, ref_lens, runs in TABLES:
        for rules in (SITES, WINDOWS):
            want = case_lookups(ref_lens, runs)
            tf, tl, bucket, tb0, _ = model(ref_lens, runs)
            arrays = [[p for _, ps in runs for p in ps], tf, tl, bucket, tb0]
            lines = [("array %d: " % k + " ".join(map(str, a))).rstrip() for k, a in enumerate(arrays)] + [str(e) for _, _, _, e in want]
            assert run(rules, rows(runs, rules), ref_lens, want) == lines, (name, rules)
    for rules in (SITES, WINDOWS, REGIONS):
        for label, items, message in error_cases(rules):
            assert run(rules, items, [] if "without references" in label else REFS3, []) == ["error " + message], (NOUN[rules], label)
