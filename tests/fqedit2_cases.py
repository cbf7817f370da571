"""Designed inputs for FastqExtractBarcode, FastqAddBarcode, FastqDownsample and FastqConcat on the device (csrc/fqedit_visit.h, csrc/fqedit.hip): small cases,
each built for one edge of a tool's arithmetic or of the feed (a file list, sides of unequal length), each asserting its own premise when the catalogue is
built. The model (tests/fqedit2_oracle.py) says what comes out; tests/test_cpu_fqedit2_emul.py holds the CPU build of the device text to it,
tests/test_gpu_fqedit2_designed.py the library."""
import random

import fqedit2_oracle as M2
from fqedit_cases import bases, entry, quals

CHUNK = 3968   # the downsample chunk of include/ngsqc.h (capi.DOWNSAMPLE_CHUNK): the ordinals one device lane of the generator walks
OPS = {"barcode_cut": 4, "barcode_add": 5, "downsample": 6, "copy": 7}
SIDES = {"barcode_cut": 1, "barcode_add": 3, "downsample": 2, "copy": 1}
STREAMS = {"barcode_cut": 2, "barcode_add": 2, "downsample": 2, "copy": 1}


def text(entries):
    return b"".join(l + b"\n" for _, e in entries for l in e)


class Case:
    """files: [one text per side of the op]: every element is one input file (or pair, or triple) that ends with `last`; kw: the library's parameters"""

    def __init__(self, name, op, kw, files):
        self.name, self.op, self.kw, self.files = name, op, kw, [tuple(f) for f in files]
        assert all(len(f) == SIDES[op] for f in self.files)

    def model(self, mutate=None):
        if self.op == "barcode_cut":
            return M2.barcode_cut(self.files[0][0], self.kw["cut1"], mutate=mutate)
        if self.op == "barcode_add":
            return M2.barcode_add(self.files, mutate=mutate)
        if self.op == "downsample":
            return M2.downsample(self.files[0][0], self.files[0][1], self.kw["seed"], self.kw["percentage"], mutate=mutate)
        return M2.concat([f[0] for f in self.files])

    def lib_kw(self):
        return dict(op=self.op, **self.kw)


def _cut_cases(rng):
    ln = 12
    es = [entry(rng, "full", ln), entry(rng, "q-short", ln, 5), entry(rng, "b-empty", 0, 3), entry(rng, "b-short-q-long", 4, ln), entry(rng, "both-empty", 0, 0)]
    out = []
    for tag, cut in (("0", 0), ("1", 1), ("len-1", ln - 1), ("len", ln), ("len+1", ln + 1)):
        c = Case("cut-" + tag, "barcode_cut", dict(cut1=cut), [(text(es),)])
        p = c.model().plan
        assert p[0, 0, 3:5].tolist() == [min(cut, ln), max(ln - cut, 0)] and p[0, 1, 3:5].tolist() == [0, min(cut, ln)]          # the full entry: main and index
        assert p[1, 0, 5:7].tolist() == [min(cut, 5), max(5 - cut, 0)] and p[1, 1, 6] == min(cut, 5)                             # the quality line is cut on its own
        assert p[2, 0, 3:5].tolist() == [0, 0] and p[2, 1, 4] == 0 and p[2, 1, 6] == min(cut, 3)                                 # no bases at all
        assert (p[:, :, 4] + 0 <= [[len(e[1])] * 2 for _, e in es]).all() and (p[:, 0, 4] + p[:, 1, 4] == [len(e[1]) for _, e in es]).all()   # main + index = the line
        out.append(c)
    assert out[4].model().plan[1, 1, 6] == 5 and out[4].model().plan[1, 0, 6] == 0   # a cut beyond a quality line shorter than its bases: the bytes there are
    return out


def _barcode(rng, name, n):
    return entry(rng, name, n, header=b"@bc " + name.encode())


def _add_cases(rng):
    out = []
    headers = {"no-space": b"@r1", "leading-space": b" @r2 x", "two-spaces": b"@r3  1:N:0 tail", "at-alone": b"@"}
    e1 = [(k, (h, bases(rng, 20), b"+", quals(rng, 20))) for k, h in headers.items()]
    e2 = [(k, (h + b"/2" if k != "at-alone" else h, bases(rng, 15), b"+x", quals(rng, 15))) for k, h in headers.items()]
    e3 = [_barcode(rng, k, 8) for k in headers]
    c = Case("add-headers", "barcode_add", {}, [(text(e1), text(e2), text(e3))])
    r = c.model()
    assert r.plan[:, 0, 1].tolist() == [3, 0, 3, 1] and r.plan[:, 1, 1].tolist() == [5, 0, 3, 1] and set(r.plan[:, :, 2].ravel().tolist()) == {5 + 1 + 8}
    assert r.out[0].split(b"\n")[4].startswith(b":8,0:") and r.out[0].split(b"\n")[12].startswith(b"@:8,0:") and r.out[0].split(b"\n")[8].startswith(b"@r3:8,0:")
    out.append(c)
    # ---- the digit-count borders of the barcode length
    lens = (0, 9, 10, 99, 100)
    e1 = [entry(rng, "d%d" % n, 10, header=b"@d%d 1" % n) for n in lens]
    e2 = [entry(rng, "d%d" % n, 11, header=b"@d%d 2" % n) for n in lens]
    c = Case("add-digits", "barcode_add", {}, [(text(e1), text(e2), text([_barcode(rng, "b%d" % n, n) for n in lens]))])
    assert c.model().plan[:, 0, 2].tolist() == [5 + 1 + 0, 5 + 1 + 9, 5 + 2 + 10, 5 + 2 + 99, 5 + 3 + 100]
    assert c.model().out[1].split(b"\n")[0] == b"@d0:0,0:, 2"
    out.append(c)
    # ---- sides of unequal entry count: the triple ends silently at its shortest file
    many = [entry(rng, "u%d" % i, 9, header=b"@u%d c" % i) for i in range(8)]
    bcs = [_barcode(rng, "b%d" % i, 6 + i) for i in range(8)]
    for name, a, b, c3, n in (("add-barcode-shortest", many[:5], many[:6], bcs[:3], 3), ("add-barcode-longest", many[:4], many[:5], bcs[:8], 4), ("add-barcode-one-more", many[:5], many[:5], bcs[:6], 5)):
        c = Case(name, "barcode_add", {}, [(text(a), text(b), text(c3))])
        assert len(c.model().plan) == n and min(len(a), len(b), len(c3)) == n
        out.append(c)
    # ---- lists of files: the second triple starts afresh behind a first one whose files differ in length
    c = Case("add-two-files", "barcode_add", {}, [(text(many[:3]), text(many[:5]), text(bcs[:4])), (text(many[5:]), text(many[5:]), text(bcs[5:]))])
    r = c.model()
    assert len(r.plan) == 3 + 3 and r.out[0].split(b"\n")[12].startswith(b"@u5:11,0:")
    out.append(c)
    return out


def pairs_text(n, extra1=0, extra2=0):
    """n pairs of reads of a few bases, and extra entries behind them on one side"""
    t = [b"".join(b"@p%d/%d\n%s\n+\n%s\n" % (i, k, (b"ACGT", b"TG")[k - 1], (b"IIII", b"HH")[k - 1]) for i in range(m)) for k, m in ((1, n + extra1), (2, n + extra2))]
    return t[0], t[1]


def _downsample_cases():
    out = []
    for n, seed, p in ((1, 1, 20.0), (CHUNK - 1, 1, 20.0), (CHUNK, 12345, 20.0), (CHUNK + 1, 1, 33.3), (2 * CHUNK + 1, 1, 20.0), (2 * CHUNK + 1, 12345, 20.0), (60, 1, 0.001), (60, 12345, 99.999), (60, 12345, 50.0)):
        c = Case("downsample-%d-seed%d-%g" % (n, seed, p), "downsample", dict(seed=seed, percentage=p), [pairs_text(n)])
        r = c.model()
        kept = r.stats["written"][0]
        assert r.stats["entries"] == n and r.side_entries == [n, n] and r.kept_headers.count(b"\n") == kept
        if n > 1 and 1 < p < 99:
            assert 0 < kept < n and abs(kept - n * p / 100) < 5 * (n * p / 100) ** 0.5
        if p < 1:
            assert kept == 0
        if p > 99:
            assert kept == n
        out.append(c)
    for name, x1, x2 in (("downsample-in2-longer", 0, 1), ("downsample-in1-longer", 1, 0)):
        c = Case(name, "downsample", dict(seed=1, percentage=20.0), [pairs_text(30, x1, x2)])
        assert c.model().stats["entries"] == 30 and c.model().side_entries == [30 + x1, 30 + x2] and 0 < c.model().stats["written"][0] < 30
        out.append(c)
    return out


def _copy_cases(rng):
    A = text([entry(rng, "a%d" % i, 10 + i) for i in range(3)])
    B = text([entry(rng, "b%d" % i, 7) for i in range(2)])
    Cc = text([entry(rng, "c%d" % i, 5, header=b"@c%d x y" % i) for i in range(4)])
    out = []
    c = Case("copy-first-lacks-final-newline", "copy", {}, [(A[:-1],), (B,), (Cc,)])
    assert not c.files[0][0].endswith(b"\n") and c.model().out[0] == A + B + Cc
    out.append(c)
    c = Case("copy-crlf", "copy", {}, [(A.replace(b"\n", b"\r\n"),)])
    assert c.files[0][0].count(b"\r\n") == 12 and c.model().out[0] == A
    out.append(c)
    c = Case("copy-empty-file", "copy", {}, [(b"",)])
    assert c.model().out[0] == b"" and c.model().stats["entries"] == 0
    out.append(c)
    c = Case("copy-only-blank-lines", "copy", {}, [(b"\n\r\n\n",)])
    assert c.model().out[0] == b"" and c.model().stats["entries"] == 0
    out.append(c)
    c = Case("copy-middle-file-incomplete", "copy", {}, [(A,), (B + b"@x\nACG\n",), (Cc,)])
    assert c.model().out[0] == A + B + b"@x\nACG\n\n\n" + Cc and c.model().stats["entries"] == 3 + 3 + 4   # §14: the missing lines read as empty
    out.append(c)
    c = Case("copy-mixed", "copy", {}, [(A[:-1],), (b"",), (b"\n\n",), (B.replace(b"\n", b"\r\n") + b"\r\n\r\n",), (Cc,)])
    assert c.model().out[0] == A + B + Cc
    out.append(c)
    return out


_catalogue = None


def catalogue():
    global _catalogue
    if _catalogue is None:
        rng = random.Random(20250307)
        _catalogue = _cut_cases(rng) + _add_cases(rng) + _downsample_cases() + _copy_cases(rng)
        assert len({c.name for c in _catalogue}) == len(_catalogue)
    return _catalogue


def by_name(name):
    return [c for c in catalogue() if c.name == name][0]
