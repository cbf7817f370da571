"""Designed FASTQ entries for the per-entry FASTQ tools (csrc/fqedit_visit.h, csrc/fqedit.hip): small groups of entries, each built for one edge of a tool's
arithmetic, each asserting its own premise when the catalogue is built ("this entry's bases are exactly start + end long"). The model (tests/fqedit_oracle.py)
says what comes out; tests/test_cpu_fqedit_emul.py holds the CPU build of the device text to it, tests/test_gpu_fqedit_designed.py the library."""
import random

import fqedit_oracle as M


class Group:
    """entries: [(name, (header, bases, header2, qualities))]; entries2: the second file of the paired tool; ids: (names, lengths) for extract"""

    def __init__(self, name, op, kw, entries, entries2=None, ids=None):
        self.name, self.op, self.kw, self.entries, self.entries2, self.ids = name, op, kw, entries, entries2, ids

    @staticmethod
    def _text(entries, crlf, final_newline):
        nl = b"\r\n" if crlf else b"\n"
        t = b"".join(l + nl for _, e in entries for l in e)
        return t if final_newline or not t else t[:-len(nl)]

    def texts(self, crlf=False, final_newline=True):
        return self._text(self.entries, crlf, final_newline), (None if self.entries2 is None else self._text(self.entries2, crlf, final_newline))

    def model(self):
        t1, t2 = self.texts()
        return M.run(self.op, t1, t2, ids=self.ids, **self.kw)

    def lib_kw(self):
        return dict(op=self.op, **self.kw)


def bases(rng, n):
    return bytes(rng.choice(b"ACGTN") for _ in range(n))


def quals(rng, n, lo=33, hi=74):
    return bytes(rng.randint(lo, hi) for _ in range(n))


def entry(rng, name, bl, ql=None, header=None, header2=b"+"):
    h = b"@" + name.encode() if header is None else header
    return name, (h, bases(rng, bl), header2, quals(rng, bl if ql is None else ql))


def _trim_groups(rng):
    out = []
    # ---- start + end, len and max_len around every threshold
    start, end, ln, max_len = 3, 4, 16, 65
    lens = {"empty": 0, "one": 1, "sum-1": start + end - 1, "sum": start + end, "sum+1": start + end + 1, "len-1": start + end + ln - 1, "len": start + end + ln,
            "len+1": start + end + ln + 1, "max_len-1": max_len - 1, "max_len": max_len, "max_len+1": max_len + 1}
    g = Group("trim-thresholds", "trim", dict(start=start, end=end, len=ln, max_len=max_len), [entry(rng, k, v) for k, v in lens.items()])
    r = g.model().plan
    by = dict(zip(lens, r.tolist()))
    assert by["empty"][0] == 0 and by["one"][0] == 0 and by["sum-1"][0] == 0 and by["sum"][0] == 0   # dropped: bases <= start + end
    assert by["sum+1"] == [1, 0, 0, start, 1, start, 1, 0]
    assert by["len-1"][4] == ln - 1 and by["len"][4] == ln and by["len+1"][4] == ln and by["len+1"][6] == ln
    assert by["max_len-1"][3:5] == [start, ln]                                                        # below max_len: trimmed, then cut to len
    assert by["max_len"] == [1, 0, 0, 0, max_len, 0, max_len, 0] and by["max_len+1"][4] == max_len + 1   # at and above: unchanged
    out.append(g)
    # ---- kept ranges of 15 / 16 / 17 and 63 / 64 / 65 bytes behind an odd start, and whole lines of those sizes
    sizes = (15, 16, 17, 63, 64, 65)
    g = Group("trim-kept-sizes", "trim", dict(start=5), [entry(rng, "kept%d" % s, s + 5) for s in sizes])
    assert g.model().plan[:, 4].tolist() == list(sizes) and g.model().plan[:, 3].tolist() == [5] * 6
    out.append(g)
    g = Group("trim-whole-sizes", "trim", dict(len=64), [entry(rng, "whole%d" % s, s) for s in sizes] + [entry(rng, "h" * (s - 1), 20) for s in sizes])
    assert g.model().plan[:6, 4].tolist() == [15, 16, 17, 63, 64, 64] and [len(e[0]) for _, e in g.entries[6:]] == list(sizes)
    out.append(g)
    g = Group("trim-end-only", "trim", dict(end=5), [entry(rng, "e%d" % s, s) for s in (4, 5, 6, 20)])
    assert g.model().plan[:, 0].tolist() == [0, 0, 1, 1] and g.model().plan[2].tolist() == [1, 0, 0, 0, 1, 0, 1, 0]
    out.append(g)
    # ---- bases and qualities of different lengths, both ways (FastqTrim does not validate)
    g = Group("trim-lines-differ", "trim", dict(start=10, end=10, len=8),
              [entry(rng, "q-behind-start", 30, 5), entry(rng, "q-inside", 30, 15), entry(rng, "q-longer", 30, 40), entry(rng, "b-short-q-long", 20, 40), entry(rng, "q-empty", 30, 0)])
    r = g.model().plan.tolist()
    assert r[0][5:7] == [5, 0] and r[1][5:7] == [10, 5] and r[2][3:7] == [10, 8, 10, 8] and r[3][0] == 0 and r[4][5:7] == [0, 0]
    out.append(g)
    # -len alone: the reference's resize() would lengthen a shorter quality line with unspecified bytes; here no line grows
    g = Group("trim-len-lines-differ", "trim", dict(len=64), [entry(rng, "q-shorter", 70, 60), entry(rng, "q-longer", 70, 80), entry(rng, "b-at-len-q-longer", 64, 80), entry(rng, "b-empty", 0, 9)])
    r = g.model().plan.tolist()
    assert r[0][4] == 64 and r[0][6] == 60 and r[1][6] == 64 and r[2][4:7:2] == [64, 80] and r[3][4:7:2] == [0, 9]
    out.append(g)
    return out


def _convert_groups(rng):
    q = bytes([31, 41, 64, 255, 32, 33, 126, 127, 128, 0x0b])   # 31 -> 0, 41 -> a line feed, 64 -> 33, 255 -> 224, 0x0b + 256 - 31
    es = [("designed-qualities", (b"@c0", bases(rng, len(q)), b"+", q)), entry(rng, "plain", 40, None), entry(rng, "q-longer", 3, 17), entry(rng, "q-shorter", 17, 3),
          ("phred64", (b"@c4 x", bases(rng, 65), b"+c4", quals(rng, 65, 64, 104)))]
    g = Group("convert", "convert", dict(), es)
    out = g.model().out[0]
    assert out.split(b"\n")[3] == b"\x00" and out.split(b"\n")[4][:3] == bytes([33, 224, 1])   # the line feed made from ')' cuts the line in two
    assert b"\n" not in q and b"\r" not in q
    return [g]


def _umi_groups(rng):
    out = []
    headers = {"no-space": b"@r1", "leading-space": b" @r2 x", "several-spaces": b"@r3 1:N:0  tail end", "trailing-space": b"@r4 ", "empty": b"", "only-space": b" "}
    e1 = [(k, (h, bases(rng, 30), b"+", quals(rng, 30))) for k, h in headers.items()]
    e2 = [(k, (h, bases(rng, 25), b"+x", quals(rng, 25))) for k, h in headers.items()]
    g = Group("umi-headers", "umi", dict(cut1=12, cut2=0), e1, e2)
    r = g.model()
    assert r.plan[:, 0, 1].tolist() == [3, 0, 3, 3, 0, 0] and set(r.plan[:, :, 2].ravel().tolist()) == {len(b":12,0:") + 12 + 1}
    assert r.out[0].split(b"\n")[4].startswith(b":12,0:") and r.out[1].split(b"\n")[0].endswith(b",")
    out.append(g)
    # ---- cut 0, equal to the read, beyond it; lines of different lengths; three digits
    e1 = [entry(rng, "a", 8), entry(rng, "b", 9), entry(rng, "c", 3), entry(rng, "d", 0), entry(rng, "e", 20, 4), entry(rng, "f", 4, 20)]
    e2 = [entry(rng, "a", 20), entry(rng, "b", 100), entry(rng, "c", 101), entry(rng, "d", 99), entry(rng, "e", 0), entry(rng, "f", 150, 120)]
    g = Group("umi-cuts", "umi", dict(cut1=8, cut2=100), e1, e2)
    r = g.model().plan
    assert r[0, 0, 3:5].tolist() == [8, 0] and r[1, 0, 3:5].tolist() == [8, 1] and r[2, 0, 3:5].tolist() == [3, 0] and r[3, 0, 3:5].tolist() == [0, 0]   # cut = the read, below it, beyond it, no read
    assert r[1, 1, 3:5].tolist() == [100, 0] and r[2, 1, 3:5].tolist() == [100, 1] and r[3, 1, 3:5].tolist() == [99, 0] and r[4, 0, 5:7].tolist() == [4, 0]
    assert r[0, 0, 2] == len(b":8,100:") + 8 + 1 + 20 and r[2, 0, 2] == len(b":8,100:") + 3 + 1 + 100   # the UMI of a short read: the bases there are
    out.append(g)
    g = Group("umi-cut-zero", "umi", dict(cut1=0, cut2=0), [entry(rng, "z%d" % i, 10 + i) for i in range(3)], [entry(rng, "z%d" % i, 12) for i in range(3)])
    assert set(g.model().plan[:, :, 2].ravel().tolist()) == {len(b":0,0:,")}
    out.append(g)
    # ---- an insertion that moves a header across 15 / 16 / 17 and 63 / 64 / 65 bytes: ":8,8:" + 8 + "," + 8 = 22 bytes
    ins = len(b":8,8:") + 17
    hl = [s - ins for s in (15, 16, 17, 63, 64, 65) if s > ins] + [15, 16, 17, 63, 64, 65]
    e1 = [("h%d" % n, ((b"@" + b"x" * (n // 2 - 1) + b" " + b"y" * (n - n // 2 - 1))[:n], bases(rng, 40), b"+", quals(rng, 40))) for n in hl]
    e2 = [("h%d" % n, (b"@" + b"w" * (n - 1), bases(rng, 40), b"+", quals(rng, 40))) for n in hl]
    g = Group("umi-header-sizes", "umi", dict(cut1=8, cut2=8), e1, e2)
    assert [len(e[0]) for _, e in e1] == hl and [len(e[0]) for _, e in e2] == hl
    for k in (0, 1):
        assert [len(l) for l in g.model().out[k].split(b"\n")[0:12:4]] == [63, 64, 65]
    out.append(g)
    # ---- inputs of unequal entry count: the run ends silently at the shorter file
    many = [entry(rng, "u%d" % i, 12) for i in range(7)]
    for name, a, b in (("umi-in1-longer", many, many[:4]), ("umi-in2-longer", many[:2], many), ("umi-in2-empty", many[:3], [])):
        g = Group(name, "umi", dict(cut1=2, cut2=3), a, b)
        assert len(g.model().plan) == min(len(a), len(b))
        out.append(g)
    return out


def _extract_groups(rng):
    out = []
    names = ["read", "read2", "rea", "read/1", "other", "dup", "minus1", "minus2", "zero", "one", "exact", "above", "below-3", "absent", "tabbed"]
    es = [entry(rng, n, 12, header=("@" + n + " 1:N:0 " + n).encode()) for n in names[:-1]]
    es.append(entry(rng, "tabbed", 12, header=b"@tabbed\t"))                                         # trimmed() takes the tab off before the id is cut
    es.append(entry(rng, "space-first", 12, header=b"@ read"))                                     # the id is empty
    es.append(entry(rng, "no-header", 12, header=b""))                                             # not validated, the id is empty
    es.append(("no-header-odd", (b"", b"acgt", b"", b"\x01")))                                     # ... whatever its lines hold
    es.append(entry(rng, "id-with-comment", 12, header=b"@comment x"))
    ids = ([b"read", b"rea", b"read/1", b"dup", b"dup", b"dup", b"minus1", b"minus2", b"zero", b"one", b"exact", b"above", b"below-3", b"missing", b"tabbed", b"comment x", b"read 1:N:0 read"],
           [None, 5, 7, 3, 9, 4, -1, -2, 0, 1, 12, 13, -3, 6, 2, 3, 3])
    for invert in (False, True):
        g = Group("extract" + ("-v" if invert else ""), "extract", dict(invert=invert), es, ids=ids)
        r = g.model()
        assert r.error is None
        by = dict(zip([n for n, _ in es], r.plan.tolist()))
        if not invert:
            assert by["read"][0] == 1 and by["read"][4] == 12          # listed without a length
            assert by["read2"][0] == 0                                  # "read" is a prefix of it: not listed
            assert by["rea"][4] == 5 and by["read/1"][4] == 7           # a prefix of a listed id, listed itself
            assert by["dup"][4] == 4                                    # the last of three lengths
            assert by["minus1"] == by["read"][:1] + by["minus1"][1:] and by["minus1"][4] == 12   # -1: no length
            assert by["minus2"][0] == 0 and by["zero"][0] == 0 and by["below-3"][0] == 0
            assert by["one"][4] == 1 and by["exact"][4] == 12 and by["above"][4] == 12 and by["above"][0] == 1   # a length beyond the read keeps the whole read
            assert by["tabbed"][4] == 2 and by["space-first"][0] == 0 and by["no-header"][0] == 0 and by["id-with-comment"][0] == 0
        else:
            assert [by[n][0] for n in ("read", "read2", "minus1", "minus2", "zero", "below-3", "absent", "space-first", "no-header", "no-header-odd")] == [0, 1, 0, 1, 0, 0, 1, 1, 1, 1]
        out.append(g)
    # ---- many ids and many entries: more than one workgroup, every probe colliding under NGSQC_NAME_HASH_BITS=4; long reads: qualities up to 126
    n = 700
    es = [entry(rng, "r%d" % i, 5 + i % 90, header=("@r%d c" % i).encode()) for i in range(n)]
    ids = ([b"r%d" % i for i in range(0, n, 3)] + [b"q%d" % i for i in range(100)], [None if i % 2 else 1 + i % 70 for i in range(0, n, 3)] + [4] * 100)
    for invert in (False, True):
        g = Group("extract-many" + ("-v" if invert else ""), "extract", dict(invert=invert), es, ids=ids)
        assert int(g.model().plan[:, 0].sum()) == (len(range(0, n, 3)) if not invert else n - len(range(0, n, 3)))
        out.append(g)
    es = [("long%d" % i, (b"@long%d x" % i, bases(rng, bl), b"+", quals(rng, bl, 33, 126))) for i, bl in enumerate((0, 1, 63, 64, 65, 129, 1000))]
    g = Group("extract-long-read", "extract", dict(long_read=True), es, ids=([b"long%d" % i for i in range(7)], [None, 5, 63, 64, 64, 200, 999]))
    assert g.model().error is None and g.model().plan[:, 4].tolist() == [0, 1, 63, 64, 64, 129, 999]
    out.append(g)
    return out


_catalogue = None


def catalogue():
    global _catalogue
    if _catalogue is None:
        rng = random.Random(20240611)
        _catalogue = _trim_groups(rng) + _convert_groups(rng) + _umi_groups(rng) + _extract_groups(rng)
        assert len({g.name for g in _catalogue}) == len(_catalogue)
    return _catalogue


def by_name(name):
    return [g for g in catalogue() if g.name == name][0]


def error_cases():
    """FastqExtract's validation: (name, text, long_read, kind, entry, part of the message). The first failing entry, and within it the first check, wins."""
    rng = random.Random(7)
    ok = lambda n: entry(rng, n, 10)[1]
    t = lambda es: b"".join(l + b"\n" for e in es for l in e)
    return [
        ("no @", t([ok("a"), (b"x", b"AC", b"+", b"II")]), False, 1, 1, "First header line does not start with '@': 'x'."),
        ("no +", t([ok("a"), ok("b"), (b"@c", b"AC", b"", b"II")]), False, 2, 2, "Second header line does not start with '+': ''."),
        ("lengths", t([(b"@c", b"ACG", b"+", b"II")]), False, 3, 0, "Differing length of bases (3) and qualities string (3) in sequence '@c'."),
        ("base", t([ok("a"), (b"@c", b"ACXG", b"+", b"III!")]), False, 4, 1, "Invalid base 'X' encountered in sequence '@c'."),
        ("quality", t([ok("a"), (b"@c", b"ACG", b"+", b"IKL")]), False, 5, 1, "Invalid quality character 'K' with value '75' encountered in sequence '@c'."),
        ("quality long read", t([ok("a"), (b"@c", b"ACG", b"+", b"IK\x7f")]), True, 5, 1, "Invalid nanopore quality character '\x7f' with value '127' encountered in sequence '@c'."),
        ("two entries fail", t([ok("a"), (b"@c", b"ACG", b"+", b"II "), ok("b"), (b"d", b"A", b"+", b"I")]), False, 5, 1, "Invalid quality character ' ' with value '32'"),
        ("incomplete last entry", t([ok("a")]) + b"@c\nACG\n", False, 2, 1, "Second header line does not start with '+': ''."),
    ]


def big(rng=None):
    """about 200 KB of text with one entry of 70 000 bases - longer than a BGZF piece of 0xff00 bytes - between short ones"""
    rng = rng or random.Random(99)
    es = [entry(rng, "s%d" % i, 100, header=("@s%d c" % i).encode()) for i in range(200)]
    es.insert(100, ("big", (b"@big read", bases(rng, 70000), b"+big", quals(rng, 70000, 33, 126))))
    es += [entry(rng, "t%d" % i, 151, header=("@t%d c" % i).encode()) for i in range(60)]
    t = b"".join(l + b"\n" for _, e in es for l in e)
    assert 190_000 < len(t) < 260_000 and 70000 > 0xff00
    return es, t
